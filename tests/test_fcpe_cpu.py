"""FCPE (f0_method="fcpe") without a GPU: the host tail against the reference's, the checkpoint loader, the argument contracts of
the four K15 entries (csrc/fcpe.hip refuses before any device call, so the refusals need no device) and the estimators that stay
unbuilt.  Fixtures: tests/golden/make_golden_fcpe.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def S():
    from rvc_amd.lib import synthetic
    return synthetic


@pytest.fixture(scope="module")
def F():
    from rvc_amd.lib.predictors import FCPE
    return FCPE


# ---- host tail ------------------------------------------------------------------------------------------------------------------
def test_host_tail_is_bit_equal_to_the_reference(F):
    """_resize_f0 -> _interpolate_f0 (fcpe.py:30-77) over every recorded voiced / unvoiced pattern, bit for bit."""
    g = load_golden("fcpe_tail")
    so = do = 0
    assert int(g["n_cases"]) >= 35
    for n, tl in zip(g["src_len"], g["target_len"]):
        src, want = g["src"][so: so + n], g["out"][do: do + tl]
        so, do = so + n, do + tl
        got = F.interpolate_f0(F.resize_f0(src, int(tl)))
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (n, tl, src, got, want)
    assert so == len(g["src"]) and do == len(g["out"])


def test_host_tail_long_unvoiced_contour_is_linear_time(F):
    """3201 masked frames (the default filter_radius = 3 on a 30 s clip) come back as zeros; the reference's loop rescans the tail
    from every frame."""
    out = F.interpolate_f0(F.resize_f0(np.zeros(3201, dtype=np.float32), 3200))
    assert out.shape == (3200,) and not out.any()


# ---- loader ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,layers", [(512, 6), (128, 2)])
def test_synthetic_checkpoint_has_the_reference_state_dict(S, hidden, layers):
    g = load_golden("fcpe_keys")
    ck = S.make_fcpe_checkpoint(0, hidden=hidden, layers=layers)
    want = dict(zip(g[f"names_{hidden}x{layers}"].tolist(), g[f"shapes_{hidden}x{layers}"].tolist()))
    got = {k: ",".join(str(d) for d in v.shape) for k, v in ck["model"].items()}
    assert got == want
    m = ck["config_dict"]["model"]
    assert (m["hidden_dims"], m["n_layers"], m["conv_only"], m["out_dims"]) == (hidden, layers, True, 360)


def test_loader_folds_both_weight_norm_spellings_and_pads(S, F):
    ck = S.make_fcpe_checkpoint(0, hidden=128, layers=2)
    cfg, w = F.fold_fcpe_checkpoint(ck)
    assert cfg["model"]["conv_dropout"] == 0.0 and cfg["model"]["atten_dropout"] == 0.0
    assert ck["config_dict"]["model"]["conv_dropout"] == 0.1           # the caller's dict is left alone
    sd = dict(ck["model"])
    g_, v_ = sd.pop("output_proj.parametrizations.weight.original0"), sd.pop("output_proj.parametrizations.weight.original1")
    legacy = dict(ck, model=dict(sd, **{"output_proj.weight_g": g_, "output_proj.weight_v": v_}))
    _, w2 = F.fold_fcpe_checkpoint(legacy)
    assert torch.equal(w["proj.w"], w2["proj.w"])
    assert w["proj.w"].shape == (384, 128) and w["proj.b"].shape == (384,)
    assert not w["proj.w"][360:].any() and not w["proj.b"][360:].any()
    want = torch._weight_norm(v_, g_, 0)
    assert torch.allclose(w["proj.w"][:360], want, rtol=1e-6, atol=1e-8)
    assert torch.equal(w["cent_table"], ck["model"]["cent_table"])
    assert w["l1.dw.w"].shape == (256, 31) and w["l1.up.w"].shape == (512, 128) and w["l1.down.w"].shape == (128, 256)


def test_loader_refuses_the_attention_branch(S, F):
    ck = S.make_fcpe_checkpoint(0, hidden=128, layers=2)
    ck["config_dict"]["model"]["conv_only"] = False
    with pytest.raises(NotImplementedError, match="conv_only"):
        F.fold_fcpe_checkpoint(ck)


# ---- ABI contracts ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rvc_amd import _native
    for name in ("rvc_glu_dwconv_silu_f32", "rvc_layernorm_rows_f32", "rvc_groupnorm_workspace_bytes", "rvc_groupnorm_lrelu_f32",
                 "rvc_fcpe_decode_f32"):
        assert name in _native.SYMBOLS
    return _native._lib


@pytest.fixture(scope="module")
def ptr():
    """A non-null, 16-byte aligned host address: every call below must be refused before anything could dereference it."""
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    yield addr
    del buf


def _refused(lib, rc, *words):
    msg = lib.rvc_last_error().decode()
    assert rc != 0 and msg, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_glu_dwconv_silu_contract(lib, ptr):
    f = lib.rvc_glu_dwconv_silu_f32
    _refused(lib, f(ptr, ptr, ptr, ptr, 17, 96, 31, None), "C (96)")
    _refused(lib, f(ptr, ptr, ptr, ptr, 17, 64, 30, None), "K (30)")
    _refused(lib, f(ptr, ptr, ptr, ptr, 17, 64, 33, None), "K (33)")
    _refused(lib, f(ptr, ptr, ptr, ptr, 0, 64, 31, None), "n_rows")
    for null in range(4):
        args = [ptr] * 4
        args[null] = None
        _refused(lib, f(*args, 17, 64, 31, None), "null pointer")


def test_layernorm_rows_contract(lib, ptr):
    f = lib.rvc_layernorm_rows_f32
    _refused(lib, f(ptr, ptr, ptr, 1e-5, ptr, 17, 1088, None), "F (1088)")
    _refused(lib, f(ptr, ptr, ptr, 1e-5, ptr, 17, 100, None), "F (100)")
    _refused(lib, f(ptr, ptr, ptr, 1e-5, ptr, 0, 512, None), "n_rows")
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr), (ptr, ptr, ptr, None)):
        _refused(lib, f(args[0], args[1], args[2], 1e-5, args[3], 17, 512, None), "null pointer")


def test_groupnorm_lrelu_contract(lib, ptr):
    f = lib.rvc_groupnorm_lrelu_f32
    need = ctypes.c_size_t()
    assert lib.rvc_groupnorm_workspace_bytes(512, 2049, 4, ctypes.byref(need)) == 0 and need.value >= 4 * 2 * 24
    _refused(lib, lib.rvc_groupnorm_workspace_bytes(510, 17, 4, ctypes.byref(need)), "groups (4) must divide C (510)")
    _refused(lib, lib.rvc_groupnorm_workspace_bytes(512, 17, 4, None), "null pointer")
    _refused(lib, f(ptr, ptr, ptr, 4, 1e-5, 0.01, ptr, 510, 17, ptr, 1 << 20, None), "groups (4) must divide C (510)")
    assert lib.rvc_groupnorm_workspace_bytes(512, 2049, 4, ctypes.byref(need)) == 0
    _refused(lib, f(ptr, ptr, ptr, 4, 1e-5, 0.01, ptr, 512, 2049, ptr, need.value - 1, None), "workspace")
    _refused(lib, f(ptr, ptr, ptr, 4, 1e-5, 0.01, ptr, 512, 2049, None, need.value, None), "null pointer")
    _refused(lib, f(None, ptr, ptr, 4, 1e-5, 0.01, ptr, 512, 2049, ptr, need.value, None), "null pointer")
    _refused(lib, f(ptr, ptr, ptr, 4, 1e-5, 0.01, None, 512, 2049, ptr, need.value, None), "null pointer")


def test_fcpe_decode_contract(lib, ptr):
    f = lib.rvc_fcpe_decode_f32
    _refused(lib, f(ptr, ptr, 360, 359, 0.006, 32.7, ptr, None, 17, None), "ld (359)")
    _refused(lib, f(ptr, ptr, 360, 384, 0.006, 32.7, ptr, None, 0, None), "n_rows")
    _refused(lib, f(None, ptr, 360, 384, 0.006, 32.7, ptr, None, 17, None), "null pointer")
    _refused(lib, f(ptr, None, 360, 384, 0.006, 32.7, ptr, None, 17, None), "null pointer")
    _refused(lib, f(ptr, ptr, 360, 384, 0.006, 32.7, None, None, 17, None), "null pointer")


# ---- what stays unbuilt ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["crepe", "crepe-tiny", "hybrid[rmvpe+fcpe]"])
def test_other_estimators_still_raise(method):
    from rvc_amd.infer.pipeline import Pipeline
    from rvc_amd.train.extract.extract import FeatureInput
    p = object.__new__(Pipeline)           # get_f0 refuses before it touches the object
    with pytest.raises(NotImplementedError, match="'rmvpe' and 'fcpe'"):
        p.get_f0("path", np.zeros(16000), 100, 0, method, 3, 128, False, 1)
    with pytest.raises(NotImplementedError, match="'rmvpe' and 'fcpe'"):
        FeatureInput(device="cpu").compute_f0(np.zeros(16000), method, 160)


def test_compute_f0_refuses_what_is_not_built(F):
    f = object.__new__(F.FCPE)
    f.sampling_rate, f.model_sr, f.hop_length = 16000, 16000, 160
    wav = np.zeros(16000)
    with pytest.raises(NotImplementedError, match="sr = 44100"):
        f.compute_f0(wav, sr=44100)
    with pytest.raises(NotImplementedError, match="argmax"):
        f.compute_f0(wav, decoder_mode="argmax")
    with pytest.raises(NotImplementedError, match="test_time_augmentation"):
        f.compute_f0(wav, test_time_augmentation=True)
