"""K18 (clean_audio, csrc/spectralgate.hip) without a GPU: every refusal of the C ABI comes before any device access, the Python
surface refuses what is not built by name, the host constants equal the SciPy restatement's (tests/spectral_gate_ref.py), the
restatement itself is an identity at prop_decrease = 0, and VoiceConverter routes clean_audio to remove_audio_noise."""
import ctypes

import numpy as np
import pytest
import torch

import spectral_gate_ref as R


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
GOOD = dict(y=1, n=9000, sr=48000, prop=0.7, chunk=600000, pad=30000, out=1, ws=1, ws_bytes=1 << 40)
REFUSALS = [   # (what changes, the words the error must carry)
    (dict(y=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(n=-1), "negative"),
    (dict(sr=5119), "sr 5119"), (dict(sr=256001), "sr 256001"), (dict(sr=0), "sr 0"), (dict(sr=-48000), "sr -48000"),
    (dict(prop=-0.001), "prop_decrease"), (dict(prop=1.001), "prop_decrease"), (dict(prop=float("nan")), "prop_decrease"),
    (dict(chunk=0), "chunk_size"), (dict(chunk=-5), "chunk_size"),
    (dict(pad=-1), "padding"),
    (dict(ws_bytes=0), "workspace too small"),
    (dict(n=1 << 40, chunk=1 << 40), "exceeds"), (dict(pad=1 << 40), "exceeds"),
]


def _forward(native, a):
    """rvc_spectral_gate_f32 on addresses that are never dereferenced: `1` stands for a host buffer the library must not touch"""
    host = (ctypes.c_float * 4)()
    ptr = lambda v: ctypes.addressof(host) if v == 1 else None
    ws_bytes = a["ws_bytes"]
    if ws_bytes == 1 << 40:   # "large enough": exactly what the query asks for
        need = ctypes.c_size_t()
        if native._lib.rvc_spectral_gate_workspace_bytes(a["n"], a["sr"], a["chunk"], a["pad"], ctypes.byref(need)) == 0:
            ws_bytes = need.value
    return native._lib.rvc_spectral_gate_f32(ptr(a["y"]), a["n"], a["sr"], a["prop"], a["chunk"], a["pad"], ptr(a["out"]), ptr(a["ws"]),
                                             ws_bytes, None)


@pytest.mark.parametrize("change,words", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_abi_refuses_before_any_device_access(native, change, words):
    assert _forward(native, {**GOOD, **change}) != 0
    assert words in _err(native), _err(native)


def test_abi_workspace_is_one_byte_short(native):
    need = ctypes.c_size_t()
    assert native._lib.rvc_spectral_gate_workspace_bytes(9000, 48000, 600000, 30000, ctypes.byref(need)) == 0
    assert need.value == 17920 * 384                      # 270 frames -> 384 GEMM rows, 17.5 KiB each
    assert _forward(native, {**GOOD, "ws_bytes": need.value - 1}) != 0
    assert "workspace too small" in _err(native)


def test_abi_empty_signal_succeeds_and_touches_nothing(native):
    need = ctypes.c_size_t(7)
    assert native._lib.rvc_spectral_gate_workspace_bytes(0, 48000, 600000, 30000, ctypes.byref(need)) == 0 and need.value == 0
    assert _forward(native, {**GOOD, "n": 0, "ws_bytes": 0}) == 0


def test_abi_workspace_query_refusals_and_bound(native):
    lib, need = native._lib, ctypes.c_size_t()
    assert lib.rvc_spectral_gate_workspace_bytes(9000, 48000, 600000, 30000, None) != 0
    for n, sr, chunk, pad in ((-1, 48000, 600000, 30000), (9000, 5119, 600000, 30000), (9000, 256001, 600000, 30000),
                              (9000, 48000, 0, 30000), (9000, 48000, 600000, -1)):
        assert lib.rvc_spectral_gate_workspace_bytes(n, sr, chunk, pad, ctypes.byref(need)) != 0, (n, sr, chunk, pad)
    # independent of n once the signal fills one group of chunks: 3 default chunks of 2579 frames fit into 8192 frames
    sizes = []
    for n in (600000 * 3, 600000 * 4, 600000 * 400 + 17):
        assert lib.rvc_spectral_gate_workspace_bytes(n, 48000, 600000, 30000, ctypes.byref(need)) == 0
        sizes.append(need.value)
    assert sizes[0] == sizes[1] == sizes[2] == 17920 * 7808   # 3 x 2579 = 7737 frames -> 7808 GEMM rows


def test_abi_params_refusals(native):
    nf, nt, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    lib = native._lib
    assert lib.rvc_spectral_gate_params(48000, None, ctypes.byref(nt), ctypes.byref(b), None, None) != 0
    assert lib.rvc_spectral_gate_params(5119, ctypes.byref(nf), ctypes.byref(nt), ctypes.byref(b), None, None) != 0
    for sr in (5120, 256000):   # the bounds themselves: both half-widths still at least 1
        assert lib.rvc_spectral_gate_params(sr, ctypes.byref(nf), ctypes.byref(nt), ctypes.byref(b), None, None) == 0
        assert (nf.value, nt.value) == R.parameters(sr)[:2] and min(nf.value, nt.value) == 1


# ---- host constants vs the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,shape", [(16000, (33, 7)), (32000, (17, 13)), (40000, (13, 15)), (48000, (11, 19))])
def test_host_constants_equal_the_restatement(native, sr, shape):
    from rvc_amd.lib.noise_reduce import gate_parameters
    nf, nt, b, filt = gate_parameters(sr)
    nf_r, nt_r, b_r, filt_r = R.parameters(sr)
    assert (nf, nt) == (nf_r, nt_r) and filt.shape == filt_r.shape == shape
    assert abs(b - b_r) <= np.spacing(b_r)
    assert np.abs(filt - filt_r).max() <= 4 * np.finfo(np.float64).eps * filt_r.max()
    assert abs(filt.sum() - 1) <= 1e-14


def test_restatement_is_an_identity_at_prop_decrease_zero():
    x = R.test_signal(9000, 48000)
    for kw in ({}, dict(chunk_size=4096, padding=2048)):
        assert np.abs(R.reduce_noise(x, 48000, 0.0, **kw) - x).max() <= 1e-12
    assert R.rms(R.reduce_noise(x, 48000, 0.7) - x) > 0.01      # ... and does something otherwise
    z = R.reduce_noise(np.zeros(3000), 48000, 0.7)
    assert np.isfinite(z).all() and not z.any()


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(stationary=True), dict(y_noise=np.zeros(16)), dict(n_fft=2048), dict(use_torch=True),
                                dict(hop_length=512), dict(win_length=512), dict(time_constant_s=1.0), dict(freq_mask_smooth_hz=250),
                                dict(time_mask_smooth_ms=25), dict(thresh_n_mult_nonstationary=1), dict(sigmoid_slope_nonstationary=5),
                                dict(n_jobs=2), dict(tmp_folder="/x")], ids=lambda kw: next(iter(kw)))
def test_unbuilt_keywords_are_refused_by_name(native, kw, monkeypatch):
    from rvc_amd.lib import noise_reduce as NR
    monkeypatch.setattr(NR._native, "spectral_gate", lambda *a, **k: pytest.fail("refused calls must not reach the library"))
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        NR.reduce_noise(np.zeros(64, dtype=np.float32), 48000, **kw)


def test_built_defaults_and_shape_checks(native, monkeypatch):
    from rvc_amd.lib import noise_reduce as NR
    seen = []

    def stub(y, sr, prop, chunk, pad):
        seen.append((y.dtype, tuple(y.shape), sr, prop, chunk, pad))
        return y.clone()
    monkeypatch.setattr(NR._native, "spectral_gate", stub)
    y = torch.zeros(64, dtype=torch.float64)
    out = NR.reduce_noise(y, 48000.0, 0.5, stationary=False, y_noise=None, n_fft=1024, win_length=None, hop_length=256, use_torch=False,
                          time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, thresh_n_mult_nonstationary=2,
                          sigmoid_slope_nonstationary=10, n_std_thresh_stationary=1.5, tmp_folder=None, clip_noise_stationary=True,
                          use_tqdm=False, n_jobs=1)
    assert out.dtype == torch.float32 and seen == [(torch.float32, (64,), 48000, 0.5, 600000, 30000)]
    NR.reduce_noise(y, 16000, chunk_size=4096, padding=2048)
    assert seen[-1][2:] == (16000, 1.0, 4096, 2048)
    for bad in (np.zeros((2, 64), dtype=np.float32), torch.zeros(2, 64)):
        with pytest.raises(ValueError, match="1-D"):
            NR.reduce_noise(bad, 48000)
    with pytest.raises(TypeError, match="no_such_keyword"):
        NR.reduce_noise(y, 48000, no_such_keyword=1)
    with pytest.raises(ValueError, match="sr"):
        NR.reduce_noise(y, 44100.5)
    assert len(seen) == 2


# ---- VoiceConverter's routing (pipeline and library stubbed) ------------------------------------------------------------------------
class _Pipe:
    trim_vocoder_pad = True

    def __init__(self, out):
        self.out = out

    def pipeline(self, **kw):
        return self.out.copy()


def _converter(out):
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter.__new__(VoiceConverter)
    vc.vc, vc.tgt_sr, vc.hubert_model, vc.net_g, vc.use_f0, vc.version, vc.trim_vocoder_pad = _Pipe(out), 40000, None, None, 1, "v2", True
    return vc


def test_clean_audio_reaches_remove_audio_noise(native, monkeypatch, capsys):
    from rvc_amd.infer import infer as I
    raw = np.linspace(-0.5, 0.5, 400, dtype=np.float32)
    vc, calls = _converter(raw), []

    def fake_reduce(y, sr, prop_decrease):
        calls.append((y.copy(), sr, prop_decrease))
        return y * 0.5
    monkeypatch.setattr(I, "reduce_noise", fake_reduce)
    a = np.zeros(1600)
    assert np.array_equal(vc.convert_array(a), raw) and calls == []                        # default: untouched, nothing called
    assert np.array_equal(vc.convert_array(a, clean_audio=False, clean_strength=0.9), raw) and calls == []
    assert np.array_equal(vc.convert_array(a, clean_audio=True), raw * 0.5)
    assert np.array_equal(calls[0][0], raw) and calls[0][1:] == (40000, 0.5)                # (audio, tgt_sr, clean_strength default)
    vc.convert_array(a, clean_audio=True, clean_strength=0.25)
    assert calls[1][1:] == (40000, 0.25)
    assert np.array_equal(I.VoiceConverter.remove_audio_noise(raw, 32000), raw * 0.5) and calls[2][1:] == (32000, 0.7)

    def broken(y, sr, prop_decrease):
        raise RuntimeError("no device")
    monkeypatch.setattr(I, "reduce_noise", broken)
    capsys.readouterr()
    assert I.VoiceConverter.remove_audio_noise(raw, 40000) is None
    assert "An error occurred removing audio noise: no device" in capsys.readouterr().out
    assert np.array_equal(vc.convert_array(a, clean_audio=True), raw)                      # None -> the uncleaned audio is kept


def test_convert_audio_passes_clean_audio_through_and_still_refuses_the_rest(native, monkeypatch, capsys, tmp_path):
    from rvc_amd.infer import infer as I
    raw = np.linspace(-0.5, 0.5, 400, dtype=np.float32)
    vc = _converter(raw)
    vc.get_vc = lambda *a: None
    vc.last_embedder_model, vc.hubert_model = "contentvec", object()
    vc.config = type("C", (), {"device": "cpu"})()
    monkeypatch.setattr(I, "load_audio_infer", lambda *a, **k: np.zeros(1600))
    monkeypatch.setattr(I, "reduce_noise", lambda y, sr, prop_decrease: y * prop_decrease)
    written = {}
    monkeypatch.setattr(I, "_write_wav", lambda path, audio, sr: written.update({path: (np.array(audio), sr)}))
    vc.convert_audio("in.wav", "plain.wav", "model.pth", "")
    vc.convert_audio("in.wav", "clean.wav", "model.pth", "", clean_audio=True, clean_strength=0.25)
    assert np.array_equal(written["plain.wav"][0], raw) and np.array_equal(written["clean.wav"][0], raw * 0.25)
    assert written["clean.wav"][1] == 40000
    capsys.readouterr()
    for kw in (dict(post_process=True), dict(export_format="MP3"), dict(clean_audio=True, post_process=True)):
        vc.convert_audio("in.wav", "refused.wav", "model.pth", "", **kw)                    # never raises: prints the NotImplementedError
        assert "post_process / non-WAV export" in capsys.readouterr().out
    assert "refused.wav" not in written
