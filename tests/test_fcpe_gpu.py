"""FCPE (f0_method="fcpe") on the MI355X: the four K15 kernels (csrc/fcpe.hip) through `_native`, the network against the reference's
float64 twin, and the three call sites against the reference's own results.  Fixtures: tests/golden/make_golden_fcpe.py.

KERNEL GATES.  Each kernel is compared with a float64 evaluation of its defining expression on the CPU, and so is torch's own fp32
evaluation of the same expression on the same operands; the kernel may leave at most a fixed multiple of torch's error.  The
multiples are the ones tests/test_front_kernels_gpu.py uses: ELEMENTWISE = 2 x on the maximum absolute error (its gate test) for the
GLU / FIR / SiLU kernel and the decoder, NORM = 1.5 x on the relative RMS error with a floor of 3e-7 and a cap of 2e-5 of the largest
value on the maximum absolute error (its LayerNorm tests) for the two normalisations.
MODEL GATES.  Latent: max abs error against the float64 twin at most REF32 = 8 x the error the fp32 reference itself leaves against
that twin (recorded in the fixture) -- the footing the K11 tests give a bf16x3 GEMM next to an fp32 one.  Voicing masks and arg-max
exact, f0 within 8 x the fp32 reference's own relative error, on every frame the fixture does not mark as a tie (top-2 latent gap or
distance from the threshold below 1e-4; the generator asserts there is none, and at most 2 % of a case may ever be skipped)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ELEMENTWISE, NORM, NORM_FLOOR, NORM_MAXABS, REF32 = 2.0, 1.5, 3e-7, 2e-5, 8.0
GLU_TILE = 128            # csrc/fcpe.hip: time rows per workgroup
SENT32 = 0x5A5A5A5A       # fp32 1.5e16: no kernel under test produces it
CONFIGS = ((512, 6), (128, 2))
LENGTHS = (2600, 48077)


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def S():
    from rvc_amd.lib import synthetic
    return synthetic


def _guarded(shape, band=4096):
    """A sentinel-filled buffer with `band` canary elements on BOTH sides of the view of `shape` -> (view, whole buffer)."""
    n = math.prod(shape)
    buf = torch.empty(n + 2 * band, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SENT32)
    return buf[band: band + n].view(shape), buf


def _canaries_intact(buf, n, band=4096):
    bits = buf.view(torch.int32)
    return bool((bits[:band] == SENT32).all().item() and (bits[band + n:] == SENT32).all().item())


def _maxabs(t, r):
    return (t.double().cpu() - r).abs().max().item()


def _rel(t, r):
    return ((t.double().cpu() - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp_min(1e-300)).item()


# ---- (a) GLU + depthwise conv + SiLU ------------------------------------------------------------------------------------------
def _glu_ref(x, w, b):
    """silu(depthwise_conv(value * sigmoid(gate))) on time-major rows, in x's dtype"""
    c, k = w.shape
    u = (x[:, :c] * torch.sigmoid(x[:, c:])).t().unsqueeze(0)
    v = F.conv1d(u, w.unsqueeze(1), b, padding=k // 2, groups=c)[0].t()
    return v * torch.sigmoid(v)


@pytest.mark.parametrize("n_rows,c,k", [(1, 64, 31), (17, 64, 31), (31, 128, 3), (301, 1024, 31), (64, 64, 1), (GLU_TILE + 1, 64, 31)])
def test_glu_dwconv_silu_matches_float64(native, n_rows, c, k):
    g = torch.Generator().manual_seed(n_rows * 1000 + c + k)
    x = torch.randn(n_rows, 2 * c, generator=g) * 1.5
    w = torch.randn(c, k, generator=g) / math.sqrt(k)
    b = torch.randn(c, generator=g) * 0.1
    ref, lib = _glu_ref(x.double(), w.double(), b.double()), _glu_ref(x, w, b)
    y, buf = _guarded((n_rows, c))
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    rc = native._lib.rvc_glu_dwconv_silu_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), n_rows, c, k, native._stream())
    torch.cuda.synchronize()
    assert rc == 0, native._lib.rvc_last_error()
    assert _canaries_intact(buf, y.numel())
    assert torch.equal(native.glu_dwconv_silu(xd, wd, bd), y)
    e, el = _maxabs(y, ref), (lib.double() - ref).abs().max().item()
    print(f"glu_dwconv_silu [{n_rows} x {c}] k {k}: max abs {e:.2e} (torch fp32 {el:.2e}, ratio {e / max(el, 1e-30):.2f})")
    assert torch.isfinite(y).all()
    assert e <= ELEMENTWISE * el, (e, el)


# ---- (b) LayerNorm over rows ----------------------------------------------------------------------------------------------------
def _norm_gate(got, ref, lib, what):
    e, r, rl = _maxabs(got, ref), _rel(got, ref), _rel(lib, ref)
    print(f"{what}: max abs {e:.2e}, rel rms {r:.2e} (torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f})")
    assert e <= NORM_MAXABS * max(1.0, ref.abs().max().item()), e
    assert r <= max(NORM * rl, NORM_FLOOR), (r, rl)


@pytest.mark.parametrize("rows", [1, 17, 301])
@pytest.mark.parametrize("features", [64, 128, 512, 1024])
def test_layernorm_rows_matches_float64(native, features, rows):
    g = torch.Generator().manual_seed(features + rows)
    gamma, beta = 1 + 0.1 * torch.randn(features, generator=g), 0.1 * torch.randn(features, generator=g)
    for mean, what in ((0.0, "unit"), (50.0, "mean 50")):          # mean 50, std 1: a one-pass E[x^2] - E[x]^2 loses the variance
        x = torch.randn(rows, features, generator=g) + mean
        ref = F.layer_norm(x.double(), (features,), gamma.double(), beta.double(), 1e-5)
        lib = F.layer_norm(x, (features,), gamma, beta, 1e-5)
        y, buf = _guarded((rows, features))
        xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        rc = native._lib.rvc_layernorm_rows_f32(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, y.data_ptr(), rows, features, native._stream())
        torch.cuda.synchronize()
        assert rc == 0, native._lib.rvc_last_error()
        assert _canaries_intact(buf, y.numel())
        assert torch.equal(native.layernorm_rows(xd, gd, bd), y)
        _norm_gate(y, ref, lib, f"layernorm_rows [{rows} x {features}] {what}")


# ---- (c) GroupNorm + LeakyReLU --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,length,groups", [(128, 17, 4), (512, 301, 4), (512, 2049, 4)])   # the last: 17 partial blocks per group
def test_groupnorm_lrelu_matches_float64(native, c, length, groups):
    g = torch.Generator().manual_seed(c + length)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    for mean, what in ((0.0, "unit"), (50.0, "mean 50")):
        x = torch.randn(c, length, generator=g) + mean
        ref = F.leaky_relu(F.group_norm(x.double().unsqueeze(0), groups, gamma.double(), beta.double(), 1e-5), 0.01)[0]
        lib = F.leaky_relu(F.group_norm(x.unsqueeze(0), groups, gamma, beta, 1e-5), 0.01)[0]
        y, buf = _guarded((c, length))
        xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        need = ctypes.c_size_t()
        assert native._lib.rvc_groupnorm_workspace_bytes(c, length, groups, ctypes.byref(need)) == 0
        ws, wsbuf = _guarded((need.value // 4,))
        rc = native._lib.rvc_groupnorm_lrelu_f32(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), groups, 1e-5, 0.01, y.data_ptr(), c, length,
                                                 ws.data_ptr(), need.value, native._stream())
        torch.cuda.synchronize()
        assert rc == 0, native._lib.rvc_last_error()
        assert _canaries_intact(buf, y.numel()) and _canaries_intact(wsbuf, ws.numel())
        assert torch.equal(native.groupnorm_lrelu(xd, gd, bd, groups), y)
        _norm_gate(y, ref, lib, f"groupnorm_lrelu [{c} x {length}] / {groups} {what}")


# ---- (d) decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [360, 384])
def test_fcpe_decode_matches_reference_decoder(native, S, ld):
    """Crafted rows (peaks whose nine-bin window is clamped at either end, two exactly equal maxima, a confidence exactly on the
    threshold, peaks that decode below f0_min, random rows) against the reference's decoder in float64: masks and arg-max exact,
    f0 within ELEMENTWISE x the fp32 reference's own relative error.  With ld = 384 the pad columns hold +1e30 (never read)."""
    g = load_golden("fcpe_decode")
    logits = torch.from_numpy(g["logits"])
    n = logits.shape[0]
    padded = torch.full((n, ld), 1e30)
    padded[:, :360] = logits
    cent = S.make_fcpe_checkpoint(0, hidden=128, layers=2)["model"]["cent_table"].to(DEV)
    for name in ("model", "80"):
        f0_min, want = float(g[f"f0_min_{name}"]), g[f"f0_{name}"]
        f0, buf = _guarded((n,))
        lat, lbuf = _guarded((n, 360))
        ld_dev = padded.to(DEV)
        rc = native._lib.rvc_fcpe_decode_f32(ld_dev.data_ptr(), cent.data_ptr(), 360, ld, float(g["threshold"]), f0_min, f0.data_ptr(),
                                             lat.data_ptr(), n, native._stream())
        torch.cuda.synchronize()
        assert rc == 0, native._lib.rvc_last_error()
        assert _canaries_intact(buf, n) and _canaries_intact(lbuf, lat.numel())
        got = f0.cpu().numpy().astype(np.float64)
        assert np.array_equal(got > 0, want > 0), (np.nonzero((got > 0) != (want > 0)), got, want)
        am = lat.cpu().numpy()
        assert np.array_equal(am.argmax(1), g["argmax"])                       # numpy's argmax: the lowest index of equals
        assert np.abs(am - torch.sigmoid(logits.double()).numpy()).max() <= 4 * 2.0 ** -24          # 4 ulp of a value below 1
        v = want > 0
        e, gate = np.abs(got[v] / want[v] - 1).max(), ELEMENTWISE * float(g[f"ref32_f0_relerr_{name}"])
        print(f"fcpe_decode ld {ld}, f0_min {f0_min}: {int(v.sum())} of {n} voiced, f0 max rel err {e:.2e} (gate {gate:.2e})")
        assert e <= gate
        f0b, _ = native.fcpe_decode(ld_dev, cent, 360, float(g["threshold"]), f0_min)      # latent_dev NULL
        assert torch.equal(f0b, f0)
    assert got[10] == 0 and got[11] > 0 and am[8, 100] == am[8, 220] and am[9, 40] == am[9, 41]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
_models = {}


def _fcpe(S, hidden=512, layers=6):
    from rvc_amd.lib.predictors.FCPE import FCPE
    if (hidden, layers) not in _models:
        _models[(hidden, layers)] = FCPE(device=DEV, checkpoint=S.make_fcpe_checkpoint(0, hidden=hidden, layers=layers))
    return _models[(hidden, layers)]


def _check_contour(g, tag, f0, latent, what):
    """masks and arg-max exact, f0 within REF32 x the fp32 reference's relative error, on every frame the fixture does not mark a tie"""
    want, lat64 = g[f"f0_{tag}"], g[f"latent_{tag}"]
    keep = (g[f"gap_{tag}"] >= float(g["tie_margin"])) & (g[f"thrdist_{tag}"] >= float(g["tie_margin"]))
    assert (~keep).sum() <= 0.02 * len(keep), f"{tag}: {(~keep).sum()} tie frames"
    assert f0.shape == want.shape
    assert np.array_equal(f0[keep] > 0, want[keep] > 0), np.nonzero((f0 > 0) != (want > 0))
    assert np.array_equal(latent.argmax(1)[keep], lat64.argmax(1)[keep])
    v = keep & (want > 0)
    e, gate = np.abs(f0[v] / want[v] - 1).max(), REF32 * float(g[f"ref32_f0_relerr_{tag}"])
    print(f"{what} {tag}: {int(v.sum())} voiced of {len(want)} frames, f0 max rel err {e:.2e} (gate {gate:.2e})")
    assert e <= gate, (e, gate)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("hidden,layers", CONFIGS)
def test_fcpe_network_matches_float64_twin(native, S, hidden, layers, n):
    g = load_golden(f"fcpe_{hidden}x{layers}")
    tag = f"{hidden}x{layers}_{n}"
    m = _fcpe(S, hidden, layers)
    audio = torch.from_numpy(S.synth_gated_glide(n, int(g[f"audio_seed_{n}"])).astype(np.float32)).to(DEV)
    mel = m.mel_device(audio)
    assert mel.shape == (128, n // 160 + 1)
    e_mel = np.abs(mel.t().cpu().numpy() - g[f"mel_{n}"]).max()
    print(f"fcpe mel {n}: max abs err {e_mel:.2e} (gate 2e-3, the K4b tests' log-domain tolerance)")
    assert e_mel <= 2e-3
    # the network on the REFERENCE's mel: the operands the float64 twin had
    logits = m.logits_device(torch.from_numpy(g[f"mel_{n}"]).to(DEV).t().contiguous())
    assert logits.shape == (n // 160 + 1, 384)
    f0, latent = native.fcpe_decode(logits, m.w["cent_table"], 360, float(g[f"threshold_{tag}"]), m.model_f0_min, want_latent=True)
    latent = latent.cpu().numpy()
    e, gate = np.abs(latent.astype(np.float64) - g[f"latent_{tag}"]).max(), REF32 * float(g[f"ref32_latent_err_{tag}"])
    print(f"fcpe latent {tag}: max abs err {e:.2e} against the float64 twin (fp32 reference {float(g[f'ref32_latent_err_{tag}']):.2e}, gate {gate:.2e})")
    assert e <= gate, (e, gate)
    _check_contour(g, tag, f0.cpu().numpy().astype(np.float64), latent, "fcpe network on the reference's mel")
    # ... and the whole estimator from the audio
    taps = {}
    f0 = m.infer_device(audio, float(g[f"threshold_{tag}"]), taps=taps)
    _check_contour(g, tag, f0.cpu().numpy().astype(np.float64), taps["latent"].cpu().numpy(), "fcpe from audio")


# ---- the three call sites ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hubert(S):
    from rvc_amd.lib.hubert import HubertModelWithFinalProj
    return HubertModelWithFinalProj(S.make_hubert_state_dict(1), device=DEV)


@pytest.fixture(scope="module")
def converter(S, hubert):
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter(device=DEV)
    vc.load_checkpoint_dict(S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0, smooth_pitch=True))
    vc.hubert_model = hubert
    vc.vc.load_fcpe_state_dict(S.make_fcpe_checkpoint(0))
    vc.vc.set_index(S.synth_index(4096, seed=0))
    return vc


def _audio_pad(audio):
    """what Pipeline.pipeline hands to get_f0: high-pass, 1 s reflect padding (pipeline.py:562, 579)"""
    from scipy import signal
    from rvc_amd.infer import pipeline as P
    return np.pad(signal.filtfilt(P.bh, P.ah, audio), (16000, 16000), mode="reflect")


def test_compute_f0_and_get_f0_match_the_reference(S, converter):
    g = load_golden("pipeline_fcpe")
    gate = REF32 * float(load_golden("fcpe_512x6")["ref32_f0_relerr_512x6_48077"])
    ap, thr = _audio_pad(g["audio"]), float(g["threshold"])
    p_len = ap.shape[0] // 160
    assert p_len == len(g["f0bak"])
    f0 = converter.vc.model_fcpe.compute_f0(ap, p_len=p_len, filter_radius=thr)
    assert f0.dtype == np.float64 and f0.shape == g["f0bak"].shape
    for x, what in ((ap, "NumPy"), (torch.from_numpy(ap).to(DEV), "device tensor")):
        coarse, f0bak = converter.vc.get_f0("path", x, p_len, 0, "fcpe", thr, 128, False, 1, None)
        assert np.array_equal(f0bak, f0)
        e = np.abs(f0bak / g["f0bak"] - 1).max()
        print(f"get_f0 fcpe ({what}): f0bak max rel err {e:.2e} (gate {gate:.2e}), coarse differs on {int((coarse != g['coarse']).sum())} frames")
        assert np.all(g["f0bak"] > 0) and e <= gate, (e, gate)
        assert np.array_equal(coarse, g["coarse"])
    assert converter.vc._fcpe() is converter.vc.model_fcpe                # cached, not reloaded per call


def test_feature_input_compute_f0_is_fcpe_compute_f0(S, converter):
    from rvc_amd.train.extract.extract import FeatureInput
    x = S.synth_gated_glide(16000, 3).astype(np.float32)
    fi = FeatureInput(device=DEV)
    fi.load_fcpe(S.make_fcpe_checkpoint(0))
    got = fi.compute_f0(x, "fcpe", 160)
    want = converter.vc.model_fcpe.compute_f0(x)
    assert got.shape == (101,) and np.array_equal(got, want) and got.any()


@pytest.mark.parametrize("as_tensor", [False, True])
def test_pipeline_fcpe_matches_reference_golden(converter, hubert, as_tensor):
    """Whole Pipeline.pipeline with f0_method="fcpe" against the REFERENCE's output: waveform RMS error <= 1e-3, unconditionally."""
    g = load_golden("pipeline_fcpe")
    audio = torch.from_numpy(g["audio"]).to(DEV) if as_tensor else g["audio"].copy()
    out = converter.vc.pipeline(hubert, converter.net_g, int(g["sid"]), audio, 0, "fcpe", "", float(g["index_rate"]), True,
                                float(g["threshold"]), 1, "v2", float(g["protect"]), 128, False, 1, None, noise_seed=int(g["seed"]))
    if as_tensor:
        assert torch.is_tensor(out) and out.is_cuda
        out = out.cpu().numpy()
    assert out.shape == g["out"].shape
    err = rms(out - g["out"])
    print(f"pipeline (fcpe, {'device tensor' if as_tensor else 'NumPy'} in) vs reference: rms err {err:.3e} (gate 1e-3)")
    assert err <= 1e-3, err


def test_default_filter_radius_masks_every_frame(converter, hubert, S):
    """convert_audio's default filter_radius = 3 reaches FCPE as its confidence threshold (pipeline.py:370): no sigmoid exceeds it,
    the contour is all zeros, the coarse pitch all ones -- the reference's behaviour, kept -- and the conversion completes."""
    audio = S.synth_gated_glide(16000, 4)
    ap = _audio_pad(audio)
    coarse, f0bak = converter.vc.get_f0("path", ap, ap.shape[0] // 160, 0, "fcpe", 3, 128, False, 1, None)
    assert not f0bak.any() and np.all(coarse == 1)
    out = converter.convert_array(audio, f0_method="fcpe", index_rate=0.0)
    assert out.ndim == 1 and out.shape[0] > 40000 and np.isfinite(out).all() and np.abs(out).max() > 0


def test_convert_audio_fcpe_reads_fcpe_pt_and_writes_a_wav(S, tmp_path, monkeypatch):
    """VoiceConverter.convert_audio(..., f0_method="fcpe", filter_radius=0.006) end to end from files: fcpe.pt of the working
    directory is the checkpoint that gets loaded (a (128, 2) one here, told apart by its width), once, and a WAV comes out."""
    import struct
    import wave
    from rvc_amd.infer.infer import VoiceConverter
    monkeypatch.chdir(tmp_path)
    os.makedirs("rvc/models/embedders/contentvec")
    os.makedirs("rvc/models/predictors")
    torch.save(S.make_hubert_state_dict(1), "rvc/models/embedders/contentvec/pytorch_model.bin")
    torch.save(S.make_fcpe_checkpoint(0, hidden=128, layers=2), "rvc/models/predictors/fcpe.pt")
    torch.save(S.make_synth_checkpoint(40000, "HiFi-GAN", seed=0, half=True), "model.pth")
    mono = S.synth_gated_glide(16000, 2).astype("<f4")
    fmt = struct.pack("<HHIIHH", 3, 1, 16000, 16000 * 4, 4, 32)
    body = b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", mono.nbytes) + mono.tobytes()
    with open("in.wav", "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)
    vc = VoiceConverter(device=DEV)
    vc.convert_audio("in.wav", "out.wav", "model.pth", "", index_rate=0.0, f0_method="fcpe", filter_radius=0.006)
    model = vc.vc.model_fcpe
    assert model is not None and model.hidden == 128 and model.n_layers == 2
    with wave.open("out.wav", "rb") as f:
        assert f.getframerate() == 40000 and f.getnframes() > 30000
        got = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert np.abs(got).max() > 0
    vc.convert_audio("in.wav", "out2.wav", "model.pth", "", index_rate=0.0, f0_method="fcpe", filter_radius=0.006)
    assert vc.vc.model_fcpe is model and os.path.getsize("out2.wav") == os.path.getsize("out.wav")
