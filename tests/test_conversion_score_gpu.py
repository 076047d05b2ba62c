"""K24 (the conversion scorer, csrc/convscore.hip) and rvc_amd.lib.tools.score on the GPU against the float64 twin of
tests/conversion_score_ref.py.

Gates.  Cepstra: e_ref = the largest absolute error of the torch-fp32 evaluation of the twin against its float64 evaluation over
the cases; the device must stay within 16 e_ref on EVERY case (K18 - K20's multiple for long fp32 dot products: the device's DFT is
fp32, everything after it float64).  Every case but n = 1 first asserts that another seed's coefficients differ by more than 100
gates; the cepstra c[1 ..] of a single sample do not depend on its value (a flat spectrum: the value moves every log mel energy by
one constant, which the DCT rows k >= 1 do not see), so for n = 1 that is asserted of the twin instead.  DTW and the F0 sums:
both sides are float64 and differ by the fused multiply-add and the order of a sum, a few 2^-53 per term: 1e-12 relative.  Every
figure is printed before it is asserted (pytest -s shows them).  Raw calls write into outputs and workspaces of exactly the
queried size with canaries on both sides."""
import functools
import math

import numpy as np
import pytest
import torch

import conversion_score_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                      # bytes on either side
FILL = 0xA5
CEP_CASES = ((1, 16000), (79, 16000), (80, 16000), (2559, 16000), (2560, 16000), (5151, 16000), (7200, 48000))
CEP_FRAMES = (1, 1, 2, 32, 33, 65, 31)
DTW_CASES = ((1, 1, None), (1, 9, None), (9, 1, None), (2, 2, None), (63, 65, None), (64, 64, None), (65, 129, None), (257, 200, None),
             (2049, 1900, None), (200, 257, 1), (257, 200, 8))
F0_CASES = (1, 63, 1025, 4101)


@pytest.fixture(scope="module")
def N():
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def M():
    from rvc_amd.lib import metrics
    return metrics


def _guarded(nbytes, dtype):
    buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf[GUARD: GUARD + nbytes].view(dtype), buf


def _intact(buf):
    return bool((buf[:GUARD] == FILL).all().item() and (buf[-GUARD:] == FILL).all().item())


def _dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def _raw_melcep(N, x32, sr, n_mels=80, n_coef=24):
    x, mel = _dev(x32), _dev(R.mel_matrix(sr, n_mels))
    T = 1 + x.numel() // (sr // 200)
    need = N._size("rvc_melcep_workspace_bytes", torch.device(DEV), x.numel(), sr)
    out, obuf = _guarded(T * n_coef * 4, torch.float32)
    ws, wbuf = _guarded(need, torch.uint8)
    N._call("rvc_melcep_f32", torch.device(DEV), x.data_ptr(), x.numel(), sr, mel.data_ptr(), n_mels, n_coef, out.data_ptr(), ws.data_ptr(),
            need)
    torch.cuda.synchronize()
    assert _intact(obuf) and _intact(wbuf)
    return out.cpu().numpy().astype(np.float64).reshape(T, n_coef)


def _raw_dtw(N, a, b, band=None):
    """-> (cost, path [L, 2]); the rows of the path past L must still hold the canary"""
    a, b = _dev(a).reshape(len(a), -1), _dev(b).reshape(len(b), -1)
    Ta, Tb = a.shape[0], b.shape[0]
    need = N._size("rvc_dtw_workspace_bytes", torch.device(DEV), Ta, Tb)
    out, obuf = _guarded(16, torch.float64)
    path, pbuf = _guarded((Ta + Tb - 1) * 8, torch.int32)
    ws, wbuf = _guarded(need, torch.uint8)
    N._call("rvc_dtw_f64", torch.device(DEV), a.data_ptr(), Ta, b.data_ptr(), Tb, a.shape[1], -1 if band is None else band, out.data_ptr(),
            path.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert _intact(obuf) and _intact(pbuf) and _intact(wbuf)
    cost, length = out.cpu().tolist()
    L = int(length)
    assert L == length and 1 <= L <= Ta + Tb - 1
    assert bool((path.view(torch.uint8)[L * 8:] == FILL).all().item()), "rows past L were written"
    return cost, path.cpu().numpy().reshape(-1, 2)[:L].astype(np.int64)


def _raw_f0(N, fa, fb):
    a, b = _dev(fa, np.float64), _dev(fb, np.float64)
    out, obuf = _guarded(12 * 8, torch.float64)
    N._call("rvc_f0_track_sums_f64", torch.device(DEV), a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr())
    torch.cuda.synchronize()
    assert _intact(obuf)
    return out.cpu().numpy()


def _raw_dist(N, a, b, T):
    a, b = _dev(a), _dev(b)
    out, obuf = _guarded(8, torch.float64)
    N._call("rvc_frame_dist_sum_f64", torch.device(DEV), a.data_ptr(), b.data_ptr(), T, a.shape[1], out.data_ptr())
    torch.cuda.synchronize()
    assert _intact(obuf)
    return float(out.item())


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


# ---- cepstra -------------------------------------------------------------------------------------------------------------------------
def _voice32(n, sr, seed):
    return R.voice(max(n, 2), sr, seed)[:n].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _cep_ref(n, sr):
    """-> (x32, twin in float64, twin in torch-fp32, another seed's twin); computed once, never modified"""
    x = _voice32(n, sr, 7)
    return x, R.melcep(x, sr), R.melcep_torch(x, sr, torch.float32), R.melcep(_voice32(n, sr, 8), sr)


@functools.lru_cache(maxsize=None)
def _cep_gate():
    e_ref = max(float(np.abs(_cep_ref(n, sr)[2] - _cep_ref(n, sr)[1]).max()) for n, sr in CEP_CASES)
    return e_ref, 16 * e_ref


@pytest.mark.parametrize("n,sr", CEP_CASES)
def test_cepstra_against_twin(N, n, sr):
    x, c64, c32, other = _cep_ref(n, sr)
    e_ref, gate = _cep_gate()
    assert c64.shape == (CEP_FRAMES[CEP_CASES.index((n, sr))], 24)
    moved = float(np.abs(other - c64).max())
    dev = _raw_melcep(N, x, sr)
    err = float(np.abs(dev - c64).max())
    print(f"[melcep] n={n} sr={sr}: T={len(c64)} max|c|={np.abs(c64).max():.4g} torch32 err={np.abs(c32 - c64).max():.3g} "
          f"device err={err:.3g} e_ref={e_ref:.3g} gate={gate:.3g} ({err / e_ref:.2f} e_ref); another seed moves c by {moved:.3g}")
    if n == 1:   # one sample: a flat spectrum whose level no c[k >= 1] sees
        assert float(np.abs(R.melcep(2 * x, sr) - c64).max()) < 1e-12
    else:
        assert moved > 100 * gate
    assert dev.shape == c64.shape and np.isfinite(dev).all()
    assert err <= gate


def test_cepstra_other_sizes_and_two_calls(N):
    """n_mels = 40 with n_coef = 13 (another filterbank and DCT), and identical bits from two calls"""
    x, sr = _cep_ref(5151, 16000)[0], 16000
    e_ref, gate = _cep_gate()
    ref = R.melcep(x, sr, 40, 13)
    dev = _raw_melcep(N, x, sr, 40, 13)
    err = float(np.abs(dev - ref).max())
    print(f"[melcep] 40 mels, 13 coefficients: device err={err:.3g} gate={gate:.3g}")
    assert err <= gate
    assert np.array_equal(dev, _raw_melcep(N, x, sr, 40, 13))


def test_cepstra_more_than_one_group(N, M):
    """2049 frames: the second group of frames holds one frame"""
    sr, n = 16000, 2048 * 80
    x = R.voice(n, sr, 9).astype(np.float32)
    e_ref, gate = _cep_gate()
    dev = M.mel_cepstra(x, sr, device=DEV).cpu().numpy().astype(np.float64)
    err = float(np.abs(dev - R.melcep(x, sr)).max())
    print(f"[melcep] 2049 frames: device err={err:.3g} gate={gate:.3g}")
    assert dev.shape == (2049, 24) and err <= gate


def test_cepstra_of_digital_silence(N):
    dev = _raw_melcep(N, np.zeros(2560, dtype=np.float32), 16000)
    print(f"[melcep] silence: max|c|={np.abs(dev).max():.3g}")
    assert np.isfinite(dev).all() and np.abs(dev).max() < 1e-9


# ---- DTW -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dtw_ref(Ta, Tb, band):
    rng = np.random.default_rng([Ta, Tb, 24])
    a, b = rng.standard_normal((Ta, 24)).astype(np.float32), rng.standard_normal((Tb, 24)).astype(np.float32)
    return (a, b) + R.dtw(a, b, band)


@pytest.mark.parametrize("Ta,Tb,band", DTW_CASES)
def test_dtw_against_twin(N, Ta, Tb, band):
    a, b, cost64, path64 = _dtw_ref(Ta, Tb, band)
    cost, path = _raw_dtw(N, a, b, band)
    resummed = R.path_cost(a, b, path)
    print(f"[dtw] {Ta} x {Tb} band={band}: twin={cost64:.15g} device={cost:.15g} rel err={rel(cost, cost64):.3g}; L={len(path)} "
          f"(twin {len(path64)}); path re-summed rel err={rel(resummed, cost64):.3g}; same path: {np.array_equal(path, path64)}")
    assert rel(cost, cost64) <= 1e-12
    R.check_path(path, Ta, Tb, band)
    assert rel(resummed, cost64) <= 1e-12


@pytest.mark.parametrize("dim,Ta,Tb", [(1, 70, 45), (25, 40, 1100), (33, 1030, 37), (64, 530, 90)])
def test_dtw_every_dim_path(N, dim, Ta, Tb):
    """the other template instances (8, 32, 48 and 64 lanes of features; 1024- and 512-row passes, more than one pass)"""
    rng = np.random.default_rng([dim, Ta, Tb])
    a, b = rng.standard_normal((Ta, dim)).astype(np.float32), rng.standard_normal((Tb, dim)).astype(np.float32)
    cost64, _ = R.dtw(a, b)
    cost, path = _raw_dtw(N, a, b)
    print(f"[dtw] dim {dim}, {Ta} x {Tb}: rel err={rel(cost, cost64):.3g}")
    assert rel(cost, cost64) <= 1e-12
    R.check_path(path, Ta, Tb)
    assert rel(R.path_cost(a, b, path), cost64) <= 1e-12


@pytest.mark.parametrize("Ta,Tb,band", [(65, 129, None), (257, 200, 8)])
def test_dtw_tie_rule_bit_equal(N, Ta, Tb, band):
    """integer-valued one-dimensional features: every distance and every sum is an exact integer and ties abound, so the total AND
    the path must equal the twin's bit for bit"""
    rng = np.random.default_rng([Ta, Tb, 1])
    a, b = rng.integers(0, 4, (Ta, 1)).astype(np.float32), rng.integers(0, 4, (Tb, 1)).astype(np.float32)
    cost64, path64 = R.dtw(a, b, band)
    cost, path = _raw_dtw(N, a, b, band)
    print(f"[dtw] ties {Ta} x {Tb} band={band}: twin={cost64} device={cost} L={len(path)} (twin {len(path64)})")
    assert cost == cost64 and np.array_equal(path, path64)


@pytest.mark.parametrize("dim,Ta,Tb,band,seed", [(1, 1100, 1200, 1, 1), (1, 1100, 1200, 8, 0), (1, 2100, 1500, 2, 2), (40, 600, 560, 1, 1),
                                                 (40, 1100, 700, 3, 3)])
def test_dtw_band_over_several_passes_bit_equal(N, dim, Ta, Tb, band, seed):
    """a band AND more than one pass of rows (1024 rows up to dim 32, 512 above): the first cell of a later pass takes its diagonal
    predecessor from the previous pass's last row, the pass walks its own column range, and the back-pointer words at the range's
    ends are partial.  Integer-valued features of which only one dimension varies: every distance is an exact integer, ties abound,
    so total and path must equal the twin's bit for bit.  The seeds of the narrow bands are ones at which the best path enters a pass
    through that corner: counting the corner's diagonal predecessor as +inf raises the total by 1 or 2 there (the band-8 case has
    too much slack for the total to move and checks the path)"""
    rng = np.random.default_rng([dim, Ta, Tb, band, seed])
    a, b = np.zeros((Ta, dim), dtype=np.float32), np.zeros((Tb, dim), dtype=np.float32)
    a[:, dim - 1], b[:, dim - 1] = rng.integers(0, 4, Ta), rng.integers(0, 4, Tb)
    cost64, path64 = R.dtw(a, b, band)
    cost, path = _raw_dtw(N, a, b, band)
    print(f"[dtw] band {band}, dim {dim}, {Ta} x {Tb}: twin={cost64} device={cost} L={len(path)} (twin {len(path64)})")
    R.check_path(path, Ta, Tb, band)
    assert cost == cost64 and np.array_equal(path, path64)


@pytest.mark.parametrize("dim,Ta,Tb,band", [(24, 1100, 1000, 8), (40, 700, 600, 2)])
def test_dtw_band_over_several_passes_random(N, dim, Ta, Tb, band):
    rng = np.random.default_rng([dim, Ta, Tb, band, 7])
    a, b = rng.standard_normal((Ta, dim)).astype(np.float32), rng.standard_normal((Tb, dim)).astype(np.float32)
    cost64, _ = R.dtw(a, b, band)
    cost, path = _raw_dtw(N, a, b, band)
    print(f"[dtw] band {band}, dim {dim}, {Ta} x {Tb}: rel err={rel(cost, cost64):.3g}")
    assert rel(cost, cost64) <= 1e-12
    R.check_path(path, Ta, Tb, band)
    assert rel(R.path_cost(a, b, path), cost64) <= 1e-12


def test_dtw_size_cap_closed_form(N):
    ramp = np.arange(16384, dtype=np.float32)[:, None]
    cost, path = _raw_dtw(N, ramp, ramp)
    print(f"[dtw] 16384 x 16384 ramp: cost={cost} L={len(path)}")
    assert cost == 0.0 and len(path) == 16384
    assert np.array_equal(path[:, 0], np.arange(16384)) and np.array_equal(path[:, 1], np.arange(16384))


def test_dtw_two_calls_identical_bits(N):
    a, b, _, _ = _dtw_ref(257, 200, None)
    c1, p1 = _raw_dtw(N, a, b)
    c2, p2 = _raw_dtw(N, a, b)
    assert np.float64(c1).tobytes() == np.float64(c2).tobytes() and np.array_equal(p1, p2)


def test_dtw_python_interface(M):
    a, b, cost64, _ = _dtw_ref(63, 65, None)
    cost, path = M.dtw(a, torch.as_tensor(b, device=DEV))
    assert rel(cost, cost64) <= 1e-12 and path.dtype == torch.int32 and path.is_cuda
    R.check_path(path.cpu().numpy(), 63, 65)
    with pytest.raises(ValueError):
        M.dtw(a, b, band=0)


# ---- F0 sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F0_CASES)
def test_f0_sums_against_twin(N, M, n):
    fa, fb = R.contour_pair(n, 3)
    if n == 1:
        fa, fb = np.array([220.0]), np.array([246.0])
    ref, dev = R.f0_sums(fa, fb), _raw_f0(N, fa, fb)
    worst = max(rel(dev[k], ref[k]) for k in range(1, 8))
    print(f"[f0] n={n}: counts twin={ref[[0, 8, 9, 10, 11]]} device={dev[[0, 8, 9, 10, 11]]}; worst sum rel err={worst:.3g}")
    assert np.array_equal(dev[[0, 8, 9, 10, 11]], ref[[0, 8, 9, 10, 11]])
    for k in range(1, 8):
        assert rel(dev[k], ref[k]) <= 1e-12, k
    want, got = R.f0_errors(fa, fb), M.f0_tracking_errors(fa, fb, device=DEV)
    for key in ("voiced_frames", "vuv_error", "gross_pitch_error"):
        assert got[key] == pytest.approx(want[key], abs=1e-15), key
    for key in ("shift_semitones", "f0_rmse_cents") + (("f0_corr",) if n > 1 else ()):
        assert got[key] == pytest.approx(want[key], rel=1e-9, abs=1e-9), key


def test_f0_identities(M):
    a, _ = R.contour_pair(1025, 5)
    r = M.f0_tracking_errors(a, a * 2.0 ** (3.0 / 12.0), device=DEV)
    print(f"[f0] a against a * 2^(3/12): {r}")
    assert r["shift_semitones"] == pytest.approx(3.0, abs=1e-9) and r["f0_rmse_cents"] <= 1e-6 and r["f0_corr"] == pytest.approx(1.0, abs=1e-9)
    assert r["vuv_error"] == 0 and r["gross_pitch_error"] == 0 and r["voiced_frames"] == int((np.nan_to_num(a) > 0).sum())
    none = M.f0_tracking_errors(np.zeros(63), np.full(63, np.nan), device=DEV)
    assert none["voiced_frames"] == 0 and none["vuv_error"] == 0 and math.isnan(none["f0_rmse_cents"])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vowels():
    xa, xb = R.vowel_sequence(R.DUR_A).astype(np.float32), R.vowel_sequence(R.DUR_B, seed=1).astype(np.float32)
    ca, cb = R.melcep(xa, 16000), R.melcep(xb, 16000)
    return xa, xb, ca, cb, R.mcd_dtw(ca, cb), R.mcd_aligned(ca, cb)


def test_mel_cepstral_distortion_end_to_end(N, M):
    xa, xb, ca, cb, twin_dtw, twin_aligned = _vowels()
    assert len(xa) == 17600 and len(xb) == 18400
    e_ref, gate = _cep_gate()
    dev_dtw = M.mel_cepstral_distortion(xa, xb, 16000, device=DEV)
    dev_aligned = M.mel_cepstral_distortion(xa, xb, 16000, align=None, device=DEV)
    da, db = M.mel_cepstra(xa, 16000, device=DEV), M.mel_cepstra(xb, 16000, device=DEV)
    own = R.mcd_dtw(da.cpu().numpy(), db.cpu().numpy())
    bound = R.MCD_CONST * 2 * math.sqrt(24) * gate
    print(f"[mcd] twin: dtw {twin_dtw:.6f} dB, aligned {twin_aligned:.6f} dB; device: dtw {dev_dtw:.6f} dB, aligned {dev_aligned:.6f} dB; "
          f"|aligned - twin|={abs(dev_aligned - twin_aligned):.3g} (bound {bound:.3g}); twin DTW on the device's cepstra {own:.15g}, "
          f"rel {rel(dev_dtw, own):.3g}")
    assert twin_dtw < 0.5 * twin_aligned
    assert dev_dtw < 0.5 * dev_aligned
    assert M.mel_cepstral_distortion(xa, xa, 16000, device=DEV) == 0.0
    assert M.mel_cepstral_distortion(xa, xa, 16000, align=None, device=DEV) == 0.0
    assert abs(dev_aligned - twin_aligned) <= bound
    assert rel(dev_dtw, own) <= 1e-12
    T = min(len(ca), len(cb))
    raw = _raw_dist(N, da.cpu().numpy(), db.cpu().numpy(), T)
    assert rel(R.MCD_CONST * raw / T, dev_aligned) <= 1e-15


class _ShiftedSecondContour:
    """the real estimator, whose second contour is multiplied by a known ratio: a synthetic-weight RMVPE does not track pitch, so a
    known transposition can only be given to the contour, not to the audio"""

    def __init__(self, inner, ratio):
        self.inner, self.ratio, self.calls = inner, ratio, 0

    def infer_from_audio(self, audio, thred=0.03):
        self.calls += 1
        f0 = self.inner.infer_from_audio(audio, thred=thred)
        return f0 * self.ratio if self.calls == 2 else f0


def test_score_conversion(M):
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.predictors.RMVPE import RMVPE0Predictor
    from rvc_amd.lib.tools import score
    rmvpe = RMVPE0Predictor(state_dict=S.make_rmvpe_state_dict(peaked=True), device=DEV)
    x = S.synth_gated_glide(16000, seed=2)
    ratio = 2.0 ** (4.0 / 12.0)
    r = score.score_conversion((x, 16000), (x.copy(), 16000), (x[:12000], 16000), predictor=_ShiftedSecondContour(rmvpe, ratio), device=DEV)
    print(f"[score] {r}")
    assert set(score.F0_KEYS) <= set(r) and {"mcd_dtw_db", "mcd_aligned_db", "dtw_path_length", "frames"} <= set(r)
    assert r["voiced_frames"] > 0 and r["frames"] >= 100
    assert r["vuv_error"] == 0
    # The estimator runs once per signal, and two fp32 evaluations of it on the same audio need not agree to the last bit.  The
    # contour's own resolution is RMVPE's 20-cent bins; one cent is far inside it and far above fp32 noise (about 1e-7 semitones).
    assert r["shift_semitones"] == pytest.approx(4.0, abs=0.01)
    assert r["f0_rmse_cents"] <= 1.0 and r["gross_pitch_error"] == 0
    assert r["dtw_path_length"] >= 201 and math.isfinite(r["mcd_dtw_db"]) and r["mcd_dtw_db"] > 0 and r["mcd_aligned_db"] > 0
    same = score.score_conversion((x, 16000), (x, 16000), (x, 16000), predictor=rmvpe, device=DEV)
    assert abs(same["shift_semitones"]) <= 0.01 and same["vuv_error"] == 0 and same["mcd_dtw_db"] == 0 and same["mcd_aligned_db"] == 0
