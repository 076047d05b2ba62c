"""K23 (the audio analyzer's spectral features, csrc/specfeat.hip) on the device against tests/spectral_features_ref.py.

The gate for centroid, bandwidth, magnitudes and dB is K18 / K19's rule: e_ref = max |r32 - r64| of the restatement's own two
paths for that quantity, and the device must stay within 16 e_ref of r64 (a 2048-term fp32 dot product grows rounding about
sqrt(2048) / log2(2048) ~ 4 times faster than the FFT; 16 leaves the factor-of-four room K19 took).  The roll-off is a bin index:
a frame is decidable when its float64 margin min_k |cumsum_k - roll_percent s0| / s0 is at least 16 e_cs, e_cs the largest
|cumsum32 - cumsum64| / s0 of the restatement's two paths; on decidable frames the bin must be equal, on the others it may differ by
one.  Every case first asserts, on the restatement alone, that at least 90 % of its frames are decidable.  Every ratio is printed
before it is asserted (pytest -s shows them).

e_ref has a floor: where the two paths of the restatement see identical magnitudes (n = 1: the lone sample sits on window position
1024, its spectrum is +-x[0] exactly in either precision) their float64 sums are the same expression and e_ref is 0, although a
1025-term float64 sum is only defined up to 1025 eps of its size -- NumPy adds pairwise, the device in bin order.  e_ref is
therefore never taken below 1025 * 2^-52 * max |r64| (2e-9 Hz for the curves, against 1e-4 Hz wherever the paths differ).
"""
import os
import wave

import numpy as np
import pytest
import torch

import spectral_features_ref as R
from formant_shift_ref import test_signal as _test_signal

pytestmark = pytest.mark.gpu
GATE = 16.0
FLOOR = 1025 * np.finfo(np.float64).eps
TILE, GROUP = 32, 4096            # frames per workgroup and per launch group of csrc/specfeat.hip


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def signal(n, sr=22050):
    """formant_shift_ref.test_signal at the case's rate; a single sample has no peak to normalise by (0 / 0), so n = 1 is the first
    sample of two"""
    return _test_signal(max(n, 2), sr)[:n].astype(np.float32)


_refs = {}


def refs(key, x, sr, p):
    """(r32, r64) of the restatement for the case `key`, computed once"""
    if key not in _refs:
        _refs[key] = (R.features(x, sr, p, db=True), R.features(x.astype(np.float64), sr, p, db=True))
    return _refs[key]


def check(native, key, x, sr=22050, p=0.85):
    """One call with both planes against the restatement; -> the device outputs as NumPy and r64"""
    r32, r64 = refs(key, x, sr, p)
    e_cs = np.abs(r32["cumn"] - r64["cumn"]).max()
    decidable = r64["margin"] >= GATE * e_cs
    print(f"[{key}] frames {len(decidable)}, e_cs {e_cs:.3e}, smallest margin {r64['margin'].min():.3e}, decidable {decidable.mean():.3f}")
    assert decidable.mean() >= 0.9
    assert (r32["rolloff_bin"][decidable] == r64["rolloff_bin"][decidable]).all()

    cent, bw, ro, mag, db = (v.cpu().numpy() for v in native.spectral_features(torch.from_numpy(x).cuda(), sr, p, want_mag=True, want_db=True))
    F = 1 + len(x) // 512
    assert cent.shape == bw.shape == ro.shape == (F,) and mag.shape == db.shape == (F, 1025)
    assert cent.dtype == bw.dtype == ro.dtype == np.float64 and mag.dtype == db.dtype == np.float32
    out = {"cent": cent, "bw": bw, "mag": mag, "db": db}
    for q, v in out.items():
        assert np.isfinite(v).all(), q
    worst = {}
    for q, v in out.items():
        e_ref = max(np.abs(r32[q].astype(np.float64) - r64[q]).max(), FLOOR * np.abs(r64[q]).max())
        err = np.abs(v.astype(np.float64) - r64[q]).max()
        worst[q] = err / e_ref if e_ref > 0 else (0.0 if err == 0 else np.inf)
        print(f"[{key}] {q}: e_ref {e_ref:.3e}, device error {err:.3e}, ratio {worst[q]:.2f} (gate {GATE:g})")
    for q in out:
        assert worst[q] <= GATE, (q, worst[q])

    f = np.arange(1025) * sr / 2048
    bins = np.rint(ro * 2048 / sr).astype(int)
    assert (bins >= 0).all() and (bins <= 1024).all() and (ro == f[bins]).all()       # k sr / 2048 is exact in float64
    d = np.abs(bins - r64["rolloff_bin"])
    print(f"[{key}] roll-off: {int((d[decidable] != 0).sum())} of {int(decidable.sum())} decidable frames differ, "
          f"largest difference on the others {int(d[~decidable].max()) if (~decidable).any() else 0} bins")
    assert (d[decidable] == 0).all() and (d <= 1).all()
    return out | {"rolloff": ro}, r64


@pytest.mark.parametrize("n", [1, 511, 512, 1023, 1024, 2047, 2048, 2049])
def test_short_signals(native, n):
    """One frame of almost only padding up to the first frame free of padding"""
    check(native, f"n={n}", signal(n))


@pytest.mark.parametrize("frames", [TILE - 1, TILE, TILE + 1])
def test_frames_around_one_tile(native, frames):
    check(native, f"F={frames}", signal((frames - 1) * 512 + 100))


def test_group_walk(native):
    """One launch group plus one frame"""
    n = GROUP * 512
    assert 1 + n // 512 == GROUP + 1
    check(native, "group+1", signal(n))


def test_48k(native):
    check(native, "48k", signal(24000, 48000), sr=48000)


@pytest.mark.parametrize("p", [0.01, 0.85, 0.99])
def test_roll_percent(native, p):
    check(native, f"p={p}", signal(22050), p=p)


def test_zeros_in_the_middle(native):
    x = signal(22050)
    x[8000:12096] = 0
    out, r64 = check(native, "zeros", x)
    silent = np.flatnonzero(r64["s0"] == 0)
    assert len(silent) >= 4
    for q in ("cent", "bw", "rolloff"):
        assert not out[q][silent].any() and out[q][np.setdiff1d(np.arange(len(r64["s0"])), silent)].all()
    assert not out["mag"][silent].any() and (out["db"][silent] == -80).all()


def test_all_zero_signal(native):
    out, _ = check(native, "silence", np.zeros(3000, np.float32))
    for q in ("cent", "bw", "rolloff", "mag", "db"):
        assert not out[q].any(), q


def test_the_80_db_floor(native):
    """A loud second followed by the same signal times 1e-6 (-120 dB): the quiet half sits on the floor"""
    loud = signal(22050)
    x = np.concatenate([loud, loud * np.float32(1e-6)])
    r32, r64 = refs("floor", x, 22050, 0.85)
    assert r64["db"].max() == 0 and (r64["db"] == r64["db"].max() - 80).mean() > 0.1
    out, _ = check(native, "floor", x)
    assert out["db"].max() == 0 and out["db"].min() == -80 and (out["db"] == -80).mean() > 0.1


def _bits(outs):
    return [None if v is None else v.cpu().numpy().tobytes() for v in outs]


def test_planes_do_not_change_the_curves_and_calls_repeat(native):
    x = torch.from_numpy(signal(40000)).cuda()
    both = _bits(native.spectral_features(x, 22050, 0.85, want_mag=True, want_db=True))
    assert _bits(native.spectral_features(x, 22050, 0.85, want_mag=True, want_db=True)) == both       # two calls: identical bits
    mag_only = native.spectral_features(x, 22050, 0.85, want_mag=True)
    db_only = native.spectral_features(x, 22050, 0.85, want_db=True)
    neither = native.spectral_features(x, 22050, 0.85)
    assert mag_only[4] is None and db_only[3] is None and neither[3] is None and neither[4] is None
    assert _bits(mag_only)[:4] == both[:4]
    assert _bits(db_only)[:3] == both[:3] and _bits(db_only)[4] == both[4]
    assert _bits(neither)[:3] == both[:3]
    assert _bits(native.spectral_features(x, 22050, 0.85)) == _bits(neither)


def test_side_stream(native):
    x = torch.from_numpy(signal(40000)).cuda()
    want = _bits(native.spectral_features(x, 22050, 0.5, want_mag=True, want_db=True))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = native.spectral_features(x, 22050, 0.5, want_mag=True, want_db=True)
    side.synchronize()
    assert _bits(got) == want


def test_numpy_in_numpy_out_tensor_in_tensor_out(native):
    from rvc_amd.lib.tools import analyzer as Z
    x = signal(6000)
    stft, duration, cent, bw, rolloff = Z.calculate_features(x, 22050)
    assert all(isinstance(v, np.ndarray) for v in (stft, cent, bw, rolloff))
    assert stft.shape == (1025, 12) and stft.dtype == np.float32 and cent.dtype == np.float64 and duration == 6000 / 22050
    xt = torch.from_numpy(x).cuda()
    stft_t, duration_t, cent_t, bw_t, rolloff_t = Z.calculate_features(xt, 22050)
    assert all(torch.is_tensor(v) and v.device == xt.device for v in (stft_t, cent_t, bw_t, rolloff_t)) and duration_t == duration
    assert stft_t.shape == (1025, 12) and not stft_t.is_contiguous()                 # a transposed view of the frame-major plane
    assert np.array_equal(stft_t.cpu().numpy(), stft) and np.array_equal(cent_t.cpu().numpy(), cent)
    assert np.array_equal(bw_t.cpu().numpy(), bw) and np.array_equal(rolloff_t.cpu().numpy(), rolloff)
    assert np.array_equal(Z.calculate_features(x.astype(np.float64), 22050)[2], cent)       # float64 NumPy is taken to float32

    got = Z.spectral_features(x, 22050, roll_percent=0.5, db=True)
    assert sorted(got) == ["bw", "cent", "db", "rolloff"] and all(isinstance(v, np.ndarray) for v in got.values())
    assert got["db"].shape == (1025, 12) and np.array_equal(got["cent"], cent) and (got["rolloff"] <= rolloff).all()
    got_t = Z.spectral_features(xt, 22050)
    assert sorted(got_t) == ["bw", "cent", "rolloff"] and all(v.device == xt.device for v in got_t.values())
    assert np.array_equal(got_t["rolloff"].cpu().numpy(), rolloff)


def test_analyze_audio_on_a_wav(native, tmp_path):
    from rvc_amd.lib.tools import analyzer as Z
    path = str(tmp_path / "second.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(48000)
        f.writeframes((signal(48000, 48000) * 32767.0).astype("<i2").tobytes())
    info, out = Z.analyze_audio(path, None)
    assert out is None
    assert info == "Sample Rate: 22050\nDuration: 1.0 seconds\nNumber of Samples: 22050\nBits per Sample: 48000\nChannels: Mono (1)"
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    png = str(tmp_path / "second.png")
    info2, out = Z.analyze_audio(path, png)
    assert info2 == info and out == png and os.path.getsize(png) > 0
