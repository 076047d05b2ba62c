"""K17 (csrc/preprocess.hip) and the dataset preprocessor built on it (rvc_amd.train.preprocess) on the device: the three kernels
against float64 NumPy / SciPy at bounds derived from the arithmetic, the slicer and the whole tool against what the reference's
own PreProcess.process_audio wrote (tests/golden/preprocess_manifest.npz), and the effects-on path teacher-forced on the
device's own filtered audio (its slice integers are not robust to the filter's 1e-6-level noise floor: DESIGN.md)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

from _preprocess_common import get_rms_numpy, signals
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LF_CHUNK = 2048          # csrc/preprocess.hip


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def manifest():
    return load_golden("preprocess_manifest")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _butter(sr):
    return signal.butter(N=5, Wn=48, btype="high", fs=sr)


# ---- 1. frame_rms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,frame,hop", [(1, 4, 1), (479, 1920, 480), (480 * 7 + 1, 1920, 480), (5000, 2880, 720), (4097, 7, 3)])
def test_frame_rms_matches_numpy(native, n, frame, hop):
    x = np.random.default_rng(n).standard_normal(n) * 0.3
    if n > 4 * frame:
        x[: 2 * frame] = 0.0                      # whole frames of zeros at the front (the left padding included)
    want = get_rms_numpy(x, frame, hop)
    xd = _dev(x)
    got_d = native.frame_rms(xd, frame, hop)
    got = got_d.cpu().numpy()
    assert got.shape == want.shape == ((n + 2 * (frame // 2) - frame) // hop + 1,)
    err = np.abs(got - want)
    print(f"frame_rms n={n} frame={frame} hop={hop}: {got.size} frames, max err / bound = {np.max(err / np.maximum(frame * 2.0 ** -52 * want, 1e-300)):.3f}")
    # a mean of `frame` squares summed in any order, then one square root
    assert (err <= frame * 2.0 ** -52 * want).all()
    assert (got[want == 0.0] == 0.0).all()
    if n > 4 * frame:
        assert (want == 0.0).sum() >= 1
    assert torch.equal(native.frame_rms(xd, frame, hop), got_d)         # no atomics: the same bits again


def test_frame_rms_all_zero_and_empty(native):
    assert (native.frame_rms(_dev(np.zeros(5000)), 1920, 480).cpu().numpy() == 0.0).all()
    assert native.frame_rms(_dev(np.zeros(0)), 4, 2).cpu().numpy().tolist() == [0.0]
    assert native.frame_rms(_dev(np.zeros(0)), 7, 3).numel() == 0


# ---- 2. lfilter -------------------------------------------------------------------------------------------------------------
def _lfilter_gate(b, a, x, s=100000, W=65536):
    """4 x the reference's own noise floor on this input: two runs of scipy.signal.lfilter started W samples apart."""
    y = signal.lfilter(b, a, x)
    floor = np.abs(y[s:] - signal.lfilter(b, a, x[s - W:])[W:]).max()
    return y, floor, 4.0 * floor


@pytest.fixture(scope="module")
def lfilter_case():
    x = 0.1 * np.random.default_rng(7).standard_normal(200003) + 0.05
    out = {}
    for sr in (32000, 48000):
        b, a = _butter(sr)
        out[sr] = (b, a, x) + _lfilter_gate(b, a, x)
    return out


@pytest.mark.parametrize("sr", [32000, 48000])
def test_lfilter_matches_scipy(native, lfilter_case, sr):
    b, a, x, want, floor, gate = lfilter_case[sr]
    got = native.lfilter_order5(_dev(x), b, a).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"lfilter sr={sr}: floor {floor:.3e}, gate {gate:.3e}, max|y| {np.abs(want).max():.3f}, max err {err:.3e}, "
          f"warm-up {native.lfilter_warmup(b, a)}")
    assert gate <= 1e-4 * np.abs(want).max()                      # the gate cannot hide a failure
    assert err <= gate
    warm = native.lfilter_warmup(b, a)
    assert np.array_equal(got[: LF_CHUNK], want[: LF_CHUNK])      # the first chunk starts from the true zero state: SciPy's bits
    # short inputs, one chunk, one chunk plus a sample: every chunk's warm-up reaches sample 0, the same operations as SciPy's
    for n in (1, 5, 1000, LF_CHUNK, LF_CHUNK + 1):
        g = native.lfilter_order5(_dev(x[:n]), b, a).cpu().numpy()
        assert g.shape == (n,) and np.abs(g - want[:n]).max() <= gate, n
        assert np.array_equal(g, want[:n]), n
    assert native.lfilter_order5(_dev(x[:0]), b, a).numel() == 0
    # DC alone has died away after the warm-up length
    dc = native.lfilter_order5(_dev(np.full(warm + 3 * LF_CHUNK + 5, 0.05)), b, a).cpu().numpy()
    print(f"lfilter sr={sr}: DC residue after {warm} samples {np.abs(dc[warm:]).max():.3e}")
    assert np.abs(dc[warm:]).max() <= gate
    assert abs(dc[0] - b[0] * 0.05) == 0.0


# ---- 3. slice_export --------------------------------------------------------------------------------------------------------
def _resample_want(seg, up, down, h):
    """float64 scipy.signal.upfirdn cut to y[j] = sum_m h[m] xup[j * down + (n_taps - 1) / 2 - m], j < ceil(len * up / down)
    (scipy.signal.resample_poly's own pre-padding of the filter)."""
    centre = (len(h) - 1) // 2
    pre = down - centre % down
    skip = (centre + pre) // down
    n_out = -(-len(seg) * up // down)
    y = signal.upfirdn(np.concatenate([np.zeros(pre), h]), seg, up, down)
    y = np.concatenate([y, np.zeros(max(0, skip + n_out - len(y)))])
    return y[skip: skip + n_out]


@pytest.mark.parametrize("sr", [32000, 40000, 48000])
def test_slice_export_matches_scipy(native, sr):
    from rvc_amd.lib import audio as A
    g = math.gcd(sr, 16000)
    up, down = 16000 // g, sr // g
    assert (up, down) == {32000: (1, 2), 40000: (2, 5), 48000: (1, 3)}[sr]
    h = A.resample_filter(up, down)
    n_taps = len(h)
    x = np.random.default_rng(3).standard_normal(40000) * 0.3
    segs = [(0, 1), (1, 3), (100, 100 + n_taps // (2 * up) - 1), (5000, 14600), (13700, 23300), (23300, 40000), (39999, 40000),
            (20011, 20011 + 9973)]
    full, lo, off_full, off_lo = native.slice_export(_dev(x), segs, up, down, _dev(h))
    full, lo = full.cpu().numpy(), lo.cpu().numpy()
    assert full.dtype == lo.dtype == np.float32
    assert off_full == np.concatenate([[0], np.cumsum([e - s for s, e in segs])]).tolist() and full.size == off_full[-1]
    assert off_lo == np.concatenate([[0], np.cumsum([-(-(e - s) * up // down) for s, e in segs])]).tolist() and lo.size == off_lo[-1]
    worst = 0.0
    for k, (s, e) in enumerate(segs):
        assert np.array_equal(full[off_full[k]: off_full[k + 1]], x[s:e].astype(np.float32)), (k, s, e)
        want = _resample_want(x[s:e], up, down, h)
        alone = A.resample(x[s:e].copy(), sr, 16000, device=DEV)                 # the project's resampler on the segment ALONE
        assert alone.shape == want.shape and np.abs(alone - want).max() <= 1e-12, (k, np.abs(alone - want).max())
        got = lo[off_lo[k]: off_lo[k + 1]].astype(np.float64)
        assert got.shape == want.shape, (k, got.shape, want.shape)
        # one float32 rounding that a float64 difference may flip, plus float64 accumulation over the taps
        bound = 2.0 ** -23 * np.abs(want) + 1e-12
        worst = max(worst, float(np.max(np.abs(got - want) / bound)))
        assert (np.abs(got - want) <= bound).all(), (k, s, e, np.max(np.abs(got - want) / bound))
    print(f"slice_export {up}/{down} ({n_taps} taps): max err / bound = {worst:.3f}")
    # a neighbour's samples must not leak in: the touching segments differ from a resampling of the file as a whole
    whole = _resample_want(x, up, down, h)
    k = 5
    j0 = -(-segs[k][0] * up // down)
    assert np.abs(lo[off_lo[k]: off_lo[k] + 8] - whole[j0: j0 + 8]).max() > 1e-3


def test_slice_export_refuses_a_negative_start_and_writes_nothing(native):
    from rvc_amd.lib import audio as A
    x = _dev(np.random.default_rng(4).standard_normal(1000))
    h = _dev(A.resample_filter(1, 3))
    with pytest.raises(native.NativeError, match="negative"):
        native.slice_export(x, [(10, 20), (-5, 30)], 1, 3, h)
    with pytest.raises(native.NativeError, match="reversed"):
        native.slice_export(x, [(30, 20)], 1, 3, h)
    # the same refusal at the C ABI, with buffers this test can look at afterwards
    tab = np.array([[10, 20], [-5, 30]], np.int64)
    off_full, off_lo = np.array([0, 10, 45], np.int64), np.array([0, 4, 16], np.int64)
    tables = torch.from_numpy(np.concatenate([tab.reshape(-1), off_full, off_lo])).to(DEV)
    full = torch.full((45,), 7.0, dtype=torch.float32, device=DEV)
    lo = torch.full((16,), 7.0, dtype=torch.float32, device=DEV)
    p = tables.data_ptr()
    rc = native._lib.rvc_slice_export_f32(x.data_ptr(), 1000, tab.ctypes.data, p, p + 32, p + 32 + 24, 2, 1, 3, h.data_ptr(), h.numel(),
                                          full.data_ptr(), 45, lo.data_ptr(), 16, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"negative" in native._lib.rvc_last_error()
    torch.cuda.synchronize()
    assert (full == 7.0).all() and (lo == 7.0).all()


# ---- 4. Slicer.slice on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [32000, 40000, 48000])
def test_slicer_on_the_device_reproduces_the_reference_chunks(native, manifest, sr):
    from rvc_amd.train.preprocess.slicer import Slicer
    s = Slicer(sr=sr, threshold=-42, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)
    full, _, short = signals(sr, int(manifest["seed"]))
    xd = _dev(full)
    chunks = s.slice(xd)
    assert [c.numel() for c in chunks] == manifest[f"chunks_{sr}"].tolist()
    assert all(c.is_cuda and c.data_ptr() >= xd.data_ptr() for c in chunks)            # views, nothing copied
    host = s.slice(full, device=DEV)
    assert [c.size for c in host] == manifest[f"chunks_{sr}"].tolist() and all(np.shares_memory(c, full) for c in host)
    assert [c.size for c in s.slice(short, device=DEV)] == [80]
    stereo = s.slice(np.stack([full, full]), device=DEV)
    assert [c.shape for c in stereo] == [(2, n) for n in manifest[f"chunks_{sr}"].tolist()]


# ---- 5. / 6. end to end, effects off ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory, manifest):
    root = tmp_path_factory.mktemp("dataset")
    seed = int(manifest["seed"])
    audio = {32000: signals(32000, seed)[0], 48000: signals(48000, seed)[0]}
    (root / "in" / "1").mkdir(parents=True)
    wavfile.write(root / "in" / "a.wav", 32000, audio[32000].astype(np.float32))
    wavfile.write(root / "in" / "1" / "b.wav", 48000, audio[48000].astype(np.float32))
    return root, audio


def _read(path):
    sr, data = wavfile.read(path)
    assert data.dtype == np.float32
    return sr, data


def _check_against_manifest(native, manifest, exp, sr, mode, prefix, audio):
    """The files `prefix`_<idx1>.wav of one run against the manifest case of (mode, sr) and against the source ranges."""
    from rvc_amd.lib import audio as A
    from rvc_amd.train.preprocess.preprocess import PreProcess
    case = f"{mode}_{sr}"
    names = sorted((f for f in os.listdir(exp / "sliced_audios") if f.startswith(prefix + "_")), key=lambda f: int(f[len(prefix) + 1:-4]))
    assert [f[len(prefix) + 1:] for f in names] == [f[len("7_3_"):] for f in manifest[f"{case}_names"].tolist()]
    pp = PreProcess(sr, str(exp), device=DEV)
    s = pp.slicer
    bounds = s.slice_bounds(get_rms_numpy(audio, s.win_size, s.hop_size), audio.size) if mode == "Automatic" else None
    plan = pp.plan_slices(audio.size, mode, 3.0, 0.3, bounds)             # pinned against the manifest by test_preprocess_cpu.py
    assert len(plan) == len(names)
    for k, name in enumerate(names):
        rate, data = _read(exp / "sliced_audios" / name)
        assert rate == sr and data.size == int(manifest[f"{case}_counts"][k])
        d = data.astype(np.float64)
        assert d.sum() == pytest.approx(float(manifest[f"{case}_sums"][k]), rel=1e-6)
        assert (d ** 2).sum() == pytest.approx(float(manifest[f"{case}_sumsq"][k]), rel=1e-6)
        b, e = plan[k][1], plan[k][2]
        assert np.array_equal(data, audio[b:e].astype(np.float32))
        rate16, lo = _read(exp / "sliced_audios_16k" / name)
        assert rate16 == 16000 and lo.size == math.ceil(data.size * 16000 / sr)
        want = A.resample(audio[b:e].copy(), sr, 16000, device=DEV)
        assert (np.abs(lo.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12).all(), name
    assert sorted(os.listdir(exp / "sliced_audios_16k")) == sorted(os.listdir(exp / "sliced_audios"))


@pytest.mark.parametrize("mode", ["Automatic", "Simple", "Skip"])
def test_end_to_end_effects_off(native, manifest, dataset, mode):
    from rvc_amd.train.preprocess.preprocess import preprocess_training_set
    root, audio = dataset
    # the walk names a.wav 0_0_* (root: speaker 0, file 0) and 1/b.wav 1_1_*; the file whose rate is the dataset's is the
    # manifest's case, the other one goes through load_audio's resampler first
    for sr, prefix in ((32000, "0_0"), (48000, "1_1")):
        exp = root / f"exp_{mode}_{sr}"
        total = preprocess_training_set(str(root / "in"), sr, 4, str(exp), mode, False, False, 0.0, 3.0, 0.3)
        _check_against_manifest(native, manifest, exp, sr, mode, prefix, audio[sr])
        other = "1_1" if prefix == "0_0" else "0_0"
        assert any(f.startswith(other + "_") for f in os.listdir(exp / "sliced_audios"))
        info = json.loads((exp / "model_info.json").read_text())
        assert float(manifest[f"{mode}_{sr}_duration"]) == 12.0
        assert info["total_seconds"] == total == 24.0 and info["total_dataset_duration"] == "00:00:24"


def test_fan_out_over_two_workers_writes_the_same_bytes(native, dataset):
    from rvc_amd.train.preprocess.preprocess import preprocess_training_set
    root, _ = dataset
    one, two = root / "fan1", root / "fan2"
    preprocess_training_set(str(root / "in"), 32000, 1, str(one), "Automatic", False, False, 0.0, 3.0, 0.3, devices=[DEV])
    preprocess_training_set(str(root / "in"), 32000, 1, str(two), "Automatic", False, False, 0.0, 3.0, 0.3, devices=[DEV, DEV])
    for sub in ("sliced_audios", "sliced_audios_16k"):
        names = sorted(os.listdir(one / sub))
        assert names == sorted(os.listdir(two / sub)) and len(names) >= 10
        for f in names:
            assert (one / sub / f).read_bytes() == (two / sub / f).read_bytes(), (sub, f)
    assert (one / "model_info.json").read_text() == (two / "model_info.json").read_text()


# ---- 7. effects on, teacher-forced ----------------------------------------------------------------------------------------------
def test_effects_on_teacher_forced(native, manifest, tmp_path):
    from rvc_amd.train.preprocess.preprocess import ALPHA, MAX_AMPLITUDE, PreProcess
    sr = 48000
    audio = (signals(sr, int(manifest["seed"]))[0] + 0.02).astype(np.float32)
    wavfile.write(tmp_path / "in.wav", sr, audio)
    audio = audio.astype(np.float64)
    pp = PreProcess(sr, str(tmp_path / "exp"), device=DEV)
    taps = {}
    assert pp.process_audio(str(tmp_path / "in.wav"), 5, 2, "Automatic", True, False, 0.0, 3.0, 0.3, debug_taps=taps) == audio.size / sr
    tapped = taps["audio"].cpu().numpy()
    # the filter and the normalisation against SciPy / NumPy, at test 2's gate recomputed on this input
    y, floor, gate = _lfilter_gate(pp.b_high, pp.a_high, audio)
    peak = np.abs(y).max()
    want = (y / peak * (MAX_AMPLITUDE * ALPHA)) + (1 - ALPHA) * y
    err = np.abs(tapped - want).max()
    print(f"effects on: floor {floor:.3e}, gate {gate:.3e}, peak {peak:.4f}, max err {err:.3e} (bound {gate * (0.675 / peak + 0.25):.3e})")
    assert err <= gate * (0.675 / peak + 0.25)
    # the slices follow from the TAPPED audio by the host logic the CPU tests pin
    s = pp.slicer
    rms = get_rms_numpy(tapped, s.win_size, s.hop_size)
    assert taps["rms"].shape == rms.shape and (np.abs(taps["rms"] - rms) <= s.win_size * 2.0 ** -52 * rms).all()
    plan = pp.plan_slices(tapped.size, "Automatic", 3.0, 0.3, s.slice_bounds(rms, tapped.size))
    assert len(plan) >= 2                                      # more than one slice, or nothing was sliced
    assert sorted(os.listdir(tmp_path / "exp" / "sliced_audios")) == sorted(f"2_5_{i}.wav" for i, _, _ in plan)
    assert sorted(os.listdir(tmp_path / "exp" / "sliced_audios_16k")) == sorted(f"2_5_{i}.wav" for i, _, _ in plan)
    for i, b, e in plan:
        rate, data = _read(tmp_path / "exp" / "sliced_audios" / f"2_5_{i}.wav")
        assert rate == sr and np.array_equal(data, tapped[b:e].astype(np.float32)), i


# ---- 8. reference behaviours --------------------------------------------------------------------------------------------------
def test_loud_and_unreadable_files(native, manifest, tmp_path, capsys):
    from rvc_amd.train.preprocess.preprocess import PreProcess
    sr = 32000
    loud = (signals(sr, int(manifest["seed"]))[0][: 3 * sr] * 20.0).astype(np.float32)       # peak ~6 after the high-pass: above 2.5
    wavfile.write(tmp_path / "loud.wav", sr, loud)
    (tmp_path / "broken.wav").write_bytes(b"RIFF\x00\x00\x00\x00junk")
    pp = PreProcess(sr, str(tmp_path / "exp"), device=DEV)
    capsys.readouterr()
    for mode in ("Skip", "Simple", "Automatic"):
        assert pp.process_audio(str(tmp_path / "loud.wav"), 4, 9, mode, True, False, 0.0, 3.0, 0.3) == 3.0
        out = capsys.readouterr().out.strip()
        assert out == "9-4-0-filtered" if mode == "Skip" else out.startswith("Error processing audio: "), (mode, out)
    assert os.listdir(tmp_path / "exp" / "sliced_audios") == [] and os.listdir(tmp_path / "exp" / "sliced_audios_16k") == []
    # with effects off the same file is written: the 2.5 limit belongs to the normalisation
    assert pp.process_audio(str(tmp_path / "loud.wav"), 4, 9, "Skip", False, False, 0.0, 3.0, 0.3) == 3.0
    assert os.listdir(tmp_path / "exp" / "sliced_audios") == ["9_4_0.wav"]
    for path in (str(tmp_path / "broken.wav"), str(tmp_path / "missing.wav"), str(tmp_path / "song.mp3")):
        assert pp.process_audio(path, 0, 0, "Automatic", True, False, 0.0, 3.0, 0.3) == 0
        assert capsys.readouterr().out.startswith("Error processing audio: ")
    assert os.listdir(tmp_path / "exp" / "sliced_audios") == ["9_4_0.wav"]
