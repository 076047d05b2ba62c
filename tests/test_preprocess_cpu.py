"""The dataset preprocessor without a device: the silence scan and the slice plan of rvc_amd.train.preprocess reproduce what the
reference's own PreProcess.process_audio wrote (tests/golden/preprocess_manifest.npz, make_golden_preprocess.py), the K17 entries
of the C ABI refuse every bad argument of their contract before anything touches a device, and the command line follows the
reference's argv.  The kernels themselves run in test_preprocess_gpu.py."""
import ctypes

import numpy as np
import pytest

from _preprocess_common import get_rms_numpy, signals
from conftest import load_golden

P = 0x10000          # a plausible, aligned, never dereferenced "device pointer"
RATES = (32000, 40000, 48000)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()                                    # the library may not exist yet when this file runs alone
    from rvc_amd import _native
    return _native._lib


@pytest.fixture(scope="module")
def manifest():
    return load_golden("preprocess_manifest")


def _pp(sr, tmp_path):
    from rvc_amd.train.preprocess.preprocess import PreProcess
    return PreProcess(sr, str(tmp_path / f"exp{sr}"))


def test_constants_and_derived_fields(lib, tmp_path):
    from rvc_amd.train.preprocess import preprocess as T
    assert (T.OVERLAP, T.PERCENTAGE, T.MAX_AMPLITUDE, T.ALPHA, T.HIGH_PASS_CUTOFF) == (0.3, 3.0, 0.9, 0.75, 48)
    s = _pp(40000, tmp_path).slicer
    assert (s.hop_size, s.win_size, s.min_length, s.min_interval, s.max_sil_kept) == (600, 2400, 100, 27, 33)
    assert s.threshold == 10 ** (-42 / 20.0)


@pytest.mark.parametrize("sr", RATES)
def test_slice_bounds_reproduces_the_reference_chunks(lib, manifest, tmp_path, sr):
    s = _pp(sr, tmp_path).slicer
    full, _, _ = signals(sr, int(manifest["seed"]))
    bounds = s.slice_bounds(get_rms_numpy(full, s.win_size, s.hop_size), full.size)
    assert [e - b for b, e in bounds] == manifest[f"chunks_{sr}"].tolist()
    assert all(0 <= b <= e <= full.size for b, e in bounds)
    if sr == 32000:
        assert [e - b for b, e in bounds] == [76800, 70560, 78720, 112320]


def _check_plan(pp, manifest, case, audio, mode):
    s = pp.slicer
    bounds = s.slice_bounds(get_rms_numpy(audio, s.win_size, s.hop_size), audio.size) if mode == "Automatic" else None
    plan = pp.plan_slices(audio.size, mode, float(manifest["chunk_len"]), float(manifest["overlap_len"]), bounds)
    assert [f"7_3_{i}.wav" for i, _, _ in plan] == manifest[f"{case}_names"].tolist(), case
    assert [e - b for _, b, e in plan] == manifest[f"{case}_counts"].tolist(), case
    for k, (_, b, e) in enumerate(plan):         # the ranges themselves: the float32 cast of audio[b:e] is what the reference wrote
        seg = audio[b:e].astype(np.float32).astype(np.float64)
        assert seg.sum() == pytest.approx(float(manifest[f"{case}_sums"][k]), rel=1e-12, abs=1e-12), (case, k)
        assert (seg ** 2).sum() == pytest.approx(float(manifest[f"{case}_sumsq"][k]), rel=1e-12), (case, k)
    return plan


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("mode", ["Skip", "Simple", "Automatic"])
def test_plan_slices_reproduces_the_reference_files(lib, manifest, tmp_path, sr, mode):
    full, _, _ = signals(sr, int(manifest["seed"]))
    plan = _check_plan(_pp(sr, tmp_path), manifest, f"{mode}_{sr}", full, mode)
    assert float(manifest[f"{mode}_{sr}_duration"]) == full.size / sr
    if (sr, mode) == (32000, "Automatic"):
        assert [e - b for _, b, e in plan] == [76800, 70560, 78720, 96000, 25920]


def test_plan_slices_silent_and_short(lib, manifest, tmp_path):
    sr = int(manifest["special_rate"])
    _, silent, short = signals(sr, int(manifest["seed"]))
    pp = _pp(sr, tmp_path)
    _check_plan(pp, manifest, f"silent_{sr}", silent, "Automatic")
    assert short.size <= pp.slicer.min_length and pp.slicer.slice_bounds(np.zeros(0), short.size) == [(0, short.size)]
    _check_plan(pp, manifest, f"short_{sr}", short, "Automatic")
    # no frame below the threshold: no tags, one chunk
    loud = np.full(5000, pp.slicer.threshold * 2)
    assert pp.slicer.slice_bounds(loud, 5000 * pp.slicer.hop_size) == [(0, 5000 * pp.slicer.hop_size)]
    assert pp.plan_slices(10, "Nothing", 3.0, 0.3) == []


def test_slicer_constructor_refusals(lib):
    from rvc_amd.train.preprocess.slicer import Slicer
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size is required"):
        Slicer(48000, min_length=200, min_interval=300, hop_size=20)
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size is required"):
        Slicer(48000, min_length=5000, min_interval=10, hop_size=20)
    with pytest.raises(ValueError, match="max_sil_kept >= hop_size is required"):
        Slicer(48000, max_sil_kept=10, hop_size=20)
    Slicer(48000)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def _refused(lib, name, *args):
    need = ctypes.c_size_t()
    assert lib.rvc_knn_workspace_bytes(100, 10, 768, 5, ctypes.byref(need)) != 0        # plant another call's error text
    rc = getattr(lib, name)(*args)
    msg = lib.rvc_last_error()
    assert rc != 0, (name, args, "accepted")
    assert msg.startswith(name.encode() + b": ") and len(msg) > len(name) + 2, (name, args, msg)
    return msg


def _coef(sr=48000):
    from scipy import signal
    b, a = signal.butter(5, 48, btype="high", fs=sr)
    return np.ascontiguousarray(np.concatenate([b, a]))


def test_lfilter_refusals_and_warmup_rule(lib):
    from scipy import signal
    c = _coef()
    cp = c.ctypes.data

    def call(x=P, n=1000, coef=cp, y=P + 0x100000):
        return ("rvc_lfilter_order5_f64", x, n, coef, y, None)

    for kw in ({"x": None}, {"coef": None}, {"y": None}):
        assert b"null pointer" in _refused(lib, *call(**kw))
    assert b"negative" in _refused(lib, *call(n=-1))
    assert b"alias" in _refused(lib, *call(y=P))
    bad = c.copy()
    bad[6] = 2.0
    assert b"a[0] must be 1" in _refused(lib, *call(coef=bad.ctypes.data))
    unstable = np.concatenate([c[:6], [1.0, -2.5, 0, 0, 0, 0]])
    assert b"unstable" in _refused(lib, *call(coef=unstable.ctypes.data))
    nan = c.copy()
    nan[2] = np.nan
    assert b"non-finite" in _refused(lib, *call(coef=nan.ctypes.data))
    assert lib.rvc_lfilter_order5_f64(P, 0, cp, P + 8, None) == 0, lib.rvc_last_error()      # n == 0: nothing launched
    # the warm-up is sized from the pole radius of the coefficients handed in: smallest multiple of 32 with rho^warm <= 2^-53
    warm = ctypes.c_int64()
    for sr in (16000, 32000, 40000, 48000):
        b, a = signal.butter(5, 48, btype="high", fs=sr)
        coef = np.ascontiguousarray(np.concatenate([b, a]))
        assert lib.rvc_lfilter_order5_warmup(coef.ctypes.data, ctypes.byref(warm)) == 0, lib.rvc_last_error()
        rho = np.abs(np.roots(a)).max()
        want = int(np.ceil(-53 * np.log(2) / np.log(rho)))
        assert warm.value % 32 == 0 and want <= warm.value < want + 32 + want * 1e-4, (sr, rho, warm.value, want)
    _refused(lib, "rvc_lfilter_order5_warmup", None, ctypes.byref(warm))
    _refused(lib, "rvc_lfilter_order5_warmup", cp, None)


def test_frame_rms_refusals(lib):
    frames, need = ctypes.c_int64(), ctypes.c_size_t()
    for n, f, h in [(-1, 4, 1), (10, 0, 1), (10, -3, 1), (10, 4, 0), (10, 4, -2)]:
        _refused(lib, "rvc_frame_rms_frames", n, f, h, ctypes.byref(frames), ctypes.byref(need))
        _refused(lib, "rvc_frame_rms_f64", P, n, f, h, P, 1, P, 1 << 30, None)
    _refused(lib, "rvc_frame_rms_frames", 10, 4, 1, None, ctypes.byref(need))
    _refused(lib, "rvc_frame_rms_frames", 10, 4, 1, ctypes.byref(frames), None)
    # the frame count is the reference's formula, by floor division
    for n, f, h in [(1, 4, 1), (479, 1920, 480), (480 * 7 + 1, 1920, 480), (5000, 2880, 720), (4097, 7, 3), (0, 4, 2), (0, 7, 3), (2, 7, 3),
                    (172_800_000, 2880, 720)]:
        assert lib.rvc_frame_rms_frames(n, f, h, ctypes.byref(frames), ctypes.byref(need)) == 0, lib.rvc_last_error()
        assert frames.value == max(0, (n + 2 * (f // 2) - f) // h + 1), (n, f, h, frames.value)
    assert lib.rvc_frame_rms_frames(5000, 2880, 720, ctypes.byref(frames), ctypes.byref(need)) == 0
    nf, ws = frames.value, need.value

    def call(x=P, n=5000, f=2880, h=720, out=P, frames=nf, w=P, wb=ws):
        return ("rvc_frame_rms_f64", x, n, f, h, out, frames, w, wb, None)

    for kw in ({"x": None}, {"out": None}, {"w": None}):
        assert b"null pointer" in _refused(lib, *call(**kw))
    assert b"workspace too small" in _refused(lib, *call(wb=ws - 1))
    assert b"workspace too small" in _refused(lib, *call(wb=0))
    assert b"n_frames" in _refused(lib, *call(frames=nf + 1))
    assert lib.rvc_frame_rms_f64(P, 0, 7, 3, P, 0, P, 1 << 20, None) == 0, lib.rvc_last_error()     # no frame: nothing launched


def test_slice_export_refusals(lib):
    tab = np.array([[0, 10], [5, 25]], np.int64)

    def call(x=P, n=100, bounds=tab, seg=P, of=P, ol=P, n_seg=2, up=1, down=3, h=P, taps=661, full=P, n_full=30, lo=P, n_lo=11):
        return ("rvc_slice_export_f32", x, n, None if bounds is None else bounds.ctypes.data, seg, of, ol, n_seg, up, down, h, taps,
                full, n_full, lo, n_lo, None)

    for kw in ({"x": None}, {"bounds": None}, {"seg": None}, {"of": None}, {"ol": None}, {"h": None}, {"full": None}, {"lo": None}):
        assert b"null pointer" in _refused(lib, *call(**kw))
    assert b"negative" in _refused(lib, *call(n=-1))
    _refused(lib, *call(n_seg=-1))
    for kw in ({"up": 0}, {"down": 0}, {"up": -1}, {"down": -2}):
        assert b"at least 1" in _refused(lib, *call(**kw))
    for taps in (660, 0, -1, 2):
        assert b"odd" in _refused(lib, *call(taps=taps))
    assert b"negative" in _refused(lib, *call(bounds=np.array([[-1, 10], [5, 25]], np.int64)))
    assert b"negative" in _refused(lib, *call(bounds=np.array([[0, 10], [-7, -2]], np.int64)))
    assert b"reversed" in _refused(lib, *call(bounds=np.array([[0, 10], [25, 5]], np.int64)))
    assert b"ends past" in _refused(lib, *call(bounds=np.array([[0, 10], [5, 101]], np.int64)))
    assert b"packed outputs" in _refused(lib, *call(n_full=29))
    assert b"packed outputs" in _refused(lib, *call(n_lo=10))
    assert b"packed outputs" in _refused(lib, *call(n_lo=12))
    empty = np.array([[7, 7]], np.int64)                                  # nothing to write: status 0, nothing launched
    assert lib.rvc_slice_export_f32(P, 100, empty.ctypes.data, P, P, P, 1, 1, 3, P, 661, P, 0, P, 0, None) == 0, lib.rvc_last_error()


def test_native_wrappers_refuse_host_tensors(lib):
    import torch
    from rvc_amd import _native
    x = torch.zeros(100, dtype=torch.float64)
    b, a = _coef()[:6], _coef()[6:]
    with pytest.raises(_native.NativeError, match="HBM"):
        _native.lfilter_order5(x, b, a)
    with pytest.raises(_native.NativeError, match="HBM"):
        _native.frame_rms(x, 4, 1)
    with pytest.raises(_native.NativeError, match="HBM"):
        _native.slice_export(x, [(0, 10)], 1, 3, torch.zeros(661, dtype=torch.float64))
    with pytest.raises(_native.NativeError, match="HBM"):
        _native.lfilter_order5(np.zeros(10), b, a)
    with pytest.raises(_native.NativeError, match=r"b\[6\], a\[6\]"):
        _native.lfilter_warmup(b[:5], a)


# ---- the tool -------------------------------------------------------------------------------------------------------------
def test_noise_reduction_is_refused_before_any_file_is_read(lib, tmp_path, monkeypatch):
    from rvc_amd.train.preprocess import preprocess as T

    def boom(*a, **k):
        raise AssertionError("nothing may be read or walked when noise reduction is asked for")

    monkeypatch.setattr(T, "load_audio", boom)
    monkeypatch.setattr(T, "find_files", boom)
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.wav").write_bytes(b"not a wav")
    with pytest.raises(NotImplementedError, match="noise reduction"):
        T.preprocess_training_set(str(tmp_path / "in"), 48000, 4, str(tmp_path / "exp"), "Automatic", True, True, 0.7, 3.0, 0.3)
    assert not (tmp_path / "exp").exists()


def test_find_files_follows_the_reference_walk(lib, tmp_path, capsys):
    from rvc_amd.train.preprocess import preprocess as T
    root = tmp_path / "in"
    (root / "3").mkdir(parents=True)
    (root / "bob").mkdir()
    for p in (root / "a.WAV", root / "notes.txt", root / "3" / "b.flac", root / "3" / "c.wav", root / "bob" / "d.wav"):
        p.write_bytes(b"")
    files = T.find_files(str(root))
    assert sorted((str(p)[len(str(root)) + 1:], sid) for p, _, sid in files) == [("3/b.flac", 3), ("3/c.wav", 3), ("a.WAV", 0)]
    assert sorted(i for _, i, _ in files) == [0, 1, 2]
    assert 'Speaker ID folder is expected to be integer, got "bob" instead.' in capsys.readouterr().out


def test_save_dataset_duration_merges(lib, tmp_path):
    import json
    from rvc_amd.train.preprocess import preprocess as T
    path = tmp_path / "model_info.json"
    path.write_text(json.dumps({"model_name": "voice"}))
    T.save_dataset_duration(str(path), 3725.5)
    assert json.loads(path.read_text()) == {"model_name": "voice", "total_dataset_duration": "01:02:05", "total_seconds": 3725.5}


def test_strtobool_and_argv(lib, monkeypatch):
    from rvc_amd.train.preprocess import preprocess as T
    assert [T.strtobool(v) for v in ("y", "YES", "t", "True", "on", "1")] == [1] * 6
    assert [T.strtobool(v) for v in ("n", "No", "f", "FALSE", "off", "0")] == [0] * 6
    for v in ("", "2", "maybe"):
        with pytest.raises(ValueError, match="invalid truth value"):
            T.strtobool(v)
    argv = ["logs/voice", "data/in", "40000", "8", "Automatic", "True", "False", "0.7", "3.0", "0.3"]
    want = dict(exp_dir="logs/voice", input_root="data/in", sr=40000, num_processes=8, cut_preprocess="Automatic", process_effects=1,
                noise_reduction=0, reduction_strength=0.7, chunk_len=3.0, overlap_len=0.3)
    assert T.parse_args(argv) == want
    assert T.parse_args(argv[:3] + ["None"] + argv[4:])["num_processes"] >= 1
    with pytest.raises(SystemExit):
        T.parse_args(argv[:9])
    seen = []
    monkeypatch.setattr(T, "preprocess_training_set", lambda **kw: seen.append(kw))
    assert T.main(argv) == 0 and seen == [want]
