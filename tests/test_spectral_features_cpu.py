"""K23 (the audio analyzer, csrc/specfeat.hip) without a GPU: every refusal of the C ABI comes before any device access, the
workspace does not grow with n beyond one launch group, the restatement of tests/spectral_features_ref.py meets its closed forms,
and analyze_audio / analyze_dataset do their host-side work (info string, figure, table) with the native call and the resampler
replaced by the restatement."""
import ctypes
import json
import os
import sys
import wave

import numpy as np
import pytest

import spectral_features_ref as R


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
GOOD = dict(x=1, n=4000, sr=22050, p=0.85, mag=None, db=None, cent=2, bw=3, ro=4, ws=5, ws_bytes=1 << 40)
REFUSALS = [   # (what changes, the words the error must carry)
    (dict(x=None), "null pointer"), (dict(cent=None), "null pointer"), (dict(bw=None), "null pointer"), (dict(ro=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(n=0), "at least 1"), (dict(n=-5), "at least 1"), (dict(n=(1 << 27) + 1), "exceeds"),
    (dict(sr=0), "sr 0"), (dict(sr=-22050), "sr -22050"),
    (dict(p=0.0), "roll_percent"), (dict(p=1.0), "roll_percent"), (dict(p=-0.1), "roll_percent"), (dict(p=1.5), "roll_percent"),
    (dict(p=float("nan")), "roll_percent"), (dict(p=float("inf")), "roll_percent"), (dict(p=float("-inf")), "roll_percent"),
    (dict(mag=6, db=6), "alias"),
    (dict(ws_bytes=0), "workspace too small"),
]


def _forward(native, a):
    """rvc_spectral_features_f32 on addresses that are never dereferenced: 1 .. 7 stand for host buffers the library must not touch"""
    host = (ctypes.c_float * 64)()
    ptr = lambda v: None if v is None else ctypes.addressof(host) + 16 * v
    ws_bytes = a["ws_bytes"]
    if ws_bytes == 1 << 40:   # "large enough": exactly what the query asks for
        need = ctypes.c_size_t()
        if native._lib.rvc_spectral_features_workspace_bytes(a["n"], ctypes.byref(need)) == 0:
            ws_bytes = need.value
    return native._lib.rvc_spectral_features_f32(ptr(a["x"]), a["n"], a["sr"], a["p"], ptr(a["mag"]), ptr(a["db"]), ptr(a["cent"]),
                                                 ptr(a["bw"]), ptr(a["ro"]), ptr(a["ws"]), ws_bytes, None)


@pytest.mark.parametrize("change,words", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_abi_refuses_before_any_device_access(native, change, words):
    assert _forward(native, {**GOOD, **change}) != 0
    assert words in _err(native), _err(native)


def test_abi_accepts_the_bounds_of_its_ranges_up_to_the_workspace_check(native):
    """The smallest and largest n, sr = 1, roll_percent next to either end and two distinct planes pass every argument check: the
    call then stops at the workspace size, the last refusal before the device"""
    for change in (dict(n=1), dict(n=1 << 27), dict(sr=1), dict(p=1e-300), dict(p=1 - 2.0 ** -53), dict(mag=6, db=7), dict(mag=6),
                   dict(db=6)):
        assert _forward(native, {**GOOD, **change, "ws_bytes": 0}) != 0
        assert "workspace too small" in _err(native), (change, _err(native))


def test_abi_workspace_is_one_byte_short(native):
    need = ctypes.c_size_t()
    assert native._lib.rvc_spectral_features_workspace_bytes(4000, ctypes.byref(need)) == 0
    assert need.value == 512                                  # 8 frames -> one workgroup: 256 + 4 bytes, rounded up to 256
    assert _forward(native, {**GOOD, "ws_bytes": need.value - 1}) != 0
    assert "workspace too small" in _err(native)


def test_abi_workspace_query_refusals_and_independence_of_n(native):
    lib, need = native._lib, ctypes.c_size_t()
    assert lib.rvc_spectral_features_workspace_bytes(4000, None) != 0 and "null pointer" in _err(native)
    for n, words in ((0, "at least 1"), (-1, "at least 1"), ((1 << 27) + 1, "exceeds")):
        assert lib.rvc_spectral_features_workspace_bytes(n, ctypes.byref(need)) != 0, n
        assert words in _err(native)
    sizes = {}
    for n in (1, 511, 512 * 31, 512 * 32, 512 * 4095, 512 * 4096, 30 * 48000 * 10, 1 << 27):
        assert lib.rvc_spectral_features_workspace_bytes(n, ctypes.byref(need)) == 0
        sizes[n] = need.value
    assert sizes[1] == sizes[511] == sizes[512 * 31] == 512             # up to 32 frames: one workgroup
    assert sizes[512 * 32] == 512                                       # 33 frames: two
    full = 256 + 4 * 128                                                # one group of 128 workgroups = 4096 frames
    assert sizes[512 * 4095] == sizes[512 * 4096] == sizes[30 * 48000 * 10] == sizes[1 << 27] == full


# ---- the restatement against closed forms -----------------------------------------------------------------------------------------
SR = 22050


@pytest.mark.parametrize("p", [0.01, 0.5, 0.85, 0.99])
def test_unit_impulse_has_a_flat_spectrum(p):
    """x[0] = 1 sits at position 1024 of the padded signal: frame 0 sees it at window position 1024 (w = 1), frame 1 at 512
    (w = 0.5), frame 2 at 0, where the periodic Hann window is 0 -- a frame of digital silence -- and frames 3, 4 not at all."""
    x = np.zeros(2048)
    x[0] = 1.0
    r = R.features(x, SR, p)
    f = np.arange(R.B) * SR / R.N
    assert np.abs(r["mag"][0] - 1.0).max() <= 1e-12 and np.abs(r["mag"][1] - 0.5).max() <= 1e-12
    k = int(np.argmax((np.arange(R.B) + 1) / R.B >= p))
    for t in (0, 1):
        assert abs(r["cent"][t] - SR / 4) <= 1e-9
        assert abs(r["bw"][t] - np.sqrt(np.mean((f - SR / 4) ** 2))) <= 1e-9
        assert r["rolloff_bin"][t] == k and r["rolloff"][t] == f[k]
    for t in (2, 3, 4):
        assert not r["mag"][t].any()
        assert r["cent"][t] == 0 and r["bw"][t] == 0 and r["rolloff"][t] == 0 and r["margin"][t] == np.inf


def test_bin_centred_sinusoid():
    """A tone on bin 100 under the Hann window is the bins 99, 100, 101 in the ratio 1 : 2 : 1: the cumulative sum passes a half at
    the tone and 85 % one bin above it."""
    k0 = 100
    x = np.sin(2 * np.pi * k0 * np.arange(8192) / R.N)
    mid = slice(4, 13)                                       # frames free of padding
    r50, r85 = R.features(x, SR, 0.5), R.features(x, SR, 0.85)
    assert np.abs(r50["cent"][mid] - k0 * SR / R.N).max() < SR / R.N
    assert np.abs(r50["cent"][mid] - k0 * SR / R.N).max() < 1e-6            # symmetric leakage: in fact on the tone
    assert (r50["rolloff_bin"][mid] == k0).all() and (r85["rolloff_bin"][mid] == k0 + 1).all()
    # sqrt(0.25 + 0.25) bins; the rounding floor of the other 1022 bins (1e-16 of the peak each, up to 11 kHz away) moves it by 1e-6 Hz
    assert np.abs(r50["bw"][mid] - np.sqrt(0.5) * SR / R.N).max() < 1e-4


def test_silence():
    x = np.concatenate([np.zeros(4096), R_signal(4096)])
    r = R.features(x, SR, db=True)
    for key in ("cent", "bw", "rolloff"):
        assert np.isfinite(r[key]).all() and not r[key][:6].any() and r[key][7:].all()      # frame 6 ends at sample 4096
    assert np.isfinite(r["db"]).all() and r["db"].max() == 0 and r["db"].min() == -80
    for dt in (np.float32, np.float64):
        r = R.features(np.zeros(3000, dt), SR, db=True)
        assert r["db"].dtype == dt and not r["db"].any() and not r["cent"].any() and not r["bw"].any() and not r["rolloff"].any()


def R_signal(n, sr=SR):
    from formant_shift_ref import test_signal
    return test_signal(max(n, 2), sr)[:n]        # a single sample has no peak to normalise by: 0 / 0


@pytest.mark.parametrize("n,frames", [(1, 1), (511, 1), (512, 2), (2048, 5)])
def test_frame_count(n, frames):
    r = R.features(R_signal(n), SR)
    assert r["mag"].shape == (frames, 1025) and r["cent"].shape == r["bw"].shape == r["rolloff"].shape == (frames,)


def test_float32_input_runs_in_float32():
    x = R_signal(22050)
    a, b = R.features(x.astype(np.float32), SR, db=True), R.features(x.astype(np.float32).astype(np.float64), SR, db=True)
    assert a["mag"].dtype == np.float32 and a["db"].dtype == np.float32 and b["mag"].dtype == np.float64
    assert 1e-6 < np.abs(a["cent"] - b["cent"]).max() < 1e-2
    assert (a["rolloff_bin"] == b["rolloff_bin"]).all()


# ---- the analyzer's host side (the native call and the resampler replaced by the restatement) -------------------------------------
def test_info_string_is_the_reference_text():
    from rvc_amd.lib.tools.analyzer import format_audio_info
    assert format_audio_info(22050, 272220 / 22050, 272220, 48000) == (
        "Sample Rate: 22050\nDuration: 12.35 seconds\nNumber of Samples: 272220\nBits per Sample: 48000\nChannels: Mono (1)")
    assert format_audio_info(22050, 90.0, 1984500, 44100) == (
        "Sample Rate: 22050\nDuration: 1.5 minutes\nNumber of Samples: 1984500\nBits per Sample: 44100\nChannels: Mono (1)")
    assert "Duration: 59.99 seconds" in format_audio_info(22050, 59.994, 1, 1)
    assert "Duration: 1.0 minutes" in format_audio_info(22050, 60.0, 1, 1)


def _wav(path, x, sr):
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes((np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())
    return str(path)


@pytest.fixture()
def stubbed(native, monkeypatch):
    """rvc_amd.lib.tools.analyzer with _native.spectral_features and audio.resample answered on the host; -> (module, calls)"""
    from scipy import signal
    from rvc_amd.lib import audio as A
    from rvc_amd.lib.tools import analyzer as Z
    calls = []

    def features(x, sr, roll_percent=0.85, want_mag=False, want_db=False):
        calls.append((tuple(x.shape), sr, roll_percent, want_mag, want_db))
        return R.native_stand_in(x, sr, roll_percent, want_mag, want_db)

    def resample(audio, orig_sr, target_sr, device="cpu"):
        g = np.gcd(orig_sr, target_sr)
        return signal.resample_poly(audio, target_sr // g, orig_sr // g)
    monkeypatch.setattr(native, "spectral_features", features)
    monkeypatch.setattr(A, "resample", resample)
    return Z, calls


def test_analyze_audio_writes_the_figure(stubbed, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    Z, calls = stubbed
    path = _wav(tmp_path / "in" / "voice.wav", R_signal(48000, 48000), 48000)
    png = str(tmp_path / "plots" / "analysis.png")
    info, out = Z.analyze_audio(path, png, device="cpu")
    assert out == png and os.path.getsize(png) > 0
    assert info == "Sample Rate: 22050\nDuration: 1.0 seconds\nNumber of Samples: 22050\nBits per Sample: 48000\nChannels: Mono (1)"
    assert calls == [((22050,), 22050, 0.85, False, True)]          # one call, the dB plane and no magnitude plane
    short = _wav(tmp_path / "in" / "short.wav", R_signal(11025, 22050), 22050)     # drawn as samples, not as an envelope
    assert os.path.getsize(Z.analyze_audio(short, str(tmp_path / "short.png"), device="cpu")[1]) > 0


def test_analyze_audio_without_a_figure_imports_no_matplotlib(stubbed, tmp_path, monkeypatch):
    Z, calls = stubbed
    for name in [m for m in sys.modules if m == "matplotlib" or m.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "matplotlib", None)            # any `import matplotlib` now raises ImportError
    path = _wav(tmp_path / "voice.wav", R_signal(24000, 48000), 48000)
    for falsy in (None, ""):
        info, out = Z.analyze_audio(path, falsy, device="cpu")
        assert out is falsy and info.startswith("Sample Rate: 22050\nDuration: 0.5 seconds\nNumber of Samples: 11025\nBits per Sample: 48000")
    assert calls == []                                              # and no kernel call either: nothing needs the features
    with pytest.raises(ImportError):
        Z.analyze_audio(path, str(tmp_path / "x.png"), device="cpu")


def test_peak_envelope():
    import torch
    from rvc_amd.lib.tools.analyzer import MAX_POINTS, peak_envelope
    x = torch.from_numpy(R_signal(3 * MAX_POINTS + 7))
    hop, env = peak_envelope(x)
    assert hop == 3 and env.shape == (MAX_POINTS + 3,)
    want = [x[i * 3:(i + 1) * 3].abs().max().item() for i in range(len(env))]
    assert env.tolist() == want


def test_analyze_dataset_table(stubbed, tmp_path):
    Z, calls = stubbed
    sr, n = 48000, 48000
    rng = np.random.default_rng(7)
    white = 0.1 * rng.standard_normal(n)
    spec = np.fft.rfft(white)
    spec[np.fft.rfftfreq(n, 1 / sr) > sr / 8] = 0                   # band-limited to a quarter of Nyquist
    dull = np.fft.irfft(spec, n) * 2
    _wav(tmp_path / "white.wav", white, sr)
    _wav(tmp_path / "sub" / "dull.wav", dull, sr)
    _wav(tmp_path / "silent.wav", np.zeros(4000), 16000)
    (tmp_path / "notes.txt").write_text("not audio")
    table = Z.analyze_dataset(str(tmp_path), device="cpu")
    with open(tmp_path / "audio_analysis.json") as f:
        assert json.load(f) == table
    assert sorted(table) == ["files", "roll_percent", "root"] and table["root"] == str(tmp_path) and table["roll_percent"] == 0.99
    assert sorted(table["files"]) == ["silent.wav", os.path.join("sub", "dull.wav"), "white.wav"]
    rec = table["files"]["white.wav"]
    assert sorted(rec) == ["bandwidth", "centroid", "duration", "effective_bandwidth_hz", "effective_bandwidth_ratio", "rolloff85",
                           "rolloff99", "samples", "sr"]
    assert (rec["sr"], rec["samples"], rec["duration"]) == (48000, 48000, 1.0)
    for key in ("centroid", "bandwidth", "rolloff85", "rolloff99"):
        assert sorted(rec[key]) == ["median", "p05", "p95"] and rec[key]["p05"] <= rec[key]["median"] <= rec[key]["p95"]
    assert rec["effective_bandwidth_hz"] == rec["rolloff99"]["median"]
    assert rec["effective_bandwidth_ratio"] == rec["effective_bandwidth_hz"] / 24000 > 0.8
    assert table["files"][os.path.join("sub", "dull.wav")]["effective_bandwidth_ratio"] < 0.3
    silent = table["files"]["silent.wav"]
    assert silent["sr"] == 16000 and silent["effective_bandwidth_hz"] == 0 and silent["centroid"] == {"median": 0.0, "p05": 0.0, "p95": 0.0}
    # two kernel calls per file, one per roll-off percentage, each file at its own rate and no plane
    assert calls == [((4000,), 16000, 0.85, False, False), ((4000,), 16000, 0.99, False, False)] + [
        ((48000,), 48000, p, False, False) for _ in range(2) for p in (0.85, 0.99)]

    # sliced_audios, when it exists, is the directory that is read
    _wav(tmp_path / "sliced_audios" / "0_0.wav", white[:8000], sr)
    table = Z.analyze_dataset(str(tmp_path), roll_percent=0.95, device="cpu")
    assert list(table["files"]) == ["0_0.wav"] and table["root"] == str(tmp_path / "sliced_audios") and table["roll_percent"] == 0.95
    assert os.path.isfile(tmp_path / "audio_analysis.json") and not os.path.exists(tmp_path / "sliced_audios" / "audio_analysis.json")


def test_cli(stubbed, tmp_path, capsys, monkeypatch):
    Z, _ = stubbed
    import torch
    monkeypatch.setattr(Z._native, "_cuda_device", lambda device=None: torch.device("cpu"))
    path = _wav(tmp_path / "a.wav", R_signal(8000, 16000), 16000)
    assert Z.main([path]) == 0
    assert capsys.readouterr().out == "Sample Rate: 22050\nDuration: 0.5 seconds\nNumber of Samples: 11025\nBits per Sample: 16000\nChannels: Mono (1)\n"
    assert Z.main(["--dataset", str(tmp_path)]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("a.wav: sr 16000, 0.50 s, effective bandwidth ") and lines[1] == str(tmp_path / "audio_analysis.json")
    with pytest.raises(SystemExit):
        Z.main([])


def test_the_real_native_call_has_no_host_path(native):
    import torch
    with pytest.raises(native.NativeError, match="HBM"):
        native.spectral_features(torch.zeros(100), 22050)
