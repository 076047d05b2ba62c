"""K24 (the conversion scorer, csrc/convscore.hip) without a GPU: every refusal of the C ABI comes before any device access and
the header agrees with the library; the restatement of tests/conversion_score_ref.py meets its closed forms; the host's finishing
arithmetic is checked on hand-made sums; and the tool's pairing, JSON and command line run with a stub predictor and the native
sums replaced by the restatement."""
import ctypes
import json
import math
import os
import re
import wave

import numpy as np
import pytest

import conversion_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


_host = (ctypes.c_double * 64)()


def _p(v):
    """1 .. 7 stand for host buffers the library must not touch"""
    return None if v is None else ctypes.addressof(_host) + 16 * v


def _need(native, query, *dims):
    need = ctypes.c_size_t()
    return need.value if getattr(native._lib, query)(*dims, ctypes.byref(need)) == 0 else 0


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
MELCEP = dict(x=1, n=4000, sr=16000, mel=2, n_mels=80, n_coef=24, out=3, ws=4, ws_bytes=None)
MELCEP_REFUSALS = [
    (dict(x=None), "null pointer"), (dict(mel=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(n=0), "at least 1"), (dict(n=-3), "at least 1"), (dict(n=(1 << 27) + 1), "exceeds"),
    (dict(sr=7800), "sr 7800"), (dict(sr=48200), "sr 48200"), (dict(sr=22050), "sr 22050"), (dict(sr=0), "sr 0"),
    (dict(n_coef=0), "n_coef"), (dict(n_coef=41), "n_coef"), (dict(n_mels=24), "n_mels"), (dict(n_mels=129), "n_mels"),
    (dict(ws_bytes=0), "workspace too small"),
]


def _melcep(native, a):
    ws_bytes = a["ws_bytes"]
    if ws_bytes is None:
        ws_bytes = _need(native, "rvc_melcep_workspace_bytes", a["n"], a["sr"])
    return native._lib.rvc_melcep_f32(_p(a["x"]), a["n"], a["sr"], _p(a["mel"]), a["n_mels"], a["n_coef"], _p(a["out"]), _p(a["ws"]),
                                      ws_bytes, None)


@pytest.mark.parametrize("change,words", MELCEP_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in MELCEP_REFUSALS])
def test_melcep_refuses_before_any_device_access(native, change, words):
    assert _melcep(native, {**MELCEP, **change}) != 0
    assert words in _err(native), _err(native)


def test_melcep_accepts_the_bounds_up_to_the_workspace_check(native):
    for change in (dict(n=1), dict(n=1 << 27), dict(sr=8000), dict(sr=48000), dict(sr=44000), dict(n_coef=1, n_mels=2),
                   dict(n_coef=40, n_mels=41), dict(n_mels=128)):
        a = {**MELCEP, **change}
        need = _need(native, "rvc_melcep_workspace_bytes", a["n"], a["sr"])
        assert need > 0
        assert _melcep(native, {**a, "ws_bytes": need - 1}) != 0
        assert "workspace too small" in _err(native), (change, _err(native))


def test_melcep_workspace_query(native):
    lib, need = native._lib, ctypes.c_size_t()
    assert lib.rvc_melcep_workspace_bytes(4000, 16000, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_melcep_workspace_bytes(0, 16000, ctypes.byref(need)) != 0 and "at least 1" in _err(native)
    assert lib.rvc_melcep_workspace_bytes(4000, 16001, ctypes.byref(need)) != 0 and "sr 16001" in _err(native)
    sizes = {n: _need(native, "rvc_melcep_workspace_bytes", n, 16000) for n in (1, 80 * 127, 80 * 128, 80 * 2047, 80 * 6000, 1 << 27)}
    assert sizes[1] == sizes[80 * 127] == 128 * 8704                      # up to 128 frames: one GEMM row block
    assert sizes[80 * 128] == 256 * 8704
    assert sizes[80 * 2047] == sizes[80 * 6000] == sizes[1 << 27] == 2048 * 8704   # one group: no growth with the signal


DTW = dict(a=1, Ta=100, b=2, Tb=90, dim=24, band=-1, out=3, path=4, ws=5, ws_bytes=None)
DTW_REFUSALS = [
    (dict(a=None), "null pointer"), (dict(b=None), "null pointer"), (dict(out=None), "null pointer"), (dict(path=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(Ta=0), "Ta = 0"), (dict(Ta=16385), "Ta = 16385"), (dict(Tb=0), "Tb = 0"), (dict(Tb=-1), "Tb = -1"), (dict(Tb=16385), "Tb = 16385"),
    (dict(dim=0), "dim = 0"), (dict(dim=65), "dim = 65"), (dict(band=0), "band = 0"), (dict(ws_bytes=0), "workspace too small"),
]


def _dtw(native, a):
    ws_bytes = a["ws_bytes"]
    if ws_bytes is None:
        ws_bytes = _need(native, "rvc_dtw_workspace_bytes", a["Ta"], a["Tb"])
    return native._lib.rvc_dtw_f64(_p(a["a"]), a["Ta"], _p(a["b"]), a["Tb"], a["dim"], a["band"], _p(a["out"]), _p(a["path"]), _p(a["ws"]),
                                   ws_bytes, None)


@pytest.mark.parametrize("change,words", DTW_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in DTW_REFUSALS])
def test_dtw_refuses_before_any_device_access(native, change, words):
    assert _dtw(native, {**DTW, **change}) != 0
    assert words in _err(native), _err(native)


def test_dtw_accepts_the_bounds_up_to_the_workspace_check(native):
    for change in (dict(Ta=1), dict(Tb=1), dict(Ta=16384, Tb=16384), dict(dim=1), dict(dim=64), dict(band=1), dict(band=1 << 40),
                   dict(band=-7)):
        a = {**DTW, **change}
        need = _need(native, "rvc_dtw_workspace_bytes", a["Ta"], a["Tb"])
        assert _dtw(native, {**a, "ws_bytes": need - 1}) != 0
        assert "workspace too small" in _err(native), (change, _err(native))


def test_dtw_workspace_query(native):
    lib, need = native._lib, ctypes.c_size_t()
    assert lib.rvc_dtw_workspace_bytes(10, 10, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_dtw_workspace_bytes(0, 10, ctypes.byref(need)) != 0 and "Ta = 0" in _err(native)
    assert lib.rvc_dtw_workspace_bytes(10, 16385, ctypes.byref(need)) != 0 and "Tb = 16385" in _err(native)
    up = lambda v: (v + 255) // 256 * 256
    for Ta, Tb in ((1, 1), (100, 90), (6001, 6001), (16384, 16384)):
        assert _need(native, "rvc_dtw_workspace_bytes", Ta, Tb) == up(8 * Tb) + up(4 * Ta * ((Tb + 15) // 16)) + up(8 * (Ta + Tb - 1))
    assert _need(native, "rvc_dtw_workspace_bytes", 16384, 16384) == (64 << 20) + (128 << 10) + (256 << 10)   # the header's 64.4 MiB


def test_small_entry_points_refuse(native):
    lib = native._lib
    for args, words in (((None, _p(2), 10, 24, _p(3), None), "null pointer"), ((_p(1), None, 10, 24, _p(3), None), "null pointer"),
                        ((_p(1), _p(2), 10, 24, None, None), "null pointer"), ((_p(1), _p(2), 0, 24, _p(3), None), "T = 0"),
                        ((_p(1), _p(2), 10, 0, _p(3), None), "dim = 0"), ((_p(1), _p(2), 10, 65, _p(3), None), "dim = 65")):
        assert lib.rvc_frame_dist_sum_f64(*args) != 0 and words in _err(native), (args, _err(native))
    for args, words in (((None, _p(2), 10, _p(3), None), "null pointer"), ((_p(1), None, 10, _p(3), None), "null pointer"),
                        ((_p(1), _p(2), 10, None, None), "null pointer"), ((_p(1), _p(2), 0, _p(3), None), "n = 0"),
                        ((_p(1), _p(2), -4, _p(3), None), "n = -4")):
        assert lib.rvc_f0_track_sums_f64(*args) != 0 and words in _err(native), (args, _err(native))


def test_header_and_library_agree(native):
    """every K24 prototype of include/rvc_amd.h is exported, is bound with as many arguments as the header declares, and the ABI
    version did not move"""
    header = open(os.path.join(ROOT, "include", "rvc_amd.h")).read()
    names = ("rvc_melcep_workspace_bytes", "rvc_melcep_f32", "rvc_dtw_workspace_bytes", "rvc_dtw_f64", "rvc_frame_dist_sum_f64",
             "rvc_f0_track_sums_f64")
    for name in names:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(native.SYMBOLS[name][1]), name
        assert hasattr(native._lib, name)
    assert native._lib.rvc_abi_version() == 4


# ---- the restatement against closed forms -----------------------------------------------------------------------------------------
def test_twin_dtw_identical_sequences():
    x = np.random.default_rng(0).standard_normal((50, 3))
    cost, path = R.dtw(x, x)
    assert cost == 0 and np.array_equal(path, np.stack([np.arange(50)] * 2, axis=1))
    cost, path = R.dtw(x, x, band=1)
    assert cost == 0 and len(path) == 50


def test_twin_dtw_one_frame_doubled():
    x = np.random.default_rng(1).standard_normal((40, 5))
    y = np.concatenate([x[:17], x[16:]])
    cost, path = R.dtw(x, y)
    assert cost == 0 and len(path) == 41
    R.check_path(path, 40, 41)
    assert R.mcd_dtw(x, y) == 0


def test_twin_dtw_against_the_plain_recurrence_and_the_band():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 3, (13, 1)).astype(float), rng.integers(0, 3, (17, 1)).astype(float)
    for band in (None, 1, 3):
        D = np.full((13, 17), np.inf)
        for i in range(13):
            for j in range(17):
                if band is not None and abs(j * 12 - i * 16) > band * 16:
                    continue
                d = abs(a[i, 0] - b[j, 0])
                prev = 0.0 if i == j == 0 else min(D[i - 1, j - 1] if i and j else np.inf, D[i - 1, j] if i else np.inf,
                                                   D[i, j - 1] if j else np.inf)
                D[i, j] = d + prev
        cost, path = R.dtw(a, b, band)
        assert cost == D[12, 16]
        R.check_path(path, 13, 17, band)
        assert R.path_cost(a, b, path) == cost
    # a single row or column: the band does not apply
    assert R.dtw(a[:1], b, 1)[0] == np.abs(a[0, 0] - b[:, 0]).sum()


def test_twin_tie_rule_prefers_the_diagonal_then_up():
    cost, path = R.dtw(np.zeros((3, 1)), np.zeros((3, 1)))
    assert cost == 0 and path.tolist() == [[0, 0], [1, 1], [2, 2]]
    cost, path = R.dtw(np.zeros((3, 1)), np.zeros((2, 1)))
    assert path.tolist() == [[0, 0], [1, 0], [2, 1]]        # (2, 1) <- diagonal (1, 0) <- j == 0: up


def test_twin_cepstra_closed_forms():
    assert R.melcep(np.zeros(80), 16000).shape == (2, 24) and R.melcep(np.zeros(79), 16000).shape == (1, 24)
    assert np.abs(R.melcep(np.zeros(2560), 16000)).max() < 1e-12          # every log mel energy is the floor: a constant has no c[k >= 1]
    x = R.voice(2560, 16000, 3)
    assert np.abs(R.melcep(3.0 * x, 16000)[5:-5] - R.melcep(x, 16000)[5:-5]).max() < 1e-9     # a gain moves c[0] alone
    assert np.abs(R.melcep_torch(x, 16000, __import__("torch").float64) - R.melcep(x, 16000)).max() < 1e-11


def test_twin_f0_shifted_copy():
    a, _ = R.contour_pair(1025, 5)
    r = R.f0_errors(a, a * 2.0 ** (3.0 / 12.0))
    assert r["shift_semitones"] == pytest.approx(3.0, abs=1e-12) and r["f0_rmse_cents"] < 1e-9
    assert r["f0_corr"] == pytest.approx(1.0, abs=1e-12) and r["vuv_error"] == 0 and r["gross_pitch_error"] == 0


# ---- host finishing from hand-made sums ---------------------------------------------------------------------------------------------
def test_finishing_from_hand_made_sums(native):
    from rvc_amd.lib import metrics as M
    # four voiced frames: la = 7, 7, 8, 8 and lb = la + 0.25 -> r = 300 cents everywhere
    la = np.array([7.0, 7.0, 8.0, 8.0])
    lb = la + 0.25
    sums = [4, 1200.0, la.sum(), lb.sum(), (la * la).sum(), (lb * lb).sum(), (la * lb).sum(), 0.0, 0, 1, 2, 3]
    r = M.f0_errors_from_sums(sums)
    assert r == {"voiced_frames": 4, "vuv_error": 0.3, "shift_semitones": 3.0, "f0_rmse_cents": 0.0, "gross_pitch_error": 0.0, "f0_corr": 1.0}
    r = M.f0_errors_from_sums([4, 0.0, la.sum(), la.sum(), (la * la).sum(), (la * la).sum(), -(la * la).sum() + 2 * 7.5 * la.sum(), 4 * 50.0 ** 2,
                               1, 0, 0, 0])
    assert r["f0_corr"] == -1.0 and r["f0_rmse_cents"] == 50.0 and r["gross_pitch_error"] == 0.25 and r["vuv_error"] == 0
    flat = M.f0_errors_from_sums([3, 0.0, 21.0, 21.0, 147.0, 147.0, 147.0, 0.0, 0, 0, 0, 0])
    assert math.isnan(flat["f0_corr"]) and flat["shift_semitones"] == 0
    none = M.f0_errors_from_sums([0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 5])
    assert none["voiced_frames"] == 0 and none["vuv_error"] == 0.5 and all(math.isnan(none[k]) for k in
                                                                          ("f0_rmse_cents", "shift_semitones", "f0_corr", "gross_pitch_error"))
    assert M.mcd_from_sums(3.0, 2) == pytest.approx(10 / math.log(10) * math.sqrt(2) * 1.5, rel=1e-15)
    assert M.GROSS_CENTS == R.GROSS_CENTS and M.MCD_CONST == R.MCD_CONST
    for k in range(1, 9):      # sums and figures agree with the definition on a real contour pair
        a, b = R.contour_pair(500, k)
        want, got = R.f0_errors(a, b), M.f0_errors_from_sums(R.f0_sums(a, b))
        for key in want:
            assert got[key] == pytest.approx(want[key], rel=1e-9, abs=1e-12), key
    with pytest.raises(ValueError):
        M._band(0)
    assert M._band(None) == -1 and M._band(200) == 200


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


class _Stub:
    """a 'pitch estimator' that reads the contour off the signal's length and level: 100 frames per second, pitch = 100 Hz x (1 + the
    file's peak)"""

    def infer_from_audio(self, audio, thred=0.03):
        frames = 1 + len(audio) // 160
        f0 = 100.0 * (1.0 + float(np.abs(audio).max())) * (1.0 + 0.1 * np.sin(np.arange(frames) / 5.0))
        f0[::7] = 0.0
        return f0


@pytest.fixture()
def tool(native, monkeypatch):
    from rvc_amd.lib import metrics as M
    from rvc_amd.lib.tools import score
    monkeypatch.setattr(M, "f0_tracking_errors", lambda a, b, device=None: M.f0_errors_from_sums(R.f0_sums(a, b)))
    return score


def test_pairing_json_and_cli(tool, tmp_path, capsys):
    da, db, dt = tmp_path / "a", tmp_path / "b", tmp_path / "t"
    for d in (da, db, dt):
        d.mkdir()
    t = np.arange(8000) / 16000
    for stem, level in (("one", 0.25), ("two", 0.5), ("only_a", 0.1)):
        _write_wav(da / f"{stem}.wav", 0.25 * np.sin(2 * np.pi * 200 * t))
        if stem != "only_a":
            _write_wav(db / f"{stem}.WAV", level * np.sin(2 * np.pi * 200 * t[:7000]))
    _write_wav(db / "only_b.wav", 0.1 * np.sin(2 * np.pi * 200 * t))
    (db / "notes.txt").write_text("not audio")
    pairs = tool.pair_files(str(da), str(db), str(dt))
    assert [(p[0], os.path.basename(p[1]), os.path.basename(p[2]), p[3]) for p in pairs] == [("one", "one.wav", "one.WAV", None),
                                                                                              ("two", "two.wav", "two.WAV", None)]
    assert tool.main(["--pairs", str(da), str(db)], predictor=_Stub(), device="cuda:0") == 0
    printed = capsys.readouterr().out.splitlines()
    assert printed[0].startswith("one: f0 rmse 0.0 cents") and printed[-1] == str(db / "conversion_scores.json")
    table = json.load(open(db / "conversion_scores.json"))
    assert sorted(table["files"]) == ["one", "two"] and table["target"] is None
    one, two = table["files"]["one"], table["files"]["two"]
    assert set(tool.F0_KEYS) <= set(one) and "mcd_dtw_db" not in one
    assert one["frames"] == 44 and one["vuv_error"] == 0 and abs(one["shift_semitones"]) < 1e-3    # 7000 samples -> 44 frames, cut to common
    assert two["shift_semitones"] == pytest.approx(12 * math.log2(1.5 / 1.25), abs=1e-3)
    assert table["median"]["shift_semitones"] == pytest.approx((one["shift_semitones"] + two["shift_semitones"]) / 2)
    out = tmp_path / "single.json"
    assert tool.main([str(da / "two.wav"), str(db / "two.WAV"), "--json", str(out)], predictor=_Stub(), device="cuda:0") == 0
    assert json.load(open(out)) == two
    with pytest.raises(SystemExit):
        tool.main([str(da / "two.wav")], predictor=_Stub(), device="cuda:0")
    with pytest.raises(ValueError):
        tool.score_pairs(str(da), str(dt), predictor=_Stub(), device="cuda:0")
    with pytest.raises(ValueError):
        tool.score_conversion(("not a pair",), (np.zeros(4), 16000), predictor=_Stub(), device="cuda:0")
    # an [n, channels] array is averaged over its channels whatever its sizes; other shapes are refused
    stereo = np.stack([np.arange(3.0), np.arange(3.0) + 2.0, np.zeros(3), np.zeros(3)], axis=1)            # n = 3 <= 4 channels
    assert tool._load((stereo, 16000), "cuda:0", "source").tolist() == [0.5, 1.0, 1.5]
    with pytest.raises(ValueError):
        tool._load((np.zeros((2, 3, 4)), 16000), "cuda:0", "source")
