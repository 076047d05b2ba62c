"""K19 (formant_shifting, csrc/formant.hip) without a GPU: every refusal of the C ABI comes before any device access, the
workspace does not grow with n beyond one launch group, the restatement of tests/formant_shift_ref.py keeps its own invariants,
and load_audio_infer / VoiceConverter route formant_shifting to shift_formants with the reference's defaults."""
import ctypes

import numpy as np
import pytest

import formant_shift_ref as R


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
GOOD = dict(x=1, n=4000, sr=16000, q=0.8e-3, d=0.8, group=0, out=2, ws=3, ws_bytes=1 << 40)
REFUSALS = [   # (what changes, the words the error must carry)
    (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(out=1), "alias"),
    (dict(n=1023), "shorter than one frame"), (dict(n=0), "shorter than one frame"), (dict(n=-5), "shorter than one frame"),
    (dict(n=(1 << 27) + 1), "exceeds"),
    (dict(sr=0), "sr 0"), (dict(sr=-16000), "sr -16000"),
    (dict(q=-1e-6), "quefrency_s"), (dict(q=float("nan")), "quefrency_s"), (dict(q=512 / 16000), "quefrency of more than 511"),
    (dict(q=float("inf")), "quefrency of more than 511"),
    (dict(d=0.0), "distortion"), (dict(d=-0.8), "distortion"), (dict(d=float("nan")), "distortion"), (dict(d=float("inf")), "distortion"),
    (dict(d=1 / 514), "leaves no bin"),
    (dict(group=-128), "group_frames"), (dict(group=64), "group_frames"), (dict(group=200), "group_frames"), (dict(group=8320), "group_frames"),
    (dict(ws_bytes=0), "workspace too small"),
]


def _forward(native, a):
    """rvc_formant_shift_f32 on addresses that are never dereferenced: 1, 2, 3 stand for host buffers the library must not touch"""
    host = (ctypes.c_float * 16)()
    ptr = lambda v: None if v is None else ctypes.addressof(host) + 16 * v
    ws_bytes = a["ws_bytes"]
    if ws_bytes == 1 << 40:   # "large enough": exactly what the query asks for
        need = ctypes.c_size_t()
        if native._lib.rvc_formant_shift_workspace_bytes(a["n"], a["group"], ctypes.byref(need)) == 0:
            ws_bytes = need.value
    return native._lib.rvc_formant_shift_f32(ptr(a["x"]), a["n"], a["sr"], a["q"], a["d"], a["group"], ptr(a["out"]), ptr(a["ws"]),
                                             ws_bytes, None)


@pytest.mark.parametrize("change,words", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_abi_refuses_before_any_device_access(native, change, words):
    assert _forward(native, {**GOOD, **change}) != 0
    assert words in _err(native), _err(native)


def test_abi_accepts_the_bounds_of_its_ranges_up_to_the_workspace_check(native):
    """Q = 511, int(513 d) = 1, the smallest and largest n and group_frames pass every argument check: the call then stops at the
    workspace size, the last refusal before the device"""
    for change in (dict(q=511 / 16000), dict(q=0.0), dict(d=1 / 513 + 1e-9), dict(d=1e300), dict(n=1024), dict(n=1 << 27),
                   dict(group=128), dict(group=8192), dict(sr=1, q=511.5)):
        assert _forward(native, {**GOOD, **change, "ws_bytes": 0}) != 0
        assert "workspace too small" in _err(native), (change, _err(native))


def test_abi_workspace_is_one_byte_short(native):
    need = ctypes.c_size_t()
    assert native._lib.rvc_formant_shift_workspace_bytes(4000, 0, ctypes.byref(need)) == 0
    assert need.value == 15616 * 128 + 141824            # 94 frames -> 128 GEMM rows, 15.25 KiB each
    assert _forward(native, {**GOOD, "ws_bytes": need.value - 1}) != 0
    assert "workspace too small" in _err(native)


def test_abi_workspace_query_refusals_and_independence_of_n(native):
    lib, need = native._lib, ctypes.c_size_t()
    assert lib.rvc_formant_shift_workspace_bytes(4000, 0, None) != 0 and "null pointer" in _err(native)
    for n, group, words in ((1023, 0, "shorter than one frame"), ((1 << 27) + 1, 0, "exceeds"), (4000, 100, "group_frames"),
                            (4000, 8192 + 128, "group_frames")):
        assert lib.rvc_formant_shift_workspace_bytes(n, group, ctypes.byref(need)) != 0, (n, group)
        assert words in _err(native)
    for group, frames in ((0, 8192), (8192, 8192), (128, 128), (1024, 1024)):
        sizes = []
        for n in (1024 + 32 * (frames - 1), 1024 + 32 * frames, 480000 if frames < 8192 else 4800000, 1 << 27):
            assert lib.rvc_formant_shift_workspace_bytes(n, group, ctypes.byref(need)) == 0
            sizes.append(need.value)
        assert sizes[0] == sizes[1] == sizes[2] == sizes[3] == 15616 * frames + 141824, (group, sizes)
    assert lib.rvc_formant_shift_workspace_bytes(1024 + 32 * 128, 0, ctypes.byref(need)) == 0       # 129 frames -> 256 rows
    assert need.value == 15616 * 256 + 141824


# ---- the restatement's own invariants -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x():
    return R.test_signal(4000)


def test_vocoder_round_trip_is_the_identity(x):
    direct, looped = R.shift_formants(x), R.shift_formants(x, vocoder=True)
    assert R.rms(direct) > 0.05
    assert np.abs(direct - looped).max() <= 1e-12


def test_quefrency_zero_equals_timbre_one(x):
    a, b = R.shift_formants(x, 16000, 0.0, 0.8), R.shift_formants(x, 16000, 0.8e-3, 1.0)
    assert np.abs(a - b).max() <= 1e-12
    assert R.rms(R.shift_formants(x) - b) > 1e-3        # ... and timbre 0.8 is another signal (9e-3)


def test_timbre_below_one_silences_the_upper_bins(x):
    S, Y = R.spectrum(x, 16000, 0.8e-3, 0.8)
    assert int(513 * 0.8) == 410
    assert not Y[:, 410:].any() and np.abs(Y[:, :410]).min() > 0 and np.abs(S[:, 410:]).min() > 0


def test_edges_and_silence(x):
    y = R.shift_formants(np.concatenate([x[:1500], np.zeros(2500)]))
    assert np.isfinite(y).all() and not y[2524:].any() and y[:2500].any()     # frames 47.. hold a zero bin; frame 46 ends at 2496
    y = R.shift_formants(x[:1055])
    assert not y[1024:].any() and y[:1024].any()                               # one frame: 31 dead tail samples


def test_float32_input_runs_in_float32(x):
    y = R.shift_formants(x.astype(np.float32))
    assert y.dtype == np.float32
    e_ref = np.abs(y - R.shift_formants(x)).max()
    assert 1e-9 < e_ref < 1e-6


# ---- routing (the native call stubbed) ----------------------------------------------------------------------------------------------
def _wav(path, n=3200, sr=16000):
    from rvc_amd.infer.infer import _write_wav
    _write_wav(str(path), (0.25 * np.sin(np.arange(n) * 0.05)).astype(np.float32), sr)
    return str(path)


def test_load_audio_infer_reaches_shift_formants_with_the_reference_defaults(native, monkeypatch, tmp_path):
    import torch
    from rvc_amd.lib import audio as A, formant_shift as FS
    calls = []

    def stub(x, sr, quefrency_s, distortion, group_frames=0):
        calls.append((x.dtype, tuple(x.shape), sr, quefrency_s, distortion, group_frames))
        return x * 0.5
    monkeypatch.setattr(FS._native, "formant_shift", stub)
    monkeypatch.setattr(FS._native, "_cuda_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    path = _wav(tmp_path / "in.wav")
    plain = A.load_audio_infer(path, 16000)
    assert calls == [] and plain.dtype == np.float64
    assert np.array_equal(A.load_audio_infer(path, 16000, formant_shifting=False, formant_qfrency=3.0), plain) and calls == []
    shifted = A.load_audio_infer(path, 16000, formant_shifting=True)
    assert calls == [(torch.float32, (3200,), 16000, 0.8 * 1e-3, 0.8, 0)]
    assert shifted.dtype == np.float64 and np.array_equal(shifted, plain.astype(np.float32).astype(np.float64) * 0.5)
    A.load_audio_infer(path, 16000, formant_shifting=True, formant_qfrency=1.5, formant_timbre=1.2)
    assert calls[1][2:] == (16000, 1.5 * 1e-3, 1.2, 0)

    def broken(*a, **k):
        raise FS._native.NativeError("rvc_formant_shift_f32: refused")
    monkeypatch.setattr(FS._native, "formant_shift", broken)
    with pytest.raises(RuntimeError, match="An error occurred loading the audio: rvc_formant_shift_f32: refused"):
        A.load_audio_infer(path, 16000, formant_shifting=True)


class _Pipe:
    trim_vocoder_pad = True

    def __init__(self):
        self.seen = []

    def pipeline(self, **kw):
        self.seen.append(np.array(kw["audio"]))
        return np.zeros(400, dtype=np.float32)


def _converter():
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter.__new__(VoiceConverter)
    vc.vc, vc.tgt_sr, vc.hubert_model, vc.net_g, vc.use_f0, vc.version, vc.trim_vocoder_pad = _Pipe(), 40000, None, None, 1, "v2", True
    vc.config = type("C", (), {"device": "cpu"})()
    return vc


def test_convert_array_shifts_before_the_peak_limiting(native, monkeypatch):
    from rvc_amd.infer import infer as I
    vc, calls = _converter(), []

    def fake_shift(audio, sr, quefrency_ms, timbre, device=None):
        calls.append((audio.dtype, sr, quefrency_ms, timbre, device))
        return audio * 4.0
    monkeypatch.setattr(I, "shift_formants", fake_shift)
    a = np.linspace(-0.5, 0.5, 1600)
    vc.convert_array(a)
    vc.convert_array(a, formant_shifting=False, formant_qfrency=2.0, formant_timbre=2.0)
    assert calls == [] and np.array_equal(vc.vc.seen[0], a) and np.array_equal(vc.vc.seen[1], a)
    vc.convert_array(a, formant_shifting=True)
    assert calls == [(np.float64, 16000, 0.8, 0.8, "cpu")]
    assert np.array_equal(vc.vc.seen[2], a * 4.0 / (2.0 / 0.95))                  # limited AFTER the shift: peak 2.0 -> 0.95
    vc.convert_array(a.astype(np.float32), formant_shifting=True, formant_qfrency=1.5, formant_timbre=1.2)
    assert calls[1] == (np.float64, 16000, 1.5, 1.2, "cpu")


def test_convert_audio_forwards_its_kwargs_to_the_loader(native, monkeypatch, capsys):
    from rvc_amd.infer import infer as I
    vc = _converter()
    vc.get_vc = lambda *a: None
    vc.last_embedder_model, vc.hubert_model = "contentvec", object()
    loads = []
    monkeypatch.setattr(I, "load_audio_infer", lambda *a, **k: loads.append((a, k)) or np.zeros(1600))
    monkeypatch.setattr(I, "shift_formants", lambda *a, **k: pytest.fail("convert_audio shifts in the loader, not a second time"))
    monkeypatch.setattr(I, "_write_wav", lambda path, audio, sr: None)
    vc.convert_audio("in.wav", "out.wav", "model.pth", "")
    vc.convert_audio("in.wav", "out.wav", "model.pth", "", formant_shifting=True, formant_qfrency=1.0, formant_timbre=1.2)
    assert "error" not in capsys.readouterr().out
    assert loads[0] == (("in.wav", 16000), dict(device="cpu"))
    assert loads[1] == (("in.wav", 16000), dict(device="cpu", formant_shifting=True, formant_qfrency=1.0, formant_timbre=1.2))
