"""K21 and the conversion stream without a GPU: every refusal of the two C calls comes before any device access, the frame
arithmetic of a stream for 32 / 40 / 48 kHz models, open_stream's refusals and convert_audio_stream's bookkeeping on a stubbed
pipeline, and the invariants of the float64 restatement (tests/sola_ref.py) the GPU tests rely on."""
import ctypes

import numpy as np
import pytest

import sola_ref as R


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
# addresses that are never dereferenced: slot v stands for a host buffer of 64 KiB the library must not touch
_HOST = (ctypes.c_char * (16 * 65536))()


def _ptr(v):
    return None if v is None else ctypes.addressof(_HOST) + 65536 * v


SOLA_GOOD = dict(infer=0, n=1600 + 400 + 400, buf=2, fade=3, x=400, s=400, b=1600, out=4, off=6, ws=7, ws_bytes=None)
SOLA_REFUSALS = [
    (dict(infer=None), "null pointer"), (dict(buf=None), "null pointer"), (dict(fade=None), "null pointer"), (dict(out=None), "null pointer"),
    (dict(off=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(x=0, n=2000), "xfade 0 must be at least 1"), (dict(x=-3, n=1997), "xfade -3 must be at least 1"),
    (dict(x=1601, n=1601 + 1600 + 400), "longer than the block"),
    (dict(s=-1, n=1999), "search -1 is negative"),
    (dict(n=2399), "is not block + xfade + search"), (dict(n=2401), "is not block + xfade + search"),
    (dict(n=(1 << 24) + 1, b=(1 << 24) + 1 - 800), "exceeds 2^24"),
    (dict(ws_bytes=4 * 401 - 1), "workspace too small"), (dict(ws_bytes=0), "workspace too small"),
    (dict(out=0), "must not alias infer_dev"), (dict(out=2), "must not alias buf_dev"),
]


def _sola(native, a):
    ws_bytes = 4 * (a["s"] + 1) if a["ws_bytes"] is None else a["ws_bytes"]
    return native._lib.rvc_sola_f32(_ptr(a["infer"]), a["n"], _ptr(a["buf"]), _ptr(a["fade"]), a["x"], a["s"], a["b"], _ptr(a["out"]),
                                    _ptr(a["off"]), _ptr(a["ws"]), max(ws_bytes, 0), None)


@pytest.mark.parametrize("change,words", SOLA_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in SOLA_REFUSALS])
def test_sola_refuses_before_any_device_access(native, change, words):
    assert _sola(native, {**SOLA_GOOD, **change}) != 0
    assert "rvc_sola_f32" in _err(native) and words in _err(native), _err(native)


def test_sola_aliasing_is_judged_by_overlap_not_by_equal_addresses(native):
    """out one sample into infer, and out ending inside buf"""
    host = ctypes.addressof(_HOST)
    lib, a = native._lib, SOLA_GOOD

    def call(infer, buf, out):
        return lib.rvc_sola_f32(infer, a["n"], buf, _ptr(3), a["x"], a["s"], a["b"], out, _ptr(6), _ptr(7), 4 * 401, None)
    assert call(host, host + 65536, host + 4) != 0 and "must not alias infer_dev" in _err(native)
    assert call(host, host + 4 * 2400 + 4 * 1599, host + 4 * 2400) != 0 and "must not alias buf_dev" in _err(native)
    assert call(host, host + 4 * 2399, host + 65536 * 4) != 0 and "buf_dev must not alias infer_dev" in _err(native)


def test_sola_accepts_the_bounds_of_its_ranges_up_to_the_workspace_check(native):
    """xfade == block, search == 0, xfade == 1, n_infer == 2^24 pass every argument check: the call then stops at the workspace
    size, the last refusal in front of the aliasing checks and the device"""
    for change in (dict(x=1600, n=3600), dict(s=0, n=2000), dict(x=1, n=2001), dict(x=1, s=0, b=1, n=2), dict(n=1 << 24, b=(1 << 24) - 800)):
        assert _sola(native, {**SOLA_GOOD, **change, "ws_bytes": 0}) != 0
        assert "workspace too small" in _err(native), (change, _err(native))


def test_sola_workspace_query(native):
    lib, need = native._lib, ctypes.c_size_t()
    for x, s in ((1, 0), (400, 400), (2400, 2400)):
        assert lib.rvc_sola_workspace_bytes(x, s, ctypes.byref(need)) == 0 and need.value == 4 * (s + 1)
    assert lib.rvc_sola_workspace_bytes(400, 400, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_sola_workspace_bytes(0, 400, ctypes.byref(need)) != 0 and "xfade 0 must be at least 1" in _err(native)
    assert lib.rvc_sola_workspace_bytes(400, -1, ctypes.byref(need)) != 0 and "search -1 is negative" in _err(native)
    assert lib.rvc_sola_workspace_bytes(400, (1 << 24) + 1, ctypes.byref(need)) != 0 and "exceeds 2^24" in _err(native)


WINDOW_REFUSALS = [
    (dict(hist=None), "null pointer"), (dict(block=None), "null pointer"), (dict(window=None), "null pointer"),
    (dict(n_hist=-1), "is negative"), (dict(n_block=-160), "is negative"),
    (dict(n_hist=(1 << 24) - 1599), "exceeds 2^24"), (dict(n_block=1 << 25), "exceeds 2^24"),
    (dict(window=0), "must not alias hist_dev"), (dict(window=1), "must not alias block_dev"),
]


@pytest.mark.parametrize("change,words", WINDOW_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in WINDOW_REFUSALS])
def test_stream_window_refuses_before_any_device_access(native, change, words):
    a = {**dict(hist=0, n_hist=4800, block=1, n_block=1600, window=2), **change}
    assert native._lib.rvc_stream_window_f32(_ptr(a["hist"]), a["n_hist"], _ptr(a["block"]), a["n_block"], _ptr(a["window"]), None) != 0
    assert "rvc_stream_window_f32" in _err(native) and words in _err(native), _err(native)


def test_stream_window_of_nothing_succeeds_without_a_device(native):
    """n_hist == n_block == 0 launches nothing; an empty hist overlaps nothing, wherever it points"""
    assert native._lib.rvc_stream_window_f32(_ptr(0), 0, _ptr(0), 0, _ptr(0), None) == 0


def test_wrappers_refuse_host_tensors(native):
    import torch
    with pytest.raises(native.NativeError, match="HBM"):
        native.stream_window(torch.zeros(4), torch.zeros(4))
    with pytest.raises(native.NativeError, match="HBM"):
        native.sola(torch.zeros(6), torch.zeros(2), torch.zeros(2), 2, 2)
    with pytest.raises(native.NativeError, match="1-D"):
        native.sola(torch.zeros(1, 6), torch.zeros(2), torch.zeros(2), 2, 2)


# ---- frame arithmetic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [32000, 40000, 48000])
def test_frame_arithmetic(native, sr):
    from rvc_amd.infer.realtime import stream_plan
    q = sr // 100
    p = stream_plan(sr)                                            # 250 / 1000 / 50 / 10 ms
    assert (p.q, p.block_samples, p.hist_samples, p.window_samples) == (q, 4000, 16960, 20960)
    assert (p.block_out, p.xfade, p.search, p.n_infer, p.latency_ms) == (25 * q, 5 * q, q, 31 * q, 310)
    # 20960 + 32000 samples = 331 frames of 10 ms: HuBERT keeps (52960 - 400) // 320 + 1 = 165 frames of 20 ms -> 330, minus the 200 of the pad
    assert p.pipeline_out == 130 * q
    p = stream_plan(sr, block_ms=100, context_ms=500, crossfade_ms=20, search_ms=10)
    assert (p.block_samples, p.hist_samples, p.window_samples, p.block_out, p.xfade, p.search) == (1600, 8480, 10080, 10 * q, 2 * q, q)
    assert p.pipeline_out == 62 * q and p.latency_ms == 130       # 263 frames -> 2 * 131 = 262
    p = stream_plan(sr, block_ms=100, context_ms=510, crossfade_ms=20, search_ms=10)
    assert p.pipeline_out == 62 * q and p.window_samples == 10240  # 264 frames -> 2 * 131: an even frame count loses two
    assert stream_plan(sr, block_ms=10, context_ms=20, crossfade_ms=10, search_ms=0).n_infer == 2 * q


def test_frame_arithmetic_refusals(native):
    from rvc_amd.infer.realtime import stream_plan
    for kw in (dict(block_ms=255), dict(context_ms=1001), dict(crossfade_ms=5), dict(search_ms=12.5), dict(block_ms=-10), dict(search_ms=-10)):
        with pytest.raises(ValueError, match="multiple of 10 ms"):
            stream_plan(48000, **kw)
    with pytest.raises(ValueError, match="at least 10"):
        stream_plan(48000, block_ms=0, crossfade_ms=0)
    with pytest.raises(ValueError, match="longer than block_ms"):
        stream_plan(48000, block_ms=40, crossfade_ms=50)
    with pytest.raises(ValueError, match="context_ms=0 is too short"):
        stream_plan(48000, context_ms=0)
    with pytest.raises(ValueError, match="context_ms=10 is too short"):       # 264 - 200 - 2 frames < 63
        stream_plan(48000, block_ms=500, context_ms=10, crossfade_ms=100, search_ms=30)
    with pytest.raises(ValueError, match="does not fit one pipeline segment"):
        stream_plan(48000, context_ms=41000)
    with pytest.raises(ValueError, match="sample rate 44150"):
        stream_plan(44150)


def test_fade_in_table(native):
    from rvc_amd.infer.realtime import fade_in_table
    f = fade_in_table(960)
    assert f.dtype == np.float32 and f[0] == 0.0 and np.array_equal(f, R.fade_in(960))
    assert np.all(np.diff(f) > 0) and abs(float(f[480]) - 0.5) < 1e-7 and f[-1] < 1.0


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,s,b,lag,seed", R.PLANTED, ids=[f"X{c[0]}-S{c[1]}-B{c[2]}-lag{c[3]}" for c in R.PLANTED])
def test_restatement_recovers_a_planted_lag_with_a_margin_above_tau(x, s, b, lag, seed):
    infer, buf = R.planted(x, s, b, lag, seed)
    out, new_buf, offset, sc = R.sola(infer, buf, R.fade_in(x), s, b)
    assert offset == lag and sc.shape == (s + 1,)
    norm = np.sqrt((buf.astype(np.float64) ** 2).sum())
    assert abs(sc[lag] - norm) <= 1e-7 * norm + 1e-8                       # nom = ||buf||^2, den = sqrt(||buf||^2 + 1e-8)
    if s:
        runner_up = np.delete(sc, lag).max()
        print(f"X={x} S={s} lag={lag}: max {sc[lag]:.4f}, runner-up {runner_up:.4f}, tau {R.tau(buf):.2e}")
        assert runner_up < sc[lag] - R.tau(buf)
    # with buf a piece of infer the crossfade is the identity up to rounding, and the new tail is copied
    assert np.abs(out - infer[lag:lag + b]).max() <= 1e-7 and np.array_equal(out[x:], infer[lag + x:lag + b].astype(np.float64))
    assert np.array_equal(new_buf, infer[lag + b:lag + b + x]) and new_buf.dtype == np.float32


def test_restatement_edge_cases():
    infer = R.test_signal(640 + 320 + 320, 9)
    out, new_buf, offset, sc = R.sola(infer, np.zeros(320, np.float32), R.fade_in(320), 320, 640)
    assert offset == 0 and not sc.any()                                      # zeros after reset: lag 0, a plain fade-in
    assert np.array_equal(out[:320], infer[:320].astype(np.float64) * R.fade_in(320)) and out[0] == 0.0
    tie = np.tile(R.test_signal(64, 10), 20)                                  # period 64: lags 5, 69, 133, ... score the same
    _, _, offset, sc = R.sola(tie, tie[5:5 + 320].copy(), R.fade_in(320), 320, 640)
    assert offset == 5 and np.sum(sc >= sc.max() - 1e-9) == 5
    forced, _, off2, _ = R.sola(tie, tie[5:5 + 320].copy(), R.fade_in(320), 320, 640, offset=69)
    assert off2 == 69 and np.abs(forced - tie[5:5 + 640]).max() <= 1e-7
    silent = R.sola(np.zeros(1280, np.float32), infer[:320], R.fade_in(320), 320, 640)
    assert silent[2] == 0 and np.isfinite(silent[3]).all()                   # the 1e-8 keeps 0 / 0 away


def test_restatement_window_rule():
    hist = np.arange(5, dtype=np.float32)
    w, h = R.window(hist, np.arange(10, 13, dtype=np.float32))               # block shorter than hist: hist moves up
    assert w.tolist() == [0, 1, 2, 3, 4, 10, 11, 12] and h.tolist() == [3, 4, 10, 11, 12]
    w, h = R.window(hist, np.arange(10, 17, dtype=np.float32))               # block longer: its end
    assert h.tolist() == [12, 13, 14, 15, 16]
    w, h = R.window(hist[:0], hist)
    assert np.array_equal(w, hist) and h.shape == (0,)


def test_test_signal_is_band_limited_and_seeded():
    a, b = R.test_signal(4096, 3), R.test_signal(4096, 3)
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, R.test_signal(4096, 4))
    assert abs(np.abs(a).max() - 0.5) < 1e-6
    spec = np.abs(np.fft.rfft(a.astype(np.float64)))
    assert spec[1100:].max() < 1e-3 * spec.max()                             # nothing above half the Nyquist frequency (bin 1024)


# ---- the stream on a stubbed pipeline -------------------------------------------------------------------------------------------------
class _Pipe:
    """Pipeline.pipeline as the identity 'resampled' by repetition: every input sample q / 160 times, of the frames the real one
    returns for a window (the last one or two are dropped)."""
    x_pad, x_max, trim_vocoder_pad = 1, 41, True

    def __init__(self, sr):
        self.sr, self.calls = sr, []

    def pipeline(self, **kw):
        import torch
        self.calls.append(kw)
        audio = kw["audio"]
        n = audio.shape[0] + 32000
        frames = min(n // 160, 2 * ((n - 400) // 320 + 1)) - 200
        return torch.repeat_interleave(audio[:frames * 160], self.sr // 100)[::160].contiguous()


def _converter(sr=40000):
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter.__new__(VoiceConverter)
    vc.vc, vc.tgt_sr, vc.hubert_model, vc.net_g, vc.use_f0, vc.version, vc.trim_vocoder_pad = _Pipe(sr), sr, object(), object(), 1, "v2", True
    vc.config = type("C", (), {"device": "cpu"})()
    vc.loaded_model, vc.last_embedder_model, vc._streams = "model.pth", "contentvec", set()
    return vc


@pytest.fixture()
def host_kernels(native, monkeypatch):
    """rvc_stream_window_f32 / rvc_sola_f32 replaced by the restatement on host tensors (no device here)"""
    import torch
    from rvc_amd.infer import realtime

    def window(hist, block):
        w, h = R.window(hist.numpy(), block.numpy())
        hist.copy_(torch.from_numpy(h))
        return torch.from_numpy(w)

    def sola(infer, buf, fade, search, block, offset=None):
        out, new_buf, off, _ = R.sola(infer.numpy(), buf.numpy(), fade.numpy(), search, block)
        buf.copy_(torch.from_numpy(new_buf))
        offset.fill_(off)
        return torch.from_numpy(out.astype(np.float32)), offset
    monkeypatch.setattr(realtime._native, "stream_window", window)
    monkeypatch.setattr(realtime._native, "sola", sola)
    return realtime


def test_open_stream_refusals(host_kernels):
    vc = _converter()
    for name, value in (("split_audio", True), ("f0_file", "f0.csv"), ("clean_audio", True), ("formant_shifting", True), ("post_process", True),
                        ("resample_sr", 44100)):
        with pytest.raises(NotImplementedError, match=name):
            vc.open_stream(**{name: value})
    with pytest.raises(TypeError, match="reverb"):
        vc.open_stream(reverb=True)
    for kw, words in ((dict(block_ms=255), "multiple of 10 ms"), (dict(crossfade_ms=45), "multiple of 10 ms"), (dict(context_ms=0.5), "multiple of 10 ms"),
                      (dict(search_ms=7), "multiple of 10 ms"), (dict(block_ms=40, crossfade_ms=50), "longer than block_ms")):
        with pytest.raises(ValueError, match=words):
            vc.open_stream(**kw)
    assert not vc._streams
    # the falsy spellings of the refused options are what convert_audio's callers pass along: accepted
    stream = vc.open_stream("model.pth", split_audio=False, f0_file=None, clean_audio=False, formant_shifting=False, post_process=False, resample_sr=0)
    assert vc._streams == {stream} and (stream.block_samples, stream.block_out, stream.sr, stream.latency_ms) == (4000, 10000, 40000, 310)
    for bad in (np.zeros(3999, np.float32), np.zeros(4001), np.zeros((1, 4000), np.float32), __import__("torch").zeros(4001)):
        with pytest.raises(ValueError, match="a block is 4000 samples"):
            stream.push(bad)
    with pytest.raises(ValueError, match="float32 or float64"):
        stream.push(np.zeros(4000, np.int16))
    # a second model on a converter with an open stream
    with pytest.raises(RuntimeError, match="open stream"):
        vc.open_stream("other.pth")
    with pytest.raises(RuntimeError, match="open stream"):
        vc.get_vc("other.pth", 0)
    with pytest.raises(RuntimeError, match="open stream"):
        vc.load_checkpoint_dict({})
    vc.get_vc("model.pth", 0)                       # the loaded one: nothing to do
    second = vc.open_stream()
    assert len(vc._streams) == 2
    stream.close(), second.close(), second.close()
    assert not vc._streams
    with pytest.raises(RuntimeError, match="closed"):
        stream.push(np.zeros(4000, np.float32))
    vc.vc = None
    with pytest.raises(RuntimeError, match="no model is loaded"):
        vc.open_stream()


def test_push_hands_the_pipeline_convert_arrays_keywords_and_a_seed_per_block(host_kernels):
    vc = _converter(32000)
    stream = vc.open_stream(None, ' "logs/trained_x.index" ', block_ms=100, context_ms=500, crossfade_ms=20, search_ms=10, pitch=3, index_rate=0.5,
                            protect=0.33, sid=2, noise_seed=7)
    stream.debug = True
    x = R.test_signal(3 * 1600, 11)
    outs = [stream.push(x[j * 1600:(j + 1) * 1600].astype(np.float64 if j == 1 else np.float32)) for j in range(3)]
    assert all(o.dtype == np.float32 and o.shape == (3200,) for o in outs)
    calls = vc.vc.calls
    assert [c["noise_seed"] for c in calls] == [7, 8, 9] and len(stream.debug_log) == 3
    kw = dict(calls[0])
    audio = kw.pop("audio")
    assert kw == dict(model=vc.hubert_model, net_g=vc.net_g, sid=2, pitch=3, f0_method="rmvpe", file_index="logs/added_x.index", index_rate=0.5,
                      pitch_guidance=1, filter_radius=3.0, volume_envelope=1, version="v2", protect=0.33, hop_length=128, f0_autotune=False,
                      f0_autotune_strength=1, f0_file=None, noise_seed=7)
    assert audio.shape == (10080,) and not audio[:8480].any() and np.array_equal(audio[8480:].numpy(), x[:1600])
    assert np.array_equal(calls[2]["audio"][8480 - 3200:].numpy(), x)          # the window's tail is the input so far
    assert stream.debug_log[0]["infer"].shape == (13 * 320,) and not stream.debug_log[0]["buf"].any() and stream.debug_log[0]["offset"] == 0
    stream.reset()
    again = stream.push(x[:1600])
    assert np.array_equal(again, outs[0]) and vc.vc.calls[-1]["noise_seed"] == 7 and stream.pushes == 1
    # a pipeline whose output length the frame arithmetic does not predict is an error, not a silent misalignment
    vc.vc.pipeline = lambda **kw: __import__("torch").zeros(62 * 320 + 1)
    with pytest.raises(RuntimeError, match="frame arithmetic expects 19840"):
        stream.push(x[:1600])


class _Clock:
    """torch.cuda.Event's timing surface on the host"""

    def __init__(self, enable_timing=False):
        self.t = None

    def record(self):
        import time
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


@pytest.mark.parametrize("n_in,blocks", [(16000, 4), (16001, 5), (9000, 3), (1, 1)])
def test_convert_audio_stream_length_and_block_count(host_kernels, monkeypatch, tmp_path, n_in, blocks):
    import wave
    from rvc_amd.infer.infer import _write_wav
    monkeypatch.setattr(host_kernels, "_Event", _Clock)
    vc = _converter(40000)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    x = R.test_signal(max(n_in, 4), 12)[:n_in]
    _write_wav(src, x, 16000)
    monkeypatch.setattr("rvc_amd.infer.infer.load_audio_infer", lambda path, sr, device=None, **kw: x.astype(np.float64))
    report = vc.convert_audio_stream(src, dst, "model.pth", "", block_ms=250, context_ms=500, crossfade_ms=50, search_ms=10)
    assert report["blocks"] == blocks == len(report["push_ms"]) == len(vc.vc.calls) and report["block_ms"] == 250
    assert report["median_ms"] == float(np.median(report["push_ms"])) and report["max_ms"] == max(report["push_ms"]) >= 0
    with wave.open(dst, "rb") as f:
        assert f.getframerate() == 40000 and f.getnframes() == n_in * 40000 // 16000
    assert not vc._streams                                                       # closed again
