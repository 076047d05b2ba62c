"""K22 (post_process, csrc/effects.hip) without a GPU: every refusal of the C ABI comes before any device access, the host
constants equal the restatement's (tests/effects_ref.py), the restatement itself obeys closed forms that a misread formula would
break, and VoiceConverter routes post_process to post_process_audio."""
import ctypes

import numpy as np
import pytest

import effects_ref as R

NAN = float("nan")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _err(native):
    return native._lib.rvc_last_error().decode()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
# Each entry point with arguments it accepts; `1` stands for a host buffer the library must never dereference, and ws_bytes =
# None for "exactly what the size query asks for".
HOST = (ctypes.c_float * 4)()


def _ptr(v):
    return ctypes.addressof(HOST) if v == 1 else None


def _ws_bytes(native, query, a, *dims):
    if a["ws_bytes"] is not None:
        return a["ws_bytes"]
    need = ctypes.c_size_t()
    return need.value if getattr(native._lib, query)(*dims, ctypes.byref(need)) == 0 else 1 << 40


def _pointwise(native, a):
    return native._lib.rvc_fx_pointwise_f32(_ptr(a["x"]), a["n"], a["stages"], a["gain_db"], a["drive_db"], a["bit_depth"],
                                            a["clip_threshold_db"], _ptr(a["out"]), None)


def _delay(native, a):
    return native._lib.rvc_fx_delay_f32(_ptr(a["x"]), a["n"], a["sr"], a["delay_seconds"], a["feedback"], a["mix"], _ptr(a["out"]), None)


def _chorus(native, a):
    ws = _ws_bytes(native, "rvc_fx_chorus_workspace_bytes", a, a["n"], a["feedback"])
    return native._lib.rvc_fx_chorus_f32(_ptr(a["x"]), a["n"], a["sr"], a["rate_hz"], a["depth"], a["centre_delay_ms"], a["feedback"],
                                         a["mix"], _ptr(a["out"]), _ptr(a["ws"]), ws, None)


def _reverb(native, a):
    ws = _ws_bytes(native, "rvc_fx_reverb_workspace_bytes", a, a["n"])
    return native._lib.rvc_fx_reverb_f32(_ptr(a["x"]), a["n"], a["sr"], a["room_size"], a["damping"], a["wet_level"], a["dry_level"],
                                         a["width"], a["freeze_mode"], _ptr(a["out"]), _ptr(a["ws"]), ws, None)


def _compressor(native, a):
    ws = _ws_bytes(native, "rvc_fx_compressor_workspace_bytes", a, a["n"], a["chunk"], 0)
    return native._lib.rvc_fx_compressor_f32(_ptr(a["x"]), a["n"], a["sr"], a["threshold_db"], a["ratio"], a["attack_ms"], a["release_ms"],
                                             a["chunk"], _ptr(a["out"]), _ptr(a["ws"]), ws, None)


def _limiter(native, a):
    ws = _ws_bytes(native, "rvc_fx_compressor_workspace_bytes", a, a["n"], a["chunk"], 1)
    return native._lib.rvc_fx_limiter_f32(_ptr(a["x"]), a["n"], a["sr"], a["threshold_db"], a["release_ms"], a["chunk"], _ptr(a["out"]),
                                          _ptr(a["ws"]), ws, None)


SIGNAL = dict(x=1, out=1, n=9000, sr=48000)
ENTRY = {   # name -> (call, accepted arguments, [(what changes, the words the error must carry)])
    "pointwise": (_pointwise, dict(SIGNAL, stages=15, gain_db=3.0, drive_db=25.0, bit_depth=8.0, clip_threshold_db=0.0), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(n=-1), "negative"), (dict(n=(1 << 27) + 1), "exceeds"),
        (dict(stages=0), "stages"), (dict(stages=16), "stages"),
        (dict(gain_db=201.0), "gain_db"), (dict(gain_db=NAN), "gain_db"), (dict(drive_db=-201.0), "drive_db"), (dict(drive_db=NAN), "drive_db"),
        (dict(bit_depth=0.0), "bit_depth"), (dict(bit_depth=32.5), "bit_depth"), (dict(bit_depth=NAN), "bit_depth"),
        (dict(clip_threshold_db=float("inf")), "clip_threshold_db"), (dict(clip_threshold_db=NAN), "clip_threshold_db")]),
    "delay": (_delay, dict(SIGNAL, delay_seconds=0.5, feedback=0.5, mix=0.5), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(n=-1), "negative"), (dict(n=(1 << 27) + 1), "exceeds"),
        (dict(sr=7999), "sr 7999"), (dict(sr=96001), "sr 96001"), (dict(sr=0), "sr 0"),
        (dict(delay_seconds=0.00002), "delay_seconds"), (dict(delay_seconds=-1.0), "delay_seconds"), (dict(delay_seconds=61.0), "delay_seconds"),
        (dict(delay_seconds=NAN), "delay_seconds"), (dict(feedback=1.5), "feedback"), (dict(feedback=NAN), "feedback"),
        (dict(mix=-0.1), "mix"), (dict(mix=1.1), "mix"), (dict(mix=NAN), "mix")]),
    "chorus": (_chorus, dict(SIGNAL, ws=1, ws_bytes=None, rate_hz=1.0, depth=0.25, centre_delay_ms=7.0, feedback=0.5, mix=0.5), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=-1), "negative"),
        (dict(sr=7999), "sr 7999"), (dict(sr=96001), "sr 96001"),
        (dict(rate_hz=-1.0), "rate_hz"), (dict(rate_hz=101.0), "rate_hz"), (dict(rate_hz=NAN), "rate_hz"),
        (dict(depth=-0.1), "depth"), (dict(depth=NAN), "depth"), (dict(centre_delay_ms=-1.0), "centre_delay_ms"),
        (dict(centre_delay_ms=99.0), "centre_delay_ms"), (dict(centre_delay_ms=NAN), "centre_delay_ms"),
        (dict(feedback=-1.5), "feedback"), (dict(feedback=NAN), "feedback"), (dict(mix=1.5), "mix"), (dict(mix=NAN), "mix"),
        (dict(ws_bytes=12 * 9000 - 1), "workspace too small")]),
    "reverb": (_reverb, dict(SIGNAL, ws=1, ws_bytes=None, room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0, freeze_mode=0.0), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=-1), "negative"),
        (dict(sr=7999), "sr 7999"), (dict(sr=96001), "sr 96001"),
        (dict(room_size=1.1), "room_size"), (dict(room_size=NAN), "room_size"), (dict(damping=-0.1), "damping"), (dict(damping=NAN), "damping"),
        (dict(wet_level=1.1), "wet_level"), (dict(wet_level=NAN), "wet_level"), (dict(dry_level=-0.1), "dry_level"), (dict(dry_level=NAN), "dry_level"),
        (dict(width=1.1), "width"), (dict(width=NAN), "width"), (dict(freeze_mode=2.0), "freeze_mode"), (dict(freeze_mode=NAN), "freeze_mode"),
        (dict(ws_bytes=36 * 9000 - 1), "workspace too small")]),
    "compressor": (_compressor, dict(SIGNAL, ws=1, ws_bytes=None, threshold_db=-20.0, ratio=4.0, attack_ms=1.0, release_ms=100.0, chunk=0), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=-1), "negative"),
        (dict(sr=7999), "sr 7999"), (dict(sr=96001), "sr 96001"),
        (dict(threshold_db=201.0), "threshold_db"), (dict(threshold_db=NAN), "threshold_db"),
        (dict(ratio=0.5), "ratio"), (dict(ratio=NAN), "ratio"), (dict(attack_ms=-1.0), "attack_ms"), (dict(attack_ms=NAN), "attack_ms"),
        (dict(release_ms=-1.0), "release_ms"), (dict(release_ms=NAN), "release_ms"), (dict(chunk=-1), "chunk"),
        (dict(ws_bytes=16 + 12 * 36 - 1), "workspace too small")]),      # 9000 samples = 36 chunks of 256
    "limiter": (_limiter, dict(SIGNAL, ws=1, ws_bytes=None, threshold_db=-6.0, release_ms=0.05, chunk=0), [
        (dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=-1), "negative"),
        (dict(sr=7999), "sr 7999"), (dict(sr=96001), "sr 96001"),
        (dict(threshold_db=-201.0), "threshold_db"), (dict(threshold_db=NAN), "threshold_db"),
        (dict(release_ms=-1.0), "release_ms"), (dict(release_ms=NAN), "release_ms"), (dict(chunk=-1), "chunk"),
        (dict(ws_bytes=16 + 12 * 36 + 4 * 9000 - 1), "workspace too small")]),
}
REFUSALS = [(name, change, words) for name, (_, _, cases) in ENTRY.items() for change, words in cases]


@pytest.mark.parametrize("name,change,words", REFUSALS, ids=[f"{n}:" + ",".join(f"{k}={v}" for k, v in c.items()) for n, c, _ in REFUSALS])
def test_abi_refuses_before_any_device_access(native, name, change, words):
    call, good, _ = ENTRY[name]
    assert call(native, {**good, **change}) != 0
    assert words in _err(native), _err(native)


@pytest.mark.parametrize("name", list(ENTRY))
def test_abi_empty_signal_succeeds_and_touches_nothing(native, name):
    call, good, _ = ENTRY[name]
    assert call(native, {**good, "n": 0, "ws_bytes": 0}) == 0, _err(native)


def test_abi_workspace_queries(native):
    lib, need = native._lib, ctypes.c_size_t(7)
    assert lib.rvc_fx_chorus_workspace_bytes(9000, 0.0, ctypes.byref(need)) == 0 and need.value == 0     # feedback 0: a gather
    assert lib.rvc_fx_chorus_workspace_bytes(9000, -0.5, ctypes.byref(need)) == 0 and need.value == 12 * 9000
    assert lib.rvc_fx_reverb_workspace_bytes(9000, ctypes.byref(need)) == 0 and need.value == 36 * 9000
    assert lib.rvc_fx_compressor_workspace_bytes(9000, 0, 0, ctypes.byref(need)) == 0 and need.value == 16 + 12 * 36
    assert lib.rvc_fx_compressor_workspace_bytes(9000, 1000, 1, ctypes.byref(need)) == 0 and need.value == 16 + 12 * 9 + 4 + 4 * 9000
    assert lib.rvc_fx_compressor_workspace_bytes(9000, 1 << 40, 0, ctypes.byref(need)) == 0 and need.value == 32
    for n in (0,):
        assert lib.rvc_fx_chorus_workspace_bytes(n, 0.5, ctypes.byref(need)) == 0 and need.value == 0
        assert lib.rvc_fx_reverb_workspace_bytes(n, ctypes.byref(need)) == 0 and need.value == 0
        assert lib.rvc_fx_compressor_workspace_bytes(n, 0, 1, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.rvc_fx_chorus_workspace_bytes(9000, 0.5, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_fx_reverb_workspace_bytes(9000, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_fx_compressor_workspace_bytes(9000, 0, 0, None) != 0 and "null pointer" in _err(native)
    assert lib.rvc_fx_chorus_workspace_bytes(-1, 0.5, ctypes.byref(need)) != 0 and "negative" in _err(native)
    assert lib.rvc_fx_chorus_workspace_bytes(9000, NAN, ctypes.byref(need)) != 0 and "feedback" in _err(native)
    assert lib.rvc_fx_reverb_workspace_bytes((1 << 27) + 1, ctypes.byref(need)) != 0 and "exceeds" in _err(native)
    assert lib.rvc_fx_compressor_workspace_bytes(9000, -1, 0, ctypes.byref(need)) != 0 and "chunk" in _err(native)
    assert lib.rvc_fx_compressor_workspace_bytes(9000, 0, 2, ctypes.byref(need)) != 0 and "limiter" in _err(native)


def test_abi_chorus_without_feedback_needs_no_workspace(native):
    call, good, _ = ENTRY["chorus"]
    assert call(native, {**good, "n": 0, "feedback": 0.0, "ws": None, "ws_bytes": 0}) == 0, _err(native)


# ---- host constants vs the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [16000, 32000, 40000, 48000])
def test_host_constants_equal_the_restatement(native, sr):
    comb, allpass = native.fx_reverb_params(sr)
    assert (comb, allpass) == tuple(R.reverb_lengths(sr))
    assert min(comb) == comb[0] == sr * 1116 // 44100
    for attack_ms, release_ms in ((1.0, 100.0), (2.0, 200.0), (0.001, 0.05), (0.0, 1e5)):
        got = native.fx_ballistics(sr, attack_ms, release_ms)
        for c, c_ref in zip(got, (R.ballistics(sr, attack_ms), R.ballistics(sr, release_ms))):
            assert abs(c - c_ref) <= np.spacing(c_ref) and 0.0 <= c < 1.0
    assert native.fx_ballistics(sr, 0.001, 0.05)[0] == 0.0                 # the limiter's attack
    for bad in (7999, 96001):
        with pytest.raises(native.NativeError, match=f"sr {bad}"):
            native.fx_reverb_params(bad)
    with pytest.raises(native.NativeError, match="release_ms"):
        native.fx_ballistics(sr, 1.0, NAN)


# ---- closed forms on the restatement ------------------------------------------------------------------------------------------------
def _impulse(n):
    x = np.zeros(n)
    x[0] = 1.0
    return x


def test_restatement_delay_impulse_response():
    D, fb, mix = 100, 0.5, 0.3                                             # delay_seconds = 100 / 16000
    y = R.delay(_impulse(1000), 16000, D / 16000, fb, mix)
    expect = np.zeros(1000)
    expect[0] = 1 - mix
    for k in range(1, 10):
        expect[k * D] = mix * fb ** (k - 1)
    assert np.abs(y - expect).max() <= 1e-15


def test_restatement_reverb_impulse_response():
    sr, kw = 16000, dict(room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.0, width=1.0, freeze_mode=0.0)
    wet1 = R.reverb_constants(**kw)[3]
    D1 = R.reverb_lengths(sr)[0][0]
    y = R.reverb(_impulse(D1 + 50), sr, **kw)
    assert wet1 == 1.5 * 0.33 * 2.0 and D1 == 404
    assert not y[:D1].any()                                                # dry = 0: silence until the shortest comb answers
    # the comb stored in = 0.015 at time 0 and hands it out at D1 (o = line, before the damping filter); each of the four
    # allpasses passes -in at once (out = b - in with an empty line): (-1)^4 = +1
    assert abs(y[D1] - 0.015 * wet1) <= 1e-17
    frozen = R.reverb(_impulse(2000), sr, **{**kw, "freeze_mode": 1.0, "dry_level": 0.25})
    assert np.array_equal(frozen, _impulse(2000) * 0.5)                    # frozen: no input reaches the (empty) lines


def test_restatement_compressor_converges_on_a_constant():
    sr, A, thr_db, ratio = 16000, 0.5, -20.0, 4.0
    x = np.full(4000, A) * np.where(np.arange(4000) % 2, -1.0, 1.0)       # |x| = A, the sign alternating
    y = R.compressor(x, sr, thr_db, ratio, 1.0, 100.0)
    g = (A / R.db_to_gain(thr_db)) ** (1 / ratio - 1)
    assert g < 0.5 and np.abs(y[-100:] / x[-100:] - g).max() <= 1e-12
    assert abs(y[0] / x[0]) > g                                            # the attack takes time


def test_restatement_limiter_never_exceeds_one():
    x = R.signal(6000, 16000, seed=3, peak=4.0)
    for dtype in (np.float64, np.float32):
        y = R.limiter(x, 16000, -6.0, 0.05, dtype)
        assert y.dtype == dtype and np.abs(y).max() <= 1.0 and np.abs(y).max() > 0.5


def test_restatement_identities():
    x = R.signal(3000, 16000, seed=4)
    assert np.array_equal(R.compressor(x, 16000, -30.0, 1.0, 1.0, 100.0), x.astype(np.float64))      # ratio 1: gain 1 everywhere
    assert np.array_equal(R.post_process(x, 16000), x.astype(np.float64))                              # nothing enabled
    assert np.array_equal(R.bitcrush(np.arange(-8, 9) / 8.0, 3), np.arange(-8, 9) / 8.0)               # already on the 3-bit grid
    assert np.array_equal(R.bitcrush(np.array([0.0625, 0.1875, -0.0625]), 3), [0.0, 0.25, -0.0])       # halves go to the even step


def test_empty_board_is_the_identity_and_launches_nothing(native, monkeypatch):
    from rvc_amd.lib import effects as E
    for name in ("fx_pointwise", "fx_delay", "fx_chorus", "fx_reverb", "fx_compressor", "fx_limiter"):
        monkeypatch.setattr(E._native, name, lambda *a, **k: pytest.fail("an empty board must not reach the library"))
    x = R.signal(100, 16000)
    assert E.Pedalboard()(x, 16000) is x and len(E.Pedalboard()) == 0
    from rvc_amd.infer.infer import VoiceConverter
    assert VoiceConverter.post_process_audio(x, 40000) is x
    assert VoiceConverter.post_process_audio(x, 40000, reverb=False, gain=False, reverb_room_size=0.9) is x


def test_pitch_shift_raises_by_name(native):
    from rvc_amd.lib import effects as E
    from rvc_amd.infer.infer import VoiceConverter
    with pytest.raises(NotImplementedError, match="PitchShift"):
        E.PitchShift(semitones=2)
    with pytest.raises(NotImplementedError, match="pitch_shift"):
        VoiceConverter.post_process_audio(np.zeros(8, dtype=np.float32), 40000, pitch_shift=True)


def test_board_fuses_neighbouring_pointwise_stages(native, monkeypatch):
    from rvc_amd.lib import effects as E
    board = E.Pedalboard([E.Reverb(), E.Limiter(), E.Gain(3), E.Distortion(), E.Chorus(), E.Bitcrush(), E.Clipping(), E.Compressor(), E.Delay()])
    assert [[type(p).__name__ for p in g] for g in board.launches()] == [
        ["Reverb"], ["Limiter"], ["Gain", "Distortion"], ["Chorus"], ["Bitcrush", "Clipping"], ["Compressor"], ["Delay"]]
    assert [len(g) for g in E.Pedalboard([E.Clipping(), E.Gain(1), E.Gain(2), E.Bitcrush()]).launches()] == [1, 1, 2]
    assert (E.Reverb().room_size, E.Reverb().damping, E.Reverb().wet_level, E.Reverb().dry_level, E.Reverb().width, E.Reverb().freeze_mode) == \
        (0.5, 0.5, 0.33, 0.4, 1.0, 0.0)
    assert (E.Limiter().threshold_db, E.Limiter().release_ms, E.Gain().gain_db, E.Distortion().drive_db) == (-6.0, 0.05, 0.0, 25.0)
    assert (E.Chorus().rate_hz, E.Chorus().depth, E.Chorus().centre_delay_ms, E.Chorus().feedback, E.Chorus().mix) == (1.0, 0.25, 7.0, 0.0, 0.5)
    assert (E.Bitcrush().bit_depth, E.Clipping().threshold_db) == (8.0, 0.0)
    assert (E.Compressor().threshold_db, E.Compressor().ratio, E.Compressor().attack_ms, E.Compressor().release_ms) == (0.0, 1.0, 1.0, 100.0)
    assert (E.Delay().delay_seconds, E.Delay().feedback, E.Delay().mix) == (0.5, 0.0, 0.5)
    with pytest.raises(ValueError, match="1-D"):
        board(np.zeros((2, 8), dtype=np.float32), 40000)
    with pytest.raises(ValueError, match="sample_rate"):
        board(np.zeros(8, dtype=np.float32), 44100.5)


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


def test_post_process_reaches_post_process_audio(native, monkeypatch):
    from rvc_amd.infer import infer as I
    raw = np.linspace(-0.5, 0.5, 400, dtype=np.float32)
    vc, calls = _converter(raw), []

    def fake_board(audio_input, sample_rate, **kwargs):
        calls.append((audio_input.copy(), sample_rate, kwargs))
        return audio_input + 1.0
    monkeypatch.setattr(I.VoiceConverter, "post_process_audio", staticmethod(fake_board))
    monkeypatch.setattr(I, "reduce_noise", lambda y, sr, prop_decrease: y * 0.5)
    a = np.zeros(1600)
    assert np.array_equal(vc.convert_array(a), raw) and calls == []                                   # default: not called
    assert np.array_equal(vc.convert_array(a, reverb=True, reverb_room_size=0.9), raw) and calls == []  # effect keywords alone do nothing
    out = vc.convert_array(a, clean_audio=True, post_process=True, reverb=True, reverb_room_size=0.9, delay=True)
    assert np.array_equal(out, raw * 0.5 + 1.0) and len(calls) == 1                                   # once, after the gate
    assert np.array_equal(calls[0][0], raw * 0.5) and calls[0][1] == 40000
    assert calls[0][2] == dict(reverb=True, reverb_room_size=0.9, delay=True)
    with pytest.raises(TypeError, match="no_such_keyword"):
        vc.convert_array(a, post_process=True, no_such_keyword=1)
    with pytest.raises(TypeError, match="reverb_size"):
        vc.convert_array(a, reverb_size=1)
    with pytest.raises(NotImplementedError, match="pitch_shift"):
        vc.convert_array(a, post_process=True, pitch_shift=True)
    assert len(calls) == 1
