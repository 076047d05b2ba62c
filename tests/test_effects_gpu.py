"""K22 (post_process, csrc/effects.hip) on the device against its float64 restatement (tests/effects_ref.py) on the same fp32
input.  The bound of every comparison is computed here, not chosen: four times what the restatement's own float32 run deviates
by on that input, with a floor of 2^-21 of the output's peak (effects_ref.tolerance) -- the device associates the recurrences
differently from a sequential float32 loop (scans, fused multiply-adds) and its tanhf / powf are a few ulp off.  Every test prints
its figures (device error, float32 error, their ratio, the bound) before it asserts."""
import functools

import numpy as np
import pytest
import torch

import effects_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _signal(n, sr, seed=0, peak=0.8):
    x = R.signal(n, sr, seed, peak)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _refs(effect, n, sr, args, seed=0, peak=0.8):
    """(ref64, ref32) of R.<effect>(signal(n, sr, seed, peak), [sr,] *args), computed once and shared."""
    x, fn = _signal(n, sr, seed, peak), getattr(R, effect)
    lead = () if effect in ("gain", "distortion", "bitcrush", "clipping") else (sr,)
    out = tuple(np.asarray(fn(x, *lead, *args, dtype=dt)) for dt in (np.float64, np.float32))
    assert out[0].dtype == np.float64 and out[1].dtype == np.float32
    for o in out:
        o.setflags(write=False)
    return out


def _compare(what, dev, ref64, ref32):
    dev = dev.cpu().numpy() if torch.is_tensor(dev) else dev
    assert dev.dtype == np.float32 and dev.shape == ref64.shape and np.isfinite(dev).all()
    tol = R.tolerance(ref32, ref64)
    e_dev = float(np.abs(dev.astype(np.float64) - ref64).max(initial=0.0))
    e_32 = float(np.abs(ref32.astype(np.float64) - ref64).max(initial=0.0))
    print(f"[effects] {what}: device {e_dev:.3e}  float32 restatement {e_32:.3e}  ratio {e_dev / e_32 if e_32 else float('nan'):.2f}  "
          f"bound {tol:.3e}  peak {np.abs(ref64).max(initial=0.0):.3f}")
    assert e_dev <= tol, (what, e_dev, tol)


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True)).cuda()


# ---- pointwise ----------------------------------------------------------------------------------------------------------------------
POINTWISE = dict(gain_db=-4.5, drive_db=25.0, bit_depth=6.5, clip_threshold_db=-3.0)
STAGE_FN = ((1, "gain", "gain_db"), (2, "distortion", "drive_db"), (4, "bitcrush", "bit_depth"), (8, "clipping", "clip_threshold_db"))


@functools.lru_cache(maxsize=None)
def _pointwise_refs(n, stages):
    out = []
    for dt in (np.float64, np.float32):
        y = _signal(n, 16000, seed=1)
        for bit, fn, key in STAGE_FN:
            if stages & bit:
                y = getattr(R, fn)(y, POINTWISE[key], dtype=dt)
        out.append(np.asarray(y, dtype=dt))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("stages", [1, 2, 4, 8, 3, 12, 15], ids=["gain", "distortion", "bitcrush", "clipping", "gain+distortion",
                                                                  "bitcrush+clipping", "all"])
def test_pointwise(native, n, stages):
    dev = native.fx_pointwise(_dev(_signal(n, 16000, seed=1)), stages, **POINTWISE)
    ref64, ref32 = _pointwise_refs(n, stages)
    if stages == 15:     # tanhf in front of the quantiser may move a sample across a step: the rule of the board with bitcrush below
        tol = R.tolerance(*_pointwise_refs(n, 3)[::-1])                    # of what enters the quantiser
        diff = np.abs(dev.cpu().numpy().astype(np.float64) - ref64)
        far = diff > tol
        print(f"[effects] pointwise stages {stages} n {n}: {int(far.sum())} of {n} samples beyond {tol:.3e}, max {diff.max():.3e}")
        assert diff.max() <= 2.0 ** -POINTWISE["bit_depth"] + tol and far.mean() <= 0.01
        return
    _compare(f"pointwise stages {stages} n {n}", dev, ref64, ref32)


@pytest.mark.parametrize("bits", [1, 8, 16, 24, 32])
def test_bitcrush_with_integer_depth_is_bit_exact(native, bits):
    x = _signal(4097, 16000, seed=1)
    dev = native.fx_pointwise(_dev(x), 4, bit_depth=bits).cpu().numpy()
    ref = R.bitcrush(x, bits)                     # x 2^b, the rounding and / 2^b are all exact in fp32 as in float64
    assert np.array_equal(dev.astype(np.float64), ref)
    assert np.array_equal(dev, R.bitcrush(x, bits, dtype=np.float32))


def test_pointwise_in_place_and_empty(native):
    x = _dev(_signal(4097, 16000, seed=1))
    want = native.fx_pointwise(x, 3, **POINTWISE)
    native._call("rvc_fx_pointwise_f32", x.device, x.data_ptr(), x.numel(), 3, -4.5, 25.0, 6.5, -3.0, x.data_ptr())
    assert torch.equal(x, want)
    assert native.fx_pointwise(torch.empty(0, device="cuda"), 15).numel() == 0


# ---- delay --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 7, 4000, 4001, 4006], ids=["1", "7", "n-1", "n", "n+5"])
def test_delay(native, D):
    n, sr, args = 4001, 16000, ((D + 0.5) / 16000, 0.5, 0.35)
    assert int(np.floor(args[0] * sr)) == D
    dev = native.fx_delay(_dev(_signal(n, sr)), sr, *args)
    _compare(f"delay D {D}", dev, *_refs("delay", n, sr, args))


# ---- chorus -------------------------------------------------------------------------------------------------------------------------
CHORUS = {   # (sr, rate_hz, depth, centre_delay_ms, feedback, mix)
    "fb=0": (16000, 3.0, 0.25, 7.0, 0.0, 0.5), "fb=0.5": (16000, 3.0, 0.25, 7.0, 0.5, 0.5), "fb=-0.5": (16000, 3.0, 0.25, 7.0, -0.5, 0.5),
    "floor,fb=0": (16000, 5.0, 1.0, 2.0, 0.0, 0.5), "floor,fb=0.5": (16000, 5.0, 1.0, 2.0, 0.5, 0.7),
    "48k,fb=0": (48000, 3.0, 0.25, 7.0, 0.0, 0.5), "48k,fb=0.5": (48000, 7.0, 0.25, 7.0, 0.5, 0.5),
}


@pytest.mark.parametrize("case", list(CHORUS))
def test_chorus(native, case):
    sr, *args = CHORUS[case]
    n = 8000
    if case.startswith("floor"):
        i, _ = R.chorus_taps(n, sr, *args[:3])
        assert i.min() == sr // 1000 and (i == sr // 1000).sum() > 100 and i.max() > 10 * sr // 1000   # the 1 ms floor is hit
    dev = native.fx_chorus(_dev(_signal(n, sr)), sr, *args)
    _compare(f"chorus {case}", dev, *_refs("chorus", n, sr, tuple(args)))


# ---- reverb -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [0.0, 1.0], ids=["live", "frozen"])
@pytest.mark.parametrize("sr", [16000, 48000])
@pytest.mark.parametrize("which", ["1", "D1-1", "D1", "D1+1", "5000"])
def test_reverb(native, which, sr, frozen):
    D1 = R.reverb_lengths(sr)[0][0]
    n = {"1": 1, "D1-1": D1 - 1, "D1": D1, "D1+1": D1 + 1, "5000": 5000}[which]
    args = (0.7, 0.4, 0.33, 0.4, 1.0, frozen)
    dev = native.fx_reverb(_dev(_signal(n, sr)), sr, *args)
    _compare(f"reverb n {n} sr {sr} frozen {frozen}", dev, *_refs("reverb", n, sr, args))


@pytest.mark.parametrize("sr", [16000, 48000])
def test_reverb_wet_alone(native, sr):
    """dry_level = 0: nothing but the combs and allpasses reaches the output, so the bound is a share of THEIR level"""
    args = (0.9, 0.2, 1.0, 0.0, 1.0, 0.0)
    dev = native.fx_reverb(_dev(_signal(5000, sr)), sr, *args)
    _compare(f"reverb wet alone sr {sr}", dev, *_refs("reverb", 5000, sr, args))


def test_reverb_impulse(native):
    sr, D1 = 16000, 404
    x = np.zeros(D1 + 50, dtype=np.float32)
    x[0] = 1.0
    y = native.fx_reverb(_dev(x), sr, 0.5, 0.5, 0.33, 0.0, 1.0, 0.0).cpu().numpy()
    assert not y[:D1].any() and y[D1] == np.float32(np.float32(0.015) * np.float32(0.99))


# ---- compressor / limiter -----------------------------------------------------------------------------------------------------------
COMPRESSOR = {   # (threshold_db, ratio, attack_ms, release_ms)
    "default-like": (-20.0, 4.0, 1.0, 100.0),
    "long release": (-30.0, 4.0, 1.0, 1e5),             # c_release = 1 - 4e-6: the upper probe hardly moves within 20000 samples
    "long both": (-60.0, 8.0, 1e5, 1e5),                # no chunk of any length closes: one lane walks the signal
    "hard knee": (-12.0, 1000.0, 0.0, 5.0),
}


@pytest.mark.parametrize("case", list(COMPRESSOR))
def test_compressor_does_not_depend_on_the_chunking(native, case):
    n, sr, args = 20000, 16000, COMPRESSOR[case]
    x = _dev(_signal(n, sr))
    outs = [native.fx_compressor(x, sr, *args, chunk=c) for c in (64, 1000, n, 0)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    _compare(f"compressor {case}", outs[0], *_refs("compressor", n, sr, args))


@pytest.mark.parametrize("args", [(-6.0, 0.05), (-12.0, 100.0), (-3.0, 1e5)], ids=["default", "slow", "long release"])
def test_limiter_does_not_depend_on_the_chunking(native, args):
    n, sr = 20000, 16000
    x = _dev(_signal(n, sr, peak=2.5))
    outs = [native.fx_limiter(x, sr, *args, chunk=c) for c in (64, 1000, n, 0)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert float(outs[0].abs().max()) <= 1.0
    _compare(f"limiter {args}", outs[0], *_refs("limiter", n, sr, args, peak=2.5))


def test_compressor_with_ratio_one_is_the_identity(native):
    x = _dev(_signal(20000, 16000))
    assert torch.equal(native.fx_compressor(x, 16000, -40.0, 1.0, 1.0, 100.0), x)


# ---- the board ----------------------------------------------------------------------------------------------------------------------
BOARD = dict(reverb=True, reverb_room_size=0.6, limiter=True, gain=True, gain_db=-2.0, distortion=True, distortion_gain=6.0,
             chorus=True, chorus_feedback=0.3, clipping=True, clipping_threshold=-1.0, compressor=True, compressor_threshold=-18.0,
             compressor_ratio=3.0, delay=True, delay_seconds=0.11, delay_feedback=0.4)
BOARD_N, BOARD_SR, BOARD_SEED = 16000, 40000, 11


@functools.lru_cache(maxsize=None)
def _board_refs(bitcrush):
    kw = dict(BOARD, bitcrush=True, bitcrush_bit_depth=8) if bitcrush else BOARD
    x = _signal(BOARD_N, BOARD_SR, BOARD_SEED)
    return R.post_process(x, BOARD_SR, np.float64, **kw), R.post_process(x, BOARD_SR, np.float32, **kw)


def test_board_in_the_reference_order_on_a_tensor_and_on_an_array(native):
    from rvc_amd.infer.infer import VoiceConverter
    x = _signal(BOARD_N, BOARD_SR, BOARD_SEED)
    ref64, ref32 = _board_refs(False)
    on_tensor = VoiceConverter.post_process_audio(_dev(x), BOARD_SR, **BOARD)
    assert torch.is_tensor(on_tensor) and on_tensor.is_cuda and on_tensor.dtype == torch.float32
    _compare("board (tensor)", on_tensor, ref64, ref32)
    on_array = VoiceConverter.post_process_audio(x.astype(np.float64), BOARD_SR, **BOARD)
    assert isinstance(on_array, np.ndarray) and on_array.dtype == np.float32
    assert np.array_equal(on_array, on_tensor.cpu().numpy())               # two calls give identical bits, whichever way in
    _compare("board (array)", on_array, ref64, ref32)


def test_board_with_bitcrush_stays_within_one_quantum(native):
    from rvc_amd.infer.infer import VoiceConverter
    kw = dict(BOARD, bitcrush=True, bitcrush_bit_depth=8)
    ref64, ref32 = _board_refs(True)
    tol = R.tolerance(*_board_refs(False)[::-1])
    # upstream rounding can move a sample across a quantisation step; the seed keeps the restatement's own float32 run under 0.5 %
    assert (np.abs(ref32.astype(np.float64) - ref64) > tol).mean() < 0.005
    dev = VoiceConverter.post_process_audio(_dev(_signal(BOARD_N, BOARD_SR, BOARD_SEED)), BOARD_SR, **kw).cpu().numpy()
    diff = np.abs(dev.astype(np.float64) - ref64)
    far = diff > tol
    print(f"[effects] board with bitcrush: {int(far.sum())} of {BOARD_N} samples beyond {tol:.3e}, max {diff.max():.3e}")
    # one quantum of 2^-8: what follows the quantiser (clipping, a compressor with gain <= 1, a delay that adds half a sample to half
    # of an echo) does not stretch the step of an isolated sample
    assert diff.max() <= 2.0 ** -8 + tol and far.mean() <= 0.01


def test_two_calls_give_identical_bits(native):
    n, sr = 20000, 16000
    x = _dev(_signal(n, sr))
    for run in (lambda: native.fx_reverb(x, sr, 0.7, 0.4, 0.33, 0.4, 1.0, 0.0), lambda: native.fx_chorus(x, sr, 3.0, 0.25, 7.0, 0.5, 0.5),
                lambda: native.fx_chorus(x, sr, 3.0, 0.25, 7.0, 0.0, 0.5), lambda: native.fx_delay(x, sr, 0.01, 0.5, 0.5),
                lambda: native.fx_compressor(x, sr, -20.0, 4.0, 1.0, 100.0), lambda: native.fx_limiter(x, sr, -6.0, 0.05),
                lambda: native.fx_pointwise(x, 15, **POINTWISE)):
        a = run()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            b = run()
        side.synchronize()
        assert torch.equal(a, b)


def test_convert_array_keyword_reaches_the_device_board(native):
    """convert_array(post_process=True, ...) with the pipeline stubbed: the board runs on the converter's device tensor."""
    from rvc_amd.infer.infer import VoiceConverter
    raw = _dev(_signal(BOARD_N, BOARD_SR, BOARD_SEED))

    class Pipe:
        trim_vocoder_pad = True

        def pipeline(self, **kw):
            return raw.clone()
    vc = VoiceConverter.__new__(VoiceConverter)
    vc.vc, vc.tgt_sr, vc.hubert_model, vc.net_g, vc.use_f0, vc.version, vc.trim_vocoder_pad = Pipe(), BOARD_SR, None, None, 1, "v2", True
    vc.config = type("C", (), {"device": "cuda:0"})()
    out = vc.convert_array(torch.zeros(1600, device="cuda"), post_process=True, **BOARD)
    assert torch.equal(out, VoiceConverter.post_process_audio(raw, BOARD_SR, **BOARD))
    assert torch.equal(vc.convert_array(torch.zeros(1600, device="cuda")), raw)
