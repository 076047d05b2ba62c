"""The yardstick of K22 (csrc/effects.hip): a NumPy restatement of the effects specified in include/rvc_amd.h, "K22", as plain
sequential recurrences (vectorised only over samples that do not depend on one another: a block no longer than the shortest
feedback path).  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs the very same statements in float32 and
measures what single precision costs, which is what the device is allowed a small multiple of.

Constants derived from parameters (10^(dB / 20), 1 - mix, 1 - damp, the ballistics coefficients ...) are formed in float64 and
rounded to ``dtype`` once, as the library forms them on the host.  The chorus tap positions are float64 in both modes."""
import numpy as np

COMB_T = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_T = (556, 441, 341, 225)


def db_to_gain(db):
    return 10.0 ** (db / 20.0)


def signal(n, sr, seed=0, peak=0.8):
    """A voiced-like test signal: a few harmonics with a slow loudness contour, some noise, quiet stretches; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) for f in (110.0, 220.0, 331.0, 1870.0, 5210.0))
    x = x * (0.15 + np.abs(np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6.28)))) + 0.05 * rng.standard_normal(n)
    return (x * (peak / max(np.abs(x).max(), 1e-30))).astype(np.float32)


# ---- pointwise ----------------------------------------------------------------------------------------------------------------------
def gain(x, gain_db, dtype=np.float64):
    return x.astype(dtype) * dtype(db_to_gain(gain_db))


def distortion(x, drive_db, dtype=np.float64):
    return np.tanh(x.astype(dtype) * dtype(db_to_gain(drive_db)))


def bitcrush(x, bit_depth, dtype=np.float64):
    scale = dtype(2.0 ** bit_depth)
    return np.rint(x.astype(dtype) * scale) / scale


def clipping(x, threshold_db, dtype=np.float64):
    t = dtype(db_to_gain(threshold_db))
    return np.clip(x.astype(dtype), -t, t)


# ---- delay --------------------------------------------------------------------------------------------------------------------------
def delay(x, sr, delay_seconds, feedback, mix, dtype=np.float64):
    x = x.astype(dtype)
    n, D = len(x), int(np.floor(delay_seconds * sr))
    assert D >= 1
    fb, dry, wet = dtype(feedback), dtype(1.0 - mix), dtype(mix)
    d = np.zeros(n, dtype)
    for s in range(D, n, D):                       # d[s .. s + D) depends on d[s - D .. s) only
        e = min(s + D, n)
        d[s:e] = x[s - D:e - D] + fb * d[s - D:e - D]
    return dry * x + wet * d


# ---- chorus -------------------------------------------------------------------------------------------------------------------------
def chorus_taps(n, sr, rate_hz, depth, centre_delay_ms):
    """-> (i, f): the integer and fractional tap delay of every sample, float64."""
    m = np.arange(n, dtype=np.float64)
    ph = rate_hz * m / float(sr)
    ph -= np.floor(ph)
    lfo = np.sin(6.283185307179586 * ph)
    ms = np.maximum(1.0, centre_delay_ms + (10.0 * depth) * lfo)
    dl = ms * float(sr) / 1000.0
    i = np.floor(dl)
    return i.astype(np.int64), dl - i


def chorus(x, sr, rate_hz, depth, centre_delay_ms, feedback, mix, dtype=np.float64):
    x = x.astype(dtype)
    n = len(x)
    if n == 0:
        return x
    i, f = chorus_taps(n, sr, rate_hz, depth, centre_delay_ms)
    f = f.astype(dtype)
    fb, dry, wet = dtype(feedback), dtype(1.0 - mix), dtype(mix)
    p = np.zeros(n + 1, dtype)                     # p[-1] (= index n) stays 0: every negative index reads a zero
    w = np.zeros(n, dtype)
    block = int(i.min())                           # w[s .. s + block) reads p[< s] only
    idx = np.arange(n)
    for s in range(0, n, block):
        e = min(s + block, n)
        m0 = idx[s:e] - i[s:e]
        m1 = m0 - 1
        p0 = np.where(m0 >= 0, p[np.maximum(m0, 0)], dtype(0))
        p1 = np.where(m1 >= 0, p[np.maximum(m1, 0)], dtype(0))
        w[s:e] = p0 + f[s:e] * (p1 - p0)
        w_prev = np.concatenate([w[s - 1:s] if s else np.zeros(1, dtype), w[s:e - 1]])
        p[s:e] = x[s:e] - fb * w_prev
    return dry * x + wet * w


# ---- reverb -------------------------------------------------------------------------------------------------------------------------
def reverb_lengths(sr):
    return [sr * t // 44100 for t in COMB_T], [sr * t // 44100 for t in ALLPASS_T]


def reverb_constants(room_size, damping, wet_level, dry_level, width, freeze_mode):
    """-> (in_gain, damp, feedback, wet1, dry), float64."""
    frozen = freeze_mode >= 0.5
    return (0.0 if frozen else 0.015, 0.0 if frozen else 0.4 * damping, 1.0 if frozen else 0.28 * room_size + 0.7,
            1.5 * wet_level * (1.0 + width), 2.0 * dry_level)


def reverb(x, sr, room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0, freeze_mode=0.0, dtype=np.float64):
    x = x.astype(dtype)
    n = len(x)
    in_gain, damp, feedback, wet1, dry = reverb_constants(room_size, damping, wet_level, dry_level, width, freeze_mode)
    damp1, damp, feedback, wet1, dry = dtype(1.0 - damp), dtype(damp), dtype(feedback), dtype(wet1), dtype(dry)
    inp = dtype(in_gain) * x
    combs, allpasses = reverb_lengths(sr)
    total = np.zeros(n, dtype)
    for L in combs:                                # line[idx] at time m holds what was stored at m - L
        line, last, out = np.zeros(L, dtype), dtype(0), np.zeros(n, dtype)
        for m in range(n):
            idx = m % L
            o = line[idx]
            last = o * damp1 + last * damp
            line[idx] = inp[m] + last * feedback
            out[m] = o
        total = total + out
    half = dtype(0.5)
    for M in allpasses:                            # a block of M samples reads the line as the block before left it
        line, out = np.zeros(M, dtype), np.zeros(n, dtype)
        for s in range(0, n, M):
            e = min(s + M, n)
            b = line[:e - s].copy()
            line[:e - s] = total[s:e] + half * b
            out[s:e] = b - total[s:e]
        total = out
    return total * wet1 + x * dry


# ---- compressor / limiter -----------------------------------------------------------------------------------------------------------
def ballistics(sr, t_ms):
    return 0.0 if t_ms <= 1e-3 else float(np.exp(-2.0 * np.pi * 1000.0 / (float(sr) * t_ms)))


def envelope(x, sr, attack_ms, release_ms, dtype=np.float64):
    c_at, c_rl = dtype(ballistics(sr, attack_ms)), dtype(ballistics(sr, release_ms))
    a = np.abs(x.astype(dtype))
    env, e = np.zeros(len(x), dtype), dtype(0)
    for m in range(len(x)):
        am = a[m]
        e = am + (c_at if am > e else c_rl) * (e - am)
        env[m] = e
    return env


def compressor(x, sr, threshold_db=0.0, ratio=1.0, attack_ms=1.0, release_ms=100.0, dtype=np.float64):
    x = x.astype(dtype)
    env = envelope(x, sr, attack_ms, release_ms, dtype)
    thr, expo = dtype(db_to_gain(threshold_db)), dtype(1.0 / ratio - 1.0)
    g = np.where(env < thr, dtype(1), np.power(np.maximum(env, thr) / thr, expo))
    return g * x


def limiter(x, sr, threshold_db=-6.0, release_ms=0.05, dtype=np.float64):
    y = compressor(x, sr, -10.0, 4.0, 2.0, 200.0, dtype)
    y = compressor(y, sr, threshold_db, 1000.0, 0.001, release_ms, dtype)
    y = y * dtype(10.0 ** (7.5 / 40.0) * 10.0 ** (-threshold_db / 20.0))
    return np.clip(y, dtype(-1), dtype(1))


# ---- the board ----------------------------------------------------------------------------------------------------------------------
# the reference's chain (rvc/infer/infer.py:130-191): (switch, effect, wants sr, [(keyword, default), ...] in the effect's argument order)
CHAIN = (
    ("reverb", reverb, True, [("reverb_room_size", 0.5), ("reverb_damping", 0.5), ("reverb_wet_level", 0.33), ("reverb_dry_level", 0.4),
                              ("reverb_width", 1.0), ("reverb_freeze_mode", 0)]),
    ("limiter", limiter, True, [("limiter_threshold", -6), ("limiter_release", 0.05)]),
    ("gain", gain, False, [("gain_db", 0)]),
    ("distortion", distortion, False, [("distortion_gain", 25)]),
    ("chorus", chorus, True, [("chorus_rate", 1.0), ("chorus_depth", 0.25), ("chorus_delay", 7), ("chorus_feedback", 0.0), ("chorus_mix", 0.5)]),
    ("bitcrush", bitcrush, False, [("bitcrush_bit_depth", 8)]),
    ("clipping", clipping, False, [("clipping_threshold", 0)]),
    ("compressor", compressor, True, [("compressor_threshold", 0), ("compressor_ratio", 1), ("compressor_attack", 1.0),
                                      ("compressor_release", 100)]),
    ("delay", delay, True, [("delay_seconds", 0.5), ("delay_feedback", 0.0), ("delay_mix", 0.5)]),
)


def post_process(x, sr, dtype=np.float64, **kw):
    """The board with the reference's keyword names, defaults and order; pitch_shift (between reverb and limiter) is not built."""
    assert not kw.get("pitch_shift", False)
    for switch, effect, wants_sr, args in CHAIN:
        if kw.get(switch, False):
            x = effect(x, *((sr,) if wants_sr else ()), *(kw.get(k, d) for k, d in args), dtype=dtype)
    return x.astype(dtype)


def tolerance(ref32, ref64):
    """The bound of every device-vs-float64 comparison: four times what the float32 run of this file deviates by on the same
    input, with a floor of 2^-21 of the output's peak."""
    return max(4.0 * float(np.abs(ref32.astype(np.float64) - ref64).max(initial=0.0)), 2.0 ** -21 * float(np.abs(ref64).max(initial=0.0)))
