"""Float64 NumPy restatement of K21 (include/rvc_amd.h): the SOLA join of two consecutive vocoder outputs and the window rule of a
stream's carried input.  The reference has no streaming mode, so this file is the yardstick of csrc/sola.hip."""
import numpy as np


def test_signal(n, seed=0, lo=0.02, hi=0.5, peak=0.5):
    """Band-limited seeded noise, float32, peak `peak`: white noise whose spectrum is kept between lo and hi of the Nyquist
    frequency (n == 1: one sample of that peak).  Band-limited like a vocoder's output, so that neighbouring lags correlate."""
    rng = np.random.default_rng(seed)
    if n < 4:
        x = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    else:
        spec = np.fft.rfft(rng.standard_normal(n))
        k = np.arange(spec.shape[0]) / (spec.shape[0] - 1)
        spec[(k < lo) | (k > hi)] = 0.0
        x = np.fft.irfft(spec, n)
    return (x * (peak / np.abs(x).max())).astype(np.float32)


test_signal.__test__ = False   # a helper, not a test


def fade_in(xfade):
    """sin^2(pi i / (2 X)) in float64, rounded to float32: what the caller uploads."""
    return (np.sin(np.pi * np.arange(xfade, dtype=np.float64) / (2.0 * xfade)) ** 2).astype(np.float32)


def scores(infer, buf, search):
    """score(o) = sum_i infer[o + i] buf[i] / sqrt(sum_i infer[o + i]^2 + 1e-8), o = 0 .. search, in float64."""
    infer, buf = np.asarray(infer, dtype=np.float64), np.asarray(buf, dtype=np.float64)
    x = buf.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(infer, x)[:search + 1]
    return (win @ buf) / np.sqrt((win * win).sum(axis=1) + 1e-8)


def tau(buf):
    """The score difference fp32 accumulation can hide: 2 X 2^-24 ||buf||_2 (X products of a score bounded by ||buf||_2)."""
    buf = np.asarray(buf, dtype=np.float64)
    return 2.0 * buf.shape[0] * 2.0 ** -24 * float(np.sqrt((buf * buf).sum()))


def sola(infer, buf, fade, search, block, offset=None):
    """Steps 1 to 4 -> (out float64 [block], new buf (the dtype of infer) [X], offset, the scores).  `offset`: use this lag instead
    of the arg-max (the tie-aware comparisons evaluate the restatement at the device's choice)."""
    infer = np.asarray(infer)
    x = np.asarray(buf).shape[0]
    assert 1 <= x <= block and search >= 0 and infer.shape[0] == block + x + search
    sc = scores(infer, buf, search)
    if offset is None:
        offset = int(np.argmax(sc))                   # the first of equal maxima: the lowest lag
    f = np.asarray(fade, dtype=np.float64)
    out = infer[offset:offset + block].astype(np.float64)
    out[:x] = out[:x] * f + np.asarray(buf, dtype=np.float64) * (1.0 - f)
    return out, infer[offset + block:offset + block + x].copy(), offset, sc


def window(hist, block):
    """-> (window = [hist | block], the new hist = the window's last len(hist) samples)."""
    w = np.concatenate([hist, block])
    return w, w[w.shape[0] - hist.shape[0]:].copy()


def planted(x, s, b, lag, seed):
    """infer = test_signal(b + x + s, seed) and buf = infer[lag : lag + x]: the score's maximum is at `lag`, strictly
    (Cauchy-Schwarz: any other lag's segment is not a positive multiple of buf)."""
    infer = test_signal(b + x + s, seed)
    return infer, infer[lag:lag + x].copy()


# (X, S, B, planted lag, seed): the kernel-parity cases of tests/test_stream_gpu.py; tests/test_stream_cpu.py proves on the host that
# each one's maximum is isolated by more than tau, so that the device must find exactly the planted lag
PLANTED = [(1, 0, 1, 0, 1), (320, 320, 640, 137, 2), (400, 400, 800, 0, 3), (400, 400, 800, 1, 4), (400, 400, 800, 199, 5),
           (400, 400, 800, 400, 6), (2400, 480, 12000, 311, 7)]
