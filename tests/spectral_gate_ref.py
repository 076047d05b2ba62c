"""The yardstick of K18 (csrc/spectralgate.hip): the non-stationary spectral gate of include/rvc_amd.h restated on SciPy.

Not a test module.  The noisereduce wheel is absent, so the specification in the header is the contract and this is its
executable form: float64 when the input is float64, and SciPy's own single-precision path (complex64 spectra) when it is float32 --
the distance between the two is the reference's own error, which the device tolerance is a multiple of.
"""
import numpy as np
from scipy import signal

N_FFT, HOP = 1024, 256
TIME_CONSTANT_S, THRESH, SLOPE = 2.0, 2, 10
FREQ_MASK_SMOOTH_HZ, TIME_MASK_SMOOTH_MS = 500, 50


def ramp(k):
    return np.concatenate([np.linspace(0, 1, k + 1, endpoint=False), np.linspace(1, 0, k + 2)])[1:-1]


def parameters(sr):
    """-> (nf, nt, b, filt)"""
    nf = int(FREQ_MASK_SMOOTH_HZ / (sr / (N_FFT / 2)))
    nt = int(TIME_MASK_SMOOTH_MS / ((HOP / sr) * 1000))
    t = TIME_CONSTANT_S * sr / HOP
    b = (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)
    filt = np.outer(ramp(nf), ramp(nt))
    return nf, nt, float(b), filt / filt.sum()


def filter_buffer(c, sr, prop_decrease):
    """One padded chunk buffer -> the filtered buffer of the same length and dtype family."""
    nf, nt, b, filt = parameters(sr)
    S = signal.stft(c, nfft=N_FFT, nperseg=N_FFT, noverlap=N_FFT - HOP, padded=False)[2]
    A = np.abs(S)
    M = signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
    live = M > 0                                            # a bin silent in every frame: X = 0, finite mask, zero output
    X = np.where(live, (A - M) / np.where(live, M, 1), 0)
    mask = 1 / (1 + np.exp(-(X - THRESH) * SLOPE))
    mask = signal.fftconvolve(mask, filt.astype(mask.dtype), mode="same")
    mask = mask * prop_decrease + (1 - prop_decrease)
    x = signal.istft(S * mask, nfft=N_FFT, nperseg=N_FFT, noverlap=N_FFT - HOP)[1]
    filtered = np.zeros(len(c), dtype=x.dtype)
    filtered[:len(x)] = x[:len(c)]
    return filtered


def reduce_noise_chunk(y, sr, prop_decrease, chunk_size, padding, s):
    """out[s:e] of the chunk that starts at sample s: it depends on y[s - padding : e + padding] alone."""
    n = len(y)
    e = min(s + chunk_size, n)
    c = np.zeros(e - s + 2 * padding, dtype=y.dtype)
    lo, hi = max(s - padding, 0), min(e + padding, n)
    c[lo - (s - padding):hi - (s - padding)] = y[lo:hi]
    return filter_buffer(c, sr, prop_decrease)[padding:padding + e - s]


def reduce_noise(y, sr, prop_decrease=1.0, chunk_size=600000, padding=30000):
    y = np.asarray(y)
    out = np.zeros(len(y), dtype=y.dtype)
    for s in range(0, len(y), chunk_size):
        out[s:s + chunk_size] = reduce_noise_chunk(y, sr, prop_decrease, chunk_size, padding, s)
    return out


def test_signal(n, sr, seed=1234):
    """0.5 sin(2 pi 220 t) switched on and off by the sign of a 3 Hz sine, plus 0.02 N(0, 1): float64."""
    t = np.arange(n) / sr
    tone = 0.5 * np.sin(2 * np.pi * 220 * t) * (np.sin(2 * np.pi * 3 * t) > 0)
    return tone + 0.02 * np.random.default_rng(seed).standard_normal(n)


test_signal.__test__ = False


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64))))) if len(v) else 0.0
