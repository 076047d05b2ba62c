"""The yardstick of K19 (csrc/formant.hip): the formant shifter of include/rvc_amd.h restated on scipy.fft.

Not a test module.  The stftpitchshift wheel is absent, so the specification in the header is the contract and this is its
executable form: float64 when the input is float64, and scipy.fft's own single-precision path (complex64 spectra, float32
logarithms and powers) when it is float32 -- the distance between the two is the reference's own error, which the device
tolerance is a multiple of.  ``vocoder=True`` adds the wheel's phase-vocoder encode / decode round trip at factors = 1, which is
the identity on the phase modulo 2 pi and which the device does not build.
"""
import numpy as np
from scipy import fft as sfft

N, H, B = 1024, 32, 513


def not_normal(v):
    return ~np.isfinite(v) | (np.abs(v) < np.finfo(v.dtype).tiny)


def resample(E, d):
    """Linear resampling of the rows of E [frames, B] by the factor d, the wheel's way: positions in float64."""
    m = int(B * d)
    out = np.zeros_like(E)
    i = np.arange(min(B, m))
    pos = i * (B / m)
    j = np.trunc(pos).astype(int)
    f = (pos - j).astype(E.dtype)
    ok = j < B - 1
    i, j, f = i[ok], j[ok], f[ok]
    out[:, i] = f * E[:, j + 1] + (1 - f) * E[:, j]
    return out


def wrap(p):
    return p - 2 * np.pi * np.floor(p / (2 * np.pi) + 0.5)


def spectrum(x, sr=16000, quefrency_s=0.8e-3, distortion=0.8, vocoder=False):
    """-> (S, Y): the forward-scaled STFT [frames, B] of x and the output spectrum of step 4."""
    x = np.asarray(x)
    dt = x.dtype
    assert dt in (np.float32, np.float64) and x.ndim == 1 and len(x) >= N
    F = (len(x) - N) // H + 1
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(dt)
    S = sfft.rfft(x[np.arange(F)[:, None] * H + np.arange(N)[None, :]] * w, axis=-1, norm="forward")
    mag = np.abs(S)
    Q = int(quefrency_s * sr)
    with np.errstate(all="ignore"):
        if Q > 0:
            c = sfft.irfft(np.log10(mag), n=N, axis=-1, norm="forward")
            c[:, 1:Q] *= 2
            c[:, Q + 1:] = 0
            E = 10 ** sfft.rfft(c, axis=-1, norm="forward").real
            mask1 = not_normal(E)
            G = mag / E
            G[mask1] = 0
            if distortion != 1:
                E[mask1] = 0
                E = resample(E, distortion)
            mask2 = not_normal(E)
            G = G * E
            G[mask2] = 0
        else:
            G = mag
        unit = np.where(mag > 0, S / np.where(mag > 0, mag, 1), 0)
    assert G.dtype == dt and S.dtype == (np.complex64 if dt == np.float32 else np.complex128)
    if vocoder:   # encode: phase -> frequency estimate; decode: frequency estimate -> accumulated phase
        k = np.arange(B)
        phase_inc, freq_inc = 2 * np.pi * H / N, sr / N
        delta = np.diff(np.angle(S), axis=0, prepend=np.zeros((1, B)))
        freq = (k + wrap(delta - k * phase_inc) / phase_inc) * freq_inc
        arg = np.cumsum((k + (freq - k * freq_inc) / freq_inc) * phase_inc, axis=0)
        unit = np.where(mag > 0, np.exp(1j * arg), 0).astype(S.dtype)
    return S, (G * unit).astype(S.dtype)


def shift_formants(x, sr=16000, quefrency_s=0.8e-3, distortion=0.8, vocoder=False):
    """x [n] (float32 or float64) -> the shifted signal [n] of the same dtype."""
    x = np.asarray(x)
    dt = x.dtype
    Y = spectrum(x, sr, quefrency_s, distortion, vocoder)[1]
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    y = sfft.irfft(Y, n=N, axis=-1, norm="forward") * (w * H / np.sum(w * w)).astype(dt)
    assert y.dtype == dt
    out = np.zeros(len(x), dtype=dt)
    for t in range(len(y)):                    # frame order
        out[t * H:t * H + N] += y[t]
    return out


def test_signal(n, sr=16000, seed=1234):
    """A 140 Hz harmonic stack (29 partials, amplitudes 1 / h) under a 3 Hz amplitude modulation, peak 0.3, plus 0.02 N(0, 1):
    float64.  No STFT bin is near zero, so log10 is well conditioned."""
    t = np.arange(n) / sr
    stack = sum(np.sin(2 * np.pi * 140 * h * t) / h for h in range(1, 30)) * (0.75 + 0.25 * np.sin(2 * np.pi * 3 * t))
    return 0.3 * stack / np.abs(stack).max() + 0.02 * np.random.default_rng(seed).standard_normal(n)


test_signal.__test__ = False


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64))))) if len(v) else 0.0
