"""The yardstick of K23 (csrc/specfeat.hip): the analyzer's spectral features of include/rvc_amd.h restated on scipy.fft.

Not a test module.  librosa is absent, so the specification in the header is the contract and this is its executable form:
float64 throughout when the input is float64, and scipy.fft's own single-precision path (complex64 spectra, float32 magnitudes,
float32 squares and logarithms of the dB plane) when it is float32 -- the distance between the two is the reference's own error,
which the device tolerance is a multiple of.  The per-frame sums are float64 in both paths, as the contract has them.
"""
import numpy as np
from scipy import fft as sfft

N, H, B = 2048, 512, 1025


def magnitudes(x):
    """x [n] (float32 or float64) -> |S| [F, B] of the same dtype: center=True, zero padding, periodic Hann, unscaled rDFT."""
    x = np.asarray(x)
    dt = x.dtype
    assert dt in (np.float32, np.float64) and x.ndim == 1 and len(x) >= 1
    F = 1 + len(x) // H
    xpad = np.concatenate([np.zeros(N // 2, dt), x, np.zeros(N // 2, dt)])
    frames = np.lib.stride_tricks.sliding_window_view(xpad, N)[::H]
    assert frames.shape[0] == F
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(dt)
    m = np.abs(sfft.rfft(frames * w, axis=-1))
    assert m.dtype == dt and m.shape == (F, B)
    return m


def amplitude_to_db(m):
    """amplitude_to_db(m, ref=np.max) in m's dtype."""
    m = np.asarray(m)
    amin = m.dtype.type(1e-10)
    R = m.max()
    db = 10 * np.log10(np.maximum(amin, m * m)) - 10 * np.log10(np.maximum(amin, R * R))
    db = np.maximum(db, db.max() - 80)
    assert db.dtype == m.dtype
    return db


def features(x, sr, roll_percent=0.85, db=False):
    """-> dict: mag [F, B] (x's dtype); cent, bw, rolloff [F] float64 in Hz; rolloff_bin [F]; s0 [F]; cumn [F, B], the cumulative
    sums over s0 (over 1 for a silent frame); margin [F] = min_k |cumsum_k - roll_percent s0| / s0, inf for a frame of digital
    silence (its roll-off bin is 0 by 0 >= 0, which no rounding can move); db [F, B] on request."""
    m = magnitudes(x)
    m64 = m.astype(np.float64)
    f = np.arange(B) * sr / N
    s0 = m64.sum(axis=-1)
    den = np.where(s0 < np.finfo(np.float32).tiny, 1.0, s0)[:, None]
    mn = m64 / den
    cent = (f * mn).sum(axis=-1)
    bw = np.sqrt((mn * (f[None, :] - cent[:, None]) ** 2).sum(axis=-1))
    cum = np.cumsum(m64, axis=-1)
    thr = roll_percent * s0
    k = np.argmax(cum >= thr[:, None], axis=-1)          # the first bin at or above the threshold; cum[-1] >= thr always
    k = np.where((cum >= thr[:, None]).any(axis=-1), k, B - 1)
    pos = np.where(s0 > 0, s0, 1.0)
    margin = np.where(s0 > 0, np.abs(cum - thr[:, None]).min(axis=-1) / pos, np.inf)
    out = {"mag": m, "cent": cent, "bw": bw, "rolloff": f[k], "rolloff_bin": k, "s0": s0, "cumn": cum / pos[:, None], "margin": margin}
    if db:
        out["db"] = amplitude_to_db(m)
    return out


def native_stand_in(x, sr, roll_percent=0.85, want_mag=False, want_db=False):
    """The signature of rvc_amd._native.spectral_features on host tensors, for the tests that run without a device."""
    import torch
    r = features(x.detach().cpu().numpy().astype(np.float32), sr, roll_percent, db=want_db)
    t = torch.from_numpy
    return (t(r["cent"]), t(r["bw"]), t(r["rolloff"]), t(np.ascontiguousarray(r["mag"])) if want_mag else None,
            t(np.ascontiguousarray(r["db"])) if want_db else None)
