"""The float64 restatement of K24 (the conversion scorer, csrc/convscore.hip) as include/rvc_amd.h spells it out: mel cepstra
via np.fft.rfft, dynamic time warping walked along anti-diagonals (so that 2049 x 1900 takes about a second), the F0 tracking
sums and the figures finished from them.  ``melcep_torch`` evaluates the same cepstra in torch at a given dtype: its fp32 error
against float64 is the e_ref the GPU gate is a multiple of.  Also the seeded test signals."""
import math

import numpy as np
import torch

N_FFT = 1024
BINS = 513
MCD_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)
GROSS_CENTS = 1200.0 * math.log2(1.2)


def mel_matrix(sr, n_mels=80):
    from rvc_amd.train.mel_processing import librosa_mel_fn
    return np.ascontiguousarray(librosa_mel_fn(int(sr), N_FFT, int(n_mels), 0, sr / 2), dtype=np.float32)


def frames(x, sr):
    """-> [T, 1024]: frame t covers samples [t hop - 512, t hop + 512) of x extended with zeros; T = 1 + n // hop"""
    hop = sr // 200
    n = len(x)
    T = 1 + n // hop
    xp = np.concatenate([np.zeros(512, x.dtype), x, np.zeros(512 + hop, x.dtype)])
    idx = np.arange(T)[:, None] * hop + np.arange(N_FFT)[None, :]
    return xp[idx]


def dct_matrix(n_mels, n_coef):
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.cos(np.pi * k * (2 * m + 1) / (2 * n_mels)) / n_mels          # [n_coef, n_mels]


def melcep(x, sr, n_mels=80, n_coef=24, mel=None):
    """float64 NumPy: x (any float dtype; the device sees its float32 rounding, so pass that) -> c [T, n_coef]"""
    x = np.asarray(x, dtype=np.float64)
    mel = mel_matrix(sr, n_mels) if mel is None else mel
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    S = np.fft.rfft(frames(x, sr) * w, axis=1)
    P = S.real ** 2 + S.imag ** 2
    M = P @ mel.astype(np.float64).T
    L = 0.5 * np.log(np.maximum(M, 1e-10))
    return L @ dct_matrix(mel.shape[0], n_coef).T


def melcep_torch(x, sr, dtype, n_mels=80, n_coef=24, mel=None):
    """the same formulas in torch at `dtype` (window, rfft, filterbank, log and DCT all at that precision) -> float64 NumPy"""
    mel = mel_matrix(sr, n_mels) if mel is None else mel
    xt = torch.from_numpy(frames(np.asarray(x, dtype=np.float64), sr)).to(dtype)
    w = (0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(N_FFT, dtype=torch.float64) / N_FFT)).to(dtype)
    S = torch.fft.rfft(xt * w, dim=1)
    P = S.real ** 2 + S.imag ** 2
    M = P @ torch.from_numpy(mel).to(dtype).T
    L = 0.5 * torch.log(torch.clamp(M, min=1e-10))
    return (L @ torch.from_numpy(dct_matrix(mel.shape[0], n_coef)).to(dtype).T).to(torch.float64).numpy()


# ---- DTW ---------------------------------------------------------------------------------------------------------------------------
def admissible(i, j, Ta, Tb, band):
    if band is None or band < 0 or Ta == 1 or Tb == 1:
        return np.ones(np.broadcast(i, j).shape, dtype=bool)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return np.abs(j * (Ta - 1) - i * (Tb - 1)) <= band * max(Ta - 1, Tb - 1)


def frame_dist(a, b):
    """sqrt(sum_q (a_q - b_q)^2) in float64, the terms added in the order of q"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    acc = np.zeros(d.shape[0])
    for q in range(d.shape[1]):
        acc += d[:, q] * d[:, q]
    return np.sqrt(acc)


def dtw(a, b, band=None):
    """-> (D(Ta-1, Tb-1), path int [L, 2]).  Predecessors tried in the order (i-1, j-1), (i-1, j), (i, j-1); a later one replaces
    the best only when strictly smaller."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    Ta, Tb = len(a), len(b)
    D = np.full((Ta + 1, Tb + 1), np.inf)           # D[i + 1, j + 1] = D(i, j); row 0 and column 0 are the outside
    code = np.zeros((Ta, Tb), dtype=np.uint8)
    for k in range(Ta + Tb - 1):
        i = np.arange(max(0, k - Tb + 1), min(Ta - 1, k) + 1)
        j = k - i
        d = frame_dist(a[i], b[j])
        best = D[i, j].copy()
        c = np.zeros(len(i), dtype=np.uint8)
        up = D[i, j + 1]
        m = up < best
        best[m], c[m] = up[m], 1
        left = D[i + 1, j]
        m = left < best
        best[m], c[m] = left[m], 2
        val = d + best
        if k == 0:
            val = d
        val[~admissible(i, j, Ta, Tb, band)] = np.inf
        D[i + 1, j + 1] = val
        code[i, j] = c
    i, j = Ta - 1, Tb - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        c = 2 if i == 0 else 1 if j == 0 else code[i, j]
        if c == 0:
            i, j = i - 1, j - 1
        elif c == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return float(D[Ta, Tb]), np.array(path[::-1], dtype=np.int64)


def path_cost(a, b, path):
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    return float(math.fsum(frame_dist(a[path[:, 0]], b[path[:, 1]])))


def check_path(path, Ta, Tb, band=None):
    """the ends, the steps and the band of a warping path"""
    path = np.asarray(path)
    assert path.ndim == 2 and path.shape[1] == 2 and max(Ta, Tb) <= len(path) <= Ta + Tb - 1, path.shape
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (Ta - 1, Tb - 1)
    step = np.diff(path, axis=0)
    assert ((step == (1, 1)).all(1) | (step == (1, 0)).all(1) | (step == (0, 1)).all(1)).all()
    assert admissible(path[:, 0], path[:, 1], Ta, Tb, band).all()


def mcd_dtw(cx, cy, band=None):
    cost, path = dtw(cx, cy, band)
    return MCD_CONST * cost / len(path)


def mcd_aligned(cx, cy):
    T = min(len(cx), len(cy))
    return MCD_CONST * float(frame_dist(cx[:T], cy[:T]).sum()) / T


# ---- F0 ----------------------------------------------------------------------------------------------------------------------------
def f0_sums(fa, fb):
    """the twelve sums of rvc_f0_track_sums_f64"""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        va, vb = fa > 0, fb > 0
    both = va & vb
    a, b = fa[both], fb[both]
    la, lb, r = np.log2(a), np.log2(b), 1200.0 * np.log2(b / a)
    n = int(both.sum())
    rbar = math.fsum(r) / n if n else 0.0
    e = r - rbar
    return np.array([n, math.fsum(r), math.fsum(la), math.fsum(lb), math.fsum(la * la), math.fsum(lb * lb), math.fsum(la * lb),
                     math.fsum(e * e), int((np.abs(e) > GROSS_CENTS).sum()), int((va & ~vb).sum()), int((vb & ~va).sum()),
                     int((~va & ~vb).sum())], dtype=np.float64)


def f0_errors(fa, fb):
    """the figures straight from the contours (no sums): the definition the host's finishing arithmetic is checked against"""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        va, vb = fa > 0, fb > 0
    both = va & vb
    la, lb = np.log2(fa[both]), np.log2(fb[both])
    r = 1200.0 * np.log2(fb[both] / fa[both])
    e = r - r.mean()
    return {"voiced_frames": int(both.sum()), "vuv_error": float((va != vb).sum()) / len(fa), "shift_semitones": float(r.mean() / 100.0),
            "f0_rmse_cents": float(np.sqrt(np.mean(e * e))), "gross_pitch_error": float((np.abs(e) > GROSS_CENTS).mean()),
            "f0_corr": float(np.corrcoef(la, lb)[0, 1]) if len(la) > 1 else math.nan}


def contour_pair(n, seed, shift=2.0):
    """two contours of n frames with mixed voicing and NaNs: b follows a `shift` semitones up with a 1 % jitter and a few octave
    jumps, and disagrees with a about voicing here and there"""
    rng = np.random.default_rng([seed, n, 24])
    t = np.arange(n)
    a = 160.0 * 2.0 ** (0.4 * np.sin(2 * np.pi * t / 97.0) + 0.02 * rng.standard_normal(n))
    b = a * 2.0 ** (shift / 12.0) * (1.0 + 0.01 * rng.standard_normal(n))
    b[rng.random(n) < 0.03] *= 2.0
    a[rng.random(n) < 0.25] = 0.0
    b[rng.random(n) < 0.25] = 0.0
    a[rng.random(n) < 0.05] = np.nan
    b[rng.random(n) < 0.05] = np.nan
    return a, b


# ---- test signals --------------------------------------------------------------------------------------------------------------------
def voice(n, sr, seed):
    """a seeded harmonic voice (a glide with vibrato, 1 / h harmonics under two formant bumps) on a 1e-3 noise floor, float64"""
    rng = np.random.default_rng([seed, n, sr])
    t = np.arange(n) / sr
    f0 = rng.uniform(100.0, 180.0) * (1.0 + 0.2 * t) + 4.0 * np.sin(2 * np.pi * 5.0 * t)
    ph = 2 * np.pi * np.cumsum(f0) / sr + rng.uniform(0, 2 * np.pi)
    f1, f2 = rng.uniform(400, 900), rng.uniform(1200, 2600)
    x = np.zeros(n)
    for h in range(1, 20):
        fh = h * f0.mean()
        if fh > 0.45 * sr:
            break
        amp = (1.0 / h) * (1.0 + 3.0 * math.exp(-((fh - f1) / 150.0) ** 2) + 2.0 * math.exp(-((fh - f2) / 250.0) ** 2))
        x += amp * np.sin(h * ph + rng.uniform(0, 2 * np.pi))
    return 0.2 * x / 3.0 + 1e-3 * rng.standard_normal(n)


VOWELS = ((730, 1090), (270, 2290), (300, 870), (530, 1840), (570, 840), (440, 1020), (660, 1720), (390, 1990))


def vowel_sequence(durations, sr=16000, seed=0, f0=120.0):
    """eight vowel-like segments (harmonics of f0 under two formants each) of the given durations in seconds, 10 ms cross-fades
    between their envelopes, on a 1e-3 noise floor"""
    rng = np.random.default_rng([seed, 8])
    n = int(round(sum(durations) * sr))
    t = np.arange(n) / sr
    edges = np.cumsum([0.0] + list(durations))
    weights = np.zeros((len(durations), n))
    for s in range(len(durations)):
        rise = np.clip((t - edges[s]) / 0.01 + 0.5, 0, 1)
        fall = np.clip((edges[s + 1] - t) / 0.01 + 0.5, 0, 1)
        weights[s] = (rise if s else 1.0) * (fall if s < len(durations) - 1 else 1.0)
    x = np.zeros(n)
    for h in range(1, 60):
        fh = h * f0
        if fh > 0.45 * sr:
            break
        amp = np.zeros(n)
        for s, (f1, f2) in enumerate(VOWELS[: len(durations)]):
            amp += weights[s] * (1.0 / h) * (0.05 + 4.0 * math.exp(-((fh - f1) / 120.0) ** 2) + 3.0 * math.exp(-((fh - f2) / 200.0) ** 2))
        x += amp * np.sin(2 * np.pi * fh * t)
    return 0.1 * x + 1e-3 * rng.standard_normal(n)


DUR_A = (0.10, 0.17, 0.12, 0.16, 0.11, 0.15, 0.13, 0.16)       # 1.10 s
DUR_B = (0.16, 0.11, 0.17, 0.12, 0.18, 0.12, 0.17, 0.12)       # 1.15 s
