"""The per-item figures of the reference's ``validation_loop`` (rvc/train/train.py:1478-1579) on the native loss kernels K20
(csrc/valmetrics.hip; the algorithms are spelled out in include/rvc_amd.h):

* ``multi_resolution_stft_loss`` -- ``auraloss.freq.MultiResolutionSTFTLoss()`` with its defaults: per resolution a spectral
  convergence term and a log-magnitude L1 term, averaged over the resolutions.  The auraloss wheel is not a dependency and was
  not available to compare against: parity with it is unpinned, the specification in the header is this build's own, and its
  float64 ``torch.stft`` restatement lives in tests/validation_ref.py;
* ``si_sdr`` -- the reference's own function (train.py:244-257);
* ``mel_l1`` -- ``F.l1_loss`` over the common columns of two mels (train.py:1525-1532).

The device writes float64 sums, merged in a fixed order (two calls give identical bits); the square roots, quotients and
logarithms are finished here in float64.  There is no host implementation: the signals are summed on the device, and each
function returns a Python float, which synchronises with the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from rvc_amd import _native

FFT_SIZES = (1024, 2048, 512)
HOP_SIZES = (120, 240, 50)
WIN_LENGTHS = (600, 1200, 240)

# the keyword arguments of auraloss.freq.MultiResolutionSTFTLoss at the only values that are built
_AURALOSS_DEFAULTS = dict(window="hann_window", w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, w_phs=0.0, sample_rate=None, scale=None,
                          n_bins=None, perceptual_weighting=False, scale_invariance=False, reduction="mean", mag_distance="L1",
                          output="loss")


def _signal(a, device, name):
    """A 1-D signal (a [1, n] or [1, 1, n] batch of one is squeezed) as a float32 tensor in HBM."""
    if torch.is_tensor(a):
        if not a.is_floating_point():
            raise ValueError(f"{name} must be floating point, got {a.dtype}")
        t = a.detach()
        if not t.is_cuda:
            t = t.to(_native._cuda_device(device))
    else:
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            raise ValueError(f"{name} must be float32 or float64, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_native._cuda_device(device))
    while t.dim() > 1 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 1:
        raise ValueError(f"{name} must be one signal (batches are scored item by item), got shape {tuple(a.shape)}")
    return t.to(torch.float32).contiguous()


def _pair(x, y, device):
    if device is None:   # an array follows the tensor it is compared with
        device = next((t.device for t in (x, y) if torch.is_tensor(t) and t.is_cuda), None)
    return _signal(x, device, "the first signal"), _signal(y, device, "the second signal")


def stft_loss_terms(x, y, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, eps: float = 1e-8, *, device=None):
    """Per resolution ``(sc, lm)``: the spectral convergence ||ymag - xmag||_F / ||ymag||_F and the mean of
    |log xmag - log ymag| of the prediction ``x`` against the target ``y``."""
    x, y = _pair(x, y, device)
    sums = _native.mrstft_sums(x, y, fft_sizes, hop_sizes, win_lengths, eps).cpu().tolist()
    return [(math.sqrt(d2 / y2), la / count) for d2, y2, la, count in sums]


def multi_resolution_stft_loss(x, y, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, eps: float = 1e-8, *,
                               device=None, **auraloss_options) -> float:
    """``auraloss.freq.MultiResolutionSTFTLoss(fft_sizes, hop_sizes, win_lengths, eps=eps)(x, y)`` for one prediction ``x`` and one
    target ``y`` (arrays or tensors of equal length; arrays and host tensors are uploaded to ``device``, default the current one):
    the mean over the resolutions of sc + lm.  Up to 4 resolutions with n_fft in {512, 1024, 2048}, win <= n_fft, hop <= 512.  Any
    other keyword of auraloss is accepted at its default only and raises NotImplementedError by name otherwise."""
    for k, v in auraloss_options.items():
        if k not in _AURALOSS_DEFAULTS:
            raise TypeError(f"multi_resolution_stft_loss: unknown option {k!r}")
        if v != _AURALOSS_DEFAULTS[k]:
            raise NotImplementedError(f"multi_resolution_stft_loss: {k}={v!r} is not built (only {k}={_AURALOSS_DEFAULTS[k]!r} is)")
    terms = stft_loss_terms(x, y, fft_sizes, hop_sizes, win_lengths, eps, device=device)
    return sum(sc + lm for sc, lm in terms) / len(terms)


def si_sdr_from_sums(sums, eps: float = 1e-8) -> float:
    """train.py:244-257 in float64 from the five sums of include/rvc_amd.h: sum p, sum t, and of the centred signals sum pc tc,
    sum tc^2, sum pc^2."""
    _, _, pt, tt, pp = (float(v) for v in sums)
    s = pt / (tt + eps)
    projection = s * s * tt
    noise = pp - 2.0 * s * pt + s * s * tt
    if noise <= pp * 2.0 ** -48:      # a difference of sums below their own resolution: the reference's fp32 noise is 0 here
        noise = 0.0
    if noise == 0.0:
        ratio = math.inf if projection > 0.0 else math.nan    # 0 / 0 in the reference's expression too
    else:
        ratio = projection / noise
    value = ratio + eps
    return 10.0 * math.log10(value) if value > 0.0 else (-math.inf if value == 0.0 else math.nan)


def si_sdr(preds, target, eps: float = 1e-8, *, device=None) -> float:
    """The reference's scale-invariant SDR in dB of one prediction against one target (at least 2 samples each).  The noise
    energy is a difference of float64 sums (``si_sdr_from_sums``): a value above about 144 dB is returned as +inf, and the last
    digits thin out as a value approaches that ceiling: the noise energy carries an error of about 1e-15 of the prediction's energy."""
    preds, target = _pair(preds, target, device)
    return si_sdr_from_sums(_native.si_sdr_sums(preds, target).cpu().tolist(), eps)


def _matrix(a, device, name):
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))
    t = a.detach()
    if not t.is_cuda:
        t = t.to(_native._cuda_device(device))
    while t.dim() > 2 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise ValueError(f"{name} must be one [channels, frames] matrix, got shape {tuple(a.shape)}")
    return t.to(torch.float32)


def mel_l1(y_hat_mel, mel, *, device=None) -> float:
    """``F.l1_loss(y_hat_mel[..., :min_t], mel[..., :min_t])`` with min_t the shorter of the two widths (train.py:1525-1532); the
    columns past min_t are never read, the matrices are not copied."""
    if device is None:
        device = next((t.device for t in (y_hat_mel, mel) if torch.is_tensor(t) and t.is_cuda), None)
    a, b = _matrix(y_hat_mel, device, "y_hat_mel"), _matrix(mel, device, "mel")
    min_t = min(a.shape[1], b.shape[1])
    return float(_native.mean_abs_diff_sum(a, b, min_t).item()) / (a.shape[0] * min_t)


# ---- the conversion scorer (K24, csrc/convscore.hip) -----------------------------------------------------------------------------
# How good a CONVERSION is, where the figures above score a vocoder on sample-aligned pairs: the mel-cepstral distortion against
# a parallel target after dynamic time warping, and the F0 tracking errors between the input and the output.  The algorithms are
# spelled out in include/rvc_amd.h and restated in float64 in tests/conversion_score_ref.py; no third-party MCD package was
# available, so parity with any is unpinned.  Silence is NOT trimmed: leading and trailing pauses take part in the alignment, and
# trimming them is the caller's job.  A sequence may hold at most 16384 frames (81.9 s at the 5 ms hop).
MCD_CONST = 10.0 / math.log(10.0) * math.sqrt(2.0)      # (10 / ln 10) sqrt 2: Euclidean cepstral distance -> dB
GROSS_CENTS = 1200.0 * math.log2(1.2)                   # a gross pitch error: more than 20 % off the shift-compensated contour
DTW_MAX_FRAMES = 16384

_mel_dev = {}


def _mel_matrix(sr: int, n_mels: int, device) -> torch.Tensor:
    key = (int(sr), int(n_mels), str(device))
    if key not in _mel_dev:
        from rvc_amd.train.mel_processing import librosa_mel_fn
        _mel_dev[key] = torch.from_numpy(np.ascontiguousarray(librosa_mel_fn(int(sr), 1024, int(n_mels), 0, sr / 2),
                                                              dtype=np.float32)).to(device)
    return _mel_dev[key]


def mel_cepstra(x, sr, n_mels: int = 80, n_coef: int = 24, *, device=None) -> torch.Tensor:
    """The mel-cepstral coefficients c[1 .. n_coef] of one signal at ``sr`` (a multiple of 200 Hz in 8000 .. 48000), one row per
    5 ms: a float32 device tensor [1 + n // (sr // 200), n_coef].  1024-point periodic-Hann frames centred on the hop grid, the
    Slaney mel filterbank of ``librosa_mel_fn(sr, 1024, n_mels, 0, sr / 2)`` on the power spectrum, half the natural log, DCT-II."""
    if int(sr) != sr:
        raise ValueError(f"mel_cepstra: sr must be a whole number of Hz, got {sr!r}")
    x = _signal(x, device, "the signal")
    return _native.melcep(x, int(sr), _mel_matrix(int(sr), n_mels, x.device), int(n_coef))


def _features(a, device, name):
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))
    t = a.detach()
    if not t.is_cuda:
        t = t.to(_native._cuda_device(device))
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2:
        raise ValueError(f"{name} must be one [frames, dim] sequence, got shape {tuple(a.shape)}")
    return t.to(torch.float32).contiguous()


def _feature_pair(a, b, device):
    if device is None:
        device = next((t.device for t in (a, b) if torch.is_tensor(t) and t.is_cuda), None)
    return _features(a, device, "the first sequence"), _features(b, device, "the second sequence")


def _band(band) -> int:
    if band is None:
        return -1
    if int(band) != band or band < 1:
        raise ValueError(f"band must be None or a whole number of frames >= 1, got {band!r}")
    return int(band)


def dtw(a, b, band=None, *, device=None):
    """Dynamic time warping of two feature sequences [Ta, dim] and [Tb, dim] (arrays or tensors; at most 16384 frames and 64
    dimensions) under the Euclidean frame distance with the steps (1, 1), (1, 0), (0, 1) -> ``(cost, path)``: the float cost of the
    best path and the path as an int32 device tensor [L, 2] from (0, 0) to (Ta - 1, Tb - 1).  ``band``: None, or the half-width in
    frames of a corridor around the straight line between the corners."""
    a, b = _feature_pair(a, b, device)
    out, path = _native.dtw(a, b, _band(band))
    cost, length = out.cpu().tolist()
    return cost, path[: int(length)]


def mcd_from_sums(total: float, count: float) -> float:
    """(10 / ln 10) sqrt 2 times the mean frame distance ``total / count``, in dB."""
    return MCD_CONST * float(total) / float(count)


def mel_cepstral_distortion(x, y, sr, align="dtw", band=None, *, n_mels: int = 80, n_coef: int = 24, device=None) -> float:
    """The mel-cepstral distortion in dB between two signals at one rate: (10 / ln 10) sqrt 2 times the mean Euclidean distance of
    their cepstra c[1 .. n_coef], over the DTW path (``align="dtw"``, the cost divided by the path's length) or over the common
    frames taken one to one (``align=None``)."""
    if align not in ("dtw", None):
        raise ValueError(f"mel_cepstral_distortion: align must be 'dtw' or None, got {align!r}")
    x, y = _pair(x, y, device)
    cx, cy = mel_cepstra(x, sr, n_mels, n_coef), mel_cepstra(y, sr, n_mels, n_coef)
    if align is None:
        frames = min(cx.shape[0], cy.shape[0])
        return mcd_from_sums(_native.frame_dist_sum(cx, cy, frames).item(), frames)
    if max(cx.shape[0], cy.shape[0]) > DTW_MAX_FRAMES:
        raise ValueError(f"mel_cepstral_distortion: {max(cx.shape[0], cy.shape[0])} frames exceed the DTW's {DTW_MAX_FRAMES} "
                         f"({DTW_MAX_FRAMES // 200} s); score the utterance in pieces")
    out, _ = _native.dtw(cx, cy, _band(band))
    total, length = out.cpu().tolist()
    return mcd_from_sums(total, length)


def f0_errors_from_sums(sums) -> dict:
    """The F0 tracking figures in float64 from the twelve sums of include/rvc_amd.h (rvc_f0_track_sums_f64)."""
    n, sr_, sla, slb, saa, sbb, sab, see, gross, a_only, b_only, neither = (float(v) for v in sums)
    frames = n + a_only + b_only + neither
    out = {"voiced_frames": int(n), "vuv_error": (a_only + b_only) / frames if frames else math.nan}
    if n == 0:
        out.update(f0_rmse_cents=math.nan, shift_semitones=math.nan, f0_corr=math.nan, gross_pitch_error=math.nan)
        return out
    out["shift_semitones"] = sr_ / n / 100.0
    out["f0_rmse_cents"] = math.sqrt(see / n)
    out["gross_pitch_error"] = gross / n
    va, vb, cov = saa - sla * sla / n, sbb - slb * slb / n, sab - sla * slb / n
    # a variance below the resolution of its own sums is a flat contour: no correlation is defined
    flat = va <= saa * 2.0 ** -44 or vb <= sbb * 2.0 ** -44
    out["f0_corr"] = math.nan if flat else max(-1.0, min(1.0, cov / math.sqrt(va * vb)))
    return out


def _contour(f, device, name):
    if torch.is_tensor(f):
        t = f.detach()
        if not t.is_cuda:
            t = t.to(_native._cuda_device(device))
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(f), dtype=np.float64)).to(_native._cuda_device(device))
    if t.dim() != 1:
        raise ValueError(f"{name} must be one 1-D contour, got shape {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def f0_tracking_errors(f0_a, f0_b, *, device=None) -> dict:
    """How well the contour ``f0_b`` (the converted output's) follows ``f0_a`` (the input's); both in Hz, equally long, 0 or NaN
    where unvoiced.  Over the frames voiced in both: ``shift_semitones`` the mean of 12 log2(b / a), ``f0_rmse_cents`` the RMS
    of what is left after that shift is taken out, ``f0_corr`` the Pearson correlation of log2 a and log2 b (NaN for a flat
    contour), ``gross_pitch_error`` the share of frames more than 20 % off the shifted contour, ``voiced_frames`` their number;
    ``vuv_error`` the share of all frames voiced in exactly one of the two."""
    if device is None:
        device = next((t.device for t in (f0_a, f0_b) if torch.is_tensor(t) and t.is_cuda), None)
    a, b = _contour(f0_a, device, "f0_a"), _contour(f0_b, device, "f0_b")
    if a.shape != b.shape or a.numel() < 1:
        raise ValueError(f"f0_tracking_errors wants two contours of one length >= 1, got {a.numel()} and {b.numel()} frames")
    return f0_errors_from_sums(_native.f0_track_sums(a, b).cpu().tolist())
