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
