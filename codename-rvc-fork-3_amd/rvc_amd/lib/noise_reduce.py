"""``reduce_noise`` -- the spectral gate behind ``convert_audio(..., clean_audio=True)`` (rvc/infer/infer.py:77-93 calls
``noisereduce.reduce_noise(y=audio, sr=sr, prop_decrease=strength)``).

What is built is noisereduce 3.x's default path -- ``stationary=False``: a mask from the ratio of each STFT bin to its own
time-smoothed level -- as the native kernel chain K18 (csrc/spectralgate.hip; the algorithm is spelled out in include/rvc_amd.h).
The noisereduce wheel is not a dependency and was not available to compare against: parity with it is unpinned, the
specification in the header is this build's own, and its float64 SciPy restatement lives in tests/spectral_gate_ref.py.  One
deliberate difference: a bin that is silent in every frame gives zeros here, not NaN.

There is no host implementation: the signal is filtered on the device, on the current stream.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from rvc_amd import _native

# every other keyword of noisereduce.reduce_noise with the value this build implements; anything else is refused by name
_BUILT = {
    "stationary": (False,), "y_noise": (None,), "time_constant_s": (2.0,), "freq_mask_smooth_hz": (500,),
    "time_mask_smooth_ms": (50,), "thresh_n_mult_nonstationary": (2,), "sigmoid_slope_nonstationary": (10,),
    "n_std_thresh_stationary": (1.5,), "tmp_folder": (None,), "n_fft": (1024,), "win_length": (None, 1024),
    "hop_length": (None, 256), "clip_noise_stationary": (True,), "use_tqdm": (False, True), "n_jobs": (1,),
    "use_torch": (False,),
}


def gate_parameters(sr: int):
    """-> (nf, nt, b, filt): the half-widths (bins, frames) of the mask smoothing filter at ``sr``, the coefficient of the
    one-pole level smoother, and the (2 nf + 1) x (2 nt + 1) filter itself (sums to 1), as the library's host code derives them."""
    nf, nt, b, ft, tt = _native.spectral_gate_params(_sample_rate(sr))
    return nf, nt, b, np.outer(np.concatenate([ft[:0:-1], ft]), np.concatenate([tt[:0:-1], tt]))


def _sample_rate(sr) -> int:
    if int(sr) != sr:
        raise ValueError(f"reduce_noise: sr must be a whole number of Hz, got {sr!r}")
    return int(sr)


def reduce_noise(y, sr, prop_decrease: float = 1.0, *, chunk_size: int = 600000, padding: int = 30000, device=None, **kw):
    """Non-stationary spectral gating of the 1-D signal ``y`` at ``sr`` Hz; ``prop_decrease`` in [0, 1] is the share of the
    estimated noise that is taken out.

    A NumPy array (float32 or float64) gives a NumPy float32 array (filtered on ``device``, default the current one); a device
    tensor gives a float32 tensor on its device, enqueued on the current stream without a host synchronisation."""
    for name, value in kw.items():
        if name not in _BUILT:
            raise TypeError(f"reduce_noise() got an unexpected keyword argument '{name}'")
        scalar = isinstance(value, numbers.Number)           # an array (y_noise) never equals a built value
        if not any(value is v or (scalar and v is not None and value == v) for v in _BUILT[name]):
            raise NotImplementedError(f"reduce_noise: {name}={value!r} is not part of this build (built: {name}={_BUILT[name][0]!r})")
    sr = _sample_rate(sr)
    if torch.is_tensor(y):
        if y.dim() != 1:
            raise ValueError(f"reduce_noise: y must be 1-D, got shape {tuple(y.shape)}")
        return _native.spectral_gate(y.to(torch.float32), sr, prop_decrease, chunk_size, padding)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"reduce_noise: y must be 1-D, got shape {y.shape}")
    if y.dtype not in (np.float32, np.float64):
        raise ValueError(f"reduce_noise: y must be float32 or float64, got {y.dtype}")
    dev = _native._cuda_device(device)
    y_dev = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        return _native.spectral_gate(y_dev, sr, prop_decrease, chunk_size, padding).cpu().numpy()
