"""``shift_formants`` -- the formant shifter behind ``convert_audio(..., formant_shifting=True)`` (rvc/lib/utils.py:70-82 runs
``stftpitchshift.StftPitchShift(1024, 32, sr).shiftpitch(audio, factors=1, quefrency=formant_qfrency * 1e-3,
distortion=formant_timbre)`` over the 16 kHz input).

What is built is that call -- the pitch factor fixed at 1, so only the cepstral envelope is moved -- as the native kernel chain
K19 (csrc/formant.hip; the algorithm is spelled out in include/rvc_amd.h).  The stftpitchshift wheel is not a dependency and was
not available to compare against: parity with it is unpinned, the specification in the header is this build's own, and its
float64 SciPy restatement lives in tests/formant_shift_ref.py.

There is no host implementation: the signal is filtered on the device, on the current stream.
"""
from __future__ import annotations

import numpy as np
import torch

from rvc_amd import _native


def shift_formants(audio, sr=16000, quefrency_ms: float = 0.8, timbre: float = 0.8, *, device=None, group_frames: int = 0):
    """Move the spectral envelope of the 1-D signal ``audio`` (at least 1024 samples) at ``sr`` Hz: the envelope is what the
    cepstrum holds below ``quefrency_ms`` milliseconds, and it is stretched along the frequency axis by ``timbre`` (> 1 moves the
    formants up, < 1 down and silences the bins above ``timbre`` x Nyquist; 1 leaves the signal as the STFT round trip).

    A NumPy array (float32 or float64) gives a NumPy array of the same dtype (filtered in float32 on ``device``, default the
    current one); a device tensor gives a tensor of its floating dtype on its device, enqueued on the current stream without a
    host synchronisation."""
    if int(sr) != sr:
        raise ValueError(f"shift_formants: sr must be a whole number of Hz, got {sr!r}")
    sr, quefrency_s = int(sr), float(quefrency_ms) * 1e-3
    if torch.is_tensor(audio):
        if audio.dim() != 1:
            raise ValueError(f"shift_formants: audio must be 1-D, got shape {tuple(audio.shape)}")
        if not audio.is_floating_point():
            raise ValueError(f"shift_formants: audio must be a floating-point tensor, got {audio.dtype}")
        return _native.formant_shift(audio.to(torch.float32), sr, quefrency_s, timbre, group_frames).to(audio.dtype)
    audio = np.asarray(audio)
    if audio.ndim != 1:
        raise ValueError(f"shift_formants: audio must be 1-D, got shape {audio.shape}")
    if audio.dtype not in (np.float32, np.float64):
        raise ValueError(f"shift_formants: audio must be float32 or float64, got {audio.dtype}")
    dev = _native._cuda_device(device)
    x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        return _native.formant_shift(x, sr, quefrency_s, timbre, group_frames).cpu().numpy().astype(audio.dtype, copy=False)
