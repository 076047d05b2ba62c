"""Shared by test_preprocess_cpu.py and test_preprocess_gpu.py: the reference's get_rms restated in NumPy and the recordings the
manifest (tests/golden/preprocess_manifest.npz, make_golden_preprocess.py) was made from."""
import numpy as np


def get_rms_numpy(y, frame_length, hop_length):
    """slicer.py:199-235 restated: zero-pad frame_length // 2 on both sides, frame t = padded[t * hop : t * hop + frame_length]."""
    pad = frame_length // 2
    y = np.pad(np.asarray(y, np.float64), (pad, pad))
    n_frames = (y.size - frame_length) // hop_length + 1
    if n_frames <= 0:
        return np.zeros(0)
    idx = np.arange(n_frames)[:, None] * hop_length + np.arange(frame_length)[None, :]
    return np.sqrt(np.mean(y[idx] ** 2, axis=1))


def signals(sr, seed):
    """-> (the recording, the all-silent one, the one shorter than min_length) as make_golden_preprocess.py cuts them"""
    from rvc_amd.lib import synthetic as S
    full = S.synth_preprocess_audio(sr, seed)
    hop = round(sr * 0.015)
    return full, full[: 45 * hop] * 0.5, full[50 * hop: 50 * hop + 80]
