"""Silence-based slicing (rvc/train/preprocess/slicer.py).  The per-frame RMS is computed on the device (rvc_frame_rms_f64, K17)
and only the RMS list comes back; the scan over it is the reference's own sequence of comparisons on the host."""
from __future__ import annotations

import numpy as np


class Slicer:
    """slicer.py:4-55: same constructor, checks, derived fields and rounding."""

    def __init__(self, sr: int, threshold: float = -40.0, min_length: int = 5000, min_interval: int = 300, hop_size: int = 20,
                 max_sil_kept: int = 5000):
        if not min_length >= min_interval >= hop_size:
            raise ValueError("min_length >= min_interval >= hop_size is required")
        if not max_sil_kept >= hop_size:
            raise ValueError("max_sil_kept >= hop_size is required")
        min_interval = sr * min_interval / 1000
        self.threshold = 10 ** (threshold / 20.0)
        self.hop_size = round(sr * hop_size / 1000)
        self.win_size = min(round(min_interval), 4 * self.hop_size)
        self.min_length = round(sr * min_length / 1000 / self.hop_size)
        self.min_interval = round(min_interval / self.hop_size)
        self.max_sil_kept = round(sr * max_sil_kept / 1000 / self.hop_size)

    def _bounds(self, n_samples: int, begin: int, end: int):
        """_apply_slice (slicer.py:57-72) as a half-open sample range; a range that starts past the end is empty, as the
        NumPy slice is."""
        start_idx = min(n_samples, begin * self.hop_size)
        end_idx = min(n_samples, end * self.hop_size)
        return (start_idx, max(start_idx, end_idx))

    def needs_rms(self, n_samples: int) -> bool:
        """slicer.py:83: a sample count against a frame count, as the reference compares them."""
        return n_samples > self.min_length

    def slice_bounds(self, rms_list, n_samples: int):
        """slicer.py:83-196 on the RMS list (float64, one value per frame) -> [(start, end), ...] sample ranges of the chunks."""
        n_samples = int(n_samples)
        if not self.needs_rms(n_samples):
            return [(0, n_samples)]
        rms_list = np.asarray(rms_list, dtype=np.float64)
        sil_tags = []
        silence_start, clip_start = None, 0
        for i, rms in enumerate(rms_list):
            if rms < self.threshold:
                if silence_start is None:
                    silence_start = i
                continue
            if silence_start is None:
                continue
            is_leading_silence = silence_start == 0 and i > self.max_sil_kept
            need_slice_middle = i - silence_start >= self.min_interval and i - clip_start >= self.min_length
            if not is_leading_silence and not need_slice_middle:
                silence_start = None
                continue
            if i - silence_start <= self.max_sil_kept:
                pos = rms_list[silence_start: i + 1].argmin() + silence_start
                if silence_start == 0:
                    sil_tags.append((0, pos))
                else:
                    sil_tags.append((pos, pos))
                clip_start = pos
            elif i - silence_start <= self.max_sil_kept * 2:
                pos = rms_list[i - self.max_sil_kept: silence_start + self.max_sil_kept + 1].argmin()
                pos += i - self.max_sil_kept
                pos_l = rms_list[silence_start: silence_start + self.max_sil_kept + 1].argmin() + silence_start
                pos_r = rms_list[i - self.max_sil_kept: i + 1].argmin() + i - self.max_sil_kept
                if silence_start == 0:
                    sil_tags.append((0, pos_r))
                    clip_start = pos_r
                else:
                    sil_tags.append((min(pos_l, pos), max(pos_r, pos)))
                    clip_start = max(pos_r, pos)
            else:
                pos_l = rms_list[silence_start: silence_start + self.max_sil_kept + 1].argmin() + silence_start
                pos_r = rms_list[i - self.max_sil_kept: i + 1].argmin() + i - self.max_sil_kept
                if silence_start == 0:
                    sil_tags.append((0, pos_r))
                else:
                    sil_tags.append((pos_l, pos_r))
                clip_start = pos_r
            silence_start = None
        total_frames = rms_list.shape[0]
        if silence_start is not None and total_frames - silence_start >= self.min_interval:
            silence_end = min(total_frames, silence_start + self.max_sil_kept)
            pos = rms_list[silence_start: silence_end + 1].argmin() + silence_start
            sil_tags.append((pos, total_frames + 1))
        if not sil_tags:
            return [(0, n_samples)]
        chunks = []
        if sil_tags[0][0] > 0:
            chunks.append(self._bounds(n_samples, 0, int(sil_tags[0][0])))
        for i in range(len(sil_tags) - 1):
            chunks.append(self._bounds(n_samples, int(sil_tags[i][1]), int(sil_tags[i + 1][0])))
        if sil_tags[-1][1] < total_frames:
            chunks.append(self._bounds(n_samples, int(sil_tags[-1][1]), total_frames))
        return chunks

    def rms(self, samples):
        """get_rms(samples, win_size, hop_size) on the device -> the float64 RMS list on the host."""
        from rvc_amd import _native
        return _native.frame_rms(samples, self.win_size, self.hop_size).cpu().numpy()

    def slice(self, waveform, device="cuda:0"):
        """slicer.py:74-196.  waveform: a float64 device tensor or a NumPy array, [n] or [channels, n]; -> views of it."""
        import torch
        multi = len(waveform.shape) > 1
        n_samples = int(waveform.shape[-1])
        if not self.needs_rms(n_samples):
            return [waveform]
        x = waveform if torch.is_tensor(waveform) else torch.from_numpy(np.ascontiguousarray(waveform, dtype=np.float64)).to(device)
        samples = x.mean(dim=0) if multi else x
        bounds = self.slice_bounds(self.rms(samples.to(torch.float64)), n_samples)
        return [waveform[:, s:e] if multi else waveform[s:e] for s, e in bounds]
