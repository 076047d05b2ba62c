"""Dataset preprocessing: a folder of WAVs -> ``<exp_dir>/sliced_audios/*.wav`` at the dataset rate and
``<exp_dir>/sliced_audios_16k/*.wav``, the inputs of rvc_amd.train.extract.extract.

This is the reference's rvc/train/preprocess/preprocess.py step by step -- optional 48 Hz high-pass and normalisation, then no
cut (``Skip``), fixed windows (``Simple``) or silence-based slicing into 3 s windows (``Automatic``) -- with the file uploaded
once and the filter, the RMS and every slice's float32 + 16 kHz copy computed on the device (K17: csrc/preprocess.hip).
Decoding covers WAV only and the 16 kHz copies use this build's own polyphase filter (rvc_amd.lib.audio; soxr parity unpinned).
Noise reduction (noisereduce, third-party) is not part of this build.

    python -m rvc_amd.train.preprocess.preprocess EXP_DIR INPUT_ROOT SR NUM_PROC CUT EFFECTS NOISE STRENGTH CHUNK OVERLAP
"""
from __future__ import annotations

import concurrent.futures
import json
import math
import os
import sys
import time

import numpy as np
import torch
from scipy import signal
from scipy.io import wavfile

from rvc_amd.lib.audio import load_audio, resample_filter
from rvc_amd.train.preprocess.slicer import Slicer

OVERLAP = 0.3
PERCENTAGE = 3.0
MAX_AMPLITUDE = 0.9
ALPHA = 0.75
HIGH_PASS_CUTOFF = 48
SAMPLE_RATE_16K = 16000

_filters_dev = {}


def _filter_dev(up: int, down: int, device) -> torch.Tensor:
    key = (up, down, str(device))
    if key not in _filters_dev:
        h = np.ones(1) if up == down else resample_filter(up, down)      # a 16 kHz dataset: the 16 kHz copy is the slice itself
        _filters_dev[key] = torch.from_numpy(h).to(device)
    return _filters_dev[key]


class PreProcess:
    def __init__(self, sr: int, exp_dir: str, device="cuda:0"):
        self.slicer = Slicer(sr=sr, threshold=-42, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)
        self.sr = sr
        self.b_high, self.a_high = signal.butter(N=5, Wn=HIGH_PASS_CUTOFF, btype="high", fs=self.sr)
        self.exp_dir = exp_dir
        self.device = device
        self.gt_wavs_dir = os.path.join(exp_dir, "sliced_audios")
        self.wavs16k_dir = os.path.join(exp_dir, "sliced_audios_16k")
        os.makedirs(self.gt_wavs_dir, exist_ok=True)
        os.makedirs(self.wavs16k_dir, exist_ok=True)

    def _normalize_audio(self, audio: torch.Tensor):
        """preprocess.py:58-62 on a float64 device tensor, one elementwise step per reference operation."""
        if audio.numel() == 0:
            return audio
        tmp_max = audio.abs().max()
        if float(tmp_max) > 2.5:
            return None
        # divided by the 0-dim DEVICE tensor: torch turns a division by a host scalar into a multiplication by its reciprocal
        return (audio / tmp_max * (MAX_AMPLITUDE * ALPHA)) + (1 - ALPHA) * audio

    def plan_slices(self, n_samples: int, cut_preprocess: str, chunk_len: float, overlap_len: float, slicer_bounds=None):
        """-> [(idx1, start, end)]: the name index and the half-open sample range of every file process_audio writes
        (preprocess.py:91-126 simple_cut, 152-194)."""
        n_samples = int(n_samples)
        if cut_preprocess == "Skip":
            return [(0, 0, n_samples)]
        if cut_preprocess == "Simple":
            chunk_length = int(self.sr * chunk_len)
            overlap_length = int(self.sr * overlap_len)
            if chunk_length - overlap_length <= 0:
                raise ValueError("chunk_len must be longer than overlap_len")     # the reference never leaves its loop here
            out, i = [], 0
            while i < n_samples:
                if min(n_samples, i + chunk_length) - i == chunk_length:          # only full-length chunks are written
                    out.append((i // (chunk_length - overlap_length), i, i + chunk_length))
                i += chunk_length - overlap_length
            return out
        if cut_preprocess == "Automatic":
            out, idx1 = [], 0
            for seg_start, seg_end in slicer_bounds:
                seg_len = seg_end - seg_start
                i = 0
                while True:
                    start = int(self.sr * (PERCENTAGE - OVERLAP) * i)
                    i += 1
                    if max(0, seg_len - start) > (PERCENTAGE + OVERLAP) * self.sr:
                        out.append((idx1, seg_start + start, seg_start + start + int(PERCENTAGE * self.sr)))
                        idx1 += 1
                    else:
                        out.append((idx1, seg_start + min(start, seg_len), seg_end))
                        idx1 += 1
                        break
            return out
        return []          # the reference does nothing for any other word

    def process_audio(self, path: str, idx0: int, sid: int, cut_preprocess: str, process_effects: bool, noise_reduction: bool,
                      reduction_strength: float, chunk_len: float, overlap_len: float, debug_taps: dict | None = None):
        """preprocess.py:128-198 -> the file's duration in seconds; never raises."""
        audio_length = 0
        try:
            audio = load_audio(path, self.sr, device=self.device)
            audio_length = len(audio) / self.sr                       # librosa.get_duration
            x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float64)).to(self.device)
            self._process_uploaded(x, idx0, sid, cut_preprocess, process_effects, noise_reduction, chunk_len, overlap_len, debug_taps)
        except Exception as error:
            print(f"Error processing audio: {error}")
        return audio_length

    def _process_uploaded(self, x, idx0, sid, cut_preprocess, process_effects, noise_reduction, chunk_len, overlap_len, debug_taps):
        from rvc_amd import _native
        if process_effects:
            x = _native.lfilter_order5(x, self.b_high, self.a_high)
            x = self._normalize_audio(x)
        if noise_reduction:
            raise NotImplementedError("noise reduction (noisereduce) is not part of this build")
        if debug_taps is not None:
            debug_taps["audio"] = x
        if x is None:                    # peak above 2.5: the reference goes on with None
            if cut_preprocess == "Skip":
                print(f"{sid}-{idx0}-0-filtered")
                return
            if cut_preprocess == "Simple":
                raise TypeError("object of type 'NoneType' has no len()")
            if cut_preprocess == "Automatic":
                raise AttributeError("'NoneType' object has no attribute 'shape'")
            return
        n = x.numel()
        bounds = None
        if cut_preprocess == "Automatic":
            rms = self.slicer.rms(x) if self.slicer.needs_rms(n) else np.zeros(0)
            if debug_taps is not None:
                debug_taps["rms"] = rms
            bounds = self.slicer.slice_bounds(rms, n)
        plan = self.plan_slices(n, cut_preprocess, chunk_len, overlap_len, bounds)
        if not plan:
            return
        g = math.gcd(int(self.sr), SAMPLE_RATE_16K)
        up, down = SAMPLE_RATE_16K // g, int(self.sr) // g
        full, lo, off_full, off_lo = _native.slice_export(x, [(s, e) for _, s, e in plan], up, down, _filter_dev(up, down, x.device))
        full, lo = full.cpu().numpy(), lo.cpu().numpy()
        for k, (idx1, _, _) in enumerate(plan):
            name = f"{sid}_{idx0}_{idx1}.wav"
            wavfile.write(os.path.join(self.gt_wavs_dir, name), self.sr, full[off_full[k]: off_full[k + 1]])
            wavfile.write(os.path.join(self.wavs16k_dir, name), SAMPLE_RATE_16K, lo[off_lo[k]: off_lo[k + 1]])


def format_duration(seconds):
    hours = int(seconds // 3600)
    minutes = int((seconds % 3600) // 60)
    seconds = int(seconds % 60)
    return f"{hours:02}:{minutes:02}:{seconds:02}"


def save_dataset_duration(file_path, dataset_duration):
    try:
        with open(file_path, "r") as f:
            data = json.load(f)
    except FileNotFoundError:
        data = {}
    data.update({"total_dataset_duration": format_duration(dataset_duration), "total_seconds": dataset_duration})
    with open(file_path, "w") as f:
        json.dump(data, f, indent=4)


def find_files(input_root: str):
    """preprocess.py:267-280 -> [(path, idx0, sid)]: the speaker id is the integer name of the sub-folder, 0 at the root."""
    files, idx = [], 0
    for root, _, filenames in os.walk(input_root):
        try:
            sid = 0 if root == input_root else int(os.path.basename(root))
            for f in filenames:
                if f.lower().endswith((".wav", ".mp3", ".flac", ".ogg")):
                    files.append((os.path.join(root, f), idx, sid))
                    idx += 1
        except ValueError:
            print(f'Speaker ID folder is expected to be integer, got "{os.path.basename(root)}" instead.')
    return files


def _device_share(sr, exp_dir, device, share, args):
    """One device's files, walked in order on a stream of this worker's own (workers may share a device)."""
    pp = PreProcess(sr, exp_dir, device=device)
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device)):
        return [pp.process_audio(path, idx0, sid, *args) for path, idx0, sid in share]


def preprocess_training_set(input_root: str, sr: int, num_processes: int, exp_dir: str, cut_preprocess: str, process_effects: bool,
                            noise_reduction: bool, reduction_strength: float, chunk_len: float, overlap_len: float, devices=None):
    """preprocess.py:251-315.  ``num_processes`` is accepted for the reference's surface and ignored: the work is on the device,
    one host thread per entry of ``devices`` (default: cuda:0), device i taking files[i::len(devices)]."""
    if noise_reduction:
        raise NotImplementedError("noise reduction (noisereduce, third-party) is not part of this build; pass noise_reduction=False")
    start_time = time.time()
    devices = list(devices) if devices else ["cuda:0"]
    print(f"Starting preprocess on {', '.join(devices)}...")
    files = find_files(input_root)
    os.makedirs(exp_dir, exist_ok=True)
    args = (cut_preprocess, process_effects, noise_reduction, reduction_strength, chunk_len, overlap_len)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(devices)) as executor:   # one host thread per GPU
        tasks = [executor.submit(_device_share, sr, exp_dir, dev, files[i::len(devices)], args) for i, dev in enumerate(devices)]
        lengths = [t.result() for t in tasks]
    audio_length = sum(sum(share) for share in lengths)
    save_dataset_duration(os.path.join(exp_dir, "model_info.json"), dataset_duration=audio_length)
    elapsed_time = time.time() - start_time
    print(f"Preprocess completed in {elapsed_time:.2f} seconds on {format_duration(audio_length)} seconds of audio.")
    return audio_length


def strtobool(value) -> int:
    """distutils.util.strtobool (gone from the standard library): 1 / 0, ValueError for anything else."""
    v = str(value).lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return 1
    if v in ("n", "no", "f", "false", "off", "0"):
        return 0
    raise ValueError(f"invalid truth value {v!r}")


def parse_args(argv):
    """The reference's ten positional arguments -> the keyword arguments of preprocess_training_set."""
    if len(argv) != 10:
        raise SystemExit("usage: python -m rvc_amd.train.preprocess.preprocess EXP_DIR INPUT_ROOT SR NUM_PROC "
                         "{Skip,Simple,Automatic} EFFECTS NOISE STRENGTH CHUNK OVERLAP")
    num_processes = os.cpu_count() if str(argv[3]).lower() == "none" else int(argv[3])
    return dict(exp_dir=str(argv[0]), input_root=str(argv[1]), sr=int(argv[2]), num_processes=num_processes,
                cut_preprocess=str(argv[4]), process_effects=strtobool(argv[5]), noise_reduction=strtobool(argv[6]),
                reduction_strength=float(argv[7]), chunk_len=float(argv[8]), overlap_len=float(argv[9]))


def main(argv=None) -> int:
    preprocess_training_set(**parse_args(list(sys.argv[1:] if argv is None else argv)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
