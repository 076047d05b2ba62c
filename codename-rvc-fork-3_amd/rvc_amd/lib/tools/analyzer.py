"""The audio analyzer (rvc/lib/tools/analyzer.py: ``calculate_features`` / ``analyze_audio``) and a dataset table on top of it.

The reference takes ``librosa.stft`` and the ``spectral_centroid`` / ``spectral_bandwidth`` / ``spectral_rolloff`` features with
their defaults and draws a three-row figure.  What is built is those calls as the native kernel K23 (csrc/specfeat.hip; the
algorithm is spelled out in include/rvc_amd.h).  librosa is not a dependency and was not available to compare against: parity
with it is unpinned, and the float64 SciPy restatement lives in tests/spectral_features_ref.py.  There is no host
implementation of the features.  ``matplotlib`` is imported only where a figure is drawn.

``analyze_dataset`` is this build's own: a per-file roll-off and bandwidth table over a training set, which shows at a glance
whether the recordings hold what their sample rate claims (a "48 kHz" file upsampled from 16 kHz has a 99 % roll-off near 8 kHz).

    python -m rvc_amd.lib.tools.analyzer FILE [PNG]
    python -m rvc_amd.lib.tools.analyzer --dataset DIR
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

from rvc_amd import _native
from rvc_amd.lib import audio as _audio

HOP = 512                 # librosa's default hop of an n_fft = 2048 STFT
LOAD_SR = 22050           # librosa.load's default rate
MAX_POINTS = 11025        # librosa.display.waveshow: longer signals are drawn as a peak envelope


def _signal(y, device, what: str):
    """-> (the 1-D float32 signal on the device, whether the caller gave NumPy)"""
    if torch.is_tensor(y):
        if y.dim() != 1 or not y.is_floating_point():
            raise ValueError(f"{what}: y must be a 1-D floating-point signal, got {y.dtype} of shape {tuple(y.shape)}")
        return y.to(torch.float32), False
    y = np.asarray(y)
    if y.ndim != 1 or y.dtype not in (np.float32, np.float64):
        raise ValueError(f"{what}: y must be a 1-D float32 or float64 signal, got {y.dtype} of shape {y.shape}")
    dev = torch.device(device) if device is not None else _native._cuda_device(None)
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev), True


def _whole_hz(sr, what: str) -> int:
    if int(sr) != sr or sr < 1:
        raise ValueError(f"{what}: sr must be a positive whole number of Hz, got {sr!r}")
    return int(sr)


def calculate_features(y, sr, *, device=None):
    """-> (stft, duration, cent, bw, rolloff): the magnitude spectrogram [1025, F] float32 (a transposed view of the frame-major
    plane), len(y) / sr, and the centroid, bandwidth and 85 % roll-off in Hz, float64 [F], F = 1 + len(y) // 512.

    A NumPy array gives NumPy arrays (computed on ``device``, default the current one); a device tensor gives tensors on its
    device, enqueued on the current stream without a host synchronisation."""
    sr = _whole_hz(sr, "calculate_features")
    x, as_numpy = _signal(y, device, "calculate_features")
    cent, bw, rolloff, mag, _ = _native.spectral_features(x, sr, 0.85, want_mag=True)
    duration = x.numel() / sr
    if as_numpy:
        return mag.cpu().numpy().T, duration, cent.cpu().numpy(), bw.cpu().numpy(), rolloff.cpu().numpy()
    return mag.t(), duration, cent, bw, rolloff


def spectral_features(y, sr, *, roll_percent=0.85, db=False, device=None) -> dict:
    """The three curves without storing a magnitude plane: {"cent", "bw", "rolloff"} float64 [F] in Hz, plus "db" [1025, F]
    float32 (amplitude_to_db(|S|, ref=max), a transposed view) when ``db`` is set.  NumPy in, NumPy out; tensor in, tensor out."""
    sr = _whole_hz(sr, "spectral_features")
    x, as_numpy = _signal(y, device, "spectral_features")
    cent, bw, rolloff, _, plane = _native.spectral_features(x, sr, float(roll_percent), want_db=bool(db))
    out = {"cent": cent, "bw": bw, "rolloff": rolloff}
    if db:
        out["db"] = plane.t()
    return {k: v.cpu().numpy() for k, v in out.items()} if as_numpy else out


def format_audio_info(sr: int, duration: float, samples: int, native_sr: int, mono: bool = True) -> str:
    """The reference's info string, character for character -- its quirk included: the "Bits per Sample" line prints the file's
    native sample rate (librosa.get_samplerate), not a bit depth."""
    length = str(round(duration, 2)) + " seconds" if duration < 60 else str(round(duration / 60, 2)) + " minutes"
    return (f"Sample Rate: {sr}\nDuration: {length}\nNumber of Samples: {samples}\nBits per Sample: {native_sr}\n"
            f"Channels: {'Mono (1)' if mono else 'Stereo (2)'}")


def peak_envelope(x: torch.Tensor):
    """waveshow's envelope of a signal of more than MAX_POINTS samples: -> (hop, max |x| per column of ``hop`` samples), on x's
    device; the last column may be short."""
    n = x.numel()
    hop = max(1, n // MAX_POINTS)
    cols = -(-n // hop)
    a = torch.nn.functional.pad(x.abs(), (0, cols * hop - n))
    return hop, a.view(cols, hop).amax(dim=1)


def _load(audio_file: str, target_sr, device):
    """-> (the mono signal as float64 NumPy at target_sr, or at its own rate when target_sr is None; the rate; the file's rate)"""
    a, native_sr = _audio.read_wav(audio_file)
    if a.ndim > 1:
        a = a.mean(axis=1)
    if target_sr is not None and native_sr != target_sr:
        a = _audio.resample(a, native_sr, target_sr, device=device)
    return np.asarray(a, dtype=np.float64), (native_sr if target_sr is None else target_sr), native_sr


def _draw(path, title, x, sr, duration, db, cent, bw, rolloff):
    import matplotlib
    if "matplotlib.pyplot" not in sys.modules:
        matplotlib.use("Agg")            # a file is written, no window is opened
    import matplotlib.pyplot as plt

    fig = plt.figure(figsize=(12, 10))
    try:
        plt.suptitle(title, fontsize=16, fontweight="bold")
        plt.subplot(3, 1, 1)
        plt.imshow(db.cpu().numpy(), origin="lower", extent=[0, duration, 0, sr / 1000], aspect="auto", cmap="inferno")
        plt.colorbar(format="%+2.0f dB")
        plt.xlabel("Time (s)")
        plt.ylabel("Frequency (kHz)")
        plt.title("Spectrogram")

        plt.subplot(3, 1, 2)
        if x.numel() > MAX_POINTS:
            hop, env = peak_envelope(x)
            env = env.cpu().numpy()
            plt.fill_between(np.arange(len(env)) * hop / sr, -env, env)
        else:
            plt.plot(np.arange(x.numel()) / sr, x.cpu().numpy())
        plt.xlabel("Time (s)")
        plt.ylabel("Amplitude")
        plt.title("Waveform")

        plt.subplot(3, 1, 3)
        times = np.arange(cent.numel()) * HOP / sr
        plt.plot(times, cent.cpu().numpy(), label="Spectral Centroid (kHz)", color="b")
        plt.plot(times, bw.cpu().numpy(), label="Spectral Bandwidth (kHz)", color="g")
        plt.plot(times, rolloff.cpu().numpy(), label="Spectral Rolloff (kHz)", color="r")
        plt.xlabel("Time (s)")
        plt.title("Spectral Features")
        plt.legend()

        plt.tight_layout()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        plt.savefig(path, bbox_inches="tight", dpi=300)
    finally:
        plt.close(fig)


def analyze_audio(audio_file, save_plot_path="logs/audio_analysis.png", *, device=None):
    """-> (audio_info, save_plot_path).  The file is read as WAV, averaged to mono and taken to 22050 Hz (librosa.load's
    defaults; the resampler is this build's Kaiser sinc, see rvc_amd.lib.audio).  With ``save_plot_path`` falsy no figure is
    drawn, matplotlib is not imported and no spectrogram is computed."""
    dev = torch.device(device) if device is not None else _native._cuda_device(None)
    y, sr, native_sr = _load(audio_file, LOAD_SR, dev)
    duration = len(y) / sr
    if save_plot_path:
        x = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
        cent, bw, rolloff, _, db = _native.spectral_features(x, sr, 0.85, want_db=True)
        _draw(save_plot_path, "Audio Analysis" + " - " + audio_file.split("/")[-1], x, sr, duration, db.t(), cent, bw, rolloff)
    return format_audio_info(sr, duration, len(y), native_sr), save_plot_path


def _points(v: torch.Tensor) -> dict:
    if v.numel() == 0:
        return {"median": 0.0, "p05": 0.0, "p95": 0.0}
    q = torch.quantile(v, torch.tensor([0.5, 0.05, 0.95], dtype=v.dtype, device=v.device)).tolist()
    return {"median": q[0], "p05": q[1], "p95": q[2]}


def analyze_dataset(path, *, roll_percent=0.99, device=None) -> dict:
    """Every .wav under ``path`` (under ``path/sliced_audios`` when that exists), each at its own rate without resampling: per
    file the rate, length, and the median, 5 % and 95 % points of centroid, bandwidth, the 85 % roll-off and the ``roll_percent``
    roll-off ("rolloff99") over the frames that are not digital silence, plus ``effective_bandwidth_hz`` (the median
    "rolloff99") and its ratio to sr / 2.  Two kernel calls per file, no spectrogram.  The table is written to
    ``path/audio_analysis.json`` and returned."""
    dev = torch.device(device) if device is not None else _native._cuda_device(None)
    root = os.path.join(path, "sliced_audios")
    if not os.path.isdir(root):
        root = path
    names = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.lower().endswith(".wav"))
    files = {}
    for name in names:
        y, sr, _ = _load(os.path.join(root, name), None, dev)
        x = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
        cent, bw, r85, _, _ = _native.spectral_features(x, sr, 0.85)
        r99 = _native.spectral_features(x, sr, float(roll_percent))[2]
        live = cent > 0        # s0 > 0: a windowed frame with any energy has some above bin 0, a silent one gives exactly 0
        rec = {"sr": sr, "samples": len(y), "duration": len(y) / sr, "centroid": _points(cent[live]), "bandwidth": _points(bw[live]),
               "rolloff85": _points(r85[live]), "rolloff99": _points(r99[live])}
        rec["effective_bandwidth_hz"] = rec["rolloff99"]["median"]
        rec["effective_bandwidth_ratio"] = rec["effective_bandwidth_hz"] / (sr / 2)
        files[name] = rec
    table = {"root": root, "roll_percent": float(roll_percent), "files": files}
    with open(os.path.join(path, "audio_analysis.json"), "w") as f:
        json.dump(table, f, indent=2)
    return table


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rvc_amd.lib.tools.analyzer", description="Analyse one WAV file, or a dataset.")
    ap.add_argument("file", nargs="?", help="a WAV file: prints its info string")
    ap.add_argument("png", nargs="?", help="where to save the figure (default: none)")
    ap.add_argument("--dataset", metavar="DIR", help="a dataset directory: prints one line per file and the path of the JSON")
    a = ap.parse_args(argv)
    if (a.file is None) == (a.dataset is None):
        ap.error("give a FILE or --dataset DIR")
    if a.dataset:
        table = analyze_dataset(a.dataset)
        for name, r in table["files"].items():
            print(f"{name}: sr {r['sr']}, {r['duration']:.2f} s, effective bandwidth {r['effective_bandwidth_hz']:.0f} Hz "
                  f"({r['effective_bandwidth_ratio']:.2f} of Nyquist), centroid {r['centroid']['median']:.0f} Hz")
        print(os.path.join(a.dataset, "audio_analysis.json"))
    else:
        print(analyze_audio(a.file, a.png)[0])
    return 0


if __name__ == "__main__":
    sys.exit(main())
