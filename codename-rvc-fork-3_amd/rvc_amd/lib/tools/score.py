"""The conversion scorer: how well a converted utterance keeps the input's pitch contour, and how close it comes to a parallel
recording of the target speaker.  The reference has no such tool; this one is this build's own, on the native kernels K24
(csrc/convscore.hip; the algorithms are spelled out in include/rvc_amd.h, the figures in rvc_amd.lib.metrics).

* F0 tracking errors between SOURCE and CONVERTED (shift-compensated RMSE in cents, the shift itself, log-F0 correlation, voicing
  decision error, gross pitch error): the pipeline is meant to carry the contour across unchanged but for the transposition.
* Mel-cepstral distortion after dynamic time warping between CONVERTED and TARGET, when a target recording is given.

Every signal is brought to 16 kHz with the library's own loader and resampler, so WAVs of any rate work and one rate serves the
pitch estimator and the cepstra.  Not pinned: parity with any third-party MCD package; silence is NOT trimmed (do that first if
the recordings carry long pauses); an utterance may hold at most 16384 frames of 5 ms (81.9 s) on either side of the DTW.

    python -m rvc_amd.lib.tools.score SOURCE.wav CONVERTED.wav [--target T.wav] [--band N] [--json OUT]
    python -m rvc_amd.lib.tools.score --pairs DIR_A DIR_B [--targets DIR_T] [--band N]
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

from rvc_amd import _native
from rvc_amd.lib import audio as _audio
from rvc_amd.lib import metrics as _metrics

SR = 16000
F0_KEYS = ("f0_rmse_cents", "shift_semitones", "f0_corr", "vuv_error", "gross_pitch_error", "voiced_frames")


def _load(signal, device, what: str) -> np.ndarray:
    """A path, or an (array, sr) pair -> the mono float64 signal at 16 kHz."""
    if isinstance(signal, (str, os.PathLike)):
        return _audio.load_audio(os.fspath(signal), SR, device=device)
    try:
        a, sr = signal
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a path or an (array, sr) pair") from None
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.ndim == 2:          # [n, channels], the layout read_wav returns; no guessing from the sizes
        a = a.mean(axis=1)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1 or a.size < 1:
        raise ValueError(f"{what}: the array must hold one signal, got shape {a.shape}")
    if int(sr) != sr or sr < 1:
        raise ValueError(f"{what}: sr must be a positive whole number of Hz, got {sr!r}")
    if int(sr) != SR:
        a = _audio.resample(a, int(sr), SR, device=device)
    return np.asarray(a, dtype=np.float64).flatten()


def make_predictor(f0_method: str, device):
    """The pitch estimator of ``f0_method`` with the weights the pipeline would load (rvc/models/predictors/)."""
    if f0_method == "rmvpe":
        from rvc_amd.lib.predictors.RMVPE import RMVPE0Predictor
        path = os.path.join("rvc", "models", "predictors", "rmvpe.pt")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path} not found: pass predictor=RMVPE0Predictor(...) with weights of your own")
        return RMVPE0Predictor(path, device=device)
    if f0_method == "fcpe":
        from rvc_amd.lib.predictors.FCPE import FCPE
        return FCPE(160, 50, 1100, SR, device, model_path=os.path.join("rvc", "models", "predictors", "fcpe.pt"))
    raise NotImplementedError(f"f0_method={f0_method!r}: only 'rmvpe' and 'fcpe' are built")


def _f0(predictor, x: np.ndarray) -> np.ndarray:
    if hasattr(predictor, "infer_from_audio"):
        f0 = predictor.infer_from_audio(x.astype(np.float32), thred=0.03)
    elif hasattr(predictor, "compute_f0"):
        f0 = predictor.compute_f0(x.astype(np.float32))
    else:
        f0 = predictor(x)
    f0 = f0.detach().cpu().numpy() if torch.is_tensor(f0) else np.asarray(f0)
    return np.asarray(f0, dtype=np.float64).reshape(-1)


def score_conversion(source, converted, target=None, *, f0_method="rmvpe", predictor=None, band=None, device=None) -> dict:
    """-> the F0 tracking errors of ``converted`` against ``source`` (``rvc_amd.lib.metrics.f0_tracking_errors`` over the common
    length of the two contours, 10 ms frames), plus ``frames``; and with a ``target``, ``mcd_dtw_db`` (converted against target,
    ``band`` as in ``metrics.dtw``), the path's length ``dtw_path_length`` and ``mcd_aligned_db`` (no warping) for comparison.
    Each signal is a WAV path or an ``(array, sr)`` pair; the array is one signal [n], or [n, channels] (samples first, as
    ``rvc_amd.lib.audio.read_wav`` returns), which is averaged to mono -- any other shape is refused.  ``predictor``: an estimator with ``infer_from_audio`` (RMVPE) or
    ``compute_f0`` (FCPE), or a callable audio -> contour; by default the one ``f0_method`` names is loaded."""
    dev = torch.device(device) if device is not None else _native._cuda_device(None)
    src, conv = _load(source, dev, "source"), _load(converted, dev, "converted")
    if predictor is None:
        predictor = make_predictor(f0_method, dev)
    fa, fb = _f0(predictor, src), _f0(predictor, conv)
    frames = min(len(fa), len(fb))
    if frames < 1:
        raise ValueError("score_conversion: the pitch estimator returned an empty contour")
    out = dict(_metrics.f0_tracking_errors(fa[:frames], fb[:frames], device=dev))
    out["frames"] = frames
    if target is not None:
        tgt = _load(target, dev, "target")
        cx, cy = _metrics.mel_cepstra(conv, SR, device=dev), _metrics.mel_cepstra(tgt, SR, device=dev)
        if max(cx.shape[0], cy.shape[0]) > _metrics.DTW_MAX_FRAMES:
            raise ValueError(f"score_conversion: {max(cx.shape[0], cy.shape[0])} frames exceed the DTW's {_metrics.DTW_MAX_FRAMES}; "
                             "score the utterance in pieces")
        res, _ = _native.dtw(cx, cy, _metrics._band(band))
        total, length = res.cpu().tolist()
        common = min(cx.shape[0], cy.shape[0])
        out["mcd_dtw_db"] = _metrics.mcd_from_sums(total, length)
        out["dtw_path_length"] = int(length)
        out["mcd_aligned_db"] = _metrics.mcd_from_sums(_native.frame_dist_sum(cx, cy, common).item(), common)
    return out


def pair_files(dir_a: str, dir_b: str, dir_t: str | None = None):
    """The .wav files of dir_a and dir_b (and dir_t) matched by file stem -> sorted [(stem, path_a, path_b, path_t or None)];
    a stem missing from dir_b is left out, one missing from dir_t is scored without a target."""
    def stems(d):
        return {os.path.splitext(f)[0]: os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".wav")}
    a, b = stems(dir_a), stems(dir_b)
    t = stems(dir_t) if dir_t else {}
    return [(s, a[s], b[s], t.get(s)) for s in sorted(a) if s in b]


def _median(values):
    v = [x for x in values if x is not None and not (isinstance(x, float) and math.isnan(x))]
    return float(np.median(v)) if v else None


def score_pairs(dir_a: str, dir_b: str, dir_t: str | None = None, **options) -> dict:
    """``score_conversion`` over every pair of ``pair_files``; the per-file figures and their medians go to
    ``dir_b/conversion_scores.json`` and are returned.  One predictor serves every file."""
    pairs = pair_files(dir_a, dir_b, dir_t)
    if not pairs:
        raise ValueError(f"no .wav stem is common to {dir_a} and {dir_b}")
    if options.get("predictor") is None:
        dev = torch.device(options["device"]) if options.get("device") is not None else _native._cuda_device(None)
        options["predictor"] = make_predictor(options.get("f0_method", "rmvpe"), dev)
    files = {stem: score_conversion(pa, pb, pt, **options) for stem, pa, pb, pt in pairs}
    keys = sorted({k for r in files.values() for k in r})
    table = {"source": dir_a, "converted": dir_b, "target": dir_t, "files": files,
             "median": {k: _median([r.get(k) for r in files.values()]) for k in keys}}
    with open(os.path.join(dir_b, "conversion_scores.json"), "w") as f:
        json.dump(table, f, indent=2)
    return table


def _line(name: str, r: dict) -> str:
    s = (f"{name}: f0 rmse {r['f0_rmse_cents']:.1f} cents, shift {r['shift_semitones']:+.2f} st, corr {r['f0_corr']:.3f}, "
         f"v/uv {100 * r['vuv_error']:.1f} %, gross {100 * r['gross_pitch_error']:.1f} %")
    if "mcd_dtw_db" in r:
        s += f", mcd {r['mcd_dtw_db']:.2f} dB (aligned {r['mcd_aligned_db']:.2f})"
    return s


def main(argv=None, **options) -> int:
    """The command line; ``options`` (a ``predictor``, a ``device``) are handed on to ``score_conversion``."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rvc_amd.lib.tools.score", description="Score a voice conversion.")
    ap.add_argument("source", nargs="?", help="the input WAV")
    ap.add_argument("converted", nargs="?", help="the converted WAV")
    ap.add_argument("--target", help="a parallel recording of the target speaker: adds the DTW mel-cepstral distortion")
    ap.add_argument("--pairs", nargs=2, metavar=("DIR_A", "DIR_B"), help="score every stem common to two directories")
    ap.add_argument("--targets", metavar="DIR_T", help="with --pairs: the directory of target recordings")
    ap.add_argument("--band", type=int, help="DTW corridor half-width in frames (default: none)")
    ap.add_argument("--f0-method", default="rmvpe", choices=("rmvpe", "fcpe"))
    ap.add_argument("--json", metavar="OUT", help="write the figures of one pair here")
    a = ap.parse_args(argv)
    if (a.pairs is None) == (a.source is None) or (a.pairs is None and a.converted is None):
        ap.error("give SOURCE CONVERTED, or --pairs DIR_A DIR_B")
    options.setdefault("f0_method", a.f0_method)
    if a.pairs:
        table = score_pairs(a.pairs[0], a.pairs[1], a.targets, band=a.band, **options)
        for name, r in table["files"].items():
            print(_line(name, r))
        print(os.path.join(a.pairs[1], "conversion_scores.json"))
    else:
        r = score_conversion(a.source, a.converted, a.target, band=a.band, **options)
        print(_line(os.path.basename(a.converted), r))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(r, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
