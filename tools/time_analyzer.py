"""Times K23 (csrc/specfeat.hip): the analyzer's spectral features of a 30 s signal at 22050 Hz and at 48000 Hz, with and without
the dB plane, with HIP events after warm-up, and the float64 SciPy restatement (tests/spectral_features_ref.py) of the same inputs
on the CPU.

    python tools/time_analyzer.py                    # both, written to profiles/analyzer.txt (needs the GPU)
    python tools/time_analyzer.py --out FILE         # ... to another file
    python tools/time_analyzer.py --restatement      # the restatement alone, printed (CPU only)

"curves" is the call analyze_dataset makes (no plane reaches HBM), "curves + dB" the one analyze_audio makes for its figure, and
"curves + |S| + dB" stores both planes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import spectral_features_ref as R  # noqa: E402
from formant_shift_ref import test_signal  # noqa: E402

SECONDS = 30
RATES = (22050, 48000)
MODES = (("curves", False, False), ("curves + dB", False, True), ("curves + |S| + dB", True, True))


def time_device(lines):
    import torch
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native as N
    lines.append(f"python tools/time_analyzer.py (one MI355X; K23, csrc/specfeat.hip; {SECONDS} s signals, HIP events, 5 warm-up calls)")
    calls, windows = 10, 20
    for sr in RATES:
        x = torch.from_numpy(test_signal(sr * SECONDS, sr).astype(np.float32)).cuda()
        for label, want_mag, want_db in MODES:
            run = lambda: N.spectral_features(x, sr, 0.85, want_mag=want_mag, want_db=want_db)  # noqa: E731
            for _ in range(5):
                run()
            torch.cuda.synchronize()
            times = []
            for _ in range(windows):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(calls):
                    run()
                stop.record()
                stop.synchronize()
                times.append(start.elapsed_time(stop) / calls)
            t = np.array(times)
            lines.append(f"sr {sr}, n {x.numel()}, {1 + x.numel() // 512} frames, {label}: median {np.median(t):.4f} ms, min {t.min():.4f}, "
                         f"max {t.max():.4f} ({windows} windows of {calls} calls)")
            print(lines[-1], flush=True)


def time_restatement(lines):
    lines.append(f"python tools/time_analyzer.py --restatement (tests/spectral_features_ref.py, float64, scipy.fft; {SECONDS} s signals; "
                 "best of 3)")
    for sr in RATES:
        x = test_signal(sr * SECONDS, sr)
        for label, db in (("curves + |S|", False), ("curves + |S| + dB", True)):
            best = np.inf
            for _ in range(3):
                t0 = time.perf_counter()
                R.features(x, sr, 0.85, db=db)
                best = min(best, time.perf_counter() - t0)
            lines.append(f"sr {sr}, n {len(x)}, {label}: {best * 1e3:.1f} ms")
            print(lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--restatement", action="store_true", help="time the restatement alone and write no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analyzer.txt"))
    a = ap.parse_args()
    lines = []
    if not a.restatement:
        time_device(lines)
        lines.append("")
    time_restatement(lines)
    if not a.restatement:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)
