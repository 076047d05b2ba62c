"""shift_formants (K19, csrc/formant.hip) on 480 000 samples at 16 kHz -- a 30 s utterance, 14 969 frames -- device tensor in and out:
HIP events around 10 back-to-back calls, median of 30 such windows after 5 warm-up calls, at Q = 12 (the default 0.8 ms), Q = 256
and Q = 511, timbre 0.8; then the float64 restatement of tests/formant_shift_ref.py on the same box (wall clock) and the device's
deviation from it at this size.  DESIGN.md K19.
    python tools/time_formant_shift.py
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/time_formant_shift.py --calls-only"""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")]
import torch
import formant_shift_ref as R
from rvc_amd.lib.formant_shift import shift_formants

n, sr, d = 480000, 16000, 0.8
x64 = R.test_signal(n, sr)
x = torch.from_numpy(x64.astype(np.float32)).cuda()
for Q in (12, 256, 511):
    ms = (Q + 0.5) / 16.0
    for _ in range(5):
        y = shift_formants(x, sr, ms, d)
    torch.cuda.synchronize()
    if "--calls-only" in sys.argv:
        for _ in range(20):
            y = shift_formants(x, sr, ms, d)
        torch.cuda.synchronize()
        continue
    times = []
    for _ in range(30):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(10):
            y = shift_formants(x, sr, ms, d)
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / 10)
    times = np.array(times)
    print(f"shift_formants n={n} sr={sr} Q={Q} d={d}: median {np.median(times):.4f} ms, min {times.min():.4f}, max {times.max():.4f}, "
          f"p10 {np.percentile(times, 10):.4f}, p90 {np.percentile(times, 90):.4f} (30 windows of 10 calls)", flush=True)
    if Q == 511:
        continue
    t0 = time.perf_counter()
    r64 = R.shift_formants(x64, sr, ms * 1e-3, d)
    t1 = time.perf_counter()
    r32 = R.shift_formants(x64.astype(np.float32), sr, ms * 1e-3, d)
    t2 = time.perf_counter()
    print(f"restatement Q={Q}: float64 {t1 - t0:.3f} s, float32 input {t2 - t1:.3f} s (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')})")
    e_ref, err = np.abs(r32 - r64).max(), np.abs(y.cpu().numpy() - r64).max()
    print(f"parity at this size: e_ref={e_ref:.3g} max|dev - r64|={err:.3g} ({err / e_ref:.1f} e_ref)", flush=True)
