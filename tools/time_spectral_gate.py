"""reduce_noise (K18, csrc/spectralgate.hip) on 1 439 040 samples at 48 kHz -- the output length of BASELINE cfg 2 -- device tensor in
and out: HIP events around 10 back-to-back calls, median of 30 such windows after 5 warm-up calls; then the SciPy restatement of
tests/spectral_gate_ref.py on the same box (wall clock) and the device's deviation from it at this size.  DESIGN.md K18.
    python tools/time_spectral_gate.py
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/time_spectral_gate.py --calls-only"""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")]
import torch
import spectral_gate_ref as R
from rvc_amd.lib.noise_reduce import reduce_noise

n, sr, prop = 1439040, 48000, 0.5
x64 = R.test_signal(n, sr)
x = torch.from_numpy(x64.astype(np.float32)).cuda()
for _ in range(5):
    y = reduce_noise(x, sr, prop)
torch.cuda.synchronize()
if "--calls-only" in sys.argv:
    for _ in range(20):
        y = reduce_noise(x, sr, prop)
    torch.cuda.synchronize()
    sys.exit(0)
times = []
for _ in range(30):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(10):
        y = reduce_noise(x, sr, prop)
    stop.record()
    stop.synchronize()
    times.append(start.elapsed_time(stop) / 10)
times = np.array(times)
print(f"reduce_noise n={n} sr={sr}: median {np.median(times):.4f} ms, min {times.min():.4f}, max {times.max():.4f}, "
      f"p10 {np.percentile(times, 10):.4f}, p90 {np.percentile(times, 90):.4f} (30 windows of 10 calls)")
t0 = time.perf_counter()
r64 = R.reduce_noise(x64, sr, prop)
t1 = time.perf_counter()
r32 = R.reduce_noise(x64.astype(np.float32), sr, prop)
t2 = time.perf_counter()
print(f"SciPy restatement: float64 {t1 - t0:.3f} s, float32 input {t2 - t1:.3f} s (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')})")
e_ref, err = np.abs(r32 - r64).max(), np.abs(y.cpu().numpy() - r64).max()
print(f"parity at this size: e_ref={e_ref:.3g} max|dev - r64|={err:.3g} ({err / e_ref:.1f} e_ref)")
