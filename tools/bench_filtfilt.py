#!/usr/bin/env python3
"""Device filtfilt (K6) on a cfg-2 utterance (480 000 samples, the pipeline's 48 Hz high-pass): time per call -- warm-up, then the
median of 30 calls, each between two events on one stream -- and the error against scipy.signal.filtfilt."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd")]
import numpy as np, torch
from scipy import signal
from rvc_amd import _native
from rvc_amd.lib import synthetic as S
b, a = signal.butter(N=5, Wn=48, btype="high", fs=16000)
x = S.synth_audio(480_000, seed=0)
xd = torch.from_numpy(x).to("cuda:0")
for _ in range(10): y = _native.filtfilt_order5(xd, b, a)
torch.cuda.synchronize()
us = []
for _ in range(30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    y = _native.filtfilt_order5(xd, b, a)
    e1.record()
    e1.synchronize()
    us.append(e0.elapsed_time(e1) * 1e3)
us.sort()
ref = signal.filtfilt(b, a, x)
print(f"filtfilt 480000 samples: median {us[len(us) // 2]:.1f} us per call (min {us[0]:.1f}, max {us[-1]:.1f}, 30 calls), "
      f"max |err| vs scipy {np.abs(y.cpu().numpy() - ref).max():.2e}")
