"""A 10-minute 48 kHz file through PreProcess.process_audio("Automatic", process_effects=True) on the device against the same steps
on the host (scipy.signal.lfilter, NumPy get_rms, scipy.signal.resample_poly with the same FIR): wall clock, medians.  DESIGN.md K17.
    python tools/time_preprocess.py"""
import os
import sys
import tempfile
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")]
import torch
from scipy import signal
from scipy.io import wavfile
from rvc_amd.lib import synthetic as S, audio as A
from rvc_amd.train.preprocess import preprocess as T
from _preprocess_common import get_rms_numpy

sr = 48000
x = np.tile(S.synth_preprocess_audio(sr), 50).astype(np.float32)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "in.wav")
wavfile.write(path, sr, x)
print("samples", x.size, "seconds", x.size / sr, flush=True)
pp = T.PreProcess(sr, os.path.join(tmp, "exp"), device="cuda:0")
h = A.resample_filter(1, 3)

def gpu():
    pp.process_audio(path, 0, 0, "Automatic", True, False, 0.0, 3.0, 0.3)
    torch.cuda.synchronize()

def host():
    a = A.read_wav(path)[0]
    y = signal.lfilter(pp.b_high, pp.a_high, a)
    peak = np.abs(y).max()
    y = (y / peak * (T.MAX_AMPLITUDE * T.ALPHA)) + (1 - T.ALPHA) * y
    s = pp.slicer
    rms = get_rms_numpy(y, s.win_size, s.hop_size)
    plan = pp.plan_slices(y.size, "Automatic", 3.0, 0.3, s.slice_bounds(rms, y.size))
    for i, b, e in plan:
        seg = y[b:e]
        wavfile.write(os.path.join(pp.gt_wavs_dir, f"h_0_{i}.wav"), sr, seg.astype(np.float32))
        lo = signal.resample_poly(seg, 1, 3, window=h)
        wavfile.write(os.path.join(pp.wavs16k_dir, f"h_0_{i}.wav"), 16000, lo.astype(np.float32))
    return len(plan)

def med(fn, runs, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)), ts

g, gts = med(gpu, 7, 2)
print("device route: median %.4f s of %s" % (g, ["%.4f" % t for t in gts]), flush=True)
print("slices", host(), flush=True)
hh, hts = med(host, 5, 0)
print("host route: median %.4f s of %s" % (hh, ["%.4f" % t for t in hts]), flush=True)
# the device steps alone (no file I/O): upload, lfilter, normalise, rms, export, download
a = A.read_wav(path)[0]
def steps():
    from rvc_amd import _native
    xd = torch.from_numpy(a).to("cuda:0")
    yd = pp._normalize_audio(_native.lfilter_order5(xd, pp.b_high, pp.a_high))
    rms = pp.slicer.rms(yd)
    plan = pp.plan_slices(yd.numel(), "Automatic", 3.0, 0.3, pp.slicer.slice_bounds(rms, yd.numel()))
    f, l, _, _ = _native.slice_export(yd, [(b, e) for _, b, e in plan], 1, 3, T._filter_dev(1, 3, xd.device))
    f.cpu(); l.cpu()
s_, sts = med(steps, 7, 2)
print("device steps without file I/O: median %.4f s" % s_, flush=True)
def lf():
    from rvc_amd import _native
    _native.lfilter_order5(xd0, pp.b_high, pp.a_high); torch.cuda.synchronize()
xd0 = torch.from_numpy(a).to("cuda:0")
print("lfilter kernel alone: median %.5f s" % med(lf, 7, 2)[0], flush=True)
