"""Times K22 (csrc/effects.hip): every effect and the board of the reference's defaults on a 30 s / 48 kHz utterance, with HIP
events after warm-up, and the float32 NumPy restatement (tests/effects_ref.py) of the same effects on the CPU.

    python tools/time_effects.py --device            # the device times (needs the GPU)
    python tools/time_effects.py --restatement       # the restatement's times (CPU only)

Both print lines for profiles/effects_time.txt.  The slow paths are timed too: a chorus with feedback (one workgroup walks the
signal) and compressors whose release is too long for any chunk to close (one lane walks the signal)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import effects_ref as R  # noqa: E402

SR, SECONDS = 48000, 30
# every switch of post_process_audio on, every parameter at the reference's default (pitch_shift is not built); the default
# gain is 0 dB, the default compressor has ratio 1 and the default delay and chorus have no feedback
BOARD = dict(reverb=True, limiter=True, gain=True, distortion=True, chorus=True, bitcrush=True, clipping=True, compressor=True, delay=True)
CASES = [   # (label, restatement function, its arguments after (x, sr), the device call)
    ("gain -3 dB", "gain", (-3.0,), lambda N, x: N.fx_pointwise(x, 1, gain_db=-3.0)),
    ("gain -> distortion 25 dB (one launch)", None, None, lambda N, x: N.fx_pointwise(x, 3, gain_db=-3.0, drive_db=25.0)),
    ("distortion 25 dB", "distortion", (25.0,), lambda N, x: N.fx_pointwise(x, 2, drive_db=25.0)),
    ("bitcrush 8 -> clipping 0 dB (one launch)", None, None, lambda N, x: N.fx_pointwise(x, 12, bit_depth=8.0, clip_threshold_db=0.0)),
    ("delay 0.5 s fb 0.3", "delay", (0.5, 0.3, 0.5), lambda N, x: N.fx_delay(x, SR, 0.5, 0.3, 0.5)),
    ("delay 1 sample fb 0.3 (one chain: slow path)", "delay", (1.5 / SR, 0.3, 0.5), lambda N, x: N.fx_delay(x, SR, 1.5 / SR, 0.3, 0.5)),
    ("chorus default (fb 0)", "chorus", (1.0, 0.25, 7.0, 0.0, 0.5), lambda N, x: N.fx_chorus(x, SR, 1.0, 0.25, 7.0, 0.0, 0.5)),
    ("chorus fb 0.3 (one workgroup: slow path)", "chorus", (1.0, 0.25, 7.0, 0.3, 0.5), lambda N, x: N.fx_chorus(x, SR, 1.0, 0.25, 7.0, 0.3, 0.5)),
    ("reverb default", "reverb", (0.5, 0.5, 0.33, 0.4, 1.0, 0.0), lambda N, x: N.fx_reverb(x, SR, 0.5, 0.5, 0.33, 0.4, 1.0, 0.0)),
    ("compressor -20 dB 4:1 1 / 100 ms", "compressor", (-20.0, 4.0, 1.0, 100.0), lambda N, x: N.fx_compressor(x, SR, -20.0, 4.0, 1.0, 100.0)),
    ("compressor release 10 s (long chunks)", "compressor", (-20.0, 4.0, 1.0, 1e4), lambda N, x: N.fx_compressor(x, SR, -20.0, 4.0, 1.0, 1e4)),
    ("compressor attack = release = 100 s (no chunk closes: one lane)", "compressor", (-40.0, 4.0, 1e5, 1e5),
     lambda N, x: N.fx_compressor(x, SR, -40.0, 4.0, 1e5, 1e5)),
    ("limiter default", "limiter", (-6.0, 0.05), lambda N, x: N.fx_limiter(x, SR, -6.0, 0.05)),
]


def time_device(args):
    import torch
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native as N
    from rvc_amd.infer.infer import VoiceConverter
    x = torch.from_numpy(R.signal(SR * SECONDS, SR)).cuda()

    def measure(run, slow):
        calls, windows = (1, 5) if slow else (10, 20)
        for _ in range(1 if slow else 5):
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
        return f"median {np.median(t):.4f} ms, min {t.min():.4f}, max {t.max():.4f} ({windows} windows of {calls} calls)"

    print(f"python tools/time_effects.py --device (one MI355X; K22, csrc/effects.hip; n={SR * SECONDS} sr={SR}, HIP events)")
    for label, _, _, call in CASES:
        print(f"{label}: {measure(lambda: call(N, x), 'slow' in label or 'one lane' in label)}", flush=True)
    print(f"board, reference defaults, all nine switches on: {measure(lambda: VoiceConverter.post_process_audio(x, SR, **BOARD), False)}", flush=True)


def time_restatement(args):
    x = R.signal(SR * SECONDS, SR)
    print(f"python tools/time_effects.py --restatement (tests/effects_ref.py, dtype=float32, one CPU thread; n={SR * SECONDS} sr={SR})")
    for label, fn, fn_args, _ in CASES:
        if fn is None:
            continue
        lead = () if fn in ("gain", "distortion") else (SR,)
        t0 = time.perf_counter()
        getattr(R, fn)(x, *lead, *fn_args, dtype=np.float32)
        print(f"{label}: {time.perf_counter() - t0:.3f} s", flush=True)
    t0 = time.perf_counter()
    R.post_process(x, SR, np.float32, **BOARD)
    print(f"board, reference defaults, all nine switches on: {time.perf_counter() - t0:.3f} s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--restatement", action="store_true")
    a = ap.parse_args()
    if not (a.device or a.restatement):
        ap.error("choose --device and / or --restatement")
    if a.device:
        time_device(a)
    if a.restatement:
        time_restatement(a)
