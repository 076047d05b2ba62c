#!/usr/bin/env python3
"""HIP-event time of one FCPE forward (K4b mel + K11 GEMMs + K15, csrc/fcpe.hip) at 3201 frames -- a 30 s utterance plus the
pipeline's 2 x 1 s of padding -- beside RMVPE's front plus back half on the same audio and the same GPU, and of each K15 kernel at
the shapes that forward gives it.

    python tools/bench_fcpe.py [--seconds 30] [--steps 20] [--warmup 5] [--out profiles/fcpe_forward.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "codename-rvc-fork-3_amd"))

from rvc_amd import _native as N  # noqa: E402
from rvc_amd.lib import synthetic as S  # noqa: E402
from rvc_amd.lib.predictors.FCPE import FCPE  # noqa: E402
from rvc_amd.lib.predictors.RMVPE import RMVPE0Predictor  # noqa: E402


def timed(fn, steps, warmup):
    """median / min of `steps` single calls, each between two HIP events on the current stream"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    n = int(16000 * a.seconds) + 32000
    audio = torch.from_numpy(S.synth_gated_glide(n, 0)).float().to(dev)
    fcpe = FCPE(device=dev, checkpoint=S.make_fcpe_checkpoint(0))
    rmvpe = RMVPE0Predictor(device=dev, state_dict=S.make_rmvpe_state_dict(0, peaked=True))
    frames = n // 160 + 1
    lines = [f"{torch.cuda.get_device_name(0)}; {a.seconds:g} s + 2 s padding = {n} samples, {frames} FCPE frames; HIP events, "
             f"median (min) of {a.steps} calls after {a.warmup}"]

    def rmvpe_both():
        gi, nf = rmvpe.front_half_device(audio)
        return rmvpe.back_half_device(gi, nf)

    for name, fn in (("FCPE forward (mel + network + decode)", lambda: fcpe.infer_device(audio, 0.006)),
                     ("RMVPE front + back half", rmvpe_both)):
        med, lo = timed(fn, a.steps, a.warmup)
        lines.append(f"{name:44s} {med:8.3f} ms ({lo:.3f})")
    # the K15 kernels alone, at the forward's shapes
    h = fcpe.hidden
    x4 = torch.randn(frames, 4 * h, device=dev)
    x1 = torch.randn(frames, h, device=dev)
    xc = torch.randn(h, frames, device=dev)
    logits = torch.randn(frames, fcpe.proj_rows, device=dev) * 0.5
    w = fcpe.w
    for name, fn, nbytes in (
            (f"glu_dwconv_silu [{frames} x {4 * h}] k 31", lambda: N.glu_dwconv_silu(x4, w["l0.dw.w"], w["l0.dw.b"]), 6 * frames * h * 4),
            (f"layernorm_rows [{frames} x {h}]", lambda: N.layernorm_rows(x1, w["l0.ln.g"], w["l0.ln.b"]), 2 * frames * h * 4),
            (f"groupnorm_lrelu [{h} x {frames}] / 4", lambda: N.groupnorm_lrelu(xc, w["gn.g"], w["gn.b"], 4), 3 * frames * h * 4),
            (f"fcpe_decode [{frames} x {fcpe.proj_rows}]", lambda: N.fcpe_decode(logits, w["cent_table"], 360, 0.006, 32.7), frames * 361 * 4)):
        med, lo = timed(fn, a.steps, a.warmup)
        lines.append(f"{name:44s} {med * 1e3:8.1f} us ({lo * 1e3:.1f}); {nbytes / 1e6:.1f} MB algorithmic = {nbytes / lo / 1e6:.0f} GB/s at the minimum "
                     "(includes the wrapper's output allocation)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
