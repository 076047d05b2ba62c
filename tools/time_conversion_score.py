"""Times K24 (csrc/convscore.hip) with HIP events after warm-up -- the cepstra of a 30 s / 16 kHz signal, the DTW of two 6001-frame
sequences of 24 coefficients without a band and with band = 200, and one whole score_conversion of 30 s utterances (RMVPE with
synthetic weights, F0 errors, cepstra of two signals, DTW, the aligned sum) by the wall clock -- and the float64 restatement
(tests/conversion_score_ref.py) of the same inputs on the CPU.

    python tools/time_conversion_score.py                    # both, written to profiles/conversion_score.txt (needs the GPU)
    python tools/time_conversion_score.py --out FILE         # ... to another file
    python tools/time_conversion_score.py --restatement      # the restatement alone, printed (CPU only)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import conversion_score_ref as R  # noqa: E402

SR, SECONDS = 16000, 30


def signals():
    return R.voice(SR * SECONDS, SR, 1).astype(np.float32), R.voice(SR * SECONDS, SR, 2).astype(np.float32)


def events(run, calls, windows, warm=3):
    import torch
    for _ in range(warm):
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


def time_device(lines):
    import torch
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native as N
    from rvc_amd.lib import metrics as M
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.predictors.RMVPE import RMVPE0Predictor
    from rvc_amd.lib.tools import score
    lines.append(f"python tools/time_conversion_score.py (one MI355X; K24, csrc/convscore.hip; {SECONDS} s signals at {SR} Hz, HIP events, "
                 "3 warm-up calls)")
    xa, xb = signals()
    da, db = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    mel = M._mel_matrix(SR, 80, da.device)
    lines.append(f"cepstra, n {da.numel()}, {1 + da.numel() // 80} frames, 80 mels, 24 coefficients: " + events(lambda: N.melcep(da, SR, mel, 24), 10, 20))
    print(lines[-1], flush=True)
    ca, cb = N.melcep(da, SR, mel, 24), N.melcep(db, SR, mel, 24)
    device = {"ca": ca.cpu().numpy(), "cb": cb.cpu().numpy()}
    for band in (-1, 200):
        lines.append(f"dtw {ca.shape[0]} x {cb.shape[0]} x 24, {'no band' if band < 0 else f'band {band}'}: " + events(lambda: N.dtw(ca, cb, band), 2, 10))
        print(lines[-1], flush=True)
        device[band] = N.dtw(ca, cb, band)[0].cpu().tolist()
    rmvpe = RMVPE0Predictor(state_dict=S.make_rmvpe_state_dict(peaked=True), device="cuda:0")
    run = lambda: score.score_conversion((xa, SR), (xb, SR), (xa, SR), predictor=rmvpe, device="cuda:0")  # noqa: E731
    run()
    best = np.inf
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        best = min(best, time.perf_counter() - t0)
    lines.append(f"score_conversion, three {SECONDS} s signals, RMVPE (synthetic weights) included, wall clock, best of 3: {best * 1e3:.1f} ms")
    print(lines[-1], flush=True)
    return device


def time_restatement(lines, device=None):
    """`device`: the device's cepstra and its (total, path length) per band; the restatement then runs on those cepstra and the totals
    are compared"""
    lines.append(f"python tools/time_conversion_score.py --restatement (tests/conversion_score_ref.py, float64 NumPy; the same inputs; cepstra "
                 "best of 3, DTW once)")
    xa, xb = signals()
    best = np.inf
    for _ in range(3):
        t0 = time.perf_counter()
        ca = R.melcep(xa, SR)
        best = min(best, time.perf_counter() - t0)
    lines.append(f"cepstra, n {len(xa)}: {best * 1e3:.1f} ms")
    print(lines[-1], flush=True)
    cb = R.melcep(xb, SR)
    ca, cb = (device["ca"], device["cb"]) if device else (ca.astype(np.float32), cb.astype(np.float32))
    total = 2 * best
    for band in (None, 200):
        t0 = time.perf_counter()
        cost, path = R.dtw(ca, cb, band)
        dt = time.perf_counter() - t0
        if band is None:
            total += dt
        lines.append(f"dtw {len(ca)} x {len(cb)} x 24, {'no band' if band is None else f'band {band}'}: {dt * 1e3:.0f} ms"
                     + (" (the restatement visits every cell whatever the band)" if band else ""))
        if device:
            dev_total, length = device[-1 if band is None else band]
            lines[-1] += f"; the device's total differs by {abs(dev_total - cost) / cost:.2g} relative, path length {int(length)} against {len(path)}"
        print(lines[-1], flush=True)
    fa, fb = R.contour_pair(100 * SECONDS + 1, 1)
    t0 = time.perf_counter()
    R.f0_errors(fa, fb)
    R.mcd_aligned(ca, cb)
    total += time.perf_counter() - t0
    lines.append(f"the scoring of one conversion (two cepstra, DTW, aligned sum, F0 figures; NO pitch estimator): {total * 1e3:.0f} ms")
    print(lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--restatement", action="store_true", help="time the restatement alone and write no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conversion_score.txt"))
    a = ap.parse_args()
    lines, device = [], None
    if not a.restatement:
        device = time_device(lines)
        lines.append("")
    time_restatement(lines, device)
    if not a.restatement:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)
