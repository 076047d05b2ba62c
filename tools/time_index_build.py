#!/usr/bin/env python3
"""Times the feature-index builder (K16) at its two workload shapes with HIP events; prints one JSON line per measurement.

  small   100 000 x 768 rows -> IVF2564,Flat, 10 Lloyd iterations                         (extract_index.py below 2e5 rows)
  large   1 000 000 x 768 rows reduced to 10 000 centres over 20 Lloyd iterations          (the reference's MiniBatchKMeans step)

  assign   rvc_kmeans_assign against the only other native route to the same answer: rvc_knn_search over the centroids in query
           chunks sized to its workspace, column 0 taken -- in its exact-fp32 regime and, where the shape allows it (>= 4096
           centroids), its fp16-screened regime.  Same process, same events, alternating.  Also the share of the 157.3 TF
           exact-fp32 matrix rate (2 n k d flop over the call's time: norms + GEMM + finish kernels).
  update   rvc_kmeans_update; n * dim * 4 bytes over its time against the 8.0 TB/s HBM peak.
  build    kmeans.lloyd / kmeans.build_ivf_flat_device end to end (host bookkeeping included), and with --host the float64 NumPy
           faiss_index.build_ivf_flat at the small shape: one iteration timed (build with 1 iteration minus build with 0) and scaled.

    python tools/time_index_build.py --warmup 1 --steps 3 [--shapes small,large] [--host]
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d OUT -- python tools/time_index_build.py --only update     (counters: a run of their own)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd")]

import numpy as np
import torch

from rvc_amd import _native
from rvc_amd.lib import faiss_index, kmeans

DEV = "cuda:0"
PEAK_F32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
SHAPES = {"small": dict(n=100_000, k=2564, d=768, iterations=10), "large": dict(n=1_000_000, k=10_000, d=768, iterations=20)}
KNN_CHUNK = 16384   # queries per rvc_knn_search call: 2 MB of its per-slot lists per stripe, 0.7 GB in the screened regime


def draw(n, d, seed):
    """rvc_amd.lib.synthetic.synth_index's recipe on the device: 512 centres, jitter 0.05"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    centres = torch.randn(512, d, device=DEV, generator=g) * 0.35
    x = torch.empty(n, d, device=DEV)
    for s in range(0, n, 1 << 18):
        e = min(n, s + (1 << 18))
        x[s:e] = centres[torch.randint(0, 512, (e - s,), device=DEV, generator=g)] + 0.05 * torch.randn(e - s, d, device=DEV, generator=g)
    return x


def timed(fn, warmup, steps):
    """seconds per call (HIP events around `steps` calls), last result"""
    out = None
    for _ in range(warmup):
        out = fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps, out


def knn_route(x, cent, aux, mode):
    _native.knn_set_mode(mode)
    try:
        return torch.cat([_native.knn_search(cent, aux, x[s:s + KNN_CHUNK])[1][:, 0] for s in range(0, x.shape[0], KNN_CHUNK)])
    finally:
        _native.knn_set_mode(0)


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--only", default="", help="'update': time nothing but rvc_kmeans_update (for a counter run of its own)")
    ap.add_argument("--host", action="store_true", help="also time faiss_index.build_ivf_flat (float64 NumPy) at the small shape")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to time without one"
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        n, k, d, iterations = sh["n"], sh["k"], sh["d"], sh["iterations"]
        x = draw(n, d, 0)
        cent = x[torch.from_numpy(np.random.default_rng(0).choice(n, k, replace=False)).to(DEV)].contiguous()
        cent, _, _ = kmeans.lloyd_step(x, cent)                      # centroids as an iteration sees them, not raw rows
        flop = 2.0 * n * k * d
        if args.only == "update":
            order, offsets, _ = kmeans._sorted_members(_native.kmeans_assign(x, cent)[0], k)
            t_upd, _ = timed(lambda: _native.kmeans_update(x, order, offsets, cent), args.warmup, args.steps)
            report(what="update", shape=name, n=n, k=k, d=d, kmeans_update_ms=t_upd * 1e3, gbytes_per_s=n * d * 4 / t_upd / 1e9)
            continue
        # ---- assign ---------------------------------------------------------------------------------------------
        aux = _native.knn_index_build(cent)
        t_new, (ids, _) = timed(lambda: _native.kmeans_assign(x, cent), args.warmup, args.steps)
        t_knn, ids_knn = timed(lambda: knn_route(x, cent, aux, 1), args.warmup, args.steps)
        t_new2, _ = timed(lambda: _native.kmeans_assign(x, cent), 0, args.steps)     # alternate: the spread of the same call
        row = dict(what="assign", shape=name, n=n, k=k, d=d, kmeans_assign_ms=t_new * 1e3, kmeans_assign_again_ms=t_new2 * 1e3,
                   knn_search_exact_ms=t_knn * 1e3, ratio_exact=t_knn / t_new, tflops=flop / t_new / 1e12,
                   share_of_f32_matrix_peak=flop / t_new / PEAK_F32_MATRIX,
                   same_ids_as_knn_search=float((ids.to(torch.int64) == ids_knn).double().mean()))
        if k >= 4096 and d % 256 == 0:
            t_scr, ids_scr = timed(lambda: knn_route(x, cent, aux, 2), args.warmup, args.steps)
            row.update(knn_search_screened_ms=t_scr * 1e3, ratio_screened=t_scr / t_new,
                       same_ids_as_screened=float((ids.to(torch.int64) == ids_scr).double().mean()))
        report(**row)
        # ---- update ---------------------------------------------------------------------------------------------
        order, offsets, _ = kmeans._sorted_members(ids, k)
        t_upd, _ = timed(lambda: _native.kmeans_update(x, order, offsets, cent), args.warmup, args.steps)
        report(what="update", shape=name, n=n, k=k, d=d, kmeans_update_ms=t_upd * 1e3, gbytes_per_s=n * d * 4 / t_upd / 1e9,
               share_of_hbm_peak=n * d * 4 / t_upd / PEAK_HBM)
        t_sort, _ = timed(lambda: kmeans._sorted_members(ids, k), args.warmup, args.steps)
        report(what="sort+offsets (torch)", shape=name, ms=t_sort * 1e3)
        # ---- the whole build ------------------------------------------------------------------------------------
        if name == "large":
            t_build, (c, inertia) = timed(lambda: kmeans.lloyd(x, k, iterations, 0), 0, 1)
            report(what="lloyd (the reduction)", shape=name, iterations=iterations, seconds=t_build, inertia_first=inertia[0], inertia_last=inertia[-1])
            del x
            big = c.cpu().numpy()
            nlist = min(int(16 * np.sqrt(k)), k // 39)
            t0 = time.perf_counter()
            ivf = kmeans.build_ivf_flat_device(big, nlist, seed=0, device=DEV)
            report(what="build_ivf_flat_device on the centres", shape=name, nlist=nlist, seconds=time.perf_counter() - t0, ntotal=ivf.ntotal)
        else:
            big = x.cpu().numpy()
            del x
            for _ in range(args.warmup):
                kmeans.build_ivf_flat_device(big, k, seed=0, iterations=iterations, device=DEV)
            t0 = time.perf_counter()
            ivf = kmeans.build_ivf_flat_device(big, k, seed=0, iterations=iterations, device=DEV)
            t_dev = time.perf_counter() - t0
            report(what="build_ivf_flat_device (upload, lloyd, lists)", shape=name, nlist=k, iterations=iterations, seconds=t_dev,
                   empty_lists=int(sum(a.size == 0 for a in ivf.list_ids)))
            if args.host:
                t0 = time.perf_counter()
                faiss_index.build_ivf_flat(big, k, seed=0, iterations=0)
                t_0 = time.perf_counter() - t0
                t0 = time.perf_counter()
                faiss_index.build_ivf_flat(big, k, seed=0, iterations=1)
                t_1 = time.perf_counter() - t0
                report(what="build_ivf_flat on the host (float64 NumPy)", shape=name, seconds_0_iterations=t_0, seconds_1_iteration=t_1,
                       seconds_scaled_to_iterations=t_0 + iterations * (t_1 - t_0), iterations=iterations,
                       threads=torch.get_num_threads())
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
