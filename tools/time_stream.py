"""Per-push latency of a conversion stream (VoiceConverter.open_stream, K21) on the BASELINE cfg 2 model: 48 kHz NSF-HiFi-GAN,
100 000 x 768 index, index_rate 0.75, rmvpe, 1 s of context, 50 ms crossfade, 10 ms search, at block_ms 100 / 250 / 500.  Device
tensors in and out; every push is timed on its own (HIP events on the stream it runs on, and the host's wall clock from the call to
the end of a synchronise: a live caller waits for every block); median and maximum of 50 pushes after 5 warm-up pushes.  Then
convert_array on the very same windows, timed the same way: the difference is what the window kernel, the SOLA join and the
stream's bookkeeping add.  Both with noise drawn on the device (noise_seed=None, how a live caller runs) and in parity mode
(noise_seed=7: the noise comes from torch's CPU generator).  DESIGN.md K21, profiles/stream_latency.txt.
    python tools/time_stream.py"""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd")]
import torch
from rvc_amd.infer.infer import VoiceConverter
from rvc_amd.lib import synthetic as S

DEV, WARM, PUSHES = "cuda:0", 5, 50
vc = VoiceConverter(device=DEV)
vc.load_checkpoint_dict(S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0))
vc.load_hubert_state_dict(S.make_hubert_state_dict(1))
vc.vc.load_rmvpe_state_dict(S.make_rmvpe_state_dict(0))
vc.vc.set_index(S.synth_index(100_000, seed=0))


def timed(fn, args):
    """fn(arg) for every arg, each timed alone -> (event ms, wall ms) arrays without the warm-up calls"""
    ev, wall = [], []
    for a in args:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        fn(a)
        stop.record()
        stop.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(start.elapsed_time(stop))
    return np.array(ev[WARM:]), np.array(wall[WARM:])


def line(what, ev, wall, block_ms):
    print(f"{what}: events median {np.median(ev):.3f} ms, max {ev.max():.3f}; wall median {np.median(wall):.3f} ms, max {wall.max():.3f}; "
          f"real-time factor {block_ms / np.median(wall):.1f} (median), {block_ms / wall.max():.1f} (slowest push)", flush=True)


for seed in (None, 7):
    for block_ms in (100, 250, 500):
        stream = vc.open_stream(block_ms=block_ms, context_ms=1000, crossfade_ms=50, search_ms=10, index_rate=0.75, protect=0.5, noise_seed=seed)
        plan, n = stream.plan, WARM + PUSHES
        audio = torch.from_numpy(S.synth_audio(n * plan.block_samples, seed=3).astype(np.float32) * 0.9).to(DEV)
        blocks = [audio[j * plan.block_samples:(j + 1) * plan.block_samples] for j in range(n)]
        padded = torch.cat([torch.zeros(plan.hist_samples, device=DEV), audio])
        windows = [padded[j * plan.block_samples:j * plan.block_samples + plan.window_samples].clone() for j in range(n)]
        torch.cuda.synchronize()
        tag = f"block {block_ms} ms (window {plan.window_samples / 16:.0f} ms, latency {stream.latency_ms} ms), noise_seed={seed}"
        ev_s, wall_s = timed(stream.push, blocks)
        line(f"push          {tag}", ev_s, wall_s, block_ms)
        counter = iter(range(n))
        ev_c, wall_c = timed(lambda w: vc.convert_array(w, index_rate=0.75, protect=0.5, noise_seed=None if seed is None else seed + next(counter)),
                             windows)
        line(f"convert_array {tag}", ev_c, wall_c, block_ms)
        print(f"  the stream adds: events {np.median(ev_s) - np.median(ev_c):+.3f} ms ({100 * (np.median(ev_s) / np.median(ev_c) - 1):+.1f} %), "
              f"wall {np.median(wall_s) - np.median(wall_c):+.3f} ms ({100 * (np.median(wall_s) / np.median(wall_c) - 1):+.1f} %) at the median",
              flush=True)
        stream.close()
