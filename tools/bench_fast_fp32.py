#!/usr/bin/env python3
"""The opt-in fast-fp32 vocoder mode (K3h, convbf1.hip: fp32 taps and activations as error-corrected fp16 pairs, three matrix products per
multiply-add) against the exact path, at the cfg-2 vocoder's 256- and 128-channel stage lengths (30 s at 48 kHz: 38 376 and 383 760 samples).

Per (C, K, dilation): the (dilated conv, conv + residual) pair of one ResBlock dilation as two launches of K3h against what the exact
handle runs for that layer -- two launches of the bf16x3 Winograd form (K3y, winobf2.hip), or the fused pair (K3f, resblock_bf.hip) at
C = 128 with 3 taps.  Both sides in one process, interleaved per shape, HIP events, median of 5 batches of 6 pairs.
Then one 30 s NSF-48k decoder forward with arithmetic "exact" and "fp16x2" (median of 7 after 2 warm-ups), and their waveform difference.
convbf1_preferred(CB1_F16X2, ..) (convbf1.hip) takes the (C, K) where K3h wins here; profiles/fastfp32_conv_shapes.txt is this tool's output."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd")]
import torch
from rvc_amd import _native
dev = "cuda:0"
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, batches=5, reps=6, warm=2):
    for _ in range(warm): fn()
    out = []
    for _ in range(batches):
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return sorted(out)[len(out) // 2]


print(f"device: {torch.cuda.get_device_name(0)}")
if "--decoder-only" not in sys.argv:
    for C, L in ((256, 38376), (128, 383760)):
        x = torch.randn(1, C, L, device=dev); bias = torch.zeros(C, device=dev)
        t1 = torch.empty_like(x); y = torch.empty_like(x)
        for K in tuple(int(k) for k in os.environ.get("BENCH_K", "3,7,11").split(",")):
            w1, w2 = torch.randn(C, C, K) * 0.03, torch.randn(C, C, K) * 0.03
            h1, h2 = _native.conv1d_f16x2_pack_weight(w1, dev), _native.conv1d_f16x2_pack_weight(w2, dev)
            pair = C == 128 and K == 3                     # resblock_bf_preferred: the exact handle runs this layer as a fused pair
            if pair:
                up = _native.resblock_bf16x3_pack_weight(w1, w2, dev)
            else:
                u1, u2 = _native.conv1d_winobf_pack_weight(w1, dev), _native.conv1d_winobf_pack_weight(w2, dev)
            for dil in (1, 3, 5):
                def exact():
                    if pair:
                        _native.resblock_bf16x3_forward(x, up, bias, bias, K, dil, 0.1, out=y)
                    else:
                        _native.conv1d_winobf_forward(x, u1, bias, C, K, dil, 0.1, out=t1)
                        _native.conv1d_winobf_forward(t1, u2, bias, C, K, 1, 0.1, res=x, out=y)

                def fast():
                    _native.conv1d_f16x2_forward(x, h1, bias, K, dil, 0.1, out=t1)
                    _native.conv1d_f16x2_forward(t1, h2, bias, K, 1, 0.1, res=x, out=y)
                mse, msf = timed(exact), timed(fast)
                mse2, msf2 = timed(exact), timed(fast)     # again, the other way round in time: drift shows as a disagreement
                exe = 2 * 2.0 * C * C * K * L * 3 / 1e9    # fp16 matrix flops executed (direct form, three products)
                print(f"C={C:3d} K={K:2d} d={dil} L={L:7d}: the pair: exact ({'K3f fused pair' if pair else 'K3y, two launches'}) {mse*1e3:7.1f} / {mse2*1e3:7.1f} us | "
                      f"fp16 pairs (K3h, two launches) {msf*1e3:7.1f} / {msf2*1e3:7.1f} us  x{min(mse, mse2)/max(msf, msf2):.2f} .. x{max(mse, mse2)/min(msf, msf2):.2f} "
                      f"({exe/msf:6.1f} TF/s on the fp16 pipe = {exe/msf/2500*100:.0f} % of 2.5 PF)", flush=True)

from rvc_amd.lib import synthetic as S
from rvc_amd.lib.algorithm.weights import fold_weight_norm
cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0)
folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
T = 3198
z = torch.randn(1, 192, T, device=dev); f0 = torch.full((1, T), 220.0, device=dev); g = torch.randn(1, 256, device=dev)
nz = torch.randn(1, T * 480, 1, device=dev); rnd = torch.zeros(1, 1, device=dev)
decs = {a: _native.Decoder("HiFi-GAN", 48000, folded, arithmetic=a) for a in ("exact", "fp16x2")}
outs, ms = {}, {}
for rnd_i in range(2):                                     # exact, fast, exact, fast
    for a, dec in decs.items():
        outs[a] = dec.forward(z, f0, g, src_randn=nz, src_rand=rnd).clone()
        ms.setdefault(a, []).append(timed(lambda: dec.forward(z, f0, g, src_randn=nz, src_rand=rnd), batches=7, reps=1))
d = (outs["fp16x2"] - outs["exact"]).double()
print(f"NSF-48k decoder forward, 30 s (T = {T}): exact {ms['exact'][0]:.2f} / {ms['exact'][1]:.2f} ms | fp16x2 {ms['fp16x2'][0]:.2f} / {ms['fp16x2'][1]:.2f} ms "
      f"(saves {min(ms['exact']) - max(ms['fp16x2']):.2f} .. {max(ms['exact']) - min(ms['fp16x2']):.2f} ms); waveform rms difference "
      f"{d.pow(2).mean().sqrt().item():.2e} (signal rms {outs['exact'].double().pow(2).mean().sqrt().item():.3f})")
