"""The vocoders' source modules past their chunk seams, sample by sample, and the glue kernels behind them through whole small decoders.

1. har_source per sample (test_har_source_per_sample): the tap of Decoder.set_tap(-1, ...) against the float32 oracle on EVERY sample,
   for inputs on which the oracle itself has no near-ties (tests/_vocoder_source_ref.py; tests/test_vocoder_source_cpu.py asserts
   delta = max |oracle32 - float64| <= 1e-6 for each of these cases).  Gate: max(4 delta, 2^-21 max(1, sum_h |lin_w[h]|)) -- 4 x for the
   device's sinf / tanhf differing from libm by a few ulp, the floor two float ulps of 1 per harmonic after the merge -- and NO sample
   may exceed it: an indexing or carry error moves the phase by O(0.1) and the output by >= 1e-3.  The cases cross every seam the
   kernels have: nsf_carry_kernel's chunks of 4096 frames, mrf_prefix_kernel's of 384 frames, the RefineGAN scan's blocks of 2048
   samples, mrf_source_kernel's 256-lane slices (upp 6 .. 1024), with batch 2, different rows and non-zero noise throughout.
2. Windows that start beyond a seam (test_window_beyond_a_seam): forward(keep=(lo, hi)) against the full forward sliced, relative
   RMS <= 1e-5 over the kept region, its first and its last frame (the gate and the triple of tests/test_decoder_window_gpu.py).
3. Whole small decoders against the oracle (test_small_decoder_matches_oracle): rms(out - ref) <= 5e-5 with rms(ref) > 0.02 (the gate of
   test_decoder_matches_oracle), separately over the waveform, its first and its last upp samples: cond_bias_kernel at gin 40 / 64 /
   100 / 256, conv_post_kernel's scalar path over whole signals (L % 4 = 1, 2, 3), odd upsampling rates, both noise-conv routes,
   RefineGAN's interpolation / down-sampling kernels at odd T.

Measured on one MI355X: see the docstrings of the tests.  The whole file takes 6 s there.
"""
import numpy as np
import pytest
import torch

import _vocoder_source_ref as R
from conftest import rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_HANDLES = {}


def handle(hs):
    """One native Decoder per handle spec for the whole module."""
    if hs not in _HANDLES:
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        from rvc_amd import _native
        _HANDLES[hs] = R.make_native_decoder(_native, hs)
        assert _HANDLES[hs].upp == R.upp_of(hs)
    return _HANDLES[hs]


def adain_zeros(hs, T):
    """RefineGAN's AdaIN noise, flat, all zero (the source tap does not depend on it)."""
    if hs.kind != "refine":
        return None
    n, length, ch = 0, T, hs.init_ch
    for r in R.weights(hs)[1]:
        length, ch = length * r, ch // 2
        n += 6 * R.BATCH * ch * length
    return torch.zeros(n, device=DEV)


def conv_inputs(hs, T, seed):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(R.BATCH, hs.inter, T, generator=gen)
    g = torch.randn(R.BATCH, hs.gin, generator=gen)
    return z.to(DEV), g.to(DEV)


# ------------------------------------------------------------------------------------------------------------------
# 1. har_source per sample
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SOURCE_CASES, ids=R.SOURCE_IDS)
def test_har_source_per_sample(case):
    """Measured on one MI355X, max |tap - oracle32| over all samples of both rows (samples above the gate: 0 in every case):
      NSF  upp 6, T = 1 / 2: 3.7e-9 / 1.5e-8; T = 4096 .. 9000, the unvoiced / voiced rows, nsf48 T = 4300 (4.1 M samples), nsf40, nsf32:
           3.0e-8 each (one ulp of a tanh near 0.4) -- gate 6.4e-7 (upp 6), 3.7e-6 / 3.2e-6 / 3.0e-6 (48 k / 40 k / 32 k: 4 delta)
      MRF  upp 6, T = 1: 7.5e-9; T = 384 / 385 / 769: 3.0e-8; T = 4300: 4.5e-8; upp 6 .. 400 at T = 40: 3.0e-8; upp 800 / 1024: 4.5e-8;
           the unvoiced / voiced rows: 3.0e-8 -- gate 1.1e-6 (2^-21 sum |lin_w|, sum = 2.34)
      RefineGAN  upp 8, T = 255 / 256 / 257 / 513 / 9000: 3.0e-8 / 3.0e-8 / 3.0e-8 / 2.2e-8 / 3.0e-8; upp 64, T = 100: 3.0e-8 -- gate 7.0e-7
    and max |tap - float64| equals the case's delta to two digits (5e-8 .. 6e-8; 9.1e-7 for nsf48): the device reproduces the oracle's
    float32 arithmetic, rounding of 2 pi phase included."""
    hs = case.hs
    dec = handle(hs)
    f0, src_rand, src_randn = R.source_inputs(case)
    o32, r64, delta, above = R.source_refs(case)
    gate = R.source_gate(case)
    assert above == 0 and delta <= R.DELTA_MAX, (delta, above)           # (tests/test_vocoder_source_cpu.py says why)
    z, g = conv_inputs(hs, case.T, 11)
    tap = torch.zeros(R.BATCH, case.T * dec.upp, device=DEV)
    dec.set_tap(-1, tap)
    try:
        out = dec.forward(z, f0.to(DEV), g, src_randn=src_randn.to(DEV), src_rand=src_rand.to(DEV), adain_randn=adain_zeros(hs, case.T))
        torch.cuda.synchronize()
    finally:
        dec.set_tap(-1, None)
    got = tap.cpu().numpy().astype(np.float64)
    diff = np.abs(got - o32.astype(np.float64))
    worst = np.unravel_index(int(diff.argmax()), diff.shape)
    n_above = int((diff > gate).sum())
    print(f"{case.name}: max |tap - oracle32| = {diff.max():.2e} at row {worst[0]}, sample {worst[1]} (frame {worst[1] // dec.upp}); "
          f"max |tap - float64| = {np.abs(got - r64).max():.2e}; delta = {delta:.2e}, gate = {gate:.2e}, samples above the gate: {n_above} of {diff.size}")
    assert out.shape == (R.BATCH, 1, case.T * dec.upp) and bool(torch.isfinite(out).all())
    assert n_above == 0, (case.name, n_above, float(diff.max()), [int(v) for v in worst])


# ------------------------------------------------------------------------------------------------------------------
# 2. windows that start beyond a seam
# ------------------------------------------------------------------------------------------------------------------
WINDOW_GATE = 1e-5
# (handle, T, the f0 changes): the small upp 6 decoders
WINDOW_HANDLES = {"nsf": (R.NSF_TINY, 9000, R.NSF_SEAMS), "mrf": (R.MRF_TINY, 1200, R.MRF_SEAMS)}
# (name, kind, seam frame, offset of the FIRST FRAME THE STACK RUNS OVER (keep_lo - margin) from the seam, kept frames)
WINDOWS = [(f"{kind}-seam{seam}-ext{off:+d}", kind, seam, off, 12)
           for kind, seams in (("nsf", (4096, 8192)), ("mrf", (384, 768))) for seam in seams for off in (-1, 0, 1)]
# ... and windows whose own first frame is the seam's neighbour / the seam, odd lo with an odd length, and an odd left-clipped one
# (ext_lo = 0, so o_lo = 6 lo is no multiple of 4; n_out = 6 x odd never is)
WINDOWS += [("nsf-keep4095-odd", "nsf", 4095, None, 7), ("nsf-keep4096", "nsf", 4096, None, 12), ("nsf-keep4097-odd", "nsf", 4097, None, 9),
            ("mrf-keep383-odd", "mrf", 383, None, 7), ("mrf-keep384", "mrf", 384, None, 12), ("mrf-keep769-odd", "mrf", 769, None, 5),
            ("nsf-keep3-odd-left-clipped", "nsf", 3, None, 7), ("mrf-keep5-odd-left-clipped", "mrf", 5, None, 3)]
_FULL = {}


def window_inputs(kind):
    """(decoder, args, noise kwargs, full forward) of a window handle: computed once, shared by every window, never modified."""
    if kind not in _FULL:
        hs, T, changes = WINDOW_HANDLES[kind]
        dec = handle(hs)
        dim = 9 if kind == "mrf" else 1
        f0 = R.grid_f0(3, T, R.BATCH, hs.sr, changes)
        gen = torch.Generator().manual_seed(77)
        src_rand = torch.rand(R.BATCH, dim, generator=gen)
        src_randn = torch.randn(R.BATCH, T * dec.upp, dim, generator=gen)
        z, g = conv_inputs(hs, T, 12)
        args = (z, f0.to(DEV), g)
        kw = dict(src_randn=src_randn.to(DEV), src_rand=src_rand.to(DEV))
        full = dec.forward(*args, **kw)
        torch.cuda.synchronize()
        _FULL[kind] = (dec, T, args, kw, full)
    return _FULL[kind]


@pytest.mark.parametrize("name,kind,frame,ext_off,n_keep", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_window_beyond_a_seam(name, kind, frame, ext_off, n_keep):
    """Measured on one MI355X (relative RMS): kept 1.5e-7 .. 4.7e-7, first frame 1.0e-7 .. 5.3e-7, last frame 1.6e-7 .. 6.5e-7 over the 20
    windows (worst: nsf-keep4096, 4.7e-7 / 4.8e-7 / 6.5e-7), against the gate of 1e-5.  The margin of the (3, 2) decoders is 35 frames, so
    o_lo = 210 (o_lo % 4 = 2) in every interior window, 18 and 30 in the left-clipped ones; n_out % 4 = 2 in the odd-length ones."""
    dec, T, args, kw, full = window_inputs(kind)
    upp, margin = dec.upp, dec.window_margin()
    assert 0 < margin < 300
    lo = frame if ext_off is None else frame + ext_off + margin      # the stack then starts at frame seam + ext_off
    hi = lo + n_keep
    got = dec.forward(*args, **kw, keep=(lo, hi))
    torch.cuda.synchronize()
    assert got.shape == (R.BATCH, 1, n_keep * upp)
    want = full[:, :, lo * upp:hi * upp].cpu().numpy().astype(np.float64)
    got = got.cpu().numpy().astype(np.float64)
    parts = (("kept", slice(None)), ("first frame", slice(0, upp)), ("last frame", slice(-upp, None)))
    o_lo = min(lo, margin) * upp
    print(f"window {name}: frames [{lo}, {hi}) of {T}, margin {margin}, o_lo % 4 = {o_lo % 4}, n_out % 4 = {n_keep * upp % 4}: relative RMS "
          + ", ".join(f"{part} {rms(got[:, :, sl] - want[:, :, sl]) / rms(want[:, :, sl]):.2e}" for part, sl in parts))
    for part, sl in parts:
        assert rms(got[:, :, sl] - want[:, :, sl]) <= WINDOW_GATE * rms(want[:, :, sl]), (name, part)


# ------------------------------------------------------------------------------------------------------------------
# 3. the glue kernels through whole small decoders
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GLUE_CASES, ids=R.GLUE_IDS)
def test_small_decoder_matches_oracle(case):
    """Measured on one MI355X, rms(out - ref) whole / first upp / last upp samples, against the gate of 5e-5:
      nsf-3x2-gin40-T33   8.8e-8 / 5.9e-8 / 5.6e-8      mrf-3x2-gin100-T34  1.2e-7 / 1.2e-7 / 9.5e-8      nsf-3x3-gin64-T33  8.8e-8 / 5.2e-8 / 7.1e-8
      mrf-3x3-gin256-T35  1.2e-7 / 8.3e-8 / 5.6e-8      nsf-5x3-T200        1.0e-7 / 8.6e-8 / 9.8e-8      mrf-9x7-T33        1.3e-7 / 9.6e-8 / 9.7e-8
      nsf-8x8-T40         9.3e-8 / 6.9e-8 / 7.2e-8      refine-4x2-gin64-T33  1.0e-7 / 8.7e-8 / 8.6e-8    refine-2x2x2-gin100-T67  1.3e-7 / 1.2e-7 / 1.1e-7
    (rms(ref) 0.13 .. 0.31 whole, 0.06 .. 0.33 over the end pieces: tests/test_vocoder_source_cpu.py asserts > 0.02 for each)"""
    hs = case.hs
    dec = handle(hs)
    upp = dec.upp
    z, f0, g, src_rand, src_randn, adain = R.glue_inputs(case)
    ref = R.glue_ref(case).astype(np.float64)
    adain_flat = torch.cat([a.reshape(-1) for a in adain]).to(DEV) if adain else None
    out = dec.forward(z.to(DEV), f0.to(DEV), g[:, :, 0].contiguous().to(DEV), src_randn=src_randn.to(DEV), src_rand=src_rand.to(DEV),
                      adain_randn=adain_flat)
    torch.cuda.synchronize()
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape == (R.BATCH, 1, case.T * upp)
    parts = (("whole", slice(None)), ("first upp", slice(0, upp)), ("last upp", slice(-upp, None)))
    print(f"{case.name}: L = {ref.shape[-1]} (L % 4 = {ref.shape[-1] % 4}): rms err "
          + ", ".join(f"{part} {rms(out[:, :, sl] - ref[:, :, sl]):.2e} (ref {rms(ref[:, :, sl]):.3f})" for part, sl in parts))
    for part, sl in parts:
        assert rms(ref[:, :, sl]) > 0.02, (case.name, part)
        assert rms(out[:, :, sl] - ref[:, :, sl]) <= 5e-5, (case.name, part, rms(out[:, :, sl] - ref[:, :, sl]))
