"""The references of tests/test_vocoder_source_gpu.py, checked against each other without a device.

For every input case the GPU file compares per sample, the float32 oracle (oracle/rvc_oracle.py: source_nsf, _sine_mrf, the first
lines of decoder_refine) and a plain float64 restatement (tests/_vocoder_source_ref.py) must agree to delta <= 1e-6 on EVERY sample:
that is what makes a per-sample gate on the device legitimate.  It holds because every f0 value is k * sr / 1024 (see the module
docstring of _vocoder_source_ref.py); with f0 = 110 + 300 rand the two disagree by more than 1e-6 on more than half the samples of
the MRF source (a flipped wrap flag moves a whole run of samples), which is why the existing gates on har_source are RMS.

Measured delta = max |oracle32 - float64| (voiced and unvoiced frames, the noise term included), no sample above 1e-6 in any case:
  nsf-upp6   T = 1 / 2: 3.9e-9 / 1.1e-8; T = 4096 .. 9000 and the unvoiced / voiced rows: 5.7e-8 .. 5.9e-8
  nsf48-T4300 9.1e-7, nsf40-T64 7.9e-7, nsf32-T64 7.4e-7: the float rounding of 2 pi phase at phase up to 17 (upp k / 1024), which the
             kernel reproduces on purpose
  mrf-upp6   T = 1: 9.1e-9; T = 384 .. 4300 and the unvoiced / voiced rows: 4.7e-8 .. 5.7e-8;  upp 6 .. 1024 at T = 40: 3.2e-8 .. 6.4e-8
  refine     upp 8, T = 255 .. 9000: 5.7e-8 .. 6.2e-8;  upp 64, T = 100: 6.1e-8
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _vocoder_source_ref as R
from conftest import rms


@pytest.mark.parametrize("case", R.SOURCE_CASES, ids=R.SOURCE_IDS)
def test_oracle32_and_float64_agree_on_every_sample(case):
    o32, r64, delta, above = R.source_refs(case)
    lin_w = R.merge_weights(case.hs)[0]
    print(f"{case.name}: L = {o32.shape[1]}, delta = {delta:.2e}, samples above {R.DELTA_MAX:g}: {above}, "
          f"sum |lin_w| = {float(lin_w.abs().sum()):.3f}, GPU gate = {R.source_gate(case):.2e}, rms(har) = {rms(r64):.3f}")
    assert np.isfinite(r64).all() and np.isfinite(o32).all()
    assert above == 0, (case.name, above)
    assert delta <= R.DELTA_MAX, (case.name, delta)


@pytest.mark.parametrize("case", R.SOURCE_CASES, ids=R.SOURCE_IDS)
def test_inputs_are_on_the_grid_and_cross_the_seams(case):
    f0, src_rand, src_randn = R.source_inputs(case)
    k = f0.numpy().astype(np.float64) * (R.GRID / case.hs.sr)
    assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() <= R.K_MAX                # k * sr / 1024, k = 0 .. 36
    assert np.array_equal(src_rand.numpy().astype(np.float64) * 2.0 ** 24, np.round(src_rand.numpy().astype(np.float64) * 2.0 ** 24))
    if case.T > 20:
        assert not torch.equal(f0[0], f0[1])                                                      # the batch rows differ
    assert not torch.equal(src_randn[0], src_randn[1]) and float(src_randn.abs().max()) > 1.0     # non-zero noise, row by row
    if case.hs.kind == "mrf":
        assert not torch.equal(src_rand[0], src_rand[1])                                          # rand_ini per batch entry
        lin_w = R.merge_weights(case.hs)[0].reshape(-1)
        assert len(lin_w) == 9 and len(torch.unique(lin_w.abs())) == 9 and float(lin_w.abs().min()) > 0.01    # every harmonic its own weight
    rows = case.rows or ("mixed",) * R.BATCH
    for b, kind in enumerate(rows):
        voiced = f0[b] > 0
        if kind == "unvoiced":
            assert not voiced.any()
        elif kind == "voiced":
            assert voiced.all() and len(torch.unique(f0[b])) > min(case.T, 8) // 2                # varies frame by frame
        else:
            for i in case.changes:
                if 1 <= i < case.T:                                                               # voiced <-> unvoiced exactly there
                    assert bool(voiced[i]) != bool(voiced[i - 1]), (case.name, b, i)
            if case.T - 1 in case.changes and case.T > 1:                                         # a last frame just behind a seam is heard
                assert bool(voiced[-1]) == (b % 2 == 0), (case.name, b)


def test_float64_restatement_sees_a_lost_carry():
    """What the GPU gate is for: dropping the running sum at one chunk seam moves the samples behind it by far more than the gate."""
    case = next(c for c in R.SOURCE_CASES if c.name == "nsf-upp6-T9000")
    f0, src_rand, src_randn = R.source_inputs(case)
    upp = R.upp_of(case.hs)
    lin_w, lin_b = R.merge_weights(case.hs)
    good = R.source_refs(case)[1]
    cut = 4097                                                  # frames from here on start from a zero carry
    tail = R.nsf_source64(f0.numpy()[:, cut:], upp, case.hs.sr, lin_w.numpy(), lin_b.numpy(), src_randn.numpy()[:, cut * upp:])
    voiced = np.repeat(f0.numpy()[:, cut:] > 0, upp, axis=1)
    diff = np.abs(tail - good[:, cut * upp:])[voiced]
    print(f"lost carry at frame {cut}: max |difference| on the voiced samples behind it = {diff.max():.2e}, gate {R.source_gate(case):.2e}")
    assert diff.max() > 1e-3 > 100 * R.source_gate(case)


def test_linear_resize64_is_torchs_rule():
    x = torch.randn(2, 37, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for n in (37 * 8, 37 * 64, 5):
        want = F.interpolate(x[:, None, :], size=n, mode="linear")[:, 0].numpy()
        assert np.abs(R.linear_resize64(x.numpy(), n) - want).max() <= 1e-12


def test_noise_conv_routes_of_the_glue_cases():
    """The comment above GLUE_CASES, computed: which stages fold the noise conv into the upsampler's GEMM (rvc_decoder_finalize)."""
    def separate(rates, init_ch):
        out = []
        for i, r in enumerate(rates):
            stride = int(np.prod(rates[i + 1:])) if i + 1 < len(rates) else 1
            nc_k = 1 if stride == 1 else stride * 2 - stride % 2
            vk_rows = ((r - 1) * stride + nc_k + 7) // 8 * 8
            out.append(vk_rows * 2 >= init_ch >> i)
        return out
    assert separate((3, 2), 128) == [False, False] and separate((3, 3), 128) == [False, False] and separate((5, 3), 128) == [False, False]
    assert separate((9, 7), 128) == [True, False] and separate((8, 8), 128) == [True, False]
    kinds = {(c.hs.kind, tuple(c.hs.rates)) for c in R.GLUE_CASES}
    assert ("mrf", (9, 7)) in kinds and ("nsf", (8, 8)) in kinds and ("nsf", (3, 2)) in kinds


@pytest.mark.parametrize("case", R.GLUE_CASES, ids=R.GLUE_IDS)
def test_glue_references_are_loud_enough(case):
    """The whole-decoder gate of the GPU file is rms(out - ref) <= 5e-5 with rms(ref) > 0.02, over the waveform and over its first and
    last upp samples: the seeds are chosen here so that the second half holds."""
    ref = R.glue_ref(case)
    upp = R.upp_of(case.hs)
    assert ref.shape == (R.BATCH, 1, case.T * upp) and np.isfinite(ref).all()
    figures = [rms(ref), rms(ref[:, :, :upp]), rms(ref[:, :, -upp:])]
    print(f"{case.name}: L = {ref.shape[-1]} (L % 4 = {ref.shape[-1] % 4}), rms(ref) whole / first upp / last upp = "
          + " / ".join(f"{v:.3f}" for v in figures))
    assert min(figures) > 0.02, figures
