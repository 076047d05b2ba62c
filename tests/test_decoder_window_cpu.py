"""rvc_decoder_window_margin against the float64 oracle, on the host: the kept region of the vocoder's output must not change AT ALL
when everything the window entry does not look at is replaced -- z and the source-noise draws outside [lo - margin, hi + margin).

Exactly 0.0 is the only check sharp enough for an off-by-one margin: one frame short shows as ~1e-10 (48 k) in float64, far below
anything an fp32 comparison on the device could see.  The margin must also stay within one frame of the smallest exact one (10 / 11 /
11 / 10 frames, measured with this probe): a huge margin would pass the first check and give the saving away."""
import numpy as np
import pytest
import torch

T, LO, HI = 64, 26, 38
CONFIGS = [("nsf48", 48000, "HiFi-GAN", 10), ("nsf40", 40000, "HiFi-GAN", 11), ("nsf32", 32000, "HiFi-GAN", 11),
           ("mrf48", 48000, "MRF HiFi-GAN", 10)]


class _Case:
    """One synthetic float64 vocoder with its inputs; run(z, randn) -> waveform [T * upp]."""

    def __init__(self, sr, voc):
        from oracle import rvc_oracle as O
        from rvc_amd.lib import synthetic as S
        from rvc_amd import _native
        self.O, self.sr, self.mrf = O, sr, voc.startswith("MRF")
        cpt = S.make_synth_checkpoint(sr, voc, seed=0)
        self.w = {k: v.double() for k, v in O.fold_weight_norm(cpt["weight"]).items()}
        self.rates, self.ksizes = list(cpt["config"][12]), list(cpt["config"][14])
        self.upp = int(np.prod(self.rates))
        self.margin = _native.decoder_window_margin(voc, sr, upsample_rates=self.rates, upsample_kernel_sizes=self.ksizes)
        gen = torch.Generator().manual_seed(11)
        dim = 9 if self.mrf else 1
        self.z = torch.randn(1, 192, T, generator=gen, dtype=torch.float64)
        self.g = torch.randn(1, 256, 1, generator=gen, dtype=torch.float64)
        f0 = 110.0 + 200.0 * torch.rand(1, T, generator=gen, dtype=torch.float64)
        f0[:, 5:9] = 0.0          # unvoiced gaps before, inside and after the window
        f0[:, 30:32] = 0.0
        f0[:, 50:53] = 0.0
        self.f0 = f0
        self.src_rand = torch.rand(1, dim, generator=gen, dtype=torch.float64)
        self.randn = torch.randn(1, T * self.upp, dim, generator=gen, dtype=torch.float64)
        self.other_z = torch.randn(1, 192, T, generator=gen, dtype=torch.float64) * 3.0
        self.other_randn = torch.randn(1, T * self.upp, dim, generator=gen, dtype=torch.float64) * 3.0
        self.ref = self.run(self.z, self.randn)

    def run(self, z, randn):
        O = self.O
        with torch.no_grad():
            if self.mrf:
                out = O.decoder_mrf(self.w, z, self.f0, self.g, self.rates, self.ksizes, self.sr, O.ListNoise([self.src_rand.clone(), randn]))
            else:
                out = O.decoder_nsf(self.w, z, self.f0, self.g, self.rates, self.ksizes, self.sr,
                                    O.ListNoise([torch.zeros(1, 1, 1, dtype=torch.float64), randn]))
        return out[0, 0].numpy()

    def outside_replaced(self, lo, hi, m):
        """max |difference| over the samples of frames [lo, hi) after replacing z and the noise draws outside [lo - m, hi + m)."""
        a, b = max(0, lo - m), min(T, hi + m)
        z, randn = self.other_z.clone(), self.other_randn.clone()
        z[:, :, a:b] = self.z[:, :, a:b]
        randn[:, a * self.upp:b * self.upp] = self.randn[:, a * self.upp:b * self.upp]
        got = self.run(z, randn)
        assert np.abs(got - self.ref).max() > 0 or (a == 0 and b == T)      # the replacement did reach the output somewhere
        return float(np.abs(got - self.ref)[lo * self.upp:hi * self.upp].max())


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def case(request):
    tag, sr, voc, smallest = request.param
    return _Case(sr, voc), smallest


def test_margin_is_tight(case):
    c, smallest = case
    assert smallest <= c.margin <= smallest + 1, (c.margin, smallest)


def test_interior_window_is_exact(case):
    c, smallest = case
    assert c.outside_replaced(LO, HI, c.margin) == 0.0
    # the probe is sharp: one frame less than the smallest exact margin does reach the kept region
    assert c.outside_replaced(LO, HI, smallest - 1) > 0.0


def test_window_clipped_at_the_left_edge_is_exact(case):
    c, _ = case
    assert c.outside_replaced(3, 15, c.margin) == 0.0


def test_window_clipped_at_the_right_edge_is_exact(case):
    c, _ = case
    assert c.outside_replaced(T - 14, T, c.margin) == 0.0


def test_refinegan_is_reported_as_unsupported():
    from rvc_amd import _native
    assert _native.decoder_window_margin("RefineGAN", 48000) == -1


def test_window_entry_refuses_bad_arguments():
    import ctypes
    from rvc_amd import _native
    lib = _native._lib
    frames = ctypes.c_int()
    assert lib.rvc_decoder_window_margin(None, ctypes.byref(frames)) != 0
    cfg = _native._decoder_config("HiFi-GAN", 48000)
    cfg.kind = 7
    assert lib.rvc_decoder_window_margin(ctypes.byref(cfg), ctypes.byref(frames)) != 0
    assert b"unknown decoder kind" in lib.rvc_last_error()
    assert lib.rvc_decoder_forward_window(None, None, None, None, None, 1, 64, 26, 38, None, None, 0, None) != 0
    assert b"rvc_decoder_forward_window" in lib.rvc_last_error()
