"""rvc_decoder_forward_window (Decoder.forward(keep=...)) against the same handle's full forward, sliced: same explicit noise, same
full-length inputs.  Gate: relative RMS <= 1e-5 (the project's gate for same-path comparisons) over the kept
region and, separately, over its first and its last frame -- where a short margin or a wrong carry offset would show first.

Measured on one MI355X (relative RMS, worst of kept region / first frame / last frame over the windows below): NSF 48k 1.0e-6,
NSF 32k 1.4e-6, MRF 48k 6.8e-7; a first or last frame that coincides with the signal's own end 0 to 3e-8.  The launchers pick tile
shapes by length, so the sums are reordered in the last bits; nothing larger.  (profiles/vocoder_window_ab.txt)"""
import numpy as np
import pytest
import torch

from conftest import rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = 1e-5
HANDLES = [("nsf48", 48000, "HiFi-GAN"), ("nsf32", 32000, "HiFi-GAN"), ("mrf48", 48000, "MRF HiFi-GAN")]
# (name, T, batch, keep_lo, keep_hi)
WINDOWS = [("interior", 64, 1, 26, 38),
           ("left-clipped", 64, 1, 3, 20),          # keep_lo below the margin: ext is clipped at frame 0
           ("to-the-end", 64, 1, 40, 64),           # keep_hi = T
           ("odd", 64, 1, 23, 36),                  # odd keep_lo, odd length: tiles and Winograd groups start elsewhere
           ("batch2", 64, 2, 26, 38),
           ("T67", 67, 1, 29, 48)]


class _Handle:
    def __init__(self, sr, voc):
        from rvc_amd import _native
        from rvc_amd.lib import synthetic as S
        from rvc_amd.lib.algorithm.weights import fold_weight_norm
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        cpt = S.make_synth_checkpoint(sr, voc, seed=0)
        rates, ksizes = cpt["config"][12], cpt["config"][14]
        folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
        self.dec = _native.Decoder(voc, sr, folded, upsample_rates=rates, upsample_kernel_sizes=ksizes)
        self.upp, self.dim = self.dec.upp, 9 if voc.startswith("MRF") else 1
        self._cache = {}

    def inputs(self, T, batch):
        """(args, noise kwargs, full forward) for (T, batch): computed once, shared by every window, never modified."""
        if (T, batch) not in self._cache:
            gen = torch.Generator().manual_seed(100 + T)
            z = torch.randn(2, 192, T, generator=gen)
            g = torch.randn(2, 256, generator=gen)
            f0 = 110.0 + 300.0 * torch.rand(2, T, generator=gen)     # varies frame by frame: the carry is a real running sum
            f0[0, 2:6] = 0.0                                          # unvoiced gaps BEFORE every window below ...
            f0[0, 15:19] = 0.0
            f0[1, 7:12] = 0.0
            f0[:, 31:33] = 0.0                                        # ... and one inside
            src_rand = torch.rand(2, self.dim, generator=gen)
            src_randn = torch.randn(2, T * self.upp, self.dim, generator=gen)
            args = tuple(t[:batch].contiguous().to(DEV) for t in (z, f0, g))
            kw = dict(src_randn=src_randn[:batch].contiguous().to(DEV), src_rand=src_rand[:batch].contiguous().to(DEV))
            full = self.dec.forward(*args, **kw)
            torch.cuda.synchronize()
            self._cache[(T, batch)] = (args, kw, full)
        return self._cache[(T, batch)]


@pytest.fixture(scope="module", params=HANDLES, ids=[h[0] for h in HANDLES])
def handle(request):
    tag, sr, voc = request.param
    return _Handle(sr, voc)


@pytest.mark.parametrize("name,T,batch,lo,hi", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_window_equals_full_forward_sliced(handle, name, T, batch, lo, hi):
    """Measured (relative RMS, kept / first frame / last frame): 5e-9 to 1.4e-6 over every case of every handle (interior, nsf48:
    9.8e-7 / 9.7e-7 / 9.2e-7; nsf32: 1.3e-6 / 1.2e-6 / 1.3e-6; mrf48: 6.5e-7 / 6.7e-7 / 6.6e-7), against the gate of 1e-5."""
    args, kw, full = handle.inputs(T, batch)
    upp = handle.upp
    got = handle.dec.forward(*args, **kw, keep=(lo, hi))
    torch.cuda.synchronize()
    assert got.shape == (batch, 1, (hi - lo) * upp)
    want = full[:, :, lo * upp:hi * upp].cpu().numpy().astype(np.float64)
    got = got.cpu().numpy().astype(np.float64)
    figures = []
    for part, sl in (("kept", slice(None)), ("first frame", slice(0, upp)), ("last frame", slice(-upp, None))):
        rel = rms(got[:, :, sl] - want[:, :, sl]) / rms(want[:, :, sl])
        figures.append(f"{part} {rel:.2e}")
    print(f"window {name} [{lo}, {hi}) of {T}, batch {batch}: relative RMS " + ", ".join(figures))
    for part, sl in (("kept", slice(None)), ("first frame", slice(0, upp)), ("last frame", slice(-upp, None))):
        assert rms(got[:, :, sl] - want[:, :, sl]) <= GATE * rms(want[:, :, sl]), (name, part)


def test_whole_range_is_the_full_forward_bit_for_bit(handle):
    args, kw, full = handle.inputs(64, 1)
    got = handle.dec.forward(*args, **kw, keep=(0, 64))
    assert torch.equal(got, full)


def test_bad_windows_and_a_set_tap_raise(handle):
    from rvc_amd import _native
    args, kw, full = handle.inputs(64, 1)
    for keep in ((-1, 10), (10, 10), (20, 10), (10, 65)):
        with pytest.raises(_native.NativeError, match="rvc_decoder_forward_window"):
            handle.dec.forward(*args, **kw, keep=keep)
    tap = torch.empty(64 * handle.upp, device=DEV)
    handle.dec.set_tap(-1, tap)
    try:
        with pytest.raises(_native.NativeError, match="debug tap"):
            handle.dec.forward(*args, **kw, keep=(26, 38))
    finally:
        handle.dec.set_tap(-1, None)
    assert torch.equal(handle.dec.forward(*args, **kw, keep=(0, 64)), full)      # the handle is as it was


def test_refinegan_handle_raises():
    from rvc_amd import _native
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    cpt = S.make_synth_checkpoint(48000, "RefineGAN", seed=0)
    folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
    dec = _native.Decoder("RefineGAN", 48000, folded, upsample_rates=cpt["config"][12], upsample_kernel_sizes=cpt["config"][14])
    assert dec.window_margin() == -1
    T = 16
    gen = torch.Generator().manual_seed(5)
    z, g, f0 = torch.randn(1, 192, T, generator=gen).to(DEV), torch.randn(1, 256, generator=gen).to(DEV), torch.full((1, T), 220.0).to(DEV)
    randn = torch.randn(1, T * dec.upp, 1, generator=gen).to(DEV)
    with pytest.raises(_native.NativeError, match="RefineGAN"):
        dec.forward(z, f0, g, src_randn=randn, src_rand=torch.zeros(1, 1, device=DEV), keep=(4, 12))


def test_pipeline_with_and_without_the_trimmed_pad():
    """A 2 s clip (400 padded frames) through VoiceConverter.convert_batch, one in flight, the device generator seeded alike:
    trim_vocoder_pad = True (the window entry) against False (the whole padded segment, then the slice)."""
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.hubert import HubertModelWithFinalProj
    vc = VoiceConverter(device=DEV)
    # trained-like RMVPE / pitch embedding: no salience near-ties that run-to-run GEMM noise could flip between the two runs
    vc.load_checkpoint_dict(S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0, smooth_pitch=True))
    vc.hubert_model = HubertModelWithFinalProj(S.make_hubert_state_dict(1), device=DEV)
    vc.vc.load_rmvpe_state_dict(S.make_rmvpe_state_dict(0, peaked=True))
    assert vc.trim_vocoder_pad is True
    audio = S.synth_audio(32000, seed=3)
    outs = {}
    for trim in (False, True):
        vc.trim_vocoder_pad = trim
        torch.cuda.manual_seed(77)
        (outs[trim],) = vc.convert_batch([audio], inflight=1, index_rate=0.0)
    assert outs[True].shape == outs[False].shape and outs[True].shape[0] > 90_000      # (398 frames of 480 samples less 2 x 48000)
    rel = rms(outs[True] - outs[False]) / rms(outs[False])
    print(f"pipeline, 2 s clip: relative RMS trimmed vs whole = {rel:.2e}")
    assert rel <= GATE
