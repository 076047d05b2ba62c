"""The opt-in fast-fp32 vocoder mode on the GPU: K3h (csrc/convbf1.hip, rvc_conv1d_f16x2_*: one square ResBlock conv with fp32 taps and
activations as error-corrected fp16 pairs, three matrix products per multiply-add) at kernel level against float64 and against the
exact bf16x3 Winograd form it replaces; the decoder handle with arithmetic="fp16x2" against the oracle and against the exact handle;
VoiceConverter.dec_arithmetic end to end.  Gates are the project's own for these layers (6e-5 at |y| ~ 1, 1.5 x the exact path's relative
RMS, 5e-5 decoder RMS against the oracle, 2e-6 between two kernel schedules of one decoder, 1e-5 between two pipeline runs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def conv1d_f64(x, w, b=None, padding=0, dilation=1):
    """F.conv1d in float64 as one float64 matrix product per tap on the device (test_kernels_gpu.py's reference); host tensor out."""
    dev0 = torch.device("cuda:0")
    xd, wd = x.to(dev0).double(), w.to(dev0).double()
    batch, _, length = xd.shape
    c_out, _, k = wd.shape
    xp = F.pad(xd, (padding, padding))
    l_out = length + 2 * padding - dilation * (k - 1)
    y = torch.zeros(batch, c_out, l_out, dtype=torch.float64, device=dev0)
    for t in range(k):
        y += torch.matmul(wd[:, :, t], xp[:, :, t * dilation: t * dilation + l_out])
    if b is not None:
        y += b.to(dev0).double()[None, :, None]
    return y.cpu()


def _rel(t, ref):
    return ((t.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,k,dil,length,batch", [
    (128, 7, 5, 31, 1),          # shorter than a tile
    (256, 11, 1, 64, 1),         # one tile
    (256, 7, 3, 1237, 2),        # ragged and batched
    (128, 11, 5, 777, 2),
    (128, 3, 1, 1001, 1),        # length not a multiple of 4: the element-wise load / store path
    (128, 11, 3, 20011, 1),      # 313 tiles: more than the CUs, the persistent loop
    (256, 3, 2, 333, 1), (256, 3, 4, 515, 2), (128, 7, 2, 200, 1), (256, 11, 4, 129, 1),   # the remaining (c, k) and dilations 2, 4
])
def test_conv1d_f16x2_matches_float64(native, dev, c, k, dil, length, batch):
    """K3h against F.conv1d in float64 on the UNROUNDED fp32 taps, with the fused activation, bias, residual, running sum and scale:
    max abs error <= 6e-5 at |y| ~ 1 (the gate of the exact kernels of these layers), also with res aliasing y (how the decoder
    calls it); relative RMS <= 1.5 x that of the exact bf16x3 Winograd form (conv1d_winobf_forward) on the same taps + 1e-8;
    two launches into never-written buffers, one NaN-filled, are bit-equal."""
    g = torch.Generator().manual_seed(c * 1000 + k * 10 + dil + 5)
    x = torch.randn(batch, c, length, generator=g)
    w = torch.randn(c, c, k, generator=g) / (c * k) ** 0.5
    b = torch.randn(c, generator=g)
    res = torch.randn(batch, c, length, generator=g)
    acc = torch.randn(batch, c, length, generator=g)
    pad = (k - 1) // 2 * dil
    conv = conv1d_f64(F.leaky_relu(x.double(), 0.1), w, b, padding=pad, dilation=dil)
    ref = (conv + res.double() + acc.double()) / 3
    u = native.conv1d_f16x2_pack_weight(w, dev)
    xd, bd = x.to(dev), b.to(dev)
    got = native.conv1d_f16x2_forward(xd, u, bd, k, dil, 0.1, res=res.to(dev), acc=acc.to(dev), out_scale=1 / 3).cpu()
    err = (got.double() - ref).abs().max().item()
    # plain conv: against the exact path and against torch's fp32 conv on the host
    ref2 = conv1d_f64(x, w, None, padding=pad, dilation=dil)
    plain = native.conv1d_f16x2_forward(xd, u, None, k, dil, 1.0).cpu()
    wino = native.conv1d_winobf_forward(xd, native.conv1d_winobf_pack_weight(w, dev), None, c, k, dil, 1.0).cpu()
    r1, rw, rt = _rel(plain, ref2), _rel(wino, ref2), _rel(F.conv1d(x, w, None, padding=pad, dilation=dil), ref2)
    print(f"C {c} k {k} d {dil} L {length} B {batch}: max abs err {err:.2e}; relative RMS vs float64: fp16 pairs {r1:.2e}, "
          f"bf16x3 Winograd {rw:.2e}, F.conv1d fp32 on the host {rt:.2e} (pairs / host {r1 / rt:.2f})")
    assert err <= 6e-5, err
    assert (plain.double() - ref2).abs().max().item() <= 6e-5
    assert r1 <= 1.5 * rw + 1e-8, (r1, rw)
    # res aliasing y
    y1 = res.to(dev).clone()
    native.conv1d_f16x2_forward(xd, u, bd, k, dil, 0.1, res=y1, out=y1)
    assert (y1.cpu().double() - (conv + res.double())).abs().max().item() <= 6e-5
    # reproducible: fresh buffers, one of them NaN-filled (nothing of y is read unless res / acc alias it)
    a1 = torch.empty_like(xd)
    a2 = torch.full_like(xd, float("nan"))
    native.conv1d_f16x2_forward(xd, u, bd, k, dil, 0.1, res=res.to(dev), out=a1)
    native.conv1d_f16x2_forward(xd, u, bd, k, dil, 0.1, res=res.to(dev), out=a2)
    assert torch.equal(a1, a2)


@pytest.fixture(scope="module")
def range_case():
    c, k, dil, length = 128, 7, 1, 1500
    g = torch.Generator().manual_seed(99)
    return c, k, dil, torch.randn(1, c, length, generator=g), torch.randn(c, c, k, generator=g) / (c * k) ** 0.5


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_conv1d_f16x2_activation_amplitude(native, dev, range_case, scale):
    """Activations of amplitude 1e-3 (the lo parts, and the smaller hi parts, are fp16 SUBNORMALS: flushed anywhere on the way they cost
    five orders of magnitude) and 1e3 meet the relative gate.  The split alone, simulated on the host with float32 accumulation, gives
    2.0e-7 and 2.1e-7 relative RMS on this shape."""
    c, k, dil, x, w = range_case
    xs = x * scale
    ref = conv1d_f64(xs, w, None, padding=(k - 1) // 2 * dil, dilation=dil)
    xd = xs.to(dev)
    got = native.conv1d_f16x2_forward(xd, native.conv1d_f16x2_pack_weight(w, dev), None, k, dil, 1.0).cpu()
    wino = native.conv1d_winobf_forward(xd, native.conv1d_winobf_pack_weight(w, dev), None, c, k, dil, 1.0).cpu()
    r1, rw = _rel(got, ref), _rel(wino, ref)
    print(f"amplitude {scale:g}: relative RMS vs float64: fp16 pairs {r1:.2e}, bf16x3 Winograd {rw:.2e}")
    assert r1 <= 1.5 * rw + 1e-8, (r1, rw)


def test_conv1d_f16x2_out_of_range_activations_stay_finite_and_local(native, dev, range_case):
    """A few samples of +-1e6 (beyond fp16): clamped to +-65504 before the split -- the output is finite everywhere and the columns
    outside those samples' receptive field are bit-equal to the run without them."""
    c, k, dil, x, w = range_case
    u = native.conv1d_f16x2_pack_weight(w, dev)
    spikes = [(0, 10, 1e6), (5, 11, -1e6), (127, 700, -1e6), (64, 1499, 1e6), (3, 0, 1e6)]
    xb = x.clone()
    for ch, t, v in spikes:
        xb[0, ch, t] = v
    clean = native.conv1d_f16x2_forward(x.to(dev), u, None, k, dil, 0.1).cpu()
    got = native.conv1d_f16x2_forward(xb.to(dev), u, None, k, dil, 0.1).cpu()
    assert torch.isfinite(got).all()
    touched = torch.zeros(x.shape[-1], dtype=torch.bool)
    h = (k - 1) // 2 * dil
    for _, t, _ in spikes:
        touched[max(0, t - h): t + h + 1] = True
    assert torch.equal(got[:, :, ~touched], clean[:, :, ~touched])
    assert not torch.equal(got[:, :, touched], clean[:, :, touched])
    # what the clamp documents: the result is the conv of the CLAMPED activation (+1e6 -> 65504, leaky(-1e6) = -1e5 -> -65504)
    xc = F.leaky_relu(xb.double(), 0.1).clamp(-65504.0, 65504.0)
    ref = conv1d_f64(xc, w, None, padding=h, dilation=dil)
    assert _rel(got, ref) <= 1e-6


def test_conv1d_f16x2_pack_refuses_taps_beyond_fp16(native, dev):
    w = torch.randn(128, 128, 3) * 0.05
    w[7, 9, 1] = 7e4
    with pytest.raises(native.NativeError, match="rvc_conv1d_f16x2_pack_weight"):
        native.conv1d_f16x2_pack_weight(w, dev)


# ---- decoder level --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voc", ["HiFi-GAN", "MRF HiFi-GAN", "RefineGAN"])
def test_decoder_fp16x2_matches_oracle_and_exact_handle(native, dev, ref_inputs, voc):
    """The synthetic 48 kHz checkpoint of test_decoder_matches_oracle at T = 64: the fast handle against the oracle (<= 5e-5 RMS, that
    test's gate) and against the exact handle on the same inputs (0 < rms <= 2e-6, test_resblock_pair_runtime_switch's gate for two
    kernel schedules of one decoder; exactly 0 would mean the mode changed nothing); an exact handle created after the fast one is
    bit-equal to the one created before."""
    from oracle import rvc_oracle as O
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    T, batch, sr = 64, 2, 48000
    cpt = S.make_synth_checkpoint(sr, voc, seed=0)
    w = O.fold_weight_norm(cpt["weight"])
    rates, ksizes = cpt["config"][12], cpt["config"][14]
    upp = int(np.prod(rates))
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(batch, 192, T, generator=gen)
    g = torch.randn(batch, 256, 1, generator=gen)
    f0 = torch.from_numpy(ref_inputs[2][:T]).float().unsqueeze(0).repeat(batch, 1)
    f0[1] = torch.roll(f0[1], 7) * 1.3
    dim = 9 if voc.startswith("MRF") else 1
    src_rand = torch.rand(batch, dim, generator=gen)
    src_randn = torch.randn(batch, T * upp, dim, generator=gen)
    refine = voc == "RefineGAN"
    adain = []
    if refine:
        length, ch = T, 512
        for r in rates:
            length, ch = length * r, ch // 2
            adain += [torch.randn(batch, ch, length, generator=gen) for _ in range(6)]
    outs = []
    for b in range(batch):
        if refine:
            noise = O.ListNoise([src_rand[b:b + 1].clone(), src_randn[b:b + 1]] + [a[b:b + 1] for a in adain])
            o = O.decoder_refine(w, z[b:b + 1], f0[b:b + 1], g[b:b + 1], rates, sr, noise)
        elif dim == 1:
            noise = O.ListNoise([torch.zeros(1, 1, 1), src_randn[b:b + 1]])
            o = O.decoder_nsf(w, z[b:b + 1], f0[b:b + 1], g[b:b + 1], rates, ksizes, sr, noise)
        else:
            noise = O.ListNoise([src_rand[b:b + 1].clone(), src_randn[b:b + 1]])
            o = O.decoder_mrf(w, z[b:b + 1], f0[b:b + 1], g[b:b + 1], rates, ksizes, sr, noise)
        outs.append(o)
    ref = torch.cat(outs, 0).numpy()

    folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
    adain_flat = torch.cat([a.reshape(-1) for a in adain]).to(dev) if refine else None
    args = (z.to(dev), f0.to(dev), g[:, :, 0].to(dev))
    kw = dict(src_randn=src_randn.to(dev), src_rand=src_rand.to(dev), adain_randn=adain_flat)
    kwd = dict(upsample_rates=rates, upsample_kernel_sizes=ksizes)
    exact = native.Decoder(voc, sr, folded, **kwd)
    assert exact.arithmetic == "exact"
    out_exact = exact.forward(*args, **kw).clone()
    fast = native.Decoder(voc, sr, folded, arithmetic="fp16x2", **kwd)
    assert fast.arithmetic == "fp16x2" and fast.upp == upp
    out_fast = fast.forward(*args, **kw).clone()
    assert torch.equal(fast.forward(*args, **kw), out_fast)                     # reproducible
    assert torch.equal(exact.forward(*args, **kw), out_exact)                   # the earlier handle keeps its kernels
    assert torch.equal(native.Decoder(voc, sr, folded, **kwd).forward(*args, **kw), out_exact)   # and so does a later exact one
    e_oracle, e_exact = rms(out_fast.cpu().numpy() - ref), rms((out_fast - out_exact).cpu().numpy())
    print(f"{voc}: fp16-pair handle vs oracle {e_oracle:.2e} (exact handle {rms(out_exact.cpu().numpy() - ref):.2e}), "
          f"vs exact handle {e_exact:.2e} (signal rms {rms(ref):.3f})")
    assert out_fast.shape == ref.shape and rms(ref) > 0.02
    assert e_oracle <= 5e-5, e_oracle
    assert 0.0 < e_exact <= 2e-6, e_exact


def test_decoder_fp16x2_refusals(native):
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0)
    folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
    with pytest.raises(native.NativeError, match="rvc_decoder_set_arithmetic.*weight_storage"):
        native.Decoder("HiFi-GAN", 48000, folded, weight_storage="bf16", arithmetic="fp16x2")
    with pytest.raises(native.NativeError, match="arithmetic"):
        native.Decoder("HiFi-GAN", 48000, folded, arithmetic="fp16")
    dec = native.Decoder("HiFi-GAN", 48000, folded)
    assert native._lib.rvc_decoder_set_arithmetic(dec._h, 1) != 0               # after finalize
    assert native._lib.rvc_last_error().startswith(b"rvc_decoder_set_arithmetic: decoder already finalized")


# ---- pipeline level -------------------------------------------------------------------------------------------------------------------
def test_pipeline_dec_arithmetic_fp16x2(native, dev):
    """A 2 s clip through VoiceConverter with dec_arithmetic = "fp16x2" against the default converter under the same noise_seed:
    0 < rms <= 1e-5, the project's run-to-run gate for equal schedules (the torch-driven nets in front of the vocoder are not bit-stable
    run to run, so no pipeline comparison here is bitwise).  The default converter is unchanged by the fast one having run: its
    waveform to that same gate, its vocoder handle -- HIP kernels only, deterministic -- bit for bit on fixed inputs.
    (~3.5 s warm; the first pipeline run of a process also pays the start-up of the libraries under the torch-driven nets, 4-5 s on an
    idle box, and this is the first pipeline test of a whole-suite run.)"""
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.hubert import HubertModelWithFinalProj
    hubert = HubertModelWithFinalProj(S.make_hubert_state_dict(1), device="cuda:0")
    # trained-like RMVPE + pitch embedding: runs are compared with each other (test_baseline_config2_properties says why)
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0, smooth_pitch=True)
    rm_sd = S.make_rmvpe_state_dict(0, peaked=True)
    big = S.synth_index(4096, seed=0)

    def converter(arithmetic):
        vc = VoiceConverter(device="cuda:0")
        assert vc.dec_arithmetic == "exact"
        if arithmetic is not None:
            vc.dec_arithmetic = arithmetic
        vc.load_checkpoint_dict(cpt)
        vc.hubert_model = hubert
        vc.vc.load_rmvpe_state_dict(rm_sd)
        vc.vc.set_index(big)
        return vc

    audio = S.synth_audio(32_000, seed=4)
    run = lambda vc: vc.vc.pipeline(hubert, vc.net_g, 0, audio.copy(), 0, "rmvpe", "", 0.75, True, 3, 1, "v2", 0.5, 128, False, 1, None,
                                    noise_seed=44)
    g = torch.Generator(device=dev).manual_seed(5)
    T = 100
    dargs = (torch.randn(1, 192, T, device=dev, generator=g), torch.full((1, T), 220.0, device=dev), torch.randn(1, 256, device=dev, generator=g))
    dkw = dict(src_randn=torch.randn(1, T * 480, 1, device=dev, generator=g), src_rand=torch.zeros(1, 1, device=dev))

    default = converter(None)
    assert default.net_g.dec_arithmetic == "exact" and default.net_g.dec.arithmetic == "exact"
    out_default = run(default)
    dec_default = default.net_g.dec.forward(*dargs, **dkw).clone()
    fast = converter("fp16x2")
    assert fast.net_g.dec_arithmetic == "fp16x2" and fast.net_g.dec.arithmetic == "fp16x2"
    out_fast = run(fast)
    dec_fast = fast.net_g.dec.forward(*dargs, **dkw).clone()
    again = run(default)
    e, e_again = rms(out_fast - out_default), rms(again - out_default)
    e_dec = rms((dec_fast - dec_default).cpu().numpy())
    print(f"pipeline fp16x2 vs default: rms {e:.2e}; default again: {e_again:.2e}; the two vocoder handles on fixed inputs: {e_dec:.2e} "
          f"(signal rms {rms(out_default):.3f})")
    assert out_fast.shape == out_default.shape and rms(out_default) > 0.01
    assert 0.0 < e <= 1e-5, e
    assert e_again <= 1e-5, e_again
    assert torch.equal(default.net_g.dec.forward(*dargs, **dkw), dec_default)
    assert 0.0 < e_dec <= 2e-6, e_dec                                           # the fast converter's handle does run other kernels

    fast.dec_weight_dtype = "bf16"                                              # the two options together: refused when the network is set up
    with pytest.raises(native.NativeError, match="rvc_decoder_set_arithmetic"):
        fast.load_checkpoint_dict(cpt)
