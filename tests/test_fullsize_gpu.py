"""Full-length parity on the MI355X: the shapes bench.py times (BASELINE cfg 1 / cfg 2), the multi-segment path, the
vocoder at T = 3198 stage by stage, and the a18 caller -- each against the oracle run on the box's host cores under the
same seed (or against a reference-generated fixture).  Gate: 1e-3 waveform RMS (north_star); integers bit-exact.
The oracle runs take tens of seconds each; they are the price of not extrapolating parity from 3 s clips.  Since round 5
they run ONCE per (kind, case) in a host process pool that starts with the session (tests/_oracle_farm.py, conftest.py) and
works underneath the kernel tests; this file runs last and reads the results."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import load_golden, rms

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    from rvc_amd.lib import synthetic
    return synthetic


@pytest.fixture(scope="module")
def hubert(S):
    from rvc_amd.lib.hubert import HubertModelWithFinalProj
    return HubertModelWithFinalProj(S.make_hubert_state_dict(1), device=DEV)


@pytest.fixture(scope="module")
def sds(S):
    return S.make_hubert_state_dict(1), S.make_rmvpe_state_dict(0)


def _converter(S, sr, voc, hubert, config=None):
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.infer.pipeline import Pipeline
    vc = VoiceConverter(device=DEV)
    vc.load_checkpoint_dict(S.make_synth_checkpoint(sr, voc, seed=0))
    vc.hubert_model = hubert
    if config is not None:
        vc.vc = Pipeline(sr, config)
    vc.vc.load_rmvpe_state_dict(S.make_rmvpe_state_dict(0))
    return vc


from conftest import SAL_TIE, F0_NOISE, f0_tie_report as _f0_tie_report  # noqa: E402  (shared with test_pipeline_gpu.py)


def _run_pair(farm, key, vc, hubert, audio, rate, seed):
    """Product and oracle on one input under one seed; the oracle side is farm job `key` (tests/_oracle_farm.py: FLAT).  If
    their f0 contours differ (only on certified near-tie frames), the oracle is re-run on the product's contour so that the
    waveform comparison tests everything downstream of that decision at full length; the number of such frames is reported
    and bounded by the caller."""
    from oracle import rvc_oracle as O
    from _oracle_farm import FLAT
    res = farm.get(key)
    want, f0_o, sal_o = res["want"], res["f0_raw"], res["salience"]
    t_oracle = float(res["t_oracle"])
    vc.vc.debug_taps = {}
    got = vc.vc.pipeline(hubert, vc.net_g, 0, audio.copy(), 0, "rmvpe", "", rate, True, 3, 1, "v2", 0.5, 128, False, 1, None,
                         noise_seed=seed)
    f0_p = vc.vc.debug_taps["f0_raw"].cpu().numpy()
    sal_p = vc.vc.debug_taps["salience"].cpu().numpy()
    vc.vc.debug_taps = None
    differ = _f0_tie_report(f0_p, sal_p, f0_o, sal_o)
    plain_err = rms(got - want) if got.shape == want.shape else float("nan")
    # The coarse pitch (integer 1..255, the pitch-embedding index; pipeline.py:401-408) rounds a mel-scaled f0: contours equal
    # to fp noise can still land on either side of a .5 boundary.  One such frame changes the embedding of 10 ms of a 45 s
    # clip -- 1.3e-3 whole-clip RMS when it happens (seen on about one run in three of the 45 s case; the GPU contour itself
    # moves by ~1e-7 relative from run to run).  Each flip must be a certified rounding near-tie; the oracle then follows
    # the product's contour like for the arg-max ties.
    n_f = min(len(f0_p), len(f0_o))
    keep = np.ones(n_f, bool)
    keep[differ[differ < n_f]] = False
    c_p, c_o = O.f0_to_coarse(f0_p[:n_f].astype(np.float64))[0], O.f0_to_coarse(f0_o[:n_f].astype(np.float64))[0]
    flips = np.nonzero((c_p != c_o) & keep)[0]
    for t in flips:
        f = float(f0_o[t])
        mel = (1127 * np.log(1 + f / 700) - O.F0_MEL_MIN) * 254 / (O.F0_MEL_MAX - O.F0_MEL_MIN) + 1
        assert abs(abs(mel - np.floor(mel)) - 0.5) <= 2e-3 and abs(int(c_p[t]) - int(c_o[t])) == 1, (t, f, mel, c_p[t], c_o[t])
    # Even with NO differing frame the two contours are only equal to fp32 noise (<= F0_NOISE relative, asserted above), and
    # the NSF source integrates f0 into phase over the whole segment: a 2e-7 relative offset is 2 pi * 200 Hz * 45 s * 2e-7
    # = 0.011 rad at the end of a 45 s clip, i.e. ~1e-3 waveform RMS (measured 1.35e-3 at 45 s, 4e-4 at 30 s).  So when the
    # plain comparison is within a factor of a few of the gate, the oracle is re-run ON THE PRODUCT'S CONTOUR: the f0 stage
    # has been checked on its own just above, this checks everything downstream of it at full length.  The plain error is
    # reported; the UNCONDITIONAL plain gate is test_full_length_plain_peaked_rmvpe below (trained-like salience).
    if len(differ) or len(flips) or plain_err > 3e-4:
        farm.submit_pipeline(key + ":follow", False, FLAT[key.split(":")[1]], f0_override=f0_p)
        want = farm.get(key + ":follow")["want"]
    rel = np.abs(f0_p[:len(f0_o)] - f0_o) / np.maximum(f0_o, 1.0)
    rel[differ] = 0
    return got, want, dict(tie_frames=len(differ), coarse_flips=len(flips), n_frames=len(f0_p), plain_err=plain_err, t_oracle=t_oracle,
                           f0_rel_max=float(rel.max()), opt_ts=list(res["opt_ts"]))


@pytest.mark.parametrize("cfg", [2, 1])
def test_baseline_config_full_length_vs_oracle(S, hubert, oracle_farm, cfg):
    """cfg 2 exactly as bench.py runs it (30 s, 48 k NSF, 100 000-row index, index_rate 0.75) and cfg 1 (10 s, 40 k,
    index_rate 0): whole Pipeline.pipeline vs oracle.pipeline under one seed.  Reference: pipeline.py:509-694.

    The NSF source integrates f0 into phase (hifigan.py:172-177), so ONE frame whose salience arg-max falls on another
    peak shifts the phase of everything after it (measured: a single flipped frame at second 23 of 30 -> 3e-2 RMS on the
    last 7 s; identical contours -> 4e-7 over the whole clip, tools/diag_fullsize.py).  The comparison is therefore
    tie-aware exactly like the neighbour ids: contours must be equal to fp noise (2e-5 relative) except on frames
    certified as salience near-ties (_f0_tie_report), and the waveform gate is applied with the oracle following the
    product on those frames."""
    secs, sr, rows, rate = (30, 48000, 100_000, 0.75) if cfg == 2 else (10, 40000, 0, 0.0)
    vc = _converter(S, sr, "HiFi-GAN", hubert)
    big = S.synth_index(rows, seed=0) if rows else None
    if rows:
        vc.vc.set_index(big)
    audio = S.synth_audio(16000 * secs, seed=0)
    got, want, info = _run_pair(oracle_farm, f"flat:cfg{cfg}", vc, hubert, audio, rate, 1234)
    assert got.dtype == np.float32 and got.shape == want.shape == ((1_439_040,) if cfg == 2 else (399_200,))
    err = rms(got - want)
    print(f"cfg {cfg} full length: rms err {err:.3e} (oracle rms {rms(want):.3f}, oracle {info['t_oracle']:.0f} s); "
          f"f0: {info['tie_frames']} of {info['n_frames']} frames are certified salience near-ties, the rest agree to "
          f"{info['f0_rel_max']:.1e} relative, {info['coarse_flips']} coarse-bin rounding flips; waveform error before following "
          f"the product on those frames: {info['plain_err']:.3e}")
    assert err <= 1e-3, err
    assert info["tie_frames"] <= 0.002 * info["n_frames"], info   # a handful per 30 s at most
    assert info["coarse_flips"] <= 0.002 * info["n_frames"], info


@pytest.mark.parametrize("case", ["cfg2", "cfg1", "45s", "cfg4", "cfg5"])
def test_full_length_plain_peaked_rmvpe(S, hubert, oracle_farm, case):
    """The north_star gate with NOTHING conditional: product vs oracle at the benchmarked lengths, each side on its OWN
    f0 contour (no f0_override, no tie certificates on f0), waveform <= 1e-3 RMS, f0 <= 2e-5 relative on EVERY frame.

    What makes that possible is the RMVPE checkpoint, not the comparison: synthetic.make_rmvpe_state_dict(peaked=True)
    has a trained-like, unimodal salience (one bump of ~+-3 bins per frame, <= 2.5e-5 elsewhere -- verified with the
    reference's own RMVPE0Predictor on exactly these inputs, tests/golden/make_golden_peaked.py), so two fp32
    evaluations of the network can only disagree about which of two NEIGHBOURING bins of the same bump is the arg-max,
    and the +-4-bin local average (RMVPE.py:487-512) is continuous across that.  The flat-salience (random-head) tests
    above stay tie-aware.  The synthesizer checkpoint uses the smooth pitch embedding (synthetic: smooth_pitch=True): the
    coarse pitch (pipeline.py:401-408) rounds a continuous value, so two contours equal to 1e-6 still round apart at a
    .5 boundary on ~1 frame in 10^4; such frames must be certified rounding near-ties and are counted, every other
    coarse integer is bit-exact.

    cfg4 / cfg5 are BASELINE configs 4 and 5 at the length bench.py times them: the MRF vocoder with bf16 weight storage
    (oracle: fp32 math on the same bf16-valued weights) over the 100 k index, and RefineGAN over the 2 M-row index (drawn on
    the device as bench.py draws it; the oracle searches a host copy of the same rows)."""
    from oracle import rvc_oracle as O
    from _oracle_farm import PEAKED
    secs, sr, rows, rate, aseed, seed, voc, bf16 = PEAKED[case]
    rm_sd = S.make_rmvpe_state_dict(0, peaked=True)
    cpt = S.make_synth_checkpoint(sr, voc, seed=0, smooth_pitch=True)
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter(device=DEV)
    if bf16:
        vc.dec_weight_dtype = "bf16"
    vc.load_checkpoint_dict(cpt)
    vc.hubert_model = hubert
    vc.vc.load_rmvpe_state_dict(rm_sd)
    if rows > 200_000:           # the rows conftest drew on the device at session start; the farm worker searches the same file
        vc.vc.set_index(torch.from_numpy(np.load(oracle_farm.cfg5_index_file)).to(DEV))
    elif rows:
        vc.vc.set_index(S.synth_index(rows, seed=0))
    audio = S.synth_audio(16000 * secs, seed=aseed)
    res = oracle_farm.get("peaked:" + case)
    want, t_oracle = res["want"], float(res["t_oracle"])
    taps = {"f0_raw": res["f0_raw"], "salience": res["salience"], "opt_ts": list(res["opt_ts"])}
    vc.vc.debug_taps = {}
    got = vc.vc.pipeline(hubert, vc.net_g, 0, audio.copy(), 0, "rmvpe", "", rate, True, 3, 1, "v2", 0.5, 128, False, 1, None,
                         noise_seed=seed)
    f0_p = vc.vc.debug_taps["f0_raw"].cpu().numpy()
    sal_p = vc.vc.debug_taps["salience"].cpu().numpy()
    vc.vc.debug_taps = None
    f0_o, sal_o = taps["f0_raw"], taps["salience"]
    assert got.dtype == np.float32 and got.shape == want.shape and f0_p.shape == f0_o.shape
    if case == "45s":
        assert len(taps["opt_ts"]) == 1
    # the salience itself, and the bump property on the PRODUCT's side too
    sal_err = float(np.abs(sal_p - sal_o).max())
    am_p, am_o = sal_p.argmax(1), sal_o.argmax(1)
    assert np.abs(am_p - am_o).max() <= 1, "arg-max moved by more than one bin"
    off = sal_p.copy()
    for k in range(-4, 5):
        off[np.arange(len(am_p)), np.clip(am_p + k, 0, 359)] = 0
    assert sal_p.max(1).min() >= 0.4 and off.max() <= 1e-4
    # f0: every frame voiced, every frame within 2e-5 relative
    assert np.all(f0_o > 0) and np.all(f0_p > 0)
    f0_rel = float(np.abs(f0_p / f0_o - 1).max())
    # coarse pitch: bit-exact except certified rounding near-ties
    c_p, c_o = O.f0_to_coarse(f0_p.astype(np.float64))[0], O.f0_to_coarse(f0_o.astype(np.float64))[0]
    flips = np.nonzero(c_p != c_o)[0]
    for t in flips:
        mel = (1127 * np.log(1 + float(f0_o[t]) / 700) - O.F0_MEL_MIN) * 254 / (O.F0_MEL_MAX - O.F0_MEL_MIN) + 1
        assert abs(abs(mel - np.floor(mel)) - 0.5) <= 2e-3 and abs(int(c_p[t]) - int(c_o[t])) == 1, (t, f0_o[t], mel, c_p[t], c_o[t])
    err = rms(got - want)
    print(f"{case} plain (peaked RMVPE, no override): waveform rms err {err:.3e} (oracle rms {rms(want):.3f}, oracle {t_oracle:.0f} s); "
          f"{len(f0_p)} frames: f0 max relative difference {f0_rel:.2e}, salience max abs difference {sal_err:.2e}, "
          f"{int((am_p != am_o).sum())} arg-max moves to the neighbouring bin, {len(flips)} coarse-bin rounding near-ties")
    assert f0_rel <= 2e-5, f0_rel
    assert len(flips) <= 0.002 * len(f0_p), len(flips)
    assert err <= 1e-3, err


def test_multi_segment_matches_reference_golden(S, hubert):
    """pipeline.py:563-577, 614-681 on the product: split points, per-segment HuBERT + synthesis, RNG stream shared by the
    segments, crops, concat -- against the REFERENCE's own output (fixture of make_golden.py::multiseg, tier 1/3/4)."""
    g = load_golden("pipeline_multiseg")

    class Tier:
        x_pad, x_query, x_center, x_max, device = 1, int(g["x_query"]), int(g["x_center"]), int(g["x_max"]), DEV

    from conftest import vs_oracle
    vc = _converter(S, 48000, "HiFi-GAN", hubert, config=Tier())
    big = S.synth_index(4096, seed=0)
    vc.vc.set_index(big)
    # (reference mode of the tie-aware comparison: the product against the reference's output; only on a miss the oracle -- which must
    # then reproduce that output -- and the certified-near-tie treatment)
    out, _, err = vs_oracle(vc, hubert, S, S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0), g["audio"], seed=int(g["seed"]), sid=int(g["sid"]),
                            big=big, index_rate=float(g["index_rate"]), protect=float(g["protect"]), reference=g["out"], label="multi-segment",
                            oracle_kw=dict(x_query=int(g["x_query"]), x_center=int(g["x_center"]), x_max=int(g["x_max"])))
    assert out.dtype == np.float32 and out.shape == g["out"].shape
    print(f"multi-segment (3 segments) vs reference: rms err {err:.3e} (ref rms {rms(g['out']):.3f})")
    assert err <= 1e-3, err


def test_45s_two_segments_vs_oracle(S, hubert, oracle_farm):
    """> 41 s at the default tier: the host-filtfilt branch, two segments, waveform (not only lengths) vs the oracle
    (tie-aware in f0 like the full-length test above)."""
    vc = _converter(S, 48000, "HiFi-GAN", hubert)
    audio = S.synth_audio(16000 * 45, seed=45)
    got, want, info = _run_pair(oracle_farm, "flat:45s", vc, hubert, audio, 0.0, 99)
    assert len(info["opt_ts"]) == 1 and got.shape == want.shape == (int(load_golden("segmentation")["outlen_45"]),)
    err = rms(got - want)
    print(f"45 s, 2 segments: rms err {err:.3e} (oracle rms {rms(want):.3f}); f0 near-tie frames {info['tie_frames']} of "
          f"{info['n_frames']}, coarse-bin rounding flips {info['coarse_flips']}; before following the product on them: "
          f"{info['plain_err']:.3e}")
    assert err <= 1e-3, err
    assert info["tie_frames"] <= 0.002 * info["n_frames"], info
    assert info["coarse_flips"] <= 0.002 * info["n_frames"], info


@pytest.mark.parametrize("case", ["nsf-hint1", "nsf-hint2", "mrf", "mrf-bf16", "refine"])
def test_decoder_T3198_stage_by_stage_vs_oracle(S, oracle_farm, case):
    """Every vocoder at the benchmarked shape (T = 3198 -> 1 535 040 samples) with a tap on the source signal and after every
    stage: NSF under both tile selections of the short first stage (rvc_set_concurrency_hint 1: 128x64 tiles, 2: 128x128);
    MRF (BASELINE cfg 4) with fp32 and with bf16 weight storage -- its 9-harmonic source integrates 1.5 M phase increments
    with wrap compensation (hifigan_mrf.py:129-175), which the product evaluates in closed form per frame; RefineGAN
    (cfg 5) with its 24 AdaIN noise tensors drawn stage by stage from a seeded CPU generator (refinegan.py:220-263, 368-405).
    Reference: hifigan_nsf.py:173-207, hifigan_mrf.py:339-366, refinegan.py:368-405."""
    from oracle import rvc_oracle as O
    from rvc_amd import _native
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    from _oracle_farm import DECODER_T as T, SeededNoise, decoder_inputs
    voc = {"nsf": "HiFi-GAN", "mrf": "MRF HiFi-GAN", "refine": "RefineGAN"}[case.split("-")[0]]
    hint = 2 if case.endswith("hint2") else 1
    bf16 = case.endswith("bf16")
    cpt = S.make_synth_checkpoint(48000, voc, seed=0)
    w = O.fold_weight_norm(cpt["weight"])
    if bf16:   # what a bf16 copy of the vocoder holds; the oracle computes in fp32 on the same values
        w = {k: (v.float().bfloat16().float() if k.startswith("dec.") else v) for k, v in w.items()}
    rates, ksizes = cpt["config"][12], cpt["config"][14]
    upp = int(np.prod(rates))
    z, g, f0, gen = decoder_inputs()                       # the farm worker (tests/_oracle_farm.py::_decoder_job) draws the same
    if voc == "HiFi-GAN":
        src_rand = None
        src_randn = torch.randn(1, T * upp, 1, generator=gen)
        adain_dev = None
    elif voc == "MRF HiFi-GAN":
        rep = SeededNoise(23)
        src_rand, src_randn = rep.rand(1, 9), rep.randn(1, T * upp, 9)
        adain_dev = None
    else:
        rep = SeededNoise(23)
        src_rand, src_randn = rep.rand(1, 1), rep.randn(1, T * upp, 1)
        shapes, length, ch = [], T, 512
        for r in rates:
            length, ch = length * r, ch // 2
            shapes += [(1, ch, length)] * 6
        adain_dev = torch.empty(sum(int(np.prod(sh)) for sh in shapes), device=DEV)
        at = 0
        for sh in shapes:                                  # the same generator, tensor by tensor, straight into the flat device buffer
            n = int(np.prod(sh))
            adain_dev[at:at + n] = rep.randn(*sh).reshape(-1).to(DEV)
            at += n
    res = oracle_farm.get("decoder:" + case.replace("-hint1", "").replace("-hint2", ""))
    ref, t_oracle = res["ref"], float(res["t_oracle"])
    folded = {k[4:]: v for k, v in (w if bf16 else fold_weight_norm(cpt["weight"])).items() if k.startswith("dec.")}
    dec = _native.Decoder(voc, 48000, folded, upsample_rates=rates, upsample_kernel_sizes=ksizes, **({"weight_storage": "bf16"} if bf16 else {}))
    _native.set_concurrency_hint(hint)
    kw = dict(src_randn=src_randn.to(DEV), src_rand=src_rand.to(DEV) if src_rand is not None else None, adain_randn=adain_dev)
    try:
        chans, length = 512, T
        for stage in range(-1, len(rates)):
            if stage >= 0:
                chans, length = chans // 2, length * rates[stage]
            shape = (1, T * upp) if stage < 0 else (1, chans, length)
            tap = torch.zeros(shape, device=DEV)
            dec.set_tap(stage, tap)
            out = dec.forward(z.to(DEV), f0.to(DEV), g[:, :, 0].to(DEV), **kw)
            torch.cuda.synchronize()
            dec.set_tap(stage, None)
            want = res["har_source"].reshape(1, -1) if stage < 0 else res[f"stage{stage}"]
            e = rms(tap.cpu().numpy() - want)
            print(f"{case} stage {stage}: rms err {e:.3e} (oracle rms {rms(want):.3f})")
            assert e <= 1e-4 * max(1.0, rms(want)), (case, stage, e)
    finally:
        _native.set_concurrency_hint(1)
    err = rms(out.cpu().numpy() - ref)
    print(f"{case} waveform: rms err {err:.3e} (oracle rms {rms(ref):.3f}, oracle {t_oracle:.0f} s)")
    assert rms(ref) > 0.02
    assert err <= 5e-5, err


@pytest.mark.parametrize("cfg", [2, 4, 5])
def test_convert_batch_full_length_inflight3_equals_sequential(S, hubert, monkeypatch, cfg):
    """The benchmarked MODE at the benchmarked LENGTH, for every vocoder bench.py runs that way: four 30 s utterances through
    convert_batch with THREE in flight (bench.py's default since round 6; rounds 2-5: two) against the same four
    converted one at a time -- cfg 2 (48 k NSF vocoder), cfg 4 (MRF vocoder, bf16 weight storage: K3f with one-term taps next to K3y)
    and cfg 5 (RefineGAN: since round 6 its narrow (conv, conv) pairs run K3f too, so wino_conv_kernel -- the fp32 kernel that
    profiles/r05_mfma_cohabitation.txt shows returning wrong words next to a co-resident bf16-matrix workgroup -- is on no default path;
    the bf16 matrix kernels of all three utterances share the chip, kept apart only by their whole-CU LDS request), 100 k index,
    index_rate 0.75.  The synthesizer's random draws are zeroed (RefineGAN: its 24 AdaIN noise tensors too) so that both runs are
    deterministic; every kernel of one utterance then runs next to the other utterances' HuBERT / retrieval / vocoder kernels for
    the whole 30 s, which the 3-6 s clips of test_convert_batch_inflight_equals_sequential do not give.  Gate 1e-5: the library
    GEMMs are not bit-stable run to run."""
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.lib.algorithm.synthesizers import Synthesizer
    real_draw = Synthesizer._draw

    def zero_draw(self, noise, b, t, t_dec=None):
        return {k: (torch.zeros_like(v) if v is not None else None) for k, v in real_draw(self, noise, b, t, t_dec).items()}

    monkeypatch.setattr(Synthesizer, "_draw", zero_draw)
    vc = VoiceConverter(device=DEV)
    voc = {2: "HiFi-GAN", 4: "MRF HiFi-GAN", 5: "RefineGAN"}[cfg]
    if cfg == 4:
        vc.dec_weight_dtype = "bf16"
    vc.load_checkpoint_dict(S.make_synth_checkpoint(48000, voc, seed=0, smooth_pitch=True))
    vc.hubert_model = hubert
    vc.vc.load_rmvpe_state_dict(S.make_rmvpe_state_dict(0, peaked=True))
    vc.vc.set_index(S.synth_index(100_000, seed=0))
    audios = [torch.from_numpy(S.synth_audio(16000 * 30, seed=50 + i)).to(DEV) for i in range(4)]
    seq = [vc.convert_array(a, index_rate=0.75).clone() for a in audios]
    torch.cuda.synchronize()
    worst = 0.0
    for rep in range(2):
        par = vc.convert_batch(audios, inflight=3, index_rate=0.75)
        torch.cuda.synchronize()
        for a, b_ in zip(seq, par):
            assert a.shape == b_.shape == (1_439_040,)
            assert bool(torch.isfinite(b_).all())
            worst = max(worst, rms((a - b_).cpu().numpy()))
    print(f"cfg {cfg} ({voc}): 4 x 30 s, three in flight vs one at a time (zero noise): worst waveform rms difference {worst:.3e} (signal rms {rms(seq[0].cpu().numpy()):.3f})")
    assert rms(seq[0].cpu().numpy()) > 0.02
    assert worst <= 1e-5, worst


def test_convert_array_caller_vs_oracle(S, hubert, sds, tmp_path):
    """a18 (infer.py:262-311): the peak limit to 0.95 and the index-path normalisation ("trained" -> "added", quotes and
    blanks stripped) as VoiceConverter.convert_array applies them, against the oracle fed with the same front end."""
    from oracle import rvc_oracle as O
    # trained-like RMVPE + pitch embedding on both sides (the oracle is evaluated here, no fixture is involved): nothing tie-aware needed
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0, smooth_pitch=True)
    rm_peaked = S.make_rmvpe_state_dict(0, peaked=True)
    vc = _converter(S, 48000, "HiFi-GAN", hubert)
    vc.load_checkpoint_dict(cpt)
    vc.vc.load_rmvpe_state_dict(rm_peaked)
    big = S.synth_index(3000, seed=4)
    np.save(os.path.join(tmp_path, "added_IVF42_Flat.npy"), big)
    asked = '  "' + os.path.join(tmp_path, "trained_IVF42_Flat.npy") + '" \n'     # what a UI text box hands over
    audio = 4.0 * S.synth_audio(30_000, seed=8)                                   # peaks ~1.3: the limiter engages
    assert np.abs(audio).max() > 1.0
    limited = audio / (np.abs(audio).max() / 0.95)                                # infer.py:262-265
    torch.manual_seed(606)
    want = O.pipeline(sds[0], rm_peaked, cpt, limited.copy(), sid=0, pitch=0, big_npy=big, index_rate=0.6, protect=0.5)
    got = vc.convert_array(audio, index_path=asked, index_rate=0.6, protect=0.5, sid=0, noise_seed=606)
    assert got.shape == want.shape
    err = rms(got - want)
    print(f"convert_array (limiter + index path): rms err {err:.3e}")
    assert err <= 1e-3, err
    no_index = vc.convert_array(audio, index_path="", index_rate=0.6, protect=0.5, sid=0, noise_seed=606)
    assert rms(no_index - got) > 1e-3                                             # the index file really was found and used


def test_convert_array_split_audio_vs_oracle(S, hubert):
    """a18's split branch on the GPU (infer.py:283-318): the input is cut at its silences (process_audio), every chunk goes
    through Pipeline.pipeline on the device, merge_audio puts them back on the time line.  Expected value: the oracle run on
    the same chunks under the same seed, merged by the same host function (process_audio / merge_audio themselves are pinned
    to the reference on CPU, tests/test_host_logic_cpu.py).  Trained-like RMVPE / pitch embedding, so nothing is tie-aware."""
    from oracle import rvc_oracle as O
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.lib.tools.split_audio import merge_audio, process_audio
    rm_sd, hub_sd = S.make_rmvpe_state_dict(0, peaked=True), S.make_hubert_state_dict(1)
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0, smooth_pitch=True)
    vc = VoiceConverter(device=DEV)
    vc.load_checkpoint_dict(cpt)
    vc.hubert_model = hubert
    vc.vc.load_rmvpe_state_dict(rm_sd)
    gap = np.zeros(12000)
    audio = np.concatenate([np.zeros(3000), S.synth_audio(28000, seed=31), gap, S.synth_audio(36000, seed=32), gap,
                            S.synth_audio(24000, seed=33), np.zeros(5000)])
    chunks, intervals = process_audio(audio, 16000)
    assert len(chunks) == 3 and all(len(c) > 16000 for c in chunks), [len(c) for c in chunks]
    want_chunks = []
    for c in chunks:
        torch.manual_seed(808)
        want_chunks.append(O.pipeline(hub_sd, rm_sd, cpt, np.asarray(c, dtype=np.float64).copy(), sid=0, pitch=0, big_npy=None,
                                      index_rate=0.0, protect=0.5).astype(np.float32))
    want = merge_audio(chunks, want_chunks, intervals, 16000, 48000)
    got = vc.convert_array(audio, index_path="", index_rate=0.0, protect=0.5, sid=0, noise_seed=808, split_audio=True)
    assert got.shape == want.shape and got.dtype == np.float32
    assert 0 <= 3 * len(audio) - got.shape[0] <= 3 * 16000 * 0.5           # the 48 kHz time line of the input, minus its trailing silence
    err = rms(got - want)
    print(f"convert_array(split_audio=True), 3 chunks: rms err {err:.3e} (oracle rms {rms(want):.3f})")
    assert err <= 1e-3, err
    whole = vc.convert_array(audio, index_path="", index_rate=0.0, protect=0.5, sid=0, noise_seed=808, split_audio=False)
    assert whole.shape != got.shape or rms(whole - got) > 1e-3               # the split path really ran


def test_rccl_single_rank_broadcast_and_device_checksum():
    """The C-ABI RCCL path on one GPU: bind librccl at run time, ncclCommInitRank with one rank, broadcast in place,
    ncclCommCount == 1; rvc_checksum64 equals the documented formula evaluated in NumPy."""
    from rvc_amd import _native
    from rvc_amd.infer import distributed as D
    comm = _native.Comm(_native.comm_unique_id(), 1, 0)
    info = comm.info()
    print("rccl:", info)
    assert info["n_ranks"] == 1 and info["rank"] == 0 and info["rccl_version"] > 0 and "rccl" in info["library"]
    t = torch.randn(1000, 768, device=DEV)
    before = t.clone()
    comm.broadcast_(t, 0)
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    comm.destroy()
    for n in (1, 3, 1000 * 768, 7_654_321):
        x = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int64, device=DEV).to(torch.int32)
        assert D.tensor_checksum(x) == D.tensor_checksum(x.cpu()), n
    x = torch.arange(10, dtype=torch.uint8, device=DEV)                # 2 words + a 2-byte tail
    assert D.tensor_checksum(x) == D.tensor_checksum(x.cpu())
    # broadcast_index with force_rccl on one rank: the bench's N = 1 path
    idx = D.broadcast_index(np.ones((64, 768), dtype=np.float32), DEV, force_rccl=True)
    assert idx.shape == (64, 768) and D.last_broadcast_info()["n_ranks"] == 1
    D.destroy_native_comm()
