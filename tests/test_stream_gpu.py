"""K21 (csrc/sola.hip) and the conversion stream on the MI355X against the float64 restatement of tests/sola_ref.py.

Gates.  Outside the crossfade `out` is a copy: bit-equal.  Inside, out = infer f + buf (1 - f) costs three fp32 roundings of values
no larger than max(|infer|, |buf|), 3 x 2^-24 of it; the gate is 8: 2^-21 max(|infer[offset + i]|, |buf[i]|) per sample.  The new buf
is a copy: bit-equal.  The offset of a planted lag must EQUAL it (tests/test_stream_cpu.py proves the margin above tau on the host);
an unplanted one is accepted iff its float64 score is within tau = 2 X 2^-24 ||buf||_2 of the maximum, and everything else is then
compared at the device's lag."""
import numpy as np
import pytest
import torch

import sola_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(infer, buf, fade, s, b):
    """One rvc_sola_f32 -> (out, the new buf, offset) on the host"""
    from rvc_amd import _native
    buf_dev = _dev(buf)
    out, offset = _native.sola(_dev(infer), buf_dev, _dev(fade), s, b)
    return out.cpu().numpy(), buf_dev.cpu().numpy(), int(offset.item())


def _compare(infer, buf, fade, s, b, out, new_buf, offset, planted=None):
    """The gates of this file's docstring; -> True when the offset needed the tie tolerance"""
    x = buf.shape[0]
    ref_out, ref_buf, best, sc = R.sola(infer, buf, fade, s, b)
    used_tau = False
    if planted is not None:
        assert offset == planted == best, (offset, planted, best)
    elif offset != best:
        assert 0 <= offset <= s and sc[offset] >= sc[best] - R.tau(buf), (offset, best, sc[offset], sc[best], R.tau(buf))
        ref_out, ref_buf, _, _ = R.sola(infer, buf, fade, s, b, offset=offset)
        used_tau = True
    assert out.dtype == np.float32 and out.shape == (b,) and new_buf.dtype == np.float32
    assert np.array_equal(out[x:], infer[offset + x:offset + b])                                  # copied samples: the same bits
    bound = 2.0 ** -21 * np.maximum(np.abs(infer[offset:offset + x]), np.abs(buf)).astype(np.float64)
    err = np.abs(out[:x].astype(np.float64) - ref_out[:x])
    assert np.all(err <= bound), (float(err.max()), int(np.argmax(err - bound)))
    assert np.array_equal(new_buf, ref_buf)
    return used_tau


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,s,b,lag,seed", R.PLANTED, ids=[f"X{c[0]}-S{c[1]}-B{c[2]}-lag{c[3]}" for c in R.PLANTED])
def test_sola_finds_a_planted_lag_and_matches_the_restatement(x, s, b, lag, seed):
    infer, buf = R.planted(x, s, b, lag, seed)
    fade = R.fade_in(x)
    out, new_buf, offset = _run(infer, buf, fade, s, b)
    _compare(infer, buf, fade, s, b, out, new_buf, offset, planted=lag)
    again = _run(infer, buf, fade, s, b)
    assert np.array_equal(out, again[0]) and np.array_equal(new_buf, again[1]) and offset == again[2]      # identical bits


def test_sola_unplanted_noise_is_tie_aware():
    x, s, b = 320, 320, 640
    fade, used = R.fade_in(x), 0
    for seed in range(8):
        infer, buf = R.test_signal(b + x + s, 20 + seed), R.test_signal(x, 40 + seed)
        out, new_buf, offset = _run(infer, buf, fade, s, b)
        used += _compare(infer, buf, fade, s, b, out, new_buf, offset)
    print(f"unplanted (320, 320, 640): {used} of 8 seeds needed the tie tolerance")


def test_sola_after_reset_fades_in_from_lag_zero():
    x, s, b = 320, 320, 640
    infer, fade = R.test_signal(b + x + s, 60), R.fade_in(x)
    out, new_buf, offset = _run(infer, np.zeros(x, np.float32), fade, s, b)
    assert offset == 0
    _compare(infer, np.zeros(x, np.float32), fade, s, b, out, new_buf, offset, planted=0)


def test_sola_leaves_its_inputs_and_neighbours_alone():
    """infer and fade_in unchanged; out and buf written only inside their lengths (guard samples on both sides)"""
    from rvc_amd import _native
    x, s, b, lag = 400, 400, 800, 399
    infer, buf = R.planted(x, s, b, lag, 61)
    fade = R.fade_in(x)
    infer_dev, fade_dev = _dev(infer), _dev(fade)
    arena = torch.full((x + 128,), 7.0, dtype=torch.float32, device=DEV)
    arena[64:64 + x] = _dev(buf)
    out, offset = _native.sola(infer_dev, arena[64:64 + x], fade_dev, s, b)
    assert int(offset.item()) == lag and out.shape == (b,)
    assert torch.equal(infer_dev, _dev(infer)) and torch.equal(fade_dev, _dev(fade))
    assert bool((arena[:64] == 7.0).all()) and bool((arena[64 + x:] == 7.0).all())
    assert np.array_equal(arena[64:64 + x].cpu().numpy(), infer[lag + b:lag + b + x])


@pytest.mark.parametrize("n_hist,n_block", [(0, 320), (160, 320), (480, 320), (480, 2500)])
def test_stream_window_rule(n_hist, n_block):
    from rvc_amd import _native
    x = R.test_signal(5 * n_block, 62)
    hist_ref = np.zeros(n_hist, np.float32)
    hist = _dev(hist_ref)
    for j in range(5):
        block = x[j * n_block:(j + 1) * n_block]
        want, hist_ref = R.window(hist_ref, block)
        window = _native.stream_window(hist, _dev(block))
        assert window.dtype == torch.float32 and np.array_equal(window.cpu().numpy(), want), j
        assert np.array_equal(hist.cpu().numpy(), hist_ref), j
        assert np.array_equal(want, np.concatenate([np.zeros(n_hist, np.float32), x])[j * n_block:(j + 1) * n_block + n_hist])


# ---- the stream, end to end ---------------------------------------------------------------------------------------------------------
STREAM = dict(block_ms=100, context_ms=500, crossfade_ms=20, search_ms=10)
PUSHES = 6


@pytest.fixture(scope="module")
def runs():
    """The synthetic 32 kHz NSF model; six pushes three times: NumPy blocks, NumPy blocks after reset(), device-tensor blocks on a
    second stream of the same converter."""
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.hubert import HubertModelWithFinalProj
    from rvc_amd.infer.infer import VoiceConverter
    vc = VoiceConverter(device=DEV)
    vc.load_checkpoint_dict(S.make_synth_checkpoint(32000, "HiFi-GAN", seed=0))
    vc.hubert_model = HubertModelWithFinalProj(S.make_hubert_state_dict(1), device=DEV)
    vc.vc.load_rmvpe_state_dict(S.make_rmvpe_state_dict(0))
    audio = R.test_signal(PUSHES * 1600, 63)
    blocks = [audio[j * 1600:(j + 1) * 1600] for j in range(PUSHES)]
    stream = vc.open_stream(noise_seed=7, **STREAM)
    stream.debug = True
    first = [stream.push(blk) for blk in blocks]
    log, final_buf = list(stream.debug_log), stream._buf.cpu().numpy()
    stream.reset()
    second = [stream.push(blk.astype(np.float64)) for blk in blocks]
    other = vc.open_stream(noise_seed=7, **STREAM)
    on_device = [other.push(_dev(blk)) for blk in blocks]
    assert len(vc._streams) == 2
    other.close()
    return dict(vc=vc, stream=stream, blocks=blocks, first=first, log=log, final_buf=final_buf, second=second, on_device=on_device)


def test_stream_outputs_are_finite_blocks(runs):
    stream = runs["stream"]
    assert (stream.sr, stream.block_samples, stream.block_out, stream.latency_ms) == (32000, 1600, 3200, 130)
    for out in runs["first"]:
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (3200,) and np.isfinite(out).all()
    assert max(float(np.abs(out).max()) for out in runs["first"]) > 1e-4            # the synthetic model is not silent
    for out in runs["on_device"]:
        assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == (3200,)


def test_stream_replays_through_the_restatement(runs):
    plan, log, used = runs["stream"].plan, runs["log"], 0
    fade = R.fade_in(plan.xfade)
    assert len(log) == PUSHES and not log[0]["buf"].any() and log[0]["offset"] == 0
    for j, entry in enumerate(log):
        assert entry["infer"].shape == (plan.n_infer,) and entry["infer"].dtype == np.float32
        new_buf = log[j + 1]["buf"] if j + 1 < PUSHES else runs["final_buf"]
        used += _compare(entry["infer"], entry["buf"], fade, plan.search, plan.block_out, runs["first"][j], new_buf, entry["offset"])
    print(f"stream: offsets {[e['offset'] for e in log]}, {used} of {PUSHES} pushes needed the tie tolerance")


def test_stream_runs_are_bit_identical(runs):
    """Three runs of the same six blocks under noise_seed=7 must give the same bits.

    Pipeline.pipeline asks MIOpen for deterministic solvers in seeded calls for this: without that, 2 of 18 runs of
    this file saw the pipeline's output for one window and seed move by ~4e-7 from call to call, in samples rvc_sola_f32 only copies."""
    for j, (a, b, c) in enumerate(zip(runs["first"], runs["second"], runs["on_device"])):
        c = c.cpu().numpy()
        print(f"push {j}: max |second - first| = {np.abs(b - a).max():.3e} ({int((a != b).sum())} samples), "
              f"max |device - first| = {np.abs(c - a).max():.3e} ({int((a != c).sum())} samples), peak {np.abs(a).max():.3e}")
    for a, b, c in zip(runs["first"], runs["second"], runs["on_device"]):
        assert np.array_equal(a, b)                                                # after reset(), float64 blocks
        assert np.array_equal(a, c.cpu().numpy())                                  # device tensors in, another stream object


def test_first_push_converts_what_convert_array_converts(runs):
    vc, plan = runs["vc"], runs["stream"].plan
    window = np.concatenate([np.zeros(plan.hist_samples, np.float32), runs["blocks"][0]])
    whole = vc.convert_array(_dev(window), noise_seed=7)
    assert whole.shape == (plan.pipeline_out,)
    assert np.array_equal(whole[-plan.n_infer:].cpu().numpy(), runs["log"][0]["infer"])


def test_a_second_model_is_refused_while_a_stream_is_open(runs):
    from rvc_amd.lib import synthetic as S
    vc = runs["vc"]
    assert vc._streams == {runs["stream"]}
    with pytest.raises(RuntimeError, match="open stream"):
        vc.load_checkpoint_dict(S.make_synth_checkpoint(40000, "HiFi-GAN", seed=0))
    assert vc.tgt_sr == 32000


def test_convert_audio_stream_times_every_push_with_events(runs, tmp_path):
    """A 16 kHz WAV of 4.5 blocks through the loaded model: five pushes, the output trimmed to the input's duration, and the file is
    what pushing the same blocks by hand gives (16-bit), since the file's stream starts from the same empty state"""
    import wave
    from rvc_amd.infer.infer import _write_wav
    vc = runs["vc"]
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    audio = np.concatenate(runs["blocks"])[:7200]
    _write_wav(src, audio, 16000)
    report = vc.convert_audio_stream(src, dst, noise_seed=7, **STREAM)
    assert report["blocks"] == 5 == len(report["push_ms"]) and report["block_ms"] == 100
    assert all(0.0 < ms < 5000.0 for ms in report["push_ms"]) and report["max_ms"] == max(report["push_ms"]) >= report["median_ms"] > 0.0
    assert vc._streams == {runs["stream"]}                                         # its own stream is closed again
    with wave.open(dst, "rb") as f:
        assert (f.getframerate(), f.getnchannels(), f.getnframes()) == (32000, 1, 14400)
        pcm = np.frombuffer(f.readframes(14400), dtype="<i2")
    assert np.abs(pcm).max() > 0
