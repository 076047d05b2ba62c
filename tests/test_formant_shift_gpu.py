"""K19 (formant_shifting, csrc/formant.hip) on the GPU against the float64 restatement of tests/formant_shift_ref.py.

Gate (per case), K18's: e_ref = max |r32 - r64|, the restatement on the float32 input against the restatement on the float64
input; the device must satisfy max |dev - r64| <= 16 e_ref.  16 x because a 1024-term fp32 dot product grows rounding about
sqrt(1024) / log2(1024) ~ 3 x faster than the FFT, once forward and once inverse; the envelope chain between the transforms is
float64 on the device and adds nothing to it.  Each parity case with Q > 0 and d != 1 first asserts that the restatement differs
from its own d = 1 result by more than 100 gates (RMS), so the comparison cannot pass vacuously.  Every figure is printed before
it is asserted (pytest -s shows them).  All cases at 16 kHz."""
import functools
import threading

import numpy as np
import pytest
import torch

import formant_shift_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SR = 16000


@pytest.fixture(scope="module")
def FS():
    from rvc_amd.lib import formant_shift
    return formant_shift


def _ms(Q):
    """a quefrency in ms whose int(q * 1e-3 * 16000) is Q, away from the rounding edge"""
    return (Q + 0.5) / 16.0 if Q else 0.0


@functools.lru_cache(maxsize=None)
def _refs(n, Q, d, seed=1234):
    """-> (x64, r64, e_ref), computed once per case and shared; callers do not modify them"""
    x64 = R.test_signal(n, SR, seed)
    r64 = R.shift_formants(x64, SR, _ms(Q) * 1e-3, d)
    r32 = R.shift_formants(x64.astype(np.float32), SR, _ms(Q) * 1e-3, d)
    for a in (x64, r64):
        a.setflags(write=False)
    return x64, r64, float(np.abs(r32.astype(np.float64) - r64).max())


def _parity(FS, name, n, Q=12, d=0.8, **kw):
    x64, r64, e_ref = _refs(n, Q, d)
    assert int(_ms(Q) * 1e-3 * SR) == Q
    gate = 16 * e_ref
    dev = FS.shift_formants(x64.astype(np.float32), SR, _ms(Q), d, device=DEV, **kw)
    assert dev.dtype == np.float32 and dev.shape == (n,)
    err = float(np.abs(dev.astype(np.float64) - r64).max())
    moved = R.rms(r64 - _refs(n, Q, 1.0)[1]) if Q > 0 and d != 1 else None
    print(f"[formant shift] {name}: n={n} Q={Q} d={d} {kw or ''}: rms(ref)={R.rms(r64):.4g} rms(ref - ref(d=1))={moved} e_ref={e_ref:.3g} "
          f"gate={gate:.3g} max|dev - r64|={err:.3g} ({err / e_ref:.1f} e_ref)")
    if moved is not None:
        assert moved > 100 * gate
    assert np.isfinite(dev).all()
    assert err <= gate, (name, err, gate)
    return dev


def test_one_frame(FS):
    _parity(FS, "one frame", 1024)


def test_one_frame_and_a_dead_tail(FS):
    dev = _parity(FS, "dead tail", 1055)
    assert not dev[1024:].any() and dev[:1024].any()           # the 31 samples no frame covers are exactly 0


@pytest.mark.parametrize("n", [1056, 1253])
def test_two_and_eight_frames(FS, n):
    dev = _parity(FS, "few frames", n)
    last = (n - 1024) // 32 * 32 + 1024
    assert not dev[last:].any()


@pytest.mark.parametrize("d", [0.8, 1.4, 1.0])
def test_timbre(FS, d):
    _parity(FS, "timbre", 4000, 12, d)


@pytest.mark.parametrize("Q,d", [(1, 0.8), (128, 1.2), (511, 0.8)])
def test_quefrency(FS, Q, d):
    """Q = 1: the lifter keeps c[0] and c[1] once each; Q = 128: two partial sums per cepstral bin; Q = 511: the widest lifter, one
    sum per bin and two bins per lane"""
    _parity(FS, "quefrency", 4000, Q, d)


def test_quefrency_zero_is_the_round_trip(FS):
    dev0 = _parity(FS, "Q = 0", 4000, 0, 0.8)
    x64, r1, e1 = _refs(4000, 12, 1.0)
    err = float(np.abs(dev0.astype(np.float64) - r1).max())
    print(f"[formant shift] Q = 0 against the d = 1 reference: e_ref={e1:.3g} gate={16 * e1:.3g} max|dev - r64|={err:.3g}")
    assert err <= 16 * e1


def test_group_seam_is_invisible(FS):
    """134 frames as groups of 128 + 6: the second group's first 31 x 32 samples sum frames of both groups"""
    n = 1024 + 32 * (128 + 5)
    x = _refs(n, 12, 0.8)[0].astype(np.float32)
    whole = _parity(FS, "default group", n)
    split = _parity(FS, "group seam", n, group_frames=128)
    assert np.array_equal(split, whole)
    assert np.array_equal(FS.shift_formants(x, SR, _ms(12), 0.8, device=DEV, group_frames=128), split)
    assert np.array_equal(FS.shift_formants(x, SR, _ms(12), 0.8, device=DEV), whole)
    from rvc_amd import _native as N
    with pytest.raises(N.NativeError, match="group_frames"):
        FS.shift_formants(x, SR, _ms(12), 0.8, device=DEV, group_frames=100)


def test_digital_silence_gives_exact_zeros(FS):
    x = np.concatenate([R.test_signal(1500, SR), np.zeros(2500)]).astype(np.float32)
    for Q, d in ((12, 0.8), (12, 1.0), (0, 0.8)):
        out = FS.shift_formants(x, SR, _ms(Q), d, device=DEV)
        assert np.isfinite(out).all() and not out[2524:].any() and out[:2496].any()
    r64 = R.shift_formants(x.astype(np.float64), SR, _ms(12) * 1e-3, 0.8)     # x holds float32 values: both paths see the same input
    e_ref = float(np.abs(R.shift_formants(x, SR, _ms(12) * 1e-3, 0.8) - r64).max())
    err = float(np.abs(FS.shift_formants(x, SR, _ms(12), 0.8, device=DEV) - r64).max())
    print(f"[formant shift] signal then silence: e_ref={e_ref:.3g} gate={16 * e_ref:.3g} max|dev - r64|={err:.3g}")
    assert err <= 16 * e_ref                                                   # the live frames still match
    out = FS.shift_formants(np.zeros(3000, dtype=np.float32), SR, _ms(12), 0.8, device=DEV)
    assert np.isfinite(out).all() and not out.any()


def test_input_kind_is_preserved_on_a_side_stream(FS):
    x64 = _refs(4000, 12, 0.8)[0]
    a = FS.shift_formants(x64.astype(np.float32), SR, 0.8, 0.8, device=DEV)
    b = FS.shift_formants(np.array(x64), SR, 0.8, 0.8, device=DEV)            # float64 in: rounded to float32 first, float64 out
    assert a.dtype == np.float32 and b.dtype == np.float64 and np.array_equal(a.astype(np.float64), b)
    side = torch.cuda.Stream(DEV)
    x_dev = torch.from_numpy(x64.astype(np.float32)).to(DEV)
    x_dev64 = torch.from_numpy(np.array(x64)).to(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        t = FS.shift_formants(x_dev, SR, 0.8, 0.8)
        t64 = FS.shift_formants(x_dev64, SR, 0.8, 0.8)
    side.synchronize()
    assert torch.is_tensor(t) and t.dtype == torch.float32 and t.device == torch.device(DEV) and t.shape == (4000,)
    assert t64.dtype == torch.float64 and t64.device == torch.device(DEV)
    assert np.array_equal(t.cpu().numpy(), a) and np.array_equal(t64.cpu().numpy(), b)
    with pytest.raises(ValueError, match="1-D"):
        FS.shift_formants(torch.zeros(2, 2048, device=DEV))
    from rvc_amd import _native as N
    with pytest.raises(N.NativeError, match="shorter than one frame"):
        FS.shift_formants(torch.zeros(1023, device=DEV))


def test_two_threads_on_two_streams_equal_their_serial_results(FS):
    """no atomics, fixed summation orders, no per-call global state: two host threads on two streams (the way convert_batch runs
    utterances), one of them walking two groups, give the bits of the serial calls"""
    n = 1024 + 32 * (128 + 5)
    xs = [torch.from_numpy(R.test_signal(n, SR, seed=s).astype(np.float32)).to(DEV) for s in (1, 2)]
    kws = [dict(timbre=0.8), dict(timbre=1.4, group_frames=128)]
    serial = [FS.shift_formants(x, SR, 0.8, **kw).cpu().numpy() for x, kw in zip(xs, kws)]
    assert not np.array_equal(serial[0], serial[1])
    results, errors = [None, None], []
    streams = [torch.cuda.Stream(DEV) for _ in xs]
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(DEV))

    def work(i):
        try:
            streams[i].wait_event(ready)
            with torch.cuda.stream(streams[i]):
                outs = [FS.shift_formants(xs[i], SR, 0.8, **kws[i]) for _ in range(4)]
                streams[i].synchronize()
            results[i] = [o.cpu().numpy() for o in outs]
        except Exception as error:
            errors.append(error)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert all(np.array_equal(o, serial[i]) for o in results[i])


def test_binding_runs_on_the_tensor_device_and_current_stream(monkeypatch):
    """The device / stream contract of rvc_amd._native for the new entry point: the forward call is noted, not made; it must see
    the tensor's device current and carry that device's current stream as its last argument."""
    from rvc_amd import _native as N
    real, calls = N._lib, []

    class Recorder:
        def __getattr__(self, name):
            if name == "rvc_formant_shift_f32":
                return lambda *args: calls.append((torch.cuda.current_device(), args[-1])) or 0
            return getattr(real, name)
    monkeypatch.setattr(N, "_lib", Recorder())
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        N.formant_shift(torch.empty(2048, device=DEV), SR, 0.8e-3, 0.8)
    N.formant_shift(torch.empty(2048, device=DEV), SR, 0.8e-3, 0.8)
    assert calls == [(0, side.cuda_stream), (0, torch.cuda.current_stream(DEV).cuda_stream)]
    with pytest.raises(N.NativeError, match="HBM"):
        N.formant_shift(torch.zeros(2048), SR, 0.8e-3, 0.8)
    assert len(calls) == 2


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_formant_shifting_end_to_end(FS, tmp_path, monkeypatch):
    """The synthetic 40 kHz checkpoint on a 1 s clip, noise_seed fixed.  convert_array(x, formant_shifting=True) must be
    convert_array(shift_formants(x)): the 16 kHz signal the pipeline receives is compared bit for bit (a spy on its `audio`
    argument), and so are the outputs whenever the conversion in front of the vocoder repeats its own bits, which
    test_pipeline_gpu.py does not promise -- the repeated plain conversion in this test says which.  formant_shifting=False
    against no keyword at all: the same, and shift_formants never runs."""
    import os
    from rvc_amd.lib import synthetic as S
    from rvc_amd.infer import infer as I
    from rvc_amd.lib.audio import load_audio_infer
    monkeypatch.chdir(tmp_path)
    os.makedirs("rvc/models/embedders/contentvec"); os.makedirs("rvc/models/predictors")
    torch.save(S.make_hubert_state_dict(1), "rvc/models/embedders/contentvec/pytorch_model.bin")
    torch.save(S.make_rmvpe_state_dict(0), "rvc/models/predictors/rmvpe.pt")
    torch.save(S.make_synth_checkpoint(40000, "HiFi-GAN", seed=0, half=True), "model.pth")
    I._write_wav("in.wav", S.synth_audio(16000, seed=5), 16000)
    vc = I.VoiceConverter(device=DEV)
    vc.convert_audio("in.wav", "plain.wav", "model.pth", "")                  # loads the model, the embedder and the predictor
    assert os.path.isfile("plain.wav")

    fed, shifts = [], []
    pipeline, shift = vc.vc.pipeline, I.shift_formants

    def spy(*args, **kw):
        a = kw["audio"]
        fed.append(a.cpu().numpy().copy() if torch.is_tensor(a) else np.array(a))
        return pipeline(*args, **{**kw, "noise_seed": 77})

    def spy_shift(*args, **kw):
        shifts.append((args[1:], kw))
        return shift(*args, **kw)
    monkeypatch.setattr(vc.vc, "pipeline", spy)
    monkeypatch.setattr(I, "shift_formants", spy_shift)
    a = load_audio_infer("in.wav", 16000, device=DEV)

    def limited(v):                                                            # infer.py:262-265
        peak = np.abs(v).max() / 0.95
        return v / peak if peak > 1 else v

    plain = [vc.convert_array(a), vc.convert_array(a, formant_shifting=False, formant_qfrency=2.0, formant_timbre=1.3)]
    assert shifts == [] and np.array_equal(fed[0], fed[1]) and np.array_equal(fed[0], limited(a))
    stable = np.array_equal(plain[0], plain[1])
    shifted = vc.convert_array(a, formant_shifting=True)
    assert shifts == [((16000, 0.8, 0.8), dict(device=DEV))]
    by_hand = FS.shift_formants(a, 16000, 0.8, 0.8, device=DEV)
    composed = vc.convert_array(by_hand)
    assert len(shifts) == 1 and np.array_equal(fed[2], fed[3]) and np.array_equal(fed[2], limited(by_hand))
    change = R.rms(by_hand - a)
    print(f"[formant shift] end to end: {len(a)} samples in, {len(shifted)} out; rms(in)={R.rms(a):.4g} rms(shifted in - in)={change:.4g}; "
          f"plain conversion repeats its bits: {stable}; rms(out - composed)={R.rms(shifted - composed):.3g} "
          f"rms(plain run 2 - run 1)={R.rms(plain[1] - plain[0]):.3g}")
    assert change > 1e-3                                                       # it did something
    assert shifted.shape == composed.shape and shifted.dtype == composed.dtype == np.float32
    if stable:
        assert np.array_equal(shifted, composed)

    # the HBM-resident path of convert_batch: the shift runs on the utterance's stream and the pipeline is fed the same signal
    outs = vc.convert_batch([torch.from_numpy(a).to(DEV)], formant_shifting=True, formant_timbre=0.8)
    assert torch.is_tensor(outs[0]) and np.array_equal(fed[4], fed[2])
    # convert_audio hands its keywords to the loader, which shifts before the peak limiting
    vc.convert_audio("in.wav", "shifted.wav", "model.pth", "", formant_shifting=True, formant_qfrency=1.0, formant_timbre=1.2)
    assert os.path.isfile("shifted.wav") and np.array_equal(fed[5], limited(FS.shift_formants(a, 16000, 1.0, 1.2, device=DEV)))
