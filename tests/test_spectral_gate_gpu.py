"""K18 (clean_audio, csrc/spectralgate.hip) on the GPU against the float64 SciPy restatement of tests/spectral_gate_ref.py.

Gate (per case): e_ref = max |r32 - r64|, the restatement on the float32 input against the restatement on the float64 input;
the device must satisfy max |dev - r64| <= 16 e_ref.  16 x because a 1024-term fp32 dot product grows rounding about
sqrt(1024) / log2(1024) ~ 3 x faster than the FFT, once forward and once inverse.  Each parity case first asserts that the
restatement changes the signal by more than 100 gates (RMS), so the comparison cannot pass vacuously.  Every figure is printed
before it is asserted (pytest -s shows them)."""
import threading
import wave

import numpy as np
import pytest
import torch

import spectral_gate_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEAMS = dict(chunk_size=4096, padding=2048)


@pytest.fixture(scope="module")
def NR():
    from rvc_amd.lib import noise_reduce
    return noise_reduce


def _refs(x64, sr, prop, **kw):
    r64 = R.reduce_noise(x64, sr, prop, **kw)
    r32 = R.reduce_noise(x64.astype(np.float32), sr, prop, **kw)
    return r64, float(np.abs(r32.astype(np.float64) - r64).max())


def _parity(NR, name, n, sr, prop, vacuity=True, floor=0.0, **kw):
    x64 = R.test_signal(n, sr)
    r64, e_ref = _refs(x64, sr, prop, **kw)
    gate = max(16 * e_ref, floor * float(np.abs(x64).max()))
    dev = NR.reduce_noise(x64.astype(np.float32), sr, prop, device=DEV, **kw)
    assert dev.dtype == np.float32 and dev.shape == (n,)
    err = float(np.abs(dev.astype(np.float64) - r64).max())
    print(f"[spectral gate] {name}: n={n} sr={sr} prop={prop} {kw or 'default chunks'}: rms(ref - in)={R.rms(r64 - x64):.4g} "
          f"e_ref={e_ref:.3g} gate={gate:.3g} max|dev - r64|={err:.3g} ({err / e_ref:.1f} e_ref)")
    if vacuity:
        assert R.rms(r64 - x64) > 100 * gate
    assert np.isfinite(dev).all()
    assert err <= gate, (name, err, gate)
    return dev


def test_single_chunk(NR):
    """n = 9000 at 48 kHz, default chunking: one buffer of 69 000 samples, 270 frames."""
    _parity(NR, "single chunk", 9000, 48000, 0.7)


def test_chunk_seams(NR):
    """the same input in 3 chunks of 4096 with 2048 of context, the last one 808 samples long"""
    _parity(NR, "chunk seams", 9000, 48000, 0.7, **SEAMS)


@pytest.mark.parametrize("n", [4096, 4097])
def test_chunk_boundary(NR, n):
    """exactly one chunk, and a second chunk of one sample"""
    _parity(NR, "chunk boundary", n, 48000, 0.7, **SEAMS)


@pytest.mark.parametrize("sr", [16000, 32000, 40000])
def test_filter_extents(NR, sr):
    """nf = 16 at 16 kHz reaches past bins 0 and 512 (nt = 3); 32 kHz: 17 x 13; 40 kHz: 13 x 15"""
    _parity(NR, "filter extents", 5000, sr, 0.7)


def test_prop_decrease_zero_returns_the_input_and_one_matches(NR):
    x64 = R.test_signal(9000, 48000)
    r64, e_ref = _refs(x64, 48000, 0.0)
    dev = NR.reduce_noise(x64.astype(np.float32), 48000, 0.0, device=DEV)
    err_ref, err_in = float(np.abs(dev - r64).max()), float(np.abs(dev - x64).max())
    print(f"[spectral gate] prop_decrease=0: e_ref={e_ref:.3g} gate={16 * e_ref:.3g} max|dev - r64|={err_ref:.3g} max|dev - in|={err_in:.3g}")
    assert np.abs(r64 - x64).max() <= 1e-12
    assert err_ref <= 16 * e_ref and err_in <= 16 * e_ref
    _parity(NR, "prop_decrease=1", 9000, 48000, 1.0)


# One sample makes e_ref degenerate: its spectrum is flat, SciPy's float32 transforms of it round next to nothing and e_ref is
# one rounding of ONE float32 number (1.25e-9 at |x| = 0.032), which measures no transform.  The gate of these two cases is
# therefore floored by the rounding model of the device's own arithmetic, not by e_ref alone: a sample is a chain of K = 1152
# fp32 multiply-adds whose terms sum, in magnitude, to at most max |x| (|S| <= max |x| for a signal shorter than the window,
# weights 2 / 1024 over 513 bins), so its rounding error is about sqrt(K) u max |x| with u = 2^-24 -- taken 4 x for the tail of the
# distribution.  (Higham's worst case, K u max |x|, is another 8 x wider.)
SHORT_FLOOR = 4 * np.sqrt(1152) * 2.0 ** -24


@pytest.mark.parametrize("n", [1, 255])
def test_signals_shorter_than_a_hop(NR, n):
    _parity(NR, "short", n, 48000, 0.7, vacuity=False, floor=SHORT_FLOOR)


def test_empty_signal(NR):
    out = NR.reduce_noise(np.zeros(0, dtype=np.float32), 48000, 0.7, device=DEV)
    assert out.dtype == np.float32 and out.shape == (0,)
    t = NR.reduce_noise(torch.zeros(0, device=DEV), 48000)
    assert t.shape == (0,) and t.device == torch.device(DEV)


def test_digital_silence_gives_exact_zeros(NR):
    """M == 0 in every bin: a finite mask and zero output, where noisereduce yields NaN"""
    out = NR.reduce_noise(np.zeros(3000, dtype=np.float32), 48000, 0.7, device=DEV)
    assert np.isfinite(out).all() and not out.any()
    x = R.test_signal(9000, 48000).astype(np.float32)
    x[2000:] = 0                                            # silence after a signal: the level decays, the output stays finite
    out = NR.reduce_noise(x, 48000, 1.0, device=DEV, **SEAMS)
    assert np.isfinite(out).all() and not out[8192:].any()  # the third chunk's buffer [6144, 11048) holds zeros only


def test_groups_of_chunks(NR):
    """More chunks than one launch group holds (8192 frames / 33 frames per chunk = 248): 249 chunks run as two groups, the last
    chunk 100 samples long.  Chunks are independent, so the restatement is evaluated on the chunks around the group seam and
    at both ends only."""
    n, sr = 248 * 4096 + 100, 48000
    x64 = R.test_signal(n, sr)
    dev = NR.reduce_noise(x64.astype(np.float32), sr, 0.7, device=DEV, **SEAMS)
    assert dev.shape == (n,) and np.isfinite(dev).all()
    for c in (0, 1, 246, 247, 248):
        s = c * 4096
        r64 = R.reduce_noise_chunk(x64, sr, 0.7, 4096, 2048, s)
        r32 = R.reduce_noise_chunk(x64.astype(np.float32), sr, 0.7, 4096, 2048, s)
        e_ref = float(np.abs(r32 - r64).max())
        err = float(np.abs(dev[s:s + 4096] - r64).max())
        print(f"[spectral gate] groups: chunk {c} ({len(r64)} samples): rms(ref - in)={R.rms(r64 - x64[s:s + 4096]):.4g} e_ref={e_ref:.3g} "
              f"max|dev - r64|={err:.3g} ({err / e_ref:.1f} e_ref)")
        assert R.rms(r64 - x64[s:s + 4096]) > 100 * 16 * e_ref
        assert err <= 16 * e_ref, (c, err, e_ref)


def test_input_kind_is_preserved(NR):
    x64 = R.test_signal(5000, 48000)
    a = NR.reduce_noise(x64.astype(np.float32), 48000, 0.7, device=DEV)
    b = NR.reduce_noise(x64, 48000, 0.7, device=DEV)                         # float64 accepted, rounded to float32 first
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype == np.float32
    assert np.array_equal(a, b)
    t = NR.reduce_noise(torch.from_numpy(x64.astype(np.float32)).to(DEV), 48000, 0.7)
    t64 = NR.reduce_noise(torch.from_numpy(x64).to(DEV), 48000, 0.7)
    for out in (t, t64):
        assert torch.is_tensor(out) and out.dtype == torch.float32 and out.device == torch.device(DEV) and out.shape == (5000,)
        assert np.array_equal(out.cpu().numpy(), a)
    with pytest.raises(ValueError, match="1-D"):
        NR.reduce_noise(torch.zeros(2, 64, device=DEV), 48000)


def test_two_calls_and_two_streams_give_identical_bits(NR):
    """no atomics, fixed summation orders, no per-call global state: a repeated call, and two host threads on two streams (the
    way convert_batch runs utterances), give the bits of the serial calls"""
    xs = [torch.from_numpy(R.test_signal(9000, 48000, seed=s).astype(np.float32)).to(DEV) for s in (1, 2)]
    kws = [{}, SEAMS]
    serial = [NR.reduce_noise(x, 48000, 0.7, **kw).cpu().numpy() for x, kw in zip(xs, kws)]
    again = [NR.reduce_noise(x, 48000, 0.7, **kw).cpu().numpy() for x, kw in zip(xs, kws)]
    assert all(np.array_equal(a, b) for a, b in zip(serial, again))
    assert not np.array_equal(serial[0], serial[1])
    results, errors = [None, None], []
    streams = [torch.cuda.Stream(DEV) for _ in xs]
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(DEV))

    def work(i):
        try:
            streams[i].wait_event(ready)
            with torch.cuda.stream(streams[i]):
                outs = [NR.reduce_noise(xs[i], 48000, 0.7, **kws[i]) for _ in range(4)]
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
    """The device / stream contract of rvc_amd._native for the new entry point (tests/test_native_call_path_gpu.py holds the
    table for the others): the forward call is noted, not made; it must see the tensor's device current and carry that device's
    current stream as its last argument."""
    from rvc_amd import _native as N
    real, calls = N._lib, []

    class Recorder:
        def __getattr__(self, name):
            if name == "rvc_spectral_gate_f32":
                return lambda *args: calls.append((torch.cuda.current_device(), args[-1])) or 0
            return getattr(real, name)
    monkeypatch.setattr(N, "_lib", Recorder())
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        N.spectral_gate(torch.empty(64, device=DEV), 48000, 0.5)
    N.spectral_gate(torch.empty(64, device=DEV), 48000, 0.5)
    assert calls == [(0, side.cuda_stream), (0, torch.cuda.current_stream(DEV).cuda_stream)]
    with pytest.raises(N.NativeError, match="HBM"):
        N.spectral_gate(torch.zeros(64), 48000, 0.5)
    assert len(calls) == 2


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _pcm(audio):
    return (np.clip(audio, -1.0, 1.0) * 32767.0).astype("<i2")


def _frames(path):
    with wave.open(path, "rb") as f:
        return f.getframerate(), np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def test_clean_audio_end_to_end(NR, tmp_path, monkeypatch):
    """The synthetic 40 kHz checkpoint of the convert_audio_batch test on a 1 s clip, noise_seed fixed.  The nets in front of the
    vocoder are not bit-stable from run to run (test_pipeline_gpu.py), so the uncleaned waveform of a conversion is taken from
    that same conversion -- a spy on the pipeline's return value, which convert_array hands on unchanged -- and the cleaned one
    must be reduce_noise of it bit for bit."""
    import os
    from rvc_amd.lib import synthetic as S
    from rvc_amd.infer.infer import VoiceConverter, _write_wav
    from rvc_amd.lib.audio import load_audio_infer
    monkeypatch.chdir(tmp_path)
    os.makedirs("rvc/models/embedders/contentvec"); os.makedirs("rvc/models/predictors")
    torch.save(S.make_hubert_state_dict(1), "rvc/models/embedders/contentvec/pytorch_model.bin")
    torch.save(S.make_rmvpe_state_dict(0), "rvc/models/predictors/rmvpe.pt")
    torch.save(S.make_synth_checkpoint(40000, "HiFi-GAN", seed=0, half=True), "model.pth")
    _write_wav("in.wav", S.synth_audio(16000, seed=5), 16000)
    vc = VoiceConverter(device=DEV)
    vc.convert_audio("in.wav", "plain.wav", "model.pth", "")                  # loads the model, the embedder and the predictor
    assert os.path.isfile("plain.wav") and vc.tgt_sr == 40000

    raw, cleaned_by = [], []
    pipeline, remove = vc.vc.pipeline, VoiceConverter.remove_audio_noise

    def spy(*args, **kw):
        raw.append(pipeline(*args, **{**kw, "noise_seed": 77}))
        return raw[-1]

    def spy_remove(data, sr, reduction_strength=0.7):
        cleaned_by.append((sr, reduction_strength))
        return remove(data, sr, reduction_strength)
    monkeypatch.setattr(vc.vc, "pipeline", spy)
    monkeypatch.setattr(VoiceConverter, "remove_audio_noise", staticmethod(spy_remove))
    a = load_audio_infer("in.wav", 16000, device=DEV)

    plain = vc.convert_array(a)
    assert np.array_equal(plain, raw[0]) and cleaned_by == []                  # clean_audio=False: unchanged, the gate never runs
    cleaned = vc.convert_array(a, clean_audio=True, clean_strength=0.5)
    assert cleaned_by == [(40000, 0.5)]
    assert cleaned.dtype == np.float32 and cleaned.shape == raw[1].shape
    assert np.array_equal(cleaned, NR.reduce_noise(raw[1], 40000, 0.5, device=DEV))
    change = R.rms(cleaned - raw[1])
    print(f"[spectral gate] end to end: {len(cleaned)} samples, rms(raw)={R.rms(raw[1]):.4g}, rms(cleaned - raw)={change:.4g}, "
          f"rms(run 2 - run 1)={R.rms(raw[1] - raw[0]):.3g}")
    assert change > 1e-4                                                       # it did something

    vc.convert_audio("in.wav", "clean.wav", "model.pth", "", clean_audio=True)  # clean_strength's default, 0.5
    assert cleaned_by[-1] == (40000, 0.5)
    sr, pcm = _frames("clean.wav")
    assert sr == 40000 and np.array_equal(pcm, _pcm(NR.reduce_noise(raw[2], 40000, 0.5, device=DEV)))
    assert not np.array_equal(pcm, _pcm(raw[2]))
    vc.convert_audio("in.wav", "plain2.wav", "model.pth", "", clean_audio=False)
    assert np.array_equal(_frames("plain2.wav")[1], _pcm(raw[3])) and len(cleaned_by) == 2
