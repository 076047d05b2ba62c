"""K20 (the validation losses, csrc/valmetrics.hip) and rvc_amd.train.validate on the GPU against the float64 twin of
tests/validation_ref.py.

Gates.  The multi-resolution STFT loss: e_ref = the largest relative error of the torch-fp32 evaluation of the twin against its
float64 evaluation over the cases with n <= 4800; the device must stay within 16 e_ref (relative) on EVERY case, 48000 included:
16 x is K18's / K19's multiple for a chain of long fp32 dot products, the device's sums are float64, so its error should not grow
with the length as torch-fp32's does.  A maximum over cases because a single case's e_ref is a scalar that can come out
accidentally tiny.  SI-SDR: 16 x the largest absolute error in dB of the torch-fp32 evaluation over the cases, the same way.
Every parity case first asserts that the loss moves by more than 100 gates when the prediction is replaced by another seed's,
so no comparison can pass vacuously.  Every figure is printed before it is asserted (pytest -s shows them).  The raw kernel
calls write into guarded buffers with canaries on both sides."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import validation_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT64 = 0x7FF8DEADBEEF1234   # a NaN pattern no kernel writes
BAND = 512
STFT_CASES = (1025, 2048, 2049, 4800, 48000)
SDR_CASES = (2, 1023, 48000)


@pytest.fixture(scope="module")
def N():
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def M():
    from rvc_amd.lib import metrics
    return metrics


def _guarded64(n):
    buf = torch.empty(n + 2 * BAND, dtype=torch.int64, device=DEV)
    buf.fill_(SENT64)
    return buf[BAND: BAND + n].view(torch.float64), buf


def _intact(buf, n):
    return bool((buf[:BAND] == SENT64).all().item() and (buf[BAND + n:] == SENT64).all().item())


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _raw_stft_sums(N, x, y, resolutions=R.RESOLUTIONS, eps=1e-8):
    """rvc_mrstft_sums_f32 with a guarded output and a guarded workspace of exactly the size the query asks for -> [n_res, 4]"""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32), device=DEV)
    y = torch.as_tensor(np.asarray(y, dtype=np.float32), device=DEV)
    arrs = [_ints([r[i] for r in resolutions]) for i in range(3)]
    need = N._size("rvc_mrstft_sums_workspace_bytes", torch.device(DEV), x.numel(), *arrs, len(resolutions))
    assert need % 8 == 0
    out, obuf = _guarded64(4 * len(resolutions))
    ws, wbuf = _guarded64(need // 8)
    N._call("rvc_mrstft_sums_f32", torch.device(DEV), x.data_ptr(), y.data_ptr(), x.numel(), *arrs, len(resolutions), eps, out.data_ptr(),
            ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert _intact(obuf, out.numel()) and _intact(wbuf, ws.numel())
    assert not (out.view(torch.int64) == SENT64).any().item()
    return out.cpu().numpy().reshape(len(resolutions), 4)


def _loss(sums):
    return float(np.mean([math.sqrt(d2 / y2) + la / count for d2, y2, la, count in sums]))


@functools.lru_cache(maxsize=None)
def _stft_ref(n, seed=100):
    """-> (x64, y64, twin loss in float64, twin loss in torch-fp32, twin sums in float64); computed once, never modified"""
    x, y = R.glide_pair(n, seed + n)
    l64 = R.mrstft_loss(torch.from_numpy(x), torch.from_numpy(y))
    l32 = R.mrstft_loss(torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32)))
    return x, y, l64, l32, R.stft_sums(torch.from_numpy(x), torch.from_numpy(y))


@functools.lru_cache(maxsize=None)
def _stft_gate():
    e_ref = max(R.rel(_stft_ref(n)[3], _stft_ref(n)[2]) for n in STFT_CASES if n <= 4800)
    return e_ref, 16 * e_ref


@pytest.mark.parametrize("n", STFT_CASES)
def test_mrstft_against_twin(N, M, n):
    x, y, l64, l32, sums64 = _stft_ref(n)
    e_ref, gate = _stft_gate()
    other = _stft_ref(STFT_CASES[(STFT_CASES.index(n) + 1) % len(STFT_CASES)])[0]
    other = np.resize(other, n)
    moved = R.rel(R.mrstft_loss(torch.from_numpy(other), torch.from_numpy(y)), l64)
    sums = _raw_stft_sums(N, x, y)
    dev = _loss(sums)
    err = R.rel(dev, l64)
    worst = max(R.rel(sums[r][c], sums64[r][c]) for r in range(3) for c in range(3))
    print(f"[mrstft] n={n}: twin64={l64:.9g} torch32={l32:.9g} (rel {R.rel(l32, l64):.3g}) device={dev:.9g} rel err={err:.3g} "
          f"e_ref={e_ref:.3g} gate={gate:.3g} ({err / e_ref:.2f} e_ref); worst single sum rel err={worst:.3g}; "
          f"another seed's x moves the loss by {moved:.3g}")
    assert moved > 100 * gate
    for r, (n_fft, hop, _) in enumerate(R.RESOLUTIONS):
        assert sums[r][3] == (n_fft // 2 + 1) * (1 + n // hop) == sums64[r][3]
    assert math.isfinite(dev)
    assert err <= gate, (n, err, gate)
    via = M.multi_resolution_stft_loss(x, y, device=DEV)        # the public function: the same sums, the same bits
    assert via == M.multi_resolution_stft_loss(torch.from_numpy(x).to(DEV), torch.from_numpy(y).float().to(DEV))
    assert abs(via - dev) <= 4e-16 * abs(dev), (via, dev)


def test_mrstft_exact_cases(N):
    x, y = _stft_ref(4800)[:2]
    s = _raw_stft_sums(N, x, x)
    print(f"[mrstft] identical pair: {s.tolist()}")
    assert (s[:, 0] == 0).all() and (s[:, 2] == 0).all() and (s[:, 1] > 0).all()
    z = np.zeros(4800, dtype=np.float32)
    s = _raw_stft_sums(N, z, z)
    print(f"[mrstft] both silent: {s.tolist()}")
    assert (s[:, 0] == 0).all() and (s[:, 2] == 0).all() and np.isfinite(s).all()
    assert np.allclose(s[:, 1], s[:, 3] * 1e-8, rtol=1e-12) and _loss(s) == 0.0
    a, b = _raw_stft_sums(N, x, y), _raw_stft_sums(N, x, y)
    assert a.tobytes() == b.tobytes()
    for sub in ((1, 2), (2,), (0,), (2, 0)):
        part = _raw_stft_sums(N, x, y, tuple(R.RESOLUTIONS[i] for i in sub))
        assert part.tobytes() == a[list(sub)].tobytes(), sub


def test_mrstft_other_windows(N):
    """win == n_fft, an odd win, hop = 512 (the largest) and hop = 1; four resolutions in one call.  The gate is the same multiple
    of torch-fp32's own error, taken over the default resolutions' cases and this set's."""
    x, y = _stft_ref(2049)[:2]
    res = ((512, 128, 512), (1024, 512, 601), (2048, 512, 2048), (512, 1, 7))
    dev = _raw_stft_sums(N, x, y, res)
    ref = R.stft_sums(torch.from_numpy(x), torch.from_numpy(y), res)
    l64 = R.mrstft_loss(torch.from_numpy(x), torch.from_numpy(y), res)
    l32 = R.mrstft_loss(torch.from_numpy(x).float(), torch.from_numpy(y).float(), res)
    gate = 16 * max(_stft_gate()[0], R.rel(l32, l64))
    for r in range(4):
        errs = [R.rel(dev[r][c], ref[r][c]) for c in range(3)]
        print(f"[mrstft] {res[r]}: rel err of the three sums {errs}, count {dev[r][3]}")
        assert dev[r][3] == ref[r][3]
    err = R.rel(_loss(dev), l64)
    print(f"[mrstft] four resolutions: twin64={l64:.9g} torch32 rel={R.rel(l32, l64):.3g} device rel err={err:.3g} gate={gate:.3g}")
    assert abs(_loss(ref) - l64) <= 1e-12 * l64
    assert err <= gate


# ---- SI-SDR -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sdr_ref(n):
    x, y = R.glide_pair(n, 700 + n)
    if n == 2:
        # two centred samples are always colinear, so at full amplitude the value is the eps-limited ~145 dB, a difference of
        # nearly equal numbers in every arithmetic; at this amplitude sum t^2 is of the order of eps and the value is well conditioned
        x, y = x * 2e-4, y * 2e-4
    q = 2.0 ** 32 if n == 2 else 2.0 ** 20     # on a grid on which the scaled and shifted copy below is exact in fp32
    x, y = np.round(x * q) / q, np.round(y * q) / q
    v64 = R.si_sdr(torch.from_numpy(x), torch.from_numpy(y))
    v32 = R.si_sdr(torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32)))
    return x, y, v64, v32


@functools.lru_cache(maxsize=None)
def _sdr_gate():
    e_ref = max(abs(_sdr_ref(n)[3] - _sdr_ref(n)[2]) for n in SDR_CASES)
    return e_ref, 16 * e_ref


def _raw_si_sdr_sums(N, p, t):
    p = torch.as_tensor(np.asarray(p, dtype=np.float32), device=DEV)
    t = torch.as_tensor(np.asarray(t, dtype=np.float32), device=DEV)
    need = N._size("rvc_si_sdr_sums_workspace_bytes", torch.device(DEV), p.numel())
    out, obuf = _guarded64(5)
    ws, wbuf = _guarded64(need // 8)
    N._call("rvc_si_sdr_sums_f32", torch.device(DEV), p.data_ptr(), t.data_ptr(), p.numel(), out.data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert _intact(obuf, 5) and _intact(wbuf, ws.numel())
    return out.cpu().numpy()


@pytest.mark.parametrize("n", SDR_CASES)
def test_si_sdr_against_twin(N, M, n):
    x, y, v64, v32 = _sdr_ref(n)
    e_ref, gate = _sdr_gate()
    sums = _raw_si_sdr_sums(N, x, y)
    dev = M.si_sdr_from_sums(sums)
    other = R.si_sdr(torch.from_numpy(np.resize(_sdr_ref(48000 if n != 48000 else 1023)[0], n)), torch.from_numpy(y))
    dc = 2.0 ** -14 if n == 2 else 0.125
    xs, ys = 0.5 * x + dc, (y if n == 2 else 0.5 * y) - dc     # n = 2: eps is part of the value, which the target's scale then moves
    assert (xs.astype(np.float32) == xs).all() and (ys.astype(np.float32) == ys).all()
    shifted = M.si_sdr(xs.astype(np.float32), ys.astype(np.float32), device=DEV)
    print(f"[si-sdr] n={n}: twin64={v64:.9g} dB torch32={v32:.9g} dB device={dev:.9g} dB |err|={abs(dev - v64):.3g} e_ref={e_ref:.3g} "
          f"gate={gate:.3g}; target scaled and shifted: {shifted:.9g} dB; another prediction: {other:.6g} dB")
    if n > 2:      # with two samples the value depends on the target alone: (sum t^2 / eps)^2
        assert abs(other - v64) > 100 * gate
    assert abs(dev - v64) <= gate, (n, dev, v64, gate)
    assert abs(shifted - v64) <= gate
    assert M.si_sdr(x, y, device=DEV) == dev
    sums2 = _raw_si_sdr_sums(N, x, y)
    assert sums.tobytes() == sums2.tobytes()
    assert abs(sums[0] - x.sum()) <= 1e-9 * max(1.0, np.abs(x).sum()) and abs(sums[1] - y.sum()) <= 1e-9 * max(1.0, np.abs(y).sum())


def test_si_sdr_identical_pair_is_inf(M):
    x = _sdr_ref(48000)[0]
    assert M.si_sdr(x, x, device=DEV) == math.inf


# ---- mean absolute difference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,wa,wb", [(128, 301, 297), (80, 40, 64), (3, 1, 1), (125, 1, 9), (128, 2000, 2000)])
def test_mel_l1(N, M, rows, wa, wb):
    rng = np.random.default_rng(rows + wa)
    a = torch.from_numpy(rng.standard_normal((rows, wa)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.standard_normal((rows, wb)).astype(np.float32)).to(DEV)
    min_t = min(wa, wb)
    ref = R.mel_l1(a.double().cpu(), b.double().cpu())
    got = M.mel_l1(a, b)
    print(f"[mel l1] {rows} x ({wa}, {wb}): device={got:.12g} float64={ref:.12g}")
    assert abs(got - ref) <= 1e-13 * ref                     # float64 sums of exact float64 differences
    assert M.mel_l1(a.unsqueeze(0), b.cpu().numpy()) == got   # a batch of one, an array
    if min_t > 2:                                             # min_t smaller than both widths, on column slices: strides stay
        out, obuf = _guarded64(1)
        need = N._size("rvc_mean_abs_diff_workspace_bytes", torch.device(DEV), rows, min_t - 2)
        ws, wbuf = _guarded64(need // 8)
        N._call("rvc_mean_abs_diff_f32", torch.device(DEV), a.data_ptr(), wa, b.data_ptr(), wb, rows, min_t - 2, out.data_ptr(),
                ws.data_ptr(), need)
        torch.cuda.synchronize()
        assert _intact(obuf, 1) and _intact(wbuf, ws.numel())
        ref2 = float((a[:, :min_t - 2].double() - b[:, :min_t - 2].double()).abs().sum())
        assert abs(out.item() - ref2) <= 1e-13 * ref2
        ref3 = float((a[:, :min_t - 2].double() - b[:, 1:min_t - 1].double()).abs().mean())     # column slices: views, not copies
        assert abs(M.mel_l1(a[:, :min_t - 2], b[:, 1:]) - ref3) <= 1e-13 * ref3


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
SR = 48000


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """Three seeded items in an experiment folder as preprocess / extract leave it; item 0's WAV is 100 samples longer than its 60
    frames (features and spectrogram agree, so the loader cuts nothing and the wave outlasts y_hat), item 1 has fewer feature
    frames than spectrogram frames, item 2 more."""
    from scipy.io import wavfile
    from rvc_amd.lib import synthetic as S
    from rvc_amd.train.extract import preparing_files as PF
    exp = tmp_path_factory.mktemp("exp")
    for d in ("sliced_audios", "extracted", "f0", "f0_voiced"):
        os.makedirs(exp / d)
    frames = (60, 72, 66)            # spectrogram frames (hop 480): 0.6 .. 0.72 s, above the bucket rule's 50
    feats = (30, 35, 34)             # feature rows before the loader repeats them twice: 60, 70, 68
    for i, (t, f) in enumerate(zip(frames, feats)):
        name = f"0_{i}_0"
        audio = S.synth_audio(t * 480 + (100 if i == 0 else 0), seed=40 + i, sr=SR).astype(np.float32)
        wavfile.write(exp / "sliced_audios" / f"{name}.wav", SR, audio)
        rng = np.random.default_rng(90 + i)
        np.save(exp / "extracted" / f"{name}.npy", rng.standard_normal((f, 768)).astype(np.float32))
        f0 = 180.0 + 60.0 * np.sin(np.arange(2 * f) / 9.0 + i)
        f0[: 4] = 0.0
        mel = 1127.0 * np.log(1.0 + f0 / 700.0)
        lo, hi = 1127.0 * np.log(1 + 50 / 700), 1127.0 * np.log(1 + 1100 / 700)
        coarse = np.rint(np.clip((mel - lo) * 254 / (hi - lo) + 1, 1, 255)).astype(int)
        np.save(exp / "f0" / f"{name}.wav.npy", coarse)
        np.save(exp / "f0_voiced" / f"{name}.wav.npy", f0)
    PF.generate_config(SR, str(exp))
    PF.generate_filelist(str(exp), SR, include_mutes=0)
    return exp


def test_validation_loop_end_to_end(N, M, experiment):
    """validation_loop's per-item figures against the twin and against rvc_amd.lib.metrics called directly, both on the waveforms
    the loop itself scored (the torch-driven nets under infer are not bit-stable from call to call, see
    test_pipeline_gpu.py; how far a second inference with the same noise lands is printed, not asserted)."""
    from rvc_amd.infer.infer import VoiceConverter
    from rvc_amd.lib import synthetic as S
    from rvc_amd.train import validate as V
    from rvc_amd.train.data_utils import TextAudioLoaderMultiNSFsid
    from rvc_amd.train.mel_processing import mel_spectrogram_torch, spec_to_mel_torch
    hps = V.load_hparams(str(experiment))
    vc = VoiceConverter(DEV)
    vc.load_checkpoint_dict(S.make_synth_checkpoint(SR))
    ds = TextAudioLoaderMultiNSFsid(hps.data, device=DEV)
    assert len(ds) == 3 and ds.lengths == [os.path.getsize(p[0]) // 1440 for p in ds.audiopaths_and_text]
    assert sorted(V.bucket_order(ds.lengths)) == [0, 1, 2]
    items = [ds[i] for i in range(3)]
    assert not [f for f in os.listdir(experiment / "sliced_audios") if f.endswith(".spec.pt")]
    waves = []
    res = V.validation_loop(vc.net_g, items, DEV, hps, noise_seed=7, waveforms=waves)
    assert res["count"] == 3 and res["pesq"] is None and len(res["per_item"]) == 3 and len(waves) == 3
    for k in ("mel_l1", "mrstft", "si_sdr"):
        assert res[k] == sum(p[k] for p in res["per_item"]) / 3
    json.dumps(res)

    _, stft_gate = _stft_gate()
    _, sdr_gate = _sdr_gate()
    want_frames = {"0_0_0": 60, "0_1_0": 70, "0_2_0": 66}
    d = hps.data
    for pos, (item, y_hat) in enumerate(zip(items, waves)):
        spec, wav, phone, pitch, pitchf, sid = item
        name = os.path.basename(ds.audiopaths_and_text[pos][0])[:-4]
        frames = want_frames[name]
        assert phone.shape == (frames, 768) and spec.shape == (1025, frames)
        assert wav.shape == (1, frames * 480 + (100 if name == "0_0_0" else 0))
        assert pitch.shape == (frames,) and pitchf.shape == (frames,) and y_hat.shape == (frames * 480,)
        again = V.infer_item(vc.net_g, item, torch.device(DEV), V.item_noise(vc.net_g, frames, 7 + pos))
        repeat = float((again - y_hat).double().pow(2).mean().sqrt())
        y_hat_mel = mel_spectrogram_torch(y_hat.unsqueeze(0), d.filter_length, d.n_mel_channels, d.sample_rate, d.hop_length, d.win_length,
                                          d.mel_fmin, d.mel_fmax)[0]
        mel = spec_to_mel_torch(spec.unsqueeze(0), d.filter_length, d.n_mel_channels, d.sample_rate, d.mel_fmin, d.mel_fmax)[0]
        got = res["per_item"][pos]
        # train.py:1526-1541, restated here: the STFT loss over min(min_t hop, len(wave), len(y_hat)) samples, SI-SDR over the common ones
        min_t = min(y_hat_mel.shape[-1], mel.shape[-1])
        cut = min(min_t * 480, wav.shape[-1], y_hat.shape[-1])
        assert cut == frames * 480 and (name != "0_0_0" or cut < wav.shape[-1])
        wave = wav[0, :cut]
        direct = {"mel_l1": M.mel_l1(y_hat_mel, mel), "mrstft": M.multi_resolution_stft_loss(y_hat[:cut], wave), "si_sdr": M.si_sdr(y_hat[:cut], wave)}
        yh64, w64 = y_hat[:cut].double().cpu(), wave.double().cpu()
        twin = {"mel_l1": R.mel_l1(y_hat_mel.double().cpu(), mel.double().cpu()), "mrstft": R.mrstft_loss(yh64, w64), "si_sdr": R.si_sdr(yh64, w64)}
        print(f"[validate] {name}: loop={ {k: got[k] for k in direct} } twin={twin}; a second inference with the same noise differs by "
              f"{repeat:.3g} RMS ({'bit-identical' if torch.equal(again, y_hat) else 'not bit-identical'})")
        assert got["frames"] == frames and got["samples"] == frames * 480
        for k in direct:
            assert got[k] == direct[k], (name, k, got[k], direct[k])          # bit for bit
        assert abs(got["mel_l1"] - twin["mel_l1"]) <= 1e-13 * twin["mel_l1"]
        assert R.rel(got["mrstft"], twin["mrstft"]) <= stft_gate
        assert abs(got["si_sdr"] - twin["si_sdr"]) <= sdr_gate


def test_validate_cli_writes_json(experiment, tmp_path, capsys):
    from rvc_amd.lib import synthetic as S
    from rvc_amd.train import validate as V
    model = tmp_path / "model.pth"
    torch.save(S.make_synth_checkpoint(SR), model)
    assert V.main([str(experiment), str(model), "--all", "--dec-weight-dtype", "bf16"]) == 0
    out = capsys.readouterr().out
    printed = json.loads(out[out.index("{"):])
    on_disk = json.load(open(experiment / "validation.json"))
    assert printed == on_disk and on_disk["count"] == 3 and on_disk["dec_weight_dtype"] == "bf16" and on_disk["pesq"] is None
    assert sorted(on_disk["items"]) == [0, 1, 2] and on_disk["left_out"] == 0 and len(on_disk["per_item"]) == 3
    for k in ("mel_l1", "mrstft", "si_sdr"):
        assert on_disk[k] == sum(p[k] for p in on_disk["per_item"]) / 3
    with pytest.raises(FileNotFoundError, match="nothing.pth"):
        V.validate_checkpoint(str(experiment), str(tmp_path / "nothing.pth"), device=DEV)
    assert V.validate_checkpoint(str(experiment), str(model), device=DEV, seed=3)["count"] == 1     # 3 items: a hold-out of one
