"""Host-side checks of the checkpoint validator (K20 and rvc_amd.train.validate): what the native entry points refuse before any
device call, the file list, the hold-out split, the bucket rule, the loader's label handling, and the float64 twin itself.  No
GPU is needed."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import validation_ref as R


@pytest.fixture(scope="module")
def N():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


FAKE = 0x10000   # a non-null, aligned "device pointer": every refusal below comes before anything touches the device


def _mrstft(N, n, n_fft, hop, win, *, x=FAKE, y=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 30, eps=1e-8):
    rc = N._lib.rvc_mrstft_sums_f32(x, y, n, _ints(*n_fft), _ints(*hop), _ints(*win), len(n_fft), eps, out, ws, ws_bytes, None)
    return rc, N._lib.rvc_last_error().decode()


def test_mrstft_refusals(N):
    rc, msg = _mrstft(N, 512, [1024], [120], [600])
    assert rc != 0 and "must exceed n_fft / 2" in msg, msg
    rc, msg = _mrstft(N, 4800, [1024, 2048], [120, 240], [600, 1200], ws_bytes=0)
    assert rc != 0 and "workspace too small" in msg, msg                      # n = n_fft / 2 + 1 and above pass the length check
    rc, msg = _mrstft(N, 4800, [768], [120], [600])
    assert rc != 0 and "n_fft 768 is not built" in msg, msg
    rc, msg = _mrstft(N, 4800, [1024], [120], [1025])
    assert rc != 0 and "win 1025 must be in [1, n_fft = 1024]" in msg, msg
    rc, msg = _mrstft(N, 4800, [1024], [0], [600])
    assert rc != 0 and "hop 0 must be in [1, 512]" in msg, msg
    rc, msg = _mrstft(N, 4800, [1024], [120], [600], eps=0.0)
    assert rc != 0 and "eps" in msg, msg
    for kw in (dict(x=None), dict(y=None), dict(out=None), dict(ws=None)):
        rc, msg = _mrstft(N, 4800, [1024], [120], [600], **kw)
        assert rc != 0 and "null pointer" in msg, (kw, msg)
    for kw in (dict(x=FAKE + 2), dict(y=FAKE + 1), dict(out=FAKE + 4), dict(ws=FAKE + 4)):
        rc, msg = _mrstft(N, 4800, [1024], [120], [600], **kw)
        assert rc != 0 and "misaligned pointer" in msg, (kw, msg)
    rc = N._lib.rvc_mrstft_sums_f32(FAKE, FAKE, 4800, None, _ints(120), _ints(600), 1, 1e-8, FAKE, FAKE, 1 << 30, None)
    assert rc != 0 and b"null pointer" in N._lib.rvc_last_error()
    rc = N._lib.rvc_mrstft_sums_f32(FAKE, FAKE, 4800, _ints(1024), _ints(120), _ints(600), 5, 1e-8, FAKE, FAKE, 1 << 30, None)
    assert rc != 0 and b"n_res 5 must be in [1, 4]" in N._lib.rvc_last_error()


def test_mrstft_workspace_query_and_one_byte_short(N):
    need = ctypes.c_size_t()
    res = ([1024, 2048, 512], [120, 240, 50], [600, 1200, 240])
    assert N._lib.rvc_mrstft_sums_workspace_bytes(4800, _ints(*res[0]), _ints(*res[1]), _ints(*res[2]), 3, ctypes.byref(need)) == 0
    # frames 41, 21, 97 -> 2, 1, 4 tiles of 32 frames x 2, 4, 1 bin groups, 24 bytes each
    assert need.value == (2 * 2 + 1 * 4 + 4 * 1) * 24
    rc, msg = _mrstft(N, 4800, *res, ws_bytes=need.value - 1)
    assert rc != 0 and f"workspace too small ({need.value - 1} < {need.value})" in msg, msg
    assert N._lib.rvc_mrstft_sums_workspace_bytes(1024, _ints(2048), _ints(240), _ints(1200), 1, ctypes.byref(need)) != 0
    assert b"must exceed n_fft / 2" in N._lib.rvc_last_error()
    assert N._lib.rvc_mrstft_sums_workspace_bytes(4800, _ints(1024), _ints(120), _ints(600), 1, None) != 0


def test_si_sdr_and_mean_abs_diff_refusals(N):
    L = N._lib
    need = ctypes.c_size_t()
    assert L.rvc_si_sdr_sums_f32(FAKE, FAKE, 1, FAKE, FAKE, 1 << 20, None) != 0
    assert b"n = 1 must be at least 2" in L.rvc_last_error()
    assert L.rvc_si_sdr_sums_workspace_bytes(1, ctypes.byref(need)) != 0
    assert L.rvc_si_sdr_sums_workspace_bytes(48000, ctypes.byref(need)) == 0 and need.value == 188 * 24
    assert L.rvc_si_sdr_sums_f32(FAKE, FAKE, 48000, FAKE, FAKE, need.value - 1, None) != 0
    assert b"workspace too small" in L.rvc_last_error()
    assert L.rvc_si_sdr_sums_f32(FAKE, None, 48000, FAKE, FAKE, need.value, None) != 0
    assert b"null pointer" in L.rvc_last_error()
    assert L.rvc_si_sdr_sums_f32(FAKE, FAKE, 48000, FAKE + 4, FAKE, need.value, None) != 0
    assert b"misaligned pointer" in L.rvc_last_error()

    assert L.rvc_mean_abs_diff_workspace_bytes(128, 300, ctypes.byref(need)) == 0 and need.value == 150 * 8
    assert L.rvc_mean_abs_diff_f32(FAKE, 300, FAKE, 299, 128, 300, FAKE, FAKE, need.value, None) != 0
    assert b"row strides 300 and 299 must be at least min_t = 300" in L.rvc_last_error()
    assert L.rvc_mean_abs_diff_f32(FAKE, 300, FAKE, 300, 128, 0, FAKE, FAKE, need.value, None) != 0
    assert b"must be at least 1" in L.rvc_last_error()
    assert L.rvc_mean_abs_diff_f32(FAKE, 300, FAKE, 300, 128, 300, FAKE, FAKE, need.value - 1, None) != 0
    assert b"workspace too small" in L.rvc_last_error()
    assert L.rvc_mean_abs_diff_f32(None, 300, FAKE, 300, 128, 300, FAKE, FAKE, need.value, None) != 0
    assert b"null pointer" in L.rvc_last_error()


def test_unbuilt_auraloss_options_raise_by_name(N):
    from rvc_amd.lib import metrics
    x = np.zeros(4800, dtype=np.float32)
    for kw in (dict(w_lin_mag=1.0), dict(scale="mel"), dict(perceptual_weighting=True), dict(window="hamming_window")):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            metrics.multi_resolution_stft_loss(x, x, **kw)
    with pytest.raises(TypeError, match="bogus"):
        metrics.multi_resolution_stft_loss(x, x, bogus=1)


def test_si_sdr_from_sums_is_the_reference_expression(N):
    from rvc_amd.lib import metrics
    rng = np.random.default_rng(5)
    t = rng.standard_normal(4001)
    p = 0.7 * t + 0.1 * rng.standard_normal(4001) + 0.3
    pc, tc = p - p.mean(), t - t.mean()
    sums = [p.sum(), t.sum(), (pc * tc).sum(), (tc * tc).sum(), (pc * pc).sum()]
    assert abs(metrics.si_sdr_from_sums(sums) - R.si_sdr(p, t)) < 1e-9
    same = [t.sum(), t.sum(), (tc * tc).sum(), (tc * tc).sum(), (tc * tc).sum()]
    assert metrics.si_sdr_from_sums(same) == float("inf")


# ---- the file list ----------------------------------------------------------------------------------------------------------------
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_generate_filelist_and_config(N, tmp_path, monkeypatch):
    from rvc_amd.train.extract import preparing_files as PF
    exp = str(tmp_path / "exp")
    names = ["0_0_0", "0_0_1", "1_0_0", "1_1_0"]
    for name in names:
        _touch(os.path.join(exp, "sliced_audios", name + ".wav"))
        _touch(os.path.join(exp, "extracted", name + ".npy"))
        _touch(os.path.join(exp, "f0_voiced", name + ".wav.npy"))
        if name != "1_1_0":                                   # this one lacks its coarse f0 and must be dropped
            _touch(os.path.join(exp, "f0", name + ".wav.npy"))
    with open(os.path.join(exp, "model_info.json"), "w") as f:
        json.dump({"title": "kept"}, f)
    monkeypatch.chdir(tmp_path)
    PF.generate_filelist(exp, 48000, include_mutes=3)
    lines = open(os.path.join(exp, "filelist.txt")).read().split("\n")
    j = os.path.join
    want = [f"{j(exp, 'sliced_audios', n)}.wav|{j(exp, 'extracted', n)}.npy|{j(exp, 'f0', n)}.wav.npy|{j(exp, 'f0_voiced', n)}.wav.npy|{n[0]}"
            for n in names[:3]]
    mute = j(str(tmp_path), "logs", "mute")
    mute_line = f"{j(mute, 'sliced_audios', 'mute48000.wav')}|{j(mute, 'extracted', 'mute.npy')}|{j(mute, 'f0', 'mute.wav.npy')}|" \
                f"{j(mute, 'f0_voiced', 'mute.wav.npy')}|"
    want += [mute_line + s for s in "01"] * 3
    assert sorted(lines) == sorted(want)
    assert json.load(open(os.path.join(exp, "model_info.json"))) == {"title": "kept", "speakers_id": 2}

    PF.generate_filelist(exp, 40000, include_mutes=0, embedder_model="spin")
    assert sorted(open(os.path.join(exp, "filelist.txt")).read().split("\n")) == sorted(want[:3])

    PF.generate_config(48000, exp)
    cfg = json.load(open(os.path.join(exp, "config.json")))
    assert cfg["data"] == {"max_wav_value": 32768.0, "sample_rate": 48000, "filter_length": 2048, "hop_length": 480, "win_length": 2048,
                           "n_mel_channels": 128, "mel_fmin": 0.0, "mel_fmax": None}
    assert cfg["train"]["seed"] == 1234 and cfg["model"]["upsample_rates"] == [12, 10, 2, 2]
    PF.generate_config(32000, exp)                            # an existing config.json is left alone
    assert json.load(open(os.path.join(exp, "config.json"))) == cfg
    assert PF.training_config(32000)["data"]["n_mel_channels"] == 80 and PF.training_config(40000)["data"]["hop_length"] == 400
    with pytest.raises(ValueError, match="44100"):
        PF.training_config(44100)


# ---- split and buckets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 10, 101])
def test_holdout_is_random_splits_own(N, n):
    from rvc_amd.train import validate as V
    train_len = int(0.90 * n)
    _, val = torch.utils.data.random_split(list(range(n)), [train_len, n - train_len], generator=torch.Generator().manual_seed(1234))
    assert V.holdout_indices(n, 1234) == list(val.indices)
    assert len(V.holdout_indices(n, 1234)) == n - train_len
    assert V.holdout_indices(n, 1) != V.holdout_indices(n, 2) or n - train_len == 0


def test_bucket_rule(N):
    from rvc_amd.train import validate as V
    lengths = [50, 51, 900, 901, 100, 101, 0, 240, 480, 100000, 300]
    # left out: 50 (not above the first boundary), 901 and 100000 (above the last), 0
    assert V.bucket_order(lengths) == [1, 4, 5, 7, 10, 8, 2]
    assert V.bucket_order([]) == [] and V.bucket_order([10, 20]) == []


# ---- the loader's host side ---------------------------------------------------------------------------------------------------------
def test_get_labels_and_length_reconciliation(N, tmp_path):
    from rvc_amd.train import data_utils as D
    ds = D.TextAudioLoaderMultiNSFsid.__new__(D.TextAudioLoaderMultiNSFsid)
    ds.hop_length = 480
    for frames in (7, 500):
        feats = np.arange(frames * 4, dtype=np.float32).reshape(frames, 4)
        np.save(tmp_path / "p.npy", feats)
        np.save(tmp_path / "c.npy", np.arange(2 * frames + 3) % 255 + 1)
        np.save(tmp_path / "f.npy", np.linspace(100, 200, 2 * frames + 3))
        phone, pitch, pitchf = ds.get_labels(str(tmp_path / "p.npy"), str(tmp_path / "c.npy"), str(tmp_path / "f.npy"))
        n = min(2 * frames, 900)
        assert phone.dtype == torch.float32 and pitch.dtype == torch.int64 and pitchf.dtype == torch.float32
        assert phone.shape == (n, 4) and pitch.shape == (n,) and pitchf.shape == (n,)
        assert torch.equal(phone, torch.from_numpy(feats[np.arange(n) // 2]))
        assert torch.equal(pitch, torch.from_numpy((np.arange(n) % 255 + 1)))
    with pytest.raises(FileNotFoundError, match="missing.npy"):
        ds.get_labels(str(tmp_path / "missing.npy"), str(tmp_path / "c.npy"), str(tmp_path / "f.npy"))
    with pytest.raises(FileNotFoundError, match="nowhere.wav"):
        ds.get_audio(str(tmp_path / "nowhere.wav"))

    spec, wav = torch.arange(3 * 12.0).reshape(3, 12), torch.arange(12 * 480 + 100.0).reshape(1, -1)
    phone, pitch, pitchf = torch.ones(10, 4), torch.arange(10), torch.arange(10.0)
    s, w, ph, pi, pf = D.reconcile_lengths(spec, wav, phone, pitch, pitchf, 480)          # features shorter
    assert s.shape == (3, 10) and w.shape == (1, 4800) and ph.shape == (10, 4) and pi.shape == (10,) and pf.shape == (10,)
    assert torch.equal(s, spec[:, :10]) and torch.equal(w, wav[:, :4800])
    s, w, ph, pi, pf = D.reconcile_lengths(spec[:, :8], wav, phone, pitch, pitchf, 480)   # spectrogram shorter
    assert s.shape == (3, 8) and w.shape == (1, 3840) and ph.shape == (8, 4) and pi.shape == (8,) and pf.shape == (8,)
    s, w, ph, pi, pf = D.reconcile_lengths(spec[:, :10], wav, phone, pitch, pitchf, 480)  # equal: nothing is cut, not even the wave
    assert s.shape == (3, 10) and w.shape == wav.shape and ph.shape == (10, 4)


def test_filter_names_a_missing_wav(N, tmp_path):
    from rvc_amd.train import data_utils as D
    (tmp_path / "filelist.txt").write_text(f"{tmp_path}/gone.wav|a.npy|b.npy|c.npy|0")
    hp = D.hparams_from_dict(dict(training_files=str(tmp_path / "filelist.txt"), max_wav_value=32768.0, sample_rate=48000,
                                  filter_length=2048, hop_length=480, win_length=2048))
    with pytest.raises(FileNotFoundError, match="gone.wav"):
        D.TextAudioLoaderMultiNSFsid(hp)


# ---- the twin -----------------------------------------------------------------------------------------------------------------------
def test_twin_si_sdr_is_the_direct_evaluation():
    rng = np.random.default_rng(9)
    t = rng.standard_normal(3000)
    p = 0.5 * t + 0.2 * rng.standard_normal(3000) - 0.1
    pc, tc = p - p.mean(), t - t.mean()
    s = (pc * tc).sum() / ((tc ** 2).sum() + 1e-8)
    direct = 10 * np.log10(((s * tc) ** 2).sum() / ((pc - s * tc) ** 2).sum() + 1e-8)
    assert abs(R.si_sdr(p, t) - direct) < 1e-10
    # the target's scale and DC do not matter; neither does the prediction's DC
    assert abs(R.si_sdr(p, 3.7 * t + 0.25) - direct) < 1e-8
    assert abs(R.si_sdr(p + 0.4, t) - direct) < 1e-8


def test_twin_stft_sums_and_terms_agree():
    x, y = R.glide_pair(4800, 3)
    sums, terms = R.stft_sums(x, y), R.stft_terms(x, y)
    for (d2, y2, la, count), (sc, lm), (n_fft, hop, _) in zip(sums, terms, R.RESOLUTIONS):
        assert count == (n_fft // 2 + 1) * (1 + 4800 // hop)
        assert abs(np.sqrt(d2 / y2) - sc) < 1e-12 * sc and abs(la / count - lm) < 1e-12 * lm
    assert R.mrstft_loss(x, x) == 0.0
    z = np.zeros(4800)
    assert R.mrstft_loss(z, z) == 0.0


def test_validate_checkpoint_has_no_cpu_fallback(N, tmp_path):
    from rvc_amd.train import validate as V
    with pytest.raises(N.NativeError):
        V.validate_checkpoint(str(tmp_path), str(tmp_path / "model.pth"), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(N.NativeError):
            V.validate_checkpoint(str(tmp_path), str(tmp_path / "model.pth"))
        with pytest.raises(N.NativeError):
            from rvc_amd.lib import metrics
            metrics.si_sdr(torch.zeros(8), torch.ones(8), device="cpu")
    with pytest.raises(N.NativeError):
        V.validation_loop(None, [], "cpu", None)
