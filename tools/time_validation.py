"""The validation losses (K20, csrc/valmetrics.hip) on a 3.6 s item at 48 kHz -- 172 800 samples, the longest the loader admits --
device tensors in, float64 sums on the device out: HIP events around 100 back-to-back calls, median of 20 such windows after 5
warm-up calls, ALTERNATED window by window with the PyTorch-ROCm evaluation of the same expressions (torch.stft and friends, fp32,
results left on the device as well).  Then the parity of both against the float64 twin at this size, and a 50-item
validation_loop over 3.6 s items with its share per stage.  DESIGN.md K20.
    python tools/time_validation.py [--no-loop]
Per-kernel times: rocprofv3 --kernel-trace --stats -- python tools/time_validation.py --calls-only"""
import os
import sys
import tempfile

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "codename-rvc-fork-3_amd"), os.path.join(ROOT, "tests")]
import torch
import validation_ref as R
from rvc_amd import _native
from rvc_amd.lib import metrics

n, sr = 172800, 48000
x64, y64 = R.glide_pair(n, 2024, sr)
x, y = (torch.from_numpy(a.astype(np.float32)).cuda() for a in (x64, y64))
mel_a, mel_b = torch.randn(128, 360, device="cuda"), torch.randn(128, 360, device="cuda")
windows = {win: torch.hann_window(win, device="cuda") for _, _, win in R.RESOLUTIONS}


def torch_mrstft(x, y):
    total = 0.0
    for n_fft, hop, win in R.RESOLUTIONS:
        mags = []
        for s in (x, y):
            S = torch.stft(s, n_fft, hop_length=hop, win_length=win, window=windows[win], center=True, pad_mode="reflect", return_complex=True)
            mags.append(torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-8)))
        xmag, ymag = mags
        total = total + torch.norm(ymag - xmag, p="fro") / torch.norm(ymag, p="fro") + (torch.log(xmag) - torch.log(ymag)).abs().mean()
    return total / len(R.RESOLUTIONS)


def torch_si_sdr(p, t, eps=1e-8):
    p, t = p - p.mean(), t - t.mean()
    s = (p * t).sum() / ((t ** 2).sum() + eps)
    return 10 * torch.log10(((s * t) ** 2).sum() / ((p - s * t) ** 2).sum() + eps)


PAIRS = {
    "mrstft": (lambda: _native.mrstft_sums(x, y, metrics.FFT_SIZES, metrics.HOP_SIZES, metrics.WIN_LENGTHS), lambda: torch_mrstft(x, y)),
    "si_sdr": (lambda: _native.si_sdr_sums(x, y), lambda: torch_si_sdr(x, y)),
    "mel_l1 128x360": (lambda: _native.mean_abs_diff_sum(mel_a, mel_b, 360), lambda: (mel_a - mel_b).abs().mean()),
}


def window(fn, calls=100):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


for name, (native, eager) in PAIRS.items():
    for _ in range(5):
        native()
        eager()
    torch.cuda.synchronize()
    if "--calls-only" in sys.argv:
        for _ in range(20):
            native()
        torch.cuda.synchronize()
        continue
    tn, te = [], []
    for _ in range(20):
        tn.append(window(native))
        te.append(window(eager))
    tn, te = np.array(tn), np.array(te)
    print(f"{name} n={n}: K20 median {np.median(tn):.4f} ms (min {tn.min():.4f}, max {tn.max():.4f}); PyTorch-ROCm fp32 median "
          f"{np.median(te):.4f} ms (min {te.min():.4f}, max {te.max():.4f}); 20 alternating windows of 100 calls", flush=True)
if "--calls-only" in sys.argv:
    sys.exit(0)

l64 = R.mrstft_loss(torch.from_numpy(x64), torch.from_numpy(y64))
dev, eager = metrics.multi_resolution_stft_loss(x, y), float(torch_mrstft(x, y))
print(f"mrstft parity at this size: float64 twin {l64:.9g}; K20 rel err {R.rel(dev, l64):.3g}; PyTorch-ROCm fp32 rel err {R.rel(eager, l64):.3g}")
s64 = R.si_sdr(torch.from_numpy(x64), torch.from_numpy(y64))
print(f"si_sdr parity at this size: float64 twin {s64:.9g} dB; K20 err {abs(metrics.si_sdr(x, y) - s64):.3g} dB; PyTorch-ROCm fp32 err "
      f"{abs(float(torch_si_sdr(x, y)) - s64):.3g} dB", flush=True)
if "--no-loop" in sys.argv:
    sys.exit(0)

# ---- a 50-item validation_loop over 3.6 s items ----------------------------------------------------------------------------------------
from scipy.io import wavfile
from rvc_amd.infer.infer import VoiceConverter
from rvc_amd.lib import synthetic as S
from rvc_amd.train import validate as V
from rvc_amd.train.data_utils import TextAudioLoaderMultiNSFsid
from rvc_amd.train.extract import preparing_files as PF

with tempfile.TemporaryDirectory() as exp:
    for d in ("sliced_audios", "extracted", "f0", "f0_voiced"):
        os.makedirs(os.path.join(exp, d))
    for i in range(50):
        name = f"0_{i}_0"
        wavfile.write(os.path.join(exp, "sliced_audios", name + ".wav"), sr, S.synth_audio(n, seed=i, sr=sr).astype(np.float32))
        rng = np.random.default_rng(i)
        np.save(os.path.join(exp, "extracted", name + ".npy"), rng.standard_normal((180, 768)).astype(np.float32))
        f0 = 180.0 + 60.0 * np.sin(np.arange(360) / 9.0 + i)
        np.save(os.path.join(exp, "f0_voiced", name + ".wav.npy"), f0)
        np.save(os.path.join(exp, "f0", name + ".wav.npy"), np.full(360, 60))
    PF.generate_config(sr, exp)
    PF.generate_filelist(exp, sr, include_mutes=0)
    hps = V.load_hparams(exp)
    vc = VoiceConverter("cuda:0")
    vc.load_checkpoint_dict(S.make_synth_checkpoint(sr))
    ds = TextAudioLoaderMultiNSFsid(hps.data, device="cuda:0")
    V.validation_loop(vc.net_g, [ds[0], ds[1]], "cuda:0", hps)       # warm-up: kernels loaded, workspaces grown
    stages = {}
    res = V.validation_loop(vc.net_g, ds, "cuda:0", hps, stage_seconds=stages)
    total = sum(stages.values())
    print(f"validation_loop over {res['count']} items of {n} samples: {total:.3f} s, " +
          ", ".join(f"{k} {v:.3f} s ({100 * v / total:.0f} %)" for k, v in stages.items()))
