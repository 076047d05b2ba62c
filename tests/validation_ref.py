"""The float64 twin of the validation losses (K20, include/rvc_amd.h), on torch.stft on the CPU: the yardstick of
tests/test_validation_gpu.py.  The same functions evaluated on float32 tensors are "what PyTorch's own fp32 path gives", whose
distance from the float64 result sets the gates."""
import math

import numpy as np
import torch

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def _magnitudes(x, y, resolutions, eps):
    """(xmag, ymag) per resolution, [n_fft / 2 + 1, 1 + n / hop] each, in the dtype of the inputs (1-D torch tensors or arrays)"""
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    for n_fft, hop, win in resolutions:
        window = torch.hann_window(win, periodic=True, dtype=x.dtype)
        mags = []
        for s in (x, y):
            S = torch.stft(s, n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect", return_complex=True)
            mags.append(torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=eps)))
        assert mags[0].shape == (n_fft // 2 + 1, 1 + x.numel() // hop)
        yield mags


def stft_sums(x, y, resolutions=RESOLUTIONS, eps=1e-8):
    """Per resolution (sum (ymag - xmag)^2, sum ymag^2, sum |log xmag - log ymag|, number of terms) of the prediction x and the
    target y: what the device writes."""
    return [(float(((ymag - xmag) ** 2).sum()), float((ymag ** 2).sum()), float((torch.log(xmag) - torch.log(ymag)).abs().sum()),
             float(xmag.numel())) for xmag, ymag in _magnitudes(x, y, resolutions, eps)]


def stft_terms(x, y, resolutions=RESOLUTIONS, eps=1e-8):
    """Per resolution (sc, lm), formed in the dtype of the inputs as a framework would: Frobenius norms and a mean."""
    return [(float(torch.norm(ymag - xmag, p="fro") / torch.norm(ymag, p="fro")), float((torch.log(xmag) - torch.log(ymag)).abs().mean()))
            for xmag, ymag in _magnitudes(x, y, resolutions, eps)]


def mrstft_loss(x, y, resolutions=RESOLUTIONS, eps=1e-8):
    terms = stft_terms(x, y, resolutions, eps)
    return sum(sc + lm for sc, lm in terms) / len(terms)


def si_sdr(preds, target, eps=1e-8):
    """rvc/train/train.py:244-257 on 1-D tensors, in their dtype."""
    preds, target = torch.as_tensor(preds), torch.as_tensor(target)
    preds = preds - preds.mean(dim=-1, keepdim=True)
    target = target - target.mean(dim=-1, keepdim=True)
    target_energy = (target ** 2).sum(dim=-1, keepdim=True)
    scaling_factor = (preds * target).sum(dim=-1, keepdim=True) / (target_energy + eps)
    projection = scaling_factor * target
    noise = preds - projection
    return float(10 * torch.log10((projection ** 2).sum(dim=-1) / (noise ** 2).sum(dim=-1) + eps))


def mel_l1(y_hat_mel, mel):
    y_hat_mel, mel = torch.as_tensor(y_hat_mel), torch.as_tensor(mel)
    min_t = min(y_hat_mel.shape[-1], mel.shape[-1])
    return float((y_hat_mel[..., :min_t] - mel[..., :min_t]).abs().mean())


def glide_pair(n, seed, sr=48000):
    """A seeded prediction / target pair at sr: the target is a gliding harmonic tone plus noise, the prediction the same glide
    with other harmonic weights, a small detune and its own noise -> (x64, y64), float64, peak about 0.5."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 110.0 + 220.0 * rng.random() + 120.0 * np.sin(2 * np.pi * (0.7 + rng.random()) * t + rng.random())
    phase = 2 * np.pi * np.cumsum(f0) / sr
    out = []
    for detune in (1.003, 1.0):
        w = rng.random(6) + 0.2
        s = sum(w[h] / (h + 1) * np.sin((h + 1) * detune * phase + rng.random()) for h in range(6))
        s = 0.4 * s / max(np.abs(s).max(), 1e-9) + 0.02 * rng.standard_normal(n)
        out.append(s.astype(np.float32).astype(np.float64))     # float32-representable: the device sees the same signal
    return out[0], out[1]


def rel(a, b):
    return abs(a - b) / abs(b) if b else math.inf
