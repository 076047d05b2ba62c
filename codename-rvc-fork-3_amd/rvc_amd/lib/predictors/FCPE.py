"""FCPE F0 estimator on the GPU (rvc/lib/predictors/fcpe.py, rvc/lib/predictors/torchfcpe/**), conv-only conformer.

* log-mel front end  -> librvc_amd K4b handle (``rvc_mel_*``; mel_extractor.py:127-151) + the frame fix-up of :253-257
* dense layers       -> K11 (``rvc_conv1d_bf16x3`` for input_stack's k = 3 convs, ``rvc_linear_bf16x3`` for the 1x1 convs of the
                        conformer blocks and the output projection, residual fused)
* everything between -> K15 (csrc/fcpe.hip): GroupNorm + LeakyReLU, LayerNorm, GLU + depthwise FIR + SiLU, decode
* host tail          -> ``_resize_f0`` / ``_interpolate_f0`` (fcpe.py:30-77) restated in float64 after ONE device -> host read

The architecture is read from the checkpoint's ``config_dict`` as the reference does (models_infer.py:342-448).  Performer
attention (``conv_only = false``), sample rates other than the model's, test-time augmentation and the "argmax" decoder are not built
and raise ``NotImplementedError``; no reference call site reaches them.
"""
from __future__ import annotations

import copy
import os
from typing import Optional, Union

import numpy as np
import torch


def fold_fcpe_checkpoint(ckpt: dict) -> tuple[dict, dict]:
    """The reference's ``{"config_dict": ..., "model": state_dict}`` -> (config, host weights): checks the configuration, folds
    ``output_proj``'s weight norm (both key spellings) and zero-pads the projection to a multiple of 128 rows for K11."""
    if not isinstance(ckpt, dict) or "config_dict" not in ckpt or "model" not in ckpt:
        raise ValueError('an FCPE checkpoint is {"config_dict": ..., "model": state_dict}')
    cfg = copy.deepcopy(dict(ckpt["config_dict"]))
    model, mel = cfg["model"], cfg["mel"]
    model["conv_dropout"] = model["atten_dropout"] = 0.0            # spawn_bundled_infer_model, models_infer.py:354-356
    if model.get("type", "CFNaiveMelPE") != "CFNaiveMelPE":
        raise ValueError(f"config_dict.model.type is {model['type']!r}, only 'CFNaiveMelPE' exists")
    if cfg.get("is_onnx"):
        raise ValueError("this checkpoint describes an ONNX model")
    if not model.get("conv_only", False):
        raise NotImplementedError("config_dict.model.conv_only is false: the Performer attention branch is not built")
    hidden, out_dims = int(model["hidden_dims"]), int(model["out_dims"])
    if hidden % 64 or hidden > 1024:
        raise NotImplementedError(f"config_dict.model.hidden_dims = {hidden}: a multiple of 64 up to 1024 is built")
    if int(mel["num_mels"]) % 16:
        raise NotImplementedError(f"config_dict.mel.num_mels = {mel['num_mels']}: a multiple of 16 is built")
    sd = {k: v.detach().float().cpu() for k, v in ckpt["model"].items()}
    w = {}
    w["in0.w"], w["in0.b"] = sd["input_stack.0.weight"], sd["input_stack.0.bias"]
    w["gn.g"], w["gn.b"] = sd["input_stack.1.weight"], sd["input_stack.1.bias"]
    w["in3.w"], w["in3.b"] = sd["input_stack.3.weight"], sd["input_stack.3.bias"]
    if model.get("use_harmonic_emb", False):                           # models.py:112-114: inference adds row 0
        w["hemb"] = sd["harmonic_emb.weight"][0]
    for i in range(int(model["n_layers"])):
        p = f"net.encoder_layers.{i}.conformer.net"
        w[f"l{i}.ln.g"], w[f"l{i}.ln.b"] = sd[p + ".0.weight"], sd[p + ".0.bias"]
        w[f"l{i}.up.w"], w[f"l{i}.up.b"] = sd[p + ".2.weight"].squeeze(-1), sd[p + ".2.bias"]
        w[f"l{i}.dw.w"], w[f"l{i}.dw.b"] = sd[p + ".4.conv.weight"].squeeze(1), sd[p + ".4.conv.bias"]
        w[f"l{i}.down.w"], w[f"l{i}.down.b"] = sd[p + ".6.weight"].squeeze(-1), sd[p + ".6.bias"]
        if w[f"l{i}.dw.w"].shape[1] % 2 == 0 or w[f"l{i}.dw.w"].shape[1] > 31:
            raise NotImplementedError(f"depthwise kernel of {w[f'l{i}.dw.w'].shape[1]} taps: odd sizes up to 31 are built")
    w["norm.g"], w["norm.b"] = sd["norm.weight"], sd["norm.bias"]
    if "output_proj.parametrizations.weight.original0" in sd:
        wg, wv = sd["output_proj.parametrizations.weight.original0"], sd["output_proj.parametrizations.weight.original1"]
    elif "output_proj.weight_g" in sd:
        wg, wv = sd["output_proj.weight_g"], sd["output_proj.weight_v"]
    else:
        wg, wv = None, sd["output_proj.weight"]
    proj = wv if wg is None else (wv.double() * (wg.double() / wv.double().norm(2, dim=1, keepdim=True))).float()
    pad = -out_dims % 128
    w["proj.w"] = torch.cat([proj, torch.zeros(pad, hidden)], 0)
    w["proj.b"] = torch.cat([sd["output_proj.bias"], torch.zeros(pad)], 0)
    w["cent_table"] = sd["cent_table"]
    return cfg, {k: v.contiguous() for k, v in w.items()}


def resize_f0(x: np.ndarray, target_len: int) -> np.ndarray:
    """fcpe.py:68-77: unvoiced frames (< 0.001) become gaps, the contour is read off at target_len equally spaced positions."""
    source = np.array(x)
    source[source < 0.001] = np.nan
    n = len(source)
    target = np.interp(np.arange(0, n * target_len, n) / target_len, np.arange(0, n), source)
    return np.nan_to_num(target)


def interpolate_f0(f0: np.ndarray) -> np.ndarray:
    """fcpe.py:30-66 (the contour it returns; the voiced flags are dropped by the caller there too).  An unvoiced run between two
    voiced frames becomes the straight line between them, a leading run takes the first voiced value, a trailing run the last one.
    The reference tests ``j < frame_number - 1`` for "a voiced frame follows", so a run that ends at a voiced LAST frame counts
    as trailing and that frame is overwritten as well.  Same float64 operations per element as the reference's loops, whose
    rescans of an unvoiced tail (quadratic in its length) are left out."""
    d = np.array(f0, dtype=np.float64).reshape(-1)
    n = d.size
    voiced = np.flatnonzero(d > 0.0)
    last = 0.0
    i = 0
    while i < n:
        if d[i] > 0.0:
            last = d[i]
            i += 1
            continue
        k = np.searchsorted(voiced, i)                       # the first voiced frame behind the run, if any
        j = int(voiced[k]) if k < voiced.size else n
        if j < n - 1:
            if last > 0.0:
                step = (d[j] - d[i - 1]) / float(j - i)
                d[i:j] = d[i - 1] + step * np.arange(1, j - i + 1, dtype=np.float64)
            else:
                d[i:j] = d[j]
            i = j
        else:
            d[i:] = last
            break
    return d


class FCPE:
    """The reference's constructor arguments (fcpe.py:80-95).  ``f0_min`` / ``f0_max`` are stored and, as there, not used: the
    model's own ``f0_min`` masks the contour.  Without a file at ``model_path`` the seeded synthetic checkpoint is loaded, the
    way RMVPE0Predictor treats a missing rmvpe.pt."""

    def __init__(self, hop_length=160, f0_min=50, f0_max=1100, sampling_rate=16000, device="cuda:0", model_path: str = None,
                 checkpoint: dict | None = None):
        self.hop_length, self.f0_min, self.f0_max, self.sampling_rate = hop_length, f0_min, f0_max, sampling_rate
        self.device = torch.device(device if device is not None else "cuda:0")
        if checkpoint is None:
            if model_path is not None and os.path.isfile(str(model_path)):
                checkpoint = torch.load(str(model_path), map_location="cpu", weights_only=True)
            else:
                from rvc_amd.lib.synthetic import make_fcpe_checkpoint
                checkpoint = make_fcpe_checkpoint(0)
        self.load_checkpoint(checkpoint)

    def load_checkpoint(self, ckpt: dict):
        from rvc_amd import _native
        from rvc_amd.train.mel_processing import librosa_mel_fn
        self.cfg, w = fold_fcpe_checkpoint(ckpt)
        m, mel = self.cfg["model"], self.cfg["mel"]
        self.hidden, self.out_dims, self.n_layers = int(m["hidden_dims"]), int(m["out_dims"]), int(m["n_layers"])
        self.model_f0_min = float(m["f0_min"])
        self.model_sr, self.hop = int(mel["sr"]), int(mel["hop_size"])
        n_fft, win = int(mel["n_fft"]), int(mel["win_size"])
        self.pad = (win - self.hop) // 2                                  # mel_extractor.py:127
        if (win - self.hop + 1) // 2 != self.pad:
            raise NotImplementedError("config_dict.mel: win_size - hop_size must be even (symmetric reflect padding)")
        fmin = mel.get("fmin") or 0
        fmax = mel.get("fmax") or self.model_sr / 2
        basis = librosa_mel_fn(self.model_sr, n_fft, int(mel["num_mels"]), fmin, fmax)
        self.mel = _native.MelTransform(n_fft, self.hop, win, self.pad, basis, mag_eps=1e-9, log_floor=float(mel.get("clip_val", 1e-5)),
                                        device=self.device)
        # weights: the GEMM operands packed once for K11, the rest as they are
        self.w, self.a = {}, {}
        for k, v in w.items():
            if k.endswith((".up.w", ".down.w", "proj.w", "in0.w", "in3.w")):
                self.a[k] = _native.gemm_bf16x3_pack_weight(v, self.device)
            else:
                self.w[k] = v.to(self.device)
        self.proj_rows = w["proj.w"].shape[0]
        return self

    # ---- device forward -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def mel_device(self, audio: torch.Tensor) -> torch.Tensor:
        """audio [n] fp32 on the device -> log-mel [num_mels, n // hop + 1] (Wav2MelModule.__call__, mel_extractor.py:252-259)."""
        n = audio.shape[0]
        if n <= self.pad:
            raise ValueError(f"FCPE needs more than {self.pad} samples (got {n}): shorter inputs are padded with constants in the "
                             "reference, which the mel kernel does not do")
        mel, _ = self.mel.forward(audio.view(1, -1))
        mel = mel[0]
        n_frames = n // self.hop + 1
        if n_frames > mel.shape[1]:
            mel = torch.cat((mel, mel[:, -1:]), 1)
        if n_frames < mel.shape[1]:
            mel = mel[:, :n_frames]
        return mel.contiguous()

    @torch.no_grad()
    def logits_device(self, mel: torch.Tensor) -> torch.Tensor:
        """log-mel [num_mels, T] -> logits [T, proj_rows] (columns >= out_dims are padding); CFNaiveMelPE.forward before the sigmoid."""
        from rvc_amd import _native as N
        w, a, h = self.w, self.a, self.hidden
        x = N.conv1d_bf16x3(mel.unsqueeze(0), a["in0.w"], w["in0.b"], h, 3, 1, 1)
        x = N.groupnorm_lrelu(x[0], w["gn.g"], w["gn.b"], 4, 1e-5, 0.01)
        x = N.conv1d_bf16x3(x.unsqueeze(0), a["in3.w"], w["in3.b"], h, 3, 1, 1)
        x = x[0].t().contiguous()                                          # time-major from here on
        if "hemb" in w:
            x = x + w["hemb"]
        for i in range(self.n_layers):
            y = N.layernorm_rows(x, w[f"l{i}.ln.g"], w[f"l{i}.ln.b"])
            y = N.linear_bf16x3(y, a[f"l{i}.up.w"], w[f"l{i}.up.b"], 4 * h)
            y = N.glu_dwconv_silu(y, w[f"l{i}.dw.w"], w[f"l{i}.dw.b"])
            x = N.linear_bf16x3(y, a[f"l{i}.down.w"], w[f"l{i}.down.b"], h, res=x)
        x = N.layernorm_rows(x, w["norm.g"], w["norm.b"])
        return N.linear_bf16x3(x, a["proj.w"], w["proj.b"], self.proj_rows)

    @torch.no_grad()
    def infer_device(self, audio: torch.Tensor, threshold: float = 0.006, taps: dict | None = None) -> torch.Tensor:
        """audio [n] on the device -> f0 [n // hop + 1] fp32 on the device, 0 = unvoiced (InferCFNaiveMelPE.infer with its defaults)."""
        from rvc_amd import _native as N
        mel = self.mel_device(audio.float().contiguous().view(-1))
        logits = self.logits_device(mel)
        f0, latent = N.fcpe_decode(logits, self.w["cent_table"], self.out_dims, threshold, self.model_f0_min, want_latent=taps is not None)
        if taps is not None:      # tests: what stands behind the contour
            taps["mel"], taps["latent"] = mel, latent
        return f0

    def compute_f0(self, wav, p_len: Optional[int] = None, filter_radius: Optional[Union[int, float]] = 0.006,
                   sr: Optional[int] = None, decoder_mode: str = "local_argmax", test_time_augmentation: bool = False) -> np.ndarray:
        """fcpe.py:107-131: NumPy (or tensor) audio at the model's rate in, float64 NumPy contour of p_len frames out.
        ``filter_radius`` is the confidence threshold of the decoder, as in the reference."""
        sr = self.sampling_rate if sr is None else sr
        if sr != self.model_sr:
            raise NotImplementedError(f"sr = {sr}: FCPE runs at the model's {self.model_sr} Hz only (no resampler in front of it)")
        if decoder_mode != "local_argmax":
            raise NotImplementedError(f"decoder_mode = {decoder_mode!r}: only 'local_argmax' is built")
        if test_time_augmentation:
            raise NotImplementedError("test_time_augmentation (key-shifted passes) is not built")
        p_len = wav.shape[0] // self.hop_length + 1 if p_len is None else p_len
        if not torch.is_tensor(wav):
            wav = torch.from_numpy(np.ascontiguousarray(wav))
        f0 = self.infer_device(wav.float().to(self.device), float(filter_radius)).cpu().numpy()
        return interpolate_f0(resize_f0(f0, p_len))
