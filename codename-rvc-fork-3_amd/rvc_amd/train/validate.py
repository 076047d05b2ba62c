"""A checkpoint validator: the reference's ``validation_loop`` (rvc/train/train.py:1478-1579) over the hold-out of an experiment
folder, on this library -- the loader of ``rvc_amd.train.data_utils``, ``Synthesizer.infer``, ``rvc_amd.train.mel_processing``
and the native loss kernels behind ``rvc_amd.lib.metrics`` (K20).  It answers "which epoch do I keep" and "what does a faster
vocoder mode cost on my recordings" with mel L1, the multi-resolution STFT loss and SI-SDR.  PESQ is not built and is reported
as ``None`` (the reference itself skips it on any exception).

    python -m rvc_amd.train.validate EXP_DIR MODEL.pth [--all] [--seed N] [--dec-weight-dtype bf16] [--dec-arithmetic fp16x2]

prints the result as JSON and writes ``EXP_DIR/validation.json``.  There is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from rvc_amd import _native
from rvc_amd.lib import metrics
from rvc_amd.train.data_utils import TextAudioLoaderMultiNSFsid, hparams_from_dict
from rvc_amd.train.mel_processing import mel_spectrogram_torch, spec_to_mel_torch

BOUNDARIES = (50, 100, 200, 300, 400, 500, 600, 700, 800, 900)   # train.py:547, :568


def holdout_indices(n_items: int, seed: int) -> list:
    """The validation share of train.py:531-538: ``random_split(dataset, [int(0.9 n), n - int(0.9 n)],
    generator=manual_seed(seed))`` permutes the indices once with that generator and hands out consecutive runs, so the hold-out
    is what follows the first int(0.9 n) entries of the permutation."""
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(int(seed))).tolist()
    return perm[int(0.90 * n_items):]


def bucket_order(lengths, boundaries=BOUNDARIES) -> list:
    """The positions that ``DistributedBucketSampler(dataset, 1, boundaries, num_replicas=1, rank=0, shuffle=False)`` visits, in
    its order (data_utils.py:277-350).  An item of length L (its WAV's bytes // (3 hop)) belongs to bucket k when
    boundaries[k] < L <= boundaries[k + 1] and to none -- it is left out -- when L <= boundaries[0] or L > boundaries[-1]: with
    the reference's boundaries, L <= 50 or L > 900.  Buckets are walked in ascending order, a bucket's items in dataset order.  At
    batch size 1 no bucket is topped up with repeats."""
    buckets = [[] for _ in range(len(boundaries) - 1)]
    for i, length in enumerate(lengths):
        for k in range(len(boundaries) - 1):
            if boundaries[k] < length <= boundaries[k + 1]:
                buckets[k].append(i)
                break
    return [i for bucket in buckets for i in bucket]


def item_noise(net_g, frames: int, seed: int) -> dict:
    """Every random tensor ``net_g.infer`` draws for one item of ``frames`` frames, from a host generator seeded with ``seed``
    (the shapes and the order of ``Synthesizer._draw``)."""
    g = torch.Generator().manual_seed(int(seed))
    length = frames * net_g.upp
    out = {"z": torch.randn(1, net_g.inter_channels, frames, generator=g)}
    if net_g.vocoder == "HiFi-GAN":
        out["src_rand"] = torch.rand(1, 1, 1, generator=g)
        out["src_randn"] = torch.randn(1, length, 1, generator=g)
    else:
        dim = 9 if net_g.vocoder == "MRF HiFi-GAN" else 1
        out["src_rand"] = torch.rand(1, dim, generator=g)
        out["src_randn"] = torch.randn(1, length, dim, generator=g)
    if net_g.vocoder == "RefineGAN":
        out["adain_randn"] = torch.cat([torch.randn(*sh, generator=g).reshape(-1) for sh in net_g._adain_shapes(1, frames)])
    return out


def infer_item(net_g, item, device, noise) -> torch.Tensor:
    """``net_g.infer`` over one loader item as a batch of one -> y_hat [samples] on the device."""
    _, _, phone, pitch, pitchf, sid = item
    frames = phone.shape[0]
    y_hat, _, _ = net_g.infer(phone.unsqueeze(0).to(device), torch.tensor([frames], device=device), pitch.unsqueeze(0).to(device),
                              pitchf.unsqueeze(0).to(device), sid.to(device), noise=noise, phone_lengths_host=[frames])
    return y_hat.reshape(-1)


def score_item(y_hat, item, hps) -> dict:
    """train.py:1504-1545 for one item: the mel L1 over the common frames min_t of the two mels, the multi-resolution STFT loss
    over the first min(min_t hop, len(wave), len(y_hat)) samples, SI-SDR over the samples both signals have (the reference's
    expression needs equal lengths)."""
    d = hps.data
    spec, wave = item[0], item[1].reshape(-1)
    y_hat_mel = mel_spectrogram_torch(y_hat.unsqueeze(0), d.filter_length, d.n_mel_channels, d.sample_rate, d.hop_length, d.win_length,
                                      d.mel_fmin, d.mel_fmax)[0]
    mel = spec_to_mel_torch(spec.unsqueeze(0), d.filter_length, d.n_mel_channels, d.sample_rate, d.mel_fmin, d.mel_fmax)[0]
    min_t = min(y_hat_mel.shape[-1], mel.shape[-1])
    min_samples = min(min_t * d.hop_length, wave.shape[-1], y_hat.shape[-1])
    common = min(wave.shape[-1], y_hat.shape[-1])
    return {"mel_l1": metrics.mel_l1(y_hat_mel, mel),
            "mrstft": metrics.multi_resolution_stft_loss(y_hat[:min_samples], wave[:min_samples]),
            "si_sdr": metrics.si_sdr(y_hat[:common], wave[:common])}


def validation_loop(net_g, dataset, device, hps, *, noise_seed: int = 0, stage_seconds: dict = None, waveforms: list = None) -> dict:
    """Score every item of ``dataset`` (anything with ``len`` and ``[i]`` that yields the loader's tuples) and average.

    Each item is scored ALONE: this is the reference's loop at batch size 1.  In a padded batch the reference's mel, STFT and
    SI-SDR terms run over the zero padding of the shorter items too, so its figures depend on how items happen to be batched;
    here zero-padding never enters a metric.  Item i is synthesised with the noise of ``item_noise(net_g, frames, noise_seed + i)``.

    -> {"mel_l1", "mrstft", "si_sdr": the means over the items, "pesq": None, "count", "per_item": [{"mel_l1", "mrstft",
    "si_sdr", "frames", "samples"}, ...]}.  ``stage_seconds``: a dict that receives the wall time per stage (load, infer, score),
    each stage synchronised -- timing runs only.  ``waveforms``: a list that receives every item's y_hat (device tensors): the
    networks under ``infer`` run on PyTorch's BLAS / conv libraries, which are not bit-stable from call to call, so whoever wants
    to re-score an item needs the waveform that was scored."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _native.NativeError(f"validation_loop needs a HIP device, got {device} (no CPU fallback)")
    per_item = []

    def lap(stage, t0):
        if stage_seconds is not None:
            torch.cuda.synchronize(device)
            stage_seconds[stage] = stage_seconds.get(stage, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    with torch.no_grad(), torch.cuda.device(device):
        for i in range(len(dataset)):
            t0 = time.perf_counter()
            item = dataset[i]
            t0 = lap("load", t0)
            frames = item[2].shape[0]
            y_hat = infer_item(net_g, item, device, item_noise(net_g, frames, noise_seed + i))
            t0 = lap("infer", t0)
            if waveforms is not None:
                waveforms.append(y_hat)
            scores = score_item(y_hat, item, hps)
            lap("score", t0)
            scores.update(frames=frames, samples=int(y_hat.shape[-1]))
            per_item.append(scores)
    count = len(per_item)
    if count == 0:
        raise ValueError("validation_loop: no item to score (the hold-out is empty, or the bucket rule left every item out)")
    out = {k: sum(p[k] for p in per_item) / count for k in ("mel_l1", "mrstft", "si_sdr")}
    out.update(pesq=None, count=count, per_item=per_item)
    return out


class _Subset:
    def __init__(self, dataset, indices):
        self.dataset, self.indices = dataset, list(indices)

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        return self.dataset[self.indices[i]]


def load_hparams(exp_dir: str):
    path = os.path.join(exp_dir, "config.json")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} does not exist (rvc_amd.train.extract.preparing_files.generate_config writes it)")
    with open(path) as f:
        hps = hparams_from_dict(json.load(f))
    hps.data.training_files = os.path.join(exp_dir, "filelist.txt")
    if not os.path.isfile(hps.data.training_files):
        raise FileNotFoundError(f"{hps.data.training_files} does not exist (generate_filelist writes it)")
    return hps


def validate_checkpoint(exp_dir: str, model_path, *, device: str = "cuda:0", seed: int = None, all_items: bool = False,
                        dec_weight_dtype: str = "f32", dec_arithmetic: str = "exact", noise_seed: int = 0) -> dict:
    """Score the exported model ``model_path`` (a ``.pth`` file, or its dict) on the experiment folder ``exp_dir`` (config.json,
    filelist.txt and what it names).  The items are the hold-out of ``holdout_indices(len(dataset), seed)`` -- ``seed`` defaults
    to the config's ``train.seed`` -- or every item with ``all_items``; either way those the bucket rule leaves out are dropped
    and the rest visited in ``bucket_order``.  ``dec_weight_dtype`` / ``dec_arithmetic`` choose the vocoder mode as on
    ``VoiceConverter``."""
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise _native.NativeError(f"validate_checkpoint needs a HIP device, got {device!r} (no CPU fallback)")
    from rvc_amd.infer.infer import VoiceConverter
    hps = load_hparams(exp_dir)
    if isinstance(model_path, dict):
        cpt, model_name = model_path, model_path.get("model_name", "<dict>")
    else:
        if not os.path.isfile(model_path):
            raise FileNotFoundError(f"{model_path} does not exist")
        cpt, model_name = torch.load(model_path, map_location="cpu", weights_only=True), str(model_path)
    if cpt["config"][-1] != hps.data.sample_rate:
        raise ValueError(f"the model is a {cpt['config'][-1]} Hz model, the experiment's config.json says {hps.data.sample_rate} Hz")
    vc = VoiceConverter(device)
    vc.dec_weight_dtype, vc.dec_arithmetic = dec_weight_dtype, dec_arithmetic
    vc.load_checkpoint_dict(cpt)
    full = TextAudioLoaderMultiNSFsid(hps.data, device=device)
    seed = hps.train.seed if seed is None else int(seed)
    chosen = list(range(len(full))) if all_items else holdout_indices(len(full), seed)
    visited = [chosen[p] for p in bucket_order([full.lengths[i] for i in chosen])]
    result = validation_loop(vc.net_g, _Subset(full, visited), device, hps, noise_seed=noise_seed)
    result.update(model=model_name, items=visited, left_out=len(chosen) - len(visited), seed=seed, all_items=bool(all_items),
                  dec_weight_dtype=dec_weight_dtype, dec_arithmetic=dec_arithmetic)
    return result


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m rvc_amd.train.validate", description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_dir")
    ap.add_argument("model")
    ap.add_argument("--all", action="store_true", help="score every item of the file list, not only the 10 %% hold-out")
    ap.add_argument("--seed", type=int, default=None, help="the split's seed (default: train.seed of config.json)")
    ap.add_argument("--dec-weight-dtype", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--dec-arithmetic", default="exact", choices=("exact", "fp16x2"))
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    result = validate_checkpoint(args.exp_dir, args.model, device=args.device, seed=args.seed, all_items=args.all,
                                 dec_weight_dtype=args.dec_weight_dtype, dec_arithmetic=args.dec_arithmetic)
    text = json.dumps(result, indent=2)
    with open(os.path.join(args.exp_dir, "validation.json"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
