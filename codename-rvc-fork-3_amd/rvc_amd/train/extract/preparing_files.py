"""The step between ``extract`` and the loader, with the reference's surface (rvc/train/extract/preparing_files.py:11-83):
``generate_config`` puts the experiment's ``config.json`` in place and ``generate_filelist`` writes ``filelist.txt`` and the
speaker count of ``model_info.json``.

``config.json`` is written from the per-rate hyper-parameters this package carries (``rvc_amd.lib.synthetic.MODEL_CONFIGS``, the
same table the synthetic checkpoints are built from) instead of being copied out of a configs folder.
"""
from __future__ import annotations

import json
import os
from random import shuffle

from rvc_amd.lib.synthetic import MODEL_CONFIGS

_SEGMENT_SIZE = {48000: 17280, 40000: 12800, 32000: 12800}
_N_MEL_CHANNELS = {48000: 128, 40000: 125, 32000: 80}


def training_config(sample_rate: int) -> dict:
    """The hyper-parameters of one sample rate in the layout of the reference's ``rvc/configs/<rate>.json``."""
    if sample_rate not in MODEL_CONFIGS:
        raise ValueError(f"no hyper-parameters for a sample rate of {sample_rate!r} (known: {sorted(MODEL_CONFIGS)})")
    c = MODEL_CONFIGS[sample_rate]
    return {
        "train": {"log_interval": 200, "seed": 1234, "learning_rate": 1e-4, "betas": [0.8, 0.99], "eps": 1e-9, "bf16_run": True,
                  "lr_decay": 0.999875, "segment_size": _SEGMENT_SIZE[sample_rate], "c_mel": 45, "c_kl": 1.0},
        "data": {"max_wav_value": 32768.0, "sample_rate": sample_rate, "filter_length": c["filter_length"],
                 "hop_length": sample_rate // 100, "win_length": c["filter_length"], "n_mel_channels": _N_MEL_CHANNELS[sample_rate],
                 "mel_fmin": 0.0, "mel_fmax": None},
        "model": {"inter_channels": 192, "hidden_channels": 192, "filter_channels": 768, "text_enc_hidden_dim": 768, "n_heads": 2,
                  "n_layers": 6, "kernel_size": 3, "p_dropout": 0, "resblock": "1", "resblock_kernel_sizes": [3, 7, 11],
                  "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]], "upsample_rates": list(c["upsample_rates"]),
                  "upsample_initial_channel": 512, "upsample_kernel_sizes": list(c["upsample_kernel_sizes"]),
                  "use_spectral_norm": False, "gin_channels": 256, "spk_embed_dim": 109},
    }


def generate_config(sample_rate: int, model_path: str):
    """preparing_files.py:11-15: ``model_path/config.json``, left alone when it exists."""
    config_save_path = os.path.join(model_path, "config.json")
    if not os.path.exists(config_save_path):
        with open(config_save_path, "w") as f:
            json.dump(training_config(sample_rate), f, indent=4)


def generate_filelist(model_path: str, sample_rate: int, include_mutes: int = 2, embedder_model: str = "contentvec"):
    """preparing_files.py:18-83.  One line ``wav|features|coarse f0|voiced f0|speaker`` per name that is present in all of
    ``sliced_audios``, ``extracted``, ``f0`` and ``f0_voiced`` (a name is what precedes the first dot, the speaker what precedes
    the first underscore), then ``include_mutes`` lines per speaker that point at the mute files of ``<cwd>/logs/mute`` (``mute_spin``
    for other embedders).  The lines are shuffled with the global ``random`` as in the reference, so their set is defined and their
    order is not.  ``model_info.json`` keeps its other entries and gains ``speakers_id``.

    The mute files are the reference's own assets: this package neither ships nor creates them, and the loader raises on a line
    whose WAV is missing, so pass ``include_mutes=0`` unless ``<cwd>/logs/mute`` is in place.  ``<cwd>`` is the working directory at
    the time of the call (the reference fixes it when its module is imported)."""
    gt_wavs_dir = os.path.join(model_path, "sliced_audios")
    feature_dir = os.path.join(model_path, "extracted")
    f0_dir = os.path.join(model_path, "f0")
    f0nsf_dir = os.path.join(model_path, "f0_voiced")
    names = None
    for folder in (gt_wavs_dir, feature_dir, f0_dir, f0nsf_dir):
        stems = set(name.split(".")[0] for name in os.listdir(folder))
        names = stems if names is None else names & stems

    mute_base_path = os.path.join(os.getcwd(), "logs", "mute" if embedder_model == "contentvec" else "mute_spin")
    options, sids = [], []
    for name in names:
        sid = name.split("_")[0]
        if sid not in sids:
            sids.append(sid)
        options.append("|".join([os.path.join(gt_wavs_dir, name) + ".wav", os.path.join(feature_dir, name) + ".npy",
                                 os.path.join(f0_dir, name) + ".wav.npy", os.path.join(f0nsf_dir, name) + ".wav.npy", sid]))
    if include_mutes > 0:
        mute = "|".join([os.path.join(mute_base_path, "sliced_audios", f"mute{sample_rate}.wav"),
                         os.path.join(mute_base_path, "extracted", "mute.npy"),
                         os.path.join(mute_base_path, "f0", "mute.wav.npy"),
                         os.path.join(mute_base_path, "f0_voiced", "mute.wav.npy")])
        for sid in sids * include_mutes:
            options.append(f"{mute}|{sid}")

    info_path = os.path.join(model_path, "model_info.json")
    data = {}
    if os.path.exists(info_path):
        with open(info_path, "r") as f:
            data = json.load(f)
    data.update({"speakers_id": len(sids)})
    with open(info_path, "w") as f:
        json.dump(data, f, indent=4)

    shuffle(options)
    with open(os.path.join(model_path, "filelist.txt"), "w") as f:
        f.write("\n".join(options))
