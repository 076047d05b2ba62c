"""The training-set loader with the reference's surface (rvc/train/data_utils.py:10-165): ``TextAudioLoaderMultiNSFsid`` reads one
``filelist.txt`` line -- WAV, features, coarse f0, voiced f0, speaker -- into ``(spec, wav, phone, pitch, pitchf, sid)``.

The WAV is decoded by ``rvc_amd.lib.audio.read_wav`` and the linear spectrogram comes from ``spectrogram_torch`` (librvc_amd's
K4b transform) on ``device``; ``spec`` and ``wav`` are device tensors, the labels stay on the host as in the reference.  The
reference caches every spectrogram next to its WAV as ``.spec.pt``; this loader neither writes nor reads such files: it leaves the
dataset folder as it found it, and the transform is a fraction of a millisecond per item.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch

from rvc_amd.lib.audio import read_wav
from rvc_amd.train.mel_processing import spectrogram_torch

MAX_FRAMES = 900   # data_utils.py:102


def load_filepaths_and_text(filename, split="|"):
    """rvc/train/utils.py:204-213"""
    with open(filename, encoding="utf-8") as f:
        return [line.strip().split(split) for line in f]


def hparams_from_dict(d):
    """A nested dict (a parsed config.json) with attribute access, like the reference's HParams."""
    return SimpleNamespace(**{k: hparams_from_dict(v) if isinstance(v, dict) else v for k, v in d.items()})


def reconcile_lengths(spec, wav, phone, pitch, pitchf, hop_length):
    """data_utils.py:74-85: when the feature count and the spectrogram length differ, everything is cut to the shorter of the two
    (the waveform to that many hops)."""
    len_phone, len_spec = phone.shape[0], spec.shape[-1]
    if len_phone != len_spec:
        len_min = min(len_phone, len_spec)
        spec, wav = spec[:, :len_min], wav[:, :len_min * hop_length]
        phone, pitch, pitchf = phone[:len_min, :], pitch[:len_min], pitchf[:len_min]
    return spec, wav, phone, pitch, pitchf


class TextAudioLoaderMultiNSFsid(torch.utils.data.Dataset):
    def __init__(self, hparams, device="cuda:0"):
        """``hparams``: the ``data`` section of config.json plus ``training_files`` (the file list); min_text_len / max_text_len
        default to 1 / 5000 as in the reference."""
        for name in ("max_wav_value", "sample_rate", "filter_length", "hop_length", "win_length"):
            setattr(self, name, getattr(hparams, name))
        self.min_text_len = getattr(hparams, "min_text_len", 1)
        self.max_text_len = getattr(hparams, "max_text_len", 5000)
        self.device = device
        self.audiopaths_and_text = load_filepaths_and_text(hparams.training_files)
        self._filter()

    def _filter(self):
        """data_utils.py:30-41: lines whose feature PATH is between min_text_len and max_text_len characters long are kept (that is
        what the reference measures), and an item's length is its WAV's size in bytes // (3 * hop_length)."""
        kept, lengths = [], []
        for audiopath, text, pitch, pitchf, dv in self.audiopaths_and_text:
            if self.min_text_len <= len(text) <= self.max_text_len:
                if not os.path.isfile(audiopath):
                    raise FileNotFoundError(f"the file list names {audiopath}, which does not exist")
                kept.append([audiopath, text, pitch, pitchf, dv])
                lengths.append(os.path.getsize(audiopath) // (3 * self.hop_length))
        self.audiopaths_and_text = kept
        self.lengths = lengths

    def get_sid(self, sid):
        """The speaker column as a LongTensor [1]; a column that is not an integer counts as speaker 0, with a note on stdout
        (data_utils.py:43-55)."""
        try:
            value = int(sid)
        except ValueError:
            print(f"speaker column {sid!r} of the file list is not an integer: speaker 0 is used")
            value = 0
        return torch.LongTensor([value])

    def get_labels(self, phone, pitch, pitchf):
        """data_utils.py:89-109: the features repeated twice along time, everything capped at 900 frames."""
        for path in (phone, pitch, pitchf):
            if not os.path.isfile(path):
                raise FileNotFoundError(f"the file list names {path}, which does not exist")
        phone = np.repeat(np.load(phone), 2, axis=0)
        pitch, pitchf = np.load(pitch), np.load(pitchf)
        n_num = min(phone.shape[0], MAX_FRAMES)
        return torch.FloatTensor(phone[:n_num, :]), torch.LongTensor(pitch[:n_num]), torch.FloatTensor(pitchf[:n_num])

    def get_audio(self, filename):
        """data_utils.py:111-150 without the .spec.pt cache: -> (spec [filter_length / 2 + 1, frames], wav [1, n]) on the device."""
        if not os.path.isfile(filename):
            raise FileNotFoundError(f"the file list names {filename}, which does not exist")
        audio, sample_rate = read_wav(filename)
        if sample_rate != self.sample_rate:
            raise ValueError(f"{filename} is sampled at {sample_rate} Hz, the experiment is configured for {self.sample_rate} Hz")
        if audio.ndim != 1:
            raise ValueError(f"{filename}: the training set holds mono files, this one has {audio.shape[1]} channels")
        audio_norm = torch.from_numpy(audio.astype(np.float32)).to(self.device).unsqueeze(0)
        spec = spectrogram_torch(audio_norm, self.filter_length, self.hop_length, self.win_length, center=False)
        return torch.squeeze(spec, 0), audio_norm

    def get_audio_text_pair(self, audiopath_and_text):
        file, phone, pitch, pitchf, dv = audiopath_and_text[:5]
        phone, pitch, pitchf = self.get_labels(phone, pitch, pitchf)
        spec, wav = self.get_audio(file)
        dv = self.get_sid(dv)
        spec, wav, phone, pitch, pitchf = reconcile_lengths(spec, wav, phone, pitch, pitchf, self.hop_length)
        return (spec, wav, phone, pitch, pitchf, dv)

    def __getitem__(self, index):
        return self.get_audio_text_pair(self.audiopaths_and_text[index])

    def __len__(self):
        return len(self.audiopaths_and_text)
