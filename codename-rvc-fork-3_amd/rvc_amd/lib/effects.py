"""``Pedalboard`` and its effects -- the board behind ``post_process`` (rvc/infer/infer.py:130-191 builds a ``pedalboard``
chain of Reverb, PitchShift, Limiter, Gain, Distortion, Chorus, Bitcrush, Clipping, Compressor and Delay and calls
``board(audio, sample_rate)``).

What is built is the native kernel family K22 (csrc/effects.hip); each effect's formula is spelled out in include/rvc_amd.h.  The
pedalboard wheel (JUCE underneath) is not a dependency and was not available to compare against: parity with it is unpinned,
the specification in the header is this build's own, and its float64 NumPy restatement lives in tests/effects_ref.py.
Parameters are constant over the signal (JUCE's 50 ms parameter smoothing is not modelled), the signal is mono, and
``PitchShift`` (Rubber Band) is not built: it raises NotImplementedError.

There is no host implementation: the signal is processed on the device, on the current stream.
"""
from __future__ import annotations

import numpy as np
import torch

from rvc_amd import _native


class _Effect:
    _stage = 0           # the pointwise effects' bit in rvc_fx_pointwise_f32's `stages`

    def _run(self, x: torch.Tensor, sr: int) -> torch.Tensor:
        raise NotImplementedError

    def __call__(self, audio, sample_rate):
        return Pedalboard([self])(audio, sample_rate)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in vars(self).items())})"


class Reverb(_Effect):
    def __init__(self, room_size: float = 0.5, damping: float = 0.5, wet_level: float = 0.33, dry_level: float = 0.4,
                 width: float = 1.0, freeze_mode: float = 0.0):
        self.room_size, self.damping, self.wet_level, self.dry_level = room_size, damping, wet_level, dry_level
        self.width, self.freeze_mode = width, freeze_mode

    def _run(self, x, sr):
        return _native.fx_reverb(x, sr, self.room_size, self.damping, self.wet_level, self.dry_level, self.width, self.freeze_mode)


class PitchShift(_Effect):
    def __init__(self, semitones: float = 0.0):
        raise NotImplementedError("PitchShift (pitch_shift) is not part of this build: pedalboard's PitchShift is Rubber Band, which "
                                  "K22 does not restate")


class Limiter(_Effect):
    def __init__(self, threshold_db: float = -6.0, release_ms: float = 0.05):
        self.threshold_db, self.release_ms = threshold_db, release_ms

    def _run(self, x, sr):
        return _native.fx_limiter(x, sr, self.threshold_db, self.release_ms)


class Gain(_Effect):
    _stage = _native.FX_GAIN

    def __init__(self, gain_db: float = 0.0):
        self.gain_db = gain_db


class Distortion(_Effect):
    _stage = _native.FX_DISTORTION

    def __init__(self, drive_db: float = 25.0):
        self.drive_db = drive_db


class Chorus(_Effect):
    def __init__(self, rate_hz: float = 1.0, depth: float = 0.25, centre_delay_ms: float = 7.0, feedback: float = 0.0, mix: float = 0.5):
        self.rate_hz, self.depth, self.centre_delay_ms, self.feedback, self.mix = rate_hz, depth, centre_delay_ms, feedback, mix

    def _run(self, x, sr):
        return _native.fx_chorus(x, sr, self.rate_hz, self.depth, self.centre_delay_ms, self.feedback, self.mix)


class Bitcrush(_Effect):
    _stage = _native.FX_BITCRUSH

    def __init__(self, bit_depth: float = 8.0):
        self.bit_depth = bit_depth


class Clipping(_Effect):
    _stage = _native.FX_CLIPPING

    def __init__(self, threshold_db: float = 0.0):
        self.threshold_db = threshold_db


class Compressor(_Effect):
    def __init__(self, threshold_db: float = 0.0, ratio: float = 1.0, attack_ms: float = 1.0, release_ms: float = 100.0):
        self.threshold_db, self.ratio, self.attack_ms, self.release_ms = threshold_db, ratio, attack_ms, release_ms

    def _run(self, x, sr):
        return _native.fx_compressor(x, sr, self.threshold_db, self.ratio, self.attack_ms, self.release_ms)


class Delay(_Effect):
    def __init__(self, delay_seconds: float = 0.5, feedback: float = 0.0, mix: float = 0.5):
        self.delay_seconds, self.feedback, self.mix = delay_seconds, feedback, mix

    def _run(self, x, sr):
        return _native.fx_delay(x, sr, self.delay_seconds, self.feedback, self.mix)


_POINTWISE_KEYWORD = {_native.FX_GAIN: ("gain_db", "gain_db"), _native.FX_DISTORTION: ("drive_db", "drive_db"),
                      _native.FX_BITCRUSH: ("bit_depth", "bit_depth"), _native.FX_CLIPPING: ("clip_threshold_db", "threshold_db")}


class Pedalboard:
    """A list of effects run in order.  ``board(audio, sample_rate)``: a NumPy float array gives a NumPy float32 array (processed
    on ``device``, default the current one); a device tensor gives a float32 tensor on its device, enqueued on the current stream
    with no synchronisation and no host copy.  An empty board returns its input unchanged and launches nothing."""

    def __init__(self, plugins=None, device=None):
        self.plugins = list(plugins or [])
        self.device = device

    def append(self, plugin):
        self.plugins.append(plugin)

    def __len__(self):
        return len(self.plugins)

    def __repr__(self):
        return f"Pedalboard({self.plugins!r})"

    def launches(self):
        """The board as the launches it makes: an effect alone, or a run of pointwise effects that rvc_fx_pointwise_f32 applies in
        one pass -- neighbours whose stages come in its order gain, distortion, bitcrush, clipping."""
        groups = []
        for p in self.plugins:
            if not isinstance(p, _Effect):
                raise TypeError(f"Pedalboard: {p!r} is not an effect of rvc_amd.lib.effects")
            last = groups[-1] if groups else None
            if p._stage and last and last[-1]._stage and last[-1]._stage < p._stage:
                last.append(p)
            else:
                groups.append([p])
        return groups

    def _run(self, x: torch.Tensor, sr: int) -> torch.Tensor:
        for group in self.launches():
            if not group[0]._stage:
                x = group[0]._run(x, sr)
                continue
            kw = {_POINTWISE_KEYWORD[p._stage][0]: getattr(p, _POINTWISE_KEYWORD[p._stage][1]) for p in group}
            x = _native.fx_pointwise(x, sum(p._stage for p in group), **kw)
        return x

    def __call__(self, audio, sample_rate):
        if int(sample_rate) != sample_rate:
            raise ValueError(f"Pedalboard: sample_rate must be a whole number of Hz, got {sample_rate!r}")
        sr = int(sample_rate)
        if not self.plugins:
            return audio
        if torch.is_tensor(audio):
            if audio.dim() != 1:
                raise ValueError(f"Pedalboard: audio must be 1-D (mono), got shape {tuple(audio.shape)}")
            return self._run(audio.to(torch.float32), sr)
        audio = np.asarray(audio)
        if audio.ndim != 1:
            raise ValueError(f"Pedalboard: audio must be 1-D (mono), got shape {audio.shape}")
        if audio.dtype not in (np.float32, np.float64):
            raise ValueError(f"Pedalboard: audio must be float32 or float64, got {audio.dtype}")
        dev = _native._cuda_device(self.device)
        x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(dev)
        with torch.cuda.device(dev):
            return self._run(x, sr).cpu().numpy()
