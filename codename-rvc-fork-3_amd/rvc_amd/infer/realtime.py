"""Streaming (block-by-block) conversion: ``VoiceConverter.open_stream`` -> ``ConversionStream``.

The reference converts whole utterances only.  A stream keeps two pieces of state on the device between pushes: the last
``context + crossfade + search`` frames of 16 kHz input (``hist``), and the tail of the previous output (``buf``).  A push

1. builds ``window = [hist | block]`` and rolls ``hist`` (rvc_stream_window_f32, one launch),
2. runs the unchanged ``Pipeline.pipeline`` on the window, with the keywords ``convert_array`` hands it,
3. keeps the last ``B + X + S`` output samples and joins them to the previous block with SOLA (rvc_sola_f32, K21, two launches):
   slide to the lag of best normalised correlation with the saved tail, crossfade over X samples, save the next tail.

All lengths are whole 10 ms frames: 160 input samples, ``q = sr // 100`` output samples.  Nothing here synchronises: a device
tensor in gives a device tensor out on the current stream.  The float64 restatement of steps 1 and 3 is tests/sola_ref.py.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from rvc_amd import _native

FRAME_IN = 160          # one 10 ms frame of 16 kHz input
REFUSED = ("split_audio", "f0_file", "clean_audio", "formant_shifting", "post_process", "resample_sr")

_Event = torch.cuda.Event   # convert_audio_stream's timer (tests without a device replace it)


@dataclass(frozen=True)
class StreamPlan:
    """The frame arithmetic of one stream.  Input lengths are 16 kHz samples, output lengths samples at ``sr``."""
    sr: int
    q: int                # output samples per frame
    block_ms: int
    latency_ms: int       # algorithmic: block + crossfade + search
    block_samples: int    # input samples per push
    hist_samples: int     # carried input: context + crossfade + search frames
    window_samples: int   # what the pipeline converts per push
    block_out: int        # B: output samples per push
    xfade: int            # X
    search: int           # S
    n_infer: int          # B + X + S
    pipeline_out: int     # what Pipeline.pipeline returns for the window


def _frames(ms, name: str) -> int:
    if isinstance(ms, bool) or int(ms) != ms or ms < 0 or int(ms) % 10:
        raise ValueError(f"{name}={ms!r} must be a non-negative multiple of 10 ms (lengths are whole 10 ms frames)")
    return int(ms) // 10


def stream_plan(sr: int, block_ms=250, context_ms=1000, crossfade_ms=50, search_ms=10, x_pad: int = 1, x_max: int = 41) -> StreamPlan:
    """-> StreamPlan; ValueError for lengths a stream cannot have.  ``x_pad`` / ``x_max``: Config's seconds of reflect padding
    around, and the longest input of, one pipeline segment."""
    sr = int(sr)
    if sr < 100 or sr % 100:
        raise ValueError(f"the model's sample rate {sr} has no whole number of samples per 10 ms frame")
    q = sr // 100
    fb, fc, fx, fs = (_frames(v, n) for v, n in ((block_ms, "block_ms"), (context_ms, "context_ms"), (crossfade_ms, "crossfade_ms"),
                                                 (search_ms, "search_ms")))
    if fb < 1 or fx < 1:
        raise ValueError(f"block_ms={block_ms} and crossfade_ms={crossfade_ms} must be at least 10")
    if fx > fb:
        raise ValueError(f"crossfade_ms={crossfade_ms} is longer than block_ms={block_ms}")
    window = (fc + fx + fs + fb) * FRAME_IN
    if window + FRAME_IN > 16000 * x_max:
        raise ValueError(f"block + context + crossfade + search = {(fc + fx + fs + fb) * 10} ms does not fit one pipeline segment ({x_max} s)")
    # Pipeline.pipeline: reflect-pad by x_pad seconds, HuBERT's conv stack keeps (n - 400) // 320 + 1 frames of 20 ms, doubled;
    # the synthesizer makes sr // 100 samples per 10 ms frame and the pad is trimmed off again
    n = window + 2 * 16000 * x_pad
    p_len = min(n // FRAME_IN, 2 * ((n - 400) // 320 + 1))
    pipeline_out = p_len * q - 2 * sr * x_pad
    n_infer = (fb + fx + fs) * q
    if pipeline_out < n_infer:
        raise ValueError(f"context_ms={context_ms} is too short: the pipeline returns {pipeline_out} samples for the window, "
                         f"the join needs block + crossfade + search = {n_infer} (HuBERT drops up to 20 ms at the end)")
    return StreamPlan(sr=sr, q=q, block_ms=fb * 10, latency_ms=(fb + fx + fs) * 10, block_samples=fb * FRAME_IN,
                      hist_samples=(fc + fx + fs) * FRAME_IN, window_samples=window, block_out=fb * q, xfade=fx * q, search=fs * q,
                      n_infer=n_infer, pipeline_out=pipeline_out)


def fade_in_table(xfade: int) -> np.ndarray:
    """sin^2(pi i / (2 X)), i < X, evaluated in float64 and rounded to float32."""
    return (np.sin(np.pi * np.arange(xfade, dtype=np.float64) / (2.0 * xfade)) ** 2).astype(np.float32)


class ConversionStream:
    """One live conversion: ``push`` a block of ``block_samples`` 16 kHz samples, get ``block_out`` samples at ``sr`` that follow
    the previous push's seamlessly.  Open with ``VoiceConverter.open_stream``.

    The input is taken as it comes, expected in [-1, 1]: convert_array's peak limiting rescales a whole utterance and would change
    the gain from block to block here.  The output trails the input by ``latency_ms`` (block + crossfade + search) plus the 10 or
    20 ms HuBERT's framing drops at the end of a window.

    Device tensor in -> device tensor out, enqueued on the current stream without synchronising (f0_method "rmvpe" without
    f0_autotune; "fcpe" and autotune read the contour on the host).  NumPy float32 / float64 in -> NumPy float32 out.  With
    ``noise_seed=k`` push j draws its noise under seed k + j: two runs give identical bits.

    The streams of one converter share its model, its pipeline and their scratch memory: push them from one thread at a time, and
    push one stream on one HIP stream (or order the HIP streams yourself): the carried state is read and written by every push.
    ``debug = True`` keeps host copies of every push's ``infer``, the ``buf`` it met and the chosen offset in ``debug_log``
    (this synchronises)."""

    def __init__(self, converter, plan: StreamPlan, pipeline_kwargs: dict, noise_seed=None):
        self._vc, self.plan, self._kw = converter, plan, dict(pipeline_kwargs)
        self.noise_seed = None if noise_seed is None else int(noise_seed)
        self.sr, self.block_samples, self.block_out, self.latency_ms = plan.sr, plan.block_samples, plan.block_out, plan.latency_ms
        self.device = torch.device(converter.config.device)
        self._hist = torch.zeros(plan.hist_samples, dtype=torch.float32, device=self.device)
        self._buf = torch.zeros(plan.xfade, dtype=torch.float32, device=self.device)
        self._fade = torch.from_numpy(fade_in_table(plan.xfade)).to(self.device)
        self._offset = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.pushes = 0
        self.debug = False
        self.debug_log = []
        self.closed = False

    def _as_block(self, block) -> torch.Tensor:
        if torch.is_tensor(block):
            if block.dim() != 1 or block.shape[0] != self.block_samples:
                raise ValueError(f"a block is {self.block_samples} samples at 16 kHz, got a tensor of shape {tuple(block.shape)}")
            return block.to(device=self.device, dtype=torch.float32).contiguous()
        block = np.asarray(block)
        if block.dtype not in (np.float32, np.float64):
            raise ValueError(f"a block is float32 or float64, got {block.dtype}")
        if block.ndim != 1 or block.shape[0] != self.block_samples:
            raise ValueError(f"a block is {self.block_samples} samples at 16 kHz, got an array of shape {block.shape}")
        return torch.from_numpy(np.ascontiguousarray(block, dtype=np.float32)).to(self.device)

    def push(self, block):
        if self.closed:
            raise RuntimeError("push on a closed stream")
        as_numpy = not torch.is_tensor(block)
        block, vc, plan = self._as_block(block), self._vc, self.plan
        window = _native.stream_window(self._hist, block)
        vc.vc.trim_vocoder_pad = bool(vc.trim_vocoder_pad)
        seed = None if self.noise_seed is None else self.noise_seed + self.pushes
        y = vc.vc.pipeline(model=vc.hubert_model, net_g=vc.net_g, audio=window, pitch_guidance=vc.use_f0, version=vc.version,
                           f0_file=None, noise_seed=seed, **self._kw)
        if y.dim() != 1 or y.shape[0] != plan.pipeline_out:
            raise RuntimeError(f"the pipeline returned {tuple(y.shape)} samples for a window of {plan.window_samples}; the stream's "
                               f"frame arithmetic expects {plan.pipeline_out}")
        infer = y[plan.pipeline_out - plan.n_infer:].float().contiguous()
        if self.debug:
            entry = {"infer": infer.cpu().numpy().copy(), "buf": self._buf.cpu().numpy().copy()}   # buf is overwritten below
        out, _ = _native.sola(infer, self._buf, self._fade, plan.search, plan.block_out, offset=self._offset)
        if self.debug:
            entry["offset"] = self.last_offset()
            self.debug_log.append(entry)
        self.pushes += 1
        return out.cpu().numpy() if as_numpy else out

    def last_offset(self) -> int:
        """The lag the last push chose, in output samples (debugging: reads the device, so it synchronises)."""
        return int(self._offset.item())

    def reset(self) -> None:
        """Forget the carried input and the saved tail, and restart the noise seeds: the next push is a first push."""
        self._hist.zero_()
        self._buf.zero_()
        self._offset.zero_()
        self.pushes = 0
        self.debug_log = []

    def close(self) -> None:
        if not self.closed:
            self.closed = True
            self._vc._streams.discard(self)
            self._hist = self._buf = self._fade = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_stream(converter, model_path=None, index_path: str = "", block_ms=250, context_ms=1000, crossfade_ms=50, search_ms=10,
                pitch: int = 0, f0_method: str = "rmvpe", index_rate: float = 0.75, protect: float = 0.5, filter_radius: float = 3.0,
                sid: int = 0, volume_envelope: float = 1, hop_length: int = 128, f0_autotune: bool = False,
                f0_autotune_strength: float = 1, noise_seed=None, embedder_model: str = "contentvec",
                embedder_model_custom: str = None, **refused) -> ConversionStream:
    """What ``VoiceConverter.open_stream`` runs (its docstring has the arguments)."""
    for name, value in refused.items():
        if name not in REFUSED:
            raise TypeError(f"open_stream() got an unexpected keyword argument {name!r}")
        if value:
            raise NotImplementedError(f"{name} works on a whole utterance and is not available on a stream")
    if model_path:
        converter.get_vc(model_path, sid)      # refuses another model while streams are open
    if converter.vc is None or converter.net_g is None:
        raise RuntimeError("open_stream: no model is loaded (pass model_path, or load a checkpoint first)")
    plan = stream_plan(converter.tgt_sr, block_ms, context_ms, crossfade_ms, search_ms, x_pad=converter.vc.x_pad, x_max=converter.vc.x_max)
    if not converter.hubert_model or (model_path and embedder_model != converter.last_embedder_model):
        converter.load_hubert(embedder_model, embedder_model_custom)
        converter.last_embedder_model = embedder_model
    file_index = index_path.strip().strip('"').strip("\n").strip('"').strip().replace("trained", "added")
    kw = dict(sid=sid, pitch=pitch, f0_method=f0_method, file_index=file_index, index_rate=index_rate, filter_radius=filter_radius,
              volume_envelope=volume_envelope, protect=protect, hop_length=hop_length, f0_autotune=f0_autotune,
              f0_autotune_strength=f0_autotune_strength)
    stream = ConversionStream(converter, plan, kw, noise_seed=noise_seed)
    converter.__dict__.setdefault("_streams", set()).add(stream)
    return stream


def convert_audio_stream(converter, audio_input_path: str, audio_output_path: str, model_path=None, index_path: str = "", **kwargs) -> dict:
    """What ``VoiceConverter.convert_audio_stream`` runs (its docstring has the arguments)."""
    from rvc_amd.infer.infer import _write_wav, load_audio_infer
    audio = np.asarray(load_audio_infer(audio_input_path, 16000, device=converter.config.device), dtype=np.float32)
    with open_stream(converter, model_path, index_path, **kwargs) as stream:
        n_blocks = max(1, -(-audio.shape[0] // stream.block_samples))
        padded = np.zeros(n_blocks * stream.block_samples, dtype=np.float32)
        padded[:audio.shape[0]] = audio
        padded = torch.from_numpy(padded).to(stream.device)
        outs, events = [], []
        for j in range(n_blocks):
            start, end = _Event(enable_timing=True), _Event(enable_timing=True)
            start.record()
            outs.append(stream.push(padded[j * stream.block_samples:(j + 1) * stream.block_samples]))
            end.record()
            events.append((start, end))
        out = torch.cat(outs)[:audio.shape[0] * stream.sr // 16000].cpu().numpy()      # the copy waits for every push
        push_ms = [float(start.elapsed_time(end)) for start, end in events]
        _write_wav(audio_output_path, out, stream.sr)
        return {"blocks": n_blocks, "block_ms": stream.plan.block_ms, "push_ms": push_ms, "median_ms": float(np.median(push_ms)),
                "max_ms": float(max(push_ms))}
