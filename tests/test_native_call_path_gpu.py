"""The device and stream contract of rvc_amd._native, checked without launching one of the library's kernels.

Every wrapper reaches an entry point that takes a `void *stream` through `_native._call`, which must make the device of the call's
tensors current (csrc/common.h: the library looks its per-device resources up by hipGetDevice) and pass that device's current
stream.  Here `_native._lib` is swapped for a stand-in: a symbol whose prototype in include/rvc_amd.h ends in `void *stream)` is
NOT executed -- the stand-in notes (symbol, torch.cuda.current_device() at the time of the call, the stream argument) and returns
0 -- so a binding that is wrong cannot misdirect a kernel; every other symbol (size queries, _supported, _frames, _warmup,
setters, create, finalize, destroy) goes through to the real library.  The wrappers' outputs are therefore uninitialised and are
never looked at, and the tensors are the smallest each wrapper's own checks accept.

A wrapper added later without an entry in CASES leaves its symbol unrecorded and fails test_every_stream_symbol_is_driven."""
import os
import re

import numpy as np
import pytest
import torch
from scipy import signal

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rvc_amd.h")
two_devices = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two HIP devices in one process")

# Stream-taking entry points that no case drives: rvc_index_broadcast is a collective over the job's RCCL communicator, which
# exists only between the ranks of a multi-process job (rvc_comm_create); infer/distributed.py makes each rank's device current
# process-wide.
EXCLUDED = {"rvc_index_broadcast"}
PASSED_THROUGH_ON_DEVICE = ("rvc_decoder_finalize", "rvc_mel_create")      # allocate and upload on the current device, no stream


def _stream_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = re.findall(r"\bint\s+(rvc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return {name for name, args in protos if " ".join(args.split()).endswith("void *stream")}


STREAM_SYMBOLS = _stream_symbols()


class Recorder:
    """Stands in for the ctypes library: notes the stream-taking calls instead of making them."""

    def __init__(self, real):
        self._real = real
        self.calls = []          # (symbol, current device, stream argument)
        self.passed = []         # (symbol, current device) of PASSED_THROUGH_ON_DEVICE

    def __getattr__(self, name):
        if name in STREAM_SYMBOLS:
            def record(*args):
                self.calls.append((name, torch.cuda.current_device(), args[-1]))
                return 0
            return record
        if name == "rvc_comm_create":
            raise AssertionError("no test here may create a communicator")
        fn = getattr(self._real, name)
        if name in PASSED_THROUGH_ON_DEVICE:
            def through(*args):
                self.passed.append((name, torch.cuda.current_device()))
                return fn(*args)
            return through
        return fn


@pytest.fixture(scope="module")
def native():
    from rvc_amd import _native
    return _native


@pytest.fixture()
def rec(native, monkeypatch):
    r = Recorder(native._lib)
    monkeypatch.setattr(native, "_lib", r)
    return r


@pytest.fixture(scope="module")
def folded():
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0)
    return {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}


def _mel(N, dev):
    return N.MelTransform(64, 16, 64, 24, np.zeros((2, 33), dtype=np.float32), device=dev)


# ---- the case table: every public wrapper once, on tensors of `dev` -------------------------------------------------------------
BUTTER = tuple(c.tolist() for c in signal.butter(5, 0.1, "high"))                     # (b[6], a[6]) with a[0] == 1
T = 4                                                                                  # decoder frames


def _e(dev, *shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=dev)


def _knn(N, dev, h):
    index, aux, q = _e(dev, 4, 256), _e(dev, 16, dtype=torch.uint8), _e(dev, 2, 256)
    N.knn_index_build(index)
    N.knn_search(index, aux, q)
    N.knn_rank_candidates(index, aux, q, _e(dev, 2, 4, dtype=torch.int32))
    N.knn_blend(index, q, _e(dev, 2, 8), _e(dev, 2, 8, dtype=torch.int64), 0.5)


def _kmeans(N, dev, h):
    x, cent = _e(dev, 4, 256), _e(dev, 2, 256)
    N.kmeans_assign(x, cent)
    N.kmeans_update(x, _e(dev, 4, dtype=torch.int32), _e(dev, 3, dtype=torch.int64), cent)


def _front(N, dev, h):
    N.logmel_rmvpe(_e(dev, 1, 1600))
    h["mel"].forward(_e(dev, 1, 64), want_mel=True, want_spec=True)
    x = _e(dev, 64, dtype=torch.float64)
    fir = _e(dev, 5, dtype=torch.float64)
    N.resample_poly(x, 1, 2, fir)
    N.filtfilt_order5(x, *BUTTER)
    N.lfilter_order5(x, *BUTTER)
    N.frame_rms(x, 8, 4)
    N.slice_export(x, [(0, 8), (8, 24)], 1, 3, fir)
    N.checksum64(x)


def _rmvpe(N, dev, h):
    N.bigru_forward(_e(dev, 1, 2, 2, 768), _e(dev, 2, 256, 768), _e(dev, 2, 768))
    N.bigru_redone(1, dev)
    x = _e(dev, 1, 2, 4)
    N.bias_relu_add_(x, _e(dev, 2), _e(dev, 1, 2, 4))
    N.rownorm_gelu_(x, _e(dev, 2), _e(dev, 2))
    N.gate_tanh_sigmoid(x)
    x2 = _e(dev, 1, 16, 4, 4)
    N.conv2d_forward(x2, N.conv2d_pack_weight(torch.zeros(16, 16, 3, 3), dev), _e(dev, 16), 16, 3)
    N.conv2d_bf16x3_forward(x2, N.conv2d_bf16x3_pack_weight(torch.zeros(32, 16, 3, 3), dev), _e(dev, 32), 32)


def _attention(N, dev, h):
    N.attention_qkv(_e(dev, 1, 4, 3 * 2 * 64), 2, 0.125, _e(dev, 21, 64), _e(dev, 21, 64))


def _vocoder_convs(N, dev, h):
    x, b = _e(dev, 1, 64, 8), _e(dev, 64)
    w = torch.zeros(64, 64, 7)
    N.conv1d_forward(x, N.conv1d_pack_weight(w, dev), b, 64, 7)
    N.conv1d_forward_into(x, _e(dev, w.numel()), b, 64, 7, out=_e(dev, 1, 64, 8))
    N.conv1d_wino_forward(x, N.conv1d_wino_pack_weight(w, dev), b, 64, 7)
    N.conv1d_winobf_forward(x, N.conv1d_winobf_pack_weight(w, dev), b, 64, 7)
    w3 = torch.zeros(64, 64, 3)
    for taps in (False, True):
        N.resblock_bf16x3_forward(x, N.resblock_bf16x3_pack_weight(w3, w3, dev, bf16_taps=taps), b, b, 3, bf16_taps=taps)
    x128, b128, w128 = _e(dev, 1, 128, 8), _e(dev, 128), torch.zeros(128, 128, 3)
    N.conv1d_bf16w_forward(x128, N.conv1d_bf16w_pack_weight(w128, dev), b128, 3)
    N.conv1d_f16x2_forward(x128, N.conv1d_f16x2_pack_weight(w128, dev), b128, 3)
    packed = N.upsample_bf16x3_pack_weight(torch.zeros(64, 32, 4), None, torch.zeros(32), 2, 1, dev)
    N.upsample_bf16x3_forward(x, None, packed, 32, 2, 4, 1)


def _hubert(N, dev, h):
    a = N.gemm_bf16x3_pack_weight(torch.zeros(128, 64), dev)
    x = _e(dev, 4, 64)
    N.linear_bf16x3(x, a, _e(dev, 128), 128, res=_e(dev, 4, 128))
    N.conv1d_bf16x3(_e(dev, 1, 64, 8), N.gemm_bf16x3_pack_weight(torch.zeros(128, 64, 3), dev), None, 128, 3)
    xs = N.split_rows_bf16x3(x)
    N.linear_bf16x3_presplit(xs, a, None, 4, 128)
    N.bias_residual_layernorm_bf16x3(_e(dev, 1, 4, 128), None, None, None, None, 1e-5)
    ys, frames = N.hubert_conv0_frames_bf16x3(_e(dev, 100), _e(dev, 64, 1, 10), _e(dev, 64), _e(dev, 64), 1e-5)
    N.conv1d_frames_bf16x3(ys, frames, N.gemm_bf16x3_pack_weight(torch.zeros(128, 3 * 64), dev), None, 128, 3, 2)
    N.posconv_gelu_bf16x3(_e(dev, 4, 48), N.posconv_bf16x3_pack_weight(torch.zeros(48, 48, 2), 1, dev), None, 1, 2, 1)


def _fcpe(N, dev, h):
    N.glu_dwconv_silu(_e(dev, 4, 128), _e(dev, 64, 3), _e(dev, 64))
    N.layernorm_rows(_e(dev, 4, 64), _e(dev, 64), _e(dev, 64))
    N.groupnorm_lrelu(_e(dev, 64, 8), _e(dev, 64), _e(dev, 64), 4)
    N.fcpe_decode(_e(dev, 4, 16), _e(dev, 16), 16, 0.05, 32.7, want_latent=True)


def _decoder(N, dev, h):
    args = (_e(dev, 1, 192, T), _e(dev, 1, T), _e(dev, 1, 256))
    noise = dict(src_randn=_e(dev, 1, T * h["dec"].upp, 1), src_rand=_e(dev, 1, 1))
    h["dec"].forward(*args, **noise)
    h["dec"].forward(*args, **noise, keep=(1, 3))


CASES = {"knn": _knn, "kmeans": _kmeans, "front": _front, "rmvpe": _rmvpe, "attention": _attention, "vocoder_convs": _vocoder_convs,
         "hubert": _hubert, "fcpe": _fcpe, "decoder": _decoder}


def _drive(N, rec, dev, folded, expect_stream=None):
    """The whole table on tensors of `dev`; every recorded call must have had `dev` current and carry its current stream, and the
    device that was current before a case is current after it.  -> the set of symbols recorded."""
    dev = torch.device(dev)
    before = torch.cuda.current_device()
    handles = {"mel": _mel(N, dev), "dec": N.Decoder("HiFi-GAN", 48000, folded, device=dev)}
    assert torch.cuda.current_device() == before
    assert handles["mel"].device == dev and handles["dec"].device == dev
    want = torch.cuda.current_stream(dev).cuda_stream
    if expect_stream is not None:
        assert want == expect_stream.cuda_stream
    for name, case in CASES.items():
        first = len(rec.calls)
        case(N, dev, handles)
        assert torch.cuda.current_device() == before, name
        assert len(rec.calls) > first, name
        for symbol, device, stream in rec.calls[first:]:
            assert device == dev.index, (name, symbol, device)
            assert stream == want, (name, symbol, stream, want)
    return {symbol for symbol, _, _ in rec.calls}


def test_every_stream_symbol_is_driven(native, rec, folded):
    """(a) today's usage: the tensors' device is current.  Also the completeness gate of the table."""
    assert len(STREAM_SYMBOLS) >= 57 and EXCLUDED <= STREAM_SYMBOLS
    with torch.cuda.device(0):
        seen = _drive(native, rec, "cuda:0", folded)
    assert seen == STREAM_SYMBOLS - EXCLUDED, sorted((STREAM_SYMBOLS - EXCLUDED) ^ seen)


def test_side_stream_is_the_stream_passed(native, rec, folded):
    """(b) inside torch.cuda.stream(s): every call carries s."""
    side = torch.cuda.Stream(0)
    assert side.cuda_stream != torch.cuda.default_stream(0).cuda_stream
    with torch.cuda.device(0), torch.cuda.stream(side):
        _drive(native, rec, "cuda:0", folded, expect_stream=side)


@two_devices
def test_tensors_of_another_device_than_the_current_one(native, rec, folded):
    """(c) tensors on cuda:1 while cuda:0 is current: device 1 during every call, its current stream passed, device 0 afterwards;
    the handles' finalize / create, which go through to the library, run with device 1 current, too."""
    side = torch.cuda.Stream(1)
    with torch.cuda.device(1):                # a side stream as device 1's current one (torch.cuda.stream(side) would also make
        default = torch.cuda.current_stream()  # device 1 current): the stream handle alone then tells the two devices apart
        torch.cuda.set_stream(side)
    try:
        with torch.cuda.device(0):
            assert torch.cuda.current_stream(0).cuda_stream != side.cuda_stream
            _drive(native, rec, "cuda:1", folded, expect_stream=side)
            assert torch.cuda.current_device() == 0
    finally:
        with torch.cuda.device(1):
            torch.cuda.set_stream(default)
    assert sorted(rec.passed) == [(name, 1) for name in sorted(PASSED_THROUGH_ON_DEVICE)]


@two_devices
def test_tensors_on_two_devices_are_refused(native, rec):
    N = native
    x0, x1 = _e("cuda:0", 2, 256), _e("cuda:1", 2, 256)
    with pytest.raises(N.NativeError, match=r"cuda:0.*cuda:1"):
        N.knn_blend(x0, x1, _e("cuda:1", 2, 8), _e("cuda:1", 2, 8, dtype=torch.int64), 0.5)
    with pytest.raises(N.NativeError, match=r"cuda:1.*cuda:0"):
        N.conv1d_forward(_e("cuda:1", 1, 64, 8), _e("cuda:0", 64 * 64 * 7), None, 64, 7)
    with pytest.raises(N.NativeError, match=r"cuda:0.*cuda:1"):
        N.bias_relu_add_(_e("cuda:0", 1, 2, 4), _e("cuda:1", 2))
    with pytest.raises(N.NativeError, match=r"cuda:0.*cuda:1"):
        N.resample_poly(_e("cuda:0", 8, dtype=torch.float64), 1, 2, _e("cuda:1", 5, dtype=torch.float64))
    assert rec.calls == []


@two_devices
def test_a_handle_refuses_tensors_of_another_device(native, rec, folded):
    N = native
    mel, dec = _mel(N, "cuda:1"), N.Decoder("HiFi-GAN", 48000, folded, device="cuda:0")
    with pytest.raises(N.NativeError, match=r"cuda:1.*cuda:0"):
        mel.forward(_e("cuda:0", 1, 64))
    with pytest.raises(N.NativeError, match=r"cuda:0.*cuda:1"):
        dec.forward(_e("cuda:1", 1, 192, T), _e("cuda:1", 1, T), _e("cuda:1", 1, 256), src_randn=_e("cuda:1", 1, T * dec.upp, 1))
    assert rec.calls == []


FORMER_ASSERTS = {                        # one input per validation that used to be an `assert` (gone under python -O)
    "attention_qkv: qkv not 3-D": lambda N, d: N.attention_qkv(_e(d, 4, 384), 2, 0.125),
    "attention_qkv: embedding shape": lambda N, d: N.attention_qkv(_e(d, 1, 4, 384), 2, 0.125, _e(d, 21, 32), _e(d, 21, 32)),
    "bias_relu_add_: x not 3-D": lambda N, d: N.bias_relu_add_(_e(d, 2, 4)),
    "bias_relu_add_: res of another shape": lambda N, d: N.bias_relu_add_(_e(d, 1, 2, 4), None, _e(d, 1, 2, 8)),
    "rownorm_gelu_: not contiguous": lambda N, d: N.rownorm_gelu_(_e(d, 1, 4, 2).transpose(1, 2)),
    "gate_tanh_sigmoid: odd channel count": lambda N, d: N.gate_tanh_sigmoid(_e(d, 1, 3, 4)),
    "linear_bf16x3: res of another shape": lambda N, d: N.linear_bf16x3(_e(d, 4, 64), _e(d, 8, dtype=torch.int16), None, 128, res=_e(d, 4, 64)),
    "filtfilt_order5: a[0] != 1": lambda N, d: N.filtfilt_order5(_e(d, 64, dtype=torch.float64), BUTTER[0], [2.0] + BUTTER[1][1:]),
    "Comm: id of the wrong length": lambda N, d: N.Comm(b"short", 1, 0),
}


@pytest.mark.parametrize("what", list(FORMER_ASSERTS))
def test_former_asserts_raise_native_error(native, rec, what):
    with pytest.raises(native.NativeError):
        FORMER_ASSERTS[what](native, "cuda:0")
    assert rec.calls == []
