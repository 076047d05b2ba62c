"""One process, two devices: every launcher whose one-time GPU resource (a kernel's dynamic-LDS limit, the built-in log-mel
tables, the CU count) the library keeps per device (csrc/common.h: reserve_lds; logmel.hip) gives on cuda:1 what it gives on
cuda:0, bit for bit -- first one device after the other, then from two host threads started together, one per device, the way
train/extract/extract.py drives several GPUs.  The devices are identical and the kernels deterministic (the kNN result does not
depend on the regime or on the order its candidates were found in), so the gate is equality; a device that was handed the other's
table pointers, or that never got a kernel's LDS attribute, shows as a refused launch or as different numbers.

Weights are packed per device; the inputs are built once on the host and never modified."""
import concurrent.futures
import threading

import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two HIP devices in one process (this machine shows fewer)")]


@pytest.fixture(scope="module")
def native():
    from rvc_amd import _native
    return _native


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _logmel(native, dev, host):
    mel, t = native.logmel_rmvpe(host["audio"].to(dev))
    return [mel, torch.tensor([t])]


def _attention(native, dev, host):       # head size 64, no relative embeddings: K7b
    return [native.attention_qkv(host["qkv"].to(dev), 2, 64 ** -0.5)]


def _gemmbf(native, dev, host):
    x, w = host["gemmbf"]
    return [native.conv1d_bf16x3(x.to(dev), native.gemm_bf16x3_pack_weight(w, dev), None, w.shape[0], w.shape[2])]


def _conv2d(native, dev, host):          # K10
    x, w, b, res = host["conv2d"]
    return [native.conv2d_forward(x.to(dev), native.conv2d_pack_weight(w, dev), b.to(dev), w.shape[0], 3, relu=True, res=res.to(dev))]


def _conv1d(forward, pack, key, dil):
    def run(native, dev, host):
        x, w, b = host[key]
        c, _, k = w.shape
        direct = native.conv1d_forward(x.to(dev), native.conv1d_pack_weight(w, dev), b.to(dev), c, k, dil, 0.1)   # its repack is host-side now, too
        return [getattr(native, forward)(x.to(dev), getattr(native, pack)(w, dev), b.to(dev), c, k, dil, 0.1), direct]
    return run


def _knn(native, dev, host):
    big, small768, q = host["knn"]
    index = big.to(dev)
    aux = native.knn_index_build(index)
    out = []
    out += native.knn_search(index, aux, q[:33].to(dev))             # <= 64 queries: streaming (knn_direct_kernel, dim 256)
    out += native.knn_search(index, aux, q.to(dev))                  # > 64 queries, 16 384 rows, dim 256: screened
    few = index[:3000].contiguous()
    out += native.knn_search(few, native.knn_index_build(few), q.to(dev))       # a small index: fp32 GEMM
    wide = small768.to(dev)                                          # streaming again at dim 768: knn_direct_kernel asks for MORE LDS than before
    out += native.knn_search(wide, native.knn_index_build(wide), small768[:5].to(dev) + 0.01)
    return out


def _decoder(native, dev, host):
    """NSF vocoder on a few frames with explicit noise; the caller holds resblock_bf16x3_set_enabled(False), so the handle built here
    runs its 32-channel 3-tap layers on the fused fp32 kernel (K3b, resblock.hip) and the rest on wino / winobf / winobf2."""
    folded, z, f0, g, src_randn = host["decoder"]
    dec = native.Decoder("HiFi-GAN", 48000, folded)
    return [dec.forward(z.to(dev), f0.to(dev), g.to(dev), src_randn=src_randn.to(dev), src_rand=torch.zeros(1, 1, device=dev))]


CASES = {
    "logmel_rmvpe": _logmel,
    "attention_qkv_hd64": _attention,
    "conv1d_bf16x3": _gemmbf,
    "conv2d_forward": _conv2d,
    "wino_c32_k3": _conv1d("conv1d_wino_forward", "conv1d_wino_pack_weight", "c32k3", 1),
    "winobf_c64_k7": _conv1d("conv1d_winobf_forward", "conv1d_winobf_pack_weight", "c64k7", 3),       # K3x
    "winobf_c128_k3": _conv1d("conv1d_winobf_forward", "conv1d_winobf_pack_weight", "c128k3", 5),     # K3y
    "winobf_c128_k11": _conv1d("conv1d_winobf_forward", "conv1d_winobf_pack_weight", "c128k11", 3),   # K3y
    "knn_search": _knn,
    "decoder_nsf_k3f_off": _decoder,
}


def _host_inputs():
    from rvc_amd.lib import synthetic as S
    from rvc_amd.lib.algorithm.weights import fold_weight_norm
    conv = lambda seed, c, k, length: (_randn(seed, 1, c, length), _randn(seed + 1, c, c, k) / (c * k) ** 0.5, _randn(seed + 2, c))
    cpt = S.make_synth_checkpoint(48000, "HiFi-GAN", seed=0)
    folded = {k[4:]: v for k, v in fold_weight_norm(cpt["weight"]).items() if k.startswith("dec.")}
    T = 32
    big = _randn(40, 16384, 256) * 0.4
    q = big[torch.randint(0, 16384, (129,), generator=torch.Generator().manual_seed(41))] + 0.02 * _randn(42, 129, 256)
    return {
        "audio": torch.from_numpy(S.synth_audio(16000, seed=3)).float()[None],                 # one second
        "qkv": _randn(10, 1, 31, 3 * 2 * 64) * 1.5,
        "gemmbf": (_randn(20, 1, 64, 300), _randn(21, 128, 64, 3) / (64 * 3) ** 0.5),
        "conv2d": (_randn(30, 1, 16, 9, 128), _randn(31, 16, 16, 3, 3) / 12.0, _randn(32, 16), _randn(33, 1, 16, 9, 128)),
        "c32k3": conv(50, 32, 3, 1000), "c64k7": conv(60, 64, 7, 700), "c128k3": conv(70, 128, 3, 31), "c128k11": conv(80, 128, 11, 513),
        "knn": (big, _randn(43, 100, 768) * 0.4, q.contiguous()),
        "decoder": (folded, _randn(90, 1, 192, T), torch.full((1, T), 220.0), _randn(91, 1, 256), _randn(92, 1, T * 480, 1)),
    }


def _run_all(native, device, host, start=None):
    """Every case on `device`, which is made current on the calling thread; results come back on the host."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        if start is not None:
            start.wait(timeout=120)          # (a thread that failed before this point breaks the barrier instead of hanging the other)
        out = {name: [t.cpu() for t in case(native, dev, host)] for name, case in CASES.items()}
        torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def runs(native):
    host = _host_inputs()
    native.resblock_bf16x3_set_enabled(False)        # process-wide: the decoder handles of BOTH phases are built while it is off
    try:
        first = _run_all(native, "cuda:0", host)
        second = _run_all(native, "cuda:1", host)
        start = threading.Barrier(2)
        with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:      # one host thread per device, started together
            tasks = [pool.submit(_run_all, native, d, host, start) for d in ("cuda:0", "cuda:1")]
            threaded = [t.result() for t in tasks]
    finally:
        native.resblock_bf16x3_set_enabled(True)
    return first, second, threaded


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CASES))
def test_second_device_equals_first(runs, name):
    first, second, _ = runs
    assert all(torch.isfinite(t).all() for t in first[name] if t.is_floating_point())
    assert _same(second[name], first[name])


@pytest.mark.parametrize("name", list(CASES))
def test_one_thread_per_device_equals_sequential(runs, name):
    first, _, threaded = runs
    assert _same(threaded[0][name], first[name])
    assert _same(threaded[1][name], first[name])
