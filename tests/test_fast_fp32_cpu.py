"""The C ABI of the opt-in fast-fp32 vocoder mode (K3h, csrc/convbf1.hip: fp32 taps and activations as error-corrected fp16 pairs) as far
as it can be shown without a device: the size query accepts exactly the documented shapes and returns the documented byte count, the
pack refuses taps an fp16 pair cannot hold BEFORE it touches the slab, and rvc_decoder_set_arithmetic refuses what its header comment
says it refuses.  Every refusal names its entry point in rvc_last_error()."""
import ctypes
import itertools

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()                                    # the library may not exist yet when this file runs alone
    from rvc_amd import _native
    return _native._lib


def _plant_other_error(lib):
    """Leave a known message of ANOTHER entry point in rvc_last_error(), so that a refusal has to write its own."""
    need = ctypes.c_size_t()
    assert lib.rvc_knn_workspace_bytes(100, 10, 768, 5, ctypes.byref(need)) != 0
    assert b"k must be 8" in lib.rvc_last_error()


def _refused(lib, name, rc):
    msg = lib.rvc_last_error()
    assert rc != 0, name
    assert msg.startswith(name.encode() + b": ") and len(msg) > len(name) + 2, (name, msg)
    return msg


def test_abi_version_is_unchanged(lib):
    assert lib.rvc_abi_version() == 4              # additions only


def test_f16x2_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    name = "rvc_conv1d_f16x2_weight_bytes"
    fn = getattr(lib, name)
    need = ctypes.c_size_t()
    n_yes = 0
    for c, k in itertools.product(range(-1, 1025), range(-1, 16)):
        want = c in (128, 256) and k in (3, 7, 11)
        if not want:
            _plant_other_error(lib)
        need.value = 0
        rc = fn(c, k, ctypes.byref(need))
        assert (rc == 0) == want, (c, k, lib.rvc_last_error())
        if want:
            # per (16 input channels, tap, 32 output channels): one 1 KiB fragment of w_hi and one of w_lo * 2^11
            assert need.value == (c // 16) * k * (c // 32) * 2048, (c, k, need.value)
            assert need.value == 4 * c * c * k       # = two fp16 per tap: the bytes of the fp32 tensor itself
            n_yes += 1
        else:
            _refused(lib, name, rc)
    assert n_yes == 6, n_yes
    _plant_other_error(lib)
    _refused(lib, name, fn(128, 3, None))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan"), 65504.0 * (1 + 2.0 ** -20), -1e6])
def test_f16x2_pack_refuses_taps_beyond_the_pair_before_touching_the_slab(lib, bad):
    name = "rvc_conv1d_f16x2_pack_weight"
    c, k = 128, 3
    w = (ctypes.c_float * (c * c * k))()
    w[c * c * k - 1] = bad                          # the last tap: the range check walks the whole tensor
    slab = ctypes.create_string_buffer(4 * c * c * k)   # a HOST buffer of the slab's size: nothing may be copied into it
    _plant_other_error(lib)
    msg = _refused(lib, name, lib.rvc_conv1d_f16x2_pack_weight(w, c, k, slab, None))
    assert b"65504" in msg
    assert slab.raw == bytes(len(slab))


def test_f16x2_pack_and_forward_refuse_bad_arguments(lib):
    w = (ctypes.c_float * (128 * 128 * 3))()
    slab = ctypes.create_string_buffer(16)
    for args in ((None, 128, 3, slab, None), (w, 128, 3, None, None), (w, 64, 3, slab, None), (w, 128, 5, slab, None)):
        _plant_other_error(lib)
        _refused(lib, "rvc_conv1d_f16x2_pack_weight", lib.rvc_conv1d_f16x2_pack_weight(*args))
    assert slab.raw == bytes(16)
    _plant_other_error(lib)
    _refused(lib, "rvc_conv1d_f16x2_forward",
             lib.rvc_conv1d_f16x2_forward(None, None, None, None, None, None, 1, 128, 64, 3, 1, 0.1, 1.0, None))


def _make_handle(lib, kind, weight_storage):
    from rvc_amd import _native
    cfg = _native.DecoderConfig()
    cfg.kind, cfg.sample_rate, cfg.in_channels, cfg.upsample_initial_channel, cfg.gin_channels = kind, 48000, 192, 512, 256
    cfg.n_ups = 4
    for i, (u, ks) in enumerate(zip((12, 10, 2, 2), (24, 20, 4, 4))):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, ks
    cfg.n_res_kernels = cfg.n_res_dilations = 3
    for i, (k, d) in enumerate(zip((3, 7, 11), (1, 3, 5))):
        cfg.res_kernel_sizes[i], cfg.res_dilations[i] = k, d
    cfg.weight_storage = weight_storage
    h = ctypes.c_void_p()
    assert lib.rvc_decoder_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, lib.rvc_last_error()
    return h


def test_decoder_set_arithmetic_refusals(lib):
    """A handle between create and finalize owns no device memory, so this runs without a GPU."""
    name = "rvc_decoder_set_arithmetic"
    _plant_other_error(lib)
    _refused(lib, name, lib.rvc_decoder_set_arithmetic(None, 1))
    h = _make_handle(lib, 0, 0)
    try:
        for mode in (2, -1, 3):
            _plant_other_error(lib)
            assert b"mode" in _refused(lib, name, lib.rvc_decoder_set_arithmetic(h, mode))
        assert lib.rvc_decoder_set_arithmetic(h, 1) == 0, lib.rvc_last_error()
        assert lib.rvc_decoder_set_arithmetic(h, 0) == 0, lib.rvc_last_error()
    finally:
        lib.rvc_decoder_destroy(h)
    h = _make_handle(lib, 1, 1)                     # MRF, bf16 weight storage: those taps already cost three products
    try:
        _plant_other_error(lib)
        assert b"weight_storage" in _refused(lib, name, lib.rvc_decoder_set_arithmetic(h, 1))
        assert lib.rvc_decoder_set_arithmetic(h, 0) == 0, lib.rvc_last_error()   # "exact" is what it runs anyway
    finally:
        lib.rvc_decoder_destroy(h)


def test_python_defaults_are_exact():
    from rvc_amd import _native
    import inspect
    assert inspect.signature(_native.Decoder.__init__).parameters["arithmetic"].default == "exact"
    assert _native.DEC_ARITHMETIC == {"exact": 0, "fp16x2": 1}
