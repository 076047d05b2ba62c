"""The shape contract of the bf16 matrix-core kernels at the C ABI (include/rvc_amd.h) -- the vocoder's convs (K3u / K3f / K3d / K3y) and the
HuBERT side (K11 GEMM slab, K14 positional conv, K7 attention workspace, K13 first-layer workspace): every `rvc_*_weight_bytes` /
`_workspace_bytes` size query accepts EXACTLY the shapes its header comment documents -- the shapes its forward has a kernel for -- and
every refusal says why in rvc_last_error().  pack_weight asks the same query first, so what it accepts is pinned with it.  Size queries
only, no device: a clean CPU checkout catches a predicate that drifts (K3u's once accepted rates 8 / 10 / 12 at 64-row tiles, which
have no kernel; the attention and K13 workspace queries once accepted any positive head_dim / channel count)."""
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


def _check_grid(lib, name, grid, documented, value=None):
    """Call `name`(*args, &bytes) over `grid`; accepted <=> documented(*args); a refusal leaves a message naming `name`; where `value` is
    given, an accepted call returns exactly value(*args) bytes."""
    fn = getattr(lib, name)
    need = ctypes.c_size_t()
    n_yes = n_no = 0
    for args in grid:
        want = documented(*args)
        if not want:
            _plant_other_error(lib)
        need.value = 0
        rc = fn(*args, ctypes.byref(need))
        assert (rc == 0) == want, (name, args, "accepted" if rc == 0 else "refused", lib.rvc_last_error())
        if want:
            assert need.value > 0, (name, args)
            if value is not None:
                assert need.value == value(*args), (name, args, need.value, value(*args))
            n_yes += 1
        else:
            msg = lib.rvc_last_error()
            assert msg.startswith(name.encode() + b": ") and len(msg) > len(name) + 2, (name, args, msg)
            n_no += 1
    return n_yes, n_no


# ---- K3u: rvc_upsample_bf16x3_weight_bytes(c_in, c_out, rate, ksize, nc_k, nc_stride) -----------------------------------------------
def _upsample_documented(c_in, c_out, rate, ksize, nc_k, nc_stride):
    if nc_k < 0 or (nc_k > 0 and nc_stride < 1):
        return False
    vk = (rate - 1) * nc_stride + nc_k if nc_k > 0 else 0          # folded noise rows; the row of ones makes vk + 1 <= 64
    return (rate in (2, 8, 10, 12) and c_in > 0 and c_in % 64 == 0 and c_out >= 1 and rate <= ksize <= 2 * rate and vk <= 63
            and (rate == 2 or rate * c_out >= 128))                # rates 8 / 10 / 12 have no 64-row (MB = 64) instantiation


UPS_C_IN = sorted(set(range(0, 1025, 32)) | {-64, 1, 63, 65, 127, 1023})
UPS_C_OUT = [-1, 0, 1, 2, 6, 7, 10, 11, 12, 13, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, 160, 256, 257, 512]


def test_upsample_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    # without a noise conv: every rate 1-16, c_in 0-1024, c_out on both sides of each rate's 128-row threshold, every ksize around [rate, 2 rate]
    grid = [(c_in, c_out, rate, ksize, 0, 1) for rate in range(1, 17) for c_in in UPS_C_IN for c_out in UPS_C_OUT
            for ksize in range(rate - 2, 2 * rate + 3)]
    n_yes, n_no = _check_grid(lib, "rvc_upsample_bf16x3_weight_bytes", grid, _upsample_documented)
    assert n_yes >= 500 and n_no >= 10 * n_yes, (n_yes, n_no)
    # with one: nc_k and nc_stride around vk = (rate - 1) nc_stride + nc_k = 63, and the arguments no noise conv can have
    grid = [(64, c_out, rate, ksize, nc_k, nc_stride) for rate in range(1, 17) for c_out in (13, 16, 64) for ksize in (rate, 2 * rate)
            for nc_k in range(-1, 66) for nc_stride in (-1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 32)]
    n_yes, n_no = _check_grid(lib, "rvc_upsample_bf16x3_weight_bytes", grid, _upsample_documented)
    assert n_yes >= 1000 and n_no >= n_yes, (n_yes, n_no)


def test_upsample_every_instantiation_is_reachable_and_nothing_else(lib):
    """The nine (rate, MB) kernels of launch_upsbf at their c_out boundaries, and the 64-row shapes of rates 8 / 10 / 12 refused by
    weight_bytes AND pack_weight (before: accepted by both, then "no instantiation" from the forward)."""
    need = ctypes.c_size_t()
    f = lib.rvc_upsample_bf16x3_weight_bytes
    for rate, c_out_lo in ((2, 1), (8, 16), (10, 13), (12, 11)):
        assert f(64, c_out_lo, rate, 2 * rate, 0, 1, ctypes.byref(need)) == 0, (rate, c_out_lo, lib.rvc_last_error())
        if rate != 2:
            _plant_other_error(lib)
            assert f(64, c_out_lo - 1, rate, 2 * rate, 0, 1, ctypes.byref(need)) != 0, (rate, c_out_lo - 1)
            assert b"rate * c_out >= 128" in lib.rvc_last_error()
    # MB = 64 / 128 / 256 for rate 2: 63 / 64 / 128 output channels
    for c_out in (63, 64, 127, 128, 160):
        assert f(64, c_out, 2, 4, 0, 1, ctypes.byref(need)) == 0
    _plant_other_error(lib)
    assert f(64, 8, 12, 24, 0, 1, ctypes.byref(need)) != 0                 # 96 GEMM rows at rate 12
    assert lib.rvc_last_error().startswith(b"rvc_upsample_bf16x3_weight_bytes: unsupported shape")
    w = (ctypes.c_float * (64 * 8 * 24))()
    slab = ctypes.create_string_buffer(1 << 18)        # a host buffer larger than any slab of this shape: nothing may be copied into it
    _plant_other_error(lib)
    assert lib.rvc_upsample_bf16x3_pack_weight(w, None, None, 64, 8, 12, 24, 0, 1, slab, None) != 0
    assert lib.rvc_last_error().startswith(b"rvc_upsample_bf16x3_weight_bytes: unsupported shape")
    assert slab.raw == bytes(len(slab))


# ---- K3f: rvc_resblock_bf16x3_weight_bytes / rvc_resblock_bf16w_weight_bytes(c, k) ----------------------------------------------------
def _resblock_documented(c, k):
    return (c in (32, 64) and k in (3, 7, 11)) or (c == 128 and k in (3, 7))


@pytest.mark.parametrize("name", ["rvc_resblock_bf16x3_weight_bytes", "rvc_resblock_bf16w_weight_bytes"])
def test_resblock_pair_weight_bytes_accepts_exactly_the_documented_shapes(lib, name):
    grid = list(itertools.product(range(-1, 1025), range(-1, 16)))
    n_yes, n_no = _check_grid(lib, name, grid, _resblock_documented)
    assert n_yes == 8, n_yes


# ---- K3d: rvc_conv1d_bf16w_weight_bytes(c, k) ------------------------------------------------------------------------------------------
def test_conv1d_bf16w_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    grid = list(itertools.product(range(-1, 1025), range(-1, 16)))
    n_yes, n_no = _check_grid(lib, "rvc_conv1d_bf16w_weight_bytes", grid, lambda c, k: c in (128, 256) and k in (3, 7, 11))
    assert n_yes == 6, n_yes


# ---- K3y / winobf: rvc_conv1d_winobf_weight_bytes(c_out, c_in, k) -------------------------------------------------------------------
def _winobf_documented(c_out, c_in, k):
    if c_in <= 0 or c_out <= 0 or c_in % 16:
        return False
    return (k in (7, 11) and c_out % 64 == 0) or (k == 3 and c_out % 128 == 0)


def test_conv1d_winobf_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    c_outs = sorted(set(range(-64, 1025, 16)) | {1, 8, 24, 40, 1023})
    c_ins = sorted(set(range(-16, 1025, 4)) | {1, 2, 1023})
    grid = [(c_out, c_in, k) for k in range(0, 14) for c_out in c_outs for c_in in c_ins]
    n_yes, n_no = _check_grid(lib, "rvc_conv1d_winobf_weight_bytes", grid, _winobf_documented)
    assert n_yes >= 1000 and n_no >= n_yes, (n_yes, n_no)


# ---- K11: rvc_gemm_bf16x3_weight_bytes(m, k) ------------------------------------------------------------------------------------------
def test_gemm_bf16x3_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    """m a positive multiple of 128; k a positive multiple of 16, or 1 .. 15 (the one-input-channel conv, padded to one k16 step)."""
    ms = sorted(set(range(-128, 4097, 64)) | {-1, 1, 127, 129, 255, 4095})
    ks = list(range(-1, 70)) + sorted(set(range(64, 3101, 16)) | {767, 769, 3071, 3073, 3100})
    grid = list(itertools.product(ms, ks))
    n_yes, n_no = _check_grid(lib, "rvc_gemm_bf16x3_weight_bytes", grid, lambda m, k: m > 0 and m % 128 == 0 and k > 0 and (k % 16 == 0 or k < 16),
                              value=lambda m, k: m * max(k, 16) * 6)
    assert n_yes >= 5000 and n_no >= n_yes, (n_yes, n_no)


# ---- K14: rvc_posconv_bf16x3_weight_bytes(d, groups, taps) ---------------------------------------------------------------------------
def _posconv_documented(d, groups, taps):
    return groups > 0 and d > 0 and d % groups == 0 and d // groups in (48, 64) and 1 <= taps <= 128


def test_posconv_weight_bytes_accepts_exactly_the_documented_shapes(lib):
    ds = sorted(set(range(-48, 1100, 16)) | {1, 47, 49, 63, 65, 767, 769, 1023, 1025})
    grid = [(d, groups, taps) for d in ds for groups in (-1, 0, 1, 2, 3, 8, 12, 15, 16, 17, 24)
            for taps in (-1, 0, 1, 2, 5, 64, 127, 128, 129, 256)]
    n_yes, n_no = _check_grid(lib, "rvc_posconv_bf16x3_weight_bytes", grid, _posconv_documented,
                              value=lambda d, groups, taps: groups * taps * (d // groups // 16) * 6144)
    assert n_yes >= 80 and n_no >= 10 * n_yes, (n_yes, n_no)
    w = (ctypes.c_float * (96 * 96 * 2))()
    slab = ctypes.create_string_buffer(1 << 16)        # a host buffer: a refused pack copies nothing into it
    _plant_other_error(lib)
    assert lib.rvc_posconv_bf16x3_pack_weight(w, 96, 1, 2, slab, None) != 0            # 96 channels per group
    assert lib.rvc_last_error().startswith(b"rvc_posconv_bf16x3_weight_bytes: ") and slab.raw == bytes(len(slab))


# ---- K7 / K7b: rvc_attention_workspace_bytes(batch, n_frames, n_heads, head_dim) ----------------------------------------------------
def test_attention_workspace_bytes_accepts_exactly_the_documented_shapes(lib):
    """The forward has kernels for head_dim 64 and 96 only (before: the query accepted any positive head_dim, and the forward then
    refused the shape the caller had sized a workspace for)."""
    grid = list(itertools.product((-1, 0, 1, 2, 3), (-1, 0, 1, 31, 32, 33, 257, 1599, 4799), (-1, 0, 1, 2, 12),
                                  list(range(-1, 130)) + [192, 256]))
    n_yes, n_no = _check_grid(lib, "rvc_attention_workspace_bytes", grid,
                              lambda b, t, h, d: b > 0 and h > 0 and t >= 0 and d in (64, 96))
    assert n_yes == 3 * 8 * 3 * 2 and n_no >= 10 * n_yes, (n_yes, n_no)


# ---- K13: rvc_hubert_conv0_workspace_bytes(channels) ------------------------------------------------------------------------------
def test_hubert_conv0_workspace_bytes_accepts_exactly_the_documented_shapes(lib):
    """channels a multiple of 64 in [64, 1024], what the forward takes (before: any positive count); 8 chunks of (sum, sum of squares) in
    float64 plus (mean, rstd) in fp32 per channel."""
    grid = [(c,) for c in range(-64, 2200)]
    n_yes, n_no = _check_grid(lib, "rvc_hubert_conv0_workspace_bytes", grid, lambda c: c % 64 == 0 and 0 < c <= 1024,
                              value=lambda c: c * (8 + 8 * 16))
    assert n_yes == 16, n_yes


def test_attention_workspace_bytes_follows_the_split_rule_the_gpu_tests_mirror(lib):
    """test_front_kernels_gpu._att_plan mirrors the split choice of csrc/attention.hip to assert which branches its sweep reaches; the
    size query exposes that choice (the partial results scale with the split count), so the mirror is held to the library here, on
    the CPU, over 1-3 utterances x 1-12 heads x 0-4800 frames.  The rule never picks 8 splits: 7 is the most a test can reach."""
    from test_front_kernels_gpu import _att_plan
    align = lambda n: -(-n // 256) * 256
    need = ctypes.c_size_t()
    seen = set()
    for batch in (1, 2, 3):
        for heads in (1, 2, 3, 5, 8, 12):
            for frames in list(range(0, 700)) + list(range(700, 4801, 37)):
                for hd in (64, 96):
                    _, s7, _, _ = _att_plan(batch, frames, heads, hd, True)          # K7's rule (the REL form always takes K7)
                    rows = batch * heads * s7 * frames
                    want = 256 if s7 == 1 else align(rows * hd * 4) + align(rows * 8)
                    if hd == 64:
                        kernel, sb, _, _ = _att_plan(batch, frames, heads, 64, False)
                        assert kernel == "K7b"
                        rows = 0 if sb == 1 else batch * heads * sb * frames
                        want = max(want, align(rows * 256) + align(rows * 8) + align(batch * heads * -(-frames // 32) * 24576))
                        seen.add(sb)
                    seen.add(s7)
                    assert lib.rvc_attention_workspace_bytes(batch, frames, heads, hd, ctypes.byref(need)) == 0
                    assert need.value == want, (batch, frames, heads, hd, need.value, want)
    assert seen == {1, 2, 3, 4, 5, 6, 7}, sorted(seen)
