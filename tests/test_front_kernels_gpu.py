"""The HuBERT-side bf16x3 kernels and the attention kernels over every argument their C ABI (include/rvc_amd.h) accepts:
K11 (gemmbf.hip), K12 (linbf.hip), K13 (hubert_front.hip), K14 (posconv.hip), K7 / K7b (attention.hip), and K8's gate.

test_kernels_gpu.py holds these kernels' product shapes on unit-scale randn data; this file walks what the product does NOT pass:
NULL optional pointers, paddings, every block height of K12 with fewer K chunks than its ring is deep, every channel count of K13,
taps / paddings / group counts of K14, empty trailing key splits and idle waves in the attention kernels, outlier columns, silence,
peaked and shifted attention scores, power-of-two operand scaling, NaN / Inf in the padding rows of the bf16 planes, and sentinel
bands behind every output.  References are float64 evaluations of the same formula ON THE DEVICE; every gate is either the one the
sibling test in test_kernels_gpu.py uses or a multiple of the error torch's own fp32 evaluation leaves on the same operands.
The sweeps draw seeded random shapes and ASSERT THEIR OWN COVERAGE, so a change of a dispatch rule cannot silently uncover a branch.
No test here reads or writes outside a buffer it allocated: "would write out of bounds" is always checked inside a sentinel band."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rvc_amd import _native
    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
SENT32, SENT16 = 0x5A5A5A5A, 0x5A5A      # fp32 1.5e16 / bf16 1.5e16: no kernel under test produces them
BF16_NAN, BF16_PINF, BF16_NINF = 0x7FC0, 0x7F80, 0xFF80


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(dev, shape, dtype=torch.float32, band=8192):
    """A sentinel-filled buffer of prod(shape) + band elements -> (the leading view of `shape`, the whole buffer)."""
    n = math.prod(shape)
    buf = torch.empty(n + band, dtype=dtype, device=dev)
    _bits(buf).fill_(SENT16 if buf.element_size() == 2 else SENT32)
    return buf[:n].view(shape), buf


def _untouched(t):
    """Every element of t still holds the sentinel."""
    return bool((_bits(t) == (SENT16 if t.element_size() == 2 else SENT32)).all().item())


def _rel(t, r):
    """Relative RMS error of t against the float64 reference r."""
    return ((t.double() - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def _maxabs(t, r):
    return (t.double() - r).abs().max().item()


def _split3(x):
    """The exact three-way bf16 split of fp32 x, in torch (round to nearest even, like the kernels) -> [3, ...] bf16."""
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    p2 = (r1 - p1.float()).bfloat16()
    return torch.stack([p0, p1, p2])


def _is_split_of(planes, value):
    """planes [3, ...] bf16 are the three-way split of fp32 `value`, digit by digit (compared as numbers: gelu gives -0.0 below -5.5,
    whose split is (-0, +0, +0) while the planes' fp32 sum has lost the sign)."""
    return torch.equal(planes.float(), _split3(value).float())


def _planes(x, n_pad, fill="nan", slack=0):
    """Planes [3][n_pad][k] of fp32 x [n][k]; rows n .. n_pad - 1 hold `fill`: "zero", "nan" (a mix of bf16 NaN, +Inf, -Inf) or
    "sentinel".  The kernels must never let those rows reach a stored result (rvc_amd.h, K12).  `slack`: that many NaN elements of
    the SAME allocation follow the planes, so that a kernel documented to read past their end reads memory this test owns."""
    n, k = x.shape
    buf = torch.full((3 * n_pad * k + slack,), float("nan"), dtype=torch.bfloat16, device=x.device)
    xs = buf[:3 * n_pad * k].view(3, n_pad, k)
    xs[:, :n] = _split3(x)
    if n_pad > n:
        pad = _bits(xs)[:, n:]
        if fill == "zero":
            pad.zero_()
        elif fill == "sentinel":
            pad.fill_(SENT16)
        else:
            pat = torch.tensor([BF16_NAN, BF16_PINF, BF16_NINF - 65536, BF16_NAN + 1, 0x7FFF], dtype=torch.int16, device=x.device)
            pad.copy_(pat[torch.arange(pad.numel(), device=x.device) % 5].view(pad.shape))
    return xs


def _conv1d_f64(x, w, b=None, stride=1, padding=0):
    """F.conv1d in float64 on the device as one float64 matrix product per tap; x [batch][c_in][L], w [c_out][c_in][k]."""
    xd, wd = x.double(), w.double()
    batch, _, length = xd.shape
    c_out, _, k = wd.shape
    xp = F.pad(xd, (padding, padding))
    l_out = (length + 2 * padding - k) // stride + 1
    y = torch.zeros(batch, c_out, l_out, dtype=torch.float64, device=x.device)
    for t in range(k):
        y += torch.matmul(wd[:, :, t], xp[:, :, t: t + (l_out - 1) * stride + 1: stride])
    if b is not None:
        y += b.double()[None, :, None]
    return y


def _last_error(native):
    return native._lib.rvc_last_error().decode(errors="replace")


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- K12: rvc_linear_bf16x3_presplit ------------------------------------------------------------------------------------------------
def _lbf_block_rows(n_rows, k, m, k_parts):
    """The block height linbf_dispatch (csrc/linbf.hip) picks: 128 output features unless 192- or 256-row blocks need fewer rounds of
    the 256 CUs at their relative block time.  (Confirmed against a kernel trace of three shapes when this test was written; k does
    not enter.)"""
    cols = -(-n_rows // 128)

    def cost(h, rel):
        return math.inf if m % h else -(-(cols * (m // h) * k_parts) // 256) * rel
    c128, c192, c256 = cost(128, 1.0), cost(192, 1.5 * 0.85), cost(256, 1.85)
    if c256 < c128 and c256 <= c192:
        return 256
    return 192 if c192 < c128 else 128


MODES = {0: "f32", 1: "gelu_planes", 2: "parts", 3: "gelu_f32"}


def _presplit_case(native, dev, n_rows, k, m, mode, k_parts, use_bias, extra_pad, seed, label=""):
    """One rvc_linear_bf16x3_presplit call against float64 at test_linear_bf16x3_presplit_matches_float64's gates.  The input planes'
    padding rows hold NaN / Inf, the output sits in front of a sentinel band (and its planes' padding rows hold the sentinel): the
    padding is never read into a result and never written.  Returns (MI, chunks per K part, list of failed checks)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n_rows, k, generator=g).to(dev)
    w = (torch.randn(m, k, generator=g) * k ** -0.5).to(dev)
    b = torch.randn(m, generator=g).to(dev) if use_bias and mode != 2 else None
    n_pad = native.rows_padded(n_rows) + 128 * extra_pad
    xs = _planes(x, n_pad, "nan")
    a = native.gemm_bf16x3_pack_weight(w, dev)
    ref = x.double() @ w.double().t()
    lib = F.linear(x, w, b)
    if b is not None:
        ref = ref + b.double()
    if mode == 1:
        out, buf = _guarded(dev, (3, n_pad, m), torch.bfloat16)
    elif mode == 2:
        out, buf = _guarded(dev, (k_parts, n_rows, m))
    else:
        out, buf = _guarded(dev, (n_rows, m))
    native.linear_bf16x3_presplit(xs, a, b, n_rows, m, MODES[mode], k_parts, out=out)
    torch.cuda.synchronize()
    bad = []
    if not _untouched(buf[out.numel():]):
        bad.append("wrote behind the output")
    if mode == 1:
        if not _untouched(out[:, n_rows:]):
            bad.append("wrote padding rows of the output planes")
        got = out[:, :n_rows].float().sum(0)
    elif mode == 2:
        got = out.double().sum(0)
    else:
        got = out
    floor = 4e-7
    if mode in (1, 3):
        ref, lib, floor = F.gelu(ref), F.gelu(lib), 3e-7
    e, r, rl = _maxabs(got, ref), _rel(got, ref), _rel(lib, ref)
    mi = _lbf_block_rows(n_rows, k, m, k_parts) // 64
    n_chunks = k // 32 // k_parts
    print(f"{label} presplit [{n_rows} (pad {n_pad}) x {k}] -> {m} mode {mode} parts {k_parts} bias {b is not None}: MI {mi}, chunks {n_chunks}, "
          f"max abs {e:.2e}, rel rms {r:.2e} (torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f})")
    if not torch.isfinite(got).all():
        bad.append("non-finite result (a padding row reached a stored value?)")
    if not e <= 2e-5 * max(1.0, ref.abs().max().item()):
        bad.append(f"max abs {e:.2e}")
    if not r <= max(1.5 * rl, floor):
        bad.append(f"rel rms {r:.2e} vs torch {rl:.2e}")
    return mi, n_chunks, bad


@pytest.mark.parametrize("n_rows,k,m,mode,k_parts,use_bias,extra_pad", [
    (12800, 32, 384, 0, 1, False, 0),      # MI 3, ONE chunk (fewer than the ring is deep), no bias: HuBERT's bias-free form
    (12800, 64, 384, 1, 1, False, 0),      # MI 3, two chunks, GELU -> planes without bias
    (12800, 96, 384, 3, 1, False, 1),      # MI 3, three chunks, GELU -> fp32 without bias, planes longer than rows_padded
    (25600, 32, 256, 0, 1, True, 0),       # MI 4, one chunk
    (25600, 64, 256, 1, 1, False, 0),      # MI 4, two chunks
    (25600, 96, 256, 2, 1, False, 0),      # MI 4, three chunks, partial sums with one part
    (25473, 32, 256, 3, 1, False, 2),      # MI 4, one chunk, one live row in the last tile
    (127, 32, 128, 1, 1, False, 0),        # MI 2, one chunk, planes out
    (129, 64, 128, 2, 2, False, 0),        # MI 2, two parts of one chunk each
    (1, 96, 256, 2, 3, False, 3),          # one row, three parts of one chunk
    (300, 768, 768, 2, 4, False, 0),       # k_parts 4 and 6 (24 steps: 6 and 4 chunks)
    (300, 768, 768, 2, 6, False, 1),
    (1599, 768, 768, 0, 1, False, 0),      # the product's shapes without their bias
    (1599, 768, 3072, 1, 1, False, 0),
])
def test_linear_presplit_every_argument_and_edge(native, dev, n_rows, k, m, mode, k_parts, use_bias, extra_pad):
    """K12 where test_linear_bf16x3_presplit_matches_float64 does not go: bias_dev NULL in modes 0 / 1 / 3 (what the feature extractor
    passes), each block height (MI 2 / 3 / 4) with 1, 2 and 3 chunks per K part -- the ring prologue's `n_chunks < D` cases --,
    k_parts 1 / 2 / 3 / 4 / 6, one live row in the last tile, planes allocated beyond rows_padded(n_rows)."""
    mi, n_chunks, bad = _presplit_case(native, dev, n_rows, k, m, mode, k_parts, use_bias, extra_pad, seed=n_rows + k + m + mode)
    assert not bad, bad


def test_linear_presplit_block_height_mirror_matches_the_documented_shapes():
    """The shapes the parametrised test relies on for MI 3 / MI 4 (and the product's own: 3072-wide feed-forward -> 192-row blocks)."""
    assert _lbf_block_rows(12800, 32, 384, 1) == 192 and _lbf_block_rows(25600, 32, 256, 1) == 256
    assert _lbf_block_rows(1599, 768, 3072, 1) == 192 and _lbf_block_rows(1599, 768, 2304, 1) == 128
    assert _lbf_block_rows(47999, 1536, 512, 1) == 256 and _lbf_block_rows(128, 32, 128, 1) == 128


def test_linear_presplit_random_sweep(native, dev):
    """40 seeded draws over block height MI 2 / 3 / 4 x mode 0 / 1 / 2 / 3 x chunks per part 1 / 2 / 3 / 4 / more x k_parts 1 / 2 / 3 / 4 / 6
    (mode 2) x bias on / off x n_rows % 128 in {0, 1, 127, other} x planes at and beyond rows_padded(n_rows).  Coverage asserted: every
    (MI, mode) pair, and chunks 1, 2 and 3 for every MI."""
    rng = np.random.default_rng(20261016)
    seen_pairs, seen_chunks, failures = set(), set(), []
    m_for = {2: [128, 256, 640, 768], 3: [384, 768, 1152], 4: [256, 512]}
    for it in range(40):
        mi_want, mode = (2, 3, 4)[it % 3], it % 4
        chunks_class = (it // 3) % 5
        n_chunks = chunks_class + 1 if chunks_class < 4 else int(rng.integers(5, 13))
        k_parts = int(rng.choice([1, 2, 3, 4, 6])) if mode == 2 else 1
        k = 32 * n_chunks * k_parts
        rem = (128, 1, 127, int(rng.integers(2, 127)))[(it // 2) % 4]
        for _ in range(10000):                                       # rejection sampling through the mirror of the dispatch
            m = int(rng.choice(m_for[mi_want]))
            cols = int(rng.integers(1, 30000 // 128 + 1))
            n_rows = (cols - 1) * 128 + rem
            if _lbf_block_rows(n_rows, k, m, k_parts) == 64 * mi_want and n_rows * k <= 30_000_000:
                break
        else:
            raise AssertionError(f"no shape for MI {mi_want}, k_parts {k_parts}")
        mi, nc, bad = _presplit_case(native, dev, n_rows, k, m, mode, k_parts, bool(rng.integers(0, 2)), int(rng.choice([0, 0, 1, 2])),
                                     seed=7000 + it, label=f"sweep {it}:")
        assert mi == mi_want and nc == n_chunks
        seen_pairs.add((mi, mode))
        seen_chunks.add((mi, min(nc, 5)))
        failures += [(it, n_rows, k, m, mode, k_parts, f) for f in bad]
    assert not failures, failures
    assert seen_pairs == {(a, b) for a in (2, 3, 4) for b in range(4)}, sorted(seen_pairs)
    assert {(a, c) for a in (2, 3, 4) for c in (1, 2, 3)} <= seen_chunks, sorted(seen_chunks)


def test_presplit_wrapper_sizes_output_planes_by_the_input_planes(native, dev):
    """The C entry has ONE n_rows_padded for the planes in and the planes out.  The wrapper once allocated the output planes for
    rows_padded(n_rows) whatever the input planes' length: with longer input planes, planes 1 and 2 of the output were written at
    the longer stride, past the tensor's end."""
    n_rows, k, m = 130, 64, 128
    x = torch.randn(n_rows, k, generator=torch.Generator().manual_seed(3)).to(dev)
    a = native.gemm_bf16x3_pack_weight(torch.randn(m, k, generator=torch.Generator().manual_seed(4)) * 0.125, dev)
    short = native.linear_bf16x3_presplit(_planes(x, 256, "nan"), a, None, n_rows, m, "gelu_planes", 1)
    long_ = native.linear_bf16x3_presplit(_planes(x, 512, "nan"), a, None, n_rows, m, "gelu_planes", 1)
    assert short.shape == (3, 256, m) and long_.shape == (3, 512, m)
    assert torch.equal(_bits(short[:, :n_rows]), _bits(long_[:, :n_rows]))


def test_split_rows_kernel_equals_the_torch_split(native, dev):
    """rvc_split_rows_bf16x3 writes exactly the round-to-nearest-even three-way split (what _split3 builds for the other tests) and
    leaves the padding rows of its planes alone."""
    for n_rows, k, extra in ((1, 16, 0), (129, 48, 1), (1599, 768, 0)):
        x = torch.randn(n_rows, k, generator=torch.Generator().manual_seed(n_rows)).to(dev)
        n_pad = native.rows_padded(n_rows) + 128 * extra
        xs, buf = _guarded(dev, (3, n_pad, k), torch.bfloat16)
        native.split_rows_bf16x3(x, out=xs)
        assert _is_split_of(xs[:, :n_rows], x)
        assert _untouched(xs[:, n_rows:]) and _untouched(buf[xs.numel():])


# ---- K12: rvc_conv1d_frames_bf16x3 --------------------------------------------------------------------------------------------------
def _conv_frames_call(native, xs, n_in, a, bias, m, taps, stride, mode, y, ys, n_out_pad):
    return native._lib.rvc_conv1d_frames_bf16x3(xs.data_ptr(), n_in, xs.shape[1], xs.shape[2], taps, stride, a.data_ptr(), _ptr(bias), _ptr(y), _ptr(ys),
                                               n_out_pad, m, mode, native._stream())


def _conv_frames_case(native, dev, frames_in, c, taps, stride, m, mode, use_bias, tight_planes, seed, label=""):
    """One rvc_conv1d_frames_bf16x3 call against float64 at test_conv1d_frames_bf16x3_matches_float64's gates; the input planes are
    either exactly frames_in rows long (tight: the last tile reads beyond them) or padded to 128 with NaN / Inf rows; sentinel band
    behind the output."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames_in, c, generator=g).to(dev)
    w = (torch.randn(m, c, taps, generator=g) * (c * taps) ** -0.5).to(dev)
    b = torch.randn(m, generator=g).to(dev) if use_bias else None
    # tight: the last tile's rows start up to 127 x stride frames past the planes' end ("read inside the planes' allocation, or as zeros
    # beyond it", rvc_amd.h): whichever of the two the hardware does, what lies there belongs to this test and is NaN
    xs = _planes(x, frames_in if tight_planes else native.rows_padded(frames_in), "nan", slack=(128 * stride + taps) * c)
    a = native.gemm_bf16x3_pack_weight(w.permute(0, 2, 1).reshape(m, -1).contiguous(), dev)
    n_out = (frames_in - taps) // stride + 1
    n_out_pad = native.rows_padded(n_out)
    ref = _conv1d_f64(x.t()[None], w, b, stride=stride)[0].t()
    lib = F.conv1d(x.t()[None].contiguous(), w, b, stride=stride)[0].t()
    if mode != 0:
        ref, lib = F.gelu(ref), F.gelu(lib)
    out, buf = _guarded(dev, (3, n_out_pad, m), torch.bfloat16) if mode == 1 else _guarded(dev, (n_out, m))
    rc = _conv_frames_call(native, xs, frames_in, a, b, m, taps, stride, mode, None if mode == 1 else out, out if mode == 1 else None, n_out_pad)
    torch.cuda.synchronize()
    assert rc == 0, _last_error(native)
    bad = []
    if not _untouched(buf[out.numel():]) or (mode == 1 and not _untouched(out[:, n_out:])):
        bad.append("wrote outside the live output rows")
    got = out[:, :n_out].float().sum(0) if mode == 1 else out
    e, r, rl = _maxabs(got, ref), _rel(got, ref), _rel(lib, ref)
    mi = _lbf_block_rows(n_out, taps * c, m, 1) // 64
    print(f"{label} conv over frames [{frames_in} x {c}] k{taps} s{stride} -> {m} mode {mode} bias {use_bias} tight {tight_planes}: MI {mi}, "
          f"{n_out} frames, max abs {e:.2e}, rel rms {r:.2e} (torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f})")
    if not torch.isfinite(got).all():
        bad.append("non-finite result")
    if not e <= 2e-5 * max(1.0, ref.abs().max().item()):
        bad.append(f"max abs {e:.2e}")
    if not r <= max(1.5 * rl, 6e-7):
        bad.append(f"rel rms {r:.2e} vs torch {rl:.2e}")
    return mi, bad


@pytest.mark.parametrize("frames_in,c,taps,stride,m,mode,use_bias,tight", [
    (2999, 512, 2, 2, 512, 0, False, False), (2999, 512, 3, 2, 512, 1, False, False), (2999, 512, 2, 2, 512, 3, False, False),   # no bias, each mode
    (300, 8, 4, 1, 128, 0, True, False), (300, 8, 4, 4, 128, 1, False, True),     # the smallest K: 8 channels x 4 taps = 32 (planes built in torch)
    (257, 64, 1, 1, 128, 0, True, False), (257, 32, 1, 3, 128, 3, False, True),   # one tap (a strided linear layer)
    (1000, 32, 2, 5, 128, 0, True, False), (1000, 64, 3, 7, 256, 1, False, True),  # stride > taps: gaps between the windows
    (500, 32, 5, 1, 128, 3, True, True),                                          # stride 1: overlapping windows
    (3, 512, 3, 2, 512, 0, False, True), (5, 64, 5, 1, 128, 1, True, True),       # frames_in == taps: one output frame
    (333, 64, 3, 2, 128, 0, False, True), (200, 128, 2, 2, 256, 1, True, True),   # planes of exactly frames_in rows (not a multiple of 128)
    (51203, 64, 2, 2, 256, 1, False, True),                                       # 25 601 output frames x 256: 256-row blocks (MI 4)
    (131, 64, 3, 2, 128, 3, False, False),                                        # 128-row blocks (MI 2)
])
def test_conv1d_frames_every_argument_and_edge(native, dev, frames_in, c, taps, stride, m, mode, use_bias, tight):
    """K12's conv over time-major frames beyond test_conv1d_frames_bf16x3_matches_float64: bias NULL in each mode (HuBERT's convs have
    none), K = 32, one tap, stride above and below taps, one output frame, input planes that end inside the last 128-frame tile
    (rvc_amd.h: read inside the allocation or as zeros, never stored), and both ends of the block-height choice."""
    mi, bad = _conv_frames_case(native, dev, frames_in, c, taps, stride, m, mode, use_bias, tight, seed=frames_in + c + taps + mode)
    if frames_in == 51203:
        assert mi == 4
    if frames_in == 131:
        assert mi == 2
    assert not bad, bad


def test_conv1d_frames_random_sweep(native, dev):
    """24 seeded draws: channels 8-512, taps 1-5, stride 1-7, 1-20 000 input frames, every mode, bias on / off, tight and padded planes.
    Coverage asserted: every mode without bias, stride > taps and stride < taps, one-output clips, tight planes with a partial tile."""
    rng = np.random.default_rng(416)
    seen, failures = set(), []
    for it in range(24):
        mode = (0, 1, 3)[it % 3]
        c = int(rng.choice([8, 16, 32, 64, 128, 512]))
        taps = int(rng.choice([t for t in (1, 2, 3, 4, 5) if (t * c) % 32 == 0]))
        stride = int(rng.choice([s for s in (1, 2, 3, 5, 7) if (s * c) % 8 == 0]))
        m = int(rng.choice([128, 256, 384, 512]))
        frames_in = taps + int(rng.integers(0, stride)) if it % 8 == 5 else int(rng.integers(taps, min(20000, 4_000_000 // c)))
        use_bias, tight = bool((it // 3) % 2), bool(rng.integers(0, 2))
        mi, bad = _conv_frames_case(native, dev, frames_in, c, taps, stride, m, mode, use_bias, tight, seed=9000 + it, label=f"sweep {it}:")
        n_out = (frames_in - taps) // stride + 1
        seen |= {("nobias", mode)} if not use_bias else set()
        seen |= {"gaps"} if stride > taps else set()
        seen |= {"overlap"} if stride < taps else set()
        seen |= {"one"} if n_out == 1 else set()
        seen |= {"tight"} if tight and frames_in % 128 else set()
        failures += [(it, frames_in, c, taps, stride, m, mode, f) for f in bad]
    assert not failures, failures
    assert {("nobias", 0), ("nobias", 1), ("nobias", 3), "gaps", "overlap", "one", "tight"} <= seen, seen


# ---- K12: rvc_bias_residual_layernorm_bf16x3 ----------------------------------------------------------------------------------------
def _layer_norm(v, gamma, beta, eps=1e-5):
    """F.layer_norm over the last dimension in v's dtype, gamma / beta optional (each on its own)."""
    y = F.layer_norm(v, (v.shape[-1],), None, None, eps)
    y = y * gamma.to(v.dtype) if gamma is not None else y
    return y + beta.to(v.dtype) if beta is not None else y


def _ln_call(native, parts, bias, res, gamma, beta, eps, y, ys, n_rows, n_pad, features):
    return native._lib.rvc_bias_residual_layernorm_bf16x3(parts.data_ptr(), parts.shape[0], _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta), float(eps),
                                                         _ptr(y), _ptr(ys), n_rows, n_pad, features, native._stream())


@pytest.mark.parametrize("features", [256, 768, 1024])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 6])
def test_layernorm_every_argument_and_edge(native, dev, features, n_parts):
    """The fused split-K reduction + bias + residual + LayerNorm at all three feature counts (1024: HuBERT-large's instantiation) and
    1 / 2 / 3 / 6 parts (1: the use behind K14), with each of bias / res / gamma / beta NULL in turn, fp32-only, planes-only and both
    outputs, and 1 / 3 / 4 / 5 / 131 rows (four rows per block).  Against float64 F.layer_norm at the sibling test's gate (relative RMS
    <= 1.5 x torch fp32's, floor 3e-7; max abs <= 2e-5 of the largest value); the planes sum to the fp32 output bit for bit; nothing
    is written behind the outputs or into the planes' padding rows."""
    g = torch.Generator().manual_seed(features + n_parts)
    failures = []
    variants = [("all", "both"), ("no bias", "both"), ("no res", "y"), ("no gamma", "ys"), ("no beta", "both"), ("none", "ys"), ("all", "y")]
    for vi, (drop, outs) in enumerate(variants):
        n_rows = (1, 3, 4, 5, 131, 4, 3)[vi]
        parts = torch.randn(n_parts, n_rows, features, generator=g).to(dev)
        bias = None if drop in ("no bias", "none") else torch.randn(features, generator=g).to(dev)
        res = None if drop in ("no res", "none") else torch.randn(n_rows, features, generator=g).to(dev)
        gamma = None if drop in ("no gamma", "none") else torch.randn(features, generator=g).to(dev)
        beta = None if drop in ("no beta", "none") else torch.randn(features, generator=g).to(dev)
        n_pad = native.rows_padded(n_rows) + (128 if vi % 2 else 0)
        y, ybuf = _guarded(dev, (n_rows, features)) if outs != "ys" else (None, None)
        ys, ysbuf = _guarded(dev, (3, n_pad, features), torch.bfloat16) if outs != "y" else (None, None)
        rc = _ln_call(native, parts, bias, res, gamma, beta, 1e-5, y, ys, n_rows, n_pad if ys is not None else n_rows, features)
        torch.cuda.synchronize()
        assert rc == 0, _last_error(native)
        v64 = parts.double().sum(0) + (bias.double() if bias is not None else 0) + (res.double() if res is not None else 0)
        ref = _layer_norm(v64, gamma, beta)
        v32 = parts.sum(0) if n_parts > 1 else parts[0]
        v32 = v32 + bias if bias is not None else v32
        v32 = v32 + res if res is not None else v32
        lib = _layer_norm(v32, gamma, beta)
        got = y if y is not None else ys[:, :n_rows].float().sum(0)
        e, r, rl = _maxabs(got, ref), _rel(got, ref), _rel(lib, ref)
        print(f"layernorm {n_parts} parts x [{n_rows} x {features}] {drop}, out {outs}: max abs {e:.2e}, rel rms {r:.2e} (torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f})")
        if y is not None and not _untouched(ybuf[y.numel():]):
            failures.append((drop, "wrote behind y"))
        if ys is not None and not (_untouched(ysbuf[ys.numel():]) and _untouched(ys[:, n_rows:])):
            failures.append((drop, "wrote outside the live rows of the planes"))
        if y is not None and ys is not None and not torch.equal(ys[:, :n_rows].float().sum(0), y):
            failures.append((drop, "planes != fp32 output"))
        if ys is not None and not _is_split_of(ys[:, :n_rows], got):
            failures.append((drop, "planes are not the exact split"))
        if not e <= 2e-5 * max(1.0, ref.abs().max().item()):
            failures.append((drop, f"max abs {e:.2e}"))
        if not r <= max(1.5 * rl, 3e-7):
            failures.append((drop, f"rel rms {r:.2e} vs torch {rl:.2e}"))
    assert not failures, failures


@pytest.mark.parametrize("features", [256, 768, 1024])
def test_layernorm_constant_rows_zero_rows_and_common_offset(native, dev, features):
    """Rows of zero variance give beta EXACTLY (constants whose fp32 row sums are exact: the mean is the constant and every deviation
    0), an all-zero row too; rows riding on a common offset of 1000 stay at torch fp32's error level (two-pass variance: no
    cancellation of squares)."""
    g = torch.Generator().manual_seed(features)
    gamma, beta = torch.randn(features, generator=g).to(dev), torch.randn(features, generator=g).to(dev)
    consts = torch.tensor([3.0, -2.0, 0.5, 0.0, 1.0], device=dev)
    parts = torch.stack([consts[:, None].expand(5, features), (2 * consts)[:, None].expand(5, features)]).contiguous()   # row sums 3 c
    y, ys = native.bias_residual_layernorm_bf16x3(parts, None, None, gamma, beta, 1e-5)
    assert torch.equal(y, beta[None].expand(5, features)), (y - beta).abs().max().item()
    assert torch.equal(ys[:, :5].float().sum(0), y)
    y0, _ = native.bias_residual_layernorm_bf16x3(parts, None, None, gamma, None, 1e-5, want_planes=False)
    assert torch.equal(y0, torch.zeros_like(y0))
    # common offset
    n_rows = 257
    x = (1000.0 + torch.randn(1, n_rows, features, generator=g)).to(dev)
    y, ys = native.bias_residual_layernorm_bf16x3(x, None, None, gamma, beta, 1e-5)
    ref = F.layer_norm(x[0].double(), (features,), gamma.double(), beta.double(), 1e-5)
    lib = F.layer_norm(x[0], (features,), gamma, beta, 1e-5)
    r, rl = _rel(y, ref), _rel(lib, ref)
    print(f"layernorm [{n_rows} x {features}] on an offset of 1000: rel rms {r:.2e} (torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f}); "
          f"max abs {_maxabs(y, ref):.2e} (torch {_maxabs(lib, ref):.2e})")
    assert r <= max(1.5 * rl, 3e-7), (r, rl)
    assert torch.equal(ys[:, :n_rows].float().sum(0), y)


# ---- K11: rvc_linear_bf16x3 / rvc_conv1d_bf16x3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,k,m,act,with_res", [(1599, 768, 768, "none", False), (149, 768, 3072, "gelu", False), (130, 16, 128, "none", True),
                                                     (1, 512, 768, "gelu", True)])
def test_linear_bf16x3_without_bias(native, dev, n_rows, k, m, act, with_res):
    """K11's linear form with bias_dev NULL (every case of test_linear_bf16x3_matches_float64 passes one), same gates."""
    g = torch.Generator().manual_seed(n_rows + k + m)
    x = torch.randn(n_rows, k, generator=g).to(dev)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(dev)
    res = torch.randn(n_rows, m, generator=g).to(dev) if with_res else None
    ref, lib = F.linear(x.double(), w.double()), F.linear(x, w)
    if act == "gelu":
        ref, lib = F.gelu(ref), F.gelu(lib)
    if with_res:
        ref, lib = ref + res.double(), lib + res
    a = native.gemm_bf16x3_pack_weight(w, dev)
    got = native.linear_bf16x3(x, a, None, m, act=act, res=res)
    r, rl = _rel(got, ref), _rel(lib, ref)
    print(f"linear {n_rows} x {k} -> {m} ({act}, no bias{', +res' if with_res else ''}): rel rms {r:.2e} (torch fp32 {rl:.2e}), max abs {_maxabs(got, ref):.2e}")
    assert _maxabs(got, ref) <= 2e-5 * max(1.0, ref.abs().max().item())
    assert r <= 2.0 * rl + 1e-7


@pytest.mark.parametrize("c_in,c_out,k,stride,padding,length,batch,use_bias,act", [
    (64, 128, 3, 1, 1, 300, 1, False, "none"), (64, 128, 3, 1, 2, 300, 2, True, "gelu"), (64, 128, 3, 2, 1, 301, 2, True, "none"),
    (32, 256, 5, 1, 4, 129, 1, True, "none"), (32, 256, 5, 2, 4, 130, 2, True, "gelu"), (16, 128, 4, 2, 2, 257, 1, False, "none"),
    (512, 512, 3, 2, 2, 640, 1, True, "gelu"),
    (64, 128, 3, 1, 1, 1, 2, True, "none"),        # l_in + 2 padding == k: one output column, all of it next to padding
    (32, 128, 5, 2, 2, 1, 1, False, "none"),
    (64, 128, 3, 1, 0, 300, 2, True, "none"),      # a bias without padding (the channel-major bias epilogue alone)
])
def test_conv1d_bf16x3_padding_and_bias(native, dev, c_in, c_out, k, stride, padding, length, batch, use_bias, act):
    """K11's conv form with padding > 0 (1, 2, k - 1; stride 1 and 2; batch 2) and a bias: the ABI accepts both and
    test_conv1d_bf16x3_matches_float64 passes neither.  The padded path is KEPT (not refused): it costs one compare per load.  Same
    gates as that test; the output sits in front of a sentinel band."""
    g = torch.Generator().manual_seed(c_in + c_out + k + length + padding)
    x = torch.randn(batch, c_in, length, generator=g).to(dev)
    w = (torch.randn(c_out, c_in, k, generator=g) / (c_in * k) ** 0.5).to(dev)
    b = torch.randn(c_out, generator=g).to(dev) if use_bias else None
    ref = _conv1d_f64(x, w, b, stride=stride, padding=padding)
    lib = F.conv1d(x, w, b, stride=stride, padding=padding)
    if act == "gelu":
        ref, lib = F.gelu(ref), F.gelu(lib)
    a = native.gemm_bf16x3_pack_weight(w, dev)
    l_out = (length + 2 * padding - k) // stride + 1
    y, buf = _guarded(dev, (batch, c_out, l_out))
    rc = native._lib.rvc_conv1d_bf16x3(x.data_ptr(), a.data_ptr(), _ptr(b), y.data_ptr(), batch, c_in, c_out, length, k, stride, padding,
                                       1 if act == "gelu" else 0, native._stream())
    torch.cuda.synchronize()
    assert rc == 0, _last_error(native)
    assert _untouched(buf[y.numel():])
    assert y.shape == ref.shape
    got = native.conv1d_bf16x3(x, a, b, c_out, k, stride=stride, padding=padding, act=act)
    assert torch.equal(got, y)
    r, rl = _rel(y, ref), _rel(lib, ref)
    print(f"conv1d {c_in}->{c_out} k {k} s {stride} p {padding} L {length} x{batch} bias {use_bias}: rel rms {r:.2e} (torch fp32 {rl:.2e}), max abs {_maxabs(y, ref):.2e}")
    assert _maxabs(y, ref) <= 2e-5 * max(1.0, ref.abs().max().item())
    assert r <= 1e-6


@pytest.mark.parametrize("c_in,l_in,k,stride,padding,batch", [(16, 2, 3, 2, 0, 1), (32, 1, 4, 4, 1, 2), (1, 9, 10, 5, 0, 1), (16, 4, 5, 7, 0, 2)])
def test_conv1d_bf16x3_input_shorter_than_one_window_writes_nothing(native, dev, c_in, l_in, k, stride, padding, batch):
    """An input shorter than one window has no output.  The entry point once computed l_out with C division, (l_in + 2 padding - k) /
    stride + 1 == 1 for a deficit below `stride` (l_in 2, k 3, stride 2), and stored one column of batch x c_out floats into a y_dev
    the caller had sized for none.  Called here with y_dev INSIDE a sentinel-filled buffer the test owns: returns 0, writes nothing.
    The wrapper returns an empty tensor without calling the library."""
    assert l_in + 2 * padding < k and (l_in + 2 * padding - k) / stride > -1
    c_out = 128
    x = torch.randn(batch, c_in, l_in, generator=torch.Generator().manual_seed(l_in)).to(dev)
    w = torch.randn(c_out, c_in, k, generator=torch.Generator().manual_seed(k))
    a = native.gemm_bf16x3_pack_weight(w, dev)
    buf = torch.empty(4 * batch * c_out + 4096, dtype=torch.float32, device=dev)
    _bits(buf).fill_(SENT32)
    y_ptr = buf.data_ptr() + 4 * 1024                      # room on both sides of where a wrong kernel's column would land
    rc = native._lib.rvc_conv1d_bf16x3(x.data_ptr(), a.data_ptr(), None, y_ptr, batch, c_in, c_out, l_in, k, stride, padding, 0, native._stream())
    torch.cuda.synchronize()
    assert rc == 0, _last_error(native)
    assert _untouched(buf), "rvc_conv1d_bf16x3 stored output columns for an input shorter than one window"
    got = native.conv1d_bf16x3(x, a, None, c_out, k, stride=stride, padding=padding)
    assert got.shape == (batch, c_out, 0)


# ---- K13: rvc_hubert_conv0_frames_bf16x3 --------------------------------------------------------------------------------------------
def _conv0_ref(wav, w, gamma, beta, stride, dtype):
    """Conv1d(1, C, 10, stride, no bias) -> GroupNorm(C, C) -> GELU -> [frames][C] in `dtype`; float64: windows x taps matrix product and
    explicit biased statistics; float32: torch's own graph (F.conv1d, F.group_norm), what the sibling test compares with."""
    c = w.shape[0]
    if dtype == torch.float32:
        v = F.conv1d(wav[None, None], w, stride=stride)
        if v.shape[2] > 1:
            return F.gelu(F.group_norm(v, c, gamma, beta, 1e-5))[0].t()
        n = (v - v.mean(2, keepdim=True)) / (v.var(2, unbiased=False, keepdim=True) + 1e-5).sqrt()      # (F.group_norm refuses one value per channel)
        n = n * gamma[None, :, None] if gamma is not None else n
        n = n + beta[None, :, None] if beta is not None else n
        return F.gelu(n)[0].t()
    v = wav.double().unfold(0, 10, stride) @ w.double()[:, 0, :].t()                     # [frames][C]
    n = (v - v.mean(0)) / (v.var(0, unbiased=False) + 1e-5).sqrt()
    n = n * gamma.double() if gamma is not None else n
    n = n + beta.double() if beta is not None else n
    return F.gelu(n)


@pytest.mark.parametrize("channels", [64, 192, 512, 1024])
def test_hubert_conv0_every_channel_count_stride_and_clip_length(native, dev, channels):
    """K13 beyond 512 channels and stride 5: 64 / 192 / 512 / 1024 channels (the `j < C / 64` loop; 60 KiB of LDS tables at 1024), strides
    1 / 5 / 7, clips of 1, 2, 31, 32, 33, 127, 128 and 129 frames (one thread block = 32 frames), gamma / beta NULL in turn.  Against the
    float64 graph at the sibling test's gate: max abs <= 2 x torch's fp32 graph (floor 2e-6 of the largest value).  Sentinel behind
    the planes and in their padding rows.  One frame: the variance is 0 and the result gelu(beta)."""
    g = torch.Generator().manual_seed(channels)
    failures = []
    for si, stride in enumerate((1, 5, 7)):
        for fi, frames in enumerate((1, 2, 31, 32, 33, 127, 128, 129)):
            n_samples = (frames - 1) * stride + 10 + (fi % stride)
            wav = (torch.randn(n_samples, generator=g) * 0.3).to(dev)
            w = (torch.randn(channels, 1, 10, generator=g) * 0.4).to(dev)
            gamma = None if (si + fi) % 3 == 1 else torch.randn(channels, generator=g).to(dev)
            beta = None if (si + fi) % 4 == 2 else torch.randn(channels, generator=g).to(dev)
            ref, lib = _conv0_ref(wav, w, gamma, beta, stride, torch.float64), _conv0_ref(wav, w, gamma, beta, stride, torch.float32)
            assert ref.shape == (frames, channels)
            n_pad = native.rows_padded(frames) + (128 if fi % 2 else 0)
            ys, buf = _guarded(dev, (3, n_pad, channels), torch.bfloat16)
            need = ctypes.c_size_t()
            assert native._lib.rvc_hubert_conv0_workspace_bytes(channels, ctypes.byref(need)) == 0
            ws = torch.zeros(need.value, dtype=torch.uint8, device=dev)
            rc = native._lib.rvc_hubert_conv0_frames_bf16x3(wav.data_ptr(), n_samples, w.data_ptr(), channels, 10, stride, _ptr(gamma), _ptr(beta), 1e-5,
                                                            ws.data_ptr(), ws.numel(), ys.data_ptr(), n_pad, native._stream())
            torch.cuda.synchronize()
            assert rc == 0, _last_error(native)
            got = ys[:, :frames].float().sum(0)
            e, el = _maxabs(got, ref), _maxabs(lib, ref)
            print(f"HuBERT layer 0, {channels} channels, stride {stride}, {frames} frames: max abs {e:.2e} (torch fp32 graph {el:.2e})")
            if not (_untouched(ys[:, frames:]) and _untouched(buf[ys.numel():])):
                failures.append((stride, frames, "wrote outside the live rows of the planes"))
            if not _is_split_of(ys[:, :frames], got):
                failures.append((stride, frames, "planes are not the exact split"))
            if not e <= max(2.0 * el, 2e-6 * max(1.0, ref.abs().max().item())):
                failures.append((stride, frames, f"max abs {e:.2e} vs torch {el:.2e}"))
    assert not failures, failures


def test_hubert_conv0_silence_and_dc(native, dev):
    """An all-zero clip: conv 0, variance 0, so every frame is gelu(beta) -- identical rows, the exact split, within two fp32 roundings
    (2^-22) of float64 gelu(beta).  A DC clip 0.9 + 1e-3 randn: the statistics are float64 sums of fp32 conv outputs, no cancellation;
    at the sibling test's gate against the float64 graph."""
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(512, 1, 10, generator=g) * 0.4).to(dev)
    gamma, beta = torch.randn(512, generator=g).to(dev), torch.randn(512, generator=g).to(dev)
    ys, frames = native.hubert_conv0_frames_bf16x3(torch.zeros(16000, device=dev), w, gamma, beta, 1e-5, stride=5)
    got = ys[:, :frames].float().sum(0)
    assert torch.equal(got, got[:1].expand_as(got)), "silence: the frames differ"
    assert _is_split_of(ys[:, :frames], got)
    ref = F.gelu(beta.double())
    assert ((got[0].double() - ref).abs() <= 2 ** -22 * ref.abs().clamp_min(1.0)).all(), (got[0].double() - ref).abs().max().item()
    wav = (0.9 + 1e-3 * torch.randn(16000, generator=g)).to(dev)
    ref, lib = _conv0_ref(wav, w, gamma, beta, 5, torch.float64), _conv0_ref(wav, w, gamma, beta, 5, torch.float32)
    ys, frames = native.hubert_conv0_frames_bf16x3(wav, w, gamma, beta, 1e-5, stride=5)
    got = ys[:, :frames].float().sum(0)
    e, el = _maxabs(got, ref), _maxabs(lib, ref)
    print(f"HuBERT layer 0 on a DC clip (0.9 + 1e-3 randn): max abs {e:.2e} (torch fp32 graph {el:.2e})")
    assert e <= max(2.0 * el, 2e-6 * ref.abs().max().item()), (e, el)


# ---- K14: rvc_posconv_gelu_bf16x3 ---------------------------------------------------------------------------------------------------
def _posconv_f64(x, w, b, groups, padding):
    """gelu(grouped conv) over time-major x [T][D] with `padding` zero frames in front and taps - 1 - padding behind: exactly T output
    frames.  float64 on the device, one batched matrix product per tap."""
    t, d = x.shape
    cg, taps = w.shape[1], w.shape[2]
    xp = F.pad(x.double().t(), (padding, taps - 1 - padding)).view(groups, cg, t + taps - 1)
    wg = w.double().view(groups, cg, cg, taps)
    y = torch.zeros(groups, cg, t, dtype=torch.float64, device=x.device)
    for k in range(taps):
        y += torch.bmm(wg[:, :, :, k], xp[:, :, k: k + t])
    y = y.view(d, t)
    if b is not None:
        y = y + b.double()[:, None]
    return F.gelu(y).t()


def _posconv_case(native, dev, frames, cg, groups, taps, padding, use_bias, seed, label=""):
    d = cg * groups
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(frames, d, generator=g).to(dev)
    w = (torch.randn(d, cg, taps, generator=g) * (cg * taps) ** -0.5).to(dev)
    b = torch.randn(d, generator=g).to(dev) if use_bias else None
    ref = _posconv_f64(x, w, b, groups, padding)
    xp32 = F.pad(x.t(), (padding, taps - 1 - padding))[None].contiguous()
    lib = F.gelu(F.conv1d(xp32, w, b, groups=groups))[0].t()
    a = native.posconv_bf16x3_pack_weight(w, groups, dev)
    y, buf = _guarded(dev, (frames, d))
    rc = native._lib.rvc_posconv_gelu_bf16x3(x.data_ptr(), a.data_ptr(), _ptr(b), y.data_ptr(), frames, d, groups, taps, padding, native._stream())
    torch.cuda.synchronize()
    assert rc == 0, _last_error(native)
    bad = [] if _untouched(buf[y.numel():]) else ["wrote behind the output"]
    e, r, rl = _maxabs(y, ref), _rel(y, ref), _rel(lib, ref)
    print(f"{label} positional conv [{frames} x {d}] groups {groups} taps {taps} padding {padding} bias {use_bias}: max abs {e:.2e}, rel rms {r:.2e} "
          f"(torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f})")
    if not e <= 2e-5 * max(1.0, ref.abs().max().item()):
        bad.append(f"max abs {e:.2e}")
    if not r <= max(2.0 * rl, 1.2e-6):
        bad.append(f"rel rms {r:.2e} vs torch {rl:.2e}")
    return bad


@pytest.mark.parametrize("frames,cg,groups,taps,pad_kind,use_bias", [
    (129, 48, 16, 1, "half", True), (129, 64, 2, 1, "zero", False), (255, 48, 2, 2, "half", False), (127, 64, 16, 2, "last", True),
    (1, 48, 1, 5, "half", True), (128, 64, 1, 5, "zero", False), (129, 48, 2, 5, "last", False), (255, 48, 16, 127, "half", False),
    (127, 64, 2, 127, "last", True), (1, 64, 1, 127, "zero", False), (129, 48, 1, 128, "zero", True), (255, 64, 16, 128, "last", False),
    (128, 48, 16, 128, "half", False), (1, 48, 16, 128, "last", True), (127, 48, 2, 128, "zero", False),
])
def test_posconv_every_argument_and_edge(native, dev, frames, cg, groups, taps, pad_kind, use_bias):
    """K14 beyond HuBERT's own (taps 128, padding 64, 16 groups, a bias): both widths per group with 1 / 2 / 5 / 127 / 128 taps, padding 0,
    taps / 2 and taps - 1, 1 / 127 / 128 / 129 / 255 frames, 1 / 2 / 16 groups, bias NULL.  Reference: a float64 conv over the input padded
    with `padding` zero frames in front and taps - 1 - padding behind; the sibling test's gates."""
    padding = {"zero": 0, "half": taps // 2, "last": taps - 1}[pad_kind]
    bad = _posconv_case(native, dev, frames, cg, groups, taps, padding, use_bias, seed=frames + cg + groups + taps)
    assert not bad, bad


def test_posconv_random_sweep(native, dev):
    """24 seeded draws over channels per group 48 / 64, groups 1-16, taps 1-128, any padding in [0, taps), 1-700 frames, bias on / off.
    Coverage asserted: both widths, taps 1 and 128, padding 0 and taps - 1, a single tile and several, no bias."""
    rng = np.random.default_rng(14)
    seen, failures = set(), []
    for it in range(24):
        cg = (48, 64)[it % 2]
        groups = int(rng.choice([1, 2, 3, 16]))
        taps = (1, 128, 2, 127)[it // 2 % 4] if it % 3 == 0 else int(rng.integers(1, 129))
        padding = (0, taps - 1, taps // 2)[it % 3] if it % 2 else int(rng.integers(0, taps))
        frames = int(rng.integers(1, 701))
        use_bias = bool(rng.integers(0, 2))
        bad = _posconv_case(native, dev, frames, cg, groups, taps, padding, use_bias, seed=1400 + it, label=f"sweep {it}:")
        seen |= {cg, ("taps", taps), ("tiles", min(-(-frames // 128), 2)), ("bias", use_bias)}
        seen |= {"pad0"} if padding == 0 else set()
        seen |= {"padlast"} if padding == taps - 1 and taps > 1 else set()
        failures += [(it, frames, cg, groups, taps, padding, f) for f in bad]
    assert not failures, failures
    assert {48, 64, ("taps", 1), ("taps", 128), ("tiles", 1), ("tiles", 2), ("bias", False), "pad0", "padlast"} <= seen, seen


# ---- K7 / K7b: attention --------------------------------------------------------------------------------------------------------------
# Floors of the "relative to torch fp32" gates: the smallest non-zero figures torch's fp32 eager evaluation showed over the cases of
# this file on an MI355X (relative RMS against float64; tiny cases fall below the noise of the comparison itself).
ATT_REL_FLOOR = 1.1e-7     # measured 1.11e-7: [1 x 4 frames x 10 heads x 64]


def _att_plan(batch, frames, heads, hd, rel):
    """Mirror of the dispatch in csrc/attention.hip (choose_splits_bf / choose_splits): which kernel runs, into how many key splits,
    with how many 32-key tiles each, and how many trailing splits own no tile."""
    nt = -(-frames // 32)
    bf = hd == 64 and not rel and batch * heads * nt * 24 * 1024 < 2 ** 31
    groups, units = (-(-frames // 256) * heads * batch, 256) if bf else (nt * heads * batch, 1024)
    best, best_cost = 1, 1e30
    for s in range(1, min(8, nt) + 1):
        cost = -(-(groups * s) // units) / s + 0.02 * s
        if cost < best_cost - 1e-9:
            best, best_cost = s, cost
    tps = -(-nt // best)
    used = -(-nt // tps) if nt else 0
    kernel = "K7b" if bf else f"K7<{hd},{'REL' if rel else 'plain'}>"
    return kernel, best, tps, best - used


def _attention_ref(qkv, heads, hd, emb_k, emb_v):
    """softmax(q k^T / sqrt(d) [+ q . emb_k[j - i + 10] / sqrt(d) for |j - i| <= 10]) v [+ sum_r p[i][i + r - 10] emb_v[r]] in qkv's dtype
    (rvc_amd.h, K7), dense [T][T] scores on the device."""
    b, t, _ = qkv.shape
    q, k, v = qkv.view(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    scale = hd ** -0.5
    s = q @ k.transpose(-1, -2) * scale
    if emb_k is not None:
        i = torch.arange(t, device=qkv.device)
        off = i[None, :] - i[:, None] + 10                                    # [query][key] -> r
        inside = (off >= 0) & (off <= 20)
        rl = F.pad(q @ emb_k.t() * scale, (0, 1))                             # [b][h][T][22], column 21 = 0
        s = s + rl.gather(-1, torch.where(inside, off, 21).expand(b, heads, t, t))
    p = torch.softmax(s, -1)
    o = p @ v
    if emb_k is not None:
        r = torch.arange(21, device=qkv.device)
        key = i[:, None] + r[None, :] - 10                                    # [query][r] -> key
        ok = (key >= 0) & (key < t)
        band = p.gather(-1, key.clamp(0, t - 1).expand(b, heads, t, 21)) * ok
        o = o + band @ emb_v
    return o.transpose(1, 2).reshape(b, t, heads * hd)


def _attention_case(native, dev, qkv, heads, hd, emb_k=None, emb_v=None, label="", outer=None):
    """One rvc_attention_qkv_f32 call against float64, gated relative to torch's fp32 eager evaluation of the same formula on the same
    operands on the device: relative RMS <= 2 x, max abs <= 4 x (six fp32 accumulations per product where fp32 has one: sqrt(6) = 2.4 x
    in rounding walk; the hardware exp2 adds 1 ulp).  `outer`: additionally max abs <= outer x max(1, |ref|max).  The output sits in
    front of a sentinel band.  Returns the list of failed checks."""
    b, t, _ = qkv.shape
    rel = emb_k is not None
    ref = _attention_ref(qkv.double(), heads, hd, emb_k.double() if rel else None, emb_v.double() if rel else None)
    lib = _attention_ref(qkv, heads, hd, emb_k, emb_v)
    out, buf = _guarded(dev, (b, t, heads * hd))
    need = ctypes.c_size_t()
    assert native._lib.rvc_attention_workspace_bytes(b, t, heads, hd, ctypes.byref(need)) == 0
    ws, wsbuf = _guarded(dev, (need.value,), torch.uint8, band=4096)
    rc = native._lib.rvc_attention_qkv_f32(qkv.data_ptr(), _ptr(emb_k), _ptr(emb_v), out.data_ptr(), b, t, heads, hd, hd ** -0.5, ws.data_ptr(), need.value,
                                           native._stream())
    torch.cuda.synchronize()
    assert rc == 0, _last_error(native)
    bad = []
    if not _untouched(buf[out.numel():]):
        bad.append("wrote behind the output")
    if not bool((wsbuf[need.value:] == 0x5A).all().item()):
        bad.append("wrote behind the workspace")
    assert torch.equal(native.attention_qkv(qkv, heads, hd ** -0.5, emb_k, emb_v), out), "two runs differ"
    e, el, r, rl = _maxabs(out, ref), _maxabs(lib, ref), _rel(out, ref), _rel(lib, ref)
    big = max(1.0, ref.abs().max().item())
    kernel, splits, tps, empty = _att_plan(b, t, heads, hd, rel)
    print(f"{label} attention [{b} x {t} x {heads} x {hd}]{' REL' if rel else ''} {kernel} splits {splits} x {tps} tiles ({empty} empty): rel rms {r:.2e} "
          f"(torch fp32 {rl:.2e}, ratio {r / max(rl, 1e-30):.2f}), max abs {e:.2e} (torch {el:.2e}, ratio {e / max(el, 1e-30):.2f})")
    if not torch.isfinite(out).all():
        bad.append("non-finite output")
    if not r <= 2.0 * max(rl, ATT_REL_FLOOR):
        bad.append(f"rel rms {r:.2e} vs torch {rl:.2e}")
    if not e <= 4.0 * max(el, ATT_REL_FLOOR * big):
        bad.append(f"max abs {e:.2e} vs torch {el:.2e}")
    if outer is not None and not e <= outer * big:
        bad.append(f"max abs {e:.2e} > {outer} x {big:.2f}")
    return bad


def _rel_embeddings(hd, g, dev):
    return (torch.randn(21, hd, generator=g) * hd ** -0.5).to(dev), (torch.randn(21, hd, generator=g) * hd ** -0.5).to(dev)


def test_attention_plan_mirror_matches_the_documented_shapes():
    """The shapes the existing tests reach an empty trailing split with by accident, now pinned: 9 tiles on 7 splits."""
    assert _att_plan(1, 257, 5, 64, False) == ("K7b", 7, 2, 2)
    assert _att_plan(2, 333, 2, 96, False) == ("K7<96,plain>", 7, 2, 1)
    assert _att_plan(1, 1599, 12, 64, False)[0] == "K7b" and _att_plan(1, 100, 3, 64, True)[0] == "K7<64,REL>"
    assert _att_plan(1, 1, 12, 64, False) == ("K7b", 1, 1, 0)


def test_attention_random_sweep(native, dev):
    """32 seeded draws over head_dim 64 / 96, relative-position terms on / off, batch 1-3, heads 1-12, 1-2000 frames.  Coverage asserted:
    all four kernels (K7b, K7<64,REL>, K7<96,plain>, K7<96,REL>), each with an empty trailing key split; split counts 1, 7 and three values
    between (7 is the largest the dispatch ever picks: its 0.02 s term makes 8 splits lose to 7 for every shape, pinned by
    test_kernel_contracts_cpu.py); a partial last tile; for K7b a last workgroup with idle waves; for REL a +-10 window that straddles a split boundary."""
    rng = np.random.default_rng(7)
    kinds = [(64, False), (64, True), (96, False), (96, True)]
    seen, splits_seen, failures = set(), set(), []
    for it in range(32):
        hd, rel = kinds[it % 4]
        if it < 8:                                         # 9 tiles with few heads: 7 splits of 2 tiles, the last two own nothing
            batch, heads, frames = 1, int(rng.integers(1, 4)), int(rng.integers(257, 289))
        elif it < 12:                                      # one tile: a single split
            batch, heads, frames = int(rng.integers(1, 4)), int(rng.integers(1, 13)), int(rng.integers(1, 33))
        else:
            batch, heads, frames = int(rng.integers(1, 4)), int(rng.integers(1, 13)), int(rng.integers(1, 2001))
        g = torch.Generator().manual_seed(3000 + it)
        qkv = (torch.randn(batch, frames, 3 * heads * hd, generator=g) * 1.5).to(dev)
        emb = _rel_embeddings(hd, g, dev) if rel else (None, None)
        kernel, splits, tps, empty = _att_plan(batch, frames, heads, hd, rel)
        bad = _attention_case(native, dev, qkv, heads, hd, *emb, label=f"sweep {it}:", outer=3e-5 if rel else 2e-5)
        failures += [(it, batch, frames, heads, hd, rel, f) for f in bad]
        seen.add(kernel)
        splits_seen.add(splits)
        seen |= {(kernel, "empty")} if empty else set()
        seen |= {"partial"} if frames % 32 else set()
        seen |= {"idle"} if kernel == "K7b" and 1 <= frames % 256 <= 224 else set()
        seen |= {"straddle"} if rel and splits - empty >= 2 else set()       # a boundary between two non-empty splits lies inside some query tile's window
    assert not failures, failures
    names = ["K7b", "K7<64,REL>", "K7<96,plain>", "K7<96,REL>"]
    assert set(names) | {(n, "empty") for n in names} | {"partial", "idle", "straddle"} <= seen, seen
    assert {1, 7} <= splits_seen and len(splits_seen & set(range(2, 7))) >= 3, sorted(splits_seen)


@pytest.mark.parametrize("hd,rel", [(64, False), (64, True), (96, False), (96, True)])
@pytest.mark.parametrize("kind", ["peaked", "shifted_keys", "rising_below", "rising_above", "falling", "flat"])
def test_attention_data_edges(native, dev, hd, rel, kind):
    """Scores no randn test produces, for each of the four kernels at 1599 frames (HuBERT's 12 heads for head_dim 64, the TextEncoder's 2
    for 96): peaked softmax (randn x 6), every key shifted by a common vector 40 u (softmax-invariant, large scores), keys ordered so
    that a row's running maximum rises by a little less / a little more than the lazy-rescale threshold (8 in the log2 domain) per
    32-key tile, a maximum that falls tile after tile, and a near-flat softmax (randn x 0.05).  Gated relative to torch fp32 only: on
    peaked scores fp32 arithmetic itself is 2e-5 of the largest value away from float64."""
    frames, heads = 1599, 12 if hd == 64 else 2
    g = torch.Generator().manual_seed(hd + len(kind))
    scale = {"peaked": 6.0, "flat": 0.05}.get(kind, 1.0)
    qkv = torch.randn(1, frames, 3, heads, hd, generator=g) * scale
    if kind == "shifted_keys":
        u = torch.randn(hd, generator=g)
        qkv[:, :, 1] += 40.0 * u / u.norm()
    elif kind in ("rising_below", "rising_above", "falling"):
        # q = a e_0 + noise, key j = b(j) e_0 + noise: score = a b(j) / sqrt(d) + small; in the log2 domain the tile maximum moves by
        # `step` per 32 keys
        step = {"rising_below": 7.5, "rising_above": 8.5, "falling": -8.5}[kind]
        a = 4.0
        per_key = step / 32 * math.log(2.0) * hd ** 0.5 / a                  # increment of b per key
        ramp = torch.arange(frames, dtype=torch.float32) * per_key
        qkv[:, :, 0] *= 0.05
        qkv[:, :, 1] *= 0.05
        qkv[:, :, 0, :, 0] += a
        qkv[:, :, 1, :, 0] += (ramp - ramp.mean())[None, :, None]
    qkv = qkv.reshape(1, frames, -1).contiguous().to(dev)
    emb = _rel_embeddings(hd, g, dev) if rel else (None, None)
    bad = _attention_case(native, dev, qkv, heads, hd, *emb, label=f"{kind}:")
    assert not bad, bad


# ---- data edges of the bf16x3 GEMMs -------------------------------------------------------------------------------------------------
# Floor of the componentwise-error gate: the smallest value torch's fp32 evaluation showed over the outlier cases on an MI355X.
OUTLIER_FLOOR = 9.0e-7     # measured 9.01e-7 (K14); the GEMM cases show 2.3e-6


def _outlier_rows(n_rows, k, g):
    x = torch.randn(n_rows, k, generator=g)
    x[:, ::97] *= 1000.0
    x[:, 5::89] *= 1e-4
    return x


def _componentwise(got, ref, bound):
    return ((got.double() - ref).abs() / bound).max().item()


@pytest.mark.parametrize("path", ["linear", "presplit_f32", "presplit_parts"])
def test_linear_outlier_columns_componentwise(native, dev, path):
    """Activations with outlier features (every 97th x 1000, another stride x 1e-4) through K11's linear form and K12's modes 0 and 2 at
    1599 x 768 -> 768.  Judged by the COMPONENTWISE error |got - ref| / (|x| |W|^T + |b|) -- an error confined to the small outputs next
    to a large one is invisible to a gate on max |ref| -- at most 4 x torch fp32's value of the same metric on the same operands."""
    n_rows, k, m = 1599, 768, 768
    g = torch.Generator().manual_seed(97)
    x = _outlier_rows(n_rows, k, g).to(dev)
    w = (torch.randn(m, k, generator=g) * k ** -0.5).to(dev)
    b = torch.randn(m, generator=g).to(dev) if path != "presplit_parts" else None
    ref = x.double() @ w.double().t() + (b.double() if b is not None else 0)
    bound = x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0)
    lib = F.linear(x, w, b)
    a = native.gemm_bf16x3_pack_weight(w, dev)
    if path == "linear":
        got = native.linear_bf16x3(x, a, b, m)
    else:
        xs = _planes(x, native.rows_padded(n_rows), "nan")
        assert torch.equal(_bits(native.split_rows_bf16x3(x)[:, :n_rows]), _bits(xs[:, :n_rows]))
        got = native.linear_bf16x3_presplit(xs, a, b, n_rows, m, "f32", 1) if path == "presplit_f32" else \
            native.linear_bf16x3_presplit(xs, a, None, n_rows, m, "parts", 3).double().sum(0)
    c, cl = _componentwise(got, ref, bound), _componentwise(lib, ref, bound)
    print(f"outlier columns through {path}: componentwise error {c:.2e} (torch fp32 {cl:.2e}, ratio {c / cl:.2f}); rel rms {_rel(got, ref):.2e} (torch {_rel(lib, ref):.2e})")
    assert c <= 4.0 * max(cl, OUTLIER_FLOOR), (c, cl)


def test_posconv_outlier_columns_componentwise(native, dev):
    """The same outlier features through K14 (HuBERT's shape, 300 frames); the bound is that of the conv in front of the GELU, whose
    slope is at most 1.13."""
    frames, d, groups, taps = 300, 768, 16, 128
    cg = d // groups
    g = torch.Generator().manual_seed(14)
    x = _outlier_rows(frames, d, g).to(dev)
    w = (torch.randn(d, cg, taps, generator=g) * (cg * taps) ** -0.5).to(dev)
    b = torch.randn(d, generator=g).to(dev)
    ref = _posconv_f64(x, w, b, groups, taps // 2)
    xa = F.pad(x.double().abs().t(), (taps // 2, taps - 1 - taps // 2)).view(groups, cg, frames + taps - 1)
    wa = w.double().abs().view(groups, cg, cg, taps)
    bound = sum(torch.bmm(wa[:, :, :, kk], xa[:, :, kk: kk + frames]) for kk in range(taps)).view(d, frames).t() + b.double().abs()
    lib = F.gelu(F.conv1d(F.pad(x.t(), (taps // 2, taps - 1 - taps // 2))[None].contiguous(), w, b, groups=groups))[0].t()
    got = native.posconv_gelu_bf16x3(x, native.posconv_bf16x3_pack_weight(w, groups, dev), b, groups, taps, taps // 2)
    c, cl = _componentwise(got, ref, bound), _componentwise(lib, ref, bound)
    print(f"outlier columns through K14: componentwise error {c:.2e} (torch fp32 {cl:.2e}, ratio {c / cl:.2f})")
    assert c <= 4.0 * max(cl, OUTLIER_FLOOR), (c, cl)


@pytest.mark.parametrize("ea,eb", [(0, 0), (10, -3), (-20, -20), (20, 20), (-30, 10), (3, 37), (-40, 0)])
def test_linear_power_of_two_scaling_is_exact(native, dev, ea, eb):
    """Scaling x by 2^a and W by 2^b scales every bf16 digit, every product and every partial sum by a power of two: the result must be
    2^(a + b) times the unscaled one BIT FOR BIT (K12 mode 2 and K11 without bias or activation).  No reference needed; any magnitude
    assumption in a split -- a clamp, a flush, an absolute epsilon -- breaks it."""
    n_rows, k, m = 300, 768, 256
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n_rows, k, generator=g).to(dev)
    w = (torch.randn(m, k, generator=g) * k ** -0.5).to(dev)
    base_a = native.gemm_bf16x3_pack_weight(w, dev)
    xs0 = native.split_rows_bf16x3(x)
    base12 = native.linear_bf16x3_presplit(xs0, base_a, None, n_rows, m, "parts", 3)
    base11 = native.linear_bf16x3(x, base_a, None, m)
    x2, w2 = x * 2.0 ** ea, w * 2.0 ** eb
    a2 = native.gemm_bf16x3_pack_weight(w2, dev)
    got12 = native.linear_bf16x3_presplit(native.split_rows_bf16x3(x2), a2, None, n_rows, m, "parts", 3)
    got11 = native.linear_bf16x3(x2, a2, None, m)
    assert torch.equal(got12, base12 * 2.0 ** (ea + eb)), (got12 - base12 * 2.0 ** (ea + eb)).abs().max().item()
    assert torch.equal(got11, base11 * 2.0 ** (ea + eb)), (got11 - base11 * 2.0 ** (ea + eb)).abs().max().item()


def test_zero_rows_through_presplit_and_layernorm(native, dev):
    """Silence in the middle of the pipeline: all-zero activation rows give exactly the bias (mode 0), exactly 0 (mode 2), gelu(bias)
    (modes 1 / 3), and LayerNorm of an all-zero row gives exactly beta."""
    n_rows, k, m = 130, 768, 768
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n_rows, k, generator=g)
    x[::3] = 0.0
    x = x.to(dev)
    w, b = (torch.randn(m, k, generator=g) * k ** -0.5).to(dev), torch.randn(m, generator=g).to(dev)
    a = native.gemm_bf16x3_pack_weight(w, dev)
    xs = native.split_rows_bf16x3(x)
    y0 = native.linear_bf16x3_presplit(xs, a, b, n_rows, m, "f32", 1)
    assert torch.equal(y0[::3], b[None].expand(y0[::3].shape))
    parts = native.linear_bf16x3_presplit(xs, a, None, n_rows, m, "parts", 3)
    assert torch.equal(parts[:, ::3], torch.zeros_like(parts[:, ::3]))
    y3 = native.linear_bf16x3_presplit(xs, a, b, n_rows, m, "gelu_f32", 1)
    y1 = native.linear_bf16x3_presplit(xs, a, b, n_rows, m, "gelu_planes", 1)
    assert torch.equal(y1[:, :n_rows].float().sum(0), y3)
    assert torch.equal(y3[::3], y3[:1].expand(y3[::3].shape))
    assert ((y3[0].double() - F.gelu(b.double())).abs() <= 2 ** -22 * F.gelu(b.double()).abs().clamp_min(1.0)).all()
    gamma, beta = torch.randn(m, generator=g).to(dev), torch.randn(m, generator=g).to(dev)
    yl, _ = native.bias_residual_layernorm_bf16x3(parts, None, None, gamma, beta, 1e-5)
    assert torch.equal(yl[::3], beta[None].expand(yl[::3].shape))


# ---- the padding rows of the planes: never read into a stored result ------------------------------------------------------------------
def test_padding_rows_of_the_input_planes_never_reach_a_result(native, dev):
    """rvc_amd.h (K12): "Rows n_rows .. n_rows_padded - 1 of a plane are never read into a stored result and never written: they need no
    initialisation" -- the product allocates planes with torch.empty.  Every plane-consuming call runs twice, once with those rows
    zeroed and once with bf16 NaN / +Inf / -Inf in them: the stored outputs are bit-equal.  K12's GEMM in all four modes (each block
    height), the conv over frames, and K13's planes chained into K12's conv."""
    g = torch.Generator().manual_seed(77)
    for n_rows, k, m, mode, k_parts in ((130, 96, 128, 0, 1), (12801, 64, 384, 1, 1), (25601, 32, 256, 3, 1), (300, 192, 256, 2, 3), (1, 32, 128, 0, 1)):
        x = torch.randn(n_rows, k, generator=g).to(dev)
        w, b = (torch.randn(m, k, generator=g) * k ** -0.5).to(dev), torch.randn(m, generator=g).to(dev)
        a = native.gemm_bf16x3_pack_weight(w, dev)
        n_pad = native.rows_padded(n_rows) + 128
        outs = []
        for fill in ("zero", "nan"):
            out = _guarded(dev, (3, n_pad, m), torch.bfloat16)[0] if mode == 1 else None       # planes out: the same n_rows_padded as the planes in
            outs.append(native.linear_bf16x3_presplit(_planes(x, n_pad, fill), a, None if mode == 2 else b, n_rows, m, MODES[mode], k_parts, out=out))
        live = (lambda t: t[:, :n_rows]) if mode == 1 else (lambda t: t)
        assert torch.equal(_bits(live(outs[0])), _bits(live(outs[1]))), (n_rows, k, m, mode)
        assert torch.isfinite(live(outs[1]).float()).all()
    for frames_in, c, taps, stride, m, mode in ((131, 64, 3, 2, 128, "f32"), (1000, 32, 5, 3, 128, "gelu_planes"), (257, 128, 2, 1, 256, "gelu_f32")):
        x = torch.randn(frames_in, c, generator=g).to(dev)
        w = (torch.randn(m, c, taps, generator=g) * (c * taps) ** -0.5).to(dev)
        a = native.gemm_bf16x3_pack_weight(w.permute(0, 2, 1).reshape(m, -1).contiguous(), dev)
        outs = [native.conv1d_frames_bf16x3(_planes(x, native.rows_padded(frames_in) + 128, fill, slack=(128 * stride + taps) * c), frames_in, a, None, m, taps, stride, mode) for fill in ("zero", "nan")]
        n_out = outs[0][1]
        live = (lambda t: t[:, :n_out]) if mode == "gelu_planes" else (lambda t: t)
        assert torch.equal(_bits(live(outs[0][0])), _bits(live(outs[1][0]))), (frames_in, c, taps, stride)
        assert torch.isfinite(live(outs[1][0]).float()).all()
    # K13 -> K12: the first layer's planes keep whatever their padding rows held; the second layer must not care
    wav = (torch.randn(4003, generator=g) * 0.3).to(dev)
    w0 = (torch.randn(512, 1, 10, generator=g) * 0.4).to(dev)
    w1 = (torch.randn(512, 512, 3, generator=g) * 1536 ** -0.5).to(dev)
    a1 = native.gemm_bf16x3_pack_weight(w1.permute(0, 2, 1).reshape(512, -1).contiguous(), dev)
    ys, frames = native.hubert_conv0_frames_bf16x3(wav, w0, None, None, 1e-5, stride=5)
    results = []
    for fill in ("zero", "nan"):
        poisoned = _planes(ys[:, :frames].float().sum(0), ys.shape[1], fill, slack=(128 * 2 + 3) * 512)
        poisoned[:, :frames] = ys[:, :frames]
        results.append(native.conv1d_frames_bf16x3(poisoned, frames, a1, None, 512, 3, 2, "gelu_f32")[0])
    assert torch.equal(_bits(results[0]), _bits(results[1])) and torch.isfinite(results[1]).all()


# ---- K8: the flow's gate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 192, 3198), (2, 96, 5), (1, 1, 1)])
def test_gate_tanh_sigmoid_matches_float64(native, dev, shape):
    """rvc_gate_tanh_sigmoid_f32 (the WaveNet gate of the flow): tanh(x[:, :H]) * sigmoid(x[:, H:]) against float64, max abs error at
    most 2 x torch fp32's on the same input; inputs of +-30, where the sigmoid saturates, included; sentinel behind the output."""
    b, h, t = shape
    g = torch.Generator().manual_seed(h + t)
    x = torch.randn(b, 2 * h, t, generator=g) * 3
    flat = x.view(-1)
    flat[::7] = 30.0
    flat[3::11] = -30.0
    x = x.to(dev)
    ref = torch.tanh(x[:, :h].double()) * torch.sigmoid(x[:, h:].double())
    lib = torch.tanh(x[:, :h]) * torch.sigmoid(x[:, h:])
    out, buf = _guarded(dev, (b, h, t))
    assert native._lib.rvc_gate_tanh_sigmoid_f32(x.data_ptr(), out.data_ptr(), b, h, t, native._stream()) == 0, _last_error(native)
    torch.cuda.synchronize()
    assert _untouched(buf[out.numel():])
    assert torch.equal(native.gate_tanh_sigmoid(x), out)
    e, el = _maxabs(out, ref), _maxabs(lib, ref)
    print(f"gate {shape}: max abs {e:.2e} (torch fp32 {el:.2e}, ratio {e / max(el, 1e-30):.2f})")
    assert torch.isfinite(out).all()
    assert e <= 2.0 * el, (e, el)


# ---- forward refusals -----------------------------------------------------------------------------------------------------------------
def _plant_other_error(native):
    need = ctypes.c_size_t()
    assert native._lib.rvc_knn_workspace_bytes(100, 10, 768, 5, ctypes.byref(need)) != 0


def test_forward_refusals_name_their_entry_and_write_nothing(native, dev):
    """One call per documented constraint of the HuBERT-side entries, violating it alone, with real device buffers: non-zero return, a
    message that starts with the entry's name, and every output still full of its sentinel."""
    lib, st = native._lib, native._stream()
    g = torch.Generator().manual_seed(1)
    outputs = []

    def out(shape, dtype=torch.float32):
        v, buf = _guarded(dev, shape, dtype, band=256)
        outputs.append(buf)
        return v

    def refused(name, rc):
        msg = _last_error(native)
        assert rc != 0, f"{name} accepted the call"
        assert msg.startswith(name + ": ") and len(msg) > len(name) + 2, (name, msg)
        torch.cuda.synchronize()
        assert all(_untouched(o) for o in outputs), f"{name} wrote into an output of a refused call"
        _plant_other_error(native)

    _plant_other_error(native)
    # K12 GEMM
    n, k, m = 130, 128, 128
    xs = _planes(torch.randn(n, k, generator=g).to(dev), 256, "zero")
    a = native.gemm_bf16x3_pack_weight(torch.randn(m, k, generator=g), dev)
    bias = torch.randn(m, generator=g).to(dev)
    y, ys, yp = out((n, m)), out((3, 256, m), torch.bfloat16), out((5, n, m))
    f = lib.rvc_linear_bf16x3_presplit
    name = "rvc_linear_bf16x3_presplit"
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), ys.data_ptr(), n, 256, k, m, 4, 1, st))              # mode
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), ys.data_ptr(), n, 256, k, m, -1, 1, st))
    refused(name, f(xs.data_ptr(), a.data_ptr(), None, yp.data_ptr(), None, n, 256, k, m, 2, 3, st))                                 # k_parts 3 does not divide 128 / 32
    refused(name, f(xs.data_ptr(), a.data_ptr(), None, yp.data_ptr(), None, n, 256, k, m, 2, 0, st))
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), None, n, 256, k, m, 0, 2, st))                       # several parts outside mode 2
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), ys.data_ptr(), n, 200, k, m, 0, 1, st))              # n_rows_padded % 128
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), ys.data_ptr(), n, 128, k, m, 0, 1, st))              # n_rows_padded < n_rows
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), None, ys.data_ptr(), n, 256, k, m, 0, 1, st))                      # mode 0 without y
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), y.data_ptr(), None, n, 256, k, m, 1, 1, st))                       # mode 1 without ys
    refused(name, f(xs.data_ptr(), a.data_ptr(), bias.data_ptr(), None, ys.data_ptr(), n, 256, k, m, 3, 1, st))                      # mode 3 without y
    # K12 conv over frames
    name = "rvc_conv1d_frames_bf16x3"
    xc = _planes(torch.randn(128, 20, generator=g).to(dev), 128, "zero")
    ac = native.gemm_bf16x3_pack_weight(torch.randn(128, 160, generator=g), dev)
    f = lib.rvc_conv1d_frames_bf16x3
    refused(name, f(xc.data_ptr(), 128, 128, 20, 8, 1, ac.data_ptr(), None, y.data_ptr(), None, 128, 128, 0, st))                    # stride x channels = 20: not a multiple of 8
    refused(name, f(xs.data_ptr(), n, 256, k, 1, 1, a.data_ptr(), None, y.data_ptr(), None, 256, m, 2, st))                          # mode 2
    refused(name, f(xs.data_ptr(), n, 256, k, 1, 1, a.data_ptr(), None, y.data_ptr(), None, 100, m, 0, st))                          # n_frames_out_padded % 128
    refused(name, f(xs.data_ptr(), n, 256, k, 1, 1, a.data_ptr(), None, None, ys.data_ptr(), 256, m, 0, st))                         # mode 0 without y
    refused(name, f(xs.data_ptr(), n, 256, k, 0, 1, a.data_ptr(), None, y.data_ptr(), None, 256, m, 0, st))                          # taps
    # LayerNorm
    name = "rvc_bias_residual_layernorm_bf16x3"
    parts = torch.randn(1, 4, 512, generator=g).to(dev)
    yl, yls = out((4, 512)), out((3, 128, 512), torch.bfloat16)
    f = lib.rvc_bias_residual_layernorm_bf16x3
    refused(name, f(parts.data_ptr(), 1, None, None, None, None, 1e-5, yl.data_ptr(), yls.data_ptr(), 4, 128, 512, st))               # features
    refused(name, f(parts.data_ptr(), 0, None, None, None, None, 1e-5, yl.data_ptr(), yls.data_ptr(), 4, 128, 256, st))               # n_parts
    refused(name, f(parts.data_ptr(), 1, None, None, None, None, 1e-5, None, None, 4, 128, 256, st))                                  # no output at all
    # K13
    name = "rvc_hubert_conv0_frames_bf16x3"
    wav = torch.randn(410, generator=g).to(dev)
    w0 = torch.randn(512 * 10, generator=g).to(dev)
    ws = torch.zeros(1024 * 136, dtype=torch.uint8, device=dev)
    y13 = out((3, 128, 512), torch.bfloat16)
    f = lib.rvc_hubert_conv0_frames_bf16x3
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 512, 9, 5, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 128, st))    # taps
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 96, 10, 5, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 128, st))    # channels % 64
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 1088, 10, 5, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 128, st))  # channels > 1024
    refused(name, f(wav.data_ptr(), 9, w0.data_ptr(), 512, 10, 5, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 128, st))     # shorter than one window
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 512, 10, 5, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 80, st))    # 81 frames into 80 rows
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 512, 10, 0, None, None, 1e-5, ws.data_ptr(), ws.numel(), y13.data_ptr(), 128, st))   # stride
    refused(name, f(wav.data_ptr(), 410, w0.data_ptr(), 512, 10, 5, None, None, 1e-5, ws.data_ptr(), 512 * 136 - 1, y13.data_ptr(), 128, st))  # workspace one byte short
    # K14
    name = "rvc_posconv_gelu_bf16x3"
    xp = torch.randn(50, 96, generator=g).to(dev)
    ap = native.posconv_bf16x3_pack_weight(torch.randn(96, 48, 5, generator=g), 2, dev)
    yp14 = out((50, 96))
    f = lib.rvc_posconv_gelu_bf16x3
    refused(name, f(xp.data_ptr(), ap.data_ptr(), None, yp14.data_ptr(), 50, 96, 2, 5, 5, st))                                       # padding == taps
    refused(name, f(xp.data_ptr(), ap.data_ptr(), None, yp14.data_ptr(), 50, 96, 2, 5, -1, st))
    refused(name, f(xp.data_ptr(), ap.data_ptr(), None, yp14.data_ptr(), 50, 96, 1, 5, 2, st))                                       # 96 channels per group
    refused(name, f(xp.data_ptr(), ap.data_ptr(), None, yp14.data_ptr(), 50, 96, 2, 129, 2, st))                                     # taps
    # attention
    name = "rvc_attention_qkv_f32"
    frames, heads = 300, 2
    f = lib.rvc_attention_qkv_f32
    for hd in (64, 96):
        qkv = torch.randn(1, frames, 3 * heads * hd, generator=g).to(dev)
        ek, ev = _rel_embeddings(hd, g, dev)
        o = out((1, frames, heads * hd))
        need = ctypes.c_size_t()
        assert lib.rvc_attention_workspace_bytes(1, frames, heads, hd, ctypes.byref(need)) == 0 and _att_plan(1, frames, heads, hd, False)[1] > 1
        wsa = torch.zeros(need.value, dtype=torch.uint8, device=dev)
        refused(name, f(qkv.data_ptr(), ek.data_ptr(), None, o.data_ptr(), 1, frames, heads, hd, 0.125, wsa.data_ptr(), need.value, st))    # one emb_rel pointer alone
        refused(name, f(qkv.data_ptr(), None, ev.data_ptr(), o.data_ptr(), 1, frames, heads, hd, 0.125, wsa.data_ptr(), need.value, st))
        refused(name, f(qkv.data_ptr(), None, None, o.data_ptr(), 1, frames, heads, hd, 0.125, wsa.data_ptr(), need.value - 1, st))       # workspace one byte short
        refused(name, f(qkv.data_ptr(), None, None, o.data_ptr(), 1, frames, heads, hd // 2, 0.125, wsa.data_ptr(), need.value, st))      # head_dim 32 / 48
        refused(name, f(qkv.data_ptr(), None, None, o.data_ptr(), 0, frames, heads, hd, 0.125, wsa.data_ptr(), need.value, st))           # batch
