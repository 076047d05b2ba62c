"""K6 (csrc/filtfilt.hip: rvc_filtfilt_order5) against an extended-precision evaluation of the same filtfilt, at a gate derived from
SciPy's own float64 error on each input (tests/_filtfilt_ref.py: gate = 4 x floor + 2^-48 max|x|); K17's lfilter (which shares
iir5.h) on the same signal families.  tests/test_filtfilt_ref_cpu.py shows, without a GPU, that every gate stays under
1e-4 max|x| and that the kernel's scheme passes every one of these cases.

Measured on an MI355X, n = 40 000: max error / floor (floor = SciPy's own error against the extended-precision answer).  `before`
is the library with its fixed 4096-term table tabulated in plain long double.

    signal          48 Hz @ 16 kHz (4096 terms)   20 Hz @ 16 kHz (9856 terms)    48 Hz @ 48 kHz (12288 terms)
                    floor    now    before        floor    now    before         floor    now    before
    uniform +-0.3   1.9e-8   0.90   1.05          9.9e-7   0.81   15.0           2.3e-6   0.64   52.6
    uniform +-1.0   7.5e-8   0.91   0.82          4.0e-6   0.48   6.21           8.2e-6   0.71   25.2
    DC 1.0          1.7e-8   1.59   1.81          6.8e-7   1.82   86.6           2.1e-6   0.92   226
    DC 0.5 + noise  2.7e-8   0.85   1.31          1.2e-6   0.98   26.3           3.2e-6   0.62   76.7
    sine 5 Hz       1.2e-8   2.87   4.16 (fails)  7.9e-7   1.49   67.9           1.6e-6   1.63   268
    sine 30 Hz      1.3e-8   2.25   2.27          3.9e-6   0.94   12.8           1.5e-6   2.30   239
    step            1.8e-8   1.72   1.21          9.4e-7   1.33   63.8           2.2e-6   0.96   211
    impulses (7)    <= 1e-8  <= 2.01  <= 2.66     <= 8e-7  <= 2.76  <= 230       <= 2e-6  <= 3.81  <= 553

`before`, the largest errors were 7.0e-5 (20 Hz @ 16 kHz) and 6.0e-4 (48 Hz @ 48 kHz), both on the impulse at x[0]; now 3.7e-6
and 5.8e-6, SciPy's own level.  The 5 Hz sine with the product's coefficients was a second finding: 4.8e-8 against a gate of
4.6e-8, not from the table's length (8192 terms: 3.7 x) but from its entries, which the long double recurrence left 6e-12 of
the peak off; tabulated in pairs of long doubles it is 3.3e-8 (2.87 x).  The 4000 Hz low-pass (128 terms) and the pure FIR
(64 terms) sit at 1.00 x floor on every signal, errors of 2e-17 to 7e-16.  All zeros give exact zeros.  Geometry (30 lengths x 2
signals, product's coefficients): <= 2.57 x floor, single-chunk lengths bit-exact.  K17's lfilter on DC, the 5 Hz sine, the step
and +-1 noise: <= 1.23 x floor at 32 kHz, 1.00 x at 48 kHz.  No case needed more than the gate's 2^-48 max|x| term."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import signal

import _filtfilt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LF_CHUNK = 2048          # csrc/preprocess.hip
SIGNALS = ["uniform_0.3", "uniform_1.0", "dc_1.0", "dc_0.5_noise", "sine_5hz", "sine_30hz", "step", "zeros", "imp_first", "imp_last",
           "imp_dropped", "imp_below_W", "imp_at_W", "imp_x0", "imp_xend"]
OTHER_SETS = [s for s in R.GATED_SETS if s != R.PRODUCT]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _run(native, set_name, x):
    b, a, _, _ = R.coef_sets()[set_name]
    return native.filtfilt_order5(_dev(x), b, a).cpu().numpy()


def _check_case(native, set_name, tag, case):
    got = _run(native, set_name, case.x)
    assert got.shape == case.x.shape
    err, _ = R.report(f"filtfilt {set_name} {tag}", got, case)
    assert np.isfinite(got).all()
    assert err <= case.gate, (set_name, tag, err, case.floor, case.gate)
    return got


# ---- 1. the sizing rule ---------------------------------------------------------------------------------------------------------------
def test_table_length_follows_the_coefficients(native):
    """4096 terms for the pipeline's filter (the hot path keeps its cost); every other set gets what the rule, mirrored in
    _filtfilt_ref.ff_terms, gives."""
    assert SIGNALS == list(R.signals_for(16000, 4096))
    for name, (b, a, zi, _) in R.coef_sets().items():
        terms = native.filtfilt_terms(b, a)
        print(f"filtfilt {name}: {terms} terms, pole radius {np.abs(np.roots(a)).max() if np.any(a[1:]) else 0.0:.6f}")
        assert terms == R.ff_terms(b, a, zi) and terms % 64 == 0, (name, terms)
    b, a, _, _ = R.coef_sets()[R.PRODUCT]
    assert native.filtfilt_terms(b, a) == 4096


# ---- 2. signals, the product's coefficients --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIGNALS)
def test_signals_with_the_products_coefficients(native, name):
    case = R.signal_cases(R.PRODUCT)[name]
    got = _check_case(native, R.PRODUCT, name, case)
    if name == "zeros":
        assert case.gate == 0.0 and not got.any()


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.geometry_lengths())
def test_geometry_with_the_products_coefficients(native, n):
    cases = R.geometry_cases()
    for kind in ("noise", "dc_noise"):
        case = cases[(n, kind)]
        got = _check_case(native, R.PRODUCT, f"n={n} ({(n + 2 * R.PAD) % R.CHUNK} past {(n + 2 * R.PAD) // R.CHUNK} chunks) {kind}", case)
        if n + 2 * R.PAD <= R.CHUNK:      # a single chunk from the exact start state: SciPy's own operations, SciPy's bits
            assert np.array_equal(got, case.scipy), (n, kind)


# ---- 4. other coefficient sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIGNALS)
@pytest.mark.parametrize("set_name", OTHER_SETS)
def test_signals_with_other_coefficients(native, set_name, name):
    case = R.signal_cases(set_name)[name]
    got = _check_case(native, set_name, name, case)
    if name == "zeros":
        assert not got.any()


# ---- 5. the table cache, the workspace, the stream ----------------------------------------------------------------------------------------
def test_alternating_coefficient_sets_give_each_sets_own_bits(native):
    x = R.signal_cases(R.PRODUCT)["dc_0.5_noise"].x
    sets = (R.PRODUCT, "hp20_16k")
    alone = {s: _run(native, s, x) for s in sets}
    assert not np.array_equal(alone[sets[0]], alone[sets[1]])
    for _ in range(3):
        for s in sets:
            assert np.array_equal(_run(native, s, x), alone[s]), s


def test_result_does_not_depend_on_the_workspace_or_the_stream(native):
    b, a, _, _ = R.coef_sets()[R.PRODUCT]
    x = _dev(R.signal_cases(R.PRODUCT)["dc_0.5_noise"].x)
    first = native.filtfilt_order5(x, b, a)
    assert torch.equal(native.filtfilt_order5(x, b, a), first)                       # two identical calls
    need = native._size("rvc_filtfilt_workspace_bytes", x.device, x.numel())
    ws = native._ws.get("filtfilt", need, x.device)
    assert ws.numel() >= need
    ws.fill_(0xFF)                                                                   # every double of the cached workspace a NaN
    assert torch.isnan(ws[: need // 8 * 8].view(torch.float64)).all()
    assert torch.equal(native.filtfilt_order5(x, b, a), first)
    # a workspace of this test's own, poisoned, exactly as large as asked for, through the binding's call path
    own = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x)
    coef = native._filtfilt_coef(b, a)
    native._call("rvc_filtfilt_order5", x.device, x.data_ptr(), x.numel(), coef.ctypes.data, y.data_ptr(), own.data_ptr(), need)
    assert torch.equal(y, first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        on_side = native.filtfilt_order5(x, b, a)
    side.synchronize()
    assert torch.equal(on_side, first)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_entry_and_write_nothing(native):
    """One call per constraint, violating it alone, with real device buffers: non-zero return, a message that starts with the
    entry's name, the output still full of its sentinel."""
    lib, st = native._lib, native._stream()
    n = 5000
    x = _dev(np.random.default_rng(5).uniform(-0.3, 0.3, n))
    y = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    need = native._size("rvc_filtfilt_workspace_bytes", x.device, n)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    b, a, zi, _ = R.coef_sets()[R.PRODUCT]
    good = np.ascontiguousarray(np.concatenate([b, a, zi]))

    def refused(what, coef=good, n=n, ws_bytes=need, expect=None):
        plant = ctypes.c_size_t()
        assert lib.rvc_knn_workspace_bytes(100, 10, 768, 5, ctypes.byref(plant)) != 0       # another call's error text
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        rc = lib.rvc_filtfilt_order5(x.data_ptr(), n, coef.ctypes.data, y.data_ptr(), ws.data_ptr(), ws_bytes, st)
        msg = lib.rvc_last_error().decode()
        torch.cuda.synchronize()
        print(f"refusal ({what}): rc {rc}, {msg!r}")
        assert rc != 0, f"{what}: accepted"
        assert msg.startswith("rvc_filtfilt_order5: ") and len(msg) > len("rvc_filtfilt_order5: "), (what, msg)
        assert expect is None or expect in msg, (what, msg)
        assert bool((y == 7.0).all()), f"{what}: a refused call wrote into its output"

    for k, v in ((2, np.nan), (0, np.inf), (8, -np.inf), (14, np.nan)):
        bad = good.copy()
        bad[k] = v
        refused(f"coef[{k}] = {v}", coef=bad, expect="non-finite")
    refused("a pole at radius 2.5", coef=np.concatenate([b, [1.0, -2.5, 0, 0, 0, 0], zi]), expect="unstable")
    a_circle = np.real(np.poly([-1.0, 0.5, -0.5, 0.3j, -0.3j]))                        # a pole at z = -1, radius exactly 1
    refused("a pole on the unit circle", coef=np.concatenate([b, a_circle, zi]), expect="pole radius")
    # stable, but so slow that the table would pass 2^17 terms: five well separated poles at radius 0.99995
    r = 0.99995
    a_slow = np.real(np.poly([r, r * np.exp(0.3j), r * np.exp(-0.3j), r * np.exp(1.0j), r * np.exp(-1.0j)]))
    b_slow = np.array([1.0, 0, 0, 0, 0, 0])
    assert a_slow[0] == 1.0 and np.abs(np.roots(a_slow)).max() < 1.0
    refused("poles at radius 0.99995", coef=np.concatenate([b_slow, a_slow, signal.lfilter_zi(b_slow, a_slow)]), expect="pole radius 0.9999")
    # the 1 Hz high-pass at 48 kHz: its poles are slower still (its float64 a[] has even lost its stability to rounding)
    b1, a1 = signal.butter(5, 1, "high", fs=48000)
    refused("butter(5, 1, 'high', fs=48000)", coef=np.concatenate([b1, a1, np.zeros(5)]), expect="pole radius")
    refused("workspace one byte short", ws_bytes=need - 1, expect="workspace too small")
    refused("n = 18", n=18)
    refused("n = 0", n=0)
    # and the call the refusals vary is itself accepted
    assert lib.rvc_filtfilt_order5(x.data_ptr(), n, good.ctypes.data, y.data_ptr(), ws.data_ptr(), need, st) == 0, lib.rvc_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), _run(native, R.PRODUCT, x.cpu().numpy()))
    with pytest.raises(native.NativeError, match="non-finite"):
        native.filtfilt_terms([np.nan] + list(b[1:]), a)


# ---- 7. K17's lfilter on the same signal families ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [32000, 48000])
def test_lfilter_on_the_filtfilt_signal_families(native, fs):
    """rvc_lfilter_order5_f64 shares ff_step and the tile movement: DC, a sub-cutoff sine, a step and +-1 noise, against the forward-only
    extended reference at the same gate, over the warm-up and three chunks past it."""
    b, a = signal.butter(5, 48, "high", fs=fs)
    warm = native.lfilter_warmup(b, a)
    n = warm + 3 * LF_CHUNK + 5
    t = np.arange(n) / fs
    sigs = {"dc_1.0": np.full(n, 1.0), "sine_5hz": np.sin(2 * np.pi * 5 * t), "step": (np.arange(n) >= n // 2).astype(np.float64),
            "uniform_1.0": np.random.default_rng(fs).uniform(-1.0, 1.0, n)}
    exts = R.lfilter_ext(b, a, list(sigs.values()))
    for (name, x), ext in zip(sigs.items(), exts):
        case = R.Case(x, ext)
        case.floor, case.gate = R.gate_of(x, signal.lfilter(b, a, x), ext)
        got = native.lfilter_order5(_dev(x), b, a).cpu().numpy()
        err, _ = R.report(f"lfilter fs={fs} warm-up {warm} n={n} {name}", got, case)
        assert case.gate <= 1e-4 * np.abs(x).max()                     # the gate cannot hide a failure
        assert err <= case.gate, (fs, name, err, case.floor, case.gate)
