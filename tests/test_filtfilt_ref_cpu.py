"""The yardstick of tests/test_filtfilt_gpu.py, checked without a GPU (tests/_filtfilt_ref.py): the extended-precision filtfilt is
the same operation as scipy.signal.filtfilt; every gate the GPU module uses stays below 1e-4 max|x|, so it cannot hide a failure;
and the kernel's scheme -- chunks of 512, start states from a table cut where the sizing rule cuts it -- emulated in NumPy,
passes every one of those gates, so the cases are passable by the algorithm."""
import ctypes

import numpy as np
import pytest
from scipy import signal

import _filtfilt_ref as R


def test_extended_reference_is_scipys_filtfilt():
    """Well-conditioned low-pass: the two agree to float64 rounding, so the restatement is the same operation (odd extension, start
    states, both directions, crop)."""
    b, a = signal.butter(5, 4000, "low", fs=16000)
    zi = signal.lfilter_zi(b, a)
    rng = np.random.default_rng(1)
    xs = [rng.uniform(-1, 1, n) for n in (19, 20, 477, 3000)] + [0.5 + rng.uniform(-0.3, 0.3, 3000)]
    for x, e in zip(xs, R.filtfilt_ext(b, a, zi, xs)):
        assert e.dtype == np.longdouble and e.shape == x.shape
        assert float(np.abs(signal.filtfilt(b, a, x) - e).max()) <= 1e-14, len(x)
    # the forward-only variant against scipy.signal.lfilter
    for x, e in zip(xs[-2:], R.lfilter_ext(b, a, xs[-2:])):
        assert float(np.abs(signal.lfilter(b, a, x) - e).max()) <= 1e-14


def test_extended_reference_agrees_with_scipy_at_the_noise_floor_for_the_products_filter():
    """The 48 Hz high-pass is ill-conditioned: SciPy's float64 result is 2e-8 to 8e-8 off on +-0.3 .. +-1 signals, and no more."""
    cases = R.signal_cases(R.PRODUCT)
    for name in ("uniform_0.3", "uniform_1.0", "dc_1.0", "sine_5hz"):
        print(f"{name}: SciPy's own error {cases[name].floor:.3e}")
        assert 1e-9 < cases[name].floor < 2e-7, (name, cases[name].floor)
    assert cases["zeros"].floor == 0.0 and cases["zeros"].gate == 0.0


def test_sizing_rule_mirror():
    """The rule's lengths for the sets of the GPU module (which checks the library against this mirror): 4096 for the product's
    filter, by the choice of the level; longer tables for slower poles; short ones for fast poles and none."""
    want = {"hp48_16k": 4096, "hp20_16k": 9856, "hp48_48k": 12288, "lp4000_16k": 128, "fir": 64}
    for name, (b, a, zi, _) in R.coef_sets().items():
        assert R.ff_terms(b, a, zi) == want[name], name
    r = 0.99995
    a_slow = np.real(np.poly([r, r * np.exp(0.3j), r * np.exp(-0.3j), r * np.exp(1.0j), r * np.exp(-1.0j)]))
    b_slow = np.array([1.0, 0, 0, 0, 0, 0])
    assert R.ff_terms(b_slow, a_slow, signal.lfilter_zi(b_slow, a_slow)) is None            # past 2^17 terms: refused


def test_library_sizes_its_table_by_the_mirror():
    """rvc_filtfilt_order5_terms is host-only arithmetic: the same lengths from the library, and its refusals."""
    import __graft_entry__ as ge
    ge.build()
    from rvc_amd import _native
    lib = _native._lib
    terms = ctypes.c_int64()
    for name, (b, a, zi, _) in R.coef_sets().items():
        coef = np.ascontiguousarray(np.concatenate([b, a, zi]))
        assert lib.rvc_filtfilt_order5_terms(coef.ctypes.data, ctypes.byref(terms)) == 0, lib.rvc_last_error()
        assert terms.value == R.ff_terms(b, a, zi) == _native.filtfilt_terms(b, a), name
    b, a, zi, _ = R.coef_sets()[R.PRODUCT]
    good = np.concatenate([b, a, zi])

    def refused(coef, expect, out=terms):
        coef = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
        rc = lib.rvc_filtfilt_order5_terms(None if coef is None else coef.ctypes.data, None if out is None else ctypes.byref(out))
        msg = lib.rvc_last_error()
        assert rc != 0 and msg.startswith(b"rvc_filtfilt_order5_terms: ") and expect in msg, (rc, msg)

    refused(None, b"null pointer")
    refused(good, b"null pointer", out=None)
    for k in (0, 7, 16):
        bad = good.copy()
        bad[k] = np.nan if k != 7 else np.inf
        refused(bad, b"non-finite")
    bad = good.copy()
    bad[6] = 2.0
    refused(bad, b"a[0] must be 1")
    refused(np.concatenate([b, [1.0, -2.5, 0, 0, 0, 0], zi]), b"unstable filter (pole radius 2.5)")
    r = 0.99995
    a_slow = np.real(np.poly([r, r * np.exp(0.3j), r * np.exp(-0.3j), r * np.exp(1.0j), r * np.exp(-1.0j)]))
    refused(np.concatenate([[1.0, 0, 0, 0, 0, 0], a_slow, np.ones(5)]), b"pole radius 0.9999")


@pytest.mark.parametrize("set_name", R.GATED_SETS)
def test_gates_are_capped_and_the_kernels_scheme_passes_them(set_name):
    """Every (signal, n = 40000) case of one coefficient set: the gate is at most 1e-4 max|x|, and the emulated kernel is inside it."""
    b, a, zi, _ = R.coef_sets()[set_name]
    terms = R.ff_terms(b, a, zi)
    worst_cap = 0.0
    for name, case in R.signal_cases(set_name).items():
        top = float(np.abs(case.x).max())
        if top > 0:
            worst_cap = max(worst_cap, case.gate / (1e-4 * top))
            assert case.gate <= 1e-4 * top, (set_name, name, case.gate, top)
        err, _ = R.report(f"emulation {set_name} ({terms} terms) {name}", R.emulate_kernel(b, a, zi, case.x, terms), case)
        assert err <= case.gate, (set_name, name, err, case.floor, case.gate)
    print(f"{set_name}: largest gate / (1e-4 max|x|) = {worst_cap:.3f}")


def test_geometry_gates_are_capped_and_the_kernels_scheme_passes_them():
    b, a, zi, _ = R.coef_sets()[R.PRODUCT]
    ns = R.geometry_lengths()
    assert {(n + 2 * R.PAD) % 8 for n in ns[2:10]} == set(range(8)) and min(ns) == 19
    assert {-(-(n + 2 * R.PAD) // R.CHUNK) % 4 for n in ns} == {0, 1, 2, 3}
    for (n, kind), case in R.geometry_cases().items():
        top = float(np.abs(case.x).max())
        assert case.gate <= 1e-4 * top, (n, kind, case.gate)
        got = R.emulate_kernel(b, a, zi, case.x, 4096)
        err = float(np.abs(got.astype(R.L) - case.ext).max())
        assert err <= case.gate, (n, kind, err, case.floor, case.gate)
        if n + 2 * R.PAD <= R.CHUNK:
            assert np.array_equal(got, case.scipy), (n, kind)
