"""An extended-precision yardstick for K6 (csrc/filtfilt.hip) and K17's lfilter (csrc/preprocess.hip), shared by
test_filtfilt_ref_cpu.py and test_filtfilt_gpu.py.

* filtfilt_ext / lfilter_ext: scipy.signal.filtfilt(b, a, x) / lfilter(b, a, x) restated from the definition in numpy.longdouble
  (80-bit on x86-64): odd extension by 18, transposed direct form II forward from zi * ext[0], the same backward from
  zi * y[-1], crop.  b, a, zi are the float64 values the kernel receives; zi is an argument, never recomputed.
* gate: 4 x SciPy's own float64 error on the same input (the project's margin over a reference's noise floor, as
  test_preprocess_gpu._lfilter_gate) + 2^-48 max|x| (about 16 ulp: only matters for well-conditioned filters, where the kernel's
  start state comes from a differently ordered, more accurate sum than SciPy's sequential one).
* ff_terms: the Python mirror of the library's table-sizing rule (rvc_filtfilt_order5_terms).
* emulate_kernel: the kernel's scheme in NumPy -- chunks of 512, each chunk's start state a dot product with the truncated
  table, SciPy's own float64 recurrence inside a chunk, both passes.  On an MI355X the kernel's errors agreed with it to four
  digits.
* the cases (coefficient sets, signals, lengths) of both test modules, so that the CPU module proves exactly what the GPU module
  runs."""
import decimal
import functools
from decimal import Decimal as D

import numpy as np
from scipy import signal

L = np.longdouble
PAD = 18                  # scipy.signal.filtfilt's default padlen for a 5th-order filter: 3 * max(len(a), len(b))
CHUNK = 512               # FF_CHUNK, csrc/filtfilt.hip
ORD = 5
FF_LEVEL = 2e-11          # FF_TAB_LEVEL, csrc/filtfilt.hip
FF_RUN = 64               # FF_TAB_RUN
FF_TERMS_MAX = 1 << 17    # FF_TERMS_MAX
N_SIG = 40000


# ---- the reference --------------------------------------------------------------------------------------------------------------
def _lfilter_rows(b, a, X, Z):
    """Transposed direct form II over the rows of X [S, N] (longdouble) from the states Z (ORD arrays [S]); -> Y [S, N]."""
    bl, al = [L(v) for v in b], [L(v) for v in a]
    z = [np.array(v, dtype=L) for v in Z]
    Y = np.empty_like(X)
    XT = np.ascontiguousarray(X.T)
    YT = np.empty_like(XT)
    for i in range(XT.shape[0]):
        x = XT[i]
        y = z[0] + bl[0] * x
        for k in range(ORD - 1):
            z[k] = z[k + 1] + bl[k + 1] * x - al[k + 1] * y
        z[ORD - 1] = bl[ORD] * x - al[ORD] * y
        YT[i] = y
    Y[:] = YT.T
    return Y


def _odd_ext(x):
    return np.concatenate([2 * x[0] - x[PAD:0:-1], x, 2 * x[-1] - x[-2:-(PAD + 2):-1]])


def filtfilt_ext(b, a, zi, xs):
    """scipy.signal.filtfilt(b, a, x) for every 1-D float64 x in `xs` (any lengths > PAD), in longdouble -> list of longdouble arrays.
    Signals of different lengths share the sample loop: rows are left-aligned and zero-filled, what a row computes past its own
    end is dropped."""
    exts = [_odd_ext(np.asarray(x, dtype=L)) for x in xs]
    S, N = len(exts), max(len(e) for e in exts)
    X = np.zeros((S, N), dtype=L)
    for s, e in enumerate(exts):
        X[s, :len(e)] = e
    zl = [L(v) for v in zi]
    Y = _lfilter_rows(b, a, X, [zl[k] * X[:, 0] for k in range(ORD)])
    R = np.zeros_like(X)
    for s, e in enumerate(exts):
        R[s, :len(e)] = Y[s, :len(e)][::-1]
    Z = _lfilter_rows(b, a, R, [zl[k] * R[:, 0] for k in range(ORD)])
    return [Z[s, :len(e)][::-1][PAD:-PAD].copy() for s, e in enumerate(exts)]


def lfilter_ext(b, a, xs):
    """scipy.signal.lfilter(b, a, x) from a zero state for every x in `xs` (equal lengths), in longdouble."""
    X = np.stack([np.asarray(x, dtype=L) for x in xs])
    Y = _lfilter_rows(b, a, X, [np.zeros(len(xs), dtype=L)] * ORD)
    return [Y[s] for s in range(len(xs))]


def gate_of(x, scipy_y, ext_y):
    """-> (floor, gate): SciPy's own float64 error on this input, and what the kernel is held to."""
    floor = float(np.abs(np.asarray(scipy_y, dtype=L) - ext_y).max())
    return floor, 4.0 * floor + 2.0 ** -48 * float(np.abs(x).max())


# ---- the sizing rule ----------------------------------------------------------------------------------------------------------------
# The responses obey the filter's own ill-conditioned recurrence: run in longdouble they come out 6e-12 of their peak off, as much as
# the tail the table drops.  They are tabulated in 60-digit decimal arithmetic (the float64 coefficients convert exactly).
def _exact():
    return decimal.localcontext(decimal.Context(prec=60))


def _response_steps(b, a, zi, n_max):
    """Yields (j, g, s): g = A^j B (a unit input sample's state j steps later) and s = A^j zi as lists of ORD Decimals, j < n_max.
    To be consumed under _exact()."""
    al = [D(float(v)) for v in a]
    g = [D(float(b[i + 1])) - al[i + 1] * D(float(b[0])) for i in range(ORD)]
    s = [D(float(v)) for v in zi]
    for j in range(n_max):
        yield j, g, s
        for v in (g, s):
            v0 = v[0]
            for i in range(ORD - 1):
                v[i] = v[i + 1] - al[i + 1] * v0
            v[ORD - 1] = -al[ORD] * v0


def _to_longdouble(v):
    hi = float(v)
    return L(hi) + L(float(v - D(hi)))


def _responses(b, a, zi, n_terms):
    """G[j], S[j], j < n_terms, rounded to longdouble: [n_terms, ORD] each (tabulated once per coefficient set and length)."""
    return _responses_cached(tuple(map(float, b)), tuple(map(float, a)), tuple(map(float, zi)), n_terms)


@functools.lru_cache(maxsize=None)
def _responses_cached(b, a, zi, n_terms):
    G, Sr = np.empty((n_terms, ORD), dtype=L), np.empty((n_terms, ORD), dtype=L)
    with _exact():
        for j, g, s in _response_steps(b, a, zi, n_terms):
            G[j], Sr[j] = [_to_longdouble(v) for v in g], [_to_longdouble(v) for v in s]
    return G, Sr


def ff_terms(b, a, zi):
    """The table length of csrc/filtfilt.hip for these coefficients: p = the first term from which both response envelopes
    (max over the five state variables, relative to the response's largest value so far) stay below FF_LEVEL for FF_RUN terms in
    a row; the length is the first multiple of 64 past p.  None when that takes more than FF_TERMS_MAX terms."""
    with _exact():
        level, max_g, max_s, run = D(FF_LEVEL), D(0), D(0), 0
        for j, g, s in _response_steps(b, a, zi, FF_TERMS_MAX):
            eg, es = max(abs(v) for v in g), max(abs(v) for v in s)
            max_g, max_s = max(max_g, eg), max(max_s, es)
            run = run + 1 if (eg <= level * max_g and es <= level * max_s) else 0
            if run == FF_RUN:
                return ((j - (FF_RUN - 1)) // 64 + 1) * 64
    return None


# ---- the kernel's scheme ------------------------------------------------------------------------------------------------------------
def _emulate_pass(b, a, zi, u, G, Sr):
    W, ne = len(G), len(u)
    ul = u.astype(L)
    y = np.empty(ne)
    for i0 in range(0, ne, CHUNK):
        if i0 == 0:
            z = zi * u[0]
        else:
            nt = min(i0, W)
            zl = ul[i0 - nt:i0][::-1] @ G[:nt]
            if i0 < W:
                zl = zl + Sr[i0] * ul[0]
            z = zl.astype(np.float64)
        y[i0:i0 + CHUNK], _ = signal.lfilter(b, a, u[i0:i0 + CHUNK], zi=z)
    return y


def emulate_kernel(b, a, zi, x, terms):
    """What csrc/filtfilt.hip computes, with its double-double sums replaced by longdouble ones."""
    G, Sr = _responses(b, a, zi, terms)
    yf = _emulate_pass(b, a, zi, _odd_ext(np.asarray(x, dtype=np.float64)), G, Sr)
    return _emulate_pass(b, a, zi, yf[::-1].copy(), G, Sr)[::-1][PAD:-PAD]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def coef_sets():
    """name -> (b, a, zi, fs): the product's set first; `fs` places the sines."""
    fir = (np.array([0.21, -0.47, 0.33, 0.55, -0.29, 0.12]), np.array([1.0, 0, 0, 0, 0, 0]))
    raw = {"hp48_16k": signal.butter(5, 48, "high", fs=16000) + (16000,),
           "hp20_16k": signal.butter(5, 20, "high", fs=16000) + (16000,),
           "hp48_48k": signal.butter(5, 48, "high", fs=48000) + (48000,),
           "lp4000_16k": signal.butter(5, 4000, "low", fs=16000) + (16000,),
           "fir": fir + (16000,)}
    return {k: (np.asarray(b, np.float64), np.asarray(a, np.float64), signal.lfilter_zi(b, a), fs) for k, (b, a, fs) in raw.items()}


PRODUCT = "hp48_16k"
GATED_SETS = ("hp48_16k", "hp20_16k", "hp48_48k", "lp4000_16k", "fir")


def impulse_positions(terms, n=N_SIG):
    """Extended-signal indices of single unit impulses that meet the first (i0 - 1) and the last (i0 - W) term of the state sum of
    a chunk starting at i0 >= W, the first dropped one (i0 - W - 1), and both sides of index W, where chunks stop adding the zi
    response; plus the two ends of the signal (the start states zi * ext[0] of both passes)."""
    i0 = CHUNK * (-(-(terms + 1024) // CHUNK))
    assert i0 + CHUNK < n
    return {"imp_first": i0 - 1, "imp_last": i0 - terms, "imp_dropped": i0 - terms - 1, "imp_below_W": terms - 1,
            "imp_at_W": terms, "imp_x0": PAD, "imp_xend": PAD + n - 1}


def signals_for(fs, terms, n=N_SIG):
    """name -> x [n] float64: the signal families of the issue, the same for every coefficient set but for the impulse places."""
    t = np.arange(n) / fs
    rng = np.random.default_rng(20261021)
    out = {"uniform_0.3": rng.uniform(-0.3, 0.3, n), "uniform_1.0": rng.uniform(-1.0, 1.0, n), "dc_1.0": np.full(n, 1.0),
           "dc_0.5_noise": 0.5 + rng.uniform(-0.3, 0.3, n), "sine_5hz": np.sin(2 * np.pi * 5 * t), "sine_30hz": np.sin(2 * np.pi * 30 * t),
           "step": (np.arange(n) >= n // 2).astype(np.float64), "zeros": np.zeros(n)}
    for name, e in impulse_positions(terms, n).items():
        x = np.zeros(n)
        x[e - PAD] = 1.0
        out[name] = x
    return out


def geometry_lengths():
    """The lengths of the geometry test (ne = n + 36): the minimum and one more; eight consecutive n (every ne % 8: the per-step tail);
    one chunk exactly and one sample more; ne = 512 k + {-1, 0, 1} around k = 2, 8, 9 (chunks that stop adding the zi response) and
    64, 65 (the second wave; n_chunks % 4 == 1 in the state kernel's 4-chunk blocks); n_chunks % 4 == 2 and 3; 128 chunks + 1."""
    ns = [19, 20] + list(range(1500, 1508)) + [476, 477]
    ns += [CHUNK * k + d - 2 * PAD for k in (2, 8, 9, 64, 65) for d in (-1, 0, 1)]
    ns += [CHUNK * 14 - 100 - 2 * PAD, CHUNK * 15 - 100 - 2 * PAD, CHUNK * 128 + 1 - 2 * PAD]
    return ns


def geometry_signals():
    """(n, kind) -> x: +-0.3 noise and DC 0.5 + noise per length."""
    rng = np.random.default_rng(20261022)
    out = {}
    for n in geometry_lengths():
        out[(n, "noise")] = rng.uniform(-0.3, 0.3, n)
        out[(n, "dc_noise")] = 0.5 + rng.uniform(-0.3, 0.3, n)
    return out


class Case:
    """One gated comparison: x, SciPy's float64 answer, the extended answer (rounded to float64 for comparing: its own rounding,
    2^-53 |y|, is far inside the gate's 2^-48 max|x| term), floor and gate."""

    def __init__(self, x, ext):
        self.x, self.ext = x, ext


@functools.lru_cache(maxsize=None)
def signal_cases(set_name):
    """name -> Case for every signal of one coefficient set (n = N_SIG); the references are computed once per process."""
    b, a, zi, fs = coef_sets()[set_name]
    terms = ff_terms(b, a, zi)
    sigs = signals_for(fs, terms)
    return _cases(b, a, zi, sigs)


@functools.lru_cache(maxsize=None)
def geometry_cases():
    b, a, zi, _ = coef_sets()[PRODUCT]
    return _cases(b, a, zi, geometry_signals())


def _cases(b, a, zi, sigs):
    names = list(sigs)
    exts = filtfilt_ext(b, a, zi, [sigs[k] for k in names])
    out = {}
    for k, e in zip(names, exts):
        c = Case(sigs[k], e)
        c.scipy = signal.filtfilt(b, a, sigs[k])
        c.floor, c.gate = gate_of(sigs[k], c.scipy, e)
        out[k] = c
    return out


def report(tag, got, case):
    """Print and return (err, worst index): measured error, floor, ratio and where in a chunk the worst sample sits."""
    d = np.abs(np.asarray(got, dtype=L) - case.ext)
    i = int(np.argmax(d))
    err = float(d[i])
    ratio = err / case.floor if case.floor > 0 else float("inf") if err > 0 else 0.0
    ne = len(d) + 2 * PAD
    print(f"{tag}: err {err:.3e}, floor {case.floor:.3e}, err/floor {ratio:.2f}, gate {case.gate:.3e}, worst sample {i} "
          f"(index % {CHUNK} in the forward pass {(i + PAD) % CHUNK}, in the backward pass {(ne - 1 - i - PAD) % CHUNK})")
    return err, i
