// The 5th-order float64 recurrence step and the LDS tile movement shared by K6 (filtfilt.hip: zero-phase high-pass of the
// inference pipeline) and K17 (preprocess.hip: the causal high-pass of the dataset preprocessor).  Both run one lane per chunk
// of consecutive samples, 64 chunks per wave, and move their samples through LDS in [64 chunks] x [FF_SB steps] tiles.  Both size
// what stands in front of a chunk from the filter's poles (pole_radius, host side).
#pragma once

#include <math.h>

#include "common.h"

namespace rvc {

constexpr int FF_ORD = 5;

struct FiltCoef {
    double b[FF_ORD + 1];
    double a[FF_ORD + 1];
    double zi[FF_ORD];
};

__device__ __forceinline__ double ff_step(const FiltCoef &c, double xv, double z[FF_ORD]) {
#pragma clang fp contract(off)
    // scipy/signal/_lfilter.c.src: y = z0 + b0*x;  z_i = z_{i+1} + x*b_{i+1} - y*a_{i+1};  z_last = x*b_n - y*a_n
    // plain operators under contract(off): the __dmul_rn/__dadd_rn helpers are ordinary operators that clang fuses.
    // Same operations and operand order as SciPy's, written so that only three of the 21 are on the step-to-step
    // dependency chain (y, y*a1, z0): a float64 VALU result takes ~25 cycles to come back, and the straightforward
    // order (mul, dependent add, mul, dependent add, ...) made every one of them wait -- 550 cycles per sample.
    double xb[FF_ORD + 1], t[FF_ORD], ya[FF_ORD];
#pragma unroll
    for (int i = 0; i <= FF_ORD; ++i) xb[i] = xv * c.b[i];          // independent of the state
    const double y = z[0] + xb[0];
#pragma unroll
    for (int i = 0; i < FF_ORD - 1; ++i) t[i] = z[i + 1] + xb[i + 1];   // independent of y
#pragma unroll
    for (int i = 0; i < FF_ORD; ++i) ya[i] = y * c.a[i + 1];
#pragma unroll
    for (int i = 0; i < FF_ORD - 1; ++i) z[i] = t[i] - ya[i];
    z[FF_ORD - 1] = xb[FF_ORD] - ya[FF_ORD - 1];
    return y;
}

// largest root radius of z^5 + a[1] z^4 + ... + a[5] (Durand-Kerner in long double; the five Butterworth poles are simple).
// Host side: K17 sizes its warm-up from it, K6 refuses unstable filters with it and names it when a table would be too long.
inline bool pole_radius(const double *a, double *rho_out) {
    typedef long double L;
    L re[FF_ORD], im[FF_ORD];
    for (int k = 0; k < FF_ORD; ++k) {   // start values on a circle, at no symmetric position
        const L ang = 0.4L + 2.0L * 3.14159265358979323846L * k / FF_ORD;
        re[k] = 0.9L * cosl(ang);
        im[k] = 0.9L * sinl(ang);
    }
    for (int it = 0; it < 500; ++it) {
        L moved = 0;
        for (int k = 0; k < FF_ORD; ++k) {
            L pr = 1, pi = 0;                         // p(z_k), Horner
            for (int c = 1; c <= FF_ORD; ++c) {
                const L nr = pr * re[k] - pi * im[k] + (L)a[c], ni = pr * im[k] + pi * re[k];
                pr = nr;
                pi = ni;
            }
            L dr = 1, di = 0;                         // prod_{j != k} (z_k - z_j)
            for (int j = 0; j < FF_ORD; ++j) {
                if (j == k) continue;
                const L er = re[k] - re[j], ei = im[k] - im[j];
                const L nr = dr * er - di * ei, ni = dr * ei + di * er;
                dr = nr;
                di = ni;
            }
            const L den = dr * dr + di * di;
            if (!(den > 0)) return false;
            const L qr = (pr * dr + pi * di) / den, qi = (pi * dr - pr * di) / den;
            re[k] -= qr;
            im[k] -= qi;
            moved = fmaxl(moved, fabsl(qr) + fabsl(qi));
        }
        if (!(moved == moved)) return false;          // NaN
        // converged to the rounding noise of p(z) over the cluster's separations (~1e-8 of a pole 2e-3 inside the circle at
        // 48 kHz: nothing against the rule's 53 bits); the iteration is quadratic from here, one more step would only jitter
        if (moved < 1e-6L) {
            L best = 0;
            for (int k = 0; k < FF_ORD; ++k) best = fmaxl(best, sqrtl(re[k] * re[k] + im[k] * im[k]));
            *rho_out = (double)best;
            return true;
        }
    }
    return false;
}

// One wave = 64 consecutive chunks, one lane per chunk.  A lane walks its chunk sequentially, so a naive load touches
// 64 different cache lines per step; instead the wave moves data in [64 chunks] x [32 steps] tiles through LDS: tile
// rows are fetched as contiguous 256-byte pieces (two chunk rows per load instruction), one step-block ahead of the
// recurrence, and the outputs of a step-block leave the same way.
constexpr int FF_SB = 32;              // steps per tile
constexpr int FF_TS = FF_SB + 1;       // tile row stride in doubles (conflict-free ds_read_b64 down a column)

// row-wise side of a tile (the global-memory side): register k of lane (hrow = lane >> 5, u = lane & 31) is element
// (row 2k + hrow, column u)
__device__ __forceinline__ void ff_tile_put_rows(double *tile, const double (&r)[32], int hrow, int u) {
#pragma unroll
    for (int k = 0; k < 32; ++k) tile[(2 * k + hrow) * FF_TS + u] = r[k];
}
__device__ __forceinline__ void ff_tile_get_rows(const double *tile, double (&r)[32], int hrow, int u) {
#pragma unroll
    for (int k = 0; k < 32; ++k) r[k] = tile[(2 * k + hrow) * FF_TS + u];
}
// lane-wise side (the recurrence's side): 8 consecutive steps of this lane's own row
__device__ __forceinline__ void ff_tile_get8(const double *tile, int lane, int s8, double (&v)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = tile[lane * FF_TS + s8 + q];
}
__device__ __forceinline__ void ff_tile_put8(double *tile, int lane, int s8, const double (&v)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) tile[lane * FF_TS + s8 + q] = v[q];
}

}  // namespace rvc
