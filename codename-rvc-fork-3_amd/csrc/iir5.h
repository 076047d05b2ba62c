// The 5th-order float64 recurrence step and the LDS tile movement shared by K6 (filtfilt.hip: zero-phase high-pass of the
// inference pipeline) and K17 (preprocess.hip: the causal high-pass of the dataset preprocessor).  Both run one lane per chunk
// of consecutive samples, 64 chunks per wave, and move their samples through LDS in [64 chunks] x [FF_SB steps] tiles.
#pragma once

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
