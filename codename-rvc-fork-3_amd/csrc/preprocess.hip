// K17 -- the dataset preprocessor's three device steps (rvc/train/preprocess/preprocess.py, slicer.py), float64 on the device so
// that a file is uploaded once and only the RMS list and the finished slices come back.
//
// 1. rvc_lfilter_order5_f64: `signal.lfilter(self.b_high, self.a_high, audio)` (preprocess.py:146), the causal 48 Hz Butterworth
//    high-pass at the dataset rate, from a zero state.  Same scheme as K6 (filtfilt.hip): SciPy's operation sequence with FMA
//    contraction off (ff_step, iir5.h), one lane per chunk of LF_CHUNK output samples, each lane starting `warm` samples early
//    from a zero state and writing only its own chunk.
//
//    WARM-UP RULE.  A zero start instead of the true state is a state error that decays like rho^k, rho the largest pole radius
//    of the coefficients handed in (the roots of z^5 + a1 z^4 + ... + a5, found on the host).  The warm-up is the smallest whole
//    number of step-blocks with rho^warm <= 2^-53: the error left is below one rounding of the states themselves.  The
//    pole moves towards 1 as the rate rises (0.99419 at 16 kHz, 0.99709 at 32 kHz, 0.99767 at 40 kHz, 0.99806 at 48 kHz), so the
//    rule gives 6 336 / 12 640 / 15 776 / 18 944 samples; K6's constant 4 096 would leave 3.5e-4 of the state at 48 kHz.
//    Chunks that begin inside the first `warm` samples read zeros in front of the signal: a zero state fed zeros stays
//    exactly zero, so they start from the true zero state at sample 0, as SciPy does, and the first chunk is bit-exact.
//
//    Accuracy: like K6's filter this direct form is ill-conditioned, more so at the higher rates: two runs of SciPy's own
//    recurrence started 65 536 samples apart differ by 2e-7 .. 4e-7 at 32 kHz and 1e-6 .. 3e-6 at 48 kHz on a +-0.5 signal
//    (DESIGN.md), which is the noise floor any chunked evaluation shares.
//
// 2. rvc_frame_rms_f64: `get_rms` (slicer.py:199-235).  Pass 1 sums the squares of every hop-long piece of the zero-padded
//    signal once (one wave per piece, lanes strided over it, a fixed xor-butterfly at the end); pass 2 adds frame_length / hop
//    consecutive pieces per frame in index order (plus frame_length % hop samples read directly when the frame is no whole
//    number of hops).  No atomics: bit-identical from run to run.
//
// 3. rvc_slice_export_f32: every slice of a file in one launch -- the float32 copy at the dataset rate and the 16 kHz copy,
//    each slice resampled ON ITS OWN (process_audio_segment / simple_cut resample the slice, not the file).  One thread per
//    output sample; the thread finds its slice by bisection in the packed offset table.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "iir5.h"

namespace rvc {

// ---- 1. causal lfilter ------------------------------------------------------------------------------------------------------
constexpr int LF_CHUNK = 2048;         // output samples per lane: 64 lanes x 2048 = 131 072 samples per wave
static_assert(LF_CHUNK % FF_SB == 0, "a chunk is whole step-blocks");

// One wave per block (64 chunks), LDS 2 x 64 x 33 x 8 = 33 KiB: four blocks per CU, one wave per SIMD.  The recurrence is bound
// by the ~25-cycle float64 dependency chain of ff_step, not by occupancy; the loads of the next step-block are in flight under it.
__global__ void __launch_bounds__(64)
lf_chunk_kernel(const double *__restrict__ x, int64_t n, FiltCoef c, int warm, int64_t n_chunks, double *__restrict__ y) {
    __shared__ double tin[64 * FF_TS];
    __shared__ double tout[64 * FF_TS];
    const int lane = threadIdx.x, u = lane & 31, hrow = lane >> 5;
    const int64_t ch0 = (int64_t)blockIdx.x * 64;
    double z[FF_ORD];
#pragma unroll
    for (int k = 0; k < FF_ORD; ++k) z[k] = 0.0;
    double r[32];
    uint32_t inside = 0;                              // bit k: r[k] is a sample of the signal (else a zero in front of or behind it)
    // element (row, column u) of step-block sb is sample (ch0 + row) * LF_CHUNK - warm + sb * FF_SB + u; zeros outside [0, n).
    // Unconditional loads from a clamped index; the zeros are applied when the tile is written a step-block later (zero_outside),
    // not here: touching a loaded value now would wait for the whole fetch before the recurrence it is meant to hide under.
    auto fetch = [&](int sb) __attribute__((always_inline)) {
        const int64_t base = (ch0 + hrow) * LF_CHUNK - warm + (int64_t)sb * FF_SB + u;
        inside = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int64_t i = base + (int64_t)2 * k * LF_CHUNK;
            const bool in = i >= 0 && i < n;
            inside |= (uint32_t)in << k;
            r[k] = x[in ? i : 0];
        }
    };
    auto zero_outside = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 32; ++k) r[k] = (inside >> k) & 1u ? r[k] : 0.0;
    };
    fetch(0);
    const int n_sb = (warm + LF_CHUNK) / FF_SB, out_sb0 = warm / FF_SB;
    for (int sb = 0; sb < n_sb; ++sb) {
        lds_barrier();                                // previous tile fully consumed
        zero_outside();
        ff_tile_put_rows(tin, r, hrow, u);
        if (sb + 1 < n_sb) fetch(sb + 1);
        lds_barrier();
        const bool emit = sb >= out_sb0;              // uniform
#pragma unroll
        for (int s8 = 0; s8 < FF_SB; s8 += 8) {
            double xin[8], yo[8];
            ff_tile_get8(tin, lane, s8, xin);
#pragma unroll
            for (int q = 0; q < 8; ++q) yo[q] = ff_step(c, xin[q], z);
            if (emit) ff_tile_put8(tout, lane, s8, yo);
        }
        if (emit) {
            lds_barrier();
            double yv[32];
            ff_tile_get_rows(tout, yv, hrow, u);
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const int64_t row_ch = ch0 + 2 * k + hrow;
                const int64_t i = row_ch * LF_CHUNK + (int64_t)(sb - out_sb0) * FF_SB + u;
                if (row_ch < n_chunks && i < n) y[i] = yv[k];
            }
        }
    }
}

// ---- 2. framed RMS ----------------------------------------------------------------------------------------------------------
// part[q] = sum of squares of padded samples [q * hop, (q + 1) * hop); padded sample k is x[k - pad], zero outside [0, n)
__global__ void __launch_bounds__(256)
rms_partial_kernel(const double *__restrict__ x, int64_t n, int64_t pad, int64_t hop, int64_t n_part, double *__restrict__ part) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_part) return;                          // whole waves leave together
    const int lane = threadIdx.x & 63;
    const int64_t lo = q * hop - pad;
    double acc = 0.0;
    for (int64_t k = lane; k < hop; k += 64) {
        const int64_t i = lo + k;
        const double v = (i >= 0 && i < n) ? x[i] : 0.0;
        acc = fma(v, v, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) part[q] = acc;
}

// frame t = part[t] + ... + part[t + m - 1] (m = frame_length / hop), then the frame_length % hop samples behind them
__global__ void __launch_bounds__(256)
rms_combine_kernel(const double *__restrict__ x, int64_t n, int64_t pad, int64_t hop, int64_t frame_length,
                   const double *__restrict__ part, double *__restrict__ out, int64_t n_frames) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_frames) return;
    const int64_t m = frame_length / hop, rest = frame_length % hop;
    double acc = 0.0;
    for (int64_t q = 0; q < m; ++q) acc += part[t + q];
    const int64_t lo = (t + m) * hop - pad;
    for (int64_t k = 0; k < rest; ++k) {
        const int64_t i = lo + k;
        const double v = (i >= 0 && i < n) ? x[i] : 0.0;
        acc = fma(v, v, acc);
    }
    out[t] = sqrt(acc / (double)frame_length);
}

// ---- 3. slice export --------------------------------------------------------------------------------------------------------
// the segment whose packed range [off[s], off[s + 1]) holds g (off: n_seg + 1 non-decreasing entries, off[0] = 0; empty segments
// are stepped over)
__device__ __forceinline__ int64_t seg_of(const int64_t *__restrict__ off, int64_t n_seg, int64_t g) {
    int64_t lo = 0, hi = n_seg;                       // invariant: off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// blocks [0, nb_full): full[g] = (float)x[start_s + g - off_full[s]];  blocks [nb_full, ...): the 16 kHz copies
__global__ void __launch_bounds__(256)
slice_export_kernel(const double *__restrict__ x, int64_t n, const int64_t *__restrict__ seg, const int64_t *__restrict__ off_full,
                    const int64_t *__restrict__ off_lo, int64_t n_seg, int up, int down, const double *__restrict__ h,
                    int64_t n_taps, float *__restrict__ full, int64_t n_full, float *__restrict__ lo, int64_t n_lo,
                    int64_t nb_full) {
    if ((int64_t)blockIdx.x < nb_full) {
        const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (g >= n_full) return;
        const int64_t s = seg_of(off_full, n_seg, g);
        const int64_t i = seg[2 * s] + (g - off_full[s]);
        if (i >= 0 && i < n && i < seg[2 * s + 1]) full[g] = (float)x[i];
        return;
    }
    const int64_t g = ((int64_t)blockIdx.x - nb_full) * blockDim.x + threadIdx.x;
    if (g >= n_lo) return;
    const int64_t s = seg_of(off_lo, n_seg, g);
    const int64_t start = seg[2 * s], len = seg[2 * s + 1] - start;
    const int64_t j = g - off_lo[s];
    if (start < 0 || len <= 0 || start + len > n) return;
    // rvc_resample_poly_f64's walk (elementwise.hip) over this segment alone: samples outside [start, start + len) are zeros
    const int64_t t = j * down + (n_taps - 1) / 2;    // position on the segment's up-sampled grid
    int64_t m = t % up;                               // smallest tap that meets a sample
    int64_t i = (t - m) / up;                         // that sample, relative to the segment
    if (i >= len) {
        m += (i - (len - 1)) * up;
        i = len - 1;
    }
    const double *xs = x + start;
    double acc = 0.0;
    for (; m < n_taps && i >= 0; m += up, --i) acc = fma(h[m], xs[i], acc);
    lo[g] = (float)acc;
}

constexpr int64_t LF_WARM_MAX = (int64_t)1 << 22;

// the warm-up rule of the header comment; 0 with the error set when the filter is unusable
static int lfilter_warm(const char *fn, const double *coef_host, int64_t *warm) {
    const double *a = coef_host + 6;
    for (int k = 0; k < 12; ++k)
        if (!isfinite(coef_host[k])) return fail("%s: non-finite coefficient", fn);
    if (a[0] != 1.0) return fail("%s: a[0] must be 1", fn);
    double rho = 0.0;
    if (!pole_radius(a, &rho)) return fail("%s: the poles of a[] could not be found", fn);
    if (!(rho < 1.0)) return fail("%s: unstable filter (pole radius %.9g)", fn, rho);
    int64_t w = FF_SB;
    if (rho > 0.0) {
        const double steps = ceil(-53.0 * M_LN2 / log(rho));
        if (steps > (double)LF_WARM_MAX)
            return fail("%s: pole radius %.9g needs a warm-up of %.0f samples (limit %lld)", fn, rho, steps, (long long)LF_WARM_MAX);
        w = ceil_div((int64_t)steps < 1 ? 1 : (int64_t)steps, FF_SB) * FF_SB;
    }
    *warm = w;
    return 0;
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_lfilter_order5_warmup(const double *coef_host, int64_t *warm) {
    if (!coef_host || !warm) return fail("rvc_lfilter_order5_warmup: null pointer");
    return lfilter_warm("rvc_lfilter_order5_warmup", coef_host, warm);
}

extern "C" int rvc_lfilter_order5_f64(const double *x_dev, int64_t n, const double *coef_host, double *y_dev, void *stream) {
    if (!x_dev || !coef_host || !y_dev) return fail("rvc_lfilter_order5_f64: null pointer");
    if (n < 0) return fail("rvc_lfilter_order5_f64: n = %lld is negative", (long long)n);
    if (x_dev == y_dev) return fail("rvc_lfilter_order5_f64: x_dev and y_dev must not alias");
    int64_t warm = 0;
    if (lfilter_warm("rvc_lfilter_order5_f64", coef_host, &warm)) return 1;
    if (n == 0) return 0;
    FiltCoef c;
    memcpy(c.b, coef_host, sizeof(c.b));
    memcpy(c.a, coef_host + 6, sizeof(c.a));
    memset(c.zi, 0, sizeof(c.zi));
    const int64_t n_chunks = ceil_div(n, LF_CHUNK), blocks = ceil_div(n_chunks, 64);
    if (blocks > 0x7fffffff) return fail("rvc_lfilter_order5_f64: n = %lld is too long for one launch", (long long)n);
    hipLaunchKernelGGL(lf_chunk_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, x_dev, n, c, (int)warm, n_chunks,
                       y_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

// frames and hop-long pieces of get_rms at this shape; non-zero (error set) on a bad shape
static int rms_shape(const char *fn, int64_t n, int64_t frame_length, int64_t hop, int64_t *n_frames, int64_t *n_part) {
    if (n < 0) return fail("%s: n = %lld is negative", fn, (long long)n);
    if (frame_length < 1) return fail("%s: frame_length = %lld must be at least 1", fn, (long long)frame_length);
    if (hop < 1) return fail("%s: hop = %lld must be at least 1", fn, (long long)hop);
    if (n > ((int64_t)1 << 40) || frame_length > ((int64_t)1 << 40) || hop > ((int64_t)1 << 40))
        return fail("%s: a size above 2^40", fn);
    const int64_t span = n + 2 * (frame_length / 2) - frame_length;          // Python's floor division: -1 // hop = -1
    *n_frames = span < 0 ? 0 : span / hop + 1;
    const int64_t m = frame_length / hop;
    *n_part = (*n_frames > 0 && m > 0) ? *n_frames - 1 + m : 0;
    return 0;
}

extern "C" int rvc_frame_rms_frames(int64_t n, int64_t frame_length, int64_t hop, int64_t *n_frames, size_t *workspace_bytes) {
    if (!n_frames || !workspace_bytes) return fail("rvc_frame_rms_frames: null pointer");
    int64_t n_part = 0;
    if (rms_shape("rvc_frame_rms_frames", n, frame_length, hop, n_frames, &n_part)) return 1;
    *workspace_bytes = align_up((size_t)n_part * 8, 256) + 256;
    return 0;
}

extern "C" int rvc_frame_rms_f64(const double *x_dev, int64_t n, int64_t frame_length, int64_t hop, double *out_dev,
                                 int64_t n_frames, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!x_dev || !out_dev || !workspace_dev) return fail("rvc_frame_rms_f64: null pointer");
    int64_t want_frames = 0, n_part = 0;
    if (rms_shape("rvc_frame_rms_f64", n, frame_length, hop, &want_frames, &n_part)) return 1;
    if (n_frames != want_frames)
        return fail("rvc_frame_rms_f64: n_frames = %lld, this shape has %lld", (long long)n_frames, (long long)want_frames);
    const size_t need = align_up((size_t)n_part * 8, 256) + 256;
    if (workspace_bytes < need) return fail("rvc_frame_rms_f64: workspace too small (%zu < %zu)", workspace_bytes, need);
    if (n_frames == 0) return 0;
    if (ceil_div(n_part, 4) > 0x7fffffff || ceil_div(n_frames, 256) > 0x7fffffff)
        return fail("rvc_frame_rms_f64: too many frames for one launch");
    const int64_t pad = frame_length / 2;
    double *part = (double *)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    if (n_part > 0) {
        hipLaunchKernelGGL(rms_partial_kernel, dim3((unsigned)ceil_div(n_part, 4)), dim3(256), 0, s, x_dev, n, pad, hop, n_part, part);
        RVC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rms_combine_kernel, dim3((unsigned)ceil_div(n_frames, 256)), dim3(256), 0, s, x_dev, n, pad, hop, frame_length,
                       part, out_dev, n_frames);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_slice_export_f32(const double *x_dev, int64_t n, const int64_t *bounds_host, const int64_t *seg_dev,
                                    const int64_t *off_full_dev, const int64_t *off_lo_dev, int64_t n_seg, int up, int down,
                                    const double *h_dev, int64_t n_taps, float *full_dev, int64_t n_full, float *lo_dev,
                                    int64_t n_lo, void *stream) {
    if (!x_dev || !bounds_host || !seg_dev || !off_full_dev || !off_lo_dev || !h_dev || !full_dev || !lo_dev)
        return fail("rvc_slice_export_f32: null pointer");
    if (n < 0) return fail("rvc_slice_export_f32: n = %lld is negative", (long long)n);
    if (n_seg < 0 || n_seg > ((int64_t)1 << 31)) return fail("rvc_slice_export_f32: n_seg = %lld out of range", (long long)n_seg);
    if (up < 1 || down < 1) return fail("rvc_slice_export_f32: up = %d, down = %d must be at least 1", up, down);
    if (n_taps < 1 || n_taps % 2 == 0) return fail("rvc_slice_export_f32: n_taps = %lld must be odd", (long long)n_taps);
    if (n > ((int64_t)1 << 40)) return fail("rvc_slice_export_f32: n above 2^40");
    int64_t sum_full = 0, sum_lo = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        const int64_t a = bounds_host[2 * s], b = bounds_host[2 * s + 1];
        if (a < 0 || b < 0) return fail("rvc_slice_export_f32: segment %lld = [%lld, %lld) is negative", (long long)s, (long long)a, (long long)b);
        if (b < a) return fail("rvc_slice_export_f32: segment %lld = [%lld, %lld) is reversed", (long long)s, (long long)a, (long long)b);
        if (b > n) return fail("rvc_slice_export_f32: segment %lld = [%lld, %lld) ends past n = %lld", (long long)s, (long long)a, (long long)b, (long long)n);
        sum_full += b - a;
        sum_lo += ceil_div((b - a) * up, down);
    }
    if (n_full != sum_full || n_lo != sum_lo)
        return fail("rvc_slice_export_f32: the packed outputs hold %lld and %lld samples, the segments need %lld and %lld",
                    (long long)n_full, (long long)n_lo, (long long)sum_full, (long long)sum_lo);
    if (n_full == 0) return 0;
    const int64_t nb_full = ceil_div(n_full, 256), nb_lo = ceil_div(n_lo, 256);
    if (nb_full + nb_lo > 0x7fffffff) return fail("rvc_slice_export_f32: too many samples for one launch");
    hipLaunchKernelGGL(slice_export_kernel, dim3((unsigned)(nb_full + nb_lo)), dim3(256), 0, (hipStream_t)stream, x_dev, n, seg_dev,
                       off_full_dev, off_lo_dev, n_seg, up, down, h_dev, n_taps, full_dev, n_full, lo_dev, n_lo, nb_full);
    RVC_LAUNCH_CHECK();
    return 0;
}
