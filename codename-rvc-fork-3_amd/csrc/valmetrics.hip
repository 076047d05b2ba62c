// K20 -- the validation losses of include/rvc_amd.h: the sums behind a multi-resolution STFT loss, SI-SDR and a mean absolute
// difference (the mel L1), each as float64 partial sums per workgroup that a second kernel merges in a fixed order.  No atomics
// anywhere: two calls give identical bits (K16's contract).
//
// mrstft_kernel is the hot one.  One launch covers every resolution; a workgroup (4 waves) owns 32 frames x 256 bins of one
// resolution.  It stages the samples its 32 frames cover (reflect padding resolved while staging) for BOTH signals in LDS, next to
// the resolution's window and one period of cos(2 pi j / n_fft), and runs the DFT as a GEMM on the exact-fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: A = windowed frames, B = cos | -sin looked up at (k * bin) mod n_fft, exact argument reduction).  The
// window is zero outside its `win` samples, so K is win, not n_fft.  A wave holds two 32 x 32 bin tiles: re and im of x and y,
// 8 accumulators of 16 registers, and as many again for the running chain: a dot product is summed as fmaf chains of 64 samples
// whose sums are added in order (stft1024.h: why a long chain is split).  The Nyquist bin rides in the imaginary slot of bin 0
// (whose own imaginary part is identically zero: its "-sin" column is (-1)^k), so the bins of a transform are n_fft / 2: whole
// tiles.  Magnitudes, differences and logarithms are formed from the accumulators in float64 registers; nothing but 3 doubles
// per workgroup goes to HBM.
#include <math.h>

#include "common.h"

namespace rvc {

constexpr int VM_MAX_RES = 4;
constexpr int VM_TILE_FRAMES = 32;
constexpr int VM_GROUP_BINS = 256;          // 4 waves x 2 tiles x 32 bins
constexpr int VM_CHAIN = 64;                // samples per fmaf chain
constexpr int VM_MAX_HOP = 512;             // 31 * 512 + 2048 samples of two signals, the table and the window: 156 KiB of LDS
constexpr int64_t VM_MAX_N = (int64_t)1 << 27;
constexpr int VM_SUM_BLOCKS = 1024;         // most workgroups of an elementwise sum

struct MrRes {
    int n_fft, hop, win;
    int woff;       // (n_fft - win) / 2: where the window starts inside the n_fft frame
    int kp;         // win rounded up to even: the GEMM's K
    int frames;     // 1 + n / hop
    int groups;     // n_fft / 2 / 256 bin groups
    int blocks;     // ceil(frames / 32) * groups
    int block0;     // first workgroup of this resolution
};
struct MrPlan {
    MrRes r[VM_MAX_RES];
    int n_res;
    int total_blocks;
    int lds_bytes;
};

static inline int mr_lds_bytes(const MrRes &r) { return (r.n_fft + r.kp + 2 * ((VM_TILE_FRAMES - 1) * r.hop + r.kp)) * 4; }

// thread c < ncomp adds red[c][0 .. 255] in index order
__device__ __forceinline__ void block_sums(double *red, const double *v, int ncomp, double *dst) {
    const int t = threadIdx.x;
    for (int c = 0; c < ncomp; ++c) red[c * 256 + t] = v[c];
    __syncthreads();
    if (t < ncomp) {
        double acc = 0.0;
        for (int i = 0; i < 256; ++i) acc += red[t * 256 + i];
        dst[t] = acc;
    }
    __syncthreads();
}

// out[c] = sum over part[b][c], b < nblk: thread t adds b = t, t + 256, ... in order, then block_sums
__device__ __forceinline__ void merge_partials(double *red, const double *part, int nblk, int ncomp, double *out) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblk; b += 256)
        for (int c = 0; c < ncomp; ++c) v[c] += part[(size_t)b * ncomp + c];
    block_sums(red, v, ncomp, out);
}

// One power pair's three terms, out of line: the epilogue calls it 48 times with register operands.
struct MrTerms { double d2, y2, la; };
__device__ __noinline__ MrTerms mr_terms(double px, double py, double eps) {
    px = px > eps ? px : eps;
    py = py > eps ? py : eps;
    const double d = sqrt(py) - sqrt(px);
    return {d * d, py, 0.5 * fabs(log(px) - log(py))};
}

// The terms of one 32 x 32 tile (re / im of x and of y) that lie in frames below `frames`, added to v in register order.  has_dc:
// this lane's column is bin 0, whose real part is the DC bin and whose imaginary slot carries the Nyquist bin.
__device__ __forceinline__ void mr_tile_terms(const f32x16 &xr, const f32x16 &xi, const f32x16 &yr, const f32x16 &yi, bool has_dc,
                                              int64_t t0, int lane, int frames, double eps, double *v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const bool live = t0 + mfma32_row(r, lane) < frames;
        const double a = (double)xr[r], b = (double)xi[r], c = (double)yr[r], d = (double)yi[r];
        if (live) {
            const MrTerms m = has_dc ? mr_terms(a * a, c * c, eps) : mr_terms(a * a + b * b, c * c + d * d, eps);
            v[0] += m.d2; v[1] += m.y2; v[2] += m.la;
        }
        if (live && has_dc) {
            const MrTerms m = mr_terms(b * b, d * d, eps);
            v[0] += m.d2; v[1] += m.y2; v[2] += m.la;
        }
    }
}

__global__ void __launch_bounds__(256)
mrstft_kernel(const float *__restrict__ x, const float *__restrict__ y, int64_t n, const MrPlan plan, double eps, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int ri = 0;
    while (ri + 1 < plan.n_res && (int)blockIdx.x >= plan.r[ri + 1].block0) ++ri;
    const MrRes R = plan.r[ri];
    const int local = (int)blockIdx.x - R.block0;
    const int tile = local / R.groups, grp = local - tile * R.groups;
    const int N = R.n_fft, H = R.hop, mask = N - 1;
    const int span = (VM_TILE_FRAMES - 1) * H + R.kp;
    float *tab = lds;                 // [N]   cos(2 pi j / N)
    float *w = tab + N;               // [kp]  periodic hann(win), 0 at kp - 1 when win is odd
    float *sx = w + R.kp;             // [span]
    float *sy = sx + span;            // [span]
    const int t = threadIdx.x;
    for (int j = t; j < N; j += 256) tab[j] = (float)cospi(2.0 * (double)j / (double)N);
    for (int j = t; j < R.kp; j += 256) w[j] = j < R.win ? (float)(0.5 - 0.5 * cospi(2.0 * (double)j / (double)R.win)) : 0.f;
    const int64_t t0 = (int64_t)tile * VM_TILE_FRAMES;
    const int64_t s_base = t0 * H - N / 2 + R.woff;
    for (int j = t; j < span; j += 256) {
        int64_t s = s_base + j;
        if (s < 0) s = -s;                       // reflect: n > N / 2, so one fold lands inside
        if (s > n - 1) s = 2 * (n - 1) - s;
        if (s < 0) s = 0;                        // only frames past the last one reach here; they are masked below
        if (s > n - 1) s = n - 1;
        sx[j] = x[s];
        sy[j] = y[s];
    }
    __syncthreads();

    const int lane = t & 63, wave = t >> 6;
    const int fi = lane & 31, kk = lane >> 5;
    int bin[2];
    bin[0] = grp * VM_GROUP_BINS + wave * 64 + fi;
    bin[1] = bin[0] + 32;
    f32x16 acc[8], run[8];     // [2 u + 0/1] of x: re, im; [4 + 2 u + 0/1] of y
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    const float *fx = sx + fi * H, *fy = sy + fi * H;
    for (int k0 = 0; k0 < R.kp; k0 += VM_CHAIN) {
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) run[a][r] = 0.f;
        const int k1 = k0 + VM_CHAIN < R.kp ? k0 + VM_CHAIN : R.kp;
        for (int k = k0; k < k1; k += 2) {
            const int ka = k + kk;
            const float wv = w[ka];
            const float ax = fx[ka] * wv, ay = fy[ka] * wv;
            const int kabs = ka + R.woff;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = (kabs * bin[u]) & mask;
                const float c = tab[idx];
                float s = tab[(idx + N / 4) & mask];           // cos(a + pi / 2) = -sin a
                if (bin[u] == 0) s = (kabs & 1) ? -1.f : 1.f;  // the Nyquist bin in bin 0's imaginary slot
                run[2 * u] = mfma32(ax, c, run[2 * u]);
                run[2 * u + 1] = mfma32(ax, s, run[2 * u + 1]);
                run[4 + 2 * u] = mfma32(ay, c, run[4 + 2 * u]);
                run[4 + 2 * u + 1] = mfma32(ay, s, run[4 + 2 * u + 1]);
            }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) acc[a] += run[a];
    }

    // Static register indices throughout: the accumulators must not be addressed by a loop variable that survives unrolling.
    double v[3] = {0.0, 0.0, 0.0};   // sum (ymag - xmag)^2, sum ymag^2, sum |log xmag - log ymag|
    mr_tile_terms(acc[0], acc[1], acc[4], acc[5], bin[0] == 0, t0, lane, R.frames, eps, v);   // only tile 0 can hold bin 0
    mr_tile_terms(acc[2], acc[3], acc[6], acc[7], false, t0, lane, R.frames, eps, v);
    __syncthreads();                         // the table and the samples are dead: the head of LDS carries the reduction
    block_sums((double *)lds, v, 3, part + (size_t)blockIdx.x * 3);
}

// block r: out[4 r + 0 .. 2] = the resolution's sums, out[4 r + 3] = frames * (n_fft / 2 + 1)
__global__ void __launch_bounds__(256) mrstft_merge_kernel(const double *__restrict__ part, const MrPlan plan, double *__restrict__ out) {
    __shared__ double red[3 * 256];
    const MrRes R = plan.r[blockIdx.x];
    merge_partials(red, part + (size_t)R.block0 * 3, R.blocks, 3, out + 4 * blockIdx.x);
    if (threadIdx.x == 0) out[4 * blockIdx.x + 3] = (double)R.frames * (double)(R.n_fft / 2 + 1);
}

// MODE 0: sum p, sum t.  MODE 1: with mp = mean[0] / n, mt = mean[1] / n: sum (p - mp)(t - mt), sum (t - mt)^2, sum (p - mp)^2.
// MODE 2: sum |a[r][c] - b[r][c]| over r < rows, c < cols (n = rows * cols), rows strided.
template <int MODE>
__global__ void __launch_bounds__(256)
pair_sums_kernel(const float *__restrict__ a, int64_t a_stride, const float *__restrict__ b, int64_t b_stride, int64_t n, int64_t cols,
                 const double *__restrict__ mean, double *__restrict__ part) {
    __shared__ double red[3 * 256];
    constexpr int NC = MODE == 0 ? 2 : MODE == 1 ? 3 : 1;
    double v[3] = {0.0, 0.0, 0.0};
    double ma = 0.0, mb = 0.0;
    if (MODE == 1) { ma = mean[0] / (double)n; mb = mean[1] / (double)n; }
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        if (MODE == 2) {
            const int64_t r = i / cols, c = i - r * cols;
            v[0] += fabs((double)a[r * a_stride + c] - (double)b[r * b_stride + c]);
        } else {
            const double p = (double)a[i] - ma, q = (double)b[i] - mb;
            if (MODE == 0) { v[0] += p; v[1] += q; }
            else { v[0] += p * q; v[1] += q * q; v[2] += p * p; }
        }
    }
    block_sums(red, v, NC, part + (size_t)blockIdx.x * NC);
}

__global__ void __launch_bounds__(256) sums_merge_kernel(const double *__restrict__ part, int nblk, int ncomp, double *__restrict__ out) {
    __shared__ double red[3 * 256];
    merge_partials(red, part, nblk, ncomp, out);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int mr_plan(const char *fn, int64_t n, const int *n_fft, const int *hop, const int *win, int n_res, MrPlan *pl) {
    if (!n_fft || !hop || !win) return fail("%s: null pointer", fn);
    if (n_res < 1 || n_res > VM_MAX_RES) return fail("%s: n_res %d must be in [1, %d]", fn, n_res, VM_MAX_RES);
    if (n > VM_MAX_N) return fail("%s: n = %lld exceeds %lld samples", fn, (long long)n, (long long)VM_MAX_N);
    int64_t total = 0;
    pl->n_res = n_res;
    pl->lds_bytes = 0;
    for (int i = 0; i < n_res; ++i) {
        MrRes &r = pl->r[i];
        r.n_fft = n_fft[i]; r.hop = hop[i]; r.win = win[i];
        if (r.n_fft != 512 && r.n_fft != 1024 && r.n_fft != 2048)
            return fail("%s: n_fft %d is not built (512, 1024 and 2048 are)", fn, r.n_fft);
        if (r.win < 1 || r.win > r.n_fft) return fail("%s: win %d must be in [1, n_fft = %d]", fn, r.win, r.n_fft);
        if (r.hop < 1 || r.hop > VM_MAX_HOP) return fail("%s: hop %d must be in [1, %d]", fn, r.hop, VM_MAX_HOP);
        if (n <= r.n_fft / 2)
            return fail("%s: n = %lld must exceed n_fft / 2 = %d (the reflect padding is undefined)", fn, (long long)n, r.n_fft / 2);
        r.woff = (r.n_fft - r.win) / 2;
        r.kp = (r.win + 1) & ~1;
        r.frames = (int)(1 + n / r.hop);
        r.groups = r.n_fft / 2 / VM_GROUP_BINS;
        r.blocks = (int)ceil_div(r.frames, VM_TILE_FRAMES) * r.groups;
        r.block0 = (int)total;
        total += r.blocks;
        if (total > ((int64_t)1 << 30)) return fail("%s: n = %lld at hop %d needs too many workgroups", fn, (long long)n, r.hop);
        const int b = mr_lds_bytes(r);
        if (b > pl->lds_bytes) pl->lds_bytes = b;
    }
    if (pl->lds_bytes < 3 * 256 * 8) pl->lds_bytes = 3 * 256 * 8;   // the reduction reuses the head of LDS
    pl->total_blocks = (int)total;
    return 0;
}

static int sum_blocks(int64_t n) {
    const int64_t b = ceil_div(n, 256);
    return (int)(b < VM_SUM_BLOCKS ? b : VM_SUM_BLOCKS);
}

static bool misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_mrstft_sums_workspace_bytes(int64_t n, const int *n_fft, const int *hop, const int *win, int n_res, size_t *bytes) {
    if (!bytes) return fail("rvc_mrstft_sums_workspace_bytes: null pointer");
    MrPlan pl;
    if (mr_plan("rvc_mrstft_sums_workspace_bytes", n, n_fft, hop, win, n_res, &pl)) return 1;
    *bytes = (size_t)pl.total_blocks * 3 * sizeof(double);
    return 0;
}

extern "C" int rvc_mrstft_sums_f32(const float *x_dev, const float *y_dev, int64_t n, const int *n_fft, const int *hop, const int *win,
                                   int n_res, double eps, double *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_mrstft_sums_f32";
    if (!x_dev || !y_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (misaligned(x_dev, 4) || misaligned(y_dev, 4) || misaligned(out_dev, 8) || misaligned(workspace_dev, 8))
        return fail("%s: misaligned pointer (signals 4 bytes, out_dev and workspace_dev 8)", fn);
    MrPlan pl;
    if (mr_plan(fn, n, n_fft, hop, win, n_res, &pl)) return 1;
    if (!(eps > 0.0) || !isfinite(eps)) return fail("%s: eps %g must be positive and finite", fn, eps);
    const size_t need = (size_t)pl.total_blocks * 3 * sizeof(double);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    if (reserve_lds((const void *)mrstft_kernel, pl.lds_bytes, fn)) return 1;
    hipLaunchKernelGGL(mrstft_kernel, dim3((unsigned)pl.total_blocks), dim3(256), (size_t)pl.lds_bytes, stream, x_dev, y_dev, n, pl, eps,
                       (double *)workspace_dev);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(mrstft_merge_kernel, dim3((unsigned)pl.n_res), dim3(256), 0, stream, (const double *)workspace_dev, pl, out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_si_sdr_sums_workspace_bytes(int64_t n, size_t *bytes) {
    if (!bytes) return fail("rvc_si_sdr_sums_workspace_bytes: null pointer");
    if (n < 2) return fail("rvc_si_sdr_sums_workspace_bytes: n = %lld must be at least 2", (long long)n);
    *bytes = (size_t)sum_blocks(n) * 3 * sizeof(double);
    return 0;
}

extern "C" int rvc_si_sdr_sums_f32(const float *preds_dev, const float *target_dev, int64_t n, double *out_dev, void *workspace_dev,
                                   size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_si_sdr_sums_f32";
    if (!preds_dev || !target_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (misaligned(preds_dev, 4) || misaligned(target_dev, 4) || misaligned(out_dev, 8) || misaligned(workspace_dev, 8))
        return fail("%s: misaligned pointer (signals 4 bytes, out_dev and workspace_dev 8)", fn);
    if (n < 2) return fail("%s: n = %lld must be at least 2", fn, (long long)n);
    const int nb = sum_blocks(n);
    const size_t need = (size_t)nb * 3 * sizeof(double);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    double *part = (double *)workspace_dev;
    hipLaunchKernelGGL(pair_sums_kernel<0>, dim3(nb), dim3(256), 0, stream, preds_dev, (int64_t)0, target_dev, (int64_t)0, n, (int64_t)0,
                       (const double *)nullptr, part);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sums_merge_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, nb, 2, out_dev);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_sums_kernel<1>, dim3(nb), dim3(256), 0, stream, preds_dev, (int64_t)0, target_dev, (int64_t)0, n, (int64_t)0,
                       (const double *)out_dev, part);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sums_merge_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, nb, 3, out_dev + 2);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_mean_abs_diff_workspace_bytes(int64_t rows, int64_t min_t, size_t *bytes) {
    if (!bytes) return fail("rvc_mean_abs_diff_workspace_bytes: null pointer");
    if (rows < 1 || min_t < 1 || rows > VM_MAX_N || min_t > VM_MAX_N || rows * min_t > ((int64_t)1 << 40))
        return fail("rvc_mean_abs_diff_workspace_bytes: rows = %lld and min_t = %lld must be at least 1 and span at most 2^40 elements",
                    (long long)rows, (long long)min_t);
    *bytes = (size_t)sum_blocks(rows * min_t) * sizeof(double);
    return 0;
}

extern "C" int rvc_mean_abs_diff_f32(const float *a_dev, int64_t a_stride, const float *b_dev, int64_t b_stride, int64_t rows, int64_t min_t,
                                     double *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_mean_abs_diff_f32";
    if (!a_dev || !b_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (misaligned(a_dev, 4) || misaligned(b_dev, 4) || misaligned(out_dev, 8) || misaligned(workspace_dev, 8))
        return fail("%s: misaligned pointer (matrices 4 bytes, out_dev and workspace_dev 8)", fn);
    if (rows < 1 || min_t < 1 || rows > VM_MAX_N || min_t > VM_MAX_N || rows * min_t > ((int64_t)1 << 40))
        return fail("%s: rows = %lld and min_t = %lld must be at least 1 and span at most 2^40 elements", fn, (long long)rows, (long long)min_t);
    if (a_stride < min_t || b_stride < min_t)
        return fail("%s: row strides %lld and %lld must be at least min_t = %lld", fn, (long long)a_stride, (long long)b_stride, (long long)min_t);
    const int64_t n = rows * min_t;
    const int nb = sum_blocks(n);
    const size_t need = (size_t)nb * sizeof(double);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    double *part = (double *)workspace_dev;
    hipLaunchKernelGGL(pair_sums_kernel<2>, dim3(nb), dim3(256), 0, stream, a_dev, a_stride, b_dev, b_stride, n, min_t, (const double *)nullptr, part);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sums_merge_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, nb, 1, out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}
