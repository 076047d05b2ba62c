// K15: the memory-bound kernels of the FCPE pitch estimator (rvc/lib/predictors/torchfcpe, conv-only conformer).
//
// The dense layers of the network run on K11 (gemmbf.hip); what is left between them is here, fp32 in and fp32 out:
//   (a) rvc_glu_dwconv_silu_f32   nn.GLU(dim=1) -> DepthWiseConv1d(k = 31, same padding) -> nn.SiLU of ConformerConvModule
//                                 (model_conformer_naive.py:144-151), on time-major rows
//   (b) rvc_layernorm_rows_f32    nn.LayerNorm over the feature axis (model_conformer_naive.py:142, models.py:83)
//   (c) rvc_groupnorm_lrelu_f32   nn.GroupNorm(4, hidden) -> nn.LeakyReLU() of input_stack (models.py:66-71), channel-major
//   (d) rvc_fcpe_decode_f32       sigmoid + latent2cents_local_decoder + cent_to_f0 + the uv mask (models.py:120, 149-176, 246-251,
//                                 models_infer.py:204-207)
// Statistics ((b), (c)) and the nine-term weighted mean of (d) are float64: these kernels move a few bytes per flop, the fp64
// vector rate is not what bounds them, and a centred float64 deviation costs no accuracy where the data ride on a large offset.
#include "common.h"

namespace rvc {

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// ---- (a) GLU -> depthwise FIR -> SiLU ------------------------------------------------------------------------------------------------
// A workgroup owns GLU_TILE time rows x 64 channels.  Lane layout: 16 lanes x float4 along the channels (one 256-byte row of the
// LDS image, all 64 banks), 16 row groups.  Pass 1 evaluates u = value * sigmoid(gate) ONCE per element into LDS for the tile and
// its K - 1 halo rows (zero outside [0, n_rows)); pass 2 runs the FIR out of LDS with the K x 4 taps of the thread's channels in
// registers: each thread walks the GLU_ROWS + K - 1 input rows of its GLU_ROWS consecutive outputs once, one ds_read_b128 per row,
// tap index ascending per output (the order of the defining sum).  The 16-lane service groups of ds_read_b128 mix two row groups,
// whose rows are a whole number of 256-byte bank rows apart: the 16 slots stay distinct, the image needs no padding.
// Halo: (K - 1) / GLU_TILE extra reads, 23 % at K = 31 (an estimate from the tile shape, not a measurement).
constexpr int GLU_TILE = 128, GLU_ROWS = 8, GLU_SLAB = 64;

template <int K>
__global__ void __launch_bounds__(256)
glu_dwconv_silu_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ y,
                       int64_t n_rows, int C) {
    extern __shared__ __attribute__((aligned(16))) float u_lds[];   // [GLU_TILE + K - 1][64]
    const int tid = threadIdx.x, cq = tid & 15, rg = tid >> 4;
    const int c0 = blockIdx.x * GLU_SLAB + 4 * cq;
    const int64_t t0 = (int64_t)blockIdx.y * GLU_TILE;
    for (int r = rg; r < GLU_TILE + K - 1; r += 16) {
        const int64_t t = t0 - K / 2 + r;
        f32x4 u = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < n_rows) {
            const float *row = x + t * 2 * C + c0;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(row);
            const f32x4 g = *reinterpret_cast<const f32x4 *>(row + C);
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = v[e] * sigmoidf(g[e]);
        }
        *reinterpret_cast<f32x4 *>(u_lds + r * GLU_SLAB + 4 * cq) = u;
    }
    float taps[4][K];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < K; ++j) taps[e][j] = w[(int64_t)(c0 + e) * K + j];
    const f32x4 b = *reinterpret_cast<const f32x4 *>(bias + c0);
    f32x4 acc[GLU_ROWS];
#pragma unroll
    for (int o = 0; o < GLU_ROWS; ++o) acc[o] = b;
    __syncthreads();
    const float *base = u_lds + rg * GLU_ROWS * GLU_SLAB + 4 * cq;
#pragma unroll
    for (int i = 0; i < GLU_ROWS + K - 1; ++i) {
        const f32x4 u = *reinterpret_cast<const f32x4 *>(base + i * GLU_SLAB);
#pragma unroll
        for (int o = 0; o < GLU_ROWS; ++o) {
            if (i - o >= 0 && i - o < K) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[o][e] = fmaf(taps[e][i - o], u[e], acc[o][e]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < GLU_ROWS; ++o) {
        const int64_t t = t0 + rg * GLU_ROWS + o;
        if (t < n_rows) {
            f32x4 v = acc[o];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] * sigmoidf(v[e]);
            *reinterpret_cast<f32x4 *>(y + t * C + c0) = v;
        }
    }
}

template <int K>
static int launch_glu(const float *x, const float *w, const float *bias, float *y, int64_t n_rows, int C, hipStream_t stream) {
    const dim3 grid((unsigned)(C / GLU_SLAB), (unsigned)ceil_div(n_rows, GLU_TILE));
    const size_t lds = (size_t)(GLU_TILE + K - 1) * GLU_SLAB * sizeof(float);
    hipLaunchKernelGGL(glu_dwconv_silu_kernel<K>, grid, dim3(256), lds, stream, x, w, bias, y, n_rows, C);
    RVC_LAUNCH_CHECK();
    return 0;
}

// ---- (b) LayerNorm over rows --------------------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup; a lane holds F / 64 <= 16 elements (lane-strided: every load instruction of the wave
// is one contiguous 256-byte piece).  Two passes over the registers: the mean first (float64 sum), then the centred squares.
__global__ void __launch_bounds__(256)
layernorm_rows_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ y,
                      int64_t n_rows, int F, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int per = F >> 6;
    const float *xr = x + row * F;
    float v[16];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        v[i] = i < per ? xr[i * 64 + lane] : 0.f;
        s += (double)v[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const double mean = s / (double)F;
    float d[16];
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        d[i] = i < per ? (float)((double)v[i] - mean) : 0.f;
        q += (double)d[i] * (double)d[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float rstd = (float)(1.0 / sqrt(q / (double)F + (double)eps));
    float *yr = y + row * F;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < per) yr[i * 64 + lane] = d[i] * rstd * gamma[i * 64 + lane] + beta[i * 64 + lane];
}

// ---- (c) GroupNorm + LeakyReLU, channel-major -------------------------------------------------------------------------------------
// A group is one contiguous run of (C / groups) x L floats.  Kernel 1: a workgroup takes GN_CHUNK elements of one group, sums them
// (float64), then re-reads them (L2-hot) for the sum of squares centred on ITS OWN mean, and writes (count, mean, M2) as three
// doubles.  Kernel 2: every workgroup merges the partials of its channel's group in float64 (Chan's pairwise update, the same for
// every thread), then normalises one stretch of one channel row.  No fp32 running sum spans more than one thread's share of a chunk.
constexpr int GN_CHUNK = 16384;

__device__ __forceinline__ double block_sum_256(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256)
groupnorm_partial_kernel(const float *__restrict__ x, double *__restrict__ part, int64_t group_elems, int n_chunks) {
    __shared__ double red[4];
    const int g = blockIdx.y, p = blockIdx.x;
    const int64_t lo = (int64_t)p * GN_CHUNK;
    const int64_t n = group_elems - lo < GN_CHUNK ? group_elems - lo : GN_CHUNK;
    const float *xg = x + (int64_t)g * group_elems + lo;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)xg[i];
    const double mean = block_sum_256(s, red) / (double)n;
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double d = (double)xg[i] - mean;
        q += d * d;
    }
    q = block_sum_256(q, red);
    if (threadIdx.x == 0) {
        double *o = part + ((int64_t)g * n_chunks + p) * 3;
        o[0] = (double)n;
        o[1] = mean;
        o[2] = q;
    }
}

__global__ void __launch_bounds__(256)
groupnorm_apply_kernel(const float *__restrict__ x, const double *__restrict__ part, const float *__restrict__ gamma,
                       const float *__restrict__ beta, float *__restrict__ y, int cpg, int64_t L, int n_chunks, float eps, float slope) {
    const int c = blockIdx.y;
    const double *pg = part + (int64_t)(c / cpg) * n_chunks * 3;
    double n = pg[0], mean = pg[1], m2 = pg[2];
    for (int p = 1; p < n_chunks; ++p) {
        const double nb = pg[3 * p], delta = pg[3 * p + 1] - mean, tot = n + nb;
        mean += delta * (nb / tot);
        m2 += pg[3 * p + 2] + delta * delta * (n * nb / tot);
        n = tot;
    }
    const float rstd = (float)(1.0 / sqrt(m2 / n + (double)eps));
    const float ga = gamma[c], be = beta[c];
    const float *xr = x + (int64_t)c * L;
    float *yr = y + (int64_t)c * L;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < L; t += (int64_t)gridDim.x * 256)
        yr[t] = lrelu((float)((double)xr[t] - mean) * rstd * ga + be, slope);
}

static int groupnorm_chunks(int C, int64_t L, int groups) { return (int)ceil_div((int64_t)(C / groups) * L, GN_CHUNK); }

// ---- (d) decode ------------------------------------------------------------------------------------------------------------------------
// One wave per frame.  Every lane walks the row with stride 64: latent = sigmoid(logit), running maximum and the LOWEST index that
// attains it, then a butterfly over (max, index).  Lanes 0..8 re-evaluate the nine clamped neighbours (the same expression on the
// same logit: the same bits as the latent) and the weighted mean of their cents is taken in float64.
__global__ void __launch_bounds__(256)
fcpe_decode_kernel(const float *__restrict__ logits, const float *__restrict__ cent_table, int out_dims, int ld, float threshold,
                   float f0_min, float *__restrict__ f0, float *__restrict__ latent, int64_t n_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float *lr = logits + row * ld;
    float best = -1.f;   // a sigmoid is >= 0
    int arg = 0x7fffffff;
    for (int i = lane; i < out_dims; i += 64) {
        const float v = sigmoidf(lr[i]);
        if (latent) latent[row * out_dims + i] = v;
        if (v > best) { best = v; arg = i; }   // ascending i per lane: the first of equals stays
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    double num = 0.0, den = 0.0;
    if (lane < 9) {
        int i = arg - 4 + lane;
        i = i < 0 ? 0 : (i > out_dims - 1 ? out_dims - 1 : i);
        const double v = (double)sigmoidf(lr[i]);
        num = (double)cent_table[i] * v;
        den = v;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) { num += __shfl_xor(num, off); den += __shfl_xor(den, off); }
    if (lane == 0) {
        float r = 0.f;
        if (best > threshold) {
            r = (float)(10.0 * exp2(num / den / 1200.0));
            if (r < f0_min) r = 0.f;
        }
        f0[row] = r;
    }
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_glu_dwconv_silu_f32(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t n_rows,
                                       int C, int K, void *stream) {
    if (!x_dev || !w_dev || !bias_dev || !y_dev) return fail("rvc_glu_dwconv_silu_f32: null pointer");
    if (n_rows < 1) return fail("rvc_glu_dwconv_silu_f32: n_rows (%lld) must be >= 1", (long long)n_rows);
    if (C < 64 || C % 64) return fail("rvc_glu_dwconv_silu_f32: C (%d) must be a positive multiple of 64", C);
    if (K < 1 || K > 31 || K % 2 == 0) return fail("rvc_glu_dwconv_silu_f32: K (%d) must be odd and within 1..31", K);
    if ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(bias_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15)
        return fail("rvc_glu_dwconv_silu_f32: x_dev, bias_dev and y_dev must be 16-byte aligned");
    if (ceil_div(n_rows, GLU_TILE) > 65535) return fail("rvc_glu_dwconv_silu_f32: n_rows (%lld) exceeds the grid", (long long)n_rows);
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
#define RVC_GLU_CASE(k) case k: return launch_glu<k>(x_dev, w_dev, bias_dev, y_dev, n_rows, C, s);
        RVC_GLU_CASE(1) RVC_GLU_CASE(3) RVC_GLU_CASE(5) RVC_GLU_CASE(7) RVC_GLU_CASE(9) RVC_GLU_CASE(11) RVC_GLU_CASE(13) RVC_GLU_CASE(15)
        RVC_GLU_CASE(17) RVC_GLU_CASE(19) RVC_GLU_CASE(21) RVC_GLU_CASE(23) RVC_GLU_CASE(25) RVC_GLU_CASE(27) RVC_GLU_CASE(29) RVC_GLU_CASE(31)
#undef RVC_GLU_CASE
    }
    return fail("rvc_glu_dwconv_silu_f32: K (%d) not instantiated", K);
}

extern "C" int rvc_layernorm_rows_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, float eps, float *y_dev,
                                      int64_t n_rows, int F, void *stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev) return fail("rvc_layernorm_rows_f32: null pointer");
    if (n_rows < 1) return fail("rvc_layernorm_rows_f32: n_rows (%lld) must be >= 1", (long long)n_rows);
    if (F < 64 || F > 1024 || F % 64) return fail("rvc_layernorm_rows_f32: F (%d) must be a multiple of 64 within 64..1024", F);
    if (!(eps >= 0.f)) return fail("rvc_layernorm_rows_f32: eps must be >= 0");
    if (ceil_div(n_rows, 4) > 0x7fffffff) return fail("rvc_layernorm_rows_f32: n_rows (%lld) exceeds the grid", (long long)n_rows);
    hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, x_dev, gamma_dev,
                       beta_dev, y_dev, n_rows, F, eps);
    RVC_LAUNCH_CHECK();
    return 0;
}

static int groupnorm_shape_ok(const char *fn, int C, int64_t L, int groups) {
    if (C < 1 || L < 1 || groups < 1) return fail("%s: bad shape (C %d, L %lld, groups %d)", fn, C, (long long)L, groups);
    if (C % groups) return fail("%s: groups (%d) must divide C (%d)", fn, groups, C);
    if (C > 65535 || groups > 65535) return fail("%s: C (%d) exceeds the grid", fn, C);
    if (ceil_div((int64_t)(C / groups) * L, GN_CHUNK) > 0x7fffffff) return fail("%s: a group of %d x %lld elements exceeds the grid", fn, C / groups, (long long)L);
    return 0;
}

extern "C" int rvc_groupnorm_workspace_bytes(int C, int64_t L, int groups, size_t *bytes) {
    if (!bytes) return fail("rvc_groupnorm_workspace_bytes: null pointer");
    if (groupnorm_shape_ok("rvc_groupnorm_workspace_bytes", C, L, groups)) return 1;
    *bytes = (size_t)groups * groupnorm_chunks(C, L, groups) * 3 * sizeof(double);
    return 0;
}

extern "C" int rvc_groupnorm_lrelu_f32(const float *x_dev, const float *gamma_dev, const float *beta_dev, int groups, float eps,
                                       float slope, float *y_dev, int C, int64_t L, void *workspace_dev, size_t workspace_bytes,
                                       void *stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev || !workspace_dev) return fail("rvc_groupnorm_lrelu_f32: null pointer");
    if (groupnorm_shape_ok("rvc_groupnorm_lrelu_f32", C, L, groups)) return 1;
    if (!(eps >= 0.f)) return fail("rvc_groupnorm_lrelu_f32: eps must be >= 0");
    const int n_chunks = groupnorm_chunks(C, L, groups);
    const size_t need = (size_t)groups * n_chunks * 3 * sizeof(double);
    if (workspace_bytes < need) return fail("rvc_groupnorm_lrelu_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 7) return fail("rvc_groupnorm_lrelu_f32: the workspace must be 8-byte aligned");
    const int cpg = C / groups;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(groupnorm_partial_kernel, dim3((unsigned)n_chunks, (unsigned)groups), dim3(256), 0, s, x_dev,
                       (double *)workspace_dev, (int64_t)cpg * L, n_chunks);
    RVC_LAUNCH_CHECK();
    int64_t bx = ceil_div(L, 1024);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(groupnorm_apply_kernel, dim3((unsigned)bx, (unsigned)C), dim3(256), 0, s, x_dev, (const double *)workspace_dev,
                       gamma_dev, beta_dev, y_dev, cpg, L, n_chunks, eps, slope);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_fcpe_decode_f32(const float *logits_dev, const float *cent_table_dev, int out_dims, int ld, float threshold,
                                   float f0_min, float *f0_dev, float *latent_dev, int64_t n_rows, void *stream) {
    if (!logits_dev || !cent_table_dev || !f0_dev) return fail("rvc_fcpe_decode_f32: null pointer");
    if (n_rows < 1) return fail("rvc_fcpe_decode_f32: n_rows (%lld) must be >= 1", (long long)n_rows);
    if (out_dims < 1) return fail("rvc_fcpe_decode_f32: out_dims (%d) must be >= 1", out_dims);
    if (ld < out_dims) return fail("rvc_fcpe_decode_f32: the row stride ld (%d) must be >= out_dims (%d)", ld, out_dims);
    if (ceil_div(n_rows, 4) > 0x7fffffff) return fail("rvc_fcpe_decode_f32: n_rows (%lld) exceeds the grid", (long long)n_rows);
    hipLaunchKernelGGL(fcpe_decode_kernel, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, (hipStream_t)stream, logits_dev,
                       cent_table_dev, out_dims, ld, threshold, f0_min, f0_dev, latent_dev, n_rows);
    RVC_LAUNCH_CHECK();
    return 0;
}
