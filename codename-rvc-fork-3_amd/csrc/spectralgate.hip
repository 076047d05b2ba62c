// K18 -- clean_audio: a non-stationary spectral gate (the default path of noisereduce 3.x's reduce_noise, restated in
// include/rvc_amd.h; the wheel is absent, parity with it is unpinned) on the converted waveform:
//   complex STFT (1024-point periodic hann, hop 256, 512 zeros on each side) -> |S| -> one-pole smoother forward and backward along
//   time -> sigmoid of the relative excess -> separable triangular smoothing of the mask -> S * mask -> inverse rDFT, window,
//   overlap-add, division by the running sum of win^2.
//
// Both transforms are dense DFTs as GEMMs on the exact-fp32 matrix-core kernel of conv.hip, as in logmel.hip, but with the roles
// swapped: the [cos; -sin] basis is the "activation" [1024][1152] and the windowed frames are the "weights" [1024][frames], so the
// spectrum comes out TIME-major, S[frame][row] (re rows [0, 513), im rows [576, 1089)).  Everything between the two GEMMs then
// reads rows of consecutive bins: the recurrence runs one lane per (chunk, bin) over coalesced rows and needs no scan.  The
// inverse GEMM wants its K axis (the spectral rows) outermost, so the kernel that applies the mask writes S * mask transposed,
// [row][frame], through an LDS tile; its product with the inverse basis [1152][1024] is the time-domain frames [frame][1024].
// Overlap-add is a gather (every output sample sums its <= 4 frames in frame order): no atomics, identical bits on every call.
//
// The chunks of reduce_noise (chunk_size samples, filtered inside +-padding samples of context) are independent; a launch
// processes a GROUP of them side by side (their frames are stacked along the GEMM's M axis), and a long input is walked group by
// group through one workspace whose size depends on chunk_size and padding but not on n.
#include "stft1024.h"

namespace rvc {

// frame length, bins, row layout, the per-device tables and the K-split GEMM helper: stft1024.h (shared with K19, formant.hip)
constexpr int SG_HOP = 256;
constexpr int SG_MP = 576;             // row pitch of the mask buffers
constexpr int SG_MAX_HALF = 50;        // widest smoothing ramp: nf = 50 at 5120 Hz, nt = 50 at 256 kHz
constexpr int64_t SG_GROUP_FRAMES = 8192;              // frames per launch group (at least one chunk)
constexpr int64_t SG_MAX_BUFFER = (int64_t)1 << 27;    // chunk_size + 2 padding: one group's spectrum stays below the GEMM's 4 GB slab

// ---- the geometry of one launch group, the same for every kernel ----------------------------------------------------------------
struct GateGroup {
    int64_t n;            // samples of the whole signal
    int64_t chunk_size, padding;
    int64_t chunk0;       // first chunk of the group
    int n_chunks;         // chunks in the group
    int pitch;            // frames per full-length chunk = rows of S per chunk
    int m_pad;            // n_chunks * pitch rounded up to 128: GEMM rows
};
// chunk c of the group: samples [s, e) of the signal, buffer length L = e - s + 2 padding, L / 256 + 1 frames
__device__ __forceinline__ void gate_chunk(const GateGroup &g, int c, int64_t &s, int64_t &L, int &frames) {
    s = (g.chunk0 + c) * g.chunk_size;
    const int64_t e = s + g.chunk_size < g.n ? s + g.chunk_size : g.n;
    L = e - s + 2 * g.padding;
    frames = (int)(L / SG_HOP) + 1;
}

struct GateRamp { float w[SG_MAX_HALF + 1]; int half; };   // w[|d|]: the normalised triangular taps, by value in the kernel arguments

// F[i][m] = window[i] * c[t * 256 + i - 512], row m = chunk * pitch + t; zero outside the buffer, the signal and the chunk's frames
__global__ void __launch_bounds__(256)
gate_frames_kernel(const float *__restrict__ y, const GateGroup g, const float *__restrict__ window, float *__restrict__ F) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (m >= g.m_pad) return;
    const int c = m / g.pitch, t = m - c * g.pitch;
    float v = 0.f;
    if (c < g.n_chunks) {
        int64_t s, L;
        int frames;
        gate_chunk(g, c, s, L, frames);
        const int64_t j = (int64_t)t * SG_HOP + i - SG_NFFT / 2;
        const int64_t src = s - g.padding + j;
        if (t < frames && j >= 0 && j < L && src >= 0 && src < g.n) v = window[i] * y[src];
    }
    F[(size_t)i * g.m_pad + m] = v;
}

__device__ __forceinline__ float gate_mag(const float *__restrict__ S, size_t row, int k) {
    const float re = S[row * SG_ROWS + k], im = S[row * SG_ROWS + SG_IM0 + k];
    return sqrtf(re * re + im * im);
}

// scipy.signal.filtfilt([b], [1, b - 1], |S|, axis = time, padtype = None), one lane per (chunk, bin):
//   forward   f[t] = b A[t] + (1 - b) f[t - 1],  f[-1] = A[0]            (lfilter_zi: the state of a constant input)
//   backward  M[t] = b f[t] + (1 - b) M[t + 1],  M[T] = f[T - 1]
// The state is float64 (one fma per step either way); f is kept as float in `buf`, which M then overwrites in place.  A chunk is
// ~2.6 k dependent steps on 9 waves, so the kernel is bound by the latency of its loads, not by their number: a batch of
// SG_UNROLL rows is in flight while the batch before it is stepped through (two register buffers, statically indexed).
constexpr int SG_UNROLL = 32;
__global__ void __launch_bounds__(64)
gate_smooth_kernel(const float *__restrict__ S, const GateGroup g, double b, float *__restrict__ buf) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= SG_BINS) return;
    int64_t s, L;
    int T;
    gate_chunk(g, c, s, L, T);
    const size_t row0 = (size_t)c * g.pitch;
    const double a = 1.0 - b;
    double st = (double)gate_mag(S, row0, k);
    typedef float batch[SG_UNROLL];
    // rows past the chunk's ends are clamped for the loads (issued together, never branched around) and skipped by the steps
    auto load_fwd = [&](batch &re, batch &im, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u) {
            const size_t row = row0 + (t0 + u < T ? t0 + u : T - 1);
            re[u] = S[row * SG_ROWS + k];
            im[u] = S[row * SG_ROWS + SG_IM0 + k];
        }
    };
    auto step_fwd = [&](const batch &re, const batch &im, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u)
            if (t0 + u < T) {
                st = fma(a, st, b * (double)sqrtf(re[u] * re[u] + im[u] * im[u]));
                buf[(row0 + t0 + u) * SG_MP + k] = (float)st;
            }
    };
    batch r0, i0, r1, i1;
    load_fwd(r0, i0, 0);
    for (int t0 = 0; t0 < T; t0 += 2 * SG_UNROLL) {
        load_fwd(r1, i1, t0 + SG_UNROLL);
        step_fwd(r0, i0, t0);
        load_fwd(r0, i0, t0 + 2 * SG_UNROLL);
        step_fwd(r1, i1, t0 + SG_UNROLL);
    }
    auto load_bwd = [&](batch &f, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u) f[u] = buf[(row0 + (t0 - u > 0 ? t0 - u : 0)) * SG_MP + k];
    };
    auto step_bwd = [&](const batch &f, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u)
            if (t0 - u >= 0) {
                st = fma(a, st, b * (double)f[u]);
                buf[(row0 + t0 - u) * SG_MP + k] = (float)st;
            }
    };
    load_bwd(r0, T - 1);            // this lane's own stores
    st = (double)r0[0];
    for (int t0 = T - 1; t0 >= 0; t0 -= 2 * SG_UNROLL) {
        load_bwd(r1, t0 - SG_UNROLL);        // rows a batch ahead: not the ones the steps below overwrite
        step_bwd(r0, t0);
        load_bwd(r0, t0 - 2 * SG_UNROLL);
        step_bwd(r1, t0 - SG_UNROLL);
    }
}

// mask0 = 1 / (1 + exp(-((A - M) / M - 2) * 10)) -- a bin with M == 0 (silent in every frame) takes X = 0: finite, and S is 0
// there -- then smoothed along the bins, zero outside [0, 513): out[row][k] = sum_d w[|d|] mask0[row][k + d]; one block per frame
__global__ void __launch_bounds__(256)
gate_freq_smooth_kernel(const float *__restrict__ S, const float *__restrict__ Mbuf, const GateGroup g, const GateRamp ramp,
                        float *__restrict__ out) {
    __shared__ float row[SG_BINS + 2 * SG_MAX_HALF];
    const int t = blockIdx.x, c = blockIdx.y;
    int64_t s, L;
    int T;
    gate_chunk(g, c, s, L, T);
    if (t >= T) return;   // uniform over the block
    const size_t r = (size_t)c * g.pitch + t;
    for (int i = threadIdx.x; i < SG_BINS + 2 * SG_MAX_HALF; i += 256) {
        const int k = i - SG_MAX_HALF;
        float v = 0.f;
        if (k >= 0 && k < SG_BINS) {
            const float A = gate_mag(S, r, k), M = Mbuf[r * SG_MP + k];
            const float X = M > 0.f ? (A - M) / M : 0.f;
            v = 1.f / (1.f + expf(-(X - 2.f) * 10.f));
        }
        row[i] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SG_BINS; k += 256) {
        float acc = 0.f;
        for (int d = -ramp.half; d <= ramp.half; ++d) acc = fmaf(ramp.w[d < 0 ? -d : d], row[k + d + SG_MAX_HALF], acc);
        out[r * SG_MP + k] = acc;
    }
}

// along time, zero outside the chunk's frames; then mask * prop + (1 - prop), S * mask, written transposed: ST[row][m].
// A block is a 32 (frames) x 32 (bins) tile, 256 threads; rows 513..575 and 1089..1151, and frames no chunk owns, become zeros.
__global__ void __launch_bounds__(256)
gate_apply_kernel(const float *__restrict__ S, const float *__restrict__ in, const GateGroup g, const GateRamp ramp, float prop,
                  float *__restrict__ ST) {
    __shared__ float tre[32][33], tim[32][33];
    const int m0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r, k = k0 + tx;
        const int c = m / g.pitch, t = m - c * g.pitch;
        float re = 0.f, im = 0.f;
        if (c < g.n_chunks && k < SG_BINS) {
            int64_t s, L;
            int T;
            gate_chunk(g, c, s, L, T);
            if (t < T) {
                const int lo = t - ramp.half > 0 ? t - ramp.half : 0, hi = t + ramp.half < T - 1 ? t + ramp.half : T - 1;
                float acc = 0.f;
                for (int u = lo; u <= hi; ++u) {
                    const int d = u - t;
                    acc = fmaf(ramp.w[d < 0 ? -d : d], in[((size_t)c * g.pitch + u) * SG_MP + k], acc);
                }
                const float mask = fmaf(acc, prop, 1.f - prop);
                re = S[(size_t)m * SG_ROWS + k] * mask;
                im = S[(size_t)m * SG_ROWS + SG_IM0 + k] * mask;
            }
        }
        tre[r][tx] = re;
        tim[r][tx] = im;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {   // r: bin within the tile, tx: frame
        ST[(size_t)(k0 + r) * g.m_pad + m0 + tx] = tre[tx][r];
        ST[(size_t)(SG_IM0 + k0 + r) * g.m_pad + m0 + tx] = tim[tx][r];
    }
}

// out[s + i] = sum over the frames t that cover buffer sample j = padding + i of window * X[t] / sum of window^2 (frames in
// ascending order); zero from L - L % 256 on (the inverse transform's length)
__global__ void __launch_bounds__(256)
gate_overlap_add_kernel(const float *__restrict__ X, const GateGroup g, const float *__restrict__ window, float *__restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;        // sample of the group
    const int64_t first = g.chunk0 * g.chunk_size;
    const int64_t idx = first + o;
    if (idx >= g.n || o >= (int64_t)g.n_chunks * g.chunk_size) return;
    const int c = (int)(o / g.chunk_size);
    int64_t s, L;
    int T;
    gate_chunk(g, c, s, L, T);
    const int64_t j = g.padding + (idx - s);
    float v = 0.f;
    if (j < L - L % SG_HOP) {
        const int64_t p = j + SG_NFFT / 2;
        int64_t t_lo = (p - (SG_NFFT - 1) + SG_HOP - 1) / SG_HOP, t_hi = p / SG_HOP;    // p >= 512: the numerator may be negative only above -256
        if (t_lo < 0) t_lo = 0;
        if (t_hi > T - 1) t_hi = T - 1;
        float acc = 0.f, norm = 0.f;
        for (int64_t t = t_lo; t <= t_hi; ++t) {
            const int i = (int)(p - t * SG_HOP);
            const float w = window[i];
            acc = fmaf(w, X[((size_t)c * g.pitch + t) * SG_NFFT + i], acc);
            norm = fmaf(w, w, norm);
        }
        v = acc / (norm > 1e-10f ? norm : 1.f);
    }
    out[idx] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct GatePlan {
    int nf = 0, nt = 0;
    double b = 0.0;
    int64_t n_chunks = 0;     // of the whole signal
    int64_t per_group = 0;    // chunks per launch group
    int pitch = 0;            // frames of a full-length chunk
    int m_pad = 0;            // GEMM rows of the largest group
};

static size_t gate_bytes_F(int m_pad) { return align_up((size_t)SG_NFFT * m_pad * 4, 256); }
static size_t gate_bytes_S(int m_pad) { return align_up((size_t)SG_ROWS * m_pad * 4, 256); }
static size_t gate_bytes_M(int m_pad) { return align_up((size_t)SG_MP * m_pad * 4, 256); }

// noisereduce's expressions, float64, in its order of operations
static int gate_params(const char *fn, int sr, int *nf, int *nt, double *b) {
    if (sr < 5120 || sr > 256000) return fail("%s: sr %d outside [5120, 256000] (the mask smoothing filter would be empty)", fn, sr);
    *nf = (int)(500.0 / ((double)sr / 512.0));
    *nt = (int)(50.0 / ((256.0 / (double)sr) * 1000.0));
    const double t = 2.0 * (double)sr / 256.0;
    *b = (sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t);
    if (*nf < 1 || *nt < 1 || *nf > SG_MAX_HALF || *nt > SG_MAX_HALF) return fail("%s: sr %d gives a %d x %d smoothing filter", fn, sr, 2 * *nf + 1, 2 * *nt + 1);
    return 0;
}

// ramp(k) / sum: (k + 1 - |d|) / (k + 1)^2
static void gate_ramp(int half, double *taps) {
    for (int d = 0; d <= half; ++d) taps[d] = (double)(half + 1 - d) / ((double)(half + 1) * (double)(half + 1));
}

static int gate_plan(const char *fn, int64_t n, int sr, int64_t chunk_size, int64_t padding, GatePlan *pl) {
    if (n < 0) return fail("%s: n = %lld is negative", fn, (long long)n);
    if (gate_params(fn, sr, &pl->nf, &pl->nt, &pl->b)) return 1;
    if (chunk_size < 1) return fail("%s: chunk_size %lld must be at least 1", fn, (long long)chunk_size);
    if (padding < 0) return fail("%s: padding %lld is negative", fn, (long long)padding);
    const int64_t full = chunk_size < n ? chunk_size : n;       // the longest chunk of this signal
    if (padding > SG_MAX_BUFFER || full + 2 * padding > SG_MAX_BUFFER)
        return fail("%s: a chunk of %lld samples with %lld of padding on each side exceeds %lld samples", fn, (long long)full, (long long)padding,
                    (long long)SG_MAX_BUFFER);
    pl->n_chunks = n == 0 ? 0 : (n - 1) / chunk_size + 1;
    pl->pitch = (int)((full + 2 * padding) / SG_HOP) + 1;
    pl->per_group = SG_GROUP_FRAMES / pl->pitch > 1 ? SG_GROUP_FRAMES / pl->pitch : 1;
    const int64_t widest = pl->n_chunks < pl->per_group ? pl->n_chunks : pl->per_group;
    pl->m_pad = (int)align_up((size_t)(widest * pl->pitch), 128);
    return 0;
}

static size_t gate_workspace(const GatePlan &pl) {
    if (pl.n_chunks == 0) return 0;
    return gate_bytes_F(pl.m_pad) + 2 * gate_bytes_S(pl.m_pad) + 2 * gate_bytes_M(pl.m_pad);
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_spectral_gate_params(int sr, int *nf, int *nt, double *b, double *freq_taps, double *time_taps) {
    if (!nf || !nt || !b) return fail("rvc_spectral_gate_params: null pointer");
    if (gate_params("rvc_spectral_gate_params", sr, nf, nt, b)) return 1;
    if (freq_taps) gate_ramp(*nf, freq_taps);
    if (time_taps) gate_ramp(*nt, time_taps);
    return 0;
}

extern "C" int rvc_spectral_gate_workspace_bytes(int64_t n, int sr, int64_t chunk_size, int64_t padding, size_t *bytes) {
    if (!bytes) return fail("rvc_spectral_gate_workspace_bytes: null pointer");
    GatePlan pl;
    if (gate_plan("rvc_spectral_gate_workspace_bytes", n, sr, chunk_size, padding, &pl)) return 1;
    *bytes = gate_workspace(pl);
    return 0;
}

extern "C" int rvc_spectral_gate_f32(const float *y_dev, int64_t n, int sr, float prop_decrease, int64_t chunk_size, int64_t padding,
                                     float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_spectral_gate_f32";
    if (!y_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    GatePlan pl;
    if (gate_plan(fn, n, sr, chunk_size, padding, &pl)) return 1;
    if (!(prop_decrease >= 0.f && prop_decrease <= 1.f)) return fail("%s: prop_decrease %g outside [0, 1]", fn, (double)prop_decrease);
    const size_t need = gate_workspace(pl);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (n == 0) return 0;
    GateTables tab;
    if (gate_tables_for_device(&tab)) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;

    GateRamp rf, rt;
    double taps[SG_MAX_HALF + 1];
    memset(&rf, 0, sizeof rf);
    memset(&rt, 0, sizeof rt);
    gate_ramp(pl.nf, taps);
    for (int d = 0; d <= pl.nf; ++d) rf.w[d] = (float)taps[d];
    rf.half = pl.nf;
    gate_ramp(pl.nt, taps);
    for (int d = 0; d <= pl.nt; ++d) rt.w[d] = (float)taps[d];
    rt.half = pl.nt;

    char *ws = (char *)workspace_dev;
    float *F = (float *)ws;                       // windowed frames [1024][m_pad]; later the inverse frames [m_pad][1024]
    float *S = (float *)(ws += gate_bytes_F(pl.m_pad));     // [m_pad][1152]
    float *ST = (float *)(ws += gate_bytes_S(pl.m_pad));    // [1152][m_pad]
    float *M0 = (float *)(ws += gate_bytes_S(pl.m_pad));    // [m_pad][576] forward state, then the smoothed level M
    float *M1 = (float *)(ws += gate_bytes_M(pl.m_pad));    // [m_pad][576] the mask smoothed along the bins

    for (int64_t c0 = 0; c0 < pl.n_chunks; c0 += pl.per_group) {
        GateGroup g;
        g.n = n; g.chunk_size = chunk_size; g.padding = padding; g.chunk0 = c0;
        g.n_chunks = (int)(pl.n_chunks - c0 < pl.per_group ? pl.n_chunks - c0 : pl.per_group);
        g.pitch = pl.pitch;
        g.m_pad = (int)align_up((size_t)g.n_chunks * pl.pitch, 128);   // <= pl.m_pad
        hipLaunchKernelGGL(gate_frames_kernel, dim3((unsigned)ceil_div(g.m_pad, 256), SG_NFFT), dim3(256), 0, stream, y_dev, g, tab.window, F);
        RVC_LAUNCH_CHECK();
        if (gate_gemm(tab.fwd, SG_NFFT, SG_ROWS, F, g.m_pad, S, SG_SPLIT_FWD, stream)) return 1;
        hipLaunchKernelGGL(gate_smooth_kernel, dim3((unsigned)ceil_div(SG_BINS, 64), g.n_chunks), dim3(64), 0, stream, S, g, pl.b, M0);
        RVC_LAUNCH_CHECK();
        hipLaunchKernelGGL(gate_freq_smooth_kernel, dim3(g.pitch, g.n_chunks), dim3(256), 0, stream, S, M0, g, rf, M1);
        RVC_LAUNCH_CHECK();
        hipLaunchKernelGGL(gate_apply_kernel, dim3(g.m_pad / 32, SG_MP / 32), dim3(256), 0, stream, S, M1, g, rt, prop_decrease, ST);
        RVC_LAUNCH_CHECK();
        if (gate_gemm(tab.inv, SG_ROWS, SG_NFFT, ST, g.m_pad, F, SG_SPLIT_INV, stream)) return 1;
        const int64_t first = c0 * chunk_size;
        const int64_t span = (first + (int64_t)g.n_chunks * chunk_size < n ? first + (int64_t)g.n_chunks * chunk_size : n) - first;
        hipLaunchKernelGGL(gate_overlap_add_kernel, dim3((unsigned)ceil_div(span, 256)), dim3(256), 0, stream, F, g, tab.window, out_dev);
        RVC_LAUNCH_CHECK();
    }
    return 0;
}
