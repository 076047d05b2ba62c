// K19 -- formant_shifting: the spectral-envelope edit of stftpitchshift's StftPitchShift(1024, 32, sr).shiftpitch(x, factors=1,
// quefrency, distortion), restated in include/rvc_amd.h (the wheel is absent, parity with it is unpinned), on the 16 kHz input:
//   STFT (1024-point periodic hann, hop 32, no centre padding, scaled 1 / 1024) -> per frame: log10 |S| -> cepstrum up to quefrency
//   Q -> liftered envelope E -> E resampled along the bins by 1 / distortion -> |S| / E * E' with S's phase -> inverse rDFT, window,
//   overlap-add.
//
// Both transforms are K18's: dense DFTs as GEMMs on the exact-fp32 matrix-core kernel of conv.hip with a time-major spectrum
// (stft1024.h: the tables, the K-split helper, the row layout).  The tables carry no 1 / 1024 forward and one inverse, which is the
// contract's scaling moved: Y = G S / |S| is homogeneous in S, so the raw spectrum is scaled only where its magnitude is taken
// (a power of two, exact).  The hop is 32, so a 30 s utterance is 14 969 frames: two launch groups of 8192.
//
// Between the GEMMs, formant_envelope_kernel runs one frame at a time per workgroup with everything in LDS and writes the gain
// ratio G / |S| per (frame, bin); formant_apply_kernel multiplies the spectrum by it and writes the product transposed, through an
// LDS tile, for the inverse GEMM (Q == 0: the ratio is 1 and the envelope kernel is not launched).  The envelope chain is float64:
// its cost is (Q + 1) x 513 multiply-adds twice per frame -- 13 k at the default Q = 12 -- and the cepstrum's leading terms are sums
// of ~1000 logarithms of size 3..5, whose fp32 rounding would reach the output as a relative error of the gain.  Cosines come from
// a 1024-entry table indexed by (q k) mod 1024: exact argument reduction.  The same kernel serves every Q up to 511 (DESIGN, K19).
//
// Overlap-add is a gather: every output sample sums its <= 32 frames in frame order, no atomics.  A group's samples need the 31
// frames before its first; those are kept from the previous group (a 124 KiB copy), so the output does not depend on group_frames.
#include <float.h>

#include "stft1024.h"

namespace rvc {

constexpr int FS_HOP = 32;
constexpr int FS_RP = 576;                 // row pitch of the gain-ratio buffer
constexpr int FS_CARRY = SG_NFFT / FS_HOP - 1;   // 31 frames of the previous group reach into a group's samples
constexpr int FS_GROUP_FRAMES = 8192;
constexpr int64_t FS_MAX_N = (int64_t)1 << 27;
constexpr int FS_MAX_Q = 511;

struct FormantGroup {
    int64_t n;          // samples of the whole signal
    int64_t n_frames;   // frames of the whole signal
    int64_t t0;         // first frame of the group
    int frames;         // frames in the group
    int m_pad;          // frames rounded up to 128: GEMM rows
    int last;           // the group that owns the tail of the signal
};

// costab[i] = cos(2 pi i / 1024) in float64; the warp positions of the contract, in float64 with its own expressions:
// pos = i * (513.0 / m), j = trunc(pos), f = pos - j for i < min(513, m); j = -1 where E' is 0 (i >= m, or j == 512)
__global__ void __launch_bounds__(256)
formant_prologue_kernel(double m, double *__restrict__ costab, double *__restrict__ ftab, int *__restrict__ jtab) {
    for (int i = threadIdx.x; i < SG_NFFT; i += 256) costab[i] = cospi((double)i / 512.0);
    for (int i = threadIdx.x; i < SG_BINS; i += 256) {
        int j = -1;
        double f = 0.0;
        if ((double)i < m) {
            const double pos = (double)i * (513.0 / m);
            const double jt = trunc(pos);
            if (jt < (double)(SG_BINS - 1)) { j = (int)jt; f = pos - jt; }
        }
        jtab[i] = j;
        ftab[i] = f;
    }
}

// F[i][m] = window[i] * x[(t0 + m) * 32 + i]; zero for the rows past the group's frames
__global__ void __launch_bounds__(256)
formant_frames_kernel(const float *__restrict__ x, const FormantGroup g, const float *__restrict__ window, float *__restrict__ F) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (m >= g.m_pad) return;
    float v = 0.f;
    if (m < g.frames) v = window[i] * x[(g.t0 + m) * FS_HOP + i];   // (t0 + m) * 32 + i <= (n_frames - 1) * 32 + 1023 < n
    F[(size_t)i * g.m_pad + m] = v;
}

__device__ __forceinline__ bool not_normal(float v) { return !(fabsf(v) >= FLT_MIN && fabsf(v) <= FLT_MAX); }

// One frame at a time per workgroup (grid-stride over the group's frames), steps 2 and 3 of the contract:
//   Lw[k] = w_k log10 |S[k]| (w = 1 for DC and Nyquist, 2 between);  c[q] = sum_k Lw[k] cos(2 pi q k / 1024), q <= Q, summed as
//   P = 2^floor(log2(256 / (Q + 1))) interleaved partial sums per q (all 256 lanes busy at small Q) that are added in order;
//   c' = lifter(c);  E[k] = 10^(sum_q c'[q] cos(2 pi q k / 1024) / 1024);  G = |S| / E * E';  R[frame][k] = G / |S|.
// A frame with a bin of magnitude 0 has a NaN envelope in the contract and contributes zeros: it is detected and written as zeros.
__global__ void __launch_bounds__(256)
formant_envelope_kernel(const float *__restrict__ S, const FormantGroup g, int Q, int P, int warp, const double *__restrict__ costab_g,
                        const double *__restrict__ ftab, const int *__restrict__ jtab, float *__restrict__ R) {
    __shared__ double costab[SG_NFFT], Lw[SG_BINS], mag[SG_BINS], E[SG_BINS], part[512], cq[512];
    __shared__ int dead;
    const int t = threadIdx.x;
    for (int i = t; i < SG_NFFT; i += 256) costab[i] = costab_g[i];
    if (t == 0) dead = 0;
    __syncthreads();
    for (int row = blockIdx.x; row < g.frames; row += gridDim.x) {
        const float *Sr = S + (size_t)row * SG_ROWS;
        float *Rr = R + (size_t)row * FS_RP;
        for (int k = t; k < SG_BINS; k += 256) {
            const double re = (double)Sr[k], im = (double)Sr[SG_IM0 + k];
            const double a = sqrt(re * re + im * im) * (1.0 / SG_NFFT);
            mag[k] = a;
            if (a == 0.0) dead = 1;
            Lw[k] = (k == 0 || k == SG_NFFT / 2 ? 1.0 : 2.0) * log10(a);
        }
        __syncthreads();
        const int is_dead = dead;
        __syncthreads();               // everyone has read the flag before it is reset
        if (is_dead) {                 // uniform over the block
            for (int k = t; k < SG_BINS; k += 256) Rr[k] = 0.f;
            if (t == 0) dead = 0;
            __syncthreads();
            continue;
        }
        for (int o = t; o < (Q + 1) * P; o += 256) {
            const int q = o / P, p = o - q * P;
            double acc = 0.0;
            for (int k = p; k < SG_BINS; k += P) acc = fma(Lw[k], costab[(q * k) & (SG_NFFT - 1)], acc);
            part[o] = acc;
        }
        __syncthreads();
        for (int q = t; q <= Q; q += 256) {
            double c = part[q * P];
            for (int p = 1; p < P; ++p) c += part[q * P + p];
            cq[q] = (q == 0 || q == Q) ? c : 2.0 * c;      // keep c[0], double c[1 .. Q-1], keep c[Q] once
        }
        __syncthreads();
        // bins t, t + 256 and (lane 0 only) 512 share the broadcast of c'[q]
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int q = 0; q <= Q; ++q) {
            const double c = cq[q];
            a0 = fma(c, costab[(q * t) & (SG_NFFT - 1)], a0);
            a1 = fma(c, costab[(q * (t + 256)) & (SG_NFFT - 1)], a1);
            if (t == 0) a2 = fma(c, costab[(q * 512) & (SG_NFFT - 1)], a2);
        }
        double g1[3];
        const double acc[3] = {a0, a1, a2};
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int k = t + 256 * u;
            g1[u] = 0.0;
            if (k < SG_BINS) {
                const double e = exp10(acc[u] * (1.0 / SG_NFFT));
                const bool masked = not_normal((float)e);
                E[k] = masked ? 0.0 : e;                  // E[mask1] = 0; at distortion 1 the same bins fail mask2
                g1[u] = masked ? 0.0 : mag[k] / e;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int k = t + 256 * u;
            if (k < SG_BINS) {
                double ep = E[k];
                if (warp) {
                    const int j = jtab[k];
                    const double f = ftab[k];
                    ep = j < 0 ? 0.0 : f * E[j + 1] + (1.0 - f) * E[j];
                }
                const double G = not_normal((float)ep) ? 0.0 : g1[u] * ep;
                const float r = (float)(G / mag[k]);       // mag > 0: the frame is not dead
                Rr[k] = not_normal(r) ? 0.f : r;
            }
        }
        __syncthreads();               // LDS is reused by the next frame
    }
}

// S * R (R == nullptr: S itself), written transposed: ST[row][m].  A block is a 32 (frames) x 32 (bins) tile, 256 threads; rows
// 513..575 and 1089..1151, and the rows past the group's frames, become zeros.
__global__ void __launch_bounds__(256)
formant_apply_kernel(const float *__restrict__ S, const float *__restrict__ R, const FormantGroup g, float *__restrict__ ST) {
    __shared__ float tre[32][33], tim[32][33];
    const int m0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r, k = k0 + tx;
        float re = 0.f, im = 0.f;
        if (m < g.frames && k < SG_BINS) {
            const float ratio = R ? R[(size_t)m * FS_RP + k] : 1.f;
            re = S[(size_t)m * SG_ROWS + k] * ratio;
            im = S[(size_t)m * SG_ROWS + SG_IM0 + k] * ratio;
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

// out[s] = sum over the frames t that cover s, ascending, of X[t][s - 32 t] * (window * H / sum of window^2); frames before the
// group's first come from `carry` (rows 0..30 = frames t0 - 31 .. t0 - 1).  The group owns samples [32 t0, 32 (t0 + frames)), the
// last group up to n; samples no frame covers get 0.
__global__ void __launch_bounds__(256)
formant_overlap_add_kernel(const float *__restrict__ X, const float *__restrict__ carry, const FormantGroup g,
                           const float *__restrict__ window, float scale, float *__restrict__ out) {
    const int64_t s0 = g.t0 * FS_HOP;
    const int64_t s1 = g.last ? g.n : (g.t0 + g.frames) * FS_HOP;
    const int64_t s = s0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= s1) return;
    int64_t t_lo = s >= SG_NFFT - 1 ? (s - (SG_NFFT - 1) + FS_HOP - 1) / FS_HOP : 0, t_hi = s / FS_HOP;
    if (t_hi > g.n_frames - 1) t_hi = g.n_frames - 1;
    float acc = 0.f;
    for (int64_t t = t_lo; t <= t_hi; ++t) {      // t_lo >= t0 - 31, t_hi <= t0 + frames - 1
        const int i = (int)(s - t * FS_HOP);
        const float v = t >= g.t0 ? X[(size_t)(t - g.t0) * SG_NFFT + i] : carry[(size_t)(t - (g.t0 - FS_CARRY)) * SG_NFFT + i];
        acc = fmaf(v, window[i] * scale, acc);
    }
    out[s] = acc;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static size_t fs_bytes_F(int m_pad) { return align_up((size_t)SG_NFFT * m_pad * 4, 256); }
static size_t fs_bytes_S(int m_pad) { return align_up((size_t)SG_ROWS * m_pad * 4, 256); }
static size_t fs_bytes_R(int m_pad) { return align_up((size_t)FS_RP * m_pad * 4, 256); }
static size_t fs_bytes_carry() { return align_up((size_t)FS_CARRY * SG_NFFT * 4, 256); }
static size_t fs_bytes_cos() { return (size_t)SG_NFFT * 8; }
static size_t fs_bytes_f() { return align_up((size_t)SG_BINS * 8, 256); }
static size_t fs_bytes_j() { return align_up((size_t)SG_BINS * 4, 256); }

struct FormantPlan {
    int64_t n_frames = 0;
    int group = 0;     // frames per launch group
    int m_pad = 0;     // GEMM rows of the largest group
};

static int formant_plan(const char *fn, int64_t n, int group_frames, FormantPlan *pl) {
    if (n < SG_NFFT) return fail("%s: n = %lld is shorter than one frame of %d samples", fn, (long long)n, SG_NFFT);
    if (n > FS_MAX_N) return fail("%s: n = %lld exceeds %lld samples", fn, (long long)n, (long long)FS_MAX_N);
    if (group_frames != 0 && (group_frames < 128 || group_frames > FS_GROUP_FRAMES || group_frames % 128))
        return fail("%s: group_frames %d is neither 0 nor a multiple of 128 in [128, %d]", fn, group_frames, FS_GROUP_FRAMES);
    pl->n_frames = (n - SG_NFFT) / FS_HOP + 1;
    pl->group = group_frames ? group_frames : FS_GROUP_FRAMES;
    const int64_t widest = pl->n_frames < pl->group ? pl->n_frames : pl->group;
    pl->m_pad = (int)align_up((size_t)widest, 128);
    return 0;
}

static size_t formant_workspace(const FormantPlan &pl) {
    return fs_bytes_F(pl.m_pad) + 2 * fs_bytes_S(pl.m_pad) + fs_bytes_R(pl.m_pad) + fs_bytes_carry() + fs_bytes_cos() + fs_bytes_f() + fs_bytes_j();
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_formant_shift_workspace_bytes(int64_t n, int group_frames, size_t *bytes) {
    if (!bytes) return fail("rvc_formant_shift_workspace_bytes: null pointer");
    FormantPlan pl;
    if (formant_plan("rvc_formant_shift_workspace_bytes", n, group_frames, &pl)) return 1;
    *bytes = formant_workspace(pl);
    return 0;
}

extern "C" int rvc_formant_shift_f32(const float *x_dev, int64_t n, int sr, double quefrency_s, double distortion, int group_frames,
                                     float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_formant_shift_f32";
    if (!x_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (out_dev == x_dev) return fail("%s: out_dev must not alias x_dev", fn);
    FormantPlan pl;
    if (formant_plan(fn, n, group_frames, &pl)) return 1;
    if (sr < 1) return fail("%s: sr %d must be at least 1", fn, sr);
    if (!(quefrency_s >= 0.0)) return fail("%s: quefrency_s %g is negative or not a number", fn, quefrency_s);
    if (!(quefrency_s * (double)sr < (double)(FS_MAX_Q + 1)))
        return fail("%s: quefrency_s %g at sr %d is a quefrency of more than %d samples", fn, quefrency_s, sr, FS_MAX_Q);
    const int Q = (int)(quefrency_s * (double)sr);
    if (!isfinite(distortion) || distortion <= 0.0) return fail("%s: distortion %g must be finite and positive", fn, distortion);
    const double m = trunc((double)SG_BINS * distortion);    // int(513 * distortion), in double
    if (m < 1.0) return fail("%s: distortion %g leaves no bin (int(513 * distortion) = 0)", fn, distortion);
    const size_t need = formant_workspace(pl);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    GateTables tab;
    if (gate_tables_for_device(&tab)) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;

    double sum_w2 = 0.0;
    for (int i = 0; i < SG_NFFT; ++i) {
        const double w = 0.5 - 0.5 * cos(2.0 * M_PI * i / SG_NFFT);
        sum_w2 += w * w;
    }
    const float scale = (float)((double)FS_HOP / sum_w2);

    char *ws = (char *)workspace_dev;
    float *F = (float *)ws;                                 // windowed frames [1024][m_pad]; later the inverse frames [m_pad][1024]
    float *S = (float *)(ws += fs_bytes_F(pl.m_pad));       // [m_pad][1152]
    float *ST = (float *)(ws += fs_bytes_S(pl.m_pad));      // [1152][m_pad]
    float *R = (float *)(ws += fs_bytes_S(pl.m_pad));       // [m_pad][576] gain ratio G / |S|
    float *carry = (float *)(ws += fs_bytes_R(pl.m_pad));   // [31][1024] the previous group's last inverse frames
    double *costab = (double *)(ws += fs_bytes_carry());
    double *ftab = (double *)(ws += fs_bytes_cos());
    int *jtab = (int *)(ws += fs_bytes_f());

    const int warp = distortion != 1.0;
    int P = 1;
    while (2 * P * (Q + 1) <= 256) P *= 2;
    if (Q > 0) {
        hipLaunchKernelGGL(formant_prologue_kernel, dim3(1), dim3(256), 0, stream, m, costab, ftab, jtab);
        RVC_LAUNCH_CHECK();
    }
    for (int64_t t0 = 0; t0 < pl.n_frames; t0 += pl.group) {
        FormantGroup g;
        g.n = n; g.n_frames = pl.n_frames; g.t0 = t0;
        g.frames = (int)(pl.n_frames - t0 < pl.group ? pl.n_frames - t0 : pl.group);
        g.m_pad = (int)align_up((size_t)g.frames, 128);     // <= pl.m_pad
        g.last = t0 + g.frames == pl.n_frames;
        hipLaunchKernelGGL(formant_frames_kernel, dim3((unsigned)ceil_div(g.m_pad, 256), SG_NFFT), dim3(256), 0, stream, x_dev, g, tab.window, F);
        RVC_LAUNCH_CHECK();
        if (gate_gemm(tab.fwd, SG_NFFT, SG_ROWS, F, g.m_pad, S, SG_SPLIT_FWD, stream)) return 1;
        if (Q > 0) {
            const int blocks = g.frames < 2048 ? g.frames : 2048;
            hipLaunchKernelGGL(formant_envelope_kernel, dim3(blocks), dim3(256), 0, stream, S, g, Q, P, warp, costab, ftab, jtab, R);
            RVC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(formant_apply_kernel, dim3(g.m_pad / 32, FS_RP / 32), dim3(256), 0, stream, S, Q > 0 ? R : (const float *)nullptr, g, ST);
        RVC_LAUNCH_CHECK();
        if (gate_gemm(tab.inv, SG_ROWS, SG_NFFT, ST, g.m_pad, F, SG_SPLIT_INV, stream)) return 1;
        const int64_t span = (g.last ? n : (t0 + g.frames) * FS_HOP) - t0 * FS_HOP;
        hipLaunchKernelGGL(formant_overlap_add_kernel, dim3((unsigned)ceil_div(span, 256)), dim3(256), 0, stream, F, carry, g, tab.window, scale, out_dev);
        RVC_LAUNCH_CHECK();
        if (!g.last)   // a group that is not the last holds pl.group >= 128 frames
            RVC_HIP(hipMemcpyAsync(carry, F + (size_t)(g.frames - FS_CARRY) * SG_NFFT, (size_t)FS_CARRY * SG_NFFT * 4, hipMemcpyDeviceToDevice, stream));
    }
    return 0;
}
