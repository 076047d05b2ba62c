// K24 -- the conversion scorer of include/rvc_amd.h: mel-cepstral coefficients, dynamic time warping, an aligned distance sum and
// the F0 tracking sums.
//
// Cepstra.  The power spectrum goes through the WORKSPACE, not LDS: the 1024-point DFT is the K-split GEMM of stft1024.h on the
// exact-fp32 matrix cores (the tables K18 and K19 already keep per device), a group of at most 2048 frames at a time, so the
// scratch does not grow with the signal.  melcep_kernel then owns 8 frames: their power |S|^2 is formed in float64 and held in LDS,
// a wave walks a mel row once for all 8 frames (lanes stride the bins, a fixed xor tree merges them), and the log and the DCT-II
// are float64 per frame.
//
// DTW.  ONE workgroup walks the lattice: no workgroup ever waits on another.  Thread t owns row r0 + t of a pass of R rows
// (R = the workgroup's size: 1024 threads up to dim 32, 512 above), keeps that row of `a` in float64 registers, and at step s
// computes cell (r0 + t, s - t): the cells of one step are an anti-diagonal.  The rows of `b` a step needs live in a ring in LDS
// (R + 32 rows, refilled 32 at a time); D(i, j - 1) is the thread's own register, D(i - 1, j) is what thread t - 1 left in LDS one
// step ago, and D(i - 1, j - 1) is the D(i - 1, j) this thread read one step ago.  The last row of a pass goes to `edge` in the
// workspace for the next pass.  One LDS-only barrier per step.  The choice of predecessor is packed 2 bits per cell, 16 cells per
// word; dtw_backtrace_kernel walks it back in at most Ta + Tb - 1 steps and writes the path forwards.
#include <float.h>
#include <math.h>

#include "common.h"
#include "stft1024.h"

namespace rvc {

// ---- mel cepstra -------------------------------------------------------------------------------------------------------------------
constexpr int MC_GROUP_FRAMES = 2048;
constexpr int MC_TILE = 8;                   // frames per workgroup of melcep_kernel
constexpr int MC_PPITCH = 516;
constexpr int MC_MAX_MELS = 128;
constexpr int MC_MAX_COEF = 40;
constexpr int64_t MC_MAX_N = (int64_t)1 << 27;

// F[i][m] = window[i] * x[(t0 + m) * hop + i - 512], x extended with zeros; zero for the rows past the group's frames
__global__ void __launch_bounds__(256)
melcep_frames_kernel(const float *__restrict__ x, int64_t n, int hop, int64_t t0, int frames, int m_pad, const float *__restrict__ window,
                     float *__restrict__ F) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (m >= m_pad) return;
    float v = 0.f;
    if (m < frames) {
        const int64_t s = (t0 + m) * hop + i - SG_NFFT / 2;
        if (s >= 0 && s < n) v = window[i] * x[s];
    }
    F[(size_t)i * m_pad + m] = v;
}

__global__ void __launch_bounds__(256)
melcep_kernel(const float *__restrict__ S, int frames, int64_t t0, const float *__restrict__ W, int n_mels, int n_coef,
              float *__restrict__ out) {
    __shared__ double P[MC_TILE][MC_PPITCH];
    __shared__ double L[MC_TILE][MC_MAX_MELS];
    const int t = threadIdx.x;
    const int f0 = blockIdx.x * MC_TILE;
    for (int e = t; e < MC_TILE * SG_BINS; e += 256) {
        const int fr = e / SG_BINS, k = e - fr * SG_BINS;
        double p = 0.0;
        if (f0 + fr < frames) {
            const float *row = S + (size_t)(f0 + fr) * SG_ROWS;
            const double re = (double)row[k], im = (double)row[SG_IM0 + k];
            p = fma(im, im, re * re);
        }
        P[fr][k] = p;
    }
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    for (int m = wave; m < n_mels; m += 4) {
        double acc[MC_TILE];
#pragma unroll
        for (int fr = 0; fr < MC_TILE; ++fr) acc[fr] = 0.0;
        const float *wr = W + (size_t)m * SG_BINS;
        for (int k = lane; k < SG_BINS; k += 64) {
            const double w = (double)wr[k];
#pragma unroll
            for (int fr = 0; fr < MC_TILE; ++fr) acc[fr] = fma(w, P[fr][k], acc[fr]);
        }
#pragma unroll
        for (int fr = 0; fr < MC_TILE; ++fr) {
            double v = acc[fr];
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) L[fr][m] = 0.5 * log(fmax(v, 1e-10));
        }
    }
    __syncthreads();
    const int period = 4 * n_mels;
    for (int e = t; e < MC_TILE * n_coef; e += 256) {
        const int fr = e / n_coef, k = e - fr * n_coef + 1;
        if (f0 + fr >= frames) continue;
        double acc = 0.0;
        for (int m = 0; m < n_mels; ++m) {
            const int ph = (k * (2 * m + 1)) % period;        // exact argument reduction
            acc = fma(L[fr][m], cospi((double)ph / (double)(2 * n_mels)), acc);
        }
        out[(size_t)(t0 + f0 + fr) * n_coef + (k - 1)] = (float)(acc / (double)n_mels);
    }
}

static size_t mc_bytes_F(int m_pad) { return align_up((size_t)SG_NFFT * m_pad * 4, 256); }
static size_t mc_bytes_S(int m_pad) { return align_up((size_t)SG_ROWS * m_pad * 4, 256); }
static int mc_m_pad(int64_t frames) {
    return (int)align_up((size_t)(frames < MC_GROUP_FRAMES ? frames : MC_GROUP_FRAMES), 128);
}

static int mc_check(const char *fn, int64_t n, int sr) {
    if (n < 1) return fail("%s: n = %lld must be at least 1", fn, (long long)n);
    if (n > MC_MAX_N) return fail("%s: n = %lld exceeds %lld samples", fn, (long long)n, (long long)MC_MAX_N);
    if (sr < 8000 || sr > 48000 || sr % 200) return fail("%s: sr %d must be a multiple of 200 in 8000 .. 48000", fn, sr);
    return 0;
}

// ---- DTW ---------------------------------------------------------------------------------------------------------------------------
constexpr int DTW_MAX_T = 16384;
constexpr int DTW_MAX_DIM = 64;
constexpr int DTW_CHUNK = 32;                // rows of b staged at a time

__device__ __forceinline__ bool dtw_admissible(bool banded, int64_t i, int64_t j, int64_t ta1, int64_t tb1, int64_t lim) {
    if (!banded) return true;
    const int64_t v = j * ta1 - i * tb1;
    return (v < 0 ? -v : v) <= lim;
}

template <int DP, int R>
struct DtwLds {
    static constexpr int RB = R + DTW_CHUNK;       // ring rows
    static constexpr int PITCH = DP + 2;           // floats; (DP + 2) / 2 is odd: 8-byte reads of consecutive rows spread over the banks
    static constexpr int BYTES = 2 * R * 8 + DTW_CHUNK * 8 + RB * PITCH * 4;
};

// BANDED = false drops the admissibility test from the cell (the guard around the distance costs the unbanded walk 10 %)
template <int DP, int R, bool BANDED>
__global__ void __launch_bounds__(R)
dtw_kernel(const float *__restrict__ a, const float *__restrict__ b, int Ta, int Tb, int dim, int64_t band, double *__restrict__ edge,
           uint32_t *__restrict__ bp, int bp_pitch, double *__restrict__ out) {
    using Lds = DtwLds<DP, R>;
    static_assert(DP % 4 == 0 && Lds::BYTES <= LDS_WHOLE_CU, "K24: the DTW ring does not fit the LDS of a CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char dtw_lds[];
    double *dbuf = (double *)dtw_lds;              // [2][R]   D of the previous and of this step, by thread
    double *eds = dbuf + 2 * R;                    // [32]     D(r0 - 1, j) of the staged columns (inf where there is none)
    float *ring = (float *)(eds + DTW_CHUNK);      // [RB][PITCH] rows of b
    const int t = threadIdx.x;
    const double inf = (double)INFINITY;
    const int64_t ta1 = Ta - 1, tb1 = Tb - 1;
    const bool banded = BANDED && band > 0 && Ta > 1 && Tb > 1;
    const int64_t lim = banded ? band * (ta1 > tb1 ? ta1 : tb1) : 0;

    for (int r0 = 0; r0 < Ta; r0 += R) {
        const int rows = Ta - r0 < R ? Ta - r0 : R;
        const int r1 = r0 + rows - 1;
        int jlo = 0, jhi = Tb - 1;                 // no cell of this pass outside [jlo, jhi] is admissible
        if (banded) {
            const int64_t lo = (int64_t)r0 * tb1 - lim, hi = ((int64_t)r1 * tb1 + lim) / ta1;
            jlo = lo <= 0 ? 0 : (int)((lo + ta1 - 1) / ta1);
            if (hi < jhi) jhi = (int)hi;
        }
        const int i = r0 + t;
        const bool row_on = t < rows;
        double ar[DP];
#pragma unroll
        for (int q = 0; q < DP; ++q) ar[q] = (row_on && q < dim) ? (double)a[(size_t)i * dim + q] : 0.0;
        double left = inf, prev_up = inf;
        uint32_t word = 0;
        const int s_begin = jlo & ~(DTW_CHUNK - 1), s_end = jhi + rows - 1;
        __syncthreads();                           // the previous pass is done with the LDS and its `edge` stores are visible
        // The diagonal predecessor of the pass's first cell (r0, jlo) is D(r0 - 1, jlo - 1): a cell of the PREVIOUS pass, admissible
        // whenever the band's lower edge of row r0 - 1 lies below jlo.  This pass stores edge[j] for j >= jlo only.
        if (BANDED && t == 0 && r0 > 0 && jlo > 0 && dtw_admissible(banded, r0 - 1, jlo - 1, ta1, tb1, lim)) prev_up = edge[jlo - 1];
        // ring slots without a division per cell: sslot = s mod RB, slot = (s - t) mod RB, both stepped with s
        int sslot = s_begin % Lds::RB;
        int slot = (s_begin - t) % Lds::RB;
        if (slot < 0) slot += Lds::RB;
        for (int s = s_begin; s <= s_end; ++s) {
            if ((s & (DTW_CHUNK - 1)) == 0) {
                for (int e = t; e < DTW_CHUNK * DP; e += R) {
                    const int rr = e / DP, q = e - rr * DP, jj = s + rr;
                    const int rs = sslot + rr < Lds::RB ? sslot + rr : sslot + rr - Lds::RB;
                    ring[rs * Lds::PITCH + q] = (q < dim && jj < Tb) ? b[(size_t)jj * dim + q] : 0.f;
                }
                if (t < DTW_CHUNK) {
                    const int jj = s + t;
                    eds[t] = (r0 > 0 && jj < Tb && dtw_admissible(banded, r0 - 1, jj, ta1, tb1, lim)) ? edge[jj] : inf;
                }
                __syncthreads();
            }
            const int j = s - t;
            if (row_on && j >= jlo && j <= jhi) {
                double d = inf;                    // an inadmissible cell: D = inf whatever its predecessors hold
                if (!BANDED || dtw_admissible(banded, i, j, ta1, tb1, lim)) {     // neighbouring rows leave the band together: mostly wave-uniform
                    const float *br = ring + slot * Lds::PITCH;
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < DP; q += 2) {
                        const float2 v = *(const float2 *)(br + q);
                        const double d0 = ar[q] - (double)v.x, d1 = ar[q + 1] - (double)v.y;
                        acc = fma(d0, d0, acc);
                        acc = fma(d1, d1, acc);
                    }
                    d = sqrt(acc);
                }
                const double up = t == 0 ? eds[j & (DTW_CHUNK - 1)] : dbuf[((s - 1) & 1) * R + t - 1];
                double best = prev_up;             // D(i - 1, j - 1)
                uint32_t code = 0;
                if (up < best) { best = up; code = 1; }
                if (left < best) { best = left; code = 2; }
                const double D = (i == 0 && j == 0) ? d : d + best;
                prev_up = up;
                left = D;
                dbuf[(s & 1) * R + t] = D;
                word |= code << (2 * (j & 15));
                if ((j & 15) == 15 || j == jhi) {
                    bp[(size_t)i * bp_pitch + (j >> 4)] = word;
                    word = 0;
                }
                if (t == rows - 1 && r1 < Ta - 1) edge[j] = D;
                if (i == Ta - 1 && j == Tb - 1) out[0] = D;
            }
            lds_barrier();
            sslot = sslot + 1 == Lds::RB ? 0 : sslot + 1;
            slot = slot + 1 == Lds::RB ? 0 : slot + 1;
        }
    }
}

__global__ void __launch_bounds__(256)
dtw_backtrace_kernel(const uint32_t *__restrict__ bp, int bp_pitch, int Ta, int Tb, int *__restrict__ rev, int *__restrict__ path,
                     double *__restrict__ out) {
    __shared__ int len;
    const int t = threadIdx.x;
    if (t == 0) {
        int i = Ta - 1, j = Tb - 1, n = 0;
        const int cap = Ta + Tb - 1;
        for (int step = 0; step < cap; ++step) {
            rev[2 * n] = i;
            rev[2 * n + 1] = j;
            ++n;
            if (i == 0 && j == 0) break;
            uint32_t code = (bp[(size_t)i * bp_pitch + (j >> 4)] >> (2 * (j & 15))) & 3u;
            if (i == 0) code = 2;
            else if (j == 0) code = 1;
            if (code == 1) --i;
            else if (code == 2) --j;
            else { --i; --j; }
        }
        len = n;
        out[1] = (double)n;
    }
    __syncthreads();
    const int L = len;
    for (int k = t; k < L; k += 256) {
        path[2 * k] = rev[2 * (L - 1 - k)];
        path[2 * k + 1] = rev[2 * (L - 1 - k) + 1];
    }
}

static int dtw_pitch(int Tb) { return (Tb + 15) / 16; }
static size_t dtw_bytes_edge(int Tb) { return align_up((size_t)Tb * 8, 256); }
static size_t dtw_bytes_bp(int Ta, int Tb) { return align_up((size_t)Ta * dtw_pitch(Tb) * 4, 256); }
static size_t dtw_bytes_rev(int Ta, int Tb) { return align_up((size_t)(Ta + Tb - 1) * 8, 256); }

static int dtw_check_t(const char *fn, int64_t Ta, int64_t Tb) {
    if (Ta < 1 || Ta > DTW_MAX_T) return fail("%s: Ta = %lld must lie in 1 .. %d", fn, (long long)Ta, DTW_MAX_T);
    if (Tb < 1 || Tb > DTW_MAX_T) return fail("%s: Tb = %lld must lie in 1 .. %d", fn, (long long)Tb, DTW_MAX_T);
    return 0;
}

template <int DP, int R, bool BANDED>
static int dtw_launch_banded(const float *a, const float *b, int Ta, int Tb, int dim, int64_t band, double *edge, uint32_t *bp, double *out,
                      hipStream_t stream) {
    constexpr int lds_bytes = DtwLds<DP, R>::BYTES;
    if (reserve_lds((const void *)dtw_kernel<DP, R, BANDED>, lds_bytes, "rvc_dtw_f64")) return 1;
    hipLaunchKernelGGL((dtw_kernel<DP, R, BANDED>), dim3(1), dim3(R), (size_t)lds_bytes, stream, a, b, Ta, Tb, dim, band, edge, bp, dtw_pitch(Tb),
                       out);
    RVC_LAUNCH_CHECK();
    return 0;
}

template <int DP, int R>
static int dtw_launch(const float *a, const float *b, int Ta, int Tb, int dim, int64_t band, double *edge, uint32_t *bp, double *out,
                      hipStream_t stream) {
    return band > 0 ? dtw_launch_banded<DP, R, true>(a, b, Ta, Tb, dim, band, edge, bp, out, stream)
                    : dtw_launch_banded<DP, R, false>(a, b, Ta, Tb, dim, band, edge, bp, out, stream);
}

// ---- aligned distance sum ------------------------------------------------------------------------------------------------------------
// thread t adds d(f, f) for f = t, t + 256, ... in order; thread 0 adds the 256 partial sums in thread order
__global__ void __launch_bounds__(256)
frame_dist_sum_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t T, int dim, double *__restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double part = 0.0;
    for (int64_t f = t; f < T; f += 256) {
        const float *ar = a + f * dim, *br = b + f * dim;
        double acc = 0.0;
        for (int q = 0; q < dim; ++q) {
            const double d = (double)ar[q] - (double)br[q];
            acc = fma(d, d, acc);
        }
        part += sqrt(acc);
    }
    red[t] = part;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int k = 0; k < 256; ++k) s += red[k];
        out[0] = s;
    }
}

// ---- F0 tracking sums ----------------------------------------------------------------------------------------------------------------
constexpr int F0_SUMS = 12;

// dst[c] = sum of v[c] over the threads, in thread order, for c < ncomp (every thread receives them)
__device__ __forceinline__ void f0_merge(double *red, const double *v, int ncomp, double *dst) {
    const int t = threadIdx.x;
    for (int c = 0; c < ncomp; ++c) red[c * 256 + t] = v[c];
    __syncthreads();
    if (t < ncomp) {
        double acc = 0.0;
        for (int k = 0; k < 256; ++k) acc += red[t * 256 + k];
        dst[t] = acc;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256)
f0_track_sums_kernel(const double *__restrict__ fa, const double *__restrict__ fb, int64_t n, double gross, double *__restrict__ out) {
    __shared__ double red[10 * 256];
    __shared__ double tot[10];
    const int t = threadIdx.x;
    double v[10];
    for (int c = 0; c < 10; ++c) v[c] = 0.0;
    for (int64_t f = t; f < n; f += 256) {
        const double x = fa[f], y = fb[f];
        const bool va = x > 0.0, vb = y > 0.0;       // NaN compares false: unvoiced
        if (va && vb) {
            const double la = log2(x), lb = log2(y), r = 1200.0 * log2(y / x);
            v[0] += 1.0;
            v[1] += r;
            v[2] += la;
            v[3] += lb;
            v[4] = fma(la, la, v[4]);
            v[5] = fma(lb, lb, v[5]);
            v[6] = fma(la, lb, v[6]);
        } else if (va) {
            v[7] += 1.0;
        } else if (vb) {
            v[8] += 1.0;
        } else {
            v[9] += 1.0;
        }
    }
    f0_merge(red, v, 10, tot);
    const double count = tot[0];
    const double rbar = count > 0.0 ? tot[1] / count : 0.0;
    double w[2] = {0.0, 0.0};
    for (int64_t f = t; f < n; f += 256) {
        const double x = fa[f], y = fb[f];
        if (x > 0.0 && y > 0.0) {
            const double e = 1200.0 * log2(y / x) - rbar;
            w[0] = fma(e, e, w[0]);
            if (fabs(e) > gross) w[1] += 1.0;
        }
    }
    if (t < 10) out[t < 7 ? t : t + 2] = tot[t];
    __syncthreads();
    f0_merge(red, w, 2, tot);
    if (t < 2) out[7 + t] = tot[t];
}

static bool cs_misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_melcep_workspace_bytes(int64_t n, int sr, size_t *bytes) {
    const char *fn = "rvc_melcep_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (mc_check(fn, n, sr)) return 1;
    const int m_pad = mc_m_pad(1 + n / (sr / 200));
    *bytes = mc_bytes_F(m_pad) + mc_bytes_S(m_pad);
    return 0;
}

extern "C" int rvc_melcep_f32(const float *x_dev, int64_t n, int sr, const float *mel_dev, int n_mels, int n_coef, float *out_dev,
                              void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_melcep_f32";
    if (!x_dev || !mel_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (cs_misaligned(x_dev, 4) || cs_misaligned(mel_dev, 4) || cs_misaligned(out_dev, 4) || cs_misaligned(workspace_dev, 4))
        return fail("%s: misaligned pointer (4 bytes)", fn);
    if (mc_check(fn, n, sr)) return 1;
    if (n_coef < 1 || n_coef > MC_MAX_COEF) return fail("%s: n_coef = %d must lie in 1 .. %d", fn, n_coef, MC_MAX_COEF);
    if (n_mels <= n_coef || n_mels > MC_MAX_MELS)
        return fail("%s: n_mels = %d must lie in n_coef + 1 = %d .. %d", fn, n_mels, n_coef + 1, MC_MAX_MELS);
    const int hop = sr / 200;
    const int64_t frames = 1 + n / hop;
    const int m_pad = mc_m_pad(frames);
    const size_t need = mc_bytes_F(m_pad) + mc_bytes_S(m_pad);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    GateTables tab;
    if (gate_tables_for_device(&tab)) return 1;
    float *F = (float *)workspace_dev;                                    // [1024][gm] windowed frames
    float *S = (float *)((char *)workspace_dev + mc_bytes_F(m_pad));      // [gm][1152]
    for (int64_t t0 = 0; t0 < frames; t0 += MC_GROUP_FRAMES) {
        const int g = (int)(frames - t0 < MC_GROUP_FRAMES ? frames - t0 : MC_GROUP_FRAMES);
        const int gm = (int)align_up((size_t)g, 128);                     // <= m_pad
        hipLaunchKernelGGL(melcep_frames_kernel, dim3((unsigned)ceil_div(gm, 256), SG_NFFT), dim3(256), 0, stream, x_dev, n, hop, t0, g, gm,
                           (const float *)tab.window, F);
        RVC_LAUNCH_CHECK();
        if (gate_gemm(tab.fwd, SG_NFFT, SG_ROWS, F, gm, S, SG_SPLIT_FWD, stream)) return 1;
        hipLaunchKernelGGL(melcep_kernel, dim3((unsigned)ceil_div(g, MC_TILE)), dim3(256), 0, stream, (const float *)S, g, t0, mel_dev,
                           n_mels, n_coef, out_dev);
        RVC_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int rvc_dtw_workspace_bytes(int64_t Ta, int64_t Tb, size_t *bytes) {
    const char *fn = "rvc_dtw_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (dtw_check_t(fn, Ta, Tb)) return 1;
    *bytes = dtw_bytes_edge((int)Tb) + dtw_bytes_bp((int)Ta, (int)Tb) + dtw_bytes_rev((int)Ta, (int)Tb);
    return 0;
}

extern "C" int rvc_dtw_f64(const float *a_dev, int64_t Ta, const float *b_dev, int64_t Tb, int dim, int64_t band, double *out_dev,
                           int *path_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_dtw_f64";
    if (!a_dev || !b_dev || !out_dev || !path_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (cs_misaligned(a_dev, 4) || cs_misaligned(b_dev, 4) || cs_misaligned(path_dev, 4) || cs_misaligned(out_dev, 8) ||
        cs_misaligned(workspace_dev, 8))
        return fail("%s: misaligned pointer (features and path 4 bytes, out and workspace 8)", fn);
    if (dtw_check_t(fn, Ta, Tb)) return 1;
    if (dim < 1 || dim > DTW_MAX_DIM) return fail("%s: dim = %d must lie in 1 .. %d", fn, dim, DTW_MAX_DIM);
    if (band == 0) return fail("%s: band = 0 admits no path; pass a negative band for none, or at least 1", fn);
    if (band > ((int64_t)1 << 31)) band = (int64_t)1 << 31;     // wider than any lattice: band * 16383 stays inside int64
    const int ta = (int)Ta, tb = (int)Tb;
    const size_t need = dtw_bytes_edge(tb) + dtw_bytes_bp(ta, tb) + dtw_bytes_rev(ta, tb);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    double *edge = (double *)workspace_dev;
    uint32_t *bp = (uint32_t *)((char *)workspace_dev + dtw_bytes_edge(tb));
    int *rev = (int *)((char *)bp + dtw_bytes_bp(ta, tb));
    int rc;
    if (dim <= 8) rc = dtw_launch<8, 1024>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    else if (dim <= 16) rc = dtw_launch<16, 1024>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    else if (dim <= 24) rc = dtw_launch<24, 1024>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    else if (dim <= 32) rc = dtw_launch<32, 1024>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    else if (dim <= 48) rc = dtw_launch<48, 512>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    else rc = dtw_launch<64, 512>(a_dev, b_dev, ta, tb, dim, band, edge, bp, out_dev, stream);
    if (rc) return 1;
    hipLaunchKernelGGL(dtw_backtrace_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t *)bp, dtw_pitch(tb), ta, tb, rev, path_dev,
                       out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_frame_dist_sum_f64(const float *a_dev, const float *b_dev, int64_t T, int dim, double *out_dev, void *hip_stream) {
    const char *fn = "rvc_frame_dist_sum_f64";
    if (!a_dev || !b_dev || !out_dev) return fail("%s: null pointer", fn);
    if (cs_misaligned(a_dev, 4) || cs_misaligned(b_dev, 4) || cs_misaligned(out_dev, 8))
        return fail("%s: misaligned pointer (features 4 bytes, out 8)", fn);
    if (T < 1 || T > ((int64_t)1 << 24)) return fail("%s: T = %lld must lie in 1 .. 2^24", fn, (long long)T);
    if (dim < 1 || dim > DTW_MAX_DIM) return fail("%s: dim = %d must lie in 1 .. %d", fn, dim, DTW_MAX_DIM);
    hipLaunchKernelGGL(frame_dist_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, a_dev, b_dev, T, dim, out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_f0_track_sums_f64(const double *f0_a_dev, const double *f0_b_dev, int64_t n, double *out_dev, void *hip_stream) {
    const char *fn = "rvc_f0_track_sums_f64";
    if (!f0_a_dev || !f0_b_dev || !out_dev) return fail("%s: null pointer", fn);
    if (cs_misaligned(f0_a_dev, 8) || cs_misaligned(f0_b_dev, 8) || cs_misaligned(out_dev, 8)) return fail("%s: misaligned pointer (8 bytes)", fn);
    if (n < 1 || n > ((int64_t)1 << 27)) return fail("%s: n = %lld must lie in 1 .. 2^27", fn, (long long)n);
    hipLaunchKernelGGL(f0_track_sums_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, f0_a_dev, f0_b_dev, n, 1200.0 * log2(1.2),
                       out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}
