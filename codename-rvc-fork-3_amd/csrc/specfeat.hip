// K23 -- the audio analyzer's spectral features of include/rvc_amd.h: librosa's stft(n_fft = 2048, hop 512, center, zero padding)
// -> |S| -> spectral centroid, bandwidth (p = 2) and roll-off per frame, and amplitude_to_db(|S|, ref = max) on request.
//
// specfeat_kernel is the hot one.  A workgroup (8 waves) owns 32 frames and ALL 1025 bins of them, because the roll-off needs a
// frame's whole spectrum twice (its sum, then the cumulative sum against a share of it).  It walks the bins in two groups of 512
// (a wave holds two 32 x 32 tiles, re and im) and runs the DFT as a GEMM on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32:
// A = windowed frames, B = cos | -sin looked up at (i k) mod 2048 in one period of the cosine in LDS, exact argument reduction),
// K20's form: a dot product is summed as fmaf chains of 64 samples whose sums are added in order, and the Nyquist bin rides in the
// imaginary slot of bin 0.  The magnitudes of the 32 frames stay in LDS (128 KiB), which leaves no room for the 70 KiB of samples
// K20 stages at once: the windowed samples are staged one 64-sample chain at a time (8 KiB), the next chain's loads in flight
// under the matrix instructions of the current one.  Zero padding is resolved while staging.
//
// The feature passes then run on the magnitudes in LDS in float64, 16 lanes per frame, each over 64 consecutive bins (the last one
// over 65), their partial sums merged in bin order: the sum, the centroid, and in one more pass the second central moment and the
// roll-off scan (TWO-PASS bandwidth: the centroid is known before the deviations are squared).  The planes are copied out of LDS
// only where the caller asked for them; the dB plane first receives magnitudes and is converted in place by specfeat_db_kernel
// once the maximum over the whole signal is known (per-workgroup maxima, merged per launch group).  No atomics: two calls give
// identical bits.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace rvc {

constexpr int SF_N = 2048;
constexpr int SF_HOP = 512;
constexpr int SF_BINS = 1025;
constexpr int SF_TILE_FRAMES = 32;
constexpr int SF_THREADS = 512;              // 8 waves, two per SIMD: one wave's table lookups and barriers hide under the other's MFMAs
constexpr int SF_WAVES = SF_THREADS / 64;
constexpr int SF_BIN_GROUPS = (SF_N / 2) / (SF_WAVES * 64);     // a wave holds 64 bins at a time
constexpr int SF_STAGE = SF_TILE_FRAMES * 64 / SF_THREADS;      // samples of a chain one thread stages
constexpr int SF_LPF = SF_THREADS / SF_TILE_FRAMES;             // lanes per frame in the feature passes
constexpr int SF_LANE_BINS = (SF_N / 2) / SF_LPF;               // consecutive bins of one such lane
constexpr int SF_CHAIN = 64;                 // samples per fmaf chain = samples staged at a time
constexpr int SF_APITCH = SF_CHAIN + 1;      // row pitch of the staged chain: lanes of different frames hit different banks
constexpr int SF_GROUP_TILES = 128;          // workgroups per launch: the workspace does not grow beyond one group
constexpr int SF_PART0 = 64;                 // workspace, in floats: [0] the running maximum, [64 ..] one maximum per workgroup
constexpr int64_t SF_MAX_N = (int64_t)1 << 27;
// LDS: one double and one int of reduction scratch per thread, the cosine period, one staged chain, the magnitudes
constexpr int SF_LDS_BYTES = SF_THREADS * 8 + SF_THREADS * 4 + (SF_N + SF_TILE_FRAMES * SF_APITCH + SF_TILE_FRAMES * SF_BINS) * 4;
static_assert(SF_LDS_BYTES <= LDS_WHOLE_CU, "K23 does not fit the LDS of a CU");

// the samples this thread stages of the chain that starts at window position k0: column kc of frames fr0, fr0 + SF_WAVES, ...
__device__ __forceinline__ void sf_fetch(const float *__restrict__ x, int64_t n, int64_t s0, float (&pre)[SF_STAGE]) {
#pragma unroll
    for (int j = 0; j < SF_STAGE; ++j) {
        const int64_t s = s0 + (int64_t)j * SF_WAVES * SF_HOP;
        pre[j] = (s >= 0 && s < n) ? x[s] : 0.f;     // center = True, pad_mode = "constant"
    }
}

__global__ void __launch_bounds__(SF_THREADS)
specfeat_kernel(const float *__restrict__ x, int64_t n, int64_t frames, int64_t tile0, double fstep, double roll,
                float *__restrict__ mag_out, float *__restrict__ db_out, double *__restrict__ cent, double *__restrict__ bw,
                double *__restrict__ rolloff, float *__restrict__ part_max) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    double *red = (double *)lds;                    // [SF_THREADS]
    int *cand = (int *)(red + SF_THREADS);          // [SF_THREADS]
    float *tab = (float *)(cand + SF_THREADS);      // [2048]  cos(2 pi j / 2048)
    float *A = tab + SF_N;                          // [32][65] the windowed samples of one chain
    float *mag = A + SF_TILE_FRAMES * SF_APITCH;    // [32][1025]
    const int t = threadIdx.x;
    for (int j = t; j < SF_N; j += SF_THREADS) tab[j] = (float)cospi(2.0 * (double)j / (double)SF_N);

    const int64_t t0 = (tile0 + blockIdx.x) * SF_TILE_FRAMES;
    const int live = frames - t0 < SF_TILE_FRAMES ? (int)(frames - t0) : SF_TILE_FRAMES;   // >= 1
    const int kc = t & 63, fr0 = t >> 6;            // staging: sample column and first frame row
    const int64_t s_stage = (t0 + fr0) * SF_HOP - SF_N / 2 + kc;
    const int lane = t & 63, wave = t >> 6;
    const int fi = lane & 31, kk = lane >> 5;
    const float *fa = A + fi * SF_APITCH;

    for (int grp = 0; grp < SF_BIN_GROUPS; ++grp) {
        int bin[2];
        bin[0] = (grp * SF_WAVES + wave) * 64 + fi;
        bin[1] = bin[0] + 32;
        f32x16 acc[4], run[4];     // [2 u + 0/1]: re, im of bin tile u
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
        float pre[SF_STAGE];
        sf_fetch(x, n, s_stage, pre);
        for (int k0 = 0; k0 < SF_N; k0 += SF_CHAIN) {
            __syncthreads();       // the previous chain has been read (first pass: the table is written)
            const float wv = (float)(0.5 - 0.5 * cospi(2.0 * (double)(k0 + kc) / (double)SF_N));
#pragma unroll
            for (int j = 0; j < SF_STAGE; ++j) A[(fr0 + SF_WAVES * j) * SF_APITCH + kc] = pre[j] * wv;
            __syncthreads();
            if (k0 + SF_CHAIN < SF_N) sf_fetch(x, n, s_stage + k0 + SF_CHAIN, pre);   // in flight under the chain below
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) run[a][r] = 0.f;
            for (int k = 0; k < SF_CHAIN; k += 2) {
                const int ka = k + kk;
                const float av = fa[ka];
                const int kabs = k0 + ka;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int idx = (kabs * bin[u]) & (SF_N - 1);
                    const float c = tab[idx];
                    float s = tab[(idx + SF_N / 4) & (SF_N - 1)];          // cos(a + pi / 2) = -sin a
                    if (bin[u] == 0) s = (kabs & 1) ? -1.f : 1.f;          // the Nyquist bin in bin 0's imaginary slot
                    run[2 * u] = mfma32(av, c, run[2 * u]);
                    run[2 * u + 1] = mfma32(av, s, run[2 * u + 1]);
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] += run[a];
        }
        // |S| in float64 from the fp32 re and im, rounded to fp32; frames past the signal's last one hold zeros
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma32_row(r, lane);
                const bool on = row < live;
                const double re = (double)acc[2 * u][r], im = (double)acc[2 * u + 1][r];
                float *mr = mag + row * SF_BINS;
                if (bin[u] == 0) {
                    mr[0] = on ? (float)fabs(re) : 0.f;
                    mr[SF_N / 2] = on ? (float)fabs(im) : 0.f;
                } else {
                    mr[bin[u]] = on ? (float)sqrt(re * re + im * im) : 0.f;
                }
            }
    }
    __syncthreads();

    // ---- the features: lane j of SF_LPF owns SF_LANE_BINS consecutive bins of frame f, the last lane bin 1024 too ------------------
    const int f = t / SF_LPF, j = t % SF_LPF;
    const float *row = mag + f * SF_BINS;
    const int kb = j * SF_LANE_BINS, ke = j == SF_LPF - 1 ? SF_BINS : kb + SF_LANE_BINS;
    double part = 0.0;
    for (int k = kb; k < ke; ++k) part += (double)row[k];
    red[t] = part;
    __syncthreads();
    double s0 = 0.0, base = 0.0;           // base: the cumulative sum in front of this lane's bins
    for (int i = 0; i < SF_LPF; ++i) {
        if (i == j) base = s0;
        s0 += red[f * SF_LPF + i];
    }
    __syncthreads();
    const double den = s0 < (double)FLT_MIN ? 1.0 : s0;      // normalize(norm = 1): a sum below `tiny` divides by 1
    part = 0.0;
    for (int k = kb; k < ke; ++k) part += ((double)k * fstep) * ((double)row[k] / den);
    red[t] = part;
    __syncthreads();
    double c = 0.0;
    for (int i = 0; i < SF_LPF; ++i) c += red[f * SF_LPF + i];
    __syncthreads();
    const double thr = roll * s0;
    double cum = base;
    int first = INT_MAX;
    part = 0.0;
    for (int k = kb; k < ke; ++k) {
        const double m = (double)row[k], d = (double)k * fstep - c;
        part += (m / den) * (d * d);
        cum += m;
        if (first == INT_MAX && cum >= thr) first = k;
    }
    red[t] = part;
    cand[t] = first;
    __syncthreads();
    if (j == 0 && f < live) {
        double b = 0.0;
        int k1 = INT_MAX;
        for (int i = 0; i < SF_LPF; ++i) {
            b += red[f * SF_LPF + i];
            if (cand[f * SF_LPF + i] < k1) k1 = cand[f * SF_LPF + i];
        }
        if (k1 == INT_MAX) k1 = SF_BINS - 1;       // the last cumulative sum fell short of roll * s0 by rounding alone
        cent[t0 + f] = c;
        bw[t0 + f] = sqrt(b);
        rolloff[t0 + f] = (double)k1 * fstep;
    }

    // ---- the planes (frame-major: the live rows of `mag` are one contiguous range of both) and the workgroup's maximum ----------
    if (!mag_out && !db_out) return;               // uniform over the workgroup
    const int cnt = live * SF_BINS;
    const size_t o = (size_t)t0 * SF_BINS;
    float mx = 0.f;
    for (int i = t; i < cnt; i += SF_THREADS) {
        const float v = mag[i];
        if (mag_out) mag_out[o + i] = v;
        if (db_out) db_out[o + i] = v;
        mx = fmaxf(mx, v);
    }
    if (!db_out) return;
    __syncthreads();                               // the features' reads of `red` are done
    float *fred = (float *)red;
    fred[t] = mx;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < SF_THREADS; ++i) mx = fmaxf(mx, fred[i]);
        part_max[blockIdx.x] = mx;
    }
}

// running[0] = max(first ? 0 : running[0], part[0 .. count)); one workgroup
__global__ void __launch_bounds__(256) specfeat_max_kernel(const float *__restrict__ part, int count, int first, float *__restrict__ running) {
    __shared__ float fred[256];
    float mx = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) mx = fmaxf(mx, part[i]);
    fred[threadIdx.x] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 256; ++i) mx = fmaxf(mx, fred[i]);
        running[0] = first ? mx : fmaxf(running[0], mx);
    }
}

// amplitude_to_db(m, ref = max) in place, in float64: 10 log10(max(1e-10, m^2)) - 10 log10(max(1e-10, R^2)), then the 80 dB floor
// below the plane's maximum.  That maximum is attained where m == R and is exactly 0 (the same expression minus itself), so the
// floor is -80; R == 0 (an all-silent signal) gives 0 everywhere.
__global__ void __launch_bounds__(256) specfeat_db_kernel(float *__restrict__ db, int64_t count, const float *__restrict__ running) {
    const double R = (double)running[0];
    const double ref = 10.0 * log10(fmax(1e-10, R * R));
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) {
        const double m = (double)db[i];
        const double v = 10.0 * log10(fmax(1e-10, m * m)) - ref;
        db[i] = (float)fmax(v, -80.0);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int sf_check_n(const char *fn, int64_t n) {
    if (n < 1) return fail("%s: n = %lld must be at least 1", fn, (long long)n);
    if (n > SF_MAX_N) return fail("%s: n = %lld exceeds %lld samples", fn, (long long)n, (long long)SF_MAX_N);
    return 0;
}

static size_t sf_workspace(int64_t n) {
    const int64_t tiles = ceil_div(1 + n / SF_HOP, SF_TILE_FRAMES);
    return align_up((size_t)(SF_PART0 + (tiles < SF_GROUP_TILES ? tiles : SF_GROUP_TILES)) * sizeof(float), 256);
}

static bool sf_misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_spectral_features_workspace_bytes(int64_t n, size_t *bytes) {
    if (!bytes) return fail("rvc_spectral_features_workspace_bytes: null pointer");
    if (sf_check_n("rvc_spectral_features_workspace_bytes", n)) return 1;
    *bytes = sf_workspace(n);
    return 0;
}

extern "C" int rvc_spectral_features_f32(const float *x_dev, int64_t n, int sr, double roll_percent, float *mag_dev, float *db_dev,
                                         double *cent_dev, double *bw_dev, double *rolloff_dev, void *workspace_dev,
                                         size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_spectral_features_f32";
    if (!x_dev || !cent_dev || !bw_dev || !rolloff_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (sf_misaligned(x_dev, 4) || sf_misaligned(mag_dev, 4) || sf_misaligned(db_dev, 4) || sf_misaligned(workspace_dev, 4) ||
        sf_misaligned(cent_dev, 8) || sf_misaligned(bw_dev, 8) || sf_misaligned(rolloff_dev, 8))
        return fail("%s: misaligned pointer (signal, planes and workspace 4 bytes, curves 8)", fn);
    if (sf_check_n(fn, n)) return 1;
    if (sr < 1) return fail("%s: sr %d must be at least 1", fn, sr);
    if (!isfinite(roll_percent) || !(roll_percent > 0.0 && roll_percent < 1.0))
        return fail("%s: roll_percent %g must lie strictly between 0 and 1", fn, roll_percent);
    if (db_dev && db_dev == mag_dev) return fail("%s: db_dev must not alias mag_dev", fn);
    const size_t need = sf_workspace(n);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    hipStream_t stream = (hipStream_t)hip_stream;
    if (reserve_lds((const void *)specfeat_kernel, SF_LDS_BYTES, fn)) return 1;

    const int64_t frames = 1 + n / SF_HOP;
    const int64_t tiles = ceil_div(frames, SF_TILE_FRAMES);
    const double fstep = (double)sr / (double)SF_N;
    float *running = (float *)workspace_dev, *part = running + SF_PART0;
    for (int64_t tile0 = 0; tile0 < tiles; tile0 += SF_GROUP_TILES) {
        const int g = (int)(tiles - tile0 < SF_GROUP_TILES ? tiles - tile0 : SF_GROUP_TILES);
        hipLaunchKernelGGL(specfeat_kernel, dim3((unsigned)g), dim3(SF_THREADS), (size_t)SF_LDS_BYTES, stream, x_dev, n, frames, tile0, fstep,
                           roll_percent, mag_dev, db_dev, cent_dev, bw_dev, rolloff_dev, part);
        RVC_LAUNCH_CHECK();
        if (db_dev) {
            hipLaunchKernelGGL(specfeat_max_kernel, dim3(1), dim3(256), 0, stream, (const float *)part, g, (int)(tile0 == 0), running);
            RVC_LAUNCH_CHECK();
        }
    }
    if (db_dev) {
        const int64_t count = frames * SF_BINS;
        const int64_t blocks = ceil_div(count, 256);
        hipLaunchKernelGGL(specfeat_db_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, db_dev, count,
                           (const float *)running);
        RVC_LAUNCH_CHECK();
    }
    return 0;
}
