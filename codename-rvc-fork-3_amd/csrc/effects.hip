// K22: the effects board behind post_process (include/rvc_amd.h, "K22"): gain / distortion / bitcrush / clipping, delay, chorus,
// Freeverb and the compressor / limiter, mono fp32 [n] -> fp32 [n] on the caller's stream.  Five of the nine effects are feedback
// recurrences; how each one is cut into parallel work:
//
//   fx_pointwise_kernel    the four memoryless stages in the board's order, any subset in ONE pass (gain -> distortion and
//                          bitcrush -> clipping are neighbours in the chain; chorus sits between the two pairs).
//   fx_delay_kernel        d[m + D] = x[m] + fb d[m]: the samples of one residue class mod D form a chain, one LANE per residue
//                          walks it with d in a register.  No delay line exists in memory at all.
//   fx_allpass_kernel      Freeverb's allpass is the same shape (v[m] = in[m] + 0.5 v[m - M]): a lane per residue mod M, in place.
//   fx_comb_kernel         one workgroup per comb, walking the signal in chunks of the comb's length L.  Inside a chunk the comb's
//                          delayed input o[] is known (it was written a chunk ago), so the damping filter last = damp last + (1 -
//                          damp) o is a first-order LINEAR recurrence: each lane composes the affine map of its <= ceil(L / 256)
//                          samples, a 64-lane shuffle scan and a 4-wave carry compose the maps, a second walk emits.  Chunks follow
//                          one another inside the workgroup (two barriers per chunk).  The comb's line is its own output row v_c[]
//                          in the WORKSPACE (o[m] = v_c[m - L]); fx_comb_sum_kernel adds the eight rows in comb order.
//   fx_chorus_kernel       feedback 0 (the reference's default): a gather with the tap position evaluated per sample in float64.
//   fx_chorus_taps_kernel + fx_chorus_fb_kernel   feedback != 0: taps (int delay, fp32 fraction) for every sample in parallel,
//                          then ONE workgroup walks the signal in blocks of B = the shortest tap delay: every w[] of a block reads
//                          p[] of earlier blocks only.  p[] lives in the WORKSPACE, the block's w[] in LDS.  This is the slow path:
//                          n / B steps of two barriers each.
//   fx_peak / fx_env_probe / fx_env_resolve / fx_env_apply   the compressor's envelope follower is nonlinear but every step is a
//                          monotone map of the state, so a chunk whose end state comes out bit-identical from the entry states 0
//                          and peak|x| has an end state that does not depend on its entry ("closed").  probe: a lane per chunk runs
//                          both; resolve: a lane per run of unclosed chunks chains them from the closed chunk in front; apply: a
//                          lane per chunk runs from its now-exact entry state and writes gain x.  The result is the sequential
//                          recurrence's, bit for bit, whatever the chunk length.  No chunk closing = one lane walks the signal.
//
// Sequential dependence lives inside one workgroup (barriers) or between launches; no workgroup waits for another.  Nothing is
// accumulated atomically except the peak (a maximum: order-free), so two calls give identical bits.
#include <math.h>

#include "common.h"

namespace rvc {

constexpr int64_t FX_MAX_N = (int64_t)1 << 27;
constexpr int FX_SR_MIN = 8000, FX_SR_MAX = 96000;
constexpr int FX_THREADS = 256;
constexpr int FX_CHAIN_THREADS = 64;           // lane-per-residue kernels: small workgroups spread the chains over the CUs
constexpr double FX_DB_MAX = 200.0;            // |dB| accepted for a gain, drive or threshold
constexpr double FX_CHORUS_MAX_MS = 100.0;     // the longest chorus tap: 9600 samples at 96 kHz
constexpr int FX_CHORUS_MAX_BLOCK = 9600;
constexpr int64_t FX_ENV_MIN_CHUNK = 256;      // the shortest chunk the library chooses by itself
constexpr int FX_COMB_T[8] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};
constexpr int FX_ALLPASS_T[4] = {556, 441, 341, 225};

enum { FX_GAIN = 1, FX_DISTORTION = 2, FX_BITCRUSH = 4, FX_CLIPPING = 8 };

struct CombLens {
    int len[8];
};

static unsigned flat_grid(int64_t n, int threads) {
    const int64_t blocks = ceil_div(n, threads);
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}

// ---- pointwise ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FX_THREADS) void fx_pointwise_kernel(const float *x, int64_t n, int stages, float gain, float drive,
                                                                   float scale, float clip, float *out) {
    for (int64_t i = blockIdx.x * (int64_t)FX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FX_THREADS) {
        float v = x[i];
        if (stages & FX_GAIN) v *= gain;
        if (stages & FX_DISTORTION) v = tanhf(v * drive);
        if (stages & FX_BITCRUSH) v = rintf(v * scale) / scale;
        if (stages & FX_CLIPPING) v = fminf(fmaxf(v, -clip), clip);
        out[i] = v;
    }
}

// ---- delay -------------------------------------------------------------------------------------------------------------------------
// lane r < min(D, n) owns the samples r, r + D, r + 2 D, ... < n
__global__ __launch_bounds__(FX_CHAIN_THREADS) void fx_delay_kernel(const float *__restrict__ x, int64_t n, int64_t D, float fb,
                                                                     float dry, float mix, float *__restrict__ out) {
    const int64_t r = blockIdx.x * (int64_t)FX_CHAIN_THREADS + threadIdx.x;
    if (r >= D || r >= n) return;
    float d = 0.f;
#pragma unroll 4
    for (int64_t m = r; m < n; m += D) {
        const float xv = x[m];
        out[m] = fmaf(mix, d, dry * xv);
        d = fmaf(fb, d, xv);
    }
}

// ---- reverb ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FX_THREADS) void fx_comb_kernel(const float *__restrict__ x, int64_t n, CombLens lens, float in_gain,
                                                              float damp, float damp1, float feedback, float *v_all) {
    const int L = lens.len[blockIdx.x];
    float *v = v_all + (int64_t)blockIdx.x * n;          // this comb's row: v[m] is what the comb stores into its line at time m
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (L + FX_THREADS - 1) / FX_THREADS;    // samples of a chunk per lane, contiguous
    __shared__ float wave_a[FX_THREADS / 64], wave_b[FX_THREADS / 64];
    __shared__ float carry;
    float last = 0.f;                                     // the filter state entering the chunk, the same in every lane
    for (int64_t s = 0; s < n; s += L) {
        const int len = (int)(n - s < L ? n - s : L);
        const int j0 = t * per < len ? t * per : len, j1 = j0 + per < len ? j0 + per : len;
        const float *o = v + s - L;                       // o[j] = v[s + j - L]: read only when s > 0, written one chunk ago
        // the affine map state -> a state + b of this lane's samples
        float a = 1.f, b = 0.f;
        for (int j = j0; j < j1; ++j) {
            b = fmaf(damp, b, (s ? o[j] : 0.f) * damp1);
            a *= damp;
        }
        // inclusive scan over the wave: (pa, pb) then (a, b) = (pa a, a pb + b)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float pa = __shfl_up(a, d, 64), pb = __shfl_up(b, d, 64);
            if (lane >= d) {
                b = fmaf(a, pb, b);
                a *= pa;
            }
        }
        if (lane == 63) {
            wave_a[wave] = a;
            wave_b[wave] = b;
        }
        const float xa = __shfl_up(a, 1, 64), xb = __shfl_up(b, 1, 64);   // the lanes in front of this one, within the wave
        __syncthreads();
        float st = last;
        for (int w = 0; w < wave; ++w) st = fmaf(wave_a[w], st, wave_b[w]);
        if (lane > 0) st = fmaf(xa, st, xb);
        for (int j = j0; j < j1; ++j) {
            st = fmaf(damp, st, (s ? o[j] : 0.f) * damp1);
            v[s + j] = fmaf(st, feedback, in_gain * x[s + j]);
        }
        if (t == FX_THREADS - 1) carry = st;              // lanes without samples hold the identity map: st is the chunk's end state
        __syncthreads();                                  // ... and orders this chunk's stores to v before the next chunk's loads
        last = carry;
    }
}

// sum[i] = sum over the combs, in comb order, of the comb's output o_c[i] = v_c[i - L_c] (0 before the line has filled)
__global__ __launch_bounds__(FX_THREADS) void fx_comb_sum_kernel(const float *__restrict__ v_all, int64_t n, CombLens lens,
                                                                  float *__restrict__ sum) {
    for (int64_t i = blockIdx.x * (int64_t)FX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FX_THREADS) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (i >= lens.len[c]) s += v_all[(int64_t)c * n + i - lens.len[c]];
        sum[i] = s;
    }
}

// lane r < min(M, n) owns r, r + M, ...: b = line, line = in + 0.5 b, out = b - in.  In place on buf; the last allpass of the
// chain writes y = out wet1 + x dry to `out` instead.
template <bool LAST>
__global__ __launch_bounds__(FX_CHAIN_THREADS) void fx_allpass_kernel(float *buf, int64_t n, int M, const float *__restrict__ x,
                                                                       float wet1, float dry, float *__restrict__ out) {
    const int64_t r = blockIdx.x * (int64_t)FX_CHAIN_THREADS + threadIdx.x;
    if (r >= M || r >= n) return;
    float line = 0.f;
#pragma unroll 4
    for (int64_t m = r; m < n; m += M) {
        const float in = buf[m], b = line;
        line = fmaf(0.5f, b, in);
        const float o = b - in;
        if (LAST)
            out[m] = fmaf(o, wet1, x[m] * dry);
        else
            buf[m] = o;
    }
}

// ---- chorus ------------------------------------------------------------------------------------------------------------------------
struct ChorusLfo {
    double rate, sr, centre, depth10;
};

// the tap of sample i: delay = di + fr samples, float64 throughout (include/rvc_amd.h spells the expressions out)
__device__ __forceinline__ void chorus_tap(const ChorusLfo &p, int64_t i, int &di, float &fr) {
    double ph = p.rate * (double)i / p.sr;
    ph -= floor(ph);
    const double lfo = sin(6.283185307179586 * ph);
    const double ms = fmax(1.0, p.centre + p.depth10 * lfo);
    const double dl = ms * p.sr / 1000.0;
    const double fl = floor(dl);
    di = (int)fl;
    fr = (float)(dl - fl);
}

__global__ __launch_bounds__(FX_THREADS) void fx_chorus_kernel(const float *__restrict__ x, int64_t n, ChorusLfo p, float dry, float mix,
                                                                float *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)FX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FX_THREADS) {
        int di;
        float fr;
        chorus_tap(p, i, di, fr);
        const int64_t m = i - di;
        const float p0 = m >= 0 ? x[m] : 0.f, p1 = m >= 1 ? x[m - 1] : 0.f;
        const float w = fmaf(fr, p1 - p0, p0);
        out[i] = fmaf(mix, w, dry * x[i]);
    }
}

__global__ __launch_bounds__(FX_THREADS) void fx_chorus_taps_kernel(int64_t n, ChorusLfo p, int *__restrict__ di, float *__restrict__ fr) {
    for (int64_t i = blockIdx.x * (int64_t)FX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FX_THREADS)
        chorus_tap(p, i, di[i], fr[i]);
}

// one workgroup; block <= every di[] (the host derives it from centre - 10 depth), so the w[] of [s, s + block) read p[< s] only
__global__ __launch_bounds__(FX_THREADS) void fx_chorus_fb_kernel(const float *__restrict__ x, int64_t n, const int *__restrict__ di,
                                                                   const float *__restrict__ fr, int block, float fb, float dry,
                                                                   float mix, float *p, float *__restrict__ out) {
    __shared__ float wbuf[FX_CHORUS_MAX_BLOCK + 1];       // wbuf[j] = w[s + j - 1]
    if (threadIdx.x == 0) wbuf[0] = 0.f;
    for (int64_t s = 0; s < n; s += block) {
        const int len = (int)(n - s < block ? n - s : block);
        for (int j = threadIdx.x; j < len; j += FX_THREADS) {
            const int64_t i = s + j, m = i - di[i];
            const float p0 = m >= 0 ? p[m] : 0.f, p1 = m >= 1 ? p[m - 1] : 0.f;
            const float w = fmaf(fr[i], p1 - p0, p0);
            wbuf[j + 1] = w;
            out[i] = fmaf(mix, w, dry * x[i]);
        }
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += FX_THREADS) p[s + j] = fmaf(-fb, wbuf[j], x[s + j]);
        const float w_end = wbuf[len];
        __syncthreads();                                  // orders the stores to p before the next block's loads, too
        if (threadIdx.x == 0) wbuf[0] = w_end;
    }
}

// ---- compressor --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float env_step(float e, float a, float c_attack, float c_release) {
    return fmaf(a > e ? c_attack : c_release, e - a, a);
}

// f(|x[j]|, j) for j in [0, len), in order; the loads of eight steps are issued together, the steps themselves are a chain
template <class F>
__device__ __forceinline__ void env_walk(const float *__restrict__ x, int64_t len, F f) {
    int64_t j = 0;
    for (; j + 8 <= len; j += 8) {
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = x[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) f(fabsf(a[u]), a[u], j + u);
    }
    for (; j < len; ++j) f(fabsf(x[j]), x[j], j);
}

__global__ __launch_bounds__(FX_THREADS) void fx_peak_kernel(const float *__restrict__ x, int64_t n, unsigned *peak_bits) {
    float m = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)FX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FX_THREADS)
        m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(peak_bits, __float_as_uint(m));   // non-negative floats order as their bit patterns
}

struct EnvState {      // the workspace of one compressor pass
    unsigned *peak_bits;
    float *end;        // [chunks] the chunk's end state, exact when closed
    float *entry;      // [chunks] the state entering the chunk
    int *closed;       // [chunks]
};

__global__ __launch_bounds__(FX_CHAIN_THREADS) void fx_env_probe_kernel(const float *__restrict__ x, int64_t n, int64_t chunk,
                                                                         int64_t chunks, float c_attack, float c_release, EnvState st) {
    const int64_t k = blockIdx.x * (int64_t)FX_CHAIN_THREADS + threadIdx.x;
    if (k >= chunks) return;
    const int64_t first = k * chunk, len = n - first < chunk ? n - first : chunk;
    float lo = 0.f, hi = __uint_as_float(*st.peak_bits);
    env_walk(x + first, len, [&](float a, float, int64_t) {
        lo = env_step(lo, a, c_attack, c_release);
        hi = env_step(hi, a, c_attack, c_release);
    });
    st.end[k] = hi;
    st.closed[k] = __float_as_uint(lo) == __float_as_uint(hi);
}

// a lane per chunk; the lane of a chunk that FOLLOWS a closed one (or is the first) walks forward through the unclosed chunks
__global__ __launch_bounds__(FX_CHAIN_THREADS) void fx_env_resolve_kernel(const float *__restrict__ x, int64_t n, int64_t chunk,
                                                                           int64_t chunks, float c_attack, float c_release, EnvState st) {
    int64_t k = blockIdx.x * (int64_t)FX_CHAIN_THREADS + threadIdx.x;
    if (k >= chunks || (k > 0 && !st.closed[k - 1])) return;
    float e = k > 0 ? st.end[k - 1] : 0.f;
    st.entry[k] = e;
    for (; k + 1 < chunks && !st.closed[k]; ++k) {
        env_walk(x + k * chunk, chunk, [&](float a, float, int64_t) { e = env_step(e, a, c_attack, c_release); });
        st.entry[k + 1] = e;
    }
}

__global__ __launch_bounds__(FX_CHAIN_THREADS) void fx_env_apply_kernel(const float *__restrict__ x, int64_t n, int64_t chunk,
                                                                         int64_t chunks, float c_attack, float c_release, float thr,
                                                                         float expo, int limiter, float post, EnvState st,
                                                                         float *__restrict__ out) {
    const int64_t k = blockIdx.x * (int64_t)FX_CHAIN_THREADS + threadIdx.x;
    if (k >= chunks) return;
    const int64_t first = k * chunk, len = n - first < chunk ? n - first : chunk;
    float e = st.entry[k];
    float *o = out + first;
    env_walk(x + first, len, [&](float a, float xv, int64_t j) {
        e = env_step(e, a, c_attack, c_release);
        float y = (e < thr ? 1.f : powf(e / thr, expo)) * xv;
        if (limiter) y = fminf(fmaxf(y * post, -1.f), 1.f);
        o[j] = y;
    });
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
    const char *p = (const char *)a, *q = (const char *)b;
    return a_bytes > 0 && b_bytes > 0 && p < q + b_bytes && q < p + a_bytes;
}

static bool within(double v, double lo, double hi) { return lo <= v && v <= hi; }   // false for NaN

static double db_to_gain(double db) { return pow(10.0, db / 20.0); }

static int check_signal(const char *fn, int64_t n, int sr) {
    if (n < 0) return fail("%s: n %lld is negative", fn, (long long)n);
    if (n > FX_MAX_N) return fail("%s: n %lld exceeds 2^27 samples", fn, (long long)n);
    if (sr < FX_SR_MIN || sr > FX_SR_MAX) return fail("%s: sr %d is outside [%d, %d]", fn, sr, FX_SR_MIN, FX_SR_MAX);
    return 0;
}

static CombLens comb_lengths(int sr) {
    CombLens l;
    for (int c = 0; c < 8; ++c) l.len[c] = (int)((int64_t)sr * FX_COMB_T[c] / 44100);
    return l;
}

static double ballistics(int sr, double t_ms) { return t_ms <= 1e-3 ? 0.0 : exp(-2.0 * M_PI * 1000.0 / ((double)sr * t_ms)); }

static int check_ballistics(const char *fn, double attack_ms, double release_ms) {
    if (!within(attack_ms, 0.0, 1e6)) return fail("%s: attack_ms %g is outside [0, 1e6]", fn, attack_ms);
    if (!within(release_ms, 0.0, 1e6)) return fail("%s: release_ms %g is outside [0, 1e6]", fn, release_ms);
    return 0;
}

// the chunk length of one envelope pass: the caller's, or long enough for the slower coefficient to shrink the distance between
// the two probes by 2^-40
static int64_t env_chunk(int64_t n, int64_t chunk, double c_attack, double c_release) {
    if (chunk == 0) {
        const double c = c_attack > c_release ? c_attack : c_release;
        const double want = c <= 0.0 ? 0.0 : (c >= 1.0 ? (double)n : ceil(28.0 / -log(c)));
        chunk = want >= (double)n ? n : (int64_t)want;
        if (chunk < FX_ENV_MIN_CHUNK) chunk = FX_ENV_MIN_CHUNK;
    }
    return chunk < n ? chunk : n;
}

static int64_t env_max_chunks(int64_t n, int64_t chunk) {
    const int64_t c = chunk == 0 ? FX_ENV_MIN_CHUNK : chunk;
    return n == 0 ? 0 : ceil_div(n, c < n ? c : n);
}

static size_t env_state_bytes(int64_t n, int64_t chunk) { return align_up(16 + 12 * (size_t)env_max_chunks(n, chunk), 16); }

// one compressor over x -> out with the state in `ws` (env_state_bytes); the arguments have been checked
static int env_pass(const float *x, int64_t n, int sr, double threshold_db, double ratio, double attack_ms, double release_ms,
                    int64_t chunk, int limiter, double post, float *out, void *ws, hipStream_t stream) {
    const double ca = ballistics(sr, attack_ms), cr = ballistics(sr, release_ms);
    chunk = env_chunk(n, chunk, ca, cr);
    const int64_t chunks = ceil_div(n, chunk), cap = env_max_chunks(n, chunk);
    EnvState st;
    st.peak_bits = (unsigned *)ws;
    st.end = (float *)((char *)ws + 16);
    st.entry = st.end + cap;
    st.closed = (int *)(st.entry + cap);
    RVC_HIP(hipMemsetAsync(st.peak_bits, 0, 16, stream));
    hipLaunchKernelGGL(fx_peak_kernel, dim3(flat_grid(n, FX_THREADS)), dim3(FX_THREADS), 0, stream, x, n, st.peak_bits);
    RVC_LAUNCH_CHECK();
    const dim3 grid((unsigned)ceil_div(chunks, FX_CHAIN_THREADS)), block(FX_CHAIN_THREADS);
    hipLaunchKernelGGL(fx_env_probe_kernel, grid, block, 0, stream, x, n, chunk, chunks, (float)ca, (float)cr, st);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fx_env_resolve_kernel, grid, block, 0, stream, x, n, chunk, chunks, (float)ca, (float)cr, st);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fx_env_apply_kernel, grid, block, 0, stream, x, n, chunk, chunks, (float)ca, (float)cr,
                       (float)db_to_gain(threshold_db), (float)(1.0 / ratio - 1.0), limiter, (float)post, st, out);
    RVC_LAUNCH_CHECK();
    return 0;
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_fx_pointwise_f32(const float *x_dev, int64_t n, int stages, double gain_db, double drive_db, double bit_depth,
                                    double clip_threshold_db, float *out_dev, void *hip_stream) {
    const char *fn = "rvc_fx_pointwise_f32";
    if (!x_dev || !out_dev) return fail("%s: null pointer", fn);
    if (n < 0) return fail("%s: n %lld is negative", fn, (long long)n);
    if (n > FX_MAX_N) return fail("%s: n %lld exceeds 2^27 samples", fn, (long long)n);
    if (stages < 1 || stages > 15) return fail("%s: stages %d is not a set of gain 1 | distortion 2 | bitcrush 4 | clipping 8", fn, stages);
    if ((stages & FX_GAIN) && !within(gain_db, -FX_DB_MAX, FX_DB_MAX)) return fail("%s: gain_db %g is outside [-200, 200]", fn, gain_db);
    if ((stages & FX_DISTORTION) && !within(drive_db, -FX_DB_MAX, FX_DB_MAX)) return fail("%s: drive_db %g is outside [-200, 200]", fn, drive_db);
    if ((stages & FX_BITCRUSH) && !(bit_depth > 0.0 && bit_depth <= 32.0)) return fail("%s: bit_depth %g is outside (0, 32]", fn, bit_depth);
    if ((stages & FX_CLIPPING) && !within(clip_threshold_db, -FX_DB_MAX, FX_DB_MAX))
        return fail("%s: clip_threshold_db %g is outside [-200, 200]", fn, clip_threshold_db);
    if (out_dev != x_dev && overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev partly overlaps x_dev", fn);
    if (n == 0) return 0;
    hipLaunchKernelGGL(fx_pointwise_kernel, dim3(flat_grid(n, FX_THREADS)), dim3(FX_THREADS), 0, (hipStream_t)hip_stream, x_dev, n, stages,
                       (float)db_to_gain(gain_db), (float)db_to_gain(drive_db), (float)exp2(bit_depth), (float)db_to_gain(clip_threshold_db),
                       out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_fx_delay_f32(const float *x_dev, int64_t n, int sr, double delay_seconds, double feedback, double mix, float *out_dev,
                                void *hip_stream) {
    const char *fn = "rvc_fx_delay_f32";
    if (!x_dev || !out_dev) return fail("%s: null pointer", fn);
    if (check_signal(fn, n, sr)) return 1;
    if (!within(delay_seconds, 0.0, 60.0)) return fail("%s: delay_seconds %g is outside [0, 60]", fn, delay_seconds);
    const int64_t D = (int64_t)floor(delay_seconds * sr);
    if (D < 1) return fail("%s: delay_seconds %g is less than one sample at sr %d", fn, delay_seconds, sr);
    if (!within(feedback, -1.0, 1.0)) return fail("%s: feedback %g is outside [-1, 1]", fn, feedback);
    if (!within(mix, 0.0, 1.0)) return fail("%s: mix %g is outside [0, 1]", fn, mix);
    if (overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev must not alias x_dev", fn);
    if (n == 0) return 0;
    const int64_t lanes = D < n ? D : n;
    hipLaunchKernelGGL(fx_delay_kernel, dim3((unsigned)ceil_div(lanes, FX_CHAIN_THREADS)), dim3(FX_CHAIN_THREADS), 0, (hipStream_t)hip_stream,
                       x_dev, n, D, (float)feedback, (float)(1.0 - mix), (float)mix, out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

static int chorus_check(const char *fn, double rate_hz, double depth, double centre_delay_ms, double feedback, double mix) {
    if (!within(rate_hz, 0.0, 100.0)) return fail("%s: rate_hz %g is outside [0, 100]", fn, rate_hz);
    if (!within(depth, 0.0, 10.0)) return fail("%s: depth %g is outside [0, 10]", fn, depth);
    if (!within(centre_delay_ms, 0.0, FX_CHORUS_MAX_MS) || !(centre_delay_ms + 10.0 * depth <= FX_CHORUS_MAX_MS))
        return fail("%s: centre_delay_ms %g (+ 10 depth = %g) is outside [0, 100]", fn, centre_delay_ms, centre_delay_ms + 10.0 * depth);
    if (!within(feedback, -1.0, 1.0)) return fail("%s: feedback %g is outside [-1, 1]", fn, feedback);
    if (!within(mix, 0.0, 1.0)) return fail("%s: mix %g is outside [0, 1]", fn, mix);
    return 0;
}

extern "C" int rvc_fx_chorus_workspace_bytes(int64_t n, double feedback, size_t *bytes) {
    const char *fn = "rvc_fx_chorus_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (n < 0) return fail("%s: n %lld is negative", fn, (long long)n);
    if (n > FX_MAX_N) return fail("%s: n %lld exceeds 2^27 samples", fn, (long long)n);
    if (!within(feedback, -1.0, 1.0)) return fail("%s: feedback %g is outside [-1, 1]", fn, feedback);
    *bytes = feedback == 0.0 ? 0 : 12 * (size_t)n;        // p, the integer delays, the fractions
    return 0;
}

extern "C" int rvc_fx_chorus_f32(const float *x_dev, int64_t n, int sr, double rate_hz, double depth, double centre_delay_ms,
                                 double feedback, double mix, float *out_dev, void *workspace_dev, size_t workspace_bytes,
                                 void *hip_stream) {
    const char *fn = "rvc_fx_chorus_f32";
    if (!x_dev || !out_dev) return fail("%s: null pointer", fn);
    if (check_signal(fn, n, sr)) return 1;
    if (chorus_check(fn, rate_hz, depth, centre_delay_ms, feedback, mix)) return 1;
    const size_t need = feedback == 0.0 ? 0 : 12 * (size_t)n;
    if (need && !workspace_dev) return fail("%s: null pointer", fn);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev must not alias x_dev", fn);
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    const ChorusLfo lfo = {rate_hz, (double)sr, centre_delay_ms, 10.0 * depth};
    const float dry = (float)(1.0 - mix);
    if (feedback == 0.0) {
        hipLaunchKernelGGL(fx_chorus_kernel, dim3(flat_grid(n, FX_THREADS)), dim3(FX_THREADS), 0, stream, x_dev, n, lfo, dry, (float)mix, out_dev);
        RVC_LAUNCH_CHECK();
        return 0;
    }
    float *p = (float *)workspace_dev;
    int *di = (int *)(p + n);
    float *fr = (float *)(di + n);
    hipLaunchKernelGGL(fx_chorus_taps_kernel, dim3(flat_grid(n, FX_THREADS)), dim3(FX_THREADS), 0, stream, n, lfo, di, fr);
    RVC_LAUNCH_CHECK();
    // every tap is at least max(1, centre - 10 depth) ms long: lfo >= -1 and each rounding in chorus_tap is monotone
    const double shortest_ms = fmax(1.0, centre_delay_ms - 10.0 * depth);
    int block = (int)floor(shortest_ms * sr / 1000.0);
    if (block > FX_CHORUS_MAX_BLOCK) block = FX_CHORUS_MAX_BLOCK;
    hipLaunchKernelGGL(fx_chorus_fb_kernel, dim3(1), dim3(FX_THREADS), 0, stream, x_dev, n, di, fr, block, (float)feedback, dry, (float)mix, p,
                       out_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_fx_reverb_params(int sr, int *comb_len, int *allpass_len) {
    const char *fn = "rvc_fx_reverb_params";
    if (!comb_len || !allpass_len) return fail("%s: null pointer", fn);
    if (check_signal(fn, 0, sr)) return 1;
    const CombLens l = comb_lengths(sr);
    for (int c = 0; c < 8; ++c) comb_len[c] = l.len[c];
    for (int a = 0; a < 4; ++a) allpass_len[a] = (int)((int64_t)sr * FX_ALLPASS_T[a] / 44100);
    return 0;
}

extern "C" int rvc_fx_reverb_workspace_bytes(int64_t n, size_t *bytes) {
    const char *fn = "rvc_fx_reverb_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (n < 0) return fail("%s: n %lld is negative", fn, (long long)n);
    if (n > FX_MAX_N) return fail("%s: n %lld exceeds 2^27 samples", fn, (long long)n);
    *bytes = 36 * (size_t)n;                               // the eight comb rows and their sum
    return 0;
}

extern "C" int rvc_fx_reverb_f32(const float *x_dev, int64_t n, int sr, double room_size, double damping, double wet_level, double dry_level,
                                 double width, double freeze_mode, float *out_dev, void *workspace_dev, size_t workspace_bytes,
                                 void *hip_stream) {
    const char *fn = "rvc_fx_reverb_f32";
    if (!x_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (check_signal(fn, n, sr)) return 1;
    if (!within(room_size, 0.0, 1.0)) return fail("%s: room_size %g is outside [0, 1]", fn, room_size);
    if (!within(damping, 0.0, 1.0)) return fail("%s: damping %g is outside [0, 1]", fn, damping);
    if (!within(wet_level, 0.0, 1.0)) return fail("%s: wet_level %g is outside [0, 1]", fn, wet_level);
    if (!within(dry_level, 0.0, 1.0)) return fail("%s: dry_level %g is outside [0, 1]", fn, dry_level);
    if (!within(width, 0.0, 1.0)) return fail("%s: width %g is outside [0, 1]", fn, width);
    if (!within(freeze_mode, 0.0, 1.0)) return fail("%s: freeze_mode %g is outside [0, 1]", fn, freeze_mode);
    const size_t need = 36 * (size_t)n;
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev must not alias x_dev", fn);
    if (overlap(workspace_dev, (int64_t)need, x_dev, n * 4) || overlap(workspace_dev, (int64_t)need, out_dev, n * 4))
        return fail("%s: workspace_dev must not alias x_dev or out_dev", fn);
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    const bool frozen = freeze_mode >= 0.5;
    const double damp = frozen ? 0.0 : 0.4 * damping, feedback = frozen ? 1.0 : 0.28 * room_size + 0.7;
    const double wet1 = 1.5 * wet_level * (1.0 + width), dry = 2.0 * dry_level;
    const CombLens lens = comb_lengths(sr);
    float *rows = (float *)workspace_dev, *sum = rows + 8 * n;
    hipLaunchKernelGGL(fx_comb_kernel, dim3(8), dim3(FX_THREADS), 0, stream, x_dev, n, lens, frozen ? 0.f : 0.015f, (float)damp,
                       (float)(1.0 - damp), (float)feedback, rows);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(fx_comb_sum_kernel, dim3(flat_grid(n, FX_THREADS)), dim3(FX_THREADS), 0, stream, rows, n, lens, sum);
    RVC_LAUNCH_CHECK();
    for (int a = 0; a < 4; ++a) {
        const int M = (int)((int64_t)sr * FX_ALLPASS_T[a] / 44100);
        const int64_t lanes = M < n ? M : n;
        const dim3 grid((unsigned)ceil_div(lanes, FX_CHAIN_THREADS)), block(FX_CHAIN_THREADS);
        if (a < 3)
            hipLaunchKernelGGL(fx_allpass_kernel<false>, grid, block, 0, stream, sum, n, M, x_dev, (float)wet1, (float)dry, out_dev);
        else
            hipLaunchKernelGGL(fx_allpass_kernel<true>, grid, block, 0, stream, sum, n, M, x_dev, (float)wet1, (float)dry, out_dev);
        RVC_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int rvc_fx_ballistics(int sr, double attack_ms, double release_ms, double *c_attack, double *c_release) {
    const char *fn = "rvc_fx_ballistics";
    if (!c_attack || !c_release) return fail("%s: null pointer", fn);
    if (check_signal(fn, 0, sr) || check_ballistics(fn, attack_ms, release_ms)) return 1;
    *c_attack = ballistics(sr, attack_ms);
    *c_release = ballistics(sr, release_ms);
    return 0;
}

extern "C" int rvc_fx_compressor_workspace_bytes(int64_t n, int64_t chunk, int limiter, size_t *bytes) {
    const char *fn = "rvc_fx_compressor_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (n < 0) return fail("%s: n %lld is negative", fn, (long long)n);
    if (n > FX_MAX_N) return fail("%s: n %lld exceeds 2^27 samples", fn, (long long)n);
    if (chunk < 0) return fail("%s: chunk %lld is negative", fn, (long long)chunk);
    if (limiter != 0 && limiter != 1) return fail("%s: limiter %d is neither 0 nor 1", fn, limiter);
    *bytes = n == 0 ? 0 : env_state_bytes(n, chunk) + (limiter ? 4 * (size_t)n : 0);   // the limiter's first compressor writes n floats
    return 0;
}

extern "C" int rvc_fx_compressor_f32(const float *x_dev, int64_t n, int sr, double threshold_db, double ratio, double attack_ms,
                                     double release_ms, int64_t chunk, float *out_dev, void *workspace_dev, size_t workspace_bytes,
                                     void *hip_stream) {
    const char *fn = "rvc_fx_compressor_f32";
    if (!x_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (check_signal(fn, n, sr)) return 1;
    if (!within(threshold_db, -FX_DB_MAX, FX_DB_MAX)) return fail("%s: threshold_db %g is outside [-200, 200]", fn, threshold_db);
    if (!within(ratio, 1.0, 1e6)) return fail("%s: ratio %g is outside [1, 1e6]", fn, ratio);
    if (check_ballistics(fn, attack_ms, release_ms)) return 1;
    if (chunk < 0) return fail("%s: chunk %lld is negative", fn, (long long)chunk);
    const size_t need = n == 0 ? 0 : env_state_bytes(n, chunk);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev must not alias x_dev", fn);
    if (overlap(workspace_dev, (int64_t)need, x_dev, n * 4) || overlap(workspace_dev, (int64_t)need, out_dev, n * 4))
        return fail("%s: workspace_dev must not alias x_dev or out_dev", fn);
    if (n == 0) return 0;
    return env_pass(x_dev, n, sr, threshold_db, ratio, attack_ms, release_ms, chunk, 0, 1.0, out_dev, workspace_dev, (hipStream_t)hip_stream);
}

extern "C" int rvc_fx_limiter_f32(const float *x_dev, int64_t n, int sr, double threshold_db, double release_ms, int64_t chunk,
                                  float *out_dev, void *workspace_dev, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_fx_limiter_f32";
    if (!x_dev || !out_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (check_signal(fn, n, sr)) return 1;
    if (!within(threshold_db, -FX_DB_MAX, FX_DB_MAX)) return fail("%s: threshold_db %g is outside [-200, 200]", fn, threshold_db);
    if (check_ballistics(fn, 0.0, release_ms)) return 1;
    if (chunk < 0) return fail("%s: chunk %lld is negative", fn, (long long)chunk);
    const size_t state = n == 0 ? 0 : env_state_bytes(n, chunk), need = state + (n == 0 ? 0 : 4 * (size_t)n);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (overlap(out_dev, n * 4, x_dev, n * 4)) return fail("%s: out_dev must not alias x_dev", fn);
    if (overlap(workspace_dev, (int64_t)need, x_dev, n * 4) || overlap(workspace_dev, (int64_t)need, out_dev, n * 4))
        return fail("%s: workspace_dev must not alias x_dev or out_dev", fn);
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)hip_stream;
    float *mid = (float *)((char *)workspace_dev + state);
    if (env_pass(x_dev, n, sr, -10.0, 4.0, 2.0, 200.0, chunk, 0, 1.0, mid, workspace_dev, stream)) return 1;
    const double post = pow(10.0, 7.5 / 40.0) * pow(10.0, -threshold_db / 20.0);
    return env_pass(mid, n, sr, threshold_db, 1000.0, 0.001, release_ms, chunk, 1, post, out_dev, workspace_dev, stream);
}
