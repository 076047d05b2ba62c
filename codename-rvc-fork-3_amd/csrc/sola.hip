// K21: the seam of block-by-block conversion (include/rvc_amd.h, "K21").  rvc_stream_window_f32 builds the window the pipeline
// converts and rolls the carried input history; rvc_sola_f32 slides the new vocoder output against the tail saved from the previous
// one to the lag of best normalised correlation, crossfades, and saves the next tail.  Three launches per push for both calls:
//
//   stream_window_kernel   one workgroup: window = [hist | block], barrier, hist <- the window's last n_hist samples.  hist is read
//                          and written by the same call, so the two phases must be ordered; a window is a second or two of 16 kHz
//                          audio (25 k samples), which one workgroup of 1024 lanes copies in ~25 steps.
//   sola_score_kernel      one workgroup per lag: nom and the energy of infer[o .. o + X) in fp32, lane-strided partial sums ->
//                          the 64-lane shuffle tree -> the four waves' sums added in wave order by lane 0.  A fixed order: two
//                          calls give identical bits.
//   sola_emit_kernel       every workgroup repeats the arg-max over the S + 1 scores (a few KB out of L2; lowest lag on a tie),
//                          then emits its 2048 output samples.  Lane i < X reads buf[i] for the crossfade and only THEN
//                          overwrites it with the next tail: the in/out buffer needs no second copy.
//
// The work is (S + 1) X multiply-adds (5.8 M at 48 kHz with 50 ms / 50 ms): no LDS tiling, no matrix cores.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace rvc {

constexpr int SOLA_THREADS = 256;
constexpr int SOLA_EMIT_PER_BLOCK = 2048;          // output samples per workgroup of sola_emit_kernel
constexpr int64_t SOLA_MAX_SAMPLES = (int64_t)1 << 24;
constexpr int WINDOW_THREADS = 1024;

// sum over the 64 lanes of a wave, valid in lane 0; the tree's shape is fixed
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(WINDOW_THREADS) void stream_window_kernel(float *hist, int64_t n_hist, const float *block,
                                                                        int64_t n_block, float *window) {
    const int64_t n = n_hist + n_block;
    for (int64_t j = threadIdx.x; j < n; j += WINDOW_THREADS) window[j] = j < n_hist ? hist[j] : block[j - n_hist];
    __syncthreads();   // orders the global stores above, too: every lane of this (only) workgroup sees the whole window
    for (int64_t i = threadIdx.x; i < n_hist; i += WINDOW_THREADS) hist[i] = window[n_block + i];
}

__global__ __launch_bounds__(SOLA_THREADS) void sola_score_kernel(const float *__restrict__ infer, const float *__restrict__ buf,
                                                                   int xfade, float *__restrict__ score) {
    const int o = blockIdx.x;          // the grid is S + 1 wide: o + i <= S + X - 1 < n_infer
    float nom = 0.f, energy = 0.f;
    for (int i = threadIdx.x; i < xfade; i += SOLA_THREADS) {
        const float v = infer[o + i];
        nom += v * buf[i];
        energy += v * v;
    }
    nom = wave_sum(nom);
    energy = wave_sum(energy);
    __shared__ float part[2][SOLA_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = nom;
        part[1][threadIdx.x >> 6] = energy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        nom = part[0][0];
        energy = part[1][0];
        for (int w = 1; w < SOLA_THREADS / 64; ++w) {
            nom += part[0][w];
            energy += part[1][w];
        }
        score[o] = nom / sqrtf(energy + 1e-8f);
    }
}

// (value, lag) pairs: `b` replaces `a` only when it scores strictly higher, or equally at a lower lag.  A lane without a score holds
// (-inf, INT_MAX) and never wins; a NaN score never wins either, so the result is always a lag that exists.
__device__ __forceinline__ void take_better(float &av, int &ai, float bv, int bi) {
    if (bv > av || (bv == av && bi < ai)) {
        av = bv;
        ai = bi;
    }
}

__global__ __launch_bounds__(SOLA_THREADS) void sola_emit_kernel(const float *__restrict__ infer, float *__restrict__ buf,
                                                                  const float *__restrict__ fade_in, const float *__restrict__ score,
                                                                  int xfade, int search, int block, float *__restrict__ out,
                                                                  int *__restrict__ offset_out) {
    const int t = threadIdx.x;
    float best = t <= search ? score[t] : -INFINITY;
    int lag = t <= search ? t : INT_MAX;
    for (int o = t + SOLA_THREADS; o <= search; o += SOLA_THREADS) take_better(best, lag, score[o], o);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) take_better(best, lag, __shfl_down(best, d, 64), __shfl_down(lag, d, 64));
    __shared__ float wave_best[SOLA_THREADS / 64];
    __shared__ int wave_lag[SOLA_THREADS / 64];
    __shared__ int chosen;
    if ((threadIdx.x & 63) == 0) {
        wave_best[threadIdx.x >> 6] = best;
        wave_lag[threadIdx.x >> 6] = lag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {            // lane 0 started from lag 0, which exists
        for (int w = 1; w < SOLA_THREADS / 64; ++w) take_better(best, lag, wave_best[w], wave_lag[w]);
        chosen = (unsigned)lag <= (unsigned)search ? lag : 0;
        if (blockIdx.x == 0) *offset_out = chosen;
    }
    __syncthreads();
    const int offset = chosen;         // offset + block + xfade <= search + block + xfade = n_infer

    const int first = blockIdx.x * SOLA_EMIT_PER_BLOCK;
    const int last = first + SOLA_EMIT_PER_BLOCK < block ? first + SOLA_EMIT_PER_BLOCK : block;
    for (int i = first + threadIdx.x; i < last; i += SOLA_THREADS) {
        float v = infer[offset + i];
        if (i < xfade) {               // xfade <= block: every i < xfade is some lane's i
            const float f = fade_in[i];
            v = v * f + buf[i] * (1.f - f);
            buf[i] = infer[offset + block + i];
        }
        out[i] = v;
    }
}

static bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
    const char *p = (const char *)a, *q = (const char *)b;
    return a_bytes > 0 && b_bytes > 0 && p < q + b_bytes && q < p + a_bytes;
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_sola_workspace_bytes(int64_t xfade, int64_t search, size_t *bytes) {
    const char *fn = "rvc_sola_workspace_bytes";
    if (!bytes) return fail("%s: null pointer", fn);
    if (xfade < 1) return fail("%s: xfade %lld must be at least 1", fn, (long long)xfade);
    if (search < 0) return fail("%s: search %lld is negative", fn, (long long)search);
    if (xfade > SOLA_MAX_SAMPLES || search > SOLA_MAX_SAMPLES)
        return fail("%s: xfade %lld / search %lld exceeds 2^24 samples", fn, (long long)xfade, (long long)search);
    *bytes = (size_t)(search + 1) * sizeof(float);
    return 0;
}

extern "C" int rvc_sola_f32(const float *infer_dev, int64_t n_infer, float *buf_dev, const float *fade_in_dev, int64_t xfade,
                            int64_t search, int64_t block, float *out_dev, int *offset_dev, void *workspace_dev,
                            size_t workspace_bytes, void *hip_stream) {
    const char *fn = "rvc_sola_f32";
    if (!infer_dev || !buf_dev || !fade_in_dev || !out_dev || !offset_dev || !workspace_dev) return fail("%s: null pointer", fn);
    if (xfade < 1) return fail("%s: xfade %lld must be at least 1", fn, (long long)xfade);
    if (xfade > block) return fail("%s: xfade %lld is longer than the block (%lld)", fn, (long long)xfade, (long long)block);
    if (search < 0) return fail("%s: search %lld is negative", fn, (long long)search);
    if (n_infer > SOLA_MAX_SAMPLES) return fail("%s: n_infer %lld exceeds 2^24 samples", fn, (long long)n_infer);
    if (block > SOLA_MAX_SAMPLES || search > SOLA_MAX_SAMPLES || n_infer != block + xfade + search)
        return fail("%s: n_infer %lld is not block + xfade + search = %lld + %lld + %lld", fn, (long long)n_infer, (long long)block,
                    (long long)xfade, (long long)search);
    const size_t need = (size_t)(search + 1) * sizeof(float);
    if (workspace_bytes < need) return fail("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
    if (overlap(out_dev, block * 4, infer_dev, n_infer * 4)) return fail("%s: out_dev must not alias infer_dev", fn);
    if (overlap(out_dev, block * 4, buf_dev, xfade * 4)) return fail("%s: out_dev must not alias buf_dev", fn);
    if (overlap(buf_dev, xfade * 4, infer_dev, n_infer * 4)) return fail("%s: buf_dev must not alias infer_dev", fn);
    hipStream_t stream = (hipStream_t)hip_stream;
    float *score = (float *)workspace_dev;
    hipLaunchKernelGGL(sola_score_kernel, dim3((unsigned)(search + 1)), dim3(SOLA_THREADS), 0, stream, infer_dev, buf_dev, (int)xfade, score);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sola_emit_kernel, dim3((unsigned)ceil_div(block, SOLA_EMIT_PER_BLOCK)), dim3(SOLA_THREADS), 0, stream, infer_dev,
                       buf_dev, fade_in_dev, score, (int)xfade, (int)search, (int)block, out_dev, offset_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_stream_window_f32(float *hist_dev, int64_t n_hist, const float *block_dev, int64_t n_block, float *window_dev,
                                     void *hip_stream) {
    const char *fn = "rvc_stream_window_f32";
    if (!hist_dev || !block_dev || !window_dev) return fail("%s: null pointer", fn);
    if (n_hist < 0 || n_block < 0) return fail("%s: n_hist %lld / n_block %lld is negative", fn, (long long)n_hist, (long long)n_block);
    if (n_hist > SOLA_MAX_SAMPLES || n_block > SOLA_MAX_SAMPLES || n_hist + n_block > SOLA_MAX_SAMPLES)
        return fail("%s: n_hist + n_block = %lld + %lld exceeds 2^24 samples", fn, (long long)n_hist, (long long)n_block);
    const int64_t n = n_hist + n_block;
    if (overlap(window_dev, n * 4, hist_dev, n_hist * 4)) return fail("%s: window_dev must not alias hist_dev", fn);
    if (overlap(window_dev, n * 4, block_dev, n_block * 4)) return fail("%s: window_dev must not alias block_dev", fn);
    if (n == 0) return 0;
    hipLaunchKernelGGL(stream_window_kernel, dim3(1), dim3(WINDOW_THREADS), 0, (hipStream_t)hip_stream, hist_dev, n_hist, block_dev,
                       n_block, window_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}
