// K16 -- the two device steps of Lloyd's k-means over the [N, D] fp32 feature matrix: nearest-centroid assignment and the
// centroid update.  Together with host bookkeeping (rvc_amd/lib/kmeans.py) they replace what the reference does on the CPU in
// rvc/train/process/extract_index.py:43-69 (sklearn MiniBatchKMeans above 2e5 rows, then faiss' IVF coarse-quantiser training
// and `add`).
//
// Assignment is a squared-L2 GEMM with a selection epilogue one deep: 2 N K D flop (15 TFLOP per pass at 2 M rows x 10 k
// centroids x 768), everything else is memory-bound.
//
// kmeans_assign_kernel
//   grid = (row tiles of 128) x (centroid stripes); block = 4 waves, block tile 128 centroids x 128 rows, wave tile 64 x 64 =
//   2 x 2 MFMA tiles of v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain, ascending k, one accumulator chain over the whole of D).
//   The centroids are the MFMA "A" (row) operand and the data rows the "B" (column) operand, as in knn_partial_kernel: a lane
//   owns ONE data row per MFMA tile and sees 16 candidate centroids of it in its accumulator registers, so the running best
//   (score, id) of that row lives in two registers of that lane.  Score = ||c||^2 - 2 x.c; ordered by cand_less (lower score,
//   then lower id), which is a total order: the winner does not depend on how rows or centroids are tiled or striped.
//   Centroids past the end of a stripe are masked with a NaN norm (never selected), rows past n_rows are computed on zeros and
//   not written.  The block merges its four (wave-row, lane-half) holders per row in LDS, slot 0..3 in that order, and writes
//   ONE (score, id) per (stripe, row).
// kmeans_finish_kernel
//   one wave per row: merges the stripes' winners in ascending stripe order, then evaluates d2 = sum_k (x_k - c_k)^2 of the
//   chosen centroid directly: lane l runs one fmaf chain over the float4 groups l, l + 64, ... of the row (x, y, z, w inside a
//   group), and the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.
//
// kmeans_update_partial_kernel / kmeans_update_combine_kernel
//   The members of centroid j are rows order[offsets[j] .. offsets[j + 1]).  A member list is cut into pieces of KM_PIECE rows;
//   piece p of centroid j has the workspace slot floor(offsets[j] / KM_PIECE) + j + p, which is unique, depends on `offsets`
//   only and is < floor(N / KM_PIECE) + K + 1.  One block per slot: it finds its (j, p) by bisection over the slot keys, then
//   walks its members in list order, thread t adding the float4 at column 4 t of each row (3 KB contiguous per row at D = 768,
//   eight rows in flight) into four float64 sums.  A centroid of one piece is finished there; longer ones are combined, in
//   piece order and in float64, by the second kernel, which also copies old -> out for centroids without members.  No atomics.
#include "knn_common.h"

namespace rvc {

constexpr int KM_BC = 128;                  // centroids per inner tile
constexpr int KM_BR = 128;                  // data rows per block
constexpr int KM_KC = 32;                   // floats of D per staged chunk
constexpr int KM_LDS_STRIDE = KM_KC + 1;
constexpr int KM_NO_ID = 0x7fffffff;
constexpr int KM_PIECE = 256;               // member rows per partial sum of the update
constexpr int64_t KM_TARGET_BLOCKS = 1024;  // the plan adds centroid stripes until the grid has this many blocks ...
constexpr int64_t KM_MAX_GRID = (int64_t)1 << 24;   // blocks of 256 threads per launch: fewer than 2^32 threads
constexpr int64_t KM_MIN_STRIPE = 4 * KM_BC;   // ... but no stripe is shorter than four centroid tiles

__global__ void __launch_bounds__(256)
kmeans_norms_kernel(const float *__restrict__ c, int64_t n, int dim, float *__restrict__ norms) {
    // one wave per centroid, float4 loads; lane chains over groups lane, lane + 64, ..., then the xor butterfly
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float4 *p = reinterpret_cast<const float4 *>(c + row * dim);
    float s = 0.f;
    for (int i = lane; i < dim / 4; i += 64) {
        const float4 v = p[i];
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) norms[row] = s;
}

// 166 VGPRs as compiled (64 accumulators + 32 staging + addresses; knn_partial_kernel's sorted top-8 needs 238): three waves per
// SIMD, i.e. three blocks per CU, which their 34 KB of LDS each allow too.  At four (128 VGPRs) it spills 116 bytes per lane.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
kmeans_assign_kernel(const float *__restrict__ x, int64_t n_rows, int dim, const float *__restrict__ cent,
                     const float *__restrict__ cnorm, int n_cent, int stripe_cents, float *__restrict__ part_s,
                     int *__restrict__ part_id) {
    __shared__ float Cs[KM_BC * KM_LDS_STRIDE];
    __shared__ float Xs[KM_BR * KM_LDS_STRIDE];
    __shared__ float cn_s[KM_BC];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1;   // which 64 centroids of the tile
    const int wn = wave & 1;    // which 64 rows of the block
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int64_t r0 = (int64_t)blockIdx.x * KM_BR;
    const int c_begin = blockIdx.y * stripe_cents;
    const int c_end = min(n_cent, c_begin + stripe_cents);
    const int n_tiles = c_end > c_begin ? (c_end - c_begin + KM_BC - 1) / KM_BC : 0;
    const int n_kc = dim / KM_KC;

    float best_s[2] = {INFINITY, INFINITY};
    int best_i[2] = {KM_NO_ID, KM_NO_ID};

    // staging registers: 4 passes x (32 rows x 8 float4) for each operand
    float4 cr[4], xr[4];
    const int srow = tid >> 3;
    const int sc4 = tid & 7;

    auto load_chunk = [&](int tile, int kc) {
        const int c_base = c_begin + tile * KM_BC;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int c = c_base + p * 32 + srow;
            cr[p] = (c < c_end) ? *reinterpret_cast<const float4 *>(cent + (int64_t)c * dim + kc * KM_KC + sc4 * 4)
                                : make_float4(0.f, 0.f, 0.f, 0.f);
            const int64_t r = r0 + p * 32 + srow;
            xr[p] = (r < n_rows) ? *reinterpret_cast<const float4 *>(x + r * dim + kc * KM_KC + sc4 * 4)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float *cd = &Cs[(p * 32 + srow) * KM_LDS_STRIDE + sc4 * 4];
            cd[0] = cr[p].x; cd[1] = cr[p].y; cd[2] = cr[p].z; cd[3] = cr[p].w;
            float *xd = &Xs[(p * 32 + srow) * KM_LDS_STRIDE + sc4 * 4];
            xd[0] = xr[p].x; xd[1] = xr[p].y; xd[2] = xr[p].z; xd[3] = xr[p].w;
        }
    };

    if (n_tiles > 0) load_chunk(0, 0);
    const float *cn_lane = &cn_s[wm * 64 + 4 * half];

    for (int tile = 0; tile < n_tiles; ++tile) {
        const int c_base = c_begin + tile * KM_BC;
        f32x16 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

        for (int kc = 0; kc < n_kc; ++kc) {
            __syncthreads();  // everyone is done reading the previous chunk (and the previous tile's cn_s)
            store_chunk();
            if (kc == 0 && tid < KM_BC) {
                const int c = c_base + tid;
                cn_s[tid] = (c < c_end) ? cnorm[c] : __builtin_nanf("");   // a NaN score compares false: never selected
            }
            __syncthreads();
            // prefetch the next chunk while this one is multiplied
            if (kc + 1 < n_kc) load_chunk(tile, kc + 1);
            else if (tile + 1 < n_tiles) load_chunk(tile + 1, 0);

            const float *ca = &Cs[(wm * 64 + l31) * KM_LDS_STRIDE + half];
            const float *xb = &Xs[(wn * 64 + l31) * KM_LDS_STRIDE + half];
#pragma unroll
            for (int kk = 0; kk < KM_KC / 2; ++kk) {
                const float a0 = ca[2 * kk];
                const float a1 = ca[32 * KM_LDS_STRIDE + 2 * kk];
                const float b0 = xb[2 * kk];
                const float b1 = xb[32 * KM_LDS_STRIDE + 2 * kk];
                acc[0][0] = mfma32(a0, b0, acc[0][0]);
                acc[0][1] = mfma32(a0, b1, acc[0][1]);
                acc[1][0] = mfma32(a1, b0, acc[1][0]);
                acc[1][1] = mfma32(a1, b1, acc[1][1]);
            }
        }
        // selection: the lane owns rows (wn*64 + nt*32 + l31); its registers hold 32 candidate centroids of each.  A lane meets
        // its candidates in ascending id (tile, m, r), so a strict < keeps the lower id of equal scores, and the winner is
        // remembered as that ordinal (tile*32 + m*16 + r: wave-uniform, so it costs no vector register) until the end.
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float cn = cn_lane[m * 32 + (r & 3) + 8 * (r >> 2)];
                const int ord = tile * 32 + m * 16 + r;
                const float s0 = fmaf(-2.f, acc[m][0][r], cn);
                const float s1 = fmaf(-2.f, acc[m][1][r], cn);
                if (s0 < best_s[0]) { best_s[0] = s0; best_i[0] = ord; }
                if (s1 < best_s[1]) { best_s[1] = s1; best_i[1] = ord; }
            }
        }
    }
    // ordinal -> centroid id
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int ord = best_i[nt];
        if (ord != KM_NO_ID)
            best_i[nt] = c_begin + (ord >> 5) * KM_BC + wm * 64 + ((ord >> 4) & 1) * 32 + mfma32_row(ord & 15, lane);
    }

    // the four (wave-row, lane-half) holders of a row -> one winner per (stripe, row), merged in slot order
    __syncthreads();
    float *ms = Cs;                                  // [4][KM_BR]
    int *mi = reinterpret_cast<int *>(Xs);           // [4][KM_BR]
    const int slot = wm * 2 + half;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        ms[slot * KM_BR + wn * 64 + nt * 32 + l31] = best_s[nt];
        mi[slot * KM_BR + wn * 64 + nt * 32 + l31] = best_i[nt];
    }
    __syncthreads();
    if (tid < KM_BR) {
        float bs = ms[tid];
        int bi = mi[tid];
#pragma unroll
        for (int s = 1; s < 4; ++s) {
            const float os = ms[s * KM_BR + tid];
            const int oi = mi[s * KM_BR + tid];
            if (cand_less(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        const int64_t r = r0 + tid;
        if (r < n_rows) {
            part_s[(int64_t)blockIdx.y * n_rows + r] = bs;
            part_id[(int64_t)blockIdx.y * n_rows + r] = bi;
        }
    }
}

__global__ void __launch_bounds__(256)
kmeans_finish_kernel(const float *__restrict__ x, int64_t n_rows, int dim, const float *__restrict__ cent, int n_cent,
                     const float *__restrict__ part_s, const int *__restrict__ part_id, int stripes,
                     int32_t *__restrict__ out_ids, float *__restrict__ out_d2) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += (int64_t)gridDim.x * 4) {
        float bs = part_s[row];
        int bi = part_id[row];
        for (int s = 1; s < stripes; ++s) {   // ascending stripe order
            const float os = part_s[(int64_t)s * n_rows + row];
            const int oi = part_id[(int64_t)s * n_rows + row];
            if (cand_less(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if ((unsigned)bi >= (unsigned)n_cent) bi = 0;   // every score of the row was NaN (non-finite data): still a valid id
        const float4 *xp = reinterpret_cast<const float4 *>(x + row * dim);
        const float4 *cp = reinterpret_cast<const float4 *>(cent + (int64_t)bi * dim);
        float s = 0.f;
        for (int i = lane; i < dim / 4; i += 64) {
            const float4 a = xp[i], b = cp[i];
            const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
            s = fmaf(dx, dx, s);
            s = fmaf(dy, dy, s);
            s = fmaf(dz, dz, s);
            s = fmaf(dw, dw, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            out_ids[row] = bi;
            out_d2[row] = s;
        }
    }
}

// ---- update -------------------------------------------------------------------------------------------------------
struct KmMembers {
    int64_t begin, count;
    int64_t slot0;   // workspace slot of the first piece
    int n_pieces;
};

__device__ __forceinline__ int64_t km_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t km_slot_key(const int64_t *offsets, int64_t j, int64_t n_rows) {
    return km_clamp(offsets[j], n_rows) / KM_PIECE + j;
}
// offsets are read defensively: whatever they hold, [begin, begin + count) stays inside order[0 .. n_rows)
__device__ __forceinline__ KmMembers km_members(const int64_t *offsets, int64_t j, int64_t n_rows) {
    KmMembers m;
    m.begin = km_clamp(offsets[j], n_rows);
    const int64_t end = km_clamp(offsets[j + 1], n_rows);
    m.count = end > m.begin ? end - m.begin : 0;
    m.slot0 = m.begin / KM_PIECE + j;
    m.n_pieces = (int)((m.count + KM_PIECE - 1) / KM_PIECE);
    return m;
}

__global__ void __launch_bounds__(256)
kmeans_update_partial_kernel(const float *__restrict__ x, int64_t n_rows, int dim, const int32_t *__restrict__ order,
                             const int64_t *__restrict__ offsets, int64_t n_cent, const float *__restrict__ old_cent,
                             float *__restrict__ out, double *__restrict__ part_sum, int *__restrict__ part_cnt) {
    __shared__ int ord_s[KM_PIECE];
    __shared__ int64_t j_s;
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (tid == 0) {   // the largest j whose first slot is <= this one (slot keys are strictly increasing in j)
        int64_t lo = -1, hi = n_cent - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (km_slot_key(offsets, mid, n_rows) <= slot) lo = mid;
            else hi = mid - 1;
        }
        j_s = lo;
    }
    __syncthreads();
    const int64_t j = j_s;
    if (j < 0) return;
    const KmMembers m = km_members(offsets, j, n_rows);
    const int64_t p = slot - m.slot0;
    if (p >= m.n_pieces) return;   // a slot no piece maps to
    const int64_t m0 = m.begin + p * KM_PIECE;
    const int len = (int)(m.count - p * KM_PIECE < KM_PIECE ? m.count - p * KM_PIECE : KM_PIECE);
    for (int i = tid; i < len; i += 256) {
        const int r = order[m0 + i];
        ord_s[i] = (r >= 0 && (int64_t)r < n_rows) ? r : -1;   // out-of-range entries are skipped
    }
    __syncthreads();
    if (tid >= dim / 4) return;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    int cnt = 0;
    const float *xc = x + tid * 4;
    for (int i0 = 0; i0 < len; i0 += 8) {
        int r[8];
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            r[u] = (i0 + u < len) ? ord_s[i0 + u] : -1;
            v[u] = (r[u] >= 0) ? *reinterpret_cast<const float4 *>(xc + (int64_t)r[u] * dim) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r[u] >= 0) {
                a0 += (double)v[u].x;
                a1 += (double)v[u].y;
                a2 += (double)v[u].z;
                a3 += (double)v[u].w;
                ++cnt;
            }
        }
    }
    if (m.n_pieces == 1) {
        float4 o;
        if (cnt > 0) {
            const double c = (double)cnt;
            o = make_float4((float)(a0 / c), (float)(a1 / c), (float)(a2 / c), (float)(a3 / c));
        } else {
            o = *reinterpret_cast<const float4 *>(old_cent + j * dim + tid * 4);
        }
        *reinterpret_cast<float4 *>(out + j * dim + tid * 4) = o;
    } else {
        double *ps = part_sum + slot * dim + tid * 4;
        ps[0] = a0; ps[1] = a1; ps[2] = a2; ps[3] = a3;
        if (tid == 0) part_cnt[slot] = cnt;
    }
}

__global__ void __launch_bounds__(256)
kmeans_update_combine_kernel(int64_t n_rows, int dim, const int64_t *__restrict__ offsets, const float *__restrict__ old_cent,
                             float *__restrict__ out, const double *__restrict__ part_sum, const int *__restrict__ part_cnt) {
    const int64_t j = blockIdx.x;
    const KmMembers m = km_members(offsets, j, n_rows);
    if (m.n_pieces == 1) return;   // finished by the partial kernel
    int64_t cnt = 0;
    for (int p = 0; p < m.n_pieces; ++p) cnt += part_cnt[m.slot0 + p];
    for (int c = threadIdx.x; c < dim; c += 256) {
        float o = old_cent[j * dim + c];
        if (cnt > 0) {
            double a = part_sum[m.slot0 * dim + c];
            for (int p = 1; p < m.n_pieces; ++p) a += part_sum[(m.slot0 + p) * dim + c];   // piece order
            o = (float)(a / (double)cnt);
        }
        out[j * dim + c] = o;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct KmPlan {
    int stripes, stripe_cents;
};

// Row tiles alone fill the device from ~131 k rows on; below that the centroids are cut into stripes of at least four tiles
// until the grid has KM_TARGET_BLOCKS blocks.  The result does not depend on the plan.
static KmPlan km_plan(int64_t n_rows, int64_t n_cent) {
    const int64_t row_tiles = ceil_div(n_rows > 0 ? n_rows : 1, KM_BR);
    int64_t want = ceil_div(KM_TARGET_BLOCKS, row_tiles);
    const int64_t max_stripes = ceil_div(n_cent, KM_MIN_STRIPE);
    if (want > max_stripes) want = max_stripes;
    if (want < 1) want = 1;
    KmPlan p;
    p.stripe_cents = (int)(ceil_div(ceil_div(n_cent, want), KM_BC) * KM_BC);
    p.stripes = (int)ceil_div(n_cent, p.stripe_cents);   // no empty stripe
    return p;
}

struct KmLayout {
    size_t norms, part_s, part_id;      // assign
    size_t part_sum, part_cnt;          // update
    size_t assign_bytes, update_bytes;
    size_t bytes() const { return assign_bytes > update_bytes ? assign_bytes : update_bytes; }   // one workspace serves both calls
    int64_t slots;
};

static KmLayout km_layout(int64_t n_rows, int64_t n_cent, int dim) {
    KmLayout l;
    const KmPlan p = km_plan(n_rows, n_cent);
    l.norms = 0;
    l.part_s = align_up((size_t)n_cent * sizeof(float), 256);
    l.part_id = l.part_s + align_up((size_t)p.stripes * (size_t)n_rows * sizeof(float), 256);
    l.assign_bytes = l.part_id + align_up((size_t)p.stripes * (size_t)n_rows * sizeof(int), 256);
    l.slots = n_rows / KM_PIECE + n_cent + 1;
    l.part_sum = 0;
    l.part_cnt = align_up((size_t)l.slots * (size_t)dim * sizeof(double), 256);
    l.update_bytes = l.part_cnt + align_up((size_t)l.slots * sizeof(int), 256);
    return l;
}

static int km_check_shape(const char *fn, int64_t n_rows, int64_t n_cent, int dim) {
    if (dim < 32 || dim > 1024 || dim % 32) return fail("%s: dim must be a multiple of 32 in [32, 1024], got %d", fn, dim);
    if (n_cent < 1) return fail("%s: n_centroids must be >= 1, got %lld", fn, (long long)n_cent);
    if (n_rows < 0) return fail("%s: n_rows must be >= 0, got %lld", fn, (long long)n_rows);
    if (n_rows >= (int64_t)1 << 31 || n_cent >= (int64_t)1 << 31)
        return fail("%s: 2^31 or more rows or centroids (%lld, %lld)", fn, (long long)n_rows, (long long)n_cent);
    return 0;
}

static bool km_misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_kmeans_workspace_bytes(int64_t n_rows, int64_t n_centroids, int dim, size_t *bytes) {
    if (!bytes) return fail("rvc_kmeans_workspace_bytes: null pointer");
    if (km_check_shape("rvc_kmeans_workspace_bytes", n_rows, n_centroids, dim)) return 1;
    const KmLayout l = km_layout(n_rows, n_centroids, dim);
    *bytes = l.bytes();
    return 0;
}

extern "C" int rvc_kmeans_assign(const float *x_dev, int64_t n_rows, int dim, const float *centroids_dev, int64_t n_centroids,
                                 int32_t *out_ids_dev, float *out_d2_dev, void *workspace_dev, size_t workspace_bytes,
                                 void *stream) {
    if (!x_dev || !centroids_dev || !out_ids_dev || !out_d2_dev || !workspace_dev) return fail("rvc_kmeans_assign: null pointer");
    if (km_check_shape("rvc_kmeans_assign", n_rows, n_centroids, dim)) return 1;
    if (km_misaligned(x_dev) || km_misaligned(centroids_dev) || km_misaligned(workspace_dev))
        return fail("rvc_kmeans_assign: x, centroids and workspace must be 16-byte aligned");
    const KmLayout l = km_layout(n_rows, n_centroids, dim);
    if (workspace_bytes < l.bytes()) return fail("rvc_kmeans_assign: workspace too small (%zu < %zu)", workspace_bytes, l.bytes());
    if (ceil_div(n_rows, KM_BR) >= KM_MAX_GRID) return fail("rvc_kmeans_assign: more than 2^31 - 128 rows");
    if (n_rows == 0) return 0;
    const KmPlan plan = km_plan(n_rows, n_centroids);
    char *ws = (char *)workspace_dev;
    float *norms = (float *)(ws + l.norms);
    float *part_s = (float *)(ws + l.part_s);
    int *part_id = (int *)(ws + l.part_id);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)ceil_div(n_centroids, 4)), dim3(256), 0, st, centroids_dev,
                       n_centroids, dim, norms);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)ceil_div(n_rows, KM_BR), (unsigned)plan.stripes), dim3(256), 0, st,
                       x_dev, n_rows, dim, centroids_dev, norms, (int)n_centroids, plan.stripe_cents, part_s, part_id);
    RVC_LAUNCH_CHECK();
    const int64_t finish_blocks = ceil_div(n_rows, 4) < KM_MAX_GRID ? ceil_div(n_rows, 4) : KM_MAX_GRID - 1;   // grid-stride beyond
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)finish_blocks), dim3(256), 0, st, x_dev, n_rows, dim,
                       centroids_dev, (int)n_centroids, part_s, part_id, plan.stripes, out_ids_dev, out_d2_dev);
    RVC_LAUNCH_CHECK();
    return 0;
}

extern "C" int rvc_kmeans_update(const float *x_dev, int64_t n_rows, int dim, const int32_t *order_dev,
                                 const int64_t *offsets_dev, int64_t n_centroids, const float *old_centroids_dev,
                                 float *out_centroids_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (!x_dev || !order_dev || !offsets_dev || !old_centroids_dev || !out_centroids_dev || !workspace_dev)
        return fail("rvc_kmeans_update: null pointer");
    if (km_check_shape("rvc_kmeans_update", n_rows, n_centroids, dim)) return 1;
    if (km_misaligned(x_dev) || km_misaligned(old_centroids_dev) || km_misaligned(out_centroids_dev) || km_misaligned(workspace_dev))
        return fail("rvc_kmeans_update: x, centroids and workspace must be 16-byte aligned");
    const KmLayout l = km_layout(n_rows, n_centroids, dim);
    if (workspace_bytes < l.bytes()) return fail("rvc_kmeans_update: workspace too small (%zu < %zu)", workspace_bytes, l.bytes());
    if (l.slots >= KM_MAX_GRID) return fail("rvc_kmeans_update: n_rows / %d + n_centroids must stay below 2^24", KM_PIECE);
    if (n_rows == 0) return 0;
    char *ws = (char *)workspace_dev;
    double *part_sum = (double *)(ws + l.part_sum);
    int *part_cnt = (int *)(ws + l.part_cnt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_update_partial_kernel, dim3((unsigned)l.slots), dim3(256), 0, st, x_dev, n_rows, dim, order_dev,
                       offsets_dev, n_centroids, old_centroids_dev, out_centroids_dev, part_sum, part_cnt);
    RVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_update_combine_kernel, dim3((unsigned)n_centroids), dim3(256), 0, st, n_rows, dim, offsets_dev,
                       old_centroids_dev, out_centroids_dev, part_sum, part_cnt);
    RVC_LAUNCH_CHECK();
    return 0;
}
