// K3h -- one square ResBlock conv with fp32 taps on ERROR-CORRECTED fp16 PAIRS, the opt-in fast-fp32 vocoder mode
// (rvc_decoder_set_arithmetic(dec, 1)), in DIRECT form on the fp16 matrix cores:
//     y = out_scale * ( conv_d( leaky(x) ) + bias [+ res] [+ running sum] )                 (one conv of residuals.py:75-86 /
//                                                                                             MRFLayer.forward, hifigan_mrf.py:13-83)
// Every fp32 operand travels as (hi, lo 2^11) (f16x2.h) and  w x ~= w_hi x_hi + 2^-11 (w_hi x_lo + w_lo x_hi):  THREE matrix
// products per multiply-add where the exact bf16 triples of K3y / K3f need six -- what K3d (convbf1.hip) pays with one-term bf16
// taps, and K3d's structure carries over unchanged:
//   * the x chunk sits in LDS as fp16 pairs in [time][hi | lo][channel] order, the window fragment of ANY tap and dilation is one
//     conflict-free 16-byte read at (column + tap d);
//   * persistent: one 8-wave workgroup per CU walks (time tile) x (64 columns, ALL output channels) tiles; the input channels come
//     in chunks of 64 through a two-buffer LDS ring that the four STAGER waves fill (HBM -> registers a chunk ahead -> leaky ReLU ->
//     clamp to +-65504 -> split -> LDS) while the four COMPUTE waves multiply the previous chunk;
//   * the compute waves issue no memory operation but their tap-fragment loads (L2); outputs leave through an LDS tile
//     [channel][column] that the stagers drain with 16-byte row stores, adding residual / running sum / scale on the way.
// What differs from K3d:
//   * two planes per LDS row instead of three, two 1 KiB tap fragments (w_hi, w_lo 2^11) per (tap, k step, row block) instead of one;
//   * TWO accumulators per tile: acc0 takes w_hi x_hi, acc1 the two cross terms, which share the 2^11 scale; the epilogue forms
//     acc0 + acc1 2^-11 before the bias.  At C = 256 that is 128 accumulator registers of a compute wave's 256 (two waves per SIMD); the
//     bias moved to the stagers to make room.
// Subnormals: the fp16 conversions (v_cvt_f16_f32, the kernel's default float mode keeps fp16 / fp64 denormals) produce subnormal
// hi / lo parts, and they must CONTRIBUTE: flushed, an activation of 1e-3 loses the lo parts below 2^-14 and the result is wrong in
// the second digit.  FOUND on gfx950: v_mfma_f32_32x32x16_f16 takes subnormal operands at full value -- at activation amplitude 1e-3 the
// relative RMS error against float64 is 2.08e-7, the 2.0e-7 of the host simulation that keeps them (profiles/fastfp32_conv_shapes.txt).
// CHOSEN: no prescale; the stagers write the plain (hi, lo 2^11) pair.
// One barrier per 64-channel chunk, one more per launch.  Fixed accumulation order: bit-reproducible from launch to launch.
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "conv.h"
#include "f16x2.h"

namespace rvc {

constexpr int CH2_NTH = 512;
constexpr int CH2_CK = 64;                  // input channels per chunk
constexpr int CH2_N1 = 64;                  // output columns per tile

struct Ch2Params {
    const float *x = nullptr;        // [batch][C][L]
    const void *u = nullptr;         // convh2_pack_host's slab
    const float *bias = nullptr;     // [C] or null
    const float *res = nullptr;      // [batch][C][L] or null
    const float *accin = nullptr;    // [batch][C][L] or null (may alias y)
    float *y = nullptr;              // [batch][C][L], must not alias x
    int64_t L = 0;
    int dil = 1;
    float slope = 1.f, out_scale = 1.f;
    int tiles_per_row = 0, n_tiles = 0, per_xcd = 0;
};

template <int KW, int C>
struct Ch2Geom {
    static constexpr int NCH = C / CH2_CK;                    // input-channel chunks per tile
    static constexpr int RBW = C / 128;                       // 32-row blocks per compute wave
    static constexpr int KS = CH2_CK / 16;                    // 16-deep k steps per chunk and tap
    static constexpr int NGC = KW * KS;                       // (tap, k step) groups per chunk
    static constexpr int NGT = NCH * NGC;                     // ... per tile
    static constexpr int H = (KW - 1) / 2;
    static constexpr int ROWB = 4 * CH2_CK + 16;              // [hi | lo][channel 64] fp16 + 16 bytes: an odd multiple of 16
    static constexpr int XROWS = CH2_N1 + (KW - 1) * 5;       // dilation <= 5
    static constexpr int X_BYTES = (XROWS + 1) * ROWB;        // + one row that takes the writes of items outside the tile
    static constexpr int RC32 = (XROWS + 31) / 32;
    static constexpr int NIT = (CH2_CK / 8) * RC32 / 4;       // (32-row chunk, channel quad pair) items per stager wave and chunk
    static constexpr int IO_BYTES = C * CH2_N1 * 4;           // the finished tile [channel][column]
    static constexpr int LDS_BYTES = 2 * X_BYTES + IO_BYTES;
    static constexpr int ROWBLOCKS = C / 32;
    static constexpr int CONV_BYTES = NGT * ROWBLOCKS * 2048; // [group][row block][hi | lo 2^11][lane][8 fp16]
    static_assert(C == 128 || C == 256, "square layers of 128 or 256 channels");
    static_assert((CH2_CK / 8) * RC32 % 4 == 0, "the items must divide over the four stager waves");
    static_assert(4 * NIT + 28 <= 60, "memory operations in flight per stager wave (the counter holds 63)");
    static_assert(LDS_BYTES <= 163840, "LDS budget");
    static_assert((ROWB / 16) % 2 == 1, "row stride must be an odd multiple of 16 bytes");
};

template <int KW, int C>
__global__ void __launch_bounds__(CH2_NTH) __attribute__((amdgpu_waves_per_eu(2, 2)))
convh2_kernel(const Ch2Params p) {
    using GM = Ch2Geom<KW, C>;
    constexpr int NCH = GM::NCH, RBW = GM::RBW, KS = GM::KS, NGC = GM::NGC, NGT = GM::NGT, H = GM::H, ROWB = GM::ROWB, NIT = GM::NIT;
    constexpr int N1 = CH2_N1, CK = CH2_CK, PA = 8 / RBW;     // tap-fragment ring: 32 KiB per block in flight (a group is 6 RBW matrix instructions, 2 RBW fragments)

    extern __shared__ __attribute__((aligned(16))) unsigned char ch_smem[];
    unsigned char *const xs = ch_smem;                                        // [2][X_BYTES]
    float *const io_lds = reinterpret_cast<float *>(ch_smem + 2 * GM::X_BYTES);   // [C][N1]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int d = p.dil, XR = N1 + (KW - 1) * d;
    const int64_t L = p.L;
    const unsigned L4 = (unsigned)(L * 4);
    const int num_bytes = (int)((int64_t)C * L * 4);

    // this block's tiles: XCD x owns a contiguous range of tiles and its blocks walk it side by side (neighbouring tiles share their
    // halo columns in the same L2)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const int tile_end = (xcd + 1) * p.per_xcd < p.n_tiles ? (xcd + 1) * p.per_xcd : p.n_tiles;
    const int tile0 = xcd * p.per_xcd + slot;
    if (tile0 >= tile_end) return;
    const int my_tiles = (tile_end - tile0 + nslot - 1) / nslot;
    const int n_q = my_tiles * NCH;                            // chunks this block walks: chunk q = (tile tile0 + (q / NCH) nslot, channels 64 (q % NCH) ..)

    if (wave >= 4) {
        // ============================================ stagers: HBM <-> LDS ============================================================
        __builtin_amdgcn_s_setprio(1);                        // few instructions, on the block's critical path (the barriers)
        const int sw = wave - 4;
        float xr[NIT][4];
        constexpr int RC = GM::RC32;
        const int lq = lane >> 5;
        // item i of this wave = (channel quad pair qp of the chunk, 32-row chunk rc) with sw * NIT + i = qp * RC + rc; the lower half-wave
        // takes quad 2 qp, the upper one quad 2 qp + 1, a lane's row is rc * 32 + (lane & 31)
        auto x_issue = [&](int q) __attribute__((always_inline)) {
            const int tl = tile0 + (q / NCH) * nslot, ch0 = (q % NCH) * CK;
            const int bb = tl / p.tiles_per_row;
            const int xt0 = (tl - bb * p.tiles_per_row) * N1 - H * d;                       // time of row 0
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(p.x + (int64_t)bb * C * L), 0, num_bytes, RSRC_RAW32);
            const unsigned Lu = (unsigned)L;
            int sw_o = sw;
            asm volatile("" : "+s"(sw_o));                    // the per-item scalars are recomputed, not hoisted and spilled
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const int wi = sw_o * NIT + i, qp = wi / RC, rc = wi - qp * RC;
                const int qd = 2 * qp + lq, r = rc * 32 + l31;
                const unsigned tg = (unsigned)(xt0 + r);                                    // negative or beyond the row: >= L as unsigned
                const bool ok = r < XR && tg < Lu;
                const unsigned base = (unsigned)(ch0 + 4 * qd) * L4 + tg * 4u;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    xr[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(ok ? base + (unsigned)e * L4 : BUF_OOB), 0, 0));
            }
        };
        const float slope = p.slope;
        auto x_write = [&](int q) __attribute__((always_inline)) {
            unsigned char *const xb = xs + (q & 1) * GM::X_BYTES;
            int sw_o = sw;
            asm volatile("" : "+s"(sw_o));
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const int wi = sw_o * NIT + i, qp = wi / RC, rc = wi - qp * RC;
                const int qd = 2 * qp + lq, r = rc * 32 + l31;
                unsigned w[2][2];                             // [channel pair][hi | lo]
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const float va = xr[i][2 * e2], vb = xr[i][2 * e2 + 1];
                    split_f16x2_np(__builtin_fmaxf(va, mul_np(va, slope)), __builtin_fmaxf(vb, mul_np(vb, slope)), w[e2][0], w[e2][1]);
                }
                unsigned char *o = xb + (r < XR ? r : GM::XROWS) * ROWB + qd * 8;
#pragma unroll
                for (int s = 0; s < 2; ++s) *reinterpret_cast<u32x2 *>(o + s * 2 * CK) = u32x2{w[0][s], w[1][s]};
                if (i & 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        // ---- the finished tile: (io tile + bias + residual + running sum) * scale -> HBM, 16 bytes per lane, whole rows ---------------
        constexpr int CHUNKS = N1 / 4, RPW = 64 / CHUNKS, PASSES = C / (4 * RPW);
        constexpr int HP = 4, NHF = PASSES / HP;              // four passes at a time: registers
        const int chunk = lane % CHUNKS, rsub = lane / CHUNKS;
        const float out_scale = p.out_scale;
        const bool l4 = (L & 3) == 0;
        const bool has_res = p.res != nullptr, has_acc = p.accin != nullptr, has_bias = p.bias != nullptr;
        const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void *)(has_bias ? p.bias : p.y), 0, C * 4, RSRC_RAW32);
        auto out_store = [&](int tl) __attribute__((always_inline)) {
            const int bb = tl / p.tiles_per_row;
            const int64_t t0 = (int64_t)(tl - bb * p.tiles_per_row) * N1;
            const bool ok = t0 + 4 * chunk < L;
            const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void *)(p.y + (int64_t)bb * C * L), 0, num_bytes, RSRC_RAW32);
            const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc((void *)((has_res ? p.res : p.y) + (int64_t)bb * C * L), 0, num_bytes, RSRC_RAW32);
            const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc((void *)((has_acc ? p.accin : p.y) + (int64_t)bb * C * L), 0, num_bytes, RSRC_RAW32);
            const unsigned o0 = ok ? (unsigned)(sw * RPW + rsub) * L4 + (unsigned)(t0 + 4 * chunk) * 4u : BUF_OOB;
            auto load4 = [&](const __amdgpu_buffer_rsrc_t &rsrc, unsigned o) __attribute__((always_inline)) -> f32x4 {
                if (l4) return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0));
                float ae[4];                                  // rows not 16-byte aligned: element by element (past the row's end: zero)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned oe = (ok && t0 + 4 * chunk + e < L) ? o + 4u * (unsigned)e : BUF_OOB;
                    ae[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)oe, 0, 0));
                }
                return f32x4{ae[0], ae[1], ae[2], ae[3]};
            };
#pragma unroll
            for (int hf = 0; hf < NHF; ++hf) {
                f32x4 v[HP], rv[HP], av[HP];
                float bv[HP];
#pragma unroll
                for (int k = 0; k < HP; ++k) {
                    const unsigned o = o0 + (unsigned)((hf * HP + k) * 4 * RPW) * L4;         // (an out-of-range o0 stays out of range)
                    rv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    av[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    bv[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(brs, (int)(has_bias ? (unsigned)((((hf * HP + k) * 4 + sw) * RPW + rsub) * 4) : BUF_OOB), 0, 0));
                    if (has_res) rv[k] = load4(rrs, o);
                    if (has_acc) av[k] = load4(ars, o);
                }
#pragma unroll
                for (int k = 0; k < HP; ++k) v[k] = *reinterpret_cast<const f32x4 *>(io_lds + (((hf * HP + k) * 4 + sw) * RPW + rsub) * N1 + 4 * chunk);
#pragma unroll
                for (int k = 0; k < HP; ++k) {
                    const unsigned o = o0 + (unsigned)((hf * HP + k) * 4 * RPW) * L4;
                    float re[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                    const float r4[4] = {rv[k].x, rv[k].y, rv[k].z, rv[k].w}, a4[4] = {av[k].x, av[k].y, av[k].z, av[k].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        re[e] = add_np(re[e], bv[k]);
                        if (has_res) re[e] = add_np(re[e], r4[e]);
                        if (has_acc) re[e] = add_np(re[e], a4[e]);
                        re[e] = mul_np(re[e], out_scale);
                    }
                    if (l4) {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{re[0], re[1], re[2], re[3]}), yrs, (int)o, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned oe = (ok && t0 + 4 * chunk + e < L) ? o + 4u * (unsigned)e : BUF_OOB;
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, re[e]), yrs, (int)oe, 0, 0);
                        }
                    }
                }
            }
        };
        // Chunk q + 1 is requested behind barrier A(q) -- after chunk q + 1's predecessor in these registers (chunk q) has been
        // written -- and written to LDS buffer (q + 1) & 1 behind barrier A(q + 1)'s predecessor ... in program order per phase:
        //   A(q): buffer q & 1 is complete and the compute waves are done with buffer (q + 1) & 1
        //   [first chunk of a tile: the previous tile's outputs are in the io tile -> store them]
        //   write chunk q + 1 (requested a phase ago) into buffer (q + 1) & 1, request chunk q + 2
        // never more than one register set + the (at most 3 x 4 per half) output operations in flight per wave.
        x_issue(0);
        x_write(0);
        if (1 < n_q) x_issue(1);
        for (int q = 0; q < n_q; ++q) {
            lds_barrier();                                    // (A)
            if (q % NCH == 0 && q > 0) out_store(tile0 + (q / NCH - 1) * nslot);
            if (q + 1 < n_q) x_write(q + 1);
            // the output operations are a few thousand cycles old by now: all but eight of them have returned before the next set is
            // requested -- never more than 8 + one set of memory operations in flight per wave (resblock_bf.hip's rule)
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            if (q + 2 < n_q) x_issue(q + 2);
        }
        lds_barrier();                                        // (E) the last tile's outputs are in the io tile
        out_store(tile0 + (my_tiles - 1) * nslot);
        return;
    }

    // ================================================ compute waves ==========================================================
    // wave w owns output channels [32 RBW w, 32 RBW (w + 1)) x all 64 columns: RBW x 2 accumulator tiles
    const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc((void *)p.u, 0, GM::CONV_BYTES, RSRC_RAW32);
    f16x8 fa[PA][RBW][2];                                     // [ring slot][row block][w_hi | w_lo 2^11]
    f16x8 fb[2][2][2];                                        // [buffer][column tile][x_hi | x_lo 2^11]
    f32x16 acc[RBW][2][2];                                    // [row block][column tile][hi hi | cross terms 2^11]
    // group g (of the tile, 0 .. NGT - 1; the stream wraps: every tile uses the same taps): this wave's RBW row blocks
    auto load_a = [&](int slot_a, int g) __attribute__((always_inline)) {
        const int soff = (g * GM::ROWBLOCKS + RBW * wave) * 2048;
#pragma unroll
        for (int f = 0; f < 2 * RBW; ++f)
            fa[slot_a][f >> 1][f & 1] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(urs, 16 * lane + f * 1024, soff, 0));
    };
    // ... one of its 2 RBW fragments: f = 2 (row block) + (hi | lo)
    auto load_a1 = [&](int slot_a, int g, int f) __attribute__((always_inline)) {
        const int soff = (g * GM::ROWBLOCKS + RBW * wave) * 2048;
        fa[slot_a][f >> 1][f & 1] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(urs, 16 * lane + f * 1024, soff, 0));
    };
    // one window fragment of group gc (of the chunk): (column tile cb, plane s: 0 = hi, 1 = lo 2^11)
    auto load_b1 = [&](int buf, const unsigned char *src, int gc, int cb, int s) __attribute__((always_inline)) {
        const int tap = gc / KS, ks = gc - tap * KS;
        fb[buf][cb][s] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4 *>(src + tap * d * ROWB + ks * 32 + cb * 32 * ROWB + s * 2 * CK));
    };
#pragma unroll
    for (int g = 0; g < PA - 1; ++g) load_a(g, g);
    const int x_lane = l31 * ROWB + half * 16;
    float *const io_mine = io_lds + (32 * RBW * wave + 4 * half) * N1 + l31;
    constexpr int NM = 6 * RBW;                               // matrix instructions per group

    // The K loop is unrolled over TWO chunks (the ring slot of a group must be a compile-time register index and 2 NGC groups are a
    // multiple of the ring's eight or four); C = 256 walks its two chunk pairs in a run-time loop.
    static_assert((2 * NGC) % PA == 0 && NCH % 2 == 0, "two chunks of groups must be whole turns of the tap ring");
    int q = 0;
    for (int t = 0; t < my_tiles; ++t) {
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rb][cb][0][r] = acc[rb][cb][1][r] = 0.f;
#pragma unroll 1
        for (int cp = 0; cp < NCH / 2; ++cp) {
            const int g0 = cp * 2 * NGC;                      // first group of this chunk pair (wave-uniform)
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2, ++q) {
                lds_barrier();                                // (A) chunk q's rows are in buffer q & 1
                const unsigned char *const src = xs + (q & 1) * GM::X_BYTES + x_lane;
#pragma unroll
                for (int k = 0; k < 4; ++k) load_b1(0, src, 0, k & 1, 1 - (k >> 1));
#pragma unroll
                for (int gc = 0; gc < NGC; ++gc) {
                    const int gl = c2 * NGC + gc;             // compile-time: the group's place in the pair -> its ring slot
                    // 6 RBW matrix instructions: w_hi x_lo -> acc1, w_hi x_hi -> acc0, w_lo x_hi -> acc1 (the two updates of acc1 as far
                    // apart as the group allows); behind instruction k, pinned: one of the NEXT group's four window fragments (lo first),
                    // then the tap fragments of the group PA - 1 ahead (the stream wraps into the next tile: every tile uses the same taps)
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                            for (int rb = 0; rb < RBW; ++rb) {
                                const int k = (2 * i + cb) * RBW + rb;
                                const int wp = i == 2, xp = i == 0, ap = i != 1;          // term i: tap plane, window plane, accumulator
                                acc[rb][cb][ap] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[gl % PA][rb][wp], fb[gc & 1][cb][xp], acc[rb][cb][ap], 0, 0, 0);
                                __builtin_amdgcn_sched_barrier(0);
                                if (k < 4 && gc + 1 < NGC) load_b1((gc + 1) & 1, src, gc + 1, k & 1, 1 - (k >> 1));
                                if (k >= NM - 2 * RBW) {
                                    int gn = g0 + gl + PA - 1;
                                    gn = gn >= NGT ? gn - NGT : gn;
                                    load_a1((gl + PA - 1) % PA, gn, k - (NM - 2 * RBW));
                                }
                                __builtin_amdgcn_sched_barrier(0);
                            }
                }
            }
        }
        // ---- epilogue: acc0 + acc1 2^-11 into the io tile (bias, residual, running sum, scale and the stores are the stagers':
        // 128 accumulator registers of a wave's 256 at C = 256 leave no room for the bias here) -----------------------------
        // (the stagers took the previous tile's outputs out of the io tile behind this tile's first barrier A)
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    io_mine[(32 * rb + (r & 3) + 8 * (r >> 2)) * N1 + cb * 32] = __builtin_fmaf(acc[rb][cb][1][r], F16X2_LO_UNSCALE, acc[rb][cb][0][r]);
    }
    lds_barrier();                                            // (E)
}

// ---- host side -------------------------------------------------------------------------------------------------------------

bool convh2_supported(int c, int k, int dil) { return (c == 128 || c == 256) && (k == 3 || k == 7 || k == 11) && dil >= 1 && dil <= 5; }

// Where a mode-1 handle takes it (profiles/fastfp32_conv_shapes.txt: us per (dilated conv, conv + residual) pair at the cfg-2 stage lengths,
// two launches here against what the exact handle runs for the layer, same box, same session, both sides measured twice):
// C = 256: 117-122 / 206-209 / 302-304 at 3 / 7 / 11 taps against K3y's 187-191 / 300-316 / 401-414; C = 128: 362-376 at 3 taps against the
// fused pair's (K3f) 395-463, 539-552 / 742-747 at 7 / 11 taps against K3y's 604-658 / 776-830.  Every supported (C, K): 1.04-1.63 x.
bool convh2_preferred(int c, int k) {
#ifdef RVC_ABLATE
    static const int on = knob("RVC_CH2", 1);
    if (!on) return false;
#endif
    return convh2_supported(c, k, 1);
}

bool convh2_fits(int c, int64_t L) { return fits_2gib((int64_t)c * L, 4); }

size_t convh2_weight_bytes(int c, int k) { return (size_t)(c / 16) * k * (c / 32) * 2048; }

// w: [c][c][k] (PyTorch Conv1d layout), fp32 -> [chunk][tap][k step][row block][hi | lo 2^11][lane][8 fp16]: lane l of a fragment holds
// output channel 32 rb + (l & 31), input channels 64 chunk + 16 ks + 8 (l >> 5) .. + 7.  Non-zero (nothing packed) when a tap is
// non-finite or beyond fp16's range.
int convh2_pack_host(const float *w, int c, int k, std::vector<uint16_t> *out) {
    const int NCH = c / CH2_CK, KS = CH2_CK / 16, RB = c / 32;
    for (size_t i = 0, n = (size_t)c * c * k; i < n; ++i)
        if (!(w[i] >= -F16_MAX && w[i] <= F16_MAX)) return 1;
    out->assign(convh2_weight_bytes(c, k) / 2, 0);
    for (int ch = 0; ch < NCH; ++ch)
        for (int tap = 0; tap < k; ++tap)
            for (int ks = 0; ks < KS; ++ks)
                for (int rb = 0; rb < RB; ++rb)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const int co = 32 * rb + (lane & 31), ci = CH2_CK * ch + 16 * ks + 8 * (lane >> 5) + e;
                            const size_t group = ((size_t)ch * k + tap) * KS + ks, at = (group * RB + rb) * 1024 + lane * 8 + e;
                            f16x2_split_host(w[((size_t)co * c + ci) * k + tap], &(*out)[at], &(*out)[at + 512]);
                        }
    return 0;
}

template <int KW, int C>
static int ch2_launch(Ch2Params p, int batch, hipStream_t stream) {
    if (reserve_whole_cu((const void *)convh2_kernel<KW, C>, "convh2")) return 1;
    p.tiles_per_row = (int)ceil_div(p.L, CH2_N1);
    p.n_tiles = p.tiles_per_row * batch;
    const PersistentGrid g = persistent_grid(p.n_tiles);
    p.per_xcd = g.per_xcd;
    hipLaunchKernelGGL((convh2_kernel<KW, C>), dim3(g.blocks), dim3(CH2_NTH), LDS_WHOLE_CU, stream, p);   // owns its CU (common.h)
    RVC_LAUNCH_CHECK();
    return 0;
}

// x, y: [batch][c][L] (y must NOT alias x: blocks read their neighbours' columns; res / accin may alias y); u: convh2_pack_host's slab
int launch_convh2(const float *x, const void *u, const float *bias, const float *res, const float *accin, float *y, int batch, int c,
                   int64_t L, int k, int dil, float slope, float out_scale, hipStream_t stream) {
    if (!convh2_supported(c, k, dil)) return fail("convh2: unsupported shape (%d channels, %d taps, dilation %d)", c, k, dil);
    if (x == y) return fail("convh2: in-place operation is not supported");
    if (!(slope >= 0.f && slope <= 1.f)) return fail("convh2: leaky slope %g outside [0, 1]", (double)slope);
    if (!convh2_fits(c, L)) return fail("convh2: a %d x %lld slab exceeds the 2 GiB buffer addressing", c, (long long)L);
    if (L <= 0 || batch <= 0) return 0;
    if ((int64_t)ceil_div(L, CH2_N1) * batch >= ((int64_t)1 << 28)) return fail("convh2: too many tiles");
    Ch2Params p;
    p.x = x; p.u = u; p.bias = bias; p.res = res; p.accin = accin; p.y = y; p.L = L; p.dil = dil; p.slope = slope; p.out_scale = out_scale;
#define RVC_CH2_CASE(KW, CC) if (k == KW && c == CC) return ch2_launch<KW, CC>(p, batch, stream)
    RVC_CH2_CASE(3, 128); RVC_CH2_CASE(7, 128); RVC_CH2_CASE(11, 128);
    RVC_CH2_CASE(3, 256); RVC_CH2_CASE(7, 256); RVC_CH2_CASE(11, 256);
#undef RVC_CH2_CASE
    return fail("convh2: unsupported shape c=%d k=%d", c, k);
}

}  // namespace rvc

using namespace rvc;

extern "C" int rvc_conv1d_f16x2_weight_bytes(int c, int k, size_t *bytes) {
    if (!bytes) return fail("rvc_conv1d_f16x2_weight_bytes: null pointer");
    if (!convh2_supported(c, k, 1)) return fail("rvc_conv1d_f16x2_weight_bytes: c must be 128 or 256, k 3, 7 or 11");
    *bytes = convh2_weight_bytes(c, k);
    return 0;
}

extern "C" int rvc_conv1d_f16x2_pack_weight(const float *w_host, int c, int k, void *u_dev, void *stream) {
    if (!w_host || !u_dev) return fail("rvc_conv1d_f16x2_pack_weight: null pointer");
    size_t bytes = 0;
    if (!convh2_supported(c, k, 1)) return fail("rvc_conv1d_f16x2_pack_weight: c must be 128 or 256, k 3, 7 or 11");
    bytes = convh2_weight_bytes(c, k);
    std::vector<uint16_t> u;
    if (convh2_pack_host(w_host, c, k, &u))
        return fail("rvc_conv1d_f16x2_pack_weight: a tap is non-finite or beyond +-65504, the range of an fp16 pair");
    return upload_packed("rvc_conv1d_f16x2_pack_weight", u.data(), bytes, u_dev, stream);
}

extern "C" int rvc_conv1d_f16x2_forward(const float *x_dev, const void *u_dev, const float *bias_dev, const float *res_dev,
                                        const float *acc_dev, float *y_dev, int batch, int c, int64_t length, int k, int dilation,
                                        float slope_in, float out_scale, void *stream) {
    if (!x_dev || !u_dev || !y_dev) return fail("rvc_conv1d_f16x2_forward: null pointer");
    return launch_convh2(x_dev, u_dev, bias_dev, res_dev, acc_dev, y_dev, batch, c, length, k, dilation, slope_in, out_scale,
                         (hipStream_t)stream);
}
