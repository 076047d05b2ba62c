// Device primitives shared by every kernel that multiplies fp32 operands on the bf16 matrix cores as exact bf16x3 splits
// (v = v_0 + v_1 + v_2, 8 + 8 + 8 significand bits), and the two buffer-addressing words all raw-buffer kernels use.
// A new kernel of the family includes this (through common.h) instead of copying a sibling's helpers.
#pragma once

#include <hip/hip_runtime.h>

namespace rvc {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Fourth word of __builtin_amdgcn_make_buffer_rsrc: raw buffer, 32-bit data format.  With it the hardware checks every access
// against the descriptor's num_bytes: a load beyond it returns 0, a store beyond it is dropped.
constexpr int RSRC_RAW32 = 0x00020000;
// A buffer offset beyond every tensor these kernels take (each slab is checked to be < 2 GiB, fits_2gib in conv.h): a lane that
// must not touch memory uses it instead of a branch -- loads return 0, stores are dropped.
constexpr unsigned BUF_OOB = 0x80000000u;

// Plain (unpacked) fp32 VALU for code that runs NEXT TO another wave's matrix instructions on the same SIMD: v_pk_add_f32 /
// v_pk_mul_f32 there waited ~100 cycles each (the stagers' 60 packed operations per tile took 7 800 cycles of a 20 000-cycle tile:
// profiles/r05_rbf_stamps.txt); inline asm, so that neither the vector types nor the SLP vectoriser can pack them again.
__device__ __forceinline__ float sub_np(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float add_np(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float mul_np(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The two halves of one level of the exact split, for kernels that schedule the levels (and the stores between them) themselves:
// split_word = v rounded to two bf16 (round to nearest even, v.x in the low half); split_rest = v minus that word, which is what the
// next level rounds (exact in fp32).
__device__ __forceinline__ unsigned split_word(f32x2 v) { return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2)); }
__device__ __forceinline__ f32x2 split_rest(f32x2 v, unsigned w) { return v - f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }
// v -> three words of two bf16 each whose sums are v.x and v.y exactly
__device__ __forceinline__ void split3(f32x2 v, unsigned w[3]) {
#pragma unroll
    for (int level = 0; level < 3; ++level) {
        w[level] = split_word(v);
        if (level < 2) v = split_rest(v, w[level]);
    }
}
// ... of (a, b), on non-packed subtracts (see sub_np)
__device__ __forceinline__ void split3_np(float a, float b, unsigned w[3]) {
#pragma unroll
    for (int level = 0; level < 3; ++level) {
        const unsigned ww = split_word(f32x2{a, b});
        w[level] = ww;
        if (level < 2) {
            a = sub_np(a, __uint_as_float(ww << 16));
            b = sub_np(b, __uint_as_float(ww & 0xffff0000u));
        }
    }
}

}  // namespace rvc
