// Device helpers shared by the decoder kernels (decoder.hip, decoder_fs.hip).
#pragma once
#include "grid_index.h"
#include "ldm_internal.h"

#include <math.h>

namespace ldm {
namespace dec {

// Where a decoder tile's points come from: a run of the dense grid (rule A1 in the kernel), a
// point list, or a quarter of a listed 8^3 brick of the dense grid (band.hip).
enum DecMode { kModeGrid = 0, kModePoints = 1, kModeBricks = 2 };

#define LDM_STR2(x) #x
#define LDM_STR(x) LDM_STR2(x)

// ------------------------------------------------------------------------------------------
// A1: one grid axis value, x = fl32(fl32(i * vs) + origin).  Contraction is disabled so the
// device rounds twice exactly like the CPU oracle (SURVEY.md §7 'Bit-exact coordinates').
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float grid_axis(int i, float vs, float origin) {
#pragma clang fp contract(off)
    float t = (float)i * vs;
    return t + origin;
}

__device__ __forceinline__ void grid_point(int p, int N, int k0, float vs, float origin,
                                           float& x, float& y, float& z) {
    const int nn = N * N;
    const int k = k0 + p / nn;
    const int r = p - (p / nn) * nn;
    const int j = r / N;
    const int i = r - j * N;
    x = grid_axis(i, vs, origin);
    y = grid_axis(j, vs, origin);
    z = grid_axis(k, vs, origin);
}


// ------------------------------------------------------------------------------------------
// Pair blocks: the two MFMAs of one point chunk (m-chunks 0 and 1 on the same B fragment) and
// that pair's share of a step's epilogue VALU, in ONE fixed order inside one asm statement
// (DESIGN.md §4 "hand-ordered window steps").  Left to the compiler's scheduler, a step's epilogue
// went where the volatile accumulator pins left room: one MFMA gap with 14 VALU and two with
// none.  A 32x32x16 MFMA holds vector issue for 8 of its 32 cycles, so fillers of ~4 cycles each
// hide while a gap holds <= 6 of them; a block puts up to 6 VALU behind its first MFMA and up to
// 4 behind its second, whose gap also takes the memory operations.  Those stay in C++ between
// the blocks (the compiler's vmcnt / lgkmcnt bookkeeping sees every load: no load or LDS read is
// issued from inside a block) and keep their place through sched_barrier(0).
//
// Wait states (the compiler pads nothing inside an asm statement and does not see the MFMAs in
// it; CDNA3/4 ISA, table of required software wait states):
//   * XDL write -> XDL SrcC read of the SAME registers, same shape (the accumulate chain of
//     c0 / c1 from one step to the next, in a block or in compiled code after it): 0.
//   * The two MFMAs of a block write different accumulators and share only source operands: none.
//   * XDL write VGPR/AGPR -> v_accvgpr_read / VALU read of those registers, 8 passes: 11.  The
//     elements e* a block reads belong to the OTHER accumulator set, last written by the previous
//     part's final step: between that MFMA and the window's first block stand at least the 8
//     MFMAs of an aux step (256 cycles), and the set a block accumulates into is not read by
//     anything but MFMAs before the part ends.  tests/test_decoder_step_codegen.py counts both.
//   * VALU write VGPR -> MFMA SrcA/B read: 2.  A block's VALU write only its own temporaries and
//     result words (early-clobber outputs, never an operand of an MFMA); the A / B fragments are
//     loaded registers, waited for by the compiler's s_waitcnt ahead of the statement.
//   * VALU -> VALU and VALU -> ds_write data: none on gfx9.
// ------------------------------------------------------------------------------------------
#define LDM_PAIR_OPS(MFMA, CVT)                                                                   \
    /* one word: elements e0, e1 -> w (16-bit pair + ReLU).  TAIL: the step's last pair, whose    \
       second gap takes the B read, the two weight loads and the unit's write: all of the VALU    \
       behind the first MFMA */                                                                   \
    template <bool TAIL>                                                                          \
    static __device__ __forceinline__ void pair_cvt1(f32x16& c0, f32x16& c1, const u32x4& a0,     \
                                                     const u32x4& a1, const u32x4& b, float e0,   \
                                                     float e1, unsigned& w) {                     \
        unsigned t0, t1;                                                                          \
        if (!TAIL)                                                                                \
            asm volatile(MFMA " %0, %5, %7, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %3, %8\n\t"                                          \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         MFMA " %1, %6, %7, %1\n\t"                                               \
                         CVT " %2, %3, %4\n\t"                                                    \
                         "v_pk_max_i16 %2, %2, 0"                                                 \
                         : "+a"(c0), "+a"(c1), "=&v"(w), "=&v"(t0), "=&v"(t1)                     \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1));                           \
        else                                                                                      \
            asm volatile(MFMA " %0, %5, %7, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %3, %8\n\t"                                          \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         CVT " %2, %3, %4\n\t"                                                    \
                         "v_pk_max_i16 %2, %2, 0\n\t"                                             \
                         MFMA " %1, %6, %7, %1"                                                   \
                         : "+a"(c0), "+a"(c1), "=&v"(w), "=&v"(t0), "=&v"(t1)                     \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1));                           \
    }                                                                                             \
    /* two words (the double-unit step): e0..e3 -> w0, w1.  TAIL: 6 of the 8 VALU behind the      \
       first MFMA */                                                                              \
    template <bool TAIL>                                                                          \
    static __device__ __forceinline__ void pair_cvt2(f32x16& c0, f32x16& c1, const u32x4& a0,     \
                                                     const u32x4& a1, const u32x4& b, float e0,   \
                                                     float e1, float e2, float e3, unsigned& w0,  \
                                                     unsigned& w1) {                              \
        unsigned t0, t1;                                                                          \
        if (!TAIL)                                                                                \
            asm volatile(MFMA " %0, %6, %8, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         "v_accvgpr_read_b32 %5, %10\n\t"                                         \
                         CVT " %2, %4, %5\n\t"                                                    \
                         "v_pk_max_i16 %2, %2, 0\n\t"                                             \
                         MFMA " %1, %7, %8, %1\n\t"                                               \
                         "v_accvgpr_read_b32 %4, %11\n\t"                                         \
                         "v_accvgpr_read_b32 %5, %12\n\t"                                         \
                         CVT " %3, %4, %5\n\t"                                                    \
                         "v_pk_max_i16 %3, %3, 0"                                                 \
                         : "+a"(c0), "+a"(c1), "=&v"(w0), "=&v"(w1), "=&v"(t0), "=&v"(t1)         \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1), "a"(e2), "a"(e3));         \
        else                                                                                      \
            asm volatile(MFMA " %0, %6, %8, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         "v_accvgpr_read_b32 %5, %10\n\t"                                         \
                         CVT " %2, %4, %5\n\t"                                                    \
                         "v_pk_max_i16 %2, %2, 0\n\t"                                             \
                         "v_accvgpr_read_b32 %4, %11\n\t"                                         \
                         "v_accvgpr_read_b32 %5, %12\n\t"                                         \
                         MFMA " %1, %7, %8, %1\n\t"                                               \
                         CVT " %3, %4, %5\n\t"                                                    \
                         "v_pk_max_i16 %3, %3, 0"                                                 \
                         : "+a"(c0), "+a"(c1), "=&v"(w0), "=&v"(w1), "=&v"(t0), "=&v"(t1)         \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1), "a"(e2), "a"(e3));         \
    }                                                                                             \
    /* the final dot product, in fin1_unit's order: p = fma(relu(e1), w1, fma(relu(e0), w0, p));  \
       ReLU as an integer max with 0 (relu_f).  TAIL: all of it behind the first MFMA */          \
    template <bool TAIL>                                                                          \
    static __device__ __forceinline__ void pair_fin(f32x16& c0, f32x16& c1, const u32x4& a0,      \
                                                    const u32x4& a1, const u32x4& b, float e0,    \
                                                    float e1, float w0, float w1, float& p) {     \
        float t0, t1;                                                                             \
        if (!TAIL)                                                                                \
            asm volatile(MFMA " %0, %5, %7, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %3, %8\n\t"                                          \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         "v_max_i32_e32 %3, 0, %3\n\t"                                            \
                         "v_max_i32_e32 %4, 0, %4\n\t"                                            \
                         MFMA " %1, %6, %7, %1\n\t"                                               \
                         "v_fmac_f32_e32 %2, %3, %10\n\t"                                         \
                         "v_fmac_f32_e32 %2, %4, %11"                                             \
                         : "+a"(c0), "+a"(c1), "+v"(p), "=&v"(t0), "=&v"(t1)                      \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1), "v"(w0), "v"(w1));         \
        else                                                                                      \
            asm volatile(MFMA " %0, %5, %7, %0\n\t"                                               \
                         "v_accvgpr_read_b32 %3, %8\n\t"                                          \
                         "v_accvgpr_read_b32 %4, %9\n\t"                                          \
                         "v_max_i32_e32 %3, 0, %3\n\t"                                            \
                         "v_max_i32_e32 %4, 0, %4\n\t"                                            \
                         "v_fmac_f32_e32 %2, %3, %10\n\t"                                         \
                         "v_fmac_f32_e32 %2, %4, %11\n\t"                                         \
                         MFMA " %1, %6, %7, %1"                                                   \
                         : "+a"(c0), "+a"(c1), "+v"(p), "=&v"(t0), "=&v"(t1)                      \
                         : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1), "v"(w0), "v"(w1));         \
    }                                                                                             \
    /* pair_fin and one element more, of another chain: q = fma(relu(x), wx, q) */                \
    static __device__ __forceinline__ void pair_fin3(f32x16& c0, f32x16& c1, const u32x4& a0,     \
                                                     const u32x4& a1, const u32x4& b, float e0,   \
                                                     float e1, float w0, float w1, float& p,      \
                                                     float x, float wx, float& q) {               \
        float t0, t1, t2;                                                                         \
        asm volatile(MFMA " %0, %7, %9, %0\n\t"                                                   \
                     "v_accvgpr_read_b32 %4, %10\n\t"                                             \
                     "v_accvgpr_read_b32 %5, %11\n\t"                                             \
                     "v_max_i32_e32 %4, 0, %4\n\t"                                                \
                     "v_max_i32_e32 %5, 0, %5\n\t"                                                \
                     "v_accvgpr_read_b32 %6, %12\n\t"                                             \
                     MFMA " %1, %8, %9, %1\n\t"                                                   \
                     "v_fmac_f32_e32 %2, %4, %13\n\t"                                             \
                     "v_fmac_f32_e32 %2, %5, %14\n\t"                                             \
                     "v_max_i32_e32 %6, 0, %6\n\t"                                                \
                     "v_fmac_f32_e32 %3, %6, %15"                                                 \
                     : "+a"(c0), "+a"(c1), "+v"(p), "+v"(q), "=&v"(t0), "=&v"(t1), "=&v"(t2)      \
                     : "v"(a0), "v"(a1), "v"(b), "a"(e0), "a"(e1), "a"(x), "v"(w0), "v"(w1),      \
                       "v"(wx));                                                                  \
    }

// The 16-bit pack of a block: the one instruction the compiler selects for Elem<T>::pack where
// it sees both halves (round to nearest even; never v_cvt_pkrtz, which truncates).
#define LDM_CVT_BF16 "v_cvt_pk_bf16_f32"
#define LDM_CVT_F16 "v_cvt_pk_f16_f32"

// ------------------------------------------------------------------------------------------
// Element conversion + MFMA per 16-bit type.
// ------------------------------------------------------------------------------------------
template <typename T>
struct Elem;
template <>
struct Elem<__bf16> {
    static __device__ __forceinline__ unsigned pack(float a, float b) {
        // one v_cvt_pk_bf16_f32 (RNE); the element-wise {(__bf16)a, (__bf16)b} form costs two
        // single conversions + a v_perm
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = {a, b};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    }
    static __device__ __forceinline__ float round(float x) { return (float)(__bf16)x; }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                       __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    // a * b (C = 0) into VGPRs.  The builtin cannot say that: in a kernel that keeps
    // accumulators in AGPRs the compiler selects the AGPR destination for every MFMA and copies
    // the product back one register at a time.  An asm statement gets NO wait states from the
    // compiler: the caller keeps 12 issue slots between this statement and the first reader of
    // the product, and writes neither operand in the 2 slots before it (mfma_v's users say how).
    static __device__ __forceinline__ f32x16 mfma_v(u32x4 a, u32x4 b) {
        f32x16 d;
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(d) : "v"(a), "v"(b));
        return d;
    }
    static __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                       __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    LDM_PAIR_OPS("v_mfma_f32_32x32x16_bf16", LDM_CVT_BF16)
};
template <>
struct Elem<_Float16> {
    static __device__ __forceinline__ unsigned pack(float a, float b) {
        f16x2 v = {(_Float16)a, (_Float16)b};
        return __builtin_bit_cast(unsigned, v);
    }
    static __device__ __forceinline__ float round(float x) { return (float)(_Float16)x; }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                      __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    // a * b (C = 0) into VGPRs.  The builtin cannot say that: in a kernel that keeps
    // accumulators in AGPRs the compiler selects the AGPR destination for every MFMA and copies
    // the product back one register at a time.  An asm statement gets NO wait states from the
    // compiler: the caller keeps 12 issue slots between this statement and the first reader of
    // the product, and writes neither operand in the 2 slots before it (mfma_v's users say how).
    static __device__ __forceinline__ f32x16 mfma_v(u32x4 a, u32x4 b) {
        f32x16 d;
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(d) : "v"(a), "v"(b));
        return d;
    }
    static __device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                      __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    LDM_PAIR_OPS("v_mfma_f32_32x32x16_f16", LDM_CVT_F16)
};


// ReLU in the 16-bit domain: bf16 and f16 order like sign-magnitude, so max with +0 as signed
// int16 is ReLU (rounding commutes with ReLU).
__device__ __forceinline__ unsigned relu2(unsigned v) {
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    s16x2 x = __builtin_bit_cast(s16x2, v);
    const s16x2 z = {0, 0};
    x = __builtin_elementwise_max(x, z);
    return __builtin_bit_cast(unsigned, x);
}

// Accumulator m-chunk (rows = features, cols = points) -> two B fragments (k-steps 2i, 2i+1).
template <typename T>
__device__ __forceinline__ void acc_to_frags(const f32x16& a, u32x4& f0, u32x4& f1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f0[q] = relu2(Elem<T>::pack(a[2 * q], a[2 * q + 1]));
        f1[q] = relu2(Elem<T>::pack(a[8 + 2 * q], a[8 + 2 * q + 1]));
    }
}

}  // namespace dec
}  // namespace ldm
