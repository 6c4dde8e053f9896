// One output row of the sampling GEMV: the arithmetic shared by the per-step kernel
// (denoiser.hip small_linear_kernel) and the persistent loop (sample_loop.hip), which is why the
// two are bit-identical.  One wave per row; lane l owns the 8-element k chunks l + 64 j
// (j < NJ = ceil(K / 8 / 64), K <= 2048).
#pragma once
#include "ldm_internal.h"
#include "ddpm_common.h"

namespace ldm {

// The lane's chunks of weight row `row` (fp32, or bf16 unpacked to fp32) into registers.  Every
// global load is unconditional (index clamped, value selected afterwards) so a wave issues all
// of its loads back to back -- a load under a divergent branch makes hipcc wait vmcnt(0) before
// leaving the branch, one round trip per load.  Chunks past K are zero.
template <typename TW, int NJ>
__device__ __forceinline__ void load_row(float (&w)[NJ][8], const void* W, int row, int ldw,
                                         int K, int lane) {
    const int nch = K >> 3;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        const bool on = c < nch;
        const size_t off = (size_t)row * ldw + (on ? c : 0) * 8;
        if constexpr (sizeof(TW) == 2) {
            uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(W) + off);
            const unsigned q[4] = {on ? u.x : 0u, on ? u.y : 0u, on ? u.z : 0u, on ? u.w : 0u};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[j][2 * i] = __builtin_bit_cast(float, q[i] << 16);
                w[j][2 * i + 1] = __builtin_bit_cast(float, q[i] & 0xffff0000u);
            }
        } else {
            const float* wp = reinterpret_cast<const float*>(W) + off;
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[j][i] = on ? w0[i] : 0.f;
                w[j][4 + i] = on ? w1[i] : 0.f;
            }
        }
    }
}

// One wave's row dot products for all batch rows of xs ([B][K] fp32 in LDS), reduced so that
// lane `writer` of group b holds acc[0] = sum_k X[b][k] w[k].  Returns acc[0].  Off lanes
// multiply zero weights with a valid chunk; rows past B repeat row 0 and are never written out.
template <int MB, int NJ>
__device__ __forceinline__ float row_dot(const float (&w)[NJ][8], const float* xs, int B, int K,
                                         int lane) {
    const int nch = K >> 3;
    float acc[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[b] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        const int cc = c < nch ? c : 0;
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            const int bb = b < B ? b : 0;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(xs + bb * K + cc * 8);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(xs + bb * K + cc * 8 + 4);
            float t = acc[b];
            t = fmaf(w[j][0], x0[0], t); t = fmaf(w[j][1], x0[1], t);
            t = fmaf(w[j][2], x0[2], t); t = fmaf(w[j][3], x0[3], t);
            t = fmaf(w[j][4], x1[0], t); t = fmaf(w[j][5], x1[1], t);
            t = fmaf(w[j][6], x1[2], t); t = fmaf(w[j][7], x1[3], t);
            acc[b] = t;
        }
    }
    // reduce-scatter: at level lv (offset o = 32 >> lv) a lane keeps the half of its n = MB >> lv
    // values selected by lane & o and adds its partner's copy of that half.  Its own butterfly,
    // not sample_loop.hip's reduce_scatter<MB>: that call changes the persistent loop's ISA.
#pragma unroll
    for (int lv = 0; lv < 6; ++lv) {
        const int o = 32 >> lv;
        const int n = MB >> lv;
        const bool upper = (lane & o) != 0;
        if (n > 1) {
            const int half = n >> 1;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                const float send = upper ? acc[i] : acc[i + half];
                const float keep = upper ? acc[i + half] : acc[i];
                acc[i] = keep + xor_lane(send, o, lane);
            }
        } else {
            acc[0] += xor_lane(acc[0], o, lane);
        }
    }
    return acc[0];
}

}  // namespace ldm
