// Voxel indices of a run of the dense grid without an integer divider (decoder_fs.hip's tile
// prologue; DESIGN.md §4 "tile prologue").  Point p of the slab [k0, k1) of an N^3 grid is the
// voxel k = k0 + p / N^2, j = p / N % N, i = p % N.  A decoder tile is 128 consecutive points
// from a wave-uniform first point, so its first voxel is decomposed ONCE (grid_first: scalar
// unit), and a lane adds its offset < 128 with two carries (grid_voxel).  Every division is a
// multiplication by a reciprocal of N formed once per launch on the host (grid_div).
//
// Plain C++ so that tests/c/grid_index_check.cpp checks it on the CPU against / and %.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LDM_HD inline
#endif

namespace ldm {
namespace dec {

// x / N == mulhi(x, m) when x * N < 2^32: with m = ceil(2^32 / N) = (2^32 + e) / N, 0 <= e < N,
// x m / 2^32 = x / N + x e / (N 2^32), and the error term stays below 1 / N.
// x / N == (x * mw) >> sh when x < 2^31: the same with mw = ceil(2^sh / N), sh = 31 +
// ceil(log2 N): x e < 2^31 N <= 2^sh; mw <= 2^32 - 2^16 for N <= 2^16 and x mw < 2^63.
struct GridDiv {
    uint32_t m, mw, sh;
};

// 2 <= N <= 46340 (a one-layer slab of N^2 < 2^31 points, the most the C ABI admits)
inline GridDiv grid_div(int N) {
    GridDiv d;
    d.m = (uint32_t)(((1ull << 32) + (uint32_t)N - 1) / (uint32_t)N);
    uint32_t lg = 0;
    while ((1u << lg) < (uint32_t)N) ++lg;
    d.sh = 31 + lg;
    d.mw = (uint32_t)(((1ull << d.sh) + (uint32_t)N - 1) / (uint32_t)N);
    return d;
}

LDM_HD uint32_t grid_mulhi(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)a * b) >> 32);
}

// a carry (<= 64) times N (< 2^24): both masks make it one full-rate v_mul_u32_u24 (a 32-bit
// v_mul_lo_u32 runs at a quarter of the rate)
LDM_HD uint32_t grid_mul24(uint32_t a, uint32_t b) {
    return (a & 0xffffffu) * (b & 0xffffffu);
}

// the voxel (i, j, k) of slab point p0 < 2^31 (k counted from the slab's first layer)
LDM_HD void grid_first(uint32_t p0, uint32_t N, GridDiv d, uint32_t& i, uint32_t& j,
                       uint32_t& k) {
    const uint32_t row = (uint32_t)(((uint64_t)p0 * d.mw) >> d.sh);   // p0 / N
    i = p0 - row * N;
    k = grid_mulhi(row, d.m);                  // row N <= p0 < 2^32
    j = row - k * N;
}

// the voxel of point p0 + off, off <= 127, from p0's voxel: i0 + off < N + 128 and
// j0 + carry < N + 64, so both products with N stay far below 2^32 (N (N + 128) < 2^32)
LDM_HD void grid_voxel(uint32_t i0, uint32_t j0, uint32_t k0, uint32_t off, uint32_t N,
                       uint32_t m, uint32_t& i, uint32_t& j, uint32_t& k) {
    const uint32_t x = i0 + off;
    const uint32_t cx = grid_mulhi(x, m);
    i = x - grid_mul24(cx, N);
    const uint32_t y = j0 + cx;
    const uint32_t cy = grid_mulhi(y, m);
    j = y - grid_mul24(cy, N);
    k = k0 + cy;
}

// a lane's offset into its tile: point min(p0 + want, npts - 1) of the ragged last tile
LDM_HD uint32_t grid_tail_off(uint32_t p0, uint32_t want, uint32_t npts) {
    const uint32_t last = npts - 1u - p0;      // the tile exists: p0 < npts
    return want < last ? want : last;
}

}  // namespace dec
}  // namespace ldm
