// Narrow-band decode, the passes around the decoder's brick mode: which 8^3
// bricks of a dense N^3 grid can hold the level set, as an ordered device list the decoder
// walks (decoder_fs.hip / decoder.hip, mode "bricks"), and the fill of every other brick.
//
// Definitions (also include/ldm_sdf.h):
//   brick    8 x 8 x 8 voxels; nb = ceil(N / 8) per axis; brick (bz, by, bx) covers the voxels
//            [8b, min(8b + 8, N)) per axis; id = (bz nb + by) nb + bx; global id = shape nb^3 + id.
//   lattice  per axis the nb + 1 fine-grid indices min(8b, N - 1), b = 0..nb: a subset of the
//            fine grid, its coordinates formed by rule A1 (grid_axis), so a lattice value is
//            the dense decode's value at that voxel bit for bit.
//   corners  a brick's 8 corners are the lattice points b and b + 1 per axis (when N - 1 is a
//            multiple of 8 the last brick is one voxel thick and its two corners coincide).
//   active   min over the corners of |v - level| <= band, or the corners not all on one side of
//            level (v > level against v <= level), or a corner not finite.
//   fill     every voxel of an inactive brick gets the brick's corner-0 value (the lattice value
//            at (bz, by, bx)); adjacent inactive bricks share corners, and all 8 corners of an
//            inactive brick lie on one side of level, so the fill puts no sign change between
//            two inactive bricks.
//
// Passes (all on the caller's stream, nothing read back to the host):
//   band_lattice_coords_kernel  [(nb+1)^3][3] coordinates for the points-mode decode
//   band_classify_kernel        one thread per brick -> active[g] (uint8)
//   flag_compact (flag_compact.h)  the active global ids in ascending order and their number:
//                               block sums per chunk of 4096 bricks, chunk scan, scatter; one
//                               segment of B nb^3 flags
//   band_fill_kernel            a sweep over the dense rows, 4 voxels per thread
// The compaction has no atomic append: the list is a pure function of `active`, whatever the
// scheduling.
#include "decoder_common.h"
#include "flag_compact.h"

namespace ldm {
namespace {
using namespace dec;

constexpr int kBrick = 8;
__host__ __device__ constexpr int band_nb(int N) { return (N + kBrick - 1) / kBrick; }

__global__ __launch_bounds__(256) void band_lattice_coords_kernel(int N, int nb, float vs,
                                                                  float origin,
                                                                  float* __restrict__ out) {
    const int n1 = nb + 1;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n1 * n1 * n1) return;
    const int lz = p / (n1 * n1), r = p - lz * n1 * n1;
    const int ly = r / n1, lx = r - ly * n1;
    out[3 * (size_t)p + 0] = grid_axis(min(kBrick * lx, N - 1), vs, origin);
    out[3 * (size_t)p + 1] = grid_axis(min(kBrick * ly, N - 1), vs, origin);
    out[3 * (size_t)p + 2] = grid_axis(min(kBrick * lz, N - 1), vs, origin);
}

// finite: the exponent field is not all ones
__device__ __forceinline__ bool band_finite(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u;
}

__global__ __launch_bounds__(256) void band_classify_kernel(const float* __restrict__ coarse,
                                                            int nb, int total, float level,
                                                            float band,
                                                            uint8_t* __restrict__ active) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int n1 = nb + 1, nb3 = nb * nb * nb;
    const int shape = g / nb3, id = g - shape * nb3;
    const int bz = id / (nb * nb), r = id - bz * nb * nb;
    const int by = r / nb, bx = r - by * nb;
    const float* c = coarse + (size_t)shape * n1 * n1 * n1 + ((size_t)bz * n1 + by) * n1 + bx;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = c[((q >> 2) * n1 + ((q >> 1) & 1)) * n1 + (q & 1)];
    bool near = false, fin = true, above = false, below = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        near = near || fabsf(v[q] - level) <= band;
        fin = fin && band_finite(v[q]);
        above = above || v[q] > level;
        below = below || v[q] <= level;
    }
    active[g] = (near || !fin || (above && below)) ? 1 : 0;
}

// Fill: thread -> 4 consecutive voxels of a dense row (they share a brick: 4 divides 8), quads
// in (shape, k, j, quad) order so a wave writes 1 KiB of a row; one 16-byte store when rows are
// 16-byte aligned (N % 4 == 0), else up to 4 scalar stores clipped at N.  A grid-stride loop: the
// quads of 64 shapes x 512^3 pass 2^31.
template <bool VEC>
__global__ __launch_bounds__(256) void band_fill_kernel(const float* __restrict__ coarse,
                                                        const uint8_t* __restrict__ active, int B,
                                                        int N, int nb, float* __restrict__ out) {
    const int Q = (N + 3) >> 2, n1 = nb + 1;
    const int64_t rows = (int64_t)B * N * N, quads = rows * Q;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < quads;
         g += (int64_t)gridDim.x * 256) {
        const int64_t row = g / Q;
        const int i0 = (int)(g - row * Q) * 4;
        const int j = (int)(row % N);
        const int64_t sk = row / N;
        const int k = (int)(sk % N), shape = (int)(sk / N);
        const int bx = i0 >> 3, by = j >> 3, bz = k >> 3;
        const int64_t gb = ((int64_t)shape * nb + bz) * nb * nb + (int64_t)by * nb + bx;
        if (active[gb]) continue;
        const float v = coarse[(int64_t)shape * n1 * n1 * n1 + ((int64_t)bz * n1 + by) * n1 + bx];
        float* dst = out + row * N + i0;         // i0 < N: in bounds
        if (VEC) {
            const f32x4 w = {v, v, v, v};
            *reinterpret_cast<f32x4*>(dst) = w;  // N % 4 == 0: i0 + 4 <= N, 16-byte aligned
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u < N) dst[u] = v;
        }
    }
}

// B >= 1, N >= 2 and B nb^3 < 2^31; the brick count through *total
int check_band_dims(const char* what, int B, int N, int64_t* total) {
    LDM_REQUIRE(N >= 2, LDM_EINVAL, "%s: N = %d < 2", what, N);
    LDM_REQUIRE(B >= 1, LDM_EINVAL, "%s: B = %d < 1", what, B);
    const int64_t nb = band_nb(N);
    LDM_REQUIRE(nb * nb * nb <= (int64_t)0x7fffffff / B, LDM_EINVAL,
                "%s: B * nb^3 = %d * %lld^3 does not fit 31 bits", what, B, (long long)nb);
    *total = (int64_t)B * nb * nb * nb;
    return 0;
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" size_t ldm_band_workspace_bytes(int B, int N) {
    int64_t total = 0;
    if (B < 1 || N < 2) return 0;
    const int64_t nb = band_nb(N);
    if (nb * nb * nb > (int64_t)0x7fffffff / B) return 0;
    total = (int64_t)B * nb * nb * nb;
    return flag_compact_ws(1, total, nullptr).bytes;
}

extern "C" int ldm_band_lattice_coords(int N, float vs, float origin, float* xyz_out,
                                       ldm_stream_t s) {
    LDM_REQUIRE(N >= 2, LDM_EINVAL, "ldm_band_lattice_coords: N = %d < 2", N);
    LDM_REQUIRE(xyz_out != nullptr, LDM_EINVAL, "ldm_band_lattice_coords: xyz_out NULL");
    LDM_REQUIRE(LDM_ALIGNED(xyz_out, 4), LDM_EALIGN, "ldm_band_lattice_coords: misaligned xyz_out");
    const int64_t n1 = band_nb(N) + 1;
    LDM_REQUIRE(n1 * n1 * n1 < (1ll << 31), LDM_EINVAL, "ldm_band_lattice_coords: N too large");
    const int64_t n = n1 * n1 * n1;
    hipLaunchKernelGGL(band_lattice_coords_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, N, (int)n1 - 1, vs, origin, xyz_out);
    return launch_status("ldm_band_lattice_coords");
}

extern "C" int ldm_band_classify(const float* coarse, int B, int N, float level, float band,
                                 uint8_t* active, int32_t* bricks, int32_t* count, void* ws,
                                 size_t ws_bytes, ldm_stream_t s) {
    int64_t total = 0;
    LDM_TRY(check_band_dims("ldm_band_classify", B, N, &total));
    LDM_REQUIRE(coarse && active && bricks && count && ws, LDM_EINVAL,
                "ldm_band_classify: NULL buffer");
    LDM_REQUIRE(band >= 0.f, LDM_EINVAL, "ldm_band_classify: band must be >= 0 (inf allowed)");
    LDM_REQUIRE(LDM_ALIGNED(coarse, 4) && LDM_ALIGNED(active, 16) && LDM_ALIGNED(bricks, 4) &&
                    LDM_ALIGNED(count, 4) && LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "ldm_band_classify: active must be 16-byte, the workspace 256-byte "
                "aligned");
    const FlagCompactWs w = flag_compact_ws(1, total, ws);
    LDM_REQUIRE(ws_bytes >= w.bytes, LDM_ENOSPC, "ldm_band_classify: workspace %zu < %zu B",
                ws_bytes, w.bytes);
    const int n = (int)total, nb = band_nb(N);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(band_classify_kernel, dim3((n + 255) / 256), dim3(256), 0, st, coarse, nb,
                       n, level, band, active);
    flag_compact(active, 1, n, w, bricks, count, st);   // active is 16-byte aligned: vector loads
    return launch_status("ldm_band_classify");
}

extern "C" int ldm_band_fill(const float* coarse, const uint8_t* active, int B, int N, float* out,
                             ldm_stream_t s) {
    int64_t total = 0;
    LDM_TRY(check_band_dims("ldm_band_fill", B, N, &total));
    LDM_REQUIRE(coarse && active && out, LDM_EINVAL, "ldm_band_fill: NULL buffer");
    LDM_REQUIRE(LDM_ALIGNED(coarse, 4) && LDM_ALIGNED(out, 16), LDM_EALIGN,
                "ldm_band_fill: out must be 16-byte aligned");
    const int64_t quads = (int64_t)B * N * N * ((N + 3) / 4);
    const int64_t want = (quads + 255) / 256;
    const unsigned grid = (unsigned)(want < (1 << 20) ? want : (1 << 20));
    hipStream_t st = (hipStream_t)s;
    if ((N & 3) == 0)
        hipLaunchKernelGGL(band_fill_kernel<true>, dim3(grid), dim3(256), 0, st, coarse, active, B,
                           N, band_nb(N), out);
    else
        hipLaunchKernelGGL(band_fill_kernel<false>, dim3(grid), dim3(256), 0, st, coarse, active,
                           B, N, band_nb(N), out);
    return launch_status("ldm_band_fill");
}
