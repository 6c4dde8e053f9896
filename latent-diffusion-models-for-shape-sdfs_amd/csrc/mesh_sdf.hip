// Signed distance from query points to a triangle soup, MI355X (gfx950).  DESIGN.md §16.
//
// The first stage of the path: DeepSDF's SdfSamples are made from raw meshes by evaluating
// 500 000 points against every triangle -- no acceleration structure, no approximation.  Per
// point: the distance to the closest triangle, that triangle's index (ties to the smaller
// index) and the generalized winding number, whose comparison with 0.5 gives the sign on
// meshes that are not watertight.  The pair arithmetic is mesh_sdf_pair.h.
//
// Kernels (all fp32 VALU; no float atomics):
//   pack     one thread per face: indices clamped to [0, V) (a clamp raises *flag), the record
//            MeshTri written to the workspace
//   eval     256 threads, one point per thread held in registers.  The triangle record is
//            read at a wave-uniform address (loop counter + blockIdx only): the compiler turns
//            that into scalar loads, and the record feeds the VALU from SGPRs.
//   combine  split form only: adds the per-chunk partials of one point in chunk order
//
// Summation shape (fixed, independent of P): faces are cut into chunks of kFaceChunk; a
// chunk's half solid angles are added in face order into a chunk partial that starts at 0; the
// partials are added in ascending chunk order into a sum that starts at 0.  The closest face is
// the lexicographic minimum of (d^2, index), which no order can change.
//   one-pass form  (P >= kSplitBelow or one chunk)  a thread walks all chunks
//   split form     (P <  kSplitBelow)  grid.y = chunks, partials (sum, d^2, index) to the
//                  workspace per tile of kSplitTile points, then combine
// Both forms perform the same additions in the same order, so a point's outputs are bitwise
// the same alone or among a million others.
#include "ldm_internal.h"
#include "mesh_sdf_pair.h"

namespace ldm {
namespace {

constexpr int kFaceChunk = 1024;       // faces per chunk: the summation shape
constexpr int64_t kSplitBelow = 16384; // P below this (and > 1 chunk): split over chunks
constexpr int kSplitTile = 4096;       // points per workspace tile of the split form
constexpr int kThreads = 256;
// points per thread.  1 in both forms: at 500 000 points x 184 384 faces 1 / 2 / 4 measured
// 372 / 377 / 392 ms (more waves per SIMD beat the packed fp32 forms two points allow, which
// issue no faster than two plain instructions)
constexpr int kPtsOnePass = 1, kPtsSplit = 1;
static_assert(kSplitTile % (kThreads * kPtsSplit) == 0, "a tile is whole workgroups");
static_assert(sizeof(MeshTri) == 80, "MeshTri: five 16-byte vectors");

struct alignas(16) Partial {
    float sum;     // the chunk's half solid angles, added in face order
    float d2;      // smallest squared distance in the chunk
    int32_t face;  // its face (the smallest index on a tie), -1 for none
    int32_t pad;
};

__global__ __launch_bounds__(kThreads) void mesh_pack_kernel(const float* __restrict__ verts,
                                                             int V,
                                                             const int32_t* __restrict__ faces,
                                                             int F, MeshTri* __restrict__ tri,
                                                             int32_t* __restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    int id[3];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int raw = faces[f * 3 + k];
        id[k] = min(max(raw, 0), V - 1);
        bad = bad || id[k] != raw;
    }
    if (bad) atomicOr(flag, 1);
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[k][c] = verts[(int64_t)id[k] * 3 + c];
    tri[f] = mesh_tri_pack(p[0], p[1], p[2]);
}

// the one place a point's three outputs are formed from (sum, d^2, face)
__device__ __forceinline__ void mesh_finish(float sum, float d2, int32_t face, int64_t i,
                                            float* __restrict__ sdf,
                                            int32_t* __restrict__ closest,
                                            float* __restrict__ winding) {
#pragma clang fp contract(off)
    const float w = sum * 0.15915494309189535f;   // sum of Omega / 2, over 2 pi
    // one v_sqrt_f32 (1 ulp), not sqrtf: the library square root compiled to two different
    // instruction sequences in the two kernels that inline this function, a last-bit
    // difference between the launch forms
    const float d = __builtin_amdgcn_sqrtf(d2);
    sdf[i] = w > 0.5f ? -d : d;
    if (closest) closest[i] = face;
    if (winding) winding[i] = w;
}

// SPLIT: blockIdx.y is the chunk, `part` takes [chunk][tile point]; else every chunk is walked
// and the outputs are written.  `pts` / outputs / `part` are those of the tile, n its points.
template <int PTS, bool SPLIT>
__global__ __launch_bounds__(kThreads) void mesh_eval_kernel(const MeshTri* __restrict__ tri,
                                                             int F,
                                                             const float* __restrict__ pts,
                                                             int64_t n,
                                                             float* __restrict__ sdf,
                                                             int32_t* __restrict__ closest,
                                                             float* __restrict__ winding,
                                                             Partial* __restrict__ part,
                                                             int tile_stride) {
#pragma clang fp contract(off)
    const int64_t base = (int64_t)blockIdx.x * (kThreads * PTS) + threadIdx.x;
    float px[PTS], py[PTS], pz[PTS], sum[PTS], best[PTS];
    int32_t bface[PTS];
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int64_t i = min(base + (int64_t)k * kThreads, n - 1);   // past the end: clamped
        px[k] = pts[i * 3 + 0];
        py[k] = pts[i * 3 + 1];
        pz[k] = pts[i * 3 + 2];
        sum[k] = 0.0f;
        best[k] = INFINITY;
        bface[k] = -1;
    }
    const int nchunk = (F + kFaceChunk - 1) / kFaceChunk;
    const int c_begin = SPLIT ? (int)blockIdx.y : 0;
    const int c_end = SPLIT ? c_begin + 1 : nchunk;
    for (int c = c_begin; c < c_end; ++c) {
        const int f0 = c * kFaceChunk, f1 = min(f0 + kFaceChunk, F);
        float cs[PTS];
#pragma unroll
        for (int k = 0; k < PTS; ++k) cs[k] = 0.0f;
        for (int f = f0; f < f1; ++f) {
            const MeshTri T = tri[f];                    // wave-uniform: scalar loads
#pragma unroll
            for (int k = 0; k < PTS; ++k) {
                float d2, h;
                pair_eval(T, px[k], py[k], pz[k], &d2, &h);
                cs[k] = cs[k] + h;
                const bool lt = d2 < best[k];            // strict: the smaller index keeps a tie
                best[k] = lt ? d2 : best[k];
                bface[k] = lt ? f : bface[k];
            }
        }
#pragma unroll
        for (int k = 0; k < PTS; ++k) sum[k] = SPLIT ? cs[k] : sum[k] + cs[k];
    }
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int64_t i = base + (int64_t)k * kThreads;
        if (i >= n) continue;
        if (SPLIT) {
            Partial o;
            o.sum = sum[k];
            o.d2 = best[k];
            o.face = bface[k];
            o.pad = 0;
            part[(int64_t)blockIdx.y * tile_stride + i] = o;
        } else {
            mesh_finish(sum[k], best[k], bface[k], i, sdf, closest, winding);
        }
    }
}

__global__ __launch_bounds__(kThreads) void mesh_combine_kernel(const Partial* __restrict__ part,
                                                                int nchunk, int tile_stride,
                                                                int n, float* __restrict__ sdf,
                                                                int32_t* __restrict__ closest,
                                                                float* __restrict__ winding) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float sum = 0.0f, best = INFINITY;
    int32_t bface = -1;
    for (int c = 0; c < nchunk; ++c) {
        const Partial p = part[(int64_t)c * tile_stride + i];
        sum = sum + p.sum;
        const bool lt = p.d2 < best;                     // chunks ascend: so do the indices
        best = lt ? p.d2 : best;
        bface = lt ? p.face : bface;
    }
    mesh_finish(sum, best, bface, i, sdf, closest, winding);
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int n_chunks(int F) { return (F + kFaceChunk - 1) / kFaceChunk; }
inline bool use_split(int F, int64_t P) { return P < kSplitBelow && n_chunks(F) > 1; }
inline size_t tri_bytes(int F) { return up256((size_t)F * sizeof(MeshTri)); }

}  // namespace
}  // namespace ldm

extern "C" int ldm_mesh_sdf_face_chunk(void) { return ldm::kFaceChunk; }
extern "C" int64_t ldm_mesh_sdf_split_below(void) { return ldm::kSplitBelow; }

extern "C" size_t ldm_mesh_sdf_ws_bytes(int F, int64_t P) {
    using namespace ldm;
    if (F < 0 || P < 0) return 0;
    size_t b = 256 + tri_bytes(F);
    if (use_split(F, P))
        b += up256((size_t)n_chunks(F) * (size_t)min((int64_t)kSplitTile, P) * sizeof(Partial));
    return b;
}

extern "C" int ldm_mesh_sdf(const float* verts, int V, const int32_t* faces, int F,
                            const float* points, int64_t P, float* sdf, int32_t* closest,
                            float* winding, int32_t* flag, void* ws, size_t ws_bytes,
                            ldm_stream_t s) {
    using namespace ldm;
    LDM_REQUIRE(V >= 0 && F >= 0 && P >= 0, LDM_EINVAL,
                "ldm_mesh_sdf: negative size (V = %d, F = %d, P = %lld)", V, F, (long long)P);
    if (P == 0) return 0;
    LDM_REQUIRE(points && sdf && flag && ws, LDM_EINVAL,
                "ldm_mesh_sdf: NULL points / sdf / flag / workspace");
    LDM_REQUIRE(F == 0 || (verts && faces && V > 0), LDM_EINVAL,
                "ldm_mesh_sdf: %d faces need vertices (V = %d) and indices", F, V);
    LDM_REQUIRE(LDM_ALIGNED(points, 4) && LDM_ALIGNED(sdf, 4) && LDM_ALIGNED(closest, 4) &&
                    LDM_ALIGNED(winding, 4) && LDM_ALIGNED(flag, 4) && LDM_ALIGNED(verts, 4) &&
                    LDM_ALIGNED(faces, 4) && LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "ldm_mesh_sdf: tensors must be 4-B, the workspace 256-B aligned");
    const size_t need = ldm_mesh_sdf_ws_bytes(F, P);
    LDM_REQUIRE(ws_bytes >= need, LDM_ENOSPC, "ldm_mesh_sdf: workspace %zu < %zu B", ws_bytes,
                need);
    // the grids of both forms, checked with the arguments: nothing is queued before a refusal
    const bool split = use_split(F, P);
    constexpr int64_t per = kThreads * kPtsOnePass;
    const int64_t blocks = (P + per - 1) / per;
    LDM_REQUIRE(split || blocks <= 0x7fffffff, LDM_EINVAL,
                "ldm_mesh_sdf: P = %lld needs more than 2^31 - 1 workgroups", (long long)P);
    const int nchunk = n_chunks(F);
    LDM_REQUIRE(!split || nchunk <= 65535, LDM_EINVAL,
                "ldm_mesh_sdf: F = %d is %d chunks, above the 65535 of grid.y, with P = %lld "
                "below %lld", F, nchunk, (long long)P, (long long)kSplitBelow);
    hipStream_t st = (hipStream_t)s;
    MeshTri* tri = reinterpret_cast<MeshTri*>(ws);
    Partial* part = reinterpret_cast<Partial*>(reinterpret_cast<char*>(ws) + tri_bytes(F));
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    LDM_REQUIRE(e == hipSuccess, (int)e, "ldm_mesh_sdf: memset: %s", hipGetErrorString(e));
    if (F > 0)
        hipLaunchKernelGGL(mesh_pack_kernel, dim3((unsigned)((F + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, verts, V, faces, F, tri, flag);
    if (!split) {
        hipLaunchKernelGGL((mesh_eval_kernel<kPtsOnePass, false>), dim3((unsigned)blocks),
                           dim3(kThreads), 0, st, tri, F, points, P, sdf, closest, winding,
                           (Partial*)nullptr, 0);
        return launch_status("ldm_mesh_sdf");
    }
    const int stride = (int)min((int64_t)kSplitTile, P);
    for (int64_t p0 = 0; p0 < P; p0 += kSplitTile) {
        const int n = (int)min((int64_t)kSplitTile, P - p0);
        constexpr int per_split = kThreads * kPtsSplit;
        hipLaunchKernelGGL((mesh_eval_kernel<kPtsSplit, true>),
                           dim3((unsigned)((n + per_split - 1) / per_split), (unsigned)nchunk),
                           dim3(kThreads), 0, st, tri, F, points + p0 * 3, (int64_t)n,
                           (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, part, stride);
        hipLaunchKernelGGL(mesh_combine_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, part, nchunk, stride, n, sdf + p0,
                           closest ? closest + p0 : nullptr, winding ? winding + p0 : nullptr);
    }
    return launch_status("ldm_mesh_sdf");
}
