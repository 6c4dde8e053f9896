// Signed distance from query points to a triangle soup, MI355X (gfx950).  DESIGN.md §16.
//
// The first stage of the path: DeepSDF's SdfSamples are made from raw meshes by evaluating
// 500 000 points against every triangle -- no acceleration structure, no approximation.  Per
// point: the distance to the closest triangle, that triangle's index (ties to the smaller
// index) and the generalized winding number, whose comparison with 0.5 gives the sign on
// meshes that are not watertight.  The pair arithmetic is mesh_sdf_pair.h.
//
// Kernels (all fp32 VALU; no float atomics):
//   pack     one thread per face: the face loaded by soup_load_face (indices clamped to
//            [0, V), a clamp raises *flag), the record MeshTri written to the workspace
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
// the same alone or among a million others.  The switch between the forms, the workspace and the
// argument checks are soup_plan.h's, shared with ray_mesh.hip.
#include "soup_plan.h"
#include "mesh_sdf_pair.h"

namespace ldm {
namespace {

constexpr int kFaceChunk = 1024;       // faces per chunk: the summation shape
constexpr int64_t kSplitBelow = 16384; // P below this (and > 1 chunk): split over chunks
constexpr int kSplitTile = 4096;       // points per workspace tile of the split form
constexpr int kThreads = 256;
static_assert(kSplitTile % kThreads == 0, "a tile is whole workgroups");
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
    float p[3][3];
    soup_load_face(verts, V, faces, f, flag, p);
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
// One point per thread: two and four measured slower (DESIGN.md §16,
// profiles/mesh_sdf/points_per_thread_*.json).
template <bool SPLIT>
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
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t ic = min(i, n - 1);                    // past the end: clamped
    const float px = pts[ic * 3 + 0], py = pts[ic * 3 + 1], pz = pts[ic * 3 + 2];
    float sum = 0.0f, best = INFINITY;
    int32_t bface = -1;
    const int nchunk = (F + kFaceChunk - 1) / kFaceChunk;
    const int c_begin = SPLIT ? (int)blockIdx.y : 0;
    const int c_end = SPLIT ? c_begin + 1 : nchunk;
    for (int c = c_begin; c < c_end; ++c) {
        const int f0 = c * kFaceChunk, f1 = min(f0 + kFaceChunk, F);
        float cs = 0.0f;
        for (int f = f0; f < f1; ++f) {
            const MeshTri T = tri[f];                    // wave-uniform: scalar loads
            float d2, h;
            pair_eval(T, px, py, pz, &d2, &h);
            cs = cs + h;
            const bool lt = d2 < best;                   // strict: the smaller index keeps a tie
            best = lt ? d2 : best;
            bface = lt ? f : bface;
        }
        sum = SPLIT ? cs : sum + cs;
    }
    if (i >= n) return;
    if (SPLIT) {
        Partial o;
        o.sum = sum;
        o.d2 = best;
        o.face = bface;
        o.pad = 0;
        part[(int64_t)blockIdx.y * tile_stride + i] = o;
    } else {
        mesh_finish(sum, best, bface, i, sdf, closest, winding);
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

SoupPlan mesh_plan(int F, int64_t P) {
    return soup_plan(kFaceChunk, kSplitBelow, kSplitTile, sizeof(MeshTri), sizeof(Partial), F, P);
}

}  // namespace
}  // namespace ldm

extern "C" int ldm_mesh_sdf_face_chunk(void) { return ldm::kFaceChunk; }
extern "C" int64_t ldm_mesh_sdf_split_below(void) { return ldm::kSplitBelow; }

extern "C" size_t ldm_mesh_sdf_ws_bytes(int F, int64_t P) {
    return F < 0 || P < 0 ? 0 : ldm::mesh_plan(F, P).ws_bytes;
}

extern "C" int ldm_mesh_sdf(const float* verts, int V, const int32_t* faces, int F,
                            const float* points, int64_t P, float* sdf, int32_t* closest,
                            float* winding, int32_t* flag, void* ws, size_t ws_bytes,
                            ldm_stream_t s) {
    using namespace ldm;
    const SoupPlan plan = mesh_plan(F, P);
    LDM_TRY(soup_check_args(
        "ldm_mesh_sdf", 'P', plan, V, verts, faces, points && sdf && flag && ws,
        "points / sdf / flag / workspace",
        LDM_ALIGNED(points, 4) && LDM_ALIGNED(sdf, 4) && LDM_ALIGNED(closest, 4) &&
            LDM_ALIGNED(winding, 4) && LDM_ALIGNED(flag, 4) && LDM_ALIGNED(verts, 4) &&
            LDM_ALIGNED(faces, 4) && LDM_ALIGNED(ws, 256),
        ws_bytes));
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)s;
    MeshTri* tri = reinterpret_cast<MeshTri*>(ws);
    Partial* part = reinterpret_cast<Partial*>(reinterpret_cast<char*>(ws) + plan.tri_bytes);
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    LDM_REQUIRE(e == hipSuccess, (int)e, "ldm_mesh_sdf: memset: %s", hipGetErrorString(e));
    if (F > 0)
        hipLaunchKernelGGL(mesh_pack_kernel, dim3((unsigned)((F + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, verts, V, faces, F, tri, flag);
    if (!plan.split) {
        hipLaunchKernelGGL(mesh_eval_kernel<false>, dim3((unsigned)plan.blocks), dim3(kThreads), 0,
                           st, tri, F, points, P, sdf, closest, winding, (Partial*)nullptr, 0);
        return launch_status("ldm_mesh_sdf");
    }
    for (int64_t p0 = 0; p0 < P; p0 += kSplitTile) {
        const int n = (int)min((int64_t)kSplitTile, P - p0);
        const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(mesh_eval_kernel<true>, dim3(gx, (unsigned)plan.nchunk), dim3(kThreads),
                           0, st, tri, F, points + p0 * 3, (int64_t)n, (float*)nullptr,
                           (int32_t*)nullptr, (float*)nullptr, part, plan.tile_stride);
        hipLaunchKernelGGL(mesh_combine_kernel, dim3(gx), dim3(kThreads), 0, st, part, plan.nchunk,
                           plan.tile_stride, n, sdf + p0, closest ? closest + p0 : nullptr,
                           winding ? winding + p0 : nullptr);
    }
    return launch_status("ldm_mesh_sdf");
}
