// Closest intersection of many rays with a triangle soup, MI355X (gfx950).  DESIGN.md §19.
//
// The sibling of mesh_sdf.hip, with which it shares soup_plan.h (the face loader, the switch
// between the launch forms, the workspace, the argument checks): every ray against every face,
// no acceleration structure.  Per
// ray: the smallest t in [t_min, t_max] with o + t d on a triangle, that triangle's index
// (ties to the smaller index) and the barycentric weights of the hit.  The pair arithmetic is
// the watertight test of ray_tri_pair.h.
//
// Kernels (all fp32 VALU; no LDS, no barrier, no float atomics):
//   pack     one thread per face: the face loaded by soup_load_face (indices clamped to
//            [0, V), a clamp raises *flag), the 48-byte record RayTri written to the workspace
//   trace    256 threads, one ray per thread held in registers.  The triangle record is read
//            at a wave-uniform address (loop counter + blockIdx only): the compiler turns that
//            into scalar loads, and the record feeds the VALU from SGPRs.  The axis
//            permutation is applied by per-lane selects.  T, the division and the range test
//            sit under a wave-uniform "some lane is inside this triangle" branch.
//   combine  split form only: the minimum over the per-chunk partials of one ray
//
// The result is the lexicographic minimum of (t, face) over the hits, which no order can
// change; faces are walked in ascending order and a later face wins only by a strictly smaller
// t.  The weights are not carried through the loop: ray_finish runs the pair once more on the
// winning face (the same operations on the same inputs) and divides there.
//   one-pass form  (R >= kSplitBelow or one chunk)  a thread walks every face
//   split form     (R <  kSplitBelow)  grid.y = chunks of kFaceChunk faces, partials (t, face)
//                  to the workspace per tile of kSplitTile rays, then combine
// Both forms give a ray bitwise the same outputs, alone or among a million others.
#include "soup_plan.h"
#include "ray_tri_pair.h"

namespace ldm {
namespace {

constexpr int kFaceChunk = 1024;          // faces per workgroup of the split form
constexpr int64_t kSplitBelow = 1 << 20;  // R below this (and > 1 chunk): split over chunks
constexpr int kSplitTile = 16384;         // rays per workspace tile of the split form
constexpr int kThreads = 256;
static_assert(kSplitTile % kThreads == 0, "a tile is whole workgroups");
static_assert(sizeof(RayTri) == 48, "RayTri: three 16-byte vectors");

struct alignas(8) Partial {
    float t;        // smallest t of the chunk's hits, +inf for none
    int32_t face;   // its face (the smallest index on a tie), -1 for none
};

__global__ __launch_bounds__(kThreads) void ray_pack_kernel(const float* __restrict__ verts,
                                                            int V,
                                                            const int32_t* __restrict__ faces,
                                                            int F, RayTri* __restrict__ tri,
                                                            int32_t* __restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    float p[3][3];
    soup_load_face(verts, V, faces, f, flag, p);
    RayTri T;
    T.ax = p[0][0]; T.ay = p[0][1]; T.az = p[0][2];
    T.bx = p[1][0]; T.by = p[1][1]; T.bz = p[1][2];
    T.cx = p[2][0]; T.cy = p[2][1]; T.cz = p[2][2];
    T.p0 = T.p1 = T.p2 = 0.0f;
    tri[f] = T;
}

__device__ __forceinline__ RayPre ray_load(const float* __restrict__ origins,
                                           const float* __restrict__ dirs, int64_t i) {
    return ray_setup(origins[i * 3 + 0], origins[i * 3 + 1], origins[i * 3 + 2],
                     dirs[i * 3 + 0], dirs[i * 3 + 1], dirs[i * 3 + 2]);
}

// the one place a ray's outputs are formed from (t, face)
__device__ __forceinline__ void ray_finish(const RayTri* __restrict__ tri, const RayPre& r,
                                           float t_min, float t_max, float best, int32_t bface,
                                           int64_t i, float* __restrict__ t_out,
                                           int32_t* __restrict__ face_out,
                                           float* __restrict__ bary_out) {
    t_out[i] = best;
    if (face_out) face_out[i] = bface;
    if (bary_out) {
        float w[3] = {0.0f, 0.0f, 0.0f}, t;
        if (bface >= 0) ray_tri_pair(tri[bface], r, t_min, t_max, &t, w);
        bary_out[i * 3 + 0] = w[0];
        bary_out[i * 3 + 1] = w[1];
        bary_out[i * 3 + 2] = w[2];
    }
}

// Faces [f0, f1) against the thread's ray.  The axis permutation is the ray's own: per-lane
// selects.  Loops compiled for a wave-uniform (kz, sign) measured slower.
__device__ __forceinline__ void trace_faces(const RayTri* __restrict__ tri, int f0, int f1,
                                            const RayPre& r, float t_min, float t_max,
                                            float& best, int32_t& bface) {
#pragma clang fp contract(off)
    for (int f = f0; f < f1; ++f) {
        const RayTri T = tri[f];                         // wave-uniform: scalar loads
        float U, V, W, det, Ak, Bk, Ck;
        const bool cand = ray_tri_edges(T, r.ox, r.oy, r.oz, r.Sx, r.Sy, r.kx, r.ky, r.kz, &U,
                                        &V, &W, &det, &Ak, &Bk, &Ck);
        if (__any(cand)) {                               // wave-uniform branch
            const float t = ray_tri_t(U, V, W, det, r.Sz, Ak, Bk, Ck);
            // strict: the smaller index keeps a tie
            const bool hit = cand && t >= t_min && t <= t_max && t < best;
            best = hit ? t : best;
            bface = hit ? f : bface;
        }
    }
}

// SPLIT: blockIdx.y is the chunk, `part` takes [chunk][tile ray]; else every face is walked
// and the outputs are written.  origins / dirs / outputs / `part` are those of the tile, n its
// rays.
template <bool SPLIT>
__global__ __launch_bounds__(kThreads) void ray_trace_kernel(const RayTri* __restrict__ tri,
                                                             int F,
                                                             const float* __restrict__ origins,
                                                             const float* __restrict__ dirs,
                                                             int64_t n, float t_min, float t_max,
                                                             float* __restrict__ t_out,
                                                             int32_t* __restrict__ face_out,
                                                             float* __restrict__ bary_out,
                                                             Partial* __restrict__ part,
                                                             int tile_stride) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const RayPre r = ray_load(origins, dirs, min(i, n - 1));      // past the end: clamped
    const int f0 = SPLIT ? (int)blockIdx.y * kFaceChunk : 0;
    const int f1 = SPLIT ? min(f0 + kFaceChunk, F) : F;
    float best = INFINITY;
    int32_t bface = -1;
    trace_faces(tri, f0, f1, r, t_min, t_max, best, bface);
    if (!r.ok) {                                         // such a ray misses everything
        best = INFINITY;
        bface = -1;
    }
    if (i >= n) return;
    if (SPLIT) {
        Partial o;
        o.t = best;
        o.face = bface;
        part[(int64_t)blockIdx.y * tile_stride + i] = o;
    } else {
        ray_finish(tri, r, t_min, t_max, best, bface, i, t_out, face_out, bary_out);
    }
}

__global__ __launch_bounds__(kThreads) void ray_combine_kernel(
    const Partial* __restrict__ part, int nchunk, int tile_stride, const RayTri* __restrict__ tri,
    const float* __restrict__ origins, const float* __restrict__ dirs, int n, float t_min,
    float t_max, float* __restrict__ t_out, int32_t* __restrict__ face_out,
    float* __restrict__ bary_out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float best = INFINITY;
    int32_t bface = -1;
    for (int c = 0; c < nchunk; ++c) {
        const Partial p = part[(int64_t)c * tile_stride + i];
        const bool lt = p.t < best;                      // chunks ascend: so do the indices
        best = lt ? p.t : best;
        bface = lt ? p.face : bface;
    }
    const RayPre r = ray_load(origins, dirs, i);
    ray_finish(tri, r, t_min, t_max, best, bface, i, t_out, face_out, bary_out);
}

SoupPlan ray_plan(int F, int64_t R) {
    return soup_plan(kFaceChunk, kSplitBelow, kSplitTile, sizeof(RayTri), sizeof(Partial), F, R);
}

}  // namespace
}  // namespace ldm

extern "C" int ldm_ray_mesh_face_chunk(void) { return ldm::kFaceChunk; }
extern "C" int64_t ldm_ray_mesh_split_below(void) { return ldm::kSplitBelow; }

extern "C" size_t ldm_ray_mesh_ws_bytes(int F, int64_t R) {
    return F < 0 || R < 0 ? 0 : ldm::ray_plan(F, R).ws_bytes;
}

extern "C" int ldm_ray_mesh(const float* verts, int V, const int32_t* faces, int F,
                            const float* origins, const float* dirs, int64_t R, float t_min,
                            float t_max, float* t_out, int32_t* face_out, float* bary_out,
                            int32_t* flag, void* ws, size_t ws_bytes, ldm_stream_t s) {
    using namespace ldm;
    // the range comes second: a negative size is left to soup_check_args, which reports it first
    LDM_REQUIRE(V < 0 || F < 0 || R < 0 || t_min <= t_max, LDM_EINVAL,
                "ldm_ray_mesh: t_min = %g, t_max = %g: need t_min <= t_max, neither a NaN",
                (double)t_min, (double)t_max);
    const SoupPlan plan = ray_plan(F, R);
    LDM_TRY(soup_check_args(
        "ldm_ray_mesh", 'R', plan, V, verts, faces, origins && dirs && t_out && flag && ws,
        "origins / dirs / t_out / flag / workspace",
        LDM_ALIGNED(origins, 4) && LDM_ALIGNED(dirs, 4) && LDM_ALIGNED(t_out, 4) &&
            LDM_ALIGNED(face_out, 4) && LDM_ALIGNED(bary_out, 4) && LDM_ALIGNED(flag, 4) &&
            LDM_ALIGNED(verts, 4) && LDM_ALIGNED(faces, 4) && LDM_ALIGNED(ws, 256),
        ws_bytes));
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)s;
    RayTri* tri = reinterpret_cast<RayTri*>(ws);
    Partial* part = reinterpret_cast<Partial*>(reinterpret_cast<char*>(ws) + plan.tri_bytes);
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), st);
    LDM_REQUIRE(e == hipSuccess, (int)e, "ldm_ray_mesh: memset: %s", hipGetErrorString(e));
    if (F > 0)
        hipLaunchKernelGGL(ray_pack_kernel, dim3((unsigned)((F + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, verts, V, faces, F, tri, flag);
    if (!plan.split) {
        hipLaunchKernelGGL((ray_trace_kernel<false>), dim3((unsigned)plan.blocks), dim3(kThreads),
                           0, st, tri, F, origins, dirs, R, t_min, t_max, t_out, face_out,
                           bary_out, (Partial*)nullptr, 0);
        return launch_status("ldm_ray_mesh");
    }
    for (int64_t r0 = 0; r0 < R; r0 += kSplitTile) {
        const int n = (int)min((int64_t)kSplitTile, R - r0);
        const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
        hipLaunchKernelGGL((ray_trace_kernel<true>), dim3(gx, (unsigned)plan.nchunk),
                           dim3(kThreads), 0, st, tri, F, origins + r0 * 3, dirs + r0 * 3,
                           (int64_t)n, t_min, t_max, (float*)nullptr, (int32_t*)nullptr,
                           (float*)nullptr, part, plan.tile_stride);
        hipLaunchKernelGGL(ray_combine_kernel, dim3(gx), dim3(kThreads), 0, st, part, plan.nchunk,
                           plan.tile_stride, tri, origins + r0 * 3, dirs + r0 * 3, n, t_min, t_max,
                           t_out + r0, face_out ? face_out + r0 : nullptr,
                           bary_out ? bary_out + r0 * 3 : nullptr);
    }
    return launch_status("ldm_ray_mesh");
}
