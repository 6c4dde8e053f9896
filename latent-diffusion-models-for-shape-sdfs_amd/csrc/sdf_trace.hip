// Sphere tracing of the decoder's field, the passes BETWEEN two decoder evaluations, MI355X
// (gfx950).  DESIGN.md §21.
//
// The marching loop is a host loop over rounds; every MLP evaluation of a round is one
// ldm_decoder_points_fwd launch over the whole batch, unchanged.  What this file adds:
//   init     per (shape, ray): the slab clip against the box, the walk to the first active brick
//            (ray_brick_dda.h), t / t_end / status / steps, the ray's "still marching" flag
//   step     per listed ray: the decoder value of its point -> hit, miss or a longer t (and the
//            walk through inactive bricks), the flag rewritten
//   compact  flag_compact.h with one segment per shape: the marching rays' indices in
//            ascending order and their number -- a pure function of the flags
//   emit     the next round's points o + t d as [B][P][3]; a shorter shape's padding slots
//            repeat its last listed point (a shape with none gets the box corner)
// Plain fp32 VALU and vector stores; no atomics, no workgroup waits on another; everything on
// the caller's stream.  The host reads the B counts once per round -- the loop's only
// synchronisation -- and that read is the caller's (ldm_sdf/render.py).
#include "flag_compact.h"
#include "ray_brick_dda.h"

namespace ldm {
namespace {

constexpr int kThreads = 256;

struct TraceWs {
    float* t_end;       // [B R]
    uint8_t* flags;     // [B R] 1: still marching
    FlagCompactWs scan; // the compaction's chunk sums and offsets, B segments of R flags
    size_t bytes;
};

TraceWs trace_ws_layout(int B, int64_t R, void* base) {
    const size_t n = (size_t)B * (size_t)R;
    TraceWs w{};
    char* b = reinterpret_cast<char*>(base);
    size_t o = 0;
    w.t_end = reinterpret_cast<float*>(b + o);
    o += up256(n * sizeof(float));
    w.flags = reinterpret_cast<uint8_t*>(b + o);
    o += up256(n);
    w.scan = flag_compact_ws(B, R, b + o);
    w.bytes = o + w.scan.bytes;
    return w;
}

struct Rays {
    const float* origins;
    const float* dirs;
    int64_t shape_stride;    // floats between two shapes' rays: 0 (shared) or 3 R
};

__device__ __forceinline__ rbd::Ray load_ray(const Rays& q, int b, int r) {
    const int64_t i = (int64_t)b * q.shape_stride + (int64_t)r * 3;
    rbd::Ray ray;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ray.o[a] = q.origins[i + a];
        ray.d[a] = q.dirs[i + a];
    }
    return ray;
}

struct Grid {
    const uint8_t* mask;     // [B nb^3] or nullptr
    int N, nb;
    float vs, origin;
};

__device__ __forceinline__ rbd::Bricks shape_bricks(const Grid& g, int b) {
    rbd::Bricks k;
    k.mask = g.mask ? g.mask + (size_t)b * g.nb * g.nb * g.nb : nullptr;
    k.N = g.N;
    k.nb = g.nb;
    k.vs = g.vs;
    k.origin = g.origin;
    return k;
}

__global__ __launch_bounds__(kThreads) void trace_init_kernel(
    Rays q, int B, int R, float lo, float hi, float t_min, float t_max, Grid g,
    float* __restrict__ t, float* __restrict__ t_end, int32_t* __restrict__ status,
    int32_t* __restrict__ steps, float* __restrict__ xyz_last, uint8_t* __restrict__ flags) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= (int64_t)B * R) return;
    const int b = (int)(s / R), r = (int)(s - (int64_t)b * R);
    const rbd::Ray ray = load_ray(q, b, r);
    float t0 = INFINITY, t1 = INFINITY;
    const int st = rbd::start(ray, shape_bricks(g, b), lo, hi, t_min, t_max, &t0, &t1);
    t[s] = st == rbd::kActive ? t0 : INFINITY;
    t_end[s] = t1;
    status[s] = st;
    steps[s] = 0;
    flags[s] = st == rbd::kActive ? 1 : 0;
    if (xyz_last) {
        const float qn = __builtin_nanf("");
        xyz_last[s * 3 + 0] = qn;
        xyz_last[s * 3 + 1] = qn;
        xyz_last[s * 3 + 2] = qn;
    }
}

// grid (ceil(P / 256), B): slot j of shape b is the ray list[b R + j], its value vals[b P + j]
__global__ __launch_bounds__(kThreads) void trace_step_kernel(
    Rays q, int R, int P, const float* __restrict__ vals, const int32_t* __restrict__ list,
    const int32_t* __restrict__ counts, float level, float lipschitz, float eps, Grid g,
    float* __restrict__ t, const float* __restrict__ t_end, int32_t* __restrict__ status,
    int32_t* __restrict__ steps, float* __restrict__ xyz_last, uint8_t* __restrict__ flags) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= P || j >= counts[b]) return;
    const int r = list[(int64_t)b * R + j];
    if ((unsigned)r >= (unsigned)R) return;                  // never read through a foreign list
    const int64_t s = (int64_t)b * R + r;
    const rbd::Ray ray = load_ray(q, b, r);
    float tt = t[s];
    if (xyz_last) {
        float p[3];
        rbd::point_at(ray, tt, p);
        xyz_last[s * 3 + 0] = p[0];
        xyz_last[s * 3 + 1] = p[1];
        xyz_last[s * 3 + 2] = p[2];
    }
    const int st = rbd::step(ray, shape_bricks(g, b), vals[(int64_t)b * P + j], level, lipschitz,
                             eps, t_end[s], &tt);
    steps[s] += 1;
    status[s] = st;
    flags[s] = st == rbd::kActive ? 1 : 0;
    t[s] = st == rbd::kMiss ? INFINITY : tt;
}

// grid (ceil(P / 256), B)
__global__ __launch_bounds__(kThreads) void trace_emit_kernel(
    Rays q, int R, int P, const float* __restrict__ t, const int32_t* __restrict__ list,
    const int32_t* __restrict__ counts, float lo, float* __restrict__ xyz) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= P) return;
    const int n = min(counts[b], R);
    float p[3] = {lo, lo, lo};
    if (n > 0) {
        const int r = min(max(list[(int64_t)b * R + min(j, n - 1)], 0), R - 1);
        rbd::point_at(load_ray(q, b, r), t[(int64_t)b * R + r], p);
    }
    float* dst = xyz + ((int64_t)b * P + j) * 3;
    dst[0] = p[0];
    dst[1] = p[1];
    dst[2] = p[2];
}

int check_dims(const char* what, int B, int64_t R) {
    LDM_REQUIRE(B >= 1, LDM_EINVAL, "%s: B = %d < 1", what, B);
    LDM_REQUIRE(R >= 1, LDM_EINVAL, "%s: R = %lld < 1", what, (long long)R);
    LDM_REQUIRE(R <= (int64_t)0x7fffffff / B, LDM_EINVAL,
                "%s: B * R = %d * %lld does not fit 31 bits", what, B, (long long)R);
    LDM_REQUIRE(flag_chunks(R) <= 65535 && B <= 65535, LDM_EINVAL,
                "%s: B = %d shapes or %lld chunks of rays exceed the 65535 of a grid axis", what,
                B, (long long)flag_chunks(R));
    return 0;
}

// mask != NULL: N >= 2 and B nb^3 < 2^31 as ldm_band_classify has them
int check_grid(const char* what, int B, const uint8_t* mask, int N, float vs, Grid* g) {
    g->mask = mask;
    g->N = N;
    g->nb = (N + rbd::kBrick - 1) / rbd::kBrick;
    g->vs = vs;
    if (!mask) return 0;
    LDM_REQUIRE(N >= 2, LDM_EINVAL, "%s: a brick mask needs N >= 2 (N = %d)", what, N);
    const int64_t nb = g->nb;
    LDM_REQUIRE(nb * nb * nb <= (int64_t)0x7fffffff / B, LDM_EINVAL,
                "%s: B * nb^3 = %d * %lld^3 does not fit 31 bits", what, B, (long long)nb);
    LDM_REQUIRE(vs > 0.f && vs < INFINITY, LDM_EINVAL, "%s: voxel size %g must be positive",
                what, (double)vs);
    return 0;
}

int check_march(const char* what, float level, float lipschitz, float eps) {
    LDM_REQUIRE(eps > 0.f && eps < INFINITY, LDM_EINVAL, "%s: eps = %g must be positive and "
                "finite", what, (double)eps);
    LDM_REQUIRE(lipschitz > 0.f && lipschitz < INFINITY, LDM_EINVAL,
                "%s: lipschitz = %g must be positive and finite", what, (double)lipschitz);
    LDM_REQUIRE(level == level, LDM_EINVAL, "%s: level is a NaN", what);
    return 0;
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" size_t ldm_sdf_trace_ws_bytes(int B, int64_t R) {
    if (B < 1 || R < 1 || R > (int64_t)0x7fffffff / B) return 0;
    return trace_ws_layout(B, R, nullptr).bytes;
}

extern "C" int ldm_sdf_trace_init(const float* origins, const float* dirs, int per_shape, int B,
                                  int64_t R, float lo, float hi, float t_min, float t_max,
                                  float level, float lipschitz, float eps, int max_steps,
                                  const uint8_t* mask, int N, float vs, float* t,
                                  int32_t* status, int32_t* steps, float* xyz_last,
                                  int32_t* list, int32_t* counts, void* ws, size_t ws_bytes,
                                  ldm_stream_t s) {
    const char* what = "ldm_sdf_trace_init";
    LDM_TRY(check_dims(what, B, R));
    LDM_REQUIRE(origins && dirs && t && status && steps && list && counts && ws, LDM_EINVAL,
                "%s: NULL origins / dirs / t / status / steps / list / counts / workspace", what);
    LDM_REQUIRE(lo < hi && hi - lo < INFINITY && lo - lo == 0.f, LDM_EINVAL,
                "%s: box [%g, %g] must be finite with lo < hi", what, (double)lo, (double)hi);
    LDM_REQUIRE(t_min <= t_max, LDM_EINVAL, "%s: t_min = %g, t_max = %g: need t_min <= t_max, "
                "neither a NaN", what, (double)t_min, (double)t_max);
    LDM_TRY(check_march(what, level, lipschitz, eps));
    LDM_REQUIRE(max_steps >= 1, LDM_EINVAL, "%s: max_steps = %d < 1", what, max_steps);
    Grid g{};
    LDM_TRY(check_grid(what, B, mask, N, vs, &g));
    g.origin = lo;
    LDM_REQUIRE(LDM_ALIGNED(origins, 4) && LDM_ALIGNED(dirs, 4) && LDM_ALIGNED(t, 4) &&
                    LDM_ALIGNED(status, 4) && LDM_ALIGNED(steps, 4) && LDM_ALIGNED(xyz_last, 4) &&
                    LDM_ALIGNED(list, 4) && LDM_ALIGNED(counts, 4) && LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "%s: tensors must be 4-B, the workspace 256-B aligned", what);
    const TraceWs w = trace_ws_layout(B, R, ws);
    LDM_REQUIRE(ws_bytes >= w.bytes, LDM_ENOSPC, "%s: workspace %zu < %zu B", what, ws_bytes,
                w.bytes);
    hipStream_t st = (hipStream_t)s;
    const Rays q{origins, dirs, per_shape ? 3 * R : 0};
    const int64_t n = (int64_t)B * R;
    hipLaunchKernelGGL(trace_init_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, q, B, (int)R, lo, hi, t_min, t_max, g, t, w.t_end,
                       status, steps, xyz_last, w.flags);
    flag_compact(w.flags, B, (int)R, w.scan, list, counts, st);
    return launch_status(what);
}

extern "C" int ldm_sdf_trace_emit(const float* origins, const float* dirs, int per_shape, int B,
                                  int64_t R, int P, float lo, const float* t,
                                  const int32_t* list, const int32_t* counts, float* xyz,
                                  ldm_stream_t s) {
    const char* what = "ldm_sdf_trace_emit";
    LDM_TRY(check_dims(what, B, R));
    LDM_REQUIRE(P >= 1 && P <= R, LDM_EINVAL, "%s: P = %d outside [1, R = %lld]", what, P,
                (long long)R);
    LDM_REQUIRE(origins && dirs && t && list && counts && xyz, LDM_EINVAL,
                "%s: NULL origins / dirs / t / list / counts / xyz", what);
    LDM_REQUIRE(lo - lo == 0.f, LDM_EINVAL, "%s: lo = %g is not finite", what, (double)lo);
    LDM_REQUIRE(LDM_ALIGNED(origins, 4) && LDM_ALIGNED(dirs, 4) && LDM_ALIGNED(t, 4) &&
                    LDM_ALIGNED(list, 4) && LDM_ALIGNED(counts, 4) && LDM_ALIGNED(xyz, 4),
                LDM_EALIGN, "%s: tensors must be 4-byte aligned", what);
    const Rays q{origins, dirs, per_shape ? 3 * R : 0};
    hipLaunchKernelGGL(trace_emit_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads), B),
                       dim3(kThreads), 0, (hipStream_t)s, q, (int)R, P, t, list, counts, lo, xyz);
    return launch_status(what);
}

extern "C" int ldm_sdf_trace_step(const float* origins, const float* dirs, int per_shape, int B,
                                  int64_t R, int P, const float* vals, float lo, float level,
                                  float lipschitz, float eps, const uint8_t* mask, int N,
                                  float vs, float* t, int32_t* status, int32_t* steps,
                                  float* xyz_last, int32_t* list, int32_t* counts, void* ws,
                                  size_t ws_bytes, ldm_stream_t s) {
    const char* what = "ldm_sdf_trace_step";
    LDM_TRY(check_dims(what, B, R));
    LDM_REQUIRE(P >= 1 && P <= R, LDM_EINVAL, "%s: P = %d outside [1, R = %lld]", what, P,
                (long long)R);
    LDM_REQUIRE(origins && dirs && vals && t && status && steps && list && counts && ws,
                LDM_EINVAL, "%s: NULL origins / dirs / vals / t / status / steps / list / counts "
                "/ workspace", what);
    LDM_REQUIRE(lo - lo == 0.f, LDM_EINVAL, "%s: lo = %g is not finite", what, (double)lo);
    LDM_TRY(check_march(what, level, lipschitz, eps));
    Grid g{};
    LDM_TRY(check_grid(what, B, mask, N, vs, &g));
    g.origin = lo;
    LDM_REQUIRE(LDM_ALIGNED(origins, 4) && LDM_ALIGNED(dirs, 4) && LDM_ALIGNED(vals, 4) &&
                    LDM_ALIGNED(t, 4) && LDM_ALIGNED(status, 4) && LDM_ALIGNED(steps, 4) &&
                    LDM_ALIGNED(xyz_last, 4) && LDM_ALIGNED(list, 4) && LDM_ALIGNED(counts, 4) &&
                    LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "%s: tensors must be 4-B, the workspace 256-B aligned", what);
    const TraceWs w = trace_ws_layout(B, R, ws);
    LDM_REQUIRE(ws_bytes >= w.bytes, LDM_ENOSPC, "%s: workspace %zu < %zu B", what, ws_bytes,
                w.bytes);
    hipStream_t st = (hipStream_t)s;
    const Rays q{origins, dirs, per_shape ? 3 * R : 0};
    hipLaunchKernelGGL(trace_step_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads), B),
                       dim3(kThreads), 0, st, q, (int)R, P, vals, list, counts, level, lipschitz,
                       eps, g, t, w.t_end, status, steps, xyz_last, w.flags);
    flag_compact(w.flags, B, (int)R, w.scan, list, counts, st);
    return launch_status(what);
}
