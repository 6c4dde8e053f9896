// Nearest points and Chamfer distances between point clouds, MI355X (gfx950).  DESIGN.md §17.
//
// The last stage of the path: is a reconstructed or generated shape any good.  DeepSDF reports
// the Chamfer distance between 30 000 surface points of two meshes; generation papers report
// MMD / COV / 1-NNA, which need the Chamfer distance between every generated and every reference
// cloud.  Every point pair is evaluated, no acceleration structure:
//   D(a -> b) = (1/n) sum_i min_j |a_i - b_j|^2        (squared distances)
//
// Pair arithmetic (fixed IEEE sequence, contraction off): dx = a.x - b.x, dy, dz formed first,
// d = dx*dx, d = fma(dy, dy, d), d = fma(dz, dz, d).  The expansion |a|^2 + |b|^2 - 2 a.b is
// not used: it cancels exactly where the metric lives (the lever not pulled).
//
// Kernels (all fp32 VALU, the sums fp64; no float atomics):
//   min      256 threads, kPts points of the first cloud per thread in registers.  The second
//            cloud is read at a wave-uniform address (loop counter + blockIdx only): scalar
//            loads, the coordinates feed the VALU from SGPRs.  Two points of it per 3-input
//            min; with IDX the index of the minimum is tracked (strict <, ascending index: the
//            lexicographic minimum of (d^2, index)), which costs a compare and two selects per
//            pair, so it is a template flag.
//   combine  split form only: the minimum over the per-split partials, ascending
//   batch    one workgroup per matrix entry (s, r): walks the tiles of a_s, every tile against
//            all of b_r, and adds the minima in fp64
//   reduce   spread form only: the same fp64 sum over minima the min kernel left in memory
//
// A minimum is exact and no order changes it, so how the second cloud is cut over workgroups is
// free.  The fp64 sum of the n minima has one shape, fixed by n and kTileA / kThreads alone
// (tile_sum below, then the tiles in ascending order), used by batch and reduce alike: out[s, r]
// is bitwise the same in either form, at any position of any batch.
#include "ldm_internal.h"

namespace ldm {
namespace {

#ifndef LDM_CHAMFER_PTS
#define LDM_CHAMFER_PTS 4
#endif
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// points of the first cloud per thread.  2 / 4 / 8 were timed (development
// builds with -DLDM_CHAMFER_PTS): 4 it is
constexpr int kPts = LDM_CHAMFER_PTS;
constexpr int kTileA = kThreads * kPts;        // points of the first cloud per workgroup tile
constexpr int kChunkB = 1024;                  // points of the second cloud per split unit
constexpr int kUnroll = 8;                     // second-cloud points per trip of the main loop
constexpr int kMaxSplit = 64;                  // most workgroups along the second cloud
constexpr int64_t kSplitBelow = 262144;        // P below this (and > 1 chunk): split form
constexpr int kSplitTile = 16384;              // points per workspace tile of the split form
constexpr int64_t kSpreadBelow = 256;          // S * R below this (and n > kTileA): spread form
constexpr int64_t kSpreadTile = kSplitBelow;   // minima kept in memory per pass of the spread form
static_assert(kSplitTile % kTileA == 0 && kSpreadTile % kTileA == 0, "tiles are whole workgroups");
static_assert(kChunkB % kUnroll == 0 && kUnroll % 2 == 0, "two points per 3-input min");

struct alignas(8) Partial {
    float d2;      // smallest squared distance in the split's range of the second cloud
    int32_t idx;   // its index (the smallest on a tie)
};

// the pair: the differences first, then a product and two fused multiply-adds
__device__ __forceinline__ float pair_d2(float ax, float ay, float az, float bx, float by,
                                         float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float d = dx * dx;
    d = __builtin_fmaf(dy, dy, d);
    d = __builtin_fmaf(dz, dz, d);
    return d;
}

// kPts points per thread against c[j0, j1): best / bidx are updated.  c is wave-uniform.
template <bool IDX>
__device__ __forceinline__ void walk(const float* __restrict__ c, int j0, int j1,
                                     const float (&px)[kPts], const float (&py)[kPts],
                                     const float (&pz)[kPts], float (&best)[kPts],
                                     int32_t (&bidx)[kPts]) {
#pragma clang fp contract(off)
    int j = j0;
    for (; j + kUnroll <= j1; j += kUnroll) {
        float b[3 * kUnroll];
#pragma unroll
        for (int u = 0; u < 3 * kUnroll; ++u) b[u] = c[(int64_t)j * 3 + u];
#pragma unroll
        for (int u = 0; u < kUnroll; u += 2) {
#pragma unroll
            for (int k = 0; k < kPts; ++k) {
                const float d0 = pair_d2(px[k], py[k], pz[k], b[3 * u], b[3 * u + 1], b[3 * u + 2]);
                const float d1 =
                    pair_d2(px[k], py[k], pz[k], b[3 * u + 3], b[3 * u + 4], b[3 * u + 5]);
                if (IDX) {
                    const bool l0 = d0 < best[k];            // strict: the smaller index keeps a tie
                    best[k] = l0 ? d0 : best[k];
                    bidx[k] = l0 ? j + u : bidx[k];
                    const bool l1 = d1 < best[k];
                    best[k] = l1 ? d1 : best[k];
                    bidx[k] = l1 ? j + u + 1 : bidx[k];
                } else {
                    best[k] = __builtin_fminf(__builtin_fminf(best[k], d0), d1);   // v_min3_f32
                }
            }
        }
    }
    for (; j < j1; ++j) {
        const float bx = c[(int64_t)j * 3], by = c[(int64_t)j * 3 + 1], bz = c[(int64_t)j * 3 + 2];
#pragma unroll
        for (int k = 0; k < kPts; ++k) {
            const float d = pair_d2(px[k], py[k], pz[k], bx, by, bz);
            if (IDX) {
                const bool lt = d < best[k];
                best[k] = lt ? d : best[k];
                bidx[k] = lt ? j : bidx[k];
            } else {
                best[k] = __builtin_fminf(best[k], d);
            }
        }
    }
}

// a tile's points: thread t holds points base + t + k * kThreads (past the end: clamped)
__device__ __forceinline__ void load_tile(const float* __restrict__ q, int64_t base, int64_t n,
                                          float (&px)[kPts], float (&py)[kPts],
                                          float (&pz)[kPts], float (&best)[kPts],
                                          int32_t (&bidx)[kPts]) {
#pragma unroll
    for (int k = 0; k < kPts; ++k) {
        const int64_t i = min(base + threadIdx.x + (int64_t)k * kThreads, n - 1);
        px[k] = q[i * 3 + 0];
        py[k] = q[i * 3 + 1];
        pz[k] = q[i * 3 + 2];
        best[k] = INFINITY;
        bidx[k] = -1;
    }
}

// SPLIT: blockIdx.y walks chunks [y * cps, (y + 1) * cps) of c and `part` takes
// [split][tile point]; else all of c is walked and d2 / idx are written.  q / d2 / idx / part
// are those of the launch's points, n of them.
template <bool IDX, bool SPLIT>
__global__ __launch_bounds__(kThreads) void chamfer_min_kernel(const float* __restrict__ q,
                                                               int64_t n,
                                                               const float* __restrict__ c, int Q,
                                                               int cps, float* __restrict__ d2,
                                                               int32_t* __restrict__ idx,
                                                               Partial* __restrict__ part,
                                                               int tile_stride) {
    const int64_t base = (int64_t)blockIdx.x * kTileA;
    float px[kPts], py[kPts], pz[kPts], best[kPts];
    int32_t bidx[kPts];
    load_tile(q, base, n, px, py, pz, best, bidx);
    int j0 = 0, j1 = Q;
    if (SPLIT) {
        j0 = (int)min((int64_t)blockIdx.y * cps * kChunkB, (int64_t)Q);
        j1 = (int)min((int64_t)j0 + (int64_t)cps * kChunkB, (int64_t)Q);
    }
    walk<IDX>(c, j0, j1, px, py, pz, best, bidx);
#pragma unroll
    for (int k = 0; k < kPts; ++k) {
        const int64_t i = base + threadIdx.x + (int64_t)k * kThreads;
        if (i >= n) continue;
        if (SPLIT) {
            Partial o;
            o.d2 = best[k];
            o.idx = bidx[k];
            part[(int64_t)blockIdx.y * tile_stride + i] = o;
        } else {
            d2[i] = best[k];
            if (IDX) idx[i] = bidx[k];
        }
    }
}

__global__ __launch_bounds__(kThreads) void chamfer_combine_kernel(
    const Partial* __restrict__ part, int nsplit, int tile_stride, int n, float* __restrict__ d2,
    int32_t* __restrict__ idx) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float best = INFINITY;
    int32_t bidx = -1;
    for (int s = 0; s < nsplit; ++s) {
        const Partial p = part[(int64_t)s * tile_stride + i];
        const bool lt = p.d2 < best;                         // splits ascend: so do the indices
        best = lt ? p.d2 : best;
        bidx = lt ? p.idx : bidx;
    }
    d2[i] = best;
    if (idx) idx[i] = bidx;
}

// The one place a tile's kTileA minima are added.  Thread t: its kPts values in order; a wave:
// the shuffle tree 32, 16, .. 1; the workgroup: the waves in order.  All in fp64.  Every thread
// calls it; the sum is returned in thread 0 (other threads: unspecified).
__device__ __forceinline__ double tile_sum(const double (&v)[kPts], double* lds) {
    double x = v[0];
#pragma unroll
    for (int k = 1; k < kPts; ++k) x = x + v[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    __syncthreads();                                         // lds free from the last tile
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t = t + lds[w];
    return t;
}

// one workgroup per entry: blockIdx.x = s * R + r
__global__ __launch_bounds__(kThreads) void chamfer_batch_kernel(const float* __restrict__ a,
                                                                 int n,
                                                                 const float* __restrict__ b,
                                                                 int R, int m,
                                                                 float* __restrict__ out) {
    __shared__ double lds[kWaves];
    const int64_t s = blockIdx.x / (unsigned)R, r = blockIdx.x % (unsigned)R;
    const float* __restrict__ as = a + s * n * 3;
    const float* __restrict__ br = b + r * m * 3;
    double acc = 0.0;
    for (int64_t base = 0; base < n; base += kTileA) {
        float px[kPts], py[kPts], pz[kPts], best[kPts];
        int32_t bidx[kPts];
        load_tile(as, base, n, px, py, pz, best, bidx);
        walk<false>(br, 0, m, px, py, pz, best, bidx);
        double v[kPts];
#pragma unroll
        for (int k = 0; k < kPts; ++k)
            v[k] = base + threadIdx.x + (int64_t)k * kThreads < n ? (double)best[k] : 0.0;
        acc = acc + tile_sum(v, lds);
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(acc / (double)n);
}

// spread form: adds the np minima of one pass (np a multiple of kTileA but for the last pass)
// to *acc in tile order; first: the sum starts at 0; last: out = fl32(sum / n)
__global__ __launch_bounds__(kThreads) void chamfer_reduce_kernel(const float* __restrict__ d2,
                                                                  int np, int first, int last,
                                                                  int64_t n,
                                                                  double* __restrict__ acc_io,
                                                                  float* __restrict__ out) {
    __shared__ double lds[kWaves];
    double acc = first ? 0.0 : *acc_io;
    for (int base = 0; base < np; base += kTileA) {
        double v[kPts];
#pragma unroll
        for (int k = 0; k < kPts; ++k) {
            const int i = base + threadIdx.x + k * kThreads;
            v[k] = i < np ? (double)d2[i] : 0.0;
        }
        acc = acc + tile_sum(v, lds);
    }
    if (threadIdx.x == 0) {
        if (last) *out = (float)(acc / (double)n);
        else *acc_io = acc;
    }
}

inline int64_t n_chunks(int64_t Q) { return (Q + kChunkB - 1) / kChunkB; }
inline bool use_split(int64_t P, int64_t Q) { return P < kSplitBelow && n_chunks(Q) > 1; }
inline int n_split(int64_t Q) { return (int)min(n_chunks(Q), (int64_t)kMaxSplit); }
inline size_t part_bytes(int64_t P, int64_t Q) {
    if (!use_split(P, Q)) return 0;
    return up256((size_t)n_split(Q) * (size_t)min((int64_t)kSplitTile, P) * sizeof(Partial));
}
inline bool use_spread(int64_t S, int64_t n, int64_t R) {
    return n > kTileA && S * R < kSpreadBelow;   // S, R <= 2^31 - 1: no overflow
}
constexpr int64_t kMaxCount = 0x7fffffff;

// the launches of ldm_nearest_points; the arguments have been checked
int nearest_launch(const float* q, int64_t P, const float* c, int Q, float* d2, int32_t* idx,
                   void* part_ws, hipStream_t st) {
    const bool want_idx = idx != nullptr;
    if (!use_split(P, Q)) {
        const dim3 grid((unsigned)((P + kTileA - 1) / kTileA));
        if (want_idx)
            hipLaunchKernelGGL((chamfer_min_kernel<true, false>), grid, dim3(kThreads), 0, st, q,
                               P, c, Q, 0, d2, idx, (Partial*)nullptr, 0);
        else
            hipLaunchKernelGGL((chamfer_min_kernel<false, false>), grid, dim3(kThreads), 0, st, q,
                               P, c, Q, 0, d2, idx, (Partial*)nullptr, 0);
        return 0;
    }
    Partial* part = reinterpret_cast<Partial*>(part_ws);
    const int nsplit = n_split(Q);
    const int cps = (int)((n_chunks(Q) + nsplit - 1) / nsplit);
    const int stride = (int)min((int64_t)kSplitTile, P);
    for (int64_t p0 = 0; p0 < P; p0 += kSplitTile) {
        const int n = (int)min((int64_t)kSplitTile, P - p0);
        const dim3 grid((unsigned)((n + kTileA - 1) / kTileA), (unsigned)nsplit);
        if (want_idx)
            hipLaunchKernelGGL((chamfer_min_kernel<true, true>), grid, dim3(kThreads), 0, st,
                               q + p0 * 3, (int64_t)n, c, Q, cps, (float*)nullptr,
                               (int32_t*)nullptr, part, stride);
        else
            hipLaunchKernelGGL((chamfer_min_kernel<false, true>), grid, dim3(kThreads), 0, st,
                               q + p0 * 3, (int64_t)n, c, Q, cps, (float*)nullptr,
                               (int32_t*)nullptr, part, stride);
        hipLaunchKernelGGL(chamfer_combine_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, st, part, nsplit, stride, n, d2 + p0,
                           want_idx ? idx + p0 : nullptr);
    }
    return 0;
}

}  // namespace
}  // namespace ldm

extern "C" int ldm_chamfer_tile_a(void) { return ldm::kTileA; }
extern "C" int ldm_chamfer_chunk_b(void) { return ldm::kChunkB; }
extern "C" int64_t ldm_chamfer_split_below(void) { return ldm::kSplitBelow; }
extern "C" int64_t ldm_chamfer_spread_below(void) { return ldm::kSpreadBelow; }

extern "C" size_t ldm_nearest_points_ws_bytes(int64_t P, int64_t Q) {
    using namespace ldm;
    if (P < 0 || Q < 0) return 0;
    return 256 + part_bytes(P, Q);
}

extern "C" int ldm_nearest_points(const float* q, int64_t P, const float* c, int64_t Q,
                                  float* d2, int32_t* idx, void* ws, size_t ws_bytes,
                                  ldm_stream_t s) {
    using namespace ldm;
    LDM_REQUIRE(P >= 0 && Q >= 0, LDM_EINVAL, "ldm_nearest_points: negative count (P = %lld, "
                "Q = %lld)", (long long)P, (long long)Q);
    if (P == 0) return 0;
    LDM_REQUIRE(Q > 0, LDM_EINVAL, "ldm_nearest_points: %lld points against an empty cloud",
                (long long)P);
    LDM_REQUIRE(q && c && d2 && ws, LDM_EINVAL,
                "ldm_nearest_points: NULL query / cloud / d2 / workspace");
    LDM_REQUIRE(LDM_ALIGNED(q, 4) && LDM_ALIGNED(c, 4) && LDM_ALIGNED(d2, 4) &&
                    LDM_ALIGNED(idx, 4) && LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "ldm_nearest_points: tensors must be 4-B, the workspace 256-B aligned");
    LDM_REQUIRE(Q <= kMaxCount, LDM_EINVAL,
                "ldm_nearest_points: Q = %lld is above the 2^31 - 1 an int32 index reaches",
                (long long)Q);
    LDM_REQUIRE(P <= kMaxCount * (int64_t)kTileA, LDM_EINVAL,
                "ldm_nearest_points: P = %lld needs more than 2^31 - 1 workgroups", (long long)P);
    const size_t need = ldm_nearest_points_ws_bytes(P, Q);
    LDM_REQUIRE(ws_bytes >= need, LDM_ENOSPC, "ldm_nearest_points: workspace %zu < %zu B",
                ws_bytes, need);
    nearest_launch(q, P, c, (int)Q, d2, idx, reinterpret_cast<char*>(ws) + 256, (hipStream_t)s);
    return launch_status("ldm_nearest_points");
}

extern "C" size_t ldm_chamfer_ws_bytes(int64_t S, int64_t n, int64_t R, int64_t m) {
    using namespace ldm;
    if (S < 0 || n < 0 || R < 0 || m < 0 || S > kMaxCount || R > kMaxCount) return 0;
    size_t b = 256;                                          // the carried fp64 sum
    if (use_spread(S, n, R)) {
        // a pass of minima, and the partials of the largest pass that splits: the only one
        // when n < kSpreadTile, else the last (a full pass is of the one-pass form)
        const int64_t np = min(n, kSpreadTile);
        b += up256((size_t)np * sizeof(float)) +
             max(part_bytes(np, m), part_bytes(n % kSpreadTile, m));
    }
    return b;
}

extern "C" int ldm_chamfer_matrix(const float* a, int64_t S, int64_t n, const float* b,
                                  int64_t R, int64_t m, float* out, void* ws, size_t ws_bytes,
                                  ldm_stream_t s) {
    using namespace ldm;
    LDM_REQUIRE(S >= 0 && n >= 0 && R >= 0 && m >= 0, LDM_EINVAL,
                "ldm_chamfer_matrix: negative count (S = %lld, n = %lld, R = %lld, m = %lld)",
                (long long)S, (long long)n, (long long)R, (long long)m);
    if (S == 0 || R == 0) return 0;
    LDM_REQUIRE(n > 0 && m > 0, LDM_EINVAL,
                "ldm_chamfer_matrix: empty clouds (n = %lld, m = %lld) have no distance",
                (long long)n, (long long)m);
    LDM_REQUIRE(a && b && out && ws, LDM_EINVAL,
                "ldm_chamfer_matrix: NULL a / b / out / workspace");
    LDM_REQUIRE(LDM_ALIGNED(a, 4) && LDM_ALIGNED(b, 4) && LDM_ALIGNED(out, 4) &&
                    LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "ldm_chamfer_matrix: tensors must be 4-B, the workspace 256-B aligned");
    LDM_REQUIRE(n <= kMaxCount && m <= kMaxCount, LDM_EINVAL,
                "ldm_chamfer_matrix: n = %lld / m = %lld is above 2^31 - 1 points per cloud",
                (long long)n, (long long)m);
    LDM_REQUIRE(S <= kMaxCount && R <= kMaxCount && S * R <= kMaxCount, LDM_EINVAL,
                "ldm_chamfer_matrix: S x R = %lld x %lld needs more than 2^31 - 1 workgroups",
                (long long)S, (long long)R);
    const size_t need = ldm_chamfer_ws_bytes(S, n, R, m);
    LDM_REQUIRE(ws_bytes >= need, LDM_ENOSPC, "ldm_chamfer_matrix: workspace %zu < %zu B",
                ws_bytes, need);
    hipStream_t st = (hipStream_t)s;
    if (!use_spread(S, n, R)) {
        hipLaunchKernelGGL(chamfer_batch_kernel, dim3((unsigned)(S * R)), dim3(kThreads), 0, st,
                           a, (int)n, b, (int)R, (int)m, out);
        return launch_status("ldm_chamfer_matrix");
    }
    // spread form: per entry, the minima of a pass of kSpreadTile points go to memory through
    // the launches of ldm_nearest_points, and one workgroup adds them in the batch form's order
    double* acc = reinterpret_cast<double*>(ws);
    float* d2 = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + 256);
    void* part = reinterpret_cast<char*>(d2) + up256((size_t)min(n, kSpreadTile) * sizeof(float));
    for (int64_t e = 0; e < S * R; ++e) {
        const float* as = a + (e / R) * n * 3;
        const float* br = b + (e % R) * m * 3;
        for (int64_t p0 = 0; p0 < n; p0 += kSpreadTile) {
            const int64_t np = min(kSpreadTile, n - p0);
            nearest_launch(as + p0 * 3, np, br, (int)m, d2, nullptr, part, st);
            hipLaunchKernelGGL(chamfer_reduce_kernel, dim3(1), dim3(kThreads), 0, st, d2, (int)np,
                               p0 == 0 ? 1 : 0, p0 + np == n ? 1 : 0, n, acc, out + e);
        }
    }
    return launch_status("ldm_chamfer_matrix");
}
