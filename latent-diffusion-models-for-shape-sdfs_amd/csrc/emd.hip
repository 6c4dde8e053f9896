// Earth mover's distance between point clouds of equal size, MI355X (gfx950).  DESIGN.md §18.
//
//   EMD(a, b) = (1/n) min over permutations pi of sum_i |a_i - b_pi(i)|        (Euclidean)
//
// An eps-optimal assignment from a Jacobi auction with eps-scaling (Bertsekas): the points of a
// bid for the points of b ("objects"), every unassigned point in every round.  The result is a
// real permutation, so its cost is an upper bound of the optimum, and by eps-complementary
// slackness it is within eps (+ the fp32 slack of the header) of it.
//
// Pair arithmetic: §17's fixed sequence for d^2 (differences first, a product, two fmas,
// contraction off), then one v_sqrt_f32 (within 1 ulp): |d - exact| <= 5 u |exact|.
//
// One workgroup per matrix entry, everything in LDS (44 B per point):
//   both clouds as x / y / z planes, price[j], key[j], owner[j], two bidder lists, choice[k]
// A round:
//   bid      a wave per list slot k (bidder i): lanes scan the objects for the smallest and the
//            second smallest t_j = d_ij + price_j (the smaller j on a tie), a butterfly merges
//            the lanes' top-2, and lane 0 offers  bid = price_j1 + ((t2 - t1) + eps)  with one
//            64-bit integer LDS maximum on key[j1] = bits(bid) << 32 | ~i.  Bids are positive
//            floats, which order as their bits: the highest bid wins, the smallest bidder on a
//            tie, whatever the order the maxima arrive in.  No float atomics.
//   barrier
//   resolve  a thread per slot: the bidder whose index stands in key[choice[k]] takes the
//            object (price = its bid), the previous owner and every loser go to the next list.
//            The order of a list changes which wave serves a bidder, never a bid.
//   barrier
// price[] changes only in resolve, so every bid of a round sees the round's starting prices.
// key[j] is never cleared: it keeps the last winning bid = price[j], and a new bid must exceed
// the price (checked), so a stale key loses to it.
// A phase ends when the list is empty; eps goes max(eps, extent / 4) -> / kTheta -> .. -> eps,
// prices kept, owners cleared.  The loop is bounded by max_rounds; an entry that hits it, whose
// extent is above the caller's bound, or whose bid leaves (price, price cap] writes NaN and
// counts itself in *unconverged.
//
// 256 threads per workgroup up to 1024 points, where several workgroups share a compute unit;
// 1024 threads above, where LDS leaves room for one workgroup and its 16 waves serve 16 bidders
// at a time.  The scan takes 4 objects per lane and trip, loads first; the arrays are padded to
// whole trips with price = +inf, which never wins.
//
// The cost adds d(owner[j], j) in fp64: a thread its objects j = t, t + threads, .. in order, the
// wave by the shuffle tree 32 .. 1, the waves in order: a shape fixed by n alone.  An entry is a
// pure function of its two clouds, bit for bit.
#include "ldm_internal.h"

namespace ldm {
namespace {

constexpr int kSmallThreads = 256;             // n <= kSmallPoints: several workgroups share a CU
constexpr int kLargeThreads = 1024;            // above: LDS leaves room for one, which takes the CU
constexpr int kSmallPoints = 1024;
constexpr int kScan = 4;                       // objects per lane and trip of the scan
constexpr int kPad = 64 * kScan;               // arrays are padded to whole trips (price = +inf)
constexpr int kMaxPoints = 2048;               // 44 B of LDS per point: 88 KiB of the CU's 160
constexpr float kTheta = 4.0f;                 // eps divides by this per phase
constexpr float kPriceCapExtents = 8.0f;       // price cap = 8 extent + 4 eps (the slack's premise)
constexpr unsigned kNone = 0xffffu;
constexpr int64_t kMaxCount = 0x7fffffff;
constexpr double kU = 5.9604644775390625e-8;   // 2^-24

__device__ __forceinline__ float pair_dist(float ax, float ay, float az, float bx, float by,
                                           float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    float d = dx * dx;
    d = __builtin_fmaf(dy, dy, d);
    d = __builtin_fmaf(dz, dz, d);
    return __builtin_amdgcn_sqrtf(d);               // v_sqrt_f32: within 1 ulp
}

// lane l reads lane l ^ X: within a row of 16 by DPP, across rows through the LDS crossbar
template <int X>
__device__ __forceinline__ int lane_xor(int v) {
    if (X == 1) return __builtin_amdgcn_update_dpp(v, v, 0xb1, 0xf, 0xf, false);   // quad [1,0,3,2]
    if (X == 2) return __builtin_amdgcn_update_dpp(v, v, 0x4e, 0xf, 0xf, false);   // quad [2,3,0,1]
    return __shfl_xor(v, X, 64);
}

struct Top2 {
    float t1, t2;   // smallest and second smallest d + price
    int j1;         // object of t1 (the smallest index on a tie)
};

template <int X>
__device__ __forceinline__ void merge(Top2& m) {
    const float pt1 = __int_as_float(lane_xor<X>(__float_as_int(m.t1)));
    const float pt2 = __int_as_float(lane_xor<X>(__float_as_int(m.t2)));
    const int pj1 = lane_xor<X>(m.j1);
    const bool theirs = (pt1 < m.t1) | ((pt1 == m.t1) & (pj1 < m.j1));
    m.t2 = __builtin_fminf(__builtin_fminf(m.t2, pt2), theirs ? m.t1 : pt1);
    m.t1 = theirs ? pt1 : m.t1;
    m.j1 = theirs ? pj1 : m.j1;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __builtin_fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

struct Args {
    const float* a;
    const float* b;
    int n, R, within;
    float eps, extent_bound;
    int max_rounds;
    float* out;
    int32_t* assign;
    int32_t* rounds;
    int32_t* unconverged;
};

__device__ __forceinline__ void write_entry(const Args& g, int64_t s, int64_t r, float v,
                                            int nrounds) {
    const int64_t e = s * g.R + r;
    g.out[e] = v;
    if (g.rounds) g.rounds[e] = nrounds;
    if (g.within) {
        g.out[r * g.R + s] = v;
        if (g.rounds) g.rounds[r * g.R + s] = nrounds;
    }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void emd_kernel(const Args g) {
    constexpr int kWaves = kThreads / 64;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double red[kWaves];
    __shared__ float box[6][kWaves];
    __shared__ float pm[kWaves];
    __shared__ int count[2];
    __shared__ int fail;

    const int n = g.n, np = (n + kPad - 1) / kPad * kPad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t s = blockIdx.x / (unsigned)g.R, r = blockIdx.x % (unsigned)g.R;
    const int64_t e = s * g.R + r;
    int32_t* const pi = g.assign ? g.assign + e * n : nullptr;

    if (g.within) {
        if (s > r) return;                          // the (r, s) workgroup writes this entry too
        if (s == r) {                               // the identity is optimal: an exact 0
            if (tid == 0) {
                g.out[e] = 0.0f;
                if (g.rounds) g.rounds[e] = 0;
            }
            if (pi)
                for (int i = tid; i < n; i += kThreads) pi[i] = i;
            return;
        }
    }
    int32_t* const pi_t = g.assign && g.within ? g.assign + (r * g.R + s) * n : nullptr;

    unsigned long long* const key = reinterpret_cast<unsigned long long*>(lds_raw);
    float* const bx = reinterpret_cast<float*>(key + np);
    float* const by = bx + np;
    float* const bz = by + np;
    float* const ax = bz + np;
    float* const ay = ax + np;
    float* const az = ay + np;
    float* const price = az + np;
    unsigned short* const owner = reinterpret_cast<unsigned short*>(price + np);
    unsigned short* const choice = owner + np;
    unsigned short* const list0 = choice + np;
    unsigned short* const list1 = list0 + np;

    // the clouds, prices and keys; the pair's bounding box
    const float* __restrict__ as = g.a + s * n * 3;
    const float* __restrict__ br = g.b + r * n * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += kThreads) {
        const float p[6] = {as[(int64_t)i * 3],     as[(int64_t)i * 3 + 1], as[(int64_t)i * 3 + 2],
                            br[(int64_t)i * 3],     br[(int64_t)i * 3 + 1], br[(int64_t)i * 3 + 2]};
        ax[i] = p[0]; ay[i] = p[1]; az[i] = p[2];
        bx[i] = p[3]; by[i] = p[4]; bz[i] = p[5];
        price[i] = 0.0f;
        key[i] = 0ull;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = __builtin_fminf(lo[c], __builtin_fminf(p[c], p[c + 3]));
            hi[c] = __builtin_fmaxf(hi[c], __builtin_fmaxf(p[c], p[c + 3]));
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = wave_min(lo[c]);
        hi[c] = wave_max(hi[c]);
        if (lane == 0) {
            box[c][wave] = lo[c];
            box[c + 3][wave] = hi[c];
        }
    }
    for (int i = n + tid; i < np; i += kThreads) {  // the padding never wins a scan
        bx[i] = by[i] = bz[i] = 0.0f;
        price[i] = INFINITY;
    }
    if (tid == 0) fail = 0;
    __syncthreads();
    float extent;
    {
#pragma clang fp contract(off)
        float ex[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float l = box[c][0], h = box[c + 3][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                l = __builtin_fminf(l, box[c][w]);
                h = __builtin_fmaxf(h, box[c + 3][w]);
            }
            ex[c] = h - l;
        }
        float q = ex[0] * ex[0];
        q = __builtin_fmaf(ex[1], ex[1], q);
        q = __builtin_fmaf(ex[2], ex[2], q);
        extent = __builtin_sqrtf(q);
    }

    int nrounds = 0;
    bool ok = extent <= g.extent_bound;             // false for a NaN too
    if (n == 1) {
        if (tid == 0) owner[0] = 0;
    } else if (ok) {
        const float eps = g.eps;
        const float cap = __builtin_fmaf(kPriceCapExtents, g.extent_bound, 4.0f * eps);
        float eps_cur = __builtin_fmaxf(eps, 0.25f * extent);
        for (;;) {                                  // a phase
            // Prices matter only up to a common constant.  Each phase starts them at minimum 0:
            // a set of well separated matches would otherwise lift all of them by about an
            // extent per phase, and the fp32 slack grows with the largest price.
            float pmin = INFINITY;
            for (int i = tid; i < n; i += kThreads) pmin = __builtin_fminf(pmin, price[i]);
            pmin = wave_min(pmin);
            if (lane == 0) pm[wave] = pmin;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < kWaves; ++w) pmin = __builtin_fminf(pmin, pm[w]);
            for (int i = tid; i < n; i += kThreads) {
                const float p = price[i] - pmin;
                price[i] = p;
                key[i] = (unsigned long long)__float_as_uint(p) << 32;
                owner[i] = (unsigned short)kNone;
                list0[i] = (unsigned short)i;
            }
            if (tid == 0) count[0] = n;
            __syncthreads();
            int cur = 0;
            for (;;) {                              // a round
                const int c = count[cur];
                if (c == 0) break;
                if (nrounds >= g.max_rounds) {
                    ok = false;
                    break;
                }
                const unsigned short* const list = cur ? list1 : list0;
                unsigned short* const next = cur ? list0 : list1;
                if (tid == 0) count[cur ^ 1] = 0;
                for (int k = wave; k < c; k += kWaves) {
                    const int i = list[k];
                    const float pax = ax[i], pay = ay[i], paz = az[i];
                    Top2 m = {INFINITY, INFINITY, n};
                    for (int j0 = lane; j0 < np; j0 += kPad) {
                        float qx[kScan], qy[kScan], qz[kScan], qp[kScan];
#pragma unroll
                        for (int u = 0; u < kScan; ++u) {   // the loads first: they overlap
                            qx[u] = bx[j0 + 64 * u];
                            qy[u] = by[j0 + 64 * u];
                            qz[u] = bz[j0 + 64 * u];
                            qp[u] = price[j0 + 64 * u];
                        }
#pragma unroll
                        for (int u = 0; u < kScan; ++u) {
                            const float t = pair_dist(pax, pay, paz, qx[u], qy[u], qz[u]) + qp[u];
                            const bool lt = t < m.t1;       // strict: the smaller index keeps a tie
                            m.t2 = __builtin_fminf(m.t2, __builtin_fmaxf(m.t1, t));
                            m.t1 = lt ? t : m.t1;
                            m.j1 = lt ? j0 + 64 * u : m.j1;
                        }
                    }
                    merge<1>(m);
                    merge<2>(m);
                    merge<4>(m);
                    merge<8>(m);
                    merge<16>(m);
                    merge<32>(m);
                    if (lane == 0) {
                        bool good = m.j1 < n;
                        if (good) {
                            const float p1 = price[m.j1];
                            const float bid = p1 + ((m.t2 - m.t1) + eps_cur);
                            good = bid > p1 && bid <= cap;
                            if (good) {
                                choice[k] = (unsigned short)m.j1;
                                atomicMax(&key[m.j1],
                                          (unsigned long long)__float_as_uint(bid) << 32 |
                                              (0xffffffffu - (unsigned)i));
                            }
                        }
                        if (!good) fail = 1;
                    }
                }
                __syncthreads();
                if (fail) {                         // written before the barrier only: uniform
                    ok = false;
                    break;
                }
                for (int k = tid; k < c; k += kThreads) {
                    const unsigned i = list[k], j = choice[k];
                    const unsigned long long kk = key[j];
                    if (0xffffffffu - (unsigned)kk == i) {
                        const unsigned o = owner[j];
                        if (o != kNone) next[atomicAdd(&count[cur ^ 1], 1)] = (unsigned short)o;
                        owner[j] = (unsigned short)i;
                        price[j] = __uint_as_float((unsigned)(kk >> 32));
                    } else {
                        next[atomicAdd(&count[cur ^ 1], 1)] = (unsigned short)i;
                    }
                }
                __syncthreads();
                cur ^= 1;
                ++nrounds;
            }
            if (!ok || eps_cur <= eps) break;
            eps_cur = __builtin_fmaxf(eps, eps_cur / kTheta);
            __syncthreads();                        // count[] was read by all before it is reset
        }
    }
    __syncthreads();

    if (!ok) {
        if (tid == 0) {
            write_entry(g, s, r, __builtin_nanf(""), nrounds);
            atomicAdd(g.unconverged, 1);
        }
        for (int i = tid; i < n; i += kThreads) {
            if (pi) pi[i] = -1;
            if (pi_t) pi_t[i] = -1;
        }
        return;
    }

    // the cost of the assignment, in fp64, in an order fixed by n
    double x = 0.0;
    for (int j = tid; j < n; j += kThreads) {
        const int i = owner[j];
        x = x + (double)pair_dist(ax[i], ay[i], az[i], bx[j], by[j], bz[j]);
        if (pi) pi[i] = j;
        if (pi_t) pi_t[j] = i;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    if (lane == 0) red[wave] = x;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t = t + red[w];
        write_entry(g, s, r, (float)(t / (double)n), nrounds);
    }
}

inline size_t lds_bytes(int64_t n) { return (size_t)((n + kPad - 1) / kPad * kPad) * 44; }

}  // namespace
}  // namespace ldm

extern "C" int64_t ldm_emd_max_points(void) { return ldm::kMaxPoints; }

// 8 x the fp32 slack: 5 u (extent + price cap) + 10 u extent with the price cap
// at 8 extents = 55 u extent
extern "C" double ldm_emd_slack(double extent) {
    return extent >= 0.0 ? 55.0 * ldm::kU * extent : 0.0;
}
extern "C" double ldm_emd_min_eps(double extent) { return 8.0 * ldm_emd_slack(extent); }

// the reference auction's round counts stay under 16 n + 2048; 16 x that
extern "C" int64_t ldm_emd_default_max_rounds(int64_t n) {
    if (n < 1 || n > ldm::kMaxPoints) return 0;
    return 256 * n + 32768;
}

extern "C" size_t ldm_emd_ws_bytes(int64_t S, int64_t R, int64_t n) {
    if (S < 0 || R < 0 || n < 0 || S > ldm::kMaxCount || R > ldm::kMaxCount) return 0;
    return 256;                                              // the unconverged count
}

extern "C" int ldm_emd_matrix(const float* a, int64_t S, const float* b, int64_t R, int64_t n,
                              float eps, float extent, int64_t max_rounds, int within,
                              float* out, int32_t* assign, int32_t* rounds,
                              int32_t* unconverged, void* ws, size_t ws_bytes, ldm_stream_t s) {
    using namespace ldm;
    LDM_REQUIRE(S >= 0 && R >= 0 && n >= 0, LDM_EINVAL,
                "ldm_emd_matrix: negative count (S = %lld, R = %lld, n = %lld)", (long long)S,
                (long long)R, (long long)n);
    if (S == 0 || R == 0) return 0;
    LDM_REQUIRE(n > 0, LDM_EINVAL, "ldm_emd_matrix: empty clouds have no distance");
    LDM_REQUIRE(n <= kMaxPoints, LDM_ENOSYS,
                "ldm_emd_matrix: n = %lld is above ldm_emd_max_points() = %d (one workgroup "
                "keeps a pair in LDS)", (long long)n, kMaxPoints);
    LDM_REQUIRE(a && b && out && ws, LDM_EINVAL, "ldm_emd_matrix: NULL a / b / out / workspace");
    LDM_REQUIRE(LDM_ALIGNED(a, 4) && LDM_ALIGNED(b, 4) && LDM_ALIGNED(out, 4) &&
                    LDM_ALIGNED(assign, 4) && LDM_ALIGNED(rounds, 4) &&
                    LDM_ALIGNED(unconverged, 4) && LDM_ALIGNED(ws, 256),
                LDM_EALIGN, "ldm_emd_matrix: tensors must be 4-B, the workspace 256-B aligned");
    LDM_REQUIRE(S <= kMaxCount && R <= kMaxCount && S * R <= kMaxCount, LDM_EINVAL,
                "ldm_emd_matrix: S x R = %lld x %lld needs more than 2^31 - 1 workgroups",
                (long long)S, (long long)R);
    LDM_REQUIRE(!within || (S == R && a == b), LDM_EINVAL,
                "ldm_emd_matrix: a within-set matrix needs b == a and R == S");
    LDM_REQUIRE(extent >= 0.0f && extent < INFINITY, LDM_EINVAL,
                "ldm_emd_matrix: the extent bound must be finite and >= 0");
    LDM_REQUIRE(eps > 0.0f && eps < INFINITY && (double)eps >= ldm_emd_min_eps((double)extent),
                LDM_EINVAL,
                "ldm_emd_matrix: eps = %g is below ldm_emd_min_eps(%g) = %g, under which fp32 "
                "rounding is no longer small against eps", (double)eps, (double)extent,
                ldm_emd_min_eps((double)extent));
    LDM_REQUIRE(max_rounds >= 0 && max_rounds <= kMaxCount, LDM_EINVAL,
                "ldm_emd_matrix: max_rounds = %lld (0: the default)", (long long)max_rounds);
    const size_t need = ldm_emd_ws_bytes(S, R, n);
    LDM_REQUIRE(ws_bytes >= need, LDM_ENOSPC, "ldm_emd_matrix: workspace %zu < %zu B", ws_bytes,
                need);
    const size_t lds = lds_bytes(n);
    if (n > kSmallPoints)
        LDM_TRY(set_max_lds_once<emd_kernel<kLargeThreads>>((int)lds_bytes(kMaxPoints),
                                                            "ldm_emd_matrix"));
    hipStream_t st = (hipStream_t)s;
    // the count lives in the workspace when the caller does not ask for it
    int32_t* cnt = unconverged ? unconverged : reinterpret_cast<int32_t*>(ws);
    if (hipMemsetAsync(cnt, 0, sizeof(int32_t), st) != hipSuccess)
        return launch_status("ldm_emd_matrix");
    Args g;
    g.a = a;
    g.b = b;
    g.n = (int)n;
    g.R = (int)R;
    g.within = within ? 1 : 0;
    g.eps = eps;
    g.extent_bound = extent;
    g.max_rounds = (int)(max_rounds ? max_rounds : ldm_emd_default_max_rounds(n));
    g.out = out;
    g.assign = assign;
    g.rounds = rounds;
    g.unconverged = cnt;
    if (n > kSmallPoints)
        hipLaunchKernelGGL(emd_kernel<kLargeThreads>, dim3((unsigned)(S * R)),
                           dim3(kLargeThreads), lds, st, g);
    else
        hipLaunchKernelGGL(emd_kernel<kSmallThreads>, dim3((unsigned)(S * R)),
                           dim3(kSmallThreads), lds, st, g);
    return launch_status("ldm_emd_matrix");
}
