// C17 training: the backward of ldm_conv1d on MI355X (gfx950), DESIGN.md §15.
//
// Two kernels, both implicit GEMMs on v_mfma_f32_16x16x4_f32 (fp32 operands, products and
// accumulation, as the forward; bf16-stored weights are widened while they are staged):
//   ldm_conv1d_bwd_data    dX = act'(X) * (W^T (*) dY): per workgroup 16 input channels x 64
//                          source positions of one shape, contraction over (tap, Cout).  The
//                          forward's packed weight [Cout16][K][Cw16] is transposed while it is
//                          staged into LDS ([tap][ci][co]), so there is no second weight copy.
//   ldm_conv1d_bwd_weight  dW = dY (*) act(X): per workgroup a 16 x 16 (co, ci) tile of every tap
//                          of one segment over one slice of the B * L_out contraction; fp32
//                          partials go to the caller's workspace and a second kernel sums the
//                          slices in slice order into the forward's packed layout.
// No atomics anywhere: every output element has one writer and a fixed summation order.
#include "ldm_internal.h"

#include <string.h>

namespace ldm {
namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int round16(int c) { return (c + 15) & ~15; }
// channel position inside a group of 16 of the packed weight (include/ldm_sdf.h); an involution
__host__ __device__ constexpr int perm16(int ci) {
    return (ci & ~15) | ((ci & 3) << 2) | ((ci >> 2) & 3);
}

#define LDM_KC __attribute__((address_space(4)))

constexpr int kMaxLdsBytes = 160 * 1024;
constexpr int kTileU = 64;       // bwd_data: source positions per workgroup (16 per wave)
constexpr int kTileL = 64;       // bwd_weight: output positions per contraction unit
// bwd_weight: slices of the B * L_out contraction.  (Sizing the slice count for ~2048 workgroups
// per launch, up to 256 slices, measured no better: 1.93 against 1.82 ms for the 18 calls of a
// config-5 step, DESIGN.md §15 -- the cost is the staging of a unit, not the chain of units.)
constexpr int kMaxSplits = 64;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
__device__ __forceinline__ float silu_grad_f(float x) {
    const float s = sigmoid_f(x);
    return s * (1.f + x * (1.f - s));
}

// ---- data gradient ------------------------------------------------------------------------
// With u the position on the conv's input grid (the 2x upsampled grid for LDM_CONV_UP2):
//   G[ci][u] = sum_k sum_co W(co,ci,k) E[co][u + pad - k],  E[co][v] = dY[co][v / stride] when
//   stride divides v and the quotient lies in [0, L_out), else 0
// and dX[p] = act'(X[p]) G[p] (DIRECT) or act'(X[p]) (G[2p] + G[2p+1]) (UP2).
// LDS: wsT [K][16 ci][pitch] and es [64 + K - 1][pitch], pitch = Cout16 + 8 floats: a lane's
// operands of 4 consecutive MFMAs (4 consecutive co) are one 16-byte read, and rows 8 mod 16
// floats apart put the 16-lane groups of a ds_read_b128 on distinct bank quads.
struct BwdDataK {
    ldm_conv1d_bwd_data_args_t a;
    int U;        // positions of the input grid (L_in, or 2 L_in for UP2)
    int pitch;
};

template <typename TW>
__global__ __launch_bounds__(256) void conv1d_bwd_data_kernel(BwdDataK ka) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const LDM_KC BwdDataK* kp = (const LDM_KC BwdDataK*)__builtin_amdgcn_kernarg_segment_ptr();
    const LDM_KC ldm_conv1d_bwd_data_args_t& a = kp->a;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int u0 = blockIdx.x * kTileU, ci0 = blockIdx.y * 16, b = blockIdx.z;
    const int K = a.seg.ksize, st = a.seg.stride, pad = a.seg.pad;
    const int Cout = a.Cout, Cout16 = round16(Cout), L_out = a.L_out;
    const int C = a.seg.C, L_in = a.seg.L_in, U = kp->U, pitch = kp->pitch;
    const int win = kTileU + K - 1;
    float* wsT = sm;                       // [K][16][pitch]
    float* es = sm + K * 16 * pitch;       // [win][pitch]

    // weights: 4 packed columns (16 / 8 bytes) of row co, tap k per item, co fastest so that
    // the transposed LDS stores of a wave fall on consecutive words
    {
        const TW* W = reinterpret_cast<const TW*>(a.seg.W);
        const int nw = K * 4 * Cout16;
        for (int it = tid; it < nw; it += 256) {
            const int r = it / Cout16, co = it - r * Cout16;
            const int q4 = r & 3, k = r >> 2;
            const int64_t gi = (int64_t)co * a.seg.ldw + (int64_t)k * a.seg.kstride + ci0 + 4 * q4;
            float w[4];
            if constexpr (sizeof(TW) == 2) {
                const u32x2 v = *reinterpret_cast<const u32x2*>(W + gi);
                w[0] = __builtin_bit_cast(float, v[0] << 16);
                w[1] = __builtin_bit_cast(float, v[0] & 0xffff0000u);
                w[2] = __builtin_bit_cast(float, v[1] << 16);
                w[3] = __builtin_bit_cast(float, v[1] & 0xffff0000u);
            } else {
                const f32x4 v = *reinterpret_cast<const f32x4*>(W + gi);
                w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ci = perm16(4 * q4 + e);      // the channel stored at that column
                LDM_DASSERT(k < K && ci < 16 && co < pitch);
                wsT[(k * 16 + ci) * pitch + co] = w[e];
            }
        }
    }
    // dY window on the stride-dilated grid, zeros where no output position maps
    {
        const int vbase = u0 + pad - (K - 1);
        const float* dYb = a.dY + (int64_t)b * Cout * L_out;
        const int ne = win * Cout16;
        for (int it = tid; it < ne; it += 256) {
            const int co = it / win, j = it - co * win;
            const int v = vbase + j;
            float x = 0.f;
            if (co < Cout && v >= 0) {
                const int l = st == 2 ? v >> 1 : v;
                if ((st == 1 || !(v & 1)) && l < L_out) x = dYb[(int64_t)co * L_out + l];
            }
            LDM_DASSERT(j < win && co < pitch);
            es[j * pitch + co] = x;
        }
    }
    __syncthreads();
    if (u0 + wave * 16 >= U) return;       // wave-uniform; no barrier below

    const int t = wave * 16 + c16;         // this lane's position of the tile (B operand column)
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int nc = Cout16 >> 4;
    for (int k = 0; k < K; ++k) {
        const float* ap = wsT + (k * 16 + c16) * pitch + 4 * g;
        const float* bp = es + (t + K - 1 - k) * pitch + 4 * g;
        LDM_DASSERT(t + K - 1 - k >= 0 && t + K - 1 - k < win);
        int c = 0;
        for (; c + 1 < nc; c += 2) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + 16 * c);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + 16 * c);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(ap + 16 * c + 16);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 16 * c + 16);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m], b0[m], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m], b1[m], acc1, 0, 0, 0);
            }
        }
        if (c < nc) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + 16 * c);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + 16 * c);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m], b0[m], acc0, 0, 0, 0);
        }
    }
    f32x4 acc = acc0 + acc1;               // lane (c16, g), register i: channel 4 g + i, column c16
    const bool up2 = a.seg.mode == LDM_CONV_UP2;
    const int u = u0 + t;
    if (up2) {
        // the two upsampled positions 2p, 2p + 1 are neighbouring columns: the even lane owns p
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += __shfl_xor(acc[i], 1);
    }
    const int p = up2 ? u >> 1 : u;
    if ((up2 && (u & 1)) || p >= L_in) return;
    const bool act = a.seg.silu_in != 0, accum = a.accumulate != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = ci0 + 4 * g + i;
        if (ci >= C) continue;
        const int64_t idx = ((int64_t)b * C + ci) * L_in + p;
        float v = acc[i];
        if (act) v *= silu_grad_f(a.seg.X[idx]);
        if (accum) v += a.dX[idx];
        a.dX[idx] = v;
    }
}

int check_seg(const ldm_conv1d_seg_t& g, int i, int L_out, const char* what) {
    LDM_REQUIRE(g.C >= 1 && g.L_in >= 1 && g.pad >= 0, LDM_EINVAL, "%s seg %d: bad operand", what, i);
    const bool ok = (g.ksize == 3 && (g.stride == 1 || g.stride == 2)) ||
                    (g.ksize == 1 && g.stride == 1) || (g.ksize == 4 && g.stride == 2);
    LDM_REQUIRE(ok, LDM_ENOSYS, "%s seg %d: no kernel for ksize %d / stride %d", what, i, g.ksize,
                g.stride);
    LDM_REQUIRE(g.mode == LDM_CONV_DIRECT || (g.mode == LDM_CONV_UP2 && g.stride == 1), LDM_EINVAL,
                "%s seg %d: bad mode %d", what, i, g.mode);
    LDM_REQUIRE(g.pad < g.ksize, LDM_EINVAL, "%s seg %d: pad %d >= ksize", what, i, g.pad);
    LDM_REQUIRE(g.kstride >= round16(g.C) && g.ldw >= g.ksize * g.kstride && g.kstride % 16 == 0 &&
                    g.ldw % 16 == 0,
                LDM_EINVAL, "%s seg %d: packed weight pitches (ldw %d, kstride %d)", what, i, g.ldw,
                g.kstride);
    const int64_t Lsrc = g.mode == LDM_CONV_UP2 ? 2 * (int64_t)g.L_in : g.L_in;
    LDM_REQUIRE(Lsrc + 2 * g.pad >= g.ksize && (Lsrc + 2 * g.pad - g.ksize) / g.stride + 1 == L_out,
                LDM_EINVAL, "%s seg %d: L_in %d does not give L_out %d", what, i, g.L_in, L_out);
    LDM_REQUIRE(Lsrc < (1ll << 30), LDM_EINVAL, "%s seg %d: L_in %d too long", what, i, g.L_in);
    return 0;
}

int check_bwd_data(const ldm_conv1d_bwd_data_args_t* a) {
    LDM_REQUIRE(a && a->dY && a->dX && a->seg.W, LDM_EINVAL, "conv1d_bwd_data: NULL operand");
    LDM_REQUIRE(a->B >= 1 && a->B <= 65535 && a->Cout >= 1 && a->L_out >= 1, LDM_EINVAL,
                "conv1d_bwd_data: bad sizes (B %d, Cout %d, L_out %d)", a->B, a->Cout, a->L_out);
    LDM_REQUIRE(a->w_dtype == LDM_F32 || a->w_dtype == LDM_BF16, LDM_EINVAL,
                "conv1d_bwd_data: bad w_dtype %d", a->w_dtype);
    LDM_TRY(check_seg(a->seg, 0, a->L_out, "conv1d_bwd_data"));
    LDM_REQUIRE(!a->seg.silu_in || a->seg.X, LDM_EINVAL, "conv1d_bwd_data: SiLU' needs seg.X");
    const uintptr_t wal = a->w_dtype == LDM_BF16 ? 32 : 64;     // 16 channels
    LDM_REQUIRE(LDM_ALIGNED(a->seg.W, wal), LDM_EALIGN,
                "conv1d_bwd_data: W must sit at a multiple of 16 channels of a 64-byte aligned "
                "packed weight");
    LDM_REQUIRE(LDM_ALIGNED(a->dY, 4) && LDM_ALIGNED(a->dX, 4) && LDM_ALIGNED(a->seg.X, 4),
                LDM_EALIGN, "conv1d_bwd_data: fp32 operands must be 4-byte aligned");
    return 0;
}

template <typename TW>
int launch_bwd_data(const ldm_conv1d_bwd_data_args_t& a, hipStream_t s) {
    const int64_t lds = (int64_t)4 * (a.seg.ksize * 16 + kTileU + a.seg.ksize - 1) *
                        ((int64_t)round16(a.Cout) + 8);
    LDM_REQUIRE(lds <= kMaxLdsBytes, LDM_ENOSPC,
                "conv1d_bwd_data: staged operands need %lld B of LDS (> %d); split Cout",
                (long long)lds, kMaxLdsBytes);
    BwdDataK ka;
    ka.a = a;
    ka.U = a.seg.mode == LDM_CONV_UP2 ? 2 * a.seg.L_in : a.seg.L_in;
    ka.pitch = round16(a.Cout) + 8;
    const dim3 grid((ka.U + kTileU - 1) / kTileU, round16(a.seg.C) / 16, a.B);
    LDM_REQUIRE(grid.y <= 65535, LDM_EINVAL, "conv1d_bwd_data: C %d too large", a.seg.C);
    LDM_TRY((set_max_lds_once<&conv1d_bwd_data_kernel<TW>>(kMaxLdsBytes, "conv1d_bwd_data")));
    hipLaunchKernelGGL((conv1d_bwd_data_kernel<TW>), grid, dim3(256), (int)lds, s, ka);
    return launch_status("ldm_conv1d_bwd_data");
}

// ---- weight gradient ----------------------------------------------------------------------
// A contraction unit is (shape b, 64 output positions).  Slice s of S owns units
// [n s / S, n (s + 1) / S).  Per unit the workgroup stages dY [16 co][64] and the activated input
// window [16 ci][63 stride + K] (UP2: already upsampled), and wave w contracts positions
// 16 w .. 16 w + 15 for every tap: A = dY (one 16-byte read: 4 consecutive positions of row co),
// B = the window at (position) stride + tap (scalar reads; odd row pitch).  After the last unit
// the four waves' tiles are summed in wave order through LDS and written to ws[s].
struct BwdWeightK {
    ldm_conv1d_bwd_weight_args_t a;
    int S, nlt;                  // slices; 64-position tiles per shape
    int64_t n_units, part;       // B * nlt; floats of one slice's partial
    int tile0[LDM_CONV_MAX_SEGS + 1];      // first ci tile (grid z) of every segment
    int64_t poff[LDM_CONV_MAX_SEGS + 1];   // float offset of a segment inside a partial
    float* dcb;                  // per-(b, co) sums of dY: a.dcbias or workspace (or NULL)
};

__global__ __launch_bounds__(256) void conv1d_bwd_weight_kernel(BwdWeightK ka) {
    __shared__ __attribute__((aligned(16))) float sm[4096];
    const LDM_KC BwdWeightK* kp = (const LDM_KC BwdWeightK*)__builtin_amdgcn_kernarg_segment_ptr();
    const LDM_KC ldm_conv1d_bwd_weight_args_t& a = kp->a;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int sl = blockIdx.x, co0 = blockIdx.y * 16;
    int si = 0;
    while (si + 1 < a.n_seg && (int)blockIdx.z >= kp->tile0[si + 1]) ++si;
    const int ci0 = ((int)blockIdx.z - kp->tile0[si]) * 16;
    const LDM_KC ldm_conv1d_seg_t& sg = a.seg[si];
    const int K = sg.ksize, st = sg.stride, pad = sg.pad, C = sg.C, L_in = sg.L_in;
    const bool up2 = sg.mode == LDM_CONV_UP2, act = sg.silu_in != 0;
    const int Lsrc = up2 ? 2 * L_in : L_in;
    const int Cout = a.Cout, L_out = a.L_out;
    const int win = (kTileL - 1) * st + K, xp = win | 1;
    constexpr int yp = kTileL + 8;
    float* dys = sm;                  // [16][yp]
    float* xs = sm + 16 * yp;         // [16][xp]  (16 * 72 + 16 * 131 = 3248 <= 4096)

    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t u_beg = kp->n_units * sl / kp->S, u_end = kp->n_units * (sl + 1) / kp->S;
    for (int64_t u = u_beg; u < u_end; ++u) {
        const int b = (int)(u / kp->nlt), l0 = (int)(u - (int64_t)b * kp->nlt) * kTileL;
        const float* dYb = a.dY + (int64_t)b * Cout * L_out;
        for (int it = tid; it < 16 * kTileL; it += 256) {
            const int co = it >> 6, j = it & 63;
            const bool ok = co0 + co < Cout && l0 + j < L_out;
            dys[co * yp + j] = ok ? dYb[(int64_t)(co0 + co) * L_out + l0 + j] : 0.f;
        }
        const int pstart = l0 * st - pad;
        const float* Xb = sg.X + (int64_t)b * C * L_in;
        for (int it = tid; it < 16 * win; it += 256) {
            const int ci = it / win, j = it - ci * win;
            const int pp = pstart + j;
            const bool ok = ci0 + ci < C && pp >= 0 && pp < Lsrc;
            float x = ok ? Xb[(int64_t)(ci0 + ci) * L_in + (up2 ? pp >> 1 : pp)] : 0.f;
            if (act) x = silu_f(x);                  // SiLU(0) = 0: the padding stays zero
            LDM_DASSERT(ci < 16 && j < xp && 16 * yp + ci * xp + j < 4096);
            xs[ci * xp + j] = x;
        }
        __syncthreads();
        const f32x4 av = *reinterpret_cast<const f32x4*>(dys + c16 * yp + wave * 16 + 4 * g);
        const float* bp = xs + c16 * xp + (wave * 16 + 4 * g) * st;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= K) break;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bp[m * st + k], acc[k], 0, 0, 0);
        }
        __syncthreads();
    }
    // the four waves' tiles, summed in wave order
    float* red = sm;                  // [wave][tap][register][lane]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[((wave * 4 + k) * 4 + i) * 64 + lane] = acc[k][i];
    __syncthreads();
    const int C16 = round16(C);
    float* part = a.ws + (int64_t)sl * kp->part + kp->poff[si];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = tid + 256 * r;
        const int ln = e & 63, i = (e >> 6) & 3, k = e >> 8;
        if (k >= K) continue;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) v += red[((w * 4 + k) * 4 + i) * 64 + ln];
        const int co = co0 + 4 * (ln >> 4) + i, ci = ci0 + perm16(ln & 15);
        LDM_DASSERT(co < round16(Cout) && ci < C16);
        part[((int64_t)co * K + k) * C16 + ci] = v;
    }
}

// dW (packed) = the slices' partials summed in slice order
__global__ __launch_bounds__(256) void conv1d_bwd_weight_reduce_kernel(BwdWeightK ka) {
    const LDM_KC BwdWeightK* kp = (const LDM_KC BwdWeightK*)__builtin_amdgcn_kernarg_segment_ptr();
    const LDM_KC ldm_conv1d_bwd_weight_args_t& a = kp->a;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= kp->part) return;
    int si = 0;
    while (si + 1 < a.n_seg && e >= kp->poff[si + 1]) ++si;
    const int K = a.seg[si].ksize, C16 = round16(a.seg[si].C);
    const int64_t r = e - kp->poff[si];
    const int ci = (int)(r % C16);
    const int64_t q = r / C16;
    const int k = (int)(q % K), co = (int)(q / K);
    float v = 0.f;
    for (int s = 0; s < kp->S; ++s) v += a.ws[(int64_t)s * kp->part + e];
    a.dW[si][(int64_t)co * a.seg[si].ldw + (int64_t)k * a.seg[si].kstride + ci] = v;
}

// dcb[b][co] = sum_l dY[b][co][l]: one wave per row, lanes stride the row, then a fixed tree
__global__ __launch_bounds__(64) void conv1d_rowsum_kernel(const float* __restrict__ dY, int L,
                                                            float* __restrict__ out) {
    const float* row = dY + (int64_t)blockIdx.x * L;
    float v = 0.f;
    for (int l = threadIdx.x; l < L; l += 64) v += row[l];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// dbias[co] = sum_b dcb[b][co], in b order
__global__ __launch_bounds__(64) void conv1d_dbias_kernel(const float* __restrict__ dcb, int B,
                                                           int Cout, float* __restrict__ dbias) {
    const int co = blockIdx.x * 64 + threadIdx.x;
    if (co >= Cout) return;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += dcb[(int64_t)b * Cout + co];
    dbias[co] = v;
}

int check_bwd_weight(const ldm_conv1d_bwd_weight_args_t* a) {
    LDM_REQUIRE(a && a->dY, LDM_EINVAL, "conv1d_bwd_weight: NULL operand");
    LDM_REQUIRE(a->B >= 1 && a->B <= 65535 && a->Cout >= 1 && a->L_out >= 1, LDM_EINVAL,
                "conv1d_bwd_weight: bad sizes (B %d, Cout %d, L_out %d)", a->B, a->Cout, a->L_out);
    LDM_REQUIRE(a->n_seg >= 1 && a->n_seg <= LDM_CONV_MAX_SEGS, LDM_EINVAL,
                "conv1d_bwd_weight: bad n_seg %d", a->n_seg);
    LDM_REQUIRE(a->Cout <= 65535 * 16 && (int64_t)a->B * a->Cout < (1ll << 31), LDM_EINVAL,
                "conv1d_bwd_weight: Cout %d too large", a->Cout);
    int64_t tiles = 0;
    for (int i = 0; i < a->n_seg; ++i) {
        LDM_REQUIRE(a->seg[i].X && a->dW[i], LDM_EINVAL, "conv1d_bwd_weight seg %d: NULL operand", i);
        LDM_TRY(check_seg(a->seg[i], i, a->L_out, "conv1d_bwd_weight"));
        LDM_REQUIRE(LDM_ALIGNED(a->dW[i], 64), LDM_EALIGN,
                    "conv1d_bwd_weight seg %d: dW must sit at a multiple of 16 channels of a "
                    "64-byte aligned packed gradient", i);
        LDM_REQUIRE(LDM_ALIGNED(a->seg[i].X, 4), LDM_EALIGN,
                    "conv1d_bwd_weight seg %d: X must be 4-byte aligned", i);
        tiles += round16(a->seg[i].C) / 16;
    }
    LDM_REQUIRE(tiles <= 65535, LDM_EINVAL, "conv1d_bwd_weight: too many channels");
    LDM_REQUIRE(LDM_ALIGNED(a->dY, 4), LDM_EALIGN, "conv1d_bwd_weight: dY must be 4-byte aligned");
    LDM_REQUIRE(LDM_ALIGNED(a->dbias, 4) && LDM_ALIGNED(a->dcbias, 4) && LDM_ALIGNED(a->ws, 4),
                LDM_EALIGN, "conv1d_bwd_weight: fp32 operands must be 4-byte aligned");
    return 0;
}

void plan_bwd_weight(const ldm_conv1d_bwd_weight_args_t& a, BwdWeightK* k) {
    k->a = a;
    k->nlt = (a.L_out + kTileL - 1) / kTileL;
    k->n_units = (int64_t)a.B * k->nlt;
    int t = 0;
    int64_t off = 0;
    for (int i = 0; i < LDM_CONV_MAX_SEGS + 1; ++i) {
        k->tile0[i] = t;
        k->poff[i] = off;
        if (i < a.n_seg) {
            t += round16(a.seg[i].C) / 16;
            off += (int64_t)round16(a.Cout) * a.seg[i].ksize * round16(a.seg[i].C);
        }
    }
    k->part = off;
    k->dcb = nullptr;
    k->S = (int)(k->n_units < kMaxSplits ? k->n_units : kMaxSplits);
}

int64_t bwd_weight_ws_floats(const BwdWeightK& k) {
    const bool own_dcb = k.a.dbias && !k.a.dcbias;
    return (int64_t)k.S * k.part + (own_dcb ? (int64_t)k.a.B * k.a.Cout : 0);
}

}  // namespace
}  // namespace ldm

extern "C" int ldm_conv1d_bwd_data(const ldm_conv1d_bwd_data_args_t* a, ldm_stream_t s) {
    using namespace ldm;
    LDM_TRY(check_bwd_data(a));
    if (a->w_dtype == LDM_BF16) return launch_bwd_data<unsigned short>(*a, (hipStream_t)s);
    return launch_bwd_data<float>(*a, (hipStream_t)s);
}

extern "C" int64_t ldm_conv1d_bwd_weight_ws_floats(const ldm_conv1d_bwd_weight_args_t* a) {
    using namespace ldm;
    if (!a || a->B < 1 || a->B > 65535 || a->Cout < 1 || a->L_out < 1 || a->n_seg < 1 ||
        a->n_seg > LDM_CONV_MAX_SEGS)
        return 0;
    for (int i = 0; i < a->n_seg; ++i)
        if (a->seg[i].C < 1 || a->seg[i].ksize < 1 || a->seg[i].ksize > 4) return 0;
    BwdWeightK k;
    plan_bwd_weight(*a, &k);
    return bwd_weight_ws_floats(k);
}

extern "C" int ldm_conv1d_bwd_weight(const ldm_conv1d_bwd_weight_args_t* a, ldm_stream_t s) {
    using namespace ldm;
    LDM_TRY(check_bwd_weight(a));
    BwdWeightK k;
    plan_bwd_weight(*a, &k);
    const int64_t need = bwd_weight_ws_floats(k);
    LDM_REQUIRE(a->ws && a->ws_floats >= need, LDM_ENOSPC,
                "conv1d_bwd_weight: workspace of %lld floats needed, %lld given "
                "(ldm_conv1d_bwd_weight_ws_floats)", (long long)need,
                (long long)(a->ws ? a->ws_floats : 0));
    hipStream_t st = (hipStream_t)s;
    const dim3 grid(k.S, round16(a->Cout) / 16, k.tile0[a->n_seg]);
    hipLaunchKernelGGL(conv1d_bwd_weight_kernel, grid, dim3(256), 0, st, k);
    LDM_TRY(launch_status("ldm_conv1d_bwd_weight"));
    hipLaunchKernelGGL(conv1d_bwd_weight_reduce_kernel, dim3((unsigned)((k.part + 255) / 256)),
                       dim3(256), 0, st, k);
    LDM_TRY(launch_status("ldm_conv1d_bwd_weight (reduce)"));
    if (a->dbias || a->dcbias) {
        float* dcb = a->dcbias ? a->dcbias : a->ws + (int64_t)k.S * k.part;
        hipLaunchKernelGGL(conv1d_rowsum_kernel, dim3((unsigned)(a->B * a->Cout)), dim3(64), 0, st,
                           a->dY, a->L_out, dcb);
        LDM_TRY(launch_status("ldm_conv1d_bwd_weight (row sums)"));
        if (a->dbias) {
            hipLaunchKernelGGL(conv1d_dbias_kernel, dim3((a->Cout + 63) / 64), dim3(64), 0, st,
                               (const float*)dcb, a->B, a->Cout, a->dbias);
            LDM_TRY(launch_status("ldm_conv1d_bwd_weight (dbias)"));
        }
    }
    return 0;
}
