// Decoder input gradients with frozen weights: for B shapes x P points, one
// launch runs the DeepSDF decoder forward AND the backward of its pre-tanh output with respect to
// the input [z || xyz] -- z through the folded biases beta (rule A2), so d/dz is the transposed
// fold of d/dbeta.  With the weights fixed the backward needs no activations, only the ReLU sign
// bits: a tile's whole forward and backward stay on one CU, weights streaming from L2.
//
// Notation: a_l the pre-activation of layer l (fp32 accumulator), h_l = relu(a_l),
// m_l = [a_l > 0], pre = w_last . h_7 + b_last, f = tanh(pre), delta_l = d pre / d a_l,
// T the operand type (fp16 / bf16), rd = round-to-nearest-even to T.
//
// Rounding map (tests/decoder_grad_emulation.py restates it):
//   a_0     = fma chain beta_0 + Wxyz_0 xyz                 fp32, nothing rounded to T
//   a_l     = rd(W_l) rd(h_{l-1}) + b_l                     MFMA, fp32 accumulation from the fp32
//                                                           bias; l = 4 starts from the fp32
//                                                           beta_4 + Wxyz_4 xyz instead
//   pre     = sum_f w_last[f] relu(a_7[f]) + b_last         fp32, a_7 unrounded
//   delta_7 = m_7 . w_last                                  fp32
//   delta_{l-1} = m_{l-1} . (rd(W_l)^T rd(delta_l))         l = 7..1; l = 4: the h columns only
//   dxyz    = s_p (Wxyz_0^T delta_0 + Wxyz_4^T delta_4)     fp32 from the unrounded deltas
//   dbeta_i = sum_p s_p delta_i,p  (i = 0, 4)               fp32, per tile then per shape
// s_p is 1 - f^2 (gradient mode) or d loss_p / d pre (loss mode, sdf_l1_term); it is applied in
// fp32 at the outputs only, so the backward never carries a loss-scaled quantity.
//
// Work split: a tile is 64 points = 2 point chunks (n) of 32; the workgroup's 4 waves split the
// OUTPUT rows of every product, wave w rows [128w, 128w + 128) as 4 m-chunks of 32 (a 256-row
// output: [64w, 64w + 64), 2 m-chunks).  v_mfma_f32_32x32x16: A = weights (row-major [out][in]
// for the forward, the transposed copy for the backward, 16-byte global loads through a 2-step
// register ring), B = the activations / deltas in LDS as B fragments in natural k order
// ([k-step][n][lane] x 16 B, 64 KiB), accumulator rows = output features, columns = points.  A
// lane holds the same (feature, point) cells in layer l's forward and in the backward product
// that yields delta_l, so the sign bits are per-lane words: [layer][wave][lane] x 16 B, 28 KiB
// for m_0..m_6 (m_7 never reaches LDS: delta_7 is formed in place from a_7).
// A 128-point tile would need 128 + 56 KiB: it does not fit the 160 KiB of a CU.
// One workgroup per tile, a tile never straddles two shapes, a ragged tile's points past P get
// s_p = 0 and are never stored.  No atomics: per-tile partial sums, summed by
// ldm_colsum_segments in a fixed order.
#include "decoder_common.h"
#include "sdf_loss.h"

namespace ldm {
namespace {
using namespace dec;

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kGTp = 64;                            // points per tile
constexpr int kGAct = 32 * 2 * 64 * 16;             // B fragments [32 k-steps][2 n][64 lanes]
constexpr int kGMask = 7 * 4 * 64 * 16;             // sign bits m_0..m_6 [7][4 waves][64 lanes]
constexpr int kGRed = 4 * 2 * 64 * 4 * 4;           // [wave][n][lane][gx, gy, gz, pre] fp32
constexpr int kGLds = kGAct + kGMask + kGRed;
static_assert(kGLds <= 160 * 1024, "LDS");

struct GArgs {
    const void* w[8];        // [1..7]: T row-major [M_l][K_l] (padded to 256 / 512)
    const void* wt[8];       // [1..7]: T row-major [K_l][M_l]
    const float* bias;       // [8][512], rows 0 and 4 unused
    const float* wxyz;       // [2][512][3]
    const float* w_last;     // [512] natural order
    const float* beta;       // [B][2][512]
    const float* xyz;        // [B][P][3]
    const float* gt;         // [B][P] or NULL (gradient mode)
    float* sdf;              // [B][P]
    float* dxyz;             // [B][P][3] or NULL
    float* part;             // [n_tiles][2][512]
    float* loss_part;        // [n_tiles]
    float b_last, delta, scale;
    int npts, tiles_per_shape, n_tiles, B;
};

// Every global read of the kernel's tables is a raw buffer load: the base in scalar registers, a
// 32-bit lane offset and constant offsets.  Plain global loads made the compiler keep a 64-bit
// VGPR address per load site live across the layers, and spill them (decoder_fs.hip, FSrc).
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, 0x7ffffff0, 0x00020000);
}
__device__ __forceinline__ u32x4 bld(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 bldf(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

constexpr int kGD = 2;      // k-steps of A fragments in flight per wave (register ring depth)

// acc[i][n] (m-chunk i, point chunk n) += W[rows of this wave][:] x the LDS B fragments.
// Lane (h = lane >> 5, r = lane & 31) holds A[row r][k = 8h + j] of each m-chunk: 16 bytes at
// W[(32 MI wave + 32 i + r) ldk + 16 ks + 8h].  nks (k-steps of 16) is a multiple of kGD.
// ZERO: the product starts from zero accumulators -- the first k-step's MFMAs take the constant
// as their C operand (a zero vector kept in registers for that was spilled).
template <typename T, int MI, bool ZERO>
__device__ __forceinline__ void gemm(const char* smem, const void* Wv, int ldk, int nks, int wave,
                                     int lane, f32x16 (&acc)[4][2]) {
    const rsrc_t rw = make_rsrc(Wv);
    const uint32_t voff = (uint32_t)((32 * MI * wave + (lane & 31)) * ldk + 8 * (lane >> 5)) * 2u;
    const uint32_t istep = (uint32_t)(32 * ldk) * 2u;      // one m-chunk down
    const u32x4* bl = reinterpret_cast<const u32x4*>(smem) + lane;
    u32x4 ring[kGD][MI];
#pragma unroll
    for (int r = 0; r < kGD; ++r)
#pragma unroll
        for (int i = 0; i < MI; ++i) ring[r][i] = bld(rw, voff + 32u * r, istep * i);
    // k-steps ks .. ks + kGD - 1 from the ring, refilled for ks + kGD ..
    auto group = [&](int ks, bool first) {
        const bool more = ks + kGD < nks;
#pragma unroll
        for (int r = 0; r < kGD; ++r) {
            const u32x4 b0 = bl[((ks + r) * 2 + 0) * 64];
            const u32x4 b1 = bl[((ks + r) * 2 + 1) * 64];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                if (first && r == 0) {
                    acc[i][0] = Elem<T>::mfma(ring[r][i], b0, f32x16{});
                    acc[i][1] = Elem<T>::mfma(ring[r][i], b1, f32x16{});
                } else {
                    acc[i][0] = Elem<T>::mfma(ring[r][i], b0, acc[i][0]);
                    acc[i][1] = Elem<T>::mfma(ring[r][i], b1, acc[i][1]);
                }
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    ring[r][i] = bld(rw, voff + 32u * r, istep * i + 32u * (uint32_t)(ks + kGD));
            }
        }
    };
    group(0, ZERO);
#pragma unroll 1
    for (int ks = kGD; ks < nks; ks += kGD) group(ks, false);
}

// The wave's accumulators, rounded to T (RELU: after ReLU), into the B-fragment buffer.
// Register v = 4q + e of lane (h, c) is row 8q + 4h + e of its m-chunk: k-step
// 2 MI wave + 2i + (q >> 1), lane half q & 1, elements 4h .. 4h + 3 of column c -- 8 bytes.
template <typename T, int MI, bool RELU>
__device__ __forceinline__ void store_frags(char* smem, int wave, int lane,
                                            const f32x16 (&acc)[4][2]) {
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ks = 2 * MI * wave + 2 * i + (q >> 1);
                u32x2 v;
                v[0] = Elem<T>::pack(acc[i][n][4 * q], acc[i][n][4 * q + 1]);
                v[1] = Elem<T>::pack(acc[i][n][4 * q + 2], acc[i][n][4 * q + 3]);
                if (RELU) {
                    v[0] = relu2(v[0]);
                    v[1] = relu2(v[1]);
                }
                *reinterpret_cast<u32x2*>(smem + ((ks * 2 + n) * 64 + 32 * (q & 1) + c) * 16 +
                                          8 * h) = v;
            }
}

// m = [a > 0] of the wave's accumulators: word i, bit 16 n + v
template <int MI>
__device__ __forceinline__ u32x4 sign_bits(const f32x16 (&acc)[4][2]) {
    u32x4 m = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        unsigned w = 0;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int v = 0; v < 16; ++v) w |= (acc[i][n][v] > 0.f ? 1u : 0u) << (16 * n + v);
        m[i] = w;
    }
    return m;
}

template <int MI>
__device__ __forceinline__ void apply_bits(f32x16 (&acc)[4][2], const u32x4 m) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                acc[i][n][v] = ((m[i] >> (16 * n + v)) & 1u) ? acc[i][n][v] : 0.f;
}

__device__ __forceinline__ u32x4* mask_slot(char* smem, int layer, int wave, int lane) {
    return reinterpret_cast<u32x4*>(smem + kGAct) + (layer * 4 + wave) * 64 + lane;
}

// acc = bias[row] for the wave's rows (row = 32 MI wave + 32 i + 8q + 4h + e)
template <int MI>
__device__ __forceinline__ void init_bias(f32x16 (&acc)[4][2], const float* __restrict__ bias,
                                          int wave, int lane) {
    const rsrc_t rb = make_rsrc(bias);
    const uint32_t voff = (uint32_t)(lane >> 5) * 16u;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 b = bldf(rb, voff, (uint32_t)(32 * MI * wave + 32 * i + 8 * q) * 4u);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[i][0][4 * q + e] = b[e];
                acc[i][1][4 * q + e] = b[e];
            }
            __builtin_amdgcn_sched_barrier(0);   // one row group's loads in flight, not all 16
        }
}

// acc = beta[row] + Wxyz[row] . xyz of the lane's two points, an fp32 fma chain (x, y, z);
// layers 0 and 4 are 512 wide: row = 128 wave + 32 i + 8q + 4h + e
__device__ __forceinline__ void init_xyz(f32x16 (&acc)[4][2], const float* __restrict__ beta,
                                         const float* __restrict__ wxyz, int wave, int lane,
                                         const float (&px)[2], const float (&py)[2],
                                         const float (&pz)[2]) {
    const rsrc_t rb = make_rsrc(beta), rx = make_rsrc(wxyz);
    const uint32_t vb = (uint32_t)(lane >> 5) * 16u, vx = (uint32_t)(lane >> 5) * 48u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t row = (uint32_t)(128 * wave + 32 * i + 8 * q);   // + 4h: the lane part
            const f32x4 b = bldf(rb, vb, row * 4u);
            const f32x4 w0 = bldf(rx, vx, row * 12u), w1 = bldf(rx, vx + 16u, row * 12u),
                        w2 = bldf(rx, vx + 32u, row * 12u);
            const float w[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1],
                                 w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    float v = b[e];
                    v = fmaf(w[3 * e + 0], px[n], v);
                    v = fmaf(w[3 * e + 1], py[n], v);
                    v = fmaf(w[3 * e + 2], pz[n], v);
                    acc[i][n][4 * q + e] = v;
                }
            __builtin_amdgcn_sched_barrier(0);   // keep the loads of one row group live at a time
        }
}

// One of delta_0 / delta_4 (in acc, fp32) into the outputs: g[n][axis] += Wxyz^T delta for the
// lane's rows, and the tile's sum over the points of s_p delta[row][p] -> part[row].  The point
// sum: the lane's two points, then an xor butterfly over the 32 columns of its lane half (every
// lane ends with the same value); lane column c < 16 keeps register v = c and stores its row.
__device__ __forceinline__ void delta_out(const f32x16 (&acc)[4][2],
                                          const float* __restrict__ wxyz, float* __restrict__ part,
                                          int wave, int lane, const float (&s)[2],
                                          float (&g)[2][3]) {
    const int h = lane >> 5, c = lane & 31;
    const rsrc_t rx = make_rsrc(wxyz);
    const uint32_t vx = (uint32_t)h * 48u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float mine = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t row = (uint32_t)(128 * wave + 32 * i + 8 * q);   // + 4h: the lane part
            const f32x4 w0 = bldf(rx, vx, row * 12u), w1 = bldf(rx, vx + 16u, row * 12u),
                        w2 = bldf(rx, vx + 32u, row * 12u);
            const float w[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1],
                                 w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = 4 * q + e;
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int a = 0; a < 3; ++a) g[n][a] = fmaf(w[3 * e + a], acc[i][n][v], g[n][a]);
                float t = fmaf(s[1], acc[i][1][v], s[0] * acc[i][0][v]);
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) t += __shfl_xor(t, o);
                mine = (c == v) ? t : mine;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (c < 16) part[128 * wave + 32 * i + (c & 3) + 8 * (c >> 2) + 4 * h] = mine;
    }
}

template <typename T, int S>
__global__ __launch_bounds__(256, 1) void dec_grad_kernel(GArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kGLds];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, c = lane & 31;
    const int tile = blockIdx.x;
    LDM_DASSERT(tile < a.n_tiles);
    if (tile >= a.n_tiles) return;
    const int shape = tile / a.tiles_per_shape;
    const int local = tile - shape * a.tiles_per_shape;
    LDM_DASSERT(shape >= 0 && shape < a.B && local * kGTp < a.npts);
    float* red = reinterpret_cast<float*>(smem + kGAct + kGMask);

    // the lane's two points: 32 n + c of the tile, a ragged tile's tail clamped to the last point
    float px[2], py[2], pz[2];
    bool valid[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        int pt = local * kGTp + 32 * n + c;
        valid[n] = pt < a.npts;
        if (!valid[n]) pt = a.npts - 1;
        LDM_DASSERT(pt >= 0 && pt < a.npts);
        const float* q = a.xyz + ((size_t)shape * a.npts + pt) * 3;
        px[n] = q[0];
        py[n] = q[1];
        pz[n] = q[2];
    }
    const float* beta0 = a.beta + (size_t)shape * 2 * kHidden;
    const float* beta4 = beta0 + kHidden;
    constexpr int MI3 = S == 256 ? 2 : 4;       // m-chunks per wave of the skip-wide h_3

    f32x16 acc[4][2];
    // ---- forward
    init_xyz(acc, beta0, a.wxyz, wave, lane, px, py, pz);
    *mask_slot(smem, 0, wave, lane) = sign_bits<4>(acc);
    store_frags<T, 4, true>(smem, wave, lane, acc);
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l <= 2; ++l) {
        init_bias<4>(acc, a.bias + l * kHidden, wave, lane);
        gemm<T, 4, false>(smem, a.w[l], kHidden, kHidden / 16, wave, lane, acc);
        *mask_slot(smem, l, wave, lane) = sign_bits<4>(acc);
        __syncthreads();
        store_frags<T, 4, true>(smem, wave, lane, acc);
        __syncthreads();
    }
    init_bias<MI3>(acc, a.bias + 3 * kHidden, wave, lane);
    gemm<T, MI3, false>(smem, a.w[3], kHidden, kHidden / 16, wave, lane, acc);
    *mask_slot(smem, 3, wave, lane) = sign_bits<MI3>(acc);
    __syncthreads();
    store_frags<T, MI3, true>(smem, wave, lane, acc);
    __syncthreads();
    init_xyz(acc, beta4, a.wxyz + 3 * kHidden, wave, lane, px, py, pz);
    gemm<T, 4, false>(smem, a.w[4], S, S / 16, wave, lane, acc);
    *mask_slot(smem, 4, wave, lane) = sign_bits<4>(acc);
    __syncthreads();
    store_frags<T, 4, true>(smem, wave, lane, acc);
    __syncthreads();
#pragma unroll 1
    for (int l = 5; l <= 6; ++l) {
        init_bias<4>(acc, a.bias + l * kHidden, wave, lane);
        gemm<T, 4, false>(smem, a.w[l], kHidden, kHidden / 16, wave, lane, acc);
        *mask_slot(smem, l, wave, lane) = sign_bits<4>(acc);
        __syncthreads();
        store_frags<T, 4, true>(smem, wave, lane, acc);
        __syncthreads();
    }
    init_bias<4>(acc, a.bias + 7 * kHidden, wave, lane);
    gemm<T, 4, false>(smem, a.w[7], kHidden, kHidden / 16, wave, lane, acc);

    // ---- pre = w_last . relu(a_7) + b_last, and delta_7 = m_7 . w_last in place
    {
        float part[2] = {0.f, 0.f};
        const rsrc_t rl = make_rsrc(a.w_last);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 wl = bldf(rl, (uint32_t)h * 16u,
                                      (uint32_t)(128 * wave + 32 * i + 8 * q) * 4u);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const float x = acc[i][n][4 * q + e];
                        part[n] = fmaf(wl[e], fmaxf(x, 0.f), part[n]);
                        acc[i][n][4 * q + e] = x > 0.f ? wl[e] : 0.f;
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        red[((wave * 2 + 0) * 64 + lane) * 4 + 3] = part[0];
        red[((wave * 2 + 1) * 64 + lane) * 4 + 3] = part[1];
    }
    __syncthreads();          // the partials are out; every wave is done reading h_6
    store_frags<T, 4, false>(smem, wave, lane, acc);
    float f[2], s[2], term[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        // the 8 partials of point 32 n + c (4 waves x 2 lane halves) in a fixed order
        float pre = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            pre += red[((w * 2 + n) * 64 + c) * 4 + 3] + red[((w * 2 + n) * 64 + c + 32) * 4 + 3];
        pre += a.b_last;
        term[n] = 0.f;
        if (a.gt) {
            int pt = local * kGTp + 32 * n + c;
            if (pt >= a.npts) pt = a.npts - 1;
            term[n] = sdf_l1_term(pre, a.gt[(size_t)shape * a.npts + pt], a.delta, a.scale, s[n]);
            f[n] = tanhf(pre);
        } else {
            f[n] = tanhf(pre);
            s[n] = fmaf(-f[n], f[n], 1.f);
        }
        if (!valid[n]) {          // a ragged tail's point contributes nothing to any sum
            s[n] = 0.f;
            term[n] = 0.f;
        }
    }
    __syncthreads();

    // ---- backward: delta_{l-1} = m_{l-1} . (W_l^T rd(delta_l))
    float g[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    float* part = a.part + (size_t)tile * 2 * kHidden;
#pragma unroll 1
    for (int l = 7; l >= 5; --l) {
        gemm<T, 4, true>(smem, a.wt[l], kHidden, kHidden / 16, wave, lane, acc);
        apply_bits<4>(acc, *mask_slot(smem, l - 1, wave, lane));
        if (l == 5) delta_out(acc, a.wxyz + 3 * kHidden, part + kHidden, wave, lane, s, g);
        __syncthreads();
        store_frags<T, 4, false>(smem, wave, lane, acc);
        __syncthreads();
    }
    // l = 4: only the h columns of W_4 -> delta_3 (skip wide)
    gemm<T, MI3, true>(smem, a.wt[4], kHidden, kHidden / 16, wave, lane, acc);
    apply_bits<MI3>(acc, *mask_slot(smem, 3, wave, lane));
    __syncthreads();
    store_frags<T, MI3, false>(smem, wave, lane, acc);
    __syncthreads();
    // l = 3: the reduction runs over the skip-wide rows of delta_3
    gemm<T, 4, true>(smem, a.wt[3], S, S / 16, wave, lane, acc);
    apply_bits<4>(acc, *mask_slot(smem, 2, wave, lane));
    __syncthreads();
    store_frags<T, 4, false>(smem, wave, lane, acc);
    __syncthreads();
#pragma unroll 1
    for (int l = 2; l >= 1; --l) {
        gemm<T, 4, true>(smem, a.wt[l], kHidden, kHidden / 16, wave, lane, acc);
        apply_bits<4>(acc, *mask_slot(smem, l - 1, wave, lane));
        if (l == 1) break;
        __syncthreads();
        store_frags<T, 4, false>(smem, wave, lane, acc);
        __syncthreads();
    }
    delta_out(acc, a.wxyz, part, wave, lane, s, g);

    // ---- outputs: thread t < 64 owns point t of the tile (n = t >> 5 = its lane half)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) red[((wave * 2 + n) * 64 + lane) * 4 + ax] = g[n][ax];
    __syncthreads();
    if (wave == 0) {
        const int n = h;
        const int pt = local * kGTp + lane;
        const float sp = n ? s[1] : s[0];
        const bool ok = pt < a.npts;
        if (ok) {
            LDM_DASSERT((size_t)shape * a.npts + pt < (size_t)a.B * a.npts);
            a.sdf[(size_t)shape * a.npts + pt] = n ? f[1] : f[0];
            if (a.dxyz) {
                float* o = a.dxyz + ((size_t)shape * a.npts + pt) * 3;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    float t = 0.f;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        t += red[((w * 2 + n) * 64 + c) * 4 + ax] +
                             red[((w * 2 + n) * 64 + c + 32) * 4 + ax];
                    o[ax] = sp * t;
                }
            }
        }
        if (a.gt) {
            float t = n ? term[1] : term[0];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o);
            if (lane == 0) a.loss_part[tile] = t;
        }
    }
}

// loss = scale * sum of the tile partials, one workgroup, fixed order
__global__ __launch_bounds__(256) void grad_loss_kernel(const float* __restrict__ part, int n,
                                                        float scale, float* __restrict__ loss) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = scale * red[0];
}

// The transposed fold: dz[b][k] = sum_f wz[0][f][k] dbeta[b][0][f] + wz[1][f][k] dbeta[b][1][f],
// summed in fp64 (the fp32 products are exact there) and rounded once, as fold_kernel does.
__global__ void fold_bwd_kernel(const float* __restrict__ wz, const float* __restrict__ dbeta,
                                int B, int L, float* __restrict__ dz) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= B * L) return;
    const int k = id % L, b = id / L;
    const float* d = dbeta + (size_t)b * 2 * kHidden;
    double acc = 0.0;
    for (int f = 0; f < 2 * kHidden; ++f) acc = fma((double)wz[(size_t)f * L + k], (double)d[f], acc);
    dz[id] = (float)acc;
}

// tiles of a launch, 0 when the sizes are invalid
long long grad_tiles(int B, int P) {
    if (B < 1 || P < 1 || B > 65535 || (long long)B * P >= (1ll << 31)) return 0;
    return (long long)B * ((P + kGTp - 1) / kGTp);
}

int check_grad_desc(const ldm_decoder_grad_t* w, const char* what) {
    LDM_REQUIRE(w != nullptr, LDM_EINVAL, "%s: descriptor is NULL", what);
    LDM_REQUIRE(w->abi_version == LDM_ABI_VERSION, LDM_EINVAL, "%s: abi_version %d != %d", what,
                w->abi_version, LDM_ABI_VERSION);
    LDM_REQUIRE(w->dtype != LDM_F32, LDM_ENOSYS, "%s: there is no fp32 gradient kernel", what);
    LDM_REQUIRE(w->dtype == LDM_BF16 || w->dtype == LDM_F16, LDM_EINVAL, "%s: bad dtype %d", what,
                w->dtype);
    LDM_REQUIRE(w->skip_width == 253 || w->skip_width == 512, LDM_ENOSYS,
                "%s: skip_width must be 253 or 512 (got %d)", what, w->skip_width);
    LDM_REQUIRE(w->latent_dim >= 1, LDM_EINVAL, "%s: latent_dim %d < 1", what, w->latent_dim);
    return 0;
}

template <typename T>
void launch_grad(const GArgs& a, int skip_width, hipStream_t s) {
    if (skip_width == 253)
        hipLaunchKernelGGL((dec_grad_kernel<T, 256>), dim3(a.n_tiles), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((dec_grad_kernel<T, 512>), dim3(a.n_tiles), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" size_t ldm_decoder_grad_ws_bytes(int B, int P, int dtype) {
    const long long t = grad_tiles(B, P);
    if (t == 0 || (dtype != LDM_BF16 && dtype != LDM_F16)) return 0;
    return (size_t)t * 2 * kHidden * sizeof(float) + up256((size_t)t * sizeof(float));
}

extern "C" int ldm_decoder_points_grad(const ldm_decoder_grad_t* w, const float* beta,
                                       const float* xyz, int B, int P, const float* gt,
                                       float delta, float scale, float* sdf_out, float* dxyz_out,
                                       float* dbeta_out, float* loss_out, void* ws,
                                       size_t ws_bytes, ldm_stream_t s) {
    const char* what = "ldm_decoder_points_grad";
    LDM_TRY(check_grad_desc(w, what));
    for (int l = 1; l < 8; ++l) {
        LDM_REQUIRE(w->w[l] && w->wt[l], LDM_EINVAL, "%s: weights of layer %d are NULL", what, l);
        LDM_REQUIRE(LDM_ALIGNED(w->w[l], 16) && LDM_ALIGNED(w->wt[l], 16), LDM_EALIGN,
                    "%s: weights of layer %d must be 16-byte aligned", what, l);
    }
    LDM_REQUIRE(w->bias && w->wxyz && w->w_last, LDM_EINVAL, "%s: bias / wxyz / w_last NULL",
                what);
    LDM_REQUIRE(LDM_ALIGNED(w->bias, 16) && LDM_ALIGNED(w->wxyz, 16) && LDM_ALIGNED(w->w_last, 16),
                LDM_EALIGN, "%s: bias / wxyz / w_last must be 16-byte aligned", what);
    LDM_REQUIRE(B >= 1 && P >= 1, LDM_EINVAL, "%s: empty call (B=%d, P=%d)", what, B, P);
    LDM_REQUIRE(B <= 65535, LDM_EINVAL, "%s: B = %d > 65535 shapes", what, B);
    LDM_REQUIRE((long long)B * P < (1ll << 31), LDM_EINVAL, "%s: B*P too large", what);
    LDM_REQUIRE(beta && xyz && sdf_out, LDM_EINVAL, "%s: beta / xyz / sdf_out NULL", what);
    LDM_REQUIRE(LDM_ALIGNED(beta, 16) && LDM_ALIGNED(xyz, 4) && LDM_ALIGNED(sdf_out, 4) &&
                    LDM_ALIGNED(gt, 4) && LDM_ALIGNED(dxyz_out, 4) && LDM_ALIGNED(dbeta_out, 4) &&
                    LDM_ALIGNED(loss_out, 4),
                LDM_EALIGN, "%s: misaligned buffers (beta: 16 bytes)", what);
    if (gt) {
        LDM_REQUIRE(delta > 0.f, LDM_EINVAL, "%s: clamp distance must be > 0 (got %g)", what,
                    (double)delta);
        LDM_REQUIRE(scale == scale, LDM_EINVAL, "%s: scale is NaN", what);
    } else {
        LDM_REQUIRE(loss_out == nullptr, LDM_EINVAL, "%s: loss_out needs gt (loss mode)", what);
    }
    const size_t need = ldm_decoder_grad_ws_bytes(B, P, w->dtype);
    LDM_REQUIRE(ws != nullptr && ws_bytes >= need, LDM_ENOSPC,
                "%s: workspace too small: need %zu bytes, got %zu", what, need,
                ws ? ws_bytes : (size_t)0);
    LDM_REQUIRE(LDM_ALIGNED(ws, 256), LDM_EALIGN, "%s: the workspace must be 256-byte aligned",
                what);
    GArgs a;
    for (int l = 0; l < 8; ++l) {
        a.w[l] = w->w[l];
        a.wt[l] = w->wt[l];
    }
    a.bias = w->bias;
    a.wxyz = w->wxyz;
    a.w_last = w->w_last;
    a.beta = beta;
    a.xyz = xyz;
    a.gt = gt;
    a.sdf = sdf_out;
    a.dxyz = dxyz_out;
    a.b_last = w->b_last;
    a.delta = delta;
    a.scale = scale;
    a.npts = P;
    a.tiles_per_shape = (P + kGTp - 1) / kGTp;
    a.n_tiles = B * a.tiles_per_shape;
    a.B = B;
    a.part = reinterpret_cast<float*>(ws);
    a.loss_part = a.part + (size_t)a.n_tiles * 2 * kHidden;
    hipStream_t st = (hipStream_t)s;
    if (w->dtype == LDM_BF16) launch_grad<__bf16>(a, w->skip_width, st);
    else launch_grad<_Float16>(a, w->skip_width, st);
    LDM_TRY(launch_status(what));
    // the second, deterministic pass: per shape, the tile partials in a fixed order
    if (dbeta_out)
        LDM_TRY(ldm_colsum_segments(a.part, B, a.tiles_per_shape, 2 * kHidden, dbeta_out, 0, s));
    if (loss_out) {
        hipLaunchKernelGGL(grad_loss_kernel, dim3(1), dim3(256), 0, st, a.loss_part, a.n_tiles,
                           scale, loss_out);
        LDM_TRY(launch_status("ldm_decoder_points_grad(loss)"));
    }
    return 0;
}

extern "C" int ldm_decoder_fold_bwd(const ldm_decoder_grad_t* w, const float* dbeta, int B,
                                    float* dz_out, ldm_stream_t s) {
    const char* what = "ldm_decoder_fold_bwd";
    LDM_TRY(check_grad_desc(w, what));
    LDM_REQUIRE(w->wz != nullptr, LDM_EINVAL, "%s: wz NULL", what);
    LDM_REQUIRE(dbeta && dz_out, LDM_EINVAL, "%s: dbeta / dz_out NULL", what);
    LDM_REQUIRE(B >= 1 && (long long)B * w->latent_dim < (1ll << 31), LDM_EINVAL,
                "%s: bad B = %d", what, B);
    LDM_REQUIRE(LDM_ALIGNED(w->wz, 4) && LDM_ALIGNED(dbeta, 4) && LDM_ALIGNED(dz_out, 4),
                LDM_EALIGN, "%s: misaligned buffers", what);
    const int n = B * w->latent_dim;
    hipLaunchKernelGGL(fold_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, w->wz,
                       dbeta, B, w->latent_dim, dz_out);
    return launch_status(what);
}
