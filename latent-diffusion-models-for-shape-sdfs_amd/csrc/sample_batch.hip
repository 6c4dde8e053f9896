// The DDPM reverse loop for sampling batches above the GEMV kernels' 16 (ldm_sample_batch): the
// inference form of the training forward (denoiser_train.hip forward()) on the matrix-core
// engine (ldm_gemm_bf16), run once per timestep.  It differs from the training forward in four
// ways: one uniform t per step; the tabulated E_k[t] (= U_k temb(t) + b_k) as the block bias
// instead of the time MLP and a second K segment; no saved activations; and the A8 update fused
// into the out-projection's epilogue (gemm_tile.h DdpmEpi), which also writes the bf16 copy of
// x that is the next step's operand.
//
// Launches: one pack (x[0] -> bf16 [Bp][D], Bp = ceil(B / 64) 64, padding rows zero), then per
// step 2 + n_blocks GEMMs:
//   in-projection   xb W_in^T + b_in                 STORE       -> h_f[0] (fp32), h_b[0] (bf16)
//   block k         h_b[k&1] W_k^T + E_k[t]          RESID_SILU  R = h_f[k&1] -> h_f[(k+1)&1]
//                   (one segment, K = H, ldb = 2H)               (not after the last), h_b[(k+1)&1]
//   out-projection  h_b[nb&1] W_out^T + b_out        DDPM step   -> x[cur^1] (fp32), xb (bf16)
// Every launch is an ordinary GEMM launch on the caller's stream: no grid barrier, no spin wait,
// no status word, no synchronisation, no allocation, no host read of device data (the schedule
// tables are read on the device at t), so the call can be captured into a graph as a linear
// chain of kernel nodes.
//
// Batch invariance: every launch runs on ONE tile configuration fixed by the network (D, H),
// never by B: 64 x 64 tiles, k walked in order from 0 by v_mfma_f32_32x32x16_bf16 (tile 24's two
// k-groups split the k-steps by a fixed pattern and are summed group 0 + group 1).  An output
// element's sum therefore depends on its row's operands alone, not on B nor on where the row
// sits in its tile, and the epilogues are element-wise: a row's latents are bitwise the same at
// any batch size.
#include "ldm_internal.h"
#include "gemm_tile.h"

#include <string.h>

namespace ldm {

int gemm_bf16(const ldm_gemm_args_t& a, hipStream_t s);
int gemm_bf16_ddpm(const ldm_gemm_args_t& a, const gtile::DdpmEpi& e, hipStream_t s);

namespace {

typedef unsigned short bf16_t;

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// x fp32 [B][D] -> bf16 [Bp][D], rows b >= B zero.  One thread per element.
__global__ __launch_bounds__(256) void pack_x_kernel(const float* __restrict__ x, int B, int Bp,
                                                     int D, bf16_t* __restrict__ xb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)Bp * D) return;
    const float v = i < (int64_t)B * D ? x[i] : 0.f;
    xb[i] = (bf16_t)(gtile::pack2_bf16(v, 0.f) & 0xffffu);
}

struct BatchWs {
    int Bp;
    bf16_t* xb;          // [Bp][D]
    float* h_f[2];       // [Bp][H] fp32 residual stream, ping-pong
    bf16_t* h_b[2];      // [Bp][H] its bf16 operand copy
    size_t bytes;
};

BatchWs layout(const ldm_denoiser_t* w, int B, void* base) {
    BatchWs L = {};
    L.Bp = (B + 63) / 64 * 64;
    size_t off = 0;
    char* b = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) -> void* {
        void* p = b ? b + off : nullptr;
        off = align256(off + bytes);
        return p;
    };
    const size_t Bp = L.Bp, D = w->D, H = w->H;
    L.xb = reinterpret_cast<bf16_t*>(take(Bp * D * 2));
    for (int i = 0; i < 2; ++i) L.h_f[i] = reinterpret_cast<float*>(take(Bp * H * 4));
    for (int i = 0; i < 2; ++i) L.h_b[i] = reinterpret_cast<bf16_t*>(take(Bp * H * 2));
    L.bytes = off;
    return L;
}

// The largest batch: the operand DMA addresses a tile's rows by 32-bit byte offsets from the
// operand's base (gemm_tile.h TileSrc), so a padded bf16 operand stays within 2^32 bytes:
// Bp * max(D, H) <= 2^31 elements.  (Epilogue and noise offsets are 64-bit.)
int max_batch(const ldm_denoiser_t* w) {
    const int64_t wide = w->H > w->D ? w->H : w->D;
    return (int)(((int64_t)1 << 31) / wide / 64 * 64);
}

int check_desc(const ldm_denoiser_t* w, int B) {
    LDM_REQUIRE(w && w->abi_version == LDM_ABI_VERSION, LDM_EINVAL,
                "ldm_sample_batch: bad denoiser descriptor / ABI version");
    LDM_REQUIRE(w->dtype == LDM_BF16, LDM_ENOSYS,
                "ldm_sample_batch runs bf16 weights (got dtype %d); fp32 sampling is "
                "ldm_sample_step / ldm_sample_loop at B <= 16", w->dtype);
    LDM_REQUIRE(w->D >= 64 && w->H >= 64 && w->D % 64 == 0 && w->H % 64 == 0 &&
                    w->n_blocks >= 1 && w->n_blocks <= LDM_MAX_BLOCKS && w->T >= 1,
                LDM_EINVAL, "ldm_sample_batch: D and H must be multiples of 64 (D=%d H=%d), "
                "1..%d blocks", w->D, w->H, LDM_MAX_BLOCKS);
    LDM_REQUIRE(w->w_in && w->b_in && w->w_out && w->b_out, LDM_EINVAL,
                "ldm_sample_batch: weight pointer missing");
    for (int k = 0; k < w->n_blocks; ++k)
        LDM_REQUIRE(w->w_blk[k] && w->e_tab[k], LDM_EINVAL,
                    "ldm_sample_batch: block %d weights or E table missing", k);
    LDM_REQUIRE(B >= 1, LDM_EINVAL, "ldm_sample_batch: batch %d", B);
    LDM_REQUIRE(B <= max_batch(w), LDM_ENOSYS,
                "ldm_sample_batch: batch %d above %d (32-bit operand offsets)", B, max_batch(w));
    return 0;
}

ldm_gemm_prob_t prob(int M, int N, int M_valid) {
    ldm_gemm_prob_t p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.M_valid = M_valid; p.mode = LDM_GEMM_STORE; p.scale = 1.f;
    return p;
}
void seg(ldm_gemm_prob_t& p, const void* A, int64_t lda, const void* B, int64_t ldb, int K) {
    ldm_gemm_seg_t& s = p.seg[p.n_seg++];
    s.A = A; s.B = B; s.lda = lda; s.ldb = ldb; s.K = K;
}

}  // namespace
}  // namespace ldm

using namespace ldm;

extern "C" int ldm_sample_batch_supported(const ldm_denoiser_t* w, int B) {
    return check_desc(w, B) == 0;
}

extern "C" size_t ldm_sample_batch_ws_bytes(const ldm_denoiser_t* w, int B) {
    if (check_desc(w, B) != 0) return 0;
    return layout(w, B, nullptr).bytes;
}

extern "C" int ldm_sample_batch(const ldm_denoiser_t* w, const ldm_sched_t* sc, float* x,
                                const float* noise, int t_hi, int steps, int B, void* ws,
                                size_t ws_bytes, ldm_stream_t stream) {
    LDM_TRY(check_desc(w, B));
    LDM_REQUIRE(sc && sc->abi_version == LDM_ABI_VERSION && sc->c1 && sc->c2 && sc->sigma,
                LDM_EINVAL, "ldm_sample_batch: bad schedule descriptor");
    LDM_REQUIRE(t_hi >= 0 && t_hi < sc->T && t_hi < w->T && steps >= 1 && steps <= t_hi + 1,
                LDM_EINVAL, "ldm_sample_batch: steps %d from t_hi %d outside the schedule "
                "(T = %d, tables %d)", steps, t_hi, sc->T, w->T);
    LDM_REQUIRE(x && ws && (noise || t_hi == 0), LDM_EINVAL,
                "ldm_sample_batch: null x / noise / ws");
    const BatchWs L = layout(w, B, ws);
    LDM_REQUIRE(ws_bytes >= L.bytes, LDM_ENOSPC,
                "ldm_sample_batch: workspace %zu bytes, needs %zu", ws_bytes, L.bytes);
    LDM_REQUIRE(LDM_ALIGNED(x, 16) && LDM_ALIGNED(noise, 16) && LDM_ALIGNED(ws, 256), LDM_EALIGN,
                "ldm_sample_batch: x / noise must be 16-byte, ws 256-byte aligned");
    LDM_REQUIRE(LDM_ALIGNED(w->w_in, 16) && LDM_ALIGNED(w->w_out, 16), LDM_EALIGN,
                "ldm_sample_batch: weights must be 16-byte aligned");
    for (int k = 0; k < w->n_blocks; ++k)
        LDM_REQUIRE(LDM_ALIGNED(w->w_blk[k], 16), LDM_EALIGN,
                    "ldm_sample_batch: weights must be 16-byte aligned");

    hipStream_t s = (hipStream_t)stream;
    const int D = w->D, H = w->H, nb = w->n_blocks, Bp = L.Bp;
    // one tile per network, whatever B (batch invariance, see the head of this file): the
    // training forward's 128-deep two-k-group tile where every K allows it, else its 64-deep one
    const int tile = (D % 128 == 0 && H % 128 == 0) ? 24 : 4;
    const size_t BD = (size_t)B * D;

    const int64_t n_pack = (int64_t)Bp * D;
    hipLaunchKernelGGL(pack_x_kernel, dim3((unsigned)((n_pack + 255) / 256)), dim3(256), 0, s, x,
                       B, Bp, D, L.xb);
    LDM_TRY(launch_status("ldm_sample_batch (pack)"));

    ldm_gemm_args_t a;
    int cur = 0;
    for (int t = t_hi; t > t_hi - steps; --t) {
        memset(&a, 0, sizeof(a));
        a.n_prob = 1; a.tile = tile;
        ldm_gemm_prob_t& fi = a.prob[0];                          // h0 = Win bf(x) + bin
        fi = prob(Bp, H, B);
        seg(fi, L.xb, D, w->w_in, D, D);
        fi.bias = w->b_in;
        fi.C = L.h_f[0]; fi.ldc = H; fi.Cb = L.h_b[0]; fi.ldcb = H;
        LDM_TRY(gemm_bf16(a, s));
        for (int k = 0; k < nb; ++k) {                            // h <- h + SiLU(W_k bf(h) + E_k[t])
            memset(&a, 0, sizeof(a));
            a.n_prob = 1; a.tile = tile;
            ldm_gemm_prob_t& fb = a.prob[0];
            fb = prob(Bp, H, B);
            seg(fb, L.h_b[k & 1], H, w->w_blk[k], 2 * (int64_t)H, H);
            fb.mode = LDM_GEMM_RESID_SILU;
            fb.bias = w->e_tab[k] + (size_t)t * H;
            fb.R = L.h_f[k & 1]; fb.ldr = H;
            if (k + 1 < nb) { fb.C = L.h_f[(k + 1) & 1]; fb.ldc = H; }
            fb.Cb = L.h_b[(k + 1) & 1]; fb.ldcb = H;
            LDM_TRY(gemm_bf16(a, s));
        }
        memset(&a, 0, sizeof(a));                                 // eps -> A8 update -> x, bf(x)
        a.n_prob = 1; a.tile = tile;
        ldm_gemm_prob_t& fo = a.prob[0];
        fo = prob(Bp, D, B);
        seg(fo, L.h_b[nb & 1], H, w->w_out, H, H);
        fo.bias = w->b_out;
        gtile::DdpmEpi e = {};
        e.x_in = x + cur * BD;
        e.z = t > 0 ? noise + (size_t)t * BD : nullptr;
        e.x_out = x + (cur ^ 1) * BD;
        e.xb = L.xb;
        e.c1 = sc->c1; e.c2 = sc->c2; e.sg = sc->sigma;
        e.ld = D; e.ldb = D; e.t = t;
        LDM_TRY(gemm_bf16_ddpm(a, e, s));
        cur ^= 1;
    }
    return 0;
}
