/* Host-side checks of the batched sampling entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_sample_batch_supported, ldm_sample_batch_ws_bytes, ldm_sample_batch): invalid arguments
 * must return LDM_EINVAL / LDM_ENOSYS / LDM_ENOSPC / LDM_EALIGN and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_sample_batch_host.py against the
 * product library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <string.h>

#include "check.h"

static ldm_denoiser_t good_denoiser(int D, int H, int nb) {
    ldm_denoiser_t w;
    memset(&w, 0, sizeof(w));
    w.abi_version = LDM_ABI_VERSION;
    w.dtype = LDM_BF16;
    w.D = D; w.H = H; w.n_blocks = nb; w.TE = 128; w.T = 1000;
    w.w_in = fake(); w.b_in = (const float*)fake();
    w.w_out = fake(); w.b_out = (const float*)fake();
    for (int k = 0; k < nb && k < LDM_MAX_BLOCKS; ++k) {
        w.w_blk[k] = fake();
        w.b_blk[k] = (const float*)fake();
        w.e_tab[k] = (const float*)fake();
    }
    return w;
}

int main(void) {
    ldm_denoiser_t w = good_denoiser(256, 1024, 4);
    ldm_sched_t sc;
    memset(&sc, 0, sizeof(sc));
    sc.abi_version = LDM_ABI_VERSION;
    sc.T = 1000;
    sc.c1 = (const float*)fake(); sc.c2 = (const float*)fake(); sc.sigma = (const float*)fake();
    float* x = (float*)fake();
    float* noise = (float*)fake();
    void* ws = fake();
    const int B = 100;
    const size_t need = ldm_sample_batch_ws_bytes(&w, B);

    /* supported / workspace: padded to 64 rows, so one size for B = 1..64 and more at 65 */
    EXPECT(ldm_sample_batch_supported(&w, 1) == 1);
    EXPECT(ldm_sample_batch_supported(&w, 17) == 1);
    EXPECT(ldm_sample_batch_supported(&w, 1 << 20) == 1);
    EXPECT(ldm_sample_batch_supported(&w, 0) == 0);
    EXPECT(ldm_sample_batch_supported(&w, -3) == 0);
    EXPECT(ldm_sample_batch_supported(NULL, 17) == 0);
    EXPECT(need > 0 && need % 256 == 0);
    for (int b = 1; b <= 64; ++b)
        EXPECT(ldm_sample_batch_ws_bytes(&w, b) == ldm_sample_batch_ws_bytes(&w, 1));
    EXPECT(ldm_sample_batch_ws_bytes(&w, 65) > ldm_sample_batch_ws_bytes(&w, 64));
    EXPECT(ldm_sample_batch_ws_bytes(&w, 65) == ldm_sample_batch_ws_bytes(&w, 128));
    /* bf16 x, two fp32 streams, two bf16 operands of 64 padded rows */
    EXPECT(ldm_sample_batch_ws_bytes(&w, 1) ==
           (size_t)64 * (256 * 2 + 2 * 1024 * 4 + 2 * 1024 * 2));
    EXPECT(ldm_sample_batch_ws_bytes(NULL, 17) == 0);
    EXPECT(ldm_sample_batch_ws_bytes(&w, 0) == 0);
    /* the stated limit on B: 2^31 / max(D, H) rows (32-bit operand offsets) */
    EXPECT(ldm_sample_batch_supported(&w, (1 << 21)) == 1);
    EXPECT(ldm_sample_batch_supported(&w, (1 << 21) + 1) == 0);
    EXPECT(ldm_sample_batch_ws_bytes(&w, (1 << 21) + 1) == 0);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 1, (1 << 21) + 1, ws, (size_t)-1, NULL),
              LDM_ENOSYS);

    /* descriptors */
    EXPECT_RC(ldm_sample_batch(NULL, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, NULL, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    {
        ldm_denoiser_t b = w;
        b.abi_version = LDM_ABI_VERSION - 1;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        ldm_sched_t s2 = sc;
        s2.abi_version = LDM_ABI_VERSION + 1;
        EXPECT_RC(ldm_sample_batch(&w, &s2, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        s2 = sc;
        s2.sigma = NULL;
        EXPECT_RC(ldm_sample_batch(&w, &s2, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    }
    {   /* fp32 weights: not this kernel */
        ldm_denoiser_t b = w;
        b.dtype = LDM_F32;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_ENOSYS);
        EXPECT(ldm_sample_batch_supported(&b, B) == 0);
        EXPECT(ldm_sample_batch_ws_bytes(&b, B) == 0);
    }
    {   /* D or H not a multiple of 64, block counts */
        ldm_denoiser_t b = w;
        b.D = 200;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.H = 1000;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.H = 0;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.n_blocks = 0;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.n_blocks = LDM_MAX_BLOCKS + 1;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    }
    {   /* missing table / weights */
        ldm_denoiser_t b = w;
        b.e_tab[2] = NULL;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        EXPECT(ldm_sample_batch_supported(&b, B) == 0);
        b = w; b.w_blk[0] = NULL;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.w_out = NULL;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
        b = w; b.b_in = NULL;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    }
    /* batch */
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, 0, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, -1, ws, need, NULL), LDM_EINVAL);
    /* t_hi / steps outside the schedule */
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 1000, 3, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, -1, 1, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 0, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 1001, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 4, 6, B, ws, need, NULL), LDM_EINVAL);
    {   /* a schedule longer than the denoiser's tables */
        ldm_denoiser_t b = w;
        b.T = 500;
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    }
    /* NULL buffers (noise may be NULL only when the run is the t = 0 step alone) */
    EXPECT_RC(ldm_sample_batch(&w, &sc, NULL, noise, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, NULL, 999, 3, B, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, B, NULL, need, NULL), LDM_EINVAL);
    /* short workspace */
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, B, ws, need - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, B, ws, 0, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, 65, ws,
                               ldm_sample_batch_ws_bytes(&w, 64), NULL), LDM_ENOSPC);
    /* alignment */
    EXPECT_RC(ldm_sample_batch(&w, &sc, (float*)off(x, 4), noise, 999, 3, B, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, (float*)off(noise, 8), 999, 3, B, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, B, off(ws, 128), need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_sample_batch(&w, &sc, x, noise, 999, 3, B, off(ws, 16), need, NULL),
              LDM_EALIGN);
    {
        ldm_denoiser_t b = w;
        b.w_blk[1] = off((void*)w.w_blk[1], 8);
        EXPECT_RC(ldm_sample_batch(&b, &sc, x, noise, 999, 3, B, ws, need, NULL), LDM_EALIGN);
    }
    /* the public GEMM still has no DDPM-step mode */
    {
        ldm_gemm_args_t a;
        memset(&a, 0, sizeof(a));
        a.n_prob = 1;
        a.prob[0].M = 64; a.prob[0].N = 64; a.prob[0].M_valid = 64; a.prob[0].n_seg = 1;
        a.prob[0].seg[0].A = fake(); a.prob[0].seg[0].B = fake();
        a.prob[0].seg[0].lda = 64; a.prob[0].seg[0].ldb = 64; a.prob[0].seg[0].K = 64;
        a.prob[0].mode = LDM_GEMM_RELU_BWD + 1;
        EXPECT_RC(ldm_gemm_bf16(&a, NULL), LDM_EINVAL);
    }

    return check_report("sample_batch_errors");
}
