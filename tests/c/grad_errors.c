/* Host-side checks of the decoder-gradient entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_decoder_grad_ws_bytes, ldm_decoder_points_grad, ldm_decoder_fold_bwd): invalid arguments
 * must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC / LDM_ENOSYS and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_grad_host.py against the product
 * library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <math.h>
#include <string.h>

#include "check.h"

static ldm_decoder_grad_t good_desc(void) {
    ldm_decoder_grad_t d;
    memset(&d, 0, sizeof(d));
    d.abi_version = LDM_ABI_VERSION;
    d.dtype = LDM_F16;
    d.skip_width = 253;
    d.latent_dim = 256;
    for (int l = 1; l < 8; ++l) {
        d.w[l] = fake();
        d.wt[l] = fake();
    }
    d.bias = (const float*)fake();
    d.wxyz = (const float*)fake();
    d.wz = (const float*)fake();
    d.w_last = (const float*)fake();
    return d;
}

int main(void) {
    float* beta = (float*)fake();
    float* xyz = (float*)fake();
    float* gt = (float*)fake();
    float* sdf = (float*)fake();
    float* dxyz = (float*)fake();
    float* dbeta = (float*)fake();
    float* loss = (float*)fake();
    float* dz = (float*)fake();
    void* ws = fake();
    const int B = 3, P = 197;

    /* workspace: [tiles][2][512] fp32 partials + the loss partials, tiles of 64 points per shape */
    const size_t need = ldm_decoder_grad_ws_bytes(B, P, LDM_F16);
    EXPECT(need >= (size_t)B * 4 * 2 * 512 * 4 + (size_t)B * 4 * 4);
    EXPECT(ldm_decoder_grad_ws_bytes(B, P, LDM_BF16) == need);
    EXPECT(ldm_decoder_grad_ws_bytes(B, 64, LDM_F16) < ldm_decoder_grad_ws_bytes(B, 65, LDM_F16));
    EXPECT(ldm_decoder_grad_ws_bytes(0, P, LDM_F16) == 0);
    EXPECT(ldm_decoder_grad_ws_bytes(B, 0, LDM_F16) == 0);
    EXPECT(ldm_decoder_grad_ws_bytes(B, P, LDM_F32) == 0);
    EXPECT(ldm_decoder_grad_ws_bytes(65536, P, LDM_F16) == 0);
    EXPECT(ldm_decoder_grad_ws_bytes(1 << 15, 1 << 16, LDM_F16) == 0);

    ldm_decoder_grad_t d = good_desc();
#define GRAD(desc, be, xy, b, p, g, de, sd, dx, db, lo, w, wb) \
    ldm_decoder_points_grad(desc, be, xy, b, p, g, de, 0.01f, sd, dx, db, lo, w, wb, NULL)
    /* descriptor */
    EXPECT_RC(GRAD(NULL, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    {
        ldm_decoder_grad_t e = d;
        e.abi_version = LDM_ABI_VERSION - 1;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.dtype = LDM_F32;      /* no fp32 gradient kernel */
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_ENOSYS);
        e.dtype = 7;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.skip_width = 254;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_ENOSYS);
        e = d;
        e.latent_dim = 0;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.w[3] = NULL;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.wt[7] = NULL;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.wt[1] = off((void*)d.wt[1], 8);
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EALIGN);
        e = d;
        e.bias = NULL;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.w_last = NULL;
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
        e = d;
        e.wxyz = (const float*)off((void*)d.wxyz, 4);
        EXPECT_RC(GRAD(&e, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EALIGN);
    }
    /* sizes */
    EXPECT_RC(GRAD(&d, beta, xyz, 0, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, 0, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, 65536, 1, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, 1 << 15, 1 << 16, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need),
              LDM_EINVAL);
    /* buffers */
    EXPECT_RC(GRAD(&d, NULL, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, NULL, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, NULL, dxyz, dbeta, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, (float*)off(beta, 4), xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need),
              LDM_EALIGN);
    EXPECT_RC(GRAD(&d, beta, (float*)off(xyz, 2), B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need),
              LDM_EALIGN);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, (float*)off(dxyz, 1), dbeta, NULL, ws, need),
              LDM_EALIGN);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, (float*)off(dbeta, 2), NULL, ws, need),
              LDM_EALIGN);
    /* modes: the loss needs gt; loss mode needs a positive finite clamp distance */
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, loss, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, gt, 0.f, sdf, dxyz, dbeta, loss, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, gt, -1.f, sdf, dxyz, dbeta, loss, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, gt, NAN, sdf, dxyz, dbeta, loss, ws, need), LDM_EINVAL);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, (float*)off(gt, 2), 0.1f, sdf, dxyz, dbeta, loss, ws, need),
              LDM_EALIGN);
    EXPECT_RC(ldm_decoder_points_grad(&d, beta, xyz, B, P, gt, 0.1f, NAN, sdf, dxyz, dbeta, loss, ws,
                                      need, NULL), LDM_EINVAL);
    /* workspace */
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, ws, need - 1), LDM_ENOSPC);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, NULL, 0), LDM_ENOSPC);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, NULL, NULL, NULL, NULL, need), LDM_ENOSPC);
    EXPECT_RC(GRAD(&d, beta, xyz, B, P, NULL, 0.f, sdf, dxyz, dbeta, NULL, off(ws, 16), need),
              LDM_EALIGN);

    /* the transposed fold */
    EXPECT_RC(ldm_decoder_fold_bwd(NULL, dbeta, B, dz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, NULL, B, dz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, dbeta, B, NULL, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, dbeta, 0, dz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, dbeta, 1 << 24, dz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, (float*)off(dbeta, 2), B, dz, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_decoder_fold_bwd(&d, dbeta, B, (float*)off(dz, 1), NULL), LDM_EALIGN);
    {
        ldm_decoder_grad_t e = d;
        e.wz = NULL;
        EXPECT_RC(ldm_decoder_fold_bwd(&e, dbeta, B, dz, NULL), LDM_EINVAL);
        e = d;
        e.abi_version = 0;
        EXPECT_RC(ldm_decoder_fold_bwd(&e, dbeta, B, dz, NULL), LDM_EINVAL);
        e = d;
        e.dtype = LDM_F32;
        EXPECT_RC(ldm_decoder_fold_bwd(&e, dbeta, B, dz, NULL), LDM_ENOSYS);
    }

    return check_report("grad_errors");
}
