/* Host-side checks of the conv1d backward entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_conv1d_bwd_data, ldm_conv1d_bwd_weight, ldm_conv1d_bwd_weight_ws_floats): invalid
 * arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC / LDM_ENOSYS and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_unet_train_host.py against the product
 * library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <string.h>

#include "check.h"

/* a k = 3, stride 1, pad 1 segment of 40 channels (packed row of 48) over 130 positions */
static ldm_conv1d_seg_t good_seg(void) {
    ldm_conv1d_seg_t g;
    memset(&g, 0, sizeof(g));
    g.X = (const float*)fake();
    g.W = fake();
    g.C = 40;
    g.L_in = 130;
    g.ksize = 3;
    g.stride = 1;
    g.pad = 1;
    g.mode = LDM_CONV_DIRECT;
    g.silu_in = 1;
    g.kstride = 48;
    g.ldw = 3 * 48;
    return g;
}

static ldm_conv1d_bwd_data_args_t good_data(void) {
    ldm_conv1d_bwd_data_args_t a;
    memset(&a, 0, sizeof(a));
    a.B = 2;
    a.Cout = 20;
    a.L_out = 130;
    a.w_dtype = LDM_F32;
    a.seg = good_seg();
    a.dY = (const float*)fake();
    a.dX = (float*)fake();
    return a;
}

static ldm_conv1d_bwd_weight_args_t good_weight(void) {
    ldm_conv1d_bwd_weight_args_t a;
    memset(&a, 0, sizeof(a));
    a.B = 2;
    a.Cout = 20;
    a.L_out = 130;
    a.n_seg = 2;
    a.seg[0] = good_seg();
    a.seg[1] = good_seg();
    a.seg[1].C = 16;
    a.seg[1].ksize = 1;
    a.seg[1].pad = 0;
    a.seg[1].silu_in = 0;
    a.seg[1].kstride = 16;
    a.seg[1].ldw = 16;
    a.dW[0] = (float*)fake();
    a.dW[1] = (float*)fake();
    a.dY = (const float*)fake();
    a.dbias = (float*)fake();
    a.ws = (float*)fake();
    a.ws_floats = ldm_conv1d_bwd_weight_ws_floats(&a);
    return a;
}

int main(void) {
    /* ---- ldm_conv1d_bwd_data ---- */
    ldm_conv1d_bwd_data_args_t d = good_data();
    EXPECT_RC(ldm_conv1d_bwd_data(NULL, NULL), LDM_EINVAL);
    d = good_data(); d.dY = NULL;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.dX = NULL;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.W = NULL;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.X = NULL;               /* SiLU' reads X */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.B = 0;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.B = 65536;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.Cout = 0;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.w_dtype = LDM_F16;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    EXPECT(strstr(ldm_last_error(), "w_dtype") != NULL);
    d = good_data(); d.L_out = 129;                /* L_in 130, k 3, pad 1 gives 130 */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    EXPECT(strstr(ldm_last_error(), "L_out") != NULL);
    d = good_data(); d.seg.mode = 7;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.mode = LDM_CONV_UP2; d.seg.stride = 2; d.L_out = 130;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.pad = 3;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.kstride = 40;           /* < round16(C), and not a multiple of 16 */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.ldw = 2 * 48;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EINVAL);
    d = good_data(); d.seg.ksize = 5; d.seg.pad = 2;   /* no kernel for this geometry */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_ENOSYS);
    d = good_data(); d.seg.ksize = 1; d.seg.stride = 2; d.seg.pad = 0; d.L_out = 65;
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_ENOSYS);
    d = good_data(); d.seg.W = off(d.seg.W, 8 * 4);    /* a c_off of 8 channels */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EALIGN);
    d = good_data(); d.w_dtype = LDM_BF16; d.seg.W = off(d.seg.W, 8 * 2);
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EALIGN);
    d = good_data(); d.dX = (float*)off(d.dX, 2);
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_EALIGN);
    d = good_data(); d.Cout = 4000;                /* the staged operands exceed the LDS */
    EXPECT_RC(ldm_conv1d_bwd_data(&d, NULL), LDM_ENOSPC);
    EXPECT(strstr(ldm_last_error(), "LDS") != NULL);

    /* ---- ldm_conv1d_bwd_weight_ws_floats ---- */
    ldm_conv1d_bwd_weight_args_t w = good_weight();
    /* units = B ceil(130 / 64) = 6 slices; a partial = 32 rows x (3 x 48 + 1 x 16) columns;
     * dbias without dcbias takes B x Cout floats more */
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 6 * 32 * (3 * 48 + 16) + 2 * 20);
    w.dcbias = (float*)fake();
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 6 * 32 * (3 * 48 + 16));
    w = good_weight(); w.B = 40; w.L_out = 256;    /* 160 units: capped at 64 slices */
    w.seg[0].L_in = w.seg[1].L_in = 256; w.dbias = NULL;
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 64 * 32 * (3 * 48 + 16));
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(NULL) == 0);
    w = good_weight(); w.n_seg = 0;
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 0);
    w = good_weight(); w.n_seg = LDM_CONV_MAX_SEGS + 1;
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 0);
    w = good_weight(); w.B = 0;
    EXPECT(ldm_conv1d_bwd_weight_ws_floats(&w) == 0);

    /* ---- ldm_conv1d_bwd_weight ---- */
    EXPECT_RC(ldm_conv1d_bwd_weight(NULL, NULL), LDM_EINVAL);
    w = good_weight(); w.dY = NULL;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.seg[1].X = NULL;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.dW[0] = NULL;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.n_seg = 0;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    EXPECT(strstr(ldm_last_error(), "n_seg") != NULL);
    w = good_weight(); w.n_seg = LDM_CONV_MAX_SEGS + 1;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.B = 65536;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.seg[1].L_in = 131;        /* the segments disagree on L_out */
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    EXPECT(strstr(ldm_last_error(), "L_out") != NULL);
    w = good_weight(); w.seg[0].ksize = 5; w.seg[0].pad = 2;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_ENOSYS);
    w = good_weight(); w.seg[0].kstride = 24;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EINVAL);
    w = good_weight(); w.dW[1] = (float*)off(w.dW[1], 8 * 4);   /* a c_off of 8 channels */
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EALIGN);
    w = good_weight(); w.dbias = (float*)off(w.dbias, 1);
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_EALIGN);
    w = good_weight(); w.ws_floats -= 1;           /* a short workspace */
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_ENOSPC);
    EXPECT(strstr(ldm_last_error(), "workspace") != NULL);
    w = good_weight(); w.ws = NULL;
    EXPECT_RC(ldm_conv1d_bwd_weight(&w, NULL), LDM_ENOSPC);

    return check_report("unet_bwd_errors");
}
