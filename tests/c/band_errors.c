/* Host-side checks of the narrow-band entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_band_workspace_bytes, ldm_band_lattice_coords, ldm_band_classify, ldm_decoder_bricks_fwd,
 * ldm_band_fill): invalid arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC and leave a
 * message in ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed:
 * the argument checks run before any device work.  Built by tests/test_band_host.py against the
 * product library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <math.h>
#include <string.h>

#include "check.h"

int main(void) {
    float* f = (float*)fake();
    float* out = (float*)fake();
    uint8_t* act = (uint8_t*)fake();
    int32_t* list = (int32_t*)fake();
    int32_t* cnt = (int32_t*)fake();
    void* ws = fake();
    const int big = 1 << 20;

    /* workspace size: positive, monotone, 0 for invalid sizes */
    EXPECT(ldm_band_workspace_bytes(1, 2) > 0);
    EXPECT(ldm_band_workspace_bytes(1, 512) >= ldm_band_workspace_bytes(1, 256));
    EXPECT(ldm_band_workspace_bytes(64, 512) >= ldm_band_workspace_bytes(1, 512));
    EXPECT(ldm_band_workspace_bytes(64, 512) > ldm_band_workspace_bytes(1, 8));
    EXPECT(ldm_band_workspace_bytes(0, 64) == 0);
    EXPECT(ldm_band_workspace_bytes(1, 1) == 0);
    EXPECT(ldm_band_workspace_bytes(big, 512) == 0);

    EXPECT_RC(ldm_band_lattice_coords(1, 0.1f, -1.f, f, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_lattice_coords(16, 0.1f, -1.f, NULL, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_lattice_coords(16, 0.1f, -1.f, (float*)off(f, 2), NULL), LDM_EALIGN);

    const size_t need = ldm_band_workspace_bytes(2, 44);
    EXPECT_RC(ldm_band_classify(NULL, 2, 44, 0.f, 0.05f, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, NULL, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, act, NULL, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, act, list, NULL, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, act, list, cnt, NULL, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 1, 0.f, 0.05f, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 0, 44, 0.f, 0.05f, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, big, 512, 0.f, 0.05f, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, -1.f, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, NAN, act, list, cnt, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, (uint8_t*)off(act, 8), list, cnt, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, act, list, cnt, off(ws, 16), need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, 0.05f, act, list, cnt, ws, need - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_band_classify(f, 2, 44, 0.f, INFINITY, act, list, cnt, ws, 0, NULL), LDM_ENOSPC);

    EXPECT_RC(ldm_band_fill(NULL, act, 2, 44, out, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, NULL, 2, 44, out, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, act, 2, 44, NULL, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, act, 2, 1, out, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, act, 0, 44, out, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, act, big, 512, out, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_band_fill(f, act, 2, 44, (float*)off(out, 4), NULL), LDM_EALIGN);

    ldm_decoder_t dec;
    memset(&dec, 0, sizeof(dec));
    dec.abi_version = LDM_ABI_VERSION;
    dec.dtype = LDM_BF16;
    dec.hidden = 512;
    dec.skip_width = 253;
    dec.latent_dim = 256;
    dec.n_stages = 384;
    dec.layout = LDM_LAYOUT_SPLIT;
    dec.weights = fake();
    dec.wz = (const float*)fake();
    dec.bz = (const float*)fake();
    dec.wxyz = (const float*)fake();
    dec.w_last = (const float*)fake();
    const size_t dws = ldm_workspace_bytes_layout(LDM_OP_DECODER_GRID, 2, 44, LDM_BF16,
                                                  LDM_LAYOUT_SPLIT);
    EXPECT(dws > 0);
    EXPECT_RC(ldm_decoder_bricks_fwd(NULL, f, 2, 44, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, NULL, 2, 44, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, NULL, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, list, NULL, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, list, cnt, NULL, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 1, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 0, 44, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, big, 512, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, (int32_t*)off(list, 1), cnt, out,
                                     ws, dws, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, (float*)off(f, 4), 2, 44, 0.05f, -1.f, list, cnt, out,
                                     ws, dws, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, list, cnt, out, ws, dws - 1, NULL),
              LDM_ENOSPC);
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, list, cnt, out, NULL, 0, NULL),
              LDM_ENOSPC);
    dec.abi_version = LDM_ABI_VERSION - 1;     /* stale descriptor */
    EXPECT_RC(ldm_decoder_bricks_fwd(&dec, f, 2, 44, 0.05f, -1.f, list, cnt, out, ws, dws, NULL),
              LDM_EINVAL);

    return check_report("band_errors");
}
