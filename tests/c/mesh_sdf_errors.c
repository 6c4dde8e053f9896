/* Host-side checks of the mesh -> signed distance entry points of libldm_sdf's C ABI
 * (include/ldm_sdf.h: ldm_mesh_sdf_ws_bytes, ldm_mesh_sdf, ldm_mesh_sdf_face_chunk,
 * ldm_mesh_sdf_split_below): invalid arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC
 * and leave a message in ldm_last_error() -- never crash, read or write out of bounds.  No GPU
 * is needed: the argument checks run before any device work.  Built by
 * tests/test_mesh_sdf_host.py against the product library and by csrc/Makefile `check-asan`
 * under host AddressSanitizer. */
#include <string.h>

#include "check.h"

int main(void) {
    float* v = (float*)fake();
    int32_t* f = (int32_t*)fake();
    float* p = (float*)fake();
    float* sdf = (float*)fake();
    int32_t* cl = (int32_t*)fake();
    float* wn = (float*)fake();
    int32_t* flag = (int32_t*)fake();
    void* ws = fake();
    const int chunk = ldm_mesh_sdf_face_chunk();
    const int64_t split = ldm_mesh_sdf_split_below();
    EXPECT(chunk > 0 && split > 0);

    /* workspace size: 0 for negative sizes, positive otherwise, monotone in F, and the split
     * form's partials bounded by a tile of points (never chunks x P) */
    EXPECT(ldm_mesh_sdf_ws_bytes(-1, 10) == 0);
    EXPECT(ldm_mesh_sdf_ws_bytes(10, -1) == 0);
    EXPECT(ldm_mesh_sdf_ws_bytes(0, 0) > 0);
    EXPECT(ldm_mesh_sdf_ws_bytes(0, 1000) > 0);
    EXPECT(ldm_mesh_sdf_ws_bytes(100000, 500000) >= ldm_mesh_sdf_ws_bytes(1000, 500000));
    EXPECT(ldm_mesh_sdf_ws_bytes(100000, 500000) >= (size_t)100000 * 36);
    EXPECT(ldm_mesh_sdf_ws_bytes(100000, 500000) < (size_t)100000 * 256);
    EXPECT(ldm_mesh_sdf_ws_bytes(100000, split - 1) >= ldm_mesh_sdf_ws_bytes(100000, 1));
    EXPECT(ldm_mesh_sdf_ws_bytes(100000, split - 1) - ldm_mesh_sdf_ws_bytes(100000, split) <
           (size_t)(100000 / chunk) * (size_t)(split - 1) * 16 / 2);
    EXPECT(ldm_mesh_sdf_ws_bytes(chunk, 1) == ldm_mesh_sdf_ws_bytes(chunk, split));

    const int V = 8, F = 12;
    const int64_t P = 100;
    const size_t need = ldm_mesh_sdf_ws_bytes(F, P);
    /* P == 0: success before any pointer is looked at */
    EXPECT(ldm_mesh_sdf(NULL, 0, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, 0, NULL) == 0);
    EXPECT(ldm_mesh_sdf(v, V, f, F, p, 0, sdf, cl, wn, flag, ws, 0, NULL) == 0);
    /* negative sizes */
    EXPECT_RC(ldm_mesh_sdf(v, -1, f, F, p, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, -1, p, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, -1, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    /* NULL required pointers (closest and winding may be NULL) */
    EXPECT_RC(ldm_mesh_sdf(NULL, V, f, F, p, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, NULL, F, p, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, NULL, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, NULL, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, wn, NULL, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, wn, flag, NULL, need, NULL), LDM_EINVAL);
    /* faces without vertices */
    EXPECT_RC(ldm_mesh_sdf(v, 0, f, F, p, P, sdf, cl, wn, flag, ws, need, NULL), LDM_EINVAL);
    /* alignment */
    EXPECT_RC(ldm_mesh_sdf((float*)off(v, 2), V, f, F, p, P, sdf, cl, wn, flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, (int32_t*)off(f, 1), F, p, P, sdf, cl, wn, flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, (float*)off(p, 2), P, sdf, cl, wn, flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, (float*)off(sdf, 1), cl, wn, flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, (int32_t*)off(cl, 2), wn, flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, (float*)off(wn, 3), flag, ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, wn, (int32_t*)off(flag, 2), ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, wn, flag, off(ws, 16), need, NULL),
              LDM_EALIGN);
    /* workspace too small, in both launch forms */
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, cl, wn, flag, ws, need - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, P, sdf, NULL, NULL, flag, ws, 0, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_mesh_sdf(v, 30000, f, 4 * chunk + 1, p, P, sdf, cl, wn, flag, ws,
                           ldm_mesh_sdf_ws_bytes(4 * chunk + 1, P) - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_mesh_sdf(v, 30000, f, 4 * chunk + 1, p, P, sdf, cl, wn, flag, ws,
                           ldm_mesh_sdf_ws_bytes(4 * chunk + 1, split), NULL), LDM_ENOSPC);
    /* a grid beyond the launch limits, in both forms: refused with the arguments, not left to
     * fail as a launch after the pack kernel is queued */
    EXPECT_RC(ldm_mesh_sdf(v, V, f, F, p, ((int64_t)1 << 31) * 256, sdf, cl, wn, flag, ws,
                           (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_mesh_sdf(v, 30000, f, 65535 * chunk + 1, p, P, sdf, cl, wn, flag, ws,
                           (size_t)-1, NULL), LDM_EINVAL);

    return check_report("mesh_sdf_errors");
}
