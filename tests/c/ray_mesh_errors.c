/* Host-side checks of the ray casting entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_ray_mesh_ws_bytes, ldm_ray_mesh, ldm_ray_mesh_face_chunk, ldm_ray_mesh_split_below):
 * invalid arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_render_host.py against the product
 * library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <math.h>
#include <string.h>

#include "check.h"

int main(void) {
    float* v = (float*)fake();
    int32_t* f = (int32_t*)fake();
    float* o = (float*)fake();
    float* d = (float*)fake();
    float* t = (float*)fake();
    int32_t* fo = (int32_t*)fake();
    float* bo = (float*)fake();
    int32_t* flag = (int32_t*)fake();
    void* ws = fake();
    const int chunk = ldm_ray_mesh_face_chunk();
    const int64_t split = ldm_ray_mesh_split_below();
    const float inf = INFINITY, qnan = NAN;
    EXPECT(chunk > 0 && split > 0);

    /* workspace size: 0 for negative sizes, positive otherwise, monotone in F, and the split
     * form's partials bounded by a tile of rays (never chunks x R) */
    EXPECT(ldm_ray_mesh_ws_bytes(-1, 10) == 0);
    EXPECT(ldm_ray_mesh_ws_bytes(10, -1) == 0);
    EXPECT(ldm_ray_mesh_ws_bytes(0, 0) > 0);
    EXPECT(ldm_ray_mesh_ws_bytes(0, 1000) > 0);
    EXPECT(ldm_ray_mesh_ws_bytes(100000, split) >= ldm_ray_mesh_ws_bytes(1000, split));
    EXPECT(ldm_ray_mesh_ws_bytes(100000, split) >= (size_t)100000 * 36);
    EXPECT(ldm_ray_mesh_ws_bytes(100000, split) < (size_t)100000 * 256);
    EXPECT(ldm_ray_mesh_ws_bytes(100000, split - 1) >= ldm_ray_mesh_ws_bytes(100000, 1));
    EXPECT(ldm_ray_mesh_ws_bytes(100000, split - 1) - ldm_ray_mesh_ws_bytes(100000, split) <
           (size_t)(100000 / chunk) * (size_t)(split - 1) * 16 / 2);
    EXPECT(ldm_ray_mesh_ws_bytes(chunk, 1) == ldm_ray_mesh_ws_bytes(chunk, split));

    const int V = 8, F = 12;
    const int64_t R = 100;
    const size_t need = ldm_ray_mesh_ws_bytes(F, R);
    /* R == 0: success before any pointer is looked at */
    EXPECT(ldm_ray_mesh(NULL, 0, NULL, 0, NULL, NULL, 0, 0.0f, inf, NULL, NULL, NULL, NULL, NULL,
                        0, NULL) == 0);
    EXPECT(ldm_ray_mesh(v, V, f, F, o, d, 0, 0.0f, inf, t, fo, bo, flag, ws, 0, NULL) == 0);
    /* negative sizes */
    EXPECT_RC(ldm_ray_mesh(v, -1, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, -1, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, -1, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    /* the bounds: t_min > t_max, a NaN on either side (also with no rays); equal bounds pass
     * the check and stop at the next one */
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 1.0f, 0.5f, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, qnan, 1.0f, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, qnan, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, 0, 2.0f, 1.0f, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 1.0f, 1.0f, t, fo, bo, flag, NULL, need, NULL),
              LDM_EINVAL);
    /* NULL required pointers (face_out and bary_out may be NULL) */
    EXPECT_RC(ldm_ray_mesh(NULL, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, NULL, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, NULL, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, NULL, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, NULL, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, NULL, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, NULL, need, NULL),
              LDM_EINVAL);
    /* faces without vertices */
    EXPECT_RC(ldm_ray_mesh(v, 0, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need, NULL),
              LDM_EINVAL);
    /* alignment */
    EXPECT_RC(ldm_ray_mesh((float*)off(v, 2), V, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, (int32_t*)off(f, 1), F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, (float*)off(o, 2), d, R, 0.0f, inf, t, fo, bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, (float*)off(d, 3), R, 0.0f, inf, t, fo, bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, (float*)off(t, 1), fo, bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, (int32_t*)off(fo, 2), bo, flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, (float*)off(bo, 3), flag, ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, (int32_t*)off(flag, 2), ws,
                           need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, off(ws, 16), need,
                           NULL), LDM_EALIGN);
    /* workspace too small, in both launch forms */
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, fo, bo, flag, ws, need - 1, NULL),
              LDM_ENOSPC);
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, R, 0.0f, inf, t, NULL, NULL, flag, ws, 0, NULL),
              LDM_ENOSPC);
    EXPECT_RC(ldm_ray_mesh(v, 30000, f, 4 * chunk + 1, o, d, R, 0.0f, inf, t, fo, bo, flag, ws,
                           ldm_ray_mesh_ws_bytes(4 * chunk + 1, R) - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_ray_mesh(v, 30000, f, 4 * chunk + 1, o, d, R, 0.0f, inf, t, fo, bo, flag, ws,
                           ldm_ray_mesh_ws_bytes(4 * chunk + 1, split), NULL), LDM_ENOSPC);
    /* a grid beyond the launch limits, in both forms: refused with the arguments, not left to
     * fail as a launch after the pack kernel is queued */
    EXPECT_RC(ldm_ray_mesh(v, V, f, F, o, d, ((int64_t)1 << 31) * 256, 0.0f, inf, t, fo, bo, flag,
                           ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_ray_mesh(v, 30000, f, 65535 * chunk + 1, o, d, R, 0.0f, inf, t, fo, bo, flag,
                           ws, (size_t)-1, NULL), LDM_EINVAL);

    return check_report("ray_mesh_errors");
}
