/* Host-side checks of the nearest-point / Chamfer entry points of libldm_sdf's C ABI
 * (include/ldm_sdf.h: ldm_nearest_points, ldm_chamfer_matrix, their workspace sizes and the four
 * constants): invalid arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC and leave a
 * message in ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed:
 * the argument checks run before any device work.  Built by tests/test_metrics_host.py against
 * the product library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <string.h>

#include "check.h"

int main(void) {
    float* q = (float*)fake();
    float* c = (float*)fake();
    float* d2 = (float*)fake();
    int32_t* idx = (int32_t*)fake();
    float* out = (float*)fake();
    void* ws = fake();
    const int ta = ldm_chamfer_tile_a(), cb = ldm_chamfer_chunk_b();
    const int64_t split = ldm_chamfer_split_below(), spread = ldm_chamfer_spread_below();
    const int64_t big = (int64_t)1 << 31;
    EXPECT(ta >= 1 && cb >= 1 && split >= 1 && spread >= 1);

    /* workspace sizes: 0 for what the call refuses, positive otherwise, bounded by the tiling */
    EXPECT(ldm_nearest_points_ws_bytes(-1, 10) == 0);
    EXPECT(ldm_nearest_points_ws_bytes(10, -1) == 0);
    EXPECT(ldm_nearest_points_ws_bytes(0, 0) > 0);
    EXPECT(ldm_nearest_points_ws_bytes(1, 1) > 0);
    EXPECT(ldm_nearest_points_ws_bytes(1, cb) == ldm_nearest_points_ws_bytes(split, cb));
    EXPECT(ldm_nearest_points_ws_bytes(split - 1, 100 * (int64_t)cb) >
           ldm_nearest_points_ws_bytes(split, 100 * (int64_t)cb));
    EXPECT(ldm_nearest_points_ws_bytes(split - 1, (int64_t)1 << 30) < ((size_t)1 << 26));
    EXPECT(ldm_chamfer_ws_bytes(-1, 1, 1, 1) == 0);
    EXPECT(ldm_chamfer_ws_bytes(1, -1, 1, 1) == 0);
    EXPECT(ldm_chamfer_ws_bytes(1, 1, -1, 1) == 0);
    EXPECT(ldm_chamfer_ws_bytes(1, 1, 1, -1) == 0);
    EXPECT(ldm_chamfer_ws_bytes(big, 1, 1, 1) == 0);
    EXPECT(ldm_chamfer_ws_bytes(0, 0, 0, 0) > 0);
    EXPECT(ldm_chamfer_ws_bytes(1000, 2048, 1000, 2048) < 4096);       /* never S x R x n */
    EXPECT(ldm_chamfer_ws_bytes(1, 30000, 1, 30000) >= (size_t)30000 * 4);
    EXPECT(ldm_chamfer_ws_bytes(1, (int64_t)1 << 30, 1, (int64_t)1 << 30) < ((size_t)1 << 26));
    EXPECT(ldm_chamfer_ws_bytes(3, (int64_t)1 << 20, 5, 30000) ==
           ldm_chamfer_ws_bytes(1, (int64_t)1 << 20, 1, 30000));

    /* ---- ldm_nearest_points ---- */
    const int64_t P = 100, Q = 3 * (int64_t)cb + 2;
    const size_t need = ldm_nearest_points_ws_bytes(P, Q);
    /* P == 0: success before any pointer is looked at */
    EXPECT(ldm_nearest_points(NULL, 0, NULL, 0, NULL, NULL, NULL, 0, NULL) == 0);
    EXPECT(ldm_nearest_points(q, 0, c, Q, d2, idx, ws, 0, NULL) == 0);
    /* negative counts, an empty cloud with work to do */
    EXPECT_RC(ldm_nearest_points(q, -1, c, Q, d2, idx, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, P, c, -1, d2, idx, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, P, c, 0, d2, idx, ws, need, NULL), LDM_EINVAL);
    /* NULL required pointers (idx may be NULL) */
    EXPECT_RC(ldm_nearest_points(NULL, P, c, Q, d2, idx, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, P, NULL, Q, d2, idx, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, NULL, idx, ws, need, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, idx, NULL, need, NULL), LDM_EINVAL);
    /* alignment */
    EXPECT_RC(ldm_nearest_points((float*)off(q, 2), P, c, Q, d2, idx, ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_nearest_points(q, P, (float*)off(c, 1), Q, d2, idx, ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, (float*)off(d2, 3), idx, ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, (int32_t*)off(idx, 2), ws, need, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, idx, off(ws, 16), need, NULL), LDM_EALIGN);
    /* workspace too small, in both launch forms */
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, idx, ws, need - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, NULL, ws, 0, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_nearest_points(q, P, c, Q, d2, idx, ws, ldm_nearest_points_ws_bytes(split, Q),
                                 NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_nearest_points(q, split, c, Q, d2, idx, ws,
                                 ldm_nearest_points_ws_bytes(split, Q) - 1, NULL), LDM_ENOSPC);
    /* beyond the launch limits: an index past int32, more workgroups than a grid has */
    EXPECT_RC(ldm_nearest_points(q, P, c, big, d2, idx, ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_nearest_points(q, (big - 1) * ta + 1, c, Q, d2, idx, ws, (size_t)-1, NULL),
              LDM_EINVAL);

    /* ---- ldm_chamfer_matrix ---- */
    const int64_t S = 3, n = ta + 1, R = 5, m = Q;
    const size_t mneed = ldm_chamfer_ws_bytes(S, n, R, m);
    /* S == 0 or R == 0: success before any pointer is looked at */
    EXPECT(ldm_chamfer_matrix(NULL, 0, 0, NULL, 0, 0, NULL, NULL, 0, NULL) == 0);
    EXPECT(ldm_chamfer_matrix(q, 0, n, c, R, m, out, ws, 0, NULL) == 0);
    EXPECT(ldm_chamfer_matrix(q, S, n, c, 0, m, out, ws, 0, NULL) == 0);
    EXPECT(ldm_chamfer_matrix(q, 0, 0, c, R, 0, out, ws, 0, NULL) == 0);
    /* negative counts, empty clouds with work to do */
    EXPECT_RC(ldm_chamfer_matrix(q, -1, n, c, R, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, -1, c, R, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, -1, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, -1, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, 0, c, R, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, 0, out, ws, mneed, NULL), LDM_EINVAL);
    /* NULL pointers */
    EXPECT_RC(ldm_chamfer_matrix(NULL, S, n, c, R, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, NULL, R, m, out, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, NULL, ws, mneed, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, out, NULL, mneed, NULL), LDM_EINVAL);
    /* alignment */
    EXPECT_RC(ldm_chamfer_matrix((float*)off(q, 2), S, n, c, R, m, out, ws, mneed, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, (float*)off(c, 1), R, m, out, ws, mneed, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, (float*)off(out, 3), ws, mneed, NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, out, off(ws, 128), mneed, NULL), LDM_EALIGN);
    /* workspace too small: the spread form, then the batch form */
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, out, ws, mneed - 1, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, m, out, ws, 0, NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_chamfer_matrix(q, spread, n, c, 1, m, out, ws,
                                 ldm_chamfer_ws_bytes(spread, n, 1, m) - 1, NULL), LDM_ENOSPC);
    EXPECT(ldm_chamfer_ws_bytes(spread, n, 1, m) < mneed);
    /* beyond the launch limits */
    EXPECT_RC(ldm_chamfer_matrix(q, S, big, c, R, m, out, ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, R, big, out, ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, big, n, c, R, m, out, ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, S, n, c, big, m, out, ws, (size_t)-1, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_chamfer_matrix(q, 65536, n, c, 32768, m, out, ws, (size_t)-1, NULL),
              LDM_EINVAL);

    return check_report("chamfer_errors");
}
