/* Host-side checks of the earth mover's distance entry points of libldm_sdf's C ABI
 * (include/ldm_sdf.h: ldm_emd_matrix, its workspace size and the four host functions): invalid
 * arguments must return LDM_EINVAL / LDM_ENOSYS / LDM_EALIGN / LDM_ENOSPC and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_emd_host.py against the product
 * library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <math.h>
#include <string.h>

#include "check.h"

int main(void) {
    float* a = (float*)fake();
    float* b = (float*)fake();
    float* out = (float*)fake();
    int32_t* asg = (int32_t*)fake();
    int32_t* rnd = (int32_t*)fake();
    int32_t* unc = (int32_t*)fake();
    void* ws = fake();
    const int64_t big = (int64_t)1 << 31;
    const int64_t nmax = ldm_emd_max_points();
    const float eps = 1e-4f, ext = 3.5f;

    /* the host functions */
    EXPECT(nmax >= 2048);
    EXPECT(ldm_emd_slack(0.0) == 0.0 && ldm_emd_slack(-1.0) == 0.0);
    EXPECT(ldm_emd_slack(2.0) == 2.0 * ldm_emd_slack(1.0) && ldm_emd_slack(1.0) > 0.0);
    EXPECT(ldm_emd_slack(1.0) < 64.0 * 5.9604644775390625e-8);          /* a few u per extent */
    EXPECT(ldm_emd_min_eps(3.0) == 8.0 * ldm_emd_slack(3.0));
    EXPECT(ldm_emd_min_eps(3.4641016151377544) < 1e-4); /* the default eps on [-1, 1]^3 */
    EXPECT(ldm_emd_default_max_rounds(0) == 0 && ldm_emd_default_max_rounds(-5) == 0);
    EXPECT(ldm_emd_default_max_rounds(nmax + 1) == 0);
    EXPECT(ldm_emd_default_max_rounds(1) >= 1);
    EXPECT(ldm_emd_default_max_rounds(nmax) > ldm_emd_default_max_rounds(1));
    EXPECT(ldm_emd_default_max_rounds(nmax) <= 0x7fffffff);
    EXPECT(ldm_emd_ws_bytes(-1, 1, 1) == 0);
    EXPECT(ldm_emd_ws_bytes(1, -1, 1) == 0);
    EXPECT(ldm_emd_ws_bytes(1, 1, -1) == 0);
    EXPECT(ldm_emd_ws_bytes(big, 1, 1) == 0);
    EXPECT(ldm_emd_ws_bytes(0, 0, 0) > 0);
    EXPECT(ldm_emd_ws_bytes(1000, 1000, nmax) < 4096);                   /* never S x R x n */

    const int64_t S = 3, R = 5, n = 100;
    const size_t need = ldm_emd_ws_bytes(S, R, n);
    /* S == 0 or R == 0: success before any pointer is looked at */
    EXPECT(ldm_emd_matrix(NULL, 0, NULL, 0, 0, 0.f, 0.f, 0, 0, NULL, NULL, NULL, NULL, NULL, 0,
                          NULL) == 0);
    EXPECT(ldm_emd_matrix(a, 0, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, 0, NULL) == 0);
    EXPECT(ldm_emd_matrix(a, S, b, 0, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, 0, NULL) == 0);
    /* negative counts, empty clouds with work to do */
    EXPECT_RC(ldm_emd_matrix(a, -1, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, -1, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, -1, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, 0, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    /* more points than a workgroup keeps in LDS */
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, nmax + 1, eps, ext, 0, 0, out, asg, rnd, unc, ws, need,
                             NULL), LDM_ENOSYS);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, big, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_ENOSYS);
    /* NULL required pointers (assign, rounds and unconverged may be NULL) */
    EXPECT_RC(ldm_emd_matrix(NULL, S, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, NULL, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, NULL, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, NULL, need, NULL),
              LDM_EINVAL);
    /* alignment */
    EXPECT_RC(ldm_emd_matrix((float*)off(a, 2), S, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws,
                             need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, (float*)off(b, 1), R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws,
                             need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, (float*)off(out, 3), asg, rnd, unc, ws,
                             need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, (int32_t*)off(asg, 2), rnd, unc,
                             ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, asg, (int32_t*)off(rnd, 1), unc,
                             ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, asg, rnd, (int32_t*)off(unc, 2),
                             ws, need, NULL), LDM_EALIGN);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, off(ws, 128), need,
                             NULL), LDM_EALIGN);
    /* beyond the launch limits */
    EXPECT_RC(ldm_emd_matrix(a, big, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, (size_t)-1,
                             NULL), LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, big, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, (size_t)-1,
                             NULL), LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, 65536, b, 32768, n, eps, ext, 0, 0, out, asg, rnd, unc, ws,
                             (size_t)-1, NULL), LDM_EINVAL);
    /* within-set: one set, a square matrix */
    EXPECT_RC(ldm_emd_matrix(a, S, b, S, n, eps, ext, 0, 1, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, a, R, n, eps, ext, 0, 1, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    /* the extent bound */
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, -1.f, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, INFINITY, 0, 0, out, asg, rnd, unc, ws, need,
                             NULL), LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, NAN, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    /* eps: positive, finite, at or above the floor for the extent */
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, 0.f, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, 0.f, 0.f, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, -eps, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, NAN, ext, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, INFINITY, ext, 0, 0, out, asg, rnd, unc, ws, need,
                             NULL), LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, (float)(0.5 * ldm_emd_min_eps(ext)), ext, 0, 0, out,
                             asg, rnd, unc, ws, need, NULL), LDM_EINVAL);
    EXPECT(strstr(ldm_last_error(), "ldm_emd_min_eps") != NULL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, 100.f, 0, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    /* max_rounds */
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, -1, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, big, 0, out, asg, rnd, unc, ws, need, NULL),
              LDM_EINVAL);
    /* workspace too small (checked last: everything else is in order here) */
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 0, 0, out, asg, rnd, unc, ws, need - 1,
                             NULL), LDM_ENOSPC);
    EXPECT_RC(ldm_emd_matrix(a, S, b, R, n, eps, ext, 7, 0, out, NULL, NULL, NULL, ws, 0, NULL),
              LDM_ENOSPC);
    EXPECT_RC(ldm_emd_matrix(a, S, a, S, n, eps, ext, 0, 1, out, asg, rnd, unc, ws, 0, NULL),
              LDM_ENOSPC);

    return check_report("emd_errors");
}
