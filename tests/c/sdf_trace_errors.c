/* Host-side checks of the sphere tracing entry points of libldm_sdf's C ABI (include/ldm_sdf.h:
 * ldm_sdf_trace_ws_bytes, ldm_sdf_trace_init, ldm_sdf_trace_emit, ldm_sdf_trace_step): invalid
 * arguments must return LDM_EINVAL / LDM_EALIGN / LDM_ENOSPC and leave a message in
 * ldm_last_error() -- never crash, read or write out of bounds.  No GPU is needed: the argument
 * checks run before any device work.  Built by tests/test_sdf_trace_reference.py against the
 * product library and by csrc/Makefile `check-asan` under host AddressSanitizer. */
#include <math.h>
#include <string.h>

#include "check.h"

int main(void) {
    float* o = (float*)fake();
    float* d = (float*)fake();
    float* t = (float*)fake();
    int32_t* st = (int32_t*)fake();
    int32_t* sp = (int32_t*)fake();
    float* xl = (float*)fake();
    int32_t* li = (int32_t*)fake();
    int32_t* cn = (int32_t*)fake();
    float* xyz = (float*)fake();
    float* va = (float*)fake();
    uint8_t* mk = (uint8_t*)fake();
    void* ws = fake();
    const float inf = INFINITY, qnan = NAN;
    const int B = 3, P = 50, N = 64, MS = 256;
    const int64_t R = 100;
    const float vs = 2.0f / 63.0f;

    /* workspace size: 0 for what the calls refuse, else positive and monotone */
    EXPECT(ldm_sdf_trace_ws_bytes(0, 10) == 0);
    EXPECT(ldm_sdf_trace_ws_bytes(1, 0) == 0);
    EXPECT(ldm_sdf_trace_ws_bytes(-1, 10) == 0);
    EXPECT(ldm_sdf_trace_ws_bytes(2, (int64_t)1 << 30) == 0);
    EXPECT(ldm_sdf_trace_ws_bytes(1, 1) > 0);
    EXPECT(ldm_sdf_trace_ws_bytes(3, 70000) >= (size_t)3 * 70000 * 5);
    EXPECT(ldm_sdf_trace_ws_bytes(3, 70000) > ldm_sdf_trace_ws_bytes(3, 100));
    const size_t need = ldm_sdf_trace_ws_bytes(B, R);

#define INIT(o_, d_, B_, R_, lo_, hi_, t0_, t1_, lv_, L_, e_, ms_, mk_, N_, vs_, t_, st_, sp_, \
             xl_, li_, cn_, ws_, wb_)                                                          \
    ldm_sdf_trace_init(o_, d_, 0, B_, R_, lo_, hi_, t0_, t1_, lv_, L_, e_, ms_, mk_, N_, vs_,  \
                       t_, st_, sp_, xl_, li_, cn_, ws_, wb_, NULL)
    /* sizes */
    EXPECT_RC(INIT(o, d, 0, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, 0, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, -5, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    /* R * B must stay below 2^31 */
    EXPECT_RC(INIT(o, d, 2, (int64_t)1 << 30, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0,
                   0.f, t, st, sp, xl, li, cn, ws, (size_t)-1), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, 1, (int64_t)1 << 31, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0,
                   0.f, t, st, sp, xl, li, cn, ws, (size_t)-1), LDM_EINVAL);
    /* NULL required pointers (xyz_last and mask may be NULL) */
    EXPECT_RC(INIT(NULL, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st,
                   sp, xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, NULL, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st,
                   sp, xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, NULL, st,
                   sp, xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, NULL,
                   sp, xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st,
                   NULL, xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, NULL, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, NULL, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, NULL, need), LDM_EINVAL);
    /* the box and the t range */
    EXPECT_RC(INIT(o, d, B, R, 1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -inf, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, qnan, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 2.f, 1.f, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, qnan, 1.f, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    /* eps > 0, lipschitz > 0, max_steps >= 1, a level */
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 0.f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, -1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, qnan, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 0.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, inf, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, 0, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, qnan, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    /* a mask needs a grid */
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, mk, 1, vs, t, st, sp, xl,
                   li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, mk, N, 0.f, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, mk, 20000, vs, t, st, sp,
                   xl, li, cn, ws, need), LDM_EINVAL);
    /* alignment */
    EXPECT_RC(INIT((float*)off(o, 2), d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0,
                   0.f, t, st, sp, xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, (float*)off(d, 1), B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0,
                   0.f, t, st, sp, xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f,
                   (float*)off(t, 2), st, sp, xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t,
                   (int32_t*)off(st, 2), sp, xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st,
                   (int32_t*)off(sp, 3), xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   (float*)off(xl, 2), li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, (int32_t*)off(li, 1), cn, ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, (int32_t*)off(cn, 2), ws, need), LDM_EALIGN);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, off(ws, 16), need), LDM_EALIGN);
    /* workspace too small */
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, NULL, 0, 0.f, t, st, sp,
                   xl, li, cn, ws, need - 1), LDM_ENOSPC);
    EXPECT_RC(INIT(o, d, B, R, -1.f, 1.f, 0.f, inf, 0.f, 1.f, 1e-3f, MS, mk, N, vs, t, st, sp,
                   NULL, li, cn, ws, 0), LDM_ENOSPC);

    /* emit */
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, 0, R, P, -1.f, t, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, 0, -1.f, t, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, (int)R + 1, -1.f, t, li, cn, xyz, NULL),
              LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(NULL, d, 0, B, R, P, -1.f, t, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, NULL, 0, B, R, P, -1.f, t, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, P, -1.f, NULL, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, P, -1.f, t, NULL, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, P, -1.f, t, li, NULL, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, P, -1.f, t, li, cn, NULL, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 0, B, R, P, qnan, t, li, cn, xyz, NULL), LDM_EINVAL);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 1, B, R, P, -1.f, t, li, cn, (float*)off(xyz, 2), NULL),
              LDM_EALIGN);
    EXPECT_RC(ldm_sdf_trace_emit(o, d, 1, B, R, P, -1.f, (float*)off(t, 1), li, cn, xyz, NULL),
              LDM_EALIGN);

#define STEP(o_, d_, B_, R_, P_, va_, lo_, lv_, L_, e_, mk_, N_, vs_, t_, st_, sp_, xl_, li_, \
             cn_, ws_, wb_)                                                                   \
    ldm_sdf_trace_step(o_, d_, 0, B_, R_, P_, va_, lo_, lv_, L_, e_, mk_, N_, vs_, t_, st_,   \
                       sp_, xl_, li_, cn_, ws_, wb_, NULL)
    EXPECT_RC(STEP(o, d, 0, R, P, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, 0, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, (int)R + 1, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl,
                   li, cn, ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, NULL, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li,
                   cn, ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, NULL, st, sp, xl, li,
                   cn, ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   NULL, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 0.f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, -1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, qnan, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, inf, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, mk, 1, vs, t, st, sp, xl, li, cn, ws,
                   need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, mk, N, -vs, t, st, sp, xl, li, cn,
                   ws, need), LDM_EINVAL);
    EXPECT_RC(STEP(o, d, B, R, P, (float*)off(va, 2), -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st,
                   sp, xl, li, cn, ws, need), LDM_EALIGN);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   off(ws, 128), need), LDM_EALIGN);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, NULL, 0, 0.f, t, st, sp, xl, li, cn,
                   ws, need - 1), LDM_ENOSPC);
    EXPECT_RC(STEP(o, d, B, R, P, va, -1.f, 0.f, 1.f, 1e-3f, mk, N, vs, t, st, sp, NULL, li, cn,
                   ws, 16), LDM_ENOSPC);

    return check_report("sdf_trace_errors");
}
