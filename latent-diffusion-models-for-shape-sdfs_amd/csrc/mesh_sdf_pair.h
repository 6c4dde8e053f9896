// The point-triangle pair of mesh_sdf.hip: squared distance in Voronoi-region
// form and half the solid angle.  Plain fp32, host- and device-compilable, so the arithmetic can
// be checked on a CPU against tests/mesh_sdf_reference.py.
//
// Every function here runs with floating-point contraction OFF and spells its fused
// multiply-adds out: the result of a pair is then a fixed sequence of IEEE operations, the same
// in every kernel that inlines it -- the batch-invariance rule rests on that.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LDM_PAIR_FN __host__ __device__ __forceinline__
#else
#define LDM_PAIR_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define LDM_PAIR_RCP(x) __builtin_amdgcn_rcpf(x)      // v_rcp_f32, 1 ulp
#define LDM_PAIR_SQRT(x) __builtin_amdgcn_sqrtf(x)    // v_sqrt_f32, 1 ulp
#else
#define LDM_PAIR_RCP(x) (1.0f / (x))
#define LDM_PAIR_SQRT(x) sqrtf(x)
#endif

namespace ldm {

// One packed triangle: 20 floats, 80 bytes.
//   [0..2] a   [3] ab.x   [4..6] b   [7] ab.y   [8..10] c   [11] ab.z   [12..14] ac   [15] n.n
//   [16..18] n = ab x ac   [19] 0
// with ab = b - a, ac = c - a, n and n.n each formed once, by the pack kernel (mesh_tri_pack).
struct MeshTri {
    float ax, ay, az, abx, bx, by, bz, aby, cx, cy, cz, abz, acx, acy, acz, nn, nx, ny, nz, pad;
};

LDM_PAIR_FN float pair_dot(float x0, float y0, float z0, float x1, float y1, float z1) {
#pragma clang fp contract(off)
    return fmaf(x0, x1, fmaf(y0, y1, z0 * z1));
}

LDM_PAIR_FN MeshTri mesh_tri_pack(const float* a, const float* b, const float* c) {
#pragma clang fp contract(off)
    MeshTri T;
    T.ax = a[0]; T.ay = a[1]; T.az = a[2];
    T.bx = b[0]; T.by = b[1]; T.bz = b[2];
    T.cx = c[0]; T.cy = c[1]; T.cz = c[2];
    T.abx = b[0] - a[0]; T.aby = b[1] - a[1]; T.abz = b[2] - a[2];
    T.acx = c[0] - a[0]; T.acy = c[1] - a[1]; T.acz = c[2] - a[2];
    T.nx = fmaf(T.aby, T.acz, -(T.abz * T.acy));
    T.ny = fmaf(T.abz, T.acx, -(T.abx * T.acz));
    T.nz = fmaf(T.abx, T.acy, -(T.aby * T.acx));
    T.nn = pair_dot(T.nx, T.ny, T.nz, T.nx, T.ny, T.nz);
    T.pad = 0.0f;
    return T;
}

// atan2(y, x) for y != 0, finite arguments and max(|x|, |y|) a normal number: one reciprocal
// and an odd polynomial of degree 15 on [0, 1] (absolute error 1.7e-7 in fp32, against 1.2e-7
// for one rounding of pi).  v_rcp_f32 reads a denormal as 0, so with both arguments denormal
// t is inf or NaN.  pair_eval's arguments are a triple product and a sum of cubic terms of the
// three corner distances: both denormal with the first nonzero needs all three distances
// near 1e-13, a point on a triangle 1e-13 across, which no mesh normalised to the unit
// sphere in fp32 holds; a guard would cost every pair a compare and a select.
LDM_PAIR_FN float pair_atan2_nz(float y, float x) {
#pragma clang fp contract(off)
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * LDM_PAIR_RCP(mx);
    const float s = t * t;
    float p = -0.004668773151934147f;
    p = fmaf(p, s, 0.02416618913412094f);
    p = fmaf(p, s, -0.0593671016395092f);
    p = fmaf(p, s, 0.09906096756458282f);
    p = fmaf(p, s, -0.14016585052013397f);
    p = fmaf(p, s, 0.19969235360622406f);
    p = fmaf(p, s, -0.33331960439682007f);
    p = fmaf(p, s, 0.9999998807907104f);
    float r = p * t;
    r = ay > ax ? 1.57079632679489662f - r : r;
    r = x < 0.0f ? 3.14159265358979324f - r : r;
    return copysignf(r, y);
}

// Squared distance from p to the triangle and half its solid angle seen from p.
//   distance: Ericson, Real-Time Collision Detection §5.1.5, regions in the order A, B, AB, C,
//             AC, BC, face; the closest point is a + v ab + w ac, one division per pair, and a
//             zero denominator gives 0 (edge BC: b + t (c - b), so b when b == c).  p - a is
//             formed before any product.  Ericson's va, vb, vc (d3 d6 - d5 d4, ...) are taken
//             in their equal cross-product form n . (bp x cp), n . (cp x ap), n . (ap x bp)
//             (Lagrange's identity) and their sum as n . n: a triangle whose n is exactly 0
//             then has va = vb = vc = 0 exactly and is its segment or point for EVERY p,
//             where the products of rounded dot products leave rounding noise of either sign
//             and, once in a while, the face formula on noise / noise.
//   angle:    Van Oosterom-Strackee; a triple product of exactly 0 contributes 0.
LDM_PAIR_FN void pair_eval(const MeshTri& T, float px, float py, float pz, float* d2_out,
                           float* half_omega) {
#pragma clang fp contract(off)
    const float apx = px - T.ax, apy = py - T.ay, apz = pz - T.az;
    const float bpx = px - T.bx, bpy = py - T.by, bpz = pz - T.bz;
    const float cpx = px - T.cx, cpy = py - T.cy, cpz = pz - T.cz;
    const float d1 = pair_dot(T.abx, T.aby, T.abz, apx, apy, apz);
    const float d2 = pair_dot(T.acx, T.acy, T.acz, apx, apy, apz);
    const float d3 = pair_dot(T.abx, T.aby, T.abz, bpx, bpy, bpz);
    const float d4 = pair_dot(T.acx, T.acy, T.acz, bpx, bpy, bpz);
    const float d5 = pair_dot(T.abx, T.aby, T.abz, cpx, cpy, cpz);
    const float d6 = pair_dot(T.acx, T.acy, T.acz, cpx, cpy, cpz);
    const float crx = fmaf(bpy, cpz, -(bpz * cpy));            // bp x cp
    const float cry = fmaf(bpz, cpx, -(bpx * cpz));
    const float crz = fmaf(bpx, cpy, -(bpy * cpx));
    const float va = pair_dot(T.nx, T.ny, T.nz, crx, cry, crz);
    const float vb = pair_dot(T.nx, T.ny, T.nz, fmaf(cpy, apz, -(cpz * apy)),
                              fmaf(cpz, apx, -(cpx * apz)), fmaf(cpx, apy, -(cpy * apx)));
    const float vc = pair_dot(T.nx, T.ny, T.nz, fmaf(apy, bpz, -(apz * bpy)),
                              fmaf(apz, bpx, -(apx * bpz)), fmaf(apx, bpy, -(apy * bpx)));
    const float e43 = d4 - d3, e56 = d5 - d6;
    // reverse priority: the face region first, every earlier region overrides
    float nv = vb, nw = vc, den = T.nn;
    bool bc = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
    nw = bc ? e43 : nw;
    den = bc ? e43 + e56 : den;
    bool m = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;          // edge AC
    nv = m ? 0.0f : nv; nw = m ? d2 : nw; den = m ? d2 - d6 : den; bc = bc && !m;
    m = d6 >= 0.0f && d5 <= d6;                               // vertex C
    nv = m ? 0.0f : nv; nw = m ? 1.0f : nw; den = m ? 1.0f : den; bc = bc && !m;
    m = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;               // edge AB
    nv = m ? d1 : nv; nw = m ? 0.0f : nw; den = m ? d1 - d3 : den; bc = bc && !m;
    m = d3 >= 0.0f && d4 <= d3;                               // vertex B
    nv = m ? 1.0f : nv; nw = m ? 0.0f : nw; den = m ? 1.0f : den; bc = bc && !m;
    m = d1 <= 0.0f && d2 <= 0.0f;                             // vertex A
    nv = m ? 0.0f : nv; nw = m ? 0.0f : nw; den = m ? 1.0f : den; bc = bc && !m;
    const float r = den == 0.0f ? 0.0f : 1.0f / den;
    const float w = nw * r;
    const float v = bc ? 1.0f - w : nv * r;
    const float qx = fmaf(-w, T.acx, fmaf(-v, T.abx, apx));
    const float qy = fmaf(-w, T.acy, fmaf(-v, T.aby, apy));
    const float qz = fmaf(-w, T.acz, fmaf(-v, T.abz, apz));
    *d2_out = pair_dot(qx, qy, qz, qx, qy, qz);

    // A = -ap, B = -bp, C = -cp: the dot products keep their sign, the triple product flips
    const float det = -pair_dot(apx, apy, apz, crx, cry, crz);
    const float la = LDM_PAIR_SQRT(pair_dot(apx, apy, apz, apx, apy, apz));
    const float lb = LDM_PAIR_SQRT(pair_dot(bpx, bpy, bpz, bpx, bpy, bpz));
    const float lc = LDM_PAIR_SQRT(pair_dot(cpx, cpy, cpz, cpx, cpy, cpz));
    const float dab = pair_dot(apx, apy, apz, bpx, bpy, bpz);
    const float dbc = pair_dot(bpx, bpy, bpz, cpx, cpy, cpz);
    const float dca = pair_dot(cpx, cpy, cpz, apx, apy, apz);
    const float dn = fmaf(dca, lb, fmaf(dbc, la, fmaf(dab, lc, (la * lb) * lc)));
    // (the atan2 of a zero triple product is evaluated on y = 1 and discarded)
    const float ang = pair_atan2_nz(det == 0.0f ? 1.0f : det, dn);
    *half_omega = det == 0.0f ? 0.0f : ang;
}

}  // namespace ldm
