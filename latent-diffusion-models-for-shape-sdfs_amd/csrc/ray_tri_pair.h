// The ray-triangle pair of ray_mesh.hip: the watertight test of Woop, Benthin
// and Wald (JCGT 2013) in plain fp32.  Host- and device-compilable, so the arithmetic can be
// checked on a CPU against the numpy emulation of tests/ray_mesh_reference.py, bit for bit.
//
// Every function here runs with floating-point contraction OFF and uses no fused multiply-add:
// the result of a pair is a fixed sequence of IEEE operations, the same in every kernel that
// inlines it -- the batch-invariance rule rests on that, and so does watertightness:
//
//   The ray is sheared and its dominant axis scaled so that it runs along +z from the origin;
//   a vertex p becomes (qx, qy) = (q[kx] - Sx q[kz], q[ky] - Sy q[kz]) with q = p - o.  These
//   two numbers depend on the vertex and the ray ALONE, not on the triangle that names the
//   vertex.  The edge function of the edge (B, C) is U = rn(rn(Cx By) - rn(Cy Bx)).  The
//   neighbouring triangle walks the same edge the other way and forms rn(rn(Bx Cy) -
//   rn(By Cx)): the two products are the same two numbers (multiplication commutes exactly),
//   subtracted in the other order, and rn(x - y) = -rn(y - x).  So the neighbour's edge
//   function is exactly -U: a ray cannot be outside both triangles across a shared edge, and
//   U == 0 sides with either, so it is inside at least one.  A fused multiply-add would round
//   Cx By - Cy Bx once, with a different error from each side, and break that.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LDM_RAY_FN __host__ __device__ __forceinline__
#else
#define LDM_RAY_FN static inline
#endif

namespace ldm {

// One packed triangle: 12 floats, 48 bytes: a, b, c, three pads.
struct RayTri {
    float ax, ay, az, bx, by, bz, cx, cy, cz, p0, p1, p2;
};

// What a ray contributes to every pair: its origin, the axis permutation and the shear.
//   kz  the component of d with the largest |d| (ties to the lowest index)
//   kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped when d[kz] < 0
//   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]   (true divisions)
//   ok  false when d[kz] is 0 or not finite or o is not finite: the ray misses everything
struct RayPre {
    float ox, oy, oz, Sx, Sy, Sz;
    int kx, ky, kz;
    bool ok;
};

LDM_RAY_FN float ray_sel3(float x, float y, float z, int k) {
    return k == 0 ? x : (k == 1 ? y : z);
}

LDM_RAY_FN bool ray_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN

LDM_RAY_FN RayPre ray_setup(float ox, float oy, float oz, float dx, float dy, float dz) {
#pragma clang fp contract(off)
    RayPre r;
    r.ox = ox; r.oy = oy; r.oz = oz;
    int kz = 0;
    float m = fabsf(dx);
    if (fabsf(dy) > m) { kz = 1; m = fabsf(dy); }
    if (fabsf(dz) > m) { kz = 2; }
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const float dk = ray_sel3(dx, dy, dz, kz);
    if (dk < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.Sx = ray_sel3(dx, dy, dz, kx) / dk;
    r.Sy = ray_sel3(dx, dy, dz, ky) / dk;
    r.Sz = 1.0f / dk;
    r.ok = dk != 0.0f && ray_finite(dk) && ray_finite(ox) && ray_finite(oy) && ray_finite(oz);
    return r;
}

// The sheared (x, y) of one vertex, and its q[kz].
LDM_RAY_FN void ray_shear(float px, float py, float pz, float ox, float oy, float oz, float Sx,
                          float Sy, int kx, int ky, int kz, float* qx, float* qy, float* qk) {
#pragma clang fp contract(off)
    const float q0 = px - ox, q1 = py - oy, q2 = pz - oz;         // q = vertex - o, first
    const float k = ray_sel3(q0, q1, q2, kz);
    const float mx = Sx * k, my = Sy * k;                         // multiply, then subtract
    *qx = ray_sel3(q0, q1, q2, kx) - mx;
    *qy = ray_sel3(q0, q1, q2, ky) - my;
    *qk = k;
}

// Edge functions and determinant of one pair; returns false when the pair is a miss whatever
// t is: U, V, W of both strict signs, or det == 0.  Ak, Bk, Ck are q[kz] of the vertices.
LDM_RAY_FN bool ray_tri_edges(const RayTri& T, float ox, float oy, float oz, float Sx, float Sy,
                              int kx, int ky, int kz, float* U, float* V, float* W, float* det,
                              float* Ak, float* Bk, float* Ck) {
#pragma clang fp contract(off)
    float Ax, Ay, Bx, By, Cx, Cy;
    ray_shear(T.ax, T.ay, T.az, ox, oy, oz, Sx, Sy, kx, ky, kz, &Ax, &Ay, Ak);
    ray_shear(T.bx, T.by, T.bz, ox, oy, oz, Sx, Sy, kx, ky, kz, &Bx, &By, Bk);
    ray_shear(T.cx, T.cy, T.cz, ox, oy, oz, Sx, Sy, kx, ky, kz, &Cx, &Cy, Ck);
    const float u0 = Cx * By, u1 = Cy * Bx;                       // never fused: see the top
    const float v0 = Ax * Cy, v1 = Ay * Cx;
    const float w0 = Bx * Ay, w1 = By * Ax;
    const float u = u0 - u1, v = v0 - v1, w = w0 - w1;
    const bool neg = u < 0.0f || v < 0.0f || w < 0.0f;
    const bool pos = u > 0.0f || v > 0.0f || w > 0.0f;
    const float d = (u + v) + w;
    *U = u; *V = v; *W = w; *det = d;
    return !(neg && pos) && d != 0.0f;
}

// t of a pair that ray_tri_edges let through: products, then sums, then one true division.
LDM_RAY_FN float ray_tri_t(float U, float V, float W, float det, float Sz, float Ak, float Bk,
                           float Ck) {
#pragma clang fp contract(off)
    const float Az = Sz * Ak, Bz = Sz * Bk, Cz = Sz * Ck;
    const float ta = U * Az, tb = V * Bz, tc = W * Cz;
    const float T = (ta + tb) + tc;
    return T / det;
}

// The whole pair: true and *t for a hit with t_min <= t <= t_max; bary (or NULL) gets the
// weights of a, b, c, U / det, V / det, W / det.
LDM_RAY_FN bool ray_tri_pair(const RayTri& T, const RayPre& r, float t_min, float t_max,
                             float* t, float* bary) {
#pragma clang fp contract(off)
    float U, V, W, det, Ak, Bk, Ck;
    const bool cand = ray_tri_edges(T, r.ox, r.oy, r.oz, r.Sx, r.Sy, r.kx, r.ky, r.kz, &U, &V,
                                    &W, &det, &Ak, &Bk, &Ck);
    if (!cand || !r.ok) return false;
    const float tt = ray_tri_t(U, V, W, det, r.Sz, Ak, Bk, Ck);
    if (!(tt >= t_min && tt <= t_max)) return false;
    *t = tt;
    if (bary) {
        bary[0] = U / det;
        bary[1] = V / det;
        bary[2] = W / det;
    }
    return true;
}

}  // namespace ldm
