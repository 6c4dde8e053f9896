// Ray geometry of the sphere tracer (sdf_trace.hip): the slab clip of a ray
// against the box, one marching step, and the walk of a ray through the 8^3-voxel bricks of
// band.hip's classification to the next brick that can hold the surface.
//
// Plain C++ in fp32 with a FIXED operation order and no contraction, host- and device-compilable:
// tests/c/ray_brick_dda_check.cpp runs this header on the CPU, tests/sdf_trace_reference.py
// restates it in numpy, and the three agree bit for bit.  Minima and maxima are written as
// selects (a < b ? a : b), never fminf / fmaxf, so a NaN takes the same way everywhere.
//
// Bricks along one axis (band.hip): nb = ceil(N / 8) of them, the boundaries are the lattice
// coordinates bound(b) = fl(fl(min(8 b, N - 1) * vs) + origin), b = 0..nb (rule A1), so the last
// brick is thinner, and has no width at all when N - 1 is a multiple of 8.  A coordinate x lies
// in the brick  cell(x) = #{ b in [1, nb - 1] : x >= bound(b) }:  every x has a brick, the ones
// outside the lattice that of the nearest face.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDM_RBD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LDM_RBD_HD inline
#endif

namespace ldm {
namespace rbd {

constexpr int kBrick = 8;

struct Ray {
    float o[3], d[3];
};

// the bricks of one shape; mask == nullptr: no skipping
struct Bricks {
    const uint8_t* mask;   // [nb^3] of this shape, (bz nb + by) nb + bx
    int N, nb;
    float vs, origin;
};

LDM_RBD_HD bool finite_f(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

LDM_RBD_HD float sel_min(float a, float b) { return a < b ? a : b; }
LDM_RBD_HD float sel_max(float a, float b) { return a > b ? a : b; }

LDM_RBD_HD float bound(int b, int N, float vs, float origin) {
#pragma clang fp contract(off)
    const int i = kBrick * b < N - 1 ? kBrick * b : N - 1;
    const float t = (float)i * vs;
    return t + origin;
}

LDM_RBD_HD int cell(float x, const Bricks& g) {
    // an estimate from the uniform spacing, then exact against the boundaries themselves
    const float w = (float)kBrick * g.vs;
    float e = (x - g.origin) / w;
    int c = e >= (float)(g.nb - 1) ? g.nb - 1 : (e > 0.0f ? (int)e : 0);   // NaN -> 0
    while (c > 0 && !(x >= bound(c, g.N, g.vs, g.origin))) --c;
    while (c < g.nb - 1 && x >= bound(c + 1, g.N, g.vs, g.origin)) ++c;
    return c;
}

LDM_RBD_HD void point_at(const Ray& r, float t, float p[3]) {
#pragma clang fp contract(off)
    for (int a = 0; a < 3; ++a) {
        const float m = t * r.d[a];
        p[a] = r.o[a] + m;
    }
}

// |d| in a fixed order
LDM_RBD_HD float dir_len(const Ray& r) {
#pragma clang fp contract(off)
    const float xx = r.d[0] * r.d[0], yy = r.d[1] * r.d[1], zz = r.d[2] * r.d[2];
    const float s = xx + yy;
    return sqrtf(s + zz);
}

// Slab clip of the ray against [lo, hi]^3, intersected with [t_min, t_max].  false: the ray
// misses (a non-finite origin, a zero or non-finite direction, or an empty interval).
LDM_RBD_HD bool clip(const Ray& r, float lo, float hi, float t_min, float t_max, float* t0,
                     float* t1) {
#pragma clang fp contract(off)
    bool ok = true, any = false;
    for (int a = 0; a < 3; ++a) {
        ok = ok && finite_f(r.o[a]) && finite_f(r.d[a]);
        any = any || r.d[a] != 0.0f;
    }
    if (!ok || !any) return false;
    float a0 = t_min, a1 = t_max;
    for (int a = 0; a < 3; ++a) {
        if (r.d[a] != 0.0f) {
            const float inv = 1.0f / r.d[a];
            const float ta = (lo - r.o[a]) * inv, tb = (hi - r.o[a]) * inv;
            a0 = sel_max(a0, sel_min(ta, tb));
            a1 = sel_min(a1, sel_max(ta, tb));
        } else if (r.o[a] < lo || r.o[a] > hi) {
            return false;
        }
    }
    if (!(a0 <= a1)) return false;
    *t0 = a0;
    *t1 = a1;
    return true;
}

// From t (<= t_end) forward to the ray's entry into the next active brick: a 3D-DDA over the
// brick boundaries.  false: there is none up to t_end (a miss).  The walk starts in the brick of
// the point o + t d itself (cell() of its three rounded coordinates).  An inactive brick is left
// through the nearest of its three far faces -- the first axis on a tie, so a ray through an
// edge or a corner crosses one face per turn at the same t -- and t never goes back: a crossing
// that the rounding puts before t moves the brick, not t.  A ray crosses at most 3 nb faces.
// The point of the returned t lies in the closure of an active brick up to the rounding of
// o + t d (it was placed ON the face it entered through).
LDM_RBD_HD bool skip(const Ray& r, const Bricks& g, float t_end, float* t_io) {
#pragma clang fp contract(off)
    float t = *t_io;
    float p[3], inv[3];
    int c[3], dir[3];
    point_at(r, t, p);
    for (int a = 0; a < 3; ++a) {
        c[a] = cell(p[a], g);
        inv[a] = r.d[a] != 0.0f ? 1.0f / r.d[a] : 0.0f;
        dir[a] = r.d[a] > 0.0f ? 1 : -1;
    }
    const int turns = 3 * g.nb + 3;
    for (int it = 0; it < turns; ++it) {
        if (g.mask[((size_t)c[2] * g.nb + c[1]) * g.nb + c[0]]) {
            *t_io = t;
            return true;
        }
        float tn = INFINITY;
        int ax = -1;
        for (int a = 0; a < 3; ++a) {
            if (r.d[a] == 0.0f) continue;
            const float face = bound(dir[a] > 0 ? c[a] + 1 : c[a], g.N, g.vs, g.origin);
            const float x = (face - r.o[a]) * inv[a];
            if (ax < 0 || x < tn) {              // a NaN takes an axis only when it is the first
                tn = x;
                ax = a;
            }
        }
        if (ax < 0) return false;                // (no direction: clip() refuses such a ray)
        c[ax] += dir[ax];
        if (c[ax] < 0 || c[ax] >= g.nb) return false;
        t = sel_max(t, tn);
        if (!(t <= t_end)) return false;
    }
    return false;                                // every brick on the way was inactive
}

enum Status { kMiss = 0, kHit = 1, kActive = 2 };

// One marching step on the decoder value v at the current t.
LDM_RBD_HD int step(const Ray& r, const Bricks& g, float v, float level, float lipschitz,
                    float eps, float t_end, float* t_io) {
#pragma clang fp contract(off)
    const float f = v - level;
    if (!finite_f(f) || f <= eps) return kHit;
    const float den = lipschitz * dir_len(r);
    const float q = sel_max(f, eps) / den;
    float t = *t_io + q;
    if (!(t <= t_end)) return kMiss;
    if (g.mask && !skip(r, g, t_end, &t)) return kMiss;
    *t_io = t;
    return kActive;
}

// The start of a ray: its first evaluation point, or a miss.
LDM_RBD_HD int start(const Ray& r, const Bricks& g, float lo, float hi, float t_min, float t_max,
                     float* t_out, float* t_end_out) {
    float t0 = 0.0f, t1 = 0.0f;
    if (!clip(r, lo, hi, t_min, t_max, &t0, &t1)) return kMiss;
    if (g.mask && !skip(r, g, t1, &t0)) return kMiss;
    *t_out = t0;
    *t_end_out = t1;
    return kActive;
}

}  // namespace rbd
}  // namespace ldm
