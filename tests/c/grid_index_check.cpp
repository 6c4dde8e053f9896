// csrc/grid_index.h against / and %: the decoder's tile prologue must name the voxels that
// grid_point() (decoder_common.h: k0 + p / N^2, p % N^2 / N, p % N^2 % N) names, for every tile
// and lane.  Built and run on the CPU by tests/test_grid_index.py; prints one line and exits 0,
// or the first mismatch and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include "grid_index.h"

using namespace ldm::dec;

static long long n_checked = 0;

// every lane of the tile that holds slab point p (npts points in the slab, first layer k0)
static int check_tile(uint32_t N, const GridDiv& d, uint32_t k0, uint32_t npts, uint32_t p) {
    const uint32_t p0 = p / 128u * 128u;
    uint32_t ti, tj, tk;
    grid_first(p0, N, d, ti, tj, tk);
    for (uint32_t want = 0; want < 128u; ++want) {
        const uint32_t off = grid_tail_off(p0, want, npts);
        uint32_t i, j, k;
        grid_voxel(ti, tj, k0 + tk, off, N, d.m, i, j, k);
        // today's form: min(pt, npts - 1), then grid_point's divisions
        uint32_t pt = p0 + want;
        if (pt >= npts) pt = npts - 1;
        const uint32_t nn = N * N;
        const uint32_t rk = k0 + pt / nn, r = pt - (pt / nn) * nn, rj = r / N, ri = r - rj * N;
        ++n_checked;
        if (i != ri || j != rj || k != rk) {
            printf("N=%u k0=%u npts=%u p0=%u lane offset %u: got (%u,%u,%u) want (%u,%u,%u)\n", N,
                   k0, npts, p0, want, i, j, k, ri, rj, rk);
            return 1;
        }
    }
    return 0;
}

// points q - 1, q and q + 1 alone, each as the lane of its tile that holds it
static int points_around(uint32_t N, const GridDiv& d, uint32_t k0, uint32_t npts, long long q) {
    for (long long pp = q - 1; pp <= q + 1; ++pp) {
        if (pp < 0 || pp >= (long long)npts) continue;
        const uint32_t p = (uint32_t)pp, p0 = p / 128u * 128u;
        uint32_t ti, tj, tk, i, j, k;
        grid_first(p0, N, d, ti, tj, tk);
        grid_voxel(ti, tj, k0 + tk, grid_tail_off(p0, p - p0, npts), N, d.m, i, j, k);
        const uint32_t nn = N * N;
        const uint32_t rk = k0 + p / nn, r = p % nn, rj = r / N, ri = r % N;
        ++n_checked;
        if (i != ri || j != rj || k != rk) {
            printf("N=%u k0=%u npts=%u p=%u: got (%u,%u,%u) want (%u,%u,%u)\n", N, k0, npts, p, i,
                   j, k, ri, rj, rk);
            return 1;
        }
    }
    return 0;
}

// every lane of the tiles around point q, q - 1 and q + 1 of an npts-point slab
static int around(uint32_t N, const GridDiv& d, uint32_t k0, uint32_t npts, long long q) {
    for (long long p = q - 1; p <= q + 1; ++p)
        if (p >= 0 && p < (long long)npts && check_tile(N, d, k0, npts, (uint32_t)p)) return 1;
    return 0;
}

int main() {
    const long long cap = 1ll << 27;
    for (uint32_t N = 2; N <= 1024; ++N) {
        const GridDiv d = grid_div((int)N);
        const long long nn = (long long)N * N;
        const long long full = nn * N < cap ? nn * N : cap;
        // the whole volume, capped at 2^27 points: every multiple of N, +- 1, as a point; every
        // multiple of N^2, +- 1, with all 128 lanes of its tile; the last tile
        for (long long q = 0; q <= full; q += N)
            if (points_around(N, d, 0, (uint32_t)full, q)) return 1;
        for (long long q = 0; q <= full; q += nn)
            if (around(N, d, 0, (uint32_t)full, q)) return 1;
        if (around(N, d, 0, (uint32_t)full, full - 1)) return 1;
        // slabs [k0, k1): one layer at the top, two in the middle, all but the first; their
        // last tiles are ragged (clamped lanes) wherever 128 does not divide the point count
        const uint32_t slabs[3][2] = {{N - 1, N}, {N / 2, N / 2 + 2 <= N ? N / 2 + 2 : N}, {1, N}};
        for (int s = 0; s < 3; ++s) {
            const uint32_t k0 = slabs[s][0], k1 = slabs[s][1];
            const long long np = (long long)(k1 - k0) * nn;
            if (k1 <= k0 || np > cap) continue;
            for (long long q = 0; q <= np; q += nn)
                if (around(N, d, k0, (uint32_t)np, q)) return 1;
            if (k1 - k0 <= 2)
                for (long long q = 0; q <= np; q += N)
                    if (points_around(N, d, k0, (uint32_t)np, q)) return 1;
            if (around(N, d, k0, (uint32_t)np, np - 1)) return 1;
        }
    }
    // every point of the small grids (N below the tile's 128 points: several carries a lane)
    for (uint32_t N = 2; N <= 40; ++N) {
        const GridDiv d = grid_div((int)N);
        for (uint32_t k0 = 0; k0 < N; k0 += (N > 8 ? N / 3 : 1))
            for (uint32_t k1 = k0 + 1; k1 <= N; k1 += (N > 8 ? N / 4 : 1)) {
                const uint32_t np = (k1 - k0) * N * N;
                for (uint32_t p = 0; p < np; p += 128)
                    if (check_tile(N, d, k0, np, p)) return 1;
            }
    }
    // the largest slabs the C ABI admits: one layer of N = 46340 (N^2 < 2^31)
    {
        const uint32_t N = 46340;
        const GridDiv d = grid_div((int)N);
        const uint32_t np = N * N;
        for (long long q = 0; q <= np; q += (long long)N * 997)
            if (around(N, d, N - 1, np, q)) return 1;
        if (around(N, d, N - 1, np, np - 1)) return 1;
    }
    printf("grid_index ok: %lld lane voxels\n", n_checked);
    return 0;
}
