// Runs csrc/ray_brick_dda.h -- the header the sphere tracer's kernels compile -- on the host, so
// that tests/test_sdf_trace_reference.py can hold the numpy restatement to it bit for bit
// and check the brick walk against brute force.  Stand-alone: no GPU, no library.
//
//   ray_brick_dda_check IN OUT
// IN : int64 n, int64 N, int64 use_mask; float lo, hi, t_min, t_max, vs, level, lipschitz, eps;
//      uint8 mask[nb^3] (nb = ceil(N / 8); present also when unused); n records of 7 floats:
//      origin, direction, and a decoder value v
// OUT: n records of 5 uint32: start()'s status, t, t_end (bit patterns), then step()'s status
//      and t when the ray, started, is given the value v at its first point (status 0, t as
//      started, for a ray that did not start)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ray_brick_dda.h"

using namespace ldm::rbd;

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[3];
    float par[8];
    if (std::fread(head, 8, 3, in) != 3 || std::fread(par, 4, 8, in) != 8) return 2;
    const int64_t n = head[0];
    const int N = (int)head[1], nb = (N + kBrick - 1) / kBrick;
    if (n < 0 || N < 2 || nb > 4096) return 2;
    std::vector<uint8_t> mask((size_t)nb * nb * nb);
    if (std::fread(mask.data(), 1, mask.size(), in) != mask.size()) return 2;
    std::vector<float> rec((size_t)n * 7);
    if (std::fread(rec.data(), 4, rec.size(), in) != rec.size()) return 2;
    std::fclose(in);
    const float lo = par[0], hi = par[1], t_min = par[2], t_max = par[3], vs = par[4];
    const float level = par[5], lipschitz = par[6], eps = par[7];
    Bricks g;
    g.mask = head[2] ? mask.data() : nullptr;
    g.N = N;
    g.nb = nb;
    g.vs = vs;
    g.origin = lo;
    std::vector<uint32_t> out((size_t)n * 5);
    for (int64_t i = 0; i < n; ++i) {
        Ray r;
        for (int a = 0; a < 3; ++a) {
            r.o[a] = rec[i * 7 + a];
            r.d[a] = rec[i * 7 + 3 + a];
        }
        float t = INFINITY, t_end = INFINITY;
        const int st = start(r, g, lo, hi, t_min, t_max, &t, &t_end);
        int st2 = kMiss;
        float t2 = t;
        if (st == kActive) st2 = step(r, g, rec[i * 7 + 6], level, lipschitz, eps, t_end, &t2);
        out[i * 5 + 0] = (uint32_t)st;
        out[i * 5 + 1] = bits(t);
        out[i * 5 + 2] = bits(t_end);
        out[i * 5 + 3] = (uint32_t)st2;
        out[i * 5 + 4] = bits(t2);
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), 4, out.size(), fo) != out.size()) return 2;
    std::fclose(fo);
    std::printf("ray_brick_dda ok: %lld rays\n", (long long)n);
    return 0;
}
