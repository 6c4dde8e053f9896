// Runs the ray-triangle pair of csrc/ray_tri_pair.h on the host, so that
// tests/test_render_host.py can compare it bit for bit with the numpy emulation of
// tests/ray_mesh_reference.py and check watertightness on the product arithmetic.  No GPU.
//
//   ray_pair_check IN OUT            single pairs
//     IN   int64 n, then n records of 17 float32: o[3] d[3] a[3] b[3] c[3] t_min t_max
//     OUT  n records of 5 x 4 bytes: uint32 hit, float32 t, bary[3] (zeros for a miss)
//   ray_pair_check --mesh IN OUT     every ray against every face, the closest hit
//     IN   int64 R, int64 F, float32 t_min, t_max, R records o[3] d[3], F records a[3] b[3] c[3]
//     OUT  R records of 5 x 4 bytes: int32 face (-1 for a miss), float32 t (+inf), bary[3] (0):
//          the lexicographic minimum of (t, face) over the hits, as csrc/ray_mesh.hip forms it
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ray_tri_pair.h"

static_assert(sizeof(float) == sizeof(uint32_t), "float32");

static bool read_all(const char* path, std::vector<char>* buf) {
    std::FILE* in = std::fopen(path, "rb");
    if (!in) return false;
    char chunk[1 << 16];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof chunk, in)) > 0) buf->insert(buf->end(), chunk, chunk + n);
    std::fclose(in);
    return true;
}

static ldm::RayTri tri_of(const float* p) {
    ldm::RayTri T;
    T.ax = p[0]; T.ay = p[1]; T.az = p[2];
    T.bx = p[3]; T.by = p[4]; T.bz = p[5];
    T.cx = p[6]; T.cy = p[7]; T.cz = p[8];
    T.p0 = T.p1 = T.p2 = 0.0f;
    return T;
}

static int run_pairs(const std::vector<char>& buf, std::vector<uint32_t>* out) {
    int64_t n = 0;
    if (buf.size() < sizeof n) return 2;
    std::memcpy(&n, buf.data(), sizeof n);
    if (n < 0 || buf.size() != sizeof n + (size_t)n * 17 * sizeof(float)) return 2;
    const float* rec = reinterpret_cast<const float*>(buf.data() + sizeof n);
    out->assign((size_t)n * 5, 0u);
    int64_t hits = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float* r = rec + (size_t)i * 17;
        const ldm::RayPre ray = ldm::ray_setup(r[0], r[1], r[2], r[3], r[4], r[5]);
        float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const bool hit = ldm::ray_tri_pair(tri_of(r + 6), ray, r[15], r[16], &res[0], &res[1]);
        uint32_t* o = out->data() + (size_t)i * 5;
        o[0] = hit ? 1u : 0u;
        if (hit) {
            std::memcpy(o + 1, res, sizeof res);
            ++hits;
        }
    }
    std::printf("ray_pair ok: %lld pairs, %lld hits\n", (long long)n, (long long)hits);
    return 0;
}

static int run_mesh(const std::vector<char>& buf, std::vector<uint32_t>* out) {
    int64_t R = 0, F = 0;
    float bounds[2];
    const size_t head = 2 * sizeof(int64_t) + sizeof bounds;
    if (buf.size() < head) return 2;
    std::memcpy(&R, buf.data(), sizeof R);
    std::memcpy(&F, buf.data() + sizeof R, sizeof F);
    std::memcpy(bounds, buf.data() + 2 * sizeof R, sizeof bounds);
    if (R < 0 || F < 0 || buf.size() != head + ((size_t)R * 6 + (size_t)F * 9) * sizeof(float))
        return 2;
    const float* rays = reinterpret_cast<const float*>(buf.data() + head);
    const float* tris = rays + (size_t)R * 6;
    std::vector<ldm::RayTri> T((size_t)F);
    for (int64_t f = 0; f < F; ++f) T[(size_t)f] = tri_of(tris + (size_t)f * 9);
    out->assign((size_t)R * 5, 0u);
    int64_t hits = 0;
    for (int64_t i = 0; i < R; ++i) {
        const float* r = rays + (size_t)i * 6;
        const ldm::RayPre ray = ldm::ray_setup(r[0], r[1], r[2], r[3], r[4], r[5]);
        float best[4] = {INFINITY, 0.0f, 0.0f, 0.0f};
        int32_t bface = -1;
        for (int64_t f = 0; f < F; ++f) {
            float res[4];
            // strict: the smaller index keeps a tie
            if (ldm::ray_tri_pair(T[(size_t)f], ray, bounds[0], bounds[1], &res[0], &res[1]) &&
                res[0] < best[0]) {
                std::memcpy(best, res, sizeof res);
                bface = (int32_t)f;
            }
        }
        uint32_t* o = out->data() + (size_t)i * 5;
        std::memcpy(o, &bface, sizeof bface);
        std::memcpy(o + 1, best, sizeof best);
        hits += bface >= 0;
    }
    std::printf("ray_pair ok: %lld rays x %lld faces, %lld rays hit\n", (long long)R,
                (long long)F, (long long)hits);
    return 0;
}

int main(int argc, char** argv) {
    const bool mesh = argc == 4 && std::strcmp(argv[1], "--mesh") == 0;
    if (!mesh && argc != 3) {
        std::fprintf(stderr, "usage: %s [--mesh] IN OUT\n", argv[0]);
        return 2;
    }
    const char* src = argv[argc - 2];
    const char* dst = argv[argc - 1];
    std::vector<char> buf;
    if (!read_all(src, &buf)) {
        std::fprintf(stderr, "cannot read %s\n", src);
        return 2;
    }
    std::vector<uint32_t> out;
    const int rc = mesh ? run_mesh(buf, &out) : run_pairs(buf, &out);
    if (rc != 0) {
        std::fprintf(stderr, "%s is cut short or malformed\n", src);
        return rc;
    }
    std::FILE* of = std::fopen(dst, "wb");
    if (!of || std::fwrite(out.data(), sizeof(uint32_t), out.size(), of) != out.size()) {
        std::fprintf(stderr, "cannot write %s\n", dst);
        return 2;
    }
    std::fclose(of);
    return 0;
}
