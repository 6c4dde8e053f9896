// What mesh_sdf.hip (points against a triangle soup) and ray_mesh.hip (rays against one) have in
// common around their different inner loops: the face loader of the pack kernels, the launch
// plan (chunks of faces, the one-pass / tiled-split switch, the workspace) and the argument
// checks both entries make.  The pair arithmetic, the partials and the combine kernels differ
// and stay in their files.
#pragma once
#include "ldm_internal.h"

namespace ldm {

// face f: its indices clamped to [0, V) (a clamp raises *flag), its vertices k = 0..2 to p[k]
__device__ __forceinline__ void soup_load_face(const float* __restrict__ verts, int V,
                                               const int32_t* __restrict__ faces, int64_t f,
                                               int32_t* __restrict__ flag, float (&p)[3][3]) {
    int id[3];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int raw = faces[f * 3 + k];
        id[k] = min(max(raw, 0), V - 1);
        bad = bad || id[k] != raw;
    }
    if (bad) atomicOr(flag, 1);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[k][c] = verts[(int64_t)id[k] * 3 + c];
}

// Faces are cut into chunks of `face_chunk`.  n >= split_below queries, or one chunk: the
// one-pass form, a thread walks every chunk.  Else the split form: grid.y = chunks, partials
// [chunk][tile query] to the workspace per tile of `split_tile` queries, then a combine.
// Workspace: 256 bytes, the packed records, the partials of one tile.
struct SoupPlan {
    int F;
    int64_t n, split_below;
    int nchunk;
    bool split;
    size_t tri_bytes, part_bytes, ws_bytes;
    int tile_stride;    // partials between two chunks of a tile
    int64_t blocks;     // workgroups of the one-pass form, 256 queries each
};

inline SoupPlan soup_plan(int face_chunk, int64_t split_below, int split_tile, size_t record,
                          size_t partial, int F, int64_t n) {
    SoupPlan p{};
    p.F = F;
    p.n = n;
    p.split_below = split_below;
    p.nchunk = (int)(((int64_t)F + face_chunk - 1) / face_chunk);
    p.split = n < split_below && p.nchunk > 1;
    p.tile_stride = (int)(n < split_tile ? n : split_tile);
    p.tri_bytes = up256((size_t)F * record);
    p.part_bytes = p.split ? up256((size_t)p.nchunk * (size_t)p.tile_stride * partial) : 0;
    p.ws_bytes = 256 + p.tri_bytes + p.part_bytes;
    p.blocks = (n + 255) / 256;
    return p;
}

// The checks both entries make, in the entries' order, with the grids of both forms: nothing is
// queued before a refusal.  `q` is the query count's letter in the messages ('P' or 'R');
// `have` says the entry's own required pointers (named in `required`) are not NULL, `aligned`
// that its own alignment list holds -- the lists stay with the entries.  n == 0 is success
// before any pointer is looked at: the entry returns then.
inline int soup_check_args(const char* entry, char q, const SoupPlan& p, int V, const void* verts,
                           const void* faces, bool have, const char* required, bool aligned,
                           size_t ws_bytes) {
    LDM_REQUIRE(V >= 0 && p.F >= 0 && p.n >= 0, LDM_EINVAL,
                "%s: negative size (V = %d, F = %d, %c = %lld)", entry, V, p.F, q, (long long)p.n);
    if (p.n == 0) return 0;
    LDM_REQUIRE(have, LDM_EINVAL, "%s: NULL %s", entry, required);
    LDM_REQUIRE(p.F == 0 || (verts && faces && V > 0), LDM_EINVAL,
                "%s: %d faces need vertices (V = %d) and indices", entry, p.F, V);
    LDM_REQUIRE(aligned, LDM_EALIGN, "%s: tensors must be 4-B, the workspace 256-B aligned", entry);
    LDM_REQUIRE(ws_bytes >= p.ws_bytes, LDM_ENOSPC, "%s: workspace %zu < %zu B", entry, ws_bytes,
                p.ws_bytes);
    LDM_REQUIRE(p.split || p.blocks <= 0x7fffffff, LDM_EINVAL,
                "%s: %c = %lld needs more than 2^31 - 1 workgroups", entry, q, (long long)p.n);
    LDM_REQUIRE(!p.split || p.nchunk <= 65535, LDM_EINVAL,
                "%s: F = %d is %d chunks, above the 65535 of grid.y, with %c = %lld below %lld",
                entry, p.F, p.nchunk, q, (long long)p.n, (long long)p.split_below);
    return 0;
}

}  // namespace ldm
