// Feature-split MFMA decoder (weight layout LDM_LAYOUT_SPLIT): SURVEY.md §8(a) A1+A3.
//
// The operand maps of DESIGN.md §3 (v_mfma_f32_32x32x16, accumulator rows as the next layer's B
// fragment) with the work inside a workgroup split by output feature (DESIGN.md §4 "split
// kernel"; it superseded the round-1/2 pass8 and quarter kernels, removed in ABI 5):
//   * a tile is 128 points = 4 point chunks (n) of 32, shared by the workgroup's 4 waves;
//   * wave w owns the OUTPUT FEATURES [128w, 128w+128) of every 512-wide layer as two parts of
//     64 rows (2 m-chunks of 32); the one-part layer 3 of DeepSDF (253 -> 256) gives each wave
//     rows [64w, 64w+64);
//   * the tile's activations live once, in LDS, as B fragments (128 KiB, 32 positions of 4
//     point chunks x 1 KiB; position 32 = the tile's xyz fragments of the aux steps); every
//     wave reads every position's 4 B fragments;
//   * each wave streams ITS OWN weight fragments (2 per k-step, 2 KiB) from L2 straight into a
//     register ring (raw buffer loads, kFsD k-steps ahead): no LDS ring, no DMA barrier.
//     Per k-step a wave reads 2 A fragments (L2) + 4 B fragments (LDS) for 8 MFMAs: each
//     fragment feeds 4 (A) or 2 (B) MFMAs (the removed quarter kernel read one LDS fragment
//     per MFMA); each weight byte feeds the tile's 128 points.
//   * a part's accumulators (2 m x 4 n tiles = 128 fp32) alternate between two sets A and B,
//     and a finished set is converted (16-bit + ReLU) straight into LDS inside a 16-step
//     window of a LATER part, half a tile per step, between its MFMAs:
//       - a layer's part 1 (set B) -> the "late" positions 16..31, during the next layer's
//         part 0 steps 0-14; a barrier inside its step 15 publishes them;
//       - a layer's part 0 (set A) -> the "early" positions 0..15, during the SAME layer's
//         part 1 steps 16-30: part 1 reads the early positions in steps 0-15, so after the
//         barrier inside its step 15 no wave reads them any more; the barrier inside its
//         step 31 publishes them to the next layer;
//       - layer 7's parts fold into the final 512 -> 1 dot product instead (fp32, w_last):
//         part 0 during part 1, part 1 during the NEXT tile's layer 1 part 0 (which also
//         stores the previous tile's outputs).
//     The barriers sit INSIDE a step, after its first MFMA pair, so the next position's reads
//     after them stay covered by the step's remaining MFMAs.  Serial LDS writes: layer 0
//     (both parts) and layer 3 of DeepSDF.
//   * the bias (and, for layers 0 and 4, xyz + the folded latent) enters as one aux MFMA step
//     at the START of each part (A = [wx,wy,wz,wx,wy,wz,b_hi,b_lo], B = [x_hi,y_hi,z_hi,x_lo,
//     y_lo,z_lo,1,1]), which also zero-initialises the accumulators.
// Barriers per tile: 3 per layer.
#include "decoder_common.h"

namespace ldm {
namespace {
using namespace dec;

// k-steps of A fragments in flight per wave (register ring depth = one 4-step stream group)
constexpr int kFsD = 4;
// History: a kernel-variant template parameter carried two switches until it was frozen
// (DESIGN.md §5 "Retired build knobs").  Bit 1, one LDS base per 4-step group instead of an
// address per step, measured +0.5 % (profiles/r04b/ab_decoder_v.log, r04a/
// ab_decoder_groupbase.log) and is what group4 does.  Bit 0, the in-stream barrier after the
// step's SECOND MFMA pair instead of its first, never became the default (no log kept) and is
// gone.  Also measured and dropped: layers 2..7 as one runtime loop with every part kind inlined
// once (74 -> 50 KB of code, 1.2 % slower: profiles/r04b/ab_decoder_v.log).

constexpr int kFsStep = 2048;                       // one wave's A fragments of one k-step
// activation buffer: 32 positions of 4 KiB + position 32 = the tile's aux B fragments
// [x_hi,y_hi,z_hi,x_lo,y_lo,z_lo,1,1] (every part's last step reads it for the next aux step)
constexpr int kFsAct = 33 * 4 * 1024;
constexpr int kFsRed = 4 * 4 * 64 * 4;              // final partials [wave][n][64 lanes] fp32
constexpr int kFsWl = 512 * 4;                      // permuted final-layer weights
// Diagnostic build only (-DFS_STAMP=1, scripts/stamp_split.py; results are wrong): wave 0 of
// every workgroup stamps s_memtime at part and layer boundaries of its second tile, dumped over
// the output at the end.
#ifndef FS_STAMP
#define FS_STAMP 0
#endif
constexpr int kFsStamp = FS_STAMP ? 128 * 8 : 0;
// Diagnostic ablations (stamp builds only, results wrong; scripts/stamp_split.py, DESIGN.md §4
// round 6): FS_ABL bit 0 = no weight stream (the ring keeps its registers), bit 1 = no epilogue
// units, bit 2 = no in-stream barriers
#ifndef FS_ABL
#define FS_ABL 0
#endif
static_assert(FS_ABL == 0 || FS_STAMP, "ablations are diagnostic builds");
constexpr int kFsLds = kFsAct + kFsRed + kFsWl + kFsStamp;
static_assert(kFsLds <= 160 * 1024, "LDS");

__host__ __device__ constexpr int fs_nparts(int S) { return S == 256 ? 15 : 16; }
__host__ __device__ constexpr int fs_nsteps(int S) { return S == 256 ? 384 : 448; }

// ------------------------------------------------------------------------------------------
// per-shape aux fragments: [B][4 waves][4 slots: L0p0, L0p1, L4p0, L4p1][2 frags][64][8].
// Lane < 32 of frag i: [wx, wy, wz, wx, wy, wz, beta_hi, beta_lo] of row 128w + 64p + 32i +
// lane (layers 0 and 4 are 512 wide); lanes >= 32 zero (they meet zero B rows: must be finite).
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void fs_aux_pack_kernel(const float* __restrict__ beta, const float* __restrict__ wxyz,
                                   int B, T* __restrict__ aux) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;   // (b, w, slot, i, lane)
    if (id >= B * 4 * 4 * 2 * 64) return;
    const int lane = id & 63;
    const int i = (id >> 6) & 1;
    const int slot = (id >> 7) & 3;
    const int w = (id >> 9) & 3;
    const int b = id >> 11;
    const int li = slot >> 1;                 // 0: layer 0, 1: layer 4
    const int p = slot & 1;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane < 32) {
        const int f = 128 * w + 64 * p + 32 * i + lane;
        const float* wx = wxyz + ((size_t)li * kHidden + f) * 3;
        const float bb = beta[((size_t)b * 2 + li) * kHidden + f];
        const float hi = Elem<T>::round(bb);
        v[0] = wx[0]; v[1] = wx[1]; v[2] = wx[2];
        v[3] = wx[0]; v[4] = wx[1]; v[5] = wx[2];
        v[6] = hi;    v[7] = bb - hi;
    }
    T* o = aux + (size_t)id * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (T)v[e];
}

struct FArgs {
    const uint8_t* stream;   // [4 waves][nsteps][2 KiB] then bias aux [4 waves][nparts][2 KiB]
    const uint8_t* aux;      // workspace [B][4 waves][4 slots][2 KiB]
    const float* w_last;     // [4 w][2 p][2 i][2 h][16] (pack.permute_w_last_split)
    const float* xyz;
    float* out;
    float b_last;
    int npts, tiles_per_shape, n_tiles;
    int N, k0;
    float vs, origin;
    // bricks mode (appended: the grid / points kernels read the fields above where they were)
    const int32_t* bricks;   // ascending global brick ids, the first *count of them valid
    const int32_t* count;    // device count of active bricks
    int nb, nbt;             // bricks per axis, B * nb^3
    GridDiv gd;              // grid mode: the reciprocals of N (grid_index.h)
};

// Epilogue kinds run inside a 16-step window of a part (on the OTHER accumulator set), every
// step of it hand-ordered (window_step, window_step_fin).  Every element is read out of the
// accumulator file at its use, as an "a" operand of a pair block: as plain values the register
// allocator copied the finished set into VGPRs in one burst at the part's start, with the
// matrix pipe idle (and the set FE_FIN1 folds, carried around the tile loop, at the loop header:
// DESIGN.md §4 "tile prologue").
//   FE_LATE / FE_EARLY: a layer's part 1 / part 0 -> the late / early positions (16-bit, ReLU)
//   FE_FIN0: layer 7 part 0 (set A) -> the final dot product, during layer 7 part 1;
//   FE_FIN1: layer 7 part 1 of the PREVIOUS tile (set B) -> the dot product, during layer 1 part
//            0 of this one; its step 14 publishes the partials (the mid barrier) and the part
//            sums them and stores the previous tile's outputs after that barrier
enum FsEpi { FE_NONE = 0, FE_LATE = 1, FE_EARLY = 2, FE_FIN0 = 3, FE_FIN1 = 4 };

// A fragment source: a buffer resource (SGPRs) + a byte offset (SGPR); the lane's 16 bytes at
// voffset lane*16 (+1024: the second fragment, an immediate).  Raw buffer loads keep every
// address in scalar registers: plain global loads made the compiler materialise (and hoist,
// then spill) a 64-bit VGPR address per load site.
struct FSrc {
    bool shape;               // per-shape aux (workspace) or the weight blob
    uint32_t off;             // byte offset in that buffer
    bool none = false;        // nothing to prefetch (the tile's last part)
};

struct FCtx {
    int lane, wave, h;
    uint32_t voff;            // lane * 16
    char* smem;
    __amdgpu_buffer_rsrc_t rw;   // the weight blob: streams then bias aux fragments
    __amdgpu_buffer_rsrc_t ra;   // the per-shape aux workspace
    uint32_t s_beg, s_end;    // this wave's stream [s_beg, s_end) in rw
    uint32_t s_iss;           // next 4-step stream group to issue
    uint32_t baux_w;          // this wave's bias aux fragments [nparts][2 KiB] in rw
    uint32_t aux_w;           // this tile's per-shape aux of this wave [4 slots][2 KiB] in ra
    uint32_t aux_next;        // ... of the next tile
    u32x4 auxn[2];            // aux A fragments of the part about to start
    u32x4 ring[kFsD][2];
    u32x4 b[4];               // the B fragments of the step about to run (rolling)
    float part[4];            // final-layer partial sums of point chunk n
    const f32x4* wlp;         // FE_FIN0 / FE_FIN1 window: this lane's final-layer weights (wl_at)
    f32x4 wl[2][4];           // ... of m-chunk i, as registers (window_step_fin)
    float* out;               // the previous tile's outputs (FE_FIN1): [shape][npts]
    int npts, prev_shape, prev_local;   // prev_local < 0: no previous tile
    float b_last;
    unsigned long long* st;   // FS_STAMP
    int st_i;
    bool st_on;
    const int32_t* bricks;    // bricks mode: the list, N, bricks per axis, B * nb^3
    int N, nb, nbt;
};

__device__ __forceinline__ void stamp(FCtx& c) {
    if (FS_STAMP) {
        if (c.st_on && c.lane == 0 && c.st_i < 128) c.st[c.st_i] = __builtin_readcyclecounter();
        ++c.st_i;
    }
}

__device__ __forceinline__ u32x4 bld(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

__device__ __forceinline__ void load_aux(FCtx& c, FSrc s) {
    if (s.none) return;
    const __amdgpu_buffer_rsrc_t r = s.shape ? c.ra : c.rw;
    c.auxn[0] = bld(r, c.voff, s.off);
    c.auxn[1] = bld(r, c.voff + 1024u, s.off);
}

// A lane's LDS byte address `voff + off` (off wave-uniform: one v_add).
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ int opaque_s(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

// LDS addressing.  Immediates are 16 bits, so most accesses need a register base past 64 KiB;
// left to itself the compiler materialised one VGPR per constant address, hoisted them out of
// the tile loop and spilled them -- and every spill reload waits vmcnt(0), i.e. for the whole
// weight ring in flight.  So every address is formed AT ITS USE from an opaque copy of voff
// (a volatile asm is neither hoisted nor folded): one or two VALU per use, nothing long-lived
// but voff itself.
__device__ __forceinline__ char* lds_at(const FCtx& c, uint32_t off) {
    return c.smem + (opaque(c.voff) + off);
}
// A group base: the SUM is opaque as well, so that what a group adds to it (< 16 KiB) stays in
// the ds_read / ds_write immediates.  Between asm statements the compiler otherwise folds each
// access's offset into the constant and spends one v_add per access past 64 KiB.
__device__ __forceinline__ char* lds_base(const FCtx& c, uint32_t off) {
    return c.smem + opaque(opaque(c.voff) + off);
}
__device__ __forceinline__ u32x4* act_wb(const FCtx& c, int late) {
    return reinterpret_cast<u32x4*>(lds_base(c, (uint32_t)(late + 4 * c.wave) * 4096u));
}
// this wave's early (0) / late (16) positions: + (2i + s) * 4 KiB + n * 1 KiB immediates
__device__ __forceinline__ u32x4* act_w(const FCtx& c, int late) {
    return reinterpret_cast<u32x4*>(lds_at(c, (uint32_t)(late + 4 * c.wave) * 4096u));
}
// final-layer weights of (this wave, part p, m-chunk i, this lane half)
__device__ __forceinline__ const f32x4* wl_at(const FCtx& c, int p, int i) {
    const uint32_t h = opaque(c.voff) >> 9;           // lane >> 5
    return reinterpret_cast<const f32x4*>(
        c.smem + kFsAct + kFsRed + (((c.wave * 2 + p) * 2 + i) * 2) * 64 + h * 64);
}

// this lane's final partials red[wave][n][lane] (+ n * 64 floats)
__device__ __forceinline__ float* red_w(const FCtx& c) {
    return reinterpret_cast<float*>(c.smem + kFsAct + c.wave * 4 * 64 * 4 + (opaque(c.voff) >> 2));
}

// LDS barrier: LDS writes done (lgkmcnt), then s_barrier.  The weight loads in flight
// (vmcnt) are NOT waited for: they feed registers only.
__device__ __forceinline__ void fs_bar() {
    if (FS_ABL & 4) return;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The activation buffer is kept in CONSUMPTION order: position j (4 KiB: 4 point chunks x
// 1 KiB) holds the k-step that ring step j of the next layer reads (pack.split_kidx): after a
// 512-wide layer, k-step 8w + 4u + 2i + s sits at position 16u + 4w + 2i + s (u = 0: part 0,
// the "early" positions; u = 1: part 1, the "late" ones); after layer 3 at skip 253, k-step
// 4w + 2i + s at position 16 + 4w + 2i + s (layer 4 reads positions 16 + j).  Step j reads
// position pos0 + j: the addresses are immediates from one group base.
__device__ __forceinline__ void read_b(FCtx& c, int pos) {
    const u32x4* p = reinterpret_cast<const u32x4*>(lds_at(c, pos * 4096));
#pragma unroll
    for (int n = 0; n < 4; ++n) c.b[n] = p[n * 64];
}

// Stream step r (0..3) of the 4-step stream group at c.s_iss into ring slot r: the
// (r & 1) * 2 KiB + fragment offset folds into the load's immediate, the (r >> 1) * 4 KiB into
// the scalar offset, so a group costs one wrap test instead of one per step.
__device__ __forceinline__ void issue(FCtx& c, int r) {
    const uint32_t so = c.s_iss + (uint32_t)(r >> 1) * 2u * kFsStep;
    const uint32_t vo = c.voff + (uint32_t)(r & 1) * kFsStep;
    if (FS_ABL & 1) return;
    c.ring[r][0] = bld(c.rw, vo, so);
    c.ring[r][1] = bld(c.rw, vo + 1024u, so);
}

__device__ __forceinline__ uint32_t next_iss(const FCtx& c) {
    const uint32_t n = c.s_iss + 4u * kFsStep;
    return n == c.s_end ? c.s_beg : n;
}
__device__ __forceinline__ void next_group(FCtx& c) { c.s_iss = next_iss(c); }

// ReLU of an fp32 value as ONE integer max: a negative float is a negative int32 (sign bit),
// so max(bits, 0) is +0 for it and the value itself otherwise (fmaxf costs a NaN-quieting
// v_max plus the max under IEEE mode: two instructions per element)
__device__ __forceinline__ float relu_f(float x) {
    return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0));
}

// One element of layer 7 part 1 in the drain after the tile loop, read out of the accumulator
// file AT ITS USE: an EMPTY asm statement with the element as an "a" operand pins it there up to
// this point, as the pair blocks' operands do inside the loop (the set is carried around the
// tile loop; one pin of the whole set instead made the allocator shuffle 64 registers through
// v_accvgpr_mov / _write).
__device__ __forceinline__ float acc_read(float a) {
    asm volatile("" : "+a"(a));
    return a;
}

// One FE_FIN1 unit u = 2t + s outside a window (the drain of the workgroup's last tile): HALF
// of tile t = 4i + n (its accumulator registers 8s..8s+7) folded into c.part[n].  The elements,
// their order and the chain per n are window_step_fin's.
__device__ __forceinline__ void fin1_unit(FCtx& c, const f32x16 (&accY)[2][4], int u) {
    const int t = u >> 1, s = u & 1;
    const int i = t >> 2, n = t & 3;
    const f32x4* w = wl_at(c, 1, i);
    float part = c.part[n];
#pragma unroll
    for (int q = 2 * s; q < 2 * s + 2; ++q) {
        const f32x4 wv = w[q];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            part = fmaf(relu_f(acc_read(accY[i][n][4 * q + e])), wv[e], part);
    }
    c.part[n] = part;
}

// MFMA pair of point chunk n of one step (both m-chunks of the wave's part)
template <typename T>
__device__ __forceinline__ void mfma_pair(f32x16 (&acc)[2][4], const u32x4& a0, const u32x4& a1,
                                          const u32x4& b, int n) {
    acc[0][n] = Elem<T>::mfma(a0, b, acc[0][n]);
    acc[1][n] = Elem<T>::mfma(a1, b, acc[1][n]);
}

// Step k < 15 of an FE_LATE / FE_EARLY window, hand-ordered: the step's four MFMA pairs as pair
// blocks (decoder_common.h) that carry unit k's conversion -- elements 8s + 2n, 8s + 2n + 1 of
// its half tile behind pair n -- with the memory operations between them, each held in its MFMA
// gap by a sched_barrier: chunk n's next B read behind pair n, the step's two weight loads and
// the unit's write behind the last.  Per gap: 2 VALU | 2 VALU + the read; the last pair 4 VALU |
// none, so the step's tail holds 4 instructions (read, two loads, write).  Step 14 carries units
// 14 and 15 = the 16 elements of tile (1, 3): pair p converts elements 4p .. 4p + 3 (4 | 4 VALU,
// 6 | 2 in the last), so unit 14's fragment is written behind pair 1 already.
// `nb`: the next position's B fragments (group4's base + immediates).
template <typename T>
__device__ __forceinline__ void window_step(FCtx& c, f32x16 (&acc)[2][4],
                                            const f32x16 (&accY)[2][4], const u32x4& a0,
                                            const u32x4& a1, const u32x4* nb, int k, int r,
                                            u32x4* wbase) {
    // the group's last step: the next group's ring offset (next_group) behind the first pair
    uint32_t nxt = 0;
    if (k < 14) {
        const int t = k >> 1, s = k & 1;
        const int i = t >> 2, nn = t & 3;
        u32x4 f;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            unsigned w;
            if (r == 3 && n == 1) nxt = next_iss(c);
            const float e0 = accY[i][nn][8 * s + 2 * n], e1 = accY[i][nn][8 * s + 2 * n + 1];
            if (n < 3)
                Elem<T>::template pair_cvt1<false>(acc[0][n], acc[1][n], a0, a1, c.b[n], e0, e1,
                                                   w);
            else
                Elem<T>::template pair_cvt1<true>(acc[0][n], acc[1][n], a0, a1, c.b[n], e0, e1,
                                                  w);
            f[n] = w;
            c.b[n] = nb[n * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
        issue(c, r);
        wbase[((2 * i + s) * 4 + nn) * 64] = f;
        if (r == 3) c.s_iss = nxt;
    } else {
        u32x4 f[2];
        const f32x16& y = accY[1][3];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            unsigned w0, w1;
            if (p < 3)
                Elem<T>::template pair_cvt2<false>(acc[0][p], acc[1][p], a0, a1, c.b[p], y[4 * p],
                                                   y[4 * p + 1], y[4 * p + 2], y[4 * p + 3], w0,
                                                   w1);
            else
                Elem<T>::template pair_cvt2<true>(acc[0][p], acc[1][p], a0, a1, c.b[p], y[4 * p],
                                                  y[4 * p + 1], y[4 * p + 2], y[4 * p + 3], w0,
                                                  w1);
            f[p >> 1][2 * (p & 1)] = w0;
            f[p >> 1][2 * (p & 1) + 1] = w1;
            c.b[p] = nb[p * 64];
            if (p == 1) wbase[(2 * 4 + 3) * 64] = f[0];
            __builtin_amdgcn_sched_barrier(0);
        }
        issue(c, r);
        wbase[(3 * 4 + 3) * 64] = f[1];
    }
    __builtin_amdgcn_sched_barrier(0);
}

// Step k < 15 of an FE_FIN0 (P = 0) / FE_FIN1 (P = 1) window, hand-ordered like window_step:
// pair n folds elements 8s + 2n, 8s + 2n + 1 of unit k < 14 into c.part (fin1_unit's elements,
// order and chain).  Three VALU an element leave no room for a double-unit step, so the 16
// elements y of tile (1, 3) -- units 14 and 15, the end of chain 3, whose earlier units are 6 and
// 7 -- ride behind the first two pairs of steps 8-13, one each (y[2 (k - 8) + n], pair_fin3), and
// of step 14, two each; chain 3 keeps its order, and the other chains never meet it.
// The final-layer weights of an m-chunk (4 x 16 bytes a lane) are read once per window instead
// of 32 bytes per step: chunk 0's ahead of the window's first block, chunk 1's one fragment
// behind each pair of step 6.  The ring's wrap test of a group's last step stands behind pair 2
// here (pairs 0-1 carry the extra element in steps 8-13).
template <typename T, int P>
__device__ __forceinline__ void window_step_fin(FCtx& c, f32x16 (&acc)[2][4],
                                                const f32x16 (&accY)[2][4], const u32x4& a0,
                                                const u32x4& a1, const u32x4* nb, int k, int r) {
    const int t = k >> 1, s = k & 1;
    const int i = t >> 2, nn = t & 3;
    const f32x16& y = accY[1][3];
    uint32_t nxt = 0;
    if (k == 0) {
        c.wlp = wl_at(c, P, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) c.wl[0][q] = c.wlp[q];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (k < 14) {
            const int e = 8 * s + 2 * n;
            const float e0 = accY[i][nn][e], e1 = accY[i][nn][e + 1];
            const float w0 = c.wl[i][e >> 2][e & 3], w1 = c.wl[i][e >> 2][(e & 3) + 1];
            const int x = 2 * (k - 8) + n;
            if (k >= 8 && n < 2)
                Elem<T>::pair_fin3(acc[0][n], acc[1][n], a0, a1, c.b[n], e0, e1, w0, w1,
                                   c.part[nn], y[x], c.wl[1][x >> 2][x & 3], c.part[3]);
            else if (n < 3)
                Elem<T>::template pair_fin<false>(acc[0][n], acc[1][n], a0, a1, c.b[n], e0, e1,
                                                  w0, w1, c.part[nn]);
            else
                Elem<T>::template pair_fin<true>(acc[0][n], acc[1][n], a0, a1, c.b[n], e0, e1,
                                                 w0, w1, c.part[nn]);
        } else if (n < 2) {
            const int x = 12 + 2 * n;
            Elem<T>::template pair_fin<false>(acc[0][n], acc[1][n], a0, a1, c.b[n], y[x],
                                              y[x + 1], c.wl[1][3][x & 3],
                                              c.wl[1][3][(x & 3) + 1],
                                              c.part[3]);
        } else {
            mfma_pair<T>(acc, a0, a1, c.b[n], n);
        }
        if (r == 3 && n == 2) nxt = next_iss(c);
        c.b[n] = nb[n * 64];
        if (k == 6) c.wl[1][n] = c.wlp[8 + n];    // m-chunk 1: + 128 bytes
        if (k == 14 && n == 2) {
            if (P == 0) {
                // the partial sums are next used in the next tile: fixed HERE, as they were
                // when the chain was compiled code (otherwise sunk below the part's plain steps)
#pragma unroll
                for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(c.part[m]));
            } else {                        // the partials -> red[wave][n][lane], published by
                float* rw = red_w(c);       // the barrier inside step 15
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    rw[m * 64] = c.part[m];
                    c.part[m] = 0.f;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    issue(c, r);
    if (r == 3) c.s_iss = nxt;
    __builtin_amdgcn_sched_barrier(0);
}

// the final layer across waves and lane halves (lanes l and l^32 hold the same point): lanes
// < 32 of wave w sum point chunk w's 8 partials (after the barrier that published them), add
// the bias, tanh, store
__device__ __forceinline__ void fin_store(const FCtx& c, int shape, int local) {
    const int lane = (int)(opaque(c.voff) >> 4);     // formed here: nothing kept live (spills)
    if (local < 0 || lane >= 32) return;
    const float* rr = reinterpret_cast<const float*>(
        c.smem + kFsAct + c.wave * 64 * 4 + (opaque(c.voff) >> 2));
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += rr[w * 4 * 64] + rr[w * 4 * 64 + 32];
    const int pt = local * kTilePoints + 32 * c.wave + lane;
    if (pt < c.npts) {
        // a buffer store off the shape's row (scalar base, 32-bit lane offset): a 64-bit VGPR
        // address here was kept live across the tile loop and spilled
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(c.out + (size_t)shape * c.npts), (short)0, 0x7ffffff0, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, tanhf(s + c.b_last)),
                                              ro, (uint32_t)pt * 4u, 0, 2 /* nt */);
    }
}

// Entry i of the brick list through the constant address space: a scalar load (the index is
// wave-uniform), which neither takes a VGPR nor joins the weight ring's vmcnt queue.  As a plain
// global load it is a vector load once the loop holds stores.  The list is written by an earlier
// launch and never during this one.
__device__ __forceinline__ int list_at(const int32_t* list, int i) {
    typedef const __attribute__((address_space(4))) int32_t* const_i32;
    return ((const_i32)(uintptr_t)list)[i];
}

// A global brick id as (shape, first voxel per axis). nb through an opaque SGPR: the divisions'
// reciprocals are formed at the use instead of hoisted out of the tile loop (and spilled).
__device__ __forceinline__ void brick_origin(int gid, int nb_, int& shape, int& i0, int& j0,
                                             int& k0) {
    const int nb = opaque_s(nb_);
    const int nb2 = nb * nb, nb3 = nb2 * nb;
    shape = gid / nb3;
    const int id = gid - shape * nb3;
    const int bz = id / nb2, r = id - bz * nb2;
    const int by = r / nb;
    i0 = 8 * (r - by * nb);
    j0 = 8 * by;
    k0 = 8 * bz;
}

// Bricks mode: `tile` is quarter tile & 3 of brick list[tile >> 2]; wave w's lane < 32 holds the
// brick-local point 128 (tile & 3) + 32 w + lane (dx = idx & 7, dy = idx >> 3 & 7, dz = idx >> 6).
// The voxel is re-derived here from the tile index alone (one scalar load of the list entry):
// nothing about the previous tile is kept live across the tile loop (spills, see lds_at).  The
// partial sums are added in fin_store's order (a point's value must not depend on the mode).
// One float at (k N + j) N + i of the shape's volume: the z-slice (wave-uniform) goes into the
// buffer base, so the lane offset (j N + i) * 4 stays inside the resource's 2 GiB range at any
// N the brick count admits.
__device__ __forceinline__ void fin_store_bricks(const FCtx& c, int tile) {
    const int lane = (int)(opaque(c.voff) >> 4);
    if (tile < 0 || lane >= 32) return;
    const float* rr = reinterpret_cast<const float*>(
        c.smem + kFsAct + c.wave * 64 * 4 + (opaque(c.voff) >> 2));
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += rr[w * 4 * 64] + rr[w * 4 * 64 + 32];
    const int gid = list_at(c.bricks, tile >> 2);
    LDM_DASSERT(gid >= 0 && gid < c.nbt);
    int shape, i0, j0, k0;
    brick_origin(gid, c.nb, shape, i0, j0, k0);
    const int idx = 128 * (tile & 3) + 32 * c.wave + lane;
    const int i = i0 + (idx & 7), j = j0 + ((idx >> 3) & 7);
    const int k = k0 + 2 * (tile & 3) + (c.wave >> 1);             // idx >> 6
    const int N = c.N;
    if ((unsigned)gid < (unsigned)c.nbt && i < N && j < N && k < N) {
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(c.out + ((size_t)shape * N + k) * N * N), (short)0, 0x7ffffff0, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, tanhf(s + c.b_last)),
                                              ro, (uint32_t)(j * N + i) * 4u, 0, 2 /* nt */);
    }
}

template <int MODE>
__device__ __forceinline__ void fin_store_mode(const FCtx& c) {
    if (MODE == kModeBricks) fin_store_bricks(c, c.prev_local);   // prev_local: the tile index
    else fin_store(c, c.prev_shape, c.prev_local);
}

// Four k-steps reading positions p0..p0+3 (ring slots 0..3), epilogue window steps K0..K0+3.
// Rolling B fragments: chunk n of step j+1 is read as soon as step j's two MFMAs on chunk n are
// issued (~6 MFMAs, ~190 cycles, before it is needed).  BAR = r: an LDS barrier INSIDE step r,
// after its first MFMA pair and before its first read of the next position:
// the waves wait on each other with the step's remaining MFMAs still to issue and the next
// position's reads still covered by them (a barrier between steps exposed one LDS round trip
// plus the pipeline drain, ~500-750 cycles per barrier).
// Steps 0-14 of a window (EK != FE_NONE) are hand-ordered (window_step, window_step_fin); its
// step 15 carries no unit and runs, like a plain group's steps, as compiled code whose order the
// sched_group_barriers pin.  A window's groups get their bases from steps16e (WIN: `gb` for the
// reads, `wb` for the units' writes), a plain group forms its read base here.
// `go` (steps_plain's rolled loop): the group's read base as an LDS offset carried from group to
// group, one position BELOW the group's first read.  It is advanced by a group in the first gap
// of the group's last step, whose own reads then take it with immediates from 0 (so the old
// value is dead and the add is in place), and the ring's wrap test stands in that gap as well:
// behind the group's last MFMA only that step's B read, its two weight loads and the loop's own
// add / compare / branch remain.
template <typename T, int EK, int K0, int BAR, bool WIN = false>
__device__ __forceinline__ void group4(FCtx& c, f32x16 (&acc)[2][4], const f32x16 (&accY)[2][4],
                                       int p0, const char* gb = nullptr, u32x4* wb = nullptr,
                                       uint32_t* go = nullptr) {
    static_assert(WIN || EK == FE_NONE, "windows run through steps16e");
    constexpr int BP = 1;                    // MFMA pairs before the in-stream barrier
    const bool carry = go != nullptr;        // (a constant once inlined: &local or nullptr)
    // ONE LDS base for the group's four next positions (r * 4 KiB + n * 1 KiB fold into the
    // ds_read immediates) instead of an address formed per step
    const char* gbase = WIN ? gb : carry ? c.smem + *go + 4096 : lds_base(c, (p0 + 1) * 4096);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool last = carry && r == 3;
        uint32_t nxt = 0;
        if (last) {
            nxt = next_iss(c);
            *go = opaque(*go + 4u * 4096u);
        }
        const u32x4* nb =
            reinterpret_cast<const u32x4*>(last ? c.smem + *go : gbase + r * 4096);
        const u32x4 a0 = c.ring[r][0], a1 = c.ring[r][1];
        const int k = K0 + r;
        if (r == BAR) {
#pragma unroll
            for (int n = 0; n < BP; ++n) mfma_pair<T>(acc, a0, a1, c.b[n], n);
            for (int n = 0; n < BP; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            fs_bar();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < BP; ++n) c.b[n] = nb[n * 64];
#pragma unroll
            for (int n = BP; n < 4; ++n) {
                mfma_pair<T>(acc, a0, a1, c.b[n], n);
                c.b[n] = nb[n * 64];
            }
            issue(c, r);
            for (int n = 0; n < BP; ++n) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            for (int n = BP; n < 4; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        } else if ((EK == FE_LATE || EK == FE_EARLY) && k < 15 && !(FS_ABL & 2)) {
            window_step<T>(c, acc, accY, a0, a1, nb, k, r, wb);
            if (r == 3) return;      // the ring's wrap test went into the step (window_step)
            continue;
        } else if ((EK == FE_FIN0 || EK == FE_FIN1) && k < 15 && !(FS_ABL & 2)) {
            window_step_fin<T, EK == FE_FIN1>(c, acc, accY, a0, a1, nb, k, r);
            if (r == 3) return;
            continue;
        } else {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                mfma_pair<T>(acc, a0, a1, c.b[n], n);
                c.b[n] = nb[n * 64];
            }
            issue(c, r);
            if (last) c.s_iss = nxt;
            // pin the step's order for the scheduler (left free it sank the B reads and weight
            // loads below the last MFMA): per point chunk n, 2 MFMAs, B read; then the 2 weight
            // loads
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                if (last && n == 0) {
                    __builtin_amdgcn_sched_group_barrier(0x004, 3, 0);    // add, compare, select
                    __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);    // the next base
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (!carry) next_group(c);
}

// 16 k-steps from position p0 carrying the 16 epilogue units of the other set; BAR: the
// window's closing barrier inside its step 15
template <typename T, int EK, bool BAR>
__device__ __forceinline__ void steps16e(FCtx& c, f32x16 (&acc)[2][4],
                                         const f32x16 (&accY)[2][4], int p0) {
    // one base each for the window's 16 next positions (the last immediate is 15 * 4 KiB + 3 KiB
    // < 64 KiB) and its 16 writes: formed per group they stood, with the ring's wrap test, in the
    // gap behind the group's last MFMA, beside that step's B read, weight loads and write
    const char* gb = lds_base(c, (p0 + 1) * 4096);
    u32x4* wb = EK == FE_LATE ? act_wb(c, 16) : EK == FE_EARLY ? act_wb(c, 0) : nullptr;
    group4<T, EK, 0, -1, true>(c, acc, accY, p0, gb, wb);
    group4<T, EK, 4, -1, true>(c, acc, accY, p0 + 4, gb + 4 * 4096, wb);
    group4<T, EK, 8, -1, true>(c, acc, accY, p0 + 8, gb + 8 * 4096, wb);
    group4<T, EK, 12, BAR ? 3 : -1, true>(c, acc, accY, p0 + 12, gb + 12 * 4096, wb);
}

// plain k-steps [j0, j1) from position pos0 as ONE runtime loop of 4-step groups (code size:
// the kernel must stay well inside the instruction cache)
template <typename T>
__device__ __forceinline__ void steps_plain(FCtx& c, f32x16 (&acc)[2][4],
                                            const f32x16 (&accY)[2][4], int pos0, int j0, int j1) {
    if (j0 >= j1) return;
    uint32_t go = opaque(opaque(c.voff) + (uint32_t)(pos0 + j0) * 4096u);
#pragma unroll 1
    for (int j = j0; j < j1; j += 4)
        group4<T, FE_NONE, 0, -1>(c, acc, accY, pos0 + j, nullptr, nullptr, &go);
}

// One part: the aux step, then nk ring steps reading positions pos0 .. pos0 + nk - 1 = 31
// (the last one reads position 32, the tile's aux B fragments, for the next part's aux step).
//   * aux step: zero-initialises acc with [wx,wy,wz,wx,wy,wz,b_hi,b_lo] x xyz (c.b on entry)
//     and, per point chunk, reads the first position's B fragment behind its MFMA pair -- or,
//     `bar0`, after a barrier (the part follows serial LDS writes: layers 1 and 4 at skip 253);
//     then it loads the NEXT part's aux A fragments (naux).
//   * E work (the other set, EK) in steps 0-15 (E16 false) or, E16 (FE_EARLY of a 32-step
//     part), in steps 16-31.
//   * `mid`: the barrier inside step 15 (the late positions written during steps 0-14 by
//     every wave / no wave reads the early positions any more before E16 writes them);
//     `endbar` (E work parts): the barrier inside the part's last step, publishing the window's
//     writes to the next part, whose aux step then reads on without a barrier.
template <typename T, int EK, bool E16, int MODE = kModeGrid>
__device__ __forceinline__ void run_part(FCtx& c, f32x16 (&acc)[2][4], const f32x16 (&accY)[2][4],
                                         int nk, bool mid, bool endbar, FSrc naux, int pos0,
                                         bool bar0) {
    const f32x16 zero = {};
    const u32x4 a0 = c.auxn[0], a1 = c.auxn[1];
    if (bar0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            acc[0][n] = Elem<T>::mfma(a0, c.b[n], zero);
            acc[1][n] = Elem<T>::mfma(a1, c.b[n], zero);
        }
        load_aux(c, naux);
        fs_bar();
        read_b(c, pos0);
    } else {
        const u32x4* p = reinterpret_cast<const u32x4*>(lds_at(c, pos0 * 4096));
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            acc[0][n] = Elem<T>::mfma(a0, c.b[n], zero);
            acc[1][n] = Elem<T>::mfma(a1, c.b[n], zero);
            c.b[n] = p[n * 64];
        }
        load_aux(c, naux);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (EK == FE_NONE) {
        // A part without E work (layer 4 part 0 at skip 253) starts with BOTH sets dead: the
        // other one was converted during the previous part, this one written out serially.
        // Everywhere else the other set is live across the aux step, so the new accumulators
        // can only take the registers of the set they replace; here they could take either
        // half of the file, and when they took the other set's the two sets had traded places
        // by the end of the tile and were moved back (v_accvgpr_mov, spills).  An empty asm
        // statement that names the dead set keeps its registers occupied across this aux step.
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int n = 0; n < 4; ++n) asm volatile("" ::"a"(accY[i][n]));
    }
    stamp(c);
    if (!E16 && EK != FE_NONE) {        // E work in steps 0-15
        // the barrier inside step 15: mid (nk 32), or the end barrier of a 16-step part
        if (mid || (endbar && nk == 16)) steps16e<T, EK, true>(c, acc, accY, pos0);
        else steps16e<T, EK, false>(c, acc, accY, pos0);
        if (EK == FE_FIN1) {
            stamp(c);
            fin_store_mode<MODE>(c);
        }
        stamp(c);
        if (endbar && nk == 32) {       // the end barrier inside step 31
            steps_plain<T>(c, acc, accY, pos0, 16, 28);
            group4<T, FE_NONE, 0, 3>(c, acc, accY, pos0 + 28);
        } else {
            steps_plain<T>(c, acc, accY, pos0, 16, nk);
        }
    } else if (E16) {                   // nk 32, mid: the window in steps 16-31
        static_assert(!E16 || EK == FE_EARLY, "E16 parts convert part 0 of their own layer");
        steps_plain<T>(c, acc, accY, pos0, 0, 12);
        group4<T, FE_NONE, 0, 3>(c, acc, accY, pos0 + 12);
        stamp(c);
        if (endbar) steps16e<T, EK, true>(c, acc, accY, pos0 + 16);
        else steps16e<T, EK, false>(c, acc, accY, pos0 + 16);
    } else {                            // plain part, no barrier (layer 4 part 0 at skip 253)
        steps_plain<T>(c, acc, accY, pos0, 0, nk < 16 ? nk : 16);
        stamp(c);
        steps_plain<T>(c, acc, accY, pos0, 16, nk);
    }
    stamp(c);
}

// a whole set into this wave's late positions 16 + 4w + 2i + s (serial: layer 3 at skip 253);
// the per-wave base and immediates per tile
template <typename T>
__device__ __forceinline__ void acc_to_lds(FCtx& c, const f32x16 (&acc)[2][4]) {
    u32x4* p = act_w(c, 16);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            u32x4 f0, f1;
            acc_to_frags<T>(acc[i][n], f0, f1);
            p[(2 * i * 4 + n) * 64] = f0;
            p[((2 * i + 1) * 4 + n) * 64] = f1;
        }
}

// One part of layer 0: a single K = 16 step per tile, [wx,wy,wz,wx,wy,wz,b_hi,b_lo] x the xyz
// fragments in c.b (which stay), straight from the matrix pipe to this wave's early (LATE =
// false) or late positions.  The 8 products (m-chunk i, point chunk n) go through two VGPR
// temporaries (Elem::mfma_v) instead of an accumulator set: nothing is read back from AGPRs,
// and set B keeps the previous tile's layer 7 part 1 untouched.  Then the next part's aux A
// fragments (naux) are loaded.
// Wait states (mfma_v: the compiler pads nothing around an asm statement).  A 32x32x16 product is
// an 8-pass XDL op; its D may be read by a VALU 12 issue slots after it (the CDNA3/4 ISA's table
// of required software wait states, row "XDL write VGPR -> VALU read/write, VMEM/LDS/FLAT read:
// 8 passes: 11", one more as the guide's margin).  Product q+1 is issued BEFORE product q is
// converted, and the scheduling barriers pin that order:
//     P0 P1 nop | cvt 0 | P2 | cvt 1 | P3 | ... | P7 | cvt 6 | cvt 7
// so between P(q) and its first reader stand P(q+1) and, for q >= 1, the whole of cvt q-1 (8
// v_cvt_pk, 8 v_pk_max, 2 ds_write); only P0 needs nops (P1 + s_nop 10 = 12 slots).  The
// operands of a product are loaded fragments, complete long before (VALU write -> MFMA read
// needs 2 slots); tests/test_decoder_codegen.py counts both distances in the assembly.
template <typename T, bool LATE>
__device__ __forceinline__ void layer0_part(FCtx& c, FSrc naux) {
    const u32x4 a[2] = {c.auxn[0], c.auxn[1]};
    u32x4* p = act_w(c, LATE ? 16 : 0);
    f32x16 t[2];
    t[0] = Elem<T>::mfma_v(a[0], c.b[0]);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int i = q & 1, n = q >> 1;
        if (q < 7) t[(q + 1) & 1] = Elem<T>::mfma_v(a[(q + 1) & 1], c.b[(q + 1) >> 1]);
        if (q == 0) {
            asm volatile("s_nop 10" : "+v"(t[0]));
            load_aux(c, naux);
            stamp(c);
        }
        __builtin_amdgcn_sched_barrier(0);
        u32x4 f0, f1;
        acc_to_frags<T>(t[q & 1], f0, f1);
        p[(2 * i * 4 + n) * 64] = f0;
        p[((2 * i + 1) * 4 + n) * 64] = f1;
        __builtin_amdgcn_sched_barrier(0);
    }
    stamp(c);
}

// MODE (decoder_common.h): where a tile's points come from and its outputs go -- a run of 128
// grid voxels, 128 listed points, or a quarter of a listed 8^3 brick of the dense grid.
template <typename T, int S, int MODE>
__global__ __launch_bounds__(256, 1) void dec_fs_kernel(FArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kFsLds];
    FCtx c;
    c.lane = threadIdx.x & 63;
    c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.h = c.lane >> 5;
    c.voff = (uint32_t)c.lane * 16u;
    c.smem = smem;
    c.out = a.out;
    c.npts = a.npts;
    c.b_last = a.b_last;
    c.prev_shape = 0;
    c.prev_local = -1;
    c.st = reinterpret_cast<unsigned long long*>(smem + kFsAct + kFsRed + kFsWl);
    c.st_i = 0;
    c.st_on = false;
    float* wl = reinterpret_cast<float*>(smem + kFsAct + kFsRed);

    for (int i = threadIdx.x; i < 512; i += 256) wl[i] = a.w_last[i];
    __syncthreads();
    // bricks mode: 4 tiles per active brick, the device count read once, here (clamped to the
    // list's capacity: the walk below never reads past the caller's list); 0 is a valid launch
    const int n_tiles = MODE == kModeBricks ? 4 * min(max(a.count[0], 0), a.nbt) : a.n_tiles;
    if (MODE == kModeBricks) {
        c.bricks = a.bricks;
        c.N = a.N;
        c.nb = a.nb;
        c.nbt = a.nbt;
    }
    if ((int)blockIdx.x >= n_tiles) return;

    constexpr int NST = fs_nsteps(S);
    constexpr int NP = fs_nparts(S);
    constexpr uint32_t kFlags = 0x00020000u;     // raw dword buffer (gfx9 word 3)
    c.rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.stream, (short)0, 0x7ffffff0, kFlags);
    c.ra = __builtin_amdgcn_make_buffer_rsrc((void*)a.aux, (short)0, 0x7ffffff0, kFlags);
    c.s_beg = (uint32_t)c.wave * NST * kFsStep;
    c.s_end = c.s_beg + NST * kFsStep;
    c.s_iss = c.s_beg;
    c.baux_w = (uint32_t)(4 * NST + c.wave * NP) * kFsStep;
    // the list entry of `tile`'s brick, clamped into [0, B nb^3): coordinates and the per-shape
    // aux address stay in range whatever the list holds (fin_store_bricks drops such an entry)
    auto brick_of = [&](int tile) -> int {
        return min(max(list_at(a.bricks, tile >> 2), 0), a.nbt - 1);
    };
    auto shape_aux = [&](int tile) -> uint32_t {
        if (MODE == kModeBricks) {
            const int nb = opaque_s(a.nb);
            return ((uint32_t)(brick_of(tile) / (nb * nb * nb)) * 4u + (uint32_t)c.wave) * 4u *
                   kFsStep;
        }
        return ((uint32_t)(tile / a.tiles_per_shape) * 4u + (uint32_t)c.wave) * 4u * kFsStep;
    };
    auto bias = [&](int pi) -> FSrc { return FSrc{false, c.baux_w + (uint32_t)pi * kFsStep}; };
    auto shp = [&](int slot) -> FSrc { return FSrc{true, c.aux_w + (uint32_t)slot * kFsStep}; };
    c.aux_w = shape_aux(blockIdx.x);
#pragma unroll
    for (int r = 0; r < kFsD; ++r) issue(c, r);
    next_group(c);

    f32x16 accA[2][4], accB[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 4; ++n) accB[i][n] = f32x16{};    // the first tile's FE_FIN1 input
#pragma unroll
    for (int n = 0; n < 4; ++n) c.part[n] = 0.f;
#pragma unroll 1
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int shape, local, bi0 = 0, bj0 = 0, bk0 = 0;
        if (MODE == kModeBricks) {
            brick_origin(brick_of(tile), a.nb, shape, bi0, bj0, bk0);
            local = tile;               // what fin_store_bricks re-derives the voxels from
        } else {
            shape = tile / a.tiles_per_shape;
            local = tile - shape * a.tiles_per_shape;
        }
        {
            const int nt = tile + (int)gridDim.x;
            c.aux_next = nt < n_tiles ? shape_aux(nt) : c.aux_w;
        }
        c.st_on = FS_STAMP && c.wave == 0 && tile == (int)blockIdx.x + (int)gridDim.x;
        c.st_i = 0;
        stamp(c);
        load_aux(c, shp(0));            // L0p0's aux fragments (latency under the xyz setup)
        // ---- aux B fragments [x_hi,y_hi,z_hi,x_lo,y_lo,z_lo,1,1] of point 32n + (lane&31) at
        // position 32.  Every wave writes the same bytes (no barrier: a wave reads back its own
        // writes, the others only ever replace them with equal values; every read of the
        // previous tile's position 32 came before its final barrier)
        // lane values formed here from an opaque voff (kept live across the tile loop, they
        // were spilled and reloaded behind the whole weight ring)
        const uint32_t lv = opaque(c.voff);
        const bool hi = lv >= 512u;                       // lane >= 32
        // grid mode: the tile's first voxel, once and on the scalar unit (grid_index.h; the
        // reciprocals of N are kernel arguments: SGPRs, nothing per lane).  The per-lane
        // divisions this replaces were 8 v_rcp_iflag sequences, ~290 VALU, a tile.
        const uint32_t p0 = (uint32_t)local * kTilePoints;
        uint32_t ti = 0, tj = 0, tk = 0;
        if (MODE == kModeGrid) {
            grid_first(p0, (uint32_t)a.N, a.gd, ti, tj, tk);
            tk += (uint32_t)a.k0;
        }
        // points mode: the shape's row of the list as a scalar pointer.  Folded into the lanes'
        // 64-bit address (shape * npts + pt as one vector mad), npts took a VGPR that was hoisted
        // out of the tile loop and spilled; its reload here waited vmcnt(0), the whole weight ring
        const float* row = nullptr;
        if (MODE == kModePoints) {
            row = a.xyz + (size_t)shape * a.npts * 3;
            asm volatile("" : "+s"(row));
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            int pt = local * kTilePoints + 32 * n + (int)((lv >> 4) & 31u);
            if (pt >= a.npts) pt = a.npts - 1;
            float x, y, z;
            if (MODE == kModeBricks) {
                // voxel indices clamped to N - 1, as the ragged tail's points are
                const int idx = 128 * (tile & 3) + 32 * n + (int)((lv >> 4) & 31u);
                const int m = a.N - 1;
                x = grid_axis(min(bi0 + (idx & 7), m), a.vs, a.origin);
                y = grid_axis(min(bj0 + ((idx >> 3) & 7), m), a.vs, a.origin);
                z = grid_axis(min(bk0 + (idx >> 6), m), a.vs, a.origin);
            } else if (MODE == kModePoints) {
                const float* qq = row + (size_t)pt * 3;
                x = qq[0];
                y = qq[1];
                z = qq[2];
            } else {
                // the lane's voxel from the tile's first one: its offset (clamped to the slab's
                // last point in the ragged tail: the point min(pt, npts - 1) above) and two
                // carries, each a multiply-high by the reciprocal of N
                const uint32_t off =
                    grid_tail_off(p0, 32u * n + ((lv >> 4) & 31u), (uint32_t)a.npts);
                uint32_t vi, vj, vk;
                grid_voxel(ti, tj, tk, off, (uint32_t)a.N, a.gd.m, vi, vj, vk);
                x = grid_axis((int)vi, a.vs, a.origin);
                y = grid_axis((int)vj, a.vs, a.origin);
                z = grid_axis((int)vk, a.vs, a.origin);
            }
            const float xh = Elem<T>::round(x), yh = Elem<T>::round(y), zh = Elem<T>::round(z);
            u32x4 f;
            f[0] = hi ? 0u : Elem<T>::pack(xh, yh);
            f[1] = hi ? 0u : Elem<T>::pack(zh, x - xh);
            f[2] = hi ? 0u : Elem<T>::pack(y - yh, z - zh);
            f[3] = hi ? 0u : Elem<T>::pack(1.f, 1.f);
            reinterpret_cast<u32x4*>(lds_at(c, 32u * 4096u))[n * 64] = f;
        }
        read_b(c, 32);

        // ---- layer 0 (aux only), both parts through VGPR temporaries into LDS serially (set B
        // still holds the previous tile's layer 7 part 1, folded into the output during L1p0);
        // the previous tile's readers all passed the end barrier of its layer 7
        layer0_part<T, false>(c, shp(1));
        layer0_part<T, true>(c, bias(2));

        // ---- two-part layers 1, 2 (and 3 when 512 wide).  L1p0 folds the previous tile's
        // layer 7 part 1 into its outputs (FE_FIN1); p1 of layer l publishes with its end barrier.
        // Every window reads its set in place, through the "a" operands of its pair blocks: no
        // instance shuffles accumulators for it (tests/test_decoder_window_codegen.py), the
        // windows of layer 2 (and 3) part 0 at skip 253 and of layer 1 part 1 included, where
        // pins on compiled conversions once cost 368 and 160 v_accvgpr_mov / _write.
        int pi = 2;
        run_part<T, FE_FIN1, false, MODE>(c, accA, accB, 32, true, false, bias(pi + 1), 0, true);
        run_part<T, FE_EARLY, true>(c, accB, accA, 32, true, true, bias(pi + 2), 0, false);
        pi += 2;
        constexpr int L2P = S == 256 ? 3 : 4;
#pragma unroll 1
        for (int l = 2; l < L2P; ++l, pi += 2) {
            // the part after layer 3 (512 wide) is layer 4's: per-shape aux
            const FSrc nx = (S == 512 && l == 3) ? shp(2) : bias(pi + 2);
            run_part<T, FE_LATE, false>(c, accA, accB, 32, true, false, bias(pi + 1), 0,
                                                false);
            run_part<T, FE_EARLY, true>(c, accB, accA, 32, true, true, nx, 0, false);
        }
        if (S == 256) {
            // layer 3: one part of rows 64w..64w+63 -> positions 16 + 4w + 2i + s (serial,
            // once every wave is done reading layer 3's inputs)
            run_part<T, FE_LATE, false>(c, accA, accB, 32, true, false, shp(2), 0,
                                                false);
            fs_bar();
            acc_to_lds<T>(c, accA);
            stamp(c);
            // layer 4 (K = 256, positions 16..31); part 0 -> early positions during part 1
            run_part<T, FE_NONE, false>(c, accA, accB, 16, false, false, shp(3), 16, true);
            run_part<T, FE_EARLY, false>(c, accB, accA, 16, false, true, bias(pi + 3),
                                                  16, false);
            pi += 3;
        } else {
            run_part<T, FE_LATE, false>(c, accA, accB, 32, true, false, shp(3), 0,
                                                false);
            run_part<T, FE_EARLY, true>(c, accB, accA, 32, true, true, bias(pi + 2), 0,
                                                 false);
            pi += 2;
        }
        // ---- layers 5, 6
#pragma unroll 1
        for (int l = 5; l < 7; ++l, pi += 2) {
            run_part<T, FE_LATE, false>(c, accA, accB, 32, true, false, bias(pi + 1), 0,
                                                 false);
            run_part<T, FE_EARLY, true>(c, accB, accA, 32, true, true, bias(pi + 2), 0,
                                                 false);
        }
        // ---- layer 7: part 0 folds into the dot product during part 1, part 1 during the
        // next tile's L1p0 (its end barrier lets the next tile overwrite every position)
        run_part<T, FE_LATE, false>(c, accA, accB, 32, true, false, bias(pi + 1), 0,
                                             false);
        // (no prefetch of the next tile's first aux fragments here: live across the whole
        // part they were spilled, each spill waiting for the whole ring)
        run_part<T, FE_FIN0, false>(c, accB, accA, 32, false, true, FSrc{true, 0, true},
                                             0, false);
        c.prev_shape = shape;
        c.prev_local = local;
        c.aux_w = c.aux_next;
    }
    // the last tile's layer 7 part 1: the FE_FIN1 units in their window order (a point's
    // value must not depend on whether its tile was its workgroup's last)
#pragma unroll
    for (int u = 0; u < 16; ++u) fin1_unit(c, accB, u);
    {
        float* rw = red_w(c);
#pragma unroll
        for (int n = 0; n < 4; ++n) rw[n * 64] = c.part[n];
    }
    fs_bar();
    fin_store_mode<MODE>(c);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (FS_STAMP && c.wave == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        for (int k = c.lane; k < 128; k += 64)
            reinterpret_cast<unsigned long long*>(a.out)[(size_t)blockIdx.x * 128 + k] = c.st[k];
    }
}

template <typename T, int S>
void launch_fs(const FArgs& a, bool points, hipStream_t s, int grid) {
    if (points)
        hipLaunchKernelGGL((dec_fs_kernel<T, S, kModePoints>), dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((dec_fs_kernel<T, S, kModeGrid>), dim3(grid), dim3(256), 0, s, a);
}

template <typename T, int S>
void launch_fs_bricks(const FArgs& a, hipStream_t s, int grid) {
    hipLaunchKernelGGL((dec_fs_kernel<T, S, kModeBricks>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

size_t decoder_fs_aux_bytes(int B) { return (size_t)B * 4 * 4 * kFsStep; }

int decoder_fs_n_stages(int skip_width) { return fs_nsteps(skip_width == 253 ? 256 : 512); }

int decoder_fs_fwd(const ldm_decoder_t* w, const float* beta, const float* xyz, int B, int npts,
                   int N, int k0, float vs, float origin, float* out, void* ws, size_t ws_bytes,
                   hipStream_t s, int num_cus, const int32_t* bricks, const int32_t* count,
                   int n_bricks) {
    const int S = w->skip_width == 253 ? 256 : 512;
    LDM_REQUIRE(w->n_stages == fs_nsteps(S), LDM_EINVAL, "split layout: n_stages %d != %d",
                w->n_stages, fs_nsteps(S));
    LDM_REQUIRE(ws != nullptr && ws_bytes >= decoder_fs_aux_bytes(B) && LDM_ALIGNED(ws, 16),
                LDM_ENOSPC, "workspace too small: need %zu bytes, got %zu",
                decoder_fs_aux_bytes(B), ws_bytes);
    LDM_REQUIRE((size_t)B * 4 * 4 * kFsStep < 0x7ffffff0u, LDM_EINVAL,
                "split layout: %d shapes exceed the aux buffer range", B);
    {
        const int n = B * 4 * 4 * 2 * 64;
        if (w->dtype == LDM_BF16)
            hipLaunchKernelGGL(fs_aux_pack_kernel<__bf16>, dim3((n + 255) / 256), dim3(256), 0, s,
                               beta, w->wxyz, B, (__bf16*)ws);
        else
            hipLaunchKernelGGL(fs_aux_pack_kernel<_Float16>, dim3((n + 255) / 256), dim3(256), 0,
                               s, beta, w->wxyz, B, (_Float16*)ws);
        if (int e = launch_status("fs_aux_pack")) return e;
    }
    FArgs a;
    a.stream = (const uint8_t*)w->weights;
    a.aux = (const uint8_t*)ws;
    a.w_last = w->w_last;
    a.xyz = xyz;
    a.out = out;
    a.b_last = w->b_last;
    a.npts = npts;
    a.tiles_per_shape = (npts + kTilePoints - 1) / kTilePoints;
    a.n_tiles = B * a.tiles_per_shape;
    a.bricks = bricks;
    a.count = count;
    a.nb = (N + 7) / 8;
    a.nbt = n_bricks;
    const int mode = bricks ? kModeBricks : xyz ? kModePoints : kModeGrid;
    // bricks mode: the kernel reads its tile count from *count; the grid covers the most it can be
    if (mode == kModeBricks) a.n_tiles = 4 * n_bricks;
    a.N = N;
    a.k0 = k0;
    a.vs = vs;
    a.origin = origin;
    a.gd = mode == kModeGrid ? grid_div(N) : GridDiv{0, 0, 0};
    const int grid = a.n_tiles < num_cus ? a.n_tiles : num_cus;
    // The brick instantiations are named after the grid / points ones, so the compiler emits
    // them last and the existing kernels keep their place in the code object: with the brick
    // kernels emitted first, the grid decode measured 0.16 % slower at identical instructions
    // (a 74 KB loop in a 64 KB instruction cache).
    if (mode != kModeBricks) {
        const bool points = mode == kModePoints;
        if (w->dtype == LDM_BF16) {
            if (S == 256) launch_fs<__bf16, 256>(a, points, s, grid);
            else launch_fs<__bf16, 512>(a, points, s, grid);
        } else {
            if (S == 256) launch_fs<_Float16, 256>(a, points, s, grid);
            else launch_fs<_Float16, 512>(a, points, s, grid);
        }
    } else if (w->dtype == LDM_BF16) {
        if (S == 256) launch_fs_bricks<__bf16, 256>(a, s, grid);
        else launch_fs_bricks<__bf16, 512>(a, s, grid);
    } else {
        if (S == 256) launch_fs_bricks<_Float16, 256>(a, s, grid);
        else launch_fs_bricks<_Float16, 512>(a, s, grid);
    }
    return launch_status("ldm_decoder_fwd(split)");
}

}  // namespace ldm
