// Host side of the one-launch training step (device: train_dag.hip, table: train_dag.h): the
// job-table builder, its extents check, the cache of uploaded tables and the table's text dump.
// The DAG is derived from the launch path itself: forward() / backward() run with a Recorder,
// so the GEMM problems (operands, epilogues, layouts) are the launch path's, and each keeps the
// k-group split of the tile its launch would run (gemm_tile_choice): bit-identical results.
#include "denoiser_train.h"
#include "wt_store.h"

#include <stdio.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <unordered_map>

namespace ldm {

int gemm_tile_choice(const ldm_gemm_args_t& a);
int gemm_tile_kgroup_period(int tile);

namespace {

uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
        h ^= c[i];
        h *= 1099511628211ull;
    }
    return h;
}

// the LDS-transposed epilogue's vector conditions (gemm_bf16.hip epi(): `ok`), for every block
bool lds_epilogue_ok(const ldm_gemm_prob_t& P) {
    auto al = [](const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; };
    return P.N % 64 == 0 && P.k_split <= 1 && (!P.C || (al(P.C, 16) && P.ldc % 4 == 0)) &&
           (!P.P || (al(P.P, 16) && P.ldp % 4 == 0)) &&
           (P.mode == LDM_GEMM_ACCUM || !P.R || (al(P.R, 16) && P.ldr % 4 == 0)) &&
           (!P.P_in || (al(P.P_in, 16) && P.ldp_in % 4 == 0)) &&
           (!P.Cb || (al(P.Cb, 8) && P.ldcb % 4 == 0)) &&
           (!P.Rb || (al(P.Rb, 8) && P.ldrb % 4 == 0)) && (!P.bias || al(P.bias, 16));
}

struct DagHost {
    uint64_t hash = 0;
    dag::Table tab;
    std::vector<uint32_t> entries;
};

// The uploaded tables, by device table address.  An entry's host copy is only read by its
// upload, which synchronises before dag_step returns, so entries may go at any time after that:
// ldm_denoiser_train_ws_init drops the one of its workspace, and the map is cleared when it
// reaches kMaxCached entries (a workload that keeps allocating workspaces of new sizes stays
// bounded; a dropped configuration re-uploads at its next step).  shared_ptr: a step in flight
// on another thread keeps its entry alive.
struct DagCache {
    static constexpr size_t kMaxCached = 32;
    std::mutex mu;
    std::unordered_map<const void*, std::shared_ptr<DagHost>> by_table;
};
DagCache& dag_cache() {
    static DagCache c;
    return c;
}

constexpr bool kSplitU = false;     // U_k's AdamW as an early update + late copies (measured: off)

// ---- operand extents vs the allocations (round 6, after the r05h illegal access) -----------
// Every byte range a job of the table may touch -- each GEMM operand over its problem's rows and
// leading dimension (ext_bytes, the same extents the kernel gives its buffer resources), the
// prep outputs, the sums' partials, each AdamW tensor -- must lie inside ONE allocation the
// caller handed over: the training workspace, a weight / bias / table of the descriptor, a
// gradient, an AdamW tensor, the schedule.  A table that fails is refused (LDM_EINVAL, named
// node and operand), so an indexing bug in the builder never reaches the GPU as a stray access.
struct Region {
    const char* p;
    int64_t bytes;
};
struct Regions {
    std::vector<Region> r;
    void add(const void* p, int64_t bytes) {
        if (p && bytes > 0) r.push_back({static_cast<const char*>(p), bytes});
    }
    bool holds(const void* p, int64_t bytes) const {
        const char* c = static_cast<const char*>(p);
        for (const Region& x : r)
            if (c >= x.p && c + bytes <= x.p + x.bytes) return true;
        return false;
    }
};

int check_dag_extents(const dag::Table& T, const ldm_denoiser_t* w, const ldm_sched_t* sc,
                      const TrainWs& L, const ldm_denoiser_grads_t* gr,
                      const ldm_adamw_tensor_t* tensors, int n, const void* eps_tag) {
    using namespace dag;
    const int64_t D = w->D, H = w->H, TE = w->TE, Tn = w->T;
    Regions R;
    R.add(L.xt_b, (int64_t)L.bytes);                        // the workspace (xt_b is its start)
    R.add(w->w_in, H * D * 2); R.add(w->w_t1, H * TE * 2); R.add(w->w_t2, H * H * 2);
    R.add(w->w_out, D * H * 2); R.add(w->wt_in, D * H * 2); R.add(w->wt_t2, H * H * 2);
    R.add(w->wt_out, H * D * 2);
    R.add(w->b_in, H * 4); R.add(w->b_t1, H * 4); R.add(w->b_t2, H * 4); R.add(w->b_out, D * 4);
    R.add(w->emb_table, Tn * TE * 4);
    for (int k = 0; k < w->n_blocks; ++k) {
        R.add(w->w_blk[k], H * 2 * H * 2); R.add(w->wt_blk[k], 2 * H * H * 2);
        R.add(w->b_blk[k], H * 4);
        R.add(gr->w_blk[k], H * 2 * H * 4); R.add(gr->b_blk[k], H * 4);
    }
    R.add(gr->w_in, H * D * 4); R.add(gr->b_in, H * 4); R.add(gr->w_t1, H * TE * 4);
    R.add(gr->b_t1, H * 4); R.add(gr->w_t2, H * H * 4); R.add(gr->b_t2, H * 4);
    R.add(gr->w_out, D * H * 4); R.add(gr->b_out, D * 4);
    R.add(sc->sqrt_ab, (int64_t)sc->T * 4); R.add(sc->sqrt_1mab, (int64_t)sc->T * 4);
    // (R so far: what the descriptors size.  An AdamW tensor's gradient and bf16 copies must
    // lie in it -- they are the step's own gradients and the descriptor's weights -- so a
    // tensor that claims more rows / columns than its gradient holds is refused below; its
    // fp32 master and moments are the caller's alone and join the regions here.)
    const Regions K = R;
    for (int i = 0; i < n; ++i) {
        const ldm_adamw_tensor_t& t = tensors[i];
        const int64_t e = (int64_t)t.rows * t.cols;
        R.add(t.p, e * 4); R.add(t.m, e * 4); R.add(t.v, e * 4);
    }
    const char* what = nullptr;
    int bad = -1;
    auto need = [&](int node, const char* name, const void* p, int64_t bytes) {
        if (!p || bytes <= 0 || bad >= 0 || p == eps_tag) return;   // eps: a launch argument
        if (bytes >= (int64_t)kMaxExtent || !R.holds(p, bytes)) {
            bad = node;
            what = name;
        }
    };
    for (int i = 0; i < T.n_nodes; ++i) {
        const Node& nd = T.node[i];
        if (nd.type == N_GEMM) {
            const ldm_gemm_prob_t& P = nd.P;
            const int64_t M = P.M, Nc = P.N, Mv = P.M_valid;
            // the job grid covers the problem and no more than one tile beyond it
            if ((int64_t)nd.tiles_m * tile_rows(nd.tile) < M ||
                (int64_t)(nd.tiles_m - 1) * tile_rows(nd.tile) >= M ||
                (int64_t)nd.tiles_n * tile_cols(nd.tile) < Nc ||
                (int64_t)(nd.tiles_n - 1) * tile_cols(nd.tile) >= Nc || Mv > M) {
                bad = i;
                what = "job grid vs problem";
            }
            int64_t ks = 0;
            for (int g = 0; g < P.n_seg; ++g) {
                const ldm_gemm_seg_t& S = P.seg[g];
                need(i, "A operand", S.A, ext_bytes(M, S.lda, S.K, 2));
                need(i, "B operand", S.B, ext_bytes(Nc, S.ldb, S.K, 2));
                if (S.K % 64 != 0) { bad = i; what = "segment K"; }
                ks += S.K / 64;
            }
            if (ks != nd.nk && bad < 0) { bad = i; what = "k-steps"; }
            need(i, "C", P.C, ext_bytes(Mv, P.ldc, Nc, 4));
            need(i, "P", P.P, ext_bytes(Mv, P.ldp, Nc, 4));
            if (P.mode != LDM_GEMM_ACCUM) need(i, "R", P.R, ext_bytes(Mv, P.ldr, Nc, 4));
            need(i, "P_in", P.P_in, ext_bytes(Mv, P.ldp_in, Nc, 4));
            need(i, "Rb", P.Rb, ext_bytes(Mv, P.ldrb, Nc, 2));
            need(i, "Cb", P.Cb, ext_bytes(M, P.ldcb, Nc, 2));
            need(i, "CbT", P.CbT, ext_bytes(Nc, P.ldct, M, 2));
            need(i, "colsum", P.colsum, ext_bytes((M - 1) / 32 + 1, Nc, Nc, 4));
            need(i, "loss_part", P.loss_part,
                 ext_bytes((M - 1) / 32 + 1, (Nc + 31) / 32, (Nc + 31) / 32, 4));
            need(i, "bias", P.bias, Nc * 4);
        } else if (nd.type == N_PREP) {
            need(i, "xt_b", nd.xt_b, ext_bytes(nd.Bp, nd.D, nd.D, 2));
            need(i, "xt_T", nd.xt_T, ext_bytes(nd.D, nd.Bp, nd.Bp, 2));
            need(i, "e_b", nd.e_b, ext_bytes(nd.Bp, nd.TE, nd.TE, 2));
            need(i, "e_T", nd.e_T, ext_bytes(nd.TE, nd.Bp, nd.Bp, 2));
            need(i, "emb", nd.emb, Tn * nd.TE * 4);
            if ((int64_t)nd.tiles_m * kBand < nd.Bp && bad < 0) { bad = i; what = "prep bands"; }
        } else if (nd.type == N_SUM) {
            need(i, "sum src", nd.src, ext_bytes(nd.rows, nd.ld, nd.len, 4));
            need(i, "sum dst", nd.dst, (int64_t)nd.len * 4);
        } else if (nd.type == N_ADAM) {
            if (nd.adam < 0 || nd.adam >= n) {
                if (bad < 0) { bad = i; what = "AdamW tensor index"; }
                continue;
            }
            const ldm_adamw_tensor_t& t = tensors[nd.adam];
            const int64_t e = (int64_t)t.rows * t.cols;
            for (const void* q : {static_cast<const void*>(t.g)})
                if (bad < 0 && q && !K.holds(q, e * 4)) { bad = i; what = "AdamW gradient"; }
            for (const void* q : {t.p_bf16, t.p_bf16_t})
                if (bad < 0 && q && !K.holds(q, e * 2)) { bad = i; what = "AdamW bf16 copy"; }
            if ((int64_t)nd.tiles_m * 64 < t.rows ||
                nd.col_off + nd.nk > (t.cols + 63) / 64) {
                if (bad < 0) { bad = i; what = "AdamW tiles vs tensor"; }
            }
        }
        if (nd.type == N_SUM && nd.adam >= 0 && nd.adam < n &&
            (int64_t)tensors[nd.adam].rows * tensors[nd.adam].cols != nd.len && bad < 0) {
            bad = i;
            what = "bias sum length vs its AdamW tensor";
        }
    }
    LDM_REQUIRE(bad < 0, LDM_EINVAL,
                "train dag: node %d: %s lies outside every allocation the step was given "
                "(or exceeds 2 GiB); table refused", bad, what ? what : "?");
    return 0;
}

// Builds the job table of one step; returns 1 (and builds nothing) when this configuration has
// no DAG form -- the caller then runs the launch path.
int build_dag(const ldm_denoiser_t* w, const ldm_sched_t* sc, const TrainWs& L,
              const ldm_denoiser_grads_t* gr, const ldm_adamw_tensor_t* tensors, int n,
              float nf, int grid, DagHost& H) {
    using namespace dag;
    const int nb = L.nb;
    Recorder rec;
    const float* kEps = reinterpret_cast<const float*>((uintptr_t)256);   // eps: a launch arg
    LDM_TRY(forward(w, L, kEps, nullptr, 2.f / nf, nullptr, &rec));
    LDM_TRY(backward(w, L, gr, nullptr, nullptr, nullptr, &rec));
    if ((int)rec.launches.size() != 2 * nb + 7) return 1;
    Table& T = H.tab;
    memset(&T, 0, sizeof(T));
    int nctr = 0;
    bool ok = true;
    auto add = [&](Node nd) -> int {
        if (T.n_nodes >= kMaxNodes) {          // (~50 nodes at 4 blocks; 8 blocks fit too)
            ok = false;
            return kMaxNodes - 1;
        }
        nd.out_band = -1;
        if (nd.type == N_GEMM || nd.type == N_PREP) {
            nd.out_band = nctr;
            nctr += nd.tiles_m;
        }
        nd.out_all = nctr++;
        T.node[T.n_nodes] = nd;
        return T.n_nodes++;
    };
    auto dep = [&](int c, int p, bool band) {
        Node& C = T.node[c];
        Node& Pn = T.node[p];
        Pn.signal = 1;
        // a band hand-off pairs the same 64-row bands: both nodes are row nodes
        if (band) ok = ok && (Pn.type == N_PREP || Pn.row) && (C.type == N_PREP || C.row);
        C.dep_ctr[C.ndep] = band ? Pn.out_band : Pn.out_all;
        C.dep_band[C.ndep] = band ? 1 : 0;
        C.dep_target[C.ndep] = band ? (unsigned)Pn.tiles_n : (unsigned)(Pn.tiles_m * Pn.tiles_n);
        ++C.ndep;
    };
    // row: the product's rows are the batch's (the forward / backward chain: band hand-offs,
    // 64 x 64 tiles); otherwise a weight-gradient product (rows = features, 128 x 128 tiles)
    auto gemm = [&](int li, int pi, bool row) -> int {
        const ldm_gemm_args_t& a = rec.launches[li];
        const ldm_gemm_prob_t& P = a.prob[pi];
        Node nd;
        memset(&nd, 0, sizeof(nd));
        nd.type = N_GEMM;
        nd.P = P;
        // row nodes: the batch's rows (the chain, band hand-offs); the tile kind: the launch
        // tile's two k-groups -> 64 x 64 in two groups, else 64 x 128 (row) or 128 x 128 (the
        // weight-gradient products) -- train_dag.hip TileCfg
        nd.row = row ? 1 : 0;
        ok = ok && (!row || P.M == L.Bp);
        for (int g = 0; g < P.n_seg; ++g) nd.nk += P.seg[g].K / 64;
        nd.kgp = gemm_tile_kgroup_period(gemm_tile_choice(a));
        bool k128 = true;                 // every segment's K a multiple of 128 (128-deep stages)
        for (int g = 0; g < P.n_seg; ++g) k128 = k128 && P.seg[g].K % 128 == 0;
        nd.tile = nd.kgp == 2 && k128 ? TILE_K2L : nd.kgp > 0 ? TILE_K2 : row ? TILE_ROW : TILE_W;
        nd.tiles_m = (P.M + tile_rows(nd.tile) - 1) / tile_rows(nd.tile);
        nd.tiles_n = (P.N + tile_cols(nd.tile) - 1) / tile_cols(nd.tile);
        nd.adam = -1;
        if (P.P_in == kEps) {
            nd.pin_eps = 1;
            nd.P.P_in = nullptr;
        }
        ok = ok && lds_epilogue_ok(nd.P) && P.ct_blk == 0 && nd.tiles_m * nd.tiles_n <= 65535;
        return add(nd);
    };
    // tensor of each gradient (AdamW), -1 if not in the table
    auto tens = [&](const float* g) {
        for (int i = 0; i < n; ++i)
            if (tensors[i].g == g) return i;
        return -1;
    };
    std::vector<bool> used(n, false);
    auto sum = [&](const float* src, float* dst, int rows, int len, int ld, float scale,
                   const float* g) -> int {
        Node nd;
        memset(&nd, 0, sizeof(nd));
        nd.type = N_SUM;
        nd.tiles_m = nd.tiles_n = 1;
        nd.src = src; nd.dst = dst; nd.rows = rows; nd.len = len; nd.ld = ld; nd.scale = scale;
        nd.adam = g ? tens(g) : -1;
        if (nd.adam >= 0) {
            const ldm_adamw_tensor_t& t = tensors[nd.adam];
            ok = ok && !t.p_bf16 && !t.p_bf16_t && (int64_t)t.rows * t.cols == len;
            used[nd.adam] = true;
        }
        return add(nd);
    };
    auto adam = [&](const float* g, int col_off, int col_tiles, int amode = 0) -> int {
        const int ti = tens(g);
        if (ti < 0) return -1;
        const ldm_adamw_tensor_t& t = tensors[ti];
        Node nd;
        memset(&nd, 0, sizeof(nd));
        nd.type = N_ADAM;
        nd.adam = ti;
        nd.amode = amode;
        nd.col_off = col_off;
        nd.tiles_m = (t.rows + 63) / 64;
        nd.nk = col_tiles ? col_tiles : (t.cols + 63) / 64;      // the node's 64-column tiles
        nd.tiles_n = (nd.nk + kAdamGroup - 1) / kAdamGroup;       // jobs: kAdamGroup of them
        used[ti] = true;
        return add(nd);
    };
    // ---- nodes in priority order (topological: every dependency is an earlier node) --------
    const int base = nb + 3, H_ = L.H;
    Node pr;
    memset(&pr, 0, sizeof(pr));
    pr.type = N_PREP;
    pr.tiles_m = (L.Bp + kBand - 1) / kBand;
    pr.row = 1;
    pr.tiles_n = (L.D + 63) / 64 + (L.TE + 63) / 64;     // 64-column chunks of [xt | e]
    pr.adam = -1;
    pr.sab = sc->sqrt_ab; pr.s1mab = sc->sqrt_1mab; pr.emb = w->emb_table;
    pr.B = L.B; pr.Bp = L.Bp; pr.D = L.D; pr.TE = L.TE;
    pr.xt_b = L.xt_b; pr.xt_T = L.xt_T; pr.e_b = L.e_b; pr.e_T = L.e_T;
    ok = ok && L.D % 4 == 0 && L.TE % 4 == 0;        // prep_job's 4-column stores
    const int prep = add(pr);
    const int f1 = gemm(0, 0, true), f3 = gemm(0, 1, true);
    dep(f1, prep, true);
    dep(f3, prep, true);
    const int f2 = gemm(1, 0, true);
    dep(f2, f1, true);
    std::vector<int> fb(nb);
    for (int k = 0; k < nb; ++k) {
        fb[k] = gemm(2 + k, 0, true);
        dep(fb[k], k == 0 ? f3 : fb[k - 1], true);
        dep(fb[k], f2, true);
    }
    const int fo = gemm(2 + nb, 0, true);
    dep(fo, fb[nb - 1], true);
    const int dhout = gemm(base, 1, true);
    dep(dhout, fo, true);
    dep(sum(L.p_bout, gr->b_out, L.Bp / 32, L.D, L.D, 1.f, gr->b_out), fo, false);
    dep(sum(L.loss_part, nullptr, (L.Bp / 32) * (L.D / 32), 1, 1, 1.f / nf, nullptr), fo,
        false);
    const int dwo = gemm(base, 0, false);
    dep(dwo, fo, false);
    std::vector<int> Dk(nb), dwk(nb), duk(nb), uupd(nb, -1);
    std::vector<bool> wdone(nb, false);
    bool wout_done = false;
    auto adam_w = [&](int k) {            // W_k's update: its gradient and dh_k (reads W_k^T)
        const int a = adam(gr->w_blk[k], 0, H_ / 64);
        if (a >= 0) {
            dep(a, dwk[k], false);
            dep(a, Dk[k], false);
        }
        wdone[k] = true;
    };
    auto adam_wout = [&]() {
        const int a = adam(gr->w_out, 0, 0);
        if (a >= 0) {
            dep(a, dwo, false);
            dep(a, dhout, false);
        }
        wout_done = true;
    };
    for (int i = 0; i < nb; ++i) {
        const int k = nb - 1 - i;
        const int gprod = k == nb - 1 ? dhout : Dk[k + 1];      // produced g_k and p_bblk[k]
        Dk[k] = gemm(base + 1 + i, 2, true);
        dep(Dk[k], gprod, true);
        dwk[k] = gemm(base + 1 + i, 0, false);
        dep(dwk[k], gprod, false);
        duk[k] = gemm(base + 1 + i, 1, false);
        dep(duk[k], gprod, false);
        dep(sum(L.p_bblk[k], gr->b_blk[k], L.Bp / 32, H_, H_, 1.f, gr->b_blk[k]), gprod, false);
        // (U_k's update waits for dtemb, which reads U_k^T: the tail below.  Split into an early
        // fp32 update here and late bf16 copies -- adamw_tile modes 1 / 2, kSplitU -- its
        // jobs took CUs from the backward chain: 321 -> 350 us per step, profiles/r05r.)
        if (kSplitU) {
            uupd[k] = adam(gr->w_blk[k], H_ / 64, H_ / 64, 1);
            if (uupd[k] >= 0) dep(uupd[k], duk[k], false);
        }
        if (k + 1 < nb) adam_w(k + 1);
        if (k == nb - 2) adam_wout();
    }
    if (!wout_done) adam_wout();
    dep(sum(L.p_bin, gr->b_in, L.Bp / 32, H_, H_, 1.f, gr->b_in), Dk[0], false);
    const int dt = gemm(base + 1 + nb, 0, true);
    dep(dt, nb >= 2 ? Dk[1] : dhout, true);      // the producer of g_0 (the chain covers g_k>0)
    adam_w(0);
    const int gt = gemm(base + 2 + nb, 1, true);
    dep(gt, dt, true);
    const int dwi = gemm(base + 3 + nb, 1, false);
    dep(dwi, Dk[0], false);
    const int dw2 = gemm(base + 2 + nb, 0, false);
    dep(dw2, dt, false);
    dep(sum(L.p_bt2, gr->b_t2, L.Bp / 32, H_, H_, 1.f, gr->b_t2), dt, false);
    // (Putting the critical tail -- dW_t1 and w_t1's update -- ahead of the U_k updates in node
    // order measured slower, 3070 -> 2972 steps/s, profiles/r05s: a queue hands out jobs in node
    // order, so a job placed before it is ready binds a workgroup to a wait.  Order by
    // readiness.)
    for (int k = nb - 1; k >= 0; --k) {      // U_k's update (or its bf16 copies): dtemb (WAR)
        const int u = adam(gr->w_blk[k], H_ / 64, H_ / 64, kSplitU ? 2 : 0);
        if (u >= 0) {
            dep(u, kSplitU ? uupd[k] : duk[k], false);
            dep(u, dt, false);
        }
    }
    const int dw1 = gemm(base + 3 + nb, 0, false);
    dep(dw1, gt, false);
    dep(sum(L.p_bt1, gr->b_t1, L.Bp / 32, H_, H_, 1.f, gr->b_t1), gt, false);
    int a = adam(gr->w_in, 0, 0);
    if (a >= 0) dep(a, dwi, false);
    a = adam(gr->w_t2, 0, 0);
    if (a >= 0) {
        dep(a, dw2, false);
        dep(a, gt, false);
    }
    a = adam(gr->w_t1, 0, 0);
    if (a >= 0) dep(a, dw1, false);
    for (int i = 0; i < n; ++i) ok = ok && used[i];         // every tensor is one of ours
    for (int i = 0; i < n; ++i) T.tensor[i] = tensors[i];
    if (!ok || nctr > kMaxCounters) return 1;
    // GEMM operands that are bf16 weight copies: a tensor's ADAM jobs rewrite its copies only
    // after every job reading them (the dependencies above), and the launch boundary before
    // the step made them visible, so those loads may go through the L2 (plain) instead of sc1
    // -- every band tile of a node re-reads the node's weights.  Measured ~1 % slower at config
    // 2 (profiles/r05v/train_ab_*.log), so only under ldm_dev_train_dag_flags kDbgWeightsL2.
    auto is_weight = [&](const void* p) {
        const char* c = static_cast<const char*>(p);
        for (int i = 0; i < n; ++i) {
            const int64_t bytes = (int64_t)tensors[i].rows * tensors[i].cols * 2;
            for (const void* w : {tensors[i].p_bf16, tensors[i].p_bf16_t}) {
                const char* w0 = static_cast<const char*>(w);
                if (w0 && c >= w0 && c < w0 + bytes) return true;
            }
        }
        return false;
    };
    for (int i = 0; i < T.n_nodes; ++i) {
        Node& nd = T.node[i];
        nd.stat = 0;
        if (nd.type != N_GEMM) continue;
        int sa = 1, sb = 2;
        for (int s = 0; s < nd.P.n_seg; ++s) {
            if (!is_weight(nd.P.seg[s].A)) sa = 0;
            if (!is_weight(nd.P.seg[s].B)) sb = 0;
        }
        nd.stat = sa | sb;
    }
    // every operand range inside an allocation the caller handed over (round 6)
    LDM_TRY(check_dag_extents(T, w, sc, L, gr, tensors, n, kEps));
    // every dependency points at an earlier node (the deadlock-freedom argument)
    for (int c = 0; c < T.n_nodes; ++c)
        for (int d = 0; d < T.node[c].ndep; ++d)
            LDM_REQUIRE(T.node[c].dep_ctr[d] < T.node[c].out_band ||
                            T.node[c].dep_ctr[d] < T.node[c].out_all,
                        LDM_EINVAL, "train dag: node %d depends on a later node", c);
    // ---- jobs -> queues: row bands of the batch stay on one queue (2 of the 16 bands each),
    // other nodes in contiguous chunks, single jobs round-robin
    std::vector<uint32_t> q[kQueues];
    int rr = 0;
    for (int i = 0; i < T.n_nodes; ++i) {
        const Node& nd = T.node[i];
        const int jobs = nd.tiles_m * nd.tiles_n;
        const bool rows = nd.type == N_PREP || (nd.type == N_GEMM && nd.row);
        for (int j = 0; j < jobs; ++j) {
            int qq;
            if (jobs == 1) qq = rr++ % kQueues;
            else if (rows) qq = (j / nd.tiles_n) * kQueues / nd.tiles_m;
            else qq = (int)((int64_t)j * kQueues / jobs);
            q[qq].push_back((uint32_t)i << 16 | (uint32_t)j);
        }
    }
    H.entries.clear();
    for (int qq = 0; qq < kQueues; ++qq) {
        T.qoff[qq] = (int)H.entries.size();
        T.qlen[qq] = (int)q[qq].size();
        H.entries.insert(H.entries.end(), q[qq].begin(), q[qq].end());
    }
    // the claim scheduler's lists: each queue split into its chain jobs and the rest
    for (int cls = 0; cls < 2; ++cls)
        for (int qq = 0; qq < kQueues; ++qq) {
            const int li = qq + cls * kQueues;
            T.qoff2[li] = (int)H.entries.size();
            for (uint32_t en : q[qq]) {
                const Node& nd = T.node[en >> 16];
                const bool chain = nd.type == N_PREP || (nd.type == N_GEMM && nd.row);
                if (chain == (cls == 0)) H.entries.push_back(en);
            }
            T.qlen2[li] = (int)H.entries.size() - T.qoff2[li];
        }
    if ((int)H.entries.size() > kMaxEntries) return 1;
    T.n_counters = nctr;
    T.n_entries = (int)H.entries.size();
    T.n_tensors = n;
    T.grid = grid;
    return 0;
}

}  // namespace

// LDM_TRAIN_AUTO's choice: the one-launch step where it measured faster than the launch path
// (not yet at config 2's batch -- profiles/r05*/train_ab.log).
bool dag_auto(int B) {
    (void)B;
    return false;
}

// The step as one launch.  Returns 1 when the configuration has no DAG form (nothing done).
int dag_step(const ldm_denoiser_t* w, const ldm_sched_t* sc, const float* x0, const float* eps,
             const int32_t* t, int B, void* saved, const ldm_denoiser_grads_t* grads,
             float* loss_out, const ldm_adamw_tensor_t* tensors, int n, const float* hy7,
             const float* d_hyper, unsigned spin, unsigned dbg, hipStream_t s) {
    const TrainWs L = layout(w, B, saved);
    int grid = 0;
    LDM_TRY(dag::dag_grid(&grid));
    // the table depends on every pointer and size it names: hash them (the kernel refuses a
    // table built for other inputs: status 3)
    uint64_t h = 1469598103934665603ull;
    h = fnv(h, w, sizeof(*w));
    h = fnv(h, sc, sizeof(*sc));
    h = fnv(h, grads, sizeof(*grads));
    h = fnv(h, tensors, sizeof(*tensors) * (size_t)n);
    h = fnv(h, &B, sizeof(B));
    h = fnv(h, &grid, sizeof(grid));
    h = fnv(h, &L.dag_table, sizeof(L.dag_table));
    const size_t tb = sizeof(dag::Table);
    h = fnv(h, &tb, sizeof(tb));
    DagCache& dc = dag_cache();
    std::shared_ptr<DagHost> hc;
    {
        std::lock_guard<std::mutex> g(dc.mu);
        if (dc.by_table.size() >= DagCache::kMaxCached && !dc.by_table.count(L.dag_table))
            dc.by_table.clear();
        std::shared_ptr<DagHost>& slot = dc.by_table[L.dag_table];
        if (!slot) slot = std::make_shared<DagHost>();
        hc = slot;
    }
    if (hc->hash != h) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        LDM_REQUIRE(hipStreamIsCapturing(s, &cs) == hipSuccess &&
                        cs == hipStreamCaptureStatusNone,
                    LDM_EINVAL, "ldm_denoiser_train_step_adamw (dag): the first step of a "
                    "configuration uploads its job table; run it once before graph capture");
        const int r = build_dag(w, sc, L, grads, tensors, n, (float)B * (float)w->D, grid, *hc);
        if (r != 0) {
            hc->hash = 0;
            return r;
        }
        hc->tab.hash = h;
        hipError_t e = hipMemcpyAsync(L.dag_table, &hc->tab, sizeof(dag::Table),
                                      hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(L.dag_table + 1, hc->entries.data(),
                               hc->entries.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemsetAsync(L.dag_sync, 0, dag::sync_bytes(dag::kMaxCounters), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);      // once per configuration
        LDM_REQUIRE(e == hipSuccess, (int)e, "train dag: table upload: %s",
                    hipGetErrorString(e));
        hc->hash = h;
    }
    dag::LaunchArgs a;
    memset(&a, 0, sizeof(a));
    a.tab = L.dag_table;
    a.sync = L.dag_sync;
    a.hash = h;
    a.x0 = x0; a.eps = eps; a.t = t; a.loss_out = loss_out;
    a.d_hyper = d_hyper;
    for (int i = 0; i < 7; ++i) a.hy[i] = hy7[i];
    a.spin_limit = spin ? spin : 2000000u;        // microseconds a wait may take: 2 s
    a.dbg = dbg;
    return dag::dag_launch(a, grid, s);
}

// ldm_denoiser_train_ws_init: the workspace is new, whatever was uploaded at this address is gone
void dag_forget(const void* table) {
    DagCache& dc = dag_cache();
    std::lock_guard<std::mutex> g(dc.mu);
    auto it = dc.by_table.find(table);
    if (it != dc.by_table.end()) dc.by_table.erase(it);     // re-built by the next step
}

}  // namespace ldm

using namespace ldm;

// Diagnostics: the job table a step of this configuration runs, as text (one line per node:
// type, jobs, k-steps, k-group period, counters, dependencies; then the queue lengths), built
// on the host exactly as the step builds it.  Returns 1 if the configuration has no DAG form.
extern "C" int ldm_denoiser_train_dag_describe(const ldm_denoiser_t* w, const ldm_sched_t* sc,
                                               int B, void* saved,
                                               const ldm_denoiser_grads_t* grads,
                                               const ldm_adamw_tensor_t* tensors, int n,
                                               char* buf, size_t len) {
    LDM_TRY(check_desc(w, B, true));
    LDM_TRY(check_grads(w, grads));
    LDM_REQUIRE(sc && saved && buf && len > 0 && tensors && n >= 1 &&
                    n <= LDM_ADAMW_MAX_TENSORS, LDM_EINVAL,
                "ldm_denoiser_train_dag_describe: bad arguments");
    const TrainWs L = layout(w, B, saved);
    int grid = 0;
    if (dag::dag_grid(&grid) != 0) grid = -1;        // (no device: the table alone)
    DagHost* h = new DagHost();
    const int r = build_dag(w, sc, L, grads, tensors, n, (float)B * (float)w->D, grid, *h);
    if (r != 0) {
        delete h;
        return r;
    }
    const dag::Table& T = h->tab;
    static const char* kType[] = {"gemm", "prep", "sum", "adam"};
    size_t o = 0;
#define put(...) (o < len ? (void)(o += (size_t)snprintf(buf + o, len - o, __VA_ARGS__)) : (void)0)
    put("grid %d nodes %d counters %d entries %d\n", T.grid, T.n_nodes, T.n_counters,
        T.n_entries);
    for (int i = 0; i < T.n_nodes; ++i) {
        const dag::Node& nd = T.node[i];
        put("%d %s %dx%d nk %d kgp %d band %d all %d sig %d wt %d deps", i, kType[nd.type],
            nd.tiles_m, nd.tiles_n, nd.nk, nd.kgp, nd.out_band, nd.out_all, nd.signal, nd.stat);
        for (int d = 0; d < nd.ndep; ++d)
            put(" [%d%s>=%u]", nd.dep_ctr[d], nd.dep_band[d] ? "+band" : "", nd.dep_target[d]);
        put("\n");
    }
    for (int q = 0; q < dag::kQueues; ++q) put("queue %d: %d jobs at %d\n", q, T.qlen[q], T.qoff[q]);
    for (int q = 0; q < 2 * dag::kQueues; ++q)
        put("claim list %d: %d jobs at %d\n", q, T.qlen2[q], T.qoff2[q]);
#undef put
    delete h;
    return 0;
}

#ifdef LDM_DEV_KNOBS
// Development build only (`make DEV=1`; not in include/ldm_sdf.h, not exported by the product
// library): skip the compute of DAG node types (bit t: type t of train_dag.h NodeType; the jobs
// still wait and signal), add the release / acquire fences to every hand-off (bit 7,
// dag::kDbgFences), the claim scheduler (kDbgClaim), weight operands through the L2
// (kDbgWeightsL2).
extern "C" int ldm_dev_train_dag_flags(unsigned flags) {
    train_cfg().dbg = flags;
    return 0;
}
#endif
