/*
 * ldm_sdf.h -- C ABI of libldm_sdf.so, the MI355X (gfx950) hot path of latent diffusion
 * over DeepSDF shape codes.
 *
 * The reference project (SGI-2022/Latent-Diffusion-Models-for-Shape-SDFs) ships no code:
 * /root/reference/README.md:1 is its only line, so it has no FFI to mirror.  Every entry
 * point below is the build-defined boundary of SURVEY.md §8(b); each cites the §8(a) row it
 * implements (and, for the Python side, the ldm_sdf/api.py function that calls it).
 *
 * Conventions:
 *   - All buffers are caller-owned DEVICE pointers (torch tensors), contiguous, 16-byte aligned
 *     (the shim checks alignment).  The library never allocates or frees device memory.
 *   - Every launch is asynchronous on the caller's stream; no hidden synchronisation, no
 *     hipMalloc / hipMemcpy (so calls can be captured into a hipGraph).  Exceptions, each
 *     documented at its declaration: the *_status reads synchronise the stream.
 *   - Return 0 on success, a negative LDM_E* code for an argument error, or a positive
 *     hipError_t.  ldm_last_error() returns a thread-local message for the last failure.
 *   - One device per process (the current HIP device, as set by torch).
 */
#ifndef LDM_SDF_H
#define LDM_SDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDM_ABI_VERSION 7

/* dtypes */
#define LDM_F32 0
#define LDM_BF16 1
#define LDM_F16 2

/* argument errors */
#define LDM_EINVAL (-22)
#define LDM_EALIGN (-14)
#define LDM_ENOSYS (-38)
#define LDM_ENOSPC (-28)

/* workspace ops for ldm_workspace_bytes() */
#define LDM_OP_DECODER_GRID 1
#define LDM_OP_DECODER_POINTS 2
/* ldm_workspace_bytes() returns the need of the (one) 16-bit layout, LDM_LAYOUT_SPLIT;
   ldm_workspace_bytes_layout() gives a layout's own size (0 for removed layouts) */

typedef void* ldm_stream_t; /* hipStream_t; NULL = the null stream */

/*
 * DeepSDF decoder weights, packed on the host by ldm_sdf/pack.py.
 * The hot kernels support hidden == 512 with 8 hidden layers and the latent re-injected at
 * layer 4 (DeepSDF); skip_width is the output width of layer 3: 253 (DeepSDF, L=256) or 512
 * (the "widen-skip" variant used for L >= H, config 5).  Layouts: DESIGN.md §3.
 */
typedef struct ldm_decoder {
    int32_t abi_version;  /* must equal LDM_ABI_VERSION */
    int32_t dtype;        /* LDM_F32 (parity kernel) / LDM_BF16 / LDM_F16 (MFMA kernel) */
    int32_t hidden;       /* H (512) */
    int32_t skip_width;   /* 253 or 512 */
    int32_t latent_dim;   /* L */
    int32_t n_stages;     /* bf16/f16: k-steps of one wave's weight stream (384 / 448 at skip
                             width 253 / 512); f32: 0 */
    const void* weights;  /* bf16/f16: per-wave stream blob (ldm_sdf/pack.py pack_split,
                             DESIGN.md §4); f32: fp32 blob */
    const float* wz;      /* fp32 [2][H][L]  latent columns of layer 0 and layer 4 */
    const float* bz;      /* fp32 [2][H]     biases of layer 0 and layer 4 */
    const float* wxyz;    /* fp32 [2][H][3]  xyz columns of layer 0 and layer 4 */
    const float* w_last;  /* fp32 [H] final 512->1 weights (bf16/f16: MFMA-row permuted) */
    float b_last;         /* final bias */
    int32_t layout;       /* bf16/f16 weight layout: LDM_LAYOUT_SPLIT */
} ldm_decoder_t;

/* Stage-blob layouts of the MFMA decoder. */
#define LDM_LAYOUT_PASS8 0   /* removed in ABI 5 (superseded by SPLIT): LDM_ENOSYS */
#define LDM_LAYOUT_QUARTER 1 /* removed in ABI 5 (superseded by SPLIT): LDM_ENOSYS */
#define LDM_LAYOUT_SPLIT 2   /* features split over the 4 waves, per-wave weight streams */
#define LDM_LAYOUT_SPLIT16 3 /* removed in ABI 7 (5.5 % slower than SPLIT): LDM_ENOSYS */

/* DDPM tables, fp32 device arrays of length T. */
typedef struct ldm_sched {
    int32_t abi_version;
    int32_t T;
    const float* sqrt_ab;   /* sqrt(abar_t) */
    const float* sqrt_1mab; /* sqrt(1 - abar_t) */
    const float* c1;        /* 1/sqrt(alpha_t) */
    const float* c2;        /* beta_t / sqrt(1 - abar_t) */
    const float* sigma;     /* sqrt(beta_t) */
} ldm_sched_t;

#define LDM_MAX_BLOCKS 8

/*
 * MLP denoiser (ldm_sdf/models.py MLPDenoiser).
 * Weights are [out][in] row-major in `dtype` (LDM_F32 or LDM_BF16); biases fp32.
 * w_blk[k] is [H][2H] = [W_k | U_k] acting on [h || temb].
 * e_tab[k] (inference only) is fp32 [T][H] = U_k temb(t) + b_k for every t.
 */
typedef struct ldm_denoiser {
    int32_t abi_version;
    int32_t dtype;
    int32_t D, H, n_blocks, TE, T;
    int32_t reserved;
    const void* w_in;   const float* b_in;    /* [H][D] */
    const void* w_t1;   const float* b_t1;    /* [H][TE] */
    const void* w_t2;   const float* b_t2;    /* [H][H] */
    const void* w_blk[LDM_MAX_BLOCKS];
    const float* b_blk[LDM_MAX_BLOCKS];       /* [H] */
    const float* e_tab[LDM_MAX_BLOCKS];       /* [T][H] */
    const void* w_out;  const float* b_out;   /* [D][H] */
    const float* emb_table;                   /* [T][TE] sinusoidal (A5) */
    /* bf16 training only (ldm_denoiser_fwd / _bwd / _train_step): TRANSPOSED bf16 copies the
     * backward's G W products read k-contiguous, kept current by ldm_adamw_multi. */
    const void* wt_in;                        /* [D][H]  = w_in^T  (only for dx)      */
    const void* wt_t2;                        /* [H][H]  = w_t2^T                     */
    const void* wt_blk[LDM_MAX_BLOCKS];       /* [2H][H] = w_blk[k]^T                 */
    const void* wt_out;                       /* [H][D]  = w_out^T                    */
} ldm_denoiser_t;

/* fp32 tensors with the denoiser's parameter shapes (gradients, masters, Adam moments). */
typedef struct ldm_denoiser_grads {
    float* w_in;  float* b_in;                /* [H][D], [H]   */
    float* w_t1;  float* b_t1;                /* [H][TE], [H]  */
    float* w_t2;  float* b_t2;                /* [H][H], [H]   */
    float* w_blk[LDM_MAX_BLOCKS];             /* [H][2H]       */
    float* b_blk[LDM_MAX_BLOCKS];             /* [H]           */
    float* w_out; float* b_out;               /* [D][H], [D]   */
} ldm_denoiser_grads_t;

/* ---- library -------------------------------------------------------------------------- */
int ldm_abi_version(void);
const char* ldm_last_error(void);
/* Device bytes of workspace an op needs (B shapes, n = N (grid) or P (points)). */
size_t ldm_workspace_bytes(int op, int B, int n, int dtype);
size_t ldm_workspace_bytes_layout(int op, int B, int n, int dtype, int layout);

/* ---- decoder: A1 grid coords, A2 latent fold, A3 fused MLP ----------------------------- */
/* A1 standalone: xyz_out fp32 [(k1-k0)*N*N][3], z slowest, x fastest, x = fl32(fl32(i*vs)+origin). */
int ldm_grid_coords(int N, int k0, int k1, float vs, float origin, float* xyz_out,
                    ldm_stream_t s);
/* A2: beta_out fp32 [B][2][H]; z fp32 [B][L]. */
int ldm_decoder_fold(const ldm_decoder_t* w, const float* z, int B, float* beta_out,
                     ldm_stream_t s);
/* out[0] (device) = max over shapes b of sqrt(mean_l z[b][l]^2), z fp32 [B][L]: the latent
 * scale the Python decode's dtype="auto" picks its 16-bit format by.
 * Non-finite input propagates: any NaN element gives NaN, else any +-Inf element gives +Inf. */
int ldm_latent_rms_max(const float* z, int B, int L, float* out, ldm_stream_t s);
/* A1+A3 grid mode: out fp32 [B][(k1-k0)*N*N] (the z-slab [k0,k1) of each shape's N^3 grid). */
int ldm_decoder_grid_fwd(const ldm_decoder_t* w, const float* beta, int B, int N, int k0,
                         int k1, float vs, float origin, float* out, void* ws,
                         size_t ws_bytes, ldm_stream_t s);
/* A3 point-list mode: xyz fp32 [B][P][3] -> out fp32 [B][P]. */
int ldm_decoder_points_fwd(const ldm_decoder_t* w, const float* beta, const float* xyz,
                           int B, int P, float* out, void* ws, size_t ws_bytes,
                           ldm_stream_t s);

/* ---- narrow-band decode: only the 8^3 bricks that can hold the level set ---
 * Brick: 8 x 8 x 8 voxels of the dense N^3 grid; nb = ceil(N / 8) per axis; brick (bz, by, bx)
 *   covers the voxels [8b, min(8b + 8, N)) per axis; id = (bz nb + by) nb + bx; global id =
 *   shape nb^3 + id.
 * Lattice: per axis the nb + 1 fine-grid indices min(8b, N - 1), b = 0..nb -- a subset of the
 *   fine grid with rule A1 coordinates, so a lattice value equals the dense decode's value at
 *   that voxel bit for bit.  A brick's 8 corners are the lattice points b and b + 1 per axis
 *   (when N - 1 is a multiple of 8 the last brick is one voxel thick and the two coincide).
 * Active: min over the corners of |v - level| <= band, or the corners not all on one side of
 *   level (v > level against v <= level), or a corner not finite.  band = L * 4 sqrt(3) * vs
 *   (half a brick's diagonal) makes every brick the surface of an L-Lipschitz field touches
 *   active; for any other field it is the caller's knob.  band = INFINITY: every brick.
 * Fill: every voxel of an inactive brick gets the brick's corner-0 value, lattice (bz, by, bx).
 * Sequence: ldm_band_lattice_coords -> ldm_decoder_points_fwd (coarse [B][(nb+1)^3]) ->
 *   ldm_band_classify -> ldm_band_fill -> ldm_decoder_bricks_fwd; the volume then equals the
 *   dense ldm_decoder_grid_fwd bit for bit on every voxel of an active brick.  Everything runs
 *   on the caller's stream; the count stays on the device. */
/* Scan scratch of ldm_band_classify (0 for invalid B / N). */
size_t ldm_band_workspace_bytes(int B, int N);
/* xyz_out fp32 [(nb+1)^3][3], z slowest: the lattice's coordinates. */
int ldm_band_lattice_coords(int N, float vs, float origin, float* xyz_out, ldm_stream_t s);
/* coarse fp32 [B][(nb+1)^3] -> active u8 [B nb^3] (16-byte aligned), bricks int32 [B nb^3]
 * capacity: the active global ids in ascending order (a pure function of the input: block sums +
 * scan, no atomics), count int32 [1] on the device.  B nb^3 < 2^31; band >= 0;
 * ws 256-byte aligned, ldm_band_workspace_bytes(B, N). */
int ldm_band_classify(const float* coarse, int B, int N, float level, float band,
                      uint8_t* active, int32_t* bricks, int32_t* count, void* ws,
                      size_t ws_bytes, ldm_stream_t s);
/* A1+A3 brick mode: decodes the voxels of the first *count bricks of the list into the dense
 * out fp32 [B][N][N][N] (ragged bricks clipped at N; entries outside [0, B nb^3) are skipped);
 * other voxels are not written.  *count is read on the device (0 is valid).  4 B nb^3 < 2^31
 * (fp32 descriptors: B nb^3 < 2^20).  ws as ldm_decoder_grid_fwd. */
int ldm_decoder_bricks_fwd(const ldm_decoder_t* w, const float* beta, int B, int N, float vs,
                           float origin, const int32_t* bricks, const int32_t* count, float* out,
                           void* ws, size_t ws_bytes, ldm_stream_t s);
/* Writes the fill into every inactive brick of out fp32 [B][N][N][N] (16-byte aligned). */
int ldm_band_fill(const float* coarse, const uint8_t* active, int B, int N, float* out,
                  ldm_stream_t s);

/* ---- decoder input gradients with frozen weights (csrc/decoder_grad.hip) ----
 * The derivative of the decoder's output with respect to its input [z || xyz]: SDF normals
 * (d f / d xyz) and the latent gradient of a frozen decoder (d / d z through the folded biases:
 * ldm_decoder_fold -> ldm_decoder_points_grad -> ldm_decoder_fold_bwd).  16-bit operands
 * (LDM_F16 / LDM_BF16), fp32 accumulation; forward and backward of a 64-point tile run in one
 * launch and keep only the ReLU sign bits.  Layers 1..7 are given twice, row-major [out][in] and
 * transposed [in][out], in `dtype`, zero padded to 256 rows / columns where the skip width is
 * 253: w[l] is [M_l][K_l], wt[l] is [K_l][M_l] with M_3 = K_4 = 256 or 512 (K_4: the h columns
 * of layer 4 only) and every other dimension 512. */
typedef struct ldm_decoder_grad {
    int32_t abi_version;  /* must equal LDM_ABI_VERSION */
    int32_t dtype;        /* LDM_F16 or LDM_BF16 (LDM_F32: LDM_ENOSYS) */
    int32_t skip_width;   /* 253 or 512 */
    int32_t latent_dim;   /* L */
    const void* w[8];     /* w[1..7] (w[0] unused), 16-byte aligned */
    const void* wt[8];    /* wt[1..7] (wt[0] unused), 16-byte aligned */
    const float* bias;    /* fp32 [8][512]: b_l zero padded; rows 0 and 4 unused (beta) */
    const float* wxyz;    /* fp32 [2][512][3]  xyz columns of layer 0 and layer 4 */
    const float* wz;      /* fp32 [2][512][L]  latent columns of layer 0 and layer 4 */
    const float* w_last;  /* fp32 [512] final 512->1 weights, natural order */
    float b_last;         /* final bias */
} ldm_decoder_grad_t;
/* Workspace of ldm_decoder_points_grad: the per-tile partial sums (0 for invalid sizes). */
size_t ldm_decoder_grad_ws_bytes(int B, int P, int dtype);
/* beta fp32 [B][2][512] (ldm_decoder_fold), xyz fp32 [B][P][3] ->
 *   sdf_out   fp32 [B][P]       tanh(pre)
 *   dxyz_out  fp32 [B][P][3]    s_p d pre_p / d xyz_p                          (nullable)
 *   dbeta_out fp32 [B][2][512]  sum_p s_p d pre_p / d beta, a fixed-order sum  (nullable)
 * gt == NULL, gradient mode: s_p = 1 - f_p^2, so the outputs are derivatives of f = tanh(pre);
 *   delta and scale are ignored and loss_out must be NULL.
 * gt fp32 [B][P], loss mode: s_p = d loss_p / d pre_p of ldm_sdf_l1_loss's clamped-L1 term
 *   (delta > 0, scale); loss_out[0] (nullable) = scale * sum_p |clamp(f_p) - clamp(gt_p)|.
 * The backward itself always carries d pre / d (.), s_p multiplies the fp32 outputs only.
 * B <= 65535, B P < 2^31; ws 256-byte aligned.  Deterministic: no atomics. */
int ldm_decoder_points_grad(const ldm_decoder_grad_t* w, const float* beta, const float* xyz,
                            int B, int P, const float* gt, float delta, float scale,
                            float* sdf_out, float* dxyz_out, float* dbeta_out, float* loss_out,
                            void* ws, size_t ws_bytes, ldm_stream_t s);
/* The transposed fold: dz_out fp32 [B][L] = wz[0]^T dbeta[b][0] + wz[1]^T dbeta[b][1], summed in
 * fp64 and rounded once. */
int ldm_decoder_fold_bwd(const ldm_decoder_grad_t* w, const float* dbeta, int B, float* dz_out,
                         ldm_stream_t s);

/* ---- DDPM: A8 reverse step, A9 q_sample + eps-MSE ------------------------------------ */
/* x_out[i] = c1[t]*(x[i] - c2[t]*eps[i]) + sigma[t]*z[i]  (z ignored at t == 0). n elements. */
int ldm_ddpm_step(const ldm_sched_t* sc, const float* x, const float* eps, const float* z,
                  int t, int n, float* x_out, ldm_stream_t s);
/* x_t[b][d] = sqrt_ab[t_b] x0 + sqrt_1mab[t_b] eps.  t int32 [B]. */
int ldm_q_sample(const ldm_sched_t* sc, const float* x0, const float* eps, const int32_t* t,
                 int B, int D, float* xt_out, ldm_stream_t s);
/* loss_out[0] = mean((eps_hat - eps)^2); grad_out = d loss / d eps_hat (may be NULL). */
int ldm_eps_mse_loss(const float* eps_hat, const float* eps, int n, float* loss_out,
                     float* grad_out, ldm_stream_t s);

/* ---- denoiser: A6 forward (sampling: uniform t) and the sampling step ------------------ */
/* eps_out fp32 [B][D] = net(x, t) for one timestep t shared by the batch (B <= 16), using
 * the tabulated e_tab.  ws: fp32 scratch of at least 2*B*H floats. */
int ldm_denoiser_fwd_uniform_t(const ldm_denoiser_t* w, const float* x, int t, int B,
                               float* eps_out, float* ws, ldm_stream_t s);
/* One DDPM reverse step fused with the denoiser (A6 + A8, the A10 loop body):
 * x_out = c1[t] (x - c2[t] net(x,t)) + sigma[t] z  (z ignored at t = 0).  x_out != x. */
int ldm_sample_step(const ldm_denoiser_t* w, const ldm_sched_t* sc, const float* x,
                    const float* z, int t, int B, float* x_out, float* ws, ldm_stream_t s);
/* The whole A10 loop as one persistent launch (whole grid resident): steps t_hi, t_hi-1, ...,
 * t_hi-steps+1 of ldm_sample_step, bit-identical to calling it per step.  x fp32 [2][B][D]
 * ping-pong with x[0] = x_T on entry; the result is x[steps & 1].  noise fp32 [T][B][D]
 * (noise[t] is the z of step t).  ws: ldm_sample_loop_ws_bytes(B, H) bytes, 256-byte aligned.
 * LDM_ENOSYS unless ldm_sample_loop_supported(w, B) (H = 1024, D in {256, 512}, 4 blocks,
 * B <= 16, and H/4 workgroups co-resident on the current device); callers then use
 * ldm_sample_step.  Every grid barrier is bounded: after the launch,
 * ldm_sample_loop_status() reads back 0 (completed) or 1 (abandoned on a timeout). */
int ldm_sample_loop_supported(const ldm_denoiser_t* w, int B);
size_t ldm_sample_loop_ws_bytes(int B, int H);
int ldm_sample_loop(const ldm_denoiser_t* w, const ldm_sched_t* sc, float* x, const float* noise,
                    int t_hi, int steps, int B, float* ws, size_t ws_bytes, ldm_stream_t s);
int ldm_sample_loop_status(const float* ws, int B, int H, unsigned* status_host, ldm_stream_t s);
/* Loop forms.  AUTO (default): the XCD-replica loop when the shape has it (bf16, status 2 on a
 * placement mismatch switches the device to XCD for good), else XCD. */
#define LDM_LOOP_AUTO 0
#define LDM_LOOP_REPLICA 1 /* one network copy per XCD, XCD-local tagged hand-offs */
#define LDM_LOOP_XCD 2     /* chip-wide loop, XCD-hierarchical grid barrier */
#define LDM_LOOP_DIRECT 3  /* chip-wide loop, hierarchical arrival, chip-wide polling */
#define LDM_LOOP_FLAT 4    /* chip-wide loop, one flat counter */
/* Explicit A/B and fault-injection control of ldm_sample_loop on the current device (the
 * library reads no environment variable): form LDM_LOOP_*, spin_limit (0 = default; a tiny
 * limit makes barriers give up, i.e. status 1), tagged (replica hand-offs: 1 = tagged
 * granules, default; 0 = XCD-local barriers).  Defaults: (LDM_LOOP_AUTO, 0, 1). */
int ldm_sample_loop_config(int form, unsigned spin_limit, int tagged);
/* The form the last ldm_sample_loop launch on the current device took (LDM_LOOP_REPLICA ..
 * LDM_LOOP_FLAT; 0 before any launch). */
int ldm_sample_loop_last_form(void);

/* The A10 loop for batches above 16 on the matrix cores (csrc/sample_batch.hip):
 * the contract of ldm_sample_loop -- x fp32 [2][B][D] ping-pong with x[0] = x_T on entry, the
 * result in x[steps & 1]; noise fp32 [T][B][D], noise[t] the z of step t, not read at t == 0;
 * steps t_hi .. t_hi-steps+1 -- as one pack launch and 2 + n_blocks ordinary ldm_gemm_bf16
 * launches per step, all enqueued by this one call on the caller's stream.  No grid barrier, no
 * spin wait and so no status word; no synchronisation, allocation or host read of device data
 * (the tables are read on the device at t): the call can be captured into a graph.
 * Arithmetic (the training forward's): bf16 operands (x and every h rounded to bf16 where a
 * product reads them), fp32 accumulation, fp32 residual stream, E_k[t] = e_tab[k] + t H as the
 * block bias, fp32 x in the update.  Not bitwise equal to the B <= 16 kernels, which keep fp32
 * activations.  A row's result does not depend on B nor on its position in the batch.
 * Supported: dtype LDM_BF16 with e_tab[k] set, D and H multiples of 64, 1..LDM_MAX_BLOCKS
 * blocks, 1 <= B <= 2^31 / max(D, H) rounded down to a multiple of 64 (LDM_ENOSYS above, and
 * for LDM_F32).  Rows >= B of x and noise are never touched.  ws: ldm_sample_batch_ws_bytes(w,
 * B) bytes (0 for an unsupported shape), 256-byte aligned (LDM_EALIGN; x and noise 16-byte);
 * LDM_ENOSPC when ws_bytes is short; LDM_EINVAL for t_hi / steps outside the schedule. */
int ldm_sample_batch_supported(const ldm_denoiser_t* w, int B);
size_t ldm_sample_batch_ws_bytes(const ldm_denoiser_t* w, int B);
int ldm_sample_batch(const ldm_denoiser_t* w, const ldm_sched_t* sc, float* x, const float* noise,
                     int t_hi, int steps, int B, void* ws, size_t ws_bytes, ldm_stream_t s);

/* ---- A6/A7/A9 training: denoiser forward with saved activations, backward, fused step ----
 * bf16 weights (w->dtype == LDM_BF16, the wt_* transposed copies set), matrix-core GEMMs
 * (ldm_gemm_bf16) with bf16 operands and fp32 accumulation, per-sample timesteps t int32 [B].
 * `saved` is a device workspace of ldm_denoiser_train_ws_bytes(w, B) bytes (256-B aligned):
 * the forward writes every activation the backward reads (bf16 GEMM operands in both layouts,
 * fp32 residual stream and pre-activations); its contents are opaque.  Gradients are fp32 in
 * the parameter shapes (ldm_denoiser_grads_t), overwritten (not accumulated).  Deterministic:
 * fixed reduction orders, no atomics.  D, H, TE multiples of 64; n_blocks 1..8. */
size_t ldm_denoiser_train_ws_bytes(const ldm_denoiser_t* w, int B);
/* eps_out fp32 [B][D] = net(x, t) (may be NULL when only the saved activations are wanted). */
int ldm_denoiser_fwd(const ldm_denoiser_t* w, const float* x, const int32_t* t, int B,
                     float* eps_out, void* saved, ldm_stream_t s);
/* Given deps = dL/d eps_hat fp32 [B][D] for the last ldm_denoiser_fwd on `saved`: every
 * parameter gradient, and dx = dL/dx fp32 [B][D] when dx != NULL. */
int ldm_denoiser_bwd(const ldm_denoiser_t* w, void* saved, const float* deps, int B,
                     const ldm_denoiser_grads_t* grads, float* dx, ldm_stream_t s);
/* A9 head.  xt_out (if not NULL) = sqrt(abar[t]) x0 + sqrt(1 - abar[t]) eps (bit-exact with the
 * fp32 oracle); eps_hat (if not NULL): loss_out[0] = mean((eps_hat - eps)^2) and grad_out (if
 * not NULL) = d loss / d eps_hat = 2 (eps_hat - eps) / (B D). */
int ldm_q_sample_loss(const ldm_sched_t* sc, const float* x0, const float* eps,
                      const int32_t* t, int B, int D, float* xt_out, const float* eps_hat,
                      float* loss_out, float* grad_out, ldm_stream_t s);
/* One whole DDPM training step's forward + backward (Alg. 1 without the optimizer):
 * q_sample -> net -> eps-MSE (loss_out[0]) -> every gradient, the loss gradient fused into
 * the out-projection's epilogue.  The data-parallel step (the update waits for the gradient
 * all-reduce).  Form per ldm_train_step_config: the launch path (17 launches, no host
 * synchronisation, graph-capturable) or the one-launch job DAG without AdamW nodes (its first
 * call per configuration uploads the table: one stream synchronisation, not inside a capture);
 * the same bits either way. */
int ldm_denoiser_train_step(const ldm_denoiser_t* w, const ldm_sched_t* sc, const float* x0,
                            const float* eps, const int32_t* t, int B, void* saved,
                            const ldm_denoiser_grads_t* grads, float* loss_out, ldm_stream_t s);

/* ---- optimizer (A7 training step) -------------------------------------------------------- */
/* Multi-tensor AdamW in ONE launch (torch.optim.AdamW's update order, as ldm_adamw_step):
 * per tensor fp32 p, g, m, v [rows][cols]; optional bf16 working copies p_bf16 [rows][cols]
 * and p_bf16_t [cols][rows] (transposed, for the backward's k-contiguous operands), rounded to
 * nearest even.  `tensors` is a HOST array of n <= LDM_ADAMW_MAX_TENSORS descriptors. */
#define LDM_ADAMW_MAX_TENSORS 40
typedef struct ldm_adamw_tensor {
    float* p; const float* g; float* m; float* v;
    void* p_bf16; void* p_bf16_t;
    int32_t rows, cols;
} ldm_adamw_tensor_t;
int ldm_adamw_multi(const ldm_adamw_tensor_t* tensors, int n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int step, ldm_stream_t s);
/* One whole single-rank training step: ldm_denoiser_train_step, then ldm_adamw_multi over
 * `tensors` (hyper-parameters as there; eps_adam is AdamW's eps).  The updates run in three
 * batches, each as soon as its gradients are final and no later launch of the step reads its
 * weights (matched by gradient pointer): grads->w_out / w_in / w_blk[k] after the backward's
 * dtemb launch, w_t1 / w_t2 after its last GEMM, everything else after the bias sums.  With a
 * `side` stream the batches run there behind fork events, on a grid capped at 2 workgroups per
 * CU, overlapping the backward's tail; s then waits for side.  side == NULL or == s: all in
 * order on s, one AdamW launch after the bias sums.  Results are those of the two calls in
 * sequence, bit for bit (each update reads only its own tensor's final gradient).  Measured
 * (DESIGN.md §5): the overlap does NOT pay at config 2 -- the HBM-bound AdamW slows the
 * latency-bound GEMMs beside it more than it hides -- so ldm_sdf.train passes side = NULL.  A data-parallel step needs the gradient all-reduce
 * in between: use the two calls there. */
int ldm_denoiser_train_step_adamw(const ldm_denoiser_t* w, const ldm_sched_t* sc,
                                  const float* x0, const float* eps, const int32_t* t, int B,
                                  void* saved, const ldm_denoiser_grads_t* grads,
                                  float* loss_out, const ldm_adamw_tensor_t* tensors, int n,
                                  double lr, double beta1, double beta2, double eps_adam,
                                  double weight_decay, int step, const float* d_hyper,
                                  ldm_stream_t s, ldm_stream_t side);
/* The whole step in ONE persistent launch (round 5, ABI 7; csrc/train_dag.hip):
 * with side == NULL (or == s), ldm_denoiser_train_step_adamw runs the step's job DAG -- input
 * preparation, every GEMM tile of the launch path with the same epilogues, the bias sums and every
 * AdamW tile -- in one launch whose workgroups take jobs as their inputs become ready (per 64-row
 * band for the residual chain, per problem for weight gradients and updates).  Results are those
 * of the launch path bit for bit.  The first call for a (descriptor, workspace, gradients, AdamW
 * table, B) configuration builds its job table on the host and uploads it into `saved` (one
 * stream synchronisation; not inside a graph capture); later calls launch at once.  Waits are
 * bounded: ldm_denoiser_train_status reads (and clears) the status word of `saved`: 0 ok, 1 a
 * wait timed out (the step's results are garbage), 3 the table in `saved` was built for other
 * inputs (nothing computed).  ldm_train_step_config selects the form per device:
 * LDM_TRAIN_AUTO (default: the form measured faster for the configuration, DESIGN.md §5 --
 * ldm_train_step_last_form tells which ran), LDM_TRAIN_LAUNCHES (the launch path), LDM_TRAIN_DAG
 * (required: LDM_ENOSYS otherwise); spin_limit: microseconds one dependency wait may take before
 * the launch gives up (0 = default, 2 s). */
#define LDM_TRAIN_AUTO 0
#define LDM_TRAIN_LAUNCHES 1
#define LDM_TRAIN_DAG 2
int ldm_train_step_config(int form, unsigned spin_limit);
int ldm_train_step_last_form(void);   /* the form the last step on this device ran (0: none) */
int ldm_denoiser_train_status(const ldm_denoiser_t* w, int B, void* saved, unsigned* status_host,
                              ldm_stream_t s);
/* Call once on a NEW `saved` workspace (fresh allocation) before its first one-launch step:
 * zeroes its sync words (on s) and drops the host's record of a job table uploaded to that
 * address.  The record is keyed by address and inputs, so a workspace allocated where a freed
 * one lay -- with the same descriptor, gradient and AdamW pointers, as a caching allocator
 * hands out -- would otherwise be taken as holding its predecessor's table and sync words,
 * which other allocations may have overwritten since (the kernel then reports status 3). */
int ldm_denoiser_train_ws_init(const ldm_denoiser_t* w, int B, void* saved, ldm_stream_t s);
/* Diagnostics (host only, no device work): the job table of this configuration as text into
 * buf[len] -- per node its type, jobs, k-steps, counters and dependencies, then the queues.
 * 1: the configuration has no one-launch form. */
int ldm_denoiser_train_dag_describe(const ldm_denoiser_t* w, const ldm_sched_t* sc, int B,
                                    void* saved, const ldm_denoiser_grads_t* grads,
                                    const ldm_adamw_tensor_t* tensors, int n, char* buf,
                                    size_t len);
/* d_hyper (may be NULL): a DEVICE array of the 7 AdamW scalars ldm_adamw_hyper computes for
 * (lr, beta1, beta2, eps_adam, weight_decay, step); the kernels read them from there instead
 * of the arguments, so a hipGraph captured once replays every step (the caller refills it).
 * ldm_adamw_hyper: host-only, the scalars exactly as the argument path derives them
 * (double, rounded once): [1 - lr wd, 1 - beta1, beta2, 1 - beta2, eps, lr / (1 - beta1^step),
 * sqrt(1 - beta2^step)]. */
void ldm_adamw_hyper(double lr, double beta1, double beta2, double eps, double weight_decay,
                     int step, float* out7);
/* AdamW on fp32 masters p [n] with grads g, moments m, v (torch.optim.AdamW's order; step is
 * 1-based).  p_bf16 (may be NULL): bf16 [n] working copy of the updated p, written in the same
 * pass (RNE). */
int ldm_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                   double lr, double beta1, double beta2, double eps, double weight_decay,
                   int step, ldm_stream_t s);

/* ---- generic fused linear (A6/A7 building block, training) ---------------------------- */
/* acc[b][m] = sum_{k<K} X[b][k] W[m][k]  +  sum_{k<K2} X2[b][k] W2[m][k]   (K2 may be 0)
 * with arbitrary element strides, so the forward (X W^T), input-gradient (G W) and
 * weight-gradient (G^T X) products -- and the block's [h || temb] [W_k | U_k]^T -- are all
 * this one call.  Epilogues (pre = acc + bias, bias optional):
 *   LDM_EPI_BIAS        Y = pre
 *   LDM_EPI_SILU        Y = SiLU(pre);      A_out = pre (if A_out)
 *   LDM_EPI_RESID_SILU  Y = R + SiLU(pre);  A_out = pre (if A_out)      (A6 block)
 *   LDM_EPI_ACCUM       Y = Y + pre
 *   LDM_EPI_ADD_R       Y = R + pre                                     (A7 dh = dy + W^T g)
 *   LDM_EPI_RELU        Y = max(pre, 0)                    (C19 decoder hidden layers)
 *   LDM_EPI_MASK_R      Y = R > 0 ? pre : 0   (C19: ReLU backward through the post-activation
 *                                              R, fused into the G W product)
 * w_dtype: LDM_F32 or LDM_BF16 (elements of W and W2). */
#define LDM_EPI_BIAS 0
#define LDM_EPI_SILU 1
#define LDM_EPI_RESID_SILU 2
#define LDM_EPI_ACCUM 3
#define LDM_EPI_ADD_R 4
#define LDM_EPI_RELU 5
#define LDM_EPI_MASK_R 6
typedef struct ldm_linear_args {
    int32_t Bn, M, K, K2;
    int32_t epi;
    int32_t w_dtype;
    const float* X;  int64_t sxb, sxk;
    const void* W;   int64_t swm, swk;
    const float* X2; int64_t sx2b, sx2k;
    const void* W2;  int64_t sw2m, sw2k;
    const float* bias;               /* [M] or NULL */
    const float* R;  int64_t srb;    /* residual rows (col stride 1) */
    float* Y;        int64_t syb, sym;
    float* A_out;    int64_t sab;    /* pre-activation rows (col stride 1) */
    int32_t compute;                 /* LDM_COMPUTE_FP32 or LDM_COMPUTE_BF16 (below) */
    float* ws; int64_t ws_floats;    /* optional split-K workspace (LDM_COMPUTE_BF16), or NULL */
} ldm_linear_args_t;
/* LDM_COMPUTE_FP32: exact fp32 products (VALU register-tiled kernel).
 * LDM_COMPUTE_BF16: matrix cores -- X and W rounded to bf16 (RNE) as they are staged, fp32
 * products and accumulation (mixed-precision training; any w_dtype). */
#define LDM_COMPUTE_FP32 0
#define LDM_COMPUTE_BF16 1
int ldm_linear(const ldm_linear_args_t* a, ldm_stream_t s);
/* Split-K (LDM_COMPUTE_BF16, K2 == 0): when the output has too few 64x64 tiles to fill the
 * chip and K is long -- the weight gradients G^T X over ~1M samples of C19 -- the K range is
 * cut into slices that run as separate workgroups, each writing a partial [Bn][M] into ws,
 * and a second kernel sums the slices in fixed order (deterministic) and applies the
 * epilogue.  Returns the ws size (floats) that enables it for these args (0: not worth it);
 * ldm_linear uses it when a->ws has at least that many floats, else runs unsplit. */
int64_t ldm_linear_workspace_floats(const ldm_linear_args_t* a);

/* SiLU backward on the block pre-activation: g = dy * silu'(a)  (A7). n elements. */
int ldm_silu_bwd(const float* dy, const float* a, int n, float* g_out, ldm_stream_t s);
/* Column sums: out[m] (+)= sum_b G[b][m]  (bias gradients).  accumulate != 0 adds. */
int ldm_colsum(const float* G, int Bn, int M, float* out, int accumulate, ldm_stream_t s);
/* Row gather: out[b][:] = table[idx[b]][:] (timestep-embedding lookup, A5). */
int ldm_gather_rows(const float* table, const int32_t* idx, int Bn, int C, float* out,
                    ldm_stream_t s);

/* ---- C19 auto-decoder training (DeepSDF decoder backward + latent codes) --- */
/* The decoder forward/backward GEMMs are ldm_linear (LDM_EPI_RELU forward; G W and G^T X
 * backward) and the bias gradients ldm_colsum; these are the remaining pieces.
 * ReLU backward on the post-activation: g = dy * (y > 0).  n elements. */
int ldm_relu_bwd(const float* dy, const float* y, int n, float* g_out, ldm_stream_t s);
/* DeepSDF clamped L1 on the decoder's pre-tanh output (deep_sdf train loop, enforce_minmax):
 * pred = tanh(pre), loss_out[0] = scale * sum_i |clamp(pred_i) - clamp(gt_i)| with clamp to
 * [-delta, delta], and grad_out[i] = d loss / d pre_i
 *   = scale * sign(clamp(pred_i) - clamp(gt_i)) * [-delta <= pred_i <= delta] * (1 - pred_i^2)
 * (sign(0) = 0; the clamp passes the gradient on the closed interval).  One workgroup, fixed
 * summation order.  grad_out may be NULL. */
int ldm_sdf_l1_loss(const float* pre, const float* gt, int n, float delta, float scale,
                    float* loss_out, float* grad_out, ldm_stream_t s);
/* Segmented column sums: out[s][m] (+)= sum_{p<P} G[s*P + p][m] for s < S (per-shape latent
 * gradients: S shapes of P samples each, rows grouped by shape).  Deterministic. */
int ldm_colsum_segments(const float* G, int S, int P, int M, float* out, int accumulate,
                        ldm_stream_t s);
/* DeepSDF code regulariser, per-sample L2 norm: loss_io[0] += coef * sum_s |z_s| and
 * grad_io[s][:] += coef * z_s / |z_s| (0 where z_s = 0), z fp32 [S][L].  With S shapes of P
 * samples each out of N = S P, DeepSDF's lambda * min(1, epoch/100) * sum_samples |z| / N is
 * coef = lambda * min(1, epoch/100) / S.  One workgroup, fixed order. */
int ldm_latent_l2_reg(const float* z, int S, int L, float coef, float* loss_io, float* grad_io,
                      ldm_stream_t s);

/* ---- grouped bf16 GEMM with fused training epilogues (csrc/gemm_bf16.hip) ---
 * Per problem:  acc[m][n] = sum_seg sum_{k < K_seg} A_seg[m][k] B_seg[n][k]
 * A_seg / B_seg: bf16, k contiguous (row strides lda / ldb in elements, multiples of 8, 16-B
 * aligned), K_seg a multiple of 64.  A K-concatenation ([h || temb] [W | U]^T) is two segments.
 * Rows m >= M_valid are padding: R / P_in / C are not read there and the fp32 outputs (C, P) not
 * written (so caller buffers need only M_valid rows), the bf16 outputs Cb / CbT get zeros (so
 * operand buffers padded to M rows stay zero-padded), and they add nothing to colsum / loss.
 * Epilogue, with pre = acc + bias[n] (bias optional):
 *   LDM_GEMM_STORE       out = pre
 *   LDM_GEMM_SILU        out = SiLU(pre);        P = pre (if P)
 *   LDM_GEMM_RESID_SILU  out = R + SiLU(pre);    P = pre (if P)                 (A6 block)
 *   LDM_GEMM_RELU        out = max(pre, 0)
 *   LDM_GEMM_ACCUM       out = C + pre
 *   LDM_GEMM_DGRAD_SILU  dh = (R +) pre -> C;  out = dh * SiLU'(P_in)  (A7: the gradient at the
 *                        layer below's pre-activation, fused into the G W product)
 *   LDM_GEMM_LOSS        d = pre - P_in (targets); out = scale * d; loss_part += d^2 (A9)
 *   LDM_GEMM_ADD_R       out = R + pre
 *   LDM_GEMM_RELU_BWD    out = Rb[m][n] > 0 ? pre : 0   (Rb bf16: the ReLU backward through the
 *                        saved post-activation, fused into the G W product; C19)
 * Outputs (each optional): C fp32 [m][n] (ldc; in DGRAD_SILU C receives dh), Cb bf16 [m][n]
 * (ldcb), CbT bf16 TRANSPOSED [n][m] (ldct; M and ldct multiples of 4), colsum fp32
 * [ceil(M/32)][N]: per 32-row block column sums of out (bias gradients, summed in fixed order
 * by the caller), loss_part fp32 [ceil(M/32)][ceil(N/32)]: sums of d^2 (LOSS).
 * Split-K (k_split > 1; n_seg == 1, mode STORE or ACCUM, C the only output, K a multiple of
 * 128 * k_split): the K range is cut into k_split slices that run as separate tiles, each
 * writing its raw fp32 partial [M_valid][N] into ws (k_split * M * N floats); a second kernel
 * sums the slices in slice order (deterministic) and applies bias / ACCUM.  For the weight
 * gradients G^T X of C19, contracted over ~1M samples into a 512 x 512 output.
 * Up to LDM_GEMM_MAX_PROBS independent problems share one launch.  tile: 0 = auto, 1 = 64x64,
 * 2 = 128x64, 3 = 128x128, 4 = 64x64 with a 3-deep ring; 5 / 6 / 7 = 64x64 / 128x128 / 128x64
 * with 8 waves in two k-groups; 16 / 17 / 18 = persistent 128x128 (4-deep ring) / 128x128
 * (2-deep ring, 2 workgroups per CU) / 64x64 (3-deep ring): one workgroup per CU slot loops
 * over tiles and its LDS ring streams the next tile's k-steps under the current tile's last
 * MFMAs and epilogue (csrc/gemm_bf16.hip). */
#define LDM_GEMM_MAX_SEGS 8
#define LDM_GEMM_MAX_PROBS 4
#define LDM_GEMM_STORE 0
#define LDM_GEMM_SILU 1
#define LDM_GEMM_RESID_SILU 2
#define LDM_GEMM_RELU 3
#define LDM_GEMM_ACCUM 4
#define LDM_GEMM_DGRAD_SILU 5
#define LDM_GEMM_LOSS 6
#define LDM_GEMM_ADD_R 7
#define LDM_GEMM_RELU_BWD 8
typedef struct ldm_gemm_seg {
    const void* A; const void* B;    /* bf16 */
    int64_t lda, ldb;
    int32_t K, reserved;
} ldm_gemm_seg_t;
typedef struct ldm_gemm_prob {
    int32_t M, N, M_valid, n_seg;
    ldm_gemm_seg_t seg[LDM_GEMM_MAX_SEGS];
    int32_t mode; float scale;
    const float* bias;
    const float* R;    int64_t ldr;
    const float* P_in; int64_t ldp_in;
    float* C;          int64_t ldc;
    float* P;          int64_t ldp;
    void* Cb;          int64_t ldcb;
    void* CbT;         int64_t ldct;
    float* colsum;
    float* loss_part;
    int32_t k_split;   /* 0 or 1: whole K per tile; > 1: split-K into ws (see above) */
    int32_t ct_blk;    /* > 0: CbT written m-blocked, [ceil(M/ct_blk)][N][ct_blk] (ldct unused):
                        * the sample-axis operands of C19, whose 1M-long rows would otherwise put
                        * every row of a tile in its own memory page */
    float* ws;
    const void* Rb;    int64_t ldrb;   /* bf16 [m][n] (LDM_GEMM_RELU_BWD) */
    int64_t slice_a, slice_b;          /* split-K: slice s starts s * slice_a (A) / s * slice_b
                                        * (B) elements in (0: s * K / k_split, contiguous K);
                                        * with ct_blk-blocked operands each slice is one block */
} ldm_gemm_prob_t;
typedef struct ldm_gemm_args {
    int32_t n_prob, tile;
    ldm_gemm_prob_t prob[LDM_GEMM_MAX_PROBS];
} ldm_gemm_args_t;
int ldm_gemm_bf16(const ldm_gemm_args_t* a, ldm_stream_t s);

/* ---- C17 1D-UNet denoiser: fused conv1d (implicit GEMM) ------------------ */
/* Y[b][co][l] = epi( sum_s sum_{ci<C_s} sum_{k<ksize_s} W_s(co,ci,k) * act_s(Xsrc_s(b,ci,l,k))
 *                    + bias[co] + bias2[co] + cbias[b*scb + co]  (+ R[b][co][l]) )
 * act_s = SiLU if silu_in else identity (applied to the input before the taps).
 * Xsrc for LDM_CONV_DIRECT: X[b][ci][l*stride + k - pad];  LDM_CONV_UP2 (nearest 2x upsample,
 * then the conv, stride 1): p = l + k - pad, X[b][ci][p >> 1] for 0 <= p < 2 L_in.
 * Out-of-range positions read 0 (zero padding).  Weights are packed for the matrix cores
 * (ldm_sdf/ops.py pack_conv_weight): a torch [Cout][Cw][K] weight becomes
 * Wp[Cout16][K][Cw16] (Cout16, Cw16 = sizes rounded up to 16, zero-filled) with the input
 * channel stored at perm16(ci) = (ci & ~15) | ((ci & 3) << 2) | ((ci >> 2) & 3), so
 * W_s(co,ci,k) = W_s[co*ldw + k*kstride + perm16(ci)] with ldw = K*Cw16, kstride = Cw16.
 * A channel concat [u || s] is two segments whose W_s point at channel offsets (multiples
 * of 16) of one packed weight.
 * Epilogues: LDM_CONV_EPI_STORE  Y = pre
 *            LDM_CONV_EPI_DDPM   Y = c1[t] (xlat - c2[t] pre) + sigma[t] z   (A8 with
 *                                eps = pre; z ignored at t = 0; the UNet's output conv)   */
#define LDM_CONV_DIRECT 0
#define LDM_CONV_UP2 1
#define LDM_CONV_MAX_SEGS 4
#define LDM_CONV_EPI_STORE 0
#define LDM_CONV_EPI_DDPM 1
typedef struct ldm_conv1d_seg {
    const float* X;  /* fp32 [B][C][L_in] */
    const void* W;   /* w_dtype, packed (see above) */
    int32_t C, L_in, ksize, stride, pad, mode, silu_in, ldw, kstride;
} ldm_conv1d_seg_t;
typedef struct ldm_conv1d_args {
    int32_t B, Cout, L_out, n_seg, w_dtype, epi;
    ldm_conv1d_seg_t seg[LDM_CONV_MAX_SEGS];
    const float* bias;                /* [Cout] or NULL */
    const float* bias2;               /* [Cout] or NULL (shortcut bias) */
    const float* cbias; int64_t scb;  /* per-(b, co) bias or NULL; scb = 0: batch-uniform */
    const float* R;                   /* residual [B][Cout][L_out] or NULL */
    float* Y;                         /* [B][Cout][L_out] */
    const float* xlat; const float* z;           /* LDM_CONV_EPI_DDPM: x_t and noise [B][L] */
    const float* c1; const float* c2; const float* sigma; int32_t t;   /* A4 device tables */
} ldm_conv1d_args_t;
int ldm_conv1d(const ldm_conv1d_args_t* a, ldm_stream_t s);

/* ---- C17 training: the backward of the fused conv (csrc/unet_bwd.hip) ----- */
/* Data gradient of ONE forward segment (the ldm_conv1d_seg_t of the forward call: X is read for
 * SiLU' only when silu_in; W is the forward's packed weight at the segment's channel offset,
 * fp32 or bf16 storage):
 *   dX[b][ci][p] (=|+=) act'(X[b][ci][p]) * sum_co sum_k sum_{l : src(l,k) = p}
 *                                                       W(co,ci,k) * dY[b][co][l]
 * act' = SiLU' if silu_in else 1; accumulate != 0 adds to dX (an activation with several
 * consumers takes its gradients through successive calls, in the caller's order: no atomics).
 * Geometries: those of ldm_conv1d (ksize 1 / 3 stride 1, ksize 3 / 4 stride 2, LDM_CONV_UP2);
 * any other ksize / stride: LDM_ENOSYS.  W must sit at a multiple of 16 channels (LDM_EALIGN),
 * ldw and kstride must be multiples of 16. */
typedef struct ldm_conv1d_bwd_data_args {
    int32_t B, Cout, L_out, w_dtype, accumulate, reserved;
    ldm_conv1d_seg_t seg;
    const float* dY;                  /* [B][Cout][L_out] */
    float* dX;                        /* [B][seg.C][seg.L_in] */
} ldm_conv1d_bwd_data_args_t;
int ldm_conv1d_bwd_data(const ldm_conv1d_bwd_data_args_t* a, ldm_stream_t s);

/* Weight gradient of ONE forward conv, all its segments sharing dY (seg[i].W is not read):
 *   dW_s(co,ci,k) = sum_b sum_l dY[b][co][l] * act_s(Xsrc_s(b,ci,l,k))
 * written fp32 in the forward's packed layout: dW[i] points into a [Cout16][ksize][Cw16] buffer at
 * the segment's channel offset (pitches seg[i].ldw / kstride), and the call writes the segment's
 * round16(C) columns of all Cout16 rows and taps, zeros in the padding.  dbias[co] = sum_{b,l} dY
 * and dcbias[b][co] = sum_l dY[b][co][l] when not NULL.  The contraction over B * L_out is split
 * over workgroups into fp32 partials in ws and reduced in fixed order: the result is a pure
 * function of the inputs.  ws needs ldm_conv1d_bwd_weight_ws_floats(a) floats (LDM_ENOSPC). */
typedef struct ldm_conv1d_bwd_weight_args {
    int32_t B, Cout, L_out, n_seg;
    ldm_conv1d_seg_t seg[LDM_CONV_MAX_SEGS];
    float* dW[LDM_CONV_MAX_SEGS];
    const float* dY;                  /* [B][Cout][L_out] */
    float* dbias;                     /* [Cout] or NULL */
    float* dcbias;                    /* [B][Cout] or NULL */
    float* ws; int64_t ws_floats;
} ldm_conv1d_bwd_weight_args_t;
/* 0 for invalid args.  S * sum_s Cout16 * ksize_s * round16(C_s), S = min(64, B * ceil(L_out / 64))
 * slices, + B * Cout when dbias is asked for without dcbias. */
int64_t ldm_conv1d_bwd_weight_ws_floats(const ldm_conv1d_bwd_weight_args_t* a);
int ldm_conv1d_bwd_weight(const ldm_conv1d_bwd_weight_args_t* a, ldm_stream_t s);

/* (ABI 6: the round-3 one-launch UNet sampling loop, ldm_unet_loop*, was retired -- at 0.53x the
 * hipGraph of ldm_conv1d launches after the round-4 conv staging) */

/* ---- C18 marching cubes on a decoded volume ---------------------------- */
/* vol: fp32 [N][N][N] (z slowest, as decode writes it); a corner is inside when v < level.
 * Vertices are one per crossing grid edge, ordered by (owner point, axis), positions by the A1
 * grid rule and p0 + t (p1 - p0), t = (level - v0) / (v1 - v0), each op rounded to fp32;
 * faces are int32 vertex triples ordered by (cube, case-table order), wound so that
 * (b - a) x (c - a) points toward larger values.  Two passes, because the caller allocates
 * the outputs: ldm_mc_count writes device int32 counts_out[2] = {n_vertices, n_faces};
 * ldm_mc_emit (same vol / level / ws) then fills verts fp32 [V][3] and faces int32 [F][3]. */
size_t ldm_mc_workspace_bytes(int N);
int ldm_mc_count(const float* vol, int N, float level, void* ws, size_t ws_bytes,
                 int32_t* counts_out, ldm_stream_t s);
int ldm_mc_emit(const float* vol, int N, float level, float vs, float origin, void* ws,
                size_t ws_bytes, float* verts, int32_t* faces, ldm_stream_t s);
/* Host: the compile-time generated case table: tri [256][16] cube-edge ids (-1 padded),
 * ntri [256].  Edge e = 4a + m runs along axis a (x, y, z) from the corner whose other two
 * coordinate bits (lower axis first) are m; corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1). */
int ldm_mc_table(int8_t* tri, uint8_t* ntri);

/* ---- mesh -> signed distance samples (additive in ABI 7) ------------------ */
/* For P points [P][3] against the triangle soup verts fp32 [V][3], faces int32 [F][3], every
 * point-triangle pair evaluated:
 *   sdf      [P]  -d when winding > 0.5, else +d; d the distance to the closest triangle
 *                 (Voronoi-region closest point; a zero-area triangle is its segment or point)
 *   closest  [P]  (or NULL) index of that triangle, the smaller index on a tie
 *   winding  [P]  (or NULL) generalized winding number, sum of solid angles / 4 pi (a pair
 *                 whose triple product is exactly 0 contributes 0)
 * A point's outputs are a pure function of the point and the mesh: bitwise the same alone or
 * in any batch, and from run to run.  F == 0 gives d = +inf, closest = -1, winding = 0; P == 0
 * returns 0 with nothing written.
 * A face index outside [0, V) is never read through: it is clamped, and the device word *flag
 * (zeroed by the call) is set to 1 -- the outputs are then meaningless.
 * ws: 256-byte aligned, ldm_mesh_sdf_ws_bytes(F, P) bytes (0 for negative sizes); it holds the
 * packed triangles and, below ldm_mesh_sdf_split_below() points with more than one chunk of
 * ldm_mesh_sdf_face_chunk() faces, one tile of per-chunk partials.
 * LDM_EINVAL also for a grid beyond the launch limits: more than 65535 chunks of faces in the
 * split form, more than 2^31 - 1 workgroups of 256 points in the other. */
size_t ldm_mesh_sdf_ws_bytes(int F, int64_t P);
int ldm_mesh_sdf(const float* verts, int V, const int32_t* faces, int F, const float* points,
                 int64_t P, float* sdf, int32_t* closest, float* winding, int32_t* flag,
                 void* ws, size_t ws_bytes, ldm_stream_t s);
/* Host: the two constants of the summation shape and the launch form. */
int ldm_mesh_sdf_face_chunk(void);
int64_t ldm_mesh_sdf_split_below(void);

/* ---- nearest points and Chamfer distances (additive in ABI 7) ------------- */
/* Clouds are fp32 [.][3].  Every point pair is evaluated, as dx = a.x - b.x (dy, dz alike),
 * d = dx dx, d = fma(dy, dy, d), d = fma(dz, dz, d): squared distances, |d - exact| <= 5 u d.
 * Coordinates must be finite: the minimum drops a NaN, so the kernels cannot be relied on to
 * propagate one; excluding them is the caller's.
 *
 * ldm_nearest_points: for q [P][3] against c [Q][3],
 *   d2   [P]  min_j |q_i - c_j|^2
 *   idx  [P]  (or NULL) the j of that minimum, the smaller index on a tie
 * ldm_chamfer_matrix: for a [S][n][3] against b [R][m][3],
 *   out  [S][R]  D(a_s -> b_r) = (1 / n) sum_i min_j |a_si - b_rj|^2: the n minima (bitwise those
 *                of ldm_nearest_points) added in fp64 in an order fixed by n and
 *                ldm_chamfer_tile_a() alone, then fl32(sum / n)
 * The other direction is the same call with the arguments swapped.  out[s][r] is a pure
 * function of (a_s, b_r), bitwise: the same for any S and R, at any position, from run to run.
 * P == 0, S == 0 or R == 0 return 0 with nothing written.  LDM_EINVAL for a NULL pointer, a
 * negative count, Q == 0 / n == 0 / m == 0 with work to do, and a grid beyond the launch limits
 * (Q, n or m above 2^31 - 1; S x R above 2^31 - 1; P above (2^31 - 1) ldm_chamfer_tile_a());
 * LDM_EALIGN for tensors off 4 B or a workspace off 256 B; LDM_ENOSPC for a short workspace.
 * ws: 256-byte aligned, ldm_nearest_points_ws_bytes(P, Q) / ldm_chamfer_ws_bytes(S, n, R, m)
 * bytes (0 for arguments the call refuses); bounded by the tiling, never S x R x n. */
size_t ldm_nearest_points_ws_bytes(int64_t P, int64_t Q);
int ldm_nearest_points(const float* q, int64_t P, const float* c, int64_t Q, float* d2,
                       int32_t* idx, void* ws, size_t ws_bytes, ldm_stream_t s);
size_t ldm_chamfer_ws_bytes(int64_t S, int64_t n, int64_t R, int64_t m);
int ldm_chamfer_matrix(const float* a, int64_t S, int64_t n, const float* b, int64_t R,
                       int64_t m, float* out, void* ws, size_t ws_bytes, ldm_stream_t s);
/* Host: points of the first cloud per workgroup tile; points of the second cloud per split
 * unit; P below which ldm_nearest_points splits the second cloud over workgroups (with more than
 * one unit of it); S x R below which ldm_chamfer_matrix spreads one entry over workgroups (with
 * more than one tile of n). */
int ldm_chamfer_tile_a(void);
int ldm_chamfer_chunk_b(void);
int64_t ldm_chamfer_split_below(void);
int64_t ldm_chamfer_spread_below(void);

/* ---- earth mover's distance (additive in ABI 7) ---------------------------- */
/* For clouds of the same size n (fp32 [.][n][3], finite coordinates: the caller's to ensure),
 *   EMD(a, b) = (1 / n) min over permutations pi of sum_i |a_i - b_pi(i)|        (Euclidean).
 * The pair distance is the squared distance of the Chamfer calls (same operation sequence)
 * followed by one square root of at most 1 ulp (v_sqrt_f32): |d - exact| <= 5 u |exact|,
 * u = 2^-24 (the 5 u of d^2 halve under the root, which adds up to 2 u of its own).
 *
 * ldm_emd_matrix runs an eps-scaled Jacobi auction per entry, one workgroup each, and returns a
 * real assignment.  With cost = (1 / n) sum_i |a_i - b_pi(i)| in exact arithmetic,
 *   EMD <= cost <= EMD + eps + ldm_emd_slack(extent)
 * (eps-complementary slackness; the slack is what fp32 rounding of values and bids adds, see
 * below).  out [S][R] = fl32(sum of the n fp32 pair distances, added in fp64 in an order fixed by
 * n alone, / n): within 6 u of cost.  An entry is a pure function of (a_s, b_r, eps), bitwise:
 * the same for any S and R, at any position, from run to run.
 *   eps          > 0: the bound above, in the units of the coordinates
 *   extent       an upper bound of the bounding-box diagonal of every pair (a_s with b_r) the
 *                caller vouches for; an entry whose own diagonal is larger is not computed
 *   max_rounds   most auction rounds per entry; 0: ldm_emd_default_max_rounds(n)
 *   within       nonzero: b == a and R == S; only s < r is computed, mirrored into r > s (the
 *                assignment inverted), and the diagonal is an exact 0 with the identity
 *   assign       [S][R][n] int32 or NULL: pi, the index into b_r that point i of a_s is matched to
 *   rounds       [S][R] int32 or NULL: auction rounds the entry took
 *   unconverged  one int32 or NULL: set to the number of entries not computed: round cap hit,
 *                extent above the bound, or a bid outside (price, 8 extent + 4 eps].  Such an
 *                entry is NaN in out and -1 throughout assign; the launch still ends.
 * The slack: values d + price and bids are rounded to fp32, which loosens eps-complementary
 * slackness by at most 5 u (extent + largest price) per pair; the kernel holds prices to
 * 8 extent + 4 eps, and the fp32 distances move both costs by at most 5 u extent each:
 * ldm_emd_slack(extent) = 55 u extent.  ldm_emd_min_eps(extent) = 8 ldm_emd_slack(extent) is the
 * smallest eps the call accepts, so that the slack stays under eps / 8.
 * S == 0 or R == 0 return 0 with nothing written.  LDM_EINVAL for a NULL a / b / out / ws, a
 * negative count, n == 0 with work to do, S x R above 2^31 - 1, within without b == a and
 * R == S, an extent that is negative or not finite, eps not positive, not finite or below the
 * floor, max_rounds outside [0, 2^31 - 1]; LDM_ENOSYS for n above ldm_emd_max_points();
 * LDM_EALIGN for tensors off 4 B or a workspace off 256 B; LDM_ENOSPC for a short workspace.
 * Every refusal happens before any device work.  ws: 256-byte aligned, ldm_emd_ws_bytes(S, R, n)
 * bytes (0 for negative or oversized counts); it holds the count when unconverged is NULL. */
size_t ldm_emd_ws_bytes(int64_t S, int64_t R, int64_t n);
int ldm_emd_matrix(const float* a, int64_t S, const float* b, int64_t R, int64_t n, float eps,
                   float extent, int64_t max_rounds, int within, float* out, int32_t* assign,
                   int32_t* rounds, int32_t* unconverged, void* ws, size_t ws_bytes,
                   ldm_stream_t s);
int64_t ldm_emd_max_points(void);
double ldm_emd_slack(double extent);
double ldm_emd_min_eps(double extent);
int64_t ldm_emd_default_max_rounds(int64_t n); /* 0 for n outside [1, ldm_emd_max_points()] */

/* ---- ray casting against a mesh (additive in ABI 7) ------------------------ */
/* For R rays origins [R][3], dirs [R][3] (fp32; a direction need not be unit) against the
 * triangle soup verts fp32 [V][3], faces int32 [F][3], every ray-triangle pair evaluated with
 * the watertight test of Woop, Benthin and Wald in plain fp32 (csrc/ray_tri_pair.h: no fused
 * multiply-add, true divisions; a ray through a shared edge or vertex of a closed mesh hits
 * one of the triangles around it):
 *   t_out    [R]     the smallest t in [t_min, t_max] with origin + t dir on a triangle (both
 *                    sides of a triangle count); +inf for a miss
 *   face_out [R]     (or NULL) index of that triangle, the smaller index on a tie; -1 for a miss
 *   bary_out [R][3]  (or NULL) the weights of the triangle's three vertices at the hit, 0 for a
 *                    miss
 * A ray whose dominant direction component is 0 or not finite, or whose origin is not finite,
 * misses everything.  A ray's outputs are a pure function of the ray, the mesh and the bounds:
 * bitwise the same alone or in any batch, and from run to run.  F == 0 gives all misses;
 * R == 0 returns 0 with nothing written.
 * A face index outside [0, V) is never read through: it is clamped, and the device word *flag
 * (zeroed by the call) is set to 1 -- the outputs are then meaningless.
 * ws: 256-byte aligned, ldm_ray_mesh_ws_bytes(F, R) bytes (0 for negative sizes); it holds the
 * packed triangles and, below ldm_ray_mesh_split_below() rays with more than one chunk of
 * ldm_ray_mesh_face_chunk() faces, one tile of per-chunk partials.
 * LDM_EINVAL for a NULL verts / faces (with F > 0) / origins / dirs / t_out / flag / ws, a
 * negative count, t_min > t_max or a NaN bound, and a grid beyond the launch limits: more than
 * 65535 chunks of faces in the split form, more than 2^31 - 1 workgroups of 256 rays in the
 * other.  LDM_EALIGN for tensors off 4 B or a workspace off 256 B; LDM_ENOSPC for a short
 * workspace.  Every refusal happens before any device work. */
size_t ldm_ray_mesh_ws_bytes(int F, int64_t R);
int ldm_ray_mesh(const float* verts, int V, const int32_t* faces, int F, const float* origins,
                 const float* dirs, int64_t R, float t_min, float t_max, float* t_out,
                 int32_t* face_out, float* bary_out, int32_t* flag, void* ws, size_t ws_bytes,
                 ldm_stream_t s);
/* Host: faces per workgroup of the split form, and the R below which it is used. */
int ldm_ray_mesh_face_chunk(void);
int64_t ldm_ray_mesh_split_below(void);

/* ---- sphere tracing of the decoder's field (additive in ABI 7) ------------- */
/* The passes between two decoder evaluations of a sphere tracer; the loop over rounds is the
 * caller's (ldm_sdf/render.py trace_sdf), and every evaluation is one ldm_decoder_points_fwd
 * over the whole batch.  B shapes, R rays each: origins / dirs fp32 [R][3] shared by the shapes
 * (per_shape == 0) or [B][R][3] (per_shape != 0); a direction need not be unit and t is in
 * units of it.  The geometry is csrc/ray_brick_dda.h in plain fp32, a fixed operation order, no
 * fused multiply-add: a ray's outputs are a pure function of the ray, its values and the
 * parameters, bitwise the same alone or in any batch.  State, all caller-owned:
 *   t        [B][R]     the ray's current t; +inf once it has missed
 *   status   [B][R]     0 miss, 1 hit (at t), 2 still marching
 *   steps    [B][R]     decoder evaluations the ray has taken
 *   xyz_last [B][R][3]  (or NULL) the point the ray was last evaluated at, NaN for none
 *   list     [B][R]     per shape the first counts[b] entries: the marching rays, ascending
 *   counts   [B]        the caller reads these back once per round
 * ldm_sdf_trace_init: a ray with a non-finite origin or a zero or non-finite direction
 * misses; else it is slab-clipped against [lo, hi]^3 and [t_min, t_max], and it starts at the
 * near end.  With mask != NULL -- brick flags [B nb^3] for an N^3 grid of voxel size vs over
 * the box: ldm_band_classify's `active`, to which a caller adds the inactive bricks that lie
 * inside the shape, where a ray must not be carried on -- it starts at its entry into the first
 * flagged brick (brick
 * boundaries: the lattice coordinates of ldm_band_lattice_coords, the thinner last brick
 * included), or misses.  level, lipschitz, eps and max_steps are only checked here, so that a
 * march is refused before its first round.
 * ldm_sdf_trace_emit: xyz [B][P][3] = the points origin + t dir of the listed rays, P >= the
 * largest count; a shorter shape's remaining slots repeat its last listed point (lo, lo, lo
 * for a shape with none).
 * ldm_sdf_trace_step: vals [B][P] the decoder's values at those points.  f = v - level:
 * f <= eps or f not finite is a hit at the current t; else t += max(f, eps) / (lipschitz |dir|),
 * with a mask then forward through inactive bricks to the next active one, past the ray's far
 * end a miss.  list and counts are rewritten for the next round.
 * LDM_EINVAL for a NULL required pointer, B < 1, R < 1, B R above 2^31 - 1, more than 65535
 * shapes or chunks of 4096 rays, P outside [1, R], a box that is not finite with lo < hi,
 * t_min > t_max or a NaN bound, eps or lipschitz not positive and finite, a NaN level,
 * max_steps < 1, and with a mask N < 2, B nb^3 above 2^31 - 1 or vs not positive; LDM_EALIGN
 * for tensors off 4 B or a workspace off 256 B; LDM_ENOSPC for a workspace below
 * ldm_sdf_trace_ws_bytes(B, R) (0 for sizes the calls refuse).  Every refusal happens before
 * any device work. */
size_t ldm_sdf_trace_ws_bytes(int B, int64_t R);
int ldm_sdf_trace_init(const float* origins, const float* dirs, int per_shape, int B, int64_t R,
                       float lo, float hi, float t_min, float t_max, float level,
                       float lipschitz, float eps, int max_steps, const uint8_t* mask, int N,
                       float vs, float* t, int32_t* status, int32_t* steps, float* xyz_last,
                       int32_t* list, int32_t* counts, void* ws, size_t ws_bytes,
                       ldm_stream_t s);
int ldm_sdf_trace_emit(const float* origins, const float* dirs, int per_shape, int B, int64_t R,
                       int P, float lo, const float* t, const int32_t* list,
                       const int32_t* counts, float* xyz, ldm_stream_t s);
int ldm_sdf_trace_step(const float* origins, const float* dirs, int per_shape, int B, int64_t R,
                       int P, const float* vals, float lo, float level, float lipschitz,
                       float eps, const uint8_t* mask, int N, float vs, float* t,
                       int32_t* status, int32_t* steps, float* xyz_last, int32_t* list,
                       int32_t* counts, void* ws, size_t ws_bytes, ldm_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* LDM_SDF_H */
