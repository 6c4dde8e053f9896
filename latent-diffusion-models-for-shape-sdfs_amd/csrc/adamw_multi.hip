// Multi-tensor AdamW (ldm_adamw_multi; the optimizer of the launch-path training step).
// One launch over every tensor: 64 x 64 tiles (a 1-D tensor is one row), each thread 4 rows x
// 4 consecutive columns.  The update is ldm_adamw_step's, operation for operation (denoiser.hip
// adamw_kernel), so both give the same bits.  The transposed bf16 copy goes through an LDS tile
// so its stores are 32-byte row runs.
#include "denoiser_train.h"
#include "adamw_tile.h"

#include <math.h>
#include <string.h>

namespace ldm {
namespace {
struct AdamJobs {
    ldm_adamw_tensor_t t[LDM_ADAMW_MAX_TENSORS];
    int first[LDM_ADAMW_MAX_TENSORS + 1];
    int n;
    float decay, omb1, b2, omb2, eps, step_size, bc2_sqrt;
    const float* dh;    // non-null: the 7 scalars above are read from device memory instead
};

typedef const __attribute__((address_space(4))) AdamJobs KJobs;

__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamJobs jobs) {
    typedef KJobs KJ;
    KJ* kj = (KJ*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ unsigned short sT[64][64 + 8];
    // grid-stride over the tiles: a capped grid leaves wave slots free on every CU for work on
    // another stream (ldm_denoiser_train_step_adamw); uncapped, one tile per workgroup
    for (int tile = blockIdx.x; tile < kj->first[kj->n]; tile += gridDim.x) {
        __syncthreads();                   // the previous tile's transposed reads of sT are done
        int j = 0;
        for (int i = 1; i < kj->n; ++i)
            if (tile >= kj->first[i]) j = i;
        const float* dh = kj->dh;
        const AdamHyper hy = {dh ? dh[0] : kj->decay, dh ? dh[1] : kj->omb1,
                              dh ? dh[2] : kj->b2,    dh ? dh[3] : kj->omb2,
                              dh ? dh[4] : kj->eps,   dh ? dh[5] : kj->step_size,
                              dh ? dh[6] : kj->bc2_sqrt};
        adamw_tile(kj->t[j], hy, sT, tile - kj->first[j]);
    }
}
}  // namespace

// The update's scalars, derived in double and rounded once, as ldm_adamw_step (and torch) do:
// [decay, 1 - beta1, beta2, 1 - beta2, eps, lr / bc1, sqrt(bc2)].
void adamw_hyper(double lr, double beta1, double beta2, double eps, double weight_decay,
                 int step, float* o) {
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    o[0] = (float)(1.0 - lr * weight_decay);
    o[1] = (float)(1.0 - beta1);
    o[2] = (float)beta2;
    o[3] = (float)(1.0 - beta2);
    o[4] = (float)eps;
    o[5] = (float)(lr / bc1);
    o[6] = (float)sqrt(bc2);
}

// One adamw_multi_kernel launch over the tensors list[0..n) (host descriptors); d_hyper
// (optional): device copy of adamw_hyper's 7 scalars, read by the kernel instead (a captured
// graph then replays with new step counts).
int adamw_launch(const ldm_adamw_tensor_t* const* list, int n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, hipStream_t s,
                 int grid_cap, const float* d_hyper) {
    if (n == 0) return 0;
    AdamJobs J;
    memset(&J, 0, sizeof(J));
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        const ldm_adamw_tensor_t& T = *list[i];
        LDM_REQUIRE(T.p && T.g && T.m && T.v && T.rows >= 1 && T.cols >= 1, LDM_EINVAL,
                    "ldm_adamw_multi: tensor %d incomplete", i);
        J.t[i] = T;
        J.first[i] = tiles;
        tiles += ((T.rows + 63) / 64) * ((T.cols + 63) / 64);
    }
    J.first[n] = tiles;
    J.n = n;
    float h[7];
    adamw_hyper(lr, beta1, beta2, eps, weight_decay, step, h);
    J.decay = h[0]; J.omb1 = h[1]; J.b2 = h[2]; J.omb2 = h[3]; J.eps = h[4];
    J.step_size = h[5]; J.bc2_sqrt = h[6];
    J.dh = d_hyper;
    const int grid = grid_cap > 0 && grid_cap < tiles ? grid_cap : tiles;
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(grid), dim3(256), 0, s, J);
    return launch_status("ldm_adamw_multi");
}
}  // namespace ldm

using namespace ldm;

extern "C" int ldm_adamw_multi(const ldm_adamw_tensor_t* tensors, int n, double lr,
                               double beta1, double beta2, double eps, double weight_decay,
                               int step, ldm_stream_t s) {
    LDM_REQUIRE(tensors && n >= 1 && n <= LDM_ADAMW_MAX_TENSORS && step >= 1, LDM_EINVAL,
                "ldm_adamw_multi: 1..%d tensors, step >= 1", LDM_ADAMW_MAX_TENSORS);
    const ldm_adamw_tensor_t* list[LDM_ADAMW_MAX_TENSORS];
    for (int i = 0; i < n; ++i) list[i] = &tensors[i];
    return adamw_launch(list, n, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)s);
}

extern "C" void ldm_adamw_hyper(double lr, double beta1, double beta2, double eps,
                                double weight_decay, int step, float* out7) {
    ldm::adamw_hyper(lr, beta1, beta2, eps, weight_decay, step, out7);
}
