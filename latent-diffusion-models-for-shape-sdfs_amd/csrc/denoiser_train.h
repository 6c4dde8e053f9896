// What crosses the training step's translation units (internal, not part of the ABI):
// denoiser_train.hip (the launch-path step and its C entry points), adamw_multi.hip (the
// multi-tensor AdamW) and train_dag_build.hip (the host builder of the one-launch step's table).
#pragma once
#include "ldm_internal.h"
#include "train_dag.h"

#include <vector>

namespace ldm {

typedef unsigned short bf16_t;

// The step's workspace (denoiser_train.hip layout()): the operands of every product in bf16, in
// both layouts, the fp32 activations and epilogue partials, the DAG step's table and sync words.
struct TrainWs {
    int B, Bp, D, H, TE, nb;
    bf16_t *xt_b, *xt_T, *e_b, *e_T, *u_b, *u_T, *temb_b, *temb_T;
    bf16_t *h_b[LDM_MAX_BLOCKS + 1], *h_T[LDM_MAX_BLOCKS + 1];
    bf16_t *g_b[LDM_MAX_BLOCKS], *g_T[LDM_MAX_BLOCKS];
    bf16_t *go_b, *go_T, *dtemb_b, *dtemb_T, *gt_T, *dh0_b, *dh0_T;
    float *a_t, *h_f[LDM_MAX_BLOCKS], *a_f[LDM_MAX_BLOCKS], *dh[2];
    float *p_bt1, *p_bt2, *p_bin, *p_bblk[LDM_MAX_BLOCKS], *p_bout, *loss_part;
    dag::Table* dag_table;      // the persistent step's job table (train_dag.h) and sync words
    unsigned* dag_sync;
    size_t bytes;
};

TrainWs layout(const ldm_denoiser_t* w, int B, void* base);

// With a recorder the launches are not made but recorded, one group per launch (build_dag).
struct Recorder {
    std::vector<ldm_gemm_args_t> launches;
};

int check_desc(const ldm_denoiser_t* w, int B, bool bwd);
int check_grads(const ldm_denoiser_t* w, const ldm_denoiser_grads_t* g);
// the launch path's GEMMs (denoiser_train.hip); with a recorder, the DAG builder's record of them
struct StepHook;
int forward(const ldm_denoiser_t* w, const TrainWs& L, const float* eps_target,
            float* eps_out, float loss_scale, hipStream_t s, Recorder* rec = nullptr);
int backward(const ldm_denoiser_t* w, const TrainWs& L, const ldm_denoiser_grads_t* gr,
             float* dx, hipStream_t s, const StepHook* hook = nullptr, Recorder* rec = nullptr);

// adamw_multi.hip
void adamw_hyper(double lr, double beta1, double beta2, double eps, double weight_decay,
                 int step, float* o);
int adamw_launch(const ldm_adamw_tensor_t* const* list, int n, double lr, double beta1,
                 double beta2, double eps, double weight_decay, int step, hipStream_t s,
                 int grid_cap = 0, const float* d_hyper = nullptr);

// ldm_train_step_config's per-device state (denoiser_train.hip)
struct TrainCfg {
    int form = LDM_TRAIN_AUTO;
    unsigned spin = 0;
    int last = 0;
    unsigned dbg = 0;           // ldm_dev_train_dag_flags (diagnostics only)
};
TrainCfg& train_cfg();

// train_dag_build.hip
bool dag_auto(int B);
int dag_step(const ldm_denoiser_t* w, const ldm_sched_t* sc, const float* x0, const float* eps,
             const int32_t* t, int B, void* saved, const ldm_denoiser_grads_t* grads,
             float* loss_out, const ldm_adamw_tensor_t* tensors, int n, const float* hy7,
             const float* d_hyper, unsigned spin, unsigned dbg, hipStream_t s);
void dag_forget(const void* table);   // drop the host's record of the table uploaded there

}  // namespace ldm
