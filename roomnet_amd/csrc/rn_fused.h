// Fused 16-bit (bf16 / fp16 storage, fp32 accumulate) MFMA execution path.
#pragma once
#include <vector>
#include "rn_bands.h"
#include "rn_internal.h"
#include "rn_stage.h"

// Pack weights into MFMA fragment order, choose per-stage launch geometry.
int rn_fused_prepare(rn_handle* h, const rn_weights* w);
// Enqueue the fused forward pass.  Exactly one of d_bgr / d_rgb is non-null.
int rn_fused_forward(rn_handle* h, const uint8_t* d_bgr, const float* d_rgb, int n, float* d_probs,
                     int64_t* d_ids);
void rn_fused_release(rn_handle* h);
// the stage under which the launch that computes `stage` reports its time (== stage for a launch of its own)
int rn_fused_launch_rep(const rn_handle* h, int stage);
// the stage's output tensor is never written to HBM on this handle (it only exists in LDS inside a fused launch)
bool rn_fused_stage_elided(const rn_handle* h, int stage);
void rn_fused_frozen_info(const rn_handle* h, int info[4]);
// constant channels nobody computes (round 6): info = {stage whose last cout quarter is constant in the handle's 16-bit store or -1,
// channels of it proven constant, channels folded (16), input channels the stage behind it still contracts (48)}
void rn_fused_const_info(const rn_handle* h, int info[4]);
// after the activation buffers exist: fill the constant channels once
int rn_fused_post_alloc(rn_handle* h);
// head launcher shared with the unfused path (defined in rn_api.hip)
int rn_run_head(rn_handle* h, int n, float* d_probs, int64_t* d_ids);
void rn_record_event(rn_handle* h, int idx);
void rn_fill_head_args(rn_handle* h, HeadArgs* a);

// ---- the last two conv stages + flatten + dense head + softmax/argmax in one launch (rn_tail.hip)
bool rn_tail_supported(const rn_handle* h);
int rn_tail_launch(rn_handle* h, const rnk::i32x4* wfrag_a, const rnk::i32x4* wfrag_b, const HeadArgs& head, int n, float* d_probs,
                   int64_t* d_ids);

// ---- the generic family (rn_generic.hip): stage_mfma_kernel, one variant per stage shape, and stage 0 as a launch of its own
struct GenericPlan {
    int variant = -1;        // index into the dispatch table
    int npt = 1;             // pixel tiles (= waves) per workgroup
    int n_colblocks = 1;
    int n_ctg = 1;           // workgroups the cout tiles are split over
    size_t lds_bytes = 0;    // (above 160 KB with npt == 1: the stage does not fit)
};
bool rn_generic_plan(int cin, int cout, int pool_k, int pool_s, bool res, int out_side, GenericPlan* plan);    // false: no variant
void rn_generic_pack(const float* w_hwio, int cin, int cout, int dtype, std::vector<unsigned short>* out);
int rn_generic_launch(const GenericPlan& p, int dtype, hipStream_t s, const rnk::StageArgs& a, int n);
int rn_stage0_launch(int dtype, hipStream_t s, const rnk::Stage0Args& a, int n);

// ---- register-weights stage kernels (rn_stage_rw.hip)
struct RwPlan {
    int variant = -1;
    int npt = 0;
    int n_colblocks = 0;
    int skipcols = 0;
    size_t lds_bytes = 0;
    bool wide = false;       // stride-2 pooling on wide tiles (15 windows per tile) instead of gapped ones (14)
    int wgs_per_cu = 1;      // workgroups of this variant resident on one CU (register / LDS budget of the instantiation)
};
bool rn_rw_supported(int cin, int cout, int pool_k, int pool_s, bool res, int out_side, int skip_side,
                     RwPlan* plan);
int rn_rw_launch(const RwPlan& p, int dtype, hipStream_t s, const rnk::StageArgs& a, dim3 grid);
int rn_rw_s0sh_colblocks(int out_side);      // column blocks (227 wide) of the shared-ring stage 0 + 1 kernel

// ---- cross-stage fused pair: conv-pool-BN -> conv-pool-BN + residual of a depth-3 block.  rn_stage23.hip (32x32x16 tiles, the
// round-2 form: test / A-B library only) and rn_stage23x.hip (16x16x32 tiles) take the same launch arguments and column blocks
bool rn_stage23_supported(int in_side);
bool rn_stage23_plan(int in_side, int* n_cblocks, int* x0, int* wo);   // column blocks (x0, wo: 4 entries)
int rn_stage23_launch(int dtype, hipStream_t s, const rnk::Stage23Args& a, int n);
// rn_stage23x.hip: own weight fragment order
void rn_stage23x_pack(const float* w_hwio, int dtype, std::vector<unsigned short>* out);
void rn_stage23x_pack_narrow(const float* w_hwio, const int* ring_cin, int dtype, std::vector<unsigned short>* out);
void rn_stage23x_pack_narrow8(const float* w_hwio, const int* ring_cin, int dtype, std::vector<unsigned short>* out);
int rn_stage23x_launch(int dtype, hipStream_t s, const rnk::Stage23Args& a, int n);

// ---- 16x16x32 matrix tiles (weight fragments: rn_pack.h) without row-register blocking (rn_conv16.hip): the un-pooled 64 -> 128 stage ...
bool rn_conv16_supported(int cin, int cout, int pool_k, bool res);
int rn_conv16_colblocks(int out_side);
int rn_conv16_launch(int dtype, hipStream_t s, const rnk::Conv16Args& a, int n);
// ... and the 128 -> 16 stage with avg-pool 4/2 (one wave = one 16-pixel tile x all 16 couts, no K split)
bool rn_conv16p_supported(int cin, int cout, int pool_k, int pool_s, bool res);
int rn_conv16p_colblocks(int out_side);
int rn_conv16p_wgs_per_cu(int out_side);
int rn_conv16p_launch(int dtype, hipStream_t s, const rnk::Conv16Args& a, int n);

// ---- 16x16x32 tiles with row-register blocking (shared device pieces: rn_rowreg.h).  rn_stage4x.hip: the 32 -> 64 stage with pool 4/2
bool rn_stage4x_supported(int cin, int cout, int pool_k, int pool_s, bool res, int in_side);
bool rn_stage4x_plan(int out_side, int* n_cb, int* xo0, int* wo);       // column blocks (xo0, wo: 4 entries)
int rn_stage4x_launch(int dtype, hipStream_t s, const rnk::StageArgs& a, int n);
// rn_stage5x.hip: the 64 -> 64 residual stage with pool 4/2
bool rn_stage5x_supported(int cin, int cout, int pool_k, int pool_s, bool res, int in_side, int skip_side);
bool rn_stage5x_plan(int out_side, int* n_cb, int* xo0, int* wo);
int rn_stage5x_launch(int dtype, hipStream_t s, const rnk::StageArgs& a, int n);
// rn_stage6x.hip: the un-pooled 64 -> 128 stage
bool rn_stage6x_supported(int cin, int cout, int pool_k, bool res, int in_side);
bool rn_stage6x_plan(int out_side, int* n_cb, int* xo0, int* wo);
int rn_stage6x_launch(int dtype, hipStream_t s, const rnk::StageArgs& a, int n);

// ---- float32 conv stages on the matrix cores (rn_stage_f32m.hip): the throughput path of RN_DTYPE_F32 handles without RN_FLAG_TAPS
// The frozen-channel folds rn_create proposes for a float32 handle, found on the caller's weights and applied to the copy `rw`
// in front of everything that uploads weights: the stage each applies to (-1: none) and its channel relabelling
struct F32Folds {
    int fold_r = -1;                 // the 64 -> 64 residual stage whose second 32-cout tile is all frozen
    std::vector<int> fold_pi;
    int kfold_r = -1;                // the stage whose last input channels are frozen
    std::vector<int> kfold_pi;
    int kfold_live = 0, kfold_proven = 0;
};
F32Folds rn_f32m_plan_folds(const rn_weights* w, int dtype, unsigned flags, RelabelledWeights* rw);
// plans every stage, keeps what the handle really folds, uploads; registers the folds' relabellings in rn_handle::node_perm
int rn_f32m_prepare(rn_handle* h, const rn_weights* w, const F32Folds& folds);
// after the activation buffers exist: every launch argument but the bands
int rn_f32m_post_alloc(rn_handle* h);
void rn_f32m_release(rn_handle* h);
bool rn_f32m_covers(const rn_handle* h, int stage);
int rn_f32m_launch(rn_handle* h, int stage, int n);      // reads the output node of stage - 1, writes the stage's
void rn_f32m_frozen_info(const rn_handle* h, int info[4]);

// ---- the back end in one launch: stage 6 -> 7 -> 8 -> 9 -> head (rn_backend.hip)
bool rn_backend_supported(const rn_handle* h);
int rn_backend_launch(rn_handle* h, const rnk::i32x4* wfrag6, const float* ptab6, const float* cstart6, const rnk::i32x4* wfrag7,
                      const float* ptab7, const rnk::i32x4* wfrag_a, const rnk::i32x4* wfrag_b, const HeadArgs& head, int n, float* d_probs,
                      int64_t* d_ids);
