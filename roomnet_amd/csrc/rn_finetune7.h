// Stage 7 of a depth-3 fine-tuning step (rn_finetune7.hip), as rn_finetune.hip launches it.
#pragma once
#include "rn_internal.h"
#include "rn_lastblock.h"

constexpr int FT7_W = 9 * rnk::LB_CIN7 * rnk::LB_C;   // floats of conv 7's kernel (and of one weight-gradient partial)

struct Ft7Args {
    const float* feats;              // the resident cache [n_items, S6, S6, 128]
    const int32_t* index;            // item of minibatch slot b = index[base + b]; null: base + b
    int64_t base;
    int S6, C7, S7;
    const float* P;                  // master parameters: conv 7's kernel HWIO, its BN's gamma and beta
    int o_w7, o_g7, o_b7;
    const float* F;                  // frozen [mean | rsqrt(var + eps)] of stage 7's BN
    int f_bn7;
    float* pre;                      // [batch, C7, C7, 16] conv 7's pre-activation; the backward pass turns it into dL/dconv7 in place
    float* xh7;                      // [batch, S7, S7, 16] the normalised pooled value, before gamma and beta
    float* x7;                       // [batch, S7, S7, 16] s7.bn of the step: what the item kernel reads
    const float* dpool;              // [batch, S7, S7, 16] dL/dpool7, written by the item kernel
    float* part;                     // [batch, bands_b, FT7_W] weight-gradient partials
    int bands_f, rows_f;             // forward: bands of rows_f pooled rows
    int bands_b, rows_b;             // backward: bands of rows_b conv rows
};

// the band counts of a minibatch of `batch` items: a function of the geometry and the batch size alone
void rn_ft7_bands(int batch, int C7, int S7, int* bands_f, int* rows_f, int* bands_b, int* rows_b);
// null, or why this geometry is refused
const char* rn_ft7_geometry_reason(int S6, int C7, int S7);
int rn_ft7_forward(hipStream_t stream, const Ft7Args& a, int batch);
int rn_ft7_backward(hipStream_t stream, const Ft7Args& a, int batch);
