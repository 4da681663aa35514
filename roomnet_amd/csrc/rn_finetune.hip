// Fine-tuning of the last two conv stages and the dense head on cached features (rn_ft_*), and the feature read-out that fills
// the cache (rn_features_*).
//
// Frozen: stages 0-7.  Everything behind x7 = s7.bn depends on x7 alone (stage 9's skip starts there), so a training set is a
// resident float32 array [n_items, S7, S7, 16] and a step never runs the trunk.
//
// Trained variables, in this order (checkpoint names; 19 for the reference graph): conv 8's kernel, its BN's gamma and beta; conv 9's
// kernel, its BN's gamma and beta, gamma and beta of the BN behind the residual add; per dense block its kernel and its BN's gamma and
// beta; the last dense layer's kernel and bias.  moving_mean / moving_variance are read and never written: every BN is the inference
// BN y = (x - mean) rsqrt(var + eps) gamma + beta with trainable gamma and beta (the reference's shipped training configuration,
// train.py:40-41: COMPUTE_BN_MEAN_VAR = False, UPDATE_BATCHNORM_MOVING_VARS = False).  Dropout only where
// rn_ft_set_dropout switches it on (rn_dropout.h: the generator and the sites; the end of this header: where it enters a step).
//
// Forward, per item, float32:  stage 8 (conv 3x3 VALID -> ReLU6 -> avg-pool 4/2 -> BN), stage 9 (the same, + legacy-bilinear
// resize of x7 -> add -> BN), flatten, dense blocks x @ W [+ b] -> ReLU6 -> [BN]; the last block's ReLU6 is applied to the logits
// as well (network.py:237, dense_block): r = relu6(z).
// Loss (network.py:56-59):  L = mean_i CE(softmax(r_i), y_i) + l2_coeff * sum_v sum(v^2) / 2 over the TRAINED variables; the
// frozen variables' share of the reference's regulariser is a constant the gradient does not see and is left out.
// Gradients, TensorFlow's rules as rn_gradcam.hip states them: Relu6Grad passes strictly inside (0, 6) -- here the last ReLU6 is on the
// path: dL/dz = (softmax - onehot) where 0 < z < 6 --, AvgPool spreads g / 16 over each window, Add feeds both inputs (the resize
// branch ends in x7: no gradient is needed there), BN: d gamma = sum g (x - mean) rsqrt(var + eps), d beta = sum g,
// dx = g gamma rsqrt(var + eps); conv: dW[ky, kx, ci, co] = sum_p in[p + k, ci] dconv[p, co]; MatMul: dW = X^T G.
// Adam (tf.train.AdamOptimizer; slots zero at rn_ft_create), all float32 on the device:
//   g = dL/dv (L2 term included);  m += (g - m)(1 - beta1);  v += (g^2 - v)(1 - beta2);  var -= lr_t m / (sqrt(v) + eps)
//   lr_t = lr(step) sqrt(1 - beta2^t) / (1 - beta1^t),  lr(step) = learn_rate * decay_rate^(step / num_steps)  (network.py:36, no
//   staircase); step counts from start_step, t from 1 at the trainer's first step.  lr_t is formed on the host in float64 and
//   handed to the launch as one float32.
//
// Two launches per step, enqueued back to back on the trainer's stream (no graph capture; one synchronisation per rn_ft_run):
//   ft_item_kernel    one workgroup per item of the minibatch (the per-element steps of rn_lastblock.h, which gc_tail_kernel is built
//                     from as well, under this kernel's own loops and epilogues): conv weights and BN tables in LDS,
//                     intermediates in a per-item float32 workspace, the item's feature read from the resident cache through the
//                     index.  Forward, softmax and the item's CE term, then the adjoint; writes the item's partials of every
//                     gradient: dW8, dW9 (plain FMAs: 144 (tap, cin) pairs x 3 row groups of threads, 16 cout accumulators each,
//                     one conv row summed apart before it joins the total), the BN d gamma / d beta terms, and for every dense
//                     layer its input vector and its output-gradient vector (no per-item outer products).  Workgroup 0 also sums
//                     v^2 over the parameters for the loss.
//   ft_update_kernel  one thread per parameter: sums the partials over the items in index order (dense kernels: X^T G over the
//                     items) -- no floating-point atomics, the same minibatch gives the same bits --, divides by n, adds
//                     l2_coeff v, applies Adam to the float32 master copy, keeps the gradient readable, and writes the step's loss
//                     (evaluated before the update) into its slot of a device array.
// rn_ft_eval runs the item kernel forward-only (loss, softmax, argmax) from the current master parameters.
// The loss's scalar sums (item CE terms, sum v^2, the log-sum-exp of num_classes values) are float64; everything else is float32.
//
// Depth.  The above is a trainer of depth 2 (rn_ft_create): two trained conv stages.  A trainer of depth 3 (rn_ft_create_depth)
// trains the whole last block: the feature is x6 = s6.bn [S6, S6, 128], stage 7's kernel, gamma and beta come in front of the list
// (22 variables), and a step is four launches; stage 7's mathematics and its two kernels are in rn_finetune7.hip:
//   ft7_fwd_kernel    x6 (through the index) -> x7 into a per-step workspace, with what the adjoint needs
//   ft_item_kernel    the depth-3 instantiation reads x7 from that workspace and goes on behind conv 8's weight gradient:
//                     g7 = dL/dx7 = conv 8's adjoint + the transpose of the skip resize (rn_lastblock.h), the item's
//                     d gamma7 = sum g7 xh7 and d beta7 = sum g7, and dL/dpool7 = g7 gamma7 rsqrt(var7 + eps) for the next launch
//   ft7_bwd_kernel    dL/dconv7 and one dW7 partial per (item, band)
//   ft_update_kernel  the depth-3 instantiation sums the dW7 partials over bands, then over items, in index order, in float64
// Both depths pass the same FtItemArgs / FtUpdateArgs: the depth-3 fields are null or zero at depth 2, and the one variable list has
// conv 7's three variables in front at depth 3.  The kernels are templates on the depth; the depth-2 instantiations run the code they
// always did.
//
// Dropout (rn_ft_set_dropout, rate > 0; a trainer at rate 0 launches exactly the above).  The item kernel's third template parameter
// DROP: fl is dropped where it is written (site 1), every hidden block's output behind its BN (site 2 + d), and the softmax, the CE
// term and the argmax read the dropped relu6(z) (site 2 + L).  Adjoint: dL/dz_j = keep_j scale (p_j - [j == y]) where 0 < z_j < 6;
// a hidden layer's dense adjoint is multiplied by keep scale BEFORE it feeds the d gamma / d beta partials and the ReLU6 mask; dL/dfl
// gets site 1's factor before stage 9.  The partials' input vectors are the dropped ones.  At depth 3 ft7_drop_kernel writes the
// minibatch's dropped s6.bn (site 0) in slot order in front of ft7_fwd_kernel: five launches.  rn_ft_eval never drops.
//
// Validation inside a run (rn_ft_run_validated; rn_ft_run is the same loop, ft_run_loop, with no points).  Behind every step the
// schedule names (ft_is_point) the resident validation set goes through the forward-only pass in chunks of max_batch, and on the
// device ft_val_chunk_kernel adds each chunk to the point's confusion matrix and float64 cross-entropy sum, ft_val_close_kernel
// writes the point's loss, counts the correct predictions and decides whether the point beats the best so far (strictly more
// correct), and ft_val_snapshot_kernel then copies the parameter slab aside.  Nothing is synchronised until the run's one read-back.
//
// Fresh views (rn_ft_run_views; rn_views.h).  The same loop with a per-step feature provider (FtFeed): in front of step s the
// handle's stream makes the minibatch's views at the trainer's global step (one launch, rn_imageops.hip) and runs the trunk's feature
// pass into one of FT_VIEW_SLOTS = 2 feature slots the trainer owns, taken in turn; an event lets the trainer's stream run the unchanged
// pass on that slot (index 0, 1, ...; labels gathered once per call in slot order by ft_gather_labels_kernel), and an event back keeps
// the handle from overwriting a slot before the pass that reads it is through.  With two slots the trunk pass of step s + 1 overlaps
// the trainer's step s (profiles/finetune_views_timing.json has the A/B against one slot); the bits do not depend on it.
#include "rn_dropout.h"
#include "rn_finetune7.h"
#include "rn_internal.h"
#include "rn_lastblock.h"
#include "rn_stage.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace rnk;

namespace {

constexpr int FT_NT = 512;           // threads of the item workgroup
constexpr int FT_W = 9 * LB_C * LB_C;
constexpr int FT_WG_PAIRS = 9 * LB_C;  // (tap, cin) pairs of a weight gradient
constexpr int FT_WG_GROUPS = 3;        // row groups (FT_WG_PAIRS * FT_WG_GROUPS <= FT_NT)
constexpr int FT_MAX_VARS = 11 + 3 * RN_MAX_DENSE;   // depth 3: conv 7's three in front
#ifndef FT_VIEW_SLOTS     // (measurement arm: csrc/build.sh RN_VARIANT_FLAGS=-DFT_VIEW_SLOTS=1 is rn_ft_run_views without the overlap)
#define FT_VIEW_SLOTS 2   // feature slots of rn_ft_run_views: the trunk pass of step s + 1 overlaps the trainer's step s
#endif

struct FtItemArgs {
    const float* feats;              // [n_items, S7, S7, 16] (depth 3: unused, the item kernel reads x7ws)
    const int32_t* labels;           // [n_items] (eval: may be null)
    const int32_t* index;            // item of workgroup b = index[base + b]; null: base + b
    int64_t base;
    int S7, C8, S8, C9, S9;
    const float* P;                  // master parameters
    const float* F;                  // frozen [mean | rsqrt(var + eps)] per BN
    int o_w8, o_g8, o_b8, o_w9, o_g9, o_b9, o_g9b, o_b9b;
    int f_bn8, f_bn9, f_bn9b;
    LbResize rs;                     // legacy bilinear tables S7 -> S9
    int n_dense, nc;
    int nin[RN_MAX_DENSE], nout[RN_MAX_DENSE];
    int o_dw[RN_MAX_DENSE], o_db[RN_MAX_DENSE], o_dg[RN_MAX_DENSE], o_dbeta[RN_MAX_DENSE], f_dbn[RN_MAX_DENSE];   // -1: absent
    float* ws;                       // per-workgroup workspace
    int64_t ws_item, off_c8, off_xh8, off_s8, off_gs8, off_c9, off_xh9, off_xh9b, off_fl, off_gfl;
    float* part;                     // per-workgroup partials record
    int64_t rec;
    int p_w8, p_w9, p_bn8, p_bn9, p_bn9b;
    int p_x[RN_MAX_DENSE], p_gz[RN_MAX_DENSE], p_dg[RN_MAX_DENSE], p_dbeta[RN_MAX_DENSE];
    double* item_loss;               // [batch] CE term of the workgroup's item
    double* l2sum;                   // sum v^2 over the parameter slab (workgroup 0; null: not wanted)
    int n_param;                     // floats of the parameter slab
    float* probs;                    // eval: [batch, nc], one chunk's staging (null in training)
    int64_t* ids;                    // eval: [batch]
    // depth 3 (null / zero at depth 2)
    const float* x7ws;               // [batch, S7, S7, 16] s7.bn of the step (ft7_fwd_kernel)
    const float* xh7;                // [batch, S7, S7, 16] its normalised value before gamma and beta
    float* dpool7;                   // [batch, S7, S7, 16] dL/dpool7 for ft7_bwd_kernel
    int64_t off_gadd;                // workspace: dL/d(stage 9's add), which the skip branch carries back to x7
    int o_g7, f_bn7, p_bn7;
    // dropout (read by the DROP instantiation alone)
    RnDropout drop;
};

// sum of `val` over the 32 threads that share channel tid & 15, in a fixed order; the result is valid for tid < 16
__device__ __forceinline__ float channel_sum(float val, float* red, int tid) {
    red[tid] = val;
    __syncthreads();
    float t = 0.f;
    if (tid < LB_C)
        for (int part = 0; part < FT_NT / LB_C; ++part) t += red[part * LB_C + tid];
    __syncthreads();
    return t;
}

// dW[k][ci][co] = sum_p in[p + k][ci] dout[p][co] over the Co x Co positions of a VALID 3x3 conv: in [S][S][16], dout [Co][Co][16]
// (both global float32), out [9][16][16].  Thread (pair, group): one (tap, cin) pair, conv rows group, group + 3, ...; every row is
// summed apart and then added to the total (two-level sum: the error grows with sqrt(Co) + sqrt(Co / 3), not with Co^2 / 3).
__device__ __forceinline__ void wgrad16(const float* in, int S, const float* dout, int Co, float* out, float* red3, int tid) {
    if (tid < FT_WG_PAIRS * FT_WG_GROUPS) {
        const int pair = tid % FT_WG_PAIRS, grp = tid / FT_WG_PAIRS;
        const int k = pair / LB_C, ci = pair % LB_C, ky = k / 3, kx = k % 3;
        float acc[LB_C];
#pragma unroll
        for (int q = 0; q < LB_C; ++q) acc[q] = 0.f;
        for (int y = grp; y < Co; y += FT_WG_GROUPS) {
            float row[LB_C];
#pragma unroll
            for (int q = 0; q < LB_C; ++q) row[q] = 0.f;
            const float* pin = in + (static_cast<int64_t>(y + ky) * S + kx) * LB_C + ci;
            const f32x4* pd = reinterpret_cast<const f32x4*>(dout + static_cast<int64_t>(y) * Co * LB_C);
            for (int x = 0; x < Co; ++x) {
                const float a = pin[x * LB_C];
#pragma unroll
                for (int c4 = 0; c4 < LB_C / 4; ++c4) {
                    const f32x4 d = pd[x * (LB_C / 4) + c4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) row[4 * c4 + q] = fmaf(a, d[q], row[4 * c4 + q]);
                }
            }
#pragma unroll
            for (int q = 0; q < LB_C; ++q) acc[q] += row[q];
        }
#pragma unroll
        for (int q = 0; q < LB_C; ++q) red3[grp * FT_W + pair * LB_C + q] = acc[q];
    }
    __syncthreads();
    for (int o = tid; o < FT_W; o += FT_NT) out[o] = (red3[o] + red3[FT_W + o]) + red3[2 * FT_W + o];
    __syncthreads();
}

// DROP (training only): dropout at sites 1 and 2 + d of rn_dropout.h, every mask bit recomputed from the generator where it is read.
// hx[0] (dense layer 0 reads fl) holds the dropped logits and hxh[L] (the last layer has no BN) their keep * scale.
template <bool TRAIN, bool D3, bool DROP = false>
__global__ __launch_bounds__(FT_NT) void ft_item_kernel(const FtItemArgs a) {
    static_assert(TRAIN || !DROP, "evaluation never drops");
    __shared__ float w8[FT_W];
    __shared__ float w9[FT_W];
    __shared__ float tab[3 * 4 * LB_C];                  // bn8 | bn9 | bn9b, each [mean | rsq | gamma | beta]
    __shared__ float hx[RN_MAX_DENSE][LB_HMAX];           // input of dense layer d (d >= 1)
    __shared__ float hxh[RN_MAX_DENSE][LB_HMAX];          // normalised ReLU6 output of dense layer d, before gamma and beta
    __shared__ float hmm[RN_MAX_DENSE][LB_HMAX];          // pre-activation of dense layer d
    __shared__ float hg[2][LB_HMAX];
    __shared__ float red[FT_NT];
    __shared__ float red3[TRAIN ? FT_WG_GROUPS * FT_W : 1];
    __shared__ double dred[TRAIN ? FT_NT : 1];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int S7 = a.S7, C8 = a.C8, S8 = a.S8, C9 = a.C9, S9 = a.S9;
    const int64_t item = a.index ? static_cast<int64_t>(a.index[a.base + b]) : a.base + b;
    const float* x7;
    if constexpr (D3)
        x7 = a.x7ws + static_cast<int64_t>(b) * S7 * S7 * LB_C;
    else
        x7 = a.feats + item * S7 * S7 * LB_C;
    float* wsi = a.ws + b * a.ws_item;
    float* c8 = wsi + a.off_c8;
    float* xh8 = wsi + a.off_xh8;
    float* s8 = wsi + a.off_s8;
    float* c9 = wsi + a.off_c9;
    float* xh9 = wsi + a.off_xh9;
    float* xh9b = wsi + a.off_xh9b;
    float* fl = wsi + a.off_fl;
    const float* P = a.P;
    const float* F = a.F;
    for (int i = tid; i < FT_W; i += FT_NT) {
        w8[i] = P[a.o_w8 + i];
        w9[i] = P[a.o_w9 + i];
    }
    if (tid < 2 * LB_C) {
        tab[tid] = F[a.f_bn8 + tid];
        tab[64 + tid] = F[a.f_bn9 + tid];
        tab[128 + tid] = F[a.f_bn9b + tid];
    } else if (tid < 3 * LB_C) {
        const int c = tid - 2 * LB_C;
        tab[32 + c] = P[a.o_g8 + c];
        tab[48 + c] = P[a.o_b8 + c];
        tab[96 + c] = P[a.o_g9 + c];
        tab[112 + c] = P[a.o_b9 + c];
        tab[160 + c] = P[a.o_g9b + c];
        tab[176 + c] = P[a.o_b9b + c];
    }
    __syncthreads();
    // ---- forward
    for (int i = tid; i < C8 * C8 * LB_C; i += FT_NT) {
        const int co = i & 15, p = i >> 4;
        c8[i] = conv16_at(x7, S7, w8, p / C8, p % C8, co);
    }
    __syncthreads();
    for (int i = tid; i < S8 * S8 * LB_C; i += FT_NT) {
        const int co = i & 15, p = i >> 4, y = p / S8, x = p % S8;
        const float t = pool_relu6_sum(c8, C8, y, x, co);
        const float xh = (t * (1.0f / 16.0f) - tab[co]) * tab[16 + co];
        if (TRAIN) xh8[i] = xh;
        s8[i] = fmaf(xh, tab[32 + co], tab[48 + co]);
    }
    __syncthreads();
    for (int i = tid; i < C9 * C9 * LB_C; i += FT_NT) {
        const int co = i & 15, p = i >> 4;
        c9[i] = conv16_at(s8, S8, w9, p / C9, p % C9, co);
    }
    __syncthreads();
    for (int i = tid; i < S9 * S9 * LB_C; i += FT_NT) {
        const int co = i & 15, p = i >> 4, y = p / S9, x = p % S9;
        const float t = pool_relu6_sum(c9, C9, y, x, co);
        const float xh = (t * (1.0f / 16.0f) - tab[64 + co]) * tab[80 + co];
        const float bv = fmaf(xh, tab[96 + co], tab[112 + co]);
        const float xhb = ((bv + skip_resize_at(x7, S7, a.rs, y, x, co)) - tab[128 + co]) * tab[144 + co];
        if (TRAIN) {
            xh9[i] = xh;
            xh9b[i] = xhb;
        }
        if constexpr (DROP)
            fl[i] = rn_dropout_apply(a.drop, RN_DROP_SITE_FLAT, b, i, fmaf(xhb, tab[160 + co], tab[176 + co]));
        else
            fl[i] = fmaf(xhb, tab[160 + co], tab[176 + co]);
    }
    __syncthreads();
    // ---- dense head forward: each layer's dot products split over FT_NT / 64 groups of k, summed in a fixed order
    for (int d = 0; d < a.n_dense; ++d) {
        const int nout = a.nout[d];
        float t = dense_splitk<FT_NT>(d == 0 ? fl : hx[d], P + a.o_dw[d], a.nin[d], nout, red, tid);
        if (tid < nout) {
            if (a.o_db[d] >= 0) t += P[a.o_db[d] + tid];
            hmm[d][tid] = t;
            if (d + 1 < a.n_dense) {
                float r = relu6f(t);
                if (a.o_dg[d] >= 0) {
                    const float xh = (r - F[a.f_dbn[d] + tid]) * F[a.f_dbn[d] + nout + tid];
                    hxh[d][tid] = xh;
                    r = fmaf(xh, P[a.o_dg[d] + tid], P[a.o_dbeta[d] + tid]);
                }
                if constexpr (DROP) r = rn_dropout_apply(a.drop, RN_DROP_SITE_DENSE + d, b, tid, r);
                hx[d + 1][tid] = r;
            } else if constexpr (DROP) {
                const bool keep = rn_dropout_keep(a.drop, RN_DROP_SITE_DENSE + d, b, tid);
                hx[0][tid] = keep ? relu6f(t) * a.drop.scale : 0.f;
                hxh[d][tid] = keep ? a.drop.scale : 0.f;
            }
        }
        __syncthreads();
    }
    // ---- softmax of relu6(z), the item's CE term, dL/dz of the last layer (the 1 / n of the mean is applied by the update kernel)
    const int L = a.n_dense - 1;
    if (tid == 0) {
        const int nc = a.nc;
        const float* z = hmm[L];
        // the logits the softmax, the CE term and the argmax read: relu6(z), behind the last block's dropout with DROP
        auto logit = [&](int j) {
            if constexpr (DROP)
                return hx[0][j];
            else
                return relu6f(z[j]);
        };
        float mx = logit(0);
        int best = 0;
        for (int j = 1; j < nc; ++j) {
            const float r = logit(j);
            if (r > mx) {
                mx = r;
                best = j;
            }
        }
        double se = 0.0;
        for (int j = 0; j < nc; ++j) se += exp(static_cast<double>(logit(j)) - static_cast<double>(mx));
        const int y = a.labels ? a.labels[item] : -1;
        if (y >= 0) a.item_loss[b] = log(se) - (static_cast<double>(logit(y)) - static_cast<double>(mx));
        for (int j = 0; j < nc; ++j) {
            const float p = static_cast<float>(exp(static_cast<double>(logit(j)) - static_cast<double>(mx)) / se);
            if constexpr (DROP)
                hg[L & 1][j] = relu6_passes(z[j]) && hxh[L][j] != 0.f ? (p - (j == y ? 1.f : 0.f)) * hxh[L][j] : 0.f;
            else if (TRAIN)
                hg[L & 1][j] = relu6_passes(z[j]) ? p - (j == y ? 1.f : 0.f) : 0.f;
            else
                a.probs[b * nc + j] = p;
        }
        if (!TRAIN) a.ids[b] = best;
    }
    if constexpr (TRAIN) {
        float* gs8 = wsi + a.off_gs8;
        float* gfl = wsi + a.off_gfl;
        float* prt = a.part + b * a.rec;
        __syncthreads();
        // ---- adjoint of the head: per layer its input and dL/dz go to the partials; MatMul -> transposed kernel, BN, ReLU6 mask
        for (int d = L; d >= 0; --d) {
            const int nin = a.nin[d], nout = a.nout[d];
            const float* gz = hg[d & 1];
            const float* xin = d == 0 ? fl : hx[d];
            const float* W = P + a.o_dw[d];
            if (tid < nout) prt[a.p_gz[d] + tid] = gz[tid];
            for (int k = tid; k < nin; k += FT_NT) {
                prt[a.p_x[d] + k] = xin[k];
                float v = dense_adjoint_at(W, nout, gz, k);
                if constexpr (DROP) v = rn_dropout_apply(a.drop, d == 0 ? RN_DROP_SITE_FLAT : RN_DROP_SITE_DENSE + d - 1, b, k, v);
                if (d == 0) {
                    gfl[k] = v;
                } else {
                    if (a.o_dg[d - 1] >= 0) {
                        prt[a.p_dg[d - 1] + k] = v * hxh[d - 1][k];
                        prt[a.p_dbeta[d - 1] + k] = v;
                        v *= P[a.o_dg[d - 1] + k] * F[a.f_dbn[d - 1] + nin + k];
                    }
                    hg[(d - 1) & 1][k] = relu6_passes(hmm[d - 1][k]) ? v : 0.f;
                }
            }
            __syncthreads();
        }
        // ---- stage 9: the BN behind the add, the add (only the conv branch is followed), the first BN; gfl becomes dL/d pool9
        {
            const int c = tid & 15;
            float dg2 = 0.f, db2 = 0.f, dg1 = 0.f, db1 = 0.f;
            const float k2 = tab[160 + c] * tab[144 + c], k1 = tab[96 + c] * tab[80 + c];
            for (int p = tid >> 4; p < S9 * S9; p += FT_NT / LB_C) {
                const int i = p * LB_C + c;
                const float g = gfl[i];
                dg2 = fmaf(g, xh9b[i], dg2);
                db2 += g;
                const float ga = g * k2;
                if constexpr (D3) (wsi + a.off_gadd)[i] = ga;
                dg1 = fmaf(ga, xh9[i], dg1);
                db1 += ga;
                gfl[i] = ga * k1;
            }
            float t;
            t = channel_sum(dg2, red, tid);
            if (tid < LB_C) prt[a.p_bn9b + tid] = t;
            t = channel_sum(db2, red, tid);
            if (tid < LB_C) prt[a.p_bn9b + LB_C + tid] = t;
            t = channel_sum(dg1, red, tid);
            if (tid < LB_C) prt[a.p_bn9 + tid] = t;
            t = channel_sum(db1, red, tid);
            if (tid < LB_C) prt[a.p_bn9 + LB_C + tid] = t;
        }
        // ---- pool 9 adjoint and conv 9's ReLU6 mask, in place over c9: dL/dconv9
        for (int i = tid; i < C9 * C9 * LB_C; i += FT_NT) {
            const int co = i & 15, p = i >> 4, Y = p / C9, X = p % C9;
            const float t = pool_cover_sum(gfl, S9, Y, X, co);
            c9[i] = relu6_passes(c9[i]) ? t * (1.0f / 16.0f) : 0.f;
        }
        __syncthreads();
#ifndef FT_NO_WGRAD   // (measurement arm: csrc/build.sh RN_VARIANT_FLAGS=-DFT_NO_WGRAD times the step without the two weight gradients)
        wgrad16(s8, S8, c9, C9, prt + a.p_w9, red3, tid);
#endif
        // ---- conv 9 adjoint -> dL/ds8.bn
        for (int i = tid; i < S8 * S8 * LB_C; i += FT_NT) {
            const int ci = i & 15, p = i >> 4, Y = p / S8, X = p % S8;
            gs8[i] = conv16_adjoint_at(c9, C9, w9, Y, X, ci);
        }
        __syncthreads();
        // ---- stage 8's BN; gs8 becomes dL/d pool8
        {
            const int c = tid & 15;
            float dg = 0.f, db = 0.f;
            const float k1 = tab[32 + c] * tab[16 + c];
            for (int p = tid >> 4; p < S8 * S8; p += FT_NT / LB_C) {
                const int i = p * LB_C + c;
                const float g = gs8[i];
                dg = fmaf(g, xh8[i], dg);
                db += g;
                gs8[i] = g * k1;
            }
            float t;
            t = channel_sum(dg, red, tid);
            if (tid < LB_C) prt[a.p_bn8 + tid] = t;
            t = channel_sum(db, red, tid);
            if (tid < LB_C) prt[a.p_bn8 + LB_C + tid] = t;
        }
        for (int i = tid; i < C8 * C8 * LB_C; i += FT_NT) {
            const int co = i & 15, p = i >> 4, Y = p / C8, X = p % C8;
            const float t = pool_cover_sum(gs8, S8, Y, X, co);
            c8[i] = relu6_passes(c8[i]) ? t * (1.0f / 16.0f) : 0.f;
        }
        __syncthreads();
#ifndef FT_NO_WGRAD
        wgrad16(x7, S7, c8, C8, prt + a.p_w8, red3, tid);
#endif
        if constexpr (D3) {
            // ---- g7 = conv 8 adjoint + transpose of the skip resize; stage 7's BN
            const float* gadd = wsi + a.off_gadd;
            const float* xh7 = a.xh7 + static_cast<int64_t>(b) * S7 * S7 * LB_C;
            float* dp7 = a.dpool7 + static_cast<int64_t>(b) * S7 * S7 * LB_C;
            const int ci = tid & 15;
            const float k1 = P[a.o_g7 + ci] * F[a.f_bn7 + LB_C + ci];
            float dg = 0.f, db = 0.f;
            for (int p = tid >> 4; p < S7 * S7; p += FT_NT / LB_C) {
                const int i = p * LB_C + ci, Y = p / S7, X = p % S7;
                const float g = conv16_adjoint_at(c8, C8, w8, Y, X, ci) + skip_resize_adjoint_at(gadd, S9, a.rs, Y, X, ci);
                dg = fmaf(g, xh7[i], dg);
                db += g;
                dp7[i] = g * k1;
            }
            float t;
            t = channel_sum(dg, red, tid);
            if (tid < LB_C) prt[a.p_bn7 + tid] = t;
            t = channel_sum(db, red, tid);
            if (tid < LB_C) prt[a.p_bn7 + LB_C + tid] = t;
        }
        // ---- sum v^2 over the parameter slab (its padding is zero), for the loss's L2 term
        if (b == 0 && a.l2sum) {
            double t = 0.0;
            for (int i = tid; i < a.n_param; i += FT_NT) t += static_cast<double>(P[i]) * static_cast<double>(P[i]);
            dred[tid] = t;
            __syncthreads();
            for (int s = FT_NT / 2; s > 0; s >>= 1) {
                if (tid < s) dred[tid] += dred[tid + s];
                __syncthreads();
            }
            if (tid == 0) *a.l2sum = dred[0];
        }
    }
}

// Site 0 of rn_dropout.h, the pre-pass of a depth-3 step with dropout: slot b's dropped copy of item index[base + b] of the resident
// cache, x6d[b] [S6, S6, 128].  ft7_fwd_kernel and ft7_bwd_kernel then read x6d in slot order: each x6 element is read by nine taps
// in both, and the generator at every read would cost more than this copy.  One thread handles four consecutive floats (one generator
// call, one 16-byte load, one 16-byte store); an item is a whole number of such quads.
struct Ft7DropArgs {
    const float* feats;              // the resident cache [n_items, S6, S6, 128]
    const int32_t* index;            // item of slot b = index[base + b]
    int64_t base;
    int64_t item_quads;              // S6 * S6 * 128 / 4
    int64_t total_quads;             // batch * item_quads
    float* x6d;                      // [batch, S6, S6, 128]
    RnDropout drop;
};

__global__ __launch_bounds__(256) void ft7_drop_kernel(const Ft7DropArgs a) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; q < a.total_quads; q += stride) {
        const int64_t b = q / a.item_quads, qi = q - b * a.item_quads;
        const int64_t item = a.index[a.base + b];
        const f32x4 x = reinterpret_cast<const f32x4*>(a.feats)[item * a.item_quads + qi];
        uint32_t w[4];
        rn_dropout_words(a.drop, RN_DROP_SITE_X6, static_cast<uint32_t>(b), static_cast<uint32_t>(qi), w);
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = rn_dropout_word_keeps(a.drop, w[k]) ? x[k] * a.drop.scale : 0.f;
        reinterpret_cast<f32x4*>(a.x6d)[q] = y;
    }
}

// keep bytes of elements [0, count) of (site, slot) for rn_ft_dropout_mask
__global__ __launch_bounds__(256) void ft_mask_kernel(const RnDropout drop, int site, int slot, int64_t count, uint8_t* keep) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < count; e += stride)
        keep[e] = rn_dropout_keep(drop, static_cast<uint32_t>(site), static_cast<uint32_t>(slot), static_cast<uint32_t>(e)) ? 1 : 0;
}

// how the update kernel forms one variable's gradient from the items' partials
enum { FT_SUM = 0, FT_OUTER = 1, FT_BANDS = 2 };
struct FtVarDev {
    int off, count;                  // in the parameter slab
    int kind;
    int src;                         // FT_SUM: offset in the partials record;  FT_OUTER: the layer's input vector;  FT_BANDS: unused
    int src_g, nout;                 // FT_OUTER: the layer's dL/dz vector and its length
};

struct FtUpdateArgs {
    int nvars, total;
    FtVarDev v[FT_MAX_VARS];
    float *P, *G, *M, *V;
    const float* part;
    int64_t rec;
    int n;
    float l2, lr_t, omb1, omb2, eps;   // omb = 1 - beta, formed in float64 on the host
    const double* item_loss;
    const double* l2sum;
    float* loss_out;                 // this step's slot
    // depth 3: conv 7's kernel is FT_BANDS, its partials one per (item, band) (rn_finetune7.hip)
    const float* part7;              // [n, bands, FT7_W]
    int bands;
};

// (templated on the depth so that the depth-2 instantiation carries no float64 band sum)
template <bool D3>
__global__ __launch_bounds__(256) void ft_update_kernel(const FtUpdateArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        double s = 0.0;
        for (int i = 0; i < a.n; ++i) s += a.item_loss[i];
        *a.loss_out = static_cast<float>(s / a.n + 0.5 * static_cast<double>(a.l2) * *a.l2sum);
    }
    if (e >= a.total) return;
    int vi = -1;
    for (int i = 0; i < a.nvars; ++i)
        if (e >= a.v[i].off && e < a.v[i].off + a.v[i].count) vi = i;
    if (vi < 0) return;                // padding between two variables
    const FtVarDev var = a.v[vi];
    const int le = e - var.off;
    float s = 0.f;
    if (D3 && var.kind == FT_BANDS) {
        if constexpr (D3) {
            // (float64: the items' gradients of a trained model all but cancel, and a float32 running sum over n x bands partials
            //  of the items' size was the largest rounding term of dW7 -- 1.1e-5 of its largest entry at batch 32, the bound 1e-5)
            const float* p = a.part7 + le;
            double t = 0.0;
            for (int i = 0; i < a.n; ++i)
                for (int k = 0; k < a.bands; ++k) t += static_cast<double>(p[(static_cast<int64_t>(i) * a.bands + k) * FT7_W]);
            s = static_cast<float>(t);
        }
    } else if (var.kind == FT_SUM) {
        const float* p = a.part + var.src + le;
#pragma unroll 8
        for (int i = 0; i < a.n; ++i) s += p[i * a.rec];             // (the loads do not depend on the sum: eight are in flight)
    } else {
        const float* px = a.part + var.src + le / var.nout;
        const float* pg = a.part + var.src_g + le % var.nout;
#pragma unroll 8
        for (int i = 0; i < a.n; ++i) s = fmaf(px[i * a.rec], pg[i * a.rec], s);
    }
    const float p = a.P[e];
    const float g = fmaf(a.l2, p, s / static_cast<float>(a.n));
    float m = a.M[e], v = a.V[e];
    m += (g - m) * a.omb1;
    v += (g * g - v) * a.omb2;
    a.G[e] = g;
    a.M[e] = m;
    a.V[e] = v;
    a.P[e] = p - a.lr_t * m / (sqrtf(v) + a.eps);
}

// ---- validation inside a run (rn_ft_run_validated).  A point is one evaluation of the resident validation set between two steps:
// per chunk of max_batch items the forward-only item kernel and ft_val_chunk_kernel, then ft_val_close_kernel and
// ft_val_snapshot_kernel once.  The point's tables are zeroed by one memset at the head of the run.
constexpr int FT_VAL_NT = 256;

// the best point so far; lives on the device, where the closer decides, and is mirrored to the host after a run's synchronisation
struct FtBestDev {
    long long step, correct, n_val;
    int valid, pad;
};

// Chunk reducer, one workgroup: the chunk's m items add to the point's confusion matrix (integer atomics) and its cross-entropy sum
// (float64: thread t sums items t, t + FT_VAL_NT, ... in order, a fixed tree joins the threads, and the chunks are chained in order
// through *ce -- the same call gives the same bits).
struct FtValChunkArgs {
    const int64_t* ids;              // [m] the chunk's argmax (ft_item_kernel, forward only)
    const double* item_loss;         // [m] its CE terms
    const int32_t* labels;           // the chunk's labels (checked on the host: inside [0, nc))
    int m, nc;
    int32_t* conf;                   // the point's [nc, nc], row = label, column = predicted
    double* ce;                      // the point's sum so far
};

__global__ __launch_bounds__(FT_VAL_NT) void ft_val_chunk_kernel(const FtValChunkArgs a) {
    __shared__ double dred[FT_VAL_NT];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int i = tid; i < a.m; i += FT_VAL_NT) {
        t += a.item_loss[i];
        const int y = a.labels[i], p = static_cast<int>(a.ids[i]);
        if (y >= 0 && y < a.nc && p >= 0 && p < a.nc) atomicAdd(a.conf + y * a.nc + p, 1);
    }
    dred[tid] = t;
    __syncthreads();
    for (int s = FT_VAL_NT / 2; s > 0; s >>= 1) {
        if (tid < s) dred[tid] += dred[tid + s];
        __syncthreads();
    }
    if (tid == 0) *a.ce += dred[0];
}

// Point closer, one workgroup: sum v^2 over the parameter slab in float64 (a fixed strided sum per thread and a fixed tree, as the
// item kernel forms it), the point's float32 loss, its number of correct predictions (the trace), and whether it beats the best so
// far: strictly more correct, so the earliest of equal points stays.  *flag tells the snapshot launch behind it.
struct FtValCloseArgs {
    const float* P;
    int n_param, nc;
    float l2;
    long long n_val, step;
    const double* ce;
    const int32_t* conf;
    float* loss;
    int32_t* flag;
    FtBestDev* best;
};

__global__ __launch_bounds__(FT_NT) void ft_val_close_kernel(const FtValCloseArgs a) {
    __shared__ double dred[FT_NT];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int i = tid; i < a.n_param; i += FT_NT) t += static_cast<double>(a.P[i]) * static_cast<double>(a.P[i]);
    dred[tid] = t;
    __syncthreads();
    for (int s = FT_NT / 2; s > 0; s >>= 1) {
        if (tid < s) dred[tid] += dred[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        *a.loss = static_cast<float>(*a.ce / static_cast<double>(a.n_val) + 0.5 * static_cast<double>(a.l2) * dred[0]);
        long long correct = 0;
        for (int c = 0; c < a.nc; ++c) correct += a.conf[c * a.nc + c];
        const bool beats = !a.best->valid || correct > a.best->correct;
        *a.flag = beats ? 1 : 0;
        if (beats) *a.best = FtBestDev{a.step, correct, a.n_val, 1, 0};
    }
}

// Snapshot: where the closer in front of it set the point's flag, the parameter slab (a whole number of quads) goes to d_P_best
__global__ __launch_bounds__(256) void ft_val_snapshot_kernel(const int32_t* flag, const float* P, float* best, int quads) {
    if (!*flag) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < quads) reinterpret_cast<f32x4*>(best)[q] = reinterpret_cast<const f32x4*>(P)[q];
}

// rn_ft_run_views: a call's labels in slot order, out[k] = labels[index[k]] (the index was range-checked on the host)
__global__ __launch_bounds__(256) void ft_gather_labels_kernel(const int32_t* labels, const int32_t* index, int64_t count, int32_t* out) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k < count) out[k] = labels[index[k]];
}

struct FtVarHost {
    std::string name;
    int off = 0, count = 0;
};

}  // namespace

struct rn_ft {
    int device = 0, max_batch = 0, nc = 0;
    int depth = 2;                                 // trained conv stages: 2 (feature s7.bn) or 3 (feature s6.bn)
    rn_ft_config cfg{};
    hipStream_t stream = nullptr;
    rn_lastblock sd{};                             // the block's sides
    std::vector<FtVarHost> vars;
    int n_param = 0;                               // floats of the parameter slab (every variable padded to 4 floats)
    FtItemArgs item{};                             // everything but the per-call fields
    FtUpdateArgs upd{};
    Ft7Args s7{};                                  // depth 3
    float *d_P = nullptr, *d_G = nullptr, *d_M = nullptr, *d_V = nullptr, *d_F = nullptr, *d_rlerp = nullptr;
    int32_t* d_rtab = nullptr;
    float *d_ws = nullptr, *d_part = nullptr;
    double *d_item_loss = nullptr, *d_l2sum = nullptr;
    float* d_losses = nullptr;                     // [losses_cap]
    int losses_cap = 0;
    float* d_probs = nullptr;                      // eval staging [max_batch, nc]
    int64_t* d_ids = nullptr;
    rn_timer timer;                                // around the step loop of the last rn_ft_run
    int64_t steps_done = 0;                        // t of the next step is steps_done + 1; global step = start_step + steps_done
    std::vector<void*> allocs;                     // trainer-owned device memory (freed by rn_ft_destroy)
    std::vector<void*> user;                       // rn_ft_upload buffers not yet freed
    // dropout (rn_ft_set_dropout): rate 0 is off and runs the launches a trainer without it runs
    float drop_rate = 0.f;
    uint64_t drop_seed = 0;
    RnDropout drop{};                              // key, threshold and scale; the step is set per launch
    float* d_x6d = nullptr;                        // depth 3: [max_batch, S6, S6, 128], allocated when dropout is first switched on
    // validation inside a run (rn_ft_run_validated): allocated when the first validated run needs them
    float* d_P_best = nullptr;                     // the parameter slab at the best point
    FtBestDev* d_best = nullptr;                   // the best point, decided on the device ...
    FtBestDev best{};                              // ... and its host copy, read back behind every validated run
    void* d_val = nullptr;                         // the per-point tables of a run: [cap] ce | [cap] loss | [cap] flag | [cap, nc, nc]
    int val_cap = 0;
    // training on fresh views (rn_ft_run_views): allocated when the first such run needs them
    float* d_vfeat[FT_VIEW_SLOTS] = {};            // the feature slots [max_batch, side, side, C] the handle's trunk fills in turn
    int32_t* d_iota = nullptr;                     // [max_batch] 0, 1, ...: the index of a pass over the slot
    int32_t* d_glabels = nullptr;                  // [glabels_cap] a call's labels in slot order
    size_t glabels_cap = 0;
    hipEvent_t ev_feats[FT_VIEW_SLOTS] = {}, ev_read[FT_VIEW_SLOTS] = {};   // slot k is filled (handle's stream) / has been read (trainer's)
};

namespace {

// trainer-owned device memory (an empty request gets 4 bytes)
template <typename T>
int ft_upload(rn_ft* ft, const T* src, size_t count, T** out) {
    return rn_owned_upload(ft->allocs, 4, src, count, out);
}
template <typename T>
int ft_zeroed(rn_ft* ft, size_t count, T** out) {
    return rn_owned_zeroed(ft->allocs, 4, count, out);
}

// the dense head must continue the last block and end in the classes
int ft_check_head(const rn_ft* ft, const rn_weights* w) {
    if (w->dense[0].nin != ft->sd.S9 * ft->sd.S9 * LB_C) {
        rn_set_error("rn_ft_create: the first dense layer takes %d inputs, the last block delivers %d", w->dense[0].nin,
                     ft->sd.S9 * ft->sd.S9 * LB_C);
        return RN_E_INVALID;
    }
    for (int d = 1; d < w->n_dense; ++d)
        if (w->dense[d].nin != w->dense[d - 1].nout) {
            rn_set_error("rn_ft_create: dense layer %d takes %d inputs, the layer before it delivers %d", d, w->dense[d].nin,
                         w->dense[d - 1].nout);
            return RN_E_INVALID;
        }
    if (w->dense[w->n_dense - 1].nout != w->num_classes) {
        rn_set_error("rn_ft_create: the last dense layer has %d outputs for %d classes", w->dense[w->n_dense - 1].nout, w->num_classes);
        return RN_E_INVALID;
    }
    return RN_OK;
}

// The trained variables in checkpoint order (ft->vars, the parameter slab P, the frozen BN moments F), one item's partials record
// and how the update kernel forms each variable's gradient from it (ft->upd.v); the offsets go into ft->item and ft->s7.
void ft_build_vars(rn_ft* ft, const rn_weights* w, std::vector<float>& P, std::vector<float>& F) {
    const int ns = w->n_stages;
    const float eps = w->bn_epsilon;
    FtItemArgs& a = ft->item;
    FtUpdateArgs& u = ft->upd;
    int rec = 0;
    auto take = [&](int cnt) {                     // a piece of the partials record
        const int off = rec;
        rec += (cnt + 3) & ~3;
        return off;
    };
    auto put_var = [&](const std::string& name, const float* src, int cnt, int kind, int src_off, int src_g = 0, int nout = 0) {
        FtVarHost v;
        v.name = name;
        v.off = static_cast<int>(P.size());
        v.count = cnt;
        P.insert(P.end(), src, src + cnt);
        P.resize((P.size() + 3) & ~static_cast<size_t>(3));
        ft->vars.push_back(v);
        u.v[u.nvars++] = FtVarDev{v.off, cnt, kind, src_off, src_g, nout};
        return v.off;
    };
    auto put_frozen = [&](const float* mean, const float* var, int cnt) {
        const int off = static_cast<int>(F.size());
        F.insert(F.end(), mean, mean + cnt);
        for (int c = 0; c < cnt; ++c) F.push_back(1.0f / sqrtf(var[c] + eps));
        F.resize((F.size() + 3) & ~static_cast<size_t>(3));
        return off;
    };
    // TensorFlow numbers its variables by creation: conv stage i is conv2d_i; BNs count every stage's and every residual add's
    auto suffix = [](const char* base, int i) { return i == 0 ? std::string(base) : std::string(base) + "_" + std::to_string(i); };
    const int first = ns - ft->depth;              // the first trained stage
    int bn_index = 0;
    for (int i = 0; i < first; ++i) bn_index += w->stages[i].gamma2 ? 2 : 1;
    // a BN's gamma and beta, their partials [d gamma | d beta] at p_bn, its frozen moments
    auto put_bn = [&](const float* gamma, const float* beta, const float* mean, const float* var, int p_bn, int* o_g, int* o_b, int* f_bn) {
        const std::string name = suffix("batch_normalization", bn_index++);
        *o_g = put_var(name + "/gamma", gamma, LB_C, FT_SUM, p_bn);
        *o_b = put_var(name + "/beta", beta, LB_C, FT_SUM, p_bn + LB_C);
        *f_bn = put_frozen(mean, var, LB_C);
    };
    a.p_w8 = take(FT_W);
    a.p_w9 = take(FT_W);
    a.p_bn8 = take(2 * LB_C);
    a.p_bn9 = take(2 * LB_C);
    a.p_bn9b = take(2 * LB_C);
    if (ft->depth == 3) {
        // conv 7's kernel, its BN's gamma and beta: in front of the others, as the checkpoint orders them
        const rn_conv_stage& st7 = w->stages[ns - 3];
        Ft7Args& s = ft->s7;
        a.p_bn7 = take(2 * LB_C);
        s.o_w7 = put_var(suffix("conv2d", ns - 3) + "/kernel", st7.kernel, FT7_W, FT_BANDS, 0);
        put_bn(st7.gamma, st7.beta, st7.mean, st7.variance, a.p_bn7, &s.o_g7, &s.o_b7, &s.f_bn7);
        a.o_g7 = s.o_g7;
        a.f_bn7 = s.f_bn7;
    }
    const rn_conv_stage &st8 = w->stages[ns - 2], &st9 = w->stages[ns - 1];
    a.o_w8 = put_var(suffix("conv2d", ns - 2) + "/kernel", st8.kernel, FT_W, FT_SUM, a.p_w8);
    put_bn(st8.gamma, st8.beta, st8.mean, st8.variance, a.p_bn8, &a.o_g8, &a.o_b8, &a.f_bn8);
    a.o_w9 = put_var(suffix("conv2d", ns - 1) + "/kernel", st9.kernel, FT_W, FT_SUM, a.p_w9);
    put_bn(st9.gamma, st9.beta, st9.mean, st9.variance, a.p_bn9, &a.o_g9, &a.o_b9, &a.f_bn9);
    put_bn(st9.gamma2, st9.beta2, st9.mean2, st9.variance2, a.p_bn9b, &a.o_g9b, &a.o_b9b, &a.f_bn9b);
    a.n_dense = w->n_dense;
    a.nc = w->num_classes;
    for (int d = 0; d < w->n_dense; ++d) {
        const rn_dense_layer& l = w->dense[d];
        a.nin[d] = l.nin;
        a.nout[d] = l.nout;
        a.p_x[d] = take(l.nin);
        a.p_gz[d] = take(l.nout);
        a.o_db[d] = a.o_dg[d] = a.o_dbeta[d] = a.f_dbn[d] = a.p_dg[d] = a.p_dbeta[d] = -1;
        a.o_dw[d] = put_var(suffix("dense", d) + "/kernel", l.kernel, l.nin * l.nout, FT_OUTER, a.p_x[d], a.p_gz[d], l.nout);
        if (l.bias) a.o_db[d] = put_var(suffix("dense", d) + "/bias", l.bias, l.nout, FT_SUM, a.p_gz[d]);
        if (l.gamma) {
            a.p_dg[d] = take(l.nout);
            a.p_dbeta[d] = take(l.nout);
            const std::string name = suffix("batch_normalization", bn_index++);
            a.o_dg[d] = put_var(name + "/gamma", l.gamma, l.nout, FT_SUM, a.p_dg[d]);
            a.o_dbeta[d] = put_var(name + "/beta", l.beta, l.nout, FT_SUM, a.p_dbeta[d]);
            a.f_dbn[d] = put_frozen(l.mean, l.variance, l.nout);
        }
    }
    ft->n_param = a.n_param = u.total = static_cast<int>(P.size());
    a.rec = u.rec = rec;
}

// the item kernel's per-workgroup workspace (every piece a multiple of 16 floats), the partials records and the loss / eval staging
int ft_build_workspace(rn_ft* ft) {
    FtItemArgs& a = ft->item;
    const rn_lastblock& sd = ft->sd;
    const int64_t n8 = static_cast<int64_t>(sd.S8) * sd.S8 * LB_C, n9 = static_cast<int64_t>(sd.S9) * sd.S9 * LB_C;
    a.off_c8 = 0;
    a.off_xh8 = a.off_c8 + static_cast<int64_t>(sd.C8) * sd.C8 * LB_C;
    a.off_s8 = a.off_xh8 + n8;
    a.off_gs8 = a.off_s8 + n8;
    a.off_c9 = a.off_gs8 + n8;
    a.off_xh9 = a.off_c9 + static_cast<int64_t>(sd.C9) * sd.C9 * LB_C;
    a.off_xh9b = a.off_xh9 + n9;
    a.off_fl = a.off_xh9b + n9;
    a.off_gfl = a.off_fl + n9;
    a.ws_item = a.off_gfl + n9;
    if (ft->depth == 3) {
        a.off_gadd = a.ws_item;
        a.ws_item += n9;
    }
    int rc;
    const size_t nb = static_cast<size_t>(ft->max_batch);
    if ((rc = ft_zeroed(ft, nb * a.ws_item, &ft->d_ws)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb * static_cast<size_t>(a.rec), &ft->d_part)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb, &ft->d_item_loss)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, 1, &ft->d_l2sum)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb * ft->nc, &ft->d_probs)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb, &ft->d_ids)) != RN_OK) return rc;
    return RN_OK;
}

// depth 3: stage 7's per-step workspace, and one weight-gradient partial per (item, band) for the batch size that needs the most
int ft_build_depth3(rn_ft* ft) {
    Ft7Args& s = ft->s7;
    const rn_lastblock& sd = ft->sd;
    const size_t nb = static_cast<size_t>(ft->max_batch), n7 = static_cast<size_t>(sd.S7) * sd.S7 * LB_C;
    size_t nparts = 0;
    for (int b = 1; b <= ft->max_batch; ++b) {
        int bf, rf, bb, rb;
        rn_ft7_bands(b, sd.C7, sd.S7, &bf, &rf, &bb, &rb);
        nparts = std::max(nparts, static_cast<size_t>(b) * bb);
    }
    int rc;
    float* d_x7 = nullptr;
    if ((rc = ft_zeroed(ft, nb * sd.C7 * sd.C7 * LB_C, &s.pre)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb * n7, &s.xh7)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb * n7, &d_x7)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nb * n7, &ft->item.dpool7)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, nparts * FT7_W, &s.part)) != RN_OK) return rc;
    s.S6 = sd.S6;
    s.C7 = sd.C7;
    s.S7 = sd.S7;
    s.P = ft->d_P;
    s.F = ft->d_F;
    s.x7 = d_x7;
    s.dpool = ft->item.dpool7;
    ft->item.x7ws = d_x7;
    ft->item.xh7 = s.xh7;
    ft->upd.part7 = s.part;
    return RN_OK;
}

int ft_build(rn_ft* ft, const rn_weights* w) {
    if (rn_lastblock_sides(w, &ft->sd) < w->n_stages) {
        rn_set_error("rn_ft_create: im_side %d is too small for the graph", w->im_side);
        return RN_E_INVALID;
    }
    int rc;
    if ((rc = ft_check_head(ft, w)) != RN_OK) return rc;
    if (ft->depth == 3)
        if (const char* why = rn_ft7_geometry_reason(ft->sd.S6, ft->sd.C7, ft->sd.S7)) {
            rn_set_error("rn_ft_create_depth: not supported on this graph (%s)", why);
            return RN_E_INVALID;
        }
    std::vector<float> P, F, lerp;
    std::vector<int32_t> rtab;
    ft_build_vars(ft, w, P, F);
    rn_lastblock_resize_tables(ft->sd, rtab, lerp);
    const size_t np = P.size();
    if ((rc = ft_upload(ft, P.data(), np, &ft->d_P)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, np, &ft->d_G)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, np, &ft->d_M)) != RN_OK) return rc;
    if ((rc = ft_zeroed(ft, np, &ft->d_V)) != RN_OK) return rc;
    if ((rc = ft_upload(ft, F.data(), F.size(), &ft->d_F)) != RN_OK) return rc;
    if ((rc = ft_upload(ft, rtab.data(), rtab.size(), &ft->d_rtab)) != RN_OK) return rc;
    if ((rc = ft_upload(ft, lerp.data(), lerp.size(), &ft->d_rlerp)) != RN_OK) return rc;
    if ((rc = ft_build_workspace(ft)) != RN_OK) return rc;
    FtItemArgs& a = ft->item;
    a.S7 = ft->sd.S7;
    a.C8 = ft->sd.C8;
    a.S8 = ft->sd.S8;
    a.C9 = ft->sd.C9;
    a.S9 = ft->sd.S9;
    a.P = ft->d_P;
    a.F = ft->d_F;
    a.rs = LbResize{ft->d_rtab, ft->d_rtab + ft->sd.S9, ft->d_rlerp};
    a.ws = ft->d_ws;
    a.part = ft->d_part;
    a.item_loss = ft->d_item_loss;
    FtUpdateArgs& u = ft->upd;
    u.P = ft->d_P;
    u.G = ft->d_G;
    u.M = ft->d_M;
    u.V = ft->d_V;
    u.part = ft->d_part;
    u.l2 = ft->cfg.l2_coeff;
    u.omb1 = static_cast<float>(1.0 - static_cast<double>(ft->cfg.beta1));
    u.omb2 = static_cast<float>(1.0 - static_cast<double>(ft->cfg.beta2));
    u.eps = ft->cfg.epsilon;
    u.item_loss = ft->d_item_loss;
    u.l2sum = ft->d_l2sum;
    return ft->depth == 3 ? ft_build_depth3(ft) : RN_OK;
}

double ft_learn_rate(const rn_ft_config& c, int64_t step) {
    return static_cast<double>(c.learn_rate) * std::pow(static_cast<double>(c.decay_rate), static_cast<double>(step) / c.num_steps);
}

}  // namespace

namespace {
int ft_create(const rn_weights* w, int device, int max_batch, const rn_ft_config* cfg, int depth, rn_ft** out) {
    if (!w || !cfg || !out || !w->stages || !w->dense) {
        rn_set_error("rn_ft_create: null argument");
        return RN_E_INVALID;
    }
    *out = nullptr;
    if (w->n_stages > RN_MAX_STAGES || w->n_dense > RN_MAX_DENSE) {
        rn_set_error("rn_ft_create: more than %d conv stages or %d dense layers", RN_MAX_STAGES, RN_MAX_DENSE);
        return RN_E_INVALID;
    }
    if (const char* why = rn_tail_graph_reason(w)) {
        rn_set_error("rn_ft_create: not supported on this graph (%s)", why);
        return RN_E_INVALID;
    }
    if (max_batch < 1) {
        rn_set_error("rn_ft_create: max_batch = %d", max_batch);
        return RN_E_INVALID;
    }
    if (!(cfg->num_steps >= 1) || !(cfg->decay_rate > 0.f) || !(cfg->learn_rate >= 0.f) || !(cfg->beta1 >= 0.f && cfg->beta1 < 1.f) ||
        !(cfg->beta2 >= 0.f && cfg->beta2 < 1.f) || !(cfg->epsilon > 0.f) || cfg->start_step < 0 || !(cfg->l2_coeff >= 0.f)) {
        rn_set_error("rn_ft_create: bad configuration (learn_rate %g, decay_rate %g, num_steps %d, start_step %d, l2_coeff %g, beta1 %g, "
                     "beta2 %g, epsilon %g)", cfg->learn_rate, cfg->decay_rate, cfg->num_steps, cfg->start_step, cfg->l2_coeff, cfg->beta1,
                     cfg->beta2, cfg->epsilon);
        return RN_E_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        rn_set_error("rn_ft_create: device %d not available (%d visible)", device, ndev);
        return RN_E_INVALID;
    }
    DeviceGuard guard(device);
    rn_ft* ft = new rn_ft();
    ft->device = device;
    ft->max_batch = max_batch;
    ft->nc = w->num_classes;
    ft->cfg = *cfg;
    ft->depth = depth;
    int rc = RN_OK;
    if (hipStreamCreateWithFlags(&ft->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        rn_set_error("rn_ft_create: hipStreamCreate failed");
        rc = RN_E_HIP;
    }
    if (rc == RN_OK) rc = ft->timer.create();
    if (rc == RN_OK) rc = ft_build(ft, w);
    if (rc != RN_OK) {
        rn_ft_destroy(ft);
        return rc;
    }
    *out = ft;
    return RN_OK;
}
}  // namespace

extern "C" int rn_ft_create(const rn_weights* w, int device, int max_batch, const rn_ft_config* cfg, rn_ft** out) {
    return ft_create(w, device, max_batch, cfg, 2, out);
}

extern "C" int rn_ft_create_depth(const rn_weights* w, int device, int max_batch, const rn_ft_config* cfg, int depth, rn_ft** out) {
    if (depth != 2 && depth != 3) {
        if (out) *out = nullptr;
        rn_set_error("rn_ft_create_depth: depth = %d is neither 2 (features s7.bn) nor 3 (features s6.bn)", depth);
        return RN_E_INVALID;
    }
    return ft_create(w, device, max_batch, cfg, depth, out);
}

extern "C" int rn_ft_depth(const rn_ft* ft) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    return ft->depth;
}

extern "C" void rn_ft_destroy(rn_ft* ft) {
    if (!ft) return;
    DeviceGuard guard(ft->device);
    if (ft->stream) (void)hipStreamSynchronize(ft->stream);
    for (void* p : ft->allocs) (void)hipFree(p);
    for (void* p : ft->user) (void)hipFree(p);
    if (ft->d_losses) (void)hipFree(ft->d_losses);
    if (ft->d_val) (void)hipFree(ft->d_val);
    if (ft->d_glabels) (void)hipFree(ft->d_glabels);
    for (hipEvent_t e : ft->ev_feats)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ft->ev_read)
        if (e) (void)hipEventDestroy(e);
    if (ft->stream) (void)hipStreamDestroy(ft->stream);
    (void)hipGetLastError();
    delete ft;
}

extern "C" int rn_ft_upload(rn_ft* ft, const void* src, size_t bytes, void** d_ptr) {
    if (!ft || !d_ptr || (!src && bytes)) {
        rn_set_error("rn_ft_upload: null argument");
        return RN_E_INVALID;
    }
    DeviceGuard guard(ft->device);
    void* p = nullptr;
    int rc = rn_owned_alloc(ft->user, bytes, 4, &p);
    if (rc != RN_OK) return rc;
    hipError_t e;
    if (bytes && (e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)) != hipSuccess) {
        rn_set_error("rn_ft_upload: hipMemcpy failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        ft->user.pop_back();
        (void)hipFree(p);
        return RN_E_HIP;
    }
    *d_ptr = p;
    return RN_OK;
}

extern "C" int rn_ft_free(rn_ft* ft, void* d_ptr) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    auto it = std::find(ft->user.begin(), ft->user.end(), d_ptr);
    if (it == ft->user.end()) {
        rn_set_error("rn_ft_free: not a buffer of rn_ft_upload on this trainer");
        return RN_E_INVALID;
    }
    DeviceGuard guard(ft->device);
    RN_HIP(hipStreamSynchronize(ft->stream));
    ft->user.erase(it);
    RN_HIP(hipFree(d_ptr));
    return RN_OK;
}

// the depth-3 launches' arguments of one call: `m` items of `feats` from `base` on, through `index` or (null) in order
static Ft7Args ft7_call(const rn_ft* ft, const float* feats, const int32_t* index, int64_t base, int m) {
    Ft7Args s = ft->s7;
    s.feats = feats;
    s.index = index;
    s.base = base;
    rn_ft7_bands(m, ft->sd.C7, ft->sd.S7, &s.bands_f, &s.rows_f, &s.bands_b, &s.rows_b);
    return s;
}

// Labels are read back and range-checked on the host before anything is enqueued: the `n_labels` of `d_labels`, or, through
// `d_index` (rn_ft_run), its `n_index` indices and the label each one selects.  `who` is the entry point's name in the message.
static int ft_check_labels(rn_ft* ft, const char* who, const int32_t* d_labels, int64_t n_labels, const int32_t* d_index, size_t n_index) {
    std::vector<int32_t> idx(d_index ? n_index : 0), lab(static_cast<size_t>(n_labels));
    RN_HIP(hipStreamSynchronize(ft->stream));
    if (d_index) RN_HIP(hipMemcpy(idx.data(), d_index, idx.size() * 4, hipMemcpyDeviceToHost));
    RN_HIP(hipMemcpy(lab.data(), d_labels, lab.size() * 4, hipMemcpyDeviceToHost));
    const size_t count = d_index ? n_index : lab.size();
    for (size_t k = 0; k < count; ++k) {
        int64_t i = static_cast<int64_t>(k);
        if (d_index) {
            i = idx[k];
            if (i < 0 || i >= n_labels) {
                rn_set_error("%s: index[%zu] = %d outside [0, %lld)", who, k, idx[k], static_cast<long long>(n_labels));
                return RN_E_RANGE;
            }
        }
        if (lab[i] < 0 || lab[i] >= ft->nc) {
            rn_set_error("%s: label[%lld] = %d outside [0, %d)", who, static_cast<long long>(i), lab[i], ft->nc);
            return RN_E_RANGE;
        }
    }
    return RN_OK;
}

// The kernels of one pass: the item kernel's six instantiations (evaluation never drops and has no update).  They are named in the
// order this file has always first used them, which is the order the code object lays them out in.
struct FtKernels {
    void (*item)(FtItemArgs);
    void (*update)(FtUpdateArgs);
};
static FtKernels ft_kernels_of(bool train, bool d3, bool drop) {
    if (train && drop)
        return d3 ? FtKernels{ft_item_kernel<true, true, true>, ft_update_kernel<true>}
                  : FtKernels{ft_item_kernel<true, false, true>, ft_update_kernel<false>};
    if (train) return d3 ? FtKernels{ft_item_kernel<true, true>, ft_update_kernel<true>} : FtKernels{ft_item_kernel<true, false>, ft_update_kernel<false>};
    return d3 ? FtKernels{ft_item_kernel<false, true>, nullptr} : FtKernels{ft_item_kernel<false, false>, nullptr};
}

// One pass over `m` slots on the trainer's stream: the items `a` names, from a.base on.  With `u` a training step (the update
// closes it; a.drop.thr != 0 drops), without it an evaluation.  Depth 2 is the item kernel [+ the update]; depth 3 puts stage 7's
// forward pass in front of the item kernel and its backward pass behind it, and, when dropping, in front of all the pre-pass that
// gathers the step's s6.bn into d_x6d, dropped -- stage 7 then reads that copy in slot order.
static int ft_enqueue_pass(rn_ft* ft, const FtItemArgs& a, FtUpdateArgs* u, int m) {
    const bool train = u != nullptr, d3 = ft->depth == 3, dropping = a.drop.thr != 0;
    const FtKernels k = ft_kernels_of(train, d3, dropping);
    const bool gathered = d3 && dropping;
    int rc;
    if (gathered) {
        const int64_t quads = static_cast<int64_t>(ft->sd.S6) * ft->sd.S6 * (LB_CIN7 / 4);
        const Ft7DropArgs dr{a.feats, a.index, a.base, quads, quads * m, ft->d_x6d, a.drop};
        const int dblocks = static_cast<int>(std::min<int64_t>((dr.total_quads + 255) / 256, 8192));
        hipLaunchKernelGGL(ft7_drop_kernel, dim3(dblocks), dim3(256), 0, ft->stream, dr);
        RN_CHECK_LAUNCH();
    }
    Ft7Args s7{};
    if (d3) {
        // stage 7 reads the gathered copy in slot order, or the caller's items
        s7 = ft7_call(ft, gathered ? ft->d_x6d : a.feats, gathered ? nullptr : a.index, gathered ? 0 : a.base, m);
        if ((rc = rn_ft7_forward(ft->stream, s7, m)) != RN_OK) return rc;
    }
    hipLaunchKernelGGL(k.item, dim3(m), dim3(FT_NT), 0, ft->stream, a);
    RN_CHECK_LAUNCH();
    if (!train) return RN_OK;
    if (d3) {
        if ((rc = rn_ft7_backward(ft->stream, s7, m)) != RN_OK) return rc;
        u->bands = s7.bands_b;
    }
    hipLaunchKernelGGL(k.update, dim3((ft->n_param + 255) / 256), dim3(256), 0, ft->stream, *u);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// The validation of a run: the resident set, the schedule, and where the results go on the host (rn_ft_run_validated)
struct FtValidation {
    const float* d_feats;
    const int32_t* d_labels;
    int64_t n;
    int every;
    float* losses;                   // [points]
    int32_t* confusion;              // [points, nc, nc]
};

// whether a point is taken behind the step that brings the global step to `g`, the last of the run or not
static bool ft_is_point(int64_t g, int every, bool last) { return last || g % every == 0; }

static int ft_count_points(int64_t g0, int steps, int every, int64_t* point_steps, int cap) {
    int points = 0;
    for (int s = 0; s < steps; ++s) {
        const int64_t g = g0 + s + 1;
        if (!ft_is_point(g, every, s == steps - 1)) continue;
        if (point_steps && points < cap) point_steps[points] = g;
        ++points;
    }
    return points;
}

// the pieces of the per-point tables, for `cap` points
struct FtValTables {
    double* ce;
    float* loss;
    int32_t* flag;
    int32_t* conf;
    size_t bytes;
};
static FtValTables ft_val_tables(const rn_ft* ft, void* base, int cap) {
    const size_t n = static_cast<size_t>(cap), cc = static_cast<size_t>(ft->nc) * ft->nc;
    FtValTables t;
    char* p = static_cast<char*>(base);
    t.ce = reinterpret_cast<double*>(p);
    t.loss = reinterpret_cast<float*>(p + 8 * n);
    t.flag = reinterpret_cast<int32_t*>(p + 12 * n);
    t.conf = reinterpret_cast<int32_t*>(p + 16 * n);
    t.bytes = 16 * n + 4 * n * cc;
    return t;
}

// what a validated run needs beside the trainer's own memory; a failed allocation leaves the trainer as it was
static int ft_val_reserve(rn_ft* ft, int points) {
    int rc;
    if (!ft->d_P_best && (rc = ft_zeroed(ft, static_cast<size_t>(ft->n_param), &ft->d_P_best)) != RN_OK) return rc;
    if (!ft->d_best && (rc = ft_zeroed(ft, 1, &ft->d_best)) != RN_OK) return rc;
    if (points > ft->val_cap) {
        void* p = nullptr;
        const size_t bytes = ft_val_tables(ft, nullptr, points).bytes;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rn_set_error("rn_ft_run_validated: hipMalloc(%zu bytes of validation tables) failed: %s", bytes, hipGetErrorString(e));
            return RN_E_NOMEM;
        }
        if (ft->d_val) (void)hipFree(ft->d_val);   // (ft_check_labels has drained the stream: nothing still reads it)
        ft->d_val = p;
        ft->val_cap = points;
    }
    return RN_OK;
}

// One validation point on the trainer's stream, behind the step that made the global step `step`: the set in chunks of max_batch
// through the forward-only pass, each chunk reduced into the point's tables, then the closer and the snapshot.
static int ft_enqueue_point(rn_ft* ft, const FtValidation& v, const FtValTables& t, int point, int64_t step) {
    FtItemArgs a = ft->item;
    a.feats = v.d_feats;
    a.labels = v.d_labels;
    a.index = nullptr;
    a.l2sum = nullptr;
    a.probs = ft->d_probs;
    a.ids = ft->d_ids;
    int32_t* conf = t.conf + static_cast<size_t>(point) * ft->nc * ft->nc;
    int rc;
    for (int64_t i = 0; i < v.n; i += ft->max_batch) {
        const int m = static_cast<int>(std::min<int64_t>(ft->max_batch, v.n - i));
        a.base = i;
        if ((rc = ft_enqueue_pass(ft, a, nullptr, m)) != RN_OK) return rc;
        const FtValChunkArgs c{ft->d_ids, ft->d_item_loss, v.d_labels + i, m, ft->nc, conf, t.ce + point};
        hipLaunchKernelGGL(ft_val_chunk_kernel, dim3(1), dim3(FT_VAL_NT), 0, ft->stream, c);
        RN_CHECK_LAUNCH();
    }
    const FtValCloseArgs c{ft->d_P, ft->n_param, ft->nc, ft->cfg.l2_coeff, static_cast<long long>(v.n), static_cast<long long>(step),
                           t.ce + point, conf, t.loss + point, t.flag + point, ft->d_best};
    hipLaunchKernelGGL(ft_val_close_kernel, dim3(1), dim3(FT_NT), 0, ft->stream, c);
    RN_CHECK_LAUNCH();
    const int quads = ft->n_param / 4;
    hipLaunchKernelGGL(ft_val_snapshot_kernel, dim3((quads + 255) / 256), dim3(256), 0, ft->stream, t.flag + point, ft->d_P, ft->d_P_best,
                       quads);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// A per-step feature provider of the step loop (rn_ft_run_views).  Without one a step reads the resident d_feats through d_index.
//   prepare  once, behind the loop's checks and before anything of the run is enqueued: what the provider allocates and gathers
//   before   in front of step s at global step g: makes the step's features and names them in the pass's arguments (feats, labels,
//            index, base); the trainer's stream must wait for them
//   after    behind the pass of step s: the features have been read
struct FtFeed {
    std::function<int()> prepare;
    std::function<int(int s, int64_t g, FtItemArgs& a)> before;
    std::function<int(int s)> after;
};

// The step loop of rn_ft_run, rn_ft_run_validated and rn_ft_run_views (`who` in the messages): the checks, `steps` training passes
// enqueued back to back, with `v` a validation point behind every step the schedule names, and one synchronisation at the end.
static int ft_run_loop(rn_ft* ft, const char* who, const float* d_feats, const int32_t* d_labels, int64_t n_items, const int32_t* d_index,
                       int batch, int steps, float* losses, const FtValidation* v, const FtFeed* feed = nullptr) {
    if (batch < 1 || batch > ft->max_batch) {
        rn_set_error("%s: batch = %d out of range (1..%d)", who, batch, ft->max_batch);
        return RN_E_RANGE;
    }
    if (steps < 1 || n_items < 1) {
        rn_set_error("%s: steps = %d, n_items = %lld", who, steps, static_cast<long long>(n_items));
        return RN_E_RANGE;
    }
    if (v && (v->every < 1 || v->n < 1)) {
        rn_set_error("%s: val_every = %d, n_val = %lld", who, v->every, static_cast<long long>(v->n));
        return RN_E_RANGE;
    }
    DeviceGuard guard(ft->device);
    (void)hipGetLastError();
    int rc;
    if ((rc = ft_check_labels(ft, who, d_labels, n_items, d_index, static_cast<size_t>(steps) * batch)) != RN_OK) return rc;
    FtValTables t{};
    int points = 0;
    if (v) {
        const std::string vwho = std::string(who) + ": validation";
        if ((rc = ft_check_labels(ft, vwho.c_str(), v->d_labels, v->n, nullptr, 0)) != RN_OK) return rc;
        points = ft_count_points(ft->cfg.start_step + ft->steps_done, steps, v->every, nullptr, 0);
        if ((rc = ft_val_reserve(ft, points)) != RN_OK) return rc;
        t = ft_val_tables(ft, ft->d_val, points);
    }
    if (steps > ft->losses_cap) {
        // the old buffer and its size go before the allocation that may fail: a failed grow leaves no stale pointer
        if (ft->d_losses) RN_HIP(hipFree(ft->d_losses));
        ft->d_losses = nullptr;
        ft->losses_cap = 0;
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&ft->d_losses), static_cast<size_t>(steps) * 4));
        ft->losses_cap = steps;
    }
    FtItemArgs a = ft->item;
    a.feats = d_feats;
    a.labels = d_labels;
    a.index = d_index;
    a.l2sum = ft->d_l2sum;
    a.probs = nullptr;
    a.ids = nullptr;
    FtUpdateArgs u = ft->upd;
    u.n = batch;
    const double b1 = ft->cfg.beta1, b2 = ft->cfg.beta2;
    const bool dropping = ft->drop.thr != 0;
    if (feed && (rc = feed->prepare()) != RN_OK) return rc;
    if ((rc = ft->timer.start(ft->stream)) != RN_OK) return rc;
    if (v) RN_HIP(hipMemsetAsync(ft->d_val, 0, t.bytes, ft->stream));
    int point = 0;
    for (int s = 0; s < steps; ++s) {
        const int64_t t1 = ft->steps_done + 1;
        const double lr = ft_learn_rate(ft->cfg, ft->cfg.start_step + ft->steps_done);
        u.lr_t = static_cast<float>(lr * std::sqrt(1.0 - std::pow(b2, static_cast<double>(t1))) / (1.0 - std::pow(b1, static_cast<double>(t1))));
        u.loss_out = ft->d_losses + s;
        a.base = static_cast<int64_t>(s) * batch;
        if (dropping) {
            const uint64_t gstep = static_cast<uint64_t>(ft->cfg.start_step + ft->steps_done);
            a.drop = ft->drop;
            a.drop.step_lo = static_cast<uint32_t>(gstep);
            a.drop.step_hi = static_cast<uint32_t>(gstep >> 32);
        }
        if (feed && (rc = feed->before(s, ft->cfg.start_step + ft->steps_done, a)) != RN_OK) return rc;
        if ((rc = ft_enqueue_pass(ft, a, &u, batch)) != RN_OK) return rc;
        if (feed && (rc = feed->after(s)) != RN_OK) return rc;
        ++ft->steps_done;
        if (v) {
            const int64_t g = ft->cfg.start_step + ft->steps_done;
            if (ft_is_point(g, v->every, s == steps - 1) && (rc = ft_enqueue_point(ft, *v, t, point++, g)) != RN_OK) return rc;
        }
    }
    if ((rc = ft->timer.stop(ft->stream)) != RN_OK) return rc;
    RN_HIP(hipMemcpyAsync(losses, ft->d_losses, static_cast<size_t>(steps) * 4, hipMemcpyDeviceToHost, ft->stream));
    if (v) {
        const size_t cc = static_cast<size_t>(ft->nc) * ft->nc;
        RN_HIP(hipMemcpyAsync(v->losses, t.loss, static_cast<size_t>(points) * 4, hipMemcpyDeviceToHost, ft->stream));
        RN_HIP(hipMemcpyAsync(v->confusion, t.conf, static_cast<size_t>(points) * cc * 4, hipMemcpyDeviceToHost, ft->stream));
        RN_HIP(hipMemcpyAsync(&ft->best, ft->d_best, sizeof(FtBestDev), hipMemcpyDeviceToHost, ft->stream));
    }
    RN_HIP(hipStreamSynchronize(ft->stream));
    return RN_OK;
}

extern "C" int rn_ft_run(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n_items, const int32_t* d_index, int batch,
                         int steps, float* losses) {
    if (!ft || !d_feats || !d_labels || !d_index || !losses) {
        rn_set_error("rn_ft_run: null argument");
        return RN_E_INVALID;
    }
    return ft_run_loop(ft, "rn_ft_run", d_feats, d_labels, n_items, d_index, batch, steps, losses, nullptr);
}

extern "C" int rn_ft_run_validated(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n_items, const int32_t* d_index,
                                   int batch, int steps, float* losses, const float* d_val_feats, const int32_t* d_val_labels,
                                   int64_t n_val, int val_every, float* val_losses, int32_t* val_confusion) {
    if (!ft || !d_feats || !d_labels || !d_index || !losses || !d_val_feats || !d_val_labels || !val_losses || !val_confusion) {
        rn_set_error("rn_ft_run_validated: null argument");
        return RN_E_INVALID;
    }
    const FtValidation v{d_val_feats, d_val_labels, n_val, val_every, val_losses, val_confusion};
    return ft_run_loop(ft, "rn_ft_run_validated", d_feats, d_labels, n_items, d_index, batch, steps, losses, &v);
}

// what a run on fresh views needs beside the trainer's own memory (FtFeed::prepare: the loop's checks have passed and
// ft_check_labels has drained the stream); a failed allocation leaves the trainer as it was.  Then the call's labels are gathered
// in slot order on the trainer's stream, in front of the first step.
static int ft_views_prepare(rn_ft* ft, const int32_t* d_labels, const int32_t* d_index, size_t count) {
    int rc;
    const size_t per = ft->depth == 3 ? static_cast<size_t>(ft->sd.S6) * ft->sd.S6 * LB_CIN7 : static_cast<size_t>(ft->sd.S7) * ft->sd.S7 * LB_C;
    for (int k = 0; k < FT_VIEW_SLOTS; ++k) {
        if (!ft->d_vfeat[k] && (rc = ft_zeroed(ft, static_cast<size_t>(ft->max_batch) * per, &ft->d_vfeat[k])) != RN_OK) return rc;
        if (!ft->ev_feats[k]) RN_HIP(hipEventCreateWithFlags(&ft->ev_feats[k], hipEventDisableTiming));
        if (!ft->ev_read[k]) RN_HIP(hipEventCreateWithFlags(&ft->ev_read[k], hipEventDisableTiming));
    }
    if (!ft->d_iota) {
        std::vector<int32_t> iota(static_cast<size_t>(ft->max_batch));
        for (size_t i = 0; i < iota.size(); ++i) iota[i] = static_cast<int32_t>(i);
        if ((rc = ft_upload(ft, iota.data(), iota.size(), &ft->d_iota)) != RN_OK) return rc;
    }
    if (count > ft->glabels_cap) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * 4);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rn_set_error("rn_ft_run_views: hipMalloc(%zu bytes of labels) failed: %s", count * 4, hipGetErrorString(e));
            return RN_E_NOMEM;
        }
        if (ft->d_glabels) (void)hipFree(ft->d_glabels);
        ft->d_glabels = static_cast<int32_t*>(p);
        ft->glabels_cap = count;
    }
    hipLaunchKernelGGL(ft_gather_labels_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, ft->stream, d_labels,
                       d_index, static_cast<int64_t>(count), ft->d_glabels);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

extern "C" int rn_ft_run_views(rn_ft* ft, rn_handle* h, const rn_views* v, const int32_t* d_labels, int64_t n_items, const int32_t* d_index,
                               int batch, int steps, uint64_t view_seed, unsigned flags, float* losses, const float* d_val_feats,
                               const int32_t* d_val_labels, int64_t n_val, int val_every, float* val_losses, int32_t* val_confusion) {
    const char* who = "rn_ft_run_views";
    if (!ft || !h || !v || !d_labels || !d_index || !losses) {
        rn_set_error("%s: null argument", who);
        return RN_E_INVALID;
    }
    const bool validated = d_val_feats || d_val_labels || n_val || val_every || val_losses || val_confusion;
    if (validated && (!d_val_feats || !d_val_labels || !val_losses || !val_confusion)) {
        rn_set_error("%s: validation takes all six of its arguments, or none", who);
        return RN_E_INVALID;
    }
    if (h->device != ft->device) {
        rn_set_error("%s: the handle is on device %d, the trainer on device %d", who, h->device, ft->device);
        return RN_E_INVALID;
    }
    if (h->bnstats) {
        rn_set_error("%s: the features are those of the inference graph; this handle normalises with batch moments (RN_FLAG_BATCH_STATS)", who);
        return RN_E_STATE;
    }
    int side = 0, channels = 0;
    int rc = rn_features_depth_shape(h, ft->depth, &side, &channels);
    if (rc != RN_OK) return rc;
    const int want_side = ft->depth == 3 ? ft->sd.S6 : ft->sd.S7, want_c = ft->depth == 3 ? LB_CIN7 : LB_C;
    if (side != want_side || channels != want_c) {
        rn_set_error("%s: the handle's depth-%d feature is %d x %d x %d, the trainer's %d x %d x %d", who, ft->depth, side, side, channels,
                     want_side, want_side, want_c);
        return RN_E_INVALID;
    }
    if (batch > h->max_batch) {
        rn_set_error("%s: batch = %d exceeds the handle's max_batch %d", who, batch, h->max_batch);
        return RN_E_RANGE;
    }
    if (n_items != v->n_items) {
        rn_set_error("%s: n_items = %lld, the views hold %lld photographs", who, static_cast<long long>(n_items),
                     static_cast<long long>(v->n_items));
        return RN_E_INVALID;
    }
    // (n = 1 and step 0 here: the loop checks the batch, and the trainer's global step is never negative)
    if ((rc = rn_views_check(who, h, v, d_index, 1, 0, flags, h->d_in_u8)) != RN_OK) return rc;
    FtFeed feed;
    feed.prepare = [&]() { return ft_views_prepare(ft, d_labels, d_index, static_cast<size_t>(steps) * batch); };
    feed.before = [&](int s, int64_t g, FtItemArgs& a) -> int {
        int rc2;
        const int k = s % FT_VIEW_SLOTS;
        // the pass that read slot k last (step s - FT_VIEW_SLOTS of this call) must be through with it
        if (s >= FT_VIEW_SLOTS) RN_HIP(hipStreamWaitEvent(h->stream, ft->ev_read[k], 0));
        if ((rc2 = rn_views_enqueue(h, v, d_index, static_cast<int64_t>(s) * batch, batch, view_seed, g, flags, h->d_in_u8)) != RN_OK) return rc2;
        if ((rc2 = rn_features_depth_u8_device(h, ft->depth, h->d_in_u8, batch, ft->d_vfeat[k])) != RN_OK) return rc2;
        RN_HIP(hipEventRecord(ft->ev_feats[k], h->stream));
        RN_HIP(hipStreamWaitEvent(ft->stream, ft->ev_feats[k], 0));
        a.feats = ft->d_vfeat[k];
        a.labels = ft->d_glabels + static_cast<int64_t>(s) * batch;
        a.index = ft->d_iota;
        a.base = 0;
        return RN_OK;
    };
    feed.after = [&](int s) -> int {
        RN_HIP(hipEventRecord(ft->ev_read[s % FT_VIEW_SLOTS], ft->stream));
        return RN_OK;
    };
    if (!validated) return ft_run_loop(ft, who, nullptr, d_labels, n_items, d_index, batch, steps, losses, nullptr, &feed);
    const FtValidation val{d_val_feats, d_val_labels, n_val, val_every, val_losses, val_confusion};
    return ft_run_loop(ft, who, nullptr, d_labels, n_items, d_index, batch, steps, losses, &val, &feed);
}

extern "C" int rn_ft_val_points(const rn_ft* ft, int steps, int val_every, int64_t* point_steps, int cap) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    if (steps < 1 || val_every < 1) {
        rn_set_error("rn_ft_val_points: steps = %d, val_every = %d", steps, val_every);
        return RN_E_RANGE;
    }
    return ft_count_points(ft->cfg.start_step + ft->steps_done, steps, val_every, point_steps, cap);
}

extern "C" int rn_ft_best(const rn_ft* ft, int64_t* step, int64_t* correct, int64_t* n_val) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    if (!ft->best.valid) {
        rn_set_error("rn_ft_best: no validation point has been taken on this trainer");
        return RN_E_STATE;
    }
    if (step) *step = ft->best.step;
    if (correct) *correct = ft->best.correct;
    if (n_val) *n_val = ft->best.n_val;
    return RN_OK;
}

extern "C" int rn_ft_eval(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n, float* mean_loss, float* probs,
                          int64_t* ids) {
    if (!ft || !d_feats || n < 1) {
        rn_set_error("rn_ft_eval: bad argument");
        return RN_E_INVALID;
    }
    if (mean_loss && !d_labels) {
        rn_set_error("rn_ft_eval: a loss needs labels");
        return RN_E_INVALID;
    }
    DeviceGuard guard(ft->device);
    (void)hipGetLastError();
    int rc;
    if (d_labels && (rc = ft_check_labels(ft, "rn_ft_eval", d_labels, n, nullptr, 0)) != RN_OK) return rc;
    FtItemArgs a = ft->item;
    a.feats = d_feats;
    a.labels = d_labels;
    a.index = nullptr;
    a.l2sum = nullptr;
    a.probs = ft->d_probs;
    a.ids = ft->d_ids;
    double ce = 0.0;
    std::vector<double> il(static_cast<size_t>(ft->max_batch));
    for (int64_t i = 0; i < n; i += ft->max_batch) {
        const int m = static_cast<int>(std::min<int64_t>(ft->max_batch, n - i));
        a.base = i;
        if ((rc = ft_enqueue_pass(ft, a, nullptr, m)) != RN_OK) return rc;
        if (probs) RN_HIP(hipMemcpyAsync(probs + i * ft->nc, ft->d_probs, static_cast<size_t>(m) * ft->nc * 4, hipMemcpyDeviceToHost, ft->stream));
        if (ids) RN_HIP(hipMemcpyAsync(ids + i, ft->d_ids, static_cast<size_t>(m) * 8, hipMemcpyDeviceToHost, ft->stream));
        if (mean_loss) RN_HIP(hipMemcpyAsync(il.data(), ft->d_item_loss, static_cast<size_t>(m) * 8, hipMemcpyDeviceToHost, ft->stream));
        RN_HIP(hipStreamSynchronize(ft->stream));
        if (mean_loss)
            for (int k = 0; k < m; ++k) ce += il[k];
    }
    if (mean_loss) {
        // the L2 term over the trained variables, as the training loss has it
        std::vector<float> P(static_cast<size_t>(ft->n_param));
        RN_HIP(hipMemcpy(P.data(), ft->d_P, P.size() * 4, hipMemcpyDeviceToHost));
        double s2 = 0.0;
        for (float v : P) s2 += static_cast<double>(v) * v;
        *mean_loss = static_cast<float>(ce / static_cast<double>(n) + 0.5 * static_cast<double>(ft->cfg.l2_coeff) * s2);
    }
    return RN_OK;
}

extern "C" int rn_ft_var_count(const rn_ft* ft) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    return static_cast<int>(ft->vars.size());
}

extern "C" int rn_ft_var_info(const rn_ft* ft, int var, char* name, size_t name_cap, int64_t* count) {
    if (!ft || var < 0 || var >= static_cast<int>(ft->vars.size())) {
        rn_set_error("rn_ft_var_info: variable %d out of range", var);
        return RN_E_RANGE;
    }
    const FtVarHost& v = ft->vars[var];
    if (name && name_cap) {
        std::strncpy(name, v.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (count) *count = v.count;
    return RN_OK;
}

extern "C" int rn_ft_read(rn_ft* ft, int what, int var, float* out, size_t cap) {
    if (!ft || !out || var < 0 || var >= static_cast<int>(ft->vars.size())) {
        rn_set_error("rn_ft_read: bad argument (variable %d)", var);
        return RN_E_RANGE;
    }
    if (what == RN_FT_BEST && !ft->best.valid) {
        rn_set_error("rn_ft_read: RN_FT_BEST before any validation point has been taken on this trainer");
        return RN_E_STATE;
    }
    const float* src = what == RN_FT_PARAM ? ft->d_P : what == RN_FT_GRAD ? ft->d_G : what == RN_FT_ADAM_M ? ft->d_M :
                       what == RN_FT_ADAM_V ? ft->d_V : what == RN_FT_BEST ? ft->d_P_best : nullptr;
    if (!src) {
        rn_set_error("rn_ft_read: what = %d is none of RN_FT_PARAM, RN_FT_GRAD, RN_FT_ADAM_M, RN_FT_ADAM_V, RN_FT_BEST", what);
        return RN_E_INVALID;
    }
    const FtVarHost& v = ft->vars[var];
    if (cap < static_cast<size_t>(v.count)) {
        rn_set_error("rn_ft_read: buffer too small (%zu < %d elements)", cap, v.count);
        return RN_E_RANGE;
    }
    DeviceGuard guard(ft->device);
    RN_HIP(hipStreamSynchronize(ft->stream));
    RN_HIP(hipMemcpy(out, src + v.off, static_cast<size_t>(v.count) * 4, hipMemcpyDeviceToHost));
    return RN_OK;
}

extern "C" int rn_ft_last_run_ms(rn_ft* ft, float* ms) {
    return rn_timer::read("rn_ft_last_run_ms", ft, ft ? &ft->timer : nullptr, "no rn_ft_run has completed on this trainer",
                          ft ? ft->device : 0, ms);
}

extern "C" int64_t rn_ft_step_count(const rn_ft* ft) { return ft ? ft->cfg.start_step + ft->steps_done : -1; }

// ---- dropout
extern "C" int rn_ft_set_dropout(rn_ft* ft, float rate, uint64_t seed) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    if (!(rate >= 0.f && rate < 1.f)) {
        rn_set_error("rn_ft_set_dropout: rate = %g outside [0, 1)", static_cast<double>(rate));
        return RN_E_RANGE;
    }
    if (rate > 0.f && ft->depth == 3 && !ft->d_x6d) {
        DeviceGuard guard(ft->device);
        const size_t n6 = static_cast<size_t>(ft->sd.S6) * ft->sd.S6 * LB_CIN7;
        int rc = ft_zeroed(ft, static_cast<size_t>(ft->max_batch) * n6, &ft->d_x6d);
        if (rc != RN_OK) {
            (void)hipGetLastError();
            return rc;
        }
    }
    ft->drop_rate = rate;
    ft->drop_seed = seed;
    ft->drop = RnDropout{};
    ft->drop.key0 = static_cast<uint32_t>(seed);
    ft->drop.key1 = static_cast<uint32_t>(seed >> 32);
    ft->drop.thr = static_cast<uint32_t>(std::ceil(static_cast<double>(rate) * 16777216.0));
    ft->drop.scale = 1.0f / (1.0f - rate);
    return RN_OK;
}

extern "C" int rn_ft_dropout(const rn_ft* ft, float* rate, uint64_t* seed) {
    if (!ft) {
        rn_set_error("null trainer");
        return RN_E_INVALID;
    }
    if (rate) *rate = ft->drop_rate;
    if (seed) *seed = ft->drop_seed;
    return RN_OK;
}

extern "C" int rn_ft_dropout_mask(rn_ft* ft, int site, int64_t step, int slot, int64_t count, uint8_t* keep) {
    if (!ft || !keep) {
        rn_set_error("rn_ft_dropout_mask: null argument");
        return RN_E_INVALID;
    }
    const int n_dense = ft->item.n_dense;
    if (site < (ft->depth == 3 ? 0 : 1) || site >= RN_DROP_SITE_DENSE + n_dense) {
        rn_set_error("rn_ft_dropout_mask: a depth-%d trainer with %d dense blocks has no site %d", ft->depth, n_dense, site);
        return RN_E_INVALID;
    }
    const int64_t size = site == RN_DROP_SITE_X6     ? static_cast<int64_t>(ft->sd.S6) * ft->sd.S6 * LB_CIN7
                         : site == RN_DROP_SITE_FLAT ? static_cast<int64_t>(ft->sd.S9) * ft->sd.S9 * LB_C
                                                     : ft->item.nout[site - RN_DROP_SITE_DENSE];
    if (count < 1 || count > size) {
        rn_set_error("rn_ft_dropout_mask: count = %lld outside [1, %lld] of site %d", static_cast<long long>(count),
                     static_cast<long long>(size), site);
        return RN_E_RANGE;
    }
    if (slot < 0 || slot >= ft->max_batch) {
        rn_set_error("rn_ft_dropout_mask: slot = %d outside [0, %d)", slot, ft->max_batch);
        return RN_E_RANGE;
    }
    if (step < 0) {
        rn_set_error("rn_ft_dropout_mask: step = %lld", static_cast<long long>(step));
        return RN_E_RANGE;
    }
    DeviceGuard guard(ft->device);
    (void)hipGetLastError();
    RnDropout d = ft->drop;
    d.step_lo = static_cast<uint32_t>(static_cast<uint64_t>(step));
    d.step_hi = static_cast<uint32_t>(static_cast<uint64_t>(step) >> 32);
    uint8_t* d_keep = nullptr;
    RN_HIP(hipMalloc(reinterpret_cast<void**>(&d_keep), static_cast<size_t>(count)));
    const int blocks = static_cast<int>(std::min<int64_t>((count + 255) / 256, 4096));
    hipLaunchKernelGGL(ft_mask_kernel, dim3(blocks), dim3(256), 0, ft->stream, d, site, slot, count, d_keep);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(keep, d_keep, static_cast<size_t>(count), hipMemcpyDeviceToHost, ft->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ft->stream);
    (void)hipFree(d_keep);
    if (e != hipSuccess) {
        rn_set_error("rn_ft_dropout_mask: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return RN_E_HIP;
    }
    return RN_OK;
}
