// Stage 7 of a depth-3 fine-tuning step: the first step of the last conv block, trained from a cached s6.bn (rn_ft_create_depth).
//
// Frozen: stages 0-6.  The feature is x6 = s6.bn [S6, S6, 128]; nothing below it is trained, so no data gradient leaves this file.
// Trained here, in front of the 19 variables of rn_finetune.hip: conv 7's kernel W7 [3][3][128][16] and its BN's gamma7, beta7.
//
// Forward, per item, float32:
//   pre[p, co]  = sum_{k, ci} x6[p + k, ci] W7[k, ci, co]            conv 3x3 VALID, C7 = S6 - 2
//   pool[q, co] = 1/16 sum over the 4 x 4 window at 2 q of relu6(pre)  avg-pool 4/2 VALID, S7 = (C7 - 4) / 2 + 1
//   xh7 = (pool - mean7) rsqrt(var7 + eps);  x7 = xh7 gamma7 + beta7    the inference BN, gamma and beta trainable
// Adjoint, TensorFlow's rules as rn_finetune.hip states them.  The item kernel of rn_finetune.hip forms g7 = dL/dx7 (conv 8's adjoint
// plus the transpose of stage 9's skip resize), d gamma7 = sum g7 xh7 and d beta7 = sum g7, and hands dpool = g7 gamma7 rsqrt(var7 + eps)
// to this file:
//   dconv7[p, co] = [0 < pre[p, co] < 6] 1/16 sum of dpool over the pooled windows that cover p     (Relu6Grad is strict; at an odd C7
//                   the last conv row and column are covered by no window and get zero)
//   dW7[k, ci, co] = sum_p x6[p + k, ci] dconv7[p, co]
//
// Two launches, each on a grid of (band, item), 8 waves per workgroup, both on v_mfma_f32_16x16x4_f32 (exact float32, one rounding
// per product: a k-ordered fmaf chain):
//   ft7_fwd_kernel  a band is rows_f pooled rows = 2 rows_f + 2 conv rows (bands overlap by the pool's halo of two conv rows; both
//                   neighbours compute them in the same order and store the same bits).  W7 from the master parameters in LDS
//                   (73.7 KB); a wave takes (2 conv rows) x (16 pixels) x (16 couts) units: A = pixels x 4 channels, B = 4 channels x
//                   couts, K runs over (ky, kx, ci) in chains of 16 channels whose results are added in float64 (so that pre is the
//                   float32 rounding of its exact value, and its ReLU6 mask the reference's).  pre goes to the step's workspace, then the band pools its rows and writes xh7, x7.
//   ft7_bwd_kernel  a band is rows_b conv rows, owned by it alone.  It first turns its rows of pre into dconv7 in place, then
//                   wave w accumulates the nine 16 (ci of block w) x 16 (co) tiles dW7[k, 16 w .., ..]: A = x6[p + k, ci] (x6 is NHWC:
//                   the 16 ci of a fragment are 64 contiguous bytes), B = dconv7[p, co], K runs over 4 consecutive positions of a
//                   conv row.  Every conv row is summed apart and then joins the band's total (the two-level sum of wgrad16).  One
//                   partial [9][128][16] per (item, band); ft_update_kernel sums them over bands, then over items, in index order (in float64).
// No atomics: the same minibatch gives the same bits.  The pool's window sum and its adjoint's sum over the covering windows are the
// functions of rn_lastblock.h that stages 8 and 9 use; the float64-chained convolution is this file's own.
#include "rn_finetune7.h"
#include "rn_stage.h"

#include <algorithm>

using namespace rnk;

namespace {

constexpr int F7_NT = 512;           // threads of both workgroups: 8 waves
constexpr int F7_NW = F7_NT / 64;
constexpr int F7_R = 2;              // conv rows of a forward unit

__global__ __launch_bounds__(F7_NT) void ft7_fwd_kernel(const Ft7Args a) {
    extern __shared__ __attribute__((aligned(16))) float wl[];        // W7 [9 * 128][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x, b = blockIdx.y;
    const int i16 = lane & 15, kg = lane >> 4, co = lane & 15;
    const int S6 = a.S6, C7 = a.C7, S7 = a.S7;
    const int64_t item = a.index ? static_cast<int64_t>(a.index[a.base + b]) : a.base + b;
    const float* x6 = a.feats + item * S6 * S6 * LB_CIN7;
    float* pre = a.pre + static_cast<int64_t>(b) * C7 * C7 * LB_C;
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.P + a.o_w7);
        for (int i = tid; i < FT7_W / 4; i += F7_NT) reinterpret_cast<f32x4*>(wl)[i] = src[i];
    }
    __syncthreads();
    const int p0 = band * a.rows_f, p1 = min(S7, p0 + a.rows_f);
    const int yb = 2 * p0, nrows = 2 * (p1 - p0) + 2;                  // conv rows [yb, yb + nrows), yb + nrows <= 2 S7 + 2 <= C7
    const int ngrp = nrows / F7_R, ntile = (C7 + 15) / 16;
    for (int u = wave; u < ngrp * ntile; u += F7_NW) {
        const int y0 = yb + (u / ntile) * F7_R, x0 = (u % ntile) * 16;
        const int X = min(x0 + i16, C7 - 1);
        // A float32 chain over all K = 1152 products misses the float64 pre-activation by up to 1e-6 (3.5e-7 of sum |x w|), which
        // puts more positions on the other side of a ReLU6 kink than the float32 rounding of the exact sum does.  So a chain is 16
        // channels of one tap long, and the 72 chains of a pre-activation are added in float64 (the vector unit is idle here).
        double acc[F7_R][4];
#pragma unroll
        for (int r = 0; r < F7_R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r][j] = 0.0;
        // input row y0 + rr feeds the conv rows y0 + rr - ky of the unit; the last one read is y0 + F7_R + 1 <= C7 + 1 = S6 - 1.
        // A conv row's sum runs in the order (ky, kx, ci) whichever unit and band computes it.
#pragma unroll
        for (int rr = 0; rr < F7_R + 2; ++rr) {
            const float* prow = x6 + (static_cast<int64_t>(y0 + rr) * S6 + X) * LB_CIN7 + 4 * kg;
            for (int kx = 0; kx < 3; ++kx) {
                const float* px = prow + kx * LB_CIN7;
#pragma unroll 2
                for (int c16 = 0; c16 < LB_CIN7 / 16; ++c16) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(px + c16 * 16);
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int yi = rr - ky;
                        if (yi < 0 || yi >= F7_R) continue;
                        const float* wt = wl + (ky * 3 + kx) * LB_CIN7 * LB_C + (4 * kg + c16 * 16) * LB_C + co;
                        f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) t = __builtin_amdgcn_mfma_f32_16x16x4f32(v[q], wt[q * LB_C], t, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[yi][j] += static_cast<double>(t[j]);
                    }
                }
            }
        }
        // C/D: pixel 4 (lane >> 4) + j, cout lane & 15
#pragma unroll
        for (int yi = 0; yi < F7_R; ++yi)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + 4 * kg + j;
                if (x < C7) pre[(static_cast<int64_t>(y0 + yi) * C7 + x) * LB_C + co] = static_cast<float>(acc[yi][j]);
            }
    }
    __syncthreads();
    // the band's pooled rows: every conv row they read was written by this workgroup
    const float* F = a.F + a.f_bn7;
    const int64_t ob = static_cast<int64_t>(b) * S7 * S7 * LB_C;
    for (int i = tid; i < (p1 - p0) * S7 * LB_C; i += F7_NT) {
        const int c = i & 15, p = i >> 4, y = p0 + p / S7, x = p % S7;
        const float t = pool_relu6_sum(pre, C7, y, x, c);
        const float xh = (t * (1.0f / 16.0f) - F[c]) * F[LB_C + c];
        const int64_t o = ob + (static_cast<int64_t>(y) * S7 + x) * LB_C + c;
        a.xh7[o] = xh;
        a.x7[o] = fmaf(xh, a.P[a.o_g7 + c], a.P[a.o_b7 + c]);
    }
}

__global__ __launch_bounds__(F7_NT) void ft7_bwd_kernel(const Ft7Args a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x, b = blockIdx.y;
    const int kg = lane >> 4, co = lane & 15;
    const int S6 = a.S6, C7 = a.C7, S7 = a.S7;
    const int64_t item = a.index ? static_cast<int64_t>(a.index[a.base + b]) : a.base + b;
    const float* x6 = a.feats + item * S6 * S6 * LB_CIN7;
    float* dc = a.pre + static_cast<int64_t>(b) * C7 * C7 * LB_C;
    const float* dp = a.dpool + static_cast<int64_t>(b) * S7 * S7 * LB_C;
    const int y0 = band * a.rows_b, y1 = min(C7, y0 + a.rows_b);
    // ---- the pool adjoint and the ReLU6 mask, in place over the band's rows of pre: dL/dconv7
    for (int i = tid; i < (y1 - y0) * C7 * LB_C; i += F7_NT) {
        const int c = i & 15, p = i >> 4, Y = y0 + p / C7, X = p % C7;
        const float t = pool_cover_sum(dp, S7, Y, X, c);
        const int64_t o = (static_cast<int64_t>(Y) * C7 + X) * LB_C + c;
        dc[o] = relu6_passes(dc[o]) ? t * (1.0f / 16.0f) : 0.f;
    }
    __syncthreads();
    // ---- dW7[k, 16 wave + i, co]: A = x6[p + k, ci] (lane: ci = lane & 15, position lane >> 4), B = dconv7[p, co] (lane: position
    // lane >> 4, co = lane & 15); C/D: ci 4 (lane >> 4) + j, co lane & 15
    const float* xa = x6 + wave * 16 + (lane & 15);
    f32x4 tot[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) tot[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int Y = y0; Y < y1; ++Y) {
        f32x4 row[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) row[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int x0 = 0; x0 < C7; x0 += 4) {
            const int x = x0 + kg;
            const int xc = min(x, C7 - 1);                             // (a position past the row: B = 0, A read inside the row)
            const float bv = x < C7 ? dc[(static_cast<int64_t>(Y) * C7 + xc) * LB_C + co] : 0.f;
            float av[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) av[ky * 3 + kx] = xa[(static_cast<int64_t>(Y + ky) * S6 + xc + kx) * LB_CIN7];
#pragma unroll
            for (int k = 0; k < 9; ++k) row[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], bv, row[k], 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) tot[k] += row[k];
    }
    float* out = a.part + (static_cast<int64_t>(b) * a.bands_b + band) * FT7_W;
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(k * LB_CIN7 + wave * 16 + 4 * kg + j) * LB_C + co] = tot[k][j];
}

}  // namespace

// Bands per item: enough workgroups for the 256 CUs at the reference's batch of 45 (6 x 45 = 270), fewer for larger batches (a
// partial is 73.7 KB), at least two pooled rows per forward band (its halo is two conv rows more).
void rn_ft7_bands(int batch, int C7, int S7, int* bands_f, int* rows_f, int* bands_b, int* rows_b) {
    const int want = std::max(1, std::min((256 + batch - 1) / batch, (S7 + 1) / 2));
    *rows_f = (S7 + want - 1) / want;
    *bands_f = (S7 + *rows_f - 1) / *rows_f;
    *rows_b = (C7 + want - 1) / want;
    *bands_b = (C7 + *rows_b - 1) / *rows_b;
}

const char* rn_ft7_geometry_reason(int S6, int C7, int S7) {
    if (C7 != S6 - 2 || C7 < 4 || S7 != (C7 - 4) / 2 + 1) return "stage 7 is not conv 3x3 VALID + avg-pool 4/2";
    return nullptr;
}

int rn_ft7_forward(hipStream_t stream, const Ft7Args& a, int batch) {
    int rc = rn_allow_big_lds<ft7_fwd_kernel>();
    if (rc != RN_OK) return rc;
    hipLaunchKernelGGL(ft7_fwd_kernel, dim3(a.bands_f, batch), dim3(F7_NT), FT7_W * sizeof(float), stream, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

int rn_ft7_backward(hipStream_t stream, const Ft7Args& a, int batch) {
    hipLaunchKernelGGL(ft7_bwd_kernel, dim3(a.bands_b, batch), dim3(F7_NT), 0, stream, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}
