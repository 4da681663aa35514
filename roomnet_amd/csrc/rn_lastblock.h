// The float32 steps of the last conv block (stages 7-9: conv 3x3 VALID 16 -> 16, ReLU6, avg-pool 4/2, BN; stage 9 adds the
// legacy-bilinear resize of s7.bn) and of the dense head, forward and adjoint, one output element at a time.  Shared by grad-CAM
// (rn_gradcam.hip) and the fine-tuning trainers (rn_finetune.hip, rn_finetune7.hip), so that a rule of the mathematics -- the strict
// Relu6Grad, the row an odd conv side leaves uncovered, the transpose of the legacy resize -- is stated once.
//
// Every function is one element's sum and nothing else: the callers keep their loops, their buffers and their epilogues (the 1/16 of
// the pool, the ReLU6 mask, the BN factors), because those differ between the callers in how they round.  The functions are
// __forceinline__: a caller's epilogue contracts with the sum exactly as it did when the loop was written out in place.
// Offsets inside one image's tensor fit an int: the largest, s6.bn at side 600, is 2.7e6 elements.
#pragma once
#include "rn_stage.h"

namespace rnk {

constexpr int LB_C = 16;             // channels of the last block (s7 .. s9)
constexpr int LB_CIN7 = 128;         // channels of s6.bn, conv 7's input
constexpr int LB_HMAX = 64;          // widest dense layer (rn_tail_graph_reason enforces nout <= 64)

// TensorFlow's Relu6Grad: strictly inside (0, 6)
__device__ __forceinline__ bool relu6_passes(float v) { return v > 0.f && v < 6.f; }

// pooled rows (or columns) whose 4 x 4 / stride-2 window covers conv row Y.  At an odd conv side VALID pooling covers the last row by
// none: lo > hi
__device__ __forceinline__ void pool_span(int Y, int So, int* lo, int* hi) {
    *lo = Y < 3 ? 0 : (Y - 2) / 2;
    *hi = min(So - 1, Y / 2);
}

// conv3x3 VALID 16 -> 16 pre-activation of one output element: in [S][S][16] float32 (global), w [9][16][16] (LDS)
__device__ __forceinline__ float conv16_at(const float* in, int S, const float* w, int y, int x, int co) {
    float acc = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const f32x4* px = reinterpret_cast<const f32x4*>(in + (static_cast<int64_t>(y + ky) * S + x + kx) * LB_C);
            const float* wt = w + (ky * 3 + kx) * LB_C * LB_C + co;
#pragma unroll
            for (int c4 = 0; c4 < LB_C / 4; ++c4) {
                const f32x4 v = px[c4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = fmaf(v[q], wt[(4 * c4 + q) * LB_C], acc);
            }
        }
    return acc;
}

// t + sum_c g[c] w[c]: g 16 float32 (global), w 16 of LDS
__device__ __forceinline__ float dot16(const float* g, const float* w, float t) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
#pragma unroll
    for (int c4 = 0; c4 < LB_C / 4; ++c4) {
        const f32x4 v = g4[c4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t = fmaf(v[q], w[4 * c4 + q], t);
    }
    return t;
}

// avg-pool 4/2 forward, without its 1/16: the sum of relu6(pre) over the window at (2 y, 2 x) of channel c; pre [C][C][16]
__device__ __forceinline__ float pool_relu6_sum(const float* pre, int C, int y, int x, int c) {
    float t = 0.f;
    for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) t += relu6f(pre[((2 * y + ky) * C + 2 * x + kx) * LB_C + c]);
    return t;
}

// avg-pool 4/2 adjoint, without its 1/16 and without the ReLU6 mask: the sum of the pooled gradient g [So][So][16] over the windows that
// cover conv position (Y, X) (none at the last row / column of an odd conv side: 0)
__device__ __forceinline__ float pool_cover_sum(const float* g, int So, int Y, int X, int c) {
    int ylo, yhi, xlo, xhi;
    pool_span(Y, So, &ylo, &yhi);
    pool_span(X, So, &xlo, &xhi);
    float t = 0.f;
    for (int y = ylo; y <= yhi; ++y)
        for (int x = xlo; x <= xhi; ++x) t += g[(y * So + x) * LB_C + c];
    return t;
}

// conv3x3 VALID adjoint towards the input, one input element: sum_{ky, kx} dot16(dconv[Y - ky, X - kx], w[k][ci]); dconv [Co][Co][16]
// (global), w [9][16][16] (LDS)
__device__ __forceinline__ float conv16_adjoint_at(const float* dconv, int Co, const float* w, int Y, int X, int ci) {
    float t = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int y = Y - ky;
        if (y < 0 || y >= Co) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int x = X - kx;
            if (x < 0 || x >= Co) continue;
            t = dot16(dconv + (y * Co + x) * LB_C, w + ((ky * 3 + kx) * LB_C + ci) * LB_C, t);
        }
    }
    return t;
}

// the legacy bilinear tables of stage 9's skip, S7 -> S9 (rn_lastblock_resize_tables)
struct LbResize {
    const int32_t* lo;
    const int32_t* hi;
    const float* lerp;
};

// stage 9's skip: the resize of x7 [S7][S7][16] at output element (y, x) of channel c
__device__ __forceinline__ float skip_resize_at(const float* x7, int S7, const LbResize& r, int y, int x, int c) {
    const int ylo = r.lo[y], yhi = r.hi[y], xlo = r.lo[x], xhi = r.hi[x];
    const float yl = r.lerp[y], xl = r.lerp[x];
    const float tl = x7[(ylo * S7 + xlo) * LB_C + c], tr = x7[(ylo * S7 + xhi) * LB_C + c];
    const float bl = x7[(yhi * S7 + xlo) * LB_C + c], br = x7[(yhi * S7 + xhi) * LB_C + c];
    const float top = tl + (tr - tl) * xl, bot = bl + (br - bl) * xl;
    return top + (bot - top) * yl;
}

// ... and its transpose at input element (Y, X): the gradient g [S9][S9][16] of the resize's output, gathered with the weights
// (1-yl)(1-xl), (1-yl) xl, yl (1-xl), yl xl of the outputs that read (Y, X)
__device__ __forceinline__ float skip_resize_adjoint_at(const float* g, int S9, const LbResize& r, int Y, int X, int c) {
    float t = 0.f;
    for (int y = 0; y < S9; ++y) {
        const float yl = r.lerp[y];
        const float wy = (r.lo[y] == Y ? 1.f - yl : 0.f) + (r.hi[y] == Y ? yl : 0.f);
        if (wy == 0.f) continue;
        float rx = 0.f;
        for (int x = 0; x < S9; ++x) {
            const float xl = r.lerp[x];
            const float wx = (r.lo[x] == X ? 1.f - xl : 0.f) + (r.hi[x] == X ? xl : 0.f);
            if (wx != 0.f) rx = fmaf(wx, g[(y * S9 + x) * LB_C + c], rx);
        }
        t = fmaf(wy, rx, t);
    }
    return t;
}

// One dense layer's x @ W by a workgroup of NT threads: thread (j = tid % 64, group tid / 64) sums its group's share of k, the NT / 64
// shares are added in group order.  Valid for tid < nout (0 elsewhere); contains one barrier, the caller puts one behind its epilogue
// before red[] is used again.  xin [nin] (LDS or global), W [nin][nout] (global)
template <int NT>
__device__ __forceinline__ float dense_splitk(const float* xin, const float* W, int nin, int nout, float* red, int tid) {
    constexpr int NG = NT / LB_HMAX;
    const int j = tid % LB_HMAX, gi = tid / LB_HMAX;
    const int per = (nin + NG - 1) / NG;
    float v = 0.f;
    if (j < nout)
        for (int k = gi * per; k < min(nin, (gi + 1) * per); ++k) v = fmaf(xin[k], W[k * nout + j], v);
    red[tid] = v;
    __syncthreads();
    float t = 0.f;
    if (tid < nout)
        for (int g = 0; g < NG; ++g) t += red[g * LB_HMAX + tid];
    return t;
}

// MatMul's adjoint towards its input, element k: sum_j W[k][j] gz[j]
__device__ __forceinline__ float dense_adjoint_at(const float* W, int nout, const float* gz, int k) {
    float v = 0.f;
    for (int j = 0; j < nout; ++j) v = fmaf(W[k * nout + j], gz[j], v);
    return v;
}

}  // namespace rnk
