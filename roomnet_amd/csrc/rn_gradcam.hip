// Grad-CAM class-evidence maps (rn_grad_cam_*): the adjoint of the network's last conv block and dense head.
//
// Score S = z[c], z = the last dense layer's x @ W + b BEFORE its ReLU6 (reference network.py:237).  Layer A = s6.bn (the
// 128-channel conv_block, network.py:231) or s7.bn (the first step of the last block, :232).  G = dS/dA with TensorFlow's
// gradient rules (Relu6Grad passes where 0 < x < 6, AvgPool VALID spreads g / k^2 over each window, the inference BN
// multiplies by inv = gamma / sqrt(var + eps), Add sends g to both inputs, the legacy ResizeBilinear takes its transpose,
// MatMul the transposed kernel); alpha[c] = mean over (y, x) of G[y, x, c]; cam = max(0, sum_c alpha[c] A[.., c]).
//
// Three launches behind the handle's own forward pass (which left s6.bn and s7.bn in HBM):
//   gc_tail_kernel    one workgroup per image: recomputes stages 8, 9 (with the skip resize from s7.bn) and the head in fp32
//                     from the stored s7.bn, runs the adjoint back from S to g7 = dS/ds7.bn (conv 8 path + residual path)
//                     and, for layer s7.bn, reduces alpha and writes the map.  Intermediates live in a per-image fp32
//                     workspace (s7.bn is 296 KB of fp32 at 600 x 600: no LDS image).
//   gc_stage7_kernel  layer s6.bn: recomputes conv 7's pre-activation from s6.bn on the matrix cores (16-bit handles:
//                     v_mfma_f32_16x16x32 on the stored 16-bit s6.bn against W7 split into two 16-bit parts, fp32
//                     accumulation; float32 handles:
//                     v_mfma_f32_16x16x4_f32), applies the ReLU6 mask to the pool adjoint of g7 and reduces it per output
//                     channel: Gamma[co] = sum_p dS/dconv7[p, co] (partial sums per wave, no atomics: same bits every call).
//   gc_map6_kernel    alpha6[c] = 1/(H6 W6) sum_co (sum_{ky,kx} W7[ky, kx, c, co]) Gamma[co] -- conv 7 is VALID, every tap maps
//                     the whole output grid one-to-one into its input, so the 46 x 46 x 128 gradient field never exists --
//                     then one pass over s6.bn for the map.
// The per-element float32 steps gc_tail_kernel is built from (pool sums, conv adjoint gather, skip resize and its transpose, the head's
// dot products) are in rn_lastblock.h, shared with the trainers; gc_stage7_kernel's fixed 2 x 2 gather is its own form on purpose.
#include "rn_internal.h"
#include "rn_lastblock.h"
#include "rn_stage.h"

#include <type_traits>

#include <algorithm>
#include <vector>

using namespace rnk;

namespace {

constexpr int GC_NT = 512;           // threads of the tail-adjoint workgroup
constexpr int GC_R7 = 4;             // conv-7 rows per wave of gc_stage7_kernel
constexpr int GC_G7ROWS = 10;        // pooled rows of g7 one stage-7 workgroup (16 conv rows) reaches

struct GcTailArgs {
    const void* x7;                  // s7.bn [N, S7, S7, 16] in the handle's storage type
    int S7, C8, S8, C9, S9;
    const float* w8;                 // HWIO [3][3][16][16]
    const float* w9;
    const float* bn8;                // [mean | inv | beta] x 16
    const float* bn9;
    const float* bn9b;               // the residual step's second BN
    LbResize rs;                     // legacy bilinear tables S7 -> S9
    int n_dense;
    int nin[RN_MAX_DENSE], nout[RN_MAX_DENSE];
    const float* dw[RN_MAX_DENSE];
    const float* db[RN_MAX_DENSE];
    const float* dinv[RN_MAX_DENSE];
    const float* dshift[RN_MAX_DENSE];
    const int32_t* cls;              // class per image (null: the forward's argmax, `ids`)
    const int64_t* ids;
    int nc;
    float* ws;                       // per-image workspace
    int64_t ws_img, off_c8, off_s8, off_c9, off_fl, off_g7, off_x7;
    float* cam;                      // layer s7.bn: [N, S7, S7] (null otherwise)
    float* alpha;                    // layer s7.bn: [N, 16] or null
};

template <int DT>
__device__ __forceinline__ float ld_act(const void* p, int64_t i) {
    if constexpr (DT == RN_DTYPE_F32)
        return static_cast<const float*>(p)[i];
    else
        return from16<DT>(static_cast<const unsigned short*>(p)[i]);
}

template <int DT>
__global__ __launch_bounds__(GC_NT) void gc_tail_kernel(const GcTailArgs a) {
    __shared__ float w8[9 * LB_C * LB_C];
    __shared__ float w9[9 * LB_C * LB_C];
    __shared__ float tab[9 * LB_C];                       // bn8 | bn9 | bn9b, each [mean | inv | beta]
    __shared__ float hx[RN_MAX_DENSE][LB_HMAX];           // input of dense layer d (d >= 1)
    __shared__ float hmm[RN_MAX_DENSE][LB_HMAX];          // pre-activation of dense layer d
    __shared__ float hg[2][LB_HMAX];
    __shared__ float red[GC_NT];
    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const int S7 = a.S7, C8 = a.C8, S8 = a.S8, C9 = a.C9, S9 = a.S9;
    float* wsi = a.ws + img * a.ws_img;
    float* c8 = wsi + a.off_c8;
    float* s8 = wsi + a.off_s8;
    float* c9 = wsi + a.off_c9;
    float* fl = wsi + a.off_fl;
    float* g7 = wsi + a.off_g7;
    float* x7 = wsi + a.off_x7;                           // s7.bn of this image in fp32
    const int64_t x7b = static_cast<int64_t>(img) * S7 * S7 * LB_C;
    for (int i = tid; i < S7 * S7 * LB_C; i += GC_NT) x7[i] = ld_act<DT>(a.x7, x7b + i);
    for (int i = tid; i < 9 * LB_C * LB_C; i += GC_NT) {
        w8[i] = a.w8[i];
        w9[i] = a.w9[i];
    }
    if (tid < 3 * LB_C) {
        tab[tid] = a.bn8[tid];
        tab[48 + tid] = a.bn9[tid];
        tab[96 + tid] = a.bn9b[tid];
    }
    __syncthreads();
    // ---- forward recompute in fp32 from the stored s7.bn
    for (int i = tid; i < C8 * C8 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4;
        c8[i] = conv16_at(x7, S7, w8, p / C8, p % C8, co);
    }
    __syncthreads();
    for (int i = tid; i < S8 * S8 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4, y = p / S8, x = p % S8;
        const float t = pool_relu6_sum(c8, C8, y, x, co);
        s8[i] = (t * (1.0f / 16.0f) - tab[co]) * tab[16 + co] + tab[32 + co];
    }
    __syncthreads();
    for (int i = tid; i < C9 * C9 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4;
        c9[i] = conv16_at(s8, S8, w9, p / C9, p % C9, co);
    }
    __syncthreads();
    for (int i = tid; i < S9 * S9 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4, y = p / S9, x = p % S9;
        const float t = pool_relu6_sum(c9, C9, y, x, co);
        const float b = (t * (1.0f / 16.0f) - tab[48 + co]) * tab[64 + co] + tab[80 + co];
        fl[i] = ((b + skip_resize_at(x7, S7, a.rs, y, x, co)) - tab[96 + co]) * tab[112 + co] + tab[128 + co];
    }
    __syncthreads();
    // ---- dense head forward: each layer's dot products split over GC_NT / 64 groups of k, summed in a fixed order
    for (int d = 0; d < a.n_dense; ++d) {
        const int nout = a.nout[d];
        float t = dense_splitk<GC_NT>(d == 0 ? fl : hx[d], a.dw[d], a.nin[d], nout, red, tid);
        if (tid < nout) {
            if (a.db[d]) t += a.db[d][tid];
            hmm[d][tid] = t;
            if (d + 1 < a.n_dense) {
                float r = relu6f(t);
                if (a.dinv[d]) r = r * a.dinv[d][tid] + a.dshift[d][tid];
                hx[d + 1][tid] = r;
            }
        }
        __syncthreads();
    }
    // ---- adjoint of the head: dS/dz = one-hot at the class, MatMul -> transposed kernel, BN -> inv, ReLU6 -> mask
    int cls = a.cls ? a.cls[img] : static_cast<int>(a.ids[img]);
    cls = min(max(cls, 0), a.nc - 1);
    if (tid < LB_HMAX) hg[(a.n_dense - 1) & 1][tid] = tid == cls ? 1.f : 0.f;
    __syncthreads();
    for (int d = a.n_dense - 1; d >= 0; --d) {
        const int nin = a.nin[d], nout = a.nout[d];
        const float* gz = hg[d & 1];
        for (int k = tid; k < nin; k += GC_NT) {
            float v = dense_adjoint_at(a.dw[d], nout, gz, k);
            if (d == 0) {
                fl[k] = v;                                // dS/dflat (the flat input is no longer needed)
            } else {
                if (a.dinv[d - 1]) v *= a.dinv[d - 1][k];
                hg[(d - 1) & 1][k] = relu6_passes(hmm[d - 1][k]) ? v : 0.f;
            }
        }
        __syncthreads();
    }
    // ---- stage 9: second BN, the residual Add (fl keeps dS/d(add)), first BN, pool, ReLU6 mask; in place over c9
    for (int i = tid; i < S9 * S9 * LB_C; i += GC_NT) fl[i] *= tab[112 + (i & 15)];
    __syncthreads();
    for (int i = tid; i < C9 * C9 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4, Y = p / C9, X = p % C9;
        const float t = pool_cover_sum(fl, S9, Y, X, co);
        c9[i] = relu6_passes(c9[i]) ? t * tab[64 + co] * (1.0f / 16.0f) : 0.f;
    }
    __syncthreads();
    // ---- conv 9 adjoint -> dS/ds8.bn, times stage 8's inv (dS/d pool8), in place over s8
    for (int i = tid; i < S8 * S8 * LB_C; i += GC_NT) {
        const int ci = i & 15, p = i >> 4, Y = p / S8, X = p % S8;
        s8[i] = conv16_adjoint_at(c9, C9, w9, Y, X, ci) * tab[16 + ci];
    }
    __syncthreads();
    for (int i = tid; i < C8 * C8 * LB_C; i += GC_NT) {
        const int co = i & 15, p = i >> 4, Y = p / C8, X = p % C8;
        const float t = pool_cover_sum(s8, S8, Y, X, co);
        c8[i] = relu6_passes(c8[i]) ? t * (1.0f / 16.0f) : 0.f;
    }
    __syncthreads();
    // ---- g7 = conv 8 adjoint + transpose of the skip resize
    for (int i = tid; i < S7 * S7 * LB_C; i += GC_NT) {
        const int ci = i & 15, p = i >> 4, Y = p / S7, X = p % S7;
        g7[i] = conv16_adjoint_at(c8, C8, w8, Y, X, ci) + skip_resize_adjoint_at(fl, S9, a.rs, Y, X, ci);
    }
    if (!a.cam) return;
    __syncthreads();
    // ---- layer s7.bn: alpha = spatial mean of g7, map = relu(sum_c alpha[c] s7.bn[.., c])
    {
        const int c = tid & 15, part = tid >> 4;
        float t = 0.f;
        for (int p = part; p < S7 * S7; p += GC_NT / 16) t += g7[p * LB_C + c];
        red[tid] = t;
    }
    __syncthreads();
    if (tid < LB_C) {
        float t = 0.f;
        for (int part = 0; part < GC_NT / 16; ++part) t += red[part * 16 + tid];
        t /= static_cast<float>(S7 * S7);
        hg[0][tid] = t;
        if (a.alpha) a.alpha[img * LB_C + tid] = t;
    }
    __syncthreads();
    for (int p = tid; p < S7 * S7; p += GC_NT) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < LB_C; ++c) t = fmaf(hg[0][c], x7[p * LB_C + c], t);
        a.cam[static_cast<int64_t>(img) * S7 * S7 + p] = fmaxf(t, 0.f);
    }
}

struct GcStage7Args {
    const void* x6;                  // s6.bn [N, S6, S6, 128]
    int S6, C7, S7;
    const i32x4* wfrag;              // 16-bit handles: [2][36 K-chunks][64 lanes] B fragments of W7: rounded, then the remainder
    const float* w7;                 // float32 handles: HWIO [3][3][128][16]
    const float* ws;
    int64_t ws_img, off_g7;
    float* part;                     // [N][npart][16]
    int npart;
};

// One workgroup = 4 waves x GC_R7 conv-7 rows of one image; a wave walks its rows in 16-pixel tiles x all 16 couts.
// MFMA operands: A = pixels (lane & 15) x K, B = K x couts (lane & 15); C/D: pixel 4 (lane >> 4) + j, cout lane & 15.
template <int DT>
__global__ __launch_bounds__(256) void gc_stage7_kernel(const GcStage7Args a) {
    extern __shared__ __attribute__((aligned(16))) float wl[];        // float32 handles: W7 [9 * 128][16]; 16-bit: the remainder fragments
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.y;
    const int i16 = lane & 15, kg = lane >> 4, co = lane & 15;
    const int S6 = a.S6, C7 = a.C7, S7 = a.S7;
    const float* g7 = a.ws + img * a.ws_img + a.off_g7;
    [[maybe_unused]] i32x4 wreg[36];
    if constexpr (DT == RN_DTYPE_F32) {
        for (int i = tid; i < 9 * LB_CIN7 * LB_C; i += 256) wl[i] = a.w7[i];
        __syncthreads();
    } else {
#pragma unroll
        for (int c = 0; c < 36; ++c) wreg[c] = a.wfrag[c * 64 + lane];
        for (int i = tid; i < 36 * 64; i += 256) reinterpret_cast<i32x4*>(wl)[i] = a.wfrag[36 * 64 + i];
        __syncthreads();
    }
    // the pooled rows of g7 this workgroup's conv rows reach (<= GC_G7ROWS), in LDS behind the weights: the pool adjoint's gathers
    // as global loads inside the epilogue serialised behind each other (0.37 ms for batch 256 at 224)
    float* g7l = wl + (DT == RN_DTYPE_F32 ? 9 * LB_CIN7 * LB_C : 36 * 64 * 4);
    const int wy0 = blockIdx.x * 4 * GC_R7;
    int glo, ghi, dummy;
    pool_span(wy0, S7, &glo, &dummy);
    pool_span(min(C7, wy0 + 4 * GC_R7) - 1, S7, &dummy, &ghi);
    for (int i = tid; i < (ghi - glo + 1) * S7 * LB_C; i += 256) g7l[i] = g7[glo * S7 * LB_C + i];
    __syncthreads();
    // Each input row is loaded once per tile and feeds the (up to) three conv rows of the wave it reaches: GC_R7 conv rows cost
    // GC_R7 + 2 operand rows instead of 3 GC_R7 (one load per (row, ky) read s6.bn nine times from the caches: 0.25 ms at batch 256)
    const int y0 = wy0 + wave * GC_R7;
    const int nrows = min(C7, y0 + GC_R7) - y0;
    float gsum = 0.f;
    for (int x0 = 0; nrows > 0 && x0 < C7; x0 += 16) {
        const int X = min(x0 + i16, C7 - 1);
        f32x4 acc[GC_R7];
#pragma unroll
        for (int r = 0; r < GC_R7; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rr = 0; rr < GC_R7 + 2; ++rr) {
            if (rr > nrows + 1) break;                    // input row y0 + rr <= the last conv row + 2 <= S6 - 1
            const int64_t rowb = (static_cast<int64_t>(img) * S6 + y0 + rr) * S6;
            if constexpr (DT == RN_DTYPE_F32) {
                const float* x6 = static_cast<const float*>(a.x6);
                for (int kx = 0; kx < 3; ++kx) {
                    const float* px = x6 + (rowb + X + kx) * LB_CIN7 + 4 * kg;
#pragma unroll 2
                    for (int c16 = 0; c16 < LB_CIN7 / 16; ++c16) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(px + c16 * 16);
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky) {
                            const int yi = rr - ky;
                            if (yi < 0 || yi >= GC_R7) continue;
                            const float* wt = wl + (ky * 3 + kx) * LB_CIN7 * LB_C + (4 * kg + c16 * 16) * LB_C + co;
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[yi] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[q], wt[q * LB_C], acc[yi], 0, 0, 0);
                        }
                    }
                }
            } else {
                const unsigned short* x6 = static_cast<const unsigned short*>(a.x6);
                i32x4 av[12];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb)
                        av[kx * 4 + cb] = *reinterpret_cast<const i32x4*>(x6 + (rowb + X + kx) * LB_CIN7 + cb * 32 + 8 * kg);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int yi = rr - ky;
                    if (yi < 0 || yi >= GC_R7) continue;
                    const i32x4* wlo = reinterpret_cast<const i32x4*>(wl) + ky * 12 * 64 + lane;
#pragma unroll
                    for (int q = 0; q < 12; ++q) {
                        acc[yi] = mfma16<DT>(av[q], wreg[ky * 12 + q], acc[yi]);
                        acc[yi] = mfma16<DT>(av[q], wlo[q * 64], acc[yi]);
                    }
                }
            }
        }
#pragma unroll
        for (int yi = 0; yi < GC_R7; ++yi) {
            if (yi >= nrows) break;
            int ylo, yhi;
            pool_span(y0 + yi, S7, &ylo, &yhi);
            ylo -= glo;
            yhi -= glo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // (a conv row / column is covered by one or two pooled ones: a fixed 2 x 2 gather, the absent terms zero.  At an
                //  odd conv side VALID pooling covers the last row / column by none (lo > hi): no gradient reaches it, and nothing
                //  is read -- its pooled index lies past the rows this workgroup staged)
                const int Xp = min(x0 + 4 * kg + j, C7 - 1);
                int xlo, xhi;
                pool_span(Xp, S7, &xlo, &xhi);
                const bool cov = ylo <= yhi && xlo <= xhi;
                const float* r0 = g7l + ylo * S7 * LB_C + co;
                const float* r1 = g7l + yhi * S7 * LB_C + co;
                const float t00 = cov ? r0[xlo * LB_C] : 0.f, t01 = cov && xhi > xlo ? r0[xhi * LB_C] : 0.f;
                const float t10 = cov && yhi > ylo ? r1[xlo * LB_C] : 0.f, t11 = cov && yhi > ylo && xhi > xlo ? r1[xhi * LB_C] : 0.f;
                const float t = (t00 + t01) + (t10 + t11);
                gsum += x0 + 4 * kg + j < C7 && relu6_passes(acc[yi][j]) ? t : 0.f;
            }
        }
    }
    gsum += __shfl_xor(gsum, 16);
    gsum += __shfl_xor(gsum, 32);
    if (lane < 16) a.part[(static_cast<int64_t>(img) * a.npart + blockIdx.x * 4 + wave) * LB_C + lane] = gsum;
}

struct GcMap6Args {
    const void* x6;
    int S6;
    const float* part;
    int npart;
    const float* w7sum;              // [128][16]: sum over the 9 taps of W7
    const float* inv7;               // [16]
    float* cam;                      // [N, S6, S6]
    float* alpha;                    // [N, 128] or null
    int pix_per_block;
};

template <int DT>
__global__ __launch_bounds__(256) void gc_map6_kernel(const GcMap6Args a) {
    __shared__ float gam[LB_C];
    __shared__ __attribute__((aligned(16))) float al[LB_CIN7];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int S6 = a.S6;
    if (tid < LB_C) {
        const float* p = a.part + static_cast<int64_t>(img) * a.npart * LB_C + tid;
        float t = 0.f;
        for (int k = 0; k < a.npart; ++k) t += p[k * LB_C];
        gam[tid] = t * (a.inv7[tid] * (1.0f / 16.0f));       // dS/d pool7 = inv7 g7; the pool adjoint's 1/16
    }
    __syncthreads();
    if (tid < LB_CIN7) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < LB_C; ++c) t = fmaf(a.w7sum[tid * LB_C + c], gam[c], t);
        t /= static_cast<float>(S6 * S6);
        al[tid] = t;
        if (a.alpha && blockIdx.x == 0) a.alpha[img * LB_CIN7 + tid] = t;
    }
    __syncthreads();
    // 16 lanes per pixel, 8 channels per lane
    const int sub = tid & 15, slot = tid >> 4;
    const int p0 = blockIdx.x * a.pix_per_block;
    const int p1 = min(S6 * S6, p0 + a.pix_per_block);
    f32x4 alo = *reinterpret_cast<const f32x4*>(al + 8 * sub), ahi = *reinterpret_cast<const f32x4*>(al + 8 * sub + 4);
    for (int pb = p0; pb < p1; pb += 16) {
        const int p = pb + slot;
        float t = 0.f;
        if (p < p1) {
            const int64_t off = (static_cast<int64_t>(img) * S6 * S6 + p) * LB_CIN7 + 8 * sub;
            float v[8];
            if constexpr (DT == RN_DTYPE_F32) {
                const f32x4 u0 = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.x6) + off);
                const f32x4 u1 = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.x6) + off + 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = u0[q];
                    v[4 + q] = u1[q];
                }
            } else {
                const uint4 u = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(a.x6) + off);
                const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[2 * q] = from16<DT>(static_cast<unsigned short>(w[q] & 0xffff));
                    v[2 * q + 1] = from16<DT>(static_cast<unsigned short>(w[q] >> 16));
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) t = fmaf(alo[q], v[q], t);
#pragma unroll
            for (int q = 0; q < 4; ++q) t = fmaf(ahi[q], v[4 + q], t);
        }
        t += __shfl_xor(t, 8);
        t += __shfl_xor(t, 4);
        t += __shfl_xor(t, 2);
        t += __shfl_xor(t, 1);
        if (sub == 0 && p < p1) a.cam[static_cast<int64_t>(img) * S6 * S6 + p] = fmaxf(t, 0.f);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// What rn_create keeps for the adjoint (rn_weights' pointers are only valid inside rn_create), and the device state the first
// grad-CAM call allocates.
struct GradCamState {
    bool supported = false;
    std::string why;
    int s6 = -1, s7 = -1, s8 = -1, s9 = -1;       // stage indices
    std::vector<float> blob;                       // host copy of everything the kernels read, uploaded once
    size_t o_w7 = 0, o_w7sum = 0, o_inv7 = 0, o_w8 = 0, o_w9 = 0, o_bn8 = 0, o_bn9 = 0, o_bn9b = 0, o_rlerp = 0;
    size_t o_dw[RN_MAX_DENSE] = {}, o_db[RN_MAX_DENSE] = {}, o_dinv[RN_MAX_DENSE] = {}, o_dshift[RN_MAX_DENSE] = {};
    bool has_b[RN_MAX_DENSE] = {}, has_bn[RN_MAX_DENSE] = {};
    rn_lastblock sd{};                             // the block's sides
    std::vector<int32_t> rtab;                     // rlo | rhi
    std::vector<unsigned short> wfrag;             // 16-bit handles: W7 as MFMA B fragments
    // device (first call)
    float* d_blob = nullptr;
    int32_t* d_rtab = nullptr;                     // rlo | rhi
    i32x4* d_wfrag = nullptr;
    float* d_ws = nullptr;
    float* d_part = nullptr;
    int32_t* d_cls = nullptr;                      // host entry points: the caller's classes
    float* d_cam = nullptr;                        // host entry points: staging of the map and alpha
    float* d_alpha = nullptr;
    int64_t ws_img = 0, off_c8 = 0, off_s8 = 0, off_c9 = 0, off_fl = 0, off_g7 = 0, off_x7 = 0;
    int npart = 0;
    bool ready = false;                            // every device buffer above exists
};

GradCamState* state(rn_handle* h) { return static_cast<GradCamState*>(h->gradcam); }

// calls f with the handle's storage type as a compile-time constant: one launch line per kernel template
template <typename F>
void by_dtype(int dtype, F&& f) {
    if (dtype == RN_DTYPE_F32)
        f(std::integral_constant<int, RN_DTYPE_F32>{});
    else if (dtype == RN_DTYPE_BF16)
        f(std::integral_constant<int, RN_DTYPE_BF16>{});
    else
        f(std::integral_constant<int, RN_DTYPE_F16>{});
}

int ensure_device(rn_handle* h, GradCamState* g) {
    if (g->ready) return RN_OK;
    const auto [S6, C7, S7, C8, S8, C9, S9] = g->sd;
    const size_t nb = static_cast<size_t>(h->max_batch);
    int rc;
    if ((rc = upload(h, g->blob.data(), g->blob.size(), &g->d_blob)) != RN_OK) return rc;
    if ((rc = upload(h, g->rtab.data(), g->rtab.size(), &g->d_rtab)) != RN_OK) return rc;
    if (!g->wfrag.empty()) {
        unsigned short* p = nullptr;
        if ((rc = upload(h, g->wfrag.data(), g->wfrag.size(), &p)) != RN_OK) return rc;
        g->d_wfrag = reinterpret_cast<i32x4*>(p);
    }
    // per-image workspace: c8 | s8 | c9 | flat | g7 | s7.bn in fp32, each a multiple of 16 floats
    g->off_c8 = 0;
    g->off_s8 = g->off_c8 + static_cast<int64_t>(C8) * C8 * LB_C;
    g->off_c9 = g->off_s8 + static_cast<int64_t>(S8) * S8 * LB_C;
    g->off_fl = g->off_c9 + static_cast<int64_t>(C9) * C9 * LB_C;
    g->off_g7 = g->off_fl + static_cast<int64_t>(S9) * S9 * LB_C;
    g->off_x7 = g->off_g7 + static_cast<int64_t>(S7) * S7 * LB_C;
    g->ws_img = g->off_x7 + static_cast<int64_t>(S7) * S7 * LB_C;
    void* p = nullptr;
    if ((rc = dev_alloc(h, nb * g->ws_img * 4, &p)) != RN_OK) return rc;
    g->d_ws = static_cast<float*>(p);
    const int nblk = (C7 + 4 * GC_R7 - 1) / (4 * GC_R7);
    g->npart = nblk * 4;
    if ((rc = dev_alloc(h, nb * g->npart * LB_C * 4, &p)) != RN_OK) return rc;
    g->d_part = static_cast<float*>(p);
    if ((rc = dev_alloc(h, nb * 4, &p)) != RN_OK) return rc;
    g->d_cls = static_cast<int32_t*>(p);
    const size_t cam_px = static_cast<size_t>(std::max(S6 * S6, S7 * S7));
    if ((rc = dev_alloc(h, nb * cam_px * 4, &p)) != RN_OK) return rc;
    g->d_cam = static_cast<float*>(p);
    if ((rc = dev_alloc(h, nb * LB_CIN7 * 4, &p)) != RN_OK) return rc;
    g->d_alpha = static_cast<float*>(p);
    g->ready = true;          // (last: after a failed allocation the next call starts over; what was allocated is freed by rn_destroy)
    return RN_OK;
}

}  // namespace

// The graphs whose last block and head the adjoint kernels walk (grad-CAM here, the fine-tuning trainer in rn_finetune.hip): null, or
// the reason a graph is refused.
const char* rn_tail_graph_reason(const rn_weights* w) {
    const int ns = w->n_stages;
    if (ns < 4 || w->n_dense < 1) return "the graph has no 128 -> 16 -> 16 -> 16 last block";
    const rn_conv_stage &st6 = w->stages[ns - 4], &st7 = w->stages[ns - 3], &st8 = w->stages[ns - 2], &st9 = w->stages[ns - 1];
    auto last_block = [](const rn_conv_stage& s) { return s.cout == LB_C && s.pool_k == 4 && s.pool_s == 2; };
    if (st6.cout != LB_CIN7 || st7.cin != LB_CIN7 || !last_block(st7) || !last_block(st8) || !last_block(st9) || st8.cin != LB_C ||
        st9.cin != LB_C || st7.skip_stage >= 0 || st8.skip_stage >= 0 || st9.skip_stage != ns - 3 || !st9.gamma2 || st6.skip_stage >= 0)
        return "the graph's last two blocks are not conv_block(128, pooling=False) + conv_block(16, 4, 2, depth 3)";
    for (int d = 0; d < w->n_dense; ++d)
        if (w->dense[d].nout > LB_HMAX || (d + 1 < w->n_dense && !w->dense[d].gamma) || (d + 1 == w->n_dense && w->dense[d].gamma))
            return "the dense head is not BN dense blocks followed by one plain dense layer";
    return nullptr;
}

int rn_gradcam_keep(rn_handle* h, const rn_weights* w) {
    auto* g = new GradCamState();
    h->gradcam = g;
    const int ns = w->n_stages;
    auto no = [&](const char* why) {
        g->why = why;
        return RN_OK;
    };
    if (const char* why = rn_tail_graph_reason(w)) return no(why);
    g->s6 = ns - 4;
    g->s7 = ns - 3;
    g->s8 = ns - 2;
    g->s9 = ns - 1;
    const rn_conv_stage &st7 = w->stages[g->s7], &st8 = w->stages[g->s8], &st9 = w->stages[g->s9];
    const float eps = w->bn_epsilon;
    std::vector<float>& b = g->blob;
    auto put = [&](const float* src, size_t cnt) {
        const size_t off = b.size();
        b.insert(b.end(), src, src + cnt);
        b.resize((b.size() + 3) & ~static_cast<size_t>(3));          // 16-byte alignment of every piece
        return off;
    };
    auto put_bn = [&](const float* gamma, const float* beta, const float* mean, const float* var) {
        std::vector<float> t(3 * LB_C);
        for (int c = 0; c < LB_C; ++c) {
            t[c] = mean[c];
            t[LB_C + c] = rn_bn_inv(var[c], gamma[c], eps);
            t[2 * LB_C + c] = beta[c];
        }
        return put(t.data(), t.size());
    };
    const size_t n7 = static_cast<size_t>(9) * LB_CIN7 * LB_C;
    g->o_w7 = put(st7.kernel, n7);
    {
        std::vector<float> ws(static_cast<size_t>(LB_CIN7) * LB_C, 0.f), inv(LB_C);
        for (int t = 0; t < 9; ++t)
            for (size_t i = 0; i < ws.size(); ++i) ws[i] += st7.kernel[t * ws.size() + i];
        g->o_w7sum = put(ws.data(), ws.size());
        for (int c = 0; c < LB_C; ++c) inv[c] = rn_bn_inv(st7.variance[c], st7.gamma[c], eps);
        g->o_inv7 = put(inv.data(), inv.size());
    }
    g->o_w8 = put(st8.kernel, 9 * LB_C * LB_C);
    g->o_w9 = put(st9.kernel, 9 * LB_C * LB_C);
    g->o_bn8 = put_bn(st8.gamma, st8.beta, st8.mean, st8.variance);
    g->o_bn9 = put_bn(st9.gamma, st9.beta, st9.mean, st9.variance);
    g->o_bn9b = put_bn(st9.gamma2, st9.beta2, st9.mean2, st9.variance2);
    // legacy bilinear tables S7 -> S9
    {
        if (rn_lastblock_sides(w, &g->sd) < ns) return no("im_side is too small for the graph");      // (build_plan reports it)
        std::vector<float> lerp;
        rn_lastblock_resize_tables(g->sd, g->rtab, lerp);
        g->o_rlerp = put(lerp.data(), lerp.size());
    }
    for (int d = 0; d < w->n_dense; ++d) {
        const rn_dense_layer& l = w->dense[d];
        g->o_dw[d] = put(l.kernel, static_cast<size_t>(l.nin) * l.nout);
        g->has_b[d] = l.bias != nullptr;
        if (l.bias) g->o_db[d] = put(l.bias, l.nout);
        g->has_bn[d] = l.gamma != nullptr;
        if (l.gamma) {
            std::vector<float> inv(l.nout), shift(l.nout);
            for (int j = 0; j < l.nout; ++j) {
                inv[j] = rn_bn_inv(l.variance[j], l.gamma[j], eps);
                shift[j] = rn_bn_shift(l.beta[j], l.mean[j], inv[j]);
            }
            g->o_dinv[d] = put(inv.data(), inv.size());
            g->o_dshift[d] = put(shift.data(), shift.size());
        }
    }
    if (h->dtype != RN_DTYPE_F32) {
        // B fragments of v_mfma_f32_16x16x32: chunk q = (tap, 32-channel block cb), lane l holds W7[tap][cb 32 + 8 (l >> 4) + j][l & 15].
        // Two sets: W7 rounded to the storage type, then the remainder w - hi rounded: the two products summed in fp32 are the fp32
        // convolution of the stored s6.bn to ~2^-16 of the weights, so the recomputed ReLU6 mask is that of the float32 weights
        // (one rounded set alone moved the map by 0.5 % of its maximum: pre-activations near 0 and 6 change side)
        g->wfrag.resize(static_cast<size_t>(2) * 36 * 64 * 8);
        for (int q = 0; q < 36; ++q) {
            const int tap = q / 4, cb = q % 4;
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int ci = cb * 32 + 8 * (l >> 4) + j, co = l & 15;
                    const float wv = st7.kernel[(static_cast<size_t>(tap) * LB_CIN7 + ci) * LB_C + co];
                    const unsigned short hi = rn_to16(wv, h->dtype);
                    g->wfrag[(static_cast<size_t>(q) * 64 + l) * 8 + j] = hi;
                    g->wfrag[(static_cast<size_t>(36 + q) * 64 + l) * 8 + j] = rn_to16(wv - rn_from16(hi, h->dtype), h->dtype);
                }
        }
    }
    g->supported = true;
    return RN_OK;
}

void rn_gradcam_release(rn_handle* h) {
    delete state(h);           // (its device buffers are in h->allocs)
    h->gradcam = nullptr;
}

// the layer nodes grad-CAM accepts: s6.bn and s7.bn of a supported graph (-1 each otherwise)
void rn_gradcam_layers(const rn_handle* h, int* node6, int* node7) {
    const GradCamState* g = static_cast<const GradCamState*>(h->gradcam);
    *node6 = *node7 = -1;
    if (!g || !g->supported) return;
    *node6 = h->stages[g->s6].node_bn;
    *node7 = h->stages[g->s7].node_bn;
}

const char* rn_gradcam_unsupported(const rn_handle* h) {
    const GradCamState* g = static_cast<const GradCamState*>(h->gradcam);
    if (!g) return "no grad-CAM plan";
    return g->supported ? nullptr : g->why.c_str();
}

// The adjoint behind a forward pass that left s6.bn and s7.bn in HBM.  d_cls: int32 classes on the device or null (argmax:
// d_ids).  Arguments are validated by the caller.
int rn_gradcam_launch(rn_handle* h, int n, const int32_t* d_cls, const int64_t* d_ids, bool layer6, float* d_cam, float* d_alpha) {
    GradCamState* g = state(h);
    int rc;
    if ((rc = ensure_device(h, g)) != RN_OK) return rc;
    const auto [S6, C7, S7, C8, S8, C9, S9] = g->sd;
    const NodeBuf& n6 = h->nodes[h->stages[g->s6].node_bn];
    const NodeBuf& n7 = h->nodes[h->stages[g->s7].node_bn];
    if (!n6.ptr || !n7.ptr || h->node_perm.count(h->stages[g->s6].node_bn) || h->node_perm.count(h->stages[g->s7].node_bn)) {
        rn_set_error("rn_grad_cam: s6.bn / s7.bn are not stored in the reference's layout on this handle");
        return RN_E_STATE;
    }
    const float* B = g->d_blob;
    GcTailArgs t{};
    t.x7 = n7.ptr;
    t.S7 = S7;
    t.C8 = C8;
    t.S8 = S8;
    t.C9 = C9;
    t.S9 = S9;
    t.w8 = B + g->o_w8;
    t.w9 = B + g->o_w9;
    t.bn8 = B + g->o_bn8;
    t.bn9 = B + g->o_bn9;
    t.bn9b = B + g->o_bn9b;
    t.rs = LbResize{g->d_rtab, g->d_rtab + S9, B + g->o_rlerp};
    t.n_dense = static_cast<int>(h->dense.size());
    for (int d = 0; d < t.n_dense; ++d) {
        t.nin[d] = h->dense[d].nin;
        t.nout[d] = h->dense[d].nout;
        t.dw[d] = B + g->o_dw[d];
        t.db[d] = g->has_b[d] ? B + g->o_db[d] : nullptr;
        t.dinv[d] = g->has_bn[d] ? B + g->o_dinv[d] : nullptr;
        t.dshift[d] = g->has_bn[d] ? B + g->o_dshift[d] : nullptr;
    }
    t.cls = d_cls;
    t.ids = d_ids;
    t.nc = h->num_classes;
    t.ws = g->d_ws;
    t.ws_img = g->ws_img;
    t.off_c8 = g->off_c8;
    t.off_s8 = g->off_s8;
    t.off_c9 = g->off_c9;
    t.off_fl = g->off_fl;
    t.off_g7 = g->off_g7;
    t.off_x7 = g->off_x7;
    t.cam = layer6 ? nullptr : d_cam;
    t.alpha = layer6 ? nullptr : d_alpha;
    by_dtype(h->dtype, [&](auto dt) { hipLaunchKernelGGL(gc_tail_kernel<decltype(dt)::value>, dim3(n), dim3(GC_NT), 0, h->stream, t); });
    RN_CHECK_LAUNCH();
    if (!layer6) return RN_OK;
    GcStage7Args s{};
    s.x6 = n6.ptr;
    s.S6 = S6;
    s.C7 = C7;
    s.S7 = S7;
    s.wfrag = g->d_wfrag;
    s.w7 = B + g->o_w7;
    s.ws = g->d_ws;
    s.ws_img = g->ws_img;
    s.off_g7 = g->off_g7;
    s.part = g->d_part;
    s.npart = g->npart;
    const dim3 grid7(g->npart / 4, n);
    const size_t g7_lds = static_cast<size_t>(GC_G7ROWS) * S7 * LB_C * 4;
    const size_t w7_lds = h->dtype == RN_DTYPE_F32 ? 9 * LB_CIN7 * LB_C * 4 : 36 * 64 * 16;
    by_dtype(h->dtype, [&](auto dt) { hipLaunchKernelGGL(gc_stage7_kernel<decltype(dt)::value>, grid7, dim3(256), w7_lds + g7_lds, h->stream, s); });
    RN_CHECK_LAUNCH();
    GcMap6Args m{};
    m.x6 = n6.ptr;
    m.S6 = S6;
    m.part = g->d_part;
    m.npart = g->npart;
    m.w7sum = B + g->o_w7sum;
    m.inv7 = B + g->o_inv7;
    m.cam = d_cam;
    m.alpha = d_alpha;
    m.pix_per_block = 128;
    const dim3 grid6((S6 * S6 + m.pix_per_block - 1) / m.pix_per_block, n);
    by_dtype(h->dtype, [&](auto dt) { hipLaunchKernelGGL(gc_map6_kernel<decltype(dt)::value>, grid6, dim3(256), 0, h->stream, m); });
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// device staging of the host entry points (allocated by the first call, sized for max_batch)
int rn_gradcam_staging(rn_handle* h, int32_t** d_cls, float** d_cam, float** d_alpha) {
    GradCamState* g = state(h);
    int rc;
    if ((rc = ensure_device(h, g)) != RN_OK) return rc;
    *d_cls = g->d_cls;
    *d_cam = g->d_cam;
    *d_alpha = g->d_alpha;
    return RN_OK;
}
