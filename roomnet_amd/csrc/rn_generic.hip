// The generic family of the fused 16-bit path: stage 0 as a launch of its own and one MFMA kernel for every other stage shape.
// A stage is   conv3x3 VALID s1 (no bias) -> ReLU6 -> [avg-pool k x k / s] -> BN
//              -> [ + legacy-bilinear(skip) -> BN ]          (reference network.py:172-208)
// Activations live in HBM as NHWC 16-bit tensors; a stage reads its input once and
// writes its post-BN output once (the stage-boundary traffic model of SURVEY.md 8d).
// Accumulation, ReLU6, pooling, BN and the residual are float32 in registers.
//
// Kernel structure (stages 1..N, `stage_mfma_kernel`):
//   * a workgroup owns one image, one band of output rows and one block of columns and
//     walks down its band one conv row per iteration ("row streaming"): the last
//     3 input rows live in an LDS ring, the next row is prefetched into registers while
//     the current one is computed -- every input row is fetched once per band.
//   * implicit GEMM on the matrix cores, D[cout][pixel] = W^T[cout][k] * im2col[k][pixel]
//     with v_mfma_f32_32x32x16_{bf16,f16}: a wave owns a tile of 32 consecutive conv
//     columns; the B operand (8 consecutive channels of one tap of one pixel = 16 B) is a
//     single ds_read_b128 from the NHWC ring, made bank-conflict free by XOR-swizzling the
//     16-byte channel chunk inside each pixel; the A operand (weights) is pre-packed on
//     the host in fragment order and read from LDS with lane-linear ds_read_b128.
//   * the accumulator layout puts the pixel on the lane and the channel in the
//     register, so ReLU6 is per register, the horizontal pool sum is two DPP wave shifts
//     per register, the vertical pool sum is a register ring across iterations, BN is
//     an fma, and the pooled tile never touches LDS or HBM before its final store.
//   * neighbouring pixel tiles overlap by k-1 columns so that no cross-wave exchange is
//     needed for the horizontal pool.
// Stage 0 (3 input channels, K = 27) runs on the matrix cores too (`stage0_kernel` below): its operand is the
// uint8 pixel value, the uint8 -> [-1,1] pre-processing of network.py:129 is folded into its weights.
#include "rn_fused.h"

using namespace rnk;

namespace {

// ------------------------------------------------------------------------------ stage 0
// uint8 BGR [N,S,S,3] -> table -> conv3x3 (3 -> 8) -> ReLU6 -> avg-pool 3x3/1 -> BN -> 16-bit NHWC.
//
// Row streaming on the matrix cores with the im2col built entirely in registers:
//   * K is laid out as (ky, kx in 0..3, c in 0..3) = 48 (kx = 3 and c = 3 are zero weights), i.e.
//     ONE 16-deep MFMA K-chunk per input row ky.  For v_mfma_f32_32x32x16 the B operand of lane
//     (r, h) is then: h = 0: pixels r and r+1 (4 x 16-bit each), h = 1: pixel r+2 and zeros.
//   * lane (r, h) loads ITS pixel x0 + r + 2h (3 bytes) and packs the byte values as fp16 numbers
//     (R,G | B,0) -- exact; the pre-processing table of network.py:129 is folded into the weights
//     (s0_pixel_halves, rn_stage.h); the lower half-wave gets pixel r+1 from its neighbour lane
//     with a DPP shift.  The fragments of the last 3 input rows stay in 12 VGPRs.
//   * D[cout][pixel]: rows 0..7 hold the hi halves of the folded weights, rows 8..15 the lo halves,
//     so a lane owns 4 channels of one conv pixel in 4 + 4 accumulator registers: add, ReLU6,
//     3-wide horizontal sum by DPP, 3-row vertical sum in a register ring, one fma for BN, one
//     8-byte store.  No LDS traffic.
// A wave owns 32 conv columns (29 output columns, tiles overlap by 3) and walks down a band of
// rows; a workgroup is up to 8 such waves side by side.
// The MFMA inputs of this stage are ALWAYS fp16, whatever the storage type of the activations:
// fp16 holds the 256 input levels exactly and the weights as hi + lo pairs, so the stage computes
// the fp32 convolution of the exact input (bf16's 8-bit significand cannot represent the levels).
constexpr int S0_AHEAD = 8;         // input rows prefetched (one dword per lane and row in registers)

template <int DT>
__global__ __launch_bounds__(512) void stage0_kernel(const Stage0Args a) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int cb = blockIdx.x % a.n_colblocks;
    const int band = blockIdx.x / a.n_colblocks;
    const int n = blockIdx.y;

    const int yo0 = band * a.rows_per_band;
    const int yo1 = min(a.So, yo0 + a.rows_per_band);
    const int nconv = (yo1 - yo0) + 2;                 // conv rows of the band (pool 3, stride 1)
    const int nin = nconv + 2;                         // input rows
    const int xt0 = (cb * a.npt + wave) * S0_TSTRIDE;  // first conv / input column of this wave's tile
    const int px = min(xt0 + r + 2 * hh, a.S - 1);     // this lane's input column (clamped at the edge)
    // One (unaligned) dword load per lane and row covers the pixel's 3 bytes -- three byte loads cost the
    // address coalescer three passes per row.  The last column reads one byte early and shifts, so no lane
    // ever touches the byte behind the caller's buffer.
    const int sh0 = px == a.S - 1 ? 8 : 0;
    const uint8_t* src = a.bgr + (static_cast<int64_t>(n) * a.S * a.S + static_cast<int64_t>(yo0) * a.S + px) * 3 - (sh0 >> 3);
    const int row_bytes = a.S * 3;

    i32x4 wreg[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) wreg[ky] = a.wfrag[ky * 64 + lane];
    const f32x4 scale = *reinterpret_cast<const f32x4*>(a.ptab + 4 * hh);
    const f32x4 shift = *reinterpret_cast<const f32x4*>(a.ptab + 8 + 4 * hh);
    const int xo = xt0 + r;
    const bool lane_out = r < S0_TSTRIDE && xo < a.So && (xo - cb * a.npt * S0_TSTRIDE) < a.npt * S0_TSTRIDE;
    unsigned short* out_lane = a.out + (static_cast<int64_t>(n) * a.So * a.So + xo) * S0_CO + 4 * hh;
    const unsigned nb_mask = hh ? 0u : 0xffffffffu;    // the upper half-wave's second pixel slot is zero

    // prefetch queue of raw bytes
    unsigned pw[S0_AHEAD];
    auto load_px = [&](int j) -> unsigned {
        unsigned w;
        __builtin_memcpy(&w, src + static_cast<int64_t>(min(j, nin - 1)) * row_bytes, 4);   // unaligned dword
        return w;
    };
#pragma unroll
    for (int i = 0; i < S0_AHEAD; ++i) pw[i] = load_px(i);

    i32x4 bfr[3];                                      // B fragments of the 3 live input rows
    float h1[4], h2[4];                                // horizontal sums of the two previous conv rows
#pragma unroll
    for (int j = 0; j < 4; ++j) h1[j] = h2[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) bfr[i] = i32x4{0, 0, 0, 0};

    // consume the oldest prefetched row into a B fragment, refill the queue slot
    auto next_frag = [&](int jrow) -> i32x4 {
        const unsigned w = pw[0] >> sh0;                       // bytes: B, G, R
        int d0, d1;
        s0_pixel_halves(w, d0, d1);
#pragma unroll
        for (int i = 0; i + 1 < S0_AHEAD; ++i) pw[i] = pw[i + 1];
        pw[S0_AHEAD - 1] = load_px(jrow + S0_AHEAD);
        i32x4 f;
        f[0] = d0;
        f[1] = d1;
        f[2] = static_cast<int>(static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, d0, 0x130, 0xf, 0xf, true)) & nb_mask);
        f[3] = static_cast<int>(static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, d1, 0x130, 0xf, 0xf, true)) & nb_mask);
        return f;
    };
    bfr[0] = next_frag(0);
    bfr[1] = next_frag(1);

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < nconv; ++it) {
        bfr[2] = next_frag(it + 2);
        f32x16 acc = mfma32<RN_DTYPE_F16>(wreg[0], bfr[0], zero);
        acc = mfma32<RN_DTYPE_F16>(wreg[1], bfr[1], acc);
        acc = mfma32<RN_DTYPE_F16>(wreg[2], bfr[2], acc);
        bfr[0] = bfr[1];
        bfr[1] = bfr[2];
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = s0_relu6(acc, j);
            const float v1 = lane_next(v);
            const float hs = (v + v1) + lane_next(v1);
            y[j] = fmaf((h2[j] + h1[j]) + hs, scale[j], shift[j]);
            h2[j] = h1[j];
            h1[j] = hs;
        }
        if (it >= 2 && lane_out)
            *reinterpret_cast<uint2*>(out_lane + static_cast<int64_t>(yo0 + it - 2) * a.So * S0_CO) =
                pack4<DT>(y[0], y[1], y[2], y[3]);
    }
}

// ------------------------------------------------------------------------ MFMA stage
template <int DT, int CIN, int COUT, int PK, int PS, bool RES, int CTW>
__global__ __launch_bounds__(512) void stage_mfma_kernel(const StageArgs a) {
    using G = StageGeom<CIN>;
    constexpr int CP = G::CP, KC = G::KC, LPT = G::LPT;
    constexpr int CT = (COUT + 31) / 32;                 // 32-wide cout tiles in the stage
    constexpr int NG = COUT >= 32 ? 4 : COUT / 8;        // groups of 4 consecutive couts per lane half-row
    constexpr int TSTRIDE = tile_stride(PK, PS);
    constexpr int NOUT_T = tile_nout(PK, PS);
    constexpr int RING = PK ? PK - 1 : 0;
    constexpr int PIXB = CIN * 2;                        // bytes per pixel
    static_assert(CIN % 8 == 0 && COUT % 8 == 0, "channels must be multiples of 8");
    static_assert(CT % CTW == 0, "cout tiles must split evenly over workgroups");
    static_assert(!PK || PS == 1 || PS == 2, "pool stride 1 or 2");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int nthreads = blockDim.x;
    const int npt = a.npt;

    int bid = blockIdx.x;
    const int ctg = bid % a.n_ctg;
    bid /= a.n_ctg;
    const int cb = bid % a.n_colblocks;
    const int band = bid / a.n_colblocks;
    const int n = blockIdx.y;

    const int ringcols = (npt - 1) * TSTRIDE + 34;
    const int rowbytes = ringcols * PIXB;
    char* const wl = smem;                                  // weights [KC][CTW][64] x 16 B
    char* const ring = smem + KC * CTW * 1024;              // NSLOT rows

    // rows of this band
    const int yo0 = band * a.rows_per_band;
    const int yo1 = min(a.Ho, yo0 + a.rows_per_band);
    const int yc0 = PK ? yo0 * PS : yo0;
    const int nconv = PK ? (yo1 - yo0 - 1) * PS + PK : (yo1 - yo0);
    const int nin = nconv + 2;
    // columns of this block
    const int x0c = cb * npt * TSTRIDE;                     // first conv / input column of the block
    const int xo_blk0 = PK ? x0c / PS : x0c;

    // ---- weights -> LDS (fragment order, lane linear)
    {
        const i32x4* src = a.wfrag;
        for (int i = tid; i < KC * CTW * 64; i += nthreads) {
            const int l = i & 63, t = i >> 6;
            const int ct = t % CTW, kc = t / CTW;
            reinterpret_cast<i32x4*>(wl)[i] = src[(kc * CT + ctg * CTW + ct) * 64 + l];
        }
    }

    // ---- input-row loader: thread owns up to LPT 16-byte chunks of a ring row
    const int nchunks = ringcols * CP;
    const unsigned short* const in_img = a.in + static_cast<int64_t>(n) * a.H * a.W * CIN;
    int ld_goff[LPT];     // element offset inside an input row, or -1 (zero fill / not mine)
    int ld_loff[LPT];     // byte offset inside a ring row
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
        const int q = tid + i * nthreads;
        const int p = q / CP, c8 = q % CP;
        ld_loff[i] = q < nchunks ? (p * CP + (c8 ^ chunk_swz<CP>(p))) * 16 : -1;
        // columns past the image edge only feed discarded lanes: clamp instead of branching
        ld_goff[i] = (q < nchunks ? min(x0c + p, a.W - 1) : 0) * CIN + c8 * 8;
    }
    i32x4 pre[LPT];
    auto fetch_row = [&](int j) {   // input row yc0 + j -> registers
        const unsigned short* row = in_img + static_cast<int64_t>(yc0 + j) * a.W * CIN;
#pragma unroll
        for (int i = 0; i < LPT; ++i) pre[i] = *reinterpret_cast<const i32x4*>(row + ld_goff[i]);
    };
    auto store_row = [&](int j) {   // registers -> ring slot j % NSLOT
        char* dst = ring + (j & (NSLOT - 1)) * rowbytes;
#pragma unroll
        for (int i = 0; i < LPT; ++i)
            if (ld_loff[i] >= 0) *reinterpret_cast<i32x4*>(dst + ld_loff[i]) = pre[i];
    };
    for (int j = 0; j < 3; ++j) {
        fetch_row(j);
        store_row(j);
    }
    __syncthreads();

    // ---- per-lane constants of this wave's pixel tile
    const int xrel0 = wave * TSTRIDE + r;             // ring column of conv column (tap kx = 0)
    int boff[3];                                      // byte offset of pixel (xrel0 + kx) chunk 0
    int bswz[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        boff[kx] = (xrel0 + kx) * PIXB;
        bswz[kx] = chunk_swz<CP>(xrel0 + kx);
    }
    const int xc = x0c + xrel0;                       // conv column of this lane
    const int xo = PK ? xc / PS : xc;                 // output column of this lane
    const bool lane_out = (PK ? (r % PS == 0 && r <= 32 - PK) : true) && xo < a.Wo &&
                          (xo - xo_blk0) < npt * NOUT_T;
    const int cout_lane = ctg * CTW * 32 + 4 * hh;    // + ct*32 + 8*g + j

    int rx_lo = 0, rx_hi = 0;
    float rx_l = 0.f;
    if constexpr (RES) {
        const int xq = min(xo, a.Wo - 1);
        rx_lo = a.rlo[xq];
        rx_hi = a.rhi[xq];
        rx_l = a.rlerp[xq];
    }

    float vring[RING > 0 ? RING : 1][CTW][16];
#pragma unroll
    for (int i = 0; i < (RING > 0 ? RING : 1); ++i)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int g = 0; g < 16; ++g) vring[i][ct][g] = 0.f;

    const char* const wl_lane = wl + lane * 16;

    for (int it = 0; it < nconv; ++it) {
        const bool have_next = it + 3 < nin;
        if (have_next) fetch_row(it + 3);

        // ---------------- implicit GEMM for conv row yc0 + it
        f32x16 acc[CTW];
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[ct][g] = 0.f;

        const char* rowp[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) rowp[ky] = ring + ((it + ky) & (NSLOT - 1)) * rowbytes;

        if constexpr (CIN >= 16) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
                const char* pb = rowp[ky] + boff[kx];
#pragma unroll
                for (int cc = 0; cc < CIN / 16; ++cc) {
                    const int kc = tap * (CIN / 16) + cc;
                    const int c8 = cc * 2 + hh;
                    const i32x4 b = *reinterpret_cast<const i32x4*>(pb + ((c8 ^ bswz[kx]) << 4));
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct) {
                        const i32x4 wv = *reinterpret_cast<const i32x4*>(wl_lane + (kc * CTW + ct) * 1024);
                        acc[ct] = mfma32<DT>(wv, b, acc[ct]);
                    }
                }
            }
        } else {
            // CIN == 8: a 16-deep chunk spans two taps; the lane half selects the tap
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                int tap = 2 * kc + hh;
                tap = tap > 8 ? 8 : tap;                      // K padded 72 -> 80: weights are zero there
                const int ky = tap / 3, kx = tap - ky * 3;
                const char* pb = ring + ((it + ky) & (NSLOT - 1)) * rowbytes + (xrel0 + kx) * PIXB;
                const i32x4 b = *reinterpret_cast<const i32x4*>(pb);
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    const i32x4 wv = *reinterpret_cast<const i32x4*>(wl_lane + (kc * CTW + ct) * 1024);
                    acc[ct] = mfma32<DT>(wv, b, acc[ct]);
                }
            }
        }

        // ---------------- ReLU6 + horizontal pool sum (lanes) + vertical pool sum (register ring)
        const int lrow = it;
        bool emit;
        int yo;
        if constexpr (PK > 0) {
            emit = lrow >= PK - 1 && ((lrow - (PK - 1)) % PS) == 0;
            yo = yo0 + (lrow - (PK - 1)) / PS;
        } else {
            emit = true;
            yo = yo0 + lrow;
        }
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) {
            float hs[16];
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const float v = relu6f(acc[ct][g]);
                if constexpr (PK == 4) {
                    const float t = v + lane_next(v);
                    hs[g] = t + lane_next(lane_next(t));
                } else if constexpr (PK == 3) {
                    const float v1 = lane_next(v);
                    hs[g] = (v + v1) + lane_next(v1);
                } else if constexpr (PK == 2) {
                    hs[g] = v + lane_next(v);
                } else {
                    hs[g] = v;
                }
            }
            float tot[16];
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float s = hs[g];
                if constexpr (RING > 0) {
                    float t = vring[0][ct][g];
#pragma unroll
                    for (int i = 1; i < RING; ++i) t += vring[i][ct][g];
                    s = t + s;
#pragma unroll
                    for (int i = 0; i + 1 < RING; ++i) vring[i][ct][g] = vring[i + 1][ct][g];
                    vring[RING - 1][ct][g] = hs[g];
                }
                tot[g] = s;
            }
            if (emit) {
                // ---------------- BN (+ residual + BN) + store, 4 consecutive channels at a time
                constexpr float inv_area = PK ? 1.0f / static_cast<float>(PK * PK) : 1.0f;
                float yl = 0.f;
                const unsigned short* sk0 = nullptr;
                const unsigned short* sk1 = nullptr;
                if constexpr (RES) {
                    const int ylo = a.rlo[yo], yhi = a.rhi[yo];
                    yl = a.rlerp[yo];
                    const unsigned short* skn = a.skip + static_cast<int64_t>(n) * a.Ss * a.Ss * COUT;
                    sk0 = skn + static_cast<int64_t>(ylo) * a.Ss * COUT;
                    sk1 = skn + static_cast<int64_t>(yhi) * a.Ss * COUT;
                }
                unsigned short* orow = a.out + ((static_cast<int64_t>(n) * a.Ho + yo) * a.Wo + xo) * COUT;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const int c0 = cout_lane + ct * 32 + 8 * g;
                    const f32x4 mean = *reinterpret_cast<const f32x4*>(a.bn_mean + c0);
                    const f32x4 inv = *reinterpret_cast<const f32x4*>(a.bn_inv + c0);
                    const f32x4 beta = *reinterpret_cast<const f32x4*>(a.bn_beta + c0);
                    float y[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[j] = (tot[4 * g + j] * inv_area - mean[j]) * inv[j] + beta[j];
                    if constexpr (RES) {
                        if (lane_out) {
                            const f32x4 tl = unpack4<DT>(*reinterpret_cast<const uint2*>(sk0 + rx_lo * COUT + c0));
                            const f32x4 tr = unpack4<DT>(*reinterpret_cast<const uint2*>(sk0 + rx_hi * COUT + c0));
                            const f32x4 bl = unpack4<DT>(*reinterpret_cast<const uint2*>(sk1 + rx_lo * COUT + c0));
                            const f32x4 br = unpack4<DT>(*reinterpret_cast<const uint2*>(sk1 + rx_hi * COUT + c0));
                            const f32x4 mean2 = *reinterpret_cast<const f32x4*>(a.bn2_mean + c0);
                            const f32x4 inv2 = *reinterpret_cast<const f32x4*>(a.bn2_inv + c0);
                            const f32x4 beta2 = *reinterpret_cast<const f32x4*>(a.bn2_beta + c0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float top = tl[j] + (tr[j] - tl[j]) * rx_l;
                                const float bot = bl[j] + (br[j] - bl[j]) * rx_l;
                                const float rs = top + (bot - top) * yl;
                                y[j] = ((y[j] + rs) - mean2[j]) * inv2[j] + beta2[j];
                            }
                        }
                    }
                    if (lane_out) *reinterpret_cast<uint2*>(orow + c0) = pack4<DT>(y[0], y[1], y[2], y[3]);
                }
            }
        }

        if (have_next) store_row(it + 3);
        __syncthreads();
    }
}

using LaunchFn = int (*)(hipStream_t, const StageArgs&, dim3, dim3, size_t);

template <int DT, int CIN, int COUT, int PK, int PS, bool RES, int CTW>
int launch_variant(hipStream_t s, const StageArgs& a, dim3 grid, dim3 block, size_t lds) {
    constexpr auto kern = stage_mfma_kernel<DT, CIN, COUT, PK, PS, RES, CTW>;
    if (int rc = rn_allow_big_lds<kern>()) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, s, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

struct Variant {
    int cin, cout, pk, ps, res, ctw;
    LaunchFn fn[2];   // [bf16, f16]
};

#define RN_VARIANT(CIN, COUT, PK, PS, RES, CTW)                                                   \
    {                                                                                             \
        CIN, COUT, PK, PS, RES, CTW, {                                                            \
            launch_variant<RN_DTYPE_BF16, CIN, COUT, PK, PS, RES != 0, CTW>,                      \
                launch_variant<RN_DTYPE_F16, CIN, COUT, PK, PS, RES != 0, CTW>                    \
        }                                                                                         \
    }

const Variant kVariants[] = {
    RN_VARIANT(8, 32, 4, 1, 0, 1),    // stage 1
    RN_VARIANT(32, 32, 4, 1, 0, 1),   // stage 2
    RN_VARIANT(32, 32, 4, 1, 1, 1),   // stage 3 (+ residual)
    RN_VARIANT(32, 64, 4, 2, 0, 2),   // stage 4
    RN_VARIANT(64, 64, 4, 2, 1, 2),   // stage 5 (+ residual)
    RN_VARIANT(64, 128, 0, 1, 0, 2),  // stage 6 (no pool; cout tiles split over 2 workgroups)
    RN_VARIANT(128, 16, 4, 2, 0, 1),  // stage 7
    RN_VARIANT(16, 16, 4, 2, 0, 1),   // stage 8
    RN_VARIANT(16, 16, 4, 2, 1, 1),   // stage 9 (+ residual)
};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

}  // namespace

// the variant of a stage shape and its geometry: as many pixel tiles per workgroup as fit the LDS next to the weights
bool rn_generic_plan(int cin, int cout, int pool_k, int pool_s, bool res, int out_side, GenericPlan* p) {
    *p = GenericPlan{};
    for (int v = 0; v < kNumVariants && p->variant < 0; ++v) {
        const Variant& k = kVariants[v];
        if (k.cin == cin && k.cout == cout && k.pk == pool_k && (pool_k == 0 || k.ps == pool_s) && k.res == (res ? 1 : 0)) p->variant = v;
    }
    if (p->variant < 0) return false;
    const int ctw = kVariants[p->variant].ctw;
    const int tstride = tile_stride(pool_k, pool_s), nout_t = tile_nout(pool_k, pool_s);
    const int tiles = (out_side + nout_t - 1) / nout_t, kc = (9 * cin + 15) / 16;
    p->npt = tiles >= 8 ? 8 : tiles;
    for (;;) {
        const int ringcols = (p->npt - 1) * tstride + 34;
        p->lds_bytes = static_cast<size_t>(kc) * ctw * 1024 + static_cast<size_t>(NSLOT) * ringcols * cin * 2;
        if (p->lds_bytes <= 160 * 1024 || p->npt == 1) break;
        --p->npt;
    }
    p->n_colblocks = (tiles + p->npt - 1) / p->npt;
    p->n_ctg = ((cout + 31) / 32) / ctw;
    return true;
}

// frag[kc][ct][lane][j] = W[k = kc*16 + 8*(lane>>5) + j][cout = ct*32 + (lane&31)]   (HWIO == [k = tap*cin + c][cout])
void rn_generic_pack(const float* w_hwio, int cin, int cout, int dtype, std::vector<unsigned short>* out) {
    const int K = 9 * cin, kc = (K + 15) / 16, ct_n = (cout + 31) / 32;
    out->assign(static_cast<size_t>(kc) * ct_n * 64 * 8, 0);
    for (int c = 0; c < kc; ++c)
        for (int t = 0; t < ct_n; ++t)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int kk = c * 16 + 8 * (l >> 5) + j, co = t * 32 + (l & 31);
                    const float v = kk < K && co < cout ? w_hwio[static_cast<size_t>(kk) * cout + co] : 0.f;
                    (*out)[((static_cast<size_t>(c) * ct_n + t) * 64 + l) * 8 + j] = rn_to16(v, dtype);
                }
}

int rn_generic_launch(const GenericPlan& p, int dtype, hipStream_t s, const StageArgs& a, int n) {
    const dim3 grid(a.n_bands * a.n_colblocks * a.n_ctg, n);
    return kVariants[p.variant].fn[dtype == RN_DTYPE_BF16 ? 0 : 1](s, a, grid, dim3(64 * p.npt), p.lds_bytes);
}

int rn_stage0_launch(int dtype, hipStream_t s, const Stage0Args& a, int n) {
    const auto kern = dtype == RN_DTYPE_BF16 ? stage0_kernel<RN_DTYPE_BF16> : stage0_kernel<RN_DTYPE_F16>;
    hipLaunchKernelGGL(kern, dim3(a.n_bands * a.n_colblocks, n), dim3(64 * a.npt), 0, s, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}
