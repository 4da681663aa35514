// Pixel stage of the split baseline-JPEG decode (the host half is rn_jpeg_host.h): int16 quantised
// coefficients in, BGR uint8 HWC images out, byte for byte libjpeg's default decode path (roomnet_amd/jpegdec.py restates it in
// NumPy and the parity tests compare all three).  Integer arithmetic throughout:
//   jpeg_idct_kernel   dequantise + jpeg_idct_islow.  8 lanes per 8x8 block, 32 blocks per workgroup: the block's rows are read
//                      as 16-byte vectors into LDS, pass 1 runs one COLUMN per lane (descale 11) into an int32 LDS workspace, pass 2
//                      one ROW per lane (descale 18, range limit) and stores the row's 8 samples as one 8-byte vector into the
//                      component's planar scratch (padded to whole blocks).  32-bit intermediates: exact for
//                      |coef * q| <= RN_JPEG_COEF_LIMIT, which rn_jpeg_entropy_decode enforces (include/roomnet_hip.h).
//   jpeg_color_kernel  4 pixels of a row per lane: "fancy" h2v1 / h2v2 chroma upsampling on the downsampled extent (replication
//                      when that is at most 2 columns), fixed-point YCbCr -> BGR, 12 bytes stored as three dwords where the row
//                      is dword-aligned.  Images with an EXIF orientation of 2..4 are stored by it at the
//                      mirrored address.
//   jpeg_color_turn_kernel  the same pixels for images of orientation 5..8, where a source row becomes an output column: 64 x 64
//                      tiles turned through LDS so that the stores stay runs of 192 contiguous bytes.  Enqueued only for a
//                      batch that holds such an image.
// Each is ONE launch per batch (blockIdx.z = image, a device table of per-image descriptors), as the batched resize is.
// HBM-bound byte work (2 B of coefficients in, 1 B of plane out and in again, 3 B of BGR out per sample); no MFMA.
#include "rn_jpeg_dev.h"
#include "rn_jpeg_host.h"

#include <algorithm>

namespace {

// One 1-D pass of jpeg_idct_islow (jidctint.c, CONST_BITS = 13) before its descale: o[k] = sum of the even and odd parts.
__device__ __forceinline__ void idct_islow_1d(const int (&x)[8], int (&o)[8]) {
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * 4433;
    const int tmp2e = z1 + z3 * (-15137);
    const int tmp3e = z1 + z2 * 6270;
    const int tmp0e = (x[0] + x[4]) * 8192;
    const int tmp1e = (x[0] - x[4]) * 8192;
    const int tmp10 = tmp0e + tmp3e, tmp13 = tmp0e - tmp3e, tmp11 = tmp1e + tmp2e, tmp12 = tmp1e - tmp2e;
    int tmp0 = x[7], tmp1 = x[5], tmp2 = x[3], tmp3 = x[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3;
    o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2;
    o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1;
    o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0;
    o[4] = tmp13 - tmp0;
}

// range_limit[v & 1023] of jdmaster.c's table, centred on 128
__device__ __forceinline__ uint32_t range_limit(int v) {
    const int m = v & 1023;
    return static_cast<uint32_t>(m < 128 ? m + 128 : (m < 512 ? 255 : (m < 896 ? 0 : m - 896)));
}

constexpr int kBlocksPerWg = 32;

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDev* __restrict__ descs) {
    const JpegDev& d = descs[blockIdx.z];
    const int comp = blockIdx.y;
    if (comp >= d.ncomp) return;
    const int bw = d.bw[comp], nblk = bw * d.bh[comp];
    const int first = blockIdx.x * kBlocksPerWg;
    if (first >= nblk) return;                     // (uniform per workgroup: in front of every barrier)
    __shared__ __attribute__((aligned(16))) int16_t s_coef[kBlocksPerWg * 64];
    __shared__ __attribute__((aligned(16))) int s_ws[kBlocksPerWg * 64];
    __shared__ int s_q[64];
    const int t = threadIdx.x, b = t >> 3, j = t & 7;
    const int blk = first + b;
    const bool live = blk < nblk;
    uint4 row = make_uint4(0, 0, 0, 0);
    if (live) row = *reinterpret_cast<const uint4*>(d.coef[comp] + static_cast<int64_t>(blk) * 64 + j * 8);
    *reinterpret_cast<uint4*>(s_coef + b * 64 + j * 8) = row;
    if (t < 64) s_q[t] = d.qt[comp][t];
    __syncthreads();
    int x[8], o[8];
    // pass 1: column j of block b
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = static_cast<int>(s_coef[b * 64 + r * 8 + j]) * s_q[r * 8 + j];
    idct_islow_1d(x, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_ws[b * 64 + r * 8 + j] = (o[r] + (1 << 10)) >> 11;
    __syncthreads();
    // pass 2: row j of block b
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = s_ws[b * 64 + j * 8 + c];
    idct_islow_1d(x, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        lo |= range_limit((o[c] + (1 << 17)) >> 18) << (8 * c);
        hi |= range_limit((o[4 + c] + (1 << 17)) >> 18) << (8 * c);
    }
    if (live) {
        const int by = blk / bw, bx = blk - by * bw;
        uint8_t* p = d.plane[comp] + (static_cast<int64_t>(by) * 8 + j) * (static_cast<int64_t>(bw) * 8) + bx * 8;
        *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    }
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// 4 upsampled chroma samples at columns x4 .. x4 + 3 of row y (x4 a multiple of 4) of a component subsampled 2:1 horizontally
// and, when v2, vertically; cw x ch is its DOWNSAMPLED extent, `stride` its plane's row length
__device__ __forceinline__ void upsample4(const uint8_t* __restrict__ p, int64_t stride, int cw, int ch, bool v2, int x4, int y,
                                          int (&out)[4]) {
    const int c0 = x4 >> 1;
    const int cm = max(c0 - 1, 0), c1 = min(c0 + 1, cw - 1), c2 = min(c0 + 2, cw - 1);
    if (!v2) {
        const uint8_t* r = p + static_cast<int64_t>(y) * stride;
        const int sm = r[cm], s0 = r[c0], s1 = r[c1], s2 = r[c2];
        if (cw <= 2) {
            out[0] = out[1] = s0;
            out[2] = out[3] = s1;
            return;
        }
        out[0] = (3 * s0 + sm + 1) >> 2;
        out[1] = (3 * s0 + s1 + 2) >> 2;
        out[2] = (3 * s1 + s0 + 1) >> 2;
        out[3] = (3 * s1 + s2 + 2) >> 2;
        return;
    }
    const int ry = y >> 1;
    const uint8_t* r = p + static_cast<int64_t>(ry) * stride;
    if (cw <= 2) {
        out[0] = out[1] = r[c0];
        out[2] = out[3] = r[c1];
        return;
    }
    const int rn = (y & 1) ? min(ry + 1, ch - 1) : max(ry - 1, 0);
    const uint8_t* q = p + static_cast<int64_t>(rn) * stride;
    const int tm = 3 * r[cm] + q[cm], t0 = 3 * r[c0] + q[c0], t1 = 3 * r[c1] + q[c1], t2 = 3 * r[c2] + q[c2];
    out[0] = (3 * t0 + tm + 8) >> 4;
    out[1] = (3 * t0 + t1 + 7) >> 4;
    out[2] = (3 * t1 + t0 + 8) >> 4;
    out[3] = (3 * t1 + t2 + 7) >> 4;
}

// The arithmetic of a pixel, stated once for both colour kernels: 4 pixels at columns x4 .. x4 + 3 (x4 a multiple of 4) of row y,
// both in STORED geometry -- the luma read, the chroma reads or upsample4, the three colour formulas and the clamp -- each as
// b | g << 8 | r << 16.  (Columns at or past the width are computed from the planes' padding; the callers store none of them.)
__device__ __forceinline__ void jpeg_pixels4(const JpegDev& d, int x4, int y, uint32_t (&px)[4]) {
    const int W = d.width, H = d.height;
    // (the luma plane's rows are whole blocks: the 4 bytes at x4 are inside the row whatever W is)
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(d.plane[0] + static_cast<int64_t>(y) * (d.bw[0] * 8) + x4);
    if (d.ncomp == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = ((y4 >> (8 * k)) & 255) * 0x010101u;
        return;
    }
    int cb[4], cr[4];
    const int64_t cs = static_cast<int64_t>(d.bw[1]) * 8;
    if (d.hsamp == 1) {
        const uint32_t cb4 = *reinterpret_cast<const uint32_t*>(d.plane[1] + y * cs + x4);
        const uint32_t cr4 = *reinterpret_cast<const uint32_t*>(d.plane[2] + y * cs + x4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cb[k] = (cb4 >> (8 * k)) & 255;
            cr[k] = (cr4 >> (8 * k)) & 255;
        }
    } else {
        const bool v2 = d.vsamp == 2;
        const int cw = (W + 1) >> 1, ch = v2 ? (H + 1) >> 1 : H;
        upsample4(d.plane[1], cs, cw, ch, v2, x4, y, cb);
        upsample4(d.plane[2], cs, cw, ch, v2, x4, y, cr);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = (y4 >> (8 * k)) & 255, u = cb[k] - 128, v = cr[k] - 128;
        const int r = clamp255(yy + ((91881 * v + 32768) >> 16));
        const int b = clamp255(yy + ((116130 * u + 32768) >> 16));
        const int g = clamp255(yy + ((-22554 * u - 46802 * v + 32768) >> 16));
        px[k] = static_cast<uint32_t>(b | (g << 8) | (r << 16));
    }
}

// Orientations 1..4 (rows stay rows): the 12-byte run of a lane's 4 pixels goes to row y or H - 1 - y, at
// column x4 or, with the pixels reversed inside it, at W - 4 - x4.  Images of orientation 5..8 are jpeg_color_turn_kernel's.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegDev* __restrict__ descs) {
    const JpegDev& d = descs[blockIdx.z];
    const int orient = d.orient;
    if (orient >= 5) return;
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int W = d.width, H = d.height;
    if (x4 >= W || y >= H) return;
    uint32_t px[4];
    jpeg_pixels4(d, x4, y, px);
    int ox = x4;                   // column of the run's first pixel; negative: the run begins left of the row (mirrored edge run)
    if (orient == 2 || orient == 3) {
        ox = W - 4 - x4;
        uint32_t t = px[0];
        px[0] = px[3];
        px[3] = t;
        t = px[1];
        px[1] = px[2];
        px[2] = t;
    }
    const int oy = orient >= 3 ? H - 1 - y : y;
    uint8_t* row = d.bgr + static_cast<int64_t>(oy) * W * 3;
    uint8_t* o = row + static_cast<int64_t>(ox) * 3;
    if (ox >= 0 && ox + 3 < W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
        o32[0] = px[0] | (px[1] << 24);
        o32[1] = (px[1] >> 8) | (px[2] << 16);
        o32[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int k = 0; k < 4; ++k) {
            const int x = ox + k;
            if (x < 0 || x >= W) continue;
            row[3 * x] = static_cast<uint8_t>(px[k]);
            row[3 * x + 1] = static_cast<uint8_t>(px[k] >> 8);
            row[3 * x + 2] = static_cast<uint8_t>(px[k] >> 16);
        }
    }
}

// Orientations 5..8 (a source row becomes an output column).  One workgroup takes a kTurnTile x kTurnTile
// tile of SOURCE pixels: it computes them with jpeg_pixels4 (16 lanes x 4 pixels across, 16 rows per step), writes each as one
// dword into LDS at its turned position, passes one barrier, and stores the tile's output rows from LDS: runs of up to 64 pixels
// = 192 contiguous bytes, as dwords from the first 4-byte boundary of the run on and as bytes at its two ends.
// LDS pitch 65 dwords.  Phase 1 (ds_write_b32, banks = dword address mod 32, lanes conflict within a 32-lane half): a half holds
// 16 column groups x 2 source rows and writes dword (4 c + j) * 65 + row, bank (4 c + j + row) mod 32: groups c and c + 8 meet,
// the two rows never do -- 2-way, which a ds_write_b32 absorbs (its 4 issue cycles cover 2 LDS-array cycles per half).  Phase 2
// (ds_read_b32): lane 4 g + m (m < 3) builds dword 3 g + m of the run from pixels p and p + 1 with p in 4 g .. 4 g + 3, distinct for
// m = 0, 1, 2 whatever the run's alignment -- 24 distinct dwords of one LDS row per half: conflict-free.  The lanes m = 3 store the
// end bytes (at most 6 per run).
constexpr int kTurnTile = 64;
[[maybe_unused]] constexpr int kTurnPitch = kTurnTile + 1;      // (unused in a -DJPEG_TURN_DIRECT build)

__global__ __launch_bounds__(256) void jpeg_color_turn_kernel(const JpegDev* __restrict__ descs) {
    const JpegDev& d = descs[blockIdx.z];
    const int orient = d.orient;
    if (orient < 5) return;
    const int W = d.width, H = d.height;
    const int sx0 = blockIdx.x * kTurnTile, sy0 = blockIdx.y * kTurnTile;
    if (sx0 >= W || sy0 >= H) return;              // (uniform per workgroup: in front of the barrier)
    const int ncols = min(kTurnTile, W - sx0), nrows = min(kTurnTile, H - sy0);      // the tile's source extent
    // output O is W x H (rows x columns): O[oy][ox] = I[sy][sx] with ox = sy (5, 8) or H - 1 - sy (6, 7), oy = sx (5, 6) or
    // W - 1 - sx (7, 8).  The tile's output extent is ncols rows of nrows pixels from (oy0, ox0).
    const bool flip_x = orient == 6 || orient == 7, flip_y = orient >= 7;
    const int ox0 = flip_x ? H - sy0 - nrows : sy0;
    const int oy0 = flip_y ? W - sx0 - ncols : sx0;
    const int t = threadIdx.x, cx = (t & 15) * 4;
#ifndef JPEG_TURN_DIRECT
    __shared__ uint32_t s_tile[kTurnTile * kTurnPitch];
#endif
    for (int sy = t >> 4; sy < nrows; sy += 16) {
        if (cx >= ncols) continue;
        uint32_t px[4];
        jpeg_pixels4(d, sx0 + cx, sy0 + sy, px);
        const int lx = flip_x ? nrows - 1 - sy : sy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cx + j >= ncols) continue;
            const int ly = flip_y ? ncols - 1 - (cx + j) : cx + j;
#ifndef JPEG_TURN_DIRECT
            s_tile[ly * kTurnPitch + lx] = px[j];
#else
            // the comparison arm: 3 bytes at a stride of 3 H straight from registers
            uint8_t* o = d.bgr + (static_cast<int64_t>(oy0 + ly) * H + ox0 + lx) * 3;
            o[0] = static_cast<uint8_t>(px[j]);
            o[1] = static_cast<uint8_t>(px[j] >> 8);
            o[2] = static_cast<uint8_t>(px[j] >> 16);
#endif
        }
    }
#ifndef JPEG_TURN_DIRECT
    __syncthreads();
    const int lane = t & 63, g = lane >> 2, m = lane & 3;
    const int run_bytes = nrows * 3;
    for (int ly = t >> 6; ly < ncols; ly += 4) {
        uint8_t* run = d.bgr + (static_cast<int64_t>(oy0 + ly) * H + ox0) * 3;
        const uint32_t* src = s_tile + ly * kTurnPitch;
        const int head = static_cast<int>((0 - reinterpret_cast<uintptr_t>(run)) & 3);      // bytes in front of the first boundary
        const int ndw = run_bytes > head ? (run_bytes - head) >> 2 : 0;
        if (m < 3) {
            const int k = 3 * g + m;
            if (k < ndw) {                         // bytes n .. n + 3 of the run: pixels p and p + 1 <= nrows - 1
                const int n = head + 4 * k, p = n / 3;
                const uint64_t two = src[p] | (static_cast<uint64_t>(src[p + 1]) << 24);
                *reinterpret_cast<uint32_t*>(run + n) = static_cast<uint32_t>(two >> (8 * (n - 3 * p)));
            }
        } else if (g < 6) {                        // end byte g: the head's, then the tail's (at most 3 each)
            const int n = g < head ? g : head + 4 * ndw + (g - head);
            if (n < run_bytes) run[n] = static_cast<uint8_t>(src[n / 3] >> (8 * (n % 3)));
        }
    }
#endif
}

}  // namespace

// the stage's state (rn_jpeg_dev.h), allocated by the first call
int rn_jpeg_state(rn_handle* h, JpegState** out) {
    if (!h->jpeg) {
        JpegState* s = new JpegState();
        h->jpeg = s;               // (rn_jpeg_release frees whatever of it exists)
        s->bgr_ptrs.resize(static_cast<size_t>(h->max_batch));
        int rc;
        for (auto& t : s->desc)
            if ((rc = t.alloc(static_cast<size_t>(h->max_batch))) != RN_OK) return rc;
        if ((rc = s->turn.create()) != RN_OK || (rc = s->timer.create()) != RN_OK) return rc;
        RN_HIP(hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming));
        RN_HIP(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
        s->ready = true;
    }
    *out = static_cast<JpegState*>(h->jpeg);
    if (!(*out)->ready) {
        rn_set_error("rn_jpeg: the stage's state could not be allocated earlier");
        return RN_E_STATE;
    }
    if (!h->copy_stream) RN_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    return RN_OK;
}

// a supported image as rn_jpeg_probe or rn_jpeg_probe_oriented fills it (supported 1, or the orientation 2..8): every size the
// kernels index with is recomputed from width, height and sampling
bool rn_jpeg_info_ok(const rn_jpeg_info& f) {
    if (f.supported < 1 || f.supported > 8 || f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return false;
    if (f.ncomp != 1 && f.ncomp != 3) return false;
    const bool s11 = f.hsamp == 1 && f.vsamp == 1, s21 = f.hsamp == 2 && f.vsamp == 1, s22 = f.hsamp == 2 && f.vsamp == 2;
    if (!(s11 || ((s21 || s22) && f.ncomp == 3))) return false;
    const int mx = (f.width + 8 * f.hsamp - 1) / (8 * f.hsamp), my = (f.height + 8 * f.vsamp - 1) / (8 * f.vsamp);
    for (int c = 0; c < f.ncomp; ++c)
        if (f.blocks_w[c] != mx * (c == 0 ? f.hsamp : 1) || f.blocks_h[c] != my * (c == 0 ? f.vsamp : 1)) return false;
    return true;
}

namespace {

// Upload + the launches (two; three when an image of orientation 5..8 is among them) for n checked images, all with host coefficients or all with coefficients a launch on the handle's stream
// left in device memory.  d_bgr == nullptr: into the handle's own image scratch (st->bgr_ptrs).
int enqueue_decode(rn_handle* h, JpegState* st, const rn_jpeg_job* jobs, int n, uint8_t* const* d_bgr) {
    size_t coef_total = 0, plane_total = 0, bgr_total = 0;
    int max_blocks = 0, max_w = 0, max_h = 0, turn_w = 0, turn_h = 0;      // (stored sizes; turn_*: of the images of orientation 5..8)
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_info& f = *jobs[i].info;
        for (int c = 0; c < f.ncomp; ++c) {
            const int nb = f.blocks_w[c] * f.blocks_h[c];          // <= 8192 * 8192
            if (!jobs[i].on_device) coef_total += static_cast<size_t>(nb) * 64;
            plane_total += static_cast<size_t>(nb) * 64;
            max_blocks = std::max(max_blocks, nb);
        }
        bgr_total += (static_cast<size_t>(f.width) * f.height * 3 + 15) & ~static_cast<size_t>(15);
        max_w = std::max(max_w, f.width);
        max_h = std::max(max_h, f.height);
        if (f.supported >= 5) {
            turn_w = std::max(turn_w, f.width);
            turn_h = std::max(turn_h, f.height);
        }
    }
    int rc, set;
    if ((rc = st->turn.acquire(&set)) != RN_OK) return rc;
    const rn_table<JpegDev>& tab = st->desc[set];
    if ((rc = rn_grow_scratch(h, &st->d_coef, &st->coef_cap, coef_total, "JPEG coefficients")) != RN_OK) return rc;
    if ((rc = rn_grow_scratch(h, &st->d_planes, &st->planes_cap, plane_total, "JPEG planes")) != RN_OK) return rc;
    if (!d_bgr && (rc = rn_grow_scratch(h, &st->d_bgr, &st->bgr_cap, bgr_total, "decoded images")) != RN_OK) return rc;
    // the previous call's launches read the coefficient scratch: the copy stream starts behind them
    RN_HIP(hipStreamWaitEvent(h->copy_stream, st->done, 0));
    size_t coef_off = 0, plane_off = 0, bgr_off = 0;
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_info& f = *jobs[i].info;
        JpegDev& d = tab.host[i];
        std::memset(&d, 0, sizeof(d));
        size_t count = 0;
        for (int c = 0; c < f.ncomp; ++c) {
            const size_t nb = static_cast<size_t>(f.blocks_w[c]) * f.blocks_h[c] * 64;
            d.coef[c] = (jobs[i].on_device ? jobs[i].coeffs : st->d_coef + coef_off) + count;
            d.plane[c] = st->d_planes + plane_off + count;
            d.bw[c] = f.blocks_w[c];
            d.bh[c] = f.blocks_h[c];
            std::memcpy(d.qt[c], f.qt[c], sizeof(d.qt[c]));
            count += nb;
        }
        if (!jobs[i].on_device) {
            RN_HIP(hipMemcpyAsync(st->d_coef + coef_off, jobs[i].coeffs, count * sizeof(int16_t), hipMemcpyHostToDevice, h->copy_stream));
            coef_off += count;
        }
        plane_off += count;
        d.width = f.width;
        d.height = f.height;
        d.ncomp = f.ncomp;
        d.hsamp = f.hsamp;
        d.vsamp = f.vsamp;
        d.orient = f.supported;
        if (d_bgr) {
            d.bgr = d_bgr[i];
        } else {
            d.bgr = st->bgr_ptrs[i] = st->d_bgr + bgr_off;
            bgr_off += (static_cast<size_t>(f.width) * f.height * 3 + 15) & ~static_cast<size_t>(15);
        }
    }
    RN_HIP(hipEventRecord(st->uploaded, h->copy_stream));
    if ((rc = tab.upload(static_cast<size_t>(n), h->stream)) != RN_OK) return rc;
    RN_HIP(hipStreamWaitEvent(h->stream, st->uploaded, 0));
    if ((rc = st->timer.start(h->stream)) != RN_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg, 3, n), dim3(256), 0, h->stream, tab.dev);
    RN_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((max_w + 255) / 256, (max_h + 3) / 4, n), dim3(256), 0, h->stream, tab.dev);
    RN_CHECK_LAUNCH();
    if (turn_w) {
        hipLaunchKernelGGL(jpeg_color_turn_kernel, dim3((turn_w + kTurnTile - 1) / kTurnTile, (turn_h + kTurnTile - 1) / kTurnTile, n),
                           dim3(256), 0, h->stream, tab.dev);
        RN_CHECK_LAUNCH();
    }
    if ((rc = st->timer.stop(h->stream)) != RN_OK) return rc;
    RN_HIP(hipEventRecord(st->done, h->stream));
    return st->turn.retire(h->stream);
}

int check_images(const char* who, rn_handle* h, const rn_jpeg_image* ims, int n) {
    const int rc = rn_check_batch(who, h, ims, n);
    if (rc != RN_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (!ims[i].coeffs || !rn_jpeg_info_ok(ims[i].info)) {
            rn_set_error("%s: image %d is not a supported JPEG as rn_jpeg_probe[_oriented] describes one (%dx%d, %d components, sampling %dx%d, supported %d)",
                         who, i, ims[i].info.width, ims[i].info.height, ims[i].info.ncomp, ims[i].info.hsamp, ims[i].info.vsamp,
                         ims[i].info.supported);
            return RN_E_INVALID;
        }
    return RN_OK;
}

std::vector<rn_jpeg_job> host_jobs(const rn_jpeg_image* ims, int n) {
    std::vector<rn_jpeg_job> jobs(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) jobs[static_cast<size_t>(i)] = rn_jpeg_job{&ims[i].info, ims[i].coeffs, false};
    return jobs;
}

}  // namespace

int rn_jpeg_classify_jobs(rn_handle* h, JpegState* st, const rn_jpeg_job* jobs, int n, float* probs, int64_t* ids) {
    int rc = enqueue_decode(h, st, jobs, n, nullptr);
    if (rc != RN_OK) return rc;
    // from here on it is rn_crop_resize_batch_u8_device + rn_forward_u8_device, as rn_classify_images_u8 runs them
    rc = rn_enqueue_resize_batch(h, n, h->d_in_u8, [&](int i) { return rn_center_window(st->bgr_ptrs[i], rn_jpeg_out_height(*jobs[i].info), rn_jpeg_out_width(*jobs[i].info)); });
    if (rc != RN_OK) return rc;
    if ((rc = rn_forward_u8_device(h, h->d_in_u8, n, h->d_probs, h->d_ids)) != RN_OK) return rc;
    return rn_results_to_host(h, n, probs, ids);
}

void rn_jpeg_release(rn_handle* h) {
    JpegState* s = static_cast<JpegState*>(h->jpeg);
    if (!s) return;
    if (s->d_coef) (void)hipFree(s->d_coef);
    if (s->d_planes) (void)hipFree(s->d_planes);
    if (s->d_bgr) (void)hipFree(s->d_bgr);
    if (s->d_scan) (void)hipFree(s->d_scan);
    if (s->d_chain) (void)hipFree(s->d_chain);
    for (hipEvent_t e : {s->uploaded, s->done, s->scan_done})
        if (e) (void)hipEventDestroy(e);
    delete s;                      // (the tables, their rotation and the timer free themselves)
    h->jpeg = nullptr;
}

extern "C" int rn_jpeg_probe(const uint8_t* data, size_t len, rn_jpeg_info* out) {
    if (!data || !out) {
        rn_set_error("rn_jpeg_probe: null argument");
        return RN_E_INVALID;
    }
    static thread_local rn_jpeg::Parsed p;
    const int rc = rn_jpeg::parse(data, len, p);
    if (rc != RN_OK) {
        rn_set_error("rn_jpeg_probe: not a JPEG file, or its headers are truncated");
        return rc;
    }
    *out = p.info;
    return RN_OK;
}

extern "C" int rn_jpeg_probe_oriented(const uint8_t* data, size_t len, rn_jpeg_info* out) {
    if (!data || !out) {
        rn_set_error("rn_jpeg_probe_oriented: null argument");
        return RN_E_INVALID;
    }
    static thread_local rn_jpeg::Parsed p;
    const int rc = rn_jpeg::parse(data, len, p, true);
    if (rc != RN_OK) {
        rn_set_error("rn_jpeg_probe_oriented: not a JPEG file, or its headers are truncated");
        return rc;
    }
    *out = p.info;
    return RN_OK;
}

extern "C" int rn_jpeg_oriented_size(const rn_jpeg_info* info, int* height, int* width) {
    if (!info || !height || !width || !rn_jpeg_info_ok(*info)) {
        rn_set_error("rn_jpeg_oriented_size: a null pointer, or not a supported info as rn_jpeg_probe[_oriented] fills it");
        return RN_E_INVALID;
    }
    *height = rn_jpeg_out_height(*info);
    *width = rn_jpeg_out_width(*info);
    return RN_OK;
}

extern "C" size_t rn_jpeg_coeff_count(const rn_jpeg_info* info) {
    if (!info || !rn_jpeg_info_ok(*info)) return 0;
    return rn_jpeg::coeff_count(*info);
}

extern "C" int rn_jpeg_entropy_decode(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap) {
    const char* why = "";
    const int rc = rn_jpeg::entropy_decode(data, len, info, coeffs, cap, &why);
    if (rc != RN_OK) rn_set_error("rn_jpeg_entropy_decode: %s", why);
    return rc;
}

extern "C" int rn_jpeg_decode_batch_device(rn_handle* h, const rn_jpeg_image* ims, int n, uint8_t* const* d_bgr) {
    int rc = check_images("rn_jpeg_decode_batch_device", h, ims, n);
    if (rc != RN_OK) return rc;
    if (!d_bgr) {
        rn_set_error("rn_jpeg_decode_batch_device: null argument");
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i)
        if (!d_bgr[i]) {
            rn_set_error("rn_jpeg_decode_batch_device: image %d has no destination", i);
            return RN_E_INVALID;
        }
    DeviceGuard guard(h->device);
    JpegState* st = nullptr;
    if ((rc = rn_jpeg_state(h, &st)) != RN_OK) return rc;
    return enqueue_decode(h, st, host_jobs(ims, n).data(), n, d_bgr);
}

extern "C" int rn_classify_jpegs(rn_handle* h, const rn_jpeg_image* ims, int n, float* probs, int64_t* ids) {
    int rc = check_images("rn_classify_jpegs", h, ims, n);
    if (rc != RN_OK) return rc;
    if (!probs || !ids) {
        rn_set_error("rn_classify_jpegs: null buffer");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    JpegState* st = nullptr;
    if ((rc = rn_jpeg_state(h, &st)) != RN_OK) return rc;
    return rn_jpeg_classify_jobs(h, st, host_jobs(ims, n).data(), n, probs, ids);
}

extern "C" int rn_jpeg_last_decode_ms(rn_handle* h, float* ms) {
    const JpegState* st = h ? static_cast<const JpegState*>(h->jpeg) : nullptr;
    return rn_timer::read("rn_jpeg_last_decode_ms", h, st ? &st->timer : nullptr, "no JPEG batch has been decoded on this handle",
                          h ? h->device : 0, ms);
}
