// The overlay and the pixel stage of the split baseline-JPEG encode (the host half is rn_jpeg_host.h): BGR
// uint8 HWC images in device memory in, int16 quantised coefficients out, bit for bit libjpeg's default compress path at 4:2:0
// (roomnet_amd/jpegenc.py restates it in NumPy and the parity tests compare it with Pillow's files).  rn_jpeg.hip mirrored:
//   jpeg_overlay_kernel  one pixel of an overlay's box per lane: v += (colour - v) * coverage in float32 without contraction,
//                        round-half-even, clamp.  One launch per overlay RANK (an image's overlays may overlap and are applied in
//                        order, with the uint8 rounding between them).
//   jpeg_ycc_kernel      2 x 4 luma pixels per lane: fixed-point BGR -> YCbCr (jccolor.c), the rows extended to the luma block
//                        grid by their last column and downwards by their last row, h2v2 downsampling with the alternating bias
//                        (jcsample.c) on the image extended by one row when its height is odd, the downsampled rows replicated
//                        down to the chroma block grid.  12 bytes of a row are read as three dwords where they are dword-aligned
//                        and inside the row; 4 luma bytes and 2 + 2 chroma bytes are stored as one vector each.
//   jpeg_fdct_kernel     8 lanes per 8x8 block, 32 blocks per workgroup: a lane reads one ROW of samples as 8 bytes, runs pass 1
//                        of jpeg_fdct_islow on it in registers into an int32 LDS workspace, pass 2 runs one COLUMN per lane,
//                        quantises (multiply-high by the table's reciprocals: exact, jpegenc.quantise_mulhi) into LDS, and each
//                        lane stores one row of 8 coefficients as one 16-byte vector.  Luma blocks beyond the image's own blocks
//                        transform the block whose DC libjpeg repeats there and keep only that DC.
// All are ONE launch per batch (blockIdx.z = image, a device table of per-image descriptors).  HBM-bound byte work (3 B of BGR in,
// 1.5 B of planes out and in again, 3 B of coefficients out per pixel); no MFMA.  32-bit intermediates are exact (include/roomnet_hip.h).
#include "rn_internal.h"
#include "rn_jpeg_host.h"

#include <algorithm>

namespace {

struct EncDev {
    const uint8_t* bgr;       // [height][width][3]
    uint8_t* plane[3];        // [blocks_h * 8][blocks_w * 8] per component
    int16_t* coef[3];         // [blocks_h][blocks_w][64] per component
    int32_t width, height;
    int32_t bw[3], bh[3];
    uint16_t q[2][64];        // luma / chroma table, natural order
    uint32_t recip[2][64];    // ceil(2^32 / (8 q))
};

struct OverlayDev {
    uint8_t* bgr;
    const float* cov;         // device, [h][w]
    int32_t x, y, w, h;       // w == 0: the image has no overlay of this rank
    int32_t stride;           // the image's width
    float col[3];
};

__global__ __launch_bounds__(256) void jpeg_overlay_kernel(const OverlayDev* __restrict__ table) {
    const OverlayDev& o = table[blockIdx.z];
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= o.w || py >= o.h) return;
    const float c = o.cov[static_cast<int64_t>(py) * o.w + px];
    uint8_t* p = o.bgr + (static_cast<int64_t>(o.y + py) * o.stride + (o.x + px)) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = static_cast<float>(p[k]);
        const float r = rintf(__fadd_rn(v, __fmul_rn(__fsub_rn(o.col[k], v), c)));
        p[k] = static_cast<uint8_t>(fminf(fmaxf(r, 0.f), 255.f));
    }
}

// pixels x4 .. x4 + 3 of a row (columns clamped to w - 1), each as b | g << 8 | r << 16
__device__ __forceinline__ void load_px4(const uint8_t* __restrict__ row, int x4, int w, uint32_t (&px)[4]) {
    const uint8_t* p = row + static_cast<int64_t>(x4) * 3;
    if (x4 + 3 < w && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
        const uint32_t a = p32[0], b = p32[1], c = p32[2];
        px[0] = a & 0xFFFFFFu;
        px[1] = (a >> 24) | ((b & 0xFFFFu) << 8);
        px[2] = (b >> 16) | ((c & 0xFFu) << 16);
        px[3] = c >> 8;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* q = row + static_cast<int64_t>(min(x4 + k, w - 1)) * 3;
            px[k] = q[0] | (q[1] << 8) | (q[2] << 16);
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_ycc_kernel(const EncDev* __restrict__ descs) {
    const EncDev& d = descs[blockIdx.z];
    const int cx2 = blockIdx.x * 64 + (threadIdx.x & 63);      // a pair of chroma columns = 4 luma columns
    const int cy = blockIdx.y * 4 + (threadIdx.x >> 6);         // a chroma row = 2 luma rows
    const int CW = d.bw[1] * 8, CH = d.bh[1] * 8;
    if (cx2 * 2 >= CW || cy >= CH) return;
    const int W = d.width, H = d.height, x4 = cx2 * 4;
    const int64_t src_row = static_cast<int64_t>(W) * 3;
    const int ch = (H + 1) >> 1;
    int sb[2] = {0, 0}, sr[2] = {0, 0};           // sums of Cb / Cr over the two 2x2 windows
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t px[4];
        load_px4(d.bgr + min(2 * cy + r, H - 1) * src_row, x4, W, px);
        uint32_t y4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = px[k] & 255, g = (px[k] >> 8) & 255, rr = px[k] >> 16;
            y4 |= static_cast<uint32_t>((19595 * rr + 38470 * g + 7471 * b + 32768) >> 16) << (8 * k);
            sb[k >> 1] += (-11059 * rr - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
            sr[k >> 1] += (32768 * rr - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
        }
        *reinterpret_cast<uint32_t*>(d.plane[0] + (static_cast<int64_t>(2 * cy + r) * CW + cx2 * 2) * 2) = y4;   // (the luma row is 2 CW long)
    }
    if (cy >= ch) {
        // below the downsampled extent: the component's own last row, which is NOT the downsampling of replicated image rows
        // when the height is even
        sb[0] = sb[1] = sr[0] = sr[1] = 0;
        const int cye = ch - 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t px[4];
            load_px4(d.bgr + min(2 * cye + r, H - 1) * src_row, x4, W, px);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = px[k] & 255, g = (px[k] >> 8) & 255, rr = px[k] >> 16;
                sb[k >> 1] += (-11059 * rr - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                sr[k >> 1] += (32768 * rr - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
        }
    }
    // bias 1 for even output columns, 2 for odd ones
    const int64_t co = static_cast<int64_t>(cy) * CW + cx2 * 2;
    *reinterpret_cast<uint16_t*>(d.plane[1] + co) = static_cast<uint16_t>(((sb[0] + 1) >> 2) | (((sb[1] + 2) >> 2) << 8));
    *reinterpret_cast<uint16_t*>(d.plane[2] + co) = static_cast<uint16_t>(((sr[0] + 1) >> 2) | (((sr[1] + 2) >> 2) << 8));
}

// One 1-D pass of jpeg_fdct_islow (jfdctint.c, CONST_BITS = 13) before its descales: o[0], o[4] are tmp10 +- tmp11, the others
// carry 13 more fraction bits.
__device__ __forceinline__ void fdct_islow_1d(const int (&x)[8], int (&o)[8]) {
    const int tmp0 = x[0] + x[7], tmp7 = x[0] - x[7], tmp1 = x[1] + x[6], tmp6 = x[1] - x[6];
    const int tmp2 = x[2] + x[5], tmp5 = x[2] - x[5], tmp3 = x[3] + x[4], tmp4 = x[3] - x[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    o[0] = tmp10 + tmp11;
    o[4] = tmp10 - tmp11;
    int z1 = (tmp12 + tmp13) * 4433;
    o[2] = z1 + tmp13 * 6270;
    o[6] = z1 + tmp12 * (-15137);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    o[7] = t4 + z1 + z3;
    o[5] = t5 + z2 + z4;
    o[3] = t6 + z2 + z3;
    o[1] = t7 + z1 + z4;
}

constexpr int kBlocksPerWg = 32;
constexpr int kWsStride = 9;      // ints per workspace row: lanes j of a block write rows j, 9 apart, to different banks

__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const EncDev* __restrict__ descs) {
    const EncDev& d = descs[blockIdx.z];
    const int comp = blockIdx.y;
    const int bw = d.bw[comp], nblk = bw * d.bh[comp];
    const int first = blockIdx.x * kBlocksPerWg;
    if (first >= nblk) return;                     // (uniform per workgroup: in front of every barrier)
    __shared__ int s_ws[kBlocksPerWg * 8 * kWsStride];
    __shared__ __attribute__((aligned(16))) int16_t s_out[kBlocksPerWg * 64];
    __shared__ uint32_t s_q4[64], s_recip[64];
    const int t = threadIdx.x, b = t >> 3, j = t & 7;
    const int blk = first + b;
    const bool live = blk < nblk;
    const int tab = comp ? 1 : 0;
    if (t < 64) {
        s_q4[t] = 4u * d.q[tab][t];
        s_recip[t] = d.recip[tab][t];
    }
    int x[8], o[8];
    bool dummy = false;
    {
        // pass 1: row j of the block's samples
        uint2 row = make_uint2(0x80808080u, 0x80808080u);
        if (live) {
            int by = blk / bw, bx = blk - by * bw;
            if (comp == 0) {
                // blocks beyond the image's own: the block before them in MCU order (the left one; below the last block row,
                // the right-hand block of the MCU's top row), of which only the DC is kept
                const int vb_w = (d.width + 7) >> 3, vb_h = (d.height + 7) >> 3;
                dummy = by >= vb_h || bx >= vb_w;
                bx = min(by < vb_h ? bx : (bx | 1), vb_w - 1);
                by = min(by, vb_h - 1);
            }
            row = *reinterpret_cast<const uint2*>(d.plane[comp] + (static_cast<int64_t>(by) * 8 + j) * (static_cast<int64_t>(bw) * 8) + bx * 8);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            x[c] = static_cast<int>((row.x >> (8 * c)) & 255u) - 128;
            x[4 + c] = static_cast<int>((row.y >> (8 * c)) & 255u) - 128;
        }
        fdct_islow_1d(x, o);
        int* w = s_ws + (b * 8 + j) * kWsStride;
        w[0] = o[0] << 2;
        w[4] = o[4] << 2;
#pragma unroll
        for (int c = 1; c < 8; ++c)
            if (c != 4) w[c] = (o[c] + (1 << 10)) >> 11;
    }
    __syncthreads();
    // pass 2: column j
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = s_ws[(b * 8 + r) * kWsStride + j];
    fdct_islow_1d(x, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int c = (r & 3) == 0 ? (o[r] + 2) >> 2 : (o[r] + (1 << 14)) >> 15;
        const uint32_t a = static_cast<uint32_t>(c < 0 ? -c : c);
        const int v = static_cast<int>(__umulhi(a + s_q4[r * 8 + j], s_recip[r * 8 + j]));      // (|c| + 4 q) / (8 q)
        const bool keep = !dummy || (r == 0 && j == 0);
        s_out[b * 64 + r * 8 + j] = static_cast<int16_t>(keep ? (c < 0 ? -v : v) : 0);
    }
    __syncthreads();
    if (live)
        *reinterpret_cast<uint4*>(d.coef[comp] + static_cast<int64_t>(blk) * 64 + j * 8) = *reinterpret_cast<const uint4*>(s_out + b * 64 + j * 8);
}

// One set of the per-batch tables (rn_batch_table.h): the next call never overwrites a table, or a coverage array, that a launch
// still reads.
struct EncSet {
    rn_table<EncDev> desc;             // [max_batch]
    rn_table<OverlayDev> ov;           // [RN_JPEG_MAX_OVERLAYS][max_batch]
    rn_table<float> cov;               // grows with the batch's boxes
};

struct EncState {
    EncSet set[2];
    rn_rotation turn;
    uint8_t* d_planes = nullptr;
    size_t planes_cap = 0;
    int16_t* d_coef = nullptr;
    size_t coef_cap = 0;               // int16 elements
    hipEvent_t encoded = nullptr, downloaded = nullptr;
    rn_timer timer;
    bool ready = false;
};

int enc_state(rn_handle* h, EncState** out) {
    if (!h->jpeg_enc) {
        EncState* s = new EncState();
        h->jpeg_enc = s;               // (rn_jpeg_enc_release frees whatever of it exists)
        const size_t nb = static_cast<size_t>(h->max_batch);
        int rc;
        for (EncSet& e : s->set)
            if ((rc = e.desc.alloc(nb)) != RN_OK || (rc = e.ov.alloc(nb * RN_JPEG_MAX_OVERLAYS)) != RN_OK) return rc;
        if ((rc = s->turn.create()) != RN_OK || (rc = s->timer.create()) != RN_OK) return rc;
        RN_HIP(hipEventCreateWithFlags(&s->encoded, hipEventDisableTiming));
        RN_HIP(hipEventCreateWithFlags(&s->downloaded, hipEventDisableTiming));
        s->ready = true;
    }
    *out = static_cast<EncState*>(h->jpeg_enc);
    if (!(*out)->ready) {
        rn_set_error("rn_jpeg_encode: the stage's state could not be allocated earlier");
        return RN_E_STATE;
    }
    if (!h->copy_stream) RN_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    return RN_OK;
}

int check_sources(const char* who, rn_handle* h, const rn_jpeg_source* srcs, int n, bool need_coeffs) {
    const int rc = rn_check_batch(who, h, srcs, n);
    if (rc != RN_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_source& s = srcs[i];
        if (!rn_jpeg::encode_info_ok(s.info)) {
            rn_set_error("%s: image %d: the info is not one rn_jpeg_encode_info fills (%dx%d, %d components, sampling %dx%d, supported %d)",
                         who, i, s.info.width, s.info.height, s.info.ncomp, s.info.hsamp, s.info.vsamp, s.info.supported);
            return RN_E_INVALID;
        }
        if (!s.d_bgr || (need_coeffs && !s.coeffs)) {
            rn_set_error("%s: image %d has no %s", who, i, s.d_bgr ? "coefficient buffer" : "device image");
            return RN_E_INVALID;
        }
        if (s.n_overlays < 0 || s.n_overlays > RN_JPEG_MAX_OVERLAYS || (s.n_overlays > 0 && !s.overlays)) {
            rn_set_error("%s: image %d: %d overlays (0..%d)", who, i, s.n_overlays, RN_JPEG_MAX_OVERLAYS);
            return RN_E_INVALID;
        }
        for (int k = 0; k < s.n_overlays; ++k) {
            const rn_jpeg_overlay& o = s.overlays[k];
            if (!o.coverage || o.w < 1 || o.h < 1 || o.x < 0 || o.y < 0 || o.x > s.info.width - o.w || o.y > s.info.height - o.h) {
                rn_set_error("%s: image %d, overlay %d: box %dx%d at (%d, %d) is empty, not inside the %dx%d image, or has no coverage",
                             who, i, k, o.w, o.h, o.x, o.y, s.info.width, s.info.height);
                return RN_E_INVALID;
            }
        }
    }
    return RN_OK;
}

// The overlays in order, then (encode) the two pixel-stage launches.  d_coef null: the coefficients go down to srcs[i].coeffs
// (rn_jpeg_encode_batch_device); else they stay in the handle's scratch and d_coef[i] is where image i's are
// (rn_jpeg_encode_files_device: the Huffman phases of rn_jpeg_huffenc.hip read them there).
int enqueue(rn_handle* h, EncState* st, const rn_jpeg_source* srcs, int n, bool encode, int16_t** d_coef) {
    int rc, set;
    if ((rc = st->turn.acquire(&set)) != RN_OK) return rc;
    EncSet& sl = st->set[set];
    size_t cov_total = 0, plane_total = 0;
    int ranks = 0, max_ow = 0, max_oh = 0, max_blocks = 0, max_cw = 0, max_ch = 0;
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_source& s = srcs[i];
        for (int k = 0; k < s.n_overlays; ++k) {
            cov_total += static_cast<size_t>(s.overlays[k].w) * s.overlays[k].h;
            max_ow = std::max(max_ow, s.overlays[k].w);
            max_oh = std::max(max_oh, s.overlays[k].h);
        }
        ranks = std::max(ranks, s.n_overlays);
        plane_total += rn_jpeg::coeff_count(s.info);
        max_blocks = std::max(max_blocks, s.info.blocks_w[0] * s.info.blocks_h[0]);      // <= 8192 * 8192
        max_cw = std::max(max_cw, s.info.blocks_w[1] * 8);
        max_ch = std::max(max_ch, s.info.blocks_h[1] * 8);
    }
    if ((rc = sl.cov.grow(cov_total)) != RN_OK) return rc;
    if (encode) {
        if ((rc = rn_grow_scratch(h, &st->d_planes, &st->planes_cap, plane_total, "JPEG encode planes")) != RN_OK) return rc;
        if ((rc = rn_grow_scratch(h, &st->d_coef, &st->coef_cap, plane_total, "JPEG encode coefficients")) != RN_OK) return rc;
    }
    const size_t nb = static_cast<size_t>(h->max_batch);
    size_t cov_off = 0, off = 0;
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_source& s = srcs[i];
        for (int k = 0; k < ranks; ++k) {
            OverlayDev& o = sl.ov.host[k * nb + i];
            std::memset(&o, 0, sizeof(o));
            if (k >= s.n_overlays) continue;
            const rn_jpeg_overlay& src = s.overlays[k];
            const size_t count = static_cast<size_t>(src.w) * src.h;
            std::memcpy(sl.cov.host + cov_off, src.coverage, count * sizeof(float));
            o.bgr = s.d_bgr;
            o.cov = sl.cov.dev + cov_off;
            o.x = src.x;
            o.y = src.y;
            o.w = src.w;
            o.h = src.h;
            o.stride = s.info.width;
            for (int c = 0; c < 3; ++c) o.col[c] = static_cast<float>(src.color_bgr[c]);
            cov_off += count;
        }
        if (!encode) continue;
        EncDev& d = sl.desc.host[i];
        std::memset(&d, 0, sizeof(d));
        d.bgr = s.d_bgr;
        d.width = s.info.width;
        d.height = s.info.height;
        for (int c = 0; c < 3; ++c) {
            d.plane[c] = st->d_planes + off;
            d.coef[c] = st->d_coef + off;
            d.bw[c] = s.info.blocks_w[c];
            d.bh[c] = s.info.blocks_h[c];
            off += static_cast<size_t>(d.bw[c]) * d.bh[c] * 64;
        }
        for (int t = 0; t < 2; ++t)
            for (int k = 0; k < 64; ++k) {
                const uint32_t q8 = 8u * s.info.qt[t][k];
                d.q[t][k] = s.info.qt[t][k];
                d.recip[t][k] = static_cast<uint32_t>(((1ull << 32) + q8 - 1) / q8);
            }
    }
    if (cov_total && (rc = sl.cov.upload(cov_total, h->stream)) != RN_OK) return rc;
    if (ranks && (rc = sl.ov.upload(ranks * nb, h->stream)) != RN_OK) return rc;
    if (encode) {
        if ((rc = sl.desc.upload(static_cast<size_t>(n), h->stream)) != RN_OK) return rc;
        if ((rc = st->timer.start(h->stream)) != RN_OK) return rc;
    }
    (void)hipGetLastError();
    for (int k = 0; k < ranks; ++k) {
        hipLaunchKernelGGL(jpeg_overlay_kernel, dim3((max_ow + 63) / 64, (max_oh + 3) / 4, n), dim3(256), 0, h->stream, sl.ov.dev + k * nb);
        RN_CHECK_LAUNCH();
    }
    if (encode) {
        hipLaunchKernelGGL(jpeg_ycc_kernel, dim3((max_cw / 2 + 63) / 64, max_ch / 4, n), dim3(256), 0, h->stream, sl.desc.dev);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((max_blocks + kBlocksPerWg - 1) / kBlocksPerWg, 3, n), dim3(256), 0, h->stream, sl.desc.dev);
        RN_CHECK_LAUNCH();
        if ((rc = st->timer.stop(h->stream)) != RN_OK) return rc;
    }
    if (encode && d_coef) {
        for (int i = 0; i < n; ++i) d_coef[i] = sl.desc.host[i].coef[0];
    } else if (encode) {
        // the coefficients go down on the copy stream; the handle's stream continues behind the download, so rn_sync covers it
        // and the next call's launches do not overwrite the scratch under it
        RN_HIP(hipEventRecord(st->encoded, h->stream));
        RN_HIP(hipStreamWaitEvent(h->copy_stream, st->encoded, 0));
        for (int i = 0; i < n; ++i)
            RN_HIP(hipMemcpyAsync(srcs[i].coeffs, sl.desc.host[i].coef[0], rn_jpeg::coeff_count(srcs[i].info) * sizeof(int16_t),
                                  hipMemcpyDeviceToHost, h->copy_stream));
        RN_HIP(hipEventRecord(st->downloaded, h->copy_stream));
        RN_HIP(hipStreamWaitEvent(h->stream, st->downloaded, 0));
    }
    return st->turn.retire(h->stream);
}

int run(const char* who, rn_handle* h, const rn_jpeg_source* srcs, int n, bool encode) {
    int rc = check_sources(who, h, srcs, n, encode);
    if (rc != RN_OK) return rc;
    DeviceGuard guard(h->device);
    EncState* st = nullptr;
    if ((rc = enc_state(h, &st)) != RN_OK) return rc;
    return enqueue(h, st, srcs, n, encode, nullptr);
}

}  // namespace

int rn_jpeg_enc_check(const char* who, rn_handle* h, const rn_jpeg_source* srcs, int n) { return check_sources(who, h, srcs, n, false); }

int rn_jpeg_enc_pixels(rn_handle* h, const rn_jpeg_source* srcs, int n, int16_t** d_coef) {
    DeviceGuard guard(h->device);
    EncState* st = nullptr;
    const int rc = enc_state(h, &st);
    return rc != RN_OK ? rc : enqueue(h, st, srcs, n, true, d_coef);
}

void rn_jpeg_enc_release(rn_handle* h) {
    EncState* s = static_cast<EncState*>(h->jpeg_enc);
    if (!s) return;
    if (s->d_planes) (void)hipFree(s->d_planes);
    if (s->d_coef) (void)hipFree(s->d_coef);
    for (hipEvent_t e : {s->encoded, s->downloaded})
        if (e) (void)hipEventDestroy(e);
    delete s;                          // (the tables, their rotation and the timer free themselves)
    h->jpeg_enc = nullptr;
}

extern "C" int rn_jpeg_encode_info(int width, int height, int quality, rn_jpeg_info* out) {
    const int rc = rn_jpeg::encode_info(width, height, quality, out);
    if (rc != RN_OK) rn_set_error("rn_jpeg_encode_info: %dx%d at quality %d (sizes 1..65535, quality 1..100)", width, height, quality);
    return rc;
}

extern "C" size_t rn_jpeg_encoded_bound(const rn_jpeg_info* info) {
    if (!info || !rn_jpeg::encode_info_ok(*info)) return 0;
    return rn_jpeg::encoded_bound(*info);
}

extern "C" int rn_jpeg_entropy_encode(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len) {
    const char* why = "";
    const int rc = rn_jpeg::entropy_encode(info, coeffs, out, cap, len, &why);
    if (rc != RN_OK) rn_set_error("rn_jpeg_entropy_encode: %s", why);
    return rc;
}

extern "C" int rn_jpeg_overlay_batch_device(rn_handle* h, const rn_jpeg_source* srcs, int n) {
    return run("rn_jpeg_overlay_batch_device", h, srcs, n, false);
}

extern "C" int rn_jpeg_encode_batch_device(rn_handle* h, const rn_jpeg_source* srcs, int n) {
    return run("rn_jpeg_encode_batch_device", h, srcs, n, true);
}

extern "C" int rn_jpeg_last_encode_ms(rn_handle* h, float* ms) {
    const EncState* st = h ? static_cast<const EncState*>(h->jpeg_enc) : nullptr;
    return rn_timer::read("rn_jpeg_last_encode_ms", h, st ? &st->timer : nullptr, "no batch has been encoded on this handle",
                          h ? h->device : 0, ms);
}
