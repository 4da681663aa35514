// Grad-CAM heat maps drawn into BGR uint8 HWC images that are in device memory: roomnet_amd/cam.py's
// overlay_image -- bilinear upsampling of a small float32 map to the photograph's centre-crop window, normalisation by the
// upsampled map's maximum, the colour ramp, the blend -- byte for byte, in float64 without contraction (rn_cam_math.h, whose
// `fp contract(off)` holds for this whole file).
//   cam_max_kernel    one window pixel per lane and row step, 64 columns x 16 rows per workgroup: the maximum of the upsampled,
//                     clamped values, folded over the wave, the workgroup and then, with one integer atomic max per workgroup on
//                     the bits of the non-negative double, the image.  A maximum is the same in every order.
//   cam_blend_kernel  4 pixels of a window row per lane: the upsampled value again (the same operations: the same bits), its
//                     colour, the blend, BGR stored in place.  A window row starts at any byte (pixels are 3 bytes, the window's
//                     offset is arbitrary), so the groups of 4 pixels are laid out from the row's first dword-aligned pixel: a
//                     whole group is read and stored as three dwords, the partial groups at the row's two ends byte by byte.
// Both are ONE launch per batch (blockIdx.z = image, a device table of per-image descriptors), as in rn_jpeg.hip and
// rn_jpeg_enc.hip.  3 B read and 3 B written per window pixel, about 60 float64 operations and one division per pixel in each launch.
#include "rn_internal.h"
#include "rn_cam_math.h"

#include <algorithm>

namespace {

struct CamDev {
    uint8_t* bgr;                   // the window's first pixel
    const float* cam;               // [mh][mw]
    unsigned long long* mx;         // bits of the image's maximum (zeroed in front of cam_max_kernel)
    int64_t row_bytes;              // the image's width * 3
    int32_t side, mh, mw;
    double sy, sx;                  // mh / double(side), mw / double(side)
};

constexpr int kMaxRows = 16;        // window rows per workgroup of cam_max_kernel (4 per lane)

__global__ __launch_bounds__(256) void cam_max_kernel(const CamDev* __restrict__ table) {
    const CamDev& d = table[blockIdx.z];
    if (static_cast<int>(blockIdx.x) * 64 >= d.side || static_cast<int>(blockIdx.y) * kMaxRows >= d.side) return;      // (uniform per workgroup: in front of the barrier)
    __shared__ double s_part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    double m = 0.0;
    if (x < d.side) {
        const rn_cam_axis xa = rn_cam_axis_of(x, d.mw, d.sx);
#pragma unroll
        for (int r = 0; r < kMaxRows / 4; ++r) {
            const int y = blockIdx.y * kMaxRows + r * 4 + wave;
            if (y < d.side) m = fmax(m, rn_cam_up(d.cam, d.mw, rn_cam_axis_of(y, d.mh, d.sy), xa));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if (lane == 0) s_part[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(s_part[0], s_part[1]), fmax(s_part[2], s_part[3]));
        // (non-negative doubles order like their bits; 0 needs no atomic)
        if (m > 0.0) atomicMax(d.mx, static_cast<unsigned long long>(__double_as_longlong(m)));
    }
}

__global__ __launch_bounds__(256) void cam_blend_kernel(const CamDev* __restrict__ table, double weight, double omw) {
    const CamDev& d = table[blockIdx.z];
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= d.side) return;
    uint8_t* row = d.bgr + y * d.row_bytes;
    // pixel p of the row is at row + 3 p: dword-aligned where p = row (mod 4).  Group g holds pixels lead + 4 (g - 1) .. + 3.
    const int lead = static_cast<int>(reinterpret_cast<uintptr_t>(row) & 3);
    const int x4 = lead + 4 * (static_cast<int>(blockIdx.x * 64 + (threadIdx.x & 63)) - 1);
    if (x4 >= d.side || x4 + 3 < 0) return;
    const bool whole = x4 >= 0 && x4 + 3 < d.side;
    const rn_cam_axis ya = rn_cam_axis_of(y, d.mh, d.sy);
    const double mx = __longlong_as_double(static_cast<long long>(*d.mx));
    uint8_t* p = row + static_cast<int64_t>(x4) * 3;      // (only dereferenced for pixels inside the row)
    uint32_t in[3] = {0, 0, 0};
    if (whole) {
        const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
        in[0] = p32[0];
        in[1] = p32[1];
        in[2] = p32[2];
    } else {
        for (int k = 0; k < 12; ++k)
            if (x4 + k / 3 >= 0 && x4 + k / 3 < d.side) in[k >> 2] |= static_cast<uint32_t>(p[k]) << (8 * (k & 3));
    }
    uint32_t out[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(max(x4 + k, 0), d.side - 1);       // (a pixel outside the row computes a neighbour's value and drops it)
        double heat[3];
        rn_cam_heat(rn_cam_up(d.cam, d.mw, ya, rn_cam_axis_of(x, d.mw, d.sx)), mx, heat);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int b = 3 * k + c;
            out[b >> 2] |= rn_cam_blend((in[b >> 2] >> (8 * (b & 3))) & 255u, heat[c], weight, omw) << (8 * (b & 3));
        }
    }
    if (whole) {
        uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
        p32[0] = out[0];
        p32[1] = out[1];
        p32[2] = out[2];
    } else {
        for (int k = 0; k < 12; ++k)
            if (x4 + k / 3 >= 0 && x4 + k / 3 < d.side) p[k] = static_cast<uint8_t>(out[k >> 2] >> (8 * (k & 3)));
    }
}

// The per-batch tables and maxima, two sets behind one rotation (rn_batch_table.h).
struct CamState {
    rn_table<CamDev> desc[2];                 // [max_batch]
    unsigned long long* d_max[2] = {nullptr, nullptr};      // [max_batch]
    rn_rotation turn;
    rn_timer timer;
    bool ready = false;
};

int cam_state(rn_handle* h, CamState** out) {
    if (!h->cam_overlay) {
        CamState* s = new CamState();
        h->cam_overlay = s;            // (rn_cam_overlay_release frees whatever of it exists)
        const size_t nb = static_cast<size_t>(h->max_batch);
        int rc;
        for (int k = 0; k < 2; ++k) {
            if ((rc = s->desc[k].alloc(nb)) != RN_OK) return rc;
            RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_max[k]), nb * sizeof(unsigned long long)));
        }
        if ((rc = s->turn.create()) != RN_OK || (rc = s->timer.create()) != RN_OK) return rc;
        s->ready = true;
    }
    *out = static_cast<CamState*>(h->cam_overlay);
    if (!(*out)->ready) {
        rn_set_error("rn_cam_overlay: the stage's state could not be allocated earlier");
        return RN_E_STATE;
    }
    return RN_OK;
}

int check_targets(rn_handle* h, const rn_cam_target* t, int n, double weight) {
    const char* who = "rn_cam_overlay_batch_device";
    const int rc = rn_check_batch(who, h, t, n);
    if (rc != RN_OK) return rc;
    if (!(weight >= 0.0 && weight <= 1.0)) {
        rn_set_error("%s: weight %g is not in [0, 1]", who, weight);
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i) {
        if (!t[i].d_bgr || !t[i].d_cam) {
            rn_set_error("%s: image %d has no %s", who, i, t[i].d_bgr ? "map" : "device image");
            return RN_E_INVALID;
        }
        if (t[i].height < 1 || t[i].width < 1 || t[i].height > 65535 || t[i].width > 65535 || t[i].cam_h < 1 || t[i].cam_w < 1 ||
            t[i].cam_h > 65535 || t[i].cam_w > 65535) {
            rn_set_error("%s: image %d: a %dx%d image and a %dx%d map (sizes 1..65535)", who, i, t[i].width, t[i].height, t[i].cam_w,
                         t[i].cam_h);
            return RN_E_INVALID;
        }
    }
    return RN_OK;
}

int enqueue(rn_handle* h, CamState* st, const rn_cam_target* targets, int n, double weight) {
    int rc, set;
    if ((rc = st->turn.acquire(&set)) != RN_OK) return rc;
    const rn_table<CamDev>& tab = st->desc[set];
    unsigned long long* d_max = st->d_max[set];
    int max_side = 0;
    for (int i = 0; i < n; ++i) {
        const rn_cam_target& t = targets[i];
        int x0, y0, side;
        rn_center_crop_window(t.height, t.width, &x0, &y0, &side);
        CamDev& d = tab.host[i];
        std::memset(&d, 0, sizeof(d));
        d.row_bytes = static_cast<int64_t>(t.width) * 3;
        d.bgr = t.d_bgr + y0 * d.row_bytes + static_cast<int64_t>(x0) * 3;
        d.cam = t.d_cam;
        d.mx = d_max + i;
        d.side = side;
        d.mh = t.cam_h;
        d.mw = t.cam_w;
        d.sy = t.cam_h / static_cast<double>(side);
        d.sx = t.cam_w / static_cast<double>(side);
        max_side = std::max(max_side, side);
    }
    if ((rc = tab.upload(static_cast<size_t>(n), h->stream)) != RN_OK) return rc;
    if ((rc = st->timer.start(h->stream)) != RN_OK) return rc;
    RN_HIP(hipMemsetAsync(d_max, 0, static_cast<size_t>(n) * sizeof(unsigned long long), h->stream));
    (void)hipGetLastError();
    hipLaunchKernelGGL(cam_max_kernel, dim3((max_side + 63) / 64, (max_side + kMaxRows - 1) / kMaxRows, n), dim3(256), 0, h->stream, tab.dev);
    RN_CHECK_LAUNCH();
    // (groups of 4 pixels: at most 3 pixels in front of the first aligned one, so (side + 3) / 4 + 1 groups reach the row's end)
    hipLaunchKernelGGL(cam_blend_kernel, dim3(((max_side + 3) / 4 + 1 + 63) / 64, (max_side + 3) / 4, n), dim3(256), 0, h->stream, tab.dev,
                       weight, 1.0 - weight);
    RN_CHECK_LAUNCH();
    if ((rc = st->timer.stop(h->stream)) != RN_OK) return rc;
    return st->turn.retire(h->stream);
}

}  // namespace

void rn_cam_overlay_release(rn_handle* h) {
    CamState* s = static_cast<CamState*>(h->cam_overlay);
    if (!s) return;
    for (unsigned long long* p : s->d_max)
        if (p) (void)hipFree(p);
    delete s;                          // (the tables, their rotation and the timer free themselves)
    h->cam_overlay = nullptr;
}

extern "C" int rn_cam_overlay_batch_device(rn_handle* h, const rn_cam_target* targets, int n, double weight) {
    int rc = check_targets(h, targets, n, weight);
    if (rc != RN_OK) return rc;
    DeviceGuard guard(h->device);
    CamState* st = nullptr;
    if ((rc = cam_state(h, &st)) != RN_OK) return rc;
    return enqueue(h, st, targets, n, weight);
}

extern "C" int rn_cam_last_overlay_ms(rn_handle* h, float* ms) {
    const CamState* st = h ? static_cast<const CamState*>(h->cam_overlay) : nullptr;
    return rn_timer::read("rn_cam_last_overlay_ms", h, st ? &st->timer : nullptr, "no heat map has been drawn on this handle",
                          h ? h->device : 0, ms);
}
