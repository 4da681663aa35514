// Occlusion-sensitivity maps: how far the class probability falls when a square of the network's input is
// covered.  Forward passes only -- the handle's own rn_forward_u8_device -- and four small kernels around them.  The definition,
// which roomnet_amd/occlusion.py restates in NumPy:
//   side S, patch P, stride T, 1 <= T <= P <= S.  Per axis G = ceil((S - P) / T) + 1 window positions p_k = min(k T, S - P): the
//   last window is flush with the edge.  Window w = ky G + kx covers rows p_ky .. p_ky + P - 1 and columns p_kx .. p_kx + P - 1 of the
//   S x S x 3 uint8 BGR input and is filled with a given BGR triple or with the image's own mean, per channel
//   (2 sum + S S) / (2 S S) in integers (the rounded mean, half up).
//   Pass 0 is the forward pass of the n images: probs / ids are rn_forward_u8_device's bits; the class c_i is class_ids[i], or
//   ids[i] of pass 0, read on the device.  The n G G (image, window) pairs, flattened as i G G + w, are cut into chunks of max_batch
//   (the last one shorter; chunks cross image boundaries); per chunk one mask launch, the forward pass, one score launch:
//   drop[i, ky, kx] = p0[i, c_i] - p_w[i, c_i], one float32 subtraction.
//   map[i, y, x] = (the float32 sum of drop[i, ky, kx] over the windows that cover (y, x), ky ascending, then kx ascending)
//   / float(their count): additions and one division, a gather with one thread per pixel; negative entries are kept.
//
//   occlusion_mean_kernel   one workgroup per image: uint32 partial sums per channel and thread (255 S S < 2^32 up to S = 4103),
//                           folded over the wave, then over the workgroup's four waves through LDS.  An integer sum: any order.
//                           A dword per lane where every image starts on a dword (3 S S a multiple of 4), else a byte per lane;
//                           a byte's channel is its offset modulo 3.
//   occlusion_mask_kernel   copy with replace.  Dword path (3 S a multiple of 4, both buffers dword-aligned: every row of every
//                           image starts on a dword): one dword per lane, 256 contiguous bytes per wave and instruction, each of
//                           its 4 bytes replaced on its own -- a window edge falls in the middle of a dword whenever 3 p_k or 3 P
//                           is no multiple of 4.  Byte path (odd sides: rows and images start at any byte): one byte per lane.
//   occlusion_score_kernel  one thread per masked image of the chunk.
//   occlusion_map_kernel    one thread per pixel; the window positions are recomputed from k, T, S, P.
// Every kernel parameter is passed by value.
#include "rn_masked_chunk.h"

#pragma clang fp contract(off)

namespace {

constexpr int64_t kMaxWindows = 1 << 20;          // n G G of one call

__device__ __host__ inline int window_pos(int k, int T, int S, int P) { return k * T < S - P ? k * T : S - P; }

// byte `b` of the image (value v) into its channel's sum: channel b % 3 (selects, so that the sums stay in registers)
__device__ inline void mean_add(uint32_t (&sum)[3], int ch, uint32_t v) {
    sum[0] += ch == 0 ? v : 0u;
    sum[1] += ch == 1 ? v : 0u;
    sum[2] += ch == 2 ? v : 0u;
}

// DWORDS: the image's 3 S S bytes are a whole number of dwords and the batch is dword-aligned, so every image starts on a dword:
// one dword per lane and step, 256 contiguous bytes per wave instruction, as the mask kernel's dword path reads.  Otherwise one
// byte per lane, consecutive lanes at consecutive bytes.
template <bool DWORDS>
__global__ __launch_bounds__(256) void occlusion_mean_kernel(const uint8_t* __restrict__ bgr, int S, uint8_t* __restrict__ fill) {
    __shared__ uint32_t s_part[4][3];
    const int npix = S * S, im_bytes = 3 * npix;
    const uint8_t* im = bgr + static_cast<int64_t>(blockIdx.x) * im_bytes;
    uint32_t sum[3] = {0, 0, 0};
    if constexpr (DWORDS) {
        const uint32_t* im32 = reinterpret_cast<const uint32_t*>(im);
        for (int t = threadIdx.x; t < im_bytes / 4; t += 256) {
            const uint32_t v = im32[t];
            const int c0 = (4 * t) % 3;
#pragma unroll
            for (int k = 0; k < 4; ++k) mean_add(sum, (c0 + k) % 3, (v >> (8 * k)) & 0xFFu);
        }
    } else {
        for (int b = threadIdx.x; b < im_bytes; b += 256) mean_add(sum, b % 3, im[b]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum[c] += __shfl_xor(sum[c], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; ++c) s_part[threadIdx.x >> 6][c] = sum[c];
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint64_t total = static_cast<uint64_t>(s_part[0][threadIdx.x]) + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] +
                               s_part[3][threadIdx.x];
        const uint64_t area = static_cast<uint64_t>(npix);
        fill[blockIdx.x * 3 + threadIdx.x] = static_cast<uint8_t>((2 * total + area) / (2 * area));
    }
}

struct MaskArgs {
    const uint8_t* src;          // [n, S, S, 3]
    uint8_t* out;                // [count, S, S, 3]
    const uint8_t* fills;        // [n, 3] per-image fills, or null: `fill`
    uint32_t fill;               // B | G << 8 | R << 16
    int32_t S, P, T, G;
    int32_t first;               // flattened index of the chunk's first (image, window) pair
};

// the masked image blockIdx.y of the chunk: its source image, its window's first row and column, its fill
__device__ inline void mask_item(const MaskArgs& a, int* image, int* y0, int* x0, uint32_t* fill) {
    const int f = a.first + static_cast<int>(blockIdx.y), gg = a.G * a.G;
    const int i = f / gg, w = f - i * gg;
    *image = i;
    *y0 = window_pos(w / a.G, a.T, a.S, a.P);
    *x0 = window_pos(w % a.G, a.T, a.S, a.P);
    *fill = a.fills ? (a.fills[3 * i] | (static_cast<uint32_t>(a.fills[3 * i + 1]) << 8) | (static_cast<uint32_t>(a.fills[3 * i + 2]) << 16))
                    : a.fill;
}

template <bool DWORDS>
__global__ __launch_bounds__(256) void occlusion_mask_kernel(MaskArgs a) {
    int image, y0, x0;
    uint32_t fill;
    mask_item(a, &image, &y0, &x0, &fill);
    const int row_bytes = 3 * a.S;
    const int64_t im_bytes = static_cast<int64_t>(row_bytes) * a.S;
    const uint8_t* src = a.src + image * im_bytes;
    uint8_t* out = a.out + blockIdx.y * im_bytes;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if constexpr (DWORDS) {
        // (3 S is a multiple of 4: a dword lies inside one row)
        if (t * 4 >= im_bytes) return;
        const int y = static_cast<int>(t * 4 / row_bytes), b0 = static_cast<int>(t * 4 - static_cast<int64_t>(y) * row_bytes);
        uint32_t v = reinterpret_cast<const uint32_t*>(src)[t];
        if (y >= y0 && y < y0 + a.P) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (b0 + k) / 3, c = (b0 + k) - 3 * x;
                if (x >= x0 && x < x0 + a.P) v = (v & ~(0xFFu << (8 * k))) | (((fill >> (8 * c)) & 0xFFu) << (8 * k));
            }
        }
        reinterpret_cast<uint32_t*>(out)[t] = v;
    } else {
        if (t >= im_bytes) return;
        const int y = static_cast<int>(t / row_bytes), b = static_cast<int>(t - static_cast<int64_t>(y) * row_bytes);
        const int x = b / 3, c = b - 3 * x;
        const bool inside = y >= y0 && y < y0 + a.P && x >= x0 && x < x0 + a.P;
        out[t] = inside ? static_cast<uint8_t>(fill >> (8 * c)) : src[t];
    }
}

// drop[first + e] = p0[i, c_i] - p_w[e, c_i] for the chunk's masked images e = 0 .. count - 1
__global__ __launch_bounds__(64) void occlusion_score_kernel(const float* __restrict__ p0, const int64_t* __restrict__ ids0,
                                                             const int32_t* __restrict__ cls, const float* __restrict__ pw, int nc,
                                                             int gg, int first, int count, float* __restrict__ drop) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= count) return;
    const int f = first + e, i = f / gg;
    const int c = cls ? cls[i] : static_cast<int>(ids0[i]);
    drop[f] = p0[i * nc + c] - pw[e * nc + c];
}

__global__ __launch_bounds__(256) void occlusion_map_kernel(const float* __restrict__ drop, int S, int P, int T, int G,
                                                            float* __restrict__ map) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= S || y >= S) return;
    const float* d = drop + static_cast<int64_t>(blockIdx.z) * G * G;
    float sum = 0.0f;
    int count = 0;
    for (int ky = 0; ky < G; ++ky) {
        const int py = window_pos(ky, T, S, P);
        if (y < py || y >= py + P) continue;
        for (int kx = 0; kx < G; ++kx) {
            const int px = window_pos(kx, T, S, P);
            if (x < px || x >= px + P) continue;
            sum = sum + d[ky * G + kx];
            ++count;
        }
    }
    map[(static_cast<int64_t>(blockIdx.z) * S + y) * S + x] = sum / static_cast<float>(count);      // (T <= P: count >= 1)
}

using OccState = rn_masked_chunk;      // (rn_masked_chunk.h: rn_faith.hip runs its masked passes through the same workspace)

struct OccPlan {
    int G, n_windows, n_chunks;
};

int check_plan(const char* who, const rn_handle* h, int n, int patch, int stride, OccPlan* p) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    const int rc = rn_occlusion_plan(h->im_side, patch, stride, n, h->max_batch, &p->G, &p->n_windows, &p->n_chunks);
    if (rc != RN_OK) {
        const std::string why = rn_last_error();
        rn_set_error("%s: %s", who, why.c_str());
    }
    return rc;
}

// The one mask enqueuer: the masked images of the flattened pairs [first, first + count) into d_out.  `mean`: the fills are
// st->d_fill (enqueue_mean ran on this stream), otherwise `fill`.
int enqueue_masks(rn_handle* h, const OccState* st, const uint8_t* d_bgr, int patch, int stride, int G, bool mean, const uint8_t* fill,
                  int first, int count, uint8_t* d_out) {
    MaskArgs a;
    a.src = d_bgr;
    a.out = d_out;
    a.fills = mean ? st->d_fill : nullptr;
    a.fill = mean ? 0u : (fill[0] | (static_cast<uint32_t>(fill[1]) << 8) | (static_cast<uint32_t>(fill[2]) << 16));
    a.S = h->im_side;
    a.P = patch;
    a.T = stride;
    a.G = G;
    a.first = first;
    const int64_t im_bytes = static_cast<int64_t>(a.S) * a.S * 3;
    const bool dwords = (3 * a.S) % 4 == 0 && (reinterpret_cast<uintptr_t>(d_bgr) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0;
    (void)hipGetLastError();
    if (dwords)
        hipLaunchKernelGGL(occlusion_mask_kernel<true>, dim3(static_cast<unsigned>((im_bytes / 4 + 255) / 256), count), dim3(256), 0,
                           h->stream, a);
    else
        hipLaunchKernelGGL(occlusion_mask_kernel<false>, dim3(static_cast<unsigned>((im_bytes + 255) / 256), count), dim3(256), 0,
                           h->stream, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// pass 0, the masked passes and the map; every argument is checked
int enqueue_all(rn_handle* h, OccState* st, const OccPlan& plan, const uint8_t* d_bgr, int n, const int32_t* d_cls, int patch, int stride,
                const uint8_t* fill, float* d_drop, float* d_map, float* d_probs, int64_t* d_ids) {
    int rc;
    // (start() marks the interval as not timed and only stop() marks it timed: a call that fails in between leaves
    //  rn_occlusion_last_ms answering RN_E_STATE, never a half-recorded interval)
    if ((rc = st->timer.start(h->stream)) != RN_OK) return rc;
    if ((rc = rn_forward_u8_device(h, d_bgr, n, d_probs, d_ids)) != RN_OK) return rc;
    if (!fill && (rc = rn_masked_enqueue_mean(h, st, d_bgr, n)) != RN_OK) return rc;
    const int gg = plan.G * plan.G;
    rc = rn_masked_passes(
        h, st, plan.n_windows,
        [&](int first, int count) { return enqueue_masks(h, st, d_bgr, patch, stride, plan.G, !fill, fill, first, count, st->d_masked); },
        [&](int first, int count) {
            (void)hipGetLastError();
            hipLaunchKernelGGL(occlusion_score_kernel, dim3((count + 63) / 64), dim3(64), 0, h->stream, d_probs, d_ids, d_cls, st->d_probs,
                               h->num_classes, gg, first, count, d_drop);
            RN_CHECK_LAUNCH();
            return RN_OK;
        });
    if (rc != RN_OK) return rc;
    if (d_map) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(occlusion_map_kernel, dim3((h->im_side + 63) / 64, (h->im_side + 3) / 4, n), dim3(256), 0, h->stream, d_drop,
                           h->im_side, patch, stride, plan.G, d_map);
        RN_CHECK_LAUNCH();
    }
    return st->timer.stop(h->stream);
}

}  // namespace

// ---- what rn_faith.hip shares (rn_masked_chunk.h)
int rn_masked_chunk_get(rn_handle* h, rn_masked_chunk** out) {
    if (!h->occlusion) {
        OccState* s = new OccState();
        h->occlusion = s;              // (rn_occlusion_release frees whatever of it exists)
        const size_t nb = static_cast<size_t>(h->max_batch), px = static_cast<size_t>(h->im_side) * h->im_side;
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_masked), nb * px * 3));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_probs), nb * h->num_classes * sizeof(float)));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_ids), nb * sizeof(int64_t)));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_fill), nb * 3));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_cls), nb * sizeof(int32_t)));
        int rc;
        if ((rc = s->timer.create()) != RN_OK) return rc;
        s->ready = true;
    }
    *out = static_cast<OccState*>(h->occlusion);
    if (!(*out)->ready) {
        rn_set_error("rn_occlusion: the workspace could not be allocated earlier");
        return RN_E_STATE;
    }
    return RN_OK;
}

int rn_masked_check_classes(const char* who, const rn_handle* h, const int32_t* cls, int n) {
    for (int i = 0; i < n; ++i)
        if (cls[i] < 0 || cls[i] >= h->num_classes) {
            rn_set_error("%s: class_ids[%d] = %d outside [0, %d)", who, i, cls[i], h->num_classes);
            return RN_E_INVALID;
        }
    return RN_OK;
}

int rn_masked_check_classes_device(const char* who, rn_handle* h, const int32_t* d_cls, int n) {
    std::vector<int32_t> cls(static_cast<size_t>(n));
    RN_HIP(hipMemcpyAsync(cls.data(), d_cls, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return rn_masked_check_classes(who, h, cls.data(), n);
}

// the per-image fills of a call without a triple -> st->d_fill
int rn_masked_enqueue_mean(rn_handle* h, rn_masked_chunk* st, const uint8_t* d_bgr, int n) {
    const bool dwords = (3 * h->im_side * h->im_side) % 4 == 0 && (reinterpret_cast<uintptr_t>(d_bgr) & 3) == 0;
    (void)hipGetLastError();
    if (dwords)
        hipLaunchKernelGGL(occlusion_mean_kernel<true>, dim3(n), dim3(256), 0, h->stream, d_bgr, h->im_side, st->d_fill);
    else
        hipLaunchKernelGGL(occlusion_mean_kernel<false>, dim3(n), dim3(256), 0, h->stream, d_bgr, h->im_side, st->d_fill);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

void rn_occlusion_release(rn_handle* h) {
    OccState* s = static_cast<OccState*>(h->occlusion);
    if (!s) return;
    for (void* p : {static_cast<void*>(s->d_masked), static_cast<void*>(s->d_probs), static_cast<void*>(s->d_ids),
                    static_cast<void*>(s->d_fill), static_cast<void*>(s->d_cls), static_cast<void*>(s->d_map),
                    static_cast<void*>(s->d_drop)})
        if (p) (void)hipFree(p);
    delete s;                          // (the timer frees itself)
    h->occlusion = nullptr;
}

extern "C" int rn_occlusion_plan(int side, int patch, int stride, int n, int max_batch, int* G, int* n_windows, int* n_chunks) {
    if (side < 1 || patch < 1 || stride < 1 || n < 1 || max_batch < 1) {
        rn_set_error("rn_occlusion_plan: side %d, patch %d, stride %d, n %d, max_batch %d: every value must be at least 1", side, patch,
                     stride, n, max_batch);
        return RN_E_INVALID;
    }
    if (stride > patch || patch > side) {
        rn_set_error("rn_occlusion_plan: 1 <= stride <= patch <= side does not hold for stride %d, patch %d, side %d", stride, patch, side);
        return RN_E_INVALID;
    }
    if (n > max_batch) {
        rn_set_error("rn_occlusion_plan: n = %d out of range (1..%d)", n, max_batch);
        return RN_E_RANGE;
    }
    const int64_t g = (side - patch + stride - 1) / stride + 1;
    const int64_t total = static_cast<int64_t>(n) * g * g;
    if (total > kMaxWindows) {
        rn_set_error("rn_occlusion_plan: %d images x %lld x %lld windows = %lld masked passes, more than %lld", n, static_cast<long long>(g),
                     static_cast<long long>(g), static_cast<long long>(total), static_cast<long long>(kMaxWindows));
        return RN_E_RANGE;
    }
    if (G) *G = static_cast<int>(g);
    if (n_windows) *n_windows = static_cast<int>(total);
    if (n_chunks) *n_chunks = static_cast<int>((total + max_batch - 1) / max_batch);
    return RN_OK;
}

extern "C" int rn_occlusion_masks_device(rn_handle* h, const uint8_t* d_bgr, int n, int patch, int stride, const uint8_t* fill_bgr, int first,
                                         int count, uint8_t* d_out) {
    const char* who = "rn_occlusion_masks_device";
    OccPlan plan;
    int rc = check_plan(who, h, n, patch, stride, &plan);
    if (rc != RN_OK) return rc;
    if (!d_bgr || !d_out) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    if (count < 1 || count > h->max_batch) {
        rn_set_error("%s: count = %d out of range (1..%d)", who, count, h->max_batch);
        return RN_E_RANGE;
    }
    if (first < 0 || first > plan.n_windows - count) {
        rn_set_error("%s: [%d, %d + %d) is not inside the call's %d masked images", who, first, first, count, plan.n_windows);
        return RN_E_RANGE;
    }
    DeviceGuard guard(h->device);
    OccState* st = nullptr;
    if ((rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    if (!fill_bgr && (rc = rn_masked_enqueue_mean(h, st, d_bgr, n)) != RN_OK) return rc;
    return enqueue_masks(h, st, d_bgr, patch, stride, plan.G, !fill_bgr, fill_bgr, first, count, d_out);
}

extern "C" int rn_occlusion_u8_device(rn_handle* h, const uint8_t* d_bgr, int n, const int32_t* d_class_ids, int patch, int stride,
                                      const uint8_t* fill_bgr, float* d_drop, float* d_map, float* d_probs, int64_t* d_ids) {
    const char* who = "rn_occlusion_u8_device";
    OccPlan plan;
    int rc = check_plan(who, h, n, patch, stride, &plan);
    if (rc != RN_OK) return rc;
    if (!d_bgr || !d_drop || !d_probs || !d_ids) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    // (validated before anything is launched: the classes are read back on the handle's stream)
    if (d_class_ids && (rc = rn_masked_check_classes_device(who, h, d_class_ids, n)) != RN_OK) return rc;
    OccState* st = nullptr;
    if ((rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    return enqueue_all(h, st, plan, d_bgr, n, d_class_ids, patch, stride, fill_bgr, d_drop, d_map, d_probs, d_ids);
}

extern "C" int rn_occlusion_u8(rn_handle* h, const uint8_t* bgr, int n, const int32_t* class_ids, int patch, int stride,
                               const uint8_t* fill_bgr, float* drop, float* map, float* probs, int64_t* ids) {
    const char* who = "rn_occlusion_u8";
    OccPlan plan;
    int rc = check_plan(who, h, n, patch, stride, &plan);
    if (rc != RN_OK) return rc;
    if (!bgr || !drop || !probs || !ids) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    if (class_ids && (rc = rn_masked_check_classes(who, h, class_ids, n)) != RN_OK) return rc;
    DeviceGuard guard(h->device);
    OccState* st = nullptr;
    if ((rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    const size_t px = static_cast<size_t>(h->im_side) * h->im_side;
    if ((rc = rn_grow_scratch(h, &st->d_drop, &st->drop_cap, static_cast<size_t>(plan.n_windows), "occlusion drops")) != RN_OK) return rc;
    if (map && !st->d_map) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_map), static_cast<size_t>(h->max_batch) * px * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            st->d_map = nullptr;
            rn_set_error("%s: hipMalloc(%zu bytes of maps) failed: %s", who, static_cast<size_t>(h->max_batch) * px * sizeof(float),
                         hipGetErrorString(e));
            return RN_E_NOMEM;
        }
    }
    RN_HIP(hipMemcpyAsync(h->d_in_u8, bgr, static_cast<size_t>(n) * px * 3, hipMemcpyHostToDevice, h->stream));
    if (class_ids) RN_HIP(hipMemcpyAsync(st->d_cls, class_ids, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_all(h, st, plan, h->d_in_u8, n, class_ids ? st->d_cls : nullptr, patch, stride, fill_bgr, st->d_drop, map ? st->d_map : nullptr,
                     h->d_probs, h->d_ids);
    if (rc != RN_OK) return rc;
    RN_HIP(hipMemcpyAsync(drop, st->d_drop, static_cast<size_t>(plan.n_windows) * 4, hipMemcpyDeviceToHost, h->stream));
    if (map) RN_HIP(hipMemcpyAsync(map, st->d_map, static_cast<size_t>(n) * px * 4, hipMemcpyDeviceToHost, h->stream));
    return rn_results_to_host(h, n, probs, ids);
}

extern "C" int rn_occlusion_last_ms(rn_handle* h, float* ms) {
    const OccState* st = h ? static_cast<const OccState*>(h->occlusion) : nullptr;
    return rn_timer::read("rn_occlusion_last_ms", h, st && st->ready ? &st->timer : nullptr,
                          "no occlusion call has enqueued all its launches on this handle", h ? h->device : 0, ms);
}
