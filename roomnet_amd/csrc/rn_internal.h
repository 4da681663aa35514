// Internal declarations shared by the translation units of libroomnet_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "roomnet_hip.h"

#define RN_VERSION_STRING "roomnet_hip 0.1 (gfx950)"

void rn_set_error(const char* fmt, ...);

// (a failing runtime call also leaves its status in the thread's sticky "last error", which RN_CHECK_LAUNCH reads: a failure
//  that was reported here must not come back as the "launch failure" of the next, innocent kernel -- consume it)
#define RN_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            rn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,     \
                         __LINE__);                                                           \
            (void)hipGetLastError();                                                          \
            return RN_E_HIP;                                                                  \
        }                                                                                     \
    } while (0)

#define RN_CHECK_LAUNCH()                                                                     \
    do {                                                                                      \
        hipError_t _e = hipGetLastError();                                                    \
        if (_e != hipSuccess) {                                                               \
            rn_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, \
                         __LINE__);                                                           \
            return RN_E_HIP;                                                                  \
        }                                                                                     \
    } while (0)

// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised before their first launch.
// The attribute is per device: remember which devices of this process have it (one handle per GPU per process is the
// normal deployment, several handles on several GPUs / threads in one process must work too).  Kern is a template argument
// so that every kernel instantiation has a mask of its own.
template <auto Kern>
int rn_allow_big_lds() {
    static std::atomic<unsigned long long> attr_devices{0};
    int dev = 0;
    RN_HIP(hipGetDevice(&dev));
    if (!(attr_devices.load(std::memory_order_acquire) >> (dev & 63) & 1ull)) {
        RN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_devices.fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
    return RN_OK;
}
// names a kernel instantiation as a value, for launch lambdas:  launch(rn_kernel<my_kernel<RN_DTYPE_BF16>>{})
template <auto Kern>
struct rn_kernel {};
// Launches the instantiation of a 16-bit kernel for the handle's storage type (RN_DTYPE_BF16: KernBF16, otherwise KernF16) with one
// argument block.  BIG_LDS: the kernel's dynamic LDS can exceed 64 KB (rn_allow_big_lds first).
template <auto KernBF16, auto KernF16, bool BIG_LDS, class Args>
int rn_launch16(int dtype, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args& a) {
    auto launch = [&]<auto Kern>(rn_kernel<Kern>) -> int {
        if constexpr (BIG_LDS)
            if (int rc = rn_allow_big_lds<Kern>()) return rc;
        hipLaunchKernelGGL(Kern, grid, block, lds_bytes, s, a);
        RN_CHECK_LAUNCH();
        return RN_OK;
    };
    return dtype == RN_DTYPE_BF16 ? launch(rn_kernel<KernBF16>{}) : launch(rn_kernel<KernF16>{});
}

// Makes `dev` the current HIP device and puts the caller's back on scope exit; `ok` = the device could be set.  Without an
// argument it only restores (the group entry points walk several devices).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    DeviceGuard();
    explicit DeviceGuard(int dev);
    ~DeviceGuard();
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#include "rn_batch_table.h"

// per-channel affine form of an inference BN: y = (x - mean) * inv + beta
struct BnDev {
    float* mean = nullptr;   // [c]
    float* inv = nullptr;    // [c]  rsqrt(var + eps) * gamma, computed on the host in fp32
    float* beta = nullptr;   // [c]
};

struct ResizeTab {           // legacy TF-1.13 bilinear tables (host-computed, fp32)
    int32_t* lo = nullptr;   // [out]
    int32_t* hi = nullptr;   // [out]
    float* lerp = nullptr;   // [out]
};

struct StagePlan {
    int cin, cout, in_side, conv_side, pool_k, pool_s, out_side;
    int skip_stage, skip_side;
    // device weights
    float* w_f32 = nullptr;      // HWIO fp32 (unfused path and stage 0)
    void* w_frag = nullptr;      // MFMA fragment-packed 16-bit weights (fused path)
    int kchunks = 0;             // number of 16-deep K chunks in w_frag
    BnDev bn, bn2;
    ResizeTab rt;                // skip_side -> out_side
    // node ids (-1 when absent)
    int node_conv = -1, node_pool = -1, node_bn = -1, node_add = -1, node_bn2 = -1;
};

struct DensePlan {
    int nin, nout;
    float* w = nullptr;          // [nin, nout]
    float* bias = nullptr;       // [nout] or null
    float* inv = nullptr;        // BN: x*inv + shift   (null: no BN)
    float* shift = nullptr;
    int node_mm = -1, node_relu = -1, node_bn = -1;
};

// the node a stage's output lives in
inline int rn_stage_out_node(const StagePlan& s) { return s.node_bn2 >= 0 ? s.node_bn2 : s.node_bn; }

struct NodeBuf {
    rn_node_info info;
    void* ptr = nullptr;         // device buffer [max_batch, h, w, c] (null: not materialised)
    int dtype = RN_DTYPE_F32;    // storage type of ptr
};

// one image of a batched crop + resize (rn_imageops.hip): crop window at `src`, scales and mode as cv::resize computes them
struct rn_resize_item {
    const uint8_t* src;
    int src_h, src_w;
    int64_t src_row_bytes;
    double scale_x, scale_y;
    int mode;
};

// one photograph of a training set (rn_views_create; rn_views.h): what does not change from step to step.  `win` is the square
// window at offset 0 -- the whole short axis, `side` along the long one -- with the scales and the mode rn_resize_item_fill forms on
// the host: they depend on the side alone, not on the offset a step draws.
struct rn_view_item {
    rn_resize_item win;
    int32_t range;               // max(height, width) - side: the offsets a draw can take are [0, range) (0 when range is 0)
    int32_t axis;                // 0: the window slides along the columns (height < width); 1: along the rows
    int32_t centre;              // the offset of rn_center_crop_window, what a launch without RN_VIEW_CROP takes
    int32_t pad;
};

struct rn_views {
    int device = 0;
    int im_side = 0;             // the side the scales were formed for: the creating handle's
    int64_t n_items = 0;
    rn_view_item* d_items = nullptr;   // [n_items]
};

struct rn_handle {
    int device = 0;
    int dtype = RN_DTYPE_F32;
    unsigned flags = 0;
    int max_batch = 0;
    int im_side = 0, num_classes = 0;
    float bn_eps = 1e-3f;
    int n_cu = 0;                // compute units of the device (launch geometry is sized in rounds of the chip)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::vector<StagePlan> stages;
    std::vector<DensePlan> dense;
    std::vector<NodeBuf> nodes;
    int node_input = -1, node_flat = -1, node_softmax = -1;
    float* lut = nullptr;        // 256-entry uint8 -> float32 table
    // staging for host-buffer calls
    uint8_t* d_in_u8 = nullptr;
    uint8_t* d_raw = nullptr;      // staging for raw (un-resized) images, rn_classify_images_u8 (grow-only, rn_grow_scratch)
    size_t raw_cap = 0;
    rn_table<rn_resize_item> items[2];     // [max_batch] crop windows of a batched resize, two sets (rn_enqueue_resize_batch allocates them)
    rn_rotation items_turn;
    float* d_probs = nullptr;
    int64_t* d_ids = nullptr;
    // two-slot host pipeline (rn_submit_u8 / rn_collect): allocated by the first submit
    struct HostSlot {
        uint8_t* d_in = nullptr;
        float* d_probs = nullptr;
        int64_t* d_ids = nullptr;
        float* h_probs = nullptr;    // pinned
        int64_t* h_ids = nullptr;    // pinned
        hipEvent_t uploaded = nullptr, done = nullptr;
        int n = 0;
        bool busy = false;
    };
    HostSlot slots[2];
    hipStream_t copy_stream = nullptr;
    std::vector<void*> allocs;   // everything to hipFree on destroy
    void* fused = nullptr;       // plan of the fused 16-bit path (rn_fused.hip)
    void* f32m = nullptr;        // plan of the float32 matrix-core stage kernels (rn_stage_f32m.hip)
    void* gradcam = nullptr;     // what the grad-CAM adjoint keeps from rn_create + its device workspace (rn_gradcam.hip)
    float* d_feat = nullptr;     // rn_features_u8: float32 staging of s7.bn, [max_batch, S7, S7, 16] (allocated by the first call)
    float* d_feat6 = nullptr;    // rn_features_depth_u8, depth 3: float32 staging of s6.bn, [max_batch, S6, S6, 128] (the same)
    void* bnstats = nullptr;     // RN_FLAG_BATCH_STATS: the 16 BNs' gamma / moment buffers and the partials' slab (rn_bnstats.hip)
    // the image stages' lazily allocated state: single stream-ordered scratch, two sets of batch tables (rn_batch_table.h), a timer
    void* jpeg = nullptr;        // rn_jpeg_*: coefficient / plane / image scratch, the JpegDev tables (rn_jpeg.hip; allocated by the first call)
    void* jpeg_enc = nullptr;    // rn_jpeg_overlay_* / rn_jpeg_encode_*: plane / coefficient scratch, the EncDev / OverlayDev / coverage tables (rn_jpeg_enc.hip; the same)
    void* jpeg_huffenc = nullptr; // rn_jpeg_huffenc_* / rn_jpeg_encode_files_device: lengths, sums, both streams, the descriptor tables (rn_jpeg_huffenc.hip; the same)
    void* cam_overlay = nullptr; // rn_cam_overlay_*: the CamDev tables and the per-image maxima (rn_cam_overlay.hip; the same)
    void* occlusion = nullptr;   // rn_occlusion_*: the masked chunk, its probabilities and ids, the per-image fills (rn_occlusion.hip; the same)
    void* faith = nullptr;       // rn_faith_*: the ranking's (key, index) sets, which also keep a call's ranks (rn_faith.hip; the same)
    bool split_backend = false;  // 16-bit handles: this call runs the back end as its split launches (grad-CAM: s6.bn, s7.bn in HBM)
    bool features_pass = false;  // rn_features_*: this call reads s6.bn / s7.bn only; a flatten head_kernel cannot take does not fail it
    // channel relabelling of the tensors the frozen-channel folds touch, float32 (rn_f32m_prepare) and 16-bit (rn_fused_prepare) alike:
    // node id -> position p of the stored tensor holds the reference's channel perm[p] (rn_tap puts them back in order)
    std::map<int, std::vector<int>> node_perm;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> events;   // [0]=start, [1]=after preprocess, [2+i]=after stage i, last=after head
    bool timing_valid = false;
    int last_n = 0;
};

// ---- launchers (rn_kernels_f32.hip) -------------------------------------------------
int rn_launch_preprocess_u8(hipStream_t s, const uint8_t* bgr, float* rgb, const float* lut, int64_t npix);
int rn_launch_conv3x3_relu6_f32(hipStream_t s, const float* in, const float* w, float* out, int n, int h,
                                int wd, int cin, int cout);
// stage 0 (3 -> 8, pool 3/1) as one launch (float32 handles without taps): same bits as the four per-node launches
int rn_launch_stage0_fused_f32(hipStream_t s, const float* in, const float* w, float* out, int n, int side, const BnDev& bn);
int rn_launch_avgpool_f32(hipStream_t s, const float* in, float* out, int n, int h, int w, int c, int k, int st);
int rn_launch_bn_f32(hipStream_t s, const float* in, float* out, int64_t npix, int c, const BnDev& bn);
int rn_launch_resize_add_f32(hipStream_t s, const float* x, const float* skip, float* out, int n, int side,
                             int skip_side, int c, const ResizeTab& rt);
// head: flatten + dense chain + softmax + argmax.  tap pointers may be null.
struct HeadArgs {
    int n_dense;
    int nin[RN_MAX_DENSE], nout[RN_MAX_DENSE];
    const float* w[RN_MAX_DENSE];
    const float* bias[RN_MAX_DENSE];
    const float* inv[RN_MAX_DENSE];
    const float* shift[RN_MAX_DENSE];
    float* tap_mm[RN_MAX_DENSE];
    float* tap_relu[RN_MAX_DENSE];
    float* tap_bn[RN_MAX_DENSE];
};
void rn_resize_item_fill(rn_resize_item* it, const uint8_t* d_src, int src_h, int src_w, int64_t src_row_bytes, int S);
int rn_launch_resize_batch_u8(hipStream_t s, const rn_resize_item* d_items, int n, uint8_t* d_dst_base, int S);
int rn_launch_resize_u8(hipStream_t s, const uint8_t* d_src, int src_h, int src_w, int64_t src_row_bytes, uint8_t* d_dst,
                        int dst_h, int dst_w);
// the body of rn_views_batch_device behind its checks (rn_ft_run_views calls it once per step): one launch on the handle's stream
int rn_views_enqueue(rn_handle* h, const rn_views* v, const int32_t* d_index, int64_t base, int n, uint64_t seed, int64_t step,
                     unsigned flags, uint8_t* d_dst);
// its checks: null arguments, a table of another device or side (RN_E_INVALID), n outside [1, max_batch] or step < 0 (RN_E_RANGE)
int rn_views_check(const char* who, const rn_handle* h, const rn_views* v, const void* d_index, int n, int64_t step, unsigned flags,
                   const void* d_dst);
int rn_launch_head(hipStream_t s, const void* flat, int flat_dtype, int n, const HeadArgs& a, float* probs,
                   int64_t* ids);
bool rn_head_takes_flatten(int flat_len);      // head_kernel keeps the flatten in LDS: up to 4096 values (im_side <= 694)
int rn_launch_convert_to_f32(hipStream_t s, const void* in, int dtype, float* out, int64_t n);

// ---- grad-CAM (rn_gradcam.hip)
const char* rn_tail_graph_reason(const rn_weights* w);
int rn_gradcam_keep(rn_handle* h, const rn_weights* w);
void rn_gradcam_release(rn_handle* h);
void rn_gradcam_layers(const rn_handle* h, int* node6, int* node7);
const char* rn_gradcam_unsupported(const rn_handle* h);
int rn_gradcam_launch(rn_handle* h, int n, const int32_t* d_cls, const int64_t* d_ids, bool layer6, float* d_cam, float* d_alpha);
int rn_gradcam_staging(rn_handle* h, int32_t** d_cls, float** d_cam, float** d_alpha);

// ---- batch-statistics BN (rn_bnstats.hip): float32 per-node handles created with RN_FLAG_BATCH_STATS
int rn_bnstats_prepare(rn_handle* h, const rn_weights* w);     // after the plan is built: what the moments launches need
void rn_bnstats_release(rn_handle* h);
// moments of x [npix, cout] on the handle's stream -> the (mean, inv) table of stage `stage`'s first / second BN
int rn_bnstats_conv(rn_handle* h, int stage, bool second, const float* x, int64_t npix);
int rn_bnstats_head(rn_handle* h, int n, float* d_probs, int64_t* d_ids);

// ---- baseline JPEG pixel stage (rn_jpeg.hip)
void rn_jpeg_release(rn_handle* h);
// ---- overlay + the encode's pixel stage (rn_jpeg_enc.hip)
void rn_jpeg_enc_release(rn_handle* h);
// the source checks of rn_jpeg_encode_batch_device, the coefficient pointer apart (nothing is enqueued)
int rn_jpeg_enc_check(const char* who, rn_handle* h, const rn_jpeg_source* srcs, int n);
// its overlays and pixel stage without the download: d_coef[i] = image i's coefficients in the handle's scratch, valid until the
// handle's next encode call.  The sources (1 .. max_batch of them) passed rn_jpeg_enc_check.
int rn_jpeg_enc_pixels(rn_handle* h, const rn_jpeg_source* srcs, int n, int16_t** d_coef);
// ---- the Huffman pass of the output file (rn_jpeg_huffenc.hip)
void rn_jpeg_huffenc_release(rn_handle* h);
// ---- grad-CAM heat maps on resident images (rn_cam_overlay.hip)
void rn_cam_overlay_release(rn_handle* h);
// ---- occlusion-sensitivity maps (rn_occlusion.hip)
void rn_occlusion_release(rn_handle* h);
// ---- deletion / insertion curves of a heat map (rn_faith.hip; what it shares with occlusion: rn_masked_chunk.h)
void rn_faith_release(rn_handle* h);
// (rn_api.hip) the centred square window of network.py:137-146 (of a packed BGR image: its top left, side and row bytes), the tail
// of a host entry point, the null-argument (RN_E_INVALID) / n in 1..max_batch (RN_E_RANGE) check the batched image stages open with
struct rn_window {
    const uint8_t* src;
    int side;
    int64_t row_bytes;
};
void rn_center_crop_window(int hh, int ww, int* x0, int* y0, int* side);
rn_window rn_center_window(const uint8_t* src, int hh, int ww);
int rn_results_to_host(rn_handle* h, int n, float* probs, int64_t* ids);
int rn_check_batch(const char* who, const rn_handle* h, const void* ptr, int n);
// One batched crop + resize of n <= max_batch windows (device memory) into d_dst_batch [n, im_side, im_side, 3] on the handle's stream:
// acquires a set of h->items, fills it from window(0) .. window(n - 1) (asked once each, in order), uploads, launches, retires.
int rn_enqueue_resize_batch(rn_handle* h, int n, uint8_t* d_dst_batch, const std::function<rn_window(int)>& window);

// ---- host helpers (rn_api.hip) -----------------------------------------------------------
// device memory owned through a list (freed by the list's owner: rn_destroy, rn_ft_destroy); a failure is RN_E_NOMEM with
// "hipMalloc(N bytes) failed: ...".  An empty request gets `min_bytes`.
int rn_owned_alloc(std::vector<void*>& owner, size_t bytes, size_t min_bytes, void** out);
template <typename T>
int rn_owned_upload(std::vector<void*>& owner, size_t min_bytes, const T* src, size_t count, T** out) {
    void* p = nullptr;
    int rc = rn_owned_alloc(owner, count * sizeof(T), min_bytes, &p);
    if (rc != RN_OK) return rc;
    RN_HIP(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<T*>(p);
    return RN_OK;
}
template <typename T>
int rn_owned_zeroed(std::vector<void*>& owner, size_t min_bytes, size_t count, T** out) {
    void* p = nullptr;
    int rc = rn_owned_alloc(owner, count * sizeof(T), min_bytes, &p);
    if (rc != RN_OK) return rc;
    RN_HIP(hipMemset(p, 0, count * sizeof(T)));
    *out = static_cast<T*>(p);
    return RN_OK;
}
// grow-only device scratch (h->d_raw, the JPEG stages' planes and coefficients): the handle's streams are drained first, so
// nothing still reads the old block; a quarter is added to what is asked for
template <typename T>
int rn_grow_scratch(rn_handle* h, T** p, size_t* cap, size_t need, const char* what) {
    if (need <= *cap) return RN_OK;
    RN_HIP(hipStreamSynchronize(h->stream));
    if (h->copy_stream) RN_HIP(hipStreamSynchronize(h->copy_stream));
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 4;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, want * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        rn_set_error("hipMalloc(%zu bytes of %s) failed: %s", want * sizeof(T), what, hipGetErrorString(e));
        return RN_E_NOMEM;
    }
    *p = static_cast<T*>(q);
    *cap = want;
    return RN_OK;
}
// ... by the handle (an empty request gets 16 bytes)
inline int dev_alloc(rn_handle* h, size_t bytes, void** out) { return rn_owned_alloc(h->allocs, bytes, 16, out); }
template <typename T>
int upload(rn_handle* h, const T* src, size_t count, T** out) {
    return rn_owned_upload(h->allocs, 16, src, count, out);
}

// TF-1.13 compute_interpolation_weights (align_corners=False, no half-pixel centres) for in -> out samples, in float32:
// lo = int(i * scale), hi = min(lo + 1, in - 1), lerp = i * scale - lo.  The one host copy of the legacy bilinear table.
void rn_legacy_resize_table(int in_size, int out_size, int32_t* lo, int32_t* hi, float* lerp);

// Side of every stage's convolution output and of its output (after pooling) for w->im_side.  Returns the number of stages that
// fit: w->n_stages, or the index of the first stage for which im_side is too small (conv / out are valid in front of it).
int rn_stage_sides(const rn_weights* w, std::vector<int>& conv, std::vector<int>& out);

// The last conv block (stages 7-9 behind s6.bn), as grad-CAM and the fine-tuning trainers walk it: the side of s6.bn, then conv side and
// output side of stages 7, 8 and 9.  rn_lastblock_sides fills it from the graph's last four stages and returns what rn_stage_sides
// returns (less than w->n_stages: im_side is too small, `s` is not filled).
struct rn_lastblock {
    int S6, C7, S7, C8, S8, C9, S9;
};
int rn_lastblock_sides(const rn_weights* w, rn_lastblock* s);
// the legacy bilinear tables of stage 9's skip resize S7 -> S9, as both users upload them: rtab = [lo | hi] (2 S9), lerp (S9)
void rn_lastblock_resize_tables(const rn_lastblock& s, std::vector<int32_t>& rtab, std::vector<float>& lerp);

// tf.nn.batch_normalization folded to y = x * inv + shift, in float32 as every path of the library evaluates it
inline float rn_bn_inv(float var, float gamma, float eps) { return (1.0f / sqrtf(var + eps)) * gamma; }
inline float rn_bn_shift(float beta, float mean, float inv) { return beta - mean * inv; }

// A copy of a network's conv stages whose channels can be relabelled (frozen-channel folding): the permuted arrays are owned
// here, `w` describes the copy.  Position p of a relabelled tensor holds the reference's channel pi[p].
struct RelabelledWeights {
    rn_weights w;
    std::vector<rn_conv_stage> stages;
    std::vector<std::vector<float>> owned;
    explicit RelabelledWeights(const rn_weights* src);
    RelabelledWeights(const RelabelledWeights&) = delete;
    RelabelledWeights& operator=(const RelabelledWeights&) = delete;
    void permute_couts(int stage, const std::vector<int>& pi);     // its kernel's couts, its BN (and the second BN of a residual stage)
    void permute_cins(int stage, const std::vector<int>& pi);      // its kernel's cins
    void permute_block(int r, const std::vector<int>& pi);         // residual stage r pairs its channels with stage r - 1's: couts of r - 1, r; cins of r, r + 1
};
// Stage r is the 64 -> 64 residual stage (pool 4/2) of a depth-2 block between a 64-cout stage and a 64-cin stage without skips, and
// nobody else pairs with the block's two tensors: the block both frozen-channel folds relabel (each adds a condition of its own)
bool rn_fold_block_at(const rn_weights* w, int r);
void rn_fold_block_register(rn_handle* h, int r, const std::vector<int>& pi);      // its two tensors' entries in rn_handle::node_perm

// ---- the 16-bit storage types on the host (rn_to16, rn_from16 and the four conversions under them): rn_host16.h
#include "rn_host16.h"
