// Deletion and insertion curves of a heat map: how the class probability falls when the pixels the map ranks
// highest are taken away a fraction at a time, and how it rises when they are put back in the same order.  Forward passes only -- the
// handle's own rn_forward_u8_device, through the masked chunk of rn_masked_chunk.h -- and four small kernels around them.  The
// definition, which roomnet_amd/faithfulness.py restates in NumPy:
//   side S, image im [S, S, 3] uint8 BGR, map m [S, S] float32 (any values), class c, steps J with 1 <= J <= S S, a fill: a BGR
//   triple or the image's own mean per channel, (2 sum + S S) / (2 S S) in integers, as occlusion defines it.
//   order    pixels by map value descending, equal values by raster index y S + x ascending, -0.0 equal to +0.0, NaN behind
//            everything else (NaNs among themselves by index): np.argsort(-m.ravel(), kind="stable").  rank[p] is pixel p's
//            position in that order, a permutation of 0 .. S S - 1.  The device sort key: rn_faith_rank.h.
//   steps    n_j = (j S S) / J in 64-bit integers for j = 0 .. J: n_0 = 0, n_J = S S.
//   images   deletion image j: pixels with rank < n_j hold the fill, the rest im; insertion image j: pixels with rank >= n_j hold
//            the fill, the rest im.  J + 1 points per curve, each its own forward pass; the endpoints the curves share are not
//            deduplicated (a forward pass need not give an image the same bits at another batch size or slot).
//   call     pass 0 is rn_forward_u8_device of the n <= max_batch unmasked images: the call's probs / ids.  c_i is class_ids[i], or
//            pass 0's ids[i], read on the device.  modes is a bit mask, RN_FAITH_DELETION = 1 | RN_FAITH_INSERTION = 2, M its set
//            bits, deletion first.  The n M (J + 1) passes, flattened as f = (i M + mode_slot) (J + 1) + j, are cut into chunks of
//            max_batch (the last one shorter; chunks cross curve and image boundaries); per chunk one mask launch, the forward pass,
//            one score launch: curve[i, mode_slot, j] = p_f[c_i], a float32 copy.
//   area     auc[i, mode_slot] = float32((sum over j = 0 .. J - 1, ascending, of float64(c_j) + float64(c_{j+1})) / (2 J)): a
//            sequential float64 sum, no fma.
//
//   faith_rank_kernel    one workgroup of 16 waves per image: the stable LSD radix sort of rn_faith_rank.h, four passes of 8-bit
//                        digits over (key, index) pairs that ping-pong between two halves of the workspace, the last pass
//                        scattering rank[index] = position.  A pass's buffers are written and re-read by different waves of the
//                        same workgroup: a workgroup barrier stands between the passes, and an image never spans workgroups.
//   faith_mask_kernel    copy with replace, driven by rank and n_j.  Dword path (3 S a multiple of 4, both buffers dword-aligned):
//                        one dword per lane; a dword spans two pixels, each of its 4 bytes is replaced on its own.  Byte path (odd
//                        sides): one byte per lane.  blockIdx.y is the masked image of the chunk.
//   faith_score_kernel   one thread per masked image of the chunk.
//   faith_auc_kernel     one thread per (image, curve).
// Every kernel parameter is passed by value.
#include "rn_masked_chunk.h"
#include "rn_faith_rank.h"

#pragma clang fp contract(off)

namespace {

using namespace rn_faith;

constexpr int64_t kMaxPasses = 1 << 20;           // n M (J + 1) of one call

struct RankArgs {
    const float* map;            // image i's map at map + i map_stride
    uint32_t* work;              // [n, 4, npix]: keys and indices, two sets
    uint32_t* rank;              // image i's ranks at rank + i rank_stride
    int64_t map_stride, rank_stride;
    int32_t npix;
};

// one tile's element of lane `lane`: its sort key and its raster index (pass 0 forms them from the map)
__device__ inline void rank_load(bool first_pass, const float* map, const uint32_t* kin, const uint32_t* iin, int e, int npix,
                                 uint32_t* key, uint32_t* idx) {
    if (e >= npix) {
        *key = 0;
        *idx = 0;
    } else if (first_pass) {
        *key = sort_key(__float_as_uint(map[e]));
        *idx = static_cast<uint32_t>(e);
    } else {
        *key = kin[e];
        *idx = iin[e];
    }
}

__device__ inline uint64_t rank_peers(uint32_t digit, bool valid) {
    uint64_t bit[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) bit[b] = __ballot(valid && ((digit >> b) & 1u));
    return peer_mask(bit, __ballot(valid), digit);
}

__global__ __launch_bounds__(kWaves * 64) void faith_rank_kernel(RankArgs a) {
    __shared__ uint32_t s_cnt[kWaves * kDigits];
    __shared__ uint32_t s_total[kDigits];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, npix = a.npix;
    const float* map = a.map + blockIdx.x * a.map_stride;
    uint32_t* work = a.work + static_cast<int64_t>(blockIdx.x) * 4 * npix;
    uint32_t* rank = a.rank + blockIdx.x * a.rank_stride;
    // (a wave's counters are read and advanced by different lanes of the wave, tile after tile: every access is issued, in order)
    volatile uint32_t* cnt = s_cnt + w * kDigits;
    int t0, t1;
    tile_range(npix, w, &t0, &t1);
    for (int pass = 0; pass < kPasses; ++pass) {
        const uint32_t* kin = work + static_cast<int64_t>((pass + 1) & 1) * 2 * npix;
        const uint32_t* iin = kin + npix;
        uint32_t* kout = work + static_cast<int64_t>(pass & 1) * 2 * npix;
        uint32_t* iout = kout + npix;
        for (int i = threadIdx.x; i < kWaves * kDigits; i += kWaves * 64) s_cnt[i] = 0;
        __syncthreads();
        // count: the walk over the wave's tiles, the next tile's element read ahead
        uint32_t key, idx, nkey = 0, nidx = 0;
        if (t0 < t1) rank_load(pass == 0, map, kin, iin, t0 * 64 + lane, npix, &nkey, &nidx);
        for (int t = t0; t < t1; ++t) {
            key = nkey;
            if (t + 1 < t1) rank_load(pass == 0, map, kin, iin, (t + 1) * 64 + lane, npix, &nkey, &nidx);
            const bool valid = t * 64 + lane < npix;
            const uint32_t d = digit_of(key, pass);
            const uint64_t peers = rank_peers(d, valid);
            if (valid && peers_lowest(peers, lane)) cnt[d] = cnt[d] + peers_all(peers);
        }
        __syncthreads();
        if (threadIdx.x < kDigits) scan_digit(s_cnt, s_total, threadIdx.x);
        __syncthreads();
        if (threadIdx.x == 0) scan_totals(s_total);
        __syncthreads();
        // scatter: the same walk; every lane reads its counter before the group's lowest lane advances it
        if (t0 < t1) rank_load(pass == 0, map, kin, iin, t0 * 64 + lane, npix, &nkey, &nidx);
        for (int t = t0; t < t1; ++t) {
            key = nkey;
            idx = nidx;
            if (t + 1 < t1) rank_load(pass == 0, map, kin, iin, (t + 1) * 64 + lane, npix, &nkey, &nidx);
            const bool valid = t * 64 + lane < npix;
            const uint32_t d = digit_of(key, pass);
            const uint64_t peers = rank_peers(d, valid);
            uint32_t pos = 0;
            if (valid) pos = s_total[d] + cnt[d] + peers_below(peers, lane);
            __builtin_amdgcn_wave_barrier();
            if (valid && peers_lowest(peers, lane)) cnt[d] = cnt[d] + peers_all(peers);
            // (the counts of a pass add up to npix and the indices are a permutation of the raster: both conditions always hold;
            //  they keep a damaged workspace from becoming a store outside the buffers)
            if (valid && pos < static_cast<uint32_t>(npix) && idx < static_cast<uint32_t>(npix)) {
                if (pass == kPasses - 1) {
                    rank[idx] = pos;
                } else {
                    kout[pos] = key;
                    iout[pos] = idx;
                }
            }
        }
        __syncthreads();      // the pass's stores are visible to the workgroup's other waves before the next pass reads them
    }
}

struct MaskArgs {
    const uint8_t* src;          // [n, S, S, 3]
    uint8_t* out;                // [count, S, S, 3]
    const uint32_t* rank;        // image i's ranks at rank + i rank_stride
    const uint8_t* fills;        // [n, 3] per-image fills, or null: `fill`
    int64_t rank_stride;
    uint32_t fill;               // B | G << 8 | R << 16
    int32_t S, J, modes;
    int32_t first;               // flattened index of the chunk's first pass
};

__device__ __host__ inline int mode_count(int modes) { return (modes & 1) + ((modes >> 1) & 1); }

// the flattened pass f: its image, its curve (0 deletion, 1 insertion) and its step
__device__ __host__ inline void pass_item(int f, int J, int modes, int* image, int* slot, int* insertion, int* j) {
    const int per = mode_count(modes) * (J + 1);
    const int i = f / per, r = f - i * per;
    *image = i;
    *slot = r / (J + 1);
    *j = r - *slot * (J + 1);
    *insertion = modes == 3 ? *slot : modes - 1;
}

template <bool DWORDS>
__global__ __launch_bounds__(256) void faith_mask_kernel(MaskArgs a) {
    int image, slot, insertion, j;
    pass_item(a.first + static_cast<int>(blockIdx.y), a.J, a.modes, &image, &slot, &insertion, &j);
    const int64_t npix = static_cast<int64_t>(a.S) * a.S, im_bytes = 3 * npix;
    const uint32_t n_j = static_cast<uint32_t>(j * npix / a.J);
    const uint32_t fill = a.fills ? (a.fills[3 * image] | (static_cast<uint32_t>(a.fills[3 * image + 1]) << 8) |
                                     (static_cast<uint32_t>(a.fills[3 * image + 2]) << 16))
                                  : a.fill;
    const uint8_t* src = a.src + image * im_bytes;
    const uint32_t* rank = a.rank + image * a.rank_stride;
    uint8_t* out = a.out + blockIdx.y * im_bytes;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if constexpr (DWORDS) {
        // (3 S S is a multiple of 4; bytes 4 t .. 4 t + 3 belong to pixels p and p + 1, and p + 1 <= S S - 1)
        if (t * 4 >= im_bytes) return;
        const int64_t p = t * 4 / 3;
        const int c0 = static_cast<int>(t * 4 - 3 * p);
        const bool f0 = (rank[p] < n_j) != (insertion != 0), f1 = (rank[p + 1] < n_j) != (insertion != 0);
        uint32_t v = reinterpret_cast<const uint32_t*>(src)[t];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool second = c0 + k >= 3;
            const int c = second ? c0 + k - 3 : c0 + k;
            if (second ? f1 : f0) v = (v & ~(0xFFu << (8 * k))) | (((fill >> (8 * c)) & 0xFFu) << (8 * k));
        }
        reinterpret_cast<uint32_t*>(out)[t] = v;
    } else {
        if (t >= im_bytes) return;
        const int64_t p = t / 3;
        const int c = static_cast<int>(t - 3 * p);
        const bool filled = (rank[p] < n_j) != (insertion != 0);
        out[t] = filled ? static_cast<uint8_t>(fill >> (8 * c)) : src[t];
    }
}

// curve[first + e] = p_f[e, c_i] for the chunk's masked images e = 0 .. count - 1
__global__ __launch_bounds__(64) void faith_score_kernel(const int64_t* __restrict__ ids0, const int32_t* __restrict__ cls,
                                                         const float* __restrict__ pw, int nc, int per_image, int first, int count,
                                                         float* __restrict__ curve) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= count) return;
    const int f = first + e, i = f / per_image;
    const int c = cls ? cls[i] : static_cast<int>(ids0[i]);
    curve[f] = pw[e * nc + c];
}

// auc[q] of curve q = i M + mode_slot: the trapezoid sum in float64, j ascending
__global__ __launch_bounds__(64) void faith_auc_kernel(const float* __restrict__ curve, int J, int n_curves, float* __restrict__ auc) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_curves) return;
    const float* c = curve + static_cast<int64_t>(q) * (J + 1);
    double sum = 0.0;
    for (int j = 0; j < J; ++j) sum = sum + (static_cast<double>(c[j]) + static_cast<double>(c[j + 1]));
    auc[q] = static_cast<float>(sum / (2.0 * static_cast<double>(J)));
}

// What the handle keeps for the ranking, sized for max_batch, and the staging of the host entry point.  16 bytes per pixel: the
// (key, index) pairs of the sort, two sets, [max_batch, 4, S S] uint32 -- set A = rows 0 (keys) and 1 (indices), set B = rows 2 and
// 3.  Pass 0 reads the map and writes A, pass 1 B, pass 2 A, pass 3 reads A and writes the ranks: into row 2 of the image's block
// (B is free by then) when the call keeps them for its masks.  rn_faith_u8 uploads its maps into row 2 as well: pass 0 has read
// them before pass 1 overwrites the row.
struct FaithState {
    uint32_t* d_work = nullptr;      // [max_batch, 4, S S]
    float* d_curve = nullptr;        // rn_faith_u8's curves (grow-only)
    size_t curve_cap = 0;
    float* d_auc = nullptr;          // [max_batch, 2] rn_faith_u8's areas
    rn_timer timer;
    bool ready = false;
};

int faith_state(rn_handle* h, FaithState** out) {
    if (!h->faith) {
        FaithState* s = new FaithState();
        h->faith = s;                  // (rn_faith_release frees whatever of it exists)
        const size_t nb = static_cast<size_t>(h->max_batch), px = static_cast<size_t>(h->im_side) * h->im_side;
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_work), nb * px * 16));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_auc), nb * 2 * sizeof(float)));
        int rc;
        if ((rc = s->timer.create()) != RN_OK) return rc;
        s->ready = true;
    }
    *out = static_cast<FaithState*>(h->faith);
    if (!(*out)->ready) {
        rn_set_error("rn_faith: the workspace could not be allocated earlier");
        return RN_E_STATE;
    }
    return RN_OK;
}

struct FaithPlan {
    int M, n_passes, n_chunks;
};

int check_plan(const char* who, const rn_handle* h, int n, int steps, int modes, FaithPlan* p) {
    if (!h) {
        rn_set_error("%s: null handle", who);
        return RN_E_INVALID;
    }
    const int rc = rn_faith_plan(h->im_side, steps, modes, n, h->max_batch, &p->n_passes, &p->n_chunks);
    if (rc != RN_OK) {
        const std::string why = rn_last_error();
        rn_set_error("%s: %s", who, why.c_str());
    }
    p->M = mode_count(modes);
    return rc;
}

int64_t pixels(const rn_handle* h) { return static_cast<int64_t>(h->im_side) * h->im_side; }
// where the call's own ranks and rn_faith_u8's maps live: row 2 of each image's block of the workspace
uint32_t* kept_row(const rn_handle* h, const FaithState* fs) { return fs->d_work + 2 * pixels(h); }

// the one rank enqueuer: n maps -> n rank arrays
int enqueue_ranks(rn_handle* h, const FaithState* fs, const float* d_map, int64_t map_stride, int n, uint32_t* d_rank, int64_t rank_stride) {
    RankArgs a;
    a.map = d_map;
    a.work = fs->d_work;
    a.rank = d_rank;
    a.map_stride = map_stride;
    a.rank_stride = rank_stride;
    a.npix = static_cast<int32_t>(pixels(h));
    (void)hipGetLastError();
    hipLaunchKernelGGL(faith_rank_kernel, dim3(n), dim3(kWaves * 64), 0, h->stream, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// The one mask enqueuer: the masked images of the flattened passes [first, first + count) into d_out, from the ranks the call keeps
// (enqueue_ranks ran on this stream).  `mean`: the fills are st->d_fill (rn_masked_enqueue_mean ran on this stream), otherwise `fill`.
int enqueue_masks(rn_handle* h, const FaithState* fs, const rn_masked_chunk* st, const uint8_t* d_bgr, int steps, int modes, bool mean,
                  const uint8_t* fill, int first, int count, uint8_t* d_out) {
    MaskArgs a;
    a.src = d_bgr;
    a.out = d_out;
    a.rank = kept_row(h, fs);
    a.rank_stride = 4 * pixels(h);
    a.fills = mean ? st->d_fill : nullptr;
    a.fill = mean ? 0u : (fill[0] | (static_cast<uint32_t>(fill[1]) << 8) | (static_cast<uint32_t>(fill[2]) << 16));
    a.S = h->im_side;
    a.J = steps;
    a.modes = modes;
    a.first = first;
    const int64_t im_bytes = pixels(h) * 3;
    const bool dwords = (3 * a.S) % 4 == 0 && (reinterpret_cast<uintptr_t>(d_bgr) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0;
    (void)hipGetLastError();
    if (dwords)
        hipLaunchKernelGGL(faith_mask_kernel<true>, dim3(static_cast<unsigned>((im_bytes / 4 + 255) / 256), count), dim3(256), 0, h->stream, a);
    else
        hipLaunchKernelGGL(faith_mask_kernel<false>, dim3(static_cast<unsigned>((im_bytes + 255) / 256), count), dim3(256), 0, h->stream, a);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// pass 0, the ranks, the masked passes and the areas; every argument is checked
int enqueue_all(rn_handle* h, FaithState* fs, rn_masked_chunk* st, const FaithPlan& plan, const uint8_t* d_bgr, const float* d_map,
                int64_t map_stride, int n, const int32_t* d_cls, int steps, int modes, const uint8_t* fill, float* d_curve, float* d_auc,
                float* d_probs, int64_t* d_ids) {
    int rc;
    // (a call that fails between start() and stop() leaves rn_faith_last_ms answering RN_E_STATE)
    if ((rc = fs->timer.start(h->stream)) != RN_OK) return rc;
    if ((rc = rn_forward_u8_device(h, d_bgr, n, d_probs, d_ids)) != RN_OK) return rc;
    if ((rc = enqueue_ranks(h, fs, d_map, map_stride, n, kept_row(h, fs), 4 * pixels(h))) != RN_OK) return rc;
    if (!fill && (rc = rn_masked_enqueue_mean(h, st, d_bgr, n)) != RN_OK) return rc;
    const int per_image = plan.M * (steps + 1);
    rc = rn_masked_passes(
        h, st, plan.n_passes,
        [&](int first, int count) { return enqueue_masks(h, fs, st, d_bgr, steps, modes, !fill, fill, first, count, st->d_masked); },
        [&](int first, int count) {
            (void)hipGetLastError();
            hipLaunchKernelGGL(faith_score_kernel, dim3((count + 63) / 64), dim3(64), 0, h->stream, d_ids, d_cls, st->d_probs, h->num_classes,
                               per_image, first, count, d_curve);
            RN_CHECK_LAUNCH();
            return RN_OK;
        });
    if (rc != RN_OK) return rc;
    if (d_auc) {
        (void)hipGetLastError();
        hipLaunchKernelGGL(faith_auc_kernel, dim3((n * plan.M + 63) / 64), dim3(64), 0, h->stream, d_curve, steps, n * plan.M, d_auc);
        RN_CHECK_LAUNCH();
    }
    return fs->timer.stop(h->stream);
}

}  // namespace

void rn_faith_release(rn_handle* h) {
    FaithState* s = static_cast<FaithState*>(h->faith);
    if (!s) return;
    for (void* p : {static_cast<void*>(s->d_work), static_cast<void*>(s->d_curve), static_cast<void*>(s->d_auc)})
        if (p) (void)hipFree(p);
    delete s;                          // (the timer frees itself)
    h->faith = nullptr;
}

extern "C" int rn_faith_plan(int side, int steps, int modes, int n, int max_batch, int* n_passes, int* n_chunks) {
    if (side < 1 || n < 1 || max_batch < 1) {
        rn_set_error("rn_faith_plan: side %d, n %d, max_batch %d: every value must be at least 1", side, n, max_batch);
        return RN_E_INVALID;
    }
    if (steps < 1 || steps > static_cast<int64_t>(side) * side) {
        rn_set_error("rn_faith_plan: steps = %d outside [1, %lld], the pixels of a side of %d", steps, static_cast<long long>(side) * side, side);
        return RN_E_INVALID;
    }
    if (modes < 1 || modes > 3) {
        rn_set_error("rn_faith_plan: modes = %d is not RN_FAITH_DELETION (1), RN_FAITH_INSERTION (2) or both (3)", modes);
        return RN_E_INVALID;
    }
    if (n > max_batch) {
        rn_set_error("rn_faith_plan: n = %d out of range (1..%d)", n, max_batch);
        return RN_E_RANGE;
    }
    const int64_t total = static_cast<int64_t>(n) * mode_count(modes) * (static_cast<int64_t>(steps) + 1);
    if (total > kMaxPasses) {
        rn_set_error("rn_faith_plan: %d images x %d curves x %d points = %lld masked passes, more than %lld", n, mode_count(modes), steps + 1,
                     static_cast<long long>(total), static_cast<long long>(kMaxPasses));
        return RN_E_RANGE;
    }
    if (n_passes) *n_passes = static_cast<int>(total);
    if (n_chunks) *n_chunks = static_cast<int>((total + max_batch - 1) / max_batch);
    return RN_OK;
}

extern "C" int rn_faith_rank_model(const float* map, int n, int npix, uint32_t* rank) {
    if (!map || !rank || n < 1 || npix < 1) {
        rn_set_error("rn_faith_rank_model: null buffer, or n = %d / npix = %d below 1", n, npix);
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i) rank_model_image(map + static_cast<int64_t>(i) * npix, npix, rank + static_cast<int64_t>(i) * npix);
    return RN_OK;
}

extern "C" int rn_faith_ranks_device(rn_handle* h, const float* d_map, int n, uint32_t* d_rank) {
    const char* who = "rn_faith_ranks_device";
    if (!h || !d_map || !d_rank || n < 1) {
        rn_set_error("%s: null argument, or n = %d below 1", who, n);
        return RN_E_INVALID;
    }
    if (n > h->max_batch) {
        rn_set_error("%s: n = %d out of range (1..%d)", who, n, h->max_batch);
        return RN_E_RANGE;
    }
    int rc;
    DeviceGuard guard(h->device);
    FaithState* fs = nullptr;
    if ((rc = faith_state(h, &fs)) != RN_OK) return rc;
    if ((rc = fs->timer.start(h->stream)) != RN_OK) return rc;
    if ((rc = enqueue_ranks(h, fs, d_map, pixels(h), n, d_rank, pixels(h))) != RN_OK) return rc;
    return fs->timer.stop(h->stream);
}

extern "C" int rn_faith_masks_device(rn_handle* h, const uint8_t* d_bgr, const float* d_map, int n, int steps, int modes,
                                     const uint8_t* fill_bgr, int first, int count, uint8_t* d_out) {
    const char* who = "rn_faith_masks_device";
    FaithPlan plan;
    int rc = check_plan(who, h, n, steps, modes, &plan);
    if (rc != RN_OK) return rc;
    if (!d_bgr || !d_map || !d_out) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    if (count < 1 || count > h->max_batch) {
        rn_set_error("%s: count = %d out of range (1..%d)", who, count, h->max_batch);
        return RN_E_RANGE;
    }
    if (first < 0 || first > plan.n_passes - count) {
        rn_set_error("%s: [%d, %d + %d) is not inside the call's %d masked images", who, first, first, count, plan.n_passes);
        return RN_E_RANGE;
    }
    DeviceGuard guard(h->device);
    FaithState* fs = nullptr;
    rn_masked_chunk* st = nullptr;
    if ((rc = faith_state(h, &fs)) != RN_OK || (rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    if ((rc = enqueue_ranks(h, fs, d_map, pixels(h), n, kept_row(h, fs), 4 * pixels(h))) != RN_OK) return rc;
    if (!fill_bgr && (rc = rn_masked_enqueue_mean(h, st, d_bgr, n)) != RN_OK) return rc;
    return enqueue_masks(h, fs, st, d_bgr, steps, modes, !fill_bgr, fill_bgr, first, count, d_out);
}

extern "C" int rn_faith_u8_device(rn_handle* h, const uint8_t* d_bgr, const float* d_map, int n, const int32_t* d_class_ids, int steps,
                                  int modes, const uint8_t* fill_bgr, float* d_curve, float* d_auc, float* d_probs, int64_t* d_ids) {
    const char* who = "rn_faith_u8_device";
    FaithPlan plan;
    int rc = check_plan(who, h, n, steps, modes, &plan);
    if (rc != RN_OK) return rc;
    if (!d_bgr || !d_map || !d_curve || !d_auc || !d_probs || !d_ids) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    // (validated before anything is launched: the classes are read back on the handle's stream)
    if (d_class_ids && (rc = rn_masked_check_classes_device(who, h, d_class_ids, n)) != RN_OK) return rc;
    FaithState* fs = nullptr;
    rn_masked_chunk* st = nullptr;
    if ((rc = faith_state(h, &fs)) != RN_OK || (rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    return enqueue_all(h, fs, st, plan, d_bgr, d_map, pixels(h), n, d_class_ids, steps, modes, fill_bgr, d_curve, d_auc, d_probs, d_ids);
}

extern "C" int rn_faith_u8(rn_handle* h, const uint8_t* bgr, const float* map, int n, const int32_t* class_ids, int steps, int modes,
                           const uint8_t* fill_bgr, float* curve, float* auc, float* probs, int64_t* ids) {
    const char* who = "rn_faith_u8";
    FaithPlan plan;
    int rc = check_plan(who, h, n, steps, modes, &plan);
    if (rc != RN_OK) return rc;
    if (!bgr || !map || !curve || !auc || !probs || !ids) {
        rn_set_error("%s: null buffer", who);
        return RN_E_INVALID;
    }
    if (class_ids && (rc = rn_masked_check_classes(who, h, class_ids, n)) != RN_OK) return rc;
    DeviceGuard guard(h->device);
    FaithState* fs = nullptr;
    rn_masked_chunk* st = nullptr;
    if ((rc = faith_state(h, &fs)) != RN_OK || (rc = rn_masked_chunk_get(h, &st)) != RN_OK) return rc;
    if ((rc = rn_grow_scratch(h, &fs->d_curve, &fs->curve_cap, static_cast<size_t>(plan.n_passes), "faithfulness curves")) != RN_OK) return rc;
    const size_t px = static_cast<size_t>(pixels(h));
    RN_HIP(hipMemcpyAsync(h->d_in_u8, bgr, static_cast<size_t>(n) * px * 3, hipMemcpyHostToDevice, h->stream));
    float* d_map = reinterpret_cast<float*>(kept_row(h, fs));          // (row 2 of each image's block: see FaithState)
    for (int i = 0; i < n; ++i)
        RN_HIP(hipMemcpyAsync(d_map + static_cast<size_t>(i) * 4 * px, map + static_cast<size_t>(i) * px, px * 4, hipMemcpyHostToDevice, h->stream));
    if (class_ids) RN_HIP(hipMemcpyAsync(st->d_cls, class_ids, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_all(h, fs, st, plan, h->d_in_u8, d_map, 4 * pixels(h), n, class_ids ? st->d_cls : nullptr, steps, modes, fill_bgr, fs->d_curve,
                     fs->d_auc, h->d_probs, h->d_ids);
    if (rc != RN_OK) return rc;
    RN_HIP(hipMemcpyAsync(curve, fs->d_curve, static_cast<size_t>(plan.n_passes) * 4, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipMemcpyAsync(auc, fs->d_auc, static_cast<size_t>(n) * plan.M * 4, hipMemcpyDeviceToHost, h->stream));
    return rn_results_to_host(h, n, probs, ids);
}

extern "C" int rn_faith_last_ms(rn_handle* h, float* ms) {
    const FaithState* fs = h ? static_cast<const FaithState*>(h->faith) : nullptr;
    return rn_timer::read("rn_faith_last_ms", h, fs && fs->ready ? &fs->timer : nullptr,
                          "no faithfulness call has enqueued all its launches on this handle", h ? h->device : 0, ms);
}
