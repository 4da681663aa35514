// What the calls made of masked forward passes share (rn_occlusion.hip: occlusion-sensitivity maps; rn_faith.hip: deletion and
// insertion curves): the handle's one workspace for a chunk of max_batch masked images, the per-image mean fills, the check of
// given class ids, and the shape of the chunk loop.  The functions live in rn_occlusion.hip.  Everything is enqueued on the
// handle's stream, so calls of either kind follow each other without a sync: a call's chunk is consumed by its own forward pass
// before the next call's mask launch overwrites it.
#pragma once
#include "rn_internal.h"

#include <algorithm>

// What the handle keeps for the masked passes, sized for max_batch, and the staging of the host entry points.
struct rn_masked_chunk {
    uint8_t* d_masked = nullptr;     // [max_batch, S, S, 3] the chunk's masked images
    float* d_probs = nullptr;        // [max_batch, num_classes] the chunk's probabilities
    int64_t* d_ids = nullptr;        // [max_batch] ... and classes (not read)
    uint8_t* d_fill = nullptr;       // [max_batch, 3] the per-image mean fills
    int32_t* d_cls = nullptr;        // [max_batch] the host entry points' class ids
    float* d_map = nullptr;          // [max_batch, S, S] rn_occlusion_u8's map
    float* d_drop = nullptr;         // rn_occlusion_u8's drops (grow-only)
    size_t drop_cap = 0;
    rn_timer timer;                  // rn_occlusion_last_ms
    bool ready = false;
};

// the handle's workspace, allocated by the first call (h->occlusion; rn_occlusion_release frees it)
int rn_masked_chunk_get(rn_handle* h, rn_masked_chunk** out);
// the per-image fills of a call without a triple, (2 sum + S S) / (2 S S) per channel -> st->d_fill
int rn_masked_enqueue_mean(rn_handle* h, rn_masked_chunk* st, const uint8_t* d_bgr, int n);
// class ids outside [0, num_classes): RN_E_INVALID.  ..._device reads them back on the handle's stream first (it waits).
int rn_masked_check_classes(const char* who, const rn_handle* h, const int32_t* cls, int n);
int rn_masked_check_classes_device(const char* who, rn_handle* h, const int32_t* d_cls, int n);

// The chunk loop: the `total` flattened masked passes in chunks of max_batch (the last one shorter).  Per chunk
// mask(first, count) enqueues the masked images into st->d_masked, the forward pass runs on them into st->d_probs, and
// score(first, count) enqueues what reads those probabilities.
template <class Mask, class Score>
int rn_masked_passes(rn_handle* h, rn_masked_chunk* st, int total, Mask&& mask, Score&& score) {
    int rc;
    for (int first = 0; first < total; first += h->max_batch) {
        const int count = std::min(h->max_batch, total - first);
        if ((rc = mask(first, count)) != RN_OK) return rc;
        if ((rc = rn_forward_u8_device(h, st->d_masked, count, st->d_probs, st->d_ids)) != RN_OK) return rc;
        if ((rc = score(first, count)) != RN_OK) return rc;
    }
    return RN_OK;
}
