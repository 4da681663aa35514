// Training views (rn_view_draw, rn_views_*): the reference feeder's per-sample augmentation (generator.py:52-67, :85-92: a random
// square window slid along the photograph's long axis, resized to the network's side, mirrored left-right with probability 1/2 and
// upside-down with probability 1/2), drawn from the trainers' counter-based generator so that host and device agree bit for bit.
//
// For global step t (what rn_ft_step_count returns before the step), minibatch slot b, a 64-bit seed and a photograph of
// height x width, with Philox4x32-10 exactly as rn_dropout.h has it:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (0, b, (uint32) t, RN_VIEW_SITE | ((uint32)(t >> 32) << 8))
// RN_VIEW_SITE = 254 is a site no dropout site can take (those are 0 .. 1 + RN_MAX_DENSE), so the view draws and the dropout masks of
// one seed never share a counter.
//   side = min(height, width),  range = max(height, width) - side
//   RN_VIEW_CROP:  offset = (uint64) out[0] * range >> 32, a value in [0, range) as np.random.randint(range) gives one: the reference
//                  never draws offset == range, and neither does this.  range == 0: offset 0 and the whole image, as h == w in the
//                  reference.  The multiply-shift maps 2^32 words onto `range` values, so a value's probability differs from
//                  1 / range by less than 2^-32: the bias against a true uniform is below range / 2^32 in total.
//   otherwise:     the centre window of rn_center_crop_window (the reference's center_crop, its validation feeder)
//   height < width: the window is columns [offset, offset + side); otherwise rows [offset, offset + side)
//   RN_VIEW_FLIP:  fliplr = out[1] >> 31, flipud = out[2] >> 31; otherwise neither
// The view is flipud(fliplr(resize(window, (S, S)))): the flips come behind the resize, as in preprocess_set.
//
// Every source read stays inside the photograph for every possible draw: offset <= range in both modes (offset < range when it is
// drawn and range > 0, 0 when range == 0, and the centre offset (range + 1) / 2 <= range), so offset + side <= range + side =
// max(height, width) along the long axis, the window spans the whole short axis, and the resize clamps its reads to the window.
#pragma once
#include "rn_dropout.h"
#include "roomnet_hip.h"

// key and counter words of one launch / one draw
struct RnViewKey {
    uint32_t key0, key1;             // seed & 0xffffffff, seed >> 32
    uint32_t step_lo, step_hi;       // the global step
    unsigned flags;                  // RN_VIEW_CROP | RN_VIEW_FLIP
};

inline RnViewKey rn_view_key(uint64_t seed, int64_t step, unsigned flags) {
    const uint64_t t = static_cast<uint64_t>(step);
    return RnViewKey{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), flags};
}

// the draw of slot `slot`: the window's offset along the long axis (`centre`: what it is without RN_VIEW_CROP) and the two flips
RN_DROPOUT_HD inline void rn_view_draw_slot(const RnViewKey& k, uint32_t slot, int32_t range, int32_t centre, int32_t* offset,
                                            int32_t* fliplr, int32_t* flipud) {
    uint32_t w[4] = {0u, slot, k.step_lo, RN_VIEW_SITE | (k.step_hi << 8)};
    rn_philox4x32_10(w, k.key0, k.key1);
    *offset = (k.flags & RN_VIEW_CROP) ? static_cast<int32_t>((static_cast<uint64_t>(w[0]) * static_cast<uint32_t>(range)) >> 32) : centre;
    *fliplr = (k.flags & RN_VIEW_FLIP) ? static_cast<int32_t>(w[1] >> 31) : 0;
    *flipud = (k.flags & RN_VIEW_FLIP) ? static_cast<int32_t>(w[2] >> 31) : 0;
}
