// Dropout of the fine-tuning trainers (rn_ft_set_dropout): one counter-based generator, no stored masks.
//
// Every mask bit is recomputed wherever it is needed -- in the forward pass, in the adjoint, in rn_ft_dropout_mask -- from
// Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
// 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85, ten rounds.
// For element e of site `site`, minibatch slot b and global step t (what rn_ft_step_count returned before the step):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (e >> 2, b, (uint32) t, site | ((uint32)(t >> 32) << 8))
//   word    = out[e & 3];   k = word >> 8, a 24-bit value
// The element is kept iff k >= thr with thr = ceil((double) rate * 2^24), formed once on the host: exactly k 2^-24 >= rate,
// TensorFlow's rule random_uniform >= rate.  A kept value becomes x * scale (one float32 product) with scale = 1.0f / (1.0f - rate),
// one float32 division on the host; a dropped value becomes +0.0f.  The adjoint is g * scale where kept and 0 where dropped.
// The slot is the position in the minibatch, not the item: an item that occurs twice in a step gets two masks.
//
// Sites (dropout at every site at or behind the cached feature; the reference's dropout behind conv blocks 0-2, and at depth 2
// behind block 3, acts on frozen stages upstream of the cache and cannot be applied to cached features):
//   0      s6.bn, the input of stage 7 (depth-3 trainers only)             e = (y * S6 + x) * 128 + c within the item
//   1      the last conv block's output, which dense 0 reads flattened     e = (y * S9 + x) * 16 + c
//   2 + d  the output of dense block d: behind its BN for d < n_dense - 1; the last block's logits relu6(z) have no BN   e = unit j
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_DROPOUT_HD __host__ __device__
#else
#define RN_DROPOUT_HD
#endif

struct RnDropout {
    uint32_t key0, key1;             // seed & 0xffffffff, seed >> 32
    uint32_t thr;                    // keep iff (word >> 8) >= thr; 0: dropout is off
    float scale;                     // 1.0f / (1.0f - rate)
    uint32_t step_lo, step_hi;       // the global step of the launch
};

constexpr int RN_DROP_SITE_X6 = 0, RN_DROP_SITE_FLAT = 1, RN_DROP_SITE_DENSE = 2;

// Philox4x32-10: the counter c[4] becomes the output, in place
RN_DROPOUT_HD inline void rn_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c[0];
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c[2];
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = static_cast<uint32_t>(p1);
        c[2] = n2;
        c[3] = static_cast<uint32_t>(p0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the four words that hold elements 4 q .. 4 q + 3 of (site, slot)
RN_DROPOUT_HD inline void rn_dropout_words(const RnDropout& d, uint32_t site, uint32_t slot, uint32_t quad, uint32_t out[4]) {
    out[0] = quad;
    out[1] = slot;
    out[2] = d.step_lo;
    out[3] = site | (d.step_hi << 8);
    rn_philox4x32_10(out, d.key0, d.key1);
}

RN_DROPOUT_HD inline bool rn_dropout_word_keeps(const RnDropout& d, uint32_t word) { return (word >> 8) >= d.thr; }

// is element e of (site, slot) kept?
RN_DROPOUT_HD inline bool rn_dropout_keep(const RnDropout& d, uint32_t site, uint32_t slot, uint32_t e) {
    uint32_t w[4];
    rn_dropout_words(d, site, slot, e >> 2, w);
    return rn_dropout_word_keeps(d, w[e & 3]);
}

// x (forward) or g (adjoint) behind the dropout of element e: one float32 product where kept, +0.0f where dropped
RN_DROPOUT_HD inline float rn_dropout_apply(const RnDropout& d, uint32_t site, uint32_t slot, uint32_t e, float x) {
    return rn_dropout_keep(d, site, slot, e) ? x * d.scale : 0.f;
}
