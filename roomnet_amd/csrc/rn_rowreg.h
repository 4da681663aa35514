// What the ROW-REGISTER kernels on 16x16x32 matrix tiles share: rn_stage4x.hip (32 -> 64, pool 4/2), rn_stage5x.hip (64 -> 64 residual,
// pool 4/2) and rn_stage6x.hip (64 -> 128, un-pooled).  The design: a wave keeps the weights of its 16 couts in registers, and every
// operand fragment (16 pixels x 32 channels of one tap column of the NEWEST input row, one ds_read_b128) feeds three accumulators:
// kernel row 0 of conv row s, row 1 of conv row s-1, row 2 of conv row s-2.  The partial accumulators of all of a wave's tiles live
// across row steps, so the LDS ring only holds the newest row and the rows in flight.
// Every piece here was admitted on the gfx950 listings of the kernels that use it (profiles/rowreg_shared_isa.txt, tools/isa_diff.py).
// Two rules came out of that.  State that lives across the step loop (acc, hp, pp2, the fragment buffers) stays declared in the
// kernel, as plain arrays, and is passed by reference.  And the matrix code is functions, but the prologue pieces are MACROS: as
// functions (with a loop, or with a pack expansion in its place) they put the scalar set-up of rn_stage5x.hip in another order, which
// moved its register allocation inside the step loop.  The block / band / image geometry stays written out in each kernel for the
// same reason (a struct filled by one function turned `nin - 1 - x` from s_not into s_sub in 4x and 5x).
#pragma once
#include "rn_stage.h"

#include <utility>

namespace rnk {

// ---- pixels W .. RINGPX - 1 of every ring slot are never written by the row DMA: zero them once (the conv fragments of the discarded
// right-hand columns read them; uninitialised LDS could hold NaN patterns).  NS slots, CH 16-byte chunks per pixel, NTH threads, W >= WMIN
#define RN_ZERO_RING_TAIL(ring, W, tid, NS, RINGPX, WMIN, CH, NTH)                                                                 \
    for (int i = (tid); i < (NS) * ((RINGPX) - (WMIN)) * (CH); i += (NTH)) {                                                       \
        const int slot = i / (((RINGPX) - (WMIN)) * (CH)), rest = i % (((RINGPX) - (WMIN)) * (CH));                                \
        const int p = (WMIN) + rest / (CH), c = rest % (CH);                                                                       \
        if (p >= (W)) *reinterpret_cast<i32x4*>((ring) + slot * ((RINGPX) * (CH) * 16) + p * ((CH) * 16) + c * 16) = i32x4{0, 0, 0, 0}; \
    }                                                                                                                              \
    static_assert(true)

// ---- weights: declares i32x4 wf[N] and loads fragment f of the wave's 16-cout group (of NG) = frag[f][group][lane] (rn_pack.h);
// RN_PIN_WFRAGS stands behind the wait for them (the compiler cannot know the statements are loads still in flight)
#define RN_LOAD_WFRAGS(wf, N, frag, NG, group, lane)                                                 \
    i32x4 wf[N];                                                                                     \
    _Pragma("unroll")                                                                                \
    for (int f = 0; f < (N); ++f) {                                                                  \
        const i32x4* src = (frag) + (f * (NG) + (group)) * 64 + (lane);                              \
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(wf[f]) : "v"(src) : "memory");         \
    }                                                                                                \
    static_assert(true)
#define RN_PIN_WFRAGS(wf, N) \
    _Pragma("unroll")        \
    for (int f = 0; f < (N); ++f) asm volatile("" : "+v"(wf[f]))

// ---- the three MFMAs one operand fragment x feeds: kernel row 0 of conv row s (START: begun from `start`), row 1 of s-1, row 2 of s-2.
// WEIGHTS_A: D[cout][pixel] (the weights are the A operand), otherwise D'[pixel][cout]
template <int DT, bool WEIGHTS_A, bool START>
__device__ __forceinline__ void mma3(f32x4& aN, f32x4& aM, f32x4& aO, const i32x4& x, const i32x4& w0, const i32x4& w1, const i32x4& w2, const f32x4& start) {
    if constexpr (WEIGHTS_A) {
        aN = mfma16<DT>(w0, x, START ? start : aN);
        aM = mfma16<DT>(w1, x, aM);
        aO = mfma16<DT>(w2, x, aO);
    } else {
        aN = mfma16<DT>(x, w0, START ? start : aN);
        aM = mfma16<DT>(x, w1, aM);
        aO = mfma16<DT>(x, w2, aO);
    }
}

// ---- the fragment chain: wait for fragment i of `cur` with the N - 1 - i fragments behind it and BEHIND newer reads still in flight
// (LGKM_CNT retires in order), run its mma3, for i = 0 .. N - 1.  Fragment i's weights are wf[r * NF + W0 + WS * i] for kernel rows
// r = 0, 1, 2; START: fragment 0 begins conv row s.  hook(IC<i>) runs behind fragment i's MFMAs (rn_stage4x.hip's row DMA).
// The rule for every caller: between the reads of `cur` and this chain there may be no control-flow join at which `cur` could live in
// different registers on the two sides (the counted wait names the registers, "+v": the compiler cannot know a load is in flight).
struct no_hook {
    template <class T>
    __device__ __forceinline__ void operator()(T) const {}
};
template <int DT, bool WEIGHTS_A, int BEHIND, bool START, int NF, int W0, int WS, int N, class Hook = no_hook>
__device__ __forceinline__ void frag_chain(i32x4 (&cur)[N], const i32x4 (&wf)[3 * NF], f32x4& aN, f32x4& aM, f32x4& aO, const f32x4& start, Hook hook = {}) {
    [&]<int... F>(std::integer_sequence<int, F...>) {
        (([&] {
             asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(cur[F]) : "n"(BEHIND + N - 1 - F));
             mma3<DT, WEIGHTS_A, START && F == 0>(aN, aM, aO, cur[F], wf[0 * NF + W0 + WS * F], wf[1 * NF + W0 + WS * F], wf[2 * NF + W0 + WS * F], start);
             hook(IC<F>{});
         }()),
         ...);
    }(std::make_integer_sequence<int, N>{});
}

// ---- operand reads of the 64-channel rings (128-byte pixels, swz8; rn_stage5x.hip, rn_stage6x.hip).  base[kx][ch]: tap column kx,
// channel half ch, of the run's first tile (first column xw) in slot 0; tile K adds 16 pixels = 2048 bytes (same swizzle).
// K48 (the input channels 48..63 are constants on the handle): fragments 3, 4 of a tile = channels 32..47 of two taps -- lane groups
// 0, 1 read chunks 4, 5 of tap column 0 (fragment 4: column 2), groups 2, 3 those of column 1 (fragment 4: zero weights; they read what
// groups 0, 1 read); their bases take the places of base[0][1], base[1][1].
// Declares `base`.
#define RN_READ_BASES(base, K48, ring_lds, xw, px16, g)                                                            \
    unsigned base[3][2];                                                                                           \
    _Pragma("unroll")                                                                                              \
    for (int kx = 0; kx < 3; ++kx)                                                                                 \
        _Pragma("unroll")                                                                                          \
        for (int ch = 0; ch < 2; ++ch) {                                                                           \
            const int p = (xw) + (px16) + kx;                                                                      \
            base[kx][ch] = (ring_lds) + static_cast<unsigned>(p * 128 + (((4 * ch + (g)) ^ swz8(p)) << 4));        \
        }                                                                                                          \
    if constexpr (K48) {                                                                                           \
        _Pragma("unroll")                                                                                          \
        for (int j = 0; j < 2; ++j) {                                                                              \
            const int p = (xw) + (px16) + (j == 0 ? ((g) >> 1) : 2);                                               \
            base[j][1] = (ring_lds) + static_cast<unsigned>(p * 128 + (((4 + ((g) & 1)) ^ swz8(p)) << 4));         \
        }                                                                                                          \
    }                                                                                                              \
    static_assert(true)
// the three fragments of tile K, channel half CH (bc = base + the slot's offset) ...
template <int K, int CH>
__device__ __forceinline__ void reads3(i32x4 (&dst)[3], const unsigned (&bc)[3][2]) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[kx]) : "v"(bc[kx][CH]), "n"(K * 2048));
}
// ... and the five of a K48 tile
template <int K>
__device__ __forceinline__ void reads5(i32x4 (&dst)[5], const unsigned (&bc)[3][2]) {
#pragma unroll
    for (int f = 0; f < 5; ++f) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[f]) : "v"(f < 3 ? bc[f][0] : bc[f - 3][1]), "n"(K * 2048));
}

// ---- the pooling operand (stride 2): a complete conv row v of a tile -> ReLU6 -> fp16 pairs; the even row (PAR 0) waits in hp, the odd
// row forms the pair sum and the operand [previous pair sum | this pair sum] of the band-matrix MFMA (RN_POOL_BANDS_S2)
template <int PAR>
__device__ __forceinline__ void pool_rows(const f32x4& v, int (&hp)[2], int (&pp2)[2], i32x4& op) {
    const int v0 = static_cast<int>(pack2_relu6_sixth(v[0], v[1]));
    const int v1 = static_cast<int>(pack2_relu6_sixth(v[2], v[3]));
    if constexpr (PAR == 0) {
        hp[0] = v0;
        hp[1] = v1;
    } else {
        const int n0 = pk_add_f16(hp[0], v0), n1 = pk_add_f16(hp[1], v1);
        op = i32x4{pp2[0], pp2[1], n0, n1};
        pp2[0] = n0;
        pp2[1] = n1;
    }
}

// ---- the lane's four outputs as two 16-bit pairs: DITHER (bf16 only): stored with pack2_sr_bf16 and the row's `seed` (rn_stage.h)
template <int DT, bool DITHER = (DT == RN_DTYPE_BF16)>
__device__ __forceinline__ i32x2 pack_out(const float (&y)[4], [[maybe_unused]] unsigned seed) {
    if constexpr (DITHER)
        return i32x2{static_cast<int>(pack2_sr_bf16(y[0], y[1], seed)), static_cast<int>(pack2_sr_bf16(y[2], y[3], seed))};
    else
        return i32x2{static_cast<int>(pack2<DT>(y[0], y[1])), static_cast<int>(pack2<DT>(y[2], y[3]))};
}

// ---- the steady loop of the pooled kernels: periods of NP pairs of row steps.  nin is even, so a band ends behind an odd step: the
// loop is left there (no tail code: its last period is cut short).  Per pair one compare decides whether the input row pointer still
// advances: even step s loads row s + 3 and moves on iff s + 4 <= nin - 1, odd step s + 1 iff s + 5 <= nin - 1 -- with left = nin - s
// even, both are left >= 6.  `early` (odd steps 1 and 3 use it): OOB in the band's first period, whose steps 1 and 3 complete no
// pooled row, 0 afterwards; early_adv: 0 in the first period, adv_steady afterwards.  pair(IC<P>, in_adv, early, early_adv) runs steps 2 P, 2 P + 1
template <int NP, class Adv, class Pair>
__device__ __forceinline__ void steady_pairs(int nin, int row_bytes, Adv adv_steady, Pair pair) {
    int left = nin;                   // steps still to run, this pair included
    int early = 0x40000000;
    Adv early_adv = 0;
#pragma nounroll      // (the compiler would peel the first period off for its constant `early`: twice the code in the instruction cache)
    for (;;) {
        bool done = false;
        [&]<int... P>(std::integer_sequence<int, P...>) {
            (([&] {
                 if (done) return;
                 const unsigned in_adv = left >= 6 ? static_cast<unsigned>(row_bytes) : 0u;
                 pair(IC<P>{}, in_adv, early, early_adv);
                 left -= 2;
                 done = left == 0;
             }()),
             ...);
        }(std::make_integer_sequence<int, NP>{});
        if (done) break;
        early = 0;
        early_adv = adv_steady;
    }
}

}  // namespace rnk
