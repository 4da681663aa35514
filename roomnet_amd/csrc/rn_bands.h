// Launch geometry: into how many bands of output rows a stage's image is cut.  A workgroup is image x column block x
// band; bands change no result bit, only how the launch fills the chip.  Pure host arithmetic, no HIP: rn_band_plan
// (include/roomnet_hip.h) exports it and tests/test_band_plan.py pins it.
#pragma once
#include <algorithm>
#include <cmath>

#include "roomnet_hip.h"

struct Bands {
    int rows_per_band, n_bands;
};

template <class Args> Args with_bands(Args a, const Bands& b) {      // the copy of bound arguments a launch works on
    a.rows_per_band = b.rows_per_band;
    a.n_bands = b.n_bands;
    return a;
}

// `bands` bands of equal height (at least min_rows rows each) that cover out_side rows
inline Bands rn_bands_from_count(int out_side, int bands, int min_rows = 1) {
    Bands r;
    r.rows_per_band = std::max((out_side + bands - 1) / bands, min_rows);
    r.n_bands = (out_side + r.rows_per_band - 1) / r.rows_per_band;
    return r;
}

// Cost of running `wgs` equal workgroups of `rows` row steps each with `slots` of them resident at a time, for the
// variants with several small workgroups per CU (they are back-filled as slots free up, so a launch does not run in
// whole rounds of the chip).  Fitted to band-count sweeps on the GPU (NOTES.md, rounds 1-2, "Band counts"):
//   * 2-wave workgroups, four per CU (32->64 stage): the fractional number of rounds plus an eighth of a round for the
//     ragged end, 1.5 row steps of prologue per workgroup (224: 2 bands; 600: 4);
//   * 4-wave workgroups, two per CU (64->128 stage): a partial last round costs at least 0.6 of a round (1.125 and 2.25
//     rounds measured as bad as 2 and 3), 3 row steps of prologue (224: 2 bands; 600: 5).
inline double rn_backfill_cost(long wgs, long slots, int rows, int wgs_per_cu) {
    const double r = std::max(1.0, static_cast<double>(wgs) / static_cast<double>(slots));
    if (wgs_per_cu >= 4) return (r + 0.12) * (rows + 1.5);
    const double whole = std::floor(r), frac = r - whole;
    return (whole + (frac > 1e-9 ? std::max(frac, 0.6) : 0.0)) * (rows + 3.0);
}

// Cost of workgroups that own a CU each: the launch runs in whole rounds of the chip, and a band costs its row steps plus
// a fixed number of steps of pipeline fill / rows its neighbour reads again.
inline long rn_rounds_cost(long wgs, long slots, long steps_per_band) {
    return (wgs + slots - 1) / slots * steps_per_band;
}

// The one search: the cheapest band count in 1 .. min(max_tried, max_bands) (the first of equal minima), then as many more
// bands as it takes to fill the `slots` workgroup slots of the chip.  per_band = workgroups per band count (images x column
// blocks); fill_first skips counts that leave slots empty.  cost(b) is a long or a double, compared as it is.
template <class Cost>
inline int rn_search_bands(long per_band, long slots, int max_bands, int max_tried, bool fill_first, Cost cost) {
    int bands = 1;
    decltype(cost(1)) best_cost = -1;
    for (int b = 1; b <= max_tried && b <= max_bands; ++b) {
        if (fill_first && per_band * b < slots && b < max_bands) continue;
        const auto c = cost(b);
        if (best_cost < 0 || c < best_cost) {
            best_cost = c;
            bands = b;
        }
    }
    if (per_band * bands < slots) bands = static_cast<int>(std::min<long>((slots + per_band - 1) / per_band, max_bands));
    return bands;
}

inline int rn_band_rows(int out_side, int b) { return (out_side + b - 1) / b; }

// ---- the families (RN_BANDS_* in roomnet_hip.h)
// stage 0 alone: ~4 workgroups of 8 waves per CU across the launch, at least 8 output rows per band
inline Bands rn_bands_stage0(int n, int out_side, int n_colblocks) {
    const int per_band = n * n_colblocks;
    int bands = (1024 + per_band - 1) / per_band;
    const int max_bands = (out_side + 7) / 8;
    if (bands > max_bands) bands = max_bands;
    if (bands < 1) bands = 1;
    return rn_bands_from_count(out_side, bands);
}

// generic kernel: aim for >= ~2 workgroups per CU across the launch, at least 4 output rows per band.  Tiny stages are pure
// latency chains (one wave per workgroup, a global-load round trip per row): every output row gets its own workgroup
// instead of 4 rows each.  wgs_per_band = column blocks x cout-tile groups.
inline Bands rn_bands_generic(int n, int out_side, int wgs_per_band) {
    const int per_band_wgs = n * wgs_per_band;
    int bands = (768 + per_band_wgs - 1) / per_band_wgs;
    const int max_bands = out_side <= 8 ? out_side : (out_side + 3) / 4;
    if (bands > max_bands) bands = max_bands;
    if (out_side <= 8) bands = max_bands;
    if (bands < 1) bands = 1;
    return rn_bands_from_count(out_side, bands);
}

// the fused pair: one workgroup per CU; bands only to fill the chip / even out the rounds (a band costs its rows plus 11
// steps of pipeline fill)
inline Bands rn_bands_pair(int n, int n_cu, int out_side, int n_cblocks) {
    const long per_band = static_cast<long>(n) * n_cblocks;
    const int bands = rn_search_bands(per_band, n_cu, (out_side + 7) / 8, 8, false,
                                      [&](int b) { return rn_rounds_cost(per_band * b, n_cu, rn_band_rows(out_side, b) + 11); });
    return rn_bands_from_count(out_side, bands);
}

// rn_conv16 (4-wave workgroups, two per CU) and rn_conv16p (3-wave workgroups, 72 KB of LDS: two per CU; 5-wave ones,
// 123 KB: one): back-filled, so the cost of a band count is the fractional number of rounds; the chip is filled first.
// The pooled kernel walks two conv rows per output row plus two of pool warm-up.
inline Bands rn_bands_conv16(int n, int n_cu, int out_side, int n_colblocks, int wgs_per_cu, bool pooled) {
    const long per_band = static_cast<long>(n) * n_colblocks;
    const long slots = static_cast<long>(wgs_per_cu) * n_cu;
    const int bands = rn_search_bands(per_band, slots, (out_side + 3) / 4, 8, true, [&](int b) {
        const int rows = rn_band_rows(out_side, b);
        return rn_backfill_cost(per_band * b, slots, pooled ? 2 * rows + 2 : rows, wgs_per_cu);
    });
    return rn_bands_from_count(out_side, bands);
}

// the row-register kernels (rn_stage4x / 5x / 6x): one workgroup (8 waves) per CU, whole rounds of the chip.  A band costs
// its input rows plus the rows its neighbour reads again (6 of the pooled stages, 2 of the un-pooled one); small batches
// take as many bands as it needs to fill the chip.
inline Bands rn_bands_rowreg(int n, int n_cu, int out_side, int n_cb, bool pooled) {
    const long per_band = static_cast<long>(n) * n_cb;
    const int rows_in = pooled ? 2 : 1, overlap = pooled ? 6 : 2;
    const int bands = rn_search_bands(per_band, n_cu, std::max(1, out_side / 4), 8, false, [&](int b) {
        return rn_rounds_cost(per_band * b, n_cu, rows_in * rn_band_rows(out_side, b) + overlap);
    });
    return rn_bands_from_count(out_side, bands);
}

// the register-weights kernels.  Workgroups per CU: one (8-wave variants; checked with HW_ID stamps) or four (the 2-wave
// workgroups of the 32->64 stage).  A band costs its rows plus ~10 rows of prologue / pool warm-up.  One workgroup per CU
// runs in whole rounds of the chip: 1 band at batch 256 x 224^2, 2 when e.g. 64 x 600^2 images x 6 column blocks = 384
// workgroups would otherwise run 1.5 rounds.  Small workgroups are back-filled as slots free up, so their cost is the
// fractional number of rounds (>= 1).  The un-pooled stage needs 4 rows per band (ring prologue depth).
inline Bands rn_bands_rw(int n, int n_cu, int out_side, int n_colblocks, int wgs_per_cu, int pool_k, int pool_s) {
    const long per_band = static_cast<long>(n) * n_colblocks;
    const long slots = static_cast<long>(n_cu) * wgs_per_cu;
    const int bands = rn_search_bands(per_band, slots, (out_side + 7) / 8, 8, false, [&](int b) {
        const long wgs = per_band * b;
        const long rows_b = rn_band_rows(out_side, b) * (pool_k ? pool_s : 1);     // conv rows of a band
        return wgs_per_cu == 1 ? static_cast<double>((wgs + slots - 1) / slots) * static_cast<double>(rows_b + 10)
                               : rn_backfill_cost(wgs, slots, static_cast<int>(rows_b) + 2, wgs_per_cu);
    });
    return rn_bands_from_count(out_side, bands, pool_k == 0 ? 4 : 1);
}

// float32 on the matrix cores: whole rounds of the chip (one workgroup per CU: the weights and the ring fill most of its
// LDS); a band costs its rows plus the rows its neighbour reads again; up to 16 bands.  wgs_per_band = column blocks x
// cout-tile groups.
inline Bands rn_bands_f32m(int n, int n_cu, int out_side, int wgs_per_band, int pool_k, int pool_s) {
    const long per_band = static_cast<long>(n) * wgs_per_band;
    const int rows_in = pool_k ? pool_s : 1, overlap = pool_k ? 5 : 2;
    const int bands = rn_search_bands(per_band, n_cu, std::max(1, out_side / 4), 16, false, [&](int b) {
        return rn_rounds_cost(per_band * b, n_cu, rows_in * rn_band_rows(out_side, b) + overlap);
    });
    return rn_bands_from_count(out_side, bands);
}

// the dispatcher behind rn_band_plan; false for an unknown family
inline bool rn_bands_family(int family, int n, int n_cu, int out_side, int n_colblocks, int wgs_per_cu, int pool_k, int pool_s, Bands* out) {
    switch (family) {
        case RN_BANDS_STAGE0: *out = rn_bands_stage0(n, out_side, n_colblocks); return true;
        case RN_BANDS_GENERIC: *out = rn_bands_generic(n, out_side, n_colblocks); return true;
        case RN_BANDS_PAIR: *out = rn_bands_pair(n, n_cu, out_side, n_colblocks); return true;
        case RN_BANDS_CONV16: *out = rn_bands_conv16(n, n_cu, out_side, n_colblocks, 2, false); return true;
        case RN_BANDS_CONV16P: *out = rn_bands_conv16(n, n_cu, out_side, n_colblocks, wgs_per_cu, true); return true;
        case RN_BANDS_ROWREG: *out = rn_bands_rowreg(n, n_cu, out_side, n_colblocks, pool_k != 0); return true;
        case RN_BANDS_RW: *out = rn_bands_rw(n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s); return true;
        case RN_BANDS_F32M: *out = rn_bands_f32m(n, n_cu, out_side, n_colblocks, pool_k, pool_s); return true;
    }
    return false;
}
