// 32 -> 64 stage with avg-pool 4/2 (reference network.py:228, first step of conv_block(64, pool 4/2, depth 2)) on 16x16x32
// matrix tiles with ROW-REGISTER BLOCKING (the shared pieces: rn_rowreg.h) -- rn_stage5x.hip without the residual:
//
//   in [N, W, W, 32] -> conv3x3 VALID -> ReLU6 -> avg-pool 4x4 stride 2 -> BN  = out [N, Wo, Wo, 64]
//
//  * a wave owns 16 couts (36 weight registers: 9 taps x 4) for 7 or 6 ADJACENT 16-pixel tiles; eight waves = 4 cout
//    quarters x 2 pixel halves, two per SIMD (7 + 6 tiles): 13 tiles cover the 203 conv columns (wide 32-pixel tiles: 224);
//  * every operand fragment (16 pixels x all 32 channels of one tap column of the NEWEST input row) feeds three
//    accumulators (kernel row 0 of conv row s, row 1 of s-1, row 2 of s-2): 3 LDS reads per tile and step for 9 MFMAs, three
//    independent chains; the partial accumulators of all tiles live across steps (84 registers); the ring only ever holds
//    the newest row and the rows in flight (4 slots);
//  * pooling (stride 2) on the matrix cores as in rn_stage5x.hip (fp16 pair sums = A operand, one accumulation per tile pair).
// The most matrix-dense launch of the pass held the lowest clock at the board's power cap (1.64 GHz, profiles/r3_clock.txt):
// the 16x16x32 shape costs less energy per FLOP (profiles/r2_power_cap.txt), and one workgroup per CU x 256 images is one
// round of the chip (the 2-wave workgroups of the row-streaming kernel ran 3.5 rounds).
// NQ = 3 (round 6): the channels of the last cout quarter are CONSTANTS on this handle (rn_fused_prepare proves per channel that the
// 16-bit store of fma(H, sc, sh) is one number for every H in [0, 16], relabels the channels so and fills them into the output
// tensor once, at rn_create): twelve waves = 3 live quarters x 4 pixel runs (4 + 3 + 3 + 3 tiles = 31 + 23 + 23 + 23 pooled
// columns), rotated over the SIMDs so that each carries 10 (one: 9) tile rows per step instead of 13.
// One workgroup = one image x one band of output rows x one COLUMN BLOCK of 95..101 pooled columns (194..206 input columns:
// the whole row of the 224 x 224 network, two blocks at 420, three at 600; rn_colblock_plan).  Blocks do not overlap in the
// output; the 4 halo columns of a block's input are read by both neighbours.
#include "rn_fused.h"
#include "rn_rowreg.h"

using namespace rnk;

namespace {

constexpr int U_NS = 4;                           // ring slots: the newest row + 3 in flight
constexpr int U_AHEAD = 3;
constexpr int U_RINGPX = 208;                     // pixels per ring row (13 tiles - 2 overlap columns + halo)
constexpr int U_ROW = U_RINGPX * 64;              // bytes per ring row (32 channels x 16 bit per pixel)
constexpr int U_TAB_BYTES = 4 * 64 * 4;
constexpr int U_RING_OFF = U_TAB_BYTES;
constexpr int U_LDS = U_RING_OFF + U_NS * U_ROW;
constexpr int U_WMIN = 193, U_WMAX = 206;

template <int DT, int NQ>
__global__ __launch_bounds__(NQ == 4 ? 512 : 768, NQ == 4 ? 2 : 3) void stage4x_kernel(const StageArgs a) {
    constexpr int U_NW = NQ == 4 ? 8 : 12;            // waves
    constexpr int U_NTH = U_NW * 64;
    constexpr int U_NT = NQ == 4 ? 7 : 4;             // tiles of the longest run
    constexpr int U_NU = (U_NT + 1) / 2;              // tile pairs (output stores per odd step) of the longest run
    RN_CLOCK_ENTRY();
    extern __shared__ __attribute__((aligned(64))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // cout quarter / pixel run.  NQ = 4: waves w and w + 4 share a SIMD (7 + 6 tiles).  NQ = 3: waves w, w + 4, w + 8 share a
    // SIMD and take the runs w, w + 1, w + 2 (mod 4) of the quarters 0, 1, 2
    const int cq = NQ == 4 ? (wave & 3) : (wave >> 2);
    const int run = NQ == 4 ? (wave >> 2) : (((wave & 3) + (wave >> 2)) & 3);
    const int px16 = lane & 15, g = lane >> 4;
    const int cb = blockIdx.x % a.n_cb, band = blockIdx.x / a.n_cb, n = blockIdx.y;
    const int Win = a.W, Wo_full = a.Wo, Ho = a.Ho;
    const int xo0 = a.cb_xo0[cb], Wo = a.cb_wo[cb];       // this block's pooled columns
    const int x0 = 2 * xo0;                               // its first input column
    const int W = min(2 * Wo + 4, Win - x0);              // input columns it reads
    const int yo0 = band * a.rows_per_band;
    const int nrows = min(Ho, yo0 + a.rows_per_band) - yo0;
    const int y0 = 2 * yo0;
    const int nconv = 2 * (nrows - 1) + 4;
    const int nin = nconv + 2;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    constexpr int OOB = 0x40000000;

    char* const ring = smem + U_RING_OFF;
    const unsigned ring_lds = lds_addr(ring);
    RN_ZERO_RING_TAIL(ring, W, tid, U_NS, U_RINGPX, U_WMIN, 4, U_NTH);

    // ---- this wave's tiles.  NQ = 4: run 0 = 7 tiles from column 0 (55 pooled columns), run 1 = 6 tiles from column 110 (47
    // pooled columns from 55).  NQ = 3: run 0 = 4 tiles (31 pooled columns), runs 1..3 = 3 tiles (23 each, from 31 / 54 / 77).
    // A run of t tiles pools 8 t - 1 columns; the next run starts 2 x that many conv columns further (2 columns of overlap).
    const bool has7 = run == 0;                           // (the longest run: U_NT tiles; the others one fewer)
    const int xo_run = NQ == 4 ? (run ? 55 : 0) : (run ? 8 + 23 * run : 0);
    const int xw = 2 * xo_run;
    const int nout_run = NQ == 4 ? (has7 ? 55 : 47) : (has7 ? 31 : 23);

    // ---- weights: fragment f = ky * 3 + kx (all 32 channels of the tap), B operand of D'[pixel][cout]
    RN_LOAD_WFRAGS(wf, 9, a.wfrag, 4, cq, lane);

    // ---- input rows by LDS-DMA: piece 0 = chunks tid (pixels 0..127); piece 1 = the remaining (W - 128) x 4 chunks, dealt
    // ceil(/8) to each wave, lane-masked (every wave keeps at least one active lane for W >= 193)
    const char* const in_img = reinterpret_cast<const char*>(a.in + static_cast<int64_t>(n) * Win * Win * 32) + x0 * 64;
    const int row_bytes = Win * 64;
    const unsigned goff0 = static_cast<unsigned>((tid >> 2) * 64 + (((tid & 3) ^ swz4x(tid >> 2)) << 4));
    // (a wave whose share of a short tail is empty loads the row's last chunk once more: the same bytes to the same place)
    const int tail_total = W * 4 - U_NTH;
    const int tailn = (tail_total + U_NW - 1) / U_NW;
    const int tail_start = min(wave * tailn, tail_total - 1);
    const int tail_cnt = max(1, min(tail_total - wave * tailn, tailn));
    const unsigned long long tail_mask = (1ull << tail_cnt) - 1ull;
    unsigned goff1;
    {
        const int q = U_NTH + tail_start + min(lane, tail_cnt - 1);
        const int p = q >> 2, c = q & 3;
        goff1 = static_cast<unsigned>(p * 64 + ((c ^ swz4x(p)) << 4));
    }
    // (the row pointer is carried by the caller, the slot is an immediate: see the steady loop)
    auto issue_row = [&](const char* row, auto SLOTC) __attribute__((always_inline)) {
        constexpr int slot = decltype(SLOTC)::value;
        unsigned o0 = goff0, o1 = goff1;
        asm volatile("" : "+v"(o0), "+v"(o1));
        dma16(row + o0, ring + slot * U_ROW + wave * 1024);
        dma16_masked(row + o1, ring + slot * U_ROW + (U_NTH + tail_start) * 16, tail_mask);
    };

    // ---- operand read bases (slot 0): tap column kx; tile k adds 16 pixels = 1024 bytes (same swizzle)
    unsigned base[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int p = xw + px16 + kx;
        base[kx] = ring_lds + static_cast<unsigned>(p * 64 + ((g ^ swz4x(p)) << 4));
    }

    // ---- pooling band matrices (stride 2)
    RN_POOL_BANDS_S2(pmA, pmB, pmC, px16, g);

    // ---- output stores: tile pair u = 16 pooled columns (pair 3 of the longer run: its 7th tile alone, 7 columns)
    int voff[U_NU];
#pragma unroll
    for (int u = 0; u < U_NU; ++u) {
        const int xo = xo_run + 16 * u + px16;
        const bool valid = 16 * u + px16 < nout_run && xo < Wo;
        voff[u] = valid ? ((xo0 + xo) * 64 + 16 * cq + 4 * g) * 2 : OOB;
    }
    // NQ = 3: the waves of quarter 2 also store the constant quarter behind theirs (lane: channels 48 + 4 g .. + 3): full lines
    [[maybe_unused]] i32x2 cq3v = {0, 0};
    if constexpr (NQ == 3) cq3v = *reinterpret_cast<const i32x2*>(a.cvals + 4 * g);
    // folded BN of the lane's 4 couts (16 cq + 4 g + i): y = S * sc + sh
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.ptab + 16 * cq + 4 * g);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(a.ptab + 64 + 16 * cq + 4 * g);

    // ---- state
    f32x4 acc[3][U_NT];           // partial accumulators of conv rows s, s-1, s-2 (index = conv row mod 3), per tile
    int hp[U_NT][2], pp2[U_NT][2];
#pragma unroll
    for (int k = 0; k < U_NT; ++k) {
        hp[k][0] = hp[k][1] = pp2[k][0] = pp2[k][1] = 0;
#pragma unroll
        for (int r3 = 0; r3 < 3; ++r3) acc[r3][k] = zero4;
    }
    const int out_row_bytes = Wo_full * 128;
    const char* const out_img = reinterpret_cast<const char*>(a.out + static_cast<int64_t>(n) * Ho * Wo_full * 64);

    // ---- row state carried from step to step instead of being recomputed from the step number:
    //  in_row   the input row the next step's DMA loads = band row min(s + U_AHEAD, nin - 1); it advances by row_bytes per step
    //           until it stands on the band's last row (nin >= 6: the prologue's three rows exist)
    //  orow     the output row the next emitting odd step stores (pooled row r = (s - 5) / 2: steps 1 and 3 emit nothing, and
    //           r < nrows holds for every s < nin = 2 nrows + 4)
    //  sd[]     the dither seeds of the period's odd steps: a period of 12 steps emits 6 rows, so the seed of the odd step 2 j + 1
    //           of every period is rn_dither_seed(yo0 + 6 n + j - 2) = that of row yo0 + j + 1 -- three wave constants
    const char* in_row = in_img + static_cast<int64_t>(y0) * row_bytes;
    issue_row(in_row, IC<0>{});
    issue_row(in_row + row_bytes, IC<1>{});
    issue_row(in_row + 2 * static_cast<int64_t>(row_bytes), IC<2>{});
    in_row += 3 * static_cast<int64_t>(row_bytes);
    const char* orow = out_img + static_cast<int64_t>(yo0) * out_row_bytes;
    [[maybe_unused]] unsigned sd[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) sd[t] = (!a.dither || cq == a.plain_q) ? RN_SEED_PLAIN : rn_dither_seed(yo0 + t + 1);
    wait_vmcnt<0>();
    RN_PIN_WFRAGS(wf, 9);
    lds_barrier();

    // operand fragments double-buffered across tiles: tile k + 1's three reads go out before tile k's MFMAs (a tile's
    // chain is only 9 MFMAs long: the LDS round trip at its head was a bubble as long as the chain itself) -- and across STEPS:
    // the first tile's fragments of row s + 1 are read at the end of step s, in front of the barrier (round 4; the barrier of a
    // step publishes the row AFTER the one the step computes).  Read behind the barrier they left both waves of every SIMD
    // waiting for LDS at the same moment, ~350 cycles of a ~2 950-cycle step with an idle matrix pipe.
    // The ring slot is part of the instruction's immediate (slot 3, tile 6: 46 080 < 2^16).
    i32x4 fq[2][3];
    auto reads_at = [&](auto KC, auto SLOTC) __attribute__((always_inline)) {
        constexpr int k = decltype(KC)::value, slot = decltype(SLOTC)::value;
        auto& dst = fq[k & 1];
        auto& bcr = base;                                              // (named outside the asm: implicit capture)
#pragma unroll
        for (int f = 0; f < 3; ++f) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst[f]) : "v"(bcr[f]), "n"(slot * U_ROW + k * 1024));
    };
    // One step = one input row s.  I = s mod 12 is compile time: the accumulator rotation (I mod 3), the row parity (I mod 2) and the
    // ring slot (I mod 4) are all immediates or register names.  H7: the wave owns the longest run (U_NT tiles; the others one fewer).
    // `early` (odd steps 1 and 3 only): OOB in the band's first period, whose steps 1 and 3 complete no pooled row, 0 afterwards.
    auto step = [&](auto IDXC, auto H7C, unsigned in_adv, int early, unsigned early_adv) __attribute__((always_inline)) {
        constexpr int I = decltype(IDXC)::value, R = I % 3, PAR = I % 2, SLOT = I % 4;
        constexpr bool H7 = decltype(H7C)::value != 0;
        constexpr int NTW = H7 ? U_NT : U_NT - 1;                      // this wave's tiles
        constexpr int iN = R, iM = (R + 2) % 3, iO = (R + 1) % 3;      // accumulators of conv rows s, s-1, s-2
        // row s + 1 has landed (row s was published by the previous step's barrier).  VM_CNT counts the output stores too and
        // retires in order: a step issues two DMA pieces behind its first MFMAs and, on odd rows, 3 (or 4: has7) stores at its
        // end.  Younger than the DMA of row s + 1 (issued at step s - 2): even s: DMA + stores of step s - 1 = 2 + 3; odd s:
        // stores of step s - 2, DMA of step s - 1 = 3 + 2 (one more with four stores: those waves wait for one piece more).
        // (NQ = 3: two stores per odd step)
        wait_vmcnt<(NQ == 4 ? 5 : 4)>();
        raw_barrier();
        // (nothing moves across the top of a step: with the whole period in one block the scheduler stretched live ranges over step
        //  borders until the twelve-wave form spilled)
        __builtin_amdgcn_sched_barrier(0);
        i32x4 op[U_NT + 1];
        op[U_NT - 1] = op[U_NT] = i32x4{0, 0, 0, 0};
        auto tile = [&](auto KC, auto NEXTC) __attribute__((always_inline)) {
            constexpr int k = decltype(KC)::value;
            constexpr bool NEXT = decltype(NEXTC)::value != 0;        // tile k + 1's reads are issued here (3 more in flight)
            if constexpr (NEXT) reads_at(IC<k + 1>{}, IC<SLOT>{});
            // (the row DMA rides behind the step's first MFMAs: into the slot of row s - 1 -- everybody is past it)
            frag_chain<DT, false, (NEXT ? 3 : 0), true, 3, 0, 1>(fq[k & 1], wf, acc[iN][k], acc[iM][k], acc[iO][k], zero4, [&](auto FC) __attribute__((always_inline)) {
                if constexpr (k == 0 && decltype(FC)::value == 0) {
                    issue_row(in_row, IC<(SLOT + U_AHEAD) % U_NS>{});
                    in_row += in_adv;
                }
            });
            // conv row j = s - 2 of this tile is complete: its pooling operand
            pool_rows<PAR>(acc[iO][k], hp[k], pp2[k], op[k]);
        };
        [&]<int... K>(std::integer_sequence<int, K...>) {
            (tile(IC<K>{}, IC<(K + 1 < NTW ? 1 : 0)>{}), ...);
        }(std::make_integer_sequence<int, NTW>{});
        if constexpr (PAR == 1) {
            // odd conv row j = s - 2 >= 3 completes pooled row r = (j - 3) / 2: the row `orow` stands on
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(orow), 0, out_row_bytes, 0x00020000);
            constexpr bool EARLY = I == 1 || I == 3;
            // bf16 handles: the row's stores are dithered by the output row (rn_stage.h); a constant quarter keeps the plain seed
            [[maybe_unused]] const unsigned seed = sd[((I - 1) / 2) % 3];
            auto out = [&](auto UC) __attribute__((always_inline)) {
                constexpr int u = decltype(UC)::value;
                f32x4 H = mfma16<RN_DTYPE_F16>(op[2 * u], pmA, zero4);
                H = mfma16<RN_DTYPE_F16>(op[2 * u + 1], pmB, H);
                if constexpr (2 * u + 2 < U_NT) H = mfma16<RN_DTYPE_F16>(op[2 * u + 2], pmC, H);
                float y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = __builtin_fmaf(H[i], sc[i], sh[i]);
                const i32x2 d = pack_out<DT>(y, seed);
                const int vo = EARLY ? (voff[u] | early) : voff[u];
                __builtin_amdgcn_raw_buffer_store_b64(d, rs, vo, 0, 0);
                if constexpr (NQ == 3)
                    if (cq == 2) __builtin_amdgcn_raw_buffer_store_b64(cq3v, rs, EARLY ? ((voff[u] + 32) | early) : voff[u] + 32, 0, 0);      // (wave-uniform; OOB stays OOB)
            };
            if constexpr (NQ == 4) {
                out(IC<0>{});
                out(IC<1>{});
                out(IC<2>{});
                if constexpr (H7) out(IC<3>{});
            } else {
                out(IC<0>{});
                out(IC<1>{});         // (the shorter runs' second pair is their third tile alone: op[3] = 0)
            }
            orow += EARLY ? early_adv : static_cast<unsigned>(out_row_bytes);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // first tile of the next row (published by this step's barrier)
        reads_at(IC<0>{}, IC<(SLOT + 1) % U_NS>{});
    };
    // The steady loop (steady_pairs, rn_rowreg.h): periods of 12 steps = lcm(ring slots 4, accumulator rotation 3, row parity 2)
    auto steady = [&](auto H7C) __attribute__((always_inline)) {
        // row 0 is published by the prologue's barrier only after every wave's pieces have landed: wait_vmcnt<0> above.  (Read here,
        // inside the instantiation: in front of the choice between the two the compiler copied the fragments' registers for one of
        // them before the data had arrived -- it cannot know that the statement is a load still in flight.)
        // The rule for every edit here: between a reads_at and the counted s_waitcnt that names its registers ("+v") there may be
        // no control-flow join at which fq could live in different registers on the two sides.  The joins that exist -- `if (done)
        // return` between pairs of steps and the loop's back edge -- have the same straight-line code (the previous step) on every
        // path that reaches them, so fq is one set of registers there; a new branch AROUND a reads_at would break that.
        reads_at(IC<0>{}, IC<0>{});
        steady_pairs<6>(nin, row_bytes, static_cast<unsigned>(out_row_bytes), [&](auto PC, unsigned in_adv, int early, unsigned early_adv) __attribute__((always_inline)) {
            constexpr int P = decltype(PC)::value;
            step(IC<2 * P>{}, H7C, in_adv, early, early_adv);
            step(IC<2 * P + 1>{}, H7C, in_adv, early, early_adv);
        });
    };
    // the longest run's waves and the others run two instantiations of the loop, chosen once (wave-uniform)
    if (has7)
        steady(IC<1>{});
    else
        steady(IC<0>{});
    wait_vmcnt<0>();
    RN_CLOCK_EXIT(a.stamp_buf, threadIdx.x == 256);
}

}  // namespace

// pooled columns per block: 2 wo + 4 input columns must lie in U_WMIN + 1 .. U_WMAX (the tail DMA piece needs > 192)
bool rn_stage4x_plan(int out_side, int* n_cb, int* xo0, int* wo) {
    return rn_colblock_plan(out_side, (U_WMIN + 1 - 4 + 1) / 2, (U_WMAX - 4) / 2, n_cb, xo0, wo);
}

bool rn_stage4x_supported(int cin, int cout, int pool_k, int pool_s, bool res, int in_side) {
    int ncb, xo0[4], wo[4];
    return cin == 32 && cout == 64 && pool_k == 4 && pool_s == 2 && !res && in_side >= U_WMIN &&
           rn_stage4x_plan((in_side - 6) / 2 + 1, &ncb, xo0, wo);
}

int rn_stage4x_launch(int dtype, hipStream_t s, const StageArgs& a, int n) {
    const dim3 grid(a.n_bands * a.n_cb, n);
    // three live quarters (StageArgs::live_q == 3): the twelve-wave form pools 100 columns per block at most
    bool q3 = a.live_q == 3;
    for (int b = 0; b < a.n_cb; ++b) q3 = q3 && a.cb_wo[b] <= 100;
    if (q3) return rn_launch16<stage4x_kernel<RN_DTYPE_BF16, 3>, stage4x_kernel<RN_DTYPE_F16, 3>, true>(dtype, grid, 768, U_LDS, s, a);
    return rn_launch16<stage4x_kernel<RN_DTYPE_BF16, 4>, stage4x_kernel<RN_DTYPE_F16, 4>, true>(dtype, grid, 512, U_LDS, s, a);
}
