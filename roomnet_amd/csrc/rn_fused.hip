// Fused 16-bit execution path (RN_DTYPE_BF16 / RN_DTYPE_F16), host side.  rn_fused_prepare decides once per handle which kernel family
// (rn_fused.h lists their files) runs every conv stage, packs its weights and tables and binds its launch arguments; rn_fused_forward
// walks the stages, adds what depends on the call (the bands of this batch size, the image pointer) and launches.
#include "rn_fused.h"
#include "rn_clock.h"
#include "rn_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace rnk;

namespace {

// The kernel family that runs a stage as a launch of its own; a stage has exactly one (choose_family).  Generic: stage_mfma_kernel
// (rn_generic.hip), any shape; RegWeights: rn_stage_rw.hip; Conv16 / Conv16P: rn_conv16.hip; Row4x / 5x / 6x: rn_stage4x / 5x / 6x.hip.
enum class Family { Generic, RegWeights, Conv16, Conv16P, Row4x, Row5x, Row6x };

struct FusedStage {
    Family family = Family::Generic;
    // the register-weights kernel could run this stage (rn_rw_supported, no RN_FLAG_GENERIC_KERNELS): it then has `rw`, `ptab` and,
    // where its kernels clamp to [0, 1], `sixth` weights whichever family runs it; the pair, the stage-0 fusion and the tail ask for it
    bool rw_capable = false;
    RwPlan rw;
    GenericPlan gen;
    bool sixth = false;          // conv weights stored / 6, folded BN scale x 6 (pack2_relu6_sixth in the stage's kernel)
    i32x4* wfrag = nullptr;      // fragments in the generic order: Generic, RegWeights, the tail, the back end, the round-2 pair
    i32x4* family_wfrag = nullptr;   // ... in its own family's order (Conv16 .. Row6x), without the constant input channels the handle folds
    float* ptab = nullptr;       // folded BN tables for every family but Generic (stage_table) ...
    std::vector<float> tab;      // ... and their host copy
    std::vector<float> wq;       // the conv weights every pack of the stage reads (host, HWIO: / 6 when `sixth`, refined rounding)
    // the launch arguments, bound at rn_create: all but the bands of a batch size (rows_per_band, n_bands), stamp_buf and the image s0_bgr
    bool conv16() const { return family == Family::Conv16 || family == Family::Conv16P; }    // `c16` is the live member, else `args`
    union {
        StageArgs args{};
        Conv16Args c16;
    };
};

struct FusedState {
    std::vector<FusedStage> st;
    // cross-stage fusion: launch_rep[i] = the stage under which the launch that computes stage i reports its time (== i: its own)
    std::vector<int> launch_rep;
    bool fuse_s0 = false;        // stage 0 is computed inside stage 1's kernel (rn_stage_rw.hip, S0F)
    bool use_tail = false;       // last two stages + head in one launch (rn_tail.hip)
    // the whole back end (stage 6 -> 7 -> 8 -> 9 -> head) in one launch, one workgroup per image (rn_backend.hip): taken when the
    // batch fills at least half the chip; smaller batches keep the launches that cut an image into bands
    bool use_backend = false;
    bool last_backend = false;   // the last forward pass ran it: stages 6 and 7 were not written
    // cross-stage fused pair (rn_stage23.hip): stages pair_first, pair_first + 1 run as one launch with `pair_args`
    int pair_first = -1;
    bool pair_x16 = false;       // the pair runs on 16x16x32 tiles (rn_stage23x.hip) with fragments and a table of its own
    int pair_frozen = 0;         // how many channels of its on-chip tensor are frozen on this handle
    Stage23Args pair_args{};     // bound at rn_create like FusedStage::args
    // frozen first-BN channels of the 64 -> 64 residual stage (fold16): its index (or -1); the convolution of two of its four 16-cout
    // quarters still runs (live_q; the channel relabelling of the tensors it touches: rn_handle::node_perm)
    int fold5_stage = -1;
    // round 6: refined rounding of the 16-bit handles (default; off under RN_FLAG_NO_DITHER and on the legacy comparison arms):
    // `refine` = conv weights rounded with the residual carried from tap to tap (diffuse_taps), `dither` (bf16 only) = the stores of
    // the large stage outputs go through v_cvt_sr_bf16_f32 with a seed that depends on the output row (rn_stage.h)
    bool refine = false;
    std::vector<char> dither_out;    // per conv stage: its output rows are dithered
    int relabel_stage = -1;          // the residual stage whose channels (and its neighbours') are stored relabelled -- also on the
                                     // arm that computes every channel (same channel order in both arms: same MFMA summation order)
    bool const_layout = false;       // positions 48..63 of the two relabelled tensors hold the constant channels (both arms)
    int const4_proven = 0;           // channels of that stage with a constant 16-bit store on this handle
    // 16 of them sit in positions 48..63 and no kernel computes them (prepare_const_channels): all are frozen channels of the residual
    // stage too, so its output has constants there as well.  Both tensors are filled once (rn_fused_post_alloc); the stages around
    // them are told through live_q, cvals, cstart and fragments of 48 input channels.
    bool const4 = false;
    unsigned short const_val[2][16] = {};   // their stored values (s4.bn positions 48..63) | those of the residual stage's output (s5.bn2)
    Stage0Args s0_args{};            // stage 0 as a launch of its own; its fragments and table also feed the fusion into stage 1
};

}  // namespace

void rn_fused_release(rn_handle* h) {
    delete static_cast<FusedState*>(h->fused);
    h->fused = nullptr;
}

// Conv weights [tap][cin][cout] -> the handle's 16-bit values with the rounding residual CARRIED from tap to tap (centre first): the
// nine taps of a (cin, cout) pair then sum to the exact sum within half an ulp of ONE weight instead of the sum of nine independent
// roundings -- smooth image content sees the tap sum (on the parity set the weight share of the bf16 logit error goes from 0.061 to
// 0.007, tools/sim16.py).  The array is rewritten with exactly representable values: every later conversion is exact, every kernel
// family packs the same numbers.
static void diffuse_taps(float* w, int cin, int cout, int dtype) {
    static const int order[9] = {4, 0, 8, 2, 6, 1, 7, 3, 5};
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co) {
            float carry = 0.f;
            for (int t : order) {
                float& x = w[(static_cast<size_t>(t) * cin + ci) * cout + co];
                const float v = x + carry;
                const float q = rn_from16(rn_to16(v, dtype), dtype);
                carry = std::isfinite(q) ? v - q : 0.f;
                x = q;
            }
        }
}

// The 16-bit store of the tensors whose kernels store through v_cvt_sr_bf16_f32 (the 64-channel block's two outputs): bf16 with the
// plain seed whether the handle dithers or not (round half away from zero), fp16 to nearest even.  (Stores that are never dithered --
// constant channels, the pair's on-chip tensor -- are rn_to16.)
static unsigned short cv_store(float v, int dtype) { return dtype == RN_DTYPE_BF16 ? rn_sr_bf16_host(v, RN_SEED_PLAIN) : f32_to_f16(v); }

// The folded BN table of a conv stage as its kernels read it, [scale | shift | inv2 | sh2] x cout:
//   y = S * (inv / k^2) + (beta - mean * inv);  y2 = (y + r) * inv2 + (beta2 - mean2 * inv2)
// Residual stages: y2 = (S * sc1 + sh1 + R) * sc2 + sh2 = S * (sc1 sc2) + R * sc2 + (sh1 sc2 + sh2): scale / shift hold the products,
// so the epilogue is two fmas around the resized skip value.  `sixth`: the conv weights are stored / 6 and the scale carries the 6.
// The kernels' tables and every proof of a frozen or constant channel read this one function.
static std::vector<float> stage_table(const rn_conv_stage& ws, float eps, bool sixth) {
    const int cout = ws.cout;
    std::vector<float> tab(static_cast<size_t>(4) * cout, 0.f);
    for (int c = 0; c < cout; ++c) {
        const float inv = rn_bn_inv(ws.variance[c], ws.gamma[c], eps);
        tab[c] = ws.pool_k ? inv / static_cast<float>(ws.pool_k * ws.pool_k) : inv;
        tab[cout + c] = rn_bn_shift(ws.beta[c], ws.mean[c], inv);
        if (ws.skip_stage >= 0) {
            const float inv2 = rn_bn_inv(ws.variance2[c], ws.gamma2[c], eps);
            const float sh2 = rn_bn_shift(ws.beta2[c], ws.mean2[c], inv2);
            tab[2 * cout + c] = inv2;
            tab[3 * cout + c] = sh2;
            tab[cout + c] = tab[cout + c] * inv2 + sh2;
            tab[c] = tab[c] * inv2;
        }
        if (sixth) tab[c] *= 6.0f;
    }
    return tab;
}

// What constant input channels add to every output of a conv: cst[co] = the sum over `terms` of (16-bit weight) x (the channel's
// stored 16-bit value) -- the products the matrix cores would form -- in double, in the order of `terms`.  A term is a row
// [tap][cin] of the HWIO weights `w` (as the stage packs them) and the stored value.
struct ConstTerm {
    size_t row;
    double val;
};
static std::vector<float> const_sum(const float* w, int cout, const std::vector<ConstTerm>& terms, int dtype) {
    std::vector<float> cst(cout);
    for (int co = 0; co < cout; ++co) {
        double sum = 0.0;
        for (const ConstTerm& t : terms) sum += static_cast<double>(rn_from16(rn_to16(w[t.row * cout + co], dtype), dtype)) * t.val;
        cst[co] = static_cast<float>(sum);
    }
    return cst;
}
// ... of input channels 48..63 of a 64-channel tensor holding vals[0..15], tap by tap
static std::vector<float> const_sum48(const float* w, int cout, const unsigned short* vals, int dtype) {
    std::vector<ConstTerm> terms;
    for (int tap = 0; tap < 9; ++tap)
        for (int p = 48; p < 64; ++p) terms.push_back({static_cast<size_t>(tap) * 64 + p, rn_from16(vals[p - 48], dtype)});
    return const_sum(w, cout, terms, dtype);
}

static int upload16(rn_handle* h, const std::vector<unsigned short>& v, i32x4** out) {
    unsigned short* d = nullptr;
    const int rc = upload(h, v.data(), v.size(), &d);
    *out = reinterpret_cast<i32x4*>(d);
    return rc;
}

// dithered outputs: the large stage tensors in front of the back end (the last four stages run in one launch per image and keep their
// tensors in LDS), except stage 0 (it lives in LDS rings inside stage 1's kernel) and the first stage of a fusable 32 -> 32 pair (its
// output is the pair's on-chip tensor; the frozen-channel fold relies on its plain rounding)
static void plan_dither(const rn_handle* h, FusedState* fs) {
    fs->refine = !(h->flags & (RN_FLAG_GENERIC_KERNELS | RN_FLAG_PAIR_32X32 | RN_FLAG_NO_DITHER));
    const bool dither = fs->refine && h->dtype == RN_DTYPE_BF16;
    fs->dither_out.assign(h->stages.size(), 0);
    const int ns = static_cast<int>(h->stages.size());
    for (int i = 1; i + 4 < ns && dither; ++i) {
        const StagePlan& s = h->stages[i];
        const bool pair_first = i + 1 < ns && s.cin == 32 && s.cout == 32 && s.pool_k == 4 && s.pool_s == 1 && s.skip_stage < 0 &&
                                h->stages[i + 1].cin == 32 && h->stages[i + 1].cout == 32 && h->stages[i + 1].skip_stage == i - 1;
        // (the stages whose kernels carry the SR store: 32+ channels in and out, residual or stride-2 pooling -- stages 3, 4, 5;
        //  the first block's first step stays plain: its 1.5 M values per image cost more as SR stores than their dither returned)
        const bool srp = s.cin >= 32 && s.cout >= 32 && (s.skip_stage >= 0 || s.pool_s == 2);
        fs->dither_out[i] = (pair_first || !srp) ? 0 : 1;
    }
}

// ---- frozen first-BN channels of a 64 -> 64 residual stage (stage 5 of the network; rn_stage5x.hip).  Its epilogue forms
// y1 = fma(H, sc1', sh1') with H = a pooled sum of ReLU6 / 6 values in [0, 16]: where |sc1'| * 16 < 2^-25 |sh1'| the fma
// returns sh1' EXACTLY in float32 for every input -- the channel's convolution cannot change a bit of the output (the
// reference's L2 regulariser drove 44 of the 64 gammas of the shipped checkpoint to ~1e-30).  With >= 32 such channels the
// channels of this stage's output are RELABELLED (a permutation of the weights of this stage, of the cout of the stage
// before -- whose output is this stage's input AND its skip tensor, paired channel by channel -- and of the cin of the stage
// behind) so that the last two 16-cout quarters are all frozen: their waves skip the convolution and its pooling.  The
// relabelling happens HERE, on a copy of the weight arrays, in front of everything else: every kernel family of every arm
// sees one consistent network; rn_tap puts the channels of the two affected tensors back in the reference's order.  The proofs
// read the tables of the original channel order (relabelling only permutes per-channel values).
static void fold16(rn_handle* h, FusedState* fs, const rn_weights* w_in, RelabelledWeights* rw) {
    if (h->flags & (RN_FLAG_GENERIC_KERNELS | RN_FLAG_PAIR_32X32)) return;
    const bool fold_ok = !(h->flags & RN_FLAG_COMPUTE_FROZEN);      // (the computing arm keeps the relabelling and folds nothing)
    for (int r = 2; r + 1 < w_in->n_stages; ++r) {
        const rn_conv_stage& s5 = w_in->stages[r];
        const rn_conv_stage& s4 = w_in->stages[r - 1];
        const StagePlan& p5 = h->stages[r];
        if (!rn_fold_block_at(w_in, r) || !rn_stage5x_supported(s5.cin, s5.cout, s5.pool_k, s5.pool_s, true, p5.in_side, p5.skip_side)) continue;
        std::vector<int> frozen, live;
        const std::vector<float> t5 = stage_table(s5, w_in->bn_epsilon, true);
        for (int c = 0; c < 64; ++c) {
            const float t0 = t5[c], t1 = t5[64 + c];
            const bool fz = static_cast<double>(std::fabs(t0)) * 16.0 * (1.0 + 1e-6) < static_cast<double>(std::fabs(t1)) * 2.98023223876953125e-8;      // 2^-25
            (fz ? frozen : live).push_back(c);
        }
        if (frozen.size() < 32) continue;
        // ---- constant channels of the stage in front (round 6).  Its kernel (rn_stage4x.hip) stores
        // pack2<DT>(fma(H, sc, sh)) with H = a pooled sum of ReLU6 / 6 values in [0, 16]; fma and the 16-bit conversion are
        // monotone in H, so where the two ends H = 0 and H = 16 convert to the same 16-bit number every input does: the
        // stored channel is that number at every pixel of every image, bit for bit what the kernel that computes it stores
        // (the shipped checkpoint: 26 channels in bf16, 23 in fp16 -- its L2 regulariser left their BN scale below half an
        // ulp of the shift -- all of them among this stage's frozen channels).
        std::vector<int> cst;
        std::vector<unsigned short> cst_val(64, 0);
        if (rn_stage4x_supported(s4.cin, s4.cout, s4.pool_k, s4.pool_s, false, h->stages[r - 1].in_side)) {
            const std::vector<float> t4 = stage_table(s4, w_in->bn_epsilon, true);
            for (int c = 0; c < 64; ++c) {
                const float sc = t4[c], sh = t4[64 + c];
                const unsigned short v0 = cv_store(std::fmaf(0.0f, sc, sh), h->dtype), v16 = cv_store(std::fmaf(16.0f, sc, sh), h->dtype);
                cst_val[c] = v0;
                if (v0 == v16 && std::isfinite(sh)) cst.push_back(c);
            }
        }
        fs->const4_proven = static_cast<int>(cst.size());
        {
            // frozen channels that are constants of the stage in front go LAST (positions 48..63 when there are 16 of them)
            std::vector<int> both, only;
            for (int c : frozen) (std::find(cst.begin(), cst.end(), c) != cst.end() ? both : only).push_back(c);
            fs->const_layout = both.size() >= 16;
            fs->const4 = fs->const_layout && fold_ok;
            frozen = only;
            frozen.insert(frozen.end(), both.begin(), both.end());
        }
        std::vector<int> pi(64);
        while (frozen.size() > 32) {             // (the spare frozen channels -- taken from the front -- are computed like live ones)
            live.push_back(frozen.front());
            frozen.erase(frozen.begin());
        }
        std::sort(live.begin(), live.end());
        for (int p = 0; p < 32; ++p) pi[p] = live[p];
        for (int p = 0; p < 32; ++p) pi[32 + p] = frozen[p];
        if (fs->const_layout)
            for (int p = 0; p < 16; ++p) fs->const_val[0][p] = cst_val[pi[48 + p]];
        rw->permute_block(r, pi);
        fs->relabel_stage = r;
        if (fold_ok) {
            fs->fold5_stage = r;
        }
        rn_fold_block_register(h, r, pi);
        return;
    }
}

// stage-0 tables (s0_pixel_halves, rn_stage.h): A fragments with K = (ky, kx<4, c<4) of the folded weights 2^8 (2 w / 255) as fp16
// hi (cout rows 0..7) + lo (rows 8..15) pairs with the constant -2^8 sum(w) in the fourth channel slot of (ky, kx) = (0, 0); folded BN
static int prepare_stage0(rn_handle* h, FusedState* fs, const rn_weights* w) {
    if (h->stages[0].cin != 3 || h->stages[0].cout != S0_CO || h->stages[0].pool_k != 3 ||
        h->stages[0].pool_s != 1 || h->stages[0].skip_stage >= 0) {
        rn_set_error("16-bit path: stage 0 must be conv(3->8) + pool 3/1 (got %d->%d pool %d/%d)", h->stages[0].cin,
                     h->stages[0].cout, h->stages[0].pool_k, h->stages[0].pool_s);
        return RN_E_INVALID;
    }
    std::vector<unsigned short> frag(3 * 64 * 8, 0);
    const float* w0 = w->stages[0].kernel;       // [ky][kx][c][cout]
    for (int ky = 0; ky < 3; ++ky)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int kk = 8 * (l >> 5) + j, kx = kk / 4, c = kk % 4, row = l & 31, co = row & 7, part = row >> 3;
                if (part >= 2) continue;
                double v;
                if (kx < 3 && c < 3) {
                    v = static_cast<double>(w0[((ky * 3 + kx) * 3 + c) * S0_CO + co]) * (2.0 / 255.0) * S0_WSCALE;
                } else if (ky == 0 && kx == 0 && c == 3) {      // the constant slot: B = 1.0
                    v = 0.0;
                    for (int t = 0; t < 27; ++t) v -= static_cast<double>(w0[t * S0_CO + co]);
                    v *= S0_WSCALE;
                } else {
                    continue;
                }
                // the folded values live in fp16 hi + lo pairs: a checkpoint whose stage-0 weights (or their sum over the
                // 27 taps) reach 65504 / 2^8 = 255.9 would turn into infinities and NaN outputs without a word.  (Small
                // weights are safe: hi + lo resolves 2^-24 absolutely, below the fp32 ulp of any weight above 2^-1.)
                if (!(std::fabs(v) < 65504.0)) {
                    rn_set_error("16-bit path: stage-0 weight fold out of fp16 range (cout %d: |%g| >= 65504 after the 2^8 scale; "
                                 "conv2d/kernel must stay below ~255 per weight and per 27-tap sum) -- use RN_DTYPE_F32", co, v);
                    return RN_E_INVALID;
                }
                const unsigned short hi = f32_to_f16(static_cast<float>(v));
                const unsigned short lo = f32_to_f16(static_cast<float>(v - static_cast<double>(f16_to_f32(hi))));
                frag[(ky * 64 + l) * 8 + j] = part == 0 ? hi : lo;
            }
    const rn_conv_stage& ws = w->stages[0];
    std::vector<float> tab(16);
    for (int c = 0; c < S0_CO; ++c) {
        const float inv = rn_bn_inv(ws.variance[c], ws.gamma[c], w->bn_epsilon);
        tab[c] = inv / 9.0f / S0_WSCALE;
        tab[8 + c] = rn_bn_shift(ws.beta[c], ws.mean[c], inv);
    }
    i32x4* d_frag = nullptr;
    float* d_tab = nullptr;
    int rc;
    if ((rc = upload16(h, frag, &d_frag)) != RN_OK || (rc = upload(h, tab.data(), tab.size(), &d_tab)) != RN_OK) return rc;
    Stage0Args& a0 = fs->s0_args;
    a0.wfrag = d_frag;
    a0.ptab = d_tab;
    a0.S = h->stages[0].in_side;
    a0.So = h->stages[0].out_side;
    const int tiles = (a0.So + S0_TSTRIDE - 1) / S0_TSTRIDE;
    a0.npt = tiles >= 8 ? 8 : tiles;
    a0.n_colblocks = (tiles + a0.npt - 1) / a0.npt;
    return RN_OK;
}

// The one family of conv stage i >= 1.  Derived from the two chains this replaces -- six flags set one after the other, then a priority
// chain over them in the forward pass.  With  rw = rn_rw_supported && !GENERIC_KERNELS  and  row = rw && !PAIR_32X32  they set
//   use_rw = rw;  use_s6x = row && 6x;  use_c16 = rw && conv16 && !use_s6x;  use_s4x = row && 4x;  use_s5x = row && 5x;  use_c16p = rw && conv16p
// (4x, 5x, 6x, conv16, conv16p: the families' own *_supported predicates; 5x also needs the skip tensor to be the stage's own input,
// a first BN output: the kernel interpolates it from its input ring), and the forward pass took the first that held of
//   use_c16 | use_s5x, use_s4x, use_s6x (in this order: launch_rowreg's) | use_c16p | use_rw | generic.
// Without rw every flag is false: Generic.  With it, reading the priority chain from the top gives the lines below; RegWeights is what
// is left.  (The predicates accept disjoint shapes except conv16 / 6x, both the 64 -> 128 stage: the row-blocked kernel wins wherever its
// geometry allows.)  conv16 and conv16p take their one shape each (64 -> 128 unpooled, 128 -> 16) on shape alone, whatever the side and
// the flags, so RegWeights is never reached with them: rw_plan still answers for both (variants 5 and 6; its answer is rw_capable),
// and rn_rw_launch has no case for either.
static Family choose_family(const rn_handle* h, size_t i, bool rw_capable) {
    const StagePlan& s = h->stages[i];
    const bool res = s.skip_stage >= 0;
    if (!rw_capable) return Family::Generic;
    const bool row = !(h->flags & RN_FLAG_PAIR_32X32);
    const bool s6x = row && rn_stage6x_supported(s.cin, s.cout, s.pool_k, res, s.in_side);
    if (rn_conv16_supported(s.cin, s.cout, s.pool_k, res) && !s6x) return Family::Conv16;
    if (row && res && rn_stage5x_supported(s.cin, s.cout, s.pool_k, s.pool_s, true, s.in_side, s.skip_side) &&
        s.skip_stage == static_cast<int>(i) - 1 && h->stages[s.skip_stage].node_bn2 < 0)
        return Family::Row5x;
    if (row && rn_stage4x_supported(s.cin, s.cout, s.pool_k, s.pool_s, res, s.in_side)) return Family::Row4x;
    if (s6x) return Family::Row6x;
    if (rn_conv16p_supported(s.cin, s.cout, s.pool_k, s.pool_s, res)) return Family::Conv16P;
    return Family::RegWeights;
}

// The family's own fragments, and what the launch of stage i is told and rn_create knows without the activation buffers
// (rn_fused_post_alloc adds those): BN, skip and resize tables, rounding, the family's fragments, table and geometry.
static int bind_stage_args(rn_handle* h, const FusedState* fs, size_t i, FusedStage* f) {
    const StagePlan& s = h->stages[i];
    const int r = fs->relabel_stage - static_cast<int>(i);
    const float* wq = f->wq.data();
    // the skip source is the first BN output of the block (network.py:195-196)
    if (s.skip_stage >= 0 && h->stages[s.skip_stage].node_bn2 >= 0) {
        rn_set_error("16-bit path: skip source with its own residual is not supported");
        return RN_E_INVALID;
    }
    StageArgs& a = f->args;
    std::vector<unsigned short> frag;
    bool (*row_plan)(int, int*, int*, int*) = nullptr;
    switch (f->family) {
    case Family::Row4x: row_plan = rn_stage4x_plan; break;
    case Family::Row5x: row_plan = rn_stage5x_plan; break;
    case Family::Row6x: row_plan = rn_stage6x_plan; break;
    case Family::Conv16:
    case Family::Conv16P: break;
    case Family::Generic:
        a.n_colblocks = f->gen.n_colblocks;
        a.n_ctg = f->gen.n_ctg;
        a.npt = f->gen.npt;
        break;
    case Family::RegWeights:
        // `sixth` weights (/ 6, BN scale x 6) are only right for kernels that clamp to [0, 1]: the pool 4/1 variants of the
        // register-weights kernel and rn_stage4x / 5x.  Its stride-2 (DPP) variants clamp at 6.
        if (f->sixth && !(s.pool_k == 4 && s.pool_s == 1)) {
            rn_set_error("16-bit path: stage %zu has weights / 6 but would run a kernel that applies ReLU6 at 6", i);
            return RN_E_STATE;
        }
        a.skipcols = f->rw.skipcols;
        a.n_colblocks = f->rw.n_colblocks;
        a.npt = f->rw.npt;
        a.n_ctg = 1;
        break;
    }
    // the families on 16x16x32 tiles: K chunks of 32 (rn_pack.h)
    if (row_plan || f->conv16()) rn_pack_k32(wq, 9 * s.cin / 32, s.cout, h->dtype, &frag);
    if (int rc = frag.empty() ? RN_OK : upload16(h, frag, &f->family_wfrag)) return rc;
    if (f->conv16()) {
        f->c16 = Conv16Args{nullptr, nullptr, f->family_wfrag, f->ptab, s.in_side, s.in_side, s.out_side, s.out_side, 0, 0,
                            f->family == Family::Conv16P ? rn_conv16p_colblocks(s.out_side) : rn_conv16_colblocks(s.out_side)};
        return RN_OK;
    }
    a.wfrag = f->wfrag;
    a.ptab = f->ptab;
    a.bn_mean = s.bn.mean;
    a.bn_inv = s.bn.inv;
    a.bn_beta = s.bn.beta;
    if (s.skip_stage >= 0) {
        a.bn2_mean = s.bn2.mean;
        a.bn2_inv = s.bn2.inv;
        a.bn2_beta = s.bn2.beta;
        a.rlo = s.rt.lo;
        a.rhi = s.rt.hi;
        a.rlerp = s.rt.lerp;
        a.Ss = s.skip_side;
        a.rscale = static_cast<float>(s.skip_side) / static_cast<float>(s.out_side);
    }
    a.H = a.W = s.in_side;
    a.Ho = a.Wo = s.out_side;
    a.dither = fs->dither_out[i];
    // (both arms: the constant channels sit in the last quarter of the two relabelled tensors and keep the plain rounding)
    a.plain_q = fs->const_layout && (r == 0 || r == 1) ? 3 : -1;
    if (!row_plan) return RN_OK;
    if (!row_plan(s.out_side, &a.n_cb, a.cb_xo0, a.cb_wo)) {
        rn_set_error("stage %zu: no column-block plan for output side %d", i, s.out_side);
        return RN_E_STATE;
    }
    a.wfrag = f->family_wfrag;
    a.live_q = (f->family == Family::Row5x && static_cast<int>(i) == fs->fold5_stage) ? 2 : 4;
    return RN_OK;
}

// conv stage i >= 1: the kernel family that runs it, its folded BN table, its weight fragments and its launch arguments
static int prepare_stage(rn_handle* h, FusedState* fs, const rn_weights* w, size_t i) {
    StagePlan& s = h->stages[i];
    FusedStage& f = fs->st[i];
    const bool res = s.skip_stage >= 0;
    if (!rn_generic_plan(s.cin, s.cout, s.pool_k, s.pool_s, res, s.out_side, &f.gen)) {
        rn_set_error("16-bit path: no kernel variant for stage %zu (cin %d cout %d pool %d/%d res %d)", i, s.cin, s.cout, s.pool_k, s.pool_s, res);
        return RN_E_INVALID;
    }
    f.rw_capable = rn_rw_supported(s.cin, s.cout, s.pool_k, s.pool_s, res, s.out_side, s.skip_side, &f.rw) && !(h->flags & RN_FLAG_GENERIC_KERNELS);
    f.family = choose_family(h, i, f.rw_capable);
    if (f.family == Family::Generic && f.gen.lds_bytes > 160 * 1024) {
        rn_set_error("16-bit path: stage %zu needs %zu bytes of LDS", i, f.gen.lds_bytes);
        return RN_E_INVALID;
    }
    // Stages whose kernel pools fp16 ReLU6 outputs on the matrix cores (the pool 4/1 register-weights variants and the
    // cross-stage kernels built on them; rn_stage4x / rn_stage5x) store their conv weights divided by 6: the ReLU6 is
    // then the free [0, 1] clamp of the fp16 conversion (pack2_relu6_sixth) and the folded BN scale carries the 6.
    f.sixth = f.rw_capable && ((s.pool_k == 4 && s.pool_s == 1) || f.family == Family::Row4x || f.family == Family::Row5x);
    int rc;
    if (f.rw_capable) {
        f.tab = stage_table(w->stages[i], w->bn_epsilon, f.sixth);
        if ((rc = upload(h, f.tab.data(), f.tab.size(), &f.ptab)) != RN_OK) return rc;
    }
    // the weights every pack of this stage reads: HWIO == [k = tap*cin + c][cout], / 6 for `sixth` stages, with the refined rounding
    // when it is on (every pack below then converts exactly)
    f.wq.assign(w->stages[i].kernel, w->stages[i].kernel + static_cast<size_t>(9) * s.cin * s.cout);
    if (f.sixth)
        for (float& v : f.wq) v /= 6.0f;
    if (fs->refine) diffuse_taps(f.wq.data(), s.cin, s.cout, h->dtype);
    std::vector<unsigned short> frag;
    rn_generic_pack(f.wq.data(), s.cin, s.cout, h->dtype, &frag);
    if ((rc = upload16(h, frag, &f.wfrag)) != RN_OK) return rc;
    return bind_stage_args(h, fs, i, &f);
}

// ---- the 16 constant channels (const4) the relabelling put last: neither the stage in front of the residual stage nor the residual
// stage computes them, when both run on their row-blocked kernels (any other kernel family computes every channel)
static int prepare_const_channels(rn_handle* h, FusedState* fs) {
    const int r = fs->fold5_stage;
    if (fs->const4 && !(r >= 1 && r + 1 < static_cast<int>(fs->st.size()) && fs->st[r - 1].family == Family::Row4x && fs->st[r].family == Family::Row5x)) fs->const4 = false;
    if (!fs->const4) return RN_OK;
    FusedStage &f4 = fs->st[r - 1], &f5 = fs->st[r], &f6 = fs->st[r + 1];
    // the residual stage's output at the positions of the constant channels: y1 = fma(0, sc1', sh1') = sh1' (frozen first BN), the
    // bilinear resize of a constant channel is the constant (its two weights are exact 16-bit numbers that sum to 1, the products are
    // exact in float32), y = fma(v, sc2, y1) -- what rn_stage5x.hip computes for them
    for (int p = 0; p < 16; ++p)
        fs->const_val[1][p] = cv_store(std::fmaf(rn_from16(fs->const_val[0][p], h->dtype), f5.tab[2 * 64 + 48 + p], f5.tab[64 + 48 + p]), h->dtype);
    unsigned short* d_vals = nullptr;                // [2][16] on the device (StageArgs::cvals)
    int rc;
    if ((rc = upload(h, fs->const_val[0], 32, &d_vals)) != RN_OK) return rc;
    // a stage without its 16 constant input channels (positions 48..63; the residual stage: 15 fragments per cout quarter instead of
    // 18): fragments that leave them out -- they replace prepare_stage's, which stay allocated until rn_destroy: whether the fold
    // holds is known only when every stage has its family -- and what they add to every conv output, the accumulators' start value
    auto drop_inputs = [&](FusedStage& f, int cout, const unsigned short* vals) {
        std::vector<unsigned short> f16;
        rn_pack_k48(f.wq.data(), cout, h->dtype, &f16);
        if (int e = upload16(h, f16, &f.family_wfrag)) return e;
        const std::vector<float> cst = const_sum48(f.wq.data(), cout, vals, h->dtype);
        float* d_cst = nullptr;
        if (int e = upload(h, cst.data(), cst.size(), &d_cst)) return e;
        f.args.wfrag = f.family_wfrag;
        f.args.cstart = d_cst;
        return static_cast<int>(RN_OK);
    };
    f4.args.live_q = 3;                  // its last cout quarter is constant
    f4.args.cvals = d_vals;
    if ((rc = drop_inputs(f5, 64, fs->const_val[0])) != RN_OK) return rc;
    f5.args.cvals = d_vals + 16;
    // the stage behind it likewise: the residual stage's output channels 48..63 are constants (const5_val)
    if (f6.family == Family::Row6x) return drop_inputs(f6, 128, fs->const_val[1]);
    return RN_OK;
}

// ---- cross-stage fusion: the last two steps of a depth-3 block (network.py:183-203 with block_depth = 3):
// stage i (32->32, pool 4/1) feeds only stage i+1 (32->32, pool 4/1 + residual), whose skip tensor is stage i's
// INPUT.  One kernel runs both; stage i's output never reaches HBM.
static int prepare_pair(rn_handle* h, FusedState* fs) {
    if (h->flags & (RN_FLAG_STAGE_LAUNCHES | RN_FLAG_GENERIC_KERNELS)) return RN_OK;
    for (size_t i = 2; i + 1 < h->stages.size(); ++i) {
        const StagePlan& s1 = h->stages[i];
        const StagePlan& s2 = h->stages[i + 1];
        auto is3232 = [](const StagePlan& s) { return s.cin == 32 && s.cout == 32 && s.pool_k == 4 && s.pool_s == 1; };
        if (!is3232(s1) || !is3232(s2) || s1.skip_stage >= 0 || s2.skip_stage != static_cast<int>(i) - 1) continue;
        if (!fs->st[i].rw_capable || !fs->st[i + 1].rw_capable || !rn_stage23_supported(s1.in_side)) continue;
        bool feeds_others = false;      // stage i's output must have no other consumer
        for (size_t k = i + 2; k < h->stages.size(); ++k) feeds_others |= h->stages[k].skip_stage == static_cast<int>(i);
        if (feeds_others) continue;
        const std::vector<float>& t1 = fs->st[i].tab;
        const std::vector<float>& t2 = fs->st[i + 1].tab;
        std::vector<float> tab(5 * 32);
        std::copy(t1.begin(), t1.begin() + 64, tab.begin());
        std::copy(t2.begin(), t2.begin() + 96, tab.begin() + 64);
        // the launch arguments: what both kernels of the pair are told; the round-2 kernel (rn_stage23.hip) takes the stages' own
        // fragments and computes every channel ...
        Stage23Args& fa = fs->pair_args;
        fa.dither = fs->dither_out[i + 1];
        fa.rlo = s2.rt.lo;
        fa.rhi = s2.rt.hi;
        fa.rlerp = s2.rt.lerp;
        fa.rscale = static_cast<float>(s2.skip_side) / static_cast<float>(s2.out_side);
        fa.W = s1.in_side;
        fa.Wo = s2.out_side;
        if (!rn_stage23_plan(s1.in_side, &fa.n_cblocks, fa.cb_x0, fa.cb_wo)) {
            rn_set_error("fused stage pair: no column-block plan for input side %d", s1.in_side);
            return RN_E_STATE;
        }
        float* d_tab = nullptr;
        int rc;
        if ((rc = upload(h, tab.data(), tab.size(), &d_tab)) != RN_OK) return rc;
        fa.wfrag2 = fs->st[i].wfrag;
        fa.wfrag3 = fs->st[i + 1].wfrag;
        fa.ptab = d_tab;
        fa.producer_halves = 2;
        fs->pair_first = static_cast<int>(i);
        if (h->flags & RN_FLAG_PAIR_32X32) return RN_OK;
        // ... rn_stage23x.hip: fragments and a table of its own, frozen channels left out
        // ---- frozen channels of the pair's on-chip tensor B (the first stage's output).  The epilogue stores
        // to16(fma(H, sc, sh)) with H = a sum of 16 ReLU6 / 6 values in [0, 16]: where |sc| * 16 < 2^-25 |sh| the fma
        // returns sh EXACTLY in float32 for every H the convolution can produce -- the channel is the constant to16(sh)
        // whatever the image, in this kernel's arithmetic bit for bit (and to 1e-10 of an O(1) tensor in the reference's
        // float32, where the same product vanishes against the same addend).  The shipped checkpoint has 18 such channels
        // of 32 (its L2 regulariser drove their BN gamma to ~1e-20): with >= 16 of them the first conv computes half of
        // its couts.  perm[p] = the channel at B-ring position p; the positions (p & 7) >= 4 -- the second half of every
        // 8-cout group -- take frozen channels.
        // Both convs' weights are the stages' own (pool 4/1 stages: / 6, with the handle's refined rounding when it is on): every use
        // below -- the two fragment packs and the frozen channels' constant -- reads THESE arrays
        const std::vector<float>* wq[2] = {&fs->st[i].wq, &fs->st[i + 1].wq};
        int perm[32];
        {
            // Round 6: the criterion is the tensor's 16-BIT STORE (as for the constant quarter of the 64-channel block): the
            // channel is constant when the two ends of the pooled sum's range, H = 0 and H = 16, store the same 16-bit number
            // (fma and the conversion are monotone in H) -- every channel whose fma returns its addend in float32 (round 5's
            // criterion: 18 on the shipped checkpoint) and those whose scale is below half an ulp of the shift (26 in bf16,
            // 25 in fp16).  With >= 24 of them the ring holds EIGHT channels (live ones at positions 0..3, 8..11: the lane
            // groups 0, 1 of the producer's half), with >= 16 sixteen (positions (p & 7) < 4).
            std::vector<int> frozen, live;
            for (int c = 0; c < 32; ++c) {
                const float sc = t1[c], sh = t1[32 + c];
                const bool fz = std::isfinite(sh) && rn_to16(std::fmaf(0.0f, sc, sh), h->dtype) == rn_to16(std::fmaf(16.0f, sc, sh), h->dtype);      // (the B ring's store: round to nearest even)
                (fz ? frozen : live).push_back(c);
            }
            fs->pair_frozen = static_cast<int>(frozen.size());
            const bool fold_pair = !(h->flags & RN_FLAG_COMPUTE_FROZEN);
            fa.producer_halves = (frozen.size() >= 16 && fold_pair) ? 1 : 2;
            fa.narrow_b = fa.producer_halves == 1 ? (frozen.size() >= 24 ? 2 : 1) : 0;
            const int n_fold = fa.narrow_b == 2 ? 24 : 16;
            const auto live_pos = [&](int p) { return fa.narrow_b == 2 ? ((p & 7) < 4 && p < 16) : (p & 7) < 4; };
            if (fa.producer_halves == 1) {
                while (static_cast<int>(frozen.size()) > n_fold) {             // the spare constant channels are computed like live ones
                    live.push_back(frozen.back());
                    frozen.pop_back();
                }
                std::sort(live.begin(), live.end());
                size_t nl = 0, nf = 0;
                for (int p = 0; p < 32; ++p) perm[p] = live_pos(p) ? live[nl++] : frozen[nf++];
            } else {
                for (int p = 0; p < 32; ++p) perm[p] = p;
            }
            std::vector<float> tabx(tab);
            tabx.resize(6 * 32, 0.f);
            for (int p = 0; p < 32; ++p) {
                tabx[p] = t1[perm[p]];
                tabx[32 + p] = t1[32 + perm[p]];
            }
            if (fa.producer_halves == 1) {
                // row 5: what the 16 frozen channels (B positions (p & 7) >= 4) add to every output of the second conv, channel by
                // channel (the stored value: the kernels' own store)
                std::vector<ConstTerm> terms;
                for (int p = 0; p < 32; ++p) {
                    if (live_pos(p)) continue;
                    const double val = rn_from16(rn_to16(t1[32 + perm[p]], h->dtype), h->dtype);
                    for (int tap = 0; tap < 9; ++tap) terms.push_back({static_cast<size_t>(tap) * 32 + perm[p], val});
                }
                const std::vector<float> cst = const_sum(wq[1]->data(), 32, terms, h->dtype);
                std::copy(cst.begin(), cst.end(), tabx.begin() + 160);
            }
            if ((rc = upload(h, tabx.data(), tabx.size(), &d_tab)) != RN_OK) return rc;
            fa.ptab = d_tab;
        }
        for (int which = 0; which < 2; ++which) {
            std::vector<unsigned short> f16;
            std::vector<float> w6(static_cast<size_t>(9) * 32 * 32);
            const float* wsrc6 = wq[which]->data();                  // [tap][cin][cout]
            for (int tap = 0; tap < 9; ++tap)
                for (int ci = 0; ci < 32; ++ci)
                    for (int co = 0; co < 32; ++co)
                        w6[(static_cast<size_t>(tap) * 32 + ci) * 32 + co] =
                            which == 0 ? wsrc6[(static_cast<size_t>(tap) * 32 + ci) * 32 + perm[co]]        // B's channels = the first conv's couts
                                       : wsrc6[(static_cast<size_t>(tap) * 32 + perm[ci]) * 32 + co];       // ... and the second conv's cins
            if (which == 1 && fa.producer_halves == 1) {
                int ring_cin[16];
                for (int r = 0; r < 16; ++r) ring_cin[r] = perm[8 * (r >> 2) + (r & 3)];       // (eight-channel ring: r < 8)
                if (fa.narrow_b == 2)
                    rn_stage23x_pack_narrow8(wsrc6, ring_cin, h->dtype, &f16);
                else
                    rn_stage23x_pack_narrow(wsrc6, ring_cin, h->dtype, &f16);
            } else
                rn_stage23x_pack(w6.data(), h->dtype, &f16);
            i32x4* d_frag = nullptr;
            if ((rc = upload16(h, f16, &d_frag)) != RN_OK) return rc;
            (which ? fa.wfrag3 : fa.wfrag2) = d_frag;
        }
        fs->pair_x16 = true;
        return RN_OK;
    }
    return RN_OK;
}

// stage 0 inside stage 1's kernel (network.py:226 feeding :227's first step), the last two stages + head in one launch, the whole back
// end in one launch
static void plan_fusion(const rn_handle* h, FusedState* fs) {
    const size_t ns = h->stages.size();
    if (!(h->flags & (RN_FLAG_STAGE_LAUNCHES | RN_FLAG_GENERIC_KERNELS)) && ns > 1) {
        // the 8-channel register-weights variant computes stage 0 for its own ring columns
        bool feeds_others = false;
        for (size_t k = 2; k < ns; ++k) feeds_others |= h->stages[k].skip_stage == 0;
        FusedStage& f1 = fs->st[1];
        fs->fuse_s0 = f1.family == Family::RegWeights && f1.rw.variant == 0 && h->stages[1].skip_stage < 0 && !feeds_others;
        if (fs->fuse_s0) {
            StageArgs& a = f1.args;      // (s0_bgr is the call's image batch)
            a.s0_wfrag = fs->s0_args.wfrag;
            a.s0_ptab = fs->s0_args.ptab;
            a.s0_S = h->stages[0].in_side;
            a.s0_private = (h->flags & RN_FLAG_PAIR_32X32) ? 1 : 0;
            // the shared-ring form of the fused stages 0 + 1 cuts rows into 227-column blocks (eight 29-column tiles - 5 halo columns)
            if (!a.s0_private && f1.rw.npt == 8) a.n_colblocks = rn_rw_s0sh_colblocks(h->stages[1].out_side);
        }
    }
    fs->use_tail = !(h->flags & (RN_FLAG_STAGE_LAUNCHES | RN_FLAG_GENERIC_KERNELS)) && rn_tail_supported(h);
    fs->use_backend = fs->use_tail && !(h->flags & RN_FLAG_PAIR_32X32) && ns >= 5 && rn_backend_supported(h) &&
                      fs->st[ns - 4].family == Family::Row6x && fs->st[ns - 3].family == Family::Conv16P;
}

int rn_fused_prepare(rn_handle* h, const rn_weights* w_in) {
    auto* fs = new FusedState();
    fs->st.resize(h->stages.size());
    h->fused = fs;
    plan_dither(h, fs);
    RelabelledWeights rw(w_in);
    fold16(h, fs, w_in, &rw);
    const rn_weights* const w = &rw.w;
    int rc;
    if ((rc = prepare_stage0(h, fs, w)) != RN_OK) return rc;
    for (size_t i = 1; i < h->stages.size(); ++i)
        if ((rc = prepare_stage(h, fs, w, i)) != RN_OK) return rc;
    if ((rc = prepare_const_channels(h, fs)) != RN_OK) return rc;
    if ((rc = prepare_pair(h, fs)) != RN_OK) return rc;
    plan_fusion(h, fs);
    const int ns = static_cast<int>(h->stages.size());
    for (int i = 0; i < ns; ++i) fs->launch_rep.push_back(i);
    if (fs->fuse_s0) fs->launch_rep[0] = 1;
    if (fs->use_tail) fs->launch_rep[ns - 2] = ns - 1;
    if (fs->pair_first >= 0) fs->launch_rep[fs->pair_first] = fs->pair_first + 1;
    return RN_OK;
}

void rn_fused_frozen_info(const rn_handle* h, int info[4]) {
    const FusedState* fs = static_cast<const FusedState*>(h->fused);
    info[0] = info[1] = 0;
    info[2] = -1;
    info[3] = 4;
    if (!fs) return;
    info[0] = fs->pair_x16 && fs->pair_args.producer_halves == 1 ? (fs->pair_args.narrow_b == 2 ? 24 : 16) : 0;
    info[1] = fs->pair_frozen;
    info[2] = fs->fold5_stage;
    info[3] = fs->fold5_stage >= 0 ? 2 : 4;
}

void rn_fused_const_info(const rn_handle* h, int info[4]) {
    const FusedState* fs = static_cast<const FusedState*>(h->fused);
    info[0] = -1;
    info[1] = info[2] = info[3] = 0;
    if (!fs || fs->fold5_stage < 1) return;
    info[1] = fs->const4_proven;
    if (!fs->const4) return;
    info[0] = fs->fold5_stage - 1;
    info[2] = 16;
    info[3] = 48;
}

namespace {
// channels c0 .. c0 + 15 of a [npix, 64] 16-bit tensor <- vals[0..15]
__global__ void fill_channels16_kernel(unsigned short* base, int64_t npix, int c0, const i32x4 v0, const i32x4 v1) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    i32x4* dst = reinterpret_cast<i32x4*>(base + p * 64 + c0);
    dst[0] = v0;
    dst[1] = v1;
}
}  // namespace

// After alloc_buffers, which fixes the node pointers: the launch arguments get their tensors; the constant channels of the two tensors
// nobody computes (const4) are written once, for every image slot of the handle; the kernels never touch these positions again, rn_tap
// and the consumers read complete tensors.
int rn_fused_post_alloc(rn_handle* h) {
    FusedState* fs = static_cast<FusedState*>(h->fused);
    if (!fs) return RN_OK;
    auto out_of = [&](const StagePlan& s) { return static_cast<unsigned short*>(h->nodes[rn_stage_out_node(s)].ptr); };
    fs->s0_args.out = out_of(h->stages[0]);
    for (size_t i = 1; i < h->stages.size(); ++i) {
        const StagePlan& s = h->stages[i];
        FusedStage& f = fs->st[i];
        const bool c16 = f.conv16();
        (c16 ? f.c16.in : f.args.in) = out_of(h->stages[i - 1]);
        (c16 ? f.c16.out : f.args.out) = out_of(s);
        if (!c16 && s.skip_stage >= 0) f.args.skip = static_cast<const unsigned short*>(h->nodes[h->stages[s.skip_stage].node_bn].ptr);
        if (static_cast<int>(i) == fs->pair_first) fs->pair_args.in = f.args.in;
        if (static_cast<int>(i) == fs->pair_first + 1 && fs->pair_first >= 0) fs->pair_args.out = f.args.out;
    }
    if (!fs->const4) return RN_OK;
    const int r = fs->fold5_stage;
    const StagePlan& s4 = h->stages[r - 1];
    const StagePlan& s5 = h->stages[r];
    struct Job { int node; int side; const unsigned short* vals; };
    const Job jobs[2] = {{s4.node_bn, s4.out_side, fs->const_val[0]}, {s5.node_bn2, s5.out_side, fs->const_val[1]}};
    for (const Job& j : jobs) {
        unsigned short* base = static_cast<unsigned short*>(h->nodes[j.node].ptr);
        if (!base) {
            rn_set_error("constant channels: node %d has no buffer", j.node);
            return RN_E_STATE;
        }
        i32x4 v[2];
        std::memcpy(v, j.vals, 32);
        const int64_t npix = static_cast<int64_t>(h->max_batch) * j.side * j.side;
        hipLaunchKernelGGL(fill_channels16_kernel, dim3(static_cast<unsigned>((npix + 255) / 256)), dim3(256), 0, h->stream, base, npix, 48, v[0], v[1]);
        RN_CHECK_LAUNCH();
    }
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

// true when the stage's output tensor is never written to HBM on this handle (it lives in LDS inside a fused launch)
bool rn_fused_stage_elided(const rn_handle* h, int stage) {
    const FusedState* fs = static_cast<const FusedState*>(h->fused);
    if (!fs) return false;
    const int ns = static_cast<int>(h->stages.size());
    if (fs->last_backend && (stage == ns - 4 || stage == ns - 3)) return true;
    return (fs->fuse_s0 && stage == 0) || (fs->pair_first >= 0 && stage == fs->pair_first);
}

int rn_fused_launch_rep(const rn_handle* h, int stage) {
    const FusedState* fs = static_cast<const FusedState*>(h->fused);
    if (!fs || stage < 0 || stage >= static_cast<int>(fs->launch_rep.size())) return stage;
    const int ns = static_cast<int>(fs->launch_rep.size());
    if (fs->last_backend && stage >= ns - 4) return ns - 1;      // (the last forward pass ran stage 6 .. head as one launch)
    return fs->launch_rep[stage];
}

// ---- the launch steps of a forward pass: each copies its bound arguments with what depends on the call -- the bands of this batch size
// from the band picker (rn_bands.h), the clock region, the image pointer -- and launches.  rn_fused_forward decides which one runs.
namespace {

int launch_stage0(const rn_handle* h, const FusedState* fs, const uint8_t* d_bgr, int n) {
    Stage0Args a0 = with_bands(fs->s0_args, rn_bands_stage0(n, fs->s0_args.So, fs->s0_args.n_colblocks));
    a0.bgr = d_bgr;
    return rn_stage0_launch(h->dtype, h->stream, a0, n);
}

// stage 6 .. head in one launch
int launch_backend(rn_handle* h, const FusedState* fs, int n, float* d_probs, int64_t* d_ids) {
    const size_t ns = h->stages.size();
    HeadArgs head;
    rn_fill_head_args(h, &head);
    const StageArgs& a6 = fs->st[ns - 4].args;      // (plan_fusion sets use_backend only where stage 6 is Row6x, stage 7 Conv16P)
    const Conv16Args& a7 = fs->st[ns - 3].c16;
    return rn_backend_launch(h, a6.wfrag, a6.ptab, a6.cstart, a7.wfrag, a7.ptab, fs->st[ns - 2].wfrag, fs->st[ns - 1].wfrag, head, n, d_probs, d_ids);
}

// the last two stages (i, i + 1), the flatten, the dense head, softmax and argmax in one launch
int launch_tail(rn_handle* h, const FusedState* fs, size_t i, int n, float* d_probs, int64_t* d_ids) {
    HeadArgs head;
    rn_fill_head_args(h, &head);
    return rn_tail_launch(h, fs->st[i].wfrag, fs->st[i + 1].wfrag, head, n, d_probs, d_ids);
}

// both stages of the pair in one launch
int launch_pair(const rn_handle* h, const FusedState* fs, int n) {
    Stage23Args fa = with_bands(fs->pair_args, rn_bands_pair(n, h->n_cu, fs->pair_args.Wo, fs->pair_args.n_cblocks));
    if (fs->pair_x16) fa.stamp_buf = rn_clock_region("stages 2+3", static_cast<size_t>(fa.n_bands) * fa.n_cblocks * n);
#ifdef RN_ROUND2_ARMS
    return fs->pair_x16 ? rn_stage23x_launch(h->dtype, h->stream, fa, n) : rn_stage23_launch(h->dtype, h->stream, fa, n);
#else
    // (the round-2 pair kernel, rn_stage23.hip, is part of the test / A-B library only: rn_create refuses RN_FLAG_PAIR_32X32 here)
    return rn_stage23x_launch(h->dtype, h->stream, fa, n);
#endif
}

// rn_conv16 (the un-pooled 64 -> 128 stage) and its pooled sibling rn_conv16p (128 -> 16 with avg-pool 4/2)
int launch_conv16(const rn_handle* h, const FusedStage& f, int n) {
    const bool pooled = f.family == Family::Conv16P;
    const Bands b = rn_bands_conv16(n, h->n_cu, f.c16.Ho, f.c16.n_colblocks, pooled ? rn_conv16p_wgs_per_cu(f.c16.Ho) : 2, pooled);
    const Conv16Args ca = with_bands(f.c16, b);
    return pooled ? rn_conv16p_launch(h->dtype, h->stream, ca, n) : rn_conv16_launch(h->dtype, h->stream, ca, n);
}

// the row-register kernels: rn_stage4x (32 -> 64), rn_stage5x (64 -> 64 residual), rn_stage6x (64 -> 128)
int launch_rowreg(const rn_handle* h, const FusedStage& f, size_t i, int n) {
    StageArgs a = with_bands(f.args, rn_bands_rowreg(n, h->n_cu, f.args.Ho, f.args.n_cb, h->stages[i].pool_k != 0));
    char what[32];
    snprintf(what, sizeof what, "stage %d", static_cast<int>(i));
    a.stamp_buf = rn_clock_region(what, static_cast<size_t>(a.n_bands) * a.n_cb * n);
    if (f.family == Family::Row5x) return rn_stage5x_launch(h->dtype, h->stream, a, n);
    if (f.family == Family::Row4x) return rn_stage4x_launch(h->dtype, h->stream, a, n);
    return rn_stage6x_launch(h->dtype, h->stream, a, n);
}

// the register-weights kernels (rn_stage_rw.hip); stage 1 computes stage 0 too when the handle fuses them
int launch_regweights(const rn_handle* h, const FusedState* fs, size_t i, const uint8_t* d_bgr, int n) {
    const StagePlan& s = h->stages[i];
    const FusedStage& f = fs->st[i];
    StageArgs a = with_bands(f.args, rn_bands_rw(n, h->n_cu, s.out_side, f.args.n_colblocks, f.rw.wgs_per_cu, s.pool_k, s.pool_s));
    if (i == 1 && fs->fuse_s0) a.s0_bgr = d_bgr;
    dim3 grid(a.n_bands * a.n_colblocks, n);
    char what[32];
    snprintf(what, sizeof what, a.s0_bgr ? "stages 0+%zu" : "stage %zu", i);
    a.stamp_buf = rn_clock_region(what, static_cast<size_t>(grid.x) * grid.y);
    return rn_rw_launch(f.rw, h->dtype, h->stream, a, grid);
}

int launch_generic(const rn_handle* h, const FusedStage& f, int n) {
    const StageArgs a = with_bands(f.args, rn_bands_generic(n, f.args.Ho, f.args.n_colblocks * f.args.n_ctg));
    return rn_generic_launch(f.gen, h->dtype, h->stream, a, n);
}

}  // namespace

int rn_fused_forward(rn_handle* h, const uint8_t* d_bgr, const float* d_rgb, int n, float* d_probs,
                     int64_t* d_ids) {
    if (!d_bgr || d_rgb) {
        rn_set_error("16-bit handles take uint8 BGR input (the pre-processing is folded into stage 0's weights)");
        return RN_E_STATE;
    }
    FusedState* fs = static_cast<FusedState*>(h->fused);
    if (!fs) {
        rn_set_error("fused plan missing");
        return RN_E_STATE;
    }
    // The events are the rn_timing / rn_stage_launch contract: slot 2 + i closes stage i, slot 2 + ns the head.  A fused launch
    // is reported under its last stage: the events of the stages in front of it are recorded before the launch and read ~0.
    const size_t ns = h->stages.size();
    auto event = [&](size_t stage) { rn_record_event(h, 2 + static_cast<int>(stage)); };
    int rc;
    rn_clock_begin();
    // stage 0 (a launch of its own unless stage 1's kernel computes it)
    if (!fs->fuse_s0 && (rc = launch_stage0(h, fs, d_bgr, n)) != RN_OK) return rc;
    event(0);
    bool head_done = false;
    for (size_t i = 1; i < ns && !head_done; ++i) {
        const FusedStage& f = fs->st[i];
        if (fs->use_backend && !h->split_backend && i + 4 == ns && 2 * n >= h->n_cu) {
            for (size_t k = i; k + 1 < ns; ++k) event(k);
            if ((rc = launch_backend(h, fs, n, d_probs, d_ids)) != RN_OK) return rc;
            fs->last_backend = true;         // (only now: a failed launch must not report s6.bn / s7.bn as elided)
            event(ns - 1);
            head_done = true;
            continue;
        }
        fs->last_backend = false;
        if (fs->use_tail && i + 2 == ns) {
            event(i);
            if ((rc = launch_tail(h, fs, i, n, d_probs, d_ids)) != RN_OK) return rc;
            event(i + 1);
            head_done = true;
            continue;
        }
        if (static_cast<int>(i) == fs->pair_first) {
            event(i);
            if ((rc = launch_pair(h, fs, n)) != RN_OK) return rc;
            event(++i);
            continue;
        }
        switch (f.family) {
        case Family::Conv16:
        case Family::Conv16P: rc = launch_conv16(h, f, n); break;
        case Family::Row4x:
        case Family::Row5x:
        case Family::Row6x: rc = launch_rowreg(h, f, i, n); break;
        case Family::RegWeights: rc = launch_regweights(h, fs, i, d_bgr, n); break;
        case Family::Generic: rc = launch_generic(h, f, n); break;
        }
        if (rc != RN_OK) return rc;
        event(i);
    }
    if (!head_done && (rc = rn_run_head(h, n, d_probs, d_ids)) != RN_OK) return rc;
    event(ns);
    rn_clock_end(h->stream);
    return RN_OK;
}

// the band picker of the launch steps above (and of rn_f32m_launch), exported for tests
extern "C" int rn_band_plan(int family, int n, int n_cu, int out_side, int n_colblocks, int wgs_per_cu, int pool_k, int pool_s,
                            int* rows_per_band, int* n_bands) {
    Bands b;
    if (n < 1 || n_cu < 1 || out_side < 1 || n_colblocks < 1 || wgs_per_cu < 1 || pool_k < 0 || pool_s < 1 || !rows_per_band || !n_bands ||
        !rn_bands_family(family, n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s, &b)) {
        rn_set_error("rn_band_plan: bad argument (family %d, n %d, n_cu %d, out_side %d, n_colblocks %d, wgs_per_cu %d, pool %d/%d)", family, n, n_cu,
                     out_side, n_colblocks, wgs_per_cu, pool_k, pool_s);
        return RN_E_INVALID;
    }
    *rows_per_band = b.rows_per_band;
    *n_bands = b.n_bands;
    return RN_OK;
}
