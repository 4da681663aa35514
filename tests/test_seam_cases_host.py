"""CPU checks of the cases tests/test_hip_seams_live.py runs: on the float64 oracle alone they show that those cases can see what
they are meant to see.

The tuned 16-bit kernels cut wide rows into column blocks (tests/block_plans.py).  At side 224 every family runs one block; at
CK.SEAM_SIDES they run two or three, at CK.FOUR_BLOCK_SIDES stage 6 (630) and stages 5 and 6 (686, the flatten at the head's limit
of 4096) run four.  What can be wrong there and still pass at 224: a block's first output column, the window
taps that reach over a seam, a lerp table indexed with the column inside the block.  The GPU cases judge every stage against
float64 on the `live` checkpoint with the two images CK.SEAM_IDX.  Asserted here:
  - the block plans of every side, pinned, and what the float32 planner and the band planner say next to them; the block counts
    of every side from 183 to 694, the largest whose flatten fits the head (no four-block pair or stage 4 among them);
  - clamp reach: the two images together meet AT_CLAMP_MIN / INSIDE_MIN in every stage 1-9 at every side (image 30 does on its own);
  - spatial sensitivity: image 14 differs between ANY two neighbouring columns, and rows, of every stage output by at least
    4 x STAGE_TOL["bf16"] of the tensor's abs-max -- and image 30 alone, a checkerboard of period 32, by less than STAGE_TOL["f16"] in
    stages 0-4: with that image alone a duplicated column passes;
  - seam mutants: three ways a block seam goes wrong, applied in NumPy to the float64 tensors at the seam columns the plans give,
    move the tensor by more than twice what the GPU test tolerates;
  - the shared check itself (stage_ref.check_stage_local): on a stand-in handle it names a duplicated column, lazy form and eager form.
One float64 oracle run of the two images per side (3 s at 224, 20 s at 600, 13-15 s at 630 and 686) is shared by all of it, reduced to the figures."""
import numpy as np
import pytest

import block_plans as BP
import checkpoints as CK
import stage_ref as SR
from conftest import parity_set_of
from oracle import roomnet_ref as R
from parity_bounds import AT_CLAMP_MIN, INSIDE_MIN, STAGE_TOL
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph

ALL_SIDES = (224, 240) + CK.SEAM_SIDES + CK.FOUR_BLOCK_SIDES
PLANNED_SIDES = CK.SEAM_SIDES + CK.FOUR_BLOCK_SIDES       # the sides whose plans are pinned and whose seams get mutants
MIN_SIDE, MAX_HEAD_SIDE, HEAD_MAX_FLAT = 183, CK.MAX_HEAD_SIDE, 4096# build_graph's smallest side; the largest whose flatten fits head_kernel
# side -> blocks of the stage pair, of stage 4, 5, 6 (0: the row-blocked kernel does not take the side, another kernel runs)
BLOCK_COUNTS = {224: (1, 1, 1, 1), 240: (0, 0, 1, 0), 409: (2, 2, 2, 2), 420: (2, 2, 2, 2), 600: (3, 3, 3, 3),
                630: (3, 3, 3, 4), 686: (0, 0, 4, 4)}
BLOCK_PLANS = {
    409: {"pair": [(0, 195), (195, 195)], 4: [(0, 97), (97, 96)], 5: [(0, 47), (47, 47)], 6: [(0, 46), (46, 46)]},
    # the pair's blocks unequal, stage 6 at its widest block (48 columns: three full 16-pixel tiles)
    420: {"pair": [(0, 201), (201, 200)], 4: [(0, 99), (99, 99)], 5: [(0, 49), (49, 48)], 6: [(0, 48), (48, 47)]},
    600: {"pair": [(0, 194), (194, 194), (388, 193)], 4: [(0, 96), (96, 96), (192, 96)], 5: [(0, 48), (48, 47), (95, 47)],
          6: [(0, 47), (47, 47), (94, 46)]},
    # stage 6 in four blocks with a ragged last one, next to three-block plans of the other families
    630: {"pair": [(0, 204), (204, 204), (408, 203)], 4: [(0, 101), (101, 101), (202, 101)], 5: [(0, 50), (50, 50), (100, 49)],
          6: [(0, 37), (37, 37), (74, 37), (111, 36)]},
    # flatten 4096: stages 5 and 6 in four blocks; the pair and stage 4 have no plan (their rows would need blocks below the minimum)
    686: {"pair": None, 4: None, 5: [(0, 41), (41, 41), (82, 41), (123, 40)], 6: [(0, 41), (41, 40), (81, 40), (121, 40)]},
}
# first side .. last side -> BLOCK_COUNTS of every side in between, where any family reaches four blocks (the whole range up to the
# head's limit: test_block_counts_of_every_side_up_to_the_heads_limit)
FOUR_BLOCK_RANGES = {(619, 630): (3, 3, 3, 4), (631, 634): (3, 0, 3, 4), (635, 670): (0, 0, 3, 4), (671, 694): (0, 0, 4, 4)}
# rn_f32m_plan's n_colblocks of stages 1-8 (the float32 matrix-core kernels cut rows by their own tile counts)
F32M_COLBLOCKS = {409: [2, 2, 2, 2, 3, 1, 3, 1], 420: [2, 2, 2, 2, 3, 1, 3, 1], 600: [3, 3, 3, 3, 4, 2, 4, 1],
                  630: [3, 3, 3, 3, 4, 2, 4, 1], 686: [3, 3, 3, 3, 4, 2, 4, 1]}
SEAM_STAGES = (3, 4, 5, 6)            # the stage whose stored output carries each family's seams (3: the pair's)
DROPPED_TAP = (0, 0)                  # mutant B: the window's first tap, the one that reaches furthest over the seam
CONTRAST_MIN = 4 * STAGE_TOL["bf16"]
MUTANT_FACTOR = 2.0


def _contrast(t):
    """Neighbour contrast of one image's stage output [h, w, c]: per adjacent column pair the largest |difference| over rows and
    channels, relative to the tensor's abs-max; the minimum over all pairs.  The same for rows."""
    m = float(np.abs(t).max())
    return (float(np.abs(np.diff(t, axis=1)).max(axis=(0, 2)).min() / m), float(np.abs(np.diff(t, axis=0)).max(axis=(1, 2)).min() / m))


def _mutants(g, w, taps, k, x0):
    """rel_err of stage k's output with its column x0 mutated, against the unmutated tensor."""
    s = g.stages[k]
    out = taps[SR.stage_out_name(s)]

    def bn(x, name):
        return R.fused_batch_norm_infer(x, *SR._bn(w, name))

    def err(col):
        m = out.copy()
        m[:, :, x0] = col
        return SR.rel_err(m, out)

    res = {"A": err(out[:, :, x0 - 1])}                 # (A) the block's first column stored from its left neighbour
    if s.pool_k:                                        # (B) one of the 16 window taps dropped at that column
        conv, ps, ho = taps["s%d.conv" % k], s.pool_s, out.shape[1]
        win = conv[:, :, ps * x0:ps * x0 + 4]
        rows = lambda ky: slice(ky, ky + (ho - 1) * ps + 1, ps)
        pooled = sum(win[:, rows(ky), kx] for ky in range(4) for kx in range(4)) / 16.0
        assert np.abs(pooled - taps["s%d.pool" % k][:, :, x0]).max() <= 1e-12
        col = bn(pooled - win[:, rows(DROPPED_TAP[0]), DROPPED_TAP[1]] / 16.0, s.bn_name)
        if s.residual:
            col = bn(col + (taps["s%d.add" % k][:, :, x0] - taps["s%d.bn" % k][:, :, x0]), s.bn2_name)
        res["B"] = err(col)
    if s.residual:                                      # (C) fraction and source columns from the column inside the block
        skip = taps[SR.stage_out_name(g.stages[s.skip_stage])]
        ylo, yhi, yl = R.resize_tables(skip.shape[1], out.shape[1])
        xlo, xhi, xl = R.resize_tables(skip.shape[2], out.shape[2])
        yl = yl.astype(np.float64)[None, :, None]

        def column(lo, hi, f):
            top = skip[:, ylo, lo] + (skip[:, ylo, hi] - skip[:, ylo, lo]) * f
            bottom = skip[:, yhi, lo] + (skip[:, yhi, hi] - skip[:, yhi, lo]) * f
            return bn(taps["s%d.bn" % k][:, :, x0] + (top + (bottom - top) * yl), s.bn2_name)

        assert np.abs(column(xlo[x0], xhi[x0], float(xl[x0])) - out[:, :, x0]).max() <= 1e-12
        # the block's own walk starts at its first source column with the table entries of column 0: fraction 0, sources + 0 and + 1
        base = int(xlo[x0])
        assert base + int(xhi[0]) <= skip.shape[2] - 1
        res["C"] = err(column(base + int(xlo[0]), base + int(xhi[0]), float(xl[0])))
        res["C_fractions"] = (float(xl[x0]), float(xl[0]))
        # What C can do at this seam whatever the images hold: it moves the column by (difference of the fractions) x BN2 scale x
        # (right - left source column); a channel of the skip tensor, the BN of a pooled ReLU6 output in [0, 6], spans at most
        # 6 |BN scale|.  Relative to the abs-max of the output:
        sc1 = np.abs(SR._bn(w, g.stages[s.skip_stage].bn_name)[0] / np.sqrt(SR._bn(w, g.stages[s.skip_stage].bn_name)[3] + R.BN_EPS))
        sc2 = np.abs(SR._bn(w, s.bn2_name)[0] / np.sqrt(SR._bn(w, s.bn2_name)[3] + R.BN_EPS))
        res["C_reach"] = abs(res["C_fractions"][0] - res["C_fractions"][1]) * float((6.0 * sc1 * sc2).max()) / float(np.abs(out).max())
    return res


_FIGURES = {}


def _figures(side):
    """Everything the tests below assert, from ONE float64 oracle run of the two images at ``side`` (the tensors are dropped)."""
    if side in _FIGURES:
        return _FIGURES[side]
    g = build_graph(6, side)
    w = CK.live(g, 0, CK.LIVE_GAIN)
    taps = R.infer(w, parity_set_of(side)[CK.SEAM_IDX], dtype=np.float64, taps=True)["taps"]
    fig = {"shares": CK.clamp_shares(taps), "shares_30": CK.clamp_shares({k: v[:1] for k, v in taps.items() if k.endswith(".conv")}),
           "contrast_30": [_contrast(taps[SR.stage_out_name(s)][0]) for s in g.stages],
           "contrast_14": [_contrast(taps[SR.stage_out_name(s)][1]) for s in g.stages], "mutants": {}, "emulated": {}}
    if side in PLANNED_SIDES:
        for k, seams in BP.seam_columns(g).items():
            s = g.stages[k]
            # the GPU test's bound, max(STAGE_TOL, 2 x emulated), on the oracle's own tensors rounded to the storage type
            x_in = SR.round_storage(taps[SR.stage_out_name(g.stages[k - 1])], "bf16")
            skip = SR.round_storage(taps[SR.stage_out_name(g.stages[s.skip_stage])], "bf16") if s.residual else None
            fig["emulated"][k] = SR.rel_err(SR.stage_local_emulated(g, w, k, x_in, skip, "bf16"), SR.stage_local(g, w, k, x_in, skip))
            for x0 in seams:
                fig["mutants"][(k, x0)] = _mutants(g, w, taps, k, x0)
    _FIGURES[side] = fig
    return fig


# ---------------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("side", ALL_SIDES)
def test_block_counts_are_pinned(side):
    g = build_graph(6, side)
    counts = BP.block_counts(g)
    assert tuple(counts[f] for f in BP.FAMILIES) == BLOCK_COUNTS[side]
    if side in CK.SEAM_SIDES:
        assert BP.block_plans(g) == BLOCK_PLANS[side]
        assert SR.fp16_pool_stages(g) == (1, 2, 3, 4, 5)
        assert min(BLOCK_COUNTS[side]) >= 2
    if side in CK.FOUR_BLOCK_SIDES:
        assert BP.block_plans(g) == BLOCK_PLANS[side]
        # stage 4 pools fp16 values only where its row-blocked kernel runs
        assert SR.fp16_pool_stages(g) == (1, 2, 3) + tuple(k for k in (4, 5) if BLOCK_PLANS[side][k])
    # every plan tiles the row: blocks follow one another, widths differ by at most one and lie inside the kernel's limits
    for f, plan in BP.block_plans(g).items():
        assert (counts[f] == 0) == (plan is None)
        out_side = g.stages[3 if f == "pair" else f].out_side
        lo, hi = (BP.X_WMIN - 10, BP.X_WMAX - 10) if f == "pair" else BP.WIDTH_LIMITS[f]
        # the widths of a cut into nb blocks of equal width +-1 lie in out_side // nb .. ceil(out_side / nb)
        fits = [nb for nb in range(1, 5) if lo <= out_side // nb and -(-out_side // nb) <= hi]
        if not plan:
            # a family without a plan: no cut of this row into one to four such blocks lies inside the limits
            assert not fits, (side, f, out_side, fits)
            continue
        assert len(plan) == fits[0]         # the fewest blocks that fit
        assert plan[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(plan, plan[1:])) and plan[-1][0] + plan[-1][1] == out_side
        widths = [wo for _, wo in plan]
        assert max(widths) - min(widths) <= 1 and lo <= min(widths) and max(widths) <= hi and widths == sorted(widths, reverse=True)


def test_seam_sides_cover_two_and_three_blocks_unequal_blocks_and_the_widest_block():
    plans = {side: BP.block_plans(build_graph(6, side)) for side in CK.SEAM_SIDES}
    for f in BP.FAMILIES:
        assert {len(plans[side][f]) for side in CK.SEAM_SIDES} == {2, 3}, f
        assert any(len({wo for _, wo in plans[side][f]}) == 2 for side in CK.SEAM_SIDES), f
    assert max(wo for side in CK.SEAM_SIDES for _, wo in plans[side][6]) == BP.WIDTH_LIMITS[6][1]
    assert BP.seam_columns(build_graph(6, 600)) == {3: [194, 388], 4: [96, 192], 5: [48, 95], 6: [47, 94]}


def test_four_block_sides_cover_four_unequal_blocks_of_stage_5_and_of_stage_6():
    plans = {side: BP.block_plans(build_graph(6, side)) for side in CK.FOUR_BLOCK_SIDES}
    for f in (5, 6):
        four = [plans[side][f] for side in CK.FOUR_BLOCK_SIDES if plans[side][f] and len(plans[side][f]) == 4]
        assert four, f
        assert any(len({wo for _, wo in p}) == 2 for p in four), f
    # 630: a four-block stage 6 behind three-block plans of everything in front of it; 686: neither the pair nor stage 4 has a plan
    assert [len(plans[630][f]) for f in BP.FAMILIES] == [3, 3, 3, 4]
    assert plans[686]["pair"] is None and plans[686][4] is None and len(plans[686][5]) == len(plans[686][6]) == 4
    assert BP.seam_columns(build_graph(6, 630)) == {3: [204, 408], 4: [101, 202], 5: [50, 100], 6: [37, 74, 111]}
    assert BP.seam_columns(build_graph(6, 686)) == {5: [41, 82, 123], 6: [41, 81, 121]}


def test_block_counts_of_every_side_up_to_the_heads_limit():
    """Every side build_graph accepts whose flatten fits head_kernel (MIN_SIDE .. MAX_HEAD_SIDE): the pair and stage 4 never run more
    than three blocks there (their four-block plans start at 751 and 783), stages 5 and 6 reach four exactly in FOUR_BLOCK_RANGES."""
    with pytest.raises(ValueError):
        build_graph(6, MIN_SIDE - 1)
    four = {}
    for side in range(MIN_SIDE, MAX_HEAD_SIDE + 1):
        counts = BP.block_counts(build_graph(6, side))
        assert counts["pair"] <= 3 and counts[4] <= 3, (side, counts)
        if max(counts.values()) == 4:
            four[side] = tuple(counts[f] for f in BP.FAMILIES)
    assert four == {side: c for (a, b), c in FOUR_BLOCK_RANGES.items() for side in range(a, b + 1)}
    assert all(any(a <= side <= b for a, b in FOUR_BLOCK_RANGES) for side in CK.FOUR_BLOCK_SIDES)
    first = lambda f: min(side for side in range(MAX_HEAD_SIDE + 1, 900) if BP.block_counts(build_graph(6, side))[f] == 4)
    assert (first("pair"), first(4)) == (751, 783)


def test_694_is_the_largest_side_whose_flatten_fits_the_head():
    """head_kernel stages the flatten in LDS: HEAD_MAX_FLAT (4096) floats (rn_kernels_f32.hip).  The flatten is 16 channels of stage 9's
    square output: 16 x 16 x 16 = 4096 at 663-694 (every side with four stage-5 blocks among them), 17 x 17 x 16 = 4624 from 695 on."""
    flat = {side: build_graph(6, side).flat_len for side in range(MIN_SIDE, MAX_HEAD_SIDE + 2)}
    assert max(side for side, n in flat.items() if n <= HEAD_MAX_FLAT) == MAX_HEAD_SIDE
    assert flat[MAX_HEAD_SIDE] == HEAD_MAX_FLAT and flat[MAX_HEAD_SIDE + 1] == 4624
    assert all(a <= b for a, b in zip(list(flat.values()), list(flat.values())[1:]))
    assert [side for side, n in flat.items() if n == HEAD_MAX_FLAT] == list(range(663, 695))
    assert flat[686] == HEAD_MAX_FLAT and flat[600] == flat[630] == 3136


@pytest.mark.parametrize("side", PLANNED_SIDES)
def test_f32_and_band_planners_beside_the_block_plans(side):
    """The float32 matrix-core stages cut their rows too (n_colblocks > 1 at every seam side): pinned.  rn_band_plan takes a
    launch's block count: with the counts of the plans it gives bands that tile the rows, for one image and for the two."""
    g = build_graph(6, side)
    got = [_capi.f32m_plan(s.cin, s.cout, s.pool_k, s.pool_s, s.skip_stage >= 0, s.in_side, s.out_side)["n_colblocks"] for s in g.stages[1:9]]
    assert got == F32M_COLBLOCKS[side] and max(got) > 1
    counts = BP.block_counts(g)
    for f, k, family in (("pair", 3, "pair"), (4, 4, "rowreg"), (5, 5, "rowreg"), (6, 6, "rowreg")):
        s = g.stages[k]
        if not counts[f]:                   # (686: the pair and stage 4 have no plan, so no launch of theirs takes a block count)
            assert side in CK.FOUR_BLOCK_SIDES
            continue
        for n in (1, 2):
            rows, bands = _capi.band_plan(family, n, 256, s.out_side, counts[f], pool_k=s.pool_k, pool_s=s.pool_s)
            assert rows >= 1 and (bands - 1) * rows < s.out_side <= bands * rows, (side, f, n, rows, bands)


# ---------------------------------------------------------------------------------------------- the images
@pytest.mark.parametrize("side", (240,) + PLANNED_SIDES)
def test_the_two_images_reach_the_clamp_in_every_stage(side):
    fig = _figures(side)
    print(side, " ".join("s%d=%.4f/%.3f" % (k, a, b) for k, (a, b) in enumerate(fig["shares"])))
    for k in range(1, 10):
        assert fig["shares"][k][0] >= AT_CLAMP_MIN and fig["shares"][k][1] >= INSIDE_MIN, (side, k, fig["shares"])
        # the checkerboard on its own as well: what the textured image adds is texture, not clamp reach
        assert fig["shares_30"][k][0] >= AT_CLAMP_MIN and fig["shares_30"][k][1] >= INSIDE_MIN, (side, k, fig["shares_30"])


@pytest.mark.parametrize("side", ALL_SIDES)
def test_the_textured_image_tells_neighbouring_columns_and_rows_apart(side):
    fig = _figures(side)
    print(side, "image 14:", " ".join("%.3f/%.3f" % c for c in fig["contrast_14"]))
    print(side, "image 30:", " ".join("%.3f/%.3f" % c for c in fig["contrast_30"]))
    for k in range(10):
        assert min(fig["contrast_14"][k]) >= CONTRAST_MIN, (side, k, fig["contrast_14"][k])
    # the checkerboard alone could not show a duplicated column or row in stages 0-4: nobody goes back to one image
    for k in range(5):
        assert max(fig["contrast_30"][k]) < STAGE_TOL["f16"], (side, k, fig["contrast_30"][k])


# ---------------------------------------------------------------------------------------------- the mutants
def _mutant_bound(fig, k):
    return MUTANT_FACTOR * max(STAGE_TOL["bf16"], 2.0 * fig["emulated"][k])


@pytest.mark.parametrize("side", CK.SEAM_SIDES)
def test_seam_mutants_a_and_b_exceed_twice_the_gpu_tolerance(side):
    _mutants_a_and_b_exceed_the_bound(side, list(SEAM_STAGES))


@pytest.mark.parametrize("side", CK.FOUR_BLOCK_SIDES)
def test_seam_mutants_a_and_b_exceed_twice_the_gpu_tolerance_at_four_block_sides(side):
    """Every seam of the side's plans: 630 has seams in stages 3-6 (stage 6: three of them), 686 in stages 5 and 6 only."""
    stages = [k for k, f in zip(SEAM_STAGES, BP.FAMILIES) if BLOCK_PLANS[side][f]]
    assert stages == {630: [3, 4, 5, 6], 686: [5, 6]}[side]
    seams = _mutants_a_and_b_exceed_the_bound(side, stages)
    assert seams == [(k, x0) for k, f in zip(SEAM_STAGES, BP.FAMILIES) if BLOCK_PLANS[side][f] for x0, _ in BLOCK_PLANS[side][f][1:]]


def _mutants_a_and_b_exceed_the_bound(side, stages):
    fig = _figures(side)
    assert sorted({k for k, _ in fig["mutants"]}) == stages
    bad = []
    for (k, x0), res in sorted(fig["mutants"].items()):
        bound = _mutant_bound(fig, k)
        print("side %d stage %d seam %3d: emulated %.4f  bound %.4f  A %.4f  B %s" % (
            side, k, x0, fig["emulated"][k], bound, res["A"], "%.4f" % res["B"] if "B" in res else "-"))
        assert ("B" in res) == (k != 6)
        bad += [(k, x0, m, res[m], bound) for m in ("A", "B") if m in res and not res[m] > bound]
    assert not bad, bad
    return sorted(fig["mutants"])


def test_seam_mutant_c_exceeds_twice_the_gpu_tolerance_at_every_seam_of_the_four_block_sides():
    """(C) at the seams of stages 3 and 5 at CK.FOUR_BLOCK_SIDES: at every one of them the global column's lerp fraction is non-zero
    and the fraction of the column inside the block is 0, so none is skipped: each must clear the bound (the tightest on the oracle:
    630, stage 3, seam 204, 0.0283 against 0.0250)."""
    seen = []
    bad = []
    for side in CK.FOUR_BLOCK_SIDES:
        fig = _figures(side)
        for (k, x0), res in sorted(fig["mutants"].items()):
            assert ("C" in res) == (k in (3, 5))
            if "C" not in res:
                continue
            bound = _mutant_bound(fig, k)
            f_global, f_local = res["C_fractions"]
            print("side %d stage %d seam %3d: fractions %.4f / %.4f  reach %.4f  bound %.4f  C %.4f" % (
                side, k, x0, f_global, f_local, res["C_reach"], bound, res["C"]))
            assert f_local == 0.0 and f_global != 0.0, (side, k, x0, res["C_fractions"])
            seen.append((side, k, x0))
            if not res["C"] > bound:
                bad.append((side, k, x0, res["C"], bound))
    assert not bad, bad
    assert seen == [(630, 3, 204), (630, 3, 408), (630, 5, 50), (630, 5, 100), (686, 5, 41), (686, 5, 82), (686, 5, 123)]


def test_seam_mutant_c_exceeds_twice_the_gpu_tolerance_wherever_the_seam_can_show_it():
    """(C) at a seam column: the lerp fraction and the source columns of the column INSIDE the block (0: fraction 0, the block's first
    source column and the next) instead of the global column's.  Where the global fraction is 0 too, both coincide and the mutant is
    the tensor itself (409, stage 3: the seam 195 x 400 / 390 = 200 exactly): skipped.  Where they nearly coincide -- 420: global
    fractions 0.0125 (stage 3) and 0.0206 (stage 5) -- the mutant moves the column by that fraction of the difference of two source
    columns: by at most C_reach whatever the images hold (0.0146 and 0.0140 of the abs-max; measured error 0.0009 and 0.0028), below
    the bound (0.025) and close to what the GPU test tolerates.  No image makes such a seam show C; it is skipped by that inequality,
    which the equal fractions satisfy with C_reach = 0.  The skipped seams are pinned; every other seam must clear the bound, and
    each residual stage keeps at least one (stage 3: both seams of 600; stage 5: 409 and both of 600)."""
    kept = {3: [], 5: []}
    skipped = []
    bad = []
    for side in CK.SEAM_SIDES:
        fig = _figures(side)
        for (k, x0), res in sorted(fig["mutants"].items()):
            if "C" not in res:
                continue
            bound = _mutant_bound(fig, k)
            f_global, f_local = res["C_fractions"]
            print("side %d stage %d seam %3d: fractions %.4f / %.4f  reach %.4f  bound %.4f  C %.4f" % (
                side, k, x0, f_global, f_local, res["C_reach"], bound, res["C"]))
            if f_global == f_local:
                assert res["C"] == 0.0
            if res["C_reach"] <= bound:
                assert res["C"] <= res["C_reach"]
                skipped.append((side, k, x0))
                continue
            kept[k].append((side, x0))
            if not res["C"] > bound:
                bad.append((side, k, x0, res["C"], bound))
    assert not bad, bad
    assert kept[3] and kept[5], kept
    assert skipped == [(409, 3, 195), (420, 3, 201), (420, 5, 49)], skipped


# ---------------------------------------------------------------------------------------------- the shared check itself
class _StoredTaps:
    """What stage_ref.check_stage_local needs of a handle: the graph, a forward pass, the stored stage outputs."""

    def __init__(self, graph, taps):
        self.graph, self._taps = graph, taps

    def forward_u8(self, ims):
        return None

    def tap(self, name, n):
        return self._taps[name][:n]


def test_check_stage_local_lazy_form_has_the_eager_bound_and_names_a_duplicated_column():
    """check_stage_local on a stand-in handle whose stored tensors ARE the emulated bf16 stages of the textured image at 224: the lazy
    form gives the eager form's errors and skips the emulation exactly where the error is inside STAGE_TOL; with one column of s3.bn2
    stored from its left neighbour it computes the emulation, fails on that stage alone and reports that column."""
    g = build_graph(6, 224)
    w = CK.live(g, 0, CK.LIVE_GAIN)
    im = parity_set_of(224)[CK.SEAM_IDX[1:]]
    def stored(duplicate=None):
        """The emulated chain as a handle would store it; ``duplicate`` = (stage, column): that column stored from its left neighbour
        (the stages behind it compute from what is stored)."""
        taps, outs = {}, []
        for k, s in enumerate(g.stages):
            x_in = SR.preprocess64(im) if k == 0 else outs[k - 1]
            out = SR.stage_local_emulated(g, w, k, x_in, outs[s.skip_stage] if s.residual else None, "bf16")
            if duplicate and duplicate[0] == k:
                out[:, :, duplicate[1]] = out[:, :, duplicate[1] - 1]
            outs.append(out)
            taps[SR.stage_out_name(s)] = out.astype(np.float32)
            np.testing.assert_array_equal(taps[SR.stage_out_name(s)], out)          # bf16 values: exact in float32
        return taps

    taps = stored()
    eager = SR.check_stage_local(_StoredTaps(g, taps), w, im, "bf16")
    lazy = SR.check_stage_local(_StoredTaps(g, taps), w, im, "bf16", lazy_emulation=True)
    assert list(eager) == list(lazy) == SR.STAGE_OUT
    for name in SR.STAGE_OUT:
        assert lazy[name]["rel_err"] == eager[name]["rel_err"] == eager[name]["emulated_rel_err"] > 0
        assert eager[name]["bound"] == max(STAGE_TOL["bf16"], 2.0 * eager[name]["emulated_rel_err"])
        assert lazy[name]["rel_err"] <= STAGE_TOL["bf16"] and lazy[name]["emulated_rel_err"] is None and lazy[name]["bound"] == STAGE_TOL["bf16"]
    x = 100
    wrong = stored(duplicate=(3, x))
    for is_lazy in (True, False):
        with pytest.raises(AssertionError) as info:
            SR.check_stage_local(_StoredTaps(g, wrong), w, im, "bf16", lazy_emulation=is_lazy)
        bad = info.value.args[0]
        # stage 3 alone: stage 4 is judged on the stored, wrong, tensor as its exact input
        assert [b[0] for b in bad] == ["s3.bn2"], bad
        name, err, bound, where = bad[0]
        assert where["at [n, y, x, c]"][2] == x and err > 4 * bound
        assert bound == eager["s3.bn2"]["bound"]
