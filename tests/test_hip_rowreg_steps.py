"""The row steps of the row-register kernels (rn_stage4x.hip, rn_stage5x.hip) at every phase of their unrolled loops.

Stage 4 runs its row steps in periods of 12 (ring slot, accumulator rotation and row parity are compile time) and leaves the
period where the band ends; stage 5 in periods of 6.  Both carry the input-row pointer, the output row and the dither seeds from
step to step.  What can go wrong is a phase of the period, the place where a band ends inside it, and carried state that goes
stale: the 224 x 224 batch-256 shape walks one residue of `nin mod period` only (one band per image), so these cases take small
batches, which the planner cuts into many short bands, and sides whose last band is ragged.

Two references.

(1) Bit for bit: the kernels against themselves under ANOTHER band plan, with dithering on.  An output row's value does not depend
on where its band starts, but its place in the period, the seed of its odd step and the carried pointers do.  The planner gives
batches 1 and 3 the same bands, so every side also runs two larger batches (BATCHES) whose stage 4 and stage 5 plans differ from
the plan of one image, and the first image of each must come out with the bytes it has alone.  The CPU test works out from
rn_band_plan which bands exist in only one of two compared plans and requires those bands to end at every residue of both
periods, to include the shortest band (one output row) and to include the two-column-block side.

(2) The handle that runs one launch per stage on the generic kernels (stage_launches + generic_kernels), at batches 1 and 3 (420:
1), against the handle under test with no_dither (that arm rounds plainly).  That arm pools in float32, does not fold the division
by 6, and its earlier stages run on other kernels as well, so the inputs of stage 4 differ by 16-bit roundings already: equality of
bits is not a property the two arms have on any build, and a bound per element in units of the element's own last place cannot be
derived either (y = fma(H, sc, sh) cancels, and so do the 288 products of a conv output: a difference of one rounding in an input
is unbounded in units of a small result's last place).  The bound is the one test_conv16_stage_matches_the_generic_kernel_at_odd_sizes
holds the same pair of arms to: per element 4 units of the last place of the tensor's largest value (2^-7 bf16 / 2^-10 f16).  With
inputs that ARE bit-identical, test_row_blocked_stage_kernels_match_the_round2_kernels_at_their_geometry_edges holds the two kernels
to 2 / 4 half units.
"""
import numpy as np
import pytest
import torch              # (in front of the first load of the project's library, as in the other test files that use both)

import block_plans as BP
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph

S4_PERIOD, S5_PERIOD = 12, 6          # rn_stage4x.hip / rn_stage5x.hip: row steps per trip of the steady loop
# image side -> batches.  The sides of one stage-4 column block (input side 193..206), two blocks at 420.  Batches 1 and 3 (bands of
# 4..5 output rows, ragged last bands; 420: batch 1) are compared with the generic arm; the first image of every further batch is
# compared bit for bit with the same image alone: 16 has another stage 4 plan than 1, 32 another plan of both stages (420: 7 and 10)
BATCHES = {213: (1, 3, 16, 32), 216: (1, 3, 16, 32), 219: (1, 3, 16, 32), 222: (1, 3, 16, 32), 224: (1, 3, 16, 32),
           226: (1, 3, 16, 32), 420: (1, 7, 10)}
GENERIC_BATCHES = {side: tuple(n for n in b if n <= 3) for side, b in BATCHES.items()}
N_CU = 256                            # MI355X: the planner's chip (the GPU tests ask the device)


def _bands(side, n, n_cu):
    """(first output row, row steps) of every band of the stage 4 and of the stage 5 launch of `n` images of `side`; a band of r
    output rows runs 2 r + 4 steps (input rows)."""
    g = build_graph(6, side)
    out = []
    for stage in (g.stages[4], g.stages[5]):
        assert stage.pool_k == 4 and stage.pool_s == 2
        rpb, nb = _capi.band_plan("rowreg", n, n_cu, stage.out_side, len(BP.stage_plan(g, stage.index)), pool_k=4, pool_s=2)
        rows = [min(stage.out_side, (b + 1) * rpb) - b * rpb for b in range(nb)]
        assert sum(rows) == stage.out_side and min(rows) >= 1
        out.append([(b * rpb, 2 * r + 4) for b, r in enumerate(rows)])
    return out


def _check_coverage(n_cu):
    """Only bands that exist in ONE of two plans whose outputs are compared bit for bit count: a band both plans have runs the same
    steps on the same rows twice."""
    seen = [set(), set()]
    blocks = set()
    for side, batches in BATCHES.items():
        alone = _bands(side, 1, n_cu)
        differs = [False, False]
        for n in batches[1:]:
            plan = _bands(side, n, n_cu)
            for st in (0, 1):
                only_one = set(alone[st]) ^ set(plan[st])
                differs[st] = differs[st] or bool(only_one)
                seen[st] |= {steps for _, steps in only_one}
        # every side is compared under two different plans of either stage
        assert differs == [True, True], (side, differs)
        blocks.add(len(BP.stage_plan(build_graph(6, side), 4)))
    # a band's step count is even (two input rows per output row + 4): every even residue must be walked
    assert {x % S4_PERIOD for x in seen[0]} == set(range(0, S4_PERIOD, 2)), sorted(seen[0])
    assert {x % S5_PERIOD for x in seen[1]} == set(range(0, S5_PERIOD, 2)), sorted(seen[1])
    # the shortest band the kernels run (one output row), and bands longer than one period of either kernel
    assert min(seen[0]) == 6 and min(seen[1]) == 6, (min(seen[0]), min(seen[1]))
    assert max(seen[0]) > 2 * S4_PERIOD and max(seen[1]) > 2 * S5_PERIOD
    assert blocks == {1, 2}, blocks


def test_the_cases_reach_every_residue_of_the_unroll_periods():
    """From rn_band_plan alone (no GPU): the bands that differ between two plans compared bit for bit end at every place of the
    periods that the geometry can reach, one of them is the shortest band there is, and both column-block counts occur."""
    _check_coverage(N_CU)


def _weights_for(weights, g, side):
    if side == 224:
        return weights
    from oracle import roomnet_ref as R
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    return w


def _images(side, n, parity_images):
    if side == 224:
        ims = parity_images
    else:
        from roomnet_amd.synth import parity_batch
        ims = parity_batch(side, seed=3)
    return ims[(np.arange(n) * 7 + 5) % len(ims)]


TAPS = ("s4.bn", "s5.bn2")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", sorted(BATCHES))
def test_row_steps_at_every_phase(weights, parity_images, side, dtype):
    g = build_graph(6, side)
    w = _weights_for(weights, g, side)
    batches = BATCHES[side]
    ims = _images(side, max(batches), parity_images)
    want = {}
    ref = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, stage_launches=True, generic_kernels=True)
    try:
        # the planner cuts bands for the chip it runs on: the coverage must hold for this device's plans
        _check_coverage(torch.cuda.get_device_properties(0).multi_processor_count)
        for nb in GENERIC_BATCHES[side]:
            ref.forward_u8(ims[:nb])
            want[nb] = {name: ref.tap(name, nb) for name in TAPS}
    finally:
        ref.close()
    lim = 4 * 2.0 ** (-7 if dtype == "bf16" else -10)
    for cf in (False, True):
        # (2) the generic arm rounds plainly: no_dither
        e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, compute_frozen=cf, no_dither=True)
        try:
            for nb in GENERIC_BATCHES[side]:
                e.forward_u8(ims[:nb])
                for name in TAPS:
                    a, b = e.tap(name, nb), want[nb][name]
                    assert a.shape == b.shape and np.isfinite(a).all()
                    scale = float(np.abs(b).max())
                    err = float(np.abs(a - b).max())
                    print("%s side %d nb %d %s cf %d: max err %.3g of %.3g allowed, %d of %d elements differ"
                          % (name, side, nb, dtype, cf, err / scale, lim, int((a != b).sum()), a.size))
                    assert err <= lim * scale, (name, side, nb, dtype, cf, err / scale)
        finally:
            e.close()
        # (1) the same image under other band plans, dithering on: the same bytes
        e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=max(batches), compute_frozen=cf)
        try:
            alone = []
            for k in range(3):
                e.forward_u8(ims[k:k + 1])
                alone.append({name: e.tap(name, 1)[0] for name in TAPS})
            for nb in batches[1:]:
                e.forward_u8(ims[:nb])
                for name in TAPS:
                    got = e.tap(name, nb)
                    for k in range(min(nb, 3)):
                        bad = np.argwhere(got[k] != alone[k][name])
                        assert bad.size == 0, (name, side, nb, dtype, cf, k, len(bad), bad[:4].tolist())
        finally:
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_row_steps_are_reproducible_at_batch_160(weights, parity_images, dtype):
    """Twelve passes over the same 160 images on one handle: the probabilities every pass, the two kernels' tensors twice -- carried
    pointers and counters are state that a stale value would corrupt only sometimes.  Default handle and computing arm."""
    g = build_graph(6, 224)
    ims = parity_images[(np.arange(160) * 7) % len(parity_images)]
    for cf in (False, True):
        e = _capi.Engine(g, weights, device=0, dtype=dtype, max_batch=160, compute_frozen=cf)
        try:
            ids0, probs0 = e.forward_u8(ims)
            t0 = {n: e.tap(n, 160) for n in TAPS}
            for rep in range(12):
                ids, probs = e.forward_u8(ims)
                np.testing.assert_array_equal(probs, probs0)
                np.testing.assert_array_equal(ids, ids0)
                if rep in (5, 11):
                    for n, t in t0.items():
                        np.testing.assert_array_equal(e.tap(n, 160), t, err_msg="%s rep %d cf %s" % (n, rep, cf))
        finally:
            e.close()
