"""GPU parity at column-block seams on the `live` checkpoint (tests/checkpoints.py): the sides CK.SEAM_SIDES, where the fused stage
pair and the row-blocked stages 4, 5 and 6 run two or three column blocks, ragged last blocks included (tests/block_plans.py), and
the float32 matrix-core stages two to four.  tests/test_hip_other_checkpoints.py judges the same kernels at 224 and 240, one block each.

Weights: `live` built for the side's own graph (every BN live, ReLU6 saturating).  Images: CK.SEAM_IDX, the image that reaches the
clamp in every stage plus the textured one.  tests/test_seam_cases_host.py asserts on the float64 oracle that these cases see a
duplicated seam column, a dropped window tap and a block-local lerp fraction.

  a. 16-bit stage-launch handles, STAGE-LOCALLY against float64 (stage_ref.check_stage_local): exact inputs, the bound of the 224 case.
  b. the product kernels (default handle: stages 0+1 fused, the fused pair) against the stage-launch handle, criteria of
     test_hip_other_checkpoints.test_cross_stage_fusion_matches_stage_launches_on_live -- with (a) that ties the pair's two-, three-
     and unequal-block forms to float64 on values that saturate.
  c. head_kernel HEAD-LOCALLY (stage_ref.check_head_local) at the long flattens 3136 (600) and 4096 (686, its limit).
  d. float32 handles (per node and matrix cores) against the float64 oracle at 420, 600 and 686.
  e. side 695, the first past the head's limit: classifying is refused by name, the features are still served.
(a) and (b) run a second time at CK.FOUR_BLOCK_SIDES -- 630: stage 6 in FOUR blocks behind three-block plans; 686: stages 5 and 6 in
four, no plan for the pair and stage 4 -- in parametrisations of their own: the seam-side tests assert two or three blocks everywhere.
Every figure is printed and recorded (sections `other_checkpoints` and `seams` of the parity report) before it is asserted."""
import numpy as np
import pytest

import block_plans as BP
import checkpoints as CK
from conftest import parity_set_of
from oracle import c_oracle, roomnet_ref as R
from parity_bounds import _downstream_same, _same_up_to_sum_order
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph
from stage_ref import NOTHING_FOLDED, SECTION, STAGE_OUT, _check_nodes, check_head_local, check_stage_local

pytestmark = pytest.mark.gpu

SEAMS = "seams"               # the parity report's section of what the four-block cases record beside SECTION's rows
_CASES = {}


def _case(side):
    """(graph, live weights, the two images) of a side, built once."""
    if side not in _CASES:
        g = build_graph(6, side)
        _CASES[side] = (g, CK.live(g, 0, CK.LIVE_GAIN), parity_set_of(side)[CK.SEAM_IDX])
    return _CASES[side]


# ---------------------------------------------------------------------------------------------- a. 16-bit, stage-local
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", CK.SEAM_SIDES)
def test_16bit_stages_locally_vs_fp64_at_seam_sides(record, side, dtype):
    g, w, ims = _case(side)
    assert min(BP.block_counts(g).values()) >= 2
    e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=len(ims), stage_launches=True)
    try:
        assert e.frozen_info() == NOTHING_FOLDED and e.const_info()["stage"] == -1
        print("side %d: seam columns %s" % (side, BP.seam_columns(g)))
        check_stage_local(e, w, ims, dtype, record, "stage_local_%d_live_%s" % (side, dtype), lazy_emulation=True)
    finally:
        e.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", CK.FOUR_BLOCK_SIDES)
def test_16bit_stages_locally_vs_fp64_at_four_block_sides(record, side, dtype):
    """Stage 6 in four column blocks (630, behind three-block plans) and stages 5 and 6 in four (686, where neither the
    pair nor stage 4 has a plan and other kernels run stages 2-4): each stage on its own stored input, the bound of every other side."""
    g, w, ims = _case(side)
    counts = BP.block_counts(g)
    assert counts[6] == 4 and counts[5] == (4 if side == 686 else 3)
    e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=len(ims), stage_launches=True)
    try:
        assert e.frozen_info() == NOTHING_FOLDED and e.const_info()["stage"] == -1
        print("side %d: seam columns %s" % (side, BP.seam_columns(g)))
        rows = check_stage_local(e, w, ims, dtype, record, "stage_local_%d_live_%s" % (side, dtype), lazy_emulation=True)
        record(SEAMS, "stage_local_%d_live_%s" % (side, dtype), {
            "block_counts": {str(f): n for f, n in counts.items()}, "seam_columns": {"s%d" % k: v for k, v in BP.seam_columns(g).items()},
            "rel_err": {name: r["rel_err"] for name, r in rows.items()}, "bound": {name: r["bound"] for name, r in rows.items()}})
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- b. the product kernels
def _where_they_differ(a, b, seams):
    """Columns of the differing elements, relative to the nearest seam: what to read when (b) fails."""
    cols = np.unique(np.argwhere(a != b)[:, 2])
    return {"columns": cols[:32].tolist(), "seams": seams,
            "distance_to_nearest_seam": [int(min(abs(int(c) - s) for s in seams)) for c in cols[:32]] if seams else []}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", CK.SEAM_SIDES)
def test_cross_stage_fusion_matches_stage_launches_on_live_at_seam_sides(side, dtype):
    g, w, ims = _case(side)
    nb = len(ims)
    fused = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=nb)
    plain = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
    try:
        assert fused.launch_groups()[:2] == [[0, 1], [2, 3]] and fused.frozen_info() == NOTHING_FOLDED
        ids_f, probs_f = fused.forward_u8(ims)
        ids_p, probs_p = plain.forward_u8(ims)
        a1, b1 = fused.tap("s1.bn", nb), plain.tap("s1.bn", nb)
        bad = np.argwhere(a1 != b1)
        assert bad.size == 0, ("s1", side, dtype, len(bad), bad[:8].tolist(), float(np.abs(a1 - b1).max()))
        a3, b3 = fused.tap("s3.bn2", nb), plain.tap("s3.bn2", nb)
        if (a3 != b3).any():
            print("s3.bn2 side %d %s: %d of %d elements differ, %s" % (side, dtype, int((a3 != b3).sum()), a3.size,
                                                                      _where_they_differ(a3, b3, BP.seam_columns(g)[3])))
        _same_up_to_sum_order(a3, b3, dtype, ("s3.bn2", side))
        _downstream_same(fused, plain, ("s8.bn", "s9.bn2", "d3.relu"), nb, dtype, probs_f, probs_p, ids_f, ids_p)
    finally:
        fused.close()
        plain.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", CK.FOUR_BLOCK_SIDES)
def test_cross_stage_fusion_matches_stage_launches_on_live_at_four_block_sides(record, side, dtype):
    """The criteria of the seam-side test above.  Which launches are fused follows from the plans: stages 0+1 at both sides, the
    pair at 630 (three blocks) and not at 686 (no plan: stages 2 and 3 are two launches in both arms)."""
    g, w, ims = _case(side)
    nb = len(ims)
    pair_plan = BP.block_plans(g)["pair"]
    assert (pair_plan is not None) == (side == 630)
    fused = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=nb)
    plain = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
    try:
        groups = fused.launch_groups()
        print("side %d %s: launch groups %s" % (side, dtype, groups))
        assert groups[0] == [0, 1] and fused.frozen_info() == NOTHING_FOLDED
        assert ([2, 3] in groups) == (pair_plan is not None), (side, groups)
        assert groups[1:3] == ([[2, 3], [4]] if pair_plan else [[2], [3]])
        ids_f, probs_f = fused.forward_u8(ims)
        ids_p, probs_p = plain.forward_u8(ims)
        a1, b1 = fused.tap("s1.bn", nb), plain.tap("s1.bn", nb)
        bad = np.argwhere(a1 != b1)
        a3, b3 = fused.tap("s3.bn2", nb), plain.tap("s3.bn2", nb)
        record(SEAMS, "fused_vs_stage_launches_%d_live_%s" % (side, dtype), {
            "launch_groups": groups, "s1.bn_elements_differing": int(len(bad)), "s3.bn2_elements_differing": int((a3 != b3).sum()),
            "s3.bn2_elements": int(a3.size), "max_abs_dprob": float(np.abs(probs_f - probs_p).max())})
        assert bad.size == 0, ("s1", side, dtype, len(bad), bad[:8].tolist(), float(np.abs(a1 - b1).max()))
        if (a3 != b3).any():
            print("s3.bn2 side %d %s: %d of %d elements differ, %s" % (side, dtype, int((a3 != b3).sum()), a3.size,
                                                                      _where_they_differ(a3, b3, BP.seam_columns(g).get(3, []))))
        _same_up_to_sum_order(a3, b3, dtype, ("s3.bn2", side))
        _downstream_same(fused, plain, ("s8.bn", "s9.bn2", "d3.relu"), nb, dtype, probs_f, probs_p, ids_f, ids_p)
    finally:
        fused.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- c. the head at long flattens
# side -> (flatten, values per K partition of the first dense layer: 1024 threads / 32 outputs = 32 partitions)
LONG_FLATTENS = {600: (3136, 98), 686: (4096, 128)}


@pytest.mark.parametrize("side,dtype", [(600, "bf16"), (600, "f16"), (686, "bf16"), (686, "f16"), (686, "f32")])
def test_head_locally_vs_fp64_at_long_flattens(record, side, dtype):
    """head_kernel with 1024 threads: the first dense layer's K loop split over 32 partitions, eight steps per trip and a remainder
    loop.  600: 98 values per partition = twelve trips + two remainder steps; 686: 128 values = sixteen trips, no remainder, the
    flatten exactly HEAD_MAX_FLAT.  Judged from the handle's own s9.bn2 (stage_ref.check_head_local): the stage-launch handles of
    (a) in both 16-bit types, and a float32 handle at 686."""
    g, w, ims = _case(side)
    flat, per_part = LONG_FLATTENS[side]
    d0 = g.dense[0]
    assert g.flat_len == d0.nin == flat and 1024 % d0.nout == 0 and flat == per_part * (1024 // d0.nout)
    assert (per_part % 8 != 0) == (side == 600)
    e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=len(ims), stage_launches=dtype != "f32")
    try:
        ids, probs = e.forward_u8(ims)
        if dtype != "f32":
            assert e.launch_groups()[-2:] == [[8], [9]]          # no tail kernel: head_kernel is the launch that classifies
        check_head_local(e, w, len(ims), ids, probs, record, "head_local_flat%d_%d_live_%s" % (flat, side, dtype))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- d. float32 handles
@pytest.mark.parametrize("side", [420, 600, 686])
def test_f32_handles_vs_fp64_at_seam_sides(record, side):
    """Per-node and matrix-core handles against ONE float64 oracle run of the side (tolerance scaled by the float32 C oracle's own
    deviation, as in test_f32_handles_vs_fp64): every node at 420, the stage outputs and the logits at 600 and at 686."""
    g, w, ims = _case(side)
    n = len(ims)
    r64, r32 = R.infer(w, ims, dtype=np.float64, taps=True), c_oracle.infer(w, ims, taps=True)
    pn = _capi.Engine(g, w, device=0, dtype="f32", max_batch=n, taps=True)
    mm = _capi.Engine(g, w, device=0, dtype="f32", max_batch=n)
    try:
        assert pn.frozen_info() == NOTHING_FOLDED and mm.frozen_info() == NOTHING_FOLDED
        ids_a, probs_a = pn.forward_u8(ims)
        ids_b, probs_b = mm.forward_u8(ims)
        names = R.node_names()
        assert set(names) == set(pn.nodes())
        _check_nodes(pn, names if side == 420 else STAGE_OUT + ["d3.relu"], n, r64, r32, record, "f32_per_node_%d_live" % side)
        _check_nodes(mm, STAGE_OUT + ["d3.relu"], n, r64, r32, record, "f32_matrix_core_%d_live" % side)
        rows = {}
        for name in STAGE_OUT:
            a, b = pn.tap(name, n), mm.tap(name, n)
            rows[name] = float(np.abs(a - b).max() / max(float(np.abs(a).max()), 1e-3))
        record(SECTION, "f32_matrix_core_vs_per_node_%d_live" % side, rows)
        print("matrix cores vs per node:", " ".join("%s=%.2g" % kv for kv in rows.items()))
        assert all(v <= 2e-5 for v in rows.values()), rows
        lg = np.sort(r64["logits"], axis=1)
        safe = lg[:, -1] - lg[:, -2] > 1e-3
        np.testing.assert_array_equal(ids_a[safe], r64["ids"][safe])
        np.testing.assert_array_equal(ids_b[safe], r64["ids"][safe])
    finally:
        pn.close()
        mm.close()


# ---------------------------------------------------------------------------------------------- e. past the head's limit
def test_side_695_is_refused_by_the_head_and_still_gives_features(record):
    """695 is the first side whose flatten (17 x 17 x 16 = 4624) exceeds head_kernel's HEAD_MAX_FLAT.  rn_create accepts it -- a handle
    that only feeds a trainer needs no head -- and every classifying call is refused by the host check of rn_launch_head, before any
    launch of head_kernel; the handle stays usable: the same image still gives its s7.bn features."""
    side = CK.MAX_HEAD_SIDE + 1
    g = build_graph(6, side)
    assert side == 695 and g.flat_len == 4624 and build_graph(6, CK.MAX_HEAD_SIDE).flat_len == 4096
    w = CK.live(g, 0, CK.LIVE_GAIN)
    im = parity_set_of(side)[CK.SEAM_IDX[1:]]
    e = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=1)
    try:
        with pytest.raises(_capi.RoomNetLibraryError, match="flatten length 4624 exceeds head kernel capacity 4096"):
            e.forward_u8(im)
        s7 = g.stages[7].out_side
        assert e.features_shape() == (s7, s7, 16)
        feat = e.features_u8(im)
        assert feat.shape == (1, s7, s7, 16) and feat.dtype == np.float32 and np.isfinite(feat).all()
        assert float(np.abs(feat).max()) > 0
        record(SEAMS, "side_695_features_after_refused_forward", {"shape": list(feat.shape), "abs_max": float(np.abs(feat).max())})
        # a second refusal behind the feature pass, then the handle goes away in order
        with pytest.raises(_capi.RoomNetLibraryError, match="exceeds head kernel capacity"):
            e.forward_u8(im)
        e.close()
        assert e._h is None
    finally:
        e.close()
