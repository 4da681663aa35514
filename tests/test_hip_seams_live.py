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
  c. float32 handles (per node and matrix cores) against the float64 oracle at 420 and 600.
Every figure is printed and recorded (section `other_checkpoints` of the parity report) before it is asserted."""
import numpy as np
import pytest

import block_plans as BP
import checkpoints as CK
from conftest import parity_set_of
from oracle import c_oracle, roomnet_ref as R
from parity_bounds import _downstream_same, _same_up_to_sum_order
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph
from stage_ref import NOTHING_FOLDED, SECTION, STAGE_OUT, _check_nodes, check_stage_local

pytestmark = pytest.mark.gpu

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


# ---------------------------------------------------------------------------------------------- c. float32 handles
@pytest.mark.parametrize("side", [420, 600])
def test_f32_handles_vs_fp64_at_seam_sides(record, side):
    """Per-node and matrix-core handles against ONE float64 oracle run of the side (tolerance scaled by the float32 C oracle's own
    deviation, as in test_f32_handles_vs_fp64): every node at 420, the stage outputs and the logits at 600."""
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
