"""GPU parity on checkpoints OTHER than the shipped one (tests/checkpoints.py): live BNs with both signs of gamma, activations
that reach the upper ReLU6 clamp in every stage, head widths other than 6.  tests/test_checkpoints_host.py asserts on the CPU
that the recipes do that -- and that the shipped checkpoint does not.

What is compared with what:
  a. 16-bit handles, STAGE-LOCALLY: stage k's stored output against the float64 restatement of stage k alone (tests/stage_ref.py)
     fed the handle's own stored output of stage k - 1 (and skip tensor): exact inputs, nothing compounds.  Bound per tensor,
     relative to the abs-max of the float64 tensor: the larger of STAGE_TOL (what the project grants ten compounded stages) and
     2 x the error of the same stage with the documented roundings emulated in NumPy (the factor 2: tap-carried weight rounding
     and the dithered store may be one ulp off instead of half).
  b. tuned launches against one launch per stage, criteria of test_hip_fused.py; the generic kernels stage-locally.
  c. the one-launch back end (stages 6-9 and the head, stages 6-7 resident in LDS) bit for bit against the split launches.
  d. the float32 head, HEAD-LOCALLY from the handle's own s9.bn2, at 1, 2, 10 and 64 classes.
  e. float32 handles (per node and matrix cores) against float64.
  f. the whole 16-bit chain against float64: recorded, only the ids of clear margins asserted.
Every figure is printed and recorded (`record` -> the parity report; profiles/other_checkpoints_parity.json) before it is asserted."""
import numpy as np
import pytest

import checkpoints as CK
import stage_ref as SR
from conftest import parity_set_of
from oracle import c_oracle, roomnet_ref as R
from parity_bounds import FUSED_AWAY, _downstream_same, _same_up_to_sum_order
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph
from stage_ref import NOTHING_FOLDED, SECTION, STAGE_OUT, _check_nodes, check_head_local, check_stage_local

pytestmark = pytest.mark.gpu

WHOLE_CHAIN_MARGIN = 0.5      # (f): ids must agree with float64 wherever its top-2 logit margin exceeds this


@pytest.fixture(scope="module")
def graph():
    return build_graph(6, 224)


@pytest.fixture(scope="module")
def ims(parity_images):
    return parity_images[CK.PARITY_IDX]


@pytest.fixture(scope="module")
def checkpoints(graph):
    return {"live": CK.live(graph, 0, CK.LIVE_GAIN), "init_scale": CK.init_scale(graph, 0)}


@pytest.fixture(scope="module")
def refs(checkpoints, ims):
    """name -> (float64 oracle run, float32 C oracle run) of the three images, computed once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            w = checkpoints[name]
            cache[name] = (R.infer(w, ims, dtype=np.float64, taps=True), c_oracle.infer(w, ims, taps=True))
        return cache[name]
    return get


# ---------------------------------------------------------------------------------------------- a. 16-bit, stage-local
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("ckpt", ["live", "init_scale"])
def test_16bit_stages_locally_vs_fp64(graph, checkpoints, ims, record, ckpt, dtype):
    w = checkpoints[ckpt]
    e = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=len(ims), stage_launches=True)
    try:
        assert e.frozen_info() == NOTHING_FOLDED and e.const_info()["stage"] == -1
        check_stage_local(e, w, ims, dtype, record, "stage_local_224_%s_%s" % (ckpt, dtype))
    finally:
        e.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_stages_locally_vs_fp64_at_side_240(record, dtype):
    """Side 240: stage 4's rows are too wide for its row-blocked kernel (the register-weights kernel runs, float32 pooling), the
    stage pair and stages 5-6 keep theirs: another kernel mix.  Two images: the one that reaches the clamp in every stage on its
    own, whose stage outputs are constant over whole regions, and the textured one, on which a wrong index shows."""
    g = build_graph(6, 240)
    w = CK.live(g, 0, CK.LIVE_GAIN)
    im = parity_set_of(240)[CK.SEAM_IDX]
    e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=len(im), stage_launches=True)
    try:
        assert e.frozen_info() == NOTHING_FOLDED and e.const_info()["stage"] == -1
        check_stage_local(e, w, im, dtype, record, "stage_local_240_live_%s" % dtype)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- b. tuned vs stage launches
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cross_stage_fusion_matches_stage_launches_on_live(graph, checkpoints, ims, dtype, nb):
    """The criteria of test_hip_fused.test_cross_stage_fusion_is_bit_identical_to_stage_launches, on values that reach the clamp."""
    w = checkpoints["live"]
    fused = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=nb)
    plain = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
    try:
        assert fused.launch_groups()[:2] == [[0, 1], [2, 3]] and fused.frozen_info() == NOTHING_FOLDED
        ids_f, probs_f = fused.forward_u8(ims[:nb])
        ids_p, probs_p = plain.forward_u8(ims[:nb])
        a1, b1 = fused.tap("s1.bn", nb), plain.tap("s1.bn", nb)
        bad = np.argwhere(a1 != b1)
        assert bad.size == 0, ("s1", dtype, len(bad), bad[:8].tolist(), float(np.abs(a1 - b1).max()))
        _same_up_to_sum_order(fused.tap("s3.bn2", nb), plain.tap("s3.bn2", nb), dtype, "s3.bn2")
        _downstream_same(fused, plain, ("s8.bn", "s9.bn2", "d3.relu"), nb, dtype, probs_f, probs_p, ids_f, ids_p)
    finally:
        fused.close()
        plain.close()


def test_generic_kernels_stages_locally_vs_fp64(graph, checkpoints, ims, record):
    """RN_FLAG_GENERIC_KERNELS: every stage on the generic kernel (float32 pooling, no division by 6, plain rounding)."""
    w = checkpoints["live"]
    e = _capi.Engine(graph, w, device=0, dtype="bf16", max_batch=len(ims), generic_kernels=True)
    try:
        check_stage_local(e, w, ims, "bf16", record, "stage_local_224_live_bf16_generic_kernels", tuned=False)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- c. one-launch back end
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_launch_back_end_on_live_is_bit_identical_to_the_split_launches(graph, checkpoints, parity_images, dtype):
    """128 images (four tiled): stages 6-9 and the head as one launch per image, stages 6 and 7 resident in LDS, on a checkpoint
    where 17-31 % of the values of stages 6-9 sit at the clamp -- against the same handle type at batch 4 (three launches)."""
    w = checkpoints["live"]
    four = parity_images[CK.PARITY_IDX + [52]]
    pick = np.arange(128) % 4
    big = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=128)
    small = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=4)
    try:
        ids, probs = big.forward_u8(four[pick])
        assert big.launch_groups()[-1] == [6, 7, 8, 9]
        ids4, probs4 = small.forward_u8(four)
        assert small.launch_groups()[-1] != [6, 7, 8, 9]
        for name in ("s8.bn", "s9.bn2", "d3.relu"):
            np.testing.assert_array_equal(big.tap(name, 128), small.tap(name, 4)[pick], err_msg=name)
        np.testing.assert_array_equal(probs, probs4[pick])
        np.testing.assert_array_equal(ids, ids4[pick])
        assert np.isfinite(probs).all()
    finally:
        big.close()
        small.close()


# ---------------------------------------------------------------------------------------------- d. head width
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", [1, 2, 10, 64])
def test_head_width_head_locally_vs_fp64(parity_images, record, nc, dtype):
    """1, 2, 10 and 64 classes (the softmax / argmax butterflies span 1, 2, 16 and 64 lanes) at batch 3 -- the tail kernel on the
    16-bit handle -- and at 128 tiled images, where the one-launch back end carries the head."""
    g = build_graph(nc, 224)
    w = CK.live(g, 0, CK.LIVE_GAIN)
    four = parity_images[CK.PARITY_IDX + [52]]
    e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=128)
    try:
        ids3, probs3 = e.forward_u8(four[:3])
        if dtype != "f32":
            assert e.launch_groups()[-1] == [8, 9]
        check_head_local(e, w, 3, ids3, probs3, record, "head_local_nc%d_%s_batch3" % (nc, dtype))
        ids, probs = e.forward_u8(four[np.arange(128) % 4])
        if dtype != "f32":
            assert e.launch_groups()[-1] == [6, 7, 8, 9]
        check_head_local(e, w, 128, ids, probs, record, "head_local_nc%d_%s_batch128" % (nc, dtype))
        # the same image gives the same head result in both calls and in every copy
        np.testing.assert_array_equal(probs[:3], probs3)
        np.testing.assert_array_equal(probs[4:128], probs[np.arange(124) % 4])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- e. float32 handles
@pytest.mark.parametrize("ckpt", ["live", "init_scale"])
def test_f32_handles_vs_fp64(graph, checkpoints, ims, refs, record, ckpt):
    w = checkpoints[ckpt]
    r64, r32 = refs(ckpt)
    n = len(ims)
    pn = _capi.Engine(graph, w, device=0, dtype="f32", max_batch=n, taps=True)
    mm = _capi.Engine(graph, w, device=0, dtype="f32", max_batch=n)
    try:
        assert pn.frozen_info() == NOTHING_FOLDED and mm.frozen_info() == NOTHING_FOLDED
        ids_a, probs_a = pn.forward_u8(ims)
        ids_b, probs_b = mm.forward_u8(ims)
        names = R.node_names()
        assert set(names) == set(pn.nodes())
        _check_nodes(pn, names, n, r64, r32, record, "f32_per_node_%s" % ckpt)
        _check_nodes(mm, STAGE_OUT + ["d3.relu"], n, r64, r32, record, "f32_matrix_core_%s" % ckpt)
        rows = {}
        for name in STAGE_OUT:
            a, b = pn.tap(name, n), mm.tap(name, n)
            rows[name] = float(np.abs(a - b).max() / max(float(np.abs(a).max()), 1e-3))
        record(SECTION, "f32_matrix_core_vs_per_node_%s" % ckpt, rows)
        print("matrix cores vs per node:", " ".join("%s=%.2g" % kv for kv in rows.items()))
        assert all(v <= 2e-5 for v in rows.values()), rows
        lg = np.sort(r64["logits"], axis=1)
        safe = lg[:, -1] - lg[:, -2] > 1e-3
        np.testing.assert_array_equal(ids_a[safe], r64["ids"][safe])
        np.testing.assert_array_equal(ids_b[safe], r64["ids"][safe])
    finally:
        pn.close()
        mm.close()


# ---------------------------------------------------------------------------------------------- f. the whole 16-bit chain
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_16bit_whole_chain_vs_fp64_recorded(graph, checkpoints, ims, refs, record, dtype):
    """End to end on `live`, default handle: how 16-bit error compounds when the BN scales are O(1) is RECORDED (per-stage relative
    error, max |dlogit|, id flips with their float64 margins); asserted: ids agree wherever the float64 top-2 margin exceeds 0.5."""
    w = checkpoints["live"]
    r64, _ = refs("live")
    n = len(ims)
    e = _capi.Engine(graph, w, device=0, dtype=dtype, max_batch=n)
    try:
        ids, probs = e.forward_u8(ims)
        rels = {name: SR.rel_err(e.tap(name, n), r64["taps"][name]) for name in STAGE_OUT if name not in FUSED_AWAY}
        logits = e.tap("d3.relu", n)
        lg = np.sort(r64["logits"], axis=1)
        margin = lg[:, -1] - lg[:, -2]
        flips = [{"image": int(i), "fp64_margin": float(margin[i]), "gpu_id": int(ids[i]), "fp64_id": int(r64["ids"][i])}
                 for i in np.flatnonzero(ids != r64["ids"])]
        row = {"stage_rel_err": rels, "max_abs_dlogit_vs_fp64": float(np.abs(logits - r64["logits"]).max()),
               "max_abs_dprob_vs_fp64": float(np.abs(probs - r64["taps"]["softmax"]).max()), "fp64_top2_margins": margin.tolist(),
               "id_flips": flips}
        print(dtype, row)
        record(SECTION, "whole_chain_224_live_%s" % dtype, row)
        assert np.isfinite(logits).all() and np.isfinite(probs).all()
        safe = margin > WHOLE_CHAIN_MARGIN
        assert safe.sum() >= 2
        np.testing.assert_array_equal(ids[safe], r64["ids"][safe])
    finally:
        e.close()
