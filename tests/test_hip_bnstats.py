"""GPU parity of the batch-statistics forward pass (RN_FLAG_BATCH_STATS) and of BN recalibration with the fp64 restatement
tests/bn_batch_ref.py, through the C ABI.

Tolerance per tensor = max(1e-4 * abs-max of the fp64 tensor, 4 x the float32 CPU restatement's own max deviation from fp64 on that
tensor): the first term is the float32 rule of test_hip_f32.py, the second is computed here from the same inputs; the factor 4
allows for another summation order and nothing else.  Moments: the scale is the abs-max of the BN's input (mean) and its square
(variance); counts are exact.

Every figure is printed and recorded (`record` -> the parity report) before it is asserted; NOTES.md, "Batch-statistics BN", says
what has been measured on an MI355X so far.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_batch_ref
from oracle import roomnet_ref as R
from parity_bounds import _tol
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet, _initializer_values

pytestmark = pytest.mark.gpu

INIT_SEED = 0          # _initializer_values seed of the init()-scale cases (checked on the CPU against the exclusion cap below)
ID_MARGIN = 0.2        # the project's id_margin_16bit
RN_E_INVALID, RN_E_STATE, RN_E_RANGE = -1, -4, -5


def _refs(weights, ims):
    return bn_batch_ref.forward(weights, ims), bn_batch_ref.forward(weights, ims, dtype=torch.float32)


def _check_call(eng, ims, r64, r32, record, key):
    """One forward call against the restatement: every BN output, the logits, the 16 moment triples.  Figures are printed and
    recorded before anything is asserted."""
    n = len(ims)
    eng.forward_u8(ims)
    stats = eng.bn_batch_stats()
    assert eng.bn_nodes() == [node for _, node in r64["bn_nodes"]]
    rows, bad = {}, []
    for bn, node in r64["bn_nodes"]:
        want = r64["bn"][node]
        got = eng.tap(node, n)
        assert got.shape == want.shape, node
        err, tol = float(np.abs(got - want).max()), _tol(want, r32["bn"][node])
        mean, var, count = stats[bn]
        m64, v64, c64 = r64["stats"][bn]
        scale = r64["in_absmax"][bn]
        em, tm = float(np.abs(mean - m64).max()), _tol(m64, r32["stats"][bn][0], scale)
        ev, tv = float(np.abs(var - v64).max()), _tol(v64, r32["stats"][bn][1], scale * scale)
        rows[node] = {"out_err": err, "out_tol": tol, "mean_err": em, "mean_tol": tm, "var_err": ev, "var_tol": tv, "count": count}
        print("%-7s out %.3g / %.3g   mean %.3g / %.3g   var %.3g / %.3g   count %d" % (node, err, tol, em, tm, ev, tv, count))
        if err > tol or em > tm or ev > tv or count != c64:
            bad.append(node)
        assert mean.dtype == np.float32 and var.dtype == np.float32 and (var >= 0).all()
    logits = eng.tap("d3.relu", n)
    el, tl = float(np.abs(logits - r64["logits"]).max()), _tol(r64["logits"], r32["logits"])
    rows["logits"] = {"out_err": el, "out_tol": tl}
    print("logits  out %.3g / %.3g" % (el, tl))
    record("bn_batch_stats_224", key, rows)
    assert not bad, bad
    assert el <= tl
    return stats


@pytest.fixture(scope="module")
def graph():
    return build_graph(6, 224)


@pytest.fixture(scope="module")
def engine(weights, graph):
    e = _capi.Engine(graph, weights, device=0, dtype="f32", max_batch=16, taps=True, batch_stats=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def shipped_refs(weights, parity_images):
    return _refs(weights, parity_images[:16])


def test_shipped_checkpoint_16_images_vs_fp64(engine, parity_images, shipped_refs, record):
    r64, r32 = shipped_refs
    stats = _check_call(engine, parity_images[:16], r64, r32, record, "shipped_checkpoint_16_images")
    assert list(stats) == [bn for bn, _ in r64["bn_nodes"]]
    assert engine.frozen_info() == {"pair_channels_not_convolved": 0, "pair_channels_proven_frozen": 0, "residual_stage_folded": -1,
                                    "residual_stage_live_quarters": 4}
    assert engine.const_info()["stage"] == -1


def test_init_scale_weights_8_images_vs_fp64(graph, parity_images, record):
    w = _initializer_values(graph, INIT_SEED)
    ims = parity_images[:8]
    r64, r32 = _refs(w, ims)
    e = _capi.Engine(graph, w, device=0, dtype="f32", max_batch=8, taps=True, batch_stats=True)
    try:
        _check_call(e, ims, r64, r32, record, "init_weights_8_images")
    finally:
        e.close()


def test_one_image_call(engine, weights, parity_images, record):
    """n = 1: the dense BNs see one value per channel -- variance 0, output beta (up to the rounding of x * inv in
    x * inv + (beta - mean * inv)); the conv-side BNs normalise over the image's pixels."""
    ims = parity_images[5:6]
    r64, r32 = _refs(weights, ims)
    stats = _check_call(engine, ims, r64, r32, record, "shipped_checkpoint_1_image")
    for d, bn in enumerate(["batch_normalization_13", "batch_normalization_14", "batch_normalization_15"]):
        mean, var, count = stats[bn]
        assert count == 1
        np.testing.assert_array_equal(var, 0.0)
        np.testing.assert_array_equal(mean, engine.tap("d%d.relu" % d, 1)[0])
        beta = weights[bn + "/beta"]
        inv = weights[bn + "/gamma"] / np.sqrt(np.float32(1e-3))
        # (two float32 roundings, of beta - x * inv and of the sum: an ulp of the larger of |x * inv| and |beta|)
        atol = float(2.0 ** -22 * (np.abs(mean * inv).max() + np.abs(beta).max())) + 1e-12
        np.testing.assert_allclose(engine.tap("d%d.bn" % d, 1)[0], beta, rtol=0, atol=atol)


def test_moments_as_moving_statistics_tie_to_the_inference_path(engine, weights, graph, parity_images):
    """The batch moments of a call written into the checkpoint as moving_*: a plain per-node float32 handle on that checkpoint runs
    the same kernels on the same table (bound of test_hip_f32.py: 2e-5 of the abs-max)."""
    ims = parity_images[:16]
    engine.forward_u8(ims)
    stats = engine.bn_batch_stats()
    got = {node: engine.tap(node, 16).copy() for node in engine.bn_nodes()}
    w = dict(weights)
    for bn, (mean, var, _count) in stats.items():
        w[bn + "/moving_mean"], w[bn + "/moving_variance"] = mean, var
    plain = _capi.Engine(graph, w, device=0, dtype="f32", max_batch=16, taps=True)
    try:
        plain.forward_u8(ims)
        for node, a in got.items():
            b = plain.tap(node, 16)
            err, bound = float(np.abs(a - b).max()), 2e-5 * max(float(np.abs(b).max()), 1e-3)
            print("%-7s %.3g / %.3g" % (node, err, bound))
            assert err <= bound, node
    finally:
        plain.close()


def test_deterministic_and_batch_dependent(engine, weights, graph, parity_images, shipped_refs):
    r64, r32 = shipped_refs
    ims = parity_images[:16]
    ids_a, probs_a = engine.forward_u8(ims)
    stats_a = engine.bn_batch_stats()
    taps_a = {node: engine.tap(node, 16).copy() for node in engine.bn_nodes() + ["d3.relu"]}
    ids_b, probs_b = engine.forward_u8(ims)
    stats_b = engine.bn_batch_stats()
    np.testing.assert_array_equal(probs_a, probs_b)                       # two calls on one batch: the same bits
    np.testing.assert_array_equal(ids_a, ids_b)
    for bn in stats_a:
        np.testing.assert_array_equal(stats_a[bn][0], stats_b[bn][0])
        np.testing.assert_array_equal(stats_a[bn][1], stats_b[bn][1])
    for node, a in taps_a.items():
        np.testing.assert_array_equal(a, engine.tap(node, 16), err_msg=node)
    # a handle that shares its scratch buffers, the pipelined entry and the float entry run the same launches
    e2 = _capi.Engine(graph, weights, device=0, dtype="f32", max_batch=16, batch_stats=True)
    try:
        ids_c, probs_c = e2.forward_u8(ims)
        np.testing.assert_array_equal(probs_a, probs_c)
        e2.submit_u8(ims, 0)
        ids_d, probs_d = e2.collect(0)
        np.testing.assert_array_equal(probs_a, probs_d)
        ids_e, probs_e = e2.forward_f32(R.preprocess_batch(ims))
        np.testing.assert_array_equal(probs_a, probs_e)
        np.testing.assert_array_equal(e2.tap("s9.bn2", 16), taps_a["s9.bn2"])
    finally:
        e2.close()
    # image 0 alone is another computation than image 0 inside the batch
    engine.forward_u8(ims[:1])
    assert float(np.abs(engine.tap("d3.relu", 1)[0] - taps_a["d3.relu"][0]).max()) > 1e-3
    assert float(np.abs(engine.tap("s0.bn", 1)[0] - taps_a["s0.bn"][0]).max()) > 1e-3
    # a permuted batch gives the permuted outputs (the moments' merge order changes: within the node tolerance)
    perm = np.random.default_rng(7).permutation(16)
    engine.forward_u8(ims[perm])
    for node, a in taps_a.items():
        want = r64["logits"] if node == "d3.relu" else r64["bn"][node]
        tol = _tol(want, r32["logits"] if node == "d3.relu" else r32["bn"][node])
        assert float(np.abs(engine.tap(node, 16) - a[perm]).max()) <= tol, node


def test_600_input_long_flatten(weights, record):
    """flat_len 3136: the first dense block splits its K sum over 1024 threads; column counts and tensor lengths differ everywhere."""
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, 600)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    ims = parity_batch(600, seed=1)[[14, 22, 37]]
    r64, r32 = _refs(w, ims)
    e = _capi.Engine(g, w, device=0, dtype="f32", max_batch=3, taps=True, batch_stats=True)
    try:
        _check_call(e, ims, r64, r32, record, "shipped_checkpoint_600_3_images")
    finally:
        e.close()


def test_recalibrate_bn_momentum_update_is_the_references_rule(engine, weights, graph, parity_images, tmp_path, monkeypatch):
    ims = parity_images[:16]
    engine.forward_u8(ims)
    stats = engine.bn_batch_stats()                                     # (deterministic: the model's own engine computes the same bits)
    nn = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, dtype="f32", max_batch=16)
    nn.init()
    nn.set_variables(weights)
    new = nn.recalibrate_bn([ims], momentum=0.99)
    assert len(new) == 32 and nn.sess.engine is None and nn.sess.bs_engine is None
    for i, (bn, (mean, var, count)) in enumerate(stats.items()):
        v = bn_batch_ref.update_variance(var, count, dense=i >= 13)
        np.testing.assert_array_equal(nn.sess.variables[bn + "/moving_mean"], bn_batch_ref.update(weights[bn + "/moving_mean"], mean, 0.99), err_msg=bn)
        np.testing.assert_array_equal(nn.sess.variables[bn + "/moving_variance"], bn_batch_ref.update(weights[bn + "/moving_variance"], v, 0.99), err_msg=bn)
        np.testing.assert_array_equal(new[bn + "/moving_mean"], nn.sess.variables[bn + "/moving_mean"])
    # a list of images of other sizes goes through the crop + resize preparation; infer_batch_stats follows infer's conventions
    ids, probs = nn.infer_batch_stats(ims)
    assert ids.dtype == np.int64 and probs.shape == (16, 6)
    with pytest.raises(ValueError):
        nn.infer_batch_stats(np.zeros((2, 100, 100, 3), np.uint8))
    with pytest.raises(ValueError, match="max_batch"):
        nn.infer_batch_stats(np.zeros((17, 224, 224, 3), np.uint8))
    nn.recalibrate_bn([[np.zeros((300, 400, 3), np.uint8) + 7 * k for k in range(4)]], momentum=0.5)
    # save() / load(): the same bits
    monkeypatch.chdir(tmp_path)
    nn.save()
    nn2 = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True)
    nn2.load(str(tmp_path / "roomnet"))
    for k, v in nn.sess.variables.items():
        np.testing.assert_array_equal(nn2.sess.variables[k], v, err_msg=k)


def test_recalibrated_init_model_classifies_in_bf16(graph, parity_images, record):
    """init() leaves moving_mean 0 / moving_variance 1: recalibrated over four batches of 8 (momentum=None) the model is usable, and
    a bf16 engine on the new statistics agrees in class id with the fp64 restatement on the same statistics wherever the fp64
    top-2 logit gap is >= 0.2; at most a quarter of the images may fall under that margin."""
    ims = parity_images[:32]
    nn = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, dtype="bf16", max_batch=32)
    nn.init()
    nn.set_variables(_initializer_values(graph, INIT_SEED))
    new = nn.recalibrate_bn([ims[i:i + 8] for i in range(0, 32, 8)], momentum=None)
    assert len(new) == 32
    ids, probs = nn.infer(ims)
    ref = bn_batch_ref.forward(nn.sess.variables, ims, moments="moving")
    srt = np.sort(ref["logits"], 1)
    gap = srt[:, -1] - srt[:, -2]
    safe = gap >= ID_MARGIN
    ref_ids = ref["logits"].argmax(1)
    wrong = [int(i) for i in np.flatnonzero(safe) if ids[i] != ref_ids[i]]
    record("bn_batch_stats_224", "recalibrated_init_model_bf16", {
        "images": 32, "excluded_below_margin": int((~safe).sum()), "id_margin": ID_MARGIN, "disagreements": wrong,
        "gaps_of_disagreements": [float(gap[i]) for i in wrong], "fp64_classes": sorted(set(ref_ids.tolist()))})
    print("excluded %d of 32, disagreements %s" % (int((~safe).sum()), wrong))
    nn.sess.close()
    assert int((~safe).sum()) <= 8
    assert not wrong


def test_error_conventions(engine, weights, graph, parity_images):
    lib = engine.lib
    with pytest.raises(ValueError, match="RN_FLAG_BATCH_STATS"):                      # RN_E_INVALID
        _capi.Engine(graph, weights, device=0, dtype="bf16", max_batch=2, batch_stats=True)
    fresh = _capi.Engine(graph, weights, device=0, dtype="f32", max_batch=2, batch_stats=True)
    plain = _capi.Engine(graph, weights, device=0, dtype="f32", max_batch=2)
    try:
        mean, var, count = np.empty(8, np.float32), np.empty(8, np.float32), C.c_int64(0)
        rc = lib.rn_bn_batch_stats(fresh.handle, 0, mean.ctypes.data, var.ctypes.data, C.byref(count))
        assert rc == RN_E_STATE and b"no forward pass" in lib.rn_last_error()
        ids_a, probs_a = fresh.forward_u8(parity_images[:2])
        assert lib.rn_bn_batch_stats(fresh.handle, 16, mean.ctypes.data, var.ctypes.data, C.byref(count)) == RN_E_RANGE
        assert lib.rn_bn_batch_stats(fresh.handle, -1, mean.ctypes.data, var.ctypes.data, C.byref(count)) == RN_E_RANGE
        info = _capi.rn_node_info()
        assert lib.rn_bn_info(fresh.handle, 16, C.byref(info)) == RN_E_RANGE
        assert lib.rn_bn_count(fresh.handle) == 16
        assert lib.rn_bn_batch_stats(fresh.handle, 0, mean.ctypes.data, var.ctypes.data, C.byref(count)) == 0
        assert count.value == 2 * 220 * 220                   # s0.bn at 224: conv 222, pool 3/1 220
        with pytest.raises(_capi.RoomNetLibraryError, match="RN_FLAG_BATCH_STATS"):   # RN_E_STATE
            fresh.grad_cam(parity_images[:2])
        assert lib.rn_bn_count(plain.handle) == RN_E_STATE
        assert lib.rn_bn_batch_stats(plain.handle, 0, mean.ctypes.data, var.ctypes.data, C.byref(count)) == RN_E_STATE
        with pytest.raises(_capi.RoomNetLibraryError):
            plain.bn_batch_stats()
        with pytest.raises(_capi.RoomNetLibraryError, match="TAPS"):                  # scratch-sharing handle: as on any per-node handle
            fresh.tap("s3.conv", 2)
        ids_b, probs_b = fresh.forward_u8(parity_images[:2])                          # the handle stays usable after each
        np.testing.assert_array_equal(probs_a, probs_b)
        plain.forward_u8(parity_images[:2])
    finally:
        fresh.close()
        plain.close()
