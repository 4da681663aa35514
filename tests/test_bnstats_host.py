"""Host side of batch-statistics BN and BN recalibration (no GPU): the update arithmetic of roomnet_amd/bnstats.py against the
restatement's own (tests/bn_batch_ref.py), the new C-ABI surface in header and binding, argument checks that happen before a device
is touched, and a self-check of the restatement against the committed fp64 goldens."""
import os
import re

import numpy as np
import pytest
import torch

import bn_batch_ref
from conftest import ROOT
from roomnet_amd import _capi, bnstats
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet

BN_NAMES = ["batch_normalization"] + ["batch_normalization_%d" % i for i in range(1, 16)]


@pytest.fixture(scope="module")
def two_batches(weights, parity_images):
    """fp64 batch moments of two small batches on the shipped checkpoint."""
    return [bn_batch_ref.forward(weights, parity_images[i:i + 3])["stats"] for i in (0, 3)]


def test_bn_order_and_ranks_follow_the_variable_order():
    ranks = bnstats.bn_ranks(build_graph(6, 224))
    assert list(ranks) == BN_NAMES
    assert [ranks[k] for k in BN_NAMES] == [4] * 13 + [2] * 3


@pytest.mark.parametrize("momentum", [0.99, 0.0])
def test_moving_update_and_variance_match_the_restatement(weights, two_batches, momentum):
    g = build_graph(6, 224)
    ranks = bnstats.bn_ranks(g)
    got = bnstats.updated_statistics(g, weights, two_batches, momentum)
    assert sorted(got) == sorted(k + s for k in BN_NAMES for s in ("/moving_mean", "/moving_variance"))
    for bn in ("batch_normalization", "batch_normalization_4", "batch_normalization_6", "batch_normalization_13", "batch_normalization_15"):
        mm, mv = weights[bn + "/moving_mean"], weights[bn + "/moving_variance"]
        for st in two_batches:
            mean, var, count = st[bn]
            v = bn_batch_ref.update_variance(var, count, dense=ranks[bn] == 2)
            np.testing.assert_array_equal(bnstats.variance_for_update(var, count, ranks[bn]), v)
            np.testing.assert_array_equal(bnstats.moving_update(mm, mean, momentum), bn_batch_ref.update(mm, mean, momentum))
            mm, mv = bn_batch_ref.update(mm, mean, momentum), bn_batch_ref.update(mv, v, momentum)
        np.testing.assert_array_equal(got[bn + "/moving_mean"], mm)
        np.testing.assert_array_equal(got[bn + "/moving_variance"], mv)
        assert got[bn + "/moving_mean"].dtype == np.float32


def test_momentum_none_is_the_equal_weight_average(weights, two_batches):
    g = build_graph(6, 224)
    ranks = bnstats.bn_ranks(g)
    got = bnstats.updated_statistics(g, weights, two_batches, None)
    for bn in BN_NAMES:
        mean = np.mean([np.asarray(st[bn][0], np.float32).astype(np.float64) for st in two_batches], 0)
        var = np.mean([bn_batch_ref.update_variance(st[bn][1], st[bn][2], dense=ranks[bn] == 2).astype(np.float64) for st in two_batches], 0)
        np.testing.assert_allclose(got[bn + "/moving_mean"], mean, rtol=1e-7, atol=1e-30)
        np.testing.assert_allclose(got[bn + "/moving_variance"], var, rtol=1e-7, atol=1e-30)


def test_variance_for_update_edges():
    v = np.array([0.25, 4.0], np.float32)
    np.testing.assert_array_equal(bnstats.variance_for_update(v, 1, 4), v)                      # N = 1: factor 1
    np.testing.assert_array_equal(bnstats.variance_for_update(v, 2, 4), v * np.float32(2.0))
    np.testing.assert_array_equal(bnstats.variance_for_update(v, 2, 2), v)
    with pytest.raises(ValueError):
        bnstats.variance_for_update(v, 2, 3)
    # the decay is float32(1.0 - momentum) with the subtraction in double: 1 - 0.99 is not 0.01
    assert np.float32(1.0 - 0.99) == np.float32(0.010000000000000009)
    np.testing.assert_array_equal(bnstats.moving_update([1.0], [3.0], 0.99), np.float32(1.0) - (np.float32(1.0) - np.float32(3.0)) * np.float32(1.0 - 0.99))


def test_header_and_binding_carry_the_new_surface():
    text = open(os.path.join(ROOT, "include", "roomnet_hip.h")).read()
    assert re.search(r"#define\s+RN_FLAG_BATCH_STATS\s+64u", text)
    assert _capi.RN_FLAG_BATCH_STATS == 64
    for name in ("rn_bn_count", "rn_bn_info", "rn_bn_batch_stats"):
        assert re.search(r"^RN_API int %s\(" % name, text, flags=re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(_capi.load_library(), name)


@pytest.mark.parametrize("kwargs", [dict(dtype="bf16"), dict(dtype="f16"), dict(dtype="f32", stage_launches=True),
                                    dict(dtype="f32", generic_kernels=True), dict(dtype="f32", pair32=True)])
def test_flag_combinations_are_refused_before_a_device_is_touched(weights, kwargs):
    with pytest.raises(ValueError, match="RN_FLAG_BATCH_STATS|RN_FLAG_PAIR_32X32"):
        _capi.Engine(build_graph(6, 224), weights, device=0, max_batch=2, batch_stats=True, lib_path=_capi.LIB_PATH, **kwargs)


def test_recalibrate_bn_needs_batches_and_the_constructor_still_refuses():
    nn = RoomNet(6, im_side=224, compute_bn_mean_var=False)
    nn.init()
    with pytest.raises(ValueError, match="no batches"):
        nn.recalibrate_bn([])
    with pytest.raises(ValueError, match="no batches"):
        nn.recalibrate_bn(iter(()), momentum=None)
    with pytest.raises(NotImplementedError):
        RoomNet(6, im_side=224)


def test_restatement_with_moving_statistics_is_the_inference_graph(weights, parity_images, golden_parity):
    """With the moments replaced by the checkpoint's moving statistics the restatement is the graph of the committed fp64 goldens."""
    ref = bn_batch_ref.forward(weights, parity_images[:16], moments="moving")
    np.testing.assert_allclose(ref["logits"], golden_parity["logits_f64"][:16], atol=1e-9, rtol=0)
    assert [n for _, n in ref["bn_nodes"]] == ["s0.bn", "s1.bn", "s2.bn", "s3.bn", "s3.bn2", "s4.bn", "s5.bn", "s5.bn2", "s6.bn", "s7.bn",
                                               "s8.bn", "s9.bn", "s9.bn2", "d0.bn", "d1.bn", "d2.bn"]
    assert [b for b, _ in ref["bn_nodes"]] == BN_NAMES


def test_restatement_float32_floor_and_batch_dependence(weights, parity_images):
    """The float32 run of the same code is the noise floor of the GPU tolerance: well inside 1e-4 of each tensor's abs-max."""
    ims = parity_images[:4]
    r64 = bn_batch_ref.forward(weights, ims)
    r32 = bn_batch_ref.forward(weights, ims, dtype=torch.float32)
    for node, want in r64["bn"].items():
        assert float(np.abs(r32["bn"][node] - want).max()) <= 1e-4 * max(float(np.abs(want).max()), 1e-3), node
    moving = bn_batch_ref.forward(weights, ims, moments="moving")
    assert float(np.abs(moving["bn"]["s0.bn"] - r64["bn"]["s0.bn"]).max()) > 1e-3      # batch moments are not the moving ones
    one = bn_batch_ref.forward(weights, ims[:1])
    for (bn, node) in one["bn_nodes"][-3:]:                                             # n = 1 on a dense BN: variance 0, y = beta
        np.testing.assert_array_equal(one["stats"][bn][1], 0.0)
        np.testing.assert_allclose(one["bn"][node][0], weights[bn + "/beta"], atol=1e-12, rtol=0)
