"""Fine-tuning on the GPU (rn_features_*, rn_ft_*): the features against rn_tap, one step's loss and gradients, a 20-step Adam
trajectory and a 100-step learning run against the float64 reference (tests/finetune_ref.py) evaluated at the handle's own
features, determinism, the 600 geometry without a trunk, RoomNet.fine_tune end to end, and errors.

The items, the bounds (with where they come from) and the checks are tests/finetune_harness.py's; here the trajectory's bound on the
parameters is 0.01 learn_rate = 2e-6.  Each test records the kernel's error beside the yardstick's through
``record("finetune", ...)``."""
import numpy as np
import pytest
import torch

import finetune_harness as H
from finetune_harness import LABELS, feats, images, starts  # noqa: F401  (fixtures)
from finetune_ref import FineTuneRef
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet

pytestmark = pytest.mark.gpu

_engine = H.engine


# ---- 1. features
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_features_equal_tap(weights, images, dtype):
    eng = _engine(weights, dtype)
    try:
        for n in (1, 32):
            f = eng.features_u8(images[:n])
            assert f.dtype == np.float32 and f.shape == (n, 21, 21, 16)
            if dtype == "f32":
                eng.forward_u8(images[:n])
            else:
                eng.grad_cam(images[:n], layer="s7.bn")
            assert f.tobytes() == eng.tap("s7.bn", n).tobytes(), (dtype, n)
        assert eng.features_shape() == (21, 21, 16)
    finally:
        eng.close()


def test_features_where_the_forward_fuses_s7_away(weights, parity_images):
    ims = np.ascontiguousarray(np.concatenate([parity_images] * 4)[:256])
    eng = _engine(weights, "bf16", max_batch=256)
    try:
        ids_f, probs_f = eng.forward_u8(ims)
        f = eng.features_u8(ims)
        assert f.tobytes() == eng.tap("s7.bn", 256).tobytes()        # the feature call's own pass wrote it
        eng.grad_cam(ims, layer="s7.bn")
        assert f.tobytes() == eng.tap("s7.bn", 256).tobytes()
        d_in = torch.from_numpy(ims).cuda()
        d_f = torch.empty((256, 21, 21, 16), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.features_u8_device(d_in.data_ptr(), 256, d_f.data_ptr())
        eng.sync()
        assert d_f.cpu().numpy().tobytes() == f.tobytes()
        ids2, probs2 = eng.forward_u8(ims)
        assert np.array_equal(ids_f, ids2) and probs_f.tobytes() == probs2.tobytes()
    finally:
        eng.close()


# ---- 2. one step's loss and gradients
@pytest.mark.parametrize("batch", [1, 3, 32, 45])
@pytest.mark.parametrize("l2", [0.06, 0.0])
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_one_step_loss_and_gradients(starts, feats, record, start, l2, batch):
    idx = np.arange(batch, dtype=np.int32) % 32
    H.check_one_step(starts[start], feats[2], LABELS, idx, l2, record, "finetune", "one_step_%s_l2_%g_batch_%d" % (start, l2, batch), 2)


# ---- 3. trajectory
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_trajectory_20_steps(starts, feats, record, start):
    H.check_trajectory(starts[start], feats[2], finetune.epoch_indices(32, 8, 20, seed=5), record, "finetune", "trajectory_%s" % start, 2)


# ---- 4. learning
def test_learning_100_steps(starts, feats, record):
    w = starts["fresh"]
    lr, l2, ns = 2e-3, 1e-2, 10000           # (l2 and num_steps: the constructor's defaults)
    index = np.tile(np.arange(32, dtype=np.int32), (100, 1))
    ref = FineTuneRef(w, 6, 224)
    Lref = ref.train(feats[2], LABELS, index, lr, ns, l2)
    L0, L1 = float(Lref[0]), float(Lref[-1])
    assert L1 < L0
    tr = H.trainer(w, learn_rate=lr, l2_coeff=l2, num_steps=ns)
    try:
        losses = tr.run_host(feats[2], LABELS, index)
    finally:
        tr.close()
    print("learning: float64 %.6f -> %.6f, GPU %.6f -> %.6f" % (L0, L1, losses[0], losses[-1]))
    record("finetune", "learning", {"ref_first": L0, "ref_last": L1, "gpu_first": float(losses[0]), "gpu_last": float(losses[-1])})
    assert abs(float(losses[-1]) - L1) <= 0.1 * (L0 - L1)


# ---- 5. determinism
def test_determinism_and_step_splitting(starts, feats):
    H.check_determinism(starts["fresh"], feats[2], finetune.epoch_indices(32, 8, 20, seed=5), 2)


# ---- 6. the 600 geometry, no trunk and no inference handle
def test_600_geometry_without_a_trunk(weights, record):
    g = build_graph(6, 600)
    w = dict(weights)
    w["dense/kernel"] = np.random.default_rng(600).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    rng = np.random.default_rng(68)
    x7 = (rng.standard_normal((2, 68, 68, 16)) * 0.5).astype(np.float32)
    y = np.array([2, 5], np.int32)
    H.check_one_step(w, x7, y, np.arange(2), 0.06, record, "finetune", "one_step_600", 2, side=600)
    tr = H.trainer(w, side=600, max_batch=2, l2_coeff=0.06)
    try:
        _, probs, ids = tr.eval_host(x7)
    finally:
        tr.close()
    assert probs.shape == (2, 6) and ids.shape == (2,)


# ---- 7. end to end through RoomNet
def test_fine_tune_end_to_end(weights, images, tmp_path, monkeypatch):
    H.check_end_to_end(weights, images, tmp_path, monkeypatch, 2)


# ---- 8. errors
def test_errors_leave_trainer_and_handle_usable(weights, feats, images):
    H.check_run_errors(weights, feats[2], 2)
    g = build_graph(6, 224)
    g.dense[1].bn_name = ""                    # a dense block without its BN: the graphs grad-CAM refuses, for the same reason
    with pytest.raises(ValueError, match="not supported on this graph"):
        _capi.Trainer(g, weights)
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dropout_enabled=True, dtype="f32", max_batch=8)
    net.init()
    with pytest.raises(ValueError, match="dropout"):
        net.fine_tune(feats[2], LABELS, steps=1)
    eng = _engine(weights, "bf16", max_batch=4)
    try:
        with pytest.raises(ValueError, match="out of range"):
            eng.features_u8_device(1, 5, 1)
        ids, probs = eng.forward_u8(images[:4])
        f = eng.features_u8(images[:4])
        ids2, probs2 = eng.forward_u8(images[:4])
        assert f.shape == (4, 21, 21, 16) and probs.tobytes() == probs2.tobytes()
    finally:
        eng.close()
