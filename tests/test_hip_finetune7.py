"""Depth-3 fine-tuning on the GPU (rn_features_depth_*, rn_ft_create_depth): the s6.bn features against rn_tap, one step's loss and
gradients, a 20-step Adam trajectory and a 100-step learning run against the float64 reference (tests/finetune_ref.py) evaluated
at the handle's own features, determinism, the 300 and 600 geometries without a trunk, depth 2 through the new entry points,
RoomNet.fine_tune end to end, and errors.

The items, the bounds (with where they come from: the project's existing ones, and conv2d_7/kernel's room Amb / n) and the checks are
tests/finetune_harness.py's.  Each test records the kernel's error beside the yardstick's through ``record("finetune7", ...)``."""
import numpy as np
import pytest
import torch

import finetune_harness as H
from finetune_harness import LABELS, LOSS_TOL, RN_E_INVALID, feats, images, starts  # noqa: F401  (fixtures)
from finetune_ref import FineTune7Ref, FineTuneRef
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

_engine = H.engine


# ---- 1. features
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_features_equal_tap(weights, images, dtype):
    eng = _engine(weights, dtype)
    try:
        ids0, probs0 = eng.forward_u8(images)
        for n in (1, 32):
            f = eng.features_u8(images[:n], depth=3)
            assert f.dtype == np.float32 and f.shape == (n, 46, 46, 128)
            if dtype == "f32":
                eng.forward_u8(images[:n])
            else:
                eng.grad_cam(images[:n], layer="s6.bn")
            assert f.tobytes() == eng.tap("s6.bn", n).tobytes(), (dtype, n)
        assert eng.features_shape(depth=3) == (46, 46, 128) and eng.features_shape(depth=2) == (21, 21, 16)
        d_in = torch.from_numpy(images).cuda()
        d_f = torch.empty((32, 46, 46, 128), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.features_u8_device(d_in.data_ptr(), 32, d_f.data_ptr(), depth=3)
        eng.sync()
        assert d_f.cpu().numpy().tobytes() == f.tobytes()
        # depth 2 through the new entry points is rn_features_*
        f2 = eng.features_u8(images)
        g2 = np.empty_like(f2)
        assert eng.lib.rn_features_depth_u8(eng.handle, 2, images.ctypes.data, 32, g2.ctypes.data) == 0
        assert g2.tobytes() == f2.tobytes()
        d_f2 = torch.empty((32, 21, 21, 16), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert eng.lib.rn_features_depth_u8_device(eng.handle, 2, d_in.data_ptr(), 32, d_f2.data_ptr()) == 0
        eng.sync()
        assert d_f2.cpu().numpy().tobytes() == f2.tobytes()
        ids1, probs1 = eng.forward_u8(images)
        assert np.array_equal(ids0, ids1) and probs0.tobytes() == probs1.tobytes()
    finally:
        eng.close()


# ---- 2. one step's loss and gradients
@pytest.mark.parametrize("batch", [1, 3, 32, 45])
@pytest.mark.parametrize("l2", [0.06, 0.0])
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_one_step_loss_and_gradients(starts, feats, record, start, l2, batch):
    idx = np.arange(batch, dtype=np.int32) % 32
    H.check_one_step(starts[start], feats[3], LABELS, idx, l2, record, "finetune7", "one_step_%s_l2_%g_batch_%d" % (start, l2, batch), 3)


# ---- 3. trajectory
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_trajectory_20_steps(starts, feats, record, start):
    """Every parameter within max(0.01 learn_rate, 3 x the float32-torch run's drift) of float64 after 20 steps; the factor 3 allows
    for another summation order.  Float32-torch drift measured on the CPU at the float64 oracle's s6.bn before the first GPU run:
    2.8e-7 from the shipped checkpoint, 2.3e-7 from the fresh head (conv2d_7/kernel: 2.2e-8 and 3.2e-8),
    so the first term, 0.01 learn_rate = 2e-6, is the bound; losses drift 9.7e-7 and 9.1e-7.  At the handle's
    features and on 16 threads the float32-torch run drifts 3.1e-6 from the shipped checkpoint (the bound there is 9.4e-6)
    and 2.3e-7 from the fresh head; the kernel 4.6e-7 and 2.0e-7."""
    H.check_trajectory(starts[start], feats[3], finetune.epoch_indices(32, 8, 20, seed=5), record, "finetune7", "trajectory_%s" % start, 3,
                       drift32_factor=3)


# ---- 4. learning
def test_learning_100_steps(starts, feats, record):
    """100 full-batch steps over the 32 items from the fresh head, as the depth-2 learning test runs them: the GPU run ends within a
    tenth of the float64 run's descent of its last loss, and -- on the CPU reference alone -- training the whole block ends below
    training stages 8-9 on the same items, the point of depth 3 (measured at the float64 oracle's s6.bn: 2.512 -> 0.988 against
    2.505 -> 1.158; at the handle's features float64 ends at 0.729, the GPU at 0.795 and depth 2 at 1.204: the run is sensitive
    to the last bits of its features, and a tenth of the descent, 0.178, is the room it gets).  The float64 run of 100 x 32 conv-7 passes is most of this test's time (about 25 s on 8 threads)."""
    w = starts["fresh"]
    lr, l2, ns = 2e-3, 1e-2, 10000
    index = np.tile(np.arange(32, dtype=np.int32), (100, 1))
    ref = FineTune7Ref(w, 6, 224)
    with torch.no_grad():
        x7 = ref.x7(ref._t(feats[3])).numpy()                 # the depth-2 feature of the same items, conv 7 as loaded
    Lref = ref.train(feats[3], LABELS, index, lr, ns, l2)
    L2 = FineTuneRef(w, 6, 224).train(x7, LABELS, index, lr, ns, l2)
    L0, L1 = float(Lref[0]), float(Lref[-1])
    assert L1 < L0
    tr = H.trainer(w, depth=3, learn_rate=lr, l2_coeff=l2, num_steps=ns)
    try:
        losses = tr.run_host(feats[3], LABELS, index)
    finally:
        tr.close()
    print("learning: float64 depth 3 %.6f -> %.6f, GPU %.6f -> %.6f; float64 depth 2 %.6f -> %.6f"
          % (L0, L1, losses[0], losses[-1], L2[0], L2[-1]))
    record("finetune7", "learning", {"ref_first": L0, "ref_last": L1, "gpu_first": float(losses[0]), "gpu_last": float(losses[-1]),
                                     "ref_depth2_first": float(L2[0]), "ref_depth2_last": float(L2[-1])})
    assert abs(float(losses[-1]) - L1) <= 0.1 * (L0 - L1)
    assert L1 < float(L2[-1])


# ---- 5. determinism
def test_determinism_and_step_splitting(starts, feats):
    H.check_determinism(starts["fresh"], feats[3], finetune.epoch_indices(32, 8, 20, seed=5), 3)


# ---- 6. odd and large geometry, no trunk and no inference handle
@pytest.mark.parametrize("side,n,s6", [(300, 2, 65), (600, 1, 140)])
def test_odd_and_large_geometry_without_a_trunk(weights, record, side, n, s6):
    """300: conv 7 is 63 x 63, the pool covers 62: the last conv row and column get no gradient.  600: one 140 x 140 x 128 item."""
    g = build_graph(6, side)
    assert finetune.feature_shape(g, depth=3) == (s6, s6, 128)
    w = dict(weights)
    w["dense/kernel"] = np.random.default_rng(side).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    rng = np.random.default_rng(s6)
    x6 = (rng.standard_normal((n, s6, s6, 128)) * 0.5).astype(np.float32)
    y = np.array([2, 5], np.int32)[:n]
    H.check_one_step(w, x6, y, np.arange(n), 0.06, record, "finetune7", "one_step_%d" % side, 3, side=side)
    tr = H.trainer(w, side=side, max_batch=2, depth=3, l2_coeff=0.06)
    try:
        loss, probs, ids = tr.eval_host(x6, y)
        ref = FineTune7Ref(w, 6, side)
        assert np.abs(probs - ref.probs(x6)).max() <= 1e-5 and probs.shape == (n, 6) and ids.shape == (n,)
        assert abs(loss - float(ref.loss(x6, y, 0.06))) <= LOSS_TOL
    finally:
        tr.close()


# ---- 7. depth 2 is untouched
def test_depth_2_through_the_new_entry_point(starts, feats):
    w, f2 = starts["fresh"], feats[2]
    index = finetune.epoch_indices(32, 8, 5, seed=3)
    out = []
    for depth_arg in (None, 2):
        # (Trainer(depth=2) calls rn_ft_create; the new entry point is called here directly)
        tr = _capi.Trainer(build_graph(6, 224), w, device=0, max_batch=8, learn_rate=2e-4, l2_coeff=0.06)
        if depth_arg is not None:
            tr.close()
            packed = _capi._Packed(tr.graph, w)
            cfg = _capi.rn_ft_config(2e-4, 0.068, 10000, 0, 0.06, 0.9, 0.999, 1e-8)
            h = _capi.C.c_void_p()
            assert tr.lib.rn_ft_create_depth(_capi.C.byref(packed.w), 0, 8, _capi.C.byref(cfg), 2, _capi.C.byref(h)) == 0
            tr._h = h
        try:
            assert tr.lib.rn_ft_depth(tr.handle) == 2
            assert [n for n, _ in tr.variables()] == finetune.trained_variables(tr.graph) and len(tr.variables()) == 19
            losses = tr.run_host(f2, LABELS, index)
            out.append((losses, tr.read(), tr.read(_capi.RN_FT_GRAD), tr.read(_capi.RN_FT_ADAM_M), tr.read(_capi.RN_FT_ADAM_V)))
        finally:
            tr.close()
    a, b = out
    assert a[0].tobytes() == b[0].tobytes()
    for k in (1, 2, 3, 4):
        for n in a[k]:
            assert a[k][n].tobytes() == b[k][n].tobytes(), n


# ---- 8. end to end through RoomNet
def test_fine_tune_end_to_end(weights, images, tmp_path, monkeypatch):
    H.check_end_to_end(weights, images, tmp_path, monkeypatch, 3)


# ---- 9. errors
def test_errors_leave_trainer_and_handle_usable(weights, feats, images):
    g = build_graph(6, 224)
    packed = _capi._Packed(g, weights)
    cfg = _capi.rn_ft_config(1e-4, 0.068, 10000, 0, 0.01, 0.9, 0.999, 1e-8)
    lib = _capi.load_library()
    for depth in (1, 4):
        h = _capi.C.c_void_p()
        assert lib.rn_ft_create_depth(_capi.C.byref(packed.w), 0, 8, _capi.C.byref(cfg), depth, _capi.C.byref(h)) == RN_E_INVALID
        assert not h.value and b"depth" in lib.rn_last_error()
        with pytest.raises(ValueError, match="depth"):
            H.trainer(weights, depth=depth)
    H.check_run_errors(weights, feats[3], 3)
    eng = _engine(weights, "bf16", max_batch=4)
    try:
        side, ch = _capi.C.c_int(0), _capi.C.c_int(0)
        for depth in (1, 4):
            assert eng.lib.rn_features_depth_shape(eng.handle, depth, _capi.C.byref(side), _capi.C.byref(ch)) == RN_E_INVALID
            assert eng.lib.rn_features_depth_u8_device(eng.handle, depth, 1, 1, 1) == RN_E_INVALID
            with pytest.raises(ValueError, match="depth"):
                eng.features_u8(images[:1], depth=depth)
        ids, probs = eng.forward_u8(images[:4])
        with pytest.raises(ValueError, match="out of range"):
            eng.features_u8_device(1, 5, 1, depth=3)
        ids2, probs2 = eng.forward_u8(images[:4])
        f = eng.features_u8(images[:4], depth=3)
        ids3, probs3 = eng.forward_u8(images[:4])
        assert f.shape == (4, 46, 46, 128) and probs.tobytes() == probs2.tobytes() == probs3.tobytes()
    finally:
        eng.close()
