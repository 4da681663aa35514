"""Fine-tuning on the GPU (rn_features_*, rn_ft_*): the features against rn_tap, one step's loss and gradients, a 20-step Adam
trajectory and a 100-step learning run against the float64 reference (tests/finetune_ref.py) evaluated at the handle's own
features, determinism, the 600 geometry without a trunk, RoomNet.fine_tune end to end, and errors.

Bounds (set with the feature, from measurements of the float32 torch run of the same mathematics on the 32 items, both starts):
gradients per variable max|d| / max|g_ref| <= 1e-5 (float32 yardstick: 7.0e-7) and |d loss| <= 5e-6 (2.6e-7); trajectory: every
parameter within 0.01 learn_rate = 2e-6 of float64 after 20 steps (yardstick drift 2.0e-7) and every loss within 5e-6 (8.9e-7).
Each test records the kernel's error beside the yardstick's through ``record("finetune", ...)``."""
import numpy as np
import pytest
import torch

from finetune_ref import FineTuneRef
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet, _initializer_values

pytestmark = pytest.mark.gpu

ITEMS = list(range(0, 8)) + list(range(40, 64))          # 32 parity images, all six classes
LABELS = np.arange(32, dtype=np.int32) % 6
GRAD_TOL, LOSS_TOL = 1e-5, 5e-6
RN_E_RANGE = -5


def _engine(weights, dtype, max_batch=32, **kw):
    return _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=max_batch, **kw)


@pytest.fixture(scope="module")
def images(parity_images):
    return np.ascontiguousarray(parity_images[ITEMS])


@pytest.fixture(scope="module")
def feats(weights, images):
    eng = _engine(weights, "f32")
    try:
        return eng.features_u8(images)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def starts(weights):
    """The two starting points: the shipped checkpoint, and the reference's load() state in training mode -- the conv trunk
    restored, the dense head at its initial values."""
    g = build_graph(6, 224)
    fresh = dict(weights)
    init = _initializer_values(g, seed=1)
    for d in g.dense:
        for name in init:
            if name.startswith(d.name + "/") or (d.bn_name and name.startswith(d.bn_name + "/")):
                fresh[name] = init[name]
    return {"shipped": weights, "fresh": fresh}


def _trainer(w, side=224, max_batch=45, **kw):
    return _capi.Trainer(build_graph(6, side), w, device=0, max_batch=max_batch, **kw)


def _grad_errors(got, ref):
    return {n: float(np.abs(got[n].astype(np.float64) - ref[n]).max() / max(np.abs(ref[n]).max(), 1e-300)) for n in ref}


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
    w = starts[start]
    idx = (np.arange(batch, dtype=np.int32) % 32).reshape(1, batch)
    ref = FineTuneRef(w, 6, 224)
    L, G = ref.loss_and_grads(feats[idx[0]], LABELS[idx[0]], l2)
    L32, G32 = FineTuneRef(w, 6, 224, dtype=torch.float32).loss_and_grads(feats[idx[0]], LABELS[idx[0]], l2)
    tr = _trainer(w, learn_rate=2e-4, l2_coeff=l2)
    try:
        assert [n for n, _ in tr.variables()] == finetune.trained_variables(tr.graph)
        losses = tr.run_host(feats, LABELS, idx)
        got = tr.read(_capi.RN_FT_GRAD)
    finally:
        tr.close()
    err, yard = _grad_errors(got, G), _grad_errors(G32, G)
    dl, dl32 = abs(float(losses[0]) - L), abs(L32 - L)
    print("one step %s l2=%g batch=%d: loss %.9g (ref %.9g) |dloss| %.3g (float32 torch %.3g); worst grad %.3g (float32 torch %.3g)"
          % (start, l2, batch, losses[0], L, dl, dl32, max(err.values()), max(yard.values())))
    record("finetune", "one_step_%s_l2_%g_batch_%d" % (start, l2, batch),
           {"loss_abs": dl, "loss_abs_float32_torch": dl32, "grad_rel_worst": max(err.values()),
            "grad_rel_worst_float32_torch": max(yard.values()), "grad_rel": err})
    assert dl <= LOSS_TOL
    for n in G:
        assert err[n] <= GRAD_TOL, (n, err[n])
        zero = G[n] == 0
        assert not got[n][zero].any(), "%s: %d entries are exactly zero in float64 and not on the GPU" % (n, int(got[n][zero].astype(bool).sum()))


# ---- 3. trajectory
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_trajectory_20_steps(starts, feats, record, start):
    w = starts[start]
    lr, l2, ns = 2e-4, 0.06, 10000
    index = finetune.epoch_indices(32, 8, 20, seed=5)
    ref = FineTuneRef(w, 6, 224)
    Lref = ref.train(feats, LABELS, index, lr, ns, l2)
    ref32 = FineTuneRef(w, 6, 224, dtype=torch.float32)
    L32 = ref32.train(feats, LABELS, index, lr, ns, l2)
    P, P32 = ref.values(), ref32.values()
    tr = _trainer(w, learn_rate=lr, l2_coeff=l2, num_steps=ns)
    d = [tr.upload(feats), tr.upload(LABELS), tr.upload(index)]
    try:
        first = tr.run(d[0], d[1], 32, d[2], 8, 1)
        g1, m1, v1 = tr.read(_capi.RN_FT_GRAD), tr.read(_capi.RN_FT_ADAM_M), tr.read(_capi.RN_FT_ADAM_V)
        rest = tr.run(d[0], d[1], 32, d[2] + 8 * 4, 8, 19)
        got = tr.read()
        assert tr.step_count() == 20
    finally:
        tr.close()
    omb1 = 1.0 - float(np.float32(0.9))
    omb2 = 1.0 - float(np.float32(0.999))
    for n in g1:
        g = g1[n].astype(np.float64)
        # one float32 rounding of each product (and one of g * g); below float32's smallest normal number there is no relative precision
        tiny = float(np.finfo(np.float32).tiny)
        assert np.all(np.abs(m1[n] - omb1 * g) <= 1.2e-7 * np.abs(omb1 * g) + tiny), n
        assert np.all(np.abs(v1[n] - omb2 * g * g) <= 2.4e-7 * omb2 * g * g + tiny), n
    losses = np.concatenate([first, rest])
    drift = max(float(np.abs(got[n] - P[n]).max()) for n in P)
    drift32 = max(float(np.abs(P32[n] - P[n]).max()) for n in P)
    moved = max(float(np.abs(P[n] - np.asarray(w[n], np.float64)).max()) for n in P)
    dl, dl32 = float(np.abs(losses - Lref).max()), float(np.abs(L32 - Lref).max())
    print("trajectory %s: parameter drift %.3g (float32 torch %.3g), parameters moved %.3g = %.1f lr; loss drift %.3g (float32 torch %.3g)"
          % (start, drift, drift32, moved, moved / lr, dl, dl32))
    record("finetune", "trajectory_%s" % start, {"param_abs": drift, "param_abs_float32_torch": drift32, "param_moved": moved,
                                                 "loss_abs": dl, "loss_abs_float32_torch": dl32, "bound_param": 0.01 * lr})
    assert drift <= 0.01 * lr
    assert dl <= LOSS_TOL


# ---- 4. learning
def test_learning_100_steps(starts, feats, record):
    w = starts["fresh"]
    lr, l2, ns = 2e-3, 1e-2, 10000           # (l2 and num_steps: the constructor's defaults)
    index = np.tile(np.arange(32, dtype=np.int32), (100, 1))
    ref = FineTuneRef(w, 6, 224)
    Lref = ref.train(feats, LABELS, index, lr, ns, l2)
    L0, L1 = float(Lref[0]), float(Lref[-1])
    assert L1 < L0
    tr = _trainer(w, learn_rate=lr, l2_coeff=l2, num_steps=ns)
    try:
        losses = tr.run_host(feats, LABELS, index)
    finally:
        tr.close()
    print("learning: float64 %.6f -> %.6f, GPU %.6f -> %.6f" % (L0, L1, losses[0], losses[-1]))
    record("finetune", "learning", {"ref_first": L0, "ref_last": L1, "gpu_first": float(losses[0]), "gpu_last": float(losses[-1])})
    assert abs(float(losses[-1]) - L1) <= 0.1 * (L0 - L1)


# ---- 5. determinism
def test_determinism_and_step_splitting(starts, feats):
    w = starts["fresh"]
    index = finetune.epoch_indices(32, 8, 20, seed=5)

    def run(split):
        tr = _trainer(w, learn_rate=2e-4, l2_coeff=0.06)
        d = [tr.upload(feats), tr.upload(LABELS), tr.upload(index)]
        try:
            if split:
                losses = np.concatenate([tr.run(d[0], d[1], 32, d[2] + 8 * 4 * s, 8, 1) for s in range(20)])
            else:
                losses = tr.run(d[0], d[1], 32, d[2], 8, 20)
            return losses, tr.read(), tr.read(_capi.RN_FT_ADAM_V)
        finally:
            tr.close()

    a, b, c = run(False), run(False), run(True)
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes()
        for k in (1, 2):
            for n in a[k]:
                assert a[k][n].tobytes() == other[k][n].tobytes(), n


# ---- 6. the 600 geometry, no trunk and no inference handle
def test_600_geometry_without_a_trunk(weights, record):
    g = build_graph(6, 600)
    w = dict(weights)
    w["dense/kernel"] = np.random.default_rng(600).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    rng = np.random.default_rng(68)
    x7 = (rng.standard_normal((2, 68, 68, 16)) * 0.5).astype(np.float32)
    y = np.array([2, 5], np.int32)
    l2 = 0.06
    L, G = FineTuneRef(w, 6, 600).loss_and_grads(x7, y, l2)
    L32, G32 = FineTuneRef(w, 6, 600, dtype=torch.float32).loss_and_grads(x7, y, l2)
    tr = _trainer(w, side=600, max_batch=2, l2_coeff=l2)
    try:
        losses = tr.run_host(x7, y, np.array([[0, 1]], np.int32))
        got = tr.read(_capi.RN_FT_GRAD)
        _, probs, ids = tr.eval_host(x7)
    finally:
        tr.close()
    err, yard = _grad_errors(got, G), _grad_errors(G32, G)
    dl = abs(float(losses[0]) - L)
    print("600: |dloss| %.3g (float32 torch %.3g); worst grad %.3g (float32 torch %.3g)" % (dl, abs(L32 - L), max(err.values()), max(yard.values())))
    record("finetune", "one_step_600", {"loss_abs": dl, "loss_abs_float32_torch": abs(L32 - L), "grad_rel": err,
                                        "grad_rel_worst_float32_torch": max(yard.values())})
    assert dl <= LOSS_TOL
    for n in G:
        assert err[n] <= GRAD_TOL, (n, err[n])
        assert not got[n][G[n] == 0].any(), n
    assert probs.shape == (2, 6) and ids.shape == (2,)


# ---- 7. end to end through RoomNet
def test_fine_tune_end_to_end(weights, images, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, learn_rate=2e-4, l2_regularizer_coeff=0.06,
                  start_step=7, dtype="f32", max_batch=32)
    net.init()
    net.set_variables({k: v for k, v in weights.items() if k in net.graph.variable_shapes()})
    try:
        f = net.extract_features(images)
        one = net.extract_features(images[3])
        assert one.tobytes() == f[3:4].tobytes()
        before = {k: v.copy() for k, v in net.sess.variables.items()}
        out = net.fine_tune(f, LABELS, steps=5, batch_size=8, seed=2, val=(f, LABELS))
        assert out["losses"].shape == (5,) and out["losses"].dtype == np.float32
        assert net.step == 12 and out["step"] == 12
        assert out["learn_rate"] == pytest.approx(2e-4 * 0.068 ** (12 / 10000))
        trained = set(finetune.trained_variables(net.graph))
        for k, v in net.sess.variables.items():
            assert (k in trained) != np.array_equal(v, before[k]), k
        tr = _capi.Trainer(net.graph, net.sess.variables, max_batch=32, l2_coeff=0.06)
        try:
            loss, probs_t, ids_t = tr.eval_host(f, LABELS)
        finally:
            tr.close()
        assert out["val"][0] == pytest.approx(loss, abs=1e-6) and out["val"][1] == pytest.approx(float(np.mean(ids_t == LABELS)))
        ids, probs = net.infer(images)
        assert np.abs(probs - probs_t).max() <= 1e-5
        net.save()
        fresh = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, dtype="f32", max_batch=32)
        fresh.load(str(tmp_path / "roomnet"))
        try:
            ids2, probs2 = fresh.infer(images)
            assert probs2.tobytes() == probs.tobytes() and np.array_equal(ids, ids2)
        finally:
            fresh.sess.close()
        for dtype in ("bf16", "f16"):
            eng = _capi.Engine(net.graph, net.sess.variables, device=0, dtype=dtype, max_batch=32)
            try:
                ids16, probs16 = eng.forward_u8(images)
                assert np.abs(probs16 - probs).max() <= 0.05
            finally:
                eng.close()
    finally:
        net.sess.close()


# ---- 8. errors
def test_errors_leave_trainer_and_handle_usable(weights, feats, images):
    tr = _trainer(weights, max_batch=8)
    d_f, d_l = tr.upload(feats), tr.upload(LABELS)
    bad_l = LABELS.copy()
    bad_l[5] = 6
    d_bad_l = tr.upload(bad_l)
    good = np.arange(8, dtype=np.int32).reshape(1, 8)
    try:
        p0 = tr.read()
        for index, labels, batch, what in ((np.array([[0, 1, 32, 3]], np.int32), d_l, 4, b"index"),
                                           (np.array([[0, -1, 2, 3]], np.int32), d_l, 4, b"index"),
                                           (np.array([[4, 5, 6, 7]], np.int32), d_bad_l, 4, b"label"),
                                           (good, d_l, 0, b"batch"), (np.tile(good, (1, 2)), d_l, 9, b"batch")):
            d_i = tr.upload(index)
            losses = np.zeros(1, np.float32)
            rc = tr.lib.rn_ft_run(tr.handle, d_f, labels, 32, d_i, batch, 1, losses.ctypes.data)
            assert rc == RN_E_RANGE and what in tr.lib.rn_last_error(), (what, rc, tr.lib.rn_last_error())
            tr.free(d_i)
        assert tr.step_count() == 0
        for n, v in tr.read().items():
            assert v.tobytes() == p0[n].tobytes()
        # items 0-3 carry good labels even in the bad label array: only indexed items are checked
        d_i = tr.upload(np.array([[0, 1, 2, 3]], np.int32))
        assert np.isfinite(tr.run(d_f, d_bad_l, 32, d_i, 4, 1)).all() and tr.step_count() == 1
        with pytest.raises(ValueError):
            tr.eval(d_f, 32, d_bad_l)
        _, probs, _ = tr.eval(d_f, 32)
        assert np.allclose(probs.sum(1), 1, atol=1e-5)
    finally:
        tr.close()
    g = build_graph(6, 224)
    g.dense[1].bn_name = ""                    # a dense block without its BN: the graphs grad-CAM refuses, for the same reason
    with pytest.raises(ValueError, match="not supported on this graph"):
        _capi.Trainer(g, weights)
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dropout_enabled=True, dtype="f32", max_batch=8)
    net.init()
    with pytest.raises(ValueError, match="dropout"):
        net.fine_tune(feats, LABELS, steps=1)
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
