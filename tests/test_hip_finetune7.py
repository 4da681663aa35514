"""Depth-3 fine-tuning on the GPU (rn_features_depth_*, rn_ft_create_depth): the s6.bn features against rn_tap, one step's loss and
gradients, a 20-step Adam trajectory and a 100-step learning run against the float64 reference (tests/finetune7_ref.py) evaluated
at the handle's own features, determinism, the 300 and 600 geometries without a trunk, depth 2 through the new entry points,
RoomNet.fine_tune end to end, and errors.

Bounds: the project's existing ones -- gradients per variable max|d| / max|g_ref| <= 1e-5, |d loss| <= 5e-6, trajectory losses
within 5e-6 -- and for conv2d_7/kernel the elementwise |d| <= 1e-5 max|g_ref| + Amb / n with delta = 1e-6, on condition that the
share of pre-activations within delta of a ReLU6 kink is <= 1e-4 (finetune7_ref.conv7_ambiguity: a float32 sum in another order may
mask such a position the other way, and Amb is the room that takes).  Float32-torch yardstick at the float64 oracle's s6.bn, batch
32: 2.2e-6 for dW7, 7.3e-7 for d gamma7, 2.5e-7 for d beta7, 2.7e-7 for the loss; share 2.4e-5.
Measured on an MI355X at the handle's features (profiles/finetune7_parity.json): dW7 within 2.0e-6 of its largest entry without the
room (float32 torch there: 6.6e-6), share 2.3e-5, the loss within 8.9e-7, the other gradients within 4.5e-6; with conv 7 as one float32 chain over K = 1152 dW7 missed by
1.08e-5 and 1.13e-5 at batch 32 and 45 from the shipped checkpoint -- masks flipped outside delta -- which is why the kernel adds chains
of 16 channels in float64.
Each test records the kernel's error beside the yardstick's through ``record("finetune7", ...)``."""
import numpy as np
import pytest
import torch

from finetune7_ref import FineTune7Ref
from finetune_ref import FineTuneRef
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet, _initializer_values

pytestmark = pytest.mark.gpu

ITEMS = list(range(0, 8)) + list(range(40, 64))          # the 32 parity items and labels of test_hip_finetune.py
LABELS = np.arange(32, dtype=np.int32) % 6
GRAD_TOL, LOSS_TOL = 1e-5, 5e-6
DELTA, SHARE_CAP = 1e-6, 1e-4
W7 = "conv2d_7/kernel"
RN_E_INVALID, RN_E_RANGE = -1, -5


def _engine(weights, dtype, max_batch=32, **kw):
    return _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=max_batch, **kw)


@pytest.fixture(scope="module")
def images(parity_images):
    return np.ascontiguousarray(parity_images[ITEMS])


@pytest.fixture(scope="module")
def feats(weights, images):
    eng = _engine(weights, "f32")
    try:
        return eng.features_u8(images, depth=3)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def starts(weights):
    """The shipped checkpoint, and the reference's load() state in training mode: the conv trunk restored, the dense head at its
    initial values."""
    g = build_graph(6, 224)
    fresh = dict(weights)
    init = _initializer_values(g, seed=1)
    for d in g.dense:
        for name in init:
            if name.startswith(d.name + "/") or (d.bn_name and name.startswith(d.bn_name + "/")):
                fresh[name] = init[name]
    return {"shipped": weights, "fresh": fresh}


def _trainer(w, side=224, max_batch=45, depth=3, **kw):
    return _capi.Trainer(build_graph(6, side), w, device=0, max_batch=max_batch, depth=depth, **kw)


def _grad_errors(got, ref):
    return {n: float(np.abs(got[n].astype(np.float64) - ref[n]).max() / max(np.abs(ref[n]).max(), 1e-300)) for n in ref}


def _check_one_step(w, side, x6, y, l2, idx, record, key):
    """One step of a depth-3 trainer on items ``idx`` of ``x6`` against float64: the bounds of the module docstring."""
    n = len(idx)
    ref = FineTune7Ref(w, 6, side)
    L, G = ref.loss_and_grads(x6[idx], y[idx], l2)
    L32, G32 = FineTune7Ref(w, 6, side, dtype=torch.float32).loss_and_grads(x6[idx], y[idx], l2)
    share, amb = ref.conv7_ambiguity(x6[idx], y[idx], l2, DELTA)
    tr = _trainer(w, side=side, max_batch=max(n, 2), learn_rate=2e-4, l2_coeff=l2)
    try:
        assert [v for v, _ in tr.variables()] == finetune.trained_variables(tr.graph, depth=3) and len(tr.variables()) == 22
        assert tr.lib.rn_ft_depth(tr.handle) == 3
        losses = tr.run_host(x6, y, np.asarray(idx, np.int32).reshape(1, n))
        got = tr.read(_capi.RN_FT_GRAD)
    finally:
        tr.close()
    err, yard = _grad_errors(got, G), _grad_errors(G32, G)
    dl, dl32 = abs(float(losses[0]) - L), abs(L32 - L)
    d7 = np.abs(got[W7].astype(np.float64) - G[W7])
    room = GRAD_TOL * np.abs(G[W7]).max() + amb / n
    print("%s: loss %.9g (ref %.9g) |dloss| %.3g (float32 torch %.3g); worst grad %.3g (float32 torch %.3g); dW7 %.3g (float32 torch "
          "%.3g), share %.3g, max Amb/n %.3g of max|g|, worst dW7 / room %.3g"
          % (key, losses[0], L, dl, dl32, max(err.values()), max(yard.values()), err[W7], yard[W7], share,
             amb.max() / n / np.abs(G[W7]).max(), float((d7 / room).max())))
    record("finetune7", key, {"loss_abs": dl, "loss_abs_float32_torch": dl32, "grad_rel_worst": max(err.values()),
                              "grad_rel_worst_float32_torch": max(yard.values()), "grad_rel": err, "grad_rel_float32_torch": yard,
                              "near_kink_share": share, "amb_over_n_max_rel": float(amb.max() / n / np.abs(G[W7]).max()),
                              "dw7_over_room_worst": float((d7 / room).max())})
    assert share <= SHARE_CAP
    assert dl <= LOSS_TOL
    assert np.all(d7 <= room), "conv2d_7/kernel: %d elements outside 1e-5 max|g| + Amb / n" % int((d7 > room).sum())
    for name in G:
        if name != W7:
            assert err[name] <= GRAD_TOL, (name, err[name])
        zero = G[name] == 0
        assert not got[name][zero].any(), name


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
    _check_one_step(starts[start], 224, feats, LABELS, l2, idx, record, "one_step_%s_l2_%g_batch_%d" % (start, l2, batch))


# ---- 3. trajectory
@pytest.mark.parametrize("start", ["shipped", "fresh"])
def test_trajectory_20_steps(starts, feats, record, start):
    """Every parameter within max(0.01 learn_rate, 3 x the float32-torch run's drift) of float64 after 20 steps; the factor 3 allows
    for another summation order.  Float32-torch drift measured on the CPU at the float64 oracle's s6.bn before the first GPU run:
    2.8e-7 from the shipped checkpoint, 2.3e-7 from the fresh head (conv2d_7/kernel: 2.2e-8 and 3.2e-8),
    so the first term, 0.01 learn_rate = 2e-6, is the bound; losses drift 9.7e-7 and 9.1e-7.  At the handle's
    features and on 16 threads the float32-torch run drifts 3.1e-6 from the shipped checkpoint (the bound there is 9.4e-6)
    and 2.3e-7 from the fresh head; the kernel 4.6e-7 and 2.0e-7."""
    w = starts[start]
    lr, l2, ns = 2e-4, 0.06, 10000
    index = finetune.epoch_indices(32, 8, 20, seed=5)
    ref = FineTune7Ref(w, 6, 224)
    Lref = ref.train(feats, LABELS, index, lr, ns, l2)
    ref32 = FineTune7Ref(w, 6, 224, dtype=torch.float32)
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
    assert len(g1) == 22
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
    bound = max(0.01 * lr, 3 * drift32)
    print("trajectory %s: parameter drift %.3g (float32 torch %.3g, bound %.3g), parameters moved %.3g = %.1f lr; loss drift %.3g "
          "(float32 torch %.3g)" % (start, drift, drift32, bound, moved, moved / lr, dl, dl32))
    record("finetune7", "trajectory_%s" % start, {"param_abs": drift, "param_abs_float32_torch": drift32, "param_moved": moved,
                                                  "loss_abs": dl, "loss_abs_float32_torch": dl32, "bound_param": bound})
    assert drift <= bound
    assert dl <= LOSS_TOL


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
        x7 = ref.x7(ref._t(feats)).numpy()                 # the depth-2 feature of the same items, conv 7 as loaded
    Lref = ref.train(feats, LABELS, index, lr, ns, l2)
    L2 = FineTuneRef(w, 6, 224).train(x7, LABELS, index, lr, ns, l2)
    L0, L1 = float(Lref[0]), float(Lref[-1])
    assert L1 < L0
    tr = _trainer(w, learn_rate=lr, l2_coeff=l2, num_steps=ns)
    try:
        losses = tr.run_host(feats, LABELS, index)
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
            assert len(a[k]) == 22
            for n in a[k]:
                assert a[k][n].tobytes() == other[k][n].tobytes(), n


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
    _check_one_step(w, side, x6, y, 0.06, np.arange(n), record, "one_step_%d" % side)
    tr = _trainer(w, side=side, max_batch=2, l2_coeff=0.06)
    try:
        loss, probs, ids = tr.eval_host(x6, y)
        ref = FineTune7Ref(w, 6, side)
        assert np.abs(probs - ref.probs(x6)).max() <= 1e-5 and probs.shape == (n, 6) and ids.shape == (n,)
        assert abs(loss - float(ref.loss(x6, y, 0.06))) <= LOSS_TOL
    finally:
        tr.close()


# ---- 7. depth 2 is untouched
def test_depth_2_through_the_new_entry_point(starts, weights, images):
    w = starts["fresh"]
    eng = _engine(weights, "f32")
    try:
        f2 = eng.features_u8(images)
    finally:
        eng.close()
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
    monkeypatch.chdir(tmp_path)
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, learn_rate=2e-4, l2_regularizer_coeff=0.06,
                  start_step=7, dtype="f32", max_batch=32)
    net.init()
    net.set_variables({k: v for k, v in weights.items() if k in net.graph.variable_shapes()})
    try:
        f = net.extract_features(images, depth=3)
        assert f.shape == (32, 46, 46, 128)
        one = net.extract_features(images[3], depth=3)
        assert one.tobytes() == f[3:4].tobytes()
        with pytest.raises(ValueError, match="depth 3"):
            net.fine_tune(net.extract_features(images[:2]), LABELS[:2], steps=1, depth=3)
        before = {k: v.copy() for k, v in net.sess.variables.items()}
        out = net.fine_tune(f, LABELS, steps=5, batch_size=8, seed=2, val=(f, LABELS))
        assert out["losses"].shape == (5,) and out["losses"].dtype == np.float32
        assert net.step == 12 and out["step"] == 12
        assert out["learn_rate"] == pytest.approx(2e-4 * 0.068 ** (12 / 10000))
        trained = set(finetune.trained_variables(net.graph, depth=3))
        assert len(trained) == 22
        for k, v in net.sess.variables.items():
            assert (k in trained) != np.array_equal(v, before[k]), k
        tr = _capi.Trainer(net.graph, net.sess.variables, max_batch=32, l2_coeff=0.06, depth=3)
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
            _trainer(weights, depth=depth)
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
        d_i = tr.upload(np.array([[0, 1, 2, 3]], np.int32))
        assert np.isfinite(tr.run(d_f, d_bad_l, 32, d_i, 4, 1)).all() and tr.step_count() == 1
        _, probs, _ = tr.eval(d_f, 32)
        assert np.allclose(probs.sum(1), 1, atol=1e-5)
    finally:
        tr.close()
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
