"""What the GPU tests of the fine-tuning trainers share (test_hip_finetune.py, test_hip_finetune7.py, test_hip_finetune_dropout.py,
test_hip_backward_live.py): the items, the bounds, the fixtures, and the one-step, trajectory, determinism, end-to-end and error
checks, each stated once against the one reference, tests/finetune_ref.py.  Not a conftest: a test module imports the fixtures it
uses by name.  Every check prints and records (``record(section, key, ...)`` -> the parity report) the kernel's error beside the
float32 torch yardstick's before it asserts."""
import numpy as np
import pytest

from finetune_ref import dropped_x6, host_masks, make_ref
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet, _initializer_values

ITEMS = list(range(0, 8)) + list(range(40, 64))          # 32 parity images, all six classes
LABELS = np.arange(32, dtype=np.int32) % 6
W7 = "conv2d_7/kernel"
RN_E_INVALID, RN_E_RANGE = -1, -5

# The bounds, set with each feature from the float32 torch run of the same mathematics (the yardstick) and unchanged since.
#
# Depth 2 (measured on the 32 items, both starts): gradients per variable max|d| / max|g_ref| <= GRAD_TOL (float32 yardstick: 7.0e-7)
# and |d loss| <= LOSS_TOL (2.6e-7); trajectory: every parameter within 0.01 learn_rate = 2e-6 of float64 after 20 steps (yardstick
# drift 2.0e-7) and every loss within LOSS_TOL (8.9e-7).
#
# Depth 3: the same, and for conv2d_7/kernel the elementwise |d| <= GRAD_TOL max|g_ref| + Amb / n with delta = DELTA, on condition
# that the share of pre-activations within delta of a ReLU6 kink is <= SHARE_CAP (finetune_ref.conv7_ambiguity: a float32 sum in
# another order may mask such a position the other way, and Amb is the room that takes).  Float32-torch yardstick at the float64
# oracle's s6.bn, batch 32: 2.2e-6 for dW7, 7.3e-7 for d gamma7, 2.5e-7 for d beta7, 2.7e-7 for the loss; share 2.4e-5.  Measured on
# an MI355X at the handle's features (profiles/finetune7_parity.json): dW7 within 2.0e-6 of its largest entry without the room
# (float32 torch there: 6.6e-6), share 2.3e-5, the loss within 8.9e-7, the other gradients within 4.5e-6; with conv 7 as one float32
# chain over K = 1152 dW7 missed by 1.08e-5 and 1.13e-5 at batch 32 and 45 from the shipped checkpoint -- masks flipped outside
# delta -- which is why the kernel adds chains of 16 channels in float64.
#
# Dropout: the same bounds against the same masked mathematics; conv7_ambiguity is evaluated on the DROPPED s6.bn.  Trajectories at
# depth 3 and with dropout: every parameter within max(0.01 learn_rate, 3 x the float32 torch run's drift) of float64.
GRAD_TOL, LOSS_TOL = 1e-5, 5e-6
DELTA, SHARE_CAP = 1e-6, 1e-4


def engine(weights, dtype, max_batch=32, **kw):
    return _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=max_batch, **kw)


def trainer(w, side=224, max_batch=45, depth=2, nc=6, **kw):
    return _capi.Trainer(build_graph(nc, side), w, device=0, max_batch=max_batch, depth=depth, **kw)


@pytest.fixture(scope="module")
def images(parity_images):
    return np.ascontiguousarray(parity_images[ITEMS])


@pytest.fixture(scope="module")
def feats(weights, images):
    """The handle's own f32 features: ``{2: s7.bn [32, 21, 21, 16], 3: s6.bn [32, 46, 46, 128]}``."""
    eng = engine(weights, "f32")
    try:
        return {2: eng.features_u8(images), 3: eng.features_u8(images, depth=3)}
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


def grad_errors(got, ref):
    """Per variable max |got - ref| / max |ref|."""
    return {n: float(np.abs(np.asarray(got[n], np.float64) - ref[n]).max() / max(np.abs(ref[n]).max(), 1e-300)) for n in ref}


def locate(got, want):
    """Where a tensor is wrong, in the style of test_hip_other_checkpoints._locate: the worst element and its values."""
    d = np.abs(np.asarray(got, np.float64) - want)
    i = np.unravel_index(int(d.argmax()), d.shape)
    return {"at": [int(v) for v in i], "got": float(np.asarray(got)[i]), "want": float(want[i]), "abs_err": float(d[i]),
            "max_abs_want": float(np.abs(want).max()), "elements_above_half_of_worst": int((d > 0.5 * d.max()).sum())}


def state(tr):
    return [tr.read(), tr.read(_capi.RN_FT_ADAM_M), tr.read(_capi.RN_FT_ADAM_V)]


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for n in x:
            assert x[n].tobytes() == y[n].tobytes(), n


# ---------------------------------------------------------------------------------------------- one step
def one_step_reference(w, x, y, idx, l2, depth, side=224, nc=6, rate=0.0, seed=0):
    """One step on slots ``idx`` of ``x`` in float64 and in the yardstick, with the host masks of step 0 when ``rate``: the
    reference ``ref`` (``ref.twin32``), its input ``xin`` (at depth 3 with dropout the dropped s6.bn), ``masks``, losses ``L`` and
    ``L32``, gradients ``G`` and ``G32`` and the yardstick's errors ``yard``."""
    masks = host_masks(build_graph(nc, side), depth, seed, 0, len(idx), rate) if rate else None
    xin = dropped_x6(x[idx], masks[0], rate) if rate and depth == 3 else x[idx]
    ref = make_ref(w, nc, side, depth, masks, rate)
    L, G = ref.loss_and_grads(xin, y[idx], l2)
    L32, G32 = ref.twin32.loss_and_grads(xin, y[idx], l2)
    return {"ref": ref, "xin": xin, "masks": masks, "L": L, "G": G, "L32": L32, "G32": G32, "yard": grad_errors(G32, G)}


def check_one_step(w, x, y, idx, l2, record, section, key, depth, side=224, nc=6, rate=0.0, seed=0, reference=None,
                   loss_bound=LOSS_TOL, delta=DELTA, condition=None, extra=None):
    """One step of a trainer on slots ``idx`` of ``x`` against float64 (``reference``: a ``one_step_reference`` computed before):
    the loss within ``loss_bound``, every variable but conv2d_7/kernel within GRAD_TOL, that one elementwise within GRAD_TOL max|g| +
    Amb / n at ``delta`` with a near-kink share <= SHARE_CAP, exact zeros wherever float64 is exactly zero.  ``condition()`` holds
    the caller's conditions on the inputs: it runs once the figures (with ``extra``) are on record and before the kernel is judged.
    Returns ``(reference, gradients, losses)``."""
    n = len(idx)
    r = reference or one_step_reference(w, x, y, idx, l2, depth, side, nc, rate, seed)
    L, G, yard = r["L"], r["G"], r["yard"]
    if depth == 3 and "amb" not in r:
        r["share"], r["amb"] = r["ref"].conv7_ambiguity(r["xin"], y[idx], l2, delta)
    tr = trainer(w, side, max(n, 2), depth, nc, learn_rate=2e-4, l2_coeff=l2, dropout_rate=rate, dropout_seed=seed if rate else 0)
    try:
        names = [v for v, _ in tr.variables()]
        assert names == finetune.trained_variables(tr.graph, depth=depth) and len(names) == len(G) == {2: 19, 3: 22}[depth]
        assert tr.lib.rn_ft_depth(tr.handle) == depth
        if rate:
            assert tr.dropout() == (float(np.float32(rate)), seed)
        losses = tr.run_host(x, y, np.asarray(idx, np.int32).reshape(1, n))
        got = tr.read(_capi.RN_FT_GRAD)
    finally:
        tr.close()
    err = grad_errors(got, G)
    dl, dl32 = abs(float(losses[0]) - L), abs(r["L32"] - L)
    rec = {"loss": L, "loss_abs": dl, "loss_abs_float32_torch": dl32, "loss_bound": loss_bound, "grad_rel_worst": max(err.values()),
           "grad_rel_worst_float32_torch": max(yard.values()), "grad_bound": GRAD_TOL, "grad_rel": err, "grad_rel_float32_torch": yard}
    text = "%s: loss %.9g (ref %.9g) |dloss| %.3g (float32 torch %.3g, bound %.3g); worst grad %.3g (float32 torch %.3g)" \
        % (key, losses[0], L, dl, dl32, loss_bound, max(err.values()), max(yard.values()))
    if depth == 3:
        gmax = float(np.abs(G[W7]).max())
        d7 = np.abs(got[W7].astype(np.float64) - G[W7])
        room = GRAD_TOL * gmax + r["amb"] / n
        over = float((d7 / room).max()) if gmax else 0.0
        rec.update({"near_kink_share": r["share"], "share_cap": SHARE_CAP, "dw7_over_room_worst": over,
                    "amb_over_n_max_rel": float(r["amb"].max() / n / max(gmax, 1e-300))})
        text += "; dW7 %.3g (float32 torch %.3g), share %.3g at delta %.3g, max Amb/n %.3g of max|g|, worst dW7 / room %.3g" \
            % (err[W7], yard[W7], r["share"], delta, rec["amb_over_n_max_rel"], over)
    rec.update(extra or {})
    print(text)
    record(section, key, rec)
    if condition:
        condition()
    assert dl <= loss_bound, (dl, loss_bound)
    if depth == 3:
        assert r["share"] <= SHARE_CAP
        assert np.all(d7 <= room), ("conv2d_7/kernel: %d elements outside 1e-5 max|g| + Amb / n" % int((d7 > room).sum()),
                                    locate(got[W7], G[W7]))
    for name in G:
        if name != W7:
            assert err[name] <= GRAD_TOL, (name, err[name], locate(got[name], G[name]))
        zero = G[name] == 0
        assert not got[name][zero].any(), "%s: %d entries are exactly zero in float64 and not on the GPU" \
            % (name, int(got[name][zero].astype(bool).sum()))
    return r, got, losses


# ---------------------------------------------------------------------------------------------- several steps
def check_trajectory(w, x, index, record, section, key, depth, drift32_factor=0, rate=0.0, seed=0):
    """The Adam steps of ``index`` on the 32 items against float64: every loss within LOSS_TOL, every parameter within
    max(0.01 learn_rate, ``drift32_factor`` x the float32 torch run's drift) -- the factor allows for another summation order --
    and, after the first step, Adam's slots against the gradient read back."""
    lr, l2, ns = 2e-4, 0.06, 10000
    steps, batch = index.shape
    ref = make_ref(w, 6, 224, depth)
    Lref = ref.train(x, LABELS, index, lr, ns, l2, seed=seed, rate=rate)
    L32 = ref.twin32.train(x, LABELS, index, lr, ns, l2, seed=seed, rate=rate)
    P, P32 = ref.values(), ref.twin32.values()
    tr = trainer(w, depth=depth, learn_rate=lr, l2_coeff=l2, num_steps=ns, dropout_rate=rate, dropout_seed=seed)
    d = [tr.upload(x), tr.upload(LABELS), tr.upload(index)]
    try:
        first = tr.run(d[0], d[1], 32, d[2], batch, 1)
        g1, m1, v1 = tr.read(_capi.RN_FT_GRAD), tr.read(_capi.RN_FT_ADAM_M), tr.read(_capi.RN_FT_ADAM_V)
        rest = tr.run(d[0], d[1], 32, d[2] + batch * 4, batch, steps - 1)
        got = tr.read()
        assert tr.step_count() == steps
    finally:
        tr.close()
    omb1 = 1.0 - float(np.float32(0.9))
    omb2 = 1.0 - float(np.float32(0.999))
    assert len(g1) == {2: 19, 3: 22}[depth]
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
    bound = max(0.01 * lr, drift32_factor * drift32)
    print("%s: parameter drift %.3g (float32 torch %.3g, bound %.3g), parameters moved %.3g = %.1f lr; loss drift %.3g "
          "(float32 torch %.3g)" % (key, drift, drift32, bound, moved, moved / lr, dl, dl32))
    record(section, key, {"param_abs": drift, "param_abs_float32_torch": drift32, "param_moved": moved,
                          "loss_abs": dl, "loss_abs_float32_torch": dl32, "bound_param": bound})
    assert drift <= bound
    assert dl <= LOSS_TOL


def check_determinism(w, x, index, depth, **kw):
    """The same calls give the same bytes -- losses, parameters and both Adam slots -- and so does one rn_ft_run per step."""
    steps, batch = index.shape

    def run(split):
        tr = trainer(w, depth=depth, learn_rate=2e-4, l2_coeff=0.06, **kw)
        d = [tr.upload(x), tr.upload(LABELS), tr.upload(index)]
        try:
            if split:
                losses = np.concatenate([tr.run(d[0], d[1], 32, d[2] + batch * 4 * s, batch, 1) for s in range(steps)])
            else:
                losses = tr.run(d[0], d[1], 32, d[2], batch, steps)
            return losses, state(tr)
        finally:
            tr.close()

    a, b, c = run(False), run(False), run(True)
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes()
        assert len(a[1][0]) == {2: 19, 3: 22}[depth]
        same_bytes(a[1], other[1])


# ---------------------------------------------------------------------------------------------- through RoomNet
def check_end_to_end(weights, images, tmp_path, monkeypatch, depth):
    monkeypatch.chdir(tmp_path)
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, learn_rate=2e-4, l2_regularizer_coeff=0.06,
                  start_step=7, dtype="f32", max_batch=32)
    net.init()
    net.set_variables({k: v for k, v in weights.items() if k in net.graph.variable_shapes()})
    try:
        f = net.extract_features(images, depth=depth)
        assert f.shape == (32,) + finetune.feature_shape(net.graph, depth)
        one = net.extract_features(images[3], depth=depth)
        assert one.tobytes() == f[3:4].tobytes()
        if depth == 3:
            with pytest.raises(ValueError, match="depth 3"):
                net.fine_tune(net.extract_features(images[:2]), LABELS[:2], steps=1, depth=3)
        before = {k: v.copy() for k, v in net.sess.variables.items()}
        out = net.fine_tune(f, LABELS, steps=5, batch_size=8, seed=2, val=(f, LABELS))
        assert out["losses"].shape == (5,) and out["losses"].dtype == np.float32
        assert net.step == 12 and out["step"] == 12
        assert out["learn_rate"] == pytest.approx(2e-4 * 0.068 ** (12 / 10000))
        trained = set(finetune.trained_variables(net.graph, depth=depth))
        assert len(trained) == {2: 19, 3: 22}[depth]
        for k, v in net.sess.variables.items():
            assert (k in trained) != np.array_equal(v, before[k]), k
        tr = _capi.Trainer(net.graph, net.sess.variables, max_batch=32, l2_coeff=0.06, depth=depth)
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


# ---------------------------------------------------------------------------------------------- errors
def check_run_errors(weights, x, depth):
    """Refused rn_ft_run calls name what was wrong and leave the trainer as it was, and it goes on working."""
    tr = trainer(weights, max_batch=8, depth=depth)
    d_f, d_l = tr.upload(x), tr.upload(LABELS)
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
