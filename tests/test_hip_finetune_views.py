"""Fine-tuning on fresh random views (rn_ft_run_views, RoomNet.fine_tune_views): byte for byte the manual loop -- make the step's views,
run the trunk's feature pass, one rn_ft_run step -- at both depths on a 16-bit and a float32 handle, however the run is split over
calls, with dropout, with validation inside the run; the refusals; the Python surface."""
import numpy as np
import pytest

import finetune_harness as harness
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet

pytestmark = pytest.mark.gpu

S, BATCH, STEPS, SEED = 224, 5, 4, (1 << 33) + 11
LABELS = np.array([0, 1, 2, 3, 4, 5, 2], np.int32)
CFG = dict(learn_rate=2e-4, l2_coeff=0.06)


@pytest.fixture(scope="module")
def photographs(parity_images):
    """Seven photographs of mixed sizes cut from the parity images: copy mode, box mode, both axes, range 1, an upscale, a larger one."""
    p = parity_images
    wide = np.concatenate([p[1], p[14][:, :76]], axis=1)                      # 224 x 300
    tall = np.concatenate([p[30], p[52][:76]], axis=0)                        # 300 x 224
    box = np.kron(p[56], np.ones((2, 2, 1), np.uint8))                        # 448 x 448
    big = np.concatenate([np.kron(p[60], np.ones((2, 2, 1), np.uint8)), np.kron(p[3], np.ones((2, 2, 1), np.uint8))[:, :192]], axis=1)  # 448 x 640
    return [np.ascontiguousarray(a) for a in (p[0], box, tall, wide, tall[:225], p[41][40:137, 20:151], big)]


@pytest.fixture(scope="module")
def index():
    idx = finetune.epoch_indices(len(LABELS), BATCH, STEPS, seed=5)
    assert idx.shape == (STEPS, BATCH) and len(set(idx[0]) | set(idx[1])) > BATCH      # a new epoch, a new shuffle
    return idx


@pytest.fixture(scope="module")
def engines(weights):
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _capi.Engine(build_graph(6, S), weights, device=0, dtype=dtype, max_batch=8)
        return made[dtype]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def val_set(weights, parity_images):
    """Cached centre-crop features of twelve parity images, per depth, and their labels."""
    eng = harness.engine(weights, "f32", max_batch=12)
    try:
        ims = np.ascontiguousarray(parity_images[40:52])
        return {2: eng.features_u8(ims), 3: eng.features_u8(ims, depth=3)}, (np.arange(12, dtype=np.int32) % 6)
    finally:
        eng.close()


def new_trainer(weights, depth, max_batch=8, **kw):
    return harness.trainer(weights, max_batch=max_batch, depth=depth, **dict(CFG, **kw))


def run_views(tr, eng, views, index, calls, **kw):
    """``index`` through ``Trainer.run_views`` in calls of ``calls`` steps each; the losses."""
    d_l, d_i = tr.upload(LABELS), tr.upload(index)
    losses, at = [], 0
    for k in calls:
        losses.append(tr.run_views(eng, views, d_l, d_i + at * index.shape[1] * 4, index.shape[1], k, seed=SEED, **kw))
        at += k
    assert at == index.shape[0]
    return np.concatenate(losses)


class Manual:
    """The manual loop on one engine: the step's views (rn_views_batch_device), rn_features_depth_u8_device into a buffer of the
    caller's, then one step of rn_ft_run (or rn_ft_run_validated) on that buffer in slot order."""

    def __init__(self, tr, eng, views, depth):
        self.tr, self.eng, self.views, self.depth = tr, eng, views, depth
        self.d_bgr = eng.device_malloc(8 * S * S * 3)
        self.d_feat = eng.device_malloc(8 * int(np.prod(finetune.feature_shape(eng.graph, depth))) * 4)
        self.d_iota = tr.upload(np.arange(8, dtype=np.int32))

    def close(self):
        self.eng.device_free(self.d_bgr)
        self.eng.device_free(self.d_feat)

    def step(self, slots, validation=None, **kw):
        eng, tr, n = self.eng, self.tr, len(slots)
        views = eng.views_batch(self.views, slots, tr.step_count(), seed=SEED, **kw)
        eng.h2d(self.d_bgr, views)
        eng.features_u8_device(self.d_bgr, n, self.d_feat, depth=self.depth)
        eng.sync()
        d_l = tr.upload(LABELS[slots])
        try:
            if validation is None:
                return tr.run(self.d_feat, d_l, n, self.d_iota, n, 1)
            return tr.run_validated(self.d_feat, d_l, n, self.d_iota, n, 1, *validation)
        finally:
            tr.free(d_l)


def manual_losses(weights, eng, views, index, depth, **trainer_kw):
    tr = new_trainer(weights, depth, **trainer_kw)
    loop = Manual(tr, eng, views, depth)
    try:
        losses = np.concatenate([loop.step(slots) for slots in index])
        return losses, harness.state(tr) + [tr.read(_capi.RN_FT_GRAD)]
    finally:
        loop.close()
        tr.close()


def views_losses(weights, eng, views, index, depth, calls=(STEPS,), **trainer_kw):
    tr = new_trainer(weights, depth, **trainer_kw)
    try:
        losses = run_views(tr, eng, views, index, calls)
        assert tr.step_count() == index.shape[0]
        return losses, harness.state(tr) + [tr.read(_capi.RN_FT_GRAD)]
    finally:
        tr.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("depth", [2, 3])
def test_run_views_is_the_manual_loop(weights, engines, photographs, index, depth, dtype):
    eng = engines(dtype)
    views = eng.views_create(photographs)
    try:
        want = manual_losses(weights, eng, views, index, depth)
        got = views_losses(weights, eng, views, index, depth)
        print("depth %d %s: losses %s" % (depth, dtype, got[0]))
        assert np.isfinite(got[0]).all() and got[0].tobytes() == want[0].tobytes()
        harness.same_bytes(got[1], want[1])
        # the views matter: the centre crops without flips train on other features
        tr = new_trainer(weights, depth)
        try:
            plain = run_views(tr, eng, views, index, (STEPS,), crop=False, flip=False)
        finally:
            tr.close()
        assert plain.tobytes() != got[0].tobytes()
    finally:
        views.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_splitting_and_repeating(weights, engines, photographs, index, depth):
    eng = engines("bf16")
    views = eng.views_create(photographs)
    try:
        whole = views_losses(weights, eng, views, index, depth)
        for calls in ((STEPS,), (2, 2), (1, 1, 1, 1)):
            other = views_losses(weights, eng, views, index, depth, calls=calls)
            assert other[0].tobytes() == whole[0].tobytes(), calls
            harness.same_bytes(other[1], whole[1])
    finally:
        views.close()


def test_dropout_keeps_manual_loop_parity(weights, engines, photographs, index):
    eng = engines("bf16")
    views = eng.views_create(photographs)
    try:
        kw = dict(dropout_rate=0.35, dropout_seed=SEED)
        want = manual_losses(weights, eng, views, index, 3, **kw)
        got = views_losses(weights, eng, views, index, 3, **kw)
        assert got[0].tobytes() == want[0].tobytes()
        harness.same_bytes(got[1], want[1])
        assert got[0].tobytes() != views_losses(weights, eng, views, index, 3)[0].tobytes()
        split = views_losses(weights, eng, views, index, 3, calls=(1, 3), **kw)
        assert split[0].tobytes() == got[0].tobytes()
    finally:
        views.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_validation_inside_the_run(weights, engines, photographs, index, val_set, depth):
    eng = engines("bf16")
    views = eng.views_create(photographs)
    vf, vl = val_set[0][depth], val_set[1]
    try:
        tr = new_trainer(weights, depth)
        try:
            d_l, d_i, val = tr.upload(LABELS), tr.upload(index), (tr.upload(vf), tr.upload(vl), len(vl), 2)
            losses, points, vlosses, conf = tr.run_views(eng, views, d_l, d_i, BATCH, STEPS, seed=SEED, d_val_feats=val[0],
                                                         d_val_labels=val[1], n_val=val[2], val_every=val[3])
            got = (losses, points, vlosses, conf, tr.best(), harness.state(tr), tr.read(_capi.RN_FT_BEST))
        finally:
            tr.close()
        assert list(got[1]) == [2, 4] and got[3].shape == (2, 6, 6) and (got[3].sum((1, 2)) == len(vl)).all()
        tr = new_trainer(weights, depth)
        loop = Manual(tr, eng, views, depth)
        try:
            val = (tr.upload(vf), tr.upload(vl), len(vl), 2)
            mlosses, mpoints, mvl, mconf = [], [], [], []
            for s, slots in enumerate(index):
                if (s + 1) % 2:
                    mlosses.append(loop.step(slots))
                else:
                    one = loop.step(slots, validation=val)
                    mlosses.append(one[0])
                    mpoints += list(one[1])
                    mvl.append(one[2])
                    mconf.append(one[3])
            want = (np.concatenate(mlosses), mpoints, np.concatenate(mvl), np.concatenate(mconf), tr.best(), harness.state(tr),
                    tr.read(_capi.RN_FT_BEST))
        finally:
            loop.close()
            tr.close()
        assert got[0].tobytes() == want[0].tobytes() and list(got[1]) == want[1]
        assert got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
        assert got[4] == want[4]
        harness.same_bytes(got[5], want[5])
        harness.same_bytes([got[6]], [want[6]])
    finally:
        views.close()


def test_refusals_leave_the_trainer_unchanged(weights, engines, photographs, index, val_set):
    """Every refusal one GPU can show (a handle on another device and a failed slot allocation need what this machine has not)."""
    eng = engines("bf16")
    views = eng.views_create(photographs)
    tr = new_trainer(weights, 2, max_batch=16)
    small = new_trainer(weights, 2, max_batch=4)
    others = []
    try:
        lib = tr.lib
        d_l, d_i = tr.upload(LABELS), tr.upload(index)
        bad_l = LABELS.copy()
        bad_l[index[0, 1]] = 6
        bad_i = index.copy()
        bad_i[1, 2] = len(LABELS)
        neg_i = index.copy()
        neg_i[0, 0] = -1
        d_bad_l, d_bad_i, d_neg_i = tr.upload(bad_l), tr.upload(bad_i), tr.upload(neg_i)
        d_vf, d_vl = tr.upload(val_set[0][2]), tr.upload(val_set[1])
        losses, vlo, vco = np.zeros(STEPS, np.float32), np.zeros(STEPS, np.float32), np.zeros((STEPS, 6, 6), np.int32)
        before = harness.state(tr)
        no_val = (None, None, 0, 0, None, None)

        def call(ft=tr, h=eng, v=views, labels=d_l, n_items=len(LABELS), idx=d_i, batch=BATCH, steps=STEPS, flags=3, out=losses,
                 val=no_val):
            return lib.rn_ft_run_views(ft.handle if ft else None, h.handle if h else None, v.handle if v else None, labels, n_items, idx,
                                       batch, steps, SEED, flags, out.ctypes.data if out is not None else None, *val)

        # null arguments, unknown flags, half a validation: RN_E_INVALID
        for kw in (dict(ft=None), dict(h=None), dict(v=None), dict(labels=None), dict(idx=None), dict(out=None), dict(flags=4),
                   dict(n_items=len(LABELS) - 1),
                   dict(val=(d_vf, d_vl, 12, 2, None, vco.ctypes.data)), dict(val=(None, d_vl, 12, 2, vlo.ctypes.data, vco.ctypes.data))):
            assert call(**kw) == harness.RN_E_INVALID, kw
        # what rn_ft_run refuses: RN_E_RANGE
        for kw, what in ((dict(batch=0), b"batch"), (dict(ft=small), b"batch"), (dict(steps=0), b"steps"), (dict(idx=d_bad_i), b"index"),
                         (dict(idx=d_neg_i), b"index"), (dict(labels=d_bad_l), b"label"),
                         (dict(val=(d_vf, d_vl, 12, 0, vlo.ctypes.data, vco.ctypes.data)), b"val_every"),
                         (dict(val=(d_vf, d_vl, 0, 2, vlo.ctypes.data, vco.ctypes.data)), b"n_val")):
            assert call(**kw) == harness.RN_E_RANGE and what in lib.rn_last_error(), (kw, lib.rn_last_error())
        # a minibatch the trainer takes and the handle does not: RN_E_RANGE
        wide = np.tile(index, (1, 2))[:, :9].copy()
        d_wide = tr.upload(wide)
        assert call(idx=d_wide, batch=9) == harness.RN_E_RANGE and b"max_batch" in lib.rn_last_error()
        # a handle that normalises with batch moments: RN_E_STATE
        bs = _capi.Engine(build_graph(6, S), weights, device=0, dtype="f32", max_batch=8, batch_stats=True)
        others.append(bs)
        assert call(h=bs) == -4 and b"RN_FLAG_BATCH_STATS" in lib.rn_last_error()
        # a graph whose feature shape differs from the trainer's: RN_E_INVALID
        g300 = build_graph(6, 300)
        w300 = dict(weights)
        kernel = g300.dense[0].name + "/kernel"
        w300[kernel] = np.zeros(g300.variable_shapes()[kernel], np.float32)
        e300 = _capi.Engine(g300, w300, device=0, dtype="bf16", max_batch=8)
        others.append(e300)
        assert call(h=e300) == harness.RN_E_INVALID and b"feature" in lib.rn_last_error()
        # ... and views made for another side than the handle's
        v300 = e300.views_create(photographs[:2])
        try:
            assert call(v=v300, n_items=2) == harness.RN_E_INVALID and b"side" in lib.rn_last_error()
        finally:
            v300.close()
        assert tr.step_count() == 0 and small.step_count() == 0
        harness.same_bytes(harness.state(tr), before)
        # and the trainer goes on working
        assert call() == 0 and np.isfinite(losses).all() and tr.step_count() == STEPS
    finally:
        for t in (tr, small):
            t.close()
        views.close()
        for e in others:
            e.close()


# ---------------------------------------------------------------------------------------------- through RoomNet
def new_net(weights, start_step=7):
    net = RoomNet(6, im_side=S, compute_bn_mean_var=False, optimized_inference=True, learn_rate=2e-4, l2_regularizer_coeff=0.06,
                  start_step=start_step, dtype="bf16", max_batch=8)
    net.init()
    net.set_variables({k: v for k, v in weights.items() if k in net.graph.variable_shapes()})
    return net


@pytest.mark.parametrize("depth", [2, 3])
def test_fine_tune_views(weights, engines, photographs, val_set, depth):
    net = new_net(weights)
    try:
        np.testing.assert_array_equal(net.training_views(photographs, 9, seed=3, index=[6, 2, 2]),
                                      np.stack([finetune.make_view(photographs[i], finetune.view_draw(3, 9, b, *photographs[i].shape[:2]), S)
                                                for b, i in enumerate([6, 2, 2])], 0))
        assert net.training_views(photographs, 0).shape == (7, S, S, 3)
        before = {k: v.copy() for k, v in net.sess.variables.items()}
        val = (val_set[0][depth], val_set[1])
        out = net.fine_tune_views(photographs, LABELS, STEPS, batch_size=BATCH, seed=3, depth=depth, val=val, val_every=2)
        plain = {"losses", "step", "learn_rate", "val"}
        assert set(out) == plain | {"val_history", "best_step"}
        assert out["losses"].shape == (STEPS,) and out["losses"].dtype == np.float32 and np.isfinite(out["losses"]).all()
        assert net.step == 7 + STEPS == out["step"] and [e["step"] for e in out["val_history"]] == [8, 10, 11]
        assert out["learn_rate"] == pytest.approx(2e-4 * 0.068 ** (11 / 10000))
        trained = set(finetune.trained_variables(net.graph, depth=depth))
        for k, v in net.sess.variables.items():
            assert (k in trained) != np.array_equal(v, before[k]), k
        # the trainer-level run with the same arguments
        idx = finetune.epoch_indices(len(LABELS), BATCH, STEPS, seed=[3, 7])
        eng = engines("bf16")
        views = eng.views_create(photographs)
        tr = harness.trainer(weights, max_batch=8, depth=depth, learn_rate=2e-4, l2_coeff=0.06, num_steps=net.num_steps, start_step=7)
        try:
            losses = tr.run_views(eng, views, tr.upload(LABELS), tr.upload(idx), BATCH, STEPS, seed=3)
            want = tr.read()
        finally:
            tr.close()
            views.close()
        assert losses.tobytes() == out["losses"].tobytes()
        for k in trained:
            assert net.sess.variables[k].tobytes() == want[k].tobytes(), k
        # without validation: the keys of fine_tune without it
        out2 = net.fine_tune_views(photographs, LABELS, 1, batch_size=BATCH, seed=3, depth=depth, random_crop=False, flip=False)
        assert set(out2) == plain and out2["val"] is None and net.step == 8 + STEPS
        with pytest.raises(ValueError, match="max_batch"):
            net.fine_tune_views(photographs * 2, np.tile(LABELS, 2), 1, batch_size=9)
        with pytest.raises(ValueError, match="images"):
            net.fine_tune_views(photographs, LABELS[:3], 1)
        with pytest.raises(NotImplementedError):
            net.train_step(None, None)
    finally:
        net.sess.close()


def test_fine_tune_from_list_with_views(weights, photographs, tmp_path, capsys):
    from roomnet_amd.imageio import imread, imwrite
    from roomnet_amd.infer import fine_tune_from_list
    paths = []
    for k, im in enumerate(photographs):
        paths.append(str(tmp_path / ("photo %d.jpg" % k)))
        assert imwrite(paths[-1], im)
    junk = str(tmp_path / "junk.jpg")
    with open(junk, "wb") as f:
        f.write(b"\xff\xd8 not an image")
    listing = str(tmp_path / "train_list.txt")
    with open(listing, "w") as f:
        f.write("".join("%s %d\n" % (p, y) for p, y in zip(paths[:3] + [junk] + paths[3:], list(LABELS[:3]) + [0] + list(LABELS[3:]))))
    a, b = new_net(weights), new_net(weights)
    try:
        got = fine_tune_from_list(a, listing, STEPS, batch_size=BATCH, seed=4, depth=2, views=True)
        assert "junk.jpg" in capsys.readouterr().out
        want = b.fine_tune_views([imread(p) for p in paths], LABELS, STEPS, batch_size=BATCH, seed=4, depth=2)
        assert got["losses"].tobytes() == want["losses"].tobytes() and got["step"] == want["step"] == 7 + STEPS
        for k in finetune.trained_variables(a.graph, depth=2):
            assert a.sess.variables[k].tobytes() == b.sess.variables[k].tobytes(), k
        flat = fine_tune_from_list(a, listing, 1, batch_size=BATCH, seed=4, depth=2, views=True, random_crop=False, flip=False)
        assert np.isfinite(flat["losses"]).all()
        with pytest.raises(ValueError, match="gpu_decode"):
            fine_tune_from_list(a, listing, 1, views=True, gpu_decode=True)
    finally:
        a.sess.close()
        b.sess.close()
