"""Host side of fine-tuning the last conv stages and the dense head (``RoomNet.fine_tune``, C ABI ``rn_ft_*``): which variables are
trained, the learning-rate schedule, the minibatch order, the validation points of a run and a NumPy statement of the Adam rule, and the dropout stream (``philox4x32``, ``dropout_keep``): the product's statement of the masks the kernels
recompute, as ``jpegenc.py`` is for the encoder.  Pure host code; the mathematics is stated once in the headers of
``csrc/rn_finetune.hip``, ``csrc/rn_finetune7.hip`` and ``csrc/rn_dropout.h``.

The *depth* of a trainer or a feature is its number of trained conv stages: 2 trains stages 8-9 on cached ``s7.bn`` (28 KB per
image at 224), 3 trains the whole last block, stages 7-9, on cached ``s6.bn`` (1.08 MB per image at 224)."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .graph import Graph

DECAY_RATE = 0.068                       # network.py:36
ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON = 0.9, 0.999, 1e-8      # tf.train.AdamOptimizer defaults


DEPTHS = (2, 3)


def _checked_depth(depth) -> int:
    if depth not in DEPTHS:
        raise ValueError("depth = %r is neither 2 (features s7.bn) nor 3 (features s6.bn)" % (depth,))
    return int(depth)


def trained_variables(graph: Graph, depth: int = 2) -> List[str]:
    """Checkpoint names of the variables ``rn_ft_*`` trains, in the trainer's order: the last ``depth`` conv stages' kernels and BN
    gamma / beta (both BNs of the residual stage), then per dense layer its kernel and its BN's gamma / beta or its bias: 19
    names at depth 2, 22 at depth 3 for the reference graph."""
    names = []
    for s in graph.stages[-_checked_depth(depth):]:
        names.append(s.conv_name + "/kernel")
        for bn in (s.bn_name, s.bn2_name):
            if bn:
                names += [bn + "/gamma", bn + "/beta"]
    for d in graph.dense:
        names.append(d.name + "/kernel")
        if d.biased:
            names.append(d.name + "/bias")
        if d.bn_name:
            names += [d.bn_name + "/gamma", d.bn_name + "/beta"]
    return names


def feature_shape(graph: Graph, depth: int = 2) -> Tuple[int, int, int]:
    """Per-image shape of the cached feature: the input of the first trained stage.  Depth 2: ``s7.bn``, the output of the last
    block's first step (21 x 21 x 16 at 224: 28 KB in float32); depth 3: ``s6.bn``, the input of the last block (46 x 46 x 128 at
    224: 1.08 MB)."""
    s = graph.stages[-_checked_depth(depth) - 1]
    return s.out_side, s.out_side, s.cout


def depth_of_features(graph: Graph, shape) -> int:
    """The depth whose feature has the per-image ``shape``; ``ValueError`` when neither has."""
    for depth in DEPTHS:
        if tuple(shape) == feature_shape(graph, depth):
            return depth
    raise ValueError("features of per-image shape %s match neither depth 2 %s nor depth 3 %s"
                     % (tuple(shape), feature_shape(graph, 2), feature_shape(graph, 3)))


def learn_rate_at(step, learn_rate, num_steps, decay_rate=DECAY_RATE):
    """``tf.train.exponential_decay(learn_rate, step, num_steps, decay_rate)`` without staircase (network.py:36)."""
    return float(learn_rate) * float(decay_rate) ** (float(step) / float(num_steps))


def epoch_indices(n_items, batch, steps, seed):
    """The reference feeder's minibatch order (generator.py:39, :126-133) as ``int32 [steps, batch]`` item indices: the items are
    shuffled, an epoch is its first ``n_items // batch`` batches in order (the remainder is dropped), and every new epoch
    shuffles again.  A batch larger than the set is cut to the set (generator.py:36-38)."""
    n_items, batch, steps = int(n_items), int(batch), int(steps)
    if n_items < 1 or batch < 1 or steps < 0:
        raise ValueError("epoch_indices: n_items %d, batch %d, steps %d" % (n_items, batch, steps))
    batch = min(batch, n_items)
    per_epoch = n_items // batch
    rng = np.random.default_rng(seed)
    order = np.arange(n_items, dtype=np.int32)
    out = np.empty((steps, batch), np.int32)
    for s in range(steps):
        k = s % per_epoch
        if k == 0:
            rng.shuffle(order)
        out[s] = order[k * batch:(k + 1) * batch]
    return out


def validation_steps(step, steps, val_every) -> List[int]:
    """The global steps at which a run of ``steps`` steps that starts at global step ``step`` validates (``rn_ft_val_points``):
    every ``g`` in ``(step, step + steps]`` with ``g % val_every == 0`` -- the reference's ``train_iter % SAVE_FREQ == 0 and
    train_iter > start_step`` (train.py:134) -- and ``step + steps`` itself if that is none of them."""
    step, steps, val_every = int(step), int(steps), int(val_every)
    if step < 0 or steps < 1 or val_every < 1:
        raise ValueError("validation_steps: step %d, steps %d, val_every %d" % (step, steps, val_every))
    points = [g for g in range(step + 1, step + steps + 1) if g % val_every == 0]
    if not points or points[-1] != step + steps:
        points.append(step + steps)
    return points


def adam_update(param, grad, m, v, t, lr, beta1=ADAM_BETA1, beta2=ADAM_BETA2, epsilon=ADAM_EPSILON):
    """One ``tf.train.AdamOptimizer`` step on arrays of any float dtype (the arithmetic runs in ``param``'s): ``t`` counts from
    1, ``lr`` is the decayed learning rate of this step.  ``m``, ``v`` are the raw moments; epsilon sits outside the root.
    Returns ``(param, m, v)``."""
    param = np.asarray(param)
    dt = param.dtype
    g = np.asarray(grad, dt)
    lr_t = dt.type(float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t))
    m = np.asarray(m, dt) + (g - np.asarray(m, dt)) * dt.type(1.0 - beta1)
    v = np.asarray(v, dt) + (g * g - np.asarray(v, dt)) * dt.type(1.0 - beta2)
    return param - lr_t * m / (np.sqrt(v) + dt.type(epsilon)), m, v


# ---- dropout (csrc/rn_dropout.h, include/roomnet_hip.h: dropout while fine-tuning)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 as published (Salmon et al., SC'11).  ``counter``: four 32-bit words, or an array ``[..., 4]`` of them;
    ``key``: two 32-bit words.  Returns uint32 of ``counter``'s shape."""
    c = np.asarray(counter, np.uint64) & _M32
    if c.shape[-1] != 4:
        raise ValueError("philox4x32: the counter has four words, got shape %s" % (c.shape,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(PHILOX_M0) * c0                       # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _checked_rate(rate) -> np.float32:
    r = np.float32(rate)
    if not (r >= 0 and r < 1):
        raise ValueError("dropout_rate = %r outside [0, 1)" % (rate,))
    return r


def dropout_threshold(rate) -> int:
    """``ceil(float32(rate) * 2^24)``: an element is kept iff its 24-bit value ``k >= threshold``, i.e. ``k * 2^-24 >= rate``."""
    return int(np.ceil(np.float64(_checked_rate(rate)) * 16777216.0))


def dropout_scale(rate) -> np.float32:
    """``1 / (1 - rate)`` as one float32 division: what a kept value is multiplied by."""
    return np.float32(1.0) / (np.float32(1.0) - _checked_rate(rate))


def dropout_sites(graph: Graph, depth: int = 2):
    """``{site: (name, size)}`` of the dropout sites of a trainer: every site at or behind the cached feature.  Site 0 (depth 3
    only) is ``s6.bn``, NHWC within the item; site 1 the last conv block's output as dense 0 reads it; site ``2 + d`` the output of
    dense block ``d`` (the last block's logits included).  The reference's dropout behind the frozen conv blocks upstream of the
    cache cannot be applied to cached features and is not there."""
    depth = _checked_depth(depth)
    sites = {}
    if depth == 3:
        s6 = graph.stages[-4]
        sites[0] = ("s%d.bn" % s6.index, s6.out_side * s6.out_side * s6.cout)
    s9 = graph.stages[-1]
    sites[1] = ("flat", s9.out_side * s9.out_side * s9.cout)
    for d, layer in enumerate(graph.dense):
        sites[2 + d] = (layer.name, int(layer.nout))
    return sites


# ---- training views (csrc/rn_views.h, include/roomnet_hip.h: fine-tuning on fresh random views)
VIEW_SITE = 254                          # a site no dropout site can take: view draws and dropout masks never share a counter
VIEW_CROP, VIEW_FLIP = 1, 2              # RN_VIEW_CROP, RN_VIEW_FLIP


def view_flags(crop=True, flip=True) -> int:
    return (VIEW_CROP if crop else 0) | (VIEW_FLIP if flip else 0)


def view_counter(step, slot):
    """The Philox counter of the view draw of minibatch slot ``slot`` at global step ``step``:
    ``(0, slot, step & 0xffffffff, VIEW_SITE | (step >> 32) << 8)``."""
    step = int(step)
    return (0, int(slot), step & 0xFFFFFFFF, (VIEW_SITE | ((step >> 32) << 8)) & 0xFFFFFFFF)


def center_crop_window(height, width):
    """``(x0, y0, side)`` of the centred square window of network.py:137-146 (``rn_center_crop_window``)."""
    height, width = int(height), int(width)
    if width > height:
        return (width - height) // 2, 0, height
    return 0, abs((width - height) // 2), width


def view_draw(seed, step, slot, height, width, crop=True, flip=True):
    """The view the feeder's augmentation gives minibatch slot ``slot`` at global step ``step`` of a ``height x width`` photograph
    (``rn_view_draw``): ``{"x0", "y0", "side", "fliplr", "flipud"}``.  ``crop``: a random square window slid along the long axis
    (generator.py:52-67), offset ``word0 * range >> 32`` in ``[0, range)`` with ``range = max(h, w) - min(h, w)`` (0: the whole
    image); otherwise the centre window.  ``flip``: each mirror with probability 1/2 (generator.py:85-92), ``word1 >> 31`` and
    ``word2 >> 31``.  The words are ``philox4x32(view_counter(step, slot), (seed & 0xffffffff, seed >> 32))``; NumPy's own stream
    is not reproduced, the distribution and the sampling rules are."""
    seed, step, slot, height, width = int(seed), int(step), int(slot), int(height), int(width)
    if seed < 0 or seed >> 64 or step < 0 or slot < 0 or height < 1 or width < 1:
        raise ValueError("view_draw: seed %d, step %d, slot %d, image %dx%d" % (seed, step, slot, width, height))
    w = [int(x) for x in philox4x32(view_counter(step, slot), (seed & 0xFFFFFFFF, seed >> 32))]
    side, rng = min(height, width), abs(height - width)
    x0, y0, _ = center_crop_window(height, width)
    if crop:
        offset = (w[0] * rng) >> 32
        x0, y0 = (offset, 0) if height < width else (0, offset)
    return {"x0": x0, "y0": y0, "side": side, "fliplr": (w[1] >> 31) if flip else 0, "flipud": (w[2] >> 31) if flip else 0}


def make_view(im, draw, S) -> np.ndarray:
    """The ``[S, S, 3]`` view ``draw`` (of ``view_draw``) takes of the BGR uint8 photograph ``im``:
    ``flipud(fliplr(resize(window, (S, S))))``, the flips behind the resize as in the reference's ``preprocess_set``."""
    from .imageops import resize_linear_u8
    x0, y0, side = draw["x0"], draw["y0"], draw["side"]
    out = resize_linear_u8(np.asarray(im)[y0:y0 + side, x0:x0 + side], int(S), int(S))
    if draw["fliplr"]:
        out = out[:, ::-1]
    if draw["flipud"]:
        out = out[::-1]
    return np.ascontiguousarray(out)


def dropout_keep(seed, step, slot, site, count, rate) -> np.ndarray:
    """The keep mask (bool ``[count]``) of elements ``0 .. count - 1`` of ``site`` in minibatch slot ``slot`` at global step
    ``step``: key ``(seed & 0xffffffff, seed >> 32)``, counter ``(e >> 2, slot, step & 0xffffffff, site | (step >> 32) << 8)``,
    word ``e & 3`` of the output, kept iff ``word >> 8 >= dropout_threshold(rate)``."""
    seed, step, count = int(seed), int(step), int(count)
    if seed < 0 or seed >> 64 or step < 0 or count < 0:
        raise ValueError("dropout_keep: seed %d, step %d, count %d" % (seed, step, count))
    thr = dropout_threshold(rate)
    quads = (count + 3) // 4
    ctr = np.empty((quads, 4), np.uint64)
    ctr[:, 0] = np.arange(quads, dtype=np.uint64)
    ctr[:, 1] = int(slot)
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = (int(site) | ((step >> 32) << 8)) & 0xFFFFFFFF
    words = philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:count]
    return (words >> np.uint32(8)) >= np.uint32(thr)
