"""Host side of fine-tuning the last conv stages and the dense head (``RoomNet.fine_tune``, C ABI ``rn_ft_*``): which variables are
trained, the learning-rate schedule, the minibatch order and a NumPy statement of the Adam rule.  Pure host code; the
mathematics is stated once in the headers of ``csrc/rn_finetune.hip`` and ``csrc/rn_finetune7.hip``.

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
