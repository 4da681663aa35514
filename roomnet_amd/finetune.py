"""Host side of fine-tuning stages 8-9 and the dense head (``RoomNet.fine_tune``, C ABI ``rn_ft_*``): which variables are
trained, the learning-rate schedule, the minibatch order and a NumPy statement of the Adam rule.  Pure host code; the
mathematics is stated once in the header of ``csrc/rn_finetune.hip``."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .graph import Graph

DECAY_RATE = 0.068                       # network.py:36
ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON = 0.9, 0.999, 1e-8      # tf.train.AdamOptimizer defaults


def trained_variables(graph: Graph) -> List[str]:
    """Checkpoint names of the variables ``rn_ft_*`` trains, in the trainer's order: the last two conv stages' kernels and BN
    gamma / beta (both BNs of the residual stage), then per dense layer its kernel and its BN's gamma / beta or its bias."""
    names = []
    for s in graph.stages[-2:]:
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


def feature_shape(graph: Graph) -> Tuple[int, int, int]:
    """Per-image shape of the cached feature ``s7.bn``: the output of the last block's first step."""
    s = graph.stages[-3]
    return s.out_side, s.out_side, s.cout


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
