"""Host arithmetic of BN recalibration: what the reference's update ops do with a batch's moments
(``network.py:64-67``: ``tf.GraphKeys.UPDATE_OPS`` of ``tf.layers.batch_normalization(training=True)``).

Pure NumPy on 32 short vectors -- no device, no oracle.  The moments themselves come from the GPU
(``Engine.bn_batch_stats`` on a ``batch_stats`` engine, ``rn_bn_batch_stats``).

Like the rest of the oracle this is argued from the TF-1.13 op semantics (``assign_moving_average`` in
``tf.layers``' BatchNormalization, the CPU FusedBatchNorm kernel, ``tf.nn.moments``) and is unpinned against
TensorFlow itself.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from .graph import Graph

Moments = Dict[str, Tuple[np.ndarray, np.ndarray, int]]      # bn prefix -> (mean, var_biased, count)


def moving_update(moving, batch_value, momentum: float) -> np.ndarray:
    """TensorFlow's ``assign_moving_average`` in float32: ``moving - (moving - value) * float32(1.0 - momentum)``.
    The decay ``1.0 - momentum`` is formed in Python double and then cast, as ``ops.convert_to_tensor`` does."""
    moving = np.asarray(moving, np.float32)
    value = np.asarray(batch_value, np.float32)
    decay = np.float32(1.0 - momentum)
    return (moving - (moving - value) * decay).astype(np.float32)


def variance_for_update(var_biased, count: int, rank: int) -> np.ndarray:
    """The variance that enters the moving-variance update, float32.

    rank 4 (the conv-side BNs: ``tf.layers`` takes the fused kernel, whose training output is Bessel-corrected):
    ``var_biased * (float32(N) / float32(N - 1))`` with N = n * h * w (N = 1: the factor is 1, as in the kernel).
    rank 2 (the dense BNs: unfused path through ``tf.nn.moments``): the biased variance itself."""
    var = np.asarray(var_biased, np.float32)
    if rank == 2:
        return var.copy()
    if rank != 4:
        raise ValueError("variance_for_update: rank must be 4 (conv-side BN) or 2 (dense BN), got %r" % (rank,))
    n = int(count)
    if n < 1:
        raise ValueError("variance_for_update: count must be >= 1, got %d" % n)
    return (var * (np.float32(n) / np.float32(max(n - 1, 1)))).astype(np.float32)


def bn_ranks(graph: Graph) -> Dict[str, int]:
    """BN variable prefix -> rank of its input (4: conv side, 2: dense), in the reference's variable order."""
    out: Dict[str, int] = {}
    for s in graph.stages:
        out[s.bn_name] = 4
        if s.bn2_name:
            out[s.bn2_name] = 4
    for d in graph.dense:
        if d.bn_name:
            out[d.bn_name] = 2
    return out


def updated_statistics(graph: Graph, variables: Dict[str, np.ndarray], batches: Iterable[Moments],
                       momentum: Optional[float] = 0.99) -> Dict[str, np.ndarray]:
    """New ``moving_mean`` / ``moving_variance`` of every BN after the given batches' moments.

    ``momentum`` a number: the reference's rule, one ``moving_update`` per batch in order (``tf.layers`` default 0.99).
    ``momentum=None``: the equal-weight average of the per-batch means and of the per-batch ``variance_for_update`` over all
    batches given (summed in float64, stored as float32) -- the practical AdaBN form; the old values do not enter."""
    ranks = bn_ranks(graph)
    batches = list(batches)
    if not batches:
        raise ValueError("updated_statistics: no batches")
    out: Dict[str, np.ndarray] = {}
    for bn, rank in ranks.items():
        means = [np.asarray(b[bn][0], np.float32) for b in batches]
        varis = [variance_for_update(b[bn][1], b[bn][2], rank) for b in batches]
        if momentum is None:
            out[bn + "/moving_mean"] = (np.sum(np.asarray(means, np.float64), 0) / len(means)).astype(np.float32)
            out[bn + "/moving_variance"] = (np.sum(np.asarray(varis, np.float64), 0) / len(varis)).astype(np.float32)
            continue
        mm = np.asarray(variables[bn + "/moving_mean"], np.float32)
        mv = np.asarray(variables[bn + "/moving_variance"], np.float32)
        for m, v in zip(means, varis):
            mm = moving_update(mm, m, momentum)
            mv = moving_update(mv, v, momentum)
        out[bn + "/moving_mean"] = mm
        out[bn + "/moving_variance"] = mv
    return out
