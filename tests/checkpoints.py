"""Seeded checkpoint recipes for the parity tests that must not depend on the shipped checkpoint (pure NumPy).

The shipped checkpoint has activations of O(1e-2) (the upper end of ReLU6 is practically never reached), many BN gammas of
about 1e-20 (frozen channels) and six classes.  These recipes give the opposite: O(1) activations, every BN live with both signs
of gamma and non-zero mean and beta, any head width.  tests/test_checkpoints_host.py asserts on the fp64 oracle that they do what
the GPU tests rely on."""
import numpy as np

from roomnet_amd.network import _initializer_values

PARITY_IDX = [14, 30, 2]      # the parity images the stage-output tests of the shipped checkpoint use
ONE_IMAGE_IDX = [30]         # the one of them that reaches the clamp in EVERY stage 1-9 on its own; a checkerboard of period 32:
                             # its stage outputs are constant over whole regions (tests/test_seam_cases_host.py)
# the clamp image plus the textured one (low-pass noise on an 8-pixel grid: neighbouring columns and rows differ at every stage
# output): together they reach the clamp in every stage AND show an error of indexing (the side-240 and the seam cases)
SEAM_IDX = [30, 14]
# sides at which the tuned 16-bit kernels cut their rows into two or three column blocks (tests/block_plans.py); 600 is the
# reference's own default side
SEAM_SIDES = (409, 420, 600)
# sides at which stage 6 (630, next to three-block plans of the pair and of stages 4 and 5) and stages 5 and 6 (686: no plan for the
# pair or stage 4, flatten 4096, the head's limit) run FOUR column blocks with a ragged last block; 694 is the largest side with a head
FOUR_BLOCK_SIDES = (630, 686)
MAX_HEAD_SIDE = 694           # flatten 16 x 16 x 16 = 4096 = head_kernel's HEAD_MAX_FLAT; at 695 it is 17 x 17 x 16 = 4624
LIVE_GAIN = 2.5               # conv-kernel gain at which every stage 1-9 has values at the clamp AND strictly inside (0, 6)


def init_scale(graph, seed):
    """The reference's ``init()``: glorot-uniform kernels, identity BNs.  Activations are O(1) and nothing saturates."""
    return _initializer_values(graph, seed)


def live(graph, seed, gain):
    """Initializer values with every conv kernel times ``gain`` and every BN live: gamma uniform(0.5, 1.5) with a random sign,
    beta uniform(-0.5, 0.5), moving_mean uniform(0, 1), moving_variance uniform(0.5, 2); dense biases uniform(-0.5, 0.5).
    Variables are visited in sorted name order with one generator seeded by 1000 + seed."""
    w = dict(_initializer_values(graph, seed))
    rng = np.random.default_rng(1000 + seed)
    for name in sorted(w):
        leaf = name.rsplit("/", 1)[1]
        v = w[name]
        n = v.shape
        if leaf == "kernel":
            if v.ndim == 4:
                w[name] = v * np.float32(gain)
        elif leaf == "gamma":
            w[name] = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        elif leaf == "beta":
            w[name] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
        elif leaf == "moving_mean":
            w[name] = rng.uniform(0.0, 1.0, n).astype(np.float32)
        elif leaf == "moving_variance":
            w[name] = rng.uniform(0.5, 2.0, n).astype(np.float32)
        elif leaf == "bias":
            w[name] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    return w


def clamp_shares(taps, n_stages=10):
    """Per conv stage: (share of conv + ReLU6 outputs exactly at 6, share strictly inside (0, 6)) of an oracle run's taps."""
    out = []
    for k in range(n_stages):
        c = np.asarray(taps["s%d.conv" % k])
        out.append((float((c == 6).mean()), float(((c > 0) & (c < 6)).mean())))
    return out


def with_bn_gammas(weights, bn_name, frozen, seed):
    """``weights`` with every gamma of the BN ``bn_name`` set to a trained-looking value and the channels ``frozen`` to 1e-24
    (their betas to a visible constant): conftest.with_gammas' recipe for any one BN of the graph."""
    rng = np.random.default_rng(seed)
    w = dict(weights)
    n = len(w[bn_name + "/gamma"])
    g = rng.uniform(0.05, 0.4, n).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
    b = w[bn_name + "/beta"].copy()
    for c in frozen:
        g[c] = np.float32(1e-24)
        b[c] = np.float32(rng.uniform(0.002, 0.02))
    w[bn_name + "/gamma"] = g
    w[bn_name + "/beta"] = b
    w[bn_name + "/moving_variance"] = np.maximum(w[bn_name + "/moving_variance"], np.float32(0.05))
    return w


def f32_frozen_channels(weights, bn_name, eps=1e-3):
    """Channels of a stage's first BN the float32 stage kernels need not compute: y1 = ((x / 16 - mean) * inv + beta) is beta for
    every x in [0, 6] where |inv| max(|mean|, |6 - mean|) < 2^-25 |beta| (the inequality of rn_stage_f32m.hip, inv in float32)."""
    gamma, beta, mean, var = (weights[bn_name + "/" + leaf] for leaf in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv = ((np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)) * gamma).astype(np.float64)
    reach = np.maximum(np.abs(mean.astype(np.float64)), np.abs(6.0 - mean.astype(np.float64)))
    return [int(c) for c in np.nonzero(np.abs(inv) * reach * (1.0 + 1e-6) < np.abs(beta.astype(np.float64)) * 2.0 ** -25)[0]]


def take_back_stage9(graph, weights):
    """The shipped checkpoint with the float32 input-channel fold landing where no kernel variant exists at all: stages 2, 4 and 5 with
    no frozen channel (so no fold takes their place) and 11 of stage 8's 16 -- whole groups of 8 -> the fold is proposed for residual
    stage 9, whose channels are relabelled, and is taken back."""
    from conftest import with_gammas
    w = with_gammas(weights, [], [], 5)
    w = with_bn_gammas(w, graph.stages[4].bn_name, [], 6)
    return with_bn_gammas(w, graph.stages[8].bn_name, np.random.default_rng(8).choice(16, 11, replace=False), 7)
