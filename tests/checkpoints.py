"""Seeded checkpoint recipes for the parity tests that must not depend on the shipped checkpoint (pure NumPy).

The shipped checkpoint has activations of O(1e-2) (the upper end of ReLU6 is practically never reached), many BN gammas of
about 1e-20 (frozen channels) and six classes.  These recipes give the opposite: O(1) activations, every BN live with both signs
of gamma and non-zero mean and beta, any head width.  tests/test_checkpoints_host.py asserts on the fp64 oracle that they do what
the GPU tests rely on."""
import numpy as np

from roomnet_amd.network import _initializer_values

PARITY_IDX = [14, 30, 2]      # the parity images the stage-output tests of the shipped checkpoint use
ONE_IMAGE_IDX = [30]         # the one of them that reaches the clamp in EVERY stage 1-9 on its own (the side-240 case)
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
