"""Bounds and comparison helpers that more than one test module uses, stated once: a test module imports them from here and never
from another test module.  Each keeps the value and the body it had where it was first written; the comments say where that was."""
import numpy as np

# ---- tests/test_hip_fused.py: the 16-bit path against the oracle
MARGIN = 0.2              # ids are compared where the fp64 top-2 logit margin exceeds this
# max |err| / absmax of the stage output.  Observed (profiles/r3_parity.json): bf16 <= 0.0067 at 224 and <= 0.0059 at 600,
# f16 <= 0.0048 / 0.0024: the bounds sit at about twice that (round 2 carried 0.04 for bf16)
STAGE_TOL = {"bf16": 0.0125, "f16": 0.006}
# never written to HBM on a default handle: s0.bn lives in the private LDS rings of stage 1's kernel (rn_stage_rw.hip,
# S0F), s2.bn in the B ring of the fused stage pair (rn_stage23.hip)
FUSED_AWAY = {"s0.bn", "s2.bn"}

# ---- tests/test_hip_other_checkpoints.py (d): an exact float64 tie counts only if every tied pre-activation is this far from 0 and 6
TIE_EDGE = 1e-3
# ---- tests/test_checkpoints_host.py: live(gain 2.5), per stage 1-9, share at exactly 6 / strictly inside (0, 6)
AT_CLAMP_MIN, INSIDE_MIN = 0.005, 0.15


# ---- tests/test_hip_bnstats.py: max(1e-4 of the fp64 tensor's abs-max, 4 x the float32 CPU restatement's own deviation from fp64)
def _tol(want64, got32, scale=None):
    scale = float(np.abs(want64).max()) if scale is None else scale
    return max(1e-4 * max(scale, 1e-3), 4.0 * float(np.abs(np.asarray(got32, np.float64) - want64).max()))


def _same_up_to_sum_order(a, b, dtype, what, frac=1e-4, n_ulp=6):
    """Equal up to the fp32 ORDER of sums, where it shows through the 16-bit rounding.  Two sources: (1) the fused pair adds
    its fp16 pooling terms in 16x16x32 MFMAs, the stage kernels in 32x32x16 ones; (2) round 5: on the shipped checkpoint the
    pair's second conv contracts 16 of the 32 channels of its input on the matrix cores and takes the other 16 -- FROZEN
    channels, constants for every image (rn_fused_prepare proves it) -- as one per-cout constant summed on the host in double:
    the same products, another summation order (and the channels sit in another order inside a tap).  Seen: 2-3e-5 of the
    elements of s3.bn2 off by one 16-bit ulp (f16; bf16 5e-6), single elements near zero by up to 3 ulps of the 1 % floor;
    downstream tensors inherit it (`frac`, `n_ulp` wider there).  The bound per element stays a few 16-bit ulps: a corrupted
    tile is orders of magnitude outside it."""
    bad = a != b
    n = int(bad.sum())
    if n == 0:
        return
    ulp = 2.0 ** (-8 if dtype == "bf16" else -11)
    scale = float(np.abs(b).max())
    # bounded PER ELEMENT: n_ulp 16-bit ulps of the element itself (values below 1 % of the tensor's abs-max are measured
    # against that floor: a folded-BN output near zero is a difference of two larger numbers)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    lim = n_ulp * ulp * np.maximum(np.abs(b.astype(np.float64)), 0.01 * scale)
    worst = float((d / lim).max())
    # (tensors of a few hundred elements -- s9.bn2 is 2 x 2 x 16 per image -- get a floor of 32 differing elements: every one of
    #  them sums the whole image, a handful of one-ulp flips upstream moves more than `frac` of them)
    assert n <= max(32 if a.size < 4096 else 2, frac * a.size) and worst <= 1.0, (what, dtype, n, a.size, worst, np.argwhere(bad)[:4].tolist())


def _downstream_same(fused, plain, names, nb, dtype, probs_f, probs_p, ids_f, ids_p):
    for name in names:
        if name.startswith("d"):              # the fp32 logits: every element moves a little, none by much
            np.testing.assert_allclose(fused.tap(name, nb), plain.tap(name, nb), rtol=0, atol=1e-2, err_msg=name)
            continue
        _same_up_to_sum_order(fused.tap(name, nb), plain.tap(name, nb), dtype, name, frac=6e-2, n_ulp=12)
    np.testing.assert_allclose(probs_f, probs_p, rtol=0, atol=2e-3)
    np.testing.assert_array_equal(ids_f, ids_p)
