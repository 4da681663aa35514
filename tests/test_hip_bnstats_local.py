"""Batch-statistics BN judged LOCALLY on the GPU: every BN's moments against the float64 two-pass moments of the very tensor the
kernel read (its input tap), and every BN's output against the float64 evaluation of the kernel's own form on the GPU's own
table -- on the ``live`` checkpoint (O(1) activations, values at the ReLU6 clamp), at full batches.

tests/test_hip_bnstats.py compares end to end within 1e-4 of the abs-max, which a lost workgroup partial passes; here

  C1  |mean - exact| <= max(4 x |model_f32 - exact|, 2^-22 absmax(x)), the variance likewise with absmax(x)^2
      (tests/bn_moments_ref.py: ``bound``; the model's own error is a fraction of the floor, so the floor decides), var >= 0,
      and the count rn_bn_batch_stats reads back from the device == n h w.  tests/test_bn_moments_host.py shows on the CPU that a lost,
      doubled or miscounted partial, a lost remainder loop and a lost tail leave this bound by a factor >= 10 (smallest: 12),
      and that the count shows the one class the moments cannot resolve.  Dense BNs (float64 two-pass on the device): the floor.
  C2  per element, |y - f64 form(x; GPU mean, var)| <= 2^-22 (|x - mean| |inv| + |beta|) for bn_f32_kernel (three float32 roundings);
      dense_bn_batch_kernel rounds four times, of x inv, mean inv and beta: 2^-22 (|x inv| + |mean inv| + |beta|)
      (bn_moments_ref.conv_bn_form / dense_bn_form).
  C3  a batch of copies of one constant-colour image: wherever the input tap is constant per channel the variance is exactly 0
      and the mean is the value, bit for bit; s0 ... s4 must be such nodes.

Cases (per-thread float4 counts from the host plan; tests/test_bn_moments_host.py asserts them):
  224 n = 1, 2     s9: 16 / 32 float4 in one workgroup; s8: one / two per thread, remainder loop only; s7 at n = 2: 2 workgroups, 6-7
                   per thread; s5: 8 per thread, no remainder step.  All 16 BNs, C1 + C2.
  224 n = 45       40 textured parity images, then 5 constant ones: s0 just over the 2048-workgroup cap (8-9 per thread), s1-s3 28-32
                   (seven or eight unrolled trips + 0-3 remainder steps), s4 13-14.  All 16 BNs, C1 + C2.  The same images with the
                   constant ones first: C1.
  224 two-colour   four black then four white images, and interleaved: C1 on the conv BNs.
  224 n = 128      C1 on s1 (90-91 per thread, the longest run tested), s5 (9 per thread at the cap, no ragged tail), s6 and the dense BNs.
  600 n = 6        s0 just over the cap at another width, s9 on 3 workgroups with a ragged tail: C1 on the conv BNs.

Every figure is recorded (``record("bn_moments_local", ...)`` -> the parity report; profiles/bn_moments_local_parity.json) before it
is asserted.
"""
import numpy as np
import pytest

import bn_moments_ref as M
import checkpoints as CK
from conftest import parity_set_of
from roomnet_amd import _capi
from roomnet_amd.graph import BN_EPSILON, build_graph

pytestmark = pytest.mark.gpu

TEXTURED_40 = list(range(8, 48))
CONSTANT_5 = [0, 1, 2, 3, 4]
CONSTANT_ONE = 6
CONV_BNS = ["s0.bn", "s1.bn", "s2.bn", "s3.bn", "s3.bn2", "s4.bn", "s5.bn", "s5.bn2", "s6.bn", "s7.bn", "s8.bn", "s9.bn", "s9.bn2"]
DENSE_BNS = ["d0.bn", "d1.bn", "d2.bn"]
ALL_BNS = CONV_BNS + DENSE_BNS
# case -> (side, parity image indices, BNs judged, C2 too)
CASES = {
    "n1": (224, [14], ALL_BNS, True),
    "n2": (224, [30, 14], ALL_BNS, True),
    "n45_constant_last": (224, TEXTURED_40 + CONSTANT_5, ALL_BNS, True),
    "n45_constant_first": (224, CONSTANT_5 + TEXTURED_40, ALL_BNS, False),
    "two_colour8": (224, [0] * 4 + [1] * 4, CONV_BNS, False),
    "two_colour8_interleaved": (224, [0, 1] * 4, CONV_BNS, False),
    "n128": (224, [8 + i % 40 for i in range(128)], ["s1.bn", "s5.bn", "s6.bn"] + DENSE_BNS, False),
    "600_n6": (600, [14, 22, 37, 11, 30, 2], CONV_BNS, False),
}
PARAMS = [(case, node) for case, (_side, _idx, nodes, _c2) in CASES.items() for node in nodes]


class _Runner:
    """One engine per (side, capacity) and one forward call per case: the tests of a case follow each other (PARAMS order)."""

    def __init__(self):
        self.engines, self.weights, self.graphs, self.sets, self.case, self.stats = {}, {}, {}, {}, None, None

    def images(self, side, idx):
        if side not in self.sets:
            self.sets[side] = parity_set_of(side)
        return self.sets[side][idx]

    def graph(self, side):
        if side not in self.graphs:
            self.graphs[side] = build_graph(6, side)
            self.weights[side] = CK.live(self.graphs[side], 0, CK.LIVE_GAIN)
        return self.graphs[side]

    def engine(self, side, n):
        cap = 128 if n > 45 else 45 if side == 224 else n
        if (side, cap) not in self.engines:
            for e in self.engines.values():              # one set of tap buffers at a time
                e.close()
            self.engines.clear()
            self.engines[(side, cap)] = _capi.Engine(self.graph(side), self.weights[side], device=0, dtype="f32", max_batch=cap, taps=True,
                                                     batch_stats=True)
        return self.engines[(side, cap)]

    def run(self, case, side, ims):
        eng = self.engine(side, len(ims))
        if self.case != case:
            eng.forward_u8(ims)
            self.stats = dict(zip(eng.bn_nodes(), eng.bn_batch_stats().items()))
            self.case = case
        return eng, self.stats

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines.clear()


@pytest.fixture(scope="module")
def runner():
    r = _Runner()
    yield r
    r.close()


def _input_tap(graph, node):
    if node in DENSE_BNS:
        return "d%s.relu" % node[1], graph.dense[int(node[1])].nout
    for bn, tap, C, _s in M.bn_inputs(graph):
        if bn == node:
            return tap, C
    raise KeyError(node)


def _moments_row(x, C, mean, var, count, dense):
    """C1's figures for one BN."""
    want_m, want_v = M.exact(x, C)
    if dense:
        bm, bv = M.bound_two_pass(x)
        model_m = model_v = 0.0
        row = {"workgroups": 1, "per_thread": [int(x.shape[0])]}
    else:
        bm, bv, model_m, model_v = M.bound(x, C, want=(want_m, want_v))
        d = M.plan(x.size // 4, C).describe()
        row = {"workgroups": d["workgroups"], "per_thread": d["per_thread"], "unrolled_trips": d["unrolled_trips"],
               "remainder_steps": d["remainder_steps"]}
    em, ev = float(np.abs(mean.astype(np.float64) - want_m).max()), float(np.abs(var.astype(np.float64) - want_v).max())
    row.update({"mean_err": em, "mean_bound": bm, "mean_err_over_bound": em / bm if bm > 0 else (0.0 if em == 0 else float("inf")),
                "var_err": ev, "var_bound": bv, "var_err_over_bound": ev / bv if bv > 0 else (0.0 if ev == 0 else float("inf")),
                "model_mean_err": model_m, "model_var_err": model_v, "absmax": M.absmax(x), "device_count": int(count),
                "count": int(x.size // C), "var_min": float(var.min())})
    return row


def _output_ratio(x, y, mean, var, gamma, beta, dense):
    """C2: max over elements of |y - form(x)| / bound, image by image."""
    form = M.dense_bn_form if dense else M.conv_bn_form
    worst = 0.0
    for i in range(x.shape[0]):
        want, b = form(x[i], mean, var, gamma, beta, BN_EPSILON)
        worst = max(worst, float((np.abs(y[i].astype(np.float64) - want) / b).max()))
    return worst


def graph_side(graph, node):
    return next(s for bn, _tap, _C, s in M.bn_inputs(graph) if bn == node)


@pytest.mark.parametrize("n", [45, 3])
def test_constant_colour_batch_is_exact(runner, record, n):
    """C3.  First Welford step: mean = x exactly; every later d is 0; every merge has d = 0; sum n_b x / sum n_b is an exact quotient
    in float64 (n_b x and their sum are exact: integers < 2^24 times a float32)."""
    ims = runner.images(224, [CONSTANT_ONE] * n)
    eng, stats = runner.run("constant%d" % n, 224, ims)
    graph = runner.graph(224)
    constant_nodes, rows = [], {}
    for node in CONV_BNS:
        _bn, (mean, var, count) = stats[node]
        tap, C = _input_tap(graph, node)
        x = eng.tap(tap, n)
        x2 = x.reshape(-1, C)
        const = np.ptp(x2, axis=0) == 0
        rows[node] = {"constant_channels": int(const.sum()), "channels": C, "device_count": int(count),
                      "var_max_on_constant": float(var[const].max()) if const.any() else 0.0,
                      "mean_is_the_value": bool(np.array_equal(mean[const], x2[0][const]))}
        if const.all():
            constant_nodes.append(node)
        else:
            rows[node].update(_moments_row(x, C, mean, var, count, False))
    print(rows)
    record("bn_moments_local", "constant_colour_n%d" % n, rows)
    for node in CONV_BNS:
        r = rows[node]
        assert r["device_count"] == n * graph_side(graph, node) ** 2, node
        assert r["var_max_on_constant"] == 0.0 and r["mean_is_the_value"], (node, r)
        if node not in constant_nodes:              # the other nodes fall under C1
            assert r["mean_err"] <= r["mean_bound"] and r["var_err"] <= r["var_bound"] and r["var_min"] >= 0, (node, r)
    missing = [node for node in ("s0.bn", "s1.bn", "s2.bn", "s3.bn", "s3.bn2", "s4.bn") if node not in constant_nodes]
    assert not missing, "input tap not constant per channel at %s" % missing


@pytest.mark.parametrize("case,node", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_moments_and_table_locally(runner, record, case, node):
    side, idx, _nodes, with_output = CASES[case]
    ims = runner.images(side, idx)
    n = len(ims)
    eng, stats = runner.run(case, side, ims)
    graph = runner.graph(side)
    bn, (mean, var, count) = stats[node]
    dense = node in DENSE_BNS
    tap, C = _input_tap(graph, node)
    x = eng.tap(tap, n)
    assert x.shape[-1] == C == mean.size == var.size
    row = _moments_row(x, C, mean, var, count, dense)
    if with_output:
        w = runner.weights[side]
        row["out_err_over_bound"] = _output_ratio(x, eng.tap(node, n), mean, var, w[bn + "/gamma"], w[bn + "/beta"], dense)
    print(case, node, row)
    record("bn_moments_local", "%s/%s" % (case, node), row)
    assert row["device_count"] == row["count"] == n * (1 if dense else x.shape[1] * x.shape[2])
    assert row["mean_err"] <= row["mean_bound"] and row["var_err"] <= row["var_bound"], row
    assert row["var_min"] >= 0
    if with_output:
        assert row["out_err_over_bound"] <= 1.0, row
