"""Host restatement of the batch-moments reduction of roomnet_amd/csrc/rn_bnstats.hip (pure NumPy; imports nothing from the library).

The kernel reduces a NHWC float32 tensor, seen as ``total4`` float4 of which C / 4 consecutive ones are a pixel, to per-channel
(mean, biased variance):

  partition  ``moments_blocks(total4)`` workgroups of 256 threads (at most 2048; short tensors: one per 2048 float4); thread
             ``gid = workgroup * 256 + tid`` reads float4 ``gid, gid + stride, gid + 2 stride, ...`` with ``stride = workgroups * 256``:
             four per trip while four are left (the unrolled loop), then one per trip (the remainder loop);
  thread     float32 Welford over those float4, one count and one reciprocal for the four channels of a float4;
  lanes      Chan merges in float64 by xor shuffles 32, 16, ... down to C / 4: lanes l, l + C / 4, ... hold the same channels;
  waves      lanes < C / 4 of each of the four wavefronts write an LDS slot; thread 4 g + j merges slot 0 with 1, 2, 3 in turn;
  finalise   one wavefront per channel: lane l sums workgroups l, l + 64, ...; xor butterfly; mean = sum n_b mean_b / sum n_b,
             M2 = sum M2_b + sum n_b (mean_b - mean)^2, variance = M2 / sum n_b.

``plan`` restates the partition and the tree, ``model_f32`` the arithmetic (float32 Welford with the fused multiply-adds emulated
through float64, then the float64 merges in the kernel's order), ``exact`` is a two-pass float64 reference, ``mutants`` are wrong
reductions on the same partition and ``bound`` is the bound of the local moment check (tests/test_hip_bnstats_local.py).
"""
import numpy as np

THREADS = 256
MAX_BLOCKS = 2048
MIN_F4_PER_THREAD = 8
WAVE = 64
WAVES = THREADS // WAVE
FLOOR = 2.0 ** -22          # of absmax(x) (mean) / absmax(x)^2 (variance): see ``bound``
FACTOR = 4.0                # parity_bounds._tol's rule: "another summation order and nothing else"


def moments_blocks(total4):
    per_block = THREADS * MIN_F4_PER_THREAD
    return int(min(max((int(total4) + per_block - 1) // per_block, 1), MAX_BLOCKS))


class Plan:
    """The partition of ``total4`` float4 with ``C`` channels, and the merge tree above it."""

    def __init__(self, total4, C):
        G = C // 4
        assert C % 4 == 0 and 2 <= G <= 32 and G & (G - 1) == 0, C
        assert total4 >= 1, total4
        self.total4, self.C, self.G = int(total4), int(C), G
        self.blocks = moments_blocks(total4)
        self.stride = self.blocks * THREADS
        self.threads = self.stride                                       # gid = block * 256 + tid in [0, threads)
        self.lane_offsets = [off for off in (32, 16, 8, 4, 2, 1) if off >= G]      # xor distances of the lane merges, in order
        self.waves = WAVES                                               # LDS slots per workgroup, merged 0 <- 1 <- 2 <- 3
        self.finalise_lanes = WAVE                                       # lane l of the finalise launch takes workgroups l, l + 64, ...
        self._counts = None

    def steps(self):
        """The kernel's two loops, all threads at once.  Yields ``(gids, index, unrolled)`` per Welford step, in the order a
        thread runs them: ``gids`` the threads that take this step, ``index`` the float4 each of them reads."""
        gid = np.arange(self.threads, dtype=np.int64)
        i = gid.copy()
        s, total4 = self.stride, self.total4
        while True:                                                      # for (; i + 3 * stride < total4; i += 4 * stride)
            act = np.flatnonzero(i + 3 * s < total4)
            if act.size == 0:
                break
            for u in range(4):
                yield act, i[act] + u * s, True
            i[act] += 4 * s
        while True:                                                      # for (; i < total4; i += stride)
            act = np.flatnonzero(i < total4)
            if act.size == 0:
                break
            yield act, i[act], False
            i[act] += s

    def counts(self):
        """``(unrolled, remainder)``: per thread, how many float4 each loop reads."""
        if self._counts is None:
            un = np.zeros(self.threads, np.int64)
            rem = np.zeros(self.threads, np.int64)
            for gids, _idx, unrolled in self.steps():
                (un if unrolled else rem)[gids] += 1
            self._counts = (un, rem)
        return self._counts

    def per_thread(self):
        """Sorted distinct per-thread float4 counts (threads that read nothing included as 0)."""
        un, rem = self.counts()
        return sorted(set((un + rem).tolist()))

    def indices(self, block, tid):
        """The float4 indices thread ``tid`` of workgroup ``block`` reads, in order: ``(unrolled list, remainder list)``."""
        g = block * THREADS + tid
        un, rem = [], []
        for gids, idx, unrolled in self.steps():
            k = np.searchsorted(gids, g)
            if k < gids.size and gids[k] == g:
                (un if unrolled else rem).append(int(idx[k]))
        return un, rem

    def describe(self):
        un, rem = self.counts()
        return {"workgroups": self.blocks, "stride": self.stride, "per_thread": self.per_thread(),
                "unrolled_trips": sorted(set((un // 4).tolist())), "remainder_steps": sorted(set(rem.tolist())),
                "lane_offsets": self.lane_offsets}


def plan(total4, C):
    return Plan(total4, C)


def _as_f4(x, C):
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.size % C == 0 and x.shape[-1] == C, (x.shape, C)
    return x.reshape(-1, 4)


def _thread_moments(x4, pl, dtype, rcp="nearest", skip=None):
    """Welford per thread over the plan's steps.  float32: the kernel's arithmetic -- d = x - mean; mean = fma(d, r, mean);
    M2 = fma(d, x - mean, M2), the fused multiply-adds through float64 (the product of two float32 is exact there), r =
    float32(1) / float32(k) (``rcp``: that value, or its neighbour below / above).  float64: the same recurrence in float64
    with r = 1 / k.  ``skip(index, unrolled)`` -> bool mask of float4 a mutant leaves out.  Returns (n [T], mean [T, 4], M2 [T, 4])
    as float64."""
    T = pl.threads
    n = np.zeros(T, np.int64)
    mean = np.zeros((T, 4), dtype)
    m2 = np.zeros((T, 4), dtype)
    for gids, idx, unrolled in pl.steps():
        if skip is not None:
            keep = ~skip(idx, unrolled)
            gids, idx = gids[keep], idx[keep]
            if gids.size == 0:
                continue
        xs = x4[idx]
        whole = gids.size == T                                           # (a full step: no gather / scatter of the state)
        n_g = n if whole else n[gids]
        n_g = n_g + 1
        mu = mean if whole else mean[gids]
        q = m2 if whole else m2[gids]
        if dtype == np.float32:
            r = np.float32(1) / n_g.astype(np.float32)
            if rcp != "nearest":                                         # (a power of two has an exact reciprocal: left alone)
                r = np.where(n_g & (n_g - 1) == 0, r, np.nextafter(r, np.float32(0 if rcp == "down" else 2)))
            d = xs - mu
            d64 = d.astype(np.float64)
            mu = (d64 * r.astype(np.float64)[:, None] + mu.astype(np.float64)).astype(np.float32)
            q = (d64 * (xs - mu).astype(np.float64) + q.astype(np.float64)).astype(np.float32)
        else:
            xs = xs.astype(np.float64)
            d = xs - mu
            mu = mu + d / n_g[:, None]
            q = q + d * (xs - mu)
        if whole:
            n, mean, m2 = n_g, mu, q
        else:
            n[gids], mean[gids], m2[gids] = n_g, mu, q
    return n.astype(np.float64), mean.astype(np.float64), m2.astype(np.float64)


def _chan(na, ma, qa, nb, mb, qb):
    """chan_merge of the kernel, float64, elementwise (n broadcast over the four channels of a float4)."""
    n = na + nb
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(n > 0, nb / np.where(n > 0, n, 1.0), 0.0)
    d = mb - ma
    return n, ma + d * f, qa + qb + d * d * na * f


def _workgroup_partials(pl, n, mean, m2, lose_slot=None):
    """Lane merges, LDS slots, wave merge -> per-workgroup partials (n [B], mean [B, C], M2 [B, C]).  ``lose_slot = (block, wave)``
    empties that LDS slot before the wave merge (a mutant)."""
    B, G = pl.blocks, pl.G
    n = n.reshape(B, WAVES, WAVE, 1)
    mean = mean.reshape(B, WAVES, WAVE, 4)
    m2 = m2.reshape(B, WAVES, WAVE, 4)
    for off in pl.lane_offsets:                                          # lane l < off: l ^ off = l + off
        n, mean, m2 = _chan(n[:, :, :off], mean[:, :, :off], m2[:, :, :off], n[:, :, off:2 * off], mean[:, :, off:2 * off], m2[:, :, off:2 * off])
    n, mean, m2 = n[:, :, :G].copy(), mean[:, :, :G].copy(), m2[:, :, :G].copy()      # the LDS slots [B, waves, G, .]
    if lose_slot is not None:
        b, w = lose_slot
        n[b, w], mean[b, w], m2[b, w] = 0.0, 0.0, 0.0
    na, ma, qa = n[:, 0], mean[:, 0], m2[:, 0]
    for w in range(1, WAVES):
        na, ma, qa = _chan(na, ma, qa, n[:, w], mean[:, w], m2[:, w])
    # thread 4 g + j writes channel 4 g + j
    return np.broadcast_to(na, (B, G, 4)).reshape(B, pl.C).copy(), ma.reshape(B, pl.C), qa.reshape(B, pl.C)


def _butterfly(v):
    """v [64, C] per-lane sums -> lane 0's value after v += shfl_xor(v, off), off = 32 ... 1."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:off] + v[off:2 * off]
    return v[0]


def _finalise(pl, pn, pm, pq):
    """The k-way merge of the finalise launch.  pn, pm, pq: [parts, C].  Returns float64 (mean, var, merged n) per channel."""
    C = pn.shape[1]

    def lane_sums(terms):
        v = np.zeros((WAVE, C))
        for b in range(terms.shape[0]):
            v[b % WAVE] += terms[b]
        return v

    sn = _butterfly(lane_sums(pn))
    snm = _butterfly(lane_sums(pn * pm))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = snm / sn
        d = pm - mean
        q = _butterfly(lane_sums(pq + pn * d * d))
        return mean, q / sn, sn


def model_f32(x, C, rcp="nearest"):
    """(mean, var) float32 [C] as the kernel computes them, up to: the contraction of float64 expressions, the rounding of
    the hardware's reciprocal (``rcp``), double rounding of the emulated float32 fma."""
    x4 = _as_f4(x, C)
    pl = plan(x4.shape[0], C)
    mean, var, _ = _finalise(pl, *_workgroup_partials(pl, *_thread_moments(x4, pl, np.float32, rcp)))
    return mean.astype(np.float32), var.astype(np.float32)


def model_count(x, C):
    """The count the finalise launch merges per channel (all equal): total4 / (C / 4)."""
    x4 = _as_f4(x, C)
    return x4.shape[0] // (C // 4)


def exact(x, C, chunk=1 << 20):
    """Two-pass float64 (mean, biased variance) per channel, in chunks of rows."""
    x2 = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, C)
    n = x2.shape[0]
    s = np.zeros(C)
    for i in range(0, n, chunk):
        s += x2[i:i + chunk].sum(0, dtype=np.float64)
    mean = s / n
    q = np.zeros(C)
    for i in range(0, n, chunk):
        d = x2[i:i + chunk].astype(np.float64) - mean
        q += (d * d).sum(0)
    return mean, q / n


def absmax(x):
    x = np.asarray(x)
    return float(max(x.max(), -x.min()))


def bound(x, C, rcp_modes=("nearest",), want=None):
    """(mean bound, variance bound) of the local moment check: max(4 x max |model_f32 - exact|, 2^-22 x absmax(x)) and the same with
    absmax(x)^2.  The factor 4 is tests/parity_bounds._tol's rule; the floor pays for the float32 rounding of the result
    (2^-24 relative) and for a reciprocal one ulp off the model's (k steps of mean += d r move the mean by <= k 2^-24 |d| / k).
    ``rcp_modes``: the model's deviation is the worst over these reciprocal roundings.  Also returns the model's own errors."""
    m64, v64 = exact(x, C) if want is None else want
    em = ev = 0.0
    for mode in rcp_modes:
        m32, v32 = model_f32(x, C, mode)
        em = max(em, float(np.abs(m32.astype(np.float64) - m64).max()))
        ev = max(ev, float(np.abs(v32.astype(np.float64) - v64).max()))
    a = absmax(x)
    return max(FACTOR * em, FLOOR * a), max(FACTOR * ev, FLOOR * a * a), em, ev


def bound_two_pass(x):
    """Bound for the dense BNs' moments (dense_bn_batch_kernel: float64 two-pass over n values, one float32 rounding of each
    result, 2^-24 relative): the floor of ``bound`` alone."""
    a = absmax(x)
    return FLOOR * a, FLOOR * a * a


MUTANTS = ("workgroup_lost", "last_workgroup_lost", "wave_slot_lost", "remainder_loop_lost", "tail_past_last_whole_stride_lost",
           "workgroup_merged_twice", "workgroup_n_off_by_one_float4")


def mutants(x, C, kinds=MUTANTS):
    """Wrong reductions on the kernel's partition, in float64: ``{name: (mean [C], var [C], merged count)}``.  A mutant that is
    the identity on this partition (no remainder step, no ragged tail, a single workgroup to lose or double, a single occupied
    LDS slot) is left out; one that loses every element returns NaN moments.  The workgroup a mutant hits is the middle one
    (``blocks // 2``), the wave slot the last occupied one of that workgroup; the n-off-by-one mutant hits the workgroup whose mean
    lies farthest from the tensor's in any channel, relative to absmax(x) (where the moments can show it best).  ``kinds``: compute
    these only."""
    x4 = _as_f4(x, C)
    pl = plan(x4.shape[0], C)
    un, rem = pl.counts()
    B, b = pl.blocks, pl.blocks // 2
    tn, tm, tq = _thread_moments(x4, pl, np.float64)
    pn, pm, pq = _workgroup_partials(pl, tn, tm, tq)
    out = {}

    def fin(n, m, q):
        mean, var, sn = _finalise(pl, n, m, q)
        return mean, var, float(sn[0])

    keep = np.ones(B, bool)
    if B >= 2:
        keep[b] = False
        out["workgroup_lost"] = fin(pn[keep], pm[keep], pq[keep])
        out["last_workgroup_lost"] = fin(pn[:-1], pm[:-1], pq[:-1])
        dup = np.concatenate([np.arange(B), [b]])
        out["workgroup_merged_twice"] = fin(pn[dup], pm[dup], pq[dup])
    occupied = [w for w in range(WAVES) if tn.reshape(B, WAVES, WAVE)[b, w].sum() > 0]
    if len(occupied) >= 2:
        out["wave_slot_lost"] = fin(*_workgroup_partials(pl, tn, tm, tq, lose_slot=(b, occupied[-1])))
    if rem.any() and "remainder_loop_lost" in kinds:
        out["remainder_loop_lost"] = fin(*_workgroup_partials(pl, *_thread_moments(x4, pl, np.float64, skip=lambda idx, unrolled: np.full(idx.shape, not unrolled))))
    whole = (pl.total4 // pl.stride) * pl.stride
    if whole != pl.total4 and "tail_past_last_whole_stride_lost" in kinds:
        out["tail_past_last_whole_stride_lost"] = fin(*_workgroup_partials(pl, *_thread_moments(x4, pl, np.float64, skip=lambda idx, unrolled: idx >= whole)))
    mean = (pn * pm).sum(0) / pn.sum(0)
    far = int(np.argmax(np.abs(pm - mean).max(1) * (pn[:, 0] > 0)))
    n1 = pn.copy()
    n1[far] += 1.0
    out["workgroup_n_off_by_one_float4"] = fin(n1, pm, pq)
    return {k: v for k, v in out.items() if k in kinds}


def conv_bn_form(x, mean32, var32, gamma, beta, eps):
    """bn_f32_kernel on the table bn_finalise_kernel writes, evaluated in float64 on float32 inputs: inv = (1 / sqrt(var + eps)) *
    gamma in float32 steps; y = (x - mean) * inv + beta.  Returns (y float64, per-element bound 2^-22 (|x - mean| |inv| + |beta|)):
    three float32 roundings (difference, product, sum) of terms no larger than |x - mean| |inv| + |beta|, 2^-24 each."""
    inv = _inv32(var32, gamma, eps).astype(np.float64)
    d = np.asarray(x, np.float64) - np.asarray(mean32, np.float64)
    b = np.asarray(beta, np.float64)
    return d * inv + b, 2.0 ** -22 * (np.abs(d) * np.abs(inv) + np.abs(b))


def dense_bn_form(x, mean32, var32, gamma, beta, eps):
    """dense_bn_batch_kernel: y = x * inv + (beta - mean * inv), evaluated in float64 on the float32 mean, inv (formed in float32
    steps as the kernel forms it) and beta.  The kernel rounds four times (mean * inv, beta - that, x * inv, the sum), one more
    than the conv form, and its terms are |x inv|, |mean inv| and |beta| rather than |x - mean| |inv|: the bound is
    2^-22 (|x inv| + |mean inv| + |beta|) -- four roundings of 2^-24 of terms no larger than that sum."""
    inv32 = _inv32(var32, gamma, eps)
    m32 = np.asarray(mean32, np.float32)
    inv, m, b = inv32.astype(np.float64), m32.astype(np.float64), np.asarray(beta, np.float64)
    x = np.asarray(x, np.float64)
    return x * inv + (b - m * inv), 2.0 ** -22 * (np.abs(x * inv) + np.abs(m * inv) + np.abs(b))


def _inv32(var32, gamma, eps):
    v = np.asarray(var32, np.float32)
    s = np.sqrt(v + np.float32(eps), dtype=np.float32)
    return ((np.float32(1) / s).astype(np.float32) * np.asarray(gamma, np.float32)).astype(np.float32)


def bn_inputs(graph):
    """[(BN output node, the tap holding the BN's input, channels, side)] of a graph's 13 conv-side BNs, in variable order
    (``graph``: anything with ``stages`` carrying index, cout, out_side, pool_k, residual)."""
    out = []
    for s in graph.stages:
        out.append(("s%d.bn" % s.index, "s%d.%s" % (s.index, "pool" if s.pool_k else "conv"), s.cout, s.out_side))
        if s.residual:
            out.append(("s%d.bn2" % s.index, "s%d.add" % s.index, s.cout, s.out_side))
    return out
