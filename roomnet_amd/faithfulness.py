"""Deletion and insertion curves of a heat map, the NumPy statement of ``rn_faith_*`` (include/roomnet_hip.h):
take away the pixels a map ranks highest, a fraction at a time, and watch the class probability fall; start from nothing, put them
back in the same order and watch it rise.  A map that points at the evidence gives a small deletion area and a large insertion area.

For side ``S``, an image ``im [S, S, 3]`` uint8 BGR, a map ``m [S, S]`` float32 of any values, a class ``c`` and ``J`` steps with
``1 <= J <= S S``:

* order: pixels by map value descending, equal values by raster index ``y S + x`` ascending, ``-0.0`` equal to ``+0.0``, NaN behind
  everything else and NaNs among themselves by index -- ``np.argsort(-m.ravel(), kind="stable")``; ``rank[p]`` is the position of
  pixel ``p`` in that order, a permutation of ``0 .. S S - 1``;
* steps: ``n_j = (j S S) // J`` for ``j = 0 .. J``, so ``n_0 = 0`` and ``n_J = S S``;
* the fill is a BGR triple or ``"mean"``, per image and channel ``(2 sum + S S) // (2 S S)`` in integers, as occlusion defines it;
* deletion image ``j``: pixels with ``rank < n_j`` hold the fill, the rest ``im``; insertion image ``j``: pixels with ``rank >= n_j`` hold
  the fill, the rest ``im``; ``J + 1`` points per curve, every point its own forward pass, shared endpoints not deduplicated;
* pass 0 is the forward pass of the unmasked images, the class ``c_i`` is ``class_ids[i]`` or pass 0's argmax; ``modes`` is a bit mask
  (``DELETION = 1``, ``INSERTION = 2``), ``M`` its set bits, deletion first; the ``n M (J + 1)`` passes, flattened as
  ``f = (i M + mode_slot) (J + 1) + j``, run in chunks of ``max_batch`` that cross curve and image boundaries;
  ``curve[i, mode_slot, j] = p_f[c_i]``;
* ``auc[i, mode_slot] = float32((sum over j = 0 .. J - 1, ascending, of float64(c_j) + float64(c_{j+1})) / (2 J))``, a sequential
  float64 sum.
"""
import numpy as np

from .occlusion import _fill_of

DELETION, INSERTION = 1, 2
MAX_PASSES = 1 << 20             # n M (J + 1) of one call (rn_faith_plan)
_MODE_NAMES = {"deletion": DELETION, "insertion": INSERTION}


def mode_mask(modes):
    """``modes`` as the bit mask: an int 1..3, a name, or a sequence of names ("deletion", "insertion")."""
    if isinstance(modes, (int, np.integer)):
        mask = int(modes)
    else:
        names = [modes] if isinstance(modes, str) else list(modes)
        if not names or any(m not in _MODE_NAMES for m in names):
            raise ValueError("faithfulness: modes must be 'deletion', 'insertion' or both, got %r" % (modes,))
        mask = 0
        for m in names:
            mask |= _MODE_NAMES[m]
    if not 1 <= mask <= 3:
        raise ValueError("faithfulness: modes must be 1 (deletion), 2 (insertion) or 3 (both), got %r" % (modes,))
    return mask


def mode_slots(modes):
    """The curves of a call in slot order, deletion first: a list of ``DELETION`` / ``INSERTION``."""
    mask = mode_mask(modes)
    return [m for m in (DELETION, INSERTION) if mask & m]


def ranks(m):
    """``rank`` of a map of any shape (taken in raster order), in the map's shape, uint32: the position of every pixel in
    ``np.argsort(-m.ravel(), kind="stable")``."""
    m = np.asarray(m, np.float32)
    order = np.argsort(-m.ravel(), kind="stable")
    rank = np.empty(order.size, np.uint32)
    rank[order] = np.arange(order.size, dtype=np.uint32)
    return rank.reshape(m.shape)


def step_counts(S, J):
    """``[n_0 .. n_J]``, ``n_j = (j S S) // J``."""
    S, J = int(S), int(J)
    if not 1 <= J <= S * S:
        raise ValueError("faithfulness: steps = %d outside [1, %d], the pixels of a side of %d" % (J, S * S, S))
    return [(j * S * S) // J for j in range(J + 1)]


def deleted(im, rank, n_j, fill="mean"):
    """The deletion image: pixels with ``rank < n_j`` hold the fill (a BGR triple or "mean", of ``im``), the rest ``im``."""
    out = np.array(im, dtype=np.uint8, copy=True)
    out[np.asarray(rank) < n_j] = _fill_of(im, fill)
    return out


def inserted(im, rank, n_j, fill="mean"):
    """The insertion image: pixels with ``rank >= n_j`` hold the fill, the rest ``im``."""
    out = np.array(im, dtype=np.uint8, copy=True)
    out[np.asarray(rank) >= n_j] = _fill_of(im, fill)
    return out


def masked_pass(ims, rank_maps, fills, f, J, modes):
    """The masked image of the flattened pass ``f = (i M + mode_slot) (J + 1) + j`` of a call."""
    slots = mode_slots(modes)
    i, r = divmod(f, len(slots) * (J + 1))
    slot, j = divmod(r, J + 1)
    n_j = step_counts(ims.shape[1], J)[j]
    return (deleted if slots[slot] == DELETION else inserted)(ims[i], rank_maps[i], n_j, fills[i])


def chunks(n_passes, max_batch):
    """The chunk plan: ``[(first, count)]`` over the flattened passes."""
    return [(first, min(max_batch, n_passes - first)) for first in range(0, n_passes, max_batch)]


def auc(curve):
    """The area under curve(s) ``[..., J + 1]`` over ``[0, 1]``: the trapezoid sum in float64, ``j`` ascending, as float32."""
    c = np.asarray(curve, np.float32).astype(np.float64)
    J = c.shape[-1] - 1
    if J < 1:
        raise ValueError("faithfulness: a curve has at least two points")
    total = np.zeros(c.shape[:-1], np.float64)
    for j in range(J):                            # (sequential: the order of the device's sum)
        total = total + (c[..., j] + c[..., j + 1])
    return (total / (2.0 * J)).astype(np.float32)


def curves_host(forward, ims, maps, class_ids=None, steps=32, modes=3, fill="mean", max_batch=64):
    """The whole call on the host: ``forward(batch [m, S, S, 3] uint8) -> probs [m, C]`` is any forward pass, called once on the
    ``n <= max_batch`` unmasked images and once per chunk of ``max_batch`` masked ones (the chunk plan of ``rn_faith_u8_device``).
    Returns ``(curves [n, M, J + 1], aucs [n, M], ids [n], probs [n, C])``."""
    ims = np.ascontiguousarray(ims, dtype=np.uint8)
    if ims.ndim != 4 or ims.shape[1] != ims.shape[2] or ims.shape[3] != 3:
        raise ValueError("faithfulness: expected an [n,S,S,3] uint8 batch, got %s" % (ims.shape,))
    n, S = ims.shape[0], ims.shape[1]
    maps = np.asarray(maps, np.float32)
    if maps.shape != (n, S, S):
        raise ValueError("faithfulness: expected maps of shape %s, got %s" % ((n, S, S), maps.shape))
    J = int(steps)
    step_counts(S, J)
    slots = mode_slots(modes)
    M = len(slots)
    if not 1 <= n <= max_batch:
        raise ValueError("faithfulness: n = %d out of range (1..%d)" % (n, max_batch))
    n_passes = n * M * (J + 1)
    if n_passes > MAX_PASSES:
        raise ValueError("faithfulness: %d x %d x %d masked passes, more than %d" % (n, M, J + 1, MAX_PASSES))
    probs = np.asarray(forward(ims), np.float32)
    ids = probs.argmax(1).astype(np.int64)
    cls = ids if class_ids is None else np.broadcast_to(np.asarray(class_ids, np.int64), (n,))
    if ((cls < 0) | (cls >= probs.shape[1])).any():
        raise ValueError("faithfulness: class_ids outside [0, %d)" % probs.shape[1])
    rank_maps = [ranks(m) for m in maps]
    fills = [_fill_of(im, fill) for im in ims]
    curve = np.empty((n_passes,), np.float32)
    for first, count in chunks(n_passes, max_batch):
        batch = np.stack([masked_pass(ims, rank_maps, fills, first + e, J, modes) for e in range(count)])
        pw = np.asarray(forward(batch), np.float32)
        for e in range(count):
            i = (first + e) // (M * (J + 1))
            curve[first + e] = pw[e, cls[i]]
    curve = curve.reshape(n, M, J + 1)
    return curve, auc(curve), ids, probs
