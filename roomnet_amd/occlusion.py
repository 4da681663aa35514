"""Occlusion-sensitivity maps, the NumPy statement of ``rn_occlusion_*`` (include/roomnet_hip.h): cover a
square of the network's input, run the forward pass, record how far the class probability falls, slide the square.

For side ``S``, patch ``P`` and stride ``T`` with ``1 <= T <= P <= S``:

* per axis the window positions are ``p_k = min(k T, S - P)`` for ``k = 0 .. G - 1``, ``G = ceil((S - P) / T) + 1``: the last window
  is flush with the edge; every pixel is covered because ``T <= P``; ``P = S`` gives ``G = 1``;
* window ``w = ky G + kx`` covers rows ``p_ky .. p_ky + P - 1`` and columns ``p_kx .. p_kx + P - 1`` of the ``S x S x 3`` uint8 BGR input;
* the fill is a BGR triple or ``"mean"``: per image and channel ``(2 sum + S S) // (2 S S)`` in integers;
* pass 0 is the forward pass of the unmasked images, the class ``c_i`` is ``class_ids[i]`` or pass 0's argmax; the ``n G G`` (image,
  window) pairs, flattened as ``i G G + w``, run in chunks of ``max_batch`` that cross image boundaries;
  ``drop[i, ky, kx] = p0[i, c_i] - p_w[i, c_i]`` in float32;
* ``map[i, y, x]`` = the float32 sum of ``drop[i, ky, kx]`` over the windows covering ``(y, x)``, ``ky`` ascending, then ``kx`` ascending,
  divided by ``float32(count)``.  Negative entries are kept.
"""
import numpy as np

MAX_WINDOWS = 1 << 20            # n G G of one call (rn_occlusion_plan)


def grid(S, P, T):
    """``G``, the window positions per axis."""
    S, P, T = int(S), int(P), int(T)
    if not 1 <= T <= P <= S:
        raise ValueError("occlusion: 1 <= stride <= patch <= side does not hold for stride %d, patch %d, side %d" % (T, P, S))
    return (S - P + T - 1) // T + 1


def positions(S, P, T):
    """The window positions of one axis, ``[min(k T, S - P) for k in range(G)]``."""
    return [min(k * T, S - P) for k in range(grid(S, P, T))]


def fill_colour(im):
    """The "mean" fill of one ``S x S x 3`` uint8 image: per channel the mean rounded half up, in integers."""
    im = np.asarray(im)
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
        raise ValueError("occlusion: expected an [S,S,3] uint8 image, got %s %s" % (im.dtype, im.shape))
    area = int(im.shape[0]) * int(im.shape[1])
    sums = im.reshape(-1, 3).astype(np.int64).sum(0)
    return np.array([(2 * int(s) + area) // (2 * area) for s in sums], np.uint8)


def _fill_of(im, fill):
    if isinstance(fill, str):
        if fill != "mean":
            raise ValueError("occlusion: fill must be 'mean' or a BGR triple, got %r" % (fill,))
        return fill_colour(im)
    f = np.asarray(fill)
    if f.shape != (3,) or (f < 0).any() or (f > 255).any():
        raise ValueError("occlusion: fill must be 'mean' or a BGR triple of 0..255, got %r" % (fill,))
    return f.astype(np.uint8)


def masked(im, y, x, P, fill):
    """A copy of ``im`` whose ``P x P`` window at row ``y``, column ``x`` holds ``fill`` (a BGR triple or "mean")."""
    out = np.array(im, dtype=np.uint8, copy=True)
    out[y:y + P, x:x + P] = _fill_of(im, fill)
    return out


def windows(im, P, T, fill="mean"):
    """All ``G G`` masked copies of one ``S x S x 3`` image, in window order: ``[G G, S, S, 3]`` uint8."""
    pos = positions(im.shape[0], P, T)
    f = _fill_of(im, fill)
    return np.stack([masked(im, y, x, P, f) for y in pos for x in pos], 0)


def pixel_map(drop, S, P, T):
    """``drop [G, G]`` (or ``[n, G, G]``) -> the ``S x S`` pixel map(s): per pixel the float32 sum of the drops of the windows that
    cover it, ``ky`` ascending, then ``kx`` ascending, divided by ``float32(count)``."""
    drop = np.asarray(drop, np.float32)
    pos = positions(S, P, T)
    G = len(pos)
    if drop.shape[-2:] != (G, G):
        raise ValueError("occlusion: drops of shape %s for a %d x %d grid" % (drop.shape, G, G))
    total = np.zeros(drop.shape[:-2] + (S, S), np.float32)
    count = np.zeros((S, S), np.int32)
    for ky, y in enumerate(pos):              # (every pixel's windows are visited in the stated order: the sum's order per pixel)
        for kx, x in enumerate(pos):
            total[..., y:y + P, x:x + P] += drop[..., ky, kx][..., None, None]
            count[y:y + P, x:x + P] += 1
    return total / count.astype(np.float32)


def chunks(n_windows, max_batch):
    """The chunk plan: ``[(first, count)]`` over the flattened (image, window) pairs."""
    return [(first, min(max_batch, n_windows - first)) for first in range(0, n_windows, max_batch)]


def occlusion_map_host(forward, ims, class_ids=None, patch=32, stride=16, fill="mean", max_batch=64, with_map=True):
    """The whole call on the host: ``forward(batch [m, S, S, 3] uint8) -> probs [m, C]`` is any forward pass, called once on the
    ``n <= max_batch`` unmasked images and once per chunk of ``max_batch`` masked ones (the chunk plan of
    ``rn_occlusion_u8_device``).  Returns ``(maps [n, S, S] or None, drops [n, G, G], ids [n], probs [n, C])``."""
    ims = np.ascontiguousarray(ims, dtype=np.uint8)
    if ims.ndim != 4 or ims.shape[1] != ims.shape[2] or ims.shape[3] != 3:
        raise ValueError("occlusion: expected an [n,S,S,3] uint8 batch, got %s" % (ims.shape,))
    n, S = ims.shape[0], ims.shape[1]
    G = grid(S, patch, stride)
    if not 1 <= n <= max_batch:
        raise ValueError("occlusion: n = %d out of range (1..%d)" % (n, max_batch))
    if n * G * G > MAX_WINDOWS:
        raise ValueError("occlusion: %d x %d x %d masked passes, more than %d" % (n, G, G, MAX_WINDOWS))
    probs = np.asarray(forward(ims), np.float32)
    ids = probs.argmax(1).astype(np.int64)
    cls = ids if class_ids is None else np.broadcast_to(np.asarray(class_ids, np.int64), (n,))
    if ((cls < 0) | (cls >= probs.shape[1])).any():
        raise ValueError("occlusion: class_ids outside [0, %d)" % probs.shape[1])
    pos = positions(S, patch, stride)
    fills = [_fill_of(im, fill) for im in ims]
    drops = np.empty((n * G * G,), np.float32)
    for first, count in chunks(n * G * G, max_batch):
        batch = np.empty((count, S, S, 3), np.uint8)
        for e in range(count):
            i, w = divmod(first + e, G * G)
            batch[e] = masked(ims[i], pos[w // G], pos[w % G], patch, fills[i])
        pw = np.asarray(forward(batch), np.float32)
        for e in range(count):
            i = (first + e) // (G * G)
            drops[first + e] = probs[i, cls[i]] - pw[e, cls[i]]
    drops = drops.reshape(n, G, G)
    return (pixel_map(drops, S, patch, stride) if with_map else None), drops, ids, probs
