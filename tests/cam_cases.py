"""The image set of the heat-map tests (test_cam_overlay_host.py, test_hip_cam_overlay.py): the smallest images at which each
rule of ``cam.overlay_image`` can go wrong, and a restatement of it whose rules can be swapped one at a time, to show that a
kernel that got one wrong would change bytes of THIS set."""
import numpy as np

from jpeg_cases import content

# square; landscape, odd widths, window rows that start at every byte offset, more than one workgroup (72 and up: more than 64
# window columns, 240: more than one row of workgroups of the maximum); portrait with an odd difference (the offset rounds up);
# two columns (a row shorter than one group of 4 pixels); a single pixel
SHAPES = [(16, 16), (8, 24), (37, 53), (17, 33), (72, 96), (120, 200), (240, 320), (53, 36), (41, 24), (50, 49), (31, 2), (1, 1)]
MAP_SIDES = (46, 21)          # s6.bn and s7.bn at 224
WEIGHTS = (0.5, 0.3, 0.0, 1.0)
ZERO_MAP, HOT_PIXEL = 3, 8    # the images that get an all-zero map and a map with a single hot entry
SEED = 0                      # (test_cam_overlay_host.py asserts that every mutant shows on the set these seeds give)


def images():
    """BGR images of SHAPES, noise and smooth content alternating; never modified."""
    ims = [np.ascontiguousarray(content(h, w, ["noise", "smooth"][k % 2], seed=k)[:, :, ::-1]) for k, (h, w) in enumerate(SHAPES)]
    for im in ims:
        im.setflags(write=False)
    return ims


def maps(turn):
    """One float32 map per image for the ``turn``-th weight: the two map sizes alternate over the images and swap from turn to
    turn; rectified noise (about half the entries 0, as a real map's), one all-zero map, one with a single hot entry."""
    out = []
    for k in range(len(SHAPES)):
        m = MAP_SIDES[(k + turn) % 2]
        rng = np.random.default_rng(SEED + 7919 * turn + 101 * k)
        cam = np.maximum(rng.standard_normal((m, m)), 0).astype(np.float32)
        if k == ZERO_MAP:
            cam[:] = 0
        elif k == HOT_PIXEL:
            cam[:] = 0
            cam[m // 3, m - 2] = 2.5
        out.append(cam)
    return out


_ANCHORS = np.array([[128, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255]], np.float64)


def restated(im, cam, weight, half_up=False, symmetric_offset=False, own_max=False, upsample_dtype=np.float64):
    """``cam.overlay_image`` written out once more, step by step as include/roomnet_hip.h lists them; each keyword swaps one rule
    for the mistake a kernel could make there."""
    h, w = im.shape[:2]
    c = min(h, w)
    offset = abs(w - h) // 2 if symmetric_offset else abs((w - h) // 2)
    y0, x0 = (0, offset) if h < w else (offset, 0)
    rnd = (lambda a: np.floor(a + 0.5)) if half_up else np.rint
    ft = upsample_dtype
    cam = np.asarray(cam, ft)

    def axis(n_in):
        src = (np.arange(c, dtype=ft) + ft(0.5)) * ft(ft(n_in) / ft(c)) - ft(0.5)
        src = np.clip(src, ft(0), ft(n_in - 1))
        lo = np.floor(src).astype(np.int64)
        return lo, np.minimum(lo + 1, n_in - 1), src - lo.astype(ft)

    ylo, yhi, yl = axis(cam.shape[0])
    xlo, xhi, xl = axis(cam.shape[1])
    top = cam[ylo][:, xlo] * (1 - xl) + cam[ylo][:, xhi] * xl
    bot = cam[yhi][:, xlo] * (1 - xl) + cam[yhi][:, xhi] * xl
    up = np.maximum(top * (1 - yl)[:, None] + bot * yl[:, None], 0).astype(np.float64)
    mx = float(max(cam.max(), 0)) if own_max else up.max()
    v = (up / mx if mx > 0 else np.zeros_like(up)).astype(np.float32)
    v64 = np.clip(v.astype(np.float64), 0, 1) * 4
    i = np.minimum(np.floor(v64).astype(np.int64), 3)
    t = (v64 - i)[..., None]
    heat = rnd(_ANCHORS[i] * (1 - t) + _ANCHORS[i + 1] * t)
    out = im.copy()
    win = im[y0:y0 + c, x0:x0 + c].astype(np.float64)
    out[y0:y0 + c, x0:x0 + c] = np.clip(rnd((1.0 - weight) * win + weight * heat), 0, 255).astype(np.uint8)
    return out
