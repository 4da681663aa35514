"""Host helpers for grad-CAM maps (``RoomNet.grad_cam``): bilinear upsampling to the crop and a colour overlay.

NumPy only (no cv2), deterministic: the same map and image give the same bytes on every machine.
"""
from __future__ import annotations

import numpy as np

# a fixed blue -> cyan -> green -> yellow -> red ramp (the usual "jet"-like look), as BGR anchors at 0, 1/4, ... 1
_ANCHORS_BGR = np.array([[128, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255]], np.float64)


def upsample(cam: np.ndarray, side: int) -> np.ndarray:
    """One map ``[h, w]`` (or a batch ``[n, h, w]``) -> bilinear (pixel-centre aligned) ``[side, side]`` float32, then
    normalised to [0, 1] per map (an all-zero map stays zero)."""
    cam = np.asarray(cam, np.float64)
    batch = cam.ndim == 3
    if not batch:
        cam = cam[None]
    if cam.ndim != 3:
        raise ValueError("expected a [h, w] or [n, h, w] map, got %s" % (cam.shape,))
    n, h, w = cam.shape

    def axis(n_in):
        src = (np.arange(side, dtype=np.float64) + 0.5) * (n_in / float(side)) - 0.5
        src = np.clip(src, 0.0, n_in - 1)
        lo = np.floor(src).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, src - lo

    ylo, yhi, yl = axis(h)
    xlo, xhi, xl = axis(w)
    top = cam[:, ylo][:, :, xlo] * (1 - xl) + cam[:, ylo][:, :, xhi] * xl
    bot = cam[:, yhi][:, :, xlo] * (1 - xl) + cam[:, yhi][:, :, xhi] * xl
    up = top * (1 - yl)[None, :, None] + bot * yl[None, :, None]
    up = np.maximum(up, 0.0)
    mx = up.reshape(n, -1).max(axis=1)
    up = np.where(mx[:, None, None] > 0, up / np.where(mx > 0, mx, 1.0)[:, None, None], 0.0).astype(np.float32)
    return up if batch else up[0]


def colormap(v: np.ndarray) -> np.ndarray:
    """Values in [0, 1] -> BGR uint8 through the fixed ramp."""
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0) * (len(_ANCHORS_BGR) - 1)
    i = np.minimum(np.floor(v).astype(np.int64), len(_ANCHORS_BGR) - 2)
    t = (v - i)[..., None]
    rgb = _ANCHORS_BGR[i] * (1 - t) + _ANCHORS_BGR[i + 1] * t
    return np.rint(rgb).astype(np.uint8)


def overlay(im_bgr_u8: np.ndarray, cam: np.ndarray, weight: float = 0.5) -> np.ndarray:
    """Blend the colour-mapped ``cam`` (any resolution; upsampled and normalised to the image) into ``im_bgr_u8``
    ``[S, S, 3]`` (the crop the network saw): ``(1 - weight) * image + weight * colour``, rounded, BGR uint8."""
    im = np.asarray(im_bgr_u8)
    if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] != im.shape[1]:
        raise ValueError("expected a square [S, S, 3] BGR image, got %s" % (im.shape,))
    if not 0.0 <= weight <= 1.0:
        raise ValueError("weight must be in [0, 1]")
    heat = colormap(upsample(cam, im.shape[0]))
    out = (1.0 - weight) * im.astype(np.float64) + weight * heat.astype(np.float64)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def crop_window(h: int, w: int):
    """``(y0, x0, side)`` of the centred square ``RoomNet.center_crop`` cuts from an ``h x w`` image: side ``min(h, w)``, offset
    ``abs((w - h) // 2)`` along the longer axis (Python's floor division: a portrait image with an odd difference rounds UP)."""
    offset = abs((w - h) // 2)
    return (0, offset, h) if h < w else (offset, 0, w)


def overlay_image(im_bgr_u8: np.ndarray, cam: np.ndarray, weight: float = 0.5) -> np.ndarray:
    """``overlay`` for a whole photograph ``[h, w, 3]`` of any shape: the heat goes on the square the network saw
    (``crop_window``), the rest of the image is untouched.  Returns a new BGR uint8 image.  The definition of what
    ``rn_cam_overlay_batch_device`` draws on the GPU, byte for byte."""
    im = np.asarray(im_bgr_u8)
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError("expected a [h, w, 3] BGR uint8 image, got %s %s" % (im.dtype, im.shape))
    y0, x0, c = crop_window(im.shape[0], im.shape[1])
    out = im.copy()
    out[y0:y0 + c, x0:x0 + c] = overlay(im[y0:y0 + c, x0:x0 + c], cam, weight)
    return out
