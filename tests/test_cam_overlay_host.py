"""``cam.overlay_image`` (the host statement of rn_cam_overlay_batch_device) against its definition, and the evidence that the GPU
test's image set (cam_cases.py) would show a kernel that got a rule wrong.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import cam_cases
from roomnet_amd import cam


@pytest.fixture(scope="module")
def images():
    return cam_cases.images()


def window(h, w):
    c = min(h, w)
    off = abs((w - h) // 2)
    return (0, off, c) if h < w else (off, 0, c)


def test_window_and_untouched_outside(images):
    assert window(41, 24) == (9, 0, 24) and window(53, 36) == (9, 0, 36) and window(50, 49) == (1, 0, 49) and window(31, 2) == (15, 0, 2)
    assert window(8, 24) == (0, 8, 8) and window(37, 53) == (0, 8, 37)
    for turn, weight in enumerate(cam_cases.WEIGHTS):
        for im, m in zip(images, cam_cases.maps(turn)):
            h, w = im.shape[:2]
            y0, x0, c = window(h, w)
            assert cam.crop_window(h, w) == (y0, x0, c)
            got = cam.overlay_image(im, m, weight)
            assert got.dtype == np.uint8 and got.shape == im.shape
            inside = np.zeros((h, w), bool)
            inside[y0:y0 + c, x0:x0 + c] = True
            np.testing.assert_array_equal(got[~inside], im[~inside])
            np.testing.assert_array_equal(got[inside].reshape(c, c, 3), cam.overlay(im[y0:y0 + c, x0:x0 + c], m, weight))
            np.testing.assert_array_equal(got, cam_cases.restated(im, m, weight), err_msg="%s at %s" % (im.shape, weight))
            if weight == 0.0:
                np.testing.assert_array_equal(got, im)


def test_square_equals_overlay_and_input_is_not_modified(images):
    im = images[0]
    keep = im.copy()
    m = cam_cases.maps(0)[0]
    np.testing.assert_array_equal(cam.overlay_image(im, m, 0.3), cam.overlay(im, m, 0.3))
    np.testing.assert_array_equal(im, keep)
    with pytest.raises(ValueError):
        cam.overlay_image(im, m, 1.5)
    with pytest.raises(ValueError):
        cam.overlay_image(im[:, :, 0], m)


def test_zero_negative_and_single_hot_maps(images):
    im = images[2]                                   # 37 x 53
    y0, x0, c = window(*im.shape[:2])
    first = np.array([128, 0, 0], np.float64)      # an all-zero map paints the ramp's first anchor
    got = cam.overlay_image(im, np.zeros((21, 21), np.float32), 0.3)
    want = np.clip(np.rint(0.7 * im[y0:y0 + c, x0:x0 + c].astype(np.float64) + 0.3 * first), 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(got[y0:y0 + c, x0:x0 + c], want)
    # a map without a positive entry is the all-zero map; negative entries next to positive ones only pull their neighbours down
    neg = -np.abs(np.random.default_rng(1).standard_normal((21, 21))).astype(np.float32)
    np.testing.assert_array_equal(cam.overlay_image(im, neg, 0.3), got)
    mixed = neg.copy()
    mixed[5, 7] = 3.0
    out = cam.overlay_image(im, mixed, 1.0)
    np.testing.assert_array_equal(out, cam_cases.restated(im, mixed, 1.0))
    assert (out[y0:y0 + c, x0:x0 + c] == [0, 0, 255]).all(2).sum() >= 1          # the hot entry reaches the ramp's last anchor
    assert (out[y0:y0 + c, x0:x0 + c] == [128, 0, 0]).all(2).sum() > c * c // 2   # ... and most of the window stays at the first
    # a single pixel, and a window smaller than the map (the map is sampled down)
    one = cam.overlay_image(images[-1], cam_cases.maps(0)[-1], 1.0)
    assert one.shape == (1, 1, 3)
    np.testing.assert_array_equal(cam.overlay_image(images[1], mixed, 0.5), cam_cases.restated(images[1], mixed, 0.5))


MUTANTS = {"half_up": dict(half_up=True), "symmetric_offset": dict(symmetric_offset=True), "own_max": dict(own_max=True),
           "float32_upsampling": dict(upsample_dtype=np.float32)}


def test_each_wrong_rule_changes_bytes_of_the_gpu_tests_image_set(images):
    """Bytes that differ from cam.overlay_image, per mutant, summed over the set at each weight.  (Weight 0 copies the image and
    shows nothing; at weight 1 the blend has no ties, so rounding shows only in the ramp.)"""
    changed = {name: [0] * len(cam_cases.SHAPES) for name in MUTANTS}
    for turn, weight in enumerate(cam_cases.WEIGHTS):
        for k, (im, m) in enumerate(zip(images, cam_cases.maps(turn))):
            want = cam.overlay_image(im, m, weight)
            for name, kw in MUTANTS.items():
                changed[name][k] += int((cam_cases.restated(im, m, weight, **kw) != want).sum())
    print(changed)
    assert sum(n > 100 for n in changed["half_up"]) >= 8
    portrait = [k for k, (h, w) in enumerate(cam_cases.SHAPES) if h > w and (h - w) % 2]
    assert len(portrait) == 4 and all(changed["symmetric_offset"][k] > 0 for k in portrait)
    assert all(changed["symmetric_offset"][k] == 0 for k in range(len(cam_cases.SHAPES)) if k not in portrait)
    assert sum(n > 100 for n in changed["own_max"]) >= 8 and changed["own_max"][cam_cases.ZERO_MAP] == 0
    # float32 upsampling moves a value across a rounding boundary only here and there: the seeds of cam_cases are chosen so that it does
    assert sum(changed["float32_upsampling"]) >= 1 and max(changed["float32_upsampling"]) < 100


def test_kernel_arithmetic_compiled_for_the_host_equals_overlay_image(images, tmp_path):
    """csrc/rn_cam_math.h -- the text the two kernels run per pixel -- through tools/cam_overlay_main.cpp."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "cam_overlay")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "roomnet_amd", "csrc"),
                           os.path.join(ROOT, "tools", "cam_overlay_main.cpp"), "-o", exe])
    for turn, weight in enumerate(cam_cases.WEIGHTS[:2]):
        for im, m in zip(images, cam_cases.maps(turn)):
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                f.write(struct.pack("<4id", im.shape[0], im.shape[1], m.shape[0], m.shape[1], weight) + im.tobytes() + m.tobytes())
            subprocess.check_call([exe, src, dst])
            got = np.fromfile(dst, np.uint8).reshape(im.shape)
            np.testing.assert_array_equal(got, cam.overlay_image(im, m, weight), err_msg="%s at %s" % (im.shape, weight))


def test_classify_im_dir_refuses_a_heat_map_without_the_overlay(tmp_path):
    from roomnet_amd.infer import classify_im_dir
    for kw in (dict(overlay=False), dict(overlay=False, gpu_decode=True), dict(overlay=True, heatmap="s5.bn"),
               dict(overlay=True, heatmap_weight=1.5)):
        kw.setdefault("heatmap", "s6.bn")
        with pytest.raises(ValueError):
            classify_im_dir(None, str(tmp_path / "nothing"), **kw)
    assert not os.path.exists(str(tmp_path / "nothing_classified"))
