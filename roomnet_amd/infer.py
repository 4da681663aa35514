"""Drop-in for the reference's inference driver ``infer.py`` (``infer.py:1-110``):
``CLASS_LABELS``, the module constants, ``force_makedir``, ``read_fpaths``,
``groundtruth_validation``, ``classify_im_dir`` and the ``__main__`` block, running on the
MI355X ``RoomNet`` of this package instead of TensorFlow.

``classify_im_dir(nn, imgs_dir, overlay=True)`` keeps the reference's observable behaviour:
one ``<imgs_dir>_classified/<label>/`` directory per class, each image written there with
the two overlay lines (or copied when ``overlay=False``), one printed line per image, and a
``<imgs_dir>_classified_results.xls`` workbook (sheet ``classification_results``, header
``IMAGE_NAME | PREDICTED_LABEL``, rows ``name | label | str(conf)``); it returns the
workbook path.  The reference classifies strictly one image per ``sess.run``; here decoded
images are grouped into batches for the GPU (``batch_size``), which does not change any
result because the graph has no cross-image coupling (inference-mode BN).
"""
from __future__ import annotations

import contextlib
from glob import glob
import os
import shutil
import sys

import numpy as np

from . import xls
from .imageio import imread, imwrite, put_text
from .imageops import resize_linear_u8
from .network import RoomNet

CLASS_LABELS = ['Backyard', 'Bathroom', 'Bedroom', 'Frontyard', 'Kitchen', 'LivingRoom']

INPUT_MODEL_PATH = './final_model/roomnet'
INPUT_IMAGES_DIR = './test_images/set2/images'
IMG_SIDE = 224

INPUT_IMG_PATH_LIST_FILE = 'val_list.txt'


def read_fpaths(list_fpath):
    """infer.py:31-38."""
    with open(list_fpath, 'r') as f:
        data = f.readlines()
    fpath_components = [fpath_set.strip().split(' ') for fpath_set in data]
    im_paths = [' '.join(fpath_component[:-1]) for fpath_component in fpath_components]
    class_id = [int(fpath_component[-1]) for fpath_component in fpath_components]
    n = len(class_id)
    return im_paths, class_id, n


def _prepare(nn, im):
    """The host half of ``RoomNet.infer_optimized`` (network.py:149-152); used for images the device pipeline does
    not take (anything but 3-channel uint8) and for model objects without ``infer_images``."""
    im = nn.center_crop(im)
    h, w, _ = im.shape
    if h != nn.im_side or w != nn.im_side:
        im = resize_linear_u8(np.ascontiguousarray(im), nn.im_side, nn.im_side)
    return np.ascontiguousarray(im)


def _classify(nn, ims):
    """``(ids, probs-or-None)`` for a list of decoded BGR images of any size.  ``RoomNet.infer_images`` hands the raw
    images to the GPU, which crops and resizes them (``rn_classify_images_u8``: byte for byte the host restatement of
    ``cv2.resize``); other model objects get the host-prepared batch through ``infer`` like the reference's caller."""
    if hasattr(nn, 'infer_images'):
        outs = nn.infer_images(ims)
    else:
        outs = nn.infer(np.stack([_prepare(nn, im) for im in ims], 0))
    return outs if isinstance(outs, tuple) else (outs, None)


class _Closer:
    def __init__(self, fn):
        self.close = fn


def _usable_cores():
    try:
        return len(os.sched_getaffinity(0))          # the cores THIS process may run on (cgroup / taskset aware)
    except (AttributeError, OSError):
        return os.cpu_count() or 1


# Pillow releases the GIL inside the decoder and imread's channel swap does too; past 16-32 threads the pool levels off on the
# page faults of its fresh 6-8 MB buffers (tools/bench_images.py --threads and tools/bench_decode.py sweep it: 16 is the optimum for
# VGA files, 32 is 13 % better for 1080p; DESIGN.md section 5 has the figures of the GPU box's 256-thread host).
DECODE_THREADS = max(1, min(16, _usable_cores()))


def _progress(n):
    """The reference walks its file list under ``tqdm(range(num_fpaths))`` (infer.py:46, :79): a progress bar on stderr.  Same here
    when tqdm is importable and stderr is a terminal or ROOMNET_PROGRESS=1 asks for it; returns an ``update(k)`` callable and a
    ``close()``."""
    try:
        from tqdm import tqdm
    except ImportError:
        return (lambda k=1: None), (lambda: None)
    want = os.environ.get('ROOMNET_PROGRESS')
    if want == '0' or (want is None and not sys.stderr.isatty()):
        return (lambda k=1: None), (lambda: None)
    bar = tqdm(total=n, file=sys.stderr)
    return bar.update, bar.close


def _decode_files(fpaths, batch_size, decode_threads=None):
    """Yield ``(index, fpath, image_bgr or None)`` per file, in list order: decoded on a small thread pool (Pillow releases
    the GIL while it decodes) that runs up to two batches of ``batch_size`` ahead of the consumer."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    nthreads = max(1, int(decode_threads or DECODE_THREADS))
    window = max(2 * batch_size, nthreads)
    todo = iter(enumerate(fpaths))
    inflight = deque()
    tick, done = _progress(len(fpaths))
    with contextlib.closing(_Closer(done)), ThreadPoolExecutor(max_workers=nthreads) as pool:
        def top_up():
            while len(inflight) < window:
                nxt = next(todo, None)
                if nxt is None:
                    return
                inflight.append((nxt[0], nxt[1], pool.submit(imread, nxt[1])))
        top_up()
        while inflight:
            i, fpath, fut = inflight.popleft()
            im = fut.result()
            tick(1)
            top_up()
            yield i, fpath, im


def _infer_files(nn, fpaths, batch_size, decode_threads=None, gpu_decode=False, gpu_huffman=False, gpu_orient=False):
    """Yield ``(index, image_bgr, idx, conf)`` per readable file, in list order.  Files are decoded on a small thread
    pool (Pillow releases the GIL while it decodes) that runs up to two batches ahead of the GPU; the GPU gets the
    decoded images in batches of ``batch_size``.  ``gpu_decode``: ``RoomNet.infer_files`` instead -- baseline JPEG files
    only pass their Huffman stage on the pool and become pixels on the GPU; ``image_bgr`` is then None (the decoded image
    never exists on the host); same ids and confidences.  ``gpu_huffman`` (with ``gpu_decode``): their Huffman stage runs on the GPU
    too and the pool only reads the files.  ``gpu_orient`` (with ``gpu_decode``): files with an EXIF orientation of 2..8 are decoded
    and turned on the GPU too instead of by ``imread``."""
    if gpu_huffman and not gpu_decode:
        raise ValueError("gpu_huffman=True needs gpu_decode=True (it feeds the GPU's pixel stage)")
    if gpu_orient and not gpu_decode:
        raise ValueError("gpu_orient=True needs gpu_decode=True (it is the GPU's pixel stage that turns the image)")
    if gpu_decode:
        # (a model object without the arguments still works while they are off)
        extra = dict(gpu_huffman=True) if gpu_huffman else {}
        if gpu_orient:
            extra["gpu_orient"] = True
        ids, probs, ok = nn.infer_files(fpaths, decode_threads=decode_threads, batch_size=batch_size, **extra)
        for i, fpath in enumerate(fpaths):
            if not ok[i]:
                print(fpath, '---> unreadable image, skipped')
                continue
            yield i, None, int(ids[i]), probs[i][ids[i]]
        return
    pending = []

    def flush():
        if not pending:
            return []
        ids, probs = _classify(nn, [p[1] for p in pending])
        # the confidence stays an np.float32 scalar like infer_outs[1][0][idx] of the reference (infer.py:84): its
        # printed form, round(conf * 100, 2) and str(conf) are float32 results
        res = [(p[0], p[1], int(ids[k]), (probs[k][ids[k]] if probs is not None else np.float32('nan')))
               for k, p in enumerate(pending)]
        pending.clear()
        return res

    for i, fpath, im in _decode_files(fpaths, batch_size, decode_threads):
        if im is None:
            # the reference crashes here (cv2.imread returns None, infer.py:81-82); report and go on
            print(fpath, '---> unreadable image, skipped')
            continue
        pending.append((i, im))
        if len(pending) >= batch_size:
            for r in flush():
                yield r
    for r in flush():
        yield r


def groundtruth_validation(nn, list_fpath=None, batch_size=64, gpu_decode=False, gpu_huffman=False, gpu_orient=False):
    """infer.py:41-57, with the list file it reads made an argument (the reference's global is
    commented out, infer.py:28).  Prints and returns accuracy and per-class precision / recall /
    f-score, computed like ``train.py:146-152``.  ``gpu_decode``: baseline JPEG files are decoded on the GPU
    (``RoomNet.infer_files``); same predictions.  ``gpu_huffman`` (with ``gpu_decode``): their Huffman pass too.  ``gpu_orient``
    (with ``gpu_decode``): so are the files with an EXIF orientation of 2..8; same predictions."""
    if gpu_huffman and not gpu_decode:
        raise ValueError("groundtruth_validation: gpu_huffman=True needs gpu_decode=True (it feeds the GPU's pixel stage)")
    if gpu_orient and not gpu_decode:
        raise ValueError("groundtruth_validation: gpu_orient=True needs gpu_decode=True (it is the GPU's pixel stage that turns the image)")
    from sklearn.metrics import accuracy_score, precision_recall_fscore_support
    fpaths, labels, num_fpaths = read_fpaths(list_fpath or INPUT_IMG_PATH_LIST_FILE)
    print('Inferring Images...')
    y_preds, y_truths = [], []
    for i, _im, idx, _conf in _infer_files(nn, fpaths, batch_size, gpu_decode=gpu_decode, gpu_huffman=gpu_huffman, gpu_orient=gpu_orient):
        y_preds.append(idx)
        y_truths.append(labels[i])
    acc = accuracy_score(y_truths, y_preds)
    prec, rec, fsc, supp = precision_recall_fscore_support(y_truths, y_preds, zero_division=0)
    performance_stats = {'accuracy': float(acc),
                         'precisions': list(map(float, list(prec))),
                         'recalls': list(map(float, list(rec))),
                         'f-scores': list(map(float, list(fsc)))}
    print(performance_stats)
    return performance_stats


def force_makedir(dir):
    """infer.py:60-62."""
    if not os.path.isdir(dir):
        os.makedirs(dir)


def _overlay_lines(h, w, pred_label, pred_conf):
    """infer.py:87-92: the two overlay lines of an ``h x w`` image as ``(text, org, font_scale, color_bgr)``."""
    return [("Predicted Class: " + pred_label, (int(.5 * w), int(.90 * h)), (h / 720.) * .85, (0, 255, 0)),
            ("Confidence: " + str(round(pred_conf * 100, 2)) + " %", (int(.5 * w), int(.95 * h)), (h / 720.) * .85, (255, 0, 0))]


def _overlay_and_write(im, pred_label, pred_conf, out_fpath):
    """infer.py:87-93 for one image: the two overlay lines, then the file."""
    h, w, _ = im.shape
    for text, org, font_scale, color in _overlay_lines(h, w, pred_label, pred_conf):
        put_text(im, text, org, font_scale, color)
    return imwrite(out_fpath, im)


def _in_batches_of_readable(results, batch_size):
    """``RoomNet.classify_files_to_dir``'s results in the order ``_infer_files`` reports on files: an unreadable file at once, the
    readable ones when ``batch_size`` of them have come together -- so the printed lines of both arms are the same sequence."""
    pending = []
    for r in results:
        if r[1] is None:
            yield r
            continue
        pending.append(r)
        if len(pending) >= batch_size:
            yield from pending
            pending.clear()
    yield from pending


def _explain_files(nn, fpaths, batch_size, layer, occlusion=None):
    """``_infer_files`` with the evidence: yields ``(index, image_bgr, idx, conf, cam)``, the grad-CAM map of each file's predicted
    class from ``nn.grad_cam`` on the same batches; ids and confidences are ``_infer_files``'s (the grad-CAM contract).
    ``layer`` "occlusion": the occlusion-sensitivity map from ``nn.occlusion_map(..., **occlusion)`` instead (the same contract)."""
    pending = []

    def flush():
        if not pending:
            return []
        if layer == 'occlusion':
            cams, _drops, ids, probs = nn.occlusion_map([p[1] for p in pending], **(occlusion or {}))
        else:
            cams, ids, probs = nn.grad_cam([p[1] for p in pending], layer=layer)
        res = [(p[0], p[1], int(ids[k]), probs[k][ids[k]], cams[k]) for k, p in enumerate(pending)]
        pending.clear()
        return res

    for i, fpath, im in _decode_files(fpaths, batch_size):
        if im is None:
            print(fpath, '---> unreadable image, skipped')
            continue
        pending.append((i, im))
        if len(pending) >= batch_size:
            yield from flush()
    yield from flush()


def _heat_overlay_and_write(im, cam_map, weight, pred_label, pred_conf, out_fpath):
    """``_overlay_and_write`` on the image with its heat map: the heat is under the text."""
    from .cam import overlay_image
    return _overlay_and_write(overlay_image(im, cam_map, weight), pred_label, pred_conf, out_fpath)


def classify_im_dir(nn, imgs_dir, overlay=True, batch_size=64, gpu_decode=False, gpu_encode=False, heatmap=None, heatmap_weight=0.5,
                    gpu_huffman=False, gpu_huffman_encode=False, gpu_orient=False, occlusion_patch=32, occlusion_stride=16):
    """infer.py:65-100.  The overlay and the encoding of the output file (the reference does both between two ``sess.run`` calls)
    run on a second thread pool behind the loop -- per 1920 x 1080 image they cost what decoding it cost -- and the function
    returns when every file is written; printed lines, workbook rows and file names are the loop's, in list order.
    ``gpu_decode`` (with ``overlay=False``, or with ``gpu_encode``): baseline JPEG files are decoded on the GPU
    (``RoomNet.infer_files``); the workbook is the same, byte for byte.  ``gpu_encode`` (with ``overlay=True`` and ``gpu_decode``):
    the overlay is drawn and the output JPEG's pixel stage runs on the GPU as well (``RoomNet.classify_files_to_dir``): a file
    stays on the device from decode to encode and only the Huffman passes run on the host; files ``imread`` decodes are uploaded
    when their output is a JPEG file and go the host way otherwise.  Output files, workbook and printed lines are the same,
    byte for byte.  ``gpu_huffman`` (with ``gpu_decode``): the Huffman pass of the input files runs on the GPU too (DESIGN.md
    section 18; with ``gpu_encode`` the input's Huffman pass stays on the host); same outputs.  ``gpu_huffman_encode`` (with
    ``gpu_encode``): the Huffman pass of the OUTPUT files runs on the GPU too: only the files' bytes come
    back and the writer pool only writes them; same outputs.  ``gpu_orient`` (with ``gpu_decode``): files with an EXIF orientation of
    2..8 -- portrait phone photos -- are decoded and turned on the GPU too instead of by ``imread``; same
    outputs.  ``heatmap`` ("s6.bn", "s7.bn": the grad-CAM map of the predicted class; "occlusion": its occlusion-sensitivity map,
    DESIGN.md section 22, with squares of ``occlusion_patch`` slid by ``occlusion_stride`` and the mean fill) is drawn on the square
    the network saw, under the text: with ``gpu_decode`` and ``gpu_encode`` on the device (``Engine.occlusion_resident`` /
    ``explain_resident``, then ``cam_overlay_batch``), otherwise per batch by ``RoomNet.occlusion_map`` / ``grad_cam`` and
    ``cam.overlay_image`` on the writer pool; same outputs."""
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    if gpu_huffman and not gpu_decode:
        raise ValueError("classify_im_dir: gpu_huffman=True needs gpu_decode=True (it feeds the GPU's pixel stage)")
    if gpu_orient and not gpu_decode:
        raise ValueError("classify_im_dir: gpu_orient=True needs gpu_decode=True (it is the GPU's pixel stage that turns the image)")
    if gpu_encode and not overlay:
        raise ValueError("classify_im_dir: gpu_encode=True needs overlay=True (without the overlay the files are copied: there is "
                         "nothing to encode)")
    if gpu_encode and not gpu_decode:
        raise ValueError("classify_im_dir: gpu_encode=True needs gpu_decode=True (it encodes the image the GPU decode left on the device)")
    if gpu_huffman_encode and not gpu_encode:
        raise ValueError("classify_im_dir: gpu_huffman_encode=True needs gpu_encode=True (it encodes the coefficients the GPU encode "
                         "left on the device)")
    if gpu_decode and overlay and not gpu_encode:
        raise ValueError("classify_im_dir: gpu_decode=True needs overlay=False (the overlay is drawn on the decoded image, "
                         "which the GPU decode path never brings to the host) or gpu_encode=True")
    if heatmap is not None and not overlay:
        raise ValueError("classify_im_dir: heatmap=%r needs overlay=True (without the overlay the files are copied: there is "
                         "nothing to draw on)" % (heatmap,))
    if heatmap is not None and heatmap not in ('s6.bn', 's7.bn', 'occlusion'):
        raise ValueError("classify_im_dir: heatmap must be None, 's6.bn', 's7.bn' or 'occlusion', got %r" % (heatmap,))
    if heatmap == 'occlusion' and not 1 <= occlusion_stride <= occlusion_patch:
        raise ValueError("classify_im_dir: 1 <= occlusion_stride <= occlusion_patch does not hold for stride %r, patch %r"
                         % (occlusion_stride, occlusion_patch))
    if heatmap is not None and not 0.0 <= heatmap_weight <= 1.0:
        raise ValueError("classify_im_dir: heatmap_weight must be in [0, 1], got %r" % (heatmap_weight,))
    print('Classifying images in', imgs_dir)
    all_im_paths = glob(imgs_dir + '/*')
    out_dir = imgs_dir + '_classified'
    xl_fpath = out_dir + '_results.xls'
    class_dirs = [out_dir + os.sep + CLASS_LABELS[i] for i in range(len(CLASS_LABELS))]
    for dir in class_dirs:
        force_makedir(dir)
    print('Beginning inference..')
    excel_file = xls.Workbook()
    sheet = excel_file.add_sheet('classification_results')
    sheet.write(0, 0, 'IMAGE_NAME')
    sheet.write(0, 1, 'PREDICTED_LABEL')
    row = 0      # unreadable files are skipped (the reference crashes on them): rows stay contiguous
    writers = ThreadPoolExecutor(max_workers=DECODE_THREADS) if overlay else None
    writing = deque()
    extra = {} if heatmap is None else dict(heatmap=heatmap, heatmap_weight=heatmap_weight)      # (a model object without the arguments still works without a heat map)
    occlusion = None
    if heatmap == 'occlusion':
        occlusion = dict(patch=occlusion_patch, stride=occlusion_stride)
        extra.update(occlusion_patch=occlusion_patch, occlusion_stride=occlusion_stride)
    if gpu_huffman_encode:
        extra["gpu_huffman_encode"] = True
    if gpu_orient and gpu_encode:
        extra["gpu_orient"] = True
    if gpu_encode:
        results = _in_batches_of_readable(
            nn.classify_files_to_dir(all_im_paths,
                                     lambda i, idx: out_dir + os.sep + CLASS_LABELS[idx] + os.sep + all_im_paths[i].split(os.sep)[-1],
                                     lambda h, w, idx, conf: _overlay_lines(h, w, CLASS_LABELS[idx], conf),
                                     writers, batch_size=batch_size, **extra), batch_size)
    elif heatmap is not None:
        results = ((i, idx, conf, (im, cam_map), None) for i, im, idx, conf, cam_map in _explain_files(nn, all_im_paths, batch_size, heatmap, occlusion))
    else:
        results = ((i, idx, conf, im, None) for i, im, idx, conf in
                   _infer_files(nn, all_im_paths, batch_size, gpu_decode=gpu_decode, gpu_huffman=gpu_huffman, gpu_orient=gpu_orient))
    try:
        for i, idx, pred_conf, im, written in results:
            fpath = all_im_paths[i]
            if idx is None:
                print(fpath, '---> unreadable image, skipped')
                continue
            row += 1
            pred_label = CLASS_LABELS[idx]
            out_fpath_dir = out_dir + os.sep + pred_label
            print(fpath, '--->', pred_label, pred_conf)
            if written is not None:
                writing.append(written)
            elif overlay:
                draw = (_heat_overlay_and_write, im[0], im[1], heatmap_weight) if isinstance(im, tuple) else (_overlay_and_write, im)
                writing.append(writers.submit(*draw, pred_label, pred_conf, out_fpath_dir + os.sep + fpath.split(os.sep)[-1]))
                while len(writing) > 4 * DECODE_THREADS:      # (a bound on the decoded images held for the writers)
                    writing.popleft().result()
            else:
                shutil.copy(fpath, out_fpath_dir)
            sheet.write(row, 0, fpath.split(os.sep)[-1])
            sheet.write(row, 1, pred_label)
            sheet.write(row, 2, str(pred_conf))
        while writing:
            writing.popleft().result()
    finally:
        if writers is not None:
            writers.shutdown(wait=True)
    excel_file.save(xl_fpath)
    return xl_fpath


def compare_heatmaps(nn, im_paths_or_dir, methods=('s6.bn', 's7.bn', 'occlusion'), steps=32, batch_size=64, **occlusion_kw):
    """Which heat map to believe on these photographs (not in the reference): per method the mean deletion area and the mean
    insertion area over the files (``RoomNet.map_faithfulness``, DESIGN.md section 23: a map that points at the evidence has a
    SMALL deletion area and a LARGE insertion area).  ``im_paths_or_dir``: a directory or a list of image files; ``methods``:
    "s6.bn" / "s7.bn" (``grad_cam`` at that layer) and "occlusion" (``occlusion_map(**occlusion_kw)``: patch, stride, fill), each for
    the predicted class with the mean fill; ``steps`` points per curve.  Prints one line per method and returns
    ``{method: {"deletion": area, "insertion": area, "images": count}}``.  A report on host arrays, not a loop anyone waits on."""
    methods = tuple(methods)
    for m in methods:
        if m not in ('s6.bn', 's7.bn', 'occlusion'):
            raise ValueError("compare_heatmaps: methods are 's6.bn', 's7.bn' and 'occlusion', got %r" % (m,))
    if not methods:
        raise ValueError("compare_heatmaps: no methods")
    paths = sorted(glob(im_paths_or_dir + '/*')) if isinstance(im_paths_or_dir, str) else list(im_paths_or_dir)
    batch_size = max(1, min(int(batch_size), nn.max_batch))
    sums = {m: np.zeros(2, np.float64) for m in methods}
    count = 0

    def flush(pending):
        batch = np.asarray(nn._batch_from(pending, "compare_heatmaps"))
        for m in methods:
            if m == 'occlusion':
                maps = nn.occlusion_map(batch, **occlusion_kw)[0]
            else:
                maps = nn.grad_cam(batch, layer=m)[0]
            _curves, aucs, _ids, _probs = nn.map_faithfulness(batch, maps, steps=steps)
            sums[m] += aucs.astype(np.float64).sum(0)
        return len(pending)

    pending = []
    for _i, fpath, im in _decode_files(paths, batch_size):
        if im is None:
            print(fpath, '---> unreadable image, skipped')
            continue
        pending.append(im)
        if len(pending) >= batch_size:
            count += flush(pending)
            pending = []
    if pending:
        count += flush(pending)
    if not count:
        raise ValueError("compare_heatmaps: no readable image")
    report = {}
    for m in methods:
        report[m] = {'deletion': float(sums[m][0] / count), 'insertion': float(sums[m][1] / count), 'images': count}
        print('%-10s deletion area %.4f   insertion area %.4f   (%d images, %d steps)' % (m, report[m]['deletion'], report[m]['insertion'],
                                                                                        count, steps))
    return report


def recalibrate_from_dir(nn, imgs_dir, batch_size=64, momentum=None, gpu_decode=False, gpu_orient=False):
    """Re-estimate the model's BN statistics on the images of a directory (``RoomNet.recalibrate_bn``; not in the reference,
    whose statistics only move while it trains, network.py:64-67): the files are decoded as ``classify_im_dir`` decodes them
    and fed in batches of ``batch_size`` (at most the model's ``max_batch``; a last batch of ONE image is dropped: its variance is 0).
    ``momentum=None``: the statistics become the average over the batches.  Returns the new statistics.  ``gpu_decode``: baseline
    JPEG files are decoded, cropped and resized on the GPU (``RoomNet.prepare_files``); the batches are the same bytes.
    ``gpu_orient`` (with ``gpu_decode``): so are the files with an EXIF orientation of 2..8."""
    if gpu_orient and not gpu_decode:
        raise ValueError("recalibrate_from_dir: gpu_orient=True needs gpu_decode=True (it is the GPU's pixel stage that turns the image)")
    all_im_paths = sorted(glob(imgs_dir + '/*'))
    orient = dict(gpu_orient=True) if gpu_orient else {}      # (a model object without the argument still works while it is off)

    def gpu_batches():
        pending = np.zeros((0, nn.im_side, nn.im_side, 3), np.uint8)
        for _at, batch, bad in nn.prepare_files(all_im_paths, batch_size=batch_size, **orient):
            for i in bad:
                print(all_im_paths[i], '---> unreadable image, skipped')
            pending = np.concatenate([pending, batch], 0)
            while len(pending) >= batch_size:
                yield pending[:batch_size]
                pending = pending[batch_size:]
        if len(pending) > 1:
            yield pending

    def batches():
        pending = []
        for _i, fpath, im in _decode_files(all_im_paths, batch_size):
            if im is None:
                print(fpath, '---> unreadable image, skipped')
                continue
            pending.append(im)
            if len(pending) >= batch_size:
                yield pending
                pending = []
        if len(pending) > 1:
            yield pending

    return nn.recalibrate_bn(gpu_batches() if gpu_decode else batches(), momentum=momentum)


def fine_tune_from_list(nn, list_fpath, steps, batch_size=45, seed=0, val_list_fpath=None, extract_batch=64, depth=2,
                        gpu_decode=False, dropout_rate=None, val_every=None, keep="last", stats_fpath=None, gpu_orient=False,
                        views=False, random_crop=True, flip=True):
    """``RoomNet.fine_tune`` on the images of a list file in the reference's ``path label`` format (``train_list.txt``, read as
    infer.py:31-38 reads it): the files are decoded as ``classify_im_dir`` decodes them, their features are extracted batch by
    batch (``RoomNet.extract_features``; unreadable files are reported and skipped), then the model is trained on the cached
    features.  ``val_list_fpath``: a second list evaluated after the last step.  ``depth=3`` trains the whole last conv block on
    cached ``s6.bn`` (1.08 MB per image at 224, against 28 KB at depth 2).  Returns what ``fine_tune`` returns.  ``gpu_decode``:
    the feature extraction decodes baseline JPEG files on the GPU (``RoomNet.prepare_files``); same features.  ``gpu_orient`` (with
    ``gpu_decode``): also the files with an EXIF orientation of 2..8; same features.
    ``dropout_rate``: passed to ``fine_tune`` (dropout at every site at or behind the cached feature).
    ``val_every``, ``keep``: passed to ``fine_tune`` (validation on the GPU every ``val_every`` steps; ``keep="best"`` keeps the best
    point's variables).  ``stats_fpath``: every point's ``step``, ``accuracy``, ``precisions``, ``recalls`` and ``f-scores`` are
    appended to that JSON file as train.py:129-155 keeps ``all_train_stats.json`` (``metrics.append_stats``), so the reference's
    ``plotter.py`` reads it as it is; needs ``val_every``.
    ``views=True``: the reference's training regime (train.py:117-118) -- the training list is decoded on the pool and kept
    resident on the GPU as whole photographs, and every step trains on fresh random views of them (``RoomNet.fine_tune_views``;
    ``random_crop``, ``flip``: its arguments); the validation list still goes through the cached centre-crop features.  Not together
    with ``gpu_decode``: keeping the GPU decoder's output resident is a later step (``ValueError``)."""
    if views and gpu_decode:
        raise ValueError("fine_tune_from_list: views=True keeps host-decoded photographs resident and does not take gpu_decode=True "
                         "yet (keeping the GPU decoder's output resident is a later step)")
    if stats_fpath is not None and val_every is None:
        raise ValueError("fine_tune_from_list: stats_fpath records validation points: pass val_every= (and val_list_fpath=)")
    if gpu_orient and not gpu_decode:
        raise ValueError("fine_tune_from_list: gpu_orient=True needs gpu_decode=True (it is the GPU's pixel stage that turns the image)")
    orient = dict(gpu_orient=True) if gpu_orient else {}      # (a model object without the argument still works while it is off)
    def features_of(path):
        fpaths, labels, _n = read_fpaths(path)
        feats, kept, pending = [], [], []
        if gpu_decode:
            for at, batch, bad in nn.prepare_files(fpaths, batch_size=extract_batch, **orient):
                for i in bad:
                    print(fpaths[i], '---> unreadable image, skipped')
                if at:
                    feats.append(nn.extract_features(batch, depth=depth))
                    kept.extend(labels[i] for i in at)
            if not feats:
                raise ValueError("fine_tune_from_list: no readable image in %r" % path)
            return np.concatenate(feats, 0), np.asarray(kept, np.int32)

        def flush():
            if pending:
                feats.append(nn.extract_features([p[1] for p in pending], depth=depth))
                kept.extend(labels[p[0]] for p in pending)
                pending.clear()

        for i, fpath, im in _decode_files(fpaths, extract_batch):
            if im is None:
                print(fpath, '---> unreadable image, skipped')
                continue
            pending.append((i, im))
            if len(pending) >= extract_batch:
                flush()
        flush()
        if not feats:
            raise ValueError("fine_tune_from_list: no readable image in %r" % path)
        return np.concatenate(feats, 0), np.asarray(kept, np.int32)

    def photographs_of(path):
        fpaths, labels, _n = read_fpaths(path)
        ims, kept = [], []
        for i, fpath, im in _decode_files(fpaths, extract_batch):
            if im is None or im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                print(fpath, '---> unreadable image, skipped')
                continue
            ims.append(im)
            kept.append(labels[i])
        if not ims:
            raise ValueError("fine_tune_from_list: no readable image in %r" % path)
        return ims, np.asarray(kept, np.int32)

    if views:
        ims, labels = photographs_of(list_fpath)
        val = features_of(val_list_fpath) if val_list_fpath else None
        out = nn.fine_tune_views(ims, labels, steps, batch_size=batch_size, seed=seed, depth=depth, random_crop=random_crop, flip=flip,
                                 val=val, val_every=val_every, keep=keep, dropout_rate=dropout_rate)
    else:
        feats, labels = features_of(list_fpath)
        val = features_of(val_list_fpath) if val_list_fpath else None
        out = nn.fine_tune(feats, labels, steps, batch_size=batch_size, seed=seed, val=val, depth=depth, dropout_rate=dropout_rate,
                           val_every=val_every, keep=keep)
    if stats_fpath is not None:
        from . import metrics
        metrics.append_stats(stats_fpath, out["val_history"])
    return out


if __name__ == '__main__':
    nn = RoomNet(num_classes=len(CLASS_LABELS), im_side=IMG_SIDE, compute_bn_mean_var=False,
                 optimized_inference=True)
    nn.load(INPUT_MODEL_PATH)

    # stats = groundtruth_validation(nn)
    xl_out_path = classify_im_dir(nn, INPUT_IMAGES_DIR)
