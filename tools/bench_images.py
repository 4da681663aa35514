"""GPU box: images/sec of the caller-side pipeline.

  python tools/bench_images.py [H W [N]]          N decoded images of one size (decode excluded):
        host centre-crop + resize (roomnet_amd.imageops) + rn_forward_u8   vs   rn_classify_images_u8 (crop + resize on the GPU)
  python tools/bench_images.py --dir [--threads=T] [H W [N]]    a generated directory of N JPEG files of that size through
        classify_im_dir(overlay=False) and groundtruth_validation (decode on the thread pool, crop + resize + forward on
        the GPU), next to decode alone and to the one-image-at-a-time loop of the reference's caller (infer.py:79-82)
  python tools/bench_images.py --dir --gpu-decode [--threads=T] [H W [N]]    then, in the same session and on the same files, the
        gpu_decode=True arm of both drivers (baseline JPEG split: Huffman pass on the pool, pixel stage on the GPU), the host
        entropy pass alone on one thread, and the device time of the pixel stage per batch; a second line with the ratios
  python tools/bench_images.py --dir --gpu-encode [--threads=T] [H W [N]]    then classify_im_dir(overlay=True) as it was (host
        decode, host overlay and re-encode on the pool) against overlay=True, gpu_decode=True, gpu_encode=True on the same files,
        alternating, three times each after a warm-up of both; the host Huffman-encode pass alone on one thread and the device time
        of the overlay + encode launches per batch; a line with the rates, the ratio and whether the files are identical
  python tools/bench_images.py --dir --gpu-huffman [--threads=T] [H W [N]]    a generated directory again, nothing of the above: both
        drivers with gpu_decode=True against gpu_decode=True, gpu_huffman=True (the Huffman pass on the GPU too)
        on the same files, alternating, three runs each after a warm-up of both; the ratio, the host's share per file and thread in
        both arms, the device time of the Huffman launches per batch, the synchronisation rounds, the count of host fallbacks
  python tools/bench_images.py --dir --gpu-huffman-encode [--threads=T] [H W [N]]    a generated directory again, nothing of the above:
        classify_im_dir(overlay=True) on the host, the gpu_decode + gpu_encode arm and the same with gpu_huffman_encode=True (the
        Huffman pass of the OUTPUT on the GPU too) on the same files, alternating, three runs each after a
        warm-up of all; the ratios, whether the files are identical, the host Huffman-encode pass alone on one thread, the device
        time of the four phases per batch beside the pixel stage's, the bytes downloaded per batch in both GPU arms, the fallbacks.
        The line that begins "overlay=True" is the --gpu-encode arm's own report from the same runs
  python tools/bench_images.py --dir --gpu-orient [--orientation=K] [--stage-only] [--threads=T] [H W [N]]    generated directories whose
        files carry a spliced EXIF orientation, cycling 1..8 or all K, nothing of the above; at 640x480 and
        1920x1080 unless a size is given: both drivers with gpu_decode=True (turned files fall back to imread: what the option is
        compared with) against gpu_decode=True, gpu_orient=True on the same files, alternating, three runs each after a warm-up
        of both, with the spread of the run times and the ways the files took (RoomNet.last_decode_paths); then the device time of
        the pixel stage (rn_jpeg_last_decode_ms) for one batch of 64 1920x1080 files, all at orientation 1, at 3 and at 6.
        --stage-only: only that last line (run it with ROOMNET_HIP_LIB=<a -DJPEG_TURN_DIRECT variant> for the comparison arm)
  python tools/bench_images.py --heatmap [--threads=T] [H W [N]]    a generated directory again, nothing of the above: the device time
        of the two heat-map launches (rn_cam_last_overlay_ms) for one batch and both layers, next to the decode's and the encode's
        pixel stages of the same batch; then classify_im_dir(overlay=True, gpu_decode=True, gpu_encode=True) with heatmap="s6.bn",
        the same call with heatmap=None and the host arm with the heat map, alternating, twice each after a warm-up round
  python tools/bench_images.py --occlusion [--out=PATH] [--threads=T] [N]    occlusion-sensitivity maps, nothing
        of the above; the lines also go to PATH (default profiles/occlusion_bench.txt).  (a) one rn_occlusion_u8_device call for N
        (default 64) resident images at 224 and the default grid (patch 32, stride 16) against the same number of plain
        rn_forward_u8_device calls with the same chunk sizes on a resident buffer: alternating in one session, three runs each
        after a warm-up of both, enqueue to sync on the host's clock, and the call's own device time (rn_occlusion_last_ms);
        (b) the same call against the Python route, occlusion.occlusion_map_host over nn.infer; (c) classify_im_dir(overlay=True,
        gpu_decode=True, gpu_encode=True) with heatmap="occlusion" against heatmap="s6.bn" on N generated 640x480 and 1920x1080 files
  python tools/bench_images.py --faithfulness [--out=PATH] [N]    deletion / insertion curves of heat maps,
        nothing of the above; the lines also go to PATH (default profiles/faithfulness_bench.txt).  (a) one rn_faith_u8_device call
        for N (default 64) resident images at 224 with 32 steps and both curves against the same number of plain
        rn_forward_u8_device calls with the same chunk sizes on a resident buffer: alternating in one session, three runs each
        after a warm-up of both, enqueue to sync on the host's clock, the call's own device time (rn_faith_last_ms), and the rank
        launch's device time alone (rn_faith_ranks_device); (b) the same call against the Python route, faithfulness.curves_host
        over nn.infer; (c) infer.compare_heatmaps on N generated 640x480 files: the three methods' mean areas
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, '.')
from roomnet_amd import _capi, imageio
from roomnet_amd.graph import build_graph
from roomnet_amd.imageops import resize_linear_u8
from roomnet_amd.tf_bundle import BundleReader

THREADS = None
for _a in sys.argv[1:]:
    if _a.startswith('--threads='):
        THREADS = int(_a.split('=', 1)[1])          # decode threads of the directory drivers (default: infer.DECODE_THREADS)
args = [a for a in sys.argv[1:] if not a.startswith('--')]
H = int(args[0]) if len(args) > 0 else 1080
W = int(args[1]) if len(args) > 1 else 1920
N = int(args[2]) if len(args) > 2 else 64


def crop(x):
    h, w_, _ = x.shape
    off = abs((w_ - h) // 2)
    return x[:, off:off + h, :] if h < w_ else (x[off:off + w_, :, :] if w_ < h else x)


def decoded_images():
    w = BundleReader('roomnet_amd/final_model/roomnet').load_all()
    e = _capi.Engine(build_graph(6, 224), w, dtype='bf16', max_batch=N)
    rng = np.random.default_rng(0)
    ims = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    e.classify_images(ims[:2])
    t0 = time.perf_counter()
    ids_g, p_g = e.classify_images(ims)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    batch = np.stack([resize_linear_u8(crop(im), 224, 224) for im in ims])
    ids_h, p_h = e.forward_u8(batch)
    t_host = time.perf_counter() - t0
    assert (ids_g == ids_h).all() and (p_g == p_h).all()
    print('%d images %dx%d: GPU crop+resize+forward %.1f img/s (%.2f ms/img, %.0f MB of crop windows uploaded)   '
          'host crop+resize + forward %.1f img/s (%.1f ms/img)' % (
              N, W, H, N / t_gpu, 1e3 * t_gpu / N, N * min(H, W) ** 2 * 3 / 1e6, N / t_host, 1e3 * t_host / N))


def generated_directory():
    """``(root, d, nn, paths, MB)``: N generated JPEG files of H x W under ``d`` and the bf16 model."""
    from roomnet_amd import infer
    from roomnet_amd.network import RoomNet
    if THREADS:
        infer.DECODE_THREADS = THREADS
    root = tempfile.mkdtemp(prefix='rn_bench_')
    d = os.path.join(root, 'images')
    os.makedirs(d)
    rng = np.random.default_rng(0)
    # photograph-like content (smooth fields + a little noise) so the JPEG files have a realistic size
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for k in range(N):
        f = rng.uniform(0.002, 0.02, 6)
        im = np.stack([127 + 100 * np.sin(f[2 * c] * xx + k) * np.cos(f[2 * c + 1] * yy) for c in range(3)], -1)
        im = np.clip(im + rng.normal(0, 6, im.shape), 0, 255).astype(np.uint8)
        imageio.imwrite(os.path.join(d, 'im_%04d.jpg' % k), im)
    mb = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) / 1e6
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, dtype='bf16', max_batch=64)
    nn.load(os.path.join('roomnet_amd', 'final_model', 'roomnet'))
    paths = sorted(os.path.join(d, f) for f in os.listdir(d))
    nn.infer_images([imageio.imread(paths[0])])
    return root, d, nn, paths, mb


def directory():
    from roomnet_amd import infer
    root, d, nn, paths, mb = generated_directory()
    t0 = time.perf_counter()
    for p in paths:
        imageio.imread(p)
    t_dec1 = time.perf_counter() - t0
    import sklearn.metrics  # noqa: F401  (groundtruth_validation imports it inside the call: keep the one-off import out of its time)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        t0 = time.perf_counter()
        infer.classify_im_dir(nn, d, overlay=False, batch_size=64)
        t_dir = time.perf_counter() - t0
        t0 = time.perf_counter()
        infer.classify_im_dir(nn, d, overlay=True, batch_size=64)          # the reference's default: overlay + re-encoded files
        t_ovl = time.perf_counter() - t0
        lst = os.path.join(root, 'list.txt')
        with open(lst, 'w') as f:
            f.writelines('%s %d\n' % (p, 0) for p in paths)
        t0 = time.perf_counter()
        infer.groundtruth_validation(nn, lst, batch_size=64)
        t_val = time.perf_counter() - t0
        # the reference's caller: one image per call (infer.py:79-82), host decode, serial
        t0 = time.perf_counter()
        for p in paths[:max(8, N // 8)]:
            nn.infer_optimized(imageio.imread(p))
        t_one = (time.perf_counter() - t0) / max(8, N // 8)
    # what the overlay path cost per image while it ran inside the loop (two put_text + imwrite, one thread)
    ims = [imageio.imread(p) for p in paths[:max(8, N // 16)]]
    t0 = time.perf_counter()
    for k, im in enumerate(ims):
        infer._overlay_and_write(im, 'LivingRoom', np.float32(0.9987), os.path.join(root, 'ovl_%d.jpg' % k))
    t_ow = (time.perf_counter() - t0) / len(ims)
    print('%d JPEG files %dx%d (%.0f MB), %d decode threads of %d host cores: classify_im_dir(overlay=False) %.1f img/s   '
          'classify_im_dir(overlay=True) %.1f img/s (overlay + write alone, one thread: %.1f img/s)   '
          'groundtruth_validation %.1f img/s   decode alone, one thread %.1f img/s   one image per call (reference loop) %.1f img/s'
          % (N, W, H, mb, infer.DECODE_THREADS, os.cpu_count() or 1, N / t_dir, N / t_ovl, 1.0 / t_ow, N / t_val, N / t_dec1, 1.0 / t_one))
    if '--gpu-decode' in sys.argv:
        gpu_decode_arm(nn, infer, d, lst, paths, N / t_dir, N / t_val, N / t_dec1)
    if '--gpu-encode' in sys.argv:
        gpu_encode_arm(nn, infer, d, paths, 1.0 / t_ow)
    shutil.rmtree(root, ignore_errors=True)


def gpu_decode_arm(nn, infer, d, lst, paths, dir_ips, val_ips, dec1_ips):
    """The gpu_decode=True arm on the files the default arm has just been timed on (same session, same box)."""
    from roomnet_amd import jpegdec
    with open(d + '_classified_results.xls', 'rb') as f:
        xls_host = f.read()
    nn.infer_files(paths[:2])                                  # first-use allocations (ring, device scratch) stay out of the times
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        t0 = time.perf_counter()
        xl = infer.classify_im_dir(nn, d, overlay=False, batch_size=64, gpu_decode=True)
        t_dir = time.perf_counter() - t0
        with open(xl, 'rb') as f:
            same = f.read() == xls_host
        t0 = time.perf_counter()
        infer.groundtruth_validation(nn, lst, batch_size=64, gpu_decode=True)
        t_val = time.perf_counter() - t0
    # the host's share: file read + marker walk + Huffman pass, one thread, into one reused buffer
    datas = [open(p, 'rb').read() for p in paths]
    infos = [jpegdec.probe(b) for b in datas]
    buf = np.empty(max(jpegdec.coeff_count(i) for i in infos), np.int16)
    t0 = time.perf_counter()
    for b in datas:
        info = jpegdec.probe(b)
        assert info.supported and jpegdec.entropy_decode_rc(b, info, buf) == 0
    t_ent = time.perf_counter() - t0
    # the device's share: the pixel stage of one batch (two launches; events on the handle's stream), median of 5 calls
    eng = nn._engine()
    n = min(len(paths), eng.max_batch)
    items = [jpegdec.entropy_decode(b, i) for b, i in zip(datas[:n], infos[:n])]
    ms = []
    for _ in range(5):
        eng.classify_jpegs(items)
        ms.append(eng.jpeg_last_decode_ms())
    ms = sorted(ms)[len(ms) // 2]
    N_ = len(paths)
    print('gpu_decode=True, same files, same session: classify_im_dir(overlay=False) %.1f img/s (x%.2f)   groundtruth_validation '
          '%.1f img/s (x%.2f)   workbook identical: %s   host entropy pass alone, one thread %.1f img/s (x%.2f of the one-thread '
          'decode)   pixel stage on the device %.3f ms per batch of %d (%.1f us per image)'
          % (N_ / t_dir, (N_ / t_dir) / dir_ips, N_ / t_val, (N_ / t_val) / val_ips, same, N_ / t_ent, (N_ / t_ent) / dec1_ips, ms, n,
             1e3 * ms / n))


def gpu_encode_arm(nn, infer, d, paths, overlay_write_ips):
    """overlay=True on the host against the gpu_decode + gpu_encode arm: same files, same session, alternating."""
    from roomnet_amd import jpegdec, jpegenc

    def outputs():
        out = {}
        for dirpath, _dirs, names in os.walk(d + '_classified'):
            for name in names:
                with open(os.path.join(dirpath, name), 'rb') as f:
                    out[name] = f.read()
        return out

    arms = {'host': dict(), 'gpu': dict(gpu_decode=True, gpu_encode=True)}
    times = {'host': [], 'gpu': []}
    files = {}
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        for rep in range(4):                              # (the first round is the warm-up of both arms)
            for arm, kw in arms.items():
                t0 = time.perf_counter()
                infer.classify_im_dir(nn, d, overlay=True, batch_size=64, **kw)
                if rep:
                    times[arm].append(time.perf_counter() - t0)
                files[arm] = outputs()
    same = files['host'] == files['gpu'] and len(files['gpu']) == len(paths)
    # the host's share of the encode: the Huffman pass of each output file, one thread (coefficients of the host restatement's source:
    # the decode of the file itself)
    eng = nn._engine()
    n = min(len(paths), eng.max_batch)
    ims = [imageio.imread(p) for p in paths[:n]]
    infos = [jpegenc.encode_info(im.shape[0], im.shape[1]) for im in ims]
    pinned = [_capi.PinnedArray((jpegdec.coeff_count(i),), np.int16) for i in infos]
    d_ims = [eng.device_malloc(im.nbytes) for im in ims]
    for p, im in zip(d_ims, ims):
        eng.h2d(p, im)
    lines = [infer._overlay_lines(im.shape[0], im.shape[1], 'LivingRoom', np.float32(0.9987)) for im in ims]
    from roomnet_amd import hershey
    ovs = [[(b[0], b[1], b[2], color) for b, color in ((hershey.coverage(t, o, s_, im.shape, 1), c) for t, o, s_, c in ln) if b is not None]
           for im, ln in zip(ims, lines)]
    items = [(p, i, o, c.array) for p, i, o, c in zip(d_ims, infos, ovs, pinned)]
    ms = []
    for _ in range(6):
        eng.jpeg_encode_batch(items)
        eng.sync()
        ms.append(eng.jpeg_last_encode_ms())
    ms = sorted(ms[1:])[2]
    t0 = time.perf_counter()
    total = 0
    for i, c in zip(infos, pinned):
        total += len(jpegenc.entropy_encode(i, c.array))
    t_huff = (time.perf_counter() - t0) / n
    for p in d_ims:
        eng.device_free(p)
    for c in pinned:
        c.close()
    N_ = len(paths)
    med = {a: sorted(t)[len(t) // 2] for a, t in times.items()}
    print('overlay=True, same files, same session, alternating, 3 runs each after a warm-up: host decode + overlay + write %.1f img/s '
          '(runs %s)   gpu_decode + gpu_encode %.1f img/s (runs %s)   x%.2f   output files identical: %s   host Huffman-encode pass '
          'alone, one thread %.1f img/s (%.2f MB per file; overlay + write alone, one thread: %.1f img/s)   overlay + encode launches on '
          'the device %.3f ms per batch of %d (%.1f us per image)'
          % (N_ / med['host'], ' '.join('%.1f' % (N_ / t) for t in times['host']), N_ / med['gpu'],
             ' '.join('%.1f' % (N_ / t) for t in times['gpu']), med['host'] / med['gpu'], same, 1.0 / t_huff, total / n / 1e6,
             overlay_write_ips, ms, n, 1e3 * ms / n))


def heatmap_arm():
    """The heat map's launches against the decode's and the encode's pixel stages, and the directory driver with and without it."""
    from roomnet_amd import infer, jpegdec, jpegenc
    root, d, nn, paths, mb = generated_directory()
    eng = nn._engine()
    n = min(len(paths), eng.max_batch)
    items = [jpegdec.entropy_decode(open(p, 'rb').read()) for p in paths[:n]]
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    cam_ms, dec_ms = {}, []
    for layer in ('s6.bn', 's7.bn'):
        ms = []
        for _ in range(6):
            _ids, _probs, addrs, shapes, d_cams, map_shape = eng.explain_resident(items, [], layer)
            dec_ms.append(eng.jpeg_last_decode_ms())
            eng.cam_overlay_batch([(addrs[k], shapes[k], d_cams[k], map_shape) for k in range(n)], 0.5)
            eng.sync()
            ms.append(eng.cam_last_overlay_ms())
        cam_ms[layer] = med(ms[1:])
    infos = [jpegenc.encode_info(h, w) for h, w in shapes]
    pinned = [_capi.PinnedArray((jpegdec.coeff_count(i),), np.int16) for i in infos]
    enc_ms = []
    for _ in range(6):
        eng.jpeg_encode_batch([(a, i, [], c.array) for a, i, c in zip(addrs, infos, pinned)])
        eng.sync()
        enc_ms.append(eng.jpeg_last_encode_ms())
    for c in pinned:
        c.close()
    side = min(H, W)
    print('%d JPEG files %dx%d (%.0f MB), one batch of %d, window %dx%d: heat map launches %.3f ms (s6.bn, 46x46 maps; %.1f us per image, '
          '%.0f GB/s of the 6 B per window pixel)  %.3f ms (s7.bn, 21x21 maps)   decode pixel stage %.3f ms   encode pixel stage %.3f ms'
          % (len(paths), W, H, mb, n, side, side, cam_ms['s6.bn'], 1e3 * cam_ms['s6.bn'] / n, n * side * side * 6 / cam_ms['s6.bn'] / 1e6,
             cam_ms['s7.bn'], med(dec_ms[1:]), med(enc_ms[1:])))
    arms = {'gpu + heat map': dict(gpu_decode=True, gpu_encode=True, heatmap='s6.bn'), 'gpu': dict(gpu_decode=True, gpu_encode=True),
            'host + heat map': dict(heatmap='s6.bn')}
    times = {a: [] for a in arms}
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        for rep in range(3):                              # (the first round is the warm-up of every arm)
            for arm, kw in arms.items():
                t0 = time.perf_counter()
                infer.classify_im_dir(nn, d, overlay=True, batch_size=64, **kw)
                if rep:
                    times[arm].append(time.perf_counter() - t0)
    N_ = len(paths)
    print('classify_im_dir(overlay=True), same files, same session, alternating, 2 runs each after a warm-up, %d decode threads:   '
          % infer.DECODE_THREADS + '   '.join('%s %s img/s' % (a, ' / '.join('%.1f' % (N_ / x) for x in t)) for a, t in times.items()))
    shutil.rmtree(root, ignore_errors=True)


def gpu_huffman_arm():
    """gpu_decode=True against gpu_decode=True, gpu_huffman=True: same files, same session, alternating."""
    from roomnet_amd import infer, jpegdec
    root, d, nn, paths, mb = generated_directory()
    lst = os.path.join(root, 'list.txt')
    with open(lst, 'w') as f:
        f.writelines('%s %d\n' % (p, 0) for p in paths)
    import sklearn.metrics  # noqa: F401
    arms = {'host Huffman': dict(gpu_decode=True), 'GPU Huffman': dict(gpu_decode=True, gpu_huffman=True)}
    t_dir = {a: [] for a in arms}
    t_val = {a: [] for a in arms}
    xls, fallbacks = {}, 0
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        for rep_ in range(4):                                  # round 0 is the warm-up of both arms
            for arm, kw in arms.items():
                t0 = time.perf_counter()
                xl = infer.classify_im_dir(nn, d, overlay=False, batch_size=64, **kw)
                t1 = time.perf_counter()
                fallbacks += getattr(nn, 'huffman_fallbacks', 0) if 'gpu_huffman' in kw else 0
                with open(xl, 'rb') as f:
                    xls[arm] = f.read()
                t2 = time.perf_counter()
                infer.groundtruth_validation(nn, lst, batch_size=64, **kw)
                t3 = time.perf_counter()
                fallbacks += getattr(nn, 'huffman_fallbacks', 0) if 'gpu_huffman' in kw else 0
                if rep_:
                    t_dir[arm].append(t1 - t0)
                    t_val[arm].append(t3 - t2)
    # the host's share per file, one thread: read + marker walk + Huffman pass against read + marker walks
    ring_c, ring_b = jpegdec.CoeffRing(1), jpegdec.ByteRing(1)
    t0 = time.perf_counter()
    for p in paths:
        assert jpegdec.load_file(p, ring_c, 0)[0] == 'jpeg'
    t_host = (time.perf_counter() - t0) / len(paths)
    t0 = time.perf_counter()
    for p in paths:
        assert jpegdec.load_file_bytes(p, ring_b, 0)[0] == 'file'
    t_bytes = (time.perf_counter() - t0) / len(paths)
    # the device's share: the Huffman launches of one batch, median of 5 calls, and the rounds phase 2 took
    eng = nn._engine()
    n = min(len(paths), eng.max_batch)
    rings = jpegdec.ByteRing(n)
    items = [jpegdec.load_file_bytes(p, rings, k)[1:] for k, p in enumerate(paths[:n])]
    ms, px = [], []
    for _ in range(5):
        _ids, _probs, status = eng.classify_jpeg_files(items)
        assert not status.any()
        ms.append(eng.jpeg_last_huffman_ms())
        px.append(eng.jpeg_last_decode_ms())
    inside, across = eng.jpeg_last_huffman_rounds(n)
    ms, px = sorted(ms)[2], sorted(px)[2]
    med = lambda t: sorted(t)[len(t) // 2]
    N_ = len(paths)
    scan_mb = sum(int(it[1].scan_len) for it in items) / 1e6
    coef_mb = sum(jpegdec.coeff_count(it[0]) for it in items) * 2 / 1e6
    print('%d JPEG files %dx%d (%.0f MB), %d decode threads of %d host cores, same files, same session, alternating, 3 runs each after a '
          'warm-up of both:' % (N_, W, H, mb, infer.DECODE_THREADS, os.cpu_count() or 1))
    for arm in arms:
        print('  %-12s classify_im_dir(overlay=False) %s img/s   groundtruth_validation %s img/s' % (
            arm + ':', ' / '.join('%.1f' % (N_ / x) for x in t_dir[arm]), ' / '.join('%.1f' % (N_ / x) for x in t_val[arm])))
    print('  ratio GPU Huffman / host Huffman (medians): classify_im_dir x%.2f   groundtruth_validation x%.2f   workbook identical: %s   '
          'host fallbacks: %d' % (med(t_dir['host Huffman']) / med(t_dir['GPU Huffman']), med(t_val['host Huffman']) / med(t_val['GPU Huffman']),
                                  xls['host Huffman'] == xls['GPU Huffman'], fallbacks))
    print('  host share per file, one thread: %.3f ms with the Huffman pass, %.3f ms without (file read + marker walks)   upload per batch '
          'of %d: %.1f MB of scan bytes instead of %.1f MB of coefficients' % (1e3 * t_host, 1e3 * t_bytes, n, scan_mb, coef_mb))
    print('  Huffman launches on the device: %.3f ms per batch of %d (%.1f us per image; pixel stage %.3f ms)   sync rounds per image: '
          'inside groups median %d, most %d; across groups median %d, most %d'
          % (ms, n, 1e3 * ms / n, px, int(np.median(inside)), int(inside.max()), int(np.median(across)), int(across.max())))
    shutil.rmtree(root, ignore_errors=True)


def gpu_huffman_encode_arm():
    """overlay=True on the host, gpu_decode + gpu_encode, and + gpu_huffman_encode: same files, same session, alternating."""
    from roomnet_amd import hershey, infer, jpegdec, jpegenc
    root, d, nn, paths, mb = generated_directory()

    def outputs():
        out = {}
        for dirpath, _dirs, names in os.walk(d + '_classified'):
            for name in names:
                with open(os.path.join(dirpath, name), 'rb') as f:
                    out[name] = f.read()
        return out

    arms = {'host': dict(), 'gpu_encode': dict(gpu_decode=True, gpu_encode=True),
            'gpu_huffman_encode': dict(gpu_decode=True, gpu_encode=True, gpu_huffman_encode=True)}
    times = {a: [] for a in arms}
    files, fallbacks = {}, 0
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        for rep_ in range(4):                             # (the first round is the warm-up of every arm)
            for arm, kw in arms.items():
                t0 = time.perf_counter()
                infer.classify_im_dir(nn, d, overlay=True, batch_size=64, **kw)
                if rep_:
                    times[arm].append(time.perf_counter() - t0)
                if 'gpu_huffman_encode' in kw:
                    fallbacks += nn.huffenc_fallbacks
                files[arm] = outputs()
    same = files['host'] == files['gpu_encode'] == files['gpu_huffman_encode'] and len(files['host']) == len(paths)
    # one batch on its own: the device time of the pixel stage and of the four phases, the bytes that come down, and the host's
    # Huffman-encode pass of the same files on one thread
    eng = nn._engine()
    n = min(len(paths), eng.max_batch)
    ims = [imageio.imread(p) for p in paths[:n]]
    infos = [jpegenc.encode_info(im.shape[0], im.shape[1]) for im in ims]
    pinned = [_capi.PinnedArray((jpegdec.coeff_count(i),), np.int16) for i in infos]
    outs = [_capi.PinnedArray((min(jpegenc.encoded_bound(i), 1024 + 2 * jpegdec.coeff_count(i)),), np.uint8) for i in infos]
    d_ims = [eng.device_malloc(im.nbytes) for im in ims]
    for p, im in zip(d_ims, ims):
        eng.h2d(p, im)
    lines = [infer._overlay_lines(im.shape[0], im.shape[1], 'LivingRoom', np.float32(0.9987)) for im in ims]
    ovs = [[(b[0], b[1], b[2], color) for b, color in ((hershey.coverage(t, o, s_, im.shape, 1), c) for t, o, s_, c in ln) if b is not None]
           for im, ln in zip(ims, lines)]
    px_ms, huff_ms, call_ms, coef_ms = [], [], [], []
    for _ in range(6):
        t0 = time.perf_counter()
        eng.jpeg_encode_batch([(p, i, [], c.array) for p, i, c in zip(d_ims, infos, pinned)])
        eng.sync()
        coef_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        lens, status = eng.jpeg_encode_files([(p, i, [], None) for p, i in zip(d_ims, infos)], outs)
        call_ms.append(1e3 * (time.perf_counter() - t0))
        assert not status.any()
        px_ms.append(eng.jpeg_last_encode_ms())
        huff_ms.append(eng.jpeg_last_huffenc_ms())
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    px_ms, huff_ms, call_ms, coef_ms = med(px_ms[1:]), med(huff_ms[1:]), med(call_ms[1:]), med(coef_ms[1:])
    t0 = time.perf_counter()
    total = 0
    for k, (i, c) in enumerate(zip(infos, pinned)):
        data = jpegenc.entropy_encode(i, c.array)
        assert data == outs[k].array[:lens[k]].tobytes()
        total += len(data)
    t_huff = (time.perf_counter() - t0) / n
    # (the overlays: drawn once at the end so the timed calls above encode the same pixels every time)
    eng.jpeg_encode_batch([(p, i, o, c.array) for p, i, o, c in zip(d_ims, infos, ovs, pinned)])
    eng.sync()
    ovl_ms = eng.jpeg_last_encode_ms()
    for p in d_ims:
        eng.device_free(p)
    for c in pinned + outs:
        c.close()
    N_ = len(paths)
    m = {a: med(t) for a, t in times.items()}
    runs = {a: ' / '.join('%.1f' % (N_ / x) for x in t) for a, t in times.items()}
    spread = {a: (max(t) - min(t)) / med(t) for a, t in times.items()}
    coef_mb = sum(jpegdec.coeff_count(i) for i in infos) * 2 / 1e6
    print('%d JPEG files %dx%d (%.0f MB), %d decode threads of %d host cores, classify_im_dir(overlay=True), same files, same session, '
          'alternating, 3 runs each after a warm-up of all:' % (N_, W, H, mb, infer.DECODE_THREADS, os.cpu_count() or 1))
    for arm in arms:
        print('  %-20s %s img/s (median %.1f, spread of the run times %.1f %%)' % (arm + ':', runs[arm], N_ / m[arm], 100 * spread[arm]))
    print('  ratio gpu_huffman_encode / gpu_encode (medians): x%.2f   gpu_encode / host: x%.2f   gpu_huffman_encode / host: x%.2f   '
          'output files identical in all three: %s   host fallbacks: %d'
          % (m['gpu_encode'] / m['gpu_huffman_encode'], m['host'] / m['gpu_encode'], m['host'] / m['gpu_huffman_encode'], same, fallbacks))
    print('  one batch of %d without overlays: pixel stage on the device %.3f ms, the four Huffman phases %.3f ms (%.1f us per image); the '
          'whole jpeg_encode_files call %.2f ms on the host clock against %.2f ms for jpeg_encode_batch + sync   downloaded per batch: '
          '%.1f MB of files instead of %.1f MB of coefficients   host Huffman-encode pass alone, one thread: %.3f ms per file '
          '(%.1f img/s, %.2f MB per file)'
          % (n, px_ms, huff_ms, 1e3 * huff_ms / n, call_ms, coef_ms, sum(lens) / 1e6, coef_mb, 1e3 * t_huff, 1.0 / t_huff, total / n / 1e6))
    print('overlay=True, same files, same session, alternating, 3 runs each after a warm-up: host decode + overlay + write %.1f img/s '
          '(runs %s)   gpu_decode + gpu_encode %.1f img/s (runs %s)   x%.2f   output files identical: %s   host Huffman-encode pass '
          'alone, one thread %.1f img/s (%.2f MB per file)   overlay + encode launches on the device %.3f ms per batch of %d (%.1f us '
          'per image)'
          % (N_ / m['host'], runs['host'], N_ / m['gpu_encode'], runs['gpu_encode'], m['host'] / m['gpu_encode'],
             files['host'] == files['gpu_encode'], 1.0 / t_huff, total / n / 1e6, ovl_ms, n, 1e3 * ovl_ms / n))
    shutil.rmtree(root, ignore_errors=True)


def exif_app1(orientation):
    """An APP1 Exif segment (little-endian TIFF) whose IFD0 holds only the orientation tag."""
    import struct
    tiff = b'II' + struct.pack('<HI', 42, 8) + struct.pack('<H', 1) + struct.pack('<HHIHH', 0x0112, 3, 1, orientation, 0) + struct.pack('<I', 0)
    body = b'Exif\x00\x00' + tiff
    return b'\xff\xe1' + struct.pack('>H', len(body) + 2) + body


def splice_orientations(paths, fixed=None):
    """Rewrite every file with an orientation spliced in behind SOI: ``fixed``, or 1..8 in turn.  Returns the count of turned files."""
    turned = 0
    for k, p in enumerate(paths):
        o = fixed or 1 + k % 8
        with open(p, 'rb') as f:
            data = f.read()
        assert data[:2] == b'\xff\xd8'
        with open(p, 'wb') as f:
            f.write(data[:2] + exif_app1(o) + data[2:])
        turned += o != 1
    return turned


def pixel_stage_by_orientation():
    """Device time of the pixel stage for one batch of 64 1920x1080 files, all at orientation 1, 3 and 6: the same coefficients,
    only info.supported differs."""
    global H, W, N
    from roomnet_amd import jpegdec
    H, W, N = 1080, 1920, 64
    root, d, nn, paths, mb = generated_directory()
    eng = nn._engine()
    items = [jpegdec.entropy_decode(open(p, 'rb').read()) for p in paths]
    out = {}
    for rep_ in range(2):                                     # (both rounds are timed; the first call of all is the warm-up)
        for o in (1, 3, 6):
            for info, _c in items:
                info.supported = o
            ms = []
            for _ in range(6):
                eng.classify_jpegs(items)
                ms.append(eng.jpeg_last_decode_ms())
            out.setdefault(o, []).append(sorted(ms[1:])[2])
    px = N * H * W
    print('pixel stage on the device (%s), one batch of %d files 1920x1080 4:2:0, median of 5 calls, two rounds:   '
          % (os.environ.get('ROOMNET_HIP_LIB', 'product library'), N)
          + '   '.join('orientation %d: %s ms (%.0f GB/s of the 3 B coefficients + 3 B planes + 3 B image per pixel)'
                       % (o, ' / '.join('%.3f' % m for m in v), 9 * px / min(v) / 1e6) for o, v in out.items()))
    shutil.rmtree(root, ignore_errors=True)


def gpu_orient_arm():
    """gpu_decode=True (turned files go to imread) against gpu_decode=True, gpu_orient=True: same files, same session, alternating."""
    global H, W
    from roomnet_amd import infer
    import sklearn.metrics  # noqa: F401
    fixed = None
    for a in sys.argv[1:]:
        if a.startswith('--orientation='):
            fixed = int(a.split('=', 1)[1])
    sizes = [(H, W)] if args else [(480, 640), (1080, 1920)]
    for H, W in sizes if '--stage-only' not in sys.argv else []:
        root, d, nn, paths, mb = generated_directory()
        turned = splice_orientations(paths, fixed)
        lst = os.path.join(root, 'list.txt')
        with open(lst, 'w') as f:
            f.writelines('%s %d\n' % (p, 0) for p in paths)
        arms = {'gpu_decode': dict(gpu_decode=True), 'gpu_decode + gpu_orient': dict(gpu_decode=True, gpu_orient=True)}
        t_dir = {a: [] for a in arms}
        t_val = {a: [] for a in arms}
        xls, ways = {}, {}
        with contextlib.redirect_stdout(io.StringIO()):
            for rep_ in range(4):                                  # round 0 is the warm-up of both arms
                for arm, kw in arms.items():
                    t0 = time.perf_counter()
                    xl = infer.classify_im_dir(nn, d, overlay=False, batch_size=64, **kw)
                    t1 = time.perf_counter()
                    ways[arm] = dict(nn.last_decode_paths)
                    with open(xl, 'rb') as f:
                        xls[arm] = f.read()
                    t2 = time.perf_counter()
                    infer.groundtruth_validation(nn, lst, batch_size=64, **kw)
                    t3 = time.perf_counter()
                    if rep_:
                        t_dir[arm].append(t1 - t0)
                        t_val[arm].append(t3 - t2)
        med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
        spread = lambda t: 100 * (max(t) - min(t)) / med(t)      # noqa: E731
        N_ = len(paths)
        print('%d JPEG files %dx%d (%.0f MB), orientation %s (%d turned), %d decode threads of %d host cores, same files, same session, '
              'alternating, 3 runs each after a warm-up of both:' % (N_, W, H, mb, fixed or 'cycling 1..8', turned, infer.DECODE_THREADS,
                                                                     os.cpu_count() or 1))
        for arm in arms:
            print('  %-24s classify_im_dir(overlay=False) %s img/s (spread of the run times %.1f %%)   groundtruth_validation %s img/s '
                  '(spread %.1f %%)   ways: %s' % (arm + ':', ' / '.join('%.1f' % (N_ / x) for x in t_dir[arm]), spread(t_dir[arm]),
                                                   ' / '.join('%.1f' % (N_ / x) for x in t_val[arm]), spread(t_val[arm]), ways[arm]))
        a, b = 'gpu_decode', 'gpu_decode + gpu_orient'
        print('  ratio gpu_orient / gpu_decode alone (medians): classify_im_dir x%.2f   groundtruth_validation x%.2f   workbook identical: %s'
              % (med(t_dir[a]) / med(t_dir[b]), med(t_val[a]) / med(t_val[b]), xls[a] == xls[b]))
        shutil.rmtree(root, ignore_errors=True)
    pixel_stage_by_orientation()


def occlusion_arm():
    """(a) the device call against the plain passes it is made of, (b) against the Python route, (c) the directory driver."""
    global H, W, N
    from roomnet_amd import infer, occlusion
    from roomnet_amd.network import RoomNet
    n = int(args[0]) if args else 64
    out_path = next((a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('--out=')), os.path.join('profiles', 'occlusion_bench.txt'))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    patch, stride, S = 32, 16, 224
    nn = RoomNet(num_classes=6, im_side=S, compute_bn_mean_var=False, optimized_inference=True, dtype='bf16', max_batch=64)
    nn.load(os.path.join('roomnet_amd', 'final_model', 'roomnet'))
    eng = nn._engine()
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    ims = np.stack([np.clip(np.stack([127 + 100 * np.sin(f[2 * c] * xx + k) * np.cos(f[2 * c + 1] * yy) for c in range(3)], -1)
                            + rng.normal(0, 6, (S, S, 3)), 0, 255).astype(np.uint8)
                    for k, f in enumerate(rng.uniform(0.01, 0.08, (n, 6)))])
    G, n_windows, n_chunks = eng.occlusion_plan(n, patch, stride)
    plan = occlusion.chunks(n_windows, eng.max_batch)
    d_bgr, d_work = eng.device_malloc(ims.nbytes), eng.device_malloc(eng.max_batch * S * S * 3)
    d_drop, d_map = eng.device_malloc(n_windows * 4), eng.device_malloc(n * S * S * 4)
    d_probs, d_ids = eng.device_malloc(eng.max_batch * 6 * 4), eng.device_malloc(eng.max_batch * 8)
    eng.h2d(d_bgr, ims)
    eng.h2d(d_work, np.ascontiguousarray(np.resize(ims, (eng.max_batch, S, S, 3))))

    def occluded():
        t0 = time.perf_counter()
        eng.occlusion_u8_device(d_bgr, n, None, patch, stride, 'mean', d_drop, d_map, d_probs, d_ids)
        eng.sync()
        return 1e3 * (time.perf_counter() - t0), eng.occlusion_last_ms()

    def plain():
        t0 = time.perf_counter()
        eng.forward_u8_device(d_bgr, n, d_probs, d_ids)
        for _first, count in plan:
            eng.forward_u8_device(d_work, count, d_probs, d_ids)
        eng.sync()
        return 1e3 * (time.perf_counter() - t0)

    occluded(), plain()                                  # the warm-up of both (the first call allocates the workspaces)
    t_occ, t_dev, t_plain = [], [], []
    for _ in range(3):
        a, b = occluded()
        t_occ.append(a)
        t_dev.append(b)
        t_plain.append(plain())
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    say('(a) %d resident images at %d, patch %d, stride %d: G = %d, %d masked passes in %d chunks of %d, bf16.  One rn_occlusion_u8_device '
        'call, enqueue to sync: %s ms (device time of the call: %s ms)   the same %d + %d plain rn_forward_u8_device calls on a resident '
        'buffer: %s ms   alternating, same session, 3 runs each after a warm-up of both   ratio of the medians: %.3f   %.0f masked '
        'passes/ms' % (n, S, patch, stride, G, n_windows, n_chunks, eng.max_batch, ' / '.join('%.2f' % x for x in t_occ),
                       ' / '.join('%.2f' % x for x in t_dev), 1, n_chunks, ' / '.join('%.2f' % x for x in t_plain),
                       med(t_occ) / med(t_plain), n_windows / med(t_occ)))
    maps = np.empty((n, S, S), np.float32)
    eng.d2h(maps, d_map)
    t0 = time.perf_counter()
    want = occlusion.occlusion_map_host(lambda b: nn.infer(b)[1], ims, patch=patch, stride=stride, max_batch=eng.max_batch)
    t_py = 1e3 * (time.perf_counter() - t0)
    say('(b) the Python route, occlusion.occlusion_map_host over nn.infer (masked copies built with NumPy, %.0f MB uploaded): %.0f ms, '
        'x%.1f the device call; maps identical: %s' % (n_windows * S * S * 3 / 1e6, t_py, t_py / med(t_occ), bool(np.array_equal(maps, want[0]))))
    for d in (d_bgr, d_work, d_drop, d_map, d_probs, d_ids):
        eng.device_free(d)
    nn.sess.close()
    for H, W in ((480, 640), (1080, 1920)):
        N = n
        root, d, nn2, paths, mb = generated_directory()
        arms = {'occlusion': dict(heatmap='occlusion'), 's6.bn': dict(heatmap='s6.bn')}
        times = {a: [] for a in arms}
        with contextlib.redirect_stdout(io.StringIO()):
            for rep in range(3):                          # (the first round is the warm-up of both arms)
                for arm, kw in arms.items():
                    t0 = time.perf_counter()
                    infer.classify_im_dir(nn2, d, overlay=True, batch_size=64, gpu_decode=True, gpu_encode=True, **kw)
                    if rep:
                        times[arm].append(time.perf_counter() - t0)
        say('(c) %d JPEG files %dx%d (%.0f MB), classify_im_dir(overlay=True, gpu_decode=True, gpu_encode=True), %d decode threads, alternating, '
            '2 runs each after a warm-up:   ' % (len(paths), W, H, mb, infer.DECODE_THREADS)
            + '   '.join('heatmap=%r %s img/s' % (a, ' / '.join('%.1f' % (len(paths) / x) for x in t)) for a, t in times.items()))
        nn2.sess.close()
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('python tools/bench_images.py --occlusion %d\n' % n + '\n'.join(lines) + '\n')


def faithfulness_arm():
    """(a) the device call against the plain passes it is made of and the rank launch alone, (b) against the Python route,
    (c) compare_heatmaps on generated files."""
    global H, W, N
    from roomnet_amd import faithfulness, infer
    from roomnet_amd.network import RoomNet
    n = int(args[0]) if args else 64
    out_path = next((a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('--out=')), os.path.join('profiles', 'faithfulness_bench.txt'))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    steps, modes, S = 32, 3, 224
    nn = RoomNet(num_classes=6, im_side=S, compute_bn_mean_var=False, optimized_inference=True, dtype='bf16', max_batch=64)
    nn.load(os.path.join('roomnet_amd', 'final_model', 'roomnet'))
    eng = nn._engine()
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    ims = np.stack([np.clip(np.stack([127 + 100 * np.sin(f[2 * c] * xx + k) * np.cos(f[2 * c + 1] * yy) for c in range(3)], -1)
                            + rng.normal(0, 6, (S, S, 3)), 0, 255).astype(np.uint8)
                    for k, f in enumerate(rng.uniform(0.01, 0.08, (n, 6)))])
    # maps as a caller has them: smooth bumps with a zero plateau (an upsampled ReLU'd coarse map)
    from roomnet_amd import cam
    maps = np.ascontiguousarray(cam.upsample(rng.normal(-0.3, 1, (n, 46, 46)), S), dtype=np.float32)
    n_passes, n_chunks = eng.faith_plan(n, steps, modes)
    plan = faithfulness.chunks(n_passes, eng.max_batch)
    d_bgr, d_work = eng.device_malloc(ims.nbytes), eng.device_malloc(eng.max_batch * S * S * 3)
    d_map, d_rank = eng.device_malloc(maps.nbytes), eng.device_malloc(n * S * S * 4)
    d_curve, d_auc = eng.device_malloc(n_passes * 4), eng.device_malloc(n * 2 * 4)
    d_probs, d_ids = eng.device_malloc(eng.max_batch * 6 * 4), eng.device_malloc(eng.max_batch * 8)
    eng.h2d(d_bgr, ims)
    eng.h2d(d_map, maps)
    eng.h2d(d_work, np.ascontiguousarray(np.resize(ims, (eng.max_batch, S, S, 3))))

    def curves():
        t0 = time.perf_counter()
        eng.faith_u8_device(d_bgr, d_map, n, None, steps, modes, 'mean', d_curve, d_auc, d_probs, d_ids)
        eng.sync()
        return 1e3 * (time.perf_counter() - t0), eng.faith_last_ms()

    def plain():
        t0 = time.perf_counter()
        eng.forward_u8_device(d_bgr, n, d_probs, d_ids)
        for _first, count in plan:
            eng.forward_u8_device(d_work, count, d_probs, d_ids)
        eng.sync()
        return 1e3 * (time.perf_counter() - t0)

    def rank_alone():
        eng.faith_ranks_device(d_map, n, d_rank)
        eng.sync()
        return eng.faith_last_ms()

    curves(), plain()                                    # the warm-up of both (the first call allocates the workspaces)
    t_call, t_dev, t_plain = [], [], []
    for _ in range(3):
        a, b = curves()
        t_call.append(a)
        t_dev.append(b)
        t_plain.append(plain())
    got_curves, got_aucs = np.empty((n, 2, steps + 1), np.float32), np.empty((n, 2), np.float32)
    eng.d2h(got_curves, d_curve)
    eng.d2h(got_aucs, d_auc)
    rank_alone()
    t_rank = [rank_alone() for _ in range(3)]
    ranks = np.empty((n, S, S), np.uint32)
    eng.d2h(ranks, d_rank)
    ranks_ok = all(np.array_equal(ranks[k], faithfulness.ranks(maps[k])) for k in range(n))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    say('(a) %d resident images at %d, %d steps, both curves: %d masked passes in %d chunks of %d, bf16.  One rn_faith_u8_device call, '
        'enqueue to sync: %s ms (device time of the call: %s ms)   the same %d + %d plain rn_forward_u8_device calls on a resident buffer: '
        '%s ms   alternating, same session, 3 runs each after a warm-up of both   ratio of the medians: %.3f   %.0f masked passes/ms   '
        'the rank launch alone (rn_faith_ranks_device, %d maps, one workgroup each): %s ms of device time, %.4f of the call; ranks equal '
        'the stable argsort: %s'
        % (n, S, steps, n_passes, n_chunks, eng.max_batch, ' / '.join('%.2f' % x for x in t_call), ' / '.join('%.2f' % x for x in t_dev), 1,
           n_chunks, ' / '.join('%.2f' % x for x in t_plain), med(t_call) / med(t_plain), n_passes / med(t_call), n,
           ' / '.join('%.3f' % x for x in t_rank), med(t_rank) / med(t_dev), ranks_ok))
    t0 = time.perf_counter()
    want = faithfulness.curves_host(lambda b: nn.infer(b)[1], ims, maps, steps=steps, modes=modes, max_batch=eng.max_batch)
    t_py = 1e3 * (time.perf_counter() - t0)
    say('(b) the Python route, faithfulness.curves_host over nn.infer (one argsort per map, masked copies built with NumPy, %.0f MB uploaded): '
        '%.0f ms, x%.1f the device call; curves identical: %s, areas identical: %s'
        % (n_passes * S * S * 3 / 1e6, t_py, t_py / med(t_call), bool(np.array_equal(got_curves, want[0])), bool(np.array_equal(got_aucs, want[1]))))
    for d in (d_bgr, d_work, d_map, d_rank, d_curve, d_auc, d_probs, d_ids):
        eng.device_free(d)
    nn.sess.close()
    H, W, N = 480, 640, n
    root, d, nn2, paths, mb = generated_directory()
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        report = infer.compare_heatmaps(nn2, d, steps=steps, batch_size=64)
        t_cmp = time.perf_counter() - t0
    say('(c) %d JPEG files %dx%d (%.0f MB), infer.compare_heatmaps(steps=%d), mean areas (deletion / insertion):   ' % (len(paths), W, H, mb, steps)
        + '   '.join('%s %.4f / %.4f' % (m, r['deletion'], r['insertion']) for m, r in report.items()) + '   in %.1f s' % t_cmp)
    nn2.sess.close()
    shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('python tools/bench_images.py --faithfulness %d\n' % n + '\n'.join(lines) + '\n')


if '--faithfulness' in sys.argv:
    faithfulness_arm()
elif '--occlusion' in sys.argv:
    occlusion_arm()
elif '--heatmap' in sys.argv:
    heatmap_arm()
elif '--dir' in sys.argv and '--gpu-orient' in sys.argv:
    gpu_orient_arm()
elif '--dir' in sys.argv and '--gpu-huffman-encode' in sys.argv:
    gpu_huffman_encode_arm()
elif '--dir' in sys.argv and '--gpu-huffman' in sys.argv:
    gpu_huffman_arm()
elif '--dir' in sys.argv:
    directory()
else:
    decoded_images()
