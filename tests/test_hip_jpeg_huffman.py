"""GPU Huffman stage of the JPEG decoder (csrc/rn_jpeg_huff.hip: rn_jpeg_huffman_batch, rn_classify_jpeg_files) and the drivers'
gpu_huffman path.  JPEG bytes are made with Pillow's encoder; the reference is the host's Huffman pass on the same bytes
(rn_jpeg_entropy_decode), byte for byte, and for the status codes the host model of the same algorithm (rn_jpeg_huffman_model)."""
import ctypes as C
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

from conftest import MODEL_PREFIX  # noqa: E402
from jpeg_cases import SAMPLINGS, VARIANTS, content, encode, hand_built_grey_8x8  # noqa: E402
from roomnet_amd import _capi, jpegdec  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 128
SUBSEQ = _capi.RN_JPEG_SUBSEQ_BYTES
SMALL = [(1, 1), (17, 33), (31, 2), (72, 96), (200, 150)]           # h x w
RN_E_INVALID, RN_E_RANGE = -1, -5


def file_item(data):
    """(info, scan, the scan's bytes as a uint8 array) of a supported file, as Engine._jpeg_files takes them."""
    info = jpegdec.probe(data)
    rc, scan = jpegdec.scan_probe_rc(data)
    assert rc == 0 and info.supported and scan.scan_len == len(data) - scan.scan_begin
    return info, scan, np.frombuffer(data, np.uint8)[int(scan.scan_begin):].copy()


def host_coeffs(data):
    info = jpegdec.probe(data)
    out = np.empty(jpegdec.coeff_count(info), np.int16)
    return jpegdec.entropy_decode_rc(data, info, out), out


@pytest.fixture(scope="module")
def engine(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """[(bytes, host coefficients)]: every small size x sampling x variant (120 files, contents alternating), then one 640 x 480
    quality-95 4:2:0 noise file; computed once."""
    p = str(tmp_path_factory.mktemp("jpeg_huff") / "c.jpg")
    out = []
    for h, w in SMALL:
        for sampling in SAMPLINGS:
            for kw in VARIANTS:
                data = encode(p, content(h, w, ["noise", "smooth"][len(out) % 2], seed=len(out)), sampling, **kw)
                rc, ref = host_coeffs(data)
                assert rc == 0
                out.append((data, ref))
    data = encode(p, content(480, 640, "noise", seed=5), 2, quality=95)
    rc, ref = host_coeffs(data)
    assert rc == 0
    out.append((data, ref))
    return out


def test_one_mixed_batch_equals_the_host_pass(engine, corpus):
    items = [file_item(data) for data, _ref in corpus]
    assert len(items) == 121 <= MAX_BATCH
    # what the batch exercises, asserted from the bytes: the launch across groups, a seam directly behind the FF of an FF 00 pair,
    # restart markers
    assert int(items[-1][1].scan_len) > _capi.RN_JPEG_SUBSEQ_BYTES * 256
    behind_ff = 0
    for _info, _scan, s in items:
        seams = np.arange(SUBSEQ, len(s), SUBSEQ)
        behind_ff += int(((s[seams] == 0x00) & (s[seams - 1] == 0xFF)).sum())
    assert behind_ff >= 1
    assert sum(1 for info, _s, _b in items if info.restart_interval) >= 1
    status, got = engine.jpeg_huffman_batch(items)
    assert status.tolist() == [0] * len(items)
    for k, (_data, ref) in enumerate(corpus):
        assert np.array_equal(got[k], ref), k
    assert engine.jpeg_last_huffman_ms() > 0
    inside, across = engine.jpeg_last_huffman_rounds(len(items))
    print("sync rounds of the 640x480 file: inside groups %d, across groups %d" % (inside[-1], across[-1]))
    assert 0 <= inside.max() < 256 and 0 <= across[-1] < -(-int(items[-1][1].scan_len) // (SUBSEQ * 256))


def test_back_to_back_calls_on_different_batches_repeat_their_bytes(engine, corpus):
    a = [file_item(d) for d, _r in corpus[:40]]
    b = [file_item(d) for d, _r in corpus[100:]]
    s1, c1 = engine.jpeg_huffman_batch(a)
    s2, c2 = engine.jpeg_huffman_batch(b)
    s3, c3 = engine.jpeg_huffman_batch(a)
    assert not s1.any() and not s2.any() and not s3.any()
    for k in range(40):
        assert np.array_equal(c1[k], corpus[k][1]) and np.array_equal(c1[k], c3[k]), k
    for k in range(len(b)):
        assert np.array_equal(c2[k], corpus[100 + k][1]), k


def test_damaged_files_get_the_models_status_and_leave_the_good_ones_exact(engine, corpus, tmp_path):
    good = encode(str(tmp_path / "g.jpg"), content(72, 96, "noise", seed=3), 2, quality=90)
    begin = int(jpegdec.scan_probe_rc(good)[1].scan_begin)
    truncated = good[:begin + (len(good) - begin) // 2]
    hit = None
    rng = np.random.default_rng(11)
    for pos in rng.integers(begin, len(good) - 2, 64):              # the first seeded overwrite that the host pass refuses
        b = bytearray(good)
        b[pos] ^= 0x5A
        if host_coeffs(bytes(b))[0] != 0:
            hit = bytes(b)
            break
    assert hit is not None
    over = hand_built_grey_8x8(1, 1097, 0)
    files = [corpus[61][0], truncated, hit, over, corpus[-1][0]]
    want = []
    for d in files:
        info = jpegdec.probe(d)
        rc, st = jpegdec.huffman_model_rc(d, info, np.empty(jpegdec.coeff_count(info), np.int16))
        assert rc == 0
        want.append(st)
        assert (st != 0) == (host_coeffs(d)[0] != 0)
    assert want[0] == 0 and want[4] == 0 and all(want[1:4]) and want[3] == _capi.RN_JPEG_ST_COEF_LIMIT
    status, got = engine.jpeg_huffman_batch([file_item(d) for d in files])
    assert status.tolist() == want
    assert np.array_equal(got[0], corpus[61][1]) and np.array_equal(got[4], corpus[-1][1])
    status, got = engine.jpeg_huffman_batch([file_item(corpus[7][0])])          # the next call on the same handle
    assert status.tolist() == [0] and np.array_equal(got[0], corpus[7][1])


def test_classify_jpeg_files_equals_classify_jpegs(engine, tmp_path):
    datas = []
    for k in range(8):
        h, w = ((300, 400), (400, 300))[k % 2]
        datas.append(encode(str(tmp_path / "c.jpg"), content(h, w, ["smooth", "noise"][(k // 2) % 2], seed=k), [0, 1, 2, "grey"][k % 4],
                            **VARIANTS[k % 6]))
    want_ids, want_probs = engine.classify_jpegs([jpegdec.entropy_decode(d) for d in datas])
    ids, probs, status = engine.classify_jpeg_files([file_item(d) for d in datas])
    assert status.tolist() == [0] * 8
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(probs, want_probs)
    # a refused file in the batch: id -1, zero probabilities, the others undisturbed
    begin = int(jpegdec.scan_probe_rc(datas[2])[1].scan_begin)
    mixed = [file_item(d) for d in datas[:2]] + [file_item(datas[2][:begin + 200])] + [file_item(datas[3])]
    ids, probs, status = engine.classify_jpeg_files(mixed)
    assert status[2] != 0 and ids[2] == -1 and not probs[2].any()
    keep = [0, 1, 3]
    assert not status[keep].any()
    np.testing.assert_array_equal(ids[keep], want_ids[keep])
    np.testing.assert_array_equal(probs[keep], want_probs[keep])


def test_infer_files_with_gpu_huffman_equals_the_host_huffman_path(tmp_path):
    from PIL import Image
    from roomnet_amd.infer import classify_im_dir, groundtruth_validation
    from roomnet_amd.network import RoomNet
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=4, dtype="bf16")
    nn.load(MODEL_PREFIX)
    d = tmp_path / "images"
    os.makedirs(str(d))
    for k in range(6):
        h, w = ((300, 400), (400, 300), (224, 224))[k % 3]
        encode(str(d / ("b%d.jpg" % k)), content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k % 3], **VARIANTS[k % 6])
    encode(str(d / "prog.jpg"), content(300, 400, "smooth", seed=7), 2, quality=90, progressive=True)
    Image.fromarray(content(260, 300, "smooth", seed=8)).save(str(d / "p.png"))
    data = encode(str(d / "cut.jpg"), content(300, 400, "noise", seed=9), 2, quality=90)
    with open(str(d / "cut.jpg"), "wb") as f:               # damaged: the scan stops half way (imread still decodes what is there)
        f.write(data[:len(data) // 2])
    with open(str(d / "junk.jpg"), "wb") as f:
        f.write(b"\xff\xd8 not an image")
    paths = sorted(os.path.join(str(d), f) for f in os.listdir(str(d)))
    want = nn.infer_files(paths, batch_size=4)
    got = nn.infer_files(paths, batch_size=4, gpu_huffman=True)
    assert nn.huffman_fallbacks == 1                        # cut.jpg
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not want[2][[os.path.basename(p) == "junk.jpg" for p in paths]].any() and want[2].sum() >= len(paths) - 2
    with pytest.raises(ValueError):
        classify_im_dir(nn, str(d), overlay=False, gpu_decode=False, gpu_huffman=True)
    with pytest.raises(ValueError):
        groundtruth_validation(nn, str(d / "none.txt"), gpu_decode=False, gpu_huffman=True)
    nn.sess.close()


def test_argument_errors_leave_the_handle_usable(engine, corpus):
    lib, h = engine.lib, engine.handle
    items = [file_item(corpus[k][0]) for k in (3, 64)]
    arr = engine._jpeg_files(items * (MAX_BATCH // 2 + 1))
    outs = [np.zeros(len(corpus[k][1]), np.int16) for k in (3, 64)] * (MAX_BATCH // 2 + 1)
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    status = np.zeros(MAX_BATCH + 2, np.int32)
    probs, ids = np.empty((MAX_BATCH + 2, 6), np.float32), np.empty(MAX_BATCH + 2, np.int64)
    for n in (0, MAX_BATCH + 1):
        assert lib.rn_jpeg_huffman_batch(h, arr, n, ptrs, status.ctypes.data) == RN_E_RANGE
        assert lib.rn_jpeg_huffman_batch_device(h, arr, n, None, status.ctypes.data) == RN_E_RANGE
        assert lib.rn_classify_jpeg_files(h, arr, n, probs.ctypes.data, ids.ctypes.data, status.ctypes.data) == RN_E_RANGE
    arr[1].info.supported = 0
    assert lib.rn_jpeg_huffman_batch(h, arr, 2, ptrs, status.ctypes.data) == RN_E_INVALID
    assert b"not a supported JPEG" in lib.rn_last_error()
    assert lib.rn_classify_jpeg_files(h, arr, 2, probs.ctypes.data, ids.ctypes.data, status.ctypes.data) == RN_E_INVALID
    arr[1].info.supported = 1
    assert lib.rn_jpeg_huffman_batch(h, arr, 2, ptrs, status.ctypes.data) == 0
    assert status[:2].tolist() == [0, 0] and np.array_equal(outs[0], corpus[3][1]) and np.array_equal(outs[1], corpus[64][1])
