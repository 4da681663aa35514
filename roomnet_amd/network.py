"""``RoomNet`` -- drop-in for the reference's ``network.RoomNet`` inference surface
(reference ``network.py:19-244``), executing on an MI355X through
libroomnet_hip.so instead of a TensorFlow session.

Kept from the reference (same names, argument meaning, return shapes/dtypes):
``RoomNet(num_classes, im_side=600, ...)``, attributes ``num_classes``,
``im_side``, ``sess``; ``init()``, ``load(model_path=None)``, ``save(suffix=None)``,
``center_crop(x)``, ``infer(im_batch)``, ``infer_optimized(im)``.
Batch-statistics BN, the forward pass of the reference's default ``compute_bn_mean_var=True`` model, arrives through
``infer_batch_stats`` and ``recalibrate_bn`` (the constructor still refuses the flag: that model is the training graph).
Whole-network training (``train_step``, loss/optimizer graph, ``network.py:49-85,158-170``) is out
of scope and raises ``NotImplementedError``; ``extract_features`` + ``fine_tune`` train the last two or three conv stages and the
dense head on the GPU, from cached ``s7.bn`` (or ``s6.bn``) features.

MI355X-only keyword arguments (not in the reference): ``device``, ``dtype``
("f32" | "bf16" | "f16"), ``max_batch``.
"""
from __future__ import annotations

import os
from glob import glob
from typing import Dict, Optional

import numpy as np

from . import tf_bundle
from ._capi import Engine
from .graph import Graph, build_graph
from .imageops import resize_linear_u8


class _Session:
    """Stand-in for the ``tf.Session`` the reference keeps in ``self.sess``: owns the
    variable values; the device engine is (re)built from them on demand."""

    def __init__(self, variables: Dict[str, np.ndarray]):
        self.variables = variables
        self.engine: Optional[Engine] = None
        self.bs_engine: Optional[Engine] = None      # the float32 batch-statistics engine (infer_batch_stats, recalibrate_bn)

    def close(self) -> None:
        if self.engine is not None:
            self.engine.close()
            self.engine = None
        if self.bs_engine is not None:
            self.bs_engine.close()
            self.bs_engine = None


def _initializer_values(graph: Graph, seed: int = 0) -> Dict[str, np.ndarray]:
    """What ``tf.global_variables_initializer`` produces for this graph
    (``network.py:87-91``): glorot-uniform kernels, zero bias, BN gamma=1, beta=0,
    moving_mean=0, moving_variance=1."""
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    for name, shape in graph.variable_shapes().items():
        leaf = name.rsplit("/", 1)[1]
        if leaf == "kernel":
            if len(shape) == 4:
                fan_in, fan_out = shape[0] * shape[1] * shape[2], shape[0] * shape[1] * shape[3]
            else:
                fan_in, fan_out = shape
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
        elif leaf in ("gamma", "moving_variance"):
            out[name] = np.ones(shape, np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


class _Placeholder:
    """What the reference keeps in ``self.x_tensor`` (``network.py:28``: ``tf.placeholder(tf.float32, [None, S, S, 3],
    name='input_x_tensor')``): there is no TensorFlow graph here, so it is a description -- ``name``, ``shape``, ``dtype`` -- and
    the first entry of ``RoomNet.layers``."""

    def __init__(self, im_side):
        self.name = 'input_x_tensor:0'
        self.shape = [None, im_side, im_side, 3]
        self.dtype = np.float32

    def __repr__(self):
        return "<placeholder %r shape=(?, %d, %d, 3) dtype=float32>" % (self.name, self.shape[1], self.shape[2])


def _layer_names(graph: Graph):
    """``RoomNet.layers`` of the reference (``network.py:30``, ``:207``, ``:222``): the placeholder, then one list per conv_block /
    dense_block with that block's tensors in creation order.  Here the entries are the NAMES the per-layer read-out answers to
    (``RoomNet.tap(name)`` -> ``rn_tap``): ``sK.conv`` (conv + ReLU6), ``sK.pool``, ``sK.bn``, ``sK.add``, ``sK.bn2`` for conv stage K,
    ``dK.mm``, ``dK.relu``, ``dK.bn`` for dense block K.  A conv_block of depth d is d consecutive stages; the block that a stage
    with a skip connection closes started at its skip stage."""
    blocks, cur = [], []
    for s in graph.stages:
        names = ["s%d.conv" % s.index] + (["s%d.pool" % s.index] if s.pool_k else []) + ["s%d.bn" % s.index]
        if s.residual:
            names += ["s%d.add" % s.index, "s%d.bn2" % s.index]
        cur.append((s, names))
    # group: a residual stage ends the block its skip stage began; other stages are blocks of their own unless inside such a span
    i, n = 0, len(cur)
    ends = {s.skip_stage: s.index for s, _ in cur if s.residual}
    while i < n:
        j = ends.get(cur[i][0].index, cur[i][0].index)
        blocks.append([nm for k in range(i, j + 1) for nm in cur[k][1]])
        i = j + 1
    for d in graph.dense:
        blocks.append(["d%d.mm" % d.index, "d%d.relu" % d.index] + (["d%d.bn" % d.index] if d.bn_name else []))
    return blocks


def _huffenc_slot_bytes(info):
    """Bytes of a page-locked output slot of ``classify_files_to_dir(gpu_huffman_encode=True)``: what the image's coefficients
    would take (16 bits per coefficient).  The worst case, ``jpegenc.encoded_bound``, is 3.25 times that and page-locked memory is
    not free; a file beyond its slot gets ``ST_CAP`` and goes through the host pass."""
    from . import jpegdec, jpegenc
    return min(jpegenc.encoded_bound(info), 1024 + 2 * jpegdec.coeff_count(info))


class RoomNet:

    def __init__(self, num_classes, im_side=600, compute_bn_mean_var=True, start_step=0, dropout_enabled=False,
                 learn_rate=1e-4, l2_regularizer_coeff=1e-2, num_steps=10000, dropout_rate=.2,
                 update_batchnorm_means_vars=True, optimized_inference=False, *, device=0, dtype="f32",
                 max_batch=64):
        self.num_classes = num_classes
        self.im_side = im_side
        self.compute_bn_mean_var = compute_bn_mean_var
        self.optimized_inference = optimized_inference
        self.start_step = start_step
        self.step = start_step
        self.learn_rate = learn_rate
        self.l2_regularizer_coeff = l2_regularizer_coeff
        self.num_steps = num_steps
        self.dropout_enabled = False if optimized_inference else dropout_enabled
        self.dropout_rate = dropout_rate          # what fine_tune(..., dropout_rate=nn.dropout_rate) passes on
        self.model_folder = 'all_trained_models/trained_models'
        self.model_fpath_prefix = self.model_folder + '/' + 'roomnet-'
        if compute_bn_mean_var:
            # training=True batch statistics (network.py:193) need the training graph
            raise NotImplementedError("compute_bn_mean_var=True (batch-statistics BN) belongs to the training "
                                      "path, which is out of scope; construct with compute_bn_mean_var=False")
        self.graph = build_graph(num_classes=num_classes, im_side=im_side)
        # network.py:28-30: the input placeholder and the per-block list of layer tensors -- here their descriptions / tap names
        self.x_tensor = _Placeholder(im_side)
        self.layers = [self.x_tensor] + _layer_names(self.graph)
        self.device = device
        self.dtype = dtype
        self.max_batch = max_batch
        self.sess: Optional[_Session] = None
        # variables created by the dense blocks are not restored in training mode
        # (restore_excluded_vars, network.py:242 / :78)
        self._restore_excluded = set()
        if not optimized_inference:
            for d in self.graph.dense:
                self._restore_excluded.add(d.name + "/")
                if d.bn_name:
                    self._restore_excluded.add(d.bn_name + "/")

    # ------------------------------------------------------------- persistence
    def init(self):
        """network.py:87-91."""
        if not self.sess:
            self.sess = _Session(_initializer_values(self.graph))

    def save(self, suffix=None):
        """network.py:93-103 (writes the index + data shard; no .meta graph)."""
        if not self.sess:
            self.init()
        if self.optimized_inference:
            tf_bundle.write_bundle('roomnet', self.sess.variables)
            print('Model Saved in optimized inference mode')
            return
        if suffix:
            save_fpath = self.model_fpath_prefix + '-' + suffix + '--' + str(self.step)
        else:
            save_fpath = self.model_fpath_prefix + '-' + str(self.step)
        tf_bundle.write_bundle(save_fpath, self.sess.variables)
        print('Model saved at', save_fpath)

    def load(self, model_path=None):
        """network.py:105-126."""
        if not self.sess:
            self.init()
        if model_path is None:
            if os.path.isdir(self.model_folder):
                existing_paths = glob(self.model_folder + '/*.index')
                if len(existing_paths) == 0:
                    print('No model found to restore from, initializing random weights')
                    return
                existing_ids = [int(p.split('--')[-1].replace('.index', '')) for p in existing_paths]
                selected_idx = np.argmax(existing_ids)
                self.step = existing_ids[selected_idx]
                self.start_step = self.step
                model_path = existing_paths[selected_idx].replace('.index', '')
            else:
                print('No model found to restore from, initializing random weights')
                return
        reader = tf_bundle.BundleReader(model_path)
        shapes = self.graph.variable_shapes()
        restored = dict(self.sess.variables)
        for name, shape in shapes.items():
            if any(name.startswith(p) for p in self._restore_excluded):
                continue
            if name not in reader:
                raise tf_bundle.BundleError("Key %s not found in checkpoint %r" % (name, model_path))
            val = reader.get(name)
            if tuple(val.shape) != tuple(shape):
                raise ValueError("Assign requires shapes of both tensors to match. lhs shape= %s rhs shape= %s "
                                 "(variable %s; is the checkpoint for im_side=%d?)"
                                 % (list(shape), list(val.shape), name, self.im_side))
            restored[name] = val.astype(np.float32)
        self.sess.close()
        self.sess.variables = restored
        print('Model restored from', model_path)

    def set_variables(self, values: Dict[str, np.ndarray]) -> None:
        """Assign variable values directly (what ``sess.run(tf.assign(...))`` does)."""
        if not self.sess:
            self.init()
        shapes = self.graph.variable_shapes()
        for k, v in values.items():
            if k not in shapes:
                raise KeyError("unknown variable %r" % k)
            if tuple(np.shape(v)) != tuple(shapes[k]):
                raise ValueError("variable %r: shape %s does not match %s" % (k, np.shape(v), shapes[k]))
            self.sess.variables[k] = np.asarray(v, np.float32)
        self.sess.close()

    def _engine(self) -> Engine:
        if not self.sess:
            raise RuntimeError("Attempted to use a closed Session. (call init() or load() first)")
        if self.sess.engine is None:
            self.sess.engine = Engine(self.graph, self.sess.variables, device=self.device, dtype=self.dtype,
                                      max_batch=self.max_batch)
        return self.sess.engine

    def _bs_engine(self) -> Engine:
        """The float32 engine whose BNs normalise with the moments of the batch (``RN_FLAG_BATCH_STATS``), built beside the
        model's own engine from the same variables, whatever ``dtype`` the model has."""
        if not self.sess:
            raise RuntimeError("Attempted to use a closed Session. (call init() or load() first)")
        if self.sess.bs_engine is None:
            self.sess.bs_engine = Engine(self.graph, self.sess.variables, device=self.device, dtype="f32",
                                         max_batch=self.max_batch, batch_stats=True)
        return self.sess.bs_engine

    def tap(self, name, n=1):
        """The per-layer read-out the reference gets from ``sess.run(self.layers[k][j], ...)``: tensor ``name`` (an entry of
        ``self.layers``) of the LAST inference call, float32 ``[n, h, w, c]`` (``rn_tap``).  Float32 engines built with taps hold
        every node; the throughput engines hold the tensors their launches write (RoomNetLibraryError otherwise)."""
        return self._engine().tap(name, n)

    # ----------------------------------------------------------------- inference
    def infer(self, im_in):
        """network.py:128-135: [N,S,S,3] BGR batch already at im_side.  Returns
        ``(argmax int64[N], softmax float32[N,C])`` in optimized mode, ``argmax``
        alone otherwise (``outs_final`` differs: network.py:45 vs :72)."""
        im = np.asarray(im_in)
        if im.ndim != 4 or im.shape[1:] != (self.im_side, self.im_side, 3):
            raise ValueError("Cannot feed value of shape %s for Tensor 'input_x_tensor:0', which has shape "
                             "'(?, %d, %d, 3)'" % (im.shape, self.im_side, self.im_side))
        eng = self._engine()
        im = self._as_feed(im)
        if im.dtype == np.uint8:
            ids, probs = eng.forward_u8(im)
        else:
            # non-uint8 input: same float64 expression as the reference, cast at the feed
            x = (((im[:, :, :, [2, 1, 0]] / 255.) * 2) - 1).astype(np.float32)
            ids, probs = eng.forward_f32(x)
        if self.optimized_inference:
            return ids, probs
        return ids

    def _as_feed(self, im):
        """The reference takes any numeric array (network.py:128-135).  The 16-bit engines fuse the uint8 ->
        [-1, 1] table into their first kernel and only take uint8: integral-valued arrays in [0, 255] are cast
        (same values, same table), anything else is refused here with the reason instead of a library error."""
        if im.dtype == np.uint8 or self.dtype == "f32":
            return im
        if im.size and (np.issubdtype(im.dtype, np.integer) or bool(np.all(im == np.rint(im)))) \
                and im.min() >= 0 and im.max() <= 255:
            return im.astype(np.uint8)
        raise ValueError("RoomNet(dtype=%r) takes uint8 images (or integral values in [0, 255]); got %s with "
                         "non-integral or out-of-range values -- construct with dtype='f32' for float feeds"
                         % (self.dtype, im.dtype))

    def center_crop(self, x):
        """network.py:137-146."""
        h, w, _ = x.shape
        offset = abs((w - h) // 2)
        if h < w:
            x_pp = x[:, offset:offset + h, :]
        elif w < h:
            x_pp = x[offset:offset + w, :, :]
        else:
            x_pp = x.copy()
        return x_pp

    def infer_optimized(self, im_in):
        """network.py:148-156: one BGR HWC image of any size -> ``(idx[1], conf[1,C])``."""
        eng = self._engine()
        if isinstance(im_in, np.ndarray) and im_in.dtype == np.uint8 and im_in.ndim == 3 and im_in.shape[2] == 3:
            # crop + cv2.resize restatement on the GPU (rn_classify_images_u8): bit-identical to the host path below
            return eng.classify_images([im_in])
        im = self.center_crop(im_in)
        h, w, _ = im.shape
        if h != self.im_side or w != self.im_side:
            im = resize_linear_u8(im, self.im_side, self.im_side)
        im = self._as_feed(np.ascontiguousarray(im))
        if im.dtype == np.uint8:
            out_label_idx, out_label_conf = eng.forward_u8(im[None])
        else:
            x = (((im[:, :, [2, 1, 0]] / 255.) * 2) - 1).astype(np.float32)
            out_label_idx, out_label_conf = eng.forward_f32(x[None])
        return out_label_idx, out_label_conf

    def infer_images(self, images):
        """Batched ``infer_optimized``: a list of BGR HWC images of ANY size -> what ``infer`` returns for the batch of
        their centre-cropped, resized versions (network.py:149-152 per image, then network.py:128-135).  3-channel
        uint8 images -- what ``cv2.imread`` yields -- go to the GPU as they are: crop + INTER_LINEAR resize run there
        (``rn_classify_images_u8``, byte for byte the host restatement); anything else is prepared on the host.  Not
        in the reference (its caller loops over ``infer_optimized``, infer.py:79-82); the directory drivers use it."""
        images = list(images)
        if not images:
            empty = np.zeros((0,), np.int64), np.zeros((0, self.num_classes), np.float32)
            return empty if self.optimized_inference else empty[0]
        if all(isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 for im in images):
            ids, probs = self._engine().classify_images(images)
            return (ids, probs) if self.optimized_inference else ids
        prepared = []
        for im in images:
            im = self.center_crop(np.asarray(im))
            if im.shape[0] != self.im_side or im.shape[1] != self.im_side:
                im = resize_linear_u8(np.ascontiguousarray(im), self.im_side, self.im_side)
            prepared.append(np.ascontiguousarray(im))
        return self.infer(np.stack(prepared, 0))

    def infer_files(self, paths, decode_threads=None, batch_size=64, gpu_huffman=False, gpu_orient=False):
        """Classify image FILES, decoding baseline JPEG on the GPU: ``(ids int64[N], probs float32[N,C], ok bool[N])`` in list
        order; ``ok[i]`` False (id -1, zero probabilities) marks a file that is not a readable image.  A pool of
        ``decode_threads`` threads (default ``infer.DECODE_THREADS``, at most 16) reads each file, walks its markers and runs its
        Huffman pass into a ring of reused page-locked buffers (``roomnet_amd.jpegdec``); dequantisation, inverse DCT, chroma
        upsampling, colour conversion, crop, resize and the forward pass run on the GPU, ``batch_size`` files (at most
        ``max_batch``) per call (``rn_classify_jpegs``) while the pool works on the next batch.  Files the split decoder does
        not take -- progressive, CMYK, with an EXIF orientation other than 1 (unless ``gpu_orient``), damaged, not JPEG at all --
        are decoded by ``imageio.imread`` on the same pool and classified by ``infer_images`` in the same call.  Every result equals ``infer_images`` of the ``imread``
        images bit for bit.  Not in the reference (infer.py:79-82 decodes with ``cv2.imread``).

        ``gpu_huffman``: the Huffman pass runs on the GPU as well.  The pool then only reads each file
        into page-locked memory and walks its markers; the file's bytes go up as they are (``rn_classify_jpeg_files``).  A file
        whose status comes back non-zero is decoded by the host's Huffman pass on the same pool and classified in the same call
        (``self.huffman_fallbacks`` counts them); the results are the same bits either way.

        ``gpu_orient``: files with an EXIF orientation of 2..8 -- what a phone held upright writes -- go through the split decoder
        too: the pool reads the orientation (``rn_jpeg_probe_oriented``), the coefficients stay those of the
        stored image, and the store of the GPU's colour kernel turns the pixels.  The same bits as ``imread``'s turned image.

        After the call ``self.last_decode_paths`` holds how many files took which way: ``"jpeg"`` (split decoder, Huffman pass on
        the host), ``"file"`` (split decoder, Huffman pass on the GPU), ``"image"`` (``imread``) and ``"unreadable"``."""
        paths = list(paths)
        n = len(paths)
        ids = np.full((n,), -1, np.int64)
        probs = np.zeros((n, self.num_classes), np.float32)
        ok = np.zeros((n,), bool)
        eng = self._engine() if n else None
        self.huffman_fallbacks = 0
        self.last_decode_paths = self._new_decode_paths()
        for lo, loaded, pool in self._file_chunks(paths, batch_size, decode_threads, gpu_huffman=gpu_huffman, gpu_orient=gpu_orient):
            taken = 0
            if gpu_huffman:
                before = self.last_decode_paths["file"]
                loaded = self._classify_file_bytes(eng, paths, lo, loaded, pool, ids, probs, ok, gpu_orient)
                taken = self.last_decode_paths["file"] - before
            self._count_decode_paths(loaded, taken)
            jp = [(lo + j, r) for j, r in enumerate(loaded) if r is not None and r[0] == "jpeg"]
            im = [(lo + j, r) for j, r in enumerate(loaded) if r is not None and r[0] == "image"]
            if jp:
                a, b = eng.classify_jpegs([(r[1], r[2]) for _i, r in jp])
                at = [i for i, _r in jp]
                ids[at], probs[at], ok[at] = a, b, True
            if im:
                a, b = eng.classify_images([r[1] for _i, r in im])
                at = [i for i, _r in im]
                ids[at], probs[at], ok[at] = a, b, True
        return ids, probs, ok

    @staticmethod
    def _new_decode_paths():
        return {"jpeg": 0, "file": 0, "image": 0, "unreadable": 0}

    def _count_decode_paths(self, loaded, taken=0):
        """Add a chunk of loader results to ``self.last_decode_paths``; ``taken`` of its None entries are files
        ``_classify_file_bytes`` classified and counted."""
        for r in loaded:
            self.last_decode_paths["unreadable" if r is None else r[0]] += 1
        self.last_decode_paths["unreadable"] -= taken

    def _classify_file_bytes(self, eng, paths, lo, loaded, pool, ids, probs, ok, gpu_orient=False):
        """The ``gpu_huffman`` half of ``infer_files`` for one chunk of ``jpegdec.load_file_bytes`` results: the ``"file"`` entries
        are classified from their bytes (``rn_classify_jpeg_files``) and their results stored; returns the chunk with them taken
        out (None in their place, already counted) and every file whose status is not 0 replaced by what ``jpegdec.load_file``
        gives for it -- the host's Huffman pass, run on the same pool -- for the caller to classify as before."""
        from . import jpegdec
        loaded = list(loaded)
        fl = [(j, r) for j, r in enumerate(loaded) if r is not None and r[0] == "file"]
        if not fl:
            return loaded
        a, b, status = eng.classify_jpeg_files([(r[1], r[2], r[3]) for _j, r in fl])
        good = [k for k in range(len(fl)) if status[k] == 0]
        at = [lo + fl[k][0] for k in good]
        if good:
            ids[at], probs[at], ok[at] = a[good], b[good], True
            self.last_decode_paths["file"] += len(good)
        for j, _r in fl:
            loaded[j] = None
        again = [fl[k][0] for k in range(len(fl)) if status[k] != 0]
        self.huffman_fallbacks += len(again)
        # (the coefficient ring is free in this mode: the slots of the chunk's first bank take the fallbacks)
        futures = [(j, pool.submit(jpegdec.load_file, paths[lo + j], self._jpeg_ring, j, gpu_orient)) for j in again]
        for j, f in futures:
            loaded[j] = f.result()
        return loaded

    def _file_chunks(self, paths, batch_size, decode_threads=None, gpu_huffman=None, gpu_orient=False):
        """Yield ``(lo, [jpegdec.load_file result of paths[lo + j]])`` chunk by chunk (``batch_size``, at most ``max_batch``, files
        each): the pool decodes chunk k + 1 into the other half of the coefficient ring while the consumer works on chunk k.  A
        chunk's coefficient buffers are valid until the consumer asks for the next chunk.  ``gpu_huffman`` not None (``infer_files``):
        yields ``(lo, results, pool)``, and when it is true the results are ``jpegdec.load_file_bytes``'s, in a ring of byte buffers.
        ``gpu_orient``: the loaders run with ``orient=True``."""
        from concurrent.futures import ThreadPoolExecutor
        from . import jpegdec
        from .infer import DECODE_THREADS
        n = len(paths)
        if not n:
            return
        chunk = max(1, min(int(batch_size), self._engine().max_batch))
        nthreads = max(1, min(16, int(decode_threads or DECODE_THREADS)))
        ring = getattr(self, "_jpeg_ring", None)
        if ring is None or len(ring) < 2 * chunk:
            if ring is not None:
                ring.close()
            ring = self._jpeg_ring = jpegdec.CoeffRing(2 * chunk)
        loader = jpegdec.load_file
        if gpu_huffman:
            ring = getattr(self, "_jpeg_byte_ring", None)
            if ring is None or len(ring) < 2 * chunk:
                if ring is not None:
                    ring.close()
                ring = self._jpeg_byte_ring = jpegdec.ByteRing(2 * chunk)
            loader = jpegdec.load_file_bytes
        orient = (True,) if gpu_orient else ()
        n_chunks = (n + chunk - 1) // chunk
        with ThreadPoolExecutor(max_workers=nthreads) as pool:
            def submit(k):
                # chunk k decodes into bank k % 2 of the ring: that bank was chunk k - 2's, which the consumer was done with when it asked for chunk k - 1
                lo = k * chunk
                return [pool.submit(loader, paths[i], ring, (k % 2) * chunk + i - lo, *orient) for i in range(lo, min(n, lo + chunk))]
            ahead = submit(0)
            for k in range(n_chunks):
                cur, ahead = ahead, (submit(k + 1) if k + 1 < n_chunks else [])
                res = [f.result() for f in cur]
                yield (k * chunk, res) if gpu_huffman is None else (k * chunk, res, pool)

    def classify_files_to_dir(self, paths, out_path_of, lines_of, writers, decode_threads=None, batch_size=64, heatmap=None,
                              heatmap_weight=0.5, gpu_huffman_encode=False, gpu_orient=False, occlusion_patch=32, occlusion_stride=16):
        """Classify image FILES and write each with its overlay as a JPEG file, decode to encode on the GPU.  Yields, in list
        order, ``(index, id, conf, image, future)``: ``future`` is the pending write (on the ``writers`` pool) of a file that went
        through the device; ``image`` (BGR) is set instead for a file whose output name ``out_path_of(index, id)`` has no JPEG
        extension -- the caller writes those; an unreadable file yields ``(index, None, None, None, None)``.

        Per chunk of ``batch_size`` files (at most ``max_batch``): the pool of ``_file_chunks`` runs the Huffman pass of baseline
        JPEG files (others are decoded by ``imageio.imread`` and uploaded), the GPU decodes, crops, resizes and classifies
        (``Engine.classify_resident``: the bits of ``infer_files``), the text lines ``lines_of(h, w, id, conf)`` -- ``put_text``
        argument tuples -- are rasterised to coverages on the ``writers`` pool, the GPU draws them and runs the encode's pixel
        stage (``rn_jpeg_encode_batch_device``), and the ``writers`` pool runs the Huffman pass of the output and writes the
        file while the GPU works on the next chunk.  The coefficients come back into a second ring of page-locked buffers,
        two banks like the decode's; a bank is reused once its files are written.  The full-size image never exists on the host.
        Every file equals ``imageio.imwrite`` of the ``put_text`` image byte for byte.

        ``heatmap`` ("s6.bn" or "s7.bn"; None: off): each file also gets the grad-CAM map of its predicted class, drawn on the
        square the network saw with ``heatmap_weight``, UNDER the text.  The chunk then runs ``Engine.explain_resident`` (the
        forward pass and its adjoint; the same ids and confidences) and ``Engine.cam_overlay_batch`` in front of the text and the
        encode, all on the device; a file the caller writes comes back with its heat map drawn on the host (``grad_cam``,
        ``cam.overlay_image``: the same bytes).  ``heatmap="occlusion"`` draws the occlusion-sensitivity map of the predicted class
        instead (``occlusion_patch``, ``occlusion_stride``, mean fill): the chunk runs
        ``Engine.occlusion_resident`` -- pass 0 gives the same ids and confidences, the masked passes and the ``S x S`` map stay on the
        device -- and the same ``Engine.cam_overlay_batch``; the host way is ``occlusion_map`` and ``cam.overlay_image``.

        ``gpu_huffman_encode``: the Huffman pass of the OUTPUT runs on the GPU as well (``Engine.jpeg_encode_files``, DESIGN.md
        section 19): no coefficient leaves the device, the files arrive in a ring of page-locked byte buffers (two banks, the
        same reuse rule) and the ``writers`` pool only writes ``buf[:len]``.  A file whose status is not 0 (in practice: one larger than its slot of 2 bytes per coefficient) is encoded again in
        the same call through ``jpeg_encode_batch`` -- WITHOUT overlays where the first call drew them (they are in the image already),
        with them for a ``ST_TOO_LARGE`` image, for which nothing was enqueued -- and
        ``jpegenc.entropy_encode``; ``self.huffenc_fallbacks`` counts those.  The same bytes.

        ``gpu_orient``: files with an EXIF orientation of 2..8 are decoded -- and turned -- on the GPU too
        instead of by ``imread``; everything behind the decode starts from the upright image either way.  The same bytes.
        ``self.last_decode_paths`` counts the ways the files took, as after ``infer_files``."""
        import os
        from . import cam, hershey, jpegdec, jpegenc
        from ._capi import GRAD_CAM_LAYERS
        if heatmap is not None and heatmap != "occlusion" and heatmap not in GRAD_CAM_LAYERS:
            raise ValueError("classify_files_to_dir: heatmap must be None, 'occlusion' or one of %s, got %r" % (GRAD_CAM_LAYERS, heatmap))
        if not 0.0 <= heatmap_weight <= 1.0:
            raise ValueError("classify_files_to_dir: heatmap_weight must be in [0, 1]")
        paths = list(paths)
        if not paths:
            return
        eng = self._engine()
        chunk = max(1, min(int(batch_size), eng.max_batch))
        ring = getattr(self, "_jpeg_enc_ring", None)
        if ring is None or len(ring) < 2 * chunk:
            if ring is not None:
                ring.close()
            ring = self._jpeg_enc_ring = jpegdec.CoeffRing(2 * chunk)
        out_ring = None
        if gpu_huffman_encode:
            out_ring = getattr(self, "_jpeg_out_ring", None)
            if out_ring is None or len(out_ring) < 2 * chunk:
                if out_ring is not None:
                    out_ring.close()
                out_ring = self._jpeg_out_ring = jpegdec.ByteRing(2 * chunk)
            self.huffenc_fallbacks = 0
        pending = [[], []]                      # the writes that still read each bank's buffers
        self.last_decode_paths = self._new_decode_paths()

        def write(info, coeffs, out_path):
            try:
                data = jpegenc.entropy_encode(info, coeffs)
                with open(out_path, "wb") as f:
                    f.write(data)
            except (OSError, ValueError):
                return False
            return True

        def write_bytes(buf, n, out_path):
            try:
                with open(out_path, "wb") as f:
                    f.write(buf[:n])
            except OSError:
                return False
            return True

        def rasterise(shape, lines):
            boxes = [(hershey.coverage(text, org, scale, shape, 1), color) for text, org, scale, color in lines]
            return [(b[0], b[1], b[2], color) for b, color in boxes if b is not None]

        for k, (lo, loaded) in enumerate(self._file_chunks(paths, chunk, decode_threads, gpu_orient=gpu_orient)):
            bank = k % 2
            self._count_decode_paths(loaded)
            for f in pending[bank]:
                f.result()
            pending[bank] = []
            jp = [j for j, r in enumerate(loaded) if r is not None and r[0] == "jpeg"]
            up = [j for j, r in enumerate(loaded) if r is not None and r[0] == "image"
                  and os.path.splitext(paths[lo + j])[1].lower() in jpegenc.JPEG_EXTENSIONS]
            host = [j for j, r in enumerate(loaded) if r is not None and r[0] == "image" and j not in up]
            out = {}
            if jp or up:
                staged = [(loaded[j][1], loaded[j][2]) for j in jp], [loaded[j][1] for j in up]
                if heatmap is None:
                    ids, probs, addrs, shapes = eng.classify_resident(*staged)
                else:
                    if heatmap == "occlusion":
                        ids, probs, addrs, shapes, d_cams, map_shape = eng.occlusion_resident(*staged, occlusion_patch, occlusion_stride)
                    else:
                        ids, probs, addrs, shapes, d_cams, map_shape = eng.explain_resident(*staged, heatmap)
                    eng.cam_overlay_batch([(addrs[m], shapes[m], d_cams[m], map_shape) for m in range(len(addrs))], heatmap_weight)
                confs = [probs[m][ids[m]] for m in range(len(ids))]
                overlays = list(writers.map(rasterise, shapes, [lines_of(h, w, int(ids[m]), confs[m]) for m, (h, w) in enumerate(shapes)]))
                infos = [jpegenc.encode_info(h, w) for h, w in shapes]
                host_pass = list(range(len(infos)))          # the files whose Huffman pass the writer pool runs
                if gpu_huffman_encode:
                    files = [out_ring.buffer(bank * chunk + m, _huffenc_slot_bytes(info)) for m, info in enumerate(infos)]
                    lens, status = eng.jpeg_encode_files([(addrs[m], infos[m], overlays[m], None) for m in range(len(infos))], files)
                    host_pass = [m for m in range(len(infos)) if status[m] != 0]
                    self.huffenc_fallbacks += len(host_pass)
                    # the call drew the overlays of every image it enqueued: those images hold them.  An image that is too
                    # large got no launch at all, so its lines are still to be drawn
                    overlays = [ov if status[m] == jpegenc.ST_TOO_LARGE else [] for m, ov in enumerate(overlays)]
                if host_pass:
                    bufs = {m: ring.buffer(bank * chunk + m, jpegdec.coeff_count(infos[m])) for m in host_pass}
                    eng.jpeg_encode_batch([(addrs[m], infos[m], overlays[m], bufs[m]) for m in host_pass])
                    eng.sync()
                for m, j in enumerate(jp + up):
                    if m in host_pass:
                        fut = writers.submit(write, infos[m], bufs[m], out_path_of(lo + j, int(ids[m])))
                    else:
                        fut = writers.submit(write_bytes, files[m], lens[m], out_path_of(lo + j, int(ids[m])))
                    pending[bank].append(fut)
                    out[j] = (int(ids[m]), confs[m], None, fut)
            if host and heatmap is None:
                ids, probs = eng.classify_images([loaded[j][1] for j in host])
                for m, j in enumerate(host):
                    out[j] = (int(ids[m]), probs[m][ids[m]], loaded[j][1], None)
            elif host:
                if heatmap == "occlusion":
                    cams, _drops, ids, probs = self.occlusion_map([loaded[j][1] for j in host], patch=occlusion_patch, stride=occlusion_stride)
                else:
                    cams, ids, probs = self.grad_cam([loaded[j][1] for j in host], layer=heatmap)
                for m, j in enumerate(host):
                    out[j] = (int(ids[m]), probs[m][ids[m]], cam.overlay_image(loaded[j][1], cams[m], heatmap_weight), None)
            for j in range(len(loaded)):
                yield (lo + j,) + out.get(j, (None, None, None, None))

    def prepare_files(self, paths, decode_threads=None, batch_size=64, gpu_orient=False):
        """Image files -> the batches ``infer`` takes, decoding baseline JPEG on the GPU: yields ``(indices, batch, unreadable)`` per
        chunk of ``batch_size`` files: ``batch`` the uint8 BGR ``[m, S, S, 3]`` centre-cropped, resized images of the readable files
        ``paths[indices]``, ``unreadable`` the indices of the chunk's files that are no readable image -- byte for byte ``center_crop`` + the ``cv2.resize`` restatement of their ``imread`` images.  JPEG
        files the split decoder takes become pixels, are cropped and resized on the GPU and only the ``S x S`` result comes back;
        other files are prepared on the host.  For the callers that need a batch and not a classification: ``recalibrate_bn``
        (its statistics are the whole batch's) and ``extract_features``.  ``gpu_orient``: files with an EXIF orientation of 2..8
        are among those the split decoder takes; the same bytes.  ``self.last_decode_paths`` counts the
        ways the files took, as after ``infer_files``."""
        eng = self._engine() if len(paths) else None
        self.last_decode_paths = self._new_decode_paths()
        for lo, loaded in self._file_chunks(list(paths), batch_size, decode_threads, gpu_orient=gpu_orient):
            self._count_decode_paths(loaded)
            at = [lo + j for j, r in enumerate(loaded) if r is not None]
            bad = [lo + j for j, r in enumerate(loaded) if r is None]
            if not at:
                yield at, np.zeros((0, self.im_side, self.im_side, 3), np.uint8), bad
                continue
            batch = np.empty((len(at), self.im_side, self.im_side, 3), np.uint8)
            live = [r for r in loaded if r is not None]
            jp = [k for k, r in enumerate(live) if r[0] == "jpeg"]
            if jp:
                batch[jp] = eng.jpegs_to_batch([(live[k][1], live[k][2]) for k in jp])
            for k, r in enumerate(live):
                if r[0] == "image":
                    batch[k] = self._batch_from([r[1]], "prepare_files")[0]
            yield at, batch, bad

    def grad_cam(self, im_in, class_ids=None, layer="s6.bn"):
        """Grad-CAM class-evidence maps (not in the reference): where in each image the network saw its class.
        ``im_in`` is an ``[N,S,S,3]`` BGR batch (the feed rules of ``infer``), or one BGR ``[H,W,3]`` image or a list of
        them, of any size (centre-cropped and resized exactly as ``infer_images`` does).  ``class_ids``: the class per image to explain
        (None: each image's argmax); ``layer``: "s6.bn" (46 x 46 at 224) or "s7.bn" (21 x 21).  Returns ``(cams [N,h,w]
        float32, not normalised, ids int64[N], probs float32[N,C])``; ``roomnet_amd.cam`` upsamples and overlays a map.
        The score is the last dense layer's pre-ReLU6 logit (include/roomnet_hip.h, grad-CAM)."""
        from ._capi import GRAD_CAM_LAYERS
        if layer not in GRAD_CAM_LAYERS:
            raise ValueError("grad_cam: layer must be one of %s, got %r" % (GRAD_CAM_LAYERS, layer))
        if isinstance(im_in, np.ndarray) and im_in.ndim == 3:
            im_in = [im_in]                                   # one HWC image: a batch of one
        if isinstance(im_in, np.ndarray) and im_in.ndim == 4:
            im = im_in
            if im.shape[1:] != (self.im_side, self.im_side, 3):
                raise ValueError("Cannot feed value of shape %s for Tensor 'input_x_tensor:0', which has shape "
                                 "'(?, %d, %d, 3)'" % (im.shape, self.im_side, self.im_side))
        elif isinstance(im_in, np.ndarray):
            raise ValueError("grad_cam: expected an [N,S,S,3] batch, one [H,W,3] image or a list of images, got shape %s"
                             % (im_in.shape,))
        else:
            prepared = []
            for one in im_in:
                one = np.asarray(one)
                if one.ndim != 3 or one.shape[2] != 3:
                    raise ValueError("grad_cam: expected [H,W,3] BGR images, got shape %s" % (one.shape,))
                one = self.center_crop(one)
                if one.shape[0] != self.im_side or one.shape[1] != self.im_side:
                    one = resize_linear_u8(np.ascontiguousarray(one, dtype=np.uint8), self.im_side, self.im_side)
                prepared.append(np.ascontiguousarray(one))
            if not prepared:
                raise ValueError("grad_cam: no images")
            im = np.stack(prepared, 0)
        eng = self._engine()
        im = self._as_feed(im)
        if im.dtype == np.uint8:
            cams, ids, probs = eng.grad_cam(im, class_ids=class_ids, layer=layer)
        else:
            x = (((im[:, :, :, [2, 1, 0]] / 255.) * 2) - 1).astype(np.float32)
            cams, ids, probs = eng.grad_cam(x, class_ids=class_ids, layer=layer)
        return cams, ids, probs

    def occlusion_map(self, im_in, class_ids=None, patch=32, stride=16, fill="mean"):
        """Occlusion-sensitivity maps (not in the reference): how far each image's class probability falls when a ``patch x patch``
        square of the network's input, slid by ``stride``, is covered with ``fill`` ("mean": the image's own mean colour, or a BGR
        triple) -- an input-resolution map from forward passes alone (``roomnet_amd.occlusion`` states the definition).  ``im_in``
        as ``grad_cam`` takes it (uint8 values); ``class_ids``: the class per image (None: each image's argmax).  Returns
        ``(maps [N,S,S] float32, drops [N,G,G] float32, ids int64[N], probs float32[N,C])``; negative entries (covering the square
        RAISED the probability) are kept, ``roomnet_amd.cam.overlay_image`` clips them."""
        if isinstance(im_in, np.ndarray) and im_in.ndim == 3:
            im_in = [im_in]                                   # one HWC image: a batch of one
        if isinstance(im_in, np.ndarray) and im_in.ndim != 4:
            raise ValueError("occlusion_map: expected an [N,S,S,3] batch, one [H,W,3] image or a list of images, got shape %s"
                             % (im_in.shape,))
        im = self._as_feed(np.asarray(self._batch_from(im_in, "occlusion_map")))
        if im.dtype != np.uint8:
            raise ValueError("occlusion_map: the squares are cut out of the uint8 input; got %s" % im.dtype)
        return self._engine().occlusion_u8(im, class_ids=class_ids, patch=patch, stride=stride, fill=fill)

    def map_faithfulness(self, im_in, maps, class_ids=None, steps=32, modes=("deletion", "insertion"), fill="mean"):
        """Deletion and insertion curves of heat maps (not in the reference): which map to believe.  Per image the pixels are ranked
        by ``maps`` (highest first, ties in raster order); the deletion curve is the class probability with the top ``j / steps`` of
        them replaced by ``fill`` ("mean": the image's own mean colour, or a BGR triple), ``j = 0 .. steps``, the insertion curve the
        probability with only those pixels present.  A map that points at the evidence gives a SMALL deletion area and a LARGE
        insertion area (``roomnet_amd.faithfulness`` states the definition; ``rn_faith_u8`` runs it on the GPU).  ``im_in`` as
        ``occlusion_map`` takes it (uint8 values); ``maps`` one map per image, ``[N,h,w]`` of any values, e.g. ``grad_cam``'s or
        ``occlusion_map``'s; ``class_ids``: the class per image (None: each image's argmax).  Maps that are not ``S x S`` go through
        ``cam.upsample(maps, S)`` first: bilinear, positive part, scaled to [0, 1] -- order-preserving up to its own rounding, and
        every negative entry joins the zero plateau, which then ranks in raster order.  Returns ``(curves [N,M,steps+1] float32,
        aucs [N,M] float32, ids int64[N], probs float32[N,C])``, ``M`` curves in the order deletion, insertion."""
        from . import cam
        if isinstance(im_in, np.ndarray) and im_in.ndim == 3:
            im_in = [im_in]                                   # one HWC image: a batch of one
        if isinstance(im_in, np.ndarray) and im_in.ndim != 4:
            raise ValueError("map_faithfulness: expected an [N,S,S,3] batch, one [H,W,3] image or a list of images, got shape %s"
                             % (im_in.shape,))
        im = self._as_feed(np.asarray(self._batch_from(im_in, "map_faithfulness")))
        if im.dtype != np.uint8:
            raise ValueError("map_faithfulness: the pixels are replaced in the uint8 input; got %s" % im.dtype)
        maps = np.asarray(maps, np.float32)
        if maps.ndim == 2:
            maps = maps[None]
        if maps.ndim != 3 or maps.shape[0] != im.shape[0]:
            raise ValueError("map_faithfulness: expected one [h,w] map per image (%d), got shape %s" % (im.shape[0], maps.shape))
        if maps.shape[1:] != (self.im_side, self.im_side):
            maps = cam.upsample(maps, self.im_side)
        return self._engine().faith_u8(im, maps, class_ids=class_ids, steps=steps, modes=modes, fill=fill)

    # ------------------------------------------------------ batch-statistics BN
    def _batch_from(self, im_in, who):
        """``[N,S,S,3]`` array as it is (the feed rules of ``infer``); a list of BGR ``[H,W,3]`` images of any size through
        ``center_crop`` + the ``cv2.resize`` restatement, as ``infer_images`` prepares them."""
        if isinstance(im_in, np.ndarray):
            if im_in.ndim != 4 or im_in.shape[1:] != (self.im_side, self.im_side, 3):
                raise ValueError("Cannot feed value of shape %s for Tensor 'input_x_tensor:0', which has shape "
                                 "'(?, %d, %d, 3)'" % (im_in.shape, self.im_side, self.im_side))
            return im_in
        prepared = []
        for one in im_in:
            one = np.asarray(one)
            if one.ndim != 3 or one.shape[2] != 3:
                raise ValueError("%s: expected [H,W,3] BGR images, got shape %s" % (who, one.shape))
            one = self.center_crop(one)
            if one.shape[0] != self.im_side or one.shape[1] != self.im_side:
                one = resize_linear_u8(np.ascontiguousarray(one, dtype=np.uint8), self.im_side, self.im_side)
            prepared.append(np.ascontiguousarray(one))
        if not prepared:
            raise ValueError("%s: no images" % who)
        return np.stack(prepared, 0)

    def _forward_batch_stats(self, im):
        eng = self._bs_engine()
        if im.shape[0] > eng.max_batch:
            raise ValueError("a batch-statistics pass normalises over the WHOLE batch: %d images exceed max_batch=%d "
                             "(construct with a larger max_batch)" % (im.shape[0], eng.max_batch))
        if im.dtype == np.uint8:
            return eng.forward_u8(im)
        x = (((im[:, :, :, [2, 1, 0]] / 255.) * 2) - 1).astype(np.float32)
        return eng.forward_f32(x)

    def infer_batch_stats(self, im_in):
        """``infer`` of a model the reference builds with its default ``compute_bn_mean_var=True``: every BN normalises with
        the moments of THIS batch (network.py:193, :202, :217) instead of the checkpoint's moving statistics, so each row
        of the result depends on the whole batch.  Same feed rules and return convention as ``infer``; runs in float32 on the
        batch-statistics engine whatever ``dtype`` the model has; the batch must fit ``max_batch``.  ``bn_batch_stats()`` of
        that engine then holds the moments."""
        im = np.asarray(im_in)
        if im.ndim != 4 or im.shape[1:] != (self.im_side, self.im_side, 3):
            raise ValueError("Cannot feed value of shape %s for Tensor 'input_x_tensor:0', which has shape "
                             "'(?, %d, %d, 3)'" % (im.shape, self.im_side, self.im_side))
        ids, probs = self._forward_batch_stats(im)
        if self.optimized_inference:
            return ids, probs
        return ids

    def recalibrate_bn(self, batches, momentum=0.99):
        """Re-estimate the moving statistics of all 16 BNs from data, without gradients (AdaBN; also what a fresh ``init()``
        or retrained model needs before ``infer`` means anything).  ``batches``: an iterable of ``[N,S,S,3]`` BGR batches,
        or of lists of BGR images of any size.  Each batch takes one batch-statistics forward pass on the GPU; then all 32
        ``moving_*`` variables are updated on the host (``roomnet_amd.bnstats``): with a number for ``momentum`` by the
        reference's rule, batch after batch (network.py:64-67; ``tf.layers`` default 0.99); with ``momentum=None`` they
        BECOME the equal-weight average of the per-batch moments.  The forward passes all run with the statistics-free
        batch normalisation, so the order of the batches only matters through the momentum rule.  Updates
        ``sess.variables`` and closes the engines (the next ``infer`` builds its engine on the new statistics); returns
        ``{variable name: new value}`` for the 32 variables.  An empty iterable raises ``ValueError``."""
        from . import bnstats
        if not self.sess:
            self.init()
        seen = []
        for batch in batches:
            im = self._batch_from(batch, "recalibrate_bn")
            self._forward_batch_stats(im)
            seen.append(self._bs_engine().bn_batch_stats())
        if not seen:
            raise ValueError("recalibrate_bn: no batches")
        new = bnstats.updated_statistics(self.graph, self.sess.variables, seen, momentum)
        self.set_variables(new)
        return new

    # ------------------------------------------------------------ fine-tuning
    def extract_features(self, im_in, depth=2):
        """The features ``fine_tune`` trains on: ``s7.bn``, the output of the last block's first step (21 x 21 x 16 at 224, 68 x 68 x
        16 at 600), of every image as float32 ``[N, S7, S7, 16]`` (``rn_features_u8``).  ``depth=3``: ``s6.bn``, the input of the
        last block (46 x 46 x 128 at 224, 140 x 140 x 128 at 600), for training the whole block, stage 7 included
        (``rn_features_depth_u8``); that cache costs 1.08 MB per image at 224, against 28 KB at depth 2.
        ``im_in`` as ``grad_cam`` takes it: an
        ``[N,S,S,3]`` BGR batch, one BGR ``[H,W,3]`` image, or a list of images of any size (centre-cropped and resized as
        ``infer_images`` does).  Everything behind these features depends on them alone, so a training set is extracted once."""
        from . import finetune
        depth = finetune._checked_depth(depth)
        if isinstance(im_in, np.ndarray) and im_in.ndim == 3:
            im_in = [im_in]
        if isinstance(im_in, np.ndarray) and im_in.ndim != 4:
            raise ValueError("extract_features: expected an [N,S,S,3] batch, one [H,W,3] image or a list of images, got shape %s"
                             % (im_in.shape,))
        im = self._as_feed(self._batch_from(im_in, "extract_features"))
        if im.dtype != np.uint8:
            if im.size and bool(np.all(im == np.rint(im))) and im.min() >= 0 and im.max() <= 255:
                im = im.astype(np.uint8)
            else:
                raise ValueError("extract_features takes uint8 images (or integral values in [0, 255]), got %s" % im.dtype)
        return self._engine().features_u8(im, depth=depth)

    def _fine_tune_checked(self, who, keep, val_every, val, dropout_rate):
        """The argument rules ``fine_tune`` and ``fine_tune_views`` share, before a device is touched; returns the dropout rate as a
        float (or None)."""
        if keep not in ("last", "best"):
            raise ValueError("%s: keep = %r is neither 'last' nor 'best'" % (who, keep))
        if val_every is not None:
            if isinstance(val_every, bool) or not isinstance(val_every, (int, np.integer)) or val_every < 1:
                raise ValueError("%s: val_every = %r is not a positive number of steps" % (who, val_every))
            if val is None:
                raise ValueError("%s: val_every = %d needs a validation set: pass val=(features, labels)" % (who, val_every))
        elif keep == "best":
            raise ValueError("%s: keep='best' needs validation points: pass val= and val_every=" % who)
        if dropout_rate is None:
            if self.dropout_enabled:
                raise ValueError("%s: dropout on the GPU path covers the sites at or behind the cached feature only and is "
                                 "asked for explicitly: pass dropout_rate= (e.g. dropout_rate=nn.dropout_rate), or construct "
                                 "with dropout_enabled=False" % who)
        else:
            try:
                dropout_rate = float(dropout_rate)
            except (TypeError, ValueError):
                raise ValueError("%s: dropout_rate = %r is not a number" % (who, dropout_rate)) from None
            if not (0.0 <= dropout_rate < 1.0):
                raise ValueError("%s: dropout_rate = %r outside [0, 1)" % (who, dropout_rate))
        if not self.sess:
            raise RuntimeError("Attempted to use a closed Session. (call init() or load() first)")
        return dropout_rate

    def fine_tune(self, features, labels, steps, batch_size=45, seed=0, val=None, depth=None, dropout_rate=None, val_every=None,
                  keep="last"):
        """Train stages 8 and 9 and the dense head on cached features, on the GPU (``rn_ft_*``; not the reference's whole-network
        ``train_step``): stages 0-7 stay as loaded, every BN keeps its moving statistics and trains gamma and beta (the
        reference's shipped configuration, train.py:40-41), Adam with the constructor's ``learn_rate``, ``num_steps`` (decay),
        ``l2_regularizer_coeff`` and ``start_step``.  ``features``: float32 ``[N, S7, S7, 16]`` of ``extract_features``;
        ``labels``: N class ids; minibatches of ``batch_size`` in the reference feeder's order (``finetune.epoch_indices``, a
        fresh shuffle per epoch from ``seed`` and the current step).  ``val``: ``(features, labels)`` evaluated after the last step.
        The depth is taken from the features' shape: ``[N, S6, S6, 128]`` of ``extract_features(..., depth=3)`` trains stage 7 as
        well, the whole last conv block (that cache is 1.08 MB per image at 224, against 28 KB at depth 2); a shape of neither
        depth, or one that contradicts an explicit ``depth``, raises ``ValueError``.
        The trained variables are written back through ``set_variables`` (the next ``infer`` builds its engine on them, ``save()``
        writes them) and ``self.step`` advances.  Returns ``{"losses": float32[steps] (each before its update), "step",
        "learn_rate" (at the new step), "val": (loss, accuracy) or None}``.  Adam's slots start at zero in every call.
        ``dropout_rate``: a float in ``[0, 1)`` trains with dropout at every site at or behind the cached feature
        (``finetune.dropout_sites``: the last conv block's output and every dense block's, at depth 3 the cached ``s6.bn`` as well),
        whatever the constructor's ``dropout_enabled``, with ``seed`` as the dropout seed.  The reference's dropout behind the frozen
        conv blocks upstream of the cache cannot be applied to cached features, which is why the opt-in is explicit: a net
        constructed with ``dropout_enabled=True`` raises ``ValueError`` unless the argument is given, e.g.
        ``nn.fine_tune(f, y, steps, dropout_rate=nn.dropout_rate)``.  ``val`` and inference never drop.
        ``val_every=k`` (needs ``val``) validates on the GPU inside the training run, as the reference's loop does every
        ``SAVE_FREQ`` steps (train.py:134-155): after every global step that is a multiple of ``k`` and after the last step
        (``finetune.validation_steps``), with no host synchronisation in between (``rn_ft_run_validated``).  The result then also
        holds ``"val_history"``, one dict per point with the reference's ``'step'``, ``'accuracy'``, ``'precisions'``,
        ``'recalls'``, ``'f-scores'`` (``metrics.stats_from_confusion``) plus ``'loss'`` and ``'confusion'`` (int32 ``[C, C]``, row =
        label), and ``"best_step"``: the earliest point with the most correct predictions; ``"val"`` is the last point's.
        ``keep="best"`` writes that point's variables back instead of the last step's (``self.step`` advances by ``steps`` either
        way); any other ``keep`` than ``"last"`` or ``"best"`` raises ``ValueError``."""
        from . import finetune
        dropout_rate = self._fine_tune_checked("fine_tune", keep, val_every, val, dropout_rate)
        feats = np.ascontiguousarray(features, np.float32)
        labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if depth is not None:
            shape = finetune.feature_shape(self.graph, depth)
        elif feats.ndim == 4:
            try:
                depth = finetune.depth_of_features(self.graph, feats.shape[1:])
            except ValueError as e:
                raise ValueError("fine_tune: %s" % e) from None
            shape = finetune.feature_shape(self.graph, depth)
        else:
            depth, shape = 2, finetune.feature_shape(self.graph)
        if feats.ndim != 4 or feats.shape[1:] != shape or feats.shape[0] != labels.shape[0] or feats.shape[0] < 1:
            raise ValueError("fine_tune: features %s and labels %s do not form [N, %d, %d, %d] and [N] (depth %d)"
                             % (feats.shape, labels.shape, shape[0], shape[1], shape[2], depth))
        steps = int(steps)
        if steps < 1:
            raise ValueError("fine_tune: steps = %d" % steps)
        index = finetune.epoch_indices(feats.shape[0], batch_size, steps, seed=[int(seed), int(self.step)])
        def run(tr):
            return tr.run_host(feats, labels, index)

        def run_validated(tr, d_vf, d_vl, n_val):
            d = [tr.upload(feats), tr.upload(labels), tr.upload(index)]
            return tr.run_validated(d[0], d[1], feats.shape[0], d[2], index.shape[1], index.shape[0], d_vf, d_vl, n_val, val_every)

        return self._fine_tune_run("fine_tune", depth, index, dropout_rate, seed, val, val_every, keep, run, run_validated)

    def _fine_tune_run(self, who, depth, index, dropout_rate, seed, val, val_every, keep, run, run_validated):
        """What ``fine_tune`` and ``fine_tune_views`` share behind their own checks: the trainer, the run -- ``run(tr)`` gives the
        losses, ``run_validated(tr, d_val_feats, d_val_labels, n_val)`` what ``Trainer.run_validated`` returns --, the validation
        record, the write-back and the result."""
        from . import finetune, metrics
        from ._capi import RN_FT_BEST, RN_FT_PARAM, Trainer
        shape = finetune.feature_shape(self.graph, depth)
        tr = Trainer(self.graph, self.sess.variables, device=self.device, max_batch=max(index.shape[1], min(self.max_batch, 256)),
                     learn_rate=self.learn_rate, num_steps=self.num_steps, start_step=self.step,
                     l2_coeff=self.l2_regularizer_coeff, depth=depth, dropout_rate=dropout_rate or 0.0,
                     dropout_seed=int(seed) if dropout_rate else 0)
        extra = {}
        try:
            out_val = None
            if val_every is not None:
                vf = np.ascontiguousarray(val[0], np.float32)
                vl = np.ascontiguousarray(val[1], np.int32).reshape(-1)
                if vf.ndim != 4 or vf.shape[1:] != shape or vf.shape[0] != vl.shape[0] or vf.shape[0] < 1:
                    raise ValueError("%s: validation features %s and labels %s do not form [N, %d, %d, %d] and [N] (depth %d)"
                                     % (who, vf.shape, vl.shape, shape[0], shape[1], shape[2], depth))
                losses, points, val_losses, confusion = run_validated(tr, tr.upload(vf), tr.upload(vl), vf.shape[0])
                history = []
                for g, vloss, cm in zip(points, val_losses, confusion):
                    entry = {"step": int(g), "loss": float(vloss), "confusion": cm.copy()}
                    entry.update((k, v) for k, v in metrics.stats_from_confusion(cm).items() if k != "support")
                    history.append(entry)
                extra = {"val_history": history, "best_step": tr.best()[0]}
                out_val = (history[-1]["loss"], history[-1]["accuracy"])
            else:
                losses = run(tr)
                if val is not None:
                    vf, vl = val
                    vl = np.ascontiguousarray(vl, np.int32).reshape(-1)
                    loss, _probs, ids = tr.eval_host(vf, vl)
                    out_val = (loss, float(np.mean(ids == vl)))
            new = tr.read(RN_FT_BEST if keep == "best" else RN_FT_PARAM)
            step = tr.step_count()
        finally:
            tr.close()
        self.set_variables(new)
        self.step = step
        out = {"losses": losses, "step": step, "val": out_val,
               "learn_rate": finetune.learn_rate_at(step, self.learn_rate, self.num_steps)}
        out.update(extra)
        return out

    def fine_tune_views(self, images, labels, steps, batch_size=45, seed=0, depth=2, random_crop=True, flip=True, val=None,
                        val_every=None, keep="last", dropout_rate=None):
        """``fine_tune`` on fresh random views of whole photographs instead of cached features, the reference's training regime
        (train.py:117-118, a feeder with ``random_crop=True, preprocess=True``): every sample of every step is a fresh random square
        window slid along the photograph's long axis, resized to the network's side and mirrored left-right and upside-down with
        probability 1/2 each (``finetune.view_draw``, ``finetune.make_view``: the draws come from the trainers' Philox generator,
        keyed by ``seed``, the global step and the minibatch slot; NumPy's own stream is not reproduced).  ``images``: a list of BGR
        uint8 arrays of any size, uploaded once into one device allocation (a failed allocation raises and says how many bytes the
        set needs); every step the GPU makes the minibatch's views, runs the frozen trunk on them and trains on those features
        (``rn_ft_run_views``).  ``depth``: 2 trains stages 8-9 and the head, 3 the whole last conv block.  ``random_crop=False`` takes
        the centre window, ``flip=False`` never mirrors.  ``val``: ``(features, labels)`` as ``fine_tune`` takes it -- cached
        centre-crop features of ``extract_features(..., depth=depth)``: the reference validates on ``random_crop=False,
        preprocess=False``.  Everything else -- ``val_every``, ``keep``, ``dropout_rate``, the result and the write-back -- is
        ``fine_tune``'s."""
        from . import finetune
        dropout_rate = self._fine_tune_checked("fine_tune_views", keep, val_every, val, dropout_rate)
        depth = finetune._checked_depth(depth)
        images = list(images)
        labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if not images or len(images) != labels.shape[0]:
            raise ValueError("fine_tune_views: %d images and labels %s do not form N photographs and [N]" % (len(images), labels.shape))
        steps = int(steps)
        if steps < 1:
            raise ValueError("fine_tune_views: steps = %d" % steps)
        index = finetune.epoch_indices(len(images), batch_size, steps, seed=[int(seed), int(self.step)])
        if index.shape[1] > self.max_batch:
            raise ValueError("fine_tune_views: a minibatch of %d views exceeds max_batch=%d (the trunk runs on every minibatch; "
                             "construct with a larger max_batch)" % (index.shape[1], self.max_batch))
        eng = self._engine()
        views = eng.views_create(images)

        def run(tr, **validation):
            return tr.run_views(eng, views, tr.upload(labels), tr.upload(index), index.shape[1], index.shape[0], seed=int(seed),
                                crop=bool(random_crop), flip=bool(flip), **validation)

        def run_validated(tr, d_vf, d_vl, n_val):
            return run(tr, d_val_feats=d_vf, d_val_labels=d_vl, n_val=n_val, val_every=val_every)

        try:
            return self._fine_tune_run("fine_tune_views", depth, index, dropout_rate, seed, val, val_every, keep, run, run_validated)
        finally:
            views.close()

    def training_views(self, images, step, seed=0, index=None, random_crop=True, flip=True):
        """The ``[n, S, S, 3]`` uint8 views the GPU makes of the BGR photographs ``images`` at global step ``step``
        (``rn_views_batch_device``): slot ``b`` is the view of ``images[index[b]]`` (``index=None``: every image in order), what
        ``fine_tune_views`` with the same ``seed`` feeds the trunk in that slot at that step.  At most ``max_batch`` slots."""
        images = list(images)
        index = np.arange(len(images), dtype=np.int32) if index is None else np.ascontiguousarray(index, np.int32).reshape(-1)
        eng = self._engine()
        views = eng.views_create(images)
        try:
            return eng.views_batch(views, index, int(step), seed=int(seed), crop=bool(random_crop), flip=bool(flip))
        finally:
            views.close()

    def train_step(self, x_in, y):
        raise NotImplementedError("training (network.py:158-170) is out of scope of the MI355X inference path")
