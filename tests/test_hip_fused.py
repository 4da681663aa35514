"""GPU parity of the fused 16-bit MFMA path (RN_DTYPE_BF16 / RN_DTYPE_F16) with the
oracle, through the C ABI.  BASELINE config 3 at parity-test sizes.

Tolerances: 16-bit storage + fp32 accumulate: logits abs <= 0.1,
ids identical where the fp64 top-2 logit margin > 0.2.  Stage outputs are compared with
the fp32 oracle taps relative to the tensor's abs-max (bf16 has an 8-bit significand and
the error compounds over ten stages)."""
import numpy as np
import pytest

from conftest import with_gammas
from oracle import c_oracle
from parity_bounds import FUSED_AWAY, MARGIN, STAGE_TOL, _downstream_same, _same_up_to_sum_order
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

TOL_LOGITS = 0.1          # SURVEY 8c's bound on |logit - fp64 truth| for 16-bit storage: the contract
# What the tests ASSERT on the parity sets since round 6 (conv weights rounded with the residual carried from tap to tap; bf16 stores
# of stages 3, 4, 5 dithered by the output row): measured 0.030 (bf16) / 0.022 (fp16) at 224 and 0.026 / 0.017 at 600
# (profiles/r6_parity.json; rounds 1-5: 0.080 / 0.022 and 0.126 / 0.014)
TOL_LOGITS_224 = {"bf16": 0.06, "f16": 0.05}
TOL_LOGITS_600 = {"bf16": 0.1, "f16": 0.05}


@pytest.fixture(scope="module", params=["bf16", "f16"])
def engine(request, weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=request.param, max_batch=8)
    e.dtype_name = request.param
    yield e
    e.close()


@pytest.fixture(scope="module", params=["bf16", "f16"])
def engine_stagewise(request, weights):
    """One launch per stage (RN_FLAG_STAGE_LAUNCHES): every stage output is materialised."""
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=request.param, max_batch=8, stage_launches=True)
    e.dtype_name = request.param
    yield e
    e.close()


def _stage_out_names(g):
    return ["s%d.%s" % (s.index, "bn2" if s.residual else "bn") for s in g.stages]


def _check_stage_outputs(engine, weights, parity_images, skip=(), record=None, label=""):
    idx = [14, 30, 2]
    ims = parity_images[idx]
    ref = c_oracle.infer(weights, ims, taps=True)
    ids, probs = engine.forward_u8(ims)
    report = []
    for name in _stage_out_names(engine.graph):
        if name in skip:
            with pytest.raises(_capi.RoomNetLibraryError):
                engine.tap(name, len(idx))
            continue
        got = engine.tap(name, len(idx))
        want = np.asarray(ref["taps"][name])
        assert got.shape == want.shape, name
        rel = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-6))
        report.append((name, rel))
    print(engine.dtype_name, " ".join("%s=%.2e" % r for r in report))
    if record:
        record("stage_rel_err_224_%s" % label, engine.dtype_name, {name: rel for name, rel in report})
    for name, rel in report:
        assert rel <= STAGE_TOL[engine.dtype_name], (name, rel, report)


def test_stage_outputs_vs_oracle(engine, weights, parity_images, record):
    _check_stage_outputs(engine, weights, parity_images, skip=FUSED_AWAY, record=record, label="fused_launches")


def test_stage_outputs_vs_oracle_stagewise(engine_stagewise, weights, parity_images, record):
    _check_stage_outputs(engine_stagewise, weights, parity_images, record=record, label="one_launch_per_stage")


def test_stage0_is_exact_up_to_the_rounding_of_its_output(engine_stagewise, weights, parity_images):
    """Stage 0 of the 16-bit path multiplies the exact byte values by weights held as fp16 hi + lo pairs (rn_stage.h,
    s0_pixel_halves) and accumulates in float32: what is left against the oracle is the ONE rounding of its output to
    the storage type -- half an ulp of the value, element by element (2^-12 of the value for fp16, 2^-9 for bf16), plus
    float32 summation noise.  With fp16-rounded inputs and weights the error was ~10 x that of the output rounding."""
    idx = [0, 3, 26, 14]
    ims = parity_images[idx]
    want = np.asarray(c_oracle.infer(weights, ims, taps=True)["taps"]["s0.bn"], dtype=np.float64)
    engine_stagewise.forward_u8(ims)
    got = engine_stagewise.tap("s0.bn", len(idx)).astype(np.float64)
    half_ulp = 2.0 ** -12 if engine_stagewise.dtype_name == "f16" else 2.0 ** -9
    # (half an ulp relative to the value can reach 2 x half_ulp just above a power of two; 5e-6 absolute: float32 sums of ~100)
    bound = 2.0 * half_ulp * np.abs(want) + 5e-6 * np.abs(want).max()
    bad = np.abs(got - want) > bound
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - want).max()), float(np.abs(want).max()))


@pytest.mark.parametrize("nb", [1, 5, 8, 33, 70])
def test_cross_stage_fusion_is_bit_identical_to_stage_launches(weights, parity_images, nb):
    """The fused s2->s3 kernel runs the same arithmetic as the two stage launches: the block output, everything
    downstream and the probabilities must agree bit for bit (up to the fp32 order of the pooling sums, see
    _same_up_to_sum_order), whatever the band decomposition (nb = 1 .. 70 images:
    26 bands .. 4 bands per image)."""
    pick = (np.arange(nb) * 7) % len(parity_images)
    ims = parity_images[pick]
    for dtype in ("bf16", "f16"):
        fused = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=nb)
        plain = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
        try:
            ids_f, probs_f = fused.forward_u8(ims)
            ids_p, probs_p = plain.forward_u8(ims)
            a1, b1 = fused.tap("s1.bn", nb), plain.tap("s1.bn", nb)
            bad = np.argwhere(a1 != b1)
            assert bad.size == 0, ("s1", dtype, len(bad), bad[:8].tolist(), float(np.abs(a1 - b1).max()))
            _same_up_to_sum_order(fused.tap("s3.bn2", nb), plain.tap("s3.bn2", nb), dtype, "s3.bn2")
            # tail kernel (rn_tail.hip) and head
            _downstream_same(fused, plain, ("s8.bn", "s9.bn2", "d3.relu"), nb, dtype, probs_f, probs_p, ids_f, ids_p)
        finally:
            fused.close()
            plain.close()


def test_logits_probs_ids_vs_golden(engine, parity_images, golden_parity, record):
    errs = []
    for i in range(0, len(parity_images), 8):    # logits of all 64 images, in chunks of the engine's capacity
        engine.forward_u8(parity_images[i:i + 8])
        errs.append(np.abs(engine.tap("d3.relu", 8) - golden_parity["logits_f64"][i:i + 8]).max(1))
    errs = np.concatenate(errs)
    ids, probs = engine.forward_u8(parity_images)
    err = errs.max()
    # every class of infer.py:22 is reached, on the GPU too, and the logit error is reported per class
    assert set(ids.tolist()) == {0, 1, 2, 3, 4, 5}
    gids = golden_parity["ids"]
    record("parity_set_64_images_224", engine.dtype_name, {
        "max_abs_dlogit_vs_fp64_by_fp64_class": {str(c): float(errs[gids == c].max()) for c in range(6)},
        "images_by_fp64_class": {str(c): int((gids == c).sum()) for c in range(6)},
        "ids_by_class_gpu": {str(c): int((ids == c).sum()) for c in range(6)},
        "max_abs_dlogit_vs_fp64": float(err), "mean_abs_dlogit_per_image_max": float(errs.mean()),
        "max_abs_dprob_vs_fp64": float(np.abs(probs - golden_parity["probs_f64"]).max()),
        "ids_differing_from_fp64": int((ids != golden_parity["ids"]).sum()),
        "smallest_top2_margin_fp64": float(golden_parity["top2_margin"].min())})
    assert err <= TOL_LOGITS_224[engine.dtype_name], err
    safe = golden_parity["top2_margin"] > MARGIN
    assert safe.sum() >= 25
    np.testing.assert_array_equal(ids[safe], golden_parity["ids"][safe])
    # north_star: "argmax IDs bit-exact".  Over ALL 64 images: how many ids differ, and none of them may belong to an
    # image whose fp64 top-2 margin exceeds the tolerance (a flip below it is a tie broken by 16-bit rounding)
    differ = np.nonzero(ids != golden_parity["ids"])[0]
    print("%s: %d of %d class ids differ from the fp64 golden%s" % (
        engine.dtype_name, len(differ), len(ids),
        "".join(" [image %d, margin %.3f]" % (i, golden_parity["top2_margin"][i]) for i in differ)))
    assert all(golden_parity["top2_margin"][i] <= MARGIN for i in differ)
    assert len(differ) == 0, "expected every id to match on the parity set (all margins there are >= 0.19)"
    np.testing.assert_allclose(probs.sum(1), 1.0, atol=1e-5)
    # probabilities follow from the logits: generous bound from the logit tolerance
    assert np.abs(probs - golden_parity["probs_f64"]).max() <= 0.05


def test_band_and_batch_invariance(engine, parity_images):
    """A different batch size changes the band decomposition (rows per workgroup); results
    must be bit-identical because every output element is computed by the same arithmetic."""
    ims = parity_images[[3, 17, 26, 31, 36]]
    ids_b, probs_b = engine.forward_u8(ims)
    s3_b = engine.tap("s3.bn2", 5)
    for i in (0, 4):
        ids_1, probs_1 = engine.forward_u8(ims[i:i + 1])
        np.testing.assert_array_equal(engine.tap("s3.bn2", 1)[0], s3_b[i])
        np.testing.assert_array_equal(probs_1[0], probs_b[i])
        assert ids_1[0] == ids_b[i]


@pytest.mark.parametrize("nb", [2, 3, 9, 33, 100, 129])
def test_results_do_not_depend_on_the_batch_geometry(weights, parity_images, nb):
    """The band count per launch follows the batch size (whole rounds of the chip): 1, 2, 4 ... 26 bands.  Whatever
    the decomposition, an image's stage outputs and probabilities are bit-identical to its batch-of-one result."""
    eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=nb)
    try:
        pick = np.arange(nb) % len(parity_images)
        ids, probs = eng.forward_u8(parity_images[pick])
        s5 = eng.tap("s5.bn2", nb)
        # from half a chip's worth of images on (128) the back end runs as ONE launch per image (rn_backend.hip): stages 6 and 7
        # stay in LDS, stage 8 is the first tensor behind them that is written
        late = "s8.bn" if nb >= 128 else "s7.bn"
        if nb >= 128:
            with pytest.raises(_capi.RoomNetLibraryError):
                eng.tap("s7.bn", nb)
        s7 = eng.tap(late, nb)
        for i in sorted({0, nb // 2, nb - 1}):
            ids1, probs1 = eng.forward_u8(parity_images[pick[i]:pick[i] + 1])
            np.testing.assert_array_equal(eng.tap("s5.bn2", 1)[0], s5[i])
            np.testing.assert_array_equal(eng.tap(late, 1)[0], s7[i])
            np.testing.assert_array_equal(probs1[0], probs[i])
            assert ids1[0] == ids[i]
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_launch_back_end_is_bit_identical_to_the_stage_launches(weights, parity_images, dtype):
    """Stage 6 -> 7 -> 8 -> 9 -> head as one launch per image (default handle, 160 images) against one launch per stage
    (RN_FLAG_STAGE_LAUNCHES): agreement up to the fp32 summation order of the fused pair in front of it; and bit for bit, every
    tensor behind the back end (s8.bn, s9.bn2, the logits) and the results, against the default handle at a small batch, whose back
    end is the three launches (64 images < half a chip of images) and whose results the oracle tests pin."""
    nb = 160
    pick = (np.arange(nb) * 3) % len(parity_images)
    ims = parity_images[pick]
    fused = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=nb)
    plain = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
    small = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=len(parity_images))
    try:
        ids_f, probs_f = fused.forward_u8(ims)
        ids_p, probs_p = plain.forward_u8(ims)
        assert fused.launch_groups()[-1] == [6, 7, 8, 9] and len(parity_images) < 128
        taps_f = {name: fused.tap(name, nb) for name in ("s8.bn", "s9.bn2", "d3.relu")}
        # against one launch per stage: the fused PAIR (stages 2+3) in front of both back ends sums its pooling windows in
        # another fp32 order than the per-stage launches (see _same_up_to_sum_order), so from s3.bn2 on the two handles agree up
        # to that -- 16-bit tensors within a few ulp on a few elements, the fp32 logits within the bound the probabilities get
        for name in ("s8.bn", "s9.bn2"):
            _same_up_to_sum_order(taps_f[name], plain.tap(name, nb), dtype, name, frac=5e-2, n_ulp=12)
        np.testing.assert_allclose(taps_f["d3.relu"], plain.tap("d3.relu", nb), rtol=0, atol=1e-2)
        np.testing.assert_allclose(probs_f, probs_p, rtol=0, atol=2e-3)
        np.testing.assert_array_equal(ids_f, ids_p)
        # against the default handle at a small batch (same fused pair, back end as three launches): bit for bit, every tensor
        ids8, probs8 = small.forward_u8(parity_images)
        for name in ("s8.bn", "s9.bn2", "d3.relu"):
            np.testing.assert_array_equal(taps_f[name], small.tap(name, len(parity_images))[pick], err_msg=name)
        np.testing.assert_array_equal(probs_f, probs8[pick])
        np.testing.assert_array_equal(ids_f, ids8[pick])
    finally:
        fused.close()
        plain.close()
        small.close()


def test_against_f32_hip_path(engine, weights, parity_images):
    f32 = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="f32", max_batch=8)
    try:
        ims = parity_images[8:16]
        engine.forward_u8(ims)
        f32.forward_u8(ims)
        assert np.abs(engine.tap("d3.relu", 8) - f32.tap("d3.relu", 8)).max() <= TOL_LOGITS
    finally:
        f32.close()


def test_rejects_float_input_and_taps(engine, weights):
    with pytest.raises(_capi.RoomNetLibraryError):
        engine.forward_f32(np.zeros((1, 224, 224, 3), np.float32))
    with pytest.raises(_capi.RoomNetLibraryError):
        engine.tap("s2.conv", 1)
    with pytest.raises(ValueError):
        _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=2, taps=True)


def test_timing(engine, parity_images):
    engine.set_profiling(True)
    engine.forward_u8(parity_images[:8])
    t = engine.timing()
    engine.set_profiling(False)
    # (stage 0 runs inside stage 1's launch, stage 2 inside stage 3's, stage 8 and the head inside stage 9's: their
    #  own slots read ~0)
    assert len(t["stage_ms"]) == 10 and all(x > 0 for i, x in enumerate(t["stage_ms"]) if i not in (0, 2, 8))
    assert engine.launch_groups() == [[0, 1], [2, 3], [4], [5], [6], [7], [8, 9]]


# ------------------------------------------------------------------ full size (BASELINE configs 3/4: batch 256)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_full_batch_256_properties(weights, parity_images, golden_parity, dtype):
    """Batch 256 (the bench configuration: one band per image, two workgroup rounds per CU) through
    size-independent properties: (1) every image's result equals, bit for bit, the result the same image
    gets in a batch of 8 (which the tests above pin to the oracle); (2) a permuted batch gives the permuted
    results; (3) a second pass over the same buffers is identical (no state leaks between launches)."""
    rng = np.random.default_rng(256)
    pick = rng.integers(0, len(parity_images), 256)
    ims = parity_images[pick]
    big = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=256)
    small = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=8)
    try:
        ids, probs = big.forward_u8(ims)
        s7 = big.tap("s8.bn", 256)              # (the first tensor behind the one-launch back end, rn_backend.hip)
        ids8, probs8 = small.forward_u8(parity_images)          # 64 images in chunks of 8
        np.testing.assert_array_equal(probs, probs8[pick])
        np.testing.assert_array_equal(ids, ids8[pick])
        safe = golden_parity["top2_margin"][pick] > MARGIN
        np.testing.assert_array_equal(ids[safe], golden_parity["ids"][pick][safe])
        perm = rng.permutation(256)
        ids_p, probs_p = big.forward_u8(ims[perm])
        np.testing.assert_array_equal(probs_p, probs[perm])
        np.testing.assert_array_equal(big.tap("s8.bn", 256), s7[perm])
        ids_2, probs_2 = big.forward_u8(ims[perm])
        np.testing.assert_array_equal(probs_2, probs_p)
        # ragged tail: 255 and 1 images through the 256-image handle
        ids_r, probs_r = big.forward_u8(ims[:255])
        np.testing.assert_array_equal(probs_r, probs[:255])
        ids_1, probs_1 = big.forward_u8(ims[255:])
        np.testing.assert_array_equal(probs_1, probs[255:])
    finally:
        big.close()
        small.close()


def test_randomized_batch_256_against_the_f32_hip_path(weights, record):
    """256 random images (uniform noise, blurred noise, extremes) through the fused bf16 path at bench size vs the
    per-node float32 HIP path: every image's logits within the 16-bit tolerance and the late stage outputs finite and
    close everywhere -- a localized corruption (one tile-row of one workgroup) cannot hide in a maximum over 64 images."""
    rng = np.random.default_rng(20261002)
    ims = rng.integers(0, 256, (256, 224, 224, 3), dtype=np.uint8)
    ims[0] = 0
    ims[1] = 255
    for i in range(2, 66):                                   # low-frequency content reaches the other classes
        k = int(rng.integers(4, 57))
        small = rng.integers(0, 256, (224 // k + 2, 224 // k + 2, 3), dtype=np.uint8)
        ims[i] = np.kron(small, np.ones((k, k, 1), np.uint8))[:224, :224]
    big = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=256)
    f32 = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="f32", max_batch=32)
    try:
        ids, probs = big.forward_u8(ims)
        logits = big.tap("d3.relu", 256)
        s7 = big.tap("s8.bn", 256)              # (stages 6 and 7 stay in LDS at this batch: rn_backend.hip)
        s3 = big.tap("s3.bn2", 256)
        assert np.isfinite(logits).all() and np.isfinite(s7).all() and np.isfinite(s3).all()
        worst = worst_stage = 0.0
        for i in range(0, 256, 32):
            f32.forward_u8(ims[i:i + 32])
            ref_logits = f32.tap("d3.relu", 32)
            ref_s7 = f32.tap("s8.bn", 32)
            ref_s3 = f32.tap("s3.bn2", 32)
            worst = max(worst, float(np.abs(logits[i:i + 32] - ref_logits).max()))
            for got, want in ((s7[i:i + 32], ref_s7), (s3[i:i + 32], ref_s3)):
                per_image = np.abs(got - want).reshape(32, -1).max(1) / max(float(np.abs(want).max()), 1e-6)
                worst_stage = max(worst_stage, float(per_image.max()))
                assert per_image.max() <= 2 * STAGE_TOL["bf16"], (i, per_image.argmax(), per_image.max())
        record("random_256_images_224", "bf16_vs_float32_hip_path", {"max_abs_dlogit": worst, "max_stage_rel_err_s3_s8": worst_stage})
        assert worst <= TOL_LOGITS_224["bf16"], worst
        np.testing.assert_allclose(probs.sum(1), 1.0, atol=1e-5)
    finally:
        big.close()
        f32.close()


def test_random_4096_images_id_agreement_with_the_f32_hip_path(weights, record):
    """4096 random images (uniform noise and block noise of random scale, which reaches several classes) through the
    fused bf16 path against the per-node float32 HIP path: count the disagreeing class ids; every disagreement must be
    a near-tie in float32 (top-2 logit margin below the 16-bit tolerance)."""
    rng = np.random.default_rng(4096)
    n, chunk = 4096, 256
    big = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=chunk)
    f32 = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="f32", max_batch=32)
    disagree, seen = [], np.zeros(6, np.int64)
    try:
        for c0 in range(0, n, chunk):
            ims = rng.integers(0, 256, (chunk, 224, 224, 3), dtype=np.uint8)
            for i in range(0, chunk, 2):                       # every other image: block noise, block size 2..80
                k = int(rng.integers(2, 81))
                small = rng.integers(0, 256, (224 // k + 2, 224 // k + 2, 3), dtype=np.uint8)
                ims[i] = np.kron(small, np.ones((k, k, 1), np.uint8))[:224, :224]
            ids16, _ = big.forward_u8(ims)
            for j in range(0, chunk, 32):
                ids32, _ = f32.forward_u8(ims[j:j + 32])
                lg = np.sort(f32.tap("d3.relu", 32), axis=1)
                margin = lg[:, -1] - lg[:, -2]
                seen += np.bincount(ids32, minlength=6)
                for t in np.nonzero(ids16[j:j + 32] != ids32)[0]:
                    disagree.append((c0 + j + int(t), float(margin[t])))
    finally:
        big.close()
        f32.close()
    print("bf16 vs float32 HIP path: %d of %d class ids differ; classes seen %s; margins of the differing ones: %s" % (
        len(disagree), n, seen.tolist(), ["%.3f" % m for _, m in disagree][:20]))
    record("random_4096_images_224", "bf16_vs_float32_hip_path", {
        "images": n, "ids_differing": len(disagree), "classes_seen_float32": seen.tolist(),
        "float32_top2_margins_of_the_differing": [round(m, 4) for _, m in disagree],
        "largest_margin_of_a_differing_id": max([m for _, m in disagree], default=0.0)})
    assert (seen > 0).sum() >= 2                               # the set is not degenerate
    assert all(m <= MARGIN for _, m in disagree), disagree
    assert len(disagree) <= n // 100


def test_batch_limits(engine):
    """Empty and over-size batches follow the error convention instead of launching."""
    buf = np.zeros((engine.max_batch + 1, 224, 224, 3), np.uint8)
    probs = np.zeros((engine.max_batch + 1, 6), np.float32)
    ids = np.zeros((engine.max_batch + 1,), np.int64)
    for n in (0, -1, engine.max_batch + 1):
        rc = engine.lib.rn_forward_u8(engine.handle, buf.ctypes.data, n, probs.ctypes.data, ids.ctypes.data)
        assert rc < 0, n
        assert b"out of range" in engine.lib.rn_last_error()
    # the Python layer splits an over-size batch into max_batch chunks instead
    ids2, probs2 = engine.forward_u8(buf[:engine.max_batch + 1])
    assert probs2.shape == (engine.max_batch + 1, 6) and np.allclose(probs2.sum(1), 1.0, atol=1e-5)
    ids0, probs0 = engine.forward_u8(buf[:0])
    assert probs0.shape == (0, 6) and ids0.shape == (0,)


# ------------------------------------------------------------------ 600x600 variant (BASELINE config 5)
@pytest.mark.parametrize("dtype,tol", [("f16", TOL_LOGITS_600["f16"]), ("bf16", TOL_LOGITS_600["bf16"]), ("f32", 1e-4)])
def test_600_variant_vs_golden(weights, dtype, tol, record):
    """Large-activation variant: conv/BN weights from the checkpoint, seeded synthetic dense/kernel
    (the shipped one only fits 224).  Exercises column blocks and multi-band launches.
    Tolerances: SURVEY 8c's 0.1 on the logits for bf16 (rounds 4-5 had to state 0.16: the first dense layer sums 3 136 rounded
    inputs, and before round 6 their rounding errors were coherent -- 0.126 on the 16-image set; with the dithered stores and the
    carried weight rounding 0.047), 0.05 for fp16 (BASELINE config 5's dtype: 0.017); the ids are held to the 0.2 margin rule."""
    import os
    from conftest import GOLDEN
    from oracle import roomnet_ref as R
    from conftest import parity_set_of
    g = np.load(os.path.join(GOLDEN, "parity_600.npz"))
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600()
    ims = parity_set_of(600)[g["image_indices"]]
    assert len(ims) >= 16 and g["top2_margin"].min() > 0.25
    e = _capi.Engine(build_graph(6, 600), w, device=0, dtype=dtype, max_batch=len(ims))
    try:
        ids, probs = e.forward_u8(ims)
        logits = e.tap("d3.relu", len(ims))
        rec = {"max_abs_dlogit_vs_fp64": float(np.abs(logits - g["logits_f64"]).max()),
               "ids_differing_from_fp64": int((ids != g["ids"]).sum()), "images": int(len(ids))}
        assert np.abs(logits - g["logits_f64"]).max() <= tol
        safe = g["top2_margin"] > (1e-3 if dtype == "f32" else MARGIN)
        np.testing.assert_array_equal(ids[safe], g["ids"][safe])
        if dtype != "f32":
            # stage outputs against the C oracle for one image
            ref = c_oracle.infer(w, ims[1:2], taps=True)
            e.forward_u8(ims[1:2])
            rels = {}
            for s in e.graph.stages:
                name = "s%d.%s" % (s.index, "bn2" if s.residual else "bn")
                if name in FUSED_AWAY:       # computed inside the next stage's kernel: never in HBM
                    continue
                got, want = e.tap(name, 1), np.asarray(ref["taps"][name])
                rels[name] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-6))
            rec["stage_rel_err"] = rels
            record("parity_600", dtype, rec)
            # (600 x 600: the late tensors are means over more rounded inputs than at 224; bf16 is not BASELINE's dtype at this
            #  size -- config 5 is fp16 -- and its s8.bn reaches 0.023 of abs-max on this image, dithered or not: factor 2, as in round 5)
            for name, rel in rels.items():
                assert rel <= STAGE_TOL[dtype] * (2.0 if dtype == "bf16" else 1.5), (name, rel)
        else:
            record("parity_600", dtype, rec)
    finally:
        e.close()


@pytest.mark.parametrize("nb", [1, 3])
def test_cross_stage_fusion_at_600_is_bit_identical_to_stage_launches(weights, nb):
    """600 x 600: rows of the stage-2 input (591 pixels) do not fit the fused kernel's LDS rings, so it runs three column
    blocks (194 + 194 + 193 output columns) per band; results must still be the two stage launches' bit for bit (block
    seams, the residual's full-width source columns, 73 bands at batch 1)."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600()
    ims = parity_batch(600, seed=1)[[37, 14, 22][:nb]]
    for dtype in ("bf16", "f16"):
        fused = _capi.Engine(build_graph(6, 600), w, device=0, dtype=dtype, max_batch=nb)
        plain = _capi.Engine(build_graph(6, 600), w, device=0, dtype=dtype, max_batch=nb, stage_launches=True)
        try:
            assert [2, 3] in [list(g) for g in fused.launch_groups()]
            ids_f, probs_f = fused.forward_u8(ims)
            ids_p, probs_p = plain.forward_u8(ims)
            _same_up_to_sum_order(fused.tap("s3.bn2", nb), plain.tap("s3.bn2", nb), dtype, "s3.bn2")
            _downstream_same(fused, plain, ("s7.bn",), nb, dtype, probs_f, probs_p, ids_f, ids_p)
        finally:
            fused.close()
            plain.close()


@pytest.mark.parametrize("side,blocks", [(202, 1), (211, 1), (409, 2), (634, 3), (439, 0), (190, 0), (671, 0), (694, 0)])
def test_cross_stage_fusion_geometry_sweep(weights, side, blocks):
    """Edges of the fused kernel's column-block plan: the narrowest supported row (stage-2 input 193 + 1: a one-lane tail
    DMA piece), an odd width, two equal blocks, three blocks of the maximum width 215 (615 output columns), and sides with
    no plan (0 blocks: two launches; 671 and 694: the first and the last side at which stage 5 runs four column blocks, the
    flatten at the head's limit of 4096).  Fused results must be the stage launches' bit for bit."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, side)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    ims = parity_batch(side, seed=1)[[31, 20]]
    fused = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=2)
    plain = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=2, stage_launches=True)
    try:
        groups = [list(x) for x in fused.launch_groups()]
        assert ([2, 3] in groups) == (blocks > 0), (side, g.stages[2].in_side, groups)
        ids_f, probs_f = fused.forward_u8(ims)
        ids_p, probs_p = plain.forward_u8(ims)
        _same_up_to_sum_order(fused.tap("s3.bn2", 2), plain.tap("s3.bn2", 2), "bf16", ("s3.bn2", side))
        _downstream_same(fused, plain, (), 2, "bf16", probs_f, probs_p, ids_f, ids_p)
    finally:
        fused.close()
        plain.close()


@pytest.mark.parametrize("side", [190, 225, 236, 237, 260])
def test_stage0_fusion_shared_ring_edges(weights, side):
    """Stages 0+1 in one launch: up to 227 output columns (side 236) the stage-0 rows sit in ONE ring shared by the
    workgroup (each wave computes 29 stage-0 columns; waves whose tile lies right of a narrow image still take part in the
    barrier), wider images keep the wave-private rings (237: one column block; 260: two).  Stage-1 output must be the
    two-launch path's bit for bit, at batch sizes that give one and several row bands."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, side)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    ims = parity_batch(side, seed=2)[[3, 17, 29]]
    fused = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=3)
    plain = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=3, stage_launches=True)
    try:
        assert [0, 1] in [list(x) for x in fused.launch_groups()]
        for nb in (3, 1):
            ids_f, probs_f = fused.forward_u8(ims[:nb])
            ids_p, probs_p = plain.forward_u8(ims[:nb])
            a, b = fused.tap("s1.bn", nb), plain.tap("s1.bn", nb)
            bad = np.argwhere(a != b)
            assert bad.size == 0, (side, nb, len(bad), bad[:8].tolist())
            # (downstream the fused arm runs the stage pair in one kernel where the side allows it: see _same_up_to_sum_order)
            _downstream_same(fused, plain, (), nb, "bf16", probs_f, probs_p, ids_f, ids_p)
    finally:
        fused.close()
        plain.close()


@pytest.mark.parametrize("side", [190, 202, 300, 420])
def test_conv16_stage_matches_the_generic_kernel_at_odd_sizes(weights, side):
    """The 64->128 and the pooled 128->16 stage run on 16x16x32 tiles (rn_conv16.hip): column blocks of 48 / 21 outputs,
    pixel tiles of 16, their own ring swizzles.  Against the generic 32x32x16 kernel (`generic_kernels=True`) the stage output may differ in the last bit of
    the 16-bit storage (other accumulation order), nowhere more: widths that are no multiple of 16 or 48, one to four
    column blocks, 1 and 3 images (different band counts)."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, side)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    ims = parity_batch(side, seed=1)[[31, 20, 25]]
    for dtype in ("bf16", "f16"):
        fast = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, no_dither=True)      # (the legacy arms round plainly)
        ref = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, generic_kernels=True)
        try:
            for nb in (1, 3):
                fast.forward_u8(ims[:nb])
                ref.forward_u8(ims[:nb])
                ulp = 2.0 ** (-7 if dtype == "bf16" else -10)
                for name in ("s6.bn", "s7.bn"):        # rn_conv16.hip: conv16_kernel, conv16p_kernel (pooled 128 -> 16)
                    a, b = fast.tap(name, nb), ref.tap(name, nb)
                    assert a.shape == b.shape and np.isfinite(a).all()
                    scale = float(np.abs(b).max())
                    # (the generic flag swaps every stage, so the two prefixes differ by 16-bit rounding already)
                    assert float(np.abs(a - b).max()) <= 4 * ulp * scale, (name, side, dtype, nb, float(np.abs(a - b).max()), scale)
        finally:
            fast.close()
            ref.close()


@pytest.mark.parametrize("side", [205, 211, 212, 219, 225, 226, 240, 420, 600, 630, 686])
def test_row_blocked_stage_kernels_match_the_round2_kernels_at_their_geometry_edges(weights, side):
    """Stages 4, 5 and 6 run with row-register blocking where their rows can be cut into column blocks of 194-206 / 66-110 /
    35-50 input columns (rn_stage4x/5x/6x.hip: one block at sides 212-225, two at 420, three at 600, four of stage 6 at 630 and of
    stages 5 and 6 at 686: the block seams), and on the
    round-2 kernels elsewhere.  `pair32=True` forces the round-2 kernels everywhere: the 32-channel block is bit-identical in
    both arms, so stage 4 sees identical inputs and may differ by the last 16-bit place (other accumulation order, fp16
    band-matrix pooling instead of fp32 sums); stages 5 and 6 inherit that.  1 and 3 images (one band / several bands)."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, side)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    ims = parity_batch(side, seed=3)[[5, 11, 38]]
    for dtype in ("bf16", "f16"):
        fast = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, no_dither=True)      # (the legacy arms round plainly)
        ref = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=3, pair32=True)
        try:
            for nb in (3, 1):
                ids_a, _ = fast.forward_u8(ims[:nb])
                ids_b, _ = ref.forward_u8(ims[:nb])
                _same_up_to_sum_order(fast.tap("s3.bn2", nb), ref.tap("s3.bn2", nb), dtype, ("s3.bn2", side))
                ulp = 2.0 ** (-8 if dtype == "bf16" else -11)
                for name, n_ulp in (("s4.bn", 2), ("s5.bn2", 4), ("s6.bn", 4)):
                    a, b = fast.tap(name, nb), ref.tap(name, nb)
                    assert a.shape == b.shape and np.isfinite(a).all()
                    scale = float(np.abs(b).max())
                    err = float(np.abs(a - b).max())
                    assert err <= n_ulp * ulp * scale, (name, side, dtype, nb, err / (ulp * scale))
                np.testing.assert_array_equal(ids_a, ids_b)
        finally:
            fast.close()
            ref.close()


@pytest.mark.parametrize("side", [212, 219, 225, 232])
def test_one_launch_back_end_at_its_geometry_edges(weights, side):
    """rn_backend.hip runs stage 6 -> head as one launch per image where stage 6's input is 35-50 columns wide (one column block) and
    the call carries at least half a chip of images.  Other 224-class sides: 130 images through the default handle (back end
    fused where it applies: checked through the launch grouping) against the same images in chunks of 8 (always the banded
    launches): bit-identical results."""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    g = build_graph(6, side)
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600(g.flat_len)
    base = parity_batch(side, seed=3)
    nb = 130
    ims = base[(np.arange(nb) * 7) % len(base)]
    big = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=nb)
    small = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=8)
    try:
        ids, probs = big.forward_u8(ims)
        fused = big.launch_groups()[-1] == [6, 7, 8, 9]
        s6_in = g.stages[6].in_side
        assert fused == (35 <= s6_in <= 50 and g.stages[7].out_side <= 21), (side, s6_in, big.launch_groups())
        last = big.tap("s9.bn2", nb)
        for i in range(0, nb, 8):
            ids8, probs8 = small.forward_u8(ims[i:i + 8])
            np.testing.assert_array_equal(probs[i:i + 8], probs8)
            np.testing.assert_array_equal(ids[i:i + 8], ids8)
            np.testing.assert_array_equal(last[i:i + 8], small.tap("s9.bn2", len(ids8)))
    finally:
        big.close()
        small.close()


def test_results_are_reproducible_run_to_run(engine, parity_images):
    """Every kernel synchronises its LDS rings with counted waits and bare barriers; a race shows as run-to-run noise
    (one was found that way in a stage-5 variant that never shipped).  Six passes over the same batch must agree bit for
    bit in the late stage outputs and the probabilities."""
    ids0, probs0 = engine.forward_u8(parity_images)
    taps0 = {k: engine.tap(k, 8) for k in ("s3.bn2", "s5.bn2", "s6.bn", "s7.bn")}
    for _ in range(5):
        ids, probs = engine.forward_u8(parity_images)
        np.testing.assert_array_equal(probs, probs0)
        np.testing.assert_array_equal(ids, ids0)
        for k, v in taps0.items():
            np.testing.assert_array_equal(engine.tap(k, 8), v)


def test_cross_stage_fusion_two_unequal_column_blocks_at_420(weights):
    """im_side 420: the stage-2 input is 411 wide -> two column blocks of 201 and 200 output columns.  Fused vs stage
    launches bit for bit, and the block output against the C oracle for one image.  (im_side 300 has no block plan --
    291 input columns would need two blocks narrower than the kernel's 193 -- and must fall back to two launches.)"""
    from oracle import roomnet_ref as R
    from roomnet_amd.synth import parity_batch
    w = dict(weights)
    g420 = build_graph(6, 420)
    w["dense/kernel"] = R.synth_dense_kernel_600(g420.flat_len)
    ims = parity_batch(420, seed=1)[[30, 12]]
    for dtype in ("bf16", "f16"):
        fused = _capi.Engine(g420, w, device=0, dtype=dtype, max_batch=2)
        plain = _capi.Engine(g420, w, device=0, dtype=dtype, max_batch=2, stage_launches=True)
        try:
            assert [2, 3] in [list(g) for g in fused.launch_groups()]
            ids_f, probs_f = fused.forward_u8(ims)
            ids_p, probs_p = plain.forward_u8(ims)
            a, b = fused.tap("s3.bn2", 2), plain.tap("s3.bn2", 2)
            _same_up_to_sum_order(a, b, dtype, "s3.bn2 at 420")
            _downstream_same(fused, plain, (), 2, dtype, probs_f, probs_p, ids_f, ids_p)
            if dtype == "bf16":
                ref = c_oracle.infer(w, ims[:1], taps=True)
                want = np.asarray(ref["taps"]["s3.bn2"])
                rel = float(np.abs(a[:1] - want).max() / max(np.abs(want).max(), 1e-6))
                assert rel <= STAGE_TOL[dtype] * 1.5, rel
        finally:
            fused.close()
            plain.close()
    w300 = dict(weights)
    g300 = build_graph(6, 300)
    w300["dense/kernel"] = R.synth_dense_kernel_600(g300.flat_len)
    e = _capi.Engine(g300, w300, device=0, dtype="bf16", max_batch=1)
    try:
        groups = [list(g) for g in e.launch_groups()]
        assert [2] in groups and [3] in groups
        ids, probs = e.forward_u8(parity_batch(300, seed=1)[30:31])
        assert abs(float(probs.sum()) - 1.0) < 1e-5
    finally:
        e.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_600_variant_at_baseline_size_64_images(weights, dtype):
    """BASELINE config 5 at its per-GPU size (64 x 600x600, 16-bit) through size-independent properties: every image's
    result equals, bit for bit, what the same image gets in the batch of 4 that the golden file pins; a permuted batch
    gives the permuted results; a second pass is identical; a ragged tail (63 + 1) is identical; stage outputs do not
    depend on the launch geometry (bands x column blocks differ between batch 1, 4 and 64)."""
    import os
    from conftest import GOLDEN
    from oracle import roomnet_ref as R
    from conftest import parity_set_of
    g = {k: v[:4] for k, v in np.load(os.path.join(GOLDEN, "parity_600.npz")).items() if k != "note"}    # the first four of the set
    w = dict(weights)
    w["dense/kernel"] = R.synth_dense_kernel_600()
    pool = parity_set_of(600)
    gi = [int(i) for i in g["image_indices"]]
    rng = np.random.default_rng(64)
    pick = np.concatenate([gi, rng.integers(0, len(pool), 60)])
    ims = pool[pick]
    big = _capi.Engine(build_graph(6, 600), w, device=0, dtype=dtype, max_batch=64)
    small = _capi.Engine(build_graph(6, 600), w, device=0, dtype=dtype, max_batch=4)
    try:
        ids, probs = big.forward_u8(ims)
        s3, s5, s7 = big.tap("s3.bn2", 64)[:4], big.tap("s5.bn2", 64)[:4], big.tap("s7.bn", 64)
        assert np.isfinite(s7).all()
        ids4, probs4 = small.forward_u8(pool[gi])
        np.testing.assert_array_equal(probs[:4], probs4)
        np.testing.assert_array_equal(ids[:4], ids4)
        np.testing.assert_array_equal(small.tap("s3.bn2", 4), s3)          # 64-image vs 4-image launch geometry
        np.testing.assert_array_equal(small.tap("s5.bn2", 4), s5)
        logits4 = small.tap("d3.relu", 4)
        assert np.abs(logits4 - g["logits_f64"]).max() <= TOL_LOGITS_600[dtype]
        safe = g["top2_margin"] > MARGIN
        np.testing.assert_array_equal(ids[:4][safe], g["ids"][safe])
        # every other image against its batch-of-4 result
        for c0 in range(4, 64, 4):
            _, p4 = small.forward_u8(ims[c0:c0 + 4])
            np.testing.assert_array_equal(probs[c0:c0 + 4], p4)
        _, p1 = small.forward_u8(ims[7:8])                                  # batch of one: yet another geometry
        np.testing.assert_array_equal(p1[0], probs[7])
        np.testing.assert_array_equal(small.tap("s3.bn2", 1)[0], big.tap("s3.bn2", 64)[7])
        perm = rng.permutation(64)
        ids_p, probs_p = big.forward_u8(ims[perm])
        np.testing.assert_array_equal(probs_p, probs[perm])
        np.testing.assert_array_equal(ids_p, ids[perm])
        np.testing.assert_array_equal(big.tap("s7.bn", 64), s7[perm])
        _, probs_2 = big.forward_u8(ims[perm])
        np.testing.assert_array_equal(probs_2, probs_p)
        _, probs_r = big.forward_u8(ims[:63])
        np.testing.assert_array_equal(probs_r, probs[:63])
        _, probs_1 = big.forward_u8(ims[63:])
        np.testing.assert_array_equal(probs_1, probs[63:])
    finally:
        big.close()
        small.close()


def test_two_slot_host_pipeline_matches_the_blocking_entry(engine, parity_images):
    """rn_submit_u8 / rn_collect: batches in flight in both slots, collected in order, give the blocking call's results;
    misuse follows the error convention."""
    batches = [parity_images[i:i + 8] for i in (0, 8, 16, 24, 32)] + [parity_images[3:6]]
    want = [engine.forward_u8(b) for b in batches]
    got = []
    engine.submit_u8(batches[0], 0)
    for k in range(len(batches)):
        if k + 1 < len(batches):
            engine.submit_u8(batches[k + 1], (k + 1) & 1)
        got.append(engine.collect(k & 1))
    for (ids_w, probs_w), (ids_g, probs_g) in zip(want, got):
        np.testing.assert_array_equal(probs_g, probs_w)
        np.testing.assert_array_equal(ids_g, ids_w)
    with pytest.raises(_capi.RoomNetLibraryError):
        engine.collect(0)                                        # nothing submitted
    engine.submit_u8(batches[0], 1)
    with pytest.raises(_capi.RoomNetLibraryError):
        engine.submit_u8(batches[1], 1)                          # slot still holds uncollected results
    engine.collect(1)


def test_two_slot_pipeline_out_of_pinned_host_buffers(engine, parity_images):
    """rn_host_alloc: page-locked batch buffers (one per slot) make rn_submit_u8's upload an asynchronous DMA; the results are the
    blocking entry's, also when a slot's buffer is refilled right after its rn_collect; the group's host entry takes them too."""
    batches = [parity_images[i:i + 8] for i in (0, 8, 16, 24, 40, 56)]
    want = [engine.forward_u8(b) for b in batches]
    pins = [_capi.PinnedArray((8, 224, 224, 3), np.uint8) for _ in range(2)]
    try:
        got = []
        pins[0].array[...] = batches[0]
        engine.submit_u8(pins[0].array, 0)
        for k in range(len(batches)):
            if k + 1 < len(batches):
                nxt = pins[(k + 1) & 1].array            # its previous batch (k - 1) was collected in the last iteration
                nxt[...] = batches[k + 1]
                engine.submit_u8(nxt, (k + 1) & 1)
            got.append(engine.collect(k & 1))
        for (ids_w, probs_w), (ids_g, probs_g) in zip(want, got):
            np.testing.assert_array_equal(probs_g, probs_w)
            np.testing.assert_array_equal(ids_g, ids_w)
        ids_b, probs_b = engine.forward_u8(pins[1].array)       # the blocking entry out of a pinned buffer
        np.testing.assert_array_equal(probs_b, want[-1][1])
    finally:
        for p in pins:
            p.close()
    assert engine.lib.rn_host_free(None) == 0
    with pytest.raises(_capi.RoomNetLibraryError):
        _capi.PinnedArray((1 << 46,), np.uint8)                   # 64 TiB: the error convention, not an abort


def _to16_rne(x, dtype):
    """float32 -> the handle's 16-bit storage and back (round to nearest even), as the kernels' v_cvt_pk_* do."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def _store16(x, dtype):
    """The handle's 16-bit store of a value whose rounding is NOT dithered (constant channels): fp16 handles round to nearest even;
    bf16 handles convert through v_cvt_sr_bf16_f32 with the plain seed: (bits + 0x8000) >> 16 (tools/ubench/cvt_sr.hip)."""
    if dtype == "f16":
        return _to16_rne(x, dtype)
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x8000) >> 16) << 16).astype(np.uint32).view(np.float32)


def _bn_tables(weights, bn_index, pool_area):
    """(scale, shift) of a pooled stage's folded BatchNorm as rn_fused_prepare builds them in float32: the kernels form
    fma(H, scale, shift) with H = the pooled SUM of ReLU6 / 6 values (network.py:189-193; weights / 6, scale x 6)."""
    n = "batch_normalization" if bn_index == 0 else "batch_normalization_%d" % bn_index
    g, b, m, v = (np.asarray(weights[n + "/" + k], np.float32) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv = (np.float32(1.0) / np.sqrt(v + np.float32(1e-3))) * g
    sc = (inv / np.float32(pool_area)) * np.float32(6.0)
    sh = b - m * inv
    return sc.astype(np.float32), sh.astype(np.float32)


def _frozen5(w):
    """Channels of stage 5 whose first BatchNorm is frozen: fma(H, sc1', sh1') returns sh1' in float32 for every pooled sum H
    (rn_fused_prepare's criterion on its table values, restated in NumPy float32)."""
    f32 = np.float32
    g6, b6, m6, v6 = (np.asarray(w["batch_normalization_6/" + k], f32) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    g7, b7, m7, v7 = (np.asarray(w["batch_normalization_7/" + k], f32) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv6 = (f32(1.0) / np.sqrt(v6 + f32(1e-3))) * g6
    inv7 = (f32(1.0) / np.sqrt(v7 + f32(1e-3))) * g7
    t1 = (b6 - m6 * inv6) * inv7 + (b7 - m7 * inv7)
    t0 = ((inv6 / f32(16.0)) * inv7) * f32(6.0)
    return {c for c in range(64) if abs(float(t0[c])) * 16.0 * (1.0 + 1e-6) < abs(float(t1[c])) * 2.0 ** -25}


def _per_channel_arms(a, b, dtype, exact_channels, what, frac=1e-3, n_ulp=12):
    """Folded against computed, channel by channel: the channels in `exact_channels` bit for bit; the others differ only where
    a one-ulp difference upstream (another fp32 summation order) tips a 16-bit rounding: at most `frac` of the elements (measured:
    3e-5), each by at most `n_ulp` 16-bit ulps of the element (1 % of the abs-max as the floor: an element near zero is a difference
    of larger numbers; measured up to 10 such units in fp16, 2.6 in bf16)."""
    for c in exact_channels:
        np.testing.assert_array_equal(a[..., c], b[..., c], err_msg="%s channel %d" % (what, c))
    ulp = 2.0 ** (-8 if dtype == "bf16" else -11)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    lim = n_ulp * ulp * np.maximum(np.abs(b.astype(np.float64)), 0.01 * float(np.abs(b).max()))
    assert int((a != b).sum()) <= max(2, frac * a.size) and float((d / lim).max()) <= 1.0, (what, dtype, int((a != b).sum()), a.size, float((d / lim).max()))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_frozen_channels_fold_against_computing_them(weights, parity_images, dtype, record):
    """Rounds 5 / 6: channels the shipped checkpoint's BatchNorm freezes are not convolved (rn_create proves them constant;
    RN_FLAG_COMPUTE_FROZEN is the arm that computes them).  Both arms against each other at batch 1 / 8 / 160 (band
    decompositions, the one-launch back end), CHANNEL BY CHANNEL: the constant channels of s4.bn (round 6: the plainly rounded
    16-bit store of fma(H, sc, sh) is one number for every H in [0, 16]) hold that number at every pixel in BOTH arms, and so do
    the channels of s5.bn2 behind them (bf16 handles: the 16 folded ones -- the stores of the other channels are dithered); every other channel differs in <= 1e-3 of its elements by a few ulps (measured: 3e-5 of the elements, one
    ulp; the round-5 bounds were 3e-2 and 16).  Both arms are held to the oracle by the shared parity tests."""
    g = build_graph(6, 224)
    sc4, sh4 = _bn_tables(weights, 5, 16)
    const4 = [c for c in range(64) if _store16(np.float32(0.0) * sc4[c] + sh4[c], dtype) == _store16(np.float32(np.float32(16.0) * sc4[c] + sh4[c]), dtype)]
    for nb in (1, 8, 160):
        pick = (np.arange(nb) * 5) % len(parity_images)
        ims = parity_images[pick]
        fold = _capi.Engine(g, weights, device=0, dtype=dtype, max_batch=nb)
        full = _capi.Engine(g, weights, device=0, dtype=dtype, max_batch=nb, compute_frozen=True)
        try:
            ci = fold.const_info()
            assert ci["stage"] == 4 and ci["channels_not_convolved"] == 16 and ci["next_stage_input_channels"] == 48, ci
            assert ci["channels_proven_constant"] == len(const4) == (26 if dtype == "bf16" else 23), (ci, len(const4))
            assert full.const_info()["stage"] == -1
            fi = fold.frozen_info()
            assert fi["pair_channels_not_convolved"] == 24 and fi["pair_channels_proven_frozen"] == (26 if dtype == "bf16" else 25), fi
            assert full.frozen_info()["pair_channels_not_convolved"] == 0
            ids_a, probs_a = fold.forward_u8(ims)
            ids_b, probs_b = full.forward_u8(ims)
            np.testing.assert_array_equal(fold.tap("s1.bn", nb), full.tap("s1.bn", nb))      # (in front of the pair: the same kernel)
            a, b = fold.tap("s3.bn2", nb), full.tap("s3.bn2", nb)
            _per_channel_arms(a, b, dtype, [], ("s3.bn2", nb))
            a4, b4 = fold.tap("s4.bn", nb), full.tap("s4.bn", nb)
            # the 16 folded channels (the highest-numbered constants of s4.bn among stage 5's frozen channels) keep the plain rounding
            # on bf16 handles, whose other stores are dithered by the output row; fp16 handles round every channel plainly
            both = sorted(set(const4) & _frozen5(weights))
            exact4 = const4 if dtype == "f16" else both[-16:]
            for arm in (a4, b4):          # the constant channels ARE their table value, in both arms, at every pixel
                for c in exact4:
                    assert (arm[..., c] == _store16(sh4[c], dtype)).all(), (dtype, nb, c)
            _per_channel_arms(a4, b4, dtype, exact4, ("s4.bn", nb))
            a5, b5 = fold.tap("s5.bn2", nb), full.tap("s5.bn2", nb)
            const5 = both if dtype == "f16" else both[-16:]        # frozen first BN + constant skip channel: constants again
            assert len(const5) >= 16
            for arm in (a5, b5):
                for c in const5:
                    assert np.unique(arm[..., c]).size == 1, (dtype, nb, c)
            _per_channel_arms(a5, b5, dtype, const5, ("s5.bn2", nb))
            np.testing.assert_allclose(probs_a, probs_b, rtol=0, atol=2e-3)
            np.testing.assert_array_equal(ids_a, ids_b)
            if nb == 160:
                record("frozen_channel_fold", dtype, {"elements_differing_in_s3_bn2": int((a != b).sum()), "elements": int(a.size),
                                                       "max_abs_diff_s3_bn2": float(np.abs(a - b).max()),
                                                       "elements_differing_in_s5_bn2": int((a5 != b5).sum()), "elements_s5_bn2": int(a5.size),
                                                       "constant_channels_s4_bn": len(const4), "constant_channels_s5_bn2": len(const5),
                                                       "max_abs_dprob": float(np.abs(probs_a - probs_b).max())})
        finally:
            fold.close()
            full.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_frozen_channels_are_their_table_value_at_every_pixel(weights, parity_images, dtype):
    """The fold's premise, on the tensors themselves (one launch per stage, so that s2.bn exists in HBM): every channel of s2.bn
    whose fma returns its addend in float32 (|sc| 16 < 2^-25 |sh|) equals to16(sh) at every pixel of every image -- computed
    (RN_FLAG_COMPUTE_FROZEN) and default handle alike; the live channels are not constants."""
    g = build_graph(6, 224)
    sc2, sh2 = _bn_tables(weights, 2, 16)
    frozen = [c for c in range(32) if abs(float(sc2[c])) * 16.0 * (1.0 + 1e-6) < abs(float(sh2[c])) * 2.0 ** -25]
    assert len(frozen) == 18
    # round 6: the pair folds by the tensor's 16-bit STORE -- a superset (the scale below half an ulp of the shift): 26 / 25 channels
    stored_const = [c for c in range(32) if _to16_rne(sh2[c], dtype) == _to16_rne(np.float32(np.float32(16.0) * sc2[c] + sh2[c]), dtype)]
    assert set(frozen) <= set(stored_const) and len(stored_const) == (26 if dtype == "bf16" else 25)
    frozen = stored_const
    ims = parity_images[[1, 14, 30, 41, 52, 56, 60, 63]]
    for cf in (False, True):
        e = _capi.Engine(g, weights, device=0, dtype=dtype, max_batch=8, stage_launches=True, compute_frozen=cf)
        try:
            e.forward_u8(ims)
            t = e.tap("s2.bn", 8)
            for c in range(32):
                if c in frozen:
                    assert (t[..., c] == _to16_rne(sh2[c], dtype)).all(), (dtype, cf, c)       # (s2.bn is stored round-to-nearest-even)
            assert sum(np.unique(t[..., c]).size > 1 for c in range(32) if c not in frozen) >= 2      # (the live channels move)
        finally:
            e.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_results_are_reproducible_at_batch_160_in_both_arms(weights, parity_images, dtype):
    """Twelve passes over the same 160 images on one handle give the same bits every time -- stage tensors, probabilities, ids --
    on the default handle and on the computing arm (a counted wait one short, a ring slot reused too early would show here as a
    rare differing tile)."""
    g = build_graph(6, 224)
    ims = parity_images[(np.arange(160) * 7) % len(parity_images)]
    for cf in (False, True):
        e = _capi.Engine(g, weights, device=0, dtype=dtype, max_batch=160, compute_frozen=cf)
        try:
            ids0, probs0 = e.forward_u8(ims)
            t0 = {n: e.tap(n, 160) for n in ("s3.bn2", "s4.bn", "s5.bn2")}
            for rep in range(12):
                ids, probs = e.forward_u8(ims)
                np.testing.assert_array_equal(probs, probs0)
                np.testing.assert_array_equal(ids, ids0)
                if rep % 4 == 3:
                    for n, t in t0.items():
                        np.testing.assert_array_equal(e.tap(n, 160), t, err_msg="%s rep %d cf %s" % (n, rep, cf))
        finally:
            e.close()


@pytest.mark.parametrize("case", ["none", "stage2_only_15_and_17", "both_other_sets", "everything_of_stage2"])
def test_frozen_channel_fold_on_other_checkpoints(weights, parity_images, case):
    """The fold is a property of the CHECKPOINT, proven at rn_create: checkpoints whose frozen channels sit elsewhere (or nowhere)
    must fold what can be folded -- and only that -- and agree with the oracle on every stage output like the shipped one."""
    g = build_graph(6, 224)
    rng = np.random.default_rng(5)
    if case == "none":
        w, want = with_gammas(weights, [], [], 1), {"pair_channels_not_convolved": 0, "residual_stage_folded": -1}
    elif case == "stage2_only_15_and_17":
        # 15 frozen channels: one short of a half -> nothing folded in the pair; 31 in stage 5: one short of two quarters
        w, want = with_gammas(weights, rng.choice(32, 15, replace=False), rng.choice(64, 31, replace=False), 2), {"pair_channels_not_convolved": 0, "residual_stage_folded": -1}
    elif case == "both_other_sets":
        w, want = with_gammas(weights, rng.choice(32, 17, replace=False), rng.choice(64, 40, replace=False), 3), {"pair_channels_not_convolved": 16, "residual_stage_folded": 5, "residual_stage_live_quarters": 2}
    else:
        w, want = with_gammas(weights, range(32), range(64), 4), {"pair_channels_not_convolved": 24, "pair_channels_proven_frozen": 32, "residual_stage_folded": 5}
    ims = parity_images[[14, 30, 2, 52]]
    ref = c_oracle.infer(w, ims, taps=True)
    for dtype in ("bf16", "f16"):
        e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=4)
        try:
            info = e.frozen_info()
            for k, v in want.items():
                assert info[k] == v, (case, dtype, info)
            # round 6: the constant channels of s4.bn fold only behind a folded stage 5, and only with 16 channels that are both
            # constants of stage 4's 16-bit store and frozen channels of stage 5 (restated here in NumPy float32)
            sc4, sh4 = _bn_tables(w, 5, 16)
            c4 = {c for c in range(64) if _store16(sh4[c], dtype) == _store16(np.float32(np.float32(16.0) * sc4[c] + sh4[c]), dtype)}
            fz5 = _frozen5(w)
            ci = e.const_info()
            expect_fold = info["residual_stage_folded"] == 5 and len(c4 & fz5) >= 16
            assert ci["stage"] == (4 if expect_fold else -1), (case, dtype, ci, len(c4), len(fz5), len(c4 & fz5))
            if info["residual_stage_folded"] == 5:
                assert ci["channels_proven_constant"] == len(c4), (case, dtype, ci, len(c4))
            ids, probs = e.forward_u8(ims)
            for name in ("s1.bn", "s3.bn2", "s4.bn", "s5.bn2", "s8.bn"):
                got, ref_t = e.tap(name, 4), np.asarray(ref["taps"][name])
                rel = float(np.abs(got - ref_t).max() / max(np.abs(ref_t).max(), 1e-6))
                assert rel <= STAGE_TOL[dtype] * 1.5, (case, dtype, name, rel)
            assert np.abs(probs - ref["probs"]).max() <= 0.05
        finally:
            e.close()


@pytest.mark.parametrize("compute_frozen", [False, True])
def test_bound_launch_arguments_do_not_go_stale_between_calls(weights, parity_images, compute_frozen):
    """A handle's launch arguments are filled once at rn_create; a call copies them and sets only what depends on it (the bands of
    its batch size, the image pointer).  A field that a call left behind in the reused struct would show as a result that depends
    on the calls before it: one handle runs image buffer A at n = 1, buffer B at ceil(n_cu / 2) images (the back end in one
    launch), a grad-CAM (the back end split), A at n = 3 and B at n = 1, and every result is, byte for byte, that of a fresh
    handle given that one call."""
    import torch
    n_big = (torch.cuda.get_device_properties(0).multi_processor_count + 1) // 2
    g = build_graph(6, 224)
    kw = dict(device=0, dtype="bf16", max_batch=n_big, compute_frozen=compute_frozen)
    buf = {"A": parity_images[(np.arange(n_big) * 3) % len(parity_images)], "B": parity_images[(np.arange(n_big) * 5 + 1) % len(parity_images)]}
    assert not np.array_equal(buf["A"][:3], buf["B"][:3])
    taps = ("s3.bn2", "s5.bn2", "s9.bn2")          # (at the large batch the last one only: the others are ~100 MB as float32)

    def forward(e, d_im, n):
        d_probs, d_ids = e.device_malloc(n * 6 * 4), e.device_malloc(n * 8)
        try:
            e.forward_u8_device(d_im, n, d_probs, d_ids)
            e.sync()
            probs, ids = np.empty((n, 6), np.float32), np.empty((n,), np.int64)
            e.d2h(probs, d_probs)
            e.d2h(ids, d_ids)
            return [probs, ids] + [e.tap(t, n) for t in (taps if n <= 3 else taps[-1:])]
        finally:
            e.device_free(d_probs)
            e.device_free(d_ids)

    def upload(e):
        d = {}
        for k, v in buf.items():
            d[k] = e.device_malloc(v.nbytes)
            e.h2d(d[k], v)
        return d

    def release(e, d):
        for p in d.values():
            e.device_free(p)
        e.close()

    calls = [("A", 1), ("B", n_big), ("cam", 2), ("A", 3), ("B", 1)]
    reused = _capi.Engine(g, weights, **kw)
    d_reused = upload(reused)
    got = []
    try:
        for which, n in calls:
            if which == "cam":
                got.append(list(reused.grad_cam(buf["B"][:n])))
            else:
                got.append(forward(reused, d_reused[which], n))
                if n == n_big:
                    assert reused.launch_groups()[-1] == [6, 7, 8, 9]
    finally:
        release(reused, d_reused)
    for (which, n), have in zip(calls, got):
        fresh = _capi.Engine(g, weights, **kw)
        d_fresh = upload(fresh)
        try:
            want = list(fresh.grad_cam(buf["B"][:n])) if which == "cam" else forward(fresh, d_fresh[which], n)
        finally:
            release(fresh, d_fresh)
        assert len(have) == len(want)
        for k, (a, b) in enumerate(zip(have, want)):
            assert a.tobytes() == b.tobytes(), (which, n, compute_frozen, k)
