/*
 * roomnet_hip.h -- C ABI of libroomnet_hip.so, the MI355X (gfx950) implementation
 * of RoomNet's forward-pass inference path.
 *
 * The reference (ironhide23586/RoomNet) has no native / FFI interface: its
 * boundary is the Python API of network.RoomNet, which hands the whole forward
 * pass to TensorFlow through tf.Session.run.  This library replaces exactly
 * that hand-off.  Each entry point names the reference interface it replaces
 * (file:line into the reference tree); INTEGRATION.md shows the ctypes binding
 * a maintainer of the reference would add to network.py.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes in; the
 *     library owns its device memory, stream(s), events and packed weights.
 *   - every function returning int returns RN_OK (0) or a negative RN_E_* code;
 *     rn_last_error() returns a thread-local message for the last failure.
 *   - a handle is bound to one device and one stream; calls on one handle must
 *     be serialised by the caller (the reference is single-threaded,
 *     infer.py:79-82); distinct handles are independent.
 *   - the asynchronous calls of one handle that are in flight together share one
 *     stream: after rn_set_stream / rn_set_stream_null, rn_sync (on the old stream)
 *     comes before the next call.  The image stages (batched resize, JPEG decode,
 *     overlay + encode, heat maps) double-buffer their per-batch tables behind
 *     events, but their plane and coefficient scratch is single and ordered by the
 *     stream alone.
 *   - tensors are NHWC, C-contiguous.  Images are [n, S, S, 3].
 */
#ifndef ROOMNET_HIP_H
#define ROOMNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RN_API __attribute__((visibility("default")))
#else
#define RN_API
#endif

#define RN_OK 0
#define RN_E_INVALID (-1)   /* bad argument / unsupported graph                     */
#define RN_E_HIP (-2)       /* a HIP runtime call failed (message has the details) */
#define RN_E_NOMEM (-3)     /* host or device allocation failed                    */
#define RN_E_STATE (-4)     /* call not valid in the handle's current state        */
#define RN_E_RANGE (-5)     /* n exceeds max_batch, bad node id, buffer too small  */

/* storage / MFMA input type of activations and conv weights.  float32 everywhere on
 * RN_DTYPE_F32 handles: without RN_FLAG_TAPS their conv stages 1-6 run as one launch each on the
 * matrix cores (v_mfma_f32_32x32x2_f32: float32 in, float32 accumulate; rn_stage_f32m.hip), with
 * RN_FLAG_TAPS as one launch per graph node (every node readable); the two differ only in the order
 * of the convolution's K sum and of the pooling window sum (<= 2e-5 of a tensor's abs-max).
 * On the 16-bit handles: conv accumulation, ReLU6, BN, the vertical
 * part of the residual interpolation, the dense head and the softmax are float32; what is
 * NOT float32 (all inside the tolerances of tests/test_hip_fused.py):
 *   - stage 0 runs on fp16 MFMAs in BOTH 16-bit modes and is exact up to the float32 summation
 *     order: the operand is the uint8 pixel value itself, the pre-processing of network.py:129
 *     is folded into the weights, and every folded weight is an fp16 hi + lo pair in two idle
 *     rows of the 32 x 32 tile (rn_stage.h, s0_pixel_halves); only its OUTPUT is rounded to
 *     the storage type;
 *   - avg-pool 4x4 stride 1 (stages 1-3): ReLU6 outputs are rounded to fp16, vertical pair
 *     sums are fp16 adds, and the window sums run on the matrix cores (fp16 x 0/1 band
 *     matrix, exact float32 accumulation); stride-2 pools are float32 VALU sums, except
 *     stages 4 and 5 wherever the row-blocked kernels run (rn_stage4x.hip / rn_stage5x.hip: rows cut
 *     into column blocks of 194-206 / 66-110 input columns -- 224, 420 and 600 inputs all qualify),
 *     which pool like the stride-1 stages (fp16 ReLU6 outputs and pair sums, band-matrix MFMA);
 *   - every stage that pools fp16 values on the matrix cores (stages 1-3 always, 4 and 5 where
 *     the row-blocked kernels run) keeps its conv weights DIVIDED BY 6 (rounded to the 16-bit
 *     type after the division): relu6(6 x) / 6 = clamp(x, 0, 1) is then the free clamp of the
 *     fp16 conversion, and the folded BN scale carries the 6;
 *   - residual resize: the horizontal interpolation is an MFMA against the interpolation
 *     matrix in the storage type -- stage 3, and stage 5 on the row-blocked kernel: one operand, lerp
 *     fraction rounded to 2^-8 (bf16) / 2^-11 (fp16) so that both weights are exact;
 *     stage 9, and stage 5 on the round-2 kernel (RN_FLAG_PAIR_32X32): hi + lo split (~16-bit weights);
 *   - rounding (round 6, default; RN_FLAG_NO_DITHER restores plain rounding): the conv weights of stages 1-9 are converted to
 *     the storage type with the rounding residual CARRIED from tap to tap of every (cin, cout) pair -- a weight may be one ulp
 *     from its nearest value, the nine taps sum to the exact sum within half an ulp -- and bf16 handles store the outputs of
 *     stages 3, 4, 5 through v_cvt_sr_bf16_f32 with a seed that depends on the output row (1/6, 3/6, 5/6 of an ulp for rows
 *     0, 1, 2 mod 3): deterministic, each stored value within one ulp of the exact one;
 *   - channels rn_create proves constant are not computed at all (rn_frozen_info, rn_const_info): same bits as computing them. */
#define RN_DTYPE_F32 0      /* reference arithmetic type (TensorFlow float32)      */
#define RN_DTYPE_BF16 1
#define RN_DTYPE_F16 2

/* rn_create flags */
#define RN_FLAG_TAPS 1u     /* unfused per-node path; every graph node can be read
                               back with rn_tap (float32 only)                     */
#define RN_FLAG_STAGE_LAUNCHES 2u /* 16-bit handles: one launch per conv stage, every
                               stage output "sK.bn"/"sK.bn2" materialised in HBM (per-stage
                               parity taps).  Default: stages are fused across their
                               boundaries where a kernel exists (the output of a stage
                               that only feeds its fused successor is then never written:
                               s0.bn, s2.bn; and, when a call carries at least half as many images
                               as the device has CUs, s6.bn and s7.bn -- the back end then runs
                               as one launch per image, rn_backend.hip; rn_tap refuses them) */
#define RN_FLAG_GENERIC_KERNELS 4u /* 16-bit handles: every stage on the generic
                               stage_mfma_kernel (diagnostic cross-check of the tuned kernels) */
#define RN_FLAG_COMPUTE_FROZEN 16u /* convolve every channel.  By default channels that rn_create PROVES constant (the stored
                                    * value is the same number for every possible input: BN gammas the reference's L2
                                    * regulariser drove to ~1e-20) are written from a table instead of being convolved and
                                    * enter the next convolution as one constant per cout -- 16-bit handles (the fused
                                    * pair's on-chip tensor, the 64 -> 64 residual stage) and float32 matrix-core handles
                                    * (the same stages) alike; this flag is the comparison arm that shows it.  See
                                    * rn_frozen_info, rn_const_info (the 16 constant output channels of the first step of
                                    * the 64-channel block, round 6, are computed under this flag too). */
#define RN_FLAG_NO_DITHER 32u /* 16-bit handles: plain rounding everywhere -- conv weights rounded to nearest one by one and no
                                dithered store, as in rounds 1-5: every store rounds to nearest even, except that bf16 handles
                                still store the outputs of stages 3, 4, 5 through v_cvt_sr_bf16_f32 with the plain
                                (undithered) seed, which rounds half away from zero.  Default (round 6): the weights' rounding residual
                                is carried from tap to tap (the nine taps of a (cin, cout) pair sum to the exact sum within half an
                                ulp), and bf16 handles store the outputs of stages 3, 4, 5 through v_cvt_sr_bf16_f32 with a
                                seed that depends on the output row -- a deterministic dither, each value within one ulp of the
                                exact one -- so that the rounding errors of a 3 x 3 window cancel instead of adding on smooth
                                image content: max |dlogit| on the parity set 0.080 -> 0.030 (600 x 600: 0.126 -> 0.026; profiles/r6_c_parity.json).
                                Comparison arm. */
#define RN_FLAG_PAIR_32X32 8u /* 16-bit handles: the round-2 kernels instead of the round-3 ones (comparison
                               arm, bench.py --pair32): the cross-stage fused pair of the 32-channel block
                               (network.py:183-203: rn_stage23.hip instead of rn_stage23x.hip; equal up to the fp32 order of
                               the pooling sums: ~1 value in 4e7 differs, by one 16-bit ulp);
                               the first step of the 64-channel block, its residual step and the 128-channel
                               step (network.py:216-235: rn_stage_rw.hip / rn_conv16.hip instead of
                               rn_stage4x/5x/6x.hip; these differ in the last 16-bit place: other
                               accumulation order, pooling of stride-2 steps as fp16 band-matrix MFMAs); the
                               stage-0 fusion with wave-private rings instead of the shared ring (bit-identical).
                               TEST / A-B LIBRARY ONLY (round 6): the round-2 pair kernel is linked into
                               roomnet_amd/lib/libroomnet_hip_ab.so (same exports, csrc/build.sh builds both); the
                               product library answers this flag with RN_E_INVALID */
#define RN_FLAG_BATCH_STATS 64u /* RN_DTYPE_F32 only: every BN normalises with the moments of the batch being fed, the forward
                               pass of tf.layers.batch_normalization(training=True) -- what the reference's default
                               RoomNet(compute_bn_mean_var=True) computes (network.py:193, :202, :217).  Per-node float32 path
                               (no matrix-core stage kernels, no channel folding: rn_frozen_info / rn_const_info report
                               nothing); at each of the 16 BN nodes: per-channel mean and biased variance of the node's
                               input over n * h * w (dense BNs: over n), inv = rsqrt(var + eps) * gamma written on the
                               device, then the same BN kernel as an inference handle.  The checkpoint's moving_mean /
                               moving_variance are not read.  Every rn_forward_* / rn_submit_u8 call then depends on the
                               whole batch (n = 1: variance 0, every BN returns beta); rn_tap as on any per-node handle
                               (with RN_FLAG_TAPS: every node); rn_bn_batch_stats reads the moments back.  16-bit dtypes
                               and RN_FLAG_GENERIC_KERNELS / _STAGE_LAUNCHES / _PAIR_32X32: RN_E_INVALID; rn_grad_cam_*:
                               RN_E_STATE; groups: RN_E_INVALID (the moments would need an all-reduce) */

#define RN_MAX_STAGES 16
#define RN_MAX_DENSE 8
#define RN_NAME_LEN 32

typedef struct rn_handle rn_handle;

/* One conv stage = conv3x3 VALID stride-1 no-bias -> ReLU6 -> [avg-pool k,s VALID]
 * -> BN(inference) -> [ + legacy bilinear resize(output of skip_stage) -> BN ].
 * Mirrors one depth step of conv_block (reference network.py:172-208). */
typedef struct rn_conv_stage {
    int32_t cin, cout;
    int32_t pool_k, pool_s;   /* pool_k == 0: no pooling                            */
    int32_t skip_stage;       /* index of the stage whose output is added, or -1    */
    const float* kernel;      /* HWIO [3,3,cin,cout]         (convN/kernel)         */
    const float* gamma;       /* BN after the pool, [cout]   (batch_normalization_N)*/
    const float* beta;
    const float* mean;
    const float* variance;
    const float* gamma2;      /* BN after the residual add, or NULL                 */
    const float* beta2;
    const float* mean2;
    const float* variance2;
} rn_conv_stage;

/* One dense_block (reference network.py:210-223): x@W [+ bias] -> ReLU6 -> [BN] */
typedef struct rn_dense_layer {
    int32_t nin, nout;
    const float* kernel;      /* [nin, nout]                                        */
    const float* bias;        /* [nout] or NULL                                     */
    const float* gamma;       /* BN params or NULL (all four NULL together)         */
    const float* beta;
    const float* mean;
    const float* variance;
} rn_dense_layer;

/* The restored model: what RoomNet.__init__ + RoomNet.load build and restore
 * (reference network.py:21-48, :105-126).  Pointers are host memory and are
 * only read during rn_create. */
typedef struct rn_weights {
    int32_t im_side;          /* RoomNet(im_side=...)                               */
    int32_t num_classes;      /* RoomNet(num_classes=...)                           */
    int32_t n_stages;
    int32_t n_dense;
    float bn_epsilon;         /* tf.layers.batch_normalization default 1e-3         */
    const rn_conv_stage* stages;
    const rn_dense_layer* dense;
} rn_weights;

/* per-call device timing of the last rn_forward_* (HIP events on the handle's stream) */
typedef struct rn_stage_ms {
    int32_t n_stages;                 /* conv stages timed                          */
    float preprocess_ms;              /* uint8 -> float (only when it is a separate launch) */
    float stage_ms[RN_MAX_STAGES];    /* one fused launch (or launch group) per stage */
    float head_ms;                    /* flatten + dense blocks + softmax + argmax  */
    float total_ms;                   /* first launch -> last launch                */
} rn_stage_ms;

typedef struct rn_node_info {
    char name[RN_NAME_LEN];           /* "s3.conv", "s3.pool", "s3.bn", "s3.add", "s3.bn2", "d0.mm", ... */
    int32_t h, w, c;                  /* per-image shape (h = w = 1 for head nodes) */
} rn_node_info;

/* ---- lifetime ------------------------------------------------------------
 * rn_create replaces RoomNet.__init__(optimized_inference=True) + RoomNet.init()
 * + RoomNet.load(path) (reference network.py:21-48, :87-91, :105-126): it builds
 * the execution plan for `w`, packs/uploads the weights and sizes the workspace
 * for up to max_batch images per call.
 *
 * Supported im_side.  The graph needs im_side >= 183 (smaller: RN_E_INVALID).  A handle CLASSIFIES at im_side 183 .. 694:
 * the head kernel keeps the flatten (16 channels of the last conv stage's square output) in LDS, 4096 values at the most --
 * 16 x 16 x 16 at 663 .. 694, 17 x 17 x 16 = 4624 from 695 on.  rn_create accepts larger sides too: such a handle serves
 * rn_features_* (the features lie in front of the head; that pass launches no head and leaves the head's nodes unwritten), and
 * every call that classifies (rn_forward_*, rn_submit_u8, rn_grad_cam_*) enqueues the conv stages and then returns RN_E_STATE
 * with "flatten length 4624 exceeds head kernel capacity 4096"; the handle stays usable.  Inside 183 .. 694 the tuned 16-bit
 * kernels cut wide rows into one to four column blocks (the table of block counts per side). */
RN_API int rn_create(const rn_weights* w, int device, int dtype, int max_batch, unsigned flags, rn_handle** out);
RN_API void rn_destroy(rn_handle* h);
RN_API const char* rn_last_error(void);
RN_API int rn_device_count(void);
RN_API const char* rn_version(void);

/* ---- forward pass ----------------------------------------------------------
 * rn_forward_u8 replaces RoomNet.infer(im_batch) (reference network.py:128-135):
 * BGR uint8 [n,S,S,3] -> channel flip + ((x/255.)*2)-1 (float64 semantics, then
 * float32) -> graph -> (argmax int64 [n], softmax float32 [n,num_classes]).
 * Host buffers; blocks until the results are in probs/ids. */
RN_API int rn_forward_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, float* probs, int64_t* ids);

/* Two-slot pipelined form of rn_forward_u8 for a caller that classifies batch after batch from host memory (the
 * directory driver, infer.py:79-82, at batch size): rn_submit_u8 uploads the batch into the slot's device buffer on a
 * copy stream and enqueues its forward pass + result download behind it; rn_collect waits for that slot and copies the
 * results out.  With  submit(0) submit(1) collect(0) submit(0) collect(1) ...  the upload of one batch overlaps the kernels
 * of the previous one (from pageable memory the upload call itself blocks the calling thread, the GPU does not idle;
 * from pinned memory -- rn_host_alloc -- it is asynchronous: the caller then keeps the slot's source buffer unchanged
 * until rn_collect(slot) has returned, i.e. one pinned buffer per slot).  slot = 0 or 1; a slot must be collected before
 * it is submitted again. */
RN_API int rn_submit_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, int slot);
RN_API int rn_collect(rn_handle* h, int slot, float* probs, int64_t* ids);

/* rn_forward_f32 replaces sess.run(outs_final, {x_tensor: im}) (reference
 * network.py:133/:155) for an already pre-processed RGB float32 batch in [-1,1]. */
RN_API int rn_forward_f32(rn_handle* h, const float* rgb_nhwc, int n, float* probs, int64_t* ids);

/* Device-resident variants: all pointers are device memory on the handle's
 * device; the call only enqueues work on the handle's stream (asynchronous).
 * Use rn_sync (or your own event on the stream) before reading the outputs. */
RN_API int rn_forward_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, float* d_probs, int64_t* d_ids);
RN_API int rn_forward_f32_device(rn_handle* h, const float* d_rgb_nhwc, int n, float* d_probs, int64_t* d_ids);
/* The caller's image pipeline on the device -- RoomNet.center_crop + cv2.resize(INTER_LINEAR) of
 * RoomNet.infer_optimized (reference network.py:137-146, :152).  `d_src` is one BGR uint8 HWC image of any size
 * in device memory; its centred square window is resized to im_side x im_side into slot `index` of a device batch
 * buffer [max_batch, im_side, im_side, 3] that rn_forward_u8_device then takes.  Integer-exact restatement of
 * OpenCV's fixed-point algorithm (bit-identical to roomnet_amd/imageops.py).  Asynchronous on the handle's stream. */
RN_API int rn_crop_resize_u8_device(rn_handle* h, const uint8_t* d_src, int src_h, int src_w, uint8_t* d_dst_batch, int index);
/* The same for a BATCH of device-resident images in ONE launch: image i (d_srcs[i], heights[i] x widths[i] BGR uint8, HWC, any
 * sizes) is centre-cropped and resized into slot i of d_dst_batch ([n, S, S, 3]).  Asynchronous on the handle's stream;
 * n <= max_batch.  The arrays are copied before the call returns; back-to-back calls without a sync are fine (the batch table
 * is double-buffered behind events).  network.py:149-152 for a whole directory's worth of decoded images at once. */
RN_API int rn_crop_resize_batch_u8_device(rn_handle* h, const uint8_t* const* d_srcs, const int* heights, const int* widths, int n,
                                          uint8_t* d_dst_batch);
/* infer.py:79-82 for a whole batch: n host images of individual sizes heights[i] x widths[i] (BGR uint8 HWC) are
 * uploaded, centre-cropped, resized and classified; probs [n, num_classes], ids [n] on the host.  Synchronous. */
RN_API int rn_classify_images_u8(rn_handle* h, const uint8_t* const* images, const int* heights, const int* widths, int n,
                                 float* probs, int64_t* ids);
RN_API int rn_sync(rn_handle* h);

/* ---- baseline JPEG files, decoded where each half of the work belongs ------------------------------
 * cv2.imread of infer.py:81 for the files a camera writes.  A JPEG decode is serial up to the end of its Huffman pass and
 * per-pixel behind it, so it is split there: the host walks the markers and runs the Huffman pass into int16 coefficients
 * (rn_jpeg_probe, rn_jpeg_entropy_decode: pure functions, no device, safe on arbitrary bytes), the GPU dequantises, runs the
 * inverse DCT, upsamples the chroma and converts YCbCr to BGR (rn_jpeg_decode_batch_device), and the full-size BGR image never
 * exists in host memory.  The pixels are byte for byte those of libjpeg's default decode path (what Pillow and OpenCV return):
 * jpeg_idct_islow on coef * q (CONST_BITS 13, PASS1_BITS 2: columns descaled by 11, then rows by 18, then range_limit[v & 1023]),
 * "fancy" triangle upsampling of h2v1 / h2v2 chroma on the component's downsampled extent (plain replication when that is at most
 * 2 columns wide), the 16-bit fixed-point YCbCr -> RGB tables; roomnet_amd/jpegdec.py restates it in NumPy.
 *
 * rn_jpeg_probe           fills *out from the file's headers: size, 1 or 3 components, the luma sampling (1x1, 2x1 or 2x2; chroma
 *                         1x1), the restart interval, each component's padded block grid (whole MCUs), its quantisation table in
 *                         natural order, and `supported`.  Supported: SOF0, 8 bits, ONE interleaved Huffman scan of all
 *                         components, 8-bit tables, grey or component ids 1,2,3, no Adobe APP14 segment, EXIF orientation (APP1,
 *                         IFD0 tag 0x0112, either byte order) absent or 1, no orientation in an XMP packet.  Anything else that
 *                         is a JPEG -- progressive, arithmetic, 12-bit, CMYK, 1x2 / 4:1:1, several scans, DNL, orientation 2-8 --
 *                         is RN_OK with supported = 0 and the reason in `reason`: a file for the general decoder.  RN_E_INVALID:
 *                         not a JPEG, or its headers are truncated.
 * rn_jpeg_entropy_decode  the Huffman pass of a supported file (table-lookup decoder; DC prediction, EOB / ZRL, FF 00 stuffing,
 *                         RSTn with predictor reset): quantised coefficients [component][block_y][block_x][64], natural order,
 *                         into coeffs; cap = int16 elements available (rn_jpeg_coeff_count of them are written; fewer:
 *                         RN_E_RANGE).  Truncated scan data, an invalid code, a run past the block, or a dequantised coefficient
 *                         |coef * q| > RN_JPEG_COEF_LIMIT: RN_E_INVALID, with nothing read or written out of range.
 * RN_JPEG_COEF_LIMIT      the pixel stage keeps 32-bit intermediates.  Every intermediate of a 1-D pass of jpeg_idct_islow is a
 *                         linear form of its 8 inputs whose absolute coefficients sum to at most 61214 (an output), so with
 *                         |coef * q| <= B no value of the column pass exceeds 61214 B + 2^10, its results are at most
 *                         W = (61214 B + 2^10) >> 11, and no value of the row pass exceeds 61214 W + 2^17: below 2^31 for
 *                         B <= 1173.  The SIMD code libjpeg-turbo really runs keeps the column pass's results in 16 bits and
 *                         saturates them, so parity with it is defined while W <= 32767: B <= 1096, the smaller of the two and
 *                         the limit.  An 8-bit image's own coefficients stay below 1016 + q / 2.
 * rn_jpeg_decode_batch_device  the pixel stage of n images of individual sizes and samplings: the coefficients (host memory;
 *                         from rn_host_alloc memory the upload is asynchronous, and the buffers then stay unchanged until
 *                         rn_sync) go up on the handle's copy stream, then TWO launches for the whole batch on the handle's
 *                         stream -- inverse DCT into planar Y / Cb / Cr scratch, then upsampling + colour + interleave -- write image
 *                         i as BGR uint8 HWC, height x width x 3 tightly packed, to d_bgr[i]: the layout
 *                         rn_crop_resize_batch_u8_device takes.  Asynchronous; back-to-back calls without a sync are fine (the
 *                         batch table is double-buffered behind events, the scratch is ordered by the streams).
 *                         n outside [1, max_batch]: RN_E_RANGE; an image
 *                         whose info is not a supported one as rn_jpeg_probe fills it: RN_E_INVALID; the handle stays usable.
 * rn_classify_jpegs       rn_classify_images_u8 for coefficient images: decoded into scratch the handle owns (allocated by the
 *                         first call, grown as needed, freed by rn_destroy), centre-cropped, resized and classified; probs and
 *                         ids are bit-identical to rn_classify_images_u8 of the same files decoded by libjpeg.  Synchronous.
 * rn_jpeg_last_decode_ms  device time of the last call's two pixel-stage launches (events on the handle's stream); waits for them. */
#define RN_JPEG_COEF_LIMIT 1096
#define RN_JPEG_REASON_LEN 48
typedef struct rn_jpeg_info {
    int32_t width, height;
    int32_t ncomp;                    /* 1 (grey) or 3 (YCbCr)                      */
    int32_t hsamp, vsamp;             /* luma sampling: 1x1, 2x1 or 2x2             */
    int32_t restart_interval;         /* MCUs between RSTn markers, 0: none         */
    int32_t blocks_w[3], blocks_h[3]; /* per component: 8x8 blocks, whole MCUs      */
    int32_t supported;                /* 0: no; 1: yes; 2..8 (the oriented probes): yes, turned by that EXIF orientation */
    uint16_t qt[3][64];               /* per component, natural (row-major) order   */
    char reason[RN_JPEG_REASON_LEN];  /* why supported == 0                         */
} rn_jpeg_info;
typedef struct rn_jpeg_image {
    rn_jpeg_info info;
    const int16_t* coeffs;            /* host: what rn_jpeg_entropy_decode wrote    */
} rn_jpeg_image;
RN_API int rn_jpeg_probe(const uint8_t* data, size_t len, rn_jpeg_info* out);
RN_API size_t rn_jpeg_coeff_count(const rn_jpeg_info* info);
RN_API int rn_jpeg_entropy_decode(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap);
RN_API int rn_jpeg_decode_batch_device(rn_handle* h, const rn_jpeg_image* ims, int n, uint8_t* const* d_bgr);
RN_API int rn_classify_jpegs(rn_handle* h, const rn_jpeg_image* ims, int n, float* probs, int64_t* ids);
RN_API int rn_jpeg_last_decode_ms(rn_handle* h, float* ms);

/* ---- the Huffman pass of those files on the GPU --------------------------------------------------
 * DESIGN.md section 18.  A Huffman bit stream can be decoded from many speculative start points whose decoder states converge
 * after a few symbols, so the pass above is not serial: the host keeps the marker walk, the file's scan bytes go up as they are,
 * and the coefficients are produced in device memory in the layout the pixel stage reads.  The scan is cut into subsequences of
 * RN_JPEG_SUBSEQ_BYTES raw bytes; per batch: (1) one lane per subsequence decodes from a guessed state and stores its exit state;
 * (2) lanes decode again from their left neighbour's stored state until nothing changes, inside groups of 256 subsequences and
 * then across groups; (3) the coefficients are zeroed, the block counts scanned, and every lane decodes from its entry state
 * with the coefficient writer and CHECKS that its exit state is the next lane's entry state; (4) the DC differences are summed
 * per component with the predictor reset at every restart interval.  A chain of states that is consistent from subsequence 0
 * is the sequential decode, so the check of (3) makes the result exact whatever (2) did.  Opt-in: nothing above changes.
 *
 * The status of an image (int32):
 *   RN_JPEG_ST_OK              the coefficients equal rn_jpeg_entropy_decode's byte for byte
 *   RN_JPEG_ST_INVALID_CODE .. RN_JPEG_ST_COEF_LIMIT   what rn_jpeg_entropy_decode refuses: a code no table has, an AC run past
 *                              the block, scan data that ends before the last block, a restart marker that is missing, early or
 *                              misnumbered, |coef * q| > RN_JPEG_COEF_LIMIT
 *   RN_JPEG_ST_NOT_SYNCED      the chain of states was not consistent (or more than 16 fill bytes precede a restart marker)
 *   RN_JPEG_ST_TOO_LARGE       a scan of more than 16 MiB
 * Every file rn_jpeg_entropy_decode refuses gets a non-zero status; the two last ones are the only ones a file it accepts may
 * get, and the caller then runs rn_jpeg_entropy_decode for that file.  With several findings the largest code is reported.  The
 * coefficients of an image with a non-zero status are unspecified (inside its buffer).
 *
 * rn_jpeg_scan_probe      rn_jpeg_probe's walk again, for what rn_jpeg_info does not hold: the byte range of the scan (to the
 *                         end of the data; the decoders stop at the marker that ends it) and the built lookup tables of each
 *                         component's DC / AC Huffman table.  Returns what rn_jpeg_probe returns; *out is zero for a file that
 *                         is not supported.
 * rn_jpeg_huffman_model   the four phases on the host, lanes one after another through the same code (csrc/rn_jpeg_huff.h), for
 *                         any subsequence length 4 .. 4096 (else RN_E_RANGE): the CPU statement of the algorithm.  Arguments and
 *                         refusals as rn_jpeg_entropy_decode; RN_OK with the image's status in *status otherwise.
 * rn_jpeg_huffman_batch_device  n files (info and scan as the two probes filled them, bytes = the scan's bytes in host memory,
 *                         data + scan_begin; from rn_host_alloc memory the upload is asynchronous): the scan bytes go up on the
 *                         handle's copy stream, then the launches of the four phases for the whole batch on the handle's stream
 *                         write image i's coefficients to d_coeffs[i] (device, rn_jpeg_coeff_count elements), or into the
 *                         handle's coefficient scratch when d_coeffs is NULL.  Waits for its own launches and fills status[n].
 *                         n outside [1, max_batch]: RN_E_RANGE; an info that is not a supported one, a null pointer: RN_E_INVALID;
 *                         the handle stays usable.
 * rn_jpeg_huffman_batch   the same into host buffers (coefficients of images with status 0 are copied).  Synchronous.
 * rn_classify_jpeg_files  rn_classify_jpegs from the files' bytes: the Huffman launches, the two pixel-stage launches on the
 *                         device coefficients, crop + resize + forward pass.  An image with a non-zero status gets id -1 and
 *                         zero probabilities and does not disturb the others.  Synchronous.
 * rn_jpeg_last_huffman_ms device time of the last call's Huffman launches; waits for them.
 * rn_jpeg_last_huffman_rounds  for the n images of the last call: the rounds phase 2 took inside groups (the most of any group)
 *                         and across groups; waits for them. */
#define RN_JPEG_ST_OK 0
#define RN_JPEG_ST_INVALID_CODE 1
#define RN_JPEG_ST_RUN_PAST_BLOCK 2
#define RN_JPEG_ST_TRUNCATED 3
#define RN_JPEG_ST_RESTART 4
#define RN_JPEG_ST_COEF_LIMIT 5
#define RN_JPEG_ST_NOT_SYNCED 6
#define RN_JPEG_ST_TOO_LARGE 7
typedef struct rn_jpeg_hufftab {
    uint16_t look[512];               /* (length << 8) | symbol of the code that is a prefix of the 9-bit index; 0: longer */
    int32_t maxcode[18];              /* largest code of length l, -1: none         */
    int32_t valoff[17];               /* vals index of the first code of length l minus that code */
    uint8_t vals[256];
} rn_jpeg_hufftab;
typedef struct rn_jpeg_scan {
    uint64_t scan_begin, scan_len;    /* bytes of the file: [scan_begin, scan_begin + scan_len) */
    rn_jpeg_hufftab dc[3], ac[3];     /* per component                              */
} rn_jpeg_scan;
typedef struct rn_jpeg_file {
    rn_jpeg_info info;
    rn_jpeg_scan scan;
    const uint8_t* bytes;             /* host, the scan's bytes                     */
} rn_jpeg_file;
RN_API int rn_jpeg_scan_probe(const uint8_t* data, size_t len, rn_jpeg_scan* out);
RN_API int rn_jpeg_huffman_model(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap,
                                 int subseq_bytes, int32_t* status);
RN_API int rn_jpeg_huffman_batch_device(rn_handle* h, const rn_jpeg_file* files, int n, int16_t* const* d_coeffs, int32_t* status);
RN_API int rn_jpeg_huffman_batch(rn_handle* h, const rn_jpeg_file* files, int n, int16_t* const* coeffs_host, int32_t* status);
RN_API int rn_classify_jpeg_files(rn_handle* h, const rn_jpeg_file* files, int n, float* probs, int64_t* ids, int32_t* status);
RN_API int rn_jpeg_last_huffman_ms(rn_handle* h, float* ms);
RN_API int rn_jpeg_last_huffman_rounds(rn_handle* h, int n, int32_t* inside, int32_t* across);

/* ---- files with an EXIF orientation, turned where the pixels are stored ---------------------------
 * DESIGN.md section 20.  A camera held upright writes its JPEG in sensor geometry with EXIF orientation 6 or 8 (front cameras:
 * 2, 4, 5, 7), and the general decoder turns the pixels after decoding them.  Coefficients, inverse DCT and chroma upsampling
 * belong to the STORED geometry (the IDCT's two passes round differently and the "fancy" filters are not symmetric), so the turn
 * is the address the pixel stage's last kernel stores each pixel at.  Opt-in: rn_jpeg_probe and rn_jpeg_scan_probe are what they
 * were, and so is every call on the infos they fill.
 *
 * rn_jpeg_info.supported  0: not supported; 1: supported, upright; k in 2..8: supported, and the decoded pixels are to be turned by
 *                         EXIF orientation k.  Only the two probes below write 2..8.  width, height, blocks_w / blocks_h stay those
 *                         of the STORED image whatever `supported` is.  With I the stored height x width image (H x W) the image O
 *                         the pixel stage writes is, as Pillow's ImageOps.exif_transpose gives it:
 *                             2: O[y][x] = I[y][W-1-x]        3: I[H-1-y][W-1-x]     4: I[H-1-y][x]                    (O is H x W)
 *                             5: O[y][x] = I[x][y]   6: I[H-1-x][y]   7: I[H-1-x][W-1-y]   8: I[x][W-1-y]              (O is W x H)
 * rn_jpeg_probe_oriented  rn_jpeg_probe, except that an EXIF orientation is no refusal: supported = 1..8.  The first "Exif\0\0"
 *                         APP1 segment decides; a tag value outside 2..8 reads as 1; supported = 0 with a reason for a later Exif
 *                         segment whose own reading differs from the first one's ("conflicting EXIF segments"), for an orientation
 *                         entry that is not one SHORT, for an orientation in an XMP packet, and for everything rn_jpeg_probe refuses
 *                         otherwise.
 * rn_jpeg_scan_probe_oriented  rn_jpeg_scan_probe on that walk: returns what rn_jpeg_probe_oriented returns; *out is zero for a file
 *                         that is not supported.
 * rn_jpeg_oriented_size   the size of O for a supported info: the stored one, swapped for 5..8.  An info that is not a supported
 *                         one, a null pointer: RN_E_INVALID.
 * rn_jpeg_entropy_decode, rn_jpeg_huffman_model  walk the headers by the oriented rules exactly when info->supported is 2..8, and
 *                         then also refuse (RN_E_INVALID) bytes whose orientation is not info->supported.  The coefficients are
 *                         those of the same file without its APP1 segment, byte for byte.
 * rn_jpeg_decode_batch_device, rn_classify_jpegs, rn_jpeg_huffman_batch[_device], rn_classify_jpeg_files  take infos with supported
 *                         1..8 (anything else: RN_E_INVALID).  d_bgr[i] receives O, rn_jpeg_oriented_size's height x width x 3
 *                         tightly packed (the same number of bytes as I), and the centre crop is O's.  A batch of upright images
 *                         is enqueued as before: the same two launches with the same grids.  Orientations 2..4 are stored by the
 *                         same colour launch (the 12-byte run of 4 pixels goes to the mirrored address); a batch that holds an
 *                         image of orientation 5..8 gets a THIRD launch, which turns 64 x 64 tiles of those images through LDS so
 *                         that the stores stay runs of 192 contiguous bytes; rn_jpeg_last_decode_ms spans all of them. */
RN_API int rn_jpeg_probe_oriented(const uint8_t* data, size_t len, rn_jpeg_info* out);
RN_API int rn_jpeg_scan_probe_oriented(const uint8_t* data, size_t len, rn_jpeg_scan* out);
RN_API int rn_jpeg_oriented_size(const rn_jpeg_info* info, int* height, int* width);

/* ---- the overlay and the output JPEG, written where the image already is --------------------------
 * cv2.putText and cv2.imwrite of infer.py:89-93 for an image the GPU holds.  An encode is the decode
 * above mirrored and splits at the same place: colour conversion, chroma downsampling, forward DCT and quantisation are per pixel
 * or per block and run on the GPU; only the Huffman pass is serial and runs on the host, on the int16 coefficients the GPU sends
 * back (1.5 x 2 B per pixel, and no BGR image in host memory).  The file is byte for byte the one libjpeg's default path writes
 * for quality q at 4:2:0 (what Pillow's save(format="JPEG", quality=q) and cv2.imwrite write): the fixed-point RGB -> YCbCr of
 * jccolor.c, h2v2_downsample with its alternating bias and expand_right_edge, jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2) on
 * sample - 128, the quantiser sign(c) * ((|c| + 4 q) / (8 q)); roomnet_amd/jpegenc.py restates it in NumPy.  Edge rules: rows are
 * extended to the luma block grid by their last column BEFORE downsampling, one row is added below only when the height is odd,
 * each downsampled component is then extended to its block grid by its own last row; luma blocks beyond ceil(w / 8) x
 * ceil(h / 8) are not transformed: their AC is 0 and their DC is that of the block before them in MCU order.
 * 32-bit intermediates are exact: |sample - 128| <= 128, a 1-D pass of jpeg_fdct_islow before its descale is a linear form whose
 * absolute coefficients sum to at most 8 * 8192 * 1.39 < 2^17 (outputs 0 and 4 sum to 8), so the row pass stays below
 * 128 * 2^17 = 2^24 and its results below 2^13 + 1; the column pass then stays below 2^13 * 2^17 + 2^14 < 2^31.
 *
 * rn_jpeg_encode_info     fills *out for a width x height file of quality 1..100 as rn_jpeg_probe would for that file: 3 components,
 *                         luma 2x2, whole-MCU block grids, libjpeg's scaling of the Annex K tables, supported = 1.  Sizes outside
 *                         1..65535 or another quality: RN_E_INVALID.
 * rn_jpeg_encoded_bound   bytes that always suffice for the file of such an info (0 for another info).
 * rn_jpeg_entropy_encode  writes the whole file into out[0 .. cap): SOI, APP0 (JFIF 1.01), two DQT, SOF0, the four Annex K DHT
 *                         (DC0, AC0, DC1, AC1), one interleaved SOS, the scan (DC differences per component, ZRL / EOB runs, FF
 *                         stuffing, the last byte padded with 1-bits, no restart markers), EOI.  coeffs: the layout
 *                         rn_jpeg_entropy_decode writes.  *len = the file's size; more than cap: RN_E_RANGE with nothing stored
 *                         past cap.  A DC difference above category 11, an AC value above category 10, or an info that
 *                         rn_jpeg_encode_info does not fill (grey, other samplings, inconsistent grids): RN_E_INVALID.
 * rn_jpeg_overlay_batch_device  draws each image's overlays in place, IN ORDER: per pixel of a box and per channel, in float32
 *                         without contraction, v = v + (colour - v) * coverage, then round-half-even, clamp, store as uint8 --
 *                         what hershey.put_text computes from the same coverage.  One launch per overlay rank for the whole
 *                         batch.  The coverage arrays are copied before the call returns.  Asynchronous.
 * rn_jpeg_encode_batch_device  the same, then the pixel stage of the encode in two launches for the whole batch (colour +
 *                         padding + downsampling into planar scratch; forward DCT + quantisation), then the coefficients go to
 *                         `coeffs` on the handle's copy stream (from rn_host_alloc memory that is asynchronous): rn_sync before
 *                         reading them.  Scratch belongs to the handle, grows as needed and is freed by rn_destroy; back-to-back
 *                         calls without a sync are fine (the batch tables are double-buffered behind events).
 *                         n outside [1, max_batch]: RN_E_RANGE.  An info that rn_jpeg_encode_info does not fill, a null image or
 *                         coefficient pointer, more than RN_JPEG_MAX_OVERLAYS overlays, an empty box, one not inside the image or
 *                         one without coverage: RN_E_INVALID.  In both cases nothing is enqueued and the handle stays usable.
 * rn_jpeg_last_encode_ms  device time of the last rn_jpeg_encode_batch_device call's launches; waits for them. */
#define RN_JPEG_MAX_OVERLAYS 8
typedef struct rn_jpeg_overlay {      /* one putText line, rasterised by the caller */
    int32_t x, y, w, h;               /* box inside the image                      */
    uint8_t color_bgr[3];
    const float* coverage;            /* host, [h, w] float32 in [0, 1]            */
} rn_jpeg_overlay;
typedef struct rn_jpeg_source {
    uint8_t* d_bgr;                   /* device, HWC, tightly packed: what rn_jpeg_decode_batch_device wrote */
    rn_jpeg_info info;                /* rn_jpeg_encode_info of its size           */
    const rn_jpeg_overlay* overlays;  /* applied IN ORDER, in place                */
    int32_t n_overlays;
    int16_t* coeffs;                  /* host (rn_host_alloc: the download is asynchronous) */
} rn_jpeg_source;
RN_API int rn_jpeg_encode_info(int width, int height, int quality, rn_jpeg_info* out);
RN_API size_t rn_jpeg_encoded_bound(const rn_jpeg_info* info);
RN_API int rn_jpeg_entropy_encode(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len);
RN_API int rn_jpeg_overlay_batch_device(rn_handle* h, const rn_jpeg_source* srcs, int n);
RN_API int rn_jpeg_encode_batch_device(rn_handle* h, const rn_jpeg_source* srcs, int n);
RN_API int rn_jpeg_last_encode_ms(rn_handle* h, float* ms);

/* ---- the Huffman pass of the output file on the GPU -----------------------------------------------
 * DESIGN.md section 19.  The encode's Huffman pass has no serial dependency that a prefix sum does not remove: a block's code
 * lengths depend on the block and on one earlier DC at a known address, bit positions are an exclusive scan of the lengths, and
 * FF 00 stuffing is a second scan.  Per batch of images of individual sizes: (1) LENGTHS: a wave per block, a lane per zigzag
 * position, writes the block's bit count; (2) OFFSETS: the exclusive scan of the counts per image in scan (MCU) order, whose
 * last element is the image's unstuffed bit total; (3) SCATTER: every block's bits go to its offset in a zeroed, unstuffed
 * stream (a block's inner words are stored, the first and last are merged with atomicOr, which commutes: the bytes repeat from
 * call to call), the last byte padded with 1-bits; (4) STUFF: the FF bytes per chunk are counted and scanned, byte i goes to
 * i + (FF bytes in front of it) with 00 behind every FF, then FF D9.  Order between phases is the launches' order; the host reads
 * the n bit totals after (2) and the n lengths after the counting half of (4) to size the streams, so the calls are synchronous.
 * Opt-in: nothing above changes.  No coefficient leaves the device in rn_jpeg_encode_files_device.
 *
 * The status of an image (int32):
 *   RN_JPEG_ENC_ST_OK         files[i][0 .. lens[i]) is the file rn_jpeg_entropy_encode writes, byte for byte
 *   RN_JPEG_ENC_ST_CATEGORY   a DC difference beyond category 11 or an AC value beyond category 10: what rn_jpeg_entropy_encode
 *                             refuses in the coefficients, every case of it (lens[i] = 0)
 *   RN_JPEG_ENC_ST_CAP        the file needs more than caps[i] bytes; lens[i] is what it needs; nothing is stored past caps[i]
 *   RN_JPEG_ENC_ST_TOO_LARGE  more than RN_JPEG_HUFFENC_MAX_BLOCKS blocks (32-bit bit offsets: 1658 bits per block at most);
 *                             decided from the info alone, before the coefficients are read or anything is enqueued for the image
 * A non-zero status for one image does not disturb the others of the batch; the caller runs rn_jpeg_entropy_encode for it.
 *
 * rn_jpeg_encode_headers  SOI .. SOS of the file of an info rn_jpeg_encode_info fills, the first bytes rn_jpeg_entropy_encode
 *                         writes (the same code): *len bytes; more than cap: RN_E_RANGE with nothing stored past cap.
 * rn_jpeg_huffenc_model   the four phases on the host, work item after work item through the same code (csrc/rn_jpeg_huffenc.h):
 *                         the CPU statement of the algorithm.  Arguments as rn_jpeg_entropy_encode's; a null pointer or an info
 *                         rn_jpeg_encode_info does not fill: RN_E_INVALID; RN_OK with the image's status in *status otherwise.
 * rn_jpeg_huffenc_batch   the kernels alone on arbitrary coefficients: coeffs_host[i] (rn_jpeg_coeff_count elements) go up, the
 *                         four phases run, and the whole file -- the headers, written by the host, the scan and EOI behind them --
 *                         arrives in files[i][0 .. caps[i]) (host; from rn_host_alloc memory the copy is asynchronous inside the
 *                         call).  lens[n], status[n] are filled.  Synchronous.
 * rn_jpeg_encode_files_device  rn_jpeg_encode_batch_device's overlays and pixel stage, then the four phases on the coefficients
 *                         where they are, in device scratch; srcs[i].coeffs is ignored and may be NULL.  Synchronous.
 *                         Both: n outside [1, max_batch]: RN_E_RANGE; a null pointer, an info rn_jpeg_encode_info does not fill,
 *                         and for the second what rn_jpeg_encode_batch_device refuses in a source: RN_E_INVALID; nothing is
 *                         enqueued and the handle stays usable.  Scratch belongs to the handle and grows to the streams' real
 *                         sizes; when it cannot (RN_E_NOMEM), the call returns before the scatter is enqueued.
 * rn_jpeg_last_huffenc_ms device time of the last call's launches of the four phases (the host's reads between them excluded);
 *                         waits for them. */
#define RN_JPEG_ENC_ST_OK 0
#define RN_JPEG_ENC_ST_CATEGORY 1
#define RN_JPEG_ENC_ST_CAP 2
#define RN_JPEG_ENC_ST_TOO_LARGE 3
#define RN_JPEG_HUFFENC_MAX_BLOCKS (0xFFFFFFFFu / 1658u)
RN_API int rn_jpeg_encode_headers(const rn_jpeg_info* info, uint8_t* out, size_t cap, size_t* len);
RN_API int rn_jpeg_huffenc_model(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len, int32_t* status);
RN_API int rn_jpeg_huffenc_batch(rn_handle* h, const rn_jpeg_info* infos, const int16_t* const* coeffs_host, int n,
                                 uint8_t* const* files, const size_t* caps, size_t* lens, int32_t* status);
RN_API int rn_jpeg_encode_files_device(rn_handle* h, const rn_jpeg_source* srcs, int n, uint8_t* const* files, const size_t* caps,
                                       size_t* lens, int32_t* status);
RN_API int rn_jpeg_last_huffenc_ms(rn_handle* h, float* ms);

/* Run on a caller-provided hipStream_t (e.g. the framework's current stream)
 * instead of the handle's own; NULL restores the handle's stream (a non-blocking stream,
 * NOT ordered against the HIP null stream).  rn_set_stream_null selects the HIP null
 * (legacy default) stream itself, which a NULL argument cannot express: use it when the
 * caller's other work is on the default stream and must be ordered with the library's. */
RN_API int rn_set_stream(rn_handle* h, void* hip_stream);
RN_API int rn_set_stream_null(rn_handle* h);

/* ---- grad-CAM class-evidence maps ---------------------------------------------
 * Where in the image did the network see class c?  For image i and class c_i (class_ids[i], or
 * the argmax of this call's own softmax when class_ids is NULL):
 *   S     = z[c_i], z = node "d3.mm": the last dense layer's x @ W + b BEFORE its ReLU6
 *           (reference network.py:237).  The reference applies ReLU6 to its logits, whose gradient
 *           is zero wherever the winning logit is <= 0 or >= 6 -- and a confident prediction can
 *           sit exactly there; the pre-activation is the only score that always has a gradient.
 *   A     = layer_node, the rn_node_info id of "s6.bn" (the 128-channel conv_block, 46 x 46 at
 *           224, 140 x 140 at 600) or "s7.bn" (first step of the last block, 21 x 21 x 16 at 224,
 *           68 x 68 x 16 at 600), as this call's forward pass stored it.  Other nodes: RN_E_INVALID.
 *   G     = dS/dA in float32 with TensorFlow's gradient rules: Relu6Grad passes where 0 < x < 6
 *           (pre-activations recomputed from the stored activations), AvgPool VALID spreads g/k^2
 *           over each (overlapping) window, inference BN multiplies by gamma/sqrt(var+eps), Add
 *           sends g to both inputs (s7.bn gets gradient through conv 8 AND the stage-9 skip), the
 *           legacy ResizeBilinear takes its transpose, MatMul the transposed kernel.
 *   alpha[c]  = mean over (y, x) of G[y, x, c]           -> alpha [n, c] (may be NULL)
 *   cam[y, x] = max(0, sum_c alpha[c] A[y, x, c])         -> cam [n, h, w], float32, not normalised
 * probs / ids are bit-identical to rn_forward_u8 of the same batch on the same handle.  On 16-bit
 * handles the call runs the back end as its split launches (stage 6, stage 7, the tail) whatever
 * n is, so that s6.bn and s7.bn are written; that choice is per call.  Runs on the handle's stream.
 * RN_E_INVALID (with a message) for an unsupported layer, class_ids[i] outside [0, num_classes)
 * or n outside [1, max_batch]; the handle stays usable.  The first call allocates the adjoint's
 * device workspace (sized for max_batch; freed by rn_destroy).  The host entry points block;
 * the device one only enqueues (its class ids, when given, are read back first to be checked). */
RN_API int rn_grad_cam_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, const int32_t* class_ids, int layer_node, float* cam,
                          float* alpha, float* probs, int64_t* ids);
RN_API int rn_grad_cam_f32(rn_handle* h, const float* rgb_nhwc, int n, const int32_t* class_ids, int layer_node, float* cam,
                           float* alpha, float* probs, int64_t* ids);
RN_API int rn_grad_cam_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, const int32_t* d_class_ids, int layer_node,
                                 float* d_cam, float* d_alpha, float* d_probs, int64_t* d_ids);

/* ---- grad-CAM heat maps drawn on the images the GPU holds ------------------------------------------
 * roomnet_amd/cam.py's overlay_image for images in device memory: what turns a map of rn_grad_cam_* into a
 * picture, between rn_jpeg_decode_batch_device and rn_jpeg_encode_batch_device, without the full-size image visiting the host.
 * The heat goes on the square the network saw, the centred window of rn_crop_resize_*: side c = min(height, width), offset
 * abs((width - height) // 2) along the longer axis with Python's floor division (a portrait image with an odd difference rounds
 * the offset UP); the rest of the image is untouched.  Per window pixel (y, x) and per channel, in float64, every product, sum and
 * quotient rounded on its own (no contraction), in cam.py's order:
 *   src  = (i + 0.5) * (n_in / double(c)) - 0.5 clipped to [0, n_in - 1], lo = floor(src), hi = min(lo + 1, n_in - 1),
 *          frac = src - lo                                   per axis (n_in = cam_h for i = y, cam_w for i = x)
 *   up   = max((a (1 - xl) + b xl) (1 - yl) + (c (1 - xl) + d xl) yl, 0)   from the four map neighbours
 *   v    = float32(up / mx), mx = the maximum of up over the window; mx = 0 (no positive entry): v = 0, the ramp's first anchor
 *   heat = rint(A[i] (1 - t) + A[i + 1] t), i = min(floor(4 v), 3), t = 4 v - i, A = the five BGR anchors (128,0,0) (255,255,0)
 *          (0,255,0) (0,255,255) (0,0,255)
 *   out  = clip(rint((1 - weight) * image + weight * heat), 0, 255), stored as uint8 in place; rint rounds half to even.
 * The bytes are those of cam.overlay_image of the same image, map and weight.  c = 1 and c < cam_h (the map is sampled down) are
 * ordinary cases.  Map entries are taken as finite.
 *
 * rn_cam_overlay_batch_device  n images of individual sizes, each with a map of its own size, in two launches for the whole batch
 *                         (the maxima -- an order-free maximum, the same bits in every schedule; then upsampling again, colour and
 *                         blend).  Asynchronous on the handle's stream, so ordered behind the calls that wrote the images and the
 *                         maps and in front of a following rn_jpeg_overlay_batch_device / rn_jpeg_encode_batch_device (the heat is
 *                         under the text); the targets are copied before the call returns.  The maxima and the batch tables belong
 *                         to the handle (allocated by the first call, double-buffered behind events, freed by rn_destroy):
 *                         back-to-back calls without a sync are fine.
 *                         n outside [1, max_batch]: RN_E_RANGE.  A null image or map pointer, a size outside 1..65535, a weight
 *                         outside [0, 1] or NaN: RN_E_INVALID.  In both cases nothing is enqueued and the handle stays usable.
 * rn_cam_last_overlay_ms  device time of the last rn_cam_overlay_batch_device call's launches; waits for them. */
typedef struct rn_cam_target {
    uint8_t* d_bgr;                   /* device, HWC, tightly packed                */
    int32_t height, width;
    const float* d_cam;               /* device map, e.g. one image's slice of rn_grad_cam_u8_device's d_cam */
    int32_t cam_h, cam_w;
} rn_cam_target;
RN_API int rn_cam_overlay_batch_device(rn_handle* h, const rn_cam_target* targets, int n, double weight);
RN_API int rn_cam_last_overlay_ms(rn_handle* h, float* ms);

/* ---- occlusion-sensitivity maps ------------------------------------------------------------------
 * An input-resolution answer to "where did the network see class c?" that needs no backward pass: cover a
 * square of the network's input, run the forward pass, record how far the class probability falls, slide the square.  For a
 * handle of side S, patch side P and stride T with 1 <= T <= P <= S (roomnet_amd/occlusion.py states the same in NumPy):
 *   positions  per axis p_k = min(k T, S - P) for k = 0 .. G - 1, G = ceil((S - P) / T) + 1: the last window is flush with the
 *              edge and may overlap its neighbour irregularly; every pixel is covered (T <= P); P = S gives G = 1.
 *   window     w = ky G + kx covers rows p_ky .. p_ky + P - 1 and columns p_kx .. p_kx + P - 1 of the S x S x 3 uint8 BGR input.
 *   fill       fill_bgr[3], or NULL for the image's own mean per channel, (2 sum + S S) / (2 S S) in integer arithmetic over its
 *              S x S input (the mean rounded half up).
 *   pass 0     the forward pass of the n unmasked images: probs / ids are the bits rn_forward_u8_device returns for that batch.
 *              The class c_i is class_ids[i], or ids[i] of pass 0 when class_ids is NULL; it is read on the device.
 *   passes     the n G G (image, window) pairs, flattened as i G G + w, are cut into chunks of max_batch (the last one shorter;
 *              chunks cross image boundaries).  Per chunk: one mask launch into a workspace [max_batch, S, S, 3], the forward pass
 *              of the chunk, one score launch: drop[i, ky, kx] = p0[i, c_i] - p_w[i, c_i], a float32 subtraction.
 *   map        map[i, y, x] = (float32 sum of drop[i, ky, kx] over the windows covering (y, x), ky ascending, then kx ascending)
 *              / float(count of those windows): additions and one division, one thread per pixel.  Negative entries are kept
 *              (rn_cam_overlay_batch_device, which draws any float32 map on the crop window, takes the positive part itself).
 * The workspaces -- the masked chunk, its probabilities and ids, the per-image fills -- belong to the handle (allocated by the
 * first call, sized for max_batch, freed by rn_destroy); everything runs on the handle's stream, so back-to-back calls without a
 * sync are fine.  All three dtypes: the pipeline only feeds the uint8 forward entry.
 *
 * rn_occlusion_plan          host only, no device: G, n_windows = n G G and n_chunks = ceil(n_windows / max_batch) (each pointer
 *                            may be NULL).  RN_E_INVALID for stride > patch, patch > side or any value below 1; RN_E_RANGE for
 *                            n > max_batch or n G G > 2^20.
 * rn_occlusion_masks_device  the masked images of the flattened indices [first, first + count) into d_out [count, S, S, 3]: the
 *                            mask enqueuer of the full call on its own.  count outside [1, max_batch] or a range outside the
 *                            call's n G G: RN_E_RANGE.  Asynchronous.
 * rn_occlusion_u8_device     pass 0, the masked passes and (d_map not NULL) the map: d_drop [n, G, G], d_map [n, S, S],
 *                            d_probs [n, num_classes], d_ids [n].  It only enqueues; class ids, when given, are read back and
 *                            checked first (outside [0, num_classes): RN_E_INVALID).  The plan's refusals are this call's; a
 *                            refused call enqueues nothing and leaves the handle usable.
 * rn_occlusion_u8            the same for host buffers; blocks.
 * rn_occlusion_last_ms       device time of the last call, pass 0 to the map; waits for it. */
RN_API int rn_occlusion_plan(int side, int patch, int stride, int n, int max_batch, int* G, int* n_windows, int* n_chunks);
RN_API int rn_occlusion_masks_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, int patch, int stride, const uint8_t* fill_bgr,
                                     int first, int count, uint8_t* d_out);
RN_API int rn_occlusion_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, const int32_t* d_class_ids, int patch, int stride,
                                  const uint8_t* fill_bgr, float* d_drop, float* d_map, float* d_probs, int64_t* d_ids);
RN_API int rn_occlusion_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, const int32_t* class_ids, int patch, int stride,
                           const uint8_t* fill_bgr, float* drop, float* map, float* probs, int64_t* ids);
RN_API int rn_occlusion_last_ms(rn_handle* h, float* ms);

/* ---- deletion and insertion curves of a heat map ------------------------------------------------
 * Which heat map to believe: take away the pixels a map ranks highest, a fraction at a time, and watch the
 * class probability fall (deletion); start from nothing, put them back in the same order and watch it rise (insertion).  A map that
 * points at the evidence gives a small deletion area and a large insertion area.  For a handle of side S, an image im [S, S, 3]
 * uint8 BGR, a map m [S, S] float32 of any values, a class c and a step count J with 1 <= J <= S S (roomnet_amd/faithfulness.py
 * states the same in NumPy, csrc/rn_faith.hip in its header comment):
 *   order      pixels by map value descending, equal values by raster index y S + x ascending, -0.0 equal to +0.0, NaN behind
 *              everything else and NaNs among themselves by index: np.argsort(-m.ravel(), kind="stable").  rank[p] is the position
 *              of pixel p in that order, a permutation of 0 .. S S - 1.
 *   sort key   0 for NaN; otherwise u = bits(v + 0.0f) and key = u ^ 0xFFFFFFFF when the sign bit of u is set, else
 *              u ^ 0x80000000; sorted by 0xFFFFFFFF - key ascending, stably (a radix sort in which no atomic decides a position:
 *              the same map gives the same ranks on every run).
 *   steps      n_j = (j S S) / J in 64-bit integers for j = 0 .. J: n_0 = 0, n_J = S S.
 *   fill       fill_bgr[3], or NULL for the image's own mean per channel, (2 sum + S S) / (2 S S), exactly as occlusion's.
 *   images     deletion image j: pixels with rank < n_j hold the fill, the rest im.  Insertion image j: pixels with rank >= n_j
 *              hold the fill, the rest im.  J + 1 points per curve, each its own forward pass; the endpoints the two curves share
 *              are not deduplicated (a forward pass need not give an image the same bits at another batch size or slot).
 *   pass 0     the forward pass of the n <= max_batch unmasked images: probs / ids are the bits rn_forward_u8_device returns.
 *              The class c_i is class_ids[i], or ids[i] of pass 0 when class_ids is NULL; it is read on the device.
 *   passes     modes is a bit mask of RN_FAITH_DELETION | RN_FAITH_INSERTION, M the number of set bits, deletion first.  The
 *              n M (J + 1) passes, flattened as f = (i M + mode_slot) (J + 1) + j, are cut into chunks of max_batch (the last one
 *              shorter; chunks cross curve and image boundaries).  Per chunk: one mask launch into the workspace occlusion uses
 *              too, the forward pass of the chunk, one score launch: curve[i, mode_slot, j] = p_f[c_i], a float32 copy.
 *   area       auc[i, mode_slot] = float32((sum over j = 0 .. J - 1, ascending, of float64(c_j) + float64(c_{j+1})) / (2 J)):
 *              a sequential float64 sum without fma.
 * The ranking's workspace (16 bytes per pixel of max_batch images, which also keeps a call's ranks) belongs to the handle: allocated
 * by the first call, freed by rn_destroy.  Everything runs on the handle's stream, so these calls and occlusion calls follow each
 * other without a sync.  All three dtypes: the pipeline only feeds the uint8 forward entry.
 *
 * rn_faith_plan          host only, no device: n_passes = n M (J + 1) and n_chunks = ceil(n_passes / max_batch) (each pointer may
 *                        be NULL).  RN_E_INVALID for steps < 1, steps > side^2, modes outside 1..3 or n, side, max_batch below 1;
 *                        RN_E_RANGE for n > max_batch or n_passes > 2^20.
 * rn_faith_rank_model    host only: the ranks of n maps of npix values each (any npix >= 1) by the kernel's own steps, its waves,
 *                        tiles and lanes run one after another (csrc/rn_faith_rank.h): the CPU statement of the sort.
 * rn_faith_ranks_device  the ranks alone: d_map [n, S, S] float32 -> d_rank [n, S, S] uint32.  Asynchronous.
 * rn_faith_masks_device  the masked images of the flattened passes [first, first + count) into d_out [count, S, S, 3]: the rank and
 *                        mask enqueuers of the full call on their own.  count outside [1, max_batch] or a range outside the call's
 *                        n M (J + 1): RN_E_RANGE.  Asynchronous.
 * rn_faith_u8_device     pass 0, the ranks, the masked passes and the areas: d_curve [n, M, J + 1], d_auc [n, M],
 *                        d_probs [n, num_classes], d_ids [n].  It only enqueues; class ids, when given, are read back and checked
 *                        first (outside [0, num_classes): RN_E_INVALID).  A null buffer is RN_E_INVALID; the plan's refusals are
 *                        this call's; a refused call enqueues nothing and leaves the handle usable.
 * rn_faith_u8            the same for host buffers; blocks.
 * rn_faith_last_ms       device time of the last rn_faith_u8_device / rn_faith_u8 call, pass 0 to the areas, or of the rank launch
 *                        of the last rn_faith_ranks_device, whichever came last; waits for it. */
#define RN_FAITH_DELETION 1
#define RN_FAITH_INSERTION 2
RN_API int rn_faith_plan(int side, int steps, int modes, int n, int max_batch, int* n_passes, int* n_chunks);
RN_API int rn_faith_rank_model(const float* map, int n, int npix, uint32_t* rank);
RN_API int rn_faith_ranks_device(rn_handle* h, const float* d_map, int n, uint32_t* d_rank);
RN_API int rn_faith_masks_device(rn_handle* h, const uint8_t* d_bgr_nhwc, const float* d_map, int n, int steps, int modes,
                                 const uint8_t* fill_bgr, int first, int count, uint8_t* d_out);
RN_API int rn_faith_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, const float* d_map, int n, const int32_t* d_class_ids, int steps,
                              int modes, const uint8_t* fill_bgr, float* d_curve, float* d_auc, float* d_probs, int64_t* d_ids);
RN_API int rn_faith_u8(rn_handle* h, const uint8_t* bgr_nhwc, const float* map, int n, const int32_t* class_ids, int steps, int modes,
                       const uint8_t* fill_bgr, float* curve, float* auc, float* probs, int64_t* ids);
RN_API int rn_faith_last_ms(rn_handle* h, float* ms);

/* ---- fine-tuning stages 8-9 and the dense head on cached features ------------------------------
 * What the reference's RoomNet(optimized_inference=False).load() prepares (network.py:242, restore_excluded_vars: the conv trunk
 * restored, the dense head left at its initial values, to be trained), cut where it is cheap: stages 0-7 stay frozen, and
 * everything behind "s7.bn" depends on s7.bn alone (21 x 21 x 16 at 224, 68 x 68 x 16 at 600).  rn_features_* fill a cache of
 * those features with the handle's fast forward pass; an rn_ft trainer then runs Adam steps on the resident cache with no
 * trunk pass, no host round trip and no inference handle.  Mathematics (forward, loss, TensorFlow's gradient rules, Adam, the
 * learning-rate schedule): the header of csrc/rn_finetune.hip.  In short: every BN is the inference BN with trainable gamma and
 * beta and fixed moving statistics (train.py:40-41), dropout only where rn_ft_set_dropout switches it on; loss = mean CE(softmax(relu6(z)), y) + l2_coeff sum(v^2) / 2 over
 * the TRAINED variables; tf.train.AdamOptimizer in float32 with lr(step) = learn_rate * decay_rate^(step / num_steps).
 *
 * rn_features_shape     side and channels of one feature ([side, side, channels] float32 per image)
 * rn_features_u8        BGR uint8 [n, S, S, 3] on the host -> this call's s7.bn widened to float32 [n, side, side, 16] on the
 *                       host; n <= max_batch; blocks
 * rn_features_u8_device the same on device buffers; only enqueues on the handle's stream
 * Both run a forward pass (on 16-bit handles with the back end as its split launches, as rn_grad_cam_* does, so that s7.bn
 * is written whatever n is); rn_tap afterwards returns that pass's tensors.  RN_E_INVALID on a graph without the last block,
 * RN_E_STATE on RN_FLAG_BATCH_STATS handles, RN_E_RANGE for n outside [1, max_batch]. */
RN_API int rn_features_shape(const rn_handle* h, int* side, int* channels);
RN_API int rn_features_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, float* feat);
RN_API int rn_features_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, float* d_feat);
/* The same for a trainer of a given depth = its number of trained conv stages.  depth 2: exactly rn_features_*.  depth 3: the
 * feature is this call's "s6.bn", the input of the last conv block, widened to float32 [n, side, side, 128] (46 x 46 at 224,
 * 140 x 140 at 600: 1.08 MB per image at 224 against 28 KB at depth 2), byte for byte what rn_tap("s6.bn") returns after the call.
 * Any other depth is RN_E_INVALID; the other error codes are those of rn_features_*. */
RN_API int rn_features_depth_shape(const rn_handle* h, int depth, int* side, int* channels);
RN_API int rn_features_depth_u8(rn_handle* h, int depth, const uint8_t* bgr_nhwc, int n, float* feat);
RN_API int rn_features_depth_u8_device(rn_handle* h, int depth, const uint8_t* d_bgr_nhwc, int n, float* d_feat);

typedef struct rn_ft rn_ft;
typedef struct rn_ft_config {
    float learn_rate;         /* RoomNet(learn_rate=...)                            */
    float decay_rate;         /* 0.068 in the reference (network.py:36)             */
    int32_t num_steps;        /* RoomNet(num_steps=...): the decay's time constant  */
    int32_t start_step;       /* RoomNet(start_step=...): the global step to resume */
    float l2_coeff;           /* RoomNet(l2_regularizer_coeff=...)                  */
    float beta1, beta2, epsilon; /* tf.train.AdamOptimizer: 0.9, 0.999, 1e-8        */
} rn_ft_config;

#define RN_FT_PARAM 0       /* the float32 master copy of a trained variable      */
#define RN_FT_GRAD 1        /* its gradient at the last step, L2 term included    */
#define RN_FT_ADAM_M 2      /* Adam's first-moment slot                           */
#define RN_FT_ADAM_V 3      /* Adam's second-moment slot                          */

/* rn_ft_create takes the model as rn_create does and keeps float32 master copies of the trained variables -- the last two conv
 * stages' kernels and BN gamma / beta (both BNs of the residual stage), every dense layer's kernel, BN gamma / beta or bias: 19
 * variables for the reference graph, in checkpoint order (rn_ft_var_info) -- with zeroed Adam slots, on `device`, with a
 * stream of its own.  It needs no rn_handle and allocates no trunk workspace; max_batch bounds the minibatch of rn_ft_run.
 * Graphs rn_grad_cam_* refuses are refused here with the same reasons (RN_E_INVALID).
 * rn_ft_run     `steps` Adam steps; step s trains on items d_index[s * batch .. (s + 1) * batch) of the resident d_feats
 *               [n_items, side, side, 16] float32 with classes d_labels [n_items] int32 (all device memory, e.g. of
 *               rn_ft_upload); two launches per step enqueued back to back, one synchronisation at the end; losses [steps]
 *               on the host: each step's loss evaluated BEFORE that step's update.  An index outside [0, n_items), a label
 *               (of an indexed item) outside [0, num_classes) or batch outside [1, max_batch] is RN_E_RANGE, checked on the
 *               host before anything is enqueued: the trainer is unchanged.  No floating-point atomics: the same calls give
 *               the same bits, and one call of k steps equals k calls of one step.
 * rn_ft_eval    forward only, from the current master parameters, for any n (chunks of max_batch inside): mean_loss (the
 *               training loss, L2 term included; needs d_labels), probs [n, num_classes], ids [n] on the host; each may be NULL.
 * rn_ft_read    one variable's values of kind `what` to host float32 (cap: elements available).
 * rn_ft_step_count  the global step: start_step + steps run.
 * rn_ft_last_run_ms  device time of the last rn_ft_run's step loop (events on the trainer's stream around its launches).
 * rn_ft_upload / rn_ft_free  device memory for the caller's features, labels and indices: allocate + copy from the host, and
 *               free (rn_ft_destroy frees what is left).  Calls on one trainer must be serialised by the caller. */
RN_API int rn_ft_create(const rn_weights* w, int device, int max_batch, const rn_ft_config* cfg, rn_ft** out);
/* rn_ft_create_depth: depth 2 is rn_ft_create.  depth 3 trains the whole last conv block from cached "s6.bn" features
 * (rn_features_depth_*, depth 3): conv 7's kernel and its BN's gamma and beta come in front of the list (22 variables for the
 * reference graph; the L2 term runs over all of them), rn_ft_run and rn_ft_eval read d_feats as [n_items, S6, S6, 128] float32,
 * and a step is four launches: conv 7 forward and its weight gradient run on the float32 matrix cores, on a grid of (row band,
 * item), with one weight-gradient partial per (item, band) summed in index order (csrc/rn_finetune7.hip).  Every guarantee of
 * rn_ft_run above holds at depth 3.  Any other depth is RN_E_INVALID.  rn_ft_depth: the depth of a trainer. */
RN_API int rn_ft_create_depth(const rn_weights* w, int device, int max_batch, const rn_ft_config* cfg, int depth, rn_ft** out);
RN_API int rn_ft_depth(const rn_ft* ft);
RN_API void rn_ft_destroy(rn_ft* ft);
RN_API int rn_ft_run(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n_items, const int32_t* d_index, int batch,
                     int steps, float* losses);
RN_API int rn_ft_eval(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n, float* mean_loss, float* probs,
                      int64_t* ids);
RN_API int rn_ft_var_count(const rn_ft* ft);
RN_API int rn_ft_var_info(const rn_ft* ft, int var, char* name, size_t name_cap, int64_t* count);
RN_API int rn_ft_read(rn_ft* ft, int what, int var, float* out, size_t cap);
RN_API int64_t rn_ft_step_count(const rn_ft* ft);
RN_API int rn_ft_last_run_ms(rn_ft* ft, float* ms);
RN_API int rn_ft_upload(rn_ft* ft, const void* src, size_t bytes, void** d_ptr);
RN_API int rn_ft_free(rn_ft* ft, void* d_ptr);

/* ---- validation inside a training run ------------------------------------------------------------
 * The other half of the reference's loop (train.py:134-155): every SAVE_FREQ steps the validation set is run and accuracy and the
 * per-class figures are recorded.  rn_ft_run_validated is rn_ft_run with evaluation passes over a second resident set enqueued
 * between steps on the trainer's stream; the run keeps its one synchronisation.
 * Points: with g0 = rn_ft_step_count at the call, one after the step that brings the global step to g, for every g in
 *               (g0, g0 + steps] with g % val_every == 0 (the reference's rule), and one more at g0 + steps if that is none.
 * rn_ft_val_points  the number of points of such a call (host only); their global steps to point_steps[0 .. min(points, cap))
 *               when point_steps is given.  steps < 1 or val_every < 1: RN_E_RANGE.
 * rn_ft_run_validated  losses [steps] as rn_ft_run; val_losses [points]: the training loss of the validation set at each point
 *               (mean cross-entropy + l2_coeff sum(v^2) / 2, what rn_ft_eval reports); val_confusion [points][nc][nc] int32,
 *               row = label, column = predicted class.  d_val_feats [n_val, ...] and d_val_labels [n_val] are device memory as
 *               the training set is; n_val may exceed max_batch (chunks of max_batch inside).  Validation never drops.
 *               The confusion matrix and the loss are reduced on the device (float64 sums in a fixed order, no floating-point
 *               atomics); the device decides whether a point has strictly more correct predictions than the best so far -- the
 *               earliest of equal points stays -- and then copies the master parameters aside.  Losses, parameters, gradients
 *               and Adam slots are byte for byte those of rn_ft_run with the same arguments, and a point with
 *               g % val_every == 0 gives the same bits however the run is split over calls.
 *               Errors, checked on the host before anything is enqueued, trainer unchanged: those of rn_ft_run; a null
 *               argument: RN_E_INVALID; val_every < 1, n_val < 1 or a validation label outside [0, num_classes): RN_E_RANGE;
 *               a failed allocation of the tables or of the second parameter slab: RN_E_NOMEM.
 * rn_ft_best    the best point so far: its global step, its number of correct predictions and the size of its validation set
 *               (each pointer may be NULL).  Trainer state: it lasts across calls.  RN_E_STATE before any point was taken; so
 *               is rn_ft_read(RN_FT_BEST, ...), which otherwise reads the variable as it was at that point.
 * rn_ft_last_run_ms covers the whole loop of the last run, validation included. */
#define RN_FT_BEST 4   /* rn_ft_read: the master parameters as they were at the best validation point */
RN_API int rn_ft_val_points(const rn_ft* ft, int steps, int val_every, int64_t* point_steps, int cap);
RN_API int rn_ft_run_validated(rn_ft* ft, const float* d_feats, const int32_t* d_labels, int64_t n_items,
                               const int32_t* d_index, int batch, int steps, float* losses,
                               const float* d_val_feats, const int32_t* d_val_labels, int64_t n_val, int val_every,
                               float* val_losses, int32_t* val_confusion);
RN_API int rn_ft_best(const rn_ft* ft, int64_t* step, int64_t* correct, int64_t* n_val);

/* ---- dropout while fine-tuning ------------------------------------------------------------------
 * The reference's other regulariser (RoomNet(dropout_enabled=True, dropout_rate=...), network.py:204-206 and :219-221; train.py:37-38
 * carries DROPOUT_RATE = .35): tf.nn.dropout behind every conv block and every dense block.  A trainer applies it at every site
 * at or behind the cached feature; the dropout behind conv blocks 0-2 (and, at depth 2, behind block 3) acts on frozen stages
 * upstream of the cache and cannot be applied to cached features.  No mask is stored: every mask bit is recomputed where it is
 * needed, forward and adjoint, from a counter-based generator, so that with dropout on the same calls still give the same bits, one
 * call of k steps equals k calls of one step, and a run resumed with start_step reproduces the same masks.
 *
 * Generator: Philox4x32-10 as published (multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85, ten rounds).
 * For element e of site `site`, minibatch slot b (the position in the minibatch, not the item: an item that occurs twice in a step
 * gets two masks) and global step t (what rn_ft_step_count returned before the step):
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (e >> 2, b, (uint32) t, site | ((uint32)(t >> 32) << 8))
 *   word    = out[e & 3];   k = word >> 8, a 24-bit value
 * The element is kept iff k >= thr, thr = ceil((double) rate * 2^24): exactly k 2^-24 >= rate, TensorFlow's random_uniform >= rate.
 * A kept value becomes x * scale, one float32 product with scale = 1.0f / (1.0f - rate) (one float32 division); a dropped value
 * becomes +0.0f; the adjoint is g * scale where kept and 0 where dropped.
 *
 *   site   tensor                                                                      element index e
 *   0      "s6.bn", the output of conv block 3 and the input of stage 7; depth 3 only  (y * S6 + x) * 128 + c within the item
 *   1      the last conv block's output, the flattened tensor dense 0 reads            (y * S9 + x) * 16 + c
 *   2 + d  the output of dense block d: behind its BN for d < n_dense - 1; the last     unit j
 *          block's logits relu6(z) have no BN and are dropped too, as the reference drops them
 * With dropout on, a depth-3 step is five launches: site 0 is a pre-pass that writes the minibatch's dropped s6.bn to a workspace
 * [max_batch, S6, S6, 128] float32, allocated when dropout is first switched on at depth 3.
 *
 * rn_ft_set_dropout   rate in [0, 1): else (NaN included) RN_E_RANGE, trainer unchanged.  rate 0: off -- the trainer runs launch for
 *                     launch what it runs without this call.  Takes effect from the next rn_ft_run; rn_ft_eval never drops (the
 *                     reference's infer feeds rate 0).  A failed workspace allocation is RN_E_NOMEM, trainer unchanged.
 * rn_ft_dropout       the current rate and seed (0 and 0 on a new trainer); either pointer may be NULL.
 * rn_ft_dropout_mask  the mask a step would use, at the trainer's current rate and seed, computed on the device: keep[0 .. count)
 *                     on the host, 0 or 1, of elements [0, count) of `site` in `slot` at global step `step`.
 *                     Errors: site 0 on a depth-2 trainer, or a site the graph lacks: RN_E_INVALID.
 *                             count < 1 or beyond the site's size, slot outside [0, max_batch), or step < 0: RN_E_RANGE.
 *                     rate 0: all ones. */
RN_API int rn_ft_set_dropout(rn_ft* ft, float rate, uint64_t seed);
RN_API int rn_ft_dropout(const rn_ft* ft, float* rate, uint64_t* seed);
RN_API int rn_ft_dropout_mask(rn_ft* ft, int site, int64_t step, int slot, int64_t count, uint8_t* keep);

/* ---- fine-tuning on fresh random views ----------------------------------------------------------
 * The reference trains on a feeder built with random_crop=True, preprocess=True (train.py:117-118): every sample of every step is a
 * fresh random square window slid along the photograph's long axis (generator.py:52-67), resized to the network's side, mirrored
 * left-right with probability 1/2 and upside-down with probability 1/2 (:85-92).  A cached feature cannot be augmented afterwards
 * (stages 0-7 are VALID convolutions and pools: their geometry does not commute with a flip or a shifted window), so the views are
 * made in front of the trunk, every step, from photographs that stay resident on the device.
 *
 * The draw, a pure function (csrc/rn_views.h).  For global step t (what rn_ft_step_count returns before the step), minibatch slot b,
 * a 64-bit seed and a photograph of height x width, with Philox4x32-10 exactly as the dropout section above has it:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (0, b, (uint32) t, RN_VIEW_SITE | ((uint32)(t >> 32) << 8));  site 254 is one no dropout site can take, so the view
 *             draws and the dropout masks of one seed never share a counter
 *   side = min(height, width),  range = max(height, width) - side
 *   RN_VIEW_CROP  offset = (uint64) out[0] * range >> 32: a value in [0, range), as np.random.randint(range) draws one (never
 *                 offset == range; range == 0: offset 0, the whole image).  Its bias against a true uniform is below range / 2^32.
 *                 Without the flag: the centre window, exactly rn_center_crop_window (the reference's center_crop).
 *                 height < width: the window is columns [offset, offset + side); otherwise rows [offset, offset + side).
 *   RN_VIEW_FLIP  fliplr = out[1] >> 31, flipud = out[2] >> 31.  Without the flag: neither.
 * The view is flipud(fliplr(resize(window, (S, S)))), the flips behind the resize as in preprocess_set: view[y][x] =
 * R[flipud ? S-1-y : y][fliplr ? S-1-x : x] with R the integer-exact cv2.resize(INTER_LINEAR) of rn_crop_resize_*, its copy mode
 * and its 2x2-box mode included.  NumPy's own random stream is not reproduced; the distribution and the sampling rules are.
 * No draw reads outside the photograph: offset <= range in both modes, so offset + side <= max(height, width).
 *
 * rn_view_draw   the draw on the host (no device): x0, y0 and side of the window, and the two flips.  A null `out`, an empty image or
 *                unknown flag bits: RN_E_INVALID; step < 0 or slot < 0: RN_E_RANGE.
 * rn_views_create  the training set as a device table that lives for the whole run: per photograph (whole, decoded, tightly packed
 *                BGR, resident on the handle's device -- the caller keeps the pixels alive) what does not change from step to step:
 *                base pointer, row stride, side, range, axis, and the two double-precision scales and the mode of the resize, formed
 *                on the host as rn_crop_resize_* forms them (they depend on the side alone, not on the offset).  A null argument,
 *                n_items < 1 or an empty photograph: RN_E_INVALID; a failed allocation: RN_E_NOMEM.
 * rn_views_destroy  frees the table (not the photographs).
 * rn_views_batch_device  ONE launch on the handle's stream makes the n views of a minibatch into d_dst [n, S, S, 3] uint8: slot b
 *                reads item d_index[base + b] (device int32), draws its own window and flips on the device and stores every pixel
 *                at its flipped address.  No per-step table, no per-step upload.  Only enqueues.  Checked on the host before
 *                anything is enqueued: a null argument, unknown flag bits, or a table made on another device or for another side:
 *                RN_E_INVALID; n outside [1, max_batch], step < 0 or base < 0: RN_E_RANGE.  The index lives on the device and is not
 *                read back here: a slot whose index lies outside [0, n_items) is left unwritten. */
#define RN_VIEW_CROP 1u
#define RN_VIEW_FLIP 2u
#define RN_VIEW_SITE 254u
typedef struct rn_view {
    int32_t x0, y0, side, fliplr, flipud;
} rn_view;
typedef struct rn_view_source {
    const uint8_t* d_bgr;     /* [height, width, 3] uint8 on the handle's device */
    int32_t height, width;
} rn_view_source;
typedef struct rn_views rn_views;
RN_API int rn_view_draw(uint64_t seed, int64_t step, int slot, int height, int width, unsigned flags, rn_view* out);
RN_API int rn_views_create(rn_handle* h, const rn_view_source* srcs, int64_t n_items, rn_views** out);
RN_API void rn_views_destroy(rn_views* v);
RN_API int rn_views_batch_device(rn_handle* h, const rn_views* v, const int32_t* d_index, int64_t base, int n, uint64_t seed,
                                 int64_t step, unsigned flags, uint8_t* d_dst);
/* rn_ft_run_views  rn_ft_run / rn_ft_run_validated (the six validation arguments all NULL / 0: no validation) with one difference:
 *                step s does not read resident features.  On the handle's stream it makes the views of slots
 *                [s * batch, (s + 1) * batch) at the trainer's global step into the handle's input batch (rn_views_batch_device) and
 *                runs the trunk's feature pass of the trainer's depth (rn_features_depth_u8_device) into a feature slot
 *                [batch, side, side, C] float32 the trainer owns (two slots taken in turn, allocated by the first such run, so
 *                that the trunk pass of step s + 1 overlaps the trainer's step s); behind an event the trainer's stream runs the
 *                step's launches on that slot, with labels gathered once per call in slot order, d_labels[d_index[s * batch + b]];
 *                an event back keeps the handle from overwriting a slot the trainer still reads.  The handle's stream and its
 *                input batch are in use until the call returns.  The step's kernels are those of rn_ft_run, the
 *                loop, the validation schedule and the one synchronisation at the end are the same code.  Dropout is unchanged
 *                (keyed by slot and step already); the validation set stays cached centre-crop features, as the reference
 *                validates on random_crop=False, preprocess=False.  d_labels [n_items] and d_index [steps, batch] are device
 *                memory; `flags` are RN_VIEW_CROP | RN_VIEW_FLIP.
 *                The handle's weights being the trainer's frozen trunk (stages 0-7 of the model the trainer was created from) is
 *                the caller's contract: neither object knows the other's weights.
 *                Guarantees: the same call gives the same bits; one call of k steps equals k calls of one step (the global step
 *                drives the draws, so a resumed run continues the same sequence); losses, parameters, gradients and Adam slots are
 *                byte for byte those of the manual loop rn_views_batch_device, rn_features_depth_u8_device, one rn_ft_run step.
 *                Errors, on the host before anything is enqueued, trainer unchanged: everything rn_ft_run (rn_ft_run_validated)
 *                refuses; a handle on another device than the trainer's, a graph whose feature shape differs from the trainer's,
 *                views of another device or side, unknown flag bits, or only some of the validation arguments: RN_E_INVALID;
 *                batch > the handle's max_batch: RN_E_RANGE; an RN_FLAG_BATCH_STATS handle: RN_E_STATE; a failed allocation of
 *                the feature slot: RN_E_NOMEM. */
RN_API int rn_ft_run_views(rn_ft* ft, rn_handle* h, const rn_views* v, const int32_t* d_labels, int64_t n_items, const int32_t* d_index,
                           int batch, int steps, uint64_t view_seed, unsigned flags, float* losses, const float* d_val_feats,
                           const int32_t* d_val_labels, int64_t n_val, int val_every, float* val_losses, int32_t* val_confusion);

/* ---- introspection -----------------------------------------------------------
 * rn_tap copies graph node `node_id` of the last forward call to host float32
 * (layout [n, h, w, c]); needs RN_FLAG_TAPS for conv/pool/add nodes; the
 * tensors a launch WRITES are always available: every stage's output node
 * ("sK.bn", for the residual stages "sK.bn2") unless the stage is fused into
 * its successor's launch.  The first BN output "sK.bn" of a residual stage
 * exists only where that stage runs one launch per graph node (float32 handles
 * with RN_FLAG_TAPS, and stages the matrix-core float32 kernels do not cover);
 * 16-bit handles never materialise it.  Asking for a node that was not written
 * returns RN_E_STATE.  This is the per-layer
 * debug read-out the reference gets from self.layers (network.py:30, :207).
 * After a grad-CAM call (rn_grad_cam_*) rn_tap returns THAT call's forward tensors: on 16-bit
 * handles it ran the back end as its split launches, so s6.bn and s7.bn are readable even
 * at a batch where rn_forward_* fuses them away; the next rn_forward_* chooses as before. */
/* What rn_create folded on this handle (zero / -1 where nothing is): info[0] = channels of the first 32 -> 32 stage's output
 * (16-bit handles: the fused pair's on-chip tensor) that are provably constant and therefore not contracted by the next stage
 * (24, 16 or 0; 16-bit handles since round 6 prove it on the tensor's 16-BIT STORE -- the two ends of the pooled sum's range store
 * the same number -- which includes every channel whose fma returns its addend in float32, the criterion of the float32
 * matrix-core handles: 16 or 0 there), info[1] = how many of its 32 channels were proven so,
 * info[2] = index of the 64 -> 64 residual stage whose frozen first-BN channels are folded (or -1), info[3] = 16-cout
 * quarters of that stage whose convolution still runs (4 = all).  RN_FLAG_COMPUTE_FROZEN and RN_FLAG_TAPS handles report
 * nothing folded. */
RN_API int rn_frozen_info(const rn_handle* h, int info[4]);
/* Constant channels nobody computes (16-bit handles; zero / -1 where nothing is): info[0] = index of the conv stage whose last 16
 * output channels are CONSTANTS in this handle's 16-bit store -- rn_create proves per channel that the store of fma(H, sc, sh) is
 * one 16-bit number for every pooled sum H the stage can produce -- and are therefore not convolved but written once, at
 * rn_create (or -1), info[1] = how many channels of that stage were proven so, info[2] = channels folded (16 or 0), info[3] =
 * input channels the stage behind it still contracts (48; its own last 16 output channels are constants as well).  The shipped
 * checkpoint: stage 4 (network.py:228, first step), 26 channels in bf16, 23 in fp16.  RN_FLAG_COMPUTE_FROZEN handles and
 * float32 handles report nothing. */
RN_API int rn_const_info(const rn_handle* h, int info[4]);
RN_API int rn_node_count(const rn_handle* h);
RN_API int rn_node_info_get(const rn_handle* h, int node_id, rn_node_info* out);
RN_API int rn_tap(rn_handle* h, int node_id, float* out, size_t cap_elems, size_t* n_elems);

/* ---- batch moments of the last forward call (RN_FLAG_BATCH_STATS handles) ------------------
 * What the reference's update ops read (network.py:64-67: tf.GraphKeys.UPDATE_OPS of every
 * tf.layers.batch_normalization(training=True)).  The BNs are numbered in the reference's variable order
 * batch_normalization, _1, ... _15: per conv stage its BN, then the BN behind the residual add where there is
 * one, then the three dense BNs.
 *   rn_bn_count        how many there are (16), or a negative code
 *   rn_bn_info         the BN's OUTPUT node ("s3.bn2", "d0.bn", ...) and its channel count in out->c
 *   rn_bn_batch_stats  mean[c] = sum x / count and var_biased[c] = sum (x - mean)^2 / count over the count =
 *                      n * h * w values per channel of the BN's input (dense BNs: n), float32; any of the three
 *                      output pointers may be NULL.  Computed as float32 Welford partials merged in float64
 *                      (rn_bnstats.hip): deterministic, and close to a float64 two-pass result.  count is
 *                      read back from the device: the number of values the merge of that call really saw per
 *                      channel (dense BNs: the n their kernel ran over), not a product formed on the host.
 *                      RN_E_STATE "merged counts disagree" -- the one message for all of these -- if the channels
 *                      of a BN saw different counts, or the value is not a whole number, or it is below 1.  The update
 *                      of the moving statistics itself is host arithmetic on 32 short vectors
 *                      (roomnet_amd/bnstats.py: moving_update, variance_for_update).
 * RN_E_STATE on a handle without the flag or before the first forward call, RN_E_RANGE for a bad index. */
RN_API int rn_bn_count(const rn_handle* h);
RN_API int rn_bn_info(const rn_handle* h, int i, rn_node_info* out);
RN_API int rn_bn_batch_stats(rn_handle* h, int i, float* mean, float* var_biased, int64_t* count);

/* Enable/disable per-stage event timing (adds event records to every forward). */
RN_API int rn_set_profiling(rn_handle* h, int enable);
RN_API int rn_timing(rn_handle* h, rn_stage_ms* out);

/* Name of the kernel that dominates the forward pass of this handle (for
 * matching rocprofv3 rows) and the stage index it belongs to. */
RN_API int rn_dominant_stage(const rn_handle* h);
/* Launch grouping of the conv stages: the index of the stage under which the launch that
 * computes `stage` reports its time in rn_stage_ms (== stage when the stage has a launch of
 * its own; the last stage of the group when stages are fused across their boundary --
 * the depth loop of conv_block, reference network.py:183-203, is then one kernel).
 * Returns a negative code for a bad argument. */
RN_API int rn_stage_launch(const rn_handle* h, int stage);

/* ---- several GPUs from one process ------------------------------------------------
 * The reference is one tf.Session on one device (network.py:89).  A group is one rn_handle
 * per device; a batch is split contiguously (device d gets images [d*n/N, (d+1)*n/N), the
 * first n % N devices one more) and the ONLY exchange on the data path is one RCCL
 * all-gather of every device's packed results over xGMI: per device `slot_bytes` =
 * max_batch_per_device * (num_classes * 4 + 8) bytes = probs [cap, C] float32 followed by
 * ids [cap] int64 (32 bytes per image).  librccl is loaded on the first rn_group_create
 * (environment ROOMNET_RCCL_LIB, read at that call only: another file to dlopen instead);
 * without it rn_group_create returns RN_E_STATE and says which dlopen failed.
 * One host thread drives all devices; calls on one group must be serialised by the caller;
 * every rn_group_* call leaves the caller's current HIP device as it found it.
 * SCALING: rn_group_forward_u8_device is the entry that scales -- the shards are already in
 * each device's HBM (as in BASELINE's measurement contract) and nothing but 32 B per image
 * crosses a link.  rn_group_forward_u8 takes one host buffer: it uploads the shards through
 * one persistent host thread per device (started by rn_group_create, parked between calls:
 * a copy out of pageable memory blocks the thread that issues it; out of an rn_host_alloc
 * buffer it does not) and is bound by the host's memory and PCIe bandwidth (38.5 MB per
 * device and call at 256 x 224 x 224), not by the GPUs.
 * VALIDATION: groups of more than one device have not run on hardware yet (the
 * development pool has one MI355X per box); the one-device group is tested on the GPU. */
typedef struct rn_group rn_group;
/* devices == NULL: devices 0 .. ndev-1.  Weights are replicated (0.7 MB). */
RN_API int rn_group_create(const rn_weights* w, int ndev, const int* devices, int dtype, int max_batch_per_device,
                           unsigned flags, rn_group** out);
RN_API void rn_group_destroy(rn_group* g);
RN_API int rn_group_size(const rn_group* g);
RN_API rn_handle* rn_group_handle(rn_group* g, int index);     /* the per-device handle (profiling, taps) */
/* RoomNet.infer(im_batch) (reference network.py:128-135) over all devices: host BGR uint8
 * [n,S,S,3] in, (softmax [n,C], argmax [n]) on the host out; n <= ndev * max_batch_per_device.
 * Blocks until the results are in probs/ids. */
RN_API int rn_group_forward_u8(rn_group* g, const uint8_t* bgr_nhwc, int n, float* probs, int64_t* ids);
/* Device-resident form: d_shards[d] = device d's images already in its HBM, counts[d] of them.
 * Asynchronous: enqueues the forward passes and the all-gather on the devices' streams;
 * afterwards rn_group_result_buffer(g, d, ...) on ANY device holds all devices' packed results
 * ([ndev][slot_bytes], device d's slot at d * slot_bytes).  rn_group_sync waits for all of it.
 * A device with counts[d] == 0 runs nothing but still takes part in the all-gather: its slot
 * keeps what its last non-empty call left there (zeros before the first); only the first
 * counts[d] entries of a slot belong to this call. */
RN_API int rn_group_forward_u8_device(rn_group* g, const uint8_t* const* d_shards, const int* counts);
RN_API int rn_group_result_buffer(rn_group* g, int index, void** d_gathered, size_t* slot_bytes);
RN_API int rn_group_sync(rn_group* g);
/* The shard / slot plan rn_group_forward_u8 applies, as a pure function (no group, no device -- testable on any host): device d
 * of ndev takes the images [offsets[d], offsets[d] + counts[d]) of an n-image batch -- contiguous shards, the first n % ndev
 * devices one image more (network.py:128-135 split over devices; the same rule as roomnet_amd/parallel.py: shard_bounds) --
 * and *slot_bytes (may be null) = the size of one device's slot in the gathered buffer: probs [max_batch_per_device, C] float32
 * followed by ids [max_batch_per_device] int64.  n > ndev * max_batch_per_device is RN_E_RANGE. */
RN_API int rn_group_plan(int n, int ndev, int max_batch_per_device, int num_classes, int* counts, int* offsets, size_t* slot_bytes);

/* ---- launch geometry of the conv stages, as a pure function (no handle, no device -- testable on any host) -------------
 * A stage's launch cuts every image into bands of output rows; a workgroup is image x column block x band.  Bands change
 * no result bit, only how the launch fills the chip.  rn_band_plan returns what rn_forward_* chooses for a launch of
 * `family` with n images on a chip of n_cu compute units: *rows_per_band rows in each of *n_bands bands.
 *   out_side     the stage's output side (the second stage's for RN_BANDS_PAIR)
 *   n_colblocks  workgroups per image and band (column blocks; x cout-tile groups for RN_BANDS_GENERIC / RN_BANDS_F32M)
 *   wgs_per_cu   workgroups resident on one CU (RN_BANDS_RW: 1 or 4; RN_BANDS_CONV16P: 2 for the 3-wave form, 1 for the
 *                5-wave form; ignored by the other families)
 *   pool_k, pool_s  the stage's pooling (pool_k == 0: none; RN_BANDS_ROWREG, RN_BANDS_RW, RN_BANDS_F32M)
 * n_cu is ignored by RN_BANDS_STAGE0 and RN_BANDS_GENERIC.  A bad argument or an unknown family is RN_E_INVALID. */
#define RN_BANDS_STAGE0 0   /* stage 0 in a launch of its own */
#define RN_BANDS_GENERIC 1  /* the generic 16-bit stage kernel */
#define RN_BANDS_PAIR 2     /* the cross-stage fused pair */
#define RN_BANDS_CONV16 3   /* the un-pooled 64 -> 128 stage on 16x16x32 tiles */
#define RN_BANDS_CONV16P 4  /* the pooled 128 -> 16 stage on 16x16x32 tiles */
#define RN_BANDS_ROWREG 5   /* the row-register kernels (32 -> 64, 64 -> 64 residual, 64 -> 128) */
#define RN_BANDS_RW 6       /* the register-weights kernels */
#define RN_BANDS_F32M 7     /* float32 stages on the matrix cores */
RN_API int rn_band_plan(int family, int n, int n_cu, int out_side, int n_colblocks, int wgs_per_cu, int pool_k, int pool_s,
                        int* rows_per_band, int* n_bands);

/* ---- plan of one conv stage on the float32 matrix-core path, as a pure function (no handle, no device) ---------------------
 * What rn_create decides for a stage of an RN_DTYPE_F32 handle without RN_FLAG_TAPS from its shape alone: the kernel, the row
 * of its variant table and the launch geometry (the dynamic LDS included, which no kernel trace shows).
 *   live_cin      input channels the stage contracts (cin, or fewer where its producer's BN freezes the last ones; where no
 *                 variant contracts that count the plan contracts all of them and says so in live_cin)
 *   frozen_couts  couts not convolved: of a residual stage, whole 32-cout tiles left to the residual-only launch (n_ctg
 *                 shrinks); otherwise constants written beside 16 live couts by the 16-cout kernel (without such a variant the
 *                 plan convolves every cout and says so in frozen_couts)
 * pinned by tests/test_f32m_plan.py.  A bad argument is RN_E_INVALID. */
#define RN_F32M_OFF 0       /* not covered: the per-node kernels run the stage */
#define RN_F32M_WIDE 1      /* 32-cout tiles, v_mfma_f32_32x32x2_f32 */
#define RN_F32M_16 2        /* 16 couts, v_mfma_f32_16x16x4_f32 */
typedef struct rn_f32m_stage_plan {
    int kind;               /* RN_F32M_* */
    int variant;            /* row of the kind's variant table (-1: none) */
    int live_cin, frozen_couts;
    int npt;                /* pixel tiles per workgroup */
    int ringcols;           /* columns of a ring row in LDS */
    int lds;                /* dynamic LDS bytes of the launch */
    int n_colblocks, n_ctg; /* column blocks; workgroups the cout tiles are split over */
    int threads;            /* threads per workgroup */
} rn_f32m_stage_plan;
RN_API int rn_f32m_plan(int cin, int cout, int pool_k, int pool_s, int residual, int in_side, int out_side, int live_cin,
                        int frozen_couts, rn_f32m_stage_plan* plan);

/* ---- simple device memory helpers (so a host language without a HIP binding
 * can keep batches resident in HBM) ---------------------------------------- */
RN_API int rn_device_malloc(rn_handle* h, size_t bytes, void** d_ptr);
RN_API int rn_device_free(rn_handle* h, void* d_ptr);
RN_API int rn_memcpy_h2d(rn_handle* h, void* d_dst, const void* src, size_t bytes);
RN_API int rn_memcpy_d2h(rn_handle* h, void* dst, const void* d_src, size_t bytes);

/* ---- pinned host memory ------------------------------------------------------------
 * The reference hands TensorFlow pageable NumPy arrays (network.py:133); a copy out of pageable
 * memory blocks the calling thread while the runtime stages it.  A batch buffer from
 * rn_host_alloc (page-locked, usable with every device of the process) makes the upload of
 * rn_submit_u8 / rn_forward_u8 / rn_group_forward_u8 a true asynchronous DMA: the two-slot
 * pipeline then hides it completely behind the previous batch's kernels.  Free with
 * rn_host_free (NULL is a no-op).  No handle is needed: call before or after rn_create. */
RN_API int rn_host_alloc(size_t bytes, void** ptr);
RN_API int rn_host_free(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* ROOMNET_HIP_H */
