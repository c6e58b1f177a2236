/* ocr_amd.h - C ABI of the MI355X-native OCR inference hot path.
 *
 * This is the FFI surface a maintainer of lazareviczoran/ocr-rs binds instead of
 * tch/libtorch for the two inference stages (INTEGRATION.md shows the Rust side).
 * Plain pointers and sizes only; no torch types; nothing unwinds across the
 * boundary (the reference builds with panic = "abort", Cargo.toml:12-15): every
 * entry point returns an int status (0 = OK) and records a thread-local message
 * readable through ocr_last_error().
 *
 * Tensors are dense row-major f32, NCHW as tch hands them to ATen.  Handles are
 * bound to one GPU and one HIP stream, are not thread-safe, and calls are
 * synchronous unless the name ends in _async (mirrors the reference's blocking,
 * single-threaded calls).  DIFFERENT handles are independent: the
 * library keeps no shared mutable state, so threads that each own their handles
 * (a serving process, or one thread per GPU) may call concurrently and get the
 * bits they would get alone (tests/test_gpu_threads.py: detection through
 * classify, and the reading calls, both CTC decoders and ocr_preprocess_batch).
 * What the library sets per device function rather than per handle (the beam
 * kernel's dynamic-LDS attribute) is set to one value whatever the call.
 */
#ifndef OCR_AMD_H
#define OCR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCR_OK 0
#define OCR_ERR_INVALID 1   /* bad argument / shape                      */
#define OCR_ERR_WEIGHTS 2   /* weight blob malformed or tensor missing   */
#define OCR_ERR_HIP 3       /* HIP runtime error (message has the call)  */
#define OCR_ERR_NOGPU 4     /* no usable gfx950 device: there is NO CPU fallback */
#define OCR_ERR_INTERNAL 5
#define OCR_ERR_DEGENERATE 6 /* expand_polygon gave None: the reference unwraps it and aborts (metrics.rs:103) */

/* memory kind of the data pointers handed to a call */
#define OCR_MEM_HOST 0
#define OCR_MEM_DEVICE 1

typedef struct ocr_det ocr_det_t;     /* detector: resnet18() graph + its weights  */
typedef struct ocr_rec ocr_rec_t;     /* recogniser: char_recognition::Net         */

/* Thread-local description of the last failure on this thread ("" if none). */
const char* ocr_last_error(void);
/* Library / ABI version, "ocr_amd <major>.<minor> gfx950". */
const char* ocr_version(void);
/* Number of visible HIP devices (never throws; 0 when there is no GPU). */
int ocr_device_count(void);

/* VarStore file -> OCRW blob, host only (no GPU needed): kind 0 / 1 = names as stored (detector), 2 = recogniser
 * (tch's name__N leafs mapped by shape).  *blob is malloc'ed by the library; release it with ocr_blob_free. */
int ocr_varstore_to_blob(const char* path, int kind, void** blob, size_t* blob_bytes);
void ocr_blob_free(void* blob);

/* ---------------------------------------------------------------------------
 * Detector.  Replaces, for inference:
 *   let net = resnet18(&vs.root()); vs.load(file)      text_detection/mod.rs:35-44
 *   net.forward_t(&x.view((n,1,h,w)), false)           text_detection/mod.rs:52-54, :196-197
 * graph definition: text_detection/model.rs:65-156.
 * `weights` is an OCRW v1 blob (ocr-rs_amd/weights.py documents the layout) whose
 * tensor names are the VarStore names of model.rs:68-105; it is copied.
 * ------------------------------------------------------------------------- */
int ocr_det_create(const void* weights, size_t weights_bytes, int device, ocr_det_t** out);
/* The same with explicit engine options, "key=value;key=value" (NULL or "" = the defaults).  The library never reads
 * the environment: which schedule runs is the caller's choice.  Every combination computes the same graph and is
 * held to the same parity bars (tests/test_gpu_parity.py::test_engine_modes_agree); they exist for A/B measurements.
 *   winograd_fused=0|1   (1)    fused Winograd F(4x4,3x3) kernel (winograd43_fused.hip) for the 3x3 s1 convs with 64 or 128 input
 *                               channels (trunk, FPN lateral terms); 0 = direct / unfused-Winograd convs
 *   out4_fused=0|1       (0)    1 = out4 (256 -> 64 at H/16) on the fused kernel too and out5 as a direct conv; 0 = both through the
 *                               unfused F(4x4,3x3) path of layer3 / layer4 (faster at these grid sizes)
 *   winograd=<cin>|0     (256)  unfused Winograd for 3x3 s1 trunk convs with Cin >= cin that have no fused form; 0 = off
 *   winograd43=<cin>|0   (256)  of those, the layers with Cin >= cin use F(4x4,3x3) (36 products per 16 outputs) instead of
 *                               F(2x2,3x3) (16 per 4); 0 = F(2x2) everywhere
 *   fpn_unfused=0|1      (0)    1 = layer-by-layer FPN (laterals, top-down sums, out_k, gathered bin_conv1) as model.rs writes it
 *   bin_pyr=0|1          (1)    bin_conv1 over the upsampled concat as one phase-conv launch (0: four launches)
 *   pyr_grouped=0|1      (1)    bin_conv1's phase launch over p5, p4, p3 (split-bf16 and bf16 kernels): the output phases y mod 8 in {1,2}, {3,4},
 *                               {5,6} (same along x) read the same source rows - such a block of phases is one 128-column tile that fetches
 *                               and splits the operand once; the four corner phases are a second, small launch.  0 = one 64-column tile per
 *                               phase.  Bit-identical
 *   phase_windows=0|1    (1)    the FPN's up-2 phase convs (split-bf16 and bf16 kernels): phase 1 of cell i and phase 0 of cell i + 1 read the same two low-res
 *                               rows, so the GEMM's rows are the (H + 1) x (W + 1) 2 x 2 windows and the four phases that read a window are four
 *                               column groups of one operand tile (outputs outside the map are dropped).  0 = one 64-column tile per phase.  Bit-identical
 *   pyr_p2_direct=0|1    (1)    bf16 precision only: p2's 3x3 term of bin_conv1 as the patch-staged 64 -> 64 conv on top of the phase
 *                               launch over p5, p4, p3 (0: all four sources in the phase launch)
 *   tail_unfused=0|1     (0)    1 = probability head as two launches
 *   overlap=0|1|2|3      (3)    second stream: 1 small independent launches; 2 the FPN branch as it stands; 3 the FPN's fused-Winograd
 *                               launches (lateral terms of p2 / p3) and bin_conv1's p2 term - f32 matrix instructions - beside layer2 / layer3 / layer4 /
 *                               the small FPN convs - bf16 matrix instructions and HBM-bound transforms: 2 % of the step in both precisions (default kernels;
 *                               otherwise, and under ocr_det_forward_profile, one stream).  Sums re-associate by one rounding.  Any other value is OCR_ERR_INVALID
 *   front_split=auto|0|<k> (auto) where overlap=3 is in effect (so never under ocr_det_forward_profile) and the batch has at least two frames: stem, layer1
 *                               and layer2 run as two frame groups, frames [0, k) on the main stream and [k, N) on the second stream, joined before layer3.
 *                               Every launch of the front is independent per frame; the group that is a launch behind fills the ragged last round of the
 *                               other's persistent grids.  Same workspace (a group is a pointer offset), same kernels, the same bits.  0 = off; k >= N = no
 *                               split; auto = two halves, in the f32 precision, when a half fills the resident slots of layer1's persistent grids once (5.12 frames of
 *                               640 x 640 on 256 CUs) and no pipelined batch is pending on the handle.  A negative or unparsable value is OCR_ERR_INVALID
 *   top_side=auto|0|<mask> (auto) where overlap=3 is in effect, in the f32 precision with out4 / out5 as three-launch F(4x4) Winograd convs: launches behind
 *                               layer3 that do not depend on their main-stream predecessors run on the second stream.  A mask of moves - 1: layer4's shortcut
 *                               conv (beside layer4's first convs), 2: in4 as a plain conv beside layer4, the top-down add up2(in5) + in4 made where out4's
 *                               input transform loads its patch (the one f32 add the conv's epilogue made, on the same operands), 4: out5's three launches
 *                               beside out4's, on a Winograd scratch of their own.  Same kernels otherwise, the same bits.  0 = off; auto = all three, and
 *                               none while a pipelined batch is pending on the handle.  A value outside 0..7 is OCR_ERR_INVALID
 *   bf16_block_fuse=0|1  (1)    bf16 precision: each BasicBlock of layer1 (conv3x3 + BN + ReLU, conv3x3 + BN, + x, ReLU: model.rs:40-55) as ONE launch, the
 *                               activation between its two convs held in LDS (basic_block_bf16_c64.hip): half the HBM traffic of the two launches, 1.25 x
 *                               their matrix work, 5-10 % less time; 0 = two conv3x3_bf16_c64 launches.  The same bits either way
 *   w43_cus=<n>          (0)    tuning: size of the fused Winograd kernel's persistent grid in CUs (two workgroups each); 0 = every CU of the device.
 *   w43_side_cus=<n>     (0)    the same for the fused Winograd launches that overlap=3 puts on the side stream; 0 = every CU.  Both 0..4096; any
 *                               grid size gives the same bits (tests/test_gpu_conv_kernel.py)
 *   post_threads=<n>     (0)    host threads of the post-processing stages (contours, unclip), the calling thread included;
 *                               0 = min(16, CPU share of the process: cgroup quota or online cores).  One process per GPU on a
 *                               shared host should pass its share (cores / ranks)
 *   device_unclip=0|1|2  (1)    behind the box scores, per candidate polygon on the GPU (unclip.hip; 1: where a call has more than 40 candidates per pool
 *                               thread - the kernel is lane-serial, 0.2 ms however few it gets -, 2: always): score threshold, miter offset, the union where
 *                               the ring is simple or only crosses itself at its concave vertices, min-size test, round(p / adj).  What it does
 *                               not settle (other self-intersections, squared-off corners, a short side within 3 px of min_size) the host
 *                               finishes inside the same call; results are bit for bit the host path's (0)
 *   device_contours=auto|0|1|2 (auto)  the contour tracing of ocr_det_postprocess / the pipelined calls on the GPU (contours.hip; one bit plane of the map
 *                               in LDS: up to 1024 x 1024, the reference's 800 x 800 included - larger maps, and images the kernel gives up on, take the host tracer inside the same call).
 *                               1: plausible border starts walked in parallel, the raster scan only replays the label tests, a row at a time as
 *                               word-wide bit arithmetic (0.35-0.5 ms per batch; the pipelined calls request it when they queue a batch); 2: one wave per image.  Identical
 *                               contours either way.  auto: 1 where the host pool (post_threads) has at most four threads, else 0: by
 *                               measurement
 *   head_cus_yield=0..4  (2)    pipelined calls, while the polygon chain of the previous batch runs beside this forward's first launches: layer1's persistent
 *                               grids (their blocks are dealt statically: a workgroup that shares its CU with the tracer's waves holds the launch up) are
 *                               1: sized for the CUs the tracer leaves (the form of the whole-CU tracer), 2..4: launched with that many workgroups per
 *                               resident slot, so that the hardware hands the later ones to whichever CU drains first.  0: nothing
 *   post_priority=0|1    (1)    the post-processing / trace streams at the device's highest stream priority: their short kernels are placed as
 *                               soon as a CU drains instead of queueing behind the next forward's workgroups
 *   device_polygons=0|1  (1)    with device contours on square maps: Douglas-Peucker, the >= 4 points filter and the box-score job list on
 *                               the GPU as well (candidates.hip): with device_unclip the whole chain from the probability map to the adjusted
 *                               polygons stays on the device and the host only collects.  0: contours back to the host pool
 *   mfma=split_bf16|f32  (split_bf16)  how the f32 precision multiplies in the MFMA-bound convs that have no Winograd kernel
 *                               of their own (stride-2 3x3, in5, FPN phase convs, bin_conv1 over the pyramid, the Winograd GEMMs of
 *                               layer3 / layer4, out4 and out5).  split_bf16: every f32 operand as the exact sum of three bf16 terms, six partial
 *                               products per pair on v_mfma_f32_32x32x16_bf16, f32 accumulation - the error of an f32 FMA chain
 *                               (dropped terms <= 2^-23 of a product; profiles/r03_bf16x3_accuracy.txt), the same parity bars, up to
 *                               2.67 x the f32 matrix rate.  f32: every conv on v_mfma_f32_32x32x2_f32 (exact f32 FMA chain).
 *   pre_stage_mb=<n>     (256)  device staging budget of ocr_preprocess_batch in MiB, 1..4096 (host sources, frames on their way to the host); a
 *                               batch that needs more runs in several chunks, an image larger than the budget grows it.  Same bits
 *   precision=f32|bf16   (f32)  same as ocr_det_set_precision
 * Any other key is OCR_ERR_INVALID ("unknown detector option").  That includes x3_wide, winograd43_x3 and transform_fuse, which earlier versions
 * accepted: the kernels they selected were measured no faster than the defaults and left the library (docs/history.md). */
int ocr_det_create_with_options(const void* weights, size_t weights_bytes, int device, const char* options,
                                ocr_det_t** out);
/* Size limit of one launch.  The kernels address every tensor with 32-bit BYTE offsets below the out-of-range marker 2^31
 * (that marker is how zero padding and ragged tiles are expressed: such a lane reads zeros / its store is dropped), so every
 * workspace tensor must stay under 2^31 bytes.  The largest one holds N x (H/4) x (W/4) x 256 f32 = 64 N H W bytes: the engine
 * runs a batch in chunks of floor((2^31 - 1) / (64 H W)) frames - 81 at 640 x 640, 31 at 1024 x 1024, 7 at 2048 x 2048 - one
 * after the other on the handle's stream.  Results do not depend on the chunking (frames are independent in eval mode;
 * tests/test_gpu_fullsize.py).  Callers see it only as launch granularity. */
/* The one-call replacement of `vs.load(file)` (text_detection/mod.rs:41-44): reads the file tch's
 * VarStore::save wrote (utils.rs:55-63) - a libtorch zip archive of named tensors - without libtorch or Python,
 * checks names and shapes against the graph of model.rs:68-105 and builds the detector. */
int ocr_det_create_from_varstore(const char* path, int device, ocr_det_t** out);
void ocr_det_destroy(ocr_det_t* det);

/* Run all later work of this handle on an existing hipStream_t (e.g. the stream
 * of a torch.cuda.Stream).  NULL restores the handle's own stream.
 * Lifetime: the stream must outlive the handle, or be reset to NULL before it is destroyed - ocr_det_destroy
 * (and ocr_rec_destroy) wait for the work they queued on it before freeing the buffers that work touches. */
int ocr_det_set_stream(ocr_det_t* det, void* hip_stream);

/* Arithmetic of the detector (the reference runs f32 only; BASELINE config 5 names bf16 as the optional
 * reduced precision).  OCR_PRECISION_F32 (default): everything f32, the parity configuration.
 * OCR_PRECISION_BF16: every convolution of the graph - conv1, layer1..4, in2..5, out2..5, bin_conv1 and
 * bin_conv_tr1 - takes bf16 activations and weights on the bf16 matrix cores with f32 accumulation; folded
 * batch norm, residual adds, ReLU are f32 on the accumulators and the stored activations are bf16.  The last
 * transposed conv (64 -> 1), the sigmoid and all of the post-processing stay f32.  Inputs and outputs of every
 * entry point keep their f32 layout (raw 0..255 luma is exact in bf16). */
#define OCR_PRECISION_F32 0
#define OCR_PRECISION_BF16 1
int ocr_det_set_precision(ocr_det_t* det, int precision);

/* forward_t(xs, train=false): x is N x 1 x H x W f32 (raw 0..255 luma, no
 * normalisation - text_detection/mod.rs:46-54), prob is N x 1 x H x W f32 in
 * (0,1).  H and W must be multiples of 32.  Blocking. */
int ocr_det_forward(ocr_det_t* det, const float* x, int n, int h, int w, float* prob, int mem_kind);

/* The same from the u8 image itself: the reference's frame IS u8 luma, turned into the f32 tensor without scaling
 * (image_ops.rs:350-364, text_detection/mod.rs:46-51); here that conversion happens inside the first kernel, so a host
 * batch crosses PCIe as 1 byte per pixel instead of 4.  Bit-identical to ocr_det_forward on (float)x.  Blocking. */
int ocr_det_forward_u8(ocr_det_t* det, const uint8_t* x, int n, int h, int w, float* prob, int mem_kind);

/* Pinned (page-locked) host memory for frames and maps: host-memory entry points copy from / to such buffers
 * asynchronously at PCIe speed; ordinary pageable memory also works, at the runtime's staging speed, and makes the
 * copy part of a call synchronous. */
int ocr_host_alloc(size_t bytes, void** out);
void ocr_host_free(void* p);

/* Same, device pointers only, returns after enqueueing on the handle's stream.
 * If bitmap != NULL it also receives binarize(prob, thresh) (metrics.rs:129-131)
 * as N x 1 x H x W u8, fused into the last kernel. */
int ocr_det_forward_async(ocr_det_t* det, const float* x_dev, int n, int h, int w, float* prob_dev,
                          uint8_t* bitmap_dev, float thresh);
int ocr_det_synchronize(ocr_det_t* det);
/* Which schedule the most recent forward of this handle took (engine option front_split): *k = frames of the first frame group, 0 = it ran
 * unsplit (the last chunk's, for a batch that ran in several).  Results never depend on it. */
int ocr_det_last_front_split(ocr_det_t* det, int32_t* k);
/* ... and which moves of engine option top_side it took: a mask of 1 (layer4's shortcut conv), 2 (in4) and 4 (out5) on the side stream, 0 =
 * none.  Results never depend on it. */
int ocr_det_last_top_side(ocr_det_t* det, int32_t* moves);

/* Per-kernel timing of one forward (hipEvents on the handle's stream around every
 * launch).  names[i] points to a static string; ms/flops/bytes are per launch:
 * algorithmic 2*MAC FLOPs and compulsory read+write bytes of that launch.
 * Returns the number of launches written (<= max_entries) through n_entries. */
int ocr_det_forward_profile(ocr_det_t* det, const float* x_dev, int n, int h, int w, float* prob_dev,
                            int max_entries, const char** names, float* ms, double* flops,
                            double* bytes, int* n_entries);

/* ---------------------------------------------------------------------------
 * Pre-processing (the step in front of the detector).  Replaces the arithmetic of
 *   preprocess_image(file, (W, H)) -> (GrayImage, adjust_x, adjust_y)   image_ops.rs:188-220
 * after decoding: rgba is h x w x 4 u8.  Aspect-preserving Triangle resize (image 0.23.11
 * sampling: vertical then horizontal pass, u8-truncating), to_luma, zero padding to
 * target_w x target_h.  gray (u8) and/or gray_f32 (the raw 0..255 values as f32, i.e. the
 * N=1 input frame of ocr_det_forward) receive target_h x target_w values; adj_xy[2] =
 * resized / original (x, y).  `det` supplies the GPU and stream.  Blocking.
 * ------------------------------------------------------------------------- */
int ocr_preprocess_image(ocr_det_t* det, const uint8_t* rgba, int w, int h, int target_w, int target_h,
                         uint8_t* gray, float* gray_f32, double* adj_xy, int mem_kind);

/* The same for a batch of decoded images of differing sizes: images[i] -> frame i of gray (N x target_h x target_w u8) and / or
 * gray_f32 (N x 1 x target_h x target_w f32, the input of ocr_det_forward), adj_xy[2i], adj_xy[2i + 1] = resized / original.
 * Rule: frame i and its adjust values are bit for bit what ocr_preprocess_image gives for images[i] alone, whatever the batch and
 * the position in it; the zero padding right of and below the resized image is written (the outputs may arrive uninitialised).
 * One kernel launch covers the batch: vertical pass, horizontal pass and luma per output tile, nothing in between goes to HBM;
 * the weight tables are built once per distinct (in, out) size pair of the call.
 * Memory kinds: the descriptor array and adj_xy are host memory.  src_mem_kind says where the pixels of EVERY image live,
 * dst_mem_kind where BOTH outputs live; all four combinations.  Host pixels may be pageable or from ocr_host_alloc, at any
 * alignment and stride; they are packed into a device staging area (engine option pre_stage_mb=<1..4096>, default 256; an image
 * larger than that grows it).  A batch that does not fit is staged and run in several chunks inside the call; results do not
 * depend on the chunking.  Device pixels must be 4-byte aligned.
 * Stream rule: runs on the handle's stream behind whatever is queued there and blocks until the outputs are complete.  Staging
 * and plans are storage of the call's own, not the post-processing scratch: the call is legal while a pipelined batch is pending
 * on the handle (ocr_det_detect_pipelined*) and leaves that batch alone.
 * Errors: OCR_ERR_INVALID for a null det, images or adj_xy, both outputs null, n < 0, an image with null pixels, w or h outside
 * 1..16384, a stride below 4 * w or not a multiple of 4, a target size below 1, a memory kind other than the two, a misaligned
 * device source; the message names the first offending image.  n = 0 does nothing and is OCR_OK.  The handle stays usable.
 * ocr_preprocess_image is unchanged and remains the single-image form. */
typedef struct ocr_image {
  const uint8_t* rgba;    /* h rows of w RGBA pixels (the reference's into_rgba()) */
  int32_t w, h;           /* 1..16384 each */
  int64_t stride_bytes;   /* distance between rows; 0 = 4 * w; otherwise >= 4 * w and a multiple of 4 */
} ocr_image_t;
int ocr_preprocess_batch(ocr_det_t* det, const ocr_image_t* images, int n, int src_mem_kind, int target_w, int target_h,
                         uint8_t* gray, float* gray_f32, int dst_mem_kind, double* adj_xy /* [2n], host */);
/* Device pixels in, device frames out; queues on the handle's stream and returns without synchronising it (nor does it wait to
 * release its plan: descriptors and weight tables go up in one copy from one of two handle-owned pinned buffers, each guarded by
 * an event, so back-to-back calls do not wait for each other's kernels).  adj_xy is computed on the host and valid on return.
 * The frames are consumable by ocr_det_forward_async on the same handle with no synchronisation in between.  Sources and
 * outputs must stay valid until ocr_det_synchronize.  Same errors as the blocking form. */
int ocr_preprocess_batch_async(ocr_det_t* det, const ocr_image_t* images, int n, int target_w, int target_h,
                               uint8_t* gray_dev, float* gray_f32_dev, double* adj_xy);

/* ---------------------------------------------------------------------------
 * Detection post-processing.  Replaces
 *   get_boxes_and_box_scores(pred, adjust_values) -> Result<PolygonScores>
 *                                                  text_detection/metrics.rs:37-56
 * (binarize :129, get_polygons_from_bitmap :58-127, box_score_fast :150-184,
 *  get_min_area_bounding_box :133-148, polygon.rs expand_polygon :51-56).
 * PolygonScores{ polygons: Vec<MultiPolygon<u32>>, scores: Vec<Vec<f64>> } is
 * returned as one CSR block owned by the library.
 * ------------------------------------------------------------------------- */
typedef struct ocr_postproc_params {
  double thresh;        /* 0.6  metrics.rs:38  */
  double box_thresh;    /* 0.7  metrics.rs:64  */
  double min_size;      /* 5.0  metrics.rs:66  */
  double unclip_ratio;  /* 2.0  metrics.rs:103 */
  /* A candidate whose offset polygon is empty (zero-area contour) makes the reference
   * abort: `expand_polygon(..).unwrap()`, metrics.rs:103 with panic = "abort".
   * 0 (default) = report it as OCR_ERR_DEGENERATE; 1 = drop that candidate and go on. */
  int32_t skip_degenerate;
  int32_t reserved;
} ocr_postproc_params_t;

typedef struct ocr_polygons {
  int32_t n_images;
  int32_t n_polygons;          /* total over the batch                       */
  int32_t n_vertices;          /* total over the batch                       */
  const int32_t* img_offsets;  /* [n_images+1]   polygon range of each image */
  const int32_t* poly_offsets; /* [n_polygons+1] vertex range of each polygon */
  const uint32_t* xy;          /* [2*n_vertices] x,y in ORIGINAL-image pixels (round(p/adj) as u32) */
  const double* scores;        /* [n_polygons]   box_score_fast of each kept polygon */
} ocr_polygons_t;

void ocr_postproc_default_params(ocr_postproc_params_t* p);

/* prob: N x 1 x H x W f32, adj_xy: N x 2 f64 (host memory, x then y scale =
 * resized/original, image_ops.rs:200-202).  params == NULL -> reference constants.
 * `det` supplies the GPU and stream (binarisation and box scores run as HIP
 * kernels; contour tracing and Clipper-style offsetting run on host threads).
 * Blocking.  *out must be released with ocr_polygons_free. */
int ocr_det_postprocess(ocr_det_t* det, const float* prob, int n, int h, int w, int mem_kind,
                        const double* adj_xy, const ocr_postproc_params_t* params,
                        ocr_polygons_t** out);
void ocr_polygons_free(ocr_polygons_t* p);
/* Where the polygon chain of this handle's post-processing calls ran so far (cumulative counters; diagnostic - the reference has no
 * counterpart, get_boxes_and_box_scores metrics.rs:37-127 runs on one core): out[0] images whose contours were traced on the GPU,
 * out[1] images traced on the host (device_contours off, a map the tracer does not take, an image it gave up), out[2] candidate polygons
 * the device unclip settled, out[3] candidates finished on the host, out[4] images whose whole chain - trace, Douglas-Peucker, box
 * score, unclip - stayed on the device, out[5] post-processing passes.  Results never depend on where a step ran. */
int ocr_det_post_stats(ocr_det_t* det, int64_t out[6]);

/* forward_t + get_boxes_and_box_scores over a STREAM of batches, software-pipelined inside the library: the call
 * enqueues the forward of THIS batch (device pointers; x_dev N x 1 x H x W f32 -> prob_dev, which must stay untouched
 * until the next call has returned) and, while the GPU runs it, post-processes the batch handed in by the PREVIOUS call
 * - its host geometry on the handle's thread pool, its kernels and copies on a second stream.  *prev_out receives that
 * previous batch's polygons (NULL on the first call).  Finish with x_dev = NULL: nothing is enqueued, the last
 * batch's polygons come back.  Results are exactly those of ocr_det_forward + ocr_det_postprocess per batch. */
int ocr_det_detect_pipelined(ocr_det_t* det, const float* x_dev, int n, int h, int w, float* prob_dev,
                             const double* adj_xy, const ocr_postproc_params_t* params, ocr_polygons_t** prev_out);

/* The same pipeline for frames in HOST memory - the form the reference's call sites have (CPU tensors in,
 * text_detection/mod.rs:46-67).  x_host: N x 1 x H x W frames, OCR_ELEM_F32 or OCR_ELEM_U8 (raw luma, 1/4 of the
 * bytes).  The call copies them into a double-buffered device staging area on a copy stream (asynchronous for
 * ocr_host_alloc'ed memory) - beside the forward of the previous batch -, enqueues this batch's forward behind that copy,
 * and post-processes the previous batch while the GPU works.  The probability map stays on the device unless
 * prob_host != NULL, which then holds this batch's map once the NEXT call (the one returning its polygons) has returned.
 * x_host may be reused as soon as the call returns only if it is pageable; a pinned buffer must stay untouched until
 * the next call returns.  Finish with x_host = NULL.  Batches may differ in size and element kind from call to call; a
 * batch that needs larger staging slots than the pending one is enqueued only after the pending batch has been finished
 * (that one call loses its overlap, results are unchanged).  The staging of this entry point is its own: blocking
 * ocr_det_forward / ocr_det_forward_u8 calls on host memory between two pipelined calls do not disturb the pending batch. */
#define OCR_ELEM_F32 0
#define OCR_ELEM_U8 1
int ocr_det_detect_pipelined_host(ocr_det_t* det, const void* x_host, int x_elem, int n, int h, int w, float* prob_host,
                                  const double* adj_xy, const ocr_postproc_params_t* params, ocr_polygons_t** prev_out);

/* Detect -> recognise link (BUILD-DEFINED: the reference never implemented its "Character
 * Segmentation" step, README.md:20-26, so there is no reference rule to match).  For every polygon
 * of `polys` (as returned by ocr_det_postprocess for the same batch) the axis-aligned bounding box,
 * mapped back to frame coordinates with adj_xy, is resampled bilinearly to 28 x 28 and divided by
 * 255 (load_image_as_tensor's scaling, image_ops.rs:80-83): crops is n_polygons x 784 f32, ready
 * for ocr_rec_forward / ocr_rec_classify.  frames: N x 1 x H x W f32 (the detector's input).
 * frames and crops share mem_kind; polys and adj_xy are host memory.  Rule: oracle/crop_oracle.py.
 * The box of a polygon, in f64: x0 = min(max(min_v x_v * adj_x, 0), W - 1), x1 = min(max(max_v x_v * adj_x + 1, x0 + 1), W),
 * likewise y: always inside the frame and at least one pixel wide and tall, wherever the polygon lies (a polygon off the frame
 * yields the nearest border pixel).  Non-finite adjust values: a NaN product x_v * adj_x takes no part in the minimum or the
 * maximum; an axis on which every product is NaN yields the last pixel, [W - 1, W] or [H - 1, H]; +-inf clamps like any other
 * value.  No adjust value makes the kernel read outside the frame.
 * Limits: N >= 0, 1 <= H, W <= 2^24 (sample positions are f32), polys->n_images == N; the frame block may exceed 2^31 bytes
 * (every offset is 64-bit; host frames are staged whole in device scratch, so device memory is the only bound).  N = 0 or a
 * block without polygons does nothing and writes nothing.  OCR_ERR_INVALID for anything outside the limits, a null pointer
 * (crops may be null only when there is no polygon) and a mem_kind other than OCR_MEM_HOST / OCR_MEM_DEVICE; nothing is
 * written and the handle stays usable.
 * Stream order: the crop kernel runs behind everything queued on the detector's stream when the call is made - except,
 * while a pipelined batch is pending (ocr_det_detect_pipelined*), the forward of that pending batch: the crops of the batch
 * that has come back are cut beside it, behind whatever was queued before that forward was.  Device frames written by work
 * queued AFTER the last pipelined call need the caller's own synchronisation. */
int ocr_extract_crops(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind,
                      const ocr_polygons_t* polys, const double* adj_xy, float* crops);

/* Glyph segmentation: detected words -> glyph boxes -> 28 x 28 glyph crops for the single-glyph recogniser (BUILD-DEFINED: the
 * reference's "Character Segmentation" step, README.md:20-26, was never built).  For every polygon of `polys` (a word), in polygon order:
 *  1. word box: the ocr_extract_crops box (f32 frame coordinates x0, y0, x1, y1) -> X0 = floor(x0), X1 = ceil(x1), Y0 = floor(y0),
 *     Y1 = ceil(y1), clamped to the frame, half-open; a box of more than 2^22 pixels is OCR_ERR_INVALID;
 *  2. q = (int)min(max(v, 0), 255), truncated toward zero, NaN -> 0, of the raw 0..255 f32 frame value v;
 *  3. Otsu over the 256-bin histogram of q in the box: for t in 0..254 class 0 is q <= t (count W0, int64 sum S0), class 1 the rest
 *     (W1, S1); t is valid when both classes are non-empty and scores d*d / ((double)W0 * (double)W1), d = (double)(S1*W0 - S0*W1)
 *     (the product is exact in int64); the highest score wins, ties to the smaller t.  No valid t (a flat box): t = -1, no glyphs;
 *  4. polarity 0 (auto): ink is the smaller class, dark ink on a tie; 1 forces dark ink (q <= t), 2 light ink (q > t);
 *  5. mu0 = (float)((double)S0 / W0), mu1 = (float)((double)S1 / W1); bg = the non-ink class's mean, ink = the ink class's mean
 *     (they differ: mu0 <= t < mu1);
 *  6. cnt[x] = ink pixels of column x over [Y0, Y1); a column is ink when cnt[x] >= min_col_ink; every maximal run of ink columns is a
 *     glyph span, left to right; a span with fewer than min_glyph_pixels ink pixels is dropped;
 *  7. a glyph box is [xs, xe) x [first ink row of the span, last ink row + 1);
 *  8. at most max_glyphs spans per word are kept; a word that had more is flagged truncated.
 * Glyph crop (ocr_extract_glyph_crops), 28 x 28 f32, aspect-preserving and centred (as MNIST / EMNIST): s = (float)max(gw, gh) /
 * (float)glyph_box, cx = (float)(x0 + x1) * 0.5f, sx = (cx + (((float)j + 0.5f) - 14.0f) * s) - 0.5f, sy likewise with row i;
 * bilinear taps at floor(sx), floor(sy) in ocr_extract_crops's operation order; a tap reads r = (v - bg) / (ink - bg) as
 * g = r > 0 ? min(r, 1) : 0 (NaN -> 0) inside the glyph box and 0 outside it; ink_high = 0 writes 1 - o.  f32, separately rounded.
 * Out of scope: touching or kerned glyphs (they stay one glyph), rotated or curved words (the box is axis-aligned and pixels are not
 * masked by the polygon), lexicons.  Spaces inside a polygon are ocr_break_words', on the block this call returns.  Oracle:
 * tests/glyph_oracle.py; kernels: csrc/glyphs.hip.
 * Both calls are blocking and run behind everything queued on the detector's stream; no overlap with a pending pipelined forward
 * (ocr_det_detect_pipelined*) is promised.  frames: N x 1 x H x W f32 in mem_kind memory; polys, adj_xy, params and the glyph block
 * are host memory; crops (n_glyphs x 784 f32) lives in the same mem_kind as frames.  OCR_ERR_INVALID for a null pointer, a bad mem_kind,
 * polys->n_images != n, a parameter out of range, a word box over 2^22 pixels, and (crops) a glyph block that does not fit the frames;
 * the handle stays usable. */
typedef struct ocr_segment_params {
  int32_t polarity;          /* 0 auto (default), 1 dark ink, 2 light ink        */
  int32_t min_col_ink;       /* >= 1, default 1                                   */
  int32_t min_glyph_pixels;  /* >= 0, default 4                                   */
  int32_t max_glyphs;        /* 1..256, default 32 (per word)                     */
  int32_t glyph_box;         /* 1..28, default 20: the glyph's longer side in the crop */
  int32_t ink_high;          /* 1 (default): ink = 1, background = 0; 0: inverted */
} ocr_segment_params_t;
typedef struct ocr_glyphs {
  int32_t n_images, n_words, n_glyphs;
  const int32_t* img_offsets;   /* [n_images+1] word range per image (= the polygons')                          */
  const int32_t* word_offsets;  /* [n_words+1]  glyph range per word                                            */
  const int32_t* word_info;     /* [4*n_words]  frame, t (-1 flat), polarity used (0 none), truncated (0 / 1)    */
  const float* word_levels;     /* [2*n_words]  bg, ink (0, 0 for a flat word)                                  */
  const int32_t* boxes;         /* [4*n_glyphs] x0, y0, x1, y1 frame pixels, half-open                          */
} ocr_glyphs_t;
void ocr_segment_default_params(ocr_segment_params_t* p);
/* params == NULL -> defaults.  *out must be released with ocr_glyphs_free. */
int ocr_segment_glyphs(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                       const double* adj_xy, const ocr_segment_params_t* params, ocr_glyphs_t** out);
/* glyph_box and ink_high of params (NULL -> defaults) shape the crops; the other fields are checked only. */
int ocr_extract_glyph_crops(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                            const ocr_segment_params_t* params, float* crops);
void ocr_glyphs_free(ocr_glyphs_t* g);

/* Glyph segmentation by connected components (BUILD-DEFINED, like ocr_segment_glyphs): a second entry point beside the column rule,
 * for words whose letters are kerned - their column ranges overlap, or a speck bridges a gap, without the letters touching.  For
 * every polygon of `polys` (a word), in polygon order:
 *  1. steps 1-5 of ocr_segment_glyphs unchanged: word box [X0, X1) x [Y0, Y1), quantise, Otsu, polarity, levels; a flat word (t = -1)
 *     gives no glyphs;
 *  2. a run is a maximal horizontal sequence of ink pixels in one row of the box, [a0, a1) in columns;
 *  3. a component is an 8-connected set of ink pixels: runs [a0, a1) and [b0, b1) of adjacent rows are connected when a0 <= b1 &&
 *     b0 <= a1;
 *  4. a component carries its half-open bounding box, its pixel count s and its anchor, the smallest raster index
 *     (y - Y0) * (X1 - X0) + (x - X0) of its pixels;
 *  5. limits: a word of more than 8192 runs, or of more than 1024 components before any filter, is segmented by the column rule
 *     (steps 6-8 of ocr_segment_glyphs, with `params`) and flagged 2; this is not an error;
 *  6. components with s < min_glyph_pixels are dropped;
 *  7. the rest is sorted by (x0, anchor) ascending;
 *  8. grouping walk: the first component opens a group; every next component c is compared with the current (last) group a, over the
 *     group's accumulated x range: ov = min(a.x1, c.x1) - max(a.x0, c.x0), nar = min(a.x1 - a.x0, c.x1 - c.x0); when
 *     merge_overlap_pct > 0 && ov > 0 && ov * 100 >= nar * merge_overlap_pct, c joins a (the boxes are united, the counts added),
 *     otherwise c opens a new group.  This keeps i-dots, accents and broken strokes with their letter;
 *  9. groups with (y1 - y0) * 100 < min_height_pct * (Y1 - Y0) are dropped;
 * 10. the first max_glyphs groups are kept; a word that had more is flagged 1 (truncated);
 * 11. a glyph box is the group's box in frame pixels; the boxes of a word come out ordered by x0 (they may overlap);
 * 12. min_col_ink is checked and unused, except by the fallback of step 5.
 * The result is an ordinary glyph block, released with ocr_glyphs_free and taken by ocr_extract_glyph_crops unchanged, except that
 * word_info[4k+3] is a bit set for this call: 1 = truncated, 2 = fell back to the column rule.
 * Still out of scope here: letters that actually touch (one component, one glyph - ocr_split_glyphs and ocr_lattice_decode, below,
 * cut such a glyph at ink minima and let the decode choose); one threshold per word (a word that is one blob under
 * its Otsu threshold stays one glyph).  ocr_extract_glyph_crops cuts a crop from its box alone, so a kerned neighbour's ink inside a
 * glyph's box shows in its crop: ocr_segment_glyphs_cc_labelled and ocr_extract_glyph_crops_masked, below, keep it out.
 * Oracle: tests/glyph_cc_oracle.py; kernel: csrc/glyph_cc.hip.
 * Memory kinds, blocking behaviour and the stream rule are ocr_segment_glyphs's.  OCR_ERR_INVALID in the same cases, and for a field
 * of `cc` out of range or a nonzero reserved field; the handle stays usable. */
typedef struct ocr_cc_params {
  int32_t merge_overlap_pct;  /* 0..100, default 50; 0 = never merge */
  int32_t min_height_pct;     /* 0..100, default 25 */
  int32_t reserved[2];        /* must be 0 */
} ocr_cc_params_t;
void ocr_cc_default_params(ocr_cc_params_t* p);
/* params == NULL, cc == NULL -> defaults.  *out must be released with ocr_glyphs_free. */
int ocr_segment_glyphs_cc(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                          const double* adj_xy, const ocr_segment_params_t* params, const ocr_cc_params_t* cc, ocr_glyphs_t** out);

/* Glyph crops masked by connected component (BUILD-DEFINED, like ocr_segment_glyphs_cc): the segmentation also keeps, per word, which
 * glyph every ink pixel went to, and the crop call reads a kerned neighbour's ink as background.
 * Label planes.  Word k with the box [X0, X1) x [Y0, Y1), bw = X1 - X0, bh = Y1 - Y0, owns a plane of bh x bw uint16_t, row-major, at
 * element offset plane_offsets[k]; plane_offsets[k + 1] - plane_offsets[k] = bw * bh.  After steps 1-11 of ocr_segment_glyphs_cc the
 * plane holds
 *   0       where the pixel is not ink, and everywhere when the word is flat (t = -1) or fell back to the column rule (flag 2):
 *           such a word is not masked;
 *   g + 1   (1 .. max_glyphs) for an ink pixel of a component in the group that became glyph g of the word (its box is
 *           word_offsets[k] + g);
 *   0xFFFF  for every other ink pixel: a component dropped at step 6, a component of a group dropped at step 9, a component of a
 *           group past the first max_glyphs (step 10), those the truncated walk never reaches included.
 * Masked tap.  The masked crop call is ocr_extract_glyph_crops with the tap changed and nothing else: sample positions, the operation
 * order of the bilinear blend and ink_high are that call's.  For glyph g of word k let m = g + 1 and L(x, y) the plane value inside
 * the word box, 0 outside it.  A tap at pixel (x, y) reads
 *   1. outside the glyph box: 0;
 *   2. l = L(x, y); l != 0 && l != m: 0;
 *   3. l == 0 && halo == 1: over the eight neighbours (x + dx, y + dy), foreign = some neighbour has L not in {0, m}, own = some
 *      neighbour has L == m; foreign && !own: 0 (the anti-aliased rim of a neighbour's stroke goes with the stroke);
 *   4. otherwise the unmasked value g = r > 0 ? min(r, 1) : 0, r = (v - bg) / (ink - bg).
 * Steps 2 and 3 are integer tests: an all-zero plane gives the bits of ocr_extract_glyph_crops, and so does every glyph whose box
 * holds no foreign ink and has none within one pixel of it.  Oracle: tests/glyph_mask_oracle.py; kernels: csrc/glyph_cc.hip
 * (segment_cc_labelled_kernel), csrc/glyphs.hip (glyph_crop_masked_kernel).
 * The labelled segmentation returns, array for array, the glyph block of ocr_segment_glyphs_cc for the same arguments (the fallback
 * of step 5 included), and the label block beside it.  The planes stay in device memory for either mem_kind - the crop call follows
 * at once - in one allocation per call that the library owns until the label block is freed; a total of more than 2^31 - 1 plane elements is
 * OCR_ERR_INVALID.  Blocking; memory kinds and the stream rule are ocr_segment_glyphs_cc's.  The read call copies all planes to host
 * memory (plane_offsets[n_words] uint16_t), blocking, for inspection and tests.
 * The masked crop call has the memory kinds, blocking behaviour and checks of ocr_extract_glyph_crops, and is OCR_ERR_INVALID also for
 * null labels, labels->n_words != glyphs->n_words, labels->device other than the handle's device, a label block whose offsets do not
 * fit its word boxes, a glyph box not inside its word's word_boxes entry, a word of more than 65534 glyphs, halo outside 0..1 or a
 * nonzero reserved field; mask == NULL -> defaults.  The handle stays usable after any error. */
typedef struct ocr_glyph_labels {
  int32_t n_words;
  int32_t device;                /* the GPU the planes live on */
  const int32_t* word_boxes;     /* [4*n_words] X0, Y0, X1, Y1 frame pixels, half-open (host) */
  const int64_t* plane_offsets;  /* [n_words+1], in elements (host) */
  const uint16_t* planes;        /* DEVICE memory, plane_offsets[n_words] elements; NULL when that is 0 */
} ocr_glyph_labels_t;
typedef struct ocr_mask_params {
  int32_t halo;         /* 0 | 1, default 1 */
  int32_t reserved[3];  /* must be 0 */
} ocr_mask_params_t;
void ocr_mask_default_params(ocr_mask_params_t* p);
/* params == NULL, cc == NULL -> defaults.  *out is released with ocr_glyphs_free, *labels with ocr_glyph_labels_free. */
int ocr_segment_glyphs_cc_labelled(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_polygons_t* polys,
                                   const double* adj_xy, const ocr_segment_params_t* params, const ocr_cc_params_t* cc,
                                   ocr_glyphs_t** out, ocr_glyph_labels_t** labels);
int ocr_glyph_labels_read(ocr_det_t* det, const ocr_glyph_labels_t* labels, uint16_t* planes_host);
int ocr_extract_glyph_crops_masked(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                                   const ocr_glyph_labels_t* labels, const ocr_segment_params_t* params, const ocr_mask_params_t* mask,
                                   float* crops);
void ocr_glyph_labels_free(ocr_glyph_labels_t* l);

/* Word strips: every detected word (a polygon, possibly rotated) warped into an upright strip of strip_height rows, all strips of a
 * batch side by side in one atlas (BUILD-DEFINED, like ocr_segment_glyphs).  Frame coordinates are continuous: frame pixel p spans
 * [p, p + 1), and a vertex (x, y) is the point (x * adj_x, y * adj_y).
 * Geometry (ocr_plan_word_strips, host C++, f64, every operation separately rounded, no FMA), for every polygon in polygon order:
 *  1. hull: the convex hull of the u32 vertices, exact in int64 (Andrew's monotone chain): repeated vertices merged, collinear points
 *     dropped, counter-clockwise in the x-right / y-up sense (cross((b - a), (c - a)) > 0 at every vertex), starting at the smallest
 *     (x, y).  A coordinate >= 2^24 or a polygon without vertices is OCR_ERR_INVALID.  m = the hull's vertex count.  Then every hull
 *     vertex P is mapped to the frame: (x * adj_x, y * adj_y).  m < 3 (one point, repeated copies of one point, two points, all points
 *     collinear) flags the word degenerate;
 *  2. rectangle: for every hull edge i (m >= 3: i = 0..m-1, from P_i to P_(i+1) mod m; m = 2: edge 0 only; m = 1: e = (1, 0) from
 *     P_0), e = P_(i+1) - P_i, ee = ex*ex + ey*ey; for every hull vertex Q, d = Q - P_i, a = dx*ex + dy*ey, b = dy*ex - dx*ey; with the
 *     ranges [a0, a1], [b0, b1] over Q, area_i = ((a1 - a0) * (b1 - b0)) / ee.  The smallest area wins, ties to the smaller i.  Corner
 *     (a, b) = (P_ix + (a*ex - b*ey) / ee, P_iy + (a*ey + b*ex) / ee); R0 = (a0, b0), R1 = (a1, b0), R2 = (a1, b1), R3 = (a0, b1);
 *  3. reading direction u: of +e, -e, +e' = (-ey, ex), -e' the one with the largest x component, ties to the smaller y component (at
 *     exactly 45 degrees the direction pointing up wins); v = (-u_y, u_x) points down the strip.  TL, TR, BR, BL = R0..R3 rotated
 *     cyclically: +e: R0 R1 R2 R3; +e': R1 R2 R3 R0; -e: R2 R3 R0 R1; -e': R3 R0 R1 R2.  So words within 45 degrees of horizontal come
 *     out upright, steeper words come out turned by 90 degrees, and upside-down text reads upside down (none of it is detected);
 *  4. U = TR - TL, |U| = sqrt(Ux*Ux + Uy*Uy) (IEEE sqrt), likewise V = BL - TL.  |U| < 1: h = (1 - |U|) * 0.5, s = sqrt(ux*ux + uy*uy),
 *     dx = h * (ux / s), dy = h * (uy / s); TL and BL move by -(dx, dy), TR and BR by +(dx, dy); U, V and their lengths are taken from
 *     the corners again.  Then the same for |V| < 1 with v (TL, TR by -, BL, BR by +);
 *  5. Ws = floor((Hs * |U|) / |V| + 0.5) with Hs = strip_height, clamped to [1, max_width]; above max_width flags the word squeezed;
 *  6. map, each value rounded once from f64 to f32: (ox, oy) = TL, (ux, uy) = U / Ws, (vx, vy) = V / Hs.
 * Sampling (ocr_extract_word_strips, csrc/strips.hip, f32, separately rounded): word k owns atlas columns [col_offsets[k],
 * col_offsets[k+1]); atlas pixel (i, j) of word k with c = j - col_offsets[k] samples frame word_info[2k] at
 * sx = ((ox + ((float)c + 0.5f) * ux) + ((float)i + 0.5f) * vx) - 0.5f, sy likewise with (oy, uy, vy), clamped as fminf(fmaxf(s, 0),
 * W - 1 or H - 1) (NaN -> 0), bilinear taps in ocr_extract_crops's operation order, the raw 0..255 value (no / 255): the atlas is a valid
 * frame for ocr_segment_glyphs, with the rectangles of ocr_word_strip_polygons and adj = (1, 1).
 * Out of scope: curved words (ocr_plan_curved_strips below reads those), pixels inside the rectangle but outside the polygon (not masked),
 * upside-down or vertical text detection.
 * Oracle: tests/strip_oracle.py.  ocr_plan_word_strips needs no GPU (det is not taken).  ocr_extract_word_strips is blocking and runs
 * behind everything queued on the detector's stream, like the glyph calls; frames (N x 1 x H x W f32) and atlas (height x total_width
 * f32, row-major) live in mem_kind memory, the strips block in host memory.  An empty polygon list gives total_width = 0 and launches
 * nothing.  OCR_ERR_INVALID for a null pointer, a bad mem_kind, polys->n_images != n (or strips->n_images != n), a bad shape, params out
 * of range or nonzero reserved fields, an adjust value that is not finite and > 0, a strips block whose offsets or frame indices do not
 * fit, and an atlas of more than 2^31 elements; the handle stays usable. */
typedef struct ocr_strip_params {
  int32_t strip_height;  /* 8..128, default 32 */
  int32_t max_width;     /* 1..8192, default 1024 (per word) */
  int32_t reserved[2];   /* must be 0 */
} ocr_strip_params_t;
typedef struct ocr_word_strips {
  int32_t n_images, n_words, height, total_width;
  const int32_t* img_offsets;  /* [n_images+1] word range per image (= the polygons')        */
  const int32_t* col_offsets;  /* [n_words+1]  atlas columns per word                       */
  const int32_t* word_info;    /* [2*n_words]  frame, flags (1 squeezed, 2 degenerate)      */
  const double* quads;         /* [8*n_words]  TL, TR, BR, BL (x, y) in frame coordinates   */
  const float* maps;           /* [6*n_words]  ox, oy, ux, uy, vx, vy as the kernel uses them */
  const double* scores;        /* [n_words]    the source polygons' scores                  */
} ocr_word_strips_t;
void ocr_strip_default_params(ocr_strip_params_t* p);
/* params == NULL -> defaults; h and w are checked only (the rectangle is not clipped to the frame).  *out: ocr_word_strips_free. */
int ocr_plan_word_strips(const ocr_polygons_t* polys, const double* adj_xy, int n, int h, int w, const ocr_strip_params_t* params,
                         ocr_word_strips_t** out);
int ocr_extract_word_strips(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_word_strips_t* strips,
                            float* atlas);
/* One image, n_words rectangles (c0, 0), (c1 - 1, 0), (c1 - 1, Hs - 1), (c0, Hs - 1) of the atlas with the source scores: with
 * adj = (1, 1) the crop box of rectangle k is exactly word k's columns.  *out: ocr_polygons_free. */
int ocr_word_strip_polygons(const ocr_word_strips_t* strips, ocr_polygons_t** out);
void ocr_word_strips_free(ocr_word_strips_t* s);

/* Curved strips: a second planner and sampler beside the word strips, for words whose baseline bends (an arc on a logo, a seal, a
 * label).  The strip follows the centreline of the polygon's own ring, and every atlas column runs along the centreline's normal, so
 * the glyphs of an arc come out upright and at full height (BUILD-DEFINED, like the word strips; nothing of those changes).
 * Geometry (ocr_plan_curved_strips, host C++, f64, every operation separately rounded, no FMA; hypot is libm's as glibc 2.35 computes
 * it, the restatement the post-processing already uses), for every polygon in polygon order:
 *  1. rectangle: steps 1-4 of ocr_plan_word_strips unchanged give TL, TR, BR, BL, U = TR - TL, V = BL - TL, |U| and |V|;
 *     eu = U / |U|, ev = V / |V| per component.  A degenerate word (flag 2) takes the straight fallback of step 9;
 *  2. ring: all vertices of the polygon in their order (not the hull), each mapped to the frame as P = (x * adj_x, y * adj_y); its
 *     rectangle coordinates are a = dx * eu_x + dy * eu_y and b = dx * ev_x + dy * ev_y with d = P - TL;
 *  3. scan lines s = 0..31 at a_s = (|U| * (s + 0.5)) / 32.  An edge A -> B of the closed ring crosses line s when
 *     (a_A <= a_s) != (a_B <= a_s), at b = b_A + ((a_s - a_A) * (b_B - b_A)) / (a_B - a_A).  top_s = min b and bot_s = max b over the
 *     crossings (both 0 on a line without one), m_s = (top_s + bot_s) * 0.5, t_s = bot_s - top_s.  More than two crossings on any
 *     line set flag 4 (folded); the min and max are still used;
 *  4. valid span: tm = element 16 of the ascending sort of the t_s.  Line s is valid when t_s * 100 >= valid_pct * tm (this excludes
 *     lines that cross an end cap instead of the two long sides).  lo and hi are the first and the last valid s; the lines between
 *     them are all used.  tm <= 0 or hi - lo < 1 takes the straight fallback;
 *  5. centreline: the polyline Q = (0, m_lo - s0 * a_lo), then (a_s, m_s) for s = lo..hi, then (|U|, m_hi + s1 * (|U| - a_hi)), with
 *     s0 = (m_(lo+1) - m_lo) / (a_(lo+1) - a_lo) and s1 = (m_hi - m_(hi-1)) / (a_hi - a_(hi-1)) the slopes of the first and the last
 *     segment of the valid span.  len_i = hypot(da, db) of segment i, start_0 = 0, start_(i+1) = start_i + len_i, L = the last start.
 *     Flag 8 (steep) is set when some segment has |db| * 10 > |da| * 7;
 *  6. half height: for every s in lo..hi, d = Q_next - Q_prev around that point, c = d_a / hypot(d_a, d_b), hh_s = (t_s * c) * 0.5;
 *     h = element cnt / 2 (integer division, cnt = hi - lo + 1) of the ascending sort of the hh_s, raised to 0.5 if smaller;
 *  7. width: Ws = floor((Hs * L) / (2 * h) + 0.5) with Hs = strip_height, clamped to [1, max_width]; above max_width flags the word
 *     squeezed (flag 1).  tscale = (float)(32.0 / Ws);
 *  8. knots r = 0..32: P_r is the point of Q at arc length l = (L * r) / 32: on the segment i with the largest index whose start_i <= l,
 *     P = Q_i + ((l - start_i) * (Q_(i+1) - Q_i)) / len_i per coordinate; P_32 is the last point of Q exactly.
 *     T_r = P_min(r+1,32) - P_max(r-1,0), each component divided by its hypot; N_r = ((-T_b) * k, T_a * k) with k = (2 * h) / Hs.
 *     In the frame p = (TL + P_a * eu) + P_b * ev and n = N_a * eu + N_b * ev per component; each of the four values is rounded once
 *     to f32;
 *  9. straight fallback (flag 16, alongside flag 2 where it applies): P_r = (TL + U * (r / 32.0)) + V * 0.5, n = V / Hs, h = |V| / 2,
 *     L = |U|, Ws as in step 5 of the straight rule.
 * Sampling (ocr_extract_curved_strips, csrc/curved_strips.hip, f32, separately rounded): word k owns atlas columns [col_offsets[k],
 * col_offsets[k+1]); atlas pixel (i, j) of word k samples frame word_info[2k]: c = j - col_offsets[k], t = ((float)c + 0.5f) * tscale,
 * r = min((int)t, 31), f = t - (float)r, px = p_r.x + f * (p_(r+1).x - p_r.x) and py, nx, ny likewise, o = ((float)i + 0.5f) -
 * 0.5f * (float)Hs, sx = (px + o * nx) - 0.5f and sy likewise.  The clamp, the bilinear taps and the blend are exactly those of
 * ocr_extract_word_strips; the atlas holds raw 0..255 values and, with the rectangles of ocr_curved_strip_polygons and adj = (1, 1),
 * is a valid frame for every glyph call.
 * Out of scope: words that turn by more than about 70 degrees in total (their end columns are extended linearly and come out slanted;
 * flag 8 reports it), folded shapes (flag 4 reports them), a second scan along the centreline's own normals, masking pixels outside
 * the polygon, vertical or upside-down text.
 * Oracle: tests/curved_strip_oracle.py.  Memory kinds, blocking, the stream rule and the error cases are those of the word strip
 * calls: ocr_plan_curved_strips needs no GPU (det is not taken); OCR_ERR_INVALID for a null pointer, a bad mem_kind, n_images != n, a
 * bad shape, a parameter out of range, a nonzero reserved field, an adjust value that is not finite and > 0, a block whose offsets,
 * frame indices or tscale values (finite and > 0) do not fit, and an atlas of more than 2^31 elements; the handle stays usable.  An
 * empty polygon list gives total_width = 0 and launches nothing. */
#define OCR_CURVE_SCANLINES 32
#define OCR_CURVE_KNOTS 33 /* K + 1, K = 32 intervals */
typedef struct ocr_curve_params {
  int32_t strip_height;  /* 8..128, default 32 */
  int32_t max_width;     /* 1..8192, default 1024 (per word) */
  int32_t valid_pct;     /* 1..100, default 80 */
  int32_t reserved;      /* must be 0 */
} ocr_curve_params_t;
typedef struct ocr_curved_strips {
  int32_t n_images, n_words, height, total_width;
  const int32_t* img_offsets;  /* [n_images+1] word range per image (= the polygons')                             */
  const int32_t* col_offsets;  /* [n_words+1]  atlas columns per word                                            */
  const int32_t* word_info;    /* [2*n_words]  frame, flags (1 squeezed, 2 degenerate, 4 folded, 8 steep, 16 straight fallback) */
  const float* knots;          /* [4*33*n_words] px, py, nx, ny per knot, as the kernel uses them                */
  const float* tscale;         /* [n_words]    (float)(32.0 / Ws)                                                */
  const double* half_heights;  /* [n_words]    h                                                                 */
  const double* lengths;       /* [n_words]    L                                                                 */
  const double* scores;        /* [n_words]    the source polygons' scores                                       */
} ocr_curved_strips_t;
void ocr_curve_default_params(ocr_curve_params_t* p);
/* params == NULL -> defaults; h and w are checked only.  *out: ocr_curved_strips_free. */
int ocr_plan_curved_strips(const ocr_polygons_t* polys, const double* adj_xy, int n, int h, int w, const ocr_curve_params_t* params,
                           ocr_curved_strips_t** out);
int ocr_extract_curved_strips(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_curved_strips_t* strips,
                              float* atlas);
/* The rule of ocr_word_strip_polygons: one image, n_words rectangles of the atlas with the source scores.  *out: ocr_polygons_free. */
int ocr_curved_strip_polygons(const ocr_curved_strips_t* strips, ocr_polygons_t** out);
void ocr_curved_strips_free(ocr_curved_strips_t* s);

/* Line grouping: the words of every page linked into text lines, the lines in reading order (BUILD-DEFINED, like the strips: the
 * reference's "output text" step was never built).  Input per image is its words as quads, 8 doubles TL, TR, BR, BL each, exactly the
 * `quads` of ocr_word_strips_t; word_img_offsets [n_images+1] is the word range per image (its img_offsets).  All arithmetic is f64,
 * every operation separately rounded, no FMA; sqrt and divide are IEEE.
 * Word k:  U = TR - TL, V = BL - TL; lu = sqrt(Ux*Ux + Uy*Uy), lv likewise from V; C = ((TLx + BRx) * 0.5, (TLy + BRy) * 0.5);
 *   u = (Ux / lu, Uy / lu), v likewise.  A word with lu == 0 or lv == 0 is isolated (flag 1): it takes part in no link and is a line
 *   of its own.
 * Word j is a right candidate of word i when both are non-isolated words of one image, j != i, and with d = Cj - Ci,
 *   a = dx*uix + dy*uiy, b = dx*vix + dy*viy, hmin = min(lvi, lvj), hmax = max(lvi, lvj):
 *    1. a > 0;
 *    2. fabs(b) <= line_tol * hmin;
 *    3. hmax <= height_ratio * hmin;
 *    4. uix*ujx + uiy*ujy >= min_cos;
 *    5. g <= max_gap * hmax, with g = a - (lui + luj) * 0.5.
 * Links:  right[i] is the candidate j with the smallest a, ties to the smaller j, -1 without one.  left[j] is the i, among all i that
 *   have j as a right candidate, with the smallest a (the a computed in i's frame), ties to the smaller i.  The link i -> j exists iff
 *   right[i] == j && left[j] == i.
 * Links form chains.  A ring of words (a seal) can close a chain into a cycle: it is cut on the link that enters its smallest-index
 *   word, which gets flag 2.  A line is a chain, head to tail.  The lines of an image are ordered by (Cy, Cx, index) of their head
 *   word, ascending.  gaps[p] is g / hmax of the link that leads to the word at position p of `order`, 0.0 for a head: callers decide
 *   from it what is a space and what is a tab.
 * Out of scope: column detection (two columns closer than max_gap heights merge line by line, and the lines of wider-spaced columns
 *   interleave by height), right-to-left and vertical scripts, paragraph structure.  Spaces inside a polygon are ocr_break_words':
 *   the reading calls put them into a word's text before the lines join the texts.
 * Oracle: tests/line_oracle.py; kernels: csrc/lines.hip (link kernel over all pairs of an image, chain kernel per image).
 * The call is blocking and runs behind everything queued on the detector's stream, like the glyph calls (no overlap with a pending
 * pipelined forward is promised).  All pointers are host memory.  OCR_ERR_INVALID for a null pointer (params == NULL -> defaults),
 * offsets that do not start at 0 or decrease, n_images < 1, a parameter out of range or a nonzero reserved field, a non-finite
 * coordinate, more than 4096 words in one image; all of it is checked on the host before anything is launched, and the handle stays
 * usable.  Zero words in the batch launch nothing and return an empty block with valid offsets. */
#define OCR_LINE_MAX_WORDS 4096 /* per image, the polygon chain's contour limit */
typedef struct ocr_line_params {
  double line_tol;      /* (0, 4],  default 0.5   */
  double height_ratio;  /* [1, 16], default 2.0   */
  double min_cos;       /* [0, 1],  default 0.866 */
  double max_gap;       /* [0, 64], default 3.0   */
  int32_t reserved[2];  /* must be 0 */
} ocr_line_params_t;
typedef struct ocr_lines {
  int32_t n_images, n_words, n_lines;
  const int32_t* img_offsets;   /* [n_images+1] line range per image              */
  const int32_t* line_offsets;  /* [n_lines+1]  range of `order` per line         */
  const int32_t* order;         /* [n_words]    batch-global word indices, reading order */
  const int32_t* word_flags;    /* [n_words]    by word index: 1 isolated, 2 cycle cut here */
  const double*  gaps;          /* [n_words]    by position in `order`            */
} ocr_lines_t;
void ocr_line_default_params(ocr_line_params_t* p);
/* *out: ocr_lines_free. */
int  ocr_group_lines(ocr_det_t* det, const double* quads, const int32_t* word_img_offsets, int n_images,
                     const ocr_line_params_t* params, ocr_lines_t** out);
void ocr_lines_free(ocr_lines_t* l);

/* Column-aware reading order: the words of every page as blocks (columns, paragraphs) in reading order, every block its lines top to
 * bottom, every line its words left to right (BUILD-DEFINED; the reference has no counterpart).  Input, arithmetic (f64, every
 * operation separately rounded, no FMA, IEEE sqrt and divide; a dot product is dx*ux + dy*uy in that order) and the word features C,
 * u, v, lu, lv and "isolated" are those of ocr_group_lines.  L = C - u * (lu * 0.5) is the midpoint of a word's left edge, R = C +
 * u * (lu * 0.5) of its right edge.  min(a, b) is b < a ? b : a and max(a, b) is b > a ? b : a; a min or max over a sequence starts
 * with its first value and replaces on a strict improvement.  Every scan ascends over indices and replaces on a strict improvement
 * only (ties go to the smaller index).  "Mutual nearest" links: next[p] is the candidate of p with the smallest a; prev[q] is the p
 * with the smallest a among those that have q as a candidate, a measured in p's frame; the link p -> q exists iff next[p] == q &&
 * prev[q] == p.
 * A. Rows: the links of ocr_group_lines with row_gap in place of max_gap, its mutual links and its cycle cut (flag 2).  A link i -> j
 *    carries g = a - (lui + luj) * 0.5 and hmax = max(lvi, lvj) of the pair test in i's frame.
 * B. Gutters: every link of A is a gap element, indexed by its right word j: centre G = (Ri + Lj) * 0.5, frame (ui, vi), half width
 *    w = g * 0.5, height h = hmax.  It is wide when g > max_gap * h and eligible when g >= min_gutter * h.  Element q is a below
 *    candidate of p when both are eligible and, with d = Gq - Gp: a = d . vp > 0; fabs(d . up) < wp + wq; a <= gutter_reach *
 *    max(hp, hq); up . uq >= min_cos.  Mutual nearest links give chains of stacked gaps; the size of an element is the number of
 *    elements of its chain (of its cycle, if the chain closes).  The link into word j is cut when the element is wide, or when it is
 *    eligible and its size is >= min_rows; the second case, alone or with the first, sets flag 4 on word j.
 * C. Lines: the chains of A after the cuts, indexed by their head word: frame (u, v) of the head word, S = L(head), E = R(tail),
 *    M = (S + E) * 0.5, len = (E - S) . u, h = max of lv over its words from head to tail.  The line of an isolated word is isolated.
 * D. Blocks: line t is a below candidate of line s when both are not isolated and, with x0 = (St - Ss) . us, x1 = (Et - Ss) . us,
 *    lo = min(x0, x1), hi = max(x0, x1), ov = min(hi, len_s) - max(lo, 0), a = (Mt - Ms) . vs, hmax = max(hs, ht), hmin = min(hs, ht):
 *    a > 0; ov > 0 and ov >= min_overlap * min(len_s, hi - lo); a <= block_reach * hmax; hmax <= height_ratio * hmin; us . ut >=
 *    min_cos.  Mutual nearest links give chains; a cycle is cut on the link into its smallest-index line (line flag 1).  A chain, head
 *    to tail, is a block, indexed by the head word of its head line.
 * E. Block order: a block has the frame (u, v) and the origin O = S of its head line.  Over its lines t from head to tail: X0 = min and
 *    X1 = max of (St - O) . u, (Et - O) . u (in that order per line); with m = (Mt - O) . v, Y0 = min of m - ht * 0.5 and Y1 = max of
 *    m + ht * 0.5.  Its quad is (Ox + ux * X) + vx * Y, (Oy + uy * X) + vy * Y at (X0, Y0), (X1, Y0), (X1, Y1), (X0, Y1); W = X1 - X0,
 *    H = Y1 - Y0.  The block of an isolated word is the axis-aligned bounding box of its quad (min / max over TL, TR, BR, BL) with
 *    u = (1, 0), v = (0, 1), W and H its differences.  Block X precedes Y (X != Y) when, with Y's four corners minus X's TL projected
 *    on X's u and v into [ax0, ax1] x [ay0, ay1] (min / max over TL, TR, BR, BL): ax0 >= W and min(ay1, H) - max(ay0, 0) > 0 (left
 *    of), or ay0 >= H and min(ax1, W) - max(ax0, 0) > 0 (above).  Levels start at 0; one round sets level[Y] = min(max_levels - 1,
 *    max over X that precede Y of level[X] + 1), or 0 when nothing precedes Y, reading all old values before writing any new one;
 *    max_levels - 1 rounds run (a round that changes nothing ends them: the result is the same).  The relation can hold cycles; the
 *    cap defines the result anyway.  The blocks of an image are ordered by (level, TL.y, TL.x, index), ascending.
 * Consequences (documented, not handled): a full-width heading within block_reach of the columns joins the column whose first line is
 *   nearest below it; a regular grid of words whose gaps reach min_gutter is a table and is read column by column.  Out of scope:
 *   tables, nested layouts (no recursive XY-cut), right-to-left and vertical scripts (spaces inside a polygon: ocr_break_words).
 * Oracle: tests/column_oracle.py; kernels: csrc/columns.hip (stage A is the launch of ocr_group_lines).  Blocking, on the detector's
 * stream, host pointers, and the error cases of ocr_group_lines (OCR_ERR_INVALID before any launch, the handle stays usable); zero
 * words launch nothing and return valid offsets; at most OCR_LINE_MAX_WORDS words an image. */
typedef struct ocr_column_params {
  ocr_line_params_t line;  /* line_tol, height_ratio, min_cos, max_gap as in ocr_group_lines */
  double row_gap;          /* [line.max_gap, 64], default 16   */
  double min_gutter;       /* [0, 64],            default 1.5  */
  double gutter_reach;     /* (0, 16],            default 2.5  */
  double min_overlap;      /* [0, 1],             default 0.25 */
  double block_reach;      /* (0, 16],            default 2.5  */
  int32_t min_rows;        /* [1, 4096],          default 3    */
  int32_t max_levels;      /* [1, 256],           default 64   */
  int32_t reserved[2];     /* must be 0 */
} ocr_column_params_t;
typedef struct ocr_columns {
  int32_t n_images, n_words, n_lines, n_blocks;
  const int32_t* img_offsets;    /* [n_images+1] block range per image             */
  const int32_t* block_offsets;  /* [n_blocks+1] line range per block              */
  const int32_t* line_offsets;   /* [n_lines+1]  range of `order` per line         */
  const int32_t* order;          /* [n_words]    batch-global word indices, reading order */
  const int32_t* word_flags;     /* [n_words]    by word index: 1 isolated, 2 cycle cut here, 4 a gutter in front of this word */
  const double*  gaps;           /* [n_words]    by position: g / hmax of the link into the word, 0.0 for a line's head */
  const int32_t* line_flags;     /* [n_lines]    1: a cycle of lines was cut in front of this line */
  const int32_t* block_levels;   /* [n_blocks]                                      */
  const double*  block_quads;    /* [n_blocks*8] TL, TR, BR, BL                     */
} ocr_columns_t;
void ocr_column_default_params(ocr_column_params_t* p);
/* *out: ocr_columns_free. */
int  ocr_group_columns(ocr_det_t* det, const double* quads, const int32_t* word_img_offsets, int n_images,
                       const ocr_column_params_t* params, ocr_columns_t** out);
void ocr_columns_free(ocr_columns_t* c);

/* ---------------------------------------------------------------------------
 * Detection quality metrics (host code; consumers of the polygon lists).  Replaces
 *   evaluate_image(gt, ignore_flags, pred) -> Result<MetricsItem>      metrics.rs:255-380
 *   combine_results(results) -> Result<(precision, recall, hmean)>     metrics.rs:229-253
 * (validate_measure :191-219 = drop predictions with score < 0.6, then evaluate_image per image;
 *  gather_measure :221-227 = combine_results over the concatenated items: see the host mirrors.)
 * Polygons are CSR: offsets[n+1] into x,y pairs, u32 as in MultiPolygon<u32>.
 * ------------------------------------------------------------------------- */
typedef struct ocr_metrics_item {   /* MetricsItem, metrics.rs:22-30 */
  double precision, recall, hmean;
  int32_t gt_care, det_care, det_matched;
} ocr_metrics_item_t;

int ocr_evaluate_image(const uint32_t* gt_xy, const int32_t* gt_offsets, int n_gt, const uint8_t* ignore_flags,
                       const uint32_t* pred_xy, const int32_t* pred_offsets, int n_pred, ocr_metrics_item_t* out);
int ocr_combine_results(const ocr_metrics_item_t* items, int n, double* precision, double* recall, double* hmean);

/* ---------------------------------------------------------------------------
 * Recogniser.  Replaces
 *   let net = Net::new(&weights.root()); weights.load(file)   char_recognition/mod.rs:44-46
 *   net.forward_t(&image_tensor, false)                       char_recognition/mod.rs:53-54
 *   .softmax(-1, Kind::Double); topk(&res, 1)                 mod.rs:55-56, utils.rs:28-43
 * graph: char_recognition/model.rs:13-39.
 * ------------------------------------------------------------------------- */
int ocr_rec_create(const void* weights, size_t weights_bytes, int device, ocr_rec_t** out);
/* `weights.load(file)` of char_recognition/mod.rs:46.  Net::new creates its four layers on one nn::Path
 * (model.rs:13-24), so the file holds tch's de-duplicated names weight, bias, weight__2, bias__3, ...; they are
 * mapped onto conv1 / conv2 / fc1 / fc2 by shape (all eight shapes differ).  conv1.weight ... names work too. */
int ocr_rec_create_from_varstore(const char* path, int device, ocr_rec_t** out);
void ocr_rec_destroy(ocr_rec_t* rec);
/* Same contract as ocr_det_set_stream, including the lifetime rule. */
int ocr_rec_set_stream(ocr_rec_t* rec, void* hip_stream);
/* Options, "key=value;key=value" (NULL or "" changes nothing; an unknown key is OCR_ERR_INVALID):
 *   small_batch=0|1   1 (default): batches of up to 1 024 crops take the latency-optimised kernels (see ocr_rec_forward);
 *                     0: every batch takes the throughput kernels, every multiply on the f32 matrix instructions - a
 *                     crop's logits are then bit-identical whatever the size of the batch it arrives in. */
int ocr_rec_set_options(ocr_rec_t* rec, const char* options);
int ocr_rec_synchronize(ocr_rec_t* rec);

/* forward_t: crops N x 784 (28x28, values in [0,1]) -> logits N x 62.  Blocking.
 * Batch-size invariance: batches of up to 1 024 crops and larger ones take different kernels (latency- against throughput-
 * optimised; the small-batch conv2 multiplies on the bf16 matrix cores from three-way split f32 operands).  Within a family a crop's
 * logits are bit-identical whatever batch it arrives in; across the two they agree to rounding (|dlogit| < 1e-4, |dp| < 1e-5:
 * tests/test_gpu_fullsize.py), so a crop whose two best classes tie within that margin may change label when the batch size
 * crosses 1 024 (ocr_rec_set_options "small_batch=0" removes the distinction).  The reference itself gives no stronger
 * guarantee (ATen's kernels differ with batch size too). */
int ocr_rec_forward(ocr_rec_t* rec, const float* crops, int n, float* logits, int mem_kind);
/* forward_t + softmax(-1, f64) + top-1: label index into VALUES (utils.rs:7) and
 * its probability.  logits may be NULL.  Device pointers; enqueues and returns. */
int ocr_rec_classify_async(ocr_rec_t* rec, const float* crops_dev, int n, float* logits_dev,
                           int32_t* labels_dev, double* probs_dev);
/* Per-kernel timing of one classify pass over n device-resident crops (hipEvents on the handle's stream around
 * every launch; same conventions as ocr_det_forward_profile: flops = MFMA FLOPs the launch executes). */
int ocr_rec_classify_profile(ocr_rec_t* rec, const float* crops_dev, int n, int32_t* labels_dev, double* probs_dev,
                             int max_entries, const char** names, float* ms, double* flops, double* bytes,
                             int* n_entries);
/* Blocking convenience over either memory kind. */
int ocr_rec_classify(ocr_rec_t* rec, const float* crops, int n, int32_t* labels, double* probs,
                     int mem_kind);
/* The label alphabet, utils.rs:7 ("A-Za-z0-9", 62 symbols, NUL terminated). */
const char* ocr_rec_alphabet(void);
/* EXTENSION - no counterpart in the reference (its recogniser classifies single 28 x 28 glyphs, char_recognition/model.rs:27-39):
 * CTC greedy (best-path) decode of a sequence recogniser's output, the stage BASELINE.json's north_star names.  logits N x T x C f32
 * (or any monotone transform of them), blank in [0, C): per crop the first class attaining each column's maximum, consecutive repeats
 * collapsed, blanks dropped -> labels N x T int32 (row i: lengths[i] classes, then -1) and lengths N.  One wave per crop on the handle's
 * GPU and stream; blocking; mem_kind says where the three buffers live.  Exact integers: oracle/ctc_oracle.py.
 * Defined for logits without NaN.  +-inf are ordinary values (a column of -inf decodes to class 0, +inf at several classes to the
 * lowest of them).  A crop that holds a NaN decodes to something unspecified - still lengths[i] in [0, T], that many classes of
 * [0, C), then -1 - and every other crop of the batch is unaffected.  Exactly N x T labels and N lengths are written.
 * T >= 1, C >= 1, N >= 0 (N = 0 does nothing).  OCR_ERR_INVALID for anything outside that, a blank outside [0, C), a null pointer
 * and a mem_kind other than OCR_MEM_HOST / OCR_MEM_DEVICE; nothing is written and the handle stays usable. */
int ocr_ctc_greedy_decode(ocr_rec_t* rec, const float* logits, int n, int t, int c, int blank, int mem_kind, int32_t* labels,
                          int32_t* lengths);
/* EXTENSION - no counterpart in the reference (see above): CTC prefix beam search returning the beam_width (B) most probable label
 * sequences of every crop with their log-probabilities.  logits N x T x C f32 (raw logits or log-probabilities: each column goes
 * through log-softmax first), blank in [0, C).  All arithmetic after the load is f64, with a (+) b = M + log1p(exp(m - M)) for
 * M = max, m = min (-inf (+) x = x).  Per column: lp = log-softmax; every beam (a distinct prefix l without blanks, lb / lnb = log P
 * of l ending on a blank / a non-blank, e = its last label or -1, tot = lb (+) lnb; at the start only the empty prefix, lb = 0,
 * lnb = -inf) offers its stay (lb' = tot + lp[blank], lnb' = lnb + lp[e] when e >= 0 else -inf) and, for every class c != blank, its
 * extension l + c (lnb' = (c == e ? lb : tot) + lp[c], lb' = -inf).  An extension whose prefix is already a beam is added ((+)) to
 * that beam's stay lnb' instead of standing on its own.  The first B candidates by score lb' (+) lnb' descending, ties by (beam
 * rank, class) ascending with a stay as class -1, are the next column's beams in that order.  Without pruning each score is the
 * exact CTC log P(l | x).  Out, in rank order: labels N x B x T int32 (row: lengths[] classes, then -1), lengths N x B, scores N x B
 * f64 (tot); slots beyond the distinct prefixes have length -1, score -inf, labels -1.  Limits 1 <= B <= 32, 1 <= T <= 1024,
 * 1 <= C <= 256; N = 0 does nothing.  OCR_ERR_INVALID for anything outside them, a null pointer, a mem_kind other than
 * OCR_MEM_HOST / OCR_MEM_DEVICE, and any NaN or +-inf logit (the message names the first such crop; the outputs are then unspecified,
 * the handle stays usable).  One 256-thread workgroup per crop on the handle's GPU and stream; blocking.  Oracle:
 * tests/ctc_beam_oracle.py. */
int ocr_ctc_beam_decode(ocr_rec_t* rec, const float* logits, int n, int t, int c, int blank, int beam_width, int mem_kind,
                        int32_t* labels, int32_t* lengths, double* scores);

/* EXTENSION - lexicon matching: the glyphs of a word read as a whole against a word list (BUILD-DEFINED, like the glyph, strip and
 * line rules; the reference has no counterpart).  Three steps: glyph costs from logits, a lexicon uploaded once, the match.
 *
 * Glyph costs.  logits n x 62 f32 (what ocr_rec_forward / ocr_rec_classify_async write) -> costs n x 62 f32, the negative log-softmax
 * computed in f64: for row i, m = max_c x[c], lse = m + log(sum_c exp((double)x[c] - m)) with the sum taken in class order,
 * cost[c] = (float)max(lse - (double)x[c], 0.0).  The device's f64 exp and log are within a few ulp of the correctly rounded ones, so a
 * cost is within one f32 ulp of the exact value (tests/test_gpu_lexicon.py states the bar).  A NaN or +-inf logit is OCR_ERR_INVALID
 * (the message names the first such row; the costs are then unspecified).  n = 0 does nothing.  On the handle's stream, blocking;
 * mem_kind covers both buffers.  One wave per row (csrc/lexicon.hip). */
int ocr_rec_glyph_costs(ocr_rec_t* rec, const float* logits, int n, float* costs, int mem_kind);

/* The lexicon.  Entry k is bytes[offsets[k] .. offsets[k+1]), every byte one of the alphabet (ocr_rec_alphabet), 1..OCR_LEX_MAX_LEN
 * bytes per entry, 1..OCR_LEX_MAX_ENTRIES entries, offsets [n_entries+1] starting at 0 and not decreasing; duplicates are legal.
 * Anything else is OCR_ERR_INVALID and the message names the first offending entry.  The entries are uploaded once to the recogniser's
 * GPU, sorted by (length, index) with the caller's index beside each, four class indices per 32-bit word and the words of one
 * position of all entries contiguous; results always name the caller's entry index.  The lexicon is bound to that GPU: a match
 * through a recogniser of another device is OCR_ERR_INVALID.  Destroying waits for the work queued on its GPU. */
typedef struct ocr_lexicon ocr_lexicon_t;
#define OCR_LEX_MAX_LEN 32        /* characters per entry, and glyphs per matched word */
#define OCR_LEX_MAX_ENTRIES (1 << 22)
int  ocr_lexicon_create(ocr_rec_t* rec, const char* bytes, const int32_t* offsets, int n_entries, ocr_lexicon_t** out);
int  ocr_lexicon_size(const ocr_lexicon_t* lex, int32_t* n_entries);
void ocr_lexicon_destroy(ocr_lexicon_t* lex);

/* The match.  costs n_glyphs x 62 f32 in mem_kind memory (ocr_rec_glyph_costs), word_offsets [n_words+1] in host memory (the
 * word_offsets of an ocr_glyphs_t): word w owns the glyph rows [word_offsets[w], word_offsets[w+1]).
 * Rule.  All arithmetic is f64, every operation rounded separately, adds and mins only.  For word w with glyph rows r_0..r_(G-1) and
 * entry e with classes c_0..c_(M-1):
 *   s(i, j) = (double)cost[r_i][c_j]; with fold_case = 1 the min of that and the same for the other-case twin of c_j (the twin of
 *     class c < 26 is c + 26, of 26 <= c < 52 it is c - 26, digits have none).
 *   D[0][0] = 0;  D[i][0] = D[i-1][0] + del_cost;  D[0][j] = D[0][j-1] + ins_cost;
 *   D[i][j] = min(D[i-1][j-1] + s(i-1, j-1), min(D[i-1][j] + del_cost, D[i][j-1] + ins_cost));  cost(w, e) = D[G][M]: the full table.
 *   ins_cost pays for a lexicon character with no glyph (a missed glyph), del_cost for a glyph with no lexicon character.
 * Candidates of w are the entries with |M - G| <= max_len_diff; n_candidates[w] is their number.  word_flags[w]: 1 for G = 0, 2 for
 * G > OCR_LEX_MAX_LEN - such a word has no candidates and gets no other flag -, else 4 when no entry has an admissible length.
 * Output of w: the first top_k candidates by (cost ascending, entry index ascending); slots past the candidates hold -1 and +inf.
 * The key is a total order, so the result does not depend on how the kernel chunks the list.
 * raw_costs[w] is the cost of the greedy reading: starting from 0.0, min_c (double)cost[r_i][c] added in glyph order (0.0 for a word
 * without glyphs; a word of more than 32 glyphs is summed like any other).
 * OCR_ERR_INVALID for a null pointer (params == NULL -> the defaults; costs may be NULL when n_glyphs = 0), a bad mem_kind, offsets
 * that do not start at 0, decrease or do not end at n_glyphs, a parameter out of range or a nonzero reserved field, a lexicon of
 * another device, and a cost that is NaN, +-inf or negative (found on the device in the same pass; the message names the first such
 * word).  The handle stays usable.  n_words = 0 launches nothing and returns an empty block.  The call runs on the recogniser's
 * stream behind what is queued there, and blocks.  Oracle: tests/lexicon_oracle.py; kernels: csrc/lexicon.hip (grid over word x
 * lexicon chunk, the word's cost table in LDS, one entry per lane with the DP column in registers, per-lane best-k, workgroup
 * merge, merge across chunks). */
typedef struct ocr_lexicon_params {
  double  ins_cost;      /* >= 0, finite; default 4.0: a lexicon character with no glyph (a missed glyph)  */
  double  del_cost;      /* >= 0, finite; default 4.0: a glyph with no lexicon character (a spurious glyph) */
  int32_t max_len_diff;  /* 0..8, default 2 */
  int32_t fold_case;     /* 0 | 1, default 1 */
  int32_t top_k;         /* 1..8, default 1 */
  int32_t reserved[3];   /* must be 0 */
} ocr_lexicon_params_t;
typedef struct ocr_lexicon_matches {
  int32_t n_words, top_k;
  const int32_t* entries;       /* [n_words*top_k] caller's entry index, -1 past the candidates */
  const double*  costs;         /* [n_words*top_k] +inf past the candidates                     */
  const double*  raw_costs;     /* [n_words]                                                    */
  const int32_t* n_candidates;  /* [n_words]                                                    */
  const int32_t* word_flags;    /* [n_words] 1 no glyphs, 2 more than 32 glyphs, 4 no entry of an admissible length */
} ocr_lexicon_matches_t;
void ocr_lexicon_default_params(ocr_lexicon_params_t* p);
/* *out: ocr_lexicon_matches_free. */
int  ocr_lexicon_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_glyphs, int mem_kind,
                       const int32_t* word_offsets, int n_words, const ocr_lexicon_params_t* params,
                       ocr_lexicon_matches_t** out);
void ocr_lexicon_matches_free(ocr_lexicon_matches_t* m);

/* EXTENSION - character language model: the glyphs of a word decoded as the cheapest paths through their classes under glyph cost
 * plus character-to-character transition cost (BUILD-DEFINED, like the lexicon rule; the reference has no counterpart).  It reads words
 * that no list contains and returns the k best readings with their costs.
 *
 * The model T: 64 x 64 f32, row-major, T[p*64 + c] the cost of class c behind class p.  Rows and columns 0..61 are the classes of
 * ocr_rec_alphabet, row 62 is begin-of-word, column 62 is end-of-word.  Every used value is finite and >= 0; row 63, column 63 and the
 * cell [62][62] are unused and must be 0.  Anything else is OCR_ERR_INVALID at create, and the message names the first offending cell.
 * The model is uploaded once to the recogniser's GPU and bound to it: a decode through a recogniser of another device is
 * OCR_ERR_INVALID.  Destroying waits for the work queued on its GPU. */
#define OCR_LM_MAX_LEN 32         /* glyphs per decoded word */
typedef struct ocr_char_lm ocr_char_lm_t;
int  ocr_char_lm_create(ocr_rec_t* rec, const float* trans /* 64*64 */, ocr_char_lm_t** out);
void ocr_char_lm_destroy(ocr_char_lm_t* lm);

/* The decode.  costs n_glyphs x 62 f32 in mem_kind memory (ocr_rec_glyph_costs), word_offsets [n_words+1] in host memory: word w owns
 * the glyph rows [word_offsets[w], word_offsets[w+1]).
 * Rule.  All arithmetic is f64 on the f32 values widened, every operation rounded on its own, adds and mins only.  For a word with glyph
 * rows r_0..r_(G-1), 1 <= G <= OCR_LM_MAX_LEN:
 *   D_0[c]   = T[62][c] + cost[r_0][c]
 *   D_i[c]   = min_p (D_(i-1)[p] + T[p][c])  +  cost[r_i][c]       (the transition is added first, the glyph cost second)
 *   total[c] = D_(G-1)[c] + T[c][62]
 * With top_k = K > 1 every state keeps a list: L_0[c] holds D_0[c] alone.  The candidates of state (i, c) are L_(i-1)[p][r] + T[p][c]
 * over all p < 62 and r < the length of L_(i-1)[p]; they are ordered by (value, p, r) ascending, cut to the first K, and then
 * cost[r_i][c] is added to each: that is L_i[c].  The word's outputs are the first K of L_(G-1)[c][r] + T[c][62] by (value, c, r), and
 * the classes of hypothesis k are read back along the (p, r) links.  The key is a total order, so the result does not depend on how
 * the kernel lays anything out; a rounded add is monotone, so the K costs are the K smallest path costs, each summed left to right in
 * the association above.  Since 62^G > 8 every decoded word has top_k hypotheses, and they are distinct strings.
 * Outputs: costs[w*top_k + k]; labels[k*n_glyphs + row] the class of glyph `row` in hypothesis k (-1 in the rows of words that were not
 * decoded); raw_costs[w] the model cost of the greedy reading - the first minimum class of every glyph, the same association, begin
 * and end transitions included, so costs[w*top_k] <= raw_costs[w]; word_flags[w]: 1 for G = 0 (costs +inf, raw cost 0.0), 2 for
 * G > OCR_LM_MAX_LEN (not decoded: costs +inf, labels -1; its raw cost is summed like any other word's).
 * OCR_ERR_INVALID for a null pointer (params == NULL -> the defaults; costs may be NULL when n_glyphs = 0), a bad mem_kind, offsets
 * that do not start at 0, decrease or do not end at n_glyphs, top_k out of range or a nonzero reserved field, a model of another
 * device, and a cost that is NaN, +-inf or negative (found on the device in the same pass; the message names the first such word).
 * The handle stays usable.  n_words = 0 launches nothing and returns an empty block.  The call runs on the recogniser's stream behind
 * what is queued there, and blocks.  Oracle: tests/char_lm_oracle.py; kernel: csrc/char_lm.hip (one wave per word, class c in lane
 * c, the model in LDS, the lists in registers, back-pointers in a per-call device buffer). */
typedef struct ocr_lm_params {
  int32_t top_k;         /* 1..8, default 1 */
  int32_t reserved[3];   /* must be 0 */
} ocr_lm_params_t;
typedef struct ocr_lm_paths {
  int32_t n_words, top_k, n_glyphs;
  const int32_t* labels;       /* [top_k*n_glyphs] class per hypothesis and glyph row, -1 where the word was not decoded */
  const double*  costs;        /* [n_words*top_k] ascending per word, +inf where the word was not decoded                */
  const double*  raw_costs;    /* [n_words] the greedy reading under the model                                           */
  const int32_t* word_flags;   /* [n_words] 1 no glyphs, 2 more than 32 glyphs                                           */
} ocr_lm_paths_t;
void ocr_lm_default_params(ocr_lm_params_t* p);
/* *out: ocr_lm_paths_free. */
int  ocr_lm_decode(ocr_rec_t* rec, const ocr_char_lm_t* lm, const float* costs, int n_glyphs, int mem_kind,
                   const int32_t* word_offsets, int n_words, const ocr_lm_params_t* params, ocr_lm_paths_t** out);
void ocr_lm_paths_free(ocr_lm_paths_t* p);

/* EXTENSION - segmentation lattice (BUILD-DEFINED, like the rules above; the reference has no counterpart): wide glyphs are cut into
 * pieces, every run of 1..M consecutive pieces (a span) is recognised, and glyph cost plus model cost choose the segmentation and the
 * classes together.  Three calls: ocr_split_glyphs (detector), ocr_glyph_spans (host), ocr_lattice_decode (recogniser); the chain is
 * segment -> split -> spans -> ocr_extract_glyph_crops of the span block -> ocr_rec_glyph_costs -> decode.
 *
 * 1. ocr_split_glyphs.  `glyphs` is any glyph block (column or component rule) of the same frames; *pieces is an ordinary glyph block
 * (ocr_glyphs_free, every crop call takes it), *map holds per piece the index of its source glyph in `glyphs` and its rank in it
 * (ocr_piece_map_free).  All integer.  For word k, hw = the largest y1 - y0 of its glyphs; ink is step 2 of ocr_segment_glyphs (the
 * same q) against the word's t and polarity used from word_info: polarity 1 means q <= t, 2 means q > t (a word with t = -1 has no
 * glyphs).  For glyph g with box [x0, x1) x [y0, y1), gw = x1 - x0:
 *   n = (200*gw + hw*aspect_pct) / (2*hw*aspect_pct)   (integer division: the rounded ratio gw*100 / (hw*aspect_pct)),
 *   n = max(1, min(n, max_pieces, gw / min_piece_w)).
 * n = 1: the glyph passes through as one piece, its box unchanged.  Otherwise cnt[x] = ink pixels of column x over [y0, y1),
 * r = max(1, gw / (4*n)), and for j = 1..n-1 with c_j = x0 + (j*gw)/n cut j is the column x in [max(c_j - r, x0 + 1),
 * min(c_j + r, x1 - 1)] that minimises (cnt[x], |x - c_j|, x).  Since min_piece_w >= 3 gives gw >= 3n, the windows of neighbouring
 * cuts are disjoint (c_(j+1) - c_j >= gw/n in integer division, which is >= 3 and > 2r), so the cuts increase strictly and every piece is at least one column wide.
 * Piece i covers the columns [cut_i, cut_(i+1)) with cut_0 = x0 and cut_n = x1; its x range is kept as cut, its y range is first ink
 * row .. last ink row + 1 inside those columns; a piece without an ink pixel is dropped.  If a word would hold more than max_word_pieces
 * pieces (counted after the drops), all its glyphs pass through unsplit and word_info[4k+3] gains bit 4.  Every other field of the block is copied.
 * Blocking, on the detector's stream behind what is queued there; frames in mem_kind memory, everything else host memory.
 * OCR_ERR_INVALID for a null pointer (params == NULL -> defaults), a bad mem_kind, glyphs->n_images != n, a glyph box outside its
 * frame, a word's frame index out of range, a polarity outside 1..2 or a t outside 0..254 in a word that has glyphs, offsets that do
 * not span the glyphs, a parameter out of range or a nonzero reserved field; the handle stays usable.
 * Oracle: tests/glyph_split_oracle.py; kernel: csrc/glyph_split.hip (one wave per glyph, count pass and write pass). */
typedef struct ocr_split_params {
  int32_t aspect_pct;        /* 25..400, default 100: the width of one letter in percent of the word's glyph height */
  int32_t max_pieces;        /* 1..4, default 3 (per glyph)                                                          */
  int32_t min_piece_w;       /* 3..64, default 3                                                                     */
  int32_t max_word_pieces;   /* 1..256, default 32                                                                   */
  int32_t reserved[4];       /* must be 0                                                                            */
} ocr_split_params_t;
typedef struct ocr_piece_map {
  int32_t n_pieces;
  const int32_t* glyph;      /* [n_pieces] index of the source glyph in the input block */
  const int32_t* rank;       /* [n_pieces] 0.. within that glyph, left to right (dropped pieces are not counted) */
} ocr_piece_map_t;
void ocr_split_default_params(ocr_split_params_t* p);
int  ocr_split_glyphs(ocr_det_t* det, const float* frames, int n, int h, int w, int mem_kind, const ocr_glyphs_t* glyphs,
                      const ocr_split_params_t* params, ocr_glyphs_t** pieces, ocr_piece_map_t** map);
void ocr_piece_map_free(ocr_piece_map_t* m);

/* 2. ocr_glyph_spans (host only, no device call).  For a word of G pieces the spans are [e-m, e) for e = 1..G and m = 1..min(M, e),
 * ordered by (e, m) ascending: sum_e min(M, e) per word.  A span's box is the union of its pieces' boxes.  *spans is an ordinary glyph
 * block whose word_offsets are the span ranges (word_info, word_levels and img_offsets copied), so ocr_extract_glyph_crops cuts the
 * span crops unchanged; M = 1 returns the piece block array for array.  *table (ocr_span_table_free) holds per span its word, end e
 * and length m, and the piece offsets.  OCR_ERR_INVALID: null pointer, max_span outside 1..OCR_LATTICE_MAX_SPAN, a broken block. */
#define OCR_LATTICE_MAX_SPAN 4
#define OCR_LATTICE_MAX_PIECES 32   /* pieces per decoded word */
typedef struct ocr_span_table {
  int32_t n_words, n_spans, n_pieces, max_span;
  const int32_t* span_word;      /* [n_spans] */
  const int32_t* span_end;       /* [n_spans] e, 1..G */
  const int32_t* span_len;       /* [n_spans] m, 1..min(M, e) */
  const int32_t* piece_offsets;  /* [n_words+1] the piece block's word_offsets */
} ocr_span_table_t;
int  ocr_glyph_spans(const ocr_glyphs_t* pieces, int max_span, ocr_glyphs_t** spans, ocr_span_table_t** table);
void ocr_span_table_free(ocr_span_table_t* t);

/* 3. ocr_lattice_decode.  costs: n_spans x 62 f32 in mem_kind memory (ocr_rec_glyph_costs of the span crops); span_offsets and
 * piece_offsets [n_words+1] in host memory; the model is ocr_char_lm_create's.
 * Rule.  f64 on the f32 values widened, every operation rounded on its own, adds and mins only.  Word w has G pieces,
 * 1 <= G <= OCR_LATTICE_MAX_PIECES, M = max_span, K = top_k, and row(e, m) is its span row in the order above.
 *   A_0[c] is the one-element list {T[62][c]} with link (p = 62, r = 0).
 *   A_j[c], j >= 1: the first K of L_j[p][r] + T[p][c] over p < 62 and r, by (value, p, r).
 *   L_e[c]: the first K by (value, m, a) of (A_(e-m)[c][a] + span_cost[m-1]) + cost[row(e, m)][c] over m = 1..min(M, e) and ranks a.
 *   Outputs: the first K of L_G[c][r] + T[c][62] by (value, c, r); segments and classes are read back along the links.
 * The keys are total orders, and a rounded add is monotone, so the K costs are the K smallest path costs over all (segmentation,
 * classes) pairs, each summed in the association above.  Hypotheses are distinct PAIRS: the same string may appear twice through two
 * segmentations.  span_cost[m-1] is added once per segment of m pieces: the caller's knob against the bias toward few segments.
 * With max_span = 1 and span_cost 0 the result is ocr_lm_decode's bit for bit (x + 0.0 = x for x >= 0; a sum that is -0.0 there is
 * +0.0 here).
 * Outputs: costs[w*top_k + k]; n_chars[w*top_k + k] the segments of hypothesis k (0 where not decoded); labels[k*n_pieces + piece] the
 * class at the first piece of a segment, -1 elsewhere; seg_len[k*n_pieces + piece] m at the first piece of a segment, 0 elsewhere;
 * raw_costs[w] the all-singletons path with the first-minimum class of every piece's own span row, in the same association,
 * span_cost[0] included, so costs[w*top_k] <= raw_costs[w]; word_flags[w]: 1 for G = 0 (costs +inf, raw cost 0.0), 2 for
 * G > OCR_LATTICE_MAX_PIECES (not decoded: costs +inf, labels -1; its raw cost is summed like any other word's).
 * OCR_ERR_INVALID: the cases of ocr_lm_decode (null pointer - params == NULL -> defaults, costs may be NULL when n_spans = 0 -, a bad
 * mem_kind, offsets that do not start at 0 or decrease, a model of another device, a cost that is NaN, +-inf or negative - found on
 * the device in the same pass, the message names the first such word), span offsets that are not exactly the count the rule gives
 * for (G, M) or do not end at n_spans, max_span or top_k out of range, a span_cost that is not finite and >= 0, a nonzero reserved
 * field.  The handle stays usable.  n_words = 0 launches nothing.  Runs on the recogniser's stream behind what is queued there, and
 * blocks.  Oracle: tests/lattice_oracle.py; kernel: csrc/lattice.hip (one wave per word, class c in lane c, the model in LDS, the
 * ring of the last M lists A in registers, back-pointers (m, p, r) as uint16 in a per-call device buffer). */
typedef struct ocr_lattice_params {
  int32_t max_span;      /* 1..OCR_LATTICE_MAX_SPAN, default 2 */
  int32_t top_k;         /* 1..8, default 1 */
  double  span_cost[4];  /* finite, >= 0, default 0 */
  int32_t reserved[2];   /* must be 0 */
} ocr_lattice_params_t;
typedef struct ocr_lattice_paths {
  int32_t n_words, top_k, n_pieces;
  const int32_t* labels;       /* [top_k*n_pieces] */
  const int32_t* seg_len;      /* [top_k*n_pieces] */
  const int32_t* n_chars;      /* [n_words*top_k]  */
  const double*  costs;        /* [n_words*top_k] ascending per word, +inf where the word was not decoded */
  const double*  raw_costs;    /* [n_words] */
  const int32_t* word_flags;   /* [n_words] 1 no pieces, 2 more than 32 pieces */
} ocr_lattice_paths_t;
void ocr_lattice_default_params(ocr_lattice_params_t* p);
/* *out: ocr_lattice_paths_free. */
int  ocr_lattice_decode(ocr_rec_t* rec, const ocr_char_lm_t* lm, const float* costs, int n_spans, int mem_kind,
                        const int32_t* span_offsets, const int32_t* piece_offsets, int n_words,
                        const ocr_lattice_params_t* params, ocr_lattice_paths_t** out);
void ocr_lattice_paths_free(ocr_lattice_paths_t* p);

/* 4. ocr_lexicon_lattice_match: the joint search.  The entries of a lexicon are matched over the PIECES of a word, a character
 * reading a span of 1..M pieces, so that a wrong cut is re-cut instead of paid as an insertion or a deletion (BUILD-DEFINED).
 * Inputs follow ocr_lattice_decode: costs n_spans x 62 f32 in mem_kind memory, span_offsets and piece_offsets [n_words+1] in host
 * memory, spans in the (e, m) order of ocr_glyph_spans; the lexicon is ocr_lexicon_create's, on the recogniser's device.
 * Rule.  f64 on the f32 values widened, every operation rounded on its own, adds and mins only.  Word w has G pieces,
 * 1 <= G <= OCR_LATTICE_MAX_PIECES, M = max_span; an entry has classes c_0..c_(L-1).
 *   s(row, c) = (double)cost[row][c]; with fold_case = 1 the min of that and the same for the other-case twin of c, exactly as in
 *     ocr_lexicon_match.  row(e, m) is the span row of ocr_glyph_spans.
 *   D[0][0] = 0;  D[i][0] = D[i-1][0] + del_cost;  D[0][j] = D[0][j-1] + ins_cost;
 *   D[i][j] = min( min over m = 1..min(M, i) of ((D[i-m][j-1] + span_cost[m-1]) + s(row(i, m), c_(j-1))),
 *                  min(D[i-1][j] + del_cost, D[i][j-1] + ins_cost) );                     cost(w, entry) = D[G][L].
 * A rounded add is monotone, so the cost is the minimum, over all alignment paths, of the path's sum taken left to right.
 * Candidates of w: the entries with max(1, ceil(G / M) - max_len_diff) <= L <= min(32, G + max_len_diff); n_candidates[w] is their
 * number.  Output of w: the first top_k candidates by (cost ascending, entry index ascending); slots past the candidates hold -1
 * and +inf.  word_flags[w]: 1 for G = 0, 2 for G > OCR_LATTICE_MAX_PIECES (no candidates, no other flag), else 4 when no entry has an
 * admissible length.
 * raw_costs[w]: the cheapest free segmentation with every span read as its cheapest class: F[0] = 0, F[e] = min over
 * m = 1..min(M, e) of (F[e-m] + span_cost[m-1]) + min_c (double)cost[row(e, m)][c]; raw = F[G] (0.0 for G = 0; a word of more than
 * 32 pieces is summed like any other).
 * With max_span = 1 and span_cost 0 the whole result - entries, costs, raw costs, candidates, flags - is ocr_lexicon_match's bit for
 * bit (x + 0.0 = x for x >= 0).
 * Alignment of every returned (word, rank): the table is walked back from (G, L); at cell (i, j) with value v the first step whose
 * recomputed value equals v bit for bit is taken, in the order: a segment of m = 1, 2, .., min(M, i) pieces (when j >= 1), a
 * deletion (when i >= 1), an insertion (when j >= 1).  seg_len[k*n_pieces + piece] is m at the first piece of a segment, 0 at its
 * other pieces, -1 at a deleted piece (0 in empty slots and in words without candidates); seg_char[k*n_pieces + piece] the entry
 * position j at the first piece of a segment, -1 elsewhere; n_ins[w*top_k + k] the entry characters that got no segment.
 * OCR_ERR_INVALID: a null pointer (params == NULL -> the defaults; costs may be NULL when n_spans = 0), a bad mem_kind, offsets that
 * do not start at 0 or decrease, span offsets that are not exactly sum_e min(M, e) per word or do not end at n_spans, a parameter
 * out of range or a nonzero reserved field, a lexicon of another device, a cost that is NaN, +-inf or negative (found on the device
 * in the same pass; the message names the first such word).  The handle stays usable.  n_words = 0 launches nothing.  Runs on the
 * recogniser's stream behind what is queued there, and blocks.  Oracle: tests/lexicon_lattice_oracle.py; kernels:
 * csrc/lexicon_lattice.hip (the grid, best-k and merges of the lexicon kernels; the word's span rows in LDS, the DP column in
 * registers with the last four old values beside it; one wave per returned pair recomputes the table and walks it back). */
typedef struct ocr_lexlat_params {
  double  ins_cost;      /* finite, >= 0; default 4.0: an entry character with no piece */
  double  del_cost;      /* finite, >= 0; default 4.0: a piece with no entry character  */
  double  span_cost[4];  /* finite, >= 0; default 0: added once per segment of m pieces */
  int32_t max_span;      /* 1..OCR_LATTICE_MAX_SPAN, default 2 */
  int32_t max_len_diff;  /* 0..8, default 2 */
  int32_t fold_case;     /* 0 | 1, default 1 */
  int32_t top_k;         /* 1..8, default 1 */
  int32_t reserved[2];   /* must be 0 */
} ocr_lexlat_params_t;
typedef struct ocr_lexlat_matches {
  int32_t n_words, top_k, n_pieces;
  const int32_t* entries;       /* [n_words*top_k] caller's entry index, -1 past the candidates */
  const double*  costs;         /* [n_words*top_k] +inf past the candidates                     */
  const double*  raw_costs;     /* [n_words]                                                    */
  const int32_t* n_candidates;  /* [n_words]                                                    */
  const int32_t* word_flags;    /* [n_words] 1 no pieces, 2 more than 32 pieces, 4 no entry of an admissible length */
  const int32_t* seg_len;       /* [top_k*n_pieces] */
  const int32_t* seg_char;      /* [top_k*n_pieces] */
  const int32_t* n_ins;         /* [n_words*top_k]  */
} ocr_lexlat_matches_t;
void ocr_lexlat_default_params(ocr_lexlat_params_t* p);
/* *out: ocr_lexlat_matches_free. */
int  ocr_lexicon_lattice_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_spans, int mem_kind,
                               const int32_t* span_offsets, const int32_t* piece_offsets, int n_words,
                               const ocr_lexlat_params_t* params, ocr_lexlat_matches_t** out);
void ocr_lexlat_matches_free(ocr_lexlat_matches_t* m);

/* EXTENSION - word breaks inside a polygon (BUILD-DEFINED, like the rules above; the reference has no counterpart).  A detector of
 * this family often returns one polygon for a phrase or a whole line.  ocr_break_words takes a glyph block whose words are polygons
 * and returns a glyph block whose words are the words inside those polygons, cut at the inter-word gaps, plus the map back to the
 * polygons.  Every decode call takes its word ranges as an offset array over glyphs and every crop, split and span call takes an
 * ordinary glyph block, so the chain is segment -> break -> whatever followed the segmentation before.
 * Rule.  All integer except one f64 score.  Source word k has the glyphs g0..g1-1, G = g1 - g0, with boxes (x0, y0, x1, y1) in block
 * order; no ordering of the boxes is assumed.
 *  1. G == 0: one sub-word without glyphs, rule 0, hw 0.  G > OCR_BREAK_MAX_GLYPHS: one sub-word holding every glyph, rule 0, hw 0,
 *     flag 2.  Otherwise:
 *  2. h_i = y1 - y0; hw is the element of index G / 2 (integer division) of the heights sorted ascending: the upper median.
 *  3. for i = 1..G-1: R_i = max over j < i of x1_j (a prefix maximum: component boxes may overlap or nest), gap_i = max(0, x0_i - R_i).
 *  4. fixed rule (rule 1): a break in front of glyph i iff gap_i * 100 >= space_pct * hw, in int64.
 *  5. adaptive rule (rule 2), with mode == 1 and n = G - 1 >= min_gaps: the gaps sorted ascending are s_0..s_(n-1).  For every c in
 *     1..n-1 with s_(c-1) < s_c: n0 = c, n1 = n - c, S0 and S1 the int64 sums of the two sides, d = (double)(S1*n0 - S0*n1) (the
 *     products are exact in int64), score = d*d / ((double)n0 * (double)n1), every operation separately rounded, no FMA: the Otsu
 *     form of step 3 of ocr_segment_glyphs.  The highest score wins, ties to the smaller c.  With L = s_(c-1) and T = s_c the split
 *     is accepted iff T*100 >= min_space_pct*hw and T*100 >= sep_pct*L (int64); then a break in front of glyph i iff gap_i >= T.
 *     No valid c (all gaps equal), a split that is not accepted, or too few gaps: the fixed rule decides (rule 1).  The adaptive
 *     rule is what reads letter-spaced text, whose letter gaps alone exceed any fixed share of the height.
 *  6. the sub-words are the maximal runs of glyphs between breaks, in order.  gap_pct of a sub-word is gap_i * 100 / hw at its first
 *     glyph (int64, integer division, clamped to INT32_MAX), 0 for the first sub-word of a source word: a caller tells a space from
 *     a tab by it.
 * source_info[4k..]: hw, the rule that decided (0 / 1 / 2), the threshold in pixels (rule 2: T; rule 1: the smallest gap that
 * breaks, ceil(space_pct*hw / 100); rule 0: 0), flags (2: more than OCR_BREAK_MAX_GLYPHS glyphs, not broken).
 * *words is an ordinary glyph block (ocr_glyphs_free): n_images and n_glyphs are the input's, boxes is the same array, word_offsets
 * holds the sub-word ranges, img_offsets counts sub-words, and every sub-word carries a copy of its source word's word_info and
 * word_levels; ocr_extract_glyph_crops, ocr_split_glyphs, ocr_glyph_spans and every decode call take it unchanged.  The masked crop
 * call does not: component labels are per source word, so masked crops are cut from the source block (its glyph order is the same).
 * Blocking, on the detector's stream behind everything queued there, all pointers host memory; no overlap with a pending pipelined
 * forward is promised (as ocr_group_lines).  OCR_ERR_INVALID before any launch for a null pointer (params == NULL -> the defaults),
 * offsets that do not start at 0, decrease or do not span the glyphs (or the words), a box with x1 <= x0 or y1 <= y0, a coordinate
 * outside 0..2^22, a parameter out of range or a nonzero reserved field; the handle stays usable.  A block without glyphs launches
 * nothing and returns valid blocks.
 * Out of scope: one threshold per polygon with no line-level context, so a single letter-spaced word whose gaps are all equal and
 * wide breaks at every letter (ocr_lexicon_phrase_match below puts such a word back together from the lexicon).
 * Oracle: tests/word_break_oracle.py; kernel: csrc/word_breaks.hip (one wave per source word, glyph i in lane i % 64, slot i / 64;
 * both sorts by rank counting over an LDS copy of the wave's keys). */
#define OCR_BREAK_MAX_GLYPHS 256
typedef struct ocr_break_params {
  int32_t mode;           /* 0 fixed, 1 adaptive with the fixed rule behind it (default) */
  int32_t space_pct;      /* 1..1000, default 35  */
  int32_t min_space_pct;  /* 1..1000, default 25  */
  int32_t sep_pct;        /* 100..1000, default 200 */
  int32_t min_gaps;       /* 3..255, default 3    */
  int32_t reserved[3];    /* must be 0 */
} ocr_break_params_t;
typedef struct ocr_word_breaks {
  int32_t n_source, n_words;
  const int32_t* source;       /* [n_words]     source word of every sub-word              */
  const int32_t* sub_offsets;  /* [n_source+1]  sub-word range per source word (>= 1 each) */
  const int32_t* gap_pct;      /* [n_words]                                                */
  const int32_t* source_info;  /* [4*n_source]  hw, rule 0/1/2, threshold in pixels, flags */
} ocr_word_breaks_t;
void ocr_break_default_params(ocr_break_params_t* p);
/* *words: ocr_glyphs_free; *breaks: ocr_word_breaks_free. */
int  ocr_break_words(ocr_det_t* det, const ocr_glyphs_t* glyphs, const ocr_break_params_t* params,
                     ocr_glyphs_t** words, ocr_word_breaks_t** breaks);
void ocr_word_breaks_free(ocr_word_breaks_t* b);

/* EXTENSION - phrase search: the glyphs of a line segmented into lexicon words (BUILD-DEFINED, like the rules above; the reference
 * has no counterpart).  ocr_break_words cuts a polygon from its gaps alone, before any character is looked at, and an entry of
 * ocr_lexicon_match reads one sub-word.  ocr_lexicon_phrase_match is dictionary word segmentation: one DP over the glyphs of a line
 * picks the word boundaries and the lexicon entries together, gap evidence enters as a soft cost per glyph, and an out-of-vocabulary
 * word costs something without making the line unreadable.
 * costs n_glyphs x 62 f32 in mem_kind memory (ocr_rec_glyph_costs), line_offsets [n_lines+1] in host memory: line l owns the glyph
 * rows [line_offsets[l], line_offsets[l+1]).  bound_cost and join_cost [n_glyphs] f32 in host memory, or both NULL for zeros:
 * bound_cost[r] is paid when a word starts at glyph row r inside a line, join_cost[r] when r continues the word of the row before it
 * (capi.phrase_gap_costs derives both from the result of ocr_break_words).
 * Rule.  All arithmetic is f64 on the f32 values widened, every operation rounded separately, adds and mins only.  Line l has the glyph
 * rows r_0..r_(G-1), 1 <= G <= OCR_PHRASE_MAX_GLYPHS.
 *   s(i, c) is ocr_lexicon_match's: (double)cost[r_i][c], with fold_case = 1 the min of that and the same for the other-case twin.
 *   raw(i) = min over c of (double)cost[r_i][c].
 *   W(i, e), entry e with classes c_0..c_(M-1) at start i, i + M <= G: start at 0.0 and add s(i+k, c_k) in k order.  No insertions or
 *     deletions inside the phrase search.
 *   L(i, M) = the minimum of W(i, e) over the entries of length M by (value, entry index) ascending; +inf / -1 without such an entry.
 *   U(i, M), an out-of-vocabulary word: start at oov_word_cost; for k = 0..M-1 add raw(i+k), then add oov_glyph_cost.
 *   J(i, M), the interior joins: start at 0.0 and add (double)join_cost[r_(i+k)] for k = 1..M-1 in order.
 *   T(i, M, 0) = (L(i, M) + word_cost) + J(i, M);  T(i, M, 1) = U(i, M) + J(i, M);  1 <= M <= min(OCR_LEX_MAX_LEN, G - i).
 *   B[0] = 0.0.  For j = 1..G the candidates (M, kind) have v = (B[j-M] + bnd(j-M)) + T(j-M, M, kind), bnd(0) = 0.0 and
 *     bnd(i) = (double)bound_cost[r_i] for i > 0; B[j] is the minimum by (v, kind, M) ascending: on a tie the lexicon comes before
 *     out-of-vocabulary, then the shorter word.  An infinite v never wins; U is finite, so there is always a finite candidate.
 *   The words of the line are read back from G along the chosen (M, kind) and come out in glyph order, with the entry of L for kind 0.
 * The key is a total order, so the result does not depend on how a kernel chunks the lexicon or the line.
 * Output: line_word_offsets [n_lines+1] the word range of every line (at least one word each), word_offsets [n_words+1] the glyph rows
 * of every word - an ordinary offset array, a tiling of all glyph rows, that ocr_lm_decode and ocr_lexicon_match take -, entries
 * [n_words] (the caller's index, -1 for an out-of-vocabulary word), word_costs [n_words] the T of the chosen segment, line_costs
 * [n_lines] B[G], raw_costs [n_lines] the greedy sum exactly as ocr_lexicon_match's raw_costs, line_flags [n_lines].
 * Flagged lines keep the tiling: G = 0 gives one word without glyphs, entry -1, word cost 0.0, line cost 0.0, flag 1; G >
 * OCR_PHRASE_MAX_GLYPHS gives one word holding every glyph, entry -1, both costs +inf, flag 2.
 * OCR_ERR_INVALID for a null pointer (params == NULL -> the defaults; costs may be NULL when n_glyphs = 0), a bad mem_kind, offsets
 * that do not start at 0, decrease or do not end at n_glyphs, a parameter out of range or a nonzero reserved field, a lexicon of
 * another device, exactly one of bound_cost / join_cost NULL, a value in them that is NaN, +-inf or negative, and a glyph cost that is
 * NaN, +-inf or negative (found on the device in the same pass; the message names the first such line).  The handle stays usable.
 * n_lines = 0 launches nothing and returns an empty block.  The call runs on the recogniser's stream behind what is queued there, and
 * blocks.  Lines are processed in groups of at most 2 048 windows of 32 starts, so the call's workspace beyond the copies of its own
 * arguments and results (costs 248 B, gap costs and results 40 B a glyph) stays under 96 MiB whatever the batch and the lexicon: 48 MiB of
 * per-chunk minima (at most 64 chunks) and 40 MiB of segment costs and entries.
 * Out of scope: insertions or deletions inside a phrase word (ocr_lexicon_match's edit distance reads one word); k-best phrases (one
 * best segmentation); a model transition across words; lattice pieces; lines of more than OCR_PHRASE_MAX_GLYPHS glyphs (flagged).
 * Oracle: tests/phrase_oracle.py; kernels: csrc/lexicon_phrase.hip (the match: grid over window of 32 starts x lexicon chunk of one
 * length, the window's cost rows in LDS, one entry per lane with 32 accumulators, butterflies by (cost, index); the segment costs: one
 * thread per (start, length); the DP: one wave per line, lane = kind * 32 + (M - 1)). */
#define OCR_PHRASE_MAX_GLYPHS 256     /* glyphs per line; OCR_BREAK_MAX_GLYPHS */
typedef struct ocr_phrase_params {
  double  word_cost;       /* >= 0 finite, default 1.0: paid once per lexicon word (keeps "int he box" behind "in the box") */
  double  oov_word_cost;   /* >= 0 finite, default 6.0: paid once per out-of-vocabulary word   */
  double  oov_glyph_cost;  /* >= 0 finite, default 1.0: paid per glyph of such a word           */
  int32_t fold_case;       /* 0 | 1, default 1: s(i, c) exactly as in ocr_lexicon_match         */
  int32_t reserved[3];     /* must be 0 */
} ocr_phrase_params_t;
typedef struct ocr_phrase_matches {
  int32_t n_lines, n_words, n_glyphs;
  const int32_t* line_word_offsets; /* [n_lines+1] word range of every line (>= 1 word each)             */
  const int32_t* word_offsets;      /* [n_words+1] glyph rows of every word: an ordinary offset array     */
  const int32_t* entries;           /* [n_words] caller's entry index, -1 for an out-of-vocabulary word   */
  const double*  word_costs;        /* [n_words] T of the chosen segment                                  */
  const double*  line_costs;        /* [n_lines] B[G]                                                     */
  const double*  raw_costs;         /* [n_lines] the greedy sum, as ocr_lexicon_match's raw_costs         */
  const int32_t* line_flags;        /* [n_lines] 1 no glyphs, 2 more than OCR_PHRASE_MAX_GLYPHS           */
} ocr_phrase_matches_t;
void ocr_phrase_default_params(ocr_phrase_params_t* p);
/* *out: ocr_phrase_matches_free. */
int  ocr_lexicon_phrase_match(ocr_rec_t* rec, const ocr_lexicon_t* lex, const float* costs, int n_glyphs, int mem_kind,
                              const int32_t* line_offsets, int n_lines, const float* bound_cost, const float* join_cost,
                              const ocr_phrase_params_t* params, ocr_phrase_matches_t** out);
void ocr_phrase_matches_free(ocr_phrase_matches_t* m);

/* ---------------------------------------------------------------------------
 * Multi-GPU exchange.  Frames and crops are independent (eval-mode batch norm), so a batch shards over the GPUs of
 * a node with no data-path collective: one process (or thread) per GPU, each with its own detector / recogniser
 * handle and its own contiguous slice of the batch.  The single exchange step is the all-gather of the results,
 * over RCCL (xGMI inside a node).  The reference has no counterpart (it is single-device); a Rust
 * host binds these four calls next to the others.
 *   rank 0: ocr_comm_unique_id(id) and hand the 128 bytes to the other ranks (file, environment, launcher ...);
 *   every rank: ocr_comm_create(id, world, rank, device, &comm)      - collective
 *               ocr_comm_all_gather_polygons(comm, mine, &all)       - collective; `all` holds the frames of rank 0,
 *                                                                      then rank 1, ...; free with ocr_polygons_free
 * RCCL is loaded on first use (librccl.so.1); without it these calls fail with a message, nothing else is affected.
 * ------------------------------------------------------------------------- */
typedef struct ocr_comm ocr_comm_t;
#define OCR_COMM_ID_BYTES 128
int ocr_comm_unique_id(uint8_t* id /* [OCR_COMM_ID_BYTES] */);
int ocr_comm_rccl_version(int* version);
int ocr_comm_create(const uint8_t* id, int world, int rank, int device, ocr_comm_t** out);
void ocr_comm_destroy(ocr_comm_t* comm);
int ocr_comm_all_gather_polygons(ocr_comm_t* comm, const ocr_polygons_t* local, ocr_polygons_t** all);
/* labels of the local crops (host memory) -> labels of every rank's crops in rank order; counts[world] receives
 * the number each rank contributed (may be NULL); fails if more than `capacity` labels arrive. */
int ocr_comm_all_gather_labels(ocr_comm_t* comm, const int32_t* labels, int n_local, int32_t* all, int capacity,
                               int32_t* counts, int* n_all);

#ifdef __cplusplus
}
#endif
#endif /* OCR_AMD_H */
