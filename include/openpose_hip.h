/*
 * openpose_hip.h — C ABI of the MI355X (gfx950) OpenPose inference path.
 *
 * Drop-in replacement for the hot path of nk35jk/Chainer_Realtime_Multi-Person_Pose_Estimation:
 * PoseDetector.__call__ (pose_detector.py:484-517) = CocoPoseNet forward
 * (models/CocoPoseNet.py:132-262) + PAF post-process (pose_detector.py:75-265).
 * The reference has no FFI of its own (pure Python); every entry point below names the
 * reference function it replaces.  The Python host package
 * (chainer_realtime_multi-person_pose_estimation_amd/) binds these with ctypes.
 *
 * Conventions: plain pointers + sizes; all host pointers, row-major, C-contiguous.
 * Every function returns an int status (OP_OK = 0); op_last_error() describes the last failure
 * on the calling thread.  A context is single-threaded and owns one HIP stream on one device.
 *
 * The training ABI grew by four calls (op_train_eval, op_train_eval_poses, op_train_get_state,
 * op_train_set_state: validation passes and snapshot / resume); nothing existing changed.  This
 * header is part of the digest op_build_info reports, so a library built before them reports
 * another digest.
 */
#ifndef OPENPOSE_HIP_H
#define OPENPOSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OP_OK 0
#define OP_ERR_INVALID 1  /* bad argument / shape */
#define OP_ERR_HIP 2      /* HIP runtime failure */
#define OP_ERR_CAPACITY 3 /* a per-frame cap (peaks/persons) was exceeded */
#define OP_ERR_INDEX 4    /* reference raises IndexError (pose_detector.py:197): a connection hit >=3 subsets */
#define OP_ERR_STATE 5    /* weights not set / no staged frames */
#define OP_ERR_TIMEOUT 6  /* a multi-GPU gather did not complete in time (a rank stalled or died) */

#define OP_N_JOINTS 18 /* JointType, entity.py:9-46 */
#define OP_N_LIMBS 19  /* params['limbs_point'], entity.py:85-105 */
#define OP_N_PAF 38
#define OP_N_HEAT 19
#define OP_N_LAYERS 92 /* models/CocoPoseNet.py:26-129 */
#define OP_MAX_SCALES 8 /* inference_scales entries (entity.py:74) */

/* Inference parameters — entity.py:70-105 (same names and meaning). */
typedef struct op_params {
  int32_t inference_img_size;   /* 368 */
  int32_t heatmap_size;         /* 320 */
  double gaussian_sigma;        /* 2.5 (scipy gaussian_filter, truncate 4.0) */
  int32_t n_integ_points;       /* 10 */
  int32_t n_integ_points_thresh;/* 8 */
  double heatmap_peak_thresh;   /* 0.05 */
  double inner_product_thresh;  /* 0.05 */
  double limb_length_ratio;     /* 1.0 */
  double length_penalty_value;  /* 1 */
  int32_t n_subset_limbs_thresh;/* 3 */
  double subset_score_thresh;   /* 0.2 */
  int32_t limbs_point[OP_N_LIMBS][2];
  int32_t downscale;            /* 8 */
  int32_t n_scales;             /* len(inference_scales) = 4 (detect_precise) */
  double inference_scales[OP_MAX_SCALES]; /* [0.5, 1, 1.5, 2] */
} op_params;

/* Capacities of a context (device buffers are sized from these; 0 = default). */
typedef struct op_limits {
  int32_t max_batch;           /* frames per run (default 1) */
  int32_t max_net_h, max_net_w;/* largest network input, multiples of 8 (default 368 x 656) */
  int32_t max_map_h, max_map_w;/* largest post-process map (default 320 x 576) */
  int32_t max_peaks_per_joint; /* default 512 */
  int32_t max_frame_h, max_frame_w; /* largest raw BGR frame for the staged path (default 720 x 1280) */
} op_limits;

/* Per-frame result header.  status is the frame's OP_* code. */
typedef struct op_frame_result {
  int32_t status;
  int32_t n_peaks;   /* len(all_peaks) */
  int32_t n_persons; /* len(subsets) after the keep filter (pose_detector.py:248) */
  int32_t map_w, map_h;
  int32_t net_w, net_h;
} op_frame_result;

typedef struct op_ctx op_ctx;

const char* op_last_error(void);

/* Provenance of the loaded binary (no reference counterpart): writes "sha256:<64 hex>;defs=<flags>"
 * + NUL into out (OP_ERR_INVALID when cap is too small), the digest of the library's sources as
 * built -- sha256 of the `sha256sum` listing of csrc/ *.hip *.hpp *.cpp, csrc/Makefile and
 * include/ *.h (paths relative to csrc/, sorted), computed by the Makefile at build time;
 * _lib.source_digest() recomputes it from the tree -- and the build flags beyond the Makefile's own
 * (DEFS, FLAGS_* overrides; empty for the product library). */
int op_build_info(char* out, int32_t cap);
int op_default_params(op_params* p);
int op_default_limits(op_limits* l);

/* Layer table of models/CocoPoseNet.py:26-129 (name, Ci, Co, ksize) in declaration order. */
int op_layer_info(int index, const char** name, int32_t* ci, int32_t* co, int32_t* ksize);

/* PoseDetector.__init__ (pose_detector.py:16-35): context on HIP device `device`. */
int op_create(const op_params* params, const op_limits* limits, int device, op_ctx** out);
int op_destroy(op_ctx* ctx);

/* Arithmetic of the forward convolutions.  OP_PRECISION_BF16X3 (default): every f32 operand is
 * split into bf16 hi + lo and each product formed as hi*hi + hi*lo + lo*hi on the bf16 matrix
 * cores with f32 accumulation (~16-bit products, 5.3x the f32-MFMA rate; |err| ~3e-5 on the maps,
 * inside the 1e-3 parity tolerance).  OP_PRECISION_FP32: exact f32 products (v_mfma_f32_32x32x2_f32). */
#define OP_PRECISION_FP32 0
#define OP_PRECISION_BF16X3 1
int op_set_precision(op_ctx* ctx, int32_t mode);
int op_get_precision(op_ctx* ctx, int32_t* mode);

/* Kernel family of the bf16x3 convolutions (a tuning knob; every family computes the same
 * products, parity-tested): 4 (default): large 3x3 launches (>= 1024 workgroups) take the
 * register-weight kernel with a double-buffered halo, conv_m16r, which sums in exactly the order of
 * conv_m16k below, so results are bit-identical to 5; 5 = 4 without it: shared-weight halo tiles
 * (conv_big.hip): the 7x7 layers
 * on v_mfma_f32_16x16x32_bf16 tap pairs over raster tiles (640-pixel ranges of the batch that
 * span frame borders), the 3x3 layers on 16x16x32 with K = 32 input channels over 8 x 32 / 4 x 48
 * tiles (32x32x16 kernel for the 64-channel ones), the 1x1 layers on co-split halo tiles;
 * 3 co-split halo tiles for every layer (conv_halo.hip); 0 the per-tap gather kernel.  Shapes a
 * family does not take use the gather kernel.  (Round-1 experiment families -- double-buffered
 * halos, rectangular 7x7 tap pairs, register weights -- live in git history: tools/build_rev.sh
 * builds that revision as an A/B variant.) */
int op_set_conv_algo(op_ctx* ctx, int32_t algo);
/* Layout of the 7x7 stage tensors of stages 2-6 (default 1; env OP_STAGE_PLANAR=0 sets new
 * contexts to 0).  1: chunk-planar ([16-channel chunk][hi/lo plane][row][col] per frame) wherever
 * the 7x7 kernel conv_m16 takes every 7x7 launch of the geometry -- its halo loads are then
 * contiguous runs (about half the HBM reads); 0: [row][col][channels].  Same kernels, same
 * arithmetic and order: the maps are bit-identical either way.  No reference counterpart (the
 * reference's tensors live in Chainer/cuDNN). */
int op_set_stage_layout(op_ctx* ctx, int32_t planar);
/* Batch invariance (default off).  A launch that fills few CUs (one frame, one crop) splits the
 * 7x7 convolutions' input channels over several workgroups and sums their f32 partials, so a
 * frame's maps then differ from the same frame inside a larger batch by f32 re-association (~1e-5;
 * near-threshold peaks of noisy maps can flip).  enable != 0 keeps one accumulation order for
 * every batch size (single-frame latency ~2x). */
int op_set_batch_invariant(op_ctx* ctx, int32_t enable);
/* Peak semantics of the single-scale post-process (op_detect, op_postprocess, op_run_staged*).
 * The reference's compute_peaks_from_heatmaps has two branches and takes the one of the array it
 * is handed: the CPU branch (pose_detector.py:82-110: scipy gaussian_filter sigma 2.5, reflect
 * boundary, normalised 21 taps; strict > 4-neighbour NMS) for a CPU detector, the GPU branch
 * (:111-132: F.convolution_2d with the ksize x ksize kernel of create_gaussian_kernel :38-44 --
 * exp(-d^2 / 2 sigma^2) / (2 pi sigma^2), not normalised -- zero padding ksize/2; >= NMS) in
 * __call__ of a detector built with device >= 0 (:29-35, :496-508).  OP_PEAKS_CPU_BRANCH (0, the
 * default and the parity target of the golden fixtures) or OP_PEAKS_GPU_BRANCH (1; ksize odd,
 * 3 .. 33, entity.py's 'ksize' is 17).  op_detect_precise and op_compute_peaks keep the CPU branch in
 * either mode, as the reference does: their heatmaps are NumPy arrays there (:470-475). */
#define OP_PEAKS_CPU_BRANCH 0
#define OP_PEAKS_GPU_BRANCH 1
int op_set_peak_mode(op_ctx* ctx, int32_t mode, int32_t ksize);

/* serializers.load_npz(weights_file, model) (pose_detector.py:26): 92 layers in op_layer_info
 * order, W as Chainer (Co, Ci, k, k) f32 and b as (Co,) f32.  Packed into the kernel layout
 * and uploaded once. */
int op_set_weights(op_ctx* ctx, const float* const* W, const float* const* b);

/* PoseDetector.__call__ (pose_detector.py:484-517), single scale.  bgr: h x w x 3 uint8,
 * row_stride bytes per row.  poses: cap x 18 x 3 f64, scores: cap f64. */
int op_detect(op_ctx* ctx, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride,
              double* poses, double* scores, int32_t cap, op_frame_result* res);

/* PoseDetector.detect_precise (pose_detector.py:433-482), the multi-scale mode (precise=True):
 * per scale of params.inference_scales a cv2.resize(INTER_CUBIC) of the frame to
 * ceil(w*m) x ceil(h*m), m = scale * inference_img_size / min(h, w), pad_image to a multiple of
 * `downscale` with BGR (104, 117, 123), the forward, cubic resizes of the last-stage maps to the
 * padded size, crop, cubic resize to h x w; the maps are averaged over the scales and
 * post-processed at the original resolution (img_len = w, no rescale).  pafs_out (38, h, w) and
 * heat_out (19, h, w) f32 receive the averaged maps (the reference's self.pafs / self.heatmaps)
 * when non-null. */
int op_detect_precise(op_ctx* ctx, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride,
                      double* poses, double* scores, int32_t cap, op_frame_result* res,
                      float* pafs_out, float* heat_out);

/* ---- Stage entry points (same semantics as the named reference code; used by the parity tests) ---- */

/* cv2.resize(src, (out_w, out_h), interpolation=cv2.INTER_CUBIC) (pose_detector.py:443, 461-467):
 * src h x w x cn, dtype 0 = uint8, 1 = float32; dst out_h x out_w x cn of the same dtype. */
int op_resize_cubic(op_ctx* ctx, const void* src, int32_t dtype, int32_t h, int32_t w, int32_t cn, void* dst,
                    int32_t out_h, int32_t out_w);

/* cv2.resize(orig_img, (out_w, out_h)) + preprocess (pose_detector.py:493-494, 426-431):
 * x_out (1, 3, out_h, out_w) f32 = u8/255 - 0.5, BGR order kept. */
int op_preprocess(op_ctx* ctx, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride,
                  int32_t out_w, int32_t out_h, float* x_out);

/* CocoPoseNet.__call__ (models/CocoPoseNet.py:132-262): x (n, 3, h, w) f32 -> last-stage
 * pafs (n, 38, h/8, w/8) and heatmaps (n, 19, h/8, w/8).  h, w multiples of 8. */
int op_forward(op_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, float* pafs, float* heatmaps);

/* As op_forward, but every stage's outputs: the (pafs, heatmaps) lists CocoPoseNet.__call__ returns
 * (models/CocoPoseNet.py:164-165, 180-181, ..., 262).  pafs (6, n, 38, h/8, w/8), heatmaps
 * (6, n, 19, h/8, w/8); stage s at index s-1. */
int op_forward_stages(op_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, float* pafs, float* heatmaps);

/* Test aid (no reference counterpart): the forward of op_forward, stopped right after probe point
 * `point`, and the tensor that point wrote returned as dense f32 (nframes, channels, h/divisor,
 * w/divisor) for frames [frame0, frame0 + nframes) of the batch; split-stored (bf16x3) values come
 * back as hi + lo.  Probe points are the launch boundaries of the forward in execution order; a
 * fused step that runs as separate launches (other conv algos, fp32, OP_HEAD_FUSED=0) is still one
 * point, after the last of them:
 *   0 the network input as stored; 1 conv1_1+conv1_2+pool; 2 conv2_1; 3 conv2_2+pool; 4-6 conv3_1 ..
 *   conv3_3; 7 conv3_4+pool; 8-10 conv4_1, conv4_2, conv4_3_CPM; 11 conv4_4_CPM; 12-14 conv5_1 ..
 *   conv5_3 (L1 | L2, 256 channels); 15 the stage-1 heads; then for stage s = 2 .. 6 at
 *   16 + 6 (s - 2) + i: i = 0 .. 4 Mconv1 .. Mconv5 (L1 | L2), i = 5 the heads (Mconv6+Mconv7).
 * The map points (15, 21, ..., 45) return 185 channels in the order of the reference's F.concat
 * (models/CocoPoseNet.py:168): paf 38, heat 19, feature 128, read from the buffer the next stage's
 * Mconv1 reads.  out_floats must equal nframes * channels * (h/divisor) * (w/divisor); a bad point,
 * frame range or out_floats is OP_ERR_INVALID before anything is launched.  The default forward is
 * unchanged: no other entry point stops early.
 * op_forward_probe_info: a point's name, channel count and size divisor (46 points, 0 .. 45). */
int op_forward_probe_info(int32_t point, const char** name, int32_t* channels, int32_t* divisor);
int op_forward_probe(op_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, int32_t point, int32_t frame0,
                     int32_t nframes, float* out, int64_t out_floats);

/* F.resize_images (pose_detector.py:501-502; Chainer <= 6 align-corners bilinear): (c,h,w) -> (c,oh,ow). */
int op_resize_images(op_ctx* ctx, const float* x, int32_t c, int32_t h, int32_t w, int32_t oh, int32_t ow, float* y);

/* Capacities.  Like the reference (pose_detector.py:75-250 has no caps) the post-process is
 * uncapped: a frame with more peaks per joint than op_limits.max_peaks_per_joint, or more subsets
 * than the batched grouping holds, is re-run alone with buffers sized from its own counts (only
 * device memory bounds it).  OP_ERR_CAPACITY then means either that device memory ran out, or
 * that the caller's output array is too small -- in which case the needed row count is written
 * to the count output (*n_peaks, conn_off[19], *n_subsets, res->n_persons) so the call can be
 * repeated with a larger array. */

/* compute_peaks_from_heatmaps (pose_detector.py:75-110, CPU semantics): heatmaps (c, h, w),
 * channel c-1 dropped.  peaks: rows [joint, x, y, score, id] f64. */
int op_compute_peaks(op_ctx* ctx, const float* heatmaps, int32_t c, int32_t h, int32_t w,
                     double* peaks, int64_t cap, int64_t* n_peaks);

/* compute_connections (pose_detector.py:161-181, with compute_candidate_connections :135-159):
 * pafs (38, h, w) at map resolution, peaks (n, 5).  conn rows [id_a, id_b, score]; limb l's rows
 * are conn[conn_off[l] .. conn_off[l+1]). */
int op_compute_connections(op_ctx* ctx, const float* pafs, int32_t h, int32_t w, const double* peaks,
                           int64_t n_peaks, double img_len, double* conn, int64_t cap, int64_t* conn_off);

/* grouping_key_points (pose_detector.py:183-250): subsets (S, 20) f64 after the keep filter. */
int op_grouping(op_ctx* ctx, const double* conn, const int64_t* conn_off, const double* peaks,
                int64_t n_peaks, double* subsets, int64_t cap, int64_t* n_subsets);

/* pose_detector.py:501-517 from the last-stage network maps (38,h,w) + (19,h,w) of one frame;
 * the image was orig_h x orig_w. */
int op_postprocess(op_ctx* ctx, const float* paf_low, const float* heat_low, int32_t h, int32_t w,
                   int32_t orig_h, int32_t orig_w, double* poses, double* scores, int32_t cap,
                   op_frame_result* res);

/* ---- Device-resident batched path (frame-parallel serving / bench) ---- */

/* Copy n BGR frames (n x h x w x 3 u8, contiguous) into the context's HBM staging area. */
int op_stage_frames(op_ctx* ctx, const uint8_t* frames, int32_t n, int32_t h, int32_t w);
/* Asynchronous staging for a frame stream: copy n BGR frames (n x h x w x 3 u8, contiguous;
 * page-locked memory from op_host_alloc makes the copy truly asynchronous) on the context's copy
 * stream into a 2-slot device ring and return.  The next op_run_staged* waits for that copy on the
 * compute stream and makes these frames the staged set, so the upload of step k+1 overlaps the
 * compute of step k (the reference uploads each frame inside __call__, pose_detector.py:496-497).
 * The copy may still be reading the host buffer after op_upload_frames and the consuming
 * op_run_staged* have returned: the buffer must stay unchanged until the copy has completed --
 * after op_upload_wait, op_synchronize, or any later call that waited for the consuming run. */
int op_upload_frames(op_ctx* ctx, const uint8_t* frames, int32_t n, int32_t h, int32_t w);
/* Block until every op_upload_frames copy issued so far has finished reading its host buffer (the
 * buffers may then be refilled).  No reference counterpart (the reference's uploads are
 * synchronous, pose_detector.py:496-497). */
int op_upload_wait(op_ctx* ctx);
/* Page-locked host memory for op_upload_frames sources. */
int op_host_alloc(size_t bytes, void** p);
int op_host_free(void* p);
/* Optional: post-process these maps (n x 57 x mh x mw: 38 PAF then 19 heat) instead of the network's
 * own (synthetic-map benchmarking; default off; op_use_staged_maps).  mh x mw = the network map size
 * (h/8 x w/8 of the network input) feeds op_run_staged; mh x mw = the staged frame size (stage the
 * frames first) feeds op_run_staged_precise's full-resolution post-process in place of the averaged
 * maps, which are still computed. */
int op_stage_maps(op_ctx* ctx, const float* maps, int32_t n, int32_t mh, int32_t mw);
int op_use_staged_maps(op_ctx* ctx, int32_t enable);
/* Enqueue the full path (resize+normalise, 92 convs, post-process) on the staged frames; async. */
int op_run_staged(op_ctx* ctx);
/* detect_precise (pose_detector.py:433-482) on every staged frame: per inference scale one batched
 * forward of all staged frames, per-frame cubic map resizes into the running mean, then the
 * full-resolution post-process; results via op_fetch_result(s) as for op_run_staged (map_w/h = the
 * frame size, net_w/h = the largest scale's network input).  Synchronous on the context stream. */
int op_run_staged_precise(op_ctx* ctx);
/* Capture op_run_staged as a hipGraph and replay it (same semantics, fewer launches). */
int op_run_staged_graph(op_ctx* ctx);
/* Contents of the step graph op_run_staged_graph captured last (debugging / regression aid; no
 * reference counterpart): node counts by kind.  host_nodes = memcpy nodes with a host-memory source
 * or destination, and host / event / other nodes -- none may exist: the step graph touches device
 * memory only (uploads and result fetches stay outside it, on their own streams / calls).
 * OP_ERR_STATE when no graph has been captured. */
int op_graph_info(op_ctx* ctx, int32_t* nodes, int32_t* kernels, int32_t* memsets, int32_t* memcpys,
                  int32_t* host_nodes);
int op_synchronize(op_ctx* ctx);
/* Results of staged frame i (after op_synchronize). */
int op_fetch_result(op_ctx* ctx, int32_t frame, double* poses, double* scores, int32_t cap, op_frame_result* res);

/* Results of staged frames [first, first+n) in three copies: poses (n x cap x 18 x 3 f64),
 * scores (n x cap f64), res (n headers).  A frame's status is in its header; the call itself
 * fails only on bad arguments / HIP errors or when a frame's person count exceeds cap. */
int op_fetch_results(op_ctx* ctx, int32_t first, int32_t n, double* poses, double* scores, int32_t cap,
                     op_frame_result* res);

/* Network maps of staged frames [first, first+n) after op_synchronize: the last-stage maps of
 * op_run_staged (pafs (n, 38, h/8, w/8), heatmaps (n, 19, h/8, w/8) of the network input h x w), or
 * after op_run_staged_precise the averaged full-resolution maps (n, 38|19, H, W) -- the
 * self.pafs / self.heatmaps detect_precise leaves (pose_detector.py:469-470).  *mh, *mw receive the
 * map size; pafs = heatmaps = NULL only queries it. */
int op_fetch_maps(op_ctx* ctx, int32_t first, int32_t n, float* pafs, float* heatmaps, int32_t* mh, int32_t* mw);
/* HIP-event timing of the last op_run_staged: ms spent in the conv kernels, the post-process kernels
 * and total, recorded on the context stream. */
int op_last_timing(op_ctx* ctx, double* conv_ms, double* post_ms, double* total_ms);
/* Per-kernel-class HIP-event timing of the launches enqueued by op_run_staged while enabled
 * (event pairs on the context stream around every launch of the class).  Classes:
 * 0 = 7x7 stage convs (the dominant kernel), 1 = 3x3 convs, 2 = 1x1 convs, 3 = post-process
 * (peaks, line integrals, greedy, grouping; single scale and detect_precise's full resolution),
 * 4 = frame input (resize + pad + normalise kernels not fused into a conv), 5 = map resizes
 * (detect_precise's cubic resizes of the last-stage maps and their scale mean), 6 = other (pools,
 * layout copies, result packing).  op_profile_read resolves pending pairs (after op_synchronize) and returns the totals since the
 * last reset: summed ms, launch count, algorithmic FLOPs and algorithmic HBM bytes. */
int op_profile_enable(op_ctx* ctx, int32_t enable);
int op_profile_read(op_ctx* ctx, int32_t cls, double* ms, int64_t* launches, double* flops, double* bytes);
int op_profile_reset(op_ctx* ctx);
/* Which classes op_profile_enable times (bit c = class c; default 0x7F = all). */
#define OP_PROFILE_CLASSES 7
int op_profile_classes(op_ctx* ctx, int32_t mask);

/* Launch census of the bf16x3 conv kernels (process-wide, all contexts; counted on the host when a
 * launch is enqueued, so a replayed hipGraph adds nothing): counts[i] for i < n, then the counts are
 * zeroed if reset.  Lets a test assert which kernel instantiation a configuration really ran (the
 * 7x7 tile size is picked per launch shape by a cost model).  No reference counterpart.
 * Slots: 1..10 = conv_m16_bf16x3<7, NPX> launches with NPX 16-px blocks per wave (640-px raster
 * tiles at 10), and: */
#define OP_CENSUS_7X7_SPLITK 11  /* 7x7 launches that split their input chunks (split-K) */
#define OP_CENSUS_7X7_OTHER 12   /* 7x7 on the conv_big fallback family */
#define OP_CENSUS_3X3_W48 13     /* conv_m16k_bf16x3<false> on 4 x 48 tiles */
#define OP_CENSUS_3X3_W32 14     /* conv_m16k_bf16x3<false> on 8 x 32 tiles */
#define OP_CENSUS_3X3_POOL 15    /* conv_m16k_bf16x3<true> (fused 2x2 max-pool) */
#define OP_CENSUS_3X3_SPLITK 16  /* conv_m16k launches with split-K */
#define OP_CENSUS_3X3_BIG 17     /* conv_big_bf16x3<3, ...> (shapes conv_m16k does not take) */
#define OP_CENSUS_CONV1_PAIR 18  /* conv1_pair_bf16x3 (fused conv1_1 + conv1_2 + pool) */
#define OP_CENSUS_3X3_R256 19    /* conv_m16r_bf16x3<8, ...> (register weights, 256 channels per workgroup) */
#define OP_CENSUS_3X3_R128 20    /* conv_m16r_bf16x3<4, ...> (128 channels per workgroup) */
#define OP_CENSUS_3X3_R_POOL 21  /* conv_m16r_bf16x3<., ., ., true> (fused 2x2 max-pool) */
#define OP_CENSUS_7X7_PLANAR 22  /* 7x7 launches on chunk-planar tensors (op_set_stage_layout) */
#define OP_CENSUS_7X7_FRAME_ALIGNED 23  /* conv_m16 7x7 launches on frame-aligned raster tiles (no tile
                                           crosses a frame; else batch rasters that do) */
#define OP_CENSUS_7X7_TIGHT 24   /* conv_m16 7x7 launches with the tight halo pitch w + 6 (wide maps) */
#define OP_CENSUS_CUBIC_FUSED 25 /* detect_precise map resizes as one fused pass (resize_cubic_fused_mean) */
#define OP_CENSUS_CUBIC_TWO_PASS 26 /* ... as the two-pass path (padded-size maps in HBM) */
/* slot 27: retired in round 5 (the in-kernel split-K experiment was removed) */
#define OP_CENSUS_CUBIC_ROWS 28  /* two-pass second resize as one row-block launch for the batch
                                    (resize_cubic_f32_planar_mean_rows), else one launch per frame */
#define OP_CENSUS_F32_LDS 29     /* exact-f32 3x3 / 7x7 launches on the LDS-halo kernel conv_f32_lds (round 5) */
#define OP_CENSUS_7X7_STAG 30       /* conv_m16 7x7 launches with the staggered halves (round 5) */
#define OP_CENSUS_7X7_PLAIN_RING 31 /* ... with one ring barrier per pair for all 8 waves */
#define OP_CENSUS_7X7_Q 32          /* 7x7 launches on the small-launch kernel conv_m16q_bf16x3 (round 5) */
#define OP_CENSUS_7X7_CIRC 33       /* staggered conv_m16 7x7 launches with circular halo planes (round 6) */
#define OP_CENSUS_PRECISE_SIDE 34   /* detect_precise runs whose small scales ran on the side stream (round 6) */
#define OP_CENSUS_7X7_Q_IWG 35      /* conv_m16q launches with both tap ranges in one 8-wave workgroup (round 6) */
#define OP_CENSUS_7X7_LIN 36        /* conv_m16 launches with linear halo sources (LIN, round 6) */
#define OP_CENSUS_7X7_Q_BPF 37      /* conv_m16q launches with B fragments one tap ahead (round 6) */
#define OP_CENSUS_7X7_PERS 38       /* conv_m16 launches as a persistent grid of one workgroup per CU (round 6) */
#define OP_CENSUS_SLOTS 40
int op_conv_census(int32_t* counts, int32_t n, int32_t reset);

/* Algorithmic FLOPs of the forward for one frame of net size h x w (2*Ci*Co*k*k*H*W summed). */
double op_forward_flops(int32_t h, int32_t w);

/* ---- Multi-GPU result gather: frames shard round-robin over one process per GPU; the
 * only exchange is the per-frame result records, gathered to rank 0 over RCCL from device memory ----
 *
 * Record of one frame (record_bytes = 32 + max_persons * 55 * 8): int32 {status, n_peaks,
 * n_persons, 0}, int64 global frame id (frame_base + i * frame_stride), 8 zero bytes, then
 * max_persons x 18 x 3 f64 poses and max_persons f64 scores (persons past max_persons are not
 * carried; n_persons still counts them; rows past n_persons are zero).  A frame over the batched
 * post-process caps carries status OP_ERR_CAPACITY (op_fetch_result re-runs it uncapped; in a
 * gather, op_comm_overflow_result). */
int op_pack_results(op_ctx* ctx, int32_t first, int32_t n, int32_t max_persons, int64_t frame_base,
                    int32_t frame_stride, void* host_records);
#define OP_COMM_ID_BYTES 128
typedef struct op_comm op_comm;
/* RCCL's unique id (ncclGetUniqueId), made by rank 0 and passed to every rank by the host. */
int op_comm_unique_id(uint8_t* id);
/* Communicator of `world` ranks on ctx's device (ncclCommInitRankConfig, non-blocking); gives up with
 * OP_ERR_TIMEOUT after timeout_s. */
int op_comm_create(op_ctx* ctx, int32_t world, int32_t rank, const uint8_t* id, double timeout_s, op_comm** out);
int op_comm_destroy(op_comm* comm);
/* Enqueue: pack the records of staged frames [first, first+n) after ctx's queued work, then
 * ncclGather them to rank 0 on the communicator's own stream (and copy them to pinned host memory
 * there).  Returns at once; at most two gathers outstanding (double-buffered: step k's gather
 * overlaps step k+1's compute).  Every rank passes the same n and max_persons. */
int op_comm_gather_results(op_comm* comm, op_ctx* ctx, int32_t first, int32_t n, int32_t max_persons,
                           int64_t frame_base, int32_t frame_stride);
/* Wait for the oldest outstanding gather, at most timeout_s (then the communicator is aborted and
 * OP_ERR_TIMEOUT returned).  Rank 0: *records = n_frames records of rec_bytes each in rank order
 * (valid until the gather two submits later); other ranks: *records = NULL, *n_frames = 0. */
int op_comm_wait(op_comm* comm, double timeout_s, const void** records, int32_t* n_frames, int64_t* rec_bytes);
/* Every frame reaches rank 0 whole (pose_detector.py:484-517 returns every frame's poses): after
 * op_comm_wait, each rank lists the frames of its own part of that gather whose record does not
 * carry the whole result -- status OP_ERR_CAPACITY (over the batched post-process caps) or more
 * persons than max_persons -- as indices i in [0, n) of its op_comm_gather_results call (global id
 * frame_base + i * frame_stride), with reasons[i] (may be NULL) = 1 over the caps, 2 past
 * max_persons.  When the records were packed, an over-cap frame's post-process input was copied
 * aside on the device (op_comm_overflow_result re-runs it alone, uncapped: the result
 * op_fetch_result would have given) and a frame past max_persons kept its complete result rows
 * (copied out as they are) -- so both are exact even after later steps have run; the host ships
 * them to rank 0 (frames.py: TCP).  Valid until the next op_comm_gather_results, which packs into
 * that gather's slot (after it, both calls return OP_ERR_STATE until the next op_comm_wait).
 * Device keep space per slot: OP_KEEP_FRAMES (env, default 8) frames of each kind, compacted (rows
 * past max_persons go to page-locked memory first, OP_KEEP_ROWS_AVG); a frame beyond that has no
 * copy and op_comm_overflow_result returns OP_ERR_CAPACITY for it. */
int op_comm_overflow(op_comm* comm, op_ctx* ctx, int32_t* frames, int32_t* reasons, int32_t cap, int32_t* count);
int op_comm_overflow_result(op_comm* comm, op_ctx* ctx, int32_t frame, double* poses, double* scores, int32_t cap,
                            op_frame_result* res);

/* ---- Face / hand keypoint detectors: FaceNet / HandNet single-branch CPM nets ----
 * face_detector.py:12-56 (FaceDetector), hand_detector.py:12-66 (HandDetector); the same conv kernels
 * as CocoPoseNet, bf16x3 arithmetic.  One context = one network on one device, one stream. */
#define OP_ARCH_FACENET 1 /* models/FaceNet.py: 71 heat maps (70 keypoints + background) */
#define OP_ARCH_HANDNET 2 /* models/HandNet.py: 22 heat maps (21 keypoints + background) */
typedef struct op_cpm_ctx op_cpm_ctx;
/* Number of conv layers of `arch` (52) and their table in models/FaceNet.py:11-76 order. */
int op_cpm_layer_count(int32_t arch);
int op_cpm_layer_info(int32_t arch, int32_t index, const char** name, int32_t* ci, int32_t* co, int32_t* ksize);
int op_cpm_create(int32_t arch, int32_t device, op_cpm_ctx** out);
int op_cpm_destroy(op_cpm_ctx* ctx);
/* serializers.load_npz(weights_file, self.model) (face_detector.py:16): layers in op_cpm_layer_info order. */
int op_cpm_set_weights(op_cpm_ctx* ctx, const float* const* W, const float* const* b);
/* FaceNet.__call__ / HandNet.__call__ (models/FaceNet.py:78-161): x (n, 3, h, w) f32 NCHW
 * (h, w multiples of 8) -> last-stage maps (n, C, h/8, w/8) f32. */
int op_cpm_forward(op_cpm_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, float* maps);
/* A test aid, as op_forward_probe is for CocoPoseNet: the forward run from x up to and including the
 * launches of probe point `point`, and the tensor that point wrote returned as dense f32 (nframes,
 * channels, h/divisor, w/divisor) for frames [frame0, frame0 + nframes); split-stored values come
 * back as hi + lo.  The points are the launch boundaries of the forward in execution order; a pair
 * or a conv + pool that runs as two launches is still one point:
 *   0 the network input as stored; 1 conv1_1+conv1_2+pool; 2 conv2_1; 3 conv2_2+pool; 4-6 conv3_1 ..
 *   conv3_3; 7 conv3_4+pool; 8-11 conv4_1 .. conv4_4; 12, 13 conv5_1, conv5_2; 14 conv5_3_CPM (the
 *   128-channel feature map); 15 the stage-1 pair conv6_1_CPM+conv6_2_CPM; then for stage s = 2 .. 6
 *   at 16 + 6 (s - 2) + i: i = 0 .. 4 Mconv1 .. Mconv5, i = 5 the pair Mconv6+Mconv7.
 * The map points (15, 21, ..., 45) return the stage buffer the next Mconv1 reads in the order of
 * the reference's concat: its heat slice as stored with the channel padding (80 channels for
 * FaceNet, 32 for HandNet; those from C on are 0), then the 128 feature channels.  A bad point,
 * frame range, out_floats (!= nframes * channels * (h/divisor) * (w/divisor)) or null pointer is
 * OP_ERR_INVALID before anything is launched, missing weights OP_ERR_STATE.  op_cpm_forward
 * enqueues the same launches as without this entry point.
 * point + OP_CPM_PROBE_HI returns the hi halves alone: hi + lo does not say which pair a kernel
 * stored when it lies exactly halfway between two bf16 values (hi rounded up and lo = -half a step,
 * or down and +half), and the next layer's products w_hi x_hi + w_hi x_lo + w_lo x_hi depend on it.
 * op_cpm_probe_info: a point's name, channel count and size divisor (46 points, 0 .. 45). */
#define OP_CPM_PROBE_HI 256
int op_cpm_probe_info(int32_t arch, int32_t point, const char** name, int32_t* channels, int32_t* divisor);
int op_cpm_forward_probe(op_cpm_ctx* ctx, const float* x, int32_t n, int32_t h, int32_t w, int32_t point,
                         int32_t frame0, int32_t nframes, float* out, int64_t out_floats);
/* compute_peaks_from_heatmaps, CPU branch (face_detector.py:58-84, hand_detector.py:68-94): for each
 * of the first c-1 maps of heatmaps (c, h, w): gaussian_filter(sigma 2.5), global max m; found[i] =
 * m > thresh (f32); keypoints[i] = [coords[1], coords[0], m] of np.where(map == m) flattened
 * ([x, y] for one maximum, [y1, y0] for several, as the reference).  flip != 0 reads the maps
 * mirrored in x (hand_detector.py:47-48: the left-hand maps are flipped before the peaks). */
int op_cpm_peaks(op_cpm_ctx* ctx, const float* heatmaps, int32_t c, int32_t h, int32_t w, float thresh,
                 int32_t flip, double* keypoints, int32_t* found);
/* FaceDetector.__call__ / HandDetector.__call__ on one BGR crop (h x w x 3 u8): cv2 LINEAR resize to
 * 368 x 368, x/256 - 0.5, forward, F.resize_images to (h, w), peaks as op_cpm_peaks (flip_maps: the
 * left-hand map flip; the left-hand input flip is the host copy the reference also makes).
 * keypoints (c-1, 3) f64, found (c-1,). */
int op_cpm_detect(op_cpm_ctx* ctx, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride, float thresh,
                  int32_t flip_maps, double* keypoints, int32_t* found);
/* op_cpm_detect over n crops of any sizes in one batched forward (demo.py:38-56's per-person face /
 * hand calls, which the reference makes one at a time): crop i = bgr[i] (h[i] x w[i] x 3 u8, row
 * stride row_stride[i]), flip_maps[i] as above (may be NULL: none).  Results equal n op_cpm_detect
 * calls up to f32 re-association (a lone crop's 7x7 convs split their input chunks over workgroups):
 * keypoints (n, c-1, 3) f64, found (n, c-1). */
int op_cpm_detect_batch(op_cpm_ctx* ctx, int32_t n, const uint8_t* const* bgr, const int32_t* h, const int32_t* w,
                        const int64_t* row_stride, float thresh, const int32_t* flip_maps, double* keypoints,
                        int32_t* found);
/* enable != 0: no split-K on small launches, so a crop's result does not depend on how many crops
 * share its batch (op_cpm_detect_batch == op_cpm_detect bit for bit).  Like op_set_batch_invariant. */
int op_cpm_set_batch_invariant(op_cpm_ctx* ctx, int32_t enable);
/* op_cpm_detect_batch fed from frames and boxes: ROI i is the box roi_box[4 i ..] = (l, t, r, b) of
 * frame roi_frame[i] (bgr[f]: fh[f] x fw[f] x 3 u8, row stride row_stride[f]), read mirrored in x
 * where roi_mirror[i] != 0 (may be NULL: none).  The crop is virtual: its (y, x) is
 * frame[t + y][l + (mirror ? r-l-1-x : x)], 0 outside the frame (PoseDetector.crop_image, then
 * [:, ::-1]); a mirrored ROI also reads its maps mirrored (the left hand of hand_detector.py).  Each
 * frame is uploaded once, the tables (24 B per frame, 48 B per ROI) once, and the launches around the
 * forward number 1 + 4 * groups whatever n is.  Results equal op_cpm_detect_batch on the host-made
 * crops bit for bit: keypoints (n, c-1, 3) f64, found (n, c-1).  OP_ERR_INVALID (naming the frame or
 * ROI) before anything is launched for: null pointers, n < 0, a frame index outside [0, n_frames), a
 * frame below 1 x 1 or a row stride below 3 * w, r-l < 2 or b-t < 2, (r-l) * (b-t) >= 2^31, a
 * coordinate beyond +-2^30.  n == 0: OP_OK, nothing is touched. */
int op_cpm_detect_rois(op_cpm_ctx* ctx, int32_t n_frames, const uint8_t* const* bgr, const int32_t* fh,
                       const int32_t* fw, const int64_t* row_stride, int32_t n, const int32_t* roi_frame,
                       const int32_t* roi_box, const int32_t* roi_mirror, float thresh, double* keypoints,
                       int32_t* found);
/* Scratch budget of one post-process group of op_cpm_detect_rois (two f32 sets of the ROIs' full-size
 * planes); consecutive ROIs share a group while they fit, a ROI beyond the budget alone is its own
 * group.  0: the default (256 MiB). */
int op_cpm_set_roi_group_bytes(op_cpm_ctx* ctx, int64_t bytes);
/* The last successful op_cpm_detect_rois: out = {groups, launches outside the forward, bytes uploaded
 * (packed frames + tables), scratch bytes laid out}. */
int op_cpm_roi_stats(op_cpm_ctx* ctx, int64_t out[4]);
/* op_cpm_detect_rois with the frames where ctx staged them (op_stage_frames, or the frames an
 * op_run_staged* took from op_upload_frames): ROI i is a box of staged frame first + roi_frame[i]
 * (roi_frame in [0, n_frames)), read in place; nothing but the tables (24 B per frame, 48 B per ROI)
 * is uploaded.  The launches run on cpm's stream behind an event recorded on ctx's stream (no host
 * synchronisation for the ordering); the call itself returns synchronised, so the frames need no
 * protection from a later stage or upload.  With op_cpm_set_roi_batch the ROIs run in consecutive
 * chunks, one forward each.  Results as op_cpm_detect_rois on the same frames given from the host,
 * bit for bit (with op_cpm_set_batch_invariant also across chunk sizes).  OP_ERR_INVALID before any
 * launch for: contexts on different devices, no staged set, frames [first, first + n_frames) outside
 * the staged set, and the ROI checks of op_cpm_detect_rois.  n == 0: OP_OK.  op_cpm_roi_stats then
 * reports the sums over the chunks; its bytes uploaded are 24 n_frames + 48 (ROIs of the chunk) per
 * chunk: no pixel bytes. */
int op_cpm_detect_rois_staged(op_cpm_ctx* cpm, op_ctx* ctx, int32_t first, int32_t n_frames, int32_t n,
                              const int32_t* roi_frame, const int32_t* roi_box, const int32_t* roi_mirror,
                              float thresh, double* keypoints, int32_t* found);
/* At most `rois` ROIs per forward in op_cpm_detect_rois_staged (0, the default: all in one, as
 * op_cpm_detect_rois); the activation arena and the scratch are sized to the largest chunk. */
int op_cpm_set_roi_batch(op_cpm_ctx* cpm, int32_t rois);

/* ---- Training iteration: Updater.update_core of train_coco_pose_estimation.py:93-123 ----
 * One context = CocoPoseNet master weights (f32), Adam state and every activation of a batch of n
 * frames of h x w (multiples of 8) on one device.  Exact f32 (v_mfma_f32_32x32x2_f32 forward and
 * input-gradient convs).  Layers in op_layer_info order. */
typedef struct op_train_ctx op_train_ctx;
int op_train_create(int32_t device, int32_t n, int32_t h, int32_t w, op_train_ctx** out);
int op_train_destroy(op_train_ctx* ctx);
/* initmodel / copy_vgg_params (:183-189): weights + biases; resets the Adam state. */
int op_train_set_weights(op_train_ctx* ctx, const float* const* W, const float* const* b);
/* Current weights / biases and the last step's (unscaled) gradients; any array may be null. */
int op_train_get_weights(op_train_ctx* ctx, float* const* W, float* const* b, float* const* gW, float* const* gb);
/* optimizers.Adam(alpha, beta1, beta2, eps) (:214); the caller's alpha schedule (:104-107) sets alpha. */
int op_train_set_hyper(op_train_ctx* ctx, double alpha, double beta1, double beta2, double eps);
/* enable_update / disable_update of one layer (:225-230, :97-102). */
int op_train_enable_layer(op_train_ctx* ctx, int32_t layer, int32_t enable);
/* GradientScaling hook (train_coco_pose_estimation.py:25-38, registered at :213-217): the step
 * multiplies this layer's W and b gradients by `scale` (f32) before Adam.  Default 1 (no hook). */
int op_train_set_grad_scale(op_train_ctx* ctx, int32_t layer, double scale);
/* One iteration: x = preprocess(imgs) (n, 3, h, w) f32; pafs_t (n, 38, h/8, w/8), heat_t (n, 19, h/8,
 * w/8) f32; ignore (n, h/8, w/8) u8 (1 = ignored); losses[12] = per stage (paf, heat) MSE of
 * compute_loss (:42-77).  Forward, loss, backward, the per-layer gradient scales
 * (op_train_set_grad_scale), Adam on the enabled layers. */
int op_train_step(op_train_ctx* ctx, const float* x, const float* pafs_t, const float* heat_t, const uint8_t* ignore,
                  double* losses);

/* ---- Training labels from keypoint annotations (coco_data_loader.py:208-268, :340) ----
 * poses: sum(counts) x 18 x 3 f64 (x, y, visibility; a joint counts when visibility > 0), frame f's
 * people at pose_offsets[f] .. pose_offsets[f+1] (pose_offsets[0] = 0, n + 1 entries); mask (n, h, w)
 * u8, nonzero = ignored, may be null (no ignored pixels); outputs are host pointers, any may be null.
 * Heat maps: per joint the max over people of exp(-0.5 d^2 / heatmap_sigma^2), channel 18 = 1 - the
 * max over all joints; PAFs: the unit limb vector within paf_width of the limb, averaged over the
 * people whose limb covers the pixel; ignore: the mask dilated by ones((16, 16)) (cv2.MORPH_DILATE).
 * downscale 1: those maps at h x w.  downscale d > 1 (h % d == 0, w % d == 0, h/d, w/d >= 2): the
 * (h/d, w/d) maps F.resize_images would make of them (compute_loss, train_coco_pose_estimation.py:
 * 56-60: targets resized, mask = resize(mask) > 0), evaluated at the four bilinear taps of every
 * output pixel only.  Arguments are validated before any device call (OP_ERR_INVALID). */
int op_make_labels(int32_t device, int32_t n, int32_t h, int32_t w, int32_t downscale, const double* poses,
                   const int32_t* pose_offsets, const uint8_t* mask, double heatmap_sigma, double paf_width,
                   float* pafs /* n,38,oh,ow */, float* heatmaps /* n,19,oh,ow */, uint8_t* ignore /* n,oh,ow */);
/* op_train_step with the targets generated on the device: the downscale-8 labels of (poses,
 * pose_offsets, mask (n, h, w) or null) are written on the context's stream straight into the
 * step's target and ignore buffers, then the same iteration runs. */
int op_train_step_poses(op_train_ctx* ctx, const float* x, const double* poses, const int32_t* pose_offsets,
                        const uint8_t* mask /* n,h,w */, double heatmap_sigma, double paf_width, double* losses);
/* Device time (ms, stream events) of the label part of the last op_train_step_poses: the uploads of
 * the pose records and the mask plus the label kernel.  OP_ERR_STATE before the first such step. */
int op_train_last_label_ms(op_train_ctx* ctx, double* ms);

/* ---- Validation (Validator.evaluate, train_coco_pose_estimation.py:129-159) ----
 * The forward and compute_loss of op_train_step over the first m frames of the context (1 <= m <= n,
 * else OP_ERR_INVALID; OP_ERR_STATE before op_train_set_weights): arrays as for op_train_step with m
 * in place of n.  No backward and no update: weights, Adam state, step counters, enabled flags,
 * gradient scales, the gradients op_train_get_weights reports and op_train_last_label_ms are all
 * left as they were.  The loss arithmetic is op_train_step's (same blocks, same reduction order), so
 * with m == n the twelve losses equal, bit for bit, the ones a following op_train_step returns for
 * the same batch. */
int op_train_eval(op_train_ctx* ctx, int32_t m, const float* x, const float* pafs_t, const float* heat_t,
                  const uint8_t* ignore, double* losses /* 12 */);
/* op_train_eval with the targets generated on the device as in op_train_step_poses (pose_offsets has
 * m + 1 entries, mask (m, h, w) or null). */
int op_train_eval_poses(op_train_ctx* ctx, int32_t m, const float* x, const double* poses,
                        const int32_t* pose_offsets, const uint8_t* mask, double heatmap_sigma, double paf_width,
                        double* losses /* 12 */);

/* ---- Optimizer state (extensions.snapshot() / --resume FILE, :255, :265-266) ----
 * Adam's first and second moments of every layer's W and b and the per-layer step counts t (a layer
 * counts only the steps it was enabled in), arrays of 92 pointers / values in op_layer_info order.
 * get waits for the stream; a null array or null entry is skipped.  set needs every pointer and
 * t[l] >= 0 (else OP_ERR_INVALID, nothing written).  op_train_set_weights zeroes this state, so a
 * restore calls op_train_set_weights first and op_train_set_state after it. */
int op_train_get_state(op_train_ctx* ctx, float* const* mW, float* const* vW, float* const* mb, float* const* vb,
                       int64_t* t /* 92 */);
int op_train_set_state(op_train_ctx* ctx, const float* const* mW, const float* const* vW, const float* const* mb,
                       const float* const* vb, const int64_t* t /* 92 */);

/* ---- Read-back of the step's tensors (a test aid, as op_forward_probe is for the forward) ----
 * op_train_buffer_info (host only): buffer i of the step's OP_TRAIN_BUFFERS activation tensors in
 * the order the step keeps them (the network input, every conv and pool output, the five 192-channel
 * stage inputs in the inference layout: feature 0..127, heat 128..146, paf 152..189, and the stage-6
 * maps: paf 0..37, heat 40..58), its physical channel count and size divisor.
 * op_train_read_buffer copies the dense (n, channels, h / divisor, w / divisor) f32 interior of
 * activation (grad == 0) or gradient (grad != 0) buffer i as the last completed op_train_step /
 * op_train_step_poses left it: the gradient of a conv output is the one its weight- and
 * input-gradient launches read (after the ReLU mask), that of a stage input or pool output the sum
 * its consumers and the loss wrote.  Nothing of the training state is touched: a step, reads, a step
 * equal two steps bit for bit.  OP_ERR_STATE before the first step; OP_ERR_INVALID for a bad index,
 * out_floats != n * channels * (h / divisor) * (w / divisor) or a null pointer. */
#define OP_TRAIN_BUFFERS 89
int op_train_buffer_info(int32_t i, const char** name, int32_t* channels, int32_t* divisor);
int op_train_read_buffer(op_train_ctx* ctx, int32_t i, int32_t grad, float* out, int64_t out_floats);

/* ---- Training-sample augmentation (coco_data_loader.py:60-205: resize, rotate, crop, colour, flip) ----
 * One sample's plan, every random draw already made on the host (augment.py draw_plan): the source
 * is resized to rw x rh (cv2.resize, linear), warped by the 2x3 forward matrix R into a bw x bh
 * image (cv2.warpAffine: cubic, border 128, for the image; linear on mask * 255, border 0, > 0 for
 * the mask), of which rows y1 .. y2, columns x1 .. x2 are copied to rows y_from .. y_to, columns
 * x_from .. x_to of an insize x insize crop filled with 127 / false (x2 < x1 or y2 < y1: nothing is
 * copied); then, when colour != 0, BGR2HSV, clip(channel + (dh, ds, dv), 0, 255), HSV2BGR; then,
 * when flip != 0, the horizontal flip.  degree and (ox, oy) are carried for the record only. */
typedef struct op_augment_plan {
  int32_t h, w;   /* source size */
  int32_t rw, rh; /* resized size */
  double degree;
  double R[6]; /* row-major 2x3, after the bounding-box shift */
  int32_t bw, bh; /* rotated size */
  int32_t ox, oy; /* crop offset */
  int32_t x1, y1, x2, y2, x_from, y_from, x_to, y_to;
  int32_t colour, dh, ds, dv; /* colour != 0: the signed deltas apply */
  int32_t flip;
  int32_t insize;
} op_augment_plan;
/* A batch of n samples on `device`: bgr[f] is sample f's h x w x 3 u8 image with row_stride[f] bytes
 * per row, mask[f] its h x w u8 ignore mask (nonzero = ignored; the array or an entry may be null:
 * nothing ignored); outputs are host pointers.  Two kernels for the whole batch (the resize, then
 * one fused pass per output pixel: the rotated image is never written), bit-identical to
 * augment.py's augment_np.  Arguments are validated before any device call (OP_ERR_INVALID, the
 * message names the field): null arrays, n < 1, insize < 1, sizes < 1, rw / rh / bw / bh above 16384
 * (the warp keeps source coordinates as shorts), a plan's insize other than the call's, non-finite
 * R, a copy window that does not fit insize or bw x bh, colour deltas outside [-10, 10], [-40, 40],
 * [-30, 30]. */
int op_augment(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
               const uint8_t* const* mask /* entries or the array may be null */, const op_augment_plan* plans,
               int32_t insize, uint8_t* out_bgr /* n,insize,insize,3 */, uint8_t* out_mask /* n,insize,insize */);
/* Device time (ms, stream events) of the uploads and kernels of the last op_augment that completed
 * on `device`; OP_ERR_STATE before the first. */
int op_augment_last_ms(int32_t device, double* ms);
/* counts[2] of that call: output pixels whose warp taps were read from the tile's box staged in
 * LDS, and from global memory (a tile whose source box exceeds the LDS budget); pixels outside
 * their copy window count in neither.  OP_ERR_STATE before the first call. */
int op_augment_last_paths(int32_t device, int64_t* counts);
/* (host only) The tables the kernels read: warpAffine's remap weights, cubic [1024][16] and linear
 * [1024][4] int16 (set ay * 32 + ax, rows of columns, every set sums to 1 << 15), and BGR2HSV's
 * sdiv[256], hdiv[256] int32.  Any pointer may be null. */
int op_augment_tables(int16_t* cubic, int16_t* linear, int32_t* sdiv, int32_t* hdiv);

/* ---- Ignore masks from COCO segmentations (gen_ignore_mask.py:23-37 gen_masks, COCO.annToMask) ----
 * A batch of n images on `device`.  Image f is hw[2f] x hw[2f + 1] (h, w) and owns the annotations
 * ann_offsets[f] .. ann_offsets[f + 1] - 1, in gen_masks' order; annotation a has the role ann_role[a]
 * (what gen_masks does with its mask, decided by the caller: OP_MASK_KEEP mask_all |= mask;
 * OP_MASK_MISS both |= mask; OP_MASK_CROWD mask_miss |= mask & ~mask_all, then mask_all |= mask) and
 * the parts part_offsets[a] .. part_offsets[a + 1] - 1, whose union is its mask (annToMask); it may
 * have none.  Part p is one polygon (part_kind[p] = OP_MASK_POLYGON: x0, y0, x1, y1, ... as doubles,
 * at least 3 points) or one uncompressed RLE (OP_MASK_RLE: run lengths of 0s and 1s alternating,
 * column-major, 0s first); its elements are xy[data_offsets[p] .. data_offsets[p + 1] - 1] or
 * counts[the same range]: the two arrays share one index space, the slots of the other kind are
 * not read (xy may be null when there is no polygon, counts when there is no RLE).
 * out_all[f] / out_miss[f]: host pointers to h * w u8 (row-major, 0 / 1), gen_masks' mask_all and
 * mask_miss of image f; out_ann[a]: annotation a's own mask.  Each of the three arrays, and any
 * entry, may be null: not wanted.  The result is masks.py's gen_masks_np / ann_to_mask_np bit for bit
 * (the polygon rasteriser restates pycocotools' rleFrPoly; that parity is unpinned).
 * Three kernels for the whole batch: polygon edges into toggle bits (one thread per point of the
 * 5x upsampled outline), RLE running sums into toggle bits, and per block of columns the parity
 * fill, the union and the three role rules.
 * Arguments are validated before any device call (OP_ERR_INVALID, the message names the field):
 * null arrays, n < 1, h or w outside 1 .. 16384, offsets that do not start at 0 or decrease, an
 * unknown role or kind, a polygon of odd length or fewer than 3 points, a coordinate that is not
 * finite or above 65536 in magnitude, an outline of more than 2^31 - 1 upsampled points in the batch,
 * an RLE whose counts do not sum to h * w. */
#define OP_MASK_KEEP 0
#define OP_MASK_MISS 1
#define OP_MASK_CROWD 2
#define OP_MASK_POLYGON 0
#define OP_MASK_RLE 1
int op_ignore_masks(int32_t device, int32_t n, const int32_t* hw, const int32_t* ann_offsets, const int32_t* ann_role,
                    const int32_t* part_offsets, const int32_t* part_kind, const int64_t* data_offsets,
                    const double* xy, const uint32_t* counts, uint8_t* const* out_all, uint8_t* const* out_miss,
                    uint8_t* const* out_ann);
/* Device time (ms, stream events) of the uploads and kernels of the last op_ignore_masks that
 * completed on `device`; OP_ERR_STATE before the first. */
int op_ignore_masks_last_ms(int32_t device, double* ms);

/* ---- The --vis viewer of gen_ignore_mask.py (:39-71 draw_masks_and_keypoints, dwaw_gen_masks) ----
 * A batch of n frames of any sizes on `device`.  bgr[f] is frame f's hw[2f] x hw[2f + 1] (h, w) x 3 u8
 * image with row_stride[f] bytes per row (host pointers, as for op_draw).  hw, ann_offsets, ann_role,
 * part_offsets, part_kind, data_offsets, xy and counts are op_ignore_masks' arguments, unchanged.
 * ann_tint[a] is the colour annotation a's mask is tinted with, decided by the caller as ann_role is:
 * the code is the BGR channel the tint raises (OP_VIEW_PERSON (1, 0, 0), OP_VIEW_NO_KEYPOINTS (0, 1, 0),
 * OP_VIEW_CROWD (0, 0, 1) in the reference's tuples).  Annotation a owns the keypoints
 * kp_offsets[a] .. kp_offsets[a + 1] - 1 of kp, int32 (x, y, v) triples: v = 1 paints a filled
 * radius-3 disc (255, 255, 0), v = 2 one of (255, 0, 255), any other v nothing (draw.draw_disc's pixels:
 * dx * dx + dy * dy <= 9).
 * out_ann[f]: host pointer to h * w * 3 u8, draw_masks_and_keypoints(frame, annotations): a float64
 * image carried from annotation to annotation, per annotation in order v = (v + 0.7 * c * 255) - 0.7 * v
 * under its mask and then its discs in order, one truncating cast at the end.  out_miss[f]:
 * dwaw_gen_masks(frame, mask_miss), that step once with (0, 0, 1) under gen_masks' mask_miss.  Either
 * array, or any entry, may be null: not wanted.  The result is maskview.py's view_np byte for byte
 * (the disc and polygon rasterisers stay unpinned against OpenCV's and pycocotools').
 * The masks come from op_ignore_masks' three kernels and stay on the device; then one kernel launch
 * for the whole batch, one workgroup per 64 x 16 pixel tile of a frame.
 * Arguments are validated before any device call (OP_ERR_INVALID, the message names the field):
 * everything op_ignore_masks refuses, null bgr / row_stride or a null frame, a row stride below 3 w, an
 * unknown tint, kp_offsets that do not start at 0 or decrease, null kp with keypoints, a keypoint
 * coordinate above 32768 in magnitude. */
#define OP_VIEW_PERSON 0
#define OP_VIEW_NO_KEYPOINTS 1
#define OP_VIEW_CROWD 2
int op_annotation_views(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
                        const int32_t* hw, const int32_t* ann_offsets, const int32_t* ann_role, const int32_t* ann_tint,
                        const int32_t* part_offsets, const int32_t* part_kind, const int64_t* data_offsets,
                        const double* xy, const uint32_t* counts, const int32_t* kp_offsets, const int32_t* kp,
                        uint8_t* const* out_ann, uint8_t* const* out_miss);
/* Device time (ms, stream events) of the uploads and kernels (the mask kernels and the view kernel)
 * of the last op_annotation_views that completed on `device`; OP_ERR_STATE before the first. */
int op_annotation_views_last_ms(int32_t device, double* ms);

/* ---- Skeleton overlays from a display list (draw.py draw_line / draw_disc, demo.py add_weighted) ----
 * One primitive of a frame's display list (render.py builds the lists on the host).  A frame's
 * primitives are painted in order, a later one over an earlier one:
 *   OP_DRAW_LINE  the pixels of draw.draw_line((x0, y0), (x1, y1), bgr, thickness): inside the box
 *                 floor(min(x0, x1) - r) .. ceil(max(x0, x1) + r) (y alike, r = thickness / 2) and
 *                 within r of the segment, in draw.py's float64 operations, one rounding each;
 *   OP_DRAW_DISC  the pixels of draw.draw_disc((x0, y0), radius, bgr): integer centre (x0, y0),
 *                 dx * dx + dy * dy <= radius * radius;
 *   OP_DRAW_BLEND at most one per frame: the picture so far becomes
 *                 saturate_u8(rint(input * wa + picture * wb + gamma)) (demo.add_weighted: float64,
 *                 summed left to right, rint to even); the primitives after it paint over the blend.
 * Fields a kind does not use are not read. */
#define OP_DRAW_LINE 0
#define OP_DRAW_DISC 1
#define OP_DRAW_BLEND 2
typedef struct op_draw_prim {
  int32_t kind;
  int32_t radius;        /* DISC: 0 .. 1024 */
  double x0, y0, x1, y1; /* LINE: end points; DISC: the centre in (x0, y0), whole numbers */
  double thickness;      /* LINE: > 0 */
  double wa, wb, gamma;  /* BLEND */
  uint8_t bgr[3];        /* LINE, DISC */
  uint8_t pad[5];
} op_draw_prim;
/* A batch of n frames of any sizes on `device`: bgr[f] is frame f's hw[2f] x hw[2f + 1] (h, w) x 3 u8
 * image with row_stride[f] bytes per row, its list prims[prim_offsets[f] .. prim_offsets[f + 1] - 1]
 * (it may be empty), out[f] a host pointer to h * w * 3 u8.  One kernel launch for the whole batch,
 * one workgroup per 64 x 16 pixel tile of a frame; the result is render.py's render_np bit for bit
 * (draw.py's rasteriser stays unpinned against OpenCV's).
 * Arguments are validated before any device call (OP_ERR_INVALID, the message names the field): null
 * arrays or entries, n < 1, h or w outside 1 .. 16384, a row stride below 3 w, offsets that do not
 * start at 0 or decrease, an unknown kind, a coordinate that is not finite or above 32768 in
 * magnitude (every integer product of the line test is then exact in float64 and the box fits
 * int32), a disc centre that is not a whole number, a thickness that is not in (0, 32768], a radius
 * outside 0 .. 1024, more than one BLEND in a frame's list, blend weights that are not finite. */
int op_draw(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride, const int32_t* hw,
            const int32_t* prim_offsets, const op_draw_prim* prims, uint8_t* const* out);
/* The same kernel on staged frames [first, first + n) of ctx (op_stage_frames, or the frames an
 * op_run_staged* took from op_upload_frames; an upload no run has taken yet is not drawn on), read in
 * place: no second upload, and the staged frames are not modified.  Frame first + f owns the list
 * prims[prim_offsets[f] .. prim_offsets[f + 1] - 1]; out is n * h * w * 3 u8 on the host.  The kernel
 * runs on the context stream, behind a queued op_run_staged*; the call returns when out is filled.
 * Validation as for op_draw, and a range outside the staged set; OP_ERR_STATE when nothing is staged. */
int op_draw_staged(op_ctx* ctx, int32_t first, int32_t n, const int32_t* prim_offsets, const op_draw_prim* prims,
                   uint8_t* out);
/* The staged frame set op_draw_staged reads: *n frames of *h x *w (all 0 when nothing is staged). */
int op_staged_info(op_ctx* ctx, int32_t* n, int32_t* h, int32_t* w);
/* Device time (ms, stream events) of the uploads and the kernel of the last op_draw or
 * op_draw_staged that completed on `device`; OP_ERR_STATE before the first. */
int op_draw_last_ms(int32_t device, double* ms);

/* ---- PAFs, heat maps and the ignore mask over frames (overlay.py; coco_data_loader.py:29-59, 372-382) ----
 * A batch of n frames of any sizes on `device`: bgr[f] is frame f's hw[2f] x hw[2f + 1] (h, w) x 3 u8
 * image with row_stride[f] bytes per row, out[f] a host pointer to h * w * 3 u8.  Each of pafs, heat
 * and mask may be NULL as a whole or hold a NULL entry for one frame: no such layer there.  pafs[f] is
 * f32 (2L, mh, mw) with paf_chw[3f ..] = (2L, mh, mw), heat[f] f32 (C, mh, mw) with heat_chw[3f ..] =
 * (C, mh, mw), mask[f] u8 (h, w) of any size with mask_hw[2f ..] = (h, w), nonzero = ignored; lut is
 * the 256 x 3 u8 BGR colour table of the heat layer, required when any frame has one.  Per pixel, in
 * this order: the maps resampled to the frame (cv2.resize INTER_LINEAR on f32, one rounded f32
 * operation each; equal sizes are copied), the limbs of the PAFs summed in f64 and shown as hue =
 * direction, saturation = value = magnitude, blended 0.6 / 0.4; the f32 maximum over the heat
 * channels * 255, clamped to 0 .. 255 and truncated, through lut, blended alike; the pixel set to 0
 * where cv2.resize(mask * 255) > 0.  One kernel launch for the whole batch, one workgroup per 64 x 16
 * pixel tile of a frame; the result is overlay.py's overlay_np bit for bit, given that the f64 atan2
 * lands in the same of the 256 hue levels (overlay.hue_margin).  The colour table, the f32 resize and
 * HSV2BGR restate OpenCV and stay unpinned against it.
 * Arguments are validated before any device call (OP_ERR_INVALID, the message names the field): n < 1,
 * null arrays or entries that are required, h or w outside 1 .. 16384, a row stride below 3 w, a PAF
 * channel count that is odd or not positive, a heat channel count below 1, a map or mask side outside
 * 1 .. 16384.  Maps that are not finite are not refused here (overlay.py refuses them): the call is
 * safe, every table index is clamped by comparisons that are false for NaN, and the pixels such
 * values reach are unspecified. */
int op_overlay(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride, const int32_t* hw,
               const float* const* pafs, const int32_t* paf_chw, const float* const* heat, const int32_t* heat_chw,
               const uint8_t* const* mask, const int32_t* mask_hw, const uint8_t* lut, uint8_t* const* out);
/* The same kernel on staged frames [first, first + n) of ctx and on the maps op_fetch_maps would
 * return for them, all read in place on the device: after op_run_staged* the last-stage network maps,
 * after op_run_staged_precise the averaged full-resolution maps (copied through, not resampled).
 * layers is a bit set; the heat layer shows channels 0 .. 17 (the background channel is left out, as
 * in the reference) and needs lut.  out is n * h * w * 3 u8 on the host.  The kernel runs on the
 * context stream, behind a queued op_run_staged*; the call returns when out is filled.  Staged
 * frames, maps and results are not modified.  OP_ERR_STATE when nothing is staged or no run has
 * produced maps of the staged frames, OP_ERR_INVALID for a range outside the staged set. */
#define OP_OVERLAY_PAFS 1
#define OP_OVERLAY_HEAT 2
int op_overlay_staged(op_ctx* ctx, int32_t first, int32_t n, int32_t layers, const uint8_t* lut, uint8_t* out);
/* Device time (ms, stream events) of the uploads and the kernel of the last op_overlay or
 * op_overlay_staged that completed on `device`; OP_ERR_STATE before the first. */
int op_overlay_last_ms(int32_t device, double* ms);

/* ---- Face / hand boxes from poses (wholebody.py; pose_detector.py:267-297, 354-399) ----
 * One kernel, one thread per person, f64 with every operation rounded on its own: unit =
 * PoseDetector.get_unit_length, box[p][0] = the face box of crop_face, box[p][1] / box[p][2] the left /
 * right hand boxes of crop_hands, each (l, t, r, b) truncated toward zero.  state: 0 absent (no nose /
 * no hand), 1 valid, 2 present but not runnable: a coordinate that is not finite or beyond +-2^30,
 * r-l < 2, b-t < 2 or (r-l) * (b-t) >= 2^31, exactly what op_cpm_detect_rois refuses; a box of state 0
 * or 2 is zeros.  The shift of the hand joints (0.3 of elbow -> hand) stays in registers: the poses are
 * not written.  Bit-identical to wholebody.body_rois_np.
 * poses (n_persons, 18, 3) f64 from the host -> unit (n_persons), box (n_persons, 3, 4), state
 * (n_persons, 3).  n_persons == 0: OP_OK. */
int op_body_rois(int32_t device, int32_t n_persons, const double* poses, double* unit, int32_t* box,
                 int32_t* state);
/* The same for the result rows of staged frames [first, first + n) where they lie on the device,
 * after ctx's queued work; persons of frame i are rows [i * cap, i * cap + min(count[i], cap)) of the
 * outputs (unit n * cap, box n * cap * 12, state n * cap * 3).  count[i] = persons found (may exceed
 * cap: OP_ERR_CAPACITY with the rows needed in count, as op_fetch_results); frame_status[i] = the
 * frame's status (a frame over the batched post-process caps has OP_ERR_CAPACITY and count 0 here: the
 * caller takes it through op_fetch_result and op_body_rois).  Only the headers and these tables come
 * back (one asynchronous copy, one synchronisation); the result rows are neither copied nor written. */
int op_body_rois_staged(op_ctx* ctx, int32_t first, int32_t n, int32_t cap, int32_t* count,
                        int32_t* frame_status, double* unit, int32_t* box, int32_t* state);
/* Device time (ms, stream events) of the uploads and the kernel of the last op_body_rois or
 * op_body_rois_staged that completed on `device`; OP_ERR_STATE before the first. */
int op_body_last_ms(int32_t device, double* ms);

/* ---- COCO keypoint matching (keypoint_eval.py; COCOeval's computeOks and evaluateImg for iouType
 * 'keypoints', restated there in NumPy: parity with pycocotools itself is unpinned) ----
 * One kernel launch per call, one workgroup per frame (image), f64 with every operation rounded on
 * its own: the detections ranked by descending score (stable; a NaN score as -inf) and cut to
 * max_dets; the object keypoint similarity of every kept detection and ground truth; per area range
 * and threshold the greedy match.  Bit-identical to keypoint_eval.match_np on every output.
 * Frame f's detections are rows [dt_offsets[f], dt_offsets[f + 1]) of dt_kpts (17 x 3 f64 each: x, y,
 * v in COCO's keypoint order) and dt_scores; its ground truths rows [gt_offsets[f], gt_offsets[f + 1])
 * of gt_kpts (17 x 3), gt_area, gt_bbox (x, y, w, h), gt_ignore and gt_iscrowd (u8).  thrs: n_thrs
 * OKS thresholds; area_rng: n_areas (lo, hi) pairs; sigmas: the 17 per-keypoint constants.
 * Outputs, with M = max_dets, A = n_areas, T = n_thrs, D' = min(detections, M), g0 = gt_offsets[f] and
 * G the frame's ground truths:
 *   dt_order  [f][M]        the kept detections' indices within the frame, -1 past D'
 *   oks       [M * g0 + r * G + g]  of kept detection r and ground truth g; NULL: not wanted
 *   dt_match  [f][A][T][M]  the ground truth (index within the frame) detection r matched, -1 for none
 *   dt_ignore [f][A][T][M]  u8
 *   gt_match  [A * T * g0 + (a * T + t) * G + g]  the detection (index within the frame), -1 for none
 *   gt_ignore_out [A * g0 + a * G + g]  u8: gt_ignore or the area outside range a
 * n_frames == 0: OP_OK.  OP_ERR_INVALID, with nothing written: a null pointer, offsets that do not
 * start at 0 or decrease, max_dets outside 1 .. 64, more than 128 ground truths in a frame (the
 * message names it), n_thrs outside 1 .. 16, n_areas outside 1 .. 4, a gt area that is not finite or
 * negative, a gt bbox, threshold, range or sigma that is not finite, a sigma that is not positive. */
int op_keypoint_match(int32_t device, int32_t n_frames, const int32_t* dt_offsets, const double* dt_kpts,
                      const double* dt_scores, const int32_t* gt_offsets, const double* gt_kpts,
                      const double* gt_area, const double* gt_bbox, const uint8_t* gt_ignore,
                      const uint8_t* gt_iscrowd, int32_t max_dets, int32_t n_thrs, const double* thrs,
                      int32_t n_areas, const double* area_rng, const double* sigmas, int32_t* dt_order, double* oks,
                      int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, uint8_t* gt_ignore_out);
/* The same with the detections read from the result rows (poses and scores) of staged frames
 * [first, first + n) where the post-process left them, after ctx's queued work; joint_map[i] = the
 * pose joint (0 .. 17) that is COCO keypoint i, applied by the kernel.  Only the ground-truth tables
 * are uploaded and only the match block comes back (one asynchronous copy, one synchronisation); the
 * result rows are neither copied nor written.  Further outputs: frame_status[i] = the frame's status
 * (a frame over the batched post-process caps has OP_ERR_CAPACITY and no detections here: the caller
 * takes it through op_fetch_result and op_keypoint_match), dt_count[i] = persons found,
 * dt_scores [i][M] = the kept detections' scores in order (0 past D').  OP_ERR_STATE when nothing is
 * staged or no run has left results of the frames, OP_ERR_INVALID for a range outside the staged set
 * and for everything op_keypoint_match refuses. */
int op_keypoint_match_staged(op_ctx* ctx, int32_t first, int32_t n, const int32_t* joint_map,
                             const int32_t* gt_offsets, const double* gt_kpts, const double* gt_area,
                             const double* gt_bbox, const uint8_t* gt_ignore, const uint8_t* gt_iscrowd,
                             int32_t max_dets, int32_t n_thrs, const double* thrs, int32_t n_areas,
                             const double* area_rng, const double* sigmas, int32_t* frame_status, int32_t* dt_count,
                             double* dt_scores, int32_t* dt_order, double* oks, int32_t* dt_match, uint8_t* dt_ignore,
                             int32_t* gt_match, uint8_t* gt_ignore_out);
/* Device time (ms, stream events) of the uploads and the kernel of the last op_keypoint_match or
 * op_keypoint_match_staged that completed on `device`; OP_ERR_STATE before the first. */
int op_keypoint_last_ms(int32_t device, double* ms);

/* ---- baseline JPEG frames decoded on the device (jpeg.py's decode_np is the statement) ----
 * The subset: SOF0, 8-bit samples, Huffman coding, one interleaved scan, 8-bit quantisation tables,
 * one component (grey -> B = G = R) or three taken as YCbCr with the luma sampled 1x1, 2x1 or 2x2 and
 * both chroma components 1x1; restart intervals and custom Huffman tables are decoded, APPn and COM
 * segments skipped.  The host parses and entropy-decodes (a pool of threads, a frame at a time per
 * thread); dequantisation, the inverse DCT (libjpeg's jidctint), chroma upsampling (libjpeg's fancy
 * filters) and YCbCr -> BGR run in two kernels over the whole batch, bit for bit what libjpeg-turbo
 * (JDCT_ISLOW) writes.  A frame outside the subset is not decoded and not guessed at: it gets a
 * status, fails no call, and the other frames decode as if it were absent. */
#define OP_JPEG_OK 0
#define OP_JPEG_UNSUPPORTED 1 /* well formed, outside the subset (progressive, arithmetic, 12-bit, 4 components,
                                 an Adobe segment, other sampling factors, 16-bit tables, several scans) */
#define OP_JPEG_CORRUPT 2     /* truncated data, an undefined Huffman code, a run past coefficient 63, a bad or
                                 missing marker, a missing table, a wrong restart sequence */
#define OP_JPEG_SIZE 3        /* op_jpeg_stage: the frame is not the h x w asked for */
#define OP_JPEG_RANGE 4       /* a block with sum |coef q| > 32768: the 32-bit inverse DCT is not provably exact */
typedef struct op_jpeg_info {
  int32_t status;       /* OP_JPEG_*; everything below is 0 unless OP_JPEG_OK */
  int32_t h, w, components;
  int32_t hs, vs;       /* the luma's sampling factors (chroma is 1 x 1) */
  int32_t blocks_w[3], blocks_h[3]; /* each component's padded block grid */
  int64_t n_blocks;     /* their sum: 64 int16 coefficients each */
} op_jpeg_info;
/* Host only: the header parse (through the SOS header) of one file.  The status lies in out->status;
 * the return value is OP_ERR_INVALID for a null pointer or negative bytes. */
int op_jpeg_probe(const uint8_t* data, int64_t bytes, op_jpeg_info* out);
/* Host only: the entropy decode of one file, what jpeg.py's coefficients_np states.  coef (coef_cap
 * int16; 64 n_blocks are needed, else OP_ERR_INVALID): the quantised coefficients in natural order,
 * component after component, each component's blocks in raster order over its padded grid; qt
 * (3 x 64): each component's quantisation table in natural order; *status: OP_JPEG_*. */
int op_jpeg_coefficients(const uint8_t* data, int64_t bytes, int16_t* coef, int64_t coef_cap, uint16_t* qt,
                         int32_t* status);
/* Host only: the predicate behind OP_JPEG_RANGE for one block of 64 coefficients and its table (both
 * in natural order): *in_range = sum |coef[k] q[k]| <= 32768. */
int op_jpeg_block_in_range(const int16_t* coef, const uint16_t* q, int32_t* in_range);
/* Decodes n files (any mix of sizes and samplings) on `device` in one call: out[f] = h w 3 bytes of
 * BGR pixels (host pointer, sizes from op_jpeg_probe), status[f] = OP_JPEG_*; a frame whose status is
 * not OP_JPEG_OK leaves out[f] untouched (and may pass a null out[f]).  Arguments are validated
 * before any device call (OP_ERR_INVALID, the message names the field): n outside 0 .. 65535, null
 * arrays, a null file, negative bytes, a null image of a decodable frame, more than 2^25 coefficient
 * blocks.  n == 0, or no decodable frame: OP_OK, no device call (and nothing for op_jpeg_last_ms).
 * OP_ERR_CAPACITY when the host runs out of memory for the batch's tables (also op_jpeg_stage). */
int op_jpeg_decode(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* bytes, uint8_t* const* out,
                   int32_t* status);
/* op_stage_frames with files instead of pixels: frame f of the staged set comes from bgr[f] (h x w x 3
 * u8, contiguous) when bgr and bgr[f] are non-null, else from the file data[f]; the kernels write
 * into the staged set in place, no decoded pixel exists on the host.  A file that is not h x w gets
 * OP_JPEG_SIZE; the slot of every frame whose status is not OP_JPEG_OK is zero-filled (the caller
 * decodes those by other means and stages once more with their bgr entries set).  The coefficients
 * go up from a page-locked buffer of the context in one asynchronous copy on its stream.  Returns
 * once the frames are staged.  h, w in 8 .. 16384, n in 1 .. 65535. */
int op_jpeg_stage(op_ctx* ctx, int32_t n, const uint8_t* const* data, const int64_t* bytes, const uint8_t* const* bgr,
                  int32_t h, int32_t w, int32_t* status);
/* Threads of the entropy-decode pool: 1 .. 64, or 0 for the default, min(16, the host's hardware
 * threads); anything else is OP_ERR_INVALID.  A call uses min(decodable frames, threads) of them. */
int op_jpeg_set_threads(int32_t threads);
/* ms[0] = the host's entropy-decode wall time, ms[1] = the device time (stream events: uploads and
 * kernels) of the last op_jpeg_decode or op_jpeg_stage that completed on `device`; OP_ERR_STATE
 * before the first. */
int op_jpeg_last_ms(int32_t device, double* ms);

/* ---- faces from a Haar cascade: cv2's detectMultiScale for new-format stump cascades (haar.py states
 * it in NumPy -- scales, grey, the integer bilinear pyramid, integrals, setWindow, the stages, the
 * visiting order with OpenCV's skip after a stage-0 failure, groupRectangles -- and the device equals
 * that statement bit for bit; parity with an OpenCV build is not pinned).  Per call: grey, one pyramid
 * launch for every layer of every frame, integrals (row scans, column scans), the cascade (stage 0
 * densely, the skip rule per row, the later stages over compacted survivor lists), and the candidates
 * come back as sorted keys; grouping runs on the host.  A batch is worked through in chunks bounded by
 * a byte budget for the pyramids. */
typedef struct op_haar op_haar;
typedef struct op_haar_params {
  double scale_factor;    /* finite, >= 1.01 */
  int32_t min_neighbors;  /* <= 0: the candidates ungrouped */
  int32_t min_w, min_h;   /* >= 1 */
  int32_t has_max;        /* 0: the frame's own size bounds the window */
  int32_t max_w, max_h;   /* >= 1 when has_max */
  int32_t max_candidates; /* per frame on the device; 0: 4096; at most 1048576 */
} op_haar_params;
#define OP_HAAR_MAX_SCALES 64
#define OP_HAAR_TIMES 5 /* op_haar_last_ms: total, grey, pyramid, integrals, cascade */
/* Uploads a cascade to `device`: a win_w x win_h window (3 .. 64 each), n_stages stages, stage s holding
 * stumps stage_first[s] .. stage_first[s + 1] - 1 (stage_first[0] = 0, ascending, n_stumps at the end)
 * and failing below stage_thr[s]; stump j: rects[j][3][4] as x, y, w, h inside the window, weights[j][3]
 * (a zero third weight: two rects), value < thr[j] ? left[j] : right[j].  OP_ERR_INVALID names the
 * field. */
int op_haar_create(int32_t device, int32_t win_w, int32_t win_h, int32_t n_stages, const int32_t* stage_first,
                   const float* stage_thr, int32_t n_stumps, const int32_t* rects, const float* weights,
                   const float* thr, const float* left, const float* right, op_haar** out);
int op_haar_destroy(op_haar* h);
/* n_frames host images of any mix of sizes: frame f is hw[2f] x hw[2f + 1] pixels of channels[f] (3: BGR,
 * 1: grey) bytes at bgr[f], row_stride[f] bytes per row.  rects [n_frames][cap][4] (x, y, w, h),
 * neighbours [n_frames][cap], count [n_frames], status [n_frames]: a frame with more candidates than
 * params->max_candidates, or more rectangles than cap, gets OP_ERR_CAPACITY and in count what it needs
 * (the candidates in the first case), the other frames are unaffected and the call returns OP_OK.
 * Validated before any device call (OP_ERR_INVALID, the message names the field): null pointers, a
 * scale_factor that is not finite or < 1.01, min / max sizes that are not positive, sides outside
 * 1 .. 16384, a row_stride below w channels, channels other than 1 and 3, more than 64 scales.  A frame
 * smaller than the window or exactly its size has no rectangle; n_frames == 0 is OP_OK. */
int op_haar_detect(const op_haar* h, int32_t n_frames, const uint8_t* const* bgr, const int32_t* hw,
                   const int64_t* row_stride, const int32_t* channels, const op_haar_params* params, int32_t cap,
                   int32_t* rects, int32_t* neighbours, int32_t* count, int32_t* status);
/* The same, ungrouped: the windows that pass every stage in (layer, y, x) order (neighbours is not
 * taken; min_neighbors is not read). */
int op_haar_candidates(const op_haar* h, int32_t n_frames, const uint8_t* const* bgr, const int32_t* hw,
                       const int64_t* row_stride, const int32_t* channels, const op_haar_params* params, int32_t cap,
                       int32_t* rects, int32_t* count, int32_t* status);
/* op_haar_detect on frames [first, first + n) of ctx's staged set, read in place on the context's
 * stream after its queued work: only tables are uploaded, only candidate keys come back.  The cascade
 * must live on the context's device. */
int op_haar_detect_staged(const op_haar* h, op_ctx* ctx, int32_t first, int32_t n, const op_haar_params* params,
                          int32_t cap, int32_t* rects, int32_t* neighbours, int32_t* count, int32_t* status);
/* One frame, every launch's output.  With pixels == NULL only the plan is returned (no device call):
 * *n_layers, layer_hw [64][2] (h, w), layer_scale [64].  Otherwise also, layer after layer: pixels
 * (h w bytes each), sum and sqsum ((h + 1) (w + 1) each) and the int8 result map over the step grid
 * (haar.result_map_np: n_stages passed, k failed stage k, -1 invalid, -2 skipped); cap[3] = the
 * elements pixels, sum / sqsum and map can hold (OP_ERR_CAPACITY when too few). */
int op_haar_probe(const op_haar* h, const uint8_t* bgr, int32_t fh, int32_t fw, int64_t row_stride, int32_t channels,
                  const op_haar_params* params, int32_t* n_layers, int32_t* layer_hw, float* layer_scale,
                  uint8_t* pixels, int32_t* sum, uint32_t* sqsum, int8_t* map, const int64_t* cap);
/* ms[OP_HAAR_TIMES] (stream events) of the last op_haar_detect, op_haar_candidates,
 * op_haar_detect_staged or op_haar_probe that completed on `device`: the whole call (uploads, kernels,
 * downloads), then the grey, pyramid, integral and cascade launches summed over its chunks;
 * OP_ERR_STATE before the first. */
int op_haar_last_ms(int32_t device, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* OPENPOSE_HIP_H */
