/* rtpose_mi355x.h — C-ABI of the MI355X-native realtime multi-person pose engine.
 *
 * This is the drop-in boundary for the ONE hot path of CMU's caffe_rtpose:
 *   float NCHW net input -> VGG-19+CPM conv stack -> ImResize -> Nms -> connectLimbs* -> joints
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference tree).  The reference consumes that path through the Caffe Net API
 * (examples/rtpose/rtpose.cpp:183-207, 1127-1166); a maintainer keeps rtpose.cpp's thread
 * structure and swaps those calls for the ones below.
 *
 * Conventions
 *   - plain C types only; caller owns every buffer it passes; all functions return 0 on
 *     success or a negative RTP_E* code and NEVER abort (the reference's glog CHECK /
 *     CUDA_CHECK abort the process, rtpose.cpp:208,247; common.hpp CUDA_CHECK).
 *   - an engine is single-owner and not thread-safe: one engine per GPU worker thread,
 *     exactly like one caffe::Net per processFrame thread (rtpose.cpp:1463-1472).
 *   - host buffers may be pageable or pinned; "_device" variants take HIP device pointers.
 *   - there is NO CPU fallback: without a gfx950 device rtp_engine_create fails with
 *     RTP_ENODEV.
 */
#ifndef RTPOSE_MI355X_H_
#define RTPOSE_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTP_OK 0
#define RTP_EINVAL (-22)   /* bad argument / bad configuration                       */
#define RTP_ENOMEM (-12)   /* host or device allocation failed                       */
#define RTP_ENODEV (-19)   /* no usable gfx950 device                                */
#define RTP_EIO (-5)       /* file could not be read / parsed                        */
#define RTP_EAGAIN (-11)   /* submit queue full / nothing to collect                 */
#define RTP_EHIP (-70)     /* a HIP runtime call failed (see rtp_last_error)         */
#define RTP_ERANGE (-34)   /* out-of-contract data (e.g. sample coordinate < 0)      */

#define RTP_MODEL_COCO_18 0 /* ModelDescriptorFactory::Type::COCO_18 (modelDescriptorFactory.cpp:30) */
#define RTP_MODEL_MPI_15 1  /* ModelDescriptorFactory::Type::MPI_15  (modelDescriptorFactory.cpp:6)  */

#define RTP_PREC_FP16 0 /* fp16 storage, MFMA f16 with fp32 accumulate: fastest, 2-2.6x OUTSIDE +-1e-3 */
#define RTP_PREC_FP32 1 /* fp32 storage, exact-f32 MFMA (parity path, 1/16 the MFMA rate)   */
#define RTP_PREC_MIXED 2 /* fp16 MFMA; the layers named by split_layers (default: the set whose fp16 rounding   *
                          * dominates the final-map error) also multiply the rounding errors of both operands:  *
                          * a_hi*W_hi + a_lo*W_hi + a_hi*W_lo into one fp32 accumulator.  On the 3x3 / 7x7      *
                          * layers the two corrections are ONE extra K chunk of MX-scaled fp8 MFMA (2 pass-     *
                          * times in all), on the 1x1 layers two more fp16 passes.  Reference arithmetic is     *
                          * fp32 throughout (base_conv_layer.cpp:257-280); this is the fastest mode that meets  *
                          * +-1e-3 on the maps.  rtp_calibrate_precision checks / widens the set on the loaded  *
                          * weights.                                                                             */
#define RTP_PREC_F16X3 3 /* every layer split: fp32-class accuracy at about 1/3 of the fp16 rate                 */

#define RTP_EXEC_GRAPH 0 /* default: the conv stack of one batch (~50 launches) is captured ONCE per     *
                          * (context, frames in the batch) into a hipGraph and replayed with one       *
                          * hipGraphLaunch; each frame's short post-processing chain + D2H is launched  *
                          * eagerly on the frame's own stream (rtp_collect waits for its frame only)    */
#define RTP_EXEC_EAGER 1 /* one HIP launch per kernel (diagnostics; per-stage event timing)            */

#define RTP_MAX_PEOPLE 96    /* RENDER_MAX_PEOPLE, include/rtpose/renderFunctions.h:6 */
#define RTP_MAX_NUM_PARTS 70 /* MAX_NUM_PARTS, rtpose.cpp:91                          */

typedef struct rtp_engine rtp_engine;

/* Replaces: flags + warmup() state (rtpose.cpp:50-72, 173-237). */
typedef struct rtp_config {
  unsigned int struct_size;/* sizeof(rtp_config) of the header rtp_config_default was COMPILED against (it writes  *
                            * it).  rtp_engine_create / rtp_plan_summary return RTP_EINVAL for any other value: a    *
                            * caller built against another version of this header (fields were appended in rounds     *
                            * 2-5) or one that skipped rtp_config_default is refused instead of being misread.        */
  int device_id;           /* --start_device + worker index (rtpose.cpp:1466)                     */
  int model;               /* RTP_MODEL_*; ignored when proto_path is given                        */
  const char* proto_path;  /* --caffeproto deploy prototxt, or NULL = built-in linevec net         */
  const char* weights_path;/* --caffemodel binary NetParameter, or NULL = synthetic (seed below)   */
  uint64_t synthetic_seed; /* deterministic He-scaled weights when weights_path == NULL            */
  int net_w, net_h;        /* --net_resolution, multiples of 16 (rtpose.cpp:65)                    */
  int num_scales;          /* --num_scales = blob N (rtpose.cpp:188, 1719)                          */
  float start_scale;       /* --start_scale -> ImResizeLayer::SetStartScale (rtpose.cpp:201)       */
  float scale_gap;         /* --scale_gap   -> ImResizeLayer::SetScaleGap   (rtpose.cpp:202)       */
                           /* The reference's flags are doubles and its producer sizes level i from the double
                            * start_scale - i * scale_gap (rtpose.cpp:359).  For the LEVEL SIZES (and the range check)
                            * these two floats — and rtp_set_scales' arguments — are read as the shortest decimal that
                            * rounds to the float (0.225f is 0.225, not 0.22499999404): the levels of
                            * rtp_preprocess_frame called with that decimal.  ImResize's crops use the floats as given. */
  int disp_w, disp_h;      /* --resolution: joints are returned in display coordinates (:1061)     */
  int precision;           /* RTP_PREC_*                                                            */
  int frames_in_flight;    /* >=1: frames that may be submitted before a collect is needed         */
  int batch_frames;        /* >=1: frames whose conv stacks share one launch sequence (0 = 1).     *
                            * The reference runs one frame (num_scales images) per Forward; with   *
                            * B > 1 the engine stages B submitted frames and runs the stack over   *
                            * B*num_scales images (bigger tiles fill the 256 CUs), then post-      *
                            * processes each frame on its own stream.  Per-frame results do not    *
                            * depend on B.  ceil(frames_in_flight / B) batches are in flight.       */
  int render;              /* 0: off.  1 + FLAGS_part_to_show: rtp_collect_rendered also returns the  *
                            * display image as render() (rtpose.cpp:270-299) draws it: 1 = the pose    *
                            * overlay (render_pose_*, renderFunctions.cu), 2.. = heat-map / PAF view   *
                            * part_to_show = render - 1 (that frame's resized map is then materialised) */
  int exec_mode;           /* RTP_EXEC_*: how a batch's ~45 launches reach the GPU.  Replaces the  *
                            * reference's per-call layer walk (net.cpp:544-556 ForwardFromTo).       */
  const char* split_layers;/* RTP_PREC_MIXED only; NULL = default set.  Comma-separated rules, each *
                            * "<pattern>[:w|:a|:x]": pattern = layer-name prefix, "*text" = name      *
                            * contains text, "@1x1" = every 1x1 layer, "@all"; ":w" splits only the  *
                            * weights, ":a" only the input activations, none = both; ":x" = both,    *
                            * with the corrections as fp16 passes instead of the fp8 chunk (three     *
                            * pass-times, no e4m3 range limits: what the calibration switches a      *
                            * group to when the fp8 corrections are not accurate enough).             */
  int keep_blobs;          /* 0 (default): blobs that only feed a fused consumer are not written (the     *
                            * convolutions in front of the three pooling layers pool in their epilogue):    *
                            * rtp_get_blob("conv1_2" / "conv2_2" / "conv3_4") then returns RTP_EINVAL —      *
                            * UNLIKE Net::blob_by_name, which has every blob.  1: every blob of the graph    *
                            * stays tappable, pooling runs as its own launch; same values either way.        */
  int calibrate_frames;    /* > 0 (RTP_PREC_MIXED only): rtp_engine_create ends with                         *
                            * rtp_calibrate_precision(e, NULL, calibrate_frames, calibrate_target, ...) on    *
                            * synthetic frames, i.e. the split set is checked — and widened if necessary —    *
                            * on the weights that were just loaded (net.cpp:750-803).                          *
                            * 0 (default): that check runs with ONE frame when weights_path != NULL (weights   *
                            * from a file: the default set was chosen on synthetic ones; ~2-3 s, a line on     *
                            * stderr if the set had to change) and not at all for synthetic weights.           *
                            * -1: never (the split set stays exactly rtp_config.split_layers / the default).   */
  float calibrate_target;  /* max |mixed - f16x3| / max |map| the calibration accepts (<= 0: 0.7e-3)         */
  int defer_weights;       /* 1: a RECEIVING replica of a one-time weight distribution: the engine is built      *
                            * (plan, arena, contexts) but no weights are read, generated, packed or uploaded —    *
                            * the arena stays zero and every entry that would run the net returns RTP_EINVAL      *
                            * until rtp_weight_blob_import / rtp_copy_weights_from has delivered another          *
                            * engine's packed weights (same plan: see there); the launch graphs are captured      *
                            * then.  Saves the N-1 reads + packs of N replicas (rtpose.bin --share_weights,       *
                            * bench.py --broadcast_weights).  No calibration runs on such an engine: create it    *
                            * with the split set the source engine ended up with (rtp_get_split_layers).          */
} rtp_config;

/* Fill cfg with the reference's flag defaults (rtpose.cpp:50-72): COCO, 656x368, 1 scale,
 * start_scale 1, scale_gap 0.3, 1280x720, RTP_PREC_MIXED, 2 frames in flight, graph replay — and
 * struct_size.  Every rtp_config must start here. */
int rtp_config_default(rtp_config* cfg);

/* Replaces: new Net<float>(proto, TEST) + CopyTrainedLayersFrom + Reshape + dry run
 * (rtpose.cpp:183-191, 233; net.cpp:49, 750-803). */
int rtp_engine_create(const rtp_config* cfg, rtp_engine** out);
void rtp_engine_destroy(rtp_engine* e);

/* Replaces: NmsLayer::GetNumParts/GetMaxPeaks (nms_layer.hpp:11-44, rtpose.cpp:194-207) and
 * the resized_map blob shape.  heat_channels = channels of concat_stage7 (57 COCO / 44 MPI). */
int rtp_engine_info(const rtp_engine* e, int* num_parts, int* max_peaks, int* heat_channels,
                    int* low_w, int* low_h);

/* Replaces: the global.* thresholds written by warmup() and the UI thread
 * (rtpose.cpp:212-226) and NmsLayer::SetThreshold (rtpose.cpp:1145).
 * connect_inter_min_above_threshold < 0 is refused (RTP_EINVAL, nothing changes): it would accept
 * pairs with no sample above the threshold, whose score is 0 / 0. */
int rtp_set_thresholds(rtp_engine* e, float nms_threshold, float connect_inter_threshold,
                       int connect_inter_min_above_threshold, int connect_min_subset_cnt,
                       float connect_min_subset_score);
int rtp_get_thresholds(const rtp_engine* e, float* nms_threshold, float* connect_inter_threshold,
                       int* connect_inter_min_above_threshold, int* connect_min_subset_cnt,
                       float* connect_min_subset_score);

/* Replaces: ImResizeLayer::SetStartScale/SetScaleGap (imresize_layer.hpp:11-45).  Every level s = start_scale - i * scale_gap
 * (i < num_scales) must be positive and its 16-aligned size 16 * ceil(net * s / 16) must fit the net input — what the producer CHECKs
 * (rtpose.cpp:363-364) — else RTP_EINVAL and the engine keeps its previous scales; the same test guards rtp_engine_create and
 * rtp_preprocess_frame.  start_scale < 1 is in contract: ImResize then crops every scale incl. the first (imresize_layer.cu:110-113).
 * s is computed in double from the shortest decimals that round to the two floats (see rtp_config.scale_gap). */
int rtp_set_scales(rtp_engine* e, float start_scale, float scale_gap);

/* ---- the per-frame hot loop (rtpose.cpp:1127-1166) ---------------------------------- */

/* Replaces: cudaMemcpy H2D into blobs()[0]->mutable_gpu_data() + ForwardFrom(0) + the
 * heatmap/peaks read-back + connectLimbs*().  Asynchronous: returns once the frame is
 * enqueued on one of the engine's frame contexts.  nchw_input: num_scales x 3 x net_h x net_w
 * floats, the output of process_and_pad_image (rtpose.cpp:239-269).  RTP_EAGAIN when all
 * frames_in_flight contexts are busy (collect first). */
int rtp_submit(rtp_engine* e, const float* nchw_input_host, uint64_t tag);
int rtp_submit_device(rtp_engine* e, const float* nchw_input_device, uint64_t tag);

/* Same frame path, but from the DECODED frame: u8 BGR HWC (any size) -> display-fit cubic warp ->
 * INTER_AREA scale pyramid -> u8/256-0.5 -> centre pad, all on the device (what the producer thread
 * does with OpenCV in rtpose.cpp:322-368), bit-identical to rtp_preprocess_frame.  *frame_scale
 * receives Frame::scale (for rtp_format_json). */
int rtp_submit_frame(rtp_engine* e, const unsigned char* bgr_host, int w, int h, uint64_t tag, float* frame_scale);
/* Parity tap for the device pre-processing alone. */
int rtp_debug_preprocess(rtp_engine* e, const unsigned char* bgr_host, int w, int h, float* net_input_host,
                         unsigned char* display_bgr_host, float* frame_scale);

/* rtp_collect + the display-resolution u8 BGR frame with the pose overlay: the image the reference
 * passes to cv::imwrite under --write_frames (rtpose.cpp:1179-1199 render, :1286-1293 float -> u8),
 * without the cv::putText overlays (= --no_text).  Needs rtp_config.render = 1 and rtp_submit_frame. */
int rtp_collect_rendered(rtp_engine* e, uint64_t* tag, float* joints_host, int* num_people, unsigned char* display_bgr_host);

/* Launch a partially filled batch now (batch_frames > 1: end of stream or a latency-sensitive
 * caller).  rtp_collect does this by itself when the oldest frame sits in an unlaunched batch. */
int rtp_flush(rtp_engine* e);

/* Blocks until the OLDEST submitted frame is finished; returns its tag, the number of people
 * (<= RTP_MAX_PEOPLE) and joints[num_people][num_parts][3] = (x, y, score) in display
 * coordinates — the array connectLimbs*() fills (rtpose.cpp:1051-1073).  joints must hold
 * RTP_MAX_PEOPLE*num_parts*3 floats.  RTP_EAGAIN if nothing is in flight. */
int rtp_collect(rtp_engine* e, uint64_t* tag, float* joints, int* num_people);

/* Number of frames submitted and not yet collected. */
int rtp_in_flight(const rtp_engine* e);

/* ---- parity taps (the Net::blob_by_name surface rtpose.cpp uses, :1093-1094, 1149-1150) - */

/* Run the conv stack only; lowres receives concat_stage7 as num_scales x C x h x w fp32. */
int rtp_forward_heatmaps(rtp_engine* e, const float* nchw_input_host, float* lowres_host);
/* ImResizeLayer::Forward_gpu on caller data: lowres (num_scales x C x h x w) -> resized (C x net_h x net_w). */
int rtp_resize(rtp_engine* e, const float* lowres_host, float* resized_host);
/* The PRODUCTION post-processing as a parity tap: rtp_submit/rtp_collect never materialise the
 * 55 MB resized map — NMS builds the resized rows of each 8-row strip in LDS and the PAF samples /
 * centroid windows are evaluated from the low-res maps on demand, with the arithmetic of
 * imresize_layer.cu, so the results equal rtp_resize -> rtp_nms -> rtp_connect bit for bit.
 * lowres: [num_scales][heat_channels][low_h][low_w]; peaks in/out like rtp_nms (may be NULL). */
int rtp_post_from_lowres(rtp_engine* e, const float* lowres_host, float* peaks_host, float* joints_host, int* num_people);

/* render() of rtpose.cpp:270-299 on caller data (parity tap of the renderer, and the --part_to_show views of --write_frames):
 * display_bgr / out_bgr = u8 BGR HWC at cfg.disp_w x cfg.disp_h (what the producer's canvas holds, rtpose.cpp:349, and what the
 * post-processing thread makes of the rendered canvas, :1287-1296); joints [num_people][num_parts][3] in display coordinates.
 * part_to_show = FLAGS_part_to_show: 0 = pose overlay (render_pose_coco_parts / render_pose_29parts; googly = the GUI's
 * googly-eyes toggle, COCO only), 1..parts = one heat map, parts+1 (COCO) = all part maps, above = PAF views
 * (render_coco_aff).  resized_host (heat_channels x net_h x net_w, rtp_resize's output) is only read when part_to_show != 0.
 * RTP_EINVAL for a part_to_show outside the model's maps (the reference would read past its blob). */
int rtp_render(rtp_engine* e, const unsigned char* display_bgr, const float* joints, int num_people, int part_to_show, int googly,
               const float* resized_host, unsigned char* out_bgr);

/* NmsLayer::Forward_gpu on caller data: resized (C x H x W) -> peaks (num_parts x (max_peaks+1) x 3).
 * peaks is IN/OUT: slots the kernel does not write keep the caller's contents. */
int rtp_nms(rtp_engine* e, const float* resized_host, float* peaks_host);
/* connectLimbs / connectLimbsCOCO on caller data -> joints, *num_people. */
int rtp_connect(rtp_engine* e, const float* resized_host, const float* peaks_host, float* joints,
                int* num_people);
/* Full synchronous frame with every intermediate returned (any pointer may be NULL). */
int rtp_forward_debug(rtp_engine* e, const float* nchw_input_host, float* lowres_host,
                      float* resized_host, float* peaks_host, float* joints, int* num_people);
/* Net::blob_by_name(name)->cpu_data() for any conv-stack blob of the LAST synchronous forward
 * (rtp_forward_heatmaps / rtp_forward_debug), as N x C x H x W fp32.  shape[4] out. */
int rtp_get_blob(rtp_engine* e, const char* name, float* out_host, size_t out_capacity_floats,
                 int shape[4]);
/* rtp_get_blob for a WHOLE batch: the named blob as the last batch that ran on batch context `ctx` (0 .. frames_in_flight /
 * batch_frames - 1) left it in that context's buffers — nframes x num_scales images, frame j's at [j * num_scales, (j + 1) *
 * num_scales); shape[0] = nframes * num_scales.  rtp_submit* fills context after context, a batch is launched when its last slot is
 * filled (or by rtp_flush / a blocking rtp_collect), through the captured graph in RTP_EXEC_GRAPH.  name: every name rtp_get_blob
 * accepts; the low-res blob (what the post-processing chains of all frames of the batch read); the graph's input blob (the
 * batch's slice of the staged input tensor, i.e. what the conv stack consumed).  tags_out (batch_frames entries, may be NULL) /
 * nframes_out (may be NULL) receive the tags of that batch's frames in slot order and their count; a one-frame tap
 * (rtp_forward_heatmaps / rtp_forward_debug, context 0) counts as a batch of one frame.  out_host == NULL: shape, tags and count
 * only.  Idle engines only.  RTP_EINVAL for a context outside the engine's, for one that has not run a batch since the engine
 * was created or re-planned, and for the input blob of a batch that read the caller's tensor in place (rtp_submit_device, eager,
 * batch_frames 1).  The buffers are returned as they stand: whatever ran on the context since (a tap on context 0,
 * rtp_profile_steps) shows. */
int rtp_get_batch_blob(rtp_engine* e, int ctx, const char* name, float* out_host, size_t out_capacity_floats, int shape[4],
                       uint64_t* tags_out, int* nframes_out);

/* ---- weights / graph (net.cpp:750-803, caffe.proto:6-22,64-95,310-330) ------------------ */
int rtp_num_conv_layers(const rtp_engine* e);
int rtp_conv_layer_info(const rtp_engine* e, int i, char* name, int name_len, int* cin, int* cout, int* k);
/* Weights in Caffe blob order: w[cout][cin][k][k], b[cout] (base_conv_layer.cpp:135-175). */
int rtp_get_conv_weights(const rtp_engine* e, int i, float* w, float* b);
int rtp_set_conv_weights(rtp_engine* e, int i, const float* w, const float* b);
/* Serialise the current weights as a binary caffe NetParameter (.caffemodel). */
int rtp_save_caffemodel(const rtp_engine* e, const char* path);
/* Emit the engine's layer graph as deploy-prototxt text. */
int rtp_save_prototxt(const rtp_engine* e, const char* path);

/* Load-time precision calibration (where trained weights arrive: CopyTrainedLayersFrom, net.cpp:750-803).  The default
 * split set of RTP_PREC_MIXED was chosen on synthetic weights; this measures it on the LOADED weights: nframes sample frames
 * (frames_host: nframes x num_scales x 3 x net_h x net_w floats as rtp_submit takes them, or NULL = seeded synthetic frames)
 * run through RTP_PREC_F16X3 (every layer split: 1e-5-class reference) and through the current mixed plan;
 * err = max |mixed - f16x3| / max |f16x3| over the final maps.  While err > target (<= 0: 0.7e-3) the layer group whose
 * promotion lowers the error most joins the split set and the engine is re-planned (arena, packed weights, graphs); if every
 * group is in and the target is still missed, groups switch their corrections from the fp8 chunk to fp16 passes (":x": e4m3
 * operands saturate beyond +-112 in the activations), best first; as a last resort the engine switches to RTP_PREC_F16X3.  rules_out (may be NULL) receives the
 * final rule list ("@f16x3" after the fallback), err_before / err_after the measured errors.  Idle engine only; seconds. */
int rtp_calibrate_precision(rtp_engine* e, const float* frames_host, int nframes, float target, char* rules_out, size_t rules_len,
                            float* err_before, float* err_after);
const char* rtp_calibration_report(const rtp_engine* e); /* what the last calibration tried and chose, as text */
/* The rule list the engine runs (after calibration: the widened one) and its precision mode.  RTP_ERANGE (and an empty buf) if the list does
 * not fit buflen bytes incl. the NUL: a truncated list would describe another plan. */
int rtp_get_split_layers(const rtp_engine* e, char* buf, size_t buflen, int* precision);

/* Caller-owned device buffers on the engine's device (replaces blobs()[0]->mutable_gpu_data() as a caller-filled H2D target,
 * rtpose.cpp:1131): what rtp_submit_device reads.  Freed by rtp_device_free or with the engine. */
int rtp_device_alloc(rtp_engine* e, size_t bytes, void** dptr);
int rtp_device_free(rtp_engine* e, void* dptr);
int rtp_device_upload(rtp_engine* e, void* dst_device, const void* src_host, size_t bytes);
int rtp_device_synchronize(rtp_engine* e);

/* The CPUs local to a device ("0-31,128-159": sysfs local_cpulist of its PCI function) for the worker thread that feeds it; returns
 * the string length, 0 when the platform does not expose it. */
int rtp_device_local_cpus(int device_id, char* buf, size_t buflen);

/* One-time weight distribution between replicas (optional; the reference reads the .caffemodel once per GPU thread,
 * rtpose.cpp:183-184).  Blob = the PACKED weight arena + the Caffe-layout floats of an idle engine; the receiver must have
 * the same plan (model, resolution, batch, precision, split set).  rtp_copy_weights_from: device to device (hipMemcpyPeer,
 * xGMI) between two engines of one process. */
long rtp_weight_blob_bytes(const rtp_engine* e);
int rtp_weight_blob_export(rtp_engine* e, void* host, size_t capacity);
int rtp_weight_blob_import(rtp_engine* e, const void* host, size_t bytes);
int rtp_copy_weights_from(rtp_engine* dst, rtp_engine* src);

/* ---- host-side pieces of the path (no GPU needed) ---------------------------------------- */
/* ModelDescriptor tables (modelDescriptorFactory.cpp:25-26,52-53). limb_seq/map_idx: 2*num_limbs ints. */
int rtp_model_tables(int model, int* num_parts, int* num_limbs, int* limb_seq, int* map_idx);
/* Default thresholds chosen by warmup() (rtpose.cpp:212-226). */
int rtp_default_thresholds(int model, float* nms_threshold, float* connect_inter_threshold,
                           int* connect_inter_min_above_threshold, int* connect_min_subset_cnt,
                           float* connect_min_subset_score);
/* process_and_pad_image (rtpose.cpp:239-269): uint8 BGR HWC -> float planar, centre zero-pad. */
int rtp_process_and_pad_image(float* target, const unsigned char* bgr, int ow, int oh, int tw, int th,
                              int normalize);
/* JSON body exactly as displayFrame writes it (rtpose.cpp:1394-1415). Returns bytes written
 * (excluding the NUL) or RTP_ERANGE if buf is too small. frame_scale = Frame::scale. */
long rtp_format_json(char* buf, size_t buflen, const float* joints, int num_people, int num_parts,
                     float frame_scale);
/* Producer-side pre-processing (row a1; rtpose.cpp:322-368, 474-518).  The OpenCV primitives are
 * restated from OpenCV's published algorithms (OpenCV is absent here and unpinned by the
 * reference): rtp_warp_display = warpAffine(M = diag(fit scale), INTER_CUBIC, BORDER_CONSTANT 0),
 * rtp_resize_area = cv::resize(INTER_AREA); rtp_preprocess_frame = the whole producer step ->
 * net input (num_scales x 3 x net_h x net_w) + Frame::scale. */
double rtp_display_fit_scale(int ow, int oh, int disp_w, int disp_h);
int rtp_resize_area(const unsigned char* bgr, int sw, int sh, unsigned char* out, int dw, int dh);
int rtp_warp_display(const unsigned char* bgr, int sw, int sh, unsigned char* out, int disp_w, int disp_h,
                     double* scale_out);
int rtp_preprocess_frame(const unsigned char* bgr, int w, int h, int disp_w, int disp_h, int net_w, int net_h,
                         int num_scales, double start_scale, double scale_gap, float* net_input,
                         unsigned char* display_bgr, float* frame_scale);
/* cv::imread(path, IMREAD_COLOR) (rtpose.cpp:323) without OpenCV: baseline and progressive JPEG
 * (libjpeg's default decode arithmetic, bit-exact), PNG (zlib), binary PPM (P6), 24-bit BMP -> BGR HWC.  out_bgr may be
 * NULL to query the size.  rtp_decode_image: the same for an encoded PNG/JPEG byte string.
 * rtp_synth_frame: frame `index` of the procedural test video. */
int rtp_load_image(const char* path, unsigned char* out_bgr, size_t capacity, int* w, int* h);
int rtp_decode_image(const unsigned char* bytes, size_t n, unsigned char* out_bgr, size_t capacity, int* w, int* h);
const char* rtp_codec_last_error(void);
/* cv::imwrite(name, img, {CV_IMWRITE_JPEG_QUALITY, quality}) (rtpose.cpp:1367-1381): libjpeg's default
 * baseline 4:2:0 encoder restated, byte-identical files.  Returns the size in bytes (out may be NULL
 * to query it) or a negative RTP_E* code. */
long rtp_encode_jpeg(const unsigned char* bgr, int w, int h, int quality, unsigned char* out, size_t capacity);
/* An 8-bit YUV frame (no reference counterpart: cv::VideoCapture hands the producer BGR): luma of pixel (x, y) is the byte
 * y[y*y_stride + x], its chroma samples u / v[(y >> chroma_shift_y)*uv_stride + (x >> chroma_shift_x)*uv_pixel_stride].  A chroma
 * plane has (width + sx) >> sx by (height + sy) >> sy samples, so odd sizes are in contract.  I420: three planes, shifts 1 1,
 * uv_pixel_stride 1 (YV12: u and v exchanged); NV12: v = u + 1, uv_pixel_stride 2 (NV21: u = v + 1); 4:2:2: shifts 1 0; 4:4:4: 0 0.
 * The pointers are host memory for rtp_convert_yuv / rtp_submit_frame_yuv and device memory for the _device entries. */
#define RTP_YUV_BT601_LIMITED 0 /* ITU-R BT.601, Y 16..235, C 16..240, in the integer arithmetic of rtp_convert_yuv */
typedef struct rtp_yuv_view {
  unsigned int struct_size;     /* sizeof(rtp_yuv_view); any other value -> RTP_EINVAL */
  int matrix;                   /* RTP_YUV_BT601_LIMITED; anything else -> RTP_EINVAL */
  void* y; void* u; void* v;    /* u == v == NULL: luma only (Y4M "mono"); exactly one NULL -> RTP_EINVAL */
  int width, height;            /* luma size, >= 1 */
  int chroma_shift_x, chroma_shift_y;  /* 0 or 1 each: 4:2:0 = 1,1; 4:2:2 = 1,0; 4:4:4 = 0,0; (0,1) is refused */
  long y_stride;                /* bytes between luma rows, >= 0 */
  long uv_stride;               /* bytes between chroma rows (same for u and v), >= 0 */
  long uv_pixel_stride;         /* 1 = planar (I420/YV12), 2 = interleaved (NV12: v = u + 1, NV21: u = v + 1) */
} rtp_yuv_view;
/* The view as packed u8 BGR HWC (width x height x 3 bytes; capacity in bytes), BT.601 limited range, integers only:
 *   c = 298 (Y - 16), d = U - 128, e = V - 128 (d = e = 0 without chroma)
 *   R = clamp255((c + 409 e + 128) >> 8), G = clamp255((c - 100 d - 208 e + 128) >> 8), B = clamp255((c + 516 d + 128) >> 8)
 * (arithmetic shift).  This is what rtp_video_read makes of a Y4M frame, and what the GPU entries below compute bit for bit.
 * RTP_EINVAL + rtp_codec_last_error for a view that fails the field checks or a capacity below the image. */
int rtp_convert_yuv(const rtp_yuv_view* host, unsigned char* bgr_out, size_t capacity);
/* The other direction: packed u8 BGR (w x h, rows row_stride >= 3 w bytes apart) -> the planes dst_host describes (same size; planar or
 * interleaved, 4:2:0 / 4:2:2 / 4:4:4 or luma only, any pitches; pitch padding is not written).  BT.601 limited range, integers only,
 * arithmetic shifts:
 *   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel;
 *   U = ((-38 R' - 74 G' + 112 B' + 128) >> 8) + 128, V = ((112 R' - 94 G' - 18 B' + 128) >> 8) + 128 per chroma sample, where
 *   (R', G', B') is the rounded mean of the sample's cell: (sum + 2) >> 2 of 2 x 2 pixels, (sum + 1) >> 1 of 2 x 1, the pixel itself at
 *   4:4:4; coordinates are clamped to the last column / row, so an odd edge cell repeats its last pixel.
 * Y stays in 16..235 and U, V in 16..240 without a clamp; rtp_convert_yuv of the 4:4:4 result is within 3 of every source channel.
 * This is the definition of every YUV output of the library: the GPU entries below write these bytes.  RTP_EINVAL +
 * rtp_codec_last_error for a view that fails the field checks of rtp_convert_yuv, a size other than the view's, or row_stride < 3 w. */
int rtp_convert_bgr_to_yuv(const unsigned char* bgr, int w, int h, long row_stride, const rtp_yuv_view* dst_host);
/* Bytes of a w x h frame's planes without pitches (Y, U, V; chroma planes of (w + 1) / 2 columns and, at 4:2:0, (h + 1) / 2 rows):
 * chroma = 420, 422, 444 or 400 (luma only).  Host only; 0 for a size below 1 or any other chroma. */
size_t rtp_yuv_bytes(int w, int h, int chroma);
/* Stream writers for the two container-less formats rtp_video_open reads (cv::VideoWriter has no counterpart in the reference, which
 * stops at --write_frames).  Append only, never seeking: path may be a FIFO that feeds an encoder.  RTP_VIDEO_Y4M: 8-bit 4:2:0
 * ("C420jpeg": the chroma samples are centre sited box averages), one "FRAME" line + the planes without pitches per
 * rtp_video_write_yuv (refused for a view of another size or chroma); RTP_VIDEO_MJPEG: the JPEG files of rtp_video_write_jpeg one after
 * the other.  A write of the other kind is refused (RTP_EINVAL, nothing written).  rtp_video_finish flushes, closes and frees the
 * writer whatever it returns: RTP_EIO if any write to the stream failed.  RTP_EIO from rtp_video_create: the file cannot be created. */
#define RTP_VIDEO_Y4M 1
#define RTP_VIDEO_MJPEG 2
typedef struct rtp_video_out rtp_video_out;
int rtp_video_create(const char* path, int w, int h, int kind, int fps_num, int fps_den, rtp_video_out** out);
int rtp_video_write_yuv(rtp_video_out* o, const rtp_yuv_view* host);
int rtp_video_write_jpeg(rtp_video_out* o, const unsigned char* bytes, size_t n);
int rtp_video_finish(rtp_video_out* o);
/* cv::VideoCapture(path) (rtpose.cpp:402-411, 431) for the container-less formats decodable here:
 * Y4M (YUV4MPEG2, 8 bit) and raw MJPEG streams.  nframes may be NULL; rtp_video_read returns
 * RTP_EAGAIN at the end of the stream. */
typedef struct rtp_video rtp_video;
int rtp_video_open(const char* path, rtp_video** v, int* w, int* h, int* nframes);
int rtp_video_read(rtp_video* v, unsigned char* out_bgr, size_t capacity);
void rtp_video_close(rtp_video* v);
/* 420, 422, 444 or 400 (luma only) for a Y4M stream, 0 for anything else (MJPEG, NULL). */
int rtp_video_chroma(const rtp_video* v);
/* rtp_video_read without the colour conversion: the next Y4M frame as a view into the reader's own buffer (planar, pitches =
 * plane widths), valid until the next read or close.  rtp_convert_yuv of it = what rtp_video_read would have returned.
 * RTP_EAGAIN at the end of the stream; RTP_EINVAL for an MJPEG stream (nothing is consumed). */
int rtp_video_read_yuv(rtp_video* v, rtp_yuv_view* out);
/* rtp_video_read without the decoding: the byte range (SOI .. EOI) of the next frame of a raw MJPEG stream, inside the reader's own
 * copy of the file, valid until close.  rtp_decode_image of it = what rtp_video_read would have returned.  RTP_EAGAIN at the end
 * of the stream; RTP_EINVAL for a Y4M stream (nothing is consumed). */
int rtp_video_read_jpeg(rtp_video* v, const unsigned char** bytes, size_t* n);
int rtp_synth_frame(unsigned char* out_bgr, int w, int h, int index, uint64_t seed);

/* Parse a deploy prototxt and report the graph it describes (for tests / tools). */
int rtp_prototxt_summary(const char* path, int* num_layers, int* num_conv, int* num_parts,
                         int* max_peaks, float* nms_threshold, int* heat_channels);

/* ---- diagnostics ------------------------------------------------------------------------- */
const char* rtp_last_error(const rtp_engine* e); /* never NULL; also valid for e == NULL (create errors) */
const char* rtp_version(void);
/* Per-stage device time of the last collected frame, ms: [0]=conv stack [1]=resize [2]=nms
 * [3]=connect [4]=total (the reference's "CNN time / Connect time" VLOGs, rtpose.cpp:1147,1168). */
int rtp_last_stage_ms(const rtp_engine* e, float ms[5]);
/* Diagnostics: each plan step alone on the chip (back-to-back launches at the full batch).
 * Returns the number of steps written (same order as rtp_plan_summary's "step" lines). */
int rtp_profile_steps(rtp_engine* e, int iters, float* ms_per_step, double* gflop_per_step, int cap);

/* Time `iters` launches of the dominant conv kernel (Mconv 7x7 128->128 pair of stage 2) with
 * HIP events on the engine's stream; returns avg ms per launch and the algorithmic FLOPs of one
 * launch.  Used by bench.py for the roofline line. */
int rtp_bench_dominant_conv(rtp_engine* e, int iters, float* avg_ms, double* flops_per_launch);
/* In-situ timing of the dominant kernel class (every paired 7x7 128->128 launch of every frame):
 * enable = 1/0 switches it on/off (resetting the totals on a change), 2 = on AND reset, enable < 0 only
 * reads; the mode can only change on an idle engine.  While on, batches are launched eagerly (no graph
 * replay) and each such launch of a FULL batch sits between a HIP event pair recorded on the stream it
 * runs on (events without the system-scope fence: time stamps only); the totals are the pairs' elapsed times.  Submit one batch at a time (collect it before the
 * next) and a pair brackets its launch alone on the chip — what a profiler's kernel trace reports.
 * Call with an idle engine to harvest.  (Round 2 compared wall-clock stamps of workgroups on different
 * XCDs; their clocks are not synchronised on every box.) */
int rtp_kernel_timing(rtp_engine* e, int enable, double* total_ms, long* launches, double* flops_per_launch);
/* The same totals split by the MFMA pass-times of the launch: 1 = plain fp16 layer, 2 = fp16 + one fp8 error-compensation
 * chunk per channel group (RTP_PREC_MIXED on 3x3 / 7x7 layers), 3 = three fp16 passes (RTP_PREC_F16X3); index 0 is unused. */
int rtp_kernel_timing_by_passes(const rtp_engine* e, double ms[4], long launches[4]);
/* enable = 3 in rtp_kernel_timing: on AND reset with an event pair around EVERY step of the plan (all convolution launches, the
 * branch-tail launches, conv1_1), not only the dominant class — its totals keep their meaning.  rtp_kernel_timing_steps then returns,
 * per plan step i (the order of rtp_plan_summary's "step" lines), the summed milliseconds and the number of launches timed; return
 * value = number of steps (fill at most `cap`).  bench.py groups them into kernel classes (`roofline.classes`). */
int rtp_kernel_timing_steps(const rtp_engine* e, double* ms, long* launches, int cap);
/* An UNPROFILED account of when the engine had work on the GPU (rocprofv3's timeline carries the tracer's own overhead).  enable = 1:
 * on + reset (idle engine only), 0: off, -1: read.  While on, rtp_collect reads — from events the per-frame path records anyway —
 * {kind, start_ms, end_ms} triples since the switch-on: kind 0 = one batch on its conv stream, from the staging of its first input to
 * the end of its conv stack; kind 1 = one frame's post-processing chain incl. the D2H of its joints.  Returns the number of triples
 * (at most `cap` are copied to `spans`, which may be NULL). */
int rtp_busy_probe(rtp_engine* e, int enable, float* spans, int cap);
/* What the probes above could not record since the engine was created: out[0] = launches rtp_kernel_timing wanted to time while its table
 * of event pairs (4096 between two harvests) was full, out[1] = frames whose rtp_busy_probe spans fell beyond its 65536-triple cap,
 * out[2] = frames the busy probe skipped because their batch ran as one whole-batch graph replay (no per-frame events there).  A
 * measurement that reads non-zero counts here is truncated and must say so (bench.py refuses to print a roofline from it). */
int rtp_probe_dropped(const rtp_engine* e, long out[3]);
/* Kernel RESIDENCY without a profiler: while on, thread 0 of every workgroup of every kernel of the per-frame path (device pre-processing,
 * conv stack, ImResize+Nms, connect) folds the chip's 100 MHz wall clock into a per-launch slot — first workgroup start, last workgroup
 * end.  enable = 1: on + reset (idle engine only; the batch graphs are re-captured with the slots), 0: off, -1: harvest + read.  spans:
 * {slot, start_us, end_us} triples; slot < 64 = plan step (rtp_plan_summary order), 64 + 8 j + k = frame j's strip / write / pairs / match /
 * assemble kernel, 200 + 2 j + k = frame j's warp / area-pad kernel.  1 - union(spans) / wall = the share of the time with NO kernel on the
 * chip (bench.py `idle_frac_kernel_stamps`).  No reference counterpart (measurement only).  Returns the number of triples. */
int rtp_stamp_probe(rtp_engine* e, int enable, float* spans, int cap);
/* Which of the engine's streams share a hardware queue of the HIP runtime, MEASURED (idle engine only, measurement only).  The engine's
 * distinct streams are numbered context by context: a context's conv stream, then the chain streams of its frames that have one.
 * owner[k] = 256 * context + frame of stream k (frame 0 = the conv stream); the last stream is the legacy stream, on which the engine's
 * synchronous hipMemset / hipMemcpy calls run: owner -1.  With reps >= 1 and ratio != NULL every pair (a, b) is timed
 * `reps` times: a one-workgroup kernel that waits 200 us on the chip's wall clock runs on both streams at once, and
 * ratio[a * n + b] = median(first start .. last end of the pair) / (one wait alone): about 1 = side by side on different queues, about 2 =
 * one waited for the other on the same queue.  opens[c] (may be NULL) = batches opened on context c since creation.  Returns n, the
 * number of streams; fills the arrays only when cap >= n (opens: the first min(opens_cap, contexts) entries), and times nothing when
 * reps = 0 or ratio = NULL. */
int rtp_debug_stream_queues(rtp_engine* e, int reps, int* owner, float* ratio, int cap, long* opens, int opens_cap);
/* Host float -> OCP e4m3 (round to nearest even, clamped to +-448): how the fp8 weight copies of split layers are made. */
int rtp_debug_f32_to_e4m3(const float* in, unsigned char* out, int n);

/* Survivors of the PAF test (temp.size(), rtpose.cpp:950) and accepted connections
 * (connection_k.size(), :980) per limb for the last synchronous frame; arrays of num_limbs ints. */
int rtp_debug_connect_stats(rtp_engine* e, int* cand_count, int* conn_count);

/* Host-only weight utilities.  rtp_synth_weights: the deterministic generator behind
 * synthetic_seed (w[cout][cin][k][k], b[cout]).  rtp_write_synthetic_caffemodel: the same weights
 * for every conv of the built-in linevec net as a binary NetParameter.  rtp_caffemodel_layer:
 * read a .caffemodel (new `layer` or V1 `layers`) — index < 0 returns the layer count. */
int rtp_synth_weights(uint64_t seed, const char* layer_name, int cout, int cin, int k, float* w, float* b);
int rtp_write_synthetic_caffemodel(int model, uint64_t seed, const char* path);
/* The built-in linevec graph (what proto_path == NULL uses) as deploy-prototxt text. */
int rtp_write_builtin_prototxt(int model, const char* path);
int rtp_caffemodel_layer(const char* path, int index, char* name, int name_len, int* num_blobs,
                         long* count0, long* count1, float* head0);

/* Build the execution plan for cfg without touching a device and describe it as text (tile
 * configuration per layer, L1/L2 pairing, arena sizes; `postproc strip_rows R nstrips S max_rows M`:
 * the strip height of the fused ImResize+Nms kernel, which halves on wide nets, its strips per part
 * and the rows of the connect tables).  Readers select lines by their first word.
 * Returns bytes written or a negative code. */
long rtp_plan_summary(const rtp_config* cfg, char* buf, size_t buflen);

/* ---- frames already in GPU memory (no reference counterpart: the producer's OpenCV frames live on the host) ---------- */

/* A u8 frame in device memory: channel c of pixel (x, y) is the byte at data + y*row_stride + x*pixel_stride + channel_offset[c].
 * HWC BGR: pixel_stride 3, offsets {0, 1, 2}; RGB: {2, 1, 0}; BGRA / RGBA: pixel_stride 4; planar CHW RGB of plane stride P:
 * pixel_stride 1, offsets {2P, P, 0}; a crop of a larger image: its first pixel as data, the larger image's row_stride. */
typedef struct rtp_frame_view {
  unsigned int struct_size;   /* sizeof(rtp_frame_view); any other value -> RTP_EINVAL */
  void* data;                 /* device memory on cfg.device_id (const for submit, written by collect) */
  int width, height;
  long row_stride;            /* bytes between rows, >= 0 */
  long pixel_stride;          /* bytes between neighbouring pixels of a row, >= 1 (3 BGR, 4 BGRA, 1 planar) */
  long channel_offset[3];     /* byte offsets of B, G, R from a pixel's address (planar RGB: 2*plane, plane, 0) */
} rtp_frame_view;

/* = rtp_submit_frame on the pixels the view describes, read on the GPU.  `stream` (a hipStream_t of the
 * producer, may be NULL): the engine reads the frame only after the work queued on `stream` so far, and work
 * queued on `stream` after this call returns runs only after the engine has finished reading the frame.
 * NULL: the frame is complete now and stays unmodified until the rtp_collect* of `tag` returns.
 * Every view is checked on the host before anything is launched (RTP_EINVAL + rtp_last_error, the engine stays
 * usable): struct_size, sizes >= 1, strides and offsets >= 0, data = device memory of cfg.device_id
 * (hipPointerGetAttributes: host, pinned host and another device's memory are refused), every addressed byte
 * inside the allocation that holds data (hipMemGetAddressRange), a stream that is not capturing, and a
 * configuration in which the device pre-processing runs (see rtp_debug_preprocess).  A process that also uses
 * PyTorch must let ONE HIP runtime serve both: import torch before loading this library. */
int rtp_submit_frame_device(rtp_engine* e, const rtp_frame_view* frame, void* stream, uint64_t tag, float* frame_scale);

/* = rtp_collect_rendered, with the display image written through `out` (disp_w x disp_h, the three named
 * channels only; a 4th channel is left untouched).  Work queued on `stream` after this call sees the
 * image.  NULL stream: the image is complete when the call returns.  Refused (RTP_EINVAL, nothing collected):
 * a view that fails the checks above or is not disp_w x disp_h, render == 0, and an oldest frame without a
 * display image (submitted as a net input: collect it with rtp_collect). */
int rtp_collect_rendered_device(rtp_engine* e, uint64_t* tag, float* joints, int* num_people,
                                const rtp_frame_view* out, void* stream);

/* ---- JPEG files encoded on the GPU: byte for byte what rtp_encode_jpeg writes (baseline, 4:2:0, standard tables) ---------- */

/* The largest file rtp_encode_jpeg / the GPU encoder can write for a w x h image (header + every block at its worst, every byte
 * stuffed + EOI).  Host only; 0 for w or h < 1. */
size_t rtp_jpeg_max_bytes(int w, int h);

/* = rtp_encode_jpeg on the pixels of a device view (the checks of rtp_submit_frame_device), encoded on the GPU after the work
 * queued on `stream` so far (NULL: the null stream).  Returns with the file in jpeg_host (NULL: only *jpeg_bytes is set);
 * capacity below the file's size -> RTP_EINVAL.  quality is clamped to 1..100 like rtp_encode_jpeg.  Uses the engine's own
 * scratch: frames in flight are not disturbed. */
int rtp_encode_jpeg_device(rtp_engine* e, const rtp_frame_view* src, int quality, void* stream, unsigned char* jpeg_host,
                           size_t capacity, size_t* jpeg_bytes);

/* JPEG mode of the renderer.  0: off (the default).  1..100: every rendered frame (overlay or part_to_show view) is encoded on
 * the GPU at this quality right after the render kernel, and only the file is copied to the host; collect it with
 * rtp_collect_rendered_jpeg (rtp_collect_rendered is refused, rtp_collect_rendered_device still works).  Refused: render == 0 or
 * quality outside 0..100, YUV mode on (rtp_set_render_yuv: one mode at a time) (RTP_EINVAL), frames in flight (RTP_EAGAIN). */
int rtp_set_render_jpeg(rtp_engine* e, int quality);

/* = rtp_collect_rendered with the JPEG file of the rendered frame in place of the raw image (*jpeg_bytes = its length).
 * Refused before the frame leaves the FIFO (RTP_EINVAL): JPEG mode off, capacity < rtp_jpeg_max_bytes(disp_w, disp_h), an
 * oldest frame without a display image. */
int rtp_collect_rendered_jpeg(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* jpeg_host,
                              size_t capacity, size_t* jpeg_bytes);

/* ---- YUV frames, converted on the GPU (the planes a video decoder or a Y4M file delivers; see rtp_yuv_view) ---------- */

/* = rtp_submit_frame on the pixels rtp_convert_yuv makes of the HOST view: same joints, frame_scale and rendered frames.  The planes
 * are staged without their pitches (1.5 bytes per pixel cross PCIe for 4:2:0 instead of 3) and converted by a kernel in front of
 * the warp.  Where the device pre-processing cannot run (see rtp_debug_preprocess) the frame is converted on the host. */
int rtp_submit_frame_yuv(rtp_engine* e, const rtp_yuv_view* frame_host, uint64_t tag, float* frame_scale);

/* = rtp_submit_frame_device for a YUV frame in device memory (a hardware decoder's NV12 surface): the contract and the `stream`
 * ordering of that entry; the caller's planes are released after the conversion kernel alone.  Checked on the host before any
 * launch (RTP_EINVAL + rtp_last_error, the engine stays usable): the fields as documented at rtp_yuv_view (also for a NULL
 * engine), extents without overflow, and for EACH of y, u, v on its own (they may be three allocations) device memory of
 * cfg.device_id whose last addressed byte lies inside its allocation; a stream that is not capturing. */
int rtp_submit_frame_yuv_device(rtp_engine* e, const rtp_yuv_view* frame_dev, void* stream, uint64_t tag, float* frame_scale);

/* The conversion alone: src_dev -> the three named channels of dst_dev (same width and height; a 4th channel is left untouched),
 * both in device memory and checked as above.  Runs after the work queued on `stream`; work queued on `stream` afterwards sees the
 * image (NULL: the null stream, and the image is complete when the call returns).  Uses no frame slot: frames in flight are not
 * disturbed. */
int rtp_convert_yuv_device(rtp_engine* e, const rtp_yuv_view* src_dev, const rtp_frame_view* dst_dev, void* stream);

/* ---- YUV planes out, converted on the GPU (yuv_export.hip): byte for byte what rtp_convert_bgr_to_yuv writes ---------------------- */

/* The conversion alone, the other way round: the three named channels of src_dev -> the planes of dst_dev (same width and height;
 * pitch padding is not written), both in device memory and checked as for rtp_convert_yuv_device.  Same `stream` contract.  Uses no
 * frame slot: frames in flight are not disturbed. */
int rtp_convert_to_yuv_device(rtp_engine* e, const rtp_frame_view* src_dev, const rtp_yuv_view* dst_dev, void* stream);

/* YUV mode of the renderer.  0: off (the default).  420: every rendered frame (overlay or part_to_show view) is converted to planar
 * 4:2:0 on the GPU right after the render kernel, and only the planes are copied to the host (rtp_yuv_bytes(disp_w, disp_h, 420)
 * bytes instead of 3 per pixel); collect them with rtp_collect_rendered_yuv (rtp_collect_rendered is refused,
 * rtp_collect_rendered_device and rtp_collect_rendered_yuv_device still work).  Refused: render == 0, any other chroma value, JPEG
 * mode on (RTP_EINVAL; rtp_set_render_jpeg is refused likewise while this mode is on), frames in flight (RTP_EAGAIN). */
int rtp_set_render_yuv(rtp_engine* e, int chroma);

/* = rtp_collect_rendered with the planes of the rendered frame in place of the raw image: Y (disp_w x disp_h), then U, then V
 * ((disp_w + 1) / 2 x (disp_h + 1) / 2 each), pitches = plane widths — the payload of a Y4M FRAME.  Refused before the frame leaves
 * the FIFO (RTP_EINVAL): YUV mode off, capacity < rtp_yuv_bytes(disp_w, disp_h, 420), an oldest frame without a display image. */
int rtp_collect_rendered_yuv(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* planes_host, size_t capacity);

/* = rtp_collect_rendered_device with the rendered frame converted into the caller's planes (disp_w x disp_h; e.g. the pitched NV12
 * surface of a hardware encoder): the checks and the `stream` contract of that entry, the view checked as in
 * rtp_convert_to_yuv_device.  Works in every mode of the renderer. */
int rtp_collect_rendered_yuv_device(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, const rtp_yuv_view* out_dev,
                                    void* stream);

/* ---- JPEG files, decoded on the GPU (jpeg_dec.hip): byte for byte the pixels of rtp_decode_image ---------------------- */

/* Where the Huffman decoding of a file ran.  DEVICE: baseline / extended sequential files (SOF0 / SOF1, 8 bit) whose one scan holds
 * all components (at most 10 blocks per MCU) with regular restart markers: only the scan crosses PCIe.  HOST: everything else the
 * host decoder accepts (progressive, several scans, irregular markers, tables behind the scan): codecs.cpp's own entropy decoder
 * fills the coefficient blocks and those are staged.  Dequantisation, IDCT, up-sampling and colour run on the GPU either way. */
#define RTP_JPEG_ENTROPY_DEVICE 0
#define RTP_JPEG_ENTROPY_HOST 1

/* Decodes the file into the three named channels of dst_dev (device memory, checked as in rtp_convert_yuv_device; width and
 * height must be the file's; a 4th channel is left untouched).  Runs after the work queued on `stream` and returns when the
 * decode status is known (the image is then complete).  Every file rtp_decode_image rejects is rejected here with the same code
 * and message (rtp_last_error), corrupt Huffman codes and AC runs past 63 found on the device included.  Uses engine scratch
 * only: frames in flight are not disturbed.  *entropy_path (may be NULL) = RTP_JPEG_ENTROPY_*. */
int rtp_decode_jpeg_device(rtp_engine* e, const unsigned char* jpeg_host, size_t n, const rtp_frame_view* dst_dev, void* stream,
                           int* entropy_path);

/* = rtp_submit_frame on the pixels rtp_decode_image makes of the file: same joints, frame_scale and rendered frames.  Only the
 * scan (or, on the HOST entropy path, the coefficients) crosses PCIe; the decode kernels run in front of the warp and the call does
 * not wait for the GPU.  Header errors are reported by the call (the code of rtp_decode_image); corrupt entropy-coded data found on
 * the device makes the rtp_collect* of this tag release the frame and return RTP_EIO with a message, and the engine stays usable.
 * *w, *h (may be NULL) = the file's size.  Where the device pre-processing cannot run the file is decoded on the host.
 * In tracking mode (rtp_set_tracking) such a frame has advanced the tracker like any other frame, on the people its chain produced. */
int rtp_submit_frame_jpeg(rtp_engine* e, const unsigned char* jpeg_host, size_t n, uint64_t tag, float* frame_scale, int* w, int* h);

/* ---- maps mode: a frame's part-confidence maps and PAFs from the async path (maps_export.hip) -------------------------- */

/* The engine computes heat_channels maps per frame (rtp_engine_info; COCO 57: 18 parts, background, 38 PAF channels).  Maps mode
 * hands chosen channels of every submitted frame to the caller.  Off by default, and then nothing about the engine changes.  On:
 * each frame's post-processing chain gains ONE kernel on the frame's own stream, which evaluates the chosen channels straight
 * from the low-res maps (the fp32 resized map is never written), converts them and writes a per-slot buffer that is copied to
 * pinned host memory behind it.  Frames submitted as net inputs (rtp_submit, rtp_submit_device) get maps too. */
#define RTP_MAPS_GRID_NET 0    /* [nch][net_h][net_w]: the resized_map blob (ImResize over all scales), the values rtp_resize returns, bit for bit */
#define RTP_MAPS_GRID_LOWRES 1 /* [num_scales][nch][low_h][low_w]: concat_stage7 as rtp_forward_heatmaps returns it */
#define RTP_MAPS_F32 0
#define RTP_MAPS_F16 1         /* IEEE binary16, round to nearest even (rtp_maps_to_f16) */
#define RTP_MAPS_U8 2          /* rtp_maps_quantize_u8 */
typedef struct rtp_maps_config {
  unsigned int struct_size; /* sizeof(rtp_maps_config) */
  int grid, format;         /* RTP_MAPS_GRID_*, RTP_MAPS_F32 / F16 / U8 */
  const int* channels;      /* indices into concat_stage7, in output order: any order, repeats allowed (copied by the call); NULL = all heat_channels */
  int num_channels;         /* 1 .. RTP_MAX_NUM_PARTS (ignored when channels == NULL) */
} rtp_maps_config;

/* Switches maps mode on (or changes it), NULL cfg = off.  Thresholds and scales may change while it is on (rtp_set_scales changes the
 * maps as it changes ImResize).  Refused, with the engine unchanged: wrong struct_size, unknown grid or format, num_channels out of
 * range, a channel outside [0, heat_channels) (RTP_EINVAL); frames in flight (RTP_EAGAIN). */
int rtp_set_maps_output(rtp_engine* e, const rtp_maps_config* cfg);

/* shape = {1, nch, net_h, net_w} (NET) or {num_scales, nch, low_h, low_w} (LOWRES), *format, *bytes = the dense payload of one
 * frame (any of the three may be NULL).  RTP_EINVAL while the mode is off. */
int rtp_maps_info(const rtp_engine* e, int shape[4], int* format, size_t* bytes);

/* Blocks until the OLDEST frame in flight is finished (a partial batch is launched, exactly as rtp_collect does) and copies its maps
 * (dense, the shape of rtp_maps_info) and its tag.  The frame STAYS in flight: follow with whichever rtp_collect* the frame needs.
 * Peeking twice returns the same maps.  Refused: mode off, maps_host NULL or capacity < bytes, a deferred-weights engine without
 * weights (RTP_EINVAL); nothing in flight (RTP_EAGAIN). */
int rtp_peek_maps(rtp_engine* e, uint64_t* tag, void* maps_host, size_t capacity);

/* Where rtp_peek_maps_device writes: element (x, y) of plane z (NET: z = output channel; LOWRES: z = scale * nch + output channel)
 * is at data + z * channel_stride + y * row_stride + x * element size, strides in bytes, row_stride >= width * element size,
 * channel_stride >= height * row_stride.  Bytes between rows and between planes are never written. */
typedef struct rtp_maps_view {
  unsigned int struct_size; /* sizeof(rtp_maps_view) */
  void* data;               /* device memory of cfg.device_id */
  long channel_stride, row_stride;
} rtp_maps_view;

/* = rtp_peek_maps with the maps written by the kernel itself into the caller's device memory, checked like an rtp_frame_view (device
 * memory of cfg.device_id, the last addressed byte inside its allocation) before anything is launched.  `stream` as in
 * rtp_collect_rendered_device: NULL = the maps are complete on return; else they are written in `stream`'s order (which must not
 * be capturing), and the engine's next batch on that frame slot waits for the write.  Any address and pitch is accepted;
 * naturally aligned views are written with wide stores.  The kernel runs a second time for this call (the caller's memory is not
 * known when the batch is launched); the frame's copy to pinned host memory has run as for rtp_peek_maps. */
int rtp_peek_maps_device(rtp_engine* e, uint64_t* tag, const rtp_maps_view* out_dev, void* stream);

/* Parity tap like rtp_post_from_lowres (idle engine, context 0): the maps of the current mode for the given low-res maps
 * [num_scales][heat_channels][low_h][low_w]. */
int rtp_maps_from_lowres(rtp_engine* e, const float* lowres_host, void* maps_host, size_t capacity);

/* Host only: the one definition of the two narrow formats.  u8, in float arithmetic: q = rintf(fminf(fmaxf(s, 0.f), 255.f)) with
 * s = v * 255.f for confidence and background channels (is_paf 0: channel <= num_parts) and s = (v + 1.f) * 127.5f for PAF channels
 * (is_paf 1); ties round to even, NaN gives 0.  f16: IEEE binary16 bits, round to nearest even, NaN stays NaN. */
int rtp_maps_quantize_u8(const float* v, size_t n, int is_paf, unsigned char* out);
int rtp_maps_to_f16(const float* v, size_t n, uint16_t* out);

/* ---- crops mode: per-person boxes and fixed-size crops of the display image (crops.hip) ------------------------------- */

/* A second stage per person (hands, faces, re-identification, a top-down refiner) wants a fixed-size patch around each person or
 * around a group of parts.  Crops mode hands every submitted frame's boxes and crops to the caller.  Off by default, and then
 * nothing about the engine changes.  On: each frame's post-processing chain gains ONE kernel on the frame's own stream behind the
 * connect kernels.  It reads num_people and the joints in device memory (no host synchronisation), derives a box per person and
 * resamples the frame's un-rendered display image into max_crops fixed-size slots.  Slot k belongs to person k (no compaction);
 * n = min(num_people, max_crops) slots are produced.  rtp_crop_people is the one definition of the arithmetic; the kernel's boxes
 * and pixels equal it bit for bit.
 *
 * THE BOX, in float32, every operation rounded on its own (no fused multiply-add), in exactly this order:
 *   A list entry p of person k counts when score > min_score and x and y are finite (a NaN score never counts).  A repeated entry
 *   counts once per repeat.  count = the number of counting entries; count < min_parts: the slot has no box.
 *   Every counting x and y is first taken as x + 0.0f (so that -0 is +0 and min / max do not depend on the order).
 *   x0 = min x, x1 = max x, y0 = min y, y1 = max y
 *   cx = (x0 + x1) * 0.5f            cy = (y0 + y1) * 0.5f
 *   w = x1 - x0                      h = y1 - y0
 *   (an infinite w or h, the overflow of two huge coordinates: the slot has no box)
 *   g = (margin * fmaxf(w, h)) * 2.0f
 *   w = fmaxf(w + g, 1.0f)           h = fmaxf(h + g, 1.0f)
 *   wa = (h * (float)crop_w) / (float)crop_h
 *   if (wa > w) w = wa;  else h = (w * (float)crop_h) / (float)crop_w;
 *   left = cx - w * 0.5f             top = cy - h * 0.5f
 *   right = left + w                 bottom = top + h
 *   The box is NOT clipped to the image.  Unless |left|, |top|, |right| and |bottom| are all <= 1048576.0f (2^20; an infinity or a
 *   NaN from an overflow fails this), the slot has no box.
 * The record of slot k, RTP_CROP_BOX_FLOATS floats: {left, top, w, h, (float)count, valid (1.0f or 0.0f)}; a slot without a box
 * holds {0, 0, 0, 0, count, 0}.  Coordinates are display pixels with pixel (c, r) covering [c, c + 1) x [r, r + 1).
 *
 * THE PIXELS, integers only past these four conversions (Q16, int64):
 *   ox = (int64)rintf(left * 65536.0f)                    oy = (int64)rintf(top * 65536.0f)
 *   dx = (int64)rintf((w / (float)crop_w) * 65536.0f)     dy = (int64)rintf((h / (float)crop_h) * 65536.0f)
 *   Sx = dx <= 98304 ? 1 : dx <= 196608 ? 2 : 4 (a step of <= 1.5, <= 3, more pixels); Sy likewise from dy.
 *   Output pixel (i, j) is the mean of Sx x Sy bilinear samples.  Sample (a, b), a < Sx, b < Sy, lies at the sub-cell centre
 *     px = ox + i * dx + ((2 * a + 1) * dx) / (2 * Sx) - 32768      py = oy + j * dy + ((2 * b + 1) * dy) / (2 * Sy) - 32768
 *   (Q16 pixel-index coordinates; the divisions are exact shifts of non-negative numbers), reads the four taps at columns
 *   X = px >> 16 (floor) and X + 1 and rows Y = py >> 16 and Y + 1, with 11-bit weights per axis
 *     fx = ((px & 65535) + 16) >> 5 (0 .. 2048), weights (2048 - fx, fx); fy likewise,
 *   and is worth  (2048 - fy) * ((2048 - fx) * p[Y][X] + fx * p[Y][X+1]) + fy * ((2048 - fx) * p[Y+1][X] + fx * p[Y+1][X+1]).
 *   A tap outside the image reads 0 in all three channels (constant border).  The samples are summed (T) and
 *     value = (T + Sx * Sy * 2097152) / (Sx * Sy * 4194304)   (round half up; a shift).
 *   A box as large as the crop at an integer position is therefore a plain copy, and a box larger than the crop is box-filtered.
 * The crop of a slot without a box is all zeros.  Crop k occupies crop_w * crop_h * 3 bytes:
 *   RTP_CROPS_HWC_BGR: [crop_h][crop_w][3], the display image's channel order;  RTP_CROPS_CHW_RGB: [3][crop_h][crop_w], planes R, G, B. */
#define RTP_CROPS_HWC_BGR 0
#define RTP_CROPS_CHW_RGB 1
#define RTP_CROP_BOX_FLOATS 6
#define RTP_CROP_MIN_SIZE 8
#define RTP_CROP_MAX_SIZE 512
typedef struct rtp_crops_config {
  unsigned int struct_size; /* sizeof(rtp_crops_config) */
  int crop_w, crop_h;       /* RTP_CROP_MIN_SIZE .. RTP_CROP_MAX_SIZE each */
  int max_crops;            /* 1 .. RTP_MAX_PEOPLE */
  const int* parts;         /* part indices that span the box, any order, repeats allowed (copied by the call); NULL = all parts */
  int num_parts;            /* 1 .. RTP_MAX_NUM_PARTS (ignored when parts == NULL) */
  float min_score;          /* >= 0 */
  int min_parts;            /* >= 1 */
  float margin;             /* >= 0, <= 16 */
  int layout;               /* RTP_CROPS_HWC_BGR | RTP_CROPS_CHW_RGB, u8 both */
} rtp_crops_config;

/* Host only (no engine, no GPU): the definition above.  display_bgr: u8 HWC BGR of w x h; joints [num_people][num_parts][3] as
 * rtp_collect returns them (num_parts here = the model's parts per person).  Writes n = min(num_people, cfg->max_crops) box records
 * and, unless crops is NULL, n crops of crop_w * crop_h * 3 bytes each; nothing behind them.  display_bgr may be NULL when crops is.
 * Returns n, or RTP_EINVAL: a NULL cfg / boxes, wrong struct_size, w or h < 1 or > 32768, num_people < 0, num_parts outside
 * 1 .. RTP_MAX_NUM_PARTS, a configuration field out of its range, a listed part outside [0, num_parts), NULL joints with people,
 * NULL display_bgr with crops. */
int rtp_crop_people(const unsigned char* display_bgr, int w, int h, const float* joints, int num_people, int num_parts,
                    const rtp_crops_config* cfg, float* boxes, unsigned char* crops);

/* Host only: the part indices of a head box for rtp_crops_config.parts (rtpose.bin --crop_parts head): nose, eyes and ears for
 * RTP_MODEL_COCO_18 (5), head and neck for RTP_MODEL_MPI_15 (2).  Returns their number, or RTP_EINVAL for another model. */
int rtp_crops_head_parts(int model, int parts[8]);

/* Switches crops mode on (or changes it), NULL cfg = off.  Refused, with the engine unchanged: wrong struct_size, a size, count,
 * margin, min_score, min_parts or layout out of range, a listed part outside the model's parts (RTP_EINVAL); frames in flight
 * (RTP_EAGAIN).  Under the experiments build's RTP_GRAPH_POST=1 the post-processing chains are launched eagerly while the mode is on. */
int rtp_set_crops_output(rtp_engine* e, const rtp_crops_config* cfg);

/* The current mode (any pointer may be NULL); *crop_bytes = crop_w * crop_h * 3.  RTP_EINVAL while the mode is off. */
int rtp_crops_info(const rtp_engine* e, int* crop_w, int* crop_h, int* max_crops, int* layout, size_t* crop_bytes);

/* Blocks until the OLDEST frame in flight is finished (as rtp_collect does) and hands out its tag, *num_boxes = n, n box records
 * into boxes_host and, where the frame has a display image (*has_pixels = 1: rtp_submit_frame* frames; 0: rtp_submit,
 * rtp_submit_device) and crops_host is not NULL, n dense crops into crops_host.  capacity = the number of records / crops the two
 * buffers hold; bytes behind the n written ones are untouched.  The frame STAYS in flight: follow with whichever rtp_collect* it
 * needs; peeking twice returns the same.  The crops come from the un-rendered display image whatever the renderer does.
 * Refused: mode off, NULL boxes_host or num_boxes, a deferred-weights engine without weights (RTP_EINVAL); nothing in flight
 * (RTP_EAGAIN); capacity < n (RTP_ERANGE, *num_boxes = n, nothing else written; the frame stays peekable). */
int rtp_peek_crops(rtp_engine* e, uint64_t* tag, float* boxes_host, int* num_boxes, unsigned char* crops_host, int capacity,
                   int* has_pixels);

/* Where rtp_peek_crops_device writes: crop k starts at data + k * crop_stride, crop_stride >= crop bytes.  Bytes between crops
 * are never written.  All max_crops slots must lie inside the allocation (n is not known when the view is checked). */
typedef struct rtp_crops_view {
  unsigned int struct_size; /* sizeof(rtp_crops_view) */
  void* data;               /* device memory of cfg.device_id */
  long crop_stride;
} rtp_crops_view;

/* = rtp_peek_crops with the n crops written by the kernel itself into the caller's device memory, checked like an rtp_frame_view
 * (device memory of cfg.device_id, the last addressed byte inside its allocation) before anything is launched; the box records
 * still go to host memory (capacity as above).  `stream` as in rtp_peek_maps_device: NULL = the crops are complete on return;
 * else they are written in `stream`'s order (which must not be capturing), and the next frame staged on that frame slot waits
 * for the write.  Any address and stride is accepted; where data and crop_stride are multiples of 16 and crop_w is one too, every
 * lane stores 16 bytes at a time.  Also refused: a frame without a display image (RTP_EINVAL; rtp_peek_crops gives its boxes). */
int rtp_peek_crops_device(rtp_engine* e, uint64_t* tag, float* boxes_host, int* num_boxes, int capacity, const rtp_crops_view* out_dev,
                          void* stream);

/* Parity tap like rtp_render (idle engine, context 0): the kernel of the async path on caller data.  display_bgr_host: u8 HWC BGR
 * of cfg.disp_w x cfg.disp_h; joints_host [num_people][num_parts][3], num_people <= RTP_MAX_PEOPLE.  Writes
 * n = min(num_people, max_crops) records and crops (crops_host may be NULL), capacity as in rtp_peek_crops; returns RTP_OK and
 * *num_boxes = n. */
int rtp_crops_from_joints(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people,
                          float* boxes_host, int* num_boxes, unsigned char* crops_host, int capacity);

/* ---- tracking mode: stable person ids across frames (track.hip) --------------------------------------------------------- */

/* Person k of one frame and person k of the next are unrelated: the connect kernels order people by how the limb assignment
 * assembled them.  Tracking mode associates every submitted frame's people with a device-resident table of tracks and hands out one
 * record per person: a stable id, the table slot, the track's age and the match cost.  Off by default, and then nothing about the
 * engine changes.  On: each frame's post-processing chain gains ONE kernel on the frame's own stream behind the connect kernels.  It
 * reads num_people and the joints in device memory (no host synchronisation), updates the table and writes the records, which are
 * copied to pinned memory with the joints.  The table is one per engine and frames update it in SUBMIT order: frame n's kernel
 * waits on the device for frame n-1's, whichever streams the two frames run on.  Records line up with rtp_collect's joints and
 * with crops mode's slots by index k.  rtp_track_update is the one definition of the arithmetic; the kernel's integers and float
 * bits equal it exactly.
 *
 * THE UPDATE, everything float32, every operation rounded on its own (no fused multiply-add), in exactly this order.  P = num_parts.
 * One update takes n = clamp(num_people, 0, RTP_MAX_PEOPLE) people (a negative device num_people is the connect kernels' RTP_ERANGE
 * flag and counts as 0).  A part (x, y, score) COUNTS when score > min_score and x and y are finite (a NaN score never counts).
 *  1. Person k is TRACKABLE when its number of counting parts is >= min_parts.
 *  2. The cost of (live slot t, trackable person k): walk the parts p = 0 .. P-1 in order; where p counts in both,
 *       dx = px - tx;  dy = py - ty;  a = dx * dx;  b = dy * dy;  c = a + b;  s = s + c;  m++          (s starts at 0.0f)
 *     m < min_common: the pair is not comparable.  The track's size is taken over ALL counting parts of the track, each x and y
 *     first taken as x + 0.0f:  x0 = min x, x1 = max x, y0 = min y, y1 = max y,
 *       w = x1 - x0;  h = y1 - y0;  ww = w * w;  hh = h * h;  d = fmaxf(ww + hh, 1.0f)
 *       q = s / (float)m;  cost = q / d
 *     The pair is a CANDIDATE when cost is finite and cost <= max_cost (an overflow to infinity or a NaN fails this).
 *  3. Greedy assignment: the candidates in ascending order of (bits of cost + 0.0f as uint32, slot t, person k) — cost is >= 0, so
 *     bit order is value order — are walked once; a candidate is accepted when neither its slot nor its person has been taken.
 *     (The repeated global minimum: the result is unique, ties included.)
 *  4. A matched slot's joints become the person's (all P x 3 floats, a bit copy); hits++, misses = 0.
 *  5. An unmatched live slot: misses++; misses > max_misses: the slot is freed (id, hits, misses 0, joints zeros) and is available
 *     in step 6 of the same frame.
 *  6. Births: the unmatched trackable people, in person order, each take the LOWEST free slot with id = next_id++ (0 is skipped at
 *     the wrap), hits = 1, misses = 0, joints = the person's.  With no free slot the person stays untracked.
 *  7. frames++.
 * THE RECORD of person k, RTP_TRACK_REC_INTS int32: {id, slot, hits, cost bits}.  Matched: the track's id, its slot, its hits
 * after the update, the bits of the match's cost + 0.0f.  Newborn: {id, slot, 1, 0} (told from a zero-cost match by hits == 1).
 * Untracked (not trackable, or the table is full): {0, -1, 0, 0}.
 *
 * The defaults of rtp_track_config_default (min_score 0, min_parts 3, min_common 2, max_cost 0.0625, max_misses 15) are choices,
 * not measurements: a max_cost of 0.0625 allows a mean squared joint displacement of 1/16 of the track's squared diagonal. */
#define RTP_MAX_TRACKS 128
#define RTP_TRACK_REC_INTS 4

typedef struct rtp_track_config {
  unsigned int struct_size; /* sizeof(rtp_track_config) */
  float min_score;          /* >= 0: a part COUNTS when score > min_score and x, y are finite (a NaN score never counts) */
  int min_parts;            /* >= 1: a person with fewer counting parts is not tracked */
  int min_common;           /* >= 1: parts that must count in BOTH for a (track, person) pair to be comparable */
  float max_cost;           /* > 0, finite */
  int max_misses;           /* >= 0: a track unmatched for MORE than this many consecutive frames is dropped */
} rtp_track_config;

typedef struct rtp_track_state { /* plain data; the device copy has the same layout */
  unsigned int struct_size;      /* sizeof(rtp_track_state) */
  int num_parts;                 /* 1 .. RTP_MAX_NUM_PARTS */
  unsigned int next_id;          /* starts at 1; wraps past 0 to 1 */
  unsigned int frames;           /* frames seen since the reset */
  int id[RTP_MAX_TRACKS];        /* 0 = free slot */
  int hits[RTP_MAX_TRACKS], misses[RTP_MAX_TRACKS];
  float joints[RTP_MAX_TRACKS][RTP_MAX_NUM_PARTS][3]; /* the joints of the track's last match; zeros in free slots and beyond num_parts */
} rtp_track_state;

/* Host only (no engine, no GPU).  rtp_track_config_default: the defaults above.  rtp_track_state_init: an empty table for a model
 * of num_parts parts (next_id 1); RTP_EINVAL for num_parts outside 1 .. RTP_MAX_NUM_PARTS. */
int rtp_track_config_default(rtp_track_config* cfg);
int rtp_track_state_init(rtp_track_state* state, int num_parts);

/* Host only: the definition above, one frame.  joints [num_people][state->num_parts][3] as rtp_collect returns them (NULL is
 * accepted where no person is read); recs receives n records.  Returns n, or RTP_EINVAL with the state untouched: a NULL state, cfg
 * or recs, NULL joints with people, a wrong struct_size in either structure, a configuration field out of its range, a
 * state->num_parts outside 1 .. RTP_MAX_NUM_PARTS. */
int rtp_track_update(rtp_track_state* state, const rtp_track_config* cfg, const float* joints, int num_people, int* recs);

/* Switches tracking mode on, NULL cfg = off (the state is discarded).  Off -> on starts from an empty state (next_id 1); while the
 * mode is on, a new cfg keeps the state.  Refused, with the engine unchanged: wrong struct_size or a field out of range
 * (RTP_EINVAL); frames in flight (RTP_EAGAIN).  Only frames that went through rtp_submit* advance the tracker (and
 * rtp_track_from_joints): the synchronous taps (rtp_forward_debug, rtp_post_from_lowres, the maps and crops taps, calibration,
 * rtp_profile_steps) never do.  A frame whose collect returns RTP_EIO (rtp_submit_frame_jpeg: a corrupt scan) or RTP_ERANGE has
 * advanced the tracker like any other frame: the kernel ran on whatever people the chain produced (none, for RTP_ERANGE).
 * Under the experiments build's RTP_GRAPH_POST=1 the post-processing chains are launched eagerly while the mode is on. */
int rtp_set_tracking(rtp_engine* e, const rtp_track_config* cfg);

/* Idle engine only (RTP_EAGAIN with frames in flight); RTP_EINVAL while the mode is off.  reset: an empty state (next_id 1).
 * get / set: the whole table, e.g. to carry the ids over to another engine; set also refuses (RTP_EINVAL) a wrong struct_size and a
 * num_parts that is not the engine's. */
int rtp_track_reset(rtp_engine* e);
int rtp_track_get_state(rtp_engine* e, rtp_track_state* state);
int rtp_track_set_state(rtp_engine* e, const rtp_track_state* state);

/* The contract of rtp_peek_crops: blocks until the OLDEST frame in flight is finished and hands out its tag, *num_recs = n and n
 * records of RTP_TRACK_REC_INTS ints into recs_host; capacity = the records recs_host holds.  The frame STAYS in flight; peeking
 * twice returns the same records.  Refused: mode off, NULL recs_host or num_recs, a negative capacity (RTP_EINVAL); nothing in
 * flight (RTP_EAGAIN); capacity < n (RTP_ERANGE, *num_recs = n, nothing else written; the frame stays peekable). */
int rtp_peek_tracks(rtp_engine* e, uint64_t* tag, int* recs_host, int* num_recs, int capacity);

/* Parity tap (idle engine, context 0): the kernel of the async path on caller data, joints_host [num_people][num_parts][3],
 * of which n = clamp(num_people, 0, RTP_MAX_PEOPLE) people are read; num_people itself goes to the device as it is.  It ADVANCES the
 * engine's state by one frame; frames submitted next continue from it.  Writes n records, capacity as in rtp_peek_tracks; returns
 * RTP_OK and *num_recs = n. */
int rtp_track_from_joints(rtp_engine* e, const float* joints_host, int num_people, int* recs_host, int* num_recs, int capacity);

/* rtp_format_json's text with "id":N, in front of every body's "joints" (N = recs[k * RTP_TRACK_REC_INTS], 0 = untracked).
 * recs == NULL: byte for byte rtp_format_json's output. */
long rtp_format_json_tracked(char* buf, size_t buflen, const float* joints, int num_people, int num_parts, float frame_scale,
                             const int* recs);

/* ---- appearance-aided tracking: a colour descriptor per person in the assignment cost (appearance.hip, track.hip) --------- */

/* The tracker's cost is joint displacement alone.  Two people who pass each other between two frames have the lower summed
 * displacement with their ids swapped, and a person who reappears where somebody else stood inherits that track.  This mode, off by
 * default and usable only while tracking mode is on, gives the tracker a look at the pixels: a colour histogram per person, taken
 * from the frame's un-rendered display image around a list of parts, a table of one smoothed histogram per track slot, and an
 * appearance term in the cost.  The per-frame descriptors also leave the engine with the joints (rtp_peek_appearance), for
 * matching people across cameras or engines.  While the mode is off nothing changes, neither a launch nor a byte.  On: each frame's
 * chain gains ONE kernel (appear_describe) on the frame's own stream behind the connect kernels, and the frame's track kernel is
 * the appearance form of the same kernel.  rtp_appearance_describe and rtp_track_update_appearance are the one definition of the
 * arithmetic; the kernels' integers and float bits equal them exactly.
 *
 * THE DESCRIPTOR of person k, from the display image (u8 HWC BGR, w x h) and the person's joints.
 *   Which parts count: the list `parts` / `num_parts` as in rtp_crops_config; NULL = the model's torso parts
 *   (rtp_appearance_torso_parts; a model of 18 parts is taken as RTP_MODEL_COCO_18, of 15 as RTP_MODEL_MPI_15, any other model: all
 *   its parts).  A list entry p counts when score > min_score and x and y are finite (a NaN score never counts).  A repeated entry
 *   counts once per repeat.  count < min_parts: the person has no descriptor (valid = 0, the bins are zeros).
 *   The box, in float32, every operation rounded on its own (no fused multiply-add), in exactly this order — the crops box up to and
 *   without its aspect step:
 *     Every counting x and y is first taken as x + 0.0f (so that -0 is +0 and min / max do not depend on the order).
 *     x0 = min x, x1 = max x, y0 = min y, y1 = max y
 *     cx = (x0 + x1) * 0.5f            cy = (y0 + y1) * 0.5f
 *     w = x1 - x0                      h = y1 - y0
 *     (an infinite w or h, the overflow of two huge coordinates: no descriptor)
 *     g = (margin * fmaxf(w, h)) * 2.0f
 *     w = fmaxf(w + g, 1.0f)           h = fmaxf(h + g, 1.0f)
 *     left = cx - w * 0.5f             top = cy - h * 0.5f
 *     right = left + w                 bottom = top + h
 *     The box is NOT clipped to the image.  Unless |left|, |top|, |right| and |bottom| are all <= 1048576.0f (2^20; an infinity or
 *     a NaN from an overflow fails this), the person has no descriptor.
 *   The samples, a fixed RTP_APPEARANCE_GRID x RTP_APPEARANCE_GRID (32 x 32) grid, integers only past these four conversions (Q16,
 *   int64):
 *     ox = (int64)rintf(left * 65536.0f)                 oy = (int64)rintf(top * 65536.0f)
 *     dx = (int64)rintf((w / 32.0f) * 65536.0f)          dy = (int64)rintf((h / 32.0f) * 65536.0f)
 *     Sample (i, j), i, j = 0 .. 31, reads the pixel at column clamp((ox + i * dx + dx / 2) >> 16, 0, w - 1) and row
 *     clamp((oy + j * dy + dy / 2) >> 16, 0, h - 1) of the image (>> is the arithmetic shift: floor; dx, dy >= 0, so / 2 is a shift
 *     too).  The border is replicated: every person with a descriptor has exactly 1024 samples.
 *   The bins: a sample's bin is (j >= 16 ? 64 : 0) + (r >> 6) * 16 + (g >> 6) * 4 + (b >> 6).  Grid rows 0 .. 15 and 16 .. 31 keep
 *   separate histograms, so that upper and lower clothing differ.  The descriptor is uint16 bins[RTP_APPEARANCE_BINS] and sums to 1024.
 *
 * THE TABLE, one entry per track slot: owner[t] and desc[t][RTP_APPEARANCE_BINS] in Q4 (counts times 16).  Slot t HAS a descriptor
 * when owner[t] == id[t] != 0 (id: the track table's).  This is smoothing mode's owner rule: nothing is cleared when a track dies.
 *
 * THE COST.  Steps 1 and 2 of rtp_track_update are unchanged: the motion cost and its max_cost gate.  Then, for a pair (t, k) that
 * passed, everything float32 and every operation rounded on its own:
 *   slot t has a descriptor (in the tables as they stand before the update) and person k's is valid:
 *     L = sum over the bins b of |desc[t][b] - 16 * bins_k[b]|  (an integer; 0 .. 32768 for descriptors this definition produced)
 *     a = (float)L / 32768.0f  (exact);  a <= max_dist, or the pair is no candidate
 *   otherwise a = unknown, and the max_dist gate is skipped.
 *   wa = weight * a;  total = cost + wa.  The pair is a CANDIDATE when total is finite.
 * Steps 3 to 7 run on the candidates' keys (bits of total + 0.0f as uint32, slot t, person k).  A matched person's record carries
 * the bits of total + 0.0f where rtp_track_update's carries the cost's.
 *
 * THE TABLE UPDATE, after step 6, for every person k with a slot t (matched or born) and a valid descriptor, id = the slot's id now:
 *   owner[t] == id:  desc[t][b] = (desc[t][b] * (256 - rate) + 16 * bins_k[b] * rate + 128) >> 8  for every bin (rate 256 replaces)
 *   otherwise:       desc[t][b] = 16 * bins_k[b],  owner[t] = id
 * A person without a valid descriptor leaves its slot's entry alone.
 *
 * With weight 0, max_dist 1 and unknown 0, records and track table are rtp_track_update's bit for bit, whatever the descriptors are.
 * The defaults of rtp_appearance_config_default (the torso parts, min_score 0, min_parts 3, margin 0, weight 0.125, max_dist 1,
 * unknown 0.25, rate 32) are choices, not measurements: at weight 0.125 a person in entirely different colours costs as much as two
 * times tracking mode's default max_cost, and rate 32 moves a slot's histogram an eighth of the way to the frame's. */
#define RTP_APPEARANCE_BINS 128
#define RTP_APPEARANCE_GRID 32
typedef struct rtp_appearance_config {
  unsigned int struct_size; /* sizeof(rtp_appearance_config) */
  const int* parts;         /* part indices that span the box, any order, repeats allowed (copied by the call); NULL = the torso parts */
  int num_parts;            /* 1 .. RTP_MAX_NUM_PARTS (ignored when parts == NULL) */
  float min_score;          /* >= 0, finite */
  int min_parts;            /* >= 1 */
  float margin;             /* >= 0, <= 16 */
  float weight;             /* >= 0, finite */
  float max_dist;           /* > 0, <= 1 */
  float unknown;            /* >= 0, <= 1 */
  int rate;                 /* 1 .. 256 */
} rtp_appearance_config;

typedef struct rtp_appearance_state { /* plain data; the device copy has the same layout */
  unsigned int struct_size;           /* sizeof(rtp_appearance_state) */
  int reserved[3];                    /* zeros (desc starts at a multiple of 16 bytes) */
  int owner[RTP_MAX_TRACKS];          /* the id the slot's descriptor belongs to; 0 = none yet */
  uint16_t desc[RTP_MAX_TRACKS][RTP_APPEARANCE_BINS]; /* Q4 */
} rtp_appearance_state;

/* Host only (no engine, no GPU).  rtp_appearance_config_default: the defaults above.  rtp_appearance_state_init: an empty table.
 * rtp_appearance_torso_parts: the part indices of a torso box for rtp_appearance_config.parts: neck, shoulders and hips for
 * RTP_MODEL_COCO_18 (5); neck, shoulders, hips and chest for RTP_MODEL_MPI_15 (6).  Returns their number, or RTP_EINVAL for another
 * model.  The first two return RTP_OK, or RTP_EINVAL for a NULL pointer. */
int rtp_appearance_config_default(rtp_appearance_config* cfg);
int rtp_appearance_state_init(rtp_appearance_state* state);
int rtp_appearance_torso_parts(int model, int parts[8]);

/* Host only: THE DESCRIPTOR above.  display_bgr: u8 HWC BGR of w x h; joints [num_people][num_parts][3] as rtp_collect returns them
 * (num_parts here = the model's parts per person).  Writes n = min(num_people, RTP_MAX_PEOPLE) descriptors into
 * bins_out [n][RTP_APPEARANCE_BINS] and n bytes (1 or 0) into valid_out; nothing behind them.  Returns n, or RTP_EINVAL: a NULL cfg,
 * bins_out or valid_out, wrong struct_size, w or h < 1 or > 32768, num_people < 0, num_parts outside 1 .. RTP_MAX_NUM_PARTS, a
 * configuration field out of its range, a listed part outside [0, num_parts), NULL joints or display_bgr with people. */
int rtp_appearance_describe(const unsigned char* display_bgr, int w, int h, const float* joints, int num_people, int num_parts,
                            const rtp_appearance_config* cfg, uint16_t* bins_out, unsigned char* valid_out);

/* Host only: rtp_track_update with THE COST and THE TABLE UPDATE above, one frame.  joints, num_people and recs as in
 * rtp_track_update; bins [n][RTP_APPEARANCE_BINS] and valid [n] are rtp_appearance_describe's for the same people.  bins == NULL: every
 * person counts as having no descriptor (a frame without a display image).  Returns n, or RTP_EINVAL with BOTH states untouched:
 * whatever rtp_track_update refuses, a NULL appearance state or configuration, a wrong struct_size in either, an appearance field
 * out of its range, bins without valid.  (The part list of appearance_cfg is not read here.) */
int rtp_track_update_appearance(rtp_track_state* track_state, rtp_appearance_state* appearance_state, const rtp_track_config* track_cfg,
                                const rtp_appearance_config* appearance_cfg, const float* joints, int num_people, const uint16_t* bins,
                                const unsigned char* valid, int* recs);

/* Switches the mode on (or changes it), NULL cfg = off (the descriptor table is discarded; the track table is kept either way).
 * Usable only while tracking mode is on, and rtp_set_tracking(e, NULL) is refused while this mode is on.  Off -> on starts from an
 * empty descriptor table; while the mode is on, a new cfg keeps it.  Refused, with the engine unchanged: wrong struct_size, a field
 * out of range, a listed part outside the model's parts, tracking mode off (RTP_EINVAL); frames in flight (RTP_EAGAIN).  The
 * descriptors always come from the RAW joints (the kernel runs in front of the tracker); smoothing, overlay, crops and redaction
 * mode read the records and joints they read without it.  A frame without a display image (rtp_submit, rtp_submit_device) gets
 * valid = 0 for everybody and is tracked with a = unknown; so are the joints-only taps (rtp_track_from_joints,
 * rtp_smooth_from_joints, rtp_overlay_from_joints) while the mode is on. */
int rtp_set_track_appearance(rtp_engine* e, const rtp_appearance_config* cfg);

/* Idle engine only (RTP_EAGAIN with frames in flight); RTP_EINVAL while the mode is off.  reset: an empty descriptor table.
 * get / set: the whole table, e.g. to carry it over to another engine with the track table; set also refuses (RTP_EINVAL) a wrong
 * struct_size.  rtp_track_reset and rtp_track_set_state leave this table alone: a slot's entry counts only while its owner is the
 * slot's id. */
int rtp_appearance_reset(rtp_engine* e);
int rtp_appearance_get_state(rtp_engine* e, rtp_appearance_state* state);
int rtp_appearance_set_state(rtp_engine* e, const rtp_appearance_state* state);

/* The contract of rtp_peek_tracks: blocks until the OLDEST frame in flight is finished and hands out its tag, *num = n and the
 * frame's n descriptors into bins_host [n][RTP_APPEARANCE_BINS] and valid_host [n]; capacity = the descriptors the two buffers hold.
 * Entry k is person k of rtp_collect, record k of rtp_peek_tracks and slot k of crops mode.  The frame STAYS in flight; peeking
 * twice returns the same.  Refused: mode off, NULL bins_host, valid_host or num, a negative capacity (RTP_EINVAL); nothing in flight
 * (RTP_EAGAIN); capacity < n (RTP_ERANGE, *num = n, nothing else written; the frame stays peekable). */
int rtp_peek_appearance(rtp_engine* e, uint64_t* tag, uint16_t* bins_host, unsigned char* valid_host, int* num, int capacity);

/* Parity taps (idle engine, context 0; the mode must be on): the kernels of the async path on caller data.  display_bgr_host: u8 HWC
 * BGR of cfg.disp_w x cfg.disp_h, or NULL = a frame without a display image; joints_host [num_people][num_parts][3], of which
 * n = clamp(num_people, 0, RTP_MAX_PEOPLE) people are read; num_people itself goes to the device as it is.  Capacity as in
 * rtp_peek_appearance; both return RTP_OK and *num = n.
 * rtp_appearance_from_joints: the describe kernel alone; writes n descriptors and valid bytes; no table is touched.
 * rtp_track_from_frame: the describe kernel and the track kernel; writes n records and (bins_host and valid_host both NULL or both
 * given) the n descriptors; it ADVANCES both tables by one frame. */
int rtp_appearance_from_joints(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people,
                               uint16_t* bins_host, unsigned char* valid_host, int* num, int capacity);
int rtp_track_from_frame(rtp_engine* e, const unsigned char* display_bgr_host, const float* joints_host, int num_people, int* recs_host,
                         uint16_t* bins_host, unsigned char* valid_host, int* num, int capacity);

/* ---- smoothing mode: tracked people filtered over time, per joint (smooth.hip) ------------------------------------------ */

/* The joints of rtp_collect are per-frame NMS peaks: on a still person they jitter by a fraction of a pixel to a few pixels, and a
 * part whose peak falls under the threshold for a frame or two vanishes and comes back.  Smoothing mode, off by default and usable
 * only while tracking mode is on, filters every tracked person's parts over time with the One-Euro filter (Casiez, Roussel and
 * Vogel, CHI 2012; time is counted in frames) and holds a part that dropped out for up to max_hold frames.  Each submitted frame's
 * chain gains ONE more kernel behind the track kernel on the frame's own stream.  It reads num_people, the joints and the frame's
 * track records in device memory (no host synchronisation), updates a device-resident filter table, one cell per (track slot,
 * part), and writes three arrays per frame, which are copied to pinned memory in front of the frame's last event:
 *   joints_s [n][P][3] float32   the filtered (x, y, score);   vel [n][P][2] float32   the filtered velocity in pixels per frame;
 *   flags [n][P] uint8           RTP_SMOOTH_FLAG_*: what happened to the part.
 * rtp_collect's joints stay the raw ones, always.  The table is one per engine and is updated in submit order, like the track table:
 * the event the next frame's chain waits on is recorded behind the smooth kernel.  rtp_smooth_update is the one definition of the
 * arithmetic; the kernel's float bits and bytes equal it exactly.
 *
 * THE UPDATE, everything float32, every operation rounded on its own (no fused multiply-add), in exactly this order; `/` is the
 * correctly rounded division.  TWO_PI = 6.2831855f (bits 0x40C90FDB).  P = num_parts.  One update takes
 * n = clamp(num_people, 0, RTP_MAX_PEOPLE) people with their n track records (rtp_track_update's, or rtp_peek_tracks').
 *  1. frames++ (0 is skipped at the wrap, as next_id is); now = frames.  Gaps are now - last in uint32 arithmetic.
 *  2. Person k whose record has id == 0 is untracked: joints_s is a bit copy of the person's triples, vel is 0, a part's flag is
 *     1 where it COUNTS and 0 otherwise.  A part counts under tracking's rule: score > min_score and x, y finite (a NaN score never
 *     counts).  No cell is touched.
 *  3. Person k with id != 0 and slot t is handled part by part, independently.  The cell C = (t, p) is LIVE when C.owner == id and
 *     C.last != 0.  g = now - C.last.
 *     - The part counts, and C is not live or g - 1 > max_hold: START.  C.owner = id, C.last = now, C.pos = (x, y), C.vel = (0, 0),
 *       C.score = score.  Output (x, y, score), vel 0, flag 1.
 *     - The part counts otherwise: FILTER.  dt = (float)g; per coordinate v (x, then y), with vh = C.pos[i], dvh = C.vel[i]:
 *         d = v - vh;  dv = d / dt
 *         rd = TWO_PI * d_cutoff;  rd = rd * dt;  ad = rd / (rd + 1.0f)
 *         t1 = ad * dv;  t2 = (1.0f - ad) * dvh;  e = t1 + t2
 *         fc = beta * fabsf(e);  fc = min_cutoff + fc
 *         r = TWO_PI * fc;  r = r * dt;  a = r / (r + 1.0f)
 *         u1 = a * v;  u2 = (1.0f - a) * vh;  vh' = u1 + u2
 *       If any of the four results (vh' and e, for x and y) is not finite, the part is STARTed instead.  Otherwise
 *       C.pos = (xh', yh'), C.vel = (ex, ey), C.score = score, C.last = now.  Output (xh', yh', score), vel (ex, ey), flag 2.
 *     - The part does not count, C is live and g <= max_hold: HELD.  Output (C.pos, C.score) and C.vel as bit copies, flag 3.  The
 *       cell is unchanged.
 *     - The part does not count otherwise: output the person's triple as a bit copy, vel 0, flag 0.  The cell is unchanged.
 *     The boundary is consistent: a part held for max_hold frames and measured in the next one continues its filter with
 *     dt = max_hold + 1.
 * A reborn slot carries a new id, so its old cells are not live: nothing has to be cleared when a track dies.  Cells beyond
 * num_parts are never touched.
 *
 * The defaults of rtp_smooth_config_default (min_score 0, min_cutoff and d_cutoff 1/30 cycles per frame = 1 Hz at 30 frames/s,
 * beta 0.01 per pixel, max_hold 5, apply 0) are choices, not measurements. */
#define RTP_SMOOTH_RENDER 1 /* apply: the rendered frame draws joints_s (held parts included: no flicker) */
#define RTP_SMOOTH_CROPS 2  /* apply: crops mode takes its boxes and crops from joints_s */
#define RTP_SMOOTH_FLAG_NONE 0
#define RTP_SMOOTH_FLAG_START 1 /* also: a counting part of an untracked person */
#define RTP_SMOOTH_FLAG_FILTER 2
#define RTP_SMOOTH_FLAG_HELD 3
#define RTP_SMOOTH_MAX_HOLD 1000

typedef struct rtp_smooth_config {
  unsigned int struct_size; /* sizeof(rtp_smooth_config) */
  float min_score;          /* >= 0, finite: a part COUNTS when score > min_score and x, y are finite */
  float min_cutoff;         /* > 0, finite: the cutoff at rest, cycles per frame */
  float beta;               /* >= 0, finite: how fast the cutoff opens with speed, 1 / pixel */
  float d_cutoff;           /* > 0, finite: the cutoff of the velocity's own filter, cycles per frame */
  int max_hold;             /* 0 .. RTP_SMOOTH_MAX_HOLD: frames a part that does not count is held at its last filtered value */
  unsigned int apply;       /* bit mask of RTP_SMOOTH_RENDER and RTP_SMOOTH_CROPS (the engine's mode only; rtp_smooth_update ignores it) */
} rtp_smooth_config;

typedef struct rtp_smooth_cell {
  int owner;         /* a track id, 0 = none */
  unsigned int last; /* the value of frames at the part's last measurement, 0 = no filter */
  float pos[2], vel[2];
  float score;
} rtp_smooth_cell;

typedef struct rtp_smooth_state { /* plain data; the device copy has the same layout */
  unsigned int struct_size;       /* sizeof(rtp_smooth_state) */
  int num_parts;                  /* 1 .. RTP_MAX_NUM_PARTS */
  unsigned int frames;            /* updates since the reset; wraps past 0 to 1 */
  rtp_smooth_cell cell[RTP_MAX_TRACKS][RTP_MAX_NUM_PARTS];
} rtp_smooth_state;

/* Host only (no engine, no GPU).  rtp_smooth_config_default: the defaults above.  rtp_smooth_state_init: an empty table for a model
 * of num_parts parts; RTP_EINVAL for num_parts outside 1 .. RTP_MAX_NUM_PARTS. */
int rtp_smooth_config_default(rtp_smooth_config* cfg);
int rtp_smooth_state_init(rtp_smooth_state* state, int num_parts);

/* Host only: the definition above, one frame.  joints [num_people][state->num_parts][3] as rtp_collect returns them and recs
 * [n][RTP_TRACK_REC_INTS] (NULL is accepted for either where no person is read); joints_s [n][P][3], vel [n][P][2] and flags [n][P]
 * receive the outputs; vel and flags may be NULL.  Returns n, or RTP_EINVAL with the state untouched: a NULL state, cfg or joints_s,
 * NULL joints or recs with people, a wrong struct_size in either structure, a configuration field out of its range, a
 * state->num_parts outside 1 .. RTP_MAX_NUM_PARTS, a record with id != 0 whose slot is outside 0 .. RTP_MAX_TRACKS - 1, two records
 * with id != 0 that name the same slot. */
int rtp_smooth_update(rtp_smooth_state* state, const rtp_smooth_config* cfg, const float* joints, int num_people, const int* recs,
                      float* joints_s, float* vel, unsigned char* flags);

/* Switches smoothing mode on, NULL cfg = off (the state is discarded).  Off -> on starts from an empty state; while the mode is on,
 * a new cfg keeps the state.  Refused, with the engine unchanged: tracking mode off, a wrong struct_size or a field out of range
 * (RTP_EINVAL); frames in flight (RTP_EAGAIN).  While smoothing is on rtp_set_tracking(e, NULL) is refused with RTP_EINVAL: switch
 * smoothing off first.  rtp_track_reset and rtp_track_set_state leave the smoothing state alone: ids stay unique, so stale cells are
 * simply not live.  Only frames that went through rtp_submit* advance the filter (and rtp_smooth_from_joints); the synchronous taps,
 * calibration and rtp_profile_steps never do, and they render and crop from the raw joints.
 * apply: with RTP_SMOOTH_RENDER the render stage of a submitted frame (cfg.render = 1) runs behind the smooth kernel and draws
 * joints_s; with RTP_SMOOTH_CROPS crops mode's kernel does and takes boxes and crops from joints_s.  Held parts carry their last
 * score, so the renderer draws them and the boxes span them.  Record k stays person k.  With apply == 0 the stages run where they
 * run without the mode. */
int rtp_set_smoothing(rtp_engine* e, const rtp_smooth_config* cfg);

/* Idle engine only (RTP_EAGAIN with frames in flight); RTP_EINVAL while the mode is off.  reset: an empty state.  get / set: the whole
 * table; set also refuses (RTP_EINVAL) a wrong struct_size and a num_parts that is not the engine's. */
int rtp_smooth_reset(rtp_engine* e);
int rtp_smooth_get_state(rtp_engine* e, rtp_smooth_state* state);
int rtp_smooth_set_state(rtp_engine* e, const rtp_smooth_state* state);

/* The contract of rtp_peek_tracks: blocks until the OLDEST frame in flight is finished and hands out its tag, *num_people = n and the
 * three arrays of n people; capacity = the people each array holds; vel_host and flags_host may be NULL.  The frame STAYS in flight;
 * peeking twice returns the same data.  Refused: mode off, NULL joints_s_host or num_people, a negative capacity (RTP_EINVAL);
 * nothing in flight (RTP_EAGAIN); capacity < n (RTP_ERANGE, *num_people = n, nothing else written; the frame stays peekable). */
int rtp_peek_smoothed(rtp_engine* e, uint64_t* tag, float* joints_s_host, float* vel_host, unsigned char* flags_host, int* num_people,
                      int capacity);

/* Parity tap (idle engine, context 0): the track kernel and then the smooth kernel of the async path on caller data, joints_host
 * [num_people][num_parts][3], of which n = clamp(num_people, 0, RTP_MAX_PEOPLE) people are read; num_people itself goes to the
 * device as it is.  It ADVANCES both states by one frame.  Writes n records (recs_host may be NULL) and the three arrays of n people
 * (vel_host and flags_host may be NULL), capacity as in rtp_peek_smoothed; returns RTP_OK and *num_out = n. */
int rtp_smooth_from_joints(rtp_engine* e, const float* joints_host, int num_people, int* recs_host, float* joints_s_host,
                           float* vel_host, unsigned char* flags_host, int* num_out, int capacity);

/* ---- overlay mode: tracked people drawn into the rendered frame: boxes, ids, trails (overlay.hip) -------------------------- */

/* The rendered frame (rtp_collect_rendered*, JPEG and YUV mode) shows anonymous skeletons.  Overlay mode, off by default and usable
 * only while tracking mode is on and rtp_config.render >= 1, draws for every tracked person of a submitted frame a box, an id label
 * in a built-in bitmap font and a fading trail of the track's recent positions, all in a colour derived from the id, BEFORE the
 * image is exported: the raw host copy, rtp_collect_rendered_device, JPEG mode and YUV mode all carry the drawing.  Each submitted
 * frame's chain gains two kernels.  overlay_update runs as one workgroup behind the track kernel (and the smooth kernel where that
 * mode is on): it reads num_people, the joints and the frame's records in device memory, advances a device-resident trail table,
 * one ring of anchor points per track slot, in submit order (the tracker's chain of events, recorded behind this kernel), and
 * writes the frame's DRAW LIST.  overlay_draw then draws the list, in item order, in place into the slot's rendered image.
 * rtp_overlay_update and rtp_overlay_draw are the one definition of both; the kernels' integers and bytes equal them exactly.
 *
 * THE UPDATE.  One update takes n = clamp(num_people, 0, RTP_MAX_PEOPLE) people with their n track records.  frames++ (0 is skipped
 * at the wrap).  Then, per person k in person order:
 *  1. A record with id == 0 produces nothing and touches nothing.  A part COUNTS under tracking's rule: score > min_score and x, y
 *     finite.  A person without a counting part produces nothing and touches nothing.
 *  2. Over the counting parts, in float32 comparisons: fx0 = min x, fx1 = max x, fy0 = min y, fy1 = max y.  Each is rounded ONCE:
 *       q(v) = (int)floorf(clampf(v, -32767.0f, 32767.0f) + 0.5f)          (round half up; the sum is one float32 addition)
 *     Everything from here on is integer arithmetic.  The box is x0 = q(fx0) - box_margin, y0 = q(fy0) - box_margin,
 *     x1 = q(fx1) + box_margin, y1 = q(fy1) + box_margin, corners inclusive.  The ANCHOR is (floor((x0 + x1) / 2), floor((y0 + y1) / 2)).
 *  3. The trail ring S of the record's slot: where S.owner != id the ring is emptied and re-owned (owner = id, count = 0, head = 0;
 *     the points stay as they are: nothing is cleared when a track dies, a reborn slot carries a new id).  The anchor is pushed:
 *     pts[head] = anchor, head = (head + 1) % RTP_TRAIL_MAX, count = min(count + 1, trail_len).  The kept points are the last `count`
 *     pushed ones; the oldest is pts[(head - count) mod RTP_TRAIL_MAX].  (trail_len 0 keeps none, a smaller trail_len forgets the oldest.)
 *  4. The person's items, in this order: with RTP_OVERLAY_TRAIL the m = max(count - 1, 0) capsules between consecutive kept points,
 *     oldest pair first; with RTP_OVERLAY_BOX the box; with RTP_OVERLAY_LABEL the label.
 * AN ITEM is RTP_OVERLAY_ITEM_INTS int32: {kind, x0, y0, x1, y1, size, colour, alpha, value}.  colour = RTP_OVERLAY_PALETTE[id & 15],
 * packed b | g << 8 | r << 16.
 *   capsule j of m: {RTP_OVERLAY_KIND_CAPSULE, ax, ay, bx, by, trail_radius, colour, alpha * (j + 1) / m (integer division), 0}
 *   box:            {RTP_OVERLAY_KIND_RECT, x0, y0, x1, y1, line_width, colour, alpha, 0}
 *   label:          {RTP_OVERLAY_KIND_LABEL, lx, ly, lx + LW - 1, ly + LH - 1, label_scale, colour, alpha, id}
 *     D = the number of decimal digits of the id taken as uint32 (1 .. 10); LW = (6 * D + 1) * label_scale, LH = 9 * label_scale.
 *     lx = x0; ly = y0 - LH: the label sits above the box's top-left corner; where ly < 0 (it would leave the image's top)
 *     ly = y0: inside the box.
 *
 * THE DRAWING walks the items in order; the blends do not commute, so the order matters.  A pixel (px, py) that an item COVERS becomes,
 * per channel c of the item's colour (the label: see below), (src * (256 - alpha) + c * alpha + 128) >> 8.  Pixels outside the image
 * are skipped, whatever the item's coordinates.
 *   RECT covers x0 <= px <= x1, y0 <= py <= y1 with px - x0 < size or x1 - px < size or py - y0 < size or y1 - py < size: an outline
 *     of `size` pixels that grows inwards (a size beyond half the box fills it).
 *   CAPSULE, a = (x0, y0), b = (x1, y1), d = b - a, r = size, in exact integer arithmetic (int64, no float): t = (p - a) . d,
 *     L = d . d.  L == 0 or t < 0: |p - a|^2 <= r^2.  t > L: |p - b|^2 <= r^2.  Otherwise cross = (px - ax) * dy - (py - ay) * dx and
 *     cross^2 <= r^2 * L (r^2 * L < 2^44: an implementation may clamp |cross| to 2^31 before squaring).
 *   LABEL covers its whole rectangle.  With s = size, u = (px - x0) / s, v = (py - y0) / s: the pixel belongs to a digit when
 *     1 <= v <= 7, u >= 1, c = (u - 1) % 6 < 5, i = (u - 1) / 6 < D, and bit (4 - c) of RTP_OVERLAY_FONT[digit i][v - 1] is set, digit 0
 *     being the most significant one of `value` as uint32.  A digit's pixel takes the text colour, every other one the item's
 *     colour.  The text colour is black (0, 0, 0) where (29 * b + 150 * g + 77 * r) >> 8 >= 128 for the item's colour, white
 *     (255, 255, 255) otherwise.  One blend per pixel.
 *   Any other kind covers nothing.
 *
 * The font (5 x 7, seven row bytes per digit, bit 4 = the leftmost column) and the palette were written for this project.  The
 * defaults of rtp_overlay_config_default (everything drawn, min_score 0, box_margin 4, line_width 2, label_scale 1, trail_len 16,
 * trail_radius 1, alpha 192) are choices, not measurements. */
#define RTP_OVERLAY_BOX 1
#define RTP_OVERLAY_LABEL 2
#define RTP_OVERLAY_TRAIL 4
#define RTP_OVERLAY_KIND_CAPSULE 1
#define RTP_OVERLAY_KIND_RECT 2
#define RTP_OVERLAY_KIND_LABEL 3
#define RTP_TRAIL_MAX 32
#define RTP_OVERLAY_ITEM_INTS 9
#define RTP_OVERLAY_MAX_ITEMS (RTP_MAX_PEOPLE * (RTP_TRAIL_MAX + 1))
#define RTP_OVERLAY_MAX_MARGIN 1024
/* packed b | g << 8 | r << 16 */
#define RTP_OVERLAY_PALETTE \
  { 0x3C14DC, 0x32CD32, 0xFF901E, 0x00D7FF, 0xD355BA, 0xD1CE00, 0x008CFF, 0x9314FF, 0x578B2E, 0xE16941, 0x20A5DA, 0xCC3299, 0xAAB220, 0x2D52A0, \
    0x7FFF00, 0xB469FF }
#define RTP_OVERLAY_FONT \
  { {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, \
    {0x1E, 0x01, 0x01, 0x0E, 0x01, 0x01, 0x1E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E}, \
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, \
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C} }

typedef struct rtp_overlay_config {
  unsigned int struct_size; /* sizeof(rtp_overlay_config) */
  unsigned int what;        /* a non-empty mask of RTP_OVERLAY_BOX | RTP_OVERLAY_LABEL | RTP_OVERLAY_TRAIL */
  float min_score;          /* >= 0, finite: a part COUNTS when score > min_score and x, y are finite */
  int box_margin;           /* 0 .. RTP_OVERLAY_MAX_MARGIN pixels around the counting parts */
  int line_width;           /* 1 .. 16 */
  int label_scale;          /* 1 .. 8: pixels per font pixel */
  int trail_len;            /* 0 .. RTP_TRAIL_MAX points kept per track */
  int trail_radius;         /* 0 .. 16 */
  int alpha;                /* 0 .. 256 */
} rtp_overlay_config;

typedef struct rtp_trail_slot {
  int owner; /* a track id, 0 = none */
  int count; /* kept points, 0 .. RTP_TRAIL_MAX */
  int head;  /* where the next point goes, 0 .. RTP_TRAIL_MAX - 1 */
  int pts[RTP_TRAIL_MAX][2];
} rtp_trail_slot;

typedef struct rtp_trail_state { /* plain data; the device copy has the same layout */
  unsigned int struct_size;      /* sizeof(rtp_trail_state) */
  int num_parts;                 /* 1 .. RTP_MAX_NUM_PARTS */
  unsigned int frames;           /* updates since the reset; wraps past 0 to 1 */
  rtp_trail_slot slot[RTP_MAX_TRACKS];
} rtp_trail_state;

/* Host only (no engine, no GPU).  rtp_overlay_config_default: the defaults above.  rtp_trail_state_init: an empty table for a model
 * of num_parts parts; RTP_EINVAL for num_parts outside 1 .. RTP_MAX_NUM_PARTS. */
int rtp_overlay_config_default(rtp_overlay_config* cfg);
int rtp_trail_state_init(rtp_trail_state* state, int num_parts);

/* Host only: THE UPDATE above, one frame.  joints [num_people][state->num_parts][3] and recs [n][RTP_TRACK_REC_INTS] (NULL is
 * accepted for either where no person is read); items receives *num_items items of RTP_OVERLAY_ITEM_INTS ints, capacity = the items
 * it holds (RTP_OVERLAY_MAX_ITEMS always suffices).  Returns RTP_OK; RTP_ERANGE with *num_items = the frame's count and the state
 * untouched where capacity is smaller; RTP_EINVAL with the state untouched: a NULL state, cfg, items or num_items, a negative
 * capacity, NULL joints or recs with people, a wrong struct_size in either structure, a configuration field out of its range, a
 * state->num_parts outside 1 .. RTP_MAX_NUM_PARTS, a ring whose count or head is out of its range, a record with id != 0 whose slot
 * is outside 0 .. RTP_MAX_TRACKS - 1, two records with id != 0 that name the same slot. */
int rtp_overlay_update(rtp_trail_state* state, const rtp_overlay_config* cfg, const float* joints, int num_people, const int* recs,
                       int* items, int* num_items, int capacity);

/* Host only: THE DRAWING above onto image_bgr, h rows of w BGR pixels, `stride` bytes from row to row (>= 3 * w).  num_items 0
 * leaves the image untouched.  RTP_EINVAL: a NULL image, NULL items with num_items > 0, a negative num_items, w or h < 1, a stride
 * below 3 * w.  An item's alpha is taken as clamp(alpha, 0, 256) and its size as clamp(size, 0, 16) (a label's: 1 .. 8); rectangle
 * and label corners and capsule end points are taken as clamp(v, -65535, 65535). */
int rtp_overlay_draw(const int* items, int num_items, unsigned char* image_bgr, int w, int h, long stride);

/* Switches overlay mode on, NULL cfg = off (the trail table is discarded).  Off -> on starts from an empty table; while the mode is
 * on, a new cfg keeps it.  Refused, with the engine unchanged: tracking mode off, rtp_config.render == 0, a wrong struct_size or a
 * field out of range (RTP_EINVAL); frames in flight (RTP_EAGAIN).  While the overlay is on rtp_set_tracking(e, NULL) is refused with
 * RTP_EINVAL.  Only frames that went through rtp_submit* advance the trail table (and rtp_overlay_from_joints); the synchronous taps
 * never do, and their rendered images carry no drawing.  With smoothing mode's RTP_SMOOTH_RENDER the overlay takes the smoothed
 * joints, held parts included, so that box and skeleton agree; otherwise the raw ones.  A frame submitted without a display image
 * (rtp_submit) advances the table and has a draw list, but nothing is drawn.  With the mode off the engine launches what it
 * launched before the mode existed. */
int rtp_set_track_overlay(rtp_engine* e, const rtp_overlay_config* cfg);

/* Idle engine only (RTP_EAGAIN with frames in flight); RTP_EINVAL while the mode is off.  reset: an empty table.  get / set: the whole
 * table; set also refuses (RTP_EINVAL) a wrong struct_size, a num_parts that is not the engine's and a ring whose count or head is
 * out of its range. */
int rtp_overlay_reset(rtp_engine* e);
int rtp_overlay_get_state(rtp_engine* e, rtp_trail_state* state);
int rtp_overlay_set_state(rtp_engine* e, const rtp_trail_state* state);

/* The contract of rtp_peek_tracks: blocks until the OLDEST frame in flight is finished and hands out its tag, *num_items and that
 * many items; capacity = the items items_host holds.  The frame STAYS in flight.  Refused: mode off, NULL items_host or num_items, a
 * negative capacity (RTP_EINVAL); nothing in flight (RTP_EAGAIN); capacity < *num_items (RTP_ERANGE, *num_items set, nothing else
 * written; the frame stays peekable). */
int rtp_peek_overlay_items(rtp_engine* e, uint64_t* tag, int* items_host, int* num_items, int capacity);

/* Parity tap (idle engine, context 0): the track, overlay_update and overlay_draw kernels of the async path on caller data.  joints_host
 * [num_people][num_parts][3], of which n = clamp(num_people, 0, RTP_MAX_PEOPLE) people are read; num_people itself goes to the device
 * as it is.  image_host_in_out: a dense w x h BGR image (1 <= w <= cfg.disp_w, 1 <= h <= cfg.disp_h; no display frame is needed) that
 * comes back with the drawing, or NULL (w and h ignored: no drawing).  It ADVANCES the track table and the trail table by one
 * frame.  Writes n records (recs_out may be NULL; room for n <= RTP_MAX_PEOPLE records) and *num_items items, capacity as in
 * rtp_peek_overlay_items. */
int rtp_overlay_from_joints(rtp_engine* e, const float* joints_host, int num_people, unsigned char* image_host_in_out, int w, int h,
                            int* recs_out, int* items_out, int* num_items, int capacity);

/* ---- redaction mode: people's heads mosaicked, blurred or filled in the rendered frame (redact.hip) ------------------------ */

/* The rendered frame shows the people's faces on every export path.  Redaction mode, off by default and usable while
 * rtp_config.render >= 1 (it does NOT need tracking mode), replaces for every person of a submitted frame a region around the listed
 * parts (the head's by default) BEFORE the image is exported: the raw host copy, rtp_collect_rendered_device, JPEG mode and YUV mode
 * all carry it, only the encoded frame crosses PCIe and the host touches no pixel.  Each submitted frame's chain gains
 * redact_regions, one workgroup that reads num_people and the joints in device memory and writes one record per person, and
 * redact_apply, one workgroup per tile of the rendered image, behind the pose overlay and in front of overlay mode's drawing: boxes,
 * ids and trails stay sharp on top of the redaction.  rtp_redact_regions and rtp_redact_apply are the one definition of both; the
 * kernels' integers and bytes equal them exactly.
 *
 * CROPS MODE AND MAPS MODE KEEP HANDING OUT UN-REDACTED DATA: crops are resampled from the un-rendered display image, and the maps
 * are the network's.  A deployment that must not leak faces must not enable them, or must treat their output as sensitive.  The
 * synchronous taps (rtp_render) carry no redaction either.
 *
 * THE REGIONS.  n = clamp(num_people, 0, RTP_MAX_PEOPLE) (a negative device num_people is the connect kernels' RTP_ERANGE flag and
 * counts as 0).  Per person k:
 *  1. A listed part COUNTS under tracking's rule: score > min_score and x, y finite.  c = the number of listed parts that count.
 *     Where c < min_parts the record is {0, 0, 0, 0, c, 0}.
 *  2. Over the counting listed parts, in float32 comparisons: fx0 = min x, fx1 = max x, fy0 = min y, fy1 = max y.  Each is rounded
 *     ONCE with overlay mode's q(v) = (int)floorf(clampf(v, -32767.0f, 32767.0f) + 0.5f): x0 = q(fx0), x1 = q(fx1), y0 = q(fy0),
 *     y1 = q(fy1).  Everything from here on is integer arithmetic.
 *  3. cx = floor((x0 + x1) / 2), cy = floor((y0 + y1) / 2) (floor for negative sums too); s = max(x1 - x0, y1 - y0) + 1;
 *     rx = clamp(((s * scale_q8) >> 9) + pad, min_radius, RTP_REDACT_MAX_RADIUS);  ry = min((rx * aspect_q8) >> 8, RTP_REDACT_MAX_RADIUS).
 * THE RECORD is RTP_REDACT_REGION_INTS int32: {cx, cy, rx, ry, c, valid (1 or 0)}.
 *
 * THE PIXELS.  A pixel (px, py) is COVERED by a valid region (valid != 0) when |px - cx| <= rx and |py - cy| <= ry and, for
 * RTP_REDACT_ELLIPSE, with dx = px - cx, dy = py - cy in int64, (dx * ry)^2 + (dy * rx)^2 <= (rx * ry)^2 (a zero radius therefore
 * covers the centre column or row).  A record's cx and cy are taken as clamp(v, -65535, 65535), its rx and ry as
 * clamp(v, 0, RTP_REDACT_MAX_RADIUS).  A pixel covered by at least one region is replaced by a value computed from the image AS IT
 * WAS BEFORE THE CALL, so the result depends neither on the order of the regions nor on how they overlap; every other byte, the
 * padding between rows included, keeps its value.  The value, per channel:
 *   RTP_REDACT_FILL    the colour (packed b | g << 8 | r << 16).
 *   RTP_REDACT_MOSAIC  cells of cell x cell pixels aligned to the image's origin, the pixel's cell being (px / cell, py / cell):
 *                      (sum + (cnt >> 1)) / cnt over the cnt pixels of that cell that lie inside the image, covered or not.
 *   RTP_REDACT_BLUR    (sum + (cnt >> 1)) / cnt over the window [px - radius, px + radius] x [py - radius, py + radius] clipped to
 *                      the image (a box filter, NOT computed in place).
 *
 * The defaults of rtp_redact_config_default (mosaic, ellipse, the model's head parts, min_score 0, min_parts 1, scale_q8 384,
 * aspect_q8 320, pad 2, min_radius 4, cell 8, radius 8, black) are choices, not measurements: a head's radius is taken as 3/4 of
 * the span of its key points, and a head as 5/4 as tall as it is wide. */
#define RTP_REDACT_MOSAIC 0
#define RTP_REDACT_BLUR 1
#define RTP_REDACT_FILL 2
#define RTP_REDACT_ELLIPSE 0
#define RTP_REDACT_RECT 1
#define RTP_REDACT_REGION_INTS 6
#define RTP_REDACT_MAX_RADIUS 4096

typedef struct rtp_redact_config {
  unsigned int struct_size; /* sizeof(rtp_redact_config) */
  int effect;               /* RTP_REDACT_MOSAIC | RTP_REDACT_BLUR | RTP_REDACT_FILL */
  int shape;                /* RTP_REDACT_ELLIPSE | RTP_REDACT_RECT */
  const int* parts;         /* part indices that span the region, any order, repeats refused (copied by the call); NULL = the model's
                             * rtp_crops_head_parts (a model of 18 parts is taken as RTP_MODEL_COCO_18, of 15 as RTP_MODEL_MPI_15) */
  int num_parts;            /* 1 .. RTP_MAX_NUM_PARTS (ignored when parts == NULL) */
  float min_score;          /* >= 0, finite */
  int min_parts;            /* >= 1: a person with fewer counting listed parts has no region */
  int scale_q8;             /* 64 .. 4096 */
  int aspect_q8;            /* 64 .. 1024 */
  int pad;                  /* 0 .. 256 */
  int min_radius;           /* 0 .. 256 */
  int cell;                 /* 2, 4, 8, 16 or 32 (RTP_REDACT_MOSAIC) */
  int radius;               /* 1 .. 16 (RTP_REDACT_BLUR) */
  unsigned int colour;      /* packed b | g << 8 | r << 16 (RTP_REDACT_FILL); the bits above are ignored */
} rtp_redact_config;

/* Host only (no engine, no GPU): the defaults above. */
int rtp_redact_config_default(rtp_redact_config* cfg);

/* Host only: THE REGIONS above.  joints [num_people][num_parts][3] as rtp_collect returns them (num_parts = the model's parts per
 * person; NULL is accepted where no person is read); regions receives n records.  Returns n, or RTP_EINVAL with regions untouched:
 * a NULL cfg or regions, NULL joints with people, a wrong struct_size, a field out of its range, a repeated part or one outside
 * [0, num_parts), num_parts outside 1 .. RTP_MAX_NUM_PARTS, NULL parts for a model of neither 18 nor 15 parts. */
int rtp_redact_regions(const float* joints, int num_people, int num_parts, const rtp_redact_config* cfg, int* regions);

/* Host only: THE PIXELS above, in place for the caller, onto image_bgr, h rows of w BGR pixels, `stride` bytes from row to row.
 * num_regions 0 leaves the image untouched.  RTP_EINVAL with the image untouched: a NULL cfg or image, NULL regions with
 * num_regions > 0, num_regions outside 0 .. RTP_MAX_PEOPLE, w or h < 1 or > 32768, a stride below 3 * w, a wrong struct_size, a
 * field out of its range (a part list is checked against RTP_MAX_NUM_PARTS). */
int rtp_redact_apply(const int* regions, int num_regions, const rtp_redact_config* cfg, unsigned char* image_bgr, int w, int h, long stride);

/* Switches redaction mode on (or changes it), NULL cfg = off.  Refused, with the engine unchanged: rtp_config.render == 0, a wrong
 * struct_size or a field out of range, a repeated part or one outside the model's (RTP_EINVAL); frames in flight (RTP_EAGAIN).  The
 * regions come from the joints the frame is rendered with: smoothing mode's joints_s, held parts included, where it has
 * RTP_SMOOTH_RENDER (a nose that drops out for one frame does not un-blur a face), the raw joints otherwise.  A frame submitted
 * without a display image (rtp_submit) has records, but nothing is redacted.  The blur's scratch image (display size, one per frame
 * slot) is allocated by this call, never per frame.  With the mode off the engine launches what it launched before the mode existed.
 * Under the experiments build's RTP_GRAPH_POST=1 the mode behaves as crops mode does. */
int rtp_set_redaction(rtp_engine* e, const rtp_redact_config* cfg);

/* The current mode: *cfg with parts = NULL and num_parts = the list's length, the list itself into parts (room for
 * RTP_MAX_NUM_PARTS ints); either pointer may be NULL.  RTP_EINVAL while the mode is off. */
int rtp_redaction_info(const rtp_engine* e, rtp_redact_config* cfg, int* parts);

/* The contract of rtp_peek_tracks: blocks until the OLDEST frame in flight is finished and hands out its tag, *num_regions = n and
 * n records; capacity = the records regions_host holds.  The frame STAYS in flight.  Refused: mode off, NULL regions_host or
 * num_regions, a negative capacity (RTP_EINVAL); nothing in flight (RTP_EAGAIN); capacity < n (RTP_ERANGE, *num_regions set,
 * nothing else written; the frame stays peekable). */
int rtp_peek_redactions(rtp_engine* e, uint64_t* tag, int* regions_host, int* num_regions, int capacity);

/* Parity tap (idle engine, context 0, mode on): the two kernels of the async path on caller data.  joints_host
 * [num_people][num_parts][3], of which n = clamp(num_people, 0, RTP_MAX_PEOPLE) people are read; num_people itself goes to the device
 * as it is.  image_host_in_out: a dense w x h BGR image (1 <= w <= cfg.disp_w, 1 <= h <= cfg.disp_h) that comes back redacted, or
 * NULL (w and h ignored: regions only).  Writes *num_regions = n and n records, capacity as in rtp_peek_redactions. */
int rtp_redact_from_joints(rtp_engine* e, const float* joints_host, int num_people, unsigned char* image_host_in_out, int w, int h,
                           int* regions_out, int* num_regions, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* RTPOSE_MI355X_H_ */
