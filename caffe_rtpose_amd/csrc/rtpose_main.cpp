// rtpose_main.cpp — rtpose.bin: the reference's CLI surface (examples/rtpose/rtpose.cpp:50-72,
// 1674-1780) over the MI355X engine.  Thread structure follows rtcpm() (rtpose.cpp:1459-1547):
//   1 producer (decode/generate -> display-fit warp -> scale pyramid -> net input)   :302/393
//   NUM_GPU workers, one engine each, all pulling from ONE shared queue              :1099-1203
//   1 re-orderer (min-heap on frame.index, window BUFFER_SIZE = 4, skips dropped)    :1214-1273
//   1 writer (JSON, latency log every 30 frames)                                     :1315-1454
// There is no collective: frames are independent.  Differences from the reference,
// all forced by the environment: no display/camera (no GUI stack), image decoding limited to
// JPEG/PNG/PPM/BMP and Y4M / raw MJPEG (codecs.cpp), `--video synthetic:WxH:frames[:seed]` generates frames procedurally, and the
// process exits at end of input also without --write_frames (the reference loops the video forever).
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <dirent.h>
#include <fstream>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <pthread.h>
#include <sched.h>
#include <queue>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <vector>

#include "../../include/rtpose_mi355x.h"

extern "C" {
// Weak here: the host-side sanitizer build of this file links against link-time stand-ins of the engine (tests/helpers/engine_stub.cpp)
// that have no GPU encoder; --dry_engine never calls these.  rtpose.bin binds them to librtpose_mi355x.so.
int rtp_set_render_jpeg(rtp_engine* e, int quality) __attribute__((weak));
int rtp_collect_rendered_jpeg(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* jpeg_host, size_t capacity,
                              size_t* jpeg_bytes) __attribute__((weak));
// (the stand-ins have no YUV entry either: without it every frame takes the BGR path, as with --host_yuv)
int rtp_submit_frame_yuv(rtp_engine* e, const rtp_yuv_view* frame_host, uint64_t tag, float* frame_scale) __attribute__((weak));
// (nor a JPEG entry: without it every file is decoded on the producer side, as with --host_decode)
int rtp_submit_frame_jpeg(rtp_engine* e, const unsigned char* jpeg_host, size_t n, uint64_t tag, float* frame_scale, int* w, int* h) __attribute__((weak));
// (nor the YUV mode of the renderer: --write_video x.y4m then needs --host_video, as under --dry_engine)
int rtp_set_render_yuv(rtp_engine* e, int chroma) __attribute__((weak));
int rtp_collect_rendered_yuv(rtp_engine* e, uint64_t* tag, float* joints, int* num_people, unsigned char* planes_host, size_t capacity) __attribute__((weak));
// (nor maps mode: --write_heatmaps then runs only under --dry_engine)
int rtp_set_maps_output(rtp_engine* e, const rtp_maps_config* cfg) __attribute__((weak));
int rtp_peek_maps(rtp_engine* e, uint64_t* tag, void* maps_host, size_t capacity) __attribute__((weak));
// (nor crops mode: --write_crops then writes box files without boxes, as under --dry_engine)
int rtp_set_crops_output(rtp_engine* e, const rtp_crops_config* cfg) __attribute__((weak));
int rtp_peek_crops(rtp_engine* e, uint64_t* tag, float* boxes_host, int* num_boxes, unsigned char* crops_host, int capacity, int* has_pixels) __attribute__((weak));
// (nor tracking mode: --track then runs rtp_track_update in the re-orderer, as under --dry_engine)
int rtp_set_tracking(rtp_engine* e, const rtp_track_config* cfg) __attribute__((weak));
int rtp_peek_tracks(rtp_engine* e, uint64_t* tag, int* recs_host, int* num_recs, int capacity) __attribute__((weak));
// (nor appearance mode: --track_appearance then runs rtp_appearance_describe and rtp_track_update_appearance in the re-orderer, as under --dry_engine)
int rtp_set_track_appearance(rtp_engine* e, const rtp_appearance_config* cfg) __attribute__((weak));
// (nor smoothing mode: --smooth then runs rtp_smooth_update in the re-orderer, as under --dry_engine)
int rtp_set_smoothing(rtp_engine* e, const rtp_smooth_config* cfg) __attribute__((weak));
int rtp_peek_smoothed(rtp_engine* e, uint64_t* tag, float* joints_s_host, float* vel_host, unsigned char* flags_host, int* num_people, int capacity) __attribute__((weak));
// (nor overlay mode: --draw_tracks then runs rtp_overlay_update and rtp_overlay_draw in the re-orderer, as with --host_draw)
int rtp_set_track_overlay(rtp_engine* e, const rtp_overlay_config* cfg) __attribute__((weak));
// (nor redaction mode: --redact then runs rtp_redact_regions and rtp_redact_apply in the re-orderer, as with --host_redact)
int rtp_set_redaction(rtp_engine* e, const rtp_redact_config* cfg) __attribute__((weak));
double rtp_display_fit_scale(int ow, int oh, int disp_w, int disp_h);
int rtp_preprocess_frame(const unsigned char* bgr, int w, int h, int disp_w, int disp_h, int net_w, int net_h, int num_scales,
                         double start_scale, double scale_gap, float* net_input, unsigned char* display_bgr, float* frame_scale);
int rtp_load_image(const char* path, unsigned char* out_bgr, size_t capacity, int* w, int* h);
int rtp_synth_frame(unsigned char* out_bgr, int w, int h, int index, uint64_t seed);
}

namespace {

double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- flags (names and defaults: rtpose.cpp:50-72) --------------------------------------------
struct Flags {
  bool host_preprocess = false;
  bool host_jpeg = false;        // --write_frames: encode on the host (rtp_encode_jpeg on an encoder pool) instead of on the GPU
  // --write_video FILE.y4m|FILE.mjpeg|FILE.mjpg: the rendered frames as ONE stream (rtp_video_create), written in order by the display
  // thread.  .y4m: the renderer's YUV mode, only the 4:2:0 planes cross PCIe; .mjpeg: its JPEG mode at the quality of --write_frames.
  // --host_video: the raw frames cross PCIe and are converted (rtp_convert_bgr_to_yuv) / encoded (rtp_encode_jpeg) by the display thread
  // instead: the same bytes, and the only path under --dry_engine.
  std::string write_video;
  int video_fps = 30;
  bool host_video = false;
  bool host_yuv = false;         // --video x.y4m: convert every frame to BGR on the producer thread (rtp_video_read) instead of on the GPU
  // JPEG files are decoded on the GPU (rtp_submit_frame_jpeg: only the file crosses PCIe) or on the producer side (rtp_decode_image).
  // Default by source (profiles/r09_jpeg_decode.txt): --video x.mjpeg on the GPU (one producer thread decodes a video), --image_dir on
  // the producer pool (many host cores outrun the GPU decoder).  --host_decode / --gpu_decode choose for both sources.
  bool host_decode = false, gpu_decode = false;
  bool fullscreen = false, no_frame_drops = false, no_display = false, no_text = false, logtostderr = false;
  int part_to_show = 0, camera = 0, start_frame = 0, start_device = 0, num_gpu = 1, num_scales = 1;
  std::string write_frames, write_json, video, image_dir;
  // --write_heatmaps PREFIX: every frame's maps (maps mode of the engine: u8 on the net grid) as PREFIX%06d.pgm, binary P5 of net_w x
  // nch * net_h with channel k in rows [k * net_h, (k + 1) * net_h), written in frame order by the display thread.
  // --heatmap_channels parts|bkg|parts+bkg|pafs|all chooses the channels (the reference's --heatmaps_add_parts / _bkg / _PAFs).
  std::string write_heatmaps, heatmap_channels = "parts+bkg";
  // --write_crops PREFIX: every frame's per-person crops of the un-rendered display image (crops mode of the engine) as
  // PREFIX%06d_%02d.ppm (binary P6, one file per slot that has a box; %02d = the person's index in the frame's joints) and one
  // PREFIX%06d_boxes.json per frame, written in frame order by the display thread.
  // --crop_size WxH, --crop_parts all|head|p0,p1,.. (the parts that span a box), --crop_margin F, --max_crops N
  std::string write_crops, crop_size = "128x128", crop_parts = "all";
  double crop_margin = 0.15;
  int max_crops = 16;
  // --track: stable person ids across frames.  One real GPU worker: the engine's tracking mode (rtp_set_tracking; the association runs
  // on the GPU in submit order).  --num_gpu N > 1, --dry_engine or --host_preprocess: the re-orderer, which sees the frames in order,
  // runs rtp_track_update on each frame's joints.  --write_json bodies and --write_crops box records then carry "id".
  bool track = false;
  double track_max_cost = 0.0625;
  int track_max_misses = 15, track_min_parts = 3;
  // --track_appearance (needs --track): a colour descriptor per person in the tracker's cost, so that ids survive a crossing.  One real
  // GPU worker: the engine's appearance mode (rtp_set_track_appearance).  Otherwise the re-orderer runs rtp_appearance_describe on the
  // frame's display image, which the producer or the worker keeps for it, and rtp_track_update_appearance where it runs rtp_track_update.
  bool track_appearance = false;
  double appearance_weight = 0.125, appearance_max_dist = 1.0;
  int appearance_rate = 32;
  std::string appearance_parts = "torso";
  // --smooth (needs --track): every tracked person's parts through the One-Euro filter, parts that drop out held for --smooth_max_hold
  // frames.  One real GPU worker: the engine's smoothing mode with both apply flags (the filter runs on the GPU behind the track kernel;
  // rendered frames and crops show the smoothed people).  Otherwise the re-orderer runs rtp_smooth_update behind rtp_track_update.
  bool smooth = false;
  double smooth_min_cutoff = 1.0 / 30.0, smooth_beta = 0.01, smooth_d_cutoff = 1.0 / 30.0;
  int smooth_max_hold = 5;
  // --draw_tracks (needs --track and --write_frames or --write_video): a box, an id label and a fading trail per tracked person in the
  // rendered frames.  One real GPU worker: the engine's overlay mode (drawn on the GPU before the frame is encoded or converted there).
  // Otherwise, or with --host_draw: the re-orderer draws with rtp_overlay_update + rtp_overlay_draw on the raw rendered frame.
  bool draw_tracks = false, host_draw = false;
  std::string draw_what = "box,label,trail";
  int trail_len = 16, label_scale = 1, draw_alpha = 192;
  // --redact (needs --write_frames or --write_video): every person's head (or the region around --redact_parts) mosaicked, blurred or
  // filled in the rendered frames.  One real GPU worker: the engine's redaction mode (on the GPU, behind the pose overlay and in front of
  // --draw_tracks' drawing, before the frame is encoded or converted there).  Otherwise, or with --host_redact: the re-orderer applies
  // rtp_redact_regions + rtp_redact_apply to the raw rendered frame, before any rtp_overlay_draw.
  bool redact = false, host_redact = false;
  std::string redact_effect = "mosaic", redact_shape = "ellipse", redact_parts = "head";
  int redact_cell = 8, redact_radius = 8, redact_pad = 2;
  double redact_scale = 1.5, redact_aspect = 1.25;
  std::string caffemodel = "model/coco/pose_iter_440000.caffemodel", caffeproto = "model/coco/pose_deploy_linevec.prototxt";
  std::string resolution = "1280x720", net_resolution = "656x368", camera_resolution = "1280x720";
  double start_scale = 1, scale_gap = 0.3;
  // extensions (not in the reference)
  std::string precision = "mixed", model = "";  // --model coco|mpi: use the built-in graph + synthetic weights
  int frames_in_flight = 2, batch_frames = 1;
  unsigned long long synthetic_seed = 1;
  std::string devices;           // "0,0,1": device of worker i (default start_device + i); lets two workers share one GPU
  int test_worker_delay_ms = 0;  // test hook: every worker sleeps this long after a submit (provokes the >0.1 s frame drops)
  // --dry_engine RATE: no GPU.  Every worker is a stand-in that copies the frame like rtp_submit_frame's staging copy and
  // completes frames at RATE frames/s (pipelined, frames_in_flight deep) with --dry_people fake people each: the host side of
  // --num_gpu N (producer -> queue -> workers -> re-orderer -> writer) can be driven at N x the measured per-GPU rate on any box.
  double dry_engine = 0;
  int dry_people = 5;
  int producer_threads = 0;      // frames are generated / decoded ahead by this many threads (0 = hardware threads / 4, clamped to [2, 16])
  bool share_weights = false;    // workers 1.. take worker 0's PACKED weight arena device to device (rtp_copy_weights_from: hipMemcpyPeer over xGMI)
                                 // instead of keeping the copy they packed themselves (the reference: one .caffemodel read per GPU thread, rtpose.cpp:183-184)
  bool pin_workers = true;       // every worker thread runs on the CPUs local to its GPU (rtp_device_local_cpus), so the pinned staging buffers it
                                 // allocates and fills are on that NUMA node; --nopin_workers leaves the placement to the scheduler
  int calibrate = 0;             // K > 0: rtp_calibrate_precision on K frames right after the weights are loaded (mixed precision only)
  int json_writers = -1;         // JSON files are written by this many threads (0 = by the display/writer thread itself, like the reference;
                                 // default: 1 thread per worker — creating a file costs the one display thread ~0.5 ms, 1600 frames/s at most)
};

int parse_flags(int argc, char** argv, Flags& F) {
  std::map<std::string, std::string*> sflags = {{"write_frames", &F.write_frames}, {"write_json", &F.write_json}, {"video", &F.video}, {"write_video", &F.write_video}, {"write_heatmaps", &F.write_heatmaps}, {"heatmap_channels", &F.heatmap_channels},
      {"write_crops", &F.write_crops}, {"crop_size", &F.crop_size}, {"crop_parts", &F.crop_parts}, {"draw_what", &F.draw_what},
      {"redact_effect", &F.redact_effect}, {"redact_shape", &F.redact_shape}, {"redact_parts", &F.redact_parts}, {"appearance_parts", &F.appearance_parts},
      {"image_dir", &F.image_dir}, {"caffemodel", &F.caffemodel}, {"caffeproto", &F.caffeproto}, {"resolution", &F.resolution},
      {"net_resolution", &F.net_resolution}, {"camera_resolution", &F.camera_resolution}, {"precision", &F.precision}, {"model", &F.model}, {"devices", &F.devices}};
  std::map<std::string, int*> iflags = {{"part_to_show", &F.part_to_show}, {"camera", &F.camera}, {"start_frame", &F.start_frame},
      {"start_device", &F.start_device}, {"num_gpu", &F.num_gpu}, {"num_scales", &F.num_scales}, {"frames_in_flight", &F.frames_in_flight}, {"batch_frames", &F.batch_frames},
      {"test_worker_delay_ms", &F.test_worker_delay_ms}, {"dry_people", &F.dry_people}, {"json_writers", &F.json_writers}, {"producer_threads", &F.producer_threads}, {"calibrate", &F.calibrate}, {"video_fps", &F.video_fps}, {"max_crops", &F.max_crops},
      {"track_max_misses", &F.track_max_misses}, {"track_min_parts", &F.track_min_parts}, {"appearance_rate", &F.appearance_rate}, {"smooth_max_hold", &F.smooth_max_hold},
      {"trail_len", &F.trail_len}, {"label_scale", &F.label_scale}, {"draw_alpha", &F.draw_alpha},
      {"redact_cell", &F.redact_cell}, {"redact_radius", &F.redact_radius}, {"redact_pad", &F.redact_pad}};
  std::map<std::string, double*> dflags = {{"start_scale", &F.start_scale}, {"scale_gap", &F.scale_gap}, {"dry_engine", &F.dry_engine}, {"crop_margin", &F.crop_margin}, {"track_max_cost", &F.track_max_cost}, {"appearance_weight", &F.appearance_weight}, {"appearance_max_dist", &F.appearance_max_dist},
      {"smooth_min_cutoff", &F.smooth_min_cutoff}, {"smooth_beta", &F.smooth_beta}, {"smooth_d_cutoff", &F.smooth_d_cutoff},
      {"redact_scale", &F.redact_scale}, {"redact_aspect", &F.redact_aspect}};
  std::map<std::string, bool*> bflags = {{"fullscreen", &F.fullscreen}, {"no_frame_drops", &F.no_frame_drops}, {"host_preprocess", &F.host_preprocess}, {"host_jpeg", &F.host_jpeg}, {"host_video", &F.host_video}, {"host_yuv", &F.host_yuv}, {"host_decode", &F.host_decode}, {"gpu_decode", &F.gpu_decode}, {"no_display", &F.no_display}, {"track", &F.track}, {"track_appearance", &F.track_appearance}, {"smooth", &F.smooth}, {"draw_tracks", &F.draw_tracks}, {"host_draw", &F.host_draw}, {"redact", &F.redact}, {"host_redact", &F.host_redact},
      {"no_text", &F.no_text}, {"logtostderr", &F.logtostderr}, {"share_weights", &F.share_weights}, {"pin_workers", &F.pin_workers}};
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--help" || a == "-help" || a == "-h") return 2;
    if (a.size() < 2 || a[0] != '-') { fprintf(stderr, "ERROR: unexpected argument '%s'\n", a.c_str()); return 1; }
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string val;
    bool has_val = false;
    const size_t eq = a.find('=');
    if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_val = true; }
    if (bflags.count(a)) {
      if (has_val) *bflags[a] = (val == "true" || val == "1");
      else *bflags[a] = true;
      continue;
    }
    if (a.rfind("no", 0) == 0 && bflags.count(a.substr(2)) && !has_val) { *bflags[a.substr(2)] = false; continue; }  // gflags --noflag
    if (!sflags.count(a) && !iflags.count(a) && !dflags.count(a) && a != "synthetic_seed") {
      fprintf(stderr, "ERROR: unknown command line flag '%s'\n", a.c_str());
      return 1;
    }
    if (!has_val) {
      if (i + 1 >= argc) { fprintf(stderr, "ERROR: flag '%s' is missing its argument\n", a.c_str()); return 1; }
      val = argv[++i];
    }
    if (sflags.count(a)) *sflags[a] = val;
    else if (iflags.count(a)) *iflags[a] = atoi(val.c_str());
    else if (dflags.count(a)) *dflags[a] = atof(val.c_str());
    else F.synthetic_seed = strtoull(val.c_str(), nullptr, 10);
  }
  return 0;
}

void usage() {
  printf("rtpose.bin (MI355X engine) — flags as examples/rtpose/rtpose.cpp:\n"
         "  --video FILE.y4m|FILE.mjpeg|synthetic:WxH:frames[:seed]   --image_dir DIR (jpg/png/bmp/ppm)   --camera N (unsupported)\n"
         "  --caffeproto FILE --caffemodel FILE   | --model coco|mpi (built-in graph, synthetic weights)\n"
         "  --resolution WxH (1280x720) --net_resolution WxH (656x368) --num_scales N (1) --scale_gap G (0.3) --start_scale S (1)\n"
         "  --num_gpu N (1) --start_device D (0) --no_frame_drops --write_json DIR --write_frames DIR --start_frame N\n"
         "  --no_display --no_text --fullscreen --part_to_show N --logtostderr   [--precision mixed|fp16|f16x3|fp32 --frames_in_flight K --batch_frames B --host_preprocess\n"
         "   --devices d0,d1,.. (device of each worker; the same device may appear twice)\n"
         "   --dry_engine RATE (no GPU: every worker is a stand-in finishing RATE frames/s; measures the host side of --num_gpu N) --dry_people P\n"
         "   --json_writers K (JSON files written by K threads instead of the one display thread) --producer_threads K (decode / generate ahead)\n"
         "   --calibrate K (check / widen the mixed-precision split set on the loaded weights with K sample frames)\n"
         "   --share_weights (workers 1.. copy worker 0's packed weights GPU to GPU) --nopin_workers (no CPU affinity next to each worker's GPU)]\n"
         "  --write_frames draws the pose overlay only: the FPS / people-count text of the reference (cv::putText, rtpose.cpp:1319-1333) is not\n"
         "  drawn, i.e. --no_text is implied.  Its JPEG files (quality 98) are encoded on the GPU and only the files cross PCIe;\n"
         "  --host_jpeg copies the raw frames to the host and encodes them there on 8 threads instead (the same bytes).\n"
         "  --write_video FILE.y4m|FILE.mjpeg|FILE.mjpg [--video_fps N (30)] writes the same rendered frames as ONE stream, in frame order.\n"
         "  .y4m: converted to YUV 4:2:0 on the GPU (BT.601 limited range), only the planes cross PCIe; not together with --write_frames (one\n"
         "  renderer mode at a time).  .mjpeg / .mjpg: the JPEG files of --write_frames one after the other (may be combined with it).\n"
         "  --host_video copies the raw frames to the host and converts / encodes them there instead (the same bytes; the only path under\n"
         "  --dry_engine).  Without --no_frame_drops the stream simply holds the frames that were processed: dropped frames leave no gap.\n"
         "  --write_heatmaps PREFIX [--heatmap_channels parts|bkg|parts+bkg|pafs|all (parts+bkg)] writes every frame's part-confidence maps /\n"
         "  PAFs at net resolution as PREFIX%%06d.pgm (binary P5, net_w x channels * net_h, channel k in rows [k * net_h, (k + 1) * net_h)), in frame\n"
         "  order: u8, confidence and background as round(255 v), PAF channels as round(127.5 (v + 1)); evaluated and quantised on the GPU\n"
         "  (maps mode of the engine), only the bytes cross PCIe.  Under --dry_engine the files hold zeros.\n"
         "  --write_crops PREFIX [--crop_size WxH (128x128)] [--crop_parts all|head|p0,p1,.. (all)] [--crop_margin F (0.15)] [--max_crops N (16)]\n"
         "  writes a fixed-size crop of the un-rendered display image around each of the first N people as PREFIX%%06d_%%02d.ppm (binary P6;\n"
         "  %%02d = the person's index; only people with a box get a file) and every frame's boxes as PREFIX%%06d_boxes.json, in frame order.\n"
         "  The box spans the listed parts (head = nose, eyes and ears; MPI: head and neck), grown by F * its larger side and widened to the\n"
         "  crop's aspect; boxes and crops are computed on the GPU (crops mode of the engine) and equal rtp_crop_people bit for bit.\n"
         "  With --host_preprocess the engine never sees the display image: boxes only.  Under --dry_engine the box files hold no boxes.\n"
         "  --track [--track_max_cost F (0.0625)] [--track_max_misses N (15)] [--track_min_parts N (3)] follows people across frames: every\n"
         "  --write_json body gains \"id\":N in front of \"joints\" and every --write_crops box record \"id\":N (0 = not tracked: too few parts,\n"
         "  or all 128 tracks taken).  A person keeps its id while it is matched to its track: the mean squared displacement of the parts both\n"
         "  have, over the track's squared diagonal, must be <= F; a track unmatched for more than N frames is dropped.  With ONE real GPU worker\n"
         "  the association runs on the GPU behind the connect kernels (tracking mode of the engine, frames in submit order).  With --num_gpu N > 1,\n"
         "  --dry_engine or --host_preprocess the re-orderer, which sees the frames in order, runs the same definition on the host\n"
         "  (rtp_track_update): the ids are the same.  Frames dropped without --no_frame_drops are simply not seen by the tracker.  Without\n"
         "  --track every file is what it was.\n"
         "  --track_appearance [--appearance_weight F (0.125)] [--appearance_max_dist F (1)] [--appearance_rate N (32, of 256)]\n"
         "  [--appearance_parts torso|all|LIST] (needs --track) adds a look at the pixels to the association: per person two 64-bin colour\n"
         "  histograms (upper and lower half of a 32 x 32 sample grid over the box of the listed parts, in the un-rendered display image), per\n"
         "  track a histogram that moves N / 256 of the way to the matched person's every frame, and F times their L1 distance (0 .. 1) added\n"
         "  to the motion cost; a pair further apart than --appearance_max_dist is no match.  Two people who swap places between two frames keep\n"
         "  their ids.  With ONE real GPU worker it runs on the GPU (appearance mode of the engine).  With --num_gpu N > 1, --dry_engine or\n"
         "  --host_preprocess the re-orderer runs the same definitions on the host (rtp_appearance_describe, rtp_track_update_appearance) on the\n"
         "  frame's display image (video files and --gpu_decode then hand the workers BGR frames, as under --host_yuv / --host_decode): the same\n"
         "  ids.  The files carry the ids as with --track alone.\n"
         "  --smooth [--smooth_min_cutoff F (1/30)] [--smooth_beta F (0.01)] [--smooth_d_cutoff F (1/30)] [--smooth_max_hold N (5)] (needs --track)\n"
         "  filters every tracked person's parts over time (One-Euro filter, cutoffs in cycles per frame, beta per pixel) and holds a part that\n"
         "  dropped out at its last filtered value for up to N frames: the --write_json bodies then hold the smoothed joints.  With ONE real GPU\n"
         "  worker the filter runs on the GPU behind the track kernel (smoothing mode of the engine, both apply flags), and --write_crops,\n"
         "  --write_frames and --write_video show the smoothed people.  With --num_gpu N > 1, --dry_engine or --host_preprocess the re-orderer\n"
         "  runs the same definition on the host (rtp_smooth_update behind rtp_track_update): the JSON files are the same, frames and crops\n"
         "  are drawn from the raw joints.  Without --smooth every file is what it was.\n"
         "  --draw_tracks [--draw_what box,label,trail] [--trail_len N (16)] [--label_scale N (1)] [--draw_alpha N (192, of 256)] [--host_draw]\n"
         "  (needs --track and --write_frames or --write_video) draws every tracked person's box, id and a fading trail of its last N positions\n"
         "  into the rendered frames, in a colour derived from the id.  With ONE real GPU worker the drawing runs on the GPU behind the track\n"
         "  kernel (overlay mode of the engine), and the GPU's JPEG encoder / YUV conversion stay in use.  With --num_gpu N > 1 or --dry_engine\n"
         "  the ids exist only in the re-orderer, which then draws on the raw rendered frame with the same definition (rtp_overlay_update +\n"
         "  rtp_overlay_draw: the same pixels), and the host encoders write the files, as with --host_jpeg / --host_video.  --host_draw asks\n"
         "  for that path with one GPU worker too: it is there to compare the two paths (the tests do), nothing is gained by it otherwise.  (--host_preprocess renders no frames at all.)  Without --draw_tracks every file is what it was.\n"
         "  --redact [--redact_effect mosaic|blur|fill (mosaic)] [--redact_shape ellipse|rect (ellipse)] [--redact_parts head|all|p0,p1,.. (head)]\n"
         "  [--redact_cell N (8: 2, 4, 8, 16 or 32)] [--redact_radius N (8: 1 .. 16)] [--redact_scale F (1.5)] [--redact_aspect F (1.25)] [--redact_pad N (2)]\n"
         "  [--host_redact] (needs --write_frames or --write_video) anonymises the rendered frames: around the listed parts of every person (the\n"
         "  head's by default) an ellipse or rectangle of half-width F x half the parts' span + N pixels, F times as tall as wide, is replaced\n"
         "  by a mosaic of N x N cells, a box blur of radius N or black (F is converted once: (int)lrintf(F * 256)).  With ONE real GPU worker\n"
         "  it runs on the GPU (redaction mode of the engine) behind the pose overlay and in front of --draw_tracks' drawing, so boxes and ids stay\n"
         "  sharp, and the GPU's JPEG encoder / YUV conversion stay in use: only the anonymised, encoded frame crosses PCIe.  With --num_gpu N > 1,\n"
         "  --dry_engine or --host_redact the re-orderer applies the same definition (rtp_redact_regions + rtp_redact_apply: the same bytes) to\n"
         "  the raw rendered frame, before any rtp_overlay_draw, and the host encoders write the files.  --write_crops and --write_heatmaps\n"
         "  are NOT redacted.  Without --redact every file is what it was.\n"
         "  --video FILE.y4m hands the file's Y, U, V planes to the engine (rtp_submit_frame_yuv: 1.5 bytes per pixel cross PCIe for 4:2:0,\n"
         "  the colour conversion runs on the GPU); --host_yuv converts to BGR on the producer thread instead (the same output).\n"
         "  --video FILE.mjpeg hands every frame's FILE bytes to the engine (rtp_submit_frame_jpeg: the producer only reads the file and its\n"
         "  header; Huffman decoding, IDCT, up-sampling and colour conversion run on the GPU); --host_decode decodes on the producer thread\n"
         "  instead.  --image_dir *.jpg|*.jpeg decodes on the producer pool (faster than the GPU decoder where host cores are free);\n"
         "  --gpu_decode hands those files' bytes to the engine as well.  Same output either way; a file whose scan is corrupt is skipped.\n");
}

// ---- queues (caffe::BlockingQueue, util/blocking_queue.cpp:26-61) -----------------------------
template <typename T> class BlockingQueue {
 public:
  void push(T v) { { std::lock_guard<std::mutex> l(m_); q_.push_back(std::move(v)); } cv_.notify_one(); }
  bool try_pop(T* v) { std::lock_guard<std::mutex> l(m_); if (q_.empty()) return false; *v = std::move(q_.front()); q_.pop_front(); return true; }
  bool pop_wait(T* v, std::atomic<bool>& quit) {
    std::unique_lock<std::mutex> l(m_);
    while (q_.empty()) { if (quit.load()) return false; cv_.wait_for(l, std::chrono::milliseconds(2)); }
    *v = std::move(q_.front()); q_.pop_front();
    return true;
  }
  size_t size() { std::lock_guard<std::mutex> l(m_); return q_.size(); }
 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<T> q_;
};

// include/caffe/cpm/frame.h:6-34
struct Frame {
  std::vector<float> data;         // net input (only with --host_preprocess)
  std::vector<unsigned char> image;  // decoded u8 BGR frame (default: pre-processing runs on the GPU), or — yuv — the planes of a Y4M frame
  bool jpeg = false;               // image = the bytes of a JPEG file (img_w x img_h from its header): decoded on the GPU (rtp_submit_frame_jpeg)
  bool yuv = false;                // image = Y (img_w x img_h), then U and V ((img_w + sx) >> sx by (img_h + sy) >> sy each; none for mono)
  int chroma_sx = 0, chroma_sy = 0;
  bool mono = false;
  std::vector<unsigned char> heatmaps;  // --write_heatmaps: the frame's u8 maps [nch][net_h][net_w] (rtp_peek_maps)
  std::vector<float> crop_boxes;        // --write_crops: the frame's box records [crop_n][RTP_CROP_BOX_FLOATS] and its crops (HWC BGR; empty
  std::vector<unsigned char> crops;     // for a frame without a display image) (rtp_peek_crops); crop_n < 0: not a --write_crops run
  int crop_n = -1;
  std::vector<float> joints_s;          // --smooth: the frame's smoothed joints [numPeople][num_parts][3] (rtp_peek_smoothed, or the re-orderer's rtp_smooth_update)
  std::vector<unsigned char> display;   // --track_appearance in the re-orderer: the frame's un-rendered display image (DISP_W x DISP_H BGR); display_raw:
  bool display_raw = false;             // the BGR frame itself (img_w x img_h), which the re-orderer warps to the display image first
  std::vector<int> track_recs;          // --track: the frame's records [numPeople][RTP_TRACK_REC_INTS] (rtp_peek_tracks, or the re-orderer's rtp_track_update)
  std::vector<unsigned char> rendered;  // --write_frames: display-resolution frame with the pose overlay (or its JPEG file: rendered_jpeg)
  bool rendered_jpeg = false;
  bool rendered_yuv = false;            // --write_video x.y4m: rendered holds the frame's 4:2:0 planes (rtp_collect_rendered_yuv)
  int img_w = 0, img_h = 0;
  double commit_time = 0, preprocessed_time = 0, gpu_fetched_time = 0, gpu_computed_time = 0, buffer_start_time = 0, buffer_end_time = 0;
  int index = 0, numPeople = 0, video_frame_number = 0;
  float scale = 1.f;
  std::string stem;
  std::vector<float> joints;
};

bool track_on_gpu();
rtp_track_config track_config();
bool appearance_on_host();
rtp_appearance_config appearance_config(int num_parts, std::vector<int>* parts);
bool smooth_on_gpu();
rtp_smooth_config smooth_config();
bool overlay_on_gpu();
rtp_overlay_config overlay_config();
bool redact_on_gpu();
bool host_pixels();
rtp_redact_config redact_config(int num_parts, std::vector<int>* parts);

struct EncodeJob { std::string path; std::vector<unsigned char> bgr; bool jpeg = false; };  // jpeg: bgr already holds the file

struct Global {
  BlockingQueue<Frame> input_queue, output_queue, output_queue_ordered;
  BlockingQueue<EncodeJob> encode_queue;  // --write_frames: JPEG encoding is spread over a few threads (files are independent)
  std::atomic<bool> encode_done{false};
  rtp_video_out* video_out = nullptr;     // --write_video: written by the display thread only
  int video_kind = 0;                     // RTP_VIDEO_Y4M / RTP_VIDEO_MJPEG
  std::atomic<bool> video_failed{false};
  std::priority_queue<int, std::vector<int>, std::greater<int>> dropped_index;
  std::mutex mutex;
  std::atomic<bool> quit_threads{false};
  std::atomic<int> produced{0}, finished{0}, dropped{0};
  std::vector<int> per_worker;  // frames each worker submitted (dynamic pull from the one shared queue)
  std::atomic<rtp_engine*> engine0{nullptr};  // --share_weights: worker 0's engine once it is up (idle until every worker is ready)
  std::atomic<int> weights_shared{0};
  std::atomic<int> share_done{0};      // receiving workers that are through with worker 0's engine (copied, or failed): worker 0 keeps it alive until all are
  std::atomic<int> workers_ready{0};  // workers start pulling once EVERY engine is up (engine creation takes seconds, short inputs milliseconds)
  std::atomic<bool> producer_done{false};
  double first_commit = 0;                     // steady-state window: first frame committed .. last file written
  std::atomic<double> last_written{0};         // (by the display thread, or by whichever JSON writer finished last)
  BlockingQueue<Frame> json_queue;             // --json_writers K
  std::atomic<bool> json_done{false};
  std::atomic<int> num_parts{18};              // every worker stores the same value (its engine's) while the JSON writers read it
  std::vector<std::string> image_list;
};

Flags F;
Global G;
int DISP_W, DISP_H, NET_W, NET_H;
const int BUFFER_SIZE = 4;  // rtpose.cpp:90

bool mkdir_p(const std::string& d) { struct stat st; if (stat(d.c_str(), &st) == 0) return S_ISDIR(st.st_mode); return mkdir(d.c_str(), 0755) == 0; }

// ---- producer -----------------------------------------------------------------------------------
void producer() {
  int global_counter = 1;
  int sw = 0, sh = 0, nframes = 0;
  unsigned long long seed = 2;
  const bool synthetic = F.video.rfind("synthetic:", 0) == 0;
  rtp_video* vid = nullptr;
  if (synthetic) {
    if (sscanf(F.video.c_str(), "synthetic:%dx%d:%d:%llu", &sw, &sh, &nframes, &seed) < 3) { fprintf(stderr, "bad --video %s\n", F.video.c_str()); G.quit_threads = true; return; }
  } else if (!F.video.empty()) {  // cv::VideoCapture(FLAGS_video), rtpose.cpp:402-411
    if (rtp_video_open(F.video.c_str(), &vid, &sw, &sh, &nframes) != RTP_OK) { fprintf(stderr, "Couldn't open video file %s: %s\n", F.video.c_str(), rtp_codec_last_error()); G.quit_threads = true; G.producer_done = true; return; }
    if (nframes < 0) nframes = 1 << 30;
    std::vector<unsigned char> skip((size_t)sw * sh * 3);
    for (int i = 0; i < F.start_frame; ++i) if (rtp_video_read(vid, skip.data(), skip.size()) != RTP_OK) break;  // CAP_PROP_POS_FRAMES, :411
  } else nframes = (int)G.image_list.size();
  // Y4M: the planes go to the engine as they are in the file, unless the frames do not reach rtp_submit_frame at all (--host_preprocess,
  // --dry_engine), --host_yuv asks for the host conversion, or this binary was linked without the entry
  const bool yuv_planes = vid && rtp_video_chroma(vid) != 0 && !F.host_yuv && !F.host_preprocess && !(F.dry_engine > 0) && !appearance_on_host() && rtp_submit_frame_yuv != nullptr;   // (--track_appearance in the re-orderer describes people on the BGR frame)
  // JPEG files go to the engine as they are on disk (the same exceptions; --host_decode asks for the host decoder)
  const bool jpeg_can = !F.host_decode && !F.host_preprocess && !(F.dry_engine > 0) && !appearance_on_host() && rtp_submit_frame_jpeg != nullptr;
  const bool jpeg_files = jpeg_can && F.gpu_decode;                           // --image_dir: the producer pool unless asked
  const bool mjpeg_bytes = vid && rtp_video_chroma(vid) == 0 && jpeg_can;     // --video x.mjpeg: the GPU unless asked
  std::vector<unsigned char> img;
  // --image_dir files and synthetic frames are produced a few ahead by a small pool (a 720p JPEG takes ~13 ms on one core, a
  // synthetic frame ~1 ms; 8 GPUs at 1 scale want ~8000 frames/s); the producer still hands the frames over in index order,
  // like the reference's single loop.  Video files are read sequentially (one decoder state).
  struct Decoded { std::vector<unsigned char> bgr; int w = 0, h = 0; std::string err; bool jpeg = false; };   // jpeg: bgr holds the file
  const int hw = (int)std::thread::hardware_concurrency();
  const int pool_n = (synthetic || vid == nullptr) ? (F.producer_threads > 0 ? std::min(F.producer_threads, 64) : std::max(2, std::min(16, hw / 4))) : 0;
  const int window = 4 * std::max(pool_n, 1);
  std::mutex pm;
  std::condition_variable pcv;
  std::map<int, Decoded> ready;            // frame index -> frame, filled by the pool
  int next_job = F.start_frame, consumed = F.start_frame;
  bool pool_quit = false;
  auto make_frame = [&](int fi) {
    Decoded d;
    if (synthetic) {
      d.w = sw; d.h = sh;
      d.bgr.resize((size_t)sw * sh * 3);
      rtp_synth_frame(d.bgr.data(), sw, sh, fi, seed);
    } else {
      const std::string& path = G.image_list[fi];
      const size_t dot = path.find_last_of('.');
      std::string ext = dot == std::string::npos ? "" : path.substr(dot);
      for (char& ch : ext) ch = (char)tolower((unsigned char)ch);
      if (jpeg_files && (ext == ".jpg" || ext == ".jpeg")) {   // the file and its header only
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) { d.err = "cannot read the file"; return d; }
        unsigned char chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) d.bgr.insert(d.bgr.end(), chunk, chunk + got);
        fclose(f);
        if (rtp_decode_image(d.bgr.data(), d.bgr.size(), nullptr, 0, &d.w, &d.h) != RTP_OK) { d.err = rtp_codec_last_error(); d.w = 0; return d; }
        d.jpeg = true;
        return d;
      }
      if (rtp_load_image(path.c_str(), nullptr, 0, &d.w, &d.h) != RTP_OK) { d.err = rtp_codec_last_error(); d.w = 0; return d; }
      d.bgr.resize((size_t)d.w * d.h * 3);
      if (rtp_load_image(path.c_str(), d.bgr.data(), d.bgr.size(), &d.w, &d.h) != RTP_OK) { d.err = rtp_codec_last_error(); d.w = 0; }
    }
    return d;
  };
  std::vector<std::thread> pool;
  for (int t = 0; t < pool_n; ++t)
    pool.emplace_back([&]() {
      while (true) {
        int fi;
        {
          std::unique_lock<std::mutex> l(pm);
          pcv.wait(l, [&] { return pool_quit || (next_job < nframes && next_job < consumed + window); });
          if (pool_quit) return;
          fi = next_job++;
        }
        Decoded d = make_frame(fi);
        { std::lock_guard<std::mutex> l(pm); ready[fi] = std::move(d); }
        pcv.notify_all();
      }
    });
  while (G.workers_ready.load() < F.num_gpu && !G.quit_threads) std::this_thread::sleep_for(std::chrono::milliseconds(1));  // no frame ages while the engines start
  for (int fi = F.start_frame; fi < nframes && !G.quit_threads; ++fi) {
    // back-pressure (rtpose.cpp:311, 424-429); the queue bound follows the number of consumers
    while ((int)G.input_queue.size() > 10 + 4 * F.num_gpu && !G.quit_threads) std::this_thread::sleep_for(std::chrono::microseconds(200));
    Frame fr;
    int w = sw, h = sh;
    if (vid) {
      int rc;
      if (yuv_planes) {   // the view points into the reader's buffer (valid until the next read): Y, U, V back to back
        rtp_yuv_view yv;
        rc = rtp_video_read_yuv(vid, &yv);
        if (rc == RTP_OK) {
          const size_t cw = (size_t)(w + yv.chroma_shift_x) >> yv.chroma_shift_x, ch = (size_t)(h + yv.chroma_shift_y) >> yv.chroma_shift_y;
          fr.yuv = true;
          fr.mono = yv.u == nullptr;
          fr.chroma_sx = yv.chroma_shift_x; fr.chroma_sy = yv.chroma_shift_y;
          const unsigned char* p = (const unsigned char*)yv.y;
          img.assign(p, p + (size_t)w * h + (fr.mono ? 0 : 2 * cw * ch));
        }
      } else if (mjpeg_bytes) {   // the frame's byte range inside the reader's copy of the file
        const unsigned char* jb = nullptr;
        size_t jn = 0;
        rc = rtp_video_read_jpeg(vid, &jb, &jn);
        if (rc == RTP_OK) rc = rtp_decode_image(jb, jn, nullptr, 0, &w, &h);
        if (rc == RTP_OK && (w != sw || h != sh)) { fprintf(stderr, "video frame %d: MJPEG: frame size changes inside the stream\n", fi); break; }   // (as rtp_video_read)
        if (rc == RTP_OK) { img.assign(jb, jb + jn); fr.jpeg = true; }
      } else {
        img.resize((size_t)w * h * 3);
        rc = rtp_video_read(vid, img.data(), img.size());
      }
      if (rc == RTP_EAGAIN) break;  // end of the stream
      if (rc != RTP_OK) { fprintf(stderr, "video frame %d: %s\n", fi, rtp_codec_last_error()); break; }
      char nm[64]; snprintf(nm, sizeof nm, "frame%06d", fi); fr.stem = nm;
    } else {
      Decoded d;
      {
        std::unique_lock<std::mutex> l(pm);
        pcv.wait(l, [&] { return ready.count(fi) != 0; });
        d = std::move(ready[fi]);
        ready.erase(fi);
        consumed = fi + 1;
      }
      pcv.notify_all();
      if (d.w == 0) { fprintf(stderr, "cannot decode %s: %s\n", G.image_list[fi].c_str(), d.err.c_str()); continue; }
      img.swap(d.bgr);
      w = d.w; h = d.h;
      fr.jpeg = d.jpeg;
      if (synthetic) { char nm[64]; snprintf(nm, sizeof nm, "frame%06d", fi); fr.stem = nm; }
      else {
        const std::string& path = G.image_list[fi];
        size_t sl = path.find_last_of('/'), dot = path.find_last_of('.');
        fr.stem = path.substr(sl == std::string::npos ? 0 : sl + 1, dot - (sl == std::string::npos ? 0 : sl + 1));
      }
    }
    fr.commit_time = wall();
    if (F.host_preprocess) {
      fr.data.resize((size_t)F.num_scales * 3 * NET_H * NET_W);
      if (appearance_on_host()) fr.display.resize((size_t)DISP_W * DISP_H * 3);   // the re-orderer describes people on it
      if (rtp_preprocess_frame(img.data(), w, h, DISP_W, DISP_H, NET_W, NET_H, F.num_scales, F.start_scale, F.scale_gap, fr.data.data(),
                               fr.display.empty() ? nullptr : fr.display.data(), &fr.scale) != RTP_OK) {
        fprintf(stderr, "preprocess failed for frame %d\n", fi);
        continue;
      }
    } else {
      fr.image = std::move(img);   // handed over, not copied (2.76 MB per 720p frame)
      img.clear();
      fr.img_w = w;
      fr.img_h = h;
    }
    fr.index = global_counter++;
    fr.video_frame_number = fi;
    fr.preprocessed_time = wall();
    if (G.first_commit == 0) G.first_commit = fr.commit_time;
    G.produced++;
    G.input_queue.push(std::move(fr));
  }
  { std::lock_guard<std::mutex> l(pm); pool_quit = true; }
  pcv.notify_all();
  for (auto& t : pool) t.join();
  if (vid) rtp_video_close(vid);
  G.producer_done = true;
}

// CPU affinity of a worker thread: the CPUs local to its GPU's PCI function ("0-31,128-159"); silently skipped where sysfs does not say
void pin_thread_near_device(int widx, int device) {
  char list[512];
  if (rtp_device_local_cpus(device, list, sizeof list) <= 0) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  int n = 0;
  for (const char* p = list; *p;) {
    char* end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p) break;
    long b = a;
    p = end;
    if (*p == '-') { b = strtol(p + 1, &end, 10); p = end; }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET((int)c, &set); ++n; }
    if (*p == ',') ++p;
  }
  if (n > 0 && pthread_setaffinity_np(pthread_self(), sizeof set, &set) == 0) fprintf(stderr, "worker %d (GPU %d) runs on CPUs %s\n", widx, device, list);
}

// ---- per-GPU worker (processFrame, rtpose.cpp:1079-1203) -----------------------------------------
void worker(int widx, int device, int* status) {
  rtp_config cfg;
  rtp_config_default(&cfg);
  cfg.device_id = device;
  if (!F.model.empty()) cfg.model = (F.model == "mpi") ? RTP_MODEL_MPI_15 : RTP_MODEL_COCO_18;
  else { cfg.proto_path = F.caffeproto.c_str(); cfg.weights_path = F.caffemodel.c_str(); }
  cfg.synthetic_seed = F.synthetic_seed;
  cfg.net_w = NET_W; cfg.net_h = NET_H; cfg.num_scales = F.num_scales;
  cfg.start_scale = (float)F.start_scale; cfg.scale_gap = (float)F.scale_gap;
  cfg.disp_w = DISP_W; cfg.disp_h = DISP_H;
  cfg.precision = F.precision == "fp32" ? RTP_PREC_FP32 : F.precision == "fp16" ? RTP_PREC_FP16 : F.precision == "f16x3" ? RTP_PREC_F16X3 : RTP_PREC_MIXED;
  cfg.frames_in_flight = F.frames_in_flight;
  cfg.batch_frames = F.batch_frames;
  const bool want_render = !F.write_frames.empty() || !F.write_video.empty();
  cfg.render = !want_render ? 0 : 1 + F.part_to_show;  // render() of rtpose.cpp:270-299: pose overlay or a --part_to_show view
  cfg.calibrate_frames = F.calibrate;
  rtp_engine* e = nullptr;
  const bool dry = F.dry_engine > 0;
  if (!dry && F.pin_workers && F.num_gpu > 1) pin_thread_near_device(widx, device);
  // --share_weights: ONE read + pack of the model for N replicas.  Worker 0 loads (and, with --calibrate or a model file, calibrates);
  // the others wait for it, are created WITHOUT weights (rtp_config.defer_weights) on worker 0's final split set and take its packed
  // arena device to device before anybody submits a frame (worker 0's engine is idle until every worker is ready).
  std::vector<char> src_rules(1 << 16);   // (a calibrated rule list names layer groups: a few hundred bytes; rtp_get_split_layers refuses a buffer that is too small)
  rtp_engine* src = nullptr;
  struct ShareDone {   // counted on EVERY way out of this function once a receiving worker exists (worker 0 waits for the count before it destroys its engine)
    bool armed = false;
    ~ShareDone() { if (armed) G.share_done++; }
  } share_done_guard;
  if (!dry && F.share_weights && widx != 0) {
    share_done_guard.armed = true;
    while (!(src = G.engine0.load()) && !G.quit_threads) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (!src) { *status = 1; return; }   // worker 0 failed and everybody is quitting: nothing was copied, nothing is counted
    int prec = cfg.precision;
    if (rtp_get_split_layers(src, src_rules.data(), src_rules.size(), &prec) != RTP_OK) { fprintf(stderr, "GPU %d: --share_weights: %s\n", device, rtp_last_error(src)); *status = 1; G.quit_threads = true; return; }
    cfg.precision = prec;
    cfg.split_layers = src_rules.data();
    cfg.calibrate_frames = -1;
    cfg.defer_weights = 1;
  }
  if (!dry && rtp_engine_create(&cfg, &e) != RTP_OK) {
    fprintf(stderr, "GPU %d: %s\n", device, rtp_last_error(nullptr));
    *status = 1;
    G.quit_threads = true;
    return;
  }
  // --write_frames: the files are encoded on the GPU (quality 98, rtpose.cpp:1367-1381) unless --host_jpeg; --dry_engine has no GPU
  // --write_video x.mjpeg takes the same files (main() refuses the combinations in which one output wants the GPU's and the other the host's)
  // --draw_tracks or --redact in the re-orderer: it needs the raw frames, and the host encoders write the files
  const bool host_draw = host_pixels();
  const bool gpu_jpeg = !dry && !host_draw && ((!F.write_frames.empty() && !F.host_jpeg) || (G.video_kind == RTP_VIDEO_MJPEG && !F.host_video));
  // --write_video x.y4m: the renderer's YUV mode unless --host_video
  const bool gpu_yuv = !dry && !host_draw && G.video_kind == RTP_VIDEO_Y4M && !F.host_video;
  if (gpu_yuv) {
    const char* err = !rtp_set_render_yuv || !rtp_collect_rendered_yuv ? "this binary was linked without the engine's YUV output"
                      : rtp_set_render_yuv(e, 420) != RTP_OK            ? rtp_last_error(e) : nullptr;
    if (err) {   // never a quiet fall-back to the host conversion: --host_video asks for it
      fprintf(stderr, "GPU %d: --write_video: %s\n", device, err);
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  if (!F.write_video.empty() && widx == 0)
    fprintf(stderr, "--write_video: frames %s\n", gpu_yuv ? "converted to YUV 4:2:0 on the GPU (rtp_collect_rendered_yuv)"
                                                  : gpu_jpeg ? "encoded on the GPU (rtp_collect_rendered_jpeg)"
                                                             : "converted / encoded on the host (--host_video, or --draw_tracks / --redact in the re-orderer)");
  std::vector<unsigned char> jpeg_buf(gpu_jpeg ? rtp_jpeg_max_bytes(DISP_W, DISP_H) : 0);
  if (gpu_jpeg) {
    const char* err = !rtp_set_render_jpeg || !rtp_collect_rendered_jpeg ? "this binary was linked without the engine's GPU JPEG encoder"
                      : rtp_set_render_jpeg(e, 98) != RTP_OK              ? rtp_last_error(e) : nullptr;
    if (err) {   // never a quiet fall-back to the host encoders: --host_jpeg asks for them
      fprintf(stderr, "GPU %d: %s: %s\n", device, F.write_frames.empty() ? "--write_video" : "--write_frames", err);
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  if (!F.write_frames.empty() && widx == 0)
    fprintf(stderr, "--write_frames: JPEG files encoded %s\n", gpu_jpeg ? "on the GPU (rtp_collect_rendered_jpeg)" : "on the host (rtp_encode_jpeg, 8 threads)");
  // a frame whose collect failed: the host encoders write the file of the zero-filled frame they are handed, so the GPU path writes
  // that same file (encoded once by rtp_encode_jpeg): both modes leave the same file set
  std::vector<unsigned char> black_jpeg;
  if (!dry && F.share_weights) {
    if (widx == 0) G.engine0 = e;
    else {
      if (rtp_copy_weights_from(e, src) != RTP_OK) {
        fprintf(stderr, "GPU %d: --share_weights: %s\n", device, rtp_last_error(e));
        *status = 1;
        G.quit_threads = true;
        rtp_engine_destroy(e);
        return;
      }
      G.weights_shared++;
    }
    if (widx != 0) { share_done_guard.armed = false; G.share_done++; }   // through with worker 0's engine
  }
  int num_parts = F.model == "mpi" ? 15 : 18, heat_channels = F.model == "mpi" ? 44 : 57;
  if (!dry) rtp_engine_info(e, &num_parts, nullptr, &heat_channels, nullptr, nullptr);
  G.num_parts.store(num_parts);
  if (appearance_on_host()) {   // the re-orderer's configuration against the model's parts, refused here as rtp_set_track_appearance refuses it on the GPU path
    std::vector<int> parts;
    const rtp_appearance_config ac = appearance_config(num_parts, &parts);
    uint16_t no_bins[RTP_APPEARANCE_BINS];
    unsigned char no_valid[1];
    if (rtp_appearance_describe(nullptr, 1, 1, nullptr, 0, num_parts, &ac, no_bins, no_valid) != 0) {
      fprintf(stderr, "GPU %d: --track_appearance: --appearance_parts lists a part outside the model's %d parts\n", device, num_parts);
      *status = 1;
      G.quit_threads = true;
      if (e) rtp_engine_destroy(e);
      return;
    }
  }
  // --write_heatmaps: maps mode, u8 on the net grid; concat_stage7 holds the parts, the background, then the PAF channels
  size_t heat_bytes = 0;
  if (!F.write_heatmaps.empty()) {
    std::vector<int> chan;
    const std::string& hc = F.heatmap_channels;
    if (hc == "parts" || hc == "parts+bkg" || hc == "all") for (int c = 0; c < num_parts; ++c) chan.push_back(c);
    if (hc == "bkg" || hc == "parts+bkg" || hc == "all") chan.push_back(num_parts);
    if (hc == "pafs" || hc == "all") for (int c = num_parts + 1; c < heat_channels; ++c) chan.push_back(c);
    heat_bytes = chan.size() * (size_t)NET_W * NET_H;
    if (!dry) {
      rtp_maps_config mc;
      memset(&mc, 0, sizeof mc);
      mc.struct_size = sizeof mc;
      mc.grid = RTP_MAPS_GRID_NET; mc.format = RTP_MAPS_U8;
      mc.channels = chan.data(); mc.num_channels = (int)chan.size();
      const char* err = !rtp_set_maps_output || !rtp_peek_maps ? "this binary was linked without the engine's maps mode"
                        : rtp_set_maps_output(e, &mc) != RTP_OK ? rtp_last_error(e) : nullptr;
      if (err) {
        fprintf(stderr, "GPU %d: --write_heatmaps: %s\n", device, err);
        *status = 1;
        G.quit_threads = true;
        rtp_engine_destroy(e);
        return;
      }
    }
  }
  // --write_crops: crops mode, HWC BGR crops (the writer swaps to the RGB of a PPM file)
  int crop_w = 0, crop_h = 0;
  if (!F.write_crops.empty()) {
    rtp_crops_config cc;
    memset(&cc, 0, sizeof cc);
    cc.struct_size = sizeof cc;
    sscanf(F.crop_size.c_str(), "%dx%d", &cc.crop_w, &cc.crop_h);
    crop_w = cc.crop_w; crop_h = cc.crop_h;
    cc.max_crops = F.max_crops; cc.min_score = 0.f; cc.min_parts = 1; cc.margin = (float)F.crop_margin; cc.layout = RTP_CROPS_HWC_BGR;
    std::vector<int> parts;
    if (F.crop_parts == "head") {
      int hp[8];
      const int nh = rtp_crops_head_parts(num_parts == 15 ? RTP_MODEL_MPI_15 : RTP_MODEL_COCO_18, hp);
      parts.assign(hp, hp + std::max(nh, 0));
    } else if (F.crop_parts != "all") {
      for (const char* q = F.crop_parts.c_str(); *q;) {
        char* end = nullptr;
        parts.push_back((int)strtol(q, &end, 10));
        if (end == q) { parts.back() = -1; break; }
        q = *end == ',' ? end + 1 : end;
      }
    }
    if (!parts.empty()) { cc.parts = parts.data(); cc.num_parts = (int)parts.size(); }
    if (!dry) {
      const char* err = !rtp_set_crops_output || !rtp_peek_crops ? "this binary was linked without the engine's crops mode"
                        : rtp_set_crops_output(e, &cc) != RTP_OK ? rtp_last_error(e) : nullptr;
      if (err) {
        fprintf(stderr, "GPU %d: --write_crops: %s\n", device, err);
        *status = 1;
        G.quit_threads = true;
        rtp_engine_destroy(e);
        return;
      }
    }
  }
  // --track with one real GPU worker: the engine's tracking mode (otherwise the re-orderer tracks on the host)
  const bool gpu_track = track_on_gpu();
  if (gpu_track) {
    const rtp_track_config tc = track_config();
    if (rtp_set_tracking(e, &tc) != RTP_OK) {
      fprintf(stderr, "GPU %d: --track: %s\n", device, rtp_last_error(e));
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  // --track_appearance likewise: the engine's appearance mode (the describe kernel and the appearance form of the track kernel)
  if (gpu_track && F.track_appearance) {
    std::vector<int> parts;
    const rtp_appearance_config ac = appearance_config(num_parts, &parts);
    if (!rtp_set_track_appearance || rtp_set_track_appearance(e, &ac) != RTP_OK) {
      fprintf(stderr, "GPU %d: --track_appearance: %s\n", device, rtp_set_track_appearance ? rtp_last_error(e) : "this library has no appearance mode");
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  // --smooth likewise: the engine's smoothing mode, applied to the rendered frames and the crops
  const bool gpu_smooth = smooth_on_gpu();
  if (gpu_smooth) {
    const rtp_smooth_config sc = smooth_config();
    if (rtp_set_smoothing(e, &sc) != RTP_OK) {
      fprintf(stderr, "GPU %d: --smooth: %s\n", device, rtp_last_error(e));
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  // --draw_tracks likewise: the engine's overlay mode, drawn into the rendered frame before it is encoded or converted
  if (overlay_on_gpu()) {
    const rtp_overlay_config oc = overlay_config();
    if (rtp_set_track_overlay(e, &oc) != RTP_OK) {
      fprintf(stderr, "GPU %d: --draw_tracks: %s\n", device, rtp_last_error(e));
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  // --redact likewise: the engine's redaction mode, applied to the rendered frame in front of the overlay mode's drawing
  if (redact_on_gpu()) {
    std::vector<int> parts;
    const rtp_redact_config rc = redact_config(num_parts, &parts);
    if (rtp_set_redaction(e, &rc) != RTP_OK) {
      fprintf(stderr, "GPU %d: --redact: %s\n", device, rtp_last_error(e));
      *status = 1;
      G.quit_threads = true;
      rtp_engine_destroy(e);
      return;
    }
  }
  if (F.redact && widx == 0)
    fprintf(stderr, "--redact: %s\n", redact_on_gpu() ? "redaction on the GPU (rtp_set_redaction)" : "redaction in the re-orderer (rtp_redact_regions + rtp_redact_apply)");
  // --dry_engine: what the engine costs the HOST per frame (the staging copy of rtp_submit_frame, the joints copy of
  // rtp_collect) and when a frame completes (RATE frames/s, at least two frame times after its submit)
  std::vector<unsigned char> dry_staging;
  std::deque<double> dry_done;   // completion times of the frames in flight
  double dry_last = 0;
  auto dry_submit = [&](const Frame& fr) {
    const size_t n = F.host_preprocess ? fr.data.size() * sizeof(float) : fr.image.size();
    if (dry_staging.size() < n) dry_staging.resize(n);
    memcpy(dry_staging.data(), F.host_preprocess ? (const void*)fr.data.data() : (const void*)fr.image.data(), n);
    const double now = wall();
    dry_last = std::max(now + 2.0 / F.dry_engine, dry_last + 1.0 / F.dry_engine);
    dry_done.push_back(dry_last);
    return RTP_OK;
  };
  auto dry_collect = [&](Frame& fr, float* joints, int* n) {
    const double t = dry_done.front();
    dry_done.pop_front();
    for (double now = wall(); now < t; now = wall()) std::this_thread::sleep_for(std::chrono::duration<double>(std::min(t - now, 0.0005)));
    const int P = std::max(0, std::min(F.dry_people, (int)RTP_MAX_PEOPLE));
    unsigned long long r = 0x9E3779B97F4A7C15ull * (unsigned long long)(fr.index + 1);
    for (int i = 0; i < P * num_parts; ++i) {
      r ^= r << 13; r ^= r >> 7; r ^= r << 17;
      joints[3 * i] = (float)(r % 1280000) / 1000.f;
      joints[3 * i + 1] = (float)((r >> 20) % 720000) / 1000.f;
      joints[3 * i + 2] = (float)((r >> 40) % 1000) / 1000.f;
    }
    *n = P;
    if (!fr.rendered.empty()) memset(fr.rendered.data(), 40 + (fr.index * 7) % 160, fr.rendered.size());  // --write_frames: what the encoders get instead of rtp_collect_rendered's frame
    return RTP_OK;
  };
  fprintf(stderr, dry ? "dry worker %d is ready (%.0f frames/s)\n" : "GPU %d is ready\n", device, F.dry_engine);
  G.workers_ready++;
  while (G.workers_ready.load() < F.num_gpu && !G.quit_threads) std::this_thread::sleep_for(std::chrono::milliseconds(1));
  std::deque<Frame> inflight;
  std::vector<float> joints((size_t)RTP_MAX_PEOPLE * num_parts * 3);
  auto collect_one = [&]() {
    uint64_t tag;
    int n = 0;
    Frame fr = std::move(inflight.front());
    inflight.pop_front();
    if (want_render && !gpu_jpeg) fr.rendered.resize(gpu_yuv ? rtp_yuv_bytes(DISP_W, DISP_H, 420) : (size_t)DISP_W * DISP_H * 3);
    size_t jpeg_bytes = 0;
    if (heat_bytes) {   // the maps of the oldest frame, which the collect below then takes off the engine's FIFO (--dry_engine: zeros)
      fr.heatmaps.assign(heat_bytes, 0);
      if (!dry && rtp_peek_maps(e, &tag, fr.heatmaps.data(), fr.heatmaps.size()) != RTP_OK) {
        fprintf(stderr, "GPU %d frame %d: --write_heatmaps: %s\n", device, fr.index, rtp_last_error(e));
        fr.heatmaps.assign(heat_bytes, 0);
      }
    }
    if (crop_w) {   // likewise the boxes and crops of the oldest frame (--dry_engine: no boxes)
      fr.crop_n = 0;
      if (!dry) {
        fr.crop_boxes.assign((size_t)F.max_crops * RTP_CROP_BOX_FLOATS, 0.f);
        fr.crops.assign((size_t)F.max_crops * crop_w * crop_h * 3, 0);
        int has_pixels = 0;
        if (rtp_peek_crops(e, &tag, fr.crop_boxes.data(), &fr.crop_n, fr.crops.data(), F.max_crops, &has_pixels) != RTP_OK) {
          fprintf(stderr, "GPU %d frame %d: --write_crops: %s\n", device, fr.index, rtp_last_error(e));
          fr.crop_n = 0;
        }
        fr.crop_boxes.resize((size_t)fr.crop_n * RTP_CROP_BOX_FLOATS);
        fr.crops.resize(has_pixels ? (size_t)fr.crop_n * crop_w * crop_h * 3 : 0);
      }
    }
    int track_n = 0;
    if (gpu_track) {   // likewise the track records of the oldest frame
      fr.track_recs.assign((size_t)RTP_MAX_PEOPLE * RTP_TRACK_REC_INTS, 0);
      if (rtp_peek_tracks(e, &tag, fr.track_recs.data(), &track_n, RTP_MAX_PEOPLE) != RTP_OK) {
        fprintf(stderr, "GPU %d frame %d: --track: %s\n", device, fr.index, rtp_last_error(e));
        track_n = 0;
      }
    }
    int smooth_n = -1;
    if (gpu_smooth) {   // and its smoothed joints
      fr.joints_s.assign((size_t)RTP_MAX_PEOPLE * num_parts * 3, 0.f);
      if (rtp_peek_smoothed(e, &tag, fr.joints_s.data(), nullptr, nullptr, &smooth_n, RTP_MAX_PEOPLE) != RTP_OK) {
        fprintf(stderr, "GPU %d frame %d: --smooth: %s\n", device, fr.index, rtp_last_error(e));
        smooth_n = -1;
      }
    }
    const int rc = dry ? dry_collect(fr, joints.data(), &n)
                   : !want_render ? rtp_collect(e, &tag, joints.data(), &n)
                   : gpu_yuv ? rtp_collect_rendered_yuv(e, &tag, joints.data(), &n, fr.rendered.data(), fr.rendered.size())
                   : gpu_jpeg ? rtp_collect_rendered_jpeg(e, &tag, joints.data(), &n, jpeg_buf.data(), jpeg_buf.size(), &jpeg_bytes)
                              : rtp_collect_rendered(e, &tag, joints.data(), &n, fr.rendered.data());
    if (rc != RTP_OK) { fprintf(stderr, "GPU %d frame %d: %s\n", device, fr.index, rtp_last_error(e)); n = 0; }
    if (rc == RTP_EIO && fr.jpeg) {   // the scan of this file was corrupt: skipped, like a file the producer cannot decode
      std::lock_guard<std::mutex> l(G.mutex);
      G.dropped_index.push(fr.index);
      G.dropped++;
      return;
    }
    if (gpu_jpeg) {  // only the file's bytes are kept
      if (rc == RTP_OK) {
        fr.rendered.assign(jpeg_buf.begin(), jpeg_buf.begin() + (long)jpeg_bytes);
      } else {
        if (black_jpeg.empty()) {
          const std::vector<unsigned char> black((size_t)DISP_W * DISP_H * 3, 0);
          black_jpeg.resize(jpeg_buf.size());
          const long nb = rtp_encode_jpeg(black.data(), DISP_W, DISP_H, 98, black_jpeg.data(), black_jpeg.size());
          black_jpeg.resize(nb > 0 ? (size_t)nb : 0);
        }
        fr.rendered = black_jpeg;
      }
      fr.rendered_jpeg = !fr.rendered.empty();
    }
    if (gpu_yuv) {
      // a frame whose collect failed: the host path converts the zero-filled frame it is handed, so this path writes those planes
      if (rc != RTP_OK) { memset(fr.rendered.data(), 16, (size_t)DISP_W * DISP_H); memset(fr.rendered.data() + (size_t)DISP_W * DISP_H, 128, fr.rendered.size() - (size_t)DISP_W * DISP_H); }
      fr.rendered_yuv = true;
    }
    fr.numPeople = n;
    if (gpu_track) {   // (a frame whose collect failed has no people; one whose peek failed has untracked people)
      for (int k = track_n; k < n; ++k) { int* r = &fr.track_recs[(size_t)k * RTP_TRACK_REC_INTS]; r[0] = 0; r[1] = -1; r[2] = 0; r[3] = 0; }
      fr.track_recs.resize((size_t)n * RTP_TRACK_REC_INTS);
    }
    fr.joints.assign(joints.begin(), joints.begin() + (size_t)n * num_parts * 3);
    if (gpu_smooth) {   // (a frame whose peek failed keeps its raw joints)
      if (smooth_n == n) fr.joints_s.resize((size_t)n * num_parts * 3);
      else fr.joints_s = fr.joints;
    }
    fr.gpu_computed_time = wall();
    fr.data.clear();
    fr.data.shrink_to_fit();
    G.output_queue.push(std::move(fr));
  };
  while (!G.quit_threads) {
    Frame fr;
    bool got = (int)inflight.size() < F.frames_in_flight && G.input_queue.try_pop(&fr);
    if (got) {
      fr.gpu_fetched_time = wall();
      if (fr.gpu_fetched_time - fr.commit_time > 0.1 && !F.no_frame_drops) {  // rtpose.cpp:1112-1124
        std::lock_guard<std::mutex> l(G.mutex);
        G.dropped_index.push(fr.index);
        G.dropped++;
        continue;
      }
      if (dry && !F.host_preprocess) fr.scale = (float)rtp_display_fit_scale(fr.img_w, fr.img_h, DISP_W, DISP_H);
      rtp_yuv_view yv;
      if (fr.yuv) {   // the producer's copy of the file's planes
        const size_t cw = (size_t)(fr.img_w + fr.chroma_sx) >> fr.chroma_sx, ch = (size_t)(fr.img_h + fr.chroma_sy) >> fr.chroma_sy;
        memset(&yv, 0, sizeof yv);
        yv.struct_size = sizeof yv;
        yv.matrix = RTP_YUV_BT601_LIMITED;
        yv.width = fr.img_w; yv.height = fr.img_h;
        yv.y = fr.image.data();
        yv.y_stride = fr.img_w;
        yv.uv_pixel_stride = 1;
        if (!fr.mono) {
          yv.u = fr.image.data() + (size_t)fr.img_w * fr.img_h;
          yv.v = fr.image.data() + (size_t)fr.img_w * fr.img_h + cw * ch;
          yv.uv_stride = (long)cw;
          yv.chroma_shift_x = fr.chroma_sx; yv.chroma_shift_y = fr.chroma_sy;
        }
      }
      const int src = dry ? dry_submit(fr)
                          : F.host_preprocess ? rtp_submit(e, fr.data.data(), (uint64_t)fr.index)
                          : fr.yuv            ? rtp_submit_frame_yuv(e, &yv, (uint64_t)fr.index, &fr.scale)
                          : fr.jpeg           ? rtp_submit_frame_jpeg(e, fr.image.data(), fr.image.size(), (uint64_t)fr.index, &fr.scale, nullptr, nullptr)
                                              : rtp_submit_frame(e, fr.image.data(), fr.img_w, fr.img_h, (uint64_t)fr.index, &fr.scale);
      // --track_appearance in the re-orderer: the BGR frame travels on (a move; the producer hands BGR frames only in that case) and
      // is warped to the display image there, off this thread
      if (appearance_on_host() && !F.host_preprocess && !fr.jpeg && !fr.yuv && fr.image.size() == (size_t)fr.img_w * fr.img_h * 3) {
        fr.display = std::move(fr.image);
        fr.display_raw = true;
      }
      fr.image.clear();
      fr.image.shrink_to_fit();
      if (src != RTP_OK && fr.jpeg && (src == RTP_EIO || src == RTP_EINVAL)) {   // a file the decoder refuses: skipped like one the producer cannot decode
        fprintf(stderr, "cannot decode frame %d: %s\n", fr.video_frame_number, rtp_last_error(e));
        std::lock_guard<std::mutex> l(G.mutex);
        G.dropped_index.push(fr.index);
        G.dropped++;
        continue;
      }
      if (src != RTP_OK) {  // nobody else may be left to drain the queue: stop the producer too
        fprintf(stderr, "GPU %d: %s\n", device, rtp_last_error(e));
        *status = 1;
        G.quit_threads = true;
        break;
      }
      G.per_worker[widx]++;
      inflight.push_back(std::move(fr));
      if (F.test_worker_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(F.test_worker_delay_ms));
      if ((int)inflight.size() < F.frames_in_flight) continue;
    }
    if (!inflight.empty()) collect_one();
    else if (G.producer_done && G.input_queue.size() == 0) break;
    else std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  while (!inflight.empty()) collect_one();
  if (e && F.share_weights && widx == 0 && !dry)   // a receiver may still be inside rtp_get_split_layers / rtp_copy_weights_from on this engine (error paths set quit_threads early)
    while (G.share_done.load() < F.num_gpu - 1) std::this_thread::sleep_for(std::chrono::milliseconds(1));
  if (e) rtp_engine_destroy(e);
}

// ---- --track ---------------------------------------------------------------------------------------------
// One real GPU worker tracks on the GPU (the engine sees its frames in submit order); every other arrangement tracks in the re-orderer
bool track_on_gpu() { return F.track && F.dry_engine <= 0 && !F.host_preprocess && F.num_gpu == 1 && rtp_set_tracking && rtp_peek_tracks; }
rtp_track_config track_config() {
  rtp_track_config tc;
  rtp_track_config_default(&tc);
  tc.max_cost = (float)F.track_max_cost;
  tc.max_misses = F.track_max_misses;
  tc.min_parts = F.track_min_parts;
  return tc;
}

// --track_appearance: on the GPU where the tracker is; otherwise in the re-orderer, with its tracker
bool appearance_on_host() { return F.track && F.track_appearance && !track_on_gpu(); }
// parts: the storage of the list the configuration points to.  Names that are none of the flag's become -1 (refused by main()).
rtp_appearance_config appearance_config(int num_parts, std::vector<int>* parts) {
  rtp_appearance_config ac;
  rtp_appearance_config_default(&ac);
  ac.weight = (float)F.appearance_weight;
  ac.max_dist = (float)F.appearance_max_dist;
  ac.rate = F.appearance_rate;
  parts->clear();
  if (F.appearance_parts == "all") {
    for (int p = 0; p < num_parts; ++p) parts->push_back(p);
  } else if (F.appearance_parts != "torso") {
    for (const char* q = F.appearance_parts.c_str(); *q;) {
      char* end = nullptr;
      parts->push_back((int)strtol(q, &end, 10));
      if (end == q) { parts->back() = -1; break; }
      q = *end == ',' ? end + 1 : end;
    }
    if (parts->empty()) parts->push_back(-1);
  }
  if (!parts->empty()) { ac.parts = parts->data(); ac.num_parts = (int)parts->size(); }
  return ac;
}

// --smooth: on the GPU where the tracker is; otherwise in the re-orderer, behind its rtp_track_update
bool smooth_on_gpu() { return F.smooth && track_on_gpu() && rtp_set_smoothing && rtp_peek_smoothed; }
rtp_smooth_config smooth_config() {
  rtp_smooth_config sc;
  rtp_smooth_config_default(&sc);
  sc.min_cutoff = (float)F.smooth_min_cutoff;
  sc.beta = (float)F.smooth_beta;
  sc.d_cutoff = (float)F.smooth_d_cutoff;
  sc.max_hold = F.smooth_max_hold;
  sc.apply = RTP_SMOOTH_RENDER | RTP_SMOOTH_CROPS;
  return sc;
}

// --draw_tracks: on the GPU where the tracker is, unless --host_draw; otherwise in the re-orderer, behind its rtp_track_update
// (and not while --redact runs in the re-orderer: the drawing goes on top of the redaction, so it has to follow it there)
bool overlay_on_gpu() { return F.draw_tracks && !F.host_draw && track_on_gpu() && rtp_set_track_overlay && !(F.redact && !redact_on_gpu()); }
rtp_overlay_config overlay_config() {
  rtp_overlay_config oc;
  rtp_overlay_config_default(&oc);
  oc.what = 0;
  for (size_t a = 0; a <= F.draw_what.size();) {
    const size_t b = std::min(F.draw_what.find(',', a), F.draw_what.size());
    const std::string w = F.draw_what.substr(a, b - a);
    oc.what |= w == "box" ? RTP_OVERLAY_BOX : w == "label" ? RTP_OVERLAY_LABEL : w == "trail" ? RTP_OVERLAY_TRAIL : 8u;   // (8: refused by main())
    a = b + 1;
  }
  oc.trail_len = F.trail_len;
  oc.label_scale = F.label_scale;
  oc.alpha = F.draw_alpha;
  return oc;
}

// --redact: on the GPU with one real GPU worker, unless --host_redact; otherwise in the re-orderer, in front of its rtp_overlay_draw
bool redact_on_gpu() { return F.redact && !F.host_redact && F.dry_engine <= 0 && !F.host_preprocess && F.num_gpu == 1 && rtp_set_redaction; }
// the re-orderer changes pixels: the workers hand it raw frames
bool host_pixels() { return (F.draw_tracks && !overlay_on_gpu()) || (F.redact && !redact_on_gpu()); }
// parts: the storage of the list the configuration points to.  Names that are none of the flag's become -1 (refused by main()).
rtp_redact_config redact_config(int num_parts, std::vector<int>* parts) {
  rtp_redact_config rc;
  rtp_redact_config_default(&rc);
  rc.effect = F.redact_effect == "mosaic" ? RTP_REDACT_MOSAIC : F.redact_effect == "blur" ? RTP_REDACT_BLUR : F.redact_effect == "fill" ? RTP_REDACT_FILL : -1;
  rc.shape = F.redact_shape == "ellipse" ? RTP_REDACT_ELLIPSE : F.redact_shape == "rect" ? RTP_REDACT_RECT : -1;
  parts->clear();
  if (F.redact_parts == "all") {
    for (int p = 0; p < num_parts; ++p) parts->push_back(p);
  } else if (F.redact_parts != "head") {
    for (const char* q = F.redact_parts.c_str(); *q;) {
      char* end = nullptr;
      parts->push_back((int)strtol(q, &end, 10));
      if (end == q) { parts->back() = -1; break; }
      q = *end == ',' ? end + 1 : end;
    }
    if (parts->empty()) parts->push_back(-1);
  }
  if (!parts->empty()) { rc.parts = parts->data(); rc.num_parts = (int)parts->size(); }
  rc.scale_q8 = (int)lrintf((float)F.redact_scale * 256);
  rc.aspect_q8 = (int)lrintf((float)F.redact_aspect * 256);
  rc.pad = F.redact_pad;
  rc.cell = F.redact_cell;
  rc.radius = F.redact_radius;
  return rc;
}

// ---- re-orderer (buffer_and_order, rtpose.cpp:1214-1273) ---------------------------------------------
struct FrameCompare { bool operator()(const Frame& a, const Frame& b) const { return a.index > b.index; } };
void reorderer(std::atomic<bool>* workers_done) {
  std::priority_queue<Frame, std::vector<Frame>, FrameCompare> buffer;
  int frame_waited = 1;
  auto skip_dropped = [&]() {
    std::lock_guard<std::mutex> l(G.mutex);
    while (!G.dropped_index.empty() && G.dropped_index.top() == frame_waited) { frame_waited++; G.dropped_index.pop(); }
  };
  // --track on the host: this thread sees the frames in order, and rtp_track_update is the definition the GPU kernel equals
  const bool host_track = F.track && !track_on_gpu();
  const rtp_track_config tc = track_config();
  std::unique_ptr<rtp_track_state> tstate;
  // --track_appearance on the host: the descriptors of the frame's display image, then rtp_track_update_appearance in rtp_track_update's place
  const bool host_appear = appearance_on_host();
  std::vector<int> appear_parts;
  std::unique_ptr<rtp_appearance_state> astate;
  std::vector<uint16_t> appear_bins(host_appear ? (size_t)RTP_MAX_PEOPLE * RTP_APPEARANCE_BINS : 0);
  std::vector<unsigned char> appear_valid(host_appear ? (size_t)RTP_MAX_PEOPLE : 0), appear_disp;
  // --smooth on the host: behind the tracker, on the records the frame carries by then (the re-orderer's or the GPU's)
  const bool host_smooth = F.smooth && F.track && !smooth_on_gpu();
  const rtp_smooth_config sc = smooth_config();
  std::unique_ptr<rtp_smooth_state> sstate;
  // --draw_tracks on the host: on the raw rendered frame, from the records the frame carries by then and the joints the frame was rendered
  // from: the raw ones, or, where the engine smooths (--smooth with one GPU worker: RTP_SMOOTH_RENDER), the smoothed ones it handed out
  const bool host_draw = F.draw_tracks && !overlay_on_gpu();
  const rtp_overlay_config oc = overlay_config();
  std::unique_ptr<rtp_trail_state> ostate;
  // --redact on the host: on the raw rendered frame, from the joints the frame was rendered from, in front of the drawing above
  const bool host_redact = F.redact && !redact_on_gpu();
  std::vector<int> redact_parts, redact_regions(host_redact ? (size_t)RTP_MAX_PEOPLE * RTP_REDACT_REGION_INTS : 0);
  std::vector<int> draw_items(host_draw ? (size_t)RTP_OVERLAY_MAX_ITEMS * RTP_OVERLAY_ITEM_INTS : 0);
  auto emit = [&](Frame f) {
    if (host_track) {
      if (!tstate) { tstate.reset(new rtp_track_state); rtp_track_state_init(tstate.get(), G.num_parts.load()); }
      f.track_recs.assign((size_t)std::max(f.numPeople, 1) * RTP_TRACK_REC_INTS, 0);
      int tracked;
      if (host_appear) {
        const int P = G.num_parts.load();
        if (!astate) { astate.reset(new rtp_appearance_state); rtp_appearance_state_init(astate.get()); }
        const rtp_appearance_config ac = appearance_config(P, &appear_parts);
        if (f.display_raw) {   // the frame warped as the engine warps it
          double s = 1;
          appear_disp.resize((size_t)DISP_W * DISP_H * 3);
          if (f.display.size() == (size_t)f.img_w * f.img_h * 3 && rtp_warp_display(f.display.data(), f.img_w, f.img_h, appear_disp.data(), DISP_W, DISP_H, &s) == RTP_OK) f.display.swap(appear_disp);
          else f.display.clear();
        }
        // (the workers have refused a part list that does not fit the model: the call fails for no frame)
        const bool described = f.display.size() == (size_t)DISP_W * DISP_H * 3 &&
                               rtp_appearance_describe(f.display.data(), DISP_W, DISP_H, f.joints.data(), f.numPeople, P, &ac, appear_bins.data(), appear_valid.data()) >= 0;
        tracked = rtp_track_update_appearance(tstate.get(), astate.get(), &tc, &ac, f.joints.data(), f.numPeople, described ? appear_bins.data() : nullptr,
                                              described ? appear_valid.data() : nullptr, f.track_recs.data());
        f.display.clear();
        f.display.shrink_to_fit();
      } else tracked = rtp_track_update(tstate.get(), &tc, f.joints.data(), f.numPeople, f.track_recs.data());
      if (tracked < 0)
        for (int k = 0; k < f.numPeople; ++k) f.track_recs[(size_t)k * RTP_TRACK_REC_INTS + 1] = -1;
      f.track_recs.resize((size_t)f.numPeople * RTP_TRACK_REC_INTS);
    }
    if (host_smooth && f.track_recs.size() == (size_t)f.numPeople * RTP_TRACK_REC_INTS) {
      if (!sstate) { sstate.reset(new rtp_smooth_state); rtp_smooth_state_init(sstate.get(), G.num_parts.load()); }
      f.joints_s.assign(std::max(f.joints.size(), (size_t)1), 0.f);
      if (rtp_smooth_update(sstate.get(), &sc, f.joints.data(), f.numPeople, f.track_recs.data(), f.joints_s.data(), nullptr, nullptr) < 0) f.joints_s = f.joints;
      f.joints_s.resize(f.joints.size());
    }
    if (host_redact && !f.rendered_jpeg && !f.rendered_yuv && f.rendered.size() == (size_t)DISP_W * DISP_H * 3) {
      const rtp_redact_config rc = redact_config(G.num_parts.load(), &redact_parts);
      const float* poses = smooth_on_gpu() && f.joints_s.size() == f.joints.size() ? f.joints_s.data() : f.joints.data();
      const int n = rtp_redact_regions(poses, f.numPeople, G.num_parts.load(), &rc, redact_regions.data());
      if (n >= 0) rtp_redact_apply(redact_regions.data(), n, &rc, f.rendered.data(), DISP_W, DISP_H, 3L * DISP_W);
    }
    if (host_draw && f.track_recs.size() == (size_t)f.numPeople * RTP_TRACK_REC_INTS) {
      if (!ostate) { ostate.reset(new rtp_trail_state); rtp_trail_state_init(ostate.get(), G.num_parts.load()); }
      int m = 0;
      const bool raw = !f.rendered_jpeg && !f.rendered_yuv && f.rendered.size() == (size_t)DISP_W * DISP_H * 3;
      const float* poses = smooth_on_gpu() && f.joints_s.size() == f.joints.size() ? f.joints_s.data() : f.joints.data();
      if (rtp_overlay_update(ostate.get(), &oc, poses, f.numPeople, f.track_recs.data(), draw_items.data(), &m, RTP_OVERLAY_MAX_ITEMS) == RTP_OK && raw)
        rtp_overlay_draw(draw_items.data(), m, f.rendered.data(), DISP_W, DISP_H, 3L * DISP_W);
    }
    f.buffer_end_time = wall();
    G.output_queue_ordered.push(std::move(f));
  };
  while (true) {
    Frame fr;
    if (!G.output_queue.try_pop(&fr)) {
      if (workers_done->load() && G.output_queue.size() == 0) break;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
      continue;
    }
    fr.buffer_start_time = wall();
    skip_dropped();
    if (fr.index == frame_waited) {
      emit(std::move(fr));
      frame_waited++;
      skip_dropped();
      while (!buffer.empty() && buffer.top().index == frame_waited) { emit(buffer.top()); buffer.pop(); frame_waited++; skip_dropped(); }
    } else buffer.push(std::move(fr));
    if ((int)buffer.size() > BUFFER_SIZE) {  // window overflow: force-emit the smallest
      Frame extra = buffer.top();
      buffer.pop();
      frame_waited = extra.index + 1;
      emit(std::move(extra));
      while (!buffer.empty() && buffer.top().index == frame_waited) { emit(buffer.top()); buffer.pop(); frame_waited++; }
    }
  }
  while (!buffer.empty()) { emit(buffer.top()); buffer.pop(); }
}

// ---- JPEG encoders for --write_frames ------------------------------------------------------------------
void encoder() {
  std::vector<unsigned char> jpg((size_t)DISP_W * DISP_H * 4 + 4096);
  while (true) {
    EncodeJob job;
    if (!G.encode_queue.try_pop(&job)) {
      if (G.encode_done.load() && G.encode_queue.size() == 0) break;
      std::this_thread::sleep_for(std::chrono::microseconds(500));
      continue;
    }
    if (job.jpeg) {  // encoded on the GPU: this thread only writes the file
      std::ofstream fs(job.path, std::ios::binary);
      fs.write((const char*)job.bgr.data(), (std::streamsize)job.bgr.size());
      continue;
    }
    const long n = rtp_encode_jpeg(job.bgr.data(), DISP_W, DISP_H, 98, jpg.data(), jpg.size());
    if (n > 0) {
      std::ofstream fs(job.path, std::ios::binary);
      fs.write((const char*)jpg.data(), n);
    } else fprintf(stderr, "JPEG encode failed for %s\n", job.path.c_str());
  }
}

// the JSON block of displayFrame (rtpose.cpp:1383-1416)
void write_json_file(const Frame& fr, std::vector<char>& buf) {
  char fname[1024];
  if (F.image_dir.empty()) snprintf(fname, sizeof fname, "%s/frame%06d.json", F.write_json.c_str(), fr.video_frame_number);  // :1388
  else snprintf(fname, sizeof fname, "%s/%s.json", F.write_json.c_str(), fr.stem.c_str());                                   // :1390-1393
  const bool ids = F.track && fr.track_recs.size() == (size_t)fr.numPeople * RTP_TRACK_REC_INTS;
  const float* joints = F.smooth && fr.joints_s.size() == fr.joints.size() ? fr.joints_s.data() : fr.joints.data();   // --smooth: the smoothed people
  const long n = ids ? rtp_format_json_tracked(buf.data(), buf.size(), joints, fr.numPeople, G.num_parts.load(), fr.scale, fr.track_recs.data())
                     : rtp_format_json(buf.data(), buf.size(), joints, fr.numPeople, G.num_parts.load(), fr.scale);
  if (n >= 0) {
    FILE* f = fopen(fname, "wb");
    if (f) { fwrite(buf.data(), 1, (size_t)n, f); fclose(f); }
    else fprintf(stderr, "cannot create %s\n", fname);
  } else fprintf(stderr, "JSON buffer too small for frame %d\n", fr.index);
}
// --json_writers K: the files are independent (named by frame number / image stem), so K threads format and write them;
// ordering is still the re-orderer's (what the display thread shows / logs)
void json_writer() {
  std::vector<char> buf(1 << 20);
  while (true) {
    Frame fr;
    if (!G.json_queue.try_pop(&fr)) {
      if (G.json_done.load() && G.json_queue.size() == 0) break;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
      continue;
    }
    write_json_file(fr, buf);
    const double now = wall();
    double prev = G.last_written.load();
    while (prev < now && !G.last_written.compare_exchange_weak(prev, now)) {}
  }
}

// ---- writer (displayFrame, rtpose.cpp:1315-1454) -------------------------------------------------------
void writer(std::atomic<bool>* reorder_done) {
  int counter = 1;
  double last_time = wall();
  std::vector<char> buf(1 << 20);
  std::vector<unsigned char> video_buf;   // --write_video --host_video: the frame's planes / its JPEG file
  while (true) {
    Frame fr;
    if (!G.output_queue_ordered.try_pop(&fr)) {
      if (reorder_done->load() && G.output_queue_ordered.size() == 0) break;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
      continue;
    }
    double t_commit = fr.commit_time, t_pre = fr.preprocessed_time, t_fetch = fr.gpu_fetched_time, t_done = fr.gpu_computed_time, t_b0 = fr.buffer_start_time, t_b1 = fr.buffer_end_time;
    const int f_index = fr.index, f_np = fr.numPeople;
    if (G.video_out && !fr.rendered.empty() && !G.video_failed.load()) {   // --write_video: this thread sees the frames in order
      int vrc;
      if (G.video_kind == RTP_VIDEO_Y4M) {
        const size_t ysz = (size_t)DISP_W * DISP_H, csz = (size_t)((DISP_W + 1) / 2) * ((DISP_H + 1) / 2);
        rtp_yuv_view yv;
        memset(&yv, 0, sizeof yv);
        yv.struct_size = sizeof yv;
        yv.matrix = RTP_YUV_BT601_LIMITED;
        yv.width = DISP_W; yv.height = DISP_H;
        yv.chroma_shift_x = yv.chroma_shift_y = 1;
        yv.y_stride = DISP_W; yv.uv_stride = (DISP_W + 1) / 2; yv.uv_pixel_stride = 1;
        unsigned char* planes = fr.rendered.data();
        if (!fr.rendered_yuv) { video_buf.resize(ysz + 2 * csz); planes = video_buf.data(); }
        yv.y = planes; yv.u = planes + ysz; yv.v = planes + ysz + csz;
        vrc = fr.rendered_yuv ? RTP_OK : rtp_convert_bgr_to_yuv(fr.rendered.data(), DISP_W, DISP_H, 3L * DISP_W, &yv);   // --host_video
        if (vrc == RTP_OK) vrc = rtp_video_write_yuv(G.video_out, &yv);
      } else {
        if (!fr.rendered_jpeg) {   // --host_video: encoded here, once; --write_frames then writes the same file
          video_buf.resize(rtp_jpeg_max_bytes(DISP_W, DISP_H));
          const long nb = rtp_encode_jpeg(fr.rendered.data(), DISP_W, DISP_H, 98, video_buf.data(), video_buf.size());
          if (nb > 0) { fr.rendered.assign(video_buf.begin(), video_buf.begin() + nb); fr.rendered_jpeg = true; }
        }
        vrc = fr.rendered_jpeg ? rtp_video_write_jpeg(G.video_out, fr.rendered.data(), fr.rendered.size()) : RTP_EINVAL;
      }
      if (vrc != RTP_OK) { fprintf(stderr, "--write_video: frame %d: %s\n", fr.index, rtp_codec_last_error()); G.video_failed = true; }
    }
    if (!F.write_heatmaps.empty() && !fr.heatmaps.empty()) {   // this thread sees the frames in order
      char fname[1024];
      snprintf(fname, sizeof fname, "%s%06d.pgm", F.write_heatmaps.c_str(), fr.video_frame_number);
      FILE* f = fopen(fname, "wb");
      if (f) {
        fprintf(f, "P5\n%d %d\n255\n", NET_W, (int)(fr.heatmaps.size() / (size_t)NET_W));
        fwrite(fr.heatmaps.data(), 1, fr.heatmaps.size(), f);
        fclose(f);
      } else fprintf(stderr, "cannot create %s\n", fname);
      fr.heatmaps.clear();
      fr.heatmaps.shrink_to_fit();
    }
    if (!F.write_crops.empty() && fr.crop_n >= 0) {   // (in frame order too)
      char fname[1024];
      int cw = 0, ch = 0;
      sscanf(F.crop_size.c_str(), "%dx%d", &cw, &ch);
      const size_t cb = (size_t)cw * ch * 3;
      std::vector<unsigned char> rgb(cb);
      snprintf(fname, sizeof fname, "%s%06d_boxes.json", F.write_crops.c_str(), fr.video_frame_number);
      FILE* f = fopen(fname, "wb");
      if (f) {
        fprintf(f, "{\n\"frame\":%d,\n\"crop_w\":%d,\n\"crop_h\":%d,\n\"boxes\":[", fr.video_frame_number, cw, ch);
        for (int k = 0; k < fr.crop_n; ++k) {
          const float* b = &fr.crop_boxes[(size_t)k * RTP_CROP_BOX_FLOATS];
          fprintf(f, "%s\n{\"person\":%d,", k ? "," : "", k);
          if (F.track) fprintf(f, "\"id\":%d,", (size_t)k * RTP_TRACK_REC_INTS < fr.track_recs.size() ? fr.track_recs[(size_t)k * RTP_TRACK_REC_INTS] : 0);
          fprintf(f, "\"left\":%.9g,\"top\":%.9g,\"width\":%.9g,\"height\":%.9g,\"parts\":%d,\"valid\":%d}", (double)b[0], (double)b[1],
                  (double)b[2], (double)b[3], (int)b[4], (int)b[5]);
        }
        fprintf(f, "\n]\n}\n");
        fclose(f);
      } else fprintf(stderr, "cannot create %s\n", fname);
      for (int k = 0; k < fr.crop_n && !fr.crops.empty(); ++k) {
        if (fr.crop_boxes[(size_t)k * RTP_CROP_BOX_FLOATS + 5] == 0.f) continue;   // no box: no file
        const unsigned char* src = &fr.crops[(size_t)k * cb];
        for (size_t q = 0; q < cb; q += 3) { rgb[q] = src[q + 2]; rgb[q + 1] = src[q + 1]; rgb[q + 2] = src[q]; }
        snprintf(fname, sizeof fname, "%s%06d_%02d.ppm", F.write_crops.c_str(), fr.video_frame_number, k);
        FILE* g = fopen(fname, "wb");
        if (g) {
          fprintf(g, "P6\n%d %d\n255\n", cw, ch);
          fwrite(rgb.data(), 1, cb, g);
          fclose(g);
        } else fprintf(stderr, "cannot create %s\n", fname);
      }
      fr.crops.clear();
      fr.crops.shrink_to_fit();
    }
    if (!F.write_frames.empty() && !fr.rendered.empty()) {  // cv::imwrite(fname, wrap_frame, {JPEG_QUALITY, 98}), rtpose.cpp:1367-1381
      char fname[1024];
      if (F.image_dir.empty()) snprintf(fname, sizeof fname, "%s/frame%06d.jpg", F.write_frames.c_str(), fr.video_frame_number);
      else snprintf(fname, sizeof fname, "%s/%s.jpg", F.write_frames.c_str(), fr.stem.c_str());
      while (G.encode_queue.size() > 32) std::this_thread::sleep_for(std::chrono::milliseconds(1));  // back-pressure on the encoders
      G.encode_queue.push(EncodeJob{fname, std::move(fr.rendered), fr.rendered_jpeg});
    }
    if (!F.write_json.empty()) {
      if (F.json_writers > 0) {
        while (G.json_queue.size() > 256) std::this_thread::sleep_for(std::chrono::microseconds(200));  // back-pressure on the JSON writers
        G.json_queue.push(std::move(fr));
      } else write_json_file(fr, buf);
    }
    G.finished++;
    {
      const double now = wall();
      double prev = G.last_written.load();
      while (prev < now && !G.last_written.compare_exchange_weak(prev, now)) {}
    }
    counter++;
    if (counter % 30 == 0) {  // rtpose.cpp:1421-1441
      const double now = wall();
      const double fps = 30.0 / (now - last_time);
      last_time = now;
      fprintf(stderr, "# %d, NP %d, Latency %.3f, Preprocess %.3f, QueueA %.3f, GPU %.3f, QueueB %.3f, Buffered %.3f, QueueD %.3f, FPS = %.1f\n",
              f_index, f_np, now - t_commit, t_pre - t_commit, t_fetch - t_pre, t_done - t_fetch, t_b0 - t_done, t_b1 - t_b0, now - t_b1, fps);
    }
  }
}

int read_image_dir() {  // readImageDirIfFlagEnabled, rtpose.cpp:1732-1755
  if (F.image_dir.empty()) return 0;
  DIR* d = opendir(F.image_dir.c_str());
  if (!d) { fprintf(stderr, "Folder %s does not exist.\n", F.image_dir.c_str()); return -1; }
  while (dirent* ent = readdir(d)) {
    const std::string n = ent->d_name;
    const size_t dot = n.find_last_of('.');
    if (dot == std::string::npos) continue;
    const std::string ext = n.substr(dot);
    std::string ext_l = ext;
    for (char& ch : ext_l) ch = (char)tolower((unsigned char)ch);
    if (ext_l == ".jpg" || ext_l == ".jpeg" || ext_l == ".png" || ext_l == ".bmp" || ext_l == ".ppm") G.image_list.push_back(F.image_dir + "/" + n);
  }
  closedir(d);
  std::sort(G.image_list.begin(), G.image_list.end());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int pf = parse_flags(argc, argv, F);
  if (pf == 2) { usage(); return 0; }
  if (pf) return 1;
  if (sscanf(F.resolution.c_str(), "%dx%d", &DISP_W, &DISP_H) != 2) { fprintf(stderr, "Error, resolution format (%s) invalid, should be e.g., 960x540\n", F.resolution.c_str()); return 1; }
  if (sscanf(F.net_resolution.c_str(), "%dx%d", &NET_W, &NET_H) != 2) { fprintf(stderr, "Error, net resolution format (%s) invalid, should be e.g., 656x368 (multiples of 16)\n", F.net_resolution.c_str()); return 1; }
  if (read_image_dir() != 0) return 1;
  if (DISP_W == -1) {  // rtpose.cpp:1676-1693
    int w = 0, h = 0;
    if (!F.image_dir.empty() && !G.image_list.empty() && rtp_load_image(G.image_list[0].c_str(), nullptr, 0, &w, &h) == RTP_OK) { DISP_W = w; DISP_H = h; }
    else if (F.video.rfind("synthetic:", 0) == 0 && sscanf(F.video.c_str(), "synthetic:%dx%d", &w, &h) == 2) { DISP_W = w; DISP_H = h; }
    else if (!F.video.empty() && F.video.rfind("synthetic:", 0) != 0) {
      rtp_video* v = nullptr;
      if (rtp_video_open(F.video.c_str(), &v, &w, &h, nullptr) != RTP_OK) { fprintf(stderr, "Couldn't open video file %s: %s\n", F.video.c_str(), rtp_codec_last_error()); return 1; }
      rtp_video_close(v);
      DISP_W = w; DISP_H = h;
    }
    else { fprintf(stderr, "Invalid resolution without video/images: %dx%d\n", DISP_W, DISP_H); return 1; }
  }
  if (F.video.empty() && F.image_dir.empty()) { fprintf(stderr, "Couldn't open camera %d (no capture stack in this build): use --video or --image_dir\n", F.camera); return 1; }
  if (!F.video.empty() && F.video.rfind("synthetic:", 0) != 0) {
    rtp_video* v = nullptr;
    if (rtp_video_open(F.video.c_str(), &v, nullptr, nullptr, nullptr) != RTP_OK) { fprintf(stderr, "Couldn't open video file %s: %s\n", F.video.c_str(), rtp_codec_last_error()); return 1; }
    rtp_video_close(v);
  }
  for (const std::string* d : {&F.write_frames, &F.write_json})
    if (!d->empty() && !mkdir_p(*d)) { fprintf(stderr, "Could not write to or create directory %s\n", d->c_str()); return 1; }
  if (F.heatmap_channels != "parts" && F.heatmap_channels != "bkg" && F.heatmap_channels != "parts+bkg" && F.heatmap_channels != "pafs" && F.heatmap_channels != "all") {
    fprintf(stderr, "--heatmap_channels must be parts, bkg, parts+bkg, pafs or all\n");
    return 1;
  }
  if (F.track && (!(F.track_max_cost > 0) || !std::isfinite(F.track_max_cost) || F.track_max_misses < 0 || F.track_min_parts < 1)) {
    fprintf(stderr, "--track: --track_max_cost must be a finite number > 0, --track_max_misses >= 0, --track_min_parts >= 1\n");
    return 1;
  }
  if (F.track_appearance) {
    std::vector<int> parts;
    const rtp_appearance_config ac = appearance_config(RTP_MAX_NUM_PARTS, &parts);
    bool bad_part = false;
    for (int p : parts) bad_part = bad_part || p < 0;
    if (!F.track || !(F.appearance_weight >= 0) || !std::isfinite(F.appearance_weight) || !(F.appearance_max_dist > 0 && F.appearance_max_dist <= 1) || ac.rate < 1 || ac.rate > 256 || bad_part) {
      fprintf(stderr, "--track_appearance needs --track; --appearance_weight must be a finite number >= 0, --appearance_max_dist in (0, 1], --appearance_rate 1 .. 256, "
                      "--appearance_parts torso, all or a comma-separated list of part indices\n");
      return 1;
    }
  }
  if (F.smooth && !F.track) {
    fprintf(stderr, "--smooth needs --track (the filter follows tracked people)\n");
    usage();
    return 1;
  }
  if (F.smooth && (!(F.smooth_min_cutoff > 0) || !std::isfinite(F.smooth_min_cutoff) || !(F.smooth_beta >= 0) || !std::isfinite(F.smooth_beta) || !(F.smooth_d_cutoff > 0) ||
                   !std::isfinite(F.smooth_d_cutoff) || F.smooth_max_hold < 0 || F.smooth_max_hold > RTP_SMOOTH_MAX_HOLD)) {
    fprintf(stderr, "--smooth: --smooth_min_cutoff and --smooth_d_cutoff must be finite numbers > 0, --smooth_beta a finite number >= 0, --smooth_max_hold 0 .. %d\n", RTP_SMOOTH_MAX_HOLD);
    return 1;
  }
  if ((F.draw_tracks || F.host_draw) && (!F.track || !F.draw_tracks || (F.write_frames.empty() && F.write_video.empty()))) {
    fprintf(stderr, "--draw_tracks needs --track and --write_frames or --write_video (it draws tracked people into the rendered frames); --host_draw needs --draw_tracks\n");
    usage();
    return 1;
  }
  if ((F.redact || F.host_redact) && (!F.redact || (F.write_frames.empty() && F.write_video.empty()))) {
    fprintf(stderr, "--redact needs --write_frames or --write_video (it anonymises the rendered frames); --host_redact needs --redact\n");
    usage();
    return 1;
  }
  if (F.redact) {
    std::vector<int> parts;
    int none[RTP_REDACT_REGION_INTS];
    const int model_parts = F.model == "mpi" ? 15 : 18;
    const rtp_redact_config rc = redact_config(model_parts, &parts);
    if (!std::isfinite(F.redact_scale) || !std::isfinite(F.redact_aspect) || rtp_redact_regions(nullptr, 0, model_parts, &rc, none) < 0) {
      fprintf(stderr, "--redact: --redact_effect mosaic|blur|fill, --redact_shape ellipse|rect, --redact_parts head|all|p0,p1,.. (each part once), --redact_cell 2|4|8|16|32, "
                      "--redact_radius 1 .. 16, --redact_scale 0.25 .. 16, --redact_aspect 0.25 .. 4, --redact_pad 0 .. 256\n");
      return 1;
    }
  }
  if (F.draw_tracks) {
    const rtp_overlay_config oc = overlay_config();
    if (oc.what == 0 || (oc.what & 8u) || oc.trail_len < 0 || oc.trail_len > RTP_TRAIL_MAX || oc.label_scale < 1 || oc.label_scale > 8 || oc.alpha < 0 || oc.alpha > 256) {
      fprintf(stderr, "--draw_tracks: --draw_what is a comma-separated list of box, label and trail, --trail_len 0 .. %d, --label_scale 1 .. 8, --draw_alpha 0 .. 256\n", RTP_TRAIL_MAX);
      return 1;
    }
  }
  if (!F.write_crops.empty()) {
    int cw = 0, ch = 0;
    char tail = 0;
    if (sscanf(F.crop_size.c_str(), "%dx%d%c", &cw, &ch, &tail) != 2 || cw < RTP_CROP_MIN_SIZE || ch < RTP_CROP_MIN_SIZE || cw > RTP_CROP_MAX_SIZE || ch > RTP_CROP_MAX_SIZE) {
      fprintf(stderr, "--crop_size must be WxH with both in [%d, %d]\n", RTP_CROP_MIN_SIZE, RTP_CROP_MAX_SIZE);
      return 1;
    }
    if (F.max_crops < 1 || F.max_crops > RTP_MAX_PEOPLE) { fprintf(stderr, "--max_crops must be in [1, %d]\n", RTP_MAX_PEOPLE); return 1; }
    if (!(F.crop_margin >= 0 && F.crop_margin <= 16)) { fprintf(stderr, "--crop_margin must be in [0, 16]\n"); return 1; }
  }
  if (F.num_gpu < 1) { fprintf(stderr, "--num_gpu must be >= 1\n"); return 1; }
  if (F.precision != "mixed" && F.precision != "fp16" && F.precision != "f16x3" && F.precision != "fp32") { fprintf(stderr, "--precision must be mixed, fp16, f16x3 or fp32\n"); return 1; }
  if (F.frames_in_flight < 1 || F.frames_in_flight > 64) { fprintf(stderr, "--frames_in_flight must be in [1, 64]\n"); return 1; }
  if (F.batch_frames < 1 || F.batch_frames > 16) { fprintf(stderr, "--batch_frames must be in [1, 16]\n"); return 1; }
  // Hardware queues of the HIP runtime (read once, at the process's first HIP call — nothing has touched HIP yet; a value from the environment
  // wins): with at least as many queues as batch contexts the engine gives every context ONE stream and so one queue to itself: +12 % frames/s
  // at batches of 2 against the default 4 queues (engine.cpp "hardware queues").
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  if (F.json_writers < 0) F.json_writers = F.num_gpu;
  if (F.dry_engine < 0 || F.json_writers > 64) { fprintf(stderr, "--dry_engine must be >= 0 and --json_writers in [0, 64]\n"); return 1; }
  std::vector<int> devs;
  for (int g = 0; g < F.num_gpu; ++g) devs.push_back(g + F.start_device);  // rtpose.cpp:1466
  if (!F.devices.empty()) {
    devs.clear();
    size_t pos = 0;
    while (pos <= F.devices.size()) {
      const size_t c = F.devices.find(',', pos);
      const std::string tok = F.devices.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
      if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) { fprintf(stderr, "bad --devices '%s'\n", F.devices.c_str()); return 1; }
      devs.push_back(atoi(tok.c_str()));
      if (c == std::string::npos) break;
      pos = c + 1;
    }
    if ((int)devs.size() != F.num_gpu) { fprintf(stderr, "--devices names %zu devices but --num_gpu is %d\n", devs.size(), F.num_gpu); return 1; }
  }
  G.per_worker.assign(F.num_gpu, 0);
  if (!F.write_video.empty()) {
    const size_t dot = F.write_video.find_last_of('.');
    std::string ext = dot == std::string::npos ? "" : F.write_video.substr(dot);
    for (char& ch : ext) ch = (char)tolower((unsigned char)ch);
    G.video_kind = ext == ".y4m" ? RTP_VIDEO_Y4M : (ext == ".mjpeg" || ext == ".mjpg") ? RTP_VIDEO_MJPEG : 0;
    if (!G.video_kind) { fprintf(stderr, "--write_video %s: the suffix chooses the format: .y4m, .mjpeg or .mjpg\n", F.write_video.c_str()); return 1; }
    if (F.video_fps < 1) { fprintf(stderr, "--video_fps must be >= 1\n"); return 1; }
    if (F.host_preprocess) { fprintf(stderr, "--write_video needs the device pre-processing path (drop --host_preprocess)\n"); return 1; }
    if (G.video_kind == RTP_VIDEO_Y4M && !F.write_frames.empty()) {
      fprintf(stderr, "--write_video %s cannot be combined with --write_frames: one renderer mode is active at a time (YUV planes or JPEG files); "
                      "write an .mjpeg video next to the frames, or run twice\n", F.write_video.c_str());
      return 1;
    }
    if (G.video_kind == RTP_VIDEO_MJPEG && !F.write_frames.empty() && !(F.dry_engine > 0) && F.host_jpeg != F.host_video && !host_pixels()) {
      fprintf(stderr, "--write_frames with --write_video x.mjpeg: both take the same files, so give --host_jpeg and --host_video together or neither\n");
      return 1;
    }
    if (rtp_video_create(F.write_video.c_str(), DISP_W, DISP_H, G.video_kind, F.video_fps, 1, &G.video_out) != RTP_OK) {
      fprintf(stderr, "--write_video: %s\n", rtp_codec_last_error());
      return 1;
    }
  }
  if (!F.write_frames.empty() && F.host_preprocess) { fprintf(stderr, "--write_frames needs the device pre-processing path (drop --host_preprocess)\n"); return 1; }

  const double t0 = wall();
  std::vector<std::thread> workers;
  std::vector<int> status(F.num_gpu, 0);
  for (int g = 0; g < F.num_gpu; ++g) workers.emplace_back(worker, g, devs[g], &status[g]);
  std::atomic<bool> workers_done{false}, reorder_done{false};
  std::thread prod(producer), reo(reorderer, &workers_done), wr(writer, &reorder_done);
  std::vector<std::thread> encoders;
  if (!F.write_frames.empty()) for (int i = 0; i < 8; ++i) encoders.emplace_back(encoder);
  std::vector<std::thread> jsonw;
  if (!F.write_json.empty()) for (int i = 0; i < F.json_writers; ++i) jsonw.emplace_back(json_writer);
  prod.join();
  for (auto& t : workers) t.join();
  workers_done = true;
  reo.join();
  reorder_done = true;
  wr.join();
  if (G.video_out && rtp_video_finish(G.video_out) != RTP_OK) { fprintf(stderr, "--write_video: %s\n", rtp_codec_last_error()); G.video_failed = true; }
  G.encode_done = true;
  for (auto& t : encoders) t.join();
  G.json_done = true;
  for (auto& t : jsonw) t.join();
  int rc = 0;
  for (int s : status) rc |= s;
  if (G.video_failed.load()) rc |= 1;
  const double dt = wall() - t0;
  for (int g = 0; g < F.num_gpu; ++g) fprintf(stderr, "worker %d (GPU %d) processed %d frames\n", g, devs[g], G.per_worker[g]);
  if (F.share_weights) fprintf(stderr, "share_weights: %d worker(s) took worker 0's packed weights\n", G.weights_shared.load());
  const double steady = (G.finished.load() > 1 && G.last_written.load() > G.first_commit) ? G.finished.load() / (G.last_written.load() - G.first_commit) : 0.0;
  fprintf(stderr, "rtcpm %s. Total time: %.3f seconds. frames produced %d, written %d, dropped %d (%.1f FPS incl. init, %.1f FPS first frame committed -> last frame written)\n",
          rc ? "FAILED" : "successfully finished", dt, G.produced.load(), G.finished.load(), G.dropped.load(), G.finished.load() / dt, steady);
  return rc;
}
