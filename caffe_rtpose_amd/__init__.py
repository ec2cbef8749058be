"""caffe_rtpose_amd — MI355X-native realtime multi-person pose engine (hot path of caffe_rtpose).

The product is `librtpose_mi355x.so` (hand-written HIP for gfx950 behind the C-ABI declared in
include/rtpose_mi355x.h) plus the C++ host `rtpose.bin`.  This Python package is only a thin
ctypes mirror of that ABI for tests and bench.py; it contains NO compute and NO CPU fallback:
importing it fails loudly if the HIP library has not been built.
"""
from ._lib import lib, LIB_PATH  # noqa: F401  (raises ImportError when the .so is missing)
from .engine import (Config, Engine, RtpError, frame_view, yuv_view, convert_yuv, convert_bgr_to_yuv, yuv_bytes, VideoWriter, VIDEO_Y4M, VIDEO_MJPEG, video_chroma, video_read_yuv, maps_quantize_u8, maps_to_f16, maps_view, crop_people, crops_head_parts, track_config, TrackState, track_update, format_json_tracked, MAX_TRACKS, TRACK_REC_INTS, appearance_config, AppearanceState, appearance_describe, appearance_torso_parts, track_update_appearance, APPEARANCE_BINS, smooth_config, SmoothState, smooth_update, SMOOTH_RENDER, SMOOTH_CROPS, overlay_config, TrailState, overlay_update, overlay_draw, OVERLAY_BOX, OVERLAY_LABEL, OVERLAY_TRAIL, OVERLAY_ITEM_INTS, OVERLAY_MAX_ITEMS, OVERLAY_PALETTE, OVERLAY_FONT, TRAIL_MAX, redact_config, redact_regions, redact_apply, REDACT_MOSAIC, REDACT_BLUR, REDACT_FILL, REDACT_ELLIPSE, REDACT_RECT, REDACT_REGION_INTS, REDACT_MAX_RADIUS, CROPS_LAYOUTS, CROP_BOX_FLOATS, model_tables, default_thresholds, process_and_pad_image,
                     format_json, prototxt_summary, plan_summary, device_local_cpus, synth_weights,
                     write_synthetic_caffemodel, read_caffemodel_layers, write_builtin_prototxt, resize_area, warp_display, preprocess_frame, synth_frame, load_image, decode_image, encode_jpeg, jpeg_max_bytes, Video, MODEL_COCO_18, MODEL_MPI_15, PREC_FP16, PREC_FP32, PREC_MIXED, PREC_F16X3, EXEC_GRAPH, EXEC_EAGER,
                     MAX_PEOPLE, RTP_OK, RTP_EINVAL, RTP_ENOMEM, RTP_ENODEV, RTP_EIO, RTP_EAGAIN, RTP_EHIP, RTP_ERANGE)  # noqa: F401
