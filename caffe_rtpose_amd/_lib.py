"""Loads librtpose_mi355x.so.  No fallback of any kind."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTP_LIB") or os.path.join(_HERE, "librtpose_mi355x.so")  # RTP_LIB: kernel experiments with an alternative build

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build the HIP engine first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C caffe_rtpose_amd/csrc). "
        "There is no CPU/PyTorch fallback for this path.")

lib = C.CDLL(LIB_PATH)


class rtp_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("device_id", C.c_int),
        ("model", C.c_int),
        ("proto_path", C.c_char_p),
        ("weights_path", C.c_char_p),
        ("synthetic_seed", C.c_uint64),
        ("net_w", C.c_int),
        ("net_h", C.c_int),
        ("num_scales", C.c_int),
        ("start_scale", C.c_float),
        ("scale_gap", C.c_float),
        ("disp_w", C.c_int),
        ("disp_h", C.c_int),
        ("precision", C.c_int),
        ("frames_in_flight", C.c_int),
        ("batch_frames", C.c_int),
        ("render", C.c_int),
        ("exec_mode", C.c_int),
        ("split_layers", C.c_char_p),
        ("keep_blobs", C.c_int),
        ("calibrate_frames", C.c_int),
        ("calibrate_target", C.c_float),
        ("defer_weights", C.c_int),
    ]


class rtp_frame_view(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("data", C.c_void_p),
        ("width", C.c_int),
        ("height", C.c_int),
        ("row_stride", C.c_long),
        ("pixel_stride", C.c_long),
        ("channel_offset", C.c_long * 3),
    ]


class rtp_yuv_view(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("matrix", C.c_int),
        ("y", C.c_void_p),
        ("u", C.c_void_p),
        ("v", C.c_void_p),
        ("width", C.c_int),
        ("height", C.c_int),
        ("chroma_shift_x", C.c_int),
        ("chroma_shift_y", C.c_int),
        ("y_stride", C.c_long),
        ("uv_stride", C.c_long),
        ("uv_pixel_stride", C.c_long),
    ]


class rtp_maps_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("grid", C.c_int),
        ("format", C.c_int),
        ("channels", C.POINTER(C.c_int)),
        ("num_channels", C.c_int),
    ]


class rtp_maps_view(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("data", C.c_void_p),
        ("channel_stride", C.c_long),
        ("row_stride", C.c_long),
    ]


class rtp_crops_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("crop_w", C.c_int),
        ("crop_h", C.c_int),
        ("max_crops", C.c_int),
        ("parts", C.POINTER(C.c_int)),
        ("num_parts", C.c_int),
        ("min_score", C.c_float),
        ("min_parts", C.c_int),
        ("margin", C.c_float),
        ("layout", C.c_int),
    ]


class rtp_crops_view(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("data", C.c_void_p),
        ("crop_stride", C.c_long),
    ]


class rtp_track_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("min_score", C.c_float),
        ("min_parts", C.c_int),
        ("min_common", C.c_int),
        ("max_cost", C.c_float),
        ("max_misses", C.c_int),
    ]


class rtp_track_state(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("num_parts", C.c_int),
        ("next_id", C.c_uint),
        ("frames", C.c_uint),
        ("id", C.c_int * 128),
        ("hits", C.c_int * 128),
        ("misses", C.c_int * 128),
        ("joints", C.c_float * (128 * 70 * 3)),
    ]


class rtp_appearance_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("parts", C.POINTER(C.c_int)),
        ("num_parts", C.c_int),
        ("min_score", C.c_float),
        ("min_parts", C.c_int),
        ("margin", C.c_float),
        ("weight", C.c_float),
        ("max_dist", C.c_float),
        ("unknown", C.c_float),
        ("rate", C.c_int),
    ]


class rtp_appearance_state(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("reserved", C.c_int * 3),
        ("owner", C.c_int * 128),
        ("desc", C.c_uint16 * (128 * 128)),
    ]


class rtp_smooth_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("min_score", C.c_float),
        ("min_cutoff", C.c_float),
        ("beta", C.c_float),
        ("d_cutoff", C.c_float),
        ("max_hold", C.c_int),
        ("apply", C.c_uint),
    ]


class rtp_smooth_cell(C.Structure):
    _fields_ = [
        ("owner", C.c_int),
        ("last", C.c_uint),
        ("pos", C.c_float * 2),
        ("vel", C.c_float * 2),
        ("score", C.c_float),
    ]


class rtp_smooth_state(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("num_parts", C.c_int),
        ("frames", C.c_uint),
        ("cell", rtp_smooth_cell * 70 * 128),
    ]


class rtp_overlay_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("what", C.c_uint),
        ("min_score", C.c_float),
        ("box_margin", C.c_int),
        ("line_width", C.c_int),
        ("label_scale", C.c_int),
        ("trail_len", C.c_int),
        ("trail_radius", C.c_int),
        ("alpha", C.c_int),
    ]


class rtp_redact_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("effect", C.c_int),
        ("shape", C.c_int),
        ("parts", C.POINTER(C.c_int)),
        ("num_parts", C.c_int),
        ("min_score", C.c_float),
        ("min_parts", C.c_int),
        ("scale_q8", C.c_int),
        ("aspect_q8", C.c_int),
        ("pad", C.c_int),
        ("min_radius", C.c_int),
        ("cell", C.c_int),
        ("radius", C.c_int),
        ("colour", C.c_uint),
    ]


class rtp_trail_slot(C.Structure):
    _fields_ = [
        ("owner", C.c_int),
        ("count", C.c_int),
        ("head", C.c_int),
        ("pts", C.c_int * 2 * 32),
    ]


class rtp_trail_state(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint),
        ("num_parts", C.c_int),
        ("frames", C.c_uint),
        ("slot", rtp_trail_slot * 128),
    ]


fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)
vp = C.c_void_p

# every symbol include/rtpose_mi355x.h declares, with its signature
SIGNATURES = {
    "rtp_config_default": (C.c_int, [C.POINTER(rtp_config)]),
    "rtp_engine_create": (C.c_int, [C.POINTER(rtp_config), C.POINTER(vp)]),
    "rtp_engine_destroy": (None, [vp]),
    "rtp_engine_info": (C.c_int, [vp, ip, ip, ip, ip, ip]),
    "rtp_set_thresholds": (C.c_int, [vp, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float]),
    "rtp_get_thresholds": (C.c_int, [vp, fp, fp, ip, ip, fp]),
    "rtp_set_scales": (C.c_int, [vp, C.c_float, C.c_float]),
    "rtp_debug_f32_to_e4m3": (C.c_int, [fp, C.POINTER(C.c_ubyte), C.c_int]),
    "rtp_kernel_timing_by_passes": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "rtp_kernel_timing_steps": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_long), C.c_int]),
    "rtp_busy_probe": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "rtp_probe_dropped": (C.c_int, [vp, C.POINTER(C.c_long)]),
    "rtp_stamp_probe": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "rtp_debug_stream_queues": (C.c_int, [vp, C.c_int, ip, fp, C.c_int, C.POINTER(C.c_long), C.c_int]),
    "rtp_submit": (C.c_int, [vp, fp, C.c_uint64]),
    "rtp_submit_device": (C.c_int, [vp, vp, C.c_uint64]),
    "rtp_submit_frame": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_uint64, fp]),
    "rtp_debug_preprocess": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int, fp, C.POINTER(C.c_ubyte), fp]),
    "rtp_flush": (C.c_int, [vp]),
    "rtp_collect_rendered": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(C.c_ubyte)]),
    "rtp_render": (C.c_int, [vp, C.POINTER(C.c_ubyte), fp, C.c_int, C.c_int, C.c_int, fp, C.POINTER(C.c_ubyte)]),
    "rtp_decode_image": (C.c_int, [C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_ubyte), C.c_size_t, ip, ip]),
    "rtp_codec_last_error": (C.c_char_p, []),
    "rtp_encode_jpeg": (C.c_long, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_size_t]),
    "rtp_video_open": (C.c_int, [C.c_char_p, C.POINTER(vp), ip, ip, ip]),
    "rtp_video_read": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_size_t]),
    "rtp_video_close": (None, [vp]),
    "rtp_post_from_lowres": (C.c_int, [vp, fp, fp, fp, ip]),
    "rtp_profile_steps": (C.c_int, [vp, C.c_int, fp, C.POINTER(C.c_double), C.c_int]),
    "rtp_collect": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip]),
    "rtp_in_flight": (C.c_int, [vp]),
    "rtp_forward_heatmaps": (C.c_int, [vp, fp, fp]),
    "rtp_resize": (C.c_int, [vp, fp, fp]),
    "rtp_nms": (C.c_int, [vp, fp, fp]),
    "rtp_connect": (C.c_int, [vp, fp, fp, fp, ip]),
    "rtp_forward_debug": (C.c_int, [vp, fp, fp, fp, fp, fp, ip]),
    "rtp_get_blob": (C.c_int, [vp, C.c_char_p, fp, C.c_size_t, ip]),
    "rtp_get_batch_blob": (C.c_int, [vp, C.c_int, C.c_char_p, fp, C.c_size_t, ip, C.POINTER(C.c_uint64), ip]),
    "rtp_num_conv_layers": (C.c_int, [vp]),
    "rtp_conv_layer_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, ip, ip, ip]),
    "rtp_get_conv_weights": (C.c_int, [vp, C.c_int, fp, fp]),
    "rtp_set_conv_weights": (C.c_int, [vp, C.c_int, fp, fp]),
    "rtp_save_caffemodel": (C.c_int, [vp, C.c_char_p]),
    "rtp_save_prototxt": (C.c_int, [vp, C.c_char_p]),
    "rtp_model_tables": (C.c_int, [C.c_int, ip, ip, ip, ip]),
    "rtp_default_thresholds": (C.c_int, [C.c_int, fp, fp, ip, ip, fp]),
    "rtp_process_and_pad_image": (C.c_int, [fp, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rtp_format_json": (C.c_long, [C.c_char_p, C.c_size_t, fp, C.c_int, C.c_int, C.c_float]),
    "rtp_display_fit_scale": (C.c_double, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rtp_resize_area": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int]),
    "rtp_warp_display": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "rtp_preprocess_frame": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, fp, C.POINTER(C.c_ubyte), fp]),
    "rtp_load_image": (C.c_int, [C.c_char_p, C.POINTER(C.c_ubyte), C.c_size_t, ip, ip]),
    "rtp_synth_frame": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "rtp_prototxt_summary": (C.c_int, [C.c_char_p, ip, ip, ip, ip, fp, ip]),
    "rtp_last_error": (C.c_char_p, [vp]),
    "rtp_version": (C.c_char_p, []),
    "rtp_last_stage_ms": (C.c_int, [vp, fp]),
    "rtp_debug_connect_stats": (C.c_int, [vp, ip, ip]),
    "rtp_synth_weights": (C.c_int, [C.c_uint64, C.c_char_p, C.c_int, C.c_int, C.c_int, fp, fp]),
    "rtp_write_synthetic_caffemodel": (C.c_int, [C.c_int, C.c_uint64, C.c_char_p]),
    "rtp_write_builtin_prototxt": (C.c_int, [C.c_int, C.c_char_p]),
    "rtp_caffemodel_layer": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, ip, C.POINTER(C.c_long), C.POINTER(C.c_long), fp]),
    "rtp_plan_summary": (C.c_long, [C.POINTER(rtp_config), C.c_char_p, C.c_size_t]),
    "rtp_kernel_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "rtp_bench_dominant_conv": (C.c_int, [vp, C.c_int, fp, C.POINTER(C.c_double)]),
    "rtp_calibrate_precision": (C.c_int, [vp, fp, C.c_int, C.c_float, C.c_char_p, C.c_size_t, fp, fp]),
    "rtp_calibration_report": (C.c_char_p, [vp]),
    "rtp_get_split_layers": (C.c_int, [vp, C.c_char_p, C.c_size_t, ip]),
    "rtp_device_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "rtp_device_free": (C.c_int, [vp, vp]),
    "rtp_device_upload": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "rtp_device_synchronize": (C.c_int, [vp]),
    "rtp_weight_blob_bytes": (C.c_long, [vp]),
    "rtp_weight_blob_export": (C.c_int, [vp, vp, C.c_size_t]),
    "rtp_weight_blob_import": (C.c_int, [vp, vp, C.c_size_t]),
    "rtp_copy_weights_from": (C.c_int, [vp, vp]),
    "rtp_device_local_cpus": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "rtp_submit_frame_device": (C.c_int, [vp, C.POINTER(rtp_frame_view), vp, C.c_uint64, fp]),
    "rtp_collect_rendered_device": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(rtp_frame_view), vp]),
    "rtp_jpeg_max_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "rtp_encode_jpeg_device": (C.c_int, [vp, C.POINTER(rtp_frame_view), C.c_int, vp, C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_size_t)]),
    "rtp_set_render_jpeg": (C.c_int, [vp, C.c_int]),
    "rtp_collect_rendered_jpeg": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_size_t)]),
    "rtp_convert_yuv": (C.c_int, [C.POINTER(rtp_yuv_view), C.POINTER(C.c_ubyte), C.c_size_t]),
    "rtp_video_chroma": (C.c_int, [vp]),
    "rtp_video_read_yuv": (C.c_int, [vp, C.POINTER(rtp_yuv_view)]),
    "rtp_submit_frame_yuv": (C.c_int, [vp, C.POINTER(rtp_yuv_view), C.c_uint64, fp]),
    "rtp_submit_frame_yuv_device": (C.c_int, [vp, C.POINTER(rtp_yuv_view), vp, C.c_uint64, fp]),
    "rtp_convert_yuv_device": (C.c_int, [vp, C.POINTER(rtp_yuv_view), C.POINTER(rtp_frame_view), vp]),
    "rtp_video_read_jpeg": (C.c_int, [vp, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_size_t)]),
    "rtp_decode_jpeg_device": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(rtp_frame_view), vp, ip]),
    "rtp_submit_frame_jpeg": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_size_t, C.c_uint64, fp, ip, ip]),
    "rtp_convert_bgr_to_yuv": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_long, C.POINTER(rtp_yuv_view)]),
    "rtp_yuv_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "rtp_video_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "rtp_video_write_yuv": (C.c_int, [vp, C.POINTER(rtp_yuv_view)]),
    "rtp_video_write_jpeg": (C.c_int, [vp, C.POINTER(C.c_ubyte), C.c_size_t]),
    "rtp_video_finish": (C.c_int, [vp]),
    "rtp_convert_to_yuv_device": (C.c_int, [vp, C.POINTER(rtp_frame_view), C.POINTER(rtp_yuv_view), vp]),
    "rtp_set_render_yuv": (C.c_int, [vp, C.c_int]),
    "rtp_collect_rendered_yuv": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(C.c_ubyte), C.c_size_t]),
    "rtp_collect_rendered_yuv_device": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(rtp_yuv_view), vp]),
    "rtp_set_maps_output": (C.c_int, [vp, C.POINTER(rtp_maps_config)]),
    "rtp_maps_info": (C.c_int, [vp, ip, ip, C.POINTER(C.c_size_t)]),
    "rtp_peek_maps": (C.c_int, [vp, C.POINTER(C.c_uint64), vp, C.c_size_t]),
    "rtp_peek_maps_device": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(rtp_maps_view), vp]),
    "rtp_maps_from_lowres": (C.c_int, [vp, fp, vp, C.c_size_t]),
    "rtp_maps_quantize_u8": (C.c_int, [fp, C.c_size_t, C.c_int, C.POINTER(C.c_ubyte)]),
    "rtp_maps_to_f16": (C.c_int, [fp, C.c_size_t, C.POINTER(C.c_uint16)]),
    "rtp_crop_people": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, fp, C.c_int, C.c_int, C.POINTER(rtp_crops_config), fp, C.POINTER(C.c_ubyte)]),
    "rtp_set_crops_output": (C.c_int, [vp, C.POINTER(rtp_crops_config)]),
    "rtp_crops_info": (C.c_int, [vp, ip, ip, ip, ip, C.POINTER(C.c_size_t)]),
    "rtp_peek_crops": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.POINTER(C.c_ubyte), C.c_int, ip]),
    "rtp_peek_crops_device": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, ip, C.c_int, C.POINTER(rtp_crops_view), vp]),
    "rtp_crops_from_joints": (C.c_int, [vp, C.POINTER(C.c_ubyte), fp, C.c_int, fp, ip, C.POINTER(C.c_ubyte), C.c_int]),
    "rtp_crops_head_parts": (C.c_int, [C.c_int, ip]),
    "rtp_track_config_default": (C.c_int, [C.POINTER(rtp_track_config)]),
    "rtp_track_state_init": (C.c_int, [C.POINTER(rtp_track_state), C.c_int]),
    "rtp_track_update": (C.c_int, [C.POINTER(rtp_track_state), C.POINTER(rtp_track_config), fp, C.c_int, ip]),
    "rtp_set_tracking": (C.c_int, [vp, C.POINTER(rtp_track_config)]),
    "rtp_track_reset": (C.c_int, [vp]),
    "rtp_track_get_state": (C.c_int, [vp, C.POINTER(rtp_track_state)]),
    "rtp_track_set_state": (C.c_int, [vp, C.POINTER(rtp_track_state)]),
    "rtp_peek_tracks": (C.c_int, [vp, C.POINTER(C.c_uint64), ip, ip, C.c_int]),
    "rtp_track_from_joints": (C.c_int, [vp, fp, C.c_int, ip, ip, C.c_int]),
    "rtp_format_json_tracked": (C.c_long, [C.c_char_p, C.c_size_t, fp, C.c_int, C.c_int, C.c_float, ip]),
    "rtp_appearance_config_default": (C.c_int, [C.POINTER(rtp_appearance_config)]),
    "rtp_appearance_state_init": (C.c_int, [C.POINTER(rtp_appearance_state)]),
    "rtp_appearance_torso_parts": (C.c_int, [C.c_int, ip]),
    "rtp_appearance_describe": (C.c_int, [C.POINTER(C.c_ubyte), C.c_int, C.c_int, fp, C.c_int, C.c_int, C.POINTER(rtp_appearance_config), C.POINTER(C.c_uint16),
                                          C.POINTER(C.c_ubyte)]),
    "rtp_track_update_appearance": (C.c_int, [C.POINTER(rtp_track_state), C.POINTER(rtp_appearance_state), C.POINTER(rtp_track_config),
                                              C.POINTER(rtp_appearance_config), fp, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte), ip]),
    "rtp_set_track_appearance": (C.c_int, [vp, C.POINTER(rtp_appearance_config)]),
    "rtp_appearance_reset": (C.c_int, [vp]),
    "rtp_appearance_get_state": (C.c_int, [vp, C.POINTER(rtp_appearance_state)]),
    "rtp_appearance_set_state": (C.c_int, [vp, C.POINTER(rtp_appearance_state)]),
    "rtp_peek_appearance": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte), ip, C.c_int]),
    "rtp_appearance_from_joints": (C.c_int, [vp, C.POINTER(C.c_ubyte), fp, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte), ip, C.c_int]),
    "rtp_track_from_frame": (C.c_int, [vp, C.POINTER(C.c_ubyte), fp, C.c_int, ip, C.POINTER(C.c_uint16), C.POINTER(C.c_ubyte), ip, C.c_int]),
    "rtp_smooth_config_default": (C.c_int, [C.POINTER(rtp_smooth_config)]),
    "rtp_smooth_state_init": (C.c_int, [C.POINTER(rtp_smooth_state), C.c_int]),
    "rtp_smooth_update": (C.c_int, [C.POINTER(rtp_smooth_state), C.POINTER(rtp_smooth_config), fp, C.c_int, ip, fp, fp, C.POINTER(C.c_ubyte)]),
    "rtp_set_smoothing": (C.c_int, [vp, C.POINTER(rtp_smooth_config)]),
    "rtp_smooth_reset": (C.c_int, [vp]),
    "rtp_smooth_get_state": (C.c_int, [vp, C.POINTER(rtp_smooth_state)]),
    "rtp_smooth_set_state": (C.c_int, [vp, C.POINTER(rtp_smooth_state)]),
    "rtp_peek_smoothed": (C.c_int, [vp, C.POINTER(C.c_uint64), fp, fp, C.POINTER(C.c_ubyte), ip, C.c_int]),
    "rtp_smooth_from_joints": (C.c_int, [vp, fp, C.c_int, ip, fp, fp, C.POINTER(C.c_ubyte), ip, C.c_int]),
    "rtp_overlay_config_default": (C.c_int, [C.POINTER(rtp_overlay_config)]),
    "rtp_trail_state_init": (C.c_int, [C.POINTER(rtp_trail_state), C.c_int]),
    "rtp_overlay_update": (C.c_int, [C.POINTER(rtp_trail_state), C.POINTER(rtp_overlay_config), fp, C.c_int, ip, ip, ip, C.c_int]),
    "rtp_overlay_draw": (C.c_int, [ip, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_long]),
    "rtp_set_track_overlay": (C.c_int, [vp, C.POINTER(rtp_overlay_config)]),
    "rtp_overlay_reset": (C.c_int, [vp]),
    "rtp_overlay_get_state": (C.c_int, [vp, C.POINTER(rtp_trail_state)]),
    "rtp_overlay_set_state": (C.c_int, [vp, C.POINTER(rtp_trail_state)]),
    "rtp_peek_overlay_items": (C.c_int, [vp, C.POINTER(C.c_uint64), ip, ip, C.c_int]),
    "rtp_overlay_from_joints": (C.c_int, [vp, fp, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, ip, ip, ip, C.c_int]),
    "rtp_redact_config_default": (C.c_int, [C.POINTER(rtp_redact_config)]),
    "rtp_redact_regions": (C.c_int, [fp, C.c_int, C.c_int, C.POINTER(rtp_redact_config), ip]),
    "rtp_redact_apply": (C.c_int, [ip, C.c_int, C.POINTER(rtp_redact_config), C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_long]),
    "rtp_set_redaction": (C.c_int, [vp, C.POINTER(rtp_redact_config)]),
    "rtp_redaction_info": (C.c_int, [vp, C.POINTER(rtp_redact_config), ip]),
    "rtp_peek_redactions": (C.c_int, [vp, C.POINTER(C.c_uint64), ip, ip, C.c_int]),
    "rtp_redact_from_joints": (C.c_int, [vp, fp, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, ip, ip, C.c_int]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args
