"""Maps mode without a GPU: the two host quantisers against numpy bit for bit, the Python wrapper's argument checks, the NULL-engine
refusals of the C entries, the CLI's --write_heatmaps under --dry_engine, and the build rules of the new kernel file."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _mapscases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
CSRC = os.path.join(ROOT, "caffe_rtpose_amd", "csrc")


def test_symbols_are_declared_exported_and_wrapped():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    header = open(os.path.join(ROOT, "include", "rtpose_mi355x.h")).read()
    for name in ("rtp_set_maps_output", "rtp_maps_info", "rtp_peek_maps", "rtp_peek_maps_device", "rtp_maps_from_lowres", "rtp_maps_quantize_u8", "rtp_maps_to_f16"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    for name in ("set_maps_output", "maps_info", "peek_maps", "peek_maps_device", "maps_from_lowres"):
        assert hasattr(r.Engine, name), name
    assert callable(r.maps_quantize_u8) and callable(r.maps_to_f16)
    assert hasattr(_lib.lib, "rtp_internal_maps_export_layout") and "rtp_internal_maps_export_layout" not in header
    assert C.sizeof(_lib.rtp_maps_config) == 32 and C.sizeof(_lib.rtp_maps_view) == 32   # the header's structs on LP64


@pytest.mark.parametrize("is_paf", [False, True])
def test_u8_quantiser_is_numpy_bit_for_bit(is_paf):
    import caffe_rtpose_amd as r
    v = mc.quantiser_grid(is_paf)
    ties = mc.u8_exact_ties(is_paf)
    assert len(ties) >= 250, "the grid must hold the exact ties k + 0.5"
    got, want = r.maps_quantize_u8(v, is_paf), mc.u8_ref(v, is_paf)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # round half to even on the exact ties, the clamps, NaN -> 0
    q = r.maps_quantize_u8(ties, is_paf)
    inside = (q > 0) & (q < 255)
    assert inside.sum() >= 250 and (q[inside] % 2 == 0).all()
    edge = r.maps_quantize_u8(np.array([np.nan, -np.nan, np.inf, -np.inf, 7.0, -7.0, 1e-45], np.float32), is_paf)
    assert list(edge) == ([0, 0, 255, 0, 255, 0, 128] if is_paf else [0, 0, 255, 0, 255, 0, 0])


def test_f16_conversion_is_numpy_bit_for_bit():
    import caffe_rtpose_amd as r
    v = mc.f16_grid()
    got, want = r.maps_to_f16(v), mc.f16_ref(v)
    assert got.dtype == np.float16 and mc.same_f16(got, want), v[np.flatnonzero(got.view(np.uint16) != want.view(np.uint16))[:10]]
    assert np.isnan(v).any() and np.array_equal(np.isnan(got), np.isnan(v))
    # EVERY binary16 value converts to itself, and every midpoint between two neighbours goes to the even one
    h = np.arange(0, 0x7c00, dtype=np.uint16)
    f = h.view(np.float16).astype(np.float32)
    assert np.array_equal(r.maps_to_f16(f).view(np.uint16), h)
    nxt = (h + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    nxt[-1] = 65536.0
    mid = ((f.astype(np.float64) + nxt) / 2).astype(np.float32)
    assert np.array_equal(r.maps_to_f16(mid).view(np.uint16), h + (h & 1))
    assert mc.same_f16(r.maps_to_f16(mid), mc.f16_ref(mid)) and mc.same_f16(r.maps_to_f16(-mid), mc.f16_ref(-mid))


def test_wrapper_refuses_bad_arguments_before_the_library_is_called():
    import caffe_rtpose_amd as r
    e = r.Engine.__new__(r.Engine)   # no device here: an engine that would fault on any library call (NULL handle)
    e.h, e.heat_channels = C.c_void_p(), 57
    for kw in (dict(grid="display"), dict(grid=0), dict(fmt="bf16"), dict(fmt=2), dict(channels=[57]), dict(channels=[-1]), dict(channels=[0, 3, 99]),
               dict(channels=[]), dict(channels=list(range(57)) + list(range(14)))):
        with pytest.raises(ValueError):
            e.set_maps_output(**kw)
    with pytest.raises(r.RtpError) as ex:   # valid arguments reach the library, which refuses the NULL engine
        e.set_maps_output("net", "u8", [0, 1])
    assert ex.value.code == r.RTP_EINVAL
    with pytest.raises(r.RtpError):
        e.maps_info()
    e.h = C.c_void_p()   # (nothing to destroy)


def test_c_entries_refuse_a_null_engine():
    import caffe_rtpose_amd as r
    from caffe_rtpose_amd import _lib
    lib = _lib.lib
    cfg = _lib.rtp_maps_config()
    cfg.struct_size = C.sizeof(cfg)
    tag = C.c_uint64(77)
    buf = np.full(16, 0xAB, np.uint8)
    view = _lib.rtp_maps_view()
    view.struct_size = C.sizeof(view)
    assert lib.rtp_set_maps_output(None, C.byref(cfg)) == r.RTP_EINVAL and b"NULL engine" in lib.rtp_last_error(None)
    assert lib.rtp_set_maps_output(None, None) == r.RTP_EINVAL
    assert lib.rtp_peek_maps(None, C.byref(tag), buf.ctypes.data_as(C.c_void_p), buf.size) == r.RTP_EINVAL and b"rtp_peek_maps" in lib.rtp_last_error(None)
    assert lib.rtp_peek_maps_device(None, C.byref(tag), C.byref(view), None) == r.RTP_EINVAL
    assert lib.rtp_maps_from_lowres(None, None, buf.ctypes.data_as(C.c_void_p), buf.size) == r.RTP_EINVAL
    assert lib.rtp_maps_info(None, None, None, None) == r.RTP_EINVAL
    assert tag.value == 77 and (buf == 0xAB).all()   # a refused call writes nothing
    assert lib.rtp_maps_quantize_u8(None, 4, 0, None) == r.RTP_EINVAL and lib.rtp_maps_to_f16(None, 4, None) == r.RTP_EINVAL
    assert lib.rtp_maps_quantize_u8(None, 0, 0, None) == r.RTP_OK


def test_cli_help_lists_the_flags():
    p = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert p.returncode == 0
    assert b"--write_heatmaps PREFIX" in p.stdout and b"--heatmap_channels parts|bkg|parts+bkg|pafs|all" in p.stdout and b"%06d.pgm" in p.stdout


@pytest.mark.parametrize("channels,nch", [(None, 19), ("parts", 18), ("bkg", 1), ("pafs", 38), ("all", 57)])
def test_cli_dry_engine_writes_well_formed_pgm_files_in_frame_order(tmp_path, channels, nch):
    prefix = tmp_path / "maps_"
    cmd = [BIN, "--video", "synthetic:320x180:5", "--model", "coco", "--net_resolution", "160x96", "--resolution", "320x180", "--dry_engine", "400",
           "--no_frame_drops", "--no_display", "--num_gpu", "2", "--write_heatmaps", str(prefix)] + (["--heatmap_channels", channels] if channels else [])
    p = subprocess.run(cmd, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    files = sorted(os.listdir(tmp_path))
    assert files == ["maps_%06d.pgm" % i for i in range(5)], files
    for f in files:
        img = mc.read_pgm(tmp_path / f)
        assert img.shape == (nch * 96, 160) and not img.any(), f     # --dry_engine: zeros
    # written by the display thread behind the re-orderer: creation order = frame order
    stamps = [os.stat(tmp_path / f).st_mtime_ns for f in files]
    assert stamps == sorted(stamps)


def test_cli_refuses_an_unknown_channel_set(tmp_path):
    p = subprocess.run([BIN, "--video", "synthetic:320x180:2", "--model", "coco", "--dry_engine", "400", "--write_heatmaps", str(tmp_path / "m"), "--heatmap_channels", "limbs"],
                       capture_output=True, timeout=60)
    assert p.returncode == 1 and b"--heatmap_channels" in p.stderr and not os.listdir(tmp_path)


def test_kernel_file_is_built_bit_exact_and_without_packed_f32():
    """maps_export.hip promises rtp_resize's bits: it shares resize_math.h with postproc.hip and is built with the same flags; like
    postproc.hip it must hold no packed-f32 VALU instruction."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^EXTRA_maps_export = \$\(BITEXACT\)$", mk, re.M)
    assert "build/maps_export.o" in mk and "build/engine_maps.o" in mk
    for f in ("maps_export.hip", "postproc.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "resize_math.h"' in src and "resize_block8(" in src, f
        assert "CubicCoef cubic_coef" not in src, f + ": one definition of the arithmetic, in resize_math.h"
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fno-vectorize", "--cuda-device-only", "-S",
                          "-o", "-", os.path.join(CSRC, "maps_export.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "maps_net_kernel" in out.stdout and not re.search(r"v_pk_[a-z]*_f32", out.stdout)
    assert re.search(r"global_store_dwordx4", out.stdout) and re.search(r"global_store_dwordx2", out.stdout), "the wide epilogues store 16 / 8 bytes at once"
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", out.stdout)]
    assert spills and not any(spills), "the 64 accumulators of a block stay in registers"
