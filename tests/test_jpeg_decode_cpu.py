"""The host side of the GPU JPEG decoder, without a GPU: the planner (which files get their Huffman decoding on the device), and the
serial emulation of the device's self-synchronising decoder (the same per-symbol step, subsequences, rounds and final pass, compiled
for the host) against the coefficients of codecs.cpp's own entropy decoder.  Equality is exact.  Files: Pillow's baseline fixtures, the
generated 4:2:0 grid, and the layout fixtures (_jpegcases.LAYOUTS: MCUs of 1 to 10 blocks, restart interval 1, tables under id 3)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import _jpegcases as jc

ROOT = jc.ROOT
BIN = os.path.join(ROOT, "caffe_rtpose_amd", "rtpose.bin")
SETTINGS = [(s, g) for s in (32, 64, 1024) for g in (4, 64)]   # S bits per subsequence, subsequences per workgroup


def test_symbols_are_declared_exported_and_wrapped():
    import caffe_rtpose_amd as r
    header = open(os.path.join(ROOT, "include", "rtpose_mi355x.h")).read()
    for name in ("rtp_decode_jpeg_device", "rtp_submit_frame_jpeg", "rtp_video_read_jpeg", "RTP_JPEG_ENTROPY_DEVICE", "RTP_JPEG_ENTROPY_HOST"):
        assert name in header, name
    for name in ("rtp_decode_jpeg_device", "rtp_submit_frame_jpeg", "rtp_video_read_jpeg", "rtp_internal_jpeg_entropy_emulate",
                 "rtp_internal_jpeg_coefficients", "rtp_internal_jpeg_decode_device", "rtp_internal_jpeg_reconstruct_device",
                 "rtp_internal_jpeg_reconstruct_host"):
        assert hasattr(r.lib, name), name
        if name.startswith("rtp_internal"):
            assert name not in header, name
    for name in ("decode_jpeg_device", "submit_frame_jpeg"):
        assert callable(getattr(r.Engine, name)), name
    assert callable(r.Video.read_jpeg)
    p = subprocess.run([BIN, "--help"], capture_output=True)
    assert b"--host_decode" in p.stdout + p.stderr and b"--gpu_decode" in p.stdout + p.stderr


def _check_file(name, data):
    rc, info = jc.plan(data)
    assert rc == 0, (name, jc.codec_error())
    assert info[0] == jc.DEVICE, (name, info)
    rc, want = jc.host_coefficients(data)
    assert rc == 0, name
    for s, g in SETTINGS:
        rc, got, info2, rounds = jc.emulate(data, s, g, info[7])
        assert rc == 0, (name, s, g, jc.codec_error())
        assert info2[0] == jc.DEVICE and info2[5] >= info[6] * 32 // s, (name, s, g, info2)
        groups = (info2[5] + g - 1) // g
        assert 1 <= rounds[0] <= groups and rounds[1] <= g, (name, s, g, rounds, groups)
        assert np.array_equal(got, want), (name, s, g)


@pytest.mark.parametrize("name", jc.BASELINE)
def test_emulation_equals_host_entropy_decoder_on_fixtures(name):
    """every baseline fixture is a single-scan sequential file: planned for the device, and the emulation's coefficients are the host's"""
    _check_file(name, jc.fixture(name))


@pytest.mark.parametrize("size", jc.SIZES, ids=[f"{w}x{h}" for w, h in jc.SIZES])
def test_emulation_equals_host_entropy_decoder_on_generated_files(size):
    tag = f"_{size[0]}x{size[1]}_"
    cases = [(n, d) for n, d in jc.grid() if tag in n]
    assert len(cases) == len(jc.KINDS) * len(jc.QUALITIES)
    for n, d in cases:
        _check_file(n, d)


DEVICE_LAYOUTS = sorted(n for n, p in jc.LAYOUTS.items() if p == jc.DEVICE)
HOST_LAYOUTS = sorted(n for n, p in jc.LAYOUTS.items() if p == jc.HOST)


def test_layout_table_names_every_file():
    assert jc.layout_files() == sorted(jc.LAYOUTS)
    assert len(HOST_LAYOUTS) == 4 and len(DEVICE_LAYOUTS) == 27


@pytest.mark.parametrize("name", DEVICE_LAYOUTS)
def test_emulation_equals_host_entropy_decoder_on_device_layouts(name):
    """MCUs of 1 to 10 blocks in every block map the fixtures have, restart interval 1, tables under id 3: planned for the device"""
    _check_file(name, jc.layout(name)[0])


@pytest.mark.parametrize("name", HOST_LAYOUTS)
def test_host_layouts_take_the_host_entropy_path(name):
    """one scan per component, fill bytes in front of RSTn, a quantiser redefined between scans"""
    data = jc.layout(name)[0]
    hrc, hmsg = jc.host_decode(data)
    rc, info = jc.plan(data)
    assert rc == hrc == 0, (name, hmsg, jc.codec_error())
    assert info[0] == jc.HOST and info[5] == 0, (name, info)
    rc, want = jc.host_coefficients(data)
    rc2, got, info2, rounds = jc.emulate(data, 32, 4, info[7])
    assert rc == 0 and rc2 == hrc and info2[0] == jc.HOST and rounds == [0, 0], (name, info2, rounds)
    assert np.array_equal(got, want), name


def _mcu_blocks(data):
    comps = jc.frame_components(data)
    return sum(h * v for _, h, v, _ in comps) if len(comps) > 1 else 1


def test_layouts_reach_the_mcu_block_limit():
    """the device layouts hold MCUs of 8, 9 and 10 (= JD_MAX_MCU_BLOCKS) blocks, and info[7] counts whole MCUs of them"""
    seen = {}
    for name in DEVICE_LAYOUTS:
        data = jc.layout(name)[0]
        comps = jc.frame_components(data)
        rc, info = jc.plan(data)
        assert rc == 0 and info[0] == jc.DEVICE
        hmax, vmax = (max(c[1] for c in comps), max(c[2] for c in comps)) if len(comps) > 1 else (1, 1)
        mcus = -(-info[1] // (8 * hmax)) * -(-info[2] // (8 * vmax))
        assert info[7] == mcus * _mcu_blocks(data), (name, info)
        seen.setdefault(_mcu_blocks(data), []).append(name)
    assert set(seen) >= {1, 3, 4, 5, 6, 8, 9, 10} and max(seen) == 10, seen
    assert len(seen[10]) >= 3 and any("dri1" in n for n in seen[10]), seen[10]
    rc, info = jc.plan(jc.layout("l42_dri1_40x20")[0])
    assert info[4] == 4, info   # every MCU its own restart segment


def _bits_to_scan(bits):
    bits += "1" * (-len(bits) % 8)
    out = bytearray()
    for i in range(0, len(bits), 8):
        out.append(int(bits[i:i + 8], 2))
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out)


def test_more_than_ten_blocks_per_mcu_fall_back_to_the_host_path():
    """every component 2x2: 12 blocks per MCU.  libjpeg refuses the file (no reference pixels); the host decoder accepts it, so the
    planner must hand it to the host without an error.  Written here: one DC table {0: '0', 3: '10'}, one AC table {EOB: '0', 0/1: '10'}."""
    W, H = 20, 17   # 2 x 2 MCUs of 16 x 16
    seg = lambda m, p: bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + bytes(p)
    head = b"\xff\xd8" + seg(0xDB, [0] + [3] * 64)
    head += seg(0xC0, [8, 0, H, 0, W, 3, 1, 0x22, 0, 2, 0x22, 0, 3, 0x22, 0])
    head += seg(0xC4, [0x00, 1, 1] + [0] * 14 + [0, 3]) + seg(0xC4, [0x10, 1, 1] + [0] * 14 + [0x00, 0x01])
    head += seg(0xDA, [3, 1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0])
    rng = np.random.default_rng(12)
    bits, want, pred = "", np.zeros((3, 4, 4, 64), np.int16), [0, 0, 0]   # want: component, block row, block column
    for my in range(2):
        for mx in range(2):
            for c in range(3):
                for by in range(2):
                    for bx in range(2):
                        diff = int(rng.choice([0, 0, 4, 7, -4, -6]))
                        bits += "0" if diff == 0 else "10" + format(diff if diff > 0 else diff + 7, "03b")
                        pred[c] += diff
                        want[c, 2 * my + by, 2 * mx + bx, 0] = pred[c]
                        ac = int(rng.choice([0, 1, -1]))
                        want[c, 2 * my + by, 2 * mx + bx, 1] = ac
                        bits += "0" if ac == 0 else "10" + ("1" if ac > 0 else "0") + "0"
    data = head + _bits_to_scan(bits) + b"\xff\xd9"
    hrc, hmsg = jc.host_decode(data)
    assert hrc == 0, hmsg
    rc, info = jc.plan(data)
    assert rc == 0 and info[0] == jc.HOST and info[5] == 0 and info[7] == 48, info
    rc, host = jc.host_coefficients(data)
    assert rc == 0 and np.array_equal(host, want.reshape(-1))
    for s, g in SETTINGS:
        rc, got, info2, rounds = jc.emulate(data, s, g, info[7])
        assert rc == 0 and info2[0] == jc.HOST and rounds == [0, 0], (s, g, info2, rounds)
        assert np.array_equal(got, host), (s, g)


def test_restart_fixture_has_several_anchored_segments():
    rc, info = jc.plan(jc.fixture("j420_rst"))
    assert rc == 0 and info[0] == jc.DEVICE and info[4] > 1, info


def test_progressive_files_take_the_host_entropy_path():
    names = jc.progressive_names()
    assert len(names) >= 6
    for name in names:
        data = jc.fixture(name)
        rc, info = jc.plan(data)
        assert rc == 0 and info[0] == jc.HOST and info[5] == 0, (name, info)
        rc, want = jc.host_coefficients(data)
        rc2, got, info2, rounds = jc.emulate(data, 64, 4, info[7])
        assert rc == 0 and rc2 == 0 and info2[0] == jc.HOST and rounds == [0, 0]
        assert np.array_equal(got, want), name


def test_irregular_files_fall_back_to_the_host_path():
    """nothing may fail that the host decoder accepts: a missing restart marker, a marker out of order, tables behind the scan"""
    data = bytearray(jc.fixture("j420_rst"))
    start = jc.scan_start(data)
    marks = [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(marks) >= 2
    swapped = bytearray(data)
    swapped[marks[0] + 1], swapped[marks[1] + 1] = data[marks[1] + 1], data[marks[0] + 1]
    removed = bytearray(data)
    del removed[marks[0]:marks[0] + 2]
    base = jc.fixture("j420_q75")
    assert base.endswith(b"\xff\xd9")
    tables_behind = base[:-2] + b"\xff\xdb\x00\x43\x00" + bytes(range(1, 65)) + b"\xff\xd9"
    for what, d in (("swapped", bytes(swapped)), ("removed", bytes(removed)), ("tables", tables_behind)):
        hrc, hmsg = jc.host_decode(d)
        rc, info = jc.plan(d)
        assert rc == hrc, (what, rc, hrc, hmsg)
        if rc == 0:
            assert info[0] == jc.HOST, (what, info)
            rc, want = jc.host_coefficients(d)
            rc2, got, _, _ = jc.emulate(d, 32, 4, info[7])
            assert rc == 0 and rc2 == 0 and np.array_equal(got, want), what


def test_rejected_files_give_the_host_decoders_error():
    data = jc.fixture("j420_q75")
    sof = data.index(b"\xff\xc0")
    cut = data[: sof + 7]   # inside the frame header
    hrc, hmsg = jc.host_decode(cut)
    assert hrc != 0
    rc, _ = jc.plan(cut)
    assert (rc, jc.codec_error()) == (hrc, hmsg)
    rc, _, _, _ = jc.emulate(cut, 64, 4, 1)
    assert (rc, jc.codec_error()) == (hrc, hmsg)
    # a Huffman code the tables do not have, somewhere in the scan: the first byte value that makes the host decoder fail
    start = jc.scan_start(data)
    _, info = jc.plan(data)
    found = 0
    for pos in range(start + 8, len(data) - 2, 7):
        d = bytearray(data)
        d[pos] = 0xFE if d[pos] != 0xFE else 0xFD
        d = bytes(d)
        hrc, hmsg = jc.host_decode(d)
        if hrc == 0 or "corrupt" not in hmsg:   # (decodable all the same, or the byte made a marker of its neighbour)
            continue
        found += 1
        rc, pinfo = jc.plan(d)
        assert rc == 0 and pinfo[0] == jc.DEVICE   # the planner does not decode: the scan goes to the device
        for s, g in ((32, 4), (1024, 64)):
            rc, _, _, _ = jc.emulate(d, s, g, info[7])
            assert (rc, jc.codec_error()) == (hrc, hmsg), (pos, s, g)
        if found == 5:
            break
    assert found >= 1


def test_truncated_scan_decodes_with_zero_bits_like_the_host():
    for name in ("j420_q75", "j420_rst", "jgray_q88"):
        data = jc.fixture(name)
        start = jc.scan_start(data)
        for frac in (0.0, 0.3, 0.8):
            cut = data[: start + int((len(data) - start) * frac)]
            hrc, hmsg = jc.host_decode(cut)
            rc, info = jc.plan(cut)
            assert rc == hrc, (name, frac, hmsg)
            if rc:
                continue
            rc, want = jc.host_coefficients(cut)
            assert rc == 0
            for s, g in ((32, 4), (64, 64), (1024, 4)):
                rc, got, info2, _ = jc.emulate(cut, s, g, info[7])
                assert rc == 0 and np.array_equal(got, want), (name, frac, s, g, info2)


def test_mutated_files_same_error_or_same_coefficients():
    """every outcome is the host decoder's: its error (code and message), or its coefficients; never a crash"""
    rnd = random.Random(4321)
    agreed_ok = agreed_err = on_device = 0
    for name in ("j420_tiny", "j420_rst"):
        base = jc.fixture(name)
        start = jc.scan_start(base)
        for it in range(700 if name == "j420_tiny" else 300):
            d = bytearray(base)
            mode = rnd.random()
            if mode < 0.45:   # in the scan
                for _ in range(rnd.randint(1, 4)):
                    d[rnd.randrange(start, len(d))] = rnd.randrange(256)
            elif mode < 0.65:   # anywhere
                for _ in range(rnd.randint(1, 4)):
                    d[rnd.randrange(len(d))] = rnd.randrange(256)
            elif mode < 0.8:
                d = d[: rnd.randrange(1, len(d))]
            elif mode < 0.9:
                i = rnd.randrange(len(d))
                d[i:i] = bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 8)))
            else:
                i = rnd.randrange(len(d) - 2)
                d[i] = 0xFF
                d[i + 1] = rnd.choice([0xC0, 0xC2, 0xC4, 0xDA, 0xDB, 0xDD, 0xD9, 0xD0, 0xD3, 0x00, 0xFF])
            d = bytes(d)
            hrc, hmsg = jc.host_decode(d)
            s, g = rnd.choice(SETTINGS)
            if hrc:
                rc, info = jc.plan(d)
                blocks = info[7] if rc == 0 else 1
                rc, _, _, _ = jc.emulate(d, s, g, blocks)
                assert (rc, jc.codec_error()) == (hrc, hmsg), (name, it)
                agreed_err += 1
                continue
            rc, info = jc.plan(d)
            assert rc == 0, (name, it, jc.codec_error())
            rc, want = jc.host_coefficients(d)
            assert rc == 0
            rc, got, info2, _ = jc.emulate(d, s, g, info[7])
            assert rc == 0, (name, it, jc.codec_error())
            assert np.array_equal(got, want), (name, it, s, g, info2)
            agreed_ok += 1
            on_device += info2[0] == jc.DEVICE
    assert agreed_ok > 100 and agreed_err > 100 and on_device > 50, (agreed_ok, agreed_err, on_device)


def test_host_reconstruction_counterpart_equals_the_decoder():
    """coefficients + quantisers -> pixels (the host counterpart of the reconstruction kernels) = rtp_decode_image"""
    import caffe_rtpose_amd as r
    data = jc.fixture("j420_q75")
    rc, coef = jc.host_coefficients(data)
    assert rc == 0
    # quantisers of the file, natural order, per component
    zz = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
    tabs = {}
    i = 2
    while data[i + 1] != 0xDA:
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDB:
            o = i + 4
            while o < i + 2 + ln:
                t = np.zeros(64, np.uint16)
                for k in range(64):
                    t[zz[k]] = data[o + 1 + k]
                tabs[data[o] & 15] = t
                o += 65
        i += 2 + ln
    qn = np.stack([tabs[0], tabs[1], tabs[1]])
    want = r.decode_image(data)
    h, w = want.shape[:2]
    hv = (C.c_int * 6)(2, 2, 1, 1, 1, 1)
    out = np.zeros_like(want)
    rc = r.lib.rtp_internal_jpeg_reconstruct_host(w, h, 3, hv, qn.ctypes.data_as(C.c_void_p), 0, coef.ctypes.data_as(C.c_void_p),
                                                  out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size))
    assert rc == 0, jc.codec_error()
    assert np.array_equal(out, want)


def test_video_read_jpeg_walks_the_stream(tmp_path):
    import caffe_rtpose_amd as r
    a, b = jc.fixture("j420_q75"), jc.fixture("j444_q90")
    m = tmp_path / "clip.mjpeg"
    m.write_bytes(a + b + a)
    v1, v2 = r.Video(m), r.Video(m)
    for want in (a, b, a):
        got = v1.read_jpeg()
        assert got == want
        assert np.array_equal(r.decode_image(got), v2.read())
    assert v1.read_jpeg() is None and v2.read() is None
    v1.close()
    v2.close()
    y = tmp_path / "c.y4m"
    y.write_bytes(b"YUV4MPEG2 W2 H2 F25:1 C420\nFRAME\n" + bytes(6))
    v = r.Video(y)
    with pytest.raises(r.RtpError) as ei:
        v.read_jpeg()
    assert ei.value.code == r.RTP_EINVAL
    assert v.read() is not None   # nothing was consumed
    v.close()
