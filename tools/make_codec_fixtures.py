#!/usr/bin/env python
"""Golden vectors for csrc/codecs.cpp, made in the BUILD container with Pillow (bundled libjpeg-turbo /
libpng — the decoders cv::imread would run): small JPEG/PNG files plus the pixels they decode to.
    python tools/make_codec_fixtures.py          -> tests/golden/codecs/*.{jpg,png,npy}
    python tools/make_codec_fixtures.py --layouts -> tests/golden/codecs/layouts/*.{jpg,npy} only: sampling factors, scan structures,
                                                     quantisers and colour markers Pillow cannot write, from a baseline writer below
JPEG expectations are PIL's decode (libjpeg default path: islow IDCT, fancy up-sampling);
PNG expectations are the source arrays mapped the way libpng does under cv::IMREAD_COLOR."""
import io
import os
import sys
import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "codecs")
os.makedirs(OUT, exist_ok=True)
rs = np.random.RandomState(7)


def scene(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 120 * np.sin(xx / 7.0 + yy / 13.0), 127 + 120 * np.cos(xx / 5.0 - yy / 9.0), (xx * 3 + yy * 5) % 256], -1)
    img += rs.randn(h, w, 3) * 12
    img[h // 3:h // 3 + 6, w // 4:w // 4 + 9] = (255, 0, 0)   # hard edges: chroma up-sampling matters
    img[h // 2:h // 2 + 5, w // 2:w // 2 + 7] = (0, 255, 255)
    return np.clip(img, 0, 255).astype(np.uint8)


def save_jpeg(name, rgb, **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", **kw)
    data = buf.getvalue()
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    open(os.path.join(OUT, name + ".jpg"), "wb").write(data)
    np.save(os.path.join(OUT, name + ".npy"), dec[:, :, ::-1].copy())  # BGR
    return data


# ---- layouts Pillow cannot write: a baseline JPEG writer (ITU T.81 Huffman sequential), `--layouts` -> tests/golden/codecs/layouts ----
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
LAYOUT_MAX_W, LAYOUT_MAX_H = 48, 40
IDCT_RANGE = 380.0   # beyond it libjpeg's range-limit table wraps and its SIMD and C IDCTs disagree


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def std_huffman():
    """{(class, id): (bits[16], values)} of the Annex K tables, read from the DHT segments of a default Pillow file"""
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG")
    d, i, tabs = buf.getvalue(), 2, {}
    while d[i + 1] != 0xDA:
        ln = int.from_bytes(d[i + 2:i + 4], "big")
        if d[i + 1] == 0xC4:
            o = i + 4
            while o < i + 2 + ln:
                bits = list(d[o + 1:o + 17])
                tabs[d[o] >> 4, d[o] & 15] = (bits, list(d[o + 17:o + 17 + sum(bits)]))
                o += 17 + sum(bits)
        i += 2 + ln
    assert sorted(tabs) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return tabs


def huff_codes(bits, vals):
    """symbol -> (code, length), T.81 C.2"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)   # byte stuffing
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)   # pad with 1-bits


def put_block(bw, blk, pred, dc, ac):
    """one block of 64 quantised coefficients (natural order): DC difference, runs, ZRL, EOB.  Returns the new predictor."""
    def value(v):
        cat = int(abs(v)).bit_length()
        return cat, (v if v >= 0 else v + (1 << cat) - 1)
    cat, extra = value(int(blk[0]) - pred)
    bw.put(*dc[cat])
    if cat:
        bw.put(extra, cat)
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        cat, extra = value(v)
        bw.put(*ac[(run << 4) | cat])
        bw.put(extra, cat)
        run = 0
    if run:
        bw.put(*ac[0x00])
    return int(blk[0])


def dqt_segment(tables, q16=False):
    """tables: {id: 64 values in natural order}"""
    p = bytearray()
    for tq, t in sorted(tables.items()):
        p.append((16 if q16 else 0) | tq)
        for k in range(64):
            p += int(t[ZIGZAG[k]]).to_bytes(2 if q16 else 1, "big")
    return segment(0xDB, p)


def write_jpeg(W, H, comps, coefs, qtabs, jfif=True, adobe=None, sof=0xC0, q16=False, separate_scans=False, dri=0, fill=0, extra=None):
    """comps: [dict(id, h, v, tq, td, ta)]; coefs[c]: (block rows, block columns, 64) quantised coefficients of the component's
    MCU-padded block grid; qtabs: {id: 64 values}; adobe: transform byte of an APP14 segment; dri: restart interval in MCUs;
    fill: FF bytes in front of every RSTn; extra: {scan index: bytes put in front of that scan's SOS}."""
    std = std_huffman()
    nc = len(comps)
    hmax, vmax = (max(c["h"] for c in comps), max(c["v"] for c in comps)) if nc > 1 else (1, 1)
    geo = [(c["h"], c["v"]) if nc > 1 else (1, 1) for c in comps]   # a single component is never interleaved
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    if adobe is not None:
        out += segment(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([adobe]))
    out += dqt_segment(qtabs, q16)
    out += segment(sof, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc]) +
                   b"".join(bytes([c["id"], (c["h"] << 4) | c["v"], c["tq"]]) for c in comps))
    used = sorted({(0, c["td"]) for c in comps} | {(1, c["ta"]) for c in comps})
    for tc, th in used:   # luma tables under id 0, chroma tables under every other id
        bits, vals = std[tc, min(th, 1)]
        out += segment(0xC4, bytes([(tc << 4) | th] + bits + vals))
    if dri:
        out += segment(0xDD, dri.to_bytes(2, "big"))
    codes = {(tc, th): huff_codes(*std[tc, min(th, 1)]) for tc, th in used}
    scans = [[i] for i in range(nc)] if separate_scans else [list(range(nc))]
    for si, members in enumerate(scans):
        out += (extra or {}).get(si, b"")
        out += segment(0xDA, bytes([len(members)]) + b"".join(bytes([comps[i]["id"], (comps[i]["td"] << 4) | comps[i]["ta"]]) for i in members) +
                       bytes([0, 63, 0]))
        if len(members) == 1:   # the component's own block raster (A.2.2), one block per MCU
            i = members[0]
            nbx, nby = -(-(-(-W * geo[i][0] // hmax)) // 8), -(-(-(-H * geo[i][1] // vmax)) // 8)
            mcus = [[(i, by, bx)] for by in range(nby) for bx in range(nbx)]
        else:
            mcus = [[(i, my * geo[i][1] + by, mx * geo[i][0] + bx) for i in members for by in range(geo[i][1]) for bx in range(geo[i][0])]
                    for my in range(mcuy) for mx in range(mcux)]
        bw, pred, rst = BitWriter(), [0] * nc, 0
        for m, blocks in enumerate(mcus):
            if dri and m and m % dri == 0:
                bw.flush()
                out += bw.out + b"\xff" * fill + bytes([0xFF, 0xD0 + rst])
                bw, pred, rst = BitWriter(), [0] * nc, (rst + 1) & 7
            for i, by, bx in blocks:
                pred[i] = put_block(bw, coefs[i][by, bx], pred[i], codes[0, comps[i]["td"]], codes[1, comps[i]["ta"]])
        bw.flush()
        out += bw.out
    return bytes(out + b"\xff\xd9")


def component_planes(rgb, comps, ycc):
    """the scene per component, box-down-sampled to the component's size and edge-padded to its MCU-padded block grid (floats, 0..255)"""
    H, W = rgb.shape[:2]
    f = rgb.astype(np.float64)
    if len(comps) == 1:
        chans, geo, hmax, vmax = [f[:, :, 1]], [(1, 1)], 1, 1
    else:
        r, g, b = f[:, :, 0], f[:, :, 1], f[:, :, 2]
        chans = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b] if ycc else [r, g, b]
        geo = [(c["h"], c["v"]) for c in comps]
        hmax, vmax = max(h for h, _ in geo), max(v for _, v in geo)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    planes = []
    for ch, (h, v) in zip(chans, geo):
        assert hmax % h == 0 and vmax % v == 0
        hs, vs = hmax // h, vmax // v
        dw, dh = -(-W * h // hmax), -(-H * v // vmax)
        p = np.pad(ch, ((0, dh * vs - H), (0, dw * hs - W)), mode="edge").reshape(dh, vs, dw, hs).mean((1, 3))
        planes.append(np.pad(p, ((0, mcuy * v * 8 - dh), (0, mcux * h * 8 - dw)), mode="edge"))
    return planes


def quantise(plane, q):
    """forward DCT (float) of every 8x8 block of the level-shifted plane, divided by the flat quantiser q"""
    nby, nbx = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = (plane - 128.0).reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)
    return np.rint(DCT @ blocks @ DCT.T / q).astype(np.int64).reshape(nby, nbx, 64)


def sparse_coefficients(shape, rnd):
    """for the large quantisers: -3..3 at DC, -1..1 at three low AC positions"""
    c = np.zeros(shape + (64,), np.int64)
    c[..., 0] = rnd.randint(-3, 4, shape)
    for k in (1, 8, 9):
        c[..., k] = rnd.randint(-1, 2, shape)
    return c


def idct_extreme(coefs, q):
    """largest magnitude of the float IDCT of the dequantised blocks, before the level shift"""
    blocks = (coefs * q).reshape(coefs.shape[:2] + (8, 8)).astype(np.float64)
    return float(np.abs(DCT.T @ blocks @ DCT).max())


def make_layouts():
    out_dir = os.path.join(OUT, "layouts")
    os.makedirs(out_dir, exist_ok=True)
    largest = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if os.path.isfile(os.path.join(OUT, f)))
    rnd = np.random.RandomState(11)
    made = []

    def store(name, data):
        im = Image.open(io.BytesIO(data))
        dec = np.asarray(im.convert("RGB"))
        assert dec.shape[1] <= LAYOUT_MAX_W and dec.shape[0] <= LAYOUT_MAX_H, (name, dec.shape)
        open(os.path.join(out_dir, name + ".jpg"), "wb").write(data)
        np.save(os.path.join(out_dir, name + ".npy"), dec[:, :, ::-1].copy())  # BGR
        for ext in (".jpg", ".npy"):
            assert os.path.getsize(os.path.join(out_dir, name + ext)) <= largest, (name, ext)
        made.append(name)

    def layout(name, w, h, factors, ids=(1, 2, 3), ycc=True, q=(6, 9, 9), tq=(0, 1, 1), tables=(0, 1, 1), qtabs=None, sparse=False, **kw):
        comps = [dict(id=ids[i], h=factors[i][0], v=factors[i][1], tq=tq[i], td=tables[i], ta=tables[i]) for i in range(len(factors))]
        planes = component_planes(scene(w, h), comps, ycc)
        coefs = [sparse_coefficients((p.shape[0] // 8, p.shape[1] // 8), rnd) if sparse else quantise(p, q[i]) for i, p in enumerate(planes)]
        extreme = max(idct_extreme(c, q[i]) for i, c in enumerate(coefs))
        assert extreme <= IDCT_RANGE, (name, extreme)
        if qtabs is None:
            qtabs = {tq[i]: [q[i]] * 64 for i in range(len(comps))}
        store(name, write_jpeg(w, h, comps, coefs, qtabs, **kw))
        return extreme

    f444, f420, f440, f42 = [(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(4, 2), (1, 1), (1, 1)]
    # sampling
    layout("l440_37x29", 37, 29, f440)
    layout("l440_2x9", 2, 9, f440)          # h1v2 is fancy at any width
    layout("l440_1x5", 1, 5, f440)
    layout("l411_37x9", 37, 9, [(4, 1), (1, 1), (1, 1)])
    layout("l42_40x20", 40, 20, f42)        # 10 blocks per MCU
    layout("l24_21x40", 21, 40, [(2, 4), (1, 1), (1, 1)])
    layout("l14_9x40", 9, 40, [(1, 4), (1, 1), (1, 1)])
    layout("l31_37x29", 37, 29, [(3, 1), (1, 1), (1, 1)])
    layout("lmixed_33x17", 33, 17, [(2, 2), (2, 1), (1, 2)])
    layout("lmixed_3x9", 3, 9, [(2, 2), (2, 1), (1, 2)])
    layout("llumaup_37x29", 37, 29, [(1, 1), (2, 2), (2, 2)])
    layout("lgray_h2v2_37x29", 37, 29, [(2, 2)], ids=(1,), q=(6,), tq=(0,), tables=(0,))
    # scans and restart intervals
    layout("l420_3scans", 37, 29, f420, separate_scans=True)
    layout("l440_3scans_dri5", 37, 29, f440, separate_scans=True, dri=5)
    layout("l420_dri1_40x24", 40, 24, f420, dri=1)
    layout("l42_dri1_40x20", 40, 20, f42, dri=1)
    layout("l420_dri2_fill", 37, 29, f420, dri=2, fill=2)
    layout("lsof1_tables3", 37, 29, f420, tq=(0, 3, 3), tables=(0, 3, 3), sof=0xC1)
    layout("lsof0_tables3", 37, 29, f420, tq=(0, 3, 3), tables=(0, 3, 3))
    # quantisers
    layout("lq16_300_260", 37, 29, f420, q=(300, 260, 260), sparse=True, q16=True)
    layout("lq8_255", 37, 29, f420, q=(255, 255, 255), sparse=True)
    layout("l3scans_requant", 37, 29, f444, q=(6, 9, 20), separate_scans=True, qtabs={0: [6] * 64, 1: [9] * 64},
           extra={2: dqt_segment({1: [20] * 64})})   # Cb latched table 1 at 9, Cr latches it at 20
    layout("lq_twice", 37, 29, f420, qtabs={0: [6] * 64, 1: [20] * 64}, extra={0: dqt_segment({1: [9] * 64})})
    # colour model: JFIF seen -> YCbCr; else the Adobe transform; else the component ids
    layout("ladobe0_rgb", 37, 29, f444, jfif=False, adobe=0, ycc=False)
    layout("ladobe1_420", 37, 29, f420, jfif=False, adobe=1)
    layout("ladobe2_ycc", 37, 29, f444, jfif=False, adobe=2)
    layout("lids_rgb", 37, 29, f444, jfif=False, ids=(ord("R"), ord("G"), ord("B")), ycc=False)
    layout("lids_012_ycc", 37, 29, f444, jfif=False, ids=(0, 1, 2))
    layout("ljfif_adobe0_ycc", 37, 29, f444, adobe=0)
    layout("ljfif_ids_rgb_ycc", 37, 29, f444, ids=(ord("R"), ord("G"), ord("B")))
    buf = io.BytesIO()
    Image.fromarray(scene(37, 29)).save(buf, "JPEG", quality=85, subsampling=0, keep_rgb=True)
    store("lkeep_rgb_q85", buf.getvalue())
    print(made, sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)), "bytes")


if "--layouts" in sys.argv[1:]:
    make_layouts()
    sys.exit(0)

a = scene(67, 45)
save_jpeg("j444_q90", a, quality=90, subsampling=0)
save_jpeg("j422_q85", a, quality=85, subsampling=1)
save_jpeg("j420_q75", a, quality=75, subsampling=2)
save_jpeg("j420_q30_opt", scene(50, 33), quality=30, subsampling=2, optimize=True)
save_jpeg("j420_rst", scene(40, 40), quality=80, subsampling=2, restart_marker_blocks=2)
save_jpeg("j420_tiny", scene(5, 3), quality=80, subsampling=2)       # down-sampled width <= 2: no fancy up-sampling
save_jpeg("j422_w3", scene(3, 9), quality=80, subsampling=1)
save_jpeg("j420_16x16", scene(16, 16), quality=95, subsampling=2)
buf = io.BytesIO(); Image.fromarray(a[:, :, 0]).save(buf, "JPEG", quality=88); d = buf.getvalue()
open(os.path.join(OUT, "jgray_q88.jpg"), "wb").write(d)
np.save(os.path.join(OUT, "jgray_q88.npy"), np.repeat(np.asarray(Image.open(io.BytesIO(d)).convert("L"))[:, :, None], 3, 2))
# progressive (SOF2): DC/AC first and refinement scans, EOB runs
save_jpeg("jprog444_q80", a, quality=80, subsampling=0, progressive=True)
save_jpeg("jprog420_q75", a, quality=75, subsampling=2, progressive=True)
save_jpeg("jprog422_q92", scene(50, 33), quality=92, subsampling=1, progressive=True)
save_jpeg("jprog420_tiny", scene(5, 3), quality=80, subsampling=2, progressive=True)
save_jpeg("jprog420_rst", scene(40, 40), quality=80, subsampling=2, progressive=True, restart_marker_blocks=3)
buf = io.BytesIO(); Image.fromarray(a[:, :, 1]).save(buf, "JPEG", quality=85, progressive=True); d = buf.getvalue()
open(os.path.join(OUT, "jproggray_q85.jpg"), "wb").write(d)
np.save(os.path.join(OUT, "jproggray_q85.npy"), np.repeat(np.asarray(Image.open(io.BytesIO(d)).convert("L"))[:, :, None], 3, 2))

# ---- PNG ----
def save_png(name, im, expect_bgr, **kw):
    im.save(os.path.join(OUT, name + ".png"), "PNG", **kw)
    np.save(os.path.join(OUT, name + ".npy"), np.ascontiguousarray(expect_bgr, np.uint8))


b = scene(37, 29)
save_png("p_rgb8", Image.fromarray(b), b[:, :, ::-1])
alpha = rs.randint(0, 256, b.shape[:2]).astype(np.uint8)
save_png("p_rgba8", Image.fromarray(np.dstack([b, alpha])), b[:, :, ::-1])              # alpha stripped, not blended
gray = b[:, :, 1]
save_png("p_gray8", Image.fromarray(gray), np.repeat(gray[:, :, None], 3, 2))
pal = Image.fromarray(b).quantize(colors=23)
save_png("p_pal8", pal, np.asarray(pal.convert("RGB"))[:, :, ::-1])
bits1 = (gray > 128)
save_png("p_gray1", Image.fromarray(bits1), np.repeat((bits1 * 255).astype(np.uint8)[:, :, None], 3, 2))
g16 = (rs.randint(0, 65536, gray.shape)).astype(np.uint16)
save_png("p_gray16", Image.fromarray(g16), np.repeat((g16 >> 8).astype(np.uint8)[:, :, None], 3, 2))   # strip_16: high byte
# interlaced RGB, written by hand (Pillow cannot): Adam7 passes through zlib
import struct, zlib
def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
c = scene(11, 9)
raw = b""
for x0, y0, dx, dy in [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]:
    sub = c[y0::dy, x0::dx]
    if sub.size == 0:
        continue
    for row in sub:
        raw += b"\x00" + row.tobytes()
png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 11, 9, 8, 2, 0, 0, 1)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")
open(os.path.join(OUT, "p_rgb8_adam7.png"), "wb").write(png)
np.save(os.path.join(OUT, "p_rgb8_adam7.npy"), c[:, :, ::-1].copy())
# ---- JPEG encoder: source pixels (BGR) + the bytes Pillow/libjpeg-turbo writes (= cv::imwrite's defaults: 4:2:0, std tables)
for w, h, q in [(67, 45, 98), (33, 17, 98), (16, 16, 75), (1, 1, 98), (8, 24, 50), (17, 33, 30), (40, 9, 98)]:
    s = scene(w, h)
    buf = io.BytesIO()
    Image.fromarray(s).save(buf, "JPEG", quality=q)
    np.save(os.path.join(OUT, f"enc_{w}x{h}_q{q}.npy"), s[:, :, ::-1].copy())
    open(os.path.join(OUT, f"enc_{w}x{h}_q{q}.jpgref"), "wb").write(buf.getvalue())
print(sorted(os.listdir(OUT)), sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)), "bytes")
