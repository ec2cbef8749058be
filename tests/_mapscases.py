"""Inputs and numpy references of the maps-mode tests (tests/test_maps_out_cpu.py, tests/test_maps_out.py).

Nothing here calls the code under test.  The narrow formats are restated in numpy, every step in float32:
  confidence / background (channel <= num_parts):  clip(rint(float32(v) * float32(255)), 0, 255)
  PAF (channel > num_parts):                       clip(rint((float32(v) + float32(1)) * float32(127.5)), 0, 255)
  NaN -> 0, ties to even (np.rint), f16 = astype(np.float16) (round to nearest even)."""
import numpy as np

NET_W, NET_H = 160, 96
DISP_W, DISP_H = 320, 180
COCO_PARTS, COCO_CHANNELS = 18, 57

# (num_scales, start_scale, scale_gap): one scale; three scales from the full size; two scales whose FIRST level is cropped
GEOMETRIES = {"1": (1, 1.0, 0.3), "3": (3, 1.0, 0.25), "2crop": (2, 0.8, 0.2)}

# output channel lists: all, one PAF channel, a permuted subset across the parts / PAF boundary (18 = background, 19.. = PAFs), a repeat
CHANNEL_LISTS = {
    "all": None,
    "one_paf": [40],
    "permuted_across_boundary": [56, 3, 19, 18, 0, 17, 20],
    "repeat": [5, 30, 5, 5],
}


def u8_ref(v, is_paf):
    """numpy restatement of the u8 format for one array"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v + np.float32(1)) * np.float32(127.5) if is_paf else v * np.float32(255)
        assert s.dtype == np.float32
        q = np.clip(np.rint(s), 0, 255)
    q = np.where(np.isnan(q), np.float32(0), q)
    return q.astype(np.uint8)


def u8_ref_planes(maps, channels, num_parts):
    """maps: [..., nch, H, W] float32 whose plane k holds channel channels[k]"""
    out = np.empty(maps.shape, np.uint8)
    for k, c in enumerate(channels):
        out[..., k, :, :] = u8_ref(maps[..., k, :, :], c > num_parts)
    return out


def f16_ref(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float32).astype(np.float16)


def same_f32(a, b):
    """bit for bit, except that a NaN only has to be a NaN (the payload of an invalid operation is the machine's)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def same_f16(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float16 and b.dtype == np.float16
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb]))


def u8_tie_values(is_paf):
    """around every tie of the u8 quantiser, (k + 0.5) / 255 resp. its PAF counterpart: the float32 quotient and its three
    neighbours on either side (u8_exact_ties picks those whose scaled value IS k + 0.5 in float32)"""
    out = []
    for k in range(-2, 257):
        t = np.float32(k + 0.5)
        x = np.float32(t / np.float32(127.5) - np.float32(1)) if is_paf else np.float32(t / np.float32(255))
        cand = [x]
        for _ in range(3):
            cand = [np.nextafter(cand[0], np.float32(-np.inf), dtype=np.float32)] + cand + [np.nextafter(cand[-1], np.float32(np.inf), dtype=np.float32)]
        out.extend(cand)
    return np.array(out, np.float32)


def u8_exact_ties(is_paf):
    """the values of u8_tie_values whose scaled value is exactly k + 0.5 in float32 arithmetic"""
    t = u8_tie_values(is_paf)
    with np.errstate(invalid="ignore"):
        s = (t + np.float32(1)) * np.float32(127.5) if is_paf else t * np.float32(255)
    return t[(s - np.floor(s)) == np.float32(0.5)]


def quantiser_grid(is_paf):
    """ties, values below 0 and above 1, +-inf, denormals, NaN"""
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.1754944e-38, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, -np.nan,
                        0.5, -0.5, 0.25, 1.5, -1.5, 0.999999, 1.000001, 1 / 255, 1 / 510, 254.5 / 255, 255.5 / 255], np.float32)
    rng = np.random.default_rng(11)
    noise = rng.uniform(-1.6, 1.6, 4096).astype(np.float32)
    return np.concatenate([u8_tie_values(is_paf), special, noise])


def f16_grid():
    """every binade boundary of binary16 (and of the denormal range) with its float32 neighbours, every kind of tie between two
    adjacent binary16 values (even and odd lower neighbour), overflow ties, denormals of float32, +-inf, NaN"""
    vals = []
    for e in range(-26, 18):
        b = np.float32(2.0) ** np.float32(e)
        vals += [np.nextafter(b, np.float32(0), dtype=np.float32), b, np.nextafter(b, np.float32(np.inf), dtype=np.float32)]
    h = np.arange(0, 0x7c00, 37, dtype=np.uint16)                       # a spread of binary16 values incl. denormals ...
    h = np.concatenate([h, np.arange(0, 16, dtype=np.uint16), np.arange(0x3fe, 0x404, dtype=np.uint16), np.arange(0x7bf8, 0x7c00, dtype=np.uint16)])
    lo = h.view(np.float16).astype(np.float32)
    hi = (h + 1).astype(np.uint16).view(np.float16).astype(np.float32)  # (0x7c00 = inf above the largest: the overflow tie 65520)
    hi = np.where(np.isinf(hi), np.float32(65536), hi)
    mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2).astype(np.float32)   # exact in float32: 11 + 1 mantissa bits
    for m in mid:
        vals += [np.nextafter(m, np.float32(0), dtype=np.float32), m, np.nextafter(m, np.float32(np.inf), dtype=np.float32)]
    vals += [0.0, 1e-45, 1e-40, 1.1754944e-38, 65504.0, 65519.996, 65520.0, 65536.0, 1e6, 3.4e38, np.inf, np.nan]
    v = np.array(vals, np.float32)
    rng = np.random.default_rng(12)
    v = np.concatenate([v, rng.uniform(-2, 2, 2048).astype(np.float32), (rng.uniform(-1, 1, 512) * 1e-6).astype(np.float32)])
    return np.concatenate([v, -v])


def planted_lowres(num, C, h, w, num_parts=COCO_PARTS, seed=7):
    """[num][C][h][w]: seeded noise of about [-1.5, 1.5] (both u8 clamps and the PAF offset are reached); part 1 and PAF channel
    num_parts + 2 of scale 0 hold exact quantiser ties of their kind; one NaN and one inf"""
    rng = np.random.default_rng(seed + 131 * num + 7 * h)
    x = rng.uniform(-1.5, 1.5, (num, C, h, w)).astype(np.float32)
    for c, paf in ((1, False), (num_parts + 2, True)):
        t = u8_exact_ties(paf)
        x[0, c] = np.resize(t[np.linspace(0, len(t) - 1, min(len(t), h * w)).astype(int)], h * w).reshape(h, w)
    x[0, 2, h // 2, w // 3] = np.nan
    x[num - 1, num_parts + 5, 1, w - 2] = np.inf
    return x


def channels_of(name, C=COCO_CHANNELS):
    ch = CHANNEL_LISTS[name]
    return list(range(C)) if ch is None else list(ch)


def read_pgm(path):
    """a binary P5 file with maxval 255 -> (h, w) u8 array; the header must be exactly 'P5\\nW H\\n255\\n'"""
    data = open(path, "rb").read()
    assert data[:3] == b"P5\n", data[:16]
    end = data.index(b"\n", 3)
    w, h = (int(t) for t in data[3:end].split())
    assert data[end + 1:end + 5] == b"255\n", data[:32]
    body = data[end + 5:]
    assert len(body) == w * h, (len(body), w, h)
    return np.frombuffer(body, np.uint8).reshape(h, w)
