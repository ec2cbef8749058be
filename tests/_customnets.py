"""Deploy graphs other than the built-in one, generated in Python — TEST INFRASTRUCTURE for the per-launch convolution check.

plan.cpp walk_graph accepts any deploy prototxt made of stride-1 "same" convolutions (k in {1, 3, 7}), 2x2 max poolings, channel concats of
convolution outputs and ImResize + Nms at the end.  The graphs here are made up for the shape-dependent branches of the planner and of the
epilogues that the built-in graph never takes (tests/test_conv_launches_cpu.py lists them and asserts that each is reached); the text they
emit has the syntax of netdef.cpp emit_prototxt, which _convcheck.Graph parses.  Weights are the engine's synthetic ones (seeded by layer name).

Also here: the concat slice offsets of plan.cpp make_tensors, restated (concat_offsets)."""
import atexit
import os
import shutil
import tempfile
from collections import OrderedDict

import _convcheck as cc


class Net:
    def __init__(self, name):
        self.name, self.layers, self.channels, self.parts = name, [], {"image": 3}, None

    def _layer(self, name, typ, bottoms, tops, body=""):
        self.layers.append('layer {\n  name: "%s"\n  type: "%s"\n' % (name, typ) + "".join('  bottom: "%s"\n' % b for b in bottoms) +
                           "".join('  top: "%s"\n' % t for t in tops) + body + "}\n")

    def conv(self, name, bottom, cout, k, relu=True):
        self._layer(name, "Convolution", [bottom], [name], "  convolution_param {\n    num_output: %d\n    pad: %d\n    kernel_size: %d\n  }\n" % (cout, k // 2, k))
        if relu:
            self._layer("relu_" + name, "ReLU", [name], [name])
        self.channels[name] = cout
        return name

    def pool(self, name, bottom):
        self._layer(name, "Pooling", [bottom], [name], "  pooling_param {\n    pool: MAX\n    kernel_size: 2\n    stride: 2\n  }\n")
        self.channels[name] = self.channels[bottom]
        return name

    def concat(self, name, bottoms):
        self._layer(name, "Concat", bottoms, [name], "  concat_param {\n    axis: 1\n  }\n")
        self.channels[name] = sum(self.channels[b] for b in bottoms)
        return name

    def tail(self, bottom):
        """ImResize + Nms; 57 channels make a COCO-shaped graph (num_parts 18), 44 an MPI-shaped one (15)"""
        self.parts = {57: 18, 44: 15}[self.channels[bottom]]
        self._layer("resized_map", "ImResize", [bottom], ["resized_map"], "  imresize_param {\n    factor: 8\n    scale_gap: 0.3\n    start_scale: 1\n  }\n")
        self._layer("joints", "Nms", ["resized_map"], ["joints"], "  nms_param {\n    threshold: 0.05\n    max_peaks: 64\n    num_parts: %d\n  }\n" % self.parts)
        return self

    def text(self):
        return 'name: "%s"\ninput: "image"\ninput_dim: 1\ninput_dim: 3\ninput_dim: 1\ninput_dim: 1\n' % self.name + "".join(self.layers)


def odd():
    """Channel counts that are no multiple of anything: a first layer off the direct route, a pooling epilogue on 40 channels, a 7x7 layer at 1/4
    resolution with a stand-alone pooling step behind it, a concat whose last slice starts at channel 147, 7x7 pairs with 130 outputs, 1x1 layers on the
    register-staged kernel (300 outputs into a 320-channel tensor), a 1x1 pair of 38 + 19 channels that writes the low-res maps, and `f`, read by 3x3
    layers and by a 1x1 layer that cannot fuse: its tensor carries a lo AND a q block under mixed @all.  So does `b1`, through its second reader `b1k3`,
    while `b2` carries a lo block only: d1 and d2 read tensors of different pixel pitch."""
    n = Net("odd")
    n.conv("c1", "image", 24, 3); n.conv("c1b", "c1", 40, 3); n.pool("p1", "c1b")
    n.conv("c2", "p1", 72, 3); n.conv("c2k1", "c2", 100, 1); n.pool("p2", "c2k1")
    n.conv("c3", "p2", 200, 3); n.conv("c3k7", "c3", 48, 7); n.pool("p3", "c3k7")
    n.conv("f", "p3", 128, 3)
    n.conv("fk1", "f", 24, 1)
    n.conv("a1", "f", 19, 3); n.conv("a2", "f", 45, 3)
    n.concat("cat1", ["a1", "a2", "f"])
    n.conv("b1", "cat1", 130, 7); n.conv("b2", "cat1", 130, 7)
    n.conv("b1k3", "b1", 16, 3)
    n.conv("d1", "b1", 300, 1); n.conv("d2", "b2", 300, 1)
    n.conv("e1", "d1", 38, 1, relu=False); n.conv("e2", "d2", 19, 1, relu=False)
    n.concat("low", ["e2", "e1"])
    return n.tail("low")


def single():
    """Wide layers and one convolution as the tail: a 3x3 ring convolution writes the 57 low-res maps itself; 3x3 and 7x7 on 320 channels; `c1b` has
    a second reader, so its pooling cannot fuse; a concat of 20 + 68 + 40 channels whose 68-channel slice starts at channel 60: on a 4-byte but on
    no 8-channel boundary, its first 16-channel chunk crossing the 64-channel group boundary of the q block."""
    n = Net("single")
    n.conv("c1", "image", 64, 3); n.conv("c1b", "c1", 64, 3); n.pool("p1", "c1b")
    n.conv("side", "c1b", 16, 3)
    n.conv("c2", "p1", 128, 3); n.pool("p2", "c2")
    n.conv("c3", "p2", 320, 3); n.pool("p3", "c3")
    n.conv("g", "p3", 320, 7)
    n.conv("s", "g", 20, 3); n.conv("t", "g", 68, 3); n.conv("u", "g", 40, 3)
    n.concat("cat2", ["s", "t", "u"])
    n.conv("low", "cat2", 57, 3, relu=False)
    return n.tail("low")


def pw():
    """An MPI-shaped graph (44 maps) with fusable 1x1 chains of middle width 256 (single) and 384 (paired), 7x7 layers at full and at half resolution
    (halo 3 at levels 0 and 1, stand-alone pooling steps that read them) and 7x7 on 224 and 256 channels."""
    n = Net("pw")
    n.conv("c1", "image", 64, 3); n.conv("c1k7", "c1", 32, 7); n.pool("p1", "c1k7")
    n.conv("c2", "p1", 128, 7); n.pool("p2", "c2")
    n.conv("c3", "p2", 224, 3); n.conv("c3k7", "c3", 256, 7); n.pool("p3", "c3k7")
    n.conv("h0", "p3", 128, 7)
    n.conv("z1", "h0", 256, 1); n.conv("z2", "z1", 64, 1)
    n.conv("h", "z2", 128, 3)
    n.conv("x1", "h", 384, 1); n.conv("x2", "h", 384, 1)
    n.conv("y1", "x1", 16, 1, relu=False); n.conv("y2", "x2", 28, 1, relu=False)
    n.concat("low", ["y2", "y1"])
    return n.tail("low")


NETS = OrderedDict([("odd", odd), ("single", single), ("pw", pw)])
_cache = {}


def net(name):
    """(prototxt text, _convcheck.Graph, num_parts) of a graph"""
    if name not in _cache:
        n = NETS[name]()
        _cache[name] = (n.text(), cc.Graph(n.text()), n.parts)
    return _cache[name]


def concat_offsets(graph, top, elem=2):
    """[(input, channel offset inside the concat's tensor)] as plan.cpp make_tensors lays them out: inputs whose size is a multiple of 8 first (a stable
    sort), then packed — or every slice on an 8-channel boundary where that needs no larger padded tensor (Cp: a multiple of 128 bytes)."""
    calign = 128 // elem
    up = lambda v, a: (v + a - 1) // a * a
    ins = graph.concats[top]
    order = sorted(range(len(ins)), key=lambda i: graph.channels[ins[i]] % 8 != 0)
    packed, aligned, off, a = {}, {}, 0, 0
    for i in order:
        packed[i] = off
        off += graph.channels[ins[i]]
        a = up(a, 8)
        aligned[i] = a
        a += graph.channels[ins[i]]
    use = aligned if up(a, calign) == up(off, calign) else packed
    return [(ins[i], use[i]) for i in range(len(ins))]


_dir = []


def proto_file(name):
    """path of the graph's prototxt, written once per process into a directory that goes away at exit"""
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix="customnets_"))
        atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
    path = os.path.join(_dir[0], name + ".prototxt")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(net(name)[0])
    return path


def config(name, mode, W, H, num_scales=1, batch_frames=1, proto_path=None):
    """engine configuration of a custom case: mixed splits every layer (`@all`), so that every tensor carries the blocks its consumers' kernels read"""
    import caffe_rtpose_amd as r
    proto_path = proto_path or proto_file(name)
    prec = {"fp16": r.PREC_FP16, "fp32": r.PREC_FP32, "mixed": r.PREC_MIXED, "f16x3": r.PREC_F16X3}[mode]
    kw = dict(split_layers="@all") if mode == "mixed" else {}
    return r.Config(proto_path=proto_path, net_w=W, net_h=H, num_scales=num_scales, scale_gap=0.3, precision=prec, frames_in_flight=batch_frames,
                    batch_frames=batch_frames, **kw)


# the configurations of tests/test_conv_launches.py for these graphs: (graph, mode, W, H, num_scales, batch_frames).  256x64 has W >= 128 at full
# resolution (the pooling epilogue) and several tiles per image, 64x48 a whole 1/8 image inside one tile, 64x256 several row wraps per tile;
# tests/test_conv_launches_cpu.py asserts what the set reaches.
CUSTOM_MATRIX = [
    ("odd", "fp16", 256, 64, 1, 1),
    ("odd", "f16x3", 256, 64, 1, 1),
    ("odd", "fp32", 64, 48, 1, 1),
    ("single", "mixed", 64, 256, 1, 1),     # portrait
    ("single", "f16x3", 256, 64, 1, 1),
    ("single", "fp32", 64, 48, 1, 1),
    ("pw", "mixed", 64, 48, 1, 1),
    ("pw", "mixed", 256, 64, 1, 1),
    ("pw", "fp16", 256, 64, 1, 1),
    ("pw", "f16x3", 256, 64, 1, 1),
    ("pw", "fp32", 256, 64, 1, 1),
    ("odd", "mixed", 256, 64, 2, 2),        # tiles chosen for four images per launch
]


def case_id(case):
    g, mode, W, H, N, B = case
    return f"{g}_{mode}_{W}x{H}" + (f"_{N}s" if N > 1 else "") + (f"_b{B}" if B > 1 else "")
