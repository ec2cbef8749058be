"""Bitwise comparison of the blobs a batch left behind with the blobs of its frames tapped alone — TEST INFRASTRUCTURE (numpy only).

The identity is derived, not measured: a batch and a one-frame tap run the same plan and the same kernel instantiations, an output element's
K order depends only on its tile coordinates inside its image, and nothing in the kernels reads gridDim except the block decode.  So frame j's
images in a batch blob ([j * N, (j + 1) * N) of nframes * N) hold the bits that frame's own forward leaves in images [0, N)."""
import numpy as np


class Diff:
    """the first differing element of a blob (in memory order of the batch blob) and how many differ"""
    def __init__(self, blob, frame, image, channel, y, x, got, want, count):
        self.blob, self.frame, self.image, self.channel, self.y, self.x, self.got, self.want, self.count = blob, frame, image, channel, y, x, got, want, count

    def __str__(self):
        return (f"{self.blob}: {self.count} elements differ, first in frame {self.frame} image {self.image} channel {self.channel} "
                f"pixel (y {self.y}, x {self.x}): got {self.got!r} want {self.want!r}")


def _differs(got, want):
    """elements np.array_equal would count as different (NaN included), and those equal as numbers with other bits (-0.0 / 0.0)"""
    return ~(got == want) | (got.view(np.uint32) != want.view(np.uint32))


def compare_blob(name, batch, singles, N):
    """batch: [nframes * N][C][H][W] float32; singles: nframes arrays [N][C][H][W], frame j's blob tapped alone.  None where every bit agrees, else a Diff."""
    batch = np.ascontiguousarray(batch, np.float32)
    assert batch.ndim == 4 and batch.shape[0] == N * len(singles), (name, batch.shape, N, len(singles))
    first, count = None, 0
    for j, want in enumerate(singles):
        want = np.ascontiguousarray(want, np.float32)
        got = batch[j * N:(j + 1) * N]
        assert got.shape == want.shape, (name, j, got.shape, want.shape)
        bad = _differs(got, want)
        n = int(bad.sum())
        if n and first is None:
            i, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
            first = (j, j * N + i, c, y, x, float(got[i, c, y, x]), float(want[i, c, y, x]))
        count += n
    return None if first is None else Diff(name, *first, count)


def compare_batch(blobs, singles, N):
    """blobs: name -> batch blob; singles: one dict name -> blob per frame of the batch, in slot order.  -> ([Diff], {blob name: differing elements})"""
    diffs, counts = [], {}
    for name, b in blobs.items():
        d = compare_blob(name, b, [s[name] for s in singles], N)
        counts[name] = d.count if d else 0
        if d:
            diffs.append(d)
    return diffs, counts
