"""Affine views of resident tensors (cofhe_amd/csrc/view.hpp): a Python reference by explicit loops over coordinates, descriptor
builders that mirror the C ones, and the case list that the CPU tier (tests/test_view_cpu.py) and the GPU tier
(tests/test_gpu_view.py) share.

A view produces a box of out_extent elements from a dense row-major source of src_extent: for the output coordinate o the source
coordinate on source axis a is c_a = start[a] + sum_d map[a][d] o_d.  Where every c_a lies in its axis, destination element
rowmajor(dst_extent, dst_start + o) is source element rowmajor(src_extent, c); otherwise it is the fill.  The destination outside
the box is left alone."""
import random

MAX_DIMS = 8
GATHER_FILL = 0xFFFFFFFF
GATHER_KEEP = 0xFFFFFFFE


class View:
    def __init__(self, out_extent, src_extent, start, map_, dst_extent=None, dst_start=None):
        self.out_extent = list(out_extent)
        self.src_extent = list(src_extent)
        self.start = list(start)
        self.map = [list(r) for r in map_]                 # [source axis][output axis]
        self.dst_extent = list(dst_extent) if dst_extent is not None else list(out_extent)
        self.dst_start = list(dst_start) if dst_start is not None else [0] * len(self.out_extent)
        assert len(self.start) == len(self.src_extent) == len(self.map)
        assert all(len(r) == len(self.out_extent) for r in self.map)
        assert len(self.dst_extent) == len(self.dst_start) == len(self.out_extent)


def count(extent):
    n = 1
    for e in extent:
        n *= e
    return n


def rowmajor(extent, coord):
    lin = 0
    for e, c in zip(extent, coord):
        lin = lin * e + c
    return lin


def coordinates(extent):
    """every coordinate of a box, the last axis fastest: an odometer, no library"""
    if count(extent) == 0:
        return
    o = [0] * len(extent)
    while True:
        yield list(o)
        d = len(extent) - 1
        while d >= 0:
            o[d] += 1
            if o[d] < extent[d]:
                break
            o[d] = 0
            d -= 1
        if d < 0:
            return


def indices(view):
    """for every element of the box in row-major order: (source index or -1 for the fill, destination index)"""
    out = []
    for o in coordinates(view.out_extent):
        c = []
        for a in range(len(view.src_extent)):
            v = view.start[a]
            for d in range(len(o)):
                v += view.map[a][d] * o[d]
            c.append(v)
        inside = all(0 <= c[a] < view.src_extent[a] for a in range(len(c)))
        dst = rowmajor(view.dst_extent, [view.dst_start[d] + o[d] for d in range(len(o))])
        out.append((rowmajor(view.src_extent, c) if inside else -1, dst))
    return out


def apply(view, src_rows, fill_row, dst_rows):
    """writes the box into dst_rows (a list, changed in place and returned); everything else in it stays"""
    assert len(src_rows) == count(view.src_extent) and len(dst_rows) == count(view.dst_extent)
    for s, d in indices(view):
        dst_rows[d] = src_rows[s] if s >= 0 else fill_row
    return dst_rows


def needs_fill(view):
    return any(s < 0 for s, _ in indices(view))


def to_c(v):
    """the C descriptor (cofhe_amd.engine.View) of a View"""
    from cofhe_amd.engine import View as CView
    c = CView()
    c.out_ndim, c.src_ndim = len(v.out_extent), len(v.src_extent)
    for d, e in enumerate(v.out_extent):
        c.out_extent[d], c.dst_extent[d], c.dst_start[d] = e, v.dst_extent[d], v.dst_start[d]
    for a, e in enumerate(v.src_extent):
        c.src_extent[a], c.start[a] = e, v.start[a]
        for d in range(len(v.out_extent)):
            c.map[a][d] = v.map[a][d]
    return c


# ---- the builders, mirroring cofhe_hip_view_permute and kin ----
def _diag(n, entries):
    m = [[0] * n for _ in range(n)]
    for a, v in enumerate(entries):
        m[a][a] = v
    return m


def permute(shape, perm):
    n = len(shape)
    m = [[0] * n for _ in range(n)]
    for d, a in enumerate(perm):
        m[a][d] = 1
    return View([shape[a] for a in perm], shape, [0] * n, m)


def slice_(shape, start, stop, step):
    """bounds in range; with a negative step a stop of -1 means down to and including element 0"""
    out = []
    for a, b, s in zip(start, stop, step):
        span = max(b - a, 0) if s > 0 else max(a - b, 0)
        out.append((span + abs(s) - 1) // abs(s))
    return View(out, shape, start, _diag(len(shape), step))


def flip(shape, axis):
    n = len(shape)
    return View(shape, shape, [shape[a] - 1 if a == axis else 0 for a in range(n)], _diag(n, [-1 if a == axis else 1 for a in range(n)]))


def pad(shape, lo, hi):
    n = len(shape)
    return View([l + s + h for l, s, h in zip(lo, shape, hi)], shape, [-l for l in lo], _diag(n, [1] * n))


def broadcast(shape, out_shape):
    n, m = len(shape), len(out_shape)
    mp = [[0] * m for _ in range(n)]
    for a in range(n):
        d = m - n + a
        assert shape[a] in (1, out_shape[d])
        if shape[a] == out_shape[d]:
            mp[a][d] = 1
    return View(out_shape, shape, [0] * n, mp)


def window_taps(B, H, W, C, kh, kw, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1):
    Ho = (H + 2 * ph - ((kh - 1) * dh + 1)) // sh + 1
    Wo = (W + 2 * pw - ((kw - 1) * dw + 1)) // sw + 1
    mp = [[0] * 6 for _ in range(4)]
    mp[0][2] = 1
    mp[1][0], mp[1][3] = dh, sh
    mp[2][1], mp[2][4] = dw, sw
    mp[3][5] = 1
    return View([kh, kw, B, Ho, Wo, C], [B, H, W, C], [0, -ph, -pw, 0], mp)


def into(view, dst_shape, dst_start):
    return View(view.out_extent, view.src_extent, view.start, view.map, dst_shape, dst_start)


def identity(shape):
    return permute(shape, list(range(len(shape))))


def _eight_axes():
    rng = random.Random(20260)
    mp = [[rng.choice((-1, 0, 1, 2)) for _ in range(8)] for _ in range(8)]
    return View([2] * 8, [2] * 8, [rng.randint(-1, 1) for _ in range(8)], mp)


# (name, [views]): the views of a case write into ONE destination, each from a source of its own
CASES = [
    ("identity", [identity([7])]),
    ("transpose", [permute([3, 5], [1, 0])]),
    ("permute", [permute([2, 3, 4, 5], [3, 1, 0, 2])]),
    ("slice_forward", [slice_([7], [1], [6], [2])]),
    ("slice_backward", [slice_([7], [5], [0], [-2])]),
    ("slice_inner", [slice_([3, 4, 5], [0, 1, 0], [3, 4, 5], [1, 2, 1])]),
    ("flip", [flip([3, 4], 1)]),
    ("broadcast_row", [broadcast([3], [4, 3])]),
    ("broadcast_middle", [broadcast([2, 1, 3], [2, 5, 3])]),
    ("pad", [pad([3, 4], [1, 2], [1, 1])]),
    ("diagonal", [View([4], [4, 4], [0, 0], [[1], [1]])]),
    ("window_taps", [window_taps(1, 5, 4, 2, 3, 2, sh=2, sw=1, ph=1, pw=1, dh=2, dw=1)]),
    ("eight_axes", [_eight_axes()]),
    ("dst_box", [into(identity([2, 2]), [2, 5], [0, 0]), into(identity([2, 3]), [2, 5], [0, 2])]),
    ("empty", [View([3, 0], [3, 4], [0, 0], [[1, 0], [0, 1]])]),
    ("all_fill", [View([4], [3], [5], [[1]])]),
    ("scalar", [View([], [], [], [])]),
]
CASE_IDS = [name for name, _ in CASES]


def gather(src_rows, index, fill_row, dst_rows):
    """dst[i] = src[index[i]]; FILL gives the fill, KEEP leaves dst[i]; another index beyond the source gives the fill (or, with no
    fill, leaves dst[i]) and is reported: returns (dst_rows, bad)"""
    bad = False
    for i, ix in enumerate(index):
        if ix == GATHER_KEEP:
            continue
        if ix < len(src_rows):
            dst_rows[i] = src_rows[ix]
            continue
        if ix != GATHER_FILL:
            bad = True
        if fill_row is not None:
            dst_rows[i] = fill_row
    return dst_rows, bad
