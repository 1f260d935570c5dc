"""The permutation between a P1 function of level L + 1 and a P2 function of level L on one macro-cell, restated in numpy for
the tests of the P1 <-> P2 conversion kernels.

Written from the parity rule and the array layouts documented in include/hyteg_hip.h alone: the point ( X, Y, Z ) of the fine
vertex array is the P2 DoF with logical index ( X // 2, Y // 2, Z // 2 ) of the kind its parities select; vertex arrays are
tetrahedral arrays of width 2^level + 1 (x fastest, then y, then z), the edge array is seven such blocks X, Y, Z, XY, XZ, YZ of
width 2^level and XYZ of width 2^level - 1.  tests/test_p1p2_conversion_map.py pins every piece against oracle.p1_oracle."""
import functools

import numpy as np

# kind (0 vertex, 1..7 X, Y, Z, XY, XZ, YZ, XYZ) by parity pattern px + 2 py + 4 pz
KIND_OF_PARITY = np.array([0, 1, 2, 4, 3, 5, 6, 7])


def tet(w):
    return w * (w + 1) * (w + 2) // 6


def tet_index(w, x, y, z):
    """index of ( x, y, z ) in a tetrahedral array of width w (vectorised)"""
    return tet(w) - tet(w - z) + y * (w - z) - y * (y - 1) // 2 + x


@functools.lru_cache(maxsize=None)
def vertex_coords(level):
    """( size, 3 ) logical coordinates of the entries of a vertex array in memory order (read-only)"""
    n = (1 << level) + 1
    z, y, x = np.indices((n, n, n), dtype=np.int32)
    keep = x + y + z <= n - 1
    out = np.stack([x[keep], y[keep], z[keep]], axis=1).astype(np.int64)  # C order of the boolean index: z, then y, then x
    out.setflags(write=False)
    return out


def class_from_flags(f0, f1, f2, f3):
    """slot 0..13 of the macro-primitive (edge0..5, face0..3, vertex0..3) from the four face flags z == 0, y == 0, x == 0,
    x + y + z == N - 1; 14 inside the cell (the order of src/hyteg/indexing/MacroCellIndexing.cpp:36-91)"""
    f0, f1, f2, f3 = (np.asarray(f, dtype=bool) for f in (f0, f1, f2, f3))
    cnt = f0.astype(int) + f1 + f2 + f3
    cls = np.full(cnt.shape, 14, dtype=np.int64)
    one = cnt == 1
    cls[one] = (6 + np.select([f0, f1, f2], [0, 1, 2], 3))[one]
    two = cnt == 2
    edge = np.select([f0 & f1, f0 & f2, f0 & f3, f1 & f2, f1 & f3], [0, 1, 2, 3, 4], 5)
    cls[two] = edge[two]
    three = cnt >= 3
    vert = np.select([f0 & f1 & f2, f0 & f1 & f3, f0 & f2 & f3], [10, 11, 12], 13)
    cls[three] = vert[three]
    return cls


@functools.lru_cache(maxsize=None)
def point_classes(level):
    """point class of every entry of a vertex array of `level` (read-only)"""
    c, n = vertex_coords(level), (1 << level) + 1
    out = class_from_flags(c[:, 2] == 0, c[:, 1] == 0, c[:, 0] == 0, c.sum(axis=1) == n - 1)
    out.setflags(write=False)
    return out


def sizes(p2_level):
    """( entries of the P2 vertex array, of the P2 edge array, of the P1 array of level p2_level + 1 )"""
    n = 1 << p2_level
    return tet(n + 1), 6 * tet(n) + tet(n - 1), tet(2 * n + 1)


@functools.lru_cache(maxsize=None)
def p1_to_p2_map(p2_level):
    """For every entry of the P1 array of level p2_level + 1, in memory order: ( kind, index ) -- kind 0: index into the P2 vertex
    array; kind 1..7: index into the P2 edge array -- and `target`, the index into the concatenation [ vertex array | edge array ]."""
    n = 1 << p2_level
    c = vertex_coords(p2_level + 1)
    kind = KIND_OF_PARITY[(c[:, 0] & 1) + 2 * (c[:, 1] & 1) + 4 * (c[:, 2] & 1)]
    x, y, z = c[:, 0] >> 1, c[:, 1] >> 1, c[:, 2] >> 1
    width = np.where(kind == 0, n + 1, np.where(kind == 7, n - 1, n))
    index = tet_index(width, x, y, z) + np.where(kind == 0, 0, (kind - 1) * tet(n))
    target = index + np.where(kind == 0, 0, tet(n + 1))
    for a in (kind, index, target):
        a.setflags(write=False)
    return kind, index, target


def selected(p2_level, mask):
    """per entry of the P1 array of level p2_level + 1: is its point class in the 15-bit mask?"""
    return ((int(mask) >> point_classes(p2_level + 1)) & 1).astype(bool)


def p1_to_p2_expected(p1, p2_vertex, p2_edge, p2_level, mask):
    """the P2 arrays after P1toP2Conversion with `mask`: selected DoFs take the P1 value, the others keep theirs"""
    _, _, target = p1_to_p2_map(p2_level)
    s = selected(p2_level, mask)
    cat = np.concatenate([p2_vertex, p2_edge])
    cat[target[s]] = p1[s]
    return cat[:p2_vertex.size], cat[p2_vertex.size:]


def p2_to_p1_expected(p1, p2_vertex, p2_edge, p2_level, mask):
    """the P1 array after P2toP1Conversion with `mask`"""
    _, _, target = p1_to_p2_map(p2_level)
    s = selected(p2_level, mask)
    out = p1.copy()
    out[s] = np.concatenate([p2_vertex, p2_edge])[target[s]]
    return out
