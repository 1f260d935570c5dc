"""CPU-only: the permutation behind P1toP2Conversion / P2toP1Conversion (tests/conversionutil.py) against the oracle's indexing,
and the argument checks of the four C-ABI entry points, which must reject bad calls before any GPU work."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import conversionutil as cu  # noqa: E402

ENTRIES = ("hyteg_hip_p1_to_p2_cells", "hyteg_hip_p2_to_p1_cells", "hyteg_hip_p1_to_p2_cell", "hyteg_hip_p2_to_p1_cell")
P2_MAX_LEVEL = 9  # HYTEG_HIP_P2_MAX_LEVEL
# X, Y, Z, XY, XZ, YZ, XYZ: the sum of the two end-point offsets of an edge DoF, i.e. twice its midpoint's offset
EDGE_END_SUMS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_map_is_pinned_to_the_oracle_indexing(level):
    """entry by entry: the image of the fine point ( X, Y, Z ) is oracle.cell_index / edge_index of the DoF whose position is that
    point, and the helper layouts are the oracle's"""
    from oracle import p1_oracle as po

    nv, ne, nf = cu.sizes(level)
    assert (nv, ne, nf) == (po.cell_size(level), po.edge_array_size(level), po.cell_size(level + 1))
    assert np.array_equal(cu.vertex_coords(level + 1), po.cell_coords(level + 1))
    assert np.array_equal(cu.point_classes(level + 1), po.slot_of_points(level + 1))
    kind, index, target = cu.p1_to_p2_map(level)
    for i, (X, Y, Z) in enumerate(cu.vertex_coords(level + 1)):
        X, Y, Z = int(X), int(Y), int(Z)
        if kind[i] == 0:
            assert (X % 2, Y % 2, Z % 2) == (0, 0, 0)
            assert index[i] == po.cell_index(level, X // 2, Y // 2, Z // 2) and target[i] == index[i]
        else:
            o = int(kind[i]) - 1
            assert (X % 2, Y % 2, Z % 2) == EDGE_END_SUMS[o]
            assert index[i] == po.edge_index(level, X // 2, Y // 2, Z // 2, o) and target[i] == nv + index[i]


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5])
def test_map_is_a_bijection_that_preserves_the_point_class(level):
    from oracle import p1_oracle as po

    nv, ne, nf = cu.sizes(level)
    kind, index, target = cu.p1_to_p2_map(level)
    assert nf == nv + ne and target.size == nf
    assert np.array_equal(np.sort(target), np.arange(nf))  # onto vertex array + edge array, every DoF once
    assert ((kind == 0) == (target < nv)).all()
    # an edge DoF belongs to the macro-primitive that holds both its end points: the one that holds its midpoint
    p2_classes = np.concatenate([po.slot_of_points(level), po.edge_classes(level)])
    assert np.array_equal(po.slot_of_points(level + 1), p2_classes[target])
    assert np.array_equal(cu.point_classes(level + 1), p2_classes[target])


def test_expected_arrays_of_the_helpers_on_a_tiny_case():
    """level 0 by hand: the fine array of width 3 is v(0,0,0) X v(1,0,0) | Y XY | v(0,1,0) || Z XZ | YZ || v(0,0,1)"""
    p1 = np.arange(10, dtype=np.float64) + 1.0
    v, e = cu.p1_to_p2_expected(p1, np.zeros(4), np.zeros(6), 0, 0x7FFF)
    assert v.tolist() == [1.0, 3.0, 6.0, 10.0]  # ( 0,0,0 ), ( 1,0,0 ), ( 0,1,0 ), ( 0,0,1 )
    assert e.tolist() == [2.0, 4.0, 7.0, 5.0, 8.0, 9.0]  # X, Y, Z, XY, XZ, YZ
    assert np.array_equal(cu.p2_to_p1_expected(np.zeros(10), v, e, 0, 0x7FFF), p1)
    # level 0 has no interior DoF: the interior mask selects nothing
    assert not cu.selected(0, 1 << 14).any()


def test_symbols_are_declared_and_exported():
    import ctypes

    from hyteg_amd import capi

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for sym in ENTRIES:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in include/hyteg_hip.h"
        assert hasattr(raw, sym), f"{sym} is not exported"
        assert sym in capi.SIGNATURES


def test_argument_validation_happens_before_any_gpu_work():
    """bad level, ncells out of range, null and aliased pointers: EINVAL on the host (this test runs without a GPU)"""
    from hyteg_amd import capi

    a, b, c = 4096, 8192, 12288
    batch = {"to_p2": lambda v, e, p, level, masks: capi.p1_to_p2_cells(v, e, p, level, masks),
             "to_p1": lambda v, e, p, level, masks: capi.p2_to_p1_cells(p, v, e, level, masks)}
    single = {"to_p2": lambda v, e, p, level: capi.p1_to_p2_cell(v, e, p, level),
              "to_p1": lambda v, e, p, level: capi.p2_to_p1_cell(p, v, e, level)}
    for call in batch.values():
        for level in (-1, P2_MAX_LEVEL + 1):
            with pytest.raises(capi.HytegHipError, match="level out of range"):
                call([a], [b], [c], level, [0x7FFF])
        with pytest.raises(capi.HytegHipError, match="ncells"):
            call([], [], [], 2, [])
        n = capi.HYTEG_HIP_MAX_BATCH + 1
        with pytest.raises(capi.HytegHipError, match="ncells"):
            call([a] * n, [b] * n, [c] * n, 2, [0x7FFF] * n)
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            call(None, [b], [c], 2, [0x7FFF])
        for v, e, p in ((0, b, c), (a, 0, c), (a, b, 0)):
            with pytest.raises(capi.HytegHipError, match="null array"):
                call([a, v], [b, e], [c, p], 2, [0x7FFF, 0x7FFF])
        for v, e, p in ((a, b, a), (a, b, b)):
            with pytest.raises(capi.HytegHipError, match="alias"):
                call([c, v], [b + 64, e], [a + 64, p], 2, [0, 0x7FFF])
    for call in single.values():
        with pytest.raises(capi.HytegHipError, match="level out of range"):
            call(a, b, c, 10)
        with pytest.raises(capi.HytegHipError, match="null"):
            call(a, None, c, 2)
        with pytest.raises(capi.HytegHipError, match="alias"):
            call(a, b, a, 2)
        with pytest.raises(capi.HytegHipError, match="alias"):
            call(a, b, b, 2)
