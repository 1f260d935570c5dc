"""CPU-only: the batched P2 grid transfer (hyteg_hip_p2_restrict_cells / hyteg_hip_p2_prolongate_cells) is declared, exported and
bound, and rejects bad arguments on the host before any GPU work (no GPU is present when this runs)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hyteg_hip_p2_restrict_cells", "hyteg_hip_p2_prolongate_cells")
P = 4096  # stands for a device pointer: nothing dereferences it, the calls below fail before any launch


@pytest.fixture(scope="module")
def capi():
    from hyteg_amd import capi

    if not capi.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    return capi


def test_both_symbols_are_declared_exported_and_bound(capi):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} is not declared in include/hyteg_hip.h"
        assert hasattr(raw, sym), f"{sym} is not exported"
        assert sym in capi.SIGNATURES


def _restrict(capi, n=2, level=2, cv=None, ce=None, fv=None, fe=None, nnc=P, masks=None):
    full = [P] * n
    capi.p2_restrict_cells(full if cv is None else cv, full if ce is None else ce, full if fv is None else fv, full if fe is None else fe,
                           level, nnc, [0x7FFF] * n if masks is None else masks)


def _prolongate(capi, n=2, level=2, fv=None, fe=None, cv=None, ce=None, masks=None, update=0):
    full = [P] * n
    capi.p2_prolongate_cells(full if fv is None else fv, full if fe is None else fe, full if cv is None else cv, full if ce is None else ce,
                             level, [0x7FFF] * n if masks is None else masks, update)


@pytest.mark.parametrize("call", [_restrict, _prolongate])
def test_cell_count_must_be_1_to_80(capi, call):
    for n in (0, 81):
        with pytest.raises(capi.HytegHipError, match="ncells"):
            call(capi, n=n)


@pytest.mark.parametrize("call", [_restrict, _prolongate])
@pytest.mark.parametrize("which", ["cv", "ce", "fv", "fe"])
def test_a_null_pointer_inside_a_pointer_list_is_rejected(capi, call, which):
    for hole in (0, 2):
        ptrs = [P] * 3
        ptrs[hole] = 0
        with pytest.raises(capi.HytegHipError, match="null"):
            call(capi, n=3, **{which: ptrs})
    # ... also in a cell whose mask selects nothing
    with pytest.raises(capi.HytegHipError, match="null"):
        call(capi, n=2, masks=[0x7FFF, 0], **{which: [P, 0]})


def test_restriction_needs_the_neighbour_count_table(capi):
    with pytest.raises(capi.HytegHipError, match="null"):
        _restrict(capi, nnc=None)


@pytest.mark.parametrize("call", [_restrict, _prolongate])
def test_coarse_level_must_be_0_to_9(capi, call):
    for level in (-1, 10):
        with pytest.raises(capi.HytegHipError, match="level"):
            call(capi, level=level)


def test_update_must_be_replace_or_add(capi):
    with pytest.raises(capi.HytegHipError, match="update"):
        _prolongate(capi, update=7)
