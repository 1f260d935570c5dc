"""The reference's FEniCS element matrices that the oracle pins compare with, also where the reference is not at hand.

oracle/_ref/libhyteg_ref_fenics.so can only be built where the reference's sources are mounted.  Its outputs for exactly the
inputs of the pins (tests/test_oracle_pins.py, test_oracle_p2.py, test_oracle_taylor_hood.py) are recorded in
tests/golden/ref_fenics_forms.npz by oracle/record_ref_fenics.py.  ref_fenics() returns an object with the library's entry
points that writes the recorded matrix; where the library is built it calls the library as well and checks that the two agree.
An input without a recorded output and without the library raises: the pins never skip."""
import ctypes as C
from pathlib import Path

import numpy as np

from oracle import p1_oracle as po

GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_fenics_forms.npz"
# entry point -> (doubles it writes, takes a component index)
ENTRY_POINTS = {"ref_p1_tet_diffusion": (16, False), "ref_p1_tet_mass": (16, False), "ref_p1_tet_pspg": (16, False),
                "ref_p1_tet_div": (16, True), "ref_p1_tet_divt": (16, True), "ref_p2_tet_diffusion": (100, False),
                "ref_p2_to_p1_tet_div": (40, True), "ref_p1_to_p2_tet_divt": (40, True)}
# set to a list by oracle/record_ref_fenics.py: every call appends (entry point, component, coordinates, output)
RECORD = None


def _doubles(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n,))


def _load():
    table = {}
    if GOLDEN.exists():
        with np.load(GOLDEN) as z:
            for name in ENTRY_POINTS:
                if f"{name}__coords" in z:
                    table[name] = (z[f"{name}__coords"], z[f"{name}__k"], z[f"{name}__out"])
    return table


class RefFenics:
    def __init__(self, live, table):
        self._live, self._table = live, table

    def _recorded(self, name, k, coords):
        if name not in self._table:
            return None
        cs, ks, outs = self._table[name]
        rows = np.flatnonzero(ks == k)
        if rows.size == 0:
            return None
        d = np.abs(cs[rows] - coords).max(axis=1)
        j = int(np.argmin(d))
        return outs[rows[j]] if d[j] <= 1e-15 * max(1.0, np.abs(coords).max()) else None

    def __getattr__(self, name):
        if name not in ENTRY_POINTS:
            raise AttributeError(name)
        size, has_k = ENTRY_POINTS[name]

        def call(out, coords, *k):
            c = _doubles(coords, 12).copy()
            comp = int(k[0]) if has_k else -1
            rec = self._recorded(name, comp, c)
            if self._live is not None:
                getattr(self._live, name)(out, coords, *k)
                got = _doubles(out, size)
                if rec is not None:
                    assert np.abs(got - rec).max() <= 1e-15 * np.abs(rec).max(), f"{name}: library and recording differ"
            elif rec is None:
                raise KeyError(f"{name} (component {comp}) has no recorded output for coordinates {c.tolist()}: "
                               "build oracle/_ref and run oracle/record_ref_fenics.py")
            else:
                _doubles(out, size)[:] = rec
            if RECORD is not None:
                RECORD.append((name, comp, c, _doubles(out, size).copy()))

        return call


def ref_fenics():
    return RefFenics(po.ref_fenics(), _load())
