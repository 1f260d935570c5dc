"""Records tests/golden/ref_fenics_forms.npz: the outputs of oracle/_ref/libhyteg_ref_fenics.so (the reference's FEniCS element
matrices, built only where the reference is mounted) for every input the oracle pins pass to it, so that the pins run without
the reference (tests/ref_golden.py).  Runs those pins once with the library and keeps what it returned.

    python oracle/record_ref_fenics.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PINS = ["tests/test_oracle_pins.py", "tests/test_oracle_p2.py", "tests/test_oracle_taylor_hood.py"]


def main():
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import pytest

    import ref_golden
    from oracle import p1_oracle as po

    if po.ref_fenics() is None:
        raise SystemExit("oracle/_ref/libhyteg_ref_fenics.so is not built (make -C oracle ref, where the reference is mounted)")
    calls = ref_golden.RECORD = []
    rc = pytest.main(["-q", "-p", "no:cacheprovider", *[str(ROOT / p) for p in PINS]])
    if rc != 0:
        raise SystemExit(f"the pins failed (pytest exit {rc}): nothing recorded")
    arrays = {}
    for name in ref_golden.ENTRY_POINTS:
        seen = {}
        for n, k, c, out in calls:
            if n == name:
                seen.setdefault((k, c.tobytes()), (k, c, out))
        if seen:
            rows = list(seen.values())
            arrays[f"{name}__k"] = np.array([r[0] for r in rows], dtype=np.int32)
            arrays[f"{name}__coords"] = np.array([r[1] for r in rows])
            arrays[f"{name}__out"] = np.array([r[2] for r in rows])
    np.savez_compressed(ref_golden.GOLDEN, **arrays)
    print(f"{ref_golden.GOLDEN.relative_to(ROOT)}: {sum(len(v) for k, v in arrays.items() if k.endswith('__k'))} matrices, "
          f"{ref_golden.GOLDEN.stat().st_size} bytes")


if __name__ == "__main__":
    main()
