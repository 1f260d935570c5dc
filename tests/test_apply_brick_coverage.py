"""CPU-only: the brick tables of the z-march apply and the store windows the kernel forms from them
(hyteg_hip_p1_apply_brick_coverage: host code, no device).  For every brick shape compiled in and both x-strides the windows
tile the interior of the macro-cell exactly once and touch nothing else -- for the aligned windows (x-stride 56) at every
phase of the destination against the 64-byte lines."""
import numpy as np
import pytest

SHAPES = [(2, 8), (4, 8), (4, 4), (2, 4), (8, 4), (6, 8)]  # ( NY, LZ ) of HYTEG_ZM_SHAPES in p1_apply.hip


@pytest.mark.parametrize("level", [4, 5, 6, 7])
def test_store_windows_tile_the_interior_exactly_once(level):
    from hyteg_amd import capi
    from oracle import p1_oracle as po

    want = po.inner_mask(level).astype(np.uint8)
    for ny, lz in SHAPES:
        count, plain = capi.p1_apply_brick_coverage(level, ny, lz, 62)
        assert np.array_equal(count, want), f"level {level}, {ny} x {lz}, x-stride 62"
        for phase in range(8):
            count, aligned = capi.p1_apply_brick_coverage(level, ny, lz, 56, phase)
            assert np.array_equal(count, want), f"level {level}, {ny} x {lz}, x-stride 56, phase {phase}"
        assert aligned >= plain > 0  # narrower bricks: never fewer of them


def test_level_8_brick_counts():
    """what the defaults run at level 8: 2028 bricks of 4 x 8 (single apply), 1466 of 6 x 8 with aligned windows (steps launch)"""
    from hyteg_amd import capi
    from oracle import p1_oracle as po

    want = po.inner_mask(8).astype(np.uint8)
    for (ny, lz, xs), bricks in (((4, 8, 62), 2028), ((6, 8, 56), 1466)):
        count, n = capi.p1_apply_brick_coverage(8, ny, lz, xs)
        assert n == bricks
        assert np.array_equal(count, want)


def test_bad_arguments_are_rejected():
    from hyteg_amd import capi

    for args in ((9, 4, 8, 62, 0), (5, 4, 9, 62, 0), (5, 4, 8, 60, 0), (5, 4, 8, 56, 8), (5, 0, 8, 62, 0)):
        with pytest.raises(capi.HytegHipError):
            capi.p1_apply_brick_coverage(*args)
