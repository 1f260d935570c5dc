"""GPU tests of the steps launch: hyteg_hip_p1_apply_cell_steps (up to 16 independent applies of one stencil in one grid,
p1_apply_zmarch_steps_kernel) and the grouping of apply_cycle in the host layer (P1ConstantOperator::applyRun).  A step of the
launch runs the arithmetic of a single apply on its own pair of arrays, so every destination is compared BIT FOR BIT with
hyteg_hip_p1_apply_cell on the same pair, the entries the apply must not touch included."""
import numpy as np
import pytest

from conftest import SKEW_TET

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    capi.lib()
    host.lib()
    return torch, capi, host, po


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _sentinel(n, k):
    """what a destination holds before the launch: distinct per step and per entry, nothing an apply of values in [0, 1) produces"""
    return -1.0e6 * (k + 1) - np.arange(n, dtype=np.float64)


def _steps_against_single(torch, capi, po, level, nsteps_list):
    rng = np.random.default_rng(50 + level)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    m = po.inner_mask(level)
    st = torch.cuda.current_stream().cuda_stream
    srcs = [_dev(torch, rng.random(n)) for _ in range(16)]
    dst0 = [_sentinel(n, k) for k in range(16)]
    for update in (capi.REPLACE, capi.ADD):
        want = []
        for k in range(16):  # the reference, once per update type: one launch per pair
            d = _dev(torch, dst0[k])
            capi.p1_apply_cell(d.data_ptr(), srcs[k].data_ptr(), level, w, update, st)
            want.append(d)
        torch.cuda.synchronize()
        want = [d.cpu().numpy() for d in want]
        assert not np.array_equal(want[0][m], want[1][m])  # different sources: a step that used another step's pair would show
        for nsteps in nsteps_list:
            dsts = [_dev(torch, dst0[k]) for k in range(nsteps)]
            capi.p1_apply_cell_steps([d.data_ptr() for d in dsts], [s.data_ptr() for s in srcs[:nsteps]], level, w, update, st)
            torch.cuda.synchronize()
            for k, d in enumerate(dsts):
                got = d.cpu().numpy()
                assert np.array_equal(got[~m], dst0[k][~m]), f"level {level}, {nsteps} steps, step {k}: boundary entries were written"
                assert np.array_equal(got, want[k]), f"level {level}, {nsteps} steps, update {update}: step {k} differs from the single apply"


@pytest.mark.parametrize("level", [2, 3, 4, 5])
def test_steps_launch_equals_single_applies_bit_for_bit(env, level):
    """level 2: a handful of bricks and mostly empty workgroups behind the rounding of the grid to 8; level 5: several z-chunks and
    tip bricks with fewer slices than the brick shape"""
    torch, capi, host, po = env
    _steps_against_single(torch, capi, po, level, [1, 2, 3, 16])


@pytest.mark.parametrize("shape", [(4, 8, 2), (8, 4, 2)])
def test_steps_launch_with_other_brick_shapes(env, shape):
    """level 5 runs 2 x 4 (Replace) and 4 x 4 (Add), one slice ahead, by default: the level-8 default shape and the widest one"""
    torch, capi, host, po = env
    try:
        capi.set_apply_shape(*shape)
        _steps_against_single(torch, capi, po, 5, [1, 2, 3, 16])
    finally:
        capi.set_apply_shape()


def test_step_counts_out_of_range_are_errors_and_launch_nothing(env):
    torch, capi, host, po = env
    level = 4
    rng = np.random.default_rng(4)
    w = po.assemble_cell_stencil(SKEW_TET, level)
    n = po.cell_size(level)
    st = torch.cuda.current_stream().cuda_stream
    srcs = [_dev(torch, rng.random(n)) for _ in range(17)]
    dsts = [_dev(torch, _sentinel(n, k)) for k in range(17)]
    for nsteps in (0, 17):
        with pytest.raises(capi.HytegHipError, match="nsteps out of range"):
            capi.p1_apply_cell_steps([d.data_ptr() for d in dsts[:nsteps]], [s.data_ptr() for s in srcs[:nsteps]], level, w, capi.REPLACE, st)
    # a destination that another step reads, or that two steps write: rejected as well
    with pytest.raises(capi.HytegHipError, match="must not be read or written by another"):
        capi.p1_apply_cell_steps([dsts[0].data_ptr(), dsts[1].data_ptr()], [srcs[0].data_ptr(), dsts[0].data_ptr()], level, w, capi.REPLACE, st)
    with pytest.raises(capi.HytegHipError, match="must not be read or written by another"):
        capi.p1_apply_cell_steps([dsts[0].data_ptr(), dsts[0].data_ptr()], [srcs[0].data_ptr(), srcs[1].data_ptr()], level, w, capi.REPLACE, st)
    torch.cuda.synchronize()
    for k, d in enumerate(dsts):
        assert np.array_equal(d.cpu().numpy(), _sentinel(n, k))


def test_apply_cycle_gives_the_same_bytes_for_every_group_size(env):
    """tet_1el, level 5, 23 steps over a ring of 5 pairs: one launch per apply (G = 1), groups of 4 and groups that hold the whole ring
    (G = 16), on one lane (maximal groups) and on the default two; and a ring in which pair 2 reads what pair 1 writes"""
    torch, capi, host, po = env
    from hostutil import MESHES

    level, npairs, steps = 5, 5, 23
    st = host.Storage.from_gmsh(MESHES / "tet_1el.msh")
    A = host.P1ConstantOperator(st, level, level)
    f = [host.P1Function(st, f"f{k}", level, level) for k in range(2 * npairs)]
    rng = np.random.default_rng(23)
    start = [rng.random(host.cell_size(level)) for _ in f]

    def run(srcs, dsts, G, lanes, update):
        for fn, a in zip(f, start):
            fn.upload_cell(0, level, a)
        st.set_apply_steps(G)
        st.set_apply_lanes(lanes)
        A.prepared_cycle(srcs, dsts, level, host.Inner, update)(2, steps)
        launches.append(st.steps_launches())
        return [fn.download_cell(0, level) for fn in f]

    launches = []

    try:
        independent = ([f[2 * k] for k in range(npairs)], [f[2 * k + 1] for k in range(npairs)])
        chained = (list(independent[0]), list(independent[1]))
        chained[0][2] = chained[1][1]  # pair 2's source is pair 1's destination
        for srcs, dsts in (independent, chained):
            for update in (host.Replace, host.Add):
                want = run(srcs, dsts, 1, 1, update)
                assert not np.array_equal(want[1], start[1])
                for G in (1, 4, 16):
                    for lanes in (1, 0):
                        got = run(srcs, dsts, G, lanes, update)
                        # the comparison means something only if grouped launches were really issued: at least one per two
                        # passes over the ring (one lane: whole-ring groups, cut where the chained ring repeats a dependency)
                        if G == 1:
                            assert launches[-1] == 0
                        else:
                            assert launches[-1] >= steps // (2 * npairs), f"G = {G}, lanes {lanes}: {launches[-1]} grouped launches"
                        for k, (a, b) in enumerate(zip(want, got)):
                            assert np.array_equal(a, b), f"G = {G}, lanes {lanes}, update {update}: function {k} differs"
    finally:
        st.set_apply_steps(0)
        st.set_apply_lanes(0)
        for o in (*f, A, st):
            o.close()
