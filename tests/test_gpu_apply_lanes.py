"""GPU tests of the stream lanes of the host layer (PrimitiveStorage::LaneScope, hyteg_amd/host/lanes.hpp): the loop of
apply_cycle places independent interior applies on two streams.  The kernel and its arguments are the ones of a single
apply() call, so every result is compared BIT FOR BIT with the same steps issued as single apply() calls -- whatever the
dependencies between the steps are, and whatever the lane count is."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi, host
    from oracle import p1_oracle as po

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host, po


class Bench:
    """tet_1el at one level: `nf` functions with fixed random start values, and the two ways of issuing a list of steps"""

    def __init__(self, host, level, nf, lanes=None):
        from hostutil import MESHES

        self.host, self.level = host, level
        self.st = host.Storage.from_gmsh(MESHES / "tet_1el.msh")
        if lanes is not None:
            self.st.set_apply_lanes(lanes)
        self.A = host.P1ConstantOperator(self.st, level, level)
        self.f = [host.P1Function(self.st, f"f{k}", level, level) for k in range(nf)]
        rng = np.random.default_rng(100 + level)
        self.start = [rng.random(host.cell_size(level)) for _ in range(nf)]

    def reset(self):
        for f, a in zip(self.f, self.start):
            f.upload_cell(0, self.level, a)

    def state(self):
        return [f.download_cell(0, self.level) for f in self.f]

    def single(self, steps, update):
        self.reset()
        for i, j in steps:
            self.A.apply(self.f[i], self.f[j], self.level, self.host.Inner, update)
        return self.state()

    def cycle(self, steps, update, download=True):
        self.reset()
        srcs, dsts = [self.f[i] for i, _ in steps], [self.f[j] for _, j in steps]
        self.A.apply_cycle(srcs, dsts, self.level, self.host.Inner, update, 0, len(steps))
        return self.state() if download else None

    def close(self):
        for o in (*self.f, self.A, self.st):
            o.close()


def _cases():
    ring = [(2 * k, 2 * k + 1) for k in range(3)]
    return {
        "ring": [ring[k % 3] for k in range(3 * 5 + 2)],              # (a) independent pairs, K several times the ring
        "ping_pong": [(0, 1) if k % 2 == 0 else (1, 0) for k in range(7)],  # (b)
        "fan_out": [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)],          # (c) one src into several dsts
        "fan_in": [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (2, 0)],    # (c) several srcs into one dst: the last writer wins
        "mixed": [(0, 1), (2, 3), (1, 2), (4, 5), (3, 0), (0, 4), (2, 3), (5, 1), (1, 2), (4, 0)],
    }


@pytest.mark.parametrize("level", [5, 8])
@pytest.mark.parametrize("lanes", [None, 1, 3])  # (d): 1 through the setter; None = the default
def test_apply_cycle_equals_single_applies_bit_for_bit(env, level, lanes):
    torch, capi, host, po = env
    b = Bench(host, level, 6, lanes)
    for name, steps in _cases().items():
        for update in (host.Replace, host.Add):
            want = b.single(steps, update)
            got = b.cycle(steps, update)
            # the comparison means something only if the cycle really used its lanes: independent steps on all of them,
            # a dependent chain on one, and none with a lane count of 1
            seen = b.st.lanes_seen()
            n = 2 if lanes is None else lanes
            if n == 1:
                assert seen == 0
            elif name in ("ring", "fan_out", "mixed"):
                assert seen == (1 << n) - 1, f"{name}: lanes seen {seen:#x}"
            else:
                assert seen == 1, f"{name}: lanes seen {seen:#x}"
            for k, (w, g) in enumerate(zip(want, got)):
                assert np.array_equal(w, g), f"{name}, update {update}: function {k} differs"
    # Add on a ring: every visit of a pair changes its destination, a lost or reordered update would show
    steps = [(0, 1), (2, 3)] * 6
    assert not np.array_equal(b.single(steps[:2], host.Add)[1], b.single(steps, host.Add)[1])
    b.close()


class _DevArray:
    """a device array of doubles behind a raw pointer, for torch.as_tensor (no copy)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


@pytest.mark.parametrize("level", [5, 8])
def test_the_callers_stream_sees_the_final_values_without_synchronising(env, level):
    """(e): what apply_cycle put on its lanes is joined into the storage's stream before it returns"""
    torch, capi, host, po = env
    b = Bench(host, level, 6)
    steps = _cases()["ring"] + _cases()["mixed"]
    want = b.single(steps, host.Replace)
    user = torch.cuda.Stream()
    b.st.set_stream(user.cuda_stream)
    b.reset()
    views = [torch.as_tensor(_DevArray(f.cell_pointer(0, level), host.cell_size(level)), device="cuda") for f in b.f]
    srcs, dsts = [b.f[i] for i, _ in steps], [b.f[j] for _, j in steps]
    with torch.cuda.stream(user):
        b.A.apply_cycle(srcs, dsts, level, host.Inner, host.Replace, 0, len(steps))
        copies = [v * 1.0 for v in views]  # torch kernels on the caller's stream, directly behind the cycle
    user.synchronize()
    for k, (w, c) in enumerate(zip(want, copies)):
        assert np.array_equal(w, c.cpu().numpy()), f"function {k}"
    b.st.set_stream(None)
    b.close()


@pytest.mark.parametrize("cell_lanes", [False, True])
def test_multi_cell_apply_matches_the_oracle(env, cell_lanes):
    """cube_6el, level 7: the comparison of test_gpu_host.test_apply_matches_the_multi_cell_oracle, with the cell loop's
    lanes off (the default) and on, for a single apply() and inside apply_cycle"""
    torch, capi, host, po = env
    from hostutil import MESHES, MultiCellOracle, download, upload

    level = 7
    st = host.Storage.from_gmsh(MESHES / "cube_6el.msh")
    st.set_apply_cell_lanes_min(2 if cell_lanes else 0)
    mo = MultiCellOracle(st)
    A = host.P1ConstantOperator(st, level, level)
    src, dst = host.P1Function(st, "src", level, level), host.P1Function(st, "dst", level, level)
    rng = np.random.default_rng(3)
    src_h = mo.interpolate(lambda x, y, z: np.sin(37.0 * x + 11.0 * y * y + 5.0 * z) + x * y, level)
    dst0 = [rng.random(po.cell_size(level)) for _ in src_h]
    mo.sync(dst0, level, host.All)
    for fl in (host.Inner, host.All):
        ref = mo.apply(src_h, [d.copy() for d in dst0], level, fl)
        results = []
        for how in ("apply", "cycle"):
            for update in (host.Replace, host.Add):
                upload(src, src_h, level)
                upload(dst, dst0, level)
                if how == "apply":
                    A.apply(src, dst, level, fl, update)
                else:
                    A.apply_cycle([src], [dst], level, fl, update, 0, 1)
                assert st.lanes_seen() == (3 if cell_lanes else 0)
                got = download(dst, level)
                results.append(got)
                for i, (g, r_, d0) in enumerate(zip(got, ref, dst0)):
                    sel = ((st.mask(i, fl) >> po.slot_of_points(level)) & 1).astype(bool)
                    assert np.array_equal(g[~sel], d0[~sel])
                    want = r_ if update == host.Replace else r_ + d0
                    assert np.linalg.norm(g[sel] - want[sel]) / np.linalg.norm(want[sel]) < 1e-12
        # the same kernels with the same arguments: apply() and apply_cycle agree to the bit
        for a, c in zip(results[0] + results[1], results[2] + results[3]):
            assert np.array_equal(a, c)
    for o in (src, dst, A, st):
        o.close()
