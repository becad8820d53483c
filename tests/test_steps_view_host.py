"""The flat-step view of a labelled variable (contrack_amd.contrack._Steps) on the host, through tests/minixr.py: slab() against
reader() for every dim order, the pieces a window is read in, only=, integer=, the fallback without isel, and restore()."""
import itertools

import numpy as np
import pytest

import minixr
from contrack_amd import contrack as cm

R, M, T, L, NY, NX = 2, 3, 5, 4, 4, 6
SIZES = dict(run=R, member=M, time=T, level=L, lat=NY, lon=NX)
LEVEL_RUNS = {(0, 1, 2, 3): [(0, 4)], (0, 1, 3): [(0, 2), (3, 1)], (1, 2): [(1, 2)]}


class Counting(minixr.DataArray):
    """records the arguments of every isel call"""

    def isel(self, **indexers):
        self.__dict__.setdefault("calls", []).append(dict(indexers))
        return super().isel(**indexers)


def variable(canon, dims, dtype=np.float64):
    """a variable with dims `dims` whose values number the elements in the order `canon`"""
    shape = tuple(SIZES[d] for d in canon)
    data = np.arange(int(np.prod(shape)), dtype=dtype).reshape(shape)
    return Counting(np.ascontiguousarray(data.transpose([canon.index(d) for d in dims])), dims), data


def view_of(da, step_dims, level=None):
    return cm._Steps(da, step_dims, "lat", "lon", level)


def partition(steps):
    """chunks of 4 steps with a short last one (no size here is a multiple of 4)"""
    return [(t0, min(4, steps - t0)) for t0 in range(0, steps, 4)]


def windows(steps):
    """(t0, nt): one step; ending exactly at a run of T steps; the whole series; the partition; crossing one boundary; crossing
    two.  A series of one run (steps == T) has no boundary to cross."""
    w = [(2, 1), (T - 3, 3), (0, steps)] + partition(steps)
    return w if steps == T else w + [(T - 2, 4), (T - 1, T + 2)]


def read(view, t0, nt, tail, **kwargs):
    out = np.full((nt,) + tail, -1.0)
    view.reader(**kwargs)(t0, nt, out)
    return out


def check(canon, dims, step_dims, level=None):
    da, data = variable(canon, dims)
    view = view_of(da, step_dims, level)
    nstep = len(step_dims)
    assert view.step_shape == tuple(SIZES[d] for d in step_dims) and view.shape == (view.steps, NY, NX)
    slab = view.slab()
    want = data.reshape((-1,) + data.shape[nstep:])                        # (canon lists the step dims first, then [level,] lat, lon)
    assert np.array_equal(slab, want)
    if dims == canon:
        assert np.shares_memory(slab, da.data)
    back = view.restore(slab, dims)
    assert np.array_equal(back, da.data) and np.shares_memory(view.restore(want, dims), want)
    for sel, runs in (LEVEL_RUNS.items() if level else [(None, None)]):
        part = slab if sel is None else slab[:, list(sel)]
        whole = np.full(part.shape, -1.0)
        for t0, nt in partition(view.steps):                               # the partition fills the slab
            view.reader(level_runs=runs)(t0, nt, whole[t0:t0 + nt])
        assert np.array_equal(whole, part)
        for t0, nt in windows(view.steps):
            da.__dict__["calls"] = []
            got = read(view, t0, nt, part.shape[1:], level_runs=runs)
            assert np.array_equal(got, part[t0:t0 + nt]), (dims, t0, nt)
            touched = (t0 + nt - 1) // T - t0 // T + 1
            calls = da.__dict__["calls"]
            assert len(calls) == touched * (1 if runs is None else len(runs)), (dims, t0, nt, calls)
            for kw in calls:
                assert isinstance(kw[step_dims[-1]], slice) and all(isinstance(kw[d], int) for d in step_dims[:-1])
                assert set(kw) == set(step_dims) | ({level} if level else set())


@pytest.mark.parametrize("dims", list(itertools.permutations(("time", "lat", "lon"))))
def test_time_alone(dims):
    check(("time", "lat", "lon"), dims, ("time",))


@pytest.mark.parametrize("dims", list(itertools.permutations(("member", "time", "lat", "lon"))))
def test_member_and_time(dims):
    check(("member", "time", "lat", "lon"), dims, ("member", "time"))


@pytest.mark.parametrize("dims", list(itertools.permutations(("time", "level", "lat", "lon"))))
def test_time_and_level(dims):
    check(("time", "level", "lat", "lon"), dims, ("time",), "level")


CANON5 = ("run", "member", "time", "level", "lat", "lon")
ORDERS5 = [CANON5, CANON5[::-1], ("time", "run", "level", "member", "lat", "lon"), ("lat", "lon", "level", "time", "member", "run"),
           ("member", "run", "time", "level", "lat", "lon"), ("level", "run", "lat", "member", "lon", "time"),
           ("run", "time", "lat", "level", "lon", "member"), ("lon", "member", "time", "lat", "run", "level")]


@pytest.mark.parametrize("dims", ORDERS5)
def test_two_outer_step_dims_and_level(dims):
    check(CANON5, dims, ("run", "member", "time"), "level")


def test_step_dims_in_their_own_order():
    """(time, member) as step dims: flat step t * M + m, the member dim the one that is sliced"""
    da, data = variable(("member", "time", "lat", "lon"), ("member", "time", "lat", "lon"))
    view = view_of(da, ("time", "member"))
    want = data.transpose(1, 0, 2, 3).reshape(T * M, NY, NX)
    assert np.array_equal(view.slab(), want)
    out = np.empty((T * M, NY, NX))
    view.reader()(0, T * M, out)
    assert np.array_equal(out, want) and len(da.calls) == T and all(isinstance(kw["member"], slice) for kw in da.calls)


@pytest.mark.parametrize("dims", [("member", "time", "lat", "lon"), ("lon", "time", "member", "lat")])
def test_only_one_member(dims):
    da, data = variable(("member", "time", "lat", "lon"), dims)
    view = view_of(da, ("member", "time"))
    slab = view.slab()
    for m in range(M):
        assert np.array_equal(view.slab(only=m), slab[m * T:(m + 1) * T]) and np.shares_memory(view.slab(only=m), da.data)
        da.__dict__["calls"] = []
        for t0, nt in ((0, T), (1, 3), (T - 1, 1)):
            assert np.array_equal(read(view, t0, nt, (NY, NX), only=m), slab[m * T + t0:m * T + t0 + nt])
        assert len(da.calls) == 3 and all(kw["member"] == m for kw in da.calls)


def test_integer_pieces_are_checked_where_they_are_read():
    da, data = variable(("member", "time", "lat", "lon"), ("time", "member", "lon", "lat"), dtype=np.int64)
    da.data[12 % T, 12 // T, 3, 2] = 2 ** 31                              # flat step 12 = member 2, step 2
    view = view_of(da, ("member", "time"))
    assert view.slab()[12].max() == 2 ** 31
    reader = view.reader(integer=True)
    out = np.empty((view.steps, NY, NX), dtype=np.int32)
    reader(0, 12, out[:12])                                                # ends before step 12
    reader(13, 2, out[13:])
    assert np.array_equal(out[:12], view.slab()[:12])
    for t0, nt in ((12, 1), (10, 4), (0, 15)):
        with pytest.raises(ValueError, match="flag ids beyond int32"):
            reader(t0, nt, out[t0:t0 + nt])
    view.reader()(12, 1, np.empty((1, NY, NX)))                            # not a flag variable: nothing to check
    floats = view_of(variable(("time", "lat", "lon"), ("time", "lat", "lon"))[0], ("time",))
    with pytest.raises(ValueError, match="flag must be an integer field"):
        floats.reader(integer=True)(0, 2, np.empty((2, NY, NX), dtype=np.int32))


class Bare:
    """a 3-D variable without isel: .data, .shape, .dims and .dtype only"""

    def __init__(self, data, dims):
        self.data, self.dims, self.shape, self.dtype = data, dims, data.shape, data.dtype


@pytest.mark.parametrize("dims", list(itertools.permutations(("time", "lat", "lon"))))
def test_without_isel(dims):
    da, data = variable(("time", "lat", "lon"), dims)
    view = view_of(Bare(da.data, dims), ("time",))
    for t0, nt in windows(T):
        assert np.array_equal(read(view, t0, nt, (NY, NX)), data[t0:t0 + nt])
    big = Bare(np.full((T, NY, NX), 2 ** 31, dtype=np.int64), ("time", "lat", "lon"))
    with pytest.raises(ValueError, match="flag ids beyond int32"):
        view_of(big, ("time",)).reader(integer=True)(0, 1, np.empty((1, NY, NX), dtype=np.int32))


def test_restore_drops_and_keeps_dims():
    dims = ("lat", "time", "level", "member", "lon")
    da, data = variable(("member", "time", "level", "lat", "lon"), dims)
    view = view_of(da, ("member", "time"), "level")
    mean = view.slab().mean(axis=1)                                        # what calc_vertical_mean hands back: (steps, lat, lon)
    out_dims = ("lat", "time", "member", "lon")
    out = view.restore(mean, out_dims)
    assert out.shape == (NY, T, M, NX) and np.shares_memory(out, mean)
    assert np.array_equal(out, da.data.mean(axis=2))
    da4, data4 = variable(("member", "time", "lat", "lon"), ("time", "lon", "member", "lat"))
    view4 = view_of(da4, ("member", "time"))
    flag = np.ascontiguousarray(view4.slab()).astype(np.int32)             # what run_contrack gets from the library: (M * T, lat, lon)
    assert np.array_equal(view4.restore(flag, da4.dims), da4.data) and np.shares_memory(view4.restore(flag, da4.dims), flag)
    assert np.array_equal(view_of(da4, ("member", "time")).restore(flag, ("member", "time", "lat", "lon")), data4)


def test_the_factory_fills_in_the_names_and_drops_a_missing_member():
    c = cm.contrack()
    c._time_name, c._latitude_name, c._longitude_name = "time", "lat", "lon"
    da, data = variable(("member", "time", "lat", "lon"), ("member", "time", "lat", "lon"))
    assert c._steps(da, ("member", "time")).step_dims == ("member", "time") and c._steps(da, ("member", "time")).shape == (M * T, NY, NX)
    da3, data3 = variable(("time", "lat", "lon"), ("lon", "time", "lat"))
    view = c._steps(da3, (None, "time"))
    assert view.step_dims == ("time",) and np.array_equal(view.slab(), data3)
    assert cm._producer_dtype(np.float32) == np.float32 and all(cm._producer_dtype(t) == np.float64 for t in (np.float64, np.float16, np.int32))
