"""The run_lifecycle reductions pinned at their table, seam and strip edges: the slabs of tests/life_forms.py on both sides of every
limit of k_life_seam / k_life_strips / k_life_finish and of k_lifecycle, with ctk_debug_lifecycle_path saying which path every time
step took.  Every case: t / label / shift / area equal to numpy's rows, the three weighted sums within rtol 1e-12 / atol 1e-9 (the
standard of tests/test_lifecycle.py), every (t, label) exactly once, ctk_lifecycle_exact over ALL rows bit for bit numpy's own
calls, and -- where the reference's frame is defined -- the frame equal to the scipy port's."""
import ctypes as C

import numpy as np
import pytest

import life_forms as lf
import life_util
from contrack_amd.contrack import lifecycle_frame
from oracle import lifecycle_port

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def tracker():
    from contrack_amd import _native
    with _native.Tracker(0) as t:
        yield t


@pytest.fixture
def fresh_tracker():
    from contrack_amd import _native
    with _native.Tracker(0) as t:
        yield t


def _check_rows(trk, c, field, rows):
    """rows of the last lifecycle call on trk against numpy; returns (path, steps)"""
    flag = c["flag"]
    T = flag.shape[0]
    path, steps = trk.debug_lifecycle_path(T)
    print("path", path, "rounds of k_lifecycle per busy step", {int(t): int(s) for t, s in enumerate(steps) if s})
    want = life_util.numpy_rows(flag, field, c["wrow"])
    assert len(rows) == len(want)
    assert len(set(zip(rows["t"].tolist(), rows["label"].tolist()))) == len(rows)          # every (t, label) once
    for k in ("t", "label", "shift", "area"):
        assert np.array_equal(rows[k], want[k]), k
    for k in ("swv", "swvy", "swvx"):
        assert np.allclose(rows[k], want[k], rtol=1e-12, atol=1e-9), k
    ex = trk.lifecycle_exact(np.arange(len(rows)))
    exact = life_util.numpy_exact_rows(flag, field, c["wrow"], want, extent=True)
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(ex[k], exact[k]), k
    if c["lat"] is not None:
        assert lifecycle_frame(rows, c["lat"], c["lon"], c["dates"], trk) == \
            lifecycle_port.run_lifecycle(flag, field, c["lat"], c["lon"], c["wrow"], c["dates"])
    assert steps.tolist() == c["steps"]
    assert path["given_up"] == sum(1 for s in c["steps"] if s) and path["launches"] == max(c["steps"])
    plan = lf.life_plan(T, flag.shape[1], flag.shape[2])
    assert (path["rw"], path["nsx"], path["nby"]) == (plan["rw"], plan["nsx"], plan["nby"])
    return path, steps


def _run(trk, c, dtype, seed=0):
    field = lf.field_for(c["flag"], dtype, seed)
    rows = trk.lifecycle(c["flag"], field, c["wrow"])
    path, steps = _check_rows(trk, c, field, rows)
    return rows, path


# ---- a. ids per step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reverse", [False, True])
def test_ids_per_step(tracker, reverse, dtype):
    """0 / 127 / 128 ids: strips; 129 / 512: one pass of k_lifecycle; 513: two residue classes -- fitting and overflowing steps in one call"""
    c = lf.ids_case(reverse)
    assert c["steps"] == ([2, 1, 1, 0, 0, 0] if reverse else [0, 0, 0, 1, 1, 2])
    rows, _ = _run(tracker, c, dtype)
    assert len(rows) == sum(lf.IDS_PER_STEP)


# ---- b. crossing ids -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_crossing_ids(tracker, dtype):
    """4 crossing ids: strips; 5 and 32: one pass of k_lifecycle; 33: two"""
    c = lf.crossing_case()
    assert c["steps"] == [0, 1, 1, 2]
    rows, _ = _run(tracker, c, dtype)
    assert [(rows["shift"][rows["t"] == t] >= 0).sum() for t in range(4)] == lf.CROSS_PER_STEP


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx", [1, 2])
def test_crossing_ids_narrow_planes(tracker, nx, dtype):
    c = lf.narrow_case(nx)
    rows, _ = _run(tracker, c, dtype)
    if nx == 1:
        assert (rows["shift"] == -2).all() and len(rows) == 9
    else:
        assert sorted(set(rows["shift"].tolist())) == [-1, 1]


def test_crossing_ids_wide_plane(tracker):
    """nxw = 65: the gap search of k_life_finish takes a second trip, the largest gap lies across its edge and a strip's"""
    c = lf.wide_case()
    rows, path = _run(tracker, c, np.float32)
    assert path["nsx"] == 9
    for t, shifts in enumerate(c["shifts"]):
        got = rows[(rows["t"] == t) & (rows["label"] >= 50)]
        assert got["shift"].tolist() == shifts


# ---- c. the seam table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_table_overflow(tracker, dtype):
    c = lf.seam_table_case()
    assert c["steps"] == [3]
    rows, _ = _run(tracker, c, dtype)
    assert len(rows) == 1040


# ---- d. hash chains and row order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dense", [False, True])
def test_hash_chains_and_row_order(tracker, dense, dtype):
    c = lf.dense_case() if dense else lf.chain_case()
    assert c["steps"] == ([0, 0] if dense else [0, 1])
    rows, path = _run(tracker, c, dtype)
    assert path["sort"] == c["sort"] == (0 if dense else 1)
    key = list(zip(rows["label"].tolist(), rows["t"].tolist()))
    assert key == sorted(key) and key[0][0] < 0 < key[-1][0]                                 # signed (label, t) order
    if not dense:
        assert key[:2] == [(-2 ** 31, 0), (-2 ** 31, 1)] and key[-2:] == [(2 ** 31 - 1, 0), (2 ** 31 - 1, 1)]


# ---- e. production rows per wave ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,plan", lf.RW_CASES)
def test_production_rows_per_wave(tracker, shape, dtype, plan):
    c = lf.rw_case(*shape)
    rows, path = _run(tracker, c, dtype)
    assert {k: path[k] for k in plan} == plan
    assert path["given_up"] == 0 and path["launches"] == 0
    assert (rows["shift"] > 0).sum() == sum(i % 5 for i in range(33))


# ---- f. the vector form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx", lf.VEC_NX)
def test_vector_form_by_row_length(tracker, nx, dtype):
    c = lf.vec_case(nx)
    assert c["steps"][2] == 1
    _, path = _run(tracker, c, dtype)
    assert path["vec"] == int(nx % 4 == 0)


@pytest.mark.parametrize("dtype,flag_off,field_off,vec", [(np.float32, 4, 0, 0), (np.float32, 0, 4, 0), (np.float64, 0, 16, 0),
                                                          (np.float64, 4, 0, 0), (np.float64, 0, 32, 1), (np.float32, 0, 16, 1)])
def test_vector_form_by_alignment(tracker, dtype, flag_off, field_off, vec):
    """nx = 256 on device buffers whose slabs start off a 16-byte (float64 field: 32-byte) boundary: the scalar-load form"""
    c = lf.vec_case(256, seed=1)
    flag = c["flag"]
    field = lf.field_for(flag, dtype, 3)
    T, ny, nx = flag.shape
    fd, vd = tracker.malloc(flag.nbytes + 64), tracker.malloc(field.nbytes + 64)
    try:
        assert fd.value % 32 == 0 and vd.value % 32 == 0
        fp, vp = C.c_void_p(fd.value + flag_off), C.c_void_p(vd.value + field_off)
        tracker.h2d(fp, flag)
        tracker.h2d(vp, field)
        rows = tracker.lifecycle_dev(fp, vp, T, ny, nx, c["wrow"], f64=dtype == np.float64)
        path, _ = _check_rows(tracker, c, field, rows)
    finally:
        tracker.free(fd)
        tracker.free(vd)
    assert path["vec"] == vec


# ---- g. the row table grows ----------------------------------------------------------------------------------------------
def test_row_table_regrowth(fresh_tracker):
    c = lf.regrowth_case()
    rows, path = _run(fresh_tracker, c, np.float32)
    assert len(rows) == 5120 and path["attempts"] == 2
    again = fresh_tracker.lifecycle(c["flag"], lf.field_for(c["flag"], np.float32), c["wrow"])     # the table is large enough now
    path, steps = fresh_tracker.debug_lifecycle_path(2)
    assert path["attempts"] == 1 and steps.tolist() == c["steps"]
    for k in ("t", "label", "shift", "area"):
        assert np.array_equal(again[k], rows[k]), k


def test_small_call_needs_one_attempt(fresh_tracker):
    from contrack_amd import _native
    with pytest.raises(_native.ContrackHipError):
        fresh_tracker.debug_lifecycle_path(2)                                                # no call yet
    c = lf.dense_case()
    _, path = _run(fresh_tracker, c, np.float32)
    assert path["attempts"] == 1
    with pytest.raises(ValueError):
        fresh_tracker.debug_lifecycle_path(3)                                                # another T than the call's
