"""ctk_lifecycle_stream_* on the GPU: the run_lifecycle reductions with both slabs passing through chunk-sized device buffers.

Every golden case at chunk lengths on both sides of its T (rows against numpy's, the frame digit for digit the scipy port's); the
exact re-evaluation taken in later chunks; 40 random slabs with every row picked (records bit for bit numpy's own calls); the table
overflows of tests/life_forms.py in a later chunk (the same rounds of k_lifecycle per plane as the resident entry); the callback
form, failing readers and picks, and the degenerate inputs."""
import functools

import numpy as np
import pytest

import life_forms as lf
import life_util
from contrack_amd.contrack import fragile_rows, lifecycle_frame
from oracle import lifecycle_port

pytestmark = pytest.mark.gpu
CASES = life_util.case_names()


@pytest.fixture(scope="module")
def tracker():
    from contrack_amd import _native
    with _native.Tracker(0) as t:
        yield t


@functools.lru_cache(maxsize=None)
def golden(name):
    """(case, numpy's rows, the port's frame), computed once per case and left unchanged"""
    g = life_util.load(name)
    dates = life_util.dates_of(g["time"])
    return (g, dates, life_util.numpy_rows(g["flag"], g["variable"], g["wrow"]),
            lifecycle_port.run_lifecycle(g["flag"], g["variable"], g["lat"], g["lon"], g["wrow"], dates))


def all_rows(rows):
    return np.arange(len(rows))


def check_rows(rows, want, area_exact=True):
    """area_exact=False: `want` holds numpy's pairwise sum of weights that are not small integers -- the device's area (exact, rounded
    once) lies within the pairwise tree's 5e-15 of it, not always on it; the exact records are what is compared bit for bit there"""
    assert len(rows) == len(want)
    for k in ("t", "label", "shift") + (("area",) if area_exact else ()):
        assert np.array_equal(rows[k], want[k]), k
    for k in ("swv", "swvy", "swvx") + (() if area_exact else ("area",)):
        assert np.allclose(rows[k], want[k], rtol=1e-12, atol=1e-9), k


# ---- golden cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", ["1", "2", "3", "T-1", "T", "T+5", "0"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_by_chunk_length(tracker, name, chunk):
    g, dates, want, frame = golden(name)
    T = g["flag"].shape[0]
    assert 3 <= T <= 16
    steps = {"T-1": T - 1, "T": T, "T+5": T + 5}.get(chunk) or int(chunk)
    rows, idx, ex = tracker.lifecycle_stream(g["flag"], g["variable"], g["wrow"], chunk_steps=steps, pick=fragile_rows)
    check_rows(rows, want)
    assert np.array_equal(idx, fragile_rows(rows))                 # the rule is per row: chunk by chunk it picks what it picks on all rows
    assert np.all(np.diff(idx) > 0)
    assert lifecycle_frame(rows, g["lat"], g["lon"], dates, exact=(idx, ex)) == frame
    path, per_step = tracker.debug_lifecycle_path(T)
    assert len(per_step) == T


@pytest.mark.parametrize("name", ["smooth2", "refslab"])
def test_later_chunks_take_the_exact_path(tracker, name):
    g, dates, want, frame = golden(name)
    rows, idx, ex = tracker.lifecycle_stream(g["flag"], g["variable"], g["wrow"], chunk_steps=4, pick=fragile_rows)
    picked_t = rows["t"][idx]
    print(name, "picked rows at t =", sorted(set(picked_t.tolist())))
    assert (picked_t >= 4).any()
    exact = life_util.numpy_exact_rows(g["flag"], g["variable"], g["wrow"], want[idx])
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(ex[k], exact[k]), k
    assert lifecycle_frame(rows, g["lat"], g["lon"], dates, exact=(idx, ex)) == frame


# ---- random cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("i", range(40))
def test_random_cases_every_row_exact(tracker, i, chunk):
    flag, field, lat, lon, wrow, dates = life_util.random_life_case(i)
    rows, idx, ex = tracker.lifecycle_stream(flag, field, wrow, chunk_steps=chunk, pick=all_rows)
    want = life_util.numpy_rows(flag, field, wrow)
    check_rows(rows, want, area_exact=False)
    assert np.array_equal(idx, np.arange(len(rows)))
    exact = life_util.numpy_exact_rows(flag, field, wrow, want)
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(ex[k], exact[k]), k
    assert lifecycle_frame(rows, lat, lon, dates, exact=(idx, ex)) == lifecycle_port.run_lifecycle(flag, field, lat, lon, wrow, dates)


# ---- table overflow in a later chunk --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["ids", "crossing"])
def test_table_overflow_in_a_later_chunk(tracker, case, dtype):
    c = lf.ids_case() if case == "ids" else lf.crossing_case()
    flag = c["flag"]
    T = flag.shape[0]
    field = lf.field_for(flag, dtype)
    rows, idx, ex = tracker.lifecycle_stream(flag, field, c["wrow"], chunk_steps=2, pick=fragile_rows)
    check_rows(rows, life_util.numpy_rows(flag, field, c["wrow"]))
    assert lifecycle_frame(rows, c["lat"], c["lon"], c["dates"], exact=(idx, ex)) == \
        lifecycle_port.run_lifecycle(flag, field, c["lat"], c["lon"], c["wrow"], c["dates"])
    path, steps = tracker.debug_lifecycle_path(T)
    want = [lf.expected_rounds(flag[t]) for t in range(T)]
    assert steps.tolist() == want == c["steps"]
    assert any(s for s in want[2:])                                       # an overflow past the first chunk
    assert path["given_up"] == sum(1 for s in want if s)
    assert path["launches"] == sum(max(want[t0:t0 + 2]) for t0 in range(0, T, 2))     # summed over the chunks
    assert path["attempts"] >= (T + 1) // 2
    plan = lf.life_plan(2, flag.shape[1], flag.shape[2], f64=dtype == np.float64)
    assert (path["rw"], path["nsx"], path["nby"]) == (plan["rw"], plan["nsx"], plan["nby"])      # the first chunk's


# ---- callback form and error cases ----------------------------------------------------------------------------------------
def readers(flag, field, fail_at=None, log=None):
    def fread(t0, nt, out):
        if log is not None:
            log.append(("flag", t0, nt))
        if fail_at is not None and t0 >= fail_at:
            raise OSError("no such slice")
        assert out.dtype == np.int32 and out.shape == (nt,) + flag.shape[1:]
        out[...] = flag[t0:t0 + nt]

    def vread(t0, nt, out):
        if log is not None:
            log.append(("field", t0, nt))
        assert out.dtype == field.dtype
        out[...] = field[t0:t0 + nt]
    return fread, vread


@pytest.mark.parametrize("name", ["smooth2", "float64"])
def test_callback_form_equals_the_array_form(tracker, name):
    g, dates, want, frame = golden(name)
    flag, field = g["flag"], g["variable"]
    T = flag.shape[0]
    a_rows, a_idx, a_ex = tracker.lifecycle_stream(flag, field, g["wrow"], chunk_steps=3, pick=fragile_rows)
    log = []
    fread, vread = readers(flag, field, log=log)
    rows, idx, ex = tracker.lifecycle_stream(fread, vread, g["wrow"], shape=flag.shape, dtype=field.dtype, chunk_steps=3, pick=fragile_rows)
    check_rows(rows, a_rows)
    assert np.array_equal(idx, a_idx) and ex.tobytes() == a_ex.tobytes()
    want_log = []
    for t0 in range(0, T, 3):                                            # increasing t0, once per chunk, the flags first
        want_log += [("flag", t0, min(3, T - t0)), ("field", t0, min(3, T - t0))]
    assert log == want_log
    times = tracker.stream_times()
    assert times["reader"] > 0 and times["input_phase"] >= times["reader"]
    # one source an array, the other a reader
    rows, idx, ex = tracker.lifecycle_stream(flag, vread, g["wrow"], dtype=field.dtype, chunk_steps=3, pick=fragile_rows)
    check_rows(rows, a_rows)
    assert np.array_equal(idx, a_idx) and ex.tobytes() == a_ex.tobytes()


def test_failing_reader_and_failing_pick_leave_the_tracker_usable(tracker):
    from contrack_amd import _native
    g, dates, want, frame = golden("smooth1")
    flag, field = g["flag"], g["variable"]
    fread, vread = readers(flag, field, fail_at=4)
    with pytest.raises(OSError):
        tracker.lifecycle_stream(fread, vread, g["wrow"], shape=flag.shape, dtype=field.dtype, chunk_steps=4, pick=fragile_rows)
    check_rows(tracker.lifecycle(flag, field, g["wrow"]), want)                        # a resident call afterwards
    # the C entry itself: a reader that returns 1 on the second chunk
    import ctypes as C
    L = _native.lib()
    T, ny, nx = flag.shape
    calls = []

    def raw(src, ctype):
        def rd(_user, t0, nt, dst):
            calls.append(t0)
            if t0 >= 4 and ctype is C.c_int32:
                return 1
            np.ctypeslib.as_array(C.cast(dst, C.POINTER(ctype)), shape=(nt, ny, nx))[...] = src[t0:t0 + nt]
            return 0
        return _native.READ_CHUNK_FN(rd)
    n, nex = C.c_int64(-1), C.c_int64(-1)
    wrow = np.ascontiguousarray(g["wrow"], dtype=np.float32)
    rc = L.ctk_lifecycle_stream_cb(tracker.handle, 4, T, ny, nx, raw(flag, C.c_int32), None, raw(field, C.c_float), None, wrow.ctypes.data, 4,
                                   _native.LIFE_PICK_FN(), None, C.byref(n), C.byref(nex))
    assert rc == -1 and b"reader" in L.ctk_last_error()                                # CTK_E_INVALID
    with pytest.raises(_native.ContrackHipError):
        tracker.debug_lifecycle_path(T)                                                # no finished call
    check_rows(tracker.lifecycle(flag, field, g["wrow"]), want)

    def bad_pick(rows):
        if rows["t"].min() >= 4:
            raise KeyError("pick")
        return fragile_rows(rows)
    with pytest.raises(KeyError):
        tracker.lifecycle_stream(flag, field, g["wrow"], chunk_steps=4, pick=bad_pick)
    rc = L.ctk_lifecycle_stream_f32(tracker.handle, flag.ctypes.data, np.ascontiguousarray(field).ctypes.data, T, ny, nx, wrow.ctypes.data, 4,
                                    _native.LIFE_PICK_FN(lambda user, rows, nrows, idx, nidx: 1), None, C.byref(n), C.byref(nex))
    assert rc == -1 and b"pick" in L.ctk_last_error()
    rows = tracker.lifecycle(flag, field, g["wrow"])
    check_rows(rows, want)
    assert lifecycle_frame(rows, g["lat"], g["lon"], dates, tracker) == frame
    # picks that are not ascending indices of the chunk's rows are refused, not followed
    for chosen in ([1, 0], [10 ** 6], [-1]):
        with pytest.raises(ValueError):
            tracker.lifecycle_stream(flag, field, g["wrow"], chunk_steps=4, pick=lambda rows: chosen)


def test_exact_after_a_streamed_call_is_a_state_error(tracker):
    from contrack_amd import _native
    g, dates, want, frame = golden("refslab")
    rows, idx, ex = tracker.lifecycle_stream(g["flag"], g["variable"], g["wrow"], chunk_steps=4, pick=fragile_rows)
    with pytest.raises(_native.ContrackHipError, match="stream"):
        tracker.lifecycle_exact(np.arange(len(rows)))
    again = tracker.lifecycle(g["flag"], g["variable"], g["wrow"])                     # works again after the next resident call
    check_rows(again, rows)
    got = tracker.lifecycle_exact(idx)                                                 # the same rows, the same summation orders: the same bits
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(got[k], ex[k]), k


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_degenerate_inputs(tracker, dtype):
    wrow = np.ones(5, dtype=np.float32)
    for T in (0, 3):
        flag = np.zeros((T, 5, 8), dtype=np.int32)
        rows, idx, ex = tracker.lifecycle_stream(flag, np.ones((T, 5, 8), dtype=dtype), wrow, chunk_steps=2, pick=fragile_rows)
        assert len(rows) == 0 and len(idx) == 0 and len(ex) == 0
        path, steps = tracker.debug_lifecycle_path(T)
        assert steps.tolist() == [0] * T
    # no pick: no rows are picked
    g, dates, want, frame = golden("smooth0")
    rows, idx, ex = tracker.lifecycle_stream(g["flag"], g["variable"], g["wrow"], chunk_steps=5)
    check_rows(rows, want)
    assert len(idx) == 0 and len(ex) == 0
