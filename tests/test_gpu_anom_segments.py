"""calc_clim / calc_anom over independent time segments on the GPU, resident (ctk_anom_seg_*) and streamed (ctk_anom_stream_*),
against oracle/anom_port.py used as it is: the climatology of the whole slab, then the port's calc_anom on every segment [s, e) with
that climatology, concatenated.  Everything is compared bit for bit (np.array_equal with equal_nan, equal dtypes), the standard of
tests/test_gpu_anom.py; no tolerance appears."""
import numpy as np
import pytest

from contrack_amd import _native
from contrack_amd.contrack import anomalies_numpy
from oracle import anom_port

from anom_forms import expected, same                # (the yardstick, shared with tests/test_gpu_anom_seg_forms.py)

pytestmark = pytest.mark.gpu

RING, PLAIN = 1, 0                 # Tracker.debug_anom_form: CtkAnomForm of csrc/ctk_forms.h
BIG_SMOOTH = 40                    # beyond the LDS ring of either dtype (float32: 32 steps, float64: 16)


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def _field(rng, T, ny, nx, dtype, nans):          # (the recipe of tests/test_gpu_anom.py)
    x = (50.0 * rng.standard_normal((T, ny, nx)) + 5500.0 + 30.0 * np.sin(np.arange(T) * 2 * np.pi / 365.0)[:, None, None]).astype(dtype)
    if nans:
        x[rng.random(x.shape) < 0.01] = np.nan
        x[:, 0, 0] = np.nan                      # a grid point without data
    return x


def _groups(T, ngroups=12, run=3):
    """ids that change every `run` steps, from an offset that puts the boundaries off the round numbers the tests break at"""
    return (((np.arange(T) + 17) // run) % ngroups).astype(np.int32), ngroups


# ---- 1. one segment is ctk_anom_*, bit for bit, in both kernel forms ---------------------------------------------------------
@pytest.mark.parametrize("case", [(120, 5, 8, np.float32, 0), (200, 13, 37, np.float32, 1), (90, 9, 16, np.float64, 1)], ids=str)
def test_one_segment_is_the_unsegmented_call(trk, case):
    T, ny, nx, dtype, nans = case
    x = _field(np.random.default_rng(T), T, ny, nx, dtype, nans)
    group, G = _groups(T, ngroups=40)
    forms = set()
    for window in (1, 4, 31):
        for smooth in (1, 2, 3, 5, 16, BIG_SMOOTH):
            want, want_c = expected(x, group, G, window, smooth, [0])
            plain, clim = trk.anomalies(x, group, G, window=window, smooth=smooth, want_clim=True)
            assert same(plain, want) and same(clim, want_c), (window, smooth, "unsegmented")        # (ctk_anom_* is the same host path)
            for seg in ([0], []):
                got, gclim = trk.anomalies(x, group, G, window=window, smooth=smooth, want_clim=True, segments=seg)
                form = trk.debug_anom_form()
                assert form == (PLAIN if smooth == BIG_SMOOTH else RING), (smooth, form)
                forms.add(form)
                assert same(got, want) and same(gclim, want_c), (window, smooth, seg)
                assert same(got, plain) and same(gclim, clim), (window, smooth, seg)
    assert forms == {RING, PLAIN}


# ---- 2. segment edges -----------------------------------------------------------------------------------------------------------
STARTS = [0, 1, 7, 8, 30, 59]      # T = 60: lengths 1, 6, 1, 22, 29, 1 -- a break at t = 1 and at t = T - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nans", [0, 1])
def test_segment_edges(trk, dtype, nans):
    T, ny, nx = 60, 13, 37                        # 481 pixels: the second workgroup is partial
    x = _field(np.random.default_rng(7 + nans), T, ny, nx, dtype, nans)
    group, G = _groups(T)
    assert any(group[s] == group[s - 1] for s in STARTS[1:])          # breaks inside a run of one group
    for smooth in (1, 2, 4, 5, 16, BIG_SMOOTH):
        got, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=STARTS)
        want, want_c = expected(x, group, G, 4, smooth, STARTS)
        assert same(clim, want_c) and same(got, want), smooth
        if nans:
            continue
        edges = STARTS + [T]
        for s, e in zip(edges[:-1], edges[1:]):
            bad = np.isnan(got[s:e]).all(axis=(1, 2))
            assert np.array_equal(np.isnan(got[s:e]).any(axis=(1, 2)), bad)
            if e - s < smooth:
                assert bad.all()                                      # a segment shorter than the window
            else:
                lead, tail = smooth // 2, (smooth - 1) // 2            # one more at the start for an even window
                assert bad[:lead].all() and bad[e - s - tail:].all() and not bad[lead:e - s - tail].any(), (smooth, s, e)
    one = trk.anomalies(x, group, G, window=4, smooth=1, segments=STARTS)[0]
    if not nans:
        assert not np.isnan(one).any()                                # segments of length 1 are valid with smooth = 1
    # the array-level entry
    a, c = anomalies_numpy(x, group, window=4, smooth=5, segments=STARTS)
    want, want_c = expected(x, group, G, 4, 5, STARTS)
    assert same(a, want) and same(c, want_c)


# ---- 3. streamed equals resident ------------------------------------------------------------------------------------------------
SEG3 = [0, 11, 12, 37]


@pytest.fixture(scope="module")
def slabs():
    out = {}
    for dtype, (T, ny, nx) in ((np.float32, (50, 13, 37)), (np.float64, (50, 5, 8))):
        x = _field(np.random.default_rng(11), T, ny, nx, dtype, 1)
        group, G = _groups(T)
        out[np.dtype(dtype).name] = (x, group, G)
    return out


@pytest.mark.parametrize("smooth", [1, 2, 5, 16, BIG_SMOOTH])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_streamed_equals_resident(trk, slabs, dt, smooth):
    x, group, G = slabs[dt]
    T = x.shape[0]
    res, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=SEG3)
    want, want_c = expected(x, group, G, 4, smooth, SEG3)
    assert same(res, want) and same(clim, want_c)
    for chunk in sorted({1, max(smooth - 1, 1), smooth, 7, T, T + 5}):
        a, c = trk.anomalies_stream(x, group, G, window=4, smooth=smooth, chunk_steps=chunk, segments=SEG3, want_clim=True)
        assert same(a, res) and same(c, clim), ("array", chunk)
        reads, writes = [], []
        out = np.full_like(x, -1.0)

        def reader(t0, nt, dst):
            reads.append((t0, nt))
            dst[...] = x[t0:t0 + nt]

        def writer(t0, nt, src):
            writes.append((t0, nt))
            out[t0:t0 + nt] = src
        _, c = trk.anomalies_stream(reader, group, G, window=4, smooth=smooth, sink=writer, shape=x.shape, dtype=x.dtype, chunk_steps=chunk,
                                    segments=SEG3, want_clim=True)
        assert same(out, res) and same(c, clim), ("callbacks", chunk)
        limit = max(chunk, smooth - 1)                                # (a chunk below smooth - 1 is raised to it)
        half = len(reads) // 2
        for one_pass in (reads[:half], reads[half:]):                 # two passes: increasing, no overlap, every step once
            assert [t for t, _ in one_pass] == list(np.cumsum([0] + [n for _, n in one_pass[:-1]]))
            assert sum(n for _, n in one_pass) == T and all(0 < n <= limit for _, n in one_pass)
        assert [t for t, _ in writes] == list(np.cumsum([0] + [n for _, n in writes[:-1]])) and sum(n for _, n in writes) == T
        # with a climatology handed in: one pass
        reads.clear()
        a, _ = trk.anomalies_stream(reader, group, G, window=4, smooth=smooth, clim=clim, shape=x.shape, dtype=x.dtype, chunk_steps=chunk, segments=SEG3)
        assert same(a, res) and sum(n for _, n in reads) == T and [t for t, _ in reads] == sorted(t for t, _ in reads)
    # no segments: the unsegmented resident call
    assert same(trk.anomalies_stream(x, group, G, window=4, smooth=smooth, chunk_steps=7)[0], trk.anomalies(x, group, G, window=4, smooth=smooth)[0])
    a, c = anomalies_numpy(x, group, window=4, smooth=smooth, segments=SEG3, chunk_steps=7)
    assert same(a, res) and same(c, clim)


def test_climatology_only_stream(trk, slabs):
    x, group, G = slabs["float32"]
    a, c = trk.anomalies_stream(x, group, G, window=4, sink=False, chunk_steps=6, want_clim=True)
    assert a is None and same(c, anom_port.calc_clim(x, group, G, 4).astype(np.float32))


def test_raising_callbacks_surface_and_the_tracker_goes_on(trk, slabs):
    x, group, G = slabs["float32"]
    calls = []

    def reader(t0, nt, dst):
        calls.append(t0)
        if len(calls) == 3:
            raise RuntimeError("reader gave up")
        dst[...] = x[t0:t0 + nt]
    with pytest.raises(RuntimeError, match="reader gave up"):
        trk.anomalies_stream(reader, group, G, smooth=3, shape=x.shape, dtype=x.dtype, chunk_steps=8)

    def writer(t0, nt, src):
        raise KeyError("writer gave up")
    with pytest.raises(KeyError):
        trk.anomalies_stream(x, group, G, smooth=3, sink=writer, chunk_steps=8)
    want, _ = expected(x, group, G, 1, 3, [0])
    assert same(trk.anomalies_stream(x, group, G, smooth=3, chunk_steps=8)[0], want)


# ---- 4. invalid starts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [[1, 5], [0, 5, 5], [0, 9, 4], [0, 50], [0, 20, 53]], ids=str)
def test_invalid_starts(trk, slabs, bad):
    x, group, G = slabs["float32"]                                   # T = 50
    with pytest.raises(ValueError, match="segment"):                # (CTK_E_INVALID)
        trk.anomalies(x, group, G, smooth=2, segments=bad)
    with pytest.raises(ValueError, match="segment"):
        trk.anomalies_stream(x, group, G, smooth=2, chunk_steps=9, segments=bad)
    want, _ = expected(x, group, G, 1, 2, [0, 20])
    assert same(trk.anomalies(x, group, G, smooth=2, segments=[0, 20])[0], want)
    assert same(trk.anomalies_stream(x, group, G, smooth=2, chunk_steps=9, segments=[0, 20])[0], want)
