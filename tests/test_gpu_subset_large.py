"""ctk_subset_dev in place past 2^31 and 2^32 elements, on the shape of tests/test_gpu_consumers_large.py: 4200 x 721 x 1440 (4.36 G
elements, 17.4 GB).  The slab is large_util.flag_spec -- ids 1..3 on a few patches of four windows of 24 steps, A wholly below element
2^31, B across it, C across element 2^32, D the last steps -- placed with one memset and four copies.  A row table keeps ids 1 and 3 in
the steps of A and D only, a by-id table keeps ids 2 and 3 everywhere; the four windows are downloaded and compared with the statement
(tests/subset_util.py) on the compact windows, the planes beside them are zero, and the whole slab holds as many non-zero words as
the statement's windows.  hits equal the statement's on the compact windows.  One device slab, ~0.5 GB of host memory."""
import numpy as np
import pytest

import large_util as lu
import subset_util as su
from contrack_amd import _native

pytestmark = pytest.mark.gpu

L = lu.LAYOUT_FULL
T, NY, NX, NPIX = L.T, L.ny, L.nx, L.npix
SLAB = T * NPIX * 4


@pytest.fixture(scope="module")
def big():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    trk = _native.Tracker(0)
    try:
        p = trk.malloc(SLAB)
    except MemoryError as e:
        trk.close()
        pytest.fail("the slab needs %.1f GB of device memory: %s" % (SLAB / 1e9, e))
    yield trk, p, lu.flag_spec(L)
    trk.free(p)
    trk.close()


def row_tables(spec):
    """(the table over all T steps, the same over the compact steps): ids 1 and 3 at every step of windows A and D"""
    keep = set()
    for t0 in (L.firsts[0], L.firsts[3]):
        keep |= set(range(t0, t0 + L.n))
    full = su.table_by_row([[1, 3] if t in keep else [] for t in range(T)])
    compact = su.table_by_row([[1, 3] if t in keep else [] for t in spec.steps()])
    assert np.array_equal(full[1], compact[1]) and len(full[1]) == 4 * L.n
    return full, compact


def check_windows(trk, p, spec, want, case):
    plane = NPIX * 4
    k, zero_steps, inside = 0, {0, T - 1}, set()
    for t0, w in spec.windows:
        got = np.empty_like(w)
        trk.d2h(got, lu._off(p, t0 * plane))
        assert np.array_equal(got, want[k:k + len(w)]), (case, "window at step", t0, int(np.count_nonzero(got != want[k:k + len(w)])))
        k += len(w)
        zero_steps |= {t0 - 1, t0 + len(w)}
        inside |= set(range(t0, t0 + len(w)))
    one = np.empty((NY, NX), dtype=np.int32)
    for t in sorted(t for t in zero_steps if 0 <= t < T and t not in inside):
        trk.d2h(one, lu._off(p, t * plane))
        assert not one.any(), (case, "background step", t)
    nz = int(np.count_nonzero(want))
    assert nz > 0 and trk.checksum_i32(p, T * NPIX, 0)[1] == nz, (case, nz)


def test_rows_of_two_windows_in_place(big):
    trk, p, spec = big
    assert T * NPIX > 2 ** 32 and L.firsts[1] * NPIX < 2 ** 31 < (L.firsts[1] + L.n) * NPIX and L.firsts[2] * NPIX < 2 ** 32 < (L.firsts[2] + L.n) * NPIX
    full, compact = row_tables(spec)
    cf, steps = spec.compact()
    want = su.subset_fast(cf, *compact)
    a, d = slice(0, L.n), slice(3 * L.n, 4 * L.n)
    assert want[0][a].any() and want[0][d].any() and not want[0][L.n:3 * L.n].any() and (want[0] == 2).sum() == 0 and want[1].all()
    lu.place(trk, p, spec)
    hits, n = trk.subset_dev(p, T, NY, NX, full, None)                          # count only: the slab stays
    assert np.array_equal(hits, want[1]) and n == want[2]
    assert trk.checksum_i32(p, T * NPIX, 0)[1] == int(np.count_nonzero(cf))
    hits, n = trk.subset_dev(p, T, NY, NX, full, p)
    assert trk.debug_subset_launch()[:2] == (_native.SUBSET_FORMS.index("row_lds"), 1)
    assert np.array_equal(hits, want[1]) and n == want[2]
    check_windows(trk, p, spec, want[0], "rows")


@pytest.mark.parametrize("hits", [False, True], ids=["bitmap", "search"])
def test_tracks_in_place_with_invert(big, hits):
    trk, p, spec = big
    table = su.table_by_id([2, 3])
    cf, steps = spec.compact()
    want = su.subset_fast(cf, *table, invert=hits)
    assert all(want[0][k * L.n:(k + 1) * L.n].any() for k in range(4)) and 0 < want[2] < np.count_nonzero(cf)
    lu.place(trk, p, spec)
    got_hits, n = trk.subset_dev(p, T, NY, NX, table, p, invert=hits, want_hits=hits)
    assert trk.debug_subset_launch()[:2] == (_native.SUBSET_FORMS.index("search_lds" if hits else "bitmap"), 1)
    assert n == want[2] and (got_hits is None or np.array_equal(got_hits, want[1]))
    check_windows(trk, p, spec, want[0], ("tracks", hits))
