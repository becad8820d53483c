"""The seam stage of the one-call pass (k_fz_mark / k_fz_rank_mark, k_fz_groups, k_seam_driver) on the constructed slabs of
tests/seam_forms.py, each of which sits on one edge of that code: 8 / 9 operations of a cluster (own slots or shared tail), 64 / 65
labels, the hook's caps, folds through 63 operations, clusters over two and three 64-step windows, 512 / 513 records of a window,
64 / 65 / 130 records of a chunk and of a step, groups across the 64-row lanes, crowded LDS hashes, a full tail, roots beyond the
ids that own slots, seam rows of a filtered component, T = 1 .. 5.

Every case: flags and n bit-identical to the C oracle; fused_pass and off_fused_path_reason what the design says (0; 512 for a
cluster beyond the driver's tables; 256 for a full tail); seam_ops and seam_rows_to_driver the restated counts; a second call on
the same handle the same flags (fused after a 256, not after a 512); the same flags from the synchronous resolver and from the
host resolver.  tests/test_seam_forms_host.py shows on the CPU that the slabs have the designed counts."""
import numpy as np
import pytest

import seam_forms as sm
from contrack_amd import _native

pytestmark = pytest.mark.gpu

OP = _native.CMP_OPS[">="]


def _need_gpu():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")


def _track(t, k):
    flag, n = t.track(k.field(), k.thr(), OP, k.wrow(), k.overlap, k.pers, True)
    return flag.copy(), int(n)


def _same(got, n, want, nw, what):
    assert np.array_equal(got, want), "%s: flag differs at %d pixels" % (what, int((got != want).sum()))
    assert n == nw, (what, n, nw)


@pytest.fixture(scope="module")
def sync_trk():
    _need_gpu()
    t = _native.Tracker(0)
    t.set_fused(False)
    yield t
    t.close()


@pytest.fixture(scope="module")
def host_trk():
    _need_gpu()
    t = _native.Tracker(0)
    t.set_device_resolve(False)
    yield t
    t.close()


@pytest.mark.parametrize("name", sm.NAMES)
def test_fused_pass(oracle_lib, name):
    """a fresh handle per case (CTK_POISON_CLUSTER is remembered for the grid): two calls"""
    _need_gpu()
    k, dr = sm.case(name), sm.driven(name)
    want, nw = sm.oracle_result(oracle_lib, name)
    with _native.Tracker(0) as t:
        if k.caps:
            t.debug_set_seam_caps(*k.caps)
        got, n = _track(t, k)
        st = t.stats()
        got2, n2 = _track(t, k)
        st2 = t.stats()
    seen = lambda s: dict(fused_pass=s["fused_pass"], reason=s["off_fused_path_reason"], seam_ops=s["seam_ops"], records=s["seam_rows_to_driver"])
    print("SEAMFORM %s design %s first %s second %s" % (name, sm.design(name), seen(st), seen(st2)))
    _same(got, n, want, nw, "first call")
    _same(got2, n2, want, nw, "second call")
    assert st["off_fused_path_reason"] == k.expect and st["fused_pass"] == (1 if k.expect == 0 else 0), seen(st)
    assert st["host_path"] == 0 and st2["host_path"] == 0
    # on the fused path both are sums of the count kernel (t_nops / rec_cnt); off it the synchronous resolver's k_rs_cand_groups
    # groups by the same rule and SeamDriver::run counts its own operations
    for s in (st, st2):
        assert s["seam_ops"] == len(dr.ops), seen(s)
        assert s["seam_rows_to_driver"] == len(dr.records), seen(s)
    if k.expect == sm.REASON_CLUSTER:
        assert st2["fused_pass"] == 0, seen(st2)                   # this grid: the host driver from now on
    else:
        assert st2["fused_pass"] == 1 and st2["off_fused_path_reason"] == 0, seen(st2)


@pytest.mark.parametrize("name", sm.NAMES)
def test_synchronous_and_host_resolver(oracle_lib, sync_trk, host_trk, name):
    """set_fused(False): k_rs_cand_mark / k_rs_cand_groups and the host's SeamDriver::run do the work.  k_rs_cand_groups groups the
    seam rows by the rule of k_fz_groups (same label pair, consecutive rows, a same-label row only of a marked label), so the record
    count is asserted there too.  set_device_resolve(False): ctk_resolve.cpp works row by row and reports no record count; its
    operations (the same inflow rule) are counted."""
    k, dr = sm.case(name), sm.driven(name)
    want, nw = sm.oracle_result(oracle_lib, name)
    got, n = _track(sync_trk, k)
    st = sync_trk.stats()
    _same(got, n, want, nw, "synchronous resolver")
    assert st["fused_pass"] == 0 and st["host_path"] == 0
    assert st["seam_ops"] == len(dr.ops) and st["seam_rows_to_driver"] == len(dr.records), (st["seam_ops"], st["seam_rows_to_driver"])
    got, n = _track(host_trk, k)
    st = host_trk.stats()
    _same(got, n, want, nw, "host resolver")
    assert st["fused_pass"] == 0 and st["host_path"] == 1
    assert st["seam_ops"] == len(dr.ops), st["seam_ops"]


@pytest.mark.parametrize("name", ["d_ladder_tall_63", "e_windows_129"])
def test_device_entry_twice(oracle_lib, name):
    """ctk_track_dev on device buffers, twice on one handle: the second call is the speculative one sized by the first"""
    _need_gpu()
    k, dr = sm.case(name), sm.driven(name)
    want, nw = sm.oracle_result(oracle_lib, name)
    a = k.field()
    T, ny, nx = a.shape
    with _native.Tracker(0) as t:
        d_in, d_out = t.malloc(a.nbytes), t.malloc(a.size * 4)
        try:
            t.h2d(d_in, a)
            for call in range(2):
                t.memset(d_out, 0xff, a.size * 4)
                n = t.track_dev(d_in, T, ny, nx, k.thr(), OP, k.wrow(), k.overlap, k.pers, True, d_out)
                got = np.empty(a.shape, dtype=np.int32)
                t.d2h(got, d_out)
                st = t.stats()
                _same(got, int(n), want, nw, "call %d" % call)
                assert st["fused_pass"] == 1 and st["off_fused_path_reason"] == 0
                assert st["seam_ops"] == len(dr.ops) and st["seam_rows_to_driver"] == len(dr.records)
        finally:
            t.free(d_in)
            t.free(d_out)
