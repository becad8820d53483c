"""Everything a handle takes from the GPU goes back with it: ctk_debug_live (device buffers, pinned buffers, events, streams held by
the owners of csrc/ctk_own.h in this process) reads the same after Tracker.close() as before Tracker(), after a handle that ran
every written sequence of tests/handle_sequences.py (which reach every entry family but the time-shard path, the band and centred
families included), once more a streamed band and a streamed centred call on inputs of their own, and one call of the time-shard
path -- and after a handle that ran nothing.  Other handles of the process (module fixtures of other test files) may be alive meanwhile: only differences are
compared.  Every call is also compared with its family's reference, exactly."""
import gc

import numpy as np
import pytest

import band_util as bu
import centred_util as cu
import handle_sequences as hs
from contrack_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def oracle_built(oracle_lib):
    return oracle_lib


def _band(trk):
    """streamed, with a field and sectors, three chunks: the pinned twins and both table sets"""
    key = hs.SMALLEST
    T, ny, nx = hs.SHAPES[key]
    flag, x, w = hs.flags(key), hs.slab(key), bu.cos_weights(ny)
    sects = [(0, 10), (nx - 6, 12)]                                         # the second one wraps
    got = trk.band(flag, (1, ny - 2), w, x, sects, chunk_steps=T // 3)
    bu.same(got, bu.band(flag, 1, ny - 2, w, x=x, sects=sects), "band")


def _centred(trk):
    x, t, row, col, bin = cu.wide_case(np.float32)
    gs, gn = trk.centred(x, t, row, col, bin, 3, 2, 3, chunk_steps=5)
    ws, wn = cu.centred(x, t, row, col, bin, 3, 2, 3)
    assert np.array_equal(gn, wn) and cu.same_bits(gs, ws)


def _one_rank_time_shard(trk):
    key = hs.SMALLEST
    T, ny, nx = hs.SHAPES[key]
    a = hs.slab(key)
    want, nw = hs.want_track(key)
    grp = _native.CommGroup(1)
    comm = _native.Comm.local(trk, grp, 0)
    d_in, d_out = trk.malloc(a.nbytes), trk.malloc(a.size * 4)
    try:
        trk.h2d(d_in, a)
        n = trk.track_sharded_dev(comm, d_in, T, 0, T, ny, nx, hs.thresholds(key, 100.0), 0, hs.wrow(key), hs.OVERLAP, 2, hs.TWOSIDED, d_out)
        f = np.empty((T, ny, nx), np.int32)
        trk.d2h(f, d_out)
    finally:
        comm.close()                                                        # (before the counters are read again)
        grp.close()
        trk.free(d_in)
        trk.free(d_out)
    assert np.array_equal(f, want) and n == nw


def test_a_used_handle_and_an_unused_one_give_everything_back():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    gc.collect()                                                            # (no forgotten handle of an earlier test goes meanwhile)
    before = _native.debug_live()
    trk = _native.Tracker(0)
    try:
        for sequence in hs.WRITTEN:
            bad = hs.run_sequence(trk, sequence())
            assert not bad, (sequence.__name__, bad)
        _band(trk)
        _centred(trk)
        key = hs.SMALLEST
        bad = hs.run_sequence(trk, [hs.track_field(key), hs.track_stream(key, chunk_steps=5, callbacks=True), hs.track(key), hs.release_io(), hs.track(key)])
        assert not bad, bad
        _one_rank_time_shard(trk)
        during = _native.debug_live()
        assert during[0] > before[0] and during[1] > before[1] and during[2] > before[2] and during[3] >= before[3] + 3, (before, during)
    finally:
        trk.close()
    assert _native.debug_live() == before
    _native.Tracker(0).close()                                              # created and closed with no call in between
    assert _native.debug_live() == before
