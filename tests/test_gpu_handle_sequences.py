"""One handle, every entry family, in the orders a script could choose (tests/handle_sequences.py): the written sequences run in file
order on ONE module-scoped Tracker -- the handle is as old as the module can make it -- and the seeded sequences share another.  Every
operation of every sequence is compared with the reference of its family's own test, exactly; after every tracking operation the
handle's ambiguous_decisions is 0; after every operation the capacities of the four shared staging buffers (ctk_debug_io_bytes) are
what the sequences' size model says the handle asked for; at the end a plain track of a golden case still equals its golden flag.

exact_rows_follow_their_slabs is the test of ctk_lifecycle_exact's staleness rule (include/contrack_hip.h): the exact rows of a
host-array lifecycle call are refused with the state error once a later call has written or released the handle's staging buffers
(or, for field = None, the resident anomaly slab), and are right again after the next lifecycle call."""
import numpy as np
import pytest

import golden_util
import handle_sequences as hs
from contrack_amd import _native

pytestmark = pytest.mark.gpu


def _tracker():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    return _native.Tracker(0)


@pytest.fixture(scope="module")
def trk():
    t = _tracker()
    yield t
    t.close()


@pytest.fixture(scope="module")
def seeded_trk():
    t = _tracker()
    yield t
    t.close()


@pytest.fixture(scope="module", autouse=True)
def oracle_built(oracle_lib):
    return oracle_lib


def _run(trk, ops):
    bad = hs.run_sequence(trk, ops)
    assert not bad, "\n".join(repr(b) for b in bad)              # (one failure per line, none cut short)


@pytest.mark.parametrize("sequence", hs.WRITTEN, ids=[f.__name__ for f in hs.WRITTEN])
def test_written_sequence(trk, sequence):
    _run(trk, sequence())


def test_stale_exact_rows_name_their_cause(trk):
    """the message of the state error, and that a lifecycle call of the caller's own device slabs is not subject to the rule"""
    key = hs.SMALLEST
    T, ny, nx = hs.SHAPES[key]
    flag, field = hs.life_flag(key), hs.slab(key)
    rows = trk.lifecycle(flag, field, hs.wrow(key))
    trk.frequency(hs.flags(key))
    with pytest.raises(_native.ContrackHipError, match="overwrote or released") as e:
        trk.lifecycle_exact(np.arange(len(rows)))
    assert not isinstance(e.value, ValueError)
    d_flag, d_field = trk.malloc(flag.nbytes), trk.malloc(field.nbytes)
    try:
        trk.h2d(d_flag, flag)
        trk.h2d(d_field, field)
        rows = trk.lifecycle_dev(d_flag, d_field, T, ny, nx, hs.wrow(key))
        trk.frequency(hs.flags(key))                                        # the handle's buffers are not where these slabs live
        ex = trk.lifecycle_exact(np.arange(len(rows)))
    finally:
        trk.free(d_flag)
        trk.free(d_field)
    want = hs.want_life(flag, field, key)
    assert hs.same_life((rows, ex), want)


@pytest.mark.parametrize("seed", range(hs.N_SEEDS))
def test_seeded_sequence(seeded_trk, seed):
    _run(seeded_trk, hs.seeded(seed))


@pytest.mark.parametrize("which", ["written", "seeded"])
def test_old_handles_still_track_a_golden(trk, seeded_trk, which):
    t = trk if which == "written" else seeded_trk
    g = golden_util.load("refslab_two")
    flag, n = t.track(g["anom"], g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    assert np.array_equal(flag, g["flag"]) and n == len(np.unique(g["flag"])) - 1
    assert t.stats()["ambiguous_decisions"] == 0
