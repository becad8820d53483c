"""The blocked-spell entries without a GPU: declared in the headers, exported by the library build() cross-compiles, bound in
_native.EXPORTS; the numpy statement of the definition (spell_util) against the known answers of the definition and against an
independent formulation; the pure parts of the Python side (mean duration, argument checks before a device is touched)."""
import importlib
import os
import re

import numpy as np
import pytest

import freq_util
import spell_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ENTRIES = ("ctk_spells_dev", "ctk_spells", "ctk_spells_cb")
DEBUG = ("ctk_debug_set_spell", "ctk_debug_time_spell")

# one pixel, above = 0: (by_id, min_duration, segment starts) -> (events, steps, longest)
SERIES = (0, 3, 3, 0, 3, 5, 5, 0)
KNOWN = (((1, 1, None), (3, 5, 2)),
         ((0, 1, None), (2, 5, 3)),
         ((1, 2, None), (2, 4, 2)),
         ((1, 1, (0, 2)), (4, 5, 2)))


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, header)).read(), flags=re.S)
    return set(re.findall(r"^\s*int\s+(ctk_\w+)\s*\(", text, flags=re.M))


def test_entries_declared_exported_and_bound():
    lib = _native.lib()
    for header, names in (("contrack_hip.h", ENTRIES), ("contrack_hip_debug.h", DEBUG)):
        declared = _declared(header)
        for name in names:
            assert name in declared, name
            assert hasattr(lib, name), name
            assert name in _native.EXPORTS, name
            assert getattr(lib, name).argtypes is not None, name
    for name in ("spells", "spells_cb", "spells_dev", "set_spell_debug", "time_spells"):
        assert callable(getattr(_native.Tracker, name)), name
    import contrack_amd
    assert contrack_amd.spells_numpy is cm.spells_numpy and contrack_amd.spell_duration is cm.spell_duration
    assert callable(cm.contrack.calc_spells)


@pytest.mark.parametrize("args,want", KNOWN)
def test_known_answers(args, want):
    by_id, min_duration, segments = args
    flag = np.array(SERIES, dtype=np.int32).reshape(8, 1, 1)
    for fn in (spell_util.spells, spell_util.spells_diff):
        got = fn(flag, None, 1, 0, bool(by_id), min_duration, segments)
        assert tuple(int(a[0, 0, 0]) for a in got) == want, (fn.__name__, args)


def test_onset_group_and_slab_end():
    """a spell belongs to the group of its first step even when it runs on into another group; one cut by the end counts"""
    flag = np.array([0, 1, 1, 1, 0, 2, 2], dtype=np.int32).reshape(7, 1, 1)
    ids = np.array([0, 0, 1, 1, 1, 1, 0], dtype=np.int32)
    for fn in (spell_util.spells, spell_util.spells_diff):
        ev, st, lg = fn(flag, ids, 2)
        assert ev[:, 0, 0].tolist() == [1, 1] and st[:, 0, 0].tolist() == [3, 2] and lg[:, 0, 0].tolist() == [3, 2], fn.__name__


@pytest.mark.parametrize("seed", range(4))
def test_loop_agrees_with_run_boundaries(seed):
    T, ny, nx = 97, 3, 5
    flag = spell_util.spell_flags(T, ny, nx, seed)
    rng = np.random.default_rng(100 + seed)
    seg_sets = (None, [0], [0, 1, 40, 41, T - 1], np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), 9, replace=False))]))
    continued = 0
    for gname, ids, G in freq_util.groupings(T):
        for by_id in (True, False):
            for min_duration in (1, 2, 5):
                for above in (0, 2):
                    for segments in seg_sets:
                        a = spell_util.spells(flag, ids, G, above, by_id, min_duration, segments)
                        b = spell_util.spells_diff(flag, ids, G, above, by_id, min_duration, segments)
                        for x, y, what in zip(a, b, ("events", "steps", "longest")):
                            assert x.shape == (G, ny, nx) and np.array_equal(x, y), (what, gname, by_id, min_duration, above)
                        continued += int((a[2] > 1).sum())
    assert continued > 1000                                  # the generator makes runs that continue under by_id, too
    d = spell_util.spell_list(flag, 0, True)[1]
    assert (d >= 5).sum() > 20 and (d == 1).sum() > 20


def test_by_id_matters_in_generated_flags():
    flag = spell_util.spell_flags(97, 3, 5, 9)
    a, b = spell_util.spells(flag, by_id=True), spell_util.spells(flag, by_id=False)
    assert np.array_equal(a[1], b[1])                       # the same flagged steps ...
    assert (a[0] > b[0]).any() and (a[2] < b[2]).any()      # ... in more and shorter spells


def test_spell_duration():
    steps = np.array([[6, 0], [5, 7]])
    events = np.array([[4, 0], [5, 2]])
    got = cm.spell_duration(steps, events)
    assert got.dtype == np.float64
    assert np.isnan(got[0, 1]) and got[0, 0] == 1.5 and got[1, 0] == 1.0 and got[1, 1] == 3.5
    assert np.isnan(cm.spell_duration(np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64))).all()
    big = np.array([2 ** 40 + 1]), np.array([3])
    assert freq_util.same_bits(cm.spell_duration(*big), big[0].astype(np.float64) / big[1].astype(np.float64))


BAD = [dict(min_duration=0), dict(min_duration=-3), dict(min_duration=1.5), dict(by_id=2), dict(by_id=-1), dict(by_id="yes"),
       dict(segments=[1, 4]), dict(segments=[0, 4, 4]), dict(segments=[0, 5, 3]), dict(segments=[0, 8]), dict(segments=[0, -2]),
       dict(segments=[]), dict(segments=[[0, 2]]), dict(segments=[0.0, 2.0]),
       dict(group=np.array([0, 1, 2, 0, 1, 2, 0, -1])), dict(group=np.zeros(7, np.int32)), dict(group=np.zeros(8)),
       dict(group=np.array([0] * 7 + [2 ** 32], np.int64)), dict(above=2 ** 31), dict(chunk_steps=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[repr(sorted(b.items())[0][0]) + str(i) for i, b in enumerate(BAD)])
def test_wrappers_reject_before_a_device_is_touched(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(cm, "_tracker", no_device)
    flag = np.zeros((8, 2, 3), dtype=np.int32)
    with pytest.raises(ValueError):
        cm.spells_numpy(flag, **bad)
    with pytest.raises(ValueError):
        cm.spells_numpy(lambda t0, nt, out: None, shape=flag.shape, **bad)


def test_wrappers_reject_bad_slabs(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(cm, "_tracker", no_device)
    with pytest.raises(ValueError):
        cm.spells_numpy(np.zeros((8, 2), dtype=np.int32))
    with pytest.raises(ValueError):
        cm.spells_numpy(np.zeros((8, 2, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        cm.spells_numpy(np.zeros((0, 2, 3), dtype=np.int32))
    with pytest.raises(ValueError):
        cm.spells_numpy(lambda t0, nt, out: None)                        # a reader without a shape
    with pytest.raises(ValueError):
        _native._spell_args(2 ** 32)                                      # durations are uint32
    with pytest.raises(ValueError):
        _native._spell_args(8, np.array([0, 1, 2, 3, 0, 1, 2, 3]), 3)    # a group out of range
    g, G, st, by, md = _native._spell_args(8, np.array([0, 1, 2, 3, 0, 1, 2, 3]), None, [0, 5], True, np.int64(2))
    assert g.dtype == np.int32 and G == 4 and st.dtype == np.int64 and st.tolist() == [0, 5] and by == 1 and md == 2
    assert _native._spell_args(8) == (None, 1, None, 1, 1)
