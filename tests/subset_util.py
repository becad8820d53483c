"""The numpy statement of ctk_subset_* (include/contrack_hip.h): what every GPU result must equal exactly.  All values are integers,
there is no tolerance.

A table is (off, ids): off int64, ids int32.  By id: off = [0, K], the K ids > 0 and strictly increasing, for every step.  By row:
off has T + 1 entries from 0 to len(ids), non-decreasing; ids[off[t]:off[t + 1]] are the ids wanted at step t, > 0 and strictly
increasing inside the slice."""
import numpy as np

ID, MASK = 0, 1


def table_by_id(ids):
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    return np.array([0, len(ids)], dtype=np.int64), ids


def table_by_row(slices):
    """slices: one sequence of ids per step"""
    off = np.zeros(len(slices) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in slices])
    ids = np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1) for s in slices]) if len(slices) else np.empty(0, dtype=np.int32)
    return off, ids.astype(np.int32)


def check_table(off, ids, T):
    off, ids = np.asarray(off), np.asarray(ids)
    assert len(off) in (2, T + 1) and off[0] == 0 and off[-1] == len(ids) and (np.diff(off) >= 0).all()
    for t in range(len(off) - 1):
        s = ids[off[t]:off[t + 1]].astype(np.int64)
        assert (s > 0).all() and (np.diff(s) > 0).all()


def subset(flag, off, ids, invert=False, kind=ID):
    """(out int32 like flag, hits uint64 [len(ids)], n_selected) -- one pixel at a time, as the header states it"""
    flag = np.asarray(flag, dtype=np.int32)
    T = flag.shape[0]
    check_table(off, ids, T)
    out = np.zeros_like(flag)
    hits = np.zeros(len(ids), dtype=np.uint64)
    n_selected = 0
    for t in range(T):
        i0, i1 = (int(off[0]), int(off[1])) if len(off) == 2 else (int(off[t]), int(off[t + 1]))
        entry = {int(v): i0 + k for k, v in enumerate(ids[i0:i1])}
        f, o = flag[t].reshape(-1), out[t].reshape(-1)
        for p in np.flatnonzero(f > 0):
            e = entry.get(int(f[p]))
            if e is not None:
                hits[e] += np.uint64(1)
            if (e is None) == bool(invert):
                o[p] = f[p] if kind == ID else 1
                n_selected += 1
    return out, hits, n_selected


def subset_fast(flag, off, ids, invert=False, kind=ID):
    """the same with array expressions (np.isin per slice, np.searchsorted for the hits): for slabs the pixel loop is too slow for;
    tests/test_subset_host.py holds it against subset()"""
    flag = np.asarray(flag, dtype=np.int32)
    T = flag.shape[0]
    out = np.zeros_like(flag)
    hits = np.zeros(len(ids), dtype=np.uint64)
    n_selected = 0
    for t in range(T):
        i0, i1 = (int(off[0]), int(off[1])) if len(off) == 2 else (int(off[t]), int(off[t + 1]))
        s = np.asarray(ids[i0:i1], dtype=np.int32)
        f = flag[t]
        pos = f > 0
        found = pos & np.isin(f, s)
        if found.any():
            hits[i0:i1] += np.bincount(np.searchsorted(s, f[found]), minlength=i1 - i0).astype(np.uint64)
        sel = (pos & ~found) if invert else found
        out[t] = np.where(sel, f if kind == ID else 1, 0)
        n_selected += int(np.count_nonzero(sel))
    return out, hits, n_selected
