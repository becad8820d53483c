"""numpy statement of the blocked spells per grid point (ctk_spells*, contrack.calc_spells) for the spell tests.  At pixel p, step t
CONTINUES step t - 1 iff
    t is not a segment start  and  flag[t-1, p] > above  and  flag[t, p] > above  and  (by_id: flag[t-1, p] == flag[t, p])
A spell is a maximal chain of continuing steps that starts at a step with flag > above; its duration is its number of steps, its
group is the group of its first step; the spells with duration >= min_duration are counted:
    events[g, p] their number, steps[g, p] the sum of their durations, longest[g, p] the longest (0: none)
`spell_list` is a plain loop over pixels and steps (the shapes of the tests are tiny; clarity counts more than speed) and `maps_of`
puts its spells on the three maps, so that tests which vary only the grouping and min_duration walk the slab once; `spells_diff` finds
the run boundaries with np.diff instead and shares no code with them."""
import numpy as np


def _starts(segments, T):
    brk = np.zeros(T, dtype=bool)
    brk[0] = True                                           # step 0 is always a start
    if segments is not None:
        brk[np.asarray(segments, dtype=np.int64)] = True
    return brk


def spell_list(flag, above=0, by_id=True, segments=None):
    """every spell of the slab, whatever its duration: int64 arrays (onset step, duration, y, x)"""
    flag = np.asarray(flag)
    T, ny, nx = flag.shape
    brk = _starts(segments, T).tolist()
    found = []
    for y in range(ny):
        for x in range(nx):
            s = flag[:, y, x].tolist()
            onset, d = 0, 0                                 # the open spell: its first step and its duration so far (0: none)
            for t in range(T):
                on = s[t] > above
                cont = t > 0 and not brk[t] and s[t - 1] > above and on and (not by_id or s[t - 1] == s[t])
                if cont:
                    d += 1
                    continue
                if d:
                    found.append((onset, d, y, x))
                onset, d = (t, 1) if on else (0, 0)
            if d:                                           # cut by the end of the slab: counts with the length it has
                found.append((onset, d, y, x))
    a = np.array(found, dtype=np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def maps_of(spell_list_, shape, ids=None, G=1, min_duration=1):
    """(events, steps, longest), int64 (G, ny, nx), of the listed spells that last min_duration steps or more, each in the group of
    its onset"""
    onset, d, y, x = spell_list_
    keep = d >= min_duration
    onset, d, y, x = onset[keep], d[keep], y[keep], x[keep]
    g = np.zeros(onset.shape, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)[onset]
    ev, st, lg = (np.zeros((G,) + tuple(shape[1:]), dtype=np.int64) for _ in range(3))
    np.add.at(ev, (g, y, x), 1)
    np.add.at(st, (g, y, x), d)
    np.maximum.at(lg, (g, y, x), d)
    return ev, st, lg


def spells(flag, ids=None, G=1, above=0, by_id=True, min_duration=1, segments=None):
    """(events, steps, longest), int64 (G, ny, nx)"""
    flag = np.asarray(flag)
    return maps_of(spell_list(flag, above, by_id, segments), flag.shape, ids, G, min_duration)


def spells_diff(flag, ids=None, G=1, above=0, by_id=True, min_duration=1, segments=None):
    """the same from run boundaries: per pixel, a key series that changes exactly where a spell cannot continue -- 0 where the pixel
    is unflagged, else (segment number, id or 1) -- and np.diff over it"""
    flag = np.asarray(flag)
    T, ny, nx = flag.shape
    seg_no = np.cumsum(_starts(segments, T)).astype(np.int64)                 # 1, 1, ..., 2, 2, ...
    gid = np.zeros(T, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    ev, st, lg = (np.zeros((G, ny, nx), dtype=np.int64) for _ in range(3))
    for y in range(ny):
        for x in range(nx):
            s = flag[:, y, x].astype(np.int64)
            on = s > above
            ident = s - above if by_id else np.ones(T, dtype=np.int64)        # > 0 where on, distinct per id
            key = np.where(on, seg_no * (2 ** 33) + ident, 0)
            edge = np.concatenate([[True], np.diff(key) != 0])                # a new run (flagged or not) starts here
            first = np.nonzero(edge)[0]
            length = np.diff(np.concatenate([first, [T]]))
            keep = on[first] & (length >= min_duration)
            for t0, d in zip(first[keep], length[keep]):
                g = gid[t0]
                ev[g, y, x] += 1
                st[g, y, x] += d
                lg[g, y, x] = max(lg[g, y, x], d)
    return ev, st, lg


def spell_flags(T, ny, nx, seed, ids=3, p_change=0.15):
    """an int32 flag slab in which spells happen: per pixel, unflagged and flagged runs of geometric lengths (means drawn from 3..6
    steps) alternate; the ids of a flagged run come from the small set 1..ids, with an occasional change of id inside the run (a
    continuing run under by_id=False that is cut under by_id=True)"""
    rng = np.random.default_rng(seed)
    flag = np.zeros((T, ny, nx), dtype=np.int32)
    for y in range(ny):
        for x in range(nx):
            t = 0
            on = bool(rng.integers(0, 2))
            mean_on, mean_off = rng.integers(3, 7, 2)
            while t < T:
                n = int(rng.geometric(1.0 / (mean_on if on else mean_off)))
                if on:
                    cur = int(rng.integers(1, ids + 1))
                    for u in range(t, min(T, t + n)):
                        if u > t and rng.random() < p_change:
                            cur = int(rng.integers(1, ids + 1))
                        flag[u, y, x] = cur
                t += n
                on = not on
    return flag
