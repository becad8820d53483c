"""The numpy statement of ctk_blockstat_* (include/contrack_hip.h): what every GPU result must equal exactly.  The reference has no
function for this step, so this loop is what every layer is pinned against.  All of it is integers and selected values: there is no
tolerance, the two floats of a row compare bit for bit.

The key of an entry is a ROW table as tests/subset_util.py states it: off int64 with T + 1 entries from 0 to len(ids), ids int32,
all > 0 and strictly increasing inside a step's slice.  For entry e = (t, id), P is the pixels of step t with flag == id in
row-major order, and the row holds

    n              |P| (uint32); 0: the entry matched nothing and every other value is its empty value
    r0, r1         the lowest and highest grid row of P                                      (empty: -1, -1)
    west, width    from occ[c] = some pixel of P lies in column c: all columns occupied gives 0, nx.  Otherwise take the maximal
                   CIRCULAR runs of unoccupied columns (a run may pass the seam; its start s is the column whose western neighbour,
                   modulo nx, is occupied), the longest of them and among equally long ones the lowest s:
                   west = (s + len) % nx, width = nx - len                                   (empty: -1, 0)
    nv             the pixels of P whose value is not NaN
    max, max_p     the largest of those values in the total order -inf < ... < -0.0 < +0.0 < ... < +inf (an_key, ctk_select.h), as
                   float64 (a float32 value widens exactly), and the lowest pixel index row * nx + col that holds exactly it
    min, min_p     the same at the other end, again the lowest index                         (nv == 0: NaN, NaN, -1, -1)

The column rule is deliberately one of its own: it is NOT the life cycle's `shift`, which copies the reference's non-circular
np.argmax(np.diff(cols)).  What `want` does not ask for ('shape': r0 .. width, 'peaks': nv .. min) holds its empty value."""
import numpy as np

SHAPE, PEAKS = 1, 2

ROW = np.dtype([("n", np.uint32), ("nv", np.uint32), ("r0", np.int32), ("r1", np.int32), ("west", np.int32), ("width", np.int32),
                ("max_p", np.int64), ("min_p", np.int64), ("max", np.float64), ("min", np.float64)], align=True)


def key(v):
    """the order-preserving integer of a float32 / float64 value (an_key), as a Python int"""
    v = np.asarray(v)
    bits = 32 if v.dtype == np.float32 else 64
    u = int(v.view(np.uint32 if bits == 32 else np.uint64))
    top = 1 << (bits - 1)
    return ((1 << bits) - 1) ^ u if u & top else u | top


def extent(occ):
    """(west, width) of a boolean column occupancy with at least one column set"""
    nx = len(occ)
    if occ.all():
        return 0, nx
    best_len, best_s = 0, -1
    for s in range(nx):                                           # rising s: an equally long later run does not replace
        if occ[s] or not occ[(s - 1) % nx]:
            continue
        ln = 0
        while not occ[(s + ln) % nx]:
            ln += 1
        if ln > best_len:
            best_len, best_s = ln, s
    return (best_s + best_len) % nx, nx - best_len


def empty_rows(n):
    rows = np.zeros(n, dtype=ROW)
    rows["r0"] = rows["r1"] = rows["west"] = rows["max_p"] = rows["min_p"] = -1
    rows["max"] = rows["min"] = np.nan
    return rows


def blockstat(flag, x, off, ids, want=SHAPE | PEAKS):
    """the rows of the table's entries, one pixel at a time"""
    flag = np.asarray(flag, dtype=np.int32)
    T, ny, nx = flag.shape
    off, ids = np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int32)
    assert len(off) == T + 1 and off[0] == 0 and off[-1] == len(ids) and (np.diff(off) >= 0).all()
    assert want in (SHAPE, PEAKS, SHAPE | PEAKS) and (x is not None or not want & PEAKS)
    if x is not None:
        x = np.asarray(x)
        assert x.shape == flag.shape and x.dtype in (np.float32, np.float64)
    rows = empty_rows(len(ids))
    for t in range(T):
        s = ids[off[t]:off[t + 1]].astype(np.int64)
        assert (s > 0).all() and (np.diff(s) > 0).all()
        f = flag[t].reshape(-1)
        for k, i in enumerate(s):
            r = rows[off[t] + k]
            P = np.flatnonzero(f == i)
            r["n"] = len(P)
            if not len(P):
                continue
            if want & SHAPE:
                r["r0"], r["r1"] = P.min() // nx, P.max() // nx
                occ = np.zeros(nx, dtype=bool)
                occ[P % nx] = True
                r["west"], r["width"] = extent(occ)
            if want & PEAKS:
                v = x[t].reshape(-1)
                hi = lo = None
                for p in P:                                       # rising p: an equal key later does not replace
                    if v[p] != v[p]:
                        continue
                    r["nv"] += 1
                    kp = key(v[p])
                    if hi is None or kp > hi[0]:
                        hi = (kp, p)
                    if lo is None or kp < lo[0]:
                        lo = (kp, p)
                if hi is not None:
                    r["max"], r["max_p"], r["min"], r["min_p"] = np.float64(v[hi[1]]), hi[1], np.float64(v[lo[1]]), lo[1]
    return rows


def same_rows(got, want):
    """equality field by field, the two floats by their bits (NaN equals NaN, -0.0 differs from +0.0)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    for name in ROW.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype != ROW[name] or b.dtype != ROW[name]:
            return False
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            return False
    return True


def diff_rows(got, want):
    """the first few (entry, field, got, want) that differ: the text of a failing assertion"""
    out = []
    for e in range(min(len(got), len(want))):
        for name in ROW.names:
            a, b = got[name][e], want[name][e]
            if (a.tobytes() if hasattr(a, "tobytes") else a) != (b.tobytes() if hasattr(b, "tobytes") else b):
                out.append((e, name, a, b))
    return out[:8]
