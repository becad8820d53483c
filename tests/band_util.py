"""The contract of the reductions over space per time step (ctk_band_*, contrack.band_numpy) as numpy loops.

Per step t and column c over the rows [y0, y1) of an integer flag slab (T, ny, nx), float64 row weights w[ny], optionally a field x:
    cnt[t, c]  = #{y : flag[t, y, c] > above}                                              (uint32)
    area[t, c] = from +0.0, for y RISING:  s = s + (w[y] if flag[t, y, c] > above else 0.0)   (float64)
    wx[t, c]   = the same walk with the float64 product w[y] * float64(x[t, y, c])
and per sector (x0, len) -- the columns x0, x0 + 1, ... modulo nx -- the column values added in that order from +0.0.  A value of x
at an unflagged pixel reaches no output.  The vectorised rules below are what the GPU is compared with, bit for bit; the naive triple
loops pin the vectorised ones (tests/test_band_host.py)."""
import numpy as np


def order_weights(ny):
    """[1e16, 1.0, -1e16, 1.0, ...]: a sum of these in another order has other bits"""
    return np.array([(1e16, 1.0, -1e16, 1.0)[y % 4] for y in range(ny)], dtype=np.float64)


def cos_weights(ny):
    """the float32 area weights of a regular grid from pole to pole (pole rows slightly negative in float32), widened to float64"""
    lat = np.linspace(-90.0, 90.0, ny) if ny > 1 else np.array([52.5])
    d = 180.0 / max(ny - 1, 1)
    return (111 * d * 111 * d * np.cos(lat * np.pi / 180)).astype(np.float32).astype(np.float64)


def columns(flag, y0, y1, w, above=0, x=None):
    """dict(cnt, area[, wx]) of (T, nx) arrays: a loop over y of vectorised additions"""
    flag = np.asarray(flag)
    w = np.asarray(w, dtype=np.float64)
    T, ny, nx = flag.shape
    assert 0 <= y0 < y1 <= ny and w.shape == (ny,)
    m = flag > above
    cnt = np.zeros((T, nx), dtype=np.uint32)
    area = np.zeros((T, nx), dtype=np.float64)
    wx = None if x is None else np.zeros((T, nx), dtype=np.float64)
    xd = None if x is None else np.asarray(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(y0, y1):
            cnt += m[:, y].astype(np.uint32)
            area = area + np.where(m[:, y], w[y], 0.0)
            if wx is not None:
                wx = wx + np.where(m[:, y], w[y] * xd[:, y].astype(np.float64), 0.0)
    out = dict(cnt=cnt, area=area)
    if wx is not None:
        out["wx"] = wx
    return out


def sectors(cols, sects):
    """dict(sec_cnt, sec_area[, sec_wx]) of (T, nsect) arrays from the column tables: a loop over the columns of every sector"""
    T, nx = cols["cnt"].shape
    sects = [(int(a), int(b)) for a, b in sects]
    out = dict(sec_cnt=np.zeros((T, len(sects)), dtype=np.uint32), sec_area=np.zeros((T, len(sects)), dtype=np.float64))
    if "wx" in cols:
        out["sec_wx"] = np.zeros((T, len(sects)), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, (x0, ln) in enumerate(sects):
            assert 0 <= x0 < nx and 1 <= ln <= nx
            for k in range(ln):
                c = (x0 + k) % nx
                out["sec_cnt"][:, s] += cols["cnt"][:, c]
                out["sec_area"][:, s] = out["sec_area"][:, s] + cols["area"][:, c]
                if "wx" in cols:
                    out["sec_wx"][:, s] = out["sec_wx"][:, s] + cols["wx"][:, c]
    return out


def band(flag, y0, y1, w, above=0, x=None, sects=None, want_columns=True):
    """what band_numpy returns: the column tables (want_columns) and, with sectors, the sector tables"""
    cols = columns(flag, y0, y1, w, above, x)
    out = dict(cols) if want_columns else {}
    if sects is not None and len(sects):
        out.update(sectors(cols, sects))
    return out


def band_total(w, y0, y1, sects=None, nx=None):
    """the same rule with every pixel flagged -- the denominator of a fraction: the float64 sum of w[y0:y1] in rising y (a scalar: every
    column has it), or with sectors (and nx) the (nsect,) sums of that value over each sector's columns in order"""
    w = np.asarray(w, dtype=np.float64)
    col = np.float64(0.0)
    for y in range(y0, y1):
        col = col + w[y]
    if sects is None:
        return col
    out = np.zeros(len(sects), dtype=np.float64)
    for s, (x0, ln) in enumerate(sects):
        assert 0 <= x0 < nx and 1 <= ln <= nx
        for _ in range(int(ln)):
            out[s] = out[s] + col
    return out


# ---- the naive triple loops -------------------------------------------------------------------------------------------------------
def columns_naive(flag, y0, y1, w, above=0, x=None):
    flag = np.asarray(flag)
    T, ny, nx = flag.shape
    cnt = np.zeros((T, nx), dtype=np.uint32)
    area = np.zeros((T, nx), dtype=np.float64)
    wx = None if x is None else np.zeros((T, nx), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            for c in range(nx):
                n, s, sx = 0, np.float64(0.0), np.float64(0.0)
                for y in range(y0, y1):
                    if flag[t, y, c] > above:
                        n += 1
                        s = s + np.float64(w[y])
                        if x is not None:
                            sx = sx + np.float64(w[y]) * np.float64(x[t, y, c])
                cnt[t, c], area[t, c] = n, s
                if x is not None:
                    wx[t, c] = sx
    out = dict(cnt=cnt, area=area)
    if wx is not None:
        out["wx"] = wx
    return out


def sectors_naive(cols, sects):
    T, nx = cols["cnt"].shape
    out = dict(sec_cnt=np.zeros((T, len(sects)), dtype=np.uint32), sec_area=np.zeros((T, len(sects)), dtype=np.float64))
    if "wx" in cols:
        out["sec_wx"] = np.zeros((T, len(sects)), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            for s, (x0, ln) in enumerate(sects):
                n, a, sx = 0, np.float64(0.0), np.float64(0.0)
                for k in range(int(ln)):
                    c = (int(x0) + k) % nx
                    n += int(cols["cnt"][t, c])
                    a = a + cols["area"][t, c]
                    if "wx" in cols:
                        sx = sx + cols["wx"][t, c]
                out["sec_cnt"][t, s], out["sec_area"][t, s] = n, a
                if "wx" in cols:
                    out["sec_wx"][t, s] = sx
    return out


# ---- comparison and test data -------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what=""):
    """every table of `want` is in `got` with the same dtype, shape and bits (NaNs compared by bits too), and nothing else is"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, k, int(np.count_nonzero(bits(g) != bits(w))))


def flags(shape, density, seed=0):
    """int32 ids 1..999 at about `density` of the pixels, 0 elsewhere (density 0: none, 1: all)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 1000, size=shape).astype(np.int32)
    return np.where(rng.random(shape) < density, ids, 0).astype(np.int32)


def field(shape, dtype, seed=0):
    rng = np.random.default_rng(seed + 1000)
    return (rng.standard_normal(shape) * 150).astype(dtype)
