"""Loader for tests/golden/life/*.npz (written by tests/golden/make_life_golden.py from the reference's own
run_lifecycle) and a numpy builder of ctk_life_row records used to test the host-side finishing step without a GPU."""
import glob
import os

import numpy as np

LIFE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "life")


def case_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(LIFE_DIR, "*.npz")))


def load(name):
    z = np.load(os.path.join(LIFE_DIR, name + ".npz"))
    if "field_ref" in z:
        field = np.load(os.path.join(os.path.dirname(LIFE_DIR), str(z["field_ref"])))["anom"].astype(np.float32)
    elif "field64" in z:
        field = np.array(z["field64"], dtype=np.float64)
    else:
        field = (z["field_q"] / 8.0).astype(np.float32)
    variable = (z["variable_q"] / 8.0).astype(np.float32) if "variable_q" in z else field
    time = z["time"].astype("datetime64[h]").astype("datetime64[ns]")
    frame = list(zip((int(v) for v in z["Flag"]), (str(v) for v in z["Date"]), (int(v) for v in z["Longitude"]),
                     (int(v) for v in z["Latitude"]), (float(v) for v in z["Intensity"]), (float(v) for v in z["Size"])))
    return dict(name=name, field=field, variable=variable, flag=np.array(z["flag"], dtype=np.int32), lat=z["lat"], lon=z["lon"],
                wrow=np.array(z["wrow"], dtype=np.float32), time=time, frame=frame)


def dates_of(time):
    import pandas as pd
    return [pd.Timestamp(v).strftime('%Y%m%d_%H') for v in time]


def numpy_rows(flags, field, wrow):
    """What ctk_lifecycle_* returns, evaluated with numpy (float64 sums in raster order)."""
    from contrack_amd._native import LIFE_ROW
    T, ny, nx = flags.shape
    w = np.asarray(wrow, dtype=np.float32).astype(np.float64)[:, None] * np.ones((1, nx))
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = []
    for t in range(T):
        for ident in np.unique(flags[t]):
            if ident == 0:
                continue
            m = flags[t] == ident
            shift = -1
            if m[:, 0].any() and m[:, -1].any():
                cols = np.unique(np.nonzero(m)[1])
                shift = int(cols[np.argmax(np.diff(cols)) + 1]) if len(cols) > 1 else -2
            xr = (xx - shift) % nx if shift > 0 else xx
            wv = field[t].astype(np.float64) * w
            out.append((t, int(ident), shift, 0, w[m].sum(), wv[m].sum(), (wv * yy)[m].sum(), (wv * xr)[m].sum()))
    rows = np.array(out, dtype=LIFE_ROW) if out else np.empty(0, dtype=LIFE_ROW)
    return rows[np.lexsort((rows["t"], rows["label"]))]


def random_life_case(i):
    """random label planes (blobs, some joined across the seam, ids not contiguous, sometimes negative) and a positive
    field: (flag, field, lat, lon, wrow, dates)"""
    from scipy import ndimage
    from contrack_amd.contrack import row_weights
    rng = np.random.default_rng(90000 + i)
    T = int(rng.integers(1, 7)); ny = int(rng.integers(3, 40)); nx = int(rng.choice([4, 7, 16, 33, 64, 65, 100, 130]))
    # labelled blobs: threshold a smooth-ish random field, label with wrap-unaware scipy, then join ids across the seam at random
    f = ndimage.uniform_filter(rng.standard_normal((T, ny, nx)), size=(1, 3, 5), mode=("nearest", "nearest", "wrap"))
    flag = np.zeros((T, ny, nx), np.int32)
    for t in range(T):
        lab, n = ndimage.label(f[t] > 0.15)
        perm = rng.permutation(np.arange(1, n + 1)) * int(rng.choice([1, 1, 7])) if n else np.array([], int)
        flag[t] = np.where(lab > 0, np.concatenate([[0], perm])[lab], 0)
        for y in range(ny):                                  # merge across the seam sometimes
            if flag[t, y, 0] and flag[t, y, -1] and rng.random() < 0.7:
                flag[t][flag[t] == flag[t, y, -1]] = flag[t, y, 0]
    if rng.random() < 0.2:
        flag[flag == flag.max()] = -5                            # a negative id
    f64 = bool(rng.integers(0, 2))
    field = (rng.random((T, ny, nx)) * 50 + 100).astype(np.float64 if f64 else np.float32)
    lat = np.linspace(90, -90, ny).astype(np.float32); lon = (np.arange(nx) * (360.0 / nx)).astype(np.float32)
    wrow = row_weights(lat, 180.0 / (ny - 1), 360.0 / nx)
    dates = ["%02d" % t for t in range(T)]
    return flag, field, lat, lon, wrow, dates


def numpy_exact_rows(flags, field, wrow, rows, extent=False):
    """what ctk_lifecycle_exact returns for `rows`, evaluated with the reference's own calls: np.sum for the area and the
    intensity numerator (contrack.py:874-875), np.bincount (what ndimage.center_of_mass sums with, :886 / :892) on the rolled plane.
    extent: evaluate on the id's row extent only -- the same elements added in the same order (the roll moves whole rows' columns,
    the other rows add only to bincount's bin 0), so bit for bit the same, and far cheaper on large planes"""
    from contrack_amd._native import LIFE_EXACT
    T, ny, nx = flags.shape
    wgrid_all = np.ones((ny, nx)) * np.asarray(wrow, dtype=np.float32)[:, None]
    yy_all, xx = np.mgrid[0:ny, 0:nx]
    out = np.zeros(len(rows), dtype=LIFE_EXACT)
    for i, r in enumerate(rows):
        plane, values, wgrid, yy = flags[r["t"]], field[r["t"]], wgrid_all, yy_all
        if extent:
            ys = np.nonzero((plane == r["label"]).any(axis=1))[0]
            band = slice(ys[0], ys[-1] + 1)
            plane, values, wgrid, yy = plane[band], values[band], wgrid_all[band], yy_all[band]
        m = plane == r["label"]
        sh = int(r["shift"]) if r["shift"] > 0 else 0
        pr, vr = np.roll(plane, -sh, axis=1), np.roll(values, -sh, axis=1)
        inp = vr * wgrid
        sel = (pr == r["label"]).ravel().astype(np.intp)
        out[i] = (np.sum(wgrid[m]), np.sum(wgrid[m] * values[m]), np.bincount(sel, weights=inp.ravel())[1],
                  np.bincount(sel, weights=(inp * yy.astype(float)).ravel())[1], np.bincount(sel, weights=(inp * xx[:len(plane)].astype(float)).ravel())[1])
    return out


# ---------------------------------------------------------------------------------------------------------------
# large contours: numpy's np.sum tree, and label planes holding ids with prescribed pixel counts
# ---------------------------------------------------------------------------------------------------------------
NP_BLOCK = 8192          # numpy's buffered reduction hands its inner loop 8192 elements at a time and adds the results in order
NP_LEAF = 128            # pairwise_sum halves a block until a part has <= 128 elements


def np_leaves(n):
    """(offset, length) of the leaves of numpy's pairwise float64 add.reduce over n contiguous elements, in the order they are
    summed: blocks of NP_BLOCK one after the other, each halved (n2 = n / 2 - (n / 2) % 8) down to parts of <= NP_LEAF"""
    out = []

    def split(off, m):
        if m <= NP_LEAF:
            out.append((off, m))
            return
        m2 = m // 2 - (m // 2) % 8
        split(off, m2)
        split(off + m2, m - m2)
    for b0 in range(0, n, NP_BLOCK):
        split(b0, min(NP_BLOCK, n - b0))
    return out


def _np_leaf_sum(a):
    """pairwise_sum on <= 128 elements: a plain loop below 8, else eight running sums (np.cumsum is a running sum) combined
    as a tree, and the rest added one by one"""
    if len(a) < 8:
        r = 0.0
        for v in a:
            r += float(v)
        return r
    m = len(a) - len(a) % 8
    r = [float(v) for v in np.cumsum(a[:m].reshape(-1, 8), axis=0)[-1]]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[m:]:
        res += float(v)
    return res


def np_tree_sum(a, block=NP_BLOCK):
    """numpy's float64 np.sum restated on the tree of np_leaves; block=None: one unblocked pairwise tree over all of a"""
    a = np.asarray(a, dtype=np.float64)

    def pw(lo, m):
        if m <= NP_LEAF:
            return _np_leaf_sum(a[lo:lo + m])
        m2 = m // 2 - (m // 2) % 8
        return pw(lo, m2) + pw(lo + m2, m - m2)
    if block is None:
        return pw(0, len(a)) if len(a) else 0.0
    acc = 0.0
    for b0 in range(0, len(a), block):
        acc += pw(b0, min(block, len(a) - b0))
    return acc


def seq_sum(a):
    """strictly sequential float64 sum (np.bincount's order)"""
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def leaf_lengths(count, lo=1, hi=NP_BLOCK):
    """the block lengths in lo..hi whose tree has `count` leaves"""
    return [n for n in range(lo, hi + 1) if len(np_leaves(n)) == count]


def sweep_lengths():
    """every length 7600..8192: all 441 block lengths with 65 leaves (7689..8191) and their neighbours"""
    return list(range(7600, NP_BLOCK + 1))


def edge_lengths():
    """the edges of the sequential sums' blocks (256 / 512 values) and of the leaf loop"""
    return [1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 511, 512, 513]


def round_lengths():
    """8192 k + r: one to four groups of the 1024-thread launch busy, a partial last round, many rounds; r = 7689 / 8191 are
    tails with 65 leaves"""
    return [NP_BLOCK * k + r for k in (1, 2, 3, 4, 12) for r in (0, 1, 7689, 8191)]


GRIDS = {"1deg": (181, 360), "0.25deg": (721, 1440)}


def grid_of(name):
    """(lat, lon, wrow) of a regular global grid: (ny, nx) or a name in GRIDS"""
    from contrack_amd.contrack import row_weights
    ny, nx = GRIDS[name] if isinstance(name, str) else name
    lat = np.linspace(90, -90, ny).astype(np.float32)
    lon = (np.arange(nx) * (360.0 / nx)).astype(np.float32)
    return lat, lon, row_weights(lat, 180.0 / (ny - 1), 360.0 / nx)


def _place_raster(lengths, ny, nx, rng):
    """raster-contiguous runs starting mid-row: (plane, flat start) per id"""
    npx, out, plane, pos = ny * nx, [], 0, 0
    for L in lengths:
        if L > npx:
            raise ValueError("an id of %d pixels does not fit a %d x %d plane" % (L, ny, nx))
        off = int(rng.integers(1, nx)) if L < npx else 0
        if pos + off + L > npx:
            plane, pos = plane + 1, 0
            off = off if off + L <= npx else 0
        out.append((plane, np.arange(pos + off, pos + off + L)))
        pos += off + L
    return out


def _place_band(lengths, ny, nx, rng):
    """bands of columns across the seam, filled row by row (the last row partial), one below the other: the columns never
    all occupied, so the roll shift is the band's first column (> 1) and the rolled order differs from the raster order"""
    out, plane, y = [], 0, 0
    for L in lengths:
        wd = int(rng.integers(max(2, nx // 2), nx - 1))
        c0 = nx - int(rng.integers(1, wd))                   # the band runs c0 .. nx-1, 0 .. wd - (nx - c0) - 1
        rows = -(-L // wd)
        if rows > ny:
            raise ValueError("an id of %d pixels does not fit a band of %d columns" % (L, wd))
        if y + rows > ny:
            plane, y = plane + 1, 0
        k = np.arange(L)
        out.append((plane, (y + k // wd) * nx + (c0 + k % wd) % nx))
        y += rows
    return out


def _place_full(lengths, ny, nx, rng):
    """full-height bands: every row, the pole rows included (pixels of row y: L // ny, one more in the first L % ny rows),
    side by side; the first one of a plane across the seam (when it is two columns wide or more)"""
    out, plane, used = [], 0, None
    for L in lengths:
        q, r = divmod(L, ny)
        wd = q + (r > 0)
        if wd > nx - 1:
            raise ValueError("an id of %d pixels is wider than the plane" % L)
        if used is not None and used + wd > nx - 1:
            plane, used = plane + 1, None
        if used is None:
            used, c = 0, nx - max(1, wd // 2)
        ys = np.repeat(np.arange(ny), [q + (y < r) for y in range(ny)])
        xs = np.concatenate([np.arange(q + (y < r)) for y in range(ny)]) if len(ys) else ys
        out.append((plane, ys * nx + (c + xs) % nx))
        c, used = (c + wd) % nx, used + wd
    return out


def large_life_case(lengths, grid="1deg", kind="raster", dtype=np.float32, positive=False, seed=0):
    """label planes holding one id per entry of `lengths` with exactly that many pixels (an id need not be connected for
    run_lifecycle), and a field of standard_normal x 10^U(-6, 6) of both signs (positive: its magnitude), on which the order of a
    sum changes its result.  kind: 'raster' (runs starting mid-row, spanning rows: both seam columns, shift 1), 'band' (columns
    across the seam, shift > 1), 'full' (full-height bands, pole rows included).  An id of a whole plane is its own plane.
    -> dict(flag, field, lat, lon, wrow, ids, lengths)"""
    rng = np.random.default_rng(seed)
    lat, lon, wrow = grid_of(grid)
    ny, nx = len(lat), len(lon)
    place = dict(raster=_place_raster, band=_place_band, full=_place_full)[kind]
    where = place(list(lengths), ny, nx, rng)
    T = max(p for p, _ in where) + 1
    flag = np.zeros((T, ny * nx), np.int32)
    ids = []
    for i, (p, px) in enumerate(where):
        ident = (3 * i + 2) * (-1 if i % 5 == 4 else 1)        # neither contiguous nor all positive
        assert not flag[p, px].any()
        flag[p, px] = ident
        ids.append(ident)
    field = rng.standard_normal((T, ny * nx)) * 10.0 ** rng.uniform(-6, 6, (T, ny * nx))
    if positive:
        field = np.abs(field)
    return dict(flag=flag.reshape(T, ny, nx), field=field.reshape(T, ny, nx).astype(dtype), lat=lat, lon=lon, wrow=wrow,
                ids=np.array(ids), lengths=np.array(lengths))
