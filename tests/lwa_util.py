"""numpy statement of the finite-amplitude local wave activity (include/contrack_hip.h, the block above ctk_lwa_f32) and the case
builders of the LWA tests.  The reference has no function for it, so these loops are what the library is pinned against.

Row table (rows): one or two DOMAINS, each the row indices of one hemisphere sorted by |lat| (equator side first; an equator row in
both); W = rint(max(cos(lat), 0) * 2^30) uint32; q = max(cos(lat), 0) * dphi with dphi the trapezoid width of the row inside its
domain (radians); S = radius / cos(lat) on active rows (lo <= |lat| <= hi inside a requested domain), 0 elsewhere.
Per plane, per domain D = (d_0 .. d_{n-1}) and per active row j = d_p (from_table):
    cap_j = nx * sum_{p' >= p} W[d_p']                                         (Python integers)
    the domain's non-NaN pixels sorted by their integer key (key: a total order, -0.0 before +0.0); A = the cumulative uint64 sum
    of their W; Z_j = the value at the first place where A >= cap_j; no such place: Z_j = NaN and the output row is NaN
    a = sum_{p' >= p, z > Z_j} (float64(z) - float64(Z_j)) * q[d_p']            y = sum_{p' < p, z < Z_j} (float64(Z_j) - float64(z)) * q[d_p']
    both from +0.0, added in rising p', product and sum rounded separately
    out[j][c] = dtype((a + y) * S[j])   (part 1: a * S[j], part 2: y * S[j])
`pixel` is that loop for ONE output pixel in plain Python floats; from_table runs the same additions for all active rows and columns
of a domain at once, still one p' after the other (tests/test_lwa_host.py holds the two against each other)."""
import numpy as np

from level_util import bits, differing, same_bits          # noqa: F401  (NaN payloads are not compared)

PARTS = ('total', 'anticyclonic', 'cyclonic')


def key(v):
    """the order-preserving integer key of float32 / float64 values (an_key of csrc/ctk_select.h)"""
    v = np.ascontiguousarray(v)
    if v.dtype == np.float32:
        u = v.view(np.uint32)
        return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))
    u = v.view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(0x8000000000000000))


def rows(lat, lat_bounds=(30, 75), hemisphere='both', radius=6.371e6):
    """the row table as a dict (ndom, dom_off, dom_rows, active, W, q, S), row by row"""
    lat = np.asarray(lat, dtype=np.float64)
    ny = len(lat)
    cosl = np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    phi = np.deg2rad(np.abs(lat))
    W = np.rint(cosl * 2.0 ** 30).astype(np.uint32)
    q, S, active = np.zeros(ny), np.zeros(ny), np.zeros(ny, dtype=np.uint8)
    doms, given = [], set()
    for name, sign in (('north', 1.0), ('south', -1.0)):
        if hemisphere not in ('both', name):
            continue
        dom = sorted([j for j in range(ny) if sign * lat[j] >= 0], key=lambda j: (abs(lat[j]), j))
        n = len(dom)
        for p, j in enumerate(dom):
            if n == 1:
                d = 0.0
            elif p == 0:
                d = (phi[dom[1]] - phi[dom[0]]) / 2
            elif p == n - 1:
                d = (phi[dom[-1]] - phi[dom[-2]]) / 2
            else:
                d = (phi[dom[p + 1]] - phi[dom[p - 1]]) / 2
            if j not in given:
                q[j] = cosl[j] * d
                given.add(j)
            if lat_bounds[0] <= abs(lat[j]) <= lat_bounds[1]:
                active[j] = 1
                S[j] = np.float64(radius) / np.cos(np.deg2rad(lat))[j]
        doms.append(dom)
    off = [0]
    for dom in doms:
        off.append(off[-1] + len(dom))
    return dict(ndom=len(doms), dom_off=np.array(off, dtype=np.int32), dom_rows=np.array([j for dom in doms for j in dom], dtype=np.int32), active=active, W=W, q=q, S=S)


def domains(tab):
    return [[int(j) for j in tab["dom_rows"][tab["dom_off"][d]:tab["dom_off"][d + 1]]] for d in range(int(tab["ndom"]))]


def caps(tab, dom, nx):
    """cap of every position of the domain (Python integers)"""
    w = [int(tab["W"][j]) for j in dom]
    return [nx * sum(w[p:]) for p in range(len(dom))]


def contours(plane, tab, dom):
    """(Z of every position of the domain as plane.dtype -- NaN where unreachable --, the sorted keys, the cumulative areas)"""
    nx = plane.shape[1]
    vals = plane[dom, :].reshape(-1)
    w = np.repeat(tab["W"][dom].astype(np.uint64), nx)
    ok = ~np.isnan(vals)
    vals, w = vals[ok], w[ok]
    order = np.argsort(key(vals), kind='stable')
    vals, cum = vals[order], np.cumsum(w[order], dtype=np.uint64)
    Z = np.full(len(dom), np.nan, dtype=plane.dtype)
    for p, cap in enumerate(caps(tab, dom, nx)):
        i = int(np.searchsorted(cum, np.uint64(cap), side='left')) if cap < 2 ** 64 else len(cum)
        if i < len(cum):
            Z[p] = vals[i]
    return Z, key(vals), cum


def pixel(plane, tab, dom, p, c, Z):
    """(a, y) of column c of the active row at position p of the domain, in Python floats (float64), one term after the other"""
    a = y = 0.0
    Zd = float(Z)
    for pp, j in enumerate(dom):
        v = plane[j, c]
        qv = float(tab["q"][j])
        with np.errstate(invalid="ignore", over="ignore"):
            if pp >= p and v > Z:
                a = a + float(np.float64(v) - np.float64(Zd)) * qv
            elif pp < p and v < Z:
                y = y + float(np.float64(Zd) - np.float64(v)) * qv
    return a, y


def from_table(z, tab, part=0, return_ref=False):
    """the statement on a row table: z (steps, ny, nx) float32 / float64 -> out in z's dtype [, ref (steps, ny)]"""
    z = np.asarray(z)
    part = PARTS.index(part) if isinstance(part, str) else int(part)
    steps, ny, nx = z.shape
    out, ref = np.zeros_like(z), np.zeros((steps, ny), dtype=z.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for dom in domains(tab):
            pos = np.array([p for p, j in enumerate(dom) if tab["active"][j]], dtype=np.int64)
            if not len(pos):
                continue
            act = np.array(dom)[pos]
            S = tab["S"][act][:, None]
            for s in range(steps):
                Z = contours(z[s], tab, dom)[0][pos]                      # (n_act,)
                Zc, Zd = Z[:, None], Z.astype(np.float64)[:, None]
                a, y = np.zeros((len(pos), nx)), np.zeros((len(pos), nx))
                for pp, j in enumerate(dom):                              # in domain order
                    v = z[s, j][None, :]
                    vd, qv = v.astype(np.float64), np.float64(tab["q"][j])
                    pole = (pp >= pos)[:, None]
                    a = np.where(pole & (v > Zc), a + (vd - Zd) * qv, a)
                    y = np.where(~pole & (v < Zc), y + (Zd - vd) * qv, y)
                r = ((a + y, a, y)[part] * S).astype(z.dtype)
                r[np.isnan(Z)] = np.nan
                out[s, act] = r
                ref[s, act] = Z
    return (out, ref) if return_ref else out


def lwa(z, lat, lat_bounds=(30, 75), hemisphere='both', radius=6.371e6, part=0, return_ref=False):
    return from_table(z, rows(lat, lat_bounds, hemisphere, radius), part, return_ref)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def grid(step, rising=False):
    """global regular latitudes from the north pole down (rising: from the south pole up)"""
    lat = 90.0 - step * np.arange(int(round(180 / step)) + 1)
    return lat[::-1].copy() if rising else lat


def gaussian(n=48):
    """the latitudes of a Gaussian grid, from the north down: irregular, no pole and no equator row"""
    return np.rad2deg(np.arcsin(np.polynomial.legendre.leggauss(n)[0]))[::-1].copy()


def shuffled(lat, seed=0):
    """the same latitudes in a random order"""
    return np.asarray(lat)[np.random.default_rng(seed).permutation(len(lat))].copy()


def field(lat, nx, steps=4, seed=0, dtype=np.float32, noise=30.0):
    """a height field that falls polewards, 5700 - 800 sin^2(phi), with tilted planetary waves of 200, 67 and 40 m, a Gaussian ridge
    of 250 m per step near 55 degrees in either hemisphere, and `noise` m of weather (a grid of ONE column has no waves: there only
    noise above the difference of neighbouring rows displaces anything)"""
    rng = np.random.default_rng(seed)
    lat = np.asarray(lat, dtype=np.float64)
    phi, lam = np.deg2rad(lat)[None, :, None], (2 * np.pi * np.arange(nx) / nx)[None, None, :]
    z = 5700.0 - 800.0 * np.sin(phi) ** 2 + np.zeros((steps, 1, nx))
    for k in (1, 3, 5):
        z = z + 200.0 / k * np.cos(phi) * np.sin(k * lam + rng.uniform(0, 2 * np.pi, (steps, 1, 1)) + 3 * phi)
    for sign in (1.0, -1.0):
        lat0 = sign * rng.uniform(45, 65, (steps, 1, 1))
        lam0 = rng.uniform(0, 2 * np.pi, (steps, 1, 1))
        dl = np.angle(np.exp(1j * (lam - lam0)))
        z = z + 250.0 * np.exp(-((lat[None, :, None] - lat0) / 10.0) ** 2 - (dl / 0.5) ** 2)
    return (z + rng.normal(0.0, noise, z.shape)).astype(dtype)


def quantised(z, step=10.0):
    """z rounded to multiples of `step` m: long tie groups, so that caps fall inside them"""
    return (np.round(np.asarray(z, dtype=np.float64) / step) * step).astype(z.dtype)


def all_equal(lat, nx, steps=3, value=5500.0, dtype=np.float32):
    return np.full((steps, len(lat), nx), value, dtype=dtype)


def sprinkle(z, tab, values, share=0.05, seed=0, steps=None):
    """a copy of z with `share` of the pixels of the domains' rows of the steps `steps` (default: all) replaced by draws from `values`"""
    rng = np.random.default_rng(seed)
    z = z.copy()
    dom_rows = np.unique(tab["dom_rows"])
    for s in range(z.shape[0]) if steps is None else steps:
        hit = rng.random((len(dom_rows), z.shape[2])) < share
        vals = rng.choice(np.asarray(values, dtype=z.dtype), size=hit.shape)
        z[s, dom_rows] = np.where(hit, vals, z[s, dom_rows])
    return z


# ---- tables and fields made to order (the edge tests) ---------------------------------------------------------------------------------
def custom_table(lengths, active, W="cos", ny=None, shared=False):
    """a row table with the keys of rows() for one or two domains of the given lengths.  The first domain runs DOWN the rows from
    lengths[0] - 1 to 0 (its pole is row 0, as on a grid from the north), the second up from there on; shared: the second domain
    starts on the first row of the first, as the equator row does (inactive in both).  active[d]: the positions in domain d that
    are active.  Position p of n has phi = linspace(0, 1.5, n)[p]; q = cos(phi) * its trapezoid width, S = 6.371e6 / cos(phi) on
    active rows.  W: "cos" rint(cos(phi) * 2^30), "max" all 2^32 - 1, "one" all 1, or an array of one weight per ROW (zeros
    allowed; an active row with no weight poleward of it is refused).  ny: the rows of the plane (default: those of the domains)."""
    lengths = [int(n) for n in lengths]
    assert len(lengths) in (1, 2) and len(active) == len(lengths) and min(lengths) >= 1 and not (shared and len(lengths) == 1)
    doms = [list(range(lengths[0] - 1, -1, -1))]
    if len(lengths) == 2:
        first = lengths[0] - int(bool(shared))
        doms.append(list(range(first, first + lengths[1])))
    used = max(max(dom) for dom in doms) + 1
    ny = used if ny is None else int(ny)
    assert ny >= used
    kind = W if isinstance(W, str) else None
    Wr = np.zeros(ny, dtype=np.uint32) if kind else np.array(W, dtype=np.uint32)
    assert Wr.shape == (ny,)
    q, S, act = np.zeros(ny), np.zeros(ny), np.zeros(ny, dtype=np.uint8)
    given = set()
    for dom, pos in zip(doms, active):
        n = len(dom)
        phi = np.linspace(0.0, 1.5, n) if n > 1 else np.zeros(1)
        width = np.gradient(phi) if n > 2 else np.full(n, 1.5 / 2 if n == 2 else 0.0)
        if n > 2:
            width[0], width[-1] = (phi[1] - phi[0]) / 2, (phi[-1] - phi[-2]) / 2
        for p, j in enumerate(dom):
            if j not in given:
                q[j] = np.cos(phi[p]) * width[p]
                if kind:
                    Wr[j] = {"cos": np.rint(np.cos(phi[p]) * 2.0 ** 30), "max": 2 ** 32 - 1, "one": 1}[kind]
                given.add(j)
        for p in pos:
            j = dom[int(p)]
            assert not act[j] and not (shared and int(p) == 0), "an active row lies in one domain"
            act[j] = 1
            S[j] = 6.371e6 / np.cos(phi[int(p)])
    off = np.cumsum([0] + [len(dom) for dom in doms]).astype(np.int32)
    tab = dict(ndom=len(doms), dom_off=off, dom_rows=np.array([j for dom in doms for j in dom], dtype=np.int32), active=act, W=Wr, q=q, S=S)
    for dom in doms:
        assert all(c > 0 for c, j in zip(caps(tab, dom, 1), dom) if act[j]), "an active row has cap 0"
    return tab


def row_phi(tab, ny):
    """phi of every row as custom_table laid it out (the first domain that names a row decides; rows of no domain: 0)"""
    phi, given = np.zeros(ny), set()
    for dom in domains(tab):
        for p, v in enumerate(np.linspace(0.0, 1.5, len(dom)) if len(dom) > 1 else np.zeros(1)):
            if dom[p] not in given:
                phi[dom[p]] = v
                given.add(dom[p])
    return phi


def steep_field(tab, nx, steps, seed, dtype, noise=60.0):
    """5700 - 800 sin^2(phi) along each domain of a custom_table plus `noise` m of weather: the rows of a long domain differ by less
    than a metre, so every row crosses its contour many times"""
    ny = len(tab["W"])
    rng = np.random.default_rng(seed)
    z = 5700.0 - 800.0 * np.sin(row_phi(tab, ny))[None, :, None] ** 2 + rng.normal(0.0, noise, (steps, ny, nx))
    return z.astype(dtype)


def two_valued(tab, nx, steps, lo, hi, seed, dtype):
    """every pixel is `lo` or `hi`; the share of `hi` falls from 0.9 at the first position of a domain to 0.1 at its pole, so that
    the contours near the equator are `hi` and those near the pole `lo`"""
    ny = len(tab["W"])
    rng = np.random.default_rng(seed)
    share = 0.9 - 0.8 * row_phi(tab, ny) / 1.5
    return np.where(rng.random((steps, ny, nx)) < share[None, :, None], dtype(hi), dtype(lo)).astype(dtype)


def bisection(plane, tab, dom):
    """k_lwa_contour's search (csrc/ctk_lwa.hip) on one plane and one domain, restated in unsigned 64-bit integers: the key range of
    the weighted non-NaN pixels, `rounds` halvings of every active row's interval, in each of them a binary search of `probes`
    halvings over the pivots per pixel, the weights in na + 1 buckets, their suffix sums against the caps, and the clamp.  Returns
    dict(keys: one per active row in domain order, None where the contour is out of reach; rounds; probes; per: buckets per
    thread of the suffix scan; clamped: how often the clamp's `mid == hi` branch was taken).  A diagnostic: the yardstick is
    contours / from_table."""
    nx = plane.shape[1]
    pos = [p for p, j in enumerate(dom) if tab["active"][j]]
    na = len(pos)
    every = caps(tab, dom, nx)
    cap = np.array([every[p] for p in pos], dtype=np.uint64)
    vals = plane[dom, :].reshape(-1)
    w = np.repeat(tab["W"][dom].astype(np.uint64), nx)
    ok = ~np.isnan(vals)
    k, w = key(vals[ok]).astype(np.uint64), w[ok]                               # what a round sees: every non-NaN pixel, its weight may be 0
    counted = w != 0
    total = int(w.sum(dtype=np.uint64))
    res = dict(keys=[None] * na, rounds=0, probes=int(na).bit_length(), per=(na + 1024) // 1024, clamped=0)
    if na == 0:
        return res
    kmin, kmax = (int(k[counted].min()), int(k[counted].max())) if total else (2 ** 64 - 1, 0)
    res["rounds"] = (kmax - kmin).bit_length() if total and kmax > kmin else 0
    lo, hi = np.full(na, kmin, dtype=np.uint64), np.full(na, kmax, dtype=np.uint64)
    one = np.uint64(1)
    for _ in range(res["rounds"]):
        mid = lo + ((hi - lo) >> one)
        assert np.all(mid[:-1] >= mid[1:]), "the pivots fall with the active rows"
        l, h = np.zeros(len(k), dtype=np.int64), np.full(len(k), na, dtype=np.int64)
        for _t in range(res["probes"]):
            go = l < h
            m = np.where(go, (l + h) >> 1, 0)
            up = mid[m] >= k
            l, h = np.where(go & up, m + 1, l), np.where(go & ~up, m, h)
        bucket = np.zeros(na + 1, dtype=np.uint64)
        np.add.at(bucket, l, w)
        behind = (np.cumsum(bucket[::-1], dtype=np.uint64)[::-1] - bucket)[:na]             # the buckets behind a: A(mid[a])
        reach = behind >= cap
        res["clamped"] += int(np.count_nonzero(~reach & (mid == hi)))
        lo, hi = np.where(reach, lo, np.where(mid < hi, mid + one, hi)), np.where(reach, mid, hi)
    res["keys"] = [int(lo[a]) if total >= int(cap[a]) else None for a in range(na)]
    return res


def contour_keys(plane, tab, dom):
    """key(contours(...)) of the active rows as bisection gives them: Python integers, None where the contour is NaN"""
    Z = contours(plane, tab, dom)[0]
    pos = [p for p, j in enumerate(dom) if tab["active"][j]]
    return [None if np.isnan(Z[p]) else int(key(Z[p:p + 1])[0]) for p in pos]


# ---- diagnostics ------------------------------------------------------------------------------------------------------------------
def nonzero_share(out, tab):
    """share of the pixels of the active rows that are finite and not 0"""
    band = out[:, np.asarray(tab["active"]) != 0]
    return float(np.count_nonzero(np.isfinite(band) & (band != 0))) / max(band.size, 1)


def tie_rows(z, tab):
    """active rows (over all steps) whose cap lies strictly inside a tie group: the contour's value is shared by two pixels or more
    of the domain, A(Z) > cap, and the keys below Z hold less than cap"""
    n = 0
    for s in range(z.shape[0]):
        for dom in domains(tab):
            Z, keys, cum = contours(z[s], tab, dom)
            for p, cap in enumerate(caps(tab, dom, z.shape[2])):
                if not tab["active"][dom[p]] or np.isnan(Z[p]):
                    continue
                k = key(Z[p:p + 1])[0]
                i0, i1 = int(np.searchsorted(keys, k, side='left')), int(np.searchsorted(keys, k, side='right'))
                below = int(cum[i0 - 1]) if i0 else 0
                n += int(i1 - i0 >= 2 and below < cap < int(cum[i1 - 1]))
    return n


def nan_rows(ref, tab):
    """(active rows whose contour is NaN, active rows whose contour is finite), per step: two (steps,) arrays"""
    band = ref[:, np.asarray(tab["active"]) != 0]
    return np.isnan(band).sum(axis=1), np.isfinite(band).sum(axis=1)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
SEL_WAVES, CELLS, LDS_MAX, GRID_MAX, XCD_MIN = 16, 2048, 65536, (1 << 24) - 1, 2048


def plan(elem_bytes, rows_, nx, ndom=1, steps=1, aligned=True):
    """ctk_lwa_plan of csrc/ctk_forms.h restated: the vector form needs aligned base pointers and rows of a multiple of 4 pixels; a
    strip is as wide as keeps rows x strip within 2048 pixels, in whole units of 4 pixels (vector) or 1 (scalar), at least one unit
    and at most the row; the call fits while the narrowest strip of the longest domain stays within 64 KB of LDS and so do the
    contour kernel's 32 bytes per row + 1 and 8 bytes for each of its 16 waves; the contour kernel has a workgroup per (step,
    domain) under the same cap and XCD rule"""
    vec = int(bool(aligned) and nx % 4 == 0)
    unit = 4 if vec else 1
    strip = min(max(CELLS // rows_ // unit, 1) * unit, -(-nx // unit) * unit)
    nstrips = -(-nx // strip)
    lds_sel = (rows_ + 1) * 32 + SEL_WAVES * 8
    blocks = steps * ndom * nstrips
    grid_, sel = min(blocks, GRID_MAX), min(steps * ndom, GRID_MAX)
    return dict(ok=int(rows_ * unit * elem_bytes <= LDS_MAX and lds_sel <= LDS_MAX), vec=vec, strip=strip, nstrips=nstrips, lds=rows_ * strip * elem_bytes, lds_sel=lds_sel,
                blocks=blocks, grid=grid_, xcd=int(grid_ >= XCD_MIN), sel_blocks=steps * ndom, sel_grid=sel, sel_xcd=int(sel >= XCD_MIN))
