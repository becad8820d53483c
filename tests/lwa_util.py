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
