"""numpy statement of the gradient-reversal blocking index (include/contrack_hip.h, the block above ctk_reversal_f32) and the case
builders of the reversal tests.  The reference has no function for it, so these loops are what the library is pinned against.

Row table, per row j with phi = lat[j], s = +1 if phi > 0 else -1:
    eq[j] the row nearest to phi - s * delta, po[j] the row nearest to phi + s * delta, eq2[j] the row nearest to phi - 2 s delta;
    "nearest" only counts closer than half the largest row spacing (and never the row itself); a row is active if
    lo <= |phi| <= hi, its hemisphere is selected and all its partners exist; dE = |lat[j] - lat[eq]|, dP = |lat[po] - lat[j]|,
    dE2 = |lat[eq] - lat[eq2]|; tS = ghgs * dE, tN = ghgn * dP, tS2 = ghgs2 * dE2
Per pixel of an active row, float64:
    dS = z[j] - z[eq] ; dN = z[po] - z[j] ; dS2 = z[eq] - z[eq2]
    blocked = dS > tS and dN < tN [and dS2 < tS2]
    out = dtype(dS / dE) if blocked else 0            ('gradient')          1 if blocked else 0            ('mask')

`f32_sub` and `div_delta` state the two ways of getting it wrong that tests/test_reversal_host.py shows the statement can see."""
import numpy as np

from level_util import bits, differing, same_bits          # noqa: F401  (the comparison of the level-mean tests: NaN payloads are not compared)


def rows(lat, delta=15., lat_bounds=(30, 75), hemisphere='both', second=False):
    """(eq, po, eq2, dE, dP, dE2): int64 partners (-1: none / inactive) and float64 distances (0 on inactive rows)"""
    lat = [float(v) for v in lat]
    ny = len(lat)
    half = max([abs(lat[i + 1] - lat[i]) for i in range(ny - 1)], default=0.0) / 2
    eq, po, eq2 = [-1] * ny, [-1] * ny, [-1] * ny
    dE, dP, dE2 = [0.0] * ny, [0.0] * ny, [0.0] * ny

    def nearest(v, j):
        best = min(range(ny), key=lambda k: (abs(lat[k] - v), k))
        return best if abs(lat[best] - v) < half and best != j else -1
    for j, phi in enumerate(lat):
        if not lat_bounds[0] <= abs(phi) <= lat_bounds[1]:
            continue
        if (hemisphere == 'north' and not phi > 0) or (hemisphere == 'south' and not phi < 0):
            continue
        s = 1.0 if phi > 0 else -1.0
        e, p = nearest(phi - s * delta, j), nearest(phi + s * delta, j)
        f = nearest(phi - 2 * s * delta, e) if second and e >= 0 else 0
        if e < 0 or p < 0 or f < 0:
            continue
        eq[j], po[j], dE[j], dP[j] = e, p, abs(lat[j] - lat[e]), abs(lat[p] - lat[j])
        if second:
            eq2[j], dE2[j] = f, abs(lat[e] - lat[f])
    return np.array(eq), np.array(po), np.array(eq2), np.array(dE), np.array(dP), np.array(dE2)


def table(lat, delta=15., ghgs=0., ghgn=-10., ghgs2=None, lat_bounds=(30, 75), hemisphere='both'):
    """the row table of ctk_reversal_* as a dict (eq, po, eq2, dE, tS, tN, tS2; eq2 and tS2 None without ghgs2)"""
    eq, po, eq2, dE, dP, dE2 = rows(lat, delta, lat_bounds, hemisphere, ghgs2 is not None)
    return dict(eq=eq.astype(np.int32), po=po.astype(np.int32), eq2=eq2.astype(np.int32) if ghgs2 is not None else None, dE=dE, tS=ghgs * dE, tN=ghgn * dP,
                tS2=ghgs2 * dE2 if ghgs2 is not None else None)


def from_table(z, tab, mask=False, f32_sub=False, div=None):
    """the per-pixel statement on a row table.  f32_sub: the differences are taken in z's dtype (wrong for float32); div: a number
    the blocked gradient is divided by instead of dE[j] (wrong wherever dE != div)"""
    z = np.asarray(z)
    out = np.zeros_like(z)
    wide = (lambda a: a) if f32_sub else (lambda a: a.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(z.shape[1]):
            e = int(tab["eq"][j])
            if e < 0:
                continue
            dS = (wide(z[:, j]) - wide(z[:, e])).astype(np.float64)
            dN = (wide(z[:, int(tab["po"][j])]) - wide(z[:, j])).astype(np.float64)
            ok = (dS > tab["tS"][j]) & (dN < tab["tN"][j])
            if tab["eq2"] is not None:
                ok &= (wide(z[:, e]) - wide(z[:, int(tab["eq2"][j])])).astype(np.float64) < tab["tS2"][j]
            val = np.ones_like(dS) if mask else dS / (tab["dE"][j] if div is None else div)
            out[:, j] = np.where(ok, val.astype(z.dtype), z.dtype.type(0))
    return out


def reversal(z, lat, delta=15., ghgs=0., ghgn=-10., ghgs2=None, lat_bounds=(30, 75), hemisphere='both', stat='gradient', f32_sub=False, div_delta=False):
    """z (steps, ny, nx) float32 / float64 -> the index in z's dtype.  div_delta: divides by delta instead of the rows' distance."""
    return from_table(z, table(lat, delta, ghgs, ghgn, ghgs2, lat_bounds, hemisphere), mask=stat == 'mask', f32_sub=f32_sub, div=delta if div_delta else None)


def grid(step, rising=False):
    """global regular latitudes from the north pole down (rising: from the south pole up)"""
    lat = 90.0 - step * np.arange(int(round(180 / step)) + 1)
    return lat[::-1].copy() if rising else lat


def gaussian(n=48):
    """the latitudes of a Gaussian grid: arcsin of the Gauss-Legendre nodes, from the north down -- irregular, most so near the poles"""
    return np.rad2deg(np.arcsin(np.polynomial.legendre.leggauss(n)[0]))[::-1].copy()


def field(lat, nx, steps=6, seed=0, dtype=np.float32):
    """z = 5600 - 900 sin^2(phi) + N(0, 150): the mean meridional profile of 500 hPa height, with weather"""
    rng = np.random.default_rng(seed)
    prof = 5600.0 - 900.0 * np.sin(np.deg2rad(np.asarray(lat, dtype=np.float64))) ** 2
    return (prof[None, :, None] + rng.normal(0.0, 150.0, (steps, len(lat), nx))).astype(dtype)


def blocked_share(out, eq):
    """share of the pixels of the active rows that are not 0"""
    band = np.asarray(eq) >= 0
    return float(np.count_nonzero(out[:, band])) / max(out[:, band].size, 1)


THREADS, GRID_MAX, XCD_MIN = 256, (1 << 24) - 1, 2048       # (a launch of 256-thread workgroups stays below 2^32 work-items)


def plan(elem_bytes, ny, nx, steps, aligned):
    """ctk_reversal_plan of csrc/ctk_forms.h restated: the vector form needs aligned base pointers and ROWS of a multiple of 16 bytes
    (a lane never straddles two rows); a lane takes 16 bytes of a row (or one pixel), 256 lanes per workgroup, a workgroup inside one
    step, at most 2^24 - 1 workgroups per launch (the kernel strides over the rest); launches of 2048 workgroups or more give every
    XCD one contiguous eighth of them"""
    vec = int(bool(aligned) and (nx * elem_bytes) % 16 == 0)
    vpt = 16 // elem_bytes if vec else 1
    lanes = ny * (nx // vpt)
    bps = -(-lanes // THREADS)
    blocks = bps * steps
    grid_ = min(blocks, GRID_MAX)
    return dict(vec=vec, vpt=vpt, bps=bps, blocks=blocks, grid=grid_, xcd=int(grid_ >= XCD_MIN))
