"""The numpy statement of the block-centred composite (include/contrack_hip.h, "block-centred composites"): the reference has no
function for it, this loop is the yardstick of tests/test_centred_host.py and tests/test_gpu_centred*.py.

    sum[b, j + hy, i + hx] = +0.0 (float64);  n[...] = 0 (uint32)
    for r = 0 .. R-1, rising (the order of the arrays as given):
        if bin[r] < 0: continue
        for j in -hy..hy, i in -hx..hx:
            y = row[r] + j;   if y < 0 or y >= ny: continue
            c = col[r] + i;   wrap: c = c mod nx;   else if c < 0 or c >= nx: continue
            v = float64(x[t[r], y, c]);   if skipna and v is NaN: continue
            sum[bin[r], j + hy, i + hx] += v;   n[...] += 1

Three arguments state the three ways of getting it wrong that a test can see: order="falling" walks the stamps in reversed order,
acc="float32" accumulates in float32, slice=k sums every k consecutive stamps on their own and then adds the partial sums (what a
split of a bin's stamps over threads would give)."""
import numpy as np

from composite_util import bits, differing, same_bits                          # noqa: F401  (the comparisons are the composite's)


def _run(x, t, row, col, bin, nbins, hy, hx, wrap, skipna, stamps, acc):
    """the loop over the listed stamps, in the listed order; the sum in `acc`"""
    T, ny, nx = x.shape
    s = np.zeros((nbins, 2 * hy + 1, 2 * hx + 1), dtype=acc)
    n = np.zeros(s.shape, dtype=np.uint32)
    jj = np.arange(-hy, hy + 1)
    ii = np.arange(-hx, hx + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in stamps:
            b = int(bin[r])
            if b < 0:
                continue
            y = int(row[r]) + jj
            c = int(col[r]) + ii
            oky = (y >= 0) & (y < ny)
            okc = np.ones(c.shape, dtype=bool) if wrap else (c >= 0) & (c < nx)
            c = c % nx
            v = x[int(t[r])][np.ix_(np.where(oky, y, 0), np.where(okc, c, 0))].astype(acc)
            sel = oky[:, None] & okc[None, :]
            if skipna:
                sel = sel & ~np.isnan(v)
            s[b][sel] = s[b][sel] + v[sel]
            n[b][sel] += 1
    return s, n


def centred(x, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, order="rising", acc="float64", slice=None):
    """(sum float64, n uint32), both (nbins, 2 hy + 1, 2 hx + 1), of x (T, ny, nx) float32 / float64 and the stamps t, row, col, bin"""
    x = np.asarray(x)
    assert x.ndim == 3 and order in ("rising", "falling")
    assert not wrap or 2 * hx + 1 <= x.shape[2]
    R = len(t)
    acc = np.dtype(acc)
    stamps = list(range(R)) if order == "rising" else list(range(R - 1, -1, -1))
    if slice is None:
        s, n = _run(x, t, row, col, bin, nbins, hy, hx, wrap, skipna, stamps, acc)
        return s.astype(np.float64), n
    s = np.zeros((nbins, 2 * hy + 1, 2 * hx + 1), dtype=acc)
    n = np.zeros(s.shape, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, R, slice):
            ps, pn = _run(x, t, row, col, bin, nbins, hy, hx, wrap, skipna, stamps[k:k + slice], acc)
            touched = pn > 0                                   # (a slice that reached nothing adds nothing)
            s[touched] = s[touched] + ps[touched]
            n += pn
    return s.astype(np.float64), n


def mean(s, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n == 0, np.nan, s / n)


def plan(elem_bytes, nbins, hy, hx, max_bin=0, kept=None, form=-1, unroll=-1, threads=-1):
    """ctk_centred_plan (csrc/ctk_forms.h) restated: the fed form where its estimate is below the plain form's and the longest bin
    has 128 stamps or more"""
    wcells = (2 * hy + 1) * (2 * hx + 1)
    per_bin = (wcells + 63) // 64
    waves = nbins * per_bin
    work = float(max_bin if kept is None else kept) * float(per_bin)
    plain_ns = max(float(max_bin) * 181.0, work * 0.076)
    fed_ns = max(float(max_bin) * 23.0, work * 0.082 + float(waves) * 3.3)
    fed = int(form != 0) if form >= 0 else int(max_bin >= 128 and fed_ns < plain_ns)
    u = 128 // max(elem_bytes, 4)
    if unroll > 0:
        u = 1
        while u * 2 <= unroll and u * 2 <= 32:
            u <<= 1
    th = 64
    if waves > 2048:
        th = 256
    if threads > 0:
        th = 64
        while th * 2 <= threads and th * 2 <= 256:
            th <<= 1
    if fed:
        u, th = 32 // max(elem_bytes, 4), 64
    u = min(u, 32)
    parts = (wcells + th - 1) // th
    return dict(form=fed, unroll=u, threads=th, parts=parts, blocks=nbins * parts, grid=min(nbins * parts, 0xffffff // 4 if fed else 0xffffff))


def wide_case(dtype, T=23, ny=7, nx=12, R=40, nbins=3, seed=0):
    """the discriminating input of the issue: x = normal x 10**uniform(-8, 10) cast to dtype; t sorted random, row and col random,
    bin random in [-1, nbins)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ny, nx)) * 10.0 ** rng.uniform(-8, 10, (T, ny, nx))).astype(dtype)
    t = np.sort(rng.integers(0, T, R)).astype(np.int64)
    row = rng.integers(0, ny, R).astype(np.int32)
    col = rng.integers(0, nx, R).astype(np.int32)
    bin = rng.integers(-1, nbins, R).astype(np.int32)
    return x, t, row, col, bin
