"""The numpy statement of the composite (include/contrack_hip.h, "composites"): the reference has no function for it, this loop is the
yardstick of tests/test_composite_host.py and tests/test_gpu_composite*.py.

    sum[g, p] = +0.0 (float64);  n[g, p] = 0 (uint32)
    for t = 0 .. T-1, rising:
        sel = flag[t, p] > above            (and, with skipna, x[t, p] is not NaN)
        if sel:  sum[ids[t], p] = sum[ids[t], p] + float64(x[t, p]);   n[ids[t], p] += 1

An unselected step adds nothing.  Three arguments state the three ways of getting it wrong that a test can see:
order="falling" sums in reversed time order, acc="float32" accumulates in float32, slice=k sums every k consecutive steps on their
own and then adds the partial sums (what a split of T over workgroups would give)."""
import numpy as np


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    """equal dtype, shape, NaN positions and, everywhere else, bit patterns (NaN payloads and signs are not compared: IEEE 754 leaves
    them to the implementation)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def differing(a, b):
    """how many outputs differ in at least one bit (NaN positions counted as above)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero((na != nb) | (~na & ~nb & (bits(a) != bits(b)))))


def _run(flag, x, ids, G, above, skipna, steps, acc):
    """the loop over the listed steps, in the listed order; the sum in `acc`"""
    shape = (G,) + flag.shape[1:]
    s = np.zeros(shape, dtype=acc)
    n = np.zeros(shape, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in steps:
            v = x[t].astype(acc)
            sel = flag[t] > above
            if skipna:
                sel = sel & ~np.isnan(v)
            g = 0 if ids is None else int(ids[t])
            s[g][sel] = s[g][sel] + v[sel]
            n[g][sel] += 1
    return s, n


def composite(flag, x, ids, G, above=0, skipna=False, order="rising", acc="float64", slice=None):
    """(sum float64 (G, ny, nx), n uint32 (G, ny, nx)) of flag (T, ny, nx) integer and x (T, ny, nx) float32 / float64; ids: T group
    ids in [0, G), or None (one group)"""
    flag, x = np.asarray(flag), np.asarray(x)
    assert flag.shape == x.shape and flag.ndim == 3 and order in ("rising", "falling")
    T = flag.shape[0]
    acc = np.dtype(acc)
    steps = list(range(T)) if order == "rising" else list(range(T - 1, -1, -1))
    if slice is None:
        s, n = _run(flag, x, ids, G, above, skipna, steps, acc)
        return s.astype(np.float64), n
    s = np.zeros((G,) + flag.shape[1:], dtype=acc)
    n = np.zeros((G,) + flag.shape[1:], dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, T, slice):
            ps, pn = _run(flag, x, ids, G, above, skipna, steps[k:k + slice], acc)
            touched = pn > 0                                   # (a slice that selected nothing adds nothing)
            s[touched] = s[touched] + ps[touched]
            n += pn
    return s.astype(np.float64), n


def plan(elem_bytes, npix, unroll=-1):
    """ctk_composite_plan (csrc/ctk_forms.h) restated"""
    want = (8 << 20) // max(npix * (4 + elem_bytes), 1)
    u = 16
    while u > 8 and u > want:
        u >>= 1
    if unroll > 0:
        u = 1
        while u * 2 <= unroll and u * 2 <= 16:
            u <<= 1
    blocks = (npix + 255) // 256
    return dict(unroll=u, blocks=blocks, grid=min(blocks, 0xffffff))


def wide_case(dtype, T=61, ny=5, nx=13, seed=0, frac=0.3):
    """the discriminating input of the issue: x = normal x 10**uniform(-8, 10) cast to dtype, `frac` of the pixels flagged (ids 1..3)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ny, nx)) * 10.0 ** rng.uniform(-8, 10, (T, ny, nx))).astype(dtype)
    flag = np.where(rng.random((T, ny, nx)) < frac, rng.integers(1, 4, (T, ny, nx)), 0).astype(np.int32)
    return flag, x
