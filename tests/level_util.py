"""numpy statement of the vertical mean over the selected levels (include/contrack_hip.h, the block above ctk_level_mean_f32) and the
case builders of the level-mean tests.  The reference has no function for this step -- its README only describes it
(README.rst:235-240) --, so this loop is what the library is pinned against:

    acc = 0.0 ; ws = 0.0                                   (float64, per step and pixel)
    for l in rising order over the levels with w[l] != 0:
        acc = acc + float64(w[l]) * float64(x[s, l, y, x])   # a rounded multiply, then a rounded add
        ws  = ws + w[l]
    out[s, y, x] = dtype(acc / ws)

`order` and `fma` state the two ways of getting it wrong that the float64 cases can see (tests/test_level_mean_host.py)."""
import numpy as np

# the pinned example: levels in hPa, bounds (150, 500), trapezoid weights over the selected levels (sum 350)
PINNED_LEVELS = np.array([1000, 850, 700, 500, 450, 400, 350, 300, 250, 225, 200, 175, 150, 125, 100], dtype=np.float64)
PINNED_WEIGHTS = np.array([0, 0, 0, 25, 50, 50, 50, 50, 37.5, 25, 25, 25, 12.5, 0, 0], dtype=np.float64)


def level_mean(x, w, skipna=False, order="rising", fma=False):
    """x (steps, nlev, ny, nx) float32 / float64, w nlev float64 -> (steps, ny, nx) in x's dtype.  order='falling' sums the selected
    levels from the top index down; fma=True replaces the rounded multiply and the rounded add by one rounding of w * x + acc,
    evaluated in np.longdouble."""
    x = np.asarray(x)
    w = np.asarray(w, dtype=np.float64)
    sel = [l for l in range(x.shape[1]) if w[l] != 0]
    if order == "falling":
        sel = sel[::-1]
    acc = np.zeros((x.shape[0],) + x.shape[2:], dtype=np.float64)
    ws = np.zeros_like(acc)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for l in sel:
            xv = x[:, l].astype(np.float64)
            if fma:
                new = (np.longdouble(w[l]) * xv.astype(np.longdouble) + acc.astype(np.longdouble)).astype(np.float64)
            else:
                prod = w[l] * xv
                new = acc + prod
            if skipna:
                ok = ~np.isnan(xv)
                acc = np.where(ok, new, acc)
                ws = np.where(ok, ws + w[l], ws)
            else:
                acc = new
                ws = ws + w[l]
        return (acc / ws).astype(x.dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """equal dtype, shape, NaN positions and, everywhere else, bit patterns.  The payload and sign of a NaN are not compared: IEEE 754
    leaves them to the implementation (0 / 0 is 0xfff8... on an x86 host and 0x7ff8... on the device), and nothing reads them."""
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


def field(dtype, steps=7, nlev=15, ny=9, nx=65, seed=0):
    """standard normal x 3"""
    return (3.0 * np.random.default_rng(seed).standard_normal((steps, nlev, ny, nx))).astype(dtype)


def random_weights_on(w, seed=1):
    """random float64 weights in (0.5, 1.5) on the levels `w` selects"""
    r = np.random.default_rng(seed).random(len(w)) + 0.5
    return np.where(np.asarray(w) != 0, r, 0.0)


def runs_of(w):
    """[(first level, length)] of the runs of neighbouring selected levels"""
    sel = np.flatnonzero(np.asarray(w) != 0)
    return [(int(r[0]), len(r)) for r in np.split(sel, np.flatnonzero(np.diff(sel) != 1) + 1)]


THREADS, UNROLL, GRID_MAX, XCD_MIN = 256, 8, (1 << 24) - 1, 2048       # (a launch of 256-thread workgroups stays below 2^32 work-items)


def plan(elem_bytes, nsel, npix, steps, aligned):
    """ctk_level_plan of csrc/ctk_forms.h restated: the vector form needs aligned base pointers and planes of a multiple of 16 bytes;
    a lane takes 16 bytes of pixels (or one pixel), 256 lanes per workgroup, a workgroup inside one step, at most 2^24 - 1 workgroups per
    launch (the kernel strides over the rest); launches of 2048 workgroups or more give every XCD one contiguous eighth of them"""
    vec = int(bool(aligned) and (npix * elem_bytes) % 16 == 0)
    vpt = 16 // elem_bytes if vec else 1
    lanes = -(-npix // vpt)
    bps = -(-lanes // THREADS)
    blocks = bps * steps
    unroll = UNROLL if nsel >= UNROLL else 4 if nsel >= 4 else 2 if nsel >= 2 else 1
    grid = min(blocks, GRID_MAX)
    return dict(vec=vec, vpt=vpt, unroll=unroll, bps=bps, blocks=blocks, grid=grid, xcd=int(grid >= XCD_MIN))
