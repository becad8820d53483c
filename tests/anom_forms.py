"""ctk_anom_plan of csrc/ctk_forms.h restated, the yardstick of the segmented / streamed anomaly tests, and the builders of their cases
(tests/test_anom_forms_host.py, tests/test_gpu_anom_seg_forms.py, tests/test_gpu_anom_segments.py).

The yardstick is oracle/anom_port.py used as it is (`expected`).  Beside it stand models of the ways the kernels of
csrc/ctk_anom_seg.hip could be wrong without a narrow slab noticing -- `anom_model` (the raw anomaly not rounded to the dtype, the window
summed newest first), the port on the time-reversed slab (group sums in falling t), `clim_acc_model` (k_clim_acc's stripes and its
flush on a group change) -- so that a test can assert, on the CPU, that its slab tells them apart before it trusts a comparison."""
import numpy as np

from oracle import anom_port

THREADS, RING_BYTES, TILE_MIN, TILE_MAX, WAVES, GRID_Y_MAX = 256, 32768, 32, 256, 16384, 65535
PLAIN, RING = 0, 1
ACC_STRIPES, ROLL_ROWS = 32, 64          # workgroup rows of k_clim_acc / k_clim_roll: min(G, .)


def ring_steps(elem_bytes):
    """the longest smoothing whose ring fits: 32 (float32), 16 (float64)"""
    return RING_BYTES // (THREADS * elem_bytes)


def plan(elem_bytes, smooth, nt, npix, waves_wanted=0, grid_y_max=0):
    """ctk_anom_plan: the ring form while smooth x 256 lanes x elem_bytes fit 32 KB; its tile is the longest that still leaves
    `waves_wanted` waves, at least 32 and 8 x the halo, at most 256; the plain form's is 32; either is raised until gridDim.y fits"""
    ww = waves_wanted if waves_wanted > 0 else WAVES
    gm = min(grid_y_max, GRID_Y_MAX) if grid_y_max > 0 else GRID_Y_MAX
    lds = smooth * THREADS * elem_bytes
    form = RING if lds <= RING_BYTES else PLAIN
    waves = -(-npix // 64)
    tile = max(1, nt * waves // ww)
    tile = min(TILE_MAX, max(tile, TILE_MIN, 8 * (smooth - 1)))
    if form == PLAIN:
        tile, lds = TILE_MIN, 0
    tile = max(tile, -(-nt // gm))
    return dict(form=form, lds=lds, tile=tile, gx=-(-npix // THREADS), gy=max(1, -(-nt // tile)))


def overrides_for_tile(elem_bytes, smooth, nt, npix, tile):
    """(waves_wanted, grid_y_max) for which the plan of this launch has `tile` output steps per workgroup: through the waves term where
    some waves_wanted gives it (nt * waves // waves_wanted skips values), else through the gridDim.y rule; None: neither can"""
    waves = -(-npix // 64)
    for ww in range(max(1, nt * waves // (tile + 1)), nt * waves // tile + 2):
        if plan(elem_bytes, smooth, nt, npix, ww)["tile"] == tile:
            return ww, 0
    gm = -(-nt // tile)
    return (0, gm) if plan(elem_bytes, smooth, nt, npix, 0, gm)["tile"] == tile else None


def stream_chunk(T, smooth, chunk_steps):
    """steps per chunk of ctk_anom_stream_* for chunk_steps > 0: at least the halo, at most T"""
    return min(max(chunk_steps, smooth - 1, 1), T)


def stream_launches(T, smooth, chunk_steps):
    """[(o0, o1)] of the anomaly launches of pass 2: chunk k completes the outputs whose window ends inside it -- (smooth - 1) // 2 steps
    behind the input --, the last chunk everything that is left; a chunk that completes nothing launches nothing"""
    chunk, fwd = stream_chunk(T, smooth, chunk_steps), (smooth - 1) // 2
    out, done = [], 0
    for c0 in range(0, T, chunk):
        nt = min(chunk, T - c0)
        o1 = T if c0 + nt == T else max(done, c0 + nt - fwd)
        if o1 > done:
            out.append((done, o1))
        done = o1
    return out


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def expected(x, group, G, window, smooth, starts, clim=None):
    """oracle/anom_port.py unchanged: the climatology of the whole slab, then calc_anom on every segment [s, e) with it"""
    with np.errstate(invalid="ignore"):
        clim = anom_port.calc_clim(x, group, G, window) if clim is None else clim
        edges = list(starts) + [x.shape[0]]
        parts = [anom_port.calc_anom(x[s:e], group[s:e], G, window, smooth, clim=clim) for s, e in zip(edges[:-1], edges[1:])]
        return np.concatenate(parts), clim.astype(x.dtype)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def differ_finite(a, b):
    """some output is finite in both and not the same number"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.any(np.isfinite(a) & np.isfinite(b) & (a != b)))


# ---- slabs and groups ------------------------------------------------------------------------------------------------------------
def slab(rng, T, shape, dtype, edges=True, inf=True):
    """the `wide` recipe and the edges of tests/test_gpu_anom_exact.py: values of either sign over seven decades, so that x - clim is
    inexact in the dtype and sums depend on their order; 3% NaN, an all-NaN pixel, an all-NaN step, +-inf at a few places"""
    x = (rng.choice([-1.0, 1.0], (T,) + shape) * 10.0 ** rng.uniform(-3, 4, (T,) + shape)).astype(dtype)
    if edges:
        f = x.reshape(T, -1)
        f[rng.random(f.shape) < 0.03] = np.nan
        if f.shape[1] > 1:
            f[:, f.shape[1] // 2] = np.nan
        if T > 2:
            f[T // 3] = np.nan
        if inf and f.shape[1] > 1:                       # (a single pixel would hold nothing else: +inf and -inf make every sum NaN)
            f[1 % T, -1] = np.inf
            f[(T - 2) % T, -1] = -np.inf
            f[3 % T, 0] = np.inf
    return x


def run_groups(T, G=12, run=3):
    """ids that change every `run` steps, from an offset that puts the changes off round numbers"""
    return (((np.arange(T) + 17) // run) % G).astype(np.int32)


GROUP_RULES = ("cyclic", "shuffled", "gaps", "one", "alternating")


def groups(rule, T, G, rng):
    if rule == "cyclic":
        return (np.arange(T) % G).astype(np.int32)
    if rule == "shuffled":
        return rng.permutation(np.arange(T) % G).astype(np.int32)
    if rule == "gaps":                                   # every third group owns no step
        ids = np.array([g for g in range(G) if g % 3 != 2])
        return ids[np.arange(T) % len(ids)].astype(np.int32)
    if rule == "one":                                    # every other group is empty (the last but one: inside the fill's window)
        return np.full(T, G - 2, dtype=np.int32)
    if rule == "alternating":                            # g, g + 32, g, g + 32: two groups of one stripe of k_clim_acc wherever G > 32
        a, b = alternating_pair(G)
        return np.where(np.arange(T) % 2 == 0, a, b).astype(np.int32)
    raise KeyError(rule)


def alternating_pair(G):
    a = max(G - 1 - ACC_STRIPES, 0)
    return a, (a + ACC_STRIPES if a + ACC_STRIPES < G else G - 1)


# ---- models of what could be wrong -----------------------------------------------------------------------------------------------
def anom_model(x, group, clim, smooth, starts, unrounded=False, newest_first=False, rotated=False):
    """the kernels' anomaly loop per segment.  As it stands it is the port.  unrounded: the raw anomaly x - clim[group] is not rounded
    to the slab's dtype before it is added (float32: it stays the float64 difference; float64: it stays the exact difference, here
    np.longdouble, and the sum is rounded once per addition).  newest_first: the window is summed from its last step down.  rotated: from
    its last step, then from the first up -- k_anom_ring's re-add begun at the slot just written instead of the oldest."""
    x = np.asarray(x)
    dt = x.dtype
    wide = np.longdouble if (unrounded and dt == np.float64) else np.float64
    c = np.asarray(clim, dtype=np.float64)
    if dt == np.float32:
        c = c.astype(np.float32).astype(np.float64)
    out = np.full(x.shape, np.nan, dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        raw = x.astype(wide) - c.astype(wide)[np.asarray(group)]
        if dt == np.float32 and not unrounded:
            raw = raw.astype(np.float32).astype(np.float64)
        edges = list(starts) + [x.shape[0]]
        for s, e in zip(edges[:-1], edges[1:]):
            first, last = smooth // 2, e - s - 1 - (smooth - 1) // 2
            if last < first:
                continue
            m = last - first + 1
            acc = np.zeros((m,) + x.shape[1:])
            order = range(smooth - 1, -1, -1) if newest_first else [smooth - 1] + list(range(smooth - 1)) if rotated else range(smooth)
            for j in order:
                acc = (acc.astype(wide) + raw[s + j:s + j + m]).astype(np.float64)
            out[s + first:s + last + 1] = (acc / smooth).astype(dt)
    return out


def clim_reversed(x, group, G, window):
    """the port's climatology with every group's steps added in falling t"""
    with np.errstate(invalid="ignore"):
        return anom_port.calc_clim(np.asarray(x)[::-1], np.asarray(group)[::-1], G, window).astype(x.dtype)


def clim_acc_model(x, group, G, window, chunk_steps, flush=True, modulus=None):
    """k_clim_acc / k_clim_fin / k_clim_roll as ctk_anom_stream_* runs them: per chunk, workgroup row y of min(G, 32) walks the chunk
    in time order, takes the groups with g % rows == y, keeps the sum and count of the group it is in and writes them back when the
    group changes and at the end of the chunk.  flush=False drops the write-back on a group change; `modulus` replaces `rows` in the
    stripe test.  As it stands it is the port's climatology."""
    x = np.asarray(x)
    T = x.shape[0]
    f = x.reshape(T, -1).astype(np.float64)
    npix = f.shape[1]
    sums, counts = np.zeros((G, npix)), np.zeros((G, npix), dtype=np.int64)
    rows = min(G, ACC_STRIPES)
    mod = rows if modulus is None else modulus
    chunk = min(max(chunk_steps, 1), T)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, T, chunk):
            for y in range(rows):
                cur, s, c = -1, None, None
                for t in range(c0, min(T, c0 + chunk)):
                    g = int(group[t])
                    if g % mod != y:
                        continue
                    if g != cur:
                        if cur >= 0 and flush:
                            sums[cur], counts[cur] = s, c
                        cur, s, c = g, sums[g].copy(), counts[g].copy()
                    ok = ~np.isnan(f[t])
                    s = np.where(ok, s + np.where(ok, f[t], 0.0), s)
                    c = c + ok
                if cur >= 0:
                    sums[cur], counts[cur] = s, c
        raw = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
        raw = raw.astype(x.dtype).astype(np.float64)
        clim = anom_port.rolling_mean_centred(raw, window, axis=0)
        fill, _ = anom_port._nanmean_rows(raw[max(0, G - window):], raw.shape[1:])
        return np.where(np.isnan(clim), fill[None], clim).astype(x.dtype).reshape((G,) + x.shape[1:])


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def ring_edge_starts(T, smooth):
    """T = 3 smooth + 7: segments of 1, smooth + 6 (it holds the slab's all-NaN step T // 3), smooth - 1 (no output), smooth (one
    output) and 1 steps: a break at 1 and at T - 1"""
    assert T == 3 * smooth + 7
    return [0, 1, smooth + 7, 2 * smooth + 6, T - 1]


RING_EDGE = [(np.float32, 31), (np.float32, 32), (np.float32, 33), (np.float64, 15), (np.float64, 16), (np.float64, 17)]

# (dtype, smooth, tile): ring forms whose 8 x halo stays below the tile -- 33, a tile that is no multiple of 8, and 256 reached by the clamp
TILE_EDGE = [(np.float32, 5, 33), (np.float64, 5, 33), (np.float32, 20, 157), (np.float64, 16, 157), (np.float32, 32, 256), (np.float64, 16, 256)]

CLIM_G = (31, 32, 33, 64, 65, 97, 366)
CLIM_CHUNKS = (1, 2, 5, 32, 33, None)                    # None: T
CLIM_WINDOWS = (1, 4, None)                              # None: G + 5
CLIM_SHAPES = ((1, 1), (5, 51), (16, 16), (1, 257))      # 1, 255, 256, 257 pixels


def clim_cases():
    """(G, rule, chunk_steps, window, shape, T): every G with every group rule, the chunk sizes, windows and plane sizes spread over them;
    the alternating pair with every chunk size that holds more than one step"""
    out, i = [], 0
    for G in CLIM_G:
        T = max(2 * G + 5, 80)
        for rule in GROUP_RULES:
            chunks = [CLIM_CHUNKS[i % 6]] if rule != "alternating" else [2, 5, 32, 33, None]
            for ch in chunks:
                w = CLIM_WINDOWS[(i // 2) % 3]
                out.append((G, rule, T if ch is None else ch, G + 5 if w is None else w, CLIM_SHAPES[(i // 3) % 4], T))
                i += 1
    return out


def assert_discriminates(x, group, G, window, smooth, starts):
    """the conditions under which a comparison with the port on this slab means something: the port's answer differs, at an output that
    is a number in both, from the raw anomaly left unrounded (smooth >= 2: one term rounds the same either way) and, for float64 with
    smooth >= 3, from the window summed newest first or from the newest step and then the oldest up (a few dozen float32 terms of
    similar size add up exactly in float64 in any order)"""
    want, clim = expected(x, group, G, window, smooth, starts)
    assert np.isfinite(want).any(), "no finite output"
    if smooth >= 2 and (x.dtype == np.float32 or np.finfo(np.longdouble).nmant > 52):
        assert differ_finite(anom_model(x, group, clim, smooth, starts, unrounded=True), want), "the (VT) cast of the raw anomaly is invisible"
    if smooth >= 3 and x.dtype == np.float64:
        assert differ_finite(anom_model(x, group, clim, smooth, starts, newest_first=True), want), "the order of the window's additions is invisible"
        assert differ_finite(anom_model(x, group, clim, smooth, starts, rotated=True), want), "the slot the ring's re-add starts from is invisible"
    return want, clim


def ring_edge_case(dtype, smooth):
    """one row of 257 pixels, T = 3 smooth + 7"""
    T = 3 * smooth + 7
    x = slab(np.random.default_rng(100 + smooth), T, (1, 257), dtype)
    return x, run_groups(T), 12, ring_edge_starts(T, smooth)


def tile_edge_case(dtype, smooth, tile, nt, brk):
    """nt steps of 130 pixels with one break: at tile - 1 and tile + 1 a valid window straddles the boundary of the first two tiles,
    at tile one ends on it"""
    x = slab(np.random.default_rng(tile * 7 + smooth), nt, (2, 65), dtype)
    return x, run_groups(nt), 12, [0, brk]


# (G, rule, pixels): seeds for which the case's float64 climatology depends on the order of a group's additions (test_anom_forms_host.py)
CLIM_SEEDS = {(31, "gaps", 1): 2, (65, "gaps", 1): 3, (366, "alternating", 1): 1}


def clim_case(dtype, case):
    G, rule, chunk, window, shape, T = case
    rng = np.random.default_rng(CLIM_SEEDS.get((G, rule, shape[0] * shape[1]), G * 131 + GROUP_RULES.index(rule)))
    group = groups(rule, T, G, rng)
    return slab(rng, T, shape, dtype), group
