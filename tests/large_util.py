"""Sparse giant slabs for tests/test_gpu_consumers_large.py, and what the existing numpy statements say about them.

A slab of T steps is a background byte (what Tracker.memset writes, so the background value is that byte four times, read in the slab's
dtype) plus a few windows (first step, array (n, ny, nx)).  Inside a window only the pixels of a few patches of the plane differ from
the background.  `place` writes such a slab to the device with one memset and one copy per window; `dense` materialises it (small
shapes only); `compact` concatenates the windows in time order and returns the real step of every compact step.

The want_* functions evaluate the statements of spell_util, composite_util, band_util, centred_util, life_util, level_util,
reversal_util, std_util, pfield_util and pctl_util on the windows (and, where a statement loops over pixels in Python, on the patches) and fill in
what the background gives.  tests/test_large_util_host.py proves on a slab that fits (LAYOUT_SMALL) that each equals the statement on
the materialised slab bit for bit, and that it changes when the last two windows are taken away; the GPU test uses the same functions
on LAYOUT_FULL, where nothing could be materialised.  Rules they rest on: an unflagged step adds nothing to a composite, so leaving
it out keeps the order of the float64 additions; a spell never crosses a background step, so the windows' spells are the slab's."""
import ctypes as C

import numpy as np

import band_util
import centred_util
import composite_util
import level_util
import pctl_util
import pfield_util
import reversal_util
import spell_util
import std_util


def _off(p, nbytes):
    return C.c_void_p(p.value + int(nbytes))


class Layout:
    """the shape of a test: the slab, the first steps of its windows (A, B, C, D) and their length, the patches (first pixel, pixels)
    of the plane, and the parameters the entries take that depend on the shape"""

    def __init__(self, T, ny, nx, firsts, n, patches, seg_start, band_rows, std_rows, sectors, level_firsts, level_n, lat, delta):
        self.T, self.ny, self.nx, self.firsts, self.n, self.patches = T, ny, nx, tuple(firsts), n, tuple(patches)
        self.npix = ny * nx
        self.seg_start, self.band_rows, self.std_rows, self.sectors = seg_start, band_rows, std_rows, sectors
        self.nlev = 4
        self.level_steps, self.level_firsts, self.level_n = T // self.nlev, tuple(level_firsts), level_n
        self.lat, self.delta = lat, delta
        assert T % self.nlev == 0 and all(0 <= p and p + k <= self.npix for p, k in patches)
        assert all(a + n < b for a, b in zip(self.firsts, self.firsts[1:] + (T + 1,))), "the windows are apart: a background step between them"
        assert firsts[2] < seg_start < firsts[2] + n and firsts[3] + n == T

    def patch_pixels(self):
        return np.concatenate([np.arange(p, p + k) for p, k in self.patches])

    def ids(self):
        return (np.arange(self.T) % 12).astype(np.int32)

    def reversal_table(self):
        """rows down to the equator are active, so that the patch next to it is read; a positive northern limit lets a pixel of a
        constant background be blocked by its southern gradient alone"""
        return reversal_util.table(self.lat, delta=self.delta, ghgs=0.0, ghgn=1.0, lat_bounds=(0, 75))


# the shape of tests/test_gpu_frequency_large.py.  Patches: the start of the plane, that test's odd block (row 359), the end of the
# plane -- and 1 801 pixels from row 360 into row 361, the band of the std and percentile entries, which the other three do not touch
LAYOUT_FULL = Layout(4200, 721, 1440, (100, 2060, 4128, 4200 - 24), 24,
                     ((0, 512), (517_003, 1_001), (360 * 1440 + 7, 1_801), (721 * 1440 - 515, 515)),
                     seg_start=4140, band_rows=(300, 420), std_rows=(360, 362), sectors=[(1400, 100), (0, 1440)],
                     level_firsts=(5, 514, 1031, 1044), level_n=6, lat=reversal_util.grid(0.25), delta=15.0)
# the same scaled down to a slab that fits a host array
LAYOUT_SMALL = Layout(60, 9, 40, (2, 18, 40, 54), 6, ((0, 6), (3 * 40 + 13, 11), (4 * 40 + 3, 45), (9 * 40 - 7, 7)),
                      seg_start=43, band_rows=(3, 7), std_rows=(4, 6), sectors=[(35, 10), (0, 40)],
                      level_firsts=(1, 5, 9, 13), level_n=2, lat=reversal_util.grid(22.5), delta=22.5)


class Sparse:
    def __init__(self, T, ny, nx, byte, dtype, windows):
        self.T, self.ny, self.nx, self.byte, self.dtype = T, ny, nx, int(byte), np.dtype(dtype)
        self.windows = sorted(((int(t0), np.ascontiguousarray(a, dtype=self.dtype)) for t0, a in windows), key=lambda w: w[0])
        assert self.dtype.itemsize == 4 and all(a.shape[1:] == (ny, nx) and t0 + len(a) <= T for t0, a in self.windows)

    @property
    def background(self):
        return np.frombuffer(bytes([self.byte]) * 4, dtype=self.dtype)[0]

    def without(self, *which):
        """the slab without the windows of those indices (background in their place)"""
        return Sparse(self.T, self.ny, self.nx, self.byte, self.dtype, [w for k, w in enumerate(self.windows) if k not in which])

    def dense(self):
        a = np.full((self.T, self.ny, self.nx), self.background, dtype=self.dtype)
        for t0, w in self.windows:
            a[t0:t0 + len(w)] = w
        return a

    def steps(self):
        """the real step of every compact step"""
        return np.concatenate([np.arange(t0, t0 + len(w)) for t0, w in self.windows]) if self.windows else np.zeros(0, dtype=np.int64)

    def compact(self, pixels=None):
        """(the windows concatenated in time order, steps()); pixels: only those of the flattened plane, as (steps, 1, len(pixels))"""
        if pixels is None:
            parts = [w for _, w in self.windows]
            return (np.concatenate(parts) if parts else np.zeros((0, self.ny, self.nx), self.dtype)), self.steps()
        parts = [w.reshape(len(w), -1)[:, pixels][:, None, :] for _, w in self.windows]
        return (np.concatenate(parts) if parts else np.zeros((0, 1, len(pixels)), self.dtype)), self.steps()

    def rows(self, y0, y1):
        """the host copy of rows [y0, y1) of every step: (T, y1 - y0, nx)"""
        a = np.full((self.T, y1 - y0, self.nx), self.background, dtype=self.dtype)
        for t0, w in self.windows:
            a[t0:t0 + len(w)] = w[:, y0:y1]
        return a


def place(trk, dev_ptr, spec):
    """the slab into device memory at dev_ptr: one memset, one copy per window"""
    plane = spec.ny * spec.nx * 4
    trk.memset(dev_ptr, spec.byte, spec.T * plane)
    for t0, w in spec.windows:
        trk.h2d(_off(dev_ptr, t0 * plane), w)


# ---- window contents ------------------------------------------------------------------------------------------------------------------
def flag_spec(L, seed=0):
    """spell_util.spell_flags (ids 1..3 with id changes) on the patch pixels of every window, 0 elsewhere"""
    px = L.patch_pixels()
    wins = []
    for k, t0 in enumerate(L.firsts):
        a = np.zeros((L.n, L.npix), dtype=np.int32)
        a[:, px] = spell_util.spell_flags(L.n, 1, len(px), seed=seed + k)[:, 0, :]
        wins.append((t0, a.reshape(L.n, L.ny, L.nx)))
    return Sparse(L.T, L.ny, L.nx, 0, np.int32, wins)


def field_spec(L, seed=0, byte=0x3f, firsts=None, n=None):
    """float32 of wide magnitude (normal x 10**uniform(-8, 10), as centred_util.wide_case) with one NaN in a hundred on the patch
    pixels of every window; the background (byte 0x3f four times: 0.747...) elsewhere"""
    rng = np.random.default_rng(1000 + seed)
    px = L.patch_pixels()
    firsts, n = L.firsts if firsts is None else firsts, L.n if n is None else n
    bg = np.frombuffer(bytes([byte]) * 4, dtype=np.float32)[0]
    wins = []
    for t0 in firsts:
        v = (rng.standard_normal((n, len(px))) * 10.0 ** rng.uniform(-8, 10, (n, len(px)))).astype(np.float32)
        v[rng.random(v.shape) < 0.01] = np.nan
        a = np.full((n, L.npix), bg, dtype=np.float32)
        a[:, px] = v
        wins.append((t0, a.reshape(n, L.ny, L.nx)))
    return Sparse(L.T, L.ny, L.nx, byte, np.float32, wins)


def level_spec(L, seed=7):
    """the input of the level mean, (level_steps, nlev, ny, nx) seen as T planes: windows of level_n steps, background 0.0"""
    return field_spec(L, seed=seed, byte=0, firsts=[s * L.nlev for s in L.level_firsts], n=L.level_n * L.nlev)


def solid_spec(L, zero_t=10, block_back=15):
    """the slab of tests/test_gpu_frequency_large.py as (byte, [(first element, elements) zeroed]): every byte 0x01, the last zero_t
    steps zeroed, and the pixels of the second patch in step T - block_back"""
    p0, k = L.patches[1]
    return 0x01, [((L.T - zero_t) * L.npix, zero_t * L.npix), ((L.T - block_back) * L.npix + p0, k)]


def place_solid(trk, dev_ptr, L, zero_t=10, block_back=15):
    byte, zeros = solid_spec(L, zero_t, block_back)
    trk.memset(dev_ptr, byte, L.T * L.npix * 4)
    for e0, n in zeros:
        trk.memset(_off(dev_ptr, e0 * 4), 0, n * 4)


def solid_dense(L, zero_t=10, block_back=15):
    byte, zeros = solid_spec(L, zero_t, block_back)
    a = np.full(L.T * L.npix, np.frombuffer(bytes([byte]) * 4, dtype=np.int32)[0], dtype=np.int32)
    for e0, n in zeros:
        a[e0:e0 + n] = 0
    return a.reshape(L.T, L.ny, L.nx)


# ---- what the statements say ----------------------------------------------------------------------------------------------------------
def spell_lists(L, flag, by_id, segments):
    """spell_util.spell_list of every window on the patch pixels, onsets in real steps, x = pixel of the flattened plane (y = 0)"""
    px = L.patch_pixels()
    parts = []
    for t0, w in flag.windows:
        local = [s - t0 for s in (segments or []) if t0 < s < t0 + len(w)]          # (a start on the window's first step changes nothing)
        on, d, y, x = spell_util.spell_list(w.reshape(len(w), 1, -1)[:, :, px], 0, by_id, local or None)
        parts.append((on + t0, d, y, px[x]))
    if not parts:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(4))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def want_spells(L, lists, ids, G, min_duration):
    """(events, steps, longest) uint32 (G, ny, nx): the windows' spells summed and maxed in the group of their real onset"""
    maps = spell_util.maps_of(lists, (L.T, 1, L.npix), ids, G, min_duration)
    return tuple(m.reshape(G, L.ny, L.nx).astype(np.uint32) for m in maps)


def want_spells_solid(L, ids, G, min_duration, zero_t=10, block_back=15):
    """one spell of T - zero_t steps per pixel in the group of step 0; in the block two, of T - block_back and block_back - zero_t - 1"""
    p0, k = L.patches[1]
    tb = L.T - block_back
    on = np.concatenate([np.zeros(L.npix - k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.full(k, tb + 1, dtype=np.int64)])
    rest = np.concatenate([np.arange(0, p0), np.arange(p0 + k, L.npix)])
    d = np.concatenate([np.full(L.npix - k, L.T - zero_t), np.full(k, tb), np.full(k, block_back - zero_t - 1)]).astype(np.int64)
    x = np.concatenate([rest, np.arange(p0, p0 + k), np.arange(p0, p0 + k)])
    return want_spells(L, (on, d, np.zeros_like(x), x), ids, G, min_duration)


def want_composite(L, flag, field, ids, G, skipna):
    """composite_util.composite on the compact slabs, patch pixels only (no flag elsewhere: sum +0.0, n 0), with compact ids"""
    px = L.patch_pixels()
    cf, steps = flag.compact(px)
    cx, steps_x = field.compact(px)
    assert np.array_equal(steps, steps_x)
    s, n = composite_util.composite(cf, cx, None if ids is None else np.asarray(ids)[steps], G, 0, skipna)
    S, N = np.zeros((G, L.npix), dtype=np.float64), np.zeros((G, L.npix), dtype=np.uint32)
    S[:, px], N[:, px] = s[:, 0], n[:, 0]
    return S.reshape(G, L.ny, L.nx), N.reshape(G, L.ny, L.nx)


def want_band(L, flag, field, w):
    """band_util.band per window; count 0 and +0.0 on every other step"""
    y0, y1 = L.band_rows
    out = None
    xw = dict(field.windows)
    for t0, fw in flag.windows:
        part = band_util.band(fw, y0, y1, w, 0, xw[t0], L.sectors, True)
        if out is None:
            out = {k: np.zeros((L.T,) + v.shape[1:], dtype=v.dtype) for k, v in part.items()}
        for k, v in part.items():
            out[k][t0:t0 + len(fw)] = v
    if out is None:
        z = np.zeros((1, L.ny, L.nx))
        out = {k: np.zeros((L.T,) + v.shape[1:], dtype=v.dtype) for k, v in band_util.band(z.astype(np.int32), y0, y1, w, 0, z.astype(np.float32), L.sectors, True).items()}
    return out


def stamps(L, field, seed=0, R=40, nbins=3, marks=()):
    """about R stamps (t sorted, row, col, bin in [-1, nbins)) on the window steps at patch pixels; marks: (step, pixel) pairs to include"""
    rng = np.random.default_rng(seed)
    steps, px = field.steps(), L.patch_pixels()
    t = list(rng.choice(steps, R - len(marks))) + [m[0] for m in marks]
    p = list(rng.choice(px, R - len(marks))) + [m[1] for m in marks]
    order = np.argsort(np.array(t), kind="stable")
    t, p = np.array(t, dtype=np.int64)[order], np.array(p, dtype=np.int64)[order]
    bins = rng.integers(-1, nbins, R).astype(np.int32)
    bins[:nbins + 1] = np.arange(-1, nbins)                                         # every bin and the dropped one are there
    return t, (p // L.nx).astype(np.int32), (p % L.nx).astype(np.int32), bins


def want_centred(L, field, st, nbins, hy, hx, skipna):
    """centred_util.centred on the compact field with the stamps' steps translated"""
    t, row, col, bins = st
    cx, steps = field.compact()
    tc = np.searchsorted(steps, t)
    keep = (tc < len(steps)) & (steps[np.minimum(tc, len(steps) - 1)] == t) if len(steps) else np.zeros(len(t), dtype=bool)
    if not keep.all():                                                              # a stamp on a background step (a window taken away)
        bgx = np.full((1, L.ny, L.nx), field.background, dtype=field.dtype)
        cx = np.concatenate([cx, bgx])
        tc = np.where(keep, tc, len(steps))
    return centred_util.centred(cx, tc, row, col, bins, nbins, hy, hx, True, skipna)


def want_level(L, spec, weights, skipna):
    """[(first step, level_util.level_mean of the window (n, ny, nx))]; every other step is the statement on a zero step: +0.0"""
    return [(t0 // L.nlev, level_util.level_mean(w.reshape(-1, L.nlev, L.ny, L.nx), weights, skipna)) for t0, w in spec.windows]


def want_reversal(L, field, tab, mask):
    """[(first step, reversal_util.from_table of the window)]; a constant plane has no gradient: 0 on every other step"""
    return [(t0, reversal_util.from_table(w, tab, mask)) for t0, w in field.windows]


def fill_windows(T, ny, nx, dtype, wins):
    a = np.zeros((T, ny, nx), dtype=dtype)
    for t0, w in wins:
        a[t0:t0 + len(w)] = w
    return a


def nonzero_words(wins):
    """the 32-bit words of the windows that are not 0 (what checksum_i32 counts)"""
    return int(sum(np.count_nonzero(np.ascontiguousarray(w).view(np.int32)) for _, w in wins))


def want_std(L, field, group, G, W, ddof, skipna):
    """std_util.want_std on the host copy of the band (T, rows, nx)"""
    y0, y1 = L.std_rows
    return std_util.want_std(field.rows(y0, y1), (0, y1 - y0), group, G, W, ddof, skipna)[0]


def life_field_spec(L, seed=3):
    """the field of the lifecycle entry: 300 + 150 x normal on the patch pixels of every window, no NaN (a NaN would turn every sum of
    its id into NaN), the same background"""
    rng = np.random.default_rng(2000 + seed)
    px = L.patch_pixels()
    spec = field_spec(L, seed)
    wins = []
    for t0, a in spec.windows:
        a = a.reshape(len(a), -1).copy()
        a[:, px] = (300.0 + 150.0 * rng.standard_normal((len(a), len(px)))).astype(np.float32)
        wins.append((t0, a.reshape(len(a), L.ny, L.nx)))
    return Sparse(L.T, L.ny, L.nx, spec.byte, np.float32, wins)


def life_wrow(L):
    """float32 row weights in eighths between 1 and 2: their float64 sums are exact in any order, so the areas compare exactly"""
    return (1.0 + (np.arange(L.ny) % 7) / 8.0).astype(np.float32)


def want_life(L, flag, field, wrow):
    """life_util.numpy_rows per window, t in real steps, sorted by (label, t) as the entry returns them; a background step has no id
    and no row"""
    import life_util
    xw = dict(field.windows)
    parts = []
    for t0, fw in flag.windows:
        r = life_util.numpy_rows(fw, xw[t0], wrow)
        r["t"] += t0
        parts.append(r)
    rows = np.concatenate(parts) if parts else life_util.numpy_rows(np.zeros((1, L.ny, L.nx), np.int32), np.zeros((1, L.ny, L.nx), np.float32), wrow)
    return rows[np.lexsort((rows["t"], rows["label"]))]


def want_life_exact(L, flag, field, wrow, rows):
    """life_util.numpy_exact_rows of `rows` (real steps), each evaluated inside its window"""
    import life_util
    xw = dict(field.windows)
    out = []
    for r in rows:
        t0, fw = next((t0, fw) for t0, fw in flag.windows if t0 <= r["t"] < t0 + len(fw))
        local = np.array([r])
        local["t"] -= t0
        out.append(life_util.numpy_exact_rows(fw, xw[t0], wrow, local, extent=True))
    return np.concatenate(out)


# The windows are 96 of the 4200 steps, and at a patch pixel about seven in ten of their values lie below the background: at q = 0.9 every
# pool's quantile IS the background, whatever the windows hold.  At PCTL_QS[1:] it is one of the windows' values, below and above it.
PCTL_QS = (0.9, 0.005, 0.998)


def want_pfield(L, field, group, G, W, qs=PCTL_QS):
    """pfield_util.want_field on the host copy of the band: (len(qs), G, rows, nx)"""
    y0, y1 = L.std_rows
    return pfield_util.want_field(field.rows(y0, y1), (0, y1 - y0), group, G, W, list(qs))


def want_pgroups(L, field, group, G, W, qs=PCTL_QS):
    """pctl_util.want on the host copy of the band: (len(qs), G)"""
    y0, y1 = L.std_rows
    band = field.rows(y0, y1)
    return np.stack([pctl_util.want(band, (0, y1 - y0), group, G, W, q) for q in qs])
