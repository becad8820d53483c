"""Constructed slabs for the capacity and length rules of the time-shard exchange path (contrack_amd/csrc/ctk_sharded.hip), and a plain
numpy / scipy.ndimage restatement of what every exchange of a ctk_track_sharded_* call should see for given cuts.

The fields are exact rectangles and isolated pixels on small grids, static in time unless said otherwise, so that their counts are
designed: every case carries the numbers it was built for (`design`), tests/test_shard_forms_host.py compares them with the
restatement on the CPU, and tests/test_gpu_shard_forms.py compares the restatement with what the library reports through
ctk_debug_shard_exchange.  TEST INFRASTRUCTURE: nothing here is imported by contrack_amd/.

The rules restated (constants of ctk_sharded.hip / ctk_kernels.hip):
  capB        capacity for the 2-D components of a cut step.  Starts at 256 in every call; every rank's last step counts (the header
              of the filter exchange carries it, the last rank's too); grows once to n + n/2 + 64.
  capC, capD  shared seam group records / labels per rank: max(remembered hint of any rank, 256), capD rounded up to a multiple of
              4; when some rank's true counts exceed them both grow to n + n/2 + 64 (capD rounded again) and the exchange is repeated.
  records     seam rows (x = 0 and x = nx - 1 both kept foreground) of a shard, run-length grouped by (t, consecutive y, label pair).
              A row whose two ends carry the SAME 3-D label only counts when that label is marked: it meets another label on some
              row of the shard, or it reaches a cut.  A group is shared when its cluster (labels united through rows with two
              different labels, per shard) holds a label that reaches one of the shard's two cuts.
  labels      the labels of the shared groups and every label that reaches one of the shard's cuts.
  ne          ids whose time extent is exchanged: the union of all ranks' shared labels.
  workgroups  k_sh_pack_ext: 32 while ne <= 2048 (or the hook's cap), else 1.
  sample      a rank sees a background pixel if one lies in the first min(T * ny * W, 16384) mask words of its shard.
"""
import functools

import numpy as np
from scipy import ndimage

from cpu_tables import label_step

CTK_CI_BLOCK = 1024                   # ctk_kernels.hip: k_compact_init sums in two levels beyond 4 * CTK_CI_BLOCK steps
CI_TWO_LEVEL = 4 * CTK_CI_BLOCK
CAP0 = 256                            # capB, and the floor of capC / capD
PACK_SHARED_CHUNK = 1024              # k_sh_pack_shared: steps per trip, offsets carried from trip to trip
SH_PE_LDS, SH_PE_BLOCKS = 2048, 32
BG_SAMPLE_WORDS = 16384
PREINIT_MIN = 1024                    # seam tables are initialised ahead only for at least this many labels
THR = 0.5                             # foreground = 1.0, background = 0.0, compared with >=

_TRACK = np.zeros((3, 3, 3), dtype=int)
_TRACK[1] = 1
_TRACK[0, 1, 1] = _TRACK[2, 1, 1] = 1


def grow(n):
    return n + n // 2 + 64


def round4(n):
    return (n + 3) & ~3


def tables_held(nt):
    """labels the ten label-indexed seam tables hold after a call with nt = NL + 2 grew all of them (buffers get need + need / 8 + 256
    bytes; the 24-byte boxes are the tightest)"""
    return (27 * nt + 256) // 24


class Case:
    def __init__(self, name, T, ny, nx, cuts, pers, f64=False):
        assert cuts[0] == 0 and cuts[-1] == T and all(b > a for a, b in zip(cuts, cuts[1:]))
        self.name, self.cuts, self.pers, self.f64 = name, list(cuts), pers, f64
        self.m = np.zeros((T, ny, nx), dtype=bool)
        self.overlap = 0.5
        self.ids = 0                  # designed: ids in the final flag
        self.design = {}              # designed counts the restatement must reproduce (see test_shard_forms_host.py)

    # ---- building blocks -----------------------------------------------------------------------------------------
    def clip(self, t0, t1):
        return max(t0, 0), min(t1, self.m.shape[0])

    def pixels(self, n, t0, t1, y0, x0=0):
        """n isolated pixels at spacing 2, raster order from row y0 (every other row, every other column from x0)"""
        T, ny, nx = self.m.shape
        t0, t1 = self.clip(t0, t1)
        per_row = (nx - x0) // 2
        assert n <= per_row * ((ny - y0 + 1) // 2), "plane too small"
        for k in range(n):
            y, x = y0 + 2 * (k // per_row), x0 + 2 * (k % per_row)
            assert x < nx - 1 and not self.m[t0:t1, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any()
            self.m[t0:t1, y, x] = True
        return y0 + 2 * ((n + per_row - 1) // per_row)          # first row that is free again (one empty row in between)

    def left(self, y, a, t0, t1):
        t0, t1 = self.clip(t0, t1)
        self.m[t0:t1, y, :a] = True

    def right(self, y, b, t0, t1):
        t0, t1 = self.clip(t0, t1)
        self.m[t0:t1, y, self.m.shape[2] - b:] = True

    def bar(self, y, a, b, t0, t1):
        """a straddling bar: two 3-D labels, one seam group per step, one merge"""
        self.left(y, a, t0, t1)
        self.right(y, b, t0, t1)

    def block(self, y0, y1, x0, x1, t0, t1):
        t0, t1 = self.clip(t0, t1)
        self.m[t0:t1, y0:y1, x0:x1] = True

    # ---- what the calls take ----------------------------------------------------------------------------------------
    @property
    def shape(self):
        return self.m.shape

    def field(self):
        return self.m.astype(np.float64 if self.f64 else np.float32)

    def thr(self):
        return np.full(self.m.shape[0], THR, dtype=np.float64)

    def wrow(self):
        ny = self.m.shape[1]
        lat = np.linspace(60.0, -60.0, ny).astype(np.float32)
        return np.array(111 * np.float32(1.0) * 111 * np.float32(1.0) * np.cos(lat * np.pi / 180)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _seam_merged(m2d):
    """2-D labels with the components that face each other across the seam united (contrack.py:691-698)"""
    lab, n = label_step(m2d)
    par = list(range(n + 1))

    def find(i):
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i
    for y in np.nonzero((lab[:, 0] > 0) & (lab[:, -1] > 0))[0]:
        a, b = find(int(lab[y, 0])), find(int(lab[y, -1]))
        if a != b:
            par[max(a, b)] = min(a, b)
    if n:
        lab = np.array([find(i) for i in range(n + 1)], dtype=np.int32)[lab]
    return lab


def filtered(m, wrow, overlap):
    """the two-sided overlap filter (contrack.py:706-742): steps 1 .. T-2 in order, backward overlap against the already filtered
    step, forward against the unfiltered one.  The fractions of the constructed fields are far from `overlap`, so the order of
    the floating-point sums does not matter.  Identical (previous, current, next) planes are evaluated once."""
    T = m.shape[0]
    kept = m.copy()
    wg = np.asarray(wrow, dtype=np.float64)[:, None] * np.ones(m.shape[2])
    memo = {}
    for t in range(1, T - 1):
        key = (kept[t - 1].tobytes(), m[t].tobytes(), m[t + 1].tobytes())
        if key not in memo:
            lab = _seam_merged(m[t])
            out = m[t].copy()
            idx = np.unique(lab[lab > 0])
            if len(idx):
                area = ndimage.sum(wg, lab, idx)
                bwd = ndimage.sum(wg * kept[t - 1], lab, idx)
                fwd = ndimage.sum(wg * m[t + 1], lab, idx)
                for i, a, b, f in zip(idx, area, bwd, fwd):
                    fb, ff = b / a, f / a
                    drop = (fb != 0 and fb < overlap) or (ff != 0 and ff < overlap)
                    if drop:
                        out[lab == i] = False
            memo[key] = out
        kept[t] = memo[key]
    return kept


def _groups_of_rank(lab3, t0, t1, marks):
    """-> (shared group records, labels sent, all group records, clusters of the shared groups as frozensets)"""
    a, b = lab3[t0:t1, :, 0], lab3[t0:t1, :, -1]
    tt, yy = np.nonzero((a > 0) & (b > 0))                      # (t, y) order
    rows = [(int(t), int(y), int(a[t, y]), int(b[t, y])) for t, y in zip(tt, yy)]
    par = {}

    def find(i):
        par.setdefault(i, i)
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i
    marked = set(marks)
    for _, _, l, r in rows:
        if l != r:
            marked.update((l, r))
            p, q = find(l), find(r)
            if p != q:
                par[max(p, q)] = min(p, q)
    groups = []
    prev = None
    for t, y, l, r in rows:
        valid = l != r or l in marked
        if valid and not (prev is not None and prev == (t, y - 1, l, r)):
            groups.append((t, y, l, r))
        prev = (t, y, l, r) if valid else None
    shared_roots = {find(l) for l in marks}
    sh = [g for g in groups if find(g[2]) in shared_roots]
    labels = set(marks)
    for _, _, l, r in sh:
        labels.update((l, r))
    return sh, labels, groups, find


def restate(case, cap_lds=SH_PE_LDS):
    """what the exchanges of a sharded call over case.cuts should see; per-rank lists are indexed by rank"""
    m, cuts = case.m, case.cuts
    T, ny, nx = m.shape
    world = len(cuts) - 1
    W = (nx + 63) // 64
    kept = filtered(m, case.wrow(), case.overlap)
    lab3, NL = ndimage.label(kept, structure=_TRACK)
    lab3 = lab3.astype(np.int32)
    nlast = [label_step(m[cuts[r + 1] - 1])[1] for r in range(world)]
    nh = [0] + nlast[:-1]
    mx = max(nlast)
    out = dict(world=world, NL=int(NL), nlast=nlast, nh=nh, capB=CAP0 if mx <= CAP0 else grow(mx), capB_repeats=int(mx > CAP0))
    on_step = lambda t: set(int(v) for v in np.unique(lab3[t]) if v > 0)
    marks = []
    for r in range(world):
        s = set()
        if r > 0:
            s |= on_step(cuts[r] - 1)
        if r + 1 < world:
            s |= on_step(cuts[r + 1] - 1)
        marks.append(s)
    crossing = [sorted(on_step(cuts[r + 1] - 1)) for r in range(world - 1)]
    out["crossing"] = crossing
    out["any_boundary"] = any(len(c) for c in crossing)
    recs, labs, allrec, glob, pairs = [], [], [], set(), []
    for r in range(world):
        sh, labels, groups, _ = _groups_of_rank(lab3, cuts[r], cuts[r + 1], marks[r])
        recs.append(len(sh)); labs.append(len(labels)); allrec.append(len(groups))
        glob |= labels
        pairs += [(l, q) for _, _, l, q in sh if l != q]
    if not out["any_boundary"]:
        recs, labs, glob = [0] * world, [0] * world, set()
    out.update(sent_records=recs, sent_labels=labs, all_records=allrec, ne=len(glob))
    # operations of the shared clusters: every label of a cluster but one is relabelled once (all pieces are rectangles inside
    # their own boxes, so one relabel removes a label for good)
    par = {}

    def find(i):
        par.setdefault(i, i)
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i
    for l, q in pairs:
        p, s = find(l), find(q)
        if p != s:
            par[max(p, s)] = min(p, s)
    out["shared_ops"] = len(par) - len({find(i) for i in par})
    out["pack_ext_workgroups"] = SH_PE_BLOCKS if out["ne"] <= cap_lds else 1
    # background sample
    seen = []
    for r in range(world):
        rows = m[cuts[r]:cuts[r + 1]].reshape(-1, nx)
        nwords = min(rows.shape[0] * W, BG_SAMPLE_WORDS)
        full, rest = divmod(nwords, W)
        z = not rows[:full].all()
        if rest:
            z = z or not rows[full, :64 * rest].all()
        seen.append(bool(z))
    out["zero_in_sample"] = seen
    out["zero_exchanged"] = int(not any(seen))
    return out


def seam_caps(hint_c, hint_d, sent_records, sent_labels):
    """-> (capC, capD, repeats) of the shared seam exchange from the largest remembered hints and the ranks' true counts"""
    capC, capD = max(hint_c, CAP0), round4(max(hint_d, CAP0))
    mc, md = max(sent_records), max(sent_labels)
    if mc <= capC and md <= capD:
        return capC, capD, 0
    return max(capC, grow(mc)), round4(max(capD, grow(md))), 1


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def _capb(n, where, nx=64, f64=False, shrink=False, halo_only=False):
    """n components in ONE cut step: 3 static bars (6 components) + isolated pixels that live on the cut step and the step behind
    it.  where = 0: the cut behind rank 0; 1: between the two middle ranks of four.  halo_only: three ranks, the middle one a
    single step whose halo is the crowded step.  shrink: a block that at the cut shrinks to a quarter and moves half aside: the
    component in front of the cut is dropped (forward overlap 1/4), which the rank behind the cut learns in the second round --
    its first step then has NO backward overlap and stays (with the first guess "all kept" it had 1/4 and was dropped)."""
    if halo_only:
        T, cuts, c = 7, [0, 3, 4, 7], 3
    else:
        T, cuts, c = 8, [0, 2, 4, 6, 8], (2, 4)[where]
    k = Case("capb", T, 56, nx, cuts, 2, f64)
    for y in (1, 3, 5):
        k.bar(y, 3, 2, 0, T)
    npx = n - 6 - (1 if shrink else 0)
    k.pixels(npx, *((c - 2, c) if halo_only else (c - 1, c + 1)), 8)      # (halo_only: gone behind the cut)
    k.ids = 3 + npx
    if shrink:
        k.block(48, 52, 10, 18, 0, c)                # 32 pixels up to the cut step ...
        k.block(48, 52, 16, 24, c, T)                # ... 32 behind it, 8 in common
        k.ids += (1 if c - 1 >= k.pers else 0) + 1
    k.design = dict(cut=cuts.index(c) - 1, n=n, capB=CAP0 if n <= CAP0 else grow(n), repeats=int(n > CAP0))
    return k


def _bars(nb, extra=None):
    """nb static bars across the only cut -> 2 nb shared labels, nb records per step (two steps per rank); extra: 'pixel' one plain
    label across the cut, 'touch' a bar whose halves touch (a full row: ONE label, but a record per step because it reaches the
    cut).  One more bar lives on the first step only: a local cluster of rank 0, driven on the device, whose record the shared
    ones have to step over."""
    T, cuts = 4, [0, 2, 4]
    k = Case("bars", T, 2 * nb + 8, 64, cuts, 1)
    for i in range(nb):
        k.bar(2 * i + 1, 3, 2, 0, T)
    if extra == "pixel":
        k.pixels(1, 0, T, 2 * nb + 2, x0=10)
    elif extra == "touch":
        k.bar(2 * nb + 2, 32, 32, 0, T)
    k.bar(2 * nb + 5, 2, 3, 0, 1)
    e = 1 if extra else 0
    te = 1 if extra == "touch" else 0
    k.ids = nb + e + 1
    k.design = dict(labels=2 * nb + e, records=[2 * (nb + te), 2 * (nb + te)], local_records=[1, 0], shared_ops=nb)
    return k


def _longbar(steps):
    """one bar alive on `steps` steps of rank 0 and on the first step of rank 1; a local bar in the middle of rank 0"""
    T = steps + 4
    k = Case("longbar", T, 16, 64, [0, steps + 1, T], 2)
    k.bar(1, 3, 2, 1, steps + 2)
    k.bar(5, 2, 2, 3, 6)
    k.ids = 2
    k.design = dict(labels=2, records=[steps, 1], local_records=[3, 0], shared_ops=1)
    return k


def _ext_natural(n, pers):
    """n ids across the only cut: n - 2 isolated pixels and one bar, all static over the four steps"""
    k = Case("ext_natural", 4, 130, 64, [0, 2, 4], pers)
    k.pixels(n - 2, 0, 4, 0)
    k.bar(129, 3, 2, 0, 4)
    k.ids = n - 1 if pers <= 4 else 0
    k.design = dict(ne=n, labels=n, workgroups=SH_PE_BLOCKS if n <= SH_PE_LDS else 1)
    return k


def _ext_small():
    """40 ids across the cut, and ids of either rank's own right below the first and right above the last of them (the two ends of
    the search for "is this id shared" in k_sh_pack_ext)"""
    T = 6
    k = Case("ext_small", T, 16, 64, [0, 3, 6], 2)
    k.pixels(1, 0, 2, 0)                             # id 1: rank 0's own, gone before the cut
    k.pixels(38, 0, T, 2)                            # ids 2 .. 39 (rows 2 and 4)
    k.bar(7, 3, 2, 0, T)                             # ids 40, 41
    k.pixels(1, 0, 2, 15, x0=62)                     # id 42: rank 0's own, the last of step 0
    k.pixels(1, 3, 5, 0, x0=4)                       # rank 1's own, born behind the cut
    k.pixels(1, 4, 6, 15, x0=58)
    k.ids = 1 + 38 + 1 + 1 + 2
    k.design = dict(ne=40, labels=40, workgroups=SH_PE_BLOCKS)
    return k


def _background(kind):
    """nx = 72: two mask words per row, 8 valid bits in the second"""
    if kind == "full":
        k = Case("bg", 6, 8, 72, [0, 2, 4, 6], 2)
        k.m[:] = True
    else:
        k = Case("bg", 44, 210, 72, [0, 2, 42, 44], 2)          # rank 1: 40 x 210 x 2 = 16800 words > 16384
        k.m[:] = True
        t, y = dict(beyond=(41, 209), inside=(2, 0), last_rank=(43, 209))[kind]
        k.m[t, y, 71] = False
    k.ids = 1
    k.design = dict(zero_exchanged=int(kind in ("full", "beyond")), hole=kind != "full")
    return k


def _pre_big():
    """1030 labels: at least 1024 (the tables are initialised ahead from the second call on), with bars across the cut"""
    k = Case("pre_big", 4, 80, 64, [0, 2, 4], 2)
    for y in (1, 3, 5):
        k.bar(y, 3, 2, 0, 4)
    k.pixels(1024, 0, 4, 8)
    k.ids = 3 + 1024
    k.design = dict(NL=1030)
    return k


def _ops(nb):
    """nb bars across both cuts of three ranks: nb shared operations; one bar inside rank 1 that reaches neither cut"""
    T = 9
    k = Case("ops", T, 2 * nb + 8, 72, [0, 3, 6, 9], 2)
    for i in range(nb):
        k.bar(2 * i + 1, 3, 2, 0, T)
    k.bar(2 * nb + 3, 2, 3, 3, 5)
    k.ids = nb + 1
    k.design = dict(shared_ops=nb, labels=2 * nb, records=[3 * nb] * 3, local_records=[0, 2, 0])
    return k


def _shapes(kind):
    if kind == "nine":
        T, cuts = 9, list(range(10))
    elif kind == "first":
        T, cuts = 6, [0, 1, 6]
    else:
        T, cuts = 6, [0, 5, 6]
    k = Case("shapes", T, 16, 72, cuts, 3)
    for y in (1, 3, 5):
        k.bar(y, 3, 2, 0, T)
    k.pixels(20, 0, T, 8)
    k.pixels(5, 2, 5, 10, x0=40)                     # three steps: they just survive persistence 3
    k.pixels(4, 1, 3, 12)                            # two steps: they do not
    k.ids = 3 + 20 + 5
    k.design = dict(NL=6 + 20 + 5 + 4)
    return k


LONG_WINDOWS = ((5, 6), (1020, 1031), (2040, 2061), (4090, 4100))      # steps (of the long shard) with a seam row of the shared bar
LONG_LOCAL = ((1010, 1023), (2030, 2050))                              # ... of the local bar


def _long(L, pos):
    """a shard of L steps as rank `pos` of two (the other shard: three steps).  Row 1: a left piece that lives for ever (it reaches
    the cut) and right pieces that come and go -- every window is a label of its own merged into the left one, the first window a
    single step, so its only record is the very first of the payload.  Row 5: a bar that never reaches a cut."""
    off = 3 * pos
    T = L + 3
    k = Case("long", T, 16, 64, [0, L, T] if pos == 0 else [0, 3, T], 2)
    k.left(1, 8, 0, T)
    nwin = 0
    for a, b in LONG_WINDOWS:
        if a + off < T:
            k.right(1, 2, a + off, b + off)
            nwin += 1
    nloc = 0
    for a, b in LONG_LOCAL:
        if a + off < T:
            k.bar(5, 3, 3, a + off, b + off)
            nloc += 1
    k.ids = 1 + nloc
    lo, hi = off, off + L                                              # the long shard's steps
    inside = lambda a, b: max(0, min(b + off, hi, T) - max(a + off, lo))
    k.design = dict(long_rank=pos, records=sum(inside(a, b) for a, b in LONG_WINDOWS if a + off < T),
                    local_records=sum(inside(a, b) for a, b in LONG_LOCAL if a + off < T), shared_ops=nwin, L=L)
    return k


LONG_LENGTHS = (PACK_SHARED_CHUNK, PACK_SHARED_CHUNK + 1, 2100, CI_TWO_LEVEL - 1, CI_TWO_LEVEL, CI_TWO_LEVEL + 1)

BUILDERS = {}
for _n in (255, 256, 257, 600):
    for _w in (0, 1):
        BUILDERS["capb_%d_cut%d" % (_n, _w)] = functools.partial(_capb, _n, _w, nx=(64, 72)[_w])
BUILDERS["capb_257_nx128"] = functools.partial(_capb, 257, 1, nx=128)
BUILDERS["capb_257_halo_only"] = functools.partial(_capb, 257, 0, halo_only=True)
BUILDERS["capb_257_shrink"] = functools.partial(_capb, 257, 1, shrink=True)
BUILDERS["capb_257_f64"] = functools.partial(_capb, 257, 0, f64=True)
BUILDERS["longbar_256"] = functools.partial(_longbar, 256)
BUILDERS["longbar_257"] = functools.partial(_longbar, 257)
BUILDERS["bars_128"] = functools.partial(_bars, 128)
BUILDERS["bars_128_pixel"] = functools.partial(_bars, 128, "pixel")
BUILDERS["bars_128_touch"] = functools.partial(_bars, 128, "touch")
BUILDERS["bars_129"] = functools.partial(_bars, 129)
BUILDERS["bars_5"] = functools.partial(_bars, 5)
for _L in LONG_LENGTHS:
    for _p in (0, 1):
        BUILDERS["long_%d_rank%d" % (_L, _p)] = functools.partial(_long, _L, _p)
for _n in (2048, 2049):
    for _p in (4, 5):
        BUILDERS["ext_%d_pers%d" % (_n, _p)] = functools.partial(_ext_natural, _n, _p)
BUILDERS["ext_small"] = _ext_small
for _k in ("full", "beyond", "inside", "last_rank"):
    BUILDERS["bg_" + _k] = functools.partial(_background, _k)
BUILDERS["pre_big"] = _pre_big
BUILDERS["ops_5"] = functools.partial(_ops, 5)
for _k in ("nine", "first", "last"):
    BUILDERS["shapes_" + _k] = functools.partial(_shapes, _k)
NAMES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    k = BUILDERS[name]()
    k.name = name
    k.m.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def expected(name, cap_lds=SH_PE_LDS):
    return restate(case(name), cap_lds)


_ORACLE = {}


def oracle_result(oracle_lib, name):
    """(flag, n_tracked) of the C oracle, computed once per case (float32 input: the fields are 0 / 1 in either type)"""
    if name not in _ORACLE:
        k = case(name)
        flag, n = oracle_lib.run_contrack(k.m.astype(np.float32), k.thr(), ">=", k.wrow(), k.overlap, k.pers, True)
        flag.setflags(write=False)
        _ORACLE[name] = (flag, int(n))
    return _ORACLE[name]
