"""Constructed slabs for the capacity, window and op-slot rules of the seam stage of the one-call pass (k_fz_mark / k_fz_rank_mark,
k_fz_groups and k_seam_driver in contrack_amd/csrc/ctk_seam_dev.hip, fz_slot / fz_box_merge in ctk_resolve_dev.hip), and a plain
numpy / scipy.ndimage restatement of what that stage should see and do: the bbox-confined relabelling of contrack.py:753-763.

The fields are exact rectangles and single pixels, static in time or isolated in time, so that their counts are designed: every
case carries the numbers it was built for (`design`), tests/test_seam_forms_host.py compares them with the restatement on the CPU,
and tests/test_gpu_seam_forms.py compares the restatement and the C oracle with what the library does and reports.
TEST INFRASTRUCTURE: nothing here is imported by contrack_amd/, and nothing here imports from it.

The rules restated (constants of ctk_seam_dev.hip / ctk_resolve_dev.hip / ctk_api.hip):
  records     seam rows (x = 0 and x = nx - 1 both kept foreground), run-length grouped by (t, consecutive y, label pair).  A row
              whose two ends carry the SAME 3-D label only counts when that label is marked: it meets another label on some row.
  clusters    labels united through rows with two different labels.  One wave drives one cluster.
  SD_LAB      64 labels of one cluster, 64 operations of one cluster (one per lane); more: CTK_POISON_CLUSTER, reason 512, and the
              grid stays on the synchronous path for this handle.
  SD_BATCH    512 records of one cluster in one window of 64 steps, the windows aligned to the cluster's first step; more: 512 too.
  SD_OPS_OWN  8 op slots belong to every label id below own_ids; a cluster with more operations, or whose root (its smallest
              label) is not below own_ids, takes a range of the shared tail.
  own_ids     min(max(ids guess, 8192), runs + 1); ids guess: runs / 32 on a fresh handle, else 1.25 x the ids of the last pass.
  tail        op_cap_hint slots, 4096 on a fresh handle (runs / 256 if that is more); a full tail: CTK_POISON_OPCAP, reason 256, the
              hint doubles and the next call fits.
  FZ_TW       k_fz_groups: 16 steps per workgroup, LDS hashes of 512 label boxes and 256 cluster ranges, 8 probes, then memory.
"""
import functools

import numpy as np
from scipy import ndimage

import shard_forms as sf
from shard_forms import filtered              # the overlap filter of contrack.py:706-742 (every case must pass it unchanged, but 'dropped')

SD_LAB = 64
SD_OPS = 64
SD_BATCH = 512
SD_WINDOW = 64
SD_OPS_OWN = 8
OWN_IDS_FLOOR = 8192
OP_CAP_HINT = 4096
FZ_TW, FZ_HS, FZ_CS, FZ_PROBES = 16, 512, 256, 8
REASON_OPCAP, REASON_CLUSTER = 256, 512

_TRACK = np.zeros((3, 3, 3), dtype=int)       # in-plane 3 x 3, centre pixel only in time (contrack.py:748-750)
_TRACK[1] = 1
_TRACK[0, 1, 1] = _TRACK[2, 1, 1] = 1


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def fresh_labels(mask):
    lab, _ = ndimage.label(mask, structure=_TRACK)
    return lab.astype(np.int32)


def _seam_rows(lab):
    a, b = lab[:, :, 0], lab[:, :, -1]
    tt, yy = np.nonzero((a > 0) & (b > 0))                      # (t, y) order
    return [(int(t), int(y)) for t, y in zip(tt, yy)]


def reference_merge(lab):
    """contrack.py:753-763 literally: find_objects ONCE, then for every (t, y) the two tests in their order, each on the flag as it
    is by then.  (Only rows with both seam pixels set can pass either test, and the set pixels never change: the loop visits
    exactly those rows, in (t, y) order.)"""
    flag = lab.copy()
    slices = ndimage.find_objects(flag)
    for tt, yy in _seam_rows(lab):
        if flag[tt, yy, 0] > 0 and flag[tt, yy, -1] > 0 and (flag[tt, yy, 0] > flag[tt, yy, -1]):
            slice_ = slices[flag[tt, yy, 0] - 1]
            flag[slice_][(flag[slice_] == flag[tt, yy, 0])] = flag[tt, yy, -1]
        if flag[tt, yy, 0] > 0 and flag[tt, yy, -1] > 0 and (flag[tt, yy, 0] < flag[tt, yy, -1]):
            slice_ = slices[flag[tt, yy, -1] - 1]
            flag[slice_][(flag[slice_] == flag[tt, yy, -1])] = flag[tt, yy, 0]
    return flag


class _Sets:
    def __init__(self):
        self.par = {}

    def find(self, i):
        par = self.par
        par.setdefault(i, i)
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i

    def unite(self, a, b):
        p, q = self.find(a), self.find(b)
        if p != q:
            self.par[max(p, q)] = min(p, q)


def clusters(lab):
    """-> (sets of labels united over rows with two different labels, label -> root = smallest label of its set)"""
    s = _Sets()
    for t, y in _seam_rows(lab):
        l, r = int(lab[t, y, 0]), int(lab[t, y, -1])
        if l != r:
            s.unite(l, r)
    root = {l: s.find(l) for l in list(s.par)}
    sets = {}
    for l, r in root.items():
        sets.setdefault(r, set()).add(l)
    return [frozenset(v) for _, v in sorted(sets.items())], root


def records(lab):
    """-> [(t, y0, y1, label at x = 0, label at x = nx - 1)] in (t, y) order: what k_fz_groups (and k_rs_cand_groups) write"""
    _, root = clusters(lab)
    out = []
    prev = None                                                   # (t, y, l, r) of the previous VALID seam row
    for t, y in _seam_rows(lab):
        l, r = int(lab[t, y, 0]), int(lab[t, y, -1])
        valid = l != r or l in root                               # marked: the label meets a different one on some row
        if not valid:
            prev = None
            continue
        if prev == (t, y - 1, l, r):
            out[-1] = out[-1][:2] + (y,) + out[-1][3:]
        else:
            out.append((t, y, y, l, r))
        prev = (t, y, l, r)
    return out


class Drive:
    """what SeamDriver::run (ctk_seam.h) records for the slab, and what each cluster asks of k_seam_driver"""

    def __init__(self, lab, inflow_rule=True, order="ty"):
        T, ny, nx = lab.shape
        boxes = ndimage.find_objects(lab)
        box = lambda l: tuple(v for s in boxes[l - 1] for v in (s.start, s.stop - 1))
        recs = records(lab)
        self.records = recs
        self.ops = []                                             # (hi, lo, (t0, t1, y0, y1, x0, x1)) in execution order
        chain, inflow = {}, {}                                    # hi -> its ops in order; lo -> last op that moved pixels into it
        self.fold_depth = 0
        ops = self.ops

        def fold(l, t, y, x):
            s = depth = 0
            moved = True
            while moved:
                moved = False
                for idx in chain.get(l, ()):
                    b = ops[idx][2]
                    if idx >= s and b[0] <= t <= b[1] and b[2] <= y <= b[3] and b[4] <= x <= b[5]:
                        l, s, depth, moved = ops[idx][1], idx + 1, depth + 1, True
                        break
            self.fold_depth = max(self.fold_depth, depth)
            return l
        rows = [(t, y, l, r) for t, y0, y1, l, r in recs for y in range(y0, y1 + 1)]
        if order == "label":                                      # (a mutation for test_seam_forms_host.py: NOT what the reference does)
            rows.sort(key=lambda q: (max(q[2], q[3]), q[0], q[1]))
        for t, y, l, r in rows:
            p0, p1 = fold(l, t, y, 0), fold(r, t, y, nx - 1)
            if p0 == p1:
                continue
            hi, lo = max(p0, p1), min(p0, p1)                     # the larger fresh label becomes the smaller (:759 / :763)
            if inflow_rule and hi in chain and inflow.get(hi, -1) < chain[hi][-1]:
                continue                                          # nothing flowed into hi since its last op: no pixel to move
            idx = len(ops)
            ops.append((hi, lo, box(hi)))
            chain.setdefault(hi, []).append(idx)
            inflow[lo] = idx
        # per cluster
        sets, root = clusters(lab)
        self.clusters = {}
        for s in sets:
            self.clusters[min(s)] = dict(labels=len(s), ops=0, records=0, t0=None, t1=None, win={})
        for t, _, _, l, _ in recs:
            c = self.clusters[root[l]]
            c["records"] += 1
            c["t0"] = t if c["t0"] is None else min(c["t0"], t)
            c["t1"] = t if c["t1"] is None else max(c["t1"], t)
        for t, _, _, l, _ in recs:
            c = self.clusters[root[l]]
            w = (t - c["t0"]) // SD_WINDOW                       # windows are aligned to the cluster's first step
            c["win"][w] = c["win"].get(w, 0) + 1
        for hi, _, _ in ops:
            self.clusters[root[hi]]["ops"] += 1
        for c in self.clusters.values():
            c["window"] = max(c["win"].values())

    def summary(self):
        cl = list(self.clusters.values())
        mx = lambda k: max([c[k] for c in cl] or [0])
        return dict(clusters=len(cl), labels=mx("labels"), ops=len(self.ops), max_ops=mx("ops"), records=len(self.records),
                    window=mx("window"), fold=self.fold_depth)


def drive(lab):
    return Drive(lab)


def apply(lab, ops):
    """the op list on the fresh labels, in order: every op moves the pixels labelled hi inside its box to lo"""
    flag = lab.copy()
    for hi, lo, (t0, t1, y0, y1, x0, x1) in ops:
        v = flag[t0:t1 + 1, y0:y1 + 1, x0:x1 + 1]
        v[v == hi] = lo
    return flag


def union_merge(lab):
    """a mutation for test_seam_forms_host.py: every cluster united into its smallest label -- what a plain union-find would give,
    NOT what the reference does (the boxes confine its relabels)"""
    _, root = clusters(lab)
    lut = np.arange(int(lab.max()) + 1, dtype=lab.dtype)
    for l, r in root.items():
        lut[l] = r
    return lut[lab]


def count_runs(m):
    """runs of set pixels along x: `runs` of the library's statistics, which size own_ids and the tail on a fresh handle"""
    return int(m[:, :, 0].sum() + (m[:, :, 1:] & ~m[:, :, :-1]).sum())


def first_call_slots(case):
    """-> (own_ids, tail slots) of the first fused pass of a fresh handle (resolve_async in ctk_api.hip)"""
    R = max(count_runs(case.m), 1)
    return min(max(R // 32, OWN_IDS_FLOOR), R + 1), max(OP_CAP_HINT, min(R // 256, 1 << 24))


def tail_ops(d, own_ids):
    """operations that go to the shared tail: those of clusters with more than SD_OPS_OWN of them or a root not below own_ids"""
    return sum(c["ops"] for root, c in d.clusters.items() if c["ops"] > SD_OPS_OWN or root >= own_ids)


def limits_broken(case, d):
    """which of the driver's per-cluster limits some cluster of the case exceeds, with the case's caps: a subset of
    {'labels', 'ops', 'window'}"""
    lab_cap, ops_cap = case.caps if case.caps else (SD_LAB, SD_OPS)
    out = set()
    for c in d.clusters.values():
        if c["labels"] > lab_cap:
            out.add("labels")
        if c["ops"] > ops_cap:
            out.add("ops")
        if c["window"] > SD_BATCH:
            out.add("window")
    return out


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
class Case(sf.Case):
    def __init__(self, name, T, ny, nx=64, pers=1):
        sf.Case.__init__(self, name, T, ny, nx, [0, T], pers)
        self.expect = 0               # off_fused_path_reason of the first call on a fresh handle: 0, 256 or 512
        self.caps = None              # (labels, ops) for debug_set_seam_caps
        self.dropped = 0              # pixels the overlap filter removes (case n only)
        self.design = dict(clusters=0, labels=0, ops=0, max_ops=0, records=0, window=0, ids=0)

    def count(self, labels, ops, records, window=None, clusters=1, ids=1):
        """one more cluster (or `clusters` alike) with these designed counts"""
        d = self.design
        d["clusters"] += clusters
        d["labels"] = max(d["labels"], labels)
        d["ops"] += ops * clusters
        d["max_ops"] = max(d["max_ops"], ops)
        d["records"] += records * clusters
        d["window"] = max(d["window"], records if window is None else window)
        d["ids"] += ids * clusters

    def comb(self, y0, teeth, bar, side="left", wide=1):
        """a bar in the seam column of `side` over the steps bar = (t0, t1) and the rows y0 .. y0 + 2 len(teeth) - 2, and on every
        other row a tooth of `wide` pixels in the opposite seam column over its own steps (t0, t1).  -> first free row"""
        n = len(teeth)
        nx = self.m.shape[2]
        b0, b1 = self.clip(*bar)
        self.m[b0:b1, y0:y0 + 2 * n - 1, 0 if side == "left" else nx - 1] = True
        for i, (t0, t1) in enumerate(teeth):
            (self.right if side == "left" else self.left)(y0 + 2 * i, wide, t0, t1)
        return y0 + 2 * n

    def rungs(self, n, y0, t0, t1):
        """TWO labels with n records per step: a bar at x = 0 and, at the right, one comb-shaped component that reaches x = nx - 1
        on every other row (the same pair on rows y and y + 2 is two records).  -> first free row"""
        nx = self.m.shape[2]
        self.block(y0, y0 + 2 * n - 1, 0, 1, t0, t1)
        self.block(y0, y0 + 2 * n - 1, nx - 3, nx - 2, t0, t1)
        for i in range(n):
            self.block(y0 + 2 * i, y0 + 2 * i + 1, nx - 2, nx, t0, t1)
        return y0 + 2 * n

    def mirror(self):
        self.m = np.ascontiguousarray(self.m[:, :, ::-1])
        return self


def _comb(k, steps, side="left", late=False, T=None, ny=None, caps=None):
    """ONE cluster of k + 1 labels, k operations and k records per step.  late: the teeth (4 pixels wide, so that they carry the
    overlap) are one step older than the bar, which then has the largest label and is `hi` first"""
    T = steps if T is None else T
    c = Case("comb", T, max(2 * k, 4) if ny is None else ny)
    c.comb(0, [(0, steps)] * k, (1 if late else 0, steps), side, 4 if late else 1)
    c.caps = caps
    rec = k * (steps - (1 if late else 0))
    win = k * min(SD_WINDOW, steps - (1 if late else 0))
    c.count(k + 1, k, rec, win)
    lab_cap, ops_cap = caps if caps else (SD_LAB, SD_OPS)
    if k + 1 > lab_cap or k > ops_cap or win > SD_BATCH:
        c.expect = REASON_CLUSTER
    return c


def _combs(ks, steps=3):
    """several combs below each other: the clusters with more than 8 operations take ranges of the shared tail in the order their
    waves arrive, the others their own slots"""
    c = Case("combs", steps, sum(2 * k for k in ks) + 2)
    y = 0
    for i, k in enumerate(ks):
        y = c.comb(y, [(0, steps)] * k, (0, steps), "left" if i % 3 else "right")
        c.count(k + 1, k, k * steps)
    return c


def _ladder(d, tall, mirror=False, tail=False):
    """components C_0 .. C_d with label(C_0) > ... > label(C_d) (a one-pixel stem in time each, born in the order d .. 0); row
    2 j + 2 pairs C_j (arm from x = 0 to column 2 + 2 j) with C_(j+1) (arm from column 4 + 2 j to x = nx - 1) on the last two steps, one
    arm-free step in between.  d operations C_j -> C_(j+1) in ONE cluster.  tall: every component also has a full-height line on
    its own first step, so every box holds every row: the second arm step folds C_0 through all d operations and one id is
    left.  Not tall: box(C_j) holds the rows 2 j .. 2 j + 2 only, a fold stops after two operations, and what C_(j-1) left
    outside box(C_j) keeps the label C_j: d ids are left, where a plain union would leave one.
    tail (tall only): one more seam row below, with a second arm of C_0 on the left and a component D born with the arms, the
    largest label, on the right.  The row ACTS, and only a fold of C_0 through all d operations finds that D becomes C_d.
    The arms' 2-D component overlaps the stems only: overlap is set to 1e-4 so that the filter keeps it."""
    T, ny, nx = d + 4, 2 * d + (4 if tail else 2), max(2 * d + 6, 64)
    c = Case("ladder", T, ny, nx)
    c.overlap = 1e-4
    for j in range(d + 1):
        c.m[d - j:, 2 * j + 1, 2 + 2 * j] = True                 # the stem (also what joins the two arms)
        if tall:
            c.m[d - j, :, 2 + 2 * j] = True
        if j < d:
            c.left(2 * j + 2, 3 + 2 * j, d + 2, T)
        if j > 0:
            c.right(2 * j, nx - (2 + 2 * j), d + 2, T)
    if tail:
        assert tall
        c.m[d:, 2 * d + 3, 2] = True                             # C_0's second stem, on its full-height line
        c.left(2 * d + 3, 4, d + 2, T)
        c.right(2 * d + 3, 4, d + 2, T)
        c.count(d + 2, d + 1, 2 * d + 2)
    else:
        c.count(d + 1, d, 2 * d, ids=1 if (tall or d == 1) else d)
    c.design["fold"] = d if tall else min(d, 2)
    return c.mirror() if mirror else c


def _stranded(mirror=False):
    """the short ladder of A = C_0, B = C_1, C = C_2 (A -> B on row 2, B -> C on row 4) and one more seam row, 8, with A on the left
    and C on the right: A and C each have a second stem there, joined to the first on the component's own first step.  Row 8
    lies outside box(B), so A's pixels there keep the label B, and the row asks for B -> C again -- on either arm step -- although
    nothing has flowed into B since B -> C: the reference finds no pixel to move and the driver records nothing"""
    d = 2
    c = _ladder(d, False)
    T, ny, nx = c.m.shape
    c.m = np.concatenate([c.m, np.zeros((T, 10 - ny, nx), dtype=bool)], axis=1)
    c.m[d, 1:9, 2] = True                                         # A's first step: down column 2 ...
    c.m[d, 8, 0:3] = True                                         # ... and along row 8
    c.m[d:, 8, 1] = True                                          # A's second stem
    c.m[0, 5:9, 6] = True                                         # the same for C, on step 0
    c.m[0, 8, 6:nx - 1] = True
    c.m[0:, 8, nx - 2] = True
    c.left(8, 3, d + 2, T)
    c.right(8, 3, d + 2, T)
    c.design.update(records=6, window=6, ids=2, fold=2)
    return c.mirror() if mirror else c


def _inflow(mirror=False):
    """a label that is `hi` of TWO operations: the only shape whose chain (op_next) is longer than one.  Four components, born in
    the order C, B, X, A (labels 1 .. 4, two steps apart), each a set of short arms on the last two steps; an arm holds a one-pixel stem in time,
    and on the component's first step its stems are joined down their own columns and along a row of its own (B's above
    everything, so that box(B) = rows 0 .. 6).
        row 2   X | B    X -> B
        row 4   A in the middle: inside box(B), on no seam
        row 6   B | C    B -> C; what X has on the rows 9 and 12 lies outside box(B) and keeps the label B
        row 9   A | X    A -> B: pixels flow into B again
        row 12  X | C    B -> C a second time, which moves A's middle piece; A's arm on row 9 keeps the label B
    On the second arm step row 12 asks once more, now with nothing flowed into B since: not recorded."""
    c = Case("inflow", 11, 20)
    arms = [("C", [("R", 6), ("R", 12)], 14), ("B", [("R", 2), ("L", 6)], 0), ("X", [("L", 2), ("R", 9), ("L", 12)], 16),
            ("A", [("L", 9), ("M", 4)], 18)]
    col0 = dict(L=(0, 10, 2), M=(26, 38, 28), R=(54, 64, 55))      # first column, end, stem column of component 0 (+ 2 per component)
    for i, (_, pieces, own_row) in enumerate(arms):
        cols = []
        for side, y in pieces:
            x0, x1, xs = col0[side]
            xs += 2 * i
            cols.append(xs)
            c.m[2 * i:, y, xs] = True                             # the stem
            c.m[2 * i, min(y, own_row):max(y, own_row) + 1, xs] = True
            c.block(y, y + 1, x0, x1, 9, 11)                      # the arm
        c.m[2 * i, own_row, min(cols):max(cols) + 1] = True
    c.overlap = 1e-4
    c.count(4, 4, 8, ids=2)
    c.design["fold"] = 2
    return c.mirror() if mirror else c


def _windows(L):
    """a comb of three teeth whose bar lives L steps, and four more teeth that live one step each: steps 0, 63, 64 and L - 1 (those
    inside the slab, once each).  They bring new labels and new operations in during later windows and later chunks"""
    once = sorted({s for s in (0, 63, 64, L - 1) if s < L})
    c = Case("windows", L, 2 * (3 + len(once)))
    c.comb(0, [(0, L)] * 3 + [(s, s + 1) for s in once], (0, L))
    per = lambda a, b: 3 * (min(b, L) - a) + sum(a <= s < b for s in once)
    c.count(4 + len(once), 3 + len(once), 3 * L + len(once), max(per(a, a + SD_WINDOW) for a in range(0, L, SD_WINDOW)))
    return c


def _batch(k, steps, extra):
    """comb(k) over `steps` steps and `extra` more teeth on the last step only: k steps + extra records"""
    c = Case("batch", steps, 2 * (k + extra))
    c.comb(0, [(0, steps)] * k + [(steps - 1, steps)] * extra, (0, steps))
    rec = k * steps + extra
    win = k * min(steps, SD_WINDOW) + (extra if steps <= SD_WINDOW else 0)
    if steps > SD_WINDOW:
        win = max(win, k * (steps - SD_WINDOW) + extra)
    c.count(k + extra + 1, k + extra, rec, win)
    if win > SD_BATCH:
        c.expect = REASON_CLUSTER
    return c


def _crowd(nbars, steps=8):
    """comb(5) and nbars small clusters (a left and a right piece on one row) beside it in the same steps: the windows of all
    clusters hold (5 + nbars) steps records, the comb's own 5 steps"""
    c = Case("crowd", steps, 10 + 2 * nbars + 2)
    y = c.comb(0, [(0, steps)] * 5, (0, steps))
    c.count(6, 5, 5 * steps)
    for i in range(nbars):
        c.bar(y + 2 * i, 2, 2, 0, steps)
    c.count(2, 1, steps, clusters=nbars)
    c.design["window_all"] = (5 + nbars) * steps
    return c


def _step(nrec, ncl):
    """nrec records in EVERY step, of ncl clusters that all start in step 0: ncl - 1 single rows and rungs for the rest"""
    c = Case("step", 2, 264)
    y, rest = 0, nrec
    if ncl == 2:                                                  # two clusters of rungs
        y = c.rungs(nrec // 2, 0, 0, 2)
        c.count(2, 1, 2 * (nrec // 2))
        rest = nrec - nrec // 2
    elif ncl > 2:
        for i in range(ncl - 1):
            c.bar(y, 2, 2, 0, 2)
            y += 2
        c.count(2, 1, 2, clusters=ncl - 1)
        rest = nrec - (ncl - 1)
    c.rungs(rest, y, 0, 2)
    c.count(2, 1, 2 * rest)
    c.design["step_records"] = nrec
    return c


def _stripes(ny, segs):
    """a bar at x = 0 over all rows and bars at x = nx - 1 over the row ranges segs (one gap row in between): one group per range.
    The lanes of k_fz_groups hold seam ROWS in order, so a gap row does not take one"""
    c = Case("stripes", 2, ny)
    c.block(0, ny, 0, 1, 0, 2)
    for a, b in segs:
        c.block(a, b + 1, 63, 64, 0, 2)
    c.count(1 + len(segs), len(segs), 2 * len(segs))
    # seam-row indices (lanes, modulo 64) at which the groups end
    ends, i = [], 0
    for a, b in segs:
        i += b - a + 1
        ends.append(i - 1)
    c.design["group_ends"] = ends
    return c


def _groups_mixed():
    """ny = 129.  Rows 0 .. 78: rungs, 40 records of one pair on rows y, y + 2, ...  Row 80: a full row of its own -- one label on
    both ends, unmarked: dropped.  Rows 82 .. 84: C = a full row and a piece down the left edge, D = one pixel at the right of row
    84: row 82 carries (C, C) with C marked -- a record -- and row 84 (C, D).  Rows 86 .. 128: a left and a right bar, one group
    whose seam rows 43 .. 85 cross the lane boundary"""
    c = Case("groups", 2, 129)
    c.rungs(40, 0, 0, 2)
    c.count(2, 1, 80)
    c.block(80, 81, 0, 64, 0, 2)
    c.design["ids"] += 1
    c.block(82, 83, 0, 64, 0, 2)
    c.block(83, 85, 0, 1, 0, 2)
    c.block(84, 85, 63, 64, 0, 2)
    c.count(2, 1, 4)
    c.block(86, 129, 0, 1, 0, 2)
    c.block(86, 129, 63, 64, 0, 2)
    c.count(2, 1, 2)
    c.design["dropped_rows"] = 2
    return c


def _hash(per_step, T):
    """per_step pairs of a left and a right pixel on every step, each alive one step only (even rows on even steps, odd rows on odd
    ones: nothing connects in time): per_step clusters and 2 per_step marked labels per step, 16 steps to a workgroup of k_fz_groups"""
    c = Case("hash", T, 66)
    for t in range(T):
        for i in range(per_step):
            c.m[t, (t & 1) + 2 * i, [0, 63]] = True
    c.count(2, 1, 1, clusters=per_step * T)
    c.design["labels_per_workgroup"] = 2 * per_step * min(T, FZ_TW)
    c.design["clusters_per_workgroup"] = per_step * min(T, FZ_TW)
    return c


def _tail(n9, n10):
    """n9 combs of 9 teeth and n10 of 10, one step each with an empty step in between, the tens spread among the nines: every
    cluster has more than 8 operations, so all 9 n9 + 10 n10 of them go to the shared tail"""
    n = n9 + n10
    c = Case("tail", 2 * n, 20, 64)
    every = n // n10
    tens = 0
    for i in range(n):
        k = 10 if (i % every == every // 2 and tens < n10) else 9
        tens += k == 10
        c.comb(0, [(2 * i, 2 * i + 1)] * k, (2 * i, 2 * i + 1))
        c.count(k + 1, k, k)
    assert tens == n10
    c.design["tail_ops"] = 9 * n9 + 10 * n10
    if c.design["tail_ops"] > OP_CAP_HINT:
        c.expect = REASON_OPCAP
    return c


def _high_root(npix=8200):
    """npix isolated pixels on step 0 take the first npix labels; comb(4) and comb(9) on the steps 2 and 3 have roots beyond the
    8192 ids that own slots on a fresh handle: the 4 operations of comb(4) go to the shared tail too"""
    c = Case("high_root", 4, 132, 256)
    c.pixels(npix, 0, 1, 0, x0=2)
    c.design.update(ids=npix)
    y = c.comb(0, [(2, 4)] * 4, (2, 4))
    c.count(5, 4, 8)
    c.comb(y, [(2, 4)] * 9, (2, 4))
    c.count(10, 9, 18)
    c.design["min_root"] = npix + 1
    c.design["tail_ops"] = 13
    return c


def _filtered_away():
    """comb(3) over five steps.  Above it, on step 2 only, a left and a right arm of 8 pixels on row 0; one pixel of the left arm
    is also set on the steps 0, 1, 3 and 4.  The two arms are one seam-merged 2-D component with 1 / 16 of its area in common with
    step 1: the filter removes it, and its seam row must bring no label, no record and no operation"""
    c = Case("filtered_away", 5, 8, 64)
    c.bar(0, 8, 8, 2, 3)
    c.block(0, 1, 7, 8, 0, 5)
    c.comb(2, [(0, 5)] * 3, (0, 5))
    c.count(4, 3, 15)
    c.design["ids"] += 2                                          # the lone pixel before and after the removed step
    c.dropped = 16
    return c


BUILDERS = {}
# (a) SD_OPS_OWN = 8: own slots or shared tail
for _k in (8, 9):
    BUILDERS["a_comb_%d" % _k] = functools.partial(_comb, _k, 3)
    BUILDERS["a_comb_%d_right" % _k] = functools.partial(_comb, _k, 3, "right")
    BUILDERS["a_comb_%d_late" % _k] = functools.partial(_comb, _k, 4, "left", True)
BUILDERS["a_combs_mixed"] = functools.partial(_combs, (8, 9, 9, 8, 8, 9, 3, 10))
# (b) SD_LAB = 64 labels
BUILDERS["b_comb_63"] = functools.partial(_comb, 63, 2, ny=128)
BUILDERS["b_comb_64"] = functools.partial(_comb, 64, 2, ny=128)
BUILDERS["b_comb_63_late"] = functools.partial(_comb, 63, 3, "right", True, ny=128)
# (c) the hook's caps: labels <= lab_cap and ops <= ops_cap stay on the device
for _caps in ((64, 12), (64, 11), (13, 64), (12, 64)):
    BUILDERS["c_comb_12_caps_%d_%d" % _caps] = functools.partial(_comb, 12, 2, caps=_caps)
# (d) fold chains
for _d in (1, 2, 3, 63):
    BUILDERS["d_ladder_tall_%d" % _d] = functools.partial(_ladder, _d, True)
for _d in (3, 20):
    BUILDERS["d_ladder_short_%d" % _d] = functools.partial(_ladder, _d, False)
BUILDERS["d_ladder_tall_3_mirror"] = functools.partial(_ladder, 3, True, True)
BUILDERS["d_ladder_tall_63_mirror"] = functools.partial(_ladder, 63, True, True)
BUILDERS["d_ladder_short_20_mirror"] = functools.partial(_ladder, 20, False, True)
BUILDERS["d_ladder_tail_3"] = functools.partial(_ladder, 3, True, False, True)
BUILDERS["d_ladder_tail_62"] = functools.partial(_ladder, 62, True, False, True)
BUILDERS["d_ladder_tail_62_mirror"] = functools.partial(_ladder, 62, True, True, True)
BUILDERS["d_inflow"] = _inflow
BUILDERS["d_inflow_mirror"] = functools.partial(_inflow, True)
BUILDERS["d_stranded"] = _stranded
BUILDERS["d_stranded_mirror"] = functools.partial(_stranded, True)
# (e) 64-step gather windows
for _L in (64, 65, 128, 129):
    BUILDERS["e_windows_%d" % _L] = functools.partial(_windows, _L)
# (f) SD_BATCH = 512 records of a cluster in a window
BUILDERS["f_batch_512"] = functools.partial(_batch, 8, 64, 0)
BUILDERS["f_batch_513"] = functools.partial(_batch, 8, 64, 1)
BUILDERS["f_batch_512_plus_8"] = functools.partial(_batch, 8, 65, 0)
# (g) 64-record chunks
BUILDERS["g_chunk_64"] = functools.partial(_batch, 8, 8, 0)
BUILDERS["g_chunk_65"] = functools.partial(_batch, 8, 8, 1)
BUILDERS["g_chunk_130"] = functools.partial(_batch, 8, 16, 2)
# (h) a window of more than 64 records over all clusters
BUILDERS["h_crowd_30"] = functools.partial(_crowd, 30)
BUILDERS["h_crowd_7"] = functools.partial(_crowd, 7)               # (5 + 7) x 8 = 96: the second trip of the gather is partial
# (i) records of one step: shuffle de-duplication up to 64, claim words beyond
for _n, _c in ((64, 1), (64, 40), (65, 1), (65, 2), (65, 40), (130, 1), (130, 2), (130, 40)):
    BUILDERS["i_step_%d_clusters_%d" % (_n, _c)] = functools.partial(_step, _n, _c)
# (j) run-length grouping
BUILDERS["j_stripes_63"] = functools.partial(_stripes, 63, [(0, 62)])
BUILDERS["j_stripes_64"] = functools.partial(_stripes, 64, [(0, 63)])
BUILDERS["j_stripes_65_cross"] = functools.partial(_stripes, 65, [(0, 64)])
BUILDERS["j_stripes_65_end63"] = functools.partial(_stripes, 65, [(0, 61), (63, 64)])
BUILDERS["j_stripes_129_end63"] = functools.partial(_stripes, 129, [(0, 63), (65, 128)])
BUILDERS["j_stripes_129_cross"] = functools.partial(_stripes, 129, [(0, 99), (101, 128)])
BUILDERS["j_stripes_129_full"] = functools.partial(_stripes, 129, [(0, 128)])
BUILDERS["j_groups_mixed"] = _groups_mixed
# (k) the LDS hashes of k_fz_groups
BUILDERS["k_hash_33_T16"] = functools.partial(_hash, 33, 16)
BUILDERS["k_hash_33_T17"] = functools.partial(_hash, 33, 17)
BUILDERS["k_hash_33_T33"] = functools.partial(_hash, 33, 33)
BUILDERS["k_hash_16_T16"] = functools.partial(_hash, 16, 16)
BUILDERS["k_hash_15_T16"] = functools.partial(_hash, 15, 16)
# (l) the shared tail, full
BUILDERS["l_tail_4096"] = functools.partial(_tail, 444, 10)
BUILDERS["l_tail_4097"] = functools.partial(_tail, 443, 11)
# (m) cluster roots beyond own_ids
BUILDERS["m_high_root"] = _high_root
# (n) seam rows of a filtered component
BUILDERS["n_filtered_away"] = _filtered_away
# (o) T = 1 .. 5
for _T in (1, 2, 3, 4, 5):
    BUILDERS["o_comb_3_T%d" % _T] = functools.partial(_comb, 3, _T)
NAMES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    k = BUILDERS[name]()
    k.name = name
    k.m.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def kept(name):
    """the mask behind the overlap filter"""
    k = case(name)
    m = filtered(k.m, k.wrow(), k.overlap)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def labels(name):
    lab = fresh_labels(kept(name))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def driven(name):
    return drive(labels(name))


def design(name):
    return dict(case(name).design, expect=case(name).expect, caps=case(name).caps)


_ORACLE = {}


def oracle_result(oracle_lib, name):
    """(flag, n_tracked) of the C oracle, computed once per case"""
    if name not in _ORACLE:
        k = case(name)
        flag, n = oracle_lib.run_contrack(k.m.astype(np.float32), k.thr(), ">=", k.wrow(), k.overlap, k.pers, True)
        flag.setflags(write=False)
        _ORACLE[name] = (flag, int(n))
    return _ORACLE[name]
