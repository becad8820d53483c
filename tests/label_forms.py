"""Which row-count, 2-D labelling and overlap kernel forms a call launches: a restatement of the rules in
contrack_amd/csrc/ctk_forms.h (ctk_rowcount_threads, ctk_rowcount_groups, ctk_label_shape for v0b / v0_ok / v0_runs, ctk_label_speculative, ctk_label_plan
for the launch after the run scan and the next call's speculative set, ctk_label_form_bits, ctk_overlap_form), of the protocol around
them in contrack_amd/csrc/ctk_api.hip (label2d_speculate, label2d_regrow's capacity check, label2d_finish_labels, launch_label2d) and
of the instances' own guards in contrack_amd/csrc/ctk_kernels.hip (k_label2d_lds: the planes it takes by RUNS / RUNS_BELOW / NYCAP, its
staged mask; k_label2d_glb; label2d_body's component tables in LDS).
Host-only.  Kept in step with the C++ by tests/test_label_forms.py which compares it with the library itself (ctk_debug_forms), and, on
the GPU, by the statistics CTK_S_LABEL_FORMS,
CTK_S_OVERLAP_FORM, CTK_S_ROWCOUNT_THREADS and CTK_S_ROWCOUNT_GROUPS that tests/test_gpu_label_forms.py asserts.

It also builds the planes that reach the forms: 0/1 planes with a prescribed number of runs, 2-D components (no wrap), seam rows
and, for the pair edges, distinct overlapping (c, d) pairs with the next plane."""
import numpy as np

CTK_LDS_RUNS = 4096              # ctk_device.h: runs an LDS variant can carry at most; beyond: k_label2d_glb
CTK_LDS_NY = 1024                # ... rows; beyond: k_label2d_glb
RC_ROWS = 2048                   # k_rowcount's first form: row totals in LDS
CTK_PSLOT = 128                  # ctk_api.hip: pair-record slots per timestep of the fused path
CTK_HASH_SLOTS = 512             # k_overlap's LDS hash of (c, d) pairs

# k_label2d_lds<RUNS, COMPS, RUNS_BELOW, THREADS, NYCAP> instances, in the order of their CTK_S_LABEL_FORMS bits
INSTANCES = {
    "one": (4096, 512, -1, 1024, CTK_LDS_NY),       # every timestep in one launch (T <= 512 with a plane above 1024 runs)
    "v1_768": (768, 272, -1, 256, 256),             # v1 of planes of 961 .. 1088 words (v0b)
    "v1_832": (832, 240, -1, 256, 256),             # v1 of planes of at most 960 words in shards of more than 65536 steps (v0_ok)
    "v1": (1024, 288, -1, 256, CTK_LDS_NY),
    "v1hi_768": (1024, 288, 768, 256, CTK_LDS_NY),  # 769 .. 1024 runs behind v1_768
    "v1hi_832": (1024, 288, 832, 256, CTK_LDS_NY),  # 833 .. 1024 runs behind v1_832
    "v2": (2048, 512, 1024, 512, CTK_LDS_NY),
    "v3": (4096, 512, 2048, 1024, CTK_LDS_NY),
}
LABEL = tuple(INSTANCES) + ("glb",)
LABEL_BIT = {name: 1 << i for i, name in enumerate(LABEL)}
DISCARDED_BIT = 1 << 9           # a speculative launch ran on too small run buffers
OVERLAP = ((4, 128, 5), (4, 512, 1), (4, 256, 1), (5, 256, 1), (6, 256, 1), (8, 256, 1))
ROWCOUNT = (512, 256, 128)


def nwords(ny, nx):
    return ny * ((nx + 63) // 64)


def rowcount_threads(T, ny, W):
    """ctk_rowcount_threads (ctk_forms.h)"""
    if W <= 64 and ny <= RC_ROWS and ny > 256 and T <= 2048:
        return 512
    return 128 if (T > 65536 and ny * W <= 2048) else 256


def rowcount_groups(threads, ny, W):
    """ctk_rowcount_groups (ctk_forms.h): the RCU of k_rowcount<RCU>, the row groups its first form keeps in flight -- as many as the
    plane needs in one step of its waves, of 4 / 6 / 8; a wave takes 64 // W whole rows of a group"""
    if W > 64:
        return 8
    per_group = (threads // 64) * (64 // W)
    need = (ny + per_group - 1) // per_group
    return 4 if need <= 4 else 6 if need <= 6 else 8


def rowcount_groups_stat(T, ny, W):
    """CTK_S_ROWCOUNT_GROUPS: the RCU of the instance launched; 0 where the plane takes one of the kernel's other two forms (or
    nothing is launched)"""
    if T == 0 or W > 64 or ny > RC_ROWS:
        return 0
    return rowcount_groups(rowcount_threads(T, ny, W), ny, W)


def rowcount_name(T, ny, W):
    return "rowcount<%d,%d>" % (rowcount_threads(T, ny, W), rowcount_groups_stat(T, ny, W))


def _v0(T, ny, W):
    """(v0b, v0_ok, v0_runs): ctk_label_shape (ctk_forms.h)"""
    v0b = ny <= 256 and 960 < ny * W <= 1088
    v0_ok = (T > 65536 and ny <= 256 and ny * W <= 960) or v0b
    return v0b, v0_ok, 768 if v0b else 832


def _v1_name(T, ny, W):
    v0b, v0_ok, _ = _v0(T, ny, W)
    return "v1_768" if v0b else ("v1_832" if v0_ok else "v1")


def _v1hi_name(T, ny, W):
    return "v1hi_768" if _v0(T, ny, W)[0] else "v1hi_832"


def label_variant(T, ny, nx, nruns, prefer_one):
    """the instance that labels a plane of nruns runs.  prefer_one: the call runs the one-launch form (T <= 512 and some plane above
    1024 runs, ctk_label_plan's prefer_one).  Each instance returns from planes outside its range (k_label2d_lds, k_label2d_glb), so
    the set launched decides nothing about a plane beyond which of these ranges exist; the ranges below are disjoint and cover all."""
    W = (nx + 63) // 64
    if nruns > CTK_LDS_RUNS or ny > CTK_LDS_NY:
        return "glb"
    if prefer_one:
        return "one"
    if nruns > 2048:
        return "v3"
    if nruns > 1024:
        return "v2"
    _, v0_ok, v0_runs = _v0(T, ny, W)
    if v0_ok and nruns > v0_runs:
        return _v1hi_name(T, ny, W)
    return _v1_name(T, ny, W)                 # (nruns == 0 included: RUNS_BELOW = -1)


def staged(variant, ny, W):
    """the instance stages the plane's mask words in LDS (k_label2d_lds).  For the two small-plane instances the staging edge
    is the selection edge: v1_768 takes only planes of at most 1088 words = its COMPS * 4, v1_832 only planes of at most 960 = its
    COMPS * 4, and v1hi_768 / v1hi_832 serve the same planes; so these always stage and have no unstaged side."""
    if variant == "glb":
        return False
    _, comps, _, threads, _ = INSTANCES[variant]
    nw = (comps * 4 + threads - 1) // threads
    return threads < 1024 and ny * W <= comps * 4 and nw <= 8


def tables_in_lds(variant, ncomp):
    """label2d_body's component tables live in LDS (ctk_kernels.hip); k_label2d_glb passes no LDS table"""
    return variant != "glb" and ncomp <= INSTANCES[variant][1]


def overlap_form(T, ny, W, seg):
    """CTK_S_OVERLAP_FORM of launch_overlap: ctk_overlap_form (ctk_forms.h)"""
    nw = ny * W
    per = (nw + 255) // 256
    if T > 65536 and nw <= 2048:
        f = (4, 128, 5)
    elif T <= 1024 and nw >= 8192:
        f = (4, 512, 1)
    elif per <= 4 or per > 8:
        f = (4, 256, 1)
    elif per == 5:
        f = (5, 256, 1)
    elif per == 6:
        f = (6, 256, 1)
    else:
        f = (8, 256, 1)
    return (1000000 if seg else 0) + f[0] * 10000 + f[1] * 10 + f[2]


def overlap_name(code):
    seg, c = divmod(code, 1000000)
    return "overlap<%d,%d,%d%s>" % (c // 10000, c // 10 % 1000, c % 10, ",SEG" if seg else "")


class Handle:
    """the speculation state of one ctk_handle (runs_cap, spec_set, spec_ny / spec_nx / spec_T) and the CTK_S_LABEL_FORMS bits of
    every call that labels (label2d_speculate .. label2d_finish_labels in ctk_api.hip, with the rules of ctk_forms.h)"""

    def __init__(self):
        self.runs_cap = 0
        self.spec = dict(v1=False, v2=False, v3=False, glb=False, one=False, v1hi=False)
        self.spec_shape = None
        self.spec_T = -1
        self.last_prefer_one = False

    def _bits(self, vs, T, ny, W):
        b = 0
        if vs["one"]:
            b |= LABEL_BIT["one"]
        if vs["v1"]:
            b |= LABEL_BIT[_v1_name(T, ny, W)]
        if vs["v1hi"]:
            b |= LABEL_BIT[_v1hi_name(T, ny, W)]
        for k in ("v2", "v3", "glb"):
            if vs[k]:
                b |= LABEL_BIT[k]
        return b

    def label2d(self, T, ny, nx, runs):
        """runs: the run count of every plane.  Returns the CTK_S_LABEL_FORMS value of the call."""
        runs = np.asarray(runs, dtype=np.int64)
        if T == 0:
            return 0
        W = (nx + 63) // 64
        _, v0_ok, v0_runs = _v0(T, ny, W)
        spec = self.runs_cap > 0 and self.spec_shape == (ny, nx) and (not self.spec["glb"] or self.spec_T >= T)
        bits = 0
        launched = dict(v1=False, v2=False, v3=False, glb=False, one=False, v1hi=False)
        if spec:
            launched = dict(self.spec)
            launched["v1hi"] = self.spec["v1hi"] and v0_ok
            bits |= self._bits(launched, T, ny, W)
        R, mx = int(runs.sum()), int(runs.max())
        need_glb = mx > CTK_LDS_RUNS or ny > CTK_LDS_NY
        if not (spec and R <= self.runs_cap):
            self.runs_cap = min(R + R // 8 + 1024, 0xffffffff)
            launched = dict(v1=False, v2=False, v3=False, glb=False, one=False, v1hi=False)
            if spec:
                bits |= DISCARDED_BIT
        prefer_one = T <= 512 and mx > 1024
        none_lds = not (launched["v1"] or launched["v2"] or launched["v3"] or launched["one"])
        need = dict(v1=True, v2=mx > 1024, v3=mx > 2048, glb=need_glb, one=False, v1hi=v0_ok and mx > v0_runs)
        if (prefer_one and (none_lds or launched["one"])) or launched["one"]:
            need = dict(v1=False, v2=False, v3=False, glb=need_glb, one=True, v1hi=False)
        missing = {k: need[k] and not launched[k] for k in need}
        bits |= self._bits(missing, T, ny, W)
        ran_one = launched["one"] or missing["one"]
        self.last_prefer_one = ran_one
        if prefer_one:
            self.spec.update(v1=False, v2=False, v3=False, one=True)
        else:
            self.spec.update(v1=True, v2=mx > 1024, v3=mx > 2048, one=False)
        self.spec.update(v1hi=need["v1hi"], glb=need["glb"])
        self.spec_shape, self.spec_T = (ny, nx), T
        return bits


def forms_reached(T, ny, nx, runs, comps, seg=(False,)):
    """the forms a call on a FRESH handle reaches with planes of these run and component counts"""
    W = (nx + 63) // 64
    runs = np.asarray(runs)
    prefer_one = T <= 512 and int(runs.max()) > 1024
    out = {"rowcount<%d>" % rowcount_threads(T, ny, W), rowcount_name(T, ny, W)}
    out |= {overlap_name(overlap_form(T, ny, W, s)) for s in seg}
    for r, c in set(zip(runs.tolist(), np.asarray(comps).tolist())):
        v = label_variant(T, ny, nx, r, prefer_one)
        out.add(v)
        if v != "glb" and r > 0:
            out.add(v + (":staged" if staged(v, ny, W) else ":global_mask"))
            out.add(v + (":tables_lds" if tables_in_lds(v, c) else ":tables_global"))
    return out


def _all_forms():
    f = set(LABEL)
    for v in INSTANCES:
        f.add(v + ":tables_lds")
        f.add(v + ":tables_global")
    f |= {v + ":staged" for v in ("v1_768", "v1_832", "v1", "v1hi_768", "v1hi_832", "v2")}
    f |= {v + ":global_mask" for v in ("v1", "v2", "v3", "one")}
    f |= {overlap_name(s * 1000000 + a * 10000 + b * 10 + c) for a, b, c in OVERLAP for s in (0, 1)}
    f |= {"rowcount<%d>" % n for n in ROWCOUNT}
    # <threads,RCU> of the first form; RCU 0: the other two forms.  (128 threads with RCU 6 or 8 need a shard of more than 65536
    # planes of at least 257 x 128: eight times the long shard below; no case reaches them)
    f |= {"rowcount<%d,%d>" % (n, u) for n in (512, 256) for u in (4, 6, 8)} | {"rowcount<128,4>", "rowcount<256,0>"}
    return frozenset(f)


FORMS = _all_forms()


# ---------------------------------------------------------------------------------------------------------------------------
# planes with prescribed counts
# ---------------------------------------------------------------------------------------------------------------------------
def _bands(nx, lo, hi):
    """column bands [x0, x1] inside [lo, hi], at least one blank column between neighbours.  First an anchor at every mask-word
    boundary b = 64 k, its run ending at bit 62, 63, 0 or 1 (k % 4; the last two cross the boundary: the word to the right
    takes a carry-in), then one-column bands in what is left."""
    anchors = []
    for k in range(1, (nx + 63) // 64):
        b = 64 * k
        x0, x1 = ((b - 2, b - 2), (b - 3, b - 1), (b - 1, b), (b - 2, b + 1))[k % 4]
        if x0 >= lo and x1 <= hi:
            anchors.append((x0, x1))
    blocked = np.zeros(nx + 2, dtype=bool)
    for x0, x1 in anchors:
        blocked[max(x0 - 1, 0):x1 + 2] = True
    rest, x = [], lo
    while x <= hi:
        if blocked[x]:
            x += 1
        else:
            rest.append((x, x))
            x += 2
    return anchors + rest


def stack_plane(ny, nx, runs, comps, seams=0, phase=0):
    """0/1 plane (uint8) with exactly `runs` runs and `comps` 8-connected components (no wrap), `seams` of its rows with pixels at
    both x = 0 and x = nx - 1 (seam rows: a stack at each edge over the same rows, two components).  Every component is a stack of
    one run per row in consecutive rows of one column band; the stacks go round the bands, those of a band one blank row apart
    from row `phase` on
    (row 0 and, when the band fills, row ny - 1 are the pole rows: their weights are ~2^-20 of the others)."""
    if comps > runs or (runs > 0 and comps == 0) or (seams and comps < 2):
        raise ValueError("inconsistent counts")
    m = np.zeros((ny, nx), dtype=np.uint8)
    if seams:
        if phase + seams > ny:
            raise ValueError("too many seam rows")
        m[phase:phase + seams, 0] = 1
        m[phase:phase + seams, nx - 1] = 1
        runs -= 2 * seams
        comps -= 2
        if comps == 0 and runs:
            raise ValueError("runs left without components")
    if comps == 0:
        return m
    heights = [runs // comps + (1 if i < runs % comps else 0) for i in range(comps)]
    bands = _bands(nx, 2, nx - 3)
    nb = min(len(bands), len(heights))          # stacks go round the bands (the anchors first), so that every anchor is used
    ycur = [phase] * len(bands)
    for i, h in enumerate(heights):
        if h > ny - phase:
            raise ValueError("stack taller than the plane")
        for j in range(len(bands)):
            b = (i + j) % nb if j < nb else j
            if ycur[b] + h <= ny:
                break
        else:
            raise ValueError("plane too small for %d runs in %d components" % (sum(heights), len(heights)))
        x0, x1 = bands[b]
        m[ycur[b]:ycur[b] + h, x0:x1 + 1] = 1
        ycur[b] += h + 1
    return m


def bars_of(plane):
    """every row of `plane` with pixels filled from its first to its last pixel: a stack_plane of one-row stacks (`dots`) and its
    bars overlap in exactly one (c, d) pair per dot, in both orders"""
    out = np.zeros_like(plane)
    for y in np.nonzero(plane.any(axis=1))[0]:
        xs = np.nonzero(plane[y])[0]
        out[y, xs[0]:xs[-1] + 1] = 1
    return out


def count_runs(mask):
    """runs per plane of a (T, ny, nx) 0/1 mask (no wrap: a row's runs end at x = nx - 1)"""
    m = np.asarray(mask, dtype=bool)
    starts = m & ~np.concatenate([np.zeros(m.shape[:2] + (1,), dtype=bool), m[:, :, :-1]], axis=2)
    return starts.sum(axis=(1, 2)).astype(np.int64)


def lattice(ny, nx):
    """a pixel at every second row and column: one run and one component per pixel (721 x 1440: 259 920)"""
    m = np.zeros((ny, nx), dtype=np.uint8)
    m[::2, ::2] = 1
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# cases: (name, T, ny, nx, planes, schedule, reach).  planes: {key: spec}; spec = ("stack", runs, comps, seams, phase) |
# ("bars", key of a stack plane) | ("lattice",); schedule(T) -> the key of every timestep; reach: the forms the case is meant to
# reach (tests/test_label_forms.py checks them against what its counts select).
# ---------------------------------------------------------------------------------------------------------------------------
def _cycle(keys):
    return lambda T: [keys[t % len(keys)] for t in range(T)]


def _quiet_then(keys, T0):
    """T0 quiet timesteps (zero runs every second one, a three-run stack the other), then `keys` in turn"""
    return lambda T: [("q0" if t % 2 else "q3") if t < T0 else keys[(t - T0) % len(keys)] for t in range(T)]


QUIET = {"q0": ("stack", 0, 0, 0, 0), "q3": ("stack", 3, 1, 0, 0)}


def _edges(pairs, comps, seams=2):
    """stack planes at the given run counts, each in two phases: pairs of consecutive planes overlap partially"""
    out = {}
    for r in pairs:
        c = 0 if r == 0 else min(comps, r)
        s = seams if c > 2 and r - 2 * seams >= c - 2 else 0
        out["r%d" % r] = ("stack", r, c, s, 0)
        out["r%d_" % r] = ("stack", r, c, s, 1)
    return out


def _keys(pl):
    return sorted(pl)


CASES = []


def _case(name, T, ny, nx, planes, schedule, reach, seg=True, slow=False):
    CASES.append(dict(name=name, T=T, ny=ny, nx=nx, planes=planes, schedule=schedule, reach=frozenset(reach), seg=seg, slow=slow))


# ---- run edges ----------------------------------------------------------------------------------------------------------
for _ny, _nx in ((181, 360), (256, 256)):                       # v0b: 1086 and 1024 words
    _pl = _edges((0, 768, 769, 1024), 60)
    _case("runs_v0b_%dx%d" % (_ny, _nx), 8, _ny, _nx, _pl, _cycle(_keys(_pl)), {"v1_768", "v1hi_768", "v1_768:staged", "v1hi_768:staged"})
    _pl = dict(QUIET, **_edges((1024, 1025, 769, 768), 60))      # T > 512: the 1025-run plane goes to v2, not to the one-launch form
    _case("runs_v0b_1025_%dx%d" % (_ny, _nx), 516, _ny, _nx, _pl, _quiet_then(_keys(_edges((1024, 1025, 769, 768), 60)), 508),
          {"v1hi_768", "v2", "v2:staged"})
_pl = dict(QUIET, **_edges((0, 1024, 1025, 2048, 2049, 4096, 4097), 100))
_case("runs_192x288", 520, 192, 288, _pl, _quiet_then(_keys(_edges((0, 1024, 1025, 2048, 2049, 4096, 4097), 100)), 506),
      {"v1", "v2", "v3", "glb", "v1:staged", "v2:staged", "v3:global_mask", "rowcount<256>", "overlap<4,256,1>"})
_pl = _edges((0, 1, 700, 1024), 80)
_case("runs_721x1440", 4, 721, 1440, _pl, _cycle(["r0", "r1", "r700_", "r1024"]), {"v1", "v1:global_mask", "rowcount<512>", "overlap<4,512,1>"})
_pl = _edges((1025, 2048, 4096, 4097), 120)
_case("one_721x1440", 4, 721, 1440, _pl, _cycle(["r1025", "r4096_", "r4097", "r2048_"]), {"one", "glb", "one:global_mask"})
_pl = dict(QUIET, **_edges((1025, 2048), 100))                 # v2 beyond its staging area: 2079 words
_case("runs_v2_33x4000", 513, 33, 4000, _pl, _quiet_then(["r1025", "r2048_"], 509), {"v2", "v2:global_mask", "overlap<4,256,1>"})

# ---- component edges (fixed run count inside each variant) --------------------------------------------------------------
_case("comps_v1_768", 4, 181, 360, {"a": ("stack", 700, 272, 2, 0), "b": ("stack", 700, 273, 2, 1)}, _cycle(["a", "b"]),
      {"v1_768:tables_lds", "v1_768:tables_global"})
_case("comps_v1hi_768", 4, 181, 360, {"a": ("stack", 900, 288, 2, 0), "b": ("stack", 900, 289, 2, 1)}, _cycle(["a", "b"]),
      {"v1hi_768:tables_lds", "v1hi_768:tables_global"})
_case("comps_v1", 4, 192, 288, {"a": ("stack", 1000, 288, 2, 0), "b": ("stack", 1000, 289, 2, 1)}, _cycle(["a", "b"]),
      {"v1:tables_lds", "v1:tables_global"})
_pl = dict(QUIET, a=("stack", 1500, 512, 2, 0), b=("stack", 1500, 513, 2, 1), c=("stack", 3000, 512, 2, 0), d=("stack", 3000, 513, 2, 1))
_case("comps_v2_v3", 516, 192, 288, _pl, _quiet_then(["a", "b", "c", "d"], 508),
      {"v2:tables_lds", "v2:tables_global", "v3:tables_lds", "v3:tables_global"})
_case("comps_one", 4, 721, 1440, {"a": ("stack", 2000, 512, 2, 0), "b": ("stack", 2000, 513, 2, 1)}, _cycle(["a", "b"]),
      {"one:tables_lds", "one:tables_global"})

# ---- staging edges (nwords = COMPS * 4 and the next word count the selection lets through) --------------------------------
# (<1024,288,-1,256>: 1152 words = 128 x 576; 1153 is prime and would need ny = 1153 > CTK_LDS_NY: 1154 = 577 x 2 instead)
_case("staged_v1_1152", 4, 128, 576, _edges((300, 1000), 100), _cycle(["r300", "r1000_", "r300_", "r1000"]), {"v1:staged"})
_case("staged_v1_1154", 4, 577, 100, _edges((300, 1000), 100), _cycle(["r300", "r1000_", "r300_", "r1000"]),
      {"v1:global_mask", "rowcount<512>"})
_pl = dict(QUIET, **_edges((1500, 2000), 200))                # <2048,512,1024,512>: 2048 = 32 x 4096 words and 2049 = 683 x 192
_case("staged_v2_2048", 513, 32, 4096, _pl, _quiet_then(["r1500", "r2000_"], 509), {"v2:staged", "overlap<8,256,1>"})
_case("staged_v2_2049", 513, 683, 192, _pl, _quiet_then(["r1500", "r2000_"], 509), {"v2:global_mask", "overlap<4,256,1>"})

# ---- overlap word edges -----------------------------------------------------------------------------------------------------
for _ny, _nx, _f in ((256, 256, "overlap<4,256,1>"), (205, 320, "overlap<5,256,1>"), (160, 512, "overlap<5,256,1>"),
                     (61, 1344, "overlap<6,256,1>"), (192, 512, "overlap<6,256,1>"), (29, 3392, "overlap<8,256,1>"),
                     (64, 2048, "overlap<8,256,1>"), (683, 192, "overlap<4,256,1>"), (8191, 64, "overlap<4,256,1>"),
                     (128, 4096, "overlap<4,512,1>")):
    _case("overlap_%dx%d" % (_ny, _nx), 6, _ny, _nx, _edges((100, 600), 300), _cycle(["r100", "r600_", "r600", "r100_"]), {_f, _f[:-1] + ",SEG>"})
_case("overlap_rows_258_words", 6, 32, 16449, _edges((100, 600), 300), _cycle(["r100", "r600_", "r600", "r100_"]), {"overlap<4,512,1>"})
_case("overlap_rows_313_words", 6, 8, 20000, _edges((100, 600), 300), _cycle(["r100", "r600_", "r600", "r100_"]), {"overlap<4,256,1>"})
_case("overlap_nx_65535", 6, 4, 65535, _edges((100, 600), 300), _cycle(["r100", "r600_", "r600", "r100_"]), {"overlap<4,256,1>"})

# ---- grid edges -------------------------------------------------------------------------------------------------------------
for _ny, _f in ((1024, "v1"), (1025, "glb"), (2048, "rowcount<512>"), (2049, "rowcount<256>")):
    _case("grid_ny_%d" % _ny, 4, _ny, 64, _edges((100, 900), 60), _cycle(["r100", "r900_", "r900", "r100_"]), {_f})
_case("lattice_721x1440", 2, 721, 1440, {"a": ("lattice",), "b": ("bars", "a")}, _cycle(["a", "b"]), {"glb"})

# ---- k_rowcount<RCU>: the 4 | 5 and 6 | 7 edges of the row groups a plane needs, and past 8 (a second, partial outer trip) ------------
# plane "a": full-height stacks in the word-boundary bands (runs across a boundary in every row, the last included) and seam rows;
# "b": one-row stacks and a seam row (x = nx - 1: the last word) in the LAST row; "c": that row filled from first to last pixel
def _rcu_planes(ny, nx):
    k = min((nx + 63) // 64 + 3, len(_bands(nx, 2, nx - 3)))
    return {"a": ("stack", 4 + k * ny, k + 2, 2, 0), "b": ("stack", 2 + k, k + 2, 1, ny - 1), "c": ("bars", "b")}


RCU_EDGES = [(360, 160, 256, 4), (360, 161, 256, 6), (360, 240, 256, 6), (360, 241, 256, 8), (360, 256, 256, 8), (360, 257, 512, 4),
             (360, 320, 512, 4), (360, 321, 512, 6), (360, 480, 512, 6), (360, 481, 512, 8), (360, 640, 512, 8), (360, 641, 512, 8),
             (1440, 32, 256, 4), (1440, 33, 256, 6), (1440, 48, 256, 6), (1440, 49, 256, 8), (1440, 64, 256, 8), (1440, 65, 256, 8),
             (130, 721, 512, 6), (4160, 20, 256, 0)]             # (nx, ny, threads, CTK_S_ROWCOUNT_GROUPS), T = 4
for _nx, _ny, _thr, _rcu in RCU_EDGES:
    _case("rcu_%dx%d" % (_ny, _nx), 4, _ny, _nx, _rcu_planes(_ny, _nx), _cycle(["a", "b", "c", "a"]), {"rowcount<%d,%d>" % (_thr, _rcu)}, seg=False)

# ---- pair edges: dots and the bars over them (one pair per dot, in both orders) -----------------------------------------------
for _p in (128, 129, 600):
    _case("pairs_%d" % _p, 6, 192, 288, {"d": ("stack", _p, _p, 0, 0), "b": ("bars", "d")}, _cycle(["d", "b"]), {"v1"})

# ---- the long shard: T = 65537 planes of 32 x 128 (64 words) -------------------------------------------------------------
LONG_T = 65537
LONG_BUSY = {"a": ("stack", 832, 240, 2, 0), "b": ("stack", 832, 241, 2, 1), "c": ("stack", 833, 288, 2, 0),
             "d": ("stack", 1024, 289, 2, 1), "e": ("stack", 1025, 300, 2, 0), "f": ("stack", 1024, 288, 2, 0)}


def long_schedule(busy_keys, t0=30000, n=400):
    return lambda T: [busy_keys[(t - t0) % len(busy_keys)] if t0 <= t < t0 + n else ("q0" if t % 2 else "q3") for t in range(T)]


_case("long_shard", LONG_T, 32, 128, dict(QUIET, **LONG_BUSY), long_schedule(["a", "b", "c", "d", "e", "f"]),
      {"v1_832", "v1hi_832", "v1_832:staged", "v1hi_832:staged", "v1_832:tables_lds", "v1_832:tables_global", "v1hi_832:tables_lds",
       "v1hi_832:tables_global", "rowcount<128>", "rowcount<128,4>", "overlap<4,128,5>", "overlap<4,128,5,SEG>"}, slow=True)
# the same shard without planes above 832 runs: no v1hi (the speculation test alternates the two)
LONG_QUIET_KEYS = ["a", "b"]


def planes_of(case):
    """{key: (ny, nx) uint8 plane}"""
    ny, nx = case["ny"], case["nx"]
    out = {}
    for k, spec in case["planes"].items():
        if spec[0] == "stack":
            out[k] = stack_plane(ny, nx, *spec[1:])
        elif spec[0] == "lattice":
            out[k] = lattice(ny, nx)
    for k, spec in case["planes"].items():
        if spec[0] == "bars":
            out[k] = bars_of(out[spec[1]])
    return out


def claimed(case, key):
    """(runs, comps) the case claims for a plane"""
    spec = case["planes"][key]
    if spec[0] == "stack":
        return spec[1], spec[2]
    ny, nx = case["ny"], case["nx"]
    if spec[0] == "lattice":
        n = ((ny + 1) // 2) * ((nx + 1) // 2)
        return n, n
    src = case["planes"][spec[1]]
    if src[0] == "lattice":
        return (ny + 1) // 2, (ny + 1) // 2
    n = int(bars_of(stack_plane(ny, nx, *src[1:])).any(axis=1).sum())
    return n, n


def schedule_of(case, T=None):
    return case["schedule"](case["T"] if T is None else T)


def mask_of(case, keys=None):
    """(T, ny, nx) uint8 mask of the case (or of another schedule of its planes)"""
    pl = planes_of(case)
    keys = schedule_of(case) if keys is None else keys
    names = sorted(set(keys))
    stack = np.stack([pl[k] for k in names])
    idx = np.array([names.index(k) for k in keys], dtype=np.int64)
    return stack[idx]


def case_forms(case):
    keys = schedule_of(case)
    rc = [claimed(case, k) for k in keys]
    return forms_reached(case["T"], case["ny"], case["nx"], [r for r, _ in rc], [c for _, c in rc],
                         seg=(False, True) if case["seg"] else (False,))


CASE_BY_NAME = {c["name"]: c for c in CASES}


# ---- speculation on one handle, same shape: (ny, nx, planes, [(T, keys of the timesteps), ...]) ------------------------------
_SPEC_PLANES = {"q700": ("stack", 700, 60, 2, 0), "q300": ("stack", 300, 40, 2, 1), "b4097": ("stack", 4097, 100, 2, 0),
                "b1500": ("stack", 1500, 100, 2, 1), "b3000": ("stack", 3000, 100, 2, 0), "b1000": ("stack", 1000, 60, 2, 1)}
_Q, _B = ["q700", "q300"], ["q700", "b4097", "b1500", "b3000"]
SPEC_SEQUENCES = [
    dict(name="spec_192x288", ny=192, nx=288, planes=_SPEC_PLANES, calls=[
        (8, _cycle(_Q)),                      # quiet: v1
        (8, _cycle(_B)),                      # busy, some plane above 4096 runs: v1 speculatively on too small buffers, then one + glb
        (8, _cycle(_Q)),                      # quiet again: the busy set (one + glb) speculatively
        (8, _cycle(_B)),                      # busy: v1 speculatively, then what is missing
        (16, _cycle(_Q)),                     # a longer T while glb is in the speculative set: no speculative launch
        (8, _cycle(["q300", "b1500"])),       # T <= 512 with a plane above 1024 runs
        (8, _cycle(["q300", "b1000"])),       # ... then at most 1024 runs
    ]),
    # a long shard whose need for v1hi changes: planes of at most 832 runs, then up to 1025, then at most 832 again
    dict(name="spec_long", ny=32, nx=128, planes=dict(QUIET, **LONG_BUSY), calls=[
        (LONG_T, long_schedule(LONG_QUIET_KEYS)),
        (LONG_T, long_schedule(["a", "b", "c", "d", "e", "f"])),
        (LONG_T, long_schedule(LONG_QUIET_KEYS)),
    ]),
]


def spec_calls(seq):
    """(T, ny, nx, runs of every plane) of every call of a speculation sequence"""
    for T, sched in seq["calls"]:
        keys = sched(T)
        yield T, seq["ny"], seq["nx"], [seq["planes"][k][1] for k in keys]
