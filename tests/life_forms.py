"""The launch rule of the run_lifecycle reductions (ctk_life_plan in contrack_amd/csrc/ctk_forms.h) and the limits of their kernels
(contrack_amd/csrc/ctk_lifecycle.hip) restated in Python, and label slabs placed on both sides of every limit.  No GPU needed:
tests/test_lifecycle_forms_host.py compares the restatement with the library's own rule, tests/test_gpu_lifecycle_forms.py runs the
slabs and asks ctk_debug_lifecycle_path which path every time step took.

Every builder returns a dict: flag (T, ny, nx) int32, lat, lon (None where the reference's frame is undefined), wrow, dates, and
`steps`, the rounds of k_lifecycle every time step must report (0: the strip kernels held it)."""
import numpy as np

# ---- the strip form (k_life_seam, k_life_strips, k_life_finish) and the fallback (k_lifecycle) --------------------------------
LB_SW = 256          # columns per strip
LB_WAVES = 4         # waves, i.e. bands of rw rows, per workgroup
LB_LH = 128          # LDS hash slots of a workgroup of k_life_strips
LB_GH = 256          # hash slots of a time step's table
LB_GN = 128          # ids per time step k_life_finish accepts
LB_KS = 4            # seam-crossing ids per time step of the strip form
LC_HASH = 1024       # hash slots of k_life_seam and k_lifecycle
LC_NL = 512          # ids per pass of k_lifecycle
KS_MAX, KS_BYTES = 32, 32768

SWEEP_T = (1, 6, 410, 2047, 2048, 2707)
SWEEP_NY = (1, 9, 33, 181, 721)
SWEEP_NX = (1, 4, 8, 255, 256, 257, 360, 1440, 2080)
# (T, ny, nx) -> (rw, nsx, nby); the first two are the design figures in the rule's own comment
PINNED = {(2707, 181, 360): (46, 2, 1), (480, 721, 1440): (37, 6, 5), (6, 721, 1440): (8, 6, 23), (2048, 181, 8): (46, 1, 1),
          (2047, 181, 8): (23, 1, 2), (410, 721, 8): (37, 1, 5)}


def rows_per_wave(T, ny, nx):
    nsx = (nx + LB_SW - 1) // LB_SW
    g = max(1, (ny + 80) // 160)
    while T * nsx * g < 2048 and (ny + 4 * g - 1) // (4 * g) > 8:
        g += 1
    return max(1, (ny + 4 * g - 1) // (4 * g))


def life_plan(T, ny, nx, f64=False, flag_align=0, field_align=0):
    """ctk_life_plan: flag_align / field_align are the slabs' device addresses modulo 32"""
    rw = rows_per_wave(T, ny, nx)
    nxw = (nx + 31) // 32
    vec = nx % 4 == 0 and flag_align % 16 == 0 and field_align % (32 if f64 else 16) == 0
    return dict(rw=rw, nsx=(nx + LB_SW - 1) // LB_SW, nby=(ny + rw * LB_WAVES - 1) // (rw * LB_WAVES), vec=int(vec),
                ks=max(1, min(KS_MAX, KS_BYTES // (nxw * 4))))


def _mul(ident):
    return ((int(ident) & 0xffffffff) * 2654435761) & 0xffffffff


def lb_start(ident, slots):
    """first slot lb_slot_insert<slots> probes"""
    return (_mul(ident) >> 16) & (slots - 1)


def lc_start(ident):
    """lc_hash: first slot lc_slot probes"""
    return _mul(ident) >> 22


def crossing_ids(plane):
    """ids present in both seam columns"""
    a, b = plane[:, 0], plane[:, -1]
    return np.intersect1d(a[a != 0], b[b != 0])


def expected_rounds(plane):
    """rounds of k_lifecycle a plane takes part in, from the limits alone: the strip form holds LB_GN ids of which LB_KS cross the
    seam; a pass of k_lifecycle holds LC_NL ids of which ks cross, else the ids are halved by residue class (uint32 id mod 2P)"""
    ids = np.unique(plane[plane != 0]).astype(np.int64) & 0xffffffff
    cross = crossing_ids(plane).astype(np.int64) & 0xffffffff
    if len(ids) <= LB_GN and len(cross) <= LB_KS:
        return 0
    ks = life_plan(1, plane.shape[0], plane.shape[1])["ks"]
    rounds, P = 1, 1
    while any(((ids % P) == j).sum() > LC_NL or ((cross % P) == j).sum() > ks for j in range(P)):
        rounds, P = rounds + 1, P * 2
    return rounds


def grid(ny, nx):
    """a regular grid away from the poles (positive row weights): lat, lon, wrow"""
    from contrack_amd.contrack import row_weights
    lat = np.linspace(60, 21, ny).astype(np.float32)
    lon = (np.arange(nx) * (360.0 / nx)).astype(np.float32)
    return lat, lon, row_weights(lat, 1.0, 1.0)


def field_for(flag, dtype, seed=0):
    return (np.random.default_rng(seed).random(flag.shape) * 50 + 100).astype(dtype)


def _case(flag, steps=None, frame=True, **extra):
    T, ny, nx = flag.shape
    lat, lon, wrow = grid(ny, nx)
    steps = [expected_rounds(p) for p in flag] if steps is None else list(steps)
    return dict(flag=flag, lat=lat if frame else None, lon=lon if frame else None, wrow=wrow, dates=["%04d" % t for t in range(T)],
                steps=steps, **extra)


# ---- a. ids per time step --------------------------------------------------------------------------------------------------
IDS_PER_STEP = [0, 127, 128, 129, 512, 513]
IDS_STEPS = [0, 0, 0, 1, 1, 2]


def ids_case(reverse=False):
    """6 x 40 x 64 (two workgroups of 20 rows per plane): ids 1..n of one or two pixels each.  Forward: four pixels apart from
    pixel 0 on, so that 128 ids fill the 128-slot LDS table of ONE workgroup to the last slot; reversed: spread over the plane, both
    workgroups, so that the time step's table and k_life_finish's count decide"""
    ny, nx = 40, 64
    counts = IDS_PER_STEP[::-1] if reverse else IDS_PER_STEP
    flag = np.zeros((len(counts), ny * nx), np.int32)
    for t, n in enumerate(counts):
        if n == 0:
            continue
        stride = max(4, (ny * nx) // n) if reverse else 4
        pos = np.arange(n) * stride
        flag[t, pos] = np.arange(1, n + 1)
        flag[t, pos[::2] + 1] = np.arange(1, n + 1)[::2]            # every other id has two pixels
    return _case(flag.reshape(-1, ny, nx), IDS_STEPS[::-1] if reverse else IDS_STEPS)


# ---- b. seam-crossing ids --------------------------------------------------------------------------------------------------
CROSS_PER_STEP = [4, 5, 32, 33]
CROSS_STEPS = [0, 1, 1, 2]


def _cross_row(row, ident, kind, nx, rng):
    """one row of a crossing id; kind 0: three equal largest gaps (the first wins), 1: every column, 2: the seam columns alone,
    3: two runs from the seam columns inwards"""
    if kind == 0:
        cols = np.array([0, (nx - 1) // 3, 2 * ((nx - 1) // 3), nx - 1])
    elif kind == 1:
        cols = np.arange(nx)
    elif kind == 2:
        cols = np.array([0, nx - 1])
    else:
        a, b = int(rng.integers(1, nx // 2 - 1)), int(rng.integers(nx // 2 + 1, nx - 1))
        cols = np.concatenate([np.arange(a + 1), np.arange(b, nx)])
    row[cols] = ident


def crossing_case():
    """4 x 80 x 64 (ks = 32): crossing ids 1000.. on two rows each, 36 other ids below them"""
    ny, nx = 80, 64
    rng = np.random.default_rng(41)
    flag = np.zeros((len(CROSS_PER_STEP), ny, nx), np.int32)
    for t, n in enumerate(CROSS_PER_STEP):
        for q in range(n):
            _cross_row(flag[t, 2 * q], 1000 + q, q % 4, nx, rng)
            if q % 3 == 0:
                flag[t, 2 * q + 1, :3] = 1000 + q
        k = 1
        for y in range(68, 80):
            for x in (5, 25, 45):
                flag[t, y, x:x + 2] = k
                k += 1
    assert life_plan(4, ny, nx)["ks"] == 32
    return _case(flag, CROSS_STEPS)


def narrow_case(nx):
    """3 x 9 x nx for nx = 1 (every id is in both seam columns, no gap exists: shift -2, the reference's frame is undefined) and
    nx = 2"""
    ny = 9
    flag = np.zeros((3, ny, nx), np.int32)
    if nx == 1:
        flag[0, [0, 3, 4, 8], 0] = [7, 9, 9, -3]                    # three ids, all crossing: the strip form holds them
        flag[1, :6, 0] = np.arange(11, 17)                          # six crossing ids: k_lifecycle
    else:
        flag[0, 0] = 5; flag[0, 2] = 6; flag[0, 3, 0] = 6           # two crossing ids, two that do not cross
        flag[0, 5, 0] = 7; flag[0, 8, 1] = 8
        for q in range(5):                                          # five crossing ids
            flag[1, q] = 20 + q
        flag[1, 7, 1] = 30
        flag[2, 4, 0] = 9
    return _case(flag, [0, 1, 0], frame=nx > 1)


WIDE_COLUMNS = [
    # per time step: (columns of a crossing id, its shift); 2048 = 8 strips of 256 columns = 64 words of column bits
    [([0, 500, 1000, 1500, 2079], 2079),                            # largest gap 1500 .. 2079, across 2047 / 2048
     (list(range(0, 2047)) + list(range(2050, 2080)), 2050),        # its only gap 2046 .. 2050
     ([0, 2047, 2048, 2079], 2047),
     ([0, 1024, 2048, 2079], 1024)],                                # two gaps of 1024: the first wins
    [([0, 2048, 2079], 2048),                                       # the gap ends on the first column of the second 64 words
     (list(range(0, 2048)) + [2079], 2079)],
]


def wide_case():
    """2 x 8 x 2080: nxw = 65 words of column bits (a second trip of k_life_finish's gap search), nine strips"""
    flag = np.zeros((2, 8, 2080), np.int32)
    for t, ids in enumerate(WIDE_COLUMNS):
        for q, (cols, _) in enumerate(ids):
            flag[t, 2 * q, cols] = 50 + q
        flag[t, 7, 100:110] = 3                                     # and one id that does not cross
    return _case(flag, [0, 0], shifts=[[s for _, s in ids] for ids in WIDE_COLUMNS])


# ---- c. the seam table ------------------------------------------------------------------------------------------------------
def seam_table_case():
    """1 x 520 x 4: 1040 ids in the seam columns, more than the 1024 slots of k_life_seam and k_lifecycle; each parity class holds
    520 > 512"""
    flag = np.zeros((1, 520, 4), np.int32)
    flag[0, :, 0] = np.arange(1, 521)
    flag[0, :, 3] = np.arange(521, 1041)
    return _case(flag, [3])


# ---- d. hash chains and the row order -------------------------------------------------------------------------------------
EXTREMES = [-2 ** 31, 2 ** 31 - 1, -1, -2, -77, -65536]


def _pick(n, start, want, skip=()):
    """the first n of 1, -1, 2, -2, ... whose probe chain starts at slot `want`"""
    k = np.arange(1, 400001, dtype=np.int64)
    cand = np.stack([k, -k], axis=1).reshape(-1)
    mul = (((cand & 0xffffffff).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)).astype(np.int64)     # (< 2^64)
    out =[int(v) for v in cand[start(mul) == want] if int(v) not in skip][:n]
    assert len(out) == n
    return out


def chain_ids():
    """100 ids whose probe chain starts at the last slot of the 128-slot AND of the 256-slot table, 300 whose chain starts at slot
    1023 of lc_hash"""
    first = _pick(100, lambda m: (m >> 16) & (LB_GH - 1), LB_GH - 1, EXTREMES)
    second = _pick(300, lambda m: m >> 22, LC_HASH - 1, set(EXTREMES) | set(first))
    assert all(lb_start(v, LB_LH) == LB_LH - 1 and lb_start(v, LB_GH) == LB_GH - 1 for v in first)
    assert all(lc_start(v) == LC_HASH - 1 for v in second)
    return first, second


def _scatter(plane, ids):
    """two neighbouring pixels per id, four pixels apart"""
    flat = plane.reshape(-1)
    pos = np.arange(len(ids)) * 4
    flat[pos] = ids
    flat[pos + 1] = ids


def chain_case():
    """2 x 24 x 64, one workgroup per plane.  Step 0: the 100 ids of the first set and the extreme ids (106 <= 128: strips);
    step 1: the 300 of the second set and the extreme ids again (k_lifecycle).  Label range 2^32: comparison sort"""
    first, second = chain_ids()
    flag = np.zeros((2, 24, 64), np.int32)
    _scatter(flag[0], np.array(first + EXTREMES, dtype=np.int64).astype(np.int32))
    _scatter(flag[1], np.array(EXTREMES + second, dtype=np.int64).astype(np.int32))
    assert life_plan(2, 24, 64)["nby"] == 1
    return _case(flag, [0, 1], sort=1)


def dense_case():
    """the twin: ids -40 .. 65 in both steps (counting sorts)"""
    ids = np.array([v for v in range(-40, 66) if v != 0], dtype=np.int32)
    flag = np.zeros((2, 24, 64), np.int32)
    _scatter(flag[0], ids)
    _scatter(flag[1], ids[::-1])
    return _case(flag, [0, 0], sort=0)


# ---- e. the production rows per wave ---------------------------------------------------------------------------------------
RW_CASES = [((2048, 181, 8), np.float32, dict(rw=46, nsx=1, nby=1)), ((2047, 181, 8), np.float32, dict(rw=23, nsx=1, nby=2)),
            ((410, 721, 8), np.float64, dict(rw=37, nsx=1, nby=5)), ((1024, 37, 260), np.float32, dict(rw=10, nsx=2, nby=1))]
CROSS_ROWS = (2, 4, 6, 12)                                           # rows of the crossing ids: inside the first wave's band


def rw_case(T, ny, nx):
    """33 non-empty steps (the first and the last among them), the same figures in each with 0 .. 4 crossing ids:
    id 1 a column of full height (and one in the partial last strip): every wave holds it in registers over its whole band;
    ids 2 / 3 alternating row by row in one column of the upper half: a lane hands its held id in on every row;
    ids 40.. seven rows tall, one right below the other in the lower half: a lane hands in an id it held over several rows (its
    first / last row bound the scans of ctk_lifecycle_exact);
    ids 10.. starting on the last row of a wave's band, three rows tall; id 5 on row ny-1; ids 6 / 7 single pixels in the corners;
    ids 100.. crossing the seam: seam columns alone | every column | a run and a pixel | pairs at both ends (nx = 8: two equal gaps,
    nx = 260: the gap ends on the strip boundary 256)"""
    rw = rows_per_wave(T, ny, nx)
    assert rw >= 10 and ny > 12
    flag = np.zeros((T, ny, nx), np.int32)
    for i, t in enumerate(np.unique(np.linspace(0, T - 1, 33).astype(int))):
        P = flag[t]
        P[:, 2] = 1
        if nx > 8:
            P[:, nx - 3] = 1
        half = ny // 2
        P[1:half:2, 5] = 2
        P[2:half:2, 5] = 3
        for k, y in enumerate(range(half, ny - 1, 7)):
            P[y:min(y + 7, ny - 1), 4:6] = 40 + k
        for w, y in enumerate(range(rw - 1, ny - 1, rw)):
            P[y:y + 3, 3 + 3 * (w % 2)] = 10 + w
        P[ny - 1, 3] = 5
        P[0, 0] = 6
        P[ny - 1, nx - 1] = 7
        for q in range(i % 5):
            y, ident = CROSS_ROWS[q], 100 + q
            if q == 0:
                P[y, [0, nx - 1]] = ident
            elif q == 1:
                P[y, :] = ident
            elif q == 2:
                P[y, [0, 1, nx - 1]] = ident
            else:
                P[y, [0, 3, nx - 4, nx - 1]] = ident
    return _case(flag, [0] * T)


# ---- f. the vector form -----------------------------------------------------------------------------------------------------
VEC_NX = (252, 255, 256, 257, 260)


def vec_case(nx, seed=0):
    """3 x 9 x nx: blobs as tests/life_util.py's random_life_case builds them in steps 0 and 1, 130 single pixels with an id each in
    step 2 (k_lifecycle)"""
    from scipy import ndimage
    rng = np.random.default_rng(7000 + nx + seed)
    T, ny = 3, 9
    f = ndimage.uniform_filter(rng.standard_normal((T, ny, nx)), size=(1, 3, 5), mode=("nearest", "nearest", "wrap"))
    flag = np.zeros((T, ny, nx), np.int32)
    for t in range(2):
        lab, n = ndimage.label(f[t] > 0.15)
        perm = rng.permutation(np.arange(1, n + 1)) * 7
        flag[t] = np.where(lab > 0, np.concatenate([[0], perm])[lab], 0)
        for y in range(ny):
            if flag[t, y, 0] and flag[t, y, -1] and rng.random() < 0.7:
                flag[t][flag[t] == flag[t, y, -1]] = flag[t, y, 0]
    flag[0][flag[0] == flag[0].max()] = -5
    flag[2].reshape(-1)[::(ny * nx) // 130][:130] = 5000 + np.arange(130)
    return _case(flag)


# ---- g. the row table grows -------------------------------------------------------------------------------------------------
def regrowth_case():
    """2 x 80 x 64 with 2560 ids in each step: 5120 rows >= 4 x (16 T + 1024), the table a fresh handle starts with"""
    T, ny, nx = 2, 80, 64
    flag = np.zeros((T, ny * nx), np.int32)
    for t in range(T):
        flag[t, t::2] = np.arange(1, ny * nx // 2 + 1)
    assert T * (ny * nx // 2) >= 4 * (16 * T + 1024)
    return _case(flag.reshape(T, ny, nx))
