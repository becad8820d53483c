"""One long-lived handle, every entry family: the operations, the written sequences and the seeded ones of
tests/test_gpu_handle_sequences.py, and what tests/test_handle_sequences_host.py checks about them without a GPU.

contrack_amd.contrack keeps one Tracker per device for the whole process, so every public call of a script goes through one
ctk_handle in whatever order and at whatever shapes the script chooses; the families' own tests each make a handle and use it for one
family.  What the families share on the handle -- io_in / io_out, the pinned chunk buffers, the copy stream and its events, the
resident anomaly and vertical-mean slabs, an_raw, the caches of thresholds, weights, threshold field and segments -- is what the
sequences here are written against.

An operation (`Op`) is a family, its arguments, and the reference function of that family's own test:
    tracking            oracle.run_contrack (the C oracle; threshold fields and resident slabs through the indicator slab, segments
                        through segment_util.expected)
    frequency           freq_util.counts
    spells              spell_util.spells
    composite           composite_util.composite
    level mean          level_util.level_mean
    anomalies           oracle/anom_port.py
    percentile          np.nanquantile on float64 columns (per grid point: ctk_debug_percentile_values); the band mean is k_nanmean's
                        documented order restated on those values (band_mean)
    percentile_groups   pctl_util.want;  percentile_field  pfield_util.want_field;  std_field  std_util.want_std
    lifecycle           life_util.numpy_rows for t / label / shift / area, life_util.numpy_exact_rows for the exact records of ALL rows
    band                band_util.band (area per step, columns, sectors; the resident forms on the anomaly slab of oracle/anom_port.py)
    centred             centred_util.centred (the reader form also answers for the chunks its reader was asked for)
    reversal            reversal_util.from_table on reversal_util.field over the shape's latitudes (REV_GRID: active rows in both
                        hemispheres, the first and the last row of the grid neither read nor written)
Every comparison is exact (bits or integers); there is no tolerance in this module.

The resident slab of the field to track has two producers, anomalies(keep) and reversal(keep): a consumer's `src` says which one made
the slab it works on (by_reversal), and its reference is computed on that producer's reference output (resident_slab).

`Op.io` is what the call asks of the shared buffers, computed from its arguments as the library computes it (bytes of io_in, io_out
and of one pinned buffer per direction; 0: not touched).  `Op.needs` / `Op.gives` / `Op.drops` name the resident slabs ("anom",
"level") it consumes, leaves and invalidates: the seeded generator draws a consumer only while its slab is resident.  The runner
compares `Op.io` with the handle's own capacities after every call (check_io), and `Op.breaks_exact` -- the call claims io_in /
io_out -- is what decides in exact_rows_follow_their_slabs whether the exact rows of an earlier lifecycle call are stale."""
import functools
import time

import numpy as np

import band_util
import centred_util
import composite_util
import freq_util
import label_forms
import level_util
import life_util
import oracle
import pctl_util
import pfield_util
import reversal_util
import segment_util
import spell_util
import std_util
from contrack_amd import synth
from oracle import anom_port

SHAPES = {"mult4": (24, 19, 36),          # plane a multiple of 4 pixels: the vector forms
          "odd": (37, 9, 65),             # odd plane: the scalar forms
          "large": (61, 31, 60)}          # every shared buffer sized by the first two must grow
SMALLEST = "mult4"
NLEV, LEVEL_W = 5, np.array([0.0, 1.5, 0.0, 2.0, 0.5])          # 5 levels, 3 selected, a hole between them
ANOM = dict(G=6, window=3, smooth=2)
DT = {"f4": np.float32, "f8": np.float64}
OVERLAP, TWOSIDED = 0.5, True
CHUNK_DEFAULT_BYTES = 256 << 20


class StateError(Exception):
    """what an operation that must be refused reports instead of a value"""


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the slabs, seeded as the families' tests seed theirs; computed once, never written -----------------------------------------
@functools.lru_cache(maxsize=None)
def slab(key, dtype="f4", seed=1):
    """tracking / composite / lifecycle field: synth.smooth_field; float64 is the float32 slab lifted (same mask, same result)"""
    T, ny, nx = SHAPES[key]
    return _frozen(np.ascontiguousarray(synth.smooth_field(T, ny, nx, seed=seed), dtype=DT[dtype]))


@functools.lru_cache(maxsize=None)
def wrow(key, variant=1):
    """row weights of a regular grid; variant 2: another profile over latitude (not a multiple of the first: overlaps change)"""
    _, ny, nx = SHAPES[key]
    lat = np.linspace(90, -90, ny).astype(np.float32)
    w = oracle.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    if variant == 2:
        w = (w * np.linspace(0.25, 4.0, ny, dtype=np.float32) + np.float32(50.0)).astype(np.float32)
    return _frozen(w)


@functools.lru_cache(maxsize=None)
def thresholds(key, value, per_step=False):
    T = SHAPES[key][0]
    if per_step:
        return _frozen(oracle.prepare_thresholds(np.linspace(value - 25.0, value + 25.0, T), T))
    return _frozen(oracle.prepare_thresholds(float(value), T))


@functools.lru_cache(maxsize=None)
def flags(key, seed=2):
    """frequency / spells / composite flag: spell_util.spell_flags"""
    T, ny, nx = SHAPES[key]
    return _frozen(spell_util.spell_flags(T, ny, nx, seed))


@functools.lru_cache(maxsize=None)
def groups(key, G=3):
    return _frozen((np.arange(SHAPES[key][0]) % G).astype(np.int32))


@functools.lru_cache(maxsize=None)
def anom_input(key, dtype="f4", seed=3):
    """anomaly input as tests/test_gpu_anom.py builds it: 5500 +- 50 with a seasonal cycle and NaNs"""
    T, ny, nx = SHAPES[key]
    rng = np.random.default_rng(seed)
    x = (50.0 * rng.standard_normal((T, ny, nx)) + 5500.0 + 30.0 * np.sin(np.arange(T) * 2 * np.pi / 365.0)[:, None, None]).astype(DT[dtype])
    x[rng.random(x.shape) < 0.01] = np.nan
    x[:, 0, 0] = np.nan
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def anom_groups(key):
    return _frozen(((np.arange(SHAPES[key][0]) + 17) % ANOM["G"]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def level_input(key, dtype="f4", seed=4):
    T, ny, nx = SHAPES[key]
    return _frozen(level_util.field(DT[dtype], T, NLEV, ny, nx, seed))


def level_selected(key, dtype="f4", seed=4):
    """what a reader delivers: the selected levels only, rising"""
    return np.ascontiguousarray(level_input(key, dtype, seed)[:, LEVEL_W != 0])


# ---- references (cached: a sequence may ask for the same one several times) -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_track(key, thr=100.0, gorl=">=", wvar=1, pers=2, per_step=False, seed=1):
    f, n = oracle.run_contrack(slab(key, "f4", seed), thresholds(key, thr, per_step), gorl, wrow(key, wvar), OVERLAP, pers, TWOSIDED)
    return _frozen(f), n


def indicator(x, thr, gorl):
    """numpy's compare as a float32 0 / 1 slab (NaN compares false): the oracle on it at 0.5 is the tracking of any compare"""
    import operator
    op = {">=": operator.ge, "<=": operator.le, ">": operator.gt, "<": operator.lt}[gorl]
    with np.errstate(invalid="ignore"):
        return op(x, thr).astype(np.float32)


def want_track_indicator(ind, key, wvar=1, pers=2):
    f, n = oracle.run_contrack(ind, np.full(ind.shape[0], 0.5), ">=", wrow(key, wvar), OVERLAP, pers, TWOSIDED)
    return f, n


@functools.lru_cache(maxsize=None)
def threshold_planes(key, nplanes=3, dtype="f8"):
    """a smooth threshold field around 100 and the plane of every step (tests/test_gpu_threshold_field.py)"""
    T, ny, nx = SHAPES[key]
    rng = np.random.default_rng(nplanes)
    y = np.linspace(0.0, np.pi, ny)[None, :, None]
    x = np.linspace(0.0, 2 * np.pi, nx, endpoint=False)[None, None, :]
    ph = rng.uniform(0.0, 2 * np.pi, (nplanes, 3, 1, 1))
    f = 100.0 + 40.0 * (np.sin(2 * y + ph[:, 0]) * np.cos(3 * x + ph[:, 1]) + 0.5 * np.cos(x + y + ph[:, 2]))
    return _frozen(f.astype(DT[dtype])), _frozen((np.arange(T) % nplanes).astype(np.int32))


@functools.lru_cache(maxsize=None)
def want_track_field(key, seed=1):
    planes, pos = threshold_planes(key)
    return want_track_indicator(indicator(slab(key, "f4", seed), planes[pos], ">="), key)


def segment_starts(key):
    T = SHAPES[key][0]
    return np.array([0, T // 3, T // 3 + 1, (2 * T) // 3], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def want_track_segments(key, thr=100.0, seed=1):
    return segment_util.expected(slab(key, "f4", seed), thresholds(key, thr), ">=", wrow(key), OVERLAP, 2, TWOSIDED, segment_starts(key))


@functools.lru_cache(maxsize=None)
def want_anom(key, dtype="f4", seed=3, segments=False):
    x = anom_input(key, dtype, seed)
    g = anom_groups(key)
    with np.errstate(invalid="ignore"):
        clim = anom_port.calc_clim(x, g, ANOM["G"], ANOM["window"])
        if not segments:
            return _frozen(anom_port.calc_anom(x, g, ANOM["G"], ANOM["window"], ANOM["smooth"])), _frozen(clim.astype(x.dtype))
        # the climatology of the whole slab, then the port's calc_anom on every segment (tests/test_gpu_anom_segments.py)
        out = np.empty_like(x)
        for a, b in segment_util.bounds(segment_starts(key), x.shape[0]):
            out[a:b] = anom_port.calc_anom(x[a:b], g[a:b], ANOM["G"], ANOM["window"], ANOM["smooth"], clim=clim)
        return _frozen(out), _frozen(clim.astype(x.dtype))


@functools.lru_cache(maxsize=None)
def want_level(key, dtype="f4", seed=4):
    return _frozen(level_util.level_mean(level_input(key, dtype, seed), LEVEL_W))


@functools.lru_cache(maxsize=None)
def want_anom_of_level(key, dtype="f4", seed=4):
    x = want_level(key, dtype, seed)
    g = anom_groups(key)
    with np.errstate(invalid="ignore"):
        return (_frozen(anom_port.calc_anom(x, g, ANOM["G"], ANOM["window"], ANOM["smooth"])),
                _frozen(anom_port.calc_clim(x, g, ANOM["G"], ANOM["window"]).astype(x.dtype)))


def band_rows(key):
    """the rows [y0, y1) of the percentile entries and of the band entries"""
    ny = SHAPES[key][1]
    return 1, ny - 2


def want_quantile_values(x, key, q):
    import warnings
    y0, y1 = band_rows(key)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        return np.nanquantile(np.asarray(x)[:, y0:y1].astype(np.float64), q, axis=0).ravel()


# ---- the reversal index: inputs and reference (reversal_util) -------------------------------------------------------------------
# per shape: delta in degrees and the latitude band.  Active rows in both hemispheres; rows 0 and ny - 1 are neither active nor
# anybody's partner, so of every plane only rows [r0, r1) with r0 > 0 travel in and rows [a0, a1) with a1 < ny travel out
REV_GRID = {"mult4": (20.0, (30, 50)), "odd": (22.5, (40, 50)), "large": (12.0, (30, 66))}
REV_GHGS2 = -5.0


def rev_lat(key):
    return np.linspace(90.0, -90.0, SHAPES[key][1])


@functools.lru_cache(maxsize=None)
def rev_input(key, dtype="f4", seed=0):
    """reversal_util.field on the shape's latitudes: the mean profile of 500 hPa height with weather"""
    T, ny, nx = SHAPES[key]
    return _frozen(reversal_util.field(rev_lat(key), nx, steps=T, seed=seed, dtype=DT[dtype]))


def rev_table(key, second=False):
    delta, bounds = REV_GRID[key]
    return reversal_util.table(rev_lat(key), delta=delta, ghgs2=REV_GHGS2 if second else None, lat_bounds=bounds)


def rev_rows(key, second=False):
    """(r0, r1, a0, a1): the rows some active row reads and the rows the active rows span (ctk_reversal_rows)"""
    tab = rev_table(key, second)
    act = np.flatnonzero(tab["eq"] >= 0)
    read = np.concatenate([act, tab["eq"][act], tab["po"][act]] + ([tab["eq2"][act]] if second else []))
    return int(read.min()), int(read.max()) + 1, int(act.min()), int(act.max()) + 1


@functools.lru_cache(maxsize=None)
def want_reversal(key, dtype="f4", seed=0, mask=False, second=False):
    return _frozen(reversal_util.from_table(rev_input(key, dtype, seed), rev_table(key, second), mask=mask))


# ---- what is resident: the `src` of a consumer -----------------------------------------------------------------------------------
# (key, dtype, seed, segments) names the slab anomalies(..., keep=True) left, (key, dtype, seed, ("reversal", mask, second)) the one
# reversal(..., keep=True) left: the fourth entry tells the producers apart
def by_reversal(src):
    return isinstance(src[3], tuple)


def resident_slab(src):
    """the reference's values of the resident slab a consumer works on"""
    if by_reversal(src):
        return want_reversal(src[0], src[1], src[2], *src[3][1:])
    return want_anom(*src)[0]


def resident_cut(src):
    """(threshold, compare) that makes a flag of the slab: anomalies of 40 or more, an index above 0 (include/contrack_hip.h)"""
    return (0.0, ">") if by_reversal(src) else (40.0, ">=")


@functools.lru_cache(maxsize=None)
def resident_flag(src):
    """the flag a lifecycle / composite of the resident anomaly slab works on: the oracle's tracking of that slab (cached: an
    operation's run asks for it as well, and the C oracle is only ever called where the references are computed)"""
    a = resident_slab(src)
    f, _ = want_track_indicator(indicator(a, *resident_cut(src)), src[0])
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def life_flag(key, seed=1):
    return want_track(key, 100.0, ">=", 1, 2, False, seed)[0]


def want_life(flag, field, key):
    """(rows, exact records): t / label / shift from life_util.numpy_rows, the exact records from life_util.numpy_exact_rows, and the
    rows' area as include/contrack_hip.h states it -- the exact sum of the weights, rounded once (math.fsum; numpy's own sum rounds
    along the way and differs from it in the last bit on a few contours of these slabs)"""
    import math
    rows = life_util.numpy_rows(flag, field, wrow(key))
    w = wrow(key).astype(np.float64)
    for r in rows:
        r["area"] = math.fsum((w * np.count_nonzero(flag[r["t"]] == r["label"], axis=1)).tolist())
    return rows, life_util.numpy_exact_rows(flag, field, wrow(key), rows, extent=True)


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def same_flag(got, want):
    return got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and got[1] == want[1]


def same_ints(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    return len(got) == len(want) and all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))


def same_composite(got, want):
    return composite_util.same_bits(got[0], want[0]) and got[1].dtype == np.uint32 and np.array_equal(got[1], want[1])


def same_values(got, want):
    """float arrays of one dtype: NaN where the reference has NaN, the reference's value everywhere else (+0 equals -0, as the anomaly
    tests compare)"""
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def same_bits64(got, want):
    """float64 results as the percentile and std tests compare them: the reference's value, NaN where it has NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def same_std(got, want):
    return same_bits64(got[0], want[0]) and same_bits64(got[1], want[1]) and got[2].dtype == np.uint32 and np.array_equal(got[2], want[2])


def same_life(got, want):
    rows, ex = got
    wrows, wex = want
    if len(rows) != len(wrows) or len(set(zip(rows["t"].tolist(), rows["label"].tolist()))) != len(rows):
        same_life.detail = "%d rows, %d wanted" % (len(rows), len(wrows))
        return False
    off = [k for k in ("t", "label", "shift", "area") if not np.array_equal(rows[k], wrows[k])]
    off += ["exact " + k for k in ("area", "swv", "s", "sy", "sx") if not np.array_equal(ex[k], wex[k], equal_nan=True)]
    same_life.detail = "rows differ in " + ", ".join(off)
    return not off


def nothing(got, want):
    return got is None


# ---- what a call asks of the shared buffers -------------------------------------------------------------------------------------
def _chunk(chunk_steps, T, step_bytes, least=1):
    c = chunk_steps if chunk_steps and chunk_steps > 0 else max(1, CHUNK_DEFAULT_BYTES // max(step_bytes, 1))
    return min(max(c, least), T)


def stream_io(key, chunk_steps, in_bytes, second_bytes=0, out_bytes=0, reader=False, reader2=False, writer=False, halo_in=0, halo_out=0, nsel=1):
    """two chunk-sized device buffers per direction (stream_setup); the second slab of a call travels through io_out / pin_out"""
    T, ny, nx = SHAPES[key]
    plane = ny * nx
    c = _chunk(chunk_steps, T, nsel * plane * in_bytes, max(halo_in, 1))
    io = dict(io_in=2 * (c + halo_in) * nsel * plane * in_bytes, io_out=0, pin_in=0, pin_out=0, chunk=c, chunks=-(-T // c))
    if reader:
        io["pin_in"] = (c + halo_in) * nsel * plane * in_bytes
    side = second_bytes or out_bytes
    if side:
        io["io_out"] = 2 * (c + halo_out) * plane * side
        if reader2 or writer:
            io["pin_out"] = (c + halo_out) * plane * side
    return io


def array_io(key, in_bytes=0, out_bytes=0):
    T, ny, nx = SHAPES[key]
    return dict(io_in=T * ny * nx * in_bytes, io_out=T * ny * nx * out_bytes, pin_in=0, pin_out=0)


NO_IO = dict(io_in=0, io_out=0, pin_in=0, pin_out=0)
BUFFERS = ("io_in", "io_out", "pin_in", "pin_out")
RUNS_IO_OUT = 256                      # track_to_host claims io_out: 256 bytes while the result travels as run tables (the default)


def dense_blocks(key):
    """a tracking result that leaves as run tables (track_to_host, and track_stream_impl with an array as the sink): deliver_runs
    claims io_out again for every block of time steps that holds a complex component, with that block's dense bytes -- which blocks
    do depends on the data; all of them together are the dense result"""
    T, ny, nx = SHAPES[key]
    return dict(io_out=T * ny * nx * 4)


class Op:
    """one call on the shared handle: run(trk, env) -> value, want() -> reference value, same(value, reference) -> bool"""

    def __init__(self, family, key, run, want, same, io=NO_IO, needs=None, gives=None, drops=(), tracking=False, note="", args=None, io_upto=None):
        self.family, self.key, self.run, self.want, self.same, self.io = family, key, run, want, same, dict(io)
        self.needs, self.gives, self.drops, self.tracking, self.note = needs, gives, tuple(drops), tracking, note
        self.args = args or {}
        # what the call asks of a buffer at the most, where that depends on the data (the dense blocks of a tracking result): `io` is
        # then the least it asks
        self.io_upto = dict(io_upto or {})

    @property
    def breaks_exact(self):
        """the call claims io_in / io_out (claim_io) or releases them: the exact rows of an earlier host-array lifecycle call are stale
        after it.  (Not the whole rule: a call that writes or drops the resident anomaly slab also breaks the rows of a lifecycle call
        with field = None.)"""
        return bool(self.io["io_in"] or self.io["io_out"]) or self.family == "release_io"

    def __repr__(self):
        return "%s[%s%s]" % (self.family, self.key, (" " + self.note) if self.note else "")


class Env:
    """what a sequence carries besides the handle: the rows of the last lifecycle op and the generations the producers left"""

    def __init__(self):
        self.life = None              # (rows, key of the shape, lat / lon / dates arguments) of the last lifecycle op
        self.generation = None        # of the resident anomaly slab, as its producer left it
        self.stale_generation = None  # ... and of the slab the producer before that one left
        self.level_generation = None


def _chunks_reader(source, fail_chunk=None, calls=None):
    """reader(t0, nt, out) over a host array; fail_chunk: gives up (raises) on that call, counted from 1"""
    count = [0]

    def rd(t0, nt, out):
        count[0] += 1
        if calls is not None:
            calls.append((t0, nt))
        if fail_chunk is not None and count[0] == fail_chunk:
            raise ReaderGaveUp("chunk %d" % count[0])
        out[...] = source[t0:t0 + nt]
    return rd


class ReaderGaveUp(RuntimeError):
    pass


def gave_up(got, want):
    return isinstance(got, ReaderGaveUp)


def _catching(fn, exc):
    def run(trk, env):
        try:
            fn(trk, env)
        except exc as e:
            return e
        return None
    return run


def _state_errors():
    from contrack_amd import _native
    return _native.ContrackHipError


STATE_RC = "rc=-6"                     # CTK_E_STATE as _native.check words it


def _refusing(fn):
    """the call must raise ContrackHipError and not a ValueError (that is a bad argument); what it says is compared by the op.  Any
    other exception -- a call that was not refused may stumble over what it read -- is handed to the comparison as it is, which then
    reports the op instead of ending the sequence"""
    def run(trk, env):
        try:
            fn(trk, env)
        except Exception as e:                                      # noqa: BLE001
            if isinstance(e, _state_errors()) and not isinstance(e, ValueError):
                return StateError(str(e))
            return e
        return None
    return run


def refused_with(*words):
    """the refusal names its cause: every one of `words` is in the message (STATE_RC: the library answered CTK_E_STATE)"""
    def same(got, want):
        return isinstance(got, StateError) and all(w in str(got) for w in words)
    return same


CMP = {">=": 0, "<=": 1, ">": 2, "<": 3}


# ---- tracking -------------------------------------------------------------------------------------------------------------------
def track(key, dtype="f4", thr=100.0, gorl=">=", wvar=1, per_step=False, pers=2, seed=1):
    def run(trk, env):
        f, n = trk.track(slab(key, dtype, seed), thresholds(key, thr, per_step), CMP[gorl], wrow(key, wvar), OVERLAP, pers, TWOSIDED, f64=dtype == "f8")
        return f.copy(), n
    io = array_io(key, 4 if dtype == "f4" else 8)
    io["io_out"] = RUNS_IO_OUT
    return Op("track", key, run, lambda: want_track(key, thr, gorl, wvar, pers, per_step, seed), same_flag, io, io_upto=dense_blocks(key),
              tracking=True, note="%s thr=%g%s %s w%d" % (dtype, thr, " per step" if per_step else "", gorl, wvar),
              args=dict(dtype=dtype, thr=thr, gorl=gorl, wvar=wvar, per_step=per_step))


def track_field(key, dtype="f4", seed=1):
    """set_threshold_field, track with thr=None, clear_threshold_field"""
    def run(trk, env):
        planes, pos = threshold_planes(key)
        trk.set_threshold_field(planes, pos)
        try:
            f, n = trk.track(slab(key, dtype, seed), None, 0, wrow(key), OVERLAP, 2, TWOSIDED, f64=dtype == "f8")
            return f.copy(), n
        finally:
            trk.clear_threshold_field()
    return Op("track_field", key, run, lambda: want_track_field(key, seed), same_flag, dict(array_io(key, 4 if dtype == "f4" else 8), io_out=RUNS_IO_OUT),
              io_upto=dense_blocks(key), tracking=True, note=dtype)


def track_segments(key, thr=100.0, seed=1):
    """set_segments, track, clear_segments"""
    def run(trk, env):
        trk.set_segments(segment_starts(key))
        try:
            f, n = trk.track(slab(key, "f4", seed), thresholds(key, thr), 0, wrow(key), OVERLAP, 2, TWOSIDED)
            return f.copy(), n
        finally:
            trk.clear_segments()
    return Op("track_segments", key, run, lambda: want_track_segments(key, thr, seed), same_flag, dict(array_io(key, 4), io_out=RUNS_IO_OUT), io_upto=dense_blocks(key),
              tracking=True)


def track_stream(key, dtype="f4", chunk_steps=0, callbacks=False, fail_chunk=None, thr=100.0, seed=1):
    esz = 4 if dtype == "f4" else 8
    T, ny, nx = SHAPES[key]

    def run(trk, env):
        a = slab(key, dtype, seed)
        if not callbacks:
            f, n = trk.track_stream(a, thresholds(key, thr), 0, wrow(key), OVERLAP, 2, TWOSIDED, chunk_steps=chunk_steps)
            return f, n
        out = np.full((T, ny, nx), -7, dtype=np.int32)

        def writer(t0, nt, chunk):
            out[t0:t0 + nt] = chunk
        _, n = trk.track_stream(_chunks_reader(a, fail_chunk), thresholds(key, thr), 0, wrow(key), OVERLAP, 2, TWOSIDED, sink=writer, shape=(T, ny, nx),
                                dtype=DT[dtype], chunk_steps=chunk_steps)
        return out, n
    io = stream_io(key, chunk_steps, esz, out_bytes=4 if callbacks else 0, reader=callbacks, writer=callbacks)
    if fail_chunk is not None:
        return Op("track_stream", key, _catching(run, ReaderGaveUp), lambda: None, gave_up, io, note="reader gives up on chunk %d" % fail_chunk,
                  args=dict(fail_chunk=fail_chunk))
    return Op("track_stream", key, run, lambda: want_track(key, thr, ">=", 1, 2, False, seed), same_flag, io, io_upto=None if callbacks else dense_blocks(key), tracking=True,
              note="%s chunk=%d%s" % (dtype, chunk_steps, " reader+writer" if callbacks else ""), args=dict(dtype=dtype))


def track_dev(key, dtype="f4", thr=100.0, seed=1):
    """slab and result in the caller's device buffers, twice: the second call runs speculatively on the first one's capacities"""
    T, ny, nx = SHAPES[key]

    def run(trk, env):
        a = slab(key, dtype, seed)
        d_in, d_out = trk.malloc(a.nbytes), trk.malloc(T * ny * nx * 4)
        try:
            trk.h2d(d_in, a)
            res = []
            for _ in range(2):
                trk.memset(d_out, 0xff, T * ny * nx * 4)
                n = trk.track_dev(d_in, T, ny, nx, thresholds(key, thr), 0, wrow(key), OVERLAP, 2, TWOSIDED, d_out, f64=dtype == "f8")
                out = np.empty((T, ny, nx), dtype=np.int32)
                trk.d2h(out, d_out)
                res.append((out, n, trk.stats()["label_forms"]))
            return res
        finally:
            trk.free(d_in)
            trk.free(d_out)
    def same(got, want):
        # the second call launched the set the first one left (label_forms.Handle), and nothing of it was discarded
        return len(got) == 2 and all(same_flag(g[:2], want) for g in got) and got[1][2] == second_call_forms(key, thr, seed)["forms"]
    return Op("track_dev", key, run, lambda: want_track(key, thr, ">=", 1, 2, False, seed), same, NO_IO, tracking=True,
              note="%s twice" % dtype, args=dict(thr=thr, seed=seed))


@functools.lru_cache(maxsize=None)
def second_call_forms(key, thr=100.0, seed=1):
    """the project's model of the labelling launches (label_forms.Handle) for a call that repeats the call before it: whether it
    launches speculatively, whether the launch is kept, and the CTK_S_LABEL_FORMS bits it reports.  What the first call leaves depends
    on its planes alone (the run capacity it leaves holds its runs whatever the handle held before), so this holds on a handle of any
    age."""
    T, ny, nx = SHAPES[key]
    runs = label_forms.count_runs(indicator(slab(key, "f4", seed), thresholds(key, thr)[:, None, None], ">="))
    m = label_forms.Handle()
    m.label2d(T, ny, nx, runs)
    speculative = m.runs_cap > 0 and m.spec_shape == (ny, nx) and (not m.spec["glb"] or m.spec_T >= T)
    forms = m.label2d(T, ny, nx, runs)
    return dict(speculative=speculative, kept=not forms & label_forms.DISCARDED_BIT, forms=forms)


def track_resident(src, thr=None, gorl=None):
    key = src[0]
    thr, gorl = (resident_cut(src)[0] if thr is None else thr), (gorl or resident_cut(src)[1])

    def run(trk, env):
        f, n = trk.track_resident(thresholds(key, thr), CMP[gorl], wrow(key), OVERLAP, 2, TWOSIDED)
        return f.copy(), n
    return Op("track_resident", key, run, lambda: want_track_indicator(indicator(resident_slab(src), thr, gorl), key), same_flag,
              dict(NO_IO, io_out=RUNS_IO_OUT), io_upto=dense_blocks(key), needs="anom", tracking=True)


# ---- frequency, spells, composite -----------------------------------------------------------------------------------------------
def _dev_flag(trk, f):
    d = trk.malloc(f.nbytes)
    trk.h2d(d, f)
    return d


def frequency(key, how="array", chunk_steps=0, G=3, above=0, fail_chunk=None, seed=2):
    T, ny, nx = SHAPES[key]
    ids = groups(key, G) if G > 1 else None

    def run(trk, env):
        f = flags(key, seed)
        if how == "array":
            return trk.frequency(f, ids, G, above, chunk_steps)
        if how == "cb":
            return trk.frequency_cb(_chunks_reader(f, fail_chunk), (T, ny, nx), ids, G, above, chunk_steps)
        d = _dev_flag(trk, f)
        try:
            return trk.frequency_dev(d, T, ny, nx, ids, G, above)
        finally:
            trk.free(d)
    fam = {"array": "frequency", "cb": "frequency_cb", "dev": "frequency_dev"}[how]
    io = NO_IO if how == "dev" else stream_io(key, chunk_steps, 4, reader=how == "cb")
    if fail_chunk is not None:
        return Op(fam, key, _catching(run, ReaderGaveUp), lambda: None, gave_up, io, note="reader gives up on chunk %d" % fail_chunk, args=dict(fail_chunk=fail_chunk))
    return Op(fam, key, run, lambda: freq_util.counts(flags(key, seed), ids, G, above), same_ints, io, note="chunk=%d G=%d" % (chunk_steps, G))


def spells(key, how="array", chunk_steps=0, G=3, by_id=True, min_duration=2, segments=False, seed=2):
    T, ny, nx = SHAPES[key]
    ids = groups(key, G) if G > 1 else None
    seg = segment_starts(key) if segments else None

    def run(trk, env):
        f = flags(key, seed)
        kw = dict(group=ids, ngroups=G, above=0, by_id=by_id, min_duration=min_duration, segments=seg)
        if how == "array":
            return trk.spells(f, chunk_steps=chunk_steps, **kw)
        if how == "cb":
            return trk.spells_cb(_chunks_reader(f), (T, ny, nx), chunk_steps=chunk_steps, **kw)
        d = _dev_flag(trk, f)
        try:
            return trk.spells_dev(d, T, ny, nx, **kw)
        finally:
            trk.free(d)
    fam = {"array": "spells", "cb": "spells_cb", "dev": "spells_dev"}[how]
    io = NO_IO if how == "dev" else stream_io(key, chunk_steps, 4, reader=how == "cb")
    return Op(fam, key, run, lambda: spell_util.spells(flags(key, seed), ids, G, 0, by_id, min_duration, seg), same_ints, io,
              note="chunk=%d%s" % (chunk_steps, " own segments" if segments else ""))


def composite(key, how="array", dtype="f4", chunk_steps=0, G=3, skipna=False, seed=2):
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8
    ids = groups(key, G) if G > 1 else None

    def run(trk, env):
        f, x = flags(key, seed), slab(key, dtype)
        if how == "array":
            return trk.composite(f, x, ids, G, 0, skipna, chunk_steps)
        if how == "cb":
            return trk.composite_cb(_chunks_reader(f), _chunks_reader(x), (T, ny, nx), DT[dtype], ids, G, 0, skipna, chunk_steps)
        d, dx = _dev_flag(trk, f), trk.malloc(x.nbytes)
        try:
            trk.h2d(dx, x)
            return trk.composite_dev(d, dx, T, ny, nx, ids, G, 0, skipna, f64=dtype == "f8")
        finally:
            trk.free(d)
            trk.free(dx)
    fam = {"array": "composite", "cb": "composite_cb", "dev": "composite_dev"}[how]
    io = NO_IO if how == "dev" else stream_io(key, chunk_steps, esz, second_bytes=4, reader=how == "cb", reader2=how == "cb")
    return Op(fam, key, run, lambda: composite_util.composite(flags(key, seed), slab(key, dtype), ids, G, 0, skipna), same_composite, io,
              note="%s chunk=%d" % (dtype, chunk_steps), args=dict(dtype=dtype))


def composite_resident(src, G=3):
    key = src[0]
    ids = groups(key, G)

    def run(trk, env):
        return trk.composite(resident_flag(src), None, ids, G, 0, True, 0, resident_f64=src[1] == "f8")
    return Op("composite_resident", key, run, lambda: composite_util.composite(resident_flag(src), resident_slab(src), ids, G, 0, True), same_composite,
              stream_io(key, 0, 4), needs="anom")


# ---- band: area per step, Hovmoeller columns, sector series ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def band_weights(key):
    return _frozen(band_util.cos_weights(SHAPES[key][1]))


def band_sectors(key):
    nx = SHAPES[key][2]
    return [(0, 10), (nx - 6, 12)]                         # the second one wraps


@functools.lru_cache(maxsize=None)
def wide_field(key, dtype="f4", seed=0):
    """values as centred_util.wide_case makes them: a reordered or split float64 sum of these shows in the bits"""
    T, ny, nx = SHAPES[key]
    rng = np.random.default_rng(seed)
    return _frozen((rng.standard_normal((T, ny, nx)) * 10.0 ** rng.uniform(-8, 10, (T, ny, nx))).astype(DT[dtype]))


def same_band(got, want):
    """band_util.same (dtype, shape and bits of every table, and no table too many) as a bool"""
    try:
        band_util.same(got, want)
    except AssertionError as e:
        same_band.detail = str(e)
        return False
    return True


def _band_call(trk, how, key, f, x, field, chunk_steps, sects, columns, readers=(None, None), resident_gen=None, resident_f64=False):
    T, ny, nx = SHAPES[key]
    rows, w = band_rows(key), band_weights(key)
    if how == "array":
        return trk.band(f, rows, w, x, sects, columns, 0, chunk_steps, resident_gen=resident_gen, resident_f64=resident_f64)
    if how == "cb":
        return trk.band_cb(readers[0], readers[1], (T, ny, nx), DT[field] if field else None, rows, w, sects, columns, 0, chunk_steps, resident_gen=resident_gen)
    d, dx = _dev_flag(trk, f), (trk.malloc(x.nbytes) if x is not None else None)
    try:
        if x is not None:
            trk.h2d(dx, x)
        return trk.band_dev(d, dx, T, ny, nx, rows, w, sects, columns, 0, f64=field == "f8", resident_gen=resident_gen)
    finally:
        trk.free(d)
        if dx is not None:
            trk.free(dx)


def band_io(key, how, field, chunk_steps, travels):
    """band_stream_impl: a field that travels is the first slab and sets the chunk length, the flags then take io_out (pin_out with a
    flag reader); otherwise the flags are the only slab.  band_dev claims neither"""
    if how == "dev":
        return NO_IO
    if travels:
        return stream_io(key, chunk_steps, 4 if field == "f4" else 8, second_bytes=4, reader=how == "cb", reader2=how == "cb")
    return stream_io(key, chunk_steps, 4, reader=how == "cb")


def band(key, how="array", field=None, chunk_steps=0, sectors=True, columns=True, fail_chunk=None, fail_which="flag", seed=2):
    """fail_which: the reader that gives up on its call `fail_chunk` -- "flag" or "field" """
    assert how in ("array", "cb", "dev") and field in (None, "f4", "f8") and (sectors or columns) and fail_which in ("flag", "field")
    sects = band_sectors(key) if sectors else None
    x = lambda: wide_field(key, field) if field else None                                     # noqa: E731

    def run(trk, env):
        f = flags(key, seed)
        readers = (_chunks_reader(f, fail_chunk if fail_which == "flag" else None),
                   _chunks_reader(x(), fail_chunk if fail_which == "field" else None) if field else None)
        return _band_call(trk, how, key, f, x(), field, chunk_steps, sects, columns, readers)
    fam = {"array": "band", "cb": "band_cb", "dev": "band_dev"}[how]
    io = band_io(key, how, field, chunk_steps, field is not None)
    note = "%s chunk=%d%s%s" % (field or "no field", chunk_steps, " columns" if columns else "", " sectors" if sectors else "")
    if fail_chunk is not None:
        assert how == "cb" and (field or fail_which == "flag")
        return Op(fam, key, _catching(run, ReaderGaveUp), lambda: None, gave_up, io, note="%s: the %s reader gives up on chunk %d" % (note, fail_which, fail_chunk),
                  args=dict(fail_chunk=fail_chunk, fail_which=fail_which, how=how))
    y0, y1 = band_rows(key)
    return Op(fam, key, run, lambda: band_util.band(flags(key, seed), y0, y1, band_weights(key), 0, x(), sects, columns), same_band, io, note=note,
              args=dict(dtype=field, how=how, sectors=sectors, columns=columns))


def band_resident(src, how="array", chunk_steps=0):
    """the field is the resident anomaly slab, named by the generation its producer left; the flags are the tracking of that slab.
    The streamed forms still send the flags through io_in"""
    key = src[0]
    sects = band_sectors(key)

    def run(trk, env):
        f = resident_flag(src)
        return _band_call(trk, how, key, f, None, src[1], chunk_steps, sects, True, (_chunks_reader(f), None), resident_gen=env.generation, resident_f64=src[1] == "f8")
    y0, y1 = band_rows(key)
    return Op("band_resident", key, run, lambda: band_util.band(resident_flag(src), y0, y1, band_weights(key), 0, resident_slab(src), sects, True), same_band,
              band_io(key, how, src[1], chunk_steps, False), needs="anom", note="%s chunk=%d" % (how, chunk_steps), args=dict(how=how))


def band_stale(src, how="array"):
    """the same call with the generation of the slab that was resident BEFORE the one that is: refused while a slab of the same shape
    and type is resident, in words that name both generations"""
    key = src[0]

    def run(trk, env):
        f = resident_flag(src)
        stale = env.stale_generation if env.stale_generation is not None else env.generation - 1
        try:
            _band_call(trk, how, key, f, None, src[1], 0, band_sectors(key), True, (_chunks_reader(f), None), resident_gen=stale, resident_f64=src[1] == "f8")
        except _state_errors() as e:
            if isinstance(e, ValueError):
                raise
            return StateError(str(e)), env.generation, stale
        return None

    def same(got, want):
        return (got is not None and got[1] != got[2] and refused_with(STATE_RC, "stale generation")(got[0], None)
                and "is generation %d," % got[1] in str(got[0]) and "stale generation %d" % got[2] in str(got[0]))
    return Op("band_resident", key, run, lambda: None, same, NO_IO, needs="anom", note="%s names a stale generation" % how, args=dict(how=how, stale_generation=True))


# ---- block-centred composite ------------------------------------------------------------------------------------------------------
CENTRED = dict(nbins=3, hy=2, hx=3)
N_STAMPS = 40


def stamp_gap(key):
    """the time steps [g0, g1) in which no stamp is kept: half of the slab, in its middle"""
    T = SHAPES[key][0]
    return T // 4, T // 4 + T // 2


@functools.lru_cache(maxsize=None)
def stamps(key, seed=0):
    """(t, row, col, bin) of N_STAMPS stamps: t sorted, bin in [-1, nbins); the rows lie in a few neighbouring rows of the grid, so the
    windows of a chunk touch a band of fewer than ny rows (the host-array form copies that band alone); the stamps inside stamp_gap
    all have bin -1, so a chunk that lies in the gap carries stamps but none that is kept"""
    T, ny, nx = SHAPES[key]
    rng = np.random.default_rng(100 + seed)
    g0, g1 = stamp_gap(key)
    outside = np.concatenate([np.arange(0, g0), np.arange(g1, T)])
    t = np.sort(np.concatenate([rng.choice(outside, N_STAMPS - 4), rng.integers(g0, g1, 4)])).astype(np.int64)
    bin = rng.integers(-1, CENTRED["nbins"], N_STAMPS).astype(np.int32)
    bin[(t >= g0) & (t < g1)] = -1
    r0, span = ny // 3, max(2, ny // 5)
    row = rng.integers(r0, r0 + span, N_STAMPS).astype(np.int32)
    col = rng.integers(0, nx, N_STAMPS).astype(np.int32)
    return tuple(_frozen(a) for a in (t, row, col, bin))


def stamps_none_kept(key, seed=0):
    """the same stamps with every bin -1: nothing is kept, nothing is read, the composite is all zeros"""
    t, row, col, bin = stamps(key, seed)
    return t, row, col, _frozen(np.full_like(bin, -1))


def carrying_chunks(key, chunk_steps, esz=4, seed=0, none_kept=False):
    """centred_stream_impl's walk restated: (chunk length, [(index of a chunk that carries a kept stamp, the rows of the band its
    windows touch), ...])"""
    T, ny, nx = SHAPES[key]
    t, row, col, bin = (stamps_none_kept if none_kept else stamps)(key, seed)
    c = _chunk(chunk_steps, T, ny * nx * esz)
    out = []
    for k in range(-(-T // c)):
        kept = (t // c == k) & (bin >= 0)
        if kept.any():
            lo, hi = int(row[kept].min()), int(row[kept].max())
            out.append((k, min(hi + CENTRED["hy"], ny - 1) - max(lo - CENTRED["hy"], 0) + 1))
    return c, out


def centred_chunk_lengths(key):
    """the chunk lengths below 20 at which a centred call has at least two carrying chunks and one chunk that carries none"""
    T = SHAPES[key][0]
    return [c for c in range(2, 20) if len(carrying_chunks(key, c)[1]) >= 2 and len(carrying_chunks(key, c)[1]) < -(-T // c)]


def centred_io(key, how, esz, chunk_steps, seed=0, none_kept=False):
    """centred_stream_impl: two buffers of chunk x (the widest band of rows of a carrying chunk, for a reader whole planes) in io_in
    and for a reader a pinned chunk; nothing at all when no stamp is kept.  The _dev entries claim nothing"""
    T, ny, nx = SHAPES[key]
    c, pieces = carrying_chunks(key, chunk_steps, esz, seed, none_kept)
    io = dict(NO_IO, chunk=c, chunks=-(-T // c), carrying=len(pieces), max_rows=max([r for _, r in pieces], default=0))
    if how != "dev" and pieces:
        one = c * (ny if how == "cb" else io["max_rows"]) * nx * esz
        io.update(io_in=2 * one, pin_in=one if how == "cb" else 0)
    return io


def same_centred(got, want):
    return got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]) and centred_util.same_bits(got[0], want[0])


def centred(key, how="array", dtype="f4", chunk_steps=0, fail_chunk=None, seed=0, none_kept=False):
    """fail_chunk counts the reader's calls, that is the carrying chunks.  The reader form also reports the reader's calls: exactly
    the carrying chunks, in order.  none_kept: every stamp is dropped -- the call claims no buffer and reads nothing"""
    assert how in ("array", "cb", "dev")
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8
    kw = dict(CENTRED)
    the_stamps = lambda: (stamps_none_kept if none_kept else stamps)(key, seed)               # noqa: E731

    def run(trk, env):
        x = wide_field(key, dtype, seed)
        t, row, col, bin = the_stamps()
        if how == "array":
            return trk.centred(x, t, row, col, bin, chunk_steps=chunk_steps, **kw)
        if how == "cb":
            calls = []
            s, n = trk.centred_cb(_chunks_reader(x, fail_chunk, calls), (T, ny, nx), DT[dtype], t, row, col, bin, chunk_steps=chunk_steps, **kw)
            return s, n, calls
        dx = trk.malloc(x.nbytes)
        try:
            trk.h2d(dx, x)
            return trk.centred_dev(dx, T, ny, nx, t, row, col, bin, f64=dtype == "f8", **kw)
        finally:
            trk.free(dx)
    fam = {"array": "centred", "cb": "centred_cb", "dev": "centred_dev"}[how]
    io = centred_io(key, how, esz, chunk_steps, seed, none_kept)
    note = "%s chunk=%d%s" % (dtype, chunk_steps, " no stamp kept" if none_kept else "")
    if fail_chunk is not None:
        assert how == "cb" and fail_chunk <= io["carrying"]
        return Op(fam, key, _catching(run, ReaderGaveUp), lambda: None, gave_up, io, note="%s: the reader gives up on carrying chunk %d" % (note, fail_chunk),
                  args=dict(fail_chunk=fail_chunk, how=how))

    def same(got, want):
        c, pieces = carrying_chunks(key, chunk_steps, esz, seed, none_kept)
        return same_centred(got, want) and (how != "cb" or got[2] == [(k * c, min(c, T - k * c)) for k, _ in pieces])
    return Op(fam, key, run, lambda: centred_util.centred(wide_field(key, dtype, seed), *the_stamps(), **kw), same, io, note=note,
              args=dict(dtype=dtype, how=how, none_kept=none_kept))


def centred_resident(src, how="array", chunk_steps=5):
    """the field is the resident anomaly slab (NaNs left out: skipna), taken by shape and type alone; one launch over all stamps"""
    key = src[0]
    T, ny, nx = SHAPES[key]
    kw = dict(CENTRED, skipna=True)

    def run(trk, env):
        t, row, col, bin = stamps(key)
        if how == "array":
            return trk.centred(None, t, row, col, bin, chunk_steps=chunk_steps, resident_f64=src[1] == "f8", shape=(T, ny, nx), **kw)
        if how == "cb":
            return trk.centred_cb(None, (T, ny, nx), DT[src[1]], t, row, col, bin, chunk_steps=chunk_steps, **kw)
        return trk.centred_dev(None, T, ny, nx, t, row, col, bin, f64=src[1] == "f8", **kw)
    return Op("centred_resident", key, run, lambda: centred_util.centred(resident_slab(src), *stamps(key), **kw), same_centred, NO_IO, needs="anom", note=how,
              args=dict(how=how))


# ---- lifecycle ------------------------------------------------------------------------------------------------------------------
def _grid_args(key):
    T, ny, nx = SHAPES[key]
    lat = np.linspace(90, -90, ny).astype(np.float32)
    lon = (np.arange(nx) * (360.0 / nx)).astype(np.float32)
    return lat, lon, ["%03d" % t for t in range(T)]


def lifecycle(key, dtype="f4", seed=1):
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        rows = trk.lifecycle(life_flag(key, seed), slab(key, dtype, seed), wrow(key))
        env.life = (rows, key, life_flag(key, seed), slab(key, dtype, seed))
        return rows, trk.lifecycle_exact(np.arange(len(rows)))
    return Op("lifecycle", key, run, lambda: want_life(life_flag(key, seed), slab(key, dtype, seed), key), same_life, array_io(key, esz, 4),
              note=dtype, args=dict(dtype=dtype))


def lifecycle_resident(src):
    key = src[0]

    def run(trk, env):
        rows = trk.lifecycle(resident_flag(src), None, wrow(key), resident_f64=src[1] == "f8")
        env.life = (rows, key, resident_flag(src), resident_slab(src))
        return rows, trk.lifecycle_exact(np.arange(len(rows)))
    return Op("lifecycle_resident", key, run, lambda: want_life(resident_flag(src), resident_slab(src), key), same_life, array_io(key, 0, 4), needs="anom")


def lifecycle_stream(key, dtype="f4", chunk_steps=0, readers=True, seed=1):
    """every row is picked: the exact records of all rows come from the chunks while they are on the device"""
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        f, x = life_flag(key, seed), slab(key, dtype, seed)
        pick = lambda rows: np.arange(len(rows))                                              # noqa: E731
        if readers:
            rows, idx, ex = trk.lifecycle_stream(_chunks_reader(f), _chunks_reader(x), wrow(key), shape=(T, ny, nx), dtype=DT[dtype], chunk_steps=chunk_steps, pick=pick)
        else:
            rows, idx, ex = trk.lifecycle_stream(f, x, wrow(key), chunk_steps=chunk_steps, pick=pick)
        env.life = None
        if not np.array_equal(idx, np.arange(len(rows))):
            return rows, None
        return rows, ex
    return Op("lifecycle_stream", key, run, lambda: want_life(life_flag(key, seed), slab(key, dtype, seed), key),
              lambda got, want: got[1] is not None and same_life(got, want), stream_io(key, chunk_steps, esz, second_bytes=4, reader=readers, reader2=readers),
              note="%s chunk=%d%s" % (dtype, chunk_steps, " readers" if readers else ""), args=dict(dtype=dtype))


def exact_rows_again():
    """lifecycle_exact over all rows of the last lifecycle op, and the frame from contrack.lifecycle_columns with the handle"""
    def run(trk, env):
        rows, key, flag, field = env.life
        from contrack_amd.contrack import lifecycle_frame
        lat, lon, dates = _grid_args(key)
        return trk.lifecycle_exact(np.arange(len(rows))), lifecycle_frame(rows, lat, lon, dates, trk), (key, flag, field)

    def same(got, want):
        from oracle import lifecycle_port
        ex, frame, (key, flag, field) = got
        lat, lon, dates = _grid_args(key)
        wex = want_life(flag, field, key)[1]
        return (all(np.array_equal(ex[k], wex[k], equal_nan=True) for k in ("area", "swv", "s", "sy", "sx"))
                and frame == lifecycle_port.run_lifecycle(flag, field, lat, lon, wrow(key), dates))
    return Op("lifecycle_exact", None, run, lambda: None, same, NO_IO, note="fresh")


def exact_rows_stale(columns=False):
    """the slabs of the last lifecycle op are gone: lifecycle_exact (columns: contrack.lifecycle_columns, which asks the handle for
    its fragile rows) raises the state error"""
    def run(trk, env):
        rows, key, flag, field = env.life
        if not columns:
            return trk.lifecycle_exact(np.arange(len(rows)))
        from contrack_amd import contrack
        lat, lon, dates = _grid_args(key)
        assert len(contrack.fragile_rows(rows)) > 0            # (rows without a fragile one would not ask the handle at all)
        return contrack.lifecycle_columns(rows, lat, lon, dates, tracker=trk)

    return Op("lifecycle_exact", None, _refusing(run), lambda: None, refused_with(STATE_RC, "overwrote or released"), NO_IO, note="stale" + (" through lifecycle_columns" if columns else ""),
              args=dict(stale=True))


# ---- level mean, anomalies ------------------------------------------------------------------------------------------------------
def level_mean(key, dtype="f4", how="array", chunk_steps=None, keep=False, fail_chunk=None, seed=4):
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8
    nsel = int(np.count_nonzero(LEVEL_W))

    def run(trk, env):
        if how == "array":
            return trk.level_mean(level_input(key, dtype, seed), LEVEL_W, chunk_steps=chunk_steps, keep_resident=keep)
        out = np.full((T, ny, nx), 7, dtype=DT[dtype])

        def sink(t0, nt, v):
            out[t0:t0 + nt] = v
        trk.level_mean_cb(_chunks_reader(level_selected(key, dtype, seed), fail_chunk), (T, nsel, ny, nx), DT[dtype], LEVEL_W[LEVEL_W != 0], sink=sink,
                          chunk_steps=chunk_steps or 0, keep_resident=keep)
        return out
    fam = "level_mean" if how == "array" else "level_mean_cb"
    io = stream_io(key, chunk_steps or 0, esz, out_bytes=0 if (keep and how == "array") else esz, reader=how == "cb", writer=how == "cb", nsel=nsel)
    gives = ("level", key, dtype, seed) if keep else None
    if fail_chunk is not None:
        return Op(fam, key, _catching(run, ReaderGaveUp), lambda: None, gave_up, io, drops=("level",), note="reader gives up on chunk %d" % fail_chunk,
                  args=dict(fail_chunk=fail_chunk))
    return Op(fam, key, run, lambda: want_level(key, dtype, seed), level_util.same_bits, io, gives=gives, drops=("level",),
              note="%s chunk=%s%s" % (dtype, chunk_steps, " keep" if keep else ""), args=dict(dtype=dtype))


def level_mean_dev(key, dtype="f4", seed=4):
    """slab and mean in the caller's device buffers: no staging buffer is claimed, a resident mean stays where it is -- under a new
    identity, as include/contrack_hip.h says of every ctk_level_mean_* call (the runner's Env follows it)"""
    T, ny, nx = SHAPES[key]

    def run(trk, env):
        x = level_input(key, dtype, seed)
        out = np.empty((T, ny, nx), dtype=DT[dtype])
        d_in, d_out = trk.malloc(x.nbytes), trk.malloc(out.nbytes)
        try:
            trk.h2d(d_in, x)
            trk.memset(d_out, 0xff, out.nbytes)
            before = trk.resident_level_mean(), trk.resident_level_mean_generation()
            trk.level_mean_dev(d_in, T, NLEV, ny, nx, LEVEL_W, d_out, f64=dtype == "f8")
            trk.d2h(out, d_out)
        finally:
            trk.free(d_in)
            trk.free(d_out)
        after = trk.resident_level_mean(), trk.resident_level_mean_generation()
        if env.level_generation is not None:
            env.level_generation = after[1]
        return out, before, after
    return Op("level_mean_dev", key, run, lambda: want_level(key, dtype, seed),
              lambda got, want: level_util.same_bits(got[0], want) and got[1][0] == got[2][0] and got[1][1] != got[2][1], NO_IO, note=dtype, args=dict(dtype=dtype))


# ---- reversal of the meridional gradient ----------------------------------------------------------------------------------------
def reversal_io(key, how, esz, chunk_steps, keep, sink=True):
    """reversal_stream_impl: ctk_stream_chunk of a whole plane; two input chunks in io_in (a reader: and a pinned chunk), two output
    chunks in io_out only without keep_resident or with a writer (then also a pinned output chunk) -- with keep_resident the kernel
    writes the resident slot and a host array is filled from there.  reversal_dev claims nothing"""
    if how == "dev":
        return NO_IO
    writer = how == "cb" and sink
    return stream_io(key, chunk_steps, esz, out_bytes=esz if (not keep or writer) else 0, reader=how == "cb", writer=writer)


def reversal(key, dtype="f4", how="array", chunk_steps=0, keep=False, mask=False, second=False, sink="array", fail_chunk=None, fail_which="reader", seed=0):
    """how: "array" (Tracker.reversal), "cb" (reversal_cb: a reader, and `sink` an "array" or a "writer"), "dev" (reversal_dev).
    fail_chunk / fail_which: the reader or the writer gives up on that call of it; with keep, nothing may be resident afterwards.
    A call without keep leaves the resident slot alone: it neither gives nor drops"""
    assert how in ("array", "cb", "dev") and sink in ("array", "writer") and fail_which in ("reader", "writer") and not (how == "dev" and keep)
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        z, tab = rev_input(key, dtype, seed), rev_table(key, second)
        if how == "array":
            return trk.reversal(z, tab, mask=mask, chunk_steps=chunk_steps, keep_resident=keep)
        if how == "dev":
            out = np.empty_like(z)
            d_in, d_out = trk.malloc(z.nbytes), trk.malloc(z.nbytes)
            try:
                trk.h2d(d_in, z)
                trk.memset(d_out, 0xff, z.nbytes)
                gen = trk.resident_generation()
                trk.reversal_dev(d_in, T, ny, nx, tab, d_out, mask=mask, f64=dtype == "f8")
                trk.d2h(out, d_out)
                return out if trk.resident_generation() == gen else None
            finally:
                trk.free(d_in)
                trk.free(d_out)
        out = np.full((T, ny, nx), 7, dtype=DT[dtype])
        count = [0]

        def writer(t0, nt, v):
            count[0] += 1
            if fail_which == "writer" and count[0] == fail_chunk:
                raise ReaderGaveUp("the writer, chunk %d" % count[0])
            out[t0:t0 + nt] = v
        reader = _chunks_reader(z, fail_chunk if fail_which == "reader" else None)
        try:
            trk.reversal_cb(reader, (T, ny, nx), DT[dtype], tab, mask=mask, sink=out if sink == "array" and fail_chunk is None else writer, chunk_steps=chunk_steps,
                            keep_resident=keep)
        except ReaderGaveUp as e:
            return e if trk.resident_anom() is None or not keep else None          # (with keep: nothing is left resident)
        return out
    fam = {"array": "reversal", "cb": "reversal_cb", "dev": "reversal_dev"}[how]
    io = reversal_io(key, how, esz, chunk_steps, keep)
    note = "%s chunk=%d%s%s%s" % (dtype, chunk_steps, " keep" if keep else "", " mask" if mask else "", " ghgs2" if second else "") + (" " + sink if how == "cb" else "")
    if fail_chunk is not None:
        assert how == "cb"
        return Op(fam, key, run, lambda: None, gave_up, io, drops=("anom",) if keep else (), note="%s: the %s gives up on chunk %d" % (note, fail_which, fail_chunk),
                  args=dict(fail_chunk=fail_chunk, fail_which=fail_which, how=how, keep=keep))
    return Op(fam, key, run, lambda: want_reversal(key, dtype, seed, mask, second), lambda got, want: got is not None and reversal_util.same_bits(got, want), io,
              gives=("anom", key, dtype, seed, ("reversal", mask, second)) if keep else None, drops=("anom",) if keep else (), note=note,
              args=dict(dtype=dtype, how=how, keep=keep, mask=mask, second=second, sink=sink))


def climatology(key, dtype="f4", segments=False, seed=3):
    """a climatology-only call on a host slab (want_anom=False): it writes io_in and an_raw, and leaves a resident anomaly slab alone"""
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        a, c = trk.anomalies(anom_input(key, dtype, seed), anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], want_anom=False, want_clim=True,
                             segments=segment_starts(key) if segments else None)
        return c if a is None else None
    return Op("climatology", key, run, lambda: want_anom(key, dtype, seed)[1], same_values, array_io(key, esz), note=dtype + (" segments" if segments else ""),
              args=dict(dtype=dtype))


def climatology_resident(src):
    """the climatology of the resident vertical mean alone: no handle buffer that a slab lives in is written"""
    _, key, dtype, seed = src

    def run(trk, env):
        a, c = trk.anomalies_resident(anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], want_anom=False, want_clim=True)
        return c if a is None else None
    return Op("climatology_resident", key, run, lambda: want_anom_of_level(key, dtype, seed)[1], same_values, NO_IO, needs="level")


def anomalies(key, dtype="f4", keep=False, segments=False, seed=3):
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        return trk.anomalies(anom_input(key, dtype, seed), anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], want_clim=True, keep_resident=keep,
                             segments=segment_starts(key) if segments else None)
    return Op("anomalies", key, run, lambda: want_anom(key, dtype, seed, segments), same_values, array_io(key, esz), gives=("anom", key, dtype, seed, segments) if keep else None,
              drops=("anom",), note="%s%s%s" % (dtype, " keep" if keep else "", " segments" if segments else ""), args=dict(dtype=dtype))


def anomalies_stream(key, dtype="f4", chunk_steps=0, callbacks=True, seed=3):
    T, ny, nx = SHAPES[key]
    esz = 4 if dtype == "f4" else 8

    def run(trk, env):
        x = anom_input(key, dtype, seed)
        if not callbacks:
            return trk.anomalies_stream(x, anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], chunk_steps=chunk_steps, want_clim=True)
        out = np.full((T, ny, nx), 7, dtype=DT[dtype])

        def sink(t0, nt, v):
            out[t0:t0 + nt] = v
        _, clim = trk.anomalies_stream(_chunks_reader(x), anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], sink=sink, shape=(T, ny, nx), dtype=DT[dtype],
                                       chunk_steps=chunk_steps, want_clim=True)
        return out, clim
    h = ANOM["smooth"] - 1
    return Op("anomalies_stream", key, run, lambda: want_anom(key, dtype, seed), same_values,
              stream_io(key, chunk_steps, esz, out_bytes=esz, reader=callbacks, writer=callbacks, halo_in=h, halo_out=h + 1),
              note="%s chunk=%d%s" % (dtype, chunk_steps, " reader+sink" if callbacks else ""), args=dict(dtype=dtype))


def anomalies_resident(src):
    """anomalies of the resident vertical mean"""
    _, key, dtype, seed = src

    def run(trk, env):
        return trk.anomalies_resident(anom_groups(key), ANOM["G"], ANOM["window"], ANOM["smooth"], want_clim=True)
    return Op("anomalies_resident", key, run, lambda: want_anom_of_level(key, dtype, seed), same_values, NO_IO, needs="level", drops=("anom",))


# ---- percentile and standard-deviation thresholds -------------------------------------------------------------------------------
def _percentile(trk, env, x, key, q):
    y0, y1 = band_rows(key)
    mean = trk.percentile(x, y0, y1, q)
    return mean, trk.debug_percentile_values((y1 - y0) * SHAPES[key][2])


def band_mean(values):
    """k_nanmean restated (csrc/ctk_anom.hip; tests/test_gpu_anom_exact.py words it): thread i of 1024 adds every 1024th value from
    i on, in order, NaNs left out; the 1024 partial sums are folded ss[i] += ss[i + d] for d = 512, 256, ..., 1; the sum is divided
    by the count of values (NaN for none)"""
    v = np.asarray(values, dtype=np.float64)
    pad = np.full(-(-max(len(v), 1) // 1024) * 1024, np.nan)
    pad[:len(v)] = v
    rows = pad.reshape(-1, 1024)
    ok = ~np.isnan(rows)
    ss = np.zeros(1024)
    with np.errstate(invalid="ignore"):
        for r, k in zip(rows, ok):
            ss = np.where(k, ss + np.where(k, r, 0.0), ss)
        d = 512
        while d:
            ss[:d] = ss[:d] + ss[d:2 * d]
            d //= 2
        n = int(ok.sum())
        return ss[0] / n if n else np.nan


def same_percentile(got, want):
    """the per-grid-point quantiles are numpy's, the band mean is band_mean of them, bit for bit"""
    return np.array_equal(got[1], want, equal_nan=True) and np.array_equal(np.float64(got[0]), np.float64(band_mean(want)), equal_nan=True)


def percentile(key, dtype="f4", q=0.9, seed=3):
    esz = 4 if dtype == "f4" else 8
    return Op("percentile", key, lambda trk, env: _percentile(trk, env, anom_input(key, dtype, seed), key, q),
              lambda: want_quantile_values(anom_input(key, dtype, seed), key, q), same_percentile, array_io(key, esz), note=dtype, args=dict(dtype=dtype))


def percentile_resident(src, q=0.9):
    key = src[0]

    return Op("percentile_resident", key, lambda trk, env: _percentile(trk, env, None, key, q), lambda: want_quantile_values(resident_slab(src), key, q),
              same_percentile, NO_IO, needs="anom")


def percentile_groups(key, dtype="f4", q=0.9, window=3, seed=3):
    def run(trk, env):
        return trk.percentile_groups(anom_input(key, dtype, seed), *band_rows(key), anom_groups(key), ANOM["G"], q, window)
    return Op("percentile_groups", key, run, lambda: pctl_util.want(anom_input(key, dtype, seed), band_rows(key), anom_groups(key), ANOM["G"], window, q), same_bits64,
              array_io(key, 4 if dtype == "f4" else 8), note=dtype, args=dict(dtype=dtype))


def percentile_field(key, dtype="f4", q=0.9, window=3, seed=3):
    def run(trk, env):
        return trk.percentile_field(anom_input(key, dtype, seed), *band_rows(key), anom_groups(key), ANOM["G"], q, window)
    return Op("percentile_field", key, run, lambda: pfield_util.want_field(anom_input(key, dtype, seed), band_rows(key), anom_groups(key), ANOM["G"], window, q),
              same_bits64, array_io(key, 4 if dtype == "f4" else 8), note=dtype, args=dict(dtype=dtype))


def std_field(key, dtype="f4", window=3, ddof=1, seed=3):
    def run(trk, env):
        return trk.std_field(anom_input(key, dtype, seed), *band_rows(key), anom_groups(key), ANOM["G"], window, ddof, True, want_mean=True, want_n=True)
    return Op("std_field", key, run, lambda: std_util.want_std(anom_input(key, dtype, seed), band_rows(key), anom_groups(key), ANOM["G"], window, ddof, True), same_std,
              array_io(key, 4 if dtype == "f4" else 8), note=dtype, args=dict(dtype=dtype))


# ---- the handle's own state -----------------------------------------------------------------------------------------------------
def release_io():
    return Op("release_io", None, lambda trk, env: trk.release_io(), lambda: None, nothing, NO_IO, drops=("anom", "level"))


def set_sticky(key):
    """segments and a threshold field set on the handle and left there"""
    def run(trk, env):
        trk.set_segments(segment_starts(key))
        trk.set_threshold_field(*threshold_planes(key))
    return Op("set_sticky", key, run, lambda: None, nothing)


def clear_sticky():
    def run(trk, env):
        trk.clear_segments()
        trk.clear_threshold_field()
    return Op("clear_sticky", None, run, lambda: None, nothing)


def generation_unchanged(src):
    """resident_generation is what the producer left (the runner records it after every op that gives a slab)"""
    return Op("resident_generation", src[0], lambda trk, env: (trk.resident_generation(), env.generation, trk.resident_anom()),
              lambda: (SHAPES[src[0]] + (src[1] == "f8",)), lambda got, want: got[0] == got[1] and got[2] == want, NO_IO, needs="anom")


def level_generation_unchanged(src):
    return Op("resident_level_generation", src[1], lambda trk, env: (trk.resident_level_mean_generation(), env.level_generation, trk.resident_level_mean()),
              lambda: (SHAPES[src[1]] + (src[2] == "f8",)), lambda got, want: got[0] == got[1] and got[2] == want, NO_IO, needs="level")


REFUSALS = {                           # what every consumer says when its slab is not resident, and who says it
    "track_resident": ("no anomaly slab is resident",),                               # Tracker.track_resident, before the library is asked
    "percentile_resident": ("no anomaly slab is resident",),                          # Tracker._slab_or_resident
    "anomalies_resident": ("no vertical mean is resident",),                          # Tracker.anomalies_resident
    "climatology_resident": ("no vertical mean is resident",),
    "lifecycle_resident": (STATE_RC, "needs a resident anomaly slab"),                # ctk_lifecycle_*: CTK_E_STATE
    "composite_resident": (STATE_RC, "needs a resident anomaly slab"),                # ctk_composite_*: CTK_E_STATE
    "band_resident": (STATE_RC, "none of this shape and type is resident"),           # ctk_band_*: CTK_E_STATE (band_resident, before the generation)
    "centred_resident": (STATE_RC, "needs a resident anomaly slab"),                  # ctk_centred_*: CTK_E_STATE (comp_resident)
}


def refuses(op):
    """the same call, which must now be refused in its own words"""
    return Op(op.family, op.key, _refusing(op.run), lambda: None, refused_with(*REFUSALS[op.family]), NO_IO, note=(op.note + ": must refuse").lstrip(": "), args=dict(op.args, refuse=True))


# ---- the written sequences ------------------------------------------------------------------------------------------------------
S, O, L = "mult4", "odd", "large"


def io_grows_and_shrinks():
    """array entries of different families: small frequency, large track, small level mean, larger anomalies, small spells, large
    composite, small lifecycle; among them a band with a float64 field and a centred composite, and a band that asks for the sector
    tables alone (its column tables stay in the handle: bd_cols, sized by its T steps) after a larger one that asked for both"""
    return [frequency(S), centred(S), track(L), level_mean(S), band(L, field="f8"), anomalies(O, "f8"), band(O, columns=False), spells(S), composite(L, dtype="f8"),
            lifecycle(S)]


def pinned_chunks_up_and_down():
    """the reader and writer entries with chunk bytes rising and then falling, across the families"""
    return [frequency(S, "cb", chunk_steps=5), centred(S, "cb", "f4", chunk_steps=3), composite(O, "cb", chunk_steps=9), band(O, "cb", "f8", chunk_steps=12),
            lifecycle_stream(L, "f8", chunk_steps=13, readers=True), centred(L, "cb", "f8", chunk_steps=7), level_mean(L, "f8", "cb", chunk_steps=16),
            band(L, "cb", chunk_steps=21), track_stream(L, "f4", chunk_steps=11, callbacks=True), anomalies_stream(O, "f4", chunk_steps=8, callbacks=True),
            centred(O, "cb", "f4", chunk_steps=4), spells(S, "cb", chunk_steps=3)]


def _resident_consumers(src):
    return ([track_resident(src), lifecycle_resident(src), composite_resident(src), percentile_resident(src)]
            + [band_resident(src, how, chunk_steps=7 if how != "dev" else 0) for how in ("array", "cb", "dev")] + [centred_resident(src, how) for how in ("array", "cb", "dev")])


def resident_anomaly_survives():
    src = (S, "f4", 3, False)
    between = [frequency(L), spells(O), level_mean(O), percentile(L), percentile_groups(L), percentile_field(O), std_field(L), track(L), lifecycle(O),
               band(L, field="f4", chunk_steps=16), centred(L, "array", "f8", chunk_steps=7), centred(O, "cb", chunk_steps=4)]
    # climatology-only calls on slabs LARGER than the resident one, from the host and from a resident vertical mean: the anomaly slot is not theirs
    clim_only = [climatology(L, "f8"), climatology(L, "f4", segments=True), level_mean(L, "f8", keep=True), climatology_resident(("level", L, "f8", 4))]
    return [anomalies(S, "f4", keep=True)] + between + clim_only + [generation_unchanged(src)] + _resident_consumers(src)


def resident_level_mean_survives():
    src = ("level", S, "f8", 4)
    between = [anomalies(L, "f8"), track(L), track_stream(O, chunk_steps=7, callbacks=True), anomalies_stream(L, chunk_steps=20), frequency(L, "cb", chunk_steps=10)]
    return [level_mean(S, "f8", keep=True)] + between + [level_generation_unchanged(src), anomalies_resident(src)]


def invalidated_residents_refuse():
    a, lv = (S, "f4", 3, False), ("level", S, "f4", 4)
    every = lambda: [refuses(op) for op in _resident_consumers(a) + [anomalies_resident(lv), climatology_resident(lv)]]                # noqa: E731
    seq = ([anomalies(S, "f4", keep=True), level_mean(S, "f4", keep=True), release_io()] + every() + [track(S)]
           + [anomalies(S, "f4", keep=True), level_mean(S, "f4", keep=True), anomalies(O), level_mean(O)] + every() + [frequency(O)])
    # a slab of the same shape and type but with other values takes the place of the first: only its generation tells them apart
    b = (S, "f4", 5, False)
    return seq + [anomalies(S, "f4", keep=True, seed=3), anomalies(S, "f4", keep=True, seed=5)] + [band_stale(b, how) for how in ("array", "cb", "dev")] + [
        band_resident(b, "array", chunk_steps=7), band_resident(b, "dev"), centred_resident(b, "array"), centred_resident(b, "dev")]


def tracking_caches(key=O):
    other = L if key != L else S
    return [track(key, thr=100.0, wvar=1, gorl=">="), composite(other, dtype="f8"), track(key, thr=130.0), track(key, thr=130.0, wvar=2),
            track(key, thr=130.0, wvar=2, gorl="<"), track(key, "f8", thr=130.0, wvar=2, gorl="<"), track(key, "f8", thr=130.0, wvar=2, gorl="<", per_step=True),
            track_field(key), track(key), track_segments(key), track(key), track_dev(key)]


def sticky_settings_do_not_leak(key=S):
    return [set_sticky(key), frequency(key), spells(key, segments=True), anomalies(key, segments=True), composite(key), band(key, field="f4", chunk_steps=9),
            centred(key, chunk_steps=3), lifecycle(key), clear_sticky(), track(key)]


def a_failed_stream_then_others():
    T = SHAPES[L][0]
    c = -(-T // 5)                                        # five chunks
    seq = [frequency(L, "cb", chunk_steps=c, fail_chunk=3), spells(S, "cb", chunk_steps=4), composite(S),
           level_mean(L, "f4", "cb", chunk_steps=c, fail_chunk=3), frequency(O, "cb", chunk_steps=6), track(O),
           track_stream(L, "f4", chunk_steps=c, callbacks=True, fail_chunk=3), anomalies_stream(S, chunk_steps=5), lifecycle(S)]
    # a band reader that gives up on chunk 3 of 5: the tables of chunks 1 and 2 are queued for the pinned twins and never land; the
    # next streamed band call, on another shape, uses the twins and both table sets at once
    for which in ("flag", "field"):
        seq += [band(L, "cb", "f4", chunk_steps=c, fail_chunk=3, fail_which=which), band(O, "cb", "f8", chunk_steps=8), composite(S)]
    # a centred reader that gives up on its third carrying chunk: two chunks are in flight on the tracker's buffers and events
    seq += [centred(L, "cb", "f4", chunk_steps=7, fail_chunk=3), track_stream(O, "f4", chunk_steps=9, callbacks=True), centred(L, "cb", "f4", chunk_steps=7)]
    # ... and a centred reader call directly after another family's failed stream
    seq += [frequency(L, "cb", chunk_steps=c, fail_chunk=3), centred(O, "cb", "f8", chunk_steps=4), lifecycle(S)]
    # a reversal that was to leave its result resident and whose reader gives up on chunk 3 of 5 (the kernel has written two chunks
    # into the resident slot): nothing is resident, every consumer refuses; then one whose writer gives up on its second chunk while
    # a resident slab of the other producer is there (it is left alone: the call keeps nothing); the next streamed reversal is right
    a, r = (S, "f4", 3, False), (L, "f4", 0, ("reversal", False, False))
    seq += [anomalies(S, "f4", keep=True), reversal(L, "f4", "cb", chunk_steps=c, keep=True, fail_chunk=3), refuses(track_resident(r)), refuses(band_resident(r, "dev")),
            spells(O, "cb", chunk_steps=6), track(O)]
    seq += [anomalies(S, "f4", keep=True), reversal(L, "f4", "cb", chunk_steps=c, fail_chunk=2, fail_which="writer"), track_resident(a),
            reversal(O, "f8", "cb", chunk_steps=8, second=True, sink="writer"), composite(S)]
    return seq


def exact_rows_follow_their_slabs():
    src = (S, "f4", 3, False)
    seq = [lifecycle(O), exact_rows_again(), frequency(L, "dev"), spells(L, "dev"), composite(L, "dev"), exact_rows_again()]
    for breaker in (frequency(S), track(S), level_mean(S), anomalies(L), percentile_field(S), release_io()):
        seq += [breaker, exact_rows_stale(), exact_rows_stale(columns=True), lifecycle(O), exact_rows_again()]
    # band and centred: the streamed forms claim the staging buffers (also a band on the resident slab: its flags travel), the _dev
    # forms, a centred composite of the resident slab and a centred call none of whose stamps is kept (it skips stream_setup) claim
    # nothing -- Op.breaks_exact says which, and the rows follow it
    # (first a call that makes io_in and io_out larger than anything this leg asks of them: no buffer moves under the rows here, so
    # a library that forgot to make them stale would answer with wrong records, which is what the sequence reports)
    seq += [anomalies(S, "f4", keep=True), composite(L, dtype="f8"), lifecycle(O), exact_rows_again()]
    for op in (band(S), band(L, "dev", "f4"), band_resident(src, "array", chunk_steps=7), centred(L, "dev", "f8"), centred(S), centred_resident(src, "dev"),
               centred(S, "cb", chunk_steps=3), band_resident(src, "dev"), centred_resident(src, "array"), band_resident(src, "cb", chunk_steps=7),
               centred(L, "array", "f8", chunk_steps=7, none_kept=True), centred(L, "cb", chunk_steps=7, none_kept=True)):
        seq += [op, exact_rows_stale(), exact_rows_stale(columns=True), lifecycle(O), exact_rows_again()] if op.breaks_exact else [op, exact_rows_again()]
    # field = None: the field is the resident anomaly slab, which any anomaly call writes or drops
    seq += [anomalies(S, "f4", keep=True), lifecycle_resident(src), exact_rows_again(), anomalies_stream(S, chunk_steps=5, callbacks=False), exact_rows_stale(),
            lifecycle_resident(src), exact_rows_again(), anomalies(S, "f4", keep=True), exact_rows_stale(), lifecycle_resident(src), exact_rows_again()]
    # ... also one that writes no staging buffer: the anomalies of a resident vertical mean go from the mean's slot to the anomaly slot, so only the
    # generation of the resident anomaly slab tells.  The climatology of that (larger) mean alone writes neither: the rows stay right
    lv = ("level", L, "f4", 4)
    seq += [level_mean(L, "f4", keep=True), anomalies(S, "f4", keep=True), lifecycle_resident(src), exact_rows_again(),
            climatology_resident(lv), exact_rows_again(), anomalies_resident(lv), exact_rows_stale(), exact_rows_stale(columns=True),
            anomalies(S, "f4", keep=True), lifecycle_resident(src), exact_rows_again()]
    return seq


def _reversal_consumers(src):
    return ([track_resident(src), percentile_resident(src)] + [band_resident(src, how, chunk_steps=7 if how != "dev" else 0) for how in ("array", "cb", "dev")]
            + [centred_resident(src, how) for how in ("array", "cb", "dev")])


def reversal_between_the_others():
    """the second producer of the resident slab among the first one's calls: a reversal that keeps nothing leaves the anomaly slab and
    its generation alone (on a larger shape, so io_in and io_out grow under it); one that keeps replaces it, and the consumers then
    work on the reversal's output; the anomalies of a resident vertical mean replace that in turn; two reversals of one shape and
    type are told apart by their generation alone"""
    a = (S, "f4", 3, False)
    r = (O, "f4", 0, ("reversal", False, True))
    lv = ("level", L, "f4", 4)
    seq = [anomalies(S, "f4", keep=True),
           reversal(L, "f8", chunk_steps=16), reversal(L, "f4", "dev", mask=True), generation_unchanged(a), track_resident(a), band_resident(a, "dev"), centred_resident(a, "array"),
           reversal(O, "f4", chunk_steps=7, keep=True, second=True), generation_unchanged(r)] + _reversal_consumers(r) + [lifecycle_resident(r), composite_resident(r)]
    seq += [level_mean(L, "f4", keep=True), level_mean_dev(S, "f8"), level_generation_unchanged(lv), anomalies_resident(lv)]
    seq += [refuses(op) for op in _reversal_consumers(r)]
    # a reader and a writer, float64, the mask, on the large shape; then the slab of another seed takes its place
    m = (L, "f8", 0, ("reversal", True, False))
    seq += [reversal(L, "f8", "cb", chunk_steps=13, keep=True, mask=True, sink="writer"), generation_unchanged(m), track_resident(m), percentile_resident(m), centred_resident(m, "dev")]
    b = (O, "f4", 1, ("reversal", False, True))
    seq += [reversal(O, "f4", keep=True, second=True), reversal(O, "f4", keep=True, second=True, seed=1), band_stale(b, "array"), band_stale(b, "dev"),
            band_resident(b, "array", chunk_steps=7), track_resident(b)]
    return seq


WRITTEN = [io_grows_and_shrinks, pinned_chunks_up_and_down, resident_anomaly_survives, resident_level_mean_survives, invalidated_residents_refuse,
           tracking_caches, sticky_settings_do_not_leak, a_failed_stream_then_others, exact_rows_follow_their_slabs, reversal_between_the_others]


# ---- the seeded sequences -------------------------------------------------------------------------------------------------------
N_SEEDS, N_OPS = 26, 10                # 26 sequences: every one of the 44 families is drawn three times or more (a consumer drawn last is skipped)


def _vocabulary():
    """family -> builder(rng, state): every family of the module; a consumer's builder is called only with its slab resident"""
    pick = lambda rng, seq: seq[int(rng.integers(len(seq)))]                                   # noqa: E731
    key = lambda rng: pick(rng, (S, O, L))                                                    # noqa: E731
    dt = lambda rng: pick(rng, ("f4", "f8"))                                                  # noqa: E731
    chunk = lambda rng: int(rng.integers(2, 20))                                              # noqa: E731
    tables = ((True, True), (True, False), (False, True))                                     # (sectors, columns) of a band call
    return {
        "track": lambda r, s: track(key(r), dt(r), thr=pick(r, (100.0, 130.0)), wvar=pick(r, (1, 2)), per_step=bool(r.integers(2))),
        "track_field": lambda r, s: track_field(key(r), dt(r)),
        "track_segments": lambda r, s: track_segments(key(r)),
        "track_stream": lambda r, s: track_stream(key(r), dt(r), chunk(r), callbacks=bool(r.integers(2))),
        "track_dev": lambda r, s: track_dev(key(r), dt(r)),
        "track_resident": lambda r, s: track_resident(s["anom"]),
        "frequency": lambda r, s: frequency(key(r), "array", pick(r, (0, chunk(r))), G=pick(r, (1, 3))),
        "frequency_cb": lambda r, s: frequency(key(r), "cb", chunk(r)),
        "frequency_dev": lambda r, s: frequency(key(r), "dev"),
        "spells": lambda r, s: spells(key(r), "array", pick(r, (0, chunk(r))), by_id=bool(r.integers(2)), segments=bool(r.integers(2))),
        "spells_cb": lambda r, s: spells(key(r), "cb", chunk(r)),
        "spells_dev": lambda r, s: spells(key(r), "dev"),
        "composite": lambda r, s: composite(key(r), "array", dt(r), pick(r, (0, chunk(r)))),
        "composite_cb": lambda r, s: composite(key(r), "cb", dt(r), chunk(r)),
        "composite_dev": lambda r, s: composite(key(r), "dev", dt(r)),
        "composite_resident": lambda r, s: composite_resident(s["anom"]),
        "band": lambda r, s: band(key(r), "array", pick(r, (None, "f4", "f8")), pick(r, (0, chunk(r))), *pick(r, tables)),
        "band_cb": lambda r, s: band(key(r), "cb", pick(r, (None, "f4", "f8")), chunk(r), *pick(r, tables)),
        "band_dev": lambda r, s: band(key(r), "dev", pick(r, (None, "f4", "f8")), 0, *pick(r, tables)),
        "band_resident": lambda r, s: band_resident(s["anom"], *pick(r, (("array", 0), ("array", chunk(r)), ("cb", chunk(r)), ("dev", 0)))),
        "centred": lambda r, s: (lambda k: centred(k, "array", dt(r), pick(r, [0] + centred_chunk_lengths(k))))(key(r)),
        "centred_cb": lambda r, s: (lambda k: centred(k, "cb", dt(r), pick(r, centred_chunk_lengths(k))))(key(r)),
        "centred_dev": lambda r, s: centred(key(r), "dev", dt(r)),
        "centred_resident": lambda r, s: centred_resident(s["anom"], pick(r, ("array", "cb", "dev"))),
        "lifecycle": lambda r, s: lifecycle(key(r), dt(r)),
        "lifecycle_stream": lambda r, s: lifecycle_stream(key(r), dt(r), chunk(r), readers=bool(r.integers(2))),
        "lifecycle_resident": lambda r, s: lifecycle_resident(s["anom"]),
        "level_mean": lambda r, s: level_mean(key(r), dt(r), "array", pick(r, (None, chunk(r))), keep=bool(r.integers(2))),
        "level_mean_cb": lambda r, s: level_mean(key(r), dt(r), "cb", chunk(r), keep=bool(r.integers(2))),
        "level_mean_dev": lambda r, s: level_mean_dev(key(r), dt(r)),
        "reversal": lambda r, s: reversal(key(r), dt(r), "array", pick(r, (0, chunk(r))), keep=bool(r.integers(2)), mask=bool(r.integers(2)), second=bool(r.integers(2))),
        "reversal_cb": lambda r, s: reversal(key(r), dt(r), "cb", chunk(r), keep=bool(r.integers(2)), mask=bool(r.integers(2)), second=bool(r.integers(2)),
                                             sink=pick(r, ("array", "writer"))),
        "reversal_dev": lambda r, s: reversal(key(r), dt(r), "dev", mask=bool(r.integers(2)), second=bool(r.integers(2))),
        "anomalies": lambda r, s: anomalies(key(r), dt(r), keep=bool(r.integers(2)), segments=bool(r.integers(2))),
        "climatology": lambda r, s: climatology(key(r), dt(r), segments=bool(r.integers(2))),
        "climatology_resident": lambda r, s: climatology_resident(s["level"]),
        "anomalies_stream": lambda r, s: anomalies_stream(key(r), dt(r), chunk(r), callbacks=bool(r.integers(2))),
        "anomalies_resident": lambda r, s: anomalies_resident(s["level"]),
        "percentile": lambda r, s: percentile(key(r), dt(r)),
        "percentile_resident": lambda r, s: percentile_resident(s["anom"]),
        "percentile_groups": lambda r, s: percentile_groups(key(r), dt(r)),
        "percentile_field": lambda r, s: percentile_field(key(r), dt(r)),
        "std_field": lambda r, s: std_field(key(r), dt(r)),
        "release_io": lambda r, s: release_io(),
    }


CONSUMERS = {"track_resident": "anom", "composite_resident": "anom", "lifecycle_resident": "anom", "percentile_resident": "anom", "band_resident": "anom",
             "centred_resident": "anom", "anomalies_resident": "level", "climatology_resident": "level"}
FAMILIES = sorted(_vocabulary())


def apply_residency(state, op):
    """the model of the resident slabs: what is resident after `op`"""
    for d in op.drops:
        state[d] = None
    if op.gives is not None:
        state[op.gives[0]] = op.gives[1:] if op.gives[0] == "anom" else op.gives


def seeded(seed):
    """N_OPS operations drawn from the whole vocabulary: the families come off a deck that is reshuffled when it runs out (so that the
    N_SEEDS sequences cover every family), the arguments from the seed's generator.  A consumer whose slab is not resident is preceded
    by its producer."""
    vocab = _vocabulary()
    deck_rng = np.random.default_rng(99)
    deck = []
    while len(deck) < (N_SEEDS + 1) * N_OPS:
        deck += [FAMILIES[i] for i in deck_rng.permutation(len(FAMILIES))]
    rng = np.random.default_rng(7000 + seed)
    state = {"anom": None, "level": None}
    ops, at = [], seed * N_OPS
    while len(ops) < N_OPS:
        fam = deck[at]
        at += 1
        need = CONSUMERS.get(fam)
        if need and state[need] is None:
            if len(ops) + 2 > N_OPS:
                continue
            k = (S, O, L)[int(rng.integers(3))]
            d = ("f4", "f8")[int(rng.integers(2))]
            if need == "level":
                producer = level_mean(k, d, keep=True)
            elif rng.integers(2):                                  # either producer of the resident slab
                producer = reversal(k, d, chunk_steps=int(rng.integers(0, 20)), keep=True, mask=bool(rng.integers(2)), second=bool(rng.integers(2)))
            else:
                producer = anomalies(k, d, keep=True)
            ops.append(producer)
            apply_residency(state, producer)
        op = vocab[fam](rng, state)
        ops.append(op)
        apply_residency(state, op)
    return ops


# ---- running a sequence ---------------------------------------------------------------------------------------------------------
def grown(cap, need, buf):
    """the capacity of a shared buffer after a call that asks `need` bytes of it (0: the call does not touch it).  All four are
    grow-only until ctk_release_io.  io_in / io_out go through claim_io -> ensure (csrc/ctk_api.hip): a buffer that holds the bytes
    stays; one that does not is released and allocated anew with head room, need + need / 8 + 256 bytes.  The pinned pairs
    (PinPair::grow, csrc/ctk_own.h) get exactly the bytes asked for."""
    if need <= cap:
        return cap
    return need + need // 8 + 256 if buf.startswith("io_") else need


def check_io(cap, op, got, raised=False):
    """`cap`: the model's capacities before `op`; `got`: Tracker.debug_io_bytes() after it.  The mismatches as (buffer, got, model);
    `cap` becomes the capacities after the call.  Where the request depends on the data (Op.io_upto) or the call gave up on the way
    (`raised`: it may have claimed its buffers before), the model is a range and the handle's own figure inside it is taken over."""
    bad = []
    for buf in BUFFERS:
        if op.family == "release_io":
            lo = hi = 0
        else:
            hi = grown(cap[buf], max(op.io[buf], op.io_upto.get(buf, 0)), buf)
            lo = cap[buf] if raised else grown(cap[buf], op.io[buf], buf)
        if not lo <= got[buf] <= hi or got[buf] < op.io[buf] * (not raised):
            bad.append((buf, got[buf], lo if lo == hi else (lo, hi)))
        cap[buf] = got[buf]
    return bad


def run_sequence(trk, ops, env=None, wants=None, on_op=None):
    """every operation in order on `trk`, each compared with its reference: the list of failures (empty: all right) as
    (position, op, what).  After every tracking operation the handle's ambiguous_decisions must be 0.  After every operation the
    capacities of the shared buffers (Tracker.debug_io_bytes) are what Op.io says the handle asked for, from the capacities the
    sequence found: (position, op, "io model", buffer, got, model) otherwise.
    wants: the references, one per operation, computed beforehand (tests/concurrent_util.py: in one thread, before several handles
    run at once) instead of op.want().  on_op(position, op, t_start, t_end): called after every operation with time.perf_counter()
    directly before and after op.run."""
    env = env or Env()
    bad = []
    cap = trk.debug_io_bytes()
    for i, op in enumerate(ops):
        t_start = time.perf_counter()
        got = op.run(trk, env)
        t_end = time.perf_counter()
        if on_op is not None:
            on_op(i, op, t_start, t_end)
        if op.gives is not None:
            if op.gives[0] == "anom":
                env.stale_generation, env.generation = env.generation, trk.resident_generation()
            else:
                env.level_generation = trk.resident_level_mean_generation()
        if not op.same(got, op.want() if wants is None else wants[i]):
            bad.append((i, repr(op), "differs from its reference", getattr(op.same, "detail", "")))
        if op.tracking and trk.stats()["ambiguous_decisions"] != 0:
            bad.append((i, repr(op), "ambiguous_decisions = %d" % trk.stats()["ambiguous_decisions"]))
        bad += [(i, repr(op), "io model") + m for m in check_io(cap, op, trk.debug_io_bytes(), raised=isinstance(got, ReaderGaveUp))]
    return bad
