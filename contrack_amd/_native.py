"""ctypes binding of libcontrack_hip.so.  No torch, no other HIP binding.  Signatures, structs, callback types and return codes are
read from include/contrack_hip.h and include/contrack_hip_debug.h when the module is imported (_abi.py); none is restated here.

The library is the product's only compute path: if it is missing or no GPU is visible the calls raise
-- there is no CPU fallback (the CPU restatement lives in oracle/ and is test infrastructure).
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTK_LIB", os.path.join(_HERE, "libcontrack_hip.so"))
INCLUDE_DIR = os.environ.get("CTK_INCLUDE", os.path.join(os.path.dirname(_HERE), "include"))
_lib = None

CMP_OPS = {">=": 0, "ge": 0, "<=": 1, "le": 1, ">": 2, "gt": 2, "<": 3, "lt": 3}
GORL_ERRMSG = ' Please select from [>, >=, <, >=] for gorl'      # contrack.py:658

TIMER_NAMES = ["k_threshold", "k_scan", "k_label2d", "k_overlap", "k_extent", "k_run_values", "k_relabel",
               "k_resolve", "k_resolve_final", "k_count", "host_seam_driver", "d2h", "h2d", "total"]


class ContrackHipError(RuntimeError):
    pass


def _headers():
    """the text of the C headers, which state the ABI once: what the library is compiled against and what this binding is made from"""
    try:
        return "\n".join(open(os.path.join(INCLUDE_DIR, h)).read() for h in _abi.HEADERS)
    except OSError as e:
        raise ContrackHipError("the C headers %s not found in %s (%s) -- they belong to the source tree next to the package; CTK_INCLUDE "
                               "names another directory, as CTK_LIB names another library" % (", ".join(_abi.HEADERS), INCLUDE_DIR, e)) from None


ABI = _abi.parse(_headers())
EXPORTS = list(ABI.functions)
CTK_E_INVALID, CTK_E_NOMEM, CTK_E_RANGE, CTK_E_COMM = (ABI.constants[k] for k in ("CTK_E_INVALID", "CTK_E_NOMEM", "CTK_E_RANGE", "CTK_E_COMM"))

READ_CHUNK_FN = ABI.callbacks["ctk_read_chunk_fn"]
WRITE_CHUNK_FN = ABI.callbacks["ctk_write_chunk_fn"]           # and ctk_write_values_fn: one signature, one ctypes class
LIFE_PICK_FN = ABI.callbacks["ctk_life_pick_fn"]


def _dtype(struct):
    """a header struct of scalars as the numpy dtype with C's layout"""
    return np.dtype([(n, np.dtype(t)) for n, t in ABI.structs[struct]], align=True)


LIFE_ROW = _dtype("ctk_life_row")
LIFE_EXACT = _dtype("ctk_life_exact")


class CommError(ContrackHipError):
    """CTK_E_COMM: another rank of the time-shard path gave up, died or did not arrive in time; the communicator is retired"""


class InvalidArgumentError(ContrackHipError, ValueError):
    """CTK_E_INVALID / CTK_E_RANGE from the composite entries: a ContrackHipError that `except ValueError` catches as well, as it
    catches the same mistakes of the frequency entries"""


class BandSpec(C.Structure):
    """ctk_band_spec of include/contrack_hip.h"""
    _fields_ = ABI.structs["ctk_band_spec"]


class BandOut(C.Structure):
    """ctk_band_out of include/contrack_hip.h"""
    _fields_ = ABI.structs["ctk_band_out"]


class FormQuery(C.Structure):
    """ctk_form_query of include/contrack_hip_debug.h"""
    _fields_ = ABI.structs["ctk_form_query"]


class FormPlan(C.Structure):
    """ctk_form_plan of include/contrack_hip_debug.h"""
    _fields_ = ABI.structs["ctk_form_plan"]


def debug_band_plan(T, nx, aligned16=True, form=-1, rows=-1):
    """ctk_debug_band_plan: what ctk_band_plan (csrc/ctk_forms.h) decides, as a dict (form 0 vector / 1 general, rows in flight, threads
    per step, workgroups); no handle, no GPU"""
    v = np.zeros(4, dtype=np.int64)
    check(lib().ctk_debug_band_plan(int(T), int(nx), int(bool(aligned16)), int(form), int(rows), v.ctypes.data))
    return dict(form=int(v[0]), rows=int(v[1]), quads=int(v[2]), grid=int(v[3]))


def debug_percentile_field_plan(keybytes, max_pool_steps, ngroups, window):
    """ctk_debug_percentile_field_plan: what ctk_pfield_plan (csrc/ctk_forms.h) decides, as a dict (form 0 direct / 1 ring, cap in pool
    timesteps, pixel tile, ring bytes); no handle, no GPU"""
    v = np.zeros(4, dtype=np.int64)
    check(lib().ctk_debug_percentile_field_plan(int(keybytes), int(max_pool_steps), int(ngroups), int(window), v.ctypes.data))
    return dict(form=int(v[0]), cap=int(v[1]), tile=int(v[2]), ring_bytes=int(v[3]))


PCTL_REFUSALS = ("fine", "window", "slots", "band", "day")


def debug_percentile_groups_plan(keybits, nband, ngroups, window, max_steps_of_a_group=1):
    """ctk_debug_percentile_groups_plan: what ctk_pctl_form and ctk_pctl_refusal (csrc/ctk_forms.h) decide, as a dict (levels, sweeps,
    stride, chunk, chunks, shift and bits of every level, refusal as one of PCTL_REFUSALS); no handle, no GPU"""
    v = np.zeros(22, dtype=np.int64)
    check(lib().ctk_debug_percentile_groups_plan(int(keybits), int(nband), int(ngroups), int(window), int(max_steps_of_a_group), v.ctypes.data))
    n = int(v[0])
    return dict(levels=n, sweeps=int(v[1]), stride=int(v[2]), chunk=int(v[3]), chunks=int(v[4]), shift=v[5:5 + n].tolist(), bits=v[13:13 + n].tolist(),
                refusal=PCTL_REFUSALS[int(v[21])])


def debug_std_field_plan(ngroups, window=1, skipna=True):
    """ctk_debug_std_field_plan: what ctk_std_plan (csrc/ctk_forms.h) decides, as a dict (tile: pixels per workgroup, 0 where even 8 do
    not fit; planes accumulated; dynamic LDS bytes; max_groups: the most groups a window below the group count may have); no handle,
    no GPU"""
    v = np.zeros(4, dtype=np.int64)
    check(lib().ctk_debug_std_field_plan(int(ngroups), int(window), int(bool(skipna)), v.ctypes.data))
    return dict(tile=int(v[0]), planes=int(v[1]), lds_bytes=int(v[2]), max_groups=int(v[3]))


def debug_lifecycle_plan(T, ny, nx, f64=False, flag_align=0, field_align=0):
    """ctk_debug_lifecycle_plan: what ctk_life_plan (csrc/ctk_forms.h) decides for slabs that start flag_align / field_align bytes past
    a 32-byte boundary, as a dict (rw rows per wave, nsx strips per row, nby workgroups per strip, vec, ks); no handle, no GPU"""
    v = np.zeros(5, dtype=np.int64)
    check(lib().ctk_debug_lifecycle_plan(int(T), int(ny), int(nx), int(bool(f64)), int(flag_align), int(field_align), v.ctypes.data))
    return dict(rw=int(v[0]), nsx=int(v[1]), nby=int(v[2]), vec=int(v[3]), ks=int(v[4]))


def anom_plan(elem_bytes, smooth, nt, npix, waves_wanted=0, grid_y_max=0):
    """ctk_debug_anom_plan: what ctk_anom_plan (csrc/ctk_forms.h) decides for an anomaly launch of nt output steps, as a dict (form 1 LDS
    ring / 0 plain, lds bytes, tile output steps per workgroup, gx, gy); waves_wanted / grid_y_max: 0 the rule's.  Host only."""
    v = np.zeros(5, dtype=np.int64)
    check(lib().ctk_debug_anom_plan(int(elem_bytes), int(smooth), int(nt), int(npix), int(waves_wanted), int(grid_y_max), v.ctypes.data))
    return dict(zip(("form", "lds", "tile", "gx", "gy"), (int(a) for a in v)))


FILTER_EDGES = {"nan": ABI.constants["CTK_FILTER_EDGES_NAN"], "renorm": ABI.constants["CTK_FILTER_EDGES_RENORM"]}


def filter_plan(elem_bytes, K, stride, nout, npix, waves_wanted=0, grid_y_max=0, forced=-1):
    """ctk_debug_filter_plan: what ctk_filter_plan (csrc/ctk_forms.h) decides for a time-filter launch of nout outputs, as a dict (form 1
    LDS ring / 0 plain, threads per workgroup, lds bytes, tile outputs per workgroup, gx, gy); waves_wanted / grid_y_max: 0 the rule's,
    forced: -1 the rule's form.  Host only."""
    v = np.zeros(6, dtype=np.int64)
    check(lib().ctk_debug_filter_plan(int(elem_bytes), int(K), int(stride), int(nout), int(npix), int(waves_wanted), int(grid_y_max), int(forced), v.ctypes.data))
    return dict(zip(("form", "threads", "lds", "tile", "gx", "gy"), (int(a) for a in v)))


def _filter_weights(weights):
    """(w as float64 array or None for box mode, K) of a `weights` that is an array of taps or an int K"""
    if np.ndim(weights) == 0:
        if isinstance(weights, (bool, np.bool_)) or int(weights) != weights:
            raise ValueError("weights must be an array of taps or an int K (box mode)")
        return None, int(weights)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError("weights must be a 1-D array of at least one tap")
    return w, int(w.size)


def filter_offset(K, stride, offset=None):
    """the offset of a filter call: as given, or the default -- a centred window (-(K // 2)) at stride 1, blocks counted from the segment
    start (0) otherwise"""
    if offset is None:
        return -(K // 2) if stride == 1 else 0
    return int(offset)


def filter_layout(T, K, stride=1, offset=None, segments=None):
    """ctk_filter_layout: where the outputs of a time filter of K taps lie on an axis of T steps, as (first, label, out_starts) -- per
    output the step of tap 0 and the label step first + K // 2, per segment its first output.  len(first) is T_out.  Host only."""
    st = _seg_starts(segments if segments is not None else [])
    off = filter_offset(int(K), int(stride), offset)
    first = np.zeros(max(int(T), 1), dtype=np.int64)
    out_starts = np.zeros(max(st.shape[0], 1), dtype=np.int64)
    n = C.c_int64(0)
    check(lib().ctk_filter_layout(int(T), int(K), int(stride), off, st.ctypes.data if st.size else None, st.shape[0], first.ctypes.data, out_starts.ctypes.data,
                                  C.byref(n)))
    first = first[:n.value].copy()
    return first, first + int(K) // 2, out_starts


def level_plan(elem_bytes, nsel, npix, steps, aligned=True):
    """ctk_debug_level_plan: what ctk_level_plan (csrc/ctk_forms.h) decides for a level_mean launch, as a dict (vec 1 vector / 0 scalar
    form, vpt pixels per thread, unroll, bps workgroups per step, blocks, grid, xcd); no handle, no GPU"""
    v = np.zeros(7, dtype=np.int64)
    check(lib().ctk_debug_level_plan(int(elem_bytes), int(nsel), int(npix), int(steps), int(bool(aligned)), v.ctypes.data))
    return dict(vec=int(v[0]), vpt=int(v[1]), unroll=int(v[2]), bps=int(v[3]), blocks=int(v[4]), grid=int(v[5]), xcd=int(v[6]))


def reversal_plan(elem_bytes, ny, nx, steps, aligned=True):
    """ctk_debug_reversal_plan: what ctk_reversal_plan (csrc/ctk_forms.h) decides for a reversal launch, as a dict (vec 1 vector / 0
    scalar form, vpt pixels per thread, bps workgroups per step, blocks, grid, xcd); no handle, no GPU"""
    v = np.zeros(6, dtype=np.int64)
    check(lib().ctk_debug_reversal_plan(int(elem_bytes), int(ny), int(nx), int(steps), int(bool(aligned)), v.ctypes.data))
    return dict(vec=int(v[0]), vpt=int(v[1]), bps=int(v[2]), blocks=int(v[3]), grid=int(v[4]), xcd=int(v[5]))


SUBSET_FORMS = ("bitmap", "search_lds", "search_glb", "row_lds", "row_glb")
SUBSET_KINDS = {"id": ABI.constants["CTK_SUBSET_ID"], "mask": ABI.constants["CTK_SUBSET_MASK"]}


def subset_plan(by_row, max_id, longest, ny, nx, steps=1, hits=False, aligned=True, grid_max=0):
    """ctk_debug_subset_plan: what ctk_subset_plan (csrc/ctk_forms.h) decides for a subset launch from the table's shape -- by_row,
    max_id the largest id of a by-id table, longest its ids or the longest slice of a row table, hits -- as a dict (form 0 .. 4 =
    SUBSET_FORMS, vec 1 vector / 0 scalar, vpt pixels per thread, lds bytes, bps parts per step, blocks parts of work, grid
    workgroups launched, xcd, and the rule's capacities: bitmap_bits, lds_ids, table_share, part_lanes); no handle, no GPU"""
    v = np.zeros(12, dtype=np.int64)
    check(lib().ctk_debug_subset_plan(int(bool(by_row)), int(max_id), int(longest), int(bool(hits)), int(ny), int(nx), int(steps), int(bool(aligned)),
                                      int(grid_max), v.ctypes.data))
    return dict(zip(("form", "vec", "vpt", "lds", "bps", "blocks", "grid", "xcd", "bitmap_bits", "lds_ids", "table_share", "part_lanes"), (int(a) for a in v)))


def _subset_table(table):
    """a table (off, ids) of a subset call (contrack.subset_table makes one) as C-contiguous int64 / int32 arrays; the library checks
    their contents"""
    off, ids = table
    off, ids = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(ids, dtype=np.int32)
    if off.ndim != 1 or ids.ndim != 1 or len(off) < 2:
        raise ValueError("a table is (off, ids): off int64 with 2 or T + 1 entries, ids int32")
    return off, ids


def _subset_kind(kind):
    if kind not in SUBSET_KINDS:
        raise ValueError("kind={!r}: 'id' or 'mask'".format(kind))
    return SUBSET_KINDS[kind]


class _SubsetCall:
    """the arguments every subset entry shares, and the counters it fills"""

    def __init__(self, table, invert, kind, want_hits=True):
        self.off, self.ids = _subset_table(table)
        self.hits = np.zeros(len(self.ids), dtype=np.uint64) if want_hits else None
        self.n = C.c_int64(0)
        self.table = (self.off.ctypes.data, len(self.off), self.ids.ctypes.data, len(self.ids), int(bool(invert)), _subset_kind(kind))

    def counts(self):
        return _ptr(self.hits), C.byref(self.n)


BLOCKSTAT_FORMS = ("row_lds", "row_glb")
BLOCK_WANTS = {"shape": ABI.constants["CTK_BLOCK_SHAPE"], "peaks": ABI.constants["CTK_BLOCK_PEAKS"]}
BLOCK_ROW = _dtype("ctk_block_row")


def _block_want(want):
    """want of a blockstat entry -- 'shape', 'peaks', a sequence of them, or the bit set itself -- as the bit set"""
    if isinstance(want, (int, np.integer)):
        return int(want)
    names = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in names if w not in BLOCK_WANTS]
    if unknown or not names:
        raise ValueError("want={!r}: 'shape', 'peaks' or both".format(want))
    return sum(BLOCK_WANTS[w] for w in set(names))


def blockstat_plan(want, longest, ny, nx, steps=1, elem_bytes=4, aligned=True, grid_max=0):
    """ctk_debug_blockstat_plan: what ctk_blockstat_plan (csrc/ctk_forms.h) decides for a blockstat launch whose table's longest slice
    has `longest` ids, as a dict (form 0 / 1 = BLOCKSTAT_FORMS, vec 1 vector / 0 scalar, vpt pixels per thread, lds bytes, bps parts
    per step, blocks parts of work, grid workgroups launched, xcd, passes launches per chunk, words of an entry's bit set, entry
    bytes of LDS per entry, and the rule's capacities: lds_budget, lds_entries at this nx, part_lanes); no handle, no GPU"""
    v = np.zeros(14, dtype=np.int64)
    check(lib().ctk_debug_blockstat_plan(_block_want(want), int(elem_bytes), int(longest), int(ny), int(nx), int(steps), int(bool(aligned)), int(grid_max),
                                         v.ctypes.data))
    return dict(zip(("form", "vec", "vpt", "lds", "bps", "blocks", "grid", "xcd", "passes", "words", "entry", "lds_budget", "lds_entries", "part_lanes"),
                    (int(a) for a in v)))


class _BlockstatCall:
    """the arguments every blockstat entry shares, and the rows it fills"""

    def __init__(self, table, want):
        self.off, self.ids = _subset_table(table)
        self.rows = np.zeros(len(self.ids), dtype=BLOCK_ROW)
        self.args = (self.off.ctypes.data, len(self.off), self.ids.ctypes.data, len(self.ids), _block_want(want), self.rows.ctypes.data)


def lwa_plan(elem_bytes, rows, nx, ndom=1, steps=1, aligned=True):
    """ctk_debug_lwa_plan: what ctk_lwa_plan (csrc/ctk_forms.h) decides for a local-wave-activity launch whose longest domain has
    `rows` rows, as a dict (ok 1 / 0 the domain does not fit in LDS, vec 1 vector / 0 scalar form, strip columns, nstrips, lds and
    lds_sel bytes of the two kernels, blocks, grid, xcd of the integrals' launch, sel_blocks, sel_grid, sel_xcd of the contours');
    no handle, no GPU"""
    v = np.zeros(12, dtype=np.int64)
    check(lib().ctk_debug_lwa_plan(int(elem_bytes), int(rows), int(nx), int(ndom), int(steps), int(bool(aligned)), v.ctypes.data))
    return dict(zip(("ok", "vec", "strip", "nstrips", "lds", "lds_sel", "blocks", "grid", "xcd", "sel_blocks", "sel_grid", "sel_xcd"), (int(a) for a in v)))


def composite_plan(elem_bytes, npix, unroll=-1):
    """ctk_debug_composite_plan: what ctk_composite_plan (csrc/ctk_forms.h) decides for a k_composite launch, as a dict (unroll: the
    widest batch of time steps, blocks, grid); unroll: what debug_set_composite would force; no handle, no GPU"""
    v = np.zeros(3, dtype=np.int64)
    check(lib().ctk_debug_composite_plan(int(elem_bytes), int(npix), int(unroll), v.ctypes.data))
    return dict(unroll=int(v[0]), blocks=int(v[1]), grid=int(v[2]))


def centred_plan(elem_bytes, nbins, hy, hx, max_bin=0, kept=None, form=-1, unroll=-1, threads=-1):
    """ctk_debug_centred_plan: what ctk_centred_plan (csrc/ctk_forms.h) decides for a centred launch whose longest bin has max_bin
    stamps and whose bins together have `kept` (None: max_bin, one bin), as a dict (form: 0 plain / 1 fed, unroll: the batch of stamps of a lane or a feeder wave, threads: cells of a bin per
    workgroup, parts: workgroups per bin, blocks, grid); form, unroll, threads: what debug_set_centred would force; no handle, no GPU"""
    v = np.zeros(6, dtype=np.int64)
    check(lib().ctk_debug_centred_plan(int(elem_bytes), int(nbins), int(hy), int(hx), int(max_bin), int(max_bin if kept is None else kept), int(form),
                                       int(unroll), int(threads), v.ctypes.data))
    return dict(form=int(v[5]), unroll=int(v[0]), threads=int(v[1]), parts=int(v[2]), blocks=int(v[3]), grid=int(v[4]))


def forms(T, ny, nx, nt=None, aligned16=True, async_passes=24, n_cus=256, **query):
    """ctk_debug_forms: what the library's launch rules (csrc/ctk_forms.h) decide for these numbers, as a dict; no handle, no GPU.
    nt defaults to T; every other field of FormQuery defaults to 0."""
    q = FormQuery(T=T, nt=T if nt is None else nt, ny=ny, nx=nx, aligned16=int(aligned16), async_passes=async_passes, n_cus=n_cus,
                  **{k: int(v) for k, v in query.items()})
    p = FormPlan()
    check(lib().ctk_debug_forms(C.byref(q), C.byref(p)))
    return {n: getattr(p, n) for n, _ in FormPlan._fields_}


def debug_live():
    """ctk_debug_live: (device buffers, pinned buffers, events, streams) the library holds in this process; no handle, no GPU."""
    out = (C.c_int64 * 4)()
    check(lib().ctk_debug_live(out))
    return tuple(out)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ContrackHipError(
            "libcontrack_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C contrack_amd/csrc`; the HIP path has no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    missing = [name for name in ABI.functions if not hasattr(L, name)]
    if missing:
        raise ContrackHipError("%s does not export %s, which the headers in %s declare" % (LIB_PATH, ", ".join(missing), INCLUDE_DIR))
    for name, (restype, argtypes) in ABI.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _seg_starts(segments):
    """segment starts given with a call as a C-contiguous int64 array (the library checks their values)"""
    st = np.asarray(segments)
    if st.ndim != 1 or (st.size and st.dtype.kind not in "iu"):
        raise ValueError("segment starts must be a 1-D integer array")
    return np.ascontiguousarray(st, dtype=np.int64)


def _thr_or_field(thr, T):
    """per-step thresholds as float64 (T,), or None: the handle's threshold field (Tracker.set_threshold_field)"""
    if thr is None:
        return None
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    if thr.shape != (T,):
        raise ValueError("thr must have shape (T,) and wrow (ny,)")
    return thr


def _groups(group, T, ngroups=None):
    """group ids per timestep as int32 (T,) and the number of groups; group None: one group (ids NULL).  Ids are checked against
    [0, ngroups) by the library; here only what the conversion to int32 could hide."""
    if group is None:
        return None, 1 if ngroups is None else int(ngroups)
    g = np.asarray(group)
    if g.ndim != 1 or g.shape[0] != T:
        raise ValueError("group must hold one id per timestep (%d), not shape %s" % (T, g.shape))
    if g.dtype.kind not in "iu":
        raise ValueError("group ids must be integers")
    if g.size and (g.min() < np.iinfo(np.int32).min or g.max() > np.iinfo(np.int32).max):
        raise ValueError("group ids beyond int32")
    g = np.ascontiguousarray(g, dtype=np.int32)
    return g, (int(g.max()) + 1 if g.size else 1) if ngroups is None else int(ngroups)


def _level_weights(weights, nlev):
    """weights of a level_mean call as a C-contiguous float64 (nlev,) array: each finite and >= 0, one > 0 (checked here, before the
    library is touched, and again by it)"""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] != nlev:
        raise ValueError("weights must hold one value per level (%d), not shape %s" % (nlev, w.shape))
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("each weight must be finite and >= 0")
    if not np.any(w > 0):
        raise ValueError("all weights are zero: no level is selected")
    return w


def _reversal_rows(rows, ny):
    """the row table of a reversal call (a mapping with eq, po, dE, tS, tN and, for the third criterion, eq2 and tS2; see
    contrack.reversal_rows / reversal_limits) as the seven pointer arguments of ctk_reversal_* and the arrays they point into"""
    second = rows.get("eq2") is not None
    if second != (rows.get("tS2") is not None):
        raise ValueError("eq2 and tS2 go together (both or neither)")
    keep = []
    for key, dt in (("eq", np.int32), ("po", np.int32), ("eq2", np.int32), ("dE", np.float64), ("tS", np.float64), ("tN", np.float64), ("tS2", np.float64)):
        if key in ("eq2", "tS2") and not second:
            keep.append(None)
            continue
        a = np.ascontiguousarray(rows[key], dtype=dt)
        if a.shape != (ny,):
            raise ValueError("rows[%r] must hold one value per latitude row (%d), not shape %s" % (key, ny, a.shape))
        keep.append(a)
    return [_ptr(a) for a in keep], keep


LWA_PARTS = ('total', 'anticyclonic', 'cyclonic')


def _lwa_rows(rows, ny):
    """the row table of a local-wave-activity call (a mapping with dom_off, dom_rows, active, W, q, S; see contrack.lwa_rows) as the
    seven table arguments of ctk_lwa_* (ndom first) and the arrays the pointers point into.  The library checks the values."""
    off = np.ascontiguousarray(rows["dom_off"], dtype=np.int32)
    if off.ndim != 1 or off.size not in (2, 3):
        raise ValueError("rows['dom_off'] must hold ndom + 1 offsets for one or two domains")
    dom = np.ascontiguousarray(rows["dom_rows"], dtype=np.int32)
    if dom.ndim != 1 or dom.size < max(int(off.max()), 1):
        raise ValueError("rows['dom_rows'] must hold the %d rows that dom_off names" % int(off.max()))
    keep = [off, dom]
    for key, dt in (("active", np.uint8), ("W", np.uint32), ("q", np.float64), ("S", np.float64)):
        a = np.ascontiguousarray(rows[key], dtype=dt)
        if a.shape != (ny,):
            raise ValueError("rows[%r] must hold one value per latitude row (%d), not shape %s" % (key, ny, a.shape))
        keep.append(a)
    return [int(off.size) - 1] + [_ptr(a) for a in keep], keep


def _lwa_part(part):
    if isinstance(part, str):
        if part not in LWA_PARTS:
            raise ValueError("part={!r}: one of {}".format(part, LWA_PARTS))
        return LWA_PARTS.index(part)
    return int(part)


def _group_ids(group, T):
    """group ids as a C-contiguous int32 (T,) array (the library checks their values)"""
    group = np.ascontiguousarray(group, dtype=np.int32)
    if group.shape != (T,):
        raise ValueError("group must hold one id per timestep")
    return group


def _above(above):
    a = int(above)
    if a < np.iinfo(np.int32).min or a > np.iinfo(np.int32).max:
        raise ValueError("above must fit int32")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _spell_args(T, group=None, ngroups=None, segments=None, by_id=True, min_duration=1):
    """the arguments the spell entries share, checked before the library is touched (it checks them again): (group ids int32 or
    None, G, segment starts int64 or None, by_id 0 / 1, min_duration).  ValueError names the value that is wrong."""
    T = int(T)
    if T < 1:
        raise ValueError("bad shape: T=%d" % T)
    if T > 2 ** 32 - 1:
        raise ValueError("T=%d timesteps do not fit the uint32 durations (at most 2^32 - 1)" % T)
    g, G = _groups(group, T, ngroups)
    if G < 1:
        raise ValueError("ngroups=%d (at least 1)" % G)
    if g is not None and g.size and (g.min() < 0 or g.max() >= G):
        raise ValueError("group ids must lie in [0, %d): found %d .. %d" % (G, g.min(), g.max()))
    st = None
    if segments is not None:
        st = _seg_starts(segments)
        if st.size == 0 or st[0] != 0:
            raise ValueError("the first segment must start at step 0 (segments = %s)" % (st[:1].tolist(),))
        if np.any(np.diff(st) <= 0):
            raise ValueError("segment starts must be strictly increasing")
        if st[-1] >= T:
            raise ValueError("segment start %d lies beyond the %d time steps" % (st[-1], T))
    if isinstance(by_id, (bool, np.bool_)):
        by_id = int(by_id)
    if not isinstance(by_id, (int, np.integer)) or by_id not in (0, 1):
        raise ValueError("by_id=%r (True / False or 1 / 0)" % (by_id,))
    if isinstance(min_duration, (bool, np.bool_)) or not isinstance(min_duration, (int, np.integer)):
        raise ValueError("min_duration=%r must be an integer" % (min_duration,))
    if min_duration < 1 or min_duration > 2 ** 63 - 1:
        raise ValueError("min_duration=%d (at least 1)" % min_duration)
    return g, G, st, int(by_id), int(min_duration)


def _check_composite(rc):
    """check() for the composite entries: a bad argument is an InvalidArgumentError"""
    if rc in (CTK_E_INVALID, CTK_E_RANGE):
        raise InvalidArgumentError("libcontrack_hip rc=%d: %s" % (rc, lib().ctk_last_error().decode("utf-8", "replace")))
    check(rc)


def _stamps(t, row, col, bin, nbins, hy, hx):
    """the stamp arguments of the centred entries as the library takes them: (R, t int64, row, col, bin int32, nbins, hy, hx).  bin
    None: one bin.  The library checks the values against the grid; here only what the conversions could hide."""
    arrs = []
    for name, a in (("t", t), ("row", row), ("col", col), ("bin", np.zeros(np.shape(t), np.int32) if bin is None else bin)):
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError("%s must be one-dimensional" % name)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("%s must be integers (dtype %s)" % (name, a.dtype))
        lim = np.iinfo(np.int64 if name == "t" else np.int32)
        if a.size and (int(a.max()) > lim.max or int(a.min()) < lim.min):
            raise ValueError("%s does not fit %s" % (name, "int64" if name == "t" else "int32"))
        arrs.append(np.ascontiguousarray(a, dtype=np.int64 if name == "t" else np.int32))
    R = arrs[0].shape[0]
    if any(a.shape[0] != R for a in arrs):
        raise ValueError("t, row, col and bin must have one length (%s)" % ", ".join(str(a.shape[0]) for a in arrs))
    if nbins is None:
        nbins = 1 if bin is None else (max(int(arrs[3].max()) + 1, 1) if R else 1)
    for name, v in (("nbins", nbins), ("hy", hy), ("hx", hx)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s=%r must be an integer" % (name, v))
        if abs(int(v)) > np.iinfo(np.int32).max:
            raise ValueError("%s=%d does not fit int32" % (name, v))
    nbins, hy, hx = int(nbins), int(hy), int(hx)
    if nbins < 1 or hy < 0 or hx < 0 or nbins * (2 * hy + 1) * (2 * hx + 1) >= 2 ** 31:
        raise InvalidArgumentError("nbins=%d hy=%d hx=%d: nbins >= 1, half widths >= 0 and nbins * (2 hy + 1) * (2 hx + 1) < 2^31" % (nbins, hy, hx))
    return (R,) + tuple(arrs) + (nbins, hy, hx)


def _band_args(T, ny, nx, rows, weights, sectors, columns, above):
    """the arguments the band entries share, checked before the library is touched (it checks them again): (y0, y1, weights float64
    (ny,), sectors int32 (nsect, 2), above).  ValueError names the value that is wrong."""
    T, ny, nx = int(T), int(ny), int(nx)
    if T < 1 or ny < 1 or nx < 1:
        raise ValueError("bad shape (T=%d ny=%d nx=%d)" % (T, ny, nx))
    if ny * nx > 2 ** 32 - 1:
        raise ValueError("a plane of ny * nx = %d pixels does not fit the uint32 counts (at most 2^32 - 1)" % (ny * nx))
    try:
        y0, y1 = (int(v) for v in rows)
    except (TypeError, ValueError):
        raise ValueError("rows must be (y0, y1), not %r" % (rows,))
    if not 0 <= y0 < y1 <= ny:
        raise ValueError("the band [%d, %d) is not inside the %d rows" % (y0, y1, ny))
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (ny,):
        raise ValueError("weights must hold one value per row (%d), not shape %s" % (ny, w.shape))
    if not np.all(np.isfinite(w)):
        raise ValueError("each weight must be finite")
    sec = np.zeros((0, 2), dtype=np.int32) if sectors is None else np.asarray(sectors)
    if sec.size == 0:
        sec = np.zeros((0, 2), dtype=np.int32)
    if sec.ndim != 2 or sec.shape[1] != 2 or sec.dtype.kind not in "iu":
        raise ValueError("sectors must be integer pairs (x0, len)")
    for k, (x0, ln) in enumerate(sec.tolist()):
        if not (0 <= x0 < nx and 1 <= ln <= nx):
            raise ValueError("sector %d = (x0=%d, len=%d) needs 0 <= x0 < %d and 1 <= len <= %d" % (k, x0, ln, nx, nx))
    if not columns and sec.shape[0] == 0:
        raise ValueError("neither the column tables nor a sector is asked for")
    return y0, y1, w, np.ascontiguousarray(sec, dtype=np.int32), _above(above)


class _BandCall:
    """the ctypes structures of ONE call of a band entry, made from checked arguments (_band_args): spec, the host outputs as a dict of
    arrays, their structure"""

    def __init__(self, T, ny, nx, rows, weights, sectors, columns, above, field, resident_gen=None):
        y0, y1, w, sec, above = _band_args(T, ny, nx, rows, weights, sectors, columns, above)
        T, ny, nx = int(T), int(ny), int(nx)
        self.T, self.ny, self.nx, self.nsect, self.field, self.columns = T, ny, nx, sec.shape[0], bool(field), bool(columns)
        self._keep = (w, sec)
        self.spec = BandSpec(y0, y1, above, sec.shape[0], w.ctypes.data, sec.ctypes.data if sec.shape[0] else None, int(bool(columns)),
                             int(resident_gen is not None), 0 if resident_gen is None else int(resident_gen))
        self.arrays = {}
        if columns:
            self.arrays.update(cnt=np.empty((T, nx), np.uint32), area=np.empty((T, nx), np.float64))
            if field:
                self.arrays["wx"] = np.empty((T, nx), np.float64)
        if self.nsect:
            self.arrays.update(sec_cnt=np.empty((T, self.nsect), np.uint32), sec_area=np.empty((T, self.nsect), np.float64))
            if field:
                self.arrays["sec_wx"] = np.empty((T, self.nsect), np.float64)

    def out(self, pointers=None):
        """ctk_band_out of the host arrays, or of `pointers` (name -> device address)"""
        src = {k: a.ctypes.data for k, a in self.arrays.items()} if pointers is None else pointers
        return BandOut(*[src.get(n) for n in "cnt area wx sec_cnt sec_area sec_wx".split()])


def _field_dtype(x):
    """float64 stays, everything else is taken as float32 (as run_lifecycle takes its field)"""
    return np.dtype(np.float64) if np.dtype(x) == np.float64 else np.dtype(np.float32)


def check(rc):
    if rc != 0:
        msg = lib().ctk_last_error().decode("utf-8", "replace")
        if rc == CTK_E_NOMEM:
            raise MemoryError(msg)
        if rc in (CTK_E_INVALID, CTK_E_RANGE):
            raise ValueError(msg)
        if rc == CTK_E_COMM:
            raise CommError("libcontrack_hip rc=%d: %s" % (rc, msg))
        raise ContrackHipError("libcontrack_hip rc=%d: %s" % (rc, msg))


class _Trampolines:
    """The Python callbacks of ONE call into the library.  An exception must not cross the C frames: a callback that raises
    returns non-zero to the library (which gives up) and the exception is kept; finish() re-raises the first one kept, in preference
    to the library's return code.  The object owns the ctypes callback objects it made: it must live as long as the C call."""

    def __init__(self):
        self.errors = []
        self._keep = []

    def wrap(self, fntype, body):
        """body(*the C arguments) as a callback of `fntype` that returns 0, or 1 after an exception"""
        def call(*a):
            try:
                body(*a)
                return 0
            except BaseException as e:
                self.errors.append(e)
                return 1
        cb = fntype(call)
        self._keep.append(cb)
        return cb

    @staticmethod
    def _view(ptr, ctype, nt, step_shape):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(nt,) + tuple(step_shape))

    def reader(self, source, ctype, step_shape):
        """READ_CHUNK_FN that fills the chunk [t0, t0 + nt), an (nt,) + step_shape view of `ctype`, from `source`: a callable
        source(t0, nt, out) or an array indexed by time.  None: the NULL reader."""
        if source is None:
            return C.cast(None, READ_CHUNK_FN)

        def rd(_user, t0, nt, dst):
            view = self._view(dst, ctype, nt, step_shape)
            if callable(source):
                source(int(t0), int(nt), view)
            else:
                view[...] = source[t0:t0 + nt]
        return self.wrap(READ_CHUNK_FN, rd)

    def writer(self, sink, ctype, step_shape):
        """WRITE_CHUNK_FN that hands the chunk [t0, t0 + nt) to `sink`: a callable sink(t0, nt, values) or an array indexed by
        time.  None: the NULL writer."""
        if sink is None:
            return C.cast(None, WRITE_CHUNK_FN)

        def wr(_user, t0, nt, src):
            view = self._view(src, ctype, nt, step_shape)
            if callable(sink):
                sink(int(t0), int(nt), view)
            else:
                sink[t0:t0 + nt] = view
        return self.wrap(WRITE_CHUNK_FN, wr)

    def finish(self, rc, check=check):
        if self.errors:
            raise self.errors[0]
        check(rc)


def _float_ctype(dt):
    return C.c_float if dt == np.float32 else C.c_double


def _float_array(x, rank, wrong_rank):
    """x as a C-contiguous float32 / float64 array of `rank` dimensions: an np.memmap stays one, another dtype becomes float64;
    wrong_rank: the ValueError's text"""
    if not isinstance(x, np.memmap):
        x = np.ascontiguousarray(x)
    if x.ndim != rank:
        raise ValueError(wrong_rank)
    if x.dtype not in (np.float32, np.float64):
        x = np.ascontiguousarray(x, dtype=np.float64)
    if not x.flags.c_contiguous:
        x = np.ascontiguousarray(x)
    return x


def _value_sink(sink, shape, dt, steps, what, instead, has_instead):
    """The `sink` of a streamed producer (level_mean_cb, reversal_cb, anomalies_stream): None (a new array), False (nothing, if the
    call yields `instead`), a C-contiguous array of `shape` and `dt`, or a writer(t0, nt, values).  Returns (the array the call
    returns or None, what the library writes to or None); steps / what / instead: the words of the ValueError texts."""
    if sink is None:
        out = np.empty(shape, dtype=dt)
        return out, out
    if sink is False:
        if not has_instead:
            raise ValueError("sink=False without %s asks for nothing" % instead)
        return None, None
    if callable(sink):
        return None, sink
    if sink.dtype != dt or sink.shape != tuple(shape) or not sink.flags.c_contiguous:
        raise ValueError("the sink array must be C-contiguous (%s, ny, nx) of the %s's dtype" % (steps, what))
    return sink, sink


def _values_cb(reader, shape, dims, dtype, bind, sink, keep_resident):
    """What level_mean_cb, reversal_cb and lwa_cb share: the reader's shape (dims: its words in the ValueError) and dtype checked, then
    the family's own arguments -- bind(dtype, shape) checks them and returns call(reader, writer), the library call --, then the sink
    (_value_sink) and the two trampolines made and the call carried out.  Returns the array the entry returns, or None."""
    if shape is None or dtype is None:
        raise ValueError("a reader needs shape=%s and dtype" % dims)
    shape = tuple(int(v) for v in shape)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("the field must be float32 or float64")
    call = bind(dt, shape)
    out, sink = _value_sink(sink, (shape[0],) + shape[-2:], dt, "steps", "field", "keep_resident", keep_resident)
    tr = _Trampolines()
    tr.finish(call(tr.reader(reader, _float_ctype(dt), shape[1:]), tr.writer(sink, _float_ctype(dt), shape[-2:])))
    return out


def _flag_i32(flag, wider_hint):
    """the flag slab of an array entry as C-contiguous int32 (time, lat, lon); narrower integers are widened, wider ones are
    refused: `wider_hint` names the entries that take them"""
    flag = np.asarray(flag)
    if flag.ndim != 3:
        raise ValueError("flag must be (time, lat, lon)")
    if flag.dtype != np.int32 and (flag.dtype.kind not in "iub" or flag.dtype.itemsize > 4 or flag.dtype == np.uint32):
        raise ValueError("flag must be int32 here (wider ids: %s)" % wider_hint)
    return np.ascontiguousarray(flag, dtype=np.int32)


def device_count():
    return int(lib().ctk_device_count())


def weights_to_limbs(wrow, npix=1 << 16, with_bits=False):
    """exact integer limbs of float32 row weights: w[y] = (lo[y] + hi[y] * 2**bits) / 2**shift.  npix = ny * nx of the grid
    (only matters when the weights span more than 62 bits).  Returns (lo, hi, shift) or (lo, hi, shift, bits)."""
    wrow = np.ascontiguousarray(wrow, dtype=np.float32)
    lo = np.empty(wrow.shape[0], dtype=np.int64)
    hi = np.empty(wrow.shape[0], dtype=np.int64)
    sh, lb = C.c_int32(0), C.c_int32(0)
    check(lib().ctk_weights_to_limbs(wrow.ctypes.data, wrow.shape[0], int(npix), lo.ctypes.data, hi.ctypes.data, C.byref(sh), C.byref(lb)))
    return (lo, hi, int(sh.value), int(lb.value)) if with_bits else (lo, hi, int(sh.value))


def expand_runs_host(mask, rowstart, run_base, run_val, nx):
    """the host-side decoder of the run-table result transfer on its own (no device call): mask uint64 (T, ny, ceil(nx / 64)),
    rowstart uint32 (T, ny), run_base uint32 (T + 1,), run_val int32 (runs,) -> (flag int32 (T, ny, nx), a zero was written,
    a negative run value was met)"""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    rowstart = np.ascontiguousarray(rowstart, dtype=np.uint32)
    run_base = np.ascontiguousarray(run_base, dtype=np.uint32)
    run_val = np.ascontiguousarray(run_val, dtype=np.int32)
    T, ny, W = mask.shape
    if W != (nx + 63) // 64 or rowstart.shape != (T, ny) or run_base.shape != (T + 1,) or (T and run_val.shape[0] < int(run_base[-1])):
        raise ValueError("table shapes do not fit (T, ny, nx)")
    flag = np.empty((T, ny, nx), dtype=np.int32)
    z, cx = C.c_int(0), C.c_int(0)
    check(lib().ctk_expand_runs_host(mask.ctypes.data, rowstart.ctypes.data, run_base.ctypes.data, run_val.ctypes.data if run_val.size else None,
                                     T, ny, nx, flag.ctypes.data, C.byref(z), C.byref(cx)))
    return flag, bool(z.value), bool(cx.value)


class Result:
    """Owner of a ctk_result (output of the host-side resolver)."""

    def __init__(self, ptr):
        self._p = ptr

    def __del__(self):
        self.free()

    def free(self):
        if getattr(self, "_p", None):
            lib().ctk_result_free(self._p)
            self._p = None

    @property
    def ptr(self):
        return self._p

    def info(self):
        v = [C.c_int64(0) for _ in range(5)]
        check(lib().ctk_result_info(self._p, *[C.byref(x) for x in v]))
        return dict(zip(("n_labels", "n_ops", "n_complex", "n_ambiguous", "n_components"), (int(x.value) for x in v)))

    def arrays(self):
        cl, ops, sco, sto = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nc, nops = C.c_int64(0), C.c_int64(0)
        check(lib().ctk_result_arrays(self._p, C.byref(cl), C.byref(nc), C.byref(ops), C.byref(nops), C.byref(sco), C.byref(sto)))
        n = int(nc.value)
        comp_label = np.ctypeslib.as_array(C.cast(cl, C.POINTER(C.c_int32)), shape=(max(n, 1),))[:n].copy()
        k = int(nops.value)
        opsa = np.ctypeslib.as_array(C.cast(ops, C.POINTER(C.c_int32)), shape=(max(k, 1) * 8,))[:k * 8].copy().reshape(k, 8)
        return comp_label, opsa

    def shard_offsets(self):
        """(component offsets, timestep offsets) of every shard inside comp_label: two int64 arrays of nshards+1"""
        cl, ops, sco, sto = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nc, nops = C.c_int64(0), C.c_int64(0)
        check(lib().ctk_result_arrays(self._p, C.byref(cl), C.byref(nc), C.byref(ops), C.byref(nops), C.byref(sco), C.byref(sto)))
        k = int(lib().ctk_result_nshards(self._p)) + 1
        co = np.ctypeslib.as_array(C.cast(sco, C.POINTER(C.c_int64)), shape=(k,)).copy()
        to = np.ctypeslib.as_array(C.cast(sto, C.POINTER(C.c_int64)), shape=(k,)).copy()
        return co, to


def resolve(blobs, overlap, twosided):
    """blobs: list of bytes-like / (address, nbytes) table blobs in time order."""
    L = lib()
    n = len(blobs)
    ptrs = (C.c_void_p * n)()
    sizes = (C.c_size_t * n)()
    keep = []
    for i, b in enumerate(blobs):
        if isinstance(b, tuple):
            ptrs[i], sizes[i] = b
        else:
            arr = np.frombuffer(b, dtype=np.uint8)
            keep.append(arr)
            ptrs[i], sizes[i] = arr.ctypes.data, arr.size
    out = C.c_void_p()
    check(L.ctk_resolve(ptrs, sizes, n, float(overlap), int(bool(twosided)), C.byref(out)))
    return Result(out)


COMM_ID_BYTES = 128


def rccl_library():
    """the librccl file the RCCL transport loaded ("" before the first RCCL communicator)"""
    return (lib().ctk_comm_rccl_library() or b"").decode()


def comm_unique_id():
    """128 opaque bytes (ncclGetUniqueId) made on rank 0; every rank passes them to Comm.rccl"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().ctk_comm_unique_id(buf))
    return buf.raw


class CommGroup:
    """Several ranks inside one process (one host thread per rank): ctk_comm_group"""

    def __init__(self, world):
        self._g = C.c_void_p()
        self.world = int(world)
        check(lib().ctk_comm_group_create(self.world, C.byref(self._g)))

    def close(self):
        if getattr(self, "_g", None):
            lib().ctk_comm_group_destroy(self._g)
            self._g = None

    def __del__(self):
        self.close()


class Comm:
    """The communicator of the time-sharded path (ctk_comm), bound to one Tracker."""

    def __init__(self, ptr, keep=None):
        self._c, self._keep = ptr, keep

    @classmethod
    def rccl(cls, tracker, unique_id, rank, world):
        c = C.c_void_p()
        check(lib().ctk_comm_init_rccl(tracker.handle, unique_id, int(rank), int(world), C.byref(c)))
        return cls(c)

    @classmethod
    def local(cls, tracker, group, rank):
        c = C.c_void_p()
        check(lib().ctk_comm_init_local(tracker.handle, group._g, int(rank), C.byref(c)))
        return cls(c, keep=group)

    @classmethod
    def shm(cls, tracker, name, rank, world):
        c = C.c_void_p()
        check(lib().ctk_comm_init_shm(tracker.handle, name.encode(), int(rank), int(world), C.byref(c)))
        return cls(c)

    @property
    def ptr(self):
        return self._c

    @property
    def rank(self):
        return int(lib().ctk_comm_rank(self._c))

    @property
    def world(self):
        return int(lib().ctk_comm_world(self._c))

    def barrier(self):
        check(lib().ctk_comm_barrier(self._c))

    def allgather(self, arr):
        """small host array (<= 4096 bytes) from every rank -> array (world, ...)"""
        arr = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + arr.shape, dtype=arr.dtype)
        check(lib().ctk_comm_allgather_host(self._c, arr.ctypes.data, out.ctypes.data, arr.nbytes))
        return out

    def set_timeout(self, seconds):
        """deadline of every wait of the time-shard path on this communicator (default 120 s / CTK_COMM_TIMEOUT_S)"""
        check(lib().ctk_comm_set_timeout(self._c, float(seconds)))

    def failed(self):
        """None, or (code, rank) of the failure published by the rank that gave up first"""
        a, b = C.c_int(0), C.c_int(-1)
        check(lib().ctk_comm_failed(self._c, C.byref(a), C.byref(b)))
        return None if a.value == 0 else (int(a.value), int(b.value))

    def abort(self, code=-5):
        """this rank gives up: the other ranks' calls return CommError instead of waiting for it"""
        check(lib().ctk_comm_abort_rank(self._c, int(code)))

    def ops(self):
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().ctk_comm_ops(self._c, C.byref(a), C.byref(b)))
        return dict(neighbour_exchanges=int(a.value), allgathers=int(b.value))

    def close(self):
        if getattr(self, "_c", None):
            lib().ctk_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()


class _ResultPool:
    """Recycles the memory of result arrays (the `flag` slabs the host-array entries return).

    A fresh np.empty array consists of pages that do not exist yet: the device -> host copy then runs behind first-touch page
    faults (47 GB/s through eight bounce threads at best; measured, tools/d2h_probe*.py).  Memory that HAS been touched can be
    registered with HIP in ~1 ms and takes the result in ONE DMA at PCIe rate (57 GB/s) -- so the blocks of results the caller has
    dropped are kept (a few, CTK_RESULT_POOL_MB in all, default 2048), registered on their first reuse, and handed out again.
    A loop over ensemble members that writes each result out and drops it gets every result but the first at DMA speed; a
    caller that keeps every result sees exactly the old behaviour.  The arrays handed out are ordinary numpy arrays; a block
    returns to the pool when the last view of it is gone (weakref on the buffer all views share)."""

    def __init__(self, tracker):
        import threading
        import collections
        self._trk = weakref.ref(tracker)
        self._lock = threading.RLock()       # re-entrant: belt and braces, see _release
        self._free = []                      # blocks: dict(mem=np.uint8 array, registered=bool)
        self._leased = {}                    # id(block) -> block
        self._returned = collections.deque()  # blocks whose last view died; filed under the lock by _drain
        self._closed = False
        self.cap = int(float(os.environ.get("CTK_RESULT_POOL_MB", "2048")) * (1 << 20))
        self.hits = self.misses = 0

    def take(self, shape, dtype=np.int32):
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        if nbytes < (8 << 20) or self.cap <= 0:            # small results: nothing to gain
            return np.empty(shape, dtype=dtype)
        blk = None
        with self._lock:
            self._drain()
            i = 0
            while i < len(self._free):
                b = self._free[i]
                if nbytes <= b["mem"].nbytes <= nbytes + nbytes // 4:
                    blk = self._free.pop(i)
                    break
                i += 1
        if blk is None:
            self.misses += 1
            blk = dict(mem=self._pages(nbytes), registered=False)
        else:
            self.hits += 1
            trk = self._trk()
            if not blk["registered"] and trk is not None and trk.handle and not trk.result_as_runs:
                # (touched by its first use: registration is cheap now; a failure just leaves the block pageable.  With the
                # result travelling as run tables -- the default -- host threads write the block: nothing to register)
                blk["registered"] = lib().ctk_host_register(trk.handle, blk["mem"].ctypes.data, blk["mem"].nbytes) == 0
        carr = (C.c_ubyte * nbytes).from_address(blk["mem"].ctypes.data)
        with self._lock:
            self._leased[id(blk)] = blk
        weakref.finalize(carr, self._release, blk)
        return np.frombuffer(carr, dtype=dtype).reshape(shape)

    @staticmethod
    def _pages(nbytes):
        """a block of pages of its own (anonymous mapping, page-aligned, whole pages).  hipHostRegister pins whole pages: a block
        from malloc can share its first and last page with a neighbouring array (the input slab, say), and registering the block
        then registers part of that array too -- its next copy to the device faulted on the GPU"""
        import mmap
        size = (nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE
        return np.frombuffer(mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE), dtype=np.uint8)

    def _unregister(self, blk):
        trk = self._trk()
        if blk["registered"] and trk is not None and trk.handle:
            lib().ctk_host_unregister(trk.handle, blk["mem"].ctypes.data)
        blk["registered"] = False

    def _release(self, blk):
        """weakref.finalize callback: runs wherever the last reference dies -- possibly inside a cyclic-GC pass that a
        thread triggered while it held the pool's lock.  So it takes no lock and allocates nothing GC-tracked: the block goes
        onto a deque (append is atomic) and is filed by the next take() / close()."""
        self._returned.append(blk)

    def _drain(self):
        """file the returned blocks (caller holds the lock)"""
        drop = []
        while True:
            try:
                blk = self._returned.popleft()
            except IndexError:
                break
            self._leased.pop(id(blk), None)
            held = 0
            for b in self._free:
                held += b["mem"].nbytes
            if not self._closed and self._trk() is not None and held + blk["mem"].nbytes <= self.cap:
                self._free.append(blk)
            else:
                drop.append(blk)
        for blk in drop:
            self._unregister(blk)

    def close(self):
        """the handle goes away: nothing stays registered (arrays still held by the caller remain valid, pageable memory)
        and nothing that comes back afterwards is kept"""
        with self._lock:
            self._closed = True
            self._drain()
            blocks = self._free + list(self._leased.values())
            self._free = []
            self._leased = {}
        for b in blocks:
            self._unregister(b)


class Tracker:
    """One GPU + stream + reusable device workspace (ctk_handle)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().ctk_create(C.byref(self._h), int(device)))
        self._pool = _ResultPool(self)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_pool", None) is not None:
                self._pool.close()
            lib().ctk_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # ---- one call, host numpy in / out ------------------------------------------------------
    def track(self, anom, thr, cmp_op, wrow, overlap, persistence, twosided=True, f64=False, out=None):
        anom = np.ascontiguousarray(anom, dtype=np.float64 if f64 else np.float32)
        T, ny, nx = anom.shape
        thr = _thr_or_field(thr, T)
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        if wrow.shape != (ny,):
            raise ValueError("thr must have shape (T,) and wrow (ny,)")
        if out is not None:
            if out.dtype != np.int32 or out.shape != (T, ny, nx) or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError("out must be a writable C-contiguous int32 array of the slab's shape")
            flag = out
        else:
            flag = self._pool.take((T, ny, nx))
        n = C.c_int64(0)
        fn = lib().ctk_track_f64 if f64 else lib().ctk_track_f32
        check(fn(self._h, anom.ctypes.data, T, ny, nx, _ptr(thr), int(cmp_op), wrow.ctypes.data,
                                  float(overlap), int(persistence), int(bool(twosided)), flag.ctypes.data, C.byref(n)))
        return flag, int(n.value)

    # ---- streaming entries (next row N4) ------------------------------------------------------------------------
    def track_stream(self, source, thr, cmp_op, wrow, overlap, persistence, twosided=True, sink=None, shape=None, dtype=None, chunk_steps=0,
                     segments=None):
        """ctk_track_* with the slab passing through chunk-sized device buffers (device footprint: 4 chunks + slab / 32).

        source: a (T, ny, nx) float32 / float64 array (np.memmap included), or a callable reader(t0, nt, out) that fills
                `out` (a (nt, ny, nx) view of pinned memory) with the timesteps [t0, t0 + nt) -- then `shape` = (T, ny, nx)
                and `dtype` are required;
        sink:   None (a new int32 array is returned), an int32 array (T, ny, nx), or a callable writer(t0, nt, flags) that
                receives each flag chunk as a (nt, ny, nx) int32 view valid during the call.
        segments: None, or the first step of every independent time segment (0 first, strictly increasing, below T) -- the
                semantics of set_segments, given with the call (ctk_track_stream_seg_*); breaks and chunks are unrelated.
        Returns (flag array or None, n_tracked)."""
        L = lib()
        if callable(source):
            if shape is None or dtype is None:
                raise ValueError("a reader callback needs shape=(T, ny, nx) and dtype")
            T, ny, nx = (int(v) for v in shape)
            dt = np.dtype(dtype)
        else:
            source = np.ascontiguousarray(source) if not isinstance(source, np.memmap) else source
            if source.dtype not in (np.float32, np.float64):
                source = np.ascontiguousarray(source, dtype=np.float64)
            T, ny, nx = source.shape
            dt = source.dtype
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the slab must be float32 or float64")
        thr = _thr_or_field(thr, T)
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        if wrow.shape != (ny,):
            raise ValueError("thr must have shape (T,) and wrow (ny,)")
        out = None
        if sink is None:
            out = sink = np.empty((T, ny, nx), dtype=np.int32)
        elif not callable(sink):
            if sink.dtype != np.int32 or sink.shape != (T, ny, nx) or not sink.flags.c_contiguous:
                raise ValueError("the sink array must be C-contiguous int32 (T, ny, nx)")
            out = sink
        n = C.c_int64(0)
        tail = (_ptr(thr), int(cmp_op), wrow.ctypes.data, float(overlap), int(persistence), int(bool(twosided)))
        st = None if segments is None else _seg_starts(segments)
        seg = () if st is None else (st.ctypes.data if st.size else None, st.shape[0])
        if not callable(source) and not callable(sink):
            if st is None:
                fn = L.ctk_track_stream_f64 if dt == np.float64 else L.ctk_track_stream_f32
            else:
                fn = L.ctk_track_stream_seg_f64 if dt == np.float64 else L.ctk_track_stream_seg_f32
            check(fn(self._h, source.ctypes.data, T, ny, nx, *tail, sink.ctypes.data, C.byref(n), int(chunk_steps), *seg))
            return out, int(n.value)
        tr = _Trampolines()
        rcb, wcb = tr.reader(source, _float_ctype(dt), (ny, nx)), tr.writer(sink, C.c_int32, (ny, nx))
        fn = L.ctk_track_stream_cb if st is None else L.ctk_track_stream_seg_cb
        tr.finish(fn(self._h, dt.itemsize, T, ny, nx, rcb, None, *tail, wcb, None, C.byref(n), int(chunk_steps), *seg))
        return out, int(n.value)

    def stream_times(self):
        """ms of the last streaming call: reader callbacks, writer callbacks, input phase, output phase"""
        ms = (C.c_double * 4)()
        check(lib().ctk_stream_times(self._h, ms))
        return dict(zip(("reader", "writer", "input_phase", "output_phase"), (float(v) for v in ms)))

    # ---- blocking frequency (README.rst:159-160) ---------------------------------------------------------------------
    def frequency(self, flag, group=None, ngroups=None, above=0, chunk_steps=0):
        """counts[g, y, x] = #{t : group[t] == g and flag[t, y, x] > above} of an int32 (T, ny, nx) host slab (ctk_frequency: chunks
        of `chunk_steps` timesteps pass through the device, 0: about 256 MB each).  group None: one group.  ngroups None:
        max(group) + 1.  Returns uint32 (ngroups, ny, nx)."""
        flag = _flag_i32(flag, "frequency_cb, or contrack.frequency_numpy")
        T, ny, nx = flag.shape
        g, G = _groups(group, T, ngroups)
        counts = np.empty((max(G, 1), ny, nx), dtype=np.uint32)
        check(lib().ctk_frequency(self._h, flag.ctypes.data, T, ny, nx, _ptr(g), G, _above(above), counts.ctypes.data, int(chunk_steps)))
        return counts

    def frequency_cb(self, reader, shape, group=None, ngroups=None, above=0, chunk_steps=0):
        """the same with the flag read chunk by chunk: reader(t0, nt, out) fills `out`, an int32 (nt, ny, nx) view of pinned memory,
        with the timesteps [t0, t0 + nt)"""
        T, ny, nx = (int(v) for v in shape)
        g, G = _groups(group, T, ngroups)
        counts = np.empty((max(G, 1), ny, nx), dtype=np.uint32)
        tr = _Trampolines()
        rcb = tr.reader(reader, C.c_int32, (ny, nx))
        tr.finish(lib().ctk_frequency_cb(self._h, T, ny, nx, rcb, None, _ptr(g), G, _above(above), counts.ctypes.data, int(chunk_steps)))
        return counts

    def frequency_dev(self, flag_dev, T, ny, nx, group=None, ngroups=None, above=0, counts_dev=None, accumulate=False):
        """ctk_frequency_dev on an int32 flag in device memory.  counts_dev None: the uint32 (ngroups, ny, nx) counts are returned;
        else they are written (accumulate: added) to that device buffer and None is returned."""
        g, G = _groups(group, T, ngroups)
        if counts_dev is not None:
            check(lib().ctk_frequency_dev(self._h, flag_dev, int(T), int(ny), int(nx), _ptr(g), G, _above(above), counts_dev, int(bool(accumulate))))
            return None
        counts = np.empty((max(G, 1), int(ny), int(nx)), dtype=np.uint32)
        self._download([counts], lambda d: check(lib().ctk_frequency_dev(self._h, flag_dev, int(T), int(ny), int(nx), _ptr(g), G, _above(above), d, 0)))
        return counts

    def debug_set_freq(self, slice_steps=0, nt=None):
        """k_freq experiments: timesteps per slice (0: the library's rule), nontemporal (True) or plain (False) 16-byte loads, None:
        the library's default (nontemporal)"""
        check(lib().ctk_debug_set_freq(self._h, int(slice_steps), -1 if nt is None else int(bool(nt))))

    def time_freq(self, flag_dev, T, ny, nx, counts_dev, group=None, ngroups=None, above=0, reps=10):
        """k_freq alone between HIP events (counts_dev: device buffer of ngroups * ny * nx uint32): (best, mean) ms per launch"""
        g, G = _groups(group, T, ngroups)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_freq(self._h, flag_dev, int(T), int(ny), int(nx), _ptr(g), G, _above(above), counts_dev, int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- blocked spells per grid point: events, steps, longest (ctk_spell.hip) -----------------------------------------
    def spells(self, flag, group=None, ngroups=None, above=0, by_id=True, min_duration=1, segments=None, chunk_steps=0):
        """(events, steps, longest), uint32 (ngroups, ny, nx), of an int32 (T, ny, nx) host slab (ctk_spells: chunks of `chunk_steps`
        timesteps pass through the device, 0: about 256 MB each).  A spell is a maximal run of steps with flag > above (by_id: and
        the same id) inside one segment; it belongs to the group of its first step and counts if it lasts min_duration steps or
        more.  group None: one group.  segments None: one segment, else the first step of every segment (0 first)."""
        flag = _flag_i32(flag, "spells_cb, or contrack.spells_numpy")
        T, ny, nx = flag.shape
        g, G, st, by, md = _spell_args(T, group, ngroups, segments, by_id, min_duration)
        out = np.empty((3, G, ny, nx), dtype=np.uint32)
        check(lib().ctk_spells(self._h, flag.ctypes.data, T, ny, nx, _ptr(g), G, _ptr(st), 0 if st is None else st.shape[0], _above(above), by, md,
                               out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, int(chunk_steps)))
        return out[0], out[1], out[2]

    def spells_cb(self, reader, shape, group=None, ngroups=None, above=0, by_id=True, min_duration=1, segments=None, chunk_steps=0):
        """the same with the flag read chunk by chunk: reader(t0, nt, out) fills `out`, an int32 (nt, ny, nx) view of pinned memory,
        with the timesteps [t0, t0 + nt)"""
        T, ny, nx = (int(v) for v in shape)
        g, G, st, by, md = _spell_args(T, group, ngroups, segments, by_id, min_duration)
        out = np.empty((3, G, ny, nx), dtype=np.uint32)
        tr = _Trampolines()
        rcb = tr.reader(reader, C.c_int32, (ny, nx))
        tr.finish(lib().ctk_spells_cb(self._h, T, ny, nx, rcb, None, _ptr(g), G, _ptr(st), 0 if st is None else st.shape[0], _above(above), by, md,
                                      out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, int(chunk_steps)))
        return out[0], out[1], out[2]

    def spells_dev(self, flag_dev, T, ny, nx, group=None, ngroups=None, above=0, by_id=True, min_duration=1, segments=None):
        """ctk_spells_dev on an int32 flag in device memory: (events, steps, longest), uint32 (ngroups, ny, nx)"""
        T, ny, nx = int(T), int(ny), int(nx)
        g, G, st, by, md = _spell_args(T, group, ngroups, segments, by_id, min_duration)
        out = np.empty((3, G, ny, nx), dtype=np.uint32)
        self._download([out], lambda d: check(lib().ctk_spells_dev(self._h, flag_dev, T, ny, nx, _ptr(g), G, _ptr(st), 0 if st is None else st.shape[0],
                                                                  _above(above), by, md, d, d.value + out[0].nbytes, d.value + 2 * out[0].nbytes)))
        return out[0], out[1], out[2]

    def set_spell_debug(self, slice_steps=0):
        """k_spell experiments and tests: timesteps per slice (0: the library's rule)"""
        check(lib().ctk_debug_set_spell(self._h, int(slice_steps)))

    def time_spells(self, flag_dev, T, ny, nx, maps_dev, group=None, ngroups=None, above=0, by_id=True, min_duration=1, segments=None, reps=10):
        """k_spell alone between HIP events (maps_dev: device buffer of 3 * ngroups * ny * nx uint32): (best, mean) ms per launch"""
        T, ny, nx = int(T), int(ny), int(nx)
        g, G, st, by, md = _spell_args(T, group, ngroups, segments, by_id, min_duration)
        ms = (C.c_double * 2)()
        one = G * ny * nx * 4
        maps_dev = maps_dev.value if isinstance(maps_dev, C.c_void_p) else int(maps_dev)
        check(lib().ctk_debug_time_spell(self._h, flag_dev, T, ny, nx, _ptr(g), G, _ptr(st), 0 if st is None else st.shape[0], _above(above), by, md,
                                         maps_dev, maps_dev + one, maps_dev + 2 * one, int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- composite over flagged time steps (the step after README.rst:156-164) ---------------------------------------
    def composite(self, flag, x, group=None, ngroups=None, above=0, skipna=False, chunk_steps=0, resident_f64=False):
        """(sum, n): sum[g, y, x] = the float64 sum, in time order, of x[t, y, x] over the t with group[t] == g and flag[t, y, x] >
        above (with skipna: and x not NaN), n[g, y, x] how many there were, of an int32 (T, ny, nx) flag slab and a float32 /
        float64 field slab of the same shape in host memory (ctk_composite_f32 / _f64: chunks of `chunk_steps` time steps of both
        pass through the device, 0: about 256 MB of field each).  x None: the anomaly slab anomalies(keep_resident=True) left on
        the device (resident_f64: its type).  Returns float64 and uint32 (ngroups, ny, nx)."""
        flag = _flag_i32(flag, "composite_cb, or contrack.composite_numpy")
        T, ny, nx = flag.shape
        if x is None:
            f64 = bool(resident_f64)
        else:
            x = np.ascontiguousarray(x, dtype=_field_dtype(np.asarray(x).dtype))
            if x.shape != flag.shape:
                raise ValueError("the field has shape %s, the flag %s" % (x.shape, flag.shape))
            f64 = x.dtype == np.float64
        g, G = _groups(group, T, ngroups)
        s = np.empty((max(G, 1), ny, nx), dtype=np.float64)
        n = np.empty((max(G, 1), ny, nx), dtype=np.uint32)
        fn = lib().ctk_composite_f64 if f64 else lib().ctk_composite_f32
        _check_composite(fn(self._h, flag.ctypes.data, _ptr(x), T, ny, nx, _ptr(g), G, _above(above), int(bool(skipna)), s.ctypes.data, n.ctypes.data,
                            int(chunk_steps)))
        return s, n

    def composite_cb(self, flag_reader, field_reader, shape, dtype, group=None, ngroups=None, above=0, skipna=False, chunk_steps=0):
        """the same with both slabs read chunk by chunk: flag_reader(t0, nt, out) fills an int32 (nt, ny, nx) view of pinned memory
        with the time steps [t0, t0 + nt), field_reader one of `dtype` (float32 / float64); the flag reader is called first.
        field_reader None: the resident anomaly slab of `dtype`."""
        T, ny, nx = (int(v) for v in shape)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        g, G = _groups(group, T, ngroups)
        s = np.empty((max(G, 1), ny, nx), dtype=np.float64)
        n = np.empty((max(G, 1), ny, nx), dtype=np.uint32)
        tr = _Trampolines()
        fcb, xcb = tr.reader(flag_reader, C.c_int32, (ny, nx)), tr.reader(field_reader, _float_ctype(dt), (ny, nx))
        tr.finish(lib().ctk_composite_cb(self._h, dt.itemsize, T, ny, nx, fcb, None, xcb, None, _ptr(g), G, _above(above), int(bool(skipna)),
                                         s.ctypes.data, n.ctypes.data, int(chunk_steps)), _check_composite)
        return s, n

    def composite_dev(self, flag_dev, x_dev, T, ny, nx, group=None, ngroups=None, above=0, skipna=False, f64=False, sum_dev=None, n_dev=None,
                      accumulate=False):
        """ctk_composite_*_dev on an int32 flag and a float32 (f64: float64) field in device memory; x_dev None: the resident anomaly
        slab.  sum_dev / n_dev None: (sum, n) are returned; else they are written to (accumulate: continued from) those device
        buffers of ngroups * ny * nx float64 / uint32 and None is returned."""
        g, G = _groups(group, T, ngroups)
        fn = lib().ctk_composite_f64_dev if f64 else lib().ctk_composite_f32_dev
        args = (self._h, flag_dev, x_dev, int(T), int(ny), int(nx), _ptr(g), G, _above(above), int(bool(skipna)))
        if (sum_dev is None) != (n_dev is None):
            raise ValueError("sum_dev and n_dev go together")
        if sum_dev is not None:
            _check_composite(fn(*args, sum_dev, n_dev, int(bool(accumulate))))
            return None
        s = np.empty((max(G, 1), int(ny), int(nx)), dtype=np.float64)
        n = np.empty((max(G, 1), int(ny), int(nx)), dtype=np.uint32)
        self._download([s, n], lambda ds, dn: _check_composite(fn(*args, ds, dn, 0)))
        return s, n

    def debug_set_composite(self, unroll=-1):
        """test hook for the following composite launches: the widest batch of time steps, -1 the rule (ctk_composite_plan)"""
        check(lib().ctk_debug_set_composite(self._h, int(unroll)))

    def debug_composite_launch(self):
        """(widest batch, workgroups) of the last composite launch; (0, 0): none yet"""
        v = np.zeros(2, dtype=np.int64)
        check(lib().ctk_debug_composite_launch(self._h, v.ctypes.data))
        return int(v[0]), int(v[1])

    def time_composite(self, flag_dev, x_dev, T, ny, nx, sum_dev, n_dev, group=None, ngroups=None, above=0, skipna=False, f64=False, reps=5):
        """k_composite alone between HIP events (sum_dev / n_dev: device buffers of ngroups * ny * nx float64 / uint32): (best, mean)
        ms per launch"""
        g, G = _groups(group, T, ngroups)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_composite(self._h, flag_dev, x_dev, int(bool(f64)), int(T), int(ny), int(nx), _ptr(g), G, _above(above),
                                             int(bool(skipna)), sum_dev, n_dev, int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- reductions over space per step: Hovmoeller columns and sector series (ctk_band.hip) ----------------------------
    def band(self, flag, rows, weights, x=None, sectors=None, columns=True, above=0, chunk_steps=0, resident_gen=None, resident_f64=False):
        """per step t of an int32 (T, ny, nx) host slab and column c, over the rows [y0, y1) = `rows` with flag > above: cnt (uint32),
        area = the float64 sum of weights[y] in rising y and, with a float32 / float64 field x of the same shape, wx = the same sum of
        weights[y] * x; per sector (x0, len) of `sectors` -- the columns x0, x0 + 1, ... modulo nx -- sec_cnt, sec_area, sec_wx: the
        column values added in that order (ctk_band_f32 / _f64: chunks of `chunk_steps` time steps pass through the device, 0: about
        256 MB each).  columns False: only the sector tables come back.  resident_gen: the field is the anomaly slab
        anomalies(keep_resident=True) left on the device, of that resident_generation() (resident_f64: its type).  Returns a dict of
        (T, nx) and (T, nsect) arrays."""
        flag = _flag_i32(flag, "band_cb, or contrack.band_numpy")
        T, ny, nx = flag.shape
        if x is not None:
            x = np.ascontiguousarray(x, dtype=_field_dtype(np.asarray(x).dtype))
            if x.shape != flag.shape:
                raise ValueError("the field has shape %s, the flag %s" % (x.shape, flag.shape))
            if resident_gen is not None:
                raise ValueError("a field is given and the resident anomaly slab is named as well")
        f64 = x.dtype == np.float64 if x is not None else bool(resident_f64)
        call = _BandCall(T, ny, nx, rows, weights, sectors, columns, above, x is not None or resident_gen is not None, resident_gen)
        if int(chunk_steps) < 0:
            raise ValueError("chunk_steps=%d (at least 0)" % int(chunk_steps))
        fn = lib().ctk_band_f64 if f64 else lib().ctk_band_f32
        check(fn(self._h, flag.ctypes.data, _ptr(x), T, ny, nx, C.byref(call.spec), C.byref(call.out()), int(chunk_steps)))
        return call.arrays

    def band_cb(self, flag_reader, field_reader, shape, dtype, rows, weights, sectors=None, columns=True, above=0, chunk_steps=0, resident_gen=None):
        """the same with the slabs read chunk by chunk: flag_reader(t0, nt, out) fills an int32 (nt, ny, nx) view of pinned memory
        with the time steps [t0, t0 + nt), field_reader one of `dtype` (float32 / float64); the flag reader is called first.
        field_reader None: no field, or with resident_gen the resident anomaly slab of `dtype`."""
        T, ny, nx = (int(v) for v in shape)
        field = field_reader is not None or resident_gen is not None
        dt = np.dtype(dtype if dtype is not None else np.float32)
        if field and dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        if field_reader is not None and resident_gen is not None:
            raise ValueError("a field is given and the resident anomaly slab is named as well")
        call = _BandCall(T, ny, nx, rows, weights, sectors, columns, above, field, resident_gen)
        if int(chunk_steps) < 0:
            raise ValueError("chunk_steps=%d (at least 0)" % int(chunk_steps))
        tr = _Trampolines()
        fcb = tr.reader(flag_reader, C.c_int32, (ny, nx))
        xcb = tr.reader(field_reader, _float_ctype(dt) if field else C.c_float, (ny, nx))
        tr.finish(lib().ctk_band_cb(self._h, dt.itemsize, T, ny, nx, fcb, None, xcb, None, C.byref(call.spec), C.byref(call.out()), int(chunk_steps)))
        return call.arrays

    def band_dev(self, flag_dev, x_dev, T, ny, nx, rows, weights, sectors=None, columns=True, above=0, f64=False, resident_gen=None):
        """ctk_band_dev on an int32 flag and a float32 (f64: float64) field in device memory (x_dev None: no field, or with
        resident_gen the resident anomaly slab): the same dict of arrays"""
        field = x_dev is not None or resident_gen is not None
        call = _BandCall(T, ny, nx, rows, weights, sectors, columns, above, field, resident_gen)
        names = list(call.arrays)

        def run(*devs):
            out = call.out({n: (d.value if isinstance(d, C.c_void_p) else int(d)) for n, d in zip(names, devs)})
            check(lib().ctk_band_dev(self._h, flag_dev, x_dev, 8 if f64 else 4, call.T, call.ny, call.nx, C.byref(call.spec), C.byref(out)))
        self._download([call.arrays[n] for n in names], run)
        return call.arrays

    def debug_set_band(self, form=-1, rows=-1):
        """test hook for the following band launches: the form (0 the 16-byte form where it is legal, 1 the general form) and the
        widest batch of rows in flight; -1 the rule (ctk_band_plan)"""
        check(lib().ctk_debug_set_band(self._h, int(form), int(rows)))

    def debug_band_launch(self):
        """(form, widest batch of rows, workgroups) of the last band launch; form -1: none yet"""
        v = np.zeros(3, dtype=np.int64)
        check(lib().ctk_debug_band_launch(self._h, v.ctypes.data))
        return int(v[0]), int(v[1]), int(v[2])

    def time_band(self, flag_dev, x_dev, T, ny, nx, rows, weights, out_dev, sectors=None, columns=True, above=0, f64=False, reps=5):
        """k_band (with sectors: and k_band_sect) alone between HIP events; out_dev: name -> device address of the tables the request
        needs (cnt, area, wx, sec_cnt, sec_area, sec_wx): (best, mean) ms per launch"""
        call = _BandCall(T, ny, nx, rows, weights, sectors, columns, above, x_dev is not None)
        out = call.out({k: (v.value if isinstance(v, C.c_void_p) else int(v)) for k, v in out_dev.items()})
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_band(self._h, flag_dev, x_dev, 8 if f64 else 4, call.T, call.ny, call.nx, C.byref(call.spec), C.byref(out), int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- block-centred composite (the step after README.rst:198-228) --------------------------------------------------
    def centred(self, x, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, chunk_steps=0, resident_f64=False, shape=None):
        """(sum, n): for the stamps r in the order given (t non-decreasing) with bin[r] >= 0, sum[bin[r], j + hy, i + hx] += the
        float64 value of x[t[r], row[r] + j, col[r] + i] for j in -hy..hy, i in -hx..hx -- rows outside the grid not counted, columns
        wrapped (wrap) or not counted, with skipna NaN not counted -- and n how many there were, of a float32 / float64 (T, ny, nx)
        field in host memory (ctk_centred_f32 / _f64: chunks of `chunk_steps` time steps pass through the device, 0: about 256 MB
        each; chunks without stamps and latitude rows no window touches do not travel).  x None: the anomaly slab
        anomalies(keep_resident=True) left on the device (resident_f64: its type; shape: the (T, ny, nx) the caller expects of it,
        None: whatever it has).  bin None:
        one bin.  Returns float64 and uint32 (nbins, 2 hy + 1, 2 hx + 1)."""
        if x is None:
            f64 = bool(resident_f64)
            T, ny, nx = (int(v) for v in shape) if shape is not None else self.resident_anom_shape()
        else:
            x = np.asarray(x)
            if x.ndim != 3:
                raise ValueError("the field must be (time, lat, lon)")
            x = np.ascontiguousarray(x, dtype=_field_dtype(x.dtype))
            T, ny, nx = x.shape
            f64 = x.dtype == np.float64
        R, t, row, col, bin, nbins, hy, hx = _stamps(t, row, col, bin, nbins, hy, hx)
        s = np.empty((nbins, 2 * hy + 1, 2 * hx + 1), dtype=np.float64)
        n = np.empty(s.shape, dtype=np.uint32)
        fn = lib().ctk_centred_f64 if f64 else lib().ctk_centred_f32
        _check_composite(fn(self._h, _ptr(x), T, ny, nx, R, _ptr(t), _ptr(row), _ptr(col), _ptr(bin), nbins, hy, hx, int(bool(wrap)), int(bool(skipna)),
                            s.ctypes.data, n.ctypes.data, int(chunk_steps)))
        return s, n

    def resident_anom_shape(self):
        """(T, ny, nx) of the anomaly slab kept on the device; (1, 1, 1) when there is none (an entry that needs it then raises the
        library's state error)"""
        res = self.resident_anom()
        return (1, 1, 1) if res is None else res[:3]

    def centred_cb(self, field_reader, shape, dtype, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, chunk_steps=0):
        """the same with the field read chunk by chunk: field_reader(t0, nt, out) fills a (nt, ny, nx) view of pinned memory of
        `dtype` (float32 / float64) with the time steps [t0, t0 + nt); it is not called for a chunk none of whose steps carries a
        stamp with bin >= 0.  field_reader None: the resident anomaly slab of `dtype`."""
        T, ny, nx = (int(v) for v in shape)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        R, t, row, col, bin, nbins, hy, hx = _stamps(t, row, col, bin, nbins, hy, hx)
        s = np.empty((nbins, 2 * hy + 1, 2 * hx + 1), dtype=np.float64)
        n = np.empty(s.shape, dtype=np.uint32)
        tr = _Trampolines()
        xcb = tr.reader(field_reader, _float_ctype(dt), (ny, nx))
        tr.finish(lib().ctk_centred_cb(self._h, dt.itemsize, T, ny, nx, xcb, None, R, _ptr(t), _ptr(row), _ptr(col), _ptr(bin), nbins, hy, hx,
                                       int(bool(wrap)), int(bool(skipna)), s.ctypes.data, n.ctypes.data, int(chunk_steps)), _check_composite)
        return s, n

    def centred_dev(self, x_dev, T, ny, nx, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, f64=False, sum_dev=None, n_dev=None,
                    accumulate=False):
        """ctk_centred_*_dev on a float32 (f64: float64) field in device memory; x_dev None: the resident anomaly slab.  sum_dev /
        n_dev None: (sum, n) are returned; else they are written to (accumulate: continued from) those device buffers of nbins *
        (2 hy + 1) * (2 hx + 1) float64 / uint32 and None is returned."""
        R, t, row, col, bin, nbins, hy, hx = _stamps(t, row, col, bin, nbins, hy, hx)
        fn = lib().ctk_centred_f64_dev if f64 else lib().ctk_centred_f32_dev
        args = (self._h, x_dev, int(T), int(ny), int(nx), R, _ptr(t), _ptr(row), _ptr(col), _ptr(bin), nbins, hy, hx, int(bool(wrap)), int(bool(skipna)))
        if (sum_dev is None) != (n_dev is None):
            raise ValueError("sum_dev and n_dev go together")
        if sum_dev is not None:
            _check_composite(fn(*args, sum_dev, n_dev, int(bool(accumulate))))
            return None
        s = np.empty((nbins, 2 * hy + 1, 2 * hx + 1), dtype=np.float64)
        n = np.empty(s.shape, dtype=np.uint32)
        self._download([s, n], lambda ds, dn: _check_composite(fn(*args, ds, dn, 0)))
        return s, n

    def debug_set_centred(self, form=-1, unroll=-1, threads=-1):
        """test hook for the following centred launches: the form (0 plain, 1 fed) and, for the plain form, the widest batch of
        stamps and the cells per workgroup; -1 the rule (ctk_centred_plan)"""
        check(lib().ctk_debug_set_centred(self._h, int(form), int(unroll), int(threads)))

    def debug_centred_launch(self):
        """(form, batch, cells per workgroup, workgroups) of the last centred launch; (0, 0, 0, 0): none yet"""
        v = np.zeros(4, dtype=np.int64)
        check(lib().ctk_debug_centred_launch(self._h, v.ctypes.data))
        return int(v[3]), int(v[0]), int(v[1]), int(v[2])

    def time_centred(self, x_dev, T, ny, nx, t, row, col, bin, nbins, hy, hx, sum_dev, n_dev, wrap=True, skipna=False, f64=False, floor=False, reps=5):
        """the centred kernel alone (the rule's form, or the one debug_set_centred forces) between HIP events (sum_dev / n_dev: device buffers of nbins * (2 hy + 1) * (2 hx + 1) float64 / uint32):
        (best, mean) ms per launch.  floor: the plain unordered gather of the same windows instead, which keeps nothing"""
        R, t, row, col, bin, nbins, hy, hx = _stamps(t, row, col, bin, nbins, hy, hx)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_centred(self._h, x_dev, int(bool(f64)), int(T), int(ny), int(nx), R, _ptr(t), _ptr(row), _ptr(col), _ptr(bin), nbins, hy, hx,
                                           int(bool(wrap)), int(bool(skipna)), sum_dev, n_dev, int(bool(floor)), int(reps), ms))
        return float(ms[0]), float(ms[1])

    # ---- calc_anom / percentile threshold on the device ---------------------------------------------------------
    def anomalies(self, x, group, ngroups, window=1, smooth=1, clim=None, want_anom=True, want_clim=False, keep_resident=False, segments=None):
        """x (T, ny, nx) float32 / float64; group: T ids in [0, ngroups).  Returns (anom or None, clim or None).
        segments: None, or the first step of every independent time segment (0 first, strictly increasing, below T): the smoothing
        stays inside a segment (ctk_anom_seg_*); the climatology is pooled over all of them."""
        x = np.ascontiguousarray(x)
        f64 = x.dtype != np.float32
        if f64:
            x = np.ascontiguousarray(x, dtype=np.float64)
        T, ny, nx = x.shape
        group = _group_ids(group, T)
        cin = None if clim is None else np.ascontiguousarray(clim, dtype=x.dtype)
        if cin is not None and cin.shape != (ngroups, ny, nx):
            raise ValueError("clim must have shape (ngroups, ny, nx)")
        anom = np.empty_like(x) if want_anom else None
        cout = np.empty((ngroups, ny, nx), dtype=x.dtype) if want_clim else None
        args = (self._h, x.ctypes.data, T, ny, nx, group.ctypes.data, int(ngroups), int(window), int(smooth),
                None if cin is None else cin.ctypes.data, None if anom is None else anom.ctypes.data,
                None if cout is None else cout.ctypes.data, int(bool(keep_resident)))
        if segments is None:
            check((lib().ctk_anom_f64 if f64 else lib().ctk_anom_f32)(*args))
        else:
            st = _seg_starts(segments)
            check((lib().ctk_anom_seg_f64 if f64 else lib().ctk_anom_seg_f32)(*args, st.ctypes.data if st.size else None, st.shape[0]))
        return anom, cout

    def anomalies_stream(self, source, group, ngroups, window=1, smooth=1, clim=None, sink=None, shape=None, dtype=None, chunk_steps=0,
                         segments=None, want_clim=False):
        """anomalies(..., segments=...) with the slab passing through chunk-sized device buffers (ctk_anom_stream_*): the device holds
        a few chunks, 12 bytes per (group, pixel) and the climatology, never the slab.  Same bits as anomalies for every chunk_steps
        (0: about 256 MB per chunk; below smooth - 1 it is raised to smooth - 1).

        source: a (T, ny, nx) float32 / float64 array (np.memmap included), or a callable reader(t0, nt, out) that fills `out` (a
                (nt, ny, nx) view of pinned memory) with the timesteps [t0, t0 + nt) -- then `shape` = (T, ny, nx) and `dtype` are
                required.  It is read twice without `clim` (climatology, then anomalies), once with it; ranges never overlap.
        sink:   None (a new array of the slab's dtype is returned), False (no anomalies: the climatology only), an array (T, ny, nx)
                of the slab's dtype, or a callable writer(t0, nt, values) that receives each chunk as a (nt, ny, nx) view valid during
                the call, every step once in rising order.
        Returns (anom array or None, clim or None)."""
        L = lib()
        if callable(source):
            if shape is None or dtype is None:
                raise ValueError("a reader callback needs shape=(T, ny, nx) and dtype")
            T, ny, nx = (int(v) for v in shape)
            dt = np.dtype(dtype)
        else:
            source = _float_array(source, 3, "the slab must be (time, lat, lon)")
            T, ny, nx = source.shape
            dt = source.dtype
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the slab must be float32 or float64")
        group = _group_ids(group, T)
        cin = None if clim is None else np.ascontiguousarray(clim, dtype=dt)
        if cin is not None and cin.shape != (ngroups, ny, nx):
            raise ValueError("clim must have shape (ngroups, ny, nx)")
        cout = np.empty((ngroups, ny, nx), dtype=dt) if want_clim else None
        out, sink = _value_sink(sink, (T, ny, nx), dt, "T", "slab", "want_clim", cout is not None)
        st = _seg_starts(segments if segments is not None else [])
        mid = (group.ctypes.data, int(ngroups), int(window), int(smooth), st.ctypes.data if st.size else None, st.shape[0], _ptr(cin))
        if not callable(source) and not callable(sink):
            fn = L.ctk_anom_stream_f64 if dt == np.float64 else L.ctk_anom_stream_f32
            check(fn(self._h, source.ctypes.data, T, ny, nx, *mid, _ptr(sink), _ptr(cout), int(chunk_steps)))
            return out, cout
        tr = _Trampolines()
        rcb, wcb = tr.reader(source, _float_ctype(dt), (ny, nx)), tr.writer(sink, _float_ctype(dt), (ny, nx))
        tr.finish(L.ctk_anom_stream_cb(self._h, dt.itemsize, T, ny, nx, rcb, None, *mid, _ptr(cout), wcb, None, int(chunk_steps)))
        return out, cout

    # ---- vertical mean over the selected levels (ctk_level_mean_*) ------------------------------------------------
    def level_mean(self, x, weights, skipna=False, chunk_steps=None, keep_resident=False, want_out=True):
        """x (steps, nlev, ny, nx) float32 / float64 (an array or np.memmap); weights: nlev values >= 0, a level of weight 0 is not
        selected (never read, never uploaded).  Returns the (steps, ny, nx) mean in x's dtype (None without want_out):
        sum of w[l] * x[:, l] over the selected levels in rising l / sum of those w[l], in float64 (include/contrack_hip.h).
        skipna: a NaN level of a pixel leaves both sums.  chunk_steps: steps per chunk on their way through the device (None:
        ctk_level_mean_*, 0: about 256 MB of input); same bits.  keep_resident: the mean stays in HBM for anomalies_resident."""
        x = _float_array(x, 4, "x must be (steps, level, lat, lon)")
        steps, nlev, ny, nx = x.shape
        w = _level_weights(weights, nlev)
        if not want_out and not keep_resident:
            raise ValueError("want_out=False without keep_resident asks for nothing")
        out = np.empty((steps, ny, nx), dtype=x.dtype) if want_out else None
        f64 = x.dtype == np.float64
        head = (self._h, x.ctypes.data, steps, nlev, ny, nx, w.ctypes.data, int(bool(skipna)), _ptr(out))
        if chunk_steps is None:
            check((lib().ctk_level_mean_f64 if f64 else lib().ctk_level_mean_f32)(*head, int(bool(keep_resident))))
        else:
            check((lib().ctk_level_mean_stream_f64 if f64 else lib().ctk_level_mean_stream_f32)(*head, int(chunk_steps), int(bool(keep_resident))))
        return out

    def level_mean_cb(self, reader, shape_sel, dtype, weights_sel, skipna=False, sink=None, chunk_steps=0, keep_resident=False):
        """level_mean with a reader(t0, nt, out) that fills `out`, a (nt, nsel, ny, nx) view of pinned memory, with the SELECTED levels
        (rising level order) of the steps [t0, t0 + nt); shape_sel = (steps, nsel, ny, nx), weights_sel their nsel non-zero
        weights.  sink: None (a new array is returned), False (nothing leaves the device: keep_resident), a C-contiguous
        (steps, ny, nx) array of `dtype`, or a writer(t0, nt, values).  Reader and writer see every step once, in rising order."""
        def bind(dt, shape):
            steps, nsel, ny, nx = shape
            w = _level_weights(weights_sel, nsel)
            if np.any(w == 0):
                raise ValueError("a reader delivers the selected levels only: every weight must be > 0")
            return lambda rcb, wcb: lib().ctk_level_mean_stream_cb(self._h, dt.itemsize, steps, nsel, ny, nx, rcb, None, w.ctypes.data, int(bool(skipna)), wcb,
                                                                   None, int(chunk_steps or 0), int(bool(keep_resident)))
        return _values_cb(reader, shape_sel, "(steps, nsel, ny, nx)", dtype, bind, sink, keep_resident)

    def level_mean_dev(self, x_dev, steps, nlev, ny, nx, weights, out_dev, skipna=False, f64=False):
        """ctk_level_mean_*_dev: x (steps, nlev, ny, nx) and out (steps, ny, nx) in device memory"""
        w = _level_weights(weights, nlev)
        fn = lib().ctk_level_mean_f64_dev if f64 else lib().ctk_level_mean_f32_dev
        check(fn(self._h, x_dev, int(steps), int(nlev), int(ny), int(nx), w.ctypes.data, int(bool(skipna)), out_dev))

    def time_level_mean(self, x_dev, steps, nlev, ny, nx, weights, out_dev, skipna=False, f64=False, reps=5):
        """measurement (tools/level_probe.py): (best, mean) ms of k_level_mean alone on slabs in device memory, HIP events"""
        w = _level_weights(weights, nlev)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_level_mean(self._h, x_dev, int(bool(f64)), int(steps), int(nlev), int(ny), int(nx), w.ctypes.data, int(bool(skipna)),
                                              out_dev, int(reps), ms))
        return float(ms[0]), float(ms[1])

    def _debug_set(self, family, xcd, grid_max):
        """ctk_debug_set_<family> of the map families (level, reversal, subset, lwa, blockstat): both numbers hold for its following launches"""
        check(getattr(lib(), "ctk_debug_set_" + family)(self._h, int(xcd), int(grid_max)))

    def _debug_launch(self, family, n):
        """the n words ctk_debug_<family>_form of those families reports of the last launch"""
        v = np.zeros(n, dtype=np.int64)
        check(getattr(lib(), "ctk_debug_%s_form" % family)(self._h, v.ctypes.data))
        return tuple(int(a) for a in v)

    def debug_set_level(self, xcd=-1, grid_max=0):
        """for the following level_mean launches -- xcd: how workgroups map to XCDs (0 launch order, 1 one contiguous eighth per XCD,
        n > 1 tiles of n; -1: the library's rule, ctk_level_plan); grid_max: a lower cap on the workgroups of a launch (0: the rule's)"""
        self._debug_set("level", xcd, grid_max)

    def debug_level_form(self):
        """the form of the last level_mean launch: 1 vector (16 bytes per lane), 0 scalar, -1 none yet"""
        return self.debug_level_launch()[0]

    def debug_level_launch(self):
        """(form, workgroups) of the last level_mean launch"""
        return self._debug_launch("level", 2)

    def resident_level_mean(self):
        """(steps, ny, nx, is float64) of the vertical mean kept in HBM, or None"""
        T, ny, nx, f = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().ctk_resident_level_mean(self._h, C.byref(T), C.byref(ny), C.byref(nx), C.byref(f)))
        return None if T.value < 0 else (int(T.value), int(ny.value), int(nx.value), bool(f.value))

    def resident_level_mean_generation(self):
        """identity of the resident vertical mean (changes with every level_mean call and with release_io)"""
        g = C.c_uint64(0)
        check(lib().ctk_resident_level_mean_generation(self._h, C.byref(g)))
        return int(g.value)

    # ---- reversal of the meridional gradient (ctk_reversal_*) -----------------------------------------------------
    def reversal(self, x, rows, mask=False, chunk_steps=0, keep_resident=False, want_out=True):
        """x (steps, ny, nx) float32 / float64 (an array or np.memmap); rows: the row table (contrack.reversal_rows +
        reversal_limits: eq, po, dE, tS, tN and, for the third criterion, eq2 and tS2).  Returns the (steps, ny, nx) index in x's
        dtype (None without want_out): on active rows the equatorward gradient per degree where the pixel is blocked (mask: 1),
        0 elsewhere (include/contrack_hip.h).  chunk_steps: steps per chunk on their way through the device (0: about 256 MB of
        input); same bits.  keep_resident: the result stays in HBM as the field to track (track_resident)."""
        x = _float_array(x, 3, "x must be (steps, lat, lon)")
        steps, ny, nx = x.shape
        ptrs, _keep = _reversal_rows(rows, ny)
        if not want_out and not keep_resident:
            raise ValueError("want_out=False without keep_resident asks for nothing")
        out = np.empty((steps, ny, nx), dtype=x.dtype) if want_out else None
        fn = lib().ctk_reversal_f64 if x.dtype == np.float64 else lib().ctk_reversal_f32
        check(fn(self._h, x.ctypes.data, steps, ny, nx, *ptrs, int(bool(mask)), _ptr(out), int(chunk_steps or 0), int(bool(keep_resident))))
        return out

    def reversal_cb(self, reader, shape, dtype, rows, mask=False, sink=None, chunk_steps=0, keep_resident=False):
        """reversal with a reader(t0, nt, out) that fills `out`, a (nt, ny, nx) view of pinned memory, with the steps [t0, t0 + nt);
        shape = (steps, ny, nx).  sink: None (a new array is returned), False (nothing leaves the device: keep_resident), a
        C-contiguous (steps, ny, nx) array of `dtype`, or a writer(t0, nt, values).  Reader and writer see every step once, in
        rising order."""
        def bind(dt, shape):
            steps, ny, nx = shape
            ptrs, keep = _reversal_rows(rows, ny)
            return lambda rcb, wcb, _keep=keep: lib().ctk_reversal_stream_cb(self._h, dt.itemsize, steps, ny, nx, rcb, None, *ptrs, int(bool(mask)), wcb, None,
                                                                             int(chunk_steps or 0), int(bool(keep_resident)))
        return _values_cb(reader, shape, "(steps, ny, nx)", dtype, bind, sink, keep_resident)

    def reversal_dev(self, x_dev, steps, ny, nx, rows, out_dev, mask=False, f64=False):
        """ctk_reversal_*_dev: x and out (steps, ny, nx) in device memory"""
        ptrs, _keep = _reversal_rows(rows, ny)
        fn = lib().ctk_reversal_f64_dev if f64 else lib().ctk_reversal_f32_dev
        check(fn(self._h, x_dev, int(steps), int(ny), int(nx), *ptrs, int(bool(mask)), out_dev))

    def time_reversal(self, x_dev, steps, ny, nx, rows, out_dev, mask=False, f64=False, reps=5):
        """measurement (tools/reversal_probe.py): (best, mean) ms of k_reversal alone on slabs in device memory, HIP events; rows
        None: the plain copy kernel over the same two buffers, the yardstick"""
        ptrs, _keep = ([None] * 7, None) if rows is None else _reversal_rows(rows, ny)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_reversal(self._h, x_dev, int(bool(f64)), int(steps), int(ny), int(nx), *ptrs, int(bool(mask)), out_dev, int(reps), ms))
        return float(ms[0]), float(ms[1])

    def debug_set_reversal(self, xcd=-1, grid_max=0):
        """for the following reversal launches -- xcd: how workgroups map to XCDs (0 launch order, 1 one contiguous eighth per XCD,
        n > 1 tiles of n; -1: the library's rule, ctk_reversal_plan); grid_max: a lower cap on the workgroups of a launch (0: the
        rule's)"""
        self._debug_set("reversal", xcd, grid_max)

    def debug_reversal_form(self):
        """the form of the last reversal launch: 1 vector (16 bytes per lane), 0 scalar, -1 none yet"""
        return self.debug_reversal_launch()[0]

    def debug_reversal_launch(self):
        """(form, workgroups) of the last reversal launch"""
        return self._debug_launch("reversal", 2)

    # ---- selection of tracks or (step, track) rows of a flag slab (ctk_subset_*) -----------------------------------------
    def subset(self, flag, table, invert=False, kind='id', chunk_steps=0, want_out=True, want_hits=True):
        """flag (T, ny, nx) int32 host slab; table = (off, ids) (contrack.subset_table; include/contrack_hip.h states it).  Returns
        (out, hits, n_selected): the int32 selection -- flag where the pixel's id is in the step's slice (invert: where it is a
        positive id that is not), 0 elsewhere; kind='mask': 1 / 0 --, uint64 hits per entry of ids, the selected pixels.
        want_out=False: a count-only call, out is None and nothing is downloaded; want_hits=False: hits is None.  chunk_steps:
        steps per chunk on their way through the device (0: about 256 MB); same bytes."""
        flag = _flag_i32(flag, "subset_cb, or contrack.subset_numpy")
        T, ny, nx = flag.shape
        c = _SubsetCall(table, invert, kind, want_hits)
        out = np.empty((T, ny, nx), dtype=np.int32) if want_out else None
        check(lib().ctk_subset(self._h, flag.ctypes.data, T, ny, nx, *c.table, _ptr(out), *c.counts(), int(chunk_steps or 0)))
        return out, c.hits, int(c.n.value)

    def subset_cb(self, reader, shape, table, invert=False, kind='id', sink=None, chunk_steps=0, want_hits=True):
        """the same with a reader(t0, nt, out) that fills `out`, an int32 (nt, ny, nx) view of pinned memory, with the steps
        [t0, t0 + nt); shape = (T, ny, nx).  sink: None (a new array is returned), False (count only: no writer is called), a
        C-contiguous int32 (T, ny, nx) array, or a writer(t0, nt, values).  Returns (out or None, hits, n_selected)."""
        if shape is None:
            raise ValueError("a reader needs shape=(T, ny, nx)")
        T, ny, nx = (int(v) for v in shape)
        c = _SubsetCall(table, invert, kind, want_hits)
        out, sink = _value_sink(sink, (T, ny, nx), np.dtype(np.int32), "T", "flag", "the counts", True)
        tr = _Trampolines()
        rcb, wcb = tr.reader(reader, C.c_int32, (ny, nx)), tr.writer(sink, C.c_int32, (ny, nx))
        tr.finish(lib().ctk_subset_cb(self._h, T, ny, nx, rcb, None, *c.table, wcb, None, *c.counts(), int(chunk_steps or 0)))
        return out, c.hits, int(c.n.value)

    def subset_dev(self, flag_dev, T, ny, nx, table, out_dev, invert=False, kind='id', want_hits=True):
        """ctk_subset_dev: flag and out (T, ny, nx) int32 in device memory; out_dev None: count only, out_dev == flag_dev: in place.
        Returns (hits, n_selected)."""
        c = _SubsetCall(table, invert, kind, want_hits)
        check(lib().ctk_subset_dev(self._h, flag_dev, int(T), int(ny), int(nx), *c.table, out_dev, *c.counts()))
        return c.hits, int(c.n.value)

    def time_subset(self, flag_dev, T, ny, nx, table, out_dev, invert=False, kind='id', want_hits=False, want_n_selected=True, reps=5):
        """measurement (tools/subset_probe.py): (best, mean) ms of k_subset alone on slabs in device memory, HIP events; table None:
        the plain copy kernel over the same two buffers, the yardstick"""
        c = None if table is None else _SubsetCall(table, invert, kind, False)
        args = (None, 0, None, 0, 0, 0) if c is None else c.table
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_subset(self._h, flag_dev, int(T), int(ny), int(nx), *args, out_dev, int(bool(want_hits)), int(bool(want_n_selected)),
                                          int(reps), ms))
        return float(ms[0]), float(ms[1])

    def debug_set_subset(self, xcd=-1, grid_max=0):
        """for the following subset launches -- xcd: how workgroups map to XCDs (0 launch order, 1 one contiguous eighth per XCD,
        n > 1 tiles of n; -1: the library's rule, ctk_subset_plan); grid_max: a lower cap on the workgroups of a launch (0: the
        rule's)"""
        self._debug_set("subset", xcd, grid_max)

    def debug_subset_launch(self):
        """(form, vec, workgroups) of the last subset launch: form 0 .. 4 = SUBSET_FORMS (-1: none yet), vec 1 vector / 0 scalar"""
        return self._debug_launch("subset", 3)

    # ---- per-block peak and extent (ctk_blockstat_*) ---------------------------------------------------------------------
    def blockstat(self, flag, table, x=None, want=('shape', 'peaks'), chunk_steps=0, resident_f64=False):
        """flag (T, ny, nx) int32 host slab, table = (off, ids) a ROW table (contrack.subset_table(ids, steps, T)), x a float32 /
        float64 field of the flag's shape.  Returns a structured array (BLOCK_ROW = ctk_block_row of include/contrack_hip.h, which
        states every field), one row per entry of ids.  x None with 'peaks': the anomaly slab anomalies(keep_resident=True) left on
        the device (resident_f64: its type), only the flags travel.  chunk_steps: steps per chunk on their way through the device
        (0: about 256 MB); same bytes."""
        flag = _flag_i32(flag, "blockstat_cb, or contrack.blockstat_numpy")
        T, ny, nx = flag.shape
        if x is None:
            f64 = bool(resident_f64)
        else:
            x = np.ascontiguousarray(x, dtype=_field_dtype(np.asarray(x).dtype))
            if x.shape != flag.shape:
                raise ValueError("the field has shape %s, the flag %s" % (x.shape, flag.shape))
            f64 = x.dtype == np.float64
        c = _BlockstatCall(table, want)
        fn = lib().ctk_blockstat_f64 if f64 else lib().ctk_blockstat_f32
        check(fn(self._h, flag.ctypes.data, _ptr(x), T, ny, nx, *c.args, int(chunk_steps or 0)))
        return c.rows

    def blockstat_cb(self, flag_reader, field_reader, shape, dtype, table, want=('shape', 'peaks'), chunk_steps=0):
        """the same with both slabs read chunk by chunk: flag_reader(t0, nt, out) fills an int32 (nt, ny, nx) view of pinned memory
        with the steps [t0, t0 + nt), field_reader one of `dtype` (float32 / float64); the flag reader is called first.  Readers may
        be arrays indexed by time.  field_reader None: the resident anomaly slab of `dtype`, or (without 'peaks') no field."""
        if shape is None:
            raise ValueError("a reader needs shape=(T, ny, nx)")
        T, ny, nx = (int(v) for v in shape)
        dt = np.dtype(np.float32 if dtype is None else dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        c = _BlockstatCall(table, want)
        tr = _Trampolines()
        fcb, xcb = tr.reader(flag_reader, C.c_int32, (ny, nx)), tr.reader(field_reader, _float_ctype(dt), (ny, nx))
        tr.finish(lib().ctk_blockstat_cb(self._h, dt.itemsize, T, ny, nx, fcb, None, xcb, None, *c.args, int(chunk_steps or 0)))
        return c.rows

    def blockstat_dev(self, flag_dev, x_dev, T, ny, nx, table, want=('shape', 'peaks'), f64=False):
        """ctk_blockstat_*_dev on an int32 flag and a float32 (f64: float64) field in device memory; x_dev None: the resident
        anomaly slab, or (without 'peaks') no field.  Returns the rows."""
        c = _BlockstatCall(table, want)
        fn = lib().ctk_blockstat_f64_dev if f64 else lib().ctk_blockstat_f32_dev
        check(fn(self._h, flag_dev, x_dev, int(T), int(ny), int(nx), *c.args))
        return c.rows

    def time_blockstat(self, flag_dev, x_dev, T, ny, nx, table, want=('shape', 'peaks'), f64=False, reps=5):
        """measurement (tools/blockstat_probe.py): (best, mean) ms of the k_blockstat launches of the whole slab alone on slabs in
        device memory, HIP events; table None: the plain stream of 16-byte loads over the same buffers, the yardstick"""
        ms = (C.c_double * 2)()
        if table is None:
            args = (None, 0, None, 0, 0)
        else:
            c = _BlockstatCall(table, want)
            args = c.args[:5]
        check(lib().ctk_debug_time_blockstat(self._h, flag_dev, x_dev, int(bool(f64)), int(T), int(ny), int(nx), *args, int(reps), ms))
        return float(ms[0]), float(ms[1])

    def debug_set_blockstat(self, xcd=-1, grid_max=0):
        """for the following blockstat launches -- xcd: how workgroups map to XCDs (0 launch order, 1 one contiguous eighth per XCD,
        n > 1 tiles of n; -1: the library's rule, ctk_blockstat_plan); grid_max: a lower cap on the workgroups of a launch (0: the
        rule's)"""
        self._debug_set("blockstat", xcd, grid_max)

    def debug_blockstat_launch(self):
        """(form, vec, workgroups) of the last blockstat launch: form 0 / 1 = BLOCKSTAT_FORMS (-1: none yet), vec 1 vector / 0 scalar"""
        return self._debug_launch("blockstat", 3)

    # ---- local wave activity (ctk_lwa_*) ---------------------------------------------------------------------------
    def lwa(self, x, rows, part='total', chunk_steps=0, keep_resident=False, want_out=True, want_ref=False):
        """x (steps, ny, nx) float32 / float64 (an array or np.memmap), a height field that falls towards the pole; rows: the row
        table (contrack.lwa_rows: dom_off, dom_rows, active, W, q, S).  Returns the (steps, ny, nx) local wave activity in x's
        dtype (None without want_out) -- part 'total' / 0, 'anticyclonic' / 1 or 'cyclonic' / 2; 0 on inactive rows
        (include/contrack_hip.h) -- and, with want_ref, (that, ref): ref (steps, ny) the equivalent-latitude contours.
        chunk_steps: steps per chunk on their way through the device (0: about 256 MB of input); same bits.  keep_resident: the
        result stays in HBM as the field to track (track_resident)."""
        x = _float_array(x, 3, "x must be (steps, lat, lon)")
        steps, ny, nx = x.shape
        args, _keep = _lwa_rows(rows, ny)
        if not want_out and not keep_resident:
            raise ValueError("want_out=False without keep_resident asks for nothing")
        out = np.empty((steps, ny, nx), dtype=x.dtype) if want_out else None
        ref = np.empty((steps, ny), dtype=x.dtype) if want_ref else None
        fn = lib().ctk_lwa_f64 if x.dtype == np.float64 else lib().ctk_lwa_f32
        check(fn(self._h, x.ctypes.data, steps, ny, nx, *args, _lwa_part(part), _ptr(out), _ptr(ref), int(chunk_steps or 0), int(bool(keep_resident))))
        return (out, ref) if want_ref else out

    def lwa_cb(self, reader, shape, dtype, rows, part='total', sink=None, chunk_steps=0, keep_resident=False, want_ref=False):
        """lwa with a reader(t0, nt, out) that fills `out`, a (nt, ny, nx) view of pinned memory, with the steps [t0, t0 + nt);
        shape = (steps, ny, nx).  sink: None (a new array is returned), False (nothing leaves the device: keep_resident), a
        C-contiguous (steps, ny, nx) array of `dtype`, or a writer(t0, nt, values).  Reader and writer see every step once, in
        rising order.  want_ref: returns (the array or None, ref)."""
        ref = None

        def bind(dt, shape):
            nonlocal ref
            steps, ny, nx = shape
            args, keep = _lwa_rows(rows, ny)
            ref = np.empty((steps, ny), dtype=dt) if want_ref else None
            return lambda rcb, wcb, _keep=keep: lib().ctk_lwa_stream_cb(self._h, dt.itemsize, steps, ny, nx, rcb, None, *args, _lwa_part(part), wcb, None, _ptr(ref),
                                                                        int(chunk_steps or 0), int(bool(keep_resident)))
        out = _values_cb(reader, shape, "(steps, ny, nx)", dtype, bind, sink, keep_resident)
        return (out, ref) if want_ref else out

    def lwa_dev(self, x_dev, steps, ny, nx, rows, out_dev, part='total', f64=False, want_ref=False):
        """ctk_lwa_*_dev: x and out (steps, ny, nx) in device memory; want_ref: returns the contours (steps, ny) on the host"""
        args, _keep = _lwa_rows(rows, ny)
        ref = np.empty((int(steps), int(ny)), dtype=np.float64 if f64 else np.float32) if want_ref else None
        fn = lib().ctk_lwa_f64_dev if f64 else lib().ctk_lwa_f32_dev
        check(fn(self._h, x_dev, int(steps), int(ny), int(nx), *args, _lwa_part(part), out_dev, _ptr(ref)))
        return ref

    def time_lwa(self, x_dev, steps, ny, nx, rows, out_dev, stage, part='total', f64=False, reps=5):
        """measurement (tools/lwa_probe.py): (best, mean) ms of one stage alone on 16-byte aligned slabs in device memory, HIP
        events -- stage 1 the contours, 2 the integrals, 0 the plain copy kernel over the same two buffers (rows may be None)"""
        args, _keep = ([1] + [None] * 6, None) if rows is None else _lwa_rows(rows, ny)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_lwa(self._h, x_dev, int(bool(f64)), int(steps), int(ny), int(nx), *args, _lwa_part(part), out_dev, int(stage), int(reps), ms))
        return float(ms[0]), float(ms[1])

    def debug_set_lwa(self, xcd=-1, grid_max=0):
        """for the following lwa launches (both kernels) -- xcd: how workgroups map to XCDs (0 launch order, 1 one contiguous eighth
        per XCD, n > 1 tiles of n; -1: the library's rule, ctk_lwa_plan); grid_max: a lower cap on the workgroups of a launch (0:
        the rule's)"""
        self._debug_set("lwa", xcd, grid_max)

    def debug_lwa_form(self):
        """the form of the last lwa launch: 1 vector (16-byte loads of the strip), 0 scalar, -1 none yet"""
        return self.debug_lwa_launch()[0]

    def debug_lwa_launch(self):
        """(form, workgroups) of the last k_lwa_integral launch"""
        return self._debug_launch("lwa", 2)

    def anomalies_resident(self, group, ngroups, window=1, smooth=1, clim=None, segments=None, keep_resident=False, want_anom=True, want_clim=False):
        """anomalies(..., segments=...) of the resident vertical mean (ctk_anom_seg_resident): nothing crosses PCIe on the way in.
        Returns (anom or None, clim or None) in the mean's dtype; raises if no mean is resident."""
        shape = self.resident_level_mean()
        if shape is None:
            raise ContrackHipError("no vertical mean is resident on the device")
        T, ny, nx, f64 = shape
        dt = np.float64 if f64 else np.float32
        group = _group_ids(group, T)
        cin = None if clim is None else np.ascontiguousarray(clim, dtype=dt)
        if cin is not None and cin.shape != (ngroups, ny, nx):
            raise ValueError("clim must have shape (ngroups, ny, nx)")
        anom = np.empty((T, ny, nx), dtype=dt) if want_anom else None
        cout = np.empty((ngroups, ny, nx), dtype=dt) if want_clim else None
        st = _seg_starts(segments if segments is not None else [])
        check(lib().ctk_anom_seg_resident(self._h, group.ctypes.data, int(ngroups), int(window), int(smooth), _ptr(cin), _ptr(anom), _ptr(cout),
                                          int(bool(keep_resident)), st.ctypes.data if st.size else None, st.shape[0]))
        return anom, cout

    def debug_anom_form(self):
        """the kernel form of the last anomalies(segments=...) / anomalies_stream launch: 1 LDS ring, 0 plain, -1 none yet"""
        v = C.c_int64(0)
        check(lib().ctk_debug_anom_form(self._h, C.byref(v)))
        return int(v.value)

    def debug_set_anom(self, waves_wanted=0, grid_y_max=0):
        """for the following anomalies(segments=...) / anomalies_stream / anomalies_resident launches: ctk_anom_plan's waves_wanted and
        grid_y_max (0: the rule's), so that a small slab reaches the tile edges"""
        check(lib().ctk_debug_set_anom(self._h, int(waves_wanted), int(grid_y_max)))

    def debug_anom_launch(self):
        """dict of the last anomaly launch (form, tile, gx, gy, lds, o0, o1) and `launches`, their number in the last call"""
        v = np.zeros(8, dtype=np.int64)
        check(lib().ctk_debug_anom_launch(self._h, v.ctypes.data))
        return dict(zip(("form", "tile", "gx", "gy", "lds", "o0", "o1", "launches"), (int(a) for a in v)))

    # ---- weighted filter / block mean along time (ctk_filter_*) ----------------------------------------------------
    @staticmethod
    def _filter_args(T, weights, stride, offset, edges, skipna, segments):
        """(the arguments from w to nseg of the ctk_filter_* entries, T_out, what must stay alive during the call)"""
        w, K = _filter_weights(weights)
        if edges not in FILTER_EDGES:
            raise ValueError("edges must be 'nan' or 'renorm'")
        st = _seg_starts(segments if segments is not None else [])
        off = filter_offset(K, int(stride), offset)
        n = C.c_int64(0)
        check(lib().ctk_filter_layout(int(T), K, int(stride), off, st.ctypes.data if st.size else None, st.shape[0], None, None, C.byref(n)))
        return (_ptr(w), K, int(stride), off, FILTER_EDGES[edges], int(bool(skipna)), st.ctypes.data if st.size else None, st.shape[0]), int(n.value), (w, st)

    def time_filter(self, x, weights, stride=1, offset=None, edges="nan", skipna=False, segments=None, chunk_steps=None, keep_resident=False, want_out=True,
                    out=None):
        """x (T, ny, nx) float32 / float64 (an array or np.memmap); weights: K taps, or an int K (box mode: the mean of K steps).
        Output q of a segment has its taps at the steps S + offset + q * stride + (0 .. K - 1) and exists where its label step
        (tap K // 2) lies in the segment; offset None: -(K // 2) at stride 1 (one output per step, centred), 0 otherwise (blocks from
        the segment start).  Taps outside the segment: edges 'nan' gives NaN, 'renorm' divides by the sum of the used weights;
        skipna: a NaN tap is left out the same way (include/contrack_hip.h).  Returns the (T_out, ny, nx) result in x's dtype (None
        without want_out).  chunk_steps: steps per chunk on their way through the device (None / 0: about 256 MB); same bits.
        keep_resident: the result stays in HBM in the level-mean slot, for anomalies_resident / time_filter_resident.
        out: a C-contiguous (T_out, ny, nx) array of x's dtype to write into instead of a new one."""
        x = _float_array(x, 3, "x must be (time, lat, lon)")
        T, ny, nx = x.shape
        if not want_out and not keep_resident:
            raise ValueError("want_out=False without keep_resident asks for nothing")
        mid, T_out, _keep = self._filter_args(T, weights, stride, offset, edges, skipna, segments)
        if out is not None and (not want_out or out.dtype != x.dtype or out.shape != (T_out, ny, nx) or not out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous (T_out, ny, nx) = (%d, %d, %d) array of x's dtype" % (T_out, ny, nx))
        if out is None:
            out = np.empty((T_out, ny, nx), dtype=x.dtype) if want_out else None
        fn = lib().ctk_filter_f64 if x.dtype == np.float64 else lib().ctk_filter_f32
        check(fn(self._h, x.ctypes.data, T, ny, nx, *mid, _ptr(out), T_out, int(chunk_steps or 0), int(bool(keep_resident))))
        return out

    def time_filter_cb(self, reader, shape, dtype, weights, stride=1, offset=None, edges="nan", skipna=False, segments=None, sink=None, chunk_steps=0,
                       keep_resident=False):
        """time_filter with a reader(t0, nt, out) that fills `out`, a (nt, ny, nx) view of pinned memory, with the steps [t0, t0 + nt);
        shape = (T, ny, nx).  sink: None (a new array is returned), False (nothing leaves the device: keep_resident), a C-contiguous
        (T_out, ny, nx) array of `dtype`, or a writer(t0, nt, values) of outputs.  The reader sees every step once, in rising order."""
        if shape is None or dtype is None:
            raise ValueError("a reader needs shape=(T, ny, nx) and dtype")
        T, ny, nx = (int(v) for v in shape)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        mid, T_out, _keep = self._filter_args(T, weights, stride, offset, edges, skipna, segments)
        out, sink = _value_sink(sink, (T_out, ny, nx), dt, "T_out", "field", "keep_resident", keep_resident)
        tr = _Trampolines()
        rcb, wcb = tr.reader(reader, _float_ctype(dt), (ny, nx)), tr.writer(sink, _float_ctype(dt), (ny, nx))
        tr.finish(lib().ctk_filter_stream_cb(self._h, dt.itemsize, T, ny, nx, rcb, None, *mid, wcb, None, T_out, int(chunk_steps or 0), int(bool(keep_resident))))
        return out

    def time_filter_resident(self, weights, stride=1, offset=None, edges="nan", skipna=False, segments=None, keep_resident=False, want_out=True):
        """time_filter of the resident level mean (ctk_filter_resident): nothing crosses PCIe on the way in.  Returns the result in the
        mean's dtype (None without want_out); keep_resident: it replaces the mean in the slot.  Raises if no mean is resident."""
        shape = self.resident_level_mean()
        if shape is None:
            raise ContrackHipError("no vertical mean is resident on the device")
        T, ny, nx, f64 = shape
        if not want_out and not keep_resident:
            raise ValueError("want_out=False without keep_resident asks for nothing")
        mid, T_out, _keep = self._filter_args(T, weights, stride, offset, edges, skipna, segments)
        out = np.empty((T_out, ny, nx), dtype=np.float64 if f64 else np.float32) if want_out else None
        check(lib().ctk_filter_resident(self._h, *mid, _ptr(out), T_out, int(bool(keep_resident))))
        return out

    def time_filter_dev(self, x_dev, T, ny, nx, weights, out_dev, stride=1, offset=None, edges="nan", skipna=False, segments=None, f64=False):
        """ctk_filter_*_dev: x (T, ny, nx) and out (T_out, ny, nx) in device memory; returns T_out"""
        mid, T_out, _keep = self._filter_args(T, weights, stride, offset, edges, skipna, segments)
        check((lib().ctk_filter_f64_dev if f64 else lib().ctk_filter_f32_dev)(self._h, x_dev, int(T), int(ny), int(nx), *mid, out_dev, T_out))
        return T_out

    def time_filter_kernel(self, x_dev, T, ny, nx, weights, out_dev, stride=1, offset=None, edges="nan", skipna=False, f64=False, copy_bytes=0, reps=5):
        """measurement (tools/filter_probe.py): (best, mean) ms of the filter kernel alone on slabs in device memory, HIP events;
        copy_bytes > 0: of the plain 16-byte copy kernel over that many bytes of the two buffers instead"""
        mid, T_out, _keep = self._filter_args(T, weights, stride, offset, edges, skipna, None)
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_filter(self._h, x_dev, int(bool(f64)), int(T), int(ny), int(nx), *mid[:6], out_dev, T_out, int(copy_bytes), int(reps), ms))
        return float(ms[0]), float(ms[1])

    def debug_set_filter(self, waves_wanted=0, grid_y_max=0, forced=-1):
        """for the following time_filter launches: ctk_filter_plan's waves_wanted and grid_y_max (0: the rule's) and the form (1 LDS ring
        where one fits, 0 plain, -1 the rule's), so that a small slab reaches every form and tile edge"""
        check(lib().ctk_debug_set_filter(self._h, int(waves_wanted), int(grid_y_max), int(forced)))

    def debug_filter_launch(self):
        """dict of the last time-filter launch (form, threads, tile, gx, gy, lds, o0, o1) and `launches`, their number in the last call"""
        v = np.zeros(9, dtype=np.int64)
        check(lib().ctk_debug_filter_launch(self._h, v.ctypes.data))
        return dict(zip(("form", "threads", "tile", "gx", "gy", "lds", "o0", "o1", "launches"), (int(a) for a in v)))

    def resident_anom(self):
        T, ny, nx, f = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().ctk_resident_anom(self._h, C.byref(T), C.byref(ny), C.byref(nx), C.byref(f)))
        return None if T.value < 0 else (int(T.value), int(ny.value), int(nx.value), bool(f.value))

    def resident_generation(self):
        """identity of the resident anomaly slab (changes whenever one is written or dropped)"""
        g = C.c_uint64(0)
        check(lib().ctk_resident_anom_generation(self._h, C.byref(g)))
        return int(g.value)

    def track_resident(self, thr, cmp_op, wrow, overlap, persistence, twosided=True):
        shape = self.resident_anom()
        if shape is None:
            raise ContrackHipError("no anomaly slab is resident on the device")
        T, ny, nx, _ = shape
        thr = _thr_or_field(thr, T)
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        flag = self._pool.take((T, ny, nx))
        n = C.c_int64(0)
        check(lib().ctk_track_resident(self._h, _ptr(thr), int(cmp_op), wrow.ctypes.data, float(overlap), int(persistence),
                                       int(bool(twosided)), flag.ctypes.data, C.byref(n)))
        return flag, int(n.value)

    def _slab_or_resident(self, x):
        """(pointer, T, ny, nx, is float64, the array the pointer points into) of a host slab -- made C-contiguous, float32 kept,
        anything else as float64 --, or of the resident anomaly slab (x None: pointer NULL)"""
        if x is None:
            shape = self.resident_anom()
            if shape is None:
                raise ContrackHipError("no anomaly slab is resident on the device")
            return (None,) + shape + (None,)
        x = np.ascontiguousarray(x)
        if x.ndim != 3:
            raise ValueError("x must be (time, lat, lon)")
        f64 = x.dtype != np.float32
        if f64:
            x = np.ascontiguousarray(x, dtype=np.float64)
        return (x.ctypes.data,) + x.shape + (f64, x)

    def percentile(self, x, y0, y1, q):
        """mean over rows [y0, y1) of the per-grid-point q-quantile over time; x = None: the resident anomaly slab"""
        out = C.c_double(0.0)
        ptr, T, ny, nx, f64, _keep = self._slab_or_resident(x)
        fn = lib().ctk_percentile_f64 if f64 else lib().ctk_percentile_f32
        check(fn(self._h, ptr, T, ny, nx, int(y0), int(y1), float(q), C.byref(out)))
        return float(out.value)

    def percentile_groups(self, x, y0, y1, group, ngroups, q, window=1):
        """per group g the exact q-quantile (np.nanquantile, 'linear', float64) of rows [y0, y1) pooled over every timestep whose
        group lies in the centred, circular window of `window` groups around g (ctk_percentile_groups_*); x (T, ny, nx) float32 /
        float64, or None: the resident anomaly slab.  group: T ids in [0, ngroups).  Returns float64 (ngroups,)."""
        ptr, T, ny, nx, f64, _keep = self._slab_or_resident(x)
        group = _group_ids(group, T)
        out = np.empty(int(ngroups), dtype=np.float64)
        fn = lib().ctk_percentile_groups_f64 if f64 else lib().ctk_percentile_groups_f32
        check(fn(self._h, ptr, T, ny, nx, int(y0), int(y1), group.ctypes.data, int(ngroups), int(window), float(q), out.ctypes.data))
        return out

    def debug_percentile_groups_state(self, ngroups):
        """test hook: (nu_day uint32, need uint32, n_of uint64), ngroups entries each, of the last percentile_groups() call"""
        nu, need, n = np.zeros(ngroups, np.uint32), np.zeros(ngroups, np.uint32), np.zeros(ngroups, np.uint64)
        check(lib().ctk_debug_percentile_groups_state(self._h, int(ngroups), nu.ctypes.data, need.ctypes.data, n.ctypes.data))
        return nu, need, n

    def debug_percentile_groups_sweeps(self):
        """test hook: band reads of the last percentile_groups() call"""
        n = C.c_int64(0)
        check(lib().ctk_debug_percentile_groups_sweeps(self._h, C.byref(n)))
        return int(n.value)

    def time_percentile_groups(self, x_dev, T, ny, nx, y0, y1, group, ngroups, q, window=1, reps=3):
        """measurement on a float32 slab in device memory (tools/pctl_probe.py): (values, ms per call, ms of one plain read of the
        band, ms of the scalar percentile's kernels, ms of every band sweep of one call)"""
        group = np.ascontiguousarray(group, dtype=np.int32)
        out = np.empty(int(ngroups), dtype=np.float64)
        ms = (C.c_double * 12)()
        check(lib().ctk_debug_time_percentile_groups(self._h, x_dev, int(T), int(ny), int(nx), int(y0), int(y1), group.ctypes.data, int(ngroups),
                                                     int(window), float(q), int(reps), out.ctypes.data, ms))
        return out, float(ms[0]), float(ms[1]), float(ms[2]), [float(v) for v in ms[3:3 + self.debug_percentile_groups_sweeps()]]

    def percentile_field(self, x, y0, y1, group, ngroups, q, window=1):
        """per group g and grid point of rows [y0, y1) the exact q-quantile (np.nanquantile, 'linear', float64) over every timestep
        whose group lies in the centred, circular window of `window` groups around g (ctk_percentile_field_*); x (T, ny, nx)
        float32 / float64, or None: the resident anomaly slab.  group: T ids in [0, ngroups).  Returns float64
        (ngroups, y1 - y0, nx)."""
        ptr, T, ny, nx, f64, _keep = self._slab_or_resident(x)
        group = _group_ids(group, T)
        out = np.empty((max(int(ngroups), 0), max(int(y1) - int(y0), 0), nx), dtype=np.float64)
        fn = lib().ctk_percentile_field_f64 if f64 else lib().ctk_percentile_field_f32
        check(fn(self._h, ptr, T, ny, nx, int(y0), int(y1), group.ctypes.data, int(ngroups), int(window), float(q), out.ctypes.data))
        return out

    def debug_percentile_field_form(self):
        """test hook: (form, longest pool in timesteps) of the last percentile_field() call; form 0 direct, 1 ring, -1 none yet"""
        v = np.zeros(2, dtype=np.int64)
        check(lib().ctk_debug_percentile_field_form(self._h, v.ctypes.data))
        return int(v[0]), int(v[1])

    def time_percentile_field(self, x_dev, T, ny, nx, y0, y1, group, ngroups, q, window=1, reps=3, f64=False, want_fields=True):
        """measurement on a slab in device memory (tools/pfield_probe.py): (field of the chosen form, field of the direct form
        forced -- both None without want_fields --, ms per call of the chosen form, ms of the direct form, ms of one plain read
        of the band, the chosen form)"""
        group = np.ascontiguousarray(group, dtype=np.int32)
        shape = (int(ngroups), int(y1) - int(y0), int(nx))
        a = np.empty(shape, dtype=np.float64) if want_fields else None
        b = np.empty(shape, dtype=np.float64) if want_fields else None
        ms = (C.c_double * 4)()
        check(lib().ctk_debug_time_percentile_field(self._h, x_dev, int(bool(f64)), int(T), int(ny), int(nx), int(y0), int(y1), group.ctypes.data,
                                                    int(ngroups), int(window), float(q), int(reps), _ptr(a), _ptr(b), ms))
        return a, b, float(ms[0]), float(ms[1]), float(ms[2]), int(ms[3])

    def std_field(self, x, y0, y1, group, ngroups, window=1, ddof=0, skipna=True, want_mean=False, want_n=False):
        """per group g and grid point of rows [y0, y1) the standard deviation over every timestep whose group lies in the centred,
        circular window of `window` groups around g, taken in time order: the two-pass float64 loop of ctk_std_field_*
        (include/contrack_hip.h; np.nanstd / np.std of the pool with `ddof` on planes of two or more points; NaN where
        count - ddof <= 0); x (T, ny, nx) float32 / float64, or None: the resident anomaly slab.  group: T ids in [0, ngroups).
        Returns float64 (ngroups, y1 - y0, nx) -- with want_mean / want_n a tuple (std, mean float64 or None, count uint32 or None)."""
        ptr, T, ny, nx, f64, _keep = self._slab_or_resident(x)
        group = _group_ids(group, T)
        shape = (max(int(ngroups), 0), max(int(y1) - int(y0), 0), nx)
        out = np.empty(shape, dtype=np.float64)
        mean = np.empty(shape, dtype=np.float64) if want_mean else None
        n = np.empty(shape, dtype=np.uint32) if want_n else None
        fn = lib().ctk_std_field_f64 if f64 else lib().ctk_std_field_f32
        check(fn(self._h, ptr, T, ny, nx, int(y0), int(y1), group.ctypes.data, int(ngroups), int(window), int(ddof), int(bool(skipna)),
                 out.ctypes.data, _ptr(mean), _ptr(n)))
        return (out, mean, n) if want_mean or want_n else out

    def debug_std_field_form(self):
        """test hook: (pixels per workgroup, longest pool in timesteps) of the last std_field() call; tile -1: none yet"""
        v = np.zeros(2, dtype=np.int64)
        check(lib().ctk_debug_std_field_form(self._h, v.ctypes.data))
        return int(v[0]), int(v[1])

    def time_std_field(self, x_dev, T, ny, nx, y0, y1, group, ngroups, window=1, ddof=0, skipna=True, reps=3, f64=False, want_field=True):
        """measurement on a slab in device memory (tools/std_probe.py): (the field or None, ms per call, pixels per workgroup)"""
        group = np.ascontiguousarray(group, dtype=np.int32)
        a = np.empty((int(ngroups), int(y1) - int(y0), int(nx)), dtype=np.float64) if want_field else None
        ms = (C.c_double * 2)()
        check(lib().ctk_debug_time_std_field(self._h, x_dev, int(bool(f64)), int(T), int(ny), int(nx), int(y0), int(y1), group.ctypes.data,
                                             int(ngroups), int(window), int(ddof), int(bool(skipna)), int(reps), _ptr(a), ms))
        return a, float(ms[0]), int(ms[1])

    def debug_percentile_values(self, n):
        """test hook: the n per-grid-point quantiles (band, row-major) of the last percentile() call"""
        v = np.empty(int(n), dtype=np.float64)
        check(lib().ctk_debug_percentile_values(self._h, v.ctypes.data, int(n)))
        return v

    def debug_io_bytes(self):
        """test hook: the capacities in bytes of the staging buffers the entries share, as a dict: io_in, io_out, and one buffer of the
        pinned pairs pin_in, pin_out (0: not allocated)"""
        v = np.zeros(4, dtype=np.int64)
        check(lib().ctk_debug_io_bytes(self._h, v.ctypes.data))
        return dict(zip(("io_in", "io_out", "pin_in", "pin_out"), (int(b) for b in v)))

    def release_io(self):
        """free the device copies of slab / result that the host-array calls keep in the handle"""
        check(lib().ctk_release_io(self._h))

    # ---- threshold field (ctk_set_threshold_field) ----------------------------------------------------------------
    def set_threshold_field(self, field, plane_of_step):
        """threshold per grid point for the following calls with thr=None: field (nplanes, ny, nx), step t compared with
        field[plane_of_step[t]].  float32 stays float32; float16 and integers of up to 16 bits are exact in float32 and become it
        (numpy compares a float32 slab with them in float32); every other dtype becomes float64 (numpy compares in float64)."""
        field = np.asarray(field)
        if field.ndim != 3:
            raise ValueError("the threshold field must be (nplanes, ny, nx)")
        if field.dtype.kind not in "fiub":
            raise TypeError("the threshold field must be numeric")
        small = field.dtype == np.float16 or (field.dtype.kind in "iub" and field.dtype.itemsize <= 2)
        field = np.ascontiguousarray(field, dtype=np.float32 if (field.dtype == np.float32 or small) else np.float64)
        pos = np.asarray(plane_of_step)
        if pos.ndim != 1 or pos.dtype.kind not in "iu":
            raise ValueError("plane_of_step must be a 1-D integer array")
        if pos.size and (pos.min() < 0 or pos.max() >= field.shape[0]):
            raise ValueError("plane_of_step must index the field's planes")
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        check(lib().ctk_set_threshold_field(self._h, field.ctypes.data, field.itemsize, field.shape[0], field.shape[1], field.shape[2],
                                            pos.ctypes.data, pos.shape[0]))

    def clear_threshold_field(self):
        check(lib().ctk_set_threshold_field(self._h, None, 4, 0, 0, 0, None, 0))

    # ---- segment breaks (ctk_set_segments) ----------------------------------------------------------------------------
    def set_segments(self, starts):
        """independent time segments for the following track calls: starts = first step of every segment (0 first, strictly
        increasing).  No overlap, filter exemption or 3-D link crosses a break; ids stay unique over the slab."""
        st = np.asarray(starts)
        if st.ndim != 1 or (st.size and st.dtype.kind not in "iu"):
            raise ValueError("segment starts must be a 1-D integer array")
        st = np.ascontiguousarray(st, dtype=np.int64)
        check(lib().ctk_set_segments(self._h, st.ctypes.data if st.size else None, st.shape[0]))

    def clear_segments(self):
        check(lib().ctk_set_segments(self._h, None, 0))

    # ---- device-resident --------------------------------------------------------------------------
    def malloc(self, nbytes):
        p = C.c_void_p()
        check(lib().ctk_dev_malloc(self._h, C.byref(p), int(nbytes)))
        return p

    def free(self, p):
        check(lib().ctk_dev_free(self._h, p))

    def _download(self, outs, call):
        """call(*buffers) with one fresh device buffer per host array of `outs`, then the buffers copied into those arrays; they are
        freed on every path"""
        devs = []
        try:
            for a in outs:
                devs.append(self.malloc(max(a.nbytes, a.itemsize)))
            call(*devs)
            for a, d in zip(outs, devs):
                self.d2h(a, d)
        finally:
            for d in devs:
                self.free(d)

    def h2d(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        check(lib().ctk_memcpy_h2d(self._h, dst, arr.ctypes.data, arr.nbytes))

    def d2h(self, arr, src):
        assert arr.flags.c_contiguous
        check(lib().ctk_memcpy_d2h(self._h, arr.ctypes.data, src, arr.nbytes))

    def sync(self):
        check(lib().ctk_sync(self._h))

    def synth_fill(self, dst, T, ny, nx, seed=0, t0=0):
        """deterministic synthetic slab (measurements and tests only); t0 > 0: the window [t0, t0 + T) of the same slab"""
        check(lib().ctk_synth_fill_window(self._h, dst, int(t0), T, ny, nx, int(seed)))

    def checksum_i32(self, ptr, n, index0=0):
        """(position-weighted 64-bit checksum, number of nonzero elements) of an int32 device array"""
        out = np.zeros(2, dtype=np.uint64)
        check(lib().ctk_checksum_i32_dev(self._h, ptr, int(n), int(index0), out.ctypes.data))
        return int(out[0]), int(out[1])

    def memset(self, ptr, byte, nbytes):
        check(lib().ctk_dev_memset(self._h, ptr, int(byte), int(nbytes)))

    def check_flag(self, anom_dev, flag_dev, T, ny, nx, thr, cmp_op, persistence, max_id):
        """device-side properties of a result (ctk_check_flag_dev): dict of counts"""
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        if thr.shape != (T,):
            raise ValueError("thr must have shape (T,)")
        out = np.zeros(6, dtype=np.uint64)
        check(lib().ctk_check_flag_dev(self._h, anom_dev, flag_dev, int(T), int(ny), int(nx), thr.ctypes.data, int(cmp_op), int(persistence), int(max_id),
                                       out.ctypes.data))
        return dict(zip(("flag_outside_mask", "ids_out_of_range", "nonzero", "ids", "ids_below_persistence", "max_id"), (int(v) for v in out)))

    def debug_fail_at(self, stage):
        check(lib().ctk_debug_fail_at(self._h, int(stage)))

    def _thr_w_ptrs(self, thr, wrow):
        """addresses of the per-step thresholds (float64) and row weights (float32); remembered while the caller passes the very same
        arrays in the right layout (a loop over passes: the conversions and two ctypes objects per call were ~3 us with the GPU idle)"""
        c = getattr(self, "_pc", None)
        if c is not None and c[0] is thr and c[1] is wrow:
            return c[2], c[3], thr, wrow
        t = None if thr is None else np.ascontiguousarray(thr, dtype=np.float64)       # None: the handle's threshold field
        w = np.ascontiguousarray(wrow, dtype=np.float32)
        tp, wp = _ptr(t), w.ctypes.data
        self._pc = (thr, wrow, tp, wp) if (t is thr and w is wrow and t is not None) else None      # (never the address of a converted copy)
        return tp, wp, t, w

    def track_dev(self, anom_dev, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag_dev, f64=False):
        """thr=None: the threshold field set with set_threshold_field; f64: anom_dev holds float64"""
        tp, wp, thr, wrow = self._thr_w_ptrs(thr, wrow)
        n = C.c_int64(0)
        if f64:
            check(lib().ctk_track_f64_dev(self._h, anom_dev, T, ny, nx, tp, int(cmp_op), wp,
                                          float(overlap), int(persistence), int(bool(twosided)), flag_dev, C.byref(n)))
            return int(n.value)
        check(lib().ctk_track_f32_dev(self._h, anom_dev, T, ny, nx, tp, int(cmp_op), wp,
                                      float(overlap), int(persistence), int(bool(twosided)), flag_dev, C.byref(n)))
        return int(n.value)

    def track_sharded_dev(self, comm, anom_dev, T_local, t_begin, T_total, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag_dev,
                          f64=False, segments=None):
        """the whole path on the time shard [t_begin, t_begin + T_local) of T_total steps; every rank of `comm` must call.
        segments: None, or the first step of every independent time segment as GLOBAL indices into [0, T_total) (0 first, strictly
        increasing), the same on every rank (ctk_track_sharded_seg_*_dev)"""
        tp, wp, thr, wrow = self._thr_w_ptrs(thr, wrow)
        if thr is not None and thr.shape != (T_local,):
            raise ValueError("thr must hold one value per local timestep")
        n = C.c_int64(0)
        if segments is None:
            fn, seg = (lib().ctk_track_sharded_f64_dev if f64 else lib().ctk_track_sharded_f32_dev), ()
        else:
            st = _seg_starts(segments)
            fn, seg = (lib().ctk_track_sharded_seg_f64_dev if f64 else lib().ctk_track_sharded_seg_f32_dev), (st.ctypes.data if st.size else None, st.shape[0])
        check(fn(self._h, comm.ptr, anom_dev, int(T_local), int(t_begin), int(T_total), ny, nx, tp, int(cmp_op), wp,
                 float(overlap), int(persistence), int(bool(twosided)), flag_dev, C.byref(n), *seg))
        return int(n.value)

    # ---- run_lifecycle reductions ------------------------------------------------------------------------
    def _life_rows(self, n):
        rows = np.empty(n, dtype=LIFE_ROW)
        check(lib().ctk_lifecycle_rows(self._h, rows.ctypes.data, n))
        return rows

    def lifecycle(self, flag, field, wrow, resident_f64=None):
        """flag (T, ny, nx) int32, field float32/float64 of the same shape -> LIFE_ROW records sorted by (label, t).
        field = None: the anomaly slab left resident by `anomalies(..., keep_resident=True)` (resident_f64: its type)"""
        flag = np.ascontiguousarray(flag, dtype=np.int32)
        if field is None:
            f64 = bool(resident_f64)
        else:
            f64 = np.asarray(field).dtype == np.float64
            field = np.ascontiguousarray(field, dtype=np.float64 if f64 else np.float32)
        if flag.ndim != 3 or (field is not None and field.shape != flag.shape):
            raise ValueError("flag and field must share one (time, lat, lon) shape")
        T, ny, nx = flag.shape
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        if wrow.shape != (ny,):
            raise ValueError("wrow must have shape (ny,)")
        n = C.c_int64(0)
        fn = lib().ctk_lifecycle_f64 if f64 else lib().ctk_lifecycle_f32
        check(fn(self._h, flag.ctypes.data, None if field is None else field.ctypes.data, T, ny, nx, wrow.ctypes.data, C.byref(n)))
        return self._life_rows(int(n.value))

    def lifecycle_exact(self, row_idx):
        """rows of the LAST lifecycle call (indices into its sorted rows) in the reference's own summation orders: LIFE_EXACT.
        Raises ContrackHipError (CTK_E_STATE) when a later call on this Tracker has overwritten or released the slabs of that call:
        any host-array or streamed entry, release_io, or -- after field=None -- an anomaly call (include/contrack_hip.h)"""
        idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        out = np.empty(len(idx), dtype=LIFE_EXACT)
        check(lib().ctk_lifecycle_exact(self._h, idx.ctypes.data, len(idx), out.ctypes.data))
        return out

    def lifecycle_stream(self, flag_source, field_source, wrow, shape=None, dtype=None, chunk_steps=0, pick=None):
        """`lifecycle` with both slabs passing through chunk-sized device buffers (ctk_lifecycle_stream_*; device footprint: two
        chunks of each slab and the tables of one chunk).

        flag_source:  an int32 (T, ny, nx) array (np.memmap included) or a callable reader(t0, nt, out) that fills `out`, an int32
                      (nt, ny, nx) view of pinned memory, with the time steps [t0, t0 + nt);
        field_source: a float32 / float64 array of the same shape or such a reader of values -- with a reader on either side
                      `shape` = (T, ny, nx) is required, with a field reader `dtype` too.  The flag reader is called first;
        chunk_steps:  time steps per chunk, 0: about 256 MB of field;
        pick:         None, or pick(rows) -> indices: called once per chunk with that chunk's LIFE_ROW records (sorted by (label, t),
                      t global), returns the ascending indices of the rows to re-evaluate in the reference's summation orders
                      while the chunk is on the device (contrack.fragile_rows is the rule run_lifecycle uses).
        Returns (rows, exact_idx, exact): all LIFE_ROW records sorted by (label, t), the picked rows as ascending indices into
        them, and their LIFE_EXACT records."""
        L = lib()
        arrays = not callable(flag_source) and not callable(field_source)
        if not callable(flag_source):
            flag_source = flag_source if isinstance(flag_source, np.memmap) and flag_source.dtype == np.int32 else np.ascontiguousarray(flag_source, dtype=np.int32)
            if flag_source.ndim != 3:
                raise ValueError("flag must be (time, lat, lon)")
        if not callable(field_source):
            if not isinstance(field_source, np.memmap) or field_source.dtype not in (np.float32, np.float64):
                field_source = np.ascontiguousarray(field_source, dtype=np.float64 if np.asarray(field_source).dtype == np.float64 else np.float32)
            if field_source.ndim != 3:
                raise ValueError("field must be (time, lat, lon)")
        if shape is None:
            have = [a.shape for a in (flag_source, field_source) if not callable(a)]
            if not have:
                raise ValueError("reader callbacks need shape=(T, ny, nx) and dtype")
            shape = have[0]
        T, ny, nx = (int(v) for v in shape)
        for a in (flag_source, field_source):
            if not callable(a) and a.shape != (T, ny, nx):
                raise ValueError("flag and field must share one (time, lat, lon) shape")
        if callable(field_source):
            if dtype is None:
                raise ValueError("a field reader needs dtype")
            dt = np.dtype(dtype)
        else:
            dt = field_source.dtype
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("the field must be float32 or float64")
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        if wrow.shape != (ny,):
            raise ValueError("wrow must have shape (ny,)")
        tr = _Trampolines()

        def pk(_user, rows, n, idx, nidx):
            view = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_byte)), shape=(n * LIFE_ROW.itemsize,)).view(LIFE_ROW)
            chosen = np.ascontiguousarray(pick(view), dtype=np.int64).reshape(-1)
            if len(chosen) > n:
                raise ValueError("pick returned more indices than rows")
            np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_int64)), shape=(max(int(n), 1),))[:len(chosen)] = chosen
            C.cast(nidx, C.POINTER(C.c_int64))[0] = len(chosen)
        pcb = tr.wrap(LIFE_PICK_FN, pk) if pick is not None else LIFE_PICK_FN()          # (a NULL pointer: no rows are picked)
        n, nx_ = C.c_int64(0), C.c_int64(0)
        tail = (wrow.ctypes.data, int(chunk_steps), pcb, None, C.byref(n), C.byref(nx_))
        if arrays:
            fn = L.ctk_lifecycle_stream_f64 if dt == np.float64 else L.ctk_lifecycle_stream_f32
            rc = fn(self._h, flag_source.ctypes.data, field_source.ctypes.data, T, ny, nx, *tail)
        else:
            fcb, vcb = tr.reader(flag_source, C.c_int32, (ny, nx)), tr.reader(field_source, _float_ctype(dt), (ny, nx))
            rc = L.ctk_lifecycle_stream_cb(self._h, dt.itemsize, T, ny, nx, fcb, None, vcb, None, *tail)
        tr.finish(rc)
        rows = self._life_rows(int(n.value))
        idx = np.empty(int(nx_.value), dtype=np.int64)
        exact = np.empty(int(nx_.value), dtype=LIFE_EXACT)
        check(L.ctk_lifecycle_stream_exact(self._h, idx.ctypes.data, exact.ctypes.data, len(idx)))
        return rows, idx, exact

    def debug_lifecycle_path(self, T):
        """test hook: the path of the last lifecycle call (of T time steps) as (dict(rw, nsx, nby, vec, given_up, launches, attempts,
        sort), steps) -- steps[t]: rounds of k_lifecycle time step t took part in, 0 = the strip kernels held it"""
        v = np.zeros(8, dtype=np.int64)
        steps = np.zeros(max(int(T), 1), dtype=np.uint8)
        check(lib().ctk_debug_lifecycle_path(self._h, v.ctypes.data, steps.ctypes.data, int(T)))
        return dict(zip("rw nsx nby vec given_up launches attempts sort".split(), (int(x) for x in v))), steps[:int(T)]

    def lifecycle_dev(self, flag_dev, field_dev, T, ny, nx, wrow, f64=False):
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        n = C.c_int64(0)
        fn = lib().ctk_lifecycle_f64_dev if f64 else lib().ctk_lifecycle_f32_dev
        check(fn(self._h, flag_dev, field_dev, T, ny, nx, wrow.ctypes.data, C.byref(n)))
        return self._life_rows(int(n.value))

    def set_timing(self, level=2):
        """0: off; 1: HIP events around k_threshold / k_relabel only; 2 (or True): around every kernel group"""
        check(lib().ctk_set_timing(self._h, 2 if level is True else int(level)))

    def set_fused(self, enable=True):
        """the one-call entries without a host hand-off (default) or always on the synchronous path"""
        check(lib().ctk_set_fused_pass(self._h, int(bool(enable))))

    def set_result_transfer(self, mode=-1):
        """how the host-array entries bring the result over PCIe: 1 run tables expanded by host threads (default), 0 the dense
        slab written by k_relabel, -1 the environment's choice (CTK_RLE_OUT); 2: test hook -- run tables wanted but made unavailable (the
        library then repeats the pass with the dense copy)"""
        check(lib().ctk_set_result_transfer(self._h, int(mode)))
        self._transfer_mode = int(mode)

    @property
    def result_as_runs(self):
        m = getattr(self, "_transfer_mode", -1)
        if m >= 0:
            return m == 1
        import re
        v = os.environ.get("CTK_RLE_OUT")                      # (as the library reads it: atoi)
        mt = re.match(r"\s*[+-]?\d+", v) if v is not None else None
        return v is None or (mt is not None and int(mt.group(0)) != 0)

    def stats(self):
        v = np.zeros(37, dtype=np.int64)
        check(lib().ctk_get_stats_n(self._h, v.ctypes.data, 37))
        names = ["runs", "max_runs_per_step", "components", "pairs", "seam_rows_to_driver", "labels_3d", "seam_ops",
                 "filter_passes", "host_path", "seam_loop_ns", "seam_folds", "seam_copy_ns", "ungrouped_pairs", "pair_table_regrows", "filter_rounds",
                 "ambiguous_decisions", "exact_fixups", "shared_seam_rows", "off_fused_path_reason", "relabel_kernel", "fused_pass", "x4_speculated", "result_as_runs", "mask_allocations_tried", "mask_ratio_x1000",
                 "mask_check_us", "mask_spacer_mb", "label_forms", "overlap_form", "rowcount_threads",
                 "filter_forms", "extent_form", "runval_form", "relabel_shape", "count_form", "device_cus", "rowcount_groups"]
        return dict(zip(names, v.tolist()))

    def debug_set_pair_capacity(self, records):
        check(lib().ctk_debug_set_pair_capacity(self._h, int(records)))

    def debug_set_seam_caps(self, labels, ops):
        check(lib().ctk_debug_set_seam_caps(self._h, int(labels), int(ops)))

    def debug_shard_exchange(self):
        """test hook: what the last track_sharded_dev call on this handle decided at its exchanges (include/contrack_hip_debug.h).
        form: 0 device; host-driven bits 1 no device attempt, 2 shared operations beyond the reserve, 4 a rank's driver gave up"""
        v = np.zeros(12, dtype=np.int64)
        check(lib().ctk_debug_shard_exchange(self._h, v.ctypes.data))
        lo, hi = (lambda x: int(x) & 0xffffffff), (lambda x: (int(x) >> 32) & 0xffffffff)
        return dict(capB=int(v[0]), capB_repeats=int(v[1]), nlast=lo(v[2]), nh=hi(v[2]), capC=lo(v[3]), capD=hi(v[3]), x5_repeats=int(v[4]),
                    sent_records=lo(v[5]), sent_labels=hi(v[5]), ne=int(v[6]), pack_ext_workgroups=int(v[7]), tables_ahead_used=int(v[8]),
                    form=int(v[9]), shared_ops=int(v[10]), zero_exchanged=int(v[11]))

    def debug_set_shared_ops_reserve(self, n):
        """test hook: shared-cluster operations the device form of the time-shard path takes (0 = its reserve); the SAME value on every
        handle of a group"""
        check(lib().ctk_debug_set_shared_ops_reserve(self._h, int(n)))

    def debug_set_spin(self, limit_ms=0.0, stall_mode=0):
        """bounded inter-workgroup waits of the one-launch filter pass: limit (0 = default 200 ms), 1 = head of the chain late, 2 = never"""
        check(lib().ctk_debug_set_spin(self._h, float(limit_ms), int(stall_mode)))

    def debug_set_mailbox(self, cand_records, labels):
        check(lib().ctk_debug_set_mailbox(self._h, int(cand_records), int(labels)))

    def set_filter_round(self, passes):
        check(lib().ctk_set_filter_round(self._h, int(passes)))

    def set_device_resolve(self, on=True):
        check(lib().ctk_set_device_resolve(self._h, int(bool(on))))

    def timing_sums(self, reset=True):
        """(mean ms per measured call, calls that measured it) per kernel group since the last reset"""
        sums = np.zeros(len(TIMER_NAMES), dtype=np.float64)
        cnt = np.zeros(len(TIMER_NAMES), dtype=np.int64)
        check(lib().ctk_get_timing_sums(self._h, sums.ctypes.data, cnt.ctypes.data, int(bool(reset))))
        return ({k: (float(v) / int(n) if n else 0.0) for k, v, n in zip(TIMER_NAMES, sums, cnt)}, dict(zip(TIMER_NAMES, cnt.tolist())))

    def time_relabel(self, flag_dev, persistence, variant, xcd=-1, reps=5):
        """ms of `reps` launches of the write kernel on the finished tables of the last track_dev pass (variant 0 k_relabel_v5, 1 without its
        SGPR limit; xcd: chunk -> XCD order, -1 the handle's)"""
        ms = np.zeros(reps, dtype=np.float64)
        check(lib().ctk_debug_time_relabel(self._h, flag_dev, int(persistence), int(variant), int(xcd), int(reps), ms.ctypes.data))
        return ms

    def stream_ceiling(self, ptr, nbytes, write, reps=5):
        """best-of-reps ms of a plain 16-byte non-temporal store (write; 2: one contiguous eighth of the buffer per XCD) / load stream
        over a device buffer (overwritten when write)"""
        ms = C.c_double(0.0)
        check(lib().ctk_debug_stream_ceiling(self._h, ptr, int(nbytes), int(write), int(reps), C.byref(ms)))
        return ms.value

    def timings(self):
        ms = np.zeros(len(TIMER_NAMES), dtype=np.float64)
        check(lib().ctk_get_timings(self._h, ms.ctypes.data))
        return dict(zip(TIMER_NAMES, ms.tolist()))

    # ---- staged (time-sharded) -------------------------------------------------------------------
    def shard_label2d(self, anom_dev, T, ny, nx, thr, cmp_op, wrow, has_prev, f64=False):
        """f64: anom_dev holds float64"""
        thr = None if thr is None else np.ascontiguousarray(thr, dtype=np.float64)
        wrow = np.ascontiguousarray(wrow, dtype=np.float32)
        fn = lib().ctk_shard_label2d_f64 if f64 else lib().ctk_shard_label2d
        check(fn(self._h, anom_dev, T, ny, nx, _ptr(thr), int(cmp_op), wrow.ctypes.data, int(bool(has_prev))))

    def halo_size(self):
        s = C.c_size_t(0)
        check(lib().ctk_shard_halo_size(self._h, C.byref(s)))
        return int(s.value)

    def halo_export(self):
        p, s = C.c_void_p(), C.c_size_t(0)
        check(lib().ctk_shard_halo_export(self._h, C.byref(p), C.byref(s)))
        return p, int(s.value)

    def halo_import(self, blob_dev, nbytes):
        check(lib().ctk_shard_halo_import(self._h, blob_dev, int(nbytes)))

    def shard_overlap(self):
        check(lib().ctk_shard_overlap(self._h))

    def shard_tables(self):
        p, s = C.c_void_p(), C.c_size_t(0)
        check(lib().ctk_shard_tables(self._h, C.byref(p), C.byref(s)))
        return C.string_at(p, s.value)

    def shard_extents(self, result, shard, t_begin):
        p, n = C.c_void_p(), C.c_int64(0)
        check(lib().ctk_shard_extents(self._h, result.ptr, int(shard), int(t_begin), C.byref(p), C.byref(n)))
        return p, int(n.value)

    def shard_write(self, persistence, flag_dev):
        n, z = C.c_int64(0), C.c_int(0)
        check(lib().ctk_shard_write(self._h, int(persistence), flag_dev, C.byref(n), C.byref(z)))
        return int(n.value), bool(z.value)

    def debug_mask(self, T, ny, nx):
        m = np.empty((T, ny, nx), dtype=np.uint8)
        check(lib().ctk_debug_mask(self._h, m.ctypes.data))
        return m

    def debug_label2d(self, T, ny, nx, before_seam):
        lab = np.empty((T, ny, nx), dtype=np.int32)
        check(lib().ctk_debug_label2d(self._h, int(bool(before_seam)), lab.ctypes.data))
        return lab
