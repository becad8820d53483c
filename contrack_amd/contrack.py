"""Drop-in `contrack` class: the public interface of steidani/ConTrack's `contrack.contrack`
(contrack/contrack.py:49-949) with `run_contrack` executed by the MI355X HIP path.

Same constructor, `read`, `read_xarray`, `set_up`, `calc_clim`, `calc_anom`, `run_contrack` signatures, the
same `ValueError` / `IOError` texts, the same INFO log lines and the same `flag` variable (dims of the input
variable, int32 ids identical to the reference's, same attrs).  `run_contrack`, `run_lifecycle`, `calc_clim` / `calc_anom`,
the percentile threshold and the blocking frequency (`calc_frequency`, README.rst:159-160) of the reference's README run on the
GPU; `calc_anom` leaves its slab resident in HBM so that the following `run_contrack` does not cross PCIe on the way in.

xarray is imported lazily: the class itself only needs the small part of the Dataset/DataArray API listed in
tests/minixr.py, so it also works on any duck-typed dataset.  `track_numpy` is the array-level entry.

Stated deviations from the reference:
  * `flag` is written back with the INVERSE of the (time, lat, lon) permutation; the reference applies the
    forward permutation twice (contrack.py:778), which is only correct when the permutation is its own
    inverse -- for every such input (including the tested (time, lat, lon) order) both agree.
  * the library computes int32 ids (more than 2^31-2 ids raise instead of wrapping); the class hands `flag` out in the
    reference's dtype -- int32, int64 from 2^31-2 elements on, as scipy.ndimage.label does (contrack.py:687, :751).  `track_numpy`
    and the C ABI stay int32.
  * the numpy array behind `ds['anom']` after `calc_anom` is read-only (its twin stays in HBM for `run_contrack`); assign a
    new array to the variable to change it.
  * `run_contrack(..., chunk_steps=n)` (extension): stream the variable through the GPU in slices of n time steps; combines with
    `segments='gaps'` and with a member dimension.
"""
import logging
import os

import numpy as np

from . import _native

logger = logging.getLogger(__name__)
logging.basicConfig(format='%(levelname)s: %(message)s', level=logging.INFO)

_TRACKERS = {}


def _tracker(device=None):
    dev = int(os.environ.get("CONTRACK_DEVICE", "0")) if device is None else int(device)
    if dev not in _TRACKERS:
        _TRACKERS[dev] = _native.Tracker(dev)
    return _TRACKERS[dev]


# ------------------------------------------------------------------------------------------------
# array-level API
# ------------------------------------------------------------------------------------------------
def row_weights(lat, dlat, dlon):
    """Row weights as contrack.py:703-704 evaluates them: cos(lat*pi/180) in the dtype of `lat`, scaled by
    111*dlat*111*dlon left to right, cast to float32 (pole rows come out slightly negative in float32)."""
    weight_lat = np.cos(np.asarray(lat) * np.pi / 180)
    return np.array((111 * dlat * 111 * dlon * weight_lat)).astype(np.float32).reshape(-1)


def prepare_thresholds(threshold, T, data_dtype):
    """Per-timestep float64 thresholds thr[t] such that (double)x <op> thr[t] is the compare the reference
    evaluates (contrack.py:650-671 under numpy's promotion rules): a Python number is cast to the array's
    dtype; a float64 numpy scalar / array promotes the compare to float64."""
    data_dtype = np.dtype(data_dtype)
    if isinstance(threshold, (bool, int, float)) and not isinstance(threshold, np.generic):
        if data_dtype.kind == "f":
            val = np.asarray(threshold, dtype=data_dtype).astype(np.float64)
        else:
            val = np.float64(threshold)
        return np.full(int(T), val, dtype=np.float64)
    arr = np.asarray(threshold)
    if arr.dtype.kind not in "fiub":
        raise TypeError("threshold must be numeric")
    if data_dtype == np.float32 and (arr.dtype == np.float32 or arr.dtype == np.float16 or
                                     (arr.dtype.kind in "iub" and arr.dtype.itemsize <= 2)):
        arr = arr.astype(np.float32)
    out = np.broadcast_to(arr.astype(np.float64).reshape(-1) if arr.ndim else arr.astype(np.float64), (int(T),))
    return np.ascontiguousarray(out, dtype=np.float64)


def is_threshold_field(threshold):
    """a numpy threshold with ndim >= 2 whose last two axes are not (1, 1) varies by grid point; scalars, (T,) and (T, 1, 1) do not"""
    if hasattr(threshold, "dims") or isinstance(threshold, (bool, int, float)):
        return False
    arr = np.asarray(threshold)
    return arr.ndim >= 2 and arr.shape[-2:] != (1, 1)


def field_planes(tll):
    """a (T, ny, nx) threshold (broadcast views allowed) -> (planes (nplanes, ny, nx), plane_of_step (T,)): ONE plane when the
    array does not vary along time (a (ny, nx) field broadcast over the steps), else one plane per step"""
    T = tll.shape[0]
    if T <= 1 or tll.strides[0] == 0:
        return np.ascontiguousarray(tll[:1]), np.zeros(T, dtype=np.int32)
    return np.ascontiguousarray(tll), np.arange(T, dtype=np.int32)


def broadcast_field(threshold, shape, sort=(0, 1, 2)):
    """numpy's broadcasting of `threshold` against a variable of `shape` (the variable's own dim order), then the (time, lat, lon)
    transpose `sort` -> (planes, plane_of_step) as field_planes"""
    arr = np.asarray(threshold)
    if arr.dtype.kind not in "fiub":
        raise TypeError("threshold must be numeric")
    try:
        full = np.broadcast_shapes(arr.shape, tuple(shape))
    except ValueError:
        full = None
    if full != tuple(shape):
        raise ValueError("a threshold of shape {} does not broadcast against the variable's shape {}".format(arr.shape, tuple(shape)))
    return field_planes(np.broadcast_to(arr, tuple(shape)).transpose(sort))


def _track_field(trk, planes, pos, call):
    """one call with the handle's threshold field set to (planes, pos); the field is cleared again afterwards (it can be GBs)"""
    trk.set_threshold_field(planes, pos)
    try:
        return call(None)
    finally:
        trk.clear_threshold_field()


def _track_segments(trk, starts, call):
    """one call with the handle's segment breaks set to `starts` (None: no segments, the call as it is); cleared again afterwards.
    `call` takes no argument: it may itself be a _track_field call."""
    if starts is None:
        return call()
    trk.set_segments(starts)
    try:
        return call()
    finally:
        trk.clear_segments()


def segment_starts(starts, T):
    """validated segment starts (int64): 1-D, starts[0] == 0, strictly increasing, every start < T"""
    st = np.asarray(starts)
    if st.ndim != 1 or st.size == 0 or st.dtype.kind not in "iu":
        raise ValueError("segments must be a non-empty 1-D integer array of start indices")
    st = st.astype(np.int64)
    if st[0] != 0:
        raise ValueError("the first segment must start at step 0 (segments[0] = {})".format(st[0]))
    if np.any(np.diff(st) <= 0):
        raise ValueError("segment starts must be strictly increasing")
    if st[-1] >= T:
        raise ValueError("segment start {} lies beyond the {} time steps".format(st[-1], T))
    return st


def gap_starts(steps):
    """segment starts of a time axis from its T - 1 steps between consecutive timestamps: a new segment wherever the step is
    larger than the smallest one (a seasonal selection, concatenated members)"""
    steps = np.asarray(steps)
    if steps.size == 0:
        return np.zeros(1, dtype=np.int64)
    return np.concatenate([[0], np.nonzero(steps > steps.min())[0] + 1]).astype(np.int64)


def track_numpy(anom, wrow, threshold, gorl, overlap, persistence, twosided=True, device=None, segments=None, chunk_steps=None):
    """run_contrack on a (time, lat, lon) numpy slab.  Returns (flag int32 (T,ny,nx), n_tracked).

    anom float32 (other dtypes are compared exactly in float64 on the device), wrow float32 (ny,) from
    `row_weights`, threshold scalar, per-timestep vector or a threshold field: a numpy array of ndim >= 2 (last two axes not (1, 1))
    that broadcasts against anom, e.g. (ny, nx) or (T, ny, nx) -- pixel (t, y, x) is compared with its own value, under numpy's
    promotion rules; gorl in {'>=','<=','>','<','ge','le','gt','lt'}.
    segments (extension): int array of segment starts (0 first, strictly increasing) -- independent series concatenated in time
    (ensemble members, seasons); no overlap, filter exemption or 3-D link crosses a break, ids stay unique over the slab.
    chunk_steps (extension): stream the slab (an array or np.memmap the host holds) through chunk-sized device buffers, that many
    time steps at a time (0: about 256 MB each); same result, with or without segments."""
    if gorl not in _native.CMP_OPS:
        raise ValueError(_native.GORL_ERRMSG)
    anom = np.asarray(anom)
    if anom.ndim != 3:
        raise ValueError("anom must be (time, lat, lon)")
    field = broadcast_field(threshold, anom.shape) if is_threshold_field(threshold) else None
    thr = None if field is not None else prepare_thresholds(threshold, anom.shape[0], anom.dtype)
    trk = _tracker(device)
    if chunk_steps is not None:
        # the streaming entries take the starts with the call (the handle's sticky segments are for the one-call entries)
        starts = None if segments is None else segment_starts(segments, anom.shape[0])
        if anom.dtype not in (np.float32, np.float64):
            if anom.dtype.kind not in "fiub":
                raise TypeError("anom must be a real numeric array")
            anom = anom.astype(np.float64)
        call = lambda t: trk.track_stream(anom, t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided, chunk_steps=int(chunk_steps),
                                          segments=starts)
        return call(thr) if field is None else _track_field(trk, field[0], field[1], call)
    if anom.dtype != np.float32:
        if anom.dtype.kind not in "fiub":
            raise TypeError("anom must be a real numeric array")
        a64 = anom.astype(np.float64)
        call = lambda t: trk.track(a64, t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided, f64=True)
    else:
        call = lambda t: trk.track(anom, t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided)
    starts = None if segments is None else segment_starts(segments, anom.shape[0])
    return _track_segments(trk, starts, lambda: call(thr) if field is None else _track_field(trk, field[0], field[1], call))


SEASONS = np.array(['DJF', 'DJF', 'MAM', 'MAM', 'MAM', 'JJA', 'JJA', 'JJA', 'SON', 'SON', 'SON', 'DJF'])


def season_of_month(month):
    """xarray's time.season: 'DJF', 'MAM', 'JJA' or 'SON' for months 1..12 (np.unique orders them DJF, JJA, MAM, SON, as
    groupby('time.season') does)"""
    month = np.asarray(month)
    if month.size and (month.min() < 1 or month.max() > 12):
        raise ValueError("months must lie in 1..12")
    return SEASONS[month.astype(np.int64) - 1]


def _flag_source(flag, shape=None):
    """the flag slab of a *_numpy call as the binding takes it: (source, shape, is_array).  An integer (time, lat, lon) array goes as
    it is when int32 or narrower; a wider one goes through a reader that narrows it chunk by chunk (an id beyond int32 raises
    ValueError from the chunk that holds it); a reader(t0, nt, out) needs shape=(T, ny, nx)."""
    if callable(flag):
        if shape is None:
            raise ValueError("a reader needs shape=(T, ny, nx)")
        return flag, shape, False
    flag = flag if isinstance(flag, np.memmap) else np.asarray(flag)
    if flag.ndim != 3:
        raise ValueError("flag must be (time, lat, lon)")
    if flag.dtype.kind not in "iub":
        raise ValueError("flag must be an integer field")
    if flag.dtype.itemsize < 4 or flag.dtype == np.int32:
        return flag, flag.shape, True

    def reader(t0, nt, out):
        out[...] = _int32_chunk(flag[t0:t0 + nt])
    return reader, flag.shape, False


def frequency_percent(counts, n):
    """counts (G, ...) / n[g] * 100 in float64, divided first as xr.where(...).sum('time') / ntime * 100 does (README.rst:159-160);
    an empty group (n[g] == 0) gives NaN, numpy's 0 / 0"""
    counts = np.asarray(counts)
    n = np.asarray(n, dtype=np.int64).reshape((-1,) + (1,) * (counts.ndim - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return counts.astype(np.float64) / n * 100


def frequency_numpy(flag, group=None, above=0, percent=True, device=None, chunk_steps=None, shape=None):
    """the blocking frequency of README.rst:159-160 on a (time, lat, lon) integer flag slab:
        np.where(flag > above, 1, 0).sum(axis=0) / T * 100           (above = 1 is the README's expression)
    per group of timesteps when `group` (one id in [0, G) per timestep, any order in time) is given.  The count runs on the GPU
    (ctk_frequency); int32 and narrower flags are read as they are, wider ones are converted to int32 chunk by chunk (an id beyond
    int32 raises ValueError).  Returns float64 percent (G, ny, nx) -- (ny, nx) without `group` -- or, with percent=False, int64
    counts of the same shape.  chunk_steps: time steps per chunk on their way through the device (None or 0: about 256 MB); with
    shape=(T, ny, nx) `flag` may be a reader(t0, nt, out) that fills an int32 (nt, ny, nx) buffer (ctk_frequency_cb)."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    trk = _tracker(device)
    source, shape, is_array = _flag_source(flag, shape)
    T = int(shape[0])
    ids, G = _native._groups(group, T)
    counts = trk.frequency(source, ids, G, above, steps) if is_array else trk.frequency_cb(source, shape, ids, G, above, steps)
    counts = counts.astype(np.int64)
    out = frequency_percent(counts, np.bincount(ids, minlength=G) if ids is not None else [T]) if percent else counts
    return out[0] if group is None else out


def spell_duration(steps, events):
    """steps / events in float64, NaN where events == 0 (numpy's 0 / 0): the mean duration of the spells spells_numpy counted"""
    steps, events = np.asarray(steps), np.asarray(events)
    with np.errstate(invalid="ignore", divide="ignore"):
        return steps.astype(np.float64) / events.astype(np.float64)


def spells_numpy(flag, group=None, above=0, by_id=True, min_duration=1, segments=None, chunk_steps=None, device=None, shape=None):
    """blocked spells per grid point of a (time, lat, lon) integer flag slab.  At a grid point, step t continues step t - 1 iff t is
    not a segment start, both flags are > above and, with by_id, they are the same id.  A spell is a maximal chain of continuing
    steps; it belongs to the group of its first step (a block that starts on 27 February is a DJF event) and counts if it lasts
    min_duration steps or more; one cut by the end of the slab or of a segment counts with the length it has.  Returns int64
    (events, steps, longest): the number of spells, the sum of their durations and the longest one, (G, ny, nx) each -- (ny, nx)
    without `group` (one id in [0, G) per timestep, any order in time).  The mean duration is spell_duration(steps, events).
    segments: None, or the first step of every independent time segment (0 first, strictly increasing, below T).  The scan runs
    on the GPU (ctk_spells); int32 and narrower flags are read as they are, wider ones are converted to int32 chunk by chunk (an id
    beyond int32 raises ValueError).  chunk_steps: time steps per chunk on their way through the device (None or 0: about 256 MB);
    with shape=(T, ny, nx) `flag` may be a reader(t0, nt, out) that fills an int32 (nt, ny, nx) buffer (ctk_spells_cb)."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    if steps < 0:
        raise ValueError("chunk_steps={} (at least 0)".format(steps))
    _native._above(above)
    source, shape, is_array = _flag_source(flag, shape)
    ids, G, st, by, md = _native._spell_args(int(shape[0]), group, None, segments, by_id, min_duration)
    trk = _tracker(device)
    out = trk.spells(source, ids, G, above, by, md, st, steps) if is_array else trk.spells_cb(source, shape, ids, G, above, by, md, st, steps)
    out = tuple(a.astype(np.int64) for a in out)
    return tuple(a[0] for a in out) if group is None else out


def _positive_int32(ids, what="ids"):
    ids = np.asarray(ids).reshape(-1)
    if ids.size and ids.dtype.kind not in "iub":
        raise ValueError("{} must be integers".format(what))
    ids = ids.astype(np.int64)
    if ids.size and (ids.min() < 1 or ids.max() > np.iinfo(np.int32).max):
        raise ValueError("{} must lie in 1 .. 2^31 - 1 (0 and negative values are background)".format(what))
    return ids


def subset_table(ids=None, steps=None, T=None):
    """the table (off int64, ids int32) the subset entries take (include/contrack_hip.h), sorted, duplicates removed, validated.
    ids alone: the tracks to keep at every step -- off = [0, K].  steps and ids, one pair per wanted (step, track) row, with T, the
    number of steps of the slab: off has T + 1 entries and ids[off[t]:off[t + 1]] are the ids wanted at step t."""
    if ids is None:
        raise ValueError("subset_table needs ids (and steps with T for rows)")
    ids = _positive_int32(ids)
    if steps is None:
        ids = np.unique(ids)
        return np.array([0, len(ids)], dtype=np.int64), ids.astype(np.int32)
    if T is None or int(T) < 1:
        raise ValueError("a row table needs T, the number of steps of the slab (at least 1)")
    T = int(T)
    steps = np.asarray(steps).reshape(-1)
    if steps.size and steps.dtype.kind not in "iub":
        raise ValueError("steps must be integers")
    steps = steps.astype(np.int64)
    if steps.shape != ids.shape:
        raise ValueError("steps and ids must pair up: {} steps, {} ids".format(steps.size, ids.size))
    if steps.size and (steps.min() < 0 or steps.max() >= T):
        raise ValueError("steps must lie in [0, {})".format(T))
    pairs = np.unique(steps * (1 << 31) + ids)                                    # (sorted by step, then id)
    off = np.zeros(T + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(pairs >> 31, minlength=T))
    return off, (pairs & ((1 << 31) - 1)).astype(np.int32)


def subset_numpy(flag, table, invert=False, kind='id', chunk_steps=None, device=None, shape=None, return_hits=False):
    """a (time, lat, lon) integer flag slab restricted to the tracks or (step, track) rows of `table` (subset_table): where a
    pixel's id is in its step's slice the id stays (kind='mask': becomes 1), everything else becomes 0; invert keeps the positive
    ids that are NOT in the slice instead.  Values <= 0 are background either way.  Runs on the GPU (ctk_subset); int32 and
    narrower flags are read as they are, wider ones are converted to int32 chunk by chunk (an id beyond int32 raises ValueError).
    Returns (out int32, n_selected) -- with return_hits (out, n_selected, hits): uint64 per entry of the table's ids, the pixels
    that entry found, whatever invert is.  chunk_steps: time steps per chunk on their way through the device (None or 0: about
    256 MB); with shape=(T, ny, nx) `flag` may be a reader(t0, nt, out) that fills an int32 (nt, ny, nx) buffer (ctk_subset_cb)."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    if steps < 0:
        raise ValueError("chunk_steps={} (at least 0)".format(steps))
    source, shape, is_array = _flag_source(flag, shape)
    trk = _tracker(device)
    if is_array:
        out, hits, n = trk.subset(source, table, invert, kind, steps, want_hits=return_hits)
    else:
        out, hits, n = trk.subset_cb(source, shape, table, invert, kind, chunk_steps=steps, want_hits=return_hits)
    return (out, n, hits) if return_hits else (out, n)


def blockstat_numpy(flag, table, x=None, want=('shape', 'peaks'), chunk_steps=None, device=None, shape=None, dtype=None):
    """per (step, track) row of `table` -- a ROW table, subset_table(ids, steps, T) -- the block's pixel count, its lowest and highest
    grid row, its zonal extent taken around the date line (west, width), and the largest and smallest value of the field `x` inside
    it with the pixel index row * nx + col where each sits first: a structured array of _native.BLOCK_ROW (ctk_block_row of
    include/contrack_hip.h, which states every field), one row per entry of the table's ids.  flag (time, lat, lon) integer, x of
    the same shape (float64 stays, everything else is taken as float32); want: 'shape', 'peaks' or both ('shape' alone needs no
    field).  Runs on the GPU (ctk_blockstat_*); everything is selection, so the rows are the same bytes whatever chunk_steps: time
    steps per chunk on both slabs' way through the device (None or 0: about 256 MB).  x None with 'peaks': the anomaly slab
    calc_anom left on the device (`dtype` its type), only the flags travel.  With shape=(T, ny, nx) and dtype, flag and x may be
    readers reader(t0, nt, out) (ctk_blockstat_cb); flags wider than int32 are narrowed chunk by chunk (an id beyond int32 raises
    ValueError)."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    if steps < 0:
        raise ValueError("chunk_steps={} (at least 0)".format(steps))
    bits = _native._block_want(want)
    peaks = bool(bits & _native.BLOCK_WANTS['peaks'])
    if not peaks:
        x = None
    if callable(flag) or callable(x):
        if shape is None or (peaks and dtype is None and (x is None or callable(x))):
            raise ValueError("a reader needs shape=(T, ny, nx) and the field's dtype")
    fread, fshape, is_array = _flag_source(flag, shape)
    shape = fshape if shape is None else shape
    if x is not None and not callable(x):
        x = x if isinstance(x, np.memmap) else np.asarray(x)
        if tuple(x.shape) != tuple(int(v) for v in shape):
            raise ValueError("the field has shape {}, the flag {}".format(x.shape, tuple(shape)))
        dtype = _native._field_dtype(x.dtype)
    dtype = np.dtype(dtype if dtype is not None else np.float32)
    trk = _tracker(device)
    if is_array and not callable(x):
        return trk.blockstat(fread, table, x, bits, steps, resident_f64=dtype == np.float64)
    xread = x
    if x is not None and not callable(x):
        def xread(t0, nt, out, slab=x):
            out[...] = slab[t0:t0 + nt]
    return trk.blockstat_cb(fread, xread, shape, dtype, table, bits, steps)


def track_table(frame):
    """one row per track of a life-cycle frame (run_lifecycle's DataFrame or a row selection of it) -- per (Flag, member) where the
    frame has a seventh, member column -- with what one selects tracks on: Onset and Decay (the first and last Date), Duration (the
    number of rows), OnsetLongitude, OnsetLatitude, DecayLongitude, DecayLatitude, MaxIntensity, MeanIntensity, MaxSize, MeanSize,
    PathLength (the sum of the great-circle distances in km between consecutive centres, rows in the frame's order) and Displacement
    (onset to decay), both with contrack.greatcircle_dist.  Host only (pandas)."""
    import pandas as pd

    def dist(*lonlat):
        return float(contrack.greatcircle_dist(None, *lonlat))
    base = ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']
    missing = [c for c in base if c not in frame.columns]
    if missing:
        raise ValueError("the frame lacks the columns {}".format(missing))
    member = [c for c in frame.columns if c not in base + ['Step', 'Row', 'Col']]
    if len(member) > 1:
        raise ValueError("the frame has more than one column besides run_lifecycle's: {}".format(member))
    keys = ['Flag'] + member
    columns = keys + ['Onset', 'Decay', 'Duration', 'OnsetLongitude', 'OnsetLatitude', 'DecayLongitude', 'DecayLatitude', 'MaxIntensity',
                      'MeanIntensity', 'MaxSize', 'MeanSize', 'PathLength', 'Displacement']
    rows = []
    for key, g in frame.groupby(keys, sort=True):
        key = key if isinstance(key, tuple) else (key,)
        lon, lat = g['Longitude'].to_numpy(), g['Latitude'].to_numpy()
        path = sum((dist(lon[i], lat[i], lon[i + 1], lat[i + 1]) for i in range(len(g) - 1)), 0.0)
        rows.append(tuple(key) + (g['Date'].iloc[0], g['Date'].iloc[-1], len(g), lon[0], lat[0], lon[-1], lat[-1], g['Intensity'].max(), g['Intensity'].mean(),
                                  g['Size'].max(), g['Size'].mean(), path, dist(lon[0], lat[0], lon[-1], lat[-1])))
    return pd.DataFrame(rows, columns=columns)


def composite_mean(sum, n):
    """sum / n in float64, NaN where n == 0 (numpy's 0 / 0): the mean of a composite from what composite_numpy returns"""
    sum = np.asarray(sum, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.asarray(n) == 0, np.nan, sum / np.asarray(n))


def composite_numpy(flag, x, group=None, above=0, skipna=False, chunk_steps=None, device=None, shape=None, dtype=None):
    """the composite of a float field over the flagged time steps, ds[var].where(ds[flag] > above).groupby(...).sum('time') with
    its count: (sum, n), sum[g] the float64 sum IN TIME ORDER of x[t] over the steps t of group g with flag[t] > above (skipna: and
    x[t] not NaN) at every grid point, n[g] (uint32) how many there were; composite_mean(sum, n) is the mean.  flag (time, lat,
    lon) integer, x of the same shape (float64 stays, everything else is taken as float32); group: one id in [0, G) per time step,
    any order in time, None: one group (the leading axis is then dropped).  The sums run on the GPU (ctk_composite_*) and are the
    same bits whatever chunk_steps: time steps per chunk on both slabs' way through the device (None or 0: about 256 MB of field).
    x None: the anomaly slab calc_anom left on the device (`dtype` its type), only the flags travel.  With shape=(T, ny, nx) and
    dtype, flag and x may be readers reader(t0, nt, out) (ctk_composite_cb); flags wider than int32 are narrowed chunk by chunk
    (an id beyond int32 raises ValueError)."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    if callable(flag) or callable(x):
        if shape is None or (dtype is None and (x is None or callable(x))):
            raise ValueError("a reader needs shape=(T, ny, nx) and the field's dtype")
    fread, fshape, is_array = _flag_source(flag, shape)
    shape = fshape if shape is None else shape
    if x is not None and not callable(x):
        x = x if isinstance(x, np.memmap) else np.asarray(x)
        if tuple(x.shape) != tuple(int(v) for v in shape):
            raise ValueError("the field has shape {}, the flag {}".format(x.shape, tuple(shape)))
        dtype = _native._field_dtype(x.dtype)
    dtype = np.dtype(dtype if dtype is not None else np.float32)
    T = int(shape[0])
    ids, G = _native._groups(group, T)
    trk = _tracker(device)
    if is_array and not callable(x):
        s, n = trk.composite(fread, x, ids, G, above, skipna, steps, resident_f64=dtype == np.float64)
    else:
        xread = x
        if x is not None and not callable(x):
            def xread(t0, nt, out, slab=x):
                out[...] = slab[t0:t0 + nt]
        s, n = trk.composite_cb(fread, xread, shape, dtype, ids, G, above, skipna, steps)
    return (s[0], n[0]) if group is None else (s, n)


def lon_sector(lon, west, east):
    """the columns of a longitude sector as band_numpy takes them: (x0, len), the len columns x0, x0 + 1, ... modulo nx whose longitude
    lies between `west` and `east` going EAST from west.  lon: the longitude coordinate, ascending, on a 0...360 or a -180...180 grid;
    the bounds may use either convention (all values are compared modulo 360); west > east is a sector that wraps, bounds a whole
    turn apart (0 and 360, -180 and 180) are the full circle, west == east is the one column at that longitude.  ValueError for a
    sector that selects no column."""
    lon = np.asarray(lon, dtype=np.float64).reshape(-1)
    west, east = float(west), float(east)
    if lon.size == 0 or not (np.isfinite(west) and np.isfinite(east)) or np.any(np.diff(lon) <= 0):
        raise ValueError("lon must be a non-empty ascending coordinate and the bounds finite")
    span = east - west
    span = 360.0 if (span != 0 and span % 360.0 == 0) else span % 360.0
    sel = np.mod(lon - west, 360.0) <= span
    n = int(np.count_nonzero(sel))
    if n == 0:
        raise ValueError("the sector ({}, {}) selects no column".format(west, east))
    if n == lon.size:
        return 0, n
    first = np.nonzero(sel & ~np.roll(sel, 1))[0]
    if len(first) != 1:
        raise ValueError("the sector ({}, {}) does not select neighbouring columns of this longitude coordinate".format(west, east))
    return int(first[0]), n


def band_total(weights, rows, sectors=None):
    """what band_numpy gives where every pixel of the band is flagged -- the denominator of a fraction: the float64 sum of
    weights[y0:y1] in rising y (one column), or with sectors the (nsect,) sums of that value over each sector's len columns"""
    w = np.asarray(weights, dtype=np.float64)
    y0, y1 = (int(v) for v in rows)
    col = np.float64(0.0)
    for y in range(y0, y1):
        col = col + w[y]
    if sectors is None:
        return col
    out = np.zeros(len(sectors), dtype=np.float64)
    for s, (_x0, ln) in enumerate(sectors):
        for _ in range(int(ln)):
            out[s] = out[s] + col
    return out


def band_fraction(area, total):
    """area / total in float64 (total: band_total's scalar, or its (nsect,) array against (..., nsect) areas); numpy's NaN / inf
    where the total is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(area, dtype=np.float64) / np.asarray(total, dtype=np.float64)


def band_numpy(flag, rows, weights, x=None, sectors=None, columns=True, above=0, chunk_steps=None, device=None, shape=None, dtype=None,
               resident_gen=None):
    """the reductions over space that keep the time axis, on a (time, lat, lon) integer flag slab: per time step t and column c, over
    the latitude rows [y0, y1) = `rows` with flag > above,
        cnt[t, c] (uint32) how many,  area[t, c] the float64 sum of weights[y] IN RISING y,  wx[t, c] that of weights[y] * x[t, y, c]
    (wx only with a field x of the same shape: float64 stays, everything else is taken as float32; a value at an unflagged pixel
    reaches nothing, a NaN at a flagged one propagates) -- the columns of a time-longitude (Hovmoeller) diagram -- and per sector
    (x0, len) of `sectors` (see lon_sector; the columns x0, x0 + 1, ... modulo nx) sec_cnt, sec_area, sec_wx[t, s]: the column
    values added in that column order -- a blocked-area series.  weights: float64 (ny,), e.g. row_weights(lat, dlat, dlon) for km^2.
    Returns a dict of (T, nx) and (T, nsect) arrays; columns=False: the sector tables only (the column tables then never leave the
    device).  The sums run on the GPU (ctk_band_*) and are the same bits whatever chunk_steps: time steps per chunk on the slabs' way
    through the device (None or 0: about 256 MB).  With shape=(T, ny, nx) (and dtype for a field) flag and x may be readers
    reader(t0, nt, out) (ctk_band_cb); flags wider than int32 are narrowed chunk by chunk (an id beyond int32 raises ValueError).
    resident_gen: the field is the anomaly slab calc_anom left on the device (`dtype` its type) of that generation
    (Tracker.resident_generation()); only the flags travel, and a slab that was replaced since is refused."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    if steps < 0:
        raise ValueError("chunk_steps={} (at least 0)".format(steps))
    if callable(flag) or callable(x):
        if shape is None or (callable(x) and dtype is None):
            raise ValueError("a reader needs shape=(T, ny, nx) and the field's dtype")
    fread, fshape, is_array = _flag_source(flag, shape)
    shape = tuple(int(v) for v in (fshape if shape is None else shape))
    if x is not None and not callable(x):
        x = x if isinstance(x, np.memmap) else np.asarray(x)
        if tuple(x.shape) != shape:
            raise ValueError("the field has shape {}, the flag {}".format(x.shape, shape))
        dtype = _native._field_dtype(x.dtype)
    dtype = np.dtype(dtype if dtype is not None else np.float32)
    _native._band_args(shape[0], shape[1], shape[2], rows, weights, sectors, columns, above)
    trk = _tracker(device)
    if is_array and not callable(x):
        return trk.band(fread, rows, weights, x, sectors, columns, above, steps, resident_gen=resident_gen, resident_f64=dtype == np.float64)
    xread = x
    if x is not None and not callable(x):
        def xread(t0, nt, out, slab=x):
            out[...] = slab[t0:t0 + nt]
    return trk.band_cb(fread, xread, shape, dtype, rows, weights, sectors, columns, above, steps, resident_gen=resident_gen)


def centred_stamps(t, row, col, bin=None):
    """the stamps of a block-centred composite as the library takes them: (t int64, row, col, bin int32) sorted STABLY by t -- the
    given order is kept among equal t -- which is the order of the additions.  bin None: one bin (all zeros)."""
    t = np.asarray(t)
    if t.ndim != 1:
        raise ValueError("t must be one-dimensional")
    arrs = [t, np.asarray(row), np.asarray(col), np.zeros(t.shape, dtype=np.int32) if bin is None else np.asarray(bin)]
    for name, a in zip(("t", "row", "col", "bin"), arrs):
        if a.shape != t.shape:
            raise ValueError("t, row, col and bin must have one length: {} has shape {}, t {}".format(name, a.shape, t.shape))
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("{} must be integers (dtype {})".format(name, a.dtype))
    order = np.argsort(arrs[0], kind="stable")
    return tuple(a[order] for a in arrs)


def centred_numpy(x, t, row, col, bin=None, nbins=None, half=(0, 0), wrap=True, skipna=False, chunk_steps=None, device=None, shape=None, dtype=None):
    """the composite of a float field in a window that moves with a list of stamps: (sum, n), both (nbins, 2 hy + 1, 2 hx + 1) with
    half = (hy, hx) in grid points.  For every stamp r with bin[r] >= 0, in time order (stamps of one time step in the order
    given), and every j in -hy..hy, i in -hx..hx, sum[bin[r], j + hy, i + hx] += float64(x[t[r], row[r] + j, col[r] + i]) and n
    += 1; a row outside the grid is not counted (no step over a pole), a column outside it is wrapped (wrap, the default: longitude
    is periodic) or not counted, with skipna a NaN is not counted.  composite_mean(sum, n) is the mean.  The sums run on the GPU
    (ctk_centred_*), are float64 added in that fixed order and so the same bits whatever chunk_steps: time steps per chunk on the
    field's way through the device (None or 0: about 256 MB); chunks without stamps and latitude rows no window touches do not
    travel.  x: an array (np.memmap included; float64 stays, everything else is taken as float32), a reader reader(t0, nt, out)
    with shape=(T, ny, nx) and dtype -- it is not called for a chunk without stamps -- or None: the anomaly slab calc_anom left
    on the device (`dtype` its type).  bin None: one bin; nbins None: max(bin) + 1."""
    steps = 0 if chunk_steps is None else int(chunk_steps)
    hy, hx = half
    if callable(x) and (shape is None or dtype is None):
        raise ValueError("a reader needs shape=(T, ny, nx) and the field's dtype")
    t, row, col, bin = centred_stamps(t, row, col, bin)
    if nbins is None:
        nbins = max(int(bin.max()) + 1, 1) if bin.size else 1
    trk = _tracker(device)
    if callable(x):
        return trk.centred_cb(x, shape, np.dtype(dtype), t, row, col, bin, nbins, hy, hx, wrap, skipna, steps)
    if x is None:
        return trk.centred(None, t, row, col, bin, nbins, hy, hx, wrap, skipna, steps, resident_f64=np.dtype(dtype if dtype is not None else np.float32) == np.float64,
                           shape=shape)
    x = x if isinstance(x, np.memmap) else np.asarray(x)
    if x.ndim != 3:
        raise ValueError("the field must be (time, lat, lon)")
    if isinstance(x, np.memmap) and (x.dtype != _native._field_dtype(x.dtype) or not x.flags.c_contiguous):
        def reader(t0, nt, out, slab=x):                   # (converted chunk by chunk, never as a whole)
            out[...] = slab[t0:t0 + nt]
        return trk.centred_cb(reader, x.shape, _native._field_dtype(x.dtype), t, row, col, bin, nbins, hy, hx, wrap, skipna, steps)
    return trk.centred(x, t, row, col, bin, nbins, hy, hx, wrap, skipna, steps)


def lifecycle_bins(block, step, by, nbins=None, max_age=None):
    """(bin int32, nbins): the life-cycle age bin of every row of a life-cycle frame (or a selection of it), for centred_numpy.
    block: a hashable key per row (the Flag, or (Flag, member) as a sequence of tuples or an (R, 2) array); step: the row's
    position on the time axis.  Per block, among the rows given: age = step - the block's first step, duration = last step - first
    step + 1.
      by='age'         bin = age (time steps since onset); rows beyond max_age get -1 (dropped).  max_age defaults to nbins - 1 if
                       nbins is given, else to the largest age present; nbins = max_age + 1
      by='to_lysis'    bin = the block's last step - step (time steps before decay), capped the same way
      by='normalized'  bin = (age * nbins) // duration in integers: nbins equal parts of the life cycle (nbins is required; a block
                       shorter than nbins steps leaves bins empty)
      by=None          one bin
      by an integer array: taken as given; negative means dropped; nbins defaults to max + 1"""
    step = np.asarray(step)
    if step.ndim != 1 or (step.size and step.dtype.kind not in "iu"):
        raise ValueError("step must be a one-dimensional integer array")
    step = step.astype(np.int64)
    R = step.shape[0]
    if by is None:
        return np.zeros(R, dtype=np.int32), 1
    if not isinstance(by, str):
        b = np.asarray(by)
        if b.shape != step.shape or (b.size and b.dtype.kind not in "iu"):
            raise ValueError("by as an array must hold one integer per row")
        if nbins is None:
            nbins = max(int(b.max()) + 1, 1) if R else 1
        if R and (int(b.max()) >= nbins or int(b.min()) < np.iinfo(np.int32).min):
            raise ValueError("a bin of {} with nbins = {}".format(int(b.max()), nbins))
        return b.astype(np.int32), int(nbins)
    if by not in ("age", "to_lysis", "normalized"):
        raise ValueError("by must be None, 'age', 'to_lysis', 'normalized' or an integer array, not {!r}".format(by))
    keys = block.tolist() if isinstance(block, np.ndarray) else list(block)
    keys = [tuple(k) if isinstance(k, (list, tuple, np.ndarray)) else k for k in keys]
    if len(keys) != R:
        raise ValueError("block has {} keys, step {} rows".format(len(keys), R))
    seen = {}
    code = np.array([seen.setdefault(k, len(seen)) for k in keys], dtype=np.int64)
    first = np.full(len(seen), np.iinfo(np.int64).max, dtype=np.int64)
    last = np.full(len(seen), np.iinfo(np.int64).min, dtype=np.int64)
    np.minimum.at(first, code, step)
    np.maximum.at(last, code, step)
    age = step - first[code] if R else step
    if by == "normalized":
        if nbins is None or int(nbins) < 1:
            raise ValueError("by='normalized' needs nbins >= 1")
        nbins = int(nbins)
        b = (age * nbins) // (last[code] - first[code] + 1) if R else age
        return b.astype(np.int32), nbins
    b = age if by == "age" else (last[code] - step if R else step)
    if max_age is None:
        max_age = int(nbins) - 1 if nbins is not None else (int(b.max()) if R else 0)
    max_age = int(max_age)
    if max_age < 0 or max_age >= np.iinfo(np.int32).max:
        raise ValueError("max_age = {}".format(max_age))
    if nbins is not None and int(nbins) != max_age + 1:
        raise ValueError("nbins = {} but max_age + 1 = {}".format(nbins, max_age + 1))
    return np.where(b > max_age, -1, b).astype(np.int32), max_age + 1


def anomalies_numpy(x, group, ngroups=None, window=1, smooth=1, clim=None, segments=None, chunk_steps=None, device=None):
    """calc_clim / calc_anom on a (time, lat, lon) float slab: `group` holds one id in [0, G) per timestep (G = ngroups, or
    max(group) + 1), the climatology is the mean per group smoothed over `window` groups (or `clim`, (G, ny, nx)), the anomaly is
    smoothed over `smooth` timesteps.  Returns (anom, clim) in the slab's dtype (float32 kept, anything else float64).
    segments: int array of segment starts (0 first, strictly increasing) -- the smoothing does not cross a break (NaN where its
    window would), the climatology is pooled over every segment.  chunk_steps: stream the slab (an array or np.memmap the host
    holds) through chunk-sized device buffers, that many time steps at a time (0: about 256 MB each); same bits."""
    x = np.asarray(x) if not isinstance(x, np.memmap) else x
    if x.ndim != 3:
        raise ValueError("x must be (time, lat, lon)")
    if x.dtype.kind != "f":
        if x.dtype.kind not in "iub":
            raise TypeError("x must be a real numeric array")
        x = x.astype(np.float64)
    if group is None:
        raise ValueError("group must hold one id per timestep")
    ids, G = _native._groups(group, x.shape[0], ngroups)
    starts = None if segments is None else segment_starts(segments, x.shape[0])
    trk = _tracker(device)
    if chunk_steps is None:
        return trk.anomalies(x, ids, G, window=window, smooth=smooth, clim=clim, want_clim=True, segments=starts)
    return trk.anomalies_stream(x, ids, G, window=window, smooth=smooth, clim=clim, chunk_steps=int(chunk_steps), segments=starts, want_clim=True)


def lanczos_weights(ntaps, cutoff, cutoff2=None, kind='lowpass'):
    """float64 weights of a Lanczos filter of `ntaps` (odd) taps, Duchon (1979): with n = (ntaps - 1) / 2 and k = -n .. n,
        w[k] = sin(2 pi fc k) / (pi k) * sin(pi k / (n + 1)) / (pi k / (n + 1)),   w[0] = 2 fc
    for the cut-off frequency fc in cycles per step (0 < fc <= 0.5).  kind 'lowpass': those weights normalised to sum 1;
    'highpass': a unit impulse at the centre minus the low-pass; 'bandpass': the low-pass of the higher of cutoff / cutoff2 minus
    the low-pass of the lower (passes the periods between 1 / higher and 1 / lower steps).  Host numpy."""
    if int(ntaps) != ntaps or ntaps < 1 or int(ntaps) % 2 == 0:
        raise ValueError("ntaps must be an odd positive integer, got {}".format(ntaps))
    if kind not in ('lowpass', 'highpass', 'bandpass'):
        raise ValueError("kind must be 'lowpass', 'highpass' or 'bandpass'")
    if (kind == 'bandpass') != (cutoff2 is not None):
        raise ValueError("cutoff2 is the second cut-off of kind='bandpass' (and only of it)")

    def low(fc):
        if not 0.0 < fc <= 0.5:
            raise ValueError("a cut-off is a frequency in cycles per step, 0 < fc <= 0.5, got {}".format(fc))
        n = (int(ntaps) - 1) // 2
        k = np.arange(-n, n + 1, dtype=np.float64)
        k[n] = 1.0                                           # (the centre is set below)
        w = np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * (np.sin(np.pi * k / (n + 1)) / (np.pi * k / (n + 1)))
        w[n] = 2.0 * fc
        return w / w.sum()
    if kind == 'bandpass':
        lo, hi = sorted((float(cutoff), float(cutoff2)))
        return low(hi) - low(lo)
    w = low(float(cutoff))
    if kind == 'highpass':
        w = -w
        w[(int(ntaps) - 1) // 2] += 1.0
    return w


def filter_layout(T, weights, stride=1, offset=None, segments=None):
    """where the outputs of time_filter_numpy lie: (label_steps, out_starts, first) -- per output its label step (tap K // 2) and the
    step of tap 0, per segment its first output.  weights: the taps or an int K.  Host only."""
    _, K = _native._filter_weights(weights)
    first, label, out_starts = _native.filter_layout(T, K, stride, offset, None if segments is None else segment_starts(segments, T))
    return label, out_starts, first


def time_filter_numpy(x, weights, stride=1, offset=None, edges='nan', skipna=False, segments=None, chunk_steps=None, device=None, shape=None, dtype=None,
                      layout=False):
    """a weighted filter or a block mean along the time axis of a (time, lat, lon) float slab on the GPU.  weights: the K taps
    (lanczos_weights, or any float64 array), or an int K: the plain mean of K steps.  Output q of a segment covers the steps
    S + offset + q * stride + (0 .. K - 1) and is labelled with the step of tap K // 2; it exists where that step lies in the
    segment.  offset None: -(K // 2) at stride 1 -- one output per step, the centred window of calc_anom's `smooth` --, 0 at a
    larger stride: blocks counted from the segment start (6-hourly to daily: weights=4, stride=4).
    edges: 'nan' -- an output whose window leaves its segment is NaN; 'renorm' -- the taps inside are used and the sum is divided
    by the sum of their weights (weights >= 0 only).  skipna: NaN taps are left out in the same way.  segments: int array of
    segment starts; no window crosses a break.  chunk_steps: stream the slab (an array, np.memmap, or a reader(t0, nt, out) with
    `shape` and `dtype`) through chunk-sized device buffers (0: about 256 MB each); same bits.
    Returns the (T_out, lat, lon) array in the slab's dtype, or (array, label_steps, out_starts) with layout=True."""
    trk = _tracker(device)
    if callable(x):
        if shape is None:
            raise ValueError("a reader needs shape=(T, ny, nx) and dtype")
        T = int(shape[0])
    else:
        x = np.asarray(x) if not isinstance(x, np.memmap) else x
        if x.ndim != 3:
            raise ValueError("x must be (time, lat, lon)")
        if x.dtype.kind != "f":
            if x.dtype.kind not in "iub":
                raise TypeError("x must be a real numeric array")
            x = x.astype(np.float64)
        T = x.shape[0]
    starts = None if segments is None else segment_starts(segments, T)
    if callable(x):
        out = trk.time_filter_cb(x, shape, dtype, weights, stride=stride, offset=offset, edges=edges, skipna=skipna, segments=starts,
                                 chunk_steps=int(chunk_steps or 0))
    else:
        out = trk.time_filter(x, weights, stride=stride, offset=offset, edges=edges, skipna=skipna, segments=starts, chunk_steps=chunk_steps)
    if not layout:
        return out
    label, out_starts, _ = filter_layout(T, weights, stride, offset, starts)
    return out, label, out_starts


def level_weights(levels, bounds=None):
    """float64 weights of a vertical mean over a level coordinate (one per level, 0: not selected): the levels p with
    min(bounds) <= p <= max(bounds) (bounds None: all of them) get the trapezoid rule over the selected levels in coordinate order --
    half the distance to each selected neighbour --, so that the weighted mean is the integral of x dp / (p_bottom - p_top), the
    vertical average of Schwierz et al. (2004) that README.rst:235-240 of the reference cites.  A single selected level gets 1.0.
    `levels` must be strictly monotonic, in either direction."""
    p = np.asarray(levels, dtype=np.float64)
    if p.ndim != 1 or p.size < 1:
        raise ValueError("levels must be a 1-D coordinate")
    d = np.diff(p)
    if not np.all(np.isfinite(p)) or (p.size > 1 and not (np.all(d > 0) or np.all(d < 0))):
        raise ValueError("the level coordinate must be strictly monotonic")
    if bounds is None:
        idx = np.arange(p.size)
    else:
        b = np.asarray(bounds, dtype=np.float64).reshape(-1)
        if b.size != 2:
            raise ValueError("bounds must be two values")
        idx = np.flatnonzero((p >= b.min()) & (p <= b.max()))
    if idx.size == 0:
        raise ValueError("bounds {} select no level of {}".format(tuple(np.asarray(bounds).tolist()), p.tolist()))
    w = np.zeros(p.size, dtype=np.float64)
    if idx.size == 1:
        w[idx[0]] = 1.0
        return w
    half = np.abs(np.diff(p[idx])) / 2                      # (a monotonic coordinate: the selected levels are neighbours)
    w[idx[:-1]] += half
    w[idx[1:]] += half
    return w


def _vertical_weights(weights, levels, bounds, nlev):
    """the weights argument of level_mean_numpy / calc_vertical_mean as nlev float64 values: an array is taken as it is, 'equal'
    gives 1.0 on every level that `bounds` selects on `levels`, 'pressure' (None with levels) the trapezoid rule (level_weights)"""
    if weights is None:
        weights = 'equal' if levels is None else 'pressure'
    if isinstance(weights, str):
        if weights not in ('equal', 'pressure'):
            raise ValueError("weights={!r}: 'pressure', 'equal' or one value per level".format(weights))
        if levels is None:
            if weights == 'pressure' or bounds is not None:
                raise ValueError("weights='pressure' and bounds need the level coordinate (levels=)")
            return np.ones(nlev, dtype=np.float64)
        w = level_weights(levels, bounds)
        if w.shape[0] != nlev:
            raise ValueError("levels holds {} values, the field has {} levels".format(w.shape[0], nlev))
        return (w > 0).astype(np.float64) if weights == 'equal' else w
    return _native._level_weights(weights, nlev)


def level_mean_numpy(x, weights=None, levels=None, bounds=None, skipna=False, chunk_steps=None, device=None, shape=None, dtype=None):
    """the vertical mean of README.rst:235-240 ("vertically averaged between 500-150 hPa") on a (steps, level, lat, lon) float field:
        sum over the selected levels l of w[l] * x[:, l] / sum of those w[l]        (float64, rising l; include/contrack_hip.h)
    on the GPU (ctk_level_mean_*).  weights: one value >= 0 per level (0: the level is not selected -- never read, never uploaded),
    'equal', or 'pressure' (the default with levels=: level_weights(levels, bounds)); without levels every level counts equally.
    skipna: a NaN level of a pixel leaves both sums.  x: an array or np.memmap, or -- with shape=(steps, nsel, ny, nx) and dtype -- a
    reader(t0, nt, out) that fills out (nt, nsel, ny, nx) with the SELECTED levels only, in rising level order.  chunk_steps: steps
    per chunk on their way through the device (0: about 256 MB of input); same bits.  Returns (steps, lat, lon) in x's dtype
    (float32 kept, anything else float64)."""
    if callable(x):
        if shape is None or dtype is None:
            raise ValueError("a reader needs shape=(steps, nsel, ny, nx) and dtype")
        if len(shape) != 4:
            raise ValueError("shape must be (steps, nsel, ny, nx)")
        nsel = int(shape[1])
        w = _vertical_weights(weights, levels, bounds, nsel if levels is None else len(np.asarray(levels)))
        w = w[w > 0]
        if w.shape[0] != nsel:
            raise ValueError("the reader delivers {} levels, the weights select {}".format(nsel, w.shape[0]))
        return _tracker(device).level_mean_cb(x, shape, dtype, w, skipna=skipna, chunk_steps=0 if chunk_steps is None else int(chunk_steps))
    x = np.asarray(x) if not isinstance(x, np.memmap) else x
    if x.ndim != 4:
        raise ValueError("x must be (steps, level, lat, lon)")
    if x.dtype.kind != "f":
        if x.dtype.kind not in "iub":
            raise TypeError("x must be a real numeric array")
        x = x.astype(np.float64)
    w = _vertical_weights(weights, levels, bounds, x.shape[1])
    return _tracker(device).level_mean(x, w, skipna=skipna, chunk_steps=None if chunk_steps is None else int(chunk_steps))


_HEMISPHERES = ('both', 'north', 'south')
_REVERSAL_STATS = ('gradient', 'mask')


def reversal_rows(lat, delta=15., lat_bounds=(30, 75), hemisphere='both', second=False):
    """the partner rows of the gradient-reversal index on the latitude coordinate `lat` (degrees, rising or falling, regular or
    not), as a dict of (ny,) arrays.  Per row j with s = +1 where lat[j] > 0, else -1 (poleward is +s):
        eq[j]   the row nearest to lat[j] - s * delta        po[j]   the row nearest to lat[j] + s * delta
        eq2[j]  the row nearest to lat[j] - 2 * s * delta    (second=True: the third criterion; else eq2 is None)
    "nearest" accepts a row only if it lies closer to the target than half the largest row spacing; otherwise the row has no
    partner (nor does a partner count that is the row itself: a delta below the spacing).  A row is ACTIVE if lat_bounds[0] <= |lat[j]| <= lat_bounds[1], its hemisphere is selected ('both', 'north': lat > 0,
    'south': lat < 0) and every partner it needs exists; inactive rows have eq = po = eq2 = -1.  float64 per active row (0
    elsewhere): dE = |lat[j] - lat[eq]|, dP = |lat[po] - lat[j]|, dE2 = |lat[eq] - lat[eq2]| -- the actual distances, not delta."""
    lat = np.asarray(lat, dtype=np.float64)
    if lat.ndim != 1 or lat.size < 1 or not np.all(np.isfinite(lat)):
        raise ValueError("lat must be a 1-D coordinate of finite values")
    if not (np.isfinite(delta) and delta > 0):
        raise ValueError("delta must be a distance in degrees > 0, not {!r}".format(delta))
    if hemisphere not in _HEMISPHERES:
        raise ValueError("hemisphere={!r}: one of {}".format(hemisphere, _HEMISPHERES))
    b = np.asarray(lat_bounds, dtype=np.float64).reshape(-1)
    if b.size != 2 or not np.all(np.isfinite(b)) or b[0] > b[1] or b[0] < 0:
        raise ValueError("lat_bounds must be (low, high) with 0 <= low <= high, in degrees of |latitude|")
    ny = lat.size
    half = np.abs(np.diff(lat)).max() / 2 if ny > 1 else 0.0

    def nearest(v):
        k = int(np.argmin(np.abs(lat - v)))
        return k if abs(lat[k] - v) < half else -1
    eq, po, eq2 = (np.full(ny, -1, dtype=np.int32) for _ in range(3))
    dE, dP, dE2 = (np.zeros(ny, dtype=np.float64) for _ in range(3))
    for j in range(ny):
        phi = lat[j]
        if not (b[0] <= abs(phi) <= b[1]) or (hemisphere == 'north' and not phi > 0) or (hemisphere == 'south' and not phi < 0):
            continue
        s = 1.0 if phi > 0 else -1.0
        e, p = nearest(phi - s * delta), nearest(phi + s * delta)
        e2 = nearest(phi - 2 * s * delta) if second else 0
        if e < 0 or p < 0 or e2 < 0 or e == j or p == j or (second and e2 == e):
            continue
        eq[j], po[j] = e, p
        dE[j], dP[j] = abs(lat[j] - lat[e]), abs(lat[p] - lat[j])
        if second:
            eq2[j], dE2[j] = e2, abs(lat[e] - lat[e2])
    return dict(eq=eq, po=po, eq2=eq2 if second else None, dE=dE, dP=dP, dE2=dE2 if second else None)


def reversal_limits(rows, ghgs=0., ghgn=-10., ghgs2=None):
    """the row table of ctk_reversal_* from reversal_rows' partners and the gradient limits per degree: the limits pre-multiplied by
    the row distances, tS = ghgs * dE, tN = ghgn * dP and (ghgs2 not None: Davini's third criterion, -5) tS2 = ghgs2 * dE2, so that
    the compares of the kernel need no division"""
    for name, v in (("ghgs", ghgs), ("ghgn", ghgn)) + ((("ghgs2", ghgs2),) if ghgs2 is not None else ()):
        if not np.isfinite(v):
            raise ValueError("{} must be finite, not {!r}".format(name, v))
    if (ghgs2 is not None) != (rows.get("eq2") is not None):
        raise ValueError("ghgs2 needs the rows of the third criterion: reversal_rows(..., second=True), and only then")
    out = dict(eq=rows["eq"], po=rows["po"], eq2=rows["eq2"], dE=rows["dE"], tS=np.float64(ghgs) * rows["dE"], tN=np.float64(ghgn) * rows["dP"], tS2=None)
    if ghgs2 is not None:
        out["tS2"] = np.float64(ghgs2) * rows["dE2"]
    return out


def reversal_numpy(z, lat, delta=15., ghgs=0., ghgn=-10., ghgs2=None, lat_bounds=(30, 75), hemisphere='both', stat='gradient', chunk_steps=None,
                   device=None, shape=None, dtype=None):
    """the two-dimensional blocking index of the reversal of the meridional height gradient (Tibaldi & Molteni 1990; Scherrer et al.
    2006; Davini et al. 2012) of a (steps, lat, lon) float field z -- geopotential height in metres, say -- on the GPU
    (ctk_reversal_*).  Per pixel of an active row (reversal_rows), in float64:
        dS = z[j] - z[eq] ;  dN = z[po] - z[j] ;  dS2 = z[eq] - z[eq2]
        blocked = dS / dE > ghgs  and  dN / dP < ghgn  [and dS2 / dE2 < ghgs2]        (evaluated as dS > ghgs * dE ...: no division)
    stat='gradient': dS / dE where blocked (units per degree), 0 elsewhere; stat='mask': 1 / 0.  Inactive rows are 0; a NaN in any of
    the rows a pixel reads leaves it unblocked.  ghgs2=-5 is Davini's third criterion.  The result has z's shape and dtype (float32
    kept, anything else float64): track_numpy(..., threshold=0, gorl='>') tracks it as it is.
    z: an array or np.memmap, or -- with shape=(steps, ny, nx) and dtype -- a reader(t0, nt, out) that fills out (nt, ny, nx).
    chunk_steps: steps per chunk on their way through the device (None / 0: about 256 MB of input); same bits.
    The one-dimensional diagram of Tibaldi & Molteni is band_numpy / calc_hovmoller over a narrow latitude band of the mask."""
    if stat not in _REVERSAL_STATS:
        raise ValueError("stat={!r}: one of {}".format(stat, _REVERSAL_STATS))
    if chunk_steps is not None and int(chunk_steps) < 0:
        raise ValueError("chunk_steps must be >= 0")
    rows = reversal_limits(reversal_rows(lat, delta, lat_bounds, hemisphere, ghgs2 is not None), ghgs, ghgn, ghgs2)
    ny = len(rows["eq"])
    if callable(z):
        if shape is None or dtype is None or len(shape) != 3:
            raise ValueError("a reader needs shape=(steps, ny, nx) and dtype")
        if int(shape[1]) != ny:
            raise ValueError("lat holds {} values, the field has {} rows".format(ny, shape[1]))
        return _tracker(device).reversal_cb(z, shape, dtype, rows, mask=stat == 'mask', chunk_steps=chunk_steps or 0)
    z = np.asarray(z) if not isinstance(z, np.memmap) else z
    if z.ndim != 3:
        raise ValueError("z must be (steps, lat, lon)")
    if z.shape[1] != ny:
        raise ValueError("lat holds {} values, the field has {} rows".format(ny, z.shape[1]))
    if z.dtype.kind != "f":
        if z.dtype.kind not in "iub":
            raise TypeError("z must be a real numeric array")
        z = z.astype(np.float64)
    return _tracker(device).reversal(z, rows, mask=stat == 'mask', chunk_steps=chunk_steps or 0)


_LWA_PARTS = ('total', 'anticyclonic', 'cyclonic')


def lwa_rows(lat, lat_bounds=(30, 75), hemisphere='both', radius=6.371e6):
    """the row table of the local wave activity (ctk_lwa_*) on the latitude coordinate `lat` (degrees; rising, falling or in any
    order, regular or not), as a dict:
        ndom, dom_off (ndom + 1), dom_rows   one or two DOMAINS ('north': the rows with lat >= 0, 'south': lat <= 0, 'both': north
                                             then south), each the row indices sorted by |lat|: from the equator side to the pole;
                                             an equator row is in both
        W (ny,) uint32    rint(max(cos(lat), 0) * 2^30): the area weight of a pixel of the row (a pole row: 0)
        q (ny,) float64   max(cos(lat), 0) * dphi, dphi the trapezoid width of the row inside its domain in radians: half the
                          distance between its two neighbours, at both ends half the distance to the one neighbour (an equator
                          row takes the width it has in the first domain)
        S (ny,) float64   radius / cos(lat) on ACTIVE rows, 0 elsewhere (radius 6.371e6: a height in m gives m^2)
        active (ny,) uint8   lat_bounds[0] <= |lat| <= lat_bounds[1], 0 < lat_bounds[0], inside a requested domain
    ValueError if the band reaches a pole row: no area lies poleward of it (W = 0), so it has no equivalent latitude."""
    lat = np.asarray(lat, dtype=np.float64)
    if lat.ndim != 1 or lat.size < 1 or not np.all(np.isfinite(lat)) or np.any(np.abs(lat) > 90):
        raise ValueError("lat must be a 1-D coordinate of finite values within [-90, 90]")
    if hemisphere not in _HEMISPHERES:
        raise ValueError("hemisphere={!r}: one of {}".format(hemisphere, _HEMISPHERES))
    b = np.asarray(lat_bounds, dtype=np.float64).reshape(-1)
    if b.size != 2 or not np.all(np.isfinite(b)) or b[0] > b[1] or not b[0] > 0:
        raise ValueError("lat_bounds must be (low, high) with 0 < low <= high, in degrees of |latitude|")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be a length > 0, not {!r}".format(radius))
    ny = lat.size
    cosl = np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    W = np.rint(cosl * 2.0 ** 30).astype(np.uint32)
    q, S, active, seen = np.zeros(ny), np.zeros(ny), np.zeros(ny, dtype=np.uint8), np.zeros(ny, dtype=bool)
    doms = []
    for name, inside in (('north', lat >= 0), ('south', lat <= 0)):
        if hemisphere not in ('both', name):
            continue
        idx = np.flatnonzero(inside)
        if not idx.size:
            raise ValueError("lat has no row in the {}ern hemisphere".format(name))
        dom = idx[np.argsort(np.abs(lat[idx]), kind='stable')]
        phi = np.deg2rad(np.abs(lat[dom]))
        dphi = np.zeros(dom.size)
        if dom.size > 1:
            dphi[1:-1] = (phi[2:] - phi[:-2]) / 2
            dphi[0], dphi[-1] = (phi[1] - phi[0]) / 2, (phi[-1] - phi[-2]) / 2
        new = ~seen[dom]
        q[dom[new]] = cosl[dom[new]] * dphi[new]
        seen[dom] = True
        act = dom[(np.abs(lat[dom]) >= b[0]) & (np.abs(lat[dom]) <= b[1])]
        poleward = np.cumsum(W[dom][::-1].astype(np.uint64))[::-1]                  # the area weight of a row and of those poleward of it
        empty = dom[(poleward == 0) & np.isin(dom, act)]
        if empty.size:
            raise ValueError("lat_bounds {} reach the pole row(s) at latitude {}: no area lies poleward of them, so they have no equivalent "
                             "latitude; end the band below the pole".format(tuple(b.tolist()), lat[empty].tolist()))
        active[act] = 1
        S[act] = np.float64(radius) / np.cos(np.deg2rad(lat[act]))
        doms.append(dom.astype(np.int32))
    return dict(ndom=len(doms), dom_off=np.concatenate([[0], np.cumsum([d.size for d in doms])]).astype(np.int32), dom_rows=np.concatenate(doms),
                active=active, W=W, q=q, S=S)


def lwa_numpy(z, lat, lat_bounds=(30, 75), hemisphere='both', radius=6.371e6, part='total', chunk_steps=None, device=None, return_reference=False,
              shape=None, dtype=None):
    """finite-amplitude local wave activity (Huang & Nakamura 2016; Chen, Lu, Burrows & Leung 2015; Martineau et al. 2017; Nakamura
    & Huang 2018) of a (steps, lat, lon) float field z on the GPU (ctk_lwa_*).  z is a height field that FALLS towards the pole --
    500 hPa geopotential height in metres, say; for a field that rises towards the pole, such as PV, pass its negative.  Per step,
    hemisphere and active row j (lwa_rows): Z_j is the contour whose poleward area equals that of the cap poleward of row j
    (exactly, by area-weighted selection among the hemisphere's pixels); per column, a = the integral of z - Z_j over the rows
    poleward of j (j included) where z > Z_j (anticyclonic: a ridge displaced poleward), y = the integral of Z_j - z over the rows
    equatorward of j where z < Z_j (cyclonic), both a cos(lat) dphi in float64; the result is radius / cos(lat_j) times a + y
    (part='total'), a ('anticyclonic': what blocks are made of) or y ('cyclonic').  Inactive rows are 0; a row whose contour the
    NaNs of the plane make unreachable is NaN.  The result has z's shape and dtype (float32 kept, anything else float64):
    track_numpy(..., threshold=<a percentile of it>, gorl='>') tracks it as it is.
    z: an array or np.memmap, or -- with shape=(steps, ny, nx) and dtype -- a reader(t0, nt, out) that fills out (nt, ny, nx).
    chunk_steps: steps per chunk on their way through the device (None / 0: about 256 MB of input); same bits.
    return_reference: returns (lwa, ref), ref (steps, ny) the contours Z_j (0 on inactive rows)."""
    if part not in _LWA_PARTS:
        raise ValueError("part={!r}: one of {}".format(part, _LWA_PARTS))
    if chunk_steps is not None and int(chunk_steps) < 0:
        raise ValueError("chunk_steps must be >= 0")
    rows = lwa_rows(lat, lat_bounds, hemisphere, radius)
    ny = len(rows["W"])
    if callable(z):
        if shape is None or dtype is None or len(shape) != 3:
            raise ValueError("a reader needs shape=(steps, ny, nx) and dtype")
        if int(shape[1]) != ny:
            raise ValueError("lat holds {} values, the field has {} rows".format(ny, shape[1]))
        return _tracker(device).lwa_cb(z, shape, dtype, rows, part=part, chunk_steps=chunk_steps or 0, want_ref=return_reference)
    z = np.asarray(z) if not isinstance(z, np.memmap) else z
    if z.ndim != 3:
        raise ValueError("z must be (steps, lat, lon)")
    if z.shape[1] != ny:
        raise ValueError("lat holds {} values, the field has {} rows".format(ny, z.shape[1]))
    if z.dtype.kind != "f":
        if z.dtype.kind not in "iub":
            raise TypeError("z must be a real numeric array")
        z = z.astype(np.float64)
    return _tracker(device).lwa(z, rows, part=part, chunk_steps=chunk_steps or 0, want_ref=return_reference)


def percentile_groups_numpy(anom, rows, group, q, window=1, device=None):
    """the threshold recipe of README.rst:235-240 on a (time, lat, lon) float slab: per group g (one id in [0, G) per timestep,
    G = max(group) + 1, any order in time) the q-quantile of rows[0] <= y < rows[1] pooled over every timestep whose group lies in
    the centred window of `window` groups around g, circular over the groups:
        np.nanquantile(anom[np.isin(group, [(g + d) % G for d in range(-(window // 2), (window - 1) // 2 + 1)]), rows[0]:rows[1]]
                       .astype(np.float64), q)
    exactly (order statistics by radix selection on the GPU, numpy's linear interpolation; NaN for an empty pool).  Returns
    float64 (G,)."""
    anom = np.asarray(anom)
    if anom.ndim != 3:
        raise ValueError("anom must be (time, lat, lon)")
    y0, y1 = (int(v) for v in rows)
    _check_percentile_args(q, window)
    if not 0 <= y0 < y1 <= anom.shape[1]:
        raise ValueError("rows {} are not rows of a grid of {}".format((y0, y1), anom.shape[1]))
    ids, G = _native._groups(group, anom.shape[0])
    if ids is None:
        ids, G = np.zeros(anom.shape[0], dtype=np.int32), 1
    if anom.dtype.kind != "f":
        anom = anom.astype(np.float64)
    return _tracker(device).percentile_groups(anom, y0, y1, ids, G, q, window)


def percentile_field_numpy(anom, rows, group, q, window=1, device=None):
    """the per-grid-point twin of percentile_groups_numpy: per group g and grid point of rows[0] <= y < rows[1] the q-quantile over
    every timestep whose group lies in the centred window of `window` groups around g, circular over the groups:
        np.nanquantile(anom[np.isin(group, [(g + d) % G for d in range(-(window // 2), (window - 1) // 2 + 1)]), rows[0]:rows[1]]
                       .astype(np.float64), q, axis=0)
    exactly (ctk_percentile_field_*; NaN for an empty or all-NaN pool).  Returns float64 (G, rows[1] - rows[0], nx)."""
    anom = np.asarray(anom)
    if anom.ndim != 3:
        raise ValueError("anom must be (time, lat, lon)")
    y0, y1 = (int(v) for v in rows)
    _check_percentile_args(q, window)
    if not 0 <= y0 < y1 <= anom.shape[1]:
        raise ValueError("rows {} are not rows of a grid of {}".format((y0, y1), anom.shape[1]))
    ids, G = _native._groups(group, anom.shape[0])
    if ids is None:
        ids, G = np.zeros(anom.shape[0], dtype=np.int32), 1
    if anom.dtype.kind != "f":
        anom = anom.astype(np.float64)
    return _tracker(device).percentile_field(anom, y0, y1, ids, G, q, window)


def std_field_numpy(anom, rows, group, window=1, ddof=0, skipna=True, device=None):
    """the array-level twin of contrack.std_field: per group g (one id in [0, G) per timestep, G = max(group) + 1, any order in time;
    None: one group) and grid point of rows[0] <= y < rows[1] the standard deviation over every timestep whose group lies in the
    centred window of `window` groups around g, circular over the groups, the pool taken in time order:
        np.nanstd(anom[np.isin(group, [(g + d) % G for d in range(-(window // 2), (window - 1) // 2 + 1)]), rows[0]:rows[1]]
                  .astype(np.float64), axis=0, ddof=ddof)                  (skipna False: np.std)
    bit for bit on bands of two or more points (ctk_std_field_*, include/contrack_hip.h: the two-pass float64 loop is the statement;
    NaN where count - ddof <= 0).  Returns float64 (G, rows[1] - rows[0], nx)."""
    anom = np.asarray(anom)
    if anom.ndim != 3:
        raise ValueError("anom must be (time, lat, lon)")
    y0, y1 = (int(v) for v in rows)
    if not 0 <= y0 < y1 <= anom.shape[1]:
        raise ValueError("rows {} are not rows of a grid of {}".format((y0, y1), anom.shape[1]))
    ids, G = _native._groups(group, anom.shape[0])
    if ids is None:
        ids, G = np.zeros(anom.shape[0], dtype=np.int32), 1
    _check_std_args(window, ddof, G, skipna)
    if anom.dtype.kind != "f":
        anom = anom.astype(np.float64)
    return _tracker(device).std_field(anom, y0, y1, ids, G, int(window), int(ddof), bool(skipna))


def _check_std_args(window, ddof, ngroups=None, skipna=True):
    """what the std entries refuse before any device call: a window or ddof that is no whole number in range, more groups than the
    kernel's accumulators hold (ctk_std_plan, csrc/ctk_forms.h -- asked of the library on the host, no GPU)"""
    if int(window) != window or int(window) < 1:
        raise ValueError("window = {} (a whole number of groups, at least 1)".format(window))
    if int(ddof) != ddof or int(ddof) < 0:
        raise ValueError("ddof = {} (a whole number, at least 0)".format(ddof))
    if ngroups is not None:
        plan = _native.debug_std_field_plan(int(ngroups), int(window), bool(skipna))
        if plan["tile"] == 0:
            raise ValueError("{} groups with a window of {}: at most {} groups fit {}".format(
                ngroups, window, plan["max_groups"], "with counts (skipna)" if skipna else "without counts"))


def _check_percentile_args(q, window):
    if not (0.0 <= float(q) <= 1.0):
        raise ValueError("q = {} is not in [0, 1]".format(q))
    if int(window) != window or int(window) < 1:
        raise ValueError("window = {} (a whole number of groups, at least 1)".format(window))


# ------------------------------------------------------------------------------------------------
# the class
# ------------------------------------------------------------------------------------------------

def fragile_rows(rows):
    """indices of the ctk_life_row records whose result sits on a rounding boundary: a centre of mass that is an integer up to
    rounding (contours one pixel wide or high: int() then gives the cell or its neighbour) or an intensity / area at the edge of
    two decimals.  These rows -- a few per cent in practice -- are re-evaluated on the device in the reference's own summation
    orders: after the call by lifecycle_columns(tracker=...), or chunk by chunk as the `pick` of Tracker.lifecycle_stream."""
    if not len(rows):
        return np.empty(0, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        intensity = rows["swv"] / rows["area"]                                                          # :876
        com_y, com_x = rows["swvy"] / rows["swv"], rows["swvx"] / rows["swv"]                           # ndimage.center_of_mass
    area = rows["area"]

    def near_int(v):
        return np.abs(v - np.rint(v)) <= 1e-9 * np.maximum(1.0, np.abs(v))

    def near_half(v, rel):                              # v * 100 close to k + 0.5: round(v, 2) could go either way
        s = np.abs(v) * 100.0
        return np.abs(s - np.floor(s) - 0.5) <= rel * np.maximum(1.0, s)
    # The area is a sum of POSITIVE float64 terms: the device's value (exact integers, rounded once) and numpy's pairwise sum
    # differ by less than 5e-15 of it (depth of the pairwise tree x 2^-53) -- 1e-11 is generous, while 1e-6 would flag every
    # contour beyond 5000 km^2 (a quarter of all rows).  Sums of field values can cancel: their window stays wide.
    with np.errstate(invalid="ignore"):
        fragile = near_int(com_y) | near_int(com_x) | near_half(intensity, 1e-6) | near_half(area, 1e-11) | ~np.isfinite(com_y) | ~np.isfinite(com_x)
    return np.nonzero(fragile)[0]


def lifecycle_columns(rows, lat, lon, dates, tracker=None, exact=None, period=None, indices=False):
    """ctk_life_row records -> the columns of the reference's frame (contrack.py:876-906), rows sorted by (Flag, Date):
    dict of arrays Flag, Date, Longitude, Latitude, Intensity, Size.

    The device sums are float64 but in another order than the reference's (np.sum pairwise, np.bincount sequential).  That shows
    only where a result sits on a rounding boundary (fragile_rows).  With the Tracker that produced `rows` at hand (tracker=) those
    rows are re-evaluated ON THE DEVICE in the reference's own summation orders (ctk_lifecycle_exact); a streamed call has done
    that chunk by chunk and hands over exact=(idx, records), the indices into `rows` and their ctk_life_exact records.
    The Tracker must not have been used for another host-array or streamed call (nor release_io) since it produced `rows`: the
    slabs are gone then and the library's state error is raised -- never the unrefined values.

    period: the slab is a member dimension flattened to steps m * period + t; `dates` are the labels of ONE member's steps, the
    column 'Member' (the position m) is added and the rows are sorted by (Flag, Member, Date).

    indices: three more int64 columns -- Step, the position on the time axis (of the member's own), and Row, Col, the grid indices
    whose coordinates the truncated Latitude and Longitude came from."""
    nx, ny = len(lon), len(lat)
    if (rows["shift"] == -2).any():
        raise ValueError("attempt to get argmax of an empty sequence")                                  # np.argmax(np.diff(.)), :883
    with np.errstate(divide="ignore", invalid="ignore"):
        intensity = rows["swv"] / rows["area"]                                                          # :876
        com_y, com_x = rows["swvy"] / rows["swv"], rows["swvx"] / rows["swv"]                           # ndimage.center_of_mass
    area = rows["area"].copy()
    idx, ex = np.empty(0, dtype=np.int64), None
    if exact is not None:
        idx, ex = np.asarray(exact[0], dtype=np.int64), exact[1]
    elif tracker is not None and len(rows):
        idx = fragile_rows(rows)
        if len(idx):
            ex = tracker.lifecycle_exact(idx)
    if len(idx):
        intensity, com_y, com_x = intensity.copy(), com_y.copy(), com_x.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            area[idx] = ex["area"]
            intensity[idx] = ex["swv"] / ex["area"]
            com_y[idx], com_x[idx] = ex["sy"] / ex["s"], ex["sx"] / ex["s"]
    if not (np.isfinite(com_y).all() and np.isfinite(com_x).all()):
        raise ValueError("cannot convert float NaN to integer")                                         # int(center_of_mass[..]), :886
    iy, ix = np.trunc(com_y).astype(np.int64), np.trunc(com_x).astype(np.int64)
    if ((iy < -ny) | (iy >= ny) | (ix < -nx) | (ix >= nx)).any():
        raise IndexError("centre of mass outside the grid")
    shift = np.where(rows["shift"] > 0, rows["shift"], 0)
    ix = np.where(ix < 0, ix + nx, ix)                                                                  # Python indexing of the rolled axis
    lon_of = np.asarray(lon)[(ix + shift) % nx]                                                         # np.roll(lon, -shift)[ix], :884-887
    lat_of = np.asarray(lat)[iy]
    step = rows["t"] if period is None else rows["t"] % int(period)
    date = np.asarray(dates, dtype=object)[step] if len(rows) else np.empty(0, dtype=object)
    cols = dict(Flag=rows["label"].astype(np.int64), Date=date,
                Longitude=np.trunc(lon_of).astype(np.int64), Latitude=np.trunc(lat_of).astype(np.int64),           # int(), :886-895
                Intensity=np.round(intensity, 2), Size=np.round(area, 2))                               # round(np.float64, 2), :899-900
    if period is not None:
        cols["Member"] = (rows["t"] // int(period)).astype(np.int64)
    if indices:
        cols["Step"] = np.asarray(step, dtype=np.int64)
        cols["Row"] = np.where(iy < 0, iy + ny, iy)                                                     # (Python indexing, as lat[iy])
        cols["Col"] = (ix + shift) % nx
    # the library returns (label, t) order -- (label, member, step of the member) for a flattened member dimension; the reference
    # sorts by the date STRING, which differs when the time axis is not increasing
    if any(a > b for a, b in zip(dates, dates[1:])):
        member = cols["Member"] if period is not None else np.zeros(len(rows), dtype=np.int64)
        order = sorted(range(len(rows)), key=lambda i: (cols["Flag"][i], member[i], cols["Date"][i]))
        cols = {k: v[order] for k, v in cols.items()}
    return cols


def lifecycle_frame(rows, lat, lon, dates, tracker=None, exact=None):
    """the same as a list of (Flag, Date, Longitude, Latitude, Intensity, Size) tuples"""
    c = lifecycle_columns(rows, lat, lon, dates, tracker, exact)
    return [(int(f), d, int(lo), int(la), float(it), float(sz)) for f, d, lo, la, it, sz in
            zip(c["Flag"], c["Date"], c["Longitude"], c["Latitude"], c["Intensity"], c["Size"])]


def _int32_chunk(part):
    """a chunk of integer flags on its way into an int32 buffer: ids beyond int32 are an error, never a wrap-around"""
    part = np.asarray(part)
    if part.dtype.kind not in "iub":
        raise ValueError("flag must be an integer field")
    if part.size and (part.dtype.itemsize > 4 or part.dtype == np.uint32) and \
            (part.max() > np.iinfo(np.int32).max or part.min() < np.iinfo(np.int32).min):              # (nothing to check for int32 and narrower)
        raise ValueError("flag ids beyond int32")
    return part


def lifecycle_numpy(flag, field, wrow, lat, lon, dates, chunk_steps=None, device=None, shape=None, dtype=None, period=None, indices=False):
    """the columns of run_lifecycle's frame (lifecycle_columns) for a (time, lat, lon) integer flag slab and a float field of the
    same shape.  chunk_steps None: both slabs go to the device whole (field None: the anomaly slab resident there, `dtype` its
    type).  Otherwise they pass through chunk-sized device buffers, that many time steps at a time (0: about 256 MB of field):
    arrays (np.memmap included; flags wider than int32 are narrowed chunk by chunk, an id beyond int32 raises ValueError from the
    chunk that holds it) or readers reader(t0, nt, out) with shape=(T, ny, nx) and the field's dtype; the rounding-boundary rows
    are re-evaluated while their chunk is on the device.  period, indices: see lifecycle_columns."""
    trk = _tracker(device)
    if chunk_steps is None:
        flag = _int32_chunk(flag)
        rows = trk.lifecycle(flag, None, wrow, resident_f64=np.dtype(dtype) == np.float64) if field is None else trk.lifecycle(flag, field, wrow)
        return lifecycle_columns(rows, lat, lon, dates, tracker=trk, period=period, indices=indices)
    if callable(flag):
        flag_source = flag
    else:
        if not isinstance(flag, np.memmap):
            flag = np.asarray(flag)
        if flag.dtype.kind not in "iub":
            raise ValueError("flag must be an integer field")
        if shape is None:
            shape = flag.shape
        flag_source = flag
        if flag.dtype != np.int32:
            def flag_source(t0, nt, out, slab=flag):
                out[...] = _int32_chunk(slab[t0:t0 + nt])
    if not callable(field):
        if field.dtype != np.float64:
            field = field.astype(np.float32, copy=False)
        dtype = field.dtype
    rows, idx, ex = trk.lifecycle_stream(flag_source, field, wrow, shape=shape, dtype=dtype, chunk_steps=int(chunk_steps), pick=fragile_rows)
    return lifecycle_columns(rows, lat, lon, dates, exact=(idx, ex), period=period, indices=indices)


INT64_FLAG_FROM = 2 ** 31 - 2       # elements from which scipy.ndimage.label (and the reference's 'flag') switch to int64


def _xr():
    import xarray as xr
    return xr


def _fingerprint(a):
    """cheap identity of a host array (address, shape, dtype and a strided sample of its bytes): is the copy that calc_anom left
    on the GPU still the array the dataset holds?  A new array, another shape or an in-place edit of a sampled element miss.
    Edits the sample cannot see are excluded differently: calc_anom hands the host copy out READ-ONLY (an in-place edit raises
    instead of silently diverging from its twin in HBM; assign a new array to the variable to change it), and an array that has
    been made writeable again never counts as resident."""
    a = np.asarray(a)
    if a.flags.writeable:
        return None
    flat = a.reshape(-1) if a.flags.c_contiguous else None
    sample = b"" if flat is None or flat.size == 0 else np.ascontiguousarray(flat[::max(1, flat.size // 2048)][:2048]).tobytes()
    return (a.__array_interface__["data"][0], a.shape, str(a.dtype), hash(sample))


def _producer_dtype(dtype):
    """the slab type of the entries that produce a field (run_contrack, calc_clim / calc_anom, calc_vertical_mean, calc_reversal):
    float32 stays, everything else becomes float64.  The consumers of a field take it by _native._field_dtype instead."""
    return np.dtype(np.float32) if np.dtype(dtype) == np.float32 else np.dtype(np.float64)


class _Steps(object):
    """a labelled variable as the (steps, lat, lon) series the library takes: `step_dims`, in the order given, count the steps --
    (time,), (member, time): flat step m * T + t, or every non-spatial dim --, `level` names a level dim kept in front of
    (lat, lon).  The variable's own dim order is free; slab() is the whole series on the host, reader() reads it slice by slice,
    restore() brings a (steps, ...) result back into labelled dims."""

    def __init__(self, da, step_dims, lat, lon, level=None):
        self.da, self.dims, self.step_dims = da, tuple(da.dims), tuple(step_dims)
        self.tail = ((level,) if level is not None else ()) + (lat, lon)
        self.step_shape = tuple(da.shape[self.dims.index(d)] for d in self.step_dims)
        self.steps = int(np.prod(self.step_shape)) if self.step_dims else 1
        self.shape = (self.steps, da.shape[self.dims.index(lat)], da.shape[self.dims.index(lon)])

    def slab(self, only=None):
        """the host array (steps, [nlev,] ny, nx): a transpose and a reshape of the variable's data -- a view of it where its dims
        are already in that order.  only=o: the series of outer step index o alone (a view: member o of (member, time))."""
        arr = np.asarray(self.da.data).transpose([self.dims.index(d) for d in self.step_dims + self.tail])
        if only is not None:
            return arr[np.unravel_index(only, self.step_shape[:-1])]
        return arr.reshape((self.steps,) + arr.shape[len(self.step_dims):])

    def reader(self, integer=False, only=None, level_runs=None):
        """reader(t0, nt, out) of the flat steps [t0, t0 + nt): one isel(outer step dims = index, innermost step dim = slice) per run
        of the innermost step dim the window touches -- a chunk that spans two members in two pieces --, so the flattened slab is
        never built on the host.  out is (nt, ny, nx); with level_runs, (first level, count) pairs, (nt, nsel, ny, nx) filled by
        one isel per run of levels.  integer: a flag variable, every piece checked on its way in (_int32_chunk).  only=o: as in
        slab.  A single step dim without `isel` is read with np.take."""
        da, outer, inner, n_in = self.da, self.step_dims[:-1], self.step_dims[-1], self.step_shape[-1]
        left = tuple(d for d in self.dims if d not in outer)                      # what isel(outer step dims = index) leaves
        sort = [left.index(d) for d in (inner,) + self.tail]
        narrow = _int32_chunk if integer else (lambda a: a)

        def piece(sel):
            if outer or hasattr(da, "isel"):
                return narrow(np.asarray(da.isel(**sel).data)).transpose(sort)
            t = sel[inner]
            return narrow(np.asarray(da.data).take(range(t.start, t.stop), axis=self.dims.index(inner))).transpose(sort)

        def reader(t0, nt, out):
            done = 0
            while done < nt:
                o, t = divmod(t0 + done, n_in)
                n = min(nt - done, n_in - t)
                sel = dict(zip(outer, (int(v) for v in np.unravel_index(o if only is None else only, self.step_shape[:-1]))))
                sel[inner] = slice(t, t + n)
                if level_runs is None:
                    out[done:done + n] = piece(sel)
                else:
                    k = 0
                    for l0, ln in level_runs:
                        sel[self.tail[0]] = slice(l0, l0 + ln)
                        out[done:done + n, k:k + ln] = piece(sel)
                        k += ln
                done += n
        return reader

    def restore(self, arr, out_dims):
        """a (steps, ...) result whose other axes are the last of ([level,] lat, lon) -> the labelled dim order `out_dims`: the steps
        reshaped to the step dims, then a transpose (a view of a contiguous `arr`)"""
        have = self.step_dims + self.tail[len(self.tail) - (arr.ndim - 1):]
        return arr.reshape(self.step_shape + arr.shape[1:]).transpose([have.index(d) for d in out_dims])


class contrack(object):
    """contrack class -- interface of steidani/ConTrack (contrack/contrack.py:49), HIP-accelerated run_contrack."""

    num_of_contrack = 0

    def __init__(self, filename="", ds=None, **kwargs):
        """contrack(filename) reads a netCDF file, contrack(ds=dataset) wraps a dataset, contrack() is empty
        (contrack.py:58-88)."""
        if not filename:
            self.ds = None if ds is None else ds
            return
        try:
            self.ds = None
            self.read(filename, **kwargs)
        except (OSError, IOError, RuntimeError):
            try:
                self.read(filename, **kwargs)
            except Exception:
                raise IOError("Unkown fileformat. Known formats are netcdf.")
        contrack.num_of_contrack += 1

    def __repr__(self):
        try:
            return "\
            Xarray dataset with {} time steps. \n\
            Available fields: {}".format(self.ntime, ", ".join(self.variables))
        except AttributeError:
            return "\
            Empty contrack container.\n\
            Hint: use read() to load data."

    def __str__(self):
        return 'Class {}: \n{}'.format(self.__class__.__name__, self.ds)

    def __len__(self):
        return len(self.ds)

    def __getattr__(self, attr):
        if attr in self.__dict__:
            return getattr(self, attr)
        if attr == "ds":
            raise AttributeError(attr)
        return getattr(self.ds, attr)

    def __getitem__(self, key):
        return self.ds[key]

    # ---- properties (contrack.py:119-161) ------------------------------------------------------
    def _dim_size(self, name):
        dims = self.ds.dims
        try:
            return dims[name]
        except (TypeError, KeyError, IndexError):          # newer xarray: dims of a Dataset may be a plain view
            return self.ds.sizes[name]

    @property
    def ntime(self):
        if len(self.ds.dims) != 3:
            logger.warning("\nBe careful with the dimensions, you want dims = 3 and shape:\n(latitude, longitude, time)")
        return self._dim_size(self._get_name_time())

    @property
    def variables(self):
        return list(self.ds.data_vars)

    @property
    def dimensions(self):
        return list(self.ds.dims)

    @property
    def grid(self):
        if len(self.ds.dims) != 3:
            logger.warning("\nBe careful with the dimensions, you want dims = 3 and shape:\n(latitude, longitude, time)")
            return None
        print("\
        latitude: {} \n\
        longitude: {}".format(self._dim_size(self._get_name_latitude()), self._dim_size(self._get_name_longitude())))

    @property
    def dataset(self):
        return self.ds

    # ---- read (contrack.py:166-199) ---------------------------------------------------------------
    def read(self, filename, **kwargs):
        if self.ds is None:
            self.ds = _xr().open_dataset(filename, **kwargs)
            logger.debug('read: {}'.format(self.__str__))
        else:
            raise ValueError('contrack() is already set!')

    def read_xarray(self, ds):
        if self.ds is None:
            try:
                xr = _xr()
                ok = isinstance(ds, xr.core.dataset.Dataset)
            except ImportError:                              # no xarray installed: accept a duck-typed dataset
                ok = hasattr(ds, "dims") and hasattr(ds, "data_vars")
            if not ok:
                raise ValueError('ds has to be a xarray data set!')
            self.ds = ds
            logger.debug('read_xarray: {}'.format(self.__str__))
        else:
            raise ValueError('contrack() is already set!')

    # ---- set up (contrack.py:204-380) ----------------------------------------------------------------
    def set_up(self, time_name=None, longitude_name=None, latitude_name=None, force=False, write=True):
        self._time_name = self._get_name_time() if time_name is None else time_name
        self._longitude_name = self._get_name_longitude() if longitude_name is None else longitude_name
        self._latitude_name = self._get_name_latitude() if latitude_name is None else latitude_name
        if (self._longitude_name and self._latitude_name) is not None:
            self._dlon = self._get_resolution(self._longitude_name, force=force)
            self._dlat = self._get_resolution(self._latitude_name, force=force)
        if self._time_name is not None:
            self._dtime = self._get_resolution(self._time_name, force=force)
        if write:
            self._log_dim_names()

    def _log_dim_names(self):
        logger.info("\n time: '{}'\n longitude: '{}'\n latitude: '{}'\n".format(
            self._time_name, self._longitude_name, self._latitude_name))

    def _units_of(self, dim):
        out = []
        da = self.ds[dim]
        for holder in (getattr(da, "attrs", None), getattr(da, "encoding", None)):
            if holder and 'units' in holder:
                out.append(holder['units'])
        return out

    def _get_name_time(self):
        for dim in self.ds.dims:
            if any('since' in u for u in self._units_of(dim)) or dim in ['time']:
                return dim
        for name in self.ds.variables:
            data = self.ds[name].data
            try:
                first = data[0]
            except IndexError:
                first = data
            if isinstance(first, np.datetime64):
                return name
        logger.warning("\n 'time' dimension (dtype='datetime64[ns]') not found.")
        return None

    def _get_name_longitude(self):
        for dim in self.ds.dims:
            attrs = getattr(self.ds[dim], "attrs", {})
            if attrs.get('units') in ['degree_east', 'degrees_east'] or dim in ['lon', 'longitude', 'x']:
                return dim
        logger.warning("\n 'longitude' dimension (unit='degrees_east') not found.")
        return None

    def _get_name_latitude(self):
        for dim in self.ds.dims:
            attrs = getattr(self.ds[dim], "attrs", {})
            if attrs.get('units') in ['degree_north', 'degrees_north'] or dim in ['lat', 'latitude', 'y']:
                return dim
        logger.warning("\n 'latitude' dimension (unit='degrees_north') not found.")
        return None

    def _get_resolution(self, dim, force=False):
        """grid spacing in degrees / time step in hours (contrack.py:327-380)"""
        if dim == self._time_name:
            try:
                stamps = np.asarray(self.ds[dim].to_index().values)
                # (numpy arithmetic: pandas >= 2 refuses TimedeltaIndex.astype('timedelta64[h]'))
                delta = np.unique((stamps[1:] - stamps[:-1]).astype('timedelta64[h]'))
            except AttributeError:
                attrs = getattr(self.ds[dim], "attrs", {})
                if 'units' in attrs and 'days' in attrs['units']:
                    var = self.ds[dim].data
                    delta = np.unique(var[1:] - var[:-1])
                else:
                    raise ValueError('Can not decode time with unit {}'.format(attrs['units']))
        else:
            data = self.ds[dim].data
            delta = abs(np.unique(data[1:] - data[:-1]))
        if len(delta) > 1:
            errmsg = 'No regular grid found for dimension {}.\n\
            Hint: use set_up(force=True).'.format(dim)
            if force and dim != self._time_name:
                logging.warning(errmsg)
                logging.warning(' '.join(['force=True: using mean of non-equidistant', 'grid {}'.format(delta)]))
                delta = round(delta.mean(), 2)
            elif dim == self._time_name:
                logging.warning(errmsg)
            else:
                raise ValueError(errmsg)
        elif delta[0] == 0:
            raise ValueError('Two equivalent values found for dimension {}.'.format(dim))
        elif delta[0] < 0:
            raise ValueError(' '.join(['{} not increasing. This should', 'not happen?!']).format(dim))
        return delta

    def _time_steps(self):
        """the steps between consecutive timestamps, decoded as _get_resolution decodes the time axis (hours; the numbers
        themselves for a numeric 'days since' axis)"""
        dim = self._time_name
        try:
            stamps = np.asarray(self.ds[dim].to_index().values)
            return (stamps[1:] - stamps[:-1]).astype('timedelta64[h]')
        except AttributeError:
            attrs = getattr(self.ds[dim], "attrs", {})
            if 'units' in attrs and 'days' in attrs['units']:
                var = np.asarray(self.ds[dim].data)
                return var[1:] - var[:-1]
            raise ValueError('Can not decode time with unit {}'.format(attrs.get('units')))

    def _ensure_set_up(self):
        logger.info("Set up dimensions...")
        if hasattr(self, '_time_name'):
            self._log_dim_names()
        else:
            self.set_up()

    # ---- pre-processing glue (contrack.py:386-581); plain xarray, not accelerated ------------------------
    def calculate_gph_from_gp(self, gp_name='z', gp_unit='m**2 s**-2', gph_name='z_height'):
        g = 9.80665
        if self.ds[gp_name].attrs['units'] != gp_unit:
            raise ValueError('Geopotential unit should be {} not {}'.format(gp_unit, self.ds[gp_name].attrs['units']))
        self.ds[gph_name] = (self.ds.variables[gp_name].dims, self.ds.variables[gp_name].data / g,
                             {'units': 'm', 'long_name': 'Geopotential Height', 'standard_name': 'geopotential height',
                              'history': 'Calculated from {} with g={}'.format(gp_name, g)})
        logger.info('Calculating GPH from GP... DONE')

    def calc_mean(self, variable):
        if not variable:
            return self['z'].mean(dim="time")
        if variable not in self.variables:
            logger.warning("\n Variable '{}' not found. Select from {}.".format(variable, self.variables))
            return None
        return self[variable].mean(dim="time")

    # ---- vertical mean over a pressure band (README.rst:235-240, first step of the third recipe) ----------------------------
    _LEVEL_NAMES = ('level', 'lev', 'plev', 'pressure_level', 'isobaricInhPa')
    _PRESSURE_UNITS = ('hPa', 'Pa', 'mbar', 'millibars')

    def _get_name_level(self, dims, level_name=None):
        """the level dimension of a variable with dims `dims`: level_name, the one dimension with a usual name, or the one dimension
        besides time, latitude and longitude whose coordinate has pressure units"""
        if level_name is not None:
            if level_name not in dims:
                raise ValueError("level_name={!r} is not a dimension of the variable (dims {})".format(level_name, dims))
            return level_name
        named = [d for d in dims if d in self._LEVEL_NAMES]
        if len(named) == 1:
            return named[0]

        def pressure(d):
            try:
                return any(u in self._PRESSURE_UNITS for u in self._units_of(d))
            except (KeyError, AttributeError):
                return False
        rest = [d for d in dims if d not in (self._time_name, self._latitude_name, self._longitude_name) and pressure(d)]
        if len(rest) == 1:
            return rest[0]
        raise ValueError("no level dimension found among the dims {} (one of {} or a coordinate in {}); name it with level_name="
                         .format(dims, self._LEVEL_NAMES, self._PRESSURE_UNITS))

    def _steps(self, da, step_dims, level=None):
        """the flat-step view (_Steps) of a variable of this dataset; a None among step_dims (no member dimension) is left out"""
        return _Steps(da, tuple(d for d in step_dims if d is not None), self._latitude_name, self._longitude_name, level)

    def _every_step(self, variable, chunk_steps, level=None):
        """what calc_vertical_mean and calc_reversal share: (da, view, resident, streamed).  view: every dim of the variable besides
        `level`, latitude and longitude counts steps; resident: the result also stays in HBM (a host call over time alone);
        streamed: the variable is read slice by slice (view.reader), else as view.slab()"""
        da = self.ds[variable]
        dims = tuple(da.dims)
        for d in (self._latitude_name, self._longitude_name):
            if d not in dims:
                raise ValueError("the variable {!r} has no dimension {!r} (dims {})".format(variable, d, dims))
        view = self._steps(da, tuple(d for d in dims if d not in (level, self._latitude_name, self._longitude_name)), level)
        resident = chunk_steps is None and view.step_dims == (self._time_name,)
        return da, view, resident, chunk_steps is not None and bool(view.step_dims)

    def calc_vertical_mean(self, variable, bounds=None, level_name=None, weights='pressure', skipna=False, name=None, chunk_steps=None):
        """adds the variable `name` (default variable + '_vmean'): the mean of `variable` over its level dimension between `bounds`
        (two coordinate values in either order, inclusive; None: every level) -- "The PV fields are vertically averaged between
        500-150 hPa" (README.rst:235-240), bounds=(150, 500) -- computed on the GPU (level_mean_numpy).
        weights: 'pressure' (trapezoid rule over the selected levels of the coordinate, level_weights: the integral over pressure /
        the depth of the band), 'equal', or one value >= 0 per level (0: not selected; bounds must be None).  skipna: NaN levels of a
        pixel are left out of its mean.  The level dimension is level_name, the one dimension called level / lev / plev /
        pressure_level / isobaricInhPa, or the one other dimension whose coordinate has units hPa / Pa / mbar / millibars.  Every
        other dimension besides latitude and longitude (time, a member dimension ...) counts steps, each reduced on its own; any
        dim order is accepted, (..., level, lat, lon) avoids a host copy.  The new variable has the variable's dims without the
        level dimension.
        chunk_steps: the variable is read slice by slice (`isel` on the step dims and on the selected levels only) and passes
        through chunk-sized device buffers; the 4-D array is never built on the host.  Without it, for a (time, level, lat, lon)
        variable in any order, the mean also stays in HBM and a following calc_anom(variable=name) starts from there."""
        self._ensure_set_up()
        dims = tuple(self.ds[variable].dims)
        lev = self._get_name_level(dims, level_name)
        da, view, resident, streamed = self._every_step(variable, chunk_steps, lev)
        nlev = da.shape[dims.index(lev)]
        if isinstance(weights, str):
            try:
                levels = np.asarray(self.ds[lev].data)
            except (KeyError, AttributeError):
                levels = None
            w = _vertical_weights(weights, levels, bounds, nlev)
        else:
            if bounds is not None:
                raise ValueError("explicit weights select the levels themselves: bounds must be None")
            w = _vertical_weights(weights, None, None, nlev)
            levels = None
        sel = np.flatnonzero(w > 0)
        out_dims = tuple(d for d in dims if d != lev)
        trk = _tracker()
        logger.info('Calculating vertical mean of {} over {} of {} levels...'.format(variable, len(sel), nlev))
        if streamed:
            runs = [(int(r[0]), len(r)) for r in np.split(sel, np.flatnonzero(np.diff(sel) != 1) + 1)]
            mean = trk.level_mean_cb(view.reader(level_runs=runs), (view.steps, len(sel)) + view.shape[1:], _producer_dtype(da.dtype), w[sel],
                                     skipna=skipna, chunk_steps=int(chunk_steps))
        else:
            arr = view.slab()
            if arr.dtype.kind != "f":
                arr = arr.astype(np.float64)
            mean = trk.level_mean(arr, w, skipna=skipna, keep_resident=resident)
        if resident:
            mean.flags.writeable = False                     # (its twin stays in HBM for calc_anom: see _fingerprint)
        out = view.restore(mean, out_dims)
        name = variable + '_vmean' if name is None else name
        attrs = {}
        if 'units' in da.attrs:
            attrs['units'] = da.attrs['units']
        attrs['long_name'] = da.attrs.get('long_name', variable) + ' vertical mean'
        rule = weights if isinstance(weights, str) else 'given'
        attrs['history'] = 'Calculated from {} with input attributes: bounds = {}, levels = {}, weights = {}{}.'.format(
            variable, None if bounds is None else tuple(np.asarray(bounds).tolist()),
            (np.asarray(levels)[sel].tolist() if levels is not None else sel.tolist()), rule, ', NaN levels skipped' if skipna else '')
        self.ds[name] = (out_dims, out, attrs)
        self._vmean_resident = (name, _fingerprint(np.asarray(self.ds[name].data)), trk.resident_level_mean_generation()) if resident else None
        logger.info('Calculating vertical mean... DONE')

    def _vmean_resident_for(self, variable, slab):
        """True if `variable` is this instance's vertical mean and its twin is still the mean resident in HBM (slab: its
        (time, lat, lon) view on the host)"""
        res = getattr(self, "_vmean_resident", None)
        if res is None or res[0] != variable or res[1] is None:
            return False
        trk = _tracker()
        return res[1] == _fingerprint(np.asarray(self.ds[variable].data)) and res[2] == trk.resident_level_mean_generation() and \
            trk.resident_level_mean() == (slab.shape[0], slab.shape[1], slab.shape[2], slab.dtype == np.float64)

    # ---- a weighted filter or block means along time -------------------------------------------------------------------------
    def calc_filter(self, variable, weights, stride=1, offset=None, edges='nan', skipna=False, segments=None, chunk_steps=None, name=None):
        """a weighted filter or a block mean of `variable` along time on the GPU (time_filter_numpy states layout and arithmetic).
        weights: the taps -- lanczos_weights(ntaps, cutoff ...) for a low-, high- or band-pass, any float64 array -- or an int K:
        the plain mean of K steps.  edges: 'nan' (an output whose window leaves its segment is NaN) or 'renorm' (the taps inside,
        divided by the sum of their weights); skipna: NaN taps are left out the same way.
        segments: the meaning it has in calc_anom -- None, 'gaps', an int array of start indices, or the name of a member dimension
        of a 4-D variable (any dim order); no window crosses a break.
        stride == 1 (and the default offset): one output per step; adds the variable `name` (default variable + '_filt') with the
        variable's dims and units.  Over time alone and without chunk_steps the result also stays in HBM and a following
        calc_anom(variable=name) starts from there; if `variable` is itself the vertical mean calc_vertical_mean left there, it is
        not uploaded either.
        stride > 1 (6-hourly to daily means: weights=4, stride=4): the time axis changes, so the result is RETURNED as a labelled
        array whose time coordinate is the time of each output's label step (tap K // 2) and nothing is added to the dataset.  A
        member dimension stays in place; every member has the same number of outputs.
        chunk_steps: the variable is read slice by slice (`isel`) and passes through chunk-sized device buffers."""
        self._ensure_set_up()
        da = self.ds[variable]
        dims = tuple(da.dims)
        member, starts, T = self._segment_args(variable, da, dims, segments)
        if member is None and len(dims) != 3:
            raise ValueError("the variable {!r} must be 3-D (time, lat, lon in any order), it has dims {}".format(variable, dims))
        view = self._steps(da, (member, self._time_name))
        _, K = _native._filter_weights(weights)
        label, out_starts, _ = filter_layout(view.steps, weights, stride, offset, starts)
        M = 1 if member is None else da.shape[dims.index(member)]
        in_place = int(stride) == 1 and len(label) == view.steps          # one output per step: the variable's own time axis
        resident = in_place and chunk_steps is None and member is None
        kw = dict(stride=stride, offset=offset, edges=edges, skipna=skipna, segments=starts)
        trk = _tracker()
        logger.info('Filtering {} along {} ({} taps, stride {})...'.format(variable, self._time_name, K, stride))
        if chunk_steps is not None:
            out = trk.time_filter_cb(view.reader(), view.shape, _producer_dtype(da.dtype), weights, chunk_steps=int(chunk_steps), **kw)
        else:
            slab = view.slab()
            slab = np.ascontiguousarray(slab, dtype=_producer_dtype(slab.dtype))
            if resident and self._vmean_resident_for(variable, slab):       # (the mean left in HBM: nothing to upload, same bits)
                out = trk.time_filter_resident(weights, keep_resident=True, **kw)
            else:
                out = trk.time_filter(slab, weights, keep_resident=resident, **kw)
        if resident:
            out.flags.writeable = False                      # (its twin stays in HBM for calc_anom: see _fingerprint)
        n_out = len(label) // M                              # (segments of one length: every member has the same outputs)
        have = view.step_dims + (self._latitude_name, self._longitude_name)
        arr = out.reshape(((M,) if member is not None else ()) + (n_out,) + out.shape[1:]).transpose([have.index(d) for d in dims])
        name = variable + '_filt' if name is None else name
        attrs = {}
        if 'units' in da.attrs:
            attrs['units'] = da.attrs['units']
        attrs['long_name'] = da.attrs.get('long_name', variable) + ' filtered in time'
        attrs['history'] = 'Calculated from {} with input attributes: taps = {}{}, stride = {}, offset = {}, edges = {}{}, segments = {} ({}).'.format(
            variable, K, ' (box)' if np.ndim(weights) == 0 else '', int(stride), _native.filter_offset(K, int(stride), offset), edges,
            ', NaN taps skipped' if skipna else '', None if segments is None else (segments if isinstance(segments, str) else 'starts'),
            1 if starts is None else len(starts))
        if in_place:
            self.ds[name] = (dims, arr, attrs)
            self._vmean_resident = (name, _fingerprint(np.asarray(self.ds[name].data)), trk.resident_level_mean_generation()) if resident else None
            logger.info('Filtering... DONE')
            return None
        if getattr(self, "_vmean_resident", None) is not None and chunk_steps is None and self._vmean_resident[0] == name:
            self._vmean_resident = None
        coords = {}
        for d in dims:
            try:
                vals = np.asarray(self.ds[d].data)
            except (KeyError, AttributeError):
                continue
            coords[d] = vals[label[:n_out]] if d == self._time_name else vals
        logger.info('Filtering... DONE')
        return self._wrap(da, arr, dims, coords, attrs, name)

    # ---- reversal of the meridional height gradient: the second family of blocking indices --------------------------------
    def calc_reversal(self, variable, delta=15., ghgs=0., ghgn=-10., ghgs2=None, lat_bounds=(30, 75), hemisphere='both', stat='gradient', name='reversal',
                      chunk_steps=None):
        """adds the variable `name`: the two-dimensional blocking index of the reversal of the meridional gradient of `variable`
        (geopotential height; Tibaldi & Molteni 1990, Scherrer et al. 2006, Davini et al. 2012), computed on the GPU
        (reversal_numpy).  A grid point at latitude phi (lat_bounds[0] <= |phi| <= lat_bounds[1], in the selected hemisphere:
        'both', 'north', 'south') is blocked where the gradient towards the equator over `delta` degrees exceeds ghgs and the
        gradient towards the pole stays below ghgn (units per degree; the defaults 0 and -10 m / degree are Tibaldi & Molteni's);
        ghgs2 (Davini's third criterion: -5) also asks the gradient between phi - delta and phi - 2 delta to stay below ghgs2.  The
        rows nearest to phi -+ delta are taken and the gradients use their actual distance (reversal_rows).
        stat='gradient': the equatorward gradient where blocked, 0 elsewhere (units `<units> / degree`); stat='mask': 1 / 0 (units 1).
        run_contrack(variable=name, threshold=0, gorl='>', ...) then tracks the blocked regions: spatial coherence, overlap and
        persistence are the tracker's.  Every dimension besides latitude and longitude (time, a member dimension ...) counts steps,
        each on its own; any dim order is accepted and kept.
        chunk_steps: the variable is read slice by slice (`isel` on the step dims) and passes through chunk-sized device buffers;
        the host slab is never built.  Without it, for a (time, lat, lon) variable in any order, the result also stays in HBM and
        a following run_contrack(variable=name) starts from there (its host twin is read-only, as calc_anom's).
        Not here: the longitudinal-extent criterion; the one-dimensional diagram of Tibaldi & Molteni is
        calc_hovmoller(flag, lat_bounds=<a narrow band>) of the tracked mask."""
        self._ensure_set_up()
        if stat not in _REVERSAL_STATS:
            raise ValueError("stat={!r}: one of {}".format(stat, _REVERSAL_STATS))
        if chunk_steps is not None and int(chunk_steps) < 0:
            raise ValueError("chunk_steps must be >= 0")
        da, view, resident, streamed = self._every_step(variable, chunk_steps)
        dims = view.dims
        lat = np.asarray(self.ds[self._latitude_name].data)
        rows = reversal_limits(reversal_rows(lat, delta, lat_bounds, hemisphere, ghgs2 is not None), ghgs, ghgn, ghgs2)
        trk = _tracker()
        logger.info('Calculating gradient reversal of {} on {} of {} rows...'.format(variable, int(np.count_nonzero(rows["eq"] >= 0)), view.shape[1]))
        if streamed:
            res = trk.reversal_cb(view.reader(), view.shape, _producer_dtype(da.dtype), rows, mask=stat == 'mask', chunk_steps=int(chunk_steps))
        else:
            arr = view.slab()
            if arr.dtype.kind != "f":
                arr = arr.astype(np.float64)
            res = trk.reversal(arr, rows, mask=stat == 'mask', keep_resident=resident)
        if resident:
            res.flags.writeable = False                      # (its twin stays in HBM for run_contrack: see _fingerprint)
        out = view.restore(res, dims)
        units = da.attrs.get('units')
        attrs = {'units': '1' if stat == 'mask' else '{} / degree'.format(units) if units else 'degree-1',
                 'long_name': da.attrs.get('long_name', variable) + (' gradient reversal mask' if stat == 'mask' else ' reversed equatorward gradient'),
                 'history': 'Calculated from {} with input attributes: delta = {}, ghgs = {}, ghgn = {}, ghgs2 = {}, lat_bounds = {}, hemisphere = {}, '
                            'stat = {}.'.format(variable, delta, ghgs, ghgn, ghgs2, tuple(np.asarray(lat_bounds).tolist()), hemisphere, stat)}
        self.ds[name] = (dims, out, attrs)
        if resident:
            # (the resident slot now holds this field: the record of calc_anom's slab, if any, is replaced with it)
            self._anom_resident = (_fingerprint(np.asarray(self.ds[name].data)), trk.resident_generation())
            self._anom_resident_name = name
        logger.info('Calculating gradient reversal... DONE')

    # ---- finite-amplitude local wave activity: the third family of blocking indices ------------------------------------------
    def calc_lwa(self, variable, lat_bounds=(30, 75), hemisphere='both', part='total', name='lwa', radius=6.371e6, chunk_steps=None, reference=None):
        """adds the variable `name`: the finite-amplitude local wave activity of `variable` (Huang & Nakamura 2016; Chen, Lu,
        Burrows & Leung 2015 for 500 hPa height, with the anticyclonic / cyclonic split; Martineau et al. 2017; Nakamura & Huang
        2018), computed on the GPU (lwa_numpy).  `variable` is a height field that falls towards the pole; for a field that rises
        towards the pole, such as PV, pass its negative.  At latitude phi (lat_bounds[0] <= |phi| <= lat_bounds[1], 0 <
        lat_bounds[0], in the selected hemisphere: 'both', 'north', 'south') the contour Z whose poleward area equals that of the
        cap poleward of phi is found per time step and hemisphere; the activity of a grid point is radius / cos(phi) times the
        meridional integral of the displaced field: z - Z poleward of phi where z > Z ('anticyclonic': ridges, the part blocks
        are made of) plus Z - z equatorward of phi where z < Z ('cyclonic': troughs); part='total' is their sum.  Units
        `<units> m` (radius in m).  percentile_threshold(variable=name, ...) / percentile_field give the threshold, and
        run_contrack(variable=name, threshold=..., gorl='>') tracks the blocked regions.  Every dimension besides latitude and
        longitude (time, a member dimension ...) counts steps, each on its own; any dim order is accepted and kept.
        chunk_steps: the variable is read slice by slice (`isel` on the step dims) and passes through chunk-sized device buffers;
        the host slab is never built.  Without it, for a (time, lat, lon) variable in any order, the result also stays in HBM and
        a following run_contrack(variable=name) starts from there (its host twin is read-only, as calc_anom's).
        reference='<name>': also adds the contours Z as a (steps..., lat) variable (0 outside lat_bounds)."""
        self._ensure_set_up()
        if part not in _LWA_PARTS:
            raise ValueError("part={!r}: one of {}".format(part, _LWA_PARTS))
        if chunk_steps is not None and int(chunk_steps) < 0:
            raise ValueError("chunk_steps must be >= 0")
        da, view, resident, streamed = self._every_step(variable, chunk_steps)
        dims = view.dims
        lat = np.asarray(self.ds[self._latitude_name].data)
        rows = lwa_rows(lat, lat_bounds, hemisphere, radius)
        want_ref = reference is not None
        trk = _tracker()
        logger.info('Calculating local wave activity of {} on {} of {} rows...'.format(variable, int(np.count_nonzero(rows["active"])), view.shape[1]))
        if streamed:
            res = trk.lwa_cb(view.reader(), view.shape, _producer_dtype(da.dtype), rows, part=part, chunk_steps=int(chunk_steps), want_ref=want_ref)
        else:
            arr = view.slab()
            if arr.dtype.kind != "f":
                arr = arr.astype(np.float64)
            res = trk.lwa(arr, rows, part=part, keep_resident=resident, want_ref=want_ref)
        res, ref = res if want_ref else (res, None)
        if resident:
            res.flags.writeable = False                      # (its twin stays in HBM for run_contrack: see _fingerprint)
        out = view.restore(res, dims)
        units = da.attrs.get('units')
        history = 'Calculated from {} with input attributes: lat_bounds = {}, hemisphere = {}, part = {}, radius = {}.'.format(
            variable, tuple(np.asarray(lat_bounds).tolist()), hemisphere, part, radius)
        attrs = {'units': '{} m'.format(units) if units else 'm',
                 'long_name': da.attrs.get('long_name', variable) + (' local wave activity' if part == 'total' else ' {} local wave activity'.format(part)),
                 'history': history}
        self.ds[name] = (dims, out, attrs)
        if want_ref:
            ref_dims = tuple(d for d in dims if d != self._longitude_name)
            rattrs = {'long_name': da.attrs.get('long_name', variable) + ' equivalent-latitude contour', 'history': history}
            if units:
                rattrs['units'] = units
            have = view.step_dims + (self._latitude_name,)
            self.ds[reference] = (ref_dims, ref.reshape(view.step_shape + ref.shape[1:]).transpose([have.index(d) for d in ref_dims]), rattrs)
        if resident:
            # (the resident slot now holds this field: the record of calc_anom's slab, if any, is replaced with it)
            self._anom_resident = (_fingerprint(np.asarray(self.ds[name].data)), trk.resident_generation())
            self._anom_resident_name = name
        logger.info('Calculating local wave activity... DONE')

    # ---- climatology / anomaly (contrack.py:458-581) on the device: SURVEY.md section 8(f) row N2 ------------------------
    def _group_ids(self, groupby):
        """(ids per timestep in 0..G-1, the G group values in ascending order) for time.<groupby> (dayofyear, month, ...)"""
        t = self.ds[self._time_name]
        try:
            vals = np.asarray(getattr(t.dt, groupby))
        except (AttributeError, TypeError):
            import pandas as pd
            idx = pd.DatetimeIndex(np.asarray(t.data))
            # (pandas has no season: the months mapped as xarray's time.season does)
            vals = season_of_month(idx.month) if groupby == 'season' else np.asarray(getattr(idx, groupby))
        uniq, ids = np.unique(vals, return_inverse=True)
        return ids.astype(np.int32), uniq

    def _wrap(self, like, data, dims, coords=None, attrs=None, name=None):
        """a labelled array of the same class as `like` (xarray.DataArray, or whatever duck-typed dataset is wrapped)"""
        try:                                         # (the climatology keeps the variable's name, as xarray's groupby().mean() does)
            return type(like)(data, dims=dims, coords=coords, attrs=attrs or {}, name=name or getattr(like, "name", None))
        except TypeError:
            return type(like)(data, dims=dims, coords=coords, attrs=attrs or {})

    def calc_clim(self, variable, window=1, groupby='dayofyear', segments=None, chunk_steps=None):
        """climatological mean per `groupby` value, smoothed with a centred running mean over `window` groups; NaNs of the
        running mean (both ends of the axis) are replaced by the mean of the last `window` groups, as the reference does.
        segments (extension): as in run_contrack; with the name of a member dimension the variable is 4-D (any dim order) and the
        climatology is pooled over all members (the ensemble climatology), over (groupby, lat, lon); breaks along time ('gaps',
        start indices) do not change a climatology.  chunk_steps (extension): the variable is read slice by slice (`isel`) and
        passes through chunk-sized device buffers, once; the slab is never built on the host."""
        if segments is None and chunk_steps is None:
            slab = self._steps(self.ds[variable], (self._time_name,)).slab()
            ids, uniq = self._group_ids(groupby)
            if slab.dtype.kind != "f":
                slab = slab.astype(np.float64)
            _, clim = _tracker().anomalies(slab, ids, len(uniq), window=window, smooth=1, want_anom=False, want_clim=True)
        else:
            self._ensure_set_up()
            ids, uniq = self._group_ids(groupby)
            source, shape, dtype, ids, _, _ = self._anom_source(variable, segments, chunk_steps, ids)
            if chunk_steps is None:
                _, clim = _tracker().anomalies(source, ids, len(uniq), window=window, smooth=1, want_anom=False, want_clim=True)
            else:
                _, clim = _tracker().anomalies_stream(source, ids, len(uniq), window=window, smooth=1, sink=False, shape=shape, dtype=dtype,
                                                      chunk_steps=int(chunk_steps), want_clim=True)
        da = self.ds[variable]
        coords = {groupby: uniq}
        for name in (self._latitude_name, self._longitude_name):
            coords[name] = np.asarray(self.ds[name].data)
        return self._wrap(da, clim, (groupby, self._latitude_name, self._longitude_name), coords)

    def _anom_source(self, variable, segments, chunk_steps, ids, only=None):
        """what calc_clim / calc_anom hand to the tracker for `segments` / `chunk_steps`: (source, (steps, ny, nx), dtype, group ids
        per flat step, segment starts or None, member dimension or None).  source is the (steps, ny, nx) float slab, or with
        chunk_steps a reader of slices of the variable; a member dimension is flattened to steps m * T + t, the group of which is
        the group of t.  only=m: member m alone (its T steps)."""
        da = self.ds[variable]
        dims = tuple(da.dims)
        member, starts, T = self._segment_args(variable, da, dims, segments)
        if member is not None and only is None:
            ids = np.tile(ids, da.shape[dims.index(member)])
        if member is None and chunk_steps is not None and len(dims) != 3:
            raise ValueError("the variable {!r} must be 3-D (time, lat, lon in any order), it has dims {}".format(variable, dims))
        view = self._steps(da, (member, self._time_name))
        if chunk_steps is not None:
            shape = view.shape if only is None else (T,) + view.shape[1:]
            return view.reader(only=only), shape, _producer_dtype(da.dtype), ids, starts, member
        slab = view.slab(only)
        slab = np.ascontiguousarray(slab, dtype=_producer_dtype(slab.dtype))
        return slab, slab.shape, slab.dtype, ids, starts, member

    def calc_anom(self, variable, window=1, smooth=1, groupby='dayofyear', clim=None, segments=None, chunk_steps=None, pool=True):
        """adds the variable 'anom': departure of `variable` from its climatology (calc_clim, or the one given as `clim`:
        a labelled array over `groupby` on this grid, or the path of one), smoothed with a centred running mean over `smooth`
        timesteps.  The slab also stays resident on the GPU: a following run_contrack(variable='anom') starts from HBM.
        segments (extension, the meaning it has in run_contrack): None -- one series, the smoothing crosses every break, as the
        reference's does; 'gaps' or an int array of start indices -- the smoothing does not cross a break ('anom' is NaN where its
        window would); the name of a member dimension -- the variable is 4-D in any dim order, the smoothing stays inside each
        member, 'anom' gets the variable's own dims and the climatology is pooled over all members (pool=True, the ensemble
        climatology) or is each member's own (pool=False: what xarray's grouped arithmetic gives on a 4-D variable, one call per
        member).  The resident slab is not kept for member calls.
        chunk_steps (extension): the variable is read slice by slice (`isel`, a chunk that spans two members in two pieces) and
        passes through chunk-sized device buffers -- twice without `clim`, once with it; only 'anom' is built on the host and
        nothing stays resident."""
        self._ensure_set_up()
        ids, uniq = self._group_ids(groupby)
        if segments is None and chunk_steps is None:
            view = self._steps(self.ds[variable], (self._time_name,))
            slab = view.slab()
            if slab.dtype.kind != "f":
                slab = slab.astype(np.float64)
        clim_arr = None
        if clim is None:
            logger.info('Calculating climatological mean from {}...'.format(variable))
            clim_txt = 'from {} with running window time steps {}'.format(variable, window)
        else:
            logger.info('Reading climatological mean from {}...'.format(clim))
            clim_txt = clim
            clim_mean = _xr().open_dataarray(clim) if isinstance(clim, str) else clim
            if groupby not in clim_mean.dims:
                raise ValueError("the climatology must have the dimension {!r}".format(groupby))
            if hasattr(clim_mean, "reindex"):       # regrid to this grid (nearest neighbour), as the reference does
                clim_mean = clim_mean.reindex(**{self._latitude_name: self.ds[self._latitude_name],
                                                 self._longitude_name: self.ds[self._longitude_name]}, method='nearest')
            cd = tuple(clim_mean.dims)
            carr = np.asarray(clim_mean.data).transpose([cd.index(d) for d in (groupby, self._latitude_name, self._longitude_name)])
            cvals = np.asarray(clim_mean[groupby].data if hasattr(clim_mean[groupby], "data") else clim_mean[groupby])
            pos = {v: i for i, v in enumerate(cvals.tolist())}
            missing = [v for v in uniq.tolist() if v not in pos]
            if missing:
                raise ValueError("the climatology has no {} {} (present in {!r}); it covers {}..{}".format(
                    groupby, missing[:5] + (['...'] if len(missing) > 5 else []), variable, cvals.min(), cvals.max()))
            clim_arr = np.stack([carr[pos[v]] for v in uniq.tolist()])       # one plane per group value present in the data
        da = self.ds[variable]
        attrs = {'units': da.attrs['units'], 'long_name': da.attrs['long_name'] + ' Anomaly',
                 'standard_name': da.attrs['long_name'] + ' anomaly',
                 'history': ' '.join(['Calculated from {} with input attributes:', 'smoothing time steps = {},',
                                      'climatology = {}.']).format(variable, smooth, clim_txt)}
        if segments is not None or chunk_steps is not None:
            self.ds['anom'] = (tuple(da.dims), self._anom_segments(variable, ids, len(uniq), window, smooth, clim_arr, segments, chunk_steps, pool, attrs), attrs)
            self._anom_resident, self._anom_resident_name = None, 'anom'
            logger.info('Calculating Anomaly... DONE')
            return
        if self._vmean_resident_for(variable, slab):         # (the mean calc_vertical_mean left in HBM: nothing to upload, same bits)
            anom, _ = _tracker().anomalies_resident(ids, len(uniq), window=window, smooth=smooth, clim=clim_arr, keep_resident=True)
        else:
            anom, _ = _tracker().anomalies(slab, ids, len(uniq), window=window, smooth=smooth, clim=clim_arr, keep_resident=True)
        anom.flags.writeable = False                         # (its twin stays in HBM for run_contrack: see _fingerprint)
        self.ds['anom'] = (view.dims, view.restore(anom, view.dims), attrs)
        # (fingerprint of the host twin, identity of the slab in HBM: another instance's calc_anom on the shared handle changes
        # the second and this instance's run_contrack goes back to its own host array)
        self._anom_resident = (_fingerprint(np.asarray(self.ds['anom'].data)), _tracker().resident_generation())
        self._anom_resident_name = 'anom'
        logger.info('Calculating Anomaly... DONE')

    def _anom_segments(self, variable, ids, G, window, smooth, clim_arr, segments, chunk_steps, pool, attrs):
        """'anom' in the variable's own dim order for calc_anom's extensions; the history attribute names the segments"""
        trk = _tracker()
        dims = tuple(self.ds[variable].dims)

        def one(only=None):
            source, shape, dtype, gids, starts, member = self._anom_source(variable, segments, chunk_steps, ids, only)
            if only is not None:
                starts = None                                       # (a member alone is one series)
            if chunk_steps is None:
                return trk.anomalies(source, gids, G, window=window, smooth=smooth, clim=clim_arr, segments=starts)[0], starts, member
            return trk.anomalies_stream(source, gids, G, window=window, smooth=smooth, clim=clim_arr, shape=shape, dtype=dtype,
                                        chunk_steps=int(chunk_steps), segments=starts)[0], starts, member
        member = self._segment_args(variable, self.ds[variable], dims, segments)[0]
        if member is not None and not pool:
            M = self.ds[variable].shape[dims.index(member)]
            parts = [one(m) for m in range(M)]
            anom, starts = np.concatenate([q[0] for q in parts]), np.arange(M)
        else:
            anom, starts, _ = one()
        if segments is not None:
            attrs['history'] += ', segments = {} ({}){}'.format(segments if isinstance(segments, str) else 'starts', 1 if starts is None else len(starts),
                                                               '' if member is None or pool else ', climatology per member')
        return self._steps(self.ds[variable], (member, self._time_name)).restore(anom, dims)

    def _resident_for(self, variable, arr, shape, is_f64, name='anom'):
        """True if `variable` is the field to track this instance left in HBM -- `name`: 'anom' for every consumer of calc_anom's
        slab; run_contrack passes the name the last producer recorded (calc_anom: 'anom', calc_reversal: its variable) -- and its
        host twin is still the slab resident there"""
        res = getattr(self, "_anom_resident", None)
        if variable != name or getattr(self, "_anom_resident_name", 'anom') != name or res is None or res[0] is None:
            return False
        trk = _tracker()
        return res[0] == _fingerprint(np.asarray(arr)) and res[1] == trk.resident_generation() and \
            trk.resident_anom() == (shape[0], shape[1], shape[2], bool(is_f64))

    def _resident_field(self, variable, shape, is_f64):
        """_resident_for as the consumers of calc_anom's slab ask it: is `variable` 'anom', its (steps, lat, lon) twin still in HBM?"""
        return self._resident_for(variable, self.ds['anom'].data if variable == 'anom' else None, shape, is_f64)

    def _band_rows(self, lat_bounds, default_all=True):
        """(y0, y1, bounds): the rows y0 <= y < y1 whose latitude lies inside lat_bounds (both ends included), which must be
        neighbours; lat_bounds None with default_all: every row, bounds then the coordinate's own extremes"""
        lat = np.asarray(self.ds[self._latitude_name].data, dtype=np.float64)
        bounds = (lat.min(), lat.max()) if lat_bounds is None and default_all else lat_bounds
        rows = np.nonzero((lat >= min(bounds)) & (lat <= max(bounds)))[0]
        if len(rows) == 0 or not np.array_equal(rows, np.arange(rows[0], rows[-1] + 1)):
            raise ValueError("latitude band {} selects no contiguous rows".format(lat_bounds))
        return int(rows[0]), int(rows[-1]) + 1, bounds

    def _slab_pooled(self, variable, segments):
        """((steps, lat, lon) slab, members) for the percentile entries: the variable itself (segments None), or a 4-D variable with
        the member dimension `segments` flattened to (member * time, lat, lon) -- pooling over time is indifferent to the breaks"""
        if segments is not None and (not isinstance(segments, str) or segments == 'gaps'):
            raise ValueError("segments={!r}: the percentile entries take the name of a member dimension (breaks along time do not "
                             "change a percentile over time)".format(segments))
        da = self.ds[variable]
        view = self._steps(da, (self._segment_args(variable, da, tuple(da.dims), segments)[0], self._time_name))
        return view.slab(), 1 if segments is None else view.step_shape[0]

    def percentile_threshold(self, variable='anom', q=0.90, lat_bounds=(50, 80), groupby=None, window=1, segments=None):
        """the more objective threshold of the reference's README (README.rst:150-151):
        block[variable].sel(latitude=band).quantile([q], dim='time').mean() -- the mean over the latitude band of the
        per-grid-point q-quantile over time.  Evaluated on the GPU (exact order statistics, numpy's linear interpolation).

        With groupby ('dayofyear', 'month', 'season', ...) the README's recommended recipe (README.rst:235-240): per value of
        time.<groupby> the q-quantile of the whole band pooled over every timestep whose group lies in the centred window of
        `window` groups around it (circular: 1 January sees late December), np.nanquantile in float64.  Returns a 1-D labelled
        array over `groupby` (the values present, ascending); with groupby='dayofyear' it can be given to
        run_contrack(threshold=...) as it is.
        segments (extension): the name of a member dimension of a 4-D variable -- the members are pooled: the variable is taken as
        (member * time, lat, lon) and every member's steps carry the groups of the time axis."""
        if groupby is not None:
            _check_percentile_args(q, window)
        self._ensure_set_up()
        slab, M = self._slab_pooled(variable, segments)
        y0, y1, _ = self._band_rows(lat_bounds, default_all=False)
        if slab.dtype.kind != "f":
            slab = slab.astype(np.float64)
        ids, uniq = (None, None) if groupby is None else self._group_ids(groupby)
        if ids is not None and M > 1:
            ids = np.tile(ids, M)
        resident = segments is None and self._resident_field(variable, slab.shape, slab.dtype != np.float32)
        if groupby is None:
            return _tracker().percentile(None if resident else slab, y0, y1, q)
        vals = _tracker().percentile_groups(None if resident else slab, y0, y1, ids, len(uniq), q, int(window))
        da = self.ds[variable]
        attrs = {'long_name': '{} percentile threshold'.format(variable), 'q': float(q), 'window': int(window),
                 'lat_bounds': (float(min(lat_bounds)), float(max(lat_bounds))),
                 'history': ' '.join(['Calculated from {} with input attributes:', 'q = {},', 'latitude band = {},', 'groupby = {},',
                                      'window = {} groups.']).format(variable, q, tuple(lat_bounds), groupby, window)}
        if 'units' in getattr(da, "attrs", {}):
            attrs['units'] = da.attrs['units']
        return self._wrap(da, vals, (groupby,), {groupby: uniq}, attrs, name='{}_q{:g}'.format(variable, float(q) * 100))

    def percentile_field(self, variable='anom', q=0.90, groupby='dayofyear', window=1, lat_bounds=None, segments=None):
        """the local definition of an extreme: per value of time.<groupby> and per grid point the q-quantile over every timestep
        whose group lies in the centred window of `window` groups around it (circular: 1 January sees late December),
        np.nanquantile in float64, evaluated exactly on the GPU.  Returns a labelled array over (groupby, latitude, longitude) on
        the whole grid (the group values present, ascending); rows outside lat_bounds (None: every row) are NaN and are never
        flagged.  With groupby='dayofyear' it can be given to run_contrack(threshold=...) as it is.
        segments (extension): the name of a member dimension of a 4-D variable; the members are pooled as in percentile_threshold."""
        _check_percentile_args(q, window)
        self._ensure_set_up()
        slab, M = self._slab_pooled(variable, segments)
        y0, y1, bounds = self._band_rows(lat_bounds)
        if slab.dtype.kind != "f":
            slab = slab.astype(np.float64)
        ids, uniq = self._group_ids(groupby)
        if M > 1:
            ids = np.tile(ids, M)
        resident = segments is None and self._resident_field(variable, slab.shape, slab.dtype != np.float32)
        band = _tracker().percentile_field(None if resident else slab, y0, y1, ids, len(uniq), q, int(window))
        vals = np.full((len(uniq),) + slab.shape[1:], np.nan)
        vals[:, y0:y1] = band
        da = self.ds[variable]
        attrs = {'long_name': '{} percentile threshold field'.format(variable), 'q': float(q), 'window': int(window),
                 'lat_bounds': (float(min(bounds)), float(max(bounds))),
                 'history': ' '.join(['Calculated from {} with input attributes:', 'q = {},', 'latitude band = {},', 'groupby = {},',
                                      'window = {} groups.']).format(variable, q, tuple(float(b) for b in bounds), groupby, window)}
        if 'units' in getattr(da, "attrs", {}):
            attrs['units'] = da.attrs['units']
        coords = {groupby: uniq}
        for name in (self._latitude_name, self._longitude_name):
            coords[name] = np.asarray(self.ds[name].data)
        return self._wrap(da, vals, (groupby, self._latitude_name, self._longitude_name), coords, attrs,
                          name='{}_q{:g}_field'.format(variable, float(q) * 100))

    def _std_band(self, variable, groupby, window, lat_bounds, ddof, skipna, segments):
        """(std planes of the band float64 (G, rows, nx), (y0, y1), the G group values or None, the (steps, lat, lon) shape, the band's
        bounds) for std_field and std_threshold: the arguments checked, the slab chosen (host or resident) as the percentile entries do"""
        _check_std_args(window, ddof)
        self._ensure_set_up()
        slab, M = self._slab_pooled(variable, segments)
        y0, y1, bounds = self._band_rows(lat_bounds)
        if slab.dtype.kind != "f":
            slab = slab.astype(np.float64)
        if groupby is None:
            ids, uniq = np.zeros(self._dim_size(self._time_name), dtype=np.int32), None
        else:
            ids, uniq = self._group_ids(groupby)
        G = 1 if uniq is None else len(uniq)
        _check_std_args(window, ddof, G, skipna)
        if M > 1:
            ids = np.tile(ids, M)
        resident = segments is None and self._resident_field(variable, slab.shape, slab.dtype != np.float32)
        band = _tracker().std_field(None if resident else slab, y0, y1, ids, G, int(window), int(ddof), bool(skipna))
        return band, (y0, y1), uniq, slab.shape, (float(min(bounds)), float(max(bounds)))

    def _std_attrs(self, variable, long_name, k, ddof, window, bounds, groupby):
        attrs = {'long_name': long_name.format(variable), 'k': float(k), 'ddof': int(ddof), 'window': int(window), 'lat_bounds': bounds,
                 'history': ' '.join(['Calculated from {} with input attributes:', 'k = {},', 'ddof = {},', 'latitude band = {},', 'groupby = {},',
                                      'window = {} groups.']).format(variable, k, ddof, bounds, groupby, window)}
        if 'units' in getattr(self.ds[variable], "attrs", {}):
            attrs['units'] = self.ds[variable].attrs['units']
        return attrs

    def std_field(self, variable='anom', k=1.0, groupby='dayofyear', window=1, lat_bounds=None, ddof=0, skipna=True, segments=None):
        """the "k standard deviations of the local anomaly" threshold (the std_dev half of the reference's open item,
        contrack.py:9-10): per value of time.<groupby> and per grid point k times the standard deviation over every timestep whose
        group lies in the centred window of `window` groups around it (circular: 1 January sees late December), in time order --
        block[variable].groupby('time.' + groupby).std('time') with a window, as np.nanstd (skipna False: np.std) with `ddof` in
        float64 gives it, evaluated exactly on the GPU (ctk_std_field_*, include/contrack_hip.h); the multiplication by k is numpy's,
        on the result; k may be negative (gorl='<=').  Returns a labelled array over (groupby, latitude, longitude) on the whole grid
        (the group values present, ascending); rows outside lat_bounds (None: every row) are NaN and are never flagged.  With
        groupby='dayofyear' it can be given to run_contrack(threshold=...) as it is.  groupby=None: one pool, an array over
        (latitude, longitude), whose values (np.asarray(field.data)) run_contrack(threshold=...) broadcasts over time (labelled, it
        asks for a 'dayofyear' dimension, as xarray's grouped compare does).
        segments (extension): the name of a member dimension of a 4-D variable; the members are pooled as in percentile_threshold,
        in the time order of the flattened (member * time, lat, lon) slab."""
        band, (y0, y1), uniq, shape, bounds = self._std_band(variable, groupby, window, lat_bounds, ddof, skipna, segments)
        vals = np.full((band.shape[0],) + tuple(shape[1:]), np.nan)
        vals[:, y0:y1] = float(k) * band
        attrs = self._std_attrs(variable, '{} standard-deviation threshold field', k, ddof, window, bounds, groupby)
        coords = {} if groupby is None else {groupby: uniq}
        for name in (self._latitude_name, self._longitude_name):
            coords[name] = np.asarray(self.ds[name].data)
        dims = (self._latitude_name, self._longitude_name)
        return self._wrap(self.ds[variable], vals[0] if groupby is None else vals, dims if groupby is None else (groupby,) + dims, coords, attrs,
                          name='{}_std_field'.format(variable))

    def std_threshold(self, variable='anom', k=1.0, lat_bounds=(50, 80), groupby=None, window=1, ddof=0, skipna=True, segments=None):
        """the scalar recipe in the shape of the reference's README (README.rst:150-151): k times
        block[variable].sel(latitude=band).std(dim='time').mean() -- the mean over the latitude band (np.mean on the host, float64) of
        the per-grid-point standard deviation over time that std_field computes on the GPU.  Returns a float; with groupby
        ('dayofyear', 'month', ...) a 1-D labelled array over `groupby` (the values present, ascending) of k * the band mean of every
        group's plane, pooled over the centred window of `window` groups -- with groupby='dayofyear' it can be given to
        run_contrack(threshold=...) as it is."""
        band, _rows, uniq, _shape, bounds = self._std_band(variable, groupby, window, lat_bounds, ddof, skipna, segments)
        vals = np.array([float(k) * np.mean(plane) for plane in band])
        if groupby is None:
            return float(vals[0])
        attrs = self._std_attrs(variable, '{} standard-deviation threshold', k, ddof, window, bounds, groupby)
        return self._wrap(self.ds[variable], vals, (groupby,), {groupby: uniq}, attrs, name='{}_std'.format(variable))

    # ---- the hot path (contrack.py:583-796) -----------------------------------------------------------------
    def _dayofyear(self):
        t = self.ds[self._time_name]
        try:
            return np.asarray(t.dt.dayofyear)
        except AttributeError:
            v = np.asarray(t.data).astype('datetime64[D]')
            return (v - v.astype('datetime64[Y]')).astype(int) + 1

    def _coord(self, da, name):
        try:
            c = da[name]
        except (KeyError, IndexError, TypeError):
            return None
        return np.asarray(getattr(c, "data", c))

    def _doy_field(self, threshold):
        """a DataArray over 'dayofyear' and the spatial dims (any order; a missing spatial dim broadcasts) -> (planes, plane_of_step):
        transposed by name, the spatial labels aligned with the dataset's (a reversed latitude is reordered), the plane of every
        step from its day of year (contrack.py:648-661 with a threshold that varies by grid point)"""
        lat_n, lon_n = self._latitude_name, self._longitude_name
        dims = tuple(threshold.dims)
        extra = [d for d in dims if d not in ('dayofyear', lat_n, lon_n)]
        if extra:
            raise ValueError("the threshold's dims {} must be 'dayofyear', {!r} and {!r}".format(dims, lat_n, lon_n))
        arr = np.asarray(threshold.data)
        for d in (lat_n, lon_n):
            if d not in dims:
                arr, dims = arr[..., None], dims + (d,)
        arr = arr.transpose([dims.index(d) for d in ('dayofyear', lat_n, lon_n)])
        for ax, d in ((1, lat_n), (2, lon_n)):
            want = np.asarray(self.ds[d].data)
            if arr.shape[ax] == 1 and d not in threshold.dims:
                arr = np.repeat(arr, len(want), axis=ax)
                continue
            have = self._coord(threshold, d)
            if have is None:
                if arr.shape[ax] != len(want):
                    raise ValueError("the threshold has {} {} values, the dataset {}".format(arr.shape[ax], d, len(want)))
                continue
            if have.shape == want.shape and np.array_equal(have, want):
                continue
            pos = {v: i for i, v in enumerate(have.tolist())}
            if len(pos) != len(have) or len(have) != len(want) or any(v not in pos for v in want.tolist()):
                raise ValueError("the threshold's {} labels are not the dataset's".format(d))
            arr = np.take(arr, [pos[v] for v in want.tolist()], axis=ax)
        coord = self._coord(threshold, 'dayofyear')
        if coord is None:
            coord = np.arange(1, arr.shape[0] + 1)
        pos = {int(d): i for i, d in enumerate(coord)}
        plane_of_step = np.array([pos[int(d)] for d in self._dayofyear()], dtype=np.int32)      # KeyError: a day the threshold lacks
        return np.ascontiguousarray(arr), plane_of_step

    def _threshold_args(self, threshold, shape, sort, T, dtype):
        """(per-step thresholds, None) or (None, (planes, plane_of_step)) for a threshold field"""
        if hasattr(threshold, "dims") and hasattr(threshold, "data") and np.ndim(threshold.data) >= 2:
            if 'dayofyear' not in threshold.dims:
                # (xarray's grouped compare refuses it as well)
                raise ValueError("a threshold with dims {} has no 'dayofyear' dimension".format(tuple(threshold.dims)))
            return None, self._doy_field(threshold)
        if is_threshold_field(threshold):
            return None, broadcast_field(threshold, shape, sort)
        return self._thresholds_per_step(threshold, T, dtype), None

    def _thresholds_per_step(self, threshold, T, dtype):
        """scalar, or a 1-D DataArray over 'dayofyear' (contrack.py:648-661) -> per-timestep values"""
        if hasattr(threshold, "dims") and hasattr(threshold, "data"):
            values = np.asarray(threshold.data)
            if 'dayofyear' in getattr(threshold, "dims", ()):
                coord = None
                try:
                    coord = np.asarray(threshold['dayofyear'].data)
                except Exception:
                    pass
                doy = self._dayofyear()
                if coord is None:
                    coord = np.arange(1, len(values) + 1)
                pos = {int(d): i for i, d in enumerate(coord)}
                values = np.array([values[pos[int(d)]] for d in doy], dtype=values.dtype)
            return prepare_thresholds(values, T, dtype)
        return prepare_thresholds(threshold, T, dtype)

    def _segment_args(self, variable, da, dims, segments):
        """`segments` as run_contrack documents it -> (name of the member dimension or None, segment starts or None, steps of the
        time axis)"""
        member = segments if isinstance(segments, str) and segments != 'gaps' else None
        if member is not None:
            if member not in dims:
                raise ValueError("segments={!r}: the variable {!r} has no such dimension (dims {})".format(member, variable, dims))
            if len(dims) != 4:
                raise ValueError("segments={!r}: the variable must be 4-D ({!r}, time, lat, lon in any order), it has dims {}".format(member, member, dims))
        T = da.shape[dims.index(self._time_name)]
        if member is not None:
            starts = np.arange(da.shape[dims.index(member)], dtype=np.int64) * T
        elif isinstance(segments, str):
            starts = gap_starts(self._time_steps())
        else:
            starts = None if segments is None else segment_starts(segments, T)
        return member, starts, T

    def run_contrack(self, variable, threshold, gorl, overlap, persistence, twosided=True, chunk_steps=None, segments=None):
        """Spatial and temporal tracking of closed contours; adds the integer variable 'flag' to the dataset.

        variable: name of the input field; threshold: number, 1-D DataArray over 'dayofyear', a threshold field -- a DataArray over
        'dayofyear' and the spatial dims (any order, labels aligned by name) or a numpy array that broadcasts against the variable
        in its own dim order (e.g. (lat, lon) or (time, lat, lon)); gorl: one of
        [>, >=, <, <=, ge, le, gt, lt]; overlap: fraction [0-1] of area overlap between consecutive steps;
        persistence: minimum life time in time steps; twosided: forward+backward overlap test (True) or forward
        only.
        chunk_steps (extension, not in the reference): stream the variable through the GPU in slices of that many time steps
        (0: about 256 MB each) instead of materialising it on the host and in HBM -- for a lazily loaded netCDF variable
        (xr.open_dataset) each slice is read from the file when its turn comes (`isel(time=slice)`), and the device holds four
        slices and the bit mask instead of twice the slab.  Same result.
        segments (extension): the time axis as independent series -- None (one series, the reference's behaviour), an int array of
        segment start indices along time, 'gaps' (a new segment wherever the step to the previous timestamp is larger than the
        smallest step: a seasonal selection) or the name of an extra dimension of the variable (e.g. 'member': each member is a
        segment; the threshold is a number, a per-time vector or a 'dayofyear' DataArray, applied to every member).  Every
        segment is tracked as if alone (no overlap, filter exemption or 3-D link across a break); ids stay unique over the
        whole result.  With chunk_steps: 'gaps' and a member dimension stream as any other call (each slice is read when its turn
        comes -- for a member dimension `isel(member=m, time=slice)`, a chunk that spans two members in two pieces; the flattened
        (member * time, lat, lon) slab is never built on the host); explicit start indices together with chunk_steps stay refused
        here -- track_numpy(..., segments=starts, chunk_steps=n) takes them."""
        if segments is not None and chunk_steps is not None and not isinstance(segments, str):
            raise ValueError("segments given as start indices and chunk_steps cannot be combined in run_contrack; use segments='gaps' or a "
                             "member dimension, or track_numpy(..., segments=starts, chunk_steps=n)")
        self._ensure_set_up()
        da = self.ds[variable]
        dims = tuple(da.dims)
        member, starts, T = self._segment_args(variable, da, dims, segments)
        nseg = 1 if starts is None else len(starts)
        logger.info("\nRun ConTrack \n########### \n    threshold:    {} {} \n    overlap:      {} \n"
                    "    persistence:  {} time steps".format(gorl, threshold, overlap, persistence) +
                    ("" if segments is None else " \n    segments:     {}".format(nseg)))
        logger.info("Find individual contours...")
        if gorl not in _native.CMP_OPS:
            raise ValueError(_native.GORL_ERRMSG)
        # a member dimension is flattened to steps m * T + t, each member one segment; the threshold of a time step applies to every member
        view = self._steps(da, (member, self._time_name))
        lat = self.ds[self._latitude_name].data
        wrow = row_weights(lat, self._dlat, self._dlon)
        trk = _tracker()

        def thresholds(dtype):
            if member is not None:
                return self._member_threshold_args(threshold, member, view.step_shape[0], T, dtype)
            return self._threshold_args(threshold, da.shape, [dims.index(d) for d in (self._time_name,) + view.tail], T, dtype)
        # threshold, 2-D labelling, overlap filter, 3-D tracking and persistence are ONE call into the library (the reference logs
        # them as it goes through them, contrack.py:646-772)
        logger.info("Apply overlap...")
        logger.info("Apply persistence...")
        if chunk_steps is not None:
            # the variable is read slice by slice when its turn comes and passes through chunk-sized device
            # buffers -- a chunk that spans two members in two pieces; the flattened slab exists nowhere on the host
            slab, reader, dtype = None, view.reader(), _producer_dtype(da.dtype)
            thr, field = thresholds(dtype)
            seg = {} if starts is None else {"segments": starts}        # (no segments: the call as it has always been made)
            call = lambda t: trk.track_stream(reader, t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided, shape=view.shape, dtype=dtype,
                                              chunk_steps=int(chunk_steps), **seg)
            flag, n_tracked = call(thr) if field is None else _track_field(trk, field[0], field[1], call)
        else:
            slab = view.slab()
            if member is not None:                           # (without members the variable's own type decides a Python threshold's)
                slab = np.ascontiguousarray(slab, dtype=_producer_dtype(slab.dtype))
            thr, field = thresholds(slab.dtype)
            if member is None and self._resident_for(variable, da.data, slab.shape, slab.dtype != np.float32,
                                                     name=getattr(self, "_anom_resident_name", 'anom')):
                # calc_anom (or calc_reversal) left this very slab in HBM: no host-to-device copy
                call = lambda t: trk.track_resident(t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided)
            else:
                host = np.ascontiguousarray(slab, dtype=_producer_dtype(slab.dtype))
                call = lambda t: trk.track(host, t, _native.CMP_OPS[gorl], wrow, overlap, persistence, twosided, f64=host.dtype == np.float64)
            flag, n_tracked = _track_segments(trk, starts, lambda: call(thr) if field is None else _track_field(trk, field[0], field[1], call))
        if slab is not None and slab.nbytes > (4 << 30):
            trk.release_io()               # a big one-off slab: do not keep 2 x its size allocated on the GPU
        logger.info("Create new variable 'flag'...")
        # scipy.ndimage.label returns int32 labels, int64 from 2^31 - 2 elements on (scipy/_measurements.py:190-199), and with it the
        # reference's 'flag' (contrack.py:687, :751).  The library writes int32 ids (more than 2^31 - 2 ids are an error, never a
        # wrap-around); slabs of that size get the reference's dtype here.
        if flag.size >= INT64_FLAG_FROM:
            flag = flag.astype(np.int64)
        attrs = {'units': 'flag', 'long_name': 'contrack flag', 'standard_name': 'contrack flag',
                 'history': ' '.join(['Calculated from {} with input attributes:', 'threshold = {} {},', 'overlap fraction = {},',
                                      'persistence time steps = {}.', 'twosided = {}']).format(
                     variable, gorl, threshold, overlap, persistence, twosided),
                 'reference': 'https://github.com/steidani/ConTrack'}
        if segments is not None:
            attrs['history'] += ', segments = {} ({})'.format(segments if isinstance(segments, str) else 'starts', nseg)
        self.ds['flag'] = (dims, view.restore(flag, dims), attrs)
        st = _tracker().stats()
        if st.get("off_fused_path_reason", 0):
            # not an error: the result is the same, the call was slower (exact areas / host resolver)
            why = {1: "the co-occurrence table had to be regrown (host resolver)", 2: "a removal cascade longer than 240 steps (host resolver)",
                   3: "table regrowth and a long removal cascade (host resolver)",
                   4: "{} overlap decisions on rounding boundaries were re-evaluated with numpy-order sums".format(st.get("exact_fixups", 0))}
            logger.info("run_contrack left the fused device path: " + why.get(st["off_fused_path_reason"], "host resolver"))
        logger.info("Running contrack... DONE\n{} contours tracked".format(n_tracked))

    def _member_threshold_args(self, threshold, member, M, T, dtype):
        """(thr, field) of a call over M members of T steps each: the threshold of a time step applies to every member"""
        if hasattr(threshold, "dims") and hasattr(threshold, "data") and np.ndim(threshold.data) >= 2:
            if 'dayofyear' not in threshold.dims:
                raise ValueError("a threshold with dims {} has no 'dayofyear' dimension".format(tuple(threshold.dims)))
            planes, pos = self._doy_field(threshold)
            return None, (planes, np.tile(pos, M))
        if is_threshold_field(threshold):
            raise ValueError("segments={!r}: a numpy threshold field cannot be combined with a member dimension; give a number, a "
                             "per-time vector or a 'dayofyear' DataArray".format(member))
        return np.tile(self._thresholds_per_step(threshold, T, dtype), M), None

    # ---- blocking frequency (README.rst:159-160), consumer of `flag` ------------------------------------------------------
    def _consumer_dims(self, name, what="flag variable"):
        """(dims, member) of a variable run_lifecycle / calc_frequency consume: time, lat, lon in any order and at most one more
        dimension (its name, else None) -- the member dimension run_contrack(segments=<dim>) tracks over"""
        dims = tuple(self.ds[name].dims)
        names = (self._time_name, self._latitude_name, self._longitude_name)
        extra = [d for d in dims if d not in names]
        if any(d not in dims for d in names) or len(extra) > 1 or len(set(dims)) != len(dims):
            raise ValueError("the {} {!r} must have the dimensions {} and at most one more (a member dimension), it has {}".format(what, name, names, dims))
        return dims, (extra[0] if extra else None)

    def _dim_values(self, name, size):
        """the coordinate of a dimension, or its indices if it has none"""
        try:
            vals = np.asarray(self.ds[name].data)
        except (KeyError, AttributeError):
            return np.arange(size)
        return vals if vals.shape == (size,) else np.arange(size)

    @staticmethod
    def _group_plan(ids, uniq, T, M=None, pool=False):
        """the groups of a map over the flat slab (_Steps) as the library takes them: (group, G, per_member).  ids: one group id
        per time step (uniq: the groups' values) or None; M: the size of the member dimension, None without one.  Members that are
        not pooled keep maps of their own: the library sees group m * G + g at flat step m * T + t.  group None: one group."""
        G = 1 if ids is None else len(uniq)
        per_member = M is not None and not pool
        gids = np.zeros(T, dtype=np.int32) if ids is None else ids
        if per_member:
            gids = (np.arange(M, dtype=np.int32)[:, None] * G + gids[None, :]).reshape(-1)
        else:
            gids = np.tile(gids, 1 if M is None else M)
        return (gids if (per_member or ids is not None) else None), G, per_member

    def _map_layout(self, dims, member, pool, groupby, uniq, M, G):
        """what a grouped map looks like as a labelled array: (out_dims, coords, shaped).  out_dims: the variable's own dims, the
        group dim in the time dim's place (no groupby: gone) and a pooled member dim gone; shaped(a) brings the library's
        (M * G or G, lat, lon) result into them."""
        names = (self._time_name, self._latitude_name, self._longitude_name)
        per_member = member is not None and not pool
        lead = ((member,) if per_member else ()) + ((groupby,) if groupby is not None else ())
        have = lead + names[1:]                                      # the axes of the result once shaped
        gone = ((self._time_name,) if groupby is None else ()) + ((member,) if member is not None and pool else ())
        out_dims = tuple(groupby if d == self._time_name else d for d in dims if d not in gone)

        def shaped(a):
            if per_member:
                a = a.reshape((M, G) + a.shape[1:])
            if groupby is None:
                a = a[:, 0] if per_member else a[0]
            return np.ascontiguousarray(a.transpose([have.index(d) for d in out_dims]))
        coords = {} if groupby is None else {groupby: uniq}
        if per_member:
            coords[member] = self._dim_values(member, M)
        for name in names[1:]:
            coords[name] = np.asarray(self.ds[name].data)
        return out_dims, coords, shaped

    def calc_frequency(self, flag='flag', groupby=None, above=0, chunk_steps=None, pool=False):
        """percentage of time steps with flag > above at every grid point: xr.where(ds[flag] > above, 1, 0).sum(dim='time') /
        ntime * 100 -- the README's blocking frequency with above=1 -- or, with groupby ('month', 'season', 'year', ...), the same
        per value of time.<groupby> (ascending; seasons as xarray orders them: DJF, JJA, MAM, SON), as groupby(...).sum() /
        group size * 100.  Returns a labelled float64 array ('%') over the variable's own spatial dims, the group dim in the time
        dim's place; it is not added to the dataset.  The count runs on the GPU (frequency_numpy).
        A 4-D flag (extension: time, lat, lon and a member dimension in any order, what run_contrack(segments=<dim>) writes) gives
        the frequency of every member, the member dimension in its place, each group's size counted inside one member; pool=True
        pools the members (the member dimension is dropped, a group's size is its size x members).  pool is ignored for a 3-D flag.
        chunk_steps (extension): the flag is read slice by slice (`isel`, a chunk that spans two members in two pieces) and passes
        through chunk-sized device buffers; the slab is never built on the host.  Same bits."""
        self._ensure_set_up()
        da = self.ds[flag]
        dims, member = self._consumer_dims(flag)
        if np.dtype(da.dtype).kind not in "iub":
            raise ValueError("flag must be an integer field")
        ids, uniq = (None, None) if groupby is None else self._group_ids(groupby)
        T = da.shape[dims.index(self._time_name)]
        M = None if member is None else da.shape[dims.index(member)]
        group, G, per_member = self._group_plan(ids, uniq, T, M, pool)
        view = self._steps(da, (member, self._time_name))
        source = view.slab() if chunk_steps is None else view.reader(integer=True)
        counts = frequency_numpy(source, group, above=above, percent=False, chunk_steps=chunk_steps, shape=view.shape)
        counts = counts.reshape((-1,) + counts.shape[-2:])
        n = np.bincount(ids, minlength=G) if ids is not None else np.array([T])
        n = np.tile(n, M) if per_member else n * (M or 1)        # a group's size inside one member / over all of them
        out_dims, coords, shaped = self._map_layout(dims, member, pool, groupby, uniq, M, G)
        attrs = {'units': '%', 'long_name': 'contrack frequency', 'standard_name': 'contrack frequency',
                 'history': ' '.join(['Calculated from {} with input attributes:', 'flag > {},', 'groupby = {}.']).format(
                     flag, above, groupby)}
        return self._wrap(da, shaped(frequency_percent(counts, n)), out_dims, coords, attrs, name='frequency')

    # ---- blocked spells per grid point: the maps beside the frequency map of a blocking climatology ---------------------------
    def calc_spells(self, flag='flag', groupby=None, above=0, by_id=True, min_duration=1, segments=None, chunk_steps=None, pool=False):
        """blocked spells at every grid point: a spell is a maximal run of consecutive time steps with flag > above (by_id: and the
        same id) that no segment break cuts; it counts if it lasts min_duration steps or more and belongs to the group (groupby:
        'month', 'season', 'year', ... as calc_frequency) of its FIRST step.  Returns a dict of labelled arrays over the flag
        variable's own spatial dims, the group dim in the time dim's place: 'events' (number of spells, '1'), 'steps' (sum of their
        durations), 'longest' (the longest one) -- int64, 'timesteps' -- and 'duration' (steps / events in float64, NaN where
        there is no event).  Nothing is added to the dataset.  The scan runs on the GPU (spells_numpy).
        segments: what run_contrack takes -- None, 'gaps' (a break wherever the time axis has a gap: what a DJF-only dataset
        needs, so that no spell bridges February and December), an array of segment starts, or the name of the member dimension
        (which changes nothing: its members are segments anyway).  A 4-D flag (time, lat, lon and a
        member dimension in any order) gives the maps of every member, the member dimension in its place, every member a segment
        of its own; pool=True pools the members (events and steps add up, longest is the maximum).  pool is ignored for a 3-D flag.
        chunk_steps: the flag is read slice by slice (`isel`, a chunk that spans two members in two pieces) and passes through
        chunk-sized device buffers; the slab is never built on the host.  Same numbers."""
        self._ensure_set_up()
        da = self.ds[flag]
        dims, member = self._consumer_dims(flag)
        if np.dtype(da.dtype).kind not in "iub":
            raise ValueError("flag variable {!r} is not an integer field".format(flag))
        seg_member, starts, T = self._segment_args(flag, da, dims, segments)
        if seg_member is not None:                               # (the member dimension by name: its members are segments anyway)
            starts = None
        ids, uniq = (None, None) if groupby is None else self._group_ids(groupby)
        M = None if member is None else da.shape[dims.index(member)]
        group, G, per_member = self._group_plan(ids, uniq, T, M, pool)
        if member is not None:                                   # every member a segment of its own, with the breaks inside it
            inner = np.zeros(1, dtype=np.int64) if starts is None else starts
            starts = (np.arange(M, dtype=np.int64)[:, None] * T + inner[None, :]).reshape(-1)
        view = self._steps(da, (member, self._time_name))
        source = view.slab() if chunk_steps is None else view.reader(integer=True)
        maps = spells_numpy(source, group, above=above, by_id=by_id, min_duration=min_duration, segments=starts, chunk_steps=chunk_steps, shape=view.shape)
        maps = [a.reshape((-1,) + a.shape[-2:]) for a in maps]
        maps.append(spell_duration(maps[1], maps[0]))
        out_dims, coords, shaped = self._map_layout(dims, member, pool, groupby, uniq, M, G)
        history = ' '.join(['Calculated from {} with input attributes:', 'flag > {},', 'groupby = {},', 'by_id = {},', 'min_duration = {}.']).format(
            flag, above, groupby, bool(by_id), min_duration)
        out = {}
        for key, a, units in zip(('events', 'steps', 'longest', 'duration'), maps, ('1', 'timesteps', 'timesteps', 'timesteps')):
            attrs = {'units': units, 'long_name': 'contrack spell ' + key, 'standard_name': 'contrack spell ' + key, 'history': history}
            out[key] = self._wrap(da, shaped(a), out_dims, coords, attrs, name=key)
        return out

    # ---- composite over the flagged time steps: what a study computes after the frequency map (README.rst:156-164) ----------
    def calc_composite(self, variable, flag='flag', groupby=None, above=0, skipna=False, stat='mean', chunk_steps=None, pool=False, return_count=False):
        """mean (stat='mean') or sum (stat='sum') of `variable` over the time steps with flag > above at every grid point:
        ds[variable].where(ds[flag] > above).mean('time') -- or, with groupby ('month', 'season', 'year', ...), the same per value
        of time.<groupby>, ordered as calc_frequency orders them.  The sums are float64 and added in time order on the GPU
        (composite_numpy), so the result is reproducible bit for bit; a grid point that is never flagged gives NaN (mean) or 0
        (sum).  skipna: a NaN value is not counted; without it one makes the result NaN.  Returns a labelled float64 array over the
        variable's spatial dims, the group dim in the time dim's place, with the variable's units; it is not added to the dataset.
        return_count=True: (composite, n), n the uint32 count of selected steps with the same dims.
        A 4-D flag (time, lat, lon and a member dimension in any order, what run_contrack(segments=<dim>) writes; `variable` must
        have the same dims) gives one composite per member, the member dimension in its place; pool=True pools the members (the
        member dimension is dropped; the order of the additions is member after member, each in time order).
        chunk_steps: both variables are read slice by slice (`isel`, a chunk that spans two members in two pieces) and pass
        through chunk-sized device buffers; neither slab is built on the host.  Same bits.  When `variable` is the anomaly
        calc_anom left in HBM, only the flags are uploaded."""
        self._ensure_set_up()
        if stat not in ('mean', 'sum'):
            raise ValueError("stat must be 'mean' or 'sum', not {!r}".format(stat))
        fda, vda = self.ds[flag], self.ds[variable]
        dims, member = self._consumer_dims(flag)
        vdims = tuple(vda.dims)
        if sorted(vdims) != sorted(dims) or any(vda.shape[vdims.index(d)] != fda.shape[dims.index(d)] for d in dims):
            raise ValueError("the variable {!r} has dims {}, the flag variable {!r} has {}: they must be the same".format(variable, vdims, flag, dims))
        if np.dtype(fda.dtype).kind not in "iub":
            raise ValueError("flag variable {!r} is not an integer field".format(flag))
        ids, uniq = (None, None) if groupby is None else self._group_ids(groupby)
        T = fda.shape[dims.index(self._time_name)]
        M = None if member is None else fda.shape[dims.index(member)]
        group, G, per_member = self._group_plan(ids, uniq, T, M, pool)
        vtype = _native._field_dtype(vda.dtype)
        fview, vview = self._steps(fda, (member, self._time_name)), self._steps(vda, (member, self._time_name))
        if chunk_steps is None:
            field = vview.slab().astype(vtype, copy=False)
            resident = self._resident_field(variable, field.shape, vtype == np.float64)
            s, n = composite_numpy(fview.slab(), None if resident else field, group, above=above, skipna=skipna, dtype=vtype)
        else:
            s, n = composite_numpy(fview.reader(integer=True), vview.reader(), group, above=above, skipna=skipna, chunk_steps=chunk_steps, shape=fview.shape,
                                   dtype=vtype)
        s, n = s.reshape((-1,) + s.shape[-2:]), n.reshape((-1,) + n.shape[-2:])
        out = composite_mean(s, n) if stat == 'mean' else s
        out_dims, coords, shaped = self._map_layout(dims, member, pool, groupby, uniq, M, G)
        attrs = {'long_name': 'contrack composite', 'standard_name': 'contrack composite',
                 'history': ' '.join(['Calculated from {} with input attributes:', 'flag = {} > {},', 'groupby = {},', 'stat = {},', 'skipna = {}.']).format(
                     variable, flag, above, groupby, stat, skipna)}
        units = getattr(vda, 'attrs', {}).get('units')
        if units is not None:
            attrs['units'] = units
        res = self._wrap(vda, shaped(out), out_dims, coords, attrs, name='composite')
        if not return_count:
            return res
        cattrs = {'long_name': 'contrack composite count', 'units': '1', 'history': attrs['history']}
        return res, self._wrap(vda, shaped(n), out_dims, coords, cattrs, name='count')

    # ---- reductions over space that keep the time axis: Hovmoeller diagram and blocked-area series ---------------------------
    def _band_tables(self, flag, lat_bounds, above, variable, chunk_steps, sectors, columns):
        """what calc_hovmoller and calc_blocked_area share: band_numpy over the flat slab of `flag` (and of `variable`), as
        (tables, dims, member, M, T, (y0, y1), weights, bounds, fda)"""
        self._ensure_set_up()
        fda = self.ds[flag]
        dims, member = self._consumer_dims(flag)
        if np.dtype(fda.dtype).kind not in "iub":
            raise ValueError("flag variable {!r} is not an integer field".format(flag))
        y0, y1, bounds = self._band_rows(lat_bounds)
        y01 = (y0, y1)
        weights = row_weights(np.asarray(self.ds[self._latitude_name].data), self._dlat, self._dlon).astype(np.float64)     # contrack.py:846-848
        T = fda.shape[dims.index(self._time_name)]
        M = None if member is None else fda.shape[dims.index(member)]
        vda = vdims = vtype = None
        if variable is not None:
            vda = self.ds[variable]
            vdims = tuple(vda.dims)
            if sorted(vdims) != sorted(dims) or any(vda.shape[vdims.index(d)] != fda.shape[dims.index(d)] for d in dims):
                raise ValueError("the variable {!r} has dims {}, the flag variable {!r} has {}: they must be the same".format(variable, vdims, flag, dims))
            vtype = _native._field_dtype(vda.dtype)
        fview = self._steps(fda, (member, self._time_name))
        vview = None if vda is None else self._steps(vda, (member, self._time_name))
        if chunk_steps is None:
            field, gen = None, None
            if vda is not None:
                field = vview.slab().astype(vtype, copy=False)
                # (the anomaly slab calc_anom left in HBM: only the flags cross PCIe)
                if self._resident_field(variable, field.shape, vtype == np.float64):
                    field, gen = None, self._anom_resident[1]
            tables = band_numpy(fview.slab(), y01, weights, field, sectors, columns, above=above, dtype=vtype, resident_gen=gen)
        else:
            tables = band_numpy(fview.reader(integer=True), y01, weights, None if vda is None else vview.reader(), sectors, columns, above=above,
                                chunk_steps=chunk_steps, shape=fview.shape, dtype=vtype)
        return tables, dims, member, M, T, y01, weights, (float(min(bounds)), float(max(bounds))), fda

    def _band_layout(self, dims, member, M, T, last, last_values):
        """(out_dims, coords, shaped) of a (M * T or T, n) table as a labelled array: the flag variable's own dims without the latitude,
        `last` (the longitude dim, or 'sector') in the longitude's place"""
        have = ((member,) if member is not None else ()) + (self._time_name, last)
        out_dims = tuple(last if d == self._longitude_name else d for d in dims if d != self._latitude_name)

        def shaped(a):
            a = a.reshape(((M,) if member is not None else ()) + (T, a.shape[-1]))
            return np.ascontiguousarray(a.transpose([have.index(d) for d in out_dims]))
        coords = {self._time_name: np.asarray(self.ds[self._time_name].data), last: last_values}
        if member is not None:
            coords[member] = self._dim_values(member, M)
        return out_dims, coords, shaped

    def calc_hovmoller(self, flag='flag', lat_bounds=(50, 75), stat='fraction', above=0, variable=None, chunk_steps=None):
        """time-longitude (Hovmoeller) diagram of a latitude band: per time step and longitude, over the rows inside lat_bounds (None:
        every row) with flag > above,
            stat='fraction'   the blocked share of the band's area (area / the band's whole area, '1'),
            stat='area'       the blocked area in km^2, summed with the reference's area weights (contrack.py:846-848, :874),
            stat='count'      the number of blocked grid points (uint32),
            stat='any'        whether any is blocked (bool),
            stat='intensity'  the area-weighted mean of `variable` over the blocked grid points, NaN where none is.
        Returns a labelled array over (time, longitude) -- the flag variable's own dims without the latitude, a member dimension (a
        4-D flag, what run_contrack(segments=<dim>) writes) in its place; it is not added to the dataset.  The sums run on the GPU in
        rising latitude (band_numpy) and are reproducible bit for bit.  chunk_steps: the variables are read slice by slice and pass
        through chunk-sized device buffers; no slab is built on the host.  Same bits.  When `variable` is the anomaly calc_anom left
        in HBM, only the flags are uploaded."""
        stats = ('fraction', 'area', 'count', 'any', 'intensity')
        if stat not in stats:
            raise ValueError("stat must be one of {}, not {!r}".format(stats, stat))
        if stat == 'intensity' and variable is None:
            raise ValueError("stat='intensity' needs a variable")
        tables, dims, member, M, T, y01, weights, bounds, fda = self._band_tables(
            flag, lat_bounds, above, variable if stat == 'intensity' else None, chunk_steps, None, True)
        units = '1'
        if stat == 'fraction':
            out = band_fraction(tables['area'], band_total(weights, y01))
        elif stat == 'area':
            out, units = tables['area'], 'km2'
        elif stat == 'count':
            out = tables['cnt']
        elif stat == 'any':
            out = tables['cnt'] > 0
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                out = np.where(tables['cnt'] == 0, np.nan, tables['wx'] / tables['area'])
            units = getattr(self.ds[variable], 'attrs', {}).get('units')
        out_dims, coords, shaped = self._band_layout(dims, member, M, T, self._longitude_name, np.asarray(self.ds[self._longitude_name].data))
        attrs = {'long_name': 'contrack hovmoller ' + stat, 'standard_name': 'contrack hovmoller ' + stat, 'lat_bounds': bounds, 'above': int(above),
                 'history': ' '.join(['Calculated from {} with input attributes:', 'flag > {},', 'latitude band = {},', 'stat = {},', 'variable = {}.']).format(
                     flag, above, bounds, stat, variable if stat == 'intensity' else None)}
        if units is not None:
            attrs['units'] = units
        return self._wrap(fda, shaped(out), out_dims, coords, attrs, name='hovmoller')

    def calc_blocked_area(self, flag='flag', lat_bounds=None, sectors=None, above=0, variable=None, chunk_steps=None):
        """blocked area per time step of longitude sectors of a latitude band (lat_bounds; None: every row).  sectors: a dict name ->
        (west, east) in degrees east, either longitude convention, west > east a sector that wraps (lon_sector); None: one sector
        'all', the full circle.  Returns a dict of labelled arrays over (time, 'sector') -- a member dimension of a 4-D flag in its
        place --: 'area' (km^2 with the reference's area weights, contrack.py:846-848, :874), 'fraction' (area / the sector's whole
        area), 'count' (grid points, uint32) and, with `variable`, 'intensity' (its area-weighted mean over the blocked grid points,
        NaN where none is).  Nothing is added to the dataset.  The sums run on the GPU (band_numpy: rising latitude inside a column,
        the sector's columns from west to east) and are reproducible bit for bit; only the (time, sector) tables leave the device.
        chunk_steps and the resident anomaly: as calc_hovmoller."""
        self._ensure_set_up()
        lon = np.asarray(self.ds[self._longitude_name].data)
        if sectors is None:
            names, pairs = ['all'], [(0, len(lon))]
        else:
            names = list(sectors)
            if not names:
                raise ValueError("sectors is empty")
            pairs = [lon_sector(lon, *sectors[k]) for k in names]
        tables, dims, member, M, T, y01, weights, bounds, fda = self._band_tables(flag, lat_bounds, above, variable, chunk_steps, pairs, False)
        maps = [('area', tables['sec_area'], 'km2'), ('fraction', band_fraction(tables['sec_area'], band_total(weights, y01, pairs)), '1'),
                ('count', tables['sec_cnt'], '1')]
        if variable is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                inten = np.where(tables['sec_cnt'] == 0, np.nan, tables['sec_wx'] / tables['sec_area'])
            maps.append(('intensity', inten, getattr(self.ds[variable], 'attrs', {}).get('units')))
        out_dims, coords, shaped = self._band_layout(dims, member, M, T, 'sector', np.asarray(names))
        history = ' '.join(['Calculated from {} with input attributes:', 'flag > {},', 'latitude band = {},', 'sectors = {},', 'variable = {}.']).format(
            flag, above, bounds, {k: (tuple(sectors[k]) if sectors is not None else 'full circle') for k in names}, variable)
        out = {}
        for key, a, units in maps:
            attrs = {'long_name': 'contrack blocked ' + key, 'standard_name': 'contrack blocked ' + key, 'lat_bounds': bounds, 'above': int(above),
                     'history': history}
            if units is not None:
                attrs['units'] = units
            out[key] = self._wrap(fda, shaped(a), out_dims, coords, attrs, name=key)
        return out

    # ---- life cycle (contrack.py:798-906), consumer of `flag` ----------------------------
    def _time_labels(self):
        """'%Y%m%d_%H' per timestep (contrack.py:862)"""
        t = self.ds[self._time_name]
        try:
            return [str(v) for v in np.asarray(t.dt.strftime('%Y%m%d_%H').values)]
        except (AttributeError, TypeError):
            vals = np.asarray(t.data)
            if vals.dtype.kind == "M":
                import pandas as pd
                return [pd.Timestamp(v).strftime('%Y%m%d_%H') for v in vals]
            return [str(v) for v in vals]

    def run_lifecycle(self, flag, variable, chunk_steps=None, indices=False):
        """Intensity, size and centre of mass of every flagged contour at every time step.

        flag: name of the flag variable (output of run_contrack); variable: field used for intensity and centre of
        mass.  Returns a pandas DataFrame ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size'] sorted by
        (Flag, Date) -- one row per (time step, flag id).

        The per-(time step, id) sums run on the GPU (ctk_lifecycle_*, include/contrack_hip.h); the divisions,
        int() truncations, coordinate look-ups and rounding of contrack.py:876-901 are done here on the few
        resulting rows.

        A 4-D flag (extension: time, lat, lon and one member dimension in any order, what run_contrack(segments=<dim>) writes;
        `variable` must have the same dims) is taken member after member: the frame gets a seventh column, named after that
        dimension, with the member's coordinate value (its index if the dimension has no coordinate), and is sorted by (Flag,
        member, Date) -- the reference's order for ids that are unique over the members, as run_contrack's are.
        chunk_steps (extension): both variables are read slice by slice (`isel`, a chunk that spans two members in two pieces) and
        pass through chunk-sized device buffers, that many time steps at a time (0: about 256 MB of field); neither slab is built
        on the host or the device.  Flags wider than int32 are narrowed chunk by chunk; an id beyond int32 raises ValueError.
        indices=True (extension): three more int64 columns after those -- 'Step', the row's position on the time axis, and 'Row',
        'Col', the grid indices whose coordinates the truncated 'Latitude' and 'Longitude' came from: what
        calc_centred_composite takes its windows from."""
        import pandas as pd
        logger.info("\nRun Lifecycle \n########### \n    flag:    {}\n    variable:    {}".format(flag, variable))
        self._ensure_set_up()
        fda, vda = self.ds[flag], self.ds[variable]
        fdims, member = self._consumer_dims(flag)
        vdims = tuple(vda.dims)
        if sorted(vdims) != sorted(fdims):
            raise ValueError("the variable {!r} has dims {}, the flag variable {!r} has {}: they must be the same".format(variable, vdims, flag, fdims))
        if np.dtype(fda.dtype).kind not in "iub":
            raise ValueError("flag variable {!r} is not an integer field".format(flag))
        lat = np.asarray(self.ds[self._latitude_name].data)
        lon = np.asarray(self.ds[self._longitude_name].data)
        wrow = row_weights(lat, self._dlat, self._dlon)                                                 # contrack.py:847-848
        T = fda.shape[fdims.index(self._time_name)]
        period = None if member is None else T
        vtype = np.dtype(np.float64) if np.dtype(vda.dtype) == np.float64 else np.dtype(np.float32)
        fview, vview = self._steps(fda, (member, self._time_name)), self._steps(vda, (member, self._time_name))
        if chunk_steps is None:
            field = vview.slab()
            if field.dtype != np.float64:
                field = field.astype(np.float32, copy=False)
            # (the anomaly slab calc_anom left in HBM: only the flags cross PCIe)
            resident = self._resident_field(variable, field.shape, field.dtype == np.float64)
            cols = lifecycle_numpy(fview.slab(), None if resident else field, wrow, lat, lon, self._time_labels(), dtype=field.dtype, period=period,
                                   indices=indices)
        else:
            # (a variable of any other type than float64 becomes float32 in the copy into the chunk buffer, as in the resident call)
            cols = lifecycle_numpy(fview.reader(integer=True), vview.reader(), wrow, lat, lon, self._time_labels(), chunk_steps=chunk_steps,
                                   shape=fview.shape, dtype=vtype, period=period, indices=indices)
        columns = ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']
        if member is not None:
            cols[member] = self._dim_values(member, fda.shape[fdims.index(member)])[cols.pop("Member")]
            columns.append(member)
        if indices:
            columns += ['Step', 'Row', 'Col']
        return pd.DataFrame(cols, columns=columns)

    def _frame_steps(self, frame, da, dims, member):
        """the flat step m * T + t of every row of a life-cycle frame on the flag variable `da` (select_blocks, calc_block_stats): its
        'Step' and, for a 4-D flag, the position of its member column's value on that dimension"""
        T = da.shape[dims.index(self._time_name)]
        need = ['Flag', 'Step'] + ([member] if member is not None else [])
        missing = [c for c in need if c not in frame]
        if missing:
            raise ValueError("the frame lacks the columns {}: pass rows of run_lifecycle(..., indices=True)".format(missing))
        step = np.asarray(frame['Step']).astype(np.int64)
        if step.size and (step.min() < 0 or step.max() >= T):
            raise ValueError("the frame's Step must lie in [0, {})".format(T))
        if member is not None:
            values = self._dim_values(member, da.shape[dims.index(member)])
            order = np.argsort(values, kind='stable')
            col = np.asarray(frame[member])
            pos = np.minimum(np.searchsorted(values[order], col), len(values) - 1)
            if (values[order][pos] != col).any():
                raise ValueError("the frame's column {!r} holds values that are not on that dimension".format(member))
            step = order[pos].astype(np.int64) * T + step
        return step

    # ---- selection: the flag of chosen tracks or (step, track) rows, what the consumers of `flag` then take ----------------------
    def select_blocks(self, flag='flag', ids=None, frame=None, invert=False, out='id', name='flag_sel', chunk_steps=None, check=True):
        """adds the variable `name`: the flag variable restricted to the blocks a study picked, computed on the GPU (subset_numpy).
        Exactly one of
          ids:   the tracks to keep, at every step (the Atlantic blocks, those of ten days or more: track_table helps to pick them);
          frame: rows of run_lifecycle(indices=True) -- 'Flag', 'Step' and, for a 4-D flag, the member column --, every row one
                 (step, track) to keep (only the mature days, only the days the centre lies in a sector).
        Pixels of the kept blocks keep their id (out='mask': become 1), all others become 0; invert=True keeps every block pixel
        that was NOT asked for instead.  `name` has the flag's dims (any order, a member dimension included) and is int32:
        calc_frequency, calc_spells, calc_composite, calc_hovmoller and calc_blocked_area take it as they take `flag`.
        chunk_steps: the flag is read slice by slice (`isel`), as calc_frequency does; same values.
        check=True: an id or row that matches no pixel raises ValueError (the frame comes from another run) and nothing is added.
        Returns the number of selected pixels."""
        self._ensure_set_up()
        if (ids is None) == (frame is None):
            raise ValueError("select_blocks takes exactly one of ids and frame")
        if out not in _native.SUBSET_KINDS:
            raise ValueError("out={!r}: 'id' or 'mask'".format(out))
        da = self.ds[flag]
        dims, member = self._consumer_dims(flag)
        if np.dtype(da.dtype).kind not in "iub":
            raise ValueError("flag must be an integer field")
        T = da.shape[dims.index(self._time_name)]
        view = self._steps(da, (member, self._time_name))
        if ids is not None:
            table = subset_table(ids)
            asked = '{} ids'.format(len(table[1]))
        else:
            table = subset_table(np.asarray(frame['Flag']), self._frame_steps(frame, da, dims, member), view.steps)
            asked = '{} rows'.format(len(table[1]))
        source = view.slab() if chunk_steps is None else view.reader(integer=True)
        res, n, hits = subset_numpy(source, table, invert=invert, kind=out, chunk_steps=chunk_steps, shape=view.shape, return_hits=True)
        if check and (hits == 0).any():
            lost = np.flatnonzero(hits == 0)
            at = np.searchsorted(table[0], lost, side='right') - 1                # the flat step of a row table's entry
            some = ', '.join(str(int(table[1][e])) if ids is not None else '(step {}, id {})'.format(int(s), int(table[1][e])) for e, s in zip(lost[:5], at[:5]))
            raise ValueError("{} of the {} requested match no pixel of {!r} (the first: {}): do they come from another run?".format(len(lost), asked, flag, some))
        attrs = {'units': '1', 'long_name': 'contrack selected {}'.format('mask' if out == 'mask' else 'flag'),
                 'history': 'Selected from {} with input attributes: {}, invert = {}, out = {}.'.format(flag, asked, bool(invert), out)}
        self.ds[name] = (dims, view.restore(res, dims), attrs)
        return n

    # ---- per-block peak and extent: what the literature selects rows of the life-cycle frame on ---------------------------------
    def calc_block_stats(self, flag='flag', variable=None, frame=None, chunk_steps=None, indices=False, check=True):
        """one row per row of `frame`, in the frame's order, with the two properties of a block at a time step that run_lifecycle
        does not give: its extent and, with `variable`, its true peak and where it sits (blockstat_numpy, on the GPU).
        frame: rows of run_lifecycle(indices=True) or any selection of them -- 'Flag', 'Step' and, for a 4-D flag, the member
        column --; None: run_lifecycle(flag, variable, indices=True) is called first (and needs `variable`).  Returns a pandas
        DataFrame: the frame's key columns ('Flag', 'Date' where the frame has it, the member column, 'Step'), then
          N                          the pixels of the block at that step
          South, North, LatExtent    the coordinate values of its lowest and highest grid row (r0, r1: South is the row with the
                                     lower index, whichever way the latitudes run) and (r1 - r0 + 1) * dlat
          West, East, LonExtent      lon[west], lon[(west + width - 1) % nx] and width * dlon, taken AROUND the date line: the
                                     complement of the longest circular run of columns the block does not touch
        and with `variable`
          Max, MaxLatitude, MaxLongitude, Min, MinLatitude, MinLongitude
                                     the largest and smallest value of the variable inside the block (NaN values apart) and the
                                     actual coordinates, not truncated, of the first pixel in row-major order that holds each.
        The usual "block intensity" is Max (Min for gorl='<'); run_lifecycle's Intensity is the area mean and lies between them.
        indices=True adds the integer columns 'Row0', 'Row1', 'ColWest', 'Width' and, with `variable`, 'NValid', 'MaxRow', 'MaxCol',
        'MinRow', 'MinCol'.  When `variable` is the anomaly calc_anom left in HBM nothing but the flags travels.  chunk_steps: both
        variables are read slice by slice (`isel`) through chunk-sized device buffers; same values.  Dims in any order, a member
        dimension included.  check=True: a row that matches no pixel raises ValueError (the frame comes from another run)."""
        import pandas as pd
        self._ensure_set_up()
        fda = self.ds[flag]
        dims, member = self._consumer_dims(flag)
        if np.dtype(fda.dtype).kind not in "iub":
            raise ValueError("flag variable {!r} is not an integer field".format(flag))
        if frame is None:
            if variable is None:
                raise ValueError("calc_block_stats without a frame calls run_lifecycle, which needs `variable`")
            frame = self.run_lifecycle(flag, variable, chunk_steps=chunk_steps, indices=True)
        fview = self._steps(fda, (member, self._time_name))
        step = self._frame_steps(frame, fda, dims, member)
        ids = _positive_int32(np.asarray(frame['Flag']), "the frame's Flag")
        table = subset_table(ids, step, fview.steps)
        want = ('shape',) if variable is None else ('shape', 'peaks')
        if variable is None:
            field, vtype = None, None
        else:
            vda = self.ds[variable]
            vdims = tuple(vda.dims)
            if sorted(vdims) != sorted(dims) or any(vda.shape[vdims.index(d)] != fda.shape[dims.index(d)] for d in dims):
                raise ValueError("the variable {!r} has dims {}, the flag variable {!r} has {}: they must be the same".format(variable, vdims, flag, dims))
            vtype = _native._field_dtype(vda.dtype)
            vview = self._steps(vda, (member, self._time_name))
        if chunk_steps is None:
            if variable is not None:
                field = vview.slab().astype(vtype, copy=False)
                if self._resident_field(variable, field.shape, vtype == np.float64):
                    field = None                                                    # (only the flags cross PCIe)
            rows = blockstat_numpy(fview.slab(), table, field, want=want, dtype=vtype)
        else:
            rows = blockstat_numpy(fview.reader(integer=True), table, None if variable is None else vview.reader(), want=want, chunk_steps=chunk_steps,
                                   shape=fview.shape, dtype=vtype)
        # the entry of every frame row: the table is the sorted set of (flat step, id) pairs
        pairs = np.repeat(np.arange(fview.steps, dtype=np.int64), np.diff(table[0])) * (1 << 31) + table[1]
        rows = rows[np.searchsorted(pairs, step * (1 << 31) + ids)]
        if check and (rows['n'] == 0).any():
            lost = np.flatnonzero(rows['n'] == 0)
            some = ', '.join('(step {}, id {})'.format(int(step[i]), int(ids[i])) for i in lost[:5])
            raise ValueError("{} of the {} rows requested match no pixel of {!r} (the first: {}): do they come from another run?".format(
                len(lost), len(rows), flag, some))
        lat = np.asarray(self.ds[self._latitude_name].data)
        lon = np.asarray(self.ds[self._longitude_name].data)
        nx = len(lon)

        def at(coord, idx, live):
            """coord[idx] as float64 where `live`, NaN elsewhere (an entry that matched nothing, or without a valid value)"""
            return np.where(live, np.asarray(coord, dtype=np.float64)[np.where(live, idx, 0)], np.nan)
        hit = rows['n'] > 0
        dlat, dlon = (abs(float(np.atleast_1d(d)[0])) for d in (self._dlat, self._dlon))
        r0, r1, west, width = (rows[k].astype(np.int64) for k in ('r0', 'r1', 'west', 'width'))
        cols = {k: np.asarray(frame[k]) for k in ['Flag', 'Date', member, 'Step'] if k is not None and k in frame}
        cols['N'] = rows['n'].astype(np.int64)
        cols['South'], cols['North'] = at(lat, r0, hit), at(lat, r1, hit)
        cols['LatExtent'] = np.where(hit, r1 - r0 + 1, 0) * dlat
        cols['West'], cols['East'] = at(lon, west, hit), at(lon, (west + width - 1) % nx, hit)
        cols['LonExtent'] = width * dlon
        if variable is not None:
            ok = rows['nv'] > 0
            for name in ('max', 'min'):
                p = rows[name + '_p']
                cols[name.capitalize()] = rows[name].copy()
                cols[name.capitalize() + 'Latitude'], cols[name.capitalize() + 'Longitude'] = at(lat, p // nx, ok), at(lon, p % nx, ok)
        if indices:
            cols['Row0'], cols['Row1'], cols['ColWest'], cols['Width'] = r0, r1, west, width
            if variable is not None:
                cols['NValid'] = rows['nv'].astype(np.int64)
                for name in ('max', 'min'):
                    p = rows[name + '_p']
                    cols[name.capitalize() + 'Row'], cols[name.capitalize() + 'Col'] = np.where(p >= 0, p // nx, -1), np.where(p >= 0, p % nx, -1)
        return pd.DataFrame(cols, columns=list(cols))

    def calc_centred_composite(self, variable, frame, half_width=(20., 40.), by=None, nbins=None, max_age=None, stat='mean', skipna=False, wrap=True,
                               chunk_steps=None, return_count=False):
        """mean (stat='mean') or sum (stat='sum') of `variable` in a window that moves with the blocks' centres, per bin of the life
        cycle: the composite in the block's own frame of reference.  frame: run_lifecycle's DataFrame or any row selection of it (a
        sector, a season, the long-lived blocks); every row is one stamp, the window of +-half_width = (degrees latitude, degrees
        longitude) around its centre at its time step (hy = round(degrees / grid spacing) grid points).  With the columns 'Step',
        'Row', 'Col' of run_lifecycle(indices=True) the centres are taken as they are; without them 'Date' is looked up among the
        time labels (which must be unique) and 'Latitude' / 'Longitude' go to the nearest grid index -- the reference's int()
        truncation of those two makes that up to one degree off the centre that was computed.
        by: None (one bin); 'age' (time steps since the block's first row), 'to_lysis' (time steps before its last), 'normalized'
        (nbins equal parts of its life cycle) as lifecycle_bins computes them among the rows GIVEN, with nbins / max_age; the name
        of an integer column of the frame; or an integer array, one bin per row (negative: the row is dropped).
        A row outside the grid's latitudes is not counted (no step over a pole); wrap=True, the default, treats longitude as
        periodic, as run_contrack does.  skipna: a NaN value is not counted; without it one makes its cell NaN.  The sums are
        float64 and added in a fixed order on the GPU (centred_numpy: time order, rows of one time step in the frame's order), so
        the result is reproducible bit for bit; a cell no window reached gives NaN (mean) or 0 (sum).
        Returns a labelled float64 array, not added to the dataset, with dims (by if it is a string else 'bin', 'rel_' + latitude
        name, 'rel_' + longitude name), the offsets in degrees as coordinates, the variable's units; return_count=True: (composite,
        n), n the uint32 count per cell.
        A 4-D variable (a member dimension) needs the frame's member column; the members are taken one after the other.
        chunk_steps: the variable is read slice by slice (`isel`) and passes through chunk-sized device buffers; chunks without
        stamps are not read.  Same bits.  When `variable` is the anomaly calc_anom left in HBM, no field bytes are uploaded."""
        self._ensure_set_up()
        if stat not in ('mean', 'sum'):
            raise ValueError("stat must be 'mean' or 'sum', not {!r}".format(stat))
        vda = self.ds[variable]
        dims, member = self._consumer_dims(variable, what="variable")
        T = vda.shape[dims.index(self._time_name)]
        lat = np.asarray(self.ds[self._latitude_name].data)
        lon = np.asarray(self.ds[self._longitude_name].data)
        have = list(frame.columns)
        column = lambda name: np.asarray(frame[name])                              # noqa: E731
        if all(c in have for c in ('Step', 'Row', 'Col')):
            step, row, col = (column(c).astype(np.int64) for c in ('Step', 'Row', 'Col'))
        else:
            labels = self._time_labels()
            where = {d: i for i, d in enumerate(labels)}
            if len(where) != len(labels):
                raise ValueError("the time labels are not unique: the frame's 'Date' does not name a time step (use run_lifecycle(indices=True))")
            try:
                step = np.array([where[str(d)] for d in column('Date')], dtype=np.int64)
            except KeyError as e:
                raise ValueError("the frame's Date {} is not a time label of the dataset".format(e))
            row = np.abs(lat[None, :].astype(np.float64) - column('Latitude').astype(np.float64)[:, None]).argmin(axis=1).astype(np.int64)
            col = np.abs(lon[None, :].astype(np.float64) - column('Longitude').astype(np.float64)[:, None]).argmin(axis=1).astype(np.int64)
        t = step
        block = column('Flag') if 'Flag' in have else np.zeros(len(step), dtype=np.int64)
        if member is not None:
            if member not in have:
                raise ValueError("the variable {!r} has the member dimension {!r}: the frame needs that column".format(variable, member))
            M = vda.shape[dims.index(member)]
            index = {v: m for m, v in enumerate(self._dim_values(member, M).tolist())}
            try:
                m_of = np.array([index[v] for v in column(member).tolist()], dtype=np.int64)
            except KeyError as e:
                raise ValueError("the frame's {} {} is not a value of that dimension".format(member, e))
            t = m_of * T + step                                                    # the flattening the other consumers use
            block = list(zip(block.tolist(), m_of.tolist()))
        if isinstance(by, str) and by not in ('age', 'to_lysis', 'normalized'):
            if by not in have:
                raise ValueError("by = {!r} is neither 'age', 'to_lysis', 'normalized' nor a column of the frame".format(by))
            bins, nb = lifecycle_bins(block, step, column(by), nbins=nbins)
        else:
            bins, nb = lifecycle_bins(block, step, by, nbins=nbins, max_age=max_age)
        dlat, dlon = (float(np.atleast_1d(d)[0]) for d in (self._dlat, self._dlon))
        half = (int(round(float(half_width[0]) / dlat)), int(round(float(half_width[1]) / dlon)))
        vtype = _native._field_dtype(vda.dtype)
        view = self._steps(vda, (member, self._time_name))
        if chunk_steps is None:
            field = view.slab().astype(vtype, copy=False)
            resident = self._resident_field(variable, field.shape, vtype == np.float64)
            s, n = centred_numpy(None if resident else field, t, row, col, bins, nb, half, wrap=wrap, skipna=skipna, shape=field.shape, dtype=vtype)
        else:
            s, n = centred_numpy(view.reader(), t, row, col, bins, nb, half, wrap=wrap, skipna=skipna, chunk_steps=chunk_steps, shape=view.shape, dtype=vtype)
        out = composite_mean(s, n) if stat == 'mean' else s
        bdim = by if isinstance(by, str) else 'bin'
        out_dims = (bdim, 'rel_' + self._latitude_name, 'rel_' + self._longitude_name)
        step_lat = float(lat[1] - lat[0]) if len(lat) > 1 else dlat
        step_lon = float(lon[1] - lon[0]) if len(lon) > 1 else dlon
        coords = {bdim: np.arange(nb), out_dims[1]: np.arange(-half[0], half[0] + 1) * step_lat, out_dims[2]: np.arange(-half[1], half[1] + 1) * step_lon}
        attrs = {'long_name': 'contrack centred composite', 'standard_name': 'contrack centred composite',
                 'history': ' '.join(['Calculated from {} with input attributes:', 'stamps = {} of {} rows,', 'half_width = {},', 'by = {},', 'stat = {},',
                                      'skipna = {},', 'wrap = {}.']).format(
                     variable, int(np.count_nonzero(bins >= 0)), len(bins), tuple(half_width), by if by is None or isinstance(by, str) else 'bins given', stat,
                     skipna, wrap)}
        units = getattr(vda, 'attrs', {}).get('units')
        if units is not None:
            attrs['units'] = units
        res = self._wrap(vda, out, out_dims, coords, attrs, name='centred_composite')
        if not return_count:
            return res
        cattrs = {'long_name': 'contrack centred composite count', 'units': '1', 'history': attrs['history']}
        return res, self._wrap(vda, n, out_dims, coords, cattrs, name='count')

    # ---- utility (contrack.py:912-949) ---------------------------------------------------------------------------
    def greatcircle_dist(self, lon1, lat1, lon2, lat2):
        """great-circle distance in km between (lon1, lat1) and (lon2, lat2) given in degrees"""
        a1, a2 = np.deg2rad(lat1), np.deg2rad(lat2)
        c = np.sin(a1) * np.sin(a2) + np.cos(a1) * np.cos(a2) * np.cos(np.deg2rad(lon1 - lon2))
        return 6371. * np.arccos(min(1., max(-1., c)))
