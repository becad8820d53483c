"""contrack_amd -- MI355X (gfx950) implementation of ConTrack's run_contrack hot path.

`contrack` is the drop-in class (same constructor / set_up / calc_anom / run_contrack signatures and the
same 'flag' output variable as steidani/ConTrack's contrack.contrack); `track_numpy` is the array-level
entry underneath it, `frequency_numpy` the blocking frequency (README.rst:159-160 of the reference) of its `flag`,
`spells_numpy` / `spell_duration` the blocked spells per grid point (events, their durations, the longest one),
`composite_numpy` / `composite_mean` the mean of a field over the flagged time steps,
`centred_numpy` / `lifecycle_bins` the composite of a field in a window that moves with the blocks' centres, per life-cycle age,
`band_numpy` / `lon_sector` / `band_fraction` the blocked area per time step and longitude of a latitude band and of longitude sectors,
`subset_numpy` / `subset_table` the flag restricted to chosen tracks or (step, track) rows, `track_table` the per-track table to choose from,
`blockstat_numpy` the true peak of a field inside every (step, track) row's block, where it sits, and the block's extent around the date line,
`anomalies_numpy` the climatology and anomalies that produce its input (over time segments, optionally streamed),
`percentile_field_numpy` the per-grid-point percentile threshold field per group of timesteps,
`std_field_numpy` the per-grid-point standard-deviation threshold field per group of timesteps,
`level_mean_numpy` the vertical mean over a pressure band that comes before them (weights: `level_weights`),
`reversal_numpy` / `reversal_rows` / `reversal_limits` the gradient-reversal blocking index, the other producer of a field to track,
`lwa_numpy` / `lwa_rows` the finite-amplitude local wave activity, the third one,
`time_filter_numpy` / `filter_layout` / `lanczos_weights` a weighted filter or block means along time of a field on its way there.
Compute goes through hand-written HIP kernels behind a ctypes C ABI
(include/contrack_hip.h); there is no CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name in ("contrack", "track_numpy", "frequency_numpy", "spells_numpy", "spell_duration", "composite_numpy", "composite_mean", "centred_numpy", "centred_stamps", "lifecycle_bins", "band_numpy", "band_total", "band_fraction", "lon_sector", "subset_numpy", "subset_table", "track_table", "blockstat_numpy", "anomalies_numpy", "percentile_field_numpy", "std_field_numpy", "level_mean_numpy", "level_weights", "reversal_numpy", "reversal_rows", "reversal_limits", "lwa_numpy", "lwa_rows", "time_filter_numpy", "filter_layout", "lanczos_weights", "row_weights", "prepare_thresholds"):
        import importlib
        _m = importlib.import_module(".contrack", __name__)     # (`from . import contrack` would ask __getattr__ for 'contrack' first)
        return getattr(_m, name)
    raise AttributeError(name)
