"""The blocking-frequency entries without a GPU: declared in include/contrack_hip.h, exported by the library build() cross-compiles,
bound in _native.EXPORTS; the pure parts of the Python side (season mapping and order, percent, argument checks)."""
import os
import re

import numpy as np
import pytest

import freq_util
import minixr
from contrack_amd import _native
from contrack_amd.contrack import contrack, frequency_percent, season_of_month

ENTRIES = ("ctk_frequency_dev", "ctk_frequency", "ctk_frequency_cb")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "contrack_hip.h")


def test_entries_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(ctk_\w+)\s*\(", text, flags=re.M))
    lib = _native.lib()
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native.EXPORTS, name
    assert hasattr(lib, "ctk_debug_set_freq") and "ctk_debug_set_freq" in _native.EXPORTS


def test_season_mapping_and_order():
    months = np.arange(1, 13)
    assert list(season_of_month(months)) == ['DJF', 'DJF', 'MAM', 'MAM', 'MAM', 'JJA', 'JJA', 'JJA', 'SON', 'SON', 'SON', 'DJF']
    assert list(np.unique(season_of_month(months))) == ['DJF', 'JJA', 'MAM', 'SON']        # xarray's groupby('time.season') order
    with pytest.raises(ValueError):
        season_of_month([0, 13])


def test_group_ids_season_without_dt_season():
    """minixr's .dt has no season (nor month): the pandas fallback maps the months"""
    T = 400
    time = (np.datetime64("2000-11-15") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(np.zeros((T, 3, 4), np.float32), np.array([10.0, 11.0, 12.0]), np.arange(4.0), time=time)
    c = contrack(ds=ds)
    c.set_up()
    ids, uniq = c._group_ids('season')
    assert list(uniq) == ['DJF', 'JJA', 'MAM', 'SON']
    month = (time.astype("datetime64[M]").astype(np.int64) % 12) + 1
    assert np.array_equal(uniq[ids], season_of_month(month))
    ids_m, uniq_m = c._group_ids('month')
    assert list(uniq_m) == list(range(1, 13)) and np.array_equal(uniq_m[ids_m], month)


def test_percent_is_the_numpy_expression_bit_for_bit():
    rng = np.random.default_rng(3)
    T = 731
    flag = (rng.random((T, 7, 9)) < 0.07).astype(np.int32) * rng.integers(1, 50, (T, 7, 9), dtype=np.int32)
    for name, ids, G in freq_util.groupings(T):
        for above in (-1, 0, 1, 50):
            c = freq_util.counts(flag, ids, G, above)
            n = [T] if ids is None else np.bincount(ids, minlength=G)
            got = frequency_percent(c, n)
            want = freq_util.percent(flag, ids, G, above)
            assert freq_util.same_bits(got[0] if ids is None else got, want), (name, above)
    assert np.isnan(frequency_percent(np.zeros((2, 3)), [0, 4])[0]).all()


def test_group_argument_checks():
    with pytest.raises(ValueError):
        _native._groups(np.zeros(5, np.int32), 6)                       # one id per timestep
    with pytest.raises(ValueError):
        _native._groups(np.zeros(5, np.float64), 5)
    with pytest.raises(ValueError):
        _native._groups(np.array([0, 2 ** 32], np.int64), 2)            # would wrap to 0 as int32
    g, G = _native._groups(np.array([0, 3, 1]), 3)
    assert g.dtype == np.int32 and G == 4
    assert _native._groups(None, 9) == (None, 1)
    with pytest.raises(ValueError):
        _native._above(2 ** 31)
