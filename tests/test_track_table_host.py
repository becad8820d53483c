"""track_table: the per-track table of a life-cycle frame, on hand-made frames.  Host only."""
import numpy as np
import pytest

pd = pytest.importorskip("pandas")

from contrack_amd.contrack import contrack, track_table            # noqa: E402

COLUMNS = ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']


def km(lon1, lat1, lon2, lat2):
    return float(contrack.greatcircle_dist(None, lon1, lat1, lon2, lat2))


def frame():
    rows = [
        # track 3 crosses the seam: 350E -> 358E -> 6E, two steps of 8 degrees along 60N
        (3, '20200101_00', 350, 60, 100.0, 4.0e6),
        (3, '20200101_06', 358, 60, 140.0, 6.0e6),
        (3, '20200101_12', 6, 60, 120.0, 5.0e6),
        # track 7 has one row
        (7, '20200105_00', 10, 45, 90.5, 1.5e6),
        # track 9 moves along a meridian and back
        (9, '20200110_00', 20, 50, 10.0, 1.0),
        (9, '20200110_06', 20, 55, 30.0, 3.0),
        (9, '20200110_12', 20, 50, 20.0, 2.0),
    ]
    return pd.DataFrame(rows, columns=COLUMNS)


def test_one_row_per_track():
    tt = track_table(frame())
    assert list(tt.columns) == ['Flag', 'Onset', 'Decay', 'Duration', 'OnsetLongitude', 'OnsetLatitude', 'DecayLongitude', 'DecayLatitude', 'MaxIntensity',
                                'MeanIntensity', 'MaxSize', 'MeanSize', 'PathLength', 'Displacement']
    assert tt['Flag'].tolist() == [3, 7, 9] and tt['Duration'].tolist() == [3, 1, 3]
    a, b, c = (tt.iloc[i] for i in range(3))
    assert (a['Onset'], a['Decay']) == ('20200101_00', '20200101_12')
    assert (a['OnsetLongitude'], a['OnsetLatitude'], a['DecayLongitude'], a['DecayLatitude']) == (350, 60, 6, 60)
    assert a['MaxIntensity'] == 140.0 and a['MeanIntensity'] == 120.0 and a['MaxSize'] == 6.0e6 and a['MeanSize'] == 5.0e6
    # across the seam the centres are 8 degrees apart, not 352: two steps of the same length, and 16 degrees from onset to decay
    step = km(350, 60, 358, 60)
    assert step == pytest.approx(km(358, 60, 6, 60), rel=1e-12) and 400 < step < 450
    assert a['PathLength'] == pytest.approx(2 * step, rel=1e-12)
    assert a['Displacement'] == pytest.approx(km(350, 60, 6, 60), rel=1e-12) and a['Displacement'] < a['PathLength']
    # one row: onset is decay, nothing travelled
    assert (b['Onset'], b['Decay'], b['Duration']) == ('20200105_00', '20200105_00', 1)
    assert b['PathLength'] == 0.0 and b['Displacement'] == 0.0 and b['MaxIntensity'] == b['MeanIntensity'] == 90.5
    # there and back: a path of twice five degrees of latitude, no displacement
    assert c['PathLength'] == pytest.approx(2 * 6371. * np.deg2rad(5.), rel=1e-9) and c['Displacement'] == pytest.approx(0.0, abs=1e-3)
    assert c['MeanIntensity'] == 20.0 and c['MeanSize'] == 2.0


def test_member_column_and_index_columns():
    f = frame()
    f['ens'] = ['a', 'a', 'b', 'a', 'b', 'b', 'b']
    f['Step'], f['Row'], f['Col'] = np.arange(7), 0, 0
    tt = track_table(f)
    assert list(tt.columns[:2]) == ['Flag', 'ens'] and 'Step' not in tt.columns
    assert list(zip(tt['Flag'], tt['ens'])) == [(3, 'a'), (3, 'b'), (7, 'a'), (9, 'b')]
    assert tt['Duration'].tolist() == [2, 1, 1, 3]
    assert tt['PathLength'].iloc[0] == pytest.approx(km(350, 60, 358, 60), rel=1e-12) and tt['PathLength'].iloc[1] == 0.0
    assert (tt['Onset'].iloc[1], tt['OnsetLongitude'].iloc[1]) == ('20200101_12', 6)


def test_a_row_selection_and_bad_frames():
    f = frame()
    tt = track_table(f[f['Intensity'] >= 100.0])
    assert tt['Flag'].tolist() == [3] and tt['Duration'].tolist() == [3]
    assert len(track_table(f.iloc[:0])) == 0
    with pytest.raises(ValueError):
        track_table(f.drop(columns=['Size']))
    f['a'], f['b'] = 1, 2
    with pytest.raises(ValueError):
        track_table(f)
