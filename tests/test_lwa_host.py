"""The numpy statement of the local wave activity (tests/lwa_util.py), contrack.lwa_rows and ctk_lwa_plan, without a GPU: what the
definition gives on fields whose answer is known, that the vectorised statement is the per-pixel loop, that the row table follows its
formulas on every kind of latitude axis, that the library's plan is the restated one at its form and capacity edges, and that every
case of tests/test_gpu_lwa_edges.py reaches the edge it is named for (lu.bisection: the kernel's search restated in integers)."""
import math

import numpy as np
import pytest

import lwa_util as lu
from contrack_amd import _native
from contrack_amd.contrack import lwa_rows


def same_table(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype for k in ("dom_off", "dom_rows", "active", "W", "q", "S")) \
        and int(a["ndom"]) == int(b["ndom"])


# ---- the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_zonally_symmetric_monotone_field_has_no_wave_activity(dtype):
    lat = lu.grid(2.5)
    prof = (5700.0 - 800.0 * np.sin(np.deg2rad(lat)) ** 2).astype(dtype)
    z = np.repeat(np.repeat(prof[None, :, None], 12, axis=2), 2, axis=0)
    tab = lu.rows(lat)
    for part in (0, 1, 2):
        out, ref = lu.from_table(z, tab, part, return_ref=True)
        assert not out.any() and not np.signbit(out).any()
        act = tab["active"] != 0
        assert np.array_equal(ref[:, act], z[:, act, 0]) and not ref[:, ~act].any()          # the contour of a row is the row's value


def test_a_ridge_gives_activity_under_it_and_the_parts_add_up():
    lat = lu.grid(2.5)
    nx = 144
    lam = 2.5 * np.arange(nx)
    z = 5700.0 - 800.0 * np.sin(np.deg2rad(lat))[None, :, None] ** 2 + 250.0 * np.exp(-((lat[None, :, None] - 60.0) / 10.0) ** 2 - ((lam[None, None, :] - 180.0) / 20.0) ** 2)
    for dtype in (np.float32, np.float64):
        zz = z.astype(dtype)
        tab = lu.rows(lat)
        tot, a, y = (lu.from_table(zz, tab, part) for part in (0, 1, 2))
        j55 = int(np.flatnonzero(lat == 55.0)[0])
        assert tot[0, j55, 72] > 1e8 and tot[0, j55, 72] > 100 * tot[0, j55, 0] >= 0          # m^2: under the ridge, far from it
        assert a[0, j55, 72] > 0 and np.all(tot >= 0) and np.all(a >= 0) and np.all(y >= 0)
        assert not tot[0, lat < 0].any()                                                       # a symmetric southern hemisphere
        # total before rounding = a + y in float64: recomputed pixel by pixel
        dom = lu.domains(tab)[0]
        Z = lu.contours(zz[0], tab, dom)[0]
        for c in (0, 60, 72, 80):
            p = dom.index(j55)
            pa, py = lu.pixel(zz[0], tab, dom, p, c, Z[p])
            S = tab["S"][j55]
            assert dtype((pa + py) * S) == tot[0, j55, c] and dtype(pa * S) == a[0, j55, c] and dtype(py * S) == y[0, j55, c]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_vectorised_statement_is_the_per_pixel_loop(dtype):
    lat = lu.grid(7.5)
    tab = lu.rows(lat)
    z = lu.field(lat, 5, steps=2, seed=3, dtype=dtype)
    z = lu.sprinkle(z, tab, [np.nan, np.inf, -np.inf, 0.0, -0.0], share=0.03, seed=1)
    outs = [lu.from_table(z, tab, part) for part in (0, 1, 2)]
    for s in range(2):
        for dom in lu.domains(tab):
            Z = lu.contours(z[s], tab, dom)[0]
            for p, j in enumerate(dom):
                if not tab["active"][j]:
                    continue
                for c in range(5):
                    a, y = lu.pixel(z[s], tab, dom, p, c, Z[p])
                    with np.errstate(invalid="ignore", over="ignore"):
                        want = [np.array(dtype(v * tab["S"][j])) if not np.isnan(Z[p]) else np.array(dtype(np.nan)) for v in (a + y, a, y)]
                    assert all(lu.same_bits(w, np.array(o[s, j, c])) for w, o in zip(want, outs)), (s, j, c)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_southern_mirror_gives_the_mirrored_bits(dtype):
    lat = lu.grid(5.0)
    assert np.array_equal(lat[::-1], -lat)
    z = lu.field(lat, 9, steps=3, seed=2, dtype=dtype)
    for part in (0, 1, 2):
        north, rn = lu.lwa(z, lat, hemisphere='north', part=part, return_ref=True)
        south, rs = lu.lwa(z[:, ::-1].copy(), lat, hemisphere='south', part=part, return_ref=True)
        assert lu.nonzero_share(north, lu.rows(lat, hemisphere='north')) > (0.5 if part == 0 else 0.2)
        assert lu.same_bits(south[:, ::-1], north) and lu.same_bits(rs[:, ::-1], rn)
        both = lu.lwa(z, lat, part=part)
        assert lu.same_bits(both[:, lat > 0], north[:, lat > 0])                               # the hemispheres do not see each other


# ---- the row table ----------------------------------------------------------------------------------------------------------------
def test_the_row_table_of_a_regular_grid_follows_the_formulas():
    lat = lu.grid(2.5)
    tab = lwa_rows(lat)
    assert same_table(tab, lu.rows(lat))
    assert tab["ndom"] == 2 and tab["dom_off"].tolist() == [0, 37, 74]
    assert tab["dom_rows"][:37].tolist() == list(range(36, -1, -1)) and tab["dom_rows"][37:].tolist() == list(range(36, 73))       # the equator row in both
    assert tab["W"].dtype == np.uint32 and tab["W"][0] == 0 and tab["W"][72] == 0 and tab["W"][36] == 2 ** 30                    # the poles, the equator
    d = math.radians(2.5)
    for j in range(73):
        c = max(math.cos(math.radians(lat[j])), 0.0)
        assert abs(int(tab["W"][j]) - c * 2 ** 30) <= 0.5 + 1e-6
        width = d / 2 if j in (0, 36, 72) else d
        assert tab["q"][j] == pytest.approx(c * width, rel=1e-14, abs=1e-30)
        act = 30 <= abs(lat[j]) <= 75
        assert tab["active"][j] == act
        assert tab["S"][j] == (pytest.approx(6.371e6 / math.cos(math.radians(lat[j])), rel=1e-14) if act else 0)
    assert np.all(np.isfinite(tab["q"])) and np.all(tab["q"] >= 0)
    for dom in lu.domains(tab):
        caps = lu.caps(tab, dom, 144)
        assert all(caps[p] > caps[p + 1] for p in range(len(dom) - 2)) and caps[-1] == 0 and caps[-2] > 0                       # strictly towards the pole; the pole row has no area
    assert lwa_rows(lat, radius=1.0)["S"][20] == pytest.approx(1.0 / math.cos(math.radians(40.0)), rel=1e-14)


@pytest.mark.parametrize("hemisphere", ["both", "north", "south"])
def test_rising_falling_and_shuffled_axes_give_the_same_domains(hemisphere):
    for base in (lu.grid(5.0), lu.gaussian(), np.array([80.0, 61.5, 47.0, 33.0, 12.0, 0.0, -20.0, -41.0, -58.5, -77.0])):
        want = None
        for lat in (base, base[::-1].copy(), lu.shuffled(base, 4)):
            tab = lwa_rows(lat, hemisphere=hemisphere)
            assert same_table(tab, lu.rows(lat, hemisphere=hemisphere))
            doms = [[float(lat[j]) for j in dom] for dom in lu.domains(tab)]
            assert len(doms) == (2 if hemisphere == 'both' else 1)
            for dom in doms:
                assert all(abs(dom[i]) <= abs(dom[i + 1]) for i in range(len(dom) - 1))
                assert all(v >= 0 for v in dom) or all(v <= 0 for v in dom)
            by_lat = (doms, sorted((float(lat[j]), int(tab["W"][j]), float(tab["q"][j]), float(tab["S"][j]), int(tab["active"][j])) for j in range(len(lat))))
            if want is None:
                want = by_lat
            assert by_lat == want                                                # the same latitudes, weights and widths whatever the order of the axis
        if 0.0 in base:
            assert sum(dom.count(0.0) for dom in doms) == (2 if hemisphere == 'both' else 1)


def test_row_table_arguments():
    lat = lu.grid(5.0)
    for bad in ((0, 75), (-10, 75), (80, 30), (np.nan, 75)):
        with pytest.raises(ValueError, match="lat_bounds"):
            lwa_rows(lat, lat_bounds=bad)
    with pytest.raises(ValueError, match="hemisphere"):
        lwa_rows(lat, hemisphere='east')
    with pytest.raises(ValueError, match="radius"):
        lwa_rows(lat, radius=0)
    with pytest.raises(ValueError, match="no row"):
        lwa_rows(np.array([10.0, 20.0, 30.0]), hemisphere='south')
    with pytest.raises(ValueError, match="lat"):
        lwa_rows(np.array([10.0, np.nan]))
    with pytest.raises(ValueError, match=r"pole row\(s\) at latitude \[90.0\]"):              # an active pole row has no equivalent latitude
        lwa_rows(lat, lat_bounds=(30, 90), hemisphere='north')
    with pytest.raises(ValueError, match=r"latitude \[-90.0\]"):
        lwa_rows(lat, lat_bounds=(30, 90), hemisphere='south')
    assert lwa_rows(lu.gaussian(), lat_bounds=(30, 90))["active"].sum() == 32          # no pole row: the band may end at 90


# ---- the fixtures of the GPU tests are not trivial -----------------------------------------------------------------------------------
def test_the_fixture_conditions_hold_on_the_statement():
    """the conditions tests/test_gpu_lwa.py asserts before it compares, with the seeds it uses"""
    import test_gpu_lwa as g
    for ny, nx in g.SHAPES:
        for dtype in (np.float32, np.float64):
            lat, z = g.fixture(ny, nx, dtype=dtype)
            tab = lu.rows(lat)
            assert g.busy(lu.from_table(z, tab), tab), (ny, nx)
    for nx in (3, 8):
        tab = lu.rows(g.TWO_ROWS, hemisphere="north")
        assert g.busy(lu.from_table(g.two_rows_field(nx), tab), tab), nx
    lat = lu.grid(5.0)
    tab = lu.rows(lat)
    z = lu.field(lat, 65, steps=3, seed=1)
    assert lu.nonzero_share(lu.from_table(z, tab), tab) >= 0.5
    zq = lu.quantised(z)
    assert lu.tie_rows(zq, tab) >= 3 and lu.tie_rows(z, tab) == 0
    # a contour is out of reach once the NaNs have eaten the area equatorward of its row: rows near the equator go first
    low = lu.rows(lat, lat_bounds=(5, 75))
    zn = lu.sprinkle(z, low, [np.nan], share=0.15, seed=5, steps=[0])
    ref = lu.from_table(zn, low, return_ref=True)[1]
    bad, good = lu.nan_rows(ref, low)
    assert bad[0] >= 2 and good[0] >= 2 and bad[1] == 0


# ---- the cases of tests/test_gpu_lwa_edges.py: each reaches the edge it is named for ---------------------------------------------------
EDGE_GROUPS = ("cap", "scan", "weight", "probe", "strip", "pair", "zero", "round")
_searched = {}


def searched(name):
    """[(step, domain, lu.bisection(...), the keys of lu.contours(...))] of an edge case, computed once"""
    import test_gpu_lwa_edges as e
    if name not in _searched:
        z, tab = e.case(name)
        _searched[name] = [(s, d, lu.bisection(z[s], tab, dom), lu.contour_keys(z[s], tab, dom)) for s in range(z.shape[0]) for d, dom in enumerate(lu.domains(tab))]
    return _searched[name]


def edge_parts(e, name):
    """the parts the GPU test of a case compares"""
    return (0, 1, 2) if e.CASES[name][0] in ("zero", "round") or name == "cap-nx4-f32" else (0,)


@pytest.mark.parametrize("group", EDGE_GROUPS)
def test_the_restated_bisection_finds_the_statements_contours_on_every_edge_case(group):
    import test_gpu_lwa_edges as e
    assert e.names(group)
    for name in e.names(group):
        for s, d, found, keys in searched(name):
            assert found["keys"] == keys, (name, s, d)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_restated_bisection_on_1_to_70_active_rows(dtype):
    for na in range(1, 71):
        tab = lu.custom_table([na + 3], [range(2, na + 2)])
        z = lu.steep_field(tab, 8, 1, na, dtype, 400.0)
        assert lu.nonzero_share(lu.from_table(z, tab), tab) >= 0.5, na
        planes = (z, lu.quantised(z, 100.0), lu.sprinkle(lu.quantised(z, 50.0), tab, [np.nan, np.inf, -np.inf, 0.0, -0.0], share=0.15, seed=na))
        for zz in planes:
            dom = lu.domains(tab)[0]
            found = lu.bisection(zz[0], tab, dom)
            assert found["keys"] == lu.contour_keys(zz[0], tab, dom) and found["probes"] == na.bit_length() and found["per"] == 1, na


@pytest.mark.parametrize("group", EDGE_GROUPS)
def test_the_statement_is_the_per_pixel_loop_on_every_edge_case(group):
    """all (step, active row, column) triples where the domains have fewer than 100 rows, 40 drawn ones per domain otherwise (the
    loop is a Python loop over the domain's rows per pixel)"""
    import test_gpu_lwa_edges as e
    for name in e.names(group):
        z, tab = e.case(name)
        dtype = z.dtype.type
        steps, _ny, nx = z.shape
        outs = {part: e.want(name, part)[0] for part in edge_parts(e, name)}
        rng = np.random.default_rng(len(name))
        for dom in lu.domains(tab):
            pos = [p for p, j in enumerate(dom) if tab["active"][j]]
            if not pos:
                continue
            triples = [(s, p, c) for s in range(steps) for p in pos for c in range(nx)]
            if len(dom) >= 100:
                triples = [triples[i] for i in rng.choice(len(triples), 40, replace=False)] + [(steps - 1, pos[0], 0), (0, pos[-1], nx - 1)]
            Z = {s: lu.contours(z[s], tab, dom)[0] for s in {t[0] for t in triples}}
            for s, p, c in triples:
                j = dom[p]
                a, y = lu.pixel(z[s], tab, dom, p, c, Z[s][p])
                with np.errstate(invalid="ignore", over="ignore"):
                    vals = [np.array(dtype(v * tab["S"][j])) if not np.isnan(Z[s][p]) else np.array(dtype(np.nan)) for v in (a + y, a, y)]
                assert all(lu.same_bits(vals[part], np.array(o[s, j, c])) for part, o in outs.items()), (name, s, j, c)


def test_every_edge_case_reaches_the_edge_it_is_named_for():
    import test_gpu_lwa_edges as e
    for name in e.CASES:                                                         # the search widths follow n_act in every case
        _z, tab = e.case(name)
        for (s, d, found, _keys), dom in zip(searched(name), lu.domains(tab) * 99):
            na = sum(int(tab["active"][j]) for j in dom)
            assert found["probes"] == na.bit_length() and found["per"] == (2 if na >= 1024 else 1), (name, s, d)
    per = {name: {f["per"] for _, _, f, _ in searched(name)} for name in e.names("cap") + e.names("scan") + e.names("weight")}
    assert all(per[name] == {1} for name in per if "na1023" in name) and sum("na1023" in name for name in per) == 2
    assert all(per[name] == {2} for name in per if "na1023" not in name) and len(per) == 4 + 12 + 2
    gaps = e.case("scan-gaps-nx4-f32")[1]
    assert int(gaps["active"].sum()) == 1024 and len(gaps["active"]) == 2043 and np.count_nonzero(np.diff(np.flatnonzero(gaps["active"])) > 1) > 300
    probes = {int(e.case(name)[1]["active"].sum()): searched(name)[0][2]["probes"] for name in e.names("probe")}
    assert sorted(probes) == list(e.PROBE_NA) and all(probes[2 ** b] == b + 1 and probes[2 ** b + 1] == b + 1 for b in range(1, 10))
    assert all(probes[2 ** b - 1] == b for b in range(1, 10)) and probes[1] == 1
    for dtype, bits in (("f32", 32), ("f64", 64)):
        for kind, rounds in (("adjacent", 1), ("zeros", 1), ("span", bits)):
            assert [f["rounds"] for _, _, f, _ in searched("round-%s-%s" % (kind, dtype))] == [rounds, rounds], (kind, dtype)
        s0, s1 = (f for _, _, f, _ in searched("round-nan-" + dtype))
        assert s0["clamped"] > 0 and None in s0["keys"] and s0["keys"][-1] is not None and s1["clamped"] == 0 and None not in s1["keys"]
        assert [f["rounds"] for _, _, f, _ in searched("zero-flat-" + dtype)] == [0, 0]
    # the plans: the LDS of both kernels at the capacity edge, strips of one unit in both forms
    p = _native.lwa_plan(8, 2043, 4)
    assert (p["ok"], p["lds"], p["lds_sel"], p["strip"], p["vec"]) == (1, 65376, 65536, 4, 1)
    assert _native.lwa_plan(4, 2043, 1, aligned=False)["strip"] == 1 and _native.lwa_plan(4, 2043, 3)["strip"] == 1 and _native.lwa_plan(4, 2043, 4, aligned=False)["nstrips"] == 4
    assert _native.lwa_plan(4, 600, 24)["nstrips"] == 6 and _native.lwa_plan(4, 600, 24)["strip"] == 4
    # (a scalar strip is one column wide from 1 025 rows on -- 2 048 // rows --, not from 513: 600 rows x 5 columns are strips of 3 and 2)
    p600, p1030 = _native.lwa_plan(4, 600, 5), _native.lwa_plan(4, 1030, 5)
    assert (p600["strip"], p600["nstrips"]) == (3, 2) and (p1030["strip"], p1030["nstrips"]) == (1, 5) and p1030["vec"] == 0
    assert _native.lwa_plan(4, 1024, 5)["strip"] == 2 and _native.lwa_plan(4, 1025, 5)["strip"] == 1 and _native.lwa_plan(4, 512, 8)["strip"] == 4 and _native.lwa_plan(4, 513, 8)["nstrips"] == 2
    for name, (rows, nx, (vec, strip, nstrips)) in e.STRIP_PLANS.items():
        p = _native.lwa_plan(4, rows, nx, 1, 3)
        assert (p["vec"], p["strip"], p["nstrips"]) == (vec, strip, nstrips) and e.case(name)[0].shape == (3, rows, nx), name
    # the weights: bucket sums near 2^45, caps below 2^63
    wmax = e.case("weight-max")[1]
    cap0 = lu.caps(wmax, lu.domains(wmax)[0], 4)[0]
    assert cap0 == 4 * 2043 * (2 ** 32 - 1) and 2 ** 44 < cap0 < 2 ** 46 and np.all(e.case("weight-one")[1]["W"] == 1)
    # the pairs: unequal numbers of active rows, a domain without one, a shared first row
    acts = {name: [sum(int(tab["active"][j]) for j in dom) for dom in lu.domains(tab)] for name, tab in ((n, e.case(n)[1]) for n in e.names("pair"))}
    assert {tuple(v) for v in acts.values()} == {(700, 10), (10, 700), (0, 10), (10, 0), (699, 10)}
    first = [dom[0] for dom in lu.domains(e.case("pair-shared-nx4")[1])]
    assert first[0] == first[1] and not e.case("pair-shared-nx4")[1]["active"][first[0]]


@pytest.mark.parametrize("group", EDGE_GROUPS)
def test_no_edge_case_can_pass_with_an_all_zero_output(group):
    """ordinary cases: at least half of the statement's active pixels are finite and not 0, the condition of tests/test_gpu_lwa.py;
    the two-valued planes (as all_equal there) hold both values among their active contours instead"""
    import test_gpu_lwa_edges as e
    for name in e.names(group):
        z, tab = e.case(name)
        out, ref = e.want(name)
        if e.CASES[name][2]:
            assert lu.nonzero_share(out, tab) >= 0.5, (name, lu.nonzero_share(out, tab))
            continue
        values = np.unique(lu.key(z.reshape(-1)))
        assert len(values) == 2
        for s in range(z.shape[0]):
            assert set(np.unique(lu.key(ref[s, tab["active"] != 0]))) == set(values), (name, s)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_zero_weight_rows_share_their_neighbours_contour(dtype):
    import test_gpu_lwa_edges as e
    z, tab = e.case("zero-steep-" + dtype)
    dom = lu.domains(tab)[0]
    caps = lu.caps(tab, dom, 8)
    same = list(e.ZERO_ROWS) + [e.ZERO_ROWS[-1] + 1]                              # positions 17 .. 21: nothing weighs between them
    assert len({caps[p] for p in same}) == 1 and caps[same[0] - 1] > caps[same[0]] > caps[same[-1] + 1] and all(tab["active"][dom[p]] for p in same)
    assert [int(tab["W"][dom[p]]) for p in same] == [0, 0, 0, 0, int(tab["W"][dom[21]])] and tab["W"][dom[21]] > 0
    ref = e.want("zero-steep-" + dtype)[1]
    for s in range(2):
        assert len({float(ref[s, dom[p]]) for p in same}) == 1 and ref[s, dom[same[0] - 1]] > ref[s, dom[same[0]]] > ref[s, dom[same[-1] + 1]]
        found = searched("zero-steep-" + dtype)[s][2]
        a0 = same[0] - e.ZERO_ACTIVE[0]
        assert len(set(found["keys"][a0:a0 + 5])) == 1
    # weighted pixels all equal, other values on the rows that weigh nothing: no round, yet an output
    z, tab = e.case("zero-flat-" + dtype)
    out, ref = e.want("zero-flat-" + dtype)
    weighted = (tab["W"] != 0) & (tab["active"] != 0)
    assert len(np.unique(z)) > 50 and np.all(z[:, tab["W"] != 0] == 5500.0) and np.all(ref[:, tab["active"] != 0] == 5500.0)
    assert np.count_nonzero(out[:, weighted]) >= 0.5 * out[:, weighted].size and np.all(np.isfinite(out))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_matches_its_restatement_at_the_form_and_capacity_edges():
    for esz in (4, 8):
        for rows in (1, 2, 13, 19, 37, 91, 361, 511, 512, 513, 682, 683, 1023, 1024, 1025, 1790, 1791, 1792, 1983, 1984, 2038, 2043, 2044, 2039, 2040, 2047, 2048, 2049, 4096, 8192, 16384, 16385):
            for nx in (1, 3, 4, 8, 24, 65, 360, 1440):
                if rows * nx > 2 ** 31 - 1:
                    continue
                for aligned in (True, False):
                    for ndom, steps in ((1, 1), (2, 7), (2, 3000)):
                        assert _native.lwa_plan(esz, rows, nx, ndom, steps, aligned) == lu.plan(esz, rows, nx, ndom, steps, aligned), (esz, rows, nx, aligned, ndom, steps)
    # the form edge: rows of a multiple of 4 pixels on aligned pointers
    assert [_native.lwa_plan(4, 37, nx)["vec"] for nx in (3, 4, 5, 8)] == [0, 1, 0, 1] and _native.lwa_plan(8, 37, 8, aligned=False)["vec"] == 0
    # the strip rule: 2048 pixels of LDS, whole units, never wider than the row -- and its edge at 361 rows (a quarter degree)
    assert _native.lwa_plan(4, 91, 360)["strip"] == 20 and _native.lwa_plan(4, 91, 360)["nstrips"] == 18
    assert _native.lwa_plan(4, 361, 4) == dict(ok=1, vec=1, strip=4, nstrips=1, lds=5776, lds_sel=11712, blocks=1, grid=1, xcd=0, sel_blocks=1, sel_grid=1, sel_xcd=0)
    assert _native.lwa_plan(4, 361, 1440)["strip"] == 4 and _native.lwa_plan(4, 361, 1441)["strip"] == 5 and _native.lwa_plan(4, 513, 1440)["strip"] == 4
    assert _native.lwa_plan(8, 19, 3)["strip"] == 3 and _native.lwa_plan(8, 19, 65)["strip"] == 65
    # the capacity edge: the contour kernel's words (2 043 rows), before the strip's pixels
    assert _native.lwa_plan(8, 2043, 4)["ok"] == 1 and _native.lwa_plan(8, 2044, 4)["ok"] == 0
    assert _native.lwa_plan(4, 2043, 1)["ok"] == 1 and _native.lwa_plan(4, 2044, 1)["ok"] == 0
    assert _native.lwa_plan(4, 37, 8, 2, 1024)["xcd"] == 1 and _native.lwa_plan(4, 37, 8, 2, 1023)["xcd"] == 0
    assert _native.lwa_plan(4, 37, 120, 2, 1024)["sel_xcd"] == 1 and _native.lwa_plan(4, 37, 120, 2, 1023) == dict(lu.plan(4, 37, 120, 2, 1023), sel_blocks=2046, sel_grid=2046, sel_xcd=0, xcd=1)
    with pytest.raises(ValueError):
        _native.lwa_plan(4, 37, 8, ndom=3)
