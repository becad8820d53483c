"""The launch rule of the run_lifecycle reductions (ctk_life_plan in contrack_amd/csrc/ctk_forms.h, through
ctk_debug_lifecycle_plan) against its restatement in tests/life_forms.py, and the slabs of tests/test_gpu_lifecycle_forms.py against
the limits they are meant to sit on.  No GPU needed."""
import numpy as np
import pytest

import life_forms as lf
from contrack_amd import _native


def test_restatement_agrees_with_the_library():
    n = 0
    for T in lf.SWEEP_T:
        for ny in lf.SWEEP_NY:
            for nx in lf.SWEEP_NX:
                for f64 in (False, True):
                    for fa, va in ((0, 0), (4, 0), (16, 0), (0, 4), (0, 8), (0, 16), (16, 16), (0, 32 if f64 else 20)):
                        got = _native.debug_lifecycle_plan(T, ny, nx, f64, fa, va)
                        assert got == lf.life_plan(T, ny, nx, f64, fa, va), (T, ny, nx, f64, fa, va)
                        n += 1
    assert n == 6 * 5 * 9 * 2 * 8


@pytest.mark.parametrize("shape,want", sorted(lf.PINNED.items()))
def test_pinned_plans(shape, want):
    p = _native.debug_lifecycle_plan(*shape)
    assert (p["rw"], p["nsx"], p["nby"]) == want
    assert p["rw"] * lf.LB_WAVES * p["nby"] >= shape[1] > p["rw"] * lf.LB_WAVES * (p["nby"] - 1)        # the bands cover the rows, none is idle


def test_vec_needs_nx_and_both_alignments():
    for nx in (4, 8, 255, 256, 257, 360):
        for f64 in (False, True):
            for fa in (0, 4, 8, 16, 20):
                for va in (0, 4, 8, 16, 24, 32):
                    want = nx % 4 == 0 and fa % 16 == 0 and va % (32 if f64 else 16) == 0
                    assert _native.debug_lifecycle_plan(6, 9, nx, f64, fa, va)["vec"] == int(want), (nx, f64, fa, va)
    assert _native.debug_lifecycle_plan(3, 9, 256, True, 0, 16)["vec"] == 0
    assert _native.debug_lifecycle_plan(3, 9, 256, False, 0, 16)["vec"] == 1


def test_crossing_ids_per_pass():
    assert [_native.debug_lifecycle_plan(1, 9, nx)["ks"] for nx in (1, 64, 8192, 8193, 65535)] == [32, 32, 32, 31, 4]


def test_bad_arguments():
    with pytest.raises(ValueError):
        _native.debug_lifecycle_plan(0, 9, 8)
    with pytest.raises(ValueError):
        _native.debug_lifecycle_plan(1, 0, 8)


def test_hashes_are_the_kernels():
    assert lf.lb_start(1, 256) == (2654435761 >> 16) & 255 and lf.lc_start(1) == 2654435761 >> 22
    assert lf.lc_start(-1) == ((2 ** 32 - 2654435761) >> 22) and lf.lb_start(-2 ** 31, 128) == (2 ** 31 >> 16) & 127
    first, second = lf.chain_ids()
    assert len(set(first)) == 100 and len(set(second)) == 300 and not set(first) & set(second)
    assert min(first) < 0 < max(first) and min(second) < 0 < max(second)


# ---- the slabs of the GPU file sit where they are meant to -----------------------------------------------------------------
def _ids(plane):
    return len(np.unique(plane[plane != 0]))


def test_stated_steps_follow_from_the_limits():
    cases = [lf.ids_case(), lf.ids_case(reverse=True), lf.crossing_case(), lf.narrow_case(1), lf.narrow_case(2), lf.wide_case(),
             lf.seam_table_case(), lf.chain_case(), lf.dense_case()]
    for c in cases:
        assert c["steps"] == [lf.expected_rounds(p) for p in c["flag"]]


def test_ids_case_counts():
    for rev in (False, True):
        c = lf.ids_case(rev)
        assert c["flag"].shape == (6, 40, 64)
        assert [_ids(p) for p in c["flag"]] == (lf.IDS_PER_STEP[::-1] if rev else lf.IDS_PER_STEP)
        assert lf.life_plan(6, 40, 64)["rw"] * lf.LB_WAVES == 20
    fwd, rev = lf.ids_case()["flag"], lf.ids_case(True)["flag"]
    assert _ids(fwd[2][:20]) == 128 and _ids(fwd[2][20:]) == 0                 # one workgroup's 128-slot table, full
    assert 0 < _ids(rev[3][:20]) < 128 and 0 < _ids(rev[3][20:]) < 128         # the same 128 ids over both workgroups
    assert 0 < _ids(rev[2][:20]) < 128 and _ids(rev[2]) == 129                 # 129: no workgroup's table overflows, the time step's count does


def test_crossing_case_counts_and_patterns():
    c = lf.crossing_case()
    assert [len(lf.crossing_ids(p)) for p in c["flag"]] == lf.CROSS_PER_STEP
    assert all(30 <= _ids(p) - n <= 60 for p, n in zip(c["flag"], lf.CROSS_PER_STEP))
    p = c["flag"][3]
    cols = [np.unique(np.nonzero(p == 1000 + q)[1]) for q in range(33)]
    gaps = np.diff(cols[4])
    assert (gaps == gaps.max()).sum() >= 2                                      # a tie for the largest gap
    assert len(cols[1]) == 64 and list(cols[2]) == [0, 63]
    w = lf.wide_case()
    assert w["flag"].shape == (2, 8, 2080) and lf.life_plan(2, 8, 2080)["nsx"] == 9
    for t, ids in enumerate(lf.WIDE_COLUMNS):
        assert 1 <= len(ids) <= lf.LB_KS
        for q, (cs, shift) in enumerate(ids):
            cs = np.array(cs)
            assert shift == cs[np.argmax(np.diff(cs)) + 1]
    big = np.array(lf.WIDE_COLUMNS[0][0][0])
    k = int(np.argmax(np.diff(big)))
    assert big[k] <= 2047 < 2048 <= big[k + 1]                                  # straddles the strip and the 64-word boundary


def test_seam_table_case_counts():
    p = lf.seam_table_case()["flag"][0]
    ids = np.unique(p[p != 0])
    assert len(ids) == 1040 > lf.LC_HASH and len(lf.crossing_ids(p)) == 0
    assert (ids % 2 == 0).sum() == (ids % 2 == 1).sum() == 520 > lf.LC_NL
    assert max((ids % 4 == j).sum() for j in range(4)) <= lf.LC_NL


def test_chain_and_dense_case_sorts():
    for c in (lf.chain_case(), lf.dense_case()):
        f = c["flag"]
        labels = np.concatenate([np.unique(p[p != 0]) for p in f]).astype(np.int64)
        lrange = int(labels.max() - labels.min()) + 1
        assert (lrange > 8 * len(labels) + 65536) == bool(c["sort"])
        assert (labels < 0).any() and len(np.intersect1d(np.unique(f[0]), np.unique(f[1]))) > 4     # ids in both steps: (label, t) order shows
    c = lf.chain_case()["flag"]
    assert _ids(c[0]) <= lf.LB_GN < _ids(c[1]) <= lf.LC_NL
    assert {-2 ** 31, 2 ** 31 - 1, -1} <= set(np.unique(c[0]).tolist()) & set(np.unique(c[1]).tolist())


@pytest.mark.parametrize("shape,dtype,plan", lf.RW_CASES)
def test_rw_cases_reach_the_stated_plan(shape, dtype, plan):
    got = _native.debug_lifecycle_plan(*shape, dtype == np.float64)
    assert {k: got[k] for k in plan} == plan
    T, ny, nx = shape
    assert (nx > lf.LB_SW and nx % lf.LB_SW != 0) == (nx == 260)                                 # a partial second strip
    c = lf.rw_case(T, ny, nx)
    f = c["flag"]
    busy = np.nonzero(f.reshape(T, -1).any(axis=1))[0]
    assert len(busy) == 33 and busy[0] == 0 and busy[-1] == T - 1
    assert sorted({len(lf.crossing_ids(f[t])) for t in busy}) == [0, 1, 2, 3, 4]
    rw = plan["rw"]
    for t in busy:
        p = f[t]
        assert lf.expected_rounds(p) == 0
        assert ((p == 1).any(axis=1)[[y for y in range(ny) if y not in lf.CROSS_ROWS]]).all()       # the tall contour, over every wave boundary
        for y in range(rw - 1, ny - 1, rw):
            ident = p[y, 3] if p[y, 3] >= 10 else p[y, 6]
            assert ident >= 10 and not (p[:y] == ident).any() and (p[y + 1] == ident).any()           # starts on the last row of a band
        assert not (p[:ny - 1] == 5).any() and (p[ny - 1] == 5).any()
        assert p[0, 0] == 6 and p[ny - 1, nx - 1] == 7 and (p == 6).sum() == (p == 7).sum() == 1
        col, half = p[:, 5], ny // 2
        assert ((col[1:half - 1] != col[2:half]) | np.isin(np.arange(1, half - 1), lf.CROSS_ROWS) | np.isin(np.arange(2, half), lf.CROSS_ROWS)).all()
        stacked = [int(v) for v in np.unique(p[half:, 4]) if v >= 40]
        assert len(stacked) >= 2 and all((p[:, 4] == v).sum() in (7, (ny - 1 - half) % 7) for v in stacked)     # one right below the other
        assert (p[half:ny - 1, 4] >= 40).all() and len(np.unique(p[p != 0])) <= lf.LB_GN


def test_vec_and_regrowth_cases():
    for nx in lf.VEC_NX:
        c = lf.vec_case(nx)
        assert c["flag"].shape == (3, 9, nx) and _ids(c["flag"][2]) == 130 and c["steps"][2] == 1
        assert _ids(c["flag"][0]) > 3 and (c["flag"] < 0).any()
    c = lf.regrowth_case()
    assert [_ids(p) for p in c["flag"]] == [2560, 2560] and c["steps"] == [4, 4]
