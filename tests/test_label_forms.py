"""The planes of tests/test_gpu_label_forms.py have the run and component counts they claim, and together they reach every row-count,
2-D labelling and overlap form on both sides of every branch the selection lets a plane reach (tests/label_forms.py restates the
selection in ctk_forms.h and the kernels' guards, and is compared here with what the library itself decides: ctk_debug_forms).  No GPU
needed."""
import numpy as np
import pytest

import label_forms as lf


def test_restatement_edges():
    # v0b: 961 .. 1088 words of at most 256 rows; v0_ok: at most 960 words in shards of more than 65536 steps
    assert lf.label_variant(8, 181, 360, 768, False) == "v1_768" and lf.label_variant(8, 181, 360, 769, False) == "v1hi_768"
    assert lf.label_variant(8, 256, 256, 1024, False) == "v1hi_768" and lf.label_variant(8, 256, 256, 1025, False) == "v2"
    assert lf.label_variant(8, 192, 288, 900, False) == "v1"
    assert lf.label_variant(65537, 192, 288, 832, False) == "v1_832" and lf.label_variant(65537, 192, 288, 833, False) == "v1hi_832"
    assert lf.label_variant(65536, 192, 288, 900, False) == "v1"
    assert lf.label_variant(8, 1024, 64, 4096, False) == "v3" and lf.label_variant(8, 1024, 64, 4097, False) == "glb"
    assert lf.label_variant(8, 1025, 64, 0, False) == "glb"
    assert lf.label_variant(8, 721, 1440, 0, True) == "one" and lf.label_variant(8, 721, 1440, 4097, True) == "glb"
    assert lf.staged("v1", 128, 9) and not lf.staged("v1", 577, 2)                   # 1152 / 1154 words
    assert lf.staged("v2", 32, 64) and not lf.staged("v2", 683, 3)                    # 2048 / 2049 words
    assert not lf.staged("v3", 4, 1) and not lf.staged("one", 4, 1)                   # 1024 threads: never staged
    assert lf.staged("v1_768", 1, 1088) and lf.staged("v1_832", 1, 960)               # the selection edge is the staging edge
    assert lf.tables_in_lds("v1_832", 240) and not lf.tables_in_lds("v1_832", 241)
    assert lf.tables_in_lds("v1_768", 272) and not lf.tables_in_lds("v1_768", 273)
    assert lf.tables_in_lds("v1", 288) and not lf.tables_in_lds("v1", 289)
    assert lf.tables_in_lds("v3", 512) and not lf.tables_in_lds("v3", 513) and not lf.tables_in_lds("glb", 1)
    ov = lambda T, ny, W: lf.overlap_name(lf.overlap_form(T, ny, W, False))
    assert [ov(8, n, 1) for n in (1024, 1025, 1280, 1281, 1536, 1537, 2048, 2049, 8191, 8192)] == \
        ["overlap<4,256,1>", "overlap<5,256,1>", "overlap<5,256,1>", "overlap<6,256,1>", "overlap<6,256,1>", "overlap<8,256,1>",
         "overlap<8,256,1>", "overlap<4,256,1>", "overlap<4,256,1>", "overlap<4,512,1>"]
    assert ov(1025, 128, 64) == "overlap<4,256,1>" and ov(65537, 32, 2) == "overlap<4,128,5>" and ov(65537, 32, 65) == "overlap<4,256,1>"
    assert lf.overlap_form(8, 32, 2, True) == 1042561 and lf.overlap_form(65537, 32, 2, False) == 41285
    assert [lf.rowcount_threads(4, ny, 1) for ny in (256, 257, 2048, 2049)] == [256, 512, 512, 256]
    assert lf.rowcount_threads(2049, 721, 23) == 256 and lf.rowcount_threads(65537, 32, 2) == 128
    # k_rowcount<RCU>: a group is one step of the workgroup's waves, threads / 64 waves x 64 // W rows; need = groups of the plane
    rcu = lambda ny, W, T=4: (lf.rowcount_threads(T, ny, W), lf.rowcount_groups(lf.rowcount_threads(T, ny, W), ny, W))
    assert [rcu(ny, 6) for ny in (160, 161, 240, 241, 256)] == [(256, 4), (256, 6), (256, 6), (256, 8), (256, 8)]            # 40 rows a group: need 4 | 5, 6 | 7, 7
    assert [rcu(ny, 6) for ny in (257, 320, 321, 480, 481, 640, 641)] == [(512, 4), (512, 4), (512, 6), (512, 6), (512, 8), (512, 8), (512, 8)]   # 80 rows: 4, 4 | 5, 6 | 7, 8 | 9
    assert [rcu(ny, 23) for ny in (32, 33, 48, 49, 64, 65)] == [(256, 4), (256, 6), (256, 6), (256, 8), (256, 8), (256, 8)]  # 8 rows a group (64 // 23 = 2 a wave)
    assert rcu(721, 3) == (512, 6)                       # 21 rows a wave step (64 % 3: a lane idle), 168 a group: need 5
    assert rcu(257, 2, 65537) == (128, 6) and rcu(32, 2, 65537) == (128, 4)
    assert rcu(20, 65) == (256, 8) and rcu(2049, 1) == (256, 8) and rcu(2048, 1) == (512, 4)
    # the statistic: the RCU of the first form only
    assert lf.rowcount_groups_stat(4, 20, 65) == 0 and lf.rowcount_groups_stat(4, 2049, 1) == 0 and lf.rowcount_groups_stat(0, 160, 6) == 0
    assert lf.rowcount_groups_stat(4, 2048, 1) == 4 and lf.rowcount_groups_stat(4, 20, 64) == 6 and lf.rowcount_groups_stat(4, 641, 6) == 8
    assert lf.rowcount_name(4, 161, 6) == "rowcount<256,6>" and lf.rowcount_name(4, 20, 65) == "rowcount<256,0>"


def test_rcu_cases_sit_on_the_edges():
    """the rcu_* cases: the restatement gives the threads and the RCU the table of edges names; their planes have runs in the last
    row, in the last word of a row and across word boundaries in the rows of the last, partial group (and of a partial second trip)"""
    for nx, ny, thr, stat in lf.RCU_EDGES:
        c = lf.CASE_BY_NAME["rcu_%dx%d" % (ny, nx)]
        W = (nx + 63) // 64
        assert (c["T"], lf.rowcount_threads(4, ny, W), lf.rowcount_groups_stat(4, ny, W)) == (4, thr, stat), c["name"]
        pl = lf.planes_of(c)
        assert set(lf.schedule_of(c)) == {"a", "b", "c"}
        a, b, full = pl["a"].astype(bool), pl["b"].astype(bool), pl["c"].astype(bool)
        assert b[ny - 1, nx - 1] and b[ny - 1].sum() > 2 and not b[:ny - 1].any()       # the last row, its last word
        assert full[ny - 1].all() and not full[:ny - 1].any()                            # one run over every word of the last row
        cross = lambda m: (m[:, 63::64][:, :(nx - 1) // 64] & m[:, 64::64][:, :(nx - 1) // 64]).any(axis=1)
        crossing = cross(a) | cross(full)                # (nx = 130: its one boundary band, 127 .. 128, lies beyond nx - 3: the last row alone crosses)
        assert crossing[ny - 1]
        if stat:
            per_group = (thr // 64) * (64 // W)
            tail = range((ny - 1) // per_group * per_group, ny)                          # rows of the last group
            assert all(a[y].any() for y in range(ny)) and (nx == 130 or all(crossing[y] for y in tail)), c["name"]
            need = (ny + per_group - 1) // per_group
            assert (need > 8) == (c["name"] in ("rcu_641x360", "rcu_65x1440")), c["name"]      # the second outer trip, partial
    names = {lf.rowcount_name(c["T"], c["ny"], (c["nx"] + 63) // 64) for c in lf.CASES}
    assert {"rowcount<%d,%d>" % (t, u) for t in (256, 512) for u in (4, 6, 8)} | {"rowcount<256,0>", "rowcount<128,4>"} == names


@pytest.mark.parametrize("case", lf.CASES, ids=lambda c: c["name"])
def test_case_planes_have_the_claimed_counts(case, oracle_lib):
    pl = lf.planes_of(case)
    for k in sorted(set(lf.schedule_of(case))):
        p = pl[k]
        runs, comps = lf.claimed(case, k)
        assert int(lf.count_runs(p[None])[0]) == runs, k
        _, n = oracle_lib.label(p[None], 0)
        assert n == comps, k
        spec = case["planes"][k]
        if spec[0] == "stack" and spec[3]:
            assert int((p[:, 0] & p[:, -1]).sum()) == spec[3], k                  # seam rows
    assert case["reach"] <= lf.case_forms(case), case["reach"] - lf.case_forms(case)


def test_cases_reach_every_form():
    got = set()
    for c in lf.CASES:
        got |= c["reach"]
    assert got == set(lf.FORMS), sorted(set(lf.FORMS) - got)


def test_run_ends_at_word_edges():
    """the stack planes put run ends at bits 62, 63, 0 and 1 of mask words and let runs cross a word boundary"""
    c = lf.CASE_BY_NAME["runs_721x1440"]
    p = lf.planes_of(c)["r1024"].astype(bool)
    ends = p & ~np.concatenate([p[:, 1:], np.zeros((p.shape[0], 1), dtype=bool)], axis=1)
    bits = set((np.nonzero(ends)[1] % 64).tolist())
    assert {62, 63, 0, 1} <= bits
    crosses = p[:, 63::64][:, :p.shape[1] // 64] & p[:, 64::64]
    assert crosses.any()
    # runs that end in a partial last word and wrap: seam rows on grids with nx % 64 != 0
    assert any(c["nx"] % 64 and any(s[0] == "stack" and s[3] for s in c["planes"].values()) for c in lf.CASES)


def test_pair_edges_count_pairs():
    """dots and bars: one distinct (c, d) pair per dot with the next plane"""
    import cpu_tables
    for name, want in (("pairs_128", 128), ("pairs_129", 129), ("pairs_600", 600)):
        c = lf.CASE_BY_NAME[name]
        m = lf.mask_of(c).astype(bool)
        tb = cpu_tables.build_tables(m[:3], np.ones(c["ny"], np.int64), np.zeros(c["ny"], np.int64))
        per_t = np.bincount([p[0] for p in tb["pairs"]], minlength=3)
        assert per_t[1] == want and per_t[2] == want


def test_speculation_sequences_reach_their_branches():
    seen = 0
    for seq in lf.SPEC_SEQUENCES:
        h = lf.Handle()
        for T, ny, nx, runs in lf.spec_calls(seq):
            seen |= h.label2d(T, ny, nx, runs)
    assert seen & lf.DISCARDED_BIT and seen & lf.LABEL_BIT["one"] and seen & lf.LABEL_BIT["glb"] and seen & lf.LABEL_BIT["v1hi_832"]


# ---- the restatement against the library's own rules (contrack_amd/csrc/ctk_forms.h, through ctk_debug_forms) -------------------
_SET = ("v1", "v2", "v3", "glb", "one", "v1hi")                  # bit i of ctk_form_query.spec_set / .launched


def _to_bits(vs):
    return sum(1 << i for i, k in enumerate(_SET) if vs[k])


def _from_bits(b):
    return {k: bool(b >> i & 1) for i, k in enumerate(_SET)}


class LibHandle:
    """lf.Handle with every decision taken by the library: the speculative launch, the launch after the scan and the next call's
    set come from ctk_label_speculative / ctk_label_plan / ctk_label_form_bits; what is left here is label2d_speculate's and
    label2d_regrow's bookkeeping (ctk_api.hip)"""

    def __init__(self):
        self.runs_cap, self.spec, self.spec_shape, self.spec_T = 0, 0, None, -1

    def label2d(self, T, ny, nx, runs):
        from contrack_amd import _native
        runs = np.asarray(runs, dtype=np.int64)
        R, mx = int(runs.sum()), int(runs.max())
        spec = self.runs_cap > 0 and self.spec_shape == (ny, nx) and (not self.spec & 8 or self.spec_T >= T)
        p = _native.forms(T, ny, nx, max_runs_step=mx, spec_set=self.spec)
        bits, launched = (p["spec_bits"], p["spec_launched"]) if spec else (0, 0)
        if not (spec and R <= self.runs_cap):
            self.runs_cap = min(R + R // 8 + 1024, 0xffffffff)
            launched = 0
            bits |= lf.DISCARDED_BIT if spec else 0
        p = _native.forms(T, ny, nx, max_runs_step=mx, launched=launched)
        self.spec, self.spec_shape, self.spec_T = p["next_spec"], (ny, nx), T
        return bits | p["missing_bits"]


_EDGE_T = (1, 512, 513, 1024, 1025, 2048, 2049, 65536, 65537)
# (ny, nx): ny * W on both sides of 960, 1088 (also within 256 rows: 240 x 4 / 31 x 31, 136 x 8 / 33 x 33), 2048 and 8192 words; ny of 256 / 257, 1024 / 1025, 2048 / 2049 rows; W of 64 / 65 words
_EDGE_GRIDS = [(ny, 64 * W) for ny, W in ((960, 1), (961, 1), (240, 4), (31, 31), (192, 5), (193, 5), (1088, 1), (1089, 1), (33, 33), (256, 4), (257, 4), (136, 8),
                                           (137, 8), (2048, 1), (2049, 1), (128, 16), (129, 16), (8191, 1), (8192, 1), (128, 64), (127, 65),
                                           (32, 2), (1024, 1), (1025, 1), (181, 6), (721, 23))] + [(181, 360), (192, 288), (721, 1440)]
# k_rowcount<RCU>: need of 4 | 5, 6 | 7, 8 | 9 groups with 128, 256 and 512 threads (W = 1: 128, 256 and 512 rows a group; W = 2: 64 with 128 threads)
_EDGE_GRIDS += [(ny, 64) for ny in (512, 513, 768, 769, 1280, 1281, 1536, 1537)] + [(ny, 128) for ny in (256, 257, 384, 385, 512, 513)] + [(721, 130), (20, 4160)]


def test_shape_rules_agree_with_the_library():
    from contrack_amd import _native
    for T in _EDGE_T:
        for ny, nx in _EDGE_GRIDS + [(c["ny"], c["nx"]) for c in lf.CASES]:
            W = (nx + 63) // 64
            for seg in (False, True):
                p = _native.forms(T, ny, nx, seg=seg)
                assert p["rowcount_threads"] == lf.rowcount_threads(T, ny, W), (T, ny, nx)
                assert p["rowcount_groups"] == lf.rowcount_groups(p["rowcount_threads"], ny, W), (T, ny, nx)
                assert (bool(p["v0b"]), bool(p["v0_ok"]), p["v0_runs"]) == lf._v0(T, ny, W), (T, ny, nx)
                assert p["overlap_form"] == lf.overlap_form(T, ny, W, seg), (T, ny, nx, seg)


def test_labelling_protocol_agrees_with_the_library():
    """one call from every state a handle can be in: every speculative set, run buffers that fit and that do not, the run edges of
    every variant, short and long shards of plain, v0 and v0b planes and of planes no LDS variant takes"""
    n = 0
    for T in (4, 512, 513, 65537):
        for ny, nx in ((181, 360), (32, 128), (721, 1440), (1025, 64)):
            for mx in (0, 768, 769, 832, 833, 1024, 1025, 2048, 2049, 4096, 4097):
                for spec in range(64):
                    for cap, spec_T in ((0, T), (1 << 30, T), (1, T), (1 << 30, T - 1)):
                        a, b = lf.Handle(), LibHandle()
                        a.runs_cap = b.runs_cap = cap
                        a.spec, b.spec = _from_bits(spec), spec
                        a.spec_shape = b.spec_shape = (ny, nx)
                        a.spec_T = b.spec_T = spec_T
                        assert a.label2d(T, ny, nx, [mx, 3]) == b.label2d(T, ny, nx, [mx, 3]), (T, ny, nx, mx, spec, cap, spec_T)
                        assert (_to_bits(a.spec), a.runs_cap) == (b.spec, b.runs_cap)
                        n += 1
    assert n > 40000


def test_cases_and_sequences_agree_with_the_library():
    for c in lf.CASES:
        runs = [lf.claimed(c, k)[0] for k in lf.schedule_of(c)]
        assert lf.Handle().label2d(c["T"], c["ny"], c["nx"], runs) == LibHandle().label2d(c["T"], c["ny"], c["nx"], runs), c["name"]
    for seq in lf.SPEC_SEQUENCES:
        a, b = lf.Handle(), LibHandle()
        for T, ny, nx, runs in lf.spec_calls(seq):
            assert a.label2d(T, ny, nx, runs) == b.label2d(T, ny, nx, runs), seq["name"]
            assert _to_bits(a.spec) == b.spec
