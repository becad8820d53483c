"""The time-shard exchange path (contrack_amd/csrc/ctk_sharded.hip: ctk_track_sharded_*, ranks as host threads on one GPU) at its
capacity and length rules, on the constructed slabs of tests/shard_forms.py:

  capB (components of a cut step)        255 / 256 / 257 / 600, restart at 256 in every call, growth with a second filter round
  capC / capD (shared records / labels)  256 / 257 records, 256 / 257 / 258 labels, remembered hints, ranks with different hints,
                                         the host-driven form, a rank that stays host-driven next to ranks in the device form
  k_sh_pack_shared                       shards of 1024 / 1025 / 2100 steps (offsets carried from trip to trip), local records between
  k_compact_init on a shard              4095 / 4096 / 4097 steps, with and without a halo in front
  k_sh_pack_ext                          2048 / 2049 natural ids, the hook's cap at ne - 1 / ne / ne + 1, own ids at both ends
  background sample                      nx = 72, a single background pixel behind / inside the sample, none at all
  seam tables initialised ahead          fresh handles, below the 1024-label floor, used, too small, used again
  shared-operations reserve              ng and ng - 1 through ctk_debug_set_shared_ops_reserve
  shard shapes                           nine one-step shards, a one-step first / last shard

Every call is compared bit for bit with the C oracle (and the one-call pass, once per slab), and what the call decided -- read back
through ctk_debug_shard_exchange on every rank -- with the restatement of tests/shard_forms.py.  Integers only.
tests/test_shard_forms_host.py shows on the CPU that the slabs hold exactly the counts named here."""
import numpy as np
import pytest

import shard_forms as sf
from contrack_amd import _native
from shard_inproc import sharded_threads

pytestmark = pytest.mark.gpu


class Group:
    """nine handles: 0 .. 7 play ranks, 8 runs the one-call pass.  `mem` models what a handle remembers from call to call: the
    capacities of the shared seam exchange it will offer as hints, and how many labels its seam tables hold."""
    def __init__(self):
        self.h = [_native.Tracker(0) for _ in range(9)]
        self.mem = [dict(capC=0, capD=0, held=0) for _ in range(9)]

    def renew(self, idx):
        for i in idx:
            self.h[i].close()
            self.h[i] = _native.Tracker(0)
            self.mem[i] = dict(capC=0, capD=0, held=0)

    def close(self):
        for h in self.h:
            h.close()


@pytest.fixture(scope="module")
def G():
    g = Group()
    yield g
    g.close()


_ONE_CALL = set()


def run(G, oracle_lib, name, ranks, forms=None, cap_lds=sf.SH_PE_LDS, outside=None, pre=False):
    """one sharded call of case `name` on the handles `ranks`; everything is asserted here.  forms: the X5 form every rank is expected
    to finish in (default: the device form).  Returns (facts of every rank, stats of every rank)."""
    k, e = sf.case(name), sf.expected(name, cap_lds)
    want, nw = sf.oracle_result(oracle_lib, name)
    args = (k.field(), k.thr(), 0, k.wrow(), k.overlap, k.pers, True)
    if name not in _ONE_CALL:
        f1, n1 = (outside or G.h[8]).track(*args, f64=k.f64)
        assert np.array_equal(f1, want) and n1 == nw, "one-call pass against the oracle"
        _ONE_CALL.add(name)
    ranks = list(ranks)
    world = e["world"]
    assert len(ranks) == world and e["any_boundary"]
    forms = list(forms) if forms else [0] * world
    got, ng, st = sharded_threads([G.h[i] for i in ranks], *args, k.cuts, f64=k.f64)
    assert ng == nw and np.array_equal(got, want), (name, ng, nw)
    facts = [G.h[i].debug_shard_exchange() for i in ranks]
    capC, capD, rep = sf.seam_caps(max(G.mem[i]["capC"] for i in ranks), max(G.mem[i]["capD"] for i in ranks), e["sent_records"], e["sent_labels"])
    for r, (i, f) in enumerate(zip(ranks, facts)):
        where = (name, "rank", r, f)
        assert (f["capB"], f["capB_repeats"], f["nlast"], f["nh"]) == (e["capB"], e["capB_repeats"], e["nlast"][r], e["nh"][r]), where
        assert (f["capC"], f["capD"], f["x5_repeats"]) == (capC, capD, rep), where + (capC, capD, rep)
        assert (f["sent_records"], f["sent_labels"]) == (e["sent_records"][r], e["sent_labels"][r]), where
        assert (f["ne"], f["pack_ext_workgroups"], f["shared_ops"]) == (e["ne"], e["pack_ext_workgroups"], e["shared_ops"]), where
        assert f["zero_exchanged"] == e["zero_exchanged"] and f["form"] == forms[r], where
        assert st[r]["fused_pass"] == (1 if forms[r] == 0 else 0) and bool(st[r]["off_fused_path_reason"] & 16) == bool(forms[r] & 6), (where, st[r])
        m = G.mem[i]
        m["capC"], m["capD"] = capC, capD
        if forms[r] & 1:
            assert f["tables_ahead_used"] == -1, where
        else:
            nt = e["NL"] + 2
            used = int(m["held"] >= sf.PREINIT_MIN and nt <= m["held"])
            if pre:
                assert f["tables_ahead_used"] == used, where + (m["held"], nt)
            assert f["tables_ahead_used"] in (0, 1), where
            m["held"] = max(m["held"], sf.tables_held(nt)) if nt > m["held"] else m["held"]
    return facts, st


# ---- a. capB ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sf.NAMES if n.startswith("capb_") and "shrink" not in n])
def test_capb_edges(G, oracle_lib, name):
    """255 / 256 components in a cut step fit the 256 every call starts with; 257 / 600 make every rank repeat the first round's
    exchange once with 449 / 964 -- behind rank 0, between the middle ranks of four, as the halo of a one-step shard, in float64"""
    d = sf.case(name).design
    facts, st = run(G, oracle_lib, name, range(sf.expected(name)["world"]))
    assert all((f["capB"], f["capB_repeats"]) == (d["capB"], d["repeats"]) for f in facts)
    assert all(s["filter_rounds"] == 1 and s["x4_speculated"] == 0 for s in st)


def test_capb_restarts_at_256_in_every_call(G, oracle_lib):
    run(G, oracle_lib, "capb_600_cut1", range(4))
    facts, _ = run(G, oracle_lib, "capb_257_cut1", range(4))
    assert all((f["capB"], f["capB_repeats"]) == (449, 1) for f in facts)


def test_capb_growth_and_a_second_filter_round(G, oracle_lib):
    """257 components and a component dropped ON the cut: the exchange is repeated inside round 1, then the ranks need a second
    round, whose exchange carries the boundary records of the 3-D labelling (speculative X4) with the grown capacity"""
    facts, st = run(G, oracle_lib, "capb_257_shrink", range(4))
    assert all((f["capB"], f["capB_repeats"]) == (449, 1) for f in facts)
    for s in st:
        assert s["filter_rounds"] >= 2 and s["x4_speculated"] == (1 if s["filter_rounds"] > 1 else 0), s


# ---- b. capC / capD, device form ---------------------------------------------------------------------------------------------
def test_shared_record_capacity_and_hints(G, oracle_lib):
    """256 records fit, 257 grow capC to 449 with one repeat; the hint is remembered (no repeat, also for a smaller case); a fresh
    handle next to one that remembers: both end at the remembered capacity"""
    G.renew([0, 1])
    facts, _ = run(G, oracle_lib, "longbar_256", [0, 1])
    assert all((f["capC"], f["capD"], f["x5_repeats"]) == (256, 256, 0) for f in facts) and facts[0]["sent_records"] == 256
    facts, _ = run(G, oracle_lib, "longbar_257", [0, 1])
    assert all((f["capC"], f["x5_repeats"]) == (449, 1) for f in facts) and facts[0]["sent_records"] == 257
    facts, _ = run(G, oracle_lib, "longbar_257", [0, 1])
    assert all((f["capC"], f["x5_repeats"]) == (449, 0) for f in facts)
    facts, _ = run(G, oracle_lib, "longbar_256", [0, 1])
    assert all((f["capC"], f["x5_repeats"]) == (449, 0) for f in facts)
    G.renew([1])
    facts, _ = run(G, oracle_lib, "longbar_257", [0, 1])
    assert all((f["capC"], f["capD"], f["x5_repeats"]) == (449, 256, 0) for f in facts)
    G.renew([0])                                                    # ... and the other way round
    facts, _ = run(G, oracle_lib, "longbar_257", [0, 1])
    assert all((f["capC"], f["capD"], f["x5_repeats"]) == (449, 256, 0) for f in facts)


@pytest.mark.parametrize("name,labels,capd,rep", [("bars_128", 256, 256, 0), ("bars_128_pixel", 257, 452, 1), ("bars_128_touch", 257, 452, 1),
                                                  ("bars_129", 258, 452, 1)])
def test_shared_label_capacity(G, oracle_lib, name, labels, capd, rep):
    """256 labels fit; 257 (a plain label across the cut, or a bar whose halves touch) and 258 grow capD to 449 / 451, rounded up to
    452; the second call remembers"""
    G.renew([0, 1])
    facts, _ = run(G, oracle_lib, name, [0, 1])
    assert all((f["sent_labels"], f["capD"], f["x5_repeats"]) == (labels, capd, rep) for f in facts)
    facts, _ = run(G, oracle_lib, name, [0, 1])
    assert all((f["capD"], f["x5_repeats"]) == (capd, 0) for f in facts)
    facts, _ = run(G, oracle_lib, "bars_5", [0, 1])                 # a smaller case: the hints stay
    assert all((f["capD"], f["x5_repeats"]) == (capd, 0) for f in facts)


# ---- c. the same counts in the host-driven form -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["longbar_256", "longbar_257", "bars_128", "bars_128_pixel", "bars_129"])
def test_host_driven_form_same_capacities(G, oracle_lib, name):
    """rank 0's device seam driver takes one label per cluster (test hook): its local bar poisons the attempt and every rank repeats
    X5 host-driven, growing the capacities from the same hints; in the call after that rank 0 stays host-driven on this grid next to
    rank 1 in the device form -- both take part in ONE all-gather, so both must arrive at the same capD (rounded up to 4)"""
    G.renew([0, 1])
    e = sf.expected(name)
    want = sf.seam_caps(0, 0, e["sent_records"], e["sent_labels"])
    try:
        G.h[0].debug_set_seam_caps(1, 1)
        facts, _ = run(G, oracle_lib, name, [0, 1], forms=[4, 4])
        assert all((f["capC"], f["capD"], f["x5_repeats"]) == want for f in facts)
        facts, _ = run(G, oracle_lib, name, [0, 1], forms=[1, 0])
        assert all((f["capC"], f["capD"], f["x5_repeats"]) == want[:2] + (0,) for f in facts) and want[1] % 4 == 0
    finally:
        G.h[0].debug_set_seam_caps(0, 0)
    run(G, oracle_lib, name, [0, 1])                                # hook cleared: both in the device form again


# ---- d. long shards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sf.NAMES if n.startswith("long_")])
def test_long_shards(G, oracle_lib, name):
    """k_sh_pack_shared walks the shard 1024 steps at a time: shared records behind step 1024 / 2048 / 4096 land behind the ones in
    front (carried offset), local records between them are stepped over; k_compact_init sums in two levels beyond 4096 steps, with
    the halo's component count in front when the shard is rank 1"""
    d = sf.case(name).design
    facts, _ = run(G, oracle_lib, name, [0, 1])
    assert facts[d["long_rank"]]["sent_records"] == d["records"] and facts[0]["shared_ops"] == d["shared_ops"]


# ---- e. k_sh_pack_ext --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sf.NAMES if n.startswith("ext_2")])
def test_extent_exchange_natural_lists(G, oracle_lib, name):
    """2048 ids: 32 workgroups with the list in LDS; 2049: one workgroup, the list in global memory; persistence 4 keeps all of them,
    5 none"""
    k, e = sf.case(name), sf.expected(name)
    facts, _ = run(G, oracle_lib, name, [0, 1])
    assert all((f["ne"], f["pack_ext_workgroups"]) == (k.design["ne"], k.design["workgroups"]) for f in facts)
    assert sf.oracle_result(oracle_lib, name)[1] == (k.design["ne"] - 1 if k.pers == 4 else 0)


def test_extent_exchange_cap_and_search_ends(G, oracle_lib):
    """40 shared ids with own ids right below the first and right above the last; the list's LDS cap (test hook) at 39 / 40 / 41"""
    try:
        for cap, wgs in ((39, 1), (40, 32), (41, 32)):
            for i in (0, 1):
                G.h[i].debug_set_mailbox(0, cap)
            facts, _ = run(G, oracle_lib, "ext_small", [0, 1], cap_lds=cap)
            assert all((f["ne"], f["pack_ext_workgroups"]) == (40, wgs) for f in facts)
    finally:
        for i in (0, 1):
            G.h[i].debug_set_mailbox(0, 0)
    facts, _ = run(G, oracle_lib, "ext_small", [0, 1])
    assert all(f["pack_ext_workgroups"] == 32 for f in facts)


# ---- f. background sample ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sf.NAMES if n.startswith("bg_")])
def test_background_sample(G, oracle_lib, name):
    """nx = 72 (8 valid bits in a row's second word): no background at all, one background pixel behind the 16384-word sample (last
    plane, last valid bit), the same pixel inside the sample, on the last rank only"""
    d = sf.case(name).design
    facts, _ = run(G, oracle_lib, name, [0, 1, 2])
    assert all(f["zero_exchanged"] == d["zero_exchanged"] for f in facts)
    assert sf.oracle_result(oracle_lib, name)[1] == (1 if d["hole"] else 0)


# ---- g. seam tables initialised ahead ------------------------------------------------------------------------------------------
def test_seam_tables_initialised_ahead(G, oracle_lib):
    """fresh handles: nothing ahead; buffers for fewer than 1024 labels: not ahead either; 1030 labels: the first call initialises
    behind the boundary resolution, the second uses the tables initialised ahead, so does a small case after it; 2048 labels do not
    fit what the buffers held; then the first cases again.  Every case has seam merges of clusters across the cut."""
    G.renew([0, 1])
    seq = [("ext_small", 0), ("ext_small", 0), ("pre_big", 0), ("pre_big", 1), ("ext_small", 1), ("ext_2048_pers4", 0), ("pre_big", 1), ("ext_small", 1)]
    for name, used in seq:
        facts, _ = run(G, oracle_lib, name, [0, 1], pre=True)
        assert all(f["tables_ahead_used"] == used for f in facts), (name, used, facts)


# ---- h. shared-operations reserve ----------------------------------------------------------------------------------------------
def test_shared_operations_reserve(G, oracle_lib):
    """five shared operations against a reserve of five (device form) and of four: every rank abandons the device attempt after its
    seam driver was launched and finishes host-driven; the next call without the hook is in the device form again"""
    ranks = [0, 1, 2]
    facts, _ = run(G, oracle_lib, "ops_5", ranks)
    ng = facts[0]["shared_ops"]
    assert ng == sf.expected("ops_5")["shared_ops"] and 3 <= ng <= 20
    try:
        for i in ranks:
            G.h[i].debug_set_shared_ops_reserve(ng)
        run(G, oracle_lib, "ops_5", ranks)
        for i in ranks:
            G.h[i].debug_set_shared_ops_reserve(ng - 1)
        _, st = run(G, oracle_lib, "ops_5", ranks, forms=[2, 2, 2])
        assert all(s["off_fused_path_reason"] & 16 for s in st)
    finally:
        for i in ranks:
            G.h[i].debug_set_shared_ops_reserve(0)
    run(G, oracle_lib, "ops_5", ranks)


# ---- i. shard shapes -----------------------------------------------------------------------------------------------------------
def test_nine_one_step_shards(G, oracle_lib):
    with _native.Tracker(0) as outside:                              # (all of 0 .. 8 play ranks here)
        facts, _ = run(G, oracle_lib, "shapes_nine", range(9), outside=outside)
    assert [f["nh"] for f in facts][1:] == [f["nlast"] for f in facts][:-1]


@pytest.mark.parametrize("name", ["shapes_first", "shapes_last"])
def test_one_step_first_and_last_shard(G, oracle_lib, name):
    run(G, oracle_lib, name, [0, 1])
