"""The constructed slabs of tests/seam_forms.py against the numbers they were built for, on the CPU: the restatement of the seam
stage gives exactly the designed counts (8 / 9 operations, 64 / 65 labels, 512 / 513 records of a window, 64 / 65 / 130 records of a
step, 4096 / 4097 operations for the shared tail ...), its operation list applied to the fresh labels is contrack.py:753-763 pixel
for pixel, and the C oracle gives the same flags.  Three wrong restatements are shown to be noticed.  This is what makes
tests/test_gpu_seam_forms.py reach its edges independently of the code under test.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import seam_forms as sm


def test_constants_are_the_sources():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contrack_amd", "csrc")
    sd, rs, api = (open(os.path.join(src, f)).read() for f in ("ctk_seam_dev.hip", "ctk_resolve_dev.hip", "ctk_api.hip"))
    num = lambda text, name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (num(sd, "SD_LAB"), num(sd, "SD_OPS_OWN"), num(sd, "SD_BATCH")) == (sm.SD_LAB, sm.SD_OPS_OWN, sm.SD_BATCH)
    assert "t0 += %d" % sm.SD_WINDOW in sd and "nrec <= 64" in sd
    assert "std::min(h->debug_sd_ops, %d) : %d" % (sm.SD_OPS, sm.SD_OPS) in api
    assert (num(rs, "FZ_TW"), num(rs, "FZ_HS"), num(rs, "FZ_CS"), num(rs, "FZ_PROBES")) == (sm.FZ_TW, sm.FZ_HS, sm.FZ_CS, sm.FZ_PROBES)
    assert "uint32_t op_cap_hint = %d;" % sm.OP_CAP_HINT in api and "std::max<size_t>(ids_guess, %d)" % sm.OWN_IDS_FLOOR in api
    assert "R / 32" in api and "R / 256" in api
    assert "|= %d" % sm.REASON_OPCAP in api and "|= %d" % sm.REASON_CLUSTER in api


@pytest.mark.parametrize("name", sm.NAMES)
def test_slab_has_the_designed_counts(oracle_lib, name):
    k, d = sm.case(name), sm.design(name)
    assert k.m.size <= 3200000
    # the overlap filter keeps everything (but what a case is built to lose)
    kept = sm.kept(name)
    assert int((kept != k.m).sum()) == k.dropped
    lab, dr = sm.labels(name), sm.driven(name)
    s = dr.summary()
    for key in ("clusters", "labels", "ops", "max_ops", "records", "window"):
        assert s[key] == d[key], (key, s[key], d[key])
    if "fold" in d:
        assert s["fold"] == d["fold"]
    assert len(sm.records(lab)) == d["records"] and len(sm.clusters(lab)[0]) == d["clusters"]
    # the operation list IS the reference's relabelling
    want = sm.reference_merge(lab)
    assert np.array_equal(sm.apply(lab, dr.ops), want)
    ids = np.unique(want)
    assert len(ids[ids > 0]) == d["ids"], (len(ids[ids > 0]), d["ids"])
    # the C oracle: the same final flags (persistence 1 removes nothing and ids are not renumbered)
    flag, n = sm.oracle_result(oracle_lib, name)
    assert np.array_equal(flag, want) and n == len(np.unique(flag)) - 1
    # the caps that keep the GPU test honest
    broken = sm.limits_broken(k, dr)
    own_ids, tail = sm.first_call_slots(k)
    in_tail = sm.tail_ops(dr, own_ids)
    if d["expect"] == 0:
        assert not broken and in_tail <= tail
        assert s["labels"] <= sm.SD_LAB and s["max_ops"] <= sm.SD_OPS and s["window"] <= sm.SD_BATCH
    elif d["expect"] == sm.REASON_CLUSTER:
        assert len(broken) == 1 and in_tail <= tail, broken
    else:
        assert d["expect"] == sm.REASON_OPCAP and not broken and in_tail == tail + 1
    if "tail_ops" in d:
        assert in_tail == d["tail_ops"] and (own_ids, tail) == (sm.OWN_IDS_FLOOR, sm.OP_CAP_HINT)
        assert sm.count_runs(k.m) // 256 <= sm.OP_CAP_HINT


def test_edges_that_the_cases_sit_on():
    s = lambda n: sm.driven(n).summary()
    e = lambda n: sm.case(n).expect
    # (a) 8 own slots
    assert [s("a_comb_%d" % k)["max_ops"] for k in (8, 9)] == [8, 9] == [sm.SD_OPS_OWN, sm.SD_OPS_OWN + 1]
    assert sorted(c["ops"] for c in sm.driven("a_combs_mixed").clusters.values()) == [3, 8, 8, 8, 9, 9, 9, 10]
    # the late bar has the largest label and is `hi` of the first operation only
    for k in (8, 9):
        ops = sm.driven("a_comb_%d_late" % k).ops
        assert ops[0][0] == k + 1 and all(o[1] == 1 for o in ops) and len({o[0] for o in ops}) == k
    # (b) 64 labels
    assert [(s(n)["labels"], e(n)) for n in ("b_comb_63", "b_comb_64")] == [(64, 0), (65, 512)]
    assert s("b_comb_64")["max_ops"] == 64                         # (the operations alone would fit: the labels do not)
    # (c) the hook
    assert [e("c_comb_12_caps_%d_%d" % c) for c in ((64, 12), (64, 11), (13, 64), (12, 64))] == [0, 512, 0, 512]
    assert (s("c_comb_12_caps_64_12")["labels"], s("c_comb_12_caps_64_12")["max_ops"]) == (13, 12)
    # (d) folds
    assert [s("d_ladder_tall_%d" % d)["fold"] for d in (1, 2, 3, 63)] == [1, 2, 3, 63]
    assert [s("d_ladder_short_%d" % d)["fold"] for d in (3, 20)] == [2, 2]
    assert sm.case("d_ladder_tall_63").shape == (67, 128, 132) and s("d_ladder_tall_63")["labels"] == 64
    for n, d in (("d_ladder_tail_3", 3), ("d_ladder_tail_62", 62), ("d_ladder_tail_62_mirror", 62)):
        assert sm.driven(n).ops[-1][:2] == (d + 2, 1) and s(n)["labels"] == d + 2 and s(n)["fold"] == d      # D -> C_d, at the end of a fold of depth d
    for n in ("d_inflow", "d_inflow_mirror"):                      # B is `hi` twice: the second time after A flowed into it
        assert [o[:2] for o in sm.driven(n).ops] == [(3, 2), (2, 1), (4, 2), (2, 1)]
        assert sm.driven(n).ops[1][2][2:4] == (0, 6)               # box(B): rows 0 .. 6
    # (e) later windows bring labels and operations
    for L, wins in ((64, 1), (65, 2), (128, 2), (129, 3)):
        dr = sm.driven("e_windows_%d" % L)
        assert len(next(iter(dr.clusters.values()))["win"]) == wins
        born = sorted({o[2][0] for o in dr.ops})                   # first steps of the `hi` boxes: where operations are recorded
        assert born == sorted({0, 63, 64, L - 1} & set(range(L)))
    # (f) 512 records of a window
    assert [(s(n)["window"], e(n)) for n in ("f_batch_512", "f_batch_513", "f_batch_512_plus_8")] == [(512, 0), (513, 512), (512, 0)]
    assert s("f_batch_512_plus_8")["records"] == 520
    # (g) chunks of 64 records
    assert [s("g_chunk_%d" % n)["records"] for n in (64, 65, 130)] == [64, 65, 130]
    for n in (65, 130):                                            # the last operations are recorded behind the first chunk
        dr = sm.driven("g_chunk_%d" % n)
        first_rec = {}
        for i, r in enumerate(dr.records):
            first_rec.setdefault(r[4], i)
        assert max(first_rec[o[0]] for o in dr.ops) >= 64
    # (h) windows of all clusters
    assert sm.design("h_crowd_30")["window_all"] == 280 and sm.design("h_crowd_7")["window_all"] == 96
    assert s("h_crowd_30")["records"] == 280 and s("h_crowd_30")["window"] == 40
    # (i) records of one step
    for nrec, ncl in ((64, 1), (64, 40), (65, 1), (65, 2), (65, 40), (130, 1), (130, 2), (130, 40)):
        dr = sm.driven("i_step_%d_clusters_%d" % (nrec, ncl))
        per = np.bincount([r[0] for r in dr.records])
        assert per.tolist() == [nrec, nrec] and len(dr.clusters) == ncl and all(c["t0"] == 0 for c in dr.clusters.values())
    # (j) groups and lanes
    assert sm.design("j_stripes_64")["group_ends"] == [63] and sm.design("j_stripes_65_end63")["group_ends"] == [61, 63]
    assert sm.design("j_stripes_129_end63")["group_ends"] == [63, 127] and sm.design("j_stripes_129_cross")["group_ends"] == [99, 127]
    for n in ("j_stripes_65_end63", "j_stripes_129_end63", "j_stripes_129_cross"):
        lab = sm.labels(n)
        rows = int(((lab[0, :, 0] > 0) & (lab[0, :, -1] > 0)).sum())
        assert rows == sm.design(n)["group_ends"][-1] + 1
    recs = [r for r in sm.driven("j_groups_mixed").records if r[0] == 0]
    assert [r[1:3] for r in recs[:40]] == [(2 * i, 2 * i) for i in range(40)] and len({r[3:] for r in recs[:40]}) == 1
    assert [r[1:] for r in recs[40:]] == [(82, 82, 4, 4), (84, 84, 4, 5), (86, 128, 6, 7)]
    lab = sm.labels("j_groups_mixed")
    assert lab[0, 80, 0] == lab[0, 80, -1] == 3 and not any(r[3] == 3 for r in recs)
    # (k) the hashes
    k = [sm.design("k_hash_%d_T16" % p) for p in (15, 16, 33)]
    assert [(q["labels_per_workgroup"], q["clusters_per_workgroup"]) for q in k] == [(480, 240), (512, 256), (1056, 528)]
    assert (k[0]["labels_per_workgroup"] < sm.FZ_HS and k[0]["clusters_per_workgroup"] < sm.FZ_CS
            and k[2]["labels_per_workgroup"] > sm.FZ_HS and k[2]["clusters_per_workgroup"] > sm.FZ_CS)
    # (l) the tail
    assert [sm.design(n)["tail_ops"] for n in ("l_tail_4096", "l_tail_4097")] == [4096, 4097] and [e("l_tail_4096"), e("l_tail_4097")] == [0, 256]
    # (m) roots beyond the ids that own slots
    dr = sm.driven("m_high_root")
    assert sorted(dr.clusters) == [8201, 8206] and min(dr.clusters) >= sm.first_call_slots(sm.case("m_high_root"))[0]
    assert sorted(c["ops"] for c in dr.clusters.values()) == [4, 9]
    # (n) the removed component would have been a cluster of its own
    raw = sm.drive(sm.fresh_labels(sm.case("n_filtered_away").m)).summary()
    assert (raw["clusters"], raw["ops"], raw["records"]) == (2, 4, 16) and s("n_filtered_away")["clusters"] == 1


# ---- the restatement has teeth: three plausible but wrong versions are noticed ------------------------------------------------
def test_plain_union_is_noticed():
    """the short ladder: what an operation leaves outside the box of the next one keeps its label"""
    for n in ("d_ladder_short_3", "d_ladder_short_20", "d_ladder_short_20_mirror"):
        lab = sm.labels(n)
        want = sm.reference_merge(lab)
        wrong = sm.union_merge(lab)
        assert not np.array_equal(wrong, want)
        assert len(np.unique(wrong)) - 1 == 1 and len(np.unique(want)) - 1 == sm.design(n)["ids"] > 1
    lab = sm.labels("d_ladder_tall_63")                            # (with boxes that hold everything the union IS the answer)
    assert np.array_equal(sm.union_merge(lab), sm.reference_merge(lab))


def test_dropping_the_inflow_rule_is_noticed():
    """without "nothing flowed into hi since its last op" the stranded fragment asks for its relabel again on every arm step: two
    more operations than the driver records (the flags stay right -- the extra operations find no pixel to move)"""
    for n, ops, more in (("d_stranded", 2, 2), ("d_stranded_mirror", 2, 2), ("d_inflow", 4, 1)):
        lab = sm.labels(n)
        wrong = sm.Drive(lab, inflow_rule=False)
        assert len(sm.driven(n).ops) == sm.design(n)["ops"] == ops and len(wrong.ops) == ops + more
        assert np.array_equal(sm.apply(lab, wrong.ops), sm.reference_merge(lab))


def test_label_order_is_noticed():
    """operations recorded in the order of their labels instead of (t, y): the short ladder's largest label sits on the FIRST row, so
    its operations come last and find the boxes of the others already emptied; the flags differ"""
    for n in ("d_ladder_short_20", "d_inflow"):
        lab = sm.labels(n)
        wrong = sm.Drive(lab, order="label")
        assert not np.array_equal(sm.apply(lab, wrong.ops), sm.reference_merge(lab))
