"""The constructed slabs of tests/shard_forms.py against the numbers they were built for, on the CPU: the restatement of the
time-shard exchanges gives exactly the designed counts (255 / 256 / 257 components in a cut step, 256 / 257 shared records, 256 /
257 / 258 shared labels, 2048 / 2049 exchanged ids, a background pixel just beyond the sample ...), the C oracle runs on every
slab and its result holds the number of ids the design says.  This is what makes tests/test_gpu_shard_forms.py reach its edges
independently of the code under test.  No GPU needed."""
import re

import numpy as np
import pytest

import shard_forms as sf


def test_constants_are_the_sources():
    import os
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contrack_amd", "csrc")
    sh, kn = open(os.path.join(src, "ctk_sharded.hip")).read(), open(os.path.join(src, "ctk_kernels.hip")).read()
    num = lambda text, name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert num(kn, "CTK_CI_BLOCK") == sf.CTK_CI_BLOCK and "T > 4 * CTK_CI_BLOCK" in sh
    assert (num(sh, "SH_PE_LDS"), num(sh, "SH_PE_BLOCKS")) == (sf.SH_PE_LDS, sf.SH_PE_BLOCKS)
    assert re.search(r"uint32_t capB = %d;" % sf.CAP0, sh) and "t0 += %d" % sf.PACK_SHARED_CHUNK in sh
    assert "%d)" % sf.BG_SAMPLE_WORDS in sh and "n >= %d" % sf.PREINIT_MIN in sh
    assert (sf.grow(257), sf.grow(600), sf.round4(sf.grow(257)), sf.round4(sf.grow(258))) == (449, 964, 452, 452)


@pytest.mark.parametrize("name", sf.NAMES)
def test_slab_has_the_designed_counts(oracle_lib, name):
    k, e = sf.case(name), sf.expected(name)
    d = k.design
    flag, n = sf.oracle_result(oracle_lib, name)
    ids = np.unique(flag)
    ids = ids[ids > 0]
    assert len(ids) == k.ids, (len(ids), k.ids)
    assert n == len(np.unique(flag)) - 1
    if name.startswith("capb"):
        r = d["cut"]
        assert e["nlast"][r] == d["n"] == e["nh"][r + 1] and max(e["nlast"]) == d["n"]
        assert (e["capB"], e["capB_repeats"]) == (d["capB"], d["repeats"])
        assert sum(v == d["n"] for v in e["nlast"]) == 1                      # the crowd stands at one cut only
    if "records" in d and not name.startswith("long_"):
        assert e["sent_records"] == d["records"]
        assert [a - s for a, s in zip(e["all_records"], e["sent_records"])] == d["local_records"]
    if "labels" in d:
        assert max(e["sent_labels"]) == d["labels"]
    if "shared_ops" in d:
        assert e["shared_ops"] == d["shared_ops"]
    if "ne" in d:
        assert e["ne"] == d["ne"] and e["pack_ext_workgroups"] == d["workgroups"]
    if "NL" in d:
        assert e["NL"] == d["NL"]
    if name.startswith("long_"):
        r = d["long_rank"]
        assert e["sent_records"][r] == d["records"] and e["all_records"][r] - e["sent_records"][r] == d["local_records"]
        L = k.cuts[r + 1] - k.cuts[r]
        assert L == d["L"] and (L > sf.PACK_SHARED_CHUNK) == (d["records"] > 5)    # records behind step 1024 need the carried offset
        assert d["local_records"] >= 12                                        # ... and local ones lie in between
    if name.startswith("bg_"):
        assert e["zero_exchanged"] == d["zero_exchanged"] and (0 in flag) == d["hole"]
        assert e["capB_repeats"] == 0 and e["ne"] == 1


def test_edges_that_the_cases_sit_on():
    e = sf.expected
    assert [e("capb_%d_cut0" % n)["capB"] for n in (255, 256, 257, 600)] == [256, 256, 449, 964]
    assert [e("longbar_%d" % n)["sent_records"][0] for n in (256, 257)] == [256, 257]
    assert [max(e(n)["sent_labels"]) for n in ("bars_128", "bars_128_pixel", "bars_128_touch", "bars_129")] == [256, 257, 257, 258]
    assert sf.seam_caps(0, 0, [256, 1], [2, 2]) == (256, 256, 0) and sf.seam_caps(0, 0, [257, 1], [2, 2]) == (449, 256, 1)
    assert sf.seam_caps(0, 0, [9], [257]) == (256, 452, 1) and sf.seam_caps(0, 0, [9], [258]) == (256, 452, 1)
    assert sf.seam_caps(449, 452, [257], [258]) == (449, 452, 0) and sf.seam_caps(0, 449, [9], [449]) == (256, 452, 0)
    assert [e("ext_%d_pers4" % n)["pack_ext_workgroups"] for n in (2048, 2049)] == [32, 1]
    assert [sf.expected("ext_small", c)["pack_ext_workgroups"] for c in (39, 40, 41)] == [1, 32, 32]
    # a one-step shard between two cuts reports the crowded step as its halo only
    h = e("capb_257_halo_only")
    assert h["nlast"] == [257, 6, 6] and h["nh"] == [0, 257, 6]
    # the block that shrinks at the cut: its last component in front of the cut is dropped by the filter
    k = sf.case("capb_257_shrink")
    kept = sf.filtered(k.m, k.wrow(), k.overlap)
    assert not kept[3, 48:52].any() and k.m[3, 48:52].sum() == 32 and (kept[[2, 4]] == k.m[[2, 4]]).all()
    # background: the hole of "beyond" lies behind the sample of its rank, in the last valid bit of a partial word
    assert e("bg_beyond")["zero_in_sample"] == [False] * 3 and e("bg_inside")["zero_in_sample"] == [False, True, False]
    assert e("bg_last_rank")["zero_in_sample"] == [False, False, True] and e("bg_full")["zero_in_sample"] == [False] * 3
    assert 40 * 210 * 2 > sf.BG_SAMPLE_WORDS and 72 % 64 == 8
    # tables initialised ahead: the sequence of test_gpu_shard_forms.py crosses the 1024-label floor and the held count
    nl = [e(n)["NL"] for n in ("ext_small", "pre_big", "ext_2048_pers4")]
    assert nl[0] + 2 < sf.PREINIT_MIN <= nl[1] + 2 and sf.tables_held(nl[0] + 2) < sf.PREINIT_MIN
    assert nl[2] + 2 > sf.tables_held(nl[1] + 2) * 3 // 2
    assert 3 <= e("ops_5")["shared_ops"] <= 20
