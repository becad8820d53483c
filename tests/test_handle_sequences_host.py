"""tests/handle_sequences.py without a GPU: every written sequence contains what its name claims (computed from the arguments of its
operations as the library computes its buffer sizes), the seeded generator is deterministic, covers every family and never draws a
consumer without its resident slab, and every reference function of the vocabulary runs on the smallest shape."""
import numpy as np
import pytest

import handle_sequences as hs


@pytest.fixture(scope="module", autouse=True)
def oracle_built(oracle_lib):
    return oracle_lib


def _rises_and_falls(values):
    """some request exceeds everything before it (the buffer must grow) and a later one is smaller (the grown buffer is reused)"""
    values = [v for v in values if v]
    grew = [i for i in range(1, len(values)) if values[i] > max(values[:i])]
    return bool(grew) and any(values[j] < values[i] for i in grew for j in range(i + 1, len(values)))


def _families_touching(ops, buf):
    return {op.family for op in ops if op.io[buf]}


def test_shapes_are_what_the_module_says():
    n = {k: int(np.prod(v)) for k, v in hs.SHAPES.items()}
    assert (hs.SHAPES["mult4"][1] * hs.SHAPES["mult4"][2]) % 4 == 0 and (hs.SHAPES["odd"][1] * hs.SHAPES["odd"][2]) % 2 == 1
    assert n["large"] > 4 * max(n["mult4"], n["odd"])             # float64 of the smaller two stays below float32 of the large one, twice over
    assert hs.NLEV == 5 and np.count_nonzero(hs.LEVEL_W) == 3 and hs.LEVEL_W[2] == 0 and hs.LEVEL_W[1] != 0 and hs.LEVEL_W[3] != 0


def test_io_grows_and_shrinks_does():
    ops = hs.io_grows_and_shrinks()
    assert [op.family for op in ops] == ["frequency", "track", "level_mean", "anomalies", "spells", "composite", "lifecycle"]
    for buf in ("io_in", "io_out"):
        assert _rises_and_falls([op.io[buf] for op in ops]), buf
        assert len(_families_touching(ops, buf)) >= 2, buf
    assert all(op.io["pin_in"] == 0 and op.io["pin_out"] == 0 for op in ops)          # array entries: nothing pinned


def test_pinned_chunks_up_and_down_does():
    ops = hs.pinned_chunks_up_and_down()
    assert [op.family for op in ops] == ["frequency_cb", "composite_cb", "lifecycle_stream", "level_mean_cb", "track_stream", "anomalies_stream", "spells_cb"]
    for buf in ("pin_in", "pin_out", "io_in", "io_out"):
        assert _rises_and_falls([op.io[buf] for op in ops]), (buf, [op.io[buf] for op in ops])
        assert len(_families_touching(ops, buf)) >= 2, buf
    assert all(op.io["chunks"] >= 2 for op in ops)                                   # both buffers of every pair are used


def test_resident_sequences_keep_their_slab_in_the_model():
    for seq, slab_name, n_consumers in ((hs.resident_anomaly_survives(), "anom", 4), (hs.resident_level_mean_survives(), "level", 1)):
        state = {"anom": None, "level": None}
        hs.apply_residency(state, seq[0])
        assert state[slab_name] is not None
        between = [op for op in seq[1:] if op.needs is None]
        assert len({op.family for op in between}) >= 5
        for op in seq[1:]:
            if op.needs:
                assert state[op.needs] is not None, op
            hs.apply_residency(state, op)
        assert sum(1 for op in seq if op.needs == slab_name and not op.family.startswith("resident")) == n_consumers
        # the calls in between write io_in / io_out with more bytes than the producer did, on another shape
        assert max(op.io["io_in"] for op in between) > seq[0].io["io_in"] and {op.key for op in between} - {seq[0].key}
    seq = hs.resident_anomaly_survives()
    fams = [op.family for op in seq]
    for f in ("frequency", "spells", "level_mean", "percentile", "percentile_groups", "percentile_field", "std_field", "track", "lifecycle"):
        assert f in fams, f
    # the climatology-only calls work on slabs larger than the resident one (a buffer sized for theirs would have to grow) and, in
    # the model, neither leave nor drop an anomaly slab
    only = [op for op in seq if op.family in ("climatology", "climatology_resident")]
    assert [op.family for op in only] == ["climatology", "climatology", "climatology_resident"]
    for op in only:
        assert np.prod(hs.SHAPES[op.key]) > np.prod(hs.SHAPES[seq[0].key]) and op.gives is None and "anom" not in op.drops
    assert fams.index("climatology_resident") < fams.index("resident_generation")


def test_invalidated_residents_refuse_in_the_model():
    seq = hs.invalidated_residents_refuse()
    state = {"anom": None, "level": None}
    refusals = 0
    for i, op in enumerate(seq):
        if op.args.get("refuse"):
            need = hs.CONSUMERS[op.family]
            assert state[need] is None, (i, op)                   # the model agrees that the slab is gone
            refusals += 1
        hs.apply_residency(state, op)
    assert refusals == 12                                         # the six consumers after release_io and after the calls without keep
    assert not seq[-1].args.get("refuse") and seq[-1].needs is None


def test_tracking_caches_changes_one_thing_at_a_time():
    ops = hs.tracking_caches()
    tracks = [op for op in ops if op.family == "track"]
    a = [op.args for op in tracks]
    assert ops[1].family != "track" and ops[1].io["io_in"] > ops[0].io["io_in"] and ops[1].io["io_out"] > 0          # another family grows both
    assert a[1]["thr"] != a[0]["thr"] and a[1]["wvar"] == a[0]["wvar"] and a[1]["gorl"] == a[0]["gorl"]                # only thr
    assert a[2]["wvar"] != a[1]["wvar"] and a[2]["thr"] == a[1]["thr"] and a[2]["gorl"] == a[1]["gorl"]                # only w
    assert a[3]["gorl"] == "<" and a[3]["wvar"] == a[2]["wvar"] and a[3]["thr"] == a[2]["thr"]                        # only the compare
    assert a[4]["dtype"] == "f8" and a[3]["dtype"] == "f4" and tracks[4].key == tracks[3].key                       # float64, the same T
    assert {k: v for k, v in a[4].items() if k != "dtype"} == {k: v for k, v in a[3].items() if k != "dtype"}
    assert a[5]["per_step"] and not a[4]["per_step"] and {k: v for k, v in a[5].items() if k != "per_step"} == {k: v for k, v in a[4].items() if k != "per_step"}
    assert [op.family for op in ops[7:]] == ["track_field", "track", "track_segments", "track", "track_dev"]
    # the second call of track_dev launches speculatively and keeps the launch: the project's model of the labelling launches says so
    spec = hs.second_call_forms(ops[-1].key, ops[-1].args["thr"], ops[-1].args["seed"])
    assert spec["speculative"] and spec["kept"] and spec["forms"] != 0
    # every change changes the result: a cache that kept the old value would be seen
    wants = [op.want() for op in tracks]
    for i in (1, 2, 3, 5):
        assert not np.array_equal(wants[i][0], wants[i - 1][0]), i
    assert np.array_equal(wants[4][0], wants[3][0])                                                               # the lifted slab: the same result
    plain = tracks[-1].want()
    assert not np.array_equal(ops[7].want()[0], plain[0]) and not np.array_equal(ops[9].want()[0], plain[0])     # field and segments matter


def test_sticky_settings_sequence():
    ops = hs.sticky_settings_do_not_leak()
    assert [op.family for op in ops] == ["set_sticky", "frequency", "spells", "anomalies", "composite", "lifecycle", "clear_sticky", "track"]
    key = ops[0].key
    # the call's own segments of spells / anomalies differ from no segments, so a leak or a loss of either would be seen
    assert not all(np.array_equal(a, b) for a, b in zip(ops[2].want(), hs.spells(key).want()))
    assert not np.array_equal(ops[3].want()[0], hs.anomalies(key).want()[0], equal_nan=True)
    assert not np.array_equal(hs.want_track_segments(key)[0], ops[-1].want()[0])


def test_failed_stream_sequence():
    ops = hs.a_failed_stream_then_others()
    failing = [i for i, op in enumerate(ops) if op.args.get("fail_chunk")]
    assert [ops[i].family for i in failing] == ["frequency_cb", "level_mean_cb", "track_stream"]
    for i in failing:
        assert ops[i].args["fail_chunk"] == 3 and ops[i].io["chunks"] == 5
        nxt, after = ops[i + 1], ops[i + 2]
        assert nxt.io["chunks"] >= 2 and nxt.family.split("_")[0] != ops[i].family.split("_")[0]                 # a streamed call of another family
        assert after.io["pin_in"] == 0 and after.family.split("_")[0] not in (ops[i].family.split("_")[0], nxt.family.split("_")[0])
    # the reader really gives up on its third call and has seen the first two chunks
    calls = []
    rd = hs._chunks_reader(np.zeros((10, 1, 1)), fail_chunk=3, calls=calls)
    out = np.empty((2, 1, 1))
    rd(0, 2, out)
    rd(2, 2, out)
    with pytest.raises(hs.ReaderGaveUp):
        rd(4, 2, out)
    assert calls == [(0, 2), (2, 2), (4, 2)]


def test_exact_rows_sequence():
    ops = hs.exact_rows_follow_their_slabs()
    fams = [op.family for op in ops]
    assert fams[:6] == ["lifecycle", "lifecycle_exact", "frequency_dev", "spells_dev", "composite_dev", "lifecycle_exact"]
    assert all(op.io == hs.NO_IO for op in ops[2:5]) and not ops[5].args.get("stale")            # caller buffers only: still fresh
    stale = [i for i, op in enumerate(ops) if op.args.get("stale")]
    breakers = [ops[i - 1].family for i in stale if not ops[i - 1].args.get("stale")]
    assert breakers == ["frequency", "track", "level_mean", "anomalies", "percentile_field", "release_io", "anomalies_stream", "anomalies", "anomalies_resident"]
    for i in stale:
        b = ops[i - 1] if not ops[i - 1].args.get("stale") else ops[i - 2]
        if b.family == "anomalies_resident":
            # no staging buffer is written: only the generation of the resident anomaly slab can refuse here, and the rows before it
            # came from lifecycle(field=None)
            assert b.io == hs.NO_IO and "anom" in b.drops
            assert [op.family for op in ops[:i] if op.family.startswith("lifecycle") and op.family != "lifecycle_exact"][-1] == "lifecycle_resident"
        else:
            assert b.family == "release_io" or b.io["io_in"] > 0                                # each other breaker writes a handle buffer
    assert sum(1 for op in ops if "lifecycle_columns" in op.note) == 7
    # the climatology of the (larger) resident mean alone writes neither: the rows after it are asked for again and must be right
    c = fams.index("climatology_resident")
    assert ops[c].io == hs.NO_IO and not ops[c].drops and fams[c - 1] == "lifecycle_exact" and fams[c + 1] == "lifecycle_exact"
    assert not ops[c + 1].args.get("stale") and np.prod(hs.SHAPES[ops[c].key]) > np.prod(hs.SHAPES[ops[c - 2].key])
    grow = [op for op in ops if op.family == "anomalies" and op.key == "large"]
    assert grow and grow[0].io["io_in"] > ops[0].io["io_in"]                                    # "a growing anomalies"
    # every stale check is followed by a lifecycle that makes the rows right again
    for i in stale:
        nxt = next(op.family for op in ops[i + 1:] if op.family.startswith("lifecycle") and not op.args.get("stale"))
        assert nxt in ("lifecycle", "lifecycle_resident"), (i, nxt)               # (a lifecycle call comes before the next fresh rows)
    assert not ops[-1].args.get("stale") and ops[-1].family == "lifecycle_exact"


def test_seeded_generator_is_deterministic_and_covers_the_vocabulary():
    seqs = [hs.seeded(s) for s in range(hs.N_SEEDS)]
    again = [hs.seeded(s) for s in range(hs.N_SEEDS)]
    assert [[repr(op) for op in q] for q in seqs] == [[repr(op) for op in q] for q in again]
    assert all(len(q) == hs.N_OPS for q in seqs)
    count = {f: 0 for f in hs.FAMILIES}
    keys, dtypes = set(), set()
    for q in seqs:
        state = {"anom": None, "level": None}
        for op in q:
            if op.needs:
                assert state[op.needs] is not None, (q, op)       # never a consumer without its resident slab
            hs.apply_residency(state, op)
            count[op.family] += 1
            keys.add(op.key)
            dtypes.add(op.args.get("dtype"))
    assert min(count.values()) >= 2, sorted(count.items(), key=lambda kv: kv[1])[:5]
    assert set(hs.SHAPES) <= keys and {"f4", "f8"} <= dtypes
    assert len({repr(q) for q in seqs}) == hs.N_SEEDS


def _one_of_each():
    k = hs.SMALLEST
    a, lv = (k, "f4", 3, False), ("level", k, "f4", 4)
    return [hs.track(k), hs.track(k, "f8", per_step=True), hs.track_field(k), hs.track_segments(k), hs.track_stream(k), hs.track_dev(k), hs.track_resident(a),
            hs.frequency(k), hs.spells(k, segments=True), hs.composite(k), hs.composite_resident(a), hs.lifecycle(k), hs.lifecycle_stream(k),
            hs.lifecycle_resident(a), hs.level_mean(k), hs.anomalies(k), hs.anomalies(k, "f8", segments=True), hs.anomalies_stream(k),
            hs.anomalies_resident(lv), hs.climatology(k), hs.climatology_resident(lv), hs.percentile(k), hs.percentile_resident(a), hs.percentile_groups(k), hs.percentile_field(k), hs.std_field(k)]


def test_every_reference_runs_on_the_smallest_shape():
    T, ny, nx = hs.SHAPES[hs.SMALLEST]
    ops = _one_of_each()
    assert {op.family for op in ops} | set(hs.CONSUMERS) | {"release_io"} >= {f.replace("_cb", "").replace("_dev", "") for f in hs.FAMILIES}
    for op in ops:
        w = op.want()
        assert w is not None, op
        first = w[0] if isinstance(w, tuple) else w
        assert np.asarray(first).size > 0, op
        assert op.same is not None
    # the references see something: contours, spells, flagged steps, finite anomalies
    assert hs.track(hs.SMALLEST).want()[1] > 10 and hs.track_resident((hs.SMALLEST, "f4", 3, False)).want()[1] > 10
    assert hs.frequency(hs.SMALLEST).want().max() > 1 and hs.spells(hs.SMALLEST).want()[2].max() > 2
    assert len(hs.lifecycle(hs.SMALLEST).want()[0]) > 20 and len(hs.lifecycle_resident((hs.SMALLEST, "f4", 3, False)).want()[0]) > 20
    assert np.isfinite(hs.anomalies(hs.SMALLEST).want()[0]).mean() > 0.8
    # the band mean's order: exact on integers, NaNs left out, NaN for none; another order gives other bits on wide values
    assert hs.band_mean(np.arange(3000.0)) == 1499.5 and hs.band_mean([np.nan, 2.0, np.nan, 4.0]) == 3.0 and np.isnan(hs.band_mean([np.nan]))
    wide = np.random.default_rng(0).standard_normal(5000) * 10.0 ** np.random.default_rng(1).uniform(-8, 8, 5000)
    assert abs(hs.band_mean(wide) - np.mean(wide)) <= 1e-9 * np.abs(wide).mean() and hs.band_mean(wide) != float(np.cumsum(wide)[-1] / 5000)
    assert hs.same_percentile((hs.band_mean(wide[:100]), wide[:100]), wide[:100]) and not hs.same_percentile((np.nextafter(hs.band_mean(wide[:100]), 9e99), wide[:100]), wide[:100])
    # a refusal is recognised by its words
    assert hs.refused_with(hs.STATE_RC, "overwrote")(hs.StateError("libcontrack_hip rc=-6: x overwrote y"), None)
    assert not hs.refused_with(hs.STATE_RC, "overwrote")(hs.StateError("libcontrack_hip rc=-5: x overwrote y"), None)
    assert set(hs.REFUSALS) == set(hs.CONSUMERS)
    # a comparison accepts its own reference and rejects a changed one
    w = hs.track(hs.SMALLEST).want()
    assert hs.same_flag((w[0].copy(), w[1]), w) and not hs.same_flag((w[0] + (w[0] == 1), w[1]), w)
    lw = hs.lifecycle(hs.SMALLEST).want()
    bent = lw[1].copy()
    bent["sx"][0] = np.nextafter(bent["sx"][0], np.inf)
    assert hs.same_life((lw[0].copy(), lw[1].copy()), lw) and not hs.same_life((lw[0], bent), lw)
