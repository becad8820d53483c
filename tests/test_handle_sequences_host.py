"""tests/handle_sequences.py without a GPU: every written sequence contains what its name claims (computed from the arguments of its
operations as the library computes its buffer sizes), the seeded generator is deterministic, covers every family and never draws a
consumer without its resident slab, and every reference function of the vocabulary runs on the smallest shape."""
import numpy as np
import pytest

import handle_sequences as hs


@pytest.fixture(scope="module", autouse=True)
def oracle_built(oracle_lib):
    return oracle_lib


def test_written_sequences_reach_every_form_of_band_and_centred():
    seen = set()
    for sequence in hs.WRITTEN:
        for op in sequence():
            if op.family.split("_")[0] in ("band", "centred") and not op.args.get("refuse") and not op.args.get("fail_chunk") and not op.args.get("stale_generation"):
                seen.add((op.family, op.args["how"]))
                if op.family == "centred" and not op.args["none_kept"]:   # the host-array form sends a band of rows, never whole planes (p.rows < ny)
                    assert 0 < op.io["max_rows"] < hs.SHAPES[op.key][1], op
                if op.family.startswith("band") and op.args.get("columns") is False:
                    seen.add((op.family, "sectors only"))
    want = {("band", "array"), ("band_cb", "cb"), ("band_dev", "dev"), ("band", "sectors only")} | {("band_resident", h) for h in ("array", "cb", "dev")}
    want |= {("centred", "array"), ("centred_cb", "cb"), ("centred_dev", "dev")} | {("centred_resident", h) for h in ("array", "cb", "dev")}
    assert want <= seen, sorted(want - seen)


def test_the_io_model_of_the_runner():
    """grown / check_io: head room where claim_io -> ensure gives it, exact bytes for the pinned pairs, grow-only, zero after release_io"""
    assert hs.grown(0, 1000, "io_in") == 1000 + 125 + 256 and hs.grown(2000, 1000, "io_in") == 2000 and hs.grown(0, 1000, "pin_in") == 1000
    assert hs.grown(1381, 1381, "io_out") == 1381 and hs.grown(1381, 1382, "io_out") == 1382 + 172 + 256 and hs.grown(500, 0, "io_in") == 500
    op = hs.frequency("mult4", "cb", chunk_steps=5)
    cap = dict(hs.NO_IO)
    got = {b: hs.grown(0, op.io[b], b) for b in hs.BUFFERS}
    assert hs.check_io(cap, op, got) == [] and cap == got and got["io_in"] > op.io["io_in"] > 0 and got["pin_in"] == op.io["pin_in"] > 0
    assert hs.check_io(dict(cap), hs.frequency("mult4", "cb", chunk_steps=3), got) == []                      # a smaller request: unchanged
    short = dict(got, io_in=got["io_in"] - 1)
    assert hs.check_io(dict(hs.NO_IO), op, short) == [("io_in", short["io_in"], got["io_in"])]
    assert hs.check_io(dict(hs.NO_IO), op, dict(got, pin_out=8)) == [("pin_out", 8, 0)]                       # a buffer the model says is not touched
    assert hs.check_io(dict(cap), hs.release_io(), got) != [] and hs.check_io(dict(cap), hs.release_io(), dict(hs.NO_IO)) == []
    # a tracking result: 256 bytes of io_out, or the dense bytes of the blocks with complex components, whichever the data ask for
    tr = hs.track("mult4")
    base = {b: hs.grown(0, tr.io[b], b) for b in hs.BUFFERS}
    assert hs.check_io(dict(hs.NO_IO), tr, base) == [] and hs.check_io(dict(hs.NO_IO), tr, dict(base, io_out=40000)) == []
    assert hs.check_io(dict(hs.NO_IO), tr, dict(base, io_out=hs.grown(0, 24 * 19 * 36 * 4, "io_out") + 1)) != []
    # a call that gave up may or may not have claimed its buffers
    fail = hs.frequency("mult4", "cb", chunk_steps=5, fail_chunk=2)
    assert hs.check_io(dict(hs.NO_IO), fail, got, raised=True) == [] and hs.check_io(dict(hs.NO_IO), fail, dict(hs.NO_IO), raised=True) == []


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
    assert [op.family for op in ops] == ["frequency", "centred", "track", "level_mean", "band", "anomalies", "band", "spells", "composite", "lifecycle"]
    for buf in ("io_in", "io_out"):
        assert _rises_and_falls([op.io[buf] for op in ops]), buf
        assert len(_families_touching(ops, buf)) >= 2, buf
    assert {"band", "centred"} <= _families_touching(ops, "io_in") and "band" in _families_touching(ops, "io_out")
    assert all(op.io["pin_in"] == 0 and op.io["pin_out"] == 0 for op in ops)          # array entries: nothing pinned
    # the band with a float64 field on the large shape makes io_in grow (the field is the first slab) and puts the flags into io_out
    bands = [op for op in ops if op.family == "band"]
    T, ny, nx = hs.SHAPES["large"]
    assert bands[0].key == "large" and bands[0].args["dtype"] == "f8" and bands[0].io["io_in"] == 2 * T * ny * nx * 8 and bands[0].io["io_out"] == 2 * T * ny * nx * 4
    assert bands[0].io["io_in"] > max(op.io["io_in"] for op in ops[:ops.index(bands[0])])
    # ... and the one after it asks for the sector tables alone, on a smaller shape, after one that asked for columns and sectors
    assert bands[0].args["columns"] and bands[0].args["sectors"] and bands[1].args["sectors"] and not bands[1].args["columns"] and bands[1].key == "odd"
    assert sorted(bands[1].want()) == ["sec_area", "sec_cnt"]
    # the centred composite of a host array sends the band of rows its windows touch, not whole planes
    ce = ops[1]
    T, ny, nx = hs.SHAPES[ce.key]
    assert ce.key == "mult4" and 0 < ce.io["max_rows"] < ny and ce.io["io_in"] == 2 * ce.io["chunk"] * ce.io["max_rows"] * nx * 4


def test_pinned_chunks_up_and_down_does():
    ops = hs.pinned_chunks_up_and_down()
    assert [op.family for op in ops] == ["frequency_cb", "centred_cb", "composite_cb", "band_cb", "lifecycle_stream", "centred_cb", "level_mean_cb", "band_cb",
                                         "track_stream", "anomalies_stream", "centred_cb", "spells_cb"]
    for buf in ("pin_in", "pin_out", "io_in", "io_out"):
        assert _rises_and_falls([op.io[buf] for op in ops]), (buf, [op.io[buf] for op in ops])
        assert len(_families_touching(ops, buf)) >= 2, buf
    assert {"band_cb", "centred_cb"} <= _families_touching(ops, "pin_in") and {"band_cb", "centred_cb"} <= _families_touching(ops, "io_in")
    assert "band_cb" in _families_touching(ops, "pin_out") and "band_cb" in _families_touching(ops, "io_out")
    assert all(op.io["chunks"] >= 2 for op in ops)                                   # both buffers of every pair are used
    # one band call with both readers (the flags go through pin_out), one with the flag reader alone (they go through pin_in)
    both, alone = [op for op in ops if op.family == "band_cb"]
    assert both.args["dtype"] == "f8" and both.io["pin_out"] == both.io["chunk"] * 9 * 65 * 4 and both.io["pin_in"] == 2 * both.io["pin_out"]
    assert alone.args["dtype"] is None and alone.io["pin_out"] == 0 and alone.io["pin_in"] == alone.io["chunk"] * 31 * 60 * 4 and alone.io["chunks"] >= 3
    # the centred calls: three carrying chunks or more (the buffer of the first is used again), and a chunk that is never read
    pins = [op.io["pin_in"] for op in ops if op.family == "centred_cb"]
    assert pins[1] > pins[0] and pins[1] > pins[2]                                   # up and down within the family as well
    for op in ops:
        if op.family == "centred_cb":
            _a_chunk_without_kept_stamps(op)


def _a_chunk_without_kept_stamps(op, carrying=3):
    """read from the stamps and the chunk length: at least `carrying` chunks hold a kept stamp, and some chunk holds stamps but none
    that is kept"""
    T = hs.SHAPES[op.key][0]
    t, row, col, bin = hs.stamps(op.key)
    c = op.io["chunk"]
    kept = sorted({int(k) for k in t[bin >= 0] // c})
    assert len(kept) == op.io["carrying"] >= carrying and op.io["chunks"] == -(-T // c) > len(kept)
    assert {int(k) for k in t[bin < 0] // c} - set(kept)


def test_resident_sequences_keep_their_slab_in_the_model():
    for seq, slab_name, n_consumers in ((hs.resident_anomaly_survives(), "anom", 10), (hs.resident_level_mean_survives(), "level", 1)):
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
    for f in ("frequency", "spells", "level_mean", "percentile", "percentile_groups", "percentile_field", "std_field", "track", "lifecycle", "band", "centred", "centred_cb"):
        assert f in fams, f
    # the band and centred calls in between are streamed (they claim the staging buffers), on larger shapes than the resident slab's,
    # and the band carries a field; the consumers reach every form of both families
    for op in seq:
        if op.family in ("band", "centred", "centred_cb") and op.needs is None:
            assert op.breaks_exact and np.prod(hs.SHAPES[op.key]) > np.prod(hs.SHAPES[seq[0].key]) and op.args["dtype"], op
    for fam in ("band_resident", "centred_resident"):
        assert [op.args["how"] for op in seq if op.family == fam] == ["array", "cb", "dev"]
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
        elif op.needs:
            assert state[op.needs] is not None, (i, op)
        hs.apply_residency(state, op)
    # the four consumers of before, three forms of band and of centred on the anomaly slab, two consumers of the vertical mean: after
    # release_io and after the calls without keep
    assert refusals == 24
    assert {(op.family, op.args.get("how")) for op in seq if op.args.get("refuse")} >= {(f, h) for f in ("band_resident", "centred_resident") for h in ("array", "cb", "dev")}
    end = next(i for i, op in enumerate(seq) if not op.args.get("refuse") and op.family == "frequency")
    assert not any(op.args.get("refuse") for op in seq[end:])
    # the stale-generation leg: two producers of one shape and type whose slabs differ, the refusals, then the consumers of the NEW slab
    leg = seq[end + 1:]
    assert [op.family for op in leg[:2]] == ["anomalies", "anomalies"] and leg[0].gives[1:3] == leg[1].gives[1:3] and leg[0].gives[3] != leg[1].gives[3]
    a3, a5 = leg[0].want()[0], leg[1].want()[0]
    assert a3.shape == a5.shape and a3.dtype == a5.dtype and not np.array_equal(a3, a5, equal_nan=True)
    assert [(op.family, op.args["how"]) for op in leg[2:5]] == [("band_resident", h) for h in ("array", "cb", "dev")] and all(op.args.get("stale_generation") for op in leg[2:5])
    after = leg[5:]
    assert {op.family for op in after} == {"band_resident", "centred_resident"} and not any(op.args.get("stale_generation") for op in after)
    old = leg[0].gives[1:]
    for op in after:                                              # their references are the new slab's, and differ from the old slab's
        other = (hs.band_resident if op.family == "band_resident" else hs.centred_resident)(old, op.args["how"])
        w, wo = op.want(), other.want()
        if op.family == "band_resident":
            assert not np.array_equal(w["wx"], wo["wx"])
        else:
            assert not np.array_equal(w[0], wo[0])
    # the words of the refusal, both generations in them
    msg = "libcontrack_hip rc=-6: ctk_band_f32: the resident anomaly slab is generation 7, the call names the stale generation 6"
    assert leg[2].same((hs.StateError(msg), 7, 6), None) and not leg[2].same((hs.StateError(msg), 8, 6), None) and not leg[2].same(None, None)


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
    assert [op.family for op in ops] == ["set_sticky", "frequency", "spells", "anomalies", "composite", "band", "centred", "lifecycle", "clear_sticky", "track"]
    assert all(op.io["chunks"] >= 2 for op in ops[5:7]) and ops[5].args["dtype"] and ops[6].io["carrying"] >= 2
    key = ops[0].key
    # the call's own segments of spells / anomalies differ from no segments, so a leak or a loss of either would be seen
    assert not all(np.array_equal(a, b) for a, b in zip(ops[2].want(), hs.spells(key).want()))
    assert not np.array_equal(ops[3].want()[0], hs.anomalies(key).want()[0], equal_nan=True)
    assert not np.array_equal(hs.want_track_segments(key)[0], ops[-1].want()[0])


def test_failed_stream_sequence():
    ops = hs.a_failed_stream_then_others()
    failing = [i for i, op in enumerate(ops) if op.args.get("fail_chunk")]
    assert [ops[i].family for i in failing] == ["frequency_cb", "level_mean_cb", "track_stream", "band_cb", "band_cb", "centred_cb", "frequency_cb", "reversal_cb", "reversal_cb"]
    # the two reversals: the reader of one that keeps gives up on chunk 3 of 5 -- in the model nothing is resident afterwards and the
    # consumers after it are refusals --, the writer of one that keeps nothing gives up on its second chunk -- the anomaly slab of
    # the call before stays, its consumer is right --, and a streamed reversal with reader and writer follows
    i, j = failing[7:]
    assert ops[i].args["keep"] and ops[i].args["fail_which"] == "reader" and ops[i].args["fail_chunk"] == 3 and ops[i].io["chunks"] == 5 and ops[i].drops == ("anom",)
    assert ops[i - 1].gives and ops[i - 1].gives[0] == "anom" and [op.args.get("refuse") for op in ops[i + 1:i + 3]] == [True, True]
    assert ops[i].io["pin_in"] > 0 and ops[i].io["pin_out"] > 0 and ops[i].io["io_out"] > 0                    # a writer: the output chunks as well
    assert not ops[j].args["keep"] and ops[j].args["fail_which"] == "writer" and ops[j].args["fail_chunk"] == 2 and ops[j].io["chunks"] == 5 and ops[j].drops == ()
    assert ops[j - 1].gives and ops[j + 1].family == "track_resident" and not ops[j + 1].args.get("refuse")
    assert ops[j + 2].family == "reversal_cb" and not ops[j + 2].args.get("fail_chunk") and ops[j + 2].io["chunks"] >= 3 and ops[j + 2].key != ops[j].key
    state = {"anom": None, "level": None}
    for op in ops:
        if op.args.get("refuse"):
            assert state[hs.CONSUMERS[op.family]] is None, op
        elif op.needs:
            assert state[op.needs] is not None, op
        hs.apply_residency(state, op)
    failing = failing[:7]
    # a band reader gives up on chunk 3 of 5 -- once the flag reader, once the field reader, which is called after the flag reader of
    # the same chunk --, and the very next call is a streamed band with readers on another shape, of at least three chunks (both
    # pinned twins and both table sets are used, the first set twice)
    assert [ops[i].args["fail_which"] for i in failing[3:5]] == ["flag", "field"]
    for i in failing[3:5]:
        assert ops[i].args["fail_chunk"] == 3 and ops[i].io["chunks"] == 5 and ops[i].io["pin_out"] > 0
        nxt = ops[i + 1]
        assert nxt.family == "band_cb" and not nxt.args.get("fail_chunk") and nxt.key != ops[i].key and nxt.io["chunks"] >= 3 and nxt.args["sectors"] and nxt.args["columns"]
        assert ops[i + 2].io["pin_in"] == 0 and not ops[i + 2].family.startswith("band")
    # a centred reader gives up on its third carrying chunk (two are in flight), then the tracker streams, then the same call succeeds
    i = failing[5]
    assert ops[i].args["fail_chunk"] == 3 and ops[i].io["carrying"] >= 4
    assert ops[i + 1].family == "track_stream" and ops[i + 1].io["pin_in"] > 0 and ops[i + 1].io["chunks"] >= 3
    assert ops[i + 2].family == "centred_cb" and not ops[i + 2].args.get("fail_chunk") and ops[i + 2].key == ops[i].key and ops[i + 2].io == ops[i].io
    _a_chunk_without_kept_stamps(ops[i + 2], carrying=4)
    # ... and a centred reader call directly after another family's failed stream
    i = failing[6]
    assert ops[i].io["chunks"] == 5 and ops[i + 1].family == "centred_cb" and not ops[i + 1].args.get("fail_chunk") and ops[i + 1].io["pin_in"] > 0
    _a_chunk_without_kept_stamps(ops[i + 1])
    for i in failing[:3]:
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
    assert breakers == ["frequency", "track", "level_mean", "anomalies", "percentile_field", "release_io", "band", "band_resident", "centred", "centred_cb", "band_resident",
                        "anomalies_stream", "anomalies", "anomalies_resident"]
    # band and centred: Op.breaks_exact -- the call claims io_in / io_out -- decides whether the rows after it are stale or right, and
    # both kinds occur, of both families
    new = [(i, op) for i, op in enumerate(ops) if op.family.split("_")[0] in ("band", "centred")]
    for i, op in new:
        assert ops[i + 1].family == "lifecycle_exact" and bool(ops[i + 1].args.get("stale")) == op.breaks_exact, (i, op)
        assert op.breaks_exact == bool(op.io["io_in"] or op.io["io_out"])
        last = [o for o in ops[:i] if o.family.startswith("lifecycle") and o.family != "lifecycle_exact"][-1]
        assert last.family == "lifecycle" and last.key == "odd"                                # rows of a host-array call: the io rule alone
    none_kept = [op for _, op in new if op.args.get("none_kept")]
    assert [(op.family, op.key) for op in none_kept] == [("centred", "large"), ("centred_cb", "large")]
    for op in none_kept:                                                                       # streamed forms that claim nothing: no stamp is kept
        assert not op.breaks_exact and op.io["carrying"] == 0 and op.io["chunks"] > 1 and {k: op.io[k] for k in hs.BUFFERS} == hs.NO_IO
        assert not op.want()[0].any() and not op.want()[1].any()
    assert hs.centred("mult4", "cb", chunk_steps=3, none_kept=True).same(hs.centred("mult4", none_kept=True).want() + ([],), hs.centred("mult4", none_kept=True).want())
    kinds = {(op.family, op.args["how"]): op.breaks_exact for _, op in new if not op.args.get("none_kept")}
    assert kinds == {("band", "array"): True, ("band_dev", "dev"): False, ("band_resident", "array"): True, ("band_resident", "cb"): True, ("band_resident", "dev"): False,
                     ("centred", "array"): True, ("centred_cb", "cb"): True, ("centred_dev", "dev"): False, ("centred_resident", "array"): False,
                     ("centred_resident", "dev"): False}
    # (the other forms, which no leg of this sequence holds)
    a = ("mult4", "f4", 3, False)
    assert hs.band("mult4", "cb").breaks_exact and hs.band("mult4", field="f4").breaks_exact and not hs.centred_resident(a, "cb").breaks_exact
    # the non-breakers work on slabs larger than the rows' own: a buffer they had claimed would have had to grow
    for _, op in new:
        if not op.breaks_exact and op.needs is None:
            assert np.prod(hs.SHAPES[op.key]) > np.prod(hs.SHAPES["odd"])
    for i in stale:
        b = ops[i - 1] if not ops[i - 1].args.get("stale") else ops[i - 2]
        if b.family == "anomalies_resident":
            # no staging buffer is written: only the generation of the resident anomaly slab can refuse here, and the rows before it
            # came from lifecycle(field=None)
            assert b.io == hs.NO_IO and "anom" in b.drops
            assert [op.family for op in ops[:i] if op.family.startswith("lifecycle") and op.family != "lifecycle_exact"][-1] == "lifecycle_resident"
        else:
            assert b.family == "release_io" or b.io["io_in"] > 0                                # each other breaker writes a handle buffer
    assert sum(1 for op in ops if "lifecycle_columns" in op.note) == 12
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


def test_reversal_grids_and_the_io_model_of_the_reversal_entries():
    import reversal_util as ru
    for key, (T, ny, nx) in hs.SHAPES.items():
        for second in (False, True):
            tab = hs.rev_table(key, second)
            act = np.flatnonzero(tab["eq"] >= 0)
            lat = hs.rev_lat(key)
            assert (lat[act] > 0).any() and (lat[act] < 0).any(), key                       # active rows in both hemispheres
            r0, r1, a0, a1 = hs.rev_rows(key, second)
            assert 0 < r0 <= a0 < a1 <= r1 < ny, (key, r0, r1, a0, a1)                       # rows 0 and ny - 1: neither read nor written
            for dtype in ("f4", "f8"):
                w = hs.want_reversal(key, dtype, 0, False, second)
                assert 0.05 <= ru.blocked_share(w, tab["eq"]) <= 0.5, (key, second)         # (as tests/test_gpu_reversal.py asks of its fixtures)
                assert not w[:, :a0].any() and not w[:, a1:].any() and w.dtype == hs.DT[dtype]
                assert ru.same_bits(hs.want_reversal(key, dtype, 0, True, second), (w != 0).astype(w.dtype))
        assert not np.array_equal(hs.want_reversal(key, "f4", 0), hs.want_reversal(key, "f4", 1))            # another seed, another slab
        assert np.count_nonzero(hs.want_reversal(key, "f4", 0)) > np.count_nonzero(hs.want_reversal(key, "f4", 0, False, True))      # the third criterion matters
        # a gradient divided by another distance than the rows' own would be seen
        assert ru.differing(hs.want_reversal(key, "f4", 0), ru.from_table(hs.rev_input(key, "f4", 0), hs.rev_table(key), div=15.0)) == np.count_nonzero(hs.want_reversal(key, "f4", 0))
    # io: chunks of whole planes, two per direction; io_out only without keep or with a writer; pinned chunks for reader and writer
    T, ny, nx = hs.SHAPES["odd"]
    plane = ny * nx
    a = hs.reversal("odd", "f8", chunk_steps=7)
    assert {b: a.io[b] for b in hs.BUFFERS} == dict(io_in=2 * 7 * plane * 8, io_out=2 * 7 * plane * 8, pin_in=0, pin_out=0) and a.io["chunks"] == -(-T // 7)
    k = hs.reversal("odd", "f8", chunk_steps=7, keep=True)
    assert {b: k.io[b] for b in hs.BUFFERS} == dict(io_in=2 * 7 * plane * 8, io_out=0, pin_in=0, pin_out=0)
    assert hs.reversal("odd", "f4").io["io_in"] == 2 * T * plane * 4 and hs.reversal("odd", "f4").io["chunks"] == 1
    for keep in (False, True):
        c = hs.reversal("odd", "f4", "cb", chunk_steps=5, keep=keep, sink="writer")
        assert {b: c.io[b] for b in hs.BUFFERS} == dict(io_in=2 * 5 * plane * 4, io_out=2 * 5 * plane * 4, pin_in=5 * plane * 4, pin_out=5 * plane * 4)
    assert {b: hs.reversal("odd", "f4", "dev").io[b] for b in hs.BUFFERS} == hs.NO_IO and {b: hs.level_mean_dev("odd").io[b] for b in hs.BUFFERS} == hs.NO_IO
    # residency: only a call that keeps touches the slot
    assert k.gives == ("anom", "odd", "f8", 0, ("reversal", False, False)) and k.drops == ("anom",) and a.gives is None and a.drops == ()
    assert k.breaks_exact and a.breaks_exact and not hs.reversal("odd", "f4", "dev").breaks_exact and not hs.level_mean_dev("odd").breaks_exact
    lm = hs.level_mean_dev("odd")
    assert lm.gives is None and lm.drops == () and lm.needs is None


def test_reversal_between_the_others_does():
    seq = hs.reversal_between_the_others()
    assert hs.reversal_between_the_others in hs.WRITTEN
    fams = [op.family for op in seq]
    assert fams[0] == "anomalies" and seq[0].gives[0] == "anom"
    state = {"anom": None, "level": None}
    producers, on = [], {"anomalies": set(), "reversal": set()}
    for i, op in enumerate(seq):
        if op.args.get("refuse"):
            assert state[hs.CONSUMERS[op.family]] is None, (i, op)
        elif op.needs:
            assert state[op.needs] is not None, (i, op)
            if op.needs == "anom" and not op.family.startswith("resident"):
                on["reversal" if hs.by_reversal(state["anom"]) else "anomalies"].add(op.family)
        before = state["anom"]
        hs.apply_residency(state, op)
        if op.family.startswith("reversal") and not op.args["keep"]:
            assert state["anom"] == before and before is not None, (i, op)                   # keeps nothing: the slab stays
        if op.gives and op.gives[0] == "anom":
            producers.append(op.family)
    assert producers == ["anomalies", "reversal", "reversal_cb", "reversal", "reversal"]
    assert on["reversal"] >= {"track_resident", "band_resident", "centred_resident", "percentile_resident", "lifecycle_resident", "composite_resident"}
    assert on["anomalies"] >= {"track_resident", "band_resident", "centred_resident"}
    # the reversals that keep nothing come first and work on a larger shape than the resident slab: io_in and io_out grow under it
    first_keep = next(i for i, op in enumerate(seq) if op.family == "reversal" and op.args["keep"])
    plain = [op for op in seq[1:first_keep] if op.family.startswith("reversal")]
    assert [op.family for op in plain] == ["reversal", "reversal_dev"] and plain[0].io["io_in"] > seq[0].io["io_in"] and plain[0].io["io_out"] > 0
    assert fams[first_keep - 4:first_keep].count("resident_generation") == 1 and fams[first_keep + 1] == "resident_generation"
    # the anomalies of the resident vertical mean replace the slab; every consumer of the reversal is then a refusal
    ar = fams.index("anomalies_resident")
    assert fams[ar - 3:ar] == ["level_mean", "level_mean_dev", "resident_level_generation"] and seq[ar - 3].gives[0] == "level"
    n = len(hs._reversal_consumers(("odd", "f4", 0, ("reversal", False, True))))
    assert all(op.args.get("refuse") for op in seq[ar + 1:ar + 1 + n]) and not seq[ar + 1 + n].args.get("refuse")
    # the references of the consumers follow the producer: on the reversal's output they differ from those on the anomaly slab
    a, r = ("odd", "f4", 3, False), ("odd", "f4", 0, ("reversal", False, True))
    assert not np.array_equal(hs.resident_slab(a), hs.resident_slab(r), equal_nan=True) and hs.resident_cut(a) == (40.0, ">=") and hs.resident_cut(r) == (0.0, ">")
    assert hs.track_resident(r).want()[1] > 10 and not np.array_equal(hs.track_resident(r).want()[0], hs.track_resident(a).want()[0])
    assert not np.array_equal(hs.percentile_resident(r).want(), hs.percentile_resident(a).want(), equal_nan=True)
    # two reversals of one shape and type with other values, then the stale generation
    st = [i for i, op in enumerate(seq) if op.args.get("stale_generation")]
    assert len(st) == 2 and [op.family for op in seq[st[0] - 2:st[0]]] == ["reversal", "reversal"]
    g0, g1 = seq[st[0] - 2].gives, seq[st[0] - 1].gives
    assert g0[1:3] == g1[1:3] and g0[3] != g1[3] and not np.array_equal(hs.resident_slab(g0[1:]), hs.resident_slab(g1[1:]))


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
    assert min(count.values()) >= 3, sorted(count.items(), key=lambda kv: kv[1])[:5]
    # the eight families of band and centred are among them (with the 32 of before: 40), and the three reversal entries and
    # level_mean_dev: 44
    assert len(hs.FAMILIES) == 44 and {f + g for f in ("band", "centred") for g in ("", "_cb", "_dev", "_resident")} <= set(hs.FAMILIES)
    assert {"reversal", "reversal_cb", "reversal_dev", "level_mean_dev"} <= set(hs.FAMILIES)
    # the seeded reversals: both dtypes, with and without keep, mask and third criterion, an array and a writer as the sink of the
    # reader form; a missing anomaly slab was made by either producer, and consumers were drawn on a reversal's output
    rev = [op for q in seqs for op in q if op.family.startswith("reversal")]
    for k in ("keep", "mask", "second"):
        assert {op.args[k] for op in rev} == {False, True}, k
    assert {op.args["dtype"] for op in rev} == {"f4", "f8"} and {op.args["sink"] for op in rev if op.family == "reversal_cb"} == {"array", "writer"}
    producers = {q[i].family for q in seqs for i in range(len(q) - 1) if q[i + 1].needs == "anom" and q[i].gives}
    assert producers >= {"anomalies", "reversal"}
    on_reversal = set()
    for q in seqs:
        state = {"anom": None, "level": None}
        for op in q:
            if op.needs == "anom" and hs.by_reversal(state["anom"]):
                on_reversal.add(op.family)
            hs.apply_residency(state, op)
    assert len(on_reversal) >= 4, on_reversal
    # io: every op names the four buffers, and nothing else decides breaks_exact
    for q in seqs:
        for op in q:
            assert set(hs.BUFFERS) <= set(op.io) and all(isinstance(op.io[b], int) and op.io[b] >= 0 for b in hs.BUFFERS), op
            assert op.gives is None or (op.gives[0] in op.drops and op.gives[1] == op.key), op
    for q in seqs:
        for op in q:
            if op.family in ("centred", "centred_cb") and op.io["chunks"] > 1:
                _a_chunk_without_kept_stamps(op, carrying=2)
    assert set(hs.SHAPES) <= keys and {"f4", "f8"} <= dtypes
    assert len({repr(q) for q in seqs}) == hs.N_SEEDS


def _one_of_each():
    k = hs.SMALLEST
    a, lv, r = (k, "f4", 3, False), ("level", k, "f4", 4), (k, "f4", 0, ("reversal", False, False))
    return [hs.track(k), hs.track(k, "f8", per_step=True), hs.track_field(k), hs.track_segments(k), hs.track_stream(k), hs.track_dev(k), hs.track_resident(a),
            hs.frequency(k), hs.spells(k, segments=True), hs.composite(k), hs.composite_resident(a), hs.lifecycle(k), hs.lifecycle_stream(k),
            hs.lifecycle_resident(a), hs.level_mean(k), hs.anomalies(k), hs.anomalies(k, "f8", segments=True), hs.anomalies_stream(k),
            hs.anomalies_resident(lv), hs.climatology(k), hs.climatology_resident(lv), hs.percentile(k), hs.percentile_resident(a), hs.percentile_groups(k), hs.percentile_field(k), hs.std_field(k),
            hs.band(k), hs.band(k, field="f8", columns=False), hs.band(k, field="f4", sectors=False), hs.band_resident(a), hs.centred(k), hs.centred(k, dtype="f8"),
            hs.centred_resident(a), hs.level_mean_dev(k), hs.reversal(k), hs.reversal(k, "f8", "cb", chunk_steps=5, keep=True, mask=True, second=True), hs.reversal(k, how="dev"),
            hs.track_resident(r), hs.percentile_resident(r), hs.band_resident(r), hs.centred_resident(r), hs.lifecycle_resident(r), hs.composite_resident(r)]


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
    # band: flagged pixels in the rows of the band, both sectors (one wraps), a field whose weighted sums are not all zero
    bw = hs.band(hs.SMALLEST, field="f8").want()
    assert sorted(bw) == ["area", "cnt", "sec_area", "sec_cnt", "sec_wx", "wx"] and bw["cnt"].max() > 1 and bw["sec_cnt"].min(axis=0).max() >= 0
    assert (bw["sec_cnt"] > 0).any(axis=0).all() and np.count_nonzero(bw["wx"]) > 10
    sects = hs.band_sectors(hs.SMALLEST)
    assert sects[1][0] + sects[1][1] > nx and hs.band_rows(hs.SMALLEST) == (1, ny - 2)
    assert hs.same_band(bw, bw) and not hs.same_band(dict(bw, wx=np.nextafter(bw["wx"], np.inf)), bw) and not hs.same_band({k: v for k, v in bw.items() if k != "wx"}, bw)
    rb = hs.band_resident((hs.SMALLEST, "f4", 3, False)).want()
    assert rb["cnt"].max() > 0 and np.isfinite(rb["wx"]).all()               # a flagged pixel of the resident slab is above 40: never a NaN
    # centred: about 40 stamps, sorted, bins from -1, every bin filled; on the wide field another order or a split sum has other bits
    t, row, col, bin = hs.stamps(hs.SMALLEST)
    assert 35 <= len(t) <= 45 and np.all(np.diff(t) >= 0) and bin.min() == -1 and set(bin.tolist()) == {-1, 0, 1, 2} and hs.CENTRED == dict(nbins=3, hy=2, hx=3)
    g0, g1 = hs.stamp_gap(hs.SMALLEST)
    assert np.all(bin[(t >= g0) & (t < g1)] == -1) and np.any((t >= g0) & (t < g1))
    x = hs.wide_field(hs.SMALLEST, "f8")
    cw = hs.centred(hs.SMALLEST, dtype="f8").want()
    assert cw[1].max() > 3 and hs.same_centred(cw, cw)
    import centred_util
    assert not hs.same_centred(centred_util.centred(x, t, row, col, bin, order="falling", **hs.CENTRED), cw)
    assert not hs.same_centred(centred_util.centred(x, t, row, col, bin, slice=4, **hs.CENTRED), cw)
    # the reader form also answers for the reader's calls: the carrying chunks, no other
    op = hs.centred(hs.SMALLEST, "cb", chunk_steps=3)
    c, pieces = hs.carrying_chunks(hs.SMALLEST, 3)
    calls = [(k * c, min(c, T - k * c)) for k, _ in pieces]
    w = op.want()
    assert op.same((w[0], w[1], calls), w) and not op.same((w[0], w[1], calls + [(T - 1, 1)]), w) and not op.same((w[0], w[1], [(0, T)]), w)
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
