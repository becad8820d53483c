"""Every write, extent, run-value, filter, rank and count form at both sides of its edges, exactly against the C oracle: the flags
and n_tracked of `track_dev` twice on one handle, of an output pointer 4 bytes off its alignment (the generic k_relabel), of `track`
with the dense result transfer, of `track_stream` and of a segmented call (the SEG builds, against tests/segment_util.expected).
The slabs come from tests/tail_forms.py, which restates the selection; after every call the statistics CTK_S_FILTER_FORMS,
CTK_S_EXTENT_FORM, CTK_S_RUNVAL_FORM, CTK_S_RELABEL_SHAPE and CTK_S_COUNT_FORM must name the forms the restatement predicts, so a
case that misses its form fails whatever its flags."""
import ctypes

import numpy as np
import pytest

import cpu_tables
import segment_util as su
import shard_inproc
import tail_forms as tf
from contrack_amd import _native, synth

pytestmark = pytest.mark.gpu

GORL, OVERLAP, TWOSIDED = ">=", 0.5, True
OP = _native.CMP_OPS[GORL]


@pytest.fixture(scope="module")
def n_cus():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    return device_cus()


def device_cus():
    """compute units of the handle's device (CTK_S_DEVICE_CUS, after a call): the k_rs_pass_blk_2pc edge depends on them"""
    a = np.ones((1, 4, 4), dtype=np.float32)
    with _native.Tracker(0) as trk:
        trk.track(a, np.zeros(1), OP, np.ones(4, dtype=np.float32), OVERLAP, 1, TWOSIDED)
        return trk.stats()["device_cus"]


def inputs(mask, oracle):
    """anomalies +-1 around a threshold of 0, the row weights of a regular grid pole to pole"""
    T, ny, nx = mask.shape
    anom = np.where(mask.astype(bool), np.float32(1.0), np.float32(-1.0))
    thr = oracle.prepare_thresholds(0.0, T)
    lat = np.linspace(90, -90, ny).astype(np.float32)
    w = oracle.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    return anom, thr, w


def small_threads(trk, extent=0, run_values=0):
    _native.check(_native.lib().ctk_debug_set_small_threads(trk.handle, extent, run_values, 0))


class Calls:
    """one handle, its restated state, and the checks after each call"""

    def __init__(self, trk, n_cus, anom, thr, w, persistence, want):
        self.trk, self.model = trk, tf.Handle(n_cus)
        self.anom, self.thr, self.w, self.pers = anom, thr, w, persistence
        self.T, self.ny, self.nx = anom.shape
        self.runs = int(tf.chunk_runs(anom > 0, 1).sum())
        self.want = want
        self.extent_forced = 0
        self.rv_forced = 0
        self.seen = []

    def check(self, pred, aligned=True, seg=False, blocks=None, fused=True):
        """the statistics of the last call against the restatement; pred: Handle.fused() before the call"""
        T, ny, nx = self.T, self.ny, self.nx
        st = self.trk.stats()
        cv = tf.chunk_copy(T, ny, nx, aligned)
        assert st["extent_form"] == tf.extent_form(T, nx, self.extent_forced)
        if fused:
            bits, cnt, NP = pred
            ff = st["filter_forms"] & 0xffff
            assert st["host_path"] == 0
            assert st["filter_forms"] >> 16 == NP                        # the passes the fused pass launched
            if st["fused_pass"] == 1:
                assert ff & ~tf.F_UNITE_ANY == bits, (ff, bits)
                assert bool(ff & tf.F_UNITE_ANY) == self.model.unite_needed(T)
                assert ff & tf.F_UNITE_ANY != tf.F_UNITE_ANY
                assert st["count_form"] == cnt
                assert st["runval_form"] == tf.runval_form(T, self.runs, True, cv, self.rv_forced)
            else:
                sync = (tf.F_SYNC_SEG if seg else tf.F_SYNC) if T > 2 else 0
                assert ff & ~(tf.F_UNITE_ANY | tf.F_RANK_MERGED | tf.F_RANK_SPLIT) == (bits & ~(tf.F_RANK_MERGED | tf.F_RANK_SPLIT)) | sync
                assert ff & tf.F_UNITE
                assert st["count_form"] == cnt | tf.write_count(st["labels_3d"])
                assert st["runval_form"] == tf.runval_form(T, self.runs, False, cv)
            self.model.after(st, NP)
        blocks = blocks or [(0, T)]
        forms = [tf.write_form(T, ny, nx, aligned, nt) for _, nt in blocks]
        assert st["relabel_kernel"] == forms[-1]["kernel"]
        assert st["relabel_shape"] == tf.relabel_shape(forms), (hex(st["relabel_shape"]), hex(tf.relabel_shape(forms)))
        self.seen.append(st)
        return st

    def check_sync(self, seg=False):
        """a call with the fused pass switched off: the synchronous resolver's k_rs_pass, k_rs_unite, ctk_shard_write"""
        st = self.check(None, fused=False)
        T = self.T
        assert st["fused_pass"] == 0 and st["host_path"] == 0
        assert st["filter_forms"] == ((tf.F_SYNC_SEG if seg else tf.F_SYNC) if T > 2 else 0) | tf.F_UNITE
        assert st["count_form"] == tf.write_count(st["labels_3d"])
        assert st["runval_form"] == tf.runval_form(T, self.runs, False, tf.chunk_copy(T, self.ny, self.nx))
        assert st["filter_rounds"] == (st["filter_passes"] + tf.CTK_JACOBI_ROUND - 1) // tf.CTK_JACOBI_ROUND
        return st

    def _eq(self, got, n):
        want, nw = self.want
        assert np.array_equal(got, want), "flag differs at %d pixels" % int((got != want).sum())
        assert n == nw, (n, nw)

    def track_dev(self, times=2, offset=0):
        trk, anom = self.trk, self.anom
        T, ny, nx = anom.shape
        d_in, d_out = trk.malloc(anom.nbytes), trk.malloc(anom.size * 4 + 16)
        sts = []
        try:
            trk.h2d(d_in, anom)
            for _ in range(times):
                trk.memset(d_out, 0xff, anom.size * 4 + 16)
                pred = self.model.fused(T, self.runs)
                dst = ctypes.c_void_p(d_out.value + offset)
                n = trk.track_dev(d_in, T, ny, nx, self.thr, OP, self.w, OVERLAP, self.pers, TWOSIDED, dst)
                out = np.empty(anom.shape, dtype=np.int32)
                trk.d2h(out, dst)
                self._eq(out, n)
                sts.append(self.check(pred, aligned=offset % 16 == 0))
        finally:
            trk.free(d_in)
            trk.free(d_out)
        return sts

    def track_dense(self):
        self.trk.set_result_transfer(0)
        try:
            pred = self.model.fused(self.T, self.runs)
            got, n = self.trk.track(self.anom, self.thr, OP, self.w, OVERLAP, self.pers, TWOSIDED)
            self._eq(got, n)
            return self.check(pred)
        finally:
            self.trk.set_result_transfer(-1)

    def track_stream(self, chunk):
        parts = {}
        _, n = self.trk.track_stream(self.anom, self.thr, OP, self.w, OVERLAP, self.pers, TWOSIDED,
                                     sink=lambda t0, nt, v: parts.__setitem__(t0, v.copy()), chunk_steps=chunk)
        got = np.concatenate([parts[k] for k in sorted(parts)], axis=0)
        self._eq(got, n)
        # (a streamed pass is never fused: the synchronous resolver and ctk_shard_write, one write launch per block)
        st = self.check(None, blocks=tf.stream_blocks(self.T, chunk), fused=False)
        assert st["runval_form"] == tf.runval_form(self.T, self.runs, False, tf.chunk_copy(self.T, self.ny, self.nx))
        assert st["count_form"] == tf.write_count(st["labels_3d"])
        return st

    def segmented(self, starts, fused=True):
        want, nw = su.expected(self.anom, self.thr, GORL, self.w, OVERLAP, self.pers, TWOSIDED, starts)
        self.trk.set_segments(starts)
        self.trk.set_result_transfer(0)
        try:
            pred = self.model.fused(self.T, self.runs, seg=True)
            got, n = self.trk.track(self.anom, self.thr, OP, self.w, OVERLAP, self.pers, TWOSIDED)
            assert np.array_equal(got, want), "segmented flag differs at %d pixels" % int((got != want).sum())
            assert n == nw
            return self.check(pred, seg=True) if fused else self.check_sync(seg=True)
        finally:
            self.trk.set_result_transfer(-1)
            self.trk.clear_segments()


def _want(oracle, anom, thr, w, pers):
    return oracle.run_contrack(anom, thr, GORL, w, OVERLAP, pers, TWOSIDED)


WRITE = [c for c in tf.CASES if c["name"].startswith(("v5_", "v4_", "generic_", "full_", "filtered_"))]


@pytest.mark.parametrize("case", WRITE, ids=lambda c: c["name"])
def test_write_case(case, oracle_lib, n_cus):
    mask = tf.mask_of(case)
    anom, thr, w = inputs(mask, oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    if mask.all():
        assert want[1] == 0 and len(np.unique(want[0])) == 1                 # (one id, or none: no background either way)
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, case["persistence"], want)
        c.track_dev()
        c.track_dev(times=1, offset=4)                                      # the generic kernel
        c.track_dense()
        c.track_stream(4)                                                   # blocks of 4 and 2 steps
        if case["name"].startswith(("v5_", "v4_")):
            c.segmented(np.array([0, 3]))
            for ex in (64, 128, 256, 1024):                                 # every k_extent form on the same tables
                small_threads(trk, extent=ex)
                c.extent_forced = ex
                c.track_dev(times=1)
            small_threads(trk)
            c.extent_forced = 0
    kernels = {s["relabel_kernel"] for s in c.seen}
    assert kernels >= {0, tf.write_form(case["T"], case["ny"], case["nx"])["kernel"]}


@pytest.mark.parametrize("ny,nx", [(91, 4608), (91, 4416), (91, 4612)])
def test_fold_case(ny, nx, oracle_lib, n_cus):
    """complex components (seam operations folded pixel by pixel) through k_relabel_v4 (4608), v5 (4416, one-row chunks) and the
    generic kernel (4612 through the offset pointer; v4 aligned)"""
    T = 8
    anom = synth.smooth_field(T, ny, nx, seed=3)
    lat, _ = synth.grid(ny, nx)
    w = oracle_lib.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    thr = oracle_lib.prepare_thresholds(120.0, T)
    want = _want(oracle_lib, anom, thr, w, 3)
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, 3, want)
        c.runs = int(tf.chunk_runs(anom >= 120.0, 1).sum())
        sts = c.track_dev()
        assert all(s["seam_ops"] > 0 for s in sts)
        c.track_dev(times=1, offset=4)
        c.track_dense()
    assert tf.write_form(T, ny, nx)["kernel"] == (5 if nx == 4416 else 4)


ALIVE = [c for c in tf.CASES if c["name"].startswith("alive")]


@pytest.mark.parametrize("case", ALIVE, ids=lambda c: c["name"])
def test_alive_count(case, oracle_lib, n_cus):
    """ids per k_run_values workgroup on both sides of the thread count (the alive count that becomes n_tracked)"""
    anom, thr, w = inputs(tf.mask_of(case), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, case["persistence"], want)
        for th in case["rv_threads"]:
            small_threads(trk, run_values=th)
            c.rv_forced = th
            for s in c.track_dev():
                assert s["labels_3d"] == case["nlab"] and s["fused_pass"] == 1


RANK = [c for c in tf.CASES if c["name"].startswith("rank_")]


@pytest.mark.parametrize("case", RANK, ids=lambda c: c["name"])
def test_rank_forms(case, oracle_lib, n_cus):
    """8192 / 8193 rank blocks: one merged launch or k_rs_rank + k_rs_labels + k_fz_mark; more than 10^6 ids, so the second call
    on the handle counts with the full k_count_alive; then a small slab on the same handle does too, and the one after it not"""
    anom, thr, w = inputs(tf.mask_of(case), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, case["persistence"], want)
        sts = c.track_dev()
        assert all(s["fused_pass"] == 1 and s["labels_3d"] == case["nlab"] and s["runs"] == case["nlab"] for s in sts)
        assert sts[0]["count_form"] == tf.C_F and sts[1]["count_form"] == tf.C_FULL
        small = tf.CASE_BY_NAME["v5_runs_181x360"]
        a2, t2, w2 = inputs(tf.mask_of(small), oracle_lib)
        c2 = Calls(trk, n_cus, a2, t2, w2, small["persistence"], _want(oracle_lib, a2, t2, w2, small["persistence"]))
        c2.model = c.model
        s2 = c2.track_dev()
        assert s2[0]["count_form"] == tf.C_FULL and s2[1]["count_form"] == tf.C_F


STAGED = [c for c in tf.CASES if c.get("staged")]


@pytest.mark.parametrize("case", STAGED, ids=lambda c: c["name"])
def test_shard_write_count(case, oracle_lib, n_cus):
    """262 144 / 262 145 ids through ctk_shard_extents / ctk_shard_write (host resolver): k_count_alive_1 or k_count_alive"""
    anom, thr, w = inputs(tf.mask_of(case), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    with _native.Tracker(0) as trk:
        flag, n, info = shard_inproc.sharded([trk], anom, thr, OP, w, OVERLAP, case["persistence"], TWOSIDED, [0, anom.shape[0]])
        st = trk.stats()
    assert np.array_equal(flag, want[0]) and n == want[1]
    assert st["count_form"] == tf.write_count(case["nlab"])
    assert st["runval_form"] == tf.runval_form(anom.shape[0], 0, False, tf.chunk_copy(*anom.shape))


def test_cascade(oracle_lib, n_cus):
    """a removal cascade of 35 Jacobi passes.  The first fused pass launches 24 (k_rs_pass_blk), does not converge and the synchronous
    resolver repeats the resolution in rounds of 10 per-pass k_rs_pass; the next call launches 48 per-pass k_rs_pass (NP > 32:
    k_count_alive_1), the one after max(10, reported + 2).  The launched counts are exact (CTK_S_FILTER_FORMS >> 16).  The reported
    pass count is that of the Jacobi iteration or, where a pass of the in-place kernel read a predecessor's bits of the same pass
    (a race of the first pass only: later passes evaluate a step only if its predecessor changed in the pass before), one less.
    A call with a pair table too small for the per-step slots unites with k_rs_unite instead of k_rs_unite_slots."""
    case = tf.CASE_BY_NAME["cascade"]
    mask = tf.mask_of(case)
    anom, thr, w = inputs(mask, oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    tb = cpu_tables.build_tables(mask.astype(bool), np.ones(case["ny"], np.int64), np.zeros(case["ny"], np.int64))
    jac = tf.jacobi_passes(tb)
    assert jac == case["cascade"]
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, case["persistence"], want)
        sts = c.track_dev(times=3)
        assert [s["filter_forms"] >> 16 for s in sts] == [24, 48, max(10, sts[1]["filter_passes"] + 2)]
        assert sts[0]["fused_pass"] == 0 and sts[0]["off_fused_path_reason"] & 64 and sts[0]["filter_forms"] & tf.F_BLK
        assert sts[0]["filter_forms"] & tf.F_SYNC and sts[0]["filter_rounds"] == (sts[0]["filter_passes"] + 9) // 10
        assert sts[1]["fused_pass"] == 1 and sts[1]["filter_forms"] & tf.F_PASS and sts[1]["count_form"] == tf.C_1
        assert sts[2]["fused_pass"] == 1 and sts[2]["filter_forms"] & tf.F_PASS and sts[2]["count_form"] == tf.C_1
        assert all(jac - 1 <= s["filter_passes"] <= jac for s in sts), [s["filter_passes"] for s in sts]
        unions = {s["filter_forms"] & tf.F_UNITE_ANY for s in sts[1:]}
        trk.debug_set_pair_capacity(case["T"] * 128 + 4095)          # (one call: the slots no longer fit beside the records)
        st = c.track_dev(times=1)[0]
        assert st["fused_pass"] == 1 and st["filter_forms"] & tf.F_UNITE_ANY == tf.F_UNITE
        unions.add(tf.F_UNITE)
        assert unions == {tf.F_UNITE_SLOTS, tf.F_UNITE}, unions
        c.track_dense()
        st = c.segmented(np.array([0, 17]))
        assert st["filter_forms"] & tf.F_PASS_SEG


def test_filter_edges(oracle_lib, n_cus):
    """timesteps of 64 / 65, 128 / 129 and 512 / 513 components and pairs, and of at most 128 components behind a predecessor of
    more, inside a k_rs_pass_blk workgroup and across one (tests/tail_forms.py FILTER_EDGES): the bars at those steps live or go by
    the predecessor's keep bits.  Through k_rs_pass_blk (fused), its SEG build, and k_rs_pass (synchronous resolver) and its SEG
    build."""
    case = tf.CASE_BY_NAME["filter_edges"]
    anom, thr, w = inputs(tf.mask_of(case), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, case["persistence"])
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, case["persistence"], want)
        sts = c.track_dev()
        assert all(s["fused_pass"] == 1 and s["filter_forms"] & tf.F_BLK for s in sts)
        c.segmented(np.array([0, 20]))
        trk.set_fused(False)
        try:
            d_in, d_out = trk.malloc(anom.nbytes), trk.malloc(anom.size * 4)
            try:
                trk.h2d(d_in, anom)
                n = trk.track_dev(d_in, *anom.shape, thr, OP, w, OVERLAP, case["persistence"], TWOSIDED, d_out)
                out = np.empty(anom.shape, dtype=np.int32)
                trk.d2h(out, d_out)
                c._eq(out, n)
                c.check_sync()
            finally:
                trk.free(d_in)
                trk.free(d_out)
            c.segmented(np.array([0, 20]), fused=False)
        finally:
            trk.set_fused(True)
