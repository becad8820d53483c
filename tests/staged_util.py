"""The staged HIP path (ctk_shard_label2d -> ctk_debug_mask / ctk_debug_label2d -> ctk_shard_overlap -> ctk_shard_tables) against
the C oracle and tests/cpu_tables.py, exactly: the threshold mask, the scipy-numbered 2-D labels before and after the seam merge
(contrack.py:684-698), and the component / pair / seam tables."""
import numpy as np

import cpu_tables
from contrack_amd import _native


def staged(trk, anom, thr, op, wrow):
    T, ny, nx = anom.shape
    d = trk.malloc(anom.nbytes)
    try:
        trk.h2d(d, anom)
        trk.shard_label2d(d, T, ny, nx, thr, op, wrow, False)
        mask = trk.debug_mask(T, ny, nx)
        lab_nw = trk.debug_label2d(T, ny, nx, True)
        lab_m = trk.debug_label2d(T, ny, nx, False)
        trk.shard_overlap()
        blob = trk.shard_tables()
    finally:
        trk.free(d)
    return mask, lab_nw, lab_m, blob


def check_staged(trk, oracle, anom, thr, gorl, wrow, overlap, persistence, twosided):
    """runs the staged path on trk and asserts every stage output equal to the oracle's; returns the parsed tables"""
    mask, lab_nw, lab_m, blob = staged(trk, anom, thr, _native.CMP_OPS[gorl], wrow)
    omask = oracle.threshold_mask(anom, thr, gorl)
    assert np.array_equal(mask, omask)
    olab, _ = oracle.label(omask, 0)
    assert np.array_equal(lab_nw, olab)
    del olab
    _, _, stage = oracle.run_contrack(anom, thr, gorl, wrow, overlap, persistence, twosided, return_stage=True)
    assert np.array_equal(lab_m, stage)
    del stage
    wlo, whi, wshift, lb = _native.weights_to_limbs(wrow, npix=omask.shape[1] * omask.shape[2], with_bits=True)
    ref = cpu_tables.parse_blob(cpu_tables.pack_blob(cpu_tables.build_tables(omask.astype(bool), wlo, whi), wshift, False, limb_bits=lb))
    got = cpu_tables.parse_blob(blob)
    assert got["T"] == ref["T"] and got["wshift"] == ref["wshift"]
    assert np.array_equal(got["ncomp"], ref["ncomp"])
    assert np.array_equal(got["mrep"], ref["mrep"])
    assert np.array_equal(got["box"], ref["box"])
    assert np.array_equal(got["area"], ref["area"])
    assert got["pairs"] == ref["pairs"]
    assert got["seams"] == ref["seams"]
    return got
