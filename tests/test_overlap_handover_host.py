"""tests/handover_cases.py on the CPU: every slab takes the k_overlap instance it is meant for and holds what its case promises (words
with common pixels per wave and step, runs across word boundaries, pieces per word, distinct pairs), and the two CPU oracles agree on
it -- the C oracle labels it exactly as oracle/scipy_port.py, the reference's own call sequence, does."""
import numpy as np
import pytest

import handover_cases as hc
import label_forms as lf
from oracle import scipy_port

WANT_FORM = {(181, 360): (5, 256), (205, 320): (5, 256), (160, 512): (5, 256), (32, 128): (4, 256), (721, 1440): (4, 512),
             (192, 512): (6, 256), (224, 512): (8, 256), (128, 4096): (4, 512), (8, 64): (4, 128)}
SHORT = [s for s in hc.SHAPES if s[2] != hc.LONG_T]


def test_shapes_take_their_instances():
    for ny, nx, T in hc.SHAPES:
        assert hc.form_of(ny, nx, T) == WANT_FORM[(ny, nx)]
    assert lf.overlap_form(hc.LONG_T, 8, 1, False) == 41285 and lf.overlap_form(4, 181, 6, True) == 1052561


def test_every_case_on_every_shape_that_holds_it():
    names = {n for n, _, _ in hc.all_slabs()}
    for ny, nx, T in SHORT:
        for c in hc.CASES:
            held = "%dx%dx%d-%s" % (T, ny, nx, c) in names
            # 64 words of one wave's step outside trip 0 need a second trip inside the plane; 32 x 128 is one wave of 64 words
            assert held or (c == "n65" and ny * ((nx + 63) // 64) <= 64)
    _, long_names = hc.long_slab()
    assert set(long_names) == set(hc.CASES) - {"n64", "n65"}          # (8 words)


@pytest.mark.parametrize("shape", SHORT, ids=lambda s: "%dx%d" % s[:2])
def test_planes_hold_their_case(shape):
    ny, nx, T = shape
    ovb, th = hc.form_of(ny, nx, T)
    W = (nx + 63) // 64
    nw = ny * W
    P, C = hc.planes("none", ny, nx, T)
    assert P.any() and C.any() and len(hc.common_words(P, C)) == 0
    P, C = hc.planes("full", ny, nx, T)
    cw = hc.common_words(P, C)
    assert len(cw) == nw                                             # every word, the past-the-end words of the last step excluded
    counts = hc.per_wave_step(ny, nx, T, cw)
    if nw > th:
        assert max(counts.values()) > 64                             # more in a wave's step than its 64 lanes
    if (ny, nx) in ((181, 360), (205, 320)):
        assert nw % (ovb * th) != 0                                  # a last step with past-the-end words
    for case, n in (("n64", 64), ("n65", 65)):
        pc = hc.planes(case, ny, nx, T)
        if pc is None:
            continue
        counts = hc.per_wave_step(ny, nx, T, hc.common_words(*pc))
        assert list(counts.values()) == [n]                          # all in ONE wave's step
        if nw > 64:
            us = {hc.word_of(ny, nx, T, int(i))[1] for i in hc.common_words(*pc)}
            assert us == {0, 1}
    P, C = hc.planes("cross", ny, nx, T)
    cw = set(hc.common_words(P, C).tolist())
    seen = set()
    for y in range(ny):
        for k in range(1, W):
            b = 64 * k
            if b + 1 < nx and C[y, b] and P[y, b]:
                kind = (int(C[y, b - 1]), int(P[y, b - 1]))          # the run crosses the boundary in t / in t-1
                seen.add(kind)
                assert y * W + k in cw
                _, u, wave, lane = hc.word_of(ny, nx, T, y * W + k)
                seen.add(("lane0",) if lane == 0 else ("wave0", wave == 0, u))
    assert {(1, 0), (0, 1), (1, 1)} <= seen
    if 64 % W:                                                       # (W | 64: lane 0 holds the first word of a row, nothing to its left)
        assert ("lane0",) in seen
    assert any(C[y, 0] and P[y, 0] and C[y - 1, nx - 1] == 0 for y in range(1, ny))       # words that are first in their row
    for case in ("alt_under_full", "alt_both"):
        P, C = hc.planes(case, ny, nx, T)
        o = (P & C).astype(bool)
        y = int(np.nonzero(o.any(axis=1))[0][0])
        assert o[y, :64].sum() == 32 and not (o[y, :-1] & o[y, 1:]).any()      # 32 pieces in a word
        if ny * nx >= 181 * 360 and ny * W <= 4096:
            assert o.sum() > lf.CTK_HASH_SLOTS                       # more distinct pairs than the hash holds


@pytest.mark.parametrize("name,case,shape", [s for s in hc.all_slabs() if s[2][0] * s[2][1] <= 205 * 320 and s[2][2] <= 8],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_oracles_agree(name, case, shape, oracle_lib):
    mask = hc.build(case, shape)
    T, ny, nx = mask.shape
    anom = np.where(mask.astype(bool), np.float32(1.0), np.float32(-1.0))
    lat = np.linspace(90, -90, ny).astype(np.float32)
    w = oracle_lib.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    want = scipy_port.run_contrack(anom, 0.0, ">=", w, 0.5, 2, True)
    got = oracle_lib.run_contrack(anom, oracle_lib.prepare_thresholds(0.0, T), ">=", w, 0.5, 2, True)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
