"""tests/anom_forms.py against the library on the host (no GPU): its restatement of ctk_anom_plan against ctk_debug_anom_plan over a
sweep, the invariants every plan must keep, the streamed launch prediction against the entry's own loop bounds, its models against
oracle/anom_port.py, and the conditions under which the cases of tests/test_gpu_anom_seg_forms.py can tell a wrong kernel from a right
one."""
import numpy as np
import pytest

from contrack_amd import _native
from oracle import anom_port

import anom_forms as af

NPIX = (1, 63, 64, 65, 255, 256, 257)
OVERRIDES = ((0, 0), (1, 0), (3, 0), (40, 0), (1 << 40, 0), (0, 1), (0, 3), (0, 7), (5, 3), (0, 65535), (0, 1 << 20))


def _nts(tile):
    return {n for k in (1, 2, 3) for n in (k * tile - 1, k * tile, k * tile + 1) if n >= 1}


def _check(elem, smooth, nt, npix, ww, gm):
    got = _native.anom_plan(elem, smooth, nt, npix, ww, gm)
    want = af.plan(elem, smooth, nt, npix, ww, gm)
    case = (elem, smooth, nt, npix, ww, gm)
    assert got == want, (case, got, want)
    cap = min(gm, 65535) if gm > 0 else 65535
    tile, gy = got["tile"], got["gy"]
    assert gy * tile >= nt and (gy - 1) * tile < nt and 1 <= gy <= cap, (case, got)
    assert (got["form"] == af.RING) == (smooth * 256 * elem <= 32768), (case, got)
    assert got["gx"] == -(-npix // 256), (case, got)
    if got["form"] == af.PLAIN:
        assert got["lds"] == 0 and tile == max(32, -(-nt // cap)), (case, got)
    else:
        assert got["lds"] == smooth * 256 * elem <= 32768, (case, got)
        assert max(32, 8 * (smooth - 1)) <= tile <= max(256, -(-nt // cap)), (case, got)
    return tile


def test_plan_restatement_and_invariants():
    seen = set()
    for elem in (4, 8):
        for smooth in range(1, 41):
            for npix in NPIX:
                for ww, gm in OVERRIDES:
                    tiles = {32, 256, max(32, 8 * (smooth - 1))}
                    done = set()
                    while tiles - done:                               # nt around every multiple of every tile the sweep produces
                        t = (tiles - done).pop()
                        done.add(t)
                        for nt in _nts(t):
                            tiles.add(_check(elem, smooth, nt, npix, ww, gm))
                        if len(done) > 12:
                            break
                    seen |= done
    assert {32, 33, 256} <= seen and any(t % 8 for t in seen if 100 < t < 256), sorted(seen)[:40]


def test_the_rules_own_terms():
    """the three parts of the rule no small slab reaches: the waves term, the clamp, gridDim.y"""
    assert _native.anom_plan(4, 2, 2707, 181 * 360) == af.plan(4, 2, 2707, 181 * 360)
    assert af.plan(4, 2, 2707, 181 * 360)["tile"] == 2707 * 1019 // 16384 == 168            # the waves term, no multiple of 8
    assert af.plan(4, 2, 14600, 721 * 1440)["tile"] == 256                                  # the clamp
    nt = 65535 * 32 + 1
    for smooth, tile in ((2, 127), (33, 33)):
        p = _native.anom_plan(4, smooth, nt, 1)
        assert p == af.plan(4, smooth, nt, 1) and p["tile"] == tile and p["gy"] == -(-nt // tile) <= 65535, p
    p = _native.anom_plan(4, 33, 65535 * 32, 1)
    assert p["tile"] == 32 and p["gy"] == 65535                                               # the last length the plain tile of 32 takes
    p = _native.anom_plan(8, 17, 0x7fffffff, 1)
    assert p == af.plan(8, 17, 0x7fffffff, 1) and p["gy"] <= 65535


def test_plan_refuses_bad_arguments():
    for bad in ((2, 1, 1, 1, 0, 0), (4, 0, 1, 1, 0, 0), (4, 1, 0, 1, 0, 0), (4, 1, 1, 0, 0, 0), (4, 1, 1, 1, -1, 0), (4, 1, 1, 1, 0, -1)):
        with pytest.raises(ValueError):
            _native.anom_plan(*bad)


def test_stream_launches_cover_every_step_once():
    for T in (1, 2, 50, 150):
        for smooth in (1, 2, 5, 16, 17, 33):
            for chunk in (1, 2, smooth - 1, smooth, 31, 32, 33, 67, T, T + 5):
                if chunk < 1:
                    continue
                ls = af.stream_launches(T, smooth, chunk)
                assert ls[0][0] == 0 and ls[-1][1] == T and all(a[1] == b[0] for a, b in zip(ls[:-1], ls[1:])) and all(o1 > o0 for o0, o1 in ls)
                c = af.stream_chunk(T, smooth, chunk)
                assert all(o1 - o0 <= c + smooth for o0, o1 in ls), (T, smooth, chunk)                     # (the output buffer's steps)
                # a chunk holds at least smooth - 1 steps, more than the (smooth - 1) // 2 the output lags by: every chunk completes a step
                assert len(ls) == -(-T // c), (T, smooth, chunk)


# ---- the models are the port as they stand, and the slabs tell their wrong versions from it --------------------------------------
@pytest.mark.parametrize("dtype,smooth", af.RING_EDGE, ids=lambda v: getattr(v, "__name__", str(v)))
def test_ring_edge_slabs_discriminate(dtype, smooth):
    x, group, G, starts = af.ring_edge_case(dtype, smooth)
    want, clim = af.expected(x, group, G, 4, smooth, starts)
    assert af.same(af.anom_model(x, group, clim, smooth, starts), want)
    af.assert_discriminates(x, group, G, 4, smooth, starts)
    T = x.shape[0]
    edges = starts + [T]
    lens = [e - s for s, e in zip(edges[:-1], edges[1:])]
    assert smooth - 1 in lens and smooth in lens and starts[1] == 1 and starts[-1] == T - 1
    finite = np.isfinite(want).any(axis=(1, 2))
    k = lens.index(smooth)
    assert finite[starts[k]:edges[k + 1]].sum() == 1                     # the segment of exactly `smooth` steps: one output
    k = lens.index(smooth - 1)
    assert not finite[starts[k]:edges[k + 1]].any()


@pytest.mark.parametrize("case", af.TILE_EDGE, ids=lambda c: "%s-smooth%d-tile%d" % (c[0].__name__, c[1], c[2]))
def test_tile_edge_cases_reach_their_tile_and_discriminate(case):
    dtype, smooth, tile = case
    elem = np.dtype(dtype).itemsize
    for nt in (2 * tile - 1, 2 * tile, 2 * tile + 1):
        ov = af.overrides_for_tile(elem, smooth, nt, 130, tile)
        assert ov is not None, (case, nt)
        p = _native.anom_plan(elem, smooth, nt, 130, *ov)
        assert p["tile"] == tile and p["form"] == af.RING and p["gy"] == (3 if nt > 2 * tile else 2), (case, nt, p)
        for brk in (tile - 1, tile, tile + 1):
            x, group, G, starts = af.tile_edge_case(dtype, smooth, tile, nt, brk)
            af.assert_discriminates(x, group, G, 4, smooth, starts)
            want, _ = af.expected(x, group, G, 4, smooth, starts)
            ok = np.isfinite(want).any(axis=(1, 2))
            # blockIdx.y * tile: the workgroups behind the first have outputs that are numbers, and they are not the first tile's
            assert ok[tile:].any() and not af.same(want[tile:2 * tile][:nt - tile], want[:tile][:nt - tile]), (case, nt, brk)


@pytest.mark.parametrize("G", af.CLIM_G)
def test_clim_cases_discriminate(G):
    """every float64 case tells falling t from rising t; the accumulate model is the port as it stands, and where two groups of one
    stripe alternate inside a chunk, dropping the flush or a wrong stripe modulus changes the climatology"""
    for case in af.clim_cases():
        if case[0] != G:
            continue
        _, rule, chunk, window, shape, T = case
        x, group = af.clim_case(np.float64, case)
        with np.errstate(invalid="ignore"):
            want = anom_port.calc_clim(x, group, G, window).astype(np.float64)
        assert af.differ_finite(af.clim_reversed(x, group, G, window), want), case
        if rule == "alternating" and shape == af.CLIM_SHAPES[0] or rule == "shuffled" and G in (33, 65):
            assert af.same(af.clim_acc_model(x, group, G, window, chunk), want), case
            a, b = af.alternating_pair(G)
            if rule == "alternating" and G > 32 and chunk > 2:
                assert a % 32 == b % 32
                assert not af.same(af.clim_acc_model(x, group, G, window, chunk, flush=False), want), case
            if G > 32:
                assert not af.same(af.clim_acc_model(x, group, G, window, chunk, modulus=64), want), case
