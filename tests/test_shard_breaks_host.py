"""GPU-free: the label numbering across time-shard cuts when some cuts are segment breaks (boundary_resolve(..., breaks) in
csrc/ctk_seam.h through the ctk_debug_boundary_resolve_breaks hook).  A rank whose first step starts a segment labels its shard
without a halo; the records of all ranks must give scipy's raster ids of every segment labelled alone, shifted by the components of
the segments before it, and no set may count as crossing a break."""
import numpy as np
import pytest
from scipy import ndimage

from contrack_amd import _native
from test_shard_host import S3, _local_labelling


def _resolve_breaks(recs):
    world = len(recs)
    nlast = np.array([len(r[0]) for r in recs], dtype=np.int32)
    nh = np.array([len(r[1]) for r in recs], dtype=np.int32)
    nroots = np.array([r[2] for r in recs], dtype=np.int32)
    last = np.ascontiguousarray(np.array(sum((r[0] for r in recs), []) + [0], dtype=np.int32))
    halo = np.ascontiguousarray(np.array(sum((r[1] for r in recs), []) + [0], dtype=np.int32))
    off = np.zeros(world + 1, dtype=np.int64)
    ll, hl = np.zeros(len(last), dtype=np.int32), np.zeros(len(halo), dtype=np.int32)
    na, ncross = np.zeros(world, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _native.check(_native.lib().ctk_debug_boundary_resolve_breaks(world, nlast.ctypes.data, nh.ctypes.data, nroots.ctypes.data, last.ctypes.data,
                                                                  halo.ctypes.data, off.ctypes.data, ll.ctypes.data, hl.ctypes.data, na.ctypes.data,
                                                                  ncross.ctypes.data))
    return off, ll, hl, na, nlast, nh, int(ncross[0])


@pytest.mark.parametrize("seed", range(40))
def test_ids_with_breaks_on_cuts(seed):
    rng = np.random.default_rng(1000 + seed)
    T, ny, nx = int(rng.integers(3, 14)), int(rng.integers(3, 12)), int(rng.integers(3, 14))
    mask = rng.random((T, ny, nx)) < float(rng.choice([0.2, 0.35, 0.5]))
    if rng.random() < 0.5:
        mask = np.repeat(mask[::2], 2, axis=0)[:T]                    # blobs that live across cuts
    world = int(rng.integers(2, min(T, 6) + 1))
    cuts = [0] + sorted(rng.choice(np.arange(1, T), size=world - 1, replace=False).tolist()) + [T]
    is_break = [False] + [bool(rng.random() < 0.5) for _ in range(world - 1)]          # the cut in front of rank r
    if seed % 4 == 0:
        is_break = [False] + [True] * (world - 1)
    # expected: every segment labelled alone, ids shifted
    want = np.zeros(mask.shape, dtype=np.int64)
    nwant, seg_starts = 0, [cuts[r] for r in range(world) if r == 0 or is_break[r]] + [T]
    for a, b in zip(seg_starts[:-1], seg_starts[1:]):
        lab, n = ndimage.label(mask[a:b], structure=S3)
        want[a:b] = np.where(lab > 0, lab + nwant, 0)
        nwant += n
    # a rank behind a break sees no previous shard
    recs = [_local_labelling(mask[cuts[r]:], 0, cuts[r + 1] - cuts[r]) if is_break[r] else _local_labelling(mask, cuts[r], cuts[r + 1])
            for r in range(world)]
    off, ll, hl, na, nlast, nh, ncross = _resolve_breaks(recs)
    assert off[-1] == nwant
    lo, ho = np.concatenate([[0], np.cumsum(nlast)]), np.concatenate([[0], np.cumsum(nh)])
    crossing = set()
    for r in range(world):
        last, halo, nroots, labs, per_plane, nhr, rank_of = recs[r]
        assert (nhr == 0) == (r == 0 or is_break[r] or nlast[r - 1] == 0)
        hlab, llab = hl[ho[r]:ho[r + 1]], ll[lo[r]:lo[r + 1]]
        # the last step's labels are scipy's; labels of sets that reach a cut which is no break are the crossing ones
        lab_last = labs[-1]
        for c in range(len(last)):
            ids = np.unique(want[cuts[r + 1] - 1][lab_last == c + 1])
            assert ids.tolist() == [llab[c]]
        if r + 1 < world and not is_break[r + 1]:
            crossing.update(int(v) for v in llab)
        for h in range(nhr):
            assert hlab[h] == ll[lo[r - 1] + h]                        # halo component h is last-step component h of the rank before
    assert ncross == len(crossing)


def test_a_break_is_only_accepted_with_breaks():
    recs = [([0], [], 1), ([0], [], 1)]                                # rank 1 reports no halo although rank 0's last step has a component
    off, ll, hl, na, nlast, nh, ncross = _resolve_breaks(recs)
    assert off.tolist() == [0, 1, 2] and ll[:2].tolist() == [1, 2] and ncross == 0
    from test_shard_host import _resolve
    with pytest.raises(ValueError):
        _resolve(recs)
