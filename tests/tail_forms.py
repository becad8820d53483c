"""Which filter, rank, extent, run-value, write and count kernel forms a call launches: a restatement of the rules in
contrack_amd/csrc/ctk_forms.h (ctk_write_rows, ctk_write_tables_lds, ctk_write_plan with the k_relabel_v5 image / budget / tab_batched
choice, ctk_write_chunk_copy, ctk_extent_form, ctk_runval_threads for the staged, fused and time-sharded path, ctk_count_form_staged,
ctk_count_form_fused, ctk_filter_plan_fused for the filter passes, union and rank form of the fused pass, ctk_filter_bits_sync for the
synchronous resolver), of the handle's pass count in resolve_async (contrack_amd/csrc/ctk_api.hip) and of the kernels' own edges in
contrack_amd/csrc/ctk_kernels.hip (k_run_values' alive count, the chunk copy and the staged run values of k_relabel_v4 and
relabel_v5_body, the valid bits of a row's last word) and ctk_resolve_dev.hip (k_rs_pass' CTK_PASS_COMPS, k_rs_pass_blk's LDS edges
PB_COMPS).  Host-only.  Kept in step with the C++ by tests/test_tail_forms.py, which compares it with the library itself
(ctk_debug_forms), and, on the GPU, by the statistics CTK_S_FILTER_FORMS, CTK_S_EXTENT_FORM, CTK_S_RUNVAL_FORM, CTK_S_RELABEL_SHAPE and CTK_S_COUNT_FORM
that tests/test_gpu_tail_forms*.py assert.

It also builds the slabs that land on the edges: planes with a prescribed number of runs in every write chunk, dot lattices with
a prescribed number of 3-D ids, and a removal cascade of a prescribed length."""
import numpy as np

CTK_CV = 64                      # ctk_device.h: run values per chunk in the chunk-ordered copy
CTK_CV_MAXCHUNK = 1024           # chunks per timestep the copy is built for
RV5 = 512                        # run values k_relabel_v5 stages in LDS
RVCAP = 2048                     # ... k_relabel_v4
CTK_RL_BLOCKS = 8192             # ctk_device.h: rank blocks of 256 runs the merged rank launch takes
PB_G = 16                        # timesteps per k_rs_pass_blk workgroup
PB_COMPS = 128                   # components / pairs of a timestep whose sums live in LDS in k_rs_pass_blk
CTK_PASS_COMPS = 512             # ... in k_rs_pass
CTK_JACOBI_ROUND = 10
CTK_MAX_JACOBI = 240
EXTENT_BLK = 1024                # CTK_S_EXTENT_FORM of k_extent_blk
MAX_SHARD_T = 4000000            # label2d_begin (ctk_api.hip): timesteps a shard may hold

# CTK_S_FILTER_FORMS bits
F_BLK, F_BLK_SEG, F_2PC, F_2PC_SEG, F_PASS, F_PASS_SEG, F_SYNC, F_SYNC_SEG, F_UNITE_SLOTS, F_UNITE, F_RANK_MERGED, F_RANK_SPLIT = \
    (1 << i for i in range(12))
F_UNITE_ANY = F_UNITE_SLOTS | F_UNITE
# CTK_S_COUNT_FORM bits
C_F, C_1, C_FULL, W_1, W_FULL = 1, 2, 4, 8, 16
# CTK_S_RELABEL_SHAPE flags
R_BATCHED, R_LOOPS, R_KB20, R_KB24, R_KB28 = 1, 2, 4, 8, 16


def _a8(n):
    return (n + 7) & ~7


def _a16(n):
    return (n + 15) & ~15


def relabel_rows(T, ny, nx):
    """rows per write chunk: ctk_write_rows (ctk_forms.h)"""
    n4r = max(1, nx // 4)
    rb = min(ny, max(1, min(64, 1024 // n4r)))
    store_cap = 2304 if n4r >= 256 else 6912
    rb_max = min(ny, max(rb, min(96, store_cap // n4r)))
    while rb < rb_max and T * ((ny + rb - 1) // rb) > 130000:
        rb += 1
    while rb < ny and T * ((ny + rb - 1) // rb) >= (1 << 24):
        rb += 1
    return rb


def _tables(rb, W):
    return rb * W * 8 + _a8(rb * W * 2) + _a8((rb + 1) * 4)


def _fast(nt, ny, nx, rb, aligned):
    """the word-sliced kernels may run: the test of ctk_write_plan (ctk_forms.h; for the chunk copy with the whole shard's T)"""
    W = (nx + 63) // 64
    nchunk = (ny + rb - 1) // rb
    return (nx % 4 == 0 and aligned and ny * nx < 0x7fffffff and nt * nchunk < (1 << 24) and nt > 0
            and _tables(rb, W) + RVCAP * 4 <= 60 * 1024)


def chunk_copy(T, ny, nx, aligned=True):
    """k_run_values builds the chunk-ordered copy (ctk_write_chunk_copy in ctk_forms.h; chunk_vals_for: not for run-table results)"""
    rb = relabel_rows(T, ny, nx)
    return _fast(T, ny, nx, rb, aligned) and (ny + rb - 1) // rb <= CTK_CV_MAXCHUNK


def write_form(T, ny, nx, aligned=True, nt=None):
    """the launch_relabel of timesteps [t0, t0 + nt) of a T-step shard: dict(kernel=5 | 4 | 0 | None, rb, sub, kb, batched)"""
    nt = T if nt is None else nt
    rb = relabel_rows(T, ny, nx)
    W = (nx + 63) // 64
    nchunk = (ny + rb - 1) // rb
    if not _fast(nt, ny, nx, rb, aligned):
        return dict(kernel=0 if nt > 0 else None, rb=rb, sub=0, kb=0, batched=False)
    tab5 = _tables(rb, W) + _a16(RV5 * 4) + 16

    def rows_per_image(bud):
        q = rb
        while q > 1 and tab5 + q * nx * 4 > bud:
            q -= 1
        return q
    kb = 20
    sub = rows_per_image(kb * 1024)
    if (rb + sub - 1) // sub > 2:
        for k2 in (24, 28):
            s2 = rows_per_image(k2 * 1024)
            if (rb + s2 - 1) // s2 <= 2:
                kb, sub = k2, s2
                break
    if tab5 + sub * nx * 4 <= kb * 1024:
        return dict(kernel=5, rb=rb, sub=sub, kb=kb, batched=nt * nchunk < 200000)
    return dict(kernel=4, rb=rb, sub=0, kb=0, batched=False)


def relabel_shape(forms):
    """CTK_S_RELABEL_SHAPE of a call whose write launches had these write_form()s"""
    v = 0
    for f in forms:
        if f["kernel"] == 5:
            v |= (f["rb"] << 24) | (f["sub"] << 8) | (R_BATCHED if f["batched"] else R_LOOPS) | {20: R_KB20, 24: R_KB24, 28: R_KB28}[f["kb"]]
        elif f["kernel"] == 4:
            v |= f["rb"] << 24
    return v


def stream_blocks(T, chunk):
    return [(t0, min(chunk, T - t0)) for t0 in range(0, T, chunk)]


def extent_form(T, nx, forced=0):
    """CTK_S_EXTENT_FORM (launch_extents: ctk_extent_form in ctk_forms.h); forced: ctk_debug_set_small_threads' extent"""
    if forced == 1024 or (forced == 0 and T > 2048 and nx < 1024):
        return EXTENT_BLK
    if forced:
        return forced
    return (128 if nx >= 1024 else 64) if T > 2048 else 256


def runval_threads(T, runs, fused, forced=0):
    """k_run_values' threads: 256 in ctk_shard_write; in the fused pass 64 for long shards of few runs per plane"""
    if not fused:
        return 256
    if forced:
        return forced
    return 64 if (T > 65536 and runs // T < 1024) else 256


def runval_form(T, runs, fused, cv, forced=0):
    return runval_threads(T, runs, fused, forced) * 10 + (1 if cv else 0)


def alive_form(T, nlab, threads):
    """k_run_values' alive count (fused pass): one id per thread and __syncthreads_count, or several and an LDS sum"""
    per = (nlab + T - 1) // T
    return "alive:count" if per <= threads else "alive:sum"


def chunk_runs(mask, rb):
    """runs of every write chunk: (T, nchunk) int64 (no wrap: a run ends at x = nx - 1)"""
    m = np.asarray(mask, dtype=bool)
    T, ny, nx = m.shape
    st = m & ~np.concatenate([np.zeros((T, ny, 1), dtype=bool), m[:, :, :-1]], axis=2)
    per_row = st.sum(axis=2)
    nchunk = (ny + rb - 1) // rb
    pad = np.zeros((T, nchunk * rb), dtype=np.int64)
    pad[:, :ny] = per_row
    return pad.reshape(T, nchunk, rb).sum(axis=2)


def chunk_value_forms(kernel, cv, runs):
    """where the write kernel takes a chunk's run values from (k_relabel_v4, relabel_v5_body in ctk_kernels.hip)"""
    out = set()
    cap = RV5 if kernel == 5 else RVCAP
    name = "v5" if kernel == 5 else "v4"
    for n in np.unique(runs).tolist():
        if n == 0:
            continue
        if cv and n <= CTK_CV:
            out.add(name + ":copy")
        else:
            out.add(name + (":staged" if n <= cap else ":unstaged"))
    return out


class Handle:
    """the resolver state of one ctk_handle the fused pass reads (async_passes, last_nlab, no_sys: resolve_async in ctk_api.hip, which hands
    them to ctk_filter_plan_fused and ctk_count_form_fused and updates them from the pass' mail) and the forms a one-call track launches"""

    def __init__(self, n_cus):
        self.n_cus = n_cus
        self.async_passes = 24
        self.last_nlab = 0

    def fused(self, T, runs, seg=False):
        """(CTK_S_FILTER_FORMS bits without the union kernel, CTK_S_COUNT_FORM bit, NP) of the fused pass"""
        sys = self.async_passes <= 24
        NP = min(max(self.async_passes, 2), 24 if sys else CTK_MAX_JACOBI) if T > 2 else 0
        bits = 0
        if sys and NP > 0:
            nb = (T - 1 + PB_G - 1) // PB_G
            bits |= (F_2PC if nb > self.n_cus else F_BLK) << (1 if seg else 0)
        if not sys and NP > 0:
            bits |= F_PASS_SEG if seg else F_PASS
        nsb = (max(runs, 1) + 255) // 256
        bits |= F_RANK_MERGED if nsb <= CTK_RL_BLOCKS else F_RANK_SPLIT
        if self.last_nlab <= 1000000 and NP <= 32:
            cnt = C_F
        elif self.last_nlab <= 1000000:
            cnt = C_1
        else:
            cnt = C_FULL
        return bits, cnt, NP

    def unite_needed(self, T):
        """a union kernel runs behind the passes (k_rs_pass_blk unites itself)"""
        sys = self.async_passes <= 24
        return not (sys and T > 2)

    def after(self, st, NP):
        """the handle's state after a one-call track with these statistics"""
        if st["fused_pass"] == 1:
            if NP > 0:
                self.async_passes = max(CTK_JACOBI_ROUND, st["filter_passes"] + 2)
            self.last_nlab = st["labels_3d"]
        elif st["off_fused_path_reason"] & 64:
            self.async_passes = min(CTK_MAX_JACOBI, NP * 2)


def write_count(n_labels):
    """ctk_shard_write's alive count: ctk_count_form_staged (ctk_forms.h)"""
    return W_1 if n_labels <= 262144 else W_FULL


# ---------------------------------------------------------------------------------------------------------------------------
# the overlap filter, restated: the number of passes a Jacobi iteration of keep[t] = f(keep[t-1]) needs over cpu_tables' tables
# ---------------------------------------------------------------------------------------------------------------------------
def jacobi_passes(tb, overlap=0.5, twosided=True, seg_edge=None, limb_bits=31):
    """passes of the Jacobi iteration until one changes nothing, that one included -- what CTK_S_FILTER_PASSES reports for an
    iteration that reads only the previous pass' bits (k_rs_pass_blk's iteration k reads its predecessor's bits of iteration k - 1;
    a pass of the in-place kernels may read newer ones and finish sooner, never later).  Components only (no seam merges: the
    cases that use it have none); areas are int64 limb sums, exact in float64 for the grids used."""
    ncomp = np.asarray(tb["ncomp"], dtype=np.int64)
    T = len(ncomp)
    off = np.concatenate([[0], np.cumsum(ncomp)])
    area = np.array([lo + hi * 2.0 ** limb_bits for lo, hi in tb["area"]], dtype=np.float64)
    pairs = [(t, c, d, lo + hi * 2.0 ** limb_bits) for t, c, d, lo, hi in tb["pairs"]]
    fwd = np.zeros(off[-1])
    for t, c, d, a in pairs:
        fwd[off[t - 1] + d] += a
    keep = np.ones(off[-1], dtype=bool)
    passes = 0
    while True:
        passes += 1
        new = keep.copy()
        for t in range(1, T - 1):
            if seg_edge is not None and seg_edge[t]:
                continue
            bwd = np.zeros(ncomp[t])
            for tt, c, d, a in pairs:
                if tt == t and keep[off[t - 1] + d]:
                    bwd[c] += a
            for c in range(ncomp[t]):
                g = off[t] + c
                inv = 1.0 / area[g]
                fb, ff = inv * bwd[c], inv * fwd[g]
                if twosided:
                    kill = (fb != 0 and ff != 0 and (fb < overlap or ff < overlap)) or (fb != 0 and ff == 0 and fb < overlap) or \
                        (fb == 0 and ff != 0 and ff < overlap)
                else:
                    kill = ff < overlap
                new[g] = not kill
        if np.array_equal(new, keep):
            return passes
        keep = new


# ---------------------------------------------------------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------------------------------------------------------
def chunk_plane(ny, nx, rb, runs_per_chunk, phase=0):
    """0/1 plane with exactly runs_per_chunk[q] runs in write chunk q (one-pixel runs at every second column of the chunk's rows;
    the pole rows 0 and ny - 1 stay empty).  phase 1: the odd columns (disjoint from phase 0, same run count)."""
    m = np.zeros((ny, nx), dtype=np.uint8)
    nchunk = (ny + rb - 1) // rb
    for q in range(nchunk):
        n = int(runs_per_chunk[q % len(runs_per_chunk)])
        rows = [y for y in range(q * rb, min(ny, (q + 1) * rb)) if 0 < y < ny - 1]
        per_row = (nx - phase + 1) // 2
        if n > len(rows) * per_row:
            raise ValueError("chunk %d cannot hold %d runs" % (q, n))
        for y in rows:
            k = min(n, per_row)
            m[y, phase:phase + 2 * k:2] = 1
            n -= k
    return m


def dots(ny, nx, n, phase):
    """n one-pixel components on the odd rows (no pole row), at the even (phase 0) or odd (phase 1) columns, raster order"""
    m = np.zeros((ny, nx), dtype=np.uint8)
    ys, xs = np.meshgrid(np.arange(1, ny - 1, 2), np.arange(phase, nx, 2), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    if n > len(ys):
        raise ValueError("%d dots do not fit" % n)
    m[ys[:n], xs[:n]] = 1
    return m


def dot_capacity(ny, nx, phase=0):
    return len(range(1, ny - 1, 2)) * len(range(phase, nx, 2))


def dots_slab(T, ny, nx, nlab):
    """nlab one-step ids: dots whose phase alternates with t (a dot never overlaps one of the step before); the planes are filled in
    turn and the last one trimmed"""
    out = np.zeros((T, ny, nx), dtype=np.uint8)
    left = nlab
    for t in range(T):
        n = min(left, dot_capacity(ny, nx, t % 2))
        out[t] = dots(ny, nx, n, t % 2)
        left -= n
    if left:
        raise ValueError("%d ids do not fit %d planes" % (nlab, T))
    return out


def pair_slab(T, ny, nx, nlab):
    """nlab ids that each last two steps (persistence 2 keeps them): the dots of steps 2k and 2k + 1 sit on the same pixels, those of
    step pairs alternate their phase; T even"""
    assert T % 2 == 0
    per = [0] * (T // 2)
    left = nlab
    for k in range(T // 2):
        per[k] = min(left, dot_capacity(ny, nx, k % 2))
        left -= per[k]
    if left:
        raise ValueError("%d ids do not fit" % nlab)
    out = np.zeros((T, ny, nx), dtype=np.uint8)
    for k in range(T // 2):
        out[2 * k] = out[2 * k + 1] = dots(ny, nx, per[k], k % 2)
    return out


def cascade_slab(T, ny=32, nx=360, w=20, s=6, q=4, y0=10, h=8):
    """a removal cascade through every filtered step: a bar X_t of w columns moves right by s columns a step; a stub Y_t of q
    columns sits one blank column ahead of it.  X_t overlaps X_{t-1} in w - s columns and Y_{t-1} in q, so its backward overlap is
    (w - s + q) / w = 0.9 while X_{t-1} survives and q / w = 0.2 once it is removed; its forward overlap is (w - s) / w = 0.7.
    X_0 is missing, so X_1 goes in the first pass, X_2 in the second, ...: T - 2 passes change something, the next one nothing.
    Every component spans the same rows: the ratios are exact."""
    assert s >= q + 2 and (T - 1) * s + w + 1 + q <= nx
    m = np.zeros((T, ny, nx), dtype=np.uint8)
    for t in range(T):
        if t > 0:
            m[t, y0:y0 + h, t * s:t * s + w] = 1
        m[t, y0:y0 + h, t * s + w + 1:t * s + w + 1 + q] = 1
    return m


def slot_plane(ny, nx, n, kind):
    """n one-row components in slots of four columns on the odd rows (no pole row): slot i = (row 1 + 2 (i // (nx // 4)), column
    4 (i % (nx // 4))); a 'dot' is that pixel, a 'bar' the three pixels from it (column nx - 1 stays empty: no wrap)"""
    m = np.zeros((ny, nx), dtype=np.uint8)
    per = nx // 4
    if n > per * len(range(1, ny - 1, 2)):
        raise ValueError("%d slots do not fit" % n)
    for i in range(n):
        y, x = 1 + 2 * (i // per), 4 * (i % per)
        m[y, x:x + (3 if kind == "bar" else 1)] = 1
    return m


def filter_slab(T, ny, nx, edges, fill=2):
    """dots(nb) at t - 1, bars(nc) at t and t + 1 for every (t, nb, nc) of `edges`; `fill` dots at every other step"""
    m = np.repeat(slot_plane(ny, nx, fill, "dot")[None], T, axis=0)
    for t, nb, nc in edges:
        m[t - 1] = slot_plane(ny, nx, nb, "dot")
        m[t] = m[t + 1] = slot_plane(ny, nx, nc, "bar")
    return m


def filter_edge_forms(ncomp, npairs, filtered=None):
    """the LDS / lane edges of k_rs_pass_blk and k_rs_pass the filtered timesteps 1 .. T-2 reach: ncomp[t] components, npairs[t]
    pair records with t - 1 (k_rs_pass, k_rs_pass_blk in ctk_resolve_dev.hip)"""
    T = len(ncomp)
    out = set()
    for t in range(1, T - 1):
        if filtered is not None and not filtered[t]:
            continue
        nct, pn, prev = int(ncomp[t]), int(npairs[t]), int(ncomp[t - 1])
        out.add("blk:comps<=64" if nct <= 64 else ("blk:comps65-128" if nct <= PB_COMPS else "blk:comps>128"))
        out.add("blk:pairs<=64" if pn <= 64 else "blk:pairs>64")
        out.add("pass:comps<=512" if nct <= CTK_PASS_COMPS else "pass:comps>512")
        w = (t - 1) % PB_G
        if nct <= PB_COMPS:
            if w > 0 and prev <= PB_COMPS:
                out.add("blk:pred_lds")
            elif prev > PB_COMPS:
                out.add("blk:pred_big_in_wg" if w > 0 else "blk:pred_big_across")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cases of tests/test_gpu_tail_forms.py: name, shape, persistence, the mask builder and the forms they are meant to reach
# ---------------------------------------------------------------------------------------------------------------------------
CASES = []


def _case(name, T, ny, nx, make, reach, persistence=2, **kw):
    CASES.append(dict(name=name, T=T, ny=ny, nx=nx, make=make, reach=frozenset(reach), persistence=persistence, **kw))


def _chunks_case(T, ny, nx, pattern, alt):
    """plane A (chunk run counts `pattern`) at every step but step 3, plane B (`alt`, the other phase: one-step ids that persistence
    removes) there"""
    def make():
        rb = relabel_rows(T, ny, nx)
        a, b = chunk_plane(ny, nx, rb, pattern, 0), chunk_plane(ny, nx, rb, alt, 1)
        m = np.repeat(a[None], T, axis=0)
        m[3] = b
        return m
    return make


# 181 x 360: 11-row chunks (17 of them), k_relabel_v5 in one 20 KB image; chunks of 64 / 65 runs (chunk copy) and 512 / 513 (staged)
_case("v5_runs_181x360", 6, 181, 360, _chunks_case(6, 181, 360, (0, 64, 65, 512, 513, 1, 1024), (65, 64, 513, 512, 0)),
      {"v5", "v5:copy", "v5:staged", "v5:unstaged", "v5:img1", "v5:kb20", "v5:batched", "copy:built", "extent<64>", "extent<256>",
       "runval<256>", "pass_blk:SEG"}, extents=(64, 128, 256, EXTENT_BLK), seg=True)
# 4608 columns (and 4612, 4668: nx % 64 = 4, 60): 15 one-row chunks whose 20 KB image does not fit -- k_relabel_v4; rows of 64 / 65
# and 2048 / 2049 runs
for _nx in (4608, 4612, 4668):
    _case("v4_runs_15x%d" % _nx, 6, 15, _nx, _chunks_case(6, 15, _nx, (0, 64, 65, 2048, 2049, 1, 7), (0, 2049, 2048, 65, 64, 3, 9)),
          {"v4", "v4:copy", "v4:staged", "v4:unstaged", "copy:built", "extent_blk"}, extents=(64, 128, 256, EXTENT_BLK), seg=True)
# a grid whose rows are no multiple of four pixels: the generic kernel, no chunk copy
_case("generic_21x362", 6, 21, 362, _chunks_case(6, 21, 362, (3, 40, 0), (9, 0, 1)), {"generic", "copy:none"})

# every pixel foreground at every step: nothing writes background (n_tracked = ids alive - 1 + 0); with nx % 64 = 4 / 60 the last
# mask word of a row has invalid bits that must not count as background (nx % 64 in {0, 4, 60} through k_relabel_v5: 384, 388, 380;
# k_relabel_v4: 4608, 4612, 4668; the generic kernel: 22 and the offset pointer)
for _ny, _nx in ((9, 4608), (9, 4612), (9, 4668), (181, 360), (181, 364), (181, 380), (181, 384), (181, 388), (10, 22)):
    _case("full_%dx%d" % (_ny, _nx), 4, _ny, _nx, lambda T=4, ny=_ny, nx=_nx: np.ones((T, ny, nx), dtype=np.uint8), {"bg:none"})
# ... and the same planes with one more step than the object lives: every pixel filtered, background comes from the ids only
for _ny, _nx in ((9, 4612), (181, 380), (181, 384), (181, 388), (10, 22)):
    _case("filtered_%dx%d" % (_ny, _nx), 4, _ny, _nx, lambda T=4, ny=_ny, nx=_nx: np.ones((T, ny, nx), dtype=np.uint8), {"bg:filtered"},
          persistence=5)

# ids per k_run_values workgroup (fused pass, T = 4): 256 / 257 with 256 threads, 64 / 65 with 64 (ctk_debug_set_small_threads)
for _nl in (1024, 1025):
    _case("alive_%d" % _nl, 4, 181, 360, lambda nl=_nl: pair_slab(4, 181, 360, nl), {"alive:count" if _nl <= 1024 else "alive:sum"},
          nlab=_nl, rv_threads=(0, 64))
for _nl in (256, 257):
    _case("alive64_%d" % _nl, 4, 181, 360, lambda nl=_nl: pair_slab(4, 181, 360, nl), {"alive:count" if _nl <= 256 else "alive:sum"},
          nlab=_nl, rv_threads=(64,))

# 2 097 152 / 2 097 153 runs in the slab (8192 / 8193 rank blocks of 256): one-step dots on 181 x 360 planes, 16 200 a plane; the
# second call on the handle sees more than 10^6 ids of the first: the full k_count_alive
RANK_EDGE = CTK_RL_BLOCKS * 256
for _n in (RANK_EDGE, RANK_EDGE + 1):
    _case("rank_%d" % _n, 130, 181, 360, lambda n=_n: dots_slab(130, 181, 360, n),
          {"rank_merged" if _n <= RANK_EDGE else "rank_split", "count_f", "count_full"}, persistence=1, nlab=_n)

# 262 144 / 262 145 ids through the staged API (ctk_shard_write's two count kernels)
for _n in (262144, 262145):
    _case("write_count_%d" % _n, 18, 181, 360, lambda n=_n: dots_slab(18, 181, 360, n), {"write_count_1" if _n <= 262144 else "write_count_full"},
          persistence=1, nlab=_n, staged=True)

# a removal cascade through 34 filtered steps: 35 passes; the first call does not converge in 24, the next launches 48 per-pass
# kernels (NP > 32: k_count_alive_1)
CASCADE_T = 36
_case("cascade", CASCADE_T, 32, 360, lambda: cascade_slab(CASCADE_T), {"pass_blk", "pass_sync", "pass_fused", "pass_fused:SEG", "count_1", "count_f", "unite", "unite_slots"},
      cascade=CASCADE_T - 1)

# the filter passes' LDS edges (CTK_PASS_COMPS of k_rs_pass, PB_COMPS of k_rs_pass_blk in ctk_resolve_dev.hip): a timestep t of nc one-row bars whose predecessor holds nb dots
# (FILTER_EDGES: (t, nb, nc)); the bars' backward overlap is 1/3 while the dots live (removed), 0 if the dots were read as removed
# (kept): a bar's fate depends on reading its predecessor's bits right.  w = (t - 1) % 16 is the wave of t in its k_rs_pass_blk
# workgroup (0: the predecessor is in the workgroup before).
FILTER_T = 40
FILTER_EDGES = ((3, 64, 64), (7, 65, 65), (11, 128, 128), (17, 200, 100), (21, 129, 129), (25, 129, 128), (29, 513, 513), (33, 512, 512))
_case("filter_edges", FILTER_T, 64, 360, lambda: filter_slab(FILTER_T, 64, 360, FILTER_EDGES),
      {"blk:comps<=64", "blk:comps65-128", "blk:comps>128", "blk:pairs<=64", "blk:pairs>64", "blk:pred_lds", "blk:pred_big_in_wg",
       "blk:pred_big_across", "pass:comps<=512", "pass:comps>512", "pass_blk", "pass_sync", "pass_sync:SEG", "pass_blk:SEG"},
      filter_edges=True, seg=True)


def mask_of(case):
    return case["make"]()


def case_forms(case, mask=None):
    """the write and background forms a case reaches through the dense one-call paths (fresh handle; aligned flag)"""
    T, ny, nx = case["T"], case["ny"], case["nx"]
    m = mask_of(case) if mask is None else mask
    out = set()
    wf = write_form(T, ny, nx)
    cv = chunk_copy(T, ny, nx)
    out.add("copy:built" if cv else "copy:none")
    k = {5: "v5", 4: "v4", 0: "generic"}[wf["kernel"]]
    out.add(k)
    if wf["kernel"] in (4, 5):
        out |= chunk_value_forms(wf["kernel"], cv, chunk_runs(m, wf["rb"]))
    if wf["kernel"] == 5:
        nimg = (wf["rb"] + wf["sub"] - 1) // wf["sub"]
        out |= {"v5:img%s" % (nimg if nimg <= 2 else "3+"), "v5:kb%d" % wf["kb"], "v5:batched" if wf["batched"] else "v5:loops"}
    out.add("extent<%d>" % extent_form(T, nx) if extent_form(T, nx) != EXTENT_BLK else "extent_blk")
    for ex in case.get("extents", ()):
        out.add("extent<%d>" % ex if ex != EXTENT_BLK else "extent_blk")
    out.add("runval<%d>" % runval_threads(T, int(chunk_runs(m, 1).sum()), True))
    for th in case.get("rv_threads", ()):
        out.add("runval<%d>" % (th or 256))
    if m.all():
        out.add("bg:filtered" if case["persistence"] > T else "bg:none")
    if "nlab" in case and "rv_threads" in case:
        for th in case["rv_threads"]:
            out.add(alive_form(T, case["nlab"], th or 256))
    if "nlab" in case and not case.get("staged") and T > 2:
        out.add("rank_merged" if (int(m.sum()) + 255) // 256 <= CTK_RL_BLOCKS else "rank_split")
        out.add("count_f")
        if case["nlab"] > 1000000:
            out.add("count_full")
    if case.get("staged"):
        out.add("write_count_1" if case["nlab"] <= 262144 else "write_count_full")
    if case.get("filter_edges"):
        import cpu_tables
        tb = cpu_tables.build_tables(m.astype(bool), np.ones(ny, np.int64), np.zeros(ny, np.int64))
        npairs = np.bincount([p[0] for p in tb["pairs"]], minlength=T)
        out |= filter_edge_forms(tb["ncomp"], npairs)
        out |= {"pass_blk", "pass_sync", "pass_sync:SEG"}
    if case.get("seg") and T > 2:
        out.add("pass_blk:SEG")
    if "cascade" in case:
        if case["cascade"] > 24:
            out |= {"pass_blk", "pass_sync", "count_f"}
        if case["cascade"] > 32:
            out |= {"pass_fused", "pass_fused:SEG", "count_1", "unite", "unite_slots"}
    return out


CASE_BY_NAME = {c["name"]: c for c in CASES}

# the large shapes of tests/test_gpu_tail_forms_large.py: (T, ny, nx, the forms they are meant to reach); test_tail_forms.py checks
# the write / extent / run-value / filter forms against the restatement
LARGE = {
    "two_per_cu_4097": (4097, 8, 64, {"pass_blk", "pass_blk:SEG"}),
    "two_per_cu_4098": (4098, 8, 64, {"pass_blk_2pc", "pass_blk_2pc:SEG"}),      # (256 CUs)
    "long_rv64": (65537, 8, 64, {"runval<64>", "extent_blk"}),
    "extent128": (2049, 4, 1024, {"extent<128>"}),
    "stream_split": (262144, 4, 4, {"v5:batched", "v5:loops"}),
    "img2_kb20": (65500, 31, 140, {"v5:img2", "v5:kb20"}),
    "img2_kb24": (65500, 5, 1440, {"v5:img2", "v5:kb24"}),
    "img2_kb28": (65500, 5, 1760, {"v5:img2", "v5:kb28"}),
    "img3_kb20": (65536, 96, 128, {"v5:img3+", "v5:kb20"}),
}


def large_forms(name, n_cus=256):
    T, ny, nx, _ = LARGE[name]
    out = set()
    wf = write_form(T, ny, nx)
    out.add({5: "v5", 4: "v4", 0: "generic"}[wf["kernel"]])
    if wf["kernel"] == 5:
        nimg = (wf["rb"] + wf["sub"] - 1) // wf["sub"]
        out |= {"v5:img%s" % (nimg if nimg <= 2 else "3+"), "v5:kb%d" % wf["kb"], "v5:batched" if wf["batched"] else "v5:loops"}
    if name == "stream_split":
        out |= {"v5:batched" if write_form(T, ny, nx, nt=nt)["batched"] else "v5:loops" for _, nt in stream_blocks(T, 200000)}
    ex = extent_form(T, nx)
    out.add("extent_blk" if ex == EXTENT_BLK else "extent<%d>" % ex)
    out.add("runval<%d>" % runval_threads(T, T, True))
    bits = Handle(n_cus).fused(T, T)[0]
    for i, nm in enumerate(FILTER_NAMES):
        if bits & (1 << i):
            out.add(nm)
        if bits & (1 << i) and i in (0, 2):
            out.add(nm + ":SEG")
    return out


# every form the statistics' encodings name (include/contrack_hip.h) and every kernel edge of the restatement
FILTER_NAMES = ("pass_blk", "pass_blk:SEG", "pass_blk_2pc", "pass_blk_2pc:SEG", "pass_fused", "pass_fused:SEG", "pass_sync",
                "pass_sync:SEG", "unite_slots", "unite", "rank_merged", "rank_split")           # CTK_S_FILTER_FORMS bits 0 .. 11
EXTENT_NAMES = ("extent<64>", "extent<128>", "extent<256>", "extent_blk")                           # CTK_S_EXTENT_FORM
RUNVAL_NAMES = ("runval<64>", "runval<256>", "copy:built", "copy:none")                             # CTK_S_RUNVAL_FORM
RELABEL_NAMES = ("v5", "v4", "generic", "v5:img1", "v5:img2", "v5:img3+", "v5:kb20", "v5:kb24", "v5:kb28", "v5:batched", "v5:loops")
COUNT_NAMES = ("count_f", "count_1", "count_full", "write_count_1", "write_count_full")             # CTK_S_COUNT_FORM bits 0 .. 4
EDGE_NAMES = ("v5:copy", "v5:staged", "v5:unstaged", "v4:copy", "v4:staged", "v4:unstaged", "bg:none", "bg:filtered", "alive:count",
              "alive:sum", "blk:comps<=64", "blk:comps65-128", "blk:comps>128", "blk:pairs<=64", "blk:pairs>64", "blk:pred_lds",
              "blk:pred_big_in_wg", "blk:pred_big_across", "pass:comps<=512", "pass:comps>512")
FORMS = frozenset(FILTER_NAMES + EXTENT_NAMES + RUNVAL_NAMES + RELABEL_NAMES + COUNT_NAMES + EDGE_NAMES)
