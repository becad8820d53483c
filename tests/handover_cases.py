"""Constructed slabs that pin k_overlap (contrack_amd/csrc/ctk_kernels.hip) at the edges of its word loop, built for a wave-level
hand-over of the words with common pixels (each wave compacts them, in word order, into a 64-entry queue and its lanes take one each;
a wave whose step has more drains and continues).  That form was built, passed these slabs and measured slower (profiles/NOTES.md,
"k_overlap: wave-level hand-over"); the slabs stay, for the kernel as it is and for the next attempt at its middle.
Host-only: the geometry of a step (which thread, wave and trip u a mask word belongs to), planes built from it, and what a slab is
meant to reach (tests/test_overlap_handover_host.py checks that; tests/test_gpu_overlap_handover.py runs the slabs).

A plane has ny * W mask words, W = ceil(nx / 64); word i = y * W + w holds the pixels 64 w .. 64 w + 63 of row y, pixel x in bit x & 63.
k_overlap<OVB, TH> takes the plane in steps of OVB * TH words: inside a step, word j belongs to trip u = j // TH and thread j % TH,
wave (j % TH) // 64, lane j % 64."""
import numpy as np

import label_forms as lf

LONG_T = 65537

# (ny, nx, T): the smallest shapes of every instance (the names are ctk_overlap_form's, tests/label_forms.overlap_form)
SHAPES = [
    (181, 360, 4),        # <5,256>: 1086 words, a partial last word in every row, a last step that ends inside trip u = 4
    (205, 320, 4),        # <5,256>: 1025 words
    (160, 512, 4),        # <5,256>: 1280 words, full last word, every step full
    (32, 128, 4),         # <4,256>: 64 words, one wave
    (721, 1440, 3),       # <4,512>: T <= 1024 planes of 16 583 words
    (192, 512, 4),        # <6,256>
    (224, 512, 4),        # <8,256>
    (128, 4096, 3),       # <4,512>
    (8, 64, LONG_T),      # <4,128,5>: 8 words
]
CASES = ("none", "full", "n64", "n65", "cross", "alt_under_full", "alt_both")


def form_of(ny, nx, T):
    """(OVB, TH) of the instance that takes the shape"""
    code = lf.overlap_form(T, ny, (nx + 63) // 64, False)
    return code // 10000, code // 10 % 1000


def word_of(ny, nx, T, i):
    """(step, u, wave, lane) of mask word i"""
    ovb, th = form_of(ny, nx, T)
    step, j = divmod(i, ovb * th)
    return step, j // th, (j % th) // 64, j % 64


def common_words(prev, cur):
    """indices of the mask words of a plane pair that hold common pixels"""
    ny, nx = cur.shape
    W = (nx + 63) // 64
    o = np.zeros((ny, W * 64), dtype=bool)
    o[:, :nx] = (prev != 0) & (cur != 0)
    return np.nonzero(o.reshape(ny, W, 64).any(axis=2).ravel())[0]


def per_wave_step(ny, nx, T, words):
    """{(step, wave): number of the given words}"""
    out = {}
    for i in words:
        s, _, w, _ = word_of(ny, nx, T, int(i))
        out[(s, w)] = out.get((s, w), 0) + 1
    return out


def _rows(ny, every, limit):
    """rows `every` apart from row 1 on (the pole rows stay empty), at most `limit`, spread over the plane, the last one included"""
    ys = list(range(1, ny - 1, every)) or [0]
    if len(ys) > limit:
        ys = [ys[k * (len(ys) - 1) // (limit - 1)] for k in range(limit)]
    return sorted(set(ys))


def _alt_rows(nx):
    """rows of alternating pixels: enough for more than 700 pixels a plane where the plane has them -- more distinct pairs than the 512
    slots of k_overlap's hash, so that some go to the ungrouped records, and few enough for the pair table as it is first allocated"""
    return max(2, -(-700 // ((nx + 1) // 2)))


def _dots(ny, nx, T, n):
    """one pixel (bit 7) in each of n words of ONE wave's step: the last wave of the last full step, lanes 0 .. 39 of trip 0, the rest
    in lanes 0 .. of trip 1.  None where the plane has no such words."""
    ovb, th = form_of(ny, nx, T)
    W = (nx + 63) // 64
    nw = ny * W
    step = max(nw // (ovb * th) - 1, 0)
    wave = th // 64 - 1
    base = step * ovb * th + wave * 64
    if nw <= 64:                                   # one wave holds the plane: all its words, and no 65th
        idx = list(range(nw)) if n == 64 and nw == 64 else None
    elif base + th + 64 <= nw and ovb >= 2:
        idx = [base + l for l in range(40)] + [base + th + l for l in range(n - 40)]
    else:
        idx = None
    if idx is None:
        return None
    m = np.zeros((ny, nx), dtype=np.uint8)
    for i in idx:
        m[i // W, (i % W) * 64 + 7] = 1
    return m


def planes(case, ny, nx, T):
    """(P, C): two planes; a slab alternates them, so that each is `t` over the other as `t-1`.  None: the shape cannot hold the case."""
    W = (nx + 63) // 64
    big = ny * W > 4096
    P = np.zeros((ny, nx), dtype=np.uint8)
    C = np.zeros((ny, nx), dtype=np.uint8)
    if case == "none":                             # no common pixel anywhere: full rows, two apart, offset by one
        P[0::4] = 1
        C[2::4] = 1
    elif case == "full":                           # every pixel in both: every word has common pixels, 64 per wave and trip
        P[:] = 1
        C[:] = 1
    elif case in ("n64", "n65"):                   # exactly 64 / 65 words with common pixels in one wave's step
        C = _dots(ny, nx, T, 64 if case == "n64" else 65)
        if C is None:
            return None
        P[:] = 1
    elif case == "cross":
        # in every second row, at every word boundary b = 64 k: a run that crosses it in C only (row type 0), in P only (1), in both
        # (2); the other plane's run starts at b, so the common pixels lie in the right word and their run began in the left one.
        # Every boundary of the plane comes up, so also those whose left word is lane 63 of the wave before or the last word of the
        # step before.  Rows of type 0 also start with a run at x = 0 over a one-pixel run in P, and end with pixels in both planes:
        # the word that is first in its row must not take the carry of the row before (and the rows are seam rows).
        for n, y in enumerate(_rows(ny, 2, 64 if big else ny)):
            typ = n % 3
            for k in range(1, W):
                b = 64 * k
                if b + 3 > nx:
                    continue
                lo_c, lo_p = (b - 2, b) if typ == 0 else (b, b - 2) if typ == 1 else (b - 2, b - 3)
                C[y, lo_c:b + 2] = 1
                P[y, lo_p:b + 3] = 1
            if typ == 0:
                C[y, 0:2] = 1
                P[y, 0:1] = 1
                C[y, nx - 2:nx] = 1
                P[y, nx - 1:nx] = 1
    elif case == "alt_under_full":                 # single pixels, two apart, under full rows: 32 pieces in a word, a pair each
        for y in _rows(ny, 2, _alt_rows(nx)):
            C[y, 0::2] = 1
            P[y, :] = 1
    elif case == "alt_both":                       # ... and one component per piece on BOTH sides: as many distinct pairs as pixels
        for y in _rows(ny, 2, _alt_rows(nx)):
            C[y, 0::2] = 1
            P[y, 0::2] = 1
    else:
        raise ValueError(case)
    return P, C


def slab(case, ny, nx, T):
    """(T, ny, nx) uint8 mask alternating P, C, P, .., or None"""
    pc = planes(case, ny, nx, T)
    if pc is None:
        return None
    m = np.zeros((T, ny, nx), dtype=np.uint8)
    m[0::2] = pc[0]
    m[1::2] = pc[1]
    return m


def long_slab():
    """the 8 x 64 shape: every case it can hold in ONE slab of LONG_T steps (a slab per case would label 65 537 planes each time),
    four planes a case, two empty planes between cases, the first case at t = 0, the last at the end"""
    ny, nx, T = SHAPES[-1]
    m = np.zeros((T, ny, nx), dtype=np.uint8)
    names = [c for c in CASES if planes(c, ny, nx, T) is not None]
    for k, c in enumerate(names):
        P, C = planes(c, ny, nx, T)
        t0 = T - 4 if k == len(names) - 1 else (0 if k == 0 else 30000 + 6 * k)
        m[t0:t0 + 4:2] = P
        m[t0 + 1:t0 + 4:2] = C
    return m, names


def all_slabs():
    """(name, case or None, (ny, nx, T)) of every slab of the test"""
    out = []
    for ny, nx, T in SHAPES:
        if T == LONG_T:
            out.append(("%dx%dx%d-all" % (T, ny, nx), None, (ny, nx, T)))
            continue
        for c in CASES:
            if planes(c, ny, nx, T) is not None:
                out.append(("%dx%dx%d-%s" % (T, ny, nx, c), c, (ny, nx, T)))
    return out


def build(case, shape):
    ny, nx, T = shape
    return long_slab()[0] if case is None else slab(case, ny, nx, T)
