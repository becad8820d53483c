"""The numpy statement of the time filter (include/contrack_hip.h, "a weighted filter or a block mean along time"): a plain loop over
outputs and taps on float64 planes, written from the contract, not from the kernels.  Shared by the filter tests."""
import numpy as np


def default_offset(K, stride):
    """the Python default: a centred window at stride 1, blocks counted from the segment start otherwise"""
    return -(K // 2) if stride == 1 else 0


def segments_of(T, segments=None):
    """[(S, E)] of the segment starts (None: one segment)"""
    st = [0] if segments is None or len(segments) == 0 else [int(s) for s in segments]
    return list(zip(st, st[1:] + [T]))


def layout(T, K, stride=1, offset=None, segments=None):
    """(first, label, out_starts): per output the step of tap 0 and the label step, per segment its first output.  Brute force: every q
    from 0 until the label leaves the segment."""
    offset = default_offset(K, stride) if offset is None else offset
    first, label, out_starts = [], [], []
    for S, E in segments_of(T, segments):
        out_starts.append(len(first))
        q = 0
        while S + offset + q * stride + K // 2 < E:
            f = S + offset + q * stride
            if f + K // 2 >= S:
                first.append(f)
                label.append(f + K // 2)
            q += 1
    return np.array(first, dtype=np.int64), np.array(label, dtype=np.int64), np.array(out_starts, dtype=np.int64)


def time_filter(x, weights, stride=1, offset=None, edges="nan", skipna=False, segments=None):
    """x (T, ny, nx) float32 / float64; weights: K float64 values, or an int K (box mode).  Returns (T_out, ny, nx) of x's dtype."""
    x = np.asarray(x)
    T = x.shape[0]
    box = np.ndim(weights) == 0
    K = int(weights) if box else len(weights)
    w = None if box else np.asarray(weights, dtype=np.float64)
    first, label, _ = layout(T, K, stride, offset, segments)
    seg = segments_of(T, segments)
    out = np.empty((len(first),) + x.shape[1:], dtype=x.dtype)
    with np.errstate(all="ignore"):
        for o, (f, lab) in enumerate(zip(first, label)):
            S, E = next((S, E) for S, E in seg if S <= lab < E)
            s = np.zeros(x.shape[1:], dtype=np.float64)
            ws = np.zeros(x.shape[1:], dtype=np.float64)
            n = np.zeros(x.shape[1:], dtype=np.int64)
            used = [i for i in range(K) if S <= f + i < E]
            for i in used:
                v = x[f + i].astype(np.float64)
                take = ~np.isnan(v) if skipna else np.ones(v.shape, dtype=bool)
                if box:
                    s = np.where(take, s + v, s)
                else:
                    prod = w[i] * v                                   # rounded to float64 ...
                    s = np.where(take, s + prod, s)                   # ... then added
                    ws = np.where(take, ws + w[i], ws)
                n = n + take
            complete = len(used) == K
            if box:
                r = s / n.astype(np.float64)
            else:
                r = np.where(complete & (n == K), s, s / ws)
            r = np.where(n == 0, np.nan, r)
            if edges == "nan" and not complete:
                r = np.full(x.shape[1:], np.nan)
            out[o] = r.astype(x.dtype)
    return out


def lanczos_closed_form(ntaps, cutoff):
    """Duchon (1979), eq. 9 with the sigma factor: the low-pass weights before normalisation, evaluated term by term"""
    n = (ntaps - 1) // 2
    w = np.zeros(ntaps, dtype=np.float64)
    for i in range(ntaps):
        k = i - n
        if k == 0:
            w[i] = 2.0 * cutoff
        else:
            w[i] = (np.sin(2.0 * np.pi * cutoff * k) / (np.pi * k)) * (np.sin(np.pi * k / (n + 1)) / (np.pi * k / (n + 1)))
    return w


def bits(a):
    """the array's bits as unsigned integers (+0.0 and -0.0 differ, every NaN is made one NaN first)"""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = 0
    return u


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a), bits(b))


def edge_field(T, ny, nx, dtype, seed=0):
    """a field with NaN, +-inf, +-0.0 and denormals sprinkled over a smooth random one"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, ny, nx)) * 100.0).astype(dtype)
    tiny = np.finfo(dtype).tiny
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, tiny / 4, -tiny / 8]
    idx = rng.integers(0, x.size, size=max(8, x.size // 50))
    x.reshape(-1)[idx] = np.array(specials, dtype=dtype)[rng.integers(0, len(specials), size=idx.size)]
    return x
