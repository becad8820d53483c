// ctk_lifecycle_stream_* (include/contrack_hip.h): the run_lifecycle reductions with both slabs passing through chunk-sized device
// buffers.  Part of ctk_api.hip's translation unit.
//
// Every time step is reduced on its own, so a chunk is a small resident call: the pieces of lifecycle_dev_impl (life_launch,
// life_settle, life_land, life_sort) run on the chunk's two buffers with ctk_life_plan evaluated for them, and the per-time-step
// tables are those of one chunk.  stream_in carries the flags as its second slab and sends chunk k+1 off before chunk k is reduced
// (StreamIO::ahead): its upload runs under the reductions.  The rows that need the reference's summation orders are chosen by the
// caller's `pick` and re-evaluated (life_exact_keys) while their chunk is still in its buffers; their records are kept with the
// rows' (label, t) and matched to the slab's sorted rows after the last chunk.

struct LifePicked { int32_t label, t; ctk_life_exact rec; };

// one chunk, uploaded: rows with global t appended to `all`, the picked ones re-evaluated and appended to `picked`
static int life_stream_chunk(ctk_handle *h, LifeRun &r, bool first, ctk_life_pick_fn pick, void *pick_user, std::vector<ctk_life_row> &sorted,
                             std::vector<int64_t> &idx, std::vector<CtkLifeKey> &keys, std::vector<ctk_life_exact> &recs,
                             std::vector<ctk_life_row> &all, std::vector<LifePicked> &picked)
{
    r.plan = ctk_life_plan(r.T, r.ny, r.nx, r.f64, (uintptr_t)r.flag, (uintptr_t)r.field);
    if (first) h->lc_plan = r.plan;
    r.cap = std::max<size_t>(h->lc_rows.cap / sizeof(CtkLifeRowDev), (size_t)r.T * 16 + 1024);
    int rc = life_launch(h, r);
    if (rc == CTK_OK) rc = life_settle(h, r);
    h->lc_attempts += r.attempts; h->lc_given_up += r.given_up; h->lc_fb_launches += r.fb_launches;
    CTKCHK(rc);
    const size_t n = (size_t)r.cnt[0];
    if (!n) return CTK_OK;
    ctk_life_row *land = nullptr;
    CTKCHK(life_land(h, n, &land));
    (void)life_sort(h, land, n, r.T, sorted);                                   // (label, t) inside the chunk, t still counted from its first step
    if (pick) {
        for (size_t i = 0; i < n; ++i) sorted[i].t += (int32_t)r.t_base;
        idx.resize(n);
        int64_t nidx = 0;
        const int prc = pick(pick_user, sorted.data(), (int64_t)n, idx.data(), &nidx);
        if (prc) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream: pick returned %d for the rows of time steps [%lld, %lld)", prc, (long long)r.t_base, (long long)(r.t_base + r.T));
        if (nidx < 0 || (size_t)nidx > n) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream: pick chose %lld of %zu rows", (long long)nidx, n);
        keys.resize((size_t)nidx);
        for (int64_t i = 0; i < nidx; ++i) {
            if (idx[(size_t)i] < 0 || (size_t)idx[(size_t)i] >= n || (i && idx[(size_t)i] <= idx[(size_t)i - 1]))
                return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream: pick must fill ascending indices below %zu", n);
            const ctk_life_row &w = sorted[(size_t)idx[(size_t)i]];
            keys[(size_t)i] = CtkLifeKey{w.t - (int32_t)r.t_base, w.label, w.shift, w.pad};          // the kernels index the chunk's own planes
        }
        if (nidx) {
            recs.resize((size_t)nidx);
            CTKCHK(life_exact_keys(h, r.flag, r.field, r.f64, r.ny, r.nx, keys, recs.data()));
            for (int64_t i = 0; i < nidx; ++i) {
                const ctk_life_row &w = sorted[(size_t)idx[(size_t)i]];
                picked.push_back(LifePicked{w.label, w.t, recs[(size_t)i]});
            }
        }
    } else
        for (size_t i = 0; i < n; ++i) sorted[i].t += (int32_t)r.t_base;
    all.insert(all.end(), sorted.begin(), sorted.end());
    return CTK_OK;
}

static int life_stream_impl(ctk_handle *h, StreamIO &io, bool f64, int64_t T, int ny, int nx, const float *wrow, int64_t chunk_steps,
                            ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (T < 0 || ny < 1 || nx < 1 || !wrow || chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream: bad shape, null weights or negative chunk_steps");
    if (T > 0 && ((!io.host_in && !io.read) || (!io.host_in2 && !io.read2))) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream: no flag source or no field source");
    CTKCHK(life_check_shape(T, ny, nx));
    HIPCHK(hipSetDevice(h->device));
    life_reset(h, T);
    h->lc_streamed = true;
    if (nrows) *nrows = 0;
    if (nexact) *nexact = 0;
    if (T == 0) { h->lc_path_T = 0; return CTK_OK; }
    io.esz = f64 ? 8 : 4;
    io.esz2 = 4;
    io.ahead = true;
    const size_t plane = (size_t)ny * nx * io.esz;
    io.chunk = ctk_stream_chunk(chunk_steps, T, plane);
    int32_t wshift = 0, limb_bits = 0;
    CTKCHK(life_weights(h, wrow, ny, nx, &wshift, &limb_bits));
    h->lc_f64 = f64; h->lc_T = T; h->lc_ny = ny; h->lc_nx = nx;
    std::vector<ctk_life_row> all, sorted;
    std::vector<LifePicked> picked;
    std::vector<int64_t> idx;
    std::vector<CtkLifeKey> keys;
    std::vector<ctk_life_exact> recs;
    const double t0 = now_ms();
    bool first = true;
    const int rc = stream_consume(h, io, f64, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        LifeRun r;
        r.flag = (const int32_t *)io.dev2; r.field = chunk; r.f64 = f64; r.T = nt; r.ny = ny; r.nx = nx;
        r.wshift = wshift; r.limb_bits = limb_bits; r.t_base = c0;
        const int crc = life_stream_chunk(h, r, first, pick, pick_user, sorted, idx, keys, recs, all, picked);
        first = false;
        return crc;
    });
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    CTKCHK(rc);
    // the chunks' rows, each sorted, become the slab's: the same sort as a resident call's, over all T steps
    h->lc_sort = life_sort(h, all.data(), all.size(), T, h->lc_host);
    // (label, t) is unique per row: the picked rows, put into the same order, are found in one pass over the sorted rows
    std::sort(picked.begin(), picked.end(), [](const LifePicked &a, const LifePicked &b) { return a.label != b.label ? a.label < b.label : a.t < b.t; });
    h->lx_idx.reserve(picked.size());
    h->lx_rec.reserve(picked.size());
    size_t j = 0;
    for (size_t i = 0; i < h->lc_host.size() && j < picked.size(); ++i)
        if (h->lc_host[i].label == picked[j].label && h->lc_host[i].t == picked[j].t) { h->lx_idx.push_back((int64_t)i); h->lx_rec.push_back(picked[j].rec); ++j; }
    if (j != picked.size()) { h->lc_host.clear(); h->lx_idx.clear(); h->lx_rec.clear(); return ctk_set_error(CTK_E_INTERNAL, "ctk_lifecycle_stream: a picked row is not among the rows"); }
    if (nrows) *nrows = (int64_t)h->lc_host.size();
    if (nexact) *nexact = (int64_t)h->lx_idx.size();
    h->lc_path_T = T;
    return CTK_OK;
}

extern "C" int ctk_lifecycle_stream_f32(ctk_handle *h, const int32_t *flag, const float *field, int64_t T, int ny, int nx, const float *wrow, int64_t chunk_steps,
                                        ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact)
{
    StreamIO io;
    io.host_in = field; io.host_in2 = flag;
    return life_stream_impl(h, io, false, T, ny, nx, wrow, chunk_steps, pick, pick_user, nrows, nexact);
}
extern "C" int ctk_lifecycle_stream_f64(ctk_handle *h, const int32_t *flag, const double *field, int64_t T, int ny, int nx, const float *wrow, int64_t chunk_steps,
                                        ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact)
{
    StreamIO io;
    io.host_in = field; io.host_in2 = flag;
    return life_stream_impl(h, io, true, T, ny, nx, wrow, chunk_steps, pick, pick_user, nrows, nexact);
}
extern "C" int ctk_lifecycle_stream_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                                       ctk_read_chunk_fn field_reader, void *field_user, const float *wrow, int64_t chunk_steps, ctk_life_pick_fn pick,
                                       void *pick_user, int64_t *nrows, int64_t *nexact)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    StreamIO io;
    io.read = field_reader; io.read_user = field_user; io.read2 = flag_reader; io.read2_user = flag_user;
    return life_stream_impl(h, io, elem_bytes == 8, T, ny, nx, wrow, chunk_steps, pick, pick_user, nrows, nexact);
}

// the rows the last streamed call's pick chose: ascending indices into its sorted rows, and their records
extern "C" int ctk_lifecycle_stream_exact(ctk_handle *h, int64_t *row_idx, ctk_life_exact *out, int64_t cap)
{
    if (!h || (cap > 0 && (!row_idx || !out))) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream_exact: null argument");
    if (!h->lc_streamed || h->lc_path_T < 0) return ctk_set_error(CTK_E_STATE, "ctk_lifecycle_stream_exact needs a finished ctk_lifecycle_stream_* call first");
    const size_t n = h->lx_idx.size();
    if (cap < 0 || (size_t)cap < n) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_stream_exact: room for %lld rows, %zu held", (long long)cap, n);
    if (n) { memcpy(row_idx, h->lx_idx.data(), n * sizeof(int64_t)); memcpy(out, h->lx_rec.data(), n * sizeof(ctk_life_exact)); }
    return CTK_OK;
}
