/*
 * contrack_hip.h -- C ABI of libcontrack_hip.so, the MI355X (gfx950) implementation of ConTrack's
 * run_contrack hot path.
 *
 * What this replaces.  The reference (steidani/ConTrack v0.4.1) has NO FFI/plugin interface: its hot
 * path is the Python method contrack.run_contrack (contrack/contrack.py:583-796), which calls
 * scipy.ndimage.label (:684, :748), scipy.ndimage.find_objects (:708, :753, :766) and numpy reductions
 * (:717-719) on a (time, lat, lon) array.  The entry points below are what a ctypes binding inside
 * run_contrack binds instead of those calls (INTEGRATION.md shows the stub).  Plain pointers and
 * sizes only; all buffers are caller-owned and borrowed for the duration of the call; the library owns
 * its device workspace (inside the opaque handle).  Every function returns 0 on success or a negative
 * CTK_E_* code; ctk_last_error() returns a thread-local message.  Nothing throws or exits.
 *
 * Conventions shared by all entry points
 *   anom      C-contiguous float32 (T, ny, nx) -- the slab after contrack.py:677-681 put it in
 *             (time, lat, lon) order.
 *   thr       T doubles; the compare evaluated is (double)anom[t,y,x] <op> thr[t].  The caller rounds a
 *             Python-number threshold to float32 first (that is what contrack.py:665 compares against
 *             for a float32 array); a float64 threshold vector is passed unrounded (contrack.py:650).
 *   cmp_op    0 '>='/'ge', 1 '<='/'le', 2 '>'/'gt', 3 '<'/'lt'     (contrack.py:649-656, :664-671)
 *   wrow      ny float32 row weights, computed by the host exactly as contrack.py:703-704 does.
 *   overlap, persistence, twosided                                   (contrack.py:587-589)
 *   flag      int32 (T, ny, nx): the ids of contrack.py:776-791, identical to the reference's
 *             (identity permutation), 0 = background.
 *   n_tracked len(np.unique(flag)) - 1                               (contrack.py:793)
 *
 * This header is the drop-in boundary: create / destroy / errors, the track entries (host arrays, device-resident, time-sharded,
 * streaming, resident anomaly slab), the staged time-shard protocol, the communicator, run_lifecycle, calc_anom / percentile, the
 * thin memory helpers a ctypes host needs, timing and workload statistics.  Test hooks (ctk_debug_*), experiment knobs and the
 * measurement support of the tests and of bench.py are declared in contrack_hip_debug.h.
 */
#ifndef CONTRACK_HIP_H
#define CONTRACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTK_OK            0
#define CTK_E_INVALID    -1   /* bad argument (shape, cmp_op, NULL, non-finite weight ...)      */
#define CTK_E_NODEVICE   -2   /* no usable HIP device / HIP runtime error                        */
#define CTK_E_NOMEM      -3   /* host or device allocation failed                                */
#define CTK_E_RANGE      -4   /* weight dynamic range or problem size beyond what the kernels carry */
#define CTK_E_INTERNAL   -5
#define CTK_E_STATE      -6   /* staged calls out of order                                       */
#define CTK_E_COMM       -7   /* time-shard path: another rank gave up, died or did not arrive in time (the message names it);
                                 the communicator is retired -- create a new one                      */

typedef struct ctk_handle ctk_handle;

/* ---- library / device ------------------------------------------------------------------------ */
int         ctk_version(void);
const char *ctk_last_error(void);
int         ctk_device_count(void);                       /* <0 on HIP error, 0 if no GPU          */
int         ctk_create(ctk_handle **h, int device);       /* binds the handle to one GPU + stream  */
void        ctk_destroy(ctk_handle *h);

/* ---- whole path, one call (replaces contrack.py:646-772 on the (time,lat,lon) slab) ----------- */
/* host buffers in, host buffers out (H2D + kernels + D2H) */
int ctk_track_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr,
                  int cmp_op, const float *wrow, double overlap, int persistence, int twosided,
                  int32_t *flag, int64_t *n_tracked);
/* device buffers in, device buffers out (anom_dev / flag_dev are HIP device pointers) */
int ctk_track_f32_dev(ctk_handle *h, const float *anom_dev, int64_t T, int ny, int nx,
                      const double *thr, int cmp_op, const float *wrow, double overlap,
                      int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked);

/* Threshold field for the following track calls on this handle (contrack.py:648-671 with a threshold that varies by grid point).
 * field: host array, elem_bytes 4 (float32) or 8 (float64), [nplanes][ny][nx]; plane_of_step[T]: plane used by step t
 * (0 <= p < nplanes).  field == NULL clears it.  A track call uses the field only when it is passed thr == NULL and its (T, ny, nx)
 * match; thr != NULL keeps today's path.  Taken by the host, _dev, resident and streaming entries; the staged and time-shard entries
 * refuse thr == NULL.  The compare is numpy's: a float32 slab against a float32 field in float32, against a float64 field exactly as
 * (double)x <op> field (the float32 copy it reads is prepared once per field and op), a float64 slab in float64.  NaN compares false.
 * The field stays on the device until it is cleared or replaced. */
int ctk_set_threshold_field(ctk_handle *h, const void *field, int elem_bytes, int64_t nplanes, int ny, int nx,
                            const int32_t *plane_of_step, int64_t T);

/* Segment breaks for the following track calls on this handle: the time axis is K independent series (ensemble members concatenated
 * in time, a seasonal selection with gaps).  starts[0] = 0 < starts[1] < ... < starts[nseg-1]; segment k is the steps
 * [starts[k], starts[k+1]) (the last one ends at T).  starts == NULL or nseg == 0 clears them.  Sticky, like the threshold field.
 * At a break the pass changes three things and nothing else:
 *   - no overlap pairs between the two planes (the first step of a segment has no predecessor, as t = 0 has);
 *   - the first and the last step of every segment are exempt from the overlap filter (contrack.py:706-742, range(1, T-1) of
 *     each segment), so their components are kept whatever twosided says;
 *   - no 3-D connection across it (contrack.py:747-751).
 * So each segment's ids minus an offset equal, bit for bit, run_contrack on that segment alone; ids are unique over the slab and keep
 * scipy's raster numbering (the offset of segment k is the number of 3-D components of segments 0 .. k-1); persistence counts
 * inside a segment; n_tracked is len(np.unique(flag)) - 1 of the whole result.  starts == {0} gives today's result.
 * Taken by the host, _dev and resident entries (with or without a threshold field).  A call whose T <= starts[nseg-1] returns
 * CTK_E_INVALID; the streaming, staged and time-shard entries return CTK_E_INVALID while segments are set.  The streaming and
 * time-shard paths take the starts as an ARGUMENT of the call instead (ctk_track_stream_seg_*, ctk_track_sharded_seg_*_dev below:
 * same rules, same semantics); those refuse a handle that also has sticky segments set. */
int ctk_set_segments(ctk_handle *h, const int64_t *starts, int64_t nseg);

/* The host-array entries keep device copies of the slab and of the result in the handle between calls (grow-only, so that
 * repeated calls do not reallocate).  ctk_release_io frees them (and the copy lanes, and the resident anomaly and vertical-mean
 * slabs): call it after a one-off large slab. */
int ctk_release_io(ctk_handle *h);

/* float64 slabs (xarray often hands float64 anomalies): the compare is evaluated in float64, exactly as
 * numpy does for a float64 array at contrack.py:665; everything downstream is identical.            */
int ctk_track_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr,
                  int cmp_op, const float *wrow, double overlap, int persistence, int twosided,
                  int32_t *flag, int64_t *n_tracked);
int ctk_track_f64_dev(ctk_handle *h, const double *anom_dev, int64_t T, int ny, int nx,
                      const double *thr, int cmp_op, const float *wrow, double overlap,
                      int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked);

/* ---- staged path: the stages of the path one by one, with the component tables resolved on the HOST (ctk_resolve).
 *      Kept for stage-level parity tests and as the table-level specification of the resolver; the multi-GPU product path
 *      is ctk_track_sharded_* above.  Each shard owns timesteps [t_begin, t_begin+T). ------ */
/* stage 1: threshold -> bit mask -> 2-D labelling with longitude wrap (contrack.py:646-698) + per
 *          component areas (contrack.py:717).  has_prev != 0 means a previous shard exists and
 *          its last timestep will be imported before stage 2.                                    */
int ctk_shard_label2d(ctk_handle *h, const float *anom_dev, int64_t T, int ny, int nx,
                      const double *thr, int cmp_op, const float *wrow, int has_prev);
int ctk_shard_label2d_f64(ctk_handle *h, const double *anom_dev, int64_t T, int ny, int nx,
                          const double *thr, int cmp_op, const float *wrow, int has_prev);
/* halo: the labelled LAST timestep of this shard, as an opaque device blob for the next rank
 *       (bit mask + run->component ids; the compressed form of the one-timestep label map).      */
int ctk_shard_halo_size(ctk_handle *h, size_t *max_bytes);           /* upper bound, same on all ranks */
int ctk_shard_halo_export(ctk_handle *h, void **blob_dev, size_t *nbytes);
int ctk_shard_halo_import(ctk_handle *h, const void *blob_dev, size_t nbytes);
/* stage 2: label co-occurrence histogram between consecutive timesteps (the overlap areas of
 *          contrack.py:718-719 and the temporal links of contrack.py:748-750).                   */
int ctk_shard_overlap(ctk_handle *h);
/* tables: serialised component / pair / seam tables of this shard (host memory owned by the
 *         handle, valid until the next staged call on it).                                       */
int ctk_shard_tables(ctk_handle *h, const void **blob, size_t *nbytes);

/* resolve: host-side, GPU-free.  Takes the table blobs of ALL shards in time order and evaluates the
 *          sequential parts of the reference on component tables: overlap filter recurrence
 *          (contrack.py:706-742), 3-D labelling ids (contrack.py:748-751), bbox-confined seam merges
 *          (contrack.py:753-763).  Returns an opaque result (free with ctk_result_free).          */
typedef struct ctk_result ctk_result;
int  ctk_resolve(const void *const *blobs, const size_t *nbytes, int nshards, double overlap,
                 int twosided, ctk_result **out);
void ctk_result_free(ctk_result *r);
int  ctk_result_info(const ctk_result *r, int64_t *n_labels, int64_t *n_ops, int64_t *n_complex,
                     int64_t *n_ambiguous, int64_t *n_components);

/* read-only views into a result (valid until ctk_result_free): comp_label[ncomps] in (shard, t, c)
 * order -- 0 = removed by the overlap filter, L > 0 = final id of every pixel of the component, -L =
 * the component must be folded pixel by pixel starting from 3-D label L; ops[nops] = the bbox-confined
 * relabel operations in execution order, 8 int32 each: hi, lo, t0, t1, y0, y1, x0, x1 (inclusive). */
int  ctk_result_arrays(const ctk_result *r, const int32_t **comp_label, int64_t *ncomps, const void **ops,
                       int64_t *nops, const int64_t **shard_comp_off, const int64_t **shard_t_off);
int  ctk_result_nshards(const ctk_result *r);          /* length-1 of the two offset arrays above */
/* exact integer limbs of the float32 row weights: w[y] = (wlo[y] + whi[y] * 2^limb_bits) * 2^-wshift.  limb_bits is 31
 * unless the weights span more than 62 bits (float64 latitudes with exact poles: cos(pi/2) = 6e-17 next to 1); then it
 * is ceil(span / 2), which needs limb_bits + ceil(log2 npix) <= 62 with npix = ny * nx, the most pixels any area sum
 * covers (CTK_E_RANGE otherwise). */
int  ctk_weights_to_limbs(const float *wrow, int ny, int64_t npix, int64_t *wlo, int64_t *whi, int32_t *wshift, int32_t *limb_bits);

/* stage 3: apply the result to this shard (index `shard` of the blobs given to ctk_resolve):
 *          per-label time extents (persistence, contrack.py:765-772), then the relabel pass that
 *          writes flag.  ext_dev: device int32 [2*(n_labels+1)] (min t | max t); when ranks > 1 the
 *          caller all-reduces the first half with MIN and the second with MAX between _extents and
 *          _write.                                                                                */
int ctk_shard_extents(ctk_handle *h, const ctk_result *r, int shard, int64_t t_begin,
                      int32_t **ext_dev, int64_t *n_labels);
int ctk_shard_write(ctk_handle *h, int persistence, int32_t *flag_dev, int64_t *n_alive_local,
                    int *wrote_background);
/* number of labels that survive persistence (identical on all ranks after the all-reduce)        */
int ctk_shard_count_tracked(ctk_handle *h, int64_t *n_alive);

/* ---- time-sharded path, one rank per GPU --------------------------------------------------------------------
 * Rank r owns the timesteps [t_begin, t_begin + T_local) of a slab of T_total steps (time order = rank order; every rank
 * owns at least one step).  ctk_track_sharded_* is ctk_track_*_dev on that shard: bulk data stays local, the ranks
 * exchange a one-timestep label-map halo with their neighbours and a few hundred boundary records through the
 * communicator (contrack_amd/csrc/ctk_sharded.hip).  flag / n_tracked are identical to what one call on the whole slab
 * returns; n_tracked is the same on every rank.  All ranks must make the call (it contains collectives).
 *
 * Communicator: RCCL over xGMI (one process per GPU; librccl.so is loaded on first use), an in-process group (several
 * handles driven by one host thread each), or a shared-memory transport for several processes on one node without RCCL. */
typedef struct ctk_comm ctk_comm;
typedef struct ctk_comm_group ctk_comm_group;
#define CTK_COMM_ID_BYTES 128
int  ctk_comm_unique_id(void *id /* CTK_COMM_ID_BYTES, made on rank 0 (ncclGetUniqueId), handed to the other ranks by the launcher */);
int  ctk_comm_init_rccl(ctk_handle *h, const void *id, int rank, int world, ctk_comm **out);
int  ctk_comm_group_create(int world, ctk_comm_group **out);
void ctk_comm_group_destroy(ctk_comm_group *g);
int  ctk_comm_init_local(ctk_handle *h, ctk_comm_group *g, int rank, ctk_comm **out);
int  ctk_comm_init_shm(ctk_handle *h, const char *segment_name, int rank, int world, ctk_comm **out);
void ctk_comm_destroy(ctk_comm *c);
int  ctk_comm_rank(const ctk_comm *c);
int  ctk_comm_world(const ctk_comm *c);
int  ctk_comm_barrier(ctk_comm *c);
int  ctk_comm_allgather_host(ctk_comm *c, const void *send, void *recv /* world * nbytes */, size_t nbytes /* <= 4096 */);
int  ctk_comm_ops(const ctk_comm *c, int64_t *shifts, int64_t *allgathers);      /* operations issued so far */
/* the librccl file the RCCL transport took its symbols from ("" before the first ctk_comm_init_rccl).  Order of choice: CTK_RCCL_LIB; a
 * copy already mapped into the process (one RCCL per process); $ROCM_PATH/lib, /opt/rocm/lib; the loader path. */
const char *ctk_comm_rccl_library(void);
/* Failure behaviour.  No rank is left waiting for one that gave up or died: the ranks of an rccl / shm communicator share a small
 * control segment in POSIX shared memory (single node) with a failure word and every rank's pid; every wait of the path polls it,
 * checks that the peers' processes still exist, and carries a deadline (seconds; default 120 or CTK_COMM_TIMEOUT_S).  A call that
 * fails on one rank makes every other rank's call return CTK_E_COMM (the message names the rank and its code) -- within
 * milliseconds, not at the deadline; the RCCL communicator is aborted (ncclCommAbort) so that kernels in flight return.  Errors
 * that every rank derives from the same gathered data (table overflow, id range) are returned by all ranks with their own code
 * and leave the communicator usable. */
int  ctk_comm_set_timeout(ctk_comm *c, double seconds);
int  ctk_comm_failed(const ctk_comm *c, int *code /* 0: fine */, int *rank);
int  ctk_comm_abort_rank(ctk_comm *c, int code /* < 0 */);                      /* this rank gives up (e.g. its caller failed elsewhere) */
int  ctk_track_sharded_f32_dev(ctk_handle *h, ctk_comm *c, const float *anom_dev, int64_t T_local, int64_t t_begin, int64_t T_total,
                               int ny, int nx, const double *thr /* T_local */, int cmp_op, const float *wrow, double overlap,
                               int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked);
int  ctk_track_sharded_f64_dev(ctk_handle *h, ctk_comm *c, const double *anom_dev, int64_t T_local, int64_t t_begin, int64_t T_total,
                               int ny, int nx, const double *thr, int cmp_op, const float *wrow, double overlap,
                               int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked);
/* ... with segment breaks (semantics: ctk_set_segments).  starts_global[nseg] are step indices into [0, T_total): starts_global[0] = 0,
 * strictly increasing, the last one below T_total (CTK_E_INVALID otherwise, and for a handle with sticky segments set).  EVERY rank
 * passes the SAME starts -- they are an argument of the collective; ranks that pass different ones get an undefined result or
 * CTK_E_INTERNAL, as ranks that disagree about T_total do.  Breaks may fall anywhere: inside a shard, on a shard cut (then the two
 * ranks exchange what they always exchange and ignore it), one per step.  flag / n_tracked are what the one-call entries return
 * with ctk_set_segments on the whole slab.  nseg == 0 or starts_global == {0} is ctk_track_sharded_*_dev, bit for bit, with the
 * same kernels. */
int  ctk_track_sharded_seg_f32_dev(ctk_handle *h, ctk_comm *c, const float *anom_dev, int64_t T_local, int64_t t_begin, int64_t T_total,
                                   int ny, int nx, const double *thr /* T_local */, int cmp_op, const float *wrow, double overlap,
                                   int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked, const int64_t *starts_global,
                                   int64_t nseg);
int  ctk_track_sharded_seg_f64_dev(ctk_handle *h, ctk_comm *c, const double *anom_dev, int64_t T_local, int64_t t_begin, int64_t T_total,
                                   int ny, int nx, const double *thr, int cmp_op, const float *wrow, double overlap,
                                   int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked, const int64_t *starts_global,
                                   int64_t nseg);

/* ---- next row N4: streaming entries (xr.open_dataset contrack.py:176 -> run_contrack -> to_netcdf README.rst:154) ------------
 * ctk_track_f32 / _f64 for slabs that should not (or cannot) sit in HBM twice: the slab passes through two chunk-sized device
 * buffers per direction; only the bit mask (1/32 of the slab) and the run / component tables stay resident between the
 * two pixel passes.
 *     chunk k+1 arrives (reader callback / host array -> H2D)   ||   k_threshold(chunk k) -> mask
 *     labelling, overlap filter, 3-D ids, seam merges, persistence on mask and tables          (nothing of the slab needed)
 *     k_relabel(chunk k+1)                                      ||   D2H(chunk k) -> writer callback / host array
 * ctk_track_stream_f32 / _f64: source and sink are host arrays (any size the host holds; device footprint 4 chunks + slab/32).
 * ctk_track_stream_cb: source and sink are callbacks, e.g. a netCDF variable read / written slice by slice.  The reader fills
 * `dst` (pinned host memory owned by the library, nt * ny * nx elements of elem_bytes) with timesteps [t0, t0 + nt) and returns 0;
 * the writer receives the int32 flag values of [t0, t0 + nt) in pinned memory valid during the call and returns 0; a nonzero
 * return aborts the call with CTK_E_INVALID.  Readers are called in increasing t0, once per chunk -- unless the call meets a
 * decision on a rounding boundary (CTK_S_EXACT_FIXUPS), in which case the input is streamed a second time.  Writers are called
 * in increasing t0, once.  chunk_steps = 0: about 256 MB of input per chunk.  Results: identical to ctk_track_*. */
typedef int (*ctk_read_chunk_fn)(void *user, int64_t t0, int64_t nt, void *dst);
typedef int (*ctk_write_chunk_fn)(void *user, int64_t t0, int64_t nt, const int32_t *src);
int ctk_track_stream_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                         double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps);
int ctk_track_stream_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                         double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps);
int ctk_track_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn reader,
                        void *reader_user, const double *thr, int cmp_op, const float *wrow, double overlap, int persistence, int twosided,
                        ctk_write_chunk_fn writer, void *writer_user, int64_t *n_tracked, int64_t chunk_steps);
/* ... with segment breaks (semantics: ctk_set_segments): starts[0] = 0, strictly increasing, the last one below T (CTK_E_INVALID
 * otherwise, and for a handle with sticky segments set).  Chunks and segments are unrelated: a break may fall inside a chunk, on a
 * chunk boundary, and a chunk may be shorter than a segment.  thr == NULL (the handle's threshold field) is taken as in
 * ctk_track_stream_*.  nseg == 0 or starts == {0} is ctk_track_stream_*, bit for bit, with the same kernels. */
int ctk_track_stream_seg_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                             double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps,
                             const int64_t *starts, int64_t nseg);
int ctk_track_stream_seg_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                             double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps,
                             const int64_t *starts, int64_t nseg);
int ctk_track_stream_seg_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn reader,
                            void *reader_user, const double *thr, int cmp_op, const float *wrow, double overlap, int persistence,
                            int twosided, ctk_write_chunk_fn writer, void *writer_user, int64_t *n_tracked, int64_t chunk_steps,
                            const int64_t *starts, int64_t nseg);
/* times of the last streaming call: {reader callbacks, writer callbacks, input phase, output phase} in ms */
int ctk_stream_times(ctk_handle *h, double *ms4);

/* ---- timing (HIP events on the handle's stream) ----------------------------------------------- */
#define CTK_K_THRESHOLD 0
#define CTK_K_SCAN      1
#define CTK_K_LABEL2D   2
#define CTK_K_OVERLAP   3
#define CTK_K_EXTENT    4
#define CTK_K_RUNLABEL  5
#define CTK_K_RELABEL   6
#define CTK_K_RESOLVE   7      /* device resolver: filter passes, 3-D union-find, ids, boxes */
#define CTK_K_RESOLVE2  8      /* device resolver: final id per component                     */
#define CTK_K_COUNT     9
#define CTK_T_HOST_RESOLVE 10  /* host: sequential seam driver (or ctk_resolve on the host path) */
#define CTK_T_D2H          11  /* downloads                                            */
#define CTK_T_H2D          12  /* uploads                                              */
#define CTK_T_TOTAL        13
#define CTK_NTIMERS        14
/* level 0: no HIP events; 1: events around ONE of the two pixel-streaming kernels in every second pass (k_threshold in passes
 * 0, 4, 8 ... of the handle, k_relabel in passes 2, 6, 10 ...; whatever was not timed reads 0 for that pass) -- what bench.py keeps
 * on during its timed region; 2: events around every kernel group (each record is a ~5 us command on the stream) */
int ctk_set_timing(ctk_handle *h, int level);
/* event times summed over the calls since the last reset, and the number of calls that measured each group ([CTK_NTIMERS] each;
 * either may be NULL): what a loop that times many passes reads ONCE at its end instead of ctk_get_timings after every call */
int ctk_get_timing_sums(ctk_handle *h, double *sums, int64_t *counts, int reset);
/* workload statistics of the last call (for bench reports: cost depends on them) */
#define CTK_S_RUNS          0   /* foreground runs in the shard                         */
#define CTK_S_MAX_RUNS_STEP 1   /* most runs in one timestep                            */
#define CTK_S_COMPONENTS    2   /* 2-D components (no wrap)                             */
#define CTK_S_PAIRS         3   /* co-occurrence records                                */
#define CTK_S_SEAM_ROWS     4   /* seam rows handed to the sequential driver            */
#define CTK_S_LABELS        5   /* fresh 3-D labels                                     */
#define CTK_S_OPS           6   /* recorded bbox-confined relabel operations            */
#define CTK_S_FILTER_PASSES 7   /* passes of the overlap-filter iteration that ran      */
#define CTK_S_HOST_PATH     8   /* 1 if the call fell back to the host resolver         */
#define CTK_S_UPAIRS        12  /* co-occurrence records that bypassed the LDS hash table   */
#define CTK_S_PAIR_REGROW   13  /* times the pair table had to be regrown (host path)       */
#define CTK_S_FILTER_ROUNDS 14  /* rounds of filter passes (convergence is checked per round) */
#define CTK_S_EXACT_FIXUPS  16  /* overlap decisions re-evaluated with numpy-order sums on the host (see CTK_S_AMBIGUOUS)  */
#define CTK_S_AMBIGUOUS     15  /* > 0: an overlap decision used an area sum that had to be ROUNDED (components touching a pole row,
                                   whose weight is ~2^-20 of the others) and came out within 8 ulp of the threshold; numpy's pairwise
                                   float64 summation may land on the other side there (only with exact ties: blocky test fields,
                                   overlap = 1.0).  Device path: 0/1 flag; host resolver: the number of such decisions. */
#define CTK_S_HOST_REASON   18  /* why a one-call track left the fused device path: bit 0 the co-occurrence table had to be regrown, bit 1
                                   the overlap filter needed more than 240 passes (both: host resolver, CTK_S_HOST_PATH = 1); 4 = decisions
                                   on rounding boundaries, re-evaluated on the device through the time-shard path with one rank;
                                   bit 3 (8) = a bounded inter-workgroup wait gave up, the resolution was repeated with one launch per
                                   filter pass */
#define CTK_S_SHARED_ROWS   17  /* time-sharded path: seam candidate groups shared between shards (driven on every rank)        */
#define CTK_S_RELABEL_KERNEL 19    /* which write kernel ran: 6 = k_relabel_sparse behind k_flag_zero, 5 = k_relabel_v5, 4 = k_relabel_v4, 0 = generic k_relabel, -1 = none (run transfer) */
#define CTK_S_FUSED         20    /* 1: the one-call pass ran without a host hand-off (device seam driver, one synchronisation) */
#define CTK_S_X4_SPECULATED 21    /* time-sharded path: 1 if the boundary records of the 3-D labelling travelled with the last round of
                                   * the overlap filter's exchange (one all-gather less) */
#define CTK_S_RLE_OUT       22    /* host-array entries: 0 = the result was written by k_relabel and copied densely; n > 0 = it travelled as
                                   * run tables and was expanded on the host, n - 1 blocks of timesteps (those holding complex
                                   * components) went through the write kernel */
#define CTK_S_MASK_TRIES    23    /* allocations of the bit mask that were checked against the slab when it was last (re)allocated (0: not checked); sticky */
#define CTK_S_MASK_RATIO    24    /* 1000 x (threshold kernel on the kept mask / the same kernel without its stores), from that check; sticky */
#define CTK_NSTATS          25    /* what ctk_get_stats writes: FROZEN at 25 (a host built against this header is never overrun by a newer library) */
int ctk_get_stats(ctk_handle *h, int64_t *out /* [CTK_NSTATS] */);
/* statistics added after that are read with an explicit length: writes min(n, CTK_NSTATS_ALL) entries, returns CTK_OK */
#define CTK_S_MASK_CHECK_US 25    /* host time of the last mask placement check, microseconds (bounded: at most one other allocation); sticky */
#define CTK_S_MASK_SPACER_MB 26   /* device memory that check held as a spacer while it ran (freed before the call went on), MB; sticky */
#define CTK_S_LABEL_FORMS   27    /* bit mask of the 2-D labelling kernels the last call launched (the speculative launch and the one after
                                   * the run scan together): 1 k_label2d_lds<4096,512,-1,1024> (one launch for every timestep),
                                   * 2 <768,272,-1,256,256>, 4 <832,240,-1,256,256>, 8 <1024,288,-1,256>, 16 <1024,288,768,256>,
                                   * 32 <1024,288,832,256>, 64 <2048,512,1024,512>, 128 <4096,512,2048,1024>, 256 k_label2d_glb;
                                   * 512: a speculative launch ran on too small run buffers and was discarded */
#define CTK_S_OVERLAP_FORM  28    /* the last k_overlap launch: OVB * 10000 + THREADS * 10 + waves per SIMD, + 1000000 for the build that
                                   * reads segment breaks */
#define CTK_S_ROWCOUNT_THREADS 29 /* threads per workgroup of the last k_rowcount launch (512, 256 or 128) */
#define CTK_S_FILTER_FORMS  30    /* bit mask of the overlap-filter, union and rank kernels the last one-call track launched (the fused pass
                                   * and, if it fell off, the synchronous resolver together): 1 k_rs_pass_blk, 2 its SEG build,
                                   * 4 k_rs_pass_blk_2pc, 8 its SEG build, 16 k_rs_pass (one launch per pass) in the fused pass, 32 its SEG
                                   * build, 64 k_rs_pass in the synchronous resolver, 128 its SEG build, 256 k_rs_unite_slots, 512 k_rs_unite,
                                   * 1024 the fused pass ranked in one launch (k_fz_rank_mark), 2048 in three (k_rs_rank, k_rs_labels,
                                   * k_fz_mark); bits 16 and up: the filter passes the fused pass launched (NP) */
#define CTK_S_EXTENT_FORM   31    /* the last k_extent launch: its threads per workgroup (64, 128 or 256), or 1024 for k_extent_blk */
#define CTK_S_RUNVAL_FORM   32    /* the last k_run_values launch: threads per workgroup * 10, + 1 if it built the chunk-ordered copy of the
                                   * run values (CTK_CV per chunk) for the write kernel */
#define CTK_S_RELABEL_SHAPE 33    /* the write launches of the last call, ORed: rows per chunk (rb) << 24 | rows per LDS image of
                                   * k_relabel_v5 (sub; 0 for the other kernels) << 8 | 1 a k_relabel_v5 launch loaded its tables in one
                                   * batch (tab_batched), 2 one with three loops, 4 / 8 / 16 its LDS budget was 20 / 24 / 28 KB.  A streamed
                                   * call launches once per block of timesteps: rb and sub are those of the whole shard, the flags of all */
#define CTK_S_COUNT_FORM    34    /* bit mask of the alive-count kernels the last call launched: 1 k_count_alive_f, 2 k_count_alive_1,
                                   * 4 k_count_alive in the fused pass; 8 k_count_alive_1, 16 k_count_alive in ctk_shard_write */
#define CTK_S_DEVICE_CUS    35    /* compute units of the handle's device (the k_rs_pass_blk_2pc edge: more workgroups than CUs) */
#define CTK_S_ROWCOUNT_GROUPS 36  /* row groups the last k_rowcount launch kept in flight: the RCU of the instance k_rowcount<RCU> it ran (4, 6
                                   * or 8); 0 where the plane took one of the kernel's other two forms (more than 64 words a row, or
                                   * more than 2048 rows), which do not read it */
#define CTK_NSTATS_ALL      40
int ctk_get_stats_n(ctk_handle *h, int64_t *out, int n);
int ctk_get_timings(ctk_handle *h, double *ms /* [CTK_NTIMERS] */);

/* ---- thin device-memory helpers so that a ctypes host needs no other HIP binding -------------- */
int ctk_dev_malloc(ctk_handle *h, void **p, size_t nbytes);
int ctk_dev_free(ctk_handle *h, void *p);
int ctk_memcpy_h2d(ctk_handle *h, void *dst_dev, const void *src, size_t nbytes);
int ctk_memcpy_d2h(ctk_handle *h, void *dst, const void *src_dev, size_t nbytes);
int ctk_sync(ctk_handle *h);
/* Result buffers without first-touch page faults for the host-array entries (ctk_track_f32 / _f64 / ctk_track_resident): a `flag`
 * pointer into memory from ctk_host_alloc (pinned, CPU-cacheable) or into a caller array registered with ctk_host_register is
 * recognised and filled with ONE DMA at PCIe rate; an ordinary (pageable, usually fresh) array goes through eight threads draining
 * pinned bounce buffers, bound by the page faults of its first touch.  What replaces np.empty at contrack.py:776-791 when results
 * are produced in a loop (ensemble members): contrack_amd/_native.py recycles such blocks. */
int ctk_host_alloc(ctk_handle *h, void **p, size_t nbytes);
int ctk_host_free(ctk_handle *h, void *p);
/* How the result of the host-array entries crosses PCIe.  1 (default; CTK_RLE_OUT=0 in the environment turns it off): as the
 * pass's own run tables -- the bit mask, the first run of every row and the final value of every foreground run (k_run_values),
 * 1/23 of the dense int32 slab at 2707 x 181 x 360 --, expanded into `flag` by sixteen host threads; the write kernel does not
 * run (blocks of timesteps that hold a "complex" component, whose pixels are folded one by one, still go through it).  Every
 * value is computed on the device; the host only decodes.  0: k_relabel writes the dense slab in HBM and it is copied (the
 * scheme above).  -1: back to the environment's choice.  The device-resident entries always write `flag_dev` densely.
 * CTK_S_RLE_OUT reports what a call did.  (contrack.py:776-791: where the reference materialises `flag`) */
int ctk_set_result_transfer(ctk_handle *h, int mode);
int ctk_host_register(ctk_handle *h, void *p, size_t nbytes);
int ctk_host_unregister(ctk_handle *h, void *p);
void *ctk_stream(ctk_handle *h);                          /* hipStream_t */
int ctk_dev_memset(ctk_handle *h, void *p_dev, int byte, size_t nbytes);

/* ---- next row N1: contrack.run_lifecycle reductions (contrack/contrack.py:798-906) --------------------------
 * One row per (time step, flag id != 0) of an int32 flag slab (time, lat, lon) and a field of the same shape:
 *   area  = np.sum(weight_grid[flag == id])                       contrack.py:874   (exact, rounded once)
 *   swv   = np.sum(weight_grid[...] * field[...])                 contrack.py:875   (float64)
 *   swvy, swvx = the two numerators of ndimage.center_of_mass(field * weight_grid, flag, [id])   contrack.py:892
 *   shift = column that becomes x = 0 when the id touches both seam columns (np.roll by -shift,
 *           contrack.py:880-889; swvx is taken in the rolled frame); -1 if not rolled; -2 if the id occupies a
 *           single column (the reference's argmax of an empty diff raises there)
 * The host finishes with  intensity = swv / area,  com = (swvy / swv, swvx / swv),  int() and the coordinate
 * look-ups (contrack.py:886-895).  ctk_lifecycle_* computes and keeps the rows in the handle (sorted by
 * (label, t) like the reference's frame, contrack.py:906) and returns their number; ctk_lifecycle_rows copies
 * them out.  wrow: float32 row weights, contrack.py:847-848.  Every byte of flag / field is read once (strips of 256 columns x
 * 64 rows per workgroup); a time step with more ids than the tables of that form hold (128, or 4 that cross the seam) is redone
 * by a one-workgroup-per-time-step kernel in passes over residue classes of the ids: no limit.
 * pad: the rows that hold the id, first | last << 16 (internal: bounds the scans of ctk_lifecycle_exact).
 * Host entries with field = NULL take the anomaly slab that ctk_anom_* left resident in HBM (same shape and type). */
typedef struct ctk_life_row {
    int32_t t, label, shift, pad;
    double area, swv, swvy, swvx;
} ctk_life_row;
int ctk_lifecycle_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *field_dev, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows);
int ctk_lifecycle_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *field_dev, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows);
int ctk_lifecycle_f32(ctk_handle *h, const int32_t *flag, const float *field, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows);
int ctk_lifecycle_f64(ctk_handle *h, const int32_t *flag, const double *field, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows);
int ctk_lifecycle_rows(ctk_handle *h, ctk_life_row *rows, int64_t cap);
/* The sums above are float64 but not in the reference's summation order; that shows only where a result sits on a rounding
 * boundary (a centre of mass that is an integer up to rounding, a value at the edge of two decimals).  The caller picks those rows
 * (indices into the sorted rows) and gets them in the reference's own orders: np.sum (pairwise) for weight_grid[mask] and
 * weight_grid[mask] * variable[mask] (contrack.py:874-875), np.bincount (sequential, raster order of the rolled plane) inside
 * ndimage.center_of_mass (:886 / :892).  Valid until the next ctk_lifecycle_* call on the handle, and only while the slabs of that
 * call are still what it left: the host-array entries keep theirs in the handle's staging buffers (the field = NULL form reads the
 * resident anomaly slab), so any later entry that takes a host array or streams through the handle, any ctk_anom_* call after a
 * field = NULL call, and ctk_release_io make ctk_lifecycle_exact return CTK_E_STATE ("a later call ... overwrote or released the
 * slabs") until the next resident ctk_lifecycle_* call.  Entries that work on the caller's device pointers alone (*_dev) do not.
 * For the *_dev entries the slabs stay the caller's: they must be alive and unchanged when ctk_lifecycle_exact runs. */
typedef struct ctk_life_exact {
    double area, swv, s, sy, sx;       /* np.sum(w), np.sum(w * v), sum p, sum p * y, sum p * x'   (p = v * w) */
} ctk_life_exact;
int ctk_lifecycle_exact(ctk_handle *h, const int64_t *row_idx, int64_t n, ctk_life_exact *out);
/* ctk_lifecycle_stream_*: the same rows with both slabs passing through chunk-sized device buffers -- two chunks of flags, two of
 * the field and the per-time-step tables of one chunk are all the device holds, so a flag written by ctk_track_stream_* can be
 * consumed.  Host arrays (_f32 / _f64) or readers (_cb: ctk_read_chunk_fn, contract and threading rules of ctk_track_stream_cb's
 * reader; called once per chunk in increasing t0, flag_reader -- int32 elements -- before field_reader, each filling pinned memory
 * the library owns).  chunk_steps: time steps per chunk, 0: about 256 MB of field; chunk_steps >= T is one chunk.  The upload of
 * chunk k+1 runs under the reductions of chunk k.
 * The rounding-boundary rows are chosen while their chunk is still on the device: after a chunk's reductions `pick` gets that
 * chunk's rows, sorted by (label, t) with t GLOBAL, fills idx[0..*nidx) with ascending indices into them and returns 0 (nonzero
 * aborts the call with CTK_E_INVALID; pick = NULL: no rows); those rows are re-evaluated as by ctk_lifecycle_exact.
 * After the call the handle holds all rows as after ctk_lifecycle_* (ctk_lifecycle_rows); ctk_lifecycle_stream_exact copies out the
 * *nexact picked rows as ascending indices into that sorted order with their records (cap: room in both arrays).
 * ctk_lifecycle_exact returns CTK_E_STATE after a streamed call -- the slabs are gone -- until the next resident call.  A failing
 * reader, a failing pick or a device error leaves the handle usable.  ctk_stream_times reports the readers and the input phase. */
typedef int (*ctk_life_pick_fn)(void *user, const ctk_life_row *rows, int64_t n, int64_t *idx, int64_t *nidx);
int ctk_lifecycle_stream_f32(ctk_handle *h, const int32_t *flag, const float *field, int64_t T, int ny, int nx, const float *wrow, int64_t chunk_steps,
                             ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact);
int ctk_lifecycle_stream_f64(ctk_handle *h, const int32_t *flag, const double *field, int64_t T, int ny, int nx, const float *wrow, int64_t chunk_steps,
                             ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact);
int ctk_lifecycle_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader,
                            void *flag_user, ctk_read_chunk_fn field_reader, void *field_user, const float *wrow, int64_t chunk_steps,
                            ctk_life_pick_fn pick, void *pick_user, int64_t *nrows, int64_t *nexact);
int ctk_lifecycle_stream_exact(ctk_handle *h, int64_t *row_idx, ctk_life_exact *out, int64_t cap);

/* ---- next rows N2 / N3: the producer of the slab on the device ----------------------------------------------------------
 * ctk_anom_*: contrack.calc_clim / calc_anom (contrack/contrack.py:458-581) on a host slab x (T, ny, nx):
 *   clim_raw[g] = mean over the timesteps t with group[t] == g, NaNs skipped           (groupby(...).mean, :483)
 *   clim[g]     = mean of clim_raw over the centred window of `window` groups; NaN (window beyond the axis, or NaN data) ->
 *                 mean of the last `window` groups of clim_raw                         (rolling(center=True).mean().fillna, :487-489)
 *   anom[t]     = mean over the centred window of `smooth` timesteps of x[j] - clim[group[j]]; NaN where the window leaves the
 *                 axis or holds a NaN                                                  (:568-570)
 *   centred window of w around i: [i - w / 2, i + (w - 1) / 2].
 * group: T ids in [0, ngroups) (the class maps the time coordinate's dayofyear / month ... to them).  clim_in (optional,
 * [ngroups][ny][nx]): use this climatology instead of computing one (the `clim=` argument).  anom_out / clim_out: optional host
 * outputs.  keep_resident != 0: the anomaly slab stays in HBM and ctk_track_resident / ctk_percentile_* (x = NULL) run on it
 * without another host-to-device copy.  Sums in float64, results in the slab's dtype (xarray's dtype rules).  T <= 2^31 - 1
 * (CTK_E_INVALID beyond, checked before x is read): the steps are int32 in the group lists, as for ctk_anom_seg_*.  The xarray calls
 * themselves cannot be run in the build container: checked against the numpy restatement oracle/anom_port.py (parity unpinned). */
int ctk_anom_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                 const float *clim_in, float *anom_out, float *clim_out, int keep_resident);
int ctk_anom_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                 const double *clim_in, double *anom_out, double *clim_out, int keep_resident);
/* ctk_anom_* over independent time segments (ensemble members, seasons): starts / nseg follow the rules of ctk_set_segments (0 first,
 * strictly increasing) with the last start below T -- CTK_E_INVALID with a message otherwise, the handle stays usable; NULL / 0 is
 * one segment.  The climatology is unchanged: pooled over every timestep of a group whatever its segment, summed in rising t.  The
 * smoothing stays inside a segment: anom[t] is the mean over [t - smooth / 2, t + (smooth - 1) / 2] only if that window lies inside t's
 * segment, NaN otherwise (as ctk_anom_* where the window leaves the axis).  Sums and rounding places are ctk_anom_*'s: one segment
 * gives its bits.  keep_resident as in ctk_anom_*.  Each step of x, group and clim is read once per tile of output steps (plus the
 * smooth - 1 steps around the tile) instead of `smooth` times per output while the last `smooth` raw anomalies of a pixel fit the
 * workgroup's LDS (float32: smooth <= 32, float64: <= 16; ctk_anom_plan, csrc/ctk_forms.h), a plain form beyond. */
int ctk_anom_seg_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                     const float *clim_in, float *anom_out, float *clim_out, int keep_resident, const int64_t *starts, int64_t nseg);
int ctk_anom_seg_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                     const double *clim_in, double *anom_out, double *clim_out, int keep_resident, const int64_t *starts, int64_t nseg);
/* ... streamed: the slab passes through chunk-sized device buffers and is never held in HBM -- a few chunks, ngroups * ny * nx * 12
 * bytes of float64 sums and int32 counts, and the climatology.  ctk_anom_stream_f32 / _f64: host array in, host array out (anom_out
 * NULL: the climatology only); ctk_anom_stream_cb: a reader (ctk_read_chunk_fn, elements of elem_bytes) and a writer of values, which
 * receives the anomalies of [t0, t0 + nt) in pinned memory valid during the call (writer NULL: the climatology only).
 *   pass 1 (skipped when clim_in is given): the chunks in increasing t0 are added into the sums; group means, then the rolling mean;
 *   pass 2 (skipped without a sink): the chunks again; the smooth - 1 steps between neighbouring chunks stay on the device.
 * The reader sees two passes without clim_in and one with it, each over non-overlapping ranges in increasing t0 that cover every
 * step once; the writer gets every step once in increasing t0 (its chunks lag the reader's by (smooth - 1) / 2 steps, the last one
 * closes the gap).  A nonzero return of either callback ends the call with CTK_E_INVALID.  chunk_steps = 0: about 256 MB per chunk;
 * a chunk_steps below smooth - 1 is raised to smooth - 1.  Result: ctk_anom_seg_* on the whole slab bit for bit, for every chunk_steps. */
typedef int (*ctk_write_values_fn)(void *user, int64_t t0, int64_t nt, const void *src);
int ctk_anom_stream_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                        const int64_t *starts, int64_t nseg, const float *clim_in, float *anom_out, float *clim_out, int64_t chunk_steps);
int ctk_anom_stream_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                        const int64_t *starts, int64_t nseg, const double *clim_in, double *anom_out, double *clim_out, int64_t chunk_steps);
int ctk_anom_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user,
                       const int32_t *group, int ngroups, int window, int smooth, const int64_t *starts, int64_t nseg, const void *clim_in,
                       void *clim_out, ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps);
int ctk_resident_anom(ctk_handle *h, int64_t *T, int *ny, int *nx, int *is_f64);       /* T = -1: nothing resident */
/* The resident slot holds THE FIELD TO TRACK, whichever producer wrote it last: the anomalies of ctk_anom_*, the gradient-reversal
 * index of ctk_reversal_* or the local wave activity of ctk_lwa_* (below), each with keep_resident.  ctk_resident_anom reports its shape.
 * Identity of the resident slab: changes whenever one of those calls writes the slot or ctk_release_io drops it.  Remember it
 * after the call that left YOUR slab resident and use the slab only while it is unchanged. */
int ctk_resident_anom_generation(ctk_handle *h, uint64_t *generation);
/* ctk_track_f32 / _f64 on the resident anomaly slab (flag: host int32 (T, ny, nx)) */
int ctk_track_resident(ctk_handle *h, const double *thr, int cmp_op, const float *wrow, double overlap, int persistence, int twosided,
                       int32_t *flag, int64_t *n_tracked);
/* README.rst:150-151: anom.sel(latitude=rows y0..y1-1).quantile(q, dim='time').mean() -- per grid point the exact q-quantile over
 * time (numpy's linear interpolation, NaNs skipped), then the mean over the band.  x = NULL: the resident anomaly slab.
 * T <= 2^31 - 1 (CTK_E_INVALID beyond, checked before x is read), as for the two entries below. */
int ctk_percentile_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, double q, double *out);
int ctk_percentile_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, double q, double *out);
/* README.rst:235-240 (the threshold "defined as the 10th percentile of the ... anomaly distribution over 30-90N at each calendar day"),
 * the producer of the 1-D dayofyear threshold that contrack.py:648-661 consumes.  Pooled, windowed, exact: for every group g
 *   pool(g) = { x[t, y, :] : y0 <= y < y1, group[t] in { (g + d) mod ngroups : -(window / 2) <= d <= (window - 1) / 2 } }
 *   out[g]  = np.nanquantile(pool(g) as float64, q)         (method 'linear', NaNs skipped; an empty pool gives NaN)
 * The window is centred as calc_clim's and taken circularly over the groups (1 January sees late December); window >= ngroups pools
 * every timestep for every group; a group without a timestep still gets the value of its window.  group: T host ints in
 * [0, ngroups).  x = NULL: the resident anomaly slab (shape and dtype must match).  The band is read 4 times (float32) or 7 times
 * (float64), whatever ngroups and window are.  Device memory: ngroups x window (1 when window >= ngroups) histograms of 8 KB,
 * 93 MB at 366 x 31.  CTK_E_INVALID: bad arguments (checked before any device call), a window below ngroups but above 1024, more
 * than 2^19 histograms (4 GB), or a group whose timesteps x band values reach 2^32 (its counters are uint32). */
int ctk_percentile_groups_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                              double q, double *out /* ngroups */);
/* README.rst:235-240 / contrack.py:648-661: the same on a float64 slab (64-bit keys: 7 reads of the band) */
int ctk_percentile_groups_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                              double q, double *out /* ngroups */);
/* The per-grid-point twin: the threshold FIELD over (group, latitude, longitude) that ctk_set_threshold_field consumes -- the
 * q-quantile over time AT EACH GRID POINT of rows [y0, y1), per group, pooled over the same centred, circular window of groups:
 *   pool(g, y, x') = { x[t, y, x'] : group[t] in { (g + d) mod ngroups : -(window / 2) <= d <= (window - 1) / 2 } }
 *   out[g][y - y0][x'] = np.nanquantile(pool as float64, q)  (method 'linear', NaNs skipped; an empty or all-NaN pool gives NaN)
 * exactly: infinities, signed zeros and subnormals as numpy's _lerp treats them.  x = NULL: the resident anomaly slab.  Two forms
 * (ctk_pfield_plan, csrc/ctk_forms.h; csrc/ctk_pfield.hip): while the longest pool has at most 4 783 timesteps (float32; 2 391 for
 * float64) a workgroup keeps the pool of its 32, 16 or 8 pixels in LDS as a ring of timesteps and walks the groups, so the slab
 * is read 1 + window / ngroups times; longer pools are selected straight from HBM, group by group.  window >= ngroups: one plane
 * is selected and replicated.  Device memory: the ngroups planes.  CTK_E_INVALID: bad arguments (checked before any device
 * call), T >= 2^31 (pool counts are uint32), ngroups x band pixels / 8 beyond 2^31 - 1. */
int ctk_percentile_field_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                             double q, double *out /* ngroups * (y1 - y0) * nx */);
int ctk_percentile_field_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                             double q, double *out /* ngroups * (y1 - y0) * nx */);
/* contrack.py:9-10 ("take 90th percentile or std_dev from anom field for threshold"), the std_dev half: the temporal standard deviation
 * AT EACH GRID POINT of rows [y0, y1), per group, over the pool of ctk_percentile_field_* TAKEN IN TIME ORDER,
 *   pool(g, y, x') = ( x[t, y, x'] : t rising, group[t] in { (g + d) mod ngroups : -(window / 2) <= d <= (window - 1) / 2 } )
 * (x[np.isin(group, members)]: window >= ngroups pools every timestep for every group -- one plane is computed and replicated), as
 * this two-pass loop in float64, which is the statement:
 *   s = 0; c = 0;  for v in pool:  (skipna and v is NaN) ? v = 0 : c += 1;   s = s + v
 *   m = s / (double)c
 *   q = 0;         for v in pool:  skip if (skipna and v is NaN);  d = v - m;  q = q + d * d       (product and sum rounded separately)
 *   out_std = c - ddof > 0 ? sqrt(q / (double)(c - ddof)) : NaN;   out_mean = m;   out_n = c
 * On C-contiguous (n, ny, nx) pools of two or more grid points these are the bits of np.nanstd(pool, axis=0, ddof=ddof) (skipna) and
 * np.std(pool.astype(np.float64), axis=0, ddof=ddof) (numpy 2.2).  A ONE-point plane is different: numpy reduces it pairwise and the
 * loop does not match it -- the loop is what this entry computes.  One NaN rule for both modes, np.nanstd's: c - ddof <= 0 gives NaN
 * (plain np.std gives inf there when q > 0); an empty or all-NaN pool gives NaN in out_std and out_mean.  Infinities need no rule:
 * inf - inf makes the NaN numpy makes.  x = NULL: the resident anomaly slab (shape and dtype must match).  out_mean / out_n may be
 * NULL.  One kernel (csrc/ctk_std.hip) holds the accumulators of every group for 32, 16 or 8 grid points in LDS (ctk_std_plan,
 * csrc/ctk_forms.h) and gives each ONE writing thread, so each sees its values in time order; the slab is read twice.  Device memory:
 * the ngroups planes asked for (8 + 8 + 4 bytes per value), T + ngroups ints.  CTK_E_INVALID: bad arguments (checked before any device
 * call), ddof < 0, T >= 2^31 (counts are uint32), a window below ngroups with more than 998 groups (skipna) or 1 248 groups (without):
 * the accumulators of 8 grid points no longer fit in LDS and there is no other form. */
int ctk_std_field_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                      int ddof, int skipna, double *out_std /* ngroups * (y1 - y0) * nx */, double *out_mean /* the same, or NULL */,
                      uint32_t *out_n /* the same, or NULL */);
int ctk_std_field_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                      int ddof, int skipna, double *out_std /* ngroups * (y1 - y0) * nx */, double *out_mean /* the same, or NULL */,
                      uint32_t *out_n /* the same, or NULL */);

/* ---- the vertical mean over a pressure band (README.rst:235-240: "The PV fields are vertically averaged between 500-150 hPa") ----
 * The first step of the README's third recipe, the producer of the slab ctk_anom_* works on.  The reference has no function for it;
 * tests/level_util.py is the numpy statement of what follows.
 * x: (steps, nlev, ny, nx), float32 or float64, C-contiguous.  weights: nlev float64, each finite and >= 0, at least one > 0.
 * A level with weights[l] == 0 is NOT SELECTED: never read, never uploaded, a NaN on it has no effect.  Per step s and pixel p, over
 * the nsel selected levels in rising l, in float64:
 *     acc = 0.0 ; ws = 0.0
 *     acc = acc + weights[l] * (double)x[s][l][p]     -- a rounded multiply, then a rounded add: no fused multiply-add
 *     ws  = ws + weights[l]
 *     out[s][p] = (dtype)(acc / ws)                    -- float64 divide, then one rounding to x's dtype
 * skipna = 0: a NaN on any selected level gives NaN.  skipna != 0: a level whose value is NaN contributes to neither acc nor ws of
 * that pixel; all selected levels NaN gives NaN (0 / 0).  The bits are those of that loop.  With trapezoid weights over the pressure
 * coordinate (contrack.level_weights) the mean is the integral of x dp over the band / its depth.
 * At most 4096 selected levels (CTK_E_INVALID beyond).  CTK_E_INVALID with a message, the handle usable: a null pointer, a size
 * below 1, a negative or non-finite weight, all weights zero, chunk_steps < 0, nothing to produce (out NULL and keep_resident 0).
 *
 * ctk_level_mean_f32_dev / _f64_dev: x and out (steps, ny, nx) in device memory; the unselected levels are skipped in place.
 * ctk_level_mean_f32 / _f64 and ctk_level_mean_stream_f32 / _f64: host arrays (out may be NULL with keep_resident).  Only the
 * selected levels are uploaded, neighbouring ones as one strided copy per chunk; the device holds two compact chunks
 * (nt, nsel, ny, nx) and two output chunks, never steps x nlev planes: chunk k + 1 travels in while the kernel reduces chunk k and
 * chunk k - 1 leaves.  chunk_steps = 0 (and the entries without it): about 256 MB of input per chunk.  Same bits for every
 * chunk_steps.
 * ctk_level_mean_stream_cb: the reader fills (nt, nsel, ny, nx) -- the SELECTED levels only, in rising level order -- for the steps
 * [t0, t0 + nt); weights_sel are their nsel non-zero weights.  writer (may be NULL with keep_resident) receives the means of
 * [t0, t0 + nt) in pinned memory valid during the call.  Both are called in increasing t0, once per chunk; a non-zero return ends
 * the call with CTK_E_INVALID and leaves nothing in flight.
 * keep_resident != 0: the mean slab stays in HBM in a buffer of its own (the tracking calls do not touch it) for
 * ctk_anom_seg_resident.  ctk_resident_level_mean: its shape (steps = -1: nothing resident).  Its identity
 * (ctk_resident_level_mean_generation) changes with every ctk_level_mean_* call and with ctk_release_io, which also frees it. */
int ctk_level_mean_f32(ctk_handle *h, const float *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out, int keep_resident);
int ctk_level_mean_f64(ctk_handle *h, const double *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out, int keep_resident);
int ctk_level_mean_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out_dev);
int ctk_level_mean_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out_dev);
int ctk_level_mean_stream_f32(ctk_handle *h, const float *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out,
                              int64_t chunk_steps, int keep_resident);
int ctk_level_mean_stream_f64(ctk_handle *h, const double *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out,
                              int64_t chunk_steps, int keep_resident);
int ctk_level_mean_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t steps, int nsel, int ny, int nx, ctk_read_chunk_fn reader,
                             void *reader_user, const double *weights_sel, int skipna, ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps,
                             int keep_resident);
int ctk_resident_level_mean(ctk_handle *h, int64_t *steps, int *ny, int *nx, int *is_f64);       /* steps = -1: nothing resident */
int ctk_resident_level_mean_generation(ctk_handle *h, uint64_t *generation);
/* ctk_anom_seg_f32 / _f64 with x taken from the resident mean: shape and dtype are the slab's, clim_in / anom_out / clim_out hold
 * that dtype; the same kernels, the same bits, the same keep_resident (of the ANOMALY).  CTK_E_INVALID if no mean is resident. */
int ctk_anom_seg_resident(ctk_handle *h, const int32_t *group, int ngroups, int window, int smooth, const void *clim_in, void *anom_out, void *clim_out,
                          int keep_resident, const int64_t *starts, int64_t nseg);

/* ---- the reversal of the meridional height gradient: the second family of blocking indices -------------------------------------
 * Tibaldi & Molteni (1990) in one dimension, Scherrer et al. (2006) and Davini et al. (2012) in two.  The reference has no function
 * for it; tests/reversal_util.py is the numpy statement of what follows.
 * x: (steps, ny, nx), float32 or float64, C-contiguous -- geopotential height in metres, say.  The caller describes the latitude
 * coordinate with a ROW TABLE of ny entries (contrack.reversal_rows builds it from lat[ny], a distance delta in degrees and the
 * gradient limits ghgs, ghgn, ghgs2 per degree):
 *     eq[j]   the row nearest to lat[j] - s * delta (s = +1 north of the equator, -1 south of it and on it): the equatorward partner;
 *             -1: row j is INACTIVE (outside the latitude band or the hemisphere asked for, or a partner is missing)
 *     po[j]   the row nearest to lat[j] + s * delta: the poleward partner
 *     eq2[j]  the row nearest to lat[j] - 2 * s * delta (the third criterion of Davini et al.; eq2 and tS2 NULL: two criteria)
 *     dE[j] = |lat[j] - lat[eq[j]]| in degrees, the ACTUAL distance of the two rows, finite and > 0
 *     tS[j] = ghgs * dE[j],  tN[j] = ghgn * |lat[po[j]] - lat[j]|,  tS2[j] = ghgs2 * |lat[eq[j]] - lat[eq2[j]]|: the limits, finite
 * Per step and pixel of an active row, in float64 with no fused multiply-add (z[r] the pixel's column in row r):
 *     dS = (double)z[j] - (double)z[eq[j]] ;  dN = (double)z[po[j]] - (double)z[j] ;  dS2 = (double)z[eq[j]] - (double)z[eq2[j]]
 *     blocked = dS > tS[j]  and  dN < tN[j]  [and dS2 < tS2[j]]          -- a NaN anywhere: every compare false, not blocked
 *     mask == 0 ('gradient'): out = blocked ? (dtype)(dS / dE[j]) : 0    -- the equatorward gradient per degree, one rounding
 *     mask != 0:              out = blocked ? 1 : 0
 * The compares use no division; the divide happens only where a pixel is blocked.  Inactive rows are 0 and nothing of x is read for
 * them.  out has x's shape and dtype: ctk_track_* with threshold 0 and the op '>' tracks it as it is.
 * CTK_E_INVALID with a message, the handle usable: a null pointer, a size below 1, steps < 1, a partner index outside [-1, ny), an
 * active row with a negative partner, a dE that is not finite and > 0, a limit that is not finite (both on active rows), eq2 without
 * tS2 or the reverse, a plane of 2^31 pixels or more, chunk_steps < 0, nothing to produce (out NULL and keep_resident 0).
 *
 * ctk_reversal_f32_dev / _f64_dev: x and out in device memory.
 * ctk_reversal_f32 / _f64: host arrays (out may be NULL with keep_resident).  Of every plane only the rows some active row reads
 * are uploaded (one strided copy per chunk) and only the rows the active rows span are downloaded; the rest of out is zeroed on the
 * host.  Two input and two output chunks: chunk k + 1 travels in while the kernel works on chunk k and chunk k - 1 leaves.
 * chunk_steps = 0: about 256 MB of input per chunk.  Same bits for every chunk_steps.
 * ctk_reversal_stream_cb: the reader fills whole planes (nt, ny, nx) for the steps [t0, t0 + nt), the writer (may be NULL with
 * keep_resident) receives whole planes in pinned memory valid during the call; both are called in increasing t0, once per chunk; a
 * non-zero return ends the call with CTK_E_INVALID and leaves nothing in flight.
 * keep_resident != 0: the full-plane result stays in HBM in the resident slot of THE FIELD TO TRACK -- the slot ctk_anom_* with
 * keep_resident fills, whichever producer wrote it last.  ctk_track_resident, ctk_percentile_* with x = NULL and the `resident`
 * consumers run on it unchanged; ctk_resident_anom reports its shape, ctk_resident_anom_generation a new identity.  A failing call
 * leaves an earlier resident slab alone (argument errors) or dropped, never half written and reported. */
int ctk_reversal_f32(ctk_handle *h, const float *x, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2 /* or NULL */,
                     const double *dE, const double *tS, const double *tN, const double *tS2 /* or NULL */, int mask, float *out /* or NULL */,
                     int64_t chunk_steps, int keep_resident);
int ctk_reversal_f64(ctk_handle *h, const double *x, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2 /* or NULL */,
                     const double *dE, const double *tS, const double *tN, const double *tS2 /* or NULL */, int mask, double *out /* or NULL */,
                     int64_t chunk_steps, int keep_resident);
int ctk_reversal_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2 /* or NULL */,
                         const double *dE, const double *tS, const double *tN, const double *tS2 /* or NULL */, int mask, float *out_dev);
int ctk_reversal_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2 /* or NULL */,
                         const double *dE, const double *tS, const double *tN, const double *tS2 /* or NULL */, int mask, double *out_dev);
int ctk_reversal_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t steps, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user,
                           const int32_t *eq, const int32_t *po, const int32_t *eq2 /* or NULL */, const double *dE, const double *tS, const double *tN,
                           const double *tS2 /* or NULL */, int mask, ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps, int keep_resident);

/* ---- finite-amplitude local wave activity: the third family of blocking indices ----------------------------------------------------
 * Huang & Nakamura (2016); Chen, Lu, Burrows & Leung (2015) for Z500, with the anticyclonic / cyclonic split; Martineau et al. (2017);
 * Nakamura & Huang (2018).  The reference has no function for it; tests/lwa_util.py is the numpy statement of what follows.
 * x: (steps, ny, nx), float32 or float64, C-contiguous -- a height field that FALLS towards the pole (for a field that rises towards
 * the pole, such as PV, pass its negative).  The kernels never see latitudes; the caller passes a ROW TABLE (contrack.lwa_rows builds
 * it from lat[ny], lat_bounds, the hemisphere and a radius):
 *     ndom = 1 or 2 DOMAINS; domain d is the rows dom_rows[dom_off[d] .. dom_off[d + 1]) = (d_0 .. d_{n-1}), ordered FROM THE EQUATOR
 *             SIDE TO THE POLE (the rows with lat >= 0, resp. lat <= 0, sorted by |lat|; an equator row is in both domains)
 *     W[ny]   uint32, the area weight of a pixel of the row: rint(max(cos(lat), 0) * 2^30); a pole row has W = 0
 *     q[ny]   float64, finite and >= 0: max(cos(lat), 0) * dphi, dphi the trapezoid width of the row inside its domain in radians
 *     S[ny]   float64: radius / cos(lat) on active rows, finite and > 0 (0 elsewhere)
 *     active[ny]  0 / 1: rows with lat_bounds[0] <= |lat| <= lat_bounds[1] (0 < lat_bounds[0]) inside a requested domain
 * Per step, per domain and per active row j = d_p:
 *  1. the equivalent-latitude contour Z_j.  cap_j = nx * sum_{p' >= p} W[d_p'], exact in uint64.  The non-NaN pixels of the domain's
 *     rows are ordered by the integer key of their value (a total order; -0.0 before +0.0); A(k) = sum of W[row] over the pixels
 *     with key <= k, exact in uint64; Z_j = the value of the smallest key with A(k) >= cap_j.  No such key (NaNs ate the area):
 *     Z_j = NaN and the whole output row j of this step is NaN.
 *  2. the integrals, per column c, in float64, multiply and add rounded separately (no fused multiply-add), each sum started from
 *     +0.0 and added IN DOMAIN ORDER (rising p'):
 *         a = sum_{p' >= p, z[d_p'][c] > Z_j} ((double)z - (double)Z_j) * q[d_p']     anticyclonic: the ridge poleward of the contour, row j included
 *         y = sum_{p' <  p, z[d_p'][c] < Z_j} ((double)Z_j - (double)z) * q[d_p']     cyclonic: the trough equatorward of it
 *     A NaN pixel fails both compares and is skipped; +-inf are ordinary values: what IEEE arithmetic gives is the answer.
 *  3. out[j][c] = (dtype)((a + y) * S[j])  (part = 0, 'total');  (dtype)(a * S[j])  (part = 1, 'anticyclonic');  (dtype)(y * S[j])
 *     (part = 2, 'cyclonic'): one rounding to x's dtype.  Inactive rows are 0 and are not read unless an active row's domain holds them.
 * ref (may be NULL): (steps, ny) in x's dtype, the Z_j -- 0 on inactive rows, NaN on unreachable ones.
 * out has x's shape and dtype: ctk_track_* with a threshold and the op '>' tracks it as it is.
 * CTK_E_INVALID with a message, the handle usable: a null pointer, a size below 1, ndom not 1 or 2, dom_off not rising from 0 or a
 * domain longer than ny, a row index outside [0, ny) or twice in one domain, an active row in no domain or in two, a q (of a domain's
 * row) that is not finite or negative, an S that is not finite and > 0 on an active row, cap_j == 0 on an active row, nx * sum W
 * of a domain >= 2^63 (a defensive check: uint32 weights on a plane below 2^31 pixels cannot reach it), part outside 0 .. 2, a plane of 2^31 pixels or more, a domain too long for the kernels' LDS (more than 2 043
 * rows: ctk_lwa_plan, csrc/ctk_forms.h -- there is no other form), chunk_steps < 0, nothing to produce (out NULL and keep_resident 0).
 *
 * ctk_lwa_f32_dev / _f64_dev: x and out in device memory (ref on the host).
 * ctk_lwa_f32 / _f64: host arrays (out may be NULL with keep_resident).  Of every plane only the rows the domains span are uploaded
 * (one strided copy per chunk) and only the rows the active rows span are downloaded; the rest of out is zeroed on the host.  Two
 * input and two output chunks, as ctk_reversal_*.  chunk_steps = 0: about 256 MB of input per chunk.  Same bits for every chunk_steps.
 * ctk_lwa_stream_cb: reader and writer as ctk_reversal_stream_cb's (whole planes; writer may be NULL with keep_resident); ref holds
 * elem_bytes per value.
 * keep_resident != 0: the full-plane result stays in HBM in the resident slot of THE FIELD TO TRACK, as ctk_reversal_*'s does, with
 * a new ctk_resident_anom_generation.  A failing call leaves an earlier resident slab alone (argument errors) or dropped, never half
 * written and reported. */
int ctk_lwa_f32(ctk_handle *h, const float *x, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                const uint32_t *W, const double *q, const double *S, int part, float *out /* or NULL */, float *ref /* or NULL */, int64_t chunk_steps, int keep_resident);
int ctk_lwa_f64(ctk_handle *h, const double *x, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                const uint32_t *W, const double *q, const double *S, int part, double *out /* or NULL */, double *ref /* or NULL */, int64_t chunk_steps, int keep_resident);
int ctk_lwa_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                    const uint32_t *W, const double *q, const double *S, int part, float *out_dev, float *ref /* host, or NULL */);
int ctk_lwa_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                    const uint32_t *W, const double *q, const double *S, int part, double *out_dev, double *ref /* host, or NULL */);
int ctk_lwa_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t steps, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, int ndom,
                      const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part,
                      ctk_write_values_fn writer, void *writer_user, void *ref /* or NULL */, int64_t chunk_steps, int keep_resident);

/* ---- selection: the chosen tracks, or (step, track) rows, of a flag slab ----------------------------------------------------------
 * A study rarely wants every block: it picks tracks from the life-cycle frame (the Atlantic ones, those of ten days or more) or rows
 * of it (the mature days, the days the centre lies in a sector) and needs the int32 flag slab (T, ny, nx) restricted to them before
 * ctk_frequency_*, ctk_spells_*, ctk_composite_* or ctk_band_*.  tests/subset_util.py is the numpy statement of what follows.
 * A TABLE is off[n_off] (int64) and ids[n_ids] (int32):
 *     by id:   n_off = 2, off = {0, K}: the K ids, all > 0 and strictly increasing, apply to every step
 *     by row:  n_off = T + 1, off[0] = 0, non-decreasing, off[T] = n_ids: ids[off[t] .. off[t + 1]) are the ids wanted at step t, all
 *              > 0 and strictly increasing inside the slice
 * (T = 1: both readings say the same.)  Per step t and pixel p, with f = flag[t][p]:
 *     found = f > 0 and f is in the slice of step t
 *     sel   = found            (invert == 0)          sel = f > 0 and not found     (invert != 0)
 *     out[t][p] = sel ? (kind == CTK_SUBSET_ID ? f : 1) : 0
 *     hits[e] += 1 for the entry e of ids that found it, whatever invert is ;  n_selected += sel
 * So values <= 0 are background: never selected, never counted, 0 in the output, with invert too; an id listed at another step only
 * is not found at this one; an empty table selects nothing, or with invert every f > 0.  All of it is integers: there is no tolerance.
 * out may be NULL when hits or n_selected is given: a count-only call, nothing is written or downloaded.  hits (host, n_ids values,
 * overwritten) and n_selected may each be NULL.
 * CTK_E_INVALID with a message, the handle usable and nothing written: a null required pointer, T, ny or nx < 1, a plane of 2^31
 * pixels or more, n_off neither 2 nor T + 1, off not as stated, an id <= 0, a slice that is not strictly increasing, kind not
 * CTK_SUBSET_ID or CTK_SUBSET_MASK, chunk_steps < 0, nothing to produce (out, hits and n_selected all NULL).
 *
 * ctk_subset_dev: flag and out in HBM; a lane writes only the elements it read, so out_dev == flag_dev selects in place.  The result
 * feeds the _dev entries of the consumers without crossing PCIe.
 * ctk_subset / _cb: a host array or a reader callback (int32 elements) and a host array or a writer callback (NULL: count only); two
 * input and two output chunks, chunk k + 1 travels in while the kernel works on chunk k and chunk k - 1 leaves (chunk_steps = 0: about
 * 256 MB per chunk).  The table is uploaded once, hits accumulate in HBM over the chunks and are copied out at the end.  The same bytes
 * for every chunk_steps.  Reader and writer are called in increasing t0, once per chunk; a non-zero return ends the call with
 * CTK_E_INVALID and leaves nothing in flight.  out == flag is allowed in ctk_subset.
 * No subset call touches the resident slot of the field to track: ctk_resident_anom_generation stays what it was. */
#define CTK_SUBSET_ID 0
#define CTK_SUBSET_MASK 1
int ctk_subset_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids,
                   int invert, int kind, int32_t *out_dev /* or NULL; == flag_dev: in place */, uint64_t *hits /* host [n_ids] or NULL */,
                   int64_t *n_selected /* or NULL */);
int ctk_subset(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids, int invert,
               int kind, int32_t *out /* host or NULL */, uint64_t *hits /* host [n_ids] or NULL */, int64_t *n_selected /* or NULL */, int64_t chunk_steps);
int ctk_subset_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int64_t *off, int64_t n_off, const int32_t *ids,
                  int64_t n_ids, int invert, int kind, ctk_write_chunk_fn writer /* or NULL */, void *writer_user, uint64_t *hits /* host [n_ids] or NULL */,
                  int64_t *n_selected /* or NULL */, int64_t chunk_steps);

/* ---- per-block peak and extent: what a study selects (step, track) rows on ----------------------------------------------------------
 * The "block intensity" of the literature is the maximum anomaly inside the block (the minimum for gorl = '<'), not the area mean
 * ctk_lifecycle_* gives; the position of that peak is the block centre of the hybrid indices, which test for a height reversal
 * equatorward of the anomaly maximum (Barriopedro et al. 2010; Dunn-Sigouin & Son 2013); and a zonal extent of at least 15 degrees of
 * longitude, with the meridional span, is part of nearly every blocking definition.  The reference has no function for it;
 * tests/blockstat_util.py is the numpy statement of what follows.
 * flag: (T, ny, nx) int32; x: a float32 / float64 field of the same shape; the key is a ROW table exactly as ctk_subset_* states it:
 * off[T + 1] (int64) and ids[n_ids] (int32), all > 0 and strictly increasing inside a step's slice.  There is no by-id reading here:
 * n_off must be T + 1.  For entry e = (t, id) of the table let P be the pixels of step t with flag == id, in row-major order; rows[e]:
 *     n             |P|.  n == 0: the entry matched nothing and every other value holds its "empty" value, given in brackets
 *     r0, r1        the lowest and the highest grid row of P                                                          [-1, -1]
 *     west, width   occ[c] says whether some pixel of P lies in column c.  All columns occupied: west = 0, width = nx.  Otherwise
 *                   take the maximal CIRCULAR runs of unoccupied columns -- a run may pass the seam; its start s is the column whose
 *                   western neighbour, modulo nx, is occupied --, the longest of them and among equally long ones the lowest s:
 *                   west = (s + len) % nx, width = nx - len                                                            [-1, 0]
 *                   (a rule of its own: NOT the `shift` of ctk_lifecycle_*, which copies the reference's non-circular
 *                   np.argmax(np.diff(cols)); lon.max() - lon.min() over a block on the seam gives 359 degrees)
 *     nv            the pixels of P whose value is not NaN                                                                  [0]
 *     max, max_p    the largest of those values in the total order -inf < ... < -0.0 < +0.0 < ... < +inf, as float64 (a float32
 *                   value widens exactly), and the lowest pixel index row * nx + col that holds exactly it   [nv == 0: NaN, -1]
 *     min, min_p    the same at the other end, again the lowest index                                        [nv == 0: NaN, -1]
 * want: CTK_BLOCK_SHAPE (r0 .. width), CTK_BLOCK_PEAKS (nv .. min) or both; what is not wanted holds its empty value, n is always
 * counted, and CTK_BLOCK_SHAPE alone needs no field.  All of it is integers and selected values: there is no tolerance, and the same
 * bytes result whatever the kernel form and the chunking (k_blockstat, ctk_blockstat.hip).
 * rows: host, n_ids entries, overwritten.  n_ids == 0: the call succeeds and writes nothing.
 * CTK_E_INVALID with a message, the handle usable and nothing written: everything ctk_subset_* refuses for a row table, n_off != T + 1,
 * want 0 or with unknown bits, CTK_BLOCK_PEAKS with no field and no resident anomaly slab of the call's shape and type, chunk_steps < 0.
 *
 * ctk_blockstat_*_dev: both slabs in HBM; x_dev == NULL with CTK_BLOCK_PEAKS: the anomaly slab ctk_anom_* left resident on this handle.
 * ctk_blockstat_f32 / _f64: host arrays through chunk-sized device buffers as ctk_composite_f32 / _f64 (chunk_steps = 0: about 256 MB
 * per chunk); x == NULL, or peaks not wanted: only the flags travel.  The records accumulate in HBM over the chunks and are copied
 * out once.
 * ctk_blockstat_cb: two readers with ctk_composite_cb's contract (the flag reader is called before the field reader for every chunk;
 * field_reader == NULL: the resident anomaly slab of elem_bytes, or no field).
 * No blockstat call touches the resident slot: ctk_resident_anom_generation stays what it was. */
#define CTK_BLOCK_SHAPE 1
#define CTK_BLOCK_PEAKS 2
typedef struct ctk_block_row {
    uint32_t n, nv;
    int32_t r0, r1, west, width;
    int64_t max_p, min_p;
    double max, min;
} ctk_block_row;
int ctk_blockstat_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *x_dev /* or NULL */, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                          const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows /* host [n_ids] */);
int ctk_blockstat_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *x_dev /* or NULL */, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                          const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows);
int ctk_blockstat_f32(ctk_handle *h, const int32_t *flag, const float *x /* or NULL */, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids,
                      int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps);
int ctk_blockstat_f64(ctk_handle *h, const int32_t *flag, const double *x /* or NULL */, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids,
                      int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps);
int ctk_blockstat_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                     ctk_read_chunk_fn field_reader /* or NULL */, void *field_user, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids, int want,
                     ctk_block_row *rows, int64_t chunk_steps);

/* ---- the blocking-frequency climatology of the reference's tutorial (README.rst:159-160) ---------------------------------------
 *   xr.where(block['flag'] > 1, 1, 0).sum(dim='time') / block.ntime * 100     -- on the int32 flag slab (T, ny, nx), per group:
 *   counts[g][y][x] = #{t : group[t] == g and flag[t][y][x] > above}            (exact; the caller divides: counts / n[g] * 100)
 * group: T host ints in [0, ngroups) (month, season ... of every timestep; any order in time), NULL = one group (ngroups = 1).
 * above = 1 is the README's expression, 0 counts every tracked id.  One read of the slab (k_freq, ctk_freq.hip), a few atomics.
 * ctk_frequency_dev: flag in HBM; accumulate = 1 adds to counts_dev (time shards, a caller's own chunks), 0 overwrites it.
 * ctk_frequency / _cb: a host array or a reader callback (ctk_read_chunk_fn, int32 elements); the flag passes through two
 * chunk-sized device buffers, chunk k+1 copied while chunk k is counted (as ctk_track_stream_*; chunk_steps = 0: about 256 MB per
 * chunk), so a slab larger than HBM or read lazily from a file works.  T must stay below 2^32 (uint32 counts). */
int ctk_frequency_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                      uint32_t *counts_dev /* [ngroups][ny][nx] */, int accumulate /* 0: overwrite, 1: add */);
int ctk_frequency(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                  uint32_t *counts /* host [ngroups][ny][nx] */, int64_t chunk_steps);
int ctk_frequency_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *group, int ngroups,
                     int32_t above, uint32_t *counts /* host */, int64_t chunk_steps);

/* ---- blocked spells per grid point: events, their durations, the longest one (the maps beside the frequency map) ----------------
 * On the int32 flag slab (T, ny, nx): at pixel p, step t CONTINUES step t-1 iff t is not a segment start, flag[t-1][p] > above and
 * flag[t][p] > above and, with by_id = 1, flag[t-1][p] == flag[t][p].  A spell is a maximal chain of continuing steps that starts at a
 * step with flag > above; its duration d is its number of steps and its group is group[onset], the group of its first step, even
 * if it runs on into another group.  A spell cut by the end of the slab or of a segment counts with the length it has.  Over the
 * spells with d >= min_duration (>= 1):
 *   events[g][y][x] = their number,  steps[g][y][x] = the sum of their durations,  longest[g][y][x] = the longest (0: none)
 * all exact uint32; the caller divides: mean duration = steps / events in float64.  group: T host ints in [0, ngroups), any order
 * in time, NULL = one group (ngroups = 1).  seg_starts: nseg first steps of independent time segments with the meaning of
 * ctk_set_segments (0 first, strictly increasing, below T), given with the call; NULL / 0: one segment.  One read of the slab
 * (k_spell, ctk_spell.hip) whatever the slice and chunk lengths: the result does not depend on them.
 * ctk_spells_dev: flag in HBM.  ctk_spells / _cb: a host array or a reader callback (ctk_read_chunk_fn, int32 elements) through two
 * chunk-sized device buffers as ctk_frequency / _cb (chunk_steps = 0: about 256 MB per chunk); a run that is open at the end of a
 * chunk is carried to the next one in HBM.  T must stay below 2^32 (uint32 durations). */
int ctk_spells_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts,
                   int64_t nseg, int32_t above, int by_id /* 0 / 1 */, int64_t min_duration, uint32_t *events_dev /* [ngroups][ny][nx] */,
                   uint32_t *steps_dev, uint32_t *longest_dev);
int ctk_spells(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts, int64_t nseg,
               int32_t above, int by_id, int64_t min_duration, uint32_t *events /* host [ngroups][ny][nx] */, uint32_t *steps, uint32_t *longest,
               int64_t chunk_steps);
int ctk_spells_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *group, int ngroups,
                  const int64_t *seg_starts, int64_t nseg, int32_t above, int by_id, int64_t min_duration, uint32_t *events /* host */, uint32_t *steps,
                  uint32_t *longest, int64_t chunk_steps);

/* ---- composites: the step after the frequency map of the reference's tutorial (README.rst:156-164) ------------------------------
 * The tutorial ends with the blocking frequency; the composite is what a study computes next: the mean of a field (the tracked
 * anomaly itself, temperature, precipitation) over the time steps at which a grid point is blocked, in all or per group:
 *   ds[var].where(ds[flag] > above).groupby(...).mean('time')
 * On the int32 flag slab and a float32 / float64 field slab over the same T time steps, per grid point p, for t = 0 .. T-1 RISING:
 *   if flag[t][p] > above (and, with skipna, x[t][p] is not NaN):  sum[group[t]][p] += (double)x[t][p];  n[group[t]][p] += 1
 * sum starts at +0.0 (float64), n at 0 (uint32); an unselected step adds nothing (not + 0.0); without skipna a selected NaN makes the
 * sum NaN; +inf and -inf make NaN.  The additions of a pixel happen in time order and T is never split over threads, so the sums are
 * reproducible bit for bit whatever the kernel form or the chunking (k_composite, ctk_composite.hip).  The caller divides:
 * mean = sum / n in float64, NaN where n == 0.  group: T host ints in [0, ngroups), any order in time; NULL = one group.
 * ctk_composite_*_dev: both slabs in HBM; x_dev == NULL: the anomaly slab ctk_anom_* left resident on this handle (its shape and type
 * must be the call's: CTK_E_STATE otherwise).  accumulate = 1 continues from the given accumulators (a caller's own chunks, later
 * time shards: the time order is then the order of the calls), 0 starts from zero.
 * ctk_composite_f32 / _f64: host arrays; both slabs pass through chunk-sized device buffers, two chunks of flags and two of the field,
 * chunk k+1 uploaded while chunk k is reduced (chunk_steps = 0: about 256 MB of field per chunk); the accumulators stay in HBM until
 * the last chunk.  x == NULL: the resident anomaly slab, only the flags cross PCIe.
 * ctk_composite_cb: two readers (ctk_read_chunk_fn: int32 flags, field elements of elem_bytes), contract and threading rules of
 * ctk_lifecycle_stream_cb's; the flag reader is called before the field reader for every chunk; field_reader == NULL: the resident
 * anomaly slab of elem_bytes.  T must stay below 2^32 (uint32 counts). */
int ctk_composite_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *x_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                          int32_t above, int skipna, double *sum_dev /* [ngroups][ny][nx] */, uint32_t *n_dev /* [ngroups][ny][nx] */,
                          int accumulate /* 0: start from zero, 1: continue */);
int ctk_composite_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *x_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                          int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate);
int ctk_composite_f32(ctk_handle *h, const int32_t *flag, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                      int skipna, double *sum /* host [ngroups][ny][nx] */, uint32_t *n /* host */, int64_t chunk_steps);
int ctk_composite_f64(ctk_handle *h, const int32_t *flag, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                      int skipna, double *sum, uint32_t *n, int64_t chunk_steps);
int ctk_composite_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                     ctk_read_chunk_fn field_reader, void *field_user, const int32_t *group, int ngroups, int32_t above, int skipna, double *sum,
                     uint32_t *n, int64_t chunk_steps);

/* ---- block-centred composites: the step after the tracks of the reference's tutorial (README.rst:198-228) ------------------------
 * The tutorial ends with the tracks and the genesis points of the life-cycle frame; a blocking study then composites in the block's
 * own frame of reference: a field in a window that moves with the block's centre, averaged over the blocks per day since onset, per
 * day before decay or per fifth of the life cycle.  On a field x (T, ny, nx), float32 or float64, and R stamps in struct-of-arrays
 * form -- t[r] (int64), row[r], col[r], bin[r] (int32) -- with nbins bins, half widths hy >= 0 and hx >= 0 in grid points, wrap (0 / 1)
 * and skipna (0 / 1), the outputs sum[nbins][2 hy + 1][2 hx + 1] (float64, from +0.0) and n[...] (uint32) of the same shape are
 *   for r = 0 .. R-1, RISING (the order of the arrays as given):
 *       if bin[r] < 0: continue                                     -- a stamp the caller dropped
 *       for j in -hy..hy, i in -hx..hx:
 *           y = row[r] + j;   if y < 0 or y >= ny: continue         -- no step over a pole: not counted
 *           c = col[r] + i;   wrap: c = c mod nx;   else if c < 0 or c >= nx: continue
 *           v = (double)x[t[r]][y][c]                               -- a plain conversion, denormals kept
 *           if skipna and v is NaN: continue
 *           sum[bin[r]][j + hy][i + hx] = sum[...] + v;   n[...] += 1
 * Without skipna a NaN makes its cell NaN.  The caller divides: mean = sum / n in float64, NaN where n == 0.  A cell meets the stamps
 * of its bin in the order given and they are never split over threads, so the sums are reproducible bit for bit whatever the kernel
 * form or the chunking (k_centred, ctk_centred.hip).
 * Arguments: t must be non-decreasing (which keeps the order of the additions independent of the chunking), 0 <= t < T,
 * 0 <= row < ny, 0 <= col < nx, bin < nbins, nbins >= 1, R < 2^32, nbins * (2 hy + 1) * (2 hx + 1) < 2^31: CTK_E_INVALID; with wrap
 * 2 hx + 1 <= nx (a wider window would count a column twice): CTK_E_RANGE.  R == 0 is valid and gives zeros.
 * ctk_centred_*_dev: the slab in HBM, the stamps host arrays; x_dev == NULL: the anomaly slab ctk_anom_* left resident on this handle
 * (its shape and type must be the call's: CTK_E_STATE otherwise).  accumulate = 1 continues from the given accumulators (a caller's
 * own pieces: the order of the additions is then the order of the calls), 0 starts from zero.
 * ctk_centred_f32 / _f64: the field a host array; it passes through two chunk-sized device buffers, chunk k+1 uploaded while chunk k
 * is reduced (chunk_steps = 0: about 256 MB of field per chunk).  A chunk none of whose time steps carries a stamp with bin >= 0 is
 * neither read nor uploaded, and of the others only the latitude rows [min(row) - hy, max(row) + hy] of that chunk's stamps, clipped
 * to the grid, travel, as one strided copy per chunk.  x == NULL: the resident anomaly slab, no field bytes cross PCIe.
 * ctk_centred_cb: a reader (ctk_read_chunk_fn: field elements of elem_bytes, whole planes), contract and threading rules of
 * ctk_composite_cb's; it is not called for a chunk without stamps; field_reader == NULL: the resident anomaly slab of elem_bytes. */
int ctk_centred_f32_dev(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, int64_t R, const int64_t *t /* host [R] */, const int32_t *row,
                        const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna,
                        double *sum_dev /* [nbins][2 hy + 1][2 hx + 1] */, uint32_t *n_dev, int accumulate /* 0: start from zero, 1: continue */);
int ctk_centred_f64_dev(ctk_handle *h, const double *x_dev, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                        const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate);
int ctk_centred_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                    const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum /* host */, uint32_t *n /* host */, int64_t chunk_steps);
int ctk_centred_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                    const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum, uint32_t *n, int64_t chunk_steps);
int ctk_centred_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn field_reader, void *field_user,
                   int64_t R, const int64_t *t, const int32_t *row, const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna,
                   double *sum, uint32_t *n, int64_t chunk_steps);

/* ---- reductions over space per time step: the time-longitude (Hovmoeller) diagram of a latitude band, the blocked area of a sector --
 * Every other consumer of the flag reduces over time or per contour; these reduce over SPACE and keep the time axis: how much of a
 * latitude band is blocked per step and longitude, and the blocked area (and the mean intensity over it) of a longitude sector per
 * step -- the daily index a study correlates with other series.  On the int32 flag slab (T, ny, nx), the rows [y0, y1), float64 row
 * weights w[ny] (finite, any sign) and optionally a float32 / float64 field x of the same shape, per step t and column c:
 *   cnt[t][c]  = #{y in [y0, y1) : flag[t][y][c] > above}                                                            (uint32)
 *   area[t][c] = from +0.0, for y = y0 .. y1 - 1 RISING:  if flag[t][y][c] > above:  s = s + w[y]                     (float64)
 *   wx[t][c]   = the same walk with  s = s + (w[y] * (double)x[t][y][c])   -- the product rounded to float64, then added
 * With the weights 111 dlat * 111 dlon * cos(lat) the reference's life cycle uses (contrack.py:846-848) `area` is in km^2 and adds up
 * to what the reference calls a contour's Size (contrack.py:874); wx / area is the area-weighted mean of the field.  A value of x at
 * an unflagged pixel is never read; a NaN or inf at a flagged pixel propagates as in np.sum (the sign bit of a NaN born from
 * inf - inf is the hardware's).  Sectors: nsect >= 0 pairs (x0, len), 0 <= x0 < nx, 1 <= len <= nx, the columns x0, x0 + 1, ...
 * modulo nx (len == nx: the full circle; sectors may overlap):
 *   sec_cnt[t][s] = the sum of the column counts;  sec_area[t][s], sec_wx[t][s] = from +0.0, the column values added in that order
 * No sum is split over threads or added atomically, so all outputs are the same bits whatever the kernel form, the chunking, the
 * pointer alignment or the source (k_band, k_band_sect: ctk_band.hip).  ny * nx must stay below 2^32 (uint32 counts): CTK_E_RANGE.
 * ctk_band_spec.columns != 0 asks for the column tables, nsect > 0 for the sector tables; neither: CTK_E_INVALID.  With sectors only
 * the column tables stay in a chunk-sized buffer of the handle and never cross PCIe.  wx / sec_wx are written only with a field.
 * resident != 0: the field is the anomaly slab ctk_anom_* left resident on this handle -- its shape and type must be the call's and
 * its generation (ctk_resident_anom_generation) must be resident_gen, which tells the slab the caller means from a later one:
 * CTK_E_STATE otherwise; only the flags travel then.
 * ctk_band_dev: the slabs in HBM (x_dev NULL without resident: no field; elem_bytes 4 / 8 is the field's), the outputs device pointers.
 * ctk_band_f32 / _f64: host arrays (x NULL: no field, or the resident slab of that type); the slabs pass through chunk-sized device
 * buffers, chunk k+1 uploaded while chunk k is reduced (chunk_steps = 0: about 256 MB per chunk), the tables of chunk k go to row c0
 * of the outputs.  ctk_band_cb: readers (ctk_read_chunk_fn: int32 flags, field elements of elem_bytes), contract and threading rules
 * of ctk_composite_cb's; the flag reader is called before the field reader for every chunk; field_reader NULL: no field, or the
 * resident slab of elem_bytes. */
typedef struct ctk_band_spec {
    int32_t y0, y1;                 /* the band: rows [y0, y1), 0 <= y0 < y1 <= ny */
    int32_t above;
    int32_t nsect;                  /* sectors, >= 0 */
    const double *w;                /* host [ny] */
    const int32_t *sectors;         /* host [nsect][2]: x0, len */
    int32_t columns;                /* != 0: the column tables are wanted */
    int32_t resident;               /* != 0: the field is the resident anomaly slab ... */
    uint64_t resident_gen;          /* ... of this generation */
} ctk_band_spec;
typedef struct ctk_band_out {
    uint32_t *cnt; double *area, *wx;                   /* [T][nx], with columns */
    uint32_t *sec_cnt; double *sec_area, *sec_wx;       /* [T][nsect], with nsect > 0 */
} ctk_band_out;
int ctk_band_dev(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx,
                 const ctk_band_spec *spec, const ctk_band_out *out_dev);
int ctk_band_f32(ctk_handle *h, const int32_t *flag, const float *x, int64_t T, int ny, int nx, const ctk_band_spec *spec, const ctk_band_out *out,
                 int64_t chunk_steps);
int ctk_band_f64(ctk_handle *h, const int32_t *flag, const double *x, int64_t T, int ny, int nx, const ctk_band_spec *spec, const ctk_band_out *out,
                 int64_t chunk_steps);
int ctk_band_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                ctk_read_chunk_fn field_reader, void *field_user, const ctk_band_spec *spec, const ctk_band_out *out, int64_t chunk_steps);

/* ---- a weighted filter or a block mean along time ---------------------------------------------------------------------------------
 * The low-, high- and band-pass filters of the blocking literature (Lanczos weights, Duchon 1979) and means over blocks of steps
 * (6-hourly to daily, daily to pentads).  The reference has no function for it; tests/filter_util.py is the numpy statement of what
 * follows.  x: (T, ny, nx), float32 or float64, C-contiguous.  w: K float64 weights (weighted mode), or NULL (box mode: the mean of
 * the K taps).  1 <= K <= 2^20, stride >= 1, offset of either sign.  Segment starts as everywhere: 0 first, strictly increasing,
 * the last below T; nseg = 0: one segment.  Segment s is the steps [S, E).
 * Layout: output q = 0, 1, ... of segment s has its taps i = 0 .. K - 1 at the steps first + i, first = S + offset + q * stride, and
 * its label step at first + K / 2 (integer division).  The output exists iff S <= label < E.  Outputs are numbered through the
 * segments in order; a segment may have none.  T_out <= T.  With stride = 1 and offset = -(K / 2) there is one output per step,
 * its window K / 2 steps back and (K - 1) / 2 forward -- the window of ctk_anom_*'s `smooth` --, and T_out == T.
 * The used taps of an output are [k0, k1), the i with S <= first + i < E; its window is complete iff k0 == 0 and k1 == K.
 * Value, per output and pixel, everything in float64, the used taps in rising i, no fused multiply-add:
 *     weighted:  s = 0, ws = 0, n = 0;  per tap  v = (double)x[first + i];  skipna and v is NaN: the tap is skipped;
 *                otherwise  s = s + (w[i] * v)  -- the product rounded, then added --,  ws = ws + w[i],  n = n + 1
 *     box:       the same with  s = s + v
 *     result:    NaN where edges == CTK_FILTER_EDGES_NAN and the window is incomplete, and where n == 0;
 *                box: (dtype)(s / (double)n);  weighted with no tap missing (complete, none skipped): (dtype)s;
 *                weighted with taps missing (incomplete under CTK_FILTER_EDGES_RENORM, or skipped): (dtype)(s / ws)
 * so CTK_FILTER_EDGES_RENORM changes the ends of a segment only.  Without skipna NaN and +-inf propagate by IEEE arithmetic.
 * The bits are those of that loop whatever the kernel form, thread count, tile, alignment, chunking or source.
 * CTK_E_INVALID with a message (also with a NULL handle), the handle usable: T, K, stride, ny or nx below 1, a weight that is NaN or
 * inf, edges == CTK_FILTER_EDGES_RENORM or skipna with a negative weight or a sum of weights that is not positive (a band-pass
 * cannot be renormalised), bad segment starts, T_out that is not the layout's, chunk_steps < 0, nothing to produce.
 *
 * ctk_filter_layout (host only, no handle): T_out, and where not NULL first_out[T_out] (T entries are always enough) and
 * out_starts[max(nseg, 1)], the first output of every segment.
 * ctk_filter_f32_dev / _f64_dev: x and out (T_out, ny, nx) in device memory, not overlapping.
 * ctk_filter_f32 / _f64: host arrays (out may be NULL with keep_resident).  The slab passes through two chunk buffers of
 * chunk_steps + K - 1 steps (0: about 256 MB per chunk; below K - 1 it is raised to K - 1); the last K - 1 steps of a chunk stay on
 * the device for the next, so no step is uploaded twice.  An output leaves with the chunk that holds step first + K - 1.
 * ctk_filter_stream_cb: reader and writer (may be NULL with keep_resident) as ctk_level_mean_stream_cb's, one plane per step; the
 * writer receives outputs [t0, t0 + nt) in rising order, not with every chunk.  Neither is asked for a step twice.
 * keep_resident != 0: the result also stays in HBM as the resident level mean (ctk_resident_level_mean reports T_out steps, its
 * generation advances), where ctk_anom_seg_resident and ctk_filter_resident take it as they take a vertical mean.
 * ctk_filter_resident: x is the resident level mean (CTK_E_INVALID if there is none): shape and dtype are its; out (NULL: none) holds
 * T_out planes of that dtype; keep_resident != 0: the result replaces the mean in the slot.  It is never filtered in place. */
#define CTK_FILTER_EDGES_NAN 0
#define CTK_FILTER_EDGES_RENORM 1
int ctk_filter_layout(int64_t T, int K, int64_t stride, int64_t offset, const int64_t *starts, int64_t nseg, int64_t *first_out, int64_t *out_starts,
                      int64_t *T_out);
int ctk_filter_f32_dev(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges,
                       int skipna, const int64_t *starts, int64_t nseg, float *out_dev, int64_t T_out);
int ctk_filter_f64_dev(ctk_handle *h, const double *x_dev, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges,
                       int skipna, const int64_t *starts, int64_t nseg, double *out_dev, int64_t T_out);
int ctk_filter_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna,
                   const int64_t *starts, int64_t nseg, float *out, int64_t T_out, int64_t chunk_steps, int keep_resident);
int ctk_filter_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna,
                   const int64_t *starts, int64_t nseg, double *out, int64_t T_out, int64_t chunk_steps, int keep_resident);
int ctk_filter_stream_cb(ctk_handle *h, int elem_bytes /* 4: float32, 8: float64 */, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user,
                         const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna, const int64_t *starts, int64_t nseg,
                         ctk_write_values_fn writer, void *writer_user, int64_t T_out, int64_t chunk_steps, int keep_resident);
int ctk_filter_resident(ctk_handle *h, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna, const int64_t *starts, int64_t nseg,
                        void *out, int64_t T_out, int keep_resident);

#ifdef __cplusplus
}
#endif
#endif /* CONTRACK_HIP_H */
