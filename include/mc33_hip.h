/* mc33_hip.h -- device-level C ABI of the MI355X MC33 extractor (plain pointers and sizes only).
 *
 * These are the entry points the reference-compatible host layer (mc33_capi.c: create_MC33,
 * calculate_isosurface, size_of_isosurface, free_MC33 - reference include/marching_cubes_33.h:228-258)
 * is built on, and what a foreign-language binding would bind.  Each one names the reference code it
 * replaces ("MC:" = reference source/marching_cubes_33.c).
 *
 * All functions return 0 on success, a negative MC33HIP_E* code otherwise (no exceptions, no exit;
 * the reference's only failure convention is a NULL return, MC:1884-1887).
 */
#ifndef MC33_HIP_H
#define MC33_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC33HIP_OK          0
#define MC33HIP_EINVAL     -1  /* bad argument                                   */
#define MC33HIP_ENOGPU     -2  /* no HIP device / runtime error at start-up       */
#define MC33HIP_ENOMEM     -3  /* host or device allocation failed                */
#define MC33HIP_ECAPACITY  -4  /* caller's output buffers are too small           */
#define MC33HIP_ERUNTIME   -5  /* a HIP call or kernel failed (see last_error)    */
#define MC33HIP_EOVERFLOW  -6  /* more than 2^32-1 vertices or triangles          */

typedef struct mc33hip_ctx mc33hip_ctx;

/* Geometry of the (slab of the) grid one context works on.  Replaces the part of create_MC33 that
 * snapshots _GRD (MC:1758-1782).  sample_bytes must match the library variant: libMC33_f32 4 (float),
 * libMC33_u8 1, libMC33_u16 2, libMC33_u32 4 (unsigned int), libMC33_f64 8 (double). */
typedef struct {
	unsigned int npx, npy;      /* points per row / rows per plane                                       */
	unsigned int npz_resident;  /* planes resident in this context                                        */
	unsigned int plane0;        /* global z index of the first resident plane (0 for a whole grid)        */
	unsigned int nz_total;      /* cell slices of the WHOLE grid (points along z - 1)                     */
	double r0[3], d[3];         /* origin and spacing of the WHOLE grid (_GRD.r0, _GRD.d)                 */
	int sample_bytes;
	int device;                 /* HIP device ordinal, -1: current device                                 */
} mc33hip_grid_desc;

/* Work range of one extraction: cell slices [z_begin, z_end) are emitted; when ghost_below is non-zero
 * slice z_begin-1 is classified too, so that ids of vertices on the slab interface - which belong to
 * the rank below - can be resolved.  Single GPU: {0, nz_total, 0, 0}. */
typedef struct {
	unsigned int z_begin, z_end;
	unsigned int ghost_below;
	unsigned int id_base;       /* number of vertices created by all slices below z_begin (global numbering) */
} mc33hip_range;

typedef struct {
	unsigned long long nV, nT;            /* vertices / triangles of slices [z_begin, z_end)                */
	unsigned long long nV_ghost, nT_ghost;/* ... of the ghost slice (0 without ghost)                       */
	unsigned long long active_cells;      /* cells cut by the surface in the classified slices             */
} mc33hip_counts;

typedef struct {
	float sweep_ms, scan_ms, emit_ms;     /* hipEvent time of each pass of the last extraction, on its stream */
	float total_ms;
	unsigned int sweep_launches;          /* >1 if the work-record buffer had to grow and the sweep re-ran     */
} mc33hip_timing;

int mc33hip_create(mc33hip_ctx **out, const mc33hip_grid_desc *desc);
void mc33hip_destroy(mc33hip_ctx *c);
const char *mc33hip_last_error(void);

/* Grid upload: replaces "M->F = G->F" (MC:1792) - the reference re-reads host memory on every call,
 * this library keeps a pitched copy in HBM.
 *   upload_rows : F[k][j] row pointers exactly as _GRD.F holds them (rows may be separate mallocs,
 *                 reference MC33_util_grd.c:147-169), k counts resident planes
 *   adopt_device: use a caller-owned device buffer in place (no copy); pitch/slice in samples
 *
 * Layout of an adopted buffer: sample (x, y, k) of resident plane k at device_samples[k * slice + y * pitch + x], any
 * pitch >= npx, any slice >= pitch * npy, any base address a sample may have.  The result never depends on the layout or on
 * what the padding holds; the speed does:
 *   - base, pitch and slice all multiples of 4 BYTES: 1- and 2-byte samples are classified a dword at a time (otherwise a
 *     sample per lane and load);
 *   - base, pitch and slice all multiples of 16 BYTES: the vertex pass stages rows in 16-byte chunks (otherwise every work
 *     record loads its own samples).
 *   (The library's own copy has both.)  Those dwords and chunks start at multiples of 4 / 16 bytes from the row's first sample and
 *   may end behind its last one, inside the pitch.  READABLE EXTENT: every row, the last row of the last resident plane
 *   included, must be readable from its first sample to the next 16-byte address boundary behind its last grid point or to
 *   the end of its pitch, whichever comes first - at most 15 bytes more than the npx samples (the next 4-byte boundary where only the first
 *   condition holds, nothing behind the last grid point where neither does).  Nothing else is read.
 *   - EINVAL: pitch < npx, slice < pitch * npy, pitch > 0xFFFFFFFF samples, or 64 rows of pitch samples take more than
 *     0xFFFFFFFF bytes (the sweep addresses a tile's rows with 32-bit offsets).                                             */
int mc33hip_upload_rows(mc33hip_ctx *c, const void *const *const *F);
int mc33hip_upload_contiguous(mc33hip_ctx *c, const void *host_samples);
int mc33hip_adopt_device(mc33hip_ctx *c, const void *device_samples, size_t pitch, size_t slice);

/* Who must say what when samples change.  The sweep can leave out the parts of the volume whose samples all lie on one side of
 * the isovalue, from a table of sample ranges (minimum and maximum per plane of a 256 x 63 cell strip, 0.01 % of the grid) that
 * it makes by the second sweep over the same samples - one extra pass over the grid, once - and keeps for as long as it KNOWS
 * the samples to be what they were:
 *   - the library's own copy (mc33hip_upload*): always; every upload drops the table.  Nothing to say.
 *   - an adopted buffer (mc33hip_adopt_device): never, unless the caller says so.  Its samples may change without this library
 *     knowing, and as adopted the buffer is volatile: every sweep reads all of it, exactly as before these calls existed.
 *       mc33hip_grid_stable(c, 1)  the caller promises to call mc33hip_grid_changed after every write to the samples, by
 *                                  whatever road (its own kernels, copies, another library), before the next call that
 *                                  classifies (count, count_async, extract, sweep_many, prepare_many).  From then on a table
 *                                  may be kept.  mc33hip_grid_stable(c, 0) takes the promise back and drops the table.
 *       mc33hip_grid_changed(c)    the samples have changed: the table is dropped (and made again by the second sweep from
 *                                  now), sweeps made ahead and a count waiting for its emit are forgotten.  Legal, and
 *                                  harmless, on any context.
 *     mc33hip_adopt_device itself drops the table and leaves the new buffer volatile.
 *   mc33hip_set_stream / mc33hip_own_stream drop the table too (it is made on the context's stream, and a new stream is not
 *   ordered behind the old one); the promise stands, the table is made again by the second sweep on the new stream.
 * A stale table is the one way to a wrong surface here: a caller that cannot keep the promise does not make it.
 * MC33_HIP_RANGES=0 in the environment when a context is created: that context never makes a table.
 * The surface never depends on whether a table exists: it is bit for bit the one every tile streamed gives. */
int mc33hip_grid_stable(mc33hip_ctx *c, int stable);
int mc33hip_grid_changed(mc33hip_ctx *c);
/* For tests, not part of any extraction.  mc33hip_range_table: the table as it is, [resident plane][y tile][row segment]{min, max}
 * of MC33_real (y tiles of 63 cell rows, row segments of 256 cells; both ends of a strip inclusive; {-inf, +inf} for a strip
 * that holds a NaN) into host memory; bytes must be the table's size; MC33HIP_EINVAL when there is no table.
 * mc33hip_sweep_skipped: {tiles of the sweep, tiles left out below the isovalue, above it} of the last single-isovalue sweep
 * made at timing level >= 1 (mc33hip_set_timing); MC33HIP_EINVAL when there was none.  Nothing is counted at level 0. */
int mc33hip_range_table(mc33hip_ctx *c, void *host_out, size_t bytes);
int mc33hip_sweep_skipped(mc33hip_ctx *c, unsigned long long out[3]);
/* The block table kept beside the range table, and what a sweep makes of it.  mc33hip_range_blocks: 20 entries
 * {min, max} per strip, [resident plane][y tile][row segment][entry] - entry 4 g + k: sample rows 16 g .. 16 g + 15 of the strip,
 * samples 64 k .. 64 k + 63 of the segment; entry 16 + g: the halo column over the rows of group g; rows and columns past the grid
 * clamped into it as the sweep's loads are; {-inf, +inf} for a block that holds a NaN.  mc33hip_block_words: the verdict word per
 * strip, [resident plane][y tile][row segment], of the last single-isovalue sweep that went by a live list - two bits per entry,
 * 0 live, 1 all samples strictly below the isovalue, 2 all strictly above; all ones where no sweep has written a word (the strips
 * of dead tiles).  mc33hip_sweep_skipped_blocks: {blocks of the live tiles, blocks left out below the isovalue, above it} of the
 * sweep mc33hip_sweep_skipped speaks of (its out[3] stays what it was: callers hand it three words).  MC33HIP_EINVAL when there is
 * no table / was no such sweep.  MC33_HIP_BLOCKS=0 in the environment when a context is created: no block table, no block left out;
 * =1: blocks are left out in every sweep that goes by a live list; not set: in those over rows of at least four segments.
 * Only the library for float samples leaves blocks out; the others keep the table. */
int mc33hip_range_blocks(mc33hip_ctx *c, void *host_out, size_t bytes);
int mc33hip_block_words(mc33hip_ctx *c, void *host_out, size_t bytes);
int mc33hip_sweep_skipped_blocks(mc33hip_ctx *c, unsigned long long out[3]);
/* mc33hip_alias_cells: the cut cells of the last count that have a corner equal to the isovalue (they take the general per-cell
 * kernels), as the device counted them; for tests. */
int mc33hip_alias_cells(mc33hip_ctx *c, unsigned long long *out);
/* mc33hip_emit_shape: the launch shape of the emit passes enqueued last on this context (mc33hip_emit, mc33hip_extract and their
 * siblings), once its counters are on the host - the call waits for the context's stream: out = {work records, slow records,
 * record batches, blocks of the vertex pass, blocks of the triangle pass, blocks of the slow pass, the slow kernel (0: a thread
 * per record, 1: a lane per pattern slot, 2: left out - the tail found no cell with a corner equal to the isovalue to plan), 1 if
 * the triangle pass went first}.  The block counts are what was launched; the counts are the device's.  To be read before the
 * next call that counts.  MC33HIP_EINVAL when the context has emitted nothing.  For tests and tracing.
 * The grids follow the device and the counts of the extraction before; in the environment when a context is created,
 * MC33_HIP_EMIT_V_BLOCKS=<n> sets the vertex pass's grid and MC33_HIP_EMIT_BLOCKS=<n> the triangle pass's, both rounded up to a
 * multiple of 8 (blocks are dealt to the 8 XCDs in whole rounds), MC33_HIP_SLOW_BLOCKS=<n> the slow kernels'. */
int mc33hip_emit_shape(mc33hip_ctx *c, unsigned long long out[8]);
/* mc33hip_tail_shape: the shape of the tail (the passes between the sweep and the emit passes) of the last count on this context
 * (mc33hip_count, mc33hip_extract and their siblings) - the call waits for the context's stream: out = {slice slots of the range,
 * groups the slow-cell and dirty-segment lists were cut into, log2 of the slots per group, chunks of 2048 row segments of the
 * prefix sums, 1 if the sums went by groups of 32 chunks (from 4096 chunks on), blocks of the slot pass, slow cells listed, dirty
 * row segments listed}.  The two totals are the device's.  mc33hip_list_counts: the first n (at most 1024) group cursors of the
 * slow-cell list and of the dirty-segment list of that tail, copied to the host after a wait for the context's stream; a group
 * beyond those in use holds 0.  Both to be read before the next call that counts (the next tail clears the cursors).
 * MC33HIP_EINVAL when the context has counted nothing.  For tests and tracing. */
int mc33hip_tail_shape(mc33hip_ctx *c, unsigned long long out[8]);
int mc33hip_list_counts(mc33hip_ctx *c, unsigned int *slow, unsigned int *dirty, size_t n);
/* For tests and tracing as well.  mc33hip_sweep_plan: the sweep's plan in force - the one the last sweep, or the last tail, went
 * by - as tiles {row segment, y tile, z_lo, z_hi} in launch order, four consecutive tiles a block, into tiles_out (room for
 * cap_tiles tiles; NULL: info only); info = {tiles, blocks the device holds at once, 0: the plan of a sweep without a range
 * table / 1: with one}.  mc33hip_sweep_live: the live list of the last sweep made with a table, one word per block that had a
 * tile to stream, in plan order: block << 4 | mask of its waves with nothing to stream; info = {entries, blocks of that sweep's
 * plan}.  mc33hip_sweep_packed: the list that sweep's kernel went by, one 16-byte entry per block that had work (room for
 * cap_entries entries; NULL: info only): four tile indices of the plan, wave k of the block streamed tile k of its entry -
 * 0xFFFFFFFF: none (only in the last entry that is not a whole block of the plan); bit 31 of the first word: the entry is a whole group of the plan, all four tiles
 * live.  A block of the plan with four live tiles stays one entry, the live tiles of the other blocks are packed four at a time in
 * plan order, and the two kinds are merged by the plan position of their first tile.  info = {entries, live tiles, tiles of the
 * plan}; entries = ceil(live tiles / 4).  MC33HIP_EINVAL when there is no plan / was no such sweep.
 * The plan of a single-isovalue sweep with a table is sized by the live tiles the sweeps find, so that the packed blocks are a set
 * share of one round of the device; MC33_HIP_TABLE_TILES=<n> in the environment when a context is created asks for n tiles whatever they find, and an
 * explicit MC33_HIP_RZ or MC33_HIP_RZ_TABLE (a depth in planes) switches the sizing off.  Precedence: MC33_HIP_RZ alone makes the
 * plans with and without a table one plan of that depth, and nothing else is looked at; otherwise MC33_HIP_TABLE_TILES, a switch
 * for tests and curves, comes before MC33_HIP_RZ_TABLE and holds for grids of less than one round too; then MC33_HIP_RZ_TABLE; then
 * the sizing.  MC33_HIP_LIST_LDS=0 (tests): k_live_compact keeps the places of its quads in memory, as for plans above 4 096 blocks.
 * mc33hip_sweep_plan_weight: the weight of a plane, in batches of sample rows, that the columns of the plan in force were cut
 * with - 0: by batches alone, as every plan but the sized plan of a single-isovalue sweep that leaves blocks out.
 * MC33_HIP_PLANE_WEIGHT=<w> in the environment when a context is created: that weight in place of the measured one (curves,
 * tests); 0: none. */
int mc33hip_sweep_plan(mc33hip_ctx *c, unsigned int *tiles_out, size_t cap_tiles, unsigned long long info[3]);
int mc33hip_sweep_plan_weight(mc33hip_ctx *c, double *weight_out);
int mc33hip_sweep_live(mc33hip_ctx *c, unsigned int *live_out, size_t cap_entries, unsigned long long info[2]);
int mc33hip_sweep_packed(mc33hip_ctx *c, unsigned int *out, size_t cap_entries, unsigned long long info[3]);

/* Inclined (non-orthogonal) grid: vertices and normals go through the cell matrices like MC33_spnC does
 * (reference marching_cubes_33.c:587-621).  grd_A / grd_Ai = _GRD._A / _GRD.A_ (3x3 row major, before the
 * scaling by d that create_MC33 applies, MC:1763-1770); triangular != 0 = the caller's mult_Abf is
 * _multTSA_bf (MC33_util_grd.c:86-97).  NULL matrices switch back to the orthogonal stores. */
int mc33hip_set_inclined(mc33hip_ctx *c, const double *grd_A, const double *grd_Ai, int triangular);

/* Orientation: on != 0 negates the normals and exchanges the first two indices of every triangle - what the reference
 * does when it is compiled with MC33_NORMAL_NEG 1 (reference source/libMC33.c:20-22, marching_cubes_33.c:509-513,
 * 1246-1250).  The libMC33_<type>_nneg.so flavour of the host layer switches it on in create_MC33. */
int mc33hip_set_normal_neg(mc33hip_ctx *c, int on);

/* Stream all work is enqueued on (a hipStream_t passed as void*; NULL = the default stream).  A caller that names its stream
 * orders its own work by it, and mc33hip_extract makes use of that: see "Completion" there.  Waits for whatever the context still
 * has on the stream it leaves. */
int mc33hip_set_stream(mc33hip_ctx *c, void *hip_stream);
/* ... or a non-blocking stream of the context's own, for callers without a HIP runtime of their own that drive several contexts
 * side by side (create_MC33 with MC33_HIP_DEVICES: one context per z-slab). */
int mc33hip_own_stream(mc33hip_ctx *c);
/* HIP devices visible to this process (0: none, or no runtime). */
int mc33hip_device_count(void);

/* Count pass only: classification + prefix sums; the device twin of size_of_isosurface (MC:1892-1940).
 * Synchronises the stream.
 * Over the library's own copy of the grid (mc33hip_upload*), a count that has not served an emit yet is reused by the next
 * mc33hip_count of the same isovalue and range: size_of_isosurface followed by calculate_isosurface of that value streams the
 * volume once.  Used once only - an extraction repeated with the same isovalue does all of its work again - and never with a
 * buffer of the caller's (mc33hip_adopt_device), whose samples may change without this library knowing. */
int mc33hip_count(mc33hip_ctx *c, double iso, const mc33hip_range *range, mc33hip_counts *out);

/* Iso sweep over the resident grid (BASELINE.json configs[4]; the caller of calculate_isosurfaces): classifies the
 * samples against n <= 8 isovalues while streaming the volume ONCE per 4 isovalues, instead of once per isovalue as n
 * separate calls do (the reference re-reads all of F for every isovalue, MC:1832-1868).  Nothing is returned: the
 * mc33hip_count / mc33hip_extract calls that follow with one of these isovalues and the same range find the sweep
 * already made and only run the passes after it.  A sweep made ahead is used once and is dropped when the grid changes.
 * Asynchronous on the context's stream. */
int mc33hip_sweep_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *range);

/* The same, and everything else a count needs as well - record ranges, cell records, prefix sums - right behind each pass
 * over the grid, one launch of every kernel for the 4 isovalues of the pass, each isovalue into buffers of its own.  The
 * mc33hip_count calls that follow only fetch counters, mc33hip_emit / mc33hip_extract only emit - in any order, any number
 * of times, until the next mc33hip_prepare_many / mc33hip_sweep_many or a change of the grid.  For callers that need the
 * counts of ALL isovalues before the first emit: z-slabs over several GPUs exchange them in ONE collective per step and
 * then emit every isovalue at its global id base (mc33_c_library_amd/slabs.py: extract_slab_many).  On one GPU
 * mc33hip_sweep_many + mc33hip_extract per isovalue is faster: an emit right behind its own tail finds the records in the
 * last-level cache.  Falls back to mc33hip_sweep_many when device memory does not allow the buffers.
 * At most 8 isovalues per call (MC33HIP_EINVAL beyond).  A mc33hip_count / mc33hip_extract of an isovalue or range that was
 * NOT prepared works in the buffers of prepared isovalue #0 and drops it: its next count sweeps the grid again (same
 * results, one more pass over the volume). */
int mc33hip_prepare_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *range);

/* Global number of the first vertex of the range last counted (z-slab decomposition: known only after
 * the ranks have exchanged their counts).  Takes effect in the next mc33hip_emit. */
int mc33hip_set_id_base(mc33hip_ctx *c, unsigned int id_base);

/* Emit pass for the range last counted, into caller-owned DEVICE buffers:
 * V: capV x 3 MC33_real (float; double in libMC33_f64), N: capV x 3 floats; T: capT x 3 unsigned.  The isovalue
 * is passed as a double and used as MC33_real.  Replaces the vertex/triangle appends of MC33_findCase
 * (MC:780-1252).  Asynchronous on the context's stream. */
int mc33hip_emit(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT);

/* A z-slab's count, count exchange and emit with no host round trip in between (the reference has no such
 * step - its one process numbers the vertices as it sweeps, MC:1783-1808).  mc33hip_count_async enqueues what mc33hip_count
 * does and returns; mc33hip_counts_to_device leaves {vertices, triangles} of the counted range as two 64-bit integers in DEVICE
 * memory (for a collective to gather: torch.distributed.all_gather_into_tensor over RCCL); mc33hip_bases_from_table turns the
 * gathered table - rank r's pair at device_table[r * stride] - into this rank's vertex id base and, with concatenated != 0, the
 * rows at which it writes into output arrays shared by all ranks (0: arrays of its own); mc33hip_emit_at_device_bases is
 * mc33hip_emit with those words read on the device (capacities are checked there too).  All four only enqueue on the context's
 * stream.  mc33hip_count_finish waits and brings the counts to the host: MC33HIP_ECAPACITY when the work records did not fit
 * (room has been made: repeat the step with mc33hip_count) or the outputs were too small. */
int mc33hip_count_async(mc33hip_ctx *c, double iso, const mc33hip_range *range);
int mc33hip_counts_to_device(mc33hip_ctx *c, long long *device_dst);
int mc33hip_bases_from_table(mc33hip_ctx *c, const long long *device_table, int stride, int rank, int concatenated);
int mc33hip_emit_at_device_bases(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT);
int mc33hip_count_finish(mc33hip_ctx *c, mc33hip_counts *out);

/* mc33hip_emit with the copy to the HOST pipelined behind it (what calculate_isosurface does, reference MC:1869-1879:
 * the surface in the caller's malloc blocks): hT (nT x 3 unsigned) is copied on a stream of the context's own as soon as the
 * passes that write T have been through, hV (nV x 3 MC33_real) and hN (nV x 3 floats) as soon as theirs have - the copies of
 * one array run beside the kernels of the other.  nV, nT are those of the mc33hip_count before.  Only enqueues;
 * mc33hip_download_wait returns when all three arrays are in host memory. */
int mc33hip_emit_download(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT,
                          void *hV, void *hN, void *hT);
int mc33hip_download_wait(mc33hip_ctx *c);

/* Whole extraction (count + emit) with ONE wait; fails with MC33HIP_ECAPACITY
 * (and reports the needed sizes in *out) when the buffers are too small.  This is the path
 * calculate_isosurface (MC:1816-1889) and bench.py use.
 * Completion.  The COUNTS (*out, the return code, MC33HIP_ECAPACITY included) are complete on return, always.  The OUTPUT ARRAYS are
 *   - complete on return when the context works on the default stream it was created with or on a stream of its own
 *     (mc33hip_own_stream), when timing is on (mc33hip_set_timing > 0), and whenever the call fails;
 *   - complete IN STREAM ORDER when the caller named the stream (mc33hip_set_stream, NULL included): the call returns as soon as
 *     the device has handed over the counters, with emit passes still queued or running on that stream.  The pass that writes
 *     the triangles hands them over as it starts: it runs first - and the call returns a whole emit stage early - up to 6 M work
 *     records; beyond that, or when the slow records run beside the fast ones, it runs behind the pass that writes
 *     V and N, and the call returns when only the triangle pass (and the slow pass) are left.  Kernels and copies
 *     the caller enqueues on the same stream behind the call see the arrays complete, and so does the next mc33hip_extract,
 *     which is enqueued behind the passes at once.  Every other entry point of the context - mc33hip_count, mc33hip_emit,
 *     mc33hip_synchronize, the downloads (the concurrent ones too), mc33hip_set_stream, mc33hip_set_timing, mc33hip_last_timing,
 *     uploads, mc33hip_adopt_device, the measuring / filtering / smoothing calls, mc33hip_destroy - waits for them first.  Reading
 *     the arrays by a road that is NOT ordered by the stream (another stream, a host pointer to the same memory, another
 *     process) needs mc33hip_synchronize first, as after mc33hip_emit.
 * When the arrays are too small, or the call fails otherwise, nothing has been written to them. */
int mc33hip_extract(mc33hip_ctx *c, double iso, const mc33hip_range *range, void *dV, void *dN, void *dT,
                    unsigned long long capV, unsigned long long capT, mc33hip_counts *out);

/* hipEvent times of the last extraction; all zero unless the context was created with MC33_HIP_TIMING=1 (whole call)
 * or 2 (per pass) in the environment - the event records cost about 20 us per call.  Waits for a pending mc33hip_emit. */
int mc33hip_last_timing(mc33hip_ctx *c, mc33hip_timing *t);

/* Switches the hipEvent timing of the context at run time (0, 1, 2 as MC33_HIP_TIMING, which only sets the level a context
 * starts with).  bench.py times its steps at level 2 - the events are recorded, never waited for - and once more at 0. */
int mc33hip_set_timing(mc33hip_ctx *c, int level);

/* Measurement aid (bench.py's `roofline.read_ceiling`): a plain read-only kernel over the resident grid -
 * every 16-byte chunk once (every block a contiguous piece, 16 loads in flight per lane: the shape that reads fastest on this part),
 * nothing written - timed with hipEvents on the context's stream, reps launches after a warm-up.
 * *bytes / *ms_best is what a read stream reaches on this device, in this process, on this very buffer: the ceiling the
 * sweep (MC:1832-1868, which reads every sample once) is set beside.  Not part of any extraction. */
int mc33hip_probe_read(mc33hip_ctx *c, int reps, float *ms_best, float *ms_median, unsigned long long *bytes);

/* Waits until everything enqueued on the context's stream (mc33hip_emit in particular) has finished.  Needed before
 * the output buffers are read by anything that is not ordered after that stream - mc33hip_download_concurrent, another
 * stream, another process. */
int mc33hip_synchronize(mc33hip_ctx *c);

/* Device-to-host copy helper for callers without a HIP runtime of their own (blocking). */
int mc33hip_download(mc33hip_ctx *c, void *host_dst, const void *device_src, size_t bytes);
/* The same on a stream of the context's own that neither waits for nor delays the work queued by the other entry
 * points: the download of one result can run while the next extraction is computed (calculate_isosurfaces does
 * that from a helper thread).  The source must not be written meanwhile.  Blocking; callable from any thread. */
int mc33hip_download_concurrent(mc33hip_ctx *c, void *host_dst, const void *device_src, size_t bytes);
/* Several copies, one wait at the end (a surface is three arrays): concurrent = 0 orders them after the context's
 * stream like mc33hip_download, != 0 uses the side stream like mc33hip_download_concurrent. */
int mc33hip_download_many(mc33hip_ctx *c, int n, void *const *host_dst, const void *const *device_src, const size_t *bytes,
                          int concurrent);
/* --- property grid: a second scalar field sampled at the vertices (no counterpart in the reference, which fills surface.color
 * with DefaultColorMC, MC:1875-1877) ----------------------------------------------------------------------------------------
 * The property grid has the extractor grid's points per axis and sample type; it is resident as a window of whole planes of its
 * own: global planes [plane0, plane0 + nplanes), independent of desc.plane0 / npz_resident.  Orthogonal grids only.
 *   upload_rows       : F[k][j] row pointers, k counts the window's planes (F = _GRD.F + plane0); staged like mc33hip_upload_rows
 *   upload_contiguous : the window's planes back to back in host memory
 *   adopt_device      : a caller-owned device buffer used in place, pitch / slice in samples (any pitch >= npx up to
 *                       0xFFFFFFFF, any slice >= pitch * npy, any alignment; only grid points are read)
 *   drop              : detaches (and frees the library's copy)
 * Attaching again replaces the window.  All four wait for the context's stream first. */
int mc33hip_property_upload_rows(mc33hip_ctx *c, const void *const *const *F, unsigned int plane0, unsigned int nplanes);
int mc33hip_property_upload_contiguous(mc33hip_ctx *c, const void *host_samples, unsigned int plane0, unsigned int nplanes);
int mc33hip_property_adopt_device(mc33hip_ctx *c, const void *device_samples, size_t pitch, size_t slice, unsigned int plane0,
                                  unsigned int nplanes);
int mc33hip_property_drop(mc33hip_ctx *c);

/* The property at nV vertices, dV: nV x 3 MC33_real in device memory (what mc33hip_emit wrote).  For a vertex v, in IEEE double
 * throughout: g = (v - r0) / d per axis; i = floor(g) clamped to [0, N]; f = g - i clamped to [0, 1], 0 where i == N;
 * lerp(p, q, f) = f == 0 ? p : p * (1 - f) + q * f (q is not read when f == 0) along x, then y, then z; the result rounded to
 * float.  mc33hip_sample_property leaves that float per vertex in dP; mc33hip_color_vertices maps it through n palette words
 * (0xAABBGGRR, 2 <= n <= 256, a HOST array, copied on the context's stream): s = (value - lo) / (hi - lo) clamped to [0, 1],
 * dC[v] = palette[(int)floor(s * (n - 1) + 0.5)], nan_color where the value is NaN.
 * Both only enqueue on the context's stream: behind an mc33hip_emit on it they see its vertices.  A vertex that needs a plane
 * outside the attached window is counted on the device (its result is NaN / nan_color): the next mc33hip_synchronize,
 * mc33hip_download, mc33hip_download_many (not concurrent) or mc33hip_download_wait returns MC33HIP_ERUNTIME and
 * mc33hip_last_error names the count.  MC33HIP_EINVAL: nothing attached, an inclined context (mc33hip_set_inclined with
 * matrices), n outside 2..256, lo >= hi or a NaN bound. */
int mc33hip_sample_property(mc33hip_ctx *c, const void *dV, unsigned long long nV, float *dP);
int mc33hip_color_vertices(mc33hip_ctx *c, const void *dV, unsigned long long nV, const int *palette, unsigned int n, double lo,
                           double hi, int nan_color, int *dC);
/* One more array for the pipelined download of mc33hip_emit_download: copied to the host on the context's copy stream as soon as
 * everything enqueued on the context's stream so far is through.  Only enqueues; mc33hip_download_wait waits for it too. */
int mc33hip_download_enqueue(mc33hip_ctx *c, void *host_dst, const void *device_src, size_t bytes);

/* --- measures of a finished mesh, taken on the device (no counterpart in the reference) -----------------------------------------
 * V (nV x 3 MC33_real) and T (nT x 3 unsigned) in device memory as mc33hip_emit wrote them for a whole grid (id base 0: T indexes
 * V directly); any such mesh, inclined grids and every sample type included.  Everything in IEEE double, nothing fused, for
 * triangle i with rows q0, q1, q2 = V[T[i][0..2]] and the reference point c[a] = r0[a] + 0.5 * ((double)N[a] * d[a]) of the
 * context's grid (it only conditions the sums):
 *   p_k = (double)q_k - c;  u = p1 - p0, w = p2 - p0;  n = u x w;  A_i = 0.5 * sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)
 *   m = p1 x p2;  W_i = ((p0.x*m.x + p0.y*m.y) + p0.z*m.z) / 6.0;  M_i[a] = A_i * (((p0[a] + p1[a]) + p2[a]) / 3.0)
 *   Q_i = A_i * ((((double)P[T[i][0]] + (double)P[T[i][1]]) + (double)P[T[i][2]]) / 3.0),  P: what mc33hip_sample_property left
 * volume is SIGNED, with the winding as T stores it: the reference's winding gives a sphere whose samples grow outwards a
 * NEGATIVE volume, a context with mc33hip_set_normal_neg on the opposite sign.  It is the enclosed volume only for a surface
 * that does not reach the grid's faces (an open sheet has no inside: `closed` of mc33hip_surface_topology below tells).  The area centroid is
 * origin + moment / area.  bbox_min / bbox_max: exact minimum / maximum of the rows of V per axis (+inf / -inf for nV == 0, a NaN
 * coordinate is skipped); NaN in V or P otherwise propagates into the sums.  The sums are accumulated in double from the first
 * addition on, without floating-point atomics: two calls on the same mesh in one process return the same bits.
 *
 * Components: two vertices are connected when a triangle names both; label[v] = the smallest vertex index connected to v; a
 * vertex no triangle names keeps label[v] = v and is unreferenced; a component is a connected set with at least one triangle.
 * The table lists the components in ascending order of root (= their label); a triangle belongs to label[T[i][0]].  The two
 * double columns are added with atomics and may differ in their last bits from call to call.
 *
 * All three enqueue on the context's stream behind whatever is on it, wait, and bring the small results to the host.  A triangle
 * that names a vertex >= nV is counted on the device, contributes nothing - nothing outside V is read - and the call returns
 * MC33HIP_ERUNTIME with the count in mc33hip_last_error.  MC33HIP_EINVAL: a null pointer where the size is not zero, nV or nT
 * above 2^32-1.  mc33hip_measure_components with capacity below the number of components returns MC33HIP_ECAPACITY with that
 * number in *components and leaves the table untouched (host_table NULL, capacity 0 asks for it); dLabel is what
 * mc33hip_label_components made for the same T and nV. */
typedef struct {
	unsigned long long nV, nT;
	double area, volume;          /* sum A_i, sum W_i                                  */
	double moment[3], origin[3];  /* sum M_i about origin = c                          */
	double bbox_min[3], bbox_max[3];
	double property_integral;     /* sum Q_i; 0 and has_property 0 when dP == NULL     */
	int has_property;
} mc33hip_measures;
typedef struct { unsigned root, nV, nT; double area, volume; } mc33hip_component;

int mc33hip_measure_surface(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT,
                            const float *dP, mc33hip_measures *out);
int mc33hip_label_components(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, unsigned *dLabel,
                             unsigned long long *components, unsigned long long *unreferenced);
int mc33hip_measure_components(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT,
                               const unsigned *dLabel, mc33hip_component *host_table, unsigned long long capacity,
                               unsigned long long *components);

/* --- topology of a finished mesh, taken on the device (no counterpart in the reference) ----------------------------------------
 * T (nT x 3 unsigned) in device memory and nV, as for mc33hip_label_components; V is not read.  Everything is an integer, and
 * two calls on the same T return the same bytes, whatever the scheduling.
 *   invalid triangle     names a vertex >= nV: counted, contributes nothing; the call returns MC33HIP_ERUNTIME with the count in
 *                        mc33hip_last_error, in the words of the measuring calls.
 *   degenerate triangle  a valid triangle with two equal indices.  Its sides a -> a are skipped, its other sides enter the
 *                        table like any side, and it still counts in nT.
 *   edge                 every other side a -> b of a valid triangle, in the order T0 -> T1, T1 -> T2, T2 -> T0, is a use of the
 *                        undirected edge {lo, hi} = {min(a, b), max(a, b)}: FORWARD if a < b, else BACKWARD.  Use counts are
 *                        exact 32-bit numbers per direction.
 *   edges                distinct edges;   boundary_edges: edges with exactly one use;   nonmanifold_edges: more than two uses;
 *   misoriented_edges    exactly two uses, both forward or both backward.
 *   referenced_vertices  vertices a valid triangle names: nV - unreferenced of mc33hip_label_components.
 *   euler                (long long) referenced_vertices - edges + (nT - invalid)
 *   boundary_loops       connected components of the graph the boundary edges form.  A count of loops only where every boundary
 *                        vertex ends two boundary edges (where corners equal the isovalue some end more); defined all the same.
 *   closed = boundary_edges == 0;  oriented = misoriented_edges == 0;
 *   manifold = nonmanifold_edges == 0 && degenerate_triangles == 0: EDGE-manifold only - a pinched vertex (two fans of
 *                        triangles that meet in one vertex and in no edge) is not detected.
 * Per component - the rows of mc33hip_measure_components, in ascending order of root: an edge belongs to label[lo] (both ends
 * have one label), a degenerate triangle to label[T[i][0]], a boundary loop to the label of its smallest vertex.  The columns
 * are the same counts, euler = nV - edges + nT of the component, and
 *   genus = (2 - euler - boundary_loops) / 2  when the component has no non-manifold edge, no degenerate triangle and no
 *           misoriented edge and that numerator is even and >= 0; else -1.
 * The surface's struct adds components, closed_components (rows with boundary_edges == 0), genus_sum (over the rows with
 * genus >= 0) and genus_defined (1 iff no row has -1).  nV and nT repeat the arguments; with nT == 0 everything else is 0,
 * closed = manifold = oriented = genus_defined = 1 and the table is empty.
 *
 * Both calls enqueue on the context's stream behind whatever is on it, wait, and bring the small results to the host.  They
 * build an edge table in device memory - 16 bytes per slot, a power of two >= 4 nT slots: 4.3 GB for 55.8 M triangles -
 * MC33HIP_ENOMEM when it cannot be had; it stays with the context until mc33hip_destroy.  mc33hip_surface_topology labels the
 * components itself, in scratch of its own, and fills *out also when it returns MC33HIP_ERUNTIME for invalid triangles (they
 * are left out).  mc33hip_component_topology takes dLabel from mc33hip_label_components for the same T and nV; MC33HIP_EINVAL,
 * MC33HIP_ECAPACITY (the number in *components, the table untouched; host_table NULL, capacity 0 asks for it) and
 * MC33HIP_ERUNTIME as mc33hip_measure_components. */
typedef struct {
	unsigned long long nV, nT, referenced_vertices, edges, boundary_edges, nonmanifold_edges, misoriented_edges,
	                   degenerate_triangles, boundary_loops, components, closed_components, genus_sum;
	long long euler;
	int closed, manifold, oriented, genus_defined;
} mc33hip_topology;
struct mc33hip_component_topology { /* (a tag, not a typedef: C keeps the function of the same name in another name space) */
	unsigned root, nV, nT;
	unsigned long long edges, boundary_edges, nonmanifold_edges, misoriented_edges, degenerate_triangles, boundary_loops;
	long long euler;
	int genus;
};

int mc33hip_surface_topology(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, mc33hip_topology *out);
int mc33hip_component_topology(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, const unsigned *dLabel,
                               struct mc33hip_component_topology *host_table, unsigned long long capacity,
                               unsigned long long *components);

/* --- keep or drop components of a finished mesh, on the device (no counterpart in the reference) ----------------------------------
 * An order-preserving, deterministic stream compaction of V (nV x 3 MC33_real), N (nV x 3 float), T (nT x 3 unsigned, id base 0)
 * and n_attr <= 2 arrays of one 4-byte word per vertex (a colour, a sampled property, anything) by component; label[nV] is what
 * mc33hip_label_components made for this T and nV; roots: a HOST array of n_roots component roots, in any order, duplicates
 * allowed.  Everything is an integer or a row moved as it is: no tolerance anywhere, and two calls on the same inputs return the
 * same bytes.
 *   valid triangle   its three indices are below nV;            referenced[v]  a valid triangle names v
 *   selected[v]      (label[v] is one of the roots) XOR (invert != 0)
 *   keep[v]          referenced[v] AND selected[v];             new[v]         the number of kept u < v
 *   kept triangle    valid, and keep[T[i][0]] holds
 *   oV[new[v]], oN[new[v]], oAttr[k][new[v]] = the bytes of row v for every kept v (ascending);  oT = the kept triangles in their
 *   original order, each index replaced by new[...];  oMap[nV] (optional) = new[v] for kept v, 0xFFFFFFFF otherwise - it lets a
 *   caller carry further arrays of its own.
 * A vertex no triangle names is always dropped: a compaction with every root selected (n_roots 0, invert 1) removes the
 * unreferenced vertices and nothing else.  A root that is not the root of a component with at least one triangle selects nothing
 * and is no error.  The call fills nV_out, nT_out and components_kept (the kept v with label[v] == v); nT == 0 gives 0, 0 and
 * success.
 *   MC33HIP_ERUNTIME   an invalid triangle is counted and left out, and so is a kept triangle that names a vertex that is not
 *                      kept (labels that are not those of this T); the count is in mc33hip_last_error, in the words of the
 *                      measuring calls, the outputs are otherwise complete, nothing outside the arrays is read or written.
 *   MC33HIP_ECAPACITY  capV < nV_out or capT < nT_out: the needed sizes are in the struct and no output array is touched (null
 *                      outputs with capacity 0 are the size query; nV and nT are always enough).
 *   MC33HIP_EINVAL     a null pointer where a size is not zero, nV or nT above 2^32-1, n_attr > 2, a root >= nV, an output byte
 *                      range (capV / capT rows, nV words of oMap) that meets an input byte range - the compaction is not in
 *                      place; the check is made on the host, on addresses.
 * The call enqueues on the context's stream behind whatever is on it, waits, and brings the three counts to the host, as
 * mc33hip_measure_components does.  Scratch: 6 bytes per vertex and a word per 1024 vertices and triangles, with the context
 * until mc33hip_destroy. */
typedef struct {
	const void *V, *N, *T;                    /* in: the mesh (device)                                  */
	const unsigned *label;                    /* in: nV words (device)                                  */
	unsigned long long nV, nT;
	const void *attr[2];                      /* in: n_attr arrays of nV 4-byte words (device)          */
	unsigned n_attr;
	int invert;
	const unsigned *roots;                    /* in: n_roots words (HOST)                               */
	unsigned long long n_roots;
	void *oV, *oN, *oT;                       /* out: capV, capV, capT rows (device)                    */
	void *oAttr[2];                           /* out: capV words each                                   */
	unsigned *oMap;                           /* out: nV words, or NULL                                 */
	unsigned long long capV, capT;
	unsigned long long nV_out, nT_out, components_kept; /* filled by the call                           */
} mc33hip_compaction;

int mc33hip_compact_components(mc33hip_ctx *c, mc33hip_compaction *a);

/* --- smooth a finished mesh on the device: Taubin's lambda | mu passes, new normals (no counterpart in the reference) -------------
 * V (nV x 3 MC33_real) and T (nT x 3 unsigned, id base 0) in device memory, as for mc33hip_label_components; any mesh, inclined
 * grids and every sample type included.  N is not read.  T is not changed: what mc33hip_surface_topology and the component calls
 * reported stays true.  Everything is a gather in a fixed order: two calls on the same inputs return the same bytes.
 *   valid triangle   its three indices are below nV.  Every side a -> b with a != b of a valid triangle, in the order T0 -> T1,
 *                    T1 -> T2, T2 -> T0, is one use of the edge {a, b} (the words of the topology block).  An invalid triangle is
 *                    counted and contributes nothing - nothing outside V is read; the call still completes and returns
 *                    MC33HIP_ERUNTIME with the count in mc33hip_last_error, in the words of the measuring calls.
 *   nb(v)            the distinct w for which {v, w} has at least one use, in ascending order;  deg(v) = |nb(v)|
 *   boundary(v)      some edge {v, w} has exactly one use
 *   fixed(v)         deg(v) == 0, or pin_boundary != 0 and boundary(v)
 *   one pass with factor f, P -> P', rows of MC33_real: for a fixed v row v is copied as it is; otherwise per axis a, in IEEE
 *                    double, nothing fused:
 *                      s = (double)P[w1][a];  s = s + (double)P[wk][a] for k = 2 .. deg, in ascending w;  m = s / (double)deg
 *                      L = m - (double)P[v][a];  P'[v][a] = (MC33_real)((double)P[v][a] + f * L)
 *                    All neighbours are read from P, never from P' (a Jacobi update).
 *   one iteration    pass(lambda) followed by pass(mu).  A factor equal to 0 skips its pass - the rows stay as they are bit for
 *                    bit; it is not p + 0 * L, which turns -0 into +0.  With iterations == 0 oV holds V's bytes.
 *   normals          from the final positions Q.  inc(v): the valid triangles that name v, ascending, each once even if it names v
 *                    twice.  g_i = u x w with p_k = (double)Q[T[i][k]], u = p1 - p0, w = p2 - p0, that is
 *                    (u.y*w.z - u.z*w.y, u.z*w.x - u.x*w.z, u.x*w.y - u.y*w.x);  n = the g_i added in that order, starting from
 *                    the first;  len = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z);  oN[v][a] = (float)(n[a] / len) when len > 0 and
 *                    finite, otherwise - and for empty inc(v) - (0, 0, 0).  The stored winding decides the sign: with the
 *                    reference's winding this agrees with the emitted N, and so it does with mc33hip_set_normal_neg on, which
 *                    exchanges two indices and negates N.
 *   NaN propagates; nothing is special-cased.
 * The call fills max_degree, isolated_vertices (deg 0), boundary_vertices (whether pinned or not) and invalid_triangles.
 * mc33hip_vertex_normals is the normals alone, of V as it is.
 *   MC33HIP_EINVAL (checked on the host, nothing is written): a null pointer where the size is not zero (oN of the struct may be
 *                    NULL: no normals); nV or nT above 2^32-1; lambda outside (0, 1], mu outside [-1, 0], or a NaN; iterations
 *                    above 1000; oV meeting V other than oV == V (in place), oV or oN meeting any other array of the call.
 *   MC33HIP_ENOMEM   the scratch cannot be had - or nT is above 715 827 882: the rows of the lists begin at 32-bit offsets.
 *   nT == 0 is success: oV holds V's bytes, oN is zeros, the four counts are 0 apart from isolated_vertices = nV.
 * Both calls enqueue on the context's stream behind whatever is on it, wait, and bring the four integers to the host, as
 * mc33hip_compact_components does.  Scratch, with the context until mc33hip_destroy: 9 bytes and one row of MC33_real (12; 24 in
 * libMC33_f64) per vertex, 24 bytes per triangle (mc33hip_vertex_normals: 9 per vertex, 12 per triangle), a word per 1024
 * vertices.  The list of the normals is built in the arrays of the adjacency when the passes are through. */
typedef struct {
	const void *V, *T;  unsigned long long nV, nT;      /* in (device) */
	unsigned iterations;  double lambda, mu;  int pin_boundary;
	void *oV;           /* out: nV x 3 MC33_real; may be exactly V (in place), otherwise must not meet V, T */
	float *oN;          /* out: nV x 3, or NULL */
	unsigned long long max_degree, isolated_vertices /* deg 0 */, boundary_vertices, invalid_triangles;   /* filled */
} mc33hip_smoothing;
int mc33hip_smooth_surface(mc33hip_ctx *c, mc33hip_smoothing *a);
int mc33hip_vertex_normals(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT, float *oN);
/* Measurement aid: hipEvent times of the context's last mc33hip_smooth_surface / mc33hip_vertex_normals, recorded only at timing
 * level 2 (mc33hip_set_timing) - the adjacency build, the normals, and the first *passes <= 64 passes (pass_ms[capacity]); zeros
 * otherwise. */
int mc33hip_smooth_timing(mc33hip_ctx *c, float *adjacency_ms, float *normals_ms, float *pass_ms, unsigned capacity, unsigned *passes);

/* --- simplify a finished mesh on the device: vertex clustering on a lattice (no counterpart in the reference) ---------------------
 * V (nV x 3 MC33_real) and T (nT x 3 unsigned, id base 0) in device memory, as for mc33hip_label_components, and n_attr <= 2
 * arrays of one 4-byte word per vertex.  The vertices that fall into one cell of an axis-aligned lattice become one vertex;
 * triangles that lose a corner that way go, and so do, when asked, triangles that repeat another.  Integer atomics and exclusive
 * sums decide everything: the result is an exact function of the input, nothing has a tolerance, and two calls on the same inputs
 * return the same bytes.  Arithmetic is IEEE double, nothing fused.
 *   valid triangle   its three indices are below nV.  An invalid triangle is counted and contributes nothing; nothing outside V
 *                    is read.
 *   referenced[v]    a valid triangle names v.  Only referenced vertices take part in anything below; an unreferenced vertex is
 *                    dropped, as in the compaction.
 *   key of v         per axis a:  g = ((double)V[v][a] - origin[a]) / cell[a];  k_a = floor(g), but k_a = 0 when !(g >= 0) - a
 *                    NaN too - and k_a = 2097151 when g >= 2097152;  t_a = g - (double)k_a, clamped to [0, 1] and 0 for a NaN;
 *                    key = k_x | k_y << 21 | k_z << 42.  A referenced vertex clamped on any axis counts once in clamped_vertices:
 *                    a statistic, not an error.
 *   cluster          the referenced vertices that share one key.  rep(v): the smallest index in v's cluster;  clusters: how many
 *                    there are;  max_cluster: the largest member count.
 *   image            of valid triangle i: (rep(T0), rep(T1), rep(T2)).  Collapsed when two of the three are equal - counted in
 *                    collapsed_triangles.  With drop_duplicates != 0, images that are not collapsed and consist of the same three
 *                    representatives, in any order and either winding, are duplicates: of each such set the triangle with the
 *                    smallest i survives, the others count in duplicate_triangles.
 *   survivors        the valid triangles that are neither collapsed nor dropped as duplicates;  nT_out: how many.
 *   kept cluster     a survivor names its representative;  new[r]: the number of kept representatives below r;  nV_out: how many.
 *   oT               the survivors in their original order, each index replaced by new[rep(.)], the winding as stored.
 *   oV[new[r]]       MC33HIP_SIMPLIFY_FIRST: the bytes of row r of V - the vertex stays on the isosurface; -0 and NaN payloads
 *                    are preserved.  MC33HIP_SIMPLIFY_MEAN, per axis a, over ALL members of the cluster (n of them):
 *                      q = (unsigned long long)floor(t_a * 4294967296.0);   S_a = the sum of the q, an exact 64-bit integer in
 *                      any order of addition (at most (2^32 - 1) members x 2^32 < 2^64);
 *                      m = (double)S_a / ((double)n * 4294967296.0);   oV = (MC33_real)(origin[a] + cell[a] * ((double)k_a + m))
 *                    The quantisation moves the mean by less than cell[a] * 2^-32.
 *   oAttr[j][new[r]] = attr[j][r], the representative's word.
 *   oMap[v]          new[rep(v)] for a referenced v of a kept cluster, otherwise 0xFFFFFFFF (optional).
 *   oN               when not NULL, exactly what mc33hip_vertex_normals(oV, nV_out, oT, nT_out) writes: the incidence and normal
 *                    passes of the smoothing block run on the outputs.
 *   MC33HIP_ERUNTIME   invalid triangles: the count is in mc33hip_last_error, in the words of the measuring calls; the outputs
 *                      are complete without them.
 *   MC33HIP_ECAPACITY  capV < nV_out or capT < nT_out: every filled field is valid and no output array is touched (null outputs
 *                      with capacity 0 are the size query; nV and nT are always enough).
 *   MC33HIP_EINVAL     checked on the host, nothing is written: a null pointer where a size is not zero (oN and oMap may be
 *                      NULL); nV or nT above 2^32-1; n_attr > 2; a mode that is neither; a cell component that is not finite and
 *                      > 0; an origin component that is not finite; an output byte range (capV / capT rows, nV words of oMap)
 *                      that meets an input range or another output range - the call is not in place.
 *   MC33HIP_ENOMEM     the scratch cannot be had.
 *   nT == 0 is success with every count 0 (oMap, when given, is all 0xFFFFFFFF).
 * The call enqueues on the context's stream behind whatever is on it, waits, and brings the eight integers to the host, as
 * mc33hip_compact_components does; with oN it waits a second time, behind the normals.  Scratch, with the context until
 * mc33hip_destroy: 14 bytes per vertex and a cluster table of 40 bytes per slot, a power of two >= 2 nV slots (80 to 160 bytes per
 * vertex); 1 byte per triangle and, with drop_duplicates, a table of 4-byte words, a power of two >= 2 nT of them (8 to 16 bytes
 * per triangle); a word per 1024 vertices and triangles; with oN the scratch of mc33hip_vertex_normals for the OUTPUT's sizes. */
#define MC33HIP_SIMPLIFY_MEAN 0
#define MC33HIP_SIMPLIFY_FIRST 1
typedef struct {
	const void *V, *T;  unsigned long long nV, nT;   /* in (device): nV x 3 MC33_real, nT x 3 unsigned, id base 0 */
	const void *attr[2]; unsigned n_attr;            /* in: <= 2 arrays of nV 4-byte words (device) */
	double origin[3], cell[3];                       /* the lattice */
	int mode;                                        /* MC33HIP_SIMPLIFY_MEAN 0, MC33HIP_SIMPLIFY_FIRST 1 */
	int drop_duplicates;
	void *oV, *oT;  float *oN /* or NULL */;  void *oAttr[2];  unsigned *oMap /* nV words, or NULL */;
	unsigned long long capV, capT;
	unsigned long long nV_out, nT_out, clusters, max_cluster, collapsed_triangles, duplicate_triangles,
	                   invalid_triangles, clamped_vertices;   /* filled */
} mc33hip_simplification;
int mc33hip_simplify_surface(mc33hip_ctx *c, mc33hip_simplification *a);

/* --- resample the resident grid into a second device grid: taps and strides (no counterpart in the reference) --------------------
 * A separable correlation with up to 17 taps per axis, the grid's edge samples replicated, and an integer stride per axis: a
 * Gaussian before the extraction, a volume reduced by 2 or 3 per axis for a preview surface, or both, without the samples leaving
 * the device.  The result is an exact function of the input: nothing has a tolerance, and two calls return the same bytes.
 *   source      the grid resident in the context - the library's own copy or an adopted buffer - with np[a] points per axis
 *               (a: x = 0, y = 1, z = 2) and samples F[z][y][x] of the library's sample type.  The context must hold a WHOLE grid:
 *               plane0 == 0 and npz_resident == nz_total + 1; a z-slab context is MC33HIP_EINVAL.
 *   per axis a  ntaps[a] odd, radius r[a] = (ntaps[a] - 1) / 2 <= 8; taps[a] a HOST array of ntaps[a] finite doubles;
 *               taps[a] == NULL means the single tap {1.0} (ntaps[a] is ignored then); stride[a] >= 1.
 *   output size np_out[a] = (np[a] - 1) / stride[a] + 1 in integer division; at least 2 on every axis, else MC33HIP_EINVAL.
 *   arithmetic  IEEE double, nothing fused; every sum starts from its first product and adds the others in ascending tap index;
 *               cl(i, n) = min(max(i, 0), n - 1).  A correlation, not a flipped convolution: tap i multiplies the sample at
 *               offset i - r.
 *                 A(x, y, z)   = (double)F[z][y][x]
 *                 Sx(X, y, z)  = sum_i  taps[0][i] * A(cl(X*stride[0] + i - r[0], np[0]), y, z)
 *                 Sy(X, Y, z)  = sum_j  taps[1][j] * Sx(X, cl(Y*stride[1] + j - r[1], np[1]), z)
 *                 Sz(X, Y, Z)  = sum_k  taps[2][k] * Sy(X, Y, cl(Z*stride[2] + k - r[2], np[2]))
 *                 out[Z][Y][X] = convert(Sz(X, Y, Z))
 *   conversion  double samples: the value itself; float: (float)v; unsigned char / short / int with MAX of the type: 0 when
 *               !(v > 0) - a NaN included -, MAX when v >= MAX, otherwise (T)floor(v + 0.5).
 *               The intermediates are exact doubles: any tiling, fusion of axes or order of passes gives the same bits.
 *   geometry    of the output grid: r0_out = r0, d_out[a] = d[a] * (double)stride[a], nz_total_out = np_out[2] - 1.
 *   dst         device memory with the layout mc33hip_adopt_device takes - pitch / slice in samples, pitch >= np_out[0],
 *               slice >= pitch * np_out[1], any base address a sample may have.  ONLY the np_out grid points are written: padding
 *               keeps its bytes.  Of the source only grid points are read, which lies within the readable extent
 *               mc33hip_adopt_device states.  The result never depends on either layout; the speed may.
 *   MC33HIP_EINVAL  checked on the host, nothing is written: a null pointer; an even ntaps or a radius above 8; a tap that is not
 *               finite; a zero stride; an output axis below 2 points; a slab context (or one without a grid); a bad pitch /
 *               slice; a dst byte range - first to last grid point - that meets the source grid's (the call is not in place).
 *   MC33HIP_ENOMEM  the scratch - the taps in device memory, 416 bytes, with the context until mc33hip_destroy - cannot be had.
 * mc33hip_resample_grid copies the taps to the device, enqueues on the context's stream behind whatever is on it, and waits.
 * mc33hip_resampled_size makes the same checks of the struct and leaves np_out; nothing is enqueued. */
typedef struct { const double *taps[3]; unsigned ntaps[3]; unsigned stride[3]; } mc33hip_resampling;
int mc33hip_resampled_size(mc33hip_ctx *c, const mc33hip_resampling *r, unsigned np_out[3]);
int mc33hip_resample_grid(mc33hip_ctx *c, const mc33hip_resampling *r, void *dst, size_t pitch, size_t slice);
/* The HIP device ordinal the context works on - what desc.device = -1 resolved to in mc33hip_create (MC33HIP_EINVAL for NULL): a
 * second context for the resampled grid is created on this device, whatever the current device has become since. */
int mc33hip_context_device(mc33hip_ctx *c);

/* --- rank-filter the resident grid into a second device grid: minimum, median, maximum windows (no counterpart in the reference) --
 * A 3 x 3 x 3 median removes isolated spikes and leaves a step edge where it is; a minimum window followed by a maximum window of
 * the same radius is an opening, the other order a closing.  A rank filter SELECTS one of its input samples and computes nothing
 * new: the result is an exact function of the input, nothing has a tolerance, any tiling gives the same bytes.
 *   source      the grid resident in the context - the library's own copy or an adopted buffer at any pitch, slice and alignment -
 *               with np[a] points per axis (a: x = 0, y = 1, z = 2) and samples F[z][y][x] of the library's sample type.  The
 *               context must hold a WHOLE grid: plane0 == 0 and npz_resident == nz_total + 1.
 *   key         the only ordering the filter uses.  Unsigned char, short and int: the value itself.  Float with bit pattern b:
 *               b ^ 0xFFFFFFFF when the sign bit is set, otherwise b | 0x80000000; double: the same on 64 bits.  Ascending keys
 *               give: NaN with the sign bit set, -inf, ..., -0, +0, ..., +inf, NaN without the sign bit.  Two samples with equal
 *               keys have equal bytes, so no tie rule is needed.  No floating-point comparison decides anything.
 *   window      with cl(i, n) = min(max(i, 0), n - 1), the window of output point (x, y, z) is the multiset of the
 *               n = (2 radius[0] + 1)(2 radius[1] + 1)(2 radius[2] + 1) samples F[cl(z + dz, np[2])][cl(y + dy, np[1])][cl(x + dx, np[0])]
 *               for |dx| <= radius[0], |dy| <= radius[1], |dz| <= radius[2]: edge samples are replicated, and a replicated sample
 *               counts once for every offset that lands on it.
 *   output      out[z][y][x] holds the bytes of the window's sample of rank k in ascending key order: k = 0 for MC33HIP_RANK_MIN,
 *               k = n - 1 for MC33HIP_RANK_MAX, k = (n - 1) / 2 for MC33HIP_RANK_MEDIAN (n is odd: the median is one sample).  The
 *               bytes are kept as they are, NaN payloads and -0 included.  The output grid has the source's size, r0, d and
 *               inclined matrices.
 *   limits      MIN and MAX: radius[a] <= 8.  MEDIAN: radius[a] <= 1 - windows of 1, 3, 9 or 27 samples, the per-slice 3 x 3 median
 *               of anisotropic stacks and the 3 x 3 x 3 median among them.  All radii 0 is a copy of the grid points.
 *   separable   the minimum of a box is the minimum along z of the minima along y of the minima along x, and every step is a pure
 *               selection: composing the three per-axis passes is exact, for the maximum likewise.  An implementation of MIN and
 *               MAX may therefore work axis by axis (this one does, inside a block); the median is not separable.
 *   dst         device memory with the layout mc33hip_adopt_device takes - pitch / slice in samples, pitch >= np[0],
 *               slice >= pitch * np[1], any base address a sample may have.  ONLY grid points are written: padding keeps its
 *               bytes.  Of the source only grid points are read.  The result never depends on either layout.
 *   MC33HIP_EINVAL  checked on the host, with nothing enqueued or written: a null pointer; a rank that is none of the three; a
 *               radius above its limit; a slab context or one without a grid; a bad pitch / slice; a dst byte range - first to
 *               last grid point - that meets the source grid's (the call is not in place).
 * The call needs no scratch memory.  It enqueues on the context's stream behind whatever is on it, and waits. */
#define MC33HIP_RANK_MIN    0
#define MC33HIP_RANK_MEDIAN 1
#define MC33HIP_RANK_MAX    2
typedef struct { unsigned radius[3]; int rank; } mc33hip_ranking;   /* radius per axis x, y, z, in samples */
int mc33hip_rank_grid(mc33hip_ctx *c, const mc33hip_ranking *r, void *dst, size_t pitch, size_t slice);

/* --- contour spectrum of the resident grid: cut cells and histogram per isovalue (Bajaj, Pascucci, Schikore 1997; no counterpart
 * in the reference) ---------------------------------------------------------------------------------------------------------------
 * For a ladder of isovalues: how many cells the surface cuts at each one, a histogram of the samples between the steps, and the
 * range of the samples - what a caller needs to choose an isovalue, from one pass over the grid instead of one mc33hip_count per
 * candidate.  Everything is an integer: nothing has a tolerance, and two calls return the same bytes.
 *   isovalues   isos: a HOST array of n doubles, 0 <= n <= 255, each converted to MC33_real as mc33hip_count converts its iso;
 *               after the conversion strictly ascending, none a NaN; +-inf is allowed.
 *   rank        of a grid point with sample F, r = (MC33_real)F: for a non-NaN r, rank(r) = #{ j : iso_j < r }, in 0 .. n; a NaN
 *               has rank n when its sign bit is set, else 0.  This is the side bit of every pass here and of the reference, for
 *               every isovalue at once: the bit for iso_k is rank > k (a NaN's sign is its own: mc33_cell.h, iso_diff).  For the
 *               isovalue -0.0 on a grid holding zeros the rule above stands (the one input that is not comparable
 *               with the reference).
 *   range       cell slices [z_begin, z_end) of the WHOLE grid; ghost_below and id_base are ignored.  z_begin < z_end <= nz_total,
 *               and the planes z_begin .. z_end must be resident in the context: whole grids and z-slab contexts both work.
 *   cut_cells[k], k < n      the cells of the range with min_rank <= k < max_rank over their eight corners: the cells
 *               mc33hip_count of iso_k reports as active_cells for the same range without a ghost slice.
 *   histogram[j], j <= n     the grid points with rank j, counted over the planes [z_begin, z_end) and plane z_end exactly when
 *               z_end == nz_total: disjoint ranges that tile the grid add up to the whole grid's histogram.
 *   points, cells            the totals just described.
 *   nan_samples              the NaN samples among the points: a statistic - they still sit in bin 0 or n.
 *   sample_min, sample_max   exact minimum and maximum of the non-NaN r as doubles, +inf / -inf when there are none; which zero
 *               is returned where both signs occur is unspecified.
 *   n == 0 is legal: histogram[0] == points and the range of the samples - the first call of a two-step ladder.
 * The result never depends on pitch, slice, alignment or what the padding holds, and only memory inside the readable extent
 * mc33hip_adopt_device states is read.  No extraction state is touched: a count waiting for its emit, sweeps and prepared
 * isovalues made ahead, the count-reuse rule, timing and attached property grids are as they were, and a mc33hip_emit or
 * mc33hip_extract behind a spectrum returns what it would have returned without it.
 *   MC33HIP_EINVAL  checked on the host, nothing is enqueued: a null pointer where a size is not zero (cut_cells and isos may be
 *               NULL with n == 0), n > 255, a NaN isovalue, isovalues not strictly ascending after the conversion (two doubles
 *               that round to one float included), a bad range, a context without a grid.
 *   MC33HIP_ENOMEM  the scratch - 6 KB, with the context until mc33hip_destroy - cannot be had.
 * The call enqueues on the context's stream behind whatever is on it, waits, and brings the small result to the host. */
typedef struct {
	const double *isos;               /* in: n isovalues (HOST)                              */
	unsigned n;
	unsigned long long *cut_cells;    /* out: n counts (HOST)                                */
	unsigned long long *histogram;    /* out: n + 1 counts (HOST)                            */
	unsigned long long points, cells, nan_samples;   /* filled by the call                   */
	double sample_min, sample_max;
} mc33hip_spectrum;
int mc33hip_grid_spectrum(mc33hip_ctx *c, const mc33hip_range *range, mc33hip_spectrum *s);

/* --- clip a finished mesh by a plane on the device: cut edges, new vertices (no counterpart in the reference) -------------------
 * V (nV x 3 MC33_real), N (nV x 3 float, may be NULL), T (nT x 3 unsigned, id base 0) in device memory, as for
 * mc33hip_compact_components, and n_attr <= 2 arrays of one 4-byte word per vertex.  The half space s >= 0 of plane[4] = a, b, c, w
 * stays (negate the four numbers for the other side): triangles inside it are kept, triangles the plane crosses are cut, and the
 * new vertex of a cut edge is shared by every triangle that uses the edge, so that a manifold input stays manifold.  Integer
 * atomics and exclusive sums decide who makes a new vertex and where every row lands; the arithmetic is IEEE double, nothing
 * fused: the result is an exact function of the input, nothing has a tolerance, two calls on the same inputs return the same bytes.
 *   s[v]             (((double)V[v][0] * a + (double)V[v][1] * b) + (double)V[v][2] * c) + w
 *   class of v       IN when s > 0, ON when s == 0, OUT otherwise - a NaN is OUT.
 *   valid triangle   its three indices are below nV.  An invalid triangle is counted and contributes nothing; nothing outside V
 *                    is read.
 *   walk             a valid triangle without an IN corner is dropped (dropped_triangles): triangles that lie in the plane or
 *                    touch it from outside go.  Otherwise its directed sides p -> q are taken in the stored order, side e =
 *                    T[e] -> T[(e + 1) % 3]: p is emitted unless it is OUT; then the cut vertex of {p, q} is emitted when one of
 *                    p, q is IN and the other OUT.  A side with an ON end is never cut: the vertices of an isosurface lie on
 *                    grid edges, a plane through a grid plane meets many of them exactly, and no zero-area triangle is planted
 *                    there.  The polygon has 3 or 4 entries e0 .. e3; the output is (e0, e1, e2) and, with four, (e0, e2, e3): the
 *                    winding is kept.  A triangle without an OUT corner is whole (whole_triangles), any other has a cut
 *                    (cut_triangles).  A triangle with two equal indices takes the same walk.
 *   cut edge         the undirected pair {lo, hi}, lo < hi by index.  t = s[lo] / (s[lo] - s[hi]); per axis the new row is
 *                    (MC33_real)((double)V[lo] + t * ((double)V[hi] - (double)V[lo])).  When s[lo] or s[hi] is not finite the new
 *                    vertex is a byte copy of the rows of the IN end: V, N and the attribute words.  nonfinite_vertices: the
 *                    vertices a valid triangle names whose s is not finite.
 *   oN               of a new vertex: x, y, z the same interpolation of the rows of N in double, m = sqrt((x*x + y*y) + z*z),
 *                    (float)(x / m), (float)(y / m), (float)(z / m); 0, 0, 0 when !(m > 0).  A kept vertex keeps the bytes of
 *                    its row.  oN needs N; with oN == NULL no normals are written.
 *   attributes       of a new vertex, by attr_mode[k]: MC33HIP_CLIP_COPY the word of the IN end; MC33HIP_CLIP_LERP_F32 the words
 *                    taken as floats, (float)((double)a_lo + t * ((double)a_hi - (double)a_lo)).  A kept vertex keeps its word.
 *   numbering        an old vertex is kept when an output triangle names it; new[v] = the number of kept vertices below v
 *                    (kept_vertices of them; on_plane_vertices: the kept ones whose class is ON).  The cut_vertices new vertices
 *                    follow at kept_vertices + rank, in ascending order of their owner: the smallest i << 2 | e over the uses
 *                    (triangle i, side e) of the cut edge.  nV_out = kept_vertices + cut_vertices.
 *   oT               the output triangles in the order of their input triangles, the one or two of a triangle side by side.
 *   oMap[v]          new[v] for a kept vertex, otherwise 0xFFFFFFFF (optional).
 *   MC33HIP_ERUNTIME   invalid triangles: the count is in mc33hip_last_error, in the words of the measuring calls; the outputs
 *                      are complete without them.
 *   MC33HIP_ECAPACITY  capV < nV_out or capT < nT_out: every filled field is valid and no output array is touched (null outputs
 *                      with capacity 0 are the size query; nV + 2 nT rows and 2 nT triangles are always enough).
 *   MC33HIP_EINVAL     checked on the host, nothing is written: a null pointer where a size is not zero (N, oN and oMap may be
 *                      NULL); nV or nT above 2^32-1; n_attr > 2; a mode of a used attribute that is neither; a plane with a
 *                      component that is not finite or with a, b, c all zero; oN without N; an output byte range (capV / capT
 *                      rows, nV words of oMap) that meets an input range or another output range - the call is not in place.
 *   MC33HIP_ENOMEM     the scratch cannot be had.
 *   nT == 0 is success with every count 0 (oMap, when given, is all 0xFFFFFFFF).
 * The call enqueues on the context's stream behind whatever is on it, waits once, and brings the ten integers to the host, as
 * mc33hip_compact_components does.  Scratch, with the context until mc33hip_destroy: 7 bytes per vertex, 1 byte per triangle, a
 * word per 1024 vertices and two per 1024 triangles, and the table of cut edges: 16 bytes per slot, a power of two >= 4 nT slots
 * (64 to 128 bytes per triangle). */
#define MC33HIP_CLIP_COPY 0
#define MC33HIP_CLIP_LERP_F32 1
typedef struct {
	const void *V, *N, *T;  unsigned long long nV, nT;   /* in (device): nV x 3 MC33_real, nV x 3 float or NULL, nT x 3 unsigned */
	const void *attr[2]; unsigned n_attr;                /* in: <= 2 arrays of nV 4-byte words (device) */
	int attr_mode[2];                                    /* MC33HIP_CLIP_COPY 0, MC33HIP_CLIP_LERP_F32 1 */
	double plane[4];                                     /* a, b, c, w: s = a x + b y + c z + w, s >= 0 stays */
	void *oV;  float *oN /* or NULL */;  void *oT;  void *oAttr[2];  unsigned *oMap /* nV words, or NULL */;
	unsigned long long capV, capT;
	unsigned long long nV_out, nT_out, kept_vertices, cut_vertices, on_plane_vertices, whole_triangles, cut_triangles,
	                   dropped_triangles, invalid_triangles, nonfinite_vertices;   /* filled */
} mc33hip_clipping;
int mc33hip_clip_surface(mc33hip_ctx *c, mc33hip_clipping *a);

/* --- section a finished mesh by a plane on the device: contour points and segments, length, area (no counterpart in the reference) --
 * V (nV x 3 MC33_real) and T (nT x 3 unsigned, id base 0) in device memory, n_attr <= 2 arrays of one 4-byte word per vertex, and
 * plane[4] = a, b, c, w.  The section is the boundary that mc33hip_clip_surface opens on the same input: the outline where the
 * plane meets the surface, as points and directed segments.  Integer atomics and exclusive sums decide who makes a point and where
 * every row lands; the arithmetic is IEEE double, nothing fused: the outputs are an exact function of the input, two calls on the
 * same inputs return the same bytes - the doubles included.
 *   s[v], classes    IN / ON / OUT (a NaN is OUT) and the valid triangle: word for word those of mc33hip_clip_surface.
 *   segment          a valid triangle with an IN corner is walked exactly as clip walks it.  Of its polygon of 3 or 4 entries the
 *                    on-plane entries are the ON corners and the cut vertices; there are at most two, and they are neighbours in
 *                    the cyclic polygon.  With two of them the triangle yields one directed segment a -> b, in the polygon's order:
 *                    the orientation follows the stored winding.  A triangle without an IN corner yields nothing (triangles in the
 *                    plane, triangles that touch it from outside).  A segment whose two ends are the same point - a triangle that
 *                    names a vertex twice across or on the plane - is dropped and counted in degenerate_segments.
 *   points           first the ON vertices that a kept segment names, in ascending v (on_points of them); then the cut_points cut
 *                    points at on_points + rank: every cut edge of clip, in clip's owner order (the smallest i << 2 | e over its
 *                    uses), with clip's t and clip's interpolation, the byte copy of the IN end when s is not finite included:
 *                    oP[on_points + r] equals oV[kept_vertices + r] of mc33hip_clip_surface on the same input, bit for bit.
 *                    nP_out = on_points + cut_points.  isolated_points: points no kept segment names (cut points all of whose
 *                    segments were dropped).
 *   attributes       an ON point carries its vertex's word; a cut point follows attr_mode[k] as in clip.
 *   oS               nS_out x 2 unsigned into oP, in the order of the input triangles.
 *   oLabel[p]        the smallest point index joined to p through kept segments; a point no kept segment names keeps p (optional).
 *   oNext[p]         the end of the one kept segment that starts at p when exactly one does, otherwise 0xFFFFFFFF (optional): a
 *                    host walks a closed loop with it in O(n).
 *   oPointMap[v]     the point of an ON vertex that became one, otherwise 0xFFFFFFFF (nV words, optional).
 *   contours         sets of points joined by kept segments (with at least one segment); closed_contours: those in which every
 *                    point starts exactly one segment and ends exactly one; open_ends: points whose counts of starting and ending
 *                    segments differ; branch_points: points that start more than one segment, or end more than one.
 *   crossing_triangles  valid triangles with an IN and an OUT corner (clip's cut_triangles); invalid_triangles, nonfinite_vertices
 *                    as in clip.
 *   the doubles      per kept segment, with p = (double)oP[a] - o and q = (double)oP[b] - o, o = origin, the reference point of the
 *                    measures: length = sum sqrt(((q-p).x^2 + (q-p).y^2) + (q-p).z^2); area_vector = sum 0.5 * (p x q) with
 *                    (p x q) = (p.y q.z - p.z q.y, p.z q.x - p.x q.z, p.x q.y - p.y q.x); area = ((G0 a + G1 b) + G2 c) /
 *                    sqrt((a a + b b) + c c) with G = area_vector.  The sums are taken as mc33hip_measure_surface takes its own:
 *                    per lane, wave, block, then the rows of block partials in a fixed order - no floating-point atomic.
 *                    area is SIGNED and follows the winding, as volume does: for a closed surface area has the sign of the volume
 *                    that mc33hip_measure_surface reports, whichever side of the plane is called IN (negating the plane turns
 *                    every segment and the normal round).  The reference's README sphere - samples growing outwards - extracted
 *                    by the plain libraries has volume < 0 and area < 0; the _nneg flavours, which store the opposite winding,
 *                    give the opposite sign.  |area| is the enclosed area only where every contour is closed.
 *   MC33HIP_ERUNTIME   invalid triangles, as in clip: the outputs are complete without them.
 *   MC33HIP_ECAPACITY  capP < nP_out or capS < nS_out: nP_out, nS_out, on_points, cut_points, degenerate_segments,
 *                      crossing_triangles, invalid_triangles and nonfinite_vertices are valid, no output array is touched, and the
 *                      counts over points and contours and the doubles are 0 (null outputs with capacity 0 are the size query; 2 nT
 *                      points and nT segments are always enough).
 *   MC33HIP_EINVAL     checked on the host, nothing is written: a null pointer where a size is not zero (oLabel, oNext and
 *                      oPointMap may be NULL); nV or nT above 2^32-1; n_attr > 2; a mode of a used attribute that is neither; a
 *                      plane with a component that is not finite or with a, b, c all zero; an output byte range (capP rows of oP,
 *                      oLabel, oNext and the attributes, capS of oS, nV words of oPointMap) that meets an input range or another
 *                      output range.
 *   MC33HIP_ENOMEM     the scratch cannot be had.
 *   nT == 0 is success with every count 0 (oPointMap, when given, is all 0xFFFFFFFF).
 * The call enqueues on the context's stream, waits once, and brings the integers and doubles to the host.  Scratch, with the
 * context until mc33hip_destroy: clip's (it is shared with mc33hip_clip_surface) and 1 byte per vertex, 1 per triangle, a word per
 * 1024 triangles, 17 bytes per point of min(capP, 2 nT) and 32 bytes per block of the sums. */
typedef struct {
	const void *V, *T;  unsigned long long nV, nT;       /* in (device): nV x 3 MC33_real, nT x 3 unsigned */
	const void *attr[2]; unsigned n_attr;                /* in: <= 2 arrays of nV 4-byte words (device) */
	int attr_mode[2];                                    /* MC33HIP_CLIP_COPY 0, MC33HIP_CLIP_LERP_F32 1 */
	double plane[4];                                     /* a, b, c, w: s = a x + b y + c z + w */
	void *oP;  void *oS;  void *oAttr[2];                /* out (device): capP x 3 MC33_real, capS x 2 unsigned, capP words each */
	unsigned *oLabel, *oNext /* capP words, or NULL */, *oPointMap /* nV words, or NULL */;
	unsigned long long capP, capS;
	unsigned long long nP_out, nS_out, on_points, cut_points, isolated_points, degenerate_segments, crossing_triangles,
	                   invalid_triangles, nonfinite_vertices, contours, closed_contours, open_ends, branch_points;   /* filled */
	double length, area_vector[3], area, origin[3];      /* filled */
} mc33hip_section;
int mc33hip_section_surface(mc33hip_ctx *c, mc33hip_section *a);

/* The contour table of a section: from its oP (nP x 3 MC33_real), oS (nS x 2 unsigned), oLabel (nP words) in device memory and the
 * plane, one row per contour - per label set that holds a segment - in ascending order of root, as mc33hip_measure_components
 * lists components.  A segment belongs to the label of its start.  points: the points of the set that a segment names; open_ends,
 * branch_points as in mc33hip_section_surface, over the set; closed: 1 where every point of the set starts exactly one segment and
 * ends exactly one.  length and area are the sums of the section's own per-segment terms - the segment's term of area is ((g.x a +
 * g.y b) + g.z c) / sqrt((a a + b b) + c c), g = 0.5 * (p x q) - added with floating-point atomics: they may differ in their last
 * bits from call to call, and their sums over the rows from the totals of the section.  host_table / capacity / *contours work as
 * for the component table: *contours is always filled; capacity < *contours is MC33HIP_ECAPACITY and leaves the table untouched
 * (capacity 0 with a NULL table is the size query).  MC33HIP_ERUNTIME: segments that name a point >= nP, or a label >= nP, are
 * counted (the words of the measuring calls) and left out.  MC33HIP_EINVAL: a null pointer where a size is not zero, nP or nS above
 * 2^32-1, a plane that is not finite or has no normal. */
typedef struct {
	unsigned root, points, segments, open_ends, branch_points;
	int closed;
	double length, area;
} mc33hip_contour;
int mc33hip_section_contours(mc33hip_ctx *c, const void *dP, unsigned long long nP, const void *dS, unsigned long long nS,
                             const unsigned *dLabel, const double plane[4], mc33hip_contour *host_table,
                             unsigned long long capacity, unsigned long long *contours);

/* The same along a stack of parallel planes, without geometry: V, T as above, a normal (a, b, c) and a HOST array of n <= 255
 * finite offsets w_k, strictly ascending.  HOST outputs: segments[n], length[n], area[n] and *invalid_triangles.  One pass over T,
 * V gathered once per triangle, no table: t depends only on {lo, hi}, so every triangle computes the same cut point.  s_k[v] is
 * formed as ((x a + y b) + z c) + w_k, so the classes of plane k are those of mc33hip_section_surface for plane (a, b, c, w_k) bit
 * for bit: segments[k] == nS_out of that call, exactly; length[k] and area[k] are sums of the very same terms, but added with
 * floating-point atomics - they may differ from that call, and from call to call, in their last bits.
 *   MC33HIP_EINVAL   n > 255; an offset that is not finite or not above the one before; a null pointer where a size is not
 *                    zero; a normal with a component that is not finite or all zero; nV or nT above 2^32-1.
 *   MC33HIP_ERUNTIME invalid triangles: counted and left out.  With n == 0 or nT == 0 nothing is read. */
int mc33hip_section_ladder(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT,
                           const double normal[3], const double *offsets, unsigned n, unsigned long long *segments, double *length,
                           double *area, unsigned long long *invalid_triangles);

/* --- close a finished mesh at the faces of a box of grid points: caps, new vertices (no counterpart in the reference) ---------------
 * V (nV x 3 MC33_real), N (nV x 3 float), T (nT x 3 unsigned, id base 0) in device memory, in arrays of capV and capT rows, as
 * mc33hip_extract left them over the RESIDENT grid for the isovalue `iso`; n_attr <= 2 arrays of capV 4-byte words per vertex.  The
 * call appends, in place, the faces that close the surface on the six faces of the box lo .. hi of grid points (lo[a] < hi[a] <=
 * N[a]; the whole grid, or the z bounds of a z-range extraction): new vertices at the solid grid points of the faces, new triangles
 * joined to the surface's rim vertices by their ids.  Integer atomics whose result does not depend on their order, exclusive sums
 * and IEEE double arithmetic with nothing fused decide everything: the result is an exact function of the input, two calls return
 * the same bytes.  tests/cap_oracle.py restates the steps below.
 *   samples          v = iso - F in MC33_real, the extractor's classification: a grid point is above when v has its sign bit
 *                    (F > iso), below when it has not, on when v == 0; a NaN sample is neither.
 *   solid            the side the surface's stored winding turns its back on.  The extractor winds a triangle so that its normal
 *                    by winding points where F falls and stores N on that side: above is solid in the plain libraries (the
 *                    reference's README sphere, whose inside is below, has volume < 0), below after mc33hip_set_normal_neg(c, 1) -
 *                    the _nneg flavours.  invert != 0 caps the other side - a dark object in a bright field: the second and third
 *                    index of every triangle of T are exchanged and the rows of N negated (their sign bits), in place, and the
 *                    steps below see that surface.  solid_above: 1 or 0, the side that was capped.
 *   faces            0 .. 5: x-lo, x-hi, y-lo, y-hi, z-lo, z-hi, outward normal the box's.  The plane of a face has the axes (u, w) =
 *                    (y, z), (x, z), (x, y); a face cell is the square (cu, cw) .. (cu + 1, cw + 1) of four neighbouring points;
 *                    "counterclockwise" is as seen from outside the box; the corners Q0 .. Q3 of a cell run counterclockwise from
 *                    its point with the smallest grid point index.
 *   1. face bits     per vertex and axis: g = ((double)V[v][a] - r0[a]) * (1.0 / d[a]), r = floor(g + 0.5), and g = r where |g - r| <=
 *                    tol[a] = min(2^-21 max(|r0[a]|, |r0[a] + N[a] d[a]|) / |d[a]|, 1/4): a vertex on grid plane k has the
 *                    coordinate (R)k * (R)d + (R)r0, rounded three times in MC33_real, which lies that close to k.  The vertex is
 *                    on face lo of the axis when g == lo[a], on face hi when g == hi[a].  nonfinite_vertices: the rows of V with a
 *                    coordinate that is not finite.
 *      sides         a valid triangle has its three indices below nV (invalid_triangles: the others, which contribute nothing).
 *                    Its sides e = T[e] -> T[(e + 1) % 3] with two different ends are counted per undirected pair.  A side used
 *                    once whose ends share no face bit is counted in off_face_edges and left alone - the rim of a hole, of a box
 *                    smaller than the surface.  Otherwise it is a rim segment a -> b of the lowest face the ends share
 *                    (rim_segments), unless its midpoint below lies outside the box: off_face_edges again.
 *   2. its cell      m = (g_a + g_b) * 0.5 on u and w with the snapped coordinates decides whether the midpoint lies in the box (lo
 *                    <= m <= hi on both axes); the cell is floor of the same midpoint of the coordinates as they were before the
 *                    snapping, clamped to lo .. hi - 1 - an end that was snapped onto a grid line must not carry the midpoint
 *                    over it.  The segments of a cell are ordered by i << 2 | e of the triangle i and side e that own them.
 *   3. regular       a cell none of whose four samples is on or a NaN, with the segments marching squares expects of its solid
 *                    corners: none for 0 or 4, one for 1, 2 adjacent or 3, two for 2 diagonal ones - and, with two, a decision
 *                    that step 4 can read.  Every other cell that has a solid corner or a segment is skipped (skipped_cells): no
 *                    triangle; the mesh stays edge-manifold and consistently wound and keeps boundary edges there.
 *   4. polygons      convex, fanned from the first entry: (p0, p1, p2), (p0, p2, p3) ...  One segment: [b, a, c1 .. ck], the
 *                    solid corners counterclockwise from the one whose clockwise neighbour is not solid.  Four solid corners:
 *                    [Q0, Q1, Q2, Q3].  Two segments, (a1, b1) before (a2, b2): corner c lies on the positive side of b -> a when
 *                    s = (g_a[u] - g_b[u]) * (c[w] - g_b[w]) - (g_a[w] - g_b[w]) * (c[u] - g_b[u]), negated on the faces x-lo,
 *                    y-hi, z-lo, is > 0.  When each segment has exactly one solid corner on its positive side, and not the
 *                    same: two triangles [b1, a1, cA], [b2, a2, cB].  When each has both solid corners there and exactly one
 *                    other corner Qj not there, and not the same: the hexagon [b1, a1, cA, b2, a2, cB] with c = Q(j + 1) mod 4.
 *                    The surface's own face-test decision is read off its segments, not made again.  Anything else: skipped.
 *                    capped_cells: the regular cells that have a polygon.
 *   5. new vertices  one per grid point that a polygon names, a point on a box edge or corner shared by the faces that meet
 *                    there; numbered from nV on in ascending order of the grid point index (z npy + y) npx + x.  V: (R)index *
 *                    (R)d[a] + (R)r0[a] per axis in MC33_real, what the vertex pass stores for t = 0.  N: n[a] = +1 / -1 / 0 where a
 *                    polygon of face hi / lo / no face of the axis names the point, (float)((double)n[a] / sqrt(n . n)), +0 where
 *                    n[a] == 0 - the sign the extractor's N has relative to its winding, in every flavour and with invert (which
 *                    exchanges both).  Attributes: by attr_mode[k], MC33HIP_CAP_WORD the word 0, MC33HIP_CAP_F32 the float NaN
 *                    0x7FC00000.  The rows below nV keep their bytes (invert apart).
 *   6. new triangles from nT on: by face, then by cell with u the faster index, then in polygon order.
 *   closed           1 when skipped_cells == 0, off_face_edges == 0 and every rim segment lies in a regular cell.
 *   MC33HIP_ERUNTIME   invalid triangles, in the words of the measuring calls; the outputs are complete without them.
 *   MC33HIP_ECAPACITY  capV < nV_out or capT < nT_out: every filled field is valid and nothing is written, invert included
 *                      (capV = capT = 0 is the size query; 2^32-1 rows are the most a mesh may have).
 *   MC33HIP_EINVAL     checked on the host, nothing is written: an inclined context; a z-slab context (plane0 != 0 or fewer
 *                      resident planes than the grid); no resident grid; a box with lo[a] >= hi[a] or hi[a] > N[a]; nV or nT
 *                      above 2^32-1; an isovalue that is a NaN; n_attr > 2 or a mode that is neither; a null pointer where a size
 *                      is not zero.
 *   An empty surface is legal: a box whose faces are all solid gets its whole shell, a box with nothing solid gets nothing.
 * Out of scope: cells with a sample equal to the isovalue (skipped and counted), caps at other planes, inclined grids.
 * The call enqueues on the context's stream behind whatever is on it, waits once, and brings the counts to the host.  Scratch, with
 * the context until mc33hip_destroy: 1 byte per vertex, 25 bytes per face cell and 8 per point of the box's surface, and the table
 * of sides: 16 bytes per slot, a power of two >= 4 nT slots.  A side with 2^24 uses would wrap the count in its word. */
#define MC33HIP_CAP_WORD 0
#define MC33HIP_CAP_F32 1
typedef struct {
	void *V, *N, *T;  unsigned long long nV, nT;         /* in and out (device): capV x 3 MC33_real, capV x 3 float, capT x 3 unsigned */
	unsigned long long capV, capT;
	double iso;                                          /* the isovalue of the extraction; used as MC33_real */
	unsigned lo[3], hi[3];                               /* the box, grid point indices: lo[a] < hi[a] <= N[a] */
	int invert;
	void *attr[2]; unsigned n_attr;                      /* in and out: <= 2 arrays of capV 4-byte words (device) */
	int attr_mode[2];                                    /* MC33HIP_CAP_WORD 0, MC33HIP_CAP_F32 1 */
	unsigned long long nV_out, nT_out, cap_vertices, cap_triangles, rim_segments, capped_cells, skipped_cells, off_face_edges,
	                   invalid_triangles, nonfinite_vertices;   /* filled */
	int solid_above, closed;                             /* filled */
} mc33hip_capping;
int mc33hip_cap_surface(mc33hip_ctx *c, mc33hip_capping *a);

/* --- draw a finished mesh on the device: a depth-tested, shaded image and an id buffer (no counterpart in the reference) ------------
 * V (nV x 3 MC33_real), N (nV x 3 float), T (nT x 3 unsigned, id base 0) in device memory, and C: nV colour words 0xAABBGGRR (NULL:
 * base_color for every vertex).  The call reads only these arrays: an inclined context and a z-slab context are accepted.  Outputs,
 * each a device array of width x height, row 0 at the top, each may be NULL (all NULL asks for the counts alone): oRGBA uint32
 * 0xAABBGGRR, oDepth float, oTri uint32 - the triangle under the pixel, 0xFFFFFFFF where nothing was drawn.  Everything below is
 * IEEE double arithmetic with nothing fused, or 64-bit integers; the depth test is an integer minimum and the counts are integer
 * sums: the result is an exact function of the input, two calls return the same bytes.  tests/render_oracle.py restates the steps.
 *   vertex       cx = ((m[0] x + m[1] y) + m[2] z) + m[3]; cy, cz, cw likewise from the next rows of m (row major: clip = m (x, y, z,
 *                1)).  Usable when all four are finite and cw > 0.  ix = cx / cw, iy = cy / cw, z = cz / cw; sx = (ix 0.5 + 0.5) width,
 *                sy = (0.5 - iy 0.5) height; X = floor(sx 256 + 0.5), Y likewise - 1/256 pixel.  Usable only if |X|, |Y| <= 2^23: that
 *                guard band is 8 x the largest viewport, and every edge function below stays under 2^49, exact in int64 and in double.
 *   triangle     in this order: invalid_triangles - an index >= nV; rejected - a corner is not usable (there is no near-plane clipping
 *                of geometry: MC33_calculate_clipped_isosurface cuts); area2 = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0); degenerate -
 *                area2 == 0; front-facing when area2 < 0 - for a matrix that does not mirror that is the side the stored N points to, in
 *                the plain and the _nneg flavours alike; culled - cull 1 and not front-facing, cull 2 and front-facing; offscreen - the
 *                bounding box of the corners holds no pixel centre of the viewport; drawn - all others.
 *   coverage     pixel (px, py) has its centre at P = (256 px + 128, 256 py + 128).  Edge A -> B in T's order (0 -> 1, 1 -> 2, 2 -> 0):
 *                dx = Bx - Ax, dy = By - Ay, E = dx (Py - Ay) - dy (Px - Ax), all three negated when area2 < 0.  The pixel is inside
 *                when for all three edges E > 0, or E == 0 and (dy < 0 or (dy == 0 and dx > 0)): a pixel centre on an edge two
 *                triangles share belongs to exactly one of them.
 *   depth        w_i = E of the edge opposite corner i (w0 of 1 -> 2, w1 of 2 -> 0, w2 of 0 -> 1); zf = (((double)w0 z0 + (double)w1
 *                z1) + (double)w2 z2) / (double)|area2|.  A fragment exists where the pixel is inside and 0 <= zf <= 1 - near and far
 *                clipping per pixel (fragments: their number).  zq = (uint32)floor(zf 4294967295.0 + 0.5), key = (uint64)zq << 32 |
 *                triangle index; the pixel keeps the minimum key: the nearest fragment, the lower index at equal zq.  covered: the
 *                pixels that hold a key.
 *   resolve      for a covered pixel and its triangle: b_i = (double)w_i / (double)|area2|, q_i = b_i / cw_i, s = (q0 + q1) + q2,
 *                L_i = q_i / s.  oDepth = (float)zf, oTri = the index.  n = ((L0 N0 + L1 N1) + L2 N2) per component, len = sqrt((nx nx +
 *                ny ny) + nz nz); l = light / |light| with |light| taken the same way, once, on the host; t = ((nx lx + ny ly) + nz
 *                lz) / len, |t| with two_sided, else t where t > 0 and 0 elsewhere; t = 0 where len is 0 or not finite.  shade =
 *                ambient + diffuse t.  For R, G, B (bits 0-7, 8-15, 16-23) with c_i the channel of corner i's word as double: x = shade
 *                ((L0 c0 + L1 c1) + L2 c2); x where x > 0, else 0 (a NaN gives 0); x where x < 255, else 255; floor(x + 0.5).  A = 255.
 *                An uncovered pixel gets background, +inf and 0xFFFFFFFF.
 *   MC33HIP_ERUNTIME   invalid triangles, in the words of the measuring calls; the outputs are complete without them.  Also when the
 *                      boxes of the triangles too large for one lane hold more than 2^32-1 screen tiles of 16 x 16 pixels (65 536
 *                      triangles that each fill a 4096 x 4096 viewport): the image is not complete then.
 *   MC33HIP_EINVAL     checked on the host, nothing is written: width or height 0 or above 4096; a matrix entry, a light component,
 *                      ambient or diffuse that is not finite; a light whose length is 0 (or overflows); a cull value outside 0 .. 2;
 *                      nV or nT above 2^32-1; a null V, N or T where its size is not zero.
 *   nT == 0 is legal and gives the background.
 * Out of scope: geometric near-plane clipping, transparency, anti-aliasing, shadows, textures, compositing several images by depth.
 * The call enqueues on the context's stream behind whatever is on it, waits once, and brings the counts to the host.  Scratch, with
 * the context until mc33hip_destroy: 8 bytes per pixel (the keys), a screen record of 24 bytes per vertex (X, Y, z, cw), and 8 bytes
 * per triangle for the list of the triangles too large for one lane and their work items.  MC33_HIP_RENDER_SMALL=<pixels>, read when
 * the context is created, is the largest box of pixel centres a single lane walks (default 16; 0: every triangle goes down the tiled
 * path); the bytes are the same in every setting. */
typedef struct {
	const void *V, *N, *T, *C;  unsigned long long nV, nT;   /* in (device): nV x 3 MC33_real, nV x 3 float, nT x 3 unsigned, nV words or NULL */
	double m[16];                                            /* row major: clip = m (x, y, z, 1) */
	unsigned width, height;                                  /* 1 .. 4096 */
	int cull, two_sided;                                     /* cull: 0 none, 1 back, 2 front */
	double light[3], ambient, diffuse;                       /* light: a direction in the coordinates of V */
	unsigned base_color, background;                         /* colour words 0xAABBGGRR */
	void *oRGBA, *oDepth, *oTri;                             /* out (device), each width x height or NULL */
	unsigned long long drawn, culled, degenerate, rejected, offscreen, invalid_triangles, fragments, covered;   /* filled */
} mc33hip_rendering;
int mc33hip_render_surface(mc33hip_ctx *c, mc33hip_rendering *a);
/* Developer timing: with MC33_HIP_TIMING >= 2 when the context is created, hipEvent times in ms of the stages of the last
 * mc33hip_render_surface call - clear, vertex pass, triangle pass, scan of the list, tiled pass, resolve; MC33HIP_EINVAL otherwise. */
int mc33hip_render_timing(mc33hip_ctx *c, float ms[6]);

/* --- distance between surfaces on the device: the nearest triangle per point (no counterpart in the reference) ---------------------
 * Query points P (nP x 3 MC33_real) and a target mesh V (nV x 3 MC33_real), T (nT x 3 unsigned, id base 0), all in device memory.
 * For every point the nearest point of the mesh: how far a simplified, smoothed or clipped surface has moved from the one it came
 * from, how thick the shell between two isovalues is, which triangle is nearest to a probe.  The call reads only these arrays: an
 * inclined context and a z-slab context are accepted.  Arithmetic is IEEE double, nothing fused; a dot product x . x' is
 * (x*x' + y*y') + z*z'.  The result is an exact function of the input - it does not depend on how the triangles are searched - and
 * two calls return the same bytes.  tests/distance_oracle.py restates the definition over all pairs.
 *   usable triangle   its three indices are below nV and its nine coordinates are finite.  A triangle with an index >= nV counts in
 *                     invalid_triangles and nothing outside V is read; a valid triangle with a coordinate that is not finite counts
 *                     in nonfinite_triangles - a statistic, not an error.  Neither kind takes part in the search.
 *   q_i(p)            the closest point of usable triangle i with corners a, b, c (rows of V as doubles): the region walk of Ericson,
 *                     Real-Time Collision Detection 5.1.5, in this order and with these comparisons:
 *                       ab = b-a; ac = c-a; ap = p-a; d1 = ab.ap; d2 = ac.ap;
 *                           if (d1 <= 0 && d2 <= 0) q = a;
 *                       else bp = p-b; d3 = ab.bp; d4 = ac.bp;
 *                           if (d3 >= 0 && d4 <= d3) q = b;
 *                       else vc = d1*d4 - d3*d2;
 *                           if (vc <= 0 && d1 >= 0 && d3 <= 0) { v = d1/(d1-d3); q = a + v*ab; }
 *                       else cp = p-c; d5 = ab.cp; d6 = ac.cp;
 *                           if (d6 >= 0 && d5 <= d6) q = c;
 *                       else vb = d5*d2 - d1*d6;
 *                           if (vb <= 0 && d2 >= 0 && d6 <= 0) { w = d2/(d2-d6); q = a + w*ac; }
 *                       else va = d3*d6 - d5*d4;
 *                           if (va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0) { w = (d4-d3)/((d4-d3)+(d5-d6)); q = b + w*(c-b); }
 *                       else { den = 1.0/((va+vb)+vc); v = vb*den; w = vc*den; q = (a + ab*v) + ac*w; }
 *                     then per axis, with lo / hi the smallest / largest of the three corners (lo = a; if (b < lo) lo = b; if (c < lo)
 *                     lo = c; hi likewise with >):  if (!(q >= lo)) q = lo;  if (!(q <= hi)) q = hi;
 *                     The clamp is part of the definition.  It does nothing on a sane triangle; on a sliver whose den is garbage q
 *                     still lies in the triangle's box and is never NaN, which is what the search's pruning rests on.
 *   D2_i              e = p - q;  D2_i = (e.x*e.x + e.y*e.y) + e.z*e.z.
 *   winner for p      triangle i beats the best so far when D2_i < best, or D2_i == best and i < best_i: the smallest D2 over all
 *                     usable triangles, ties to the smallest index.  A NaN or infinite D2 never wins; a point with a coordinate that
 *                     is not finite has no winner, and neither has any point when no triangle is usable.
 *   oDist[p]          (float)sqrt(D2); with signed_distance != 0 negated when e . (ab x ac) < 0 for the winning triangle, the cross
 *                     product taken component-wise as y*z' - z*y' etc.  Near an edge or a corner of the mesh the sign is only as good
 *                     as the winning triangle's plane: it is the side of THAT plane p lies on, not an inside / outside test.
 *   oTri[p]           the winner's index;   oPoint[p] (3 MC33_real): the winner's q, converted.
 *                     Without a winner: +inf, 0xFFFFFFFF and three quiet NaN (0x7FC00000 / 0x7FF8000000000000); the point counts in
 *                     unmatched_points.  Each of the three pointers may be NULL.
 *   filled            over matched points only: matched_points, unmatched_points; max and min - sqrt of the largest / smallest
 *                     winning D2, unsigned even with signed_distance; argmax and argmin - the smallest point index that attains
 *                     them; sum (of sqrt(D2)) and sum_sq (of D2), accumulated in double in a fixed order without floating-point
 *                     atomics: two calls on one context return the same bits.  All six are 0 when no point is matched.
 *                     lattice[3] and triangle_tests: the cells per axis the search used and the point-triangle evaluations it made -
 *                     implementation statistics, outside the definition.
 *   MC33HIP_ERUNTIME   invalid triangles: the count is in mc33hip_last_error, in the words of the measuring calls; the outputs are
 *                      complete without them.
 *   MC33HIP_EINVAL     checked on the host, nothing is written: a null P, V or T where its size is not zero; nP, nV or nT above
 *                      2^32-1; an output byte range (nP rows) that meets an input range or another output range.
 *   MC33HIP_ENOMEM     the scratch cannot be had.
 *   nP == 0 or nT == 0 is success; in the latter case every point is unmatched.
 * The search is a uniform lattice over the box of the usable triangles, made anew by every call: a list of triangles per cell, and
 * per point shells of cells of growing radius until a lower bound on everything not yet visited exceeds the point's best (DESIGN.md
 * 25).  The call enqueues on the context's stream behind whatever is on it, waits for the box and for the size of the lists, and a
 * last time for the summary.  Scratch, with the context until mc33hip_destroy: 8 bytes per lattice cell (at most 256 cells per axis),
 * 4 bytes per list entry, 8 bytes per point.  MC33_HIP_DISTANCE_CELLS=<n>, read when the context is created, forces n cells on every
 * axis of the lattice (within the library's own limits; 1: every point tests every triangle); the bytes are the same in every
 * setting.
 * Out of scope: distance fields on the grid, a lattice kept between calls, samples inside the query mesh's triangles. */
typedef struct {
	const void *P;  unsigned long long nP;                   /* in (device): nP x 3 MC33_real */
	const void *V, *T;  unsigned long long nV, nT;           /* in (device): nV x 3 MC33_real, nT x 3 unsigned, id base 0 */
	int signed_distance;
	float *oDist;  unsigned *oTri;  void *oPoint;            /* out (device), nP rows each, or NULL */
	unsigned long long matched_points, unmatched_points, invalid_triangles, nonfinite_triangles;   /* filled */
	double max, min, sum, sum_sq;
	unsigned long long argmax, argmin;
	unsigned lattice[3];
	unsigned long long triangle_tests;
} mc33hip_distance;
int mc33hip_surface_distance(mc33hip_ctx *c, mc33hip_distance *a);
/* Developer timing: with MC33_HIP_TIMING >= 2 when the context is created, hipEvent times in ms of the passes of the last
 * mc33hip_surface_distance call - build (box, count, scan, fill), query, reduce; MC33HIP_EINVAL otherwise. */
int mc33hip_distance_timing(mc33hip_ctx *c, float ms[3]);

/* --- curvature of the implicit surface at the vertices, from the grid's second differences (no counterpart in the reference) ------
 * Mean, Gaussian and principal curvatures of the surface F = iso at nV vertices dV (nV x 3 MC33_real in device memory, what
 * mc33hip_emit wrote, or any points), taken from the gradient g and the Hessian H of the RESIDENT grid - the curvature of the field's
 * level set through the vertex, which is where N comes from too; nothing is taken from the triangles.  Orthogonal grids only.
 * Everything in IEEE double, nothing fused, only + - * / and sqrt: the outputs are an exact function of the inputs.
 *   grid        N[a] cells, points 0 .. N[a], spacing d[a], origin r0[a] (the doubles of the descriptor), N[a] >= 2 on every axis;
 *               S(i, j, k) the resident sample converted to double.
 *   per node    for node index n along axis a, the other two indices the node's own:
 *                 p = min(n + 1, N[a]);  m = max(n - 1, 0);  c = min(max(n, 1), N[a] - 1)
 *                 g_a  = (S(p) - S(m)) / ((double)(p - m) * d[a])
 *                 H_aa = ((S(c + 1) - S(c)) - (S(c) - S(c - 1))) / (d[a] * d[a])
 *               (on a grid face the second difference is taken about the nearest interior point), and for a < b
 *                 H_ab = ((S(pa, pb) - S(pa, mb)) - (S(ma, pb) - S(ma, mb))) / (((double)(pa - ma) * d[a]) * ((double)(pb - mb) * d[b]))
 *   per vertex  1. g[a], i[a], f[a] of mc33hip_sample_property, word for word: the clamps, f = 0 where i == N, a NaN coordinate.
 *               2. each of gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz of the nodes i + {0, 1} is interpolated with that definition's
 *                  lerp along x, then y, then z; a node with f == 0 on its axis is not evaluated and its samples are not read.
 *               3. g2 = (gx*gx + gy*gy) + gz*gz;  gl = sqrt(g2);  tr = (hxx + hyy) + hzz
 *               4. gHg = (((gx*gx)*hxx + (gy*gy)*hyy) + (gz*gz)*hzz) + 2.0 * ((((gx*gy)*hxy) + ((gx*gz)*hxz)) + ((gy*gz)*hyz))
 *               5. mean = sign * ((gHg - g2*tr) / ((2.0*g2) * gl))
 *               6. axx = hyy*hzz - hyz*hyz;  ayy = hxx*hzz - hxz*hxz;  azz = hxx*hyy - hxy*hxy
 *                  axy = hxz*hyz - hxy*hzz;  axz = hxy*hyz - hxz*hyy;  ayz = hxy*hxz - hxx*hyz
 *               7. gAg = step 4 with a.. in place of h..;  gauss = gAg / (g2*g2)
 *               8. disc = mean*mean - gauss;  r = sqrt(disc < 0 ? 0 : disc);  k1 = mean + r;  k2 = mean - r
 *               9. oMean, oGauss, oK1, oK2 [v] = those doubles rounded to float.
 *               Nothing is special-cased: a vanishing gradient gives 0/0 = NaN, NaN and infinite samples propagate.
 *   sign        +1 or -1.  With +1 a blob of HIGH samples is convex and has mean > 0 - seen from the side the plain libraries' N
 *               points to; the MC33_NORMAL_NEG flavours of the C API pass -1.
 *   outputs     device arrays of nV floats; each may be NULL, all NULL asks for the summary alone.
 *   summary     lo[q], hi[q], q = mean, gauss, k1, k2: minimum and maximum of the FINITE floats of output q as doubles, +inf / -inf
 *               when it has none; finite: the vertices whose four floats are all finite; undefined = nV - finite.  Taken with
 *               integer atomics on ordered keys: two calls return the same bytes.
 * The grid may be the library's copy or an adopted buffer at any pitch, slice and alignment; only grid points are read.  The call
 * enqueues on the context's stream behind whatever is on it, waits, and brings the summary to the host; nV == 0 succeeds and
 * touches nothing.  MC33HIP_EINVAL, checked on the host, nothing is written: no resident grid; a z-slab context (plane0 != 0 or
 * npz_resident != nz_total + 1); an inclined context; an axis with fewer than 2 cells; a sign other than +-1; dV == NULL with
 * nV > 0.  Scratch, with the context until mc33hip_destroy: 40 bytes. */
typedef struct {
	const void *dV;  unsigned long long nV;  int sign;   /* in */
	float *oMean, *oGauss, *oK1, *oK2;                   /* out (device), each nV floats or NULL */
	double lo[4], hi[4];                                 /* filled: mean, gauss, k1, k2 */
	unsigned long long finite, undefined;                /* filled */
} mc33hip_curvature;
int mc33hip_curvature_vertices(mc33hip_ctx *c, mc33hip_curvature *a);
/* The colour step of mc33hip_color_vertices over any nV floats dP in device memory - what mc33hip_sample_property or
 * mc33hip_curvature_vertices left: dC[v] = palette[(int)floor(s * (n - 1) + 0.5)], s = ((double)dP[v] - lo) / (hi - lo) clamped to
 * [0, 1], nan_color where dP[v] is NaN.  For the floats of mc33hip_sample_property these are the words mc33hip_color_vertices
 * gives.  Only enqueues on the context's stream; needs no property grid and takes an inclined context.  MC33HIP_EINVAL: a null
 * pointer where the size is not zero, a NULL palette, n outside 2..256, lo >= hi or a NaN bound. */
int mc33hip_color_values(mc33hip_ctx *c, const float *dP, unsigned long long nV, const int *palette, unsigned int n, double lo,
                         double hi, int nan_color, int *dC);

/* Plain device allocations on the context's device (for language bindings). */
int mc33hip_device_alloc(mc33hip_ctx *c, void **dptr, size_t bytes);
int mc33hip_device_free(mc33hip_ctx *c, void *dptr);

#ifdef __cplusplus
}
#endif
#endif
