// mc33_context.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, in order; not a header to include elsewhere):
// host side, part 1: errors, the context (mc33hip_ctx), environment switches, create / destroy, grid upload.

static thread_local char g_err[512] = "";
static void set_err(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	if (getenv("MC33_HIP_VERBOSE")) fprintf(stderr, "[mc33hip] %s\n", g_err);
}
#define HIP_TRY(expr)                                                                         \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if (e_ != hipSuccess) {                                                               \
			set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return e_ == hipErrorOutOfMemory ? MC33HIP_ENOMEM : MC33HIP_ERUNTIME;             \
		}                                                                                     \
	} while (0)

// Growable device arrays: plain pointer and capacity fields (the context is calloc'ed and free'd); dev_release is how one is
// released, dev_room / dev_room_all how it is made to hold at least n elements.  The caller adds its slack to n and names the
// bytes; a caller with something to do when an array is new looks at the capacity first.  What an array held is not kept.
//   success: *cap >= n, every array there;   failure: every array nullptr, *cap = 0, set_err called, the code HIP_TRY returns.
// dev_room_all is all or nothing for arrays that share one capacity: they are released together and allocated in the order
// given (where a buffer lands moves the emit kernels, DESIGN.md 7.1: the order of the allocations is part of the behaviour).
struct DevArray { void **p; uint64_t bytes; };
template <typename E>
static DevArray dev_array(E **p, uint64_t n, uint64_t elem_bytes = sizeof(E)) { return DevArray{(void **)p, n * elem_bytes}; }
template <typename E>
static void dev_release(E **p) { (void)hipFree(*p); *p = nullptr; }
static int dev_room_all(const char *what, uint64_t *cap, uint64_t n, std::initializer_list<DevArray> arrays) {
	bool there = *cap >= n;
	for (const DevArray &a : arrays) there = there && *a.p;
	if (there) return 0;
	for (const DevArray &a : arrays) dev_release(a.p);
	*cap = 0;
	for (const DevArray &a : arrays) {
		const hipError_t e = hipMalloc(a.p, a.bytes);
		if (e == hipSuccess) continue;
		for (const DevArray &b : arrays) dev_release(b.p);
		set_err("%s (%llu elements) failed: %s", what, (unsigned long long)n, hipGetErrorString(e));
		return e == hipErrorOutOfMemory ? MC33HIP_ENOMEM : MC33HIP_ERUNTIME;
	}
	*cap = n;
	return 0;
}
template <typename E>
static int dev_room(const char *what, E **p, uint64_t *cap, uint64_t n, uint64_t elem_bytes = sizeof(E)) {
	return dev_room_all(what, cap, n, {dev_array(p, n, elem_bytes)});
}

// Per-isovalue output of the sweep (SweepLane) and its bookkeeping on the host
constexpr int MC33_LANES = 8;
constexpr int MC33_MANY_PASSES = 4;  // passes of one mc33hip_sweep_many call: 8 isovalues = 4 + 4, 7 = 4 + 2 + 1
struct IsoLane {
	SliceHeader *slice_hdr;   // one record per (wave tile, cell slice) of the sweep
	uint4 *slice_bits;
	uint32_t *slice_compact;
	uint8_t *plane_fmt;
	unsigned long long *slot_part;
	uint4 *edge_bits, *edge_hdr;
	uint64_t slice_cap, edge_cap;
	uint32_t epoch;           // extractions since the slice headers were last cleared
	// a sweep made ahead of time by mc33hip_sweep_many, waiting for the count / extract call of its isovalue
	bool swept, boundary_done;
	bool tail_pending;        // a sweep has added this lane's slices into slot_part and no tail (k_slots) has consumed them yet
	bool tail_done;           // ... and the tail (k_slots ... k_scan_apply) of that sweep has been enqueued too, into the lane's own
	                          // TailSet: the count / extract call finds record ranges, records and prefix sums made
	double iso;
	mc33hip_range range;
	uint32_t pack;            // samples per lane and load of the sweep that filled it (lane_of_column)
	PlanRef plan;             // the plan (slot of mc33hip_ctx::plan, target, weight) that sweep went by: its edge records are indexed by that plan's tiles
	int many_pass, many_ni;   // which pass of mc33hip_sweep_many filled it (its events), and how many isovalues that pass classified
};

// A block plan of k_sweep (plan_sweep): the tiles, and the pairs of tiles that meet in z.  What a sweep leaves for k_boundary is indexed
// by the tiles of the plan it went by, so a lane keeps a PlanRef (IsoLane::plan) until its tail is made.
struct SweepPlan {
	SweepTile *d_tiles;
	TileBoundary *d_bounds;   // (made to measure for every plan: nbounds is its capacity)
	uint64_t tiles_cap, ntiles, nbounds;
	PlanKey key;              // what names it (mc33_sweep_plan.h); ze == 0: not a plan
};

// Everything a tail (k_slots ... k_scan_apply) writes and the emit passes read, for ONE isovalue.  Lane k of the sweep buffers
// works with set k.  A single extraction uses lane 0 and set 0; an iso sweep (mc33hip_sweep_many) fills the sets of all its
// isovalues right behind each pass over the grid - one launch of every tail kernel for the up to four isovalues of the pass
// (PerLane) - and the count / extract calls that follow only emit (round 4; until then the one set was shared and every
// isovalue ran its nine tail launches by itself: 72 launches per 8-isovalue step, now 18).
struct TailSet {
	uint32_t *seg_cnt;
	SegDir *seg_dir;
	SegBase *seg_base;
	uint64_t seg_cap;
	uint64_t *bsV, *bsT;
	uint64_t bs_cap;
	EntryA *entries_a;
	EntryB *entries_b;
	EntryC *entries_c;
	uint32_t *entry_seg, *slow_list, *dirty_list;
	uint64_t entry_cap;
	BatchDesc *batches;       // the records in batches of <= 64 of one slice slot (k_cells writes, the emit passes walk)
	uint64_t batch_cap;
	uint32_t *list_cnt;       // [2][LIST_CHUNKS] cursors of the slow / dirty list parts (ListChunks)
	ListChunks lc;            // ... for the range last counted
	uint2 *slot_base;
	uint64_t slot_base_cap;
	uint32_t *live_list;      // [slot_base_cap]: slots with cut cells, k_slots -> k_cells
	uint32_t tail_serial;     // tails enqueued (seg_tagged)
	bool tail_incomplete;     // a tail was begun and did not reach its last launch: Counters::live_cursor may not be zero
	uint32_t records_hint;    // work records of the last extraction whose counters were read (grid of the triangle pass, first guess of a new set)
	uint32_t slow_hint;       // ... and its slow records + 1 (0: not known yet): the grid of k_emit_slow
	bool count_known, count_needed;  // ... and whether it had records waiting for k_slow_count (corners equal to the isovalue): see enqueue_tail
	bool alias_known;         // ... and whether it had slow cells at all (Counters::alias_cells; alias_last: how many)
	uint32_t alias_last;
	bool alias_gated;         // the last tail into this set left the slow kernels out (enqueue_tail): its counts and surface stand only if it had no slow cells
	uint32_t seq;             // the sequence word of the last extraction that returned at its counts (counters_seq(h_ctr): wait_counters)
	Counters *d_ctr, *h_ctr;
	bool ctr_published;       // the emit pass enqueued last leaves the counters in h_ctr itself (k_emit_fast_triangles)
};

// The environment switches (tuning knobs, the tests that force a code path, developer tracing), read ONCE when a context is created: a getenv walks
// the whole environment, and there were some twenty of them on every call.  0 / -1 / nullptr = not set: the library decides.
struct Switches {
	uint32_t rz, sweep_blocks_per_cu, min_depth, cells_blocks, slow_blocks, emit_blocks, emit_v_blocks_per_cu, slow_slots_max;
	bool no_pack, no_stage, verbose;
	int slow_count, no_fork, slow_slots, tri_first;  // -1: not set
	char *trace_cells, *trace_file;                               // (developer tracing: file names; copies)
	uint32_t debug, cells_dev;  // (looked at by -DMC33_DEV builds only)
	uint32_t rz_table;          // MC33_HIP_RZ_TABLE: depth of the plan a sweep with a range table goes by (plan_sweep)
	int live;                   // MC33_HIP_LIVE: 1 / 0 = a sweep with a table always / never goes by a live list; -1 (not set): sweep_live decides
	uint32_t table_tiles;       // MC33_HIP_TABLE_TILES: the tile count plan 1 is asked for, whatever the sweeps find (the tests, the curve of profiles/r10_sweep_pack.txt)
	uint32_t list_lds;          // MC33_HIP_LIST_LDS: plans of up to this many blocks keep the places of their quads in LDS (k_live_compact; 4096, the most; the tests set 0)
	uint32_t render_small;      // MC33_HIP_RENDER_SMALL: the largest box of pixel centres one lane of k_render_triangles walks (mc33_render.hip.h; the tests set 0 and a huge value)
	uint32_t distance_cells;    // MC33_HIP_DISTANCE_CELLS: cells per axis of the lattice of mc33hip_surface_distance, 0: it decides (mc33_distance.hip.h; the tests set 1 and a huge value;
	                            //  the word was padding: with the context 24 bytes smaller, the C3 emit stage measured 4 us slower)
	uint32_t emit_v_blocks;     // MC33_HIP_EMIT_V_BLOCKS: blocks of k_emit_vertices, whatever the device holds (the tests: fewer waves than batches, so that a wave walks several)
};

struct mc33hip_ctx {
	mc33hip_grid_desc desc;
	Switches sw;
	int device;
	hipStream_t stream;
	bool own_stream;          // the stream came from the pool (mc33hip_own_stream) and goes back there
	bool stream_given;        // the caller named the stream (mc33hip_set_stream): its work is ordered by it, and mc33hip_extract may return at the counts
	sample_t *d_grid;
	bool owns_grid;
	size_t pitch, slice;  // in samples
	uint16_t *d_lut;
	uint32_t *d_rules;
	uint8_t *d_rule_index;
	uint4 *d_fast;
	EntryB *d_fast_b;
	uint32_t *d_pat;
	uint64_t *d_pat_order;  // build_pattern_order
	IsoLane lanes[MC33_LANES]; // what a sweep leaves behind, per isovalue (lane 0: the single-isovalue calls)
	TailSet ts[MC33_LANES];    // ... and what its tail leaves behind (set k belongs to lane k)
	TailSet *w;                // the set of the lane the last count used: what emit and the counters refer to
	uint32_t cells_blocks;   // blocks of k_cells the GPU holds at once
	uint32_t epoch_wrap;      // the stamps start over at this count (2^30; MC33_HIP_EPOCH_WRAP for the test that crosses it)
	IsoLane *cur_lane;        // the lane the last count used (its epoch is what the emit pass needs)
	bool lane_presweeped;     // ... and it had been filled by mc33hip_sweep_many
	bool lane_pretailed;      // ... tail included
	SweepPlan plan[3];        // the plans of k_sweep for the current range (plan_sweep): [0] without a range table, [1] with one, [2] with one and sized (table_retarget)
	int cur_plan;             // ... and the one in force: what the sweep to be launched, or the lane whose tail is being made, goes by
	uint32_t resident_blocks; // k_sweep blocks the device holds at once
	uint8_t *d_verdict;       // with a table: k_tile_verdicts' byte per block of the plan, and the live list k_live_compact makes of
	uint32_t *d_live;         // them (the count, then a word per block with a live tile: mc33hip_sweep_live) - of the last sweep with a table
	uint32_t *d_packed;       // ... and the packed list k_sweep_live goes by (SweepArgs::live; k_live_compact for the layout)
	uint64_t verdict_cap, live_cap, packed_cap;
	uint64_t live_blocks;     // blocks of the plan that sweep went by (0: no such sweep yet)
	unsigned long long *h_live;  // pinned: what k_live_compact published last (live tiles << 32 | tiles << 1 | plan; 0: nothing yet)
	TablePolicy table;        // which plan the sweeps with a table go by, at what size, and which of them get a list (mc33_sweep_plan.h)
	// the range table (RangeEntry, sweep_ranges): made for a grid whose samples this library knows to be unchanged - its own copy,
	// or an adopted buffer the caller has declared stable - by the second sweep since they last changed
	RangeEntry *d_ranges;
	uint64_t ranges_cap;
	bool ranges_valid;        // the table holds the ranges of the samples as they are
	bool ranges_off;          // MC33_HIP_RANGES=0: never made (read at create)
	bool grid_stable;         // mc33hip_grid_stable(c, 1) since the buffer was adopted
	uint32_t sweeps_seen;     // sweeps since the samples last changed, while there is no table
	uint32_t *d_skipped;      // mc33hip_sweep_skipped: SweepArgs::skipped of the last single-isovalue sweep at timing level >= 1
	uint64_t skipped_tiles;   // ... its tiles (0: no such sweep yet)
	// the block table (k_ranges: RANGE_BLOCKS entries per strip), made with the range table, in the same launch, and good exactly as
	// long as it is (ranges_valid); and the verdict word per strip of the last sweep that left blocks out (k_block_verdicts)
	RangeEntry *d_blocks;
	unsigned long long *d_blockw;
	uint64_t blocks_cap, blockw_cap;
	bool blocks_made;         // the last k_ranges wrote the block table too
	bool blocks_off;          // MC33_HIP_BLOCKS=0: no block table, no block left out (read at create)
	bool blocks_always;       // MC33_HIP_BLOCKS=1: blocks are left out wherever a sweep goes by a list; not set: where it pays (launch_sweep_zm)
	double plane_weight;      // the weight of a plane the sized plans of sweeps that leave blocks out are cut with (sweep_plane_weight; MC33_HIP_PLANE_WEIGHT, read at create, for curves: 0 none)
	int cus;                  // compute units of the device
	int emit_v_blocks_per_cu; // blocks of k_emit_vertices a CU holds
	hipEvent_t ev[4];
	hipEvent_t ev_many[MC33_MANY_PASSES][3];  // mc33hip_sweep_many's passes: recorded before the sweep, behind it, behind the tails made ahead; read in read_timing (nobody waits)
	hipStream_t aux, aux2;    // the triangle pass and the slow-record pass run beside the vertex pass
	hipStream_t copy;         // mc33hip_download_concurrent
	hipEvent_t ev_fork, ev_join, ev_join2;
	unsigned long long *d_bases;  // {id base, output vertex row, output triangle row} made on the device (mc33hip_bases_from_table)
	bool async_count;         // the last count was enqueued without waiting for its counters (mc33hip_count_async)
	bool count_unused;        // the last mc33hip_count has not served an emit yet: a count of the same isovalue and range may reuse it
	bool alias_gate;          // the call under way reads the counters before it returns and repeats its tail on a miss: the tail may leave the
	                          // slow kernels out (enqueue_tail)
	hipEvent_t ev_dl[2];      // mc33hip_emit_download: behind the pass that completes T / behind the one that completes V and N
	bool emit_pending;        // an emit was enqueued after the last timing read
	uint32_t emit_queued;     // extractions that returned when their counts were known, their emit passes still queued or running ...
	uint32_t emit_finished;   // ... and up to which of them the stream has been waited for since (finish_pending_emit)
	int timing_level;         // MC33_HIP_TIMING: 0 none (default), 1 whole call, 2 per pass - the event records cost ~20 us per call
	bool inclined, triangular;   // non-orthogonal grid (MC33_spnC): _GRD._A / _GRD.A_ as given
	bool normal_neg;             // front and back exchanged (the reference's MC33_NORMAL_NEG compile-time switch)
	double grd_A[9], grd_Ai[9];
	unsigned long long *trace;  // developer tracing (MC33_HIP_TRACE_FILE)
	uint64_t trace_waves;
	unsigned long long *trace_cells;  // (MC33_HIP_TRACE_CELLS)
	uint64_t trace_cells_n;
	// state of the last count
	bool counted;
	Params P;
	mc33hip_range range;
	uint64_t nsegs, ghost_segs;
	mc33hip_counts counts;
	mc33hip_timing timing;
	// the property grid (mc33_property.hip.h): a second scalar field sampled at the vertices; its plane window is its own
	sample_t *d_prop;
	bool prop_owned;          // the library's pitched copy (mc33hip_property_upload*), not a caller's buffer
	bool prop_pending;        // a sampling kernel was enqueued since the violation word was last looked at (prop_check)
	size_t prop_pitch, prop_slice, prop_cap;  // in samples
	unsigned prop_plane0, prop_nplanes;
	uint32_t *d_prop_pal;     // the palette of the colour kernel enqueued last
	unsigned long long *d_prop_viol, *h_prop_viol;  // vertices that needed a plane outside the window: device word, pinned copy
	hipEvent_t ev_prop;       // mc33hip_download_enqueue
	struct MeasureState *meas;  // scratch of the measuring passes (mc33_measure.hip.h), made by the first of them
	// the launch shape of the emit enqueued last (mc33hip_emit_shape): the set it read, the grids of the vertex, triangle and slow
	// passes as launched, the slow kernel (0 a thread per record, 1 a lane per slot, 2 left out: alias-gated), the triangle pass first
	TailSet *shape_set;       // (nullptr: no emit yet)
	uint32_t shape[5];
};
static void prop_destroy(mc33hip_ctx *c);
static void meas_destroy(mc33hip_ctx *c);
static int prop_check(mc33hip_ctx *c);

extern "C" const char *mc33hip_last_error(void) { return g_err; }
static uint32_t env_u32(const char *name, uint32_t dflt);
static uint32_t render_small_switch();
static uint32_t distance_cells_switch();
static double plane_weight_switch();

static int env_flag(const char *name) {  // -1: not set
	const char *s = getenv(name);
	return s && *s ? (atoi(s) != 0 ? 1 : 0) : -1;
}
static void read_switches(Switches &w) {
	w.rz = env_u32("MC33_HIP_RZ", 0); w.sweep_blocks_per_cu = env_u32("MC33_HIP_SWEEP_BLOCKS_PER_CU", 0); w.min_depth = env_u32("MC33_HIP_MIN_DEPTH", 0); w.rz_table = env_u32("MC33_HIP_RZ_TABLE", 0); w.live = env_flag("MC33_HIP_LIVE"); w.table_tiles = env_u32("MC33_HIP_TABLE_TILES", 0); w.list_lds = std::min(4096u, env_u32("MC33_HIP_LIST_LDS", 4096u));
	w.cells_blocks = env_u32("MC33_HIP_CELLS_BLOCKS", 0); w.slow_blocks = env_u32("MC33_HIP_SLOW_BLOCKS", 0); w.emit_blocks = (env_u32("MC33_HIP_EMIT_BLOCKS", 0) + 7u) & ~7u;  // (whole rounds of the 8 XCDs: XcdWalk)
	w.emit_v_blocks = (env_u32("MC33_HIP_EMIT_V_BLOCKS", 0) + 7u) & ~7u; w.emit_v_blocks_per_cu = env_u32("MC33_HIP_EMIT_V_BLOCKS_PER_CU", 0); w.slow_slots_max = env_u32("MC33_HIP_SLOW_SLOTS_MAX", 0);
	w.no_pack = env_u32("MC33_HIP_NO_PACK", 0) != 0; w.no_stage = env_u32("MC33_HIP_NO_STAGE", 0) != 0; w.verbose = getenv("MC33_HIP_VERBOSE") != nullptr;
	w.slow_count = env_flag("MC33_HIP_SLOW_COUNT"); w.no_fork = env_flag("MC33_HIP_NO_FORK");
	w.slow_slots = env_flag("MC33_HIP_SLOW_SLOTS"); w.tri_first = env_flag("MC33_HIP_TRI_FIRST");
	w.trace_cells = getenv("MC33_HIP_TRACE_CELLS") ? strdup(getenv("MC33_HIP_TRACE_CELLS")) : nullptr;
	w.trace_file = getenv("MC33_HIP_TRACE_FILE") ? strdup(getenv("MC33_HIP_TRACE_FILE")) : nullptr;
	w.render_small = render_small_switch();
	w.distance_cells = distance_cells_switch();
	w.debug = env_u32("MC33_HIP_DEBUG", 0); w.cells_dev = env_u32("MC33_HIP_CELLS_DEV", 0);
}
static void forget_ranges(mc33hip_ctx *c) {  // the samples changed, or may have: no table until the second sweep from now
	c->ranges_valid = false;
	c->blocks_made = false;
	c->sweeps_seen = 0;
	table_forget(c->table);
	if (c->h_live) __atomic_store_n(c->h_live, 0ull, __ATOMIC_RELAXED);
}

// An extraction on a caller's stream returns when its counts are known (count_until_fits), with its emit passes still queued or
// running.  Whatever is ordered by that stream needs nothing: the next extraction, a caller's kernels and copies.  Everything else
// waits here first: what reads the outputs by another road (the copy stream), what frees or regrows buffers the passes use, what
// changes the stream, what reads events.  Every entry point comes through use_device, which is where most of them get it.
// (Two counters, not a flag: mc33hip_download_concurrent / mc33hip_download_many may come from another thread than the context's.
// A thread notes how many extractions had returned early when it came, waits for the stream - which covers all of them, their
// passes were enqueued before they were counted - and only then records that number as finished, never lowering it: a thread
// that arrives while another is still waiting waits too, and an extraction that returns meanwhile stays pending.)
static bool emit_pending_now(const mc33hip_ctx *c) {
	return __atomic_load_n(&c->emit_finished, __ATOMIC_ACQUIRE) != __atomic_load_n(&c->emit_queued, __ATOMIC_ACQUIRE);
}
static int finish_pending_emit(mc33hip_ctx *c) {
	const uint32_t upto = __atomic_load_n(&c->emit_queued, __ATOMIC_ACQUIRE);
	if (__atomic_load_n(&c->emit_finished, __ATOMIC_ACQUIRE) == upto) return 0;
	HIP_TRY(hipStreamSynchronize(c->stream));
	uint32_t seen = __atomic_load_n(&c->emit_finished, __ATOMIC_RELAXED);
	while ((int32_t)(upto - seen) > 0 && !__atomic_compare_exchange_n(&c->emit_finished, &seen, upto, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) {}
	return 0;
}
// keep_emit: the call is the next extraction over the same range on the same stream - nothing of the host's is in the passes' way
static int use_device(mc33hip_ctx *c, bool keep_emit = false) {
	HIP_TRY(hipSetDevice(c->device));
	return keep_emit ? 0 : finish_pending_emit(c);
}

// Side streams are taken from a process-wide pool and handed back, never destroyed: hipStreamDestroy of a stream
// that events were recorded on leaves the HIP runtime (ROCm 7.x) with a dangling reference - its reference count
// is decremented after the stream object has been freed, which corrupts whatever the heap put there next
// (found with tools/uaf_trap.c under tools/soak.py: thousands of create_MC33 / free_MC33 pairs in one process).
namespace {
struct StreamPool {
	std::mutex m;
	std::vector<std::pair<int, hipStream_t>> idle;
};
StreamPool &stream_pool() {
	static StreamPool *p = new StreamPool;  // never destructed: no ordering problem with the runtime's own teardown
	return *p;
}
hipError_t pool_take(int device, hipStream_t *out) {
	StreamPool &sp = stream_pool();
	{
		std::lock_guard<std::mutex> g(sp.m);
		for (size_t k = 0; k < sp.idle.size(); k++)
			if (sp.idle[k].first == device) {
				*out = sp.idle[k].second;
				sp.idle[k] = sp.idle.back();
				sp.idle.pop_back();
				return hipSuccess;
			}
	}
	return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void pool_give(int device, hipStream_t s) {
	if (!s) return;
	(void)hipStreamSynchronize(s);
	StreamPool &sp = stream_pool();
	std::lock_guard<std::mutex> g(sp.m);
	sp.idle.emplace_back(device, s);
}
}  // namespace

// row pitch (samples) of the library's own copy of the grid: every row starts on a 16-byte boundary, whatever the sample
// type (the sweep loads dwords, k_emit_vertices stages 16-byte chunks of the rows)
static size_t own_pitch(size_t npx) {
	const size_t unit = sizeof(sample_t) >= 4 ? 4 : 16 / sizeof(sample_t);
	return (npx + unit - 1) / unit * unit;
}

static void free_set(TailSet &w) {  // (everything of the set; it can be filled again by ensure_set)
	dev_release(&w.seg_cnt); dev_release(&w.seg_dir); dev_release(&w.seg_base); dev_release(&w.bsV);
	dev_release(&w.entries_a); dev_release(&w.entries_b); dev_release(&w.entries_c); dev_release(&w.entry_seg); dev_release(&w.slow_list); dev_release(&w.dirty_list);
	dev_release(&w.batches); dev_release(&w.list_cnt); dev_release(&w.slot_base); dev_release(&w.live_list); dev_release(&w.d_ctr);
	if (w.h_ctr) (void)hipHostFree(w.h_ctr);
	w = TailSet{};
}

extern "C" int mc33hip_create(mc33hip_ctx **out, const mc33hip_grid_desc *d) {
	if (!out || !d) return MC33HIP_EINVAL;
	*out = nullptr;
	if (d->sample_bytes != MC33_SAMPLE_BYTES) { set_err("sample_bytes %d does not match this library (%d)", d->sample_bytes, MC33_SAMPLE_BYTES); return MC33HIP_EINVAL; }
	if (d->npx < 2 || d->npy < 2 || d->npz_resident < 2 || d->nz_total < 1) { set_err("grid needs at least 2 points per axis"); return MC33HIP_EINVAL; }
	if ((uint64_t)d->plane0 + d->npz_resident > (uint64_t)d->nz_total + 1) { set_err("resident planes exceed the grid"); return MC33HIP_EINVAL; }
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device available"); return MC33HIP_ENOGPU; }
	mc33hip_ctx *c = (mc33hip_ctx *)calloc(1, sizeof *c);
	if (!c) return MC33HIP_ENOMEM;
	c->desc = *d;
	read_switches(c->sw);
	if (d->device >= 0) c->device = d->device;
	else if (hipGetDevice(&c->device) != hipSuccess) { free(c); set_err("hipGetDevice failed"); return MC33HIP_ENOGPU; }
	*out = c;
	int rc = use_device(c);
	if (rc) { free(c); *out = nullptr; return rc; }
	c->pitch = own_pitch(d->npx);
	c->slice = c->pitch * d->npy;
	hipError_t e;
#define CREATE_TRY(expr)                                                                    \
	if ((e = (expr)) != hipSuccess) {                                                       \
		set_err("%s failed: %s", #expr, hipGetErrorString(e));                              \
		mc33hip_destroy(c);                                                                 \
		*out = nullptr;                                                                     \
		return e == hipErrorOutOfMemory ? MC33HIP_ENOMEM : MC33HIP_ERUNTIME;                \
	}
	CREATE_TRY(hipMalloc(&c->d_lut, sizeof mc33_lut));
	CREATE_TRY(hipMalloc(&c->d_rules, sizeof mc33_rule_words));
	CREATE_TRY(hipMalloc(&c->d_rule_index, sizeof mc33_rule_index));
	CREATE_TRY(hipMemcpy(c->d_lut, mc33_lut, sizeof mc33_lut, hipMemcpyHostToDevice));
	CREATE_TRY(hipMemcpy(c->d_rules, mc33_rule_words, sizeof mc33_rule_words, hipMemcpyHostToDevice));
	CREATE_TRY(hipMemcpy(c->d_rule_index, mc33_rule_index, sizeof mc33_rule_index, hipMemcpyHostToDevice));
	{
		uint32_t fast[256];
		uint4 rec[256];
		build_fast_table(mc33_lut, fast);
		fast_record_table(fast, rec);
		CREATE_TRY(hipMalloc(&c->d_fast, sizeof rec));
		CREATE_TRY(hipMemcpy(c->d_fast, rec, sizeof rec, hipMemcpyHostToDevice));
		EntryB fb[256];
		fast_b_table(fast, fb);
		CREATE_TRY(hipMalloc(&c->d_fast_b, sizeof fb));
		CREATE_TRY(hipMemcpy(c->d_fast_b, fb, sizeof fb, hipMemcpyHostToDevice));
		constexpr uint32_t lut_n = sizeof mc33_lut / sizeof mc33_lut[0];
		uint32_t pat[lut_n];
		build_pattern_info(mc33_lut, lut_n, pat);
		CREATE_TRY(hipMalloc(&c->d_pat, sizeof pat));
		CREATE_TRY(hipMemcpy(c->d_pat, pat, sizeof pat, hipMemcpyHostToDevice));
		uint64_t order[lut_n];
		build_pattern_order(mc33_lut, lut_n, order);
		CREATE_TRY(hipMalloc(&c->d_pat_order, sizeof order));
		CREATE_TRY(hipMemcpy(c->d_pat_order, order, sizeof order, hipMemcpyHostToDevice));
	}
	c->w = &c->ts[0];  // (the sets get their memory when a range is known: ensure_set)
	for (int k = 0; k < 4; k++) CREATE_TRY(hipEventCreate(&c->ev[k]));
	for (int k = 0; k < MC33_MANY_PASSES; k++)
		for (int j = 0; j < 3; j++) CREATE_TRY(hipEventCreate(&c->ev_many[k][j]));
	CREATE_TRY(pool_take(c->device, &c->aux));
	CREATE_TRY(pool_take(c->device, &c->aux2));
	CREATE_TRY(pool_take(c->device, &c->copy));
	c->timing_level = getenv("MC33_HIP_TIMING") ? atoi(getenv("MC33_HIP_TIMING")) : 0;
	c->epoch_wrap = std::min(1u << 30, std::max(3u, env_u32("MC33_HIP_EPOCH_WRAP", 1u << 30)));
	c->ranges_off = env_flag("MC33_HIP_RANGES") == 0;
	c->blocks_off = env_flag("MC33_HIP_BLOCKS") == 0;
	c->blocks_always = env_flag("MC33_HIP_BLOCKS") == 1;
	c->plane_weight = plane_weight_switch();
	CREATE_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
	CREATE_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
	CREATE_TRY(hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
	for (int k = 0; k < 2; k++) CREATE_TRY(hipEventCreateWithFlags(&c->ev_dl[k], hipEventDisableTiming));
#undef CREATE_TRY
	return MC33HIP_OK;
}

extern "C" void mc33hip_destroy(mc33hip_ctx *c) {
	if (!c) return;
	(void)hipSetDevice(c->device);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	else (void)hipDeviceSynchronize();
	if (c->owns_grid) dev_release(&c->d_grid);
	prop_destroy(c);
	meas_destroy(c);
	dev_release(&c->d_lut); dev_release(&c->d_rules); dev_release(&c->d_rule_index); dev_release(&c->d_fast);
	dev_release(&c->d_fast_b); dev_release(&c->d_pat); dev_release(&c->d_pat_order);
	for (int k = 0; k < MC33_LANES; k++) free_set(c->ts[k]);
	for (int k = 0; k < MC33_LANES; k++) {
		IsoLane &L = c->lanes[k];
		dev_release(&L.slice_hdr); dev_release(&L.slice_bits); dev_release(&L.slice_compact); dev_release(&L.plane_fmt); dev_release(&L.slot_part); dev_release(&L.edge_bits); dev_release(&L.edge_hdr);
	}
	for (SweepPlan &pl : c->plan) { dev_release(&pl.d_tiles); dev_release(&pl.d_bounds); }
	dev_release(&c->d_verdict); dev_release(&c->d_live); dev_release(&c->d_packed);
	if (c->h_live) (void)hipHostFree(c->h_live);
	c->h_live = nullptr;
	dev_release(&c->d_ranges); dev_release(&c->d_skipped); dev_release(&c->d_blocks); dev_release(&c->d_blockw);
	dev_release(&c->d_bases);
	dev_release(&c->trace); dev_release(&c->trace_cells);
	if (c->aux) (void)hipStreamSynchronize(c->aux);
	if (c->aux2) (void)hipStreamSynchronize(c->aux2);
	if (c->copy) (void)hipStreamSynchronize(c->copy);
	for (int k = 0; k < 4; k++) if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
	for (int k = 0; k < MC33_MANY_PASSES; k++)
		for (int j = 0; j < 3; j++) if (c->ev_many[k][j]) (void)hipEventDestroy(c->ev_many[k][j]);
	if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
	if (c->ev_join) (void)hipEventDestroy(c->ev_join);
	if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
	for (int k = 0; k < 2; k++) if (c->ev_dl[k]) (void)hipEventDestroy(c->ev_dl[k]);
	pool_give(c->device, c->aux); pool_give(c->device, c->aux2); pool_give(c->device, c->copy);  // after the events
	if (c->own_stream) pool_give(c->device, c->stream);
	free(c->sw.trace_cells); free(c->sw.trace_file);
	free(c);
}

static void forget_sweeps(mc33hip_ctx *c) {  // the grid changed: sweeps made ahead of time are worthless
	for (int k = 0; k < MC33_LANES; k++) { c->lanes[k].swept = false; c->lanes[k].tail_done = false; }
	forget_ranges(c);  // (every upload and mc33hip_adopt_device come through here)
}

// Who may keep a table over which samples (include/mc33_hip.h): the library's own copy is written by the uploads alone, which drop
// the table; an adopted buffer is the caller's, and only the caller can say that it stays as it is.
extern "C" int mc33hip_grid_stable(mc33hip_ctx *c, int stable) {
	if (!c) return MC33HIP_EINVAL;
	c->grid_stable = stable != 0;
	if (!c->grid_stable && !c->owns_grid) forget_ranges(c);
	return MC33HIP_OK;
}
extern "C" int mc33hip_grid_changed(mc33hip_ctx *c) {
	if (!c) return MC33HIP_EINVAL;
	c->counted = false;
	forget_sweeps(c);
	return MC33HIP_OK;
}

extern "C" int mc33hip_set_stream(mc33hip_ctx *c, void *s) {
	if (!c) return MC33HIP_EINVAL;
	if (int rc = use_device(c)) return rc;  // (what the old stream still holds is finished on the old stream)
	if (c->own_stream) { pool_give(c->device, c->stream); c->own_stream = false; }
	c->stream = (hipStream_t)s;
	forget_ranges(c);  // (the new stream is not ordered behind the old one, on which the table may still be in the making)
	c->stream_given = true;
	return MC33HIP_OK;
}

extern "C" int mc33hip_own_stream(mc33hip_ctx *c) {
	if (!c) return MC33HIP_EINVAL;
	if (c->own_stream) return MC33HIP_OK;
	int rc = use_device(c);
	if (rc) return rc;
	hipStream_t st = nullptr;
	HIP_TRY(pool_take(c->device, &st));
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	c->stream = st;
	forget_ranges(c);
	c->own_stream = true;
	c->stream_given = false;
	return MC33HIP_OK;
}

extern "C" int mc33hip_device_count(void) {
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

static int ensure_grid(mc33hip_ctx *c) {
	if (c->d_grid && c->owns_grid) return 0;
	if (c->d_grid && !c->owns_grid) { c->d_grid = nullptr; }
	c->pitch = own_pitch(c->desc.npx);
	c->slice = c->pitch * c->desc.npy;
	// +64 samples of slack: tile loads clamp their addresses into the row, never past the buffer
	HIP_TRY(hipMalloc(&c->d_grid, (c->slice * c->desc.npz_resident + 64) * sizeof(sample_t)));
	c->owns_grid = true;
	return 0;
}

// Rows packed into the pitched device layout through pinned staging buffers, one group of planes at a time.  row(k, j): host
// address of row j of resident plane k.  What it costs is the packing - a memcpy per row, a million scattered 4 KiB rows for a
// 1024^3 float grid made by alloc_F (every row an allocation of its own: what generate_grid_from_fn and the reference's file
// readers make, MC33_util_grd.c:147-169): 240 ms on one core, whether or not the copies over the link (77 ms) run beside it - so
// large grids are packed by up to four threads, each with two buffers of its own in turn (a group is packed while the thread's
// group before it goes over the link) and every fourth group of planes: profiles/r05_upload_rows.txt.
// dst / npz / pitch: the pitched device copy that is filled - the sample grid's own, or the property grid's (mc33_property.hip.h).
template <typename RowFn>
static int upload_staged(mc33hip_ctx *c, RowFn row, sample_t *dst, uint32_t npz, size_t pitch) {
	const uint32_t npy = c->desc.npy;
	const size_t rowb = (size_t)c->desc.npx * sizeof(sample_t);
	const size_t planeb = pitch * npy * sizeof(sample_t);
	size_t planes_per = (16u << 20) / planeb;
	if (planes_per < 1) planes_per = 1;
	if (planes_per > npz) planes_per = npz;
	const uint32_t ngroups = (uint32_t)((npz + planes_per - 1) / planes_per);
	const unsigned hw = std::thread::hardware_concurrency();
	const unsigned nthreads = (uint64_t)planeb * npz < (256ull << 20) ? 1u : std::min(std::min(4u, std::max(1u, hw / 2u)), ngroups);
	HIP_TRY(hipStreamSynchronize(c->stream));  // (nothing enqueued earlier may still be reading the grid: the copies run on a stream of their own)
	std::vector<hipError_t> err(nthreads, hipSuccess);
	auto worker = [&](unsigned t) {
		hipError_t e = hipSetDevice(c->device);
		char *stage[2] = {nullptr, nullptr};
		hipEvent_t done[2] = {nullptr, nullptr};
		const bool two = ngroups > nthreads;  // (a thread with one group needs one buffer)
		if (e == hipSuccess) e = hipHostMalloc(&stage[0], planes_per * planeb, hipHostMallocDefault);
		if (e == hipSuccess && two) e = hipHostMalloc(&stage[1], planes_per * planeb, hipHostMallocDefault);
		for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipEventCreateWithFlags(&done[b], hipEventDisableTiming);
		uint32_t turn = 0;
		for (uint32_t g = t; g < ngroups && e == hipSuccess; g += nthreads, turn++) {
			const uint32_t b = two ? (turn & 1u) : 0u, k0 = g * (uint32_t)planes_per;
			const uint32_t kn = (uint32_t)((k0 + planes_per <= npz) ? planes_per : npz - k0);
			if (turn >= (two ? 2u : 1u) && (e = hipEventSynchronize(done[b])) != hipSuccess) break;  // (the buffer's last copy has left it)
			for (uint32_t k = 0; k < kn; k++)
				for (uint32_t j = 0; j < npy; j++)
					memcpy(stage[b] + k * planeb + (size_t)j * pitch * sizeof(sample_t), row(k0 + k, j), rowb);
			if ((e = hipMemcpyAsync((char *)dst + (size_t)k0 * planeb, stage[b], (size_t)kn * planeb, hipMemcpyHostToDevice, c->copy)) == hipSuccess)
				e = hipEventRecord(done[b], c->copy);
		}
		for (int b = 0; b < 2; b++) {  // (its own copies done before its buffers go)
			if (done[b]) { if (e == hipSuccess && turn > (uint32_t)b) e = hipEventSynchronize(done[b]); (void)hipEventDestroy(done[b]); }
		}
		if (e != hipSuccess) (void)hipStreamSynchronize(c->copy);
		for (int b = 0; b < 2; b++)
			if (stage[b]) (void)hipHostFree(stage[b]);
		err[t] = e;
	};
	std::vector<std::thread> th;
	std::vector<unsigned> inline_share;  // (a thread that could not be started: its groups on this thread)
	for (unsigned t = 1; t < nthreads; t++) {
		try { th.emplace_back(worker, t); } catch (...) { inline_share.push_back(t); }
	}
	worker(0u);
	for (unsigned t : inline_share) worker(t);
	for (auto &x : th) x.join();
	(void)hipSetDevice(c->device);
	HIP_TRY(hipStreamSynchronize(c->copy));
	for (unsigned t = 0; t < nthreads; t++)
		if (err[t] != hipSuccess) { set_err("grid upload failed: %s", hipGetErrorString(err[t])); return err[t] == hipErrorOutOfMemory ? MC33HIP_ENOMEM : MC33HIP_ERUNTIME; }
	return MC33HIP_OK;
}

extern "C" int mc33hip_upload_contiguous(mc33hip_ctx *c, const void *host) {
	if (!c || !host) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = ensure_grid(c))) return rc;
	const size_t rowb = (size_t)c->desc.npx * sizeof(sample_t);
	if (c->pitch != c->desc.npx && rowb % 4 != 0) {
		// rows that are not a whole number of dwords (odd-length uchar / ushort rows): the runtime's pitched copy from
		// pageable memory falls to 0.1-0.3 GB/s (3 s for a 0.8 GB grid); packing the rows ourselves runs at memcpy speed
		const char *h = (const char *)host;
		const size_t npy = c->desc.npy;
		if ((rc = upload_staged(c, [=](uint32_t k, uint32_t j) { return h + ((size_t)k * npy + j) * rowb; }, c->d_grid, c->desc.npz_resident, c->pitch))) return rc;
	} else
		HIP_TRY(hipMemcpy2D(c->d_grid, c->pitch * sizeof(sample_t), host, rowb, rowb, (size_t)c->desc.npy * c->desc.npz_resident,
		                    hipMemcpyHostToDevice));
	c->counted = false;
	forget_sweeps(c);
	return MC33HIP_OK;
}

extern "C" int mc33hip_upload_rows(mc33hip_ctx *c, const void *const *const *F) {
	if (!c || !F) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = ensure_grid(c))) return rc;
	const uint32_t npy = c->desc.npy, npz = c->desc.npz_resident;
	const size_t rowb = (size_t)c->desc.npx * sizeof(sample_t);
	// fast path: rows laid out back to back (grid_from_data_pointer, reference MC33_util_grd.c:609-611)
	bool contiguous = true;
	const char *expect = (const char *)F[0][0];
	for (uint32_t k = 0; k < npz && contiguous; k++)
		for (uint32_t j = 0; j < npy; j++, expect += rowb)
			if ((const char *)F[k][j] != expect) { contiguous = false; break; }
	if (contiguous) return mc33hip_upload_contiguous(c, F[0][0]);
	// rows are separate allocations (alloc_F, reference MC33_util_grd.c:147-169)
	if ((rc = upload_staged(c, [=](uint32_t k, uint32_t j) { return (const char *)F[k][j]; }, c->d_grid, c->desc.npz_resident, c->pitch))) return rc;
	c->counted = false;
	forget_sweeps(c);
	return MC33HIP_OK;
}

extern "C" int mc33hip_adopt_device(mc33hip_ctx *c, const void *dptr, size_t pitch, size_t slice) {
	if (!c || !dptr || pitch < c->desc.npx || slice < pitch * c->desc.npy || pitch > 0xFFFFFFFFull) return MC33HIP_EINVAL;
	// (k_sweep addresses the 64 sample rows of a tile with 32-bit byte offsets from the tile's first row)
	if ((uint64_t)pitch * sizeof(sample_t) * 64u > 0xFFFFFFFFull) {
		set_err("pitch of %llu samples: the 64 rows of a tile (%llu bytes) do not fit 32-bit offsets", (unsigned long long)pitch,
		        (unsigned long long)pitch * sizeof(sample_t) * 64u);
		return MC33HIP_EINVAL;
	}
	int rc = use_device(c);
	if (rc) return rc;
	if (c->owns_grid) dev_release(&c->d_grid);
	c->d_grid = (sample_t *)dptr;
	c->owns_grid = false;
	c->grid_stable = false;  // (volatile until the caller says otherwise: mc33hip_grid_stable)
	c->pitch = pitch;
	c->slice = slice;
	c->plan[0].key.ze = c->plan[1].key.ze = c->plan[2].key.ze = 0u;  // (the plan counts its work in batches of the form - packed or not - this buffer's alignment allows)
	c->counted = false;
	forget_sweeps(c);
	return MC33HIP_OK;
}
