// mc33_extract.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, in order; not a header to include elsewhere):
// host side, part 2: planning and enqueueing the passes, the C ABI entry points of include/mc33_hip.h.

static int check_range(mc33hip_ctx *c, const mc33hip_range *r) {
	const mc33hip_grid_desc &d = c->desc;
	if (!r || r->z_begin >= r->z_end || r->z_end > d.nz_total) { set_err("bad z range"); return MC33HIP_EINVAL; }
	if (r->ghost_below && r->z_begin == 0) { set_err("ghost slice below z = 0"); return MC33HIP_EINVAL; }
	const uint32_t zs = r->z_begin - (r->ghost_below ? 1u : 0u);
	// planes the passes touch: cells need planes z and z+1; normals read z+2 (MC:888, 1036, 1182, 1217)
	// when it exists, and z-1 for vertices on grid points (MC:643-647, 836, 909, 980, 1058)
	const uint32_t lo = zs ? zs - 1 : 0, hi = (r->z_end + 1 <= d.nz_total) ? r->z_end + 1 : d.nz_total;
	if (lo < d.plane0 || hi > d.plane0 + d.npz_resident - 1) {
		set_err("range needs planes %u..%u, resident are %u..%u", lo, hi, d.plane0, d.plane0 + d.npz_resident - 1);
		return MC33HIP_EINVAL;
	}
	if (!c->d_grid) { set_err("no grid uploaded"); return MC33HIP_EINVAL; }
	return 0;
}

static void fill_params(mc33hip_ctx *c, double iso, const mc33hip_range *r) {
	const mc33hip_grid_desc &d = c->desc;
	Params &P = c->P;
	P.nx = d.npx - 1; P.ny = d.npy - 1; P.nz = d.nz_total;
	P.nseg = (P.nx + SEG_CELLS - 1) / SEG_CELLS;
	P.zs = r->z_begin - (r->ghost_below ? 1u : 0u);
	P.iso = (real_t)iso;
	// store selection and float copies: MC:1772-1782
	if (d.d[0] != d.d[1] || d.d[1] != d.d[2]) { P.store_mode = 2; P.ca = (real_t)(d.d[2] / d.d[0]); P.cb = (real_t)(d.d[2] / d.d[1]); }
	else { P.store_mode = (d.d[0] == 1 && d.r0[0] == 0 && d.r0[1] == 0 && d.r0[2] == 0) ? 0 : 1; P.ca = P.cb = 1.0f; }
	P.triangular = 0;
	P.normal_neg = c->normal_neg ? 1 : 0;
	P.negzero_iso = (P.iso == 0 && sign_of(P.iso)) ? 1 : 0;
	for (int k = 0; k < 9; k++) P.A[k] = P.Ai[k] = 0.0;
	if (c->inclined) {  // G->nonortho: MC:1763-1770
		P.store_mode = 3;
		P.triangular = c->triangular;
		for (int j = 0; j < 3; j++)
			for (int i = 0; i < 3; i++) {
				P.A[3 * j + i] = c->grd_A[3 * j + i] * d.d[i];
				P.Ai[3 * j + i] = c->grd_Ai[3 * j + i] / d.d[j];
			}
	}
	for (int k = 0; k < 3; k++) { P.O[k] = (real_t)d.r0[k]; P.D[k] = (real_t)d.d[k]; }
	c->range = *r;
	c->nsegs = (uint64_t)(r->z_end - P.zs) * P.ny * P.nseg;
	c->ghost_segs = r->ghost_below ? (uint64_t)P.ny * P.nseg : 0;
}

static uint32_t env_u32(const char *name, uint32_t dflt) {
	const char *s = getenv(name);
	if (!s || !*s) return dflt;
	long v = strtol(s, nullptr, 10);
	return v > 0 ? (uint32_t)v : dflt;
}

// the record arrays of a set, all or nothing: a set with some of its arrays would pass for a complete one (ensure_set looks at entries_a)
static int alloc_entries(TailSet &w, uint64_t cap) {
	if (cap > 0xFFFFFF00ull) cap = 0xFFFFFF00ull;
	return dev_room_all("work-record buffers", &w.entry_cap, cap,
	                    {dev_array(&w.entries_a, cap + 2),  // (+ 2: the triangle pass reads records in pairs)
	                     dev_array(&w.entries_b, cap),      // (touched for tested and slow records only)
	                     dev_array(&w.entries_c, cap),      // (... for slow records only)
	                     dev_array(&w.entry_seg, cap), dev_array(&w.slow_list, cap), dev_array(&w.dirty_list, cap)});
}

// the buffers of set w for the current range (c->nsegs, c->P, c->range); hint: work records to make room for at first (0: a guess from the range)
static int ensure_set(mc33hip_ctx *c, TailSet &w, uint64_t hint = 0) {
	if (!w.d_ctr) {
		HIP_TRY(hipMalloc(&w.d_ctr, sizeof(Counters)));
		HIP_TRY(hipMemset(w.d_ctr, 0, sizeof(Counters)));  // (live_cursor: every tail leaves it zero for the next)
		HIP_TRY(hipMalloc(&w.list_cnt, 2 * LIST_CHUNKS * sizeof(uint32_t)));
		HIP_TRY(hipHostMalloc(&w.h_ctr, COUNTERS_HOST_BYTES, hipHostMallocDefault));  // (counters, then the sequence word: counters_seq)
		memset(w.h_ctr, 0, COUNTERS_HOST_BYTES);
		w.seq = 0;
	}
	if (w.seg_cap < c->nsegs) {
		if (int rc = dev_room_all("row-segment arrays", &w.seg_cap, c->nsegs,
		                          {dev_array(&w.seg_cnt, c->nsegs), dev_array(&w.seg_dir, c->nsegs),
		                           dev_array(&w.seg_base, c->nsegs + 1)}))  // (+ 1: the triangle pass reads bases in pairs)
			return rc;
		w.tail_serial = 0;  // (the first tail clears the new seg_cnt)
	}
	const uint64_t nb = (c->nsegs + SCAN_CHUNK - 1) / SCAN_CHUNK;
	if (w.bs_cap < nb) {
		w.bsT = nullptr;
		if (int rc = dev_room_all("scan sums", &w.bs_cap, nb, {dev_array(&w.bsV, 2 * (nb + scan_groups(nb)))})) return rc;  // chunk sums V, T; then group sums V, T
		w.bsT = w.bsV + nb;
	}
	if (!w.entries_a || !w.entry_cap) {
		// first guess: one cell in 32 is cut (BASELINE fields: 0.4-6 % of the cells); grown on demand
		const uint64_t cells = (uint64_t)c->P.nx * c->P.ny * (c->range.z_end - c->P.zs);
		return alloc_entries(w, hint ? hint + hint / 4 + 65536 : cells / 32 + 65536);
	}
	return 0;
}
static int ensure_workspaces(mc33hip_ctx *c) { return ensure_set(c, c->ts[0]); }

static int grow_entries(TailSet &w, uint64_t need) {
	const uint64_t cap = need + need / 8 + 65536;
	if (cap > 0xFFFFFF00ull) { set_err("more than 2^32 work records"); return MC33HIP_EOVERFLOW; }
	return alloc_entries(w, cap);
}

// The plans of k_sweep: what they are, what names them and how their tiles are made is mc33_sweep_plan.h; here the context's
// share - the batch of its samples, the weight its sized plans are cut with, and putting a plan in force on the device.
static bool sweep_packed(const mc33hip_ctx *c);
static PlanGrid plan_grid(const mc33hip_ctx *c) { return PlanGrid{c->P.ny, c->P.nseg, sweep_packed(c) ? 4u * (uint32_t)SWEEP_PACK : 4u}; }
static double plane_weight_switch() {  // MC33_HIP_PLANE_WEIGHT, read when a context is created: for curves and tests; 0: plans are cut by batches alone
	const char *s = getenv("MC33_HIP_PLANE_WEIGHT");
	if (!s || !*s) return PLANE_WEIGHT_BLOCKS;
	const double v = atof(s);
	return v > 0.0 && v <= 1024.0 ? v : 0.0;
}
static double sweep_plane_weight(const mc33hip_ctx *c) {
	if (!MC33_BLOCK_SKIP || c->blocks_off || !(c->blocks_always || c->P.nseg >= 4u)) return 0.0;
	return c->plane_weight;
}
// Puts the plan for [zs, ze) in force (c->cur_plan), making it when its slot holds another.  table: the plan of a sweep with a range
// table, sized to `target` tiles cut with `weight` (plan_slot), or without.  This runs in every count call: nothing is allocated
// while the slot holds the plan.
static int plan_sweep(mc33hip_ctx *c, uint32_t zs, uint32_t ze, bool table, uint32_t target = 0u, double weight = 0.0) {
	const PlanSlot ps = plan_slot(table, zs, ze, target, weight, c->sw.rz, c->sw.rz_table);
	SweepPlan &pl = c->plan[ps.slot];
	c->cur_plan = ps.slot;
	if (pl.d_tiles && pl.key == ps.key) return 0;
	if (!c->resident_blocks) {
		int per_cu = 0, cus = 0;
		HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep<1, 1>, 256, 0));
		HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
		const uint32_t want = c->sw.sweep_blocks_per_cu ? c->sw.sweep_blocks_per_cu : 4u;
		c->resident_blocks = (uint32_t)std::max(1, cus) * (uint32_t)std::max(1, std::min(per_cu, (int)want));
	}
	std::vector<SweepTile> tiles; std::vector<TileBoundary> bounds;
	uint64_t total = 0;
	if (!plan_tiles(plan_grid(c), ps.key, c->resident_blocks, c->sw.min_depth, tiles, bounds, total)) { set_err("grid too large for one launch"); return MC33HIP_EINVAL; }
	// A sweep made ahead by mc33hip_sweep_many may still be reading the old plan: the copies below go through the null stream,
	// which a non-blocking stream (any torch.cuda.Stream) is not ordered with
	HIP_TRY(hipStreamSynchronize(c->stream));
	pl.key.ze = 0u;  // (not a plan until both arrays are in place)
	if (pl.tiles_cap < tiles.size())
		if (int rc = dev_room("sweep tiles", &pl.d_tiles, &pl.tiles_cap, tiles.size())) return rc;
	HIP_TRY(hipMemcpy(pl.d_tiles, tiles.data(), tiles.size() * sizeof(SweepTile), hipMemcpyHostToDevice));
	pl.ntiles = tiles.size();
	dev_release(&pl.d_bounds);  // (made to measure for every plan: nbounds is its capacity)
	pl.nbounds = 0;
	if (!bounds.empty()) {
		if (int rc = dev_room("tile boundaries", &pl.d_bounds, &pl.nbounds, bounds.size())) return rc;
		HIP_TRY(hipMemcpy(pl.d_bounds, bounds.data(), bounds.size() * sizeof(TileBoundary), hipMemcpyHostToDevice));
	}
	pl.key = ps.key;
	if (const uint64_t columns = c->sw.verbose ? (uint64_t)plan_y_tiles(plan_grid(c)) * c->P.nseg : 0u)
		fprintf(stderr, "[mc33hip] sweep plan %d: %llu wave tiles (%u resident, %u asked for, plane weight %.2f), %llu columns, depth %.1f\n", ps.slot, (unsigned long long)pl.ntiles,
		        c->resident_blocks * 4, ps.key.target, ps.key.weight, (unsigned long long)columns, (double)(ze - zs) * columns / (double)pl.ntiles);
	return 0;
}

// slot geometry of the range being classified
struct SlotGeom {
	uint32_t nYT, nseg;
	SlotDims sd;
	uint64_t cell_blocks, nslots, nchunks;
};
static int slot_geometry(mc33hip_ctx *c, SlotGeom &g) {
	const Params &P = c->P;
	g.nYT = (P.ny + 62) / 63;
	g.nseg = P.nseg;  // (the slots of a slice group are its real row segments)
	g.sd = SlotDims{(c->range.z_end - P.zs + 1 + 3) / 4, g.nYT, g.nseg};  // the plane above the last slice has a slot too
	g.cell_blocks = (uint64_t)g.sd.nZG * g.nYT * g.nseg;
	if (g.cell_blocks > 0x3FFFFFFFull) { set_err("grid too large for one launch"); return MC33HIP_EINVAL; }
	g.nslots = g.cell_blocks * 4;
	g.nchunks = 0;
	return 0;
}

// buffers of one isovalue lane for the current range and the tile plan in force; a new extraction number (epoch)
static int begin_lane(mc33hip_ctx *c, IsoLane &L, const SlotGeom &g, hipStream_t st) {
	if (L.slice_cap < g.nslots) {
		const uint64_t part_bytes = ((g.nslots + SLOT_CHUNK - 1) / SLOT_CHUNK) * 8;
		if (int rc = dev_room_all("slice buffers", &L.slice_cap, g.nslots,
		                          {dev_array(&L.slice_hdr, g.nslots), dev_array(&L.slice_bits, g.nslots, 2048),  // (slots of planes: SlotDims)
		                           dev_array(&L.slice_compact, g.nslots, 256), dev_array(&L.plane_fmt, g.nslots),
		                           dev_array(&L.slot_part, 2, part_bytes)}))  // two halves, used by alternate extractions
			return rc;
		L.slice_cap = 0;  // (not this lane's until they are clean: a failure below has them made again)
		HIP_TRY(hipMemsetAsync(L.slice_hdr, 0, g.nslots * sizeof(SliceHeader), st));
		HIP_TRY(hipMemsetAsync(L.slot_part, 0, 2 * part_bytes, st));
		L.epoch = 0;
		L.tail_pending = false;
		L.slice_cap = g.nslots;
	}
	const uint64_t ntiles = c->plan[c->cur_plan].ntiles;  // (the buffers follow the larger plan: they only grow)
	if (L.edge_cap < ntiles)
		if (int rc = dev_room_all("tile edge buffers", &L.edge_cap, ntiles,
		                          {dev_array(&L.edge_bits, ntiles, 2 * 128 * sizeof(uint4)), dev_array(&L.edge_hdr, ntiles, 2 * 2 * sizeof(uint4))}))
			return rc;
	L.plan = PlanRef{c->cur_plan, c->plan[c->cur_plan].key.target, c->plan[c->cur_plan].key.weight};
	const uint64_t nchunks = (L.slice_cap + SLOT_CHUNK - 1) / SLOT_CHUNK;  // (capacity: the halves keep their place)
	if (++L.epoch >= c->epoch_wrap) {  // stamps wrap: start over with clean headers AND clean partial sums - the call before
		// accumulated into the half an odd epoch selects and cleared only the other one, and epoch 1 is odd again
		HIP_TRY(hipMemsetAsync(L.slice_hdr, 0, L.slice_cap * sizeof(SliceHeader), st));
		HIP_TRY(hipMemsetAsync(L.slot_part, 0, 2 * nchunks * 8, st));
		L.epoch = 1;
	}
	if (L.tail_pending) {
		// The sweep before this one added its slices into the half its epoch selected, and no k_slots ever consumed them and
		// cleared the other half for this epoch (a sweep made ahead by mc33hip_sweep_many whose isovalue was never asked for,
		// the grid was re-uploaded, a call failed in between): the half this epoch accumulates into still holds the sums of
		// two extractions ago.  Start from clean sums.
		HIP_TRY(hipMemsetAsync(L.slot_part, 0, 2 * nchunks * 8, st));
		L.tail_pending = false;
	}
	L.swept = false;
	L.tail_done = false;
	L.boundary_done = false;
	return 0;
}
static unsigned long long *lane_part(const IsoLane &L, bool next) {
	const uint64_t nchunks = (L.slice_cap + SLOT_CHUNK - 1) / SLOT_CHUNK;
	return L.slot_part + ((L.epoch + (next ? 1u : 0u)) & 1u) * nchunks;
}

// Kernel arguments that come from the context: the resident grid, the reference's tables, and the arrays of a TailSet under the
// names the argument structs share - rec: CellsArgs, SlowArgs or EmitCtx; lists: CellsArgs, SlowArgs or EmitArgs (w.lc first)
static GridView<sample_t> grid_view(const mc33hip_ctx *c) { return GridView<sample_t>{c->d_grid, (uint32_t)c->pitch, c->desc.plane0, c->slice}; }
static Tables tables(const mc33hip_ctx *c) { return Tables{c->d_lut, c->d_rules, c->d_rule_index}; }
template <typename Rec, typename Lists>
static void set_arrays(const TailSet &w, Rec &rec, Lists &lists) {
	rec.entries_a = w.entries_a; rec.entries_b = w.entries_b; rec.entry_seg = w.entry_seg; rec.seg_dir = w.seg_dir;
	lists.slow_list = w.slow_list; lists.lc = w.lc; lists.slot_base = w.slot_base;
	lists.entry_cap = (uint32_t)w.entry_cap; lists.ctr = w.d_ctr;
}

static void sweep_args(mc33hip_ctx *c, const SlotGeom &g, SweepArgs &a) {
	a.G = grid_view(c);
	a.P = c->P;
	a.sd = g.sd;
	a.tiles = c->plan[c->cur_plan].d_tiles;
	a.ntiles = (uint32_t)c->plan[c->cur_plan].ntiles;
	a.z_end = c->range.z_end;
	a.trace = nullptr;
	a.ranges = nullptr;
	a.skipped = nullptr;
	a.live = nullptr;
	a.blockw = nullptr;
	a.debug = 0;
	for (int q = 0; q < SWEEP_MAXNI; q++) a.lane[q] = SweepLane{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, (real_t)0, 0, 0xFFFFFFFFu};
}
// The range table for the sweep that is about to be enqueued on st, or nullptr: no table (the sweep streams every tile).
// Trust: only over samples this library knows to be unchanged - its own copy (every upload comes through forget_sweeps), or an
// adopted buffer between mc33hip_grid_stable(c, 1) and the next mc33hip_grid_changed / mc33hip_adopt_device.
// When: by the SECOND sweep since the samples last changed - a one-shot extraction and a caller whose samples change every step
// never pay for it.  The build is one launch on st in front of the sweep; the host waits for nothing.  No memory for the table,
// or a grid beyond one launch: no table, which is not an error.
static const RangeEntry *sweep_ranges(mc33hip_ctx *c, hipStream_t st) {
	if (c->ranges_off || !c->d_grid || !(c->owns_grid || c->grid_stable)) return nullptr;
	if (c->ranges_valid) return c->d_ranges;
	if (++c->sweeps_seen < 2u) return nullptr;
	const Params &P = c->P;
	const uint32_t nYT = (P.ny + 62) / 63, nXG = (P.nseg + 3) / 4, npl = c->desc.npz_resident;
	const uint64_t n = (uint64_t)npl * nYT * P.nseg, blocks = (uint64_t)npl * nYT * nXG;
	if (blocks > 0x7FFFFFFFull) return nullptr;
	if (c->ranges_cap < n && dev_room("range table", &c->d_ranges, &c->ranges_cap, n) != 0) { (void)hipGetLastError(); return nullptr; }
	// (the block table beside it, from the same pass: no memory for it, or MC33_HIP_BLOCKS=0, and the sweeps leave no block out)
	RangeEntry *fine = nullptr;
	if (!c->blocks_off) {
		if (c->blocks_cap >= n * RANGE_BLOCKS || dev_room("block table", &c->d_blocks, &c->blocks_cap, n * RANGE_BLOCKS) == 0) fine = c->d_blocks;
		else (void)hipGetLastError();
	}
	const bool vec = (uintptr_t)c->d_grid % 16u == 0 && (c->pitch * sizeof(sample_t)) % 16u == 0 && (c->slice * sizeof(sample_t)) % 16u == 0;
	if (vec) hipLaunchKernelGGL(k_ranges<true>, dim3((uint32_t)blocks), dim3(256), 0, st, grid_view(c), P, nYT, npl, c->d_ranges, fine);
	else hipLaunchKernelGGL(k_ranges<false>, dim3((uint32_t)blocks), dim3(256), 0, st, grid_view(c), P, nYT, npl, c->d_ranges, fine);
	if (hipGetLastError() != hipSuccess) return nullptr;
	c->ranges_valid = true;
	c->blocks_made = fine != nullptr;
	return c->d_ranges;
}

// The policy of the sweeps with a table - which plan, what size, who gets a list - is mc33_sweep_plan.h (TablePolicy); here the
// context's share: the published word as it stands, the facts, the list's buffers.
static unsigned long long live_word(const mc33hip_ctx *c) { return c->h_live ? __atomic_load_n(c->h_live, __ATOMIC_RELAXED) : 0ull; }
// plan: the plan in force, or the one the policy's target names - nullptr when its slot holds another (table_retarget)
static TableFacts table_facts(const mc33hip_ctx *c, uint32_t zs, uint32_t ze, const SweepPlan *plan) {
	return TableFacts{sweep_unit(plan_grid(c), zs, ze), c->resident_blocks, c->sw.min_depth, sweep_plane_weight(c), c->sw.sweep_blocks_per_cu != 0u, c->sw.rz, c->sw.rz_table, c->sw.table_tiles, c->sw.live, plan ? plan->ntiles : 0u, plan == &c->plan[2]};
}
static void table_retarget(mc33hip_ctx *c, uint32_t zs, uint32_t ze) {
	const SweepPlan &pl = c->plan[c->table.target ? 2 : 1];
	const bool held = pl.d_tiles && plan_is_sized_as(pl.key, zs, ze, c->table.target, sweep_plane_weight(c));  // (else the slot holds another plan, and the count goes by the word's own tiles)
	const unsigned long long w = live_word(c), was = c->table.target;
	table_retarget(c->table, w, table_facts(c, zs, ze, held ? &pl : nullptr));
	if (c->sw.verbose && !c->sw.table_tiles && c->table.target != was)
		fprintf(stderr, "[mc33hip] table plan: %llu of %llu tiles live, %u tiles asked for (were %u)\n", (unsigned long long)(w >> 32), (unsigned long long)((w & 0xFFFFFFFFull) >> 1), c->table.target, (uint32_t)was);
}
// Room for the live list of the sweep about to be launched, when it goes by one (table_wants_list).  No memory for the list: the
// preamble form, which is not an error.
static void sweep_live(mc33hip_ctx *c, SweepArgs &a) {
	c->live_blocks = 0;
	if (!a.ranges) return;
	const SweepPlan &pl = c->plan[c->cur_plan];
	const uint64_t blocks = (pl.ntiles + 3) / 4;
	if (!table_wants_list(c->table, table_facts(c, pl.key.zs, pl.key.ze, &pl))) return;
	if (!c->h_live && hipHostMalloc(&c->h_live, sizeof *c->h_live, hipHostMallocDefault) == hipSuccess) *c->h_live = 0ull;
	else if (!c->h_live) (void)hipGetLastError();  // (no pinned word: nothing is published, the finer plan stays)
	if ((c->verdict_cap < blocks && dev_room("tile verdicts", &c->d_verdict, &c->verdict_cap, blocks) != 0) ||
	    (c->live_cap < blocks + 1 && dev_room("live list", &c->d_live, &c->live_cap, blocks + 1) != 0) ||
	    (c->packed_cap < 5 * blocks + 4 && dev_room("packed live list", &c->d_packed, &c->packed_cap, 5 * blocks + 4) != 0)) {  // (header, entries, a word per quad: k_live_compact)
		(void)hipGetLastError();
		return;
	}
	a.live = c->d_packed;
}

// SweepLane::iso_gt / iso_eq of an isovalue for packed samples of `top` as their largest value
static void sweep_iso_words(real_t v, real_t top, int32_t &gt, uint32_t &eq) {
	const real_t fl = std::floor(v);
	gt = !(v == v) ? 0x7FFFFFFF : fl < 0 ? -1 : fl >= top ? (int32_t)top : (int32_t)fl;
	eq = (v == fl && fl >= 0 && fl <= top) ? (uint32_t)fl : 0xFFFFFFFFu;
}
static void set_lane(SweepArgs &a, int q, const IsoLane &L, double iso) {
	a.lane[q] = SweepLane{L.slice_hdr, L.slice_bits, L.slice_compact, L.plane_fmt, lane_part(L, false), L.edge_bits, L.edge_hdr, L.epoch, (real_t)iso, 0, 0xFFFFFFFFu};
	if (SWEEP_PACK > 1) sweep_iso_words((real_t)iso, SWEEP_PACK == 2 ? (real_t)65535 : (real_t)255, a.lane[q].iso_gt, a.lane[q].iso_eq);
}

// narrow samples are loaded as dwords when every row of the grid starts on a dword boundary (always true for the
// library's own pitched copy; a caller's device buffer may have any pitch)
// (The three terms are about aligned loads, not about the result: a dword is addressed from its row's first sample, so with a
// base, pitch or slice that is no multiple of 4 bytes the same bytes would come from misaligned dword loads, which this device
// serves - dropping the slice term leaves every surface of tests/test_gpu_layouts.py bit-identical, layout slice_odd included.
// The terms keep the packed form to loads that are aligned on every device, and to one cache line each.)
static bool sweep_packed(const mc33hip_ctx *c) {
	return SWEEP_PACK > 1 && !c->sw.no_pack && ((uintptr_t)c->d_grid % 4u) == 0 && (c->pitch * sizeof(sample_t)) % 4u == 0 &&
	       (c->slice * sizeof(sample_t)) % 4u == 0;
}

// one k_sweep launch over NI = 1, 2 or 4 lanes that begin_lane has prepared
// (all return the samples per lane and load of the form that was launched: k_cells needs it - lane_of_column)
template <int NI, int ZM>
static uint32_t launch_sweep_zm(mc33hip_ctx *c, const SweepArgs &a_in, hipStream_t st) {
	SweepArgs a = a_in;
	const uint64_t blocks = (c->plan[c->cur_plan].ntiles + 3) / 4;
	if (a.live) {  // the verdicts and the live list, in front of the sweep that goes by them (sweep_live)
		hipLaunchKernelGGL(k_tile_verdicts<NI>, dim3((uint32_t)((blocks + 3) / 4)), dim3(256), 0, st, a, c->d_verdict, (uint32_t)blocks);
		// The block verdicts of the live tiles, for the one form of the sweep that leaves blocks out (sweep_tile: BS) - a word per strip
		// of the resident planes, so the room does not depend on the plan.  No block table or no memory: every block is streamed.
		// Where it pays: rows of at least four segments, whose blocks are grouped - three waves in four take their halo bits from the
		// mailbox and a dead quarter is a whole instruction less.  On narrower grids every wave loads its own halo column and the launch
		// in front (11 us at 1024^3) was not won back: 768^3 measured 0.8 % slower with it (profiles/r11_block_skip.txt D).
		// MC33_HIP_BLOCKS=1: wherever there is a list (the tests run on narrow grids).
		if (MC33_BLOCK_SKIP && NI == 1 && ZM == 0 && a.ranges && c->blocks_made && c->d_blocks && !c->blocks_off && (c->blocks_always || a.sd.nseg >= 4u)) {
			const uint64_t n = (uint64_t)c->desc.npz_resident * a.sd.nYT * a.sd.nseg;
			bool room = c->blockw_cap >= n;
			if (!room && dev_room("block verdicts", &c->d_blockw, &c->blockw_cap, n) == 0)  // (new memory: all ones, which no verdict is - mc33hip_block_words shows the strips no sweep has written)
				room = hipMemsetAsync(c->d_blockw, 0xFF, n * sizeof(unsigned long long), st) == hipSuccess;
			if (room) {
				hipLaunchKernelGGL(k_block_verdicts, dim3(a.ntiles), dim3(256), 0, st, a, c->d_verdict, c->d_blocks, c->d_blockw);
				a.blockw = c->d_blockw;
			} else (void)hipGetLastError();
		}
		hipLaunchKernelGGL(k_live_compact, dim3(1), dim3(1024), 0, st, c->d_verdict, (uint32_t)blocks, c->d_live, c->d_packed, c->h_live, c->cur_plan ? 1u : 0u, a.ntiles, c->sw.list_lds);
		c->live_blocks = blocks;
	}
	// (packed narrow samples, several isovalues, classified by subtraction - an isovalue of -0.0 among them: the conversions of
	// a batch and the sets of bit rows do not fit the registers of 3 waves per SIMD - 468 bytes of scratch per lane for uchar
	// with four isovalues, 20 for ushort, 8 for uchar with two; that corner takes the unpacked form, which has none)
	constexpr bool packed_form = !(SWEEP_PACK >= 2 && NI >= 2 && ZM == 0);
	if (packed_form && sweep_packed(c)) {
		if (a.live) hipLaunchKernelGGL((k_sweep_live<packed_form ? SWEEP_PACK : 1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
		else if (a.ranges) hipLaunchKernelGGL((k_sweep<packed_form ? SWEEP_PACK : 1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
		else hipLaunchKernelGGL((k_sweep_all<packed_form ? SWEEP_PACK : 1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
		return (uint32_t)SWEEP_PACK;
	}
	if constexpr (MC33_BLOCK_SKIP && NI == 1 && ZM == 0) {
		if (a.live && a.blockw) { hipLaunchKernelGGL((k_sweep_live_blocks<ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a); return 1u; }
	}
	if (a.live) hipLaunchKernelGGL((k_sweep_live<1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
	else if (a.ranges) hipLaunchKernelGGL((k_sweep<1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
	else hipLaunchKernelGGL((k_sweep_all<1, NI, ZM>), dim3((uint32_t)blocks), dim3(256), 0, st, a);
	return 1u;
}
template <int NI>
static uint32_t launch_sweep_ni(mc33hip_ctx *c, const SweepArgs &a, hipStream_t st) {
#ifdef MC33_INT_SAMPLES
	// which classification the isovalues of this pass allow (k_sweep's ZM)
	bool negzero = false, can_equal = false;
	for (int q = 0; q < NI; q++) {
		const real_t iso = a.lane[q].iso;
		negzero |= iso == 0 && sign_of(iso);
		can_equal |= iso >= 0 && iso <= (real_t)std::numeric_limits<sample_t>::max() && iso == std::floor(iso);
	}
	if (!negzero) {
		if (can_equal) return launch_sweep_zm<NI, 1>(c, a, st);
		return launch_sweep_zm<NI, 2>(c, a, st);
	}
#endif
	return launch_sweep_zm<NI, 0>(c, a, st);
}

// Parameters of the passes for the isovalue of one lane (fill_params made c->P for the call's own isovalue)
static Params lane_params(const mc33hip_ctx *c, double iso) {
	Params P = c->P;
	P.iso = (real_t)iso;
	P.negzero_iso = (P.iso == 0 && sign_of(P.iso)) ? 1 : 0;
	return P;
}

// Everything after the sweep for the slices the lanes idx[0 .. n) hold (n <= SWEEP_MAXNI; lane idx[q] works into set sidx[q]): tile
// boundaries, record ranges, cell records, slow-cell planning, scans - ONE launch of each kernel for all n isovalues
// (PerLane, blockIdx.y), on the context's stream, no synchronisation.  isos[q]: the isovalue of lane idx[q].
static int enqueue_tail(mc33hip_ctx *c, const int *idx, const int *sidx, const double *isos, int n, const SlotGeom &g) {
	hipStream_t st = c->stream;
	const uint32_t ze = c->range.z_end;
	// (the lanes of a call were swept by one pass, so by one plan: the one their edge records are paired by)
	const PlanRef &lr = c->lanes[idx[0]].plan;
	if (int rc = plan_sweep(c, c->P.zs, ze, lr.slot != 0, lr.target, lr.weight)) return rc;
	const SweepPlan &pl = c->plan[c->cur_plan];
	SweepArgs a;
	sweep_args(c, g, a);
#ifdef MC33_DEV
	a.debug = c->sw.debug;
#endif
	PerLane<SlotsArgs> SA;
	PerLane<CellsArgs> CA;
	PerLane<SlowArgs> WA;
	PerLane<ScanArgs> NA;
	static_assert(sizeof(PerLane<CellsArgs>) <= 3584 && sizeof(PerLane<SlowArgs>) <= 3584, "kernel argument segment");
	memset(&SA, 0, sizeof SA); memset(&CA, 0, sizeof CA); memset(&WA, 0, sizeof WA); memset(&NA, 0, sizeof NA);
	if (!c->cells_blocks) {  // (asked before anything of the tail is launched: nothing below can return between k_slots and k_scan_apply)
		int per_cu = 0, cus = 0;
		HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_cells, 256, 0));
		HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
		c->cells_blocks = (uint32_t)std::max(1, per_cu) * (uint32_t)std::max(1, cus);
	}
	const uint32_t nb = (uint32_t)((c->nsegs + SCAN_CHUNK - 1) / SCAN_CHUNK);
	bool boundaries = false;
	for (int q = 0; q < n; q++) {
		IsoLane &L = c->lanes[idx[q]];
		TailSet &w = c->ts[sidx[q]];
		const Params P = lane_params(c, isos[q]);
		if (w.slot_base_cap < g.nslots)
			if (int rc = dev_room_all("slot bases", &w.slot_base_cap, g.nslots, {dev_array(&w.slot_base, g.nslots), dev_array(&w.live_list, g.nslots)})) return rc;
		// batch descriptors: every 64 records one, plus at most one partly filled batch per slice slot
		if (const uint64_t need = w.entry_cap / 64 + g.nslots + 64; w.batch_cap < need)
			if (int rc = dev_room("batch descriptors", &w.batches, &w.batch_cap, need)) return rc;
		set_lane(a, q, L, isos[q]);
		boundaries |= !L.boundary_done;
		CellsArgs &ca = CA.a[q];
		ca.pack = L.pack ? L.pack : 1u;
		ca.dev = 0;
#ifdef MC33_DEV
		ca.dev = c->sw.cells_dev;
#endif
		ca.G = grid_view(c);
		ca.P = P; ca.fast = c->d_fast; ca.pat = c->d_pat; ca.pat_order = c->d_pat_order;
		ca.ze = ze; ca.sd = g.sd;
		ca.slice_hdr = L.slice_hdr; ca.slice_bits = L.slice_bits; ca.slice_compact = L.slice_compact; ca.plane_fmt = L.plane_fmt;
		// the tag of this tail's row-segment counts; the array is cleared whenever the tags start over
		if (w.tail_serial % SEG_TAGS == 0) HIP_TRY(hipMemsetAsync(w.seg_cnt, 0, w.seg_cap * 4, st));
		const uint32_t seg_tag = w.tail_serial % SEG_TAGS + 1u;
		w.tail_serial++;
		ca.seg_tag = seg_tag;
		ca.live_list = w.live_list; ca.live_cap = (uint32_t)std::min<uint64_t>(g.nslots, 0xFFFFFFFFull);
		ca.epoch = L.epoch;
		ca.seg_cnt = w.seg_cnt; ca.dirty_list = w.dirty_list;
		ca.batches = w.batches; ca.batch_cap = (uint32_t)std::min<uint64_t>(w.batch_cap, 0xFFFFFFFFull);
		ca.trace = nullptr;
		if (n == 1 && c->sw.trace_cells) {
			c->trace_cells_n = 0;  // (a new one for every tail)
			if (int rc = dev_room("cell trace", &c->trace_cells, &c->trace_cells_n, g.nslots, 32)) return rc;
			HIP_TRY(hipMemsetAsync(c->trace_cells, 0, g.nslots * 32, st));
			ca.trace = c->trace_cells;
		}
		{  // groups of slots for the slow / dirty lists: at most LIST_CHUNKS
			uint32_t shift = 6;
			while (((g.nslots + (1ull << shift) - 1) >> shift) > LIST_CHUNKS) shift++;
			w.lc = ListChunks{w.list_cnt, w.list_cnt + LIST_CHUNKS, (uint32_t)((g.nslots + (1ull << shift) - 1) >> shift), shift};
		}
		set_arrays(w, ca, ca);
		const uint64_t nchunks = (L.slice_cap + SLOT_CHUNK - 1) / SLOT_CHUNK;
		SA.a[q] = SlotsArgs{L.slice_hdr, lane_part(L, false), lane_part(L, true), (uint32_t)nchunks, L.epoch, w.slot_base, w.d_ctr, w.lc,
		                    (unsigned long long *)(w.bsV + 2 * w.bs_cap), (uint32_t)(2 * scan_groups(w.bs_cap)), w.live_list, ca.live_cap};
		SlowArgs &sa = WA.a[q];
		sa.G = ca.G; sa.P = P;
		sa.tab = tables(c);
		sa.z_emit = c->range.z_begin;
		set_arrays(w, sa, sa);
		sa.entries_c = w.entries_c; sa.fast_b = c->d_fast_b;
		sa.seg_cnt = w.seg_cnt; sa.seg_tag = seg_tag; sa.dirty_list = w.dirty_list;
		uint64_t *grV = scans_grouped(nb) ? w.bsV + 2 * w.bs_cap : nullptr, *grT = grV ? grV + scan_groups(w.bs_cap) : nullptr;
		NA.a[q] = ScanArgs{w.seg_cnt, seg_tag, w.lc.slow_cnt, w.lc.n, w.bsV, w.bsT, grV, grT, w.seg_base, w.d_ctr};
		// k_slots appends to live_list from Counters::live_cursor on, and k_scan_apply - the last kernel of a tail - leaves the
		// cursor zero for the next.  A tail that was cut short (a launch error) leaves it wherever it was: the next one starts clean.
		if (w.tail_incomplete) HIP_TRY(hipMemsetAsync(&w.d_ctr->live_cursor, 0, sizeof(uint32_t), st));
		w.tail_incomplete = true;
		w.ctr_published = false;  // (the counters of THIS tail are on the device until somebody brings them over)
	}
	const uint32_t ny = (uint32_t)n;
	if (pl.nbounds && boundaries && !(MC33_DEBUG_BITS(a) & 2u))  // (the lanes of a call are all fresh, or it is one lane)
		hipLaunchKernelGGL(k_boundary, dim3((uint32_t)((pl.nbounds + 3) / 4), ny), dim3(256), 0, st, a, pl.d_bounds, (uint32_t)pl.nbounds);
	for (int q = 0; q < n; q++) c->lanes[idx[q]].boundary_done = true;  // (its slices are in the partial sums now: a repeated tail - more room for records - must not add them again)
	hipLaunchKernelGGL(k_slots, dim3((uint32_t)((g.nslots + SLOT_CHUNK - 1) / SLOT_CHUNK), ny), dim3(256), 0, st, SA, g.nslots);
	for (int q = 0; q < n; q++) c->lanes[idx[q]].tail_pending = false;  // k_slots has read this epoch's partial sums and cleared the half of the next one
	// (four times what the GPU holds at once: slices differ in length, and a block that starts late evens the waves out -
	// 76 -> 66 us at 1024^3; a block per group of four slots, as until round 3, is 17 408 blocks there)
	hipLaunchKernelGGL(k_cells, dim3((uint32_t)std::min<uint64_t>(g.cell_blocks, c->sw.cells_blocks ? c->sw.cells_blocks : 4u * c->cells_blocks), ny), dim3(256), 0, st, CA);
	// (blocks beyond the lists end at once.  A grid sized from the last extraction's counts - 69 blocks instead of 1024 at 1024^3,
	// whose 8 820 slow cells are 35 blocks' worth - changes nothing: 13.5 / 6 / 8.7 us either way.  What these kernels take is
	// the chain of dependent loads of the cells that ARE slow, not their empty blocks; round 3)
	const uint32_t slow_blocks = c->sw.slow_blocks ? c->sw.slow_blocks : 1024u;
	// planning, identity counts and segment offsets: three launches (as one launch with grid barriers: slower, EXPERIMENTS.md).
	// The slow kernels serve the cells with a corner equal to the isovalue (cells on the grid's faces are finished by k_cells: FACE
	// records) - none at all on most fields, where the three launches cost ~25 us of nothing.  A call that reads the counters before it
	// returns (mc33hip_extract, mc33hip_count: alias_gate) leaves them out when the last extraction of the set had no slow cells; k_scan_apply
	// counts them all the same (Counters::alias_cells), the emit passes refuse such a tail (emit_prepare), and the call makes it again
	// with them (a miss).  Everything that hands counts on before a host synchronisation keeps them.
	bool gate = c->alias_gate && n == 1;
	for (int q = 0; q < n; q++) gate = gate && c->ts[sidx[q]].alias_known && c->ts[sidx[q]].alias_last == 0u;
	for (int q = 0; q < n; q++) c->ts[sidx[q]].alias_gated = gate;
	if (!gate) {
		hipLaunchKernelGGL(k_slow_plan, dim3(slow_blocks, ny), dim3(256), 0, st, WA);
		// k_slow_count only when the last extraction of (one of) the set(s) had records for it, or nothing is known: k_seg_fix counts what is left over
		bool wanted = false;
		for (int q = 0; q < n; q++) wanted |= !c->ts[sidx[q]].count_known || c->ts[sidx[q]].count_needed;
		if (c->sw.slow_count >= 0) wanted = c->sw.slow_count != 0;
		if (wanted) hipLaunchKernelGGL(k_slow_count, dim3(slow_blocks, ny), dim3(256), 0, st, WA);
		hipLaunchKernelGGL(k_seg_fix, dim3(slow_blocks, ny), dim3(256), 0, st, WA);
	}
	hipLaunchKernelGGL(k_scan_reduce, dim3(nb, ny), dim3(256), 0, st, NA, c->nsegs, c->P);
	hipLaunchKernelGGL(k_scan_apply, dim3(nb, ny), dim3(256), 0, st, NA, c->nsegs, c->P, c->ghost_segs);
	HIP_TRY(hipGetLastError());
	for (int q = 0; q < n; q++) c->ts[sidx[q]].tail_incomplete = false;
	return 0;
}

// the isovalue a lane was swept for, compared by bit pattern: +0.0 and -0.0 compare equal but classify samples equal to
// them differently (v = iso - F = -0 is "zero AND negative", Params::negzero_iso), and a NaN is the same NaN
static bool same_bits(real_t a, real_t b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same_range(const mc33hip_range &x, const mc33hip_range &y) {
	return x.z_begin == y.z_begin && x.z_end == y.z_end && (x.ghost_below != 0) == (y.ghost_below != 0);
}

// enqueue sweep + cell records + slow-cell planning + scans on the context's stream (no synchronisation).  When
// mc33hip_sweep_many has already classified this isovalue over this range, its lane is used and nothing is streamed - and
// when it has made the tail ahead as well (the lane's own TailSet), nothing is enqueued at all: the counters are waiting.
static int enqueue_count(mc33hip_ctx *c, bool rerun = false) {
	const Params &P = c->P;
	hipStream_t st = c->stream;
	SlotGeom g;
	if (int rc = slot_geometry(c, g)) return rc;
	IsoLane *L = nullptr;
	bool tail_made = false;
	if (rerun && c->cur_lane && c->lane_presweeped) L = c->cur_lane;  // same call, more room for records: the sweep's result stands, the tail is made again
	else
		for (int k = 0; k < MC33_LANES && !L; k++)
			if (c->lanes[k].swept && same_bits((real_t)c->lanes[k].iso, P.iso) && same_range(c->lanes[k].range, c->range) &&
			    c->lanes[k].slice_cap >= g.nslots) {
				// (the plan it was swept by is looked at, not put in force: when its place holds another range's plan by now, the tail
				// makes it again - the same plan, which the lane's edge buffers had room for)
				const SweepPlan &lp = c->plan[c->lanes[k].plan.slot];
				if (lp.d_tiles && plan_is_lanes(lp.key, c->lanes[k].plan, P.zs, c->range.z_end) && c->lanes[k].edge_cap < lp.ntiles) continue;
				L = &c->lanes[k];
				tail_made = L->tail_done;
			}
	if (c->timing_level > 0) HIP_TRY(hipEventRecord(c->ev[0], st));
	if (L) {
		// a sweep made ahead is used once when its tail is made here (in the shared set 0, which the next isovalue overwrites); a
		// lane whose tail was made ahead as well - in a set of its own - stays good for any number of count / emit calls until the
		// next mc33hip_sweep_many or a change of the grid (slabs: count all isovalues, ONE exchange of counts, then the emits)
		if (!tail_made) { L->swept = false; L->tail_done = false; }
		c->lane_presweeped = true;
	} else {
		L = &c->lanes[0];
		const RangeEntry *ranges = sweep_ranges(c, st);
		table_retarget(c, P.zs, c->range.z_end);
		if (int rc = plan_sweep(c, P.zs, c->range.z_end, ranges && table_plan(c->table, live_word(c)), c->table.target, sweep_plane_weight(c))) return rc;
		if (int rc = begin_lane(c, *L, g, st)) return rc;
		c->lane_presweeped = false;
		SweepArgs a;
		sweep_args(c, g, a);
		set_lane(a, 0, *L, P.iso);
		a.ranges = ranges;
		sweep_live(c, a);
		c->skipped_tiles = 0;
		if (c->timing_level > 0 && (c->d_skipped || hipMalloc(&c->d_skipped, 8 * sizeof(uint32_t)) == hipSuccess)) {  // (mc33hip_sweep_skipped; never on the production path)
			HIP_TRY(hipMemsetAsync(c->d_skipped, 0, 8 * sizeof(uint32_t), st));
			a.skipped = c->d_skipped;
			c->skipped_tiles = a.ntiles;
		} else if (c->timing_level > 0) (void)hipGetLastError();
#ifdef MC33_DEV
		a.debug = c->sw.debug;
		if (a.debug) {  // never silent: with this set the call measures the sweep's read stream and finds no surface
			static bool warned = false;
			if (!warned) fprintf(stderr, "[mc33hip] MC33_HIP_DEBUG=%u: timing experiment, every extraction returns an EMPTY surface\n", a.debug);
			warned = true;
		}
#endif
		if (c->sw.trace_file) {
			c->trace_waves = 0;  // (a new one for every sweep)
			if (int rc = dev_room("sweep trace", &c->trace, &c->trace_waves, (((uint64_t)a.ntiles + 3) / 4) * 4, 32)) return rc;
			HIP_TRY(hipMemsetAsync(c->trace, 0, c->trace_waves * 32, st));
			a.trace = c->trace;
			if (c->timing_level > 0) HIP_TRY(hipEventRecord(c->ev[0], st));
		}
		// nothing is cleared between extractions: headers carry the epoch, k_slots resets the counters and the
		// partial sums of the next call, the counts of the row segments carry the tag of the tail that wrote them (seg_tagged)
		L->pack = launch_sweep_ni<1>(c, a, st);
		L->tail_pending = true;
		HIP_TRY(hipGetLastError());
	}
	c->cur_lane = L;
	if (!rerun) c->lane_pretailed = tail_made;  // (a repeated count of the same call: the lane still has its own set)
	const int li = (int)(L - c->lanes);
	if (c->timing_level > 1) HIP_TRY(hipEventRecord(c->ev[1], st));
	if (tail_made) c->w = &c->ts[li];  // (made behind its sweep pass, in the lane's own set)
	else {
		// a tail made here works in the lane's own set when it has one (a repeated tail - more room for records - of a lane that had
		// been made ahead), in set 0 otherwise
		const int si = (rerun && c->lane_pretailed) ? li : 0;
		c->w = &c->ts[si];
		if (int rc = ensure_set(c, *c->w)) return rc;
		const double iso = (double)P.iso;
		if (int rc = enqueue_tail(c, &li, &si, &iso, 1, g)) return rc;
		if (rerun && c->lane_pretailed) { L->swept = true; L->tail_done = true; }  // (made again in its own set: good for further calls, as before)
	}
	if (c->timing_level > 1) HIP_TRY(hipEventRecord(c->ev[2], st));
	return 0;
}

// Sweeps for n isovalues over one range, SWEEP_MAXNI isovalues per pass over the grid; the count / extract calls that follow
// (same isovalue, same range) find their lane and go straight to the tail.  tails_ahead (mc33hip_prepare_many): the tails
// too, right behind each pass, one launch of each tail kernel per pass, every isovalue into a TailSet of its own - the calls
// then have nothing left to do but fetch the counters / emit, in any order, any number of times (when there is not enough
// device memory for the sets: sweeps only, as without the flag).
// Measured (round 4, 2048 x 2048 x 1024 ushort, 8 isovalues, profiles/r04_tails_ahead.txt): the batched tails take 0.29 ms per
// isovalue instead of 0.345 (k_cells 188 us per isovalue instead of 214, k_boundary 16 instead of 23; the scans gain nothing),
// but the vertex pass of an isovalue whose records were written eight tails ago instead of just now takes 30 % longer (avg
// 575 instead of 442 us: its per-batch chain of record and row-base fetches finds them in HBM instead of the 256 MB
// last-level cache) - 14.2 ms per step against 13.2.  So a single GPU keeps tail and emit of an isovalue adjacent
// (mc33hip_sweep_many), and the sets are for callers that need ALL counts before the first emit (z-slabs over several GPUs:
// one exchange of counts per step instead of one per isovalue).
static int enqueue_sweep_many(mc33hip_ctx *c, const double *isos, int n, bool tails_ahead) {
	hipStream_t st = c->stream;
	SlotGeom g;
	if (int rc = slot_geometry(c, g)) return rc;
	if (tails_ahead) {
		// records to make room for in a new set: what the last extraction of this context needed
		uint64_t hint = 0;
		for (int k = 0; k < MC33_LANES; k++) hint = std::max<uint64_t>(hint, c->ts[k].records_hint);
		for (int k = 0; k < n && tails_ahead; k++)
			if (ensure_set(c, c->ts[k], hint) != 0) {  // (out of device memory: no sets beyond the first, no tails ahead)
				forget_sweeps(c);  // (first: a lane that still said "tail made" would send a later count to a set that is gone)
				for (int j = 1; j <= k; j++) free_set(c->ts[j]);
				(void)hipGetLastError();
				c->w = &c->ts[0];  // (the last count may have worked in one of the sets that are gone)
				c->shape_set = nullptr;  // (... and the last emit)
				c->counted = false;
				tails_ahead = false;
			}
		if (!tails_ahead) { if (int rc = ensure_set(c, c->ts[0])) return rc; }
	}
	int k = 0, pass = 0;
	while (k < n) {
		const int ni = (n - k >= 4) ? 4 : (n - k >= 2) ? 2 : 1;
		// (the table may be built in front of the second pass: every pass goes by the plan of what it has, and its lanes keep it)
		const RangeEntry *ranges = sweep_ranges(c, st);
		// (every pass of the call by the same plan with a table: its default depth, or the size MC33_HIP_TABLE_TILES forces - table_retarget)
		if (int rc = plan_sweep(c, c->P.zs, c->range.z_end, ranges && table_plan(c->table, live_word(c)), c->sw.table_tiles)) return rc;
		SweepArgs a;
		sweep_args(c, g, a);
#ifdef MC33_DEV
		a.debug = c->sw.debug;
#endif
		for (int q = 0; q < ni; q++) {
			IsoLane &L = c->lanes[k + q];
			if (int rc = begin_lane(c, L, g, st)) return rc;
			set_lane(a, q, L, isos[k + q]);
		}
		a.ranges = ranges;
		sweep_live(c, a);
		// (events around the pass are only recorded; read_timing asks for the elapsed time when the lane is consumed)
		const bool timed = c->timing_level > 0 && pass < MC33_MANY_PASSES;
		if (timed) HIP_TRY(hipEventRecord(c->ev_many[pass][0], st));
		const uint32_t pack = ni == 4 ? launch_sweep_ni<4>(c, a, st) : ni == 2 ? launch_sweep_ni<2>(c, a, st) : launch_sweep_ni<1>(c, a, st);
		HIP_TRY(hipGetLastError());
		if (timed) HIP_TRY(hipEventRecord(c->ev_many[pass][1], st));
		int idx[SWEEP_MAXNI];
		for (int q = 0; q < ni; q++) {
			IsoLane &L = c->lanes[k + q];
			L.swept = true; L.tail_pending = true; L.tail_done = false; L.iso = isos[k + q]; L.range = c->range; L.pack = pack;
			L.many_pass = timed ? pass : -1; L.many_ni = ni;
			idx[q] = k + q;
		}
		if (tails_ahead) {
			if (int rc = enqueue_tail(c, idx, idx, isos + k, ni, g)) return rc;
			for (int q = 0; q < ni; q++) c->lanes[k + q].tail_done = true;
		}
		if (timed) HIP_TRY(hipEventRecord(c->ev_many[pass][2], st));
		k += ni;
		pass++;
	}
	return 0;
}

// Host destinations of a pipelined download (mc33hip_emit_download): every array is copied on the context's copy stream as soon as
// the passes that write it have been through, while the remaining passes still run.
struct DownloadPlan { void *hV, *hN, *hT; size_t bV, bN, bT; };

static int enqueue_emit(mc33hip_ctx *c, void *dV, void *dN, void *dT, uint64_t capV, uint64_t capT, const DownloadPlan *dl = nullptr,
                        const unsigned long long *dev_base = nullptr, uint32_t seq = 0) {
	EmitArgs a;
	a.dev_base = dev_base;
	a.seq = seq;
	c->count_unused = false;  // (the count has served an emit: the next count of this isovalue is made anew)
	a.c.tab = tables(c);
	a.c.P = c->P;
	a.c.G = grid_view(c);
	set_arrays(*c->w, a.c, a);
	a.c.seg_base = c->w->seg_base; a.c.entries_c = c->w->entries_c; a.c.fast_b = c->d_fast_b; a.c.fast_b_in_lds = false;
	a.c.V = (real_t *)dV; a.c.N = (float *)dN; a.c.Tri = (uint32_t *)dT;
	a.c.z_emit = c->range.z_begin; a.c.v_skip = a.c.t_skip = a.c.id_delta = 0;
	a.capV = capV; a.capT = capT;
	a.ghost_segs = c->ghost_segs;
	a.id_base = c->range.id_base;
	a.batches = c->w->batches; a.batch_cap = (uint32_t)std::min<uint64_t>(c->w->batch_cap, 0xFFFFFFFFull);
	a.host_ctr = c->w->h_ctr;  // (hipHostMalloc'ed: the same address on the device)
	a.alias_gated = c->w->alias_gated ? 1u : 0u;
	c->w->ctr_published = true;
	// rows may be staged in 16-byte chunks when every row of the grid starts on a 16-byte boundary (always so for the library's
	// own copy; a caller's device buffer may have any pitch: its records then load for themselves)
	// (as in sweep_packed: chunks are addressed from the row's first sample, so the terms - the slice term too: a plane above the
	// first starts at base + k * slice - keep the 16-byte loads aligned; without them the result is the same, bit for bit)
	a.stage_rows = ((uintptr_t)c->d_grid % 16u) == 0 && (c->pitch * sizeof(sample_t)) % 16u == 0 && (c->slice * sizeof(sample_t)) % 16u == 0 &&
	               !c->sw.no_stage;
	// The triangle pass is fastest with a thread per record (C5, 14.4 M records: 16 384 / 32 768 / 65 536 blocks 392 / 363 /
	// 352 us; C3, 3.9 M: 2 048 / 4 096 / 8 192 / 16 384 blocks 106 / 98 / 93 / 88 us).  How many records this extraction has is
	// on the device only: the grid follows the last extraction whose counters were read, 16 384 blocks at least.
	const uint32_t blocks = c->sw.emit_blocks ? c->sw.emit_blocks : std::max(256u * 64u, std::min(1u << 20, ((c->w->records_hint + 255u) / 256u + 7u) & ~7u));
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	// The three emit passes are independent (V/N vs T, fast vs slow records).  While each of them waited through a chain of
	// dependent loads (rounds 1 and most of 2) running them side by side on three streams paid on large grids (0.15 instead
	// of 0.18 ms at 768^3); with the loads of a round trip asked for together they keep the GPU busy by themselves and
	// one after the other is as fast or faster (C3 tail 0.401 against 0.404 - 0.409 ms, C5 step 15.97 against 16.18 ms), without
	// the events between the streams.  MC33_HIP_NO_FORK=0 still runs them side by side.
	// MC33_HIP_NO_FORK: 0 = all three side by side, 1 = all in sequence, unset = the two fast passes in sequence and the slow one
	// behind them (few slow records) or, on large grids, beside them on a second stream (many: see below).
	const bool fork_env = c->sw.no_fork >= 0;
	const uint64_t range_cells = (uint64_t)c->P.nx * c->P.ny * (c->range.z_end - c->P.zs);
	const bool fork_all = c->sw.no_fork == 0;
	// Which fast pass goes first (round 4).  The triangle pass lives on dependent look-ups in what the tail has just written - records,
	// directory lines, segment bases: 144 MB at 1024^3 float - and right behind the tail it finds them in the 256 MB last-level cache;
	// behind the vertex pass, which pulls 0.45 GB of sample lines through that cache, it does not: 85 -> 68 - 70 us at 1024^3 with
	// the triangles first, the vertex pass unchanged (110 - 115), the step 1.05 - 1.06 -> 1.02 - 1.03 ms.  On the 2048 x 2048 x 1024
	// ushort grid (14.4 M records per isovalue: the set does not fit either way) the order costs the triangle pass 20 - 25 us and
	// gives the vertex pass 14: the vertex pass stays first there.  MC33_HIP_TRI_FIRST=0 / 1 forces the order.
	// The slow pass.  FEW slow records - the usual case: cells on the grid's faces, a corner equal to the isovalue here and there - go
	// through k_emit_slow_slots in sequence behind the two fast passes (8 800 records of the 1024^3 cos field in 14 us with the GPU to
	// itself; a thread per record: 31).  Until round 4 the pass always ran beside the fast passes on a second stream: an event at the
	// fork and a cross-queue wait at the join (6 - 7 us each inside an emit stage of 200), and once the triangle pass went first, slow
	// blocks still resident when the vertex pass placed its own - that kernel is as many blocks as the device holds (3 per CU by its
	// LDS image) with a fixed share of the batches each, and 26 KB of a slow block in the middle of a CU's LDS kept the CU's third
	// vertex block out until one of the other two had finished: 170 instead of 112 us in a third of the calls whenever the slow pass
	// ended 0 - 3 us behind the triangle pass (profiles/r04_vertex_pass_bimodal.txt).  MANY slow records (noise, integer isovalues on
	// integer grids) - or an unknown number - take a thread each (k_emit_slow), on large grids beside the fast passes on the second
	// stream as before, the vertex pass first as before.  MC33_HIP_SLOW_SLOTS=0 / 1 forces the kernel, MC33_HIP_NO_FORK the streams.
	const bool slow_slots = c->sw.slow_slots >= 0 ? c->sw.slow_slots != 0 : (c->w->slow_hint != 0u && c->w->slow_hint <= (c->sw.slow_slots_max ? c->sw.slow_slots_max : 32768u));
	const bool fork_slow = fork_all || (!fork_env && !slow_slots && range_cells >= 300000000ull);  // (small grids: the events cost more than they gain)
	const bool tri_first = !fork_all && (c->sw.tri_first >= 0 ? c->sw.tri_first != 0 : (c->w->records_hint <= 6000000u && !fork_slow));
	hipStream_t sv = fork_all ? c->aux : c->stream, ss = fork_slow ? c->aux2 : c->stream;
	if (fork_slow) {
		HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
		if (fork_all) HIP_TRY(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
		HIP_TRY(hipStreamWaitEvent(c->aux2, c->ev_fork, 0));
	}
	// Both slow kernels walk the slow list with a grid stride: any grid is right.  A thread per record: as many blocks as the last
	// extraction's slow records fill four times over, 64 at least (waves that are started beside the vertex pass only to find the list
	// exhausted cost it), 1 024 at most and while nothing is known.  A lane per slot, 16 records per block and round: as many blocks as
	// the records need and an eighth more, 1 024 at least (a block beyond the list leaves at once, and should the count have been an
	// earlier isovalue's and far too small, the kernel goes through the list with a thread per record: it needs the threads then).
	const uint32_t slow_grid = c->sw.slow_blocks ? c->sw.slow_blocks
	                           : slow_slots ? std::max(1024u, (c->w->slow_hint + c->w->slow_hint / 8u + 15u) / 16u)
	                           : c->w->slow_hint ? std::min(1024u, std::max(64u, (c->w->slow_hint + 255u) / 256u * 4u)) : 1024u;
#define MC33_LAUNCH_SLOW(st) do { if (a.alias_gated) break; if (slow_slots) hipLaunchKernelGGL(k_emit_slow_slots, dim3(slow_grid), dim3(256), 0, st, a); else hipLaunchKernelGGL(k_emit_slow, dim3(slow_grid), dim3(256), 0, st, a); } while (0)
	if (fork_slow) {  // (first: it is the one with the long chains)
		MC33_LAUNCH_SLOW(ss);
		HIP_TRY(hipEventRecord(c->ev_join2, c->aux2));
	}
	// A pipelined download wants every array complete as early as possible: the slow records - which write V, N AND T - go first
	// then (in sequence all the same: 14 us with the GPU to itself), and each fast pass is followed by the copies it completes.
	const bool dl_split = dl && !fork_all && !fork_slow;
	if (dl_split) MC33_LAUNCH_SLOW(ss);
	auto copy_T = [&]() -> int {
		HIP_TRY(hipEventRecord(c->ev_dl[0], c->stream));
		HIP_TRY(hipStreamWaitEvent(c->copy, c->ev_dl[0], 0));
		if (dl->bT) HIP_TRY(hipMemcpyAsync(dl->hT, dT, dl->bT, hipMemcpyDeviceToHost, c->copy));
		return 0;
	};
	auto copy_VN = [&]() -> int {
		HIP_TRY(hipEventRecord(c->ev_dl[1], c->stream));
		HIP_TRY(hipStreamWaitEvent(c->copy, c->ev_dl[1], 0));
		if (dl->bV) HIP_TRY(hipMemcpyAsync(dl->hV, dV, dl->bV, hipMemcpyDeviceToHost, c->copy));
		if (dl->bN) HIP_TRY(hipMemcpyAsync(dl->hN, dN, dl->bN, hipMemcpyDeviceToHost, c->copy));
		return 0;
	};
	if (tri_first) {
		hipLaunchKernelGGL(k_emit_fast_triangles, dim3(blocks), dim3(256), 0, sv, a);
		if (dl_split) { if (int rc = copy_T()) return rc; }
	}
	// as many blocks as the device holds at once (one more round of blocks would run with most of the GPU idle); every wave
	// walks many batches, its next batch's records in flight while it works on one
	if (!c->emit_v_blocks_per_cu) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->emit_v_blocks_per_cu, k_emit_vertices<3>, 256, 0));
	// (MC33_HIP_EMIT_V_BLOCKS: the grid itself, below what the device holds - fewer waves than batches, every wave walks several)
	const uint32_t vblocks = c->sw.emit_v_blocks ? c->sw.emit_v_blocks
	                         : (uint32_t)std::max(1, c->cus) * (c->sw.emit_v_blocks_per_cu ? c->sw.emit_v_blocks_per_cu : (uint32_t)std::max(1, c->emit_v_blocks_per_cu));
	const dim3 vgrid((vblocks + 7u) & ~7u);
	c->shape_set = c->w;  // what was launched, for mc33hip_emit_shape
	c->shape[0] = vgrid.x; c->shape[1] = blocks; c->shape[2] = slow_grid; c->shape[3] = a.alias_gated ? 2u : slow_slots ? 1u : 0u; c->shape[4] = tri_first ? 1u : 0u;
	switch (c->P.store_mode) {
	case 0: hipLaunchKernelGGL(k_emit_vertices<0>, vgrid, dim3(256), 0, c->stream, a); break;
	case 1: hipLaunchKernelGGL(k_emit_vertices<1>, vgrid, dim3(256), 0, c->stream, a); break;
	case 2: hipLaunchKernelGGL(k_emit_vertices<2>, vgrid, dim3(256), 0, c->stream, a); break;
	default: hipLaunchKernelGGL(k_emit_vertices<3>, vgrid, dim3(256), 0, c->stream, a); break;
	}
	if (dl_split) { if (int rc = copy_VN()) return rc; }
	if (!tri_first) {
		hipLaunchKernelGGL(k_emit_fast_triangles, dim3(blocks), dim3(256), 0, sv, a);
		if (dl_split) { if (int rc = copy_T()) return rc; }
	}
	if (fork_all) HIP_TRY(hipEventRecord(c->ev_join, c->aux));
	if (!fork_slow && !dl_split) MC33_LAUNCH_SLOW(ss);
#undef MC33_LAUNCH_SLOW
	HIP_TRY(hipGetLastError());
	if (fork_all) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
	if (fork_slow) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join2, 0));
	if (dl && !dl_split) {  // (passes on several streams: everything behind the join)
		if (int rc = copy_T()) return rc;
		if (int rc = copy_VN()) return rc;
	}
	if (c->timing_level > 0) HIP_TRY(hipEventRecord(c->ev[3], c->stream));
	c->emit_pending = true;
	return 0;
}

// what the host keeps of a set's counters once they are in h_ctr: the shape of the next tail and emit into this set
static void note_counters(mc33hip_ctx *c) {
	c->w->records_hint = c->w->h_ctr->entry_cursor == 0xFFFFFFFFu ? 0u : c->w->h_ctr->entry_cursor;
	c->w->slow_hint = c->w->h_ctr->slow_cursor + 1u;
	c->w->count_known = true; c->w->count_needed = c->w->h_ctr->count_pending != 0u;
	c->w->alias_known = true; c->w->alias_last = c->w->h_ctr->alias_cells;
	if (c->sw.verbose)
		fprintf(stderr, "[mc33hip] cut cells %u (slow %u - cells with a corner equal to the isovalue %u -, dirty segments %u, record batches %u%s)\n",
		        c->w->h_ctr->entry_cursor, c->w->h_ctr->slow_cursor, c->w->h_ctr->alias_cells, c->w->h_ctr->dirty_cursor, c->w->h_ctr->batch_cursor,
		        c->w->alias_gated ? "; slow kernels left out" : "");
}

// The counters of an extraction whose triangle pass was given the sequence word `seq` (enqueue_emit), without waiting for all of
// the emit passes: the first wave of that pass leaves counters, emit_skipped and then the word in pinned memory.  How early that
// is depends on where enqueue_emit puts the pass: first behind the tail while the record set fits the last-level cache (tri_first:
// up to 6 M records, the single-GPU float bench) - the call then returns with both fast passes still to run - but behind the
// vertex pass with more records or with the slow pass on its own stream (2048 x 2048 x 1024 ushort), where the call returns
// only once k_emit_vertices is through and little is gained.  That is the price of publishing from this pass and not from
// k_scan_apply (count_until_fits says why).  The wait is bounded: past the deadline the stream is synchronised as ever, which
// finds the counters there all the same.
static inline void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
	__builtin_ia32_pause();
#elif defined(__aarch64__)
	asm volatile("yield" ::: "memory");
#else
	std::this_thread::yield();
#endif
}
static int wait_counters(mc33hip_ctx *c, uint32_t seq) {
	const uint32_t *word = counters_seq(c->w->h_ctr);
	const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(50);
	for (uint32_t spins = 0; __atomic_load_n(word, __ATOMIC_ACQUIRE) != seq; spins++) {
		spin_pause();
		if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() > deadline) {
			HIP_TRY(hipStreamSynchronize(c->stream));
			if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != seq) { set_err("the counters of the extraction did not arrive"); return MC33HIP_ERUNTIME; }
			break;
		}
	}
	note_counters(c);
	return 0;
}

static int fetch_counters(mc33hip_ctx *c) {
	// (after an emit pass the triangle kernel has already written them into h_ctr: only the wait is left)
	if (!c->w->ctr_published) HIP_TRY(hipMemcpyAsync(c->w->h_ctr, c->w->d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
	c->w->ctr_published = true;  // (h_ctr matches the set's counters until the next tail into this set: enqueue_tail)
	HIP_TRY(hipStreamSynchronize(c->stream));  // (polling the stream before blocking - hipStreamQuery for up to 3 ms - gains nothing: 1.086 / 1.087 / 1.097 against 1.063 / 1.094 / 1.126 ms per step at 1024^3, round 4)
	note_counters(c);
	if (c->w->h_ctr->debug[0])
		fprintf(stderr, "[mc33hip] DEBUG words %u: first %u count %u z %u y0 %u xbase %u batch %u of %u\n", c->w->h_ctr->debug[0], c->w->h_ctr->debug[1], c->w->h_ctr->debug[2],
		        c->w->h_ctr->debug[3], c->w->h_ctr->debug[4], c->w->h_ctr->debug[5], c->w->h_ctr->debug[6], c->w->h_ctr->debug[7]);
	if (c->trace_cells && c->sw.trace_cells) {
		void *h = malloc(c->trace_cells_n * 32);
		if (h && hipMemcpy(h, c->trace_cells, c->trace_cells_n * 32, hipMemcpyDeviceToHost) == hipSuccess) {
			FILE *f = fopen(c->sw.trace_cells, "wb");
			if (f) { fwrite(h, 32, c->trace_cells_n, f); fclose(f); }
		}
		free(h);
	}
	if (c->trace && c->sw.trace_file) {  // developer tracing: per-wave stamps of the last sweep
		void *h = malloc(c->trace_waves * 32);
		if (h && hipMemcpy(h, c->trace, c->trace_waves * 32, hipMemcpyDeviceToHost) == hipSuccess) {
			FILE *f = fopen(c->sw.trace_file, "wb");
			if (f) { fwrite(h, 32, c->trace_waves, f); fclose(f); }
		}
		free(h);
	}
	return 0;
}

static int finish_counts(mc33hip_ctx *c, mc33hip_counts *out) {
	const Counters &h = *c->w->h_ctr;
	const uint64_t gV = c->ghost_segs ? h.ghostV : 0, gT = c->ghost_segs ? h.ghostT : 0;
	c->counts.nV = h.totV - gV; c->counts.nT = h.totT - gT;
	c->counts.nV_ghost = gV; c->counts.nT_ghost = gT;
	c->counts.active_cells = h.entry_cursor;
	if (out) *out = c->counts;
	if (h.totV > 0xFFFFFFFFull || h.totT > 0xFFFFFFFFull || (uint64_t)c->range.id_base + c->counts.nV > 0xFFFFFFFFull) {
		set_err("surface exceeds 2^32-1 vertices or triangles");
		return MC33HIP_EOVERFLOW;
	}
	return 0;
}

static void read_timing(mc33hip_ctx *c, bool with_emit, unsigned launches) {
	mc33hip_timing &t = c->timing;
	c->emit_pending = false;
	t.sweep_ms = t.scan_ms = t.emit_ms = t.total_ms = 0.f;
	t.sweep_launches = launches;
	if (c->timing_level > 1) {
		(void)hipEventElapsedTime(&t.sweep_ms, c->ev[0], c->ev[1]);
		(void)hipEventElapsedTime(&t.scan_ms, c->ev[1], c->ev[2]);
		if (with_emit) (void)hipEventElapsedTime(&t.emit_ms, c->ev[2], c->ev[3]);
	}
	if (c->timing_level > 0 && with_emit) (void)hipEventElapsedTime(&t.total_ms, c->ev[0], c->ev[3]);
	else if (c->timing_level > 1) (void)hipEventElapsedTime(&t.total_ms, c->ev[0], c->ev[2]);
	if (c->lane_presweeped && c->cur_lane && c->timing_level > 0 && c->cur_lane->many_pass >= 0) {
		// the sweep was made ahead of time, NI isovalues per pass: its share.  (The pass lies before this call's work on the same
		// stream, which fetch_counters has waited for: its events are complete)
		float ms = 0.f;
		if (hipEventElapsedTime(&ms, c->ev_many[c->cur_lane->many_pass][0], c->ev_many[c->cur_lane->many_pass][1]) == hipSuccess) {
			ms /= (float)c->cur_lane->many_ni;
			t.sweep_ms += ms;
			t.total_ms += ms;
		}
		// ... and of the tails made behind that pass, one launch of each kernel for its NI isovalues
		if (c->lane_pretailed && hipEventElapsedTime(&ms, c->ev_many[c->cur_lane->many_pass][1], c->ev_many[c->cur_lane->many_pass][2]) == hipSuccess) {
			ms /= (float)c->cur_lane->many_ni;
			t.scan_ms += ms;
			t.total_ms += ms;
		}
	}
}

// What every call that classifies the grid begins with: the device, the range, the last count forgotten, c->P / c->range / c->nsegs
// for this isovalue and range, the buffers of set 0
static int begin_call(mc33hip_ctx *c, double iso, const mc33hip_range *range, bool keep_emit = false) {
	int rc = use_device(c, keep_emit);
	if (rc) return rc;
	if ((rc = check_range(c, range))) return rc;
	c->counted = false;
	fill_params(c, iso, range);
	return ensure_workspaces(c);
}

// Count until it fits, for the calls that read the counters before they return: sweep and tail - with emit targets, the emit passes
// right behind them, which check the capacities of the targets on the device - then the counters, and again
//   - when the tail left the slow kernels out (alias_gate: enqueue_tail) and there were slow cells after all: a miss.  The counts
//     do not stand and the emit passes have refused (emit_prepare); the tail again, with the slow kernels - fetch_counters has noted
//     that the set has slow cells;
//   - when the records did not fit: nothing was emitted, the record arrays grow to what the counters ask for.
// A repeated round keeps the sweep's result (enqueue_count: rerun).
// A call that emits on a stream the caller named returns when its counts are known (returns_at_counts): the triangle pass hands
// counters and emit_skipped - the device's own verdict on capacity, record overflow and alias miss, the one every emit kernel
// reaches (emit_prepare) - to the host as it starts, and an extraction that fits leaves its emit passes to the stream
// (mc33hip_ctx::emit_queued, finish_pending_emit).  A round that does not fit has emitted nothing; the stream is drained as before.
// Where this departs from the plan it was built to (k_scan_apply publishes; emit_skipped in a pinned word of its own; the host
// decides the fit with a function it shares with emit_prepare):
//   - the counters are published by k_emit_fast_triangles.  No block of k_scan_apply has them all: the totals are written by its
//     last block, live_cursor and alias_cells by block 0, the ghost offsets by the block that holds the first emitted segment,
//     so publishing from there takes a grid-wide ticket - an atomic per block on one word, 2 045 of them at 1024^3 in a 12 us
//     kernel that everything behind it waits for.  The triangle pass already left the counters in h_ctr as its first wave starts;
//   - emit_skipped stays a word of h_ctr: that same wave writes the verdict of ITS emit_prepare there, in front of the sequence
//     word, so the host has the device's own decision when it has the counters and needs neither a second pinned word nor a
//     comparison of its own that could differ from the device's.
struct EmitTargets { void *dV, *dN, *dT; unsigned long long capV, capT; };
static bool returns_at_counts(const mc33hip_ctx *c) {
	// (the developer traces are read back through the null stream when the counters are there: fetch_counters)
	return c->stream_given && !c->own_stream && c->timing_level == 0 && !c->sw.trace_cells && !c->sw.trace_file;
}
static int count_until_fits(mc33hip_ctx *c, const EmitTargets *emit) {
	unsigned launches = 0;
	const bool early = emit && returns_at_counts(c);
	for (;;) {
		c->alias_gate = true;
		int rc = enqueue_count(c, launches > 0);
		c->alias_gate = false;
		if (rc) return rc;
		launches++;
		uint32_t seq = 0;
		if (early) seq = ++c->w->seq ? c->w->seq : ++c->w->seq;  // (never 0: no word asked for)
		if (emit && (rc = enqueue_emit(c, emit->dV, emit->dN, emit->dT, emit->capV, emit->capT, nullptr, nullptr, seq))) return rc;
		if ((rc = early ? wait_counters(c, seq) : fetch_counters(c))) return rc;
		const bool miss = c->w->alias_gated && c->w->h_ctr->alias_cells != 0u;
		const bool fits = c->w->h_ctr->entry_cursor <= c->w->entry_cap && !miss;
		if (early) {
			if (fits && !c->w->h_ctr->emit_skipped) __atomic_fetch_add(&c->emit_queued, 1u, __ATOMIC_ACQ_REL);
			else HIP_TRY(hipStreamSynchronize(c->stream));  // (nothing was emitted; what follows frees or reuses what the passes look at)
		}
		if (fits) break;
		if (c->w->h_ctr->entry_cursor > c->w->entry_cap && (rc = grow_entries(*c->w, c->w->h_ctr->entry_cursor))) return rc;
	}
	read_timing(c, emit != nullptr, launches);
	return 0;
}

extern "C" int mc33hip_count(mc33hip_ctx *c, double iso, const mc33hip_range *range, mc33hip_counts *out) {
	if (!c) return MC33HIP_EINVAL;
	// The same isovalue over the same range of the library's OWN copy of the grid, counted by the call before and not emitted yet
	// (size_of_isosurface and then calculate_isosurface of the value it asked about: what a viewer does to show the memory a
	// surface will take, reference MC:1892-1940 / 1816-1889): everything the count made is still there - nothing is streamed
	// again.  Only a COUNT is reused, once: an extraction repeated with the same isovalue does all its work again, like the
	// reference's.  Not for a caller's device buffer (mc33hip_adopt_device): its samples may have been rewritten without this
	// library knowing.  (The range is the one that count checked, and nothing here touches the device.)
	if (range && c->counted && c->count_unused && !c->async_count && c->owns_grid && c->timing_level == 0 && same_bits((real_t)iso, c->P.iso) && same_range(*range, c->range)) {
		c->range.id_base = range->id_base;
		return finish_counts(c, out);
	}
	int rc = begin_call(c, iso, range);
	if (rc) return rc;
	if ((rc = count_until_fits(c, nullptr))) return rc;
	if ((rc = finish_counts(c, out))) return rc;
	c->counted = true;
	c->count_unused = true;
	return MC33HIP_OK;
}

static int sweep_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *range, bool tails_ahead) {
	if (!c || !isos || n < 1 || n > MC33_LANES) return MC33HIP_EINVAL;
	if (int rc = begin_call(c, isos[0], range)) return rc;
	return enqueue_sweep_many(c, isos, n, tails_ahead);
}
extern "C" int mc33hip_sweep_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *range) { return sweep_many(c, isos, n, range, false); }
extern "C" int mc33hip_prepare_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *range) { return sweep_many(c, isos, n, range, true); }

extern "C" int mc33hip_set_inclined(mc33hip_ctx *c, const double *grd_A, const double *grd_Ai, int triangular) {
	if (!c) return MC33HIP_EINVAL;
	c->inclined = grd_A && grd_Ai;
	c->triangular = triangular != 0;
	if (c->inclined) { memcpy(c->grd_A, grd_A, sizeof c->grd_A); memcpy(c->grd_Ai, grd_Ai, sizeof c->grd_Ai); }
	c->counted = false;
	return MC33HIP_OK;
}

extern "C" int mc33hip_set_normal_neg(mc33hip_ctx *c, int on) {
	if (!c) return MC33HIP_EINVAL;
	c->normal_neg = on != 0;
	c->counted = false;
	return MC33HIP_OK;
}

extern "C" int mc33hip_set_timing(mc33hip_ctx *c, int level) {
	if (!c || level < 0 || level > 2) return MC33HIP_EINVAL;
	if (int rc = use_device(c)) return rc;  // (an emit still queued was enqueued without events)
	c->timing_level = level;
	return MC33HIP_OK;
}

extern "C" int mc33hip_set_id_base(mc33hip_ctx *c, unsigned int id_base) {
	if (!c || !c->counted) return MC33HIP_EINVAL;
	if ((uint64_t)id_base + c->counts.nV > 0xFFFFFFFFull) { set_err("vertex ids exceed 2^32-1"); return MC33HIP_EOVERFLOW; }
	c->range.id_base = id_base;
	return MC33HIP_OK;
}

extern "C" int mc33hip_emit(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT) {
	if (!c || !c->counted) { set_err("mc33hip_emit needs a successful mc33hip_count first"); return MC33HIP_EINVAL; }
	if (capV < c->counts.nV || capT < c->counts.nT) { set_err("output buffers too small"); return MC33HIP_ECAPACITY; }
	if ((c->counts.nV && (!dV || !dN)) || (c->counts.nT && !dT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	return enqueue_emit(c, dV, dN, dT, capV, capT);
}

// ---- a z-slab's count, exchange and emit without a host round trip in between (slabs.py: extract_slab) ----
extern "C" int mc33hip_count_async(mc33hip_ctx *c, double iso, const mc33hip_range *range) {
	if (!c) return MC33HIP_EINVAL;
	int rc = begin_call(c, iso, range);
	if (rc) return rc;
	if ((rc = enqueue_count(c, false))) return rc;
	memset(&c->counts, 0, sizeof c->counts);  // (not known on the host until mc33hip_count_finish)
	c->counted = true;
	c->async_count = true;
	return MC33HIP_OK;
}

extern "C" int mc33hip_counts_to_device(mc33hip_ctx *c, long long *device_dst) {
	if (!c || !c->counted || !device_dst) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(1), 0, c->stream, (const Counters *)c->w->d_ctr, c->ghost_segs, device_dst);
	HIP_TRY(hipGetLastError());
	return MC33HIP_OK;
}

extern "C" int mc33hip_bases_from_table(mc33hip_ctx *c, const long long *device_table, int stride, int rank, int concatenated) {
	if (!c || !device_table || stride < 2 || rank < 0) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if (!c->d_bases) HIP_TRY(hipMalloc(&c->d_bases, 3 * sizeof(unsigned long long)));
	hipLaunchKernelGGL(k_slab_bases, dim3(1), dim3(1), 0, c->stream, device_table, stride, rank, concatenated, c->d_bases);
	HIP_TRY(hipGetLastError());
	return MC33HIP_OK;
}

extern "C" int mc33hip_emit_at_device_bases(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT) {
	if (!c || !c->counted || !c->d_bases) { set_err("mc33hip_emit_at_device_bases needs a count and mc33hip_bases_from_table first"); return MC33HIP_EINVAL; }
	if (!dV || !dN || !dT) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	return enqueue_emit(c, dV, dN, dT, capV, capT, nullptr, c->d_bases);  // (capacities are checked on the device: emit_prepare)
}

extern "C" int mc33hip_count_finish(mc33hip_ctx *c, mc33hip_counts *out) {
	if (!c || !c->counted) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = fetch_counters(c))) return rc;
	c->async_count = false;
	if (c->w->h_ctr->entry_cursor > c->w->entry_cap) {  // the records did not fit: nothing was emitted; the synchronous path makes room
		const uint32_t need = c->w->h_ctr->entry_cursor;
		c->counted = false;
		if ((rc = grow_entries(*c->w, need))) return rc;
		set_err("work records did not fit (%u): repeat with mc33hip_count", need);
		return MC33HIP_ECAPACITY;
	}
	read_timing(c, false, 1);
	if ((rc = finish_counts(c, out))) return rc;
	if (c->w->h_ctr->emit_skipped) { set_err("output buffers too small: need %llu vertices, %llu triangles", c->counts.nV, c->counts.nT); return MC33HIP_ECAPACITY; }
	return MC33HIP_OK;
}

extern "C" int mc33hip_emit_download(mc33hip_ctx *c, void *dV, void *dN, void *dT, unsigned long long capV, unsigned long long capT,
                                     void *hV, void *hN, void *hT) {
	if (!c || !c->counted) { set_err("mc33hip_emit_download needs a successful mc33hip_count first"); return MC33HIP_EINVAL; }
	if (capV < c->counts.nV || capT < c->counts.nT) { set_err("output buffers too small"); return MC33HIP_ECAPACITY; }
	if ((c->counts.nV && (!dV || !dN || !hV || !hN)) || (c->counts.nT && (!dT || !hT))) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	const DownloadPlan dl{hV, hN, hT, (size_t)c->counts.nV * 3 * sizeof(real_t), (size_t)c->counts.nV * 12, (size_t)c->counts.nT * 12};
	return enqueue_emit(c, dV, dN, dT, capV, capT, &dl);
}

extern "C" int mc33hip_download_wait(mc33hip_ctx *c) {
	if (!c) return MC33HIP_EINVAL;
	if (use_device(c)) return MC33HIP_ERUNTIME;
	HIP_TRY(hipStreamSynchronize(c->copy));    // (ordered behind the passes by the events: the arrays are complete and on the host)
	HIP_TRY(hipStreamSynchronize(c->stream));  // (... and nothing of the emit is left running when the caller gets its surface)
	return prop_check(c);
}

extern "C" int mc33hip_extract(mc33hip_ctx *c, double iso, const mc33hip_range *range, void *dV, void *dN, void *dT,
                               unsigned long long capV, unsigned long long capT, mc33hip_counts *out) {
	if (!c) return MC33HIP_EINVAL;
	// The extraction before this one may still be emitting (it returned at its counts).  Over the same range on the same stream
	// this one is enqueued behind it as it is: no buffer of the context changes size between two extractions of one range, and
	// the host reads nothing of the set before this call's own counters arrive.  Anything else waits for the emit first.
	const bool keep_emit = emit_pending_now(c) && range && same_range(*range, c->range) && returns_at_counts(c);
	int rc = begin_call(c, iso, range, keep_emit);
	if (rc) return rc;
	const EmitTargets emit{dV, dN, dT, capV, capT};
	if ((rc = count_until_fits(c, &emit))) return rc;
	if ((rc = finish_counts(c, out))) return rc;
	c->counted = true;
	if (c->w->h_ctr->emit_skipped) { set_err("output buffers too small: need %llu vertices, %llu triangles", c->counts.nV, c->counts.nT); return MC33HIP_ECAPACITY; }
	return MC33HIP_OK;
}

extern "C" int mc33hip_last_timing(mc33hip_ctx *c, mc33hip_timing *t) {
	if (!c || !t) return MC33HIP_EINVAL;
	if (int rc = use_device(c)) return rc;
	if (c->timing_level == 0) {  // no events were recorded for the last call: zeros, not an older call's numbers
		c->emit_pending = false;
		c->timing.sweep_ms = c->timing.scan_ms = c->timing.emit_ms = c->timing.total_ms = 0.f;
	}
	if (c->emit_pending) {  // a separate mc33hip_emit: wait for it and add its time
		if (hipEventSynchronize(c->ev[3]) == hipSuccess) {
			(void)hipEventElapsedTime(&c->timing.emit_ms, c->ev[2], c->ev[3]);
			(void)hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[3]);
		}
		c->emit_pending = false;
	}
	*t = c->timing;
	return MC33HIP_OK;
}

// ---------------------------------------------------------------------------------------------------
// mc33hip_probe_read: what a plain read of the resident grid reaches on this device, in this process, on this buffer -
// the ceiling the sweep's `roofline.frac` is set beside ("of peak" and "of a measured read ceiling").
// Every 16-byte chunk once, nontemporal, nothing written.  The launch shape is the best of tools/read_ceiling_probe.hip
// (profiles/r04_read_ceiling_probe.txt): every block a CONTIGUOUS piece of the buffer, 16 loads in flight per lane - 7.1 - 7.2
// TB/s at any occupancy on a 4 GiB buffer, where a grid-stride loop over 8 blocks per CU (the first form of this probe) reaches
// 6.2 - 6.4 and flattered the sweep.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_probe_read(const u32x4_t *p, uint64_t n16, uint32_t *sink) {
	constexpr int U = 16;
	const uint64_t per = ((n16 + gridDim.x - 1) / gridDim.x + 255u) & ~(uint64_t)255, lo = (uint64_t)blockIdx.x * per, hi = lo + per < n16 ? lo + per : n16;
	u32x4_t acc = {0u, 0u, 0u, 0u};
	uint64_t i = lo + threadIdx.x;
	for (; i + (U - 1) * 256u < hi; i += U * 256u) {
		u32x4_t v[U];
#pragma unroll
		for (int k = 0; k < U; k++) v[k] = __builtin_nontemporal_load(p + i + k * 256u);
#pragma unroll
		for (int k = 0; k < U; k++) acc ^= v[k];
	}
	for (; i < hi; i += 256u) acc ^= __builtin_nontemporal_load(p + i);
	if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u && sink) atomicAdd(sink, 1u);  // (keeps the loads; the word is as likely as any other)
}

extern "C" int mc33hip_probe_read(mc33hip_ctx *c, int reps, float *ms_best, float *ms_median, unsigned long long *bytes) {
	if (!c || reps < 1 || reps > 64 || !c->d_grid) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	// (a grid the context does not own may be a strided view into a larger allocation: its last plane ends with its last row)
	const uint64_t nsamples = c->owns_grid ? (uint64_t)c->slice * c->desc.npz_resident
	                                       : (uint64_t)c->slice * (c->desc.npz_resident - 1u) + (uint64_t)c->pitch * (c->desc.npy - 1u) + c->desc.npx;
	const uint64_t nbytes = (nsamples * sizeof(sample_t)) & ~(uint64_t)15;
	if (nbytes < 64) return MC33HIP_EINVAL;
	const u32x4_t *p = (const u32x4_t *)(((uintptr_t)c->d_grid + 15u) & ~(uintptr_t)15);
	const uint64_t n16 = (nbytes - ((uintptr_t)p - (uintptr_t)c->d_grid)) / 16;
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_err("hipEventCreate failed"); return MC33HIP_ERUNTIME; }
	std::vector<float> t;
	for (int k = 0; k < reps + 1; k++) {  // (the first launch is a warm-up)
		(void)hipEventRecord(e0, c->stream);
		hipLaunchKernelGGL(k_probe_read, dim3((uint32_t)std::max(1, c->cus) * 4u), dim3(256), 0, c->stream, p, n16, (uint32_t *)nullptr);
		(void)hipEventRecord(e1, c->stream);
		if (hipEventSynchronize(e1) != hipSuccess) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); set_err("k_probe_read failed"); return MC33HIP_ERUNTIME; }
		float ms = 0.f;
		(void)hipEventElapsedTime(&ms, e0, e1);
		if (k) t.push_back(ms);
	}
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	std::sort(t.begin(), t.end());
	if (ms_best) *ms_best = t.front();
	if (ms_median) *ms_median = t[t.size() / 2];
	if (bytes) *bytes = n16 * 16ull;
	return MC33HIP_OK;
}

// ---- what the tests look at of the range table (include/mc33_hip.h); neither is on the path of an extraction ----
extern "C" int mc33hip_range_table(mc33hip_ctx *c, void *host_out, size_t bytes) {
	if (!c || !host_out) return MC33HIP_EINVAL;
	if (!c->ranges_valid || !c->d_ranges) { set_err("no range table (none built yet, dropped, or the grid is volatile)"); return MC33HIP_EINVAL; }
	const uint64_t n = (uint64_t)c->desc.npz_resident * ((c->desc.npy - 1u + 62u) / 63u) * ((c->desc.npx - 1u + SEG_CELLS - 1u) / SEG_CELLS);
	if (bytes != n * sizeof(RangeEntry)) { set_err("range table: %llu bytes, not %llu", (unsigned long long)(n * sizeof(RangeEntry)), (unsigned long long)bytes); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(host_out, c->d_ranges, bytes, hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}
extern "C" int mc33hip_sweep_skipped(mc33hip_ctx *c, unsigned long long *out /*[3]*/) {
	if (!c || !out) return MC33HIP_EINVAL;
	if (!c->skipped_tiles || !c->d_skipped) { set_err("no single-isovalue sweep at timing level >= 1 yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	uint32_t w[4];
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(w, c->d_skipped, sizeof w, hipMemcpyDeviceToHost));
	out[0] = c->skipped_tiles; out[1] = w[1]; out[2] = w[2];
	return MC33HIP_OK;
}
extern "C" int mc33hip_sweep_skipped_blocks(mc33hip_ctx *c, unsigned long long *out /*[3]*/) {
	if (!c || !out) return MC33HIP_EINVAL;
	if (!c->skipped_tiles || !c->d_skipped) { set_err("no single-isovalue sweep at timing level >= 1 yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	uint32_t w[8];
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(w, c->d_skipped, sizeof w, hipMemcpyDeviceToHost));
	out[0] = w[4]; out[1] = w[5]; out[2] = w[6];
	return MC33HIP_OK;
}
extern "C" int mc33hip_alias_cells(mc33hip_ctx *c, unsigned long long *out) {
	if (!c || !out) return MC33HIP_EINVAL;
	if (!c->counted || !c->w || !c->w->h_ctr) { set_err("no count yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	*out = c->w->alias_known ? c->w->alias_last : c->w->h_ctr->alias_cells;
	return MC33HIP_OK;
}
extern "C" int mc33hip_emit_shape(mc33hip_ctx *c, unsigned long long *out /*[8]*/) {
	if (!c || !out) return MC33HIP_EINVAL;
	if (!c->shape_set || !c->shape_set->h_ctr) { set_err("no emit yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));  // (the triangle pass of that emit has left the counters in h_ctr by now, if no count had)
	const Counters &h = *c->shape_set->h_ctr;
	out[0] = h.entry_cursor == 0xFFFFFFFFu ? 0u : h.entry_cursor; out[1] = h.slow_cursor; out[2] = h.batch_cursor;
	for (int k = 0; k < 5; k++) out[3 + k] = c->shape[k];
	return MC33HIP_OK;
}
extern "C" int mc33hip_tail_shape(mc33hip_ctx *c, unsigned long long *out /*[8]*/) {
	if (!c || !out) return MC33HIP_EINVAL;
	if (!c->counted || !c->w || !c->w->h_ctr) { set_err("no count yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	SlotGeom g;
	if (int rc = slot_geometry(c, g)) return rc;  // (c->P, c->range and c->nsegs are still those of the count: what enqueue_tail went by)
	HIP_TRY(hipStreamSynchronize(c->stream));
	const Counters &h = *c->w->h_ctr;
	const uint64_t nb = (c->nsegs + SCAN_CHUNK - 1) / SCAN_CHUNK;
	out[0] = g.nslots; out[1] = c->w->lc.n; out[2] = c->w->lc.shift;
	out[3] = nb; out[4] = scans_grouped(nb) ? 1u : 0u; out[5] = (g.nslots + SLOT_CHUNK - 1) / SLOT_CHUNK;
	out[6] = h.slow_cursor; out[7] = h.dirty_cursor;
	return MC33HIP_OK;
}
extern "C" int mc33hip_list_counts(mc33hip_ctx *c, unsigned int *slow, unsigned int *dirty, size_t n) {
	if (!c || !slow || !dirty || n > LIST_CHUNKS) return MC33HIP_EINVAL;
	if (!c->counted || !c->w || !c->w->lc.slow_cnt) { set_err("no count yet"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (n) {
		HIP_TRY(hipMemcpy(slow, c->w->lc.slow_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(dirty, c->w->lc.dirty_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	}
	return MC33HIP_OK;
}
extern "C" int mc33hip_range_blocks(mc33hip_ctx *c, void *host_out, size_t bytes) {
	if (!c || !host_out) return MC33HIP_EINVAL;
	if (!c->ranges_valid || !c->blocks_made || !c->d_blocks) { set_err("no block table (no range table yet, dropped, the grid is volatile, or MC33_HIP_BLOCKS=0)"); return MC33HIP_EINVAL; }
	const uint64_t n = (uint64_t)c->desc.npz_resident * ((c->desc.npy - 1u + 62u) / 63u) * ((c->desc.npx - 1u + SEG_CELLS - 1u) / SEG_CELLS) * RANGE_BLOCKS;
	if (bytes != n * sizeof(RangeEntry)) { set_err("block table: %llu bytes, not %llu", (unsigned long long)(n * sizeof(RangeEntry)), (unsigned long long)bytes); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(host_out, c->d_blocks, bytes, hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}
extern "C" int mc33hip_block_words(mc33hip_ctx *c, void *host_out, size_t bytes) {
	if (!c || !host_out) return MC33HIP_EINVAL;
	if (!c->ranges_valid || !c->blocks_made || !c->d_blockw) { set_err("no sweep has left blocks out yet"); return MC33HIP_EINVAL; }
	const uint64_t n = (uint64_t)c->desc.npz_resident * ((c->desc.npy - 1u + 62u) / 63u) * ((c->desc.npx - 1u + SEG_CELLS - 1u) / SEG_CELLS);
	if (bytes != n * 8u) { set_err("block verdicts: %llu bytes, not %llu", (unsigned long long)(n * 8u), (unsigned long long)bytes); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(host_out, c->d_blockw, bytes, hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}

// ---- ... and of the plan and the live list (tests/test_gpu_sweep_refill.py, tools/trace_sweep.py) ----
extern "C" int mc33hip_sweep_plan(mc33hip_ctx *c, unsigned int *tiles_out, size_t cap_tiles, unsigned long long *info /*[3]*/) {
	if (!c || !info) return MC33HIP_EINVAL;
	const SweepPlan &pl = c->plan[c->cur_plan];
	if (!pl.d_tiles || !pl.key.ze) { set_err("no sweep plan yet"); return MC33HIP_EINVAL; }
	info[0] = pl.ntiles; info[1] = c->resident_blocks; info[2] = c->cur_plan ? 1ull : 0ull;  // (sized or not: the plan with a table)
	if (!tiles_out) return MC33HIP_OK;
	if (cap_tiles < pl.ntiles) { set_err("sweep plan: %llu tiles, room for %llu", (unsigned long long)pl.ntiles, (unsigned long long)cap_tiles); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(tiles_out, pl.d_tiles, pl.ntiles * sizeof(SweepTile), hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}
extern "C" int mc33hip_sweep_plan_weight(mc33hip_ctx *c, double *out) {
	if (!c || !out) return MC33HIP_EINVAL;
	const SweepPlan &pl = c->plan[c->cur_plan];
	if (!pl.d_tiles || !pl.key.ze) { set_err("no sweep plan yet"); return MC33HIP_EINVAL; }
	*out = pl.key.weight;
	return MC33HIP_OK;
}
extern "C" int mc33hip_sweep_packed(mc33hip_ctx *c, unsigned int *out, size_t cap_entries, unsigned long long *info /*[3]*/) {
	if (!c || !info) return MC33HIP_EINVAL;
	if (!c->live_blocks || !c->d_packed) { set_err("the last sweep went by no live list"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	uint32_t h[4] = {0u, 0u, 0u, 0u};
	HIP_TRY(hipMemcpy(h, c->d_packed, sizeof h, hipMemcpyDeviceToHost));
	info[0] = h[0]; info[1] = h[1]; info[2] = h[2];
	if (!out) return MC33HIP_OK;
	if (h[0] > c->live_blocks || cap_entries < h[0]) { set_err("packed live list: %u entries of %llu blocks, room for %llu", h[0], (unsigned long long)c->live_blocks, (unsigned long long)cap_entries); return MC33HIP_EINVAL; }
	if (h[0]) HIP_TRY(hipMemcpy(out, c->d_packed + 4, (size_t)h[0] * 16u, hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}
extern "C" int mc33hip_sweep_live(mc33hip_ctx *c, unsigned int *live_out, size_t cap_entries, unsigned long long *info /*[2]*/) {
	if (!c || !info) return MC33HIP_EINVAL;
	if (!c->live_blocks || !c->d_live) { set_err("the last sweep went by no live list"); return MC33HIP_EINVAL; }
	if (int rc = use_device(c)) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	uint32_t n = 0;
	HIP_TRY(hipMemcpy(&n, c->d_live, sizeof n, hipMemcpyDeviceToHost));
	info[0] = n; info[1] = c->live_blocks;
	if (!live_out) return MC33HIP_OK;
	if (n > c->live_blocks || cap_entries < n) { set_err("live list: %u entries of %llu blocks, room for %llu", n, (unsigned long long)c->live_blocks, (unsigned long long)cap_entries); return MC33HIP_EINVAL; }
	if (n) HIP_TRY(hipMemcpy(live_out, c->d_live + 1, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}

#ifdef MC33_DEV
extern "C" int mc33hip_debug_words(mc33hip_ctx *c, unsigned int *out /*[8]*/) {  // what a guarded kernel found wrong (developer builds)
	if (!c || !out) return MC33HIP_EINVAL;
	HIP_TRY(hipStreamSynchronize(c->stream));
	HIP_TRY(hipMemcpy(out, (const char *)c->w->d_ctr + offsetof(Counters, debug), 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return MC33HIP_OK;
}
#endif

extern "C" int mc33hip_synchronize(mc33hip_ctx *c) {
	if (!c) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	return prop_check(c);
}

extern "C" int mc33hip_download_many(mc33hip_ctx *c, int n, void *const *dst, const void *const *src, const size_t *bytes, int concurrent) {
	if (!c || n < 0 || (n && (!dst || !src || !bytes))) return MC33HIP_EINVAL;
	if (use_device(c)) return MC33HIP_ERUNTIME;  // (the concurrent form may come from another thread; the copy stream is not ordered behind an emit still queued)
	hipStream_t st = concurrent ? c->copy : c->stream;
	for (int k = 0; k < n; k++) {
		if (!bytes[k]) continue;
		if (!dst[k] || !src[k]) return MC33HIP_EINVAL;
		if (hipMemcpyAsync(dst[k], src[k], bytes[k], hipMemcpyDeviceToHost, st) != hipSuccess) { (void)hipStreamSynchronize(st); return MC33HIP_ERUNTIME; }
	}
	if (hipStreamSynchronize(st) != hipSuccess) return MC33HIP_ERUNTIME;
	return concurrent ? MC33HIP_OK : prop_check(c);  // (the side stream says nothing about the sampling kernels on the context's own)
}

extern "C" int mc33hip_download_concurrent(mc33hip_ctx *c, void *dst, const void *src, size_t bytes) {
	if (!c || (bytes && (!dst || !src))) return MC33HIP_EINVAL;
	if (!bytes) return MC33HIP_OK;
	if (use_device(c)) return MC33HIP_ERUNTIME;  // (may be another thread than the context's; as above)
	if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->copy) != hipSuccess) return MC33HIP_ERUNTIME;
	return hipStreamSynchronize(c->copy) == hipSuccess ? MC33HIP_OK : MC33HIP_ERUNTIME;
}

extern "C" int mc33hip_download(mc33hip_ctx *c, void *dst, const void *src, size_t bytes) {
	if (!c || (bytes && (!dst || !src))) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if (!bytes) return MC33HIP_OK;
	HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return prop_check(c);
}

extern "C" int mc33hip_device_alloc(mc33hip_ctx *c, void **dptr, size_t bytes) {
	if (!c || !dptr) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	*dptr = nullptr;
	HIP_TRY(hipMalloc(dptr, bytes ? bytes : 16));
	return MC33HIP_OK;
}

extern "C" int mc33hip_device_free(mc33hip_ctx *c, void *dptr) {
	if (!c) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	HIP_TRY(hipFree(dptr));
	return MC33HIP_OK;
}
