// mc33_sweep_plan.h -- everything about a sweep's plan that needs no device, as plain functions over plain data (no HIP type, no
// context): the tiles and boundaries of a plan (plan_tiles), what names a plan (PlanKey, PlanRef, plan_slot), and the policy of
// the sweeps with a range table (TablePolicy: which plan, what size, who gets a list).  Included by mc33_kernels.hip (through
// mc33_records.hip.h) and by host programs (tests/sweep_plan_host.cpp, tests/sweep_pack_host.cpp).
#ifndef MC33_SWEEP_PLAN_H
#define MC33_SWEEP_PLAN_H
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

// One block of k_sweep: the 4 row segments of group xg, the 63 cell rows of y tile yt, cell slices [z_lo, z_hi).
// The host cuts every (xg, yt) column into chunks of equal WORK (rows x planes), as many in total as the
// GPU holds blocks at once: waves of one SIMD are served oldest first, so a CU that got one block more
// than the others ends that much later, and short tiles (the last y tile) get deeper chunks.
struct SweepTile { uint32_t seg, yt, z_lo, z_hi; };  // the piece of the volume ONE WAVE of k_sweep streams: row segment, y tile, planes
struct TileBoundary { uint32_t below, above, z, yt, seg, pad_[3]; };  // tile (wave) indices of k_sweep; slice z (k_boundary)

// ---- the cost of a wave's life ---------------------------------------------------------------------------------------------------------
// A wave streams one tile: a run of planes of one column (row segment x y tile).  Its life is a sum over its planes, of the
// batches of sample rows it waits for and of work that does not depend on the rows - plane completion, the mailbox barrier of
// a grouped block, the block-word loads:  life ~ a x batches + b x planes  (profiles/r12_plan_balance.txt A).  b / a is the
// WEIGHT OF A PLANE IN BATCHES.  For a sweep that streams every block of a live tile the batches carry the life and the weight
// is 0: columns are cut into equal numbers of batches.  Where dead blocks are left out a batch of a dead quarter costs no memory
// access and the plane term weighs: a column of few rows (the last y tile) cut to the batches of a full one is several times as
// many planes deep and ends last.
struct PlanFrac { double f; uint64_t col; };

// Chunks (z pieces) per column of a plan of B wave tiles.  Column i has waves[i] waves (its segments) of w[i] work per plane
// each - batches, or batches + the weight of a plane, in any one unit - and gets the share B x w[i] / W of the chunks, W = sum of
// w[i] x waves[i]: at least one chunk, at most nzc (a chunk is at least one plane), the fractions rounded down and the remainder
// dealt one chunk each to the columns with the largest fractions until the tiles are B.  frac: room for ncol entries.
// Returns the tiles: sum of chunks[i] x waves[i].
static inline uint64_t plan_shares(const double *w, const uint32_t *waves, uint64_t ncol, uint64_t B, uint32_t nzc, uint32_t *chunks, PlanFrac *frac) {
	double W = 0;
	for (uint64_t i = 0; i < ncol; i++) W += w[i] * waves[i];
	uint64_t total = 0;
	for (uint64_t i = 0; i < ncol; i++) {
		const double share = (double)B * w[i] / W;
		const uint32_t n = (uint32_t)std::min<double>(std::max(1.0, std::floor(share)), (double)nzc);
		chunks[i] = n; total += (uint64_t)n * waves[i];
		frac[i] = PlanFrac{share - std::floor(share), i};
	}
	std::sort(frac, frac + ncol, [](const PlanFrac &x, const PlanFrac &y) { return x.f > y.f; });
	for (uint64_t k = 0; k < ncol && total < B; k++)
		if (chunks[frac[k].col] < nzc) { chunks[frac[k].col]++; total += waves[frac[k].col]; }
	return total;
}

// The work of a column per plane that plan_shares is given: its batches alone (in sample rows: `rows`, whole batches of
// rows_per_batch), or with the weight of a plane, which is counted in batches.
static inline double plan_column_weight(double rows, uint32_t rows_per_batch, double plane_weight) {
	return plane_weight > 0.0 ? rows + plane_weight * (double)rows_per_batch : rows;
}

// ---- the columns of a grid -------------------------------------------------------------------------------------------------------------
// What a plan needs to know of the grid: cells in y, row segments (256 cells in x), and the sample rows of one batch - 4 rows of
// float samples, 8 / 16 of packed ushort / uchar ones (4 x SWEEP_PACK).
struct PlanGrid { uint32_t ny, nseg, rows_per_batch; };
static inline uint32_t plan_y_tiles(const PlanGrid &g) { return (g.ny + 62u) / 63u; }
// work of one WAVE of y tile yt per slice: its sample rows
// (in whole BATCHES of sample rows: a wave's time is the
// number of batches it waits for, and a y tile of 2 rows costs a batch per plane like one of 4.  Counted in rows, the
// 2-row last y tile of a 128^3 grid got pieces twice as deep as its time allows and the sweep took 0.060 ms where the
// 256^3 one takes 0.035: VERDICT r4 weak 12)
static inline double column_work(const PlanGrid &g, uint32_t yt) {
	return (double)((std::min(64u, g.ny + 1 - yt * 63u) + g.rows_per_batch - 1u) / g.rows_per_batch * g.rows_per_batch);
}
// the tiles the slices [zs, ze) would make at ONE plane per tile: the work of all waves x slices / 64 rows (what plan_tiles divides by a depth)
static inline double sweep_unit(const PlanGrid &g, uint32_t zs, uint32_t ze) {
	double W = 0;
	for (uint32_t yt = 0; yt < plan_y_tiles(g); yt++) W += column_work(g, yt) * g.nseg;
	return W * (ze - zs) / 64.0;
}
// A tile is what ONE wave streams: a row segment (256 samples in x) x a y tile (64 sample rows) x a run of planes.
// Planning is done per group of up to 4 neighbouring segments (they read the same 4 KiB rows and are launched
// side by side), but every wave gets a tile of its own, so a group with fewer than 4 segments (grids that are
// not a multiple of 1024 samples wide, narrow grids) does not leave the waves of a block idle.
// The columns (groups), y tile major: w, the work of one WAVE of the group per slice, and its waves.  Returns the work of all waves.
static inline double plan_columns(const PlanGrid &g, std::vector<double> &w, std::vector<uint32_t> &waves) {
	const uint32_t nXG = (g.nseg + 3) / 4, nYT = plan_y_tiles(g);
	w.resize((uint64_t)nXG * nYT); waves.resize(w.size());
	double W = 0;
	for (uint32_t yt = 0; yt < nYT; yt++)
		for (uint32_t xg = 0; xg < nXG; xg++) {
			const uint64_t i = (uint64_t)yt * nXG + xg;
			waves[i] = std::min(4u, g.nseg - xg * 4);
			w[i] = column_work(g, yt);
			W += w[i] * waves[i];
		}
	return W;
}

// ---- what names a plan -----------------------------------------------------------------------------------------------------------------
// Block plan of k_sweep for cell slices [zs, ze): every (segment group, y tile) column is cut along z into
// chunks of about equal work (sample rows x waves x planes; a chunk re-reads one plane, so they are kept
// about `depth` slices deep), and the number of chunks is a whole multiple of what the device holds at
// once whenever the grid is large enough.  Measured on MI355X at 1024^3: with 1088 equal tiles on 256 CUs
// the 64 CUs that got a fifth block finished 12 % after the others.
//
// Two plans are kept: 0, for a sweep without a range table, is about
// SWEEP_DEPTH slices deep - one tile per wave slot of the device, one round; 1, for a sweep with one, about SWEEP_DEPTH_TABLE.  With a table
// most tiles of a smooth field are dead and never streamed (k_tile_verdicts), and the live ones have to fill the device by
// themselves: the plan is several rounds of the resident set, k_sweep's live blocks come first in the launch, and the hardware
// hands a freed slot to the next of them.  An explicit MC33_HIP_RZ is the depth of both, which are then one plan (number 0);
// MC33_HIP_RZ_TABLE is the depth of plan 1 alone (the tests make the two differ on small grids with it, the profiles try depths).
// A lane swept ahead keeps a PlanRef to its plan, and its tail asks for that plan again: the plan is a function
// of the range, the depth and the device, so a plan made again for a range is the plan the lane's edge records are indexed by.
// target (plan 1 only; 0: none): the number of tiles wanted, in place of a depth - what table_retarget makes of the live tiles the
// sweeps find, so that the packed live blocks are a set share of ONE round of the device.  The chunks are shared out as for a depth, only the
// sum is no whole number of rounds: dead tiles cost nothing.  A sized plan has a slot of its own, number 2 (plan 1
// with a target), so that a caller who mixes single-isovalue calls (sized) with passes over several isovalues (the default
// depth, slot 1) has both resident and makes neither again.  A lane keeps the slot and the target (PlanRef).
// weight (sized plans only; 0: none): the weight of a plane in batches the columns are cut by (above).  Equal numbers
// of BATCHES per tile make equal lives while the batches carry a wave's life.  A sweep that leaves dead blocks out pays for a batch
// of a dead quarter with no memory access, and what it does once per plane weighs about PLANE_WEIGHT_BLOCKS batches
// (profiles/r12_plan_balance.txt A): cut by batches alone, the tiles of a short last y tile - 4 batches per plane where the others
// have 16 - were four times as deep as the others and ended last, 246 us into a kernel whose median wave lived 159
// (profiles/r11_block_skip.txt E).  So the share of a column of such a plan goes by batches + weight per plane; the sum stays the
// target, and sweep_unit and table_target's cap stay counted in batches.  The weight is that of a single-isovalue sweep of a
// context that leaves blocks out (sweep_plane_weight: decided by the build, MC33_HIP_BLOCKS and the width of the grid - things
// fixed when the context is made, never by whether a block table happens to exist); every other plan, and every plan of the
// double and integer libraries, is cut by batches as before.  It is part of what names a plan: the key holds it beside the
// target, a lane keeps it there too, and the functions below compare it wherever they compare the target.
constexpr uint32_t SWEEP_DEPTH = 16u, SWEEP_DEPTH_TABLE = 5u;  // (measured, 1024^3 float: profiles/r09_sweep_refill.txt A, B)
constexpr double PLANE_WEIGHT_BLOCKS = 3.0;  // b / a of k_sweep_live_blocks: 2.4 fitted on the plan cut by batches, 3.3 on one cut with 3 (profiles/r12_plan_balance.txt A)

// target - plan 1: the tile count it was asked for in place of a depth (table_retarget), 0: by its depth; weight: of a plane in
// batches its columns were cut by, 0: by batches alone
struct PlanKey { uint32_t zs, ze, depth, target; double weight; };
static inline bool operator==(const PlanKey &a, const PlanKey &b) { return a.zs == b.zs && a.ze == b.ze && a.depth == b.depth && a.target == b.target && a.weight == b.weight; }
// What a lane keeps of the plan it was swept by: slot and target make the plan again, with the weight it was cut with.
struct PlanRef { int slot; uint32_t target; double weight; };
// does a slot that holds `held` still hold the plan a lane was swept by, for the range [zs, ze)?  (The depth is not asked: it
// is a function of the slot and of switches read once.)
static inline bool plan_is_lanes(const PlanKey &held, const PlanRef &r, uint32_t zs, uint32_t ze) { return held.zs == zs && held.ze == ze && held.target == r.target && held.weight == r.weight; }
// is `held` the plan whose tile count a published count is to be scaled to (table_retarget)?  Deliberately not ==: the depth is
// the slot's and says nothing here, and a plan without a target was cut by batches whatever the sweep's own weight is - asking
// its weight would take every default plan of a context that leaves blocks out for another plan.
static inline bool plan_is_sized_as(const PlanKey &held, uint32_t zs, uint32_t ze, uint32_t target, double weight) { return held.zs == zs && held.ze == ze && held.target == target && (!target || held.weight == weight); }
// The slot and the key of the plan a caller asks for: `table` - the plan of a sweep with a range table (1; a PlanRef's slot 1 or
// 2) or without (0) - with the target and weight that come with it, under the depth switches.
struct PlanSlot { int slot; PlanKey key; };
static inline PlanSlot plan_slot(bool table, uint32_t zs, uint32_t ze, uint32_t target, double weight, uint32_t rz, uint32_t rz_table) {
	if (rz && !rz_table) table = false;   // (one depth for both: one plan)
	if (!table) target = 0u;
	if (!target || !(weight > 0.0)) weight = 0.0;
	const uint32_t depth = table ? (rz_table ? rz_table : SWEEP_DEPTH_TABLE) : (rz ? rz : SWEEP_DEPTH);
	return PlanSlot{table ? (target ? 2 : 1) : 0, PlanKey{zs, ze, depth, target, weight}};
}

// ---- the tiles of a plan ---------------------------------------------------------------------------------------------------------------
// tiles in launch order and the pairs of tiles that meet in z, for key.target tiles or, without a target, for tiles key.depth
// slices deep in whole rounds of the device (4 x resident_blocks wave slots).  total: what plan_shares dealt.  False: more
// tiles than one launch takes.
static inline bool plan_tiles(const PlanGrid &g, const PlanKey &key, uint32_t resident_blocks, uint32_t min_depth, std::vector<SweepTile> &tiles, std::vector<TileBoundary> &bounds, uint64_t &total) {
	const uint32_t nXG = (g.nseg + 3) / 4, nYT = plan_y_tiles(g), nzc = key.ze - key.zs;
	std::vector<double> w; std::vector<uint32_t> waves;
	const double W = plan_columns(g, w, waves);
	const uint64_t ncol = w.size();
	// wave tiles wanted: W * nzc / (64 * depth), rounded to whole rounds of the resident set
	const double pref = W * nzc / (64.0 * key.depth);
	uint64_t B = (uint64_t)resident_blocks * 4;
	if (key.target) B = key.target;
	else if (pref >= (double)B) B *= (uint64_t)(pref / (double)B + 0.5);
	else B = std::max<uint64_t>(1, std::min<uint64_t>(B, (uint64_t)(W * nzc / (64.0 * std::max(1u, min_depth)))));  // small grid: fill the GPU, tiles down to one plane deep (k_boundary then does the slices)
	std::vector<uint32_t> chunks(ncol); std::vector<PlanFrac> frac(ncol);  // chunks: z pieces of the group (each is one tile per wave of the group)
	if (key.weight > 0.0)  // (a plane's own cost on top of its batches)
		for (uint64_t i = 0; i < ncol; i++) w[i] = plan_column_weight(w[i], g.rows_per_batch, key.weight);
	total = plan_shares(w.data(), waves.data(), ncol, B, nzc, chunks.data(), frac.data());
	if (total > 0x3FFFFFFFull) return false;
	struct Planned { SweepTile t; uint64_t col; };  // col: the wave's column (yt, seg)
	std::vector<Planned> planned; planned.reserve(total);
	for (uint64_t i = 0; i < ncol; i++)
		for (uint32_t k = 0; k < chunks[i]; k++) {
			const uint32_t lo = key.zs + (uint32_t)((uint64_t)nzc * k / chunks[i]), hi = key.zs + (uint32_t)((uint64_t)nzc * (k + 1) / chunks[i]);
			if (hi <= lo) continue;
			const uint32_t yt = (uint32_t)(i / nXG), xg = (uint32_t)(i % nXG);
			for (uint32_t sgm = xg * 4; sgm < xg * 4 + waves[i]; sgm++)
				planned.push_back(Planned{SweepTile{sgm, yt, lo, hi}, (uint64_t)yt * g.nseg + sgm});
		}
	// launch order: by depth first, so that waves running together read neighbouring memory (the segments of a group
	// stay next to each other: the sort is stable)
	std::stable_sort(planned.begin(), planned.end(), [](const Planned &x, const Planned &y) { return x.t.z_lo < y.t.z_lo; });
	tiles.resize(planned.size()); bounds.clear();
	std::vector<uint32_t> below((uint64_t)nYT * g.nseg, 0xFFFFFFFFu);  // the tile of the column that ends where the next one begins
	for (uint32_t b = 0; b < planned.size(); b++) {   // (ascending z_lo: a column's tiles come in order)
		const SweepTile &t = planned[b].t;
		tiles[b] = t;
		if (below[planned[b].col] != 0xFFFFFFFFu) bounds.push_back(TileBoundary{below[planned[b].col], b, t.z_lo, t.yt, t.seg, {0, 0, 0}});
		below[planned[b].col] = b;
	}
	return true;
}

// ---- the size of the plan --------------------------------------------------------------------------------------------------------------
// A sweep with a table streams its live tiles only, and a block keeps its four wave slots for the life of a tile: the kernel's
// length is a whole number of rounds of the resident set times that life.  So the plan is asked for as many tiles as make the
// PACKED live blocks - ceil(live / 4) - the share `fill` of one round of the device.  The live share of a field hardly depends on
// the size of the plan, so the count one sweep published (`live` of `tiles`) predicts the live tiles of a plan of another size:
//   target = fill * 4 * resident_blocks * tiles / live,
// but never more tiles than are `min_depth` planes deep: `unit` is the number of tiles the range would have at a depth of one
// plane, and the target is cut to unit / min_depth.  (A cut plan has FEWER packed blocks than a round, never more: one round is
// always enough, and there is no case for a second.)  And never fewer tiles than one round, 4 * resident_blocks: a plan below
// that gets no list, so no count would ever size it again.  0: no count, nothing to go by.
static inline uint32_t table_target(uint64_t live, uint64_t tiles, uint32_t resident_blocks, double unit, double min_depth, double fill) {
	if (!live || !tiles || !resident_blocks) return 0u;
	double t = fill * 4.0 * (double)resident_blocks * (double)tiles / (double)live;
	const double cap = unit / (min_depth > 0.0 ? min_depth : 1.0);
	if (t > cap) t = cap;
	if (t < 4.0 * (double)resident_blocks) t = 4.0 * (double)resident_blocks;
	if (t > 1073741823.0) t = 1073741823.0;
	return t < 1.0 ? 1u : (uint32_t)t;
}
// A plan is kept while the packed blocks its sweeps find stay inside a band around the target: lo .. hi of the resident blocks.
// hi is never above 1: a block more than the device holds costs a whole tile's life (the caller's band ends well below).
static inline int table_keeps(uint64_t live, uint32_t resident_blocks, double lo, double hi) {
	const double packed = (double)((live + 3u) / 4u), r = (double)resident_blocks;
	return packed >= lo * r && packed <= hi * r;
}

// ---- which fill and band a sized plan goes by -----------------------------------------------------------------------------------------
// {fill, band lo, band hi} of table_target / table_keeps.  `plain` are the constants every sized plan went by before plans were
// weighted (TABLE_FILL, TABLE_BAND_LO, TABLE_BAND_HI); `balanced` a second set for plans cut with a plane weight, read off a size
// curve that was measured at the device's default residency and nowhere else - so it holds only for a weighted plan of a context
// whose residency nobody forced (MC33_HIP_SWEEP_BLOCKS_PER_CU not set).  A band never ends above one round (table_keeps).
struct TableBand { double fill, lo, hi; };
static inline TableBand table_band(double plane_weight, bool forced_residency, TableBand plain, TableBand balanced) {
	if (!(plane_weight > 0.0) || forced_residency) return plain;
	if (balanced.hi > 1.0) balanced.hi = 1.0;
	return balanced;
}

// ---- the policy of the sweeps with a table ---------------------------------------------------------------------------------------------
// A small state machine over the word k_live_compact published last (live tiles << 32 | tiles << 1 | plan; 0: nothing yet) and
// this state.  The caller reads the word, as it stands - of the last sweep or of one or two before it; nobody waits for it.
//   coarse          sweeps with a table go by plan 0 for now: the last ones left too little out for the finer plan to pay (table_plan)
//   coarse_sweeps   ... sweeps made that way since (table_wants_list: one in 16 goes by a list)
//   target          the tile count plan 1 is asked for (table_retarget), 0: its default depth
//   pending         ... and the one the last call would have asked for instead: replaced when the next call agrees
struct TablePolicy { bool coarse; uint32_t coarse_sweeps, target, pending; };
static_assert(sizeof(PlanKey) == 24 && sizeof(PlanRef) == 16 && sizeof(TablePolicy) == 16, "the context's layout is measured: mc33_context.hip.h");
// What the policy is told of the context and of the range about to be swept.
//   unit                       sweep_unit of the range
//   resident_blocks, min_depth k_sweep blocks the device holds at once; MC33_HIP_MIN_DEPTH
//   weight                     the weight of a plane this context's sized plans are cut with (sweep_plane_weight)
//   forced_residency           MC33_HIP_SWEEP_BLOCKS_PER_CU is set
//   rz, rz_table, table_tiles  MC33_HIP_RZ, MC33_HIP_RZ_TABLE, MC33_HIP_TABLE_TILES
//   live                       MC33_HIP_LIVE: 1 / 0 always / never a list, -1 the policy decides
//   plan_tiles                 tiles of the plan in force - table_retarget: of the plan the policy's target names, 0 when the slot holds another
//   plan_sized                 ... and whether it is a sized plan (slot 2)
struct TableFacts { double unit; uint32_t resident_blocks, min_depth; double weight; bool forced_residency; uint32_t rz, rz_table, table_tiles; int live; uint64_t plan_tiles; bool plan_sized; };

// Which plan a sweep with a table goes by: 1, the finer one, unless the sweeps say it does not pay.  A finer plan is a gain by the
// slots dead tiles free for live ones, and a loss by its per-tile start and end and three times the boundaries.  Measured at 1024^3
// float (profiles/r09_sweep_refill.txt C, D): 63 % of the one-round plan's tiles dead, 12 % faster; nothing dead, 5 - 8 % slower; between
// the two, taken as linear in the dead share, they break even near four tiles in five live.  So: a sweep by the finer plan that
// found more than 90 % of its tiles live sends the following ones to plan 0, the one-round plan (with the table and its list all
// the same), and a sweep by plan 0 that found fewer than 75 % live sends them back.  The finer plan never has the larger live share of
// the two, so a field stays where it was sent.  New samples start from the finer plan (table_forget).
static inline int table_plan(TablePolicy &p, unsigned long long word) {
	const uint64_t tiles = (word & 0xFFFFFFFFull) >> 1, live = word >> 32;
	if (tiles) {
		if ((word & 1ull) && live * 100 > tiles * 90) { p.coarse_sweeps = p.coarse ? p.coarse_sweeps : 0u; p.coarse = true; }
		else if (!(word & 1ull) && live * 100 < tiles * 75) p.coarse = false;
	}
	return p.coarse ? 0 : 1;
}
// How many tiles the finer plan is asked for (p.target; 0: its default depth).  The packed live blocks of a sweep are
// ceil(live tiles / 4) (k_live_compact), and the kernel's length is a whole number of rounds of the resident set times the life of
// a tile: the plan is sized so that they are LESS than one round - TABLE_FILL of the resident blocks (table_target) - from the
// count the last sweep by plan 1 published; the live share hardly depends on the size of the plan.  A
// new plan costs a wait for the stream and two copies (plan_sweep), so the plan stays while the count says its packed blocks lie
// between TABLE_BAND_LO and TABLE_BAND_HI of a round.  Tiles are never asked shallower than TABLE_MIN_DEPTH planes; a grid whose
// default plan is shallower than that already - cut down to MC33_HIP_MIN_DEPTH to make one round at all - goes by that depth
// instead.
// The constants are read off the measured curve of the flagship, profiles/r10_sweep_pack.txt C, D: every size between 0.63 and
// 0.73 of a round (7 168 - 8 350 tiles) takes 0.572 - 0.580 ms per step against the parent's 0.60 - 0.61, the sizes between 0.75
// and 0.81 (8 564 - 9 216) are SLOWER than the parent (a tail of late tiles at a regular spacing in z, not understood), a full
// round (0.91: 10 400) gains 1 %, 0.95 - 1.0 gain 3 %, and past one round the gain is gone.  So the fill is 0.68 and the band
// ends at 0.72, a margin short of the sizes that lose while their cause is not known.  Nothing shallower than 3.4 planes was measured.
// Never fewer tiles than ONE ROUND (4 x resident blocks; table_target): with more than 0.68 of its tiles live a plan would be
// asked for less, the sweep would go without a list (table_wants_list), nothing would publish a count again, and the context would sit
// on that plan whatever isovalue came next.  For the same reason a sized plan always gets its list.
// Left alone: an explicit MC33_HIP_RZ / MC33_HIP_RZ_TABLE, plans of less than one round (small grids), sweeps by plan 0, no count
// yet (new samples: table_forget).  MC33_HIP_TABLE_TILES forces a target: it is for tests and curves, comes before
// MC33_HIP_RZ_TABLE and holds for small plans too; only MC33_HIP_RZ alone, which makes the two plans one, comes before it.
// Two calls in a row have to ask for about the same size (5 %) before the plan is replaced: a caller that moves between isovalues
// with very different live shares would otherwise pay for a new plan in every call - 0.31 -> 0.52 ms per count at 1024^3 with the
// isovalues 0 and 1.5 alternated (profiles/r10_sweep_pack.txt F) - and now stays on the plan it has.
// Those constants hold for plans cut by batches alone and for every context whose residency is forced.  Cut to the batches of a
// full y tile, the tiles of a short last one are several times as many planes deep, and with blocks left out a plane costs about
// three batches' worth of time whatever its rows: they ended last.  A plan cut with that weight has no such tail and
// gains most right below one round, so it goes by a second fill and band (TABLE_FILL_BALANCED below; table_band makes the
// choice).  (The sizes at 0.75 - 0.81 of a round are still 0.01 ms behind 0.68 with the balanced cut,
// profiles/r12_plan_balance.txt B: the deep tiles were not the whole of that loss.)
// Only the single-isovalue calls are sized (enqueue_count).  The passes of mc33hip_sweep_many / mc33hip_prepare_many go by the
// default depth: their forms over several isovalues hold three blocks per CU, not four, a tile is live when ANY of its isovalues
// cuts it, and sized by this rule c5 (2048 x 2048 x 1024 ushort, 8 isovalues) was 5 % slower (r10 F).
constexpr double TABLE_FILL = 0.68, TABLE_BAND_LO = 0.62, TABLE_BAND_HI = 0.72, TABLE_MIN_DEPTH = 3.0;
// Plans cut with a plane weight, at the device's own residency: read off profiles/r12_plan_balance.txt B.  With the cut
// balanced the step falls all the way to one round: 0.525 ms at 0.69 of a round, 0.516 - 0.523 between 0.86 and 0.97, and 0.493 -
// 0.501 on the three sizes between 0.978 and 0.996 (11 200 - 11 400 tiles; parents 0.559 - 0.570, noise 0.008) - the widest run
// within the noise of the best, so the band is that run and the fill its centre.  Past one round (1.01) the step is 0.539: worse
// than the best by 0.045 and than 0.69 of a round by 0.013, still ahead of the parent.  A plan that misses the band on either side
// is sized again by the next two calls; hi stays below 1 (table_keeps).  The curve was measured at four blocks per compute unit
// and nowhere else: a context whose residency is forced (MC33_HIP_SWEEP_BLOCKS_PER_CU) keeps the constants above (table_band).
constexpr double TABLE_FILL_BALANCED = 0.987, TABLE_BAND_BALANCED_LO = 0.978, TABLE_BAND_BALANCED_HI = 0.997;
static inline void table_retarget(TablePolicy &p, unsigned long long word, const TableFacts &f) {
	if (f.table_tiles) { p.target = f.table_tiles; return; }
	if (f.rz || f.rz_table || !f.resident_blocks) return;
	const uint64_t tiles = (word & 0xFFFFFFFFull) >> 1, live = word >> 32;
	if (!(word & 1ull) || !tiles || !live) return;
	const double one_round = 4.0 * f.resident_blocks;
	double min_depth = TABLE_MIN_DEPTH;
	if (f.unit / SWEEP_DEPTH_TABLE < one_round) {  // (plan_tiles: such a grid gets one round, or what its slices make at the smallest depth)
		min_depth = (double)std::max(1u, f.min_depth);
		if (f.unit / min_depth < one_round) return;
	}
	// (the word is read as it stands: its count may be of the plan before the one in force)
	const uint64_t cur = f.plan_tiles ? f.plan_tiles : tiles;
	const TableBand band = table_band(f.weight, f.forced_residency, TableBand{TABLE_FILL, TABLE_BAND_LO, TABLE_BAND_HI}, TableBand{TABLE_FILL_BALANCED, TABLE_BAND_BALANCED_LO, TABLE_BAND_BALANCED_HI});
	if (table_keeps(live * cur / tiles, f.resident_blocks, band.lo, band.hi)) { p.pending = 0u; return; }
	const uint32_t t = table_target(live, tiles, f.resident_blocks, f.unit, min_depth, band.fill);
	if (!t || t == p.target) { p.pending = 0u; return; }
	if (!p.pending || std::fabs((double)t - (double)p.pending) > 0.05 * (double)p.pending) { p.pending = t; return; }  // (a second call has to agree)
	p.pending = 0u; p.target = t;
}
// Whether the sweep about to be launched with a table goes by a live list (k_tile_verdicts, k_live_compact, k_sweep_live) or works
// its verdicts out itself (k_sweep).  The list pays where dead tiles have to make room for live ones: a plan
// of at least one round of the device.  Below that every tile has a slot of its own anyway, and the two small launches are a
// loss - 7.5 us of the 110 a 256^3 step takes (profiles/r09_sweep_refill.txt D).  MC33_HIP_LIVE=1 / 0: always / never (the tests
// of the list run on small grids).
// While the one-round plan stands in for the finer one (table_plan) every tile has its slot and the preamble form is the faster
// one - it is the parent's sweep, where the list's two launches cost 10 us of 940 (r09 F) - but only a list's count can end the
// stand-in: one sweep in 16 goes by a list, the first of them at once.
static inline bool table_wants_list(TablePolicy &p, const TableFacts &f) {
	bool want = f.plan_tiles >= (uint64_t)f.resident_blocks * 4 || f.plan_sized;  // (a sized plan always: only a list's count can size it again)
	if (p.coarse) want = (p.coarse_sweeps++ % 16u) == 0u;
	return f.live > 0 || (f.live < 0 && want);
}
// the samples changed, or may have: the finer plan until a sweep says otherwise, at its default depth until one has published a count
static inline void table_forget(TablePolicy &p) { p.coarse = false; p.target = 0u; p.pending = 0u; }
#endif
