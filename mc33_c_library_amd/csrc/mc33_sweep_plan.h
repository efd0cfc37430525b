// mc33_sweep_plan.h -- how plan_sweep shares the tiles of a plan out among its columns, and which fill and band a sized plan goes
// by, as plain functions over caller-provided arrays (no HIP type).  Included by mc33_kernels.hip behind mc33_sweep_pack.h and by
// host programs (tests/sweep_plan_host.cpp).
#ifndef MC33_SWEEP_PLAN_H
#define MC33_SWEEP_PLAN_H
#include <stdint.h>

#include <algorithm>
#include <cmath>

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
#endif
