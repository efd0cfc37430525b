// mc33_sweep_pack.h -- the layout of the packed live list of a sweep with a range table, as plain functions (no HIP type): where
// its entries go (k_live_compact).  How many tiles the plan of such a sweep is asked for: mc33_sweep_plan.h.
// Included by mc33_kernels.hip and by host programs (tests/sweep_pack_host.cpp).
#ifndef MC33_SWEEP_PACK_H
#define MC33_SWEEP_PACK_H
#include <stdint.h>

#include "mc33_sweep_plan.h"  // (the size of the plan - table_target, table_keeps - comes with this header for the programs that include it alone)

#if defined(__HIPCC__)
#define MC33_PACK_FN __host__ __device__ static inline
#else
#define MC33_PACK_FN static inline
#endif

// ---- the packed live list ------------------------------------------------------------------------------------------------------------
// One 16-byte entry per block k_sweep_live has work for: four tile indices of the plan, wave k of the block streams tile k of its
// entry.  PACK_NONE: no tile (only the last quad of a list may have such waves).  Bit 31 of the FIRST word (a plan has fewer than
// 2^30 tiles): the entry is a whole group - a block of the plan with all four tiles live, which the plan made of the segments
// seg .. seg + 3 of one y tile over the same planes: its waves pass their halo bits through the mailbox.
// A verdict byte (k_tile_verdicts): bits 0 - 3, wave k of the plan's block has nothing to stream; bit 4, the plan grouped the block.
//
// Order.  A block of the plan with all four tiles live stays one entry (whole block); the live tiles of all other blocks (leftover
// tiles) are packed four at a time, in plan order (quads).  Whole blocks and quads are merged by the plan position of their first
// tile, which keeps the plan's ascending z_lo.  With W(b) the whole blocks before plan block b and L(b) the leftover tiles before b:
//   whole block b                                goes to W(b) + ceil(L(b) / 4)   (behind every quad that has begun),
//   quad q, whose first tile lies in block b,    goes to q + W(b).
// A whole block between the tiles of a quad thus comes right behind that quad; the list has ceil(live tiles / 4) entries.
#define MC33_PACK_NONE 0xFFFFFFFFu
#define MC33_PACK_GROUP 0x80000000u
#define MC33_VERDICT_GROUPED 16u

MC33_PACK_FN uint32_t pack_whole_at(uint32_t W, uint32_t L) { return W + (L + 3u) / 4u; }
MC33_PACK_FN uint32_t pack_quad_at(uint32_t q, uint32_t W) { return q + W; }

// The whole list from the verdict bytes, one block after the other (what k_live_compact does with 1024 threads and two prefix
// sums).  entries: room for 4 * nblocks words.  Returns the number of entries; *live_tiles: the live tiles.
static inline uint32_t pack_live_list(const uint8_t *verdict, uint32_t nblocks, uint32_t *entries, uint32_t *live_tiles) {
	uint32_t W = 0, L = 0, at = 0;
	for (uint32_t b = 0; b < nblocks; b++) {
		const uint32_t v = verdict[b] & 15u;
		if (v == 0u) {
			uint32_t *e = entries + 4u * pack_whole_at(W, L);
			e[0] = (4u * b) | ((verdict[b] & MC33_VERDICT_GROUPED) ? MC33_PACK_GROUP : 0u);
			e[1] = 4u * b + 1u; e[2] = 4u * b + 2u; e[3] = 4u * b + 3u;
			W++;
			continue;
		}
		for (uint32_t k = 0; k < 4u; k++) {
			if ((v >> k) & 1u) continue;
			if ((L & 3u) == 0u) at = pack_quad_at(L >> 2, W);
			entries[4u * at + (L & 3u)] = 4u * b + k;
			L++;
		}
	}
	for (uint32_t s = L & 3u; s && s < 4u; s++) entries[4u * at + s] = MC33_PACK_NONE;
	if (live_tiles) *live_tiles = 4u * W + L;
	return W + (L + 3u) / 4u;
}
#endif
