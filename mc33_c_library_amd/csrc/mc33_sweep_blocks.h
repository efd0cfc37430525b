// mc33_sweep_blocks.h -- the walk of the sweep that leaves dead blocks out (k_sweep_live_blocks) over the live blocks of one plane of
// its tile, as pure functions of the plane's block word (k_block_verdicts): no HIP type, no context, host and device alike.
// Included by mc33_kernels.hip (through mc33_records.hip.h) and by a host program (tests/sweep_blocks_host.cpp).
//
// The word: bits 2 j, 2 j + 1 hold the code of block j = 4 g + k - row group g (sample rows 16 g .. 16 g + 15 of the tile), quarter k
// (samples 64 k .. 64 k + 63 of the row segment) - for j < 16, and bits 32 + 2 g, 33 + 2 g the code of the halo block of row group g
// (the first sample of the next segment over the rows of the group).  Code 0: the block is live; 1: all its samples lie strictly
// below the isovalue; 2: all strictly above.  (3 is never written; it is taken as "not live, not above".)
#ifndef MC33_SWEEP_BLOCKS_H
#define MC33_SWEEP_BLOCKS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC33_BLOCKS_FN __host__ __device__ static inline
#else
#define MC33_BLOCKS_FN static inline
#endif

constexpr uint32_t SWEEP_BLOCK_NONE = 16u;  // "no live block at or after this position": one past the last block of a plane

MC33_BLOCKS_FN uint32_t sweep_block_code(uint64_t word, uint32_t g, uint32_t k) { return (uint32_t)(word >> (8u * g + 2u * k)) & 3u; }
MC33_BLOCKS_FN uint32_t sweep_halo_code(uint64_t word, uint32_t g) { return (uint32_t)(word >> (32u + 2u * g)) & 3u; }

// The blocks of a plane the wave streams, bit j for block j: the live blocks of the tile's row groups (row_groups: 1 .. 4, the
// groups that hold a sample row of the tile) and, for a wave that loads its own halo column (own_halo), the quarter-3 block of
// every row group whose halo block is live - the halo load rides on the batch of quarter 3, so that batch has to exist; what it
// streams of a dead block classifies as the block's constant does (all strictly on one side, none equal to the isovalue).  A wave
// that takes its halo bits from its neighbour's mailbox does not look at the halo codes.
MC33_BLOCKS_FN uint32_t sweep_live_mask(uint64_t word, uint32_t row_groups, bool own_halo) {
	const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
	uint32_t e = ~(lo | lo >> 1) & 0x55555555u;  // bit 2 j: block j is live
	e = (e | e >> 1) & 0x33333333u;              // ... gathered into bit j
	e = (e | e >> 2) & 0x0F0F0F0Fu;
	e = (e | e >> 4) & 0x00FF00FFu;
	e = (e | e >> 8) & 0x0000FFFFu;
	if (own_halo) {
		const uint32_t h = ~(hi | hi >> 1) & 0x55u;  // bit 2 g: the halo block of row group g is live
		e |= (h & 1u) << 3 | (h & 4u) << 5 | (h & 16u) << 7 | (h & 64u) << 9;
	}
	return e & ((1u << (4u * row_groups)) - 1u);
}

// The first block of `mask` at or after position j (j <= 16), SWEEP_BLOCK_NONE where there is none
MC33_BLOCKS_FN uint32_t sweep_next_block(uint32_t mask, uint32_t j) {
	const uint32_t m = j < 16u ? (mask & 0xFFFFu) >> j << j : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
	return m ? (uint32_t)__builtin_ctz(m) : SWEEP_BLOCK_NONE;  // (s_ff1_i32_b32)
#else
	for (uint32_t b = j; b < 16u; b++)
		if ((m >> b) & 1u) return b;
	return SWEEP_BLOCK_NONE;
#endif
}

// What a plane's bit rows start as, before any block is streamed: word k of a lane (a sample row) of row group g - all ones where
// block (g, k) lies above the isovalue (the sign bit of iso - F), zero where it lies below, and zero where it is live (its batch
// writes the rows)
MC33_BLOCKS_FN uint64_t sweep_const_word(uint64_t word, uint32_t g, uint32_t k) { return sweep_block_code(word, g, k) == 2u ? ~0ull : 0ull; }
// ... and the halo sample of the rows of group g as a float's bits: -inf below, +inf above; a live halo block: +0, until its load
// puts the sample there
MC33_BLOCKS_FN uint32_t sweep_const_halo_bits(uint64_t word, uint32_t g) {
	const uint32_t c = sweep_halo_code(word, g);
	return c == 0u ? 0u : c == 1u ? 0xFF800000u : 0x7F800000u;
}
#endif
