// The walk of the block sweep over the live blocks of a plane (mc33_c_library_amd/csrc/mc33_sweep_blocks.h) in a stand-alone host
// program: the same text the library compiles.  Test infrastructure (tests/test_sweep_blocks_cpu.py builds it with g++ and holds
// its output to a numpy restatement); a stand-alone program, so that it can also be built with -fsanitize=address,undefined.
//
//   sweep_blocks_host <file>
// file: one line per case, "<word in hex> <row groups 1 .. 4> <own halo 0 | 1>".
// Prints one line per case:
//   the live mask (hex); the walk - sweep_next_block from position 0, then from one past every block it returns, until none (the
//   positions it returned as 16 hex digits' worth of a second mask, and its last answer); sweep_next_block(mask, j) for every
//   j = 0 .. 16 (17 numbers); for every row group the four constant words as one nibble (bit k: word k is all ones; a word that is
//   neither zero nor all ones ends the program with status 3) and the halo constant's bits (hex).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../mc33_c_library_amd/csrc/mc33_sweep_blocks.h"

int main(int argc, char **argv) {
	if (argc != 2) { fprintf(stderr, "usage: sweep_blocks_host <file>\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) return 2;
	unsigned long long w;
	unsigned groups, own;
	while (fscanf(f, "%llx %u %u", &w, &groups, &own) == 3) {
		if (groups < 1u || groups > 4u || own > 1u) { fclose(f); return 2; }
		const uint32_t mask = sweep_live_mask((uint64_t)w, groups, own != 0u);
		uint32_t walked = 0u, j = 0u, steps = 0u, last;
		for (;;) {
			last = sweep_next_block(mask, j);
			if (last == SWEEP_BLOCK_NONE) break;
			if (last < j || last > 15u || ++steps > 16u) { fclose(f); return 3; }
			walked |= 1u << last;
			j = last + 1u;
		}
		printf("%x %x %u", mask, walked, last);
		for (uint32_t at = 0; at <= 16u; at++) printf(" %u", sweep_next_block(mask, at));
		for (uint32_t g = 0; g < 4u; g++) {
			uint32_t ones = 0u;
			for (uint32_t k = 0; k < 4u; k++) {
				const uint64_t c = sweep_const_word((uint64_t)w, g, k);
				if (c != 0ull && c != ~0ull) { fclose(f); return 3; }
				if (c) ones |= 1u << k;
			}
			printf(" %x %x", ones, sweep_const_halo_bits((uint64_t)w, g));
		}
		printf("\n");
	}
	fclose(f);
	return 0;
}
