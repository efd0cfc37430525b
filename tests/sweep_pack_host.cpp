// The two device-free rules of the sweep with a range table - the packed live list (mc33_c_library_amd/csrc/mc33_sweep_pack.h) and the
// size of the plan (mc33_sweep_plan.h) - in a stand-alone host program: the same text the library compiles.  Test infrastructure (tests/test_sweep_pack_cpu.py builds it with g++ and holds its
// output to a numpy restatement); a stand-alone program, so that it can also be built with -fsanitize=address,undefined.
//
//   sweep_pack_host pack <verdict file> <threads>
// verdict file: one byte per block of a plan (bits 0 - 3: the wave has nothing to stream, bit 4: the plan grouped the block).
// threads == 0: pack_live_list, block after block.  threads > 0: the list as k_live_compact makes it - every thread a contiguous
// run of blocks, the places from two exclusive prefix sums over the threads (whole blocks, leftover tiles) and the place of a quad
// left behind by the thread that holds its first tile - with the threads run one after the other, in DESCENDING order in the
// second pass: nothing may depend on the order.
// Prints: entries, live tiles, then the four words of every entry, one entry per line.  The entries are written into a buffer
// of exactly 4 * ceil(live / 4) words ... for the sanitizers; a place outside it ends the program with status 3.
//
//   sweep_pack_host target <live> <tiles> <resident blocks> <unit> <min depth> <fill> <lo> <hi> <live of the plan in force>
// Prints: table_target, table_keeps.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mc33_c_library_amd/csrc/mc33_sweep_pack.h"
#include "../mc33_c_library_amd/csrc/mc33_sweep_plan.h"

static int popc4(uint32_t v) { return (int)((v & 1u) + ((v >> 1) & 1u) + ((v >> 2) & 1u) + ((v >> 3) & 1u)); }

int main(int argc, char **argv) {
	if (argc >= 2 && !strcmp(argv[1], "target") && argc == 11) {
		const uint64_t live = strtoull(argv[2], nullptr, 10), tiles = strtoull(argv[3], nullptr, 10), live_now = strtoull(argv[10], nullptr, 10);
		const uint32_t resident = (uint32_t)strtoul(argv[4], nullptr, 10);
		const double unit = atof(argv[5]), min_depth = atof(argv[6]), fill = atof(argv[7]), lo = atof(argv[8]), hi = atof(argv[9]);
		printf("%u %d\n", table_target(live, tiles, resident, unit, min_depth, fill), table_keeps(live_now, resident, lo, hi));
		return 0;
	}
	if (argc != 4 || strcmp(argv[1], "pack")) { fprintf(stderr, "usage: sweep_pack_host pack <verdict file> <threads> | target ...\n"); return 2; }
	FILE *f = fopen(argv[2], "rb");
	if (!f) return 2;
	std::vector<uint8_t> verdict;
	for (int ch; (ch = fgetc(f)) != EOF;) verdict.push_back((uint8_t)ch);
	fclose(f);
	const uint32_t nblocks = (uint32_t)verdict.size(), threads = (uint32_t)strtoul(argv[3], nullptr, 10);
	uint32_t whole = 0, left = 0;
	for (uint8_t vb : verdict) { const uint32_t v = vb & 15u; if (v == 0u) whole++; else left += 4u - (uint32_t)popc4(v); }
	const uint32_t nent = whole + (left + 3u) / 4u;
	std::vector<uint32_t> ent((size_t)nent * 4u, 0xDEADBEEFu);
	uint32_t n = 0, live_tiles = 0;
	if (threads == 0u) {
		// (pack_live_list asks for room for 4 * nblocks words: a buffer of that size, and the entries copied, so that the exact one above
		// still says what was written)
		std::vector<uint32_t> room((size_t)nblocks * 4u + 4u, 0xDEADBEEFu);
		n = pack_live_list(verdict.data(), nblocks, room.data(), &live_tiles);
		if (n != nent) return 3;
		if (!ent.empty()) memcpy(ent.data(), room.data(), ent.size() * sizeof(uint32_t));
		for (size_t k = ent.size(); k < room.size(); k++) if (room[k] != 0xDEADBEEFu) return 3;
	} else {
		const uint32_t per = (nblocks + threads - 1u) / threads;
		std::vector<uint32_t> W0(threads), L0(threads), quad_at((left + 3u) / 4u + 1u, 0xFFFFFFFFu);
		uint32_t W = 0, L = 0;
		auto run = [&](uint32_t t, uint32_t &b0, uint32_t &b1) { b0 = t * per < nblocks ? t * per : nblocks; b1 = b0 + per < nblocks ? b0 + per : nblocks; };
		for (uint32_t t = 0; t < threads; t++) {  // the two exclusive prefix sums
			uint32_t b0, b1;
			run(t, b0, b1);
			W0[t] = W; L0[t] = L;
			for (uint32_t b = b0; b < b1; b++) { const uint32_t v = verdict[b] & 15u; if (v == 0u) W++; else L += 4u - (uint32_t)popc4(v); }
		}
		for (uint32_t t = 0; t < threads; t++) {  // pass 1: whole blocks, and where the quads go
			uint32_t b0, b1;
			run(t, b0, b1);
			uint32_t w = W0[t], l = L0[t];
			for (uint32_t b = b0; b < b1; b++) {
				const uint32_t vb = verdict[b], v = vb & 15u;
				if (v == 0u) {
					const uint32_t at = pack_whole_at(w, l);
					if (at >= nent) return 3;
					ent[4u * at] = (4u * b) | ((vb & MC33_VERDICT_GROUPED) ? MC33_PACK_GROUP : 0u);
					ent[4u * at + 1u] = 4u * b + 1u; ent[4u * at + 2u] = 4u * b + 2u; ent[4u * at + 3u] = 4u * b + 3u;
					w++;
				} else
					for (uint32_t k = 0; k < 4u; k++)
						if (!((v >> k) & 1u)) { if ((l & 3u) == 0u) quad_at[l >> 2] = pack_quad_at(l >> 2, w); l++; }
			}
		}
		for (uint32_t t = threads; t-- > 0u;) {  // pass 2: the leftover tiles
			uint32_t b0, b1;
			run(t, b0, b1);
			uint32_t l = L0[t];
			for (uint32_t b = b0; b < b1; b++) {
				const uint32_t v = verdict[b] & 15u;
				if (v == 0u) continue;
				for (uint32_t k = 0; k < 4u; k++)
					if (!((v >> k) & 1u)) {
						if (quad_at[l >> 2] >= nent) return 3;
						ent[4u * quad_at[l >> 2] + (l & 3u)] = 4u * b + k;
						l++;
					}
			}
		}
		for (uint32_t s = L & 3u; s && s < 4u; s++) ent[4u * quad_at[L >> 2] + s] = MC33_PACK_NONE;
		n = W + (L + 3u) / 4u; live_tiles = 4u * W + L;
	}
	printf("%u %u\n", n, live_tiles);
	for (uint32_t e = 0; e < n; e++) printf("%u %u %u %u\n", ent[4u * e], ent[4u * e + 1u], ent[4u * e + 2u], ent[4u * e + 3u]);
	return 0;
}
