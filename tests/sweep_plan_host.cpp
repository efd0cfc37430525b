// How a sweep's plan is made and named, and the policy of the sweeps with a range table
// (mc33_c_library_amd/csrc/mc33_sweep_plan.h), in a stand-alone host program: the same text the library compiles.  Test
// infrastructure (tests/test_sweep_plan_cpu.py builds it with g++ and holds its output to a numpy restatement); a stand-alone
// program, so that it can also be built with -fsanitize=address,undefined.
//
//   sweep_plan_host shares <points z> <points y> <points x> <nzc> <B> <plane weight>
// the columns of that grid (plan_columns: y tile major, groups of up to four segments, the sample rows of the y tile in whole
// batches of four), with plan_column_weight's share for a plane, and plan_shares over them.
// The arrays are exactly ncol long ... for the sanitizers.  Prints: tiles, then the chunks of every column.
//
//   sweep_plan_host old <points z> <points y> <points x> <nzc> <B>
// the same columns shared out by the rule as it stood before there was a weight, restated here as plan_sweep had it.
//
//   sweep_plan_host band <plane weight> <forced residency 0|1> <fill> <lo> <hi> <fill2> <lo2> <hi2>
// Prints: table_band's fill, lo, hi.
//
//   sweep_plan_host plan <cells y> <segments> <rows per batch> <zs> <ze> <table 0|1> <target> <weight> <rz> <rz table> <resident blocks> <min depth>
// plan_slot, then plan_tiles.  Prints: slot zs ze depth target weight; then "large", or total, tiles and boundaries, a line per
// tile (seg yt z_lo z_hi) and a line per boundary (below above z yt seg).
//
//   sweep_plan_host policy <file>
// a TablePolicy that starts from zeros, and a line per step: plan | retarget | list | forget, the published word, then the
// TableFacts in the order of the struct.  Prints per step: the decision (plan: 0 | 1, list: 0 | 1, otherwise -), then coarse,
// coarse_sweeps, target, pending.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../mc33_c_library_amd/csrc/mc33_sweep_plan.h"

static uint32_t u32(const char *s) { return (uint32_t)strtoul(s, nullptr, 10); }

static int plan_mode(char **a) {
	const PlanGrid g{u32(a[2]), u32(a[3]), u32(a[4])};
	const PlanSlot ps = plan_slot(atoi(a[7]) != 0, u32(a[5]), u32(a[6]), u32(a[8]), atof(a[9]), u32(a[10]), u32(a[11]));
	printf("%d %u %u %u %u %.17g\n", ps.slot, ps.key.zs, ps.key.ze, ps.key.depth, ps.key.target, ps.key.weight);
	std::vector<SweepTile> tiles;
	std::vector<TileBoundary> bounds;
	uint64_t total = 0;
	if (!plan_tiles(g, ps.key, u32(a[12]), u32(a[13]), tiles, bounds, total)) { printf("large\n"); return 0; }
	printf("%llu %zu %zu\n", (unsigned long long)total, tiles.size(), bounds.size());
	for (const SweepTile &t : tiles) printf("%u %u %u %u\n", t.seg, t.yt, t.z_lo, t.z_hi);
	for (const TileBoundary &b : bounds) printf("%u %u %u %u %u\n", b.below, b.above, b.z, b.yt, b.seg);
	return 0;
}

static int policy_mode(const char *file) {
	FILE *f = fopen(file, "r");
	if (!f) return 2;
	TablePolicy p{false, 0u, 0u, 0u};
	char op[16];
	unsigned long long word, plan_tiles;
	TableFacts t{};
	int forced, sized;
	while (fscanf(f, "%15s %llu %lf %u %u %lf %d %u %u %u %d %llu %d", op, &word, &t.unit, &t.resident_blocks, &t.min_depth, &t.weight, &forced, &t.rz, &t.rz_table,
	              &t.table_tiles, &t.live, &plan_tiles, &sized) == 13) {
		t.forced_residency = forced != 0; t.plan_tiles = plan_tiles; t.plan_sized = sized != 0;
		if (!strcmp(op, "plan")) printf("%d", table_plan(p, word));
		else if (!strcmp(op, "list")) printf("%d", table_wants_list(p, t) ? 1 : 0);
		else if (!strcmp(op, "retarget")) { table_retarget(p, word, t); printf("-"); }
		else if (!strcmp(op, "forget")) { table_forget(p); printf("-"); }
		else { fclose(f); return 2; }
		printf(" %d %u %u %u\n", p.coarse ? 1 : 0, p.coarse_sweeps, p.target, p.pending);
	}
	fclose(f);
	return 0;
}

int main(int argc, char **argv) {
	if (argc == 14 && !strcmp(argv[1], "plan")) return plan_mode(argv);
	if (argc == 3 && !strcmp(argv[1], "policy")) return policy_mode(argv[2]);
	if (argc == 10 && !strcmp(argv[1], "band")) {
		const TableBand b = table_band(atof(argv[2]), atoi(argv[3]) != 0, TableBand{atof(argv[4]), atof(argv[5]), atof(argv[6])}, TableBand{atof(argv[7]), atof(argv[8]), atof(argv[9])});
		printf("%.17g %.17g %.17g\n", b.fill, b.lo, b.hi);
		return 0;
	}
	const bool old = argc == 7 && !strcmp(argv[1], "old");
	if (!old && !(argc == 8 && !strcmp(argv[1], "shares"))) { fprintf(stderr, "usage: sweep_plan_host shares | old | band | plan | policy ...\n"); return 2; }
	const uint32_t npy = (uint32_t)strtoul(argv[3], nullptr, 10), npx = (uint32_t)strtoul(argv[4], nullptr, 10), nzc = (uint32_t)strtoul(argv[5], nullptr, 10);
	const uint64_t B = strtoull(argv[6], nullptr, 10);
	std::vector<double> w;
	std::vector<uint32_t> waves;
	plan_columns(PlanGrid{npy - 1u, (npx - 1u + 255u) / 256u, 4u}, w, waves);
	const uint64_t ncol = w.size();
	std::vector<uint32_t> chunks(ncol);
	uint64_t total = 0;
	if (old) {
		double W = 0;
		for (uint64_t i = 0; i < ncol; i++) W += w[i] * waves[i];
		std::vector<std::pair<double, uint64_t>> frac(ncol);
		for (uint64_t i = 0; i < ncol; i++) {
			const double share = (double)B * w[i] / W;
			const uint32_t n = (uint32_t)std::min<double>(std::max(1.0, std::floor(share)), (double)nzc);
			chunks[i] = n; total += (uint64_t)n * waves[i];
			frac[i] = {share - std::floor(share), i};
		}
		std::sort(frac.begin(), frac.end(), [](const std::pair<double, uint64_t> &x, const std::pair<double, uint64_t> &y) { return x.first > y.first; });
		for (uint64_t k = 0; k < ncol && total < B; k++)
			if (chunks[frac[k].second] < nzc) { chunks[frac[k].second]++; total += waves[frac[k].second]; }
	} else {
		const double weight = atof(argv[7]);
		for (uint64_t i = 0; i < ncol; i++) w[i] = plan_column_weight(w[i], 4u, weight);
		std::vector<PlanFrac> frac(ncol);
		total = plan_shares(w.data(), waves.data(), ncol, B, nzc, chunks.data(), frac.data());
	}
	printf("%llu\n", (unsigned long long)total);
	for (uint64_t i = 0; i < ncol; i++) printf("%u\n", chunks[i]);
	return 0;
}
