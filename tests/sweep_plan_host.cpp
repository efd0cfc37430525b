// How a sweep's plan shares its tiles out among its columns, and which fill and band a sized plan goes by
// (mc33_c_library_amd/csrc/mc33_sweep_plan.h), in a stand-alone host program: the same text the library compiles.  Test
// infrastructure (tests/test_sweep_plan_cpu.py builds it with g++ and holds its output to a numpy restatement); a stand-alone
// program, so that it can also be built with -fsanitize=address,undefined.
//
//   sweep_plan_host shares <points z> <points y> <points x> <nzc> <B> <plane weight>
// the columns of that grid (y tile major, groups of up to four segments), their work per plane as plan_sweep states it - the
// sample rows of the y tile in whole batches of four, with plan_column_weight's share for a plane - and plan_shares over them.
// The arrays are exactly ncol long ... for the sanitizers.  Prints: tiles, then the chunks of every column.
//
//   sweep_plan_host old <points z> <points y> <points x> <nzc> <B>
// the same columns shared out by the rule as it stood before there was a weight, restated here as plan_sweep had it.
//
//   sweep_plan_host band <plane weight> <forced residency 0|1> <fill> <lo> <hi> <fill2> <lo2> <hi2>
// Prints: table_band's fill, lo, hi.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../mc33_c_library_amd/csrc/mc33_sweep_pack.h"
#include "../mc33_c_library_amd/csrc/mc33_sweep_plan.h"

static void columns_of(uint32_t npy, uint32_t npx, std::vector<double> &rows, std::vector<uint32_t> &waves) {
	const uint32_t ny = npy - 1u, nx = npx - 1u, nseg = (nx + 255u) / 256u, nXG = (nseg + 3u) / 4u, nYT = (ny + 62u) / 63u;
	for (uint32_t yt = 0; yt < nYT; yt++)
		for (uint32_t xg = 0; xg < nXG; xg++) {
			waves.push_back(std::min(4u, nseg - xg * 4u));
			rows.push_back((double)((std::min(64u, ny + 1u - yt * 63u) + 3u) / 4u * 4u));
		}
}

int main(int argc, char **argv) {
	if (argc == 10 && !strcmp(argv[1], "band")) {
		const TableBand b = table_band(atof(argv[2]), atoi(argv[3]) != 0, TableBand{atof(argv[4]), atof(argv[5]), atof(argv[6])}, TableBand{atof(argv[7]), atof(argv[8]), atof(argv[9])});
		printf("%.17g %.17g %.17g\n", b.fill, b.lo, b.hi);
		return 0;
	}
	const bool old = argc == 7 && !strcmp(argv[1], "old");
	if (!old && !(argc == 8 && !strcmp(argv[1], "shares"))) { fprintf(stderr, "usage: sweep_plan_host shares | old | band ...\n"); return 2; }
	const uint32_t npy = (uint32_t)strtoul(argv[3], nullptr, 10), npx = (uint32_t)strtoul(argv[4], nullptr, 10), nzc = (uint32_t)strtoul(argv[5], nullptr, 10);
	const uint64_t B = strtoull(argv[6], nullptr, 10);
	std::vector<double> w;
	std::vector<uint32_t> waves;
	columns_of(npy, npx, w, waves);
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
