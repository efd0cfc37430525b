// The arithmetic and indexing of k_sp_spectrum (mc33_c_library_amd/csrc/mc33_spectrum.hip.h) compiled for the host: the same text
// the device compiles, its phases run lane by lane in the order the kernel's barrier allows, the work items dealt to a few
// "blocks" as the kernel's grid-stride loop deals them.  Test infrastructure (tests/test_spectrum_cpu.py builds it with g++ and
// holds its output to the numpy oracle); a stand-alone program, so that it can also be built with -fsanitize=address,undefined.
//
//   spectrum_host <case file> <output file>
// case file: 12 int64 words - sample type (0 f32, 1 f64, 2 u8, 3 u16, 4 u32), npx, npy, npz, pitch, slice, offset (in samples),
// samples per load (1, or 2 / 4 for the packed form of 2- / 1-byte samples), z_begin, z_end, whether plane z_end counts, n -,
// 255 doubles of isovalues (the first n are used), the length of the flat source buffer in samples as one more int64 and the
// buffer.  The buffer holds exactly what the call may read: a read outside it is the sanitizer's to find.
// output file: 256 uint64 histogram, 256 int64 difference array, uint64 NaN samples, two doubles: minimum and maximum.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#define SP_HD inline
#include "../mc33_c_library_amd/csrc/mc33_spectrum.hip.h"

constexpr int BLOCKS = 3;   // (fewer than the items of most cases: a block takes several, and keeps its lanes' state between them)

struct HostCounters {
	uint32_t *h;
	int *d;
	void hist(bool valid, uint32_t rank) { if (valid) h[rank]++; }
	void diff(bool cut, uint32_t mn, uint32_t mx) { if (cut) { d[mn]++; d[mx]--; } }
};

struct Out {
	uint64_t hist[256];
	int64_t diff[256];
	uint64_t nan;
	double lo, hi;
};

template <typename T, typename R, int S>
static void run(const SpPlan &p, const double *isos_in, const T *src, Out &out) {
	memset(&out, 0, sizeof out);
	uint64_t klo = sp_key(__builtin_huge_val()), khi = sp_key(-__builtin_huge_val());
	for (int b = 0; b < BLOCKS; b++) {
		// what the kernel keeps in LDS; the rank planes begin poisoned, as a block finds them
		R isos[256];
		uint32_t hist[256] = {0};
		int diff[256] = {0};
		uint8_t table[256];
		std::vector<uint8_t> ranks(2 * SP_RANK_PLANE, 0xEE);
		for (int k = 0; k < 256; k++) isos[k] = k < (int)p.n ? (R)isos_in[k] : (R)__builtin_huge_val();
		for (int k = 0; k < 256; k++) table[k] = sizeof(T) == 1 ? (uint8_t)sp_rank<R>(isos, p.n, p.top, (R)(T)k) : (uint8_t)0;
		std::vector<SpLane> st(SP_THREADS);
		for (auto &s : st) sp_lane_init(s);
		HostCounters ctr{hist, diff};
		for (uint64_t item = (uint64_t)b; item < p.items; item += BLOCKS) {
			uint32_t X0, Y0, kb, ke;
			sp_item(p, item, X0, Y0, kb, ke);
			for (uint32_t k = kb; k <= ke; k++) {
				uint8_t *plane = ranks.data() + ((k - kb) & 1u) * SP_RANK_PLANE;
				const bool counts = k < ke || (ke == p.k_end && p.last_plane_counts != 0u);
				for (int lane = 0; lane < SP_THREADS; lane++) sp_stage<T, R, S>(p, src, k, X0, Y0, counts, isos, table, plane, st[lane], ctr, lane);
				for (int lane = SP_THREADS - 1; lane >= 0; lane--) sp_cells(p, plane, X0, Y0, k == kb, st[lane], ctr, lane);
			}
		}
		for (int k = 0; k < 256; k++) { out.hist[k] += hist[k]; out.diff[k] += diff[k]; }
		for (auto &s : st) {
			out.nan += s.nan;
			if (sp_key(s.lo) < klo) klo = sp_key(s.lo);
			if (sp_key(s.hi) > khi) khi = sp_key(s.hi);
		}
	}
	out.lo = sp_unkey(klo);
	out.hi = sp_unkey(khi);
}

template <typename T, typename R>
static int typed(const SpPlan &p, int pack, const double *isos, const std::vector<char> &src, long long off, Out &out) {
	const T *s = (const T *)src.data() + off;
	if (pack == 1) run<T, R, 1>(p, isos, s, out);
	else if (sizeof(T) < 4 && pack == (int)(4 / sizeof(T))) run<T, R, (sizeof(T) < 4 ? 4 / sizeof(T) : 1)>(p, isos, s, out);
	else return 3;
	return 0;
}

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	long long h[12], ns = 0;
	double isos[255];
	static const size_t bytes_of[5] = {4, 8, 1, 2, 4};
	if (!read_all(f, h, sizeof h) || !read_all(f, isos, sizeof isos) || !read_all(f, &ns, sizeof ns) || h[0] < 0 || h[0] > 4 || h[11] < 0 || h[11] > SP_MAX_ISOS) {
		fprintf(stderr, "bad case file\n");
		return 2;
	}
	const size_t sb = bytes_of[h[0]];
	std::vector<char> src((size_t)ns * sb);
	if (!read_all(f, src.data(), src.size())) return 2;
	fclose(f);
	if (h[1] < 2 || h[2] < 2 || h[3] < 2 || !(h[8] < h[9]) || h[9] > h[3] - 1 || h[4] < h[1] || h[5] < h[4] * h[2]) { fprintf(stderr, "refused\n"); return 3; }
	SpPlan p;
	memset(&p, 0, sizeof p);
	sp_plan(p, (uint32_t)h[1], (uint32_t)h[2], (uint32_t)h[8], (uint32_t)h[9], h[10] != 0, (uint32_t)h[11], (size_t)h[4], (size_t)h[5]);
	Out out;
	int rc;
	switch (h[0]) {
	case 0: rc = typed<float, float>(p, (int)h[7], isos, src, h[6], out); break;
	case 1: rc = typed<double, double>(p, (int)h[7], isos, src, h[6], out); break;
	case 2: rc = typed<uint8_t, float>(p, (int)h[7], isos, src, h[6], out); break;
	case 3: rc = typed<uint16_t, float>(p, (int)h[7], isos, src, h[6], out); break;
	default: rc = typed<uint32_t, float>(p, (int)h[7], isos, src, h[6], out); break;
	}
	if (rc) { fprintf(stderr, "refused\n"); return rc; }
	f = fopen(argv[2], "wb");
	if (!f || fwrite(&out, 1, sizeof out, f) != sizeof out || fclose(f) != 0) { perror(argv[2]); return 2; }
	printf("%u x %u tiles, %u chunks, %llu items on %d blocks, first step %u\n", p.tiles_x, p.tiles_y, p.chunks_z, (unsigned long long)p.items, BLOCKS, p.top);
	return 0;
}
