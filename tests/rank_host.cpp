// The selection and indexing of k_rk_minmax and k_rk_median (mc33_c_library_amd/csrc/mc33_rank.hip.h) compiled for the host: the
// same text the device compiles, its phases run lane by lane in the order the kernels' barriers allow - every phase in ascending
// or in descending lane order, alternating from phase to phase; the third argument exchanges the two.  Test infrastructure
// (tests/test_rank_cpu.py builds it with g++ and holds its output to the numpy oracle bit for bit); a stand-alone program, so
// that it can also be built with -fsanitize=address,undefined and run by hand.
//
//   rank_host <case file> <output file> <0 | 1: which phases run in descending lane order>
// case file: 16 int64 words - sample type (0 f32, 1 f64, 2 u8, 3 u16, 4 u32), np[3], radius[3], rank, source pitch, slice,
// offset, output pitch, slice, offset (in samples), two unused -, the flat source buffer (its length in samples as one int64
// before it) and the flat output buffer as it is before the call (likewise).  The output file is the flat output buffer afterwards.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RK_HD inline
#include "../mc33_c_library_amd/csrc/mc33_rank.hip.h"

// a phase over all lanes, ascending or descending
template <typename F>
static void lanes(bool down, F f) {
	if (down) for (int lane = RK_THREADS - 1; lane >= 0; lane--) f(lane);
	else for (int lane = 0; lane < RK_THREADS; lane++) f(lane);
}

template <typename T, int NXY, int NZ>
static void run(const RkPlan &p, const T *src, T *dst, bool flip_order) {
	typedef typename RkKey<T>::K K;
	const bool median = p.rank == RK_RANK_MEDIAN;
	std::vector<K> lds(p.lds_keys), regs((size_t)RK_THREADS * RK_FETCH);
	K *raw = lds.data(), *sx = raw + (size_t)p.nrows * p.ncols, *ring = median ? raw : sx + (size_t)p.nrows * p.tx;
	const size_t plane = (size_t)p.tx * p.ty, staged = (size_t)p.nrows * p.ncols;
	const bool a = flip_order, b = !flip_order;
	for (long long blk = 0; blk < p.tiles_x * p.tiles_y * p.chunks_z; blk++) {
		long long bb = blk;
		const long long bx = bb % p.tiles_x; bb /= p.tiles_x;
		const long long by = bb % p.tiles_y, bz = bb / p.tiles_y;
		const long long X0 = bx * p.tx, Y0 = by * p.ty, Z0 = bz * RK_ZCHUNK;
		const long long Z1 = Z0 + RK_ZCHUNK < p.n[2] ? Z0 + RK_ZCHUNK : p.n[2];
		// (a block finds LDS and its registers as the block before it left them: here, poisoned with the key that wins a maximum)
		memset(lds.data(), 0xFF, lds.size() * sizeof(K));
		memset(regs.data(), 0xFF, regs.size() * sizeof(K));
		const long long u0 = Z0 - p.r[2], u1 = Z1 - 1 + p.r[2];
		lanes(a, [&](int lane) { rk_fetch(p, src, rk_clamp(u0, p.n[2]), X0, Y0, &regs[(size_t)lane * RK_FETCH], lane, RK_THREADS); });
		for (long long u = u0; u <= u1; u++) {
			if (!median) {
				lanes(b, [&](int lane) { rk_put(p, &regs[(size_t)lane * RK_FETCH], raw, lane, RK_THREADS); });
				if (u < u1) lanes(a, [&](int lane) { rk_fetch(p, src, rk_clamp(u + 1, p.n[2]), X0, Y0, &regs[(size_t)lane * RK_FETCH], lane, RK_THREADS); });
				lanes(b, [&](int lane) { rk_rows(p, raw, sx, lane, RK_THREADS); });
				lanes(a, [&](int lane) {   // (no barrier between the two in the kernel: a lane runs them back to back)
					rk_cols(p, sx, ring + (size_t)rk_slot(p, u) * plane, lane, RK_THREADS);
					if (u - p.r[2] >= Z0) rk_emit_max(p, ring, u - p.r[2], X0, Y0, dst, lane, RK_THREADS);
				});
			} else {
				K *sorted = ring + NZ * staged;
				lanes(b, [&](int lane) { rk_put(p, &regs[(size_t)lane * RK_FETCH], ring + (size_t)rk_slot(p, u) * staged, lane, RK_THREADS); });
				if (u < u1) lanes(a, [&](int lane) { rk_fetch(p, src, rk_clamp(u + 1, p.n[2]), X0, Y0, &regs[(size_t)lane * RK_FETCH], lane, RK_THREADS); });
				if (u - p.r[2] < Z0) continue;
				if (NZ == 3) {
					lanes(b, [&](int lane) { rk_sort_columns(p, ring, u - 1, sorted, lane, RK_THREADS); });
					lanes(a, [&](int lane) { rk_emit_median<T, NXY, NZ>(p, sorted, u - 1, X0, Y0, dst, lane, RK_THREADS); });
				} else lanes(a, [&](int lane) { rk_emit_median<T, NXY, NZ>(p, ring, u, X0, Y0, dst, lane, RK_THREADS); });
			}
		}
	}
}

template <typename T>
static void typed(const RkPlan &p, const std::vector<char> &src, std::vector<char> &dst, long long soff, long long doff, bool flip_order) {
	const T *s = (const T *)src.data() + soff;
	T *d = (T *)dst.data() + doff;
	if (p.rank != RK_RANK_MEDIAN) { run<T, 1, 1>(p, s, d, flip_order); return; }
	switch ((2 * p.r[0] + 1) * (2 * p.r[1] + 1) * 10 + 2 * p.r[2] + 1) {   // (the dispatch of mc33hip_rank_grid)
	case 11: run<T, 1, 1>(p, s, d, flip_order); break;
	case 31: run<T, 3, 1>(p, s, d, flip_order); break;
	case 91: run<T, 9, 1>(p, s, d, flip_order); break;
	case 13: run<T, 1, 3>(p, s, d, flip_order); break;
	case 33: run<T, 3, 3>(p, s, d, flip_order); break;
	default: run<T, 9, 3>(p, s, d, flip_order); break;
	}
}

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 4) { fprintf(stderr, "usage: %s <case file> <output file> <0 | 1>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	long long h[16];
	long long ns = 0, nd = 0;
	static const size_t bytes_of[5] = {4, 8, 1, 2, 4};
	if (!read_all(f, h, sizeof h) || h[0] < 0 || h[0] > 4) { fprintf(stderr, "bad case file\n"); return 2; }
	const size_t sb = bytes_of[h[0]];
	std::vector<char> src, dst;
	if (!read_all(f, &ns, sizeof ns)) return 2;
	src.resize((size_t)ns * sb);
	if (!read_all(f, src.data(), src.size()) || !read_all(f, &nd, sizeof nd)) return 2;
	dst.resize((size_t)nd * sb);
	if (!read_all(f, dst.data(), dst.size())) return 2;
	fclose(f);
	RkPlan p;
	memset(&p, 0, sizeof p);
	unsigned radius[3];
	for (int a = 0; a < 3; a++) {
		if (h[1 + a] < 1 || h[4 + a] < 0 || h[4 + a] > 64) { fprintf(stderr, "refused\n"); return 3; }
		p.n[a] = h[1 + a]; p.r[a] = (int)h[4 + a]; radius[a] = (unsigned)h[4 + a];
	}
	if (!rk_accepts((int)h[7], radius)) { fprintf(stderr, "refused\n"); return 3; }
	p.rank = (int)h[7];
	p.spitch = (size_t)h[8]; p.sslice = (size_t)h[9]; p.dpitch = (size_t)h[11]; p.dslice = (size_t)h[12];
	rk_plan_tiles(p, sb == 8 ? 8 : 4);
	if (p.nrows * p.ncols > RK_FETCH * RK_THREADS) { fprintf(stderr, "a staged plane of %d x %d keys is more than the lanes fetch\n", p.nrows, p.ncols); return 4; }
	// the buffers hold exactly what the call may touch: a read or write outside them is the sanitizer's to find
	const bool flip_order = argv[3][0] == '1';
	switch (h[0]) {
	case 0: typed<float>(p, src, dst, h[10], h[13], flip_order); break;
	case 1: typed<double>(p, src, dst, h[10], h[13], flip_order); break;
	case 2: typed<uint8_t>(p, src, dst, h[10], h[13], flip_order); break;
	case 3: typed<uint16_t>(p, src, dst, h[10], h[13], flip_order); break;
	default: typed<uint32_t>(p, src, dst, h[10], h[13], flip_order); break;
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(dst.data(), 1, dst.size(), f) != dst.size() || fclose(f) != 0) { perror(argv[2]); return 2; }
	printf("tile %d x %d, %d x %d staged, %zu bytes of LDS, %lld blocks\n", p.tx, p.ty, p.ncols, p.nrows, p.lds_keys * (sb == 8 ? 8 : 4),
	       p.tiles_x * p.tiles_y * p.chunks_z);
	return 0;
}
