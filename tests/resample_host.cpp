// The arithmetic and indexing of k_rs_resample (mc33_c_library_amd/csrc/mc33_resample.hip.h) compiled for the host: the same text
// the device compiles, its phases run lane by lane in the order the kernel's barriers allow.  Test infrastructure
// (tests/test_resample_cpu.py builds it with g++ and holds its output to the numpy oracle bit for bit); a stand-alone program, so
// that it can also be built with -fsanitize=address,undefined and run by hand.
//
//   resample_host <case file> <output file>
// case file: 16 int64 words - sample type (0 f32, 1 f64, 2 u8, 3 u16, 4 u32), np[3], ntaps[3], stride[3], source pitch, slice,
// offset, output pitch, slice, offset (in samples) -, 3 x 17 doubles of taps, the flat source buffer (its length in samples as one
// more int64 before it) and the flat output buffer as it is before the call (likewise).  The output file is the flat output buffer
// afterwards.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using std::floor;
#define RS_HD inline
#include "../mc33_c_library_amd/csrc/mc33_resample.hip.h"

template <typename T>
static void run(const RsPlan &p, const double *taps52, const T *src, T *dst) {
	std::vector<double> lds(rs_lds_doubles(p));
	double *taps = lds.data(), *raw = taps + RS_TAP_WORDS, *sx = raw + (size_t)p.nrows * p.ncols, *ring = sx + (size_t)p.nrows * p.tx;
	const RsAxis az = p.ax[2];
	const size_t plane = (size_t)p.tx * p.ty;
	for (long long blk = 0; blk < p.tiles_x * p.tiles_y * p.chunks_z; blk++) {
		long long b = blk;
		const long long bx = b % p.tiles_x; b /= p.tiles_x;
		const long long by = b % p.tiles_y, bz = b / p.tiles_y;
		const long long X0 = bx * p.tx, Y0 = by * p.ty, Z0 = bz * RS_ZCHUNK;
		const long long Z1 = Z0 + RS_ZCHUNK < az.n_out ? Z0 + RS_ZCHUNK : az.n_out;
		for (size_t k = 0; k < lds.size(); k++) lds[k] = NAN;  // (a block finds LDS as the block before it left it: here, poisoned)
		for (int k = 0; k < RS_TAP_WORDS; k++) taps[k] = taps52[k];
		long long next_u = Z0 * az.stride - az.r;
		for (long long Z = Z0; Z < Z1; Z++) {
			const long long lo = Z * az.stride - az.r, hi = lo + az.ntaps - 1;
			for (long long u = next_u > lo ? next_u : lo; u <= hi; u++) {
				for (int lane = 0; lane < RS_THREADS; lane++) rs_stage(p, src, rs_clamp(u, az.n_src), X0, Y0, raw, lane, RS_THREADS);
				for (int lane = RS_THREADS - 1; lane >= 0; lane--) rs_rows(p, taps, raw, sx, lane, RS_THREADS);
				for (int lane = 0; lane < RS_THREADS; lane++) rs_cols(p, taps, sx, ring + (size_t)rs_ring_slot(az, u) * plane, lane, RS_THREADS);
			}
			next_u = hi + 1;
			for (int lane = RS_THREADS - 1; lane >= 0; lane--) rs_emit(p, taps, ring, Z, X0, Y0, dst, lane, RS_THREADS);
		}
	}
}

template <typename T>
static int typed(const RsPlan &p, const double *taps, const std::vector<char> &src, std::vector<char> &dst, long long soff, long long doff) {
	run<T>(p, taps, (const T *)src.data() + soff, (T *)dst.data() + doff);
	return 0;
}

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	long long h[16];
	double taps[RS_TAP_WORDS] = {0};
	long long ns = 0, nd = 0;
	static const size_t bytes_of[5] = {4, 8, 1, 2, 4};
	if (!read_all(f, h, sizeof h) || !read_all(f, taps, 3 * RS_MAX_TAPS * sizeof(double)) || h[0] < 0 || h[0] > 4) { fprintf(stderr, "bad case file\n"); return 2; }
	const size_t sb = bytes_of[h[0]];
	std::vector<char> src, dst;
	if (!read_all(f, &ns, sizeof ns)) return 2;
	src.resize((size_t)ns * sb);
	if (!read_all(f, src.data(), src.size()) || !read_all(f, &nd, sizeof nd)) return 2;
	dst.resize((size_t)nd * sb);
	if (!read_all(f, dst.data(), dst.size())) return 2;
	fclose(f);
	RsPlan p;
	memset(&p, 0, sizeof p);
	for (int a = 0; a < 3; a++) {
		if (!(h[4 + a] & 1) || h[4 + a] > RS_MAX_TAPS || h[7 + a] < 1) { fprintf(stderr, "refused\n"); return 3; }
		rs_axis(p.ax[a], h[1 + a], (int)h[4 + a], (int)h[7 + a]);
		if (p.ax[a].n_out < 2) { fprintf(stderr, "refused\n"); return 3; }
	}
	p.spitch = (size_t)h[10]; p.sslice = (size_t)h[11]; p.dpitch = (size_t)h[13]; p.dslice = (size_t)h[14];
	rs_plan_tiles(p);
	// the buffers hold exactly what the call may touch: a read or write outside them is the sanitizer's to find
	switch (h[0]) {
	case 0: typed<float>(p, taps, src, dst, h[12], h[15]); break;
	case 1: typed<double>(p, taps, src, dst, h[12], h[15]); break;
	case 2: typed<uint8_t>(p, taps, src, dst, h[12], h[15]); break;
	case 3: typed<uint16_t>(p, taps, src, dst, h[12], h[15]); break;
	default: typed<uint32_t>(p, taps, src, dst, h[12], h[15]); break;
	}
	f = fopen(argv[2], "wb");
	if (!f || fwrite(dst.data(), 1, dst.size(), f) != dst.size() || fclose(f) != 0) { perror(argv[2]); return 2; }
	printf("tile %d x %d, %d x %d staged, %zu bytes of LDS, %lld blocks\n", p.tx, p.ty, p.ncols, p.nrows, rs_lds_doubles(p) * sizeof(double),
	       p.tiles_x * p.tiles_y * p.chunks_z);
	return 0;
}
