// The arithmetic and indexing of k_curvature (mc33_c_library_amd/csrc/mc33_curvature.hip.h) compiled for the host: curv_vertex, the
// same text the device compiles, run vertex by vertex.  Test infrastructure (tests/test_curvature_cpu.py builds it with g++ and
// holds its output to the numpy oracle bit for bit); a stand-alone program, so that it can also be built with
// -fsanitize=address,undefined.
//
//   curvature_host <case file> <output file>
// case file: 8 int64 words - sample type (0 f32, 1 f64, 2 u8, 3 u16, 4 u32), npx, npy, npz, pitch, slice (in samples), nV, sign -,
// 6 doubles r0[3], d[3], the length of the flat source buffer in samples as one more int64, the buffer, and nV x 3 vertex
// coordinates (doubles for sample type 1, floats otherwise: MC33_real).  The buffer begins with the first grid point and ends with
// the last: it holds exactly what the call may read, a read outside it is the sanitizer's to find (and what lies between the rows
// is poisoned by the test, so a read there shows in the output).
// output file: nV x 4 floats (mean, gauss, k1, k2), then the summary as the device keeps it: 9 uint32 - keys of lo[4], hi[4], undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CV_HD inline
#include "../mc33_c_library_amd/csrc/mc33_curvature.hip.h"

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <typename T, typename R>
static int run(const CurvGrid &g, const std::vector<char> &src, FILE *f, long long nV, std::vector<float> &out, CurvSum &sum) {
	std::vector<R> V((size_t)nV * 3);
	if (!read_all(f, V.data(), V.size() * sizeof(R))) return 2;
	const T *grid = (const T *)src.data();
	curv_sum_init(sum);
	for (long long v = 0; v < nV; v++) {
		float val[4];
		curv_vertex<T, R>(g, grid, V.data() + v * 3, val);
		for (int k = 0; k < 4; k++) out[(size_t)v * 4 + k] = val[k];
		curv_sum_add(sum, val);
	}
	return 0;
}

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s <case file> <output file>\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	long long h[8], ns = 0;
	double geo[6];
	static const size_t bytes_of[5] = {4, 8, 1, 2, 4};
	if (!read_all(f, h, sizeof h) || !read_all(f, geo, sizeof geo) || !read_all(f, &ns, sizeof ns) || h[0] < 0 || h[0] > 4 || h[6] < 0 || ns < 0) {
		fprintf(stderr, "bad case file\n");
		return 2;
	}
	// the refusals of mc33hip_curvature_vertices, and a buffer of exactly the readable extent
	if (h[1] < 3 || h[2] < 3 || h[3] < 3 || h[4] < h[1] || h[5] < h[4] * h[2] || (h[7] != 1 && h[7] != -1) ||
	    ns != (h[3] - 1) * h[5] + (h[2] - 1) * h[4] + h[1]) {
		fprintf(stderr, "refused\n");
		return 3;
	}
	std::vector<char> src((size_t)ns * bytes_of[h[0]]);
	if (!read_all(f, src.data(), src.size())) return 2;
	CurvGrid g;
	g.pitch = (uint64_t)h[4]; g.slice = (uint64_t)h[5];
	g.N[0] = (uint32_t)h[1] - 1u; g.N[1] = (uint32_t)h[2] - 1u; g.N[2] = (uint32_t)h[3] - 1u;
	for (int k = 0; k < 3; k++) { g.r0[k] = geo[k]; g.d[k] = geo[3 + k]; }
	g.sign = (double)h[7];
	std::vector<float> out((size_t)h[6] * 4);
	CurvSum sum;
	int rc;
	switch (h[0]) {
	case 0: rc = run<float, float>(g, src, f, h[6], out, sum); break;
	case 1: rc = run<double, double>(g, src, f, h[6], out, sum); break;
	case 2: rc = run<uint8_t, float>(g, src, f, h[6], out, sum); break;
	case 3: rc = run<uint16_t, float>(g, src, f, h[6], out, sum); break;
	default: rc = run<uint32_t, float>(g, src, f, h[6], out, sum); break;
	}
	fclose(f);
	if (rc) { fprintf(stderr, "bad case file\n"); return rc; }
	f = fopen(argv[2], "wb");
	if (!f || !(out.empty() || fwrite(out.data(), sizeof(float), out.size(), f) == out.size()) || fwrite(&sum, 1, sizeof sum, f) != sizeof sum || fclose(f) != 0) {
		perror(argv[2]);
		return 2;
	}
	printf("%lld vertices, %u undefined\n", h[6], sum.undefined);
	return 0;
}
