// mc33_distance.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// the nearest point of a triangle mesh in device memory for each of many query points - how far a changed surface has moved from
// the one it came from, how thick a shell is, which triangle is nearest to a probe (include/mc33_hip.h: mc33hip_surface_distance).
// DESIGN.md 25.
//
// The definition is in include/mc33_hip.h; tests/distance_oracle.py restates it in numpy, over all pairs.  The result is the
// smallest D2 over the usable triangles with ties to the smallest index: an exact function of the input, whatever is searched in
// whatever order.
// The passes: k_dist_bounds finds the box of the usable triangles (integer atomicMin / atomicMax on order-preserving keys of the
// doubles) and counts the others; the host cuts a uniform lattice over the box; k_dist_bin<false> counts the cells each usable
// triangle's box overlaps, the tile scan of mc33_mesh.hip.h turns the counts into cell starts, k_dist_bin<true> writes the triangle
// indices into the cell lists; k_dist_query, the hot path, a lane per point, visits cubic shells of cells around the point's own
// cell until a lower bound on everything not yet visited exceeds its best; k_dist_arg and k_dist_sum finish the summary.
// Nothing a block wrote with plain stores is read by another block of the same kernel: counts, cursors and the summary words are
// integer atomics, their readers are later kernels.

struct DistLattice {
	double origin[3], cell[3];  // cell k of axis a begins at origin[a] + k cell[a]
	double slack;               // what the stopping bound gives away: 2^-40 of the largest magnitude among the lattice's bounds
	uint32_t n[3];              // cells per axis; n[0] == 0: no usable triangle, no lattice
	uint32_t pad_;
};

struct DistOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long lo[3], hi[3];        // dist_key of the box of the usable triangles
	unsigned long long usable, bad, nonfinite;
	unsigned long long entries;             // cell-list entries of the lattice counted last
	unsigned long long matched, tests;
	unsigned long long max_bits, min_bits;  // the bits of the largest / smallest winning D2 (a non-negative double: its bits order as it does)
	unsigned long long argmax, argmin;
	double sum, sum_sq;
};

struct DistState {          // scratch of these passes besides the shared tile sums: on the MeasureState from the first call on, grown on demand, freed with it
	DistOut *d_out, *h_out;
	uint32_t *d_cells;      // [cells + 1] counts, scanned in place into the starts of the cell lists
	uint64_t cells_cap;
	uint32_t *d_cursor;     // [cells] entries written so far
	uint64_t cursor_cap;
	uint32_t *d_list;       // [entries] triangle indices, cell by cell
	uint64_t list_cap;
	unsigned long long *d_d2;  // [nP] the bits of the winning D2, all ones without a winner
	uint64_t d2_cap;
	double *d_part;         // [2 blocks] per-block sums of sqrt(D2) and of D2, in block order
	uint64_t part_cap;
	hipEvent_t ev[6];
	bool ev_made, timed;
	float ms[3];            // build, query, reduce of the last call at timing level 2
};

constexpr uint32_t DIST_MAX_CELLS = 256u;             // cells per axis at the most: 2^24 cells, 128 MB of starts and cursors
constexpr unsigned long long DIST_NO_D2 = ~0ull;
constexpr double DIST_HUGE = 1.7976931348623157e308;  // the largest finite double

__device__ __forceinline__ bool dist_finite(double x) { return fabs(x) <= DIST_HUGE; }
// a 64-bit word that orders as the double does (finite values, and the infinities at the ends)
__device__ __forceinline__ unsigned long long dist_key(double x) {
	const unsigned long long b = (unsigned long long)__double_as_longlong(x);
	return (b >> 63) ? ~b : b | (1ull << 63);
}
static double dist_unkey(unsigned long long k) {
	const unsigned long long b = (k >> 63) ? k & ~(1ull << 63) : ~k;
	double x;
	memcpy(&x, &b, sizeof x);
	return x;
}
__device__ __forceinline__ double dist_dot(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// The one mapping of a coordinate to a cell of axis a: what bins the triangles, what finds a point's first cell, and what the
// stopping bound is taken from.  Not decreasing in x; !(g >= 0) - a NaN too - gives 0, +inf gives the last cell.
__device__ __forceinline__ int dist_cell(double x, const DistLattice &L, int a) {
	const double g = (x - L.origin[a]) / L.cell[a];
	if (!(g >= 0.0)) return 0;
	if (g >= (double)L.n[a]) return (int)L.n[a] - 1;
	return (int)floor(g);
}

// the corners of triangle i as doubles.  0: an index outside V, nothing was read; 1: a coordinate that is not finite; 2: usable
template <typename R>
__device__ __forceinline__ uint32_t dist_corners(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t i, double a[3], double b[3], double c[3]) {
	const uint32_t *t = T + i * 3u;
	const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
	if (t0 >= nV || t1 >= nV || t2 >= nV) return 0u;
	bool fin = true;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		a[k] = (double)V[(uint64_t)t0 * 3u + k]; b[k] = (double)V[(uint64_t)t1 * 3u + k]; c[k] = (double)V[(uint64_t)t2 * 3u + k];
		fin = fin && dist_finite(a[k]) && dist_finite(b[k]) && dist_finite(c[k]);
	}
	return fin ? 2u : 1u;
}
// per axis the smallest / largest of the three corners: a, replaced by b where b is smaller / larger, then by c likewise
__device__ __forceinline__ void dist_box(const double a[3], const double b[3], const double c[3], double lo[3], double hi[3]) {
#pragma unroll
	for (int k = 0; k < 3; k++) {
		double l = a[k], h = a[k];
		if (b[k] < l) l = b[k];
		if (c[k] < l) l = c[k];
		if (b[k] > h) h = b[k];
		if (c[k] > h) h = c[k];
		lo[k] = l; hi[k] = h;
	}
}

// The closest point q of a usable triangle to p: the region walk of Ericson 5.1.5 in the order and with the comparisons of
// include/mc33_hip.h, then clamped per axis into the triangle's box - q is never NaN and never outside the box, which is what
// the search's pruning rests on.
__device__ __forceinline__ void dist_closest(const double a[3], const double b[3], const double c[3], const double p[3], double q[3]) {
	double ab[3], ac[3], ap[3];
#pragma unroll
	for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
	const double d1 = dist_dot(ab, ap), d2 = dist_dot(ac, ap);
	do {
		if (d1 <= 0.0 && d2 <= 0.0) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; break; }
		double x[3];
#pragma unroll
		for (int k = 0; k < 3; k++) x[k] = p[k] - b[k];
		const double d3 = dist_dot(ab, x), d4 = dist_dot(ac, x);
		if (d3 >= 0.0 && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; break; }
		const double vc = d1 * d4 - d3 * d2;
		if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
			const double v = d1 / (d1 - d3);
#pragma unroll
			for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
			break;
		}
#pragma unroll
		for (int k = 0; k < 3; k++) x[k] = p[k] - c[k];
		const double d5 = dist_dot(ab, x), d6 = dist_dot(ac, x);
		if (d6 >= 0.0 && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; break; }
		const double vb = d5 * d2 - d1 * d6;
		if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
			const double w = d2 / (d2 - d6);
#pragma unroll
			for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
			break;
		}
		const double va = d3 * d6 - d5 * d4;
		if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
			const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
			for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
			break;
		}
		const double den = 1.0 / ((va + vb) + vc);
		const double v = vb * den, w = vc * den;
#pragma unroll
		for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
	} while (0);
	double lo[3], hi[3];
	dist_box(a, b, c, lo, hi);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		if (!(q[k] >= lo[k])) q[k] = lo[k];
		if (!(q[k] <= hi[k])) q[k] = hi[k];
	}
}
__device__ __forceinline__ double dist_d2(const double p[3], const double q[3], double e[3]) {
#pragma unroll
	for (int k = 0; k < 3; k++) e[k] = p[k] - q[k];
	return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// the box of the usable triangles and the counts of the others.  The bounds are exact: a lane keeps the extremes of its finite
// corners, a wave reduces them with comparisons, its first lane lowers / raises the device's keys with integer atomics.
template <typename R>
__global__ __launch_bounds__(256) void k_dist_bounds(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t nT, DistOut *__restrict__ out) {
	double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()}, hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
	uint32_t bad = 0u, nonfinite = 0u, usable = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		double a[3], b[3], c[3], l[3], h[3];
		const uint32_t kind = dist_corners(V, nV, T, i, a, b, c);
		if (kind == 0u) { bad++; continue; }
		if (kind == 1u) { nonfinite++; continue; }
		usable++;
		dist_box(a, b, c, l, h);
#pragma unroll
		for (int k = 0; k < 3; k++) {
			if (l[k] < lo[k]) lo[k] = l[k];
			if (h[k] > hi[k]) hi[k] = h[k];
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const double l = shfl_down_f64(lo[k], d), h = shfl_down_f64(hi[k], d);
			if (l < lo[k]) lo[k] = l;
			if (h > hi[k]) hi[k] = h;
		}
	}
	bad = wave_sum_u32(bad); nonfinite = wave_sum_u32(nonfinite); usable = wave_sum_u32(usable);
	if ((threadIdx.x & 63u) == 0u) {
		if (bad) atomicAdd(&out->bad, (unsigned long long)bad);
		if (nonfinite) atomicAdd(&out->nonfinite, (unsigned long long)nonfinite);
		if (usable) {
			atomicAdd(&out->usable, (unsigned long long)usable);
#pragma unroll
			for (int k = 0; k < 3; k++) {
				atomicMin(&out->lo[k], dist_key(lo[k]));
				atomicMax(&out->hi[k], dist_key(hi[k]));
			}
		}
	}
}

// FILL false: cells[x] += 1 for every cell the box of a usable triangle overlaps; entries: how many in all.  FILL true, behind the
// scan of those counts: the triangle's index into the list of each of those cells, at the place a cursor per cell hands out (the
// order inside a list is not fixed - the winner of a point does not depend on it).
template <typename R, bool FILL>
__global__ __launch_bounds__(256) void k_dist_bin(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t nT, DistLattice L, uint32_t *cells,
                                                  uint32_t *cursor, uint32_t *__restrict__ list, uint64_t entries, DistOut *__restrict__ out) {
	unsigned long long mine = 0ull;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		double a[3], b[3], c[3], lo[3], hi[3];
		if (dist_corners(V, nV, T, i, a, b, c) != 2u) continue;
		dist_box(a, b, c, lo, hi);
		int c0[3], c1[3];
#pragma unroll
		for (int k = 0; k < 3; k++) { c0[k] = dist_cell(lo[k], L, k); c1[k] = dist_cell(hi[k], L, k); }
		for (int z = c0[2]; z <= c1[2]; z++)
			for (int y = c0[1]; y <= c1[1]; y++)
				for (int x = c0[0]; x <= c1[0]; x++) {
					const uint32_t cell = ((uint32_t)z * L.n[1] + (uint32_t)y) * L.n[0] + (uint32_t)x;
					if (FILL) {
						const uint64_t at = (uint64_t)cells[cell] + atomicAdd(&cursor[cell], 1u);  // (cells: the starts, an earlier kernel's)
						if (at < entries) list[at] = (uint32_t)i;
					} else {
						atomicAdd(&cells[cell], 1u);
						mine++;
					}
				}
	}
	if (!FILL) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) mine += shfl_down_u64(mine, d);
		if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(&out->entries, mine);
	}
}

// The hot path: a lane per point, every block a contiguous piece of P.  The point starts from the cell its position clamps to and
// visits the cells at Chebyshev distance r = 0, 1, 2, .. from it that the lattice has: the block of cells within r is tested in
// full after shell r.  Every triangle whose box meets the block is in the list of one of its cells and has been tested; an
// untested one lies, on some axis, wholly in cells below the block or wholly above it, and so does its q (dist_closest clamps q
// into the box, dist_cell does not decrease).  `bound` is the distance from p to the nearest face of the block that has cells
// beyond it, from the same mapping, less the slack: no untested triangle has a computed D2 below bound^2, so the point stops when
// that exceeds its best - equality goes on, an equal D2 with a smaller index may still wait there.  A block that covers the lattice
// has no such face: the point stops with what it has.  A point that is not finite visits nothing.
template <typename R>
__global__ __launch_bounds__(256) void k_dist_query(const R *__restrict__ P, uint64_t nP, uint64_t chunk, const R *__restrict__ V, const uint32_t *__restrict__ T, uint64_t nV,
                                                    DistLattice L, const uint32_t *__restrict__ starts, const uint32_t *__restrict__ list, uint32_t sgn,
                                                    float *__restrict__ oDist, uint32_t *__restrict__ oTri, R *__restrict__ oPoint, unsigned long long *__restrict__ d2bits,
                                                    double *__restrict__ part, DistOut *__restrict__ out) {
	__shared__ double shd[8];
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nP ? beg + chunk : nP;
	double s1 = 0.0, s2 = 0.0;
	unsigned long long tests = 0ull, mx = 0ull, mn = DIST_NO_D2;
	uint32_t matched = 0u;
	const int n0 = (int)L.n[0], n1 = (int)L.n[1], n2 = (int)L.n[2];
	for (uint64_t i = beg + threadIdx.x; i < end; i += 256u) {
		double p[3];
#pragma unroll
		for (int k = 0; k < 3; k++) p[k] = (double)P[i * 3u + k];
		double best = __builtin_huge_val();
		uint32_t bi = MESH_NONE;
		if (n0 && dist_finite(p[0]) && dist_finite(p[1]) && dist_finite(p[2])) {
			const int c0 = dist_cell(p[0], L, 0), c1 = dist_cell(p[1], L, 1), c2 = dist_cell(p[2], L, 2);
			double slack = fmax(fmax(fabs(p[0]), fabs(p[1])), fabs(p[2])) * 0x1p-40;
			slack = slack > L.slack ? slack : L.slack;
			for (int r = 0;; r++) {
				const int x0 = c0 - r > 0 ? c0 - r : 0, x1 = c0 + r < n0 - 1 ? c0 + r : n0 - 1;
				const int y0 = c1 - r > 0 ? c1 - r : 0, y1 = c1 + r < n1 - 1 ? c1 + r : n1 - 1;
				const int z0 = c2 - r > 0 ? c2 - r : 0, z1 = c2 + r < n2 - 1 ? c2 + r : n2 - 1;
				for (int z = z0; z <= z1; z++)
					for (int y = y0; y <= y1; y++) {
						// a row on the shell's z or y faces: all of it; another row: its two ends, where the lattice has them
						const bool face = z == c2 - r || z == c2 + r || y == c1 - r || y == c1 + r;
						const int step = face || !r ? 1 : 2 * r;  // (not a face: r > 0)
						for (int x = face ? x0 : c0 - r; x <= (face ? x1 : c0 + r); x += step) {
							if (x < 0 || x >= n0) continue;
							const uint32_t cell = ((uint32_t)z * (uint32_t)n1 + (uint32_t)y) * (uint32_t)n0 + (uint32_t)x;
							const uint32_t e1 = starts[cell + 1u];
							for (uint32_t e = starts[cell]; e < e1; e++) {
								const uint32_t t = list[e];
								double a[3], b[3], c[3], q[3], d[3];
								(void)dist_corners(V, nV, T, t, a, b, c);  // (a listed triangle is usable)
								dist_closest(a, b, c, p, q);
								const double D2 = dist_d2(p, q, d);
								tests++;
								if (D2 <= DIST_HUGE && (D2 < best || (D2 == best && t < bi))) { best = D2; bi = t; }
							}
						}
					}
				bool open = false;
				double bound = __builtin_huge_val();
#pragma unroll
				for (int k = 0; k < 3; k++) {
					const int b0 = k == 0 ? x0 : k == 1 ? y0 : z0, b1 = k == 0 ? x1 : k == 1 ? y1 : z1;
					if (b0 > 0) {
						const double d = (p[k] - (L.origin[k] + (double)b0 * L.cell[k])) - slack;
						bound = d < bound ? d : bound;
						open = true;
					}
					if (b1 < (int)L.n[k] - 1) {
						const double d = ((L.origin[k] + (double)(b1 + 1) * L.cell[k]) - p[k]) - slack;
						bound = d < bound ? d : bound;
						open = true;
					}
				}
				if (!open) break;
				if (bound > 0.0 && bound * bound > best) break;
			}
		}
		float dist = __builtin_huge_valf();
		unsigned long long bits = DIST_NO_D2;
		R oq[3];
		if (sizeof(R) == 4) { oq[0] = oq[1] = oq[2] = (R)__uint_as_float(0x7FC00000u); }
		else { oq[0] = oq[1] = oq[2] = (R)__longlong_as_double(0x7FF8000000000000ll); }
		if (bi != MESH_NONE) {
			double a[3], b[3], c[3], q[3], e[3];
			(void)dist_corners(V, nV, T, bi, a, b, c);
			dist_closest(a, b, c, p, q);
			(void)dist_d2(p, q, e);  // (== best: the same function of the same inputs)
			const double root = sqrt(best);
			dist = (float)root;
			if (sgn) {
				double ab[3], ac[3], nn[3];
#pragma unroll
				for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; }
				nn[0] = ab[1] * ac[2] - ab[2] * ac[1];
				nn[1] = ab[2] * ac[0] - ab[0] * ac[2];
				nn[2] = ab[0] * ac[1] - ab[1] * ac[0];
				if (dist_dot(e, nn) < 0.0) dist = -dist;
			}
			oq[0] = (R)q[0]; oq[1] = (R)q[1]; oq[2] = (R)q[2];
			bits = (unsigned long long)__double_as_longlong(best);
			s1 += root; s2 += best;
			matched++;
			mx = bits > mx ? bits : mx;
			mn = bits < mn ? bits : mn;
		}
		if (oDist) oDist[i] = dist;
		if (oTri) oTri[i] = bi;
		if (oPoint) { oPoint[i * 3u] = oq[0]; oPoint[i * 3u + 1u] = oq[1]; oPoint[i * 3u + 2u] = oq[2]; }
		d2bits[i] = bits;
	}
	// the block's two sums, always in this order: down the lanes of a wave, then wave 0 .. 3
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		s1 += shfl_down_f64(s1, d); s2 += shfl_down_f64(s2, d);
		tests += shfl_down_u64(tests, d);
		const unsigned long long ox = shfl_down_u64(mx, d), on = shfl_down_u64(mn, d);
		mx = ox > mx ? ox : mx;
		mn = on < mn ? on : mn;
	}
	matched = wave_sum_u32(matched);
	if ((threadIdx.x & 63u) == 0u) {
		shd[threadIdx.x >> 6] = s1; shd[4u + (threadIdx.x >> 6)] = s2;
		if (matched) {
			atomicAdd(&out->matched, (unsigned long long)matched);
			atomicMax(&out->max_bits, mx);
			atomicMin(&out->min_bits, mn);
		}
		if (tests) atomicAdd(&out->tests, tests);
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		part[(uint64_t)blockIdx.x * 2u] = ((shd[0] + shd[1]) + shd[2]) + shd[3];
		part[(uint64_t)blockIdx.x * 2u + 1u] = ((shd[4] + shd[5]) + shd[6]) + shd[7];
	}
}

// the smallest point index whose winning D2 is the largest / the smallest (max_bits, min_bits: the query's, a kernel ago)
__global__ __launch_bounds__(256) void k_dist_arg(const unsigned long long *__restrict__ d2bits, uint64_t nP, DistOut *out) {
	const unsigned long long mx = out->max_bits, mn = out->min_bits;
	unsigned long long amax = ~0ull, amin = ~0ull;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nP; i += (uint64_t)gridDim.x * 256u) {
		const unsigned long long b = d2bits[i];
		if (b == DIST_NO_D2) continue;
		if (b == mx && amax == ~0ull) amax = i;  // (a lane's indices ascend)
		if (b == mn && amin == ~0ull) amin = i;
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {  // (the surface against itself: every point attains the minimum - one atomic a wave, not a lane)
		const unsigned long long ox = shfl_down_u64(amax, d), on = shfl_down_u64(amin, d);
		amax = ox < amax ? ox : amax;
		amin = on < amin ? on : amin;
	}
	if ((threadIdx.x & 63u) == 0u) {
		if (amax != ~0ull) atomicMin(&out->argmax, amax);
		if (amin != ~0ull) atomicMin(&out->argmin, amin);
	}
}

// one block: the per-block sums in index order.  The lanes fetch 256 pairs side by side, lane 0 adds them one after the other.
__global__ __launch_bounds__(256) void k_dist_sum(const double *__restrict__ part, uint32_t blocks, DistOut *__restrict__ out) {
	__shared__ double sh[512];
	double s1 = 0.0, s2 = 0.0;
	for (uint32_t base = 0; base < blocks; base += 256u) {  // (block-uniform)
		const uint32_t k = base + threadIdx.x;
		__syncthreads();
		if (k < blocks) { sh[threadIdx.x] = part[(uint64_t)k * 2u]; sh[256u + threadIdx.x] = part[(uint64_t)k * 2u + 1u]; }
		__syncthreads();
		if (threadIdx.x == 0u) {
			const uint32_t n = blocks - base < 256u ? blocks - base : 256u;
			for (uint32_t j = 0; j < n; j++) { s1 += sh[j]; s2 += sh[256u + j]; }
		}
	}
	if (threadIdx.x == 0u) { out->sum = s1; out->sum_sq = s2; }
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void dist_release(void *state) {
	DistState *s = (DistState *)state;
	dev_release(&s->d_cells); dev_release(&s->d_cursor); dev_release(&s->d_list); dev_release(&s->d_d2); dev_release(&s->d_part);
	for (int k = 0; s->ev_made && k < 6; k++) (void)hipEventDestroy(s->ev[k]);
	s->ev_made = false;
}

static uint32_t distance_cells_switch() {  // MC33_HIP_DISTANCE_CELLS, read when a context is created: 0 / not set = the library decides
	const char *e = getenv("MC33_HIP_DISTANCE_CELLS");
	if (!e || !*e) return 0u;
	const unsigned long long v = strtoull(e, nullptr, 10);
	return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

// The lattice over the box lo .. hi of `usable` triangles: `per_axis` cells along the longest axis, the others in proportion, an
// axis without extent one cell.  forced != 0 (MC33_HIP_DISTANCE_CELLS): that many cells on every axis with an extent.  Either way
// at most DIST_MAX_CELLS per axis and about 8 cells per triangle in all - a point far from every triangle walks the whole lattice,
// and a triangle is listed in every cell its box overlaps.
static void dist_lattice(const double lo[3], const double hi[3], uint64_t usable, uint32_t forced, uint32_t shrink, DistLattice *L) {
	double ext[3], longest = 0.0, mag = 0.0;
	for (int k = 0; k < 3; k++) {
		ext[k] = hi[k] - lo[k];
		if (!(ext[k] > 0.0) || !std::isfinite(ext[k])) ext[k] = 0.0;  // (a box wider than the doubles reach: one cell)
		longest = std::max(longest, ext[k]);
		mag = std::max(mag, std::max(fabs(lo[k]), fabs(hi[k])));
	}
	const double own = std::min((double)DIST_MAX_CELLS, floor(cbrt(8.0 * (double)usable + 512.0)));
	double per_axis = forced ? std::min((double)forced, own) : std::min(own, ceil(sqrt((double)usable / 16.0)));
	per_axis = std::max(1.0, floor(per_axis / (double)shrink));
	for (int k = 0; k < 3; k++) {
		double n = ext[k] > 0.0 ? (forced ? per_axis : ceil(per_axis * (ext[k] / longest))) : 1.0;
		n = std::min(std::max(n, 1.0), per_axis);
		L->n[k] = (uint32_t)n;
		L->origin[k] = lo[k];
		L->cell[k] = ext[k] > 0.0 ? ext[k] / n : 1.0;
		if (!(L->cell[k] > 0.0)) { L->cell[k] = 1.0; L->n[k] = 1u; }  // (an extent that underflows when divided)
	}
	L->slack = mag * 0x1p-40;
	L->pad_ = 0u;
}

extern "C" int mc33hip_surface_distance(mc33hip_ctx *c, mc33hip_distance *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->matched_points = a->unmatched_points = a->invalid_triangles = a->nonfinite_triangles = a->argmax = a->argmin = a->triangle_tests = 0;
	a->max = a->min = a->sum = a->sum_sq = 0.0;
	a->lattice[0] = a->lattice[1] = a->lattice[2] = 0u;
	const unsigned long long nP = a->nP, nV = a->nV, nT = a->nT;
	if (nP > 0xFFFFFFFFull || !mesh_sizes_ok(nV, nT)) { set_err("more than 2^32-1 points, vertices or triangles"); return MC33HIP_EINVAL; }
	if ((nP && !a->P) || (nV && !a->V) || (nT && !a->T)) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	const MeshRange in[3] = {{a->P, nP * 3u * sizeof(real_t)}, {a->V, nV * 3u * sizeof(real_t)}, {a->T, nT * 12u}};
	const MeshRange outs[3] = {{a->oDist, nP * 4u}, {a->oTri, nP * 4u}, {a->oPoint, nP * 3u * sizeof(real_t)}};
	if (!mesh_ranges_ok(in, 3, outs, 3, true, "distance")) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	DistState *s;
	if ((rc = mesh_op_state(&c->meas->mesh, dist_release, &s))) return rc;
	MeshHost &h = c->meas->mesh;
	const real_t *P = (const real_t *)a->P, *V = (const real_t *)a->V;
	const uint32_t *T = (const uint32_t *)a->T;
	const bool timing = c->timing_level >= 2;
	if (timing && !s->ev_made) {
		for (int k = 0; k < 6; k++) HIP_TRY(hipEventCreate(&s->ev[k]));
		s->ev_made = true;
	}
	s->timed = false;
#define DIST_MARK(k) do { if (timing) HIP_TRY(hipEventRecord(s->ev[k], c->stream)); } while (0)
	const uint32_t gridT = meas_grid(c, nT, 16u);
	DistOut zero;
	memset(&zero, 0, sizeof zero);
	zero.lo[0] = zero.lo[1] = zero.lo[2] = zero.min_bits = zero.argmax = zero.argmin = ~0ull;
	*s->h_out = zero;  // (pinned: the copy reads it when it runs, and nothing writes it before the fetch below)
	HIP_TRY(hipMemcpyAsync(s->d_out, s->h_out, sizeof zero, hipMemcpyHostToDevice, c->stream));
	DIST_MARK(0);
	if (nT) hipLaunchKernelGGL((k_dist_bounds<real_t>), dim3(gridT), dim3(256), 0, c->stream, V, (uint64_t)nV, T, (uint64_t)nT, s->d_out);
	DIST_MARK(1);
	if ((rc = mesh_op_fetch(c, s))) return rc;  // the box, for the lattice
	DistLattice L;
	memset(&L, 0, sizeof L);
	uint64_t entries = 0u;
	DIST_MARK(2);
	if (s->h_out->usable) {
		double lo[3], hi[3];
		for (int k = 0; k < 3; k++) { lo[k] = dist_unkey(s->h_out->lo[k]); hi[k] = dist_unkey(s->h_out->hi[k]); }
		// the lists of a lattice name at most 2^32-1 triangles (the scan's sums are 32-bit words): a coarser one until they do -
		// one cell names every usable triangle once
		for (uint32_t shrink = 1u;; shrink *= 2u) {
			dist_lattice(lo, hi, s->h_out->usable, c->sw.distance_cells, shrink, &L);
			const uint64_t cells = (uint64_t)L.n[0] * L.n[1] * L.n[2];
			if ((rc = meas_room(&s->d_cells, &s->cells_cap, cells + 1u))) return rc;
			if ((rc = meas_room(&s->d_cursor, &s->cursor_cap, cells))) return rc;
			if ((rc = meas_room(&h.d_bsum, &h.bsum_cap, (cells + MESH_TILE - 1u) / MESH_TILE))) return rc;
			HIP_TRY(hipMemsetAsync(s->d_cells, 0, (cells + 1u) * 4u, c->stream));
			HIP_TRY(hipMemsetAsync(s->d_cursor, 0, cells * 4u, c->stream));
			HIP_TRY(hipMemsetAsync(&s->d_out->entries, 0, sizeof(unsigned long long), c->stream));
			hipLaunchKernelGGL((k_dist_bin<real_t, false>), dim3(gridT), dim3(256), 0, c->stream, V, (uint64_t)nV, T, (uint64_t)nT, L, s->d_cells, s->d_cursor,
			                   (uint32_t *)nullptr, (uint64_t)0u, s->d_out);
			mesh_scan<MeshCount, MESH_STARTS>(c, s->d_cells, cells, h.d_bsum, nullptr, s->d_cells);
			if ((rc = mesh_op_fetch(c, s))) return rc;  // the entries, for the list
			entries = s->h_out->entries;
			if (entries <= 0xFFFFFFFFull || cells == 1u) break;
		}
		if ((rc = meas_room(&s->d_list, &s->list_cap, entries))) return rc;
		hipLaunchKernelGGL((k_dist_bin<real_t, true>), dim3(gridT), dim3(256), 0, c->stream, V, (uint64_t)nV, T, (uint64_t)nT, L, s->d_cells, s->d_cursor, s->d_list,
		                   entries, s->d_out);
	}
	DIST_MARK(3);
	uint32_t gridP = 0u;
	if (nP) {
		gridP = meas_grid(c, nP, 16u);
		const uint64_t chunk = (nP + gridP - 1u) / gridP;
		if ((rc = meas_room(&s->d_d2, &s->d2_cap, nP))) return rc;
		if ((rc = meas_room(&s->d_part, &s->part_cap, (uint64_t)gridP * 2u))) return rc;
		hipLaunchKernelGGL((k_dist_query<real_t>), dim3(gridP), dim3(256), 0, c->stream, P, (uint64_t)nP, chunk, V, T, (uint64_t)nV, L, (const uint32_t *)s->d_cells,
		                   (const uint32_t *)s->d_list, a->signed_distance ? 1u : 0u, a->oDist, (uint32_t *)a->oTri, (real_t *)a->oPoint, s->d_d2, s->d_part, s->d_out);
	}
	DIST_MARK(4);
	if (nP) {
		hipLaunchKernelGGL(k_dist_arg, dim3(meas_grid(c, nP, 16u)), dim3(256), 0, c->stream, (const unsigned long long *)s->d_d2, (uint64_t)nP, s->d_out);
		hipLaunchKernelGGL(k_dist_sum, dim3(1), dim3(256), 0, c->stream, (const double *)s->d_part, gridP, s->d_out);
	}
	DIST_MARK(5);
#undef DIST_MARK
	if ((rc = mesh_op_fetch(c, s))) return rc;
	if (timing) {
		float bounds_ms, bin_ms;
		HIP_TRY(hipEventElapsedTime(&bounds_ms, s->ev[0], s->ev[1]));
		HIP_TRY(hipEventElapsedTime(&bin_ms, s->ev[2], s->ev[3]));
		s->ms[0] = bounds_ms + bin_ms;
		HIP_TRY(hipEventElapsedTime(&s->ms[1], s->ev[3], s->ev[4]));
		HIP_TRY(hipEventElapsedTime(&s->ms[2], s->ev[4], s->ev[5]));
		s->timed = true;
	}
	const DistOut o = *s->h_out;
	a->matched_points = o.matched; a->unmatched_points = nP - o.matched;
	a->invalid_triangles = o.bad; a->nonfinite_triangles = o.nonfinite;
	a->triangle_tests = o.tests;
	for (int k = 0; k < 3; k++) a->lattice[k] = L.n[k];
	if (o.matched) {
		double mx, mn;
		memcpy(&mx, &o.max_bits, sizeof mx); memcpy(&mn, &o.min_bits, sizeof mn);
		a->max = sqrt(mx); a->min = sqrt(mn);
		a->argmax = o.argmax; a->argmin = o.argmin;
		a->sum = o.sum; a->sum_sq = o.sum_sq;
	}
	return mesh_bad(o.bad, nV);
}

extern "C" int mc33hip_distance_timing(mc33hip_ctx *c, float ms[3]) {
	MeshOp *op = c && c->meas && ms ? mesh_op_peek(&c->meas->mesh, dist_release) : nullptr;
	const DistState *s = op ? (const DistState *)op->state : nullptr;
	if (!s || !s->timed) { set_err("no timed distance call on this context (MC33_HIP_TIMING >= 2 when it is created)"); return MC33HIP_EINVAL; }
	for (int k = 0; k < 3; k++) ms[k] = s->ms[k];
	return MC33HIP_OK;
}
