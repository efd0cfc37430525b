// mc33_cap.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h and the scratch helpers of mc33_measure.hip.h; not a header to include elsewhere):
// a FINISHED V, N, T in device memory closed at the six faces of a box of grid points - on a face the solid region is a marching-
// squares problem on a plane of samples that is resident, and the rim of the cap is the surface's own boundary - so that what
// measures a volume, wants a closed component or goes to a printer gets one mesh without boundary (include/mc33_hip.h:
// mc33hip_cap_surface).  DESIGN.md 23.
//
// The definition is in include/mc33_hip.h; tests/cap_oracle.py restates it in numpy, step for step.  Which side is a rim segment,
// which cell it belongs to, which cells are regular, where a row lands and what it holds are decided by integer atomics whose
// result does not depend on their order (sums, minima, maxima, ors), exclusive scans and IEEE double arithmetic with nothing fused:
// the result is an exact function of the input.
//
// The solid side is the side the stored winding turns its back on.  The extractor winds every triangle so that its normal by
// winding points where F falls, and stores N on that side too (store_vertex: N = -grad F normalised; emit: MC:1246-1250): the plain
// libraries turn their back on F > iso - "above" is solid, the README sphere of the reference, whose inside is below, has volume
// < 0 - and normal_neg exchanges both, winding and N: the _nneg flavours have "below" solid.  In every flavour N lies on the side of
// the winding, so the N of a cap vertex is the outward normal of its faces with the sign +; invert exchanges winding and N of the
// surface together and leaves that as it is.
//
// The passes: k_cap_flag, a lane per vertex, leaves the faces a vertex lies on in a byte; k_cap_sides, a lane per triangle, enters
// every side into the table of mc33_mesh.hip.h and adds 1 << 40 | i << 2 | e to the word behind the key - a side used once is the
// one whose word has the count 1, and then the word names it; k_cap_rim, a lane per triangle, looks its sides up again and gives
// every rim segment to its face cell: a minimum, a maximum and a count per cell, which is all a regular cell can hold; k_cap_cell, a
// lane per face cell and a launch per face, reads the four samples, decides whether the cell is regular, counts its triangles and ors the face into the
// word of every grid point its polygons name; two tile scans, over the triangles of the cells and over the points named;
// k_cap_emit, a lane per cell, makes the polygons again and writes them; k_cap_verts, a lane per named point, writes its rows;
// k_cap_invert exchanges and negates.  Why every side goes through the table, not only the sides with both ends on a face:
// off_face_edges counts the sides used once that lie on NO face, and whether a side is used once is known only when all are in.

struct CapSlot { unsigned long long key, word; };  // 16 bytes; word: the sum over the uses of 1 << 40 | i << 2 | e
constexpr unsigned long long CAP_USE = 1ull << 40;

struct CapOut {             // what a call brings to the host (device copy and pinned twin)
	unsigned long long capv, capt, rim, capped, skipped, off, bad, nonfinite, used, full;
	unsigned long long pad_[2];
};

struct CapState {           // scratch of these passes besides the shared keep (the face byte of a vertex) and tile sums (the cell tiles, behind them
                            // the point tiles): on the MeasureState from the first call on, grown on demand, freed with it
	CapOut *d_out, *h_out;
	CapSlot *d_slots;       // the table of sides: a power of two >= 4 nT slots
	uint64_t slots_cap;
	unsigned long long *d_segmin, *d_segmax;  // [cells] the smallest and the largest word of the cell's segments
	uint32_t *d_cnt, *d_rank;                 // [cells] its segments; the triangles of the cells before it
	uint8_t *d_ntri;                          // [cells] its triangles
	uint64_t cells_cap;
	uint32_t *d_use, *d_new;                  // [points] the faces whose polygons name the point; its rank among the named
	uint64_t points_cap;
};

struct CapBox {
	uint32_t lo[3], hi[3], b[3];   // the box in grid points, points per axis
	uint32_t face_off[7];          // the cells of the faces before face f; [6]: all
	uint64_t plane, ring, points;  // points of a z face, of the ring of a plane between them, of the box's surface
	uint64_t pitch, slice;         // of the resident grid, in samples
	double r0[3], rd[3], tol[3];   // origin, 1 / spacing, the tolerance of step 1
	real_t iso, O[3], D[3];
	uint32_t solid_above, invert;
};

__device__ __forceinline__ bool cap_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for a NaN)
template <typename X>
__device__ __forceinline__ X cap_pick(const X v[3], uint32_t k) { return k == 0u ? v[0] : (k == 1u ? v[1] : v[2]); }
// the in-plane axes of a face: u, the faster one, and w
__host__ __device__ __forceinline__ uint32_t cap_u(uint32_t f) { return (f >> 1) == 0u ? 1u : 0u; }
__host__ __device__ __forceinline__ uint32_t cap_w(uint32_t f) { return (f >> 1) == 2u ? 1u : 2u; }
// P0 P1 P2 P3 of a face cell run clockwise as seen from outside: x-lo, y-hi, z-lo
__device__ __forceinline__ bool cap_flip(uint32_t f) { return f == 0u || f == 3u || f == 4u; }

// step 1: the grid coordinate of x, an integer where x lies within tol of one.  rd = 1 / d, rounded once on the host: a product, not
// a quotient - a lane of k_cap_cell forms eight of these side by side, and eight IEEE double divisions do not fit 64 registers
__device__ __forceinline__ double cap_raw(double x, double r0, double rd) { return (x - r0) * rd; }
__device__ __forceinline__ double cap_snap(double g, double tol) {
	const double r = floor(g + 0.5);
	return fabs(g - r) <= tol ? r : g;  // (false for a NaN)
}
__device__ __forceinline__ double cap_g(double x, double r0, double rd, double tol) { return cap_snap(cap_raw(x, r0, rd), tol); }

// a triangle as the caps see it: with invert, the second and third index exchanged
__device__ __forceinline__ void cap_tri(const uint32_t *__restrict__ T, uint64_t i, uint32_t invert, uint32_t &t0, uint32_t &t1, uint32_t &t2) {
	const uint32_t *t = T + i * 3u;
	const uint32_t a = t[1], b = t[2];
	t0 = t[0]; t1 = invert ? b : a; t2 = invert ? a : b;
}
__device__ __forceinline__ unsigned long long cap_key(uint32_t p, uint32_t q) {
	return p < q ? ((unsigned long long)p << 32) | q : ((unsigned long long)q << 32) | p;
}

template <typename R>
__global__ __launch_bounds__(256) void k_cap_flag(const R *__restrict__ V, uint64_t nV, CapBox B, uint8_t *__restrict__ flag, CapOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t nonf = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const R *p = V + v * 3u;
		uint32_t bits = 0u;
		bool fin = true;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const double x = (double)p[a];
			fin = fin && cap_finite(x);
			const double g = cap_g(x, B.r0[a], B.rd[a], B.tol[a]);
			if (g == (double)B.lo[a]) bits |= 1u << (2 * a);
			if (g == (double)B.hi[a]) bits |= 2u << (2 * a);
		}
		flag[v] = (uint8_t)bits;
		nonf += fin ? 0u : 1u;
	}
	nonf = block_sum_u32_256(nonf, sh);
	if (threadIdx.x == 0u && nonf) atomicAdd(&out->nonfinite, (unsigned long long)nonf);
}

__global__ __launch_bounds__(256) void k_cap_sides(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, uint32_t invert, CapSlot *slots, uint64_t mask,
                                                   CapOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t bad = 0u, full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		uint32_t t0, t1, t2;
		cap_tri(T, i, invert, t0, t1, t2);
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
#pragma unroll
		for (uint32_t e = 0; e < 3u; e++) {
			const uint32_t p = e == 0u ? t0 : e == 1u ? t1 : t2, q = e == 0u ? t1 : e == 1u ? t2 : t0;
			if (p == q) continue;
			const uint64_t s = mesh_claim(slots, mask, cap_key(p, q));
			if (s == MESH_NOSLOT) full++;
			else atomicAdd(&slots[s].word, CAP_USE | ((unsigned long long)i << 2) | e);
		}
	}
	bad = block_sum_u32_256(bad, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (bad) atomicAdd(&out->bad, (unsigned long long)bad);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// step 2: the sides used once - off a face, or a rim segment into its cell
template <typename R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_cap_rim(const R *__restrict__ V, const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, CapBox B,
                                                 const uint8_t *__restrict__ flag, const CapSlot *__restrict__ slots, uint64_t mask, unsigned long long *segmin,
                                                 unsigned long long *segmax, uint32_t *cnt, CapOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t rim = 0u, off = 0u, full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		uint32_t t0, t1, t2;
		cap_tri(T, i, B.invert, t0, t1, t2);
		if (t0 >= nV || t1 >= nV || t2 >= nV) continue;
#pragma unroll
		for (uint32_t e = 0; e < 3u; e++) {
			const uint32_t p = e == 0u ? t0 : e == 1u ? t1 : t2, q = e == 0u ? t1 : e == 1u ? t2 : t0;
			if (p == q) continue;
			const uint64_t s = mesh_find(slots, mask, cap_key(p, q));
			if (s == MESH_NOSLOT) { full++; continue; }
			if ((slots[s].word >> 40) != 1ull) continue;
			const uint32_t common = (uint32_t)flag[p] & (uint32_t)flag[q];
			if (!common) { off++; continue; }
			const uint32_t f = (uint32_t)__ffs((int)common) - 1u, u = cap_u(f), w = cap_w(f);
			const R *vp = V + (uint64_t)p * 3u, *vq = V + (uint64_t)q * 3u;
			const double r0u = cap_pick(B.r0, u), du = cap_pick(B.rd, u), tu = cap_pick(B.tol, u);
			const double r0w = cap_pick(B.r0, w), dw = cap_pick(B.rd, w), tw = cap_pick(B.tol, w);
			const double pu = (double)(u == 0u ? vp[0] : vp[1]), qu = (double)(u == 0u ? vq[0] : vq[1]);
			const double pw = (double)(w == 1u ? vp[1] : vp[2]), qw = (double)(w == 1u ? vq[1] : vq[2]);
			// inside the box by the snapped coordinates; the cell by the coordinates as they are - an end within tol of a grid line, snapped
			// onto it, would carry a midpoint over the line when the other end lies on it
			const double gpu = cap_raw(pu, r0u, du), gqu = cap_raw(qu, r0u, du), gpw = cap_raw(pw, r0w, dw), gqw = cap_raw(qw, r0w, dw);
			const double mu = (cap_snap(gpu, tu) + cap_snap(gqu, tu)) * 0.5;
			const double mw = (cap_snap(gpw, tw) + cap_snap(gqw, tw)) * 0.5;
			const uint32_t lou = cap_pick(B.lo, u), hiu = cap_pick(B.hi, u), low = cap_pick(B.lo, w), hiw = cap_pick(B.hi, w);
			if (!(mu >= (double)lou && mu <= (double)hiu && mw >= (double)low && mw <= (double)hiw)) { off++; continue; }
			const double ru = floor((gpu + gqu) * 0.5), rw = floor((gpw + gqw) * 0.5);
			const uint32_t cu = !(ru > (double)lou) ? lou : (ru < (double)(hiu - 1u) ? (uint32_t)ru : hiu - 1u);
			const uint32_t cw = !(rw > (double)low) ? low : (rw < (double)(hiw - 1u) ? (uint32_t)rw : hiw - 1u);
			const uint64_t cell = (uint64_t)B.face_off[f] + (uint64_t)(cw - low) * (hiu - lou) + (cu - lou);
			const unsigned long long word = ((unsigned long long)i << 2) | e;
			atomicMin(&segmin[cell], word);
			atomicMax(&segmax[cell], word);
			atomicAdd(&cnt[cell], 1u);
			rim++;
		}
	}
	rim = block_sum_u32_256(rim, sh);
	off = block_sum_u32_256(off, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (rim) atomicAdd(&out->rim, (unsigned long long)rim);
		if (off) atomicAdd(&out->off, (unsigned long long)off);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// --- steps 3 and 4: one face cell ----------------------------------------------------------------------------------------------------------

struct CapCell {            // where a face cell lies
	uint32_t f, cu, cw;     // its face, its place in the plane (absolute grid indices)
};
__device__ __forceinline__ CapCell cap_cell_of(const CapBox &B, uint32_t f, uint32_t r) {  // cell r of face f, u the faster index
	CapCell c;
	c.f = f;
	const uint32_t u = cap_u(f), w = cap_w(f);
	const uint32_t lou = cap_pick(B.lo, u), nu = cap_pick(B.hi, u) - lou;
	c.cu = lou + r % nu;
	c.cw = cap_pick(B.lo, w) + r / nu;
	return c;
}
// corner k of the cell, counterclockwise as seen from outside from P0: its steps in the plane, its grid point
__device__ __forceinline__ void cap_corner(const CapBox &B, const CapCell &c, uint32_t k, uint32_t p[3]) {
	const bool flip = cap_flip(c.f);
	const uint32_t su = (k == 2u || k == (flip ? 3u : 1u)) ? 1u : 0u, sw = (k == 2u || k == (flip ? 1u : 3u)) ? 1u : 0u;
	const uint32_t a = c.f >> 1, fixed = (c.f & 1u) ? cap_pick(B.hi, a) : cap_pick(B.lo, a);
	const uint32_t pu = c.cu + su, pw = c.cw + sw;
	p[0] = a == 0u ? fixed : pu;
	p[1] = a == 1u ? fixed : (a == 0u ? pu : pw);
	p[2] = a == 2u ? fixed : pw;
}
// the place of a point of the box's surface among all of them, in ascending order of the grid point index
__device__ __forceinline__ uint64_t cap_point_index(const CapBox &B, const uint32_t p[3]) {
	const uint32_t x = p[0] - B.lo[0], y = p[1] - B.lo[1], z = p[2] - B.lo[2];
	const uint32_t bx = B.b[0], by = B.b[1], bz = B.b[2];
	if (z == 0u) return (uint64_t)y * bx + x;
	if (z == bz - 1u) return B.plane + (uint64_t)(bz - 2u) * B.ring + (uint64_t)y * bx + x;
	const uint64_t base = B.plane + (uint64_t)(z - 1u) * B.ring;
	if (y == 0u) return base + x;
	if (y == by - 1u) return base + bx + 2ull * (by - 2u) + x;
	return base + bx + 2ull * (y - 1u) + (x ? 1u : 0u);
}

// the solid bit of a grid point, and bit 4 of the result when the sample is the isovalue or a NaN
__device__ __forceinline__ uint32_t cap_class(const CapBox &B, const sample_t *__restrict__ grid, const uint32_t p[3]) {
	const real_t v = iso_diff(B.iso, (real_t)grid[(uint64_t)p[2] * B.slice + (uint64_t)p[1] * B.pitch + p[0]]);
	if (v != v || v == (real_t)0) return 16u;
	const uint32_t above = sign_of(v);
	return above == B.solid_above ? 1u : 0u;
}

// the two ends a -> b of the segment `word` = i << 2 | e
__device__ __forceinline__ void cap_ends(const uint32_t *__restrict__ T, const CapBox &B, unsigned long long word, uint32_t &a, uint32_t &b) {
	uint32_t t0, t1, t2;
	cap_tri(T, word >> 2, B.invert, t0, t1, t2);
	const uint32_t e = (uint32_t)word & 3u;
	a = e == 0u ? t0 : e == 1u ? t1 : t2;
	b = e == 0u ? t1 : e == 1u ? t2 : t0;
}

// bit k: corner k lies on the positive side of b -> a in the plane of the face, counterclockwise as seen from outside
template <typename R>
__device__ __forceinline__ uint32_t cap_positive(const R *__restrict__ V, const CapBox &B, const CapCell &c, uint32_t a, uint32_t b) {
	const uint32_t u = cap_u(c.f), w = cap_w(c.f);
	const R *va = V + (uint64_t)a * 3u, *vb = V + (uint64_t)b * 3u;
	const double r0u = cap_pick(B.r0, u), du = cap_pick(B.rd, u), tu = cap_pick(B.tol, u);
	const double r0w = cap_pick(B.r0, w), dw = cap_pick(B.rd, w), tw = cap_pick(B.tol, w);
	const double au = cap_g((double)(u == 0u ? va[0] : va[1]), r0u, du, tu), bu = cap_g((double)(u == 0u ? vb[0] : vb[1]), r0u, du, tu);
	const double aw = cap_g((double)(w == 1u ? va[1] : va[2]), r0w, dw, tw), bw = cap_g((double)(w == 1u ? vb[1] : vb[2]), r0w, dw, tw);
	const bool flip = cap_flip(c.f);
	uint32_t bits = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint32_t su = (k == 2u || k == (flip ? 3u : 1u)) ? 1u : 0u, sw = (k == 2u || k == (flip ? 1u : 3u)) ? 1u : 0u;
		const double x = (double)(c.cu + su), y = (double)(c.cw + sw);
		const double p = (au - bu) * (y - bw);
		const double q = (aw - bw) * (x - bu);
		const double s = p - q;
		if ((flip ? -s : s) > 0.0) bits |= 1u << k;
	}
	return bits;
}

// The polygons of a cell: up to six entries - a vertex of the surface, or a corner 0 .. 3 where `corners` has the entry's bit - as
// one polygon fanned from its first entry, or - two - as two triangles.  state: 0 nothing here, 1 regular, 2 skipped.
struct CapPlan {
	uint32_t e0, e1, e2, e3, e4, e5;
	uint32_t n, corners, two, state, segs;
	__device__ __forceinline__ uint32_t triangles() const { return state != 1u || !n ? 0u : (two ? 2u : n - 2u); }
	__device__ __forceinline__ uint32_t named() const {  // bit k: a polygon names corner k
		return ((corners & 1u) ? 1u << e0 : 0u) | ((corners & 2u) ? 1u << e1 : 0u) | ((corners & 4u) ? 1u << e2 : 0u) | ((corners & 8u) ? 1u << e3 : 0u) |
		       ((corners & 16u) ? 1u << e4 : 0u) | ((corners & 32u) ? 1u << e5 : 0u);
	}
};
__device__ __forceinline__ uint32_t cap_one_bit(uint32_t m) { return (uint32_t)__ffs((int)m) - 1u; }

template <typename R>
__device__ __forceinline__ CapPlan cap_plan(const R *__restrict__ V, const uint32_t *__restrict__ T, const sample_t *__restrict__ grid, const CapBox &B, const CapCell &c,
                                            uint32_t nseg, unsigned long long wmin, unsigned long long wmax) {
	CapPlan g;
	g.e0 = g.e1 = g.e2 = g.e3 = g.e4 = g.e5 = 0u;
	g.n = g.corners = g.two = g.state = 0u;
	g.segs = nseg;
	uint32_t solid = 0u, bad = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		uint32_t p[3];
		cap_corner(B, c, k, p);
		const uint32_t cl = cap_class(B, grid, p);
		solid |= (cl & 1u) << k;
		bad |= cl >> 4;
	}
	if (!solid && !nseg) return g;
	g.state = 2u;
	if (bad) return g;
	const uint32_t ns = (uint32_t)__popc(solid);
	const bool diagonal = solid == 5u || solid == 10u;
	const uint32_t expect = (ns == 0u || ns == 4u) ? 0u : (diagonal ? 2u : 1u);
	if (nseg != expect) return g;
	g.state = 1u;
	if (ns == 0u) return g;
	if (ns == 4u) {
		g.e0 = 0u; g.e1 = 1u; g.e2 = 2u; g.e3 = 3u;
		g.n = 4u; g.corners = 15u;
		return g;
	}
	if (expect == 1u) {
		uint32_t a, b;
		cap_ends(T, B, wmin, a, b);
		// the solid corner whose clockwise neighbour is not solid
		const uint32_t first = cap_one_bit(solid & ~(((solid << 1) | (solid >> 3)) & 15u));
		g.e0 = b; g.e1 = a;
		g.e2 = first; g.e3 = (first + 1u) & 3u; g.e4 = (first + 2u) & 3u;
		g.n = 2u + ns;
		g.corners = ((1u << ns) - 1u) << 2;
		return g;
	}
	uint32_t a1 = 0u, b1 = 0u, a2 = 0u, b2 = 0u, pos1 = 0u, pos2 = 0u;
#pragma unroll 1
	for (uint32_t j = 0; j < 2u; j++) {  // (one segment at a time: the divisions of one are not kept beside those of the other)
		uint32_t a, b;
		cap_ends(T, B, j ? wmax : wmin, a, b);
		const uint32_t pos = cap_positive(V, B, c, a, b);
		if (j) { a2 = a; b2 = b; pos2 = pos; } else { a1 = a; b1 = b; pos1 = pos; }
	}
	const uint32_t empty = solid ^ 15u;
	const uint32_t cut1 = pos1 & solid, cut2 = pos2 & solid;
	g.e0 = b1; g.e1 = a1; g.e3 = b2; g.e4 = a2;
	g.n = 6u; g.corners = (1u << 2) | (1u << 5);
	if (__popc(cut1) == 1 && __popc(cut2) == 1 && cut1 != cut2) {  // every segment cuts off a solid corner of its own
		g.e2 = cap_one_bit(cut1); g.e5 = cap_one_bit(cut2);
		g.two = 1u;
		return g;
	}
	const uint32_t out1 = ~pos1 & empty, out2 = ~pos2 & empty;
	if (cut1 == solid && cut2 == solid && __popc(out1) == 1 && __popc(out2) == 1 && out1 != out2) {  // the solid corner behind the empty one a segment cuts off
		g.e2 = (cap_one_bit(out1) + 1u) & 3u; g.e5 = (cap_one_bit(out2) + 1u) & 3u;
		return g;
	}
	g.state = 2u; g.n = 0u; g.corners = 0u;
	return g;
}

template <typename R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_cap_cell(const R *__restrict__ V, const uint32_t *__restrict__ T, const sample_t *__restrict__ grid, CapBox B,
                                                  const unsigned long long *__restrict__ segmin, const unsigned long long *__restrict__ segmax,
                                                  const uint32_t *__restrict__ cnt, uint8_t *__restrict__ ntri, uint32_t *use, CapOut *__restrict__ out, uint32_t f, uint32_t first, uint32_t cells) {
	__shared__ uint32_t sh[4];
	// (the face is the launch's: what depends on it alone is uniform; first, cells: B.face_off[f] and the cells of the face - indexing B by f in here would put B into scratch)
	uint32_t capped = 0u, skipped = 0u, used = 0u;
	for (uint64_t at = (uint64_t)blockIdx.x * 256u + threadIdx.x; at < cells; at += (uint64_t)gridDim.x * 256u) {
		const uint32_t ci = first + (uint32_t)at;
		const CapCell c = cap_cell_of(B, f, (uint32_t)at);
		const CapPlan g = cap_plan(V, T, grid, B, c, cnt[ci], segmin[ci], segmax[ci]);
		const uint32_t nt = g.triangles();
		ntri[ci] = (uint8_t)nt;
		if (g.state == 2u) skipped++;
		if (g.state != 1u) continue;
		used += g.segs;
		if (!nt) continue;
		capped++;
#pragma unroll 1
		for (uint32_t k = 0; k < 4u; k++) {  // (one corner at a time: four point indices side by side cost registers and gain nothing)
			if (!((g.named() >> k) & 1u)) continue;
			uint32_t p[3];
			cap_corner(B, c, k, p);
			atomicOr(&use[cap_point_index(B, p)], 1u << c.f);
		}
	}
	capped = block_sum_u32_256(capped, sh);
	skipped = block_sum_u32_256(skipped, sh);
	used = block_sum_u32_256(used, sh);
	if (threadIdx.x == 0u) {
		if (capped) atomicAdd(&out->capped, (unsigned long long)capped);
		if (skipped) atomicAdd(&out->skipped, (unsigned long long)skipped);
		if (used) atomicAdd(&out->used, (unsigned long long)used);
	}
}

// what the tile scans count: the triangles of a cell, the points a polygon names
struct CapTris { using E = uint8_t; static __device__ __forceinline__ uint32_t count(uint32_t b) { return b; } };
struct CapNamed { using E = uint32_t; static __device__ __forceinline__ uint32_t count(uint32_t b) { return b ? 1u : 0u; } };

__device__ __forceinline__ bool cap_fits(const CapOut *__restrict__ out, uint64_t nV, uint64_t nT, uint64_t capV, uint64_t capT) {
	return nV + out->capv <= capV && nT + out->capt <= capT;
}

// steps 5 and 6, the triangles: the polygons of a cell once more, at the cell's place behind the nT rows of the surface
template <typename R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_cap_emit(const R *__restrict__ V, uint32_t *T, uint64_t nT, uint64_t nV, const sample_t *__restrict__ grid, CapBox B,
                                                  const unsigned long long *__restrict__ segmin, const unsigned long long *__restrict__ segmax,
                                                  const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ ntri, const uint32_t *__restrict__ rank,
                                                  const uint32_t *__restrict__ newid, const CapOut *__restrict__ out, uint64_t capV, uint64_t capT, uint32_t f, uint32_t first,
                                                  uint32_t cells) {
	if (!cap_fits(out, nV, nT, capV, capT)) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	for (uint64_t at = (uint64_t)blockIdx.x * 256u + threadIdx.x; at < cells; at += (uint64_t)gridDim.x * 256u) {
		const uint32_t ci = first + (uint32_t)at;
		if (!ntri[ci]) continue;
		const CapCell c = cap_cell_of(B, f, (uint32_t)at);
		const CapPlan g = cap_plan(V, (const uint32_t *)T, grid, B, c, cnt[ci], segmin[ci], segmax[ci]);  // (rows below nT: nobody writes them here)
		uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;  // the new ids of the corners named
		const uint32_t named = g.named();
#pragma unroll 1
		for (uint32_t k = 0; k < 4u; k++) {
			if (!((named >> k) & 1u)) continue;
			uint32_t p[3];
			cap_corner(B, c, k, p);
			const uint32_t v = (uint32_t)nV + newid[cap_point_index(B, p)];
			if (k == 0u) c0 = v; else if (k == 1u) c1 = v; else if (k == 2u) c2 = v; else c3 = v;
		}
		uint32_t id[6];
#pragma unroll
		for (uint32_t k = 0; k < 6u; k++) {
			const uint32_t e = k == 0u ? g.e0 : k == 1u ? g.e1 : k == 2u ? g.e2 : k == 3u ? g.e3 : k == 4u ? g.e4 : g.e5;
			id[k] = ((g.corners >> k) & 1u) ? (e == 0u ? c0 : e == 1u ? c1 : e == 2u ? c2 : c3) : e;
		}
		uint32_t *o = T + (nT + rank[ci]) * 3u;
		if (g.two) {
			o[0] = id[0]; o[1] = id[1]; o[2] = id[2];
			o[3] = id[3]; o[4] = id[4]; o[5] = id[5];
			continue;
		}
		o[0] = id[0]; o[1] = id[1]; o[2] = id[2];
		if (g.n > 3u) { o[3] = id[0]; o[4] = id[2]; o[5] = id[3]; }
		if (g.n > 4u) { o[6] = id[0]; o[7] = id[3]; o[8] = id[4]; }
		if (g.n > 5u) { o[9] = id[0]; o[10] = id[4]; o[11] = id[5]; }
	}
}

// step 5, the rows: a lane per point of the box's surface; a named one writes its rows at nV + its rank
template <typename R>
__global__ __launch_bounds__(256) void k_cap_verts(R *V, float *N, uint32_t *A0, uint32_t *A1, uint32_t fill0, uint32_t fill1, uint64_t nV, uint64_t nT, CapBox B,
                                                   const uint32_t *__restrict__ use, const uint32_t *__restrict__ newid, const CapOut *__restrict__ out, uint64_t capV,
                                                   uint64_t capT) {
	if (!cap_fits(out, nV, nT, capV, capT)) return;
	for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < B.points; s += (uint64_t)gridDim.x * 256u) {
		const uint32_t faces = use[s];
		if (!faces) continue;
		const uint32_t bx = B.b[0], by = B.b[1], bz = B.b[2];
		const uint64_t top = B.plane + (uint64_t)(bz - 2u) * B.ring;
		uint32_t x, y, z;
		if (s < B.plane) { z = 0u; y = (uint32_t)(s / bx); x = (uint32_t)(s % bx); }
		else if (s >= top) { const uint64_t t = s - top; z = bz - 1u; y = (uint32_t)(t / bx); x = (uint32_t)(t % bx); }
		else {
			const uint64_t t = s - B.plane;
			z = 1u + (uint32_t)(t / B.ring);
			uint32_t q = (uint32_t)(t % B.ring);
			if (q < bx) { y = 0u; x = q; }
			else if (q >= bx + 2u * (by - 2u)) { y = by - 1u; x = q - bx - 2u * (by - 2u); }
			else { q -= bx; y = 1u + (q >> 1); x = (q & 1u) ? bx - 1u : 0u; }
		}
		const uint32_t p[3] = {x + B.lo[0], y + B.lo[1], z + B.lo[2]};
		const uint64_t row = nV + newid[s];
		R *ov = V + row * 3u;
		float *on = N + row * 3u;
		int n[3];
#pragma unroll
		for (int a = 0; a < 3; a++) {
			ov[a] = (R)p[a] * B.D[a] + B.O[a];  // the vertex pass with t = 0 (store_vertex)
			n[a] = (int)((faces >> (2 * a + 1)) & 1u) - (int)((faces >> (2 * a)) & 1u);
		}
		const double m = sqrt((double)((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]));
#pragma unroll
		for (int a = 0; a < 3; a++) on[a] = n[a] ? (float)((double)n[a] / m) : 0.0f;
		if (A0) A0[row] = fill0;
		if (A1) A1[row] = fill1;
	}
}

// invert, in place: the second and third index of every triangle of the surface exchanged, its normals negated
__global__ __launch_bounds__(256) void k_cap_invert(uint32_t *T, uint64_t nT, uint32_t *N, uint64_t nV, const CapOut *__restrict__ out, uint64_t capV, uint64_t capT) {
	if (!cap_fits(out, nV, nT, capV, capT)) return;
	const uint64_t words = nV * 3u, n = nT > words ? nT : words;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		if (i < nT) {
			uint32_t *t = T + i * 3u;
			const uint32_t a = t[1], b = t[2];
			t[1] = b; t[2] = a;
		}
		if (i < words) N[i] ^= 0x80000000u;
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void cap_release(void *state) {
	CapState *s = (CapState *)state;
	dev_release(&s->d_slots); dev_release(&s->d_segmin); dev_release(&s->d_segmax); dev_release(&s->d_cnt); dev_release(&s->d_rank); dev_release(&s->d_ntri);
	dev_release(&s->d_use); dev_release(&s->d_new);
}

static void cap_fill(mc33hip_capping *a, const CapOut &h) {
	a->cap_vertices = h.capv; a->cap_triangles = h.capt; a->nV_out = a->nV + h.capv; a->nT_out = a->nT + h.capt;
	a->rim_segments = h.rim; a->capped_cells = h.capped; a->skipped_cells = h.skipped; a->off_face_edges = h.off;
	a->invalid_triangles = h.bad; a->nonfinite_vertices = h.nonfinite;
	a->closed = h.skipped == 0ull && h.off == 0ull && h.used == h.rim ? 1 : 0;
}

extern "C" int mc33hip_cap_surface(mc33hip_ctx *c, mc33hip_capping *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nV_out = a->nT_out = a->cap_vertices = a->cap_triangles = a->rim_segments = a->capped_cells = a->skipped_cells = a->off_face_edges = a->invalid_triangles =
	    a->nonfinite_vertices = 0;
	a->solid_above = a->closed = 0;
	const mc33hip_grid_desc &d = c->desc;
	if (!c->d_grid) { set_err("no grid is resident in this context"); return MC33HIP_EINVAL; }
	if (d.plane0 != 0u || d.npz_resident != d.nz_total + 1u) { set_err("the context holds a z-slab: the caps need the whole grid"); return MC33HIP_EINVAL; }
	if (c->inclined) { set_err("the caps are defined for orthogonal grids only"); return MC33HIP_EINVAL; }
	if (!(a->iso == a->iso)) { set_err("the isovalue is a NaN"); return MC33HIP_EINVAL; }
	const uint32_t Nc[3] = {d.npx - 1u, d.npy - 1u, d.nz_total};
	for (int k = 0; k < 3; k++)
		if (!(a->lo[k] < a->hi[k] && a->hi[k] <= Nc[k])) {
			set_err("box: lo[%d] = %u, hi[%d] = %u must satisfy lo < hi <= %u", k, a->lo[k], k, a->hi[k], Nc[k]);
			return MC33HIP_EINVAL;
		}
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_counts_ok(a->n_attr, nV, nT)) return MC33HIP_EINVAL;
	for (unsigned k = 0; k < a->n_attr; k++)
		if (a->attr_mode[k] != MC33HIP_CAP_WORD && a->attr_mode[k] != MC33HIP_CAP_F32) {
			set_err("attr_mode[%u] = %d is neither MC33HIP_CAP_WORD nor MC33HIP_CAP_F32", k, a->attr_mode[k]);
			return MC33HIP_EINVAL;
		}
	const uint64_t capV = mesh_cap(a->capV), capT = mesh_cap(a->capT);
	bool null = ((nV || capV) && (!a->V || !a->N)) || ((nT || capT) && !a->T);
	for (unsigned k = 0; k < a->n_attr; k++) null = null || ((nV || capV) && !a->attr[k]);
	if (null) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	CapState *s;
	if ((rc = mesh_op_state(&c->meas->mesh, cap_release, &s))) return rc;
	MeshHost &h = c->meas->mesh;

	CapBox B;
	memset(&B, 0, sizeof B);
	for (int k = 0; k < 3; k++) {
		B.lo[k] = a->lo[k]; B.hi[k] = a->hi[k]; B.b[k] = a->hi[k] - a->lo[k] + 1u;
		B.r0[k] = d.r0[k]; B.rd[k] = 1.0 / d.d[k];
		B.O[k] = (real_t)d.r0[k]; B.D[k] = (real_t)d.d[k];
		// A vertex on grid plane k has the coordinate (R)k * (R)d + (R)r0 rounded three times in MC33_real: within 2^-21 of the largest
		// coordinate of the axis, 2^-21 max(|r0|, |r0 + N d|) / |d| in grid units; a quarter of a cell at most
		const double m = std::max(fabs(d.r0[k]), fabs(d.r0[k] + (double)Nc[k] * d.d[k]));
		B.tol[k] = std::min(ldexp(m, -21) / fabs(d.d[k]), 0.25);
	}
	uint64_t cells = 0;
	for (uint32_t f = 0; f < 6u; f++) {
		if (cells > 0xFFFFFFFFull) break;
		B.face_off[f] = (uint32_t)cells;
		cells += (uint64_t)(B.b[cap_u(f)] - 1u) * (B.b[cap_w(f)] - 1u);
	}
	if (cells > 0xFFFFFFFFull) { set_err("more than 2^32-1 face cells"); return MC33HIP_EINVAL; }
	B.face_off[6] = (uint32_t)cells;
	B.plane = (uint64_t)B.b[0] * B.b[1];
	B.ring = 2ull * B.b[0] + 2ull * (B.b[1] - 2u);
	B.points = 2u * B.plane + (uint64_t)(B.b[2] - 2u) * B.ring;
	B.pitch = c->pitch; B.slice = c->slice;
	B.iso = (real_t)a->iso;
	B.invert = a->invert ? 1u : 0u;
	B.solid_above = (c->normal_neg ? 1u : 0u) == B.invert ? 1u : 0u;
	a->solid_above = (int)B.solid_above;

	const uint64_t tilesC = (cells + MESH_TILE - 1u) / MESH_TILE, tilesP = (B.points + MESH_TILE - 1u) / MESH_TILE;
	const uint64_t nslots = mesh_table_size(nT, 4u, 1ull << 40);
	if ((rc = meas_scratch(c, nV, tilesC + tilesP))) return rc;
	if ((s->slots_cap < nslots || !s->d_slots) && (rc = dev_room("table of sides", &s->d_slots, &s->slots_cap, nslots))) return rc;  // (a power of two as it is: no slack)
	if (s->cells_cap < cells || !s->d_ntri) {
		const uint64_t n = cells + cells / 8u + 256u;
		if ((rc = dev_room_all("face cells", &s->cells_cap, n, {dev_array(&s->d_segmin, n, 8u), dev_array(&s->d_segmax, n, 8u), dev_array(&s->d_cnt, n, 4u),
		                                                       dev_array(&s->d_rank, n, 4u), dev_array(&s->d_ntri, n, 1u)})))
			return rc;
	}
	if (s->points_cap < B.points || !s->d_use) {
		const uint64_t n = B.points + B.points / 8u + 256u;
		if ((rc = dev_room_all("box points", &s->points_cap, n, {dev_array(&s->d_use, n, 4u), dev_array(&s->d_new, n, 4u)}))) return rc;
	}
	uint32_t *bsumC = h.d_bsum, *bsumP = h.d_bsum + tilesC;
	real_t *V = (real_t *)a->V;
	float *N = (float *)a->N;
	uint32_t *T = (uint32_t *)a->T;
	uint32_t *A0 = (uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr), *A1 = (uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr);
	const uint32_t fill0 = a->n_attr > 0u && a->attr_mode[0] == MC33HIP_CAP_F32 ? 0x7FC00000u : 0u, fill1 = a->n_attr > 1u && a->attr_mode[1] == MC33HIP_CAP_F32 ? 0x7FC00000u : 0u;
	const uint32_t gridV = meas_grid(c, nV, 16u), gridT = meas_grid(c, nT, 8u), gridP = meas_grid(c, B.points, 16u);
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(CapOut), c->stream));
	HIP_TRY(hipMemsetAsync(s->d_segmin, 0xFF, cells * 8u, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_segmax, 0, cells * 8u, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_cnt, 0, cells * 4u, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_use, 0, B.points * 4u, c->stream));
	if (nV) hipLaunchKernelGGL((k_cap_flag<real_t>), dim3(gridV), dim3(256), 0, c->stream, (const real_t *)V, (uint64_t)nV, B, h.d_keep, s->d_out);
	if (nT) {
		hipLaunchKernelGGL(k_mesh_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, (ulonglong2 *)s->d_slots, nslots, 0ull);
		hipLaunchKernelGGL(k_cap_sides, dim3(gridT), dim3(256), 0, c->stream, (const uint32_t *)T, (uint64_t)nT, (uint64_t)nV, B.invert, s->d_slots, nslots - 1u, s->d_out);
		hipLaunchKernelGGL((k_cap_rim<real_t>), dim3(gridT), dim3(256), 0, c->stream, (const real_t *)V, (const uint32_t *)T, (uint64_t)nT, (uint64_t)nV, B,
		                   (const uint8_t *)h.d_keep, (const CapSlot *)s->d_slots, nslots - 1u, s->d_segmin, s->d_segmax, s->d_cnt, s->d_out);
	}
	for (uint32_t f = 0; f < 6u; f++)  // (a launch per face: the axes of the face are the launch's, not the lane's)
		hipLaunchKernelGGL((k_cap_cell<real_t>), dim3(meas_grid(c, B.face_off[f + 1u] - B.face_off[f], 16u)), dim3(256), 0, c->stream, (const real_t *)V, (const uint32_t *)T,
		                   (const sample_t *)c->d_grid, B, (const unsigned long long *)s->d_segmin, (const unsigned long long *)s->d_segmax, (const uint32_t *)s->d_cnt,
		                   s->d_ntri, s->d_use, s->d_out, f, B.face_off[f], B.face_off[f + 1u] - B.face_off[f]);
	mesh_scan<CapTris, MESH_RANK>(c, s->d_ntri, cells, bsumC, &s->d_out->capt, s->d_rank);
	mesh_scan<CapNamed, MESH_NEW>(c, s->d_use, B.points, bsumP, &s->d_out->capv, s->d_new);
	// the writing passes: they compare the totals with the capacities on the device, so that the host waits once
	for (uint32_t f = 0; f < 6u; f++)
		hipLaunchKernelGGL((k_cap_emit<real_t>), dim3(meas_grid(c, B.face_off[f + 1u] - B.face_off[f], 16u)), dim3(256), 0, c->stream, (const real_t *)V, T, (uint64_t)nT,
		                   (uint64_t)nV, (const sample_t *)c->d_grid, B, (const unsigned long long *)s->d_segmin, (const unsigned long long *)s->d_segmax,
		                   (const uint32_t *)s->d_cnt, (const uint8_t *)s->d_ntri, (const uint32_t *)s->d_rank, (const uint32_t *)s->d_new, (const CapOut *)s->d_out, capV,
		                   capT, f, B.face_off[f], B.face_off[f + 1u] - B.face_off[f]);
	hipLaunchKernelGGL((k_cap_verts<real_t>), dim3(gridP), dim3(256), 0, c->stream, V, N, A0, A1, fill0, fill1, (uint64_t)nV, (uint64_t)nT, B, (const uint32_t *)s->d_use,
	                   (const uint32_t *)s->d_new, (const CapOut *)s->d_out, capV, capT);
	if (B.invert && (nT || nV))
		hipLaunchKernelGGL(k_cap_invert, dim3(meas_grid(c, std::max<uint64_t>(nT, nV * 3u), 16u)), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint32_t *)N, (uint64_t)nV,
		                   (const CapOut *)s->d_out, capV, capT);
	if ((rc = mesh_op_fetch(c, s))) return rc;
	const CapOut o = *s->h_out;
	cap_fill(a, o);
	if (o.full) { set_err("%llu sides found no slot in the table", o.full); return MC33HIP_ERUNTIME; }
	if (a->nV_out > 0xFFFFFFFFull || a->nT_out > 0xFFFFFFFFull) { set_err("the capped mesh has more than 2^32-1 vertices or triangles"); return MC33HIP_ECAPACITY; }
	if ((rc = mesh_capacity("capped", a->nV_out, a->nT_out, capV, capT))) return rc;
	return mesh_bad(o.bad, nV);
}
