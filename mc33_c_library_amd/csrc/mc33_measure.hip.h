// mc33_measure.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// questions about a FINISHED mesh in device memory, answered there - area, signed volume, first moments, bounding box, the
// integral of a sampled property, connected components - so that a few doubles cross the link instead of the mesh
// (include/mc33_hip.h: mc33hip_measure_surface, mc33hip_label_components, mc33hip_measure_components).  DESIGN.md 10.
//
// The definition (everything in IEEE double, no a*b+c fused: -ffp-contract=off), for triangle i with rows q0, q1, q2 = V[T[i][0..2]]
// and the reference point c[a] = r0[a] + 0.5 * ((double)N[a] * d[a]):
//   p_k = (double)q_k - c;  u = p1 - p0, w = p2 - p0;  n = u x w;  A_i = 0.5 * sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)
//   m = p1 x p2;  W_i = ((p0.x*m.x + p0.y*m.y) + p0.z*m.z) / 6.0        (signed, with the winding as T stores it)
//   M_i[a] = A_i * (((p0[a] + p1[a]) + p2[a]) / 3.0);  Q_i = A_i * ((((double)P[t0] + (double)P[t1]) + (double)P[t2]) / 3.0)
// tests/measure_oracle.py restates it in numpy.  A triangle that names a vertex >= nV is counted, contributes nothing, and is
// tested BEFORE anything is gathered through it: nothing outside V (P, the label array) is ever read.
//
// The global sums are reproducible: per lane in registers, per wave by shuffles, per block through LDS, one row of partials per
// block written with plain stores, k_measure_finish adds the rows in a fixed order - a function of the inputs and the launch
// geometry only, no floating-point atomic anywhere in them.  Only the per-component area / volume columns are added with
// double atomics (one per run of equal components, not per triangle).

struct MeasOut {            // what a call brings to the host (device copy and pinned twin)
	double sum[8];          // area, volume, moment[3], property integral
	double bbox[6];         // min[3], max[3]
	unsigned long long bad; // triangles that name a vertex >= nV (or, with a caller's label array, a label >= nV)
	unsigned long long comps, unref;
	unsigned long long pad_;
};

struct MeasureState {       // scratch of these passes: on the context from the first call on, grown on demand, freed in mc33hip_destroy
	MeasOut *d_out, *h_out;
	double *d_part;         // [rows][8] block partials of k_measure_triangles, behind them [rows][6] of k_measure_bbox
	uint64_t part_cap;      // in doubles
	uint8_t *d_flags;       // [nV] 1: the vertex is a root that owns a triangle
	uint64_t flags_cap;
	uint32_t *d_rank;       // [nV] exclusive sum of the flags: the component's row in the table
	uint64_t rank_cap;
	mc33hip_component *d_table;
	uint64_t table_cap;
	MeshHost mesh;          // the states of the parts behind this one, and the scratch they share with it (mc33_mesh.hip.h)
};

// sum over the block's 256 lanes in a fixed order: offsets 32 .. 1 inside a wave, the four waves in index order.  Lane 0 of the
// block holds the result.
__device__ __forceinline__ double block_sum_256(double x, double *sh /* [4] */) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) x += shfl_down_f64(x, d);
	__syncthreads();
	if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = x;
	__syncthreads();
	return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct TriTerms { double A, W, M[3]; };

// the terms of one triangle, rows already tested to lie inside V
template <typename R>
__device__ __forceinline__ TriTerms tri_terms(const R *__restrict__ V, uint32_t t0, uint32_t t1, uint32_t t2, double c0, double c1, double c2) {
	const R *r0 = V + (uint64_t)t0 * 3u, *r1 = V + (uint64_t)t1 * 3u, *r2 = V + (uint64_t)t2 * 3u;
	const double p0x = (double)r0[0] - c0, p0y = (double)r0[1] - c1, p0z = (double)r0[2] - c2;
	const double p1x = (double)r1[0] - c0, p1y = (double)r1[1] - c1, p1z = (double)r1[2] - c2;
	const double p2x = (double)r2[0] - c0, p2y = (double)r2[1] - c1, p2z = (double)r2[2] - c2;
	const double ux = p1x - p0x, uy = p1y - p0y, uz = p1z - p0z;
	const double wx = p2x - p0x, wy = p2y - p0y, wz = p2z - p0z;
	const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
	TriTerms t;
	t.A = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
	const double mx = p1y * p2z - p1z * p2y, my = p1z * p2x - p1x * p2z, mz = p1x * p2y - p1y * p2x;
	t.W = ((p0x * mx + p0y * my) + p0z * mz) / 6.0;
	t.M[0] = t.A * (((p0x + p1x) + p2x) / 3.0);
	t.M[1] = t.A * (((p0y + p1y) + p2y) / 3.0);
	t.M[2] = t.A * (((p0z + p1z) + p2z) / 3.0);
	return t;
}

// Every block a contiguous piece of T (chunk triangles, a multiple of 256), a lane a triangle per step: the wave reads 768
// contiguous bytes of T and gathers 192 rows of V, which - triangles being stored in sweep order - lie close together.
template <typename R, bool HASP>
__global__ __launch_bounds__(256) void k_measure_triangles(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t nT,
                                                           const float *__restrict__ P, double c0, double c1, double c2, uint64_t chunk,
                                                           double *__restrict__ part, unsigned long long *__restrict__ bad_out) {
	__shared__ double sh[4];
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nT ? beg + chunk : nT;
	double sA = 0.0, sW = 0.0, sM0 = 0.0, sM1 = 0.0, sM2 = 0.0, sQ = 0.0;
	uint32_t bad = 0u;
	for (uint64_t i = beg + threadIdx.x; i < end; i += 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		const TriTerms x = tri_terms<R>(V, t0, t1, t2, c0, c1, c2);
		sA += x.A; sW += x.W; sM0 += x.M[0]; sM1 += x.M[1]; sM2 += x.M[2];
		if (HASP) sQ += x.A * ((((double)P[t0] + (double)P[t1]) + (double)P[t2]) / 3.0);
	}
	double *row = part + (uint64_t)blockIdx.x * 8u;
	double r;
	r = block_sum_256(sA, sh);  if (threadIdx.x == 0u) row[0] = r;
	r = block_sum_256(sW, sh);  if (threadIdx.x == 0u) row[1] = r;
	r = block_sum_256(sM0, sh); if (threadIdx.x == 0u) row[2] = r;
	r = block_sum_256(sM1, sh); if (threadIdx.x == 0u) row[3] = r;
	r = block_sum_256(sM2, sh); if (threadIdx.x == 0u) row[4] = r;
	if (HASP) r = block_sum_256(sQ, sh);
	if (threadIdx.x == 0u) { row[5] = HASP ? r : 0.0; row[6] = 0.0; row[7] = 0.0; }
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// minimum / maximum of the rows of V per axis, exact in any order; a NaN coordinate fails both comparisons and is skipped
template <typename R>
__global__ __launch_bounds__(256) void k_measure_bbox(const R *__restrict__ V, uint64_t nV, double *__restrict__ bpart) {
	__shared__ double sh[4][6];
	const double inf = __builtin_huge_val();
	double m[6] = {inf, inf, inf, -inf, -inf, -inf};
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const R *row = V + v * 3u;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const double x = (double)row[a];
			if (x < m[a]) m[a] = x;
			if (x > m[3 + a]) m[3 + a] = x;
		}
	}
#pragma unroll
	for (int k = 0; k < 6; k++) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const double o = shfl_down_f64(m[k], d);
			if (k < 3 ? o < m[k] : o > m[k]) m[k] = o;
		}
		if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6][k] = m[k];
	}
	__syncthreads();
	if (threadIdx.x < 6u) {
		const uint32_t k = threadIdx.x;
		double x = sh[0][k];
		for (int w = 1; w < 4; w++) {
			const double o = sh[w][k];
			if (k < 3u ? o < x : o > x) x = o;
		}
		bpart[(uint64_t)blockIdx.x * 6u + k] = x;
	}
}

// One block: the partial rows in index order - lane t adds rows t, t + 256, ..., then a tree over the lanes - and the bounding box.
__global__ __launch_bounds__(256) void k_measure_finish(const double *__restrict__ part, uint32_t nrows, const double *__restrict__ bpart, uint32_t nbrows,
                                                        MeasOut *__restrict__ out) {
	__shared__ double sh[6][256];
	const uint32_t t = threadIdx.x;
	double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (uint32_t r = t; r < nrows; r += 256u) {
#pragma unroll
		for (int k = 0; k < 6; k++) s[k] += part[(uint64_t)r * 8u + k];
	}
#pragma unroll
	for (int k = 0; k < 6; k++) sh[k][t] = s[k];
	__syncthreads();
	for (uint32_t d = 128u; d >= 1u; d >>= 1) {
		if (t < d) {
#pragma unroll
			for (int k = 0; k < 6; k++) sh[k][t] += sh[k][t + d];
		}
		__syncthreads();
	}
	if (t < 6u) out->sum[t] = sh[t][0];
	if (t >= 6u && t < 8u) out->sum[t] = 0.0;
	__syncthreads();
	const double inf = __builtin_huge_val();
	double m[6] = {inf, inf, inf, -inf, -inf, -inf};
	for (uint32_t r = t; r < nbrows; r += 256u) {
#pragma unroll
		for (int k = 0; k < 6; k++) {
			const double o = bpart[(uint64_t)r * 6u + k];
			if (k < 3 ? o < m[k] : o > m[k]) m[k] = o;
		}
	}
#pragma unroll
	for (int k = 0; k < 6; k++) sh[k][t] = m[k];
	__syncthreads();
	for (uint32_t d = 128u; d >= 1u; d >>= 1) {
		if (t < d) {
#pragma unroll
			for (int k = 0; k < 6; k++) {
				const double o = sh[k][t + d];
				if (k < 3 ? o < sh[k][t] : o > sh[k][t]) sh[k][t] = o;
			}
		}
		__syncthreads();
	}
	if (t < 6u) out->bbox[t] = sh[t][0];
}

// --- connected components: a union-find over vertex ids, one word per vertex, in the caller's label array ------------------
// The larger root is always hooked under the smaller, so parent[x] <= x throughout, the final root of a set is its smallest
// vertex and the result does not depend on scheduling.  The eight XCDs' L2s are not coherent for plain accesses: every word of
// `parent` is read and written with relaxed agent-scope atomics while unions are under way, and what decides how a walk goes on
// after a lost race is the value the failed compare-and-swap returned.  (Walking with plain loads instead - every value read a
// possibly stale ancestor - took mc33hip_label_components from 4.1 to 2.8 ms on the bench surface and from 4.2 to 3.9 ms on
// 15 625 blobs: not where most of the time goes, and not worth reads that race with the atomics.  profiles/r08_measure.txt)
#define MC33_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__global__ __launch_bounds__(256) void k_cc_init(uint32_t *__restrict__ parent, uint64_t nV) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) parent[v] = (uint32_t)v;
}

// root of x, with path halving: a non-root never becomes a root again, and any ancestor is a valid parent
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x) {
	uint32_t p = __hip_atomic_load(parent + x, MC33_RLX_AGENT);
	while (p != x) {
		const uint32_t g = __hip_atomic_load(parent + p, MC33_RLX_AGENT);
		if (g != p) __hip_atomic_store(parent + x, g, MC33_RLX_AGENT);
		x = p;
		p = g;
	}
	return x;
}

__device__ __forceinline__ void cc_unite(uint32_t *parent, uint32_t u, uint32_t v) {
	for (;;) {
		u = cc_find(parent, u);
		v = cc_find(parent, v);
		if (u == v) return;
		if (u < v) { const uint32_t s = u; u = v; v = s; }
		const uint32_t old = atomicCAS(parent + u, u, v);  // (relaxed, agent scope)
		if (old == u) return;
		u = old;  // hooked by somebody else meanwhile: go on from where it hangs now
	}
}

__global__ __launch_bounds__(256) void k_cc_union(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, uint32_t *parent, unsigned long long *__restrict__ bad_out) {
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		if (t1 != t0) cc_unite(parent, t0, t1);
		if (t2 != t0 && t2 != t1) cc_unite(parent, t0, t2);
	}
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// every word its root (no union runs beside this: the walks only read, the stores only shorten)
__global__ __launch_bounds__(256) void k_cc_flatten(uint32_t *parent, uint64_t nV) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		uint32_t x = (uint32_t)v, p = __hip_atomic_load(parent + x, MC33_RLX_AGENT);
		while (p != x) { x = p; p = __hip_atomic_load(parent + x, MC33_RLX_AGENT); }
		__hip_atomic_store(parent + v, x, MC33_RLX_AGENT);
	}
}

// flags[r] = 1 for every root that owns a triangle (a triangle belongs to label[T[i][0]]); one store per run of equal roots in a wave
__global__ __launch_bounds__(256) void k_cc_flag(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ label,
                                                 uint8_t *__restrict__ flags, unsigned long long *__restrict__ bad_out) {
	uint32_t bad = 0u;
	const uint64_t rounds = (nT + (uint64_t)gridDim.x * 256u - 1u) / ((uint64_t)gridDim.x * 256u);
	for (uint64_t k = 0; k < rounds; k++) {  // (every lane of a wave takes every step: the shuffle below)
		const uint64_t i = (k * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
		uint32_t r = 0xFFFFFFFFu;
		if (i < nT) {
			const uint32_t *t = T + i * 3u;
			const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
			if (t0 >= nV || t1 >= nV || t2 >= nV) bad++;
			else {
				r = label[t0];
				if (r >= nV) { bad++; r = 0xFFFFFFFFu; }
			}
		}
		const uint32_t before = __shfl_up(r, 1, 64);
		if (r != 0xFFFFFFFFu && ((threadIdx.x & 63u) == 0u || before != r)) flags[r] = 1;
	}
	if (bad && bad_out) atomicAdd(bad_out, (unsigned long long)bad);
}

// components (flagged roots) and unreferenced vertices (roots of themselves that own nothing), and the flags per tile for the scan
__global__ __launch_bounds__(256) void k_cc_count(const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags, uint64_t nV,
                                                  uint32_t *__restrict__ bsum, MeasOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const uint64_t v0 = mesh_tile_e0();
	uint32_t own = 0u, lone = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint64_t v = v0 + k;
		if (v < nV) {
			const uint32_t f = flags[v];
			own += f;
			lone += (!f && label[v] == (uint32_t)v) ? 1u : 0u;
		}
	}
	const uint32_t tot_own = block_sum_u32_256(own, sh), tot_lone = block_sum_u32_256(lone, sh);
	if (threadIdx.x == 0u) {
		bsum[blockIdx.x] = tot_own;
		if (tot_own) atomicAdd(&out->comps, (unsigned long long)tot_own);
		if (tot_lone) atomicAdd(&out->unref, (unsigned long long)tot_lone);
	}
}

__device__ __forceinline__ void table_flush(mc33hip_component *table, uint32_t key, uint32_t n, double a, double w) {
	atomicAdd(&table[key].nT, n);
	unsafeAtomicAdd(&table[key].area, a);
	unsafeAtomicAdd(&table[key].volume, w);
}

struct HeldRow { uint32_t key, n; double a, w; };

// What the lanes of a block hold when their piece is through: runs of equal keys in a wave summed once more, then the four
// waves' first runs joined where they are the same component - a block inside ONE component issues one set of atomics.  (One
// address takes some 90 atomics per microsecond: with a set per wave the 7.8 M triangles of a one-component surface waited
// 0.56 ms for 49 000 of them, the 3.9 M vertices 0.69 ms for 61 000.)  TRI: rows of k_cc_table_triangles, else vertex counts.
template <bool TRI>
__device__ __forceinline__ void table_flush_block(mc33hip_component *table, uint32_t held, uint32_t n, double a, double w, HeldRow *sh /* [4] */) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t before = __shfl_up(held, 1, 64);
	const bool head = lane == 0u || before != held;
	const unsigned long long heads = __ballot(head);
	n = run_sum_u32(n, heads, lane);
	if (TRI) { a = run_sum_f64(a, heads, lane); w = run_sum_f64(w, heads, lane); }
	if (lane == 0u) { sh[wave].key = held; sh[wave].n = n; sh[wave].a = a; sh[wave].w = w; }
	else if (head && held != 0xFFFFFFFFu) {
		if (TRI) table_flush(table, held, n, a, w);
		else atomicAdd(&table[held].nV, n);
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		HeldRow r = sh[0];
		for (int q = 1; q <= 4; q++) {
			if (q < 4 && sh[q].key == r.key) { r.n += sh[q].n; r.a += sh[q].a; r.w += sh[q].w; continue; }
			if (r.key != 0xFFFFFFFFu) {
				if (TRI) table_flush(table, r.key, r.n, r.a, r.w);
				else atomicAdd(&table[r.key].nV, r.n);
			}
			if (q < 4) r = sh[q];
		}
	}
}

// {1, A_i, W_i} of every triangle into the row of its component.  Every block a contiguous piece of T, a wave 64 consecutive
// triangles per step; the runs of equal components among them are summed in the wave, and the lane that begins a run keeps
// adding to what it holds while its component stays the same.
template <typename R>
__global__ __launch_bounds__(256) void k_cc_table_triangles(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t nT,
                                                            const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ rank, double c0, double c1, double c2, uint64_t chunk,
                                                            mc33hip_component *table, unsigned long long *__restrict__ bad_out) {
	__shared__ HeldRow sh[4];
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nT ? beg + chunk : nT;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t held = 0xFFFFFFFFu, held_n = 0u, bad = 0u;
	double held_a = 0.0, held_w = 0.0;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {  // (wave-uniform)
		const uint64_t i = base + lane;
		uint32_t key = 0xFFFFFFFFu;
		double a = 0.0, w = 0.0;
		if (i < end) {
			const uint32_t *t = T + i * 3u;
			const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
			if (t0 >= nV || t1 >= nV || t2 >= nV) bad++;
			else {
				const uint32_t r = label[t0];
				if (r >= nV || !flags[r]) bad++;
				else {
					key = rank[r];
					const TriTerms x = tri_terms<R>(V, t0, t1, t2, c0, c1, c2);
					a = x.A; w = x.W;
				}
			}
		}
		const uint32_t before = __shfl_up(key, 1, 64);
		const bool head = lane == 0u || before != key;
		const unsigned long long heads = __ballot(head);
		const uint32_t n = run_sum_u32(key != 0xFFFFFFFFu ? 1u : 0u, heads, lane);
		a = run_sum_f64(a, heads, lane);
		w = run_sum_f64(w, heads, lane);
		if (head && key != 0xFFFFFFFFu) {
			if (key != held) {
				if (held != 0xFFFFFFFFu) table_flush(table, held, held_n, held_a, held_w);
				held = key; held_n = 0u; held_a = 0.0; held_w = 0.0;
			}
			held_n += n; held_a += a; held_w += w;
		}
	}
	table_flush_block<true>(table, held, held_n, held_a, held_w, sh);
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// 1 per referenced vertex into its component's row, and the root's own index; pieces, runs and held counts as above
__global__ __launch_bounds__(256) void k_cc_table_vertices(const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank,
                                                           uint64_t nV, uint64_t chunk, mc33hip_component *table) {
	__shared__ HeldRow sh[4];
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nV ? beg + chunk : nV;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t held = 0xFFFFFFFFu, held_n = 0u;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {
		const uint64_t v = base + lane;
		uint32_t key = 0xFFFFFFFFu;
		if (v < end) {
			const uint32_t r = label[v];
			if (r < nV && flags[r]) {  // (a vertex no triangle names is its own root and owns nothing)
				key = rank[r];
				if (r == (uint32_t)v) table[key].root = r;
			}
		}
		const uint32_t before = __shfl_up(key, 1, 64);
		const bool head = lane == 0u || before != key;
		const unsigned long long heads = __ballot(head);
		const uint32_t n = run_sum_u32(key != 0xFFFFFFFFu ? 1u : 0u, heads, lane);
		if (head && key != 0xFFFFFFFFu) {
			if (key != held) {
				if (held != 0xFFFFFFFFu) atomicAdd(&table[held].nV, held_n);
				held = key; held_n = 0u;
			}
			held_n += n;
		}
	}
	table_flush_block<false>(table, held, held_n, 0.0, 0.0, sh);
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void meas_destroy(mc33hip_ctx *c) {
	MeasureState *m = c->meas;
	if (!m) return;
	mesh_host_destroy(&m->mesh);
	dev_release(&m->d_out); dev_release(&m->d_part); dev_release(&m->d_flags); dev_release(&m->d_rank); dev_release(&m->d_table);
	if (m->h_out) (void)hipHostFree(m->h_out);
	free(m);
	c->meas = nullptr;
}

static int meas_state(mc33hip_ctx *c) {
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	if (c->meas) return 0;
	MeasureState *m = (MeasureState *)calloc(1, sizeof *m);
	if (!m) return MC33HIP_ENOMEM;
	c->meas = m;  // (what it holds so far goes with the context)
	HIP_TRY(hipMalloc(&m->d_out, sizeof(MeasOut)));
	HIP_TRY(hipHostMalloc(&m->h_out, sizeof(MeasOut), hipHostMallocDefault));
	return 0;
}

// room for `need` elements, with an eighth and 256 to spare when the array has to be made anew; nothing of an earlier call is in
// flight (every entry point waits before it returns)
template <typename E>
static int meas_room(E **p, uint64_t *cap, uint64_t need) {
	return *cap >= need && *p ? 0 : dev_room("measuring scratch", p, cap, need + need / 8u + 256u);
}

static uint32_t meas_grid(const mc33hip_ctx *c, uint64_t n, uint32_t per_cu) {  // lanes of 256 up to per_cu blocks per CU
	return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>((n + 255u) / 256u, (uint64_t)std::max(1, c->cus) * per_cu));
}

static void meas_origin(const mc33hip_ctx *c, double o[3]) {
	const double N[3] = {(double)(c->desc.npx - 1u), (double)(c->desc.npy - 1u), (double)c->desc.nz_total};
	for (int a = 0; a < 3; a++) o[a] = c->desc.r0[a] + 0.5 * (N[a] * c->desc.d[a]);
}

static int meas_zero_counters(mc33hip_ctx *c) {
	HIP_TRY(hipMemsetAsync(&c->meas->d_out->bad, 0, 4 * sizeof(unsigned long long), c->stream));
	return 0;
}

static int meas_fetch(mc33hip_ctx *c) { return mesh_op_fetch(c, c->meas); }

// room in the scratch the mesh parts share: flags and new indices of nV vertices, `tiles` tile sums
static int meas_scratch(mc33hip_ctx *c, uint64_t nV, uint64_t tiles) {
	MeshHost &h = c->meas->mesh;
	int rc;
	if ((rc = meas_room(&h.d_keep, &h.keep_cap, nV))) return rc;
	if ((rc = meas_room(&h.d_map, &h.map_cap, nV))) return rc;
	return meas_room(&h.d_bsum, &h.bsum_cap, tiles);
}

extern "C" int mc33hip_measure_surface(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT, const float *dP,
                                       mc33hip_measures *out) {
	if (!c || !out || (nV && !dV) || (nT && !dT) || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	MeasureState *m = c->meas;
	// 16 blocks per CU: pieces short enough that the CUs stay full until the end, few enough rows for the one finishing block
	const uint32_t gridT = nT ? meas_grid(c, nT, 16u) : 0u, gridV = nV ? meas_grid(c, nV, 16u) : 0u;
	const uint64_t chunk = nT ? ((nT + gridT - 1u) / gridT + 255u) / 256u * 256u : 0u;
	if ((rc = meas_room(&m->d_part, &m->part_cap, (uint64_t)gridT * 8u + (uint64_t)gridV * 6u))) return rc;
	double *bpart = m->d_part + (uint64_t)gridT * 8u;
	double o[3];
	meas_origin(c, o);
	if ((rc = meas_zero_counters(c))) return rc;
	if (nT) {
		if (dP) hipLaunchKernelGGL((k_measure_triangles<real_t, true>), dim3(gridT), dim3(256), 0, c->stream, (const real_t *)dV, (uint64_t)nV, (const uint32_t *)dT,
		                           (uint64_t)nT, dP, o[0], o[1], o[2], chunk, m->d_part, &m->d_out->bad);
		else hipLaunchKernelGGL((k_measure_triangles<real_t, false>), dim3(gridT), dim3(256), 0, c->stream, (const real_t *)dV, (uint64_t)nV, (const uint32_t *)dT,
		                        (uint64_t)nT, (const float *)nullptr, o[0], o[1], o[2], chunk, m->d_part, &m->d_out->bad);
	}
	if (nV) hipLaunchKernelGGL((k_measure_bbox<real_t>), dim3(gridV), dim3(256), 0, c->stream, (const real_t *)dV, (uint64_t)nV, bpart);
	hipLaunchKernelGGL(k_measure_finish, dim3(1), dim3(256), 0, c->stream, m->d_part, gridT, bpart, gridV, m->d_out);
	if ((rc = meas_fetch(c))) return rc;
	const MeasOut &h = *m->h_out;
	memset(out, 0, sizeof *out);
	out->nV = nV; out->nT = nT;
	out->area = h.sum[0]; out->volume = h.sum[1];
	for (int a = 0; a < 3; a++) { out->moment[a] = h.sum[2 + a]; out->origin[a] = o[a]; out->bbox_min[a] = h.bbox[a]; out->bbox_max[a] = h.bbox[3 + a]; }
	out->has_property = dP ? 1 : 0;
	out->property_integral = dP ? h.sum[5] : 0.0;
	return mesh_bad(h.bad, nV);
}

// flags of the roots that own a triangle, their number and the unreferenced vertices (enqueues; the counters were zeroed).
// check: the label array is a caller's - count what k_cc_flag cannot use (after k_cc_union it has counted them already)
static int cc_flag_and_count(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, const unsigned *dLabel, bool check) {
	MeasureState *m = c->meas;
	int rc;
	const uint64_t tiles = (nV + MESH_TILE - 1u) / MESH_TILE;
	if ((rc = meas_room(&m->d_flags, &m->flags_cap, nV))) return rc;
	if ((rc = meas_room(&m->mesh.d_bsum, &m->mesh.bsum_cap, tiles))) return rc;
	if (!nV) return 0;
	HIP_TRY(hipMemsetAsync(m->d_flags, 0, nV, c->stream));
	if (nT) hipLaunchKernelGGL(k_cc_flag, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, (const uint32_t *)dT, (uint64_t)nT, (uint64_t)nV, dLabel, m->d_flags,
	                           check ? &m->d_out->bad : (unsigned long long *)nullptr);
	hipLaunchKernelGGL(k_cc_count, dim3((uint32_t)tiles), dim3(256), 0, c->stream, dLabel, m->d_flags, (uint64_t)nV, m->mesh.d_bsum, m->d_out);
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" int mc33hip_label_components(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, unsigned *dLabel,
                                        unsigned long long *components, unsigned long long *unreferenced) {
	if (!c || (nV && !dLabel) || (nT && !dT) || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	MeasureState *m = c->meas;
	if ((rc = meas_zero_counters(c))) return rc;
	if (nV) hipLaunchKernelGGL(k_cc_init, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, dLabel, (uint64_t)nV);
	if (nT) hipLaunchKernelGGL(k_cc_union, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, (const uint32_t *)dT, (uint64_t)nT, (uint64_t)nV, dLabel, &m->d_out->bad);
	if (nV) hipLaunchKernelGGL(k_cc_flatten, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, dLabel, (uint64_t)nV);
	HIP_TRY(hipGetLastError());
	if ((rc = cc_flag_and_count(c, dT, nT, nV, dLabel, false))) return rc;
	if ((rc = meas_fetch(c))) return rc;
	if (components) *components = m->h_out->comps;
	if (unreferenced) *unreferenced = m->h_out->unref;
	return mesh_bad(m->h_out->bad, nV);
}

extern "C" int mc33hip_measure_components(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT, const unsigned *dLabel,
                                          mc33hip_component *host_table, unsigned long long capacity, unsigned long long *components) {
	if (!c || !components || (nV && (!dV || !dLabel)) || (nT && !dT) || (capacity && !host_table) || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	MeasureState *m = c->meas;
	*components = 0;
	if ((rc = meas_zero_counters(c))) return rc;
	if ((rc = cc_flag_and_count(c, dT, nT, nV, dLabel, true))) return rc;
	if ((rc = meas_fetch(c))) return rc;
	if ((rc = mesh_bad(m->h_out->bad, nV))) return rc;
	const unsigned long long ncomp = m->h_out->comps;
	*components = ncomp;
	if (capacity < ncomp) { set_err("the component table needs %llu rows, the caller's has %llu", ncomp, capacity); return MC33HIP_ECAPACITY; }
	if (!ncomp) return MC33HIP_OK;
	if ((rc = meas_room(&m->d_rank, &m->rank_cap, nV))) return rc;
	if ((rc = meas_room(&m->d_table, &m->table_cap, ncomp))) return rc;
	HIP_TRY(hipMemsetAsync(m->d_table, 0, ncomp * sizeof(mc33hip_component), c->stream));
	if ((rc = meas_zero_counters(c))) return rc;
	double o[3];
	meas_origin(c, o);
	// (8 blocks per CU: every block ends with a set of atomics, and on a one-component surface they all meet in one row)
	const uint32_t gridT = meas_grid(c, nT, 8u), gridV = meas_grid(c, nV, 8u);
	const uint64_t chunk = ((nT + gridT - 1u) / gridT + 255u) / 256u * 256u, chunkV = ((nV + gridV - 1u) / gridV + 255u) / 256u * 256u;
	mesh_scan_sums<MeshFlag, MESH_RANK>(c, m->d_flags, nV, m->mesh.d_bsum, nullptr, m->d_rank);
	hipLaunchKernelGGL((k_cc_table_triangles<real_t>), dim3(gridT), dim3(256), 0, c->stream, (const real_t *)dV, (uint64_t)nV, (const uint32_t *)dT, (uint64_t)nT, dLabel,
	                   m->d_flags, m->d_rank, o[0], o[1], o[2], chunk, m->d_table, &m->d_out->bad);
	hipLaunchKernelGGL(k_cc_table_vertices, dim3(gridV), dim3(256), 0, c->stream, dLabel, m->d_flags, m->d_rank, (uint64_t)nV, chunkV, m->d_table);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(host_table, m->d_table, ncomp * sizeof(mc33hip_component), hipMemcpyDeviceToHost, c->stream));
	if ((rc = meas_fetch(c))) return rc;
	return mesh_bad(m->h_out->bad, nV);
}
