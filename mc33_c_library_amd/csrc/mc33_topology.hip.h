// mc33_topology.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h and mc33_measure.hip.h; not a header to include elsewhere):
// the topology of a FINISHED triangle list in device memory - distinct edges, boundary / non-manifold / misoriented edges,
// degenerate triangles, boundary loops, Euler number and genus, for the surface and per connected component - so that a few
// integers cross the link instead of the mesh (include/mc33_hip.h: mc33hip_surface_topology, mc33hip_component_topology).
// DESIGN.md 11.  Only T is read; labels, flags, ranks and the union-find (k_cc_*, cc_unite) are those of mc33_measure.hip.h.
//
// The definition: a triangle that names a vertex >= nV is counted and contributes nothing; a valid one with two equal indices
// is degenerate: its sides a -> a are skipped, its other sides enter like any side.  Every other side a -> b, in the order
// T0 -> T1, T1 -> T2, T2 -> T0, is a use of the edge {lo, hi} = {min, max}, forward when a < b.  tests/topology_oracle.py restates
// it in numpy.  Everything is an integer and added with integer atomics: the results do not depend on scheduling.
//
// The edge table: the table of mc33_mesh.hip.h, 16 bytes per slot - the key lo << 32 | hi (all ones: empty; lo < hi, so no
// key has it) and one word of two exact 32-bit use counters, forward in the low half, backward in the high half (either is at
// most nT <= 2^32 - 1: the low half never carries).  A power of two >= 4 nT slots for at most 3 nT edges.  Insert-only.

struct TopoSlot { unsigned long long key, uses; };
using TopoRow = struct mc33hip_component_topology;  // (the plain name is the function's)

constexpr uint32_t TOPO_NONE = 0xFFFFFFFFu;
// counters of the component rows the kernels add into (unsigned long long [components][TOPO_COLS])
enum { TC_NV = 0, TC_NT, TC_EDGES, TC_BOUNDARY, TC_NONMANIFOLD, TC_MISORIENTED, TC_DEGENERATE, TC_LOOPS, TC_ROOT, TOPO_COLS };

struct TopoOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long invalid, degenerate, edges, boundary, nonmanifold, misoriented, loops;
	unsigned long long full;                // sides that found no slot (cannot happen with >= 4 nT slots; checked all the same)
	unsigned long long closed_components, genus_sum, genus_undefined;
	unsigned long long pad_;
};

struct TopoState {          // scratch of these passes: on the MeasureState from the first call on, grown on demand, freed with it
	TopoOut *d_out, *h_out;
	TopoSlot *d_slots;
	uint64_t slots_cap;
	uint32_t *d_loop;       // [nV] the second union-find: vertices joined by boundary edges
	uint64_t loop_cap;
	uint8_t *d_bflag;       // [nV] 1: the vertex ends a boundary edge
	uint64_t bflag_cap;
	uint32_t *d_label;      // [nV] labels mc33hip_surface_topology makes for itself
	uint64_t label_cap;
	unsigned long long *d_rows;  // [components][TOPO_COLS]
	uint64_t rows_cap;
	TopoRow *d_table;
	uint64_t table_cap;
};

// One use of the edge {a, b}, a != b: the slot claimed, the use added to its counter.  Returns false when every slot was tried.
__device__ __forceinline__ bool topo_use(TopoSlot *slots, uint64_t mask, uint32_t a, uint32_t b) {
	const bool fwd = a < b;
	const uint64_t s = mesh_claim(slots, mask, fwd ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a);
	if (s == MESH_NOSLOT) return false;
	atomicAdd(&slots[s].uses, fwd ? 1ull : 1ull << 32);
	return true;
}

// one pass over T: validate, count, and enter the sides (a lane a triangle: neighbouring lanes name neighbouring vertices)
__global__ __launch_bounds__(256) void k_topo_insert(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, TopoSlot *slots, uint64_t mask,
                                                     TopoOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t bad = 0u, deg = 0u, full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		if (t0 == t1 || t1 == t2 || t2 == t0) deg++;
		if (t0 != t1 && !topo_use(slots, mask, t0, t1)) full++;
		if (t1 != t2 && !topo_use(slots, mask, t1, t2)) full++;
		if (t2 != t0 && !topo_use(slots, mask, t2, t0)) full++;
	}
	bad = block_sum_u32_256(bad, sh);
	deg = block_sum_u32_256(deg, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (bad) atomicAdd(&out->invalid, (unsigned long long)bad);
		if (deg) atomicAdd(&out->degenerate, (unsigned long long)deg);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// K counters per component row, added once per run of equal components: the runs among the 64 lanes of a step are summed in
// the wave (as k_cc_table_* do), and the lane that begins a run keeps adding to what it holds while its component stays the
// same.  Every lane of the wave takes every step.
template <int K>
struct TopoHeld {
	uint32_t key, n[K];
	__device__ __forceinline__ void flush(unsigned long long *rows, const int (&col)[K]) const {
		if (key == TOPO_NONE) return;
#pragma unroll
		for (int k = 0; k < K; k++)
			if (n[k]) atomicAdd(rows + (uint64_t)key * TOPO_COLS + col[k], (unsigned long long)n[k]);
	}
	__device__ __forceinline__ void step(unsigned long long *rows, const int (&col)[K], uint32_t k_, uint32_t (&x)[K]) {
		const uint32_t lane = threadIdx.x & 63u;
		const uint32_t before = __shfl_up(k_, 1, 64);
		const bool head = lane == 0u || before != k_;
		const unsigned long long heads = __ballot(head);
#pragma unroll
		for (int k = 0; k < K; k++) x[k] = run_sum_u32(x[k], heads, lane);
		if (head && k_ != TOPO_NONE) {
			if (k_ != key) {
				flush(rows, col);
				key = k_;
#pragma unroll
				for (int k = 0; k < K; k++) n[k] = 0u;
			}
#pragma unroll
			for (int k = 0; k < K; k++) n[k] += x[k];
		}
	}
};

// the row of the component a vertex (< nV) belongs to; TOPO_NONE where the label array does not name a root that owns a triangle
__device__ __forceinline__ uint32_t topo_row(uint32_t v, uint64_t nV, const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags,
                                             const uint32_t *__restrict__ rank) {
	const uint32_t r = label[v];
	return r < nV && flags[r] ? rank[r] : TOPO_NONE;
}

// One pass over the slots, every block a contiguous piece: the four edge counters for the surface and per component (an edge
// belongs to label[lo]), and every boundary edge united in `loop`.
__global__ __launch_bounds__(256) void k_topo_classify(const TopoSlot *__restrict__ slots, uint64_t nslots, uint64_t chunk, uint64_t nV,
                                                       const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank,
                                                       uint32_t *loop, uint8_t *__restrict__ bflag, unsigned long long *rows, TopoOut *__restrict__ out,
                                                       unsigned long long *__restrict__ bad_out) {
	__shared__ uint32_t sh[4];
	const int col[4] = {TC_EDGES, TC_BOUNDARY, TC_NONMANIFOLD, TC_MISORIENTED};
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nslots ? beg + chunk : nslots;
	const uint32_t lane = threadIdx.x & 63u;
	TopoHeld<4> held;
	held.key = TOPO_NONE;
	uint32_t tot[4] = {0u, 0u, 0u, 0u}, bad = 0u;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {  // (wave-uniform)
		const uint64_t s = base + lane;
		uint32_t key = TOPO_NONE, x[4] = {0u, 0u, 0u, 0u};
		if (s < end) {
			const ulonglong2 e = *(const ulonglong2 *)(slots + s);
			if (e.x != MESH_EMPTY) {
				const uint32_t lo = (uint32_t)(e.x >> 32), hi = (uint32_t)e.x;
				const uint32_t f = (uint32_t)e.y, b = (uint32_t)(e.y >> 32);
				const uint64_t uses = (uint64_t)f + b;
				x[0] = 1u;
				x[1] = uses == 1u ? 1u : 0u;
				x[2] = uses > 2u ? 1u : 0u;
				x[3] = uses == 2u && f != 1u ? 1u : 0u;
#pragma unroll
				for (int k = 0; k < 4; k++) tot[k] += x[k];
				if (x[1]) {
					cc_unite(loop, lo, hi);
					bflag[lo] = 1; bflag[hi] = 1;
				}
				key = topo_row(lo, nV, label, flags, rank);
				if (key == TOPO_NONE) bad++;
			}
		}
		held.step(rows, col, key, x);
	}
	held.flush(rows, col);
	unsigned long long *const dst[4] = {&out->edges, &out->boundary, &out->nonmanifold, &out->misoriented};
#pragma unroll
	for (int k = 0; k < 4; k++) {
		const uint32_t t = block_sum_u32_256(tot[k], sh);
		if (threadIdx.x == 0u && t) atomicAdd(dst[k], (unsigned long long)t);
	}
	bad = block_sum_u32_256(bad, sh);
	if (threadIdx.x == 0u && bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// {1, degenerate} of every valid triangle into the row of its component (a triangle belongs to label[T[i][0]])
__global__ __launch_bounds__(256) void k_topo_rows_triangles(const uint32_t *__restrict__ T, uint64_t nT, uint64_t chunk, uint64_t nV, const uint32_t *__restrict__ label,
                                                             const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank, unsigned long long *rows,
                                                             unsigned long long *__restrict__ bad_out) {
	const int col[2] = {TC_NT, TC_DEGENERATE};
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nT ? beg + chunk : nT;
	const uint32_t lane = threadIdx.x & 63u;
	TopoHeld<2> held;
	held.key = TOPO_NONE;
	uint32_t bad = 0u;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {
		const uint64_t i = base + lane;
		uint32_t key = TOPO_NONE, x[2] = {0u, 0u};
		if (i < end) {
			const uint32_t *t = T + i * 3u;
			const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
			if (t0 < nV && t1 < nV && t2 < nV) {  // (the others: k_topo_insert has counted them)
				key = topo_row(t0, nV, label, flags, rank);
				if (key == TOPO_NONE) bad++;
				else { x[0] = 1u; x[1] = t0 == t1 || t1 == t2 || t2 == t0 ? 1u : 0u; }
			}
		}
		held.step(rows, col, key, x);
	}
	held.flush(rows, col);
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// 1 per referenced vertex and 1 per boundary loop - a root of `loop` that ends a boundary edge: the smallest vertex of its
// loop - into the row of the vertex's component, and the root's own index
__global__ __launch_bounds__(256) void k_topo_rows_vertices(uint64_t nV, uint64_t chunk, const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ rank, const uint32_t *__restrict__ loop, const uint8_t *__restrict__ bflag,
                                                            unsigned long long *rows, TopoOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const int col[2] = {TC_NV, TC_LOOPS};
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nV ? beg + chunk : nV;
	const uint32_t lane = threadIdx.x & 63u;
	TopoHeld<2> held;
	held.key = TOPO_NONE;
	uint32_t loops = 0u;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {
		const uint64_t v = base + lane;
		uint32_t key = TOPO_NONE, x[2] = {0u, 0u};
		if (v < end) {
			const uint32_t is_loop = bflag[v] && loop[v] == (uint32_t)v ? 1u : 0u;
			loops += is_loop;
			key = topo_row((uint32_t)v, nV, label, flags, rank);  // (a vertex no triangle names is its own root and owns nothing)
			if (key != TOPO_NONE) {
				x[0] = 1u; x[1] = is_loop;
				if (label[v] == (uint32_t)v) rows[(uint64_t)key * TOPO_COLS + TC_ROOT] = v;
			}
		}
		held.step(rows, col, key, x);
	}
	held.flush(rows, col);
	loops = block_sum_u32_256(loops, sh);
	if (threadIdx.x == 0u && loops) atomicAdd(&out->loops, (unsigned long long)loops);
}

// the rows of the table from the counters: Euler number and genus per component, and what the surface's struct says of them
__global__ __launch_bounds__(256) void k_topo_finish(const unsigned long long *__restrict__ rows, uint64_t ncomp, TopoRow *__restrict__ table,
                                                     TopoOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t closed = 0u, undefined = 0u;
	unsigned long long gsum = 0ull;
	for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < ncomp; r += (uint64_t)gridDim.x * 256u) {
		const unsigned long long *x = rows + r * TOPO_COLS;
		TopoRow t;
		t.root = (unsigned)x[TC_ROOT]; t.nV = (unsigned)x[TC_NV]; t.nT = (unsigned)x[TC_NT];
		t.edges = x[TC_EDGES]; t.boundary_edges = x[TC_BOUNDARY]; t.nonmanifold_edges = x[TC_NONMANIFOLD];
		t.misoriented_edges = x[TC_MISORIENTED]; t.degenerate_triangles = x[TC_DEGENERATE]; t.boundary_loops = x[TC_LOOPS];
		t.euler = ((long long)x[TC_NV] - (long long)x[TC_EDGES]) + (long long)x[TC_NT];
		const long long twice = (2 - t.euler) - (long long)x[TC_LOOPS];
		const bool defined = !x[TC_NONMANIFOLD] && !x[TC_DEGENERATE] && !x[TC_MISORIENTED] && twice >= 0 && !(twice & 1);
		t.genus = defined ? (int)(twice / 2) : -1;
		table[r] = t;
		closed += x[TC_BOUNDARY] ? 0u : 1u;
		if (defined) gsum += (unsigned long long)(twice / 2);
		else undefined++;
	}
	closed = block_sum_u32_256(closed, sh);
	undefined = block_sum_u32_256(undefined, sh);
	if (threadIdx.x == 0u) {
		if (closed) atomicAdd(&out->closed_components, (unsigned long long)closed);
		if (undefined) atomicAdd(&out->genus_undefined, (unsigned long long)undefined);
	}
	if (gsum) atomicAdd(&out->genus_sum, gsum);
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void topo_release(void *state) {
	TopoState *t = (TopoState *)state;
	dev_release(&t->d_slots); dev_release(&t->d_loop); dev_release(&t->d_bflag); dev_release(&t->d_label); dev_release(&t->d_rows); dev_release(&t->d_table);
}
static int topo_state(mc33hip_ctx *c, TopoState **t) {
	const int rc = meas_state(c);
	return rc ? rc : mesh_op_state(&c->meas->mesh, topo_release, t);
}

// Everything behind the labels, flags and the number of components (m->d_flags, the tile sums as cc_flag_and_count left them):
// ranks, the edge table, the rows, the table in t->d_table and the totals in t->d_out.  Enqueues; nT, nV, ncomp > 0.
static int topo_enqueue(mc33hip_ctx *c, TopoState *t, const void *dT, uint64_t nT, uint64_t nV, const uint32_t *dLabel, uint64_t ncomp) {
	MeasureState *m = c->meas;
	int rc;
	const uint64_t nslots = mesh_table_size(nT, 4u, 1ull << 40);
	if ((rc = meas_room(&m->d_rank, &m->rank_cap, nV))) return rc;
	if (t->slots_cap < nslots || !t->d_slots) {  // (a power of two as it is: no slack)
		if ((rc = dev_room("edge table", &t->d_slots, &t->slots_cap, nslots))) return rc;
	}
	if ((rc = meas_room(&t->d_loop, &t->loop_cap, nV))) return rc;
	if ((rc = meas_room(&t->d_bflag, &t->bflag_cap, nV))) return rc;
	if ((rc = meas_room(&t->d_rows, &t->rows_cap, ncomp * TOPO_COLS))) return rc;
	if ((rc = meas_room(&t->d_table, &t->table_cap, ncomp))) return rc;
	HIP_TRY(hipMemsetAsync(t->d_out, 0, sizeof(TopoOut), c->stream));
	HIP_TRY(hipMemsetAsync(t->d_bflag, 0, nV, c->stream));
	HIP_TRY(hipMemsetAsync(t->d_rows, 0, ncomp * TOPO_COLS * sizeof(unsigned long long), c->stream));
	// (8 blocks per CU where a block ends with a set of atomics, as for the component table)
	const uint32_t gridS = meas_grid(c, nslots, 8u), gridT = meas_grid(c, nT, 8u), gridV = meas_grid(c, nV, 8u);
	const uint64_t chunkS = ((nslots + gridS - 1u) / gridS + 255u) / 256u * 256u, chunkT = ((nT + gridT - 1u) / gridT + 255u) / 256u * 256u,
	               chunkV = ((nV + gridV - 1u) / gridV + 255u) / 256u * 256u;
	mesh_scan_sums<MeshFlag, MESH_RANK>(c, m->d_flags, nV, m->mesh.d_bsum, nullptr, m->d_rank);
	hipLaunchKernelGGL(k_mesh_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, (ulonglong2 *)t->d_slots, nslots, 0ull);
	hipLaunchKernelGGL(k_cc_init, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, t->d_loop, nV);
	hipLaunchKernelGGL(k_topo_insert, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, (const uint32_t *)dT, nT, nV, t->d_slots, nslots - 1u, t->d_out);
	hipLaunchKernelGGL(k_topo_classify, dim3(gridS), dim3(256), 0, c->stream, t->d_slots, nslots, chunkS, nV, dLabel, m->d_flags, m->d_rank, t->d_loop, t->d_bflag,
	                   t->d_rows, t->d_out, &m->d_out->bad);
	hipLaunchKernelGGL(k_cc_flatten, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, t->d_loop, nV);
	hipLaunchKernelGGL(k_topo_rows_triangles, dim3(gridT), dim3(256), 0, c->stream, (const uint32_t *)dT, nT, chunkT, nV, dLabel, m->d_flags, m->d_rank, t->d_rows,
	                   &m->d_out->bad);
	hipLaunchKernelGGL(k_topo_rows_vertices, dim3(gridV), dim3(256), 0, c->stream, nV, chunkV, dLabel, m->d_flags, m->d_rank, t->d_loop, t->d_bflag, t->d_rows, t->d_out);
	hipLaunchKernelGGL(k_topo_finish, dim3(meas_grid(c, ncomp, 8u)), dim3(256), 0, c->stream, t->d_rows, ncomp, t->d_table, t->d_out);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(t->h_out, t->d_out, sizeof(TopoOut), hipMemcpyDeviceToHost, c->stream));
	return 0;
}

static int topo_full(unsigned long long n) {
	if (!n) return 0;
	set_err("%llu sides found no slot in the edge table", n);
	return MC33HIP_ERUNTIME;
}

extern "C" int mc33hip_surface_topology(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, mc33hip_topology *out) {
	if (!c || !out || (nT && !dT) || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	TopoState *t;
	if ((rc = topo_state(c, &t))) return rc;
	MeasureState *m = c->meas;
	memset(out, 0, sizeof *out);
	out->nV = nV; out->nT = nT;
	out->closed = out->manifold = out->oriented = out->genus_defined = 1;
	if (!nT) return MC33HIP_OK;
	if (!nV) return mesh_bad(nT, nV);  // (every triangle names a vertex outside the 0 rows of V)
	// the labels, in scratch of this call's own: what mc33hip_label_components does
	if ((rc = meas_room(&t->d_label, &t->label_cap, nV))) return rc;
	if ((rc = meas_zero_counters(c))) return rc;
	hipLaunchKernelGGL(k_cc_init, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, t->d_label, (uint64_t)nV);
	hipLaunchKernelGGL(k_cc_union, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, (const uint32_t *)dT, (uint64_t)nT, (uint64_t)nV, t->d_label, &m->d_out->bad);
	hipLaunchKernelGGL(k_cc_flatten, dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, t->d_label, (uint64_t)nV);
	HIP_TRY(hipGetLastError());
	if ((rc = cc_flag_and_count(c, dT, nT, nV, t->d_label, false))) return rc;
	if ((rc = meas_fetch(c))) return rc;
	const unsigned long long invalid = m->h_out->bad, ncomp = m->h_out->comps, unref = m->h_out->unref;
	out->referenced_vertices = nV - unref;
	out->components = ncomp;
	out->euler = (long long)out->referenced_vertices;
	if (!ncomp) return mesh_bad(invalid, nV);  // (no valid triangle)
	if ((rc = meas_zero_counters(c))) return rc;
	if ((rc = topo_enqueue(c, t, dT, nT, nV, t->d_label, ncomp))) return rc;
	if ((rc = meas_fetch(c))) return rc;
	const TopoOut &h = *t->h_out;
	if ((rc = topo_full(h.full))) return rc;
	out->edges = h.edges; out->boundary_edges = h.boundary; out->nonmanifold_edges = h.nonmanifold; out->misoriented_edges = h.misoriented;
	out->degenerate_triangles = h.degenerate; out->boundary_loops = h.loops;
	out->closed_components = h.closed_components; out->genus_sum = h.genus_sum;
	out->euler = ((long long)out->referenced_vertices - (long long)h.edges) + (long long)(nT - h.invalid);
	out->closed = h.boundary == 0; out->manifold = h.nonmanifold == 0 && h.degenerate == 0; out->oriented = h.misoriented == 0;
	out->genus_defined = h.genus_undefined == 0;
	return mesh_bad(h.invalid + m->h_out->bad, nV);
}

extern "C" int mc33hip_component_topology(mc33hip_ctx *c, const void *dT, unsigned long long nT, unsigned long long nV, const unsigned *dLabel,
                                          struct mc33hip_component_topology *host_table, unsigned long long capacity, unsigned long long *components) {
	if (!c || !components || (nV && !dLabel) || (nT && !dT) || (capacity && !host_table) || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	TopoState *t;
	if ((rc = topo_state(c, &t))) return rc;
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
	if ((rc = meas_zero_counters(c))) return rc;
	if ((rc = topo_enqueue(c, t, dT, nT, nV, dLabel, ncomp))) return rc;
	HIP_TRY(hipMemcpyAsync(host_table, t->d_table, ncomp * sizeof(TopoRow), hipMemcpyDeviceToHost, c->stream));
	if ((rc = meas_fetch(c))) return rc;
	if ((rc = topo_full(t->h_out->full))) return rc;
	return mesh_bad(t->h_out->invalid + m->h_out->bad, nV);
}
