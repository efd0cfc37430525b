// mc33_simplify.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h, and on mc33_smooth.hip.h for the normals of its output; not a header to include elsewhere):
// vertex clustering of a FINISHED mesh in device memory on an axis-aligned lattice - every lattice cell's vertices become one,
// triangles that lose a corner or repeat another go - so that a surface of the resolution a caller wants crosses the link
// (include/mc33_hip.h: mc33hip_simplify_surface).  DESIGN.md 14.
//
// The definition is in include/mc33_hip.h; tests/simplify_oracle.py restates it in numpy.  Integer atomics and exclusive scans
// decide everything: the result is an exact function of the input.
// The passes: k_mesh_ref flags the referenced vertices; k_simp_cluster, the hot path, a lane per vertex, claims the slot of the
// vertex's key in the table of mc33_mesh.hip.h and adds into it - atomicMin of the representative, atomicAdd of the member count
// and of the three 64-bit sums - once per run of equal keys in a wave; k_simp_reps gathers rep(v) and counts clusters;
// k_simp_tri_insert enters the images that are not collapsed into a table of 32-bit words that hold TRIANGLE INDICES - the key of a word is recomputed
// from the triangle it names, the smallest index of an image stays by atomicMin -; k_simp_tri_keep flags the survivors and
// their representatives; the tile scans of mc33_mesh.hip.h place vertices and triangles; k_simp_rows and
// k_simp_tris write.  Nothing a block wrote with plain stores is read by another block of the same kernel: slots, reps, counts
// and sums are atomics, their readers are later kernels.

struct SimpSlot { unsigned long long key; uint32_t rep, cnt; unsigned long long sum[3]; };  // 40 bytes; keys have 63 bits
struct SimpLattice { double origin[3], cell[3]; };

constexpr double SIMP_CELLS = 2097152.0;          // 2^21 cells per axis
constexpr double SIMP_UNIT = 4294967296.0;        // 2^32 steps inside a cell

struct SimpOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long nV_out, nT_out, clusters, max_cluster, collapsed, duplicates, bad, clamped;
	unsigned long long full;      // keys or images that found no slot (cannot happen: the tables are larger than what enters; checked all the same)
	unsigned long long pad_[3];
};

struct SimpState {          // scratch of these passes besides the shared keep (1: a surviving triangle names this representative), map (new[r]) and
                            // tile sums (the vertex tiles, behind them the triangle tiles): on the MeasureState from the first call on, grown on demand, freed with it
	SimpOut *d_out, *h_out;
	uint8_t *d_ref;         // [nV] referenced
	uint64_t ref_cap;
	uint32_t *d_slot;       // [nV] the slot of the vertex's cluster, MESH_NONE where no triangle names it
	uint64_t slot_cap;
	uint32_t *d_rep;        // [nV] rep(v), MESH_NONE likewise
	uint64_t rep_cap;
	uint8_t *d_surv;        // [nT] 1: the triangle survives
	uint64_t surv_cap;
	SimpSlot *d_slots;      // the cluster table: a power of two >= 2 nV slots
	uint64_t slots_cap;
	uint32_t *d_tri;        // the image table: a power of two >= 2 nT words
	uint64_t tri_cap;
};

// key and position inside the cell of one coordinate; returns 1 when it was clamped
__device__ __forceinline__ uint32_t simp_axis(double x, double origin, double cell, unsigned long long *k, double *t) {
	const double g = (x - origin) / cell;
	uint32_t clamped = 0u;
	unsigned long long ka;
	if (!(g >= 0.0)) { ka = 0ull; clamped = 1u; }
	else if (g >= SIMP_CELLS) { ka = 2097151ull; clamped = 1u; }
	else ka = (unsigned long long)floor(g);
	double ta = g - (double)ka;
	if (!(ta >= 0.0)) ta = 0.0;  // (NaN too)
	else if (ta > 1.0) ta = 1.0;
	*k = ka; *t = ta;
	return clamped;
}

__global__ __launch_bounds__(256) void k_simp_clear(SimpSlot *__restrict__ slots, uint64_t n) {
	for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256u) {
		SimpSlot e;
		e.key = MESH_EMPTY; e.rep = MESH_NONE; e.cnt = 0u; e.sum[0] = e.sum[1] = e.sum[2] = 0ull;
		slots[s] = e;
	}
}

// The hot path.  Every block a contiguous piece of V, every wave 64 consecutive vertices a step; every lane of the wave takes
// every step.  The emit stage's order is spatially coherent: most of a step's lanes share a few keys, and consecutive lanes with
// one key are a run - its first lane (the smallest v of the run) claims the slot (mesh_claim) and adds the run's sums.
// A slot that takes thousands of members scattered over the array takes as many atomics: slow, and as right as any other.
template <typename R>
__global__ __launch_bounds__(256) void k_simp_cluster(const R *__restrict__ V, const uint8_t *__restrict__ ref, uint64_t nV, uint64_t chunk, SimpLattice L, uint32_t mean,
                                                      SimpSlot *slots, uint64_t mask, uint32_t *__restrict__ slotof, SimpOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nV ? beg + chunk : nV;
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t clamped = 0u, full = 0u;
	for (uint64_t base = beg + (threadIdx.x & ~63u); base < end; base += 256u) {  // (wave-uniform)
		const uint64_t v = base + lane;
		unsigned long long key = MESH_EMPTY, q[3] = {0ull, 0ull, 0ull};
		if (v < end && ref[v]) {
			const R *p = V + v * 3u;
			unsigned long long k[3];
			uint32_t cl = 0u;
#pragma unroll
			for (int a = 0; a < 3; a++) {
				double t;
				cl |= simp_axis((double)p[a], L.origin[a], L.cell[a], &k[a], &t);
				q[a] = (unsigned long long)floor(t * SIMP_UNIT);
			}
			clamped += cl;
			key = k[0] | (k[1] << 21) | (k[2] << 42);
		}
		const uint32_t before_lo = __shfl_up((uint32_t)key, 1, 64), before_hi = __shfl_up((uint32_t)(key >> 32), 1, 64);
		const bool head = lane == 0u || (((unsigned long long)before_hi << 32) | before_lo) != key;
		const unsigned long long heads = __ballot(head);
		const uint32_t n = run_sum_u32(key != MESH_EMPTY ? 1u : 0u, heads, lane);
		if (mean) {  // (uniform)
#pragma unroll
			for (int a = 0; a < 3; a++) q[a] = run_sum_u64(q[a], heads, lane);
		}
		uint32_t slot = MESH_NONE;
		if (head && key != MESH_EMPTY) {
			const uint64_t s = mesh_claim(slots, mask, key);
			if (s != MESH_NOSLOT) {
				slot = (uint32_t)s;
				atomicMin(&slots[slot].rep, (uint32_t)v);
				atomicAdd(&slots[slot].cnt, n);
				if (mean) {
					atomicAdd(&slots[slot].sum[0], q[0]);
					atomicAdd(&slots[slot].sum[1], q[1]);
					atomicAdd(&slots[slot].sum[2], q[2]);
				}
			} else full++;
		}
		const int first = 63 - __clzll((long long)(heads & (~0ull >> (63u - lane))));  // the lane that began this lane's run (lane 0 begins one)
		slot = __shfl(slot, first, 64);
		if (v < end) slotof[v] = key != MESH_EMPTY ? slot : MESH_NONE;
	}
	clamped = block_sum_u32_256(clamped, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (clamped) atomicAdd(&out->clamped, (unsigned long long)clamped);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// rep(v) out of the table, and the two counts of clusters (a cluster is counted where v is its representative)
__global__ __launch_bounds__(256) void k_simp_reps(const SimpSlot *__restrict__ slots, const uint32_t *__restrict__ slotof, uint64_t nV, uint32_t *__restrict__ rep,
                                                   SimpOut *__restrict__ out) {
	uint32_t n = 0u, maxc = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t s = slotof[v];
		uint32_t r = MESH_NONE;
		if (s != MESH_NONE) {
			r = slots[s].rep;
			if (r == (uint32_t)v) {
				const uint32_t c = slots[s].cnt;
				n++;
				maxc = c > maxc ? c : maxc;
			}
		}
		rep[v] = r;
	}
	n = wave_sum_u32(n); maxc = wave_max_u32(maxc);
	if ((threadIdx.x & 63u) == 0u) {
		if (n) atomicAdd(&out->clusters, (unsigned long long)n);
		if (maxc) atomicMax(&out->max_cluster, (unsigned long long)maxc);
	}
}

// the image of triangle i, ascending in s[]: 0 invalid (or a vertex without a slot: the table was full), 1 collapsed, 2 neither
__device__ __forceinline__ uint32_t simp_image(const uint32_t *__restrict__ T, uint64_t i, uint64_t nV, const uint32_t *__restrict__ rep, uint32_t r[3], uint32_t s[3]) {
	const uint32_t *t = T + i * 3u;
	const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
	if (t0 >= nV || t1 >= nV || t2 >= nV) return 0u;  // (tested before anything is gathered through it)
	r[0] = rep[t0]; r[1] = rep[t1]; r[2] = rep[t2];
	if (r[0] == MESH_NONE || r[1] == MESH_NONE || r[2] == MESH_NONE) return 0u;
	if (r[0] == r[1] || r[1] == r[2] || r[2] == r[0]) return 1u;
	uint32_t a = r[0], b = r[1], c = r[2], x;
	if (a > b) { x = a; a = b; b = x; }
	if (b > c) { x = b; b = c; c = x; }
	if (a > b) { x = a; a = b; b = x; }
	s[0] = a; s[1] = b; s[2] = c;
	return 2u;
}
__device__ __forceinline__ uint64_t simp_image_home(const uint32_t s[3]) {
	return mesh_mix(mesh_mix(((uint64_t)s[0] << 32) | s[1]) + s[2]);
}

// Duplicate removal, first half.  A word of the table names a triangle; the word's key is that triangle's sorted image, read
// through T and rep - inputs of earlier kernels.  An empty word takes i; a word whose triangle has i's image takes min(itself, i)
// - whatever it holds afterwards has that image still -; any other word: probe on.
__global__ __launch_bounds__(256) void k_simp_tri_insert(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ rep, uint32_t *tab,
                                                         uint64_t mask, SimpOut *__restrict__ out) {
	uint32_t full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		uint32_t r[3], s[3], rj[3], sj[3];
		if (simp_image(T, i, nV, rep, r, s) != 2u) continue;
		uint64_t h = simp_image_home(s) & mask;
		bool placed = false;
		for (uint64_t tries = 0; tries <= mask; tries++, h = (h + 1u) & mask) {
			const uint32_t old = atomicCAS(&tab[h], MESH_NONE, (uint32_t)i);
			if (old == MESH_NONE) { placed = true; break; }
			if (simp_image(T, old, nV, rep, rj, sj) == 2u && sj[0] == s[0] && sj[1] == s[1] && sj[2] == s[2]) {
				atomicMin(&tab[h], (uint32_t)i);
				placed = true;
				break;
			}
		}
		if (!placed) full++;
	}
	if (full) atomicAdd(&out->full, (unsigned long long)full);
}

// Second half: triangle i survives iff the word of its image holds i (drop == 0: iff it is valid and not collapsed).  The
// representatives of the survivors are marked, and only theirs.
__global__ __launch_bounds__(256) void k_simp_tri_keep(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ rep,
                                                       const uint32_t *__restrict__ tab, uint64_t mask, uint32_t drop, uint8_t *__restrict__ surv,
                                                       uint8_t *__restrict__ keep, SimpOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t collapsed = 0u, dup = 0u, full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		uint32_t r[3], s[3], rj[3], sj[3];
		const uint32_t kind = simp_image(T, i, nV, rep, r, s);
		uint32_t alive = kind == 2u ? 1u : 0u;
		if (kind == 1u) collapsed++;
		if (alive && drop) {
			uint64_t h = simp_image_home(s) & mask;
			bool found = false;
			for (uint64_t tries = 0; tries <= mask; tries++, h = (h + 1u) & mask) {
				const uint32_t j = tab[h];
				if (j == MESH_NONE) break;  // (the insertion found no slot: counted there)
				if (j == (uint32_t)i) { found = true; break; }
				if (simp_image(T, j, nV, rep, rj, sj) == 2u && sj[0] == s[0] && sj[1] == s[1] && sj[2] == s[2]) { found = true; alive = 0u; dup++; break; }
			}
			if (!found) { alive = 0u; full++; }
		}
		surv[i] = (uint8_t)alive;
		if (alive) { keep[r[0]] = 1; keep[r[1]] = 1; keep[r[2]] = 1; }
	}
	collapsed = block_sum_u32_256(collapsed, sh);
	dup = block_sum_u32_256(dup, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (collapsed) atomicAdd(&out->collapsed, (unsigned long long)collapsed);
		if (dup) atomicAdd(&out->duplicates, (unsigned long long)dup);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// the survivors of a tile, renumbered, at the tile's place in oT
__global__ __launch_bounds__(256) void k_simp_tris(const uint32_t *__restrict__ T, uint64_t nT, const uint32_t *__restrict__ rep, const uint8_t *__restrict__ surv,
                                                   const uint32_t *__restrict__ map, const uint32_t *__restrict__ bsum, const SimpOut *__restrict__ out, uint64_t capV,
                                                   uint64_t capT, uint32_t *__restrict__ oT) {
	__shared__ uint32_t sh[256];
	if (out->nV_out > capV || out->nT_out > capT) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	const uint64_t i0 = mesh_tile_e0();
	uint32_t f[4];
	const uint32_t own = mesh_tile_load<MeshFlag>(surv, nT, f);
	uint64_t r = mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		if (f[k]) {
			const uint32_t *t = T + (i0 + k) * 3u;  // (a survivor is valid and its three representatives are kept)
			const uint32_t m0 = map[rep[t[0]]], m1 = map[rep[t[1]]], m2 = map[rep[t[2]]];
			uint32_t *o = oT + r * 3u;
			o[0] = m0; o[1] = m1; o[2] = m2;
			r++;
		}
	}
}

// oMap for every vertex; for a kept representative its row of oV - the bytes of its own row, or the mean of its cluster out of
// the slot's integers - and its attribute words.  R: MC33_real - a row of V is 12 or 24 bytes.
template <typename R>
__global__ __launch_bounds__(256) void k_simp_rows(const R *__restrict__ V, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                                   const uint32_t *__restrict__ rep, const uint32_t *__restrict__ slotof, const SimpSlot *__restrict__ slots,
                                                   const uint32_t *__restrict__ map, uint64_t nV, SimpLattice L, uint32_t mean, const SimpOut *__restrict__ out,
                                                   uint64_t capV, uint64_t capT, R *__restrict__ oV, uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1,
                                                   uint32_t *__restrict__ oMap) {
	if (out->nV_out > capV || out->nT_out > capT) return;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t r = rep[v];
		const uint32_t m = r != MESH_NONE ? map[r] : MESH_NONE;
		if (oMap) oMap[v] = m;
		if (m == MESH_NONE || r != (uint32_t)v) continue;
		R *oq = oV + (uint64_t)m * 3u;
		if (mean) {
			const SimpSlot *s = slots + slotof[v];
			const unsigned long long key = s->key;
			const double den = (double)s->cnt * SIMP_UNIT;
#pragma unroll
			for (int a = 0; a < 3; a++) {
				const double k = (double)((key >> (21 * a)) & 0x1FFFFFull);
				const double mm = (double)s->sum[a] / den;
				oq[a] = (R)(L.origin[a] + L.cell[a] * (k + mm));
			}
		} else {
			mesh_copy_row(V, (const float *)nullptr, v, oV, (float *)nullptr, m);
		}
		if (A0) oA0[m] = A0[v];
		if (A1) oA1[m] = A1[v];
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void simp_release(void *state) {
	SimpState *s = (SimpState *)state;
	dev_release(&s->d_ref); dev_release(&s->d_slot); dev_release(&s->d_rep); dev_release(&s->d_surv); dev_release(&s->d_slots); dev_release(&s->d_tri);
}
static int simp_state(mc33hip_ctx *c, SimpState **s) {
	const int rc = meas_state(c);
	return rc ? rc : mesh_op_state(&c->meas->mesh, simp_release, s);
}

static void simp_fill(mc33hip_simplification *a, const SimpOut &h) {
	a->nV_out = h.nV_out; a->nT_out = h.nT_out; a->clusters = h.clusters; a->max_cluster = h.max_cluster;
	a->collapsed_triangles = h.collapsed; a->duplicate_triangles = h.duplicates; a->invalid_triangles = h.bad; a->clamped_vertices = h.clamped;
}

extern "C" int mc33hip_simplify_surface(mc33hip_ctx *c, mc33hip_simplification *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nV_out = a->nT_out = a->clusters = a->max_cluster = a->collapsed_triangles = a->duplicate_triangles = a->invalid_triangles = a->clamped_vertices = 0;
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_counts_ok(a->n_attr, nV, nT)) return MC33HIP_EINVAL;
	if (a->mode != MC33HIP_SIMPLIFY_MEAN && a->mode != MC33HIP_SIMPLIFY_FIRST) { set_err("mode %d is neither MC33HIP_SIMPLIFY_MEAN nor MC33HIP_SIMPLIFY_FIRST", a->mode); return MC33HIP_EINVAL; }
	for (int k = 0; k < 3; k++) {
		if (!(a->cell[k] > 0.0 && a->cell[k] < __builtin_huge_val())) { set_err("cell[%d] must be finite and > 0", k); return MC33HIP_EINVAL; }
		if (!(a->origin[k] > -__builtin_huge_val() && a->origin[k] < __builtin_huge_val())) { set_err("origin[%d] must be finite", k); return MC33HIP_EINVAL; }
	}
	const uint64_t capV = mesh_cap(a->capV), capT = mesh_cap(a->capT);
	if (!mesh_pointers_ok((nV && !a->V) || (nT && !a->T) || (capV && !a->oV) || (capT && !a->oT), a->n_attr, a->attr, a->oAttr, nV, capV)) return MC33HIP_EINVAL;
	// the call is not in place: no output may share a byte with an input or with another output
	const MeshRange in[4] = {{a->V, nV * 3u * sizeof(real_t)}, {a->T, nT * 12u}, {a->n_attr > 0u ? a->attr[0] : nullptr, nV * 4u}, {a->n_attr > 1u ? a->attr[1] : nullptr, nV * 4u}};
	const MeshRange out[6] = {{a->oV, capV * 3u * sizeof(real_t)}, {a->oT, capT * 12u}, {a->oN, capV * 12u}, {a->oMap, nV * 4u}, {a->n_attr > 0u ? a->oAttr[0] : nullptr, capV * 4u},
	                          {a->n_attr > 1u ? a->oAttr[1] : nullptr, capV * 4u}};
	if (!mesh_ranges_ok(in, 4, out, 6, true, "simplification")) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	SimpState *s;
	if ((rc = simp_state(c, &s))) return rc;
	if (!nT || !nV) {  // every count is 0
		if ((rc = mesh_empty(c, a->oMap, nV))) return rc;
		a->invalid_triangles = nT;
		return mesh_bad(nT, nV);
	}
	MeshHost &h = c->meas->mesh;
	const uint64_t tilesV = (nV + MESH_TILE - 1u) / MESH_TILE, tilesT = (nT + MESH_TILE - 1u) / MESH_TILE;
	const uint64_t nslots = mesh_table_size(nV, 2u, 1ull << 32), ntri = a->drop_duplicates ? mesh_table_size(nT, 2u, 1ull << 32) : 0u;  // (slot numbers are 32-bit words)
	if ((rc = meas_scratch(c, nV, tilesV + tilesT))) return rc;
	if ((rc = meas_room(&s->d_ref, &s->ref_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_slot, &s->slot_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_rep, &s->rep_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_surv, &s->surv_cap, nT))) return rc;
	if ((s->slots_cap < nslots || !s->d_slots) && (rc = dev_room("cluster table", &s->d_slots, &s->slots_cap, nslots))) return rc;  // (powers of two as they are: no slack)
	if (ntri && (s->tri_cap < ntri || !s->d_tri) && (rc = dev_room("image table", &s->d_tri, &s->tri_cap, ntri))) return rc;
	uint32_t *bsumV = h.d_bsum, *bsumT = h.d_bsum + tilesV;
	const real_t *V = (const real_t *)a->V;
	const uint32_t *T = (const uint32_t *)a->T;
	const uint32_t mean = a->mode == MC33HIP_SIMPLIFY_MEAN ? 1u : 0u, drop = a->drop_duplicates ? 1u : 0u;
	SimpLattice L;
	for (int k = 0; k < 3; k++) { L.origin[k] = a->origin[k]; L.cell[k] = a->cell[k]; }
	// (8 blocks per CU where a block ends with a set of atomics, as for the component table)
	const uint32_t gridV = meas_grid(c, nV, 16u), gridT = meas_grid(c, nT, 16u), gridC = meas_grid(c, nV, 8u);
	const uint64_t chunkC = ((nV + gridC - 1u) / gridC + 255u) / 256u * 256u;
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(SimpOut), c->stream));
	HIP_TRY(hipMemsetAsync(s->d_ref, 0, nV, c->stream));
	HIP_TRY(hipMemsetAsync(h.d_keep, 0, nV, c->stream));
	if (ntri) HIP_TRY(hipMemsetAsync(s->d_tri, 0xFF, ntri * sizeof(uint32_t), c->stream));
	hipLaunchKernelGGL(k_simp_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, s->d_slots, nslots);
	hipLaunchKernelGGL(k_mesh_ref, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_ref, &s->d_out->bad);
	hipLaunchKernelGGL((k_simp_cluster<real_t>), dim3(gridC), dim3(256), 0, c->stream, V, s->d_ref, (uint64_t)nV, chunkC, L, mean, s->d_slots, nslots - 1u, s->d_slot,
	                   s->d_out);
	hipLaunchKernelGGL(k_simp_reps, dim3(gridV), dim3(256), 0, c->stream, s->d_slots, s->d_slot, (uint64_t)nV, s->d_rep, s->d_out);
	if (drop) hipLaunchKernelGGL(k_simp_tri_insert, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_rep, s->d_tri, ntri - 1u, s->d_out);
	hipLaunchKernelGGL(k_simp_tri_keep, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_rep, s->d_tri, ntri ? ntri - 1u : 0u, drop, s->d_surv,
	                   h.d_keep, s->d_out);
	mesh_scan<MeshFlag, MESH_NEW>(c, h.d_keep, nV, bsumV, &s->d_out->nV_out, h.d_map);
	mesh_scan<MeshFlag>(c, s->d_surv, nT, bsumT, &s->d_out->nT_out);  // (k_simp_tris places)
	// the copies: they compare the totals with the capacities on the device, so that the host waits once before the normals
	hipLaunchKernelGGL((k_simp_rows<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, (const uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr),
	                   (const uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr), s->d_rep, s->d_slot, s->d_slots, h.d_map, (uint64_t)nV, L, mean, s->d_out, capV, capT,
	                   (real_t *)a->oV, (uint32_t *)(a->n_attr > 0u ? a->oAttr[0] : nullptr), (uint32_t *)(a->n_attr > 1u ? a->oAttr[1] : nullptr), (uint32_t *)a->oMap);
	hipLaunchKernelGGL(k_simp_tris, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, s->d_rep, s->d_surv, h.d_map, bsumT, s->d_out, capV, capT,
	                   (uint32_t *)a->oT);
	if ((rc = mesh_op_fetch(c, s))) return rc;
	const SimpOut o = *s->h_out;
	simp_fill(a, o);
	if (o.full) { set_err("%llu keys or images found no slot in the tables", o.full); return MC33HIP_ERUNTIME; }
	if ((rc = mesh_capacity("simplified", o.nV_out, o.nT_out, capV, capT))) return rc;
	// The normals of the output.  Every kernel of this call has run: of the shared scratch its map and keep are dead, and the tile
	// sums - all the normals overwrite - have been read for the last time.
	if (a->oN && o.nV_out && (rc = sm_normals_call(c, (const real_t *)a->oV, (const uint32_t *)a->oT, o.nT_out, o.nV_out, a->oN, nullptr))) return rc;
	return mesh_bad(o.bad, nV);
}
