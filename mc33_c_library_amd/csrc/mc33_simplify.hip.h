// mc33_simplify.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, last; not a header to include elsewhere):
// vertex clustering of a FINISHED mesh in device memory on an axis-aligned lattice - every lattice cell's vertices become one,
// triangles that lose a corner or repeat another go - so that a surface of the resolution a caller wants crosses the link
// (include/mc33_hip.h: mc33hip_simplify_surface).  DESIGN.md 14.
//
// The definition is in include/mc33_hip.h; tests/simplify_oracle.py restates it in numpy.  Integer atomics and exclusive scans
// decide everything: the result is an exact function of the input.
// The passes: k_simp_ref flags the referenced vertices (the form of k_filt_ref); k_simp_cluster, the hot path, a lane per vertex,
// claims the slot of the vertex's key in an open-addressing table by 64-bit compare-and-swap (the table of mc33_topology.hip.h)
// and adds into it - atomicMin of the representative, atomicAdd of the member count and of the three 64-bit sums - once per run
// of equal keys in a wave (the run sums of TopoHeld); k_simp_reps gathers rep(v) and counts clusters; k_simp_tri_insert enters
// the images that are not collapsed into a table of 32-bit words that hold TRIANGLE INDICES - the key of a word is recomputed
// from the triangle it names, the smallest index of an image stays by atomicMin -; k_simp_tri_keep flags the survivors and
// their representatives; k_simp_tile_count / k_filt_scan_top / k_filt_new are the scans of section 12; k_simp_rows and
// k_simp_tris write.  Nothing a block wrote with plain stores is read by another block of the same kernel: slots, reps, counts
// and sums are atomics, their readers are later kernels.

struct SimpSlot { unsigned long long key; uint32_t rep, cnt; unsigned long long sum[3]; };  // 40 bytes; key all ones: empty
struct SimpLattice { double origin[3], cell[3]; };

constexpr unsigned long long SIMP_EMPTY = ~0ull;  // (keys have 63 bits)
constexpr uint32_t SIMP_NONE = 0xFFFFFFFFu;
constexpr double SIMP_CELLS = 2097152.0;          // 2^21 cells per axis
constexpr double SIMP_UNIT = 4294967296.0;        // 2^32 steps inside a cell

struct SimpOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long nV_out, nT_out, clusters, max_cluster, collapsed, duplicates, bad, clamped;
	unsigned long long full;      // keys or images that found no slot (cannot happen: the tables are larger than what enters; checked all the same)
	unsigned long long pad_[3];
};

struct SimpState {          // scratch of these passes: on the MeasureState from the first call on, grown on demand, freed with it
	SimpOut *d_out, *h_out;
	uint8_t *d_ref;         // [nV] referenced
	uint64_t ref_cap;
	uint32_t *d_slot;       // [nV] the slot of the vertex's cluster, SIMP_NONE where no triangle names it
	uint64_t slot_cap;
	uint32_t *d_rep;        // [nV] rep(v), SIMP_NONE likewise
	uint64_t rep_cap;
	uint8_t *d_keep;        // [nV] 1: a surviving triangle names this representative
	uint64_t keep_cap;
	uint32_t *d_map;        // [nV] new[r], FILT_NONE where r is not a kept representative
	uint64_t map_cap;
	uint8_t *d_surv;        // [nT] 1: the triangle survives
	uint64_t surv_cap;
	uint32_t *d_bsum;       // flags per tile, scanned in place: the vertex tiles, behind them the triangle tiles
	uint64_t bsum_cap;
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

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long x, int d) {
	const uint32_t lo = __shfl_down((uint32_t)x, d, 64), hi = __shfl_down((uint32_t)(x >> 32), d, 64);
	return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long run_sum_u64(unsigned long long x, unsigned long long heads, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = shfl_down_u64(x, d);
		if (run_open(heads, lane, d)) x += o;
	}
	return x;
}

__global__ __launch_bounds__(256) void k_simp_clear(SimpSlot *__restrict__ slots, uint64_t n) {
	for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256u) {
		SimpSlot e;
		e.key = SIMP_EMPTY; e.rep = SIMP_NONE; e.cnt = 0u; e.sum[0] = e.sum[1] = e.sum[2] = 0ull;
		slots[s] = e;
	}
}

__global__ __launch_bounds__(256) void k_simp_ref(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, uint8_t *__restrict__ ref, SimpOut *__restrict__ out) {
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		ref[t0] = 1; ref[t1] = 1; ref[t2] = 1;  // (every racing store writes the same 1)
	}
	if (bad) atomicAdd(&out->bad, (unsigned long long)bad);
}

// The hot path.  Every block a contiguous piece of V, every wave 64 consecutive vertices a step; every lane of the wave takes
// every step.  The emit stage's order is spatially coherent: most of a step's lanes share a few keys, and consecutive lanes with
// one key are a run - its first lane (the smallest v of the run) claims the slot and adds the run's sums.  What the
// compare-and-swap on the key RETURNS decides - empty or equal: this is the cluster's slot; anything else: probe on, linearly.
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
		unsigned long long key = SIMP_EMPTY, q[3] = {0ull, 0ull, 0ull};
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
		const uint32_t n = run_sum_u32(key != SIMP_EMPTY ? 1u : 0u, heads, lane);
		if (mean) {  // (uniform)
#pragma unroll
			for (int a = 0; a < 3; a++) q[a] = run_sum_u64(q[a], heads, lane);
		}
		uint32_t slot = SIMP_NONE;
		if (head && key != SIMP_EMPTY) {
			uint64_t s = topo_mix(key) & mask;
			for (uint64_t tries = 0; tries <= mask; tries++, s = (s + 1u) & mask) {
				const unsigned long long old = atomicCAS(&slots[s].key, SIMP_EMPTY, key);
				if (old == SIMP_EMPTY || old == key) { slot = (uint32_t)s; break; }
			}
			if (slot != SIMP_NONE) {
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
		if (v < end) slotof[v] = key != SIMP_EMPTY ? slot : SIMP_NONE;
	}
	clamped = topo_block_sum(clamped, sh);
	full = topo_block_sum(full, sh);
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
		uint32_t r = SIMP_NONE;
		if (s != SIMP_NONE) {
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
	if (r[0] == SIMP_NONE || r[1] == SIMP_NONE || r[2] == SIMP_NONE) return 0u;
	if (r[0] == r[1] || r[1] == r[2] || r[2] == r[0]) return 1u;
	uint32_t a = r[0], b = r[1], c = r[2], x;
	if (a > b) { x = a; a = b; b = x; }
	if (b > c) { x = b; b = c; c = x; }
	if (a > b) { x = a; a = b; b = x; }
	s[0] = a; s[1] = b; s[2] = c;
	return 2u;
}
__device__ __forceinline__ uint64_t simp_image_home(const uint32_t s[3]) {
	return topo_mix(topo_mix(((uint64_t)s[0] << 32) | s[1]) + s[2]);
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
			const uint32_t old = atomicCAS(&tab[h], SIMP_NONE, (uint32_t)i);
			if (old == SIMP_NONE) { placed = true; break; }
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
				if (j == SIMP_NONE) break;  // (the insertion found no slot: counted there)
				if (j == (uint32_t)i) { found = true; break; }
				if (simp_image(T, j, nV, rep, rj, sj) == 2u && sj[0] == s[0] && sj[1] == s[1] && sj[2] == s[2]) { found = true; alive = 0u; dup++; break; }
			}
			if (!found) { alive = 0u; full++; }
		}
		surv[i] = (uint8_t)alive;
		if (alive) { keep[r[0]] = 1; keep[r[1]] = 1; keep[r[2]] = 1; }
	}
	collapsed = topo_block_sum(collapsed, sh);
	dup = topo_block_sum(dup, sh);
	full = topo_block_sum(full, sh);
	if (threadIdx.x == 0u) {
		if (collapsed) atomicAdd(&out->collapsed, (unsigned long long)collapsed);
		if (dup) atomicAdd(&out->duplicates, (unsigned long long)dup);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// the flags of a tile of CC_TILE elements, 4 per lane, counted
__global__ __launch_bounds__(256) void k_simp_tile_count(const uint8_t *__restrict__ flag, uint64_t n, uint32_t *__restrict__ bsum) {
	__shared__ uint32_t sh[4];
	const uint64_t e0 = (uint64_t)blockIdx.x * CC_TILE + threadIdx.x * 4u;
	uint32_t own = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++)
		if (e0 + k < n) own += flag[e0 + k] ? 1u : 0u;
	const uint32_t tot = block_sum_u32_256(own, sh);
	if (threadIdx.x == 0u) bsum[blockIdx.x] = tot;
}

// the survivors of a tile, renumbered, at the tile's place in oT
__global__ __launch_bounds__(256) void k_simp_tris(const uint32_t *__restrict__ T, uint64_t nT, const uint32_t *__restrict__ rep, const uint8_t *__restrict__ surv,
                                                   const uint32_t *__restrict__ map, const uint32_t *__restrict__ bsum, const SimpOut *__restrict__ out, uint64_t capV,
                                                   uint64_t capT, uint32_t *__restrict__ oT) {
	__shared__ uint32_t sh[256];
	if (out->nV_out > capV || out->nT_out > capT) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	const uint64_t i0 = (uint64_t)blockIdx.x * CC_TILE + threadIdx.x * 4u;
	uint32_t f[4], own = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		f[k] = i0 + k < nT && surv[i0 + k] ? 1u : 0u;
		own += f[k];
	}
	uint32_t tot;
	uint64_t r = (uint64_t)bsum[blockIdx.x] + block_excl_scan_256(own, sh, &tot);
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
		const uint32_t m = r != SIMP_NONE ? map[r] : FILT_NONE;
		if (oMap) oMap[v] = m;
		if (m == FILT_NONE || r != (uint32_t)v) continue;
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
			const R *q = V + v * 3u;
			const R q0 = q[0], q1 = q[1], q2 = q[2];
			oq[0] = q0; oq[1] = q1; oq[2] = q2;
		}
		if (A0) oA0[m] = A0[v];
		if (A1) oA1[m] = A1[v];
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void simp_destroy(MeasureState *m) {
	SimpState *s = m->simp;
	if (!s) return;
	dev_release(&s->d_out); dev_release(&s->d_ref); dev_release(&s->d_slot); dev_release(&s->d_rep); dev_release(&s->d_keep); dev_release(&s->d_map);
	dev_release(&s->d_surv); dev_release(&s->d_bsum); dev_release(&s->d_slots); dev_release(&s->d_tri);
	if (s->h_out) (void)hipHostFree(s->h_out);
	free(s);
	m->simp = nullptr;
}

static int simp_state(mc33hip_ctx *c) {
	int rc = meas_state(c);
	if (rc) return rc;
	SimpState *s = c->meas->simp;
	if (!s) {
		if (!(s = (SimpState *)calloc(1, sizeof *s))) return MC33HIP_ENOMEM;
		c->meas->simp = s;  // (what it holds so far goes with the context)
	}
	if (!s->d_out) HIP_TRY(hipMalloc(&s->d_out, sizeof(SimpOut)));
	if (!s->h_out) HIP_TRY(hipHostMalloc(&s->h_out, sizeof(SimpOut), hipHostMallocDefault));
	return 0;
}

static uint64_t simp_table_size(uint64_t n) {  // a power of two >= 2 n, at most 2^32 (> n all the same: slot numbers are 32-bit words)
	uint64_t s = 256u;
	while (s < 2u * n && s < (1ull << 32)) s <<= 1;
	return s;
}

static void simp_fill(mc33hip_simplification *a, const SimpOut &h) {
	a->nV_out = h.nV_out; a->nT_out = h.nT_out; a->clusters = h.clusters; a->max_cluster = h.max_cluster;
	a->collapsed_triangles = h.collapsed; a->duplicate_triangles = h.duplicates; a->invalid_triangles = h.bad; a->clamped_vertices = h.clamped;
}

extern "C" int mc33hip_simplify_surface(mc33hip_ctx *c, mc33hip_simplification *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nV_out = a->nT_out = a->clusters = a->max_cluster = a->collapsed_triangles = a->duplicate_triangles = a->invalid_triangles = a->clamped_vertices = 0;
	const unsigned long long nV = a->nV, nT = a->nT;
	if (a->n_attr > 2u) { set_err("at most two attribute arrays, not %u", a->n_attr); return MC33HIP_EINVAL; }
	if (!meas_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	if (a->mode != MC33HIP_SIMPLIFY_MEAN && a->mode != MC33HIP_SIMPLIFY_FIRST) { set_err("mode %d is neither MC33HIP_SIMPLIFY_MEAN nor MC33HIP_SIMPLIFY_FIRST", a->mode); return MC33HIP_EINVAL; }
	for (int k = 0; k < 3; k++) {
		if (!(a->cell[k] > 0.0 && a->cell[k] < __builtin_huge_val())) { set_err("cell[%d] must be finite and > 0", k); return MC33HIP_EINVAL; }
		if (!(a->origin[k] > -__builtin_huge_val() && a->origin[k] < __builtin_huge_val())) { set_err("origin[%d] must be finite", k); return MC33HIP_EINVAL; }
	}
	const uint64_t capV = std::min<unsigned long long>(a->capV, 0xFFFFFFFFull), capT = std::min<unsigned long long>(a->capT, 0xFFFFFFFFull);
	bool null = (nV && !a->V) || (nT && !a->T) || (capV && !a->oV) || (capT && !a->oT);
	for (unsigned k = 0; k < a->n_attr; k++) null = null || (nV && !a->attr[k]) || (capV && !a->oAttr[k]);
	if (null) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	// the call is not in place: no output may share a byte with an input or with another output
	const void *in[4] = {a->V, a->T, a->n_attr > 0u ? a->attr[0] : nullptr, a->n_attr > 1u ? a->attr[1] : nullptr};
	const uint64_t in_bytes[4] = {nV * 3u * sizeof(real_t), nT * 12u, nV * 4u, nV * 4u};
	const void *outp[6] = {a->oV, a->oT, a->oN, a->oMap, a->n_attr > 0u ? a->oAttr[0] : nullptr, a->n_attr > 1u ? a->oAttr[1] : nullptr};
	const uint64_t out_bytes[6] = {capV * 3u * sizeof(real_t), capT * 12u, capV * 12u, nV * 4u, capV * 4u, capV * 4u};
	for (int o = 0; o < 6; o++) {
		for (int i = 0; i < 4; i++)
			if (filt_ranges_meet(in[i], in_bytes[i], outp[o], out_bytes[o])) { set_err("an output array overlaps an input array: the simplification is not in place"); return MC33HIP_EINVAL; }
		for (int p = o + 1; p < 6; p++)
			if (filt_ranges_meet(outp[p], out_bytes[p], outp[o], out_bytes[o])) { set_err("two output arrays overlap"); return MC33HIP_EINVAL; }
	}
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = simp_state(c))) return rc;
	SimpState *s = c->meas->simp;
	if (!nT || !nV) {  // no valid triangle: nothing is referenced, every count is 0 (nV == 0: every triangle is invalid)
		if (nV && a->oMap) HIP_TRY(hipMemsetAsync(a->oMap, 0xFF, nV * 4u, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if ((rc = prop_check(c))) return rc;
		a->invalid_triangles = nT;
		return meas_bad(nT, nV);
	}
	const uint64_t tilesV = (nV + CC_TILE - 1u) / CC_TILE, tilesT = (nT + CC_TILE - 1u) / CC_TILE;
	const uint64_t nslots = simp_table_size(nV), ntri = a->drop_duplicates ? simp_table_size(nT) : 0u;
	if ((rc = meas_room(&s->d_ref, &s->ref_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_slot, &s->slot_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_rep, &s->rep_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_keep, &s->keep_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_map, &s->map_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_surv, &s->surv_cap, nT))) return rc;
	if ((rc = meas_room(&s->d_bsum, &s->bsum_cap, tilesV + tilesT))) return rc;
	if ((s->slots_cap < nslots || !s->d_slots) && (rc = dev_room("cluster table", &s->d_slots, &s->slots_cap, nslots))) return rc;  // (powers of two as they are: no slack)
	if (ntri && (s->tri_cap < ntri || !s->d_tri) && (rc = dev_room("image table", &s->d_tri, &s->tri_cap, ntri))) return rc;
	uint32_t *bsumV = s->d_bsum, *bsumT = s->d_bsum + tilesV;
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
	HIP_TRY(hipMemsetAsync(s->d_keep, 0, nV, c->stream));
	if (ntri) HIP_TRY(hipMemsetAsync(s->d_tri, 0xFF, ntri * sizeof(uint32_t), c->stream));
	hipLaunchKernelGGL(k_simp_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, s->d_slots, nslots);
	hipLaunchKernelGGL(k_simp_ref, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_ref, s->d_out);
	hipLaunchKernelGGL((k_simp_cluster<real_t>), dim3(gridC), dim3(256), 0, c->stream, V, s->d_ref, (uint64_t)nV, chunkC, L, mean, s->d_slots, nslots - 1u, s->d_slot,
	                   s->d_out);
	hipLaunchKernelGGL(k_simp_reps, dim3(gridV), dim3(256), 0, c->stream, s->d_slots, s->d_slot, (uint64_t)nV, s->d_rep, s->d_out);
	if (drop) hipLaunchKernelGGL(k_simp_tri_insert, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_rep, s->d_tri, ntri - 1u, s->d_out);
	hipLaunchKernelGGL(k_simp_tri_keep, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_rep, s->d_tri, ntri ? ntri - 1u : 0u, drop, s->d_surv,
	                   s->d_keep, s->d_out);
	hipLaunchKernelGGL(k_simp_tile_count, dim3((uint32_t)tilesV), dim3(256), 0, c->stream, s->d_keep, (uint64_t)nV, bsumV);
	hipLaunchKernelGGL(k_filt_scan_top, dim3(1), dim3(256), 0, c->stream, bsumV, tilesV, &s->d_out->nV_out);
	hipLaunchKernelGGL(k_filt_new, dim3((uint32_t)tilesV), dim3(256), 0, c->stream, s->d_keep, bsumV, (uint64_t)nV, s->d_map);
	hipLaunchKernelGGL(k_simp_tile_count, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, s->d_surv, (uint64_t)nT, bsumT);
	hipLaunchKernelGGL(k_filt_scan_top, dim3(1), dim3(256), 0, c->stream, bsumT, tilesT, &s->d_out->nT_out);
	// the copies: they compare the totals with the capacities on the device, so that the host waits once before the normals
	hipLaunchKernelGGL((k_simp_rows<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, (const uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr),
	                   (const uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr), s->d_rep, s->d_slot, s->d_slots, s->d_map, (uint64_t)nV, L, mean, s->d_out, capV, capT,
	                   (real_t *)a->oV, (uint32_t *)(a->n_attr > 0u ? a->oAttr[0] : nullptr), (uint32_t *)(a->n_attr > 1u ? a->oAttr[1] : nullptr), (uint32_t *)a->oMap);
	hipLaunchKernelGGL(k_simp_tris, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, s->d_rep, s->d_surv, s->d_map, bsumT, s->d_out, capV, capT,
	                   (uint32_t *)a->oT);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, sizeof(SimpOut), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if ((rc = prop_check(c))) return rc;
	const SimpOut h = *s->h_out;
	simp_fill(a, h);
	if (h.full) { set_err("%llu keys or images found no slot in the tables", h.full); return MC33HIP_ERUNTIME; }
	if (h.nV_out > capV || h.nT_out > capT) {
		set_err("the simplified mesh needs %llu rows of V and %llu of T, the caller's arrays have %llu and %llu", h.nV_out, h.nT_out, (unsigned long long)capV,
		        (unsigned long long)capT);
		return MC33HIP_ECAPACITY;
	}
	// the normals of the output, by the passes of mc33hip_vertex_normals (oT names no vertex outside oV)
	if (a->oN && h.nV_out) {
		if ((rc = smooth_state(c))) return rc;
		SmoothState *sm = c->meas->smooth;
		sm->timers.adjacency = sm->timers.normals = false;
		sm->timers.passes = 0u;
		if ((rc = sm_room(c, h.nV_out, h.nT_out, false, 0u))) return rc;
		HIP_TRY(hipMemsetAsync(sm->d_out, 0, sizeof(SmOut), c->stream));
		if ((rc = sm_normals(c, (const real_t *)a->oV, (const uint32_t *)a->oT, h.nT_out, h.nV_out, a->oN, false))) return rc;
		if ((rc = sm_fetch(c))) return rc;
	}
	return meas_bad(h.bad, nV);
}
