// mc33_section.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h, on the union-find and the
// block sums of mc33_measure.hip.h and on the class, table and new-row functions of mc33_clip.hip.h; not a header to include
// elsewhere): a FINISHED mesh in device memory met by one plane - the contour where the plane crosses the surface as points and
// directed segments, its length and the area it encloses - so that a few thousand points cross the link instead of the mesh
// (include/mc33_hip.h: mc33hip_section_surface, mc33hip_section_contours, mc33hip_section_ladder).  DESIGN.md 20.
//
// The definition is in include/mc33_hip.h; tests/section_oracle.py restates it in numpy, operation for operation.  The section is
// the boundary mc33hip_clip_surface opens: classes, cut edges, owners and ranks are clip's - k_clip_class, k_clip_tri and
// k_clip_own run unchanged over clip's own scratch (ClipState) - and a cut point is clip_new_row's row without normals.
// The passes behind those three: k_section_tri, a lane per triangle, repeats the walk, finds the two on-plane entries of the
// polygon, drops the segment whose ends are one point and flags the ON vertices a kept segment names; tile scans over those flags,
// the owned sides and the kept segments; k_section_rows moves the ON rows and writes oPointMap; k_section_new, the owner's lane,
// writes the cut points at on_points + rank and leaves the rank in the slot; k_section_init clears a word of degree, label, next
// and open flag per point; k_section_emit repeats the walk, writes the segment at its scanned place and - integer atomics only -
// counts the starts and ends of its two points, lowers next[a] to b and unites a and b; k_section_points, a lane per point,
// flattens the label and takes the counts over the points; k_section_count the contours; k_section_sums and k_section_finish the
// doubles in the fixed order of k_measure_triangles / k_measure_finish.  Nothing a block wrote with plain stores is read by another
// block of the same kernel: degree, next and label words are touched only by atomics in k_section_emit, their readers are later
// kernels.  k_section_ladder: many parallel planes in one pass over T, no table (every use of a cut edge computes the same point).

struct SectionOut {         // what a call brings to the host (device copy and pinned twin)
	unsigned long long onp, cutv, nS, degenerate, nonfinite, isolated, open_ends, branch, contours, closed;
	unsigned long long bad, cut, full;      // of clip's passes (ClipOut), copied by k_section_finish
	unsigned long long pad_;
	double sum[4];          // length, area vector
};

struct SectionState {       // scratch of these passes besides clip's (classes, triangle bytes, table) and the shared keep, map and tile sums
	SectionOut *d_out, *h_out;
	uint8_t *d_on;          // [nV] 1: an ON vertex a kept segment names
	uint64_t on_cap;
	uint8_t *d_seg;         // [nT] 1: the triangle yields a kept segment
	uint64_t seg_cap;
	unsigned long long *d_deg;  // [points] segments that start at the point | segments that end there << 32
	uint64_t deg_cap;
	uint32_t *d_label;      // [points] the union-find over the points
	uint64_t label_cap;
	uint32_t *d_next;       // [points] the smallest end of the segments that start at the point
	uint64_t next_cap;
	uint8_t *d_open;        // [points] 1: the set of this root has a point that does not start one and end one segment
	uint64_t open_cap;
	double *d_part;         // [rows][4] block partials of k_section_sums
	uint64_t part_cap;
	unsigned long long *d_lad;  // ladder: [n] segments, behind them [n][4] doubles
	uint64_t lad_cap;
	mc33hip_contour *d_table;   // the contour table (its flags, ranks and degrees live in d_open, d_next and d_deg)
	uint64_t table_cap;
};

// the id of an on-plane entry: v << 32 | v for the ON vertex v, lo << 32 | hi (lo < hi) for a cut edge - never equal
__device__ __forceinline__ unsigned long long section_vertex_id(uint32_t v) { return ((unsigned long long)v << 32) | v; }
__device__ __forceinline__ bool section_is_vertex(unsigned long long id) { return (uint32_t)(id >> 32) == (uint32_t)id; }

// The walk of a valid triangle with an IN corner (classes a0 .. a2, cut sides `cuts`): the on-plane entries of its polygon.  True
// with a -> b, in the polygon's cyclic order, when there are two; they are neighbours there.
__device__ __forceinline__ bool section_walk(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t cuts,
                                             unsigned long long *a, unsigned long long *b) {
	unsigned long long f = 0ull, g = 0ull;
	uint32_t pf = 0u, pg = 0u, n = 0u, pos = 0u;
#pragma unroll
	for (uint32_t e = 0; e < 3u; e++) {
		const uint32_t p = e == 0u ? t0 : e == 1u ? t1 : t2, q = e == 0u ? t1 : e == 1u ? t2 : t0, ap = e == 0u ? a0 : e == 1u ? a1 : a2;
		if (ap != CLIP_OUT) {
			if (ap == CLIP_ON) {
				if (n == 0u) { f = section_vertex_id(p); pf = pos; } else { g = section_vertex_id(p); pg = pos; }
				n++;
			}
			pos++;
		}
		if ((cuts >> e) & 1u) {
			if (n == 0u) { f = clip_key(p, q); pf = pos; } else { g = clip_key(p, q); pg = pos; }
			n++;
			pos++;
		}
	}
	if (n != 2u) return false;
	const bool fwd = pg == pf + 1u;  // (otherwise they are the last and the first entry)
	*a = fwd ? f : g;
	*b = fwd ? g : f;
	return true;
}

// a lane per triangle: the byte of the kept segments, the flags of the ON vertices they name, the dropped segments
__global__ __launch_bounds__(256) void k_section_tri(const uint32_t *__restrict__ T, uint64_t nT, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ info,
                                                     uint8_t *__restrict__ on, uint8_t *__restrict__ seg, SectionOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	uint32_t degenerate = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t word = info[i];
		uint32_t kept = 0u;
		if (word & 3u) {  // (a triangle with outputs is valid and has an IN corner)
			const uint32_t *t = T + i * 3u;
			const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
			unsigned long long a, b;
			if (section_walk(t0, t1, t2, cls[t0] & 3u, cls[t1] & 3u, cls[t2] & 3u, (word >> 2) & 7u, &a, &b)) {
				if (a == b) degenerate++;
				else {
					kept = 1u;
					if (section_is_vertex(a)) on[(uint32_t)a] = 1;  // (every racing store writes the same 1)
					if (section_is_vertex(b)) on[(uint32_t)b] = 1;
				}
			}
		}
		seg[i] = (uint8_t)kept;
	}
	degenerate = block_sum_u32_256(degenerate, sh);
	if (threadIdx.x == 0u && degenerate) atomicAdd(&out->degenerate, (unsigned long long)degenerate);
}

__device__ __forceinline__ bool section_fits(const SectionOut *__restrict__ out, uint64_t capP, uint64_t capS) {
	return out->onp + out->cutv <= capP && out->nS <= capS;
}

// oPointMap for every vertex; the rows and attribute words of the ON points to their places; the vertices whose s is not finite
template <typename R>
__global__ __launch_bounds__(256) void k_section_rows(const R *__restrict__ V, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                                      const uint32_t *__restrict__ map, const uint8_t *__restrict__ nf, uint64_t nV, SectionOut *__restrict__ out,
                                                      uint64_t capP, uint64_t capS, R *__restrict__ oP, uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1,
                                                      uint32_t *__restrict__ oMap) {
	__shared__ uint32_t sh[4];
	const bool fits = section_fits(out, capP, capS);  // (the totals are those of earlier kernels; this one adds to another word)
	uint32_t nonf = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		nonf += nf[v] ? 1u : 0u;
		if (!fits) continue;
		const uint32_t m = map[v];
		if (oMap) oMap[v] = m;
		if (m == MESH_NONE) continue;
		mesh_copy_row(V, (const float *)nullptr, v, oP, (float *)nullptr, m);
		if (A0) oA0[m] = A0[v];
		if (A1) oA1[m] = A1[v];
	}
	nonf = block_sum_u32_256(nonf, sh);
	if (threadIdx.x == 0u && nonf) atomicAdd(&out->nonfinite, (unsigned long long)nonf);
}

// the owned sides of a tile of triangles: clip's new rows, without normals, behind the ON points; the rank into the slot
template <typename R>
__global__ __launch_bounds__(256) void k_section_new(const R *__restrict__ V, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1, uint32_t lerp0,
                                                     uint32_t lerp1, ClipPlane P, const uint32_t *__restrict__ T, uint64_t nT, const uint8_t *__restrict__ info,
                                                     const uint32_t *__restrict__ bsum, ClipSlot *__restrict__ slots, uint64_t mask,
                                                     const SectionOut *__restrict__ out, uint64_t capP, uint64_t capS, R *__restrict__ oP,
                                                     uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1) {
	__shared__ uint32_t sh[256];
	if (!section_fits(out, capP, capS)) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	const uint64_t onp = out->onp;
	const uint64_t i0 = mesh_tile_e0();
	uint32_t f[4];
	const uint32_t own = mesh_tile_load<ClipOwned>(info, nT, f);
	uint64_t r = mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		f[k] >>= 5;  // (the owned sides)
		if (!f[k]) continue;
		const uint32_t *t = T + (i0 + k) * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
#pragma unroll
		for (uint32_t e = 0; e < 3u; e++) {
			if (!((f[k] >> e) & 1u)) continue;
			const uint32_t p = e == 0u ? t0 : e == 1u ? t1 : t2, q = e == 0u ? t1 : e == 1u ? t2 : t0;
			clip_new_row(V, (const float *)nullptr, A0, A1, lerp0, lerp1, P, p, q, onp + r, oP, (float *)nullptr, oA0, oA1);
			const uint64_t s = mesh_find(slots, mask, clip_key(p, q));
			if (s != MESH_NOSLOT) slots[s].owner = r;  // (the owner found its slot in k_clip_own)
			r++;
		}
	}
}

// a word of degree, label, next and open flag per point
__global__ __launch_bounds__(256) void k_section_init(const SectionOut *__restrict__ out, uint64_t capP, uint64_t capS, unsigned long long *__restrict__ deg,
                                                      uint32_t *__restrict__ label, uint32_t *__restrict__ next, uint8_t *__restrict__ open) {
	if (!section_fits(out, capP, capS)) return;
	const uint64_t nP = out->onp + out->cutv;
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nP; p += (uint64_t)gridDim.x * 256u) {
		deg[p] = 0ull; label[p] = (uint32_t)p; next[p] = MESH_NONE; open[p] = 0;
	}
}

// the point of an on-plane entry: an ON vertex through the map, a cut edge through its rank in the table
__device__ __forceinline__ uint32_t section_point(unsigned long long id, const uint32_t *__restrict__ map, const ClipSlot *__restrict__ slots, uint64_t mask, uint32_t onp) {
	if (section_is_vertex(id)) return map[(uint32_t)id];
	const uint64_t s = mesh_find(slots, mask, id);
	return onp + (s != MESH_NOSLOT ? (uint32_t)slots[s].owner : 0u);
}

// the walk again: the segment of a kept triangle at the tile's place in oS; starts, ends, next and the union by atomics
__global__ __launch_bounds__(256) void k_section_emit(const uint32_t *__restrict__ T, uint64_t nT, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ info,
                                                      const uint8_t *__restrict__ seg, const uint32_t *__restrict__ map, const ClipSlot *__restrict__ slots, uint64_t mask,
                                                      const uint32_t *__restrict__ bsum, const SectionOut *__restrict__ out, uint64_t capP, uint64_t capS,
                                                      uint32_t *__restrict__ oS, unsigned long long *deg, uint32_t *label, uint32_t *next) {
	__shared__ uint32_t sh[256];
	if (!section_fits(out, capP, capS)) return;
	const uint32_t onp = (uint32_t)out->onp;
	const uint64_t i0 = mesh_tile_e0();
	uint32_t f[4];
	const uint32_t own = mesh_tile_load<MeshFlag>(seg, nT, f);
	uint64_t r = mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		if (!f[k]) continue;
		const uint64_t i = i0 + k;
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		unsigned long long ia, ib;
		if (!section_walk(t0, t1, t2, cls[t0] & 3u, cls[t1] & 3u, cls[t2] & 3u, ((uint32_t)info[i] >> 2) & 7u, &ia, &ib)) continue;  // (k_section_tri found it)
		const uint32_t a = section_point(ia, map, slots, mask, onp), b = section_point(ib, map, slots, mask, onp);
		oS[r * 2u] = a; oS[r * 2u + 1u] = b;
		r++;
		atomicAdd(&deg[a], 1ull);
		atomicAdd(&deg[b], 1ull << 32);
		atomicMin(&next[a], b);
		cc_unite(label, a, b);
	}
}

// a lane per point: its label flattened (no union runs beside this), its next kept only where one segment starts, the counts
__global__ __launch_bounds__(256) void k_section_points(SectionOut *__restrict__ out, uint64_t capP, uint64_t capS, const unsigned long long *__restrict__ deg,
                                                        uint32_t *label, uint32_t *__restrict__ next, uint8_t *__restrict__ open, uint32_t *__restrict__ oNext) {
	__shared__ uint32_t sh[4];
	if (!section_fits(out, capP, capS)) return;
	const uint64_t nP = out->onp + out->cutv;
	uint32_t isolated = 0u, ends = 0u, branch = 0u;
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nP; p += (uint64_t)gridDim.x * 256u) {
		uint32_t x = (uint32_t)p, up = __hip_atomic_load(label + x, MC33_RLX_AGENT);
		while (up != x) { x = up; up = __hip_atomic_load(label + x, MC33_RLX_AGENT); }
		__hip_atomic_store(label + p, x, MC33_RLX_AGENT);
		const unsigned long long d = deg[p];
		const uint32_t starts = (uint32_t)d, stops = (uint32_t)(d >> 32);
		if (!d) isolated++;
		if (starts != stops) ends++;
		if (starts > 1u || stops > 1u) branch++;
		if (d && (starts != 1u || stops != 1u)) open[x] = 1;  // (every racing store writes the same 1)
		const uint32_t nx = starts == 1u ? next[p] : MESH_NONE;
		if (oNext) oNext[p] = nx;
	}
	isolated = block_sum_u32_256(isolated, sh);
	ends = block_sum_u32_256(ends, sh);
	branch = block_sum_u32_256(branch, sh);
	if (threadIdx.x == 0u) {
		if (isolated) atomicAdd(&out->isolated, (unsigned long long)isolated);
		if (ends) atomicAdd(&out->open_ends, (unsigned long long)ends);
		if (branch) atomicAdd(&out->branch, (unsigned long long)branch);
	}
}

// the contours: roots with a segment; closed where no point of the set raised the root's flag.  oLabel from the flattened words.
__global__ __launch_bounds__(256) void k_section_count(SectionOut *__restrict__ out, uint64_t capP, uint64_t capS, const unsigned long long *__restrict__ deg,
                                                       const uint32_t *__restrict__ label, const uint8_t *__restrict__ open, uint32_t *__restrict__ oLabel) {
	__shared__ uint32_t sh[4];
	if (!section_fits(out, capP, capS)) return;
	const uint64_t nP = out->onp + out->cutv;
	uint32_t contours = 0u, closed = 0u;
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nP; p += (uint64_t)gridDim.x * 256u) {
		const uint32_t r = label[p];
		if (oLabel) oLabel[p] = r;
		if (r == (uint32_t)p && deg[p]) {
			contours++;
			if (!open[p]) closed++;
		}
	}
	contours = block_sum_u32_256(contours, sh);
	closed = block_sum_u32_256(closed, sh);
	if (threadIdx.x == 0u) {
		if (contours) atomicAdd(&out->contours, (unsigned long long)contours);
		if (closed) atomicAdd(&out->closed, (unsigned long long)closed);
	}
}

struct SegTerms { double len, gx, gy, gz; };

// the terms of one segment p -> q, both already relative to the reference point
__device__ __forceinline__ SegTerms seg_terms(double px, double py, double pz, double qx, double qy, double qz) {
	const double dx = qx - px, dy = qy - py, dz = qz - pz;
	SegTerms t;
	t.len = sqrt((dx * dx + dy * dy) + dz * dz);
	t.gx = 0.5 * (py * qz - pz * qy);
	t.gy = 0.5 * (pz * qx - px * qz);
	t.gz = 0.5 * (px * qy - py * qx);
	return t;
}

// Every block a contiguous piece of oS (a multiple of 256 segments, from the device's count and the launch geometry), a lane a
// segment per step; a row of partials per block, as k_measure_triangles leaves them.
template <typename R>
__global__ __launch_bounds__(256) void k_section_sums(const R *__restrict__ oP, const uint32_t *__restrict__ oS, const SectionOut *__restrict__ out, uint64_t capP,
                                                      uint64_t capS, double c0, double c1, double c2, double *__restrict__ part) {
	__shared__ double sh[4];
	const uint64_t nS = section_fits(out, capP, capS) ? out->nS : 0u;
	const uint64_t chunk = ((nS + gridDim.x - 1u) / gridDim.x + 255u) / 256u * 256u;
	const uint64_t beg = (uint64_t)blockIdx.x * chunk, end = beg + chunk < nS ? beg + chunk : nS;
	double sL = 0.0, sX = 0.0, sY = 0.0, sZ = 0.0;
	for (uint64_t i = beg + threadIdx.x; i < end; i += 256u) {
		const R *p = oP + (uint64_t)oS[i * 2u] * 3u, *q = oP + (uint64_t)oS[i * 2u + 1u] * 3u;
		const SegTerms x = seg_terms((double)p[0] - c0, (double)p[1] - c1, (double)p[2] - c2, (double)q[0] - c0, (double)q[1] - c1, (double)q[2] - c2);
		sL += x.len; sX += x.gx; sY += x.gy; sZ += x.gz;
	}
	double *row = part + (uint64_t)blockIdx.x * 4u;
	double r;
	r = block_sum_256(sL, sh); if (threadIdx.x == 0u) row[0] = r;
	r = block_sum_256(sX, sh); if (threadIdx.x == 0u) row[1] = r;
	r = block_sum_256(sY, sh); if (threadIdx.x == 0u) row[2] = r;
	r = block_sum_256(sZ, sh); if (threadIdx.x == 0u) row[3] = r;
}

// One block: the partial rows in index order - lane t adds rows t, t + 256, ..., then a tree over the lanes, as k_measure_finish
// does - and the three counts of clip's passes into this part's block.
__global__ __launch_bounds__(256) void k_section_finish(const double *__restrict__ part, uint32_t nrows, const ClipOut *__restrict__ clip, SectionOut *__restrict__ out) {
	__shared__ double sh[4][256];
	const uint32_t t = threadIdx.x;
	double s[4] = {0.0, 0.0, 0.0, 0.0};
	for (uint32_t r = t; r < nrows; r += 256u) {
#pragma unroll
		for (int k = 0; k < 4; k++) s[k] += part[(uint64_t)r * 4u + k];
	}
#pragma unroll
	for (int k = 0; k < 4; k++) sh[k][t] = s[k];
	__syncthreads();
	for (uint32_t d = 128u; d >= 1u; d >>= 1) {
		if (t < d) {
#pragma unroll
			for (int k = 0; k < 4; k++) sh[k][t] += sh[k][t + d];
		}
		__syncthreads();
	}
	if (t < 4u) out->sum[t] = sh[t][0];
	if (t == 4u) { out->bad = clip->bad; out->cut = clip->cut; out->full = clip->full; }
}

// --- the contour table: a row per label set with a segment, from the oP, oS and oLabel of a section -----------------------------
// A segment belongs to the label of its start.  A segment that names a point >= nP, or whose start has a label >= nP, is counted
// and left out, and is tested BEFORE anything is gathered through it.

// starts and ends per point, the flag of every root that owns a segment
__global__ __launch_bounds__(256) void k_section_table_degree(const uint32_t *__restrict__ S, uint64_t nS, uint64_t nP, const uint32_t *__restrict__ label,
                                                              unsigned long long *deg, uint8_t *__restrict__ flags, unsigned long long *__restrict__ bad_out) {
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nS; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t a = S[i * 2u], b = S[i * 2u + 1u];
		if (a >= nP || b >= nP) { bad++; continue; }
		const uint32_t r = label[a];
		if (r >= nP) { bad++; continue; }
		atomicAdd(&deg[a], 1ull);
		atomicAdd(&deg[b], 1ull << 32);
		flags[r] = 1;  // (every racing store writes the same 1)
	}
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// a lane per point a segment names: 1, its open end, its branching and whether it breaks the loop into the row of its label
// (`closed` counts the points that do not start one and end one segment; the host turns the count into the flag)
__global__ __launch_bounds__(256) void k_section_table_points(const unsigned long long *__restrict__ deg, const uint32_t *__restrict__ label,
                                                              const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank, uint64_t nP,
                                                              mc33hip_contour *table) {
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nP; p += (uint64_t)gridDim.x * 256u) {
		const unsigned long long d = deg[p];
		if (!d) continue;
		const uint32_t r = label[p];
		if (r >= nP || !flags[r]) continue;  // (a label array that is not the section's own)
		mc33hip_contour *row = table + rank[r];
		const uint32_t starts = (uint32_t)d, stops = (uint32_t)(d >> 32);
		atomicAdd(&row->points, 1u);
		if (starts != stops) atomicAdd(&row->open_ends, 1u);
		if (starts > 1u || stops > 1u) atomicAdd(&row->branch_points, 1u);
		if (starts != 1u || stops != 1u) atomicAdd(&row->closed, 1);
	}
}

// the root of every row (a lane per flagged root: one plain store per word), and 1, length and area of every segment by atomics
template <typename R>
__global__ __launch_bounds__(256) void k_section_table_segments(const R *__restrict__ P, uint64_t nP, const uint32_t *__restrict__ S, uint64_t nS,
                                                                const uint32_t *__restrict__ label, const uint8_t *__restrict__ flags,
                                                                const uint32_t *__restrict__ rank, double c0, double c1, double c2, double na, double nb,
                                                                double nc, double norm, mc33hip_contour *table) {
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nS; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t a = S[i * 2u], b = S[i * 2u + 1u];
		if (a >= nP || b >= nP) continue;  // (counted by k_section_table_degree)
		const uint32_t r = label[a];
		if (r >= nP) continue;
		mc33hip_contour *row = table + rank[r];
		const R *p = P + (uint64_t)a * 3u, *q = P + (uint64_t)b * 3u;
		const SegTerms x = seg_terms((double)p[0] - c0, (double)p[1] - c1, (double)p[2] - c2, (double)q[0] - c0, (double)q[1] - c1, (double)q[2] - c2);
		atomicAdd(&row->segments, 1u);
		unsafeAtomicAdd(&row->length, x.len);
		unsafeAtomicAdd(&row->area, ((x.gx * na + x.gy * nb) + x.gz * nc) / norm);
	}
}
__global__ __launch_bounds__(256) void k_section_table_roots(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ rank, uint64_t nP, mc33hip_contour *table) {
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nP; p += (uint64_t)gridDim.x * 256u)
		if (flags[p]) table[rank[p]].root = (uint32_t)p;
}

// --- many parallel planes in one pass over T --------------------------------------------------------------------------------
// s_k[v] = base[v] + w_k with base = (x a + y b) + z c: the classes of plane k are those of the single-plane call bit for bit.
// base + w > 0 exactly when base > -w (IEEE addition is monotone and x + w == 0 only for x == -w), so the planes for which a
// triangle has an IN corner and one that is not IN are found from the largest and the smallest base of its corners.

constexpr uint32_t SECTION_LADDER_MAX = 255u;
struct LadderArgs { double a, b, c; uint32_t n; double w[SECTION_LADDER_MAX]; };

// the row of a point of plane k: the ON vertex's own, or clip's cut point of {lo, hi} (from the smaller index, whoever computes it)
template <typename R>
__device__ __forceinline__ void ladder_point(const R *__restrict__ V, unsigned long long id, const double base[3], const uint32_t tv[3], double w, double c0, double c1,
                                             double c2, double *x, double *y, double *z) {
	if (section_is_vertex(id)) {
		const R *r = V + (uint64_t)(uint32_t)id * 3u;
		*x = (double)r[0] - c0; *y = (double)r[1] - c1; *z = (double)r[2] - c2;
		return;
	}
	const uint32_t lo = (uint32_t)(id >> 32), hi = (uint32_t)id;
	double blo = 0.0, bhi = 0.0;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		if (tv[k] == lo) blo = base[k];
		if (tv[k] == hi) bhi = base[k];
	}
	const double slo = blo + w, shi = bhi + w;
	const bool copy = !clip_finite(slo) || !clip_finite(shi);
	const uint32_t in = slo > 0.0 ? lo : hi;
	const double t = slo / (slo - shi);
	const R *a = V + (uint64_t)lo * 3u, *b = V + (uint64_t)hi * 3u, *e = V + (uint64_t)in * 3u;
	double o[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const double u = (double)a[k], v = (double)b[k];
		o[k] = copy ? (double)e[k] : (double)(R)(u + t * (v - u));
	}
	*x = o[0] - c0; *y = o[1] - c1; *z = o[2] - c2;
}

template <typename R>
__global__ __launch_bounds__(256) void k_section_ladder(const R *__restrict__ V, uint64_t nV, const uint32_t *__restrict__ T, uint64_t nT, LadderArgs L, double c0,
                                                        double c1, double c2, unsigned long long *__restrict__ count, double *__restrict__ sums,
                                                        unsigned long long *__restrict__ bad_out) {
	__shared__ uint32_t sc[SECTION_LADDER_MAX + 1u];
	__shared__ double sd[SECTION_LADDER_MAX + 1u][4];
	for (uint32_t k = threadIdx.x; k < L.n; k += 256u) { sc[k] = 0u; sd[k][0] = sd[k][1] = sd[k][2] = sd[k][3] = 0.0; }
	__syncthreads();
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t tv[3] = {t[0], t[1], t[2]};
		if (tv[0] >= nV || tv[1] >= nV || tv[2] >= nV) { bad++; continue; }
		double base[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const R *p = V + (uint64_t)tv[k] * 3u;
			base[k] = ((double)p[0] * L.a + (double)p[1] * L.b) + (double)p[2] * L.c;
		}
		// the planes with an IN corner: w > -max; with a corner that is not IN: !(min + w > 0), and a NaN corner is never IN
		double hi = -__builtin_huge_val(), lo = __builtin_huge_val();
		bool nan = false;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			if (base[k] != base[k]) nan = true;
			else { hi = base[k] > hi ? base[k] : hi; lo = base[k] < lo ? base[k] : lo; }
		}
		for (uint32_t k = 0; k < L.n; k++) {
			const double w = L.w[k];
			if (!(hi + w > 0.0)) continue;          // no IN corner (yet: the offsets ascend)
			if (!nan && lo + w > 0.0) break;        // every corner IN, and for every later plane
			uint32_t a[3];
#pragma unroll
			for (int j = 0; j < 3; j++) {
				const double s = base[j] + w;
				a[j] = s > 0.0 ? CLIP_IN : s == 0.0 ? CLIP_ON : CLIP_OUT;
			}
			unsigned long long ia, ib;
			if (!section_walk(tv[0], tv[1], tv[2], a[0], a[1], a[2], clip_cuts(a[0], a[1], a[2]), &ia, &ib) || ia == ib) continue;
			double px, py, pz, qx, qy, qz;
			ladder_point(V, ia, base, tv, w, c0, c1, c2, &px, &py, &pz);
			ladder_point(V, ib, base, tv, w, c0, c1, c2, &qx, &qy, &qz);
			const SegTerms x = seg_terms(px, py, pz, qx, qy, qz);
			atomicAdd(&sc[k], 1u);
			atomicAdd(&sd[k][0], x.len); atomicAdd(&sd[k][1], x.gx); atomicAdd(&sd[k][2], x.gy); atomicAdd(&sd[k][3], x.gz);
		}
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < L.n; k += 256u) {
		if (!sc[k]) continue;
		atomicAdd(&count[k], (unsigned long long)sc[k]);
#pragma unroll
		for (int j = 0; j < 4; j++) unsafeAtomicAdd(&sums[(uint64_t)k * 4u + j], sd[k][j]);
	}
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void section_release(void *state) {
	SectionState *s = (SectionState *)state;
	dev_release(&s->d_on); dev_release(&s->d_seg); dev_release(&s->d_deg); dev_release(&s->d_label); dev_release(&s->d_next); dev_release(&s->d_open);
	dev_release(&s->d_part); dev_release(&s->d_lad); dev_release(&s->d_table);
}
static int section_state(mc33hip_ctx *c, SectionState **s) {
	const int rc = meas_state(c);
	return rc ? rc : mesh_op_state(&c->meas->mesh, section_release, s);
}

static bool section_plane_ok(const double *n, int count, const char *what) {
	for (int k = 0; k < count; k++)
		if (!clip_finite(n[k])) { set_err("%s[%d] must be finite", what, k); return false; }
	if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) { set_err("the plane has no normal: a, b and c are all zero"); return false; }
	return true;
}

static double section_area(const double G[3], const double n[3]) {
	return ((G[0] * n[0] + G[1] * n[1]) + G[2] * n[2]) / sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}

extern "C" int mc33hip_section_surface(mc33hip_ctx *c, mc33hip_section *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nP_out = a->nS_out = a->on_points = a->cut_points = a->isolated_points = a->degenerate_segments = a->crossing_triangles = a->invalid_triangles =
	    a->nonfinite_vertices = a->contours = a->closed_contours = a->open_ends = a->branch_points = 0;
	a->length = a->area = a->area_vector[0] = a->area_vector[1] = a->area_vector[2] = 0.0;
	meas_origin(c, a->origin);
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_counts_ok(a->n_attr, nV, nT)) return MC33HIP_EINVAL;
	for (unsigned k = 0; k < a->n_attr; k++)
		if (a->attr_mode[k] != MC33HIP_CLIP_COPY && a->attr_mode[k] != MC33HIP_CLIP_LERP_F32) {
			set_err("attr_mode[%u] = %d is neither MC33HIP_CLIP_COPY nor MC33HIP_CLIP_LERP_F32", k, a->attr_mode[k]);
			return MC33HIP_EINVAL;
		}
	if (!section_plane_ok(a->plane, 4, "plane")) return MC33HIP_EINVAL;
	const uint64_t capP = mesh_cap(a->capP), capS = mesh_cap(a->capS);
	if (!mesh_pointers_ok((nV && !a->V) || (nT && !a->T) || (capP && !a->oP) || (capS && !a->oS), a->n_attr, a->attr, a->oAttr, nV, capP)) return MC33HIP_EINVAL;
	// the call is not in place: no output may share a byte with an input or with another output
	const MeshRange in[4] = {{a->V, nV * 3u * sizeof(real_t)}, {a->T, nT * 12u}, {a->n_attr > 0u ? a->attr[0] : nullptr, nV * 4u},
	                         {a->n_attr > 1u ? a->attr[1] : nullptr, nV * 4u}};
	const MeshRange out[7] = {{a->oP, capP * 3u * sizeof(real_t)}, {a->oS, capS * 8u}, {a->oLabel, capP * 4u}, {a->oNext, capP * 4u}, {a->oPointMap, nV * 4u},
	                          {a->n_attr > 0u ? a->oAttr[0] : nullptr, capP * 4u}, {a->n_attr > 1u ? a->oAttr[1] : nullptr, capP * 4u}};
	if (!mesh_ranges_ok(in, 4, out, 7, true, "section")) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	ClipState *cs;
	SectionState *s;
	if ((rc = clip_state(c, &cs))) return rc;
	if ((rc = section_state(c, &s))) return rc;
	if (!nT || !nV) {  // every count is 0
		if ((rc = mesh_empty(c, a->oPointMap, nV))) return rc;
		a->invalid_triangles = nT;
		return mesh_bad(nT, nV);
	}
	MeshHost &h = c->meas->mesh;
	const uint64_t tilesV = (nV + MESH_TILE - 1u) / MESH_TILE, tilesT = (nT + MESH_TILE - 1u) / MESH_TILE;
	const uint64_t nslots = mesh_table_size(nT, 4u, 1ull << 40);
	const uint64_t points = std::min<uint64_t>(capP, 2u * nT);  // (a triangle has at most two on-plane entries; with less room nothing is written)
	const uint32_t gridV = meas_grid(c, nV, 16u), gridT = meas_grid(c, nT, 16u), gridH = meas_grid(c, nT, 8u), gridP = meas_grid(c, std::max<uint64_t>(points, 1u), 16u);
	const uint32_t gridS = std::min(meas_grid(c, nT, 16u), 256u);  // (of the input alone: the order of the sums does not depend on the capacities; a section is short)
	if ((rc = meas_scratch(c, nV, tilesV + 2u * tilesT))) return rc;
	if ((rc = meas_room(&cs->d_cls, &cs->cls_cap, nV))) return rc;
	if ((rc = meas_room(&cs->d_nf, &cs->nf_cap, nV))) return rc;
	if ((rc = meas_room(&cs->d_info, &cs->info_cap, nT))) return rc;
	if ((cs->slots_cap < nslots || !cs->d_slots) && (rc = dev_room("cut edge table", &cs->d_slots, &cs->slots_cap, nslots))) return rc;
	if ((rc = meas_room(&s->d_on, &s->on_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_seg, &s->seg_cap, nT))) return rc;
	if ((rc = meas_room(&s->d_deg, &s->deg_cap, points))) return rc;
	if ((rc = meas_room(&s->d_label, &s->label_cap, points))) return rc;
	if ((rc = meas_room(&s->d_next, &s->next_cap, points))) return rc;
	if ((rc = meas_room(&s->d_open, &s->open_cap, points))) return rc;
	if ((rc = meas_room(&s->d_part, &s->part_cap, (uint64_t)gridS * 4u))) return rc;
	uint32_t *bsumV = h.d_bsum, *bsumO = h.d_bsum + tilesV, *bsumS = bsumO + tilesT;
	const real_t *V = (const real_t *)a->V;
	const uint32_t *T = (const uint32_t *)a->T;
	const uint32_t *A0 = (const uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr), *A1 = (const uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr);
	uint32_t *oA0 = (uint32_t *)(a->n_attr > 0u ? a->oAttr[0] : nullptr), *oA1 = (uint32_t *)(a->n_attr > 1u ? a->oAttr[1] : nullptr);
	const uint32_t lerp0 = a->n_attr > 0u && a->attr_mode[0] == MC33HIP_CLIP_LERP_F32 ? 1u : 0u, lerp1 = a->n_attr > 1u && a->attr_mode[1] == MC33HIP_CLIP_LERP_F32 ? 1u : 0u;
	ClipPlane P;
	P.a = a->plane[0]; P.b = a->plane[1]; P.c = a->plane[2]; P.w = a->plane[3];
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(SectionOut), c->stream));
	HIP_TRY(hipMemsetAsync(cs->d_out, 0, sizeof(ClipOut), c->stream));
	HIP_TRY(hipMemsetAsync(h.d_keep, 0, nV, c->stream));
	HIP_TRY(hipMemsetAsync(cs->d_nf, 0, nV, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_on, 0, nV, c->stream));
	// clip's passes as they stand: classes, the cut-edge table with its owners, the owned sides
	hipLaunchKernelGGL(k_mesh_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, (ulonglong2 *)cs->d_slots, nslots, ~0ull);
	hipLaunchKernelGGL((k_clip_class<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, (uint64_t)nV, P, cs->d_cls);
	hipLaunchKernelGGL(k_clip_tri, dim3(gridH), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, cs->d_cls, cs->d_slots, nslots - 1u, h.d_keep, cs->d_nf, cs->d_info,
	                   cs->d_out);
	hipLaunchKernelGGL(k_clip_own, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, cs->d_slots, nslots - 1u, cs->d_info, cs->d_out);
	hipLaunchKernelGGL(k_section_tri, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, cs->d_cls, cs->d_info, s->d_on, s->d_seg, s->d_out);
	// the three scans - ON flags (oPointMap), owned sides (k_section_new places), kept segments (k_section_emit places): their tile
	// sums, then ONE launch for the three single-block passes over them, which do not depend on each other
	hipLaunchKernelGGL((k_mesh_tile_sum<MeshFlag>), dim3((uint32_t)tilesV), dim3(256), 0, c->stream, (const uint8_t *)s->d_on, (uint64_t)nV, bsumV);
	hipLaunchKernelGGL((k_mesh_tile_sum<ClipOwned>), dim3((uint32_t)tilesT), dim3(256), 0, c->stream, (const uint8_t *)cs->d_info, (uint64_t)nT, bsumO);
	hipLaunchKernelGGL((k_mesh_tile_sum<MeshFlag>), dim3((uint32_t)tilesT), dim3(256), 0, c->stream, (const uint8_t *)s->d_seg, (uint64_t)nT, bsumS);
	hipLaunchKernelGGL(k_mesh_scan_top3, dim3(3), dim3(256), 0, c->stream, MeshTop{bsumV, tilesV, &s->d_out->onp}, MeshTop{bsumO, tilesT, &s->d_out->cutv},
	                   MeshTop{bsumS, tilesT, &s->d_out->nS});
	hipLaunchKernelGGL((k_mesh_place<MeshFlag, MESH_NEW>), dim3((uint32_t)tilesV), dim3(256), 0, c->stream, (const uint8_t *)s->d_on, (const uint32_t *)bsumV, (uint64_t)nV,
	                   h.d_map);
	// the writing passes: they compare the totals with the capacities on the device, so that the host waits once
	hipLaunchKernelGGL((k_section_rows<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, A0, A1, h.d_map, cs->d_nf, (uint64_t)nV, s->d_out, capP, capS, (real_t *)a->oP, oA0,
	                   oA1, (uint32_t *)a->oPointMap);
	hipLaunchKernelGGL((k_section_new<real_t>), dim3((uint32_t)tilesT), dim3(256), 0, c->stream, V, A0, A1, lerp0, lerp1, P, T, (uint64_t)nT, cs->d_info, bsumO, cs->d_slots,
	                   nslots - 1u, s->d_out, capP, capS, (real_t *)a->oP, oA0, oA1);
	hipLaunchKernelGGL(k_section_init, dim3(gridP), dim3(256), 0, c->stream, s->d_out, capP, capS, s->d_deg, s->d_label, s->d_next, s->d_open);
	hipLaunchKernelGGL(k_section_emit, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, cs->d_cls, cs->d_info, s->d_seg, h.d_map, cs->d_slots, nslots - 1u,
	                   bsumS, s->d_out, capP, capS, (uint32_t *)a->oS, s->d_deg, s->d_label, s->d_next);
	hipLaunchKernelGGL(k_section_points, dim3(gridP), dim3(256), 0, c->stream, s->d_out, capP, capS, s->d_deg, s->d_label, s->d_next, s->d_open, (uint32_t *)a->oNext);
	hipLaunchKernelGGL(k_section_count, dim3(gridP), dim3(256), 0, c->stream, s->d_out, capP, capS, s->d_deg, s->d_label, s->d_open, (uint32_t *)a->oLabel);
	hipLaunchKernelGGL((k_section_sums<real_t>), dim3(gridS), dim3(256), 0, c->stream, (const real_t *)a->oP, (const uint32_t *)a->oS, s->d_out, capP, capS, a->origin[0],
	                   a->origin[1], a->origin[2], s->d_part);
	hipLaunchKernelGGL(k_section_finish, dim3(1), dim3(256), 0, c->stream, s->d_part, gridS, cs->d_out, s->d_out);
	if ((rc = mesh_op_fetch(c, s))) return rc;
	const SectionOut o = *s->h_out;
	a->nP_out = o.onp + o.cutv; a->nS_out = o.nS; a->on_points = o.onp; a->cut_points = o.cutv; a->isolated_points = o.isolated;
	a->degenerate_segments = o.degenerate; a->crossing_triangles = o.cut; a->invalid_triangles = o.bad; a->nonfinite_vertices = o.nonfinite;
	a->contours = o.contours; a->closed_contours = o.closed; a->open_ends = o.open_ends; a->branch_points = o.branch;
	a->length = o.sum[0];
	for (int k = 0; k < 3; k++) a->area_vector[k] = o.sum[1 + k];
	a->area = section_area(a->area_vector, a->plane);
	if (o.full) { set_err("%llu cut sides found no slot in the table", o.full); return MC33HIP_ERUNTIME; }
	if (a->nP_out > capP || o.nS > capS) {
		set_err("the section needs %llu rows of points and %llu of segments, the caller's arrays have %llu and %llu", a->nP_out, o.nS, (unsigned long long)capP,
		        (unsigned long long)capS);
		return MC33HIP_ECAPACITY;
	}
	return mesh_bad(o.bad, nV);
}

extern "C" int mc33hip_section_contours(mc33hip_ctx *c, const void *dP, unsigned long long nP, const void *dS, unsigned long long nS, const unsigned *dLabel,
                                        const double plane[4], mc33hip_contour *host_table, unsigned long long capacity, unsigned long long *contours) {
	if (!c || !contours || !plane || (nP && (!dP || !dLabel)) || (nS && !dS) || (capacity && !host_table) || !mesh_sizes_ok(nP, nS)) return MC33HIP_EINVAL;
	if (!section_plane_ok(plane, 4, "plane")) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	SectionState *s;
	if ((rc = section_state(c, &s))) return rc;
	MeasureState *m = c->meas;
	*contours = 0;
	if (!nP || !nS) {  // no row; every segment of a mesh without points is invalid
		HIP_TRY(hipStreamSynchronize(c->stream));
		if ((rc = prop_check(c))) return rc;
		return nP ? MC33HIP_OK : mesh_bad(nS, nP);
	}
	// the section's own per-point scratch under other names: starts and ends, root flags, ranks
	const uint64_t tiles = (nP + MESH_TILE - 1u) / MESH_TILE;
	if ((rc = meas_room(&s->d_deg, &s->deg_cap, nP))) return rc;
	if ((rc = meas_room(&s->d_open, &s->open_cap, nP))) return rc;
	if ((rc = meas_room(&s->d_next, &s->next_cap, nP))) return rc;
	if ((rc = meas_room(&m->mesh.d_bsum, &m->mesh.bsum_cap, tiles))) return rc;
	uint8_t *flags = s->d_open;
	uint32_t *rank = s->d_next;
	const uint32_t gridP = meas_grid(c, nP, 16u), gridS = meas_grid(c, nS, 16u);
	if ((rc = meas_zero_counters(c))) return rc;
	HIP_TRY(hipMemsetAsync(s->d_deg, 0, nP * 8u, c->stream));
	HIP_TRY(hipMemsetAsync(flags, 0, nP, c->stream));
	hipLaunchKernelGGL(k_section_table_degree, dim3(gridS), dim3(256), 0, c->stream, (const uint32_t *)dS, (uint64_t)nS, (uint64_t)nP, dLabel, s->d_deg, flags, &m->d_out->bad);
	hipLaunchKernelGGL(k_cc_count, dim3((uint32_t)tiles), dim3(256), 0, c->stream, dLabel, flags, (uint64_t)nP, m->mesh.d_bsum, m->d_out);
	if ((rc = meas_fetch(c))) return rc;
	const unsigned long long bad = m->h_out->bad, rows = m->h_out->comps;
	*contours = rows;
	if (capacity < rows) { set_err("the contour table needs %llu rows, the caller's has %llu", rows, capacity); return MC33HIP_ECAPACITY; }
	if (!rows) return mesh_bad(bad, nP);
	if ((rc = meas_room(&s->d_table, &s->table_cap, rows))) return rc;
	HIP_TRY(hipMemsetAsync(s->d_table, 0, rows * sizeof(mc33hip_contour), c->stream));
	double o[3];
	meas_origin(c, o);
	const double norm = sqrt((plane[0] * plane[0] + plane[1] * plane[1]) + plane[2] * plane[2]);
	mesh_scan_sums<MeshFlag, MESH_RANK>(c, flags, nP, m->mesh.d_bsum, nullptr, rank);
	hipLaunchKernelGGL(k_section_table_roots, dim3(gridP), dim3(256), 0, c->stream, flags, rank, (uint64_t)nP, s->d_table);
	hipLaunchKernelGGL(k_section_table_points, dim3(gridP), dim3(256), 0, c->stream, s->d_deg, dLabel, flags, rank, (uint64_t)nP, s->d_table);
	hipLaunchKernelGGL((k_section_table_segments<real_t>), dim3(gridS), dim3(256), 0, c->stream, (const real_t *)dP, (uint64_t)nP, (const uint32_t *)dS, (uint64_t)nS, dLabel,
	                   flags, rank, o[0], o[1], o[2], plane[0], plane[1], plane[2], norm, s->d_table);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(host_table, s->d_table, rows * sizeof(mc33hip_contour), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if ((rc = prop_check(c))) return rc;
	for (unsigned long long k = 0; k < rows; k++) host_table[k].closed = host_table[k].closed == 0;  // (the device counted the points that break the loop)
	return mesh_bad(bad, nP);
}

extern "C" int mc33hip_section_ladder(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT, const double normal[3],
                                      const double *offsets, unsigned n, unsigned long long *segments, double *length, double *area,
                                      unsigned long long *invalid_triangles) {
	if (!c || !normal || !invalid_triangles) return MC33HIP_EINVAL;
	*invalid_triangles = 0;
	if (n > SECTION_LADDER_MAX) { set_err("at most %u offsets, not %u", SECTION_LADDER_MAX, n); return MC33HIP_EINVAL; }
	if ((nV && !dV) || (nT && !dT) || (n && (!offsets || !segments || !length || !area))) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	if (!mesh_sizes_ok(nV, nT) || !section_plane_ok(normal, 3, "normal")) return MC33HIP_EINVAL;
	for (unsigned k = 0; k < n; k++) {
		if (!clip_finite(offsets[k])) { set_err("offsets[%u] must be finite", k); return MC33HIP_EINVAL; }
		if (k && !(offsets[k] > offsets[k - 1u])) { set_err("the offsets must ascend strictly: offsets[%u] <= offsets[%u]", k, k - 1u); return MC33HIP_EINVAL; }
	}
	int rc = use_device(c);
	if (rc) return rc;
	SectionState *s;
	if ((rc = section_state(c, &s))) return rc;
	for (unsigned k = 0; k < n; k++) { segments[k] = 0; length[k] = area[k] = 0.0; }
	if (!nT || !n) {  // (without planes the triangles are not read)
		HIP_TRY(hipStreamSynchronize(c->stream));
		return prop_check(c);
	}
	if (!nV) { *invalid_triangles = nT; return mesh_bad(nT, nV); }
	if ((rc = meas_room(&s->d_lad, &s->lad_cap, (uint64_t)SECTION_LADDER_MAX * 5u))) return rc;
	LadderArgs L;
	L.a = normal[0]; L.b = normal[1]; L.c = normal[2]; L.n = n;
	for (unsigned k = 0; k < n; k++) L.w[k] = offsets[k];
	for (unsigned k = n; k < SECTION_LADDER_MAX; k++) L.w[k] = 0.0;
	double o[3];
	meas_origin(c, o);
	double *d_sums = (double *)(s->d_lad + SECTION_LADDER_MAX);
	HIP_TRY(hipMemsetAsync(s->d_lad, 0, (uint64_t)SECTION_LADDER_MAX * 5u * 8u, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(SectionOut), c->stream));
	// (8 blocks per CU: every block ends with a set of atomics per plane)
	hipLaunchKernelGGL((k_section_ladder<real_t>), dim3(meas_grid(c, nT, 8u)), dim3(256), 0, c->stream, (const real_t *)dV, (uint64_t)nV, (const uint32_t *)dT, (uint64_t)nT, L,
	                   o[0], o[1], o[2], s->d_lad, d_sums, &s->d_out->bad);
	HIP_TRY(hipGetLastError());
	std::vector<unsigned long long> hc(n);
	std::vector<double> hs((size_t)n * 4u);
	HIP_TRY(hipMemcpyAsync(hc.data(), s->d_lad, (size_t)n * 8u, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(hs.data(), d_sums, (size_t)n * 32u, hipMemcpyDeviceToHost, c->stream));
	if ((rc = mesh_op_fetch(c, s))) return rc;
	for (unsigned k = 0; k < n; k++) {
		segments[k] = hc[k];
		length[k] = hs[(size_t)k * 4u];
		area[k] = section_area(&hs[(size_t)k * 4u + 1u], normal);
	}
	*invalid_triangles = s->h_out->bad;
	return mesh_bad(s->h_out->bad, nV);
}
