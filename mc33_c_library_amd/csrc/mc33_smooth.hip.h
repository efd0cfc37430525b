// mc33_smooth.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// Taubin's lambda | mu smoothing of a FINISHED mesh in device memory and vertex normals recomputed from its triangles
// (include/mc33_hip.h: mc33hip_smooth_surface, mc33hip_vertex_normals).  DESIGN.md 13.
//
// The definition (IEEE double, nothing fused: -ffp-contract=off; tests/smooth_oracle.py restates it in numpy):
//   valid triangle   its three indices are below nV; every side a -> b with a != b, in the order T0 -> T1, T1 -> T2, T2 -> T0, is
//                    one use of the edge {a, b}
//   nb(v)            the distinct w for which {v, w} has a use, ascending; deg(v) = |nb(v)|;  boundary(v): some {v, w} has one use
//   fixed(v)         deg(v) == 0, or pin_boundary and boundary(v)
//   pass(f)          P'[v] = P[v] for a fixed v; otherwise per axis s = P[w1], s = s + P[wk] (k = 2 .. deg, ascending w),
//                    m = s / deg, L = m - P[v], P'[v] = (MC33_real)(P[v] + f * L); every neighbour is read from P (Jacobi)
//   normals          inc(v): the valid triangles that name v, ascending, each once; n = the sum of g_i = (p1 - p0) x (p2 - p0) in
//                    that order, starting from the first; oN[v] = (float)(n / sqrt((n.x*n.x + n.y*n.y) + n.z*n.z)) where that
//                    length is > 0 and finite, else (0, 0, 0)
// The passes: both lists are CSR arrays made straight from T - k_sm_count adds 2 directed entries per side (1 per distinct corner
// for the incidence list) with integer atomics, the tile scan of mc33_mesh.hip.h turns the counts into row starts,
// k_sm_fill places the entries through an atomic cursor.  The order inside a row depends on scheduling until a LATER kernel - one
// lane per row - has sorted it: k_sm_rows sorts, collapses equal neighbours (a neighbour that stood once in the row is an edge with
// one use: boundary) and leaves deg and the fixed flag; k_sm_normals sorts its row of triangles before it adds.  Nothing a block
// wrote with plain stores is read by another block of the same kernel.  k_sm_pass is the hot path: 2 x iterations launches, a lane
// per vertex.  The incidence list is built in the arrays of the adjacency, when the passes are through.

struct SmOut {              // what a call brings to the host (device copy and pinned twin)
	unsigned long long max_degree, isolated, boundary, bad;
	unsigned long long entries;   // of the list last built (the scan's total)
	unsigned long long pad_[3];
};

constexpr uint32_t SM_TIMED_PASSES = 64u;
struct SmoothTimers {       // a measurement aid (tools/time_smooth.py), not part of any result
	hipEvent_t ev[SM_TIMED_PASSES + 4u];  // 0, 1 around the adjacency; 2, 3 around the normals; 4 + j behind pass j
	bool made, adjacency, normals;
	uint32_t passes;
};

struct SmoothState {        // scratch of these passes besides the shared tile sums: on the MeasureState from the first call on, grown on demand, freed with it
	SmOut *d_out, *h_out;
	uint32_t *d_start;      // [nV + 1] counts, then row starts
	uint64_t start_cap;
	uint32_t *d_deg;        // [nV] the cursor of k_sm_fill, then deg
	uint64_t deg_cap;
	uint32_t *d_ent;        // [6 nT] neighbours ([3 nT] triangles) row by row
	uint64_t ent_cap;
	uint8_t *d_fixed;       // [nV]
	uint64_t fixed_cap;
	void *d_tmp;            // [nV x 3 MC33_real] the other side of the ping-pong
	uint64_t tmp_cap;       // in bytes
	SmoothTimers timers;
};

// INC 0: 2 directed entries per side a -> b, a != b (the adjacency); INC 1: 1 entry per distinct corner (the incidence list).
// bad_out: where invalid triangles are counted, or null (a call that builds both lists counts them once)
template <int INC>
__global__ __launch_bounds__(256) void k_sm_count(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, uint32_t *__restrict__ cnt,
                                                  unsigned long long *__restrict__ bad_out) {
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		if (INC) {
			atomicAdd(cnt + t0, 1u);
			if (t1 != t0) atomicAdd(cnt + t1, 1u);
			if (t2 != t0 && t2 != t1) atomicAdd(cnt + t2, 1u);
		} else {
			const uint32_t n0 = (t0 != t1 ? 1u : 0u) + (t2 != t0 ? 1u : 0u), n1 = (t0 != t1 ? 1u : 0u) + (t1 != t2 ? 1u : 0u),
			               n2 = (t1 != t2 ? 1u : 0u) + (t2 != t0 ? 1u : 0u);
			if (n0) atomicAdd(cnt + t0, n0);
			if (n1) atomicAdd(cnt + t1, n1);
			if (n2) atomicAdd(cnt + t2, n2);
		}
	}
	if (bad && bad_out) atomicAdd(bad_out, (unsigned long long)bad);
}

__device__ __forceinline__ void sm_put(const uint32_t *__restrict__ start, uint32_t *__restrict__ cur, uint32_t *__restrict__ ent, uint32_t row, uint32_t what) {
	ent[start[row] + atomicAdd(cur + row, 1u)] = what;  // (below start[row + 1]: k_sm_count counted this very entry)
}

template <int INC>
__global__ __launch_bounds__(256) void k_sm_fill(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ start,
                                                 uint32_t *__restrict__ cur, uint32_t *__restrict__ ent) {
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) continue;
		if (INC) {
			sm_put(start, cur, ent, t0, (uint32_t)i);
			if (t1 != t0) sm_put(start, cur, ent, t1, (uint32_t)i);
			if (t2 != t0 && t2 != t1) sm_put(start, cur, ent, t2, (uint32_t)i);
		} else {
			if (t0 != t1) { sm_put(start, cur, ent, t0, t1); sm_put(start, cur, ent, t1, t0); }
			if (t1 != t2) { sm_put(start, cur, ent, t1, t2); sm_put(start, cur, ent, t2, t1); }
			if (t2 != t0) { sm_put(start, cur, ent, t2, t0); sm_put(start, cur, ent, t0, t2); }
		}
	}
}

// One lane sorts the n words of its row where they lie (no other lane touches them; a lane sees its own stores): insertion for the
// short rows a surface has, a heap sort beyond 32 words - any length is sorted, the time of a long row is its lane's alone.
__device__ __forceinline__ void sm_sift(uint32_t *r, uint32_t i, uint32_t n) {
	const uint32_t x = r[i];
	for (;;) {
		uint32_t k = 2u * i + 1u;
		if (k >= n) break;
		uint32_t y = r[k];
		if (k + 1u < n) {
			const uint32_t z = r[k + 1u];
			if (z > y) { y = z; k++; }
		}
		if (y <= x) break;
		r[i] = y;
		i = k;
	}
	r[i] = x;
}
__device__ __forceinline__ void sm_sort_row(uint32_t *r, uint32_t n) {
	if (n <= 32u) {
		for (uint32_t i = 1u; i < n; i++) {
			const uint32_t x = r[i];
			uint32_t j = i;
			while (j > 0u) {
				const uint32_t y = r[j - 1u];
				if (y <= x) break;
				r[j] = y;
				j--;
			}
			r[j] = x;
		}
		return;
	}
	for (uint32_t i = n / 2u; i > 0u; i--) sm_sift(r, i - 1u, n);
	for (uint32_t m = n - 1u; m > 0u; m--) {
		const uint32_t top = r[0];
		r[0] = r[m];
		r[m] = top;
		sm_sift(r, 0u, m);
	}
}

// a lane per row of the adjacency: sort, collapse, deg (over the cursor), fixed, and the call's three counts of vertices
__global__ __launch_bounds__(256) void k_sm_rows(const uint32_t *__restrict__ start, uint32_t *ent, uint32_t *__restrict__ deg, uint8_t *__restrict__ fixed,
                                                 uint64_t nV, uint32_t pin, SmOut *__restrict__ out) {
	uint32_t maxd = 0u, lone = 0u, nbnd = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t b = start[v], n = start[v + 1u] - b;
		uint32_t *r = ent + b;
		sm_sort_row(r, n);
		uint32_t d = 0u, bnd = 0u;
		for (uint32_t i = 0u; i < n;) {
			const uint32_t w = r[i];
			uint32_t uses = 1u;
			while (i + uses < n && r[i + uses] == w) uses++;
			r[d++] = w;
			if (uses == 1u) bnd = 1u;
			i += uses;
		}
		deg[v] = d;
		fixed[v] = (uint8_t)((d == 0u || (pin && bnd)) ? 1u : 0u);
		maxd = d > maxd ? d : maxd;
		lone += d == 0u ? 1u : 0u;
		nbnd += bnd;
	}
	maxd = wave_max_u32(maxd); lone = wave_sum_u32(lone); nbnd = wave_sum_u32(nbnd);
	if ((threadIdx.x & 63u) == 0u) {
		if (maxd) atomicMax(&out->max_degree, (unsigned long long)maxd);
		if (lone) atomicAdd(&out->isolated, (unsigned long long)lone);
		if (nbnd) atomicAdd(&out->boundary, (unsigned long long)nbnd);
	}
}

// One pass P -> Q with factor f, a lane per vertex.  The row's neighbours are taken four at a time - indices, then rows, then the
// additions in their order - so that a lane has up to twelve gathers in flight.  R: MC33_real.
template <typename R>
__global__ __launch_bounds__(256) void k_sm_pass(const R *__restrict__ P, R *__restrict__ Q, const uint32_t *__restrict__ start, const uint32_t *__restrict__ deg,
                                                 const uint32_t *__restrict__ ent, const uint8_t *__restrict__ fixed, uint64_t nV, double f) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const R *p = P + v * 3u;
		R *q = Q + v * 3u;
		const R p0 = p[0], p1 = p[1], p2 = p[2];
		if (fixed[v]) { q[0] = p0; q[1] = p1; q[2] = p2; continue; }
		const uint32_t d = deg[v];
		const uint32_t *r = ent + start[v];
		const R *w0 = P + (uint64_t)r[0] * 3u;
		double s0 = (double)w0[0], s1 = (double)w0[1], s2 = (double)w0[2];
		uint32_t k = 1u;
		for (; k + 4u <= d; k += 4u) {
			const uint32_t a = r[k], b = r[k + 1u], c = r[k + 2u], e = r[k + 3u];
			const R *wa = P + (uint64_t)a * 3u, *wb = P + (uint64_t)b * 3u, *wc = P + (uint64_t)c * 3u, *we = P + (uint64_t)e * 3u;
			const R a0 = wa[0], a1 = wa[1], a2 = wa[2], b0 = wb[0], b1 = wb[1], b2 = wb[2];
			const R c0 = wc[0], c1 = wc[1], c2 = wc[2], e0 = we[0], e1 = we[1], e2 = we[2];
			s0 = s0 + (double)a0; s1 = s1 + (double)a1; s2 = s2 + (double)a2;
			s0 = s0 + (double)b0; s1 = s1 + (double)b1; s2 = s2 + (double)b2;
			s0 = s0 + (double)c0; s1 = s1 + (double)c1; s2 = s2 + (double)c2;
			s0 = s0 + (double)e0; s1 = s1 + (double)e1; s2 = s2 + (double)e2;
		}
		for (; k < d; k++) {
			const R *w = P + (uint64_t)r[k] * 3u;
			const R x0 = w[0], x1 = w[1], x2 = w[2];
			s0 = s0 + (double)x0; s1 = s1 + (double)x1; s2 = s2 + (double)x2;
		}
		const double dd = (double)d;
		const double L0 = s0 / dd - (double)p0, L1 = s1 / dd - (double)p1, L2 = s2 / dd - (double)p2;
		q[0] = (R)((double)p0 + f * L0);
		q[1] = (R)((double)p1 + f * L1);
		q[2] = (R)((double)p2 + f * L2);
	}
}

// a lane per row of the incidence list: sort the triangles, add their cross products in that order, normalise
template <typename R>
__global__ __launch_bounds__(256) void k_sm_normals(const R *__restrict__ Q, const uint32_t *__restrict__ T, const uint32_t *__restrict__ start, uint32_t *ent,
                                                    uint64_t nV, float *__restrict__ oN) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t b = start[v], n = start[v + 1u] - b;
		uint32_t *r = ent + b;
		sm_sort_row(r, n);
		double nx = 0.0, ny = 0.0, nz = 0.0;
		for (uint32_t k = 0u; k < n; k++) {
			const uint32_t *t = T + (uint64_t)r[k] * 3u;  // (a valid triangle: k_sm_fill entered no other)
			const R *r0 = Q + (uint64_t)t[0] * 3u, *r1 = Q + (uint64_t)t[1] * 3u, *r2 = Q + (uint64_t)t[2] * 3u;
			const double p0x = (double)r0[0], p0y = (double)r0[1], p0z = (double)r0[2];
			const double ux = (double)r1[0] - p0x, uy = (double)r1[1] - p0y, uz = (double)r1[2] - p0z;
			const double wx = (double)r2[0] - p0x, wy = (double)r2[1] - p0y, wz = (double)r2[2] - p0z;
			const double gx = uy * wz - uz * wy, gy = uz * wx - ux * wz, gz = ux * wy - uy * wx;
			if (k == 0u) { nx = gx; ny = gy; nz = gz; }
			else { nx = nx + gx; ny = ny + gy; nz = nz + gz; }
		}
		const double len = sqrt((nx * nx + ny * ny) + nz * nz);
		float *o = oN + v * 3u;
		if (n != 0u && len > 0.0 && len < __builtin_huge_val()) { o[0] = (float)(nx / len); o[1] = (float)(ny / len); o[2] = (float)(nz / len); }
		else { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void smooth_release(void *state) {
	SmoothState *s = (SmoothState *)state;
	dev_release(&s->d_start); dev_release(&s->d_deg); dev_release(&s->d_ent); dev_release(&s->d_fixed); dev_release(&s->d_tmp);
	if (s->timers.made)
		for (hipEvent_t &e : s->timers.ev) (void)hipEventDestroy(e);
}
// the state, with no timing taken yet by this call
static int smooth_state(mc33hip_ctx *c, SmoothState **s) {
	int rc = meas_state(c);
	if (rc || (rc = mesh_op_state(&c->meas->mesh, smooth_release, s))) return rc;
	(*s)->timers.adjacency = (*s)->timers.normals = false;
	(*s)->timers.passes = 0u;
	return 0;
}

// the events of mc33hip_smooth_timing: recorded only at timing level 2 (mc33hip_set_timing), never waited for by the call itself
static int sm_mark(mc33hip_ctx *c, SmoothState *s, uint32_t k) {
	SmoothTimers &t = s->timers;
	if (c->timing_level < 2 || k >= SM_TIMED_PASSES + 4u) return 0;
	if (!t.made) {
		for (hipEvent_t &e : t.ev) HIP_TRY(hipEventCreate(&e));
		t.made = true;
	}
	HIP_TRY(hipEventRecord(t.ev[k], c->stream));
	return 0;
}

// the CSR list of T in d_start / d_deg (the cursor) / d_ent: enqueues
template <int INC>
static int sm_build_list(mc33hip_ctx *c, SmoothState *s, const uint32_t *T, uint64_t nT, uint64_t nV, bool count_bad) {
	const uint32_t gridT = meas_grid(c, nT, 16u);
	HIP_TRY(hipMemsetAsync(s->d_start, 0, (nV + 1u) * sizeof(uint32_t), c->stream));
	HIP_TRY(hipMemsetAsync(s->d_deg, 0, nV * sizeof(uint32_t), c->stream));
	hipLaunchKernelGGL((k_sm_count<INC>), dim3(gridT), dim3(256), 0, c->stream, T, nT, nV, s->d_start, count_bad ? &s->d_out->bad : (unsigned long long *)nullptr);
	mesh_scan<MeshCount, MESH_STARTS>(c, s->d_start, nV, c->meas->mesh.d_bsum, &s->d_out->entries, s->d_start);  // (in place: counts -> row starts, start[nV] = the total)
	hipLaunchKernelGGL((k_sm_fill<INC>), dim3(gridT), dim3(256), 0, c->stream, T, nT, nV, s->d_start, s->d_deg, s->d_ent);
	HIP_TRY(hipGetLastError());
	return 0;
}

static int sm_room(mc33hip_ctx *c, SmoothState *s, uint64_t nV, uint64_t nT, bool adjacency, uint64_t tmp_bytes) {
	int rc;
	// (row starts are 32-bit words)
	if ((adjacency ? 6u : 3u) * nT > 0xFFFFFFFFull) { set_err("the lists of %llu triangles need more than 2^32-1 entries", (unsigned long long)nT); return MC33HIP_ENOMEM; }
	if ((rc = meas_room(&s->d_start, &s->start_cap, nV + 1u))) return rc;
	if ((rc = meas_room(&s->d_deg, &s->deg_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_ent, &s->ent_cap, (adjacency ? 6u : 3u) * nT))) return rc;
	if ((rc = meas_room(&s->d_fixed, &s->fixed_cap, nV))) return rc;
	if ((rc = meas_room(&c->meas->mesh.d_bsum, &c->meas->mesh.bsum_cap, (nV + MESH_TILE - 1u) / MESH_TILE))) return rc;  // (of the shared scratch only the tile sums)
	if (tmp_bytes > s->tmp_cap || !s->d_tmp) {
		dev_release(&s->d_tmp);
		s->tmp_cap = 0;
		const uint64_t want = tmp_bytes + tmp_bytes / 8u + 256u;
		if (hipMalloc(&s->d_tmp, want) != hipSuccess) { (void)hipGetLastError(); set_err("no device memory for %llu bytes of smoothing scratch", (unsigned long long)want); return MC33HIP_ENOMEM; }
		s->tmp_cap = want;
	}
	return 0;
}

static int sm_normals(mc33hip_ctx *c, SmoothState *s, const real_t *Q, const uint32_t *T, uint64_t nT, uint64_t nV, float *oN, bool count_bad) {
	int rc;
	if ((rc = sm_mark(c, s, 2u))) return rc;
	if ((rc = sm_build_list<1>(c, s, T, nT, nV, count_bad))) return rc;
	hipLaunchKernelGGL((k_sm_normals<real_t>), dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, Q, T, s->d_start, s->d_ent, nV, oN);
	HIP_TRY(hipGetLastError());
	s->timers.normals = c->timing_level >= 2;
	return sm_mark(c, s, 3u);
}

// The normals of a mesh with nV, nT > 0, as mc33hip_vertex_normals takes them and as a part takes those of the mesh it has just
// written (T names no vertex outside V then).  It overwrites the shared tile sums - nothing else of the shared scratch - behind
// what the caller enqueued, and waits.
static int sm_normals_call(mc33hip_ctx *c, const real_t *V, const uint32_t *T, uint64_t nT, uint64_t nV, float *oN, unsigned long long *bad) {
	SmoothState *s;
	int rc = smooth_state(c, &s);
	if (rc || (rc = sm_room(c, s, nV, nT, false, 0u))) return rc;
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(SmOut), c->stream));
	if ((rc = sm_normals(c, s, V, T, nT, nV, oN, bad != nullptr))) return rc;
	if ((rc = mesh_op_fetch(c, s))) return rc;
	if (bad) *bad = s->h_out->bad;
	return 0;
}

extern "C" int mc33hip_smooth_surface(mc33hip_ctx *c, mc33hip_smoothing *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->max_degree = a->isolated_vertices = a->boundary_vertices = a->invalid_triangles = 0;
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	if ((nV && (!a->V || !a->oV)) || (nT && !a->T)) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	if (!(a->lambda > 0.0 && a->lambda <= 1.0) || !(a->mu >= -1.0 && a->mu <= 0.0)) { set_err("lambda must lie in (0, 1] and mu in [-1, 0]"); return MC33HIP_EINVAL; }
	if (a->iterations > 1000u) { set_err("at most 1000 iterations, not %u", a->iterations); return MC33HIP_EINVAL; }
	const uint64_t vbytes = nV * 3u * sizeof(real_t), nbytes = nV * 12u, tbytes = nT * 12u;
	if ((a->oV != a->V && mesh_ranges_meet(a->oV, vbytes, a->V, vbytes)) || mesh_ranges_meet(a->oV, vbytes, a->T, tbytes) || mesh_ranges_meet(a->oN, nbytes, a->V, vbytes) ||
	    mesh_ranges_meet(a->oN, nbytes, a->T, tbytes) || mesh_ranges_meet(a->oN, nbytes, a->oV, vbytes)) {
		set_err("an output array overlaps another array of the call (oV may be exactly V, nothing else)");
		return MC33HIP_EINVAL;
	}
	int rc = use_device(c);
	if (rc) return rc;
	SmoothState *s;
	if ((rc = smooth_state(c, &s))) return rc;
	const real_t *V = (const real_t *)a->V;
	real_t *oV = (real_t *)a->oV;
	const uint32_t *T = (const uint32_t *)a->T;
	if (!nV || !nT) {  // nothing to build: every vertex is isolated, every triangle (of no vertices) invalid
		if (nV && oV != V) HIP_TRY(hipMemcpyAsync(oV, V, vbytes, hipMemcpyDeviceToDevice, c->stream));
		if (nV && a->oN) HIP_TRY(hipMemsetAsync(a->oN, 0, nbytes, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if ((rc = prop_check(c))) return rc;
		a->isolated_vertices = nV;
		a->invalid_triangles = nT;
		return mesh_bad(nT, nV);
	}
	const uint32_t passes = a->iterations * (a->mu != 0.0 ? 2u : 1u);
	if ((rc = sm_room(c, s, nV, nT, true, passes ? vbytes : 0u))) return rc;
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(SmOut), c->stream));
	if ((rc = sm_mark(c, s, 0u))) return rc;
	if ((rc = sm_build_list<0>(c, s, T, nT, nV, true))) return rc;
	const uint32_t gridV = meas_grid(c, nV, 16u);
	hipLaunchKernelGGL(k_sm_rows, dim3(gridV), dim3(256), 0, c->stream, s->d_start, s->d_ent, s->d_deg, s->d_fixed, (uint64_t)nV, a->pin_boundary ? 1u : 0u, s->d_out);
	HIP_TRY(hipGetLastError());
	if ((rc = sm_mark(c, s, 1u))) return rc;
	s->timers.adjacency = c->timing_level >= 2;
	// The ping-pong: pass j writes oV when an even number of passes follows it, the scratch rows otherwise, so that the last pass
	// lands in oV.  In place with an odd number of passes the first one would write the rows it gathers from: the passes then
	// begin in the scratch rows, end there, and the rows are copied.
	real_t *tmp = (real_t *)s->d_tmp;
	const bool shifted = oV == V && (passes & 1u);
	const real_t *src = V;
	uint32_t j = 0u;
	for (uint32_t it = 0u; it < a->iterations; it++)
		for (int half = 0; half < (a->mu != 0.0 ? 2 : 1); half++, j++) {
			real_t *dst = (((passes - 1u - j) & 1u) != 0u) != shifted ? tmp : oV;
			hipLaunchKernelGGL((k_sm_pass<real_t>), dim3(gridV), dim3(256), 0, c->stream, src, dst, s->d_start, s->d_deg, s->d_ent, s->d_fixed, (uint64_t)nV,
			                   half ? a->mu : a->lambda);
			if ((rc = sm_mark(c, s, 4u + j))) return rc;
			src = dst;
		}
	HIP_TRY(hipGetLastError());
	s->timers.passes = c->timing_level >= 2 ? std::min(passes, SM_TIMED_PASSES) : 0u;
	if (src != oV) HIP_TRY(hipMemcpyAsync(oV, src, vbytes, hipMemcpyDeviceToDevice, c->stream));  // (no pass at all, or the shifted ones)
	if (a->oN && (rc = sm_normals(c, s, oV, T, nT, nV, a->oN, false))) return rc;
	if ((rc = mesh_op_fetch(c, s))) return rc;
	const SmOut &h = *s->h_out;
	a->max_degree = h.max_degree; a->isolated_vertices = h.isolated; a->boundary_vertices = h.boundary; a->invalid_triangles = h.bad;
	return mesh_bad(h.bad, nV);
}

extern "C" int mc33hip_vertex_normals(mc33hip_ctx *c, const void *dV, unsigned long long nV, const void *dT, unsigned long long nT, float *oN) {
	if (!c || !mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	if ((nV && (!dV || !oN)) || (nT && !dT)) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	if (mesh_ranges_meet(oN, nV * 12u, dV, nV * 3u * sizeof(real_t)) || mesh_ranges_meet(oN, nV * 12u, dT, nT * 12u)) {
		set_err("oN overlaps an input array");
		return MC33HIP_EINVAL;
	}
	int rc = use_device(c);
	if (rc) return rc;
	if (!nV || !nT) {
		SmoothState *s;
		if ((rc = smooth_state(c, &s))) return rc;
		if (nV) HIP_TRY(hipMemsetAsync(oN, 0, nV * 12u, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		if ((rc = prop_check(c))) return rc;
		return mesh_bad(nT, nV);
	}
	unsigned long long bad;
	if ((rc = sm_normals_call(c, (const real_t *)dV, (const uint32_t *)dT, nT, nV, oN, &bad))) return rc;
	return mesh_bad(bad, nV);
}

extern "C" int mc33hip_smooth_timing(mc33hip_ctx *c, float *adjacency_ms, float *normals_ms, float *pass_ms, unsigned capacity, unsigned *passes) {
	if (!c || !passes || (capacity && !pass_ms)) return MC33HIP_EINVAL;
	*passes = 0;
	if (adjacency_ms) *adjacency_ms = 0.f;
	if (normals_ms) *normals_ms = 0.f;
	const MeshOp *op = c->meas ? mesh_op_peek(&c->meas->mesh, smooth_release) : nullptr;
	if (!op) return MC33HIP_OK;
	const SmoothTimers &t = ((const SmoothState *)op->state)->timers;
	if (adjacency_ms && t.adjacency) { HIP_TRY(hipEventElapsedTime(adjacency_ms, t.ev[0], t.ev[1])); }
	if (normals_ms && t.normals) { HIP_TRY(hipEventElapsedTime(normals_ms, t.ev[2], t.ev[3])); }
	*passes = t.passes;
	for (uint32_t j = 0u; j < t.passes && j < capacity; j++) HIP_TRY(hipEventElapsedTime(pass_ms + j, t.ev[j ? 3u + j : 1u], t.ev[4u + j]));
	return MC33HIP_OK;
}
