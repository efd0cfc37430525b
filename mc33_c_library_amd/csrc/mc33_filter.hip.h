// mc33_filter.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// keep or drop whole components of a FINISHED mesh in device memory - an order-preserving, deterministic stream compaction of
// V, N, T and up to two per-vertex words by component label, so that only the kept rows cross the link
// (include/mc33_hip.h: mc33hip_compact_components).  DESIGN.md 12.
//
// The definition (integers only; tests/filter_oracle.py restates it in numpy):
//   valid triangle   its three indices are below nV;          referenced[v]  a valid triangle names v
//   selected[v]      (label[v] is one of the roots) != (invert != 0)
//   keep[v]          referenced[v] && selected[v];            new[v]         the number of kept u < v
//   kept triangle    valid, and its three vertices are kept (a valid triangle whose FIRST vertex is kept and another is not -
//                    labels that are not those of this T - is counted and left out, like an invalid one)
// The passes: k_filt_roots / k_mesh_ref scatter one byte per root / per corner (every racing store writes the same 1);
// k_filt_keep gathers selected through label[v] and counts the kept per tile of 1024 vertices; k_mesh_scan_top turns the tile
// counts into their exclusive sums and leaves the total; k_mesh_place writes new[v] (0xFFFFFFFF: dropped); k_filt_tri_count /
// k_mesh_scan_top again for the triangles; k_filt_rows and k_filt_tris copy.  Where a row lands is decided by the sums alone:
// no atomic takes part in it, and no floating-point instruction touches a row - rows are moved as words.  The two copying
// kernels read the totals on the device and do nothing when the caller's arrays are too small: one wait per call.

struct FiltOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long nV_out, nT_out, comps;
	unsigned long long bad;       // triangles that name a vertex >= nV
	unsigned long long dangling;  // valid triangles whose first vertex is kept and another is not
	unsigned long long pad_[3];
};

struct FilterState {        // scratch of these passes besides the shared keep (referenced, then keep), map (new[v]) and tile sums (the vertex
                            // tiles, behind them the triangle tiles): on the MeasureState from the first call on, grown on demand, freed with it
	FiltOut *d_out, *h_out;
	uint8_t *d_sel;         // [nV] 1: the vertex is one of the caller's roots
	uint64_t sel_cap;
	uint32_t *d_roots;      // the caller's roots
	uint64_t roots_cap;
};

__global__ __launch_bounds__(256) void k_filt_roots(const uint32_t *__restrict__ roots, uint64_t n, uint8_t *__restrict__ sel) {
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) sel[roots[i]] = 1;  // (the host has seen every root < nV)
}

// keep[v] over a tile of MESH_TILE vertices, 4 per lane, in place of referenced[v]; the tile's count; the kept roots (a count, it
// places nothing)
__global__ __launch_bounds__(256) void k_filt_keep(const uint32_t *__restrict__ label, const uint8_t *__restrict__ sel, uint8_t *__restrict__ keep, uint64_t nV,
                                                   uint32_t invert, uint32_t *__restrict__ bsum, FiltOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const uint64_t v0 = mesh_tile_e0();
	uint32_t n = 0u, roots = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint64_t v = v0 + k;
		if (v < nV) {
			const uint32_t l = label[v];
			const uint32_t s = l < nV ? sel[l] : 0u;  // (a label outside the array is no root of the caller's)
			const uint32_t kp = (keep[v] != 0u && (s != 0u) != (invert != 0u)) ? 1u : 0u;
			keep[v] = (uint8_t)kp;
			n += kp;
			roots += (kp && l == (uint32_t)v) ? 1u : 0u;
		}
	}
	const uint32_t tot = block_sum_u32_256(n, sh), tot_roots = block_sum_u32_256(roots, sh);
	if (threadIdx.x == 0u) {
		bsum[blockIdx.x] = tot;
		if (tot_roots) atomicAdd(&out->comps, (unsigned long long)tot_roots);
	}
}

// triangle i of a tile through map: 1 kept (m: its new indices), 0 left out; counts what is left out although its first vertex is kept
__device__ __forceinline__ uint32_t filt_triangle(const uint32_t *__restrict__ T, uint64_t i, uint64_t nV, const uint32_t *__restrict__ map, uint32_t m[3], uint32_t *dangling) {
	const uint32_t *t = T + i * 3u;
	const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
	if (t0 >= nV || t1 >= nV || t2 >= nV) return 0u;  // (tested before anything is gathered through it)
	m[0] = map[t0];
	if (m[0] == MESH_NONE) return 0u;
	m[1] = map[t1]; m[2] = map[t2];
	if (m[1] == MESH_NONE || m[2] == MESH_NONE) { (*dangling)++; return 0u; }
	return 1u;
}

__global__ __launch_bounds__(256) void k_filt_tri_count(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ map,
                                                        uint32_t *__restrict__ bsum, FiltOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const uint64_t i0 = mesh_tile_e0();
	uint32_t n = 0u, dangling = 0u, m[3];
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++)
		if (i0 + k < nT) n += filt_triangle(T, i0 + k, nV, map, m, &dangling);
	const uint32_t tot = block_sum_u32_256(n, sh), tot_d = block_sum_u32_256(dangling, sh);
	if (threadIdx.x == 0u) {
		bsum[blockIdx.x] = tot;
		if (tot_d) atomicAdd(&out->dangling, (unsigned long long)tot_d);
	}
}

// the kept triangles of a tile, renumbered, at the tile's place in oT
__global__ __launch_bounds__(256) void k_filt_tris(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint32_t *__restrict__ map,
                                                   const uint32_t *__restrict__ bsum, const FiltOut *__restrict__ out, uint64_t capV, uint64_t capT,
                                                   uint32_t *__restrict__ oT) {
	__shared__ uint32_t sh[256];
	if (out->nV_out > capV || out->nT_out > capT) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	const uint64_t i0 = mesh_tile_e0();
	uint32_t f[4], m[4][3], own = 0u, dangling = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		f[k] = i0 + k < nT ? filt_triangle(T, i0 + k, nV, map, m[k], &dangling) : 0u;
		own += f[k];
	}
	uint64_t r = mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		if (f[k]) {
			uint32_t *o = oT + r * 3u;
			o[0] = m[k][0]; o[1] = m[k][1]; o[2] = m[k][2];
			r++;
		}
	}
}

// the kept rows of V, N and the attribute words to their new places (ascending: consecutive kept vertices store consecutive
// rows), and the caller's copy of the map.  R: MC33_real - a row of V is 12 or 24 bytes.
template <typename R>
__global__ __launch_bounds__(256) void k_filt_rows(const R *__restrict__ V, const float *__restrict__ N, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                                   const uint32_t *__restrict__ map, uint64_t nV, const FiltOut *__restrict__ out, uint64_t capV, uint64_t capT,
                                                   R *__restrict__ oV, float *__restrict__ oN, uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1,
                                                   uint32_t *__restrict__ oMap) {
	if (out->nV_out > capV || out->nT_out > capT) return;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t m = map[v];
		if (oMap) oMap[v] = m;
		if (m == MESH_NONE) continue;
		mesh_copy_row(V, N, v, oV, oN, m);
		if (A0) oA0[m] = A0[v];
		if (A1) oA1[m] = A1[v];
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void filt_release(void *state) {
	FilterState *f = (FilterState *)state;
	dev_release(&f->d_sel); dev_release(&f->d_roots);
}
static int filt_state(mc33hip_ctx *c, FilterState **f) {
	const int rc = meas_state(c);
	return rc ? rc : mesh_op_state(&c->meas->mesh, filt_release, f);
}

extern "C" int mc33hip_compact_components(mc33hip_ctx *c, mc33hip_compaction *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nV_out = a->nT_out = a->components_kept = 0;
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_counts_ok(a->n_attr, nV, nT)) return MC33HIP_EINVAL;
	const uint64_t capV = mesh_cap(a->capV), capT = mesh_cap(a->capT);
	if (!mesh_pointers_ok((nV && (!a->V || !a->N || !a->label)) || (nT && !a->T) || (a->n_roots && !a->roots) || (capV && (!a->oV || !a->oN)) || (capT && !a->oT), a->n_attr,
	                      a->attr, a->oAttr, nV, capV))
		return MC33HIP_EINVAL;
	for (unsigned long long k = 0; k < a->n_roots; k++)
		if (a->roots[k] >= nV) { set_err("root %u is not below the %llu rows of V", a->roots[k], nV); return MC33HIP_EINVAL; }
	// the compaction is not in place: no output may share a byte with an input
	const MeshRange in[6] = {{a->V, nV * 3u * sizeof(real_t)}, {a->N, nV * 12u}, {a->T, nT * 12u}, {a->label, nV * 4u}, {a->n_attr > 0u ? a->attr[0] : nullptr, nV * 4u},
	                         {a->n_attr > 1u ? a->attr[1] : nullptr, nV * 4u}};
	const MeshRange out[6] = {{a->oV, capV * 3u * sizeof(real_t)}, {a->oN, capV * 12u}, {a->oT, capT * 12u}, {a->oMap, nV * 4u}, {a->n_attr > 0u ? a->oAttr[0] : nullptr, capV * 4u},
	                          {a->n_attr > 1u ? a->oAttr[1] : nullptr, capV * 4u}};
	if (!mesh_ranges_ok(in, 6, out, 6, false, "compaction")) return MC33HIP_EINVAL;  // (an output may meet another output: the call has never looked)
	int rc = use_device(c);
	if (rc) return rc;
	FilterState *f;
	if ((rc = filt_state(c, &f))) return rc;
	MeshHost &h = c->meas->mesh;
	const uint64_t tilesV = (nV + MESH_TILE - 1u) / MESH_TILE, tilesT = (nT + MESH_TILE - 1u) / MESH_TILE;
	if ((rc = meas_scratch(c, nV, tilesV + tilesT))) return rc;
	if ((rc = meas_room(&f->d_sel, &f->sel_cap, nV))) return rc;
	if ((rc = meas_room(&f->d_roots, &f->roots_cap, a->n_roots))) return rc;
	uint32_t *bsumV = h.d_bsum, *bsumT = h.d_bsum + tilesV;
	const uint32_t *T = (const uint32_t *)a->T;
	HIP_TRY(hipMemsetAsync(f->d_out, 0, sizeof(FiltOut), c->stream));
	if (nV) {
		HIP_TRY(hipMemsetAsync(h.d_keep, 0, nV, c->stream));
		HIP_TRY(hipMemsetAsync(f->d_sel, 0, nV, c->stream));
		if (a->n_roots) {
			HIP_TRY(hipMemcpyAsync(f->d_roots, a->roots, a->n_roots * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
			hipLaunchKernelGGL(k_filt_roots, dim3(meas_grid(c, a->n_roots, 16u)), dim3(256), 0, c->stream, f->d_roots, (uint64_t)a->n_roots, f->d_sel);
		}
	}
	if (nT) hipLaunchKernelGGL(k_mesh_ref, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, h.d_keep, &f->d_out->bad);
	if (nV) {
		hipLaunchKernelGGL(k_filt_keep, dim3((uint32_t)tilesV), dim3(256), 0, c->stream, a->label, f->d_sel, h.d_keep, (uint64_t)nV, a->invert ? 1u : 0u, bsumV, f->d_out);
		mesh_scan_sums<MeshFlag, MESH_NEW>(c, h.d_keep, nV, bsumV, &f->d_out->nV_out, h.d_map);
	}
	if (nT) {
		hipLaunchKernelGGL(k_filt_tri_count, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, h.d_map, bsumT, f->d_out);
		mesh_scan_sums<MeshFlag>(c, nullptr, nT, bsumT, &f->d_out->nT_out);  // (k_filt_tris places)
	}
	// the copies: they compare the totals with the capacities on the device, so that the host waits once
	if (nV) hipLaunchKernelGGL((k_filt_rows<real_t>), dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, (const real_t *)a->V, (const float *)a->N,
	                           (const uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr), (const uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr), h.d_map, (uint64_t)nV,
	                           f->d_out, capV, capT, (real_t *)a->oV, (float *)a->oN, (uint32_t *)(a->n_attr > 0u ? a->oAttr[0] : nullptr),
	                           (uint32_t *)(a->n_attr > 1u ? a->oAttr[1] : nullptr), (uint32_t *)a->oMap);
	if (nT) hipLaunchKernelGGL(k_filt_tris, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, h.d_map, bsumT, f->d_out, capV, capT,
	                           (uint32_t *)a->oT);
	if ((rc = mesh_op_fetch(c, f))) return rc;
	const FiltOut &o = *f->h_out;
	a->nV_out = o.nV_out; a->nT_out = o.nT_out; a->components_kept = o.comps;
	if ((rc = mesh_capacity("compacted", o.nV_out, o.nT_out, capV, capT))) return rc;
	const unsigned long long left_out = o.bad + o.dangling;
	if (left_out) {
		set_err("%llu triangle%s left out: %llu name%s a vertex outside the %llu rows of V, %llu a vertex that is not kept (labels of another mesh)", left_out,
		        left_out == 1 ? "" : "s", o.bad, o.bad == 1 ? "s" : "", nV, o.dangling);
		return MC33HIP_ERUNTIME;
	}
	return MC33HIP_OK;
}
