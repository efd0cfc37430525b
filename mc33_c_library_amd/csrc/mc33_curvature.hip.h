// mc33_curvature.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there; not a header to include elsewhere):
// mean, Gaussian and principal curvatures of the implicit surface F = iso at the vertices of a finished V array, from the gradient
// and the Hessian of the resident grid by finite differences - k_curvature, one more pass over V that gathers the grid the way
// k_property gathers a property grid - and a palette over any float array (include/mc33_hip.h: mc33hip_curvature_vertices,
// mc33hip_color_values).  DESIGN.md 22.
//
// The definition is in include/mc33_hip.h; tests/curvature_oracle.py restates it in numpy float64, one operation per line.
// Everything is IEEE double, nothing fused (-ffp-contract=off), only + - * / and sqrt: the outputs are held to the oracle bit for bit.
//
// The first part of this file - everything down to the line that says so - has no HIP in it: curv_vertex is the kernel's whole
// arithmetic and indexing, and tests/curvature_host.cpp compiles this text with the host compiler, runs it vertex by vertex on a
// buffer that holds exactly what the call may read, and is held to the oracle.

#ifndef CV_HD
#define CV_HD __host__ __device__ __forceinline__
#endif
#ifdef __HIPCC__
#define CV_UNROLL _Pragma("unroll")
#else
#define CV_UNROLL
#endif

struct CurvGrid {
	uint64_t pitch, slice;   // samples per row / per plane of the resident grid
	uint32_t N[3];           // cells per axis (x, y, z), each >= 2
	double r0[3], d[3];
	double sign;             // +1.0 or -1.0
};

CV_HD double curv_lerp(double p, double q, double f) { return f == 0.0 ? p : p * (1.0 - f) + q * f; }

// step 4 of the definition (and, with the adjugate for h, step 7)
CV_HD double curv_form(const double g[3], double hxx, double hyy, double hzz, double hxy, double hxz, double hyz) {
	return (((g[0] * g[0]) * hxx + (g[1] * g[1]) * hyy) + (g[2] * g[2]) * hzz) + 2.0 * ((((g[0] * g[1]) * hxy) + ((g[0] * g[2]) * hxz)) + ((g[1] * g[2]) * hyz));
}

// The quantities of the node n (0 <= n[a] <= N[a]) that GROUP asks for, side by side in q in this order: CURV_G gx, gy, gz and
// CURV_H hxx, hyy, hzz from seven samples - the node and two more on each axis line through it: n - 1 and n + 1, on a face the
// two that complete c - 1, c, c + 1 about the nearest interior point c; CURV_X hxy, hxz, hyz from twelve - the four corners
// (p | m, p | m) in each of the three planes.  The samples of a call - nineteen for all nine quantities - are loaded together,
// before any is used.  Every index is clamped to 0 .. N[a] as the definition clamps it, so only grid points are read.
constexpr int CURV_G = 1, CURV_H = 2, CURV_X = 4, CURV_ALL = 7;
constexpr int curv_count(int group) { return 3 * ((group & 1) + ((group >> 1) & 1) + ((group >> 2) & 1)); }

template <typename T, int GROUP>
CV_HD void curv_node(const CurvGrid &a, const T *grid, const uint32_t n[3], double *q) {
	constexpr bool LINES = (GROUP & (CURV_G | CURV_H)) != 0, PLANES = (GROUP & CURV_X) != 0;
	const int64_t stride[3] = {1, (int64_t)a.pitch, (int64_t)a.slice};
	bool low[3], high[3];
	double span[3];
	CV_UNROLL
	for (int k = 0; k < 3; k++) {
		low[k] = n[k] == 0u;
		high[k] = n[k] == a.N[k];
		span[k] = (double)((high[k] ? 0 : 1) + (low[k] ? 0 : 1)) * a.d[k];   // (double)(p - m) * d
	}
	const T *c = grid + ((uint64_t)n[2] * a.slice + (uint64_t)n[1] * a.pitch + n[0]);
	T rc = (T)0, rlo[3] = {(T)0, (T)0, (T)0}, rhi[3] = {(T)0, (T)0, (T)0}, rd[3][4] = {{(T)0, (T)0, (T)0, (T)0}, {(T)0, (T)0, (T)0, (T)0}, {(T)0, (T)0, (T)0, (T)0}};
	if constexpr (LINES) {
		rc = c[0];
		CV_UNROLL
		for (int k = 0; k < 3; k++) {
			rlo[k] = c[(low[k] ? 1 : (high[k] ? -2 : -1)) * stride[k]];
			rhi[k] = c[(low[k] ? 2 : (high[k] ? -1 : 1)) * stride[k]];
		}
	}
	if constexpr (PLANES) {
		CV_UNROLL
		for (int e = 0; e < 3; e++) {   // the planes xy, xz, yz
			const int u = e == 2 ? 1 : 0, w = e == 0 ? 1 : 2;
			const int64_t pu = high[u] ? 0 : stride[u], mu = low[u] ? 0 : -stride[u];   // p = min(n + 1, N), m = max(n - 1, 0)
			const int64_t pw = high[w] ? 0 : stride[w], mw = low[w] ? 0 : -stride[w];
			rd[e][0] = c[pu + pw]; rd[e][1] = c[pu + mw]; rd[e][2] = c[mu + pw]; rd[e][3] = c[mu + mw];
		}
	}
	if constexpr (LINES) {
		const double sc = (double)rc;
		CV_UNROLL
		for (int k = 0; k < 3; k++) {
			const double l = (double)rlo[k], h = (double)rhi[k];
			// S(c - 1), S(c), S(c + 1): the node in the middle, or at the face's end of the three
			const double a0 = low[k] ? sc : l, a1 = low[k] ? l : (high[k] ? h : sc), a2 = high[k] ? sc : h;
			if constexpr ((GROUP & CURV_G) != 0) {
				const double sp = low[k] ? a1 : a2, sm = high[k] ? a1 : a0;
				q[k] = (sp - sm) / span[k];
			}
			if constexpr ((GROUP & CURV_H) != 0) q[curv_count(GROUP & CURV_G) + k] = ((a2 - a1) - (a1 - a0)) / (a.d[k] * a.d[k]);
		}
	}
	if constexpr (PLANES) {
		CV_UNROLL
		for (int e = 0; e < 3; e++) {
			const int u = e == 2 ? 1 : 0, w = e == 0 ? 1 : 2;
			q[curv_count(GROUP & (CURV_G | CURV_H)) + e] = (((double)rd[e][0] - (double)rd[e][1]) - ((double)rd[e][2] - (double)rd[e][3])) / (span[u] * span[w]);
		}
	}
}

// where a vertex lies: its cell, which axes have f != 0 (L of them), and the f of those axes in the order x, y, z
struct CurvPlace {
	uint32_t i[3], L;
	bool dx, dy, dz;
	double f[3];
};

// The quantities of a GROUP interpolated at the vertex, into v.  The 2^L live nodes are counted by one number whose bits go to the
// live axes in the order x, y, z, so a lane makes exactly as many turns as it has nodes, and the lerps along x, then y, then z are
// folded as the nodes arrive: a node whose bit of an axis is 0 waits in that axis' slot, its partner is lerped with it and moves
// up.  A node with f == 0 on its axis is never formed and its samples are never read.  LEVELS: the slots there are, >= L.
template <typename T, int GROUP, int LEVELS>
CV_HD void curv_gather(const CurvGrid &a, const T *grid, const CurvPlace &p, double *v) {
	constexpr int NQ = curv_count(GROUP);
	double s[LEVELS][NQ];
	CV_UNROLL
	for (int l = 0; l < LEVELS; l++) { CV_UNROLL for (int k = 0; k < NQ; k++) s[l][k] = 0.0; }
	for (uint32_t n = 0; n < (1u << p.L); n++) {
		const uint32_t b0 = n & 1u, b1 = (n >> 1) & 1u, b2 = n >> 2;
		const uint32_t node[3] = {p.i[0] + (p.dx ? b0 : 0u), p.i[1] + (p.dy ? (p.dx ? b1 : b0) : 0u), p.i[2] + (p.dz ? (p.L == 3u ? b2 : (p.L == 2u ? b1 : b0)) : 0u)};
		curv_node<T, GROUP>(a, grid, node, v);
		if (p.L >= 1u) {
			if (!b0) { CV_UNROLL for (int k = 0; k < NQ; k++) s[0][k] = v[k]; }
			else {
				CV_UNROLL for (int k = 0; k < NQ; k++) v[k] = curv_lerp(s[0][k], v[k], p.f[0]);
				if constexpr (LEVELS >= 2) {
					if (p.L >= 2u) {
						if (!b1) { CV_UNROLL for (int k = 0; k < NQ; k++) s[1][k] = v[k]; }
						else {
							CV_UNROLL for (int k = 0; k < NQ; k++) v[k] = curv_lerp(s[1][k], v[k], p.f[1]);
							if constexpr (LEVELS >= 3) {
								if (p.L == 3u) {
									if (!b2) { CV_UNROLL for (int k = 0; k < NQ; k++) s[2][k] = v[k]; }
									else { CV_UNROLL for (int k = 0; k < NQ; k++) v[k] = curv_lerp(s[2][k], v[k], p.f[2]); }
								}
							}
						}
					}
				}
			}
		}
	}
}

// One vertex: row = its three coordinates, out = mean, gauss, k1, k2.  An extracted vertex lies on a grid edge: one f is not 0 and
// two nodes exist for it; a made-up one has 1, 2, 4 or 8.  With one or two nodes all nine quantities of a node come from one round
// of nineteen loads and wait in one slot.  A vertex in a grid face (four nodes, two slots per quantity) takes the six quantities of
// the axis lines and the three of the planes in two walks over its nodes, a vertex inside a cell (eight nodes, three slots) takes
// g, the diagonal of H and the rest of H in three: the slots of any walk are at most twelve doubles, which is what keeps the
// kernel inside 128 registers.  Only the last splits samples that one round would share - the seven of the axis lines twice.
template <typename T, typename R>
CV_HD void curv_vertex(const CurvGrid &a, const T *grid, const R *row, float out[4]) {
	const double x[3] = {(double)row[0], (double)row[1], (double)row[2]};
	CurvPlace p;
	double f[3];
	CV_UNROLL
	for (int k = 0; k < 3; k++) {   // steps 1 - 2 of the property definition (mc33_property.hip.h)
		const double g = (x[k] - a.r0[k]) / a.d[k];
		const double fl = floor(g), top = (double)a.N[k];
		const double ic = !(fl >= 0.0) ? 0.0 : (fl > top ? top : fl);
		double fr = g - ic;
		fr = fr < 0.0 ? 0.0 : (fr > 1.0 ? 1.0 : fr);
		p.i[k] = (uint32_t)ic;
		f[k] = p.i[k] == a.N[k] ? 0.0 : fr;
	}
	p.dx = f[0] != 0.0; p.dy = f[1] != 0.0; p.dz = f[2] != 0.0;
	p.L = (p.dx ? 1u : 0u) + (p.dy ? 1u : 0u) + (p.dz ? 1u : 0u);
	p.f[0] = p.dx ? f[0] : (p.dy ? f[1] : f[2]); p.f[1] = p.dx && p.dy ? f[1] : f[2]; p.f[2] = f[2];
	double v[9];
	CV_UNROLL
	for (int k = 0; k < 9; k++) v[k] = 0.0;
	if (p.L < 2u) curv_gather<T, CURV_ALL, 1>(a, grid, p, v);
	else if (p.L == 2u) {
		curv_gather<T, CURV_G | CURV_H, 2>(a, grid, p, v);
		curv_gather<T, CURV_X, 2>(a, grid, p, v + 6);
	} else {
		curv_gather<T, CURV_G, 3>(a, grid, p, v);
		curv_gather<T, CURV_H, 3>(a, grid, p, v + 3);
		curv_gather<T, CURV_X, 3>(a, grid, p, v + 6);
	}
	const double hxx = v[3], hyy = v[4], hzz = v[5], hxy = v[6], hxz = v[7], hyz = v[8];
	const double g2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
	const double gl = sqrt(g2);
	const double tr = (hxx + hyy) + hzz;
	const double gHg = curv_form(v, hxx, hyy, hzz, hxy, hxz, hyz);
	const double mean = a.sign * ((gHg - g2 * tr) / ((2.0 * g2) * gl));
	const double axx = hyy * hzz - hyz * hyz, ayy = hxx * hzz - hxz * hxz, azz = hxx * hyy - hxy * hxy;
	const double axy = hxz * hyz - hxy * hzz, axz = hxy * hyz - hxz * hyy, ayz = hxy * hxz - hxx * hyz;
	const double gAg = curv_form(v, axx, ayy, azz, axy, axz, ayz);
	const double gauss = gAg / (g2 * g2);
	const double disc = mean * mean - gauss;
	const double r = sqrt(disc < 0.0 ? 0.0 : disc);
	out[0] = (float)mean;
	out[1] = (float)gauss;
	out[2] = (float)(mean + r);
	out[3] = (float)(mean - r);
}

// a float as an unsigned key in the order of the values, and back (the spectrum's sp_key on 32 bits)
CV_HD uint32_t curv_key(float v) {
	const uint32_t b = __builtin_bit_cast(uint32_t, v);
	return (b >> 31) ? ~b : b | 0x80000000u;
}
CV_HD float curv_unkey(uint32_t k) { return __builtin_bit_cast(float, (k >> 31) ? k & 0x7FFFFFFFu : ~k); }
CV_HD bool curv_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u; }

// the summary as a lane and the device keep it: keys of the extremes of the finite values of each output, and the vertices that
// have a value that is not finite
struct CurvSum {
	uint32_t lo[4], hi[4], undefined;
};
struct CurvOut {
	uint32_t lo[4], hi[4];
	unsigned long long undefined;
};
CV_HD uint32_t curv_none_lo() { return curv_key(__builtin_huge_valf()); }
CV_HD uint32_t curv_none_hi() { return curv_key(-__builtin_huge_valf()); }
CV_HD void curv_sum_init(CurvSum &o) {
	for (int k = 0; k < 4; k++) { o.lo[k] = curv_none_lo(); o.hi[k] = curv_none_hi(); }
	o.undefined = 0u;
}
CV_HD void curv_sum_add(CurvSum &o, const float val[4]) {
	bool all = true;
	CV_UNROLL
	for (int k = 0; k < 4; k++) {
		const bool fin = curv_finite(val[k]);
		const uint32_t key = curv_key(val[k]);
		o.lo[k] = fin && key < o.lo[k] ? key : o.lo[k];
		o.hi[k] = fin && key > o.hi[k] ? key : o.hi[k];
		all = all && fin;
	}
	o.undefined += all ? 0u : 1u;
}

// ---- everything above compiles without HIP (tests/curvature_host.cpp) ---------------------------------------------------------------
#ifdef __HIPCC__

struct CurvState {   // on the MeasureState from the first call on, freed with it
	CurvOut *d_out, *h_out;
};

__global__ void k_curv_init(CurvOut *__restrict__ out) {
	if (threadIdx.x < 4u) { out->lo[threadIdx.x] = curv_none_lo(); out->hi[threadIdx.x] = curv_none_hi(); }
	if (threadIdx.x == 0u) out->undefined = 0ull;
}

// One lane per vertex, grid stride, launched like k_property.  The lanes of a wave sit on x-, y- and z-edges mixed: each walks its
// own live nodes (curv_vertex), so a wave of extracted vertices makes two turns of the node loop, not eight.  The summary is kept
// per lane, joined over the wave by shuffles when the lane has no vertex left, and leaves the wave as one atomic per quantity on
// ordered keys: minimum and maximum do not depend on the order, two calls return the same bytes.  A wave first looks at the word
// and keeps an atomic that could not change it to itself - the extremes only ever move outwards, so what it skips is a no-op - and
// counts the undefined vertices, of which a surface has few or none, not the finite ones: most waves leave no atomic at all.
template <typename R>
__global__ __launch_bounds__(256) void k_curvature(CurvGrid a, const sample_t *__restrict__ grid, const R *__restrict__ V, uint64_t nV,
                                                                                          float *__restrict__ oMean, float *__restrict__ oGauss, float *__restrict__ oK1,
                                                                                          float *__restrict__ oK2, CurvOut *out) {
	CurvSum mine;
	curv_sum_init(mine);
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		float val[4];
		curv_vertex<sample_t, R>(a, grid, V + v * 3u, val);
		if (oMean) oMean[v] = val[0];
		if (oGauss) oGauss[v] = val[1];
		if (oK1) oK1[v] = val[2];
		if (oK2) oK2[v] = val[3];
		curv_sum_add(mine, val);
	}
#pragma unroll
	for (int s = 32; s; s >>= 1) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint32_t l = (uint32_t)__shfl_xor((int)mine.lo[k], s), h = (uint32_t)__shfl_xor((int)mine.hi[k], s);
			mine.lo[k] = l < mine.lo[k] ? l : mine.lo[k];
			mine.hi[k] = h > mine.hi[k] ? h : mine.hi[k];
		}
		mine.undefined += (uint32_t)__shfl_xor((int)mine.undefined, s);   // (a lane has far fewer than 2^26 vertices)
	}
	if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (mine.lo[k] < __hip_atomic_load(&out->lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&out->lo[k], mine.lo[k]);
			if (mine.hi[k] > __hip_atomic_load(&out->hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&out->hi[k], mine.hi[k]);
		}
		if (mine.undefined) atomicAdd(&out->undefined, (unsigned long long)mine.undefined);
	}
}

// step 6 of the property definition over any float array: k_property<R, true>'s colour, word for word
__global__ __launch_bounds__(256) void k_color_values(const float *__restrict__ P, uint64_t nV, const uint32_t *__restrict__ palette, uint32_t n, uint32_t nan_color,
                                                      double lo, double hi, uint32_t *__restrict__ out) {
	__shared__ uint32_t pal[256];
	pal[threadIdx.x] = threadIdx.x < n ? palette[threadIdx.x] : 0u;
	__syncthreads();
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const float val = P[v];
		uint32_t col = nan_color;
		if (val == val) {
			double s = ((double)val - lo) / (hi - lo);
			s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
			col = pal[(uint32_t)floor(s * (double)(n - 1u) + 0.5)];
		}
		out[v] = col;
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void curv_release(void *) {}   // (the state holds nothing beyond its result block; the function is the key of the registration)

static uint32_t curv_blocks(mc33hip_ctx *c, unsigned long long nV) {   // a lane per vertex up to 64 blocks per CU, a grid stride beyond (prop_enqueue)
	return (uint32_t)std::min<uint64_t>((nV + 255u) / 256u, (uint64_t)std::max(1, c->cus) * 64u);
}

extern "C" int mc33hip_curvature_vertices(mc33hip_ctx *c, mc33hip_curvature *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	const mc33hip_grid_desc &d = c->desc;
	if (!c->d_grid) { set_err("no grid is resident in this context"); return MC33HIP_EINVAL; }
	if (d.plane0 != 0u || d.npz_resident != d.nz_total + 1u) { set_err("the context holds a z-slab: curvature needs the whole grid"); return MC33HIP_EINVAL; }
	if (c->inclined) { set_err("curvature is defined for orthogonal grids only"); return MC33HIP_EINVAL; }
	if (d.npx < 3u || d.npy < 3u || d.nz_total < 2u) { set_err("curvature needs 2 cells on every axis, not %u x %u x %u", d.npx - 1u, d.npy - 1u, d.nz_total); return MC33HIP_EINVAL; }
	if (a->sign != 1 && a->sign != -1) { set_err("sign = %d: +1 or -1", a->sign); return MC33HIP_EINVAL; }
	if (a->nV && !a->dV) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	for (int k = 0; k < 4; k++) { a->lo[k] = __builtin_huge_val(); a->hi[k] = -__builtin_huge_val(); }
	a->finite = a->undefined = 0ull;
	if (!a->nV) return MC33HIP_OK;
	int rc;
	if ((rc = use_device(c))) return rc;
	if ((rc = meas_state(c))) return rc;
	CurvState *s;
	if ((rc = mesh_op_state(&c->meas->mesh, curv_release, &s))) return rc;
	CurvGrid g;
	g.pitch = c->pitch; g.slice = c->slice;
	g.N[0] = d.npx - 1u; g.N[1] = d.npy - 1u; g.N[2] = d.nz_total;
	for (int k = 0; k < 3; k++) { g.r0[k] = d.r0[k]; g.d[k] = d.d[k]; }
	g.sign = (double)a->sign;
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	hipLaunchKernelGGL(k_curv_init, dim3(1), dim3(64), 0, c->stream, s->d_out);
	hipLaunchKernelGGL((k_curvature<real_t>), dim3(curv_blocks(c, a->nV)), dim3(256), 0, c->stream, g, (const sample_t *)c->d_grid, (const real_t *)a->dV, (uint64_t)a->nV,
	                   a->oMean, a->oGauss, a->oK1, a->oK2, s->d_out);
	if ((rc = mesh_op_fetch(c, s))) return rc;
	for (int k = 0; k < 4; k++) { a->lo[k] = (double)curv_unkey(s->h_out->lo[k]); a->hi[k] = (double)curv_unkey(s->h_out->hi[k]); }
	a->undefined = s->h_out->undefined;
	a->finite = a->nV - a->undefined;
	return MC33HIP_OK;
}

extern "C" int mc33hip_color_values(mc33hip_ctx *c, const float *dP, unsigned long long nV, const int *palette, unsigned int n, double lo, double hi, int nan_color,
                                    int *dC) {
	if (!c || !palette || (nV && (!dP || !dC))) return MC33HIP_EINVAL;
	if (n < 2u || n > 256u || !(lo < hi)) { set_err("colour map needs 2..256 colours and lo < hi"); return MC33HIP_EINVAL; }
	int rc = use_device(c);
	if (rc || (rc = prop_scratch(c))) return rc;
	if (!nV) return MC33HIP_OK;
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	HIP_TRY(hipMemcpyAsync(c->d_prop_pal, palette, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_color_values, dim3(curv_blocks(c, nV)), dim3(256), 0, c->stream, dP, (uint64_t)nV, (const uint32_t *)c->d_prop_pal, n, (uint32_t)nan_color, lo, hi,
	                   (uint32_t *)dC);
	HIP_TRY(hipGetLastError());
	return MC33HIP_OK;
}

#endif  // __HIPCC__
