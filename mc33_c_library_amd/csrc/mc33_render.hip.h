// mc33_render.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// a finished V, N, T and an optional colour word per vertex in device memory, drawn into a depth-tested, shaded image and an id
// buffer there (mc33hip_render_surface; the definition is in include/mc33_hip.h, restated in tests/render_oracle.py).
//   k_render_clear      every key of the key buffer to RENDER_NOKEY
//   k_render_vertices   a screen record per vertex: X, Y in 1/256 pixel, z, cw - or "not usable"
//   k_render_triangles  a lane per triangle: its class, and where its box of pixel centres holds at most `small` pixels the lane walks
//                       it and lowers the keys with a 64-bit atomicMin; the others go to a list (one atomicAdd per wave)
//   k_render_tiles      the listed triangles: a wave per 16 x 16 screen tile of a listed triangle's box, the work items by mesh_scan
//                       over the tiles of every list entry - no triangle's pixels fall on one lane or one wave
//   k_render_resolve    a lane per pixel: the key's triangle once more at that pixel, perspective-correct weights, depth, id, shade
// Everything that decides a byte is int64 or IEEE double arithmetic with nothing fused; the keys are lowered by an integer minimum,
// whose result does not depend on the order, and the counts are integer sums: two calls return the same bytes, whatever `small` is.

constexpr unsigned long long RENDER_NOKEY = ~0ull;  // (a real key has a triangle index below 2^32-1 in its low word: nT <= 2^32-1)
constexpr int32_t RENDER_UNUSABLE = INT32_MIN;      // RenderVert::X of a vertex that is not usable
constexpr uint32_t RENDER_TILE = 16u;               // a work item of k_render_tiles: 16 x 16 pixels, four a lane
constexpr uint32_t RENDER_SMALL_DEFAULT = 16u;      // pixels of a box a single lane still walks
constexpr int RENDER_STAGES = 6;                    // clear, vertices, triangles, scan, tiles, resolve

struct RenderVert { int32_t X, Y; double z, cw; };  // 24 bytes
struct RenderView { double m[16]; double W, H; uint32_t width, height; int cull; uint32_t small; };
struct RenderShade { double l[3], ambient, diffuse; uint32_t base, background; int two_sided; };
struct RenderOut {
	unsigned long long drawn, culled, degenerate, rejected, offscreen, bad;  // by class, in the order of RenderClass
	unsigned long long fragments, covered;
	unsigned long long listed;   // entries of the list of large triangles
	unsigned long long tiles;    // the work items of k_render_tiles as the scan summed them (32 bits) ...
	unsigned long long tiles64;  // ... and as they are: more than 2^32-1 is refused
	unsigned long long pad_;
};
struct RenderState {
	RenderOut *d_out, *h_out;
	unsigned long long *d_key;   // [pixels] zq << 32 | triangle
	uint64_t key_cap;
	RenderVert *d_vert;          // [nV]
	uint64_t vert_cap;
	uint32_t *d_list, *d_cnt;    // [nT] the large triangles; [nT + 1] the tiles of every list entry, then where its work items begin
	uint64_t list_cap;
	// MC33_HIP_TIMING >= 2: events around the kernels of the last call, read by mc33hip_render_timing (tools/time_render.py)
	hipEvent_t ev[RENDER_STAGES + 1];
	bool ev_made, timed;
	float ms[RENDER_STAGES];
};

enum RenderClass { RENDER_DRAWN, RENDER_CULLED, RENDER_DEGENERATE, RENDER_REJECTED, RENDER_OFFSCREEN, RENDER_BAD };

// A triangle ready for its pixels.  Edge e runs from corner e to corner e + 1; dx, dy and with them E are negated when area2 < 0, so
// that E >= 0 inside either way: E = dx (Py - Y) - dy (Px - X) with |dx|, |dy| <= 2^24 and |P - corner| < 2^24 + 2^20 stays below 2^49.
// bias: 0 where the edge owns its pixel centres (dy < 0, or dy == 0 and dx > 0), else 1 - the pixel is inside when E >= bias on all three.
struct RenderTri {
	int32_t X[3], Y[3], dx[3], dy[3], bias[3];
	int32_t x0, x1, y0, y1;  // the pixels whose centres the bounding box holds, cut to the viewport
	double z[3], cw[3], area;
	uint32_t v[3];
};

__device__ __forceinline__ int render_setup(const uint32_t *__restrict__ T, uint64_t i, uint64_t nV, const RenderVert *__restrict__ vert, const RenderView &w, RenderTri &t) {
	const uint32_t *q = T + i * 3u;
	t.v[0] = q[0]; t.v[1] = q[1]; t.v[2] = q[2];
	if (t.v[0] >= nV || t.v[1] >= nV || t.v[2] >= nV) return RENDER_BAD;
	bool usable = true;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const RenderVert r = vert[t.v[k]];
		t.X[k] = r.X; t.Y[k] = r.Y; t.z[k] = r.z; t.cw[k] = r.cw;
		usable = usable && r.X != RENDER_UNUSABLE;
	}
	if (!usable) return RENDER_REJECTED;
	const int64_t area2 = (int64_t)(t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (int64_t)(t.X[2] - t.X[0]) * (t.Y[1] - t.Y[0]);
	if (area2 == 0) return RENDER_DEGENERATE;
	const bool front = area2 < 0;
	if ((w.cull == 1 && !front) || (w.cull == 2 && front)) return RENDER_CULLED;
	const int32_t s = front ? -1 : 1;
#pragma unroll
	for (int e = 0; e < 3; e++) {
		const int n = e == 2 ? 0 : e + 1;
		t.dx[e] = s * (t.X[n] - t.X[e]);
		t.dy[e] = s * (t.Y[n] - t.Y[e]);
		t.bias[e] = t.dy[e] < 0 || (t.dy[e] == 0 && t.dx[e] > 0) ? 0 : 1;
	}
	t.area = (double)(front ? -area2 : area2);
	// pixel centres 256 p + 128 with min <= centre <= max: p from ceil((min - 128) / 256) to floor((max - 128) / 256); >> is the floor
	const int32_t xl = min(t.X[0], min(t.X[1], t.X[2])), xh = max(t.X[0], max(t.X[1], t.X[2]));
	const int32_t yl = min(t.Y[0], min(t.Y[1], t.Y[2])), yh = max(t.Y[0], max(t.Y[1], t.Y[2]));
	t.x0 = max((xl - 128 + 255) >> 8, 0); t.x1 = min((xh - 128) >> 8, (int32_t)w.width - 1);
	t.y0 = max((yl - 128 + 255) >> 8, 0); t.y1 = min((yh - 128) >> 8, (int32_t)w.height - 1);
	if (t.x0 > t.x1 || t.y0 > t.y1) return RENDER_OFFSCREEN;
	return RENDER_DRAWN;
}

__device__ __forceinline__ int64_t render_edge(const RenderTri &t, int e, int32_t Px, int32_t Py) {
	return (int64_t)t.dx[e] * (Py - t.Y[e]) - (int64_t)t.dy[e] * (Px - t.X[e]);
}

// the weights of pixel (px, py) - w_i = E of the edge opposite corner i -, whether its centre is inside, and its depth
__device__ __forceinline__ bool render_pixel(const RenderTri &t, int32_t px, int32_t py, int64_t wt[3], double *zf) {
	const int32_t Px = 256 * px + 128, Py = 256 * py + 128;
	const int64_t E0 = render_edge(t, 0, Px, Py), E1 = render_edge(t, 1, Px, Py), E2 = render_edge(t, 2, Px, Py);
	wt[0] = E1; wt[1] = E2; wt[2] = E0;
	*zf = (((double)E1 * t.z[0] + (double)E2 * t.z[1]) + (double)E0 * t.z[2]) / t.area;
	return E0 >= t.bias[0] && E1 >= t.bias[1] && E2 >= t.bias[2];
}

// one fragment test and, where there is a fragment, the key lowered; returns 1 for a fragment
__device__ __forceinline__ uint32_t render_fragment(const RenderTri &t, uint32_t i, int32_t px, int32_t py, uint32_t width, unsigned long long *key) {
	int64_t wt[3];
	double zf;
	if (!render_pixel(t, px, py, wt, &zf) || !(zf >= 0.0 && zf <= 1.0)) return 0u;
	const uint32_t zq = (uint32_t)floor(zf * 4294967295.0 + 0.5);
	const unsigned long long k = ((unsigned long long)zq << 32) | i;
	unsigned long long *slot = key + ((uint64_t)py * width + (uint32_t)px);
	// The early test is a plain load.  Within this call the keys only fall: k_render_clear, a kernel of its own before the first of
	// them, wrote RENDER_NOKEY, and nothing but atomicMin touches a key until k_render_resolve, a later kernel.  A value read from
	// an L1 or an XCD's L2 that another XCD's atomic has since lowered is a value the key HAD in this call, so it can only be too
	// large: where k >= it, k >= the key as it is now, and the atomic would change nothing; where k < it the atomic at device scope
	// decides.  A stale read costs an atomic and never a pixel.  (DESIGN.md 10's rule for claimed memory forbids plain loads of
	// words whose value decides a branch that cannot be taken back; this one only leaves out an operation that is a no-op.)
	if (k < *slot) atomicMin(slot, k);
	return 1u;
}

__device__ __forceinline__ unsigned long long render_wave_sum_u64(unsigned long long x) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) x += shfl_down_u64(x, d);
	return x;  // (lane 0)
}

__global__ __launch_bounds__(256) void k_render_clear(unsigned long long *__restrict__ key, uint64_t n) {
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256u) key[p] = RENDER_NOKEY;
}

template <typename R>
__global__ __launch_bounds__(256) void k_render_vertices(const R *__restrict__ V, uint64_t nV, RenderView w, RenderVert *__restrict__ out) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const R *q = V + v * 3u;
		const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
		double c[4];
#pragma unroll
		for (int r = 0; r < 4; r++) c[r] = ((w.m[4 * r] * x + w.m[4 * r + 1] * y) + w.m[4 * r + 2] * z) + w.m[4 * r + 3];
		RenderVert o;
		o.X = RENDER_UNUSABLE; o.Y = 0; o.z = 0.0; o.cw = 0.0;
		if (isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(c[3]) && c[3] > 0.0) {
			const double ix = c[0] / c[3], iy = c[1] / c[3], zz = c[2] / c[3];
			const double sx = (ix * 0.5 + 0.5) * w.W, sy = (0.5 - iy * 0.5) * w.H;
			const double fx = floor(sx * 256.0 + 0.5), fy = floor(sy * 256.0 + 0.5);
			if (fabs(fx) <= 8388608.0 && fabs(fy) <= 8388608.0) {  // (an infinite quotient fails here)
				o.X = (int32_t)fx; o.Y = (int32_t)fy; o.z = zz; o.cw = c[3];
			}
		}
		out[v] = o;
	}
}

__global__ __launch_bounds__(256) void k_render_triangles(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const RenderVert *__restrict__ vert, RenderView w,
                                                          unsigned long long *key, uint32_t *__restrict__ list, uint32_t *__restrict__ cnt, RenderOut *out) {
	__shared__ uint32_t sh[4];
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t)gridDim.x * 256u, rounds = (nT + stride - 1u) / stride;
	uint32_t n[6] = {0u, 0u, 0u, 0u, 0u, 0u};
	unsigned long long frags = 0ull, tiles = 0ull;
	for (uint64_t r = 0; r < rounds; r++) {  // (every lane of a wave makes every round: the ballot below is the whole wave's)
		const uint64_t i = r * stride + (uint64_t)blockIdx.x * 256u + threadIdx.x;
		RenderTri t;
		bool large = false;
		if (i < nT) {
			const int cls = render_setup(T, i, nV, vert, w, t);
#pragma unroll
			for (int k = 0; k < 6; k++) n[k] += cls == k ? 1u : 0u;  // (registers, not an indexed array)
			if (cls == RENDER_DRAWN) {
				large = (uint32_t)(t.x1 - t.x0 + 1) * (uint32_t)(t.y1 - t.y0 + 1) > w.small;
				if (!large)
					for (int32_t py = t.y0; py <= t.y1; py++)
						for (int32_t px = t.x0; px <= t.x1; px++) frags += render_fragment(t, (uint32_t)i, px, py, w.width, key);
			}
		}
		const unsigned long long m = __ballot(large);
		if (m) {  // one atomicAdd for the wave's entries; the order of the list decides nothing
			const int leader = __ffsll((long long)m) - 1;
			unsigned long long base = 0ull;
			if ((int)lane == leader) base = atomicAdd(&out->listed, (unsigned long long)__popcll(m));
			base = ((unsigned long long)__shfl((uint32_t)(base >> 32), leader, 64) << 32) | __shfl((uint32_t)base, leader, 64);
			if (large) {
				const uint64_t slot = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));  // (< nT: a triangle is listed once)
				const uint32_t nt = (uint32_t)((t.x1 >> 4) - (t.x0 >> 4) + 1) * (uint32_t)((t.y1 >> 4) - (t.y0 >> 4) + 1);
				list[slot] = (uint32_t)i;
				cnt[slot] = nt;
				tiles += nt;
			}
		}
	}
#pragma unroll
	for (int k = 0; k < 6; k++) {
		const uint32_t tot = block_sum_u32_256(n[k], sh);
		if (threadIdx.x == 0u && tot) atomicAdd(&out->drawn + k, (unsigned long long)tot);
	}
	frags = render_wave_sum_u64(frags);
	tiles = render_wave_sum_u64(tiles);
	if (lane == 0u) {
		if (frags) atomicAdd(&out->fragments, frags);
		if (tiles) atomicAdd(&out->tiles64, tiles);
	}
}

// starts: cnt after its scan - where the work items of list entry j begin, starts[nT] their number.  A wave takes work item `it`:
// tile (it - starts[j]) of entry j's box, tiles counted along x first.  Whatever `it` and the tile come to, a pixel is touched
// only inside the triangle's own box, which lies in the viewport.
__global__ __launch_bounds__(256) void k_render_tiles(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const RenderVert *__restrict__ vert, RenderView w,
                                                      unsigned long long *key, const uint32_t *__restrict__ list, const uint32_t *__restrict__ starts, RenderOut *out) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t items = starts[nT], waves = (uint64_t)gridDim.x * 4u;
	const uint32_t listed = (uint32_t)min(out->listed, (unsigned long long)nT);  // (written by k_render_triangles, a kernel before this one)
	unsigned long long frags = 0ull;
	if (listed)
		for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < items; it += waves) {
			uint32_t lo = 0u, hi = listed;  // starts[lo] <= it < starts[hi]
			while (hi - lo > 1u) {
				const uint32_t mid = lo + ((hi - lo) >> 1);
				if (starts[mid] <= it) lo = mid; else hi = mid;
			}
			const uint32_t i = list[lo];
			if (i >= nT) continue;
			RenderTri t;
			if (render_setup(T, i, nV, vert, w, t) != RENDER_DRAWN) continue;
			const uint32_t local = (uint32_t)(it - starts[lo]), txn = (uint32_t)((t.x1 >> 4) - (t.x0 >> 4) + 1);
			const int32_t bx = (int32_t)(((uint32_t)(t.x0 >> 4) + local % txn) * RENDER_TILE), by = (int32_t)(((uint32_t)(t.y0 >> 4) + local / txn) * RENDER_TILE);
			// E is linear: an edge that has all four corner pixels of the tile outside has the whole tile outside
			bool out_of = false;
#pragma unroll
			for (int e = 0; e < 3; e++) {
				const int64_t a = render_edge(t, e, 256 * bx + 128, 256 * by + 128), b = render_edge(t, e, 256 * (bx + 15) + 128, 256 * by + 128);
				const int64_t c = render_edge(t, e, 256 * bx + 128, 256 * (by + 15) + 128), d = render_edge(t, e, 256 * (bx + 15) + 128, 256 * (by + 15) + 128);
				out_of = out_of || (a < t.bias[e] && b < t.bias[e] && c < t.bias[e] && d < t.bias[e]);
			}
			if (out_of) continue;
			const int32_t px = bx + (int32_t)(lane & 15u);
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const int32_t py = by + (int32_t)(lane >> 4) + 4 * k;
				if (px >= t.x0 && px <= t.x1 && py >= t.y0 && py <= t.y1) frags += render_fragment(t, i, px, py, w.width, key);
			}
		}
	frags = render_wave_sum_u64(frags);
	if (lane == 0u && frags) atomicAdd(&out->fragments, frags);
}

__device__ __forceinline__ uint32_t render_channel(double shade, double l0, double l1, double l2, uint32_t c0, uint32_t c1, uint32_t c2, int shift) {
	double x = shade * ((l0 * (double)((c0 >> shift) & 255u) + l1 * (double)((c1 >> shift) & 255u)) + l2 * (double)((c2 >> shift) & 255u));
	x = x > 0.0 ? x : 0.0;  // (a NaN gives 0)
	x = x < 255.0 ? x : 255.0;
	return (uint32_t)floor(x + 0.5);
}

__global__ __launch_bounds__(256) void k_render_resolve(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const RenderVert *__restrict__ vert, const float *__restrict__ N,
                                                        const uint32_t *__restrict__ C, RenderView w, RenderShade s, const unsigned long long *__restrict__ key,
                                                        uint32_t *__restrict__ oRGBA, float *__restrict__ oDepth, uint32_t *__restrict__ oTri, RenderOut *out) {
	__shared__ uint32_t sh[4];
	const uint64_t pixels = (uint64_t)w.width * w.height;
	uint32_t covered = 0u;
	for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < pixels; p += (uint64_t)gridDim.x * 256u) {
		const unsigned long long k = key[p];
		const uint32_t i = (uint32_t)k;
		RenderTri t;
		if (k == RENDER_NOKEY || i >= nT || render_setup(T, i, nV, vert, w, t) != RENDER_DRAWN) {  // (a key names a drawn triangle)
			if (oRGBA) oRGBA[p] = s.background;
			if (oDepth) oDepth[p] = __int_as_float(0x7F800000);
			if (oTri) oTri[p] = 0xFFFFFFFFu;
			continue;
		}
		covered++;
		int64_t wt[3];
		double zf;
		(void)render_pixel(t, (int32_t)(p % w.width), (int32_t)(p / w.width), wt, &zf);
		if (oDepth) oDepth[p] = (float)zf;
		if (oTri) oTri[p] = i;
		if (!oRGBA) continue;
		const double q0 = ((double)wt[0] / t.area) / t.cw[0], q1 = ((double)wt[1] / t.area) / t.cw[1], q2 = ((double)wt[2] / t.area) / t.cw[2];
		const double sum = (q0 + q1) + q2;
		const double l0 = q0 / sum, l1 = q1 / sum, l2 = q2 / sum;
		const float *n0 = N + (uint64_t)t.v[0] * 3u, *n1 = N + (uint64_t)t.v[1] * 3u, *n2 = N + (uint64_t)t.v[2] * 3u;
		const double nx = (l0 * (double)n0[0] + l1 * (double)n1[0]) + l2 * (double)n2[0];
		const double ny = (l0 * (double)n0[1] + l1 * (double)n1[1]) + l2 * (double)n2[1];
		const double nz = (l0 * (double)n0[2] + l1 * (double)n1[2]) + l2 * (double)n2[2];
		const double len = sqrt((nx * nx + ny * ny) + nz * nz);
		double td = 0.0;
		if (isfinite(len) && len != 0.0) {
			td = ((nx * s.l[0] + ny * s.l[1]) + nz * s.l[2]) / len;
			td = s.two_sided ? fabs(td) : (td > 0.0 ? td : 0.0);
		}
		const double shade = s.ambient + s.diffuse * td;
		const uint32_t c0 = C ? C[t.v[0]] : s.base, c1 = C ? C[t.v[1]] : s.base, c2 = C ? C[t.v[2]] : s.base;
		oRGBA[p] = render_channel(shade, l0, l1, l2, c0, c1, c2, 0) | (render_channel(shade, l0, l1, l2, c0, c1, c2, 8) << 8) |
		           (render_channel(shade, l0, l1, l2, c0, c1, c2, 16) << 16) | 0xFF000000u;
	}
	const uint32_t tot = block_sum_u32_256(covered, sh);
	if (threadIdx.x == 0u && tot) atomicAdd(&out->covered, (unsigned long long)tot);
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void render_release(void *state) {
	RenderState *s = (RenderState *)state;
	dev_release(&s->d_key); dev_release(&s->d_vert); dev_release(&s->d_list); dev_release(&s->d_cnt);
	for (int k = 0; s->ev_made && k <= RENDER_STAGES; k++) (void)hipEventDestroy(s->ev[k]);
	s->ev_made = false;
}

static uint32_t render_small_switch() {  // MC33_HIP_RENDER_SMALL, read when a context is created: 0 is a value here, not "unset"
	const char *e = getenv("MC33_HIP_RENDER_SMALL");
	if (!e || !*e) return RENDER_SMALL_DEFAULT;
	const unsigned long long v = strtoull(e, nullptr, 10);
	return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

extern "C" int mc33hip_render_surface(mc33hip_ctx *c, mc33hip_rendering *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->drawn = a->culled = a->degenerate = a->rejected = a->offscreen = a->invalid_triangles = a->fragments = a->covered = 0;
	if (a->width == 0u || a->width > 4096u || a->height == 0u || a->height > 4096u) { set_err("an image of %u x %u: both sizes are 1 .. 4096", a->width, a->height); return MC33HIP_EINVAL; }
	bool finite = std::isfinite(a->ambient) && std::isfinite(a->diffuse);
	for (int k = 0; k < 16; k++) finite = finite && std::isfinite(a->m[k]);
	for (int k = 0; k < 3; k++) finite = finite && std::isfinite(a->light[k]);
	if (!finite) { set_err("a matrix entry, a light component, ambient or diffuse is not finite"); return MC33HIP_EINVAL; }
	const double llen = sqrt((a->light[0] * a->light[0] + a->light[1] * a->light[1]) + a->light[2] * a->light[2]);
	if (!(llen > 0.0) || !std::isfinite(llen)) { set_err("the light has no direction"); return MC33HIP_EINVAL; }
	if (a->cull < 0 || a->cull > 2) { set_err("cull = %d is none of 0 (none), 1 (back), 2 (front)", a->cull); return MC33HIP_EINVAL; }
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_sizes_ok(nV, nT)) return MC33HIP_EINVAL;
	if ((nV && (!a->V || !a->N)) || (nT && !a->T)) { set_err("a null pointer where the size is not zero"); return MC33HIP_EINVAL; }
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = meas_state(c))) return rc;
	RenderState *s;
	if ((rc = mesh_op_state(&c->meas->mesh, render_release, &s))) return rc;
	MeshHost &h = c->meas->mesh;

	RenderView w;
	RenderShade sd;
	memset(&w, 0, sizeof w);
	memset(&sd, 0, sizeof sd);
	for (int k = 0; k < 16; k++) w.m[k] = a->m[k];
	w.W = (double)a->width; w.H = (double)a->height; w.width = a->width; w.height = a->height; w.cull = a->cull; w.small = c->sw.render_small;
	for (int k = 0; k < 3; k++) sd.l[k] = a->light[k] / llen;
	sd.ambient = a->ambient; sd.diffuse = a->diffuse; sd.base = a->base_color; sd.background = a->background; sd.two_sided = a->two_sided ? 1 : 0;

	const uint64_t pixels = (uint64_t)a->width * a->height, tilesT = (nT + MESH_TILE - 1u) / MESH_TILE;
	if ((rc = meas_room(&s->d_key, &s->key_cap, pixels))) return rc;
	if (nV && (rc = meas_room(&s->d_vert, &s->vert_cap, nV))) return rc;
	if (nT) {
		if ((rc = meas_room(&h.d_bsum, &h.bsum_cap, tilesT))) return rc;
		if (s->list_cap < nT + 1u || !s->d_cnt) {
			const uint64_t n = nT + nT / 8u + 256u;
			if ((rc = dev_room_all("list of large triangles", &s->list_cap, n, {dev_array(&s->d_list, n), dev_array(&s->d_cnt, n)}))) return rc;
		}
	}
	const bool timing = c->timing_level >= 2;
	if (timing && !s->ev_made) {
		for (int k = 0; k <= RENDER_STAGES; k++) HIP_TRY(hipEventCreate(&s->ev[k]));
		s->ev_made = true;
	}
	s->timed = false;
#define RENDER_MARK(k) do { if (timing) HIP_TRY(hipEventRecord(s->ev[k], c->stream)); } while (0)
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(RenderOut), c->stream));
	RENDER_MARK(0);
	hipLaunchKernelGGL(k_render_clear, dim3(meas_grid(c, pixels, 16u)), dim3(256), 0, c->stream, s->d_key, pixels);
	RENDER_MARK(1);
	if (nV) hipLaunchKernelGGL((k_render_vertices<real_t>), dim3(meas_grid(c, nV, 16u)), dim3(256), 0, c->stream, (const real_t *)a->V, (uint64_t)nV, w, s->d_vert);
	RENDER_MARK(2);
	if (nT) {
		HIP_TRY(hipMemsetAsync(s->d_cnt, 0, (nT + 1u) * 4u, c->stream));
		hipLaunchKernelGGL(k_render_triangles, dim3(meas_grid(c, nT, 16u)), dim3(256), 0, c->stream, (const uint32_t *)a->T, (uint64_t)nT, (uint64_t)nV,
		                   (const RenderVert *)s->d_vert, w, s->d_key, s->d_list, s->d_cnt, s->d_out);
		RENDER_MARK(3);
		// the work items of the listed triangles: an exclusive scan of their tile counts, in place (entries behind the list count 0)
		mesh_scan<MeshCount, MESH_STARTS>(c, s->d_cnt, nT, h.d_bsum, &s->d_out->tiles, s->d_cnt);
		RENDER_MARK(4);
		hipLaunchKernelGGL(k_render_tiles, dim3((uint32_t)std::max(1, c->cus) * 8u), dim3(256), 0, c->stream, (const uint32_t *)a->T, (uint64_t)nT, (uint64_t)nV,
		                   (const RenderVert *)s->d_vert, w, s->d_key, (const uint32_t *)s->d_list, (const uint32_t *)s->d_cnt, s->d_out);
	}
	else { RENDER_MARK(3); RENDER_MARK(4); }
	RENDER_MARK(5);
	hipLaunchKernelGGL(k_render_resolve, dim3(meas_grid(c, pixels, 16u)), dim3(256), 0, c->stream, (const uint32_t *)a->T, (uint64_t)nT, (uint64_t)nV, (const RenderVert *)s->d_vert,
	                   (const float *)a->N, (const uint32_t *)a->C, w, sd, (const unsigned long long *)s->d_key, (uint32_t *)a->oRGBA, (float *)a->oDepth, (uint32_t *)a->oTri, s->d_out);
	RENDER_MARK(6);
#undef RENDER_MARK
	if ((rc = mesh_op_fetch(c, s))) return rc;
	if (timing) {
		for (int k = 0; k < RENDER_STAGES; k++) HIP_TRY(hipEventElapsedTime(&s->ms[k], s->ev[k], s->ev[k + 1]));
		s->timed = true;
	}
	const RenderOut o = *s->h_out;
	a->drawn = o.drawn; a->culled = o.culled; a->degenerate = o.degenerate; a->rejected = o.rejected; a->offscreen = o.offscreen; a->invalid_triangles = o.bad;
	a->fragments = o.fragments; a->covered = o.covered;
	if (o.tiles64 > 0xFFFFFFFFull) { set_err("the large triangles cover %llu screen tiles, more than 2^32-1: the image is not complete", o.tiles64); return MC33HIP_ERUNTIME; }
	return mesh_bad(o.bad, nV);
}

extern "C" int mc33hip_render_timing(mc33hip_ctx *c, float ms[6]) {
	MeshOp *op = c && c->meas && ms ? mesh_op_peek(&c->meas->mesh, render_release) : nullptr;
	const RenderState *s = op ? (const RenderState *)op->state : nullptr;
	if (!s || !s->timed) { set_err("no timed rendering on this context (MC33_HIP_TIMING >= 2 when it is created)"); return MC33HIP_EINVAL; }
	for (int k = 0; k < RENDER_STAGES; k++) ms[k] = s->ms[k];
	return MC33HIP_OK;
}
