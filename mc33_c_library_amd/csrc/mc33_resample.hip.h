// mc33_resample.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, last; not a header to include elsewhere):
// the resident grid resampled into a second device grid before anything is extracted from it - a separable correlation with up to
// 17 taps per axis, edge samples replicated, and an integer stride per axis (include/mc33_hip.h: mc33hip_resample_grid).  DESIGN.md 15.
//
// The definition is in include/mc33_hip.h; tests/resample_oracle.py restates it in numpy.  Every intermediate is an exact double
// and every sum runs in ascending tap order from its first product: tiles, chunks and the order of the passes change no bit.
//
// One kernel, k_rs_resample, one pass over the source.  A block of 256 lanes owns a tile of tx x ty OUTPUT points and RS_ZCHUNK
// output planes; it walks the source planes its outputs need in ascending order.  Per source plane: rs_stage brings the samples
// the tile needs - only the rows and columns some output of the tile has a tap on - into LDS as doubles; rs_rows sums along x for
// those rows; rs_cols sums along y into one plane of a ring of ntaps[2] planes of doubles; when the ring holds the window of the
// next output plane, rs_emit sums along z, converts and stores.  A lane owns the same outputs of the tile in rs_cols and in
// rs_emit: nobody else reads its ring entries, and two barriers per source plane are all there is.
// The first part of this file - everything down to the line that says so - has no HIP in it: the functions are the kernel's whole
// arithmetic and indexing, taking the lane number as an argument, and tests/resample_host.cpp compiles this text with the host
// compiler, runs the phases lane by lane and is held to the oracle bit for bit.

#ifndef RS_HD
#define RS_HD __host__ __device__ __forceinline__
#endif

constexpr int RS_MAX_RADIUS = 8;
constexpr int RS_MAX_TAPS = 2 * RS_MAX_RADIUS + 1;
constexpr int RS_ZCHUNK = 64;        // output planes per block: a block recomputes 2 r[2] source planes of its neighbour below
constexpr int RS_THREADS = 256;
constexpr int RS_TILE_X = 32, RS_TILE_Y = 16;   // the tile of outputs when it fits RS_LDS_BUDGET (rs_plan halves ty, then tx, until it does)
constexpr size_t RS_LDS_BUDGET = 64u << 10;
constexpr int RS_TAP_WORDS = 52;     // 3 x 17 taps, rounded up to 16 bytes

// One axis.  The staged entries of a tile along this axis: with stride <= ntaps the windows of neighbouring outputs overlap or
// touch and the entries are the source points from the first output's first tap to the last output's last, once each; with a
// larger stride every output has its own ntaps entries and what lies between is never read.
struct RsAxis {
	long long n_src, n_out;
	int stride, ntaps, r;
	int step;            // min(stride, ntaps): entries between the windows of neighbouring outputs
};

struct RsPlan {
	RsAxis ax[3];
	int tx, ty;                      // outputs per tile
	int ncols, nrows;                // staged entries per tile along x, y
	long long tiles_x, tiles_y, chunks_z;
	size_t spitch, sslice, dpitch, dslice;   // in samples
	size_t lds_bytes;
};

RS_HD long long rs_clamp(long long i, long long n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
RS_HD int rs_extent(const RsAxis &a, int tile) { return (tile - 1) * a.step + a.ntaps; }
// the source point (clamped into the grid) of staged entry e of a tile whose first output is o0
RS_HD long long rs_source(const RsAxis &a, long long o0, int e) {
	long long u;
	if (a.stride <= a.ntaps) u = o0 * a.stride - a.r + e;
	else u = (o0 + e / a.ntaps) * a.stride + (e % a.ntaps) - a.r;
	return rs_clamp(u, a.n_src);
}
// a sum of the definition: the first product, then the others added in ascending tap order (nothing fused: -ffp-contract=off)
RS_HD double rs_sum(const double *w, int n, const double *v, int step) {
	double acc = w[0] * v[0];
	for (int i = 1; i < n; i++) acc = acc + w[i] * v[(size_t)i * step];
	return acc;
}

template <typename T> struct RsConvert;
template <> struct RsConvert<double> { static RS_HD double to(double v) { return v; } };
template <> struct RsConvert<float> { static RS_HD float to(double v) { return (float)v; } };
template <typename T> struct RsConvert {   // unsigned char / short / int
	static RS_HD T to(double v) {
		const double top = (double)(T)~(T)0;
		if (!(v > 0.0)) return (T)0;   // (a NaN too)
		if (v >= top) return (T)~(T)0;
		return (T)floor(v + 0.5);
	}
};

// LDS of a block, in doubles: taps[RS_TAP_WORDS] | raw[nrows][ncols] | sx[nrows][tx] | ring[ntaps z][ty][tx]
RS_HD size_t rs_lds_doubles(const RsPlan &p) {
	return (size_t)RS_TAP_WORDS + (size_t)p.nrows * p.ncols + (size_t)p.nrows * p.tx + (size_t)p.ax[2].ntaps * p.tx * p.ty;
}

// phase 1: the samples of source plane zsrc the tile needs, as doubles
template <typename T>
RS_HD void rs_stage(const RsPlan &p, const T *src, long long zsrc, long long X0, long long Y0, double *raw, int lane, int lanes) {
	const int n = p.nrows * p.ncols;
	const T *plane = src + (size_t)zsrc * p.sslice;
	for (int e = lane; e < n; e += lanes) {
		const int q = e / p.ncols, c = e - q * p.ncols;
		const long long y = rs_source(p.ax[1], Y0, q), x = rs_source(p.ax[0], X0, c);
		raw[e] = (double)plane[(size_t)y * p.spitch + (size_t)x];
	}
}
// What limits these phases is the number of LDS reads - a tap and a value per product when every sum is taken by itself - so a
// lane takes four sums side by side where it can: one read of the tap serves four products, and where the four windows overlap
// (rs_cols at stride 1) one read of a value does too.  Every sum still adds its own products in ascending tap order.
//
// phase 2: Sx for every staged row and every output column of the tile.  Consecutive lanes take consecutive columns (no bank
// conflict); a lane takes rows q, q + g, q + 2 g, q + 3 g with g = ceil(nrows / 4) and shares the taps between them.
RS_HD void rs_rows(const RsPlan &p, const double *taps, const double *raw, double *sx, int lane, int lanes) {
	const int g = (p.nrows + 3) / 4, n = g * p.tx, nt = p.ax[0].ntaps;
	for (int e = lane; e < n; e += lanes) {
		const int q = e / p.tx, xl = e - q * p.tx;
		// (a row beyond the last staged one is computed from row q again and not stored: no branch inside the loop)
		const int q1 = q + g < p.nrows ? q + g : q, q2 = q + 2 * g < p.nrows ? q + 2 * g : q, q3 = q + 3 * g < p.nrows ? q + 3 * g : q;
		const double *v0 = raw + (size_t)q * p.ncols + xl * p.ax[0].step, *v1 = raw + (size_t)q1 * p.ncols + xl * p.ax[0].step;
		const double *v2 = raw + (size_t)q2 * p.ncols + xl * p.ax[0].step, *v3 = raw + (size_t)q3 * p.ncols + xl * p.ax[0].step;
		double w = taps[0];
		double a0 = w * v0[0], a1 = w * v1[0], a2 = w * v2[0], a3 = w * v3[0];
		for (int i = 1; i < nt; i++) {
			w = taps[i];
			a0 = a0 + w * v0[i]; a1 = a1 + w * v1[i]; a2 = a2 + w * v2[i]; a3 = a3 + w * v3[i];
		}
		sx[(size_t)q * p.tx + xl] = a0;
		if (q1 != q) sx[(size_t)q1 * p.tx + xl] = a1;
		if (q2 != q) sx[(size_t)q2 * p.tx + xl] = a2;
		if (q3 != q) sx[(size_t)q3 * p.tx + xl] = a3;
	}
}
// phase 3: Sy of the tile into one plane of the ring.  With four rows of outputs or more a lane takes column xl of output rows
// yl .. yl + 3 (ty is a power of two): at stride 1 their windows are one run of ntaps + 3 values of Sx that slides through four
// registers; otherwise the four sums only share the taps.
RS_HD void rs_cols(const RsPlan &p, const double *taps, const double *sx, double *ring_plane, int lane, int lanes) {
	const int nt = p.ax[1].ntaps, step = p.ax[1].step;
	const double *wy = taps + RS_MAX_TAPS;
	if ((p.ty & 3) != 0) {   // tiles of one or two rows of outputs: every sum by itself
		const int n = p.tx * p.ty;
		for (int e = lane; e < n; e += lanes) {
			const int yl = e / p.tx, xl = e - yl * p.tx;
			ring_plane[e] = rs_sum(wy, nt, sx + (size_t)(yl * step) * p.tx + xl, p.tx);
		}
		return;
	}
	const int n = p.tx * (p.ty / 4);
	const size_t tx = (size_t)p.tx;
	for (int e = lane; e < n; e += lanes) {
		const int yg = e / p.tx, xl = e - yg * p.tx, yl = yg * 4;
		double a0, a1, a2, a3;
		if (step == 1) {
			const double *v = sx + (size_t)yl * tx + xl;   // v[k * tx]: Sx of staged row yl + k
			double v0 = v[0], v1 = v[tx], v2 = v[2 * tx], v3 = v[3 * tx], w = wy[0];
			a0 = w * v0; a1 = w * v1; a2 = w * v2; a3 = w * v3;
			for (int j = 1; j < nt; j++) {
				v0 = v1; v1 = v2; v2 = v3; v3 = v[(size_t)(j + 3) * tx];
				w = wy[j];
				a0 = a0 + w * v0; a1 = a1 + w * v1; a2 = a2 + w * v2; a3 = a3 + w * v3;
			}
		} else {
			const double *v0 = sx + (size_t)(yl * step) * tx + xl, *v1 = v0 + (size_t)step * tx, *v2 = v1 + (size_t)step * tx, *v3 = v2 + (size_t)step * tx;
			double w = wy[0];
			a0 = w * v0[0]; a1 = w * v1[0]; a2 = w * v2[0]; a3 = w * v3[0];
			for (int j = 1; j < nt; j++) {
				w = wy[j];
				a0 = a0 + w * v0[(size_t)j * tx]; a1 = a1 + w * v1[(size_t)j * tx]; a2 = a2 + w * v2[(size_t)j * tx]; a3 = a3 + w * v3[(size_t)j * tx];
			}
		}
		double *o = ring_plane + (size_t)yl * tx + xl;
		o[0] = a0; o[tx] = a1; o[2 * tx] = a2; o[3 * tx] = a3;
	}
}
// the ring plane of unclamped source plane u >= -r[2]
RS_HD int rs_ring_slot(const RsAxis &az, long long u) { return (int)((u + az.r) % az.ntaps); }
// phase 4: output plane Z of the tile from the ring (it holds planes Z * stride - r .. + r), converted and stored
template <typename T>
RS_HD void rs_emit(const RsPlan &p, const double *taps, const double *ring, long long Z, long long X0, long long Y0, T *dst, int lane, int lanes) {
	const int n = p.tx * p.ty, nt = p.ax[2].ntaps;
	const double *w = taps + 2 * RS_MAX_TAPS;
	const int s0 = rs_ring_slot(p.ax[2], Z * p.ax[2].stride - p.ax[2].r);
	if ((p.ty & 3) != 0) {
		for (int e = lane; e < n; e += lanes) {
			int s = s0;
			double acc = w[0] * ring[(size_t)s * n + e];
			for (int k = 1; k < nt; k++) {
				s = s + 1 == nt ? 0 : s + 1;
				acc = acc + w[k] * ring[(size_t)s * n + e];
			}
			const int yl = e / p.tx, xl = e - yl * p.tx;
			const long long X = X0 + xl, Y = Y0 + yl;
			if (X < p.ax[0].n_out && Y < p.ax[1].n_out) dst[(size_t)Z * p.dslice + (size_t)Y * p.dpitch + (size_t)X] = RsConvert<T>::to(acc);
		}
		return;
	}
	// the four outputs whose ring entries this lane wrote in rs_cols; the taps are read once for the four
	const int ng = p.tx * (p.ty / 4);
	const size_t tx = (size_t)p.tx;
	for (int e = lane; e < ng; e += lanes) {
		const int yg = e / p.tx, xl = e - yg * p.tx, yl = yg * 4;
		const double *v = ring + (size_t)yl * tx + xl;
		int s = s0;
		double wk = w[0];
		double a0 = wk * v[(size_t)s * n], a1 = wk * v[(size_t)s * n + tx], a2 = wk * v[(size_t)s * n + 2 * tx], a3 = wk * v[(size_t)s * n + 3 * tx];
		for (int k = 1; k < nt; k++) {
			s = s + 1 == nt ? 0 : s + 1;
			wk = w[k];
			const double *u = v + (size_t)s * n;
			a0 = a0 + wk * u[0]; a1 = a1 + wk * u[tx]; a2 = a2 + wk * u[2 * tx]; a3 = a3 + wk * u[3 * tx];
		}
		const double a[4] = {a0, a1, a2, a3};
		const long long X = X0 + xl;
		for (int k = 0; k < 4; k++) {   // (unrolled: a[] stays in registers)
			const long long Y = Y0 + yl + k;
			if (X < p.ax[0].n_out && Y < p.ax[1].n_out) dst[(size_t)Z * p.dslice + (size_t)Y * p.dpitch + (size_t)X] = RsConvert<T>::to(a[k]);
		}
	}
}

// one axis of the plan from its three numbers (checked by the caller: ntaps odd, 1 .. 17; stride >= 1)
static inline void rs_axis(RsAxis &ax, long long n_src, int ntaps, int stride) {
	ax.ntaps = ntaps;
	ax.r = (ntaps - 1) / 2;
	ax.stride = stride;
	ax.step = stride < ntaps ? stride : ntaps;
	ax.n_src = n_src;
	ax.n_out = (n_src - 1) / stride + 1;
}

// the tile and what it stages: the largest of 32 x 16, 32 x 8, ... 32 x 1, 16 x 1, ... whose LDS fits the budget
static inline void rs_plan_tiles(RsPlan &p) {
	p.tx = RS_TILE_X; p.ty = RS_TILE_Y;
	for (;;) {
		p.ncols = rs_extent(p.ax[0], p.tx); p.nrows = rs_extent(p.ax[1], p.ty);
		p.lds_bytes = rs_lds_doubles(p) * sizeof(double);
		if (p.lds_bytes <= RS_LDS_BUDGET || (p.tx == 1 && p.ty == 1)) break;
		if (p.ty > 1) p.ty /= 2; else p.tx /= 2;
	}
	p.tiles_x = (p.ax[0].n_out + p.tx - 1) / p.tx;
	p.tiles_y = (p.ax[1].n_out + p.ty - 1) / p.ty;
	p.chunks_z = (p.ax[2].n_out + RS_ZCHUNK - 1) / RS_ZCHUNK;
}

// ---- everything above compiles without HIP (tests/resample_host.cpp) ---------------------------------------------------------------
#ifdef __HIPCC__

struct ResampleState {       // scratch of the resampling: on the MeasureState from the first call on, freed with it
	double *d_taps;          // [RS_TAP_WORDS]: taps[a][i] at a * RS_MAX_TAPS + i
};

// The hot path.  blockIdx.x counts (tile x, tile y, z chunk), x fastest: neighbouring blocks share the halo columns they stage.
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void k_rs_resample(const T *__restrict__ src, T *__restrict__ dst, const double *__restrict__ d_taps, RsPlan p) {
	extern __shared__ double rs_lds[];
	double *taps = rs_lds, *raw = taps + RS_TAP_WORDS, *sx = raw + (size_t)p.nrows * p.ncols, *ring = sx + (size_t)p.nrows * p.tx;
	const int lane = (int)threadIdx.x;
	long long b = blockIdx.x;
	const long long bx = b % p.tiles_x; b /= p.tiles_x;
	const long long by = b % p.tiles_y, bz = b / p.tiles_y;
	const long long X0 = bx * p.tx, Y0 = by * p.ty, Z0 = bz * RS_ZCHUNK;
	const long long Z1 = Z0 + RS_ZCHUNK < p.ax[2].n_out ? Z0 + RS_ZCHUNK : p.ax[2].n_out;
	if (lane < RS_TAP_WORDS) taps[lane] = d_taps[lane];
	__syncthreads();
	const RsAxis az = p.ax[2];
	const size_t plane = (size_t)p.tx * p.ty;
	long long next_u = Z0 * az.stride - az.r;   // the first source plane (unclamped) not yet in the ring
	for (long long Z = Z0; Z < Z1; Z++) {       // (block-uniform loops: every lane meets every barrier)
		const long long lo = Z * az.stride - az.r, hi = lo + az.ntaps - 1;
		for (long long u = next_u > lo ? next_u : lo; u <= hi; u++) {
			rs_stage(p, src, rs_clamp(u, az.n_src), X0, Y0, raw, lane, RS_THREADS);
			__syncthreads();
			rs_rows(p, taps, raw, sx, lane, RS_THREADS);
			__syncthreads();
			rs_cols(p, taps, sx, ring + (size_t)rs_ring_slot(az, u) * plane, lane, RS_THREADS);
		}
		next_u = hi + 1;
		rs_emit(p, taps, ring, Z, X0, Y0, dst, lane, RS_THREADS);
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void rs_release(void *state) { dev_release(&((ResampleState *)state)->d_taps); }

// arguments -> plan and taps; MC33HIP_EINVAL with the reason in mc33hip_last_error
static int rs_check(mc33hip_ctx *c, const mc33hip_resampling *r, RsPlan &p, double taps[RS_TAP_WORDS]) {
	if (!c || !r) return MC33HIP_EINVAL;
	const mc33hip_grid_desc &d = c->desc;
	if (d.plane0 != 0u || d.npz_resident != d.nz_total + 1u) { set_err("the context holds a z-slab: only a whole grid is resampled"); return MC33HIP_EINVAL; }
	const unsigned np[3] = {d.npx, d.npy, d.npz_resident};
	memset(&p, 0, sizeof p);
	for (int k = 0; k < RS_TAP_WORDS; k++) taps[k] = 0.0;
	for (int a = 0; a < 3; a++) {
		RsAxis &ax = p.ax[a];
		int ntaps = 1;
		if (!r->taps[a]) taps[a * RS_MAX_TAPS] = 1.0;
		else {
			if (!(r->ntaps[a] & 1u) || r->ntaps[a] > (unsigned)RS_MAX_TAPS) { set_err("ntaps[%d] = %u: an odd number up to %d", a, r->ntaps[a], RS_MAX_TAPS); return MC33HIP_EINVAL; }
			ntaps = (int)r->ntaps[a];
			for (int i = 0; i < ntaps; i++) {
				const double w = r->taps[a][i];
				if (!(w > -__builtin_huge_val() && w < __builtin_huge_val())) { set_err("taps[%d][%d] is not finite", a, i); return MC33HIP_EINVAL; }
				taps[a * RS_MAX_TAPS + i] = w;
			}
		}
		if (r->stride[a] < 1u || r->stride[a] > 0x7FFFFFFFu) { set_err("stride[%d] = %u", a, r->stride[a]); return MC33HIP_EINVAL; }
		rs_axis(ax, np[a], ntaps, (int)r->stride[a]);
		if (ax.n_out < 2) { set_err("stride[%d] = %u leaves %lld points of %u: an axis needs 2", a, r->stride[a], ax.n_out, np[a]); return MC33HIP_EINVAL; }
	}
	return 0;
}

extern "C" int mc33hip_resampled_size(mc33hip_ctx *c, const mc33hip_resampling *r, unsigned np_out[3]) {
	if (!np_out) return MC33HIP_EINVAL;
	RsPlan p;
	double taps[RS_TAP_WORDS];
	int rc = rs_check(c, r, p, taps);
	if (rc) return rc;
	for (int a = 0; a < 3; a++) np_out[a] = (unsigned)p.ax[a].n_out;
	return MC33HIP_OK;
}

extern "C" int mc33hip_resample_grid(mc33hip_ctx *c, const mc33hip_resampling *r, void *dst, size_t pitch, size_t slice) {
	RsPlan p;
	double taps[RS_TAP_WORDS];
	int rc = rs_check(c, r, p, taps);
	if (rc) return rc;
	if (!dst) return MC33HIP_EINVAL;
	if (!c->d_grid) { set_err("no grid is resident in this context"); return MC33HIP_EINVAL; }
	if (pitch < (size_t)p.ax[0].n_out || slice / pitch < (size_t)p.ax[1].n_out) { set_err("pitch %zu / slice %zu too small for %lld x %lld points", pitch, slice, p.ax[0].n_out, p.ax[1].n_out); return MC33HIP_EINVAL; }
	// not in place: the bytes from the first to the last grid point of either grid must not meet
	const uint64_t src_bytes = (((uint64_t)p.ax[2].n_src - 1u) * c->slice + ((uint64_t)p.ax[1].n_src - 1u) * c->pitch + (uint64_t)p.ax[0].n_src) * sizeof(sample_t);
	const uint64_t dst_bytes = (((uint64_t)p.ax[2].n_out - 1u) * slice + ((uint64_t)p.ax[1].n_out - 1u) * pitch + (uint64_t)p.ax[0].n_out) * sizeof(sample_t);
	if (mesh_ranges_meet(c->d_grid, src_bytes, dst, dst_bytes)) { set_err("dst overlaps the source grid: the resampling is not in place"); return MC33HIP_EINVAL; }
	p.spitch = c->pitch; p.sslice = c->slice; p.dpitch = pitch; p.dslice = slice;
	rs_plan_tiles(p);
	const long long blocks = p.tiles_x * p.tiles_y * p.chunks_z;
	if (blocks > 0x7FFFFFFFll) { set_err("%lld tiles: more than a launch takes", blocks); return MC33HIP_EINVAL; }
	if ((rc = use_device(c))) return rc;
	if ((rc = meas_state(c))) return rc;
	MeshOp *op;
	if ((rc = mesh_op_find(&c->meas->mesh, rs_release, sizeof(ResampleState), &op))) return rc;
	ResampleState *s = (ResampleState *)op->state;
	if (!s->d_taps) HIP_TRY(hipMalloc(&s->d_taps, RS_TAP_WORDS * sizeof(double)));
	// (the taps are in pageable host memory: the copy has left it when the call returns, and is ordered on the stream)
	HIP_TRY(hipMemcpyAsync(s->d_taps, taps, RS_TAP_WORDS * sizeof(double), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL((k_rs_resample<sample_t>), dim3((uint32_t)blocks), dim3(RS_THREADS), p.lds_bytes, c->stream, (const sample_t *)c->d_grid, (sample_t *)dst,
	                   (const double *)s->d_taps, p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c->stream));
	return MC33HIP_OK;
}

extern "C" int mc33hip_context_device(mc33hip_ctx *c) { return c ? c->device : MC33HIP_EINVAL; }

// the other way from the resident grid to a second device grid, behind this one in the translation unit: rank windows
#include "mc33_rank.hip.h"

#endif  // __HIPCC__
