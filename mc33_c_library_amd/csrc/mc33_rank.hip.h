// mc33_rank.hip.h -- part of the ONE translation unit mc33_kernels.hip (included at the end of mc33_resample.hip.h; not a header
// to include elsewhere): the resident grid rank-filtered into a second device grid before anything is extracted from it - the minimum,
// the median or the maximum of a box window, edge samples replicated (include/mc33_hip.h: mc33hip_rank_grid).  DESIGN.md 26.
//
// The definition is in include/mc33_hip.h; tests/rank_oracle.py restates it in numpy.  A rank filter selects one of its inputs:
// everything here works on KEYS - unsigned integers whose order is the definition's - made once when a sample is staged and turned
// back into the sample's bytes on store.  Only unsigned integer comparisons decide anything.  1-, 2- and 4-byte samples share the
// 32-bit key code, doubles have 64-bit keys.  MIN is MAX on complemented keys (rk_flip), so there is one code path for the two.
//
// Two kernels, each one pass over the source and one write of the output, built like k_rs_resample: a block of 256
// lanes owns a tile of tx x ty outputs and RK_ZCHUNK output planes and marches along z over the source planes it needs, each once.
//   k_rk_minmax  per source plane: rk_put leaves the keys of the tile and its halo in LDS; rk_rows takes the maximum along x for
//                every staged row, rk_cols along y into one plane of a ring of 2 r[2] + 1 planes, rk_emit_max along z out of the
//                ring (the box maximum is the composition of the three, exactly: every step is a selection).  A lane owns the same
//                outputs in rk_cols and rk_emit_max: two barriers per plane.
//   k_rk_median  the ring holds the staged key planes themselves, 1 or 3 of them.  With three, rk_sort_columns sorts the three keys
//                of every staged z-column once - a sorted column serves the nine windows it lies in - and rk_emit_median selects
//                from the sorted columns of a window in registers (rk_median_sorted: of 27 keys 14 are dropped by their place in
//                their column, the median of the 13 left comes from a selection network that forgets); with one plane it selects
//                among the 1, 3 or 9 keys of the window directly.
// In both, rk_fetch loads the NEXT plane's samples into registers (RK_FETCH per lane) right after the barrier that publishes the
// current one: the loads are in flight while the current plane is worked on - what DESIGN.md 15 names as the remedy for its own
// kernel's load - barrier - work chain.
// The first part of this file - everything down to the line that says so - has no HIP in it: the functions are the kernels' whole
// selection and indexing, taking the lane number as an argument, and tests/rank_host.cpp compiles this text with the host
// compiler, runs the phases lane by lane and is held to the oracle bit for bit.

#ifndef RK_HD
#define RK_HD __host__ __device__ __forceinline__
#endif
#if defined(__clang__)
#define RK_UNROLL _Pragma("unroll")
#else
#define RK_UNROLL _Pragma("GCC unroll 32")
#endif

constexpr int RK_RANK_MIN = 0, RK_RANK_MEDIAN = 1, RK_RANK_MAX = 2;   // MC33HIP_RANK_* (include/mc33_hip.h)
constexpr int RK_MINMAX_RADIUS = 8, RK_MEDIAN_RADIUS = 1;
constexpr int RK_ZCHUNK = 64;        // output planes per block: a block stages 2 r[2] source planes of its neighbours again
constexpr int RK_THREADS = 256;
constexpr int RK_TILE_X = 64, RK_TILE_Y = 16;   // the tile of outputs when it fits RK_LDS_BUDGET (rk_plan_tiles halves ty, then tx, until it does)
constexpr int RK_FETCH = 10;         // staged keys per lane and plane at most: (64 + 16) x (16 + 16) / 256
constexpr size_t RK_LDS_BUDGET = 64u << 10;

struct RkPlan {
	long long n[3];                  // grid points per axis
	int r[3];                        // radius per axis
	int rank;                        // RK_RANK_*
	int tx, ty;                      // outputs per tile
	int ncols, nrows;                // staged entries per tile along x, y: tx + 2 r[0], ty + 2 r[1]
	int woff[9];                     // median: the window's in-plane offsets in a staged plane, x fastest
	long long tiles_x, tiles_y, chunks_z;
	size_t spitch, sslice, dpitch, dslice;   // in samples
	size_t lds_keys;
};

// sample <-> key.  The primary template is the three unsigned integer types: the value itself.
template <typename T> struct RkKey {
	typedef uint32_t K;
	static RK_HD K to(T v) { return (K)v; }
	static RK_HD T from(K k) { return (T)k; }
};
template <> struct RkKey<float> {
	typedef uint32_t K;
	static RK_HD K to(float v) { K b; __builtin_memcpy(&b, &v, sizeof b); return (b >> 31) ? ~b : (b | 0x80000000u); }
	static RK_HD float from(K k) { const K b = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k; float v; __builtin_memcpy(&v, &b, sizeof v); return v; }
};
template <> struct RkKey<double> {
	typedef uint64_t K;
	static RK_HD K to(double v) { K b; __builtin_memcpy(&b, &v, sizeof b); return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
	static RK_HD double from(K k) { const K b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k; double v; __builtin_memcpy(&v, &b, sizeof v); return v; }
};

RK_HD long long rk_clamp(long long i, long long n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// MIN is MAX on complemented keys: staged keys are key ^ rk_flip, the store undoes it
template <typename K> RK_HD K rk_flip(const RkPlan &p) { return p.rank == RK_RANK_MIN ? (K) ~(K)0 : (K)0; }
template <typename K> RK_HD K rk_max(K a, K b) { return a > b ? a : b; }
template <typename K> RK_HD void rk_ce(K &a, K &b) { const K lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }
// the ring plane of unclamped source plane u >= -r[2]
RK_HD int rk_slot(const RkPlan &p, long long u) { return (int)((u + p.r[2]) % (2 * p.r[2] + 1)); }

// LDS of a block, in keys.  min / max: raw[nrows][ncols] | sx[nrows][tx] | ring[2 r2 + 1][ty][tx]; median: ring[2 r2 + 1][nrows][ncols]
// and, with r2 = 1, sorted[3][nrows][ncols] behind it
RK_HD size_t rk_lds_keys(const RkPlan &p) {
	const size_t staged = (size_t)p.nrows * p.ncols, nz = 2 * (size_t)p.r[2] + 1;
	return p.rank == RK_RANK_MEDIAN ? (nz + (p.r[2] ? 3 : 0)) * staged : staged + (size_t)p.nrows * p.tx + nz * p.tx * p.ty;
}

// phase 1a: the samples of source plane zsrc the tile needs - its outputs and a halo of r[0], r[1], clamped into the grid - as
// keys in the lane's registers: entry e = lane + i * lanes of the staged plane in regs[i]
template <typename T>
RK_HD void rk_fetch(const RkPlan &p, const T *src, long long zsrc, long long X0, long long Y0, typename RkKey<T>::K *regs, int lane, int lanes) {
	typedef typename RkKey<T>::K K;
	const int n = p.nrows * p.ncols;
	const K flip = rk_flip<K>(p);
	const T *plane = src + (size_t)zsrc * p.sslice;
	RK_UNROLL
	for (int i = 0; i < RK_FETCH; i++) {
		const int e = lane + i * lanes;
		if (e < n) {
			const int q = e / p.ncols, c = e - q * p.ncols;
			const long long y = rk_clamp(Y0 - p.r[1] + q, p.n[1]), x = rk_clamp(X0 - p.r[0] + c, p.n[0]);
			regs[i] = RkKey<T>::to(plane[(size_t)y * p.spitch + (size_t)x]) ^ flip;
		}
	}
}
// phase 1b: ... from the registers into a staged plane in LDS
template <typename K>
RK_HD void rk_put(const RkPlan &p, const K *regs, K *staged, int lane, int lanes) {
	const int n = p.nrows * p.ncols;
	RK_UNROLL
	for (int i = 0; i < RK_FETCH; i++) {
		const int e = lane + i * lanes;
		if (e < n) staged[e] = regs[i];
	}
}

// min / max, phase 2: the maximum along x for every staged row and every output column (consecutive lanes, consecutive columns)
template <typename K>
RK_HD void rk_rows(const RkPlan &p, const K *raw, K *sx, int lane, int lanes) {
	const int n = p.nrows * p.tx, nt = 2 * p.r[0] + 1;
	for (int e = lane; e < n; e += lanes) {
		const int q = e / p.tx, xl = e - q * p.tx;
		const K *v = raw + (size_t)q * p.ncols + xl;
		K m = v[0];
		for (int i = 1; i < nt; i++) m = rk_max(m, v[i]);
		sx[e] = m;
	}
}
// phase 3: ... along y, into one plane of the ring
template <typename K>
RK_HD void rk_cols(const RkPlan &p, const K *sx, K *ring_plane, int lane, int lanes) {
	const int n = p.tx * p.ty, nt = 2 * p.r[1] + 1;
	for (int e = lane; e < n; e += lanes) {
		const K *v = sx + e;   // staged rows yl .. yl + 2 r[1] of column xl: e = yl * tx + xl
		K m = v[0];
		for (int j = 1; j < nt; j++) m = rk_max(m, v[(size_t)j * p.tx]);
		ring_plane[e] = m;
	}
}
// phase 4: output plane Z from the ring (it holds planes Z - r[2] .. Z + r[2]; a maximum needs no order), turned back and stored
template <typename T>
RK_HD void rk_emit_max(const RkPlan &p, const typename RkKey<T>::K *ring, long long Z, long long X0, long long Y0, T *dst, int lane, int lanes) {
	typedef typename RkKey<T>::K K;
	const int n = p.tx * p.ty, nt = 2 * p.r[2] + 1;
	const K flip = rk_flip<K>(p);
	for (int e = lane; e < n; e += lanes) {
		K m = ring[e];
		for (int k = 1; k < nt; k++) m = rk_max(m, ring[(size_t)k * n + e]);
		const int yl = e / p.tx, xl = e - yl * p.tx;
		const long long X = X0 + xl, Y = Y0 + yl;
		if (X < p.n[0] && Y < p.n[1]) dst[(size_t)Z * p.dslice + (size_t)Y * p.dpitch + (size_t)X] = RkKey<T>::from(m ^ flip);
	}
}

// The median of N keys held in registers: a selection network that forgets.  Of any N / 2 + 2 elements the smallest has more than
// half of the N at or above it and the largest more than half at or below it: neither is the median, and without the two the
// median of the rest is the same.  So the network holds N / 2 + 2 keys, moves the smallest and the largest of them to the ends
// (compare-exchanges; the others stay unordered), drops both and takes one more key, until three are left.  Everything is
// unrolled: v[] are registers.
template <int N, typename K>
RK_HD K rk_median_of(const K *w) {
	if constexpr (N == 1) return w[0];
	else {
		constexpr int M = N / 2 + 2;
		K v[M];
		RK_UNROLL
		for (int i = 0; i < M; i++) v[i] = w[i];
		RK_UNROLL
		for (int live = M; live >= 3; live--) {
			RK_UNROLL
			for (int i = 1; i < live; i++) rk_ce(v[0], v[i]);              // v[0]: the smallest
			RK_UNROLL
			for (int i = 1; i < live - 1; i++) rk_ce(v[i], v[live - 1]);   // v[live - 1]: the largest
			if (live > 3) v[0] = w[M + (M - live)];                        // (v[live - 1] is beyond the next round)
		}
		return v[1];
	}
}
template <typename K> RK_HD K rk_min(K a, K b) { return a < b ? a : b; }
template <typename K> RK_HD K rk_med3(K a, K b, K c) { return rk_max(rk_min(a, b), rk_min(rk_max(a, b), c)); }
// nine keys in ascending order: the 25 compare-exchanges of the smallest known network for nine (what of it feeds no key that is
// used afterwards, the compiler drops)
template <typename K>
RK_HD void rk_sort9(K *v) {
	rk_ce(v[0], v[3]); rk_ce(v[1], v[7]); rk_ce(v[2], v[5]); rk_ce(v[4], v[8]);
	rk_ce(v[0], v[7]); rk_ce(v[2], v[4]); rk_ce(v[3], v[8]); rk_ce(v[5], v[6]);
	rk_ce(v[0], v[2]); rk_ce(v[1], v[3]); rk_ce(v[4], v[5]); rk_ce(v[7], v[8]);
	rk_ce(v[1], v[4]); rk_ce(v[3], v[6]); rk_ce(v[5], v[7]);
	rk_ce(v[0], v[1]); rk_ce(v[2], v[4]); rk_ce(v[3], v[5]); rk_ce(v[6], v[8]);
	rk_ce(v[2], v[3]); rk_ce(v[4], v[5]); rk_ce(v[6], v[7]);
	rk_ce(v[1], v[2]); rk_ce(v[3], v[4]); rk_ce(v[5], v[6]);
}
// The median of NXY z-columns of three keys that rk_sort_columns has sorted: lo <= mid <= hi per column, at lo[off[j]] and so on.
// One column: its mid.  Three columns: the median of the largest lo, the median mid and the smallest hi (the 3 x 3 rule of the
// sorted columns).  Nine columns, 27 keys, the median has 13 on either side.  The k-th smallest lo (k = 0 ..) has 8 - k lo at or
// above it and mid and hi of those columns and of its own, 26 - 3 k keys: 14 or more for k <= 4, so the five smallest lo lie below
// the median, and likewise the five largest hi above it.  The k-th smallest mid has 17 - 2 k keys at or above it: the two smallest
// mid lie below the median, the two largest above.  Seven keys are dropped on either side, and the median of the 27 is the median
// of the 13 left: the four largest lo, the five middle mid, the four smallest hi.
template <int NXY, typename K>
RK_HD K rk_median_sorted(const K *lo, const K *mid, const K *hi, const int *off) {
	if constexpr (NXY == 1) return mid[off[0]];
	else if constexpr (NXY == 3)
		return rk_med3(rk_max(rk_max(lo[off[0]], lo[off[1]]), lo[off[2]]), rk_med3(mid[off[0]], mid[off[1]], mid[off[2]]),
		               rk_min(rk_min(hi[off[0]], hi[off[1]]), hi[off[2]]));
	else {
		K v[9], w[13];
		RK_UNROLL
		for (int j = 0; j < 9; j++) v[j] = lo[off[j]];
		rk_sort9(v);
		w[0] = v[5]; w[1] = v[6]; w[2] = v[7]; w[3] = v[8];
		RK_UNROLL
		for (int j = 0; j < 9; j++) v[j] = mid[off[j]];
		rk_sort9(v);
		w[4] = v[2]; w[5] = v[3]; w[6] = v[4]; w[7] = v[5]; w[8] = v[6];
		RK_UNROLL
		for (int j = 0; j < 9; j++) v[j] = hi[off[j]];
		rk_sort9(v);
		w[9] = v[0]; w[10] = v[1]; w[11] = v[2]; w[12] = v[3];
		return rk_median_of<13, K>(w);
	}
}
// median with r[2] = 1, phase 2: the three keys of every staged z-column of output plane Z (the ring holds planes Z - 1, Z, Z + 1)
// in ascending order, into three planes behind the ring: lo | mid | hi.  A sorted column serves the nine windows it lies in.
template <typename K>
RK_HD void rk_sort_columns(const RkPlan &p, const K *ring, long long Z, K *sorted, int lane, int lanes) {
	const int n = p.nrows * p.ncols;
	const K *b0 = ring + (size_t)rk_slot(p, Z - 1) * n, *b1 = ring + (size_t)rk_slot(p, Z) * n, *b2 = ring + (size_t)rk_slot(p, Z + 1) * n;
	for (int e = lane; e < n; e += lanes) {
		K a = b0[e], b = b1[e], c = b2[e];
		rk_ce(a, b); rk_ce(b, c); rk_ce(a, b);
		sorted[e] = a; sorted[(size_t)n + e] = b; sorted[2 * (size_t)n + e] = c;
	}
}
// median, last phase: output plane Z of the tile, turned back and stored - with NZ == 1 from the one staged plane in the ring,
// with NZ == 3 from the sorted columns
template <typename T, int NXY, int NZ>
RK_HD void rk_emit_median(const RkPlan &p, const typename RkKey<T>::K *planes, long long Z, long long X0, long long Y0, T *dst, int lane, int lanes) {
	typedef typename RkKey<T>::K K;
	const int n = p.tx * p.ty;
	const size_t staged = (size_t)p.nrows * p.ncols;
	for (int e = lane; e < n; e += lanes) {
		const int yl = e / p.tx, xl = e - yl * p.tx;
		const K *at = planes + (size_t)yl * p.ncols + xl;   // the window's first staged entry
		K m;
		if constexpr (NZ == 3) m = rk_median_sorted<NXY, K>(at, at + staged, at + 2 * staged, p.woff);
		else {
			K w[NXY];
			RK_UNROLL
			for (int j = 0; j < NXY; j++) w[j] = at[p.woff[j]];
			m = rk_median_of<NXY, K>(w);
		}
		const long long X = X0 + xl, Y = Y0 + yl;
		if (X < p.n[0] && Y < p.n[1]) dst[(size_t)Z * p.dslice + (size_t)Y * p.dpitch + (size_t)X] = RkKey<T>::from(m);
	}
}

// the tile and what it stages: the largest of 64 x 16, 64 x 8, ... 64 x 1, 32 x 1, ... whose LDS fits the budget
// (key_bytes: 4, or 8 for doubles; the radii, the rank and n[] are set and checked by the caller)
static inline void rk_plan_tiles(RkPlan &p, size_t key_bytes) {
	p.tx = RK_TILE_X; p.ty = RK_TILE_Y;
	for (;;) {
		p.ncols = p.tx + 2 * p.r[0]; p.nrows = p.ty + 2 * p.r[1];
		p.lds_keys = rk_lds_keys(p);
		if (p.lds_keys * key_bytes <= RK_LDS_BUDGET || (p.tx == 1 && p.ty == 1)) break;
		if (p.ty > 1) p.ty /= 2; else p.tx /= 2;
	}
	const int nx = 2 * p.r[0] + 1, ny = 2 * p.r[1] + 1;
	for (int j = 0; j < 9; j++) p.woff[j] = 0;
	if (p.rank == RK_RANK_MEDIAN)
		for (int j = 0; j < nx * ny; j++) p.woff[j] = (j / nx) * p.ncols + j % nx;
	p.tiles_x = (p.n[0] + p.tx - 1) / p.tx;
	p.tiles_y = (p.n[1] + p.ty - 1) / p.ty;
	p.chunks_z = (p.n[2] + RK_ZCHUNK - 1) / RK_ZCHUNK;
}
// what mc33hip_rank_grid refuses of the struct (the limits of include/mc33_hip.h)
static inline bool rk_accepts(int rank, const unsigned radius[3]) {
	if (rank != RK_RANK_MIN && rank != RK_RANK_MEDIAN && rank != RK_RANK_MAX) return false;
	const unsigned top = rank == RK_RANK_MEDIAN ? (unsigned)RK_MEDIAN_RADIUS : (unsigned)RK_MINMAX_RADIUS;
	return radius[0] <= top && radius[1] <= top && radius[2] <= top;
}

// ---- everything above compiles without HIP (tests/rank_host.cpp) -------------------------------------------------------------------
#ifdef __HIPCC__

// The hot paths.  blockIdx.x counts (tile x, tile y, z chunk), x fastest: neighbouring blocks share the halo columns they stage.
struct RkBlock { long long X0, Y0, Z0, Z1; };
static __device__ __forceinline__ RkBlock rk_block(const RkPlan &p) {
	long long b = blockIdx.x;
	const long long bx = b % p.tiles_x; b /= p.tiles_x;
	const long long by = b % p.tiles_y, bz = b / p.tiles_y;
	RkBlock k;
	k.X0 = bx * p.tx; k.Y0 = by * p.ty; k.Z0 = bz * RK_ZCHUNK;
	k.Z1 = k.Z0 + RK_ZCHUNK < p.n[2] ? k.Z0 + RK_ZCHUNK : p.n[2];
	return k;
}

template <typename T>
__global__ __launch_bounds__(RK_THREADS) void k_rk_minmax(const T *__restrict__ src, T *__restrict__ dst, RkPlan p) {
	typedef typename RkKey<T>::K K;
	extern __shared__ unsigned long long rk_lds[];
	K *raw = (K *)rk_lds, *sx = raw + (size_t)p.nrows * p.ncols, *ring = sx + (size_t)p.nrows * p.tx;
	const int lane = (int)threadIdx.x;
	const RkBlock k = rk_block(p);
	const size_t plane = (size_t)p.tx * p.ty;
	const long long u0 = k.Z0 - p.r[2], u1 = k.Z1 - 1 + p.r[2];   // the source planes of the chunk, unclamped
	K regs[RK_FETCH];
	rk_fetch(p, src, rk_clamp(u0, p.n[2]), k.X0, k.Y0, regs, lane, RK_THREADS);
	for (long long u = u0; u <= u1; u++) {   // (block-uniform: every lane meets every barrier)
		rk_put(p, regs, raw, lane, RK_THREADS);
		__syncthreads();
		if (u < u1) rk_fetch(p, src, rk_clamp(u + 1, p.n[2]), k.X0, k.Y0, regs, lane, RK_THREADS);   // in flight while this plane is worked on
		rk_rows(p, raw, sx, lane, RK_THREADS);
		__syncthreads();
		rk_cols(p, sx, ring + (size_t)rk_slot(p, u) * plane, lane, RK_THREADS);
		if (u - p.r[2] >= k.Z0) rk_emit_max(p, ring, u - p.r[2], k.X0, k.Y0, dst, lane, RK_THREADS);
	}
}

template <typename T, int NXY, int NZ>
__global__ __launch_bounds__(RK_THREADS) void k_rk_median(const T *__restrict__ src, T *__restrict__ dst, RkPlan p) {
	typedef typename RkKey<T>::K K;
	extern __shared__ unsigned long long rk_lds[];
	K *ring = (K *)rk_lds;
	const int lane = (int)threadIdx.x;
	const RkBlock k = rk_block(p);
	const size_t staged = (size_t)p.nrows * p.ncols;
	K *sorted = ring + NZ * staged;
	const long long u0 = k.Z0 - p.r[2], u1 = k.Z1 - 1 + p.r[2];
	K regs[RK_FETCH];
	rk_fetch(p, src, rk_clamp(u0, p.n[2]), k.X0, k.Y0, regs, lane, RK_THREADS);
	for (long long u = u0; u <= u1; u++) {
		// (the plane this one overwrites was last read before the second barrier of the step before - by rk_sort_columns, or, with
		// NZ == 1, never after the barrier below)
		if (NZ == 1) __syncthreads();
		rk_put(p, regs, ring + (size_t)rk_slot(p, u) * staged, lane, RK_THREADS);
		__syncthreads();
		if (u < u1) rk_fetch(p, src, rk_clamp(u + 1, p.n[2]), k.X0, k.Y0, regs, lane, RK_THREADS);   // in flight while this plane is worked on
		if (u - p.r[2] < k.Z0) continue;   // (block-uniform)
		if (NZ == 3) {
			rk_sort_columns(p, ring, u - 1, sorted, lane, RK_THREADS);   // (the step before has read `sorted` before the barrier above)
			__syncthreads();
			rk_emit_median<T, NXY, NZ>(p, sorted, u - 1, k.X0, k.Y0, dst, lane, RK_THREADS);
		} else rk_emit_median<T, NXY, NZ>(p, ring, u, k.X0, k.Y0, dst, lane, RK_THREADS);
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

extern "C" int mc33hip_rank_grid(mc33hip_ctx *c, const mc33hip_ranking *r, void *dst, size_t pitch, size_t slice) {
	if (!c || !r || !dst) return MC33HIP_EINVAL;
	static_assert(RK_RANK_MIN == MC33HIP_RANK_MIN && RK_RANK_MEDIAN == MC33HIP_RANK_MEDIAN && RK_RANK_MAX == MC33HIP_RANK_MAX, "the ranks of mc33_hip.h");
	const mc33hip_grid_desc &d = c->desc;
	if (d.plane0 != 0u || d.npz_resident != d.nz_total + 1u) { set_err("the context holds a z-slab: only a whole grid is rank-filtered"); return MC33HIP_EINVAL; }
	if (!rk_accepts(r->rank, r->radius)) {
		set_err("rank %d with radius %u, %u, %u: MIN (0) and MAX (2) up to %d per axis, MEDIAN (1) up to %d", r->rank, r->radius[0], r->radius[1], r->radius[2], RK_MINMAX_RADIUS, RK_MEDIAN_RADIUS);
		return MC33HIP_EINVAL;
	}
	if (!c->d_grid) { set_err("no grid is resident in this context"); return MC33HIP_EINVAL; }
	if (pitch < (size_t)d.npx || slice / pitch < (size_t)d.npy) { set_err("pitch %zu / slice %zu too small for %u x %u points", pitch, slice, d.npx, d.npy); return MC33HIP_EINVAL; }
	// not in place: the bytes from the first to the last grid point of either grid must not meet
	const uint64_t src_bytes = (((uint64_t)d.npz_resident - 1u) * c->slice + ((uint64_t)d.npy - 1u) * c->pitch + (uint64_t)d.npx) * sizeof(sample_t);
	const uint64_t dst_bytes = (((uint64_t)d.npz_resident - 1u) * slice + ((uint64_t)d.npy - 1u) * pitch + (uint64_t)d.npx) * sizeof(sample_t);
	if (mesh_ranges_meet(c->d_grid, src_bytes, dst, dst_bytes)) { set_err("dst overlaps the source grid: the rank filter is not in place"); return MC33HIP_EINVAL; }
	RkPlan p;
	memset(&p, 0, sizeof p);
	p.n[0] = d.npx; p.n[1] = d.npy; p.n[2] = d.npz_resident;
	for (int a = 0; a < 3; a++) p.r[a] = (int)r->radius[a];
	p.rank = r->rank;
	p.spitch = c->pitch; p.sslice = c->slice; p.dpitch = pitch; p.dslice = slice;
	typedef RkKey<sample_t>::K K;
	rk_plan_tiles(p, sizeof(K));
	const long long blocks = p.tiles_x * p.tiles_y * p.chunks_z;
	if (blocks > 0x7FFFFFFFll) { set_err("%lld tiles: more than a launch takes", blocks); return MC33HIP_EINVAL; }
	int rc;
	if ((rc = use_device(c))) return rc;
	const size_t lds = p.lds_keys * sizeof(K);
	const sample_t *src = (const sample_t *)c->d_grid;
#define RK_LAUNCH(kernel) hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(RK_THREADS), lds, c->stream, src, (sample_t *)dst, p)
	if (p.rank != RK_RANK_MEDIAN) RK_LAUNCH((k_rk_minmax<sample_t>));
	else switch ((2 * p.r[0] + 1) * (2 * p.r[1] + 1) * 10 + 2 * p.r[2] + 1) {
		case 11: RK_LAUNCH((k_rk_median<sample_t, 1, 1>)); break;
		case 31: RK_LAUNCH((k_rk_median<sample_t, 3, 1>)); break;
		case 91: RK_LAUNCH((k_rk_median<sample_t, 9, 1>)); break;
		case 13: RK_LAUNCH((k_rk_median<sample_t, 1, 3>)); break;
		case 33: RK_LAUNCH((k_rk_median<sample_t, 3, 3>)); break;
		default: RK_LAUNCH((k_rk_median<sample_t, 9, 3>)); break;
	}
#undef RK_LAUNCH
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c->stream));
	return MC33HIP_OK;
}

#endif  // __HIPCC__
