// mc33_spectrum.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, last; not a header to include elsewhere):
// the contour spectrum of the resident grid - for a ladder of up to 255 ascending isovalues, how many cells the surface cuts at each
// one, a histogram of the samples between the steps, and the range of the samples - in one pass over the grid
// (include/mc33_hip.h: mc33hip_grid_spectrum).  DESIGN.md 16.
//
// The definition is in include/mc33_hip.h; tests/spectrum_oracle.py restates it in numpy.  Everything is an integer: the order in
// which blocks, waves and lanes add changes no bit.
//
// rank(r) = #{ j : iso_j < r } is the side bit of a sample for every isovalue at once (the bit for iso_k is rank > k), so a cell
// is cut at exactly the isovalues k with min_rank <= k < max_rank over its eight corners: one +1 at diff[min_rank] and one -1 at
// diff[max_rank], and cut_cells is the running sum of diff.
//
// One hot kernel, k_sp_spectrum.  A block of 256 lanes takes work items (tile of 64 x 16 cells, chunk of SP_ZCHUNK cell slices)
// in a grid-stride loop and marches along z.  Per plane: sp_stage loads the 65 x 17 samples of the tile once, ranks each - a
// branch-free binary search over the isovalues in LDS, a 256-entry table for 1-byte samples - leaves the ranks as bytes in LDS
// and counts the samples the tile owns in the block's histogram; sp_cells takes min and max over the four corners a cell has in
// this plane, joins them with the pair the lane kept from the plane before (a lane owns the same four cells all the way) and
// counts the cell where min < max.  The rank planes are double buffered: one barrier per plane.  The block's 32-bit counters go
// to the 64-bit device counters once, when the block has no work left.
// The first part of this file - everything down to the line that says so - has no HIP in it: the functions are the kernel's whole
// arithmetic and indexing, taking the lane number and the counters as arguments, and tests/spectrum_host.cpp compiles this text
// with the host compiler, runs the phases lane by lane and is held to the oracle.

#ifndef SP_HD
#define SP_HD __host__ __device__ __forceinline__
#endif
#ifdef __HIPCC__
#define SP_UNROLL _Pragma("unroll")
#else
#define SP_UNROLL
#endif

constexpr int SP_THREADS = 256;
constexpr int SP_TILE_X = 64, SP_TILE_Y = 16;   // cells per tile; a lane owns cell column (lane & 63) of rows 4 (lane >> 6) .. + 3
constexpr int SP_ZCHUNK = 32;        // cell slices per work item: the item stages one plane more than it has slices
constexpr int SP_MAX_ISOS = 255;
constexpr int SP_ROWS = SP_TILE_Y + 1, SP_COLS = SP_TILE_X + 1;   // samples of a tile's plane
constexpr int SP_RANK_PITCH = 68;    // bytes per row of a rank plane in LDS
constexpr int SP_RANK_PLANE = SP_ROWS * SP_RANK_PITCH;
constexpr int SP_LANE_CELLS = SP_TILE_X * SP_TILE_Y / SP_THREADS;
constexpr int SP_OUT_WORDS = 2 * 256 + 3;   // device counters: hist[256] | diff[256] | NaN samples | key of the minimum | key of the maximum
static_assert(SP_LANE_CELLS == 4 && SP_TILE_X == 64, "sp_cells packs the four cells of a lane into one word");

struct SpPlan {
	uint32_t npx, npy;            // points per row, rows per plane
	uint32_t k_begin, k_end;      // resident planes: cell slices [k_begin, k_end), sample planes k_begin .. k_end
	uint32_t last_plane_counts;   // the samples of plane k_end belong to the histogram (the range ends where the grid does)
	uint32_t tiles_x, tiles_y, chunks_z;
	uint32_t n, top;              // isovalues; the largest power of two <= n (0 for n == 0): the first step of the search
	uint64_t items;               // tiles_x * tiles_y * chunks_z
	size_t pitch, slice;          // in samples
};

// what a lane carries from plane to plane and from item to item
struct SpLane {
	uint32_t pmin, pmax;   // min / max rank over the four corners each of its four cells has in the plane before, a byte per cell
	uint32_t nan;
	double lo, hi;         // extremes of the non-NaN samples it counted, as doubles (exact for float and double)
};
SP_HD void sp_lane_init(SpLane &s) { s.pmin = s.pmax = 0u; s.nan = 0u; s.lo = __builtin_huge_val(); s.hi = -__builtin_huge_val(); }

SP_HD uint32_t sp_sign(float f) { return __builtin_bit_cast(uint32_t, f) >> 31; }
SP_HD uint32_t sp_sign(double f) { return (uint32_t)(__builtin_bit_cast(uint64_t, f) >> 63); }

// rank of r among isos[0 .. n), ascending and padded with +inf to 256 entries: entry pos + step - 1 is read only while
// pos + step <= 2 top - 1 <= 255.  A NaN compares false everywhere; its rank is its own sign's (mc33_cell.h: iso_diff).
template <typename R>
SP_HD uint32_t sp_rank(const R *isos, uint32_t n, uint32_t top, R r) {
	uint32_t pos = 0u;
	for (uint32_t step = top; step; step >>= 1) pos += isos[pos + step - 1u] < r ? step : 0u;
	if (r != r) pos = sp_sign(r) ? n : 0u;
	return pos;
}

// a double as an unsigned key in the order of the values (-inf lowest, +inf highest of the non-NaN), and back
SP_HD uint64_t sp_key(double d) {
	const uint64_t b = __builtin_bit_cast(uint64_t, d);
	return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
SP_HD double sp_unkey(uint64_t k) { return __builtin_bit_cast(double, (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k); }

// sample s of what a load brought
template <typename T, int S, typename L>
SP_HD T sp_unpack(L raw, int s) {
	if constexpr (S == 1) return (T)raw;
	else return (T)(raw >> (8 * (int)sizeof(T) * s));
}

// rank of one sample: the search, or the table for 1-byte samples
template <typename T, typename R>
SP_HD uint32_t sp_rank_of(const SpPlan &p, T v, const R *isos, const uint8_t *table) {
	if constexpr (sizeof(T) == 1) return table[(uint32_t)v & 255u];
	else return sp_rank(isos, p.n, p.top, (R)v);
}

// one sample of the tile and its rank: into the rank plane, and - where the tile owns it - into the counters
template <typename T, typename R, typename C>
SP_HD void sp_sample(T v, uint32_t rank, bool valid, bool owned, int q, int c, uint8_t *ranks, SpLane &st, C &ctr) {
	if (valid) {
		ranks[q * SP_RANK_PITCH + c] = (uint8_t)rank;
		if (owned) {
			const R r = (R)v;
			if (r != r) st.nan++;
			else {
				const double d = (double)r;
				st.lo = d < st.lo ? d : st.lo;
				st.hi = d > st.hi ? d : st.hi;
			}
		}
	}
	ctr.hist(valid && owned, rank);
}

// phase 1: the samples of resident plane k the tile at (X0, Y0) needs.  S samples per load: 1, or a dword of 2 / 4 narrow samples
// where base, pitch and slice are multiples of 4 bytes (X0 is a multiple of 64 samples: the tile's rows begin on a dword too).  A
// dword that holds a grid point may end behind the row's last one, inside the pitch - the readable extent mc33hip_adopt_device
// states; nothing else is read.  A tile owns the samples of its 64 x 16 cells' lower corners, and the last column / row of the
// grid where it ends there: every sample is counted by exactly one tile.  Every lane makes the same number of turns, in three
// rounds: all its loads first - they are in flight together -, then all its searches - every step of a search waits for the LDS
// read of the step before, and the searches of a lane's samples do not depend on one another -, then ranks and counters.
template <typename T, typename R, int S, typename C>
SP_HD void sp_stage(const SpPlan &p, const T *src, uint32_t k, uint32_t X0, uint32_t Y0, bool count_plane, const R *isos, const uint8_t *table,
                    uint8_t *ranks, SpLane &st, C &ctr, int lane) {
	const T *plane = src + (size_t)k * p.slice;
	constexpr int W = S == 1 ? SP_COLS : SP_TILE_X / S + 1;   // loads per row
	constexpr int TURNS = (SP_ROWS * W + SP_THREADS - 1) / SP_THREADS;
	const uint32_t row_loads = (p.npx + (uint32_t)S - 1u) / (uint32_t)S;   // loads that hold a grid point of a row
	typedef typename std::conditional<S == 1, T, uint32_t>::type load_t;
	load_t raw[TURNS];
	uint32_t rank[TURNS * S];
	SP_UNROLL
	for (int t = 0; t < TURNS; t++) {
		const int e = t * SP_THREADS + lane;
		const int q = e / W, w = e - q * W;
		const uint32_t y = Y0 + (uint32_t)q, li = X0 / (uint32_t)S + (uint32_t)w;
		const bool there = e < SP_ROWS * W && y < p.npy && li < row_loads;
		const T *row = plane + (size_t)y * p.pitch;
		raw[t] = (load_t)0;
		if (there) raw[t] = ((const load_t *)row)[li];
	}
	SP_UNROLL
	for (int t = 0; t < TURNS; t++) {   // (a sample that is not there ranks as 0 and is not used)
		SP_UNROLL
		for (int s = 0; s < S; s++) rank[t * S + s] = sp_rank_of<T, R>(p, sp_unpack<T, S>(raw[t], s), isos, table);
	}
	SP_UNROLL
	for (int t = 0; t < TURNS; t++) {
		const int e = t * SP_THREADS + lane;
		const int q = e / W, w = e - q * W;
		const uint32_t y = Y0 + (uint32_t)q, li = X0 / (uint32_t)S + (uint32_t)w;
		const bool there = e < SP_ROWS * W && y < p.npy && li < row_loads;
		const bool own_row = count_plane && (q < SP_TILE_Y || y == p.npy - 1u);
		SP_UNROLL
		for (int s = 0; s < S; s++) {
			const int c = w * S + s;
			const uint32_t x = X0 + (uint32_t)c;
			const T v = sp_unpack<T, S>(raw[t], s);
			sp_sample<T, R>(v, rank[t * S + s], there && c < SP_COLS && x < p.npx, own_row && (c < SP_TILE_X || x == p.npx - 1u), q, c, ranks, st, ctr);
		}
	}
}

// phase 2: the lane's four cells between the plane before and this one.  Ranks of samples outside the grid are whatever LDS
// held; the cells that would use them are outside too and are not counted.
template <typename C>
SP_HD void sp_cells(const SpPlan &p, const uint8_t *ranks, uint32_t X0, uint32_t Y0, bool first_plane, SpLane &st, C &ctr, int lane) {
	const int cx = lane & (SP_TILE_X - 1), cy0 = (lane >> 6) * SP_LANE_CELLS;
	const uint8_t *a = ranks + cy0 * SP_RANK_PITCH + cx;
	uint32_t lo[SP_LANE_CELLS + 1], hi[SP_LANE_CELLS + 1];
	SP_UNROLL
	for (int j = 0; j <= SP_LANE_CELLS; j++) {
		const uint32_t u = a[j * SP_RANK_PITCH], v = a[j * SP_RANK_PITCH + 1];
		lo[j] = u < v ? u : v;
		hi[j] = u < v ? v : u;
	}
	const bool in_x = X0 + (uint32_t)cx + 1u < p.npx;
	uint32_t pmin = 0u, pmax = 0u;
	SP_UNROLL
	for (int j = 0; j < SP_LANE_CELLS; j++) {
		const uint32_t mn = lo[j] < lo[j + 1] ? lo[j] : lo[j + 1], mx = hi[j] > hi[j + 1] ? hi[j] : hi[j + 1];
		pmin |= mn << (8 * j);
		pmax |= mx << (8 * j);
		const uint32_t bn = (st.pmin >> (8 * j)) & 255u, bx = (st.pmax >> (8 * j)) & 255u;
		const uint32_t cn = mn < bn ? mn : bn, cm = mx > bx ? mx : bx;
		const bool inside = in_x && Y0 + (uint32_t)(cy0 + j) + 1u < p.npy;
		ctr.diff(!first_plane && inside && cn < cm, cn, cm);
	}
	st.pmin = pmin;
	st.pmax = pmax;
}

// work item -> tile and chunk (x fastest: neighbouring blocks share the halo column they stage)
SP_HD void sp_item(const SpPlan &p, uint64_t item, uint32_t &X0, uint32_t &Y0, uint32_t &kb, uint32_t &ke) {
	const uint32_t tx = (uint32_t)(item % p.tiles_x);
	item /= p.tiles_x;
	const uint32_t ty = (uint32_t)(item % p.tiles_y), tz = (uint32_t)(item / p.tiles_y);
	X0 = tx * (uint32_t)SP_TILE_X;
	Y0 = ty * (uint32_t)SP_TILE_Y;
	kb = p.k_begin + tz * (uint32_t)SP_ZCHUNK;
	ke = p.k_end - kb > (uint32_t)SP_ZCHUNK ? kb + (uint32_t)SP_ZCHUNK : p.k_end;
}

// the plan of a range of resident planes (checked by the caller)
static inline void sp_plan(SpPlan &p, uint32_t npx, uint32_t npy, uint32_t k_begin, uint32_t k_end, bool last_plane_counts, uint32_t n, size_t pitch, size_t slice) {
	p.npx = npx; p.npy = npy; p.k_begin = k_begin; p.k_end = k_end; p.last_plane_counts = last_plane_counts ? 1u : 0u;
	p.tiles_x = (npx - 1u + (uint32_t)SP_TILE_X - 1u) / (uint32_t)SP_TILE_X;
	p.tiles_y = (npy - 1u + (uint32_t)SP_TILE_Y - 1u) / (uint32_t)SP_TILE_Y;
	p.chunks_z = (k_end - k_begin + (uint32_t)SP_ZCHUNK - 1u) / (uint32_t)SP_ZCHUNK;
	p.n = n;
	p.top = 0u;
	for (uint32_t s = 1u; s <= n; s <<= 1) p.top = s;
	p.items = (uint64_t)p.tiles_x * p.tiles_y * p.chunks_z;
	p.pitch = pitch; p.slice = slice;
}

// ---- everything above compiles without HIP (tests/spectrum_host.cpp) ---------------------------------------------------------------
#ifdef __HIPCC__

struct SpectrumState {       // scratch of the spectrum: on the MeasureState from the first call on, freed with it
	real_t *d_isos;                  // [256], padded with +inf
	unsigned long long *d_out;       // [SP_OUT_WORDS]
	unsigned long long *h_out;       // pinned copy
	int blocks_per_cu[2];            // of k_sp_spectrum, a sample per load / packed: asked of the runtime once
};

// The block's counters in LDS.  Neighbouring samples mostly share a rank: the lanes of a wave that hold the rank of its first
// counting lane add their number in one LDS atomic, the others add for themselves.
struct SpDevCounters {
	uint32_t *h;
	int *d;
	__device__ __forceinline__ void hist(bool valid, uint32_t rank) {
		if (valid) {
			const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rank);
			const bool same = rank == r0;
			const unsigned long long m = __ballot(same);   // (of the lanes in here)
			if (!same) atomicAdd(&h[rank], 1u);
			else if ((int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicAdd(&h[r0], (uint32_t)__popcll(m));
		}
	}
	__device__ __forceinline__ void diff(bool cut, uint32_t mn, uint32_t mx) {
		if (cut) { atomicAdd(&d[mn], 1); atomicSub(&d[mx], 1); }
	}
};

__global__ __launch_bounds__(SP_THREADS) void k_sp_init(unsigned long long *__restrict__ out) {
	for (int k = (int)threadIdx.x; k < SP_OUT_WORDS; k += SP_THREADS)
		out[k] = k == 2 * 256 + 1 ? sp_key(__builtin_huge_val()) : k == 2 * 256 + 2 ? sp_key(-__builtin_huge_val()) : 0ull;
}

// The hot path.  S: samples per load (sp_stage).
template <typename T, int S>
__global__ __launch_bounds__(SP_THREADS) void k_sp_spectrum(const T *__restrict__ src, const real_t *__restrict__ d_isos, unsigned long long *__restrict__ out, SpPlan p) {
	__shared__ real_t isos[256];
	__shared__ uint32_t hist[256];
	__shared__ int diff[256];
	__shared__ uint8_t table[256];
	__shared__ uint8_t ranks[2][SP_RANK_PLANE];
	__shared__ unsigned long long ext[2];
	__shared__ uint32_t nans;
	const int lane = (int)threadIdx.x;
	isos[lane] = d_isos[lane];
	hist[lane] = 0u;
	diff[lane] = 0;
	if (lane == 0) { ext[0] = sp_key(__builtin_huge_val()); ext[1] = sp_key(-__builtin_huge_val()); nans = 0u; }
	__syncthreads();
	if constexpr (sizeof(T) == 1) {
		table[lane] = (uint8_t)sp_rank<real_t>(isos, p.n, p.top, (real_t)(T)lane);
		__syncthreads();
	}
	SpLane st;
	sp_lane_init(st);
	SpDevCounters ctr{hist, diff};
	for (uint64_t item = blockIdx.x; item < p.items; item += gridDim.x) {   // (block-uniform loops: every lane meets every barrier)
		uint32_t X0, Y0, kb, ke;
		sp_item(p, item, X0, Y0, kb, ke);
		for (uint32_t k = kb; k <= ke; k++) {
			uint8_t *plane = ranks[(k - kb) & 1u];
			sp_stage<T, real_t, S>(p, src, k, X0, Y0, k < ke || (ke == p.k_end && p.last_plane_counts != 0u), isos, table, plane, st, ctr, lane);
			__syncthreads();
			sp_cells(p, plane, X0, Y0, k == kb, st, ctr, lane);
		}
		__syncthreads();   // (the next item stages into plane 0, which the cells of an even last plane still read)
	}
	atomicMin(&ext[0], sp_key(st.lo));
	atomicMax(&ext[1], sp_key(st.hi));
	if (st.nan) atomicAdd(&nans, st.nan);
	__syncthreads();
	if (hist[lane]) atomicAdd(&out[lane], (unsigned long long)hist[lane]);
	if (diff[lane]) atomicAdd(&out[256 + lane], (unsigned long long)(long long)diff[lane]);   // (two's complement: the sum of all blocks is exact)
	if (lane == 0) {
		if (nans) atomicAdd(&out[2 * 256], (unsigned long long)nans);
		atomicMin(&out[2 * 256 + 1], ext[0]);
		atomicMax(&out[2 * 256 + 2], ext[1]);
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void sp_release(void *state) {  // (the result block is an array of words, not a struct: made and freed here)
	SpectrumState *s = (SpectrumState *)state;
	dev_release(&s->d_isos);
	dev_release(&s->d_out);
	if (s->h_out) (void)hipHostFree(s->h_out);
}

// As many blocks as the device holds at once - a block keeps its counters until it has no work left, and a second round of blocks
// would run with part of the GPU idle - and no fewer than the 32-bit counters of a block allow: at most 32768 items of
// 64 x 16 x 32 cells and 65 x 17 x 33 samples each (the cells' counters are signed).
template <int S>
static int sp_launch(mc33hip_ctx *c, SpectrumState *s, const SpPlan &p) {
	int &per_cu = s->blocks_per_cu[S > 1];
	if (!per_cu) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sp_spectrum<sample_t, S>, SP_THREADS, 0));
	uint64_t blocks = std::min<uint64_t>(p.items, (uint64_t)std::max(1, c->cus) * (uint64_t)std::max(1, per_cu));
	blocks = std::max<uint64_t>(blocks, (p.items + 32767u) / 32768u);
	if (blocks > 0x7FFFFFFFull) { set_err("%llu work items: more than a launch takes", (unsigned long long)p.items); return MC33HIP_EINVAL; }
	hipLaunchKernelGGL((k_sp_spectrum<sample_t, S>), dim3((uint32_t)blocks), dim3(SP_THREADS), 0, c->stream, (const sample_t *)c->d_grid, (const real_t *)s->d_isos, s->d_out, p);
	return 0;
}

extern "C" int mc33hip_grid_spectrum(mc33hip_ctx *c, const mc33hip_range *range, mc33hip_spectrum *a) {
	if (!c || !range || !a) return MC33HIP_EINVAL;
	if (a->n > (unsigned)SP_MAX_ISOS) { set_err("%u isovalues: at most %d", a->n, SP_MAX_ISOS); return MC33HIP_EINVAL; }
	if (!a->histogram || (a->n && (!a->isos || !a->cut_cells))) return MC33HIP_EINVAL;
	real_t isos[256];
	for (unsigned k = 0; k < 256u; k++) isos[k] = (real_t)__builtin_huge_val();
	for (unsigned k = 0; k < a->n; k++) {
		isos[k] = (real_t)a->isos[k];   // (as mc33hip_count takes its isovalue)
		if (isos[k] != isos[k]) { set_err("isovalue %u is a NaN", k); return MC33HIP_EINVAL; }
		if (k && !(isos[k - 1u] < isos[k])) { set_err("isovalues %u and %u are not strictly ascending as MC33_real", k - 1u, k); return MC33HIP_EINVAL; }
	}
	const mc33hip_grid_desc &d = c->desc;
	if (!(range->z_begin < range->z_end) || range->z_end > d.nz_total || range->z_begin < d.plane0 ||
	    (uint64_t)range->z_end > (uint64_t)d.plane0 + d.npz_resident - 1u) {
		set_err("cell slices [%u, %u): not a range of the %u slices whose planes [%u, %u) are resident", range->z_begin, range->z_end, d.nz_total, d.plane0, d.plane0 + d.npz_resident);
		return MC33HIP_EINVAL;
	}
	if (!c->d_grid) { set_err("no grid is resident in this context"); return MC33HIP_EINVAL; }
	const bool last = range->z_end == d.nz_total;
	SpPlan p;
	memset(&p, 0, sizeof p);
	sp_plan(p, d.npx, d.npy, range->z_begin - d.plane0, range->z_end - d.plane0, last, a->n, c->pitch, c->slice);
	int rc;
	if ((rc = use_device(c))) return rc;
	if ((rc = meas_state(c))) return rc;
	MeshOp *op;
	if ((rc = mesh_op_find(&c->meas->mesh, sp_release, sizeof(SpectrumState), &op))) return rc;
	SpectrumState *s = (SpectrumState *)op->state;
	if (!s->d_isos) HIP_TRY(hipMalloc(&s->d_isos, 256 * sizeof(real_t)));
	if (!s->d_out) HIP_TRY(hipMalloc(&s->d_out, SP_OUT_WORDS * sizeof(unsigned long long)));
	if (!s->h_out) HIP_TRY(hipHostMalloc(&s->h_out, SP_OUT_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
	// (the isovalues are in pageable host memory: the copy has left it when the call returns, and is ordered on the stream)
	HIP_TRY(hipMemcpyAsync(s->d_isos, isos, sizeof isos, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_sp_init, dim3(1), dim3(SP_THREADS), 0, c->stream, s->d_out);
	if ((rc = sweep_packed(c) ? sp_launch<SWEEP_PACK>(c, s, p) : sp_launch<1>(c, s, p))) return rc;   // (packed: narrow samples, rows on dword boundaries - mc33_extract.hip.h)
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, SP_OUT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const unsigned long long *o = s->h_out;
	const unsigned long long planes = (unsigned long long)(range->z_end - range->z_begin) + (last ? 1u : 0u);
	a->points = (unsigned long long)d.npx * d.npy * planes;
	a->cells = (unsigned long long)(d.npx - 1u) * (d.npy - 1u) * (range->z_end - range->z_begin);
	unsigned long long run = 0ull;
	for (unsigned k = 0; k <= a->n; k++) {
		a->histogram[k] = o[k];
		run += o[256 + k];
		if (k < a->n) a->cut_cells[k] = run;
	}
	a->nan_samples = o[2 * 256];
	a->sample_min = sp_unkey(o[2 * 256 + 1]);
	a->sample_max = sp_unkey(o[2 * 256 + 2]);
	return MC33HIP_OK;
}

#endif  // __HIPCC__
