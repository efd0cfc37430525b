// mc33_mesh.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_context.hip.h; not a header to include elsewhere):
// what the passes over a FINISHED V, N, T in device memory have in common - mc33_measure, mc33_topology, mc33_filter, mc33_smooth,
// mc33_simplify, mc33_clip, mc33_section, mc33_cap and mc33_render build on it and on nothing of each other's but what their opening lines name.  DESIGN.md 18.
//   block primitives   sums and scans over the 256 lanes of a block, sums over runs of equal keys in a wave
//   the tile scan      an exclusive scan of what the elements of an array count, in tiles of MESH_TILE: a sum per tile, one block
//                      over the tile sums, a placing pass - or a writing kernel of a part's own that opens like one
//   the table          open addressing over 64-bit keys in device memory, claimed by compare-and-swap
//   flags and rows     the vertices valid triangles name; a row of V and N moved as words
//   host side          a part's state and result block registered on the MeasureState, the scratch no two parts use at once,
//                      the argument checks of the calls that write a new mesh

constexpr uint32_t MESH_TILE = 1024u;             // elements per block of the tile scan: 256 lanes x 4
constexpr uint32_t MESH_NONE = 0xFFFFFFFFu;       // no row: a dropped vertex in a map, a vertex without a slot
constexpr unsigned long long MESH_EMPTY = ~0ull;  // the key of an empty slot (no part's keys have all 64 bits)
constexpr uint64_t MESH_NOSLOT = ~0ull;

// --- block primitives -----------------------------------------------------------------------------------------------------

__device__ __forceinline__ double shfl_down_f64(double x, int d) { return __shfl_down(x, d, 64); }
__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long x, int d) {
	const uint32_t lo = __shfl_down((uint32_t)x, d, 64), hi = __shfl_down((uint32_t)(x >> 32), d, 64);
	return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
	return x;  // (lane 0)
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_down(x, d, 64); x = o > x ? o : x; }
	return x;
}

// sum over the block's 256 lanes; every lane gets it.  sh: [4]
__device__ __forceinline__ uint32_t block_sum_u32_256(uint32_t x, uint32_t *sh) {
	x = wave_sum_u32(x);
	__syncthreads();
	if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = x;
	__syncthreads();
	return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// exclusive sum over the block's 256 lanes of x; *total: the block's sum.  sh: [256]
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t x, uint32_t *sh, uint32_t *total) {
	const uint32_t t = threadIdx.x;
	__syncthreads();
	sh[t] = x;
	__syncthreads();
	for (uint32_t d = 1u; d < 256u; d <<= 1) {
		const uint32_t o = t >= d ? sh[t - d] : 0u;
		__syncthreads();
		sh[t] += o;
		__syncthreads();
	}
	*total = sh[255];
	return sh[t] - x;
}

// Sums over runs of equal keys in consecutive lanes of a wave: `heads` has a bit for every lane that begins a run; after the
// call the first lane of each run holds the run's sum.
__device__ __forceinline__ bool run_open(unsigned long long heads, uint32_t lane, int d) {  // lane + d belongs to lane's run
	return lane + (uint32_t)d < 64u && ((heads >> (lane + 1u)) & ((1ull << d) - 1ull)) == 0ull;
}
__device__ __forceinline__ double run_sum_f64(double x, unsigned long long heads, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const double o = shfl_down_f64(x, d);
		if (run_open(heads, lane, d)) x += o;
	}
	return x;
}
__device__ __forceinline__ uint32_t run_sum_u32(uint32_t x, unsigned long long heads, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_down(x, d, 64);
		if (run_open(heads, lane, d)) x += o;
	}
	return x;
}
__device__ __forceinline__ unsigned long long run_sum_u64(unsigned long long x, unsigned long long heads, uint32_t lane) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = shfl_down_u64(x, d);
		if (run_open(heads, lane, d)) x += o;
	}
	return x;
}

// --- the tile scan --------------------------------------------------------------------------------------------------------
// Where an element's output lands is decided by the sums alone: no atomic takes part in it.  What an element counts is a type W
// with the element's type E and count(e), count(0) == 0; a part with a field of its own in a byte defines its own W.

struct MeshFlag { using E = uint8_t; static __device__ __forceinline__ uint32_t count(uint32_t b) { return b ? 1u : 0u; } };
struct MeshCount { using E = uint32_t; static __device__ __forceinline__ uint32_t count(uint32_t n) { return n; } };

// the lane's four elements of tile blockIdx.x begin at this index
__device__ __forceinline__ uint64_t mesh_tile_e0() { return (uint64_t)blockIdx.x * MESH_TILE + threadIdx.x * 4u; }
// f: the lane's four elements (0 behind the end of the array); returns what they count
template <typename W>
__device__ __forceinline__ uint32_t mesh_tile_load(const typename W::E *x, uint64_t n, uint32_t f[4]) {
	const uint64_t e0 = mesh_tile_e0();
	uint32_t own = 0u;
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		f[k] = e0 + k < n ? (uint32_t)x[e0 + k] : 0u;
		own += W::count(f[k]);
	}
	return own;
}
// The placing prologue: where the first output of the lane lands when its four elements count `own` - the scanned sum of the
// tiles before this one and of the lanes before this one.  The lane then walks its four.  sh: [256]
__device__ __forceinline__ uint64_t mesh_tile_place(const uint32_t *__restrict__ bsum, uint32_t own, uint32_t *sh) {
	uint32_t tot;
	return (uint64_t)bsum[blockIdx.x] + block_excl_scan_256(own, sh, &tot);
}

template <typename W>
__global__ __launch_bounds__(256) void k_mesh_tile_sum(const typename W::E *__restrict__ x, uint64_t n, uint32_t *__restrict__ bsum) {
	__shared__ uint32_t sh[4];
	uint32_t f[4];
	const uint32_t tot = block_sum_u32_256(mesh_tile_load<W>(x, n, f), sh);
	if (threadIdx.x == 0u) bsum[blockIdx.x] = tot;
}

// one block: bsum -> its exclusive sums, in place, 256 tiles a round; *total (where not null): their sum
__device__ __forceinline__ void mesh_scan_top_block(uint32_t *__restrict__ bsum, uint64_t n, unsigned long long *__restrict__ total, uint32_t *sh /* [256] */) {
	uint32_t carry = 0u;
	for (uint64_t base = 0; base < n; base += 256u) {
		const uint64_t k = base + threadIdx.x;
		const uint32_t x = k < n ? bsum[k] : 0u;
		uint32_t tot;
		const uint32_t e = block_excl_scan_256(x, sh, &tot);
		if (k < n) bsum[k] = carry + e;
		carry += tot;
	}
	if (total && threadIdx.x == 0u) *total = carry;
}
__global__ __launch_bounds__(256) void k_mesh_scan_top(uint32_t *__restrict__ bsum, uint64_t n, unsigned long long *__restrict__ total) {
	__shared__ uint32_t sh[256];
	mesh_scan_top_block(bsum, n, total, sh);
}
// the same for three arrays of tile sums side by side, a block each: a part whose scans do not depend on each other waits for one
// chain of rounds, not three
struct MeshTop { uint32_t *bsum; uint64_t n; unsigned long long *total; };
__global__ __launch_bounds__(256) void k_mesh_scan_top3(MeshTop a, MeshTop b, MeshTop c) {
	__shared__ uint32_t sh[256];
	const MeshTop t = blockIdx.x == 0u ? a : blockIdx.x == 1u ? b : c;
	mesh_scan_top_block(t.bsum, t.n, t.total, sh);
}

// what the placing pass leaves in out[e]: the sum below e (a rank); that where e counts and MESH_NONE where it does not (the
// new index of a kept element); the sum below e and the total in out[n] (row starts - out may be x: a lane reads its four
// counts before it writes over them)
enum { MESH_RANK, MESH_NEW, MESH_STARTS, MESH_NOWHERE };
template <typename W, int HOW>
__global__ __launch_bounds__(256) void k_mesh_place(const typename W::E *x, const uint32_t *__restrict__ bsum, uint64_t n, uint32_t *out) {
	__shared__ uint32_t sh[256];
	const uint64_t e0 = mesh_tile_e0();
	uint32_t f[4];
	const uint32_t own = mesh_tile_load<W>(x, n, f);
	uint32_t r = (uint32_t)mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint32_t w = W::count(f[k]);
		if (e0 + k < n) out[e0 + k] = HOW == MESH_NEW && !w ? MESH_NONE : r;
		r += w;
		if (HOW == MESH_STARTS && e0 + k + 1u == n) out[n] = r;
	}
}

// Enqueue the scan of one array: mesh_scan from the array on, mesh_scan_sums behind tile sums already in bsum (a kernel that
// counts while it does other work left them).  HOW MESH_NOWHERE: no placing pass - a writing kernel of the part's places.
template <typename W, int HOW = MESH_NOWHERE>
static void mesh_scan_sums(mc33hip_ctx *c, const typename W::E *x, uint64_t n, uint32_t *bsum, unsigned long long *total, uint32_t *out = nullptr) {
	const uint64_t tiles = (n + MESH_TILE - 1u) / MESH_TILE;
	if (!n) return;  // (the total stays as the part zeroed it)
	hipLaunchKernelGGL(k_mesh_scan_top, dim3(1), dim3(256), 0, c->stream, bsum, tiles, total);
	if constexpr (HOW != MESH_NOWHERE) hipLaunchKernelGGL((k_mesh_place<W, HOW>), dim3((uint32_t)tiles), dim3(256), 0, c->stream, x, (const uint32_t *)bsum, n, out);
}
template <typename W, int HOW = MESH_NOWHERE>
static void mesh_scan(mc33hip_ctx *c, const typename W::E *x, uint64_t n, uint32_t *bsum, unsigned long long *total, uint32_t *out = nullptr) {
	if (!n) return;
	hipLaunchKernelGGL((k_mesh_tile_sum<W>), dim3((uint32_t)((n + MESH_TILE - 1u) / MESH_TILE)), dim3(256), 0, c->stream, x, n, bsum);
	mesh_scan_sums<W, HOW>(c, x, n, bsum, total, out);
}

// --- the table ------------------------------------------------------------------------------------------------------------
// A power of two of slots whose first member is the 64-bit key, MESH_EMPTY where the slot is free; insert-only; linear probing.

// the splitmix64 finalizer: every bit of the key reaches every bit of the home slot
__device__ __forceinline__ uint64_t mesh_mix(uint64_t x) {
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}

static uint64_t mesh_table_size(uint64_t n, uint64_t factor, uint64_t max) {  // a power of two >= factor n, at most max
	uint64_t s = 256u;
	while (s < factor * n && s < max) s <<= 1;
	return s;
}

// The slot of `key`, claimed where the table did not hold it.  What the compare-and-swap on the key RETURNS decides - empty or
// equal: this is the key's slot; anything else: probe on, linearly.  A kernel that claims never reads a slot with a plain load,
// the key no more than the words behind it (the XCDs' L2s are not coherent for those): it adds to them with atomics, and their
// readers are later kernels.  MESH_NOSLOT when every slot was tried.
template <typename S>
__device__ __forceinline__ uint64_t mesh_claim(S *slots, uint64_t mask, unsigned long long key) {
	uint64_t s = mesh_mix(key) & mask;
	for (uint64_t tries = 0; tries <= mask; tries++, s = (s + 1u) & mask) {
		const unsigned long long old = atomicCAS(&slots[s].key, MESH_EMPTY, key);
		if (old == MESH_EMPTY || old == key) return s;
	}
	return MESH_NOSLOT;
}
// the slot of a key a finished table holds (a later kernel: plain loads), MESH_NOSLOT when it does not
template <typename S>
__device__ __forceinline__ uint64_t mesh_find(const S *__restrict__ slots, uint64_t mask, unsigned long long key) {
	uint64_t s = mesh_mix(key) & mask;
	for (uint64_t tries = 0; tries <= mask; tries++, s = (s + 1u) & mask) {
		const unsigned long long k = slots[s].key;
		if (k == key) return s;
		if (k == MESH_EMPTY) break;
	}
	return MESH_NOSLOT;
}

// every 16-byte slot empty, `second` in the word behind the key
__global__ __launch_bounds__(256) void k_mesh_clear(ulonglong2 *__restrict__ slots, uint64_t n, unsigned long long second) {
	for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256u) slots[s] = make_ulonglong2(MESH_EMPTY, second);
}

// --- referenced flags and rows --------------------------------------------------------------------------------------------

// ref[v] = 1 for every vertex a valid triangle names (every racing store writes the same 1); the others are counted
__global__ __launch_bounds__(256) void k_mesh_ref(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, uint8_t *__restrict__ ref, unsigned long long *__restrict__ bad_out) {
	uint32_t bad = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		if (t0 >= nV || t1 >= nV || t2 >= nV) { bad++; continue; }
		ref[t0] = 1; ref[t1] = 1; ref[t2] = 1;
	}
	if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// row `from` of V, and of N where oN is not null, to row `to`: no floating-point instruction touches a row.  R: MC33_real
template <typename R>
__device__ __forceinline__ void mesh_copy_row(const R *__restrict__ V, const float *__restrict__ N, uint64_t from, R *__restrict__ oV, float *__restrict__ oN, uint64_t to) {
	const R *q = V + from * 3u;
	R *oq = oV + to * 3u;
	const R q0 = q[0], q1 = q[1], q2 = q[2];
	oq[0] = q0; oq[1] = q1; oq[2] = q2;
	if (oN) {
		const float *n = N + from * 3u;
		float *on = oN + to * 3u;
		const float n0 = n[0], n1 = n[1], n2 = n[2];
		on[0] = n0; on[1] = n1; on[2] = n2;
	}
}

// --- host side ------------------------------------------------------------------------------------------------------------

// A part's state on the MeasureState: made by the part's first call, freed with the context.  A state struct S begins with
// `Out *d_out, *h_out` - what a call brings to the host, device copy and pinned twin - or, made by mesh_op_find alone, has none.
struct MeshOp {
	void *state, *d_out, *h_out;
	void (*release)(void *state);  // the device arrays the state holds; it is the key of the registration too
};
struct MeshHost {
	MeshOp op[12];              // topology, filter, smooth, simplify, clip, resample, spectrum, section, curvature, cap, render, distance: a part beyond that makes this larger
	uint32_t nops;
	// scratch no two parts use at once (every entry point waits before it returns), grown on demand by meas_room
	uint8_t *d_keep;            // [nV] a flag per vertex: referenced, kept
	uint64_t keep_cap;
	uint32_t *d_map;            // [nV] the new index of a vertex, MESH_NONE where it has none
	uint64_t map_cap;
	uint32_t *d_bsum;           // tile sums, scanned in place: a part's arrays side by side
	uint64_t bsum_cap;
};

static MeshOp *mesh_op_peek(MeshHost *h, void (*release)(void *)) {  // the registration, null before the part's first call
	for (uint32_t k = 0; k < h->nops; k++)
		if (h->op[k].release == release) return &h->op[k];
	return nullptr;
}
static int mesh_op_find(MeshHost *h, void (*release)(void *), size_t state_bytes, MeshOp **op) {
	if ((*op = mesh_op_peek(h, release))) return 0;
	if (h->nops == sizeof h->op / sizeof h->op[0]) { set_err("no room to register another mesh part"); return MC33HIP_ERUNTIME; }
	void *s = calloc(1, state_bytes);
	if (!s) return MC33HIP_ENOMEM;
	*op = &h->op[h->nops++];  // (what it holds so far goes with the context)
	(*op)->state = s; (*op)->release = release;
	return 0;
}
template <typename S>
static int mesh_op_state(MeshHost *h, void (*release)(void *), S **state) {
	MeshOp *op;
	if (int rc = mesh_op_find(h, release, sizeof(S), &op)) return rc;
	S *s = *state = (S *)op->state;
	// (the members, not the struct: a call after a failed allocation tries that allocation again)
	if (!s->d_out) HIP_TRY(hipMalloc(&s->d_out, sizeof *s->d_out));
	op->d_out = s->d_out;
	if (!s->h_out) HIP_TRY(hipHostMalloc(&s->h_out, sizeof *s->h_out, hipHostMallocDefault));
	op->h_out = s->h_out;
	return 0;
}
static void mesh_host_destroy(MeshHost *h) {
	for (uint32_t k = 0; k < h->nops; k++) {
		MeshOp &op = h->op[k];
		op.release(op.state);
		(void)hipFree(op.d_out);
		if (op.h_out) (void)hipHostFree(op.h_out);
		free(op.state);
	}
	h->nops = 0;
	dev_release(&h->d_keep); dev_release(&h->d_map); dev_release(&h->d_bsum);
}

// the tail of a call: the result block of the state to the host behind everything enqueued; waits
template <typename S>
static int mesh_op_fetch(mc33hip_ctx *c, S *s) {
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, sizeof *s->d_out, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return prop_check(c);
}

// --- the argument checks of the calls that write a new mesh (compaction, simplification, clipping) ---------------------------

static bool mesh_sizes_ok(unsigned long long nV, unsigned long long nT) {
	if (nV > 0xFFFFFFFFull || nT > 0xFFFFFFFFull) { set_err("more than 2^32-1 vertices or triangles"); return false; }
	return true;
}
static int mesh_bad(unsigned long long n, unsigned long long nV) {
	if (!n) return 0;
	set_err("%llu triangle%s name%s a vertex outside the %llu rows of V (or of the label array): left out of every sum", n, n == 1 ? "" : "s", n == 1 ? "s" : "", nV);
	return MC33HIP_ERUNTIME;
}
static bool mesh_counts_ok(unsigned n_attr, unsigned long long nV, unsigned long long nT) {
	if (n_attr > 2u) { set_err("at most two attribute arrays, not %u", n_attr); return false; }
	return mesh_sizes_ok(nV, nT);
}
static uint64_t mesh_cap(unsigned long long cap) { return std::min<unsigned long long>(cap, 0xFFFFFFFFull); }  // (row numbers are 32-bit words)

// `null`: what the call found among its own pointers; the attribute arrays are tested here
static bool mesh_pointers_ok(bool null, unsigned n_attr, const void *const attr[2], void *const oAttr[2], uint64_t nV, uint64_t capV) {
	for (unsigned k = 0; k < n_attr; k++) null = null || (nV && !attr[k]) || (capV && !oAttr[k]);
	if (null) set_err("a null pointer where the size is not zero");
	return !null;
}

struct MeshRange { const void *p; uint64_t bytes; };
static bool mesh_ranges_meet(const void *a, uint64_t na, const void *b, uint64_t nb) {
	if (!a || !b || !na || !nb) return false;
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return x < y + nb && y < x + na;
}
// no output may share a byte with an input, nor - `among` - with another output.  what: "compaction", "simplification", "clipping"
static bool mesh_ranges_ok(const MeshRange *in, int n_in, const MeshRange *out, int n_out, bool among, const char *what) {
	for (int o = 0; o < n_out; o++) {
		for (int i = 0; i < n_in; i++)
			if (mesh_ranges_meet(in[i].p, in[i].bytes, out[o].p, out[o].bytes)) { set_err("an output array overlaps an input array: the %s is not in place", what); return false; }
		for (int p = o + 1; among && p < n_out; p++)
			if (mesh_ranges_meet(out[p].p, out[p].bytes, out[o].p, out[o].bytes)) { set_err("two output arrays overlap"); return false; }
	}
	return true;
}

// no valid triangle (nT == 0, or nV == 0: every triangle is invalid): nothing is kept and oMap, where the caller has one, says so
static int mesh_empty(mc33hip_ctx *c, void *oMap, uint64_t nV) {
	if (nV && oMap) HIP_TRY(hipMemsetAsync(oMap, 0xFF, nV * 4u, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return prop_check(c);
}

static int mesh_capacity(const char *what, unsigned long long nV_out, unsigned long long nT_out, uint64_t capV, uint64_t capT) {
	if (nV_out <= capV && nT_out <= capT) return 0;
	set_err("the %s mesh needs %llu rows of V and %llu of T, the caller's arrays have %llu and %llu", what, nV_out, nT_out, (unsigned long long)capV, (unsigned long long)capT);
	return MC33HIP_ECAPACITY;
}
