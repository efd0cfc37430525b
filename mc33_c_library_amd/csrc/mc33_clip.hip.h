// mc33_clip.hip.h -- part of the ONE translation unit mc33_kernels.hip (builds on mc33_mesh.hip.h; not a header to include elsewhere):
// a FINISHED mesh in device memory cut by one plane - the half space s >= 0 stays, triangles the plane crosses are cut, the new
// vertices on the cut edges are shared between the triangles on either side - so that only the part a viewer shows crosses the
// link (include/mc33_hip.h: mc33hip_clip_surface).  DESIGN.md 17.
//
// The definition is in include/mc33_hip.h; tests/clip_oracle.py restates it in numpy, operation for operation.  Which triangle
// owns a cut edge, where a row lands and what it holds are decided by integer atomics, exclusive scans and IEEE double arithmetic
// with nothing fused: the result is an exact function of the input.
// The passes: k_clip_class, a lane per vertex, leaves the class of every vertex in a byte; k_clip_tri, the hot path, a lane per
// triangle, validates, classifies, counts 0, 1 or 2 output triangles, marks the kept vertices and enters each cut side into a
// table of 16-byte slots - the key lo << 32 | hi claimed by 64-bit compare-and-swap (the table of mc33_mesh.hip.h), the owner
// word i << 2 | e by a 64-bit atomicMin - but not where the lane before it in the wave, the triangle before it in T, holds the
// same edge: that lane's word is the smaller one; k_clip_own flags the sides that find their own word in the slot; the tile
// scans of mc33_mesh.hip.h run over the kept flags, the owned sides and the output triangles; k_clip_rows moves the kept rows and writes oMap; k_clip_new, the owner's lane, computes t and
// writes the new rows at kept_vertices + rank and leaves the rank in the slot; k_clip_emit repeats the walk and writes the
// triangles at their scanned place.  Nothing a block wrote with plain stores is read by another block of the same kernel: the
// words of the table are touched only by atomics in k_clip_tri, their readers are later kernels; the rank is stored by
// k_clip_new and read by k_clip_emit.

struct ClipSlot { unsigned long long key, owner; };  // 16 bytes (lo < hi, so no key is MESH_EMPTY)
struct ClipPlane { double a, b, c, w; };

enum { CLIP_OUT = 0, CLIP_ON = 1, CLIP_IN = 2, CLIP_NONFINITE = 4 };  // the class byte of a vertex: low two bits, and s not finite
// the byte of a triangle: output triangles (0, 1, 2) | cut sides << 2 | owned sides << 5

struct ClipOut {            // what a call brings to the host (device copy and pinned twin)
	unsigned long long kept, cutv, nT_out, on_plane, whole, cut, dropped, bad, nonfinite;
	unsigned long long full;      // cut sides that found no slot (cannot happen: the table is larger than what enters; checked all the same)
	unsigned long long pad_[2];
};

struct ClipState {          // scratch of these passes besides the shared keep (1: an output triangle names the vertex), map (new[v]) and tile sums
                            // (the vertex tiles, behind them the triangle tiles twice: owned sides, outputs): on the MeasureState from the first call on, grown on demand, freed with it
	ClipOut *d_out, *h_out;
	uint8_t *d_cls;         // [nV] class of the vertex
	uint64_t cls_cap;
	uint8_t *d_nf;          // [nV] 1: a valid triangle names the vertex and its s is not finite
	uint64_t nf_cap;
	uint8_t *d_info;        // [nT] the byte of the triangle
	uint64_t info_cap;
	ClipSlot *d_slots;      // the edge table: a power of two >= 4 nT slots
	uint64_t slots_cap;
};

template <typename R>
__device__ __forceinline__ double clip_s(const R *__restrict__ V, uint64_t v, const ClipPlane &P) {
	const R *p = V + v * 3u;
	const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
	return ((x * P.a + y * P.b) + z * P.c) + P.w;
}
__host__ __device__ __forceinline__ bool clip_finite(double s) { return fabs(s) <= 1.7976931348623157e308; }  // (false for a NaN)

__device__ __forceinline__ unsigned long long clip_key(uint32_t p, uint32_t q) {
	return p < q ? ((unsigned long long)p << 32) | q : ((unsigned long long)q << 32) | p;
}
// bit e: side e = corner e -> corner (e + 1) % 3 has one end in and one out (2 ^ 0; a side with an end on the plane is never cut)
__device__ __forceinline__ uint32_t clip_cuts(uint32_t a0, uint32_t a1, uint32_t a2) {
	return ((a0 ^ a1) == 2u ? 1u : 0u) | ((a1 ^ a2) == 2u ? 2u : 0u) | ((a2 ^ a0) == 2u ? 4u : 0u);
}

// one use of a cut edge: the slot claimed, the owner word lowered.  Returns false when every slot was tried.
__device__ __forceinline__ bool clip_enter(ClipSlot *slots, uint64_t mask, unsigned long long key, unsigned long long owner) {
	const uint64_t s = mesh_claim(slots, mask, key);
	if (s == MESH_NOSLOT) return false;
	atomicMin(&slots[s].owner, owner);
	return true;
}

template <typename R>
__global__ __launch_bounds__(256) void k_clip_class(const R *__restrict__ V, uint64_t nV, ClipPlane P, uint8_t *__restrict__ cls) {
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const double s = clip_s(V, v, P);
		uint32_t c = s > 0.0 ? CLIP_IN : s == 0.0 ? CLIP_ON : CLIP_OUT;  // (a NaN is out)
		if (!clip_finite(s)) c |= CLIP_NONFINITE;
		cls[v] = (uint8_t)c;
	}
}

// The hot path.  Every wave 64 consecutive triangles a step; every lane of the wave takes every step.  A lane holds at most two
// cut edges.  The emit stage writes neighbouring triangles side by side: lane l - 1 is triangle i - 1, whose owner words are
// smaller than any of triangle i's - an edge both hold needs no atomic from lane l, whether lane l - 1 enters it itself or
// leaves it to the lane before for the same reason.
__global__ __launch_bounds__(256) void k_clip_tri(const uint32_t *__restrict__ T, uint64_t nT, uint64_t nV, const uint8_t *__restrict__ cls, ClipSlot *slots,
                                                  uint64_t mask, uint8_t *__restrict__ keep, uint8_t *__restrict__ nf, uint8_t *__restrict__ info,
                                                  ClipOut *__restrict__ out) {
	__shared__ uint32_t sh[4];
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t bad = 0u, whole = 0u, cut = 0u, dropped = 0u, full = 0u;
	for (uint64_t base = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); base < nT; base += (uint64_t)gridDim.x * 256u) {  // (wave-uniform)
		const uint64_t i = base + lane;
		unsigned long long k0 = MESH_EMPTY, k1 = MESH_EMPTY, w0 = 0ull, w1 = 0ull;
		if (i < nT) {
			const uint32_t *t = T + i * 3u;
			const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
			uint32_t word = 0u;
			if (t0 >= nV || t1 >= nV || t2 >= nV) bad++;  // (tested before anything is gathered through it)
			else {
				const uint32_t c0 = cls[t0], c1 = cls[t1], c2 = cls[t2];
				if ((c0 | c1 | c2) & CLIP_NONFINITE) {  // (every racing store writes the same 1)
					if (c0 & CLIP_NONFINITE) nf[t0] = 1;
					if (c1 & CLIP_NONFINITE) nf[t1] = 1;
					if (c2 & CLIP_NONFINITE) nf[t2] = 1;
				}
				const uint32_t a0 = c0 & 3u, a1 = c1 & 3u, a2 = c2 & 3u;
				if (a0 != CLIP_IN && a1 != CLIP_IN && a2 != CLIP_IN) dropped++;
				else {
					const uint32_t cuts = clip_cuts(a0, a1, a2);
					const uint32_t entries = (a0 != CLIP_OUT ? 1u : 0u) + (a1 != CLIP_OUT ? 1u : 0u) + (a2 != CLIP_OUT ? 1u : 0u) + (uint32_t)__popc(cuts);
					word = (entries - 2u) | (cuts << 2);
					if (cuts) cut++; else whole++;
					if (a0 != CLIP_OUT) keep[t0] = 1;
					if (a1 != CLIP_OUT) keep[t1] = 1;
					if (a2 != CLIP_OUT) keep[t2] = 1;
					if (cuts & 1u) { k0 = clip_key(t0, t1); w0 = (unsigned long long)i << 2; }
					if (cuts & 2u) {
						const unsigned long long k = clip_key(t1, t2), w = ((unsigned long long)i << 2) | 1ull;
						if (k0 == MESH_EMPTY) { k0 = k; w0 = w; } else { k1 = k; w1 = w; }
					}
					if (cuts & 4u) {
						const unsigned long long k = clip_key(t2, t0), w = ((unsigned long long)i << 2) | 2ull;
						if (k0 == MESH_EMPTY) { k0 = k; w0 = w; } else { k1 = k; w1 = w; }
					}
					if (k1 == k0) k1 = MESH_EMPTY;  // (a triangle with two equal indices: the side that comes first owns)
				}
			}
			info[i] = (uint8_t)word;
		}
		const unsigned long long p0 = ((unsigned long long)__shfl_up((uint32_t)(k0 >> 32), 1, 64) << 32) | __shfl_up((uint32_t)k0, 1, 64);
		const unsigned long long p1 = ((unsigned long long)__shfl_up((uint32_t)(k1 >> 32), 1, 64) << 32) | __shfl_up((uint32_t)k1, 1, 64);
		if (lane != 0u) {
			if (k0 == p0 || k0 == p1) k0 = MESH_EMPTY;  // (an empty word never equals a key; two empty words need no atomic either)
			if (k1 == p0 || k1 == p1) k1 = MESH_EMPTY;
		}
		if (k0 != MESH_EMPTY && !clip_enter(slots, mask, k0, w0)) full++;
		if (k1 != MESH_EMPTY && !clip_enter(slots, mask, k1, w1)) full++;
	}
	bad = block_sum_u32_256(bad, sh);
	whole = block_sum_u32_256(whole, sh);
	cut = block_sum_u32_256(cut, sh);
	dropped = block_sum_u32_256(dropped, sh);
	full = block_sum_u32_256(full, sh);
	if (threadIdx.x == 0u) {
		if (bad) atomicAdd(&out->bad, (unsigned long long)bad);
		if (whole) atomicAdd(&out->whole, (unsigned long long)whole);
		if (cut) atomicAdd(&out->cut, (unsigned long long)cut);
		if (dropped) atomicAdd(&out->dropped, (unsigned long long)dropped);
		if (full) atomicAdd(&out->full, (unsigned long long)full);
	}
}

// a (triangle, side) owns its cut edge when the slot holds its word: the smallest i << 2 | e of the edge's uses
__global__ __launch_bounds__(256) void k_clip_own(const uint32_t *__restrict__ T, uint64_t nT, const ClipSlot *__restrict__ slots, uint64_t mask,
                                                  uint8_t *__restrict__ info, ClipOut *__restrict__ out) {
	uint32_t full = 0u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nT; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t word = info[i], cuts = (word >> 2) & 7u;
		if (!cuts) continue;
		const uint32_t *t = T + i * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];  // (a triangle with a cut side is valid)
		uint32_t own = 0u;
		if (cuts & 1u) {
			const uint64_t s = mesh_find(slots, mask, clip_key(t0, t1));
			if (s == MESH_NOSLOT) full++;
			else if (slots[s].owner == ((unsigned long long)i << 2)) own |= 1u;
		}
		if (cuts & 2u) {
			const uint64_t s = mesh_find(slots, mask, clip_key(t1, t2));
			if (s == MESH_NOSLOT) full++;
			else if (slots[s].owner == (((unsigned long long)i << 2) | 1ull)) own |= 2u;
		}
		if (cuts & 4u) {
			const uint64_t s = mesh_find(slots, mask, clip_key(t2, t0));
			if (s == MESH_NOSLOT) full++;
			else if (slots[s].owner == (((unsigned long long)i << 2) | 2ull)) own |= 4u;
		}
		if (own) info[i] = (uint8_t)(word | (own << 5));
	}
	if (full) atomicAdd(&out->full, (unsigned long long)full);
}

// what the byte of a triangle counts for the tile scans: its owned sides, its output triangles
struct ClipOwned { using E = uint8_t; static __device__ __forceinline__ uint32_t count(uint32_t b) { return (uint32_t)__popc(b >> 5); } };
struct ClipOutputs { using E = uint8_t; static __device__ __forceinline__ uint32_t count(uint32_t b) { return b & 3u; } };

__device__ __forceinline__ bool clip_fits(const ClipOut *__restrict__ out, uint64_t capV, uint64_t capT) {
	return out->kept + out->cutv <= capV && out->nT_out <= capT;
}

// oMap for every vertex; the kept rows of V, N and the attribute words to their new places, as words; the two
// counts over the vertices (they are taken whether the caller's arrays are large enough or not).  R: MC33_real.
template <typename R>
__global__ __launch_bounds__(256) void k_clip_rows(const R *__restrict__ V, const float *__restrict__ N, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                                   const uint32_t *__restrict__ map, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ nf, uint64_t nV,
                                                   ClipOut *__restrict__ out, uint64_t capV, uint64_t capT, R *__restrict__ oV, float *__restrict__ oN,
                                                   uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1, uint32_t *__restrict__ oMap) {
	__shared__ uint32_t sh[4];
	const bool fits = clip_fits(out, capV, capT);  // (the totals are those of earlier kernels; this one adds to other words)
	uint32_t onp = 0u, nonf = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const uint32_t m = map[v];
		nonf += nf[v] ? 1u : 0u;
		if (m != MESH_NONE && (cls[v] & 3u) == CLIP_ON) onp++;
		if (!fits) continue;
		if (oMap) oMap[v] = m;
		if (m == MESH_NONE) continue;
		mesh_copy_row(V, N, v, oV, oN, m);
		if (A0) oA0[m] = A0[v];
		if (A1) oA1[m] = A1[v];
	}
	onp = block_sum_u32_256(onp, sh);
	nonf = block_sum_u32_256(nonf, sh);
	if (threadIdx.x == 0u) {
		if (onp) atomicAdd(&out->on_plane, (unsigned long long)onp);
		if (nonf) atomicAdd(&out->nonfinite, (unsigned long long)nonf);
	}
}

// one attribute word of a new vertex
__device__ __forceinline__ uint32_t clip_word(const uint32_t *__restrict__ A, uint32_t lo, uint32_t hi, uint32_t in, double t, bool copy, uint32_t lerp) {
	if (copy || !lerp) return A[in];
	const double x = (double)__uint_as_float(A[lo]), y = (double)__uint_as_float(A[hi]);
	return __float_as_uint((float)(x + t * (y - x)));
}

// The new vertex of the cut edge {p, q} at row `row` of the outputs, and its rank in the edge's slot.  lo < hi by index, so the
// row does not depend on the direction of the side that owns the edge.
template <typename R>
__device__ __forceinline__ void clip_new_row(const R *__restrict__ V, const float *__restrict__ N, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                             uint32_t lerp0, uint32_t lerp1, const ClipPlane &P, uint32_t p, uint32_t q, uint64_t row, R *__restrict__ oV,
                                             float *__restrict__ oN, uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1) {
	const uint32_t lo = p < q ? p : q, hi = p < q ? q : p;
	const double slo = clip_s(V, lo, P), shi = clip_s(V, hi, P);
	const uint32_t in = slo > 0.0 ? lo : hi;  // (one end is in, the other out)
	const bool copy = !clip_finite(slo) || !clip_finite(shi);
	const double t = slo / (slo - shi);
	R *oq = oV + row * 3u;
	if (copy) mesh_copy_row(V, N, in, oV, oN, row);  // the bytes of the end that is in
	else {
		const R *a = V + (uint64_t)lo * 3u, *b = V + (uint64_t)hi * 3u;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const double x = (double)a[k], y = (double)b[k];
			oq[k] = (R)(x + t * (y - x));
		}
		if (oN) {
			const float *na = N + (uint64_t)lo * 3u, *nb = N + (uint64_t)hi * 3u;
			float *on = oN + row * 3u;
			const double ax = (double)na[0], ay = (double)na[1], az = (double)na[2];
			const double x = ax + t * ((double)nb[0] - ax), y = ay + t * ((double)nb[1] - ay), z = az + t * ((double)nb[2] - az);
			const double m = sqrt((x * x + y * y) + z * z);
			const bool ok = m > 0.0;
			on[0] = ok ? (float)(x / m) : 0.0f;
			on[1] = ok ? (float)(y / m) : 0.0f;
			on[2] = ok ? (float)(z / m) : 0.0f;
		}
	}
	if (A0) oA0[row] = clip_word(A0, lo, hi, in, t, copy, lerp0);
	if (A1) oA1[row] = clip_word(A1, lo, hi, in, t, copy, lerp1);
}

// the owned sides of a tile of triangles: their ranks by the scan, their rows behind the kept vertices, the rank into the slot
template <typename R>
__global__ __launch_bounds__(256) void k_clip_new(const R *__restrict__ V, const float *__restrict__ N, const uint32_t *__restrict__ A0, const uint32_t *__restrict__ A1,
                                                  uint32_t lerp0, uint32_t lerp1, ClipPlane P, const uint32_t *__restrict__ T, uint64_t nT,
                                                  const uint8_t *__restrict__ info, const uint32_t *__restrict__ bsum, ClipSlot *__restrict__ slots, uint64_t mask,
                                                  const ClipOut *__restrict__ out, uint64_t capV, uint64_t capT, R *__restrict__ oV, float *__restrict__ oN,
                                                  uint32_t *__restrict__ oA0, uint32_t *__restrict__ oA1) {
	__shared__ uint32_t sh[256];
	if (!clip_fits(out, capV, capT)) return;  // (block-uniform: the caller's arrays are too small, nothing is written)
	const uint64_t kept = out->kept;
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
			clip_new_row(V, N, A0, A1, lerp0, lerp1, P, p, q, kept + r, oV, oN, oA0, oA1);
			const uint64_t s = mesh_find(slots, mask, clip_key(p, q));
			if (s != MESH_NOSLOT) slots[s].owner = r;  // (the owner found its slot in k_clip_own)
			r++;
		}
	}
}

// the polygon of a walk, entry by entry (selects, not an indexed array)
struct ClipPoly {
	uint32_t e0, e1, e2, e3, n;
	__device__ __forceinline__ void push(uint32_t x) {
		if (n == 0u) e0 = x; else if (n == 1u) e1 = x; else if (n == 2u) e2 = x; else e3 = x;
		n++;
	}
};

// the walk again: the corners that are kept through map (a corner of a triangle that has outputs is out exactly when it is not
// kept), the cut vertices through the ranks in the table; 1 or 2 triangles at the tile's place in oT
__global__ __launch_bounds__(256) void k_clip_emit(const uint32_t *__restrict__ T, uint64_t nT, const uint8_t *__restrict__ info, const uint32_t *__restrict__ map,
                                                   const ClipSlot *__restrict__ slots, uint64_t mask, const uint32_t *__restrict__ bsum,
                                                   const ClipOut *__restrict__ out, uint64_t capV, uint64_t capT, uint32_t *__restrict__ oT) {
	__shared__ uint32_t sh[256];
	if (!clip_fits(out, capV, capT)) return;
	const uint32_t kept = (uint32_t)out->kept;
	const uint64_t i0 = mesh_tile_e0();
	uint32_t f[4];
	const uint32_t own = mesh_tile_load<ClipOutputs>(info, nT, f);
	uint64_t r = mesh_tile_place(bsum, own, sh);
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++) {
		const uint32_t n = f[k] & 3u, cuts = (f[k] >> 2) & 7u;
		if (!n) continue;
		const uint32_t *t = T + (i0 + k) * 3u;
		const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
		ClipPoly g;
		g.e0 = g.e1 = g.e2 = g.e3 = 0u; g.n = 0u;
#pragma unroll
		for (uint32_t e = 0; e < 3u; e++) {
			const uint32_t p = e == 0u ? t0 : e == 1u ? t1 : t2, q = e == 0u ? t1 : e == 1u ? t2 : t0;
			const uint32_t m = map[p];
			if (m != MESH_NONE) g.push(m);
			if ((cuts >> e) & 1u) {
				const uint64_t s = mesh_find(slots, mask, clip_key(p, q));
				g.push(kept + (s != MESH_NOSLOT ? (uint32_t)slots[s].owner : 0u));
			}
		}
		uint32_t *o = oT + r * 3u;
		o[0] = g.e0; o[1] = g.e1; o[2] = g.e2;
		if (n == 2u) { o[3] = g.e0; o[4] = g.e2; o[5] = g.e3; }
		r += n;
	}
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void clip_release(void *state) {
	ClipState *s = (ClipState *)state;
	dev_release(&s->d_cls); dev_release(&s->d_nf); dev_release(&s->d_info); dev_release(&s->d_slots);
}
static int clip_state(mc33hip_ctx *c, ClipState **s) {
	const int rc = meas_state(c);
	return rc ? rc : mesh_op_state(&c->meas->mesh, clip_release, s);
}

static void clip_fill(mc33hip_clipping *a, const ClipOut &h) {
	a->nV_out = h.kept + h.cutv; a->nT_out = h.nT_out; a->kept_vertices = h.kept; a->cut_vertices = h.cutv; a->on_plane_vertices = h.on_plane;
	a->whole_triangles = h.whole; a->cut_triangles = h.cut; a->dropped_triangles = h.dropped; a->invalid_triangles = h.bad; a->nonfinite_vertices = h.nonfinite;
}

extern "C" int mc33hip_clip_surface(mc33hip_ctx *c, mc33hip_clipping *a) {
	if (!c || !a) return MC33HIP_EINVAL;
	a->nV_out = a->nT_out = a->kept_vertices = a->cut_vertices = a->on_plane_vertices = a->whole_triangles = a->cut_triangles = a->dropped_triangles =
	    a->invalid_triangles = a->nonfinite_vertices = 0;
	const unsigned long long nV = a->nV, nT = a->nT;
	if (!mesh_counts_ok(a->n_attr, nV, nT)) return MC33HIP_EINVAL;
	for (unsigned k = 0; k < a->n_attr; k++)
		if (a->attr_mode[k] != MC33HIP_CLIP_COPY && a->attr_mode[k] != MC33HIP_CLIP_LERP_F32) {
			set_err("attr_mode[%u] = %d is neither MC33HIP_CLIP_COPY nor MC33HIP_CLIP_LERP_F32", k, a->attr_mode[k]);
			return MC33HIP_EINVAL;
		}
	for (int k = 0; k < 4; k++)
		if (!clip_finite(a->plane[k])) { set_err("plane[%d] must be finite", k); return MC33HIP_EINVAL; }
	if (a->plane[0] == 0.0 && a->plane[1] == 0.0 && a->plane[2] == 0.0) { set_err("the plane has no normal: a, b and c are all zero"); return MC33HIP_EINVAL; }
	const uint64_t capV = mesh_cap(a->capV), capT = mesh_cap(a->capT);
	if (!mesh_pointers_ok((nV && !a->V) || (nT && !a->T) || (capV && !a->oV) || (capT && !a->oT), a->n_attr, a->attr, a->oAttr, nV, capV)) return MC33HIP_EINVAL;
	if (a->oN && !a->N) { set_err("oN without N: the normals of the output are interpolated from those of the input"); return MC33HIP_EINVAL; }
	// the call is not in place: no output may share a byte with an input or with another output
	const MeshRange in[5] = {{a->V, nV * 3u * sizeof(real_t)}, {a->N, nV * 12u}, {a->T, nT * 12u}, {a->n_attr > 0u ? a->attr[0] : nullptr, nV * 4u},
	                         {a->n_attr > 1u ? a->attr[1] : nullptr, nV * 4u}};
	const MeshRange out[6] = {{a->oV, capV * 3u * sizeof(real_t)}, {a->oT, capT * 12u}, {a->oN, capV * 12u}, {a->oMap, nV * 4u}, {a->n_attr > 0u ? a->oAttr[0] : nullptr, capV * 4u},
	                          {a->n_attr > 1u ? a->oAttr[1] : nullptr, capV * 4u}};
	if (!mesh_ranges_ok(in, 5, out, 6, true, "clipping")) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	ClipState *s;
	if ((rc = clip_state(c, &s))) return rc;
	if (!nT || !nV) {  // every count is 0
		if ((rc = mesh_empty(c, a->oMap, nV))) return rc;
		a->invalid_triangles = nT;
		return mesh_bad(nT, nV);
	}
	MeshHost &h = c->meas->mesh;
	const uint64_t tilesV = (nV + MESH_TILE - 1u) / MESH_TILE, tilesT = (nT + MESH_TILE - 1u) / MESH_TILE;
	const uint64_t nslots = mesh_table_size(nT, 4u, 1ull << 40);
	if ((rc = meas_scratch(c, nV, tilesV + 2u * tilesT))) return rc;
	if ((rc = meas_room(&s->d_cls, &s->cls_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_nf, &s->nf_cap, nV))) return rc;
	if ((rc = meas_room(&s->d_info, &s->info_cap, nT))) return rc;
	if ((s->slots_cap < nslots || !s->d_slots) && (rc = dev_room("cut edge table", &s->d_slots, &s->slots_cap, nslots))) return rc;  // (a power of two as it is: no slack)
	uint32_t *bsumV = h.d_bsum, *bsumO = h.d_bsum + tilesV, *bsumT = bsumO + tilesT;
	const real_t *V = (const real_t *)a->V;
	const float *N = a->oN ? (const float *)a->N : nullptr;
	const uint32_t *T = (const uint32_t *)a->T;
	const uint32_t *A0 = (const uint32_t *)(a->n_attr > 0u ? a->attr[0] : nullptr), *A1 = (const uint32_t *)(a->n_attr > 1u ? a->attr[1] : nullptr);
	uint32_t *oA0 = (uint32_t *)(a->n_attr > 0u ? a->oAttr[0] : nullptr), *oA1 = (uint32_t *)(a->n_attr > 1u ? a->oAttr[1] : nullptr);
	const uint32_t lerp0 = a->n_attr > 0u && a->attr_mode[0] == MC33HIP_CLIP_LERP_F32 ? 1u : 0u, lerp1 = a->n_attr > 1u && a->attr_mode[1] == MC33HIP_CLIP_LERP_F32 ? 1u : 0u;
	ClipPlane P;
	P.a = a->plane[0]; P.b = a->plane[1]; P.c = a->plane[2]; P.w = a->plane[3];
	// (8 blocks per CU where a block ends with a set of atomics, as for the component table)
	const uint32_t gridV = meas_grid(c, nV, 16u), gridT = meas_grid(c, nT, 16u), gridH = meas_grid(c, nT, 8u);
	HIP_TRY(hipMemsetAsync(s->d_out, 0, sizeof(ClipOut), c->stream));
	HIP_TRY(hipMemsetAsync(h.d_keep, 0, nV, c->stream));
	HIP_TRY(hipMemsetAsync(s->d_nf, 0, nV, c->stream));
	hipLaunchKernelGGL(k_mesh_clear, dim3(meas_grid(c, nslots, 16u)), dim3(256), 0, c->stream, (ulonglong2 *)s->d_slots, nslots, ~0ull);  // (the owner: above every word)
	hipLaunchKernelGGL((k_clip_class<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, (uint64_t)nV, P, s->d_cls);
	hipLaunchKernelGGL(k_clip_tri, dim3(gridH), dim3(256), 0, c->stream, T, (uint64_t)nT, (uint64_t)nV, s->d_cls, s->d_slots, nslots - 1u, h.d_keep, s->d_nf, s->d_info,
	                   s->d_out);
	hipLaunchKernelGGL(k_clip_own, dim3(gridT), dim3(256), 0, c->stream, T, (uint64_t)nT, s->d_slots, nslots - 1u, s->d_info, s->d_out);
	mesh_scan<MeshFlag, MESH_NEW>(c, h.d_keep, nV, bsumV, &s->d_out->kept, h.d_map);
	mesh_scan<ClipOwned>(c, s->d_info, nT, bsumO, &s->d_out->cutv);    // (k_clip_new places)
	mesh_scan<ClipOutputs>(c, s->d_info, nT, bsumT, &s->d_out->nT_out);  // (k_clip_emit places)
	// the writing passes: they compare the totals with the capacities on the device, so that the host waits once
	hipLaunchKernelGGL((k_clip_rows<real_t>), dim3(gridV), dim3(256), 0, c->stream, V, N, A0, A1, h.d_map, s->d_cls, s->d_nf, (uint64_t)nV, s->d_out, capV, capT,
	                   (real_t *)a->oV, (float *)a->oN, oA0, oA1, (uint32_t *)a->oMap);
	hipLaunchKernelGGL((k_clip_new<real_t>), dim3((uint32_t)tilesT), dim3(256), 0, c->stream, V, N, A0, A1, lerp0, lerp1, P, T, (uint64_t)nT, s->d_info, bsumO, s->d_slots,
	                   nslots - 1u, s->d_out, capV, capT, (real_t *)a->oV, (float *)a->oN, oA0, oA1);
	hipLaunchKernelGGL(k_clip_emit, dim3((uint32_t)tilesT), dim3(256), 0, c->stream, T, (uint64_t)nT, s->d_info, h.d_map, s->d_slots, nslots - 1u, bsumT, s->d_out, capV,
	                   capT, (uint32_t *)a->oT);
	if ((rc = mesh_op_fetch(c, s))) return rc;
	const ClipOut o = *s->h_out;
	clip_fill(a, o);
	if (o.full) { set_err("%llu cut sides found no slot in the table", o.full); return MC33HIP_ERUNTIME; }
	if ((rc = mesh_capacity("clipped", o.kept + o.cutv, o.nT_out, capV, capT))) return rc;
	return mesh_bad(o.bad, nV);
}
