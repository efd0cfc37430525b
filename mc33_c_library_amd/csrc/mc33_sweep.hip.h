// mc33_sweep.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, in order; not a header to include elsewhere):
// k_sweep (the one pass over the volume) and k_boundary (the slices between its tiles).

// ---------------------------------------------------------------------------------------------------
// k_sweep: one wave per tile (256 samples in x, 64 sample rows, a run of planes).  The waves are independent; the
// plan puts the tiles of neighbouring row segments next to each other, so that the 4 waves of a block normally read
// whole 1024-sample (4 KiB) row pieces, and fills blocks with whatever tiles come next where a grid is not a multiple
// of 1024 samples wide (plan_sweep).
//
// Every lane loads 4 samples of a row (x = xbase + 64k + lane: fully coalesced 256-byte requests),
// v = iso - F, the sign bits of the 64 lanes are collected by ballot into one 64-bit word per k, and the
// 4 words of sample row r are parked in lane r.  After a plane is in, lane r holds the bits of row r for
// planes z and z+1 and gets row r+1 from its neighbour lane: the "all 8 corners on the same side" test
// (MC:1860) of the 63 x 256 cells of the tile slice is ~100 logic ops per wave.  Slices with cut cells
// have their bit rows written out (4 KiB) for k_cells; nothing else is stored, nothing is allocated:
// the wave only streams.  (Doing the per-cell work here made the kernel end on a long tail of a few
// waves whose tiles hold most of the surface.)
//
// Tiles of one column do not overlap: a tile reads the planes z_lo+1 .. z_hi (the lowest tile of the column also
// z_lo) and handles the slices between them; the slice between its first plane and the last plane of the tile
// below is put together by k_boundary from the bit rows both tiles leave behind (2 KiB each) - re-reading that
// plane instead cost 1/depth of the traffic (6 % at depth 16).
// ---------------------------------------------------------------------------------------------------
// How a ballot (the sign bits of 64 samples of one row, an SGPR pair) is parked in the lane of its row: ONE v_mov_b64 with EXEC
// narrowed to that lane (gfx940+ moves 64 bits in one instruction, and an SGPR pair is a legal source), the passes over several
// isovalues two isovalues per EXEC switch: 4 instead of 8 vector instructions per row and isovalue - the passes over four
// isovalues of narrow samples are bound by exactly these (round 4; the v_writelane_b32 form of rounds 1 - 3: EXPERIMENTS.md)
#if defined(MC33_GRD_U16)
constexpr int SWEEP_PACK = 2;  // samples per dword
#elif defined(MC33_GRD_U8)
constexpr int SWEEP_PACK = 4;
#else
constexpr int SWEEP_PACK = 1;
#endif

// ---------------------------------------------------------------------------------------------------
// k_ranges: the range table (RangeEntry) of the resident planes, one streaming pass.  A wave per strip, the four waves of a block
// the four strips of a 1024-sample group of row segments (the 4 KiB row pieces the sweep reads).  Minimum and maximum are taken of
// the CONVERTED samples ((MC33_real)F, what MC33_LOAD makes of them: the conversion is monotone, but not one to one for 32-bit
// integers).  Addresses past the strip are clamped into it - a sample taken twice changes no minimum - so every lane has the same
// number of loads in flight and only grid points are ever read.
// V: rows in 16-byte pieces (base, pitch and slice all multiples of 16 bytes - the library's own copy, any whole tensor), taken
// by the strips that are 256 samples wide; the strips at the end of a row, and every strip of a buffer aligned otherwise, go
// sample by sample, which is correct for any base, pitch and slice.
// ---------------------------------------------------------------------------------------------------
// The block table (RangeEntry, RANGE_BLOCKS entries per strip, [strip][entry]; `blocks`, nullptr: not kept): the ranges of the 64 x 16
// sample blocks one load instruction of the float sweep covers.  Entry 4 g + k: the sample rows 16 g .. 16 g + 15 of the strip (g = 3
// holds the row shared with the next y tile) and the samples 64 k .. 64 k + 63 of the segment; entries 16 + g: the halo column over
// the rows of group g.  A block's range is taken over what the sweep's loads of that block return, its addresses clamped as the sweep
// clamps them (xo[], so, xh in sweep_tile): a row past the tile is the tile's last row, a sample past the grid is the grid's last
// column - so a block wholly beyond the grid has the range of the clamped column or row, and the strip's entry is the minimum and
// maximum over its 20 blocks, which is how it is made here.  A NaN makes its block {-inf, +inf}, and with it the strip.
// The wave works through the four row groups one after the other.  V: a lane's pieces of a group all lie in the same quarter of the
// row (rows of 8 bytes per sample: in one of two), so a quarter is reduced over the lanes that share it - 16 neighbouring lanes, a DPP
// row, for 4-byte samples - and nothing but the finished ranges goes through LDS.
template <bool V>
__global__ __launch_bounds__(256) void k_ranges(const GridView<sample_t> G, const Params P, const uint32_t nYT, const uint32_t nplanes, RangeEntry *out, RangeEntry *blocks) {
	constexpr uint32_t VS = 16u / (uint32_t)sizeof(sample_t);  // samples of a 16-byte piece
	struct alignas(16) Piece { sample_t s[VS]; };
	constexpr real_t INF = std::numeric_limits<real_t>::infinity();
	// The halo column of a strip is column 0 of the next one: a wave keeps the ranges of its column 0 apart and hands them to the wave
	// on its left through LDS; only a wave with no wave to its right in the block loads that column itself -
	// a 64-byte line per row for one sample, which for every strip was 12 % more traffic than the grid holds.
	__shared__ real_t s_col0[4][4][2];             // [wave][row group]{min, max} of column 0
	__shared__ real_t s_blk[4][RANGE_BLOCKS][2];   // [wave][entry]{min, max}
	const uint32_t lane = threadIdx.x & 63u, nXG = (P.nseg + 3u) / 4u, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint32_t xg = blockIdx.x % nXG, yt = (blockIdx.x / nXG) % nYT, pl = blockIdx.x / nXG / nYT;
	const uint32_t seg = xg * 4u + wv;
	const bool active = seg < P.nseg && pl < nplanes;  // (wave-uniform; an idle wave still comes to the barriers)
	const uint32_t xbase = seg * SEG_CELLS, y0 = yt * 63u, nrows = min(64u, P.ny + 1u - y0), xlast = min(xbase + SEG_CELLS, P.nx);
	const sample_t *base = G.p + (uint64_t)pl * G.slice + (uint64_t)y0 * G.pitch;
	const bool right = wv < 3u && seg + 1u < P.nseg;  // the wave to the right is active: it has this strip's halo column as its column 0, over the same rows
	auto take = [&](real_t &lo, real_t &hi, sample_t s) __attribute__((always_inline)) {
		const real_t f = (real_t)s;
		lo = real_min(lo, f); hi = f > hi ? f : hi;  // (a NaN changes neither)
#ifdef MC33_NAN_SAMPLES
		lo = f != f ? -INF : lo; hi = f != f ? INF : hi;
#endif
	};
	auto merge = [&](real_t &lo, real_t &hi, int dlt) __attribute__((always_inline)) {
		const real_t l2 = __shfl_xor(lo, dlt), h2 = __shfl_xor(hi, dlt);
		lo = real_min(lo, l2); hi = h2 > hi ? h2 : hi;
	};
	if (active) {
		const bool vec = V && xbase + SEG_CELLS - 1u <= P.nx;  // (wave-uniform)
#pragma unroll 1
		for (uint32_t g = 0; g < 4u; g++) {
			real_t lo0 = INF, hi0 = -INF;
			const bool past = 16u * g >= nrows;  // a row group wholly past a short tile is the tile's last row 16 times: one round of loads covers it
			if (vec) {
				constexpr uint32_t VR = SEG_CELLS / VS;           // pieces per row of the strip
				constexpr uint32_t NA = VR > 64u ? VR / 64u : 1u;  // quarters a lane's pieces fall into
				constexpr uint32_t GP = 16u * VR;                  // pieces of a row group
				constexpr uint32_t U = GP / 64u < 8u ? GP / 64u : 8u;  // loads in flight per lane
				static_assert(U % NA == 0u && GP % (64u * U) == 0u, "a round of loads covers whole rows");
				real_t lo[NA], hi[NA];
#pragma unroll
				for (uint32_t j = 0; j < NA; j++) { lo[j] = INF; hi[j] = -INF; }
				for (uint32_t e0 = 0; e0 < (past ? 64u * U : GP); e0 += 64u * U) {
					Piece v[U];
					bool first[U];
#pragma unroll
					for (uint32_t k = 0; k < U; k++) {
						const uint32_t e = e0 + 64u * k + lane;
						first[k] = (e % VR) == 0u;
						v[k] = *(const Piece *)(base + (uint64_t)min(16u * g + e / VR, nrows - 1u) * G.pitch + xbase + (e % VR) * VS);
					}
#pragma unroll
					for (uint32_t k = 0; k < U; k++) {
#pragma unroll
						for (uint32_t j = 0; j < VS; j++) take(lo[k % NA], hi[k % NA], v[k].s[j]);
						if (first[k]) take(lo0, hi0, v[k].s[0]);
					}
				}
#pragma unroll
				for (uint32_t j = 0; j < NA; j++) {
#pragma unroll
					for (int dlt = 32; dlt; dlt >>= 1)
						if ((uint32_t)dlt < VR / 4u || (uint32_t)dlt >= VR) merge(lo[j], hi[j], dlt);  // (the lanes whose pieces lie in the same quarter)
					const uint32_t q = (((64u * j + lane) % VR) * 4u) / VR;
					s_blk[wv][4u * g + q][0] = lo[j]; s_blk[wv][4u * g + q][1] = hi[j];  // (every lane of the quarter, the same words)
				}
			} else {
				real_t lo[4], hi[4];  // 64 samples of a row per load: a quarter
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++) { lo[q] = INF; hi[q] = -INF; }
				for (uint32_t e0 = 0; e0 < (past ? 8u : 64u); e0 += 8u) {
					sample_t v[8];
#pragma unroll
					for (uint32_t k = 0; k < 8u; k++)
						v[k] = base[(uint64_t)min(16u * g + ((e0 + k) >> 2), nrows - 1u) * G.pitch + min(xbase + 64u * (k & 3u) + lane, xlast)];
#pragma unroll
					for (uint32_t k = 0; k < 8u; k++) {
						take(lo[k & 3u], hi[k & 3u], v[k]);
						if (lane == 0u && (k & 3u) == 0u) take(lo0, hi0, v[k]);
					}
				}
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++) {
#pragma unroll
					for (int dlt = 32; dlt; dlt >>= 1) merge(lo[q], hi[q], dlt);
					if (lane == 0u) { s_blk[wv][4u * g + q][0] = lo[q]; s_blk[wv][4u * g + q][1] = hi[q]; }
				}
			}
#pragma unroll
			for (int dlt = 32; dlt; dlt >>= 1) merge(lo0, hi0, dlt);
			if (lane == 0u) { s_col0[wv][g][0] = lo0; s_col0[wv][g][1] = hi0; }
		}
		// The halo column - xlast: column 0 of the next segment, or the grid's last column where the strip ends at it or inside it -
		// is loaded by the wave that has no wave to its right in this block: lane r the sample of row r, a row group 16 lanes.
		if (!right) {
			real_t lo = INF, hi = -INF;
			take(lo, hi, base[(uint64_t)min(lane, nrows - 1u) * G.pitch + xlast]);
#pragma unroll
			for (int dlt = 8; dlt; dlt >>= 1) merge(lo, hi, dlt);
			if ((lane & 15u) == 0u) { s_blk[wv][16u + (lane >> 4)][0] = lo; s_blk[wv][16u + (lane >> 4)][1] = hi; }
		}
	}
	__syncthreads();
	if (active && right && lane < 4u) { s_blk[wv][16u + lane][0] = s_col0[wv + 1u][lane][0]; s_blk[wv][16u + lane][1] = s_col0[wv + 1u][lane][1]; }
	__syncthreads();
	if (!active) return;
	const uint64_t strip = ((uint64_t)pl * nYT + yt) * P.nseg + seg;
	real_t lo = INF, hi = -INF;
	if (lane < RANGE_BLOCKS) {
		lo = s_blk[wv][lane][0]; hi = s_blk[wv][lane][1];
		if (blocks) blocks[strip * RANGE_BLOCKS + lane] = RangeEntry{lo, hi};
	}
#pragma unroll
	for (int dlt = 16; dlt; dlt >>= 1) merge(lo, hi, dlt);  // (the entries sit in lanes 0 .. 19)
	if (lane == 0) out[strip] = RangeEntry{lo, hi};
}

// ---------------------------------------------------------------------------------------------------
// k_block_verdicts: the block verdicts of a single-isovalue sweep that goes by the live list - one 64-bit word per strip a live tile
// reads, [plane - G.z0][y tile][segment] like the tables (so the word does not depend on the plan): bits 2 j, 2 j + 1 for entry j of
// the strip's 20 blocks - 0 the block is live, 1 all its samples lie strictly below the isovalue, 2 all strictly above; both
// comparisons strict and in MC33_real, as k_tile_verdicts makes them and for the reasons given there.  A block per tile of the plan,
// half a wave per plane; the tiles k_tile_verdicts found dead have no words.  SweepArgs::skipped (timing level >= 1): words 4 .. 6
// count the blocks of live tiles, those left out below and those left out above.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_block_verdicts(const SweepArgs a, const uint8_t *verdict, const RangeEntry *blocks, unsigned long long *words) {
	const uint32_t j = threadIdx.x & 31u, half = threadIdx.x >> 5;  // (eight planes at a time: a tile of the flagship's plan is one round trip)
	const uint32_t t = blockIdx.x;
	if ((verdict[t >> 2] >> (t & 3u)) & 1u) return;  // (block-uniform: a dead tile)
	const SweepTile tile = a.tiles[t];
	const uint32_t p0r = tile.z_lo == a.P.zs ? tile.z_lo : tile.z_lo + 1u;
	const real_t v = a.lane[0].iso;
	for (uint32_t pp = p0r; pp <= tile.z_hi; pp += 8u) {
		const uint32_t p = pp + half;
		const bool there = p <= tile.z_hi;
		const uint64_t strip = ((uint64_t)(min(p, tile.z_hi) - a.G.z0) * a.sd.nYT + tile.yt) * a.sd.nseg + tile.seg;
		uint32_t code = 0u;
		if (there && j < RANGE_BLOCKS) {
			const RangeEntry e = blocks[strip * RANGE_BLOCKS + j];
			code = e.hi < v ? 1u : e.lo > v ? 2u : 0u;
		}
		uint32_t wlo = j < 16u ? code << (2u * j) : 0u, whi = j >= 16u ? code << (2u * (j - 16u)) : 0u;
#pragma unroll
		for (int dlt = 16; dlt; dlt >>= 1) { wlo |= (uint32_t)__shfl_xor((int)wlo, dlt); whi |= (uint32_t)__shfl_xor((int)whi, dlt); }
		if (there && j == 0u) {
			words[strip] = u64(wlo, whi);
			if (a.skipped) {
				atomicAdd(a.skipped + 4, RANGE_BLOCKS);
				atomicAdd(a.skipped + 5, (uint32_t)(__popc(wlo & 0x55555555u) + __popc(whi & 0x55u)));
				atomicAdd(a.skipped + 6, (uint32_t)(__popc(wlo & 0xAAAAAAAAu) + __popc(whi & 0xAAu)));
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------
// k_tile_verdicts / k_live_compact: which tiles of the plan the sweep with a range table (k_sweep) has to stream, decided in front
// of it.  A tile whose strips - of the planes it would READ, pl0 .. z_hi - all lie strictly above, or all strictly below, every
// isovalue of the pass holds no cut cell and no sample equal to an isovalue, and is not streamed.  Both comparisons are strict and
// made in MC33_real, on the values the sweep would have compared:
//   lo > iso: every sample F of the tile has F > iso, so d = iso - F is negative and NOT zero - the difference of two different
//     floating-point numbers is never zero while denormals are kept, and the code objects keep them (float_denorm_mode 3; no
//     flush-to-zero option in the build) - its sign bit is 1 (the integer forms classify by F > iso itself): all bits 1;
//   hi < iso: d is positive and not zero: all bits 0.
//   iso == +-0 against a sample +-0 compares equal: neither holds, the tile is streamed.  A NaN isovalue: neither holds.  A strip
//   with a NaN sample has {-inf, +inf}: neither holds for any isovalue.
// A wave of k_tile_verdicts per block of the sweep (four consecutive tiles of the plan).  Lane l looks at the strips of the planes
// pl0 + l, + 64, ...: one 8- / 16-byte load per lane, tile and 64 planes, the comparisons in the lane, one AND over the wave; the four
// tiles of a block the plan has grouped (the segments seg .. seg + 3 of one y tile over the same planes) are four neighbouring
// entries of the table per plane and take one pass.
// What a dead tile leaves behind is what a streamed one would have for k_boundary, and nothing else: the headers of the edge
// records of its first plane (when the tile below exists) and last plane (when a tile above does) - halo bits all 0 / all 1, no
// row and no lane with a sample equal to the isovalue, PLANE_UNIFORM0 / PLANE_UNIFORM1 (no record) - per isovalue lane.  No slice
// header (an older one carries an older epoch), nothing added to slot_part.
// The block's verdict is a byte: bit k, wave k has nothing to stream (its tile is dead, or the plan ends before it).  k_live_compact -
// ONE block - turns the bytes into the live list (SweepArgs::live) in plan order, which is ascending z_lo, the locality the plan's
// sort exists for: no atomic decides the order.  Both are ordered with the sweep by the stream and by nothing else.
// ---------------------------------------------------------------------------------------------------
// bit 2 NI k + 2 q of the result: all strips of tile k (k < nk: the segments seg0 + k over the planes of `tile`) lie below isovalue q; + 1: all above
template <int NI>
__device__ __forceinline__ uint32_t tile_sides(const SweepArgs &a, const SweepTile &tile, uint32_t seg0, uint32_t nk, uint32_t lane) {
	const uint32_t p0r = tile.z_lo == a.P.zs ? tile.z_lo : tile.z_lo + 1u;
	uint32_t m = 0xFFFFFFFFu;
	for (uint32_t p = p0r + lane; p <= tile.z_hi; p += 64u) {
		const RangeEntry *row = a.ranges + (((uint64_t)(p - a.G.z0) * a.sd.nYT + tile.yt) * a.sd.nseg + seg0);
		static_for<4>([&](auto kc) __attribute__((always_inline)) {
			constexpr int k = decltype(kc)::value;
			if ((uint32_t)k < nk) {  // (wave-uniform)
				const RangeEntry e = row[k];
				static_for<NI>([&](auto qc) __attribute__((always_inline)) {
					constexpr int q = decltype(qc)::value;
					const real_t v = a.lane[q].iso;
					m &= ~(((e.hi < v ? 0u : 1u) | (e.lo > v ? 0u : 2u)) << (2 * NI * k + 2 * q));
				});
			}
		});
	}
#pragma unroll
	for (int dlt = 32; dlt; dlt >>= 1) m &= (uint32_t)__shfl_xor((int)m, dlt);
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}
template <int NI>
__global__ __launch_bounds__(256) void k_tile_verdicts(const SweepArgs a, uint8_t *verdict, const uint32_t nblocks) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t b = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (b >= nblocks) return;
	const uint32_t t0 = b * 4u, nt = min(4u, a.ntiles - t0);
	SweepTile t[4];
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) t[k] = a.tiles[min(t0 + k, a.ntiles - 1u)];
	bool grouped = nt == 4u;  // (as k_sweep decides it)
#pragma unroll
	for (uint32_t k = 1; k < 4; k++) grouped = grouped && t[k].seg == t[0].seg + k && t[k].yt == t[0].yt && t[k].z_lo == t[0].z_lo && t[k].z_hi == t[0].z_hi;
	constexpr uint32_t EVEN = NI == 4 ? 0x55u : NI == 2 ? 0x5u : 0x1u, ALLQ = (1u << (2 * NI)) - 1u;
	uint32_t m = 0u;
	if (grouped) m = tile_sides<NI>(a, t[0], t[0].seg, 4u, lane);
	else
		static_for<4>([&](auto kc) __attribute__((always_inline)) {
			constexpr int k = decltype(kc)::value;
			if ((uint32_t)k < nt) m |= (tile_sides<NI>(a, t[k], t[k].seg, 1u, lane) & ALLQ) << (2 * NI * k);
		});
	uint32_t dead = 0u;
	static_for<4>([&](auto kc) __attribute__((always_inline)) {
		constexpr int k = decltype(kc)::value;
		if ((uint32_t)k >= nt) { dead |= 1u << k; return; }
		const uint32_t mine = (m >> (2 * NI * k)) & ALLQ;  // bit 2q: all strips of the tile below isovalue q; bit 2q + 1: all above
		if (((mine | mine >> 1) & EVEN) != EVEN) return;   // a tile is dead when each of its isovalues has one of its two bits
		dead |= 1u << k;
		if (lane == 0) {
			const bool has_below = t[k].z_lo != a.P.zs, has_above = t[k].z_hi < a.z_end;
			static_for<NI>([&](auto qc) __attribute__((always_inline)) {
				constexpr int q = decltype(qc)::value;
				const bool above = ((mine >> (2 * q)) & 2u) != 0u;
				const uint32_t hb = above ? 0xFFFFFFFFu : 0u;
				uint4 *h = a.lane[q].edge_hdr + (uint64_t)(t0 + k) * 2u * 2u;
				if (has_below) { h[0] = uint4{hb, hb, 0u, 0u}; h[1] = uint4{0u, 0u, above ? PLANE_UNIFORM1 : PLANE_UNIFORM0, 0u}; }
				if (has_above) { h[2] = uint4{hb, hb, 0u, 0u}; h[3] = uint4{0u, 0u, above ? PLANE_UNIFORM1 : PLANE_UNIFORM0, 0u}; }
			});
			if (NI == 1 && a.skipped) atomicAdd(a.skipped + ((mine & 2u) ? 2 : 1), 1u);
		}
	});
	if (lane == 0) verdict[b] = (uint8_t)(dead | (grouped ? MC33_VERDICT_GROUPED : 0u));  // (bit 4: what k_sweep_live need not find out again from four tiles)
}
// published (pinned host memory, nullptr: none): live TILES << 32 | tiles << 1 | plan, in ONE 8-byte store - what the host's choice
// between the two plans of a sweep with a table, and of the finer plan's size, goes by (table_plan, table_retarget), read there
// whenever it comes by, never waited for.
// Two lists are written.  live: word 0 the number of blocks of the plan with a live tile, then a word per such block, in plan
// order: block << 4 | its dead waves (mc33hip_sweep_live).  packed: what k_sweep_live goes by - words 0 .. 3 {entries, live tiles,
// tiles of the plan, 0}, the 16-byte entries (mc33_sweep_pack.h: whole blocks stay, the live tiles of mixed blocks go four to an
// entry), and behind room for nblocks entries a word per quad: where it goes.  Every thread walks a contiguous run of blocks, so
// an entry's place is two prefix sums (whole blocks, leftover tiles) - and the place of a quad is known to the thread that holds
// its FIRST tile only, which leaves it in memory for the threads that hold the others (one block: a barrier orders them).
__global__ __launch_bounds__(1024) void k_live_compact(const uint8_t *verdict, const uint32_t nblocks, uint32_t *live, uint32_t *packed, unsigned long long *published, const uint32_t plan, const uint32_t ntiles, const uint32_t lds_blocks) {
	constexpr uint32_t LDS_QUADS = 4096u;  // (plans of up to lds_blocks <= 4 096 blocks, 16 384 tiles, keep the places of their quads in LDS: a round trip to memory less in a kernel that is nothing but latency; MC33_HIP_LIST_LDS)
	__shared__ uint32_t s_wave[3][16], s_quad[LDS_QUADS];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	const uint32_t per = (nblocks + 1023u) / 1024u, b0 = min(tid * per, nblocks), b1 = min(b0 + per, nblocks);  // thread tid: the blocks b0 .. b1 - 1
	uint32_t val[3] = {0u, 0u, 0u};  // blocks with a live tile, whole blocks, leftover tiles (a wave past the plan's end counts as dead: k_tile_verdicts)
	for (uint32_t b = b0; b < b1; b++) {
		const uint32_t v = verdict[b] & 15u;
		val[0] += v != 15u ? 1u : 0u; val[1] += v == 0u ? 1u : 0u; val[2] += v == 0u ? 0u : 4u - (uint32_t)__popc(v);
	}
	uint32_t incl[3];
#pragma unroll
	for (int j = 0; j < 3; j++) {
		incl[j] = val[j];
#pragma unroll
		for (int dlt = 1; dlt < 64; dlt <<= 1) {
			const uint32_t o = __shfl_up(incl[j], dlt);
			incl[j] += lane >= (uint32_t)dlt ? o : 0u;
		}
		if (lane == 63u) s_wave[j][wv] = incl[j];
	}
	__syncthreads();
	uint32_t before[3], total[3];
#pragma unroll
	for (int j = 0; j < 3; j++) {
		before[j] = incl[j] - val[j]; total[j] = 0u;
		for (uint32_t w = 0; w < 16u; w++) { before[j] += w < wv ? s_wave[j][w] : 0u; total[j] += s_wave[j][w]; }
	}
	uint4 *ent = (uint4 *)(packed + 4);
	uint32_t *ent_w = packed + 4, *quad_at = nblocks <= min(lds_blocks, LDS_QUADS) ? s_quad : packed + 4u + 4u * (uint64_t)nblocks;  // (quads <= blocks)
	uint32_t at = before[0], W = before[1], L = before[2];
	for (uint32_t b = b0; b < b1; b++) {
		const uint32_t vb = verdict[b], v = vb & 15u;
		if (v != 15u) live[1u + at++] = b << 4 | v;
		if (v == 0u) { ent[pack_whole_at(W, L)] = uint4{(4u * b) | ((vb & MC33_VERDICT_GROUPED) ? MC33_PACK_GROUP : 0u), 4u * b + 1u, 4u * b + 2u, 4u * b + 3u}; W++; }
		else
			for (uint32_t k = 0; k < 4u; k++)
				if (!((v >> k) & 1u)) { if ((L & 3u) == 0u) quad_at[L >> 2] = pack_quad_at(L >> 2, W); L++; }
	}
	__syncthreads();
	L = before[2];
	for (uint32_t b = b0; b < b1; b++) {
		const uint32_t v = verdict[b] & 15u;
		if (v == 0u) continue;
		for (uint32_t k = 0; k < 4u; k++)
			if (!((v >> k) & 1u)) { ent_w[4u * (uint64_t)quad_at[L >> 2] + (L & 3u)] = 4u * b + k; L++; }
	}
	if (tid == 0) {
		const uint32_t Lt = total[2], tiles_live = 4u * total[1] + Lt;
		for (uint32_t s = Lt & 3u; s && s < 4u; s++) ent_w[4u * (uint64_t)quad_at[Lt >> 2] + s] = MC33_PACK_NONE;  // (only the last quad may be short)
		live[0] = total[0];
		packed[0] = total[1] + (Lt + 3u) / 4u; packed[1] = tiles_live; packed[2] = ntiles; packed[3] = 0u;
		if (published) __atomic_store_n(published, (unsigned long long)tiles_live << 32 | (unsigned long long)ntiles << 1 | (plan & 1u), __ATOMIC_RELAXED);
	}
}

// S: samples per lane and load.  S = 1: every lane loads single samples (all types); S = SWEEP_PACK > 1: dwords of 2
// unsigned shorts / 4 unsigned chars - needs rows that start on a dword boundary (the host checks), and makes a batch
// 8 / 16 sample rows instead of 4, so that a wave keeps the same 16 x 256 bytes in flight.
// ZM: how a sample is classified.  0: d = iso - F, its sign bit and d == 0, exactly as the reference writes it (float and
// double samples - NaN samples, signed zeros - and the isovalue -0.0).  Integer samples (MC33_INT_SAMPLES) otherwise: the
// sign bit of iso - F is F > iso and iso - F == 0 is F == iso (both converted to MC33_real as the reference does), so the
// subtraction, the |d| and the running minimum go: 1: one compare for the sign, one for "equals the isovalue"; 2: no
// isovalue of the pass is an integer of the sample type's range - nothing can equal it, one compare per sample and isovalue
// (the 4-isovalue pass over ushort samples is bound by its instructions: 94 -> 58 per sample row).
// R: what the kernel knows of the range table.  0 (k_sweep_all, what a sweep without a table launches - a volatile grid, the first
// sweep over new samples, MC33_HIP_RANGES=0): nothing; block b streams the tiles 4 b .. 4 b + 3 and the body is the one the kernel
// had before there was a table, instruction for instruction: code for the table being THERE cost the packed passes over several
// isovalues 3 % whether or not it ran (profiles/r08_range_skip.txt D), and a caller without a table pays nothing for it.
// 1 (k_sweep): every wave works out its verdict itself, in a preamble - plans of less than one round of the device (small grids).
// 2 (k_sweep_live): the verdicts were made in front of the kernel, and block blockIdx.x streams the four tiles of entry blockIdx.x
// of the packed live list - plans of one round and more, whose live tiles have to fill the device by themselves: four to a block,
// so that no block holds wave slots for dead tiles.
template <int S, int NI, int ZM, int R, bool BLOCKS = false>
__device__ __forceinline__ void sweep_tile(const SweepArgs &a) {
	constexpr int LPR = 4 / S;    // loads per sample row
	constexpr int RB = 16 / LPR;  // sample rows per batch
	const uint32_t lane = threadIdx.x & 63u;
	// R: the block's tiles come from the packed live list.  The launch is one block per planned block; those beyond the list
	// end here, at their first instructions.  A wave without a tile in a block that has some (the last quad of the list; R == 1: a
	// dead tile) does not return here (a second exit gave the packed forms over several isovalues a quarter more SGPRs parked in VGPR
	// lanes): it has no batches - T = 0 below - so it walks past the loop, flushes an empty log, and ends where every wave ends.  The one batch issued ahead of the loop goes
	// through a descriptor of zero bytes: no memory access.
	uint32_t wtile = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform, in an SGPR
	bool whole = true;  // (block-uniform) R == 2: the block's entry is a whole group of the plan
	bool dead_me = false;
	if constexpr (R == 2) {
		// (a.live: the packed list - its entry gives every wave of the block its tile of the plan, any four live tiles in plan order, and
		// says whether they are a group the plan made: nothing is read from the other three tiles)
		if (blockIdx.x >= a.live[0]) return;
		const uint4 e = ((const uint4 *)a.live)[1u + blockIdx.x];
		const uint32_t wme = wtile & 3u, first = e.x & ~MC33_PACK_GROUP;
		const uint32_t mine = wme == 0u ? first : wme == 1u ? e.y : wme == 2u ? e.z : e.w;
		dead_me = mine == MC33_PACK_NONE;  // (the last quad of a list: such a wave walks through with the entry's first tile and T = 0)
		wtile = dead_me ? first : mine;
		whole = (e.x & MC33_PACK_GROUP) != 0u;
	}
	if (wtile >= a.ntiles) return;
	const SweepTile tile = a.tiles[wtile];
	const uint32_t yt = tile.yt, seg = tile.seg;
	const Params &P = a.P;
	// The halo column (the first sample of the next row segment, one per row) used to be a load of its own: RB lanes of a
	// batch each touching a different line for ONE sample - 8 % of the sweep's fabric reads at 1024^3 float, 15 % on the
	// ushort grid of configs[4], two thirds of them missing L2 (the main loads are non-temporal), 6 % of the float sweep's
	// time (tools/halo_cost.sh, profiles/r03_halo_cost_before.txt / r03_halo_cost_after.txt).  When the four waves of a block are the four segments of one
	// 1024-sample group over the same rows and planes (the plan makes them so wherever the grid allows), wave k gets the bit
	// from wave k + 1, which has just classified that very sample: every wave posts the column-0 bits of the plane it has
	// completed (one ballot) in an LDS mailbox, one block barrier per PLANE (the four waves run in step anyway: a plane is
	// ~270 loads), and only the last segment of the group still loads its halo.  All four waves complete the same number
	// of planes (same rows, same z range), so every wave reaches every barrier; blocks of unrelated tiles keep the load.
	bool grouped = true;
	if constexpr (R == 2) grouped = whole;  // (any other entry runs ungrouped: its live waves load their own halo column, and there is no barrier in it)
	else {
		const uint32_t t0 = wtile & ~3u;
		if (t0 + 3u >= a.ntiles) grouped = false;
		else {
			const SweepTile first = a.tiles[t0];
#pragma unroll
			for (uint32_t k = 1; k < 4; k++) {
				const SweepTile o = a.tiles[t0 + k];
				grouped = grouped && o.seg == first.seg + k && o.yt == first.yt && o.z_lo == first.z_lo && o.z_hi == first.z_hi;
			}
		}
	}
	const unsigned long long t_start = a.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;
	const unsigned long long c_start = a.trace ? __builtin_amdgcn_s_memtime() : 0ull;
	// R == 1, the preamble: the verdicts (see k_tile_verdicts for the arithmetic - it is the same) worked out by the wave itself, for
	// plans of less than one round of the device, where two small launches in front of the sweep cost more than they give.  Lane l
	// looks at the strips of the planes pl0 + l, + 64, ...; every wave of a block that could be grouped works out the verdicts of all
	// four tiles - the same four computations in all four waves, so the result is block-uniform - and a block with a dead tile runs
	// UNGROUPED.  A dead wave leaves the headers of its edge records from lane 0 and has no batches (T = 0 below).
	if (R == 1 && a.ranges) {
		const uint32_t wme = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		// (a grouped block: the four tiles are the segments seg .. seg + 3 of one y tile over the same planes - four neighbouring
		// entries of the table per plane, all four verdicts from one pass; any other block: the wave's own tile only)
		const uint32_t seg0 = grouped ? seg - wme : seg, nk = grouped ? 4u : 1u, me = grouped ? wme : 0u;
		const uint32_t p0r = tile.z_lo == a.P.zs ? tile.z_lo : tile.z_lo + 1u;
		uint32_t m = 0xFFFFFFFFu;  // bit 2 NI k + 2 q: all strips of tile k of the block lie below isovalue q; + 1: all above
		for (uint32_t p = p0r + lane; p <= tile.z_hi; p += 64u) {
			const RangeEntry *row = a.ranges + (((uint64_t)(p - a.G.z0) * a.sd.nYT + yt) * a.sd.nseg + seg0);
			static_for<4>([&](auto kc) __attribute__((always_inline)) {
				constexpr int k = decltype(kc)::value;
				if ((uint32_t)k < nk) {  // (wave-uniform)
					const RangeEntry e = row[k];
					static_for<NI>([&](auto qc) __attribute__((always_inline)) {
						constexpr int q = decltype(qc)::value;
						const real_t v = a.lane[q].iso;
						m &= ~(((e.hi < v ? 0u : 1u) | (e.lo > v ? 0u : 2u)) << (2 * NI * k + 2 * q));
					});
				}
			});
		}
#pragma unroll
		for (int dlt = 32; dlt; dlt >>= 1) m &= (uint32_t)__shfl_xor((int)m, dlt);
		m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
		// a tile is dead when each of its isovalues has one of its two bits
		constexpr uint32_t EVEN = NI == 4 ? 0x55u : NI == 2 ? 0x5u : 0x1u, ALLQ = (1u << (2 * NI)) - 1u;
		const uint32_t one_side = (m | m >> 1);  // bit 2 NI k + 2 q: isovalue q of tile k has a side
		bool dead_any = false;
		static_for<4>([&](auto kc) __attribute__((always_inline)) {
			constexpr int k = decltype(kc)::value;
			if ((uint32_t)k < nk) dead_any = dead_any || ((one_side >> (2 * NI * k)) & EVEN) == EVEN;
		});
		const uint32_t mine = (m >> (2u * NI * me)) & ALLQ;  // bit 2q: all strips of this wave's tile below isovalue q; bit 2q + 1: all above
		dead_me = ((mine | mine >> 1) & EVEN) == EVEN;
		if (dead_any) grouped = false;
		if (dead_me) {
			if (lane == 0) {
				static_for<NI>([&](auto qc) __attribute__((always_inline)) {
					constexpr int q = decltype(qc)::value;
					const bool above = ((mine >> (2 * q)) & 2u) != 0u;
					const uint32_t hb = above ? 0xFFFFFFFFu : 0u;
					uint4 *h = a.lane[q].edge_hdr + (uint64_t)wtile * 2u * 2u;
					if (p0r != tile.z_lo) { h[0] = uint4{hb, hb, 0u, 0u}; h[1] = uint4{0u, 0u, above ? PLANE_UNIFORM1 : PLANE_UNIFORM0, 0u}; }
					if (tile.z_hi < a.z_end) { h[2] = uint4{hb, hb, 0u, 0u}; h[3] = uint4{0u, 0u, above ? PLANE_UNIFORM1 : PLANE_UNIFORM0, 0u}; }
				});
				if (NI == 1 && a.skipped) atomicAdd(a.skipped + ((mine & 2u) ? 2 : 1), 1u);
			}
		}
	}
	__shared__ uint64_t s_mail[2][4][NI][2];  // [plane parity][wave][isovalue]{column-0 bits of the rows, rows whose column-0 sample may equal the isovalue}
	const bool from_right = grouped && (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) < 3u;  // this wave's halo bits come from the wave to its right
	const uint32_t xbase = seg * SEG_CELLS, y0 = yt * 63u;
	const uint32_t nrows = min(64u, P.ny + 1 - y0);  // sample rows of this tile
	const uint32_t z_lo = tile.z_lo, z_hi = tile.z_hi;
	const uint32_t pl0 = z_lo == P.zs ? z_lo : z_lo + 1u;  // first plane this tile reads
	const bool has_above = z_hi < a.z_end;

	// per-lane byte offsets of its loads inside a row (clamped into the row: bits of samples beyond the grid belong
	// to cells that the valid masks remove)
	const uint32_t rowbytes = a.G.pitch * (uint32_t)sizeof(sample_t);
	uint32_t xo[LPR];
#pragma unroll
	for (int k = 0; k < LPR; k++)
		xo[k] = S == 1 ? min(xbase + 64u * k + lane, P.nx) * (uint32_t)sizeof(sample_t)
		               : min(xbase + (256u / LPR) * k + (uint32_t)S * lane, P.nx & ~(uint32_t)(S - 1)) * (uint32_t)sizeof(sample_t);
	uint64_t valid[4];
	{
		uint64_t vstd[4];
		valid_masks(xbase, P.nx, vstd);
		from_standard<S>(vstd, valid);
	}
	const bool rowvalid = lane < 63u && y0 + lane < P.ny;
	// halo column: lane r needs the first sample of the next segment in row r; it is fetched by the batch
	// that holds row r (RB lanes per batch; the other lanes aim outside the descriptor: no memory access)
	const uint32_t xh = min(lane, nrows - 1) * rowbytes + min(xbase + SEG_CELLS, P.nx) * (uint32_t)sizeof(sample_t);

	// sign bits of the tile: word k of sample row r lives in lane r (layout S).  *_h: the halo sample's bit;
	// *_z (wave-uniform): "some sample of this plane of the tile (halo included) equals the isovalue"
	// (one set per isovalue lane; with 4 lanes the bit rows of the plane below wait in LDS - they are touched once per
	// plane, and in registers they cost the kernel a third of its waves)
	constexpr bool PREV_LDS = NI >= 4;
	__shared__ uint64_t s_prev[PREV_LDS ? NI : 1][4][PREV_LDS ? 256 : 1];
	__shared__ uint64_t s_prevz[PREV_LDS ? NI : 1][2][4];  // ... and its 'sample equals the isovalue' row / lane masks, per wave
	__shared__ uint32_t s_prevh[PREV_LDS ? NI : 1][PREV_LDS ? 256 : 1];  // ... and its halo-column bits
	constexpr bool DEFER = NI == 1;   // the hand-over goes through the wave's log in LDS (SweepLog)
	__shared__ typename std::conditional<DEFER, SweepLog, uint32_t>::type s_log[DEFER ? 4 : 1];
	uint32_t log_np = 0, log_ns = 0, log_edge = LOG_NONE;  // planes / slices in the log; the format of the pending first edge record (wave-uniform)
	uint32_t pend_chunk[NI];            // (NI >= 2) partial sums not yet added to memory: their chunk of slots ...
	unsigned long long pend_sum[NI];    // ... batches << 32 | cells (wave-uniform)
#pragma unroll
	for (int q = 0; q < NI; q++) { pend_chunk[q] = 0u; pend_sum[q] = 0ull; }
	const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	uint64_t cur[NI][4], prev[PREV_LDS ? 1 : NI][4];
	uint64_t c64[NI][4];  // the rows being assembled
	uint32_t cur_h[NI], prev_h[PREV_LDS ? 1 : NI];
	uint64_t cur_zc[NI], prev_zc[PREV_LDS ? 1 : NI], zcacc[NI];  // ... and the lanes that loaded one
	uint64_t cur_z[NI], prev_z[PREV_LDS ? 1 : NI], zacc[NI];  // sample rows of the plane that hold a sample equal to the isovalue (wave-uniform),
	                                           // to the batch of RB rows: one compare per batch, not per row
	constexpr bool ZMIN_REG = !(sizeof(real_t) == 8 && NI >= 4);
	real_t zmin[NI];  // min |iso - F| over the lane's samples of the batch being processed (ZM = 0, ZMIN_REG)
	uint64_t zeq[NI]; // lanes that loaded a sample equal to the isovalue in the batch being processed (ZM = 1, or ZM = 0 without ZMIN_REG; wave-uniform)
	bool cur_written[NI], prev_written[NI];  // the plane's bit rows are already in slice_bits
	real_t iso[NI];
#pragma unroll
	for (int q = 0; q < NI; q++) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if constexpr (PREV_LDS) s_prev[q][k][threadIdx.x] = 0; else prev[q][k] = 0;
			c64[q][k] = 0;
		}
		cur_h[q] = 0; cur_z[q] = zacc[q] = 0; cur_zc[q] = zcacc[q] = 0;
		if constexpr (PREV_LDS) { s_prevz[q][0][wv] = 0; s_prevz[q][1][wv] = 0; s_prevh[q][threadIdx.x] = 0; } else { prev_z[q] = 0; prev_zc[q] = 0; prev_h[q] = 0; }
		cur_written[q] = prev_written[q] = false; zmin[q] = 1; zeq[q] = 0;
		iso[q] = a.lane[q].iso;
	}

	// The tile is consumed as a linear stream of batches of RB sample rows (16 coalesced 256-byte loads per
	// wave), plane after plane.  Two register buffers: the loads of batch t+1 are in flight while batch t
	// is turned into bit rows.  Loads go through a buffer descriptor per plane (scalar base + 32-bit
	// offsets, hardware range check).
	const uint32_t NB = (nrows + (uint32_t)RB - 1u) / (uint32_t)RB;
	const uint32_t T = dead_me ? 0u : (z_hi - pl0 + 1u) * NB;  // (a tile the range table rules out: nothing to stream)
	const uint32_t tile_bytes = dead_me ? 0u : nrows * rowbytes;
// Cache policy of the sweep's loads (every sample is read once).  `nt` (aux bit 1) for 4- and 8-byte samples: 0.866 - 0.875 ->
// 0.78 - 0.85 ms at 1024^3 float over four processes each way; the narrow types, whose sweep is bound by instructions rather
// than by the stream, lose with it (ushort 4-isovalue pass + 1.5 %, uchar + 10 %) and keep the default.
#ifndef MC33_SWEEP_AUX
#if defined(MC33_GRD_U16) || defined(MC33_GRD_U8)
#define MC33_SWEEP_AUX 0
#else
#define MC33_SWEEP_AUX 2
#endif
#endif
#if defined(MC33_GRD_U16)
#define MC33_LOAD(rs, vo, so) ((float)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, vo, so, MC33_SWEEP_AUX))
#elif defined(MC33_GRD_U8)
#define MC33_LOAD(rs, vo, so) ((float)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, vo, so, MC33_SWEEP_AUX))
#elif defined(MC33_GRD_U32)
#define MC33_LOAD(rs, vo, so) ((float)(uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, vo, so, MC33_SWEEP_AUX))
#elif defined(MC33_GRD_F64)
#define MC33_LOAD(rs, vo, so) (__builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, so, MC33_SWEEP_AUX)))
#else
#define MC33_LOAD(rs, vo, so) (__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, vo, so, MC33_SWEEP_AUX)))
#endif
	typedef typename std::conditional<S == 1, real_t, uint32_t>::type raw_t;  // what a load leaves in a register
	// BS: dead blocks inside the live tile are left out (k_block_verdicts): this form has a batch stream of its own, below (`the block
	// stream`) - a batch is one live block of the plane, and the word of the plane (block_word) says which those are, what the bit rows
	// of the dead ones are worth and what their halo samples.  A kernel of its own (k_sweep_live_blocks) has this form: k_sweep_live stays
	// the code it was, for the sweeps without words.  No word (SweepArgs::blockw == nullptr): every block is live.
	constexpr bool BS = BLOCKS;
	static_assert(!BLOCKS || (MC33_BLOCK_SKIP && R == 2 && NI == 1 && S == 1), "blocks are left out by the float single-isovalue sweep with a live list");
	auto block_word = [&](uint32_t p) __attribute__((always_inline)) -> uint64_t {
		if constexpr (BS) {
			if (a.blockw) {
				// (through the constant address space - the words were written in front of this kernel and nothing in it writes them: a SCALAR
				// load, which the waits of the batches in flight do not count.  As a global load behind the kernel's stores it was a vector
				// load, and the wave waited for it with vmcnt(0): every batch in flight drained once per plane.)
				typedef const __attribute__((address_space(4))) unsigned long long *const_words_t;
				return ((const_words_t)(uintptr_t)a.blockw)[((uint64_t)(min(p, z_hi) - a.G.z0) * a.sd.nYT + yt) * a.sd.nseg + seg];
			}
		}
		return 0ull;
	};
	// A batch is the same number of loads whatever the position in the tile, so that the wait counts the compiler derives keep
	// the prefetched batch in flight: exactly 17 in the forms that always issue the halo load (several isovalues, double
	// samples); 16 or 17 in the single-isovalue forms over 1- to 4-byte samples, whose halo load stands behind a branch (below)
	auto issue = [&](raw_t (&d)[16], real_t &hv, uint32_t p, uint32_t bi) __attribute__((always_inline)) {
		const sample_t *base = a.G.p + (uint64_t)(p - a.G.z0) * a.G.slice + (uint64_t)y0 * a.G.pitch;
		const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, tile_bytes, 0x00020000);
		const uint32_t r = bi * (uint32_t)RB;
#pragma unroll
		for (int rr = 0; rr < RB; rr++) {
			const uint32_t so = min(r + rr, nrows - 1) * rowbytes;
#pragma unroll
			for (int k = 0; k < LPR; k++) {
				if constexpr (S == 1) d[rr * LPR + k] = MC33_LOAD(rs, xo[k], so);
				else d[rr * LPR + k] = __builtin_amdgcn_raw_buffer_load_b32(rs, xo[k], so, MC33_SWEEP_AUX);
			}
		}
		// (MC33_HIP_DEBUG 64, developer builds: no halo sample is ever fetched - what the one-sample-per-row load costs the stream)
		if constexpr (NI == 1 && sizeof(real_t) == 4) {  // (double samples: the form costs k_sweep<1, 1, 0> its 129th register - they keep the old one)
			// The 17th load under a lane condition: a lane that is switched off costs the memory pipeline nothing, a lane that is
			// refused by the descriptor's range check does (the same measurement as at `fetch` in mc33_emit.hip.h) - and until round 7
			// 60 lanes of this load were refused in the waves that need it, all 64 in the three waves of a grouped block that take
			// their halo bits from the mailbox.  What the compiler makes of it (read in the gfx950 code of k_sweep<1, 1, 0>):
			// s_and_saveexec_b64 / s_cbranch_execz around the load - it keeps such a branch around any memory instruction - so a wave
			// whose lanes all stay out (from_right) issues 16 loads per batch, every other wave 17 with four lanes on, and the waits
			// are derived for the smaller number: vmcnt(16) where the old form had vmcnt(17).  Exact for the three mailbox waves of a
			// grouped block; a wave that does load its halo - the fourth of a grouped block, every wave of an ungrouped one (grids
			// narrower than four row segments, the segments behind the last whole group) - waits until the FIRST load of the
			// prefetched batch has come back as well, the other 16 still in flight.  Two copies of the batch loop, one per kind of
			// wave, would make the counts exact in both and double a 30 KB kernel; measured instead, grouped and ungrouped shapes:
			// profiles/r07_dead_time.txt.  The lanes left out keep the value they had, which `process` does not look at.
			const bool wanted = ((lane / (uint32_t)RB) == bi) & !from_right & !(MC33_DEBUG_BITS(a) & 64u);
			if (wanted) hv = MC33_LOAD(rs, xh, 0u);
		} else
		hv = MC33_LOAD(rs, ((lane / (uint32_t)RB) == bi && !from_right && !(MC33_DEBUG_BITS(a) & 64u)) ? xh : 0xFFFFFFF0u, 0u);
	};
	// the four samples of row rr of a batch in word order of layout S
	auto sample = [&](const raw_t (&dd)[16], int rr, int k) -> real_t {
		if constexpr (S == 1) return dd[rr * 4 + k];
		else if constexpr (S == 2) return (real_t)((dd[rr * 2 + (k >> 1)] >> (16 * (k & 1))) & 0xFFFFu);
		else return (real_t)((dd[rr] >> (8 * k)) & 0xFFu);
	};

	// Packed narrow samples against an isovalue without converting them (ZM 1, 2): F > iso is F > floor(iso) in integers -
	// one compare on the halfword / byte where it sits in the loaded dword instead of a conversion and a compare (the
	// 4-isovalue pass over ushort samples is bound by its instructions).
	// (the integer words come with the kernel arguments: SweepLane::iso_gt / iso_eq)
	auto raw_sample = [&](const raw_t (&dd)[16], int rr, int k) -> uint32_t {  // (S >= 2) the sample as it was loaded
		if constexpr (S == 2) return ((uint32_t)dd[rr * 2 + (k >> 1)] >> (16 * (k & 1))) & 0xFFFFu;
		else if constexpr (S == 4) return ((uint32_t)dd[rr] >> (8 * k)) & 0xFFu;
		else return 0u;
	};
	// ---- the wave's log of what it hands on (DEFER; see SweepLog) ----
	auto log_flush = [&]() __attribute__((always_inline)) {
		if constexpr (DEFER) {
			SweepLog &G = s_log[wv];
			const SweepLane &L0 = a.lane[0];
			const uint32_t ln = fresh_lane();
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			for (uint32_t k = 0; k < log_np; k++) {  // wave-uniform
				const uint64_t slot = readlane64(G.plane_slot[k], 0);
				__builtin_amdgcn_raw_buffer_store_b32(G.plane[k][ln], record_rsrc(L0.slice_compact + slot * 64u, 256u), ln * 4u, 0u, 0);
				if (ln == 0) L0.plane_fmt[slot] = (uint8_t)PLANE_COMPACT;
			}
			{  // a lane per slice: its header; the partial sums (k_slots) added up per chunk of slots first - the slices of a tile come in
				// rising slot order, so the slices of one chunk are neighbouring lanes, and the first of them adds for all (a tile's 6
				// cut slices lie in 1 - 2 chunks: a third of the atomics, all of which arrive in the kernel's last microseconds)
				const bool mine = ln < log_ns;
				const uint32_t e = mine ? ln : 0u;
				const uint32_t *w = G.hdr[e];
				const uint64_t slot = G.hdr_slot[e];
				if (mine) {
					uint32_t *h = (uint32_t *)(L0.slice_hdr + slot);
					*(uint4 *)h = uint4{w[0], w[1], w[2], w[3]};
					*(uint4 *)(h + 4) = uint4{w[4], w[5], w[6], w[7]};
					*(uint2 *)(h + 8) = uint2{w[8], w[9]};
				}
				const uint32_t chunk = mine ? (uint32_t)(slot / SLOT_CHUNK) : 0xFFFFFFFFu;
				const uint32_t cells = mine ? w[5] : 0u, batches = mine ? w[10] : 0u;
				uint32_t sum_c = cells, sum_b = batches;
#pragma unroll 1  // (rolled: unrolled, its 57 cross-lane reads were all asked for at once and cost the kernel a wave per SIMD)
				for (uint32_t dlt = 1; dlt < log_ns; dlt++) {
					const uint32_t c2 = __shfl_down(chunk, dlt), v2 = __shfl_down(cells, dlt), b2 = __shfl_down(batches, dlt);
					const bool same = c2 == chunk && ln + dlt < 64u;
					sum_c += same ? v2 : 0u; sum_b += same ? b2 : 0u;
				}
				const uint32_t before = __shfl_up(chunk, 1);
				if (mine && (ln == 0u || before != chunk)) atomicAdd(L0.slot_part + chunk, (unsigned long long)sum_b << 32 | sum_c);
			}
			if (log_edge != LOG_NONE) {  // the first plane's edge record: compact, or wholly on one side (header only)
				if (log_edge == PLANE_COMPACT) __builtin_amdgcn_raw_buffer_store_b32(G.edge[ln], record_rsrc(L0.edge_bits + (uint64_t)wtile * 2u * 128u, 2048u), ln * 4u, 0u, 0);
				if (ln == 0) {
					const uint32_t *e = G.edge_hdr;
					L0.edge_hdr[(uint64_t)wtile * 2u * 2u] = uint4{e[0], e[1], e[2], e[3]};
					L0.edge_hdr[(uint64_t)wtile * 2u * 2u + 1u] = uint4{e[4], e[5], e[6], e[7]};
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the log is written again)
			log_np = 0; log_ns = 0; log_edge = LOG_NONE;
		}
	};
	// a plane of a cut slice: into the log when it has the compact form, to memory at once when it needs the raw one
	auto log_plane = [&](uint64_t slot, const uint64_t (&w)[4], uint32_t ln) __attribute__((always_inline)) {
		if constexpr (DEFER) {
			uint32_t desc;
			if (encode_plane<S>(w, desc)) {  // (wave-uniform)
				if (log_np == LOG_PLANES) log_flush();
				SweepLog &G = s_log[wv];
				G.plane[log_np][ln] = desc;
				if (ln == 0) G.plane_slot[log_np] = slot;
				log_np++;
			} else {
				store_plane_raw<S>(a.lane[0].slice_bits + slot * 128u, w, ln);
				if (ln == 0) a.lane[0].plane_fmt[slot] = (uint8_t)PLANE_RAW;
			}
		}
	};
	auto log_header = [&](uint64_t slot, uint64_t bp, uint64_t bc, uint64_t zrows, uint64_t zcols, const uint64_t (&act)[4], uint32_t ln) __attribute__((always_inline)) {
		if constexpr (DEFER) {
			uint32_t ncell = __popcll(act[0]) + __popcll(act[1]) + __popcll(act[2]) + __popcll(act[3]);
#pragma unroll
			for (int dlt = 32; dlt; dlt >>= 1) ncell += __shfl_xor(ncell, dlt);
			if (log_ns == LOG_SLICES) log_flush();
			if (ln == 0) {
				SweepLog &G = s_log[wv];
				uint32_t *w = G.hdr[log_ns];
				w[0] = a.lane[0].epoch << 2 | SLICE_VALID | (zrows ? SLICE_HAS_ISO : 0u);
				w[1] = (uint32_t)bp; w[2] = (uint32_t)(bp >> 32); w[3] = (uint32_t)bc; w[4] = (uint32_t)(bc >> 32); w[5] = ncell;
				w[6] = (uint32_t)zrows; w[7] = (uint32_t)(zrows >> 32); w[8] = (uint32_t)zcols; w[9] = (uint32_t)(zcols >> 32);
				w[10] = (ncell + 63u) >> 6;  // the records of a slice are handed to the emit passes 64 at a time (BatchDesc)
				G.hdr_slot[log_ns] = slot;
			}
			log_ns++;
		}
	};
	real_t halo = 0;  // lane r: halo sample of row r of the plane being assembled
	// (always_inline: the body is called twice, and in the largest forms - packed uchar samples, four isovalues, equality tests - the
	// compiler made a real FUNCTION of it, every captured array behind a pointer into 1.5 KiB of scratch memory per lane)
	auto process = [&](const raw_t (&dd)[16], const real_t &hv, uint32_t p, uint32_t bi) __attribute__((always_inline)) {
		const uint32_t r = bi * (uint32_t)RB;
		if constexpr (!BS) {  // (the block form has its own batches - process_next - and comes here, with bi = NB - 1, for the completion of a plane alone)
		halo = (lane / (uint32_t)RB) == bi ? hv : halo;
		unrolled_for<RB, (S >= 4)>([&](auto rc) __attribute__((always_inline)) {
			const int rr = rc;
			real_t f[4];
#pragma unroll
			for (int k = 0; k < 4; k++) f[k] = sample(dd, rr, k);
			uint64_t bwq[NI][4];  // (NI >= 2: the ballots of the row for all isovalues, parked two isovalues per EXEC switch)
			static_for<NI>([&](auto qc) __attribute__((always_inline)) {
				constexpr int q = decltype(qc)::value;
				uint64_t bw[4];
#pragma unroll
				for (int k = 0; k < 4; k++) {
					uint64_t bb;
					if constexpr (ZM == 0) {
						const real_t d = iso[q] - f[k];                       // MC:1852-1855
						bb = __ballot(sign_of(d) != 0);                       // MC:1856-1859 (sign bit)
#ifdef MC33_NAN_SAMPLES
						bb ^= __ballot(d != d);  // NaN sample: the sign the reference sees is the NaN's own (see iso_diff)
#endif
						// "equals the isovalue": a running minimum of |d| per lane, looked at once per batch (one instruction per sample) -
						// except in the double-precision pass over four isovalues, which has no four register pairs for it: a compare
						// per sample there, gathered in SGPRs
						if constexpr (ZMIN_REG) zmin[q] = real_min(zmin[q], real_abs(d));
						else zeq[q] |= __ballot(d == 0);
					} else if constexpr (S >= 2) {
						const uint32_t ri = raw_sample(dd, rr, k);
						bb = __ballot((int32_t)ri > a.lane[q].iso_gt);
						if constexpr (ZM == 1) zeq[q] |= __ballot(ri == a.lane[q].iso_eq);
					} else {
						bb = __ballot(f[k] > iso[q]);                         // = the sign bit of iso - F for an integer sample
						if constexpr (ZM == 1) zeq[q] |= __ballot(f[k] == iso[q]);
					}
					bw[k] = bb;
				}
				// park the bit row of sample row r+rr in lane r+rr
				// (references and the row number named here: operands of an asm statement do not capture by themselves inside a generic lambda;
				// the row number through readfirstlane - uniform anyway, but short of SGPRs the compiler moved the batch counter into
				// a vector register and handed THAT to the "s" operand)
				const uint32_t rowsel = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r + (uint32_t)rr));
				if constexpr (NI >= 2) {
#pragma unroll
					for (int k = 0; k < 4; k++) bwq[q][k] = bw[k];
				} else {
					// EXEC = that one lane, four 64-bit moves from the SGPR pairs, EXEC back (it is all ones here: the wave's control flow is
					// uniform; saved and restored all the same).  SALU writes of EXEC need no wait states before a VALU instruction.
					uint64_t &w0 = c64[q][0], &w1 = c64[q][1], &w2 = c64[q][2], &w3 = c64[q][3];
					uint64_t saved;
					asm volatile(
					    "s_mov_b64 %4, exec\n\t"
					    "s_lshl_b64 exec, 1, %9\n\t"
					    "v_mov_b64 %0, %5\n\tv_mov_b64 %1, %6\n\tv_mov_b64 %2, %7\n\tv_mov_b64 %3, %8\n\t"
					    "s_mov_b64 exec, %4"
					    : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3), "=&s"(saved)
					    : "s"(bw[0]), "s"(bw[1]), "s"(bw[2]), "s"(bw[3]), "s"(rowsel)
					    : "scc");  // (s_lshl_b64 sets SCC: without the clobber the compiler carried a loop condition across the statement in it)
				}
			});
			if constexpr (NI >= 2) {
				static_for<NI / 2>([&](auto hc) __attribute__((always_inline)) {
					constexpr int q0 = 2 * decltype(hc)::value;
					const uint32_t rowsel = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r + (uint32_t)rr));
					uint64_t &w0 = c64[q0][0], &w1 = c64[q0][1], &w2 = c64[q0][2], &w3 = c64[q0][3];
					uint64_t &w4 = c64[q0 + 1][0], &w5 = c64[q0 + 1][1], &w6 = c64[q0 + 1][2], &w7 = c64[q0 + 1][3];
					const uint64_t b0 = bwq[q0][0], b1 = bwq[q0][1], b2 = bwq[q0][2], b3 = bwq[q0][3];
					const uint64_t b4 = bwq[q0 + 1][0], b5 = bwq[q0 + 1][1], b6 = bwq[q0 + 1][2], b7 = bwq[q0 + 1][3];
					uint64_t saved;
					asm volatile(
					    "s_mov_b64 %8, exec\n\t"
					    "s_lshl_b64 exec, 1, %17\n\t"
					    "v_mov_b64 %0, %9\n\tv_mov_b64 %1, %10\n\tv_mov_b64 %2, %11\n\tv_mov_b64 %3, %12\n\t"
					    "v_mov_b64 %4, %13\n\tv_mov_b64 %5, %14\n\tv_mov_b64 %6, %15\n\tv_mov_b64 %7, %16\n\t"
					    "s_mov_b64 exec, %8"
					    : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3), "+v"(w4), "+v"(w5), "+v"(w6), "+v"(w7), "=&s"(saved)
					    : "s"(b0), "s"(b1), "s"(b2), "s"(b3), "s"(b4), "s"(b5), "s"(b6), "s"(b7), "s"(rowsel)
					    : "scc");
				});
			}
		});
		if constexpr (ZM != 2)
			static_for<NI>([&](auto qc) __attribute__((always_inline)) {  // a sample of these RB rows equals the isovalue: mark the rows
				constexpr int q = decltype(qc)::value;
				const uint64_t zb = (ZM == 0 && ZMIN_REG) ? __ballot(zmin[q] == 0) : zeq[q];
				if (zb) { zacc[q] |= ((1ull << RB) - 1ull) << r; zcacc[q] |= zb; }
				zmin[q] = 1; zeq[q] = 0;
			});
		}
		if (bi != NB - 1) return;
		// ---- the plane is complete ----
		// (the forms over several isovalues sit at their register limit: the lane's number is computed afresh here - fresh_lane)
		const uint32_t lp = NI >= 2 ? fresh_lane() : lane;
		const uint32_t tid = NI >= 2 ? wv * 64u + lp : threadIdx.x;
		const uint32_t par = (p - pl0) & 1u;
		if (grouped) {  // (block-uniform) column 0 of this plane for the wave to the left; the right neighbour's for this wave
			static_for<NI>([&](auto qc) __attribute__((always_inline)) {
				constexpr int q = decltype(qc)::value;
				const uint64_t hb = __ballot(((uint32_t)c64[q][0] & 1u) != 0u);  // (word 0 bit 0 is the segment's first sample in every layout S)
				if (lp == 0) {
					s_mail[par][wv][q][0] = hb;
					s_mail[par][wv][q][1] = (ZM != 2 && (zcacc[q] & 1ull)) ? zacc[q] : 0ull;  // (lane 0 loaded column 0; rows to the batch: a superset is fine)
				}
			});
			// (not __syncthreads(): that also waits for the prefetched batch's loads - only the mailbox's LDS writes must have landed)
			asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
		}
		static_for<NI>([&](auto qc) __attribute__((always_inline)) {
			constexpr int q = decltype(qc)::value;
			const SweepLane &L = a.lane[q];
#pragma unroll
			for (int k = 0; k < 4; k++) { cur[q][k] = c64[q][k]; c64[q][k] = 0; }
			if (from_right) {  // (wave-uniform; the mailbox word is read here, per isovalue: held over the loop it cost the 4-isovalue form registers it does not have)
				const uint64_t nb_bits = s_mail[par][wv + 1u][q][0], nb_zero = ZM != 2 ? s_mail[par][wv + 1u][q][1] : 0ull;
				cur_h[q] = (uint32_t)((nb_bits >> lp) & 1ull);
				const uint64_t zh = nb_zero & (nrows >= 64u ? ~0ull : ((1ull << nrows) - 1ull));
				cur_z[q] = zacc[q] | zh;
				cur_zc[q] = zh ? ~0ull : zcacc[q];
				zacc[q] = zcacc[q] = 0;
			} else {
				const real_t dh = iso[q] - halo;
				cur_h[q] = sign_of(dh);
#ifdef MC33_NAN_SAMPLES
				cur_h[q] ^= (uint32_t)(dh != dh);
#endif
				const uint64_t zh = __ballot(lp < nrows && dh == 0);  // (lanes past the tile never loaded a halo sample)
				cur_z[q] = zacc[q] | zh;
				cur_zc[q] = zh ? ~0ull : zcacc[q];  // (a halo sample: any column)
				zacc[q] = zcacc[q] = 0;
			}
			auto leave_edge = [&](uint32_t which) __attribute__((always_inline)) {  // bit rows of this plane for k_boundary (a plane record like those of slice_bits)
				// (in compact form where it fits.  The tile's first plane of a single-isovalue pass waits in the log; its last plane comes at
				// the tile's end anyway and is stored at once.  As raw records these cost the round-3 float sweep 0.065 of its 0.73 ms - the
				// two 1 KiB stores, not the header: profiles/r03_sweep_parts.txt; the other forms measured: EXPERIMENTS.md)
				uint32_t fmt = PLANE_RAW;
				uint4 *rec = L.edge_bits + ((uint64_t)wtile * 2u + which) * 128u;
				// A plane of the tile that lies wholly on one side of the surface - two thirds of them on a smooth field - leaves no
				// record, only the header with its side (round 4: the records are two thirds of what the single-isovalue sweep writes)
				const uint64_t w_or = cur[q][0] | cur[q][1] | cur[q][2] | cur[q][3], w_and = cur[q][0] & cur[q][1] & cur[q][2] & cur[q][3];
				const bool all0 = __ballot(w_or != 0ull) == 0ull, all1 = __ballot(w_and != ~0ull) == 0ull;
				bool deferred = false;  // (the tile's FIRST plane: its record, when it is small, waits in the log with everything else)
				if (all0 || all1) { fmt = all0 ? PLANE_UNIFORM0 : PLANE_UNIFORM1; deferred = DEFER && which == 0u && !MC33_DEBUG_BITS(a); }
				else if (DEFER && which == 0u && !MC33_DEBUG_BITS(a)) {
					uint32_t desc;
					if (encode_plane<S>(cur[q], desc)) {
						if constexpr (DEFER) s_log[wv].edge[lp] = desc;
						fmt = PLANE_COMPACT; deferred = true;
					} else store_plane_raw<S>(rec, cur[q], lp);
				}
				else fmt = store_plane_record<S>(rec, (uint32_t *)rec, cur[q], lp);
				const uint64_t bh = __ballot(cur_h[q] != 0);
				if (deferred) {
					if constexpr (DEFER) {
						if (lp == 0) {
							uint32_t *e = s_log[wv].edge_hdr;
							e[0] = (uint32_t)bh; e[1] = (uint32_t)(bh >> 32); e[2] = (uint32_t)cur_z[q]; e[3] = (uint32_t)(cur_z[q] >> 32);
							e[4] = (uint32_t)cur_zc[q]; e[5] = (uint32_t)(cur_zc[q] >> 32); e[6] = fmt; e[7] = 0u;
						}
						log_edge = fmt;
					}
				} else
				if (lp == 0 && !(MC33_DEBUG_BITS(a) & 4096u)) {  // (developer builds: 4096 no header)
					L.edge_hdr[((uint64_t)wtile * 2u + which) * 2u] = uint4{(uint32_t)bh, (uint32_t)(bh >> 32), (uint32_t)cur_z[q], (uint32_t)(cur_z[q] >> 32)};
					L.edge_hdr[((uint64_t)wtile * 2u + which) * 2u + 1u] = uint4{(uint32_t)cur_zc[q], (uint32_t)(cur_zc[q] >> 32), fmt, 0u};
				}
			};
			if (MC33_DEBUG_BITS(a) & 2u) {
			} else {
				// (developer builds: 256 no edge records, 1024 / 2048 none for the first / last plane, 512 no cut-cell test)
				if (p == pl0 && pl0 != z_lo && !(MC33_DEBUG_BITS(a) & (256u | 1024u))) leave_edge(0);
				if (p > pl0 && !(MC33_DEBUG_BITS(a) & 512u)) {
					uint64_t act[4], pq[4];
#pragma unroll
					for (int k = 0; k < 4; k++) {
						if constexpr (PREV_LDS) pq[k] = s_prev[q][k][tid]; else pq[k] = prev[q][k];
					}
					uint32_t ph;
					if constexpr (PREV_LDS) ph = s_prevh[q][tid]; else ph = prev_h[q];
					active_cells<S>(pq, cur[q], ph, cur_h[q], valid, rowvalid, act);
					if (__ballot((act[0] | act[1] | act[2] | act[3]) != 0ull) && !(MC33_DEBUG_BITS(a) & 16u)) {  // wave-uniform: hand the slice to k_cells
						uint64_t pz, pzc;
						if constexpr (PREV_LDS) { pz = readlane64(s_prevz[q][0][wv], 0); pzc = readlane64(s_prevz[q][1][wv], 0); }  // (wave-uniform: into SGPRs, not four registers held from an early LDS read to the header's store)
						else { pz = prev_z[q]; pzc = prev_zc[q]; }
						if (DEFER && !MC33_DEBUG_BITS(a)) {  // (developer switches keep the direct stores they were written for)
							const uint64_t slot = slice_slot(p - 1 - P.zs, yt, seg, a.sd), slot_up = slice_slot(p - P.zs, yt, seg, a.sd);
							if (!prev_written[q]) log_plane(slot, pq, lp);
							log_plane(slot_up, cur[q], lp);
							log_header(slot, __ballot(ph != 0), __ballot(cur_h[q] != 0), pz | cur_z[q], pzc | cur_zc[q], act, lp);
						} else
						hand_over_slice<S>(L, slice_slot(p - 1 - P.zs, yt, seg, a.sd), slice_slot(p - P.zs, yt, seg, a.sd), pq, cur[q],
						                   !prev_written[q], true, __ballot(ph != 0), __ballot(cur_h[q] != 0), pz | cur_z[q], pzc | cur_zc[q], act, lp,
						                   MC33_DEBUG_BITS(a), NI >= 2 ? &pend_chunk[q] : nullptr, NI >= 2 ? &pend_sum[q] : nullptr);
						cur_written[q] = true;
					}
				}
				if (p == z_hi && has_above && !(MC33_DEBUG_BITS(a) & (256u | 2048u))) leave_edge(1);
			}
#pragma unroll
			for (int k = 0; k < 4; k++) {
				if constexpr (PREV_LDS) s_prev[q][k][tid] = cur[q][k]; else prev[q][k] = cur[q][k];
			}
			if constexpr (PREV_LDS) s_prevh[q][tid] = cur_h[q]; else prev_h[q] = cur_h[q];
			if constexpr (PREV_LDS) { s_prevz[q][0][wv] = cur_z[q]; s_prevz[q][1][wv] = cur_zc[q]; } else { prev_z[q] = cur_z[q]; prev_zc[q] = cur_zc[q]; }
			prev_written[q] = cur_written[q];
			cur_written[q] = false;
			// (one isovalue's plane work at a time: interleaved by the scheduler, the four of them need more registers than 3 waves per SIMD leave)
			if constexpr (NI >= 2) __builtin_amdgcn_sched_barrier(0);
		});
	};

	raw_t dA[16], dB[16];
	real_t hA = 0, hB = 0;
	if constexpr (BS) {
		// ---- the block stream: a batch is one LIVE block (g, k) of the plane - the sample rows 16 g .. 16 g + 15 of quarter k, 16 loads - and
		// a dead block costs no instruction.  Two cursors walk (plane, live block) through the functions of mc33_sweep_blocks.h: the
		// one that issues, a batch ahead of the one that processes; each keeps the blocks of its plane it has not taken yet (rem_i, rem_p)
		// and the word of the plane behind, asked for a plane ahead.  There is no count of batches: the loop ends when the processing
		// cursor has completed plane z_hi.  A plane's bit rows and halo samples START as what its dead blocks are worth (plane_start)
		// and the batches overwrite the rows of the live ones; a plane is completed when the processing cursor leaves it - at once
		// after its last batch, and one after the other the planes in which this wave has no batch at all, so that every wave of a
		// grouped block reaches every plane's mailbox barrier exactly once.
		// Rows and lanes: the per-quarter form, whose batches were 4 rows, wrote the rows below 4 NB and left the lanes above them
		// zero; so does this one (lane_in, rows_in), and the records it leaves are the same bytes.
		// Registers (gfx950 code of k_sweep_live_blocks<0>): 115 VGPRs, no scratch, 4 waves per SIMD; 50 SGPRs parked in VGPR lanes where
		// the per-quarter form had 43 - each cursor now carries its plane, the blocks left of it and two words through the loop.
		const uint32_t nrg = (NB + 3u) >> 2;      // row groups that hold a row of the tile
		const bool own_halo = !from_right;
		const uint32_t lg = lane >> 4;            // the row group of the sample row this lane holds
		const bool lane_in = lane < NB * 4u;
		const uint64_t rows_in = NB >= 16u ? ~0ull : (1ull << (4u * NB)) - 1ull;
		const uint32_t xl = xbase + lane, so_last = (nrows - 1u) * rowbytes;
		uint64_t bwi = block_word(pl0), bwi_n = block_word(pl0 + 1u), bwp = bwi, bwp_n = bwi_n;
		uint32_t ip = pl0, pp = pl0;
		uint32_t rem_i = sweep_live_mask(bwi, nrg, own_halo), rem_p = rem_i;
		// the next live block at or after the issuing cursor, through the planes that have none; past the last one (`false`) the
		// 16 loads go through a descriptor of zero bytes - no memory access - and are never looked at.  Always 16 loads, and the halo
		// column of the row group as the 17th with the batch of quarter 3 (sweep_live_mask sees to it that this batch exists wherever
		// the halo block is live) under the lane condition of the other forms: see `issue`.
		auto issue_next = [&](raw_t (&d)[16], real_t &hv) __attribute__((always_inline)) -> bool {
			while (rem_i == 0u && ip < z_hi) {
				++ip; bwi = bwi_n; bwi_n = block_word(ip + 1u);
				rem_i = sweep_live_mask(bwi, nrg, own_halo);
			}
			const bool there = rem_i != 0u;
			const uint32_t j = there ? sweep_next_block(rem_i, 0u) : 0u;
			rem_i &= rem_i - 1u;
			const uint32_t g = j >> 2, k = j & 3u;
			const sample_t *base = a.G.p + (uint64_t)(ip - a.G.z0) * a.G.slice + (uint64_t)y0 * a.G.pitch;
			const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, there ? tile_bytes : 0u, 0x00020000);
			const uint32_t vo = min(xl + 64u * k, P.nx) * (uint32_t)sizeof(sample_t);
			uint32_t so = 16u * g * rowbytes;  // (16 g < nrows: the row group holds a row of the tile)
#pragma unroll
			for (int rr = 0; rr < 16; rr++) {
				d[rr] = MC33_LOAD(rs, vo, so);
				so = min(so + rowbytes, so_last);  // (a row past the tile is the tile's last row)
			}
			const bool wanted = (lg == g) & lane_in & (k == 3u) & own_halo & there & !(MC33_DEBUG_BITS(a) & 64u) & (sweep_halo_code(bwi, g) == 0u);
			if (wanted) hv = MC33_LOAD(rs, xh, 0u);
			return there;
		};
		auto plane_start = [&]() __attribute__((always_inline)) {
#pragma unroll
			for (int k = 0; k < 4; k++) c64[0][k] = lane_in ? sweep_const_word(bwp, lg, (uint32_t)k) : 0ull;
			halo = lane_in ? __uint_as_float(sweep_const_halo_bits(bwp, lg)) : 0.0f;
		};
		// the batch in dd, when there is one (`have`: only the very first call can come without), is the next block of the processing
		// cursor; then every plane that has no block left is completed.  true: plane z_hi is complete, the tile is done.
		auto process_next = [&](const raw_t (&dd)[16], const real_t &hv, bool have) __attribute__((always_inline)) -> bool {
			if (have) {
				const uint32_t j = sweep_next_block(rem_p, 0u);
				rem_p &= rem_p - 1u;
				const uint32_t g = j >> 2, k = j & 3u;
				uint64_t row = 0;  // lane 16 g + rr: the bit row of sample row rr of the block
#pragma unroll
				for (int rr = 0; rr < 16; rr++) {
					const real_t d = iso[0] - dd[rr];                     // MC:1852-1855
					uint64_t bb = __ballot(sign_of(d) != 0);              // MC:1856-1859 (sign bit)
#ifdef MC33_NAN_SAMPLES
					bb ^= __ballot(d != d);
#endif
					zmin[0] = real_min(zmin[0], real_abs(d));
					// (one lane of EXEC, one 64-bit move from the SGPR pair: see `process`)
					const uint32_t rowsel = (uint32_t)__builtin_amdgcn_readfirstlane((int)(16u * g + (uint32_t)rr));
					uint64_t saved;
					asm volatile(
					    "s_mov_b64 %1, exec\n\t"
					    "s_lshl_b64 exec, 1, %3\n\t"
					    "v_mov_b64 %0, %2\n\t"
					    "s_mov_b64 exec, %1"
					    : "+v"(row), "=&s"(saved)
					    : "s"(bb), "s"(rowsel)
					    : "scc");
				}
				const bool mine = (lg == g) & lane_in;
#pragma unroll
				for (int kk = 0; kk < 4; kk++) c64[0][kk] = (mine & (k == (uint32_t)kk)) ? row : c64[0][kk];
				if (k == 3u && sweep_halo_code(bwp, g) == 0u) halo = mine ? hv : halo;  // (wave-uniform; a wave that takes its halo bits from the mailbox never looks at `halo`)
				// a sample of the block equals the isovalue: its 16 rows are marked (a superset - k_cells lets the cell's own samples decide)
				const uint64_t zb = __ballot(zmin[0] == 0);
				if (zb) { zacc[0] |= (0xFFFFull << (16u * g)) & rows_in; zcacc[0] |= zb; }
				zmin[0] = 1;
			}
			while (rem_p == 0u) {
				process(dd, hv, pp, NB - 1u);  // (the completion of plane pp: its bit rows, halo samples and marks are handed on)
				if (pp == z_hi) {
					// (the batch prefetched past the end is waited for HERE: left in flight, the way out met the loop's back edge with loads
					// pending on registers the plane's rows had moved into, and the compiler's wait for them - vmcnt(0), read in the gfx950
					// code - stood in the block both paths share: every second batch waited for the one just issued)
					__builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
					return true;
				}
				++pp; bwp = bwp_n; bwp_n = block_word(pp + 1u);
				rem_p = sweep_live_mask(bwp, nrg, own_halo);
				plane_start();
			}
			return false;
		};
		if (!dead_me) {  // (a wave without a tile - the last quad of a list, never in a grouped block - has no plane to complete)
			plane_start();
			bool have = rem_p != 0u;
#ifdef MC33_DEV  // MC33_HIP_DEBUG 16384: the loads alone - every batch waited for and dropped, no classification at all
			if (MC33_DEBUG_BITS(a) & 16384u) {
				auto drop = [&](const raw_t (&dd)[16], const real_t &hv) __attribute__((always_inline)) {
#pragma unroll
					for (int k = 0; k < 16; k++) asm volatile("" ::"v"(dd[k]));
					asm volatile("" ::"v"(hv));
				};
				bool more = issue_next(dA, hA);
				while (more) {
					more = issue_next(dB, hB);
					drop(dA, hA);
					if (!more) break;
					more = issue_next(dA, hA);
					drop(dB, hB);
				}
				return;
			}
#endif
			if (have) issue_next(dA, hA);
			for (;;) {
				issue_next(dB, hB);
				if (process_next(dA, hA, have)) break;
				issue_next(dA, hA);
				if (process_next(dB, hB, true)) break;
				have = true;
			}
		}
	} else {
	uint32_t ip = pl0, ib = 0, pp = pl0, pb = 0;  // (plane, batch) of the next issue / of the next process
	// past the end of the tile the prefetch simply re-reads the last batch (it is never processed)
#define MC33_ADV(p_, b_) do { if (++(b_) == NB) { (b_) = 0; ++(p_); } } while (0)
#define MC33_ADV_ISSUE() do { if (ip != z_hi || ib + 1 != NB) MC33_ADV(ip, ib); } while (0)
	// (Tried in round 3: the loads that refill a buffer issued as soon as its rows are bit rows, BEFORE the work on a complete
	// plane, so that two batches stay in flight during that work and a hand-over's stores are younger than the refill.  The
	// refill's registers are then live across the plane's work: 92 -> 134 VGPRs for one isovalue per pass = 3 waves per SIMD
	// instead of 4, float 1024^3 0.73 -> 0.82 ms; held to 128 (36 bytes of scratch) 0.73 - 0.75 -> 0.74 - 0.75, ushort
	// 1.66 -> 1.72 ms.  No gain.  What the plane's work costs the stream is its stores, wherever they are issued:
	// profiles/r03_sweep_parts.txt.)
	issue(dA, hA, ip, ib); MC33_ADV_ISSUE();
#ifdef MC33_DEV  // MC33_HIP_DEBUG 16384: the loads alone - every batch waited for and dropped, no classification at all
	if (MC33_DEBUG_BITS(a) & 16384u) {
		auto drop = [&](const raw_t (&dd)[16], const real_t &hv) __attribute__((always_inline)) {
#pragma unroll
			for (int k = 0; k < 16; k++) asm volatile("" ::"v"(dd[k]));
			asm volatile("" ::"v"(hv));
		};
		for (uint32_t t = 0; t < T; t += 2) {
			issue(dB, hB, ip, ib); MC33_ADV_ISSUE();
			drop(dA, hA);
			issue(dA, hA, ip, ib); MC33_ADV_ISSUE();
			drop(dB, hB);
		}
		return;
	}
#endif
	for (uint32_t t = 0; t < T; t += 2) {
		issue(dB, hB, ip, ib); MC33_ADV_ISSUE();
		process(dA, hA, pp, pb); MC33_ADV(pp, pb);
		issue(dA, hA, ip, ib); MC33_ADV_ISSUE();
		if (t + 1 < T) { process(dB, hB, pp, pb); MC33_ADV(pp, pb); }
	}
	}
	log_flush();  // (DEFER: everything the tile hands on, behind its last load)
	if constexpr (NI >= 2) {
#pragma unroll
		for (int q = 0; q < NI; q++)
			if (pend_sum[q] && lane == 0) atomicAdd(a.lane[q].slot_part + pend_chunk[q], pend_sum[q]);
	}
	if (a.trace && lane == 0) {
		unsigned long long *tr = a.trace + 4ull * (blockIdx.x * 4u + wv);  // (by launched wave: block index mod 8 is the XCD; the tile is that of the block's entry in the packed list)
		tr[0] = t_start; tr[1] = __builtin_amdgcn_s_memrealtime(); tr[2] = c_start; tr[3] = __builtin_amdgcn_s_memtime();
	}
#undef MC33_ADV_ISSUE
#undef MC33_ADV
#undef MC33_LOAD
}
template <int S, int NI, int ZM = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_sweep(const SweepArgs a) {  // (3 waves per SIMD: at most 168 VGPRs - the 4-lane form sits right at that edge)
	sweep_tile<S, NI, ZM, 1>(a);
}
template <int S, int NI, int ZM = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_sweep_live(const SweepArgs a) {
	sweep_tile<S, NI, ZM, 2>(a);
}
// ... and leaves the dead blocks of its live tiles out (SweepArgs::blockw; sweep_tile: BS)
template <int ZM = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_sweep_live_blocks(const SweepArgs a) {
	if constexpr (MC33_BLOCK_SKIP) sweep_tile<1, 1, ZM, 2, true>(a);
}
template <int S, int NI, int ZM = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void k_sweep_all(const SweepArgs a) {
	sweep_tile<S, NI, ZM, 0>(a);
}

// ---------------------------------------------------------------------------------------------------
// k_boundary: the slice between the last plane of a tile and the first plane of the tile above it, from the bit
// rows the two left behind.  One wave per pair of tiles.
// ---------------------------------------------------------------------------------------------------
// (TileBoundary - tile (wave) indices of k_sweep, slice z: mc33_sweep_plan.h)
__global__ __launch_bounds__(256) void k_boundary(const SweepArgs a, const TileBoundary *bounds, uint32_t nbounds) {
	const SweepLane &L = a.lane[blockIdx.y];  // (the isovalue lanes of the sweep that left the edge records)
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t bi = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	if (bi >= nbounds) return;
	const TileBoundary b = bounds[bi];
	const Params &P = a.P;
	const uint32_t seg = b.seg;
	const uint64_t rp = (uint64_t)b.below * 2u + 1u, rc = (uint64_t)b.above * 2u;  // top of below, bottom of above
	const uint4 hp = L.edge_hdr[rp * 2u], hc = L.edge_hdr[rc * 2u], zp = L.edge_hdr[rp * 2u + 1u], zc = L.edge_hdr[rc * 2u + 1u];
	// Both planes wholly on the same side, halo columns included - every pair of dead tiles (k_tile_verdicts), and most pairs of a
	// smooth field under a plan with a table, which has three times the pairs: no cell between them is cut, whatever equals the
	// isovalue (such a sample has bit 0), and the wave ends on the four header words without asking for a record.
	if (zp.z >= PLANE_UNIFORM0 && zp.z == zc.z) {  // (wave-uniform)
		const uint32_t side = zp.z == PLANE_UNIFORM1 ? 0xFFFFFFFFu : 0u;
		if (hp.x == side && hp.y == side && hc.x == side && hc.y == side) return;
	}
	const uint4 p0 = L.edge_bits[rp * 128u + lane], p1 = L.edge_bits[rp * 128u + 64u + lane];
	const uint4 c0 = L.edge_bits[rc * 128u + lane], c1 = L.edge_bits[rc * 128u + 64u + lane];
	// (both forms of both records are asked for at once - which one a plane has stands in its header, zp.z / zc.z)
	const uint32_t dp = ((const uint32_t *)(L.edge_bits + rp * 128u))[lane], dc = ((const uint32_t *)(L.edge_bits + rc * 128u))[lane];
	uint64_t prev[4] = {u64(p0.x, p0.y), u64(p0.z, p0.w), u64(p1.x, p1.y), u64(p1.z, p1.w)};
	uint64_t cur[4] = {u64(c0.x, c0.y), u64(c0.z, c0.w), u64(c1.x, c1.y), u64(c1.z, c1.w)};
	if (zp.z == PLANE_COMPACT) decode_row(dp, prev);
	if (zc.z == PLANE_COMPACT) decode_row(dc, cur);
	if (zp.z >= PLANE_UNIFORM0) { prev[0] = prev[1] = prev[2] = prev[3] = zp.z == PLANE_UNIFORM1 ? ~0ull : 0ull; }  // (no record was written: what was loaded is an older extraction's)
	if (zc.z >= PLANE_UNIFORM0) { cur[0] = cur[1] = cur[2] = cur[3] = zc.z == PLANE_UNIFORM1 ? ~0ull : 0ull; }
	const uint64_t bp = u64(hp.x, hp.y), bc = u64(hc.x, hc.y);
	uint64_t valid[4], act[4];
	valid_masks(seg * SEG_CELLS, P.nx, valid);
	const bool rowvalid = lane < 63u && b.yt * 63u + lane < P.ny;
	active_cells(prev, cur, (uint32_t)((bp >> lane) & 1ull), (uint32_t)((bc >> lane) & 1ull), valid, rowvalid, act);
	if (__ballot((act[0] | act[1] | act[2] | act[3]) != 0ull))
		// (the two tiles may have written these planes for slices of their own: same bytes again)
		hand_over_slice<1>(L, slice_slot(b.z - P.zs, b.yt, seg, a.sd), slice_slot(b.z + 1u - P.zs, b.yt, seg, a.sd), prev, cur,
		                true, true, bp, bc, u64(hp.z, hp.w) | u64(hc.z, hc.w), u64(zp.x, zp.y) | u64(zc.x, zc.y), act, lane);
}
