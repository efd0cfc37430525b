// mc33_kernels.hip -- HIP kernels (gfx950 / CDNA4, wave64) and the device-level C ABI (include/mc33_hip.h)
// of the MI355X Marching Cubes 33 extractor.  One shared object per grid sample type, like the
// reference's one-type-per-compile model (reference include/marching_cubes_33.h:57-88):
//     default            -> float samples           (libMC33_f32.so)
//     -DMC33_GRD_F64     -> double samples AND double arithmetic / vertices (libMC33_f64.so)
//     -DMC33_GRD_U8 / _U16 / _U32 -> unsigned char / short / int samples (libMC33_u8 / _u16 / _u32.so)
//
// Passes of one extraction, in launch order ("MC:" = reference source/marching_cubes_33.c):
//   k_sweep<S,NI,ZM> - streams the volume once (MC:1832-1868) and does nothing else that costs bandwidth: sign bit per
//                   sample by wave ballot, the bit rows of a 64-row x 256-sample tile slice parked one row per LANE, so
//                   that "is any cell of this slice cut" is a handful of 64-bit logic ops.  For each slice that is cut it
//                   leaves the bit planes (each plane once; 256 bytes in compact form), a header (cut cells, halo bits)
//                   and a partial sum for k_slots.  The halo column comes from the neighbouring wave through an LDS
//                   mailbox.  S: narrow samples are loaded S to a dword; NI: isovalues classified per pass
//                   (mc33hip_sweep_many), each with its own "lane" of output buffers; ZM: how a sample is classified.
//   k_boundary    - the slice between two z-tiles of k_sweep, from the edge planes both left behind.
//   k_slots       - exclusive sums of (cut cells, batches of 64 of them) over the slice slots in storage order.
//   k_cells       - the waves take cut slices off a list k_slots made, 64 cut cells per step: sign index from the bit planes; fast cells (interior,
//                   no test needed, no sample == iso) finished from a 256-entry table, cells whose sign index needs the
//                   face / interior tests tested here (TESTED records), the rest queued for k_slow_plan; one 8-byte work
//                   record per cut cell, contiguous in the reference's visiting order, (#new vertices, #triangles) per
//                   row segment, and one descriptor per batch of 64 records for the vertex pass.
//   k_slow_plan   - the generic plan (MC:683-779, 788-1224: cells on the grid's 0-faces, corners equal to the isovalue).
//   k_slow_count  - triangles of cells with a corner equal to the isovalue, by vertex identity (MC:1235); enqueued when the
//                   context's last extraction had such cells.
//   k_seg_fix     - offsets of the row segments a slow cell changed (and the identity counts k_slow_count was not enqueued for).
//   k_scan_*      - exclusive prefix sums over the row segments in the reference's sweep order: this IS the
//                   reference's vertex / triangle numbering.
//   k_emit_vertices<MODE> - one WAVE per batch of 64 records of one slice slot: the sample rows the batch needs staged in
//                   LDS by cooperative 16-byte loads, one lane per vertex (MC:810-1230, 485-585).
//   k_emit_fast_triangles - one thread per record: vertex ids of the nine shared edges through the owners' records,
//                   triangles (MC:1235-1250); leaves the counters of the extraction in the host's pinned copy.  First of the
//                   emit passes while the record set fits the last-level cache, behind the vertex pass otherwise.
//   k_emit_slow_slots / k_emit_slow - the generic emit of the slow records: 16 lanes per record (a lane per pattern slot) in
//                   sequence behind the fast passes when they are few; a thread per record, on large grids on a second
//                   stream beside the fast passes, when they are many.
// Not part of an extraction: k_property<R,COLOR> - a property grid sampled at the vertices of a finished V array, one lane per
//                   vertex; float values or palette colours (mc33_property.hip.h).
//                   k_mesh_* - what the passes over a finished mesh share: the tile scan (sums per tile, one block over them, a
//                   placing pass), the table of 64-bit keys claimed by compare-and-swap, referenced flags; the registration of
//                   the parts' states and their shared scratch (mc33_mesh.hip.h).
//                   k_measure_* / k_cc_* - area, volume, moments, bounding box and connected components of a finished V, T pair;
//                   a few doubles come back instead of the mesh (mc33_measure.hip.h).
//                   k_topo_* - an edge table of a finished T in device memory: boundary, non-manifold and misoriented edges,
//                   boundary loops, Euler number and genus, for the surface and per component (mc33_topology.hip.h).
//                   k_filt_* - keep or drop whole components of a finished V, N, T: flags, two tile scans, two copying passes;
//                   the rows keep their order (mc33_filter.hip.h).
//                   k_sm_* - Taubin smoothing of a finished V over the adjacency of T, a CSR list made on the device, and vertex
//                   normals recomputed from the triangles; k_sm_pass is its hot path (mc33_smooth.hip.h).
//                   k_curvature<R> - mean, Gaussian and principal curvatures of the level set at the vertices of a finished V, from
//                   the gradient and Hessian of the resident grid: one lane per vertex walks the nodes its vertex has, 19 samples
//                   each; k_curv_init clears its summary; k_color_values - a palette over any float array (mc33_curvature.hip.h,
//                   DESIGN.md 22).
//                   k_simp_* - vertex clustering of a finished V, T on a lattice: a table of clusters filled by 64-bit compare-and-swap,
//                   duplicate triangles through a table of triangle indices, two exclusive scans, two writing passes;
//                   k_simp_cluster is its hot path (mc33_simplify.hip.h).
//                   k_clip_* - a finished V, N, T cut by a plane: classes, a table of cut edges filled by 64-bit compare-and-swap and
//                   atomicMin of the owner, three exclusive scans, three writing passes; k_clip_tri is its hot path
//                   (mc33_clip.hip.h).
//                   k_section_* - a finished V, T met by a plane: clip's classes, table and owners as they stand, then the contour
//                   as points and directed segments, a union-find over the points, length and enclosed area in the fixed order of
//                   the measures; k_section_ladder - many parallel planes in one pass over T (mc33_section.hip.h).
//                   k_cap_* - a finished V, N, T closed at the faces of a box of grid points: face bits of the vertices, the table of
//                   sides for the ones used once, a minimum, a maximum and a count of rim segments per face cell, marching squares
//                   over the resident samples of the faces, two exclusive scans, two writing passes; k_cap_sides is its hot path
//                   (mc33_cap.hip.h).
//                   k_render_* - a finished V, N, T and a colour word per vertex drawn into an image, a depth buffer and an id buffer: a
//                   screen record per vertex, a lane per triangle lowering 64-bit depth | id keys with atomicMin, a wave per screen tile
//                   of the triangles too large for a lane, a lane per pixel to shade; k_render_triangles is its hot path
//                   (mc33_render.hip.h).
//                   k_dist_* - the nearest triangle of a finished V, T for each of many points: the box of the usable triangles, a
//                   uniform lattice over it, a count, an exclusive scan and a fill of the cell lists, a lane per point visiting shells
//                   of cells until a lower bound on the rest exceeds its best; k_dist_query is its hot path (mc33_distance.hip.h,
//                   DESIGN.md 25).
// Before an extraction: k_rs_resample - the resident grid into a second device grid, a separable correlation of up to 17 taps per axis
//                   with an integer stride, one pass over the source: a block stages the rows its tile of outputs needs in LDS,
//                   sums along x and y into a ring of planes and along z out of it (mc33_resample.hip.h).
//                   k_rk_minmax, k_rk_median - the resident grid into a second device grid through a box window's minimum, maximum
//                   or median, one pass over the source: sample keys staged in LDS with the next plane's loads in flight, the
//                   maximum axis by axis through a ring of planes, the median by a selection network in registers
//                   (mc33_rank.hip.h).
//                   k_sp_spectrum - the contour spectrum of the resident grid for up to 255 isovalues in one pass: every sample
//                   ranked among the isovalues in LDS, cells cut and samples counted per rank in the block's LDS counters, 64-bit
//                   device counters once per block; k_sp_init clears those (mc33_spectrum.hip.h).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <algorithm>
#include <cmath>
#include <limits>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mc33_hip.h"
#ifdef MC33_GRD_F64
#define MC33_REAL_DOUBLE  // MC33_real is double in the double build (reference marching_cubes_33.h:80-82)
#endif
#if !defined(MC33_GRD_U8) && !defined(MC33_GRD_U16) && !defined(MC33_GRD_U32)
#define MC33_NAN_SAMPLES 1  // float / double grids may hold NaN samples
#else
#define MC33_INT_SAMPLES 1  // unsigned integer samples: no NaN, no signed zero (k_sweep's ZM)
#endif
#include "mc33_cell.h"
#include "mc33_lut_data.h"
#include "mc33_rules_data.h"

using namespace mc33;

#if defined(MC33_GRD_U16)
typedef uint16_t sample_t;
#define MC33_SAMPLE_BYTES 2
#elif defined(MC33_GRD_U8)
typedef uint8_t sample_t;
#define MC33_SAMPLE_BYTES 1
#elif defined(MC33_GRD_U32)
typedef uint32_t sample_t;
#define MC33_SAMPLE_BYTES 4
#elif defined(MC33_GRD_F64)
typedef double sample_t;
#define MC33_SAMPLE_BYTES 8
#else
typedef float sample_t;
#define MC33_SAMPLE_BYTES 4
#endif

// The translation unit in parts (round 5: it had grown to 4 500 lines), included in this order:
// (mc33_resample.hip.h ends with #include "mc33_rank.hip.h": the rank filter of the grid follows its resampling)
#include "mc33_sweep_plan.h"
#include "mc33_sweep_blocks.h"
#include "mc33_records.hip.h"
#include "mc33_sweep_pack.h"
#include "mc33_sweep.hip.h"
#include "mc33_tail.hip.h"
#include "mc33_emit.hip.h"
#include "mc33_context.hip.h"
#include "mc33_extract.hip.h"
#include "mc33_property.hip.h"
#include "mc33_mesh.hip.h"
#include "mc33_measure.hip.h"
#include "mc33_topology.hip.h"
#include "mc33_filter.hip.h"
#include "mc33_smooth.hip.h"
#include "mc33_cap.hip.h"
#include "mc33_render.hip.h"
#include "mc33_distance.hip.h"
#include "mc33_simplify.hip.h"
#include "mc33_clip.hip.h"
#include "mc33_section.hip.h"
#include "mc33_resample.hip.h"
#include "mc33_curvature.hip.h"
#include "mc33_spectrum.hip.h"
