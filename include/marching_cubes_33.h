/* marching_cubes_33.h -- public C API of the MI355X-native MC33 library (libMC33_{f32,f64,u8,u16,u32}.so).
 *
 * Binary- and source-compatible with the header of dvega68/MC33_c_library (reference
 * include/marching_cubes_33.h): same type names, same struct layouts (checked by static asserts in
 * mc33_capi.c against the offsets recorded in SURVEY.md 8(a)-11), same function names and argument
 * meaning.  A program written against the reference header links against this library unchanged;
 * calculate_isosurface runs on the GPU (see include/mc33_hip.h for the device-level entry points).
 *
 * Compile-time variants, as in the reference (reference header :57-88):
 *   default                         GRD_data_type = float,          MC33_real = float
 *   -DINTEGER_GRD -DGRD_TYPE_SIZE=1 GRD_data_type = unsigned char,  MC33_real = float
 *   -DINTEGER_GRD -DGRD_TYPE_SIZE=2 GRD_data_type = unsigned short, MC33_real = float
 *   -DINTEGER_GRD -DGRD_TYPE_SIZE=4 GRD_data_type = unsigned int,   MC33_real = float
 *   -DGRD_TYPE_SIZE=8               GRD_data_type = double,         MC33_real = double (vertices, isovalue)
 *   -DGRD_ORTHOGONAL (with any of the above): _GRD and MC33 without the inclined-grid members (reference
 *   header :116-120, :173-175); link the libMC33_<type>_ortho.so flavour.
 * One library per variant, like the reference's one-type-per-compile model.
 */
#ifndef marching_cubes_33_h
#define marching_cubes_33_h

#define MC33C_VERSION_MAJOR 5
#define MC33C_VERSION_MINOR 5

/* ---- sample type (GRD_data_type) and arithmetic / vertex type (MC33_real) of this build ------------------- */
#ifdef INTEGER_GRD
#  if !defined(GRD_TYPE_SIZE) || (GRD_TYPE_SIZE != 1 && GRD_TYPE_SIZE != 2 && GRD_TYPE_SIZE != 4)
#    error "INTEGER_GRD needs GRD_TYPE_SIZE 1, 2 or 4"
#  endif
#  if GRD_TYPE_SIZE == 1
#    define MC33_SAMPLE_C_TYPE unsigned char
#  elif GRD_TYPE_SIZE == 2
#    define MC33_SAMPLE_C_TYPE unsigned short
#  else
#    define MC33_SAMPLE_C_TYPE unsigned
#  endif
#  define MC33_REAL_C_TYPE float
#elif defined(GRD_TYPE_SIZE) && GRD_TYPE_SIZE == 8
#  define MC33_SAMPLE_C_TYPE double
#  define MC33_REAL_C_TYPE double
#else
#  undef GRD_TYPE_SIZE
#  define GRD_TYPE_SIZE 4
#  define MC33_SAMPLE_C_TYPE float
#  define MC33_REAL_C_TYPE float
#endif
typedef MC33_SAMPLE_C_TYPE GRD_data_type;
typedef MC33_REAL_C_TYPE MC33_real;

#ifdef __cplusplus
extern "C" {
#endif

/* ---- _GRD: regular grid of samples F[k][j][i] (k: z, j: y, i: x); N[] intervals per axis, N[]+1 points -----
 * Byte layout of the reference's _GRD (reference header :111-124): 416 bytes, 256 with GRD_ORTHOGONAL. */
typedef struct mc33_grid {
	GRD_data_type ***F;        /* plane -> row -> samples; rows may be separate allocations              */
	unsigned N[3];             /* intervals in x, y, z                                                  */
	double r0[3];              /* origin                                                                */
	double d[3];               /* spacing                                                               */
	float L[3];                /* extent (unused by the isosurface path)                                */
#ifndef GRD_ORTHOGONAL
	float Ang[3];              /* cell angles in degrees                                                */
	int nonortho;              /* inclined grid: positions / normals go through _A / A_ (MC33_spnC)     */
	double _A[3][3];           /* fractional -> cartesian cell matrix (unit edges) ...                  */
	double A_[3][3];           /* ... and the matrix applied (transposed) to the gradients              */
#endif
	int periodic;
	int internal_data;         /* 1: rows were allocated by alloc_F and are freed by free_memory_grd    */
	char title[160];
} _GRD;

/* ---- surface: result of calculate_isosurface (reference header :133-152), 64 bytes ------------------------
 * T, V, N, color and the struct itself are five separate malloc blocks owned by the caller
 * (free_surface_memory).  MC33 starts with the same members. */
typedef unsigned mc33_triangle[3];
typedef MC33_real mc33_position[3];
typedef float mc33_normal[3];
#define MC33_SURFACE_MEMBERS                                                                     \
	mc33_triangle *T;  /* triangles: three vertex indices each                                */ \
	mc33_position *V;  /* vertex positions                                                    */ \
	mc33_normal *N;    /* unit normals                                                        */ \
	int *color;        /* one 0xAABBGGRR colour per vertex                                    */ \
	unsigned nV;                                                                                 \
	unsigned nT;                                                                                 \
	unsigned capt;     /* allocated triangles                                                 */ \
	unsigned capv;     /* allocated vertices                                                  */ \
	MC33_real iso;

typedef union mc33_user_data { /* 8 bytes free for the caller */
	void *p;
	long long ul;
	int i[2];
	short si[4];
	char c[8];
	float f[2];
	double df;
} mc33_user_data;

typedef struct mc33_surface {
	MC33_SURFACE_MEMBERS
	mc33_user_data user;
} surface;

/* ---- MC33: extraction object (reference header :154-179); 304-byte public part (344 double build; 144 less
 * with GRD_ORTHOGONAL).  This library allocates a larger private object whose first member is this struct;
 * the five id caches of the reference's sweep are unused (NULL), the GPU context hangs behind the public part. */
typedef struct mc33_extractor {
	MC33_SURFACE_MEMBERS
	int memoryfault;           /* non-zero after a failed calculate_isosurface (out of memory, GPU error) */
	const GRD_data_type ***F;
	MC33_real O[3];            /* origin, spacing as MC33_real                                           */
	MC33_real D[3];
	MC33_real ca;              /* d[2]/d[0], d[2]/d[1] (anisotropic spacing)                             */
	MC33_real cb;
	unsigned nx;
	unsigned ny;
	unsigned nz;
	unsigned (*store)(void *, MC33_real *);
#ifndef GRD_ORTHOGONAL
	double _A[3][3];           /* cell matrices scaled by the spacing (inclined grids)                   */
	double A_[3][3];
#endif
	unsigned **Dx;
	unsigned **Dy;
	unsigned **Ux;
	unsigned **Uy;
	unsigned **Lz;
} MC33;

/* colour given to every vertex, 0xAABBGGRR (reference header :181) */
extern int DefaultColorMC;

/* ---- isosurface path (reference header :228-258) --------------------------------------------------------- */
MC33 *create_MC33(_GRD *grid);                                   /* uploads the grid to HBM once          */
surface *calculate_isosurface(MC33 *extractor, MC33_real isovalue); /* GPU extraction; NULL on failure      */
unsigned long long size_of_isosurface(MC33 *extractor, MC33_real isovalue,
                                      unsigned *vertices, unsigned *triangles);
void free_MC33(MC33 *extractor);
void free_surface_memory(surface *s);
void adjustvectorlenght_s(surface *s);                           /* shrink the arrays to nV / nT          */

/* extension (not in the reference): several isovalues of the grid that is resident in HBM.
 * out[k] = what calculate_isosurface(M, iso[k]) would return (NULL where it failed; the caller frees each with
 * free_surface_memory).  The device-to-host copy of surface k runs beside the extraction of surface k+1.
 * Returns the number of surfaces produced. */
unsigned calculate_isosurfaces(MC33 *extractor, const MC33_real *isovalues, unsigned count, surface **out);

/* extension (not in the reference): the caller has rewritten samples of the grid `extractor` was created from.  The
 * reference reads G->F anew on every call (source/marching_cubes_33.c:1792, 1832-1868); this library keeps a copy in
 * HBM, and uploads G->F again before the next extraction after this call.  (MC33_HIP_REUPLOAD=1 in the environment does
 * that before EVERY extraction, for callers that cannot be changed.) */
void MC33_grid_changed(MC33 *extractor);

/* extension (not in the reference, which gives every vertex DefaultColorMC, source/marching_cubes_33.c:1875-1877): colours from
 * a second grid - a density to cut the surface from, a potential to paint on it.
 * MC33_set_property_grid uploads `property` (same N as the extractor's grid, same GRD_data_type; orthogonal grids only) beside
 * the grid in HBM; NULL detaches it; calling it again uploads again (that is also how a caller says "I rewrote the samples").
 * MC33_set_color_map keeps a copy of `count` palette words (0xAABBGGRR, 2 <= count <= 256) and the value range lo < hi they
 * span; NULL removes it.  Both return 0, or -1 when refused (nothing changes then).
 * While both are set, calculate_isosurface(s) samples the property grid at every vertex on the GPU - trilinear, in double, at
 * (v - r0) / d - and writes palette[round((p - lo) / (hi - lo) * (count - 1))] into surface.color, the ends of the palette
 * beyond the range, DefaultColorMC where the value is NaN.  With either missing the colours are DefaultColorMC as before. */
int MC33_set_property_grid(MC33 *extractor, _GRD *property);
int MC33_set_color_map(MC33 *extractor, const int *palette, unsigned count, double lo, double hi);

/* extension (not in the reference): questions about an isosurface answered on the GPU - the surface is extracted into device
 * memory and measured there; no `surface` is allocated and nothing but these structs comes back.
 * For triangle i with vertices q0, q1, q2 (T's order), in double, about origin[a] = r0[a] + 0.5 * (N[a] * d[a]): p_k = q_k - origin,
 *   area     = sum 0.5 * |(p1 - p0) x (p2 - p0)|
 *   volume   = sum p0 . (p1 x p2) / 6      SIGNED, with the winding as T stores it: the reference's winding gives a sphere whose
 *              samples grow outwards (the README example) a NEGATIVE volume, the _nneg flavours of the library the opposite
 *              sign.  It is the enclosed volume only for a surface that does not reach the grid's faces.
 *   moment   = sum area_i * (p0 + p1 + p2) / 3      (the area centroid is origin + moment / area)
 *   property_integral = sum area_i * (P(q0) + P(q1) + P(q2)) / 3 with the property grid of MC33_set_property_grid sampled at
 *              the vertices (a colour map is not needed); 0, and has_property 0, when none is attached
 *   bbox_min, bbox_max = the extent of the vertices (+inf / -inf for an empty surface)
 * The exact order of operations is in mc33_hip.h (mc33hip_measure_surface).  MC33_measure_components lists the connected
 * components (vertices joined through triangles) that have at least one triangle, in ascending order of `root`, the smallest
 * vertex index of the component; *unreferenced = vertices no triangle names.  With `capacity` below the number of components it
 * returns -2, the number in *components, and writes no row (table NULL, capacity 0 asks for the number).
 * MC33_measure_isosurface returns 0, or -1; MC33_measure_isosurfaces measures `count` isovalues, classifying up to eight per
 * pass over the grid like calculate_isosurfaces, and returns how many succeeded (a failed one leaves its struct zeroed).
 * All set extractor->iso like size_of_isosurface and leave memoryfault alone.
 * Refused with -1: an extractor spread over several devices (MC33_HIP_DEVICES with more than one slab: a slab's triangles name
 * vertices that live in its neighbour's arrays, so neither the sums nor the components are local to a device). */
typedef struct mc33_measure { unsigned nV, nT; double area, volume, moment[3], origin[3], bbox_min[3], bbox_max[3];
                              double property_integral; int has_property; } mc33_measure;
typedef struct mc33_component { unsigned root, nV, nT; double area, volume; } mc33_component;
int MC33_measure_isosurface(MC33 *extractor, MC33_real isovalue, mc33_measure *out);
unsigned MC33_measure_isosurfaces(MC33 *extractor, const MC33_real *isovalues, unsigned count, mc33_measure *out);
int MC33_measure_components(MC33 *extractor, MC33_real isovalue, mc33_component *table, unsigned capacity, unsigned *components,
                            unsigned *unreferenced);

/* extension (not in the reference): the topology of an isosurface, answered on the GPU from the triangle list alone - is it
 * closed, edge-manifold, consistently wound, and what is its genus.  The surface is extracted into device memory as for
 * MC33_measure_isosurface and nothing but these structs comes back.  Every side a -> b (a != b) of a triangle uses the edge
 * {min, max}: edges = distinct edges, boundary_edges = used once, nonmanifold_edges = used more than twice, misoriented_edges =
 * used twice in the same direction; degenerate_triangles name a vertex twice; boundary_loops = connected sets of boundary
 * edges; euler = referenced_vertices - edges + nT; closed = no boundary edge, oriented = no misoriented edge, manifold = no
 * non-manifold edge and no degenerate triangle (edge-manifold only: a pinched vertex is not detected).  Per component - the
 * rows of MC33_measure_components - the same counts and genus = (2 - euler - boundary_loops) / 2 where the component is manifold
 * and oriented and that is a whole number >= 0, else -1; genus_sum adds the rows with genus >= 0, genus_defined is 1 iff no row
 * has -1.  The exact definitions are in mc33_hip.h (mc33hip_surface_topology).
 * MC33_isosurface_topology returns 0, or -1; MC33_component_topology returns 0, -1, or -2 with the number in *components and
 * no row written when `capacity` is below it (table NULL, capacity 0 asks for the number).  Both set extractor->iso, leave
 * memoryfault alone and refuse with -1 an extractor spread over several devices. */
typedef struct mc33_topology { unsigned nV, nT; unsigned long long referenced_vertices, edges, boundary_edges, nonmanifold_edges,
                               misoriented_edges, degenerate_triangles, boundary_loops, components, closed_components, genus_sum;
                               long long euler; int closed, manifold, oriented, genus_defined; } mc33_topology;
typedef struct mc33_component_topology { unsigned root, nV, nT; unsigned long long edges, boundary_edges, nonmanifold_edges,
                                         misoriented_edges, degenerate_triangles, boundary_loops; long long euler; int genus;
                                       } mc33_component_topology;
int MC33_isosurface_topology(MC33 *extractor, MC33_real isovalue, mc33_topology *out);
int MC33_component_topology(MC33 *extractor, MC33_real isovalue, mc33_component_topology *table, unsigned capacity,
                            unsigned *components);

/* extension (not in the reference): how the surface bends - mean, Gaussian and principal curvatures of the level set of the grid
 * through every vertex, from the grid's gradient and second differences on the GPU (orthogonal grids, one device, at least 2
 * cells per axis; the operations one by one are in mc33_hip.h, mc33hip_curvature_vertices).  mean > 0 is convex seen from the
 * side N points to, in the plain flavours and in the _nneg ones alike: for a blob of high samples extracted by the plain library.
 * MC33_set_color_source chooses what a colour map (MC33_set_color_map) paints: MC33_COLOR_PROPERTY - the default - the property
 * grid, as before; MC33_COLOR_MEAN, _GAUSS, _K1, _K2 one of the curvatures, for which no property grid is needed.  With a map and
 * a curvature source calculate_isosurface(s), the filtered, smoothed, simplified and clipped calls and the points of a section
 * fill surface.color from the curvature of the FIELD at the vertices they colour today (a smoothed or simplified vertex has left
 * the field's surface: it gets the curvature of the level set it now lies on).  It returns 0, or -1 with nothing changed: an
 * unknown source; for a curvature source an inclined grid, an extractor spread over several devices, an axis with fewer than 2
 * cells, a device layer without the pass.
 * MC33_isosurface_curvature extracts into device memory like MC33_measure_isosurface and returns only the struct: the sizes,
 * lo[q] / hi[q] - the extremes of the finite values of mean, gauss, k1, k2 (q = 0 .. 3; +inf / -inf when there are none), what a
 * caller needs to choose the colour map's range -, the vertices whose four values are all finite and the others, and
 * total_mean / total_gauss: sum area_i * (C(q0) + C(q1) + C(q2)) / 3 of the mean and the Gaussian curvature, exactly the sum
 * MC33_measure_isosurface makes of a property (NaN, both, when a vertex is undefined).  For a closed surface total_gauss
 * approximates 2 pi times the Euler number of MC33_isosurface_topology.  It returns 0, or -1; sets extractor->iso, leaves
 * memoryfault alone, and refuses what MC33_set_color_source refuses for a curvature source. */
#define MC33_COLOR_PROPERTY 0
#define MC33_COLOR_MEAN 1
#define MC33_COLOR_GAUSS 2
#define MC33_COLOR_K1 3
#define MC33_COLOR_K2 4
typedef struct mc33_curvature { unsigned nV, nT; double lo[4], hi[4]; unsigned long long finite, undefined;
                                double total_mean, total_gauss; } mc33_curvature;
int MC33_set_color_source(MC33 *extractor, int source);
int MC33_isosurface_curvature(MC33 *extractor, MC33_real isovalue, mc33_curvature *out);

/* extension (not in the reference): keep or drop whole components of an isosurface on the GPU, so that only the kept rows cross
 * the link.  MC33_select_components is the ONE place where components are chosen - host C, no GPU: from the n rows of
 * MC33_measure_components (and, for closed_only, the n rows of MC33_component_topology; NULL otherwise) it writes the roots of the
 * rows to keep into roots[n], ascending, and returns how many; -1 on bad arguments (a null filter, null arrays with n > 0,
 * closed_only without topology rows).  A row passes when nT >= min_triangles AND area >= min_area AND |volume| >= min_abs_volume
 * AND (closed_only == 0 OR its boundary_edges == 0).  With largest > 0 only the `largest` passing rows with the most triangles
 * stay; ties go to the smaller root.  A zeroed filter keeps every row.  The area and volume columns are summed with atomics and
 * differ in their last bits from call to call: a threshold that close to a component's value may fall either way.
 * MC33_calculate_filtered_isosurface extracts the surface into device memory, colours it when a property grid and a colour map
 * are set, labels and measures its components there (and their topology, only when closed_only is set: the edge table takes
 * 16 bytes x 4 nT of device memory), selects, compacts on the device - vertices in ascending order, triangles in their order,
 * indices renumbered; a vertex no triangle names is always dropped (the definition is in mc33_hip.h, mc33hip_compact_components)
 * - and downloads the kept rows into a caller-owned `surface` like calculate_isosurface's.  *kept / *dropped count components
 * (either may be NULL).  Without colours surface.color is DefaultColorMC.  The extractor's iso, nV, nT and memoryfault are left as
 * calculate_isosurface leaves them for a surface of the returned size.  NULL on failure, for a null filter and for an extractor
 * spread over several devices. */
typedef struct { unsigned min_triangles; double min_area, min_abs_volume; unsigned largest; int closed_only; } mc33_component_filter;
int MC33_select_components(const mc33_component *table, const mc33_component_topology *topo /* NULL unless closed_only */,
                           unsigned n, const mc33_component_filter *f, unsigned *roots /* n */);   /* returns how many, -1 on bad arguments */
surface *MC33_calculate_filtered_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_component_filter *f, unsigned *kept,
                                            unsigned *dropped);

/* extension (not in the reference): a smoothed isosurface.  The integer grids of CT and MRI give staircase surfaces; Taubin's
 * lambda | mu smoothing - `iterations` times a pass with factor lambda in (0, 1] followed by one with mu in [-1, 0], every vertex
 * moved by the factor times (the mean of its edge neighbours - itself) - removes the steps without shrinking the surface.
 * pin_boundary != 0 leaves the vertices of open edges (the surface's rim on the grid's faces) where they are; a vertex without
 * neighbours never moves.  The exact order of operations is in mc33_hip.h (mc33hip_smooth_surface).
 * MC33_calculate_smoothed_isosurface extracts the surface into device memory, colours it from the UNSMOOTHED vertices when a
 * property grid and a colour map are set, smooths in place, recomputes N from the smoothed triangles (the sum of their cross
 * products per vertex, normalised; the stored winding decides the sign, in the _nneg flavours too) and downloads into a
 * caller-owned `surface` like calculate_isosurface's: T, nV and nT are unchanged.  The extractor's iso, nV, nT and memoryfault are
 * left as calculate_isosurface leaves them.  NULL for a null struct and for refused parameters (lambda, mu outside their ranges
 * or NaN, iterations above 1000) - the extractor is not touched then -, for an extractor spread over several devices, and on
 * failure (memoryfault 1). */
typedef struct { unsigned iterations; double lambda, mu; int pin_boundary; } mc33_smoothing;
surface *MC33_calculate_smoothed_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_smoothing *s);

/* extension (not in the reference): a simplified isosurface.  A 1024^3 extraction has tens of millions of triangles where a viewer,
 * a file or a remote client wants a few hundred thousand.  Vertex clustering: the vertices inside one cell of a lattice - origin
 * the grid's r0, cell[a] grid spacings d[a] wide along axis a; any positive finite number, 2 halves the resolution - become one
 * vertex, the mean of the cell's vertices (mode 0) or the first of them, which stays on the isosurface (mode 1); triangles that
 * lose a corner that way go and, with drop_duplicates != 0, so do triangles that repeat another; the winding of the others is
 * kept.  The exact definition is in mc33_hip.h (mc33hip_simplify_surface).
 * MC33_calculate_simplified_isosurface extracts the surface into device memory, colours it from the extracted vertices when a
 * property grid and a colour map are set (a merged vertex has the colour of the first of its cell), clusters on the device,
 * recomputes N from the simplified triangles (the stored winding decides the sign, in the _nneg flavours too) and downloads the
 * kept rows into a caller-owned `surface` like calculate_isosurface's.  The extractor's iso, nV, nT and memoryfault are left as
 * calculate_isosurface leaves them for a surface of the returned size.  NULL for a null struct and for refused parameters (a cell
 * component that is not finite and > 0, a mode that is neither) - the extractor is not touched then -, for an inclined grid, for an
 * extractor spread over several devices, and on failure (memoryfault 1). */
typedef struct { double cell[3]; int mode; int drop_duplicates; } mc33_simplification;   /* cell in units of the grid spacing d */
surface *MC33_calculate_simplified_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_simplification *s);

/* extension (not in the reference): an isosurface cut open by planes, or cropped to a box - what a viewer of nested or closed
 * surfaces does first.  Of every plane a x + b y + c z + w, in the coordinates of surface.V, the half space >= 0 stays: triangles
 * inside stay, triangles the plane crosses are cut, and the new vertices on the cut edges are shared by the triangles on either
 * side, with interpolated normals.  A vertex that lies exactly on a plane is never duplicated.  The cut is not capped.  The exact
 * definition is in mc33_hip.h (mc33hip_clip_surface).
 * MC33_clip_box is host C, no GPU: the six planes of the box [lo, hi] in the fixed order x - lo[0], hi[0] - x, y - lo[1],
 * hi[1] - y, z - lo[2], hi[2] - z - plane[2 a] = +1 on axis a with w = -lo[a], plane[2 a + 1] = -1 on axis a with w = hi[a] -
 * and n = 6.  It returns 0, or -1 - nothing is written then - for a null pointer, a bound that is not finite or lo[a] >= hi[a].
 * MC33_calculate_clipped_isosurface extracts the surface into device memory, applies the n <= 6 planes one after another on the
 * device, colours the FINAL vertices when a property grid and a colour map are set (a new vertex gets the colour of its own
 * position) and downloads only the kept rows into a caller-owned `surface` like calculate_isosurface's.  n == 0 is plain
 * extraction; a result without triangles is an empty surface, not a failure.  Inclined grids are accepted: the planes are in the
 * coordinates of the returned vertices.  The extractor's iso, nV, nT and memoryfault are left as calculate_isosurface leaves them
 * for a surface of the returned size.  NULL for a null struct, n > 6 and a refused plane (a component that is not finite, or a, b,
 * c all zero) - the extractor is not touched then -, for an extractor spread over several devices, and on failure (memoryfault 1). */
typedef struct { unsigned n; double plane[6][4]; } mc33_clip;   /* the coordinates of surface.V */
surface *MC33_calculate_clipped_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_clip *planes);
int MC33_clip_box(const double lo[3], const double hi[3], mc33_clip *out);

/* extension (not in the reference): an isosurface closed where it runs into the faces of the grid - MC33 stops there and leaves
 * the surface open, so that its signed volume means nothing, its components do not count as closed and a printer or a mesher
 * cannot take it.  The caps are made on the device: on every face of a box of grid points lo .. hi (lo[a] < hi[a] <= N[a]; hi all
 * zero: the whole grid) the solid side of the face's samples is triangulated cell by cell, with new vertices at the solid grid
 * points, joined to the surface's own rim vertices: one consistently wound mesh without boundary.  The solid side is the one the
 * surface's winding turns its back on - F > isovalue in the plain libraries, F < isovalue in the _nneg flavours; invert != 0 caps
 * the other side and returns the surface with its winding and normals reversed (a dark object in a bright field).  Face cells
 * with a sample equal to the isovalue (integer isovalues in CT data) or a NaN are skipped and counted: the result keeps boundary
 * edges there and closed is 0.  The exact definition is in mc33_hip.h (mc33hip_cap_surface).
 * MC33_calculate_capped_isosurface extracts the surface into device memory, caps it there, colours the FINAL vertices when a
 * property grid and a colour map are set (a new vertex gets the colour of its own position) and downloads once into a caller-owned
 * `surface` like calculate_isosurface's.  options NULL: the whole grid, invert 0; info NULL: no counts wanted.  The extractor's iso,
 * nV, nT and memoryfault are left as calculate_isosurface leaves them for a surface of the returned size.  NULL for an inclined
 * grid, for an extractor spread over several devices and for a refused box - the extractor is not touched then - and on failure
 * (memoryfault 1). */
typedef struct { unsigned lo[3], hi[3]; int invert; } mc33_cap;
typedef struct {
	unsigned nV, nT;                  /* of the returned surface */
	unsigned cap_vertices, cap_triangles, rim_segments, capped_cells, skipped_cells, off_face_edges;
	int solid_above, closed;          /* the side that was capped (1: F > isovalue); 1: nothing was skipped, the surface has no boundary */
} mc33_cap_info;
surface *MC33_calculate_capped_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_cap *options, mc33_cap_info *info);

/* extension (not in the reference, whose only callers are two interactive viewers): pictures of an isosurface made on the device - a
 * depth-tested, shaded image, a depth buffer and an id buffer (the triangle under every pixel: picking).  A card without a display
 * usually sits in a machine nobody sits at; a 1024 x 1024 picture is 4 MB where the surface it shows is hundreds.
 * mc33_view: m, row major, takes (x, y, z, 1) in the coordinates of the vertices to clip coordinates - x, y in -1 .. 1 over the image
 * after the division by w, y up, depth 0 .. 1; cull 0 none, 1 back, 2 front (the front is the side the normals point to);
 * two_sided != 0 lights both sides; light is a direction in the coordinates of the vertices; a pixel's colour is the interpolated
 * vertex colour times ambient + diffuse cos; background is a colour word 0xAABBGGRR like surface.color.  The exact definition is
 * in mc33_hip.h (mc33hip_render_surface).
 * MC33_render_isosurface extracts once into device memory - colours from the property grid or the curvature source when a colour
 * map is set, else DefaultColorMC -, renders the n views one after another and downloads only the arrays `want` names (MC33_IMAGE_RGBA
 * | MC33_IMAGE_DEPTH | MC33_IMAGE_IDS) into malloc blocks that MC33_free_image releases; row 0 is the top row.  Returns n, or -1 with
 * out untouched.  It sets the extractor's iso like size_of_isosurface and leaves memoryfault, nV, nT, T and V alone.  -1 with the
 * extractor untouched as well: a null pointer, n == 0, `want` without a known bit, a view the device call refuses (a size outside
 * 1 .. 4096, a matrix entry, light component, ambient or diffuse that is not finite, a light without direction, a cull outside 0 ..
 * 2), an extractor spread over several devices.
 * MC33_view_fit (host only) fills *out with a view that frames the grid's bounding box - of an inclined grid, its sheared box - seen
 * along dir with up upwards: fov_degrees 0 is orthographic, up to 170 a perspective with that vertical field of view; pixels are
 * square; depth 0 .. 1 spans the box; light = -dir (a headlight), ambient 0.2, diffuse 0.8, cull 0, two_sided 1, background opaque
 * black.  -1 with nothing written: a null pointer, a zero or non-finite dir or up, up parallel to dir, fov outside [0, 170], a size
 * outside 1 .. 4096.
 * MC33_write_image_ppm writes rgba as a binary P6 file; -1 without an rgba array or when the file cannot be written. */
#define MC33_IMAGE_RGBA 1u
#define MC33_IMAGE_DEPTH 2u
#define MC33_IMAGE_IDS 4u
typedef struct {
	double m[16];
	unsigned width, height;
	int cull, two_sided;
	double light[3], ambient, diffuse;
	unsigned background;
} mc33_view;
typedef struct {
	unsigned width, height;
	unsigned *rgba;                   /* width x height words 0xAABBGGRR, or NULL */
	float *depth;                     /* +inf where nothing was drawn */
	unsigned *triangle;               /* 0xFFFFFFFF where nothing was drawn */
	unsigned drawn, culled, degenerate, rejected, offscreen, invalid_triangles;   /* triangles by class */
	unsigned long long fragments, covered;
	unsigned nV, nT;                  /* of the surface that was drawn */
} mc33_image;
int MC33_render_isosurface(MC33 *extractor, MC33_real isovalue, const mc33_view *views, unsigned n, unsigned want, mc33_image *out);
void MC33_free_image(mc33_image *image);
int MC33_view_fit(MC33 *extractor, const double dir[3], const double up[3], double fov_degrees, unsigned width, unsigned height, mc33_view *out);
int MC33_write_image_ppm(const mc33_image *image, const char *filename);

/* extension (not in the reference): how far two surfaces are from each other, taken on the device - the nearest triangle of one for
 * every vertex of the other.  The surfaces stay in device memory; a few numbers come back.  The exact definition is in mc33_hip.h
 * (mc33hip_surface_distance); the distance is a property of V and T alone, so inclined grids are accepted.
 * MC33_isosurface_distance: the vertices of the surface of iso_from against the triangles of the surface of iso_to, of the same
 * grid - the thickness of the shell between two isovalues, seen from the first.
 * MC33_simplification_error: what MC33_calculate_simplified_isosurface(iso, s) gives away - out[0] the simplified surface's vertices
 * against the full surface, out[1] the full surface's vertices against the simplified one.  Orthogonal grids only, as the
 * simplification itself.
 * Both are SAMPLED AT VERTICES: the interior of a coarse triangle can be farther from the other surface than any of its corners.
 * points: the vertices with a nearest triangle; unmatched: those without (a coordinate that is not finite); max, min, mean, rms over
 * the former; argmax: the first vertex that attains max.
 * 0; -1 when refused - a null pointer, parameters the simplification refuses, an extractor spread over several devices - with the
 * extractor untouched, or when the device fails; -2 when either surface is empty, with out zeroed.  Both set the extractor's iso
 * and leave nV, nT and memoryfault alone, as the measuring calls do. */
typedef struct { unsigned long long points, unmatched; double max, min, mean, rms; unsigned argmax; } mc33_distance;
int MC33_isosurface_distance(MC33 *extractor, MC33_real iso_from, MC33_real iso_to, mc33_distance *out);
int MC33_simplification_error(MC33 *extractor, MC33_real isovalue, const mc33_simplification *s, mc33_distance out[2]);

/* extension (not in the reference): the section of an isosurface by a plane - the outline a viewer draws over a slice image, its
 * length, the area it encloses, and the same along a stack of parallel planes: the cross-sectional area profile of a vessel, a
 * bone or a pore.  The surface stays in device memory; only the outline, or a few numbers per plane, come back.  plane[4] = a, b,
 * c, w in the coordinates of surface.V (inclined grids are accepted); the section is the boundary that
 * MC33_calculate_clipped_isosurface opens with the same plane.  The exact definition is in mc33_hip.h (mc33hip_section_surface).
 * MC33_section_isosurface extracts, sections on the device, colours the points - each at its own position - when a property grid
 * and a colour map are set (DefaultColorMC otherwise) and downloads the section into malloc blocks that MC33_free_section
 * releases: P (nP points), S (nS directed segments a -> b of point indices, in the order of the surface's triangles: the
 * orientation follows the winding), contour (per point: the smallest point index joined to it through segments), next (per point:
 * the end of the one segment that starts there, 0xFFFFFFFF when none or several do - a closed contour is walked with it), color,
 * the counts, length, area and the plane.  area is SIGNED: area has the sign of the volume that MC33_measure_isosurface reports for
 * a closed surface - it follows the stored winding, so the MC33_NORMAL_NEG flavours give the opposite sign (for the reference's
 * README sphere, samples growing outwards, the plain libraries give volume < 0 and area < 0) - and |area| is the enclosed area only
 * where every contour is closed (closed_contours == contours).  A plane that misses gives an empty section, not a failure.
 * MC33_section_contours fills one row per contour, in ascending order of root (= the contour word of its points): 0; -1 on
 * failure; -2 when the table is too small - *contours is filled, the table untouched (capacity 0 with a NULL table asks for the
 * number).  The double columns are added with atomics on the device and may differ in their last bits from call to call.
 * MC33_section_profile: n <= 255 finite offsets w_k, strictly ascending; out[k] holds what MC33_section_isosurface would report
 * for the plane (normal, w_k) - segments exactly, length and area up to the order of their additions - from one pass over the
 * triangles: 0, or -1.
 * All three set the extractor's iso and leave nV, nT and memoryfault alone, as the measuring calls do.  NULL / -1 and the extractor
 * untouched: a null pointer, a plane or normal with a component that is not finite or with a, b, c all zero, bad offsets, an
 * extractor spread over several devices. */
typedef struct {
	unsigned nP, nS;
	MC33_real (*P)[3];
	unsigned (*S)[2];
	unsigned *contour, *next;
	int *color;
	unsigned on_points, cut_points, contours, closed_contours, open_ends, branch_points, degenerate_segments;
	double length, area;
	double plane[4];
} mc33_section;
typedef struct {
	unsigned root, points, segments, open_ends, branch_points;
	int closed;
	double length, area;
} mc33_contour;
typedef struct { unsigned long long segments; double length, area; } mc33_section_level;
mc33_section *MC33_section_isosurface(MC33 *extractor, MC33_real isovalue, const double plane[4]);
void MC33_free_section(mc33_section *section);
int MC33_section_contours(MC33 *extractor, MC33_real isovalue, const double plane[4], mc33_contour *table, unsigned capacity, unsigned *contours);
int MC33_section_profile(MC33 *extractor, MC33_real isovalue, const double normal[3], const double *offsets, unsigned n, mc33_section_level *out);

/* extension (not in the reference): the grid resampled on the GPU before anything is extracted from it.  A Gaussian of about one
 * sample removes the speckle of CT / MRI volumes that otherwise becomes thousands of tiny components; a stride of 2 or 3 per axis
 * gives a preview surface of an eighth or a twenty-seventh of the triangles without extracting the full one first.  Per axis a
 * (x, y, z): a Gaussian of sigma[a] SAMPLES cut off at radius[a] <= 8 samples (0: ceil(3 sigma), at least 1; sigma 0: no smoothing
 * along that axis), then every stride[a]-th point is kept, the first included: (N[a] / stride[a]) intervals, d[a] * stride[a] wide,
 * r0 unchanged.  Edge samples are replicated.  Integer grids are rounded to nearest and clamped to their range.  The arithmetic is
 * double and its order is fixed: the exact definition is in mc33_hip.h (mc33hip_resample_grid).
 * MC33_gaussian_taps is host C, no GPU: the 2 r + 1 weights into taps[] (room for 17), e_i = exp(-(i * i) / (2 sigma^2)) for
 * i = 0 .. r, normalised by S = e_0 + sum of (e_i + e_i) in ascending i.  It returns r, or -1 for a negative, NaN or infinite sigma,
 * a NULL taps or r > 8.
 * MC33_create_resampled returns a NEW, independent extractor whose grid exists only in device memory (the library allocates it and
 * free_MC33 releases it; `source` may be freed first): nx, ny, nz are the new interval counts, O is unchanged, D, ca, cb follow
 * from the new spacing by the rules of create_MC33, F is NULL; an inclined source stays inclined.  The property grid and the colour
 * map are not carried over (MC33_set_property_grid with a _GRD of the new size works as on any object); MC33_grid_changed and
 * MC33_HIP_REUPLOAD do nothing on it; every other entry point works as on any object, MC33_create_resampled included.
 * NULL, with `source` untouched: a null or refused struct (the rules of MC33_gaussian_taps, a zero stride, fewer than 2 points left
 * on an axis), a source spread over several devices (MC33_HIP_DEVICES), a failure of the device.
 * MC33_resampled_grid downloads that grid into a fresh _GRD with alloc_F rows - N, r0, the new d, the inclined members - to be
 * released with free_memory_grd; NULL for an object that neither MC33_create_resampled nor MC33_create_ranked made. */
typedef struct { double sigma[3]; unsigned radius[3]; unsigned stride[3]; } mc33_resampling;  /* sigma in samples; 0: none; radius 0: ceil(3 sigma) */
int MC33_gaussian_taps(double sigma, unsigned radius, double *taps);
MC33 *MC33_create_resampled(MC33 *source, const mc33_resampling *r);
_GRD *MC33_resampled_grid(MC33 *resampled);

/* extension (not in the reference): the grid rank-filtered on the GPU before anything is extracted from it.  Every grid point is
 * replaced by the minimum, the median or the maximum of the samples in a box window of radius[a] samples along axis a (x, y, z)
 * around it, edge samples replicated.  A 3 x 3 x 3 median (radius 1, 1, 1) removes isolated spikes and leaves a step edge where it
 * is, which a Gaussian does not; radius (1, 1, 0) is the per-slice 3 x 3 median of anisotropic stacks.  A minimum followed by a
 * maximum of the same radius is an opening (small specks go), the other order a closing (small gaps are bridged): the objects
 * chain.  The filter selects one of its input samples and computes nothing new - NaN samples and -0 have a place in its order and
 * keep their bytes; the exact definition is in mc33_hip.h (mc33hip_rank_grid).  MC33_RANK_MIN and MC33_RANK_MAX take radii up to 8,
 * MC33_RANK_MEDIAN up to 1; all radii 0 copies the grid.
 * MC33_create_ranked returns a NEW, independent extractor of the same nx, ny, nz, O and D whose grid exists only in device memory,
 * with everything MC33_create_resampled says about its object: free_MC33 releases it and `source` may be freed first; F is NULL; an
 * inclined source stays inclined; the property grid and the colour map are not carried over; MC33_grid_changed and
 * MC33_HIP_REUPLOAD do nothing on it; every other entry point works as on any object, MC33_create_ranked and MC33_create_resampled
 * included; MC33_resampled_grid downloads its grid.
 * NULL, with `source` untouched: a null or refused struct (a rank that is none of the three, a radius above its limit), a source
 * spread over several devices (MC33_HIP_DEVICES), a failure of the device. */
#define MC33_RANK_MIN    0
#define MC33_RANK_MEDIAN 1
#define MC33_RANK_MAX    2
typedef struct { unsigned radius[3]; int rank; } mc33_ranking;  /* radius per axis x, y, z, in samples */
MC33 *MC33_create_ranked(MC33 *source, const mc33_ranking *r);

/* extension (not in the reference): the contour spectrum of the grid - what a caller needs to choose an isovalue, from one pass
 * over the volume on the GPU instead of one size_of_isosurface per candidate.  For `count` <= 255 isovalues, strictly ascending as
 * MC33_real, none a NaN: cut_cells[k] is the number of cells the surface of isovalues[k] cuts, histogram[j], j <= count, the number
 * of grid points whose sample lies above exactly j of the isovalues (a NaN sample: count when its sign bit is set, else 0), and
 * *info (may be NULL) the totals, the NaN samples and the exact range of the other samples as MC33_real.  count == 0 is legal:
 * histogram[0] grid points and the range - the first call of a two-step ladder.  The exact definition is in mc33_hip.h
 * (mc33hip_grid_spectrum).  A grid marked by MC33_grid_changed / MC33_HIP_REUPLOAD is uploaded first, as size_of_isosurface does;
 * the MC33 struct stays byte for byte as it was, iso, nV, nT and memoryfault included.  Works on objects made by
 * MC33_create_resampled and - unlike the mesh extensions - on an extractor spread over several devices (MC33_HIP_DEVICES): every
 * slab counts its own slices, the integers are added and the extremes combined.  Returns 0, or -1 - nothing is written then - for a
 * refused argument or a failure of the device.
 * MC33_isovalue_ladder is host C, no GPU: n <= 255 steps strictly between lo and hi,
 * out[k] = (MC33_real)(lo + (hi - lo) * ((double)(k + 1) / (double)(n + 1))).  It returns n, or -1 for bounds that are not finite,
 * lo >= hi, n > 255, a NULL array, or steps that are not strictly ascending after the conversion. */
typedef struct {
	unsigned long long points, cells, nan_samples;
	double sample_min, sample_max;   /* +inf / -inf when every sample is a NaN */
} mc33_spectrum_info;
int MC33_grid_spectrum(MC33 *M, const MC33_real *isovalues, unsigned count, unsigned long long *cut_cells, unsigned long long *histogram,
                       mc33_spectrum_info *info);
int MC33_isovalue_ladder(double lo, double hi, unsigned n, MC33_real *out);

/* ---- inclined grids (reference header :186-191) ---------------------------------------------------------
 * c = A b (transposed == 0) or A^T b for a 3x3 matrix; _multTSA_bf assumes an upper triangular A.  A caller may
 * point mult_Abf at either; calculate_isosurface looks at the pointer when it is called and runs the matching
 * form on the GPU (any other function: NULL + memoryfault). */
void _multA_bf(const double (*A)[3], MC33_real *b, MC33_real *c, int transposed);
void _multTSA_bf(const double (*A)[3], MC33_real *b, MC33_real *c, int transposed);
extern void (*mult_Abf)(const double (*A)[3], MC33_real *b, MC33_real *c, int transposed);

/* ---- surface files (reference header :193-222), host C: csrc/mc33_surface_io.c --------------------------- */
int write_bin_s(surface *s, const char *path);     /* ".sup" / ".sud" binary container; 0 on success, -1 on failure */
surface *read_bin_s(const char *path);             /* NULL on failure; reads both precisions                         */
int write_txt_s(surface *s, const char *path);
int write_obj_s(surface *s, const char *path);     /* Wavefront OBJ with per-vertex normals                          */
int write_ply_s(surface *s, const char *path, const char *author, const char *object); /* ASCII PLY               */

/* ---- grid containers (reference header :263-329), host C --------------------------------------------------- */
int alloc_F(_GRD *grid);                            /* rows for N[] + 1 points per axis; 0 on success               */
void free_memory_grd(_GRD *grid);
_GRD *grid_from_data_pointer(unsigned points_x, unsigned points_y, unsigned points_z, GRD_data_type *samples);
_GRD *generate_grid_from_fn(double x0, double y0, double z0, double x1, double y1, double z1,
                            double step_x, double step_y, double step_z, double (*f)(double, double, double));

/* ---- grid files (reference header :263-311), host C: csrc/mc33_grid_io.c; NULL on failure ------------------ */
_GRD *read_grd(const char *path);                   /* DMol .grd text file (may describe an inclined cell)         */
_GRD *read_grd_binary(const char *path);            /* the library's own binary container ("_GRD")                 */
_GRD *read_scanfiles(const char *first_file, unsigned resolution, int swap_bytes); /* numbered res x res u16 slices */
_GRD *read_raw_file(const char *path, unsigned *points, int bytes_per_sample, int is_float); /* bare samples     */
_GRD *read_dat_file(const char *path);              /* u16 nx, ny, nz header + u16 samples                         */

#ifdef __cplusplus
}
#endif
#endif /* marching_cubes_33_h */
