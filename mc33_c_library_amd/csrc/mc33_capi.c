/* mc33_capi.c -- host layer in C: the reference's public API (include/marching_cubes_33.h) on top of the
 * device-level C ABI (include/mc33_hip.h).  No HIP types here; everything GPU-side happens behind
 * mc33hip_*.  "MC:" = reference source/marching_cubes_33.c, "UTIL:" = reference source/MC33_util_grd.c.
 *
 * Behaviour kept from the reference:
 *   - create_MC33 snapshots N, r0, d (MC:1758-1782) and returns NULL on failure (MC:1753-1757);
 *   - calculate_isosurface returns a caller-owned `surface` whose T, V, N, color and the struct itself
 *     are five separate malloc blocks (MC:84-92 frees them one by one); an empty result is a zeroed,
 *     non-NULL surface (MC:1880-1883); failure is NULL with M->memoryfault = 1 (MC:1884-1887);
 *   - every vertex gets DefaultColorMC (MC:1875-1877); S->user is left alone (MC:1873 copies 52 bytes).
 * Deliberate difference: the grid is copied to HBM in create_MC33 and stays resident.  A caller that
 * rewrites G->F between calls sets MC33_HIP_REUPLOAD=1 (re-upload before every extraction).
 */
#define _DEFAULT_SOURCE /* madvise, clock_gettime */
#include <float.h>
#include <math.h>
#include <malloc.h> /* malloc_usable_size: asked only about blocks this library allocated itself */
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <string.h>
#include <sys/mman.h>

#include "../../include/marching_cubes_33.h"
#include "../../include/mc33_hip.h"

/* layout contract with programs compiled against the reference header */
#ifdef GRD_ORTHOGONAL /* measured against the reference header compiled with -DGRD_ORTHOGONAL */
_Static_assert(sizeof(_GRD) == 256 && offsetof(_GRD, d) == 48 && offsetof(_GRD, periodic) == 84 &&
               offsetof(_GRD, internal_data) == 88 && offsetof(_GRD, title) == 92, "_GRD layout differs from the reference (GRD_ORTHOGONAL)");
#else
_Static_assert(sizeof(_GRD) == 416 && offsetof(_GRD, d) == 48 && offsetof(_GRD, nonortho) == 96 &&
               offsetof(_GRD, internal_data) == 252, "_GRD layout differs from the reference");
#endif
_Static_assert(sizeof(surface) == 64 && offsetof(surface, iso) == 48 && offsetof(surface, user) == 56,
               "surface layout differs from the reference");
#ifdef GRD_ORTHOGONAL
#define MC33_MATS 0 /* bytes of _A, A_ missing from MC33 */
#else
#define MC33_MATS 144
#endif
#if GRD_TYPE_SIZE == 8 /* measured against the reference header compiled with -DGRD_TYPE_SIZE=8 */
_Static_assert(sizeof(MC33) == 200 + MC33_MATS && offsetof(MC33, memoryfault) == 56 && offsetof(MC33, O) == 72 && offsetof(MC33, nx) == 136 &&
               offsetof(MC33, store) == 152 && offsetof(MC33, Dx) == 160 + MC33_MATS, "MC33 layout differs from the reference (double build)");
#else
_Static_assert(sizeof(MC33) == 160 + MC33_MATS && offsetof(MC33, memoryfault) == 52 && offsetof(MC33, nx) == 96 &&
               offsetof(MC33, store) == 112 && offsetof(MC33, Dx) == 120 + MC33_MATS, "MC33 layout differs from the reference");
#endif

#ifndef DEFAULT_SURFACE_COLOR
#define DEFAULT_SURFACE_COLOR 0xff5c5c5c /* grey, 0xAABBGGRR (MC:76-78) */
#endif
#ifndef MC33_NORMAL_NEG
#define MC33_NORMAL_NEG 0 /* 1: front and back exchanged, reference source/libMC33.c:20-22 (the _nneg flavour of the library) */
#endif
int DefaultColorMC = (int)DEFAULT_SURFACE_COLOR;

/* The property-grid entry points of the device layer are referenced weakly: a device layer without them (the emulated one of
 * the CPU tests of this file's host logic) leaves their addresses null, and MC33_set_property_grid then refuses. */
#pragma weak mc33hip_property_upload_rows
#pragma weak mc33hip_property_drop
#pragma weak mc33hip_color_vertices
#pragma weak mc33hip_download_enqueue
/* ... and so are the measuring ones (MC33_measure_*): without them these functions return -1 */
#pragma weak mc33hip_sample_property
#pragma weak mc33hip_measure_surface
#pragma weak mc33hip_label_components
#pragma weak mc33hip_measure_components
#pragma weak mc33hip_surface_topology
#pragma weak mc33hip_component_topology
#pragma weak mc33hip_compact_components
#pragma weak mc33hip_smooth_surface
#pragma weak mc33hip_simplify_surface
#pragma weak mc33hip_clip_surface
#pragma weak mc33hip_cap_surface
#pragma weak mc33hip_render_surface
#pragma weak mc33hip_surface_distance
#pragma weak mc33hip_section_surface
#pragma weak mc33hip_section_contours
#pragma weak mc33hip_section_ladder
#pragma weak mc33hip_download /* (the host layer uses it for the blocks of a section only) */
/* ... and the resampling ones (MC33_create_resampled): without them it returns NULL */
#pragma weak mc33hip_resampled_size
#pragma weak mc33hip_resample_grid
#pragma weak mc33hip_context_device
#pragma weak mc33hip_rank_grid /* (MC33_create_ranked: without it NULL) */
#pragma weak mc33hip_adopt_device /* (the host layer uses it for the resampled grid only) */
#pragma weak mc33hip_grid_stable  /* (... whose samples nobody but this library writes) */
/* ... and the contour spectrum (MC33_grid_spectrum): without it that function returns -1 */
#pragma weak mc33hip_grid_spectrum
/* ... and the curvature pass (MC33_set_color_source, MC33_isosurface_curvature): without it both refuse a curvature */
#pragma weak mc33hip_curvature_vertices
#pragma weak mc33hip_color_values
_Static_assert(sizeof(mc33_component) == sizeof(mc33hip_component) && offsetof(mc33_component, area) == offsetof(mc33hip_component, area),
               "mc33_component and mc33hip_component are one layout");

/* One z-slab of the grid on one device (the same cut as mc33_c_library_amd/slabs.py makes per rank): cell slices
 * [z_begin, z_end), one ghost slice below (its vertices belong to the slab underneath, but the slab's triangles refer to them),
 * resident sample planes [p_lo, p_hi] = the cells' own, one above for the central differences of the normals (MC:888-890,
 * 1036-1038), the ghost slice's lower plane and one below that for vertices on grid points (MC:643-647).  Without
 * MC33_HIP_DEVICES there is one slab: the whole grid on the current device. */
#define MC33_MAX_DEVICES 16
struct staging {     /* device staging of a result, grown on demand; two sets so that calculate_isosurfaces can */
	void *dV, *dN, *dT; /* download one surface while the next is being extracted                           */
	unsigned long long capV, capT;
	void *dC;           /* colours of the vertices in dV (only with a property grid and a colour map)           */
	unsigned long long capC;
};
struct mc33_private_s;
typedef struct {
	struct mc33_private_s *owner;
	mc33hip_ctx *ctx;
	int device;
	unsigned z_begin, z_end, ghost, p_lo, p_hi;
	struct staging set[2];
	mc33hip_counts cnt; /* of the count in flight */
	MC33_real iso;
	int rc;
	struct mc33_surface *out;   /* the surface being filled, and where this slab's vertices / triangles begin in it */
	unsigned long long vbase, tbase;
	mc33hip_spectrum *spectrum; /* MC33_grid_spectrum: this slab's share, for the length of the call */
} mc33_slab;

/* private object: the public MC33 first, so callers can keep treating the pointer as MC33* */
typedef struct mc33_private_s {
	MC33 pub;
	unsigned long long magic;
	int nslab;           /* 1, or the number of devices named by MC33_HIP_DEVICES */
	mc33_slab slab[MC33_MAX_DEVICES];
	_GRD *grid;          /* for MC33_HIP_REUPLOAD */
	int reupload;
	int grid_dirty;      /* MC33_grid_changed: the caller rewrote samples of G->F, upload them before the next extraction */
	int inclined;        /* G->nonortho at create time: the MC33_spnC store */
	double grd_A[9], grd_Ai[9];
	double grd_r0[3], grd_d[3]; /* G->r0, G->d at create time: the lattice of MC33_calculate_simplified_isosurface */
	_GRD *prop;          /* MC33_set_property_grid: attached on every slab (only read while it is being uploaded) */
	int has_map;         /* MC33_set_color_map */
	unsigned map_n;
	int map[256];
	double map_lo, map_hi;
	int nan_color;       /* DefaultColorMC when the surface under way was made */
	void *own_grid;      /* MC33_create_resampled, MC33_create_ranked: the grid, in device memory only, adopted by slab[0].ctx; released in free_MC33 */
	size_t own_pitch, own_slice; /* ... its layout, in samples */
	void *dP, *dL;       /* MC33_measure_*: property values / component labels of the vertices in slab[0].set[0] (device) */
	unsigned long long capP, capL;
	int color_source;    /* MC33_set_color_source: MC33_COLOR_PROPERTY, or the curvature the map paints (one slab then) */
	void *dG;            /* MC33_isosurface_curvature: the Gaussian curvature beside the mean in dP (device) */
	unsigned long long capG;
	void *dImg[3];       /* MC33_render_isosurface: colour, depth and id image of the view under way (device) */
	unsigned long long capImg[3];
} mc33_private;
#define MC33_MAGIC 0x4D43333348495031ull /* "MC33HIP1" */

static mc33_private *priv(MC33 *M) {
	mc33_private *p = (mc33_private *)M;
	return (p && p->magic == MC33_MAGIC) ? p : 0;
}

/* Growable device arrays (the staging arrays, the measuring words): dev_room is the one place where one is made to hold at least n
 * elements of elem_bytes - released and made anew with an eighth and 1024 elements to spare when it is missing or too small; what
 * it held is not kept.  Success leaves *cap >= n; failure leaves (0, 0) and returns -1. */
static void dev_release(mc33hip_ctx *ctx, void **ptr, unsigned long long *cap) {
	if (*ptr) mc33hip_device_free(ctx, *ptr);
	*ptr = 0; *cap = 0;
}
static int dev_room(mc33hip_ctx *ctx, void **ptr, unsigned long long *cap, unsigned long long n, size_t elem_bytes) {
	if (*ptr && *cap >= n)
		return 0;
	dev_release(ctx, ptr, cap);
	const unsigned long long c = n + n / 8 + 1024;
	if (mc33hip_device_alloc(ctx, ptr, c * elem_bytes) != MC33HIP_OK) return -1;
	*cap = c;
	return 0;
}
static void staging_release(mc33hip_ctx *ctx, struct staging *g) {
	unsigned long long capN = 0; /* (V and N share capV) */
	dev_release(ctx, &g->dV, &g->capV); dev_release(ctx, &g->dN, &capN); dev_release(ctx, &g->dT, &g->capT); dev_release(ctx, &g->dC, &g->capC);
}

/* runs fn on every slab: the slabs of one device one after the other, the devices side by side - the device-level calls block
 * (count: until the counters are on the host; emit: the runtime's copies into pageable memory return when the data has arrived),
 * so every device gets a thread and its link is busy at the same time as the others'.  (Slabs that share a device - the
 * rehearsal on a one-GPU machine - gain nothing from threads of their own: eight threads copying from one GPU into pieces of the
 * same arrays took 10 ms where one takes 3.5, profiles/r05_capi_walls.txt.) */
struct slab_group {
	void *(*fn)(void *);
	mc33_slab *slab[MC33_MAX_DEVICES];
	int n;
};
static void *slab_group_run(void *arg) {
	struct slab_group *g = (struct slab_group *)arg;
	for (int k = 0; k != g->n; k++)
		g->fn(g->slab[k]);
	return 0;
}
static void for_each_slab(mc33_private *p, void *(*fn)(void *)) {
	struct slab_group grp[MC33_MAX_DEVICES];
	int ngrp = 0;
	for (int k = 0; k != p->nslab; k++) {
		int g = 0;
		while (g != ngrp && grp[g].slab[0]->device != p->slab[k].device) g++;
		if (g == ngrp) { grp[ngrp].fn = fn; grp[ngrp].n = 0; ngrp++; }
		grp[g].slab[grp[g].n++] = &p->slab[k];
	}
	pthread_t th[MC33_MAX_DEVICES];
	int started[MC33_MAX_DEVICES];
	for (int g = 1; g < ngrp; g++)
		started[g] = pthread_create(&th[g], 0, slab_group_run, &grp[g]) == 0;
	slab_group_run(&grp[0]); /* the first device's on the calling thread */
	for (int g = 1; g < ngrp; g++) {
		if (started[g]) pthread_join(th[g], 0);
		else slab_group_run(&grp[g]);
	}
}

/* ... and the code of the first slab whose fn failed (MC33HIP_OK: none did) */
static int run_slabs(mc33_private *p, void *(*fn)(void *)) {
	for_each_slab(p, fn);
	for (int k = 0; k != p->nslab; k++)
		if (p->slab[k].rc != MC33HIP_OK)
			return p->slab[k].rc;
	return MC33HIP_OK;
}

static void *slab_create(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	mc33_private *p = s->owner;
	const _GRD *G = p->grid;
	mc33hip_grid_desc d;
	memset(&d, 0, sizeof d);
	d.npx = G->N[0] + 1; d.npy = G->N[1] + 1; d.npz_resident = s->p_hi - s->p_lo + 1;
	d.plane0 = s->p_lo; d.nz_total = G->N[2];
	for (int j = 0; j != 3; j++) { d.r0[j] = G->r0[j]; d.d[j] = G->d[j]; }
	d.sample_bytes = (int)sizeof(GRD_data_type);
	d.device = s->device;
	s->rc = mc33hip_create(&s->ctx, &d);
	if (s->rc == MC33HIP_OK) s->rc = mc33hip_set_normal_neg(s->ctx, MC33_NORMAL_NEG);
	if (s->rc == MC33HIP_OK && p->nslab > 1) s->rc = mc33hip_own_stream(s->ctx); /* several contexts: each on a stream of its own */
	if (s->rc == MC33HIP_OK) s->rc = mc33hip_upload_rows(s->ctx, (const void *const *const *)(G->F + s->p_lo));
	return 0;
}

static void *slab_upload(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	s->rc = mc33hip_upload_rows(s->ctx, (const void *const *const *)(s->owner->grid->F + s->p_lo));
	return 0;
}

/* MC33_HIP_DEVICES: "all", or a comma-separated list of HIP device ordinals - the z-slabs of the grid go to these devices in this
 * order.  An ordinal may appear several times (several slabs on one GPU: how the path is rehearsed on a one-GPU machine).
 * Returns the number of entries (0: not set - one slab on the current device). */
static int parse_devices(int *dev) {
	const char *e = getenv("MC33_HIP_DEVICES");
	if (!e || !*e)
		return 0;
	const int have = mc33hip_device_count();
	if (have <= 0)
		return 0;
	int n = 0;
	if (!strcmp(e, "all")) {
		for (; n < have && n < MC33_MAX_DEVICES; n++) dev[n] = n;
		return n;
	}
	while (*e && n < MC33_MAX_DEVICES) {
		char *end = 0;
		const long v = strtol(e, &end, 10);
		if (end == e || v < 0 || v >= have)
			return -1; /* not a list of devices of this machine */
		dev[n++] = (int)v;
		e = end;
		while (*e == ',' || *e == ' ') e++;
	}
	return *e ? -1 : n;
}

static int g_objects; /* MC33 objects alive (the host block cache is trimmed when the last one goes) */
static void cache_trim(size_t keep);
static size_t cache_limit(int *is_set);

/* A new private object for a grid of nx x ny x nz cells at r0 with spacing d - A, Ai: the cell matrices of an inclined grid (nine
 * doubles each, row major), or null: the public sizes, O and D, the matrices MC33_spnC multiplies with or ca / cb, and one more
 * object alive.  free_MC33 is what undoes it.  NULL without memory. */
static mc33_private *new_object(unsigned nx, unsigned ny, unsigned nz, const double *r0, const double *d, const double *A, const double *Ai) {
	mc33_private *p = (mc33_private *)calloc(1, sizeof *p);
	if (!p)
		return 0;
	p->magic = MC33_MAGIC;
	MC33 *M = &p->pub;
	M->nx = nx; M->ny = ny; M->nz = nz;
	for (int j = 0; j != 3; j++) { /* MC:1779-1782 */
		M->O[j] = (MC33_real)r0[j];
		M->D[j] = (MC33_real)d[j];
		p->grd_r0[j] = r0[j]; p->grd_d[j] = d[j];
	}
#ifndef GRD_ORTHOGONAL
	if (A) { /* MC:1763-1770 */
		for (int j = 0; j != 3; j++)
			for (int i = 0; i != 3; i++) {
				M->_A[j][i] = A[3 * j + i] * d[i];
				M->A_[j][i] = Ai[3 * j + i] / d[j];
			}
		p->inclined = 1;
		memcpy(p->grd_A, A, sizeof p->grd_A);
		memcpy(p->grd_Ai, Ai, sizeof p->grd_Ai);
	} else
#else
	(void)A; (void)Ai;
#endif
	if (d[0] != d[1] || d[1] != d[2]) { /* MC:1772-1775 */
		M->ca = (MC33_real)(d[2] / d[0]);
		M->cb = (MC33_real)(d[2] / d[1]);
	}
	__atomic_add_fetch(&g_objects, 1, __ATOMIC_RELAXED);
	return p;
}

MC33 *create_MC33(_GRD *G) {
	if (!G || !G->F)
		return 0;
	const double *A = 0, *Ai = 0;
#ifndef GRD_ORTHOGONAL
	if (G->nonortho) { A = &G->_A[0][0]; Ai = &G->A_[0][0]; }
#endif
	mc33_private *p = new_object(G->N[0], G->N[1], G->N[2], G->r0, G->d, A, Ai);
	if (!p)
		return 0;
	MC33 *M = &p->pub;
	M->F = (const GRD_data_type ***)G->F;
	const char *e = getenv("MC33_HIP_REUPLOAD");
	p->reupload = e && *e && *e != '0';
	p->grid = G;
	int dev[MC33_MAX_DEVICES];
	int n = parse_devices(dev);
	if (G->N[0] < 1 || G->N[1] < 1 || G->N[2] < 1 || n < 0) {
		free_MC33(M);
		return 0;
	}
	if (n == 0) { n = 1; dev[0] = -1; } /* the current device */
	if ((unsigned)n > G->N[2]) n = (int)G->N[2]; /* a slab is at least one cell slice */
	p->nslab = n;
	for (int k = 0; k != n; k++) { /* even split along z (slabs.py: Slab) */
		mc33_slab *s = &p->slab[k];
		s->owner = p;
		s->device = dev[k];
		s->z_begin = (unsigned)((unsigned long long)k * G->N[2] / (unsigned)n);
		s->z_end = (unsigned)((unsigned long long)(k + 1) * G->N[2] / (unsigned)n);
		s->ghost = k ? 1u : 0u;
		s->p_lo = s->z_begin >= s->ghost + 1u ? s->z_begin - s->ghost - 1u : 0u;
		s->p_hi = s->z_end + 1u <= G->N[2] ? s->z_end + 1u : G->N[2];
	}
	if (run_slabs(p, slab_create) != MC33HIP_OK) { /* the 1 / n of G->F of every device goes over its own link */
		free_MC33(M);
		return 0;
	}
	return M;
}

void free_MC33(MC33 *M) {
	mc33_private *p = priv(M);
	if (!p)
		return;
	for (int q = 0; q != p->nslab; q++) {
		mc33_slab *s = &p->slab[q];
		if (!s->ctx)
			continue;
		for (int k = 0; k != 2; k++)
			staging_release(s->ctx, &s->set[k]);
		if (q == 0) { dev_release(s->ctx, &p->dP, &p->capP); dev_release(s->ctx, &p->dL, &p->capL); dev_release(s->ctx, &p->dG, &p->capG); }
		for (int k = 0; q == 0 && k != 3; k++) dev_release(s->ctx, &p->dImg[k], &p->capImg[k]);
		if (q == 0 && p->own_grid) { /* the grid of MC33_create_resampled: through the context while it lives, when nothing reads it any more */
			(void)mc33hip_synchronize(s->ctx);
			(void)mc33hip_device_free(s->ctx, p->own_grid);
			p->own_grid = 0;
		}
		mc33hip_destroy(s->ctx);
	}
	p->magic = 0;
	free(p);
	if (__atomic_sub_fetch(&g_objects, 1, __ATOMIC_RELAXED) == 0)
		cache_trim(cache_limit(0)); /* no extractor left: what free_surface_memory kept beyond the plain limit goes back */
}

/* --- mult_Abf (reference header :186-191, MC33_util_grd.c:86-114) --------------------------------- */
void _multTSA_bf(const double (*A)[3], MC33_real *b, MC33_real *c, int t) {
	if (t) { /* rows of A^T, last first: c may alias b */
		c[2] = A[0][2] * b[0] + A[1][2] * b[1] + A[2][2] * b[2];
		c[1] = A[0][1] * b[0] + A[1][1] * b[1];
		c[0] = A[0][0] * b[0];
	} else {
		c[0] = A[0][0] * b[0] + A[0][1] * b[1] + A[0][2] * b[2];
		c[1] = A[1][1] * b[1] + A[1][2] * b[2];
		c[2] = A[2][2] * b[2];
	}
}

void _multA_bf(const double (*A)[3], MC33_real *b, MC33_real *c, int t) {
	const int r = t ? 3 : 1, s = t ? 1 : 3; /* element (i, j) of the matrix applied = ((const double *)A)[i*s + j*r] */
	const double *a = &A[0][0];
	const double c0 = a[0] * b[0] + a[r] * b[1] + a[2 * r] * b[2];
	const double c1 = a[s] * b[0] + a[s + r] * b[1] + a[s + 2 * r] * b[2];
	c[2] = a[2 * s] * b[0] + a[2 * s + r] * b[1] + a[2 * s + 2 * r] * b[2];
	c[0] = c0;
	c[1] = c1;
}

void (*mult_Abf)(const double (*)[3], MC33_real *, MC33_real *, int) = _multA_bf;

static int refresh_grid(mc33_private *p) {
	if (p->inclined) { /* the reference calls through mult_Abf for every vertex (MC:608, 612) */
		if (mult_Abf != _multA_bf && mult_Abf != _multTSA_bf)
			return MC33HIP_EINVAL; /* a caller-supplied function cannot run on the GPU */
		for (int k = 0; k != p->nslab; k++)
			if (mc33hip_set_inclined(p->slab[k].ctx, p->grd_A, p->grd_Ai, mult_Abf == _multTSA_bf) != MC33HIP_OK)
				return MC33HIP_EINVAL;
	}
	if (!p->grid || (!p->reupload && !p->grid_dirty)) /* (no host grid: the object of MC33_create_resampled) */
		return 0;
	p->grid_dirty = 0;
	return run_slabs(p, slab_upload);
}

/* Extension (not in the reference, which reads G->F anew on every call, MC:1792, 1832-1868): tells the extractor that
 * samples of the grid it was created from have been rewritten.  The next size_of_isosurface / calculate_isosurface(s)
 * uploads G->F again first.  The _GRD and its rows must still be alive then, as for the reference's own M->F. */
void MC33_grid_changed(MC33 *M) {
	mc33_private *p = priv(M);
	if (p && p->grid)
		p->grid_dirty = 1;
}

/* --- extension: colours from a property grid ------------------------------------------------------------------------------
 * A slab's own vertices lie in its cell slices [z_begin, z_end) - up to rounding: a vertex on a grid plane inverts to a hair
 * below or above it - so the slab holds property planes [max(z_begin, 1) - 1, min(z_end + 1, nz)]. */
static void *slab_property(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	const _GRD *P = s->owner->prop;
	const unsigned lo = (s->z_begin > 1u ? s->z_begin : 1u) - 1u, hi = s->z_end + 1u < P->N[2] ? s->z_end + 1u : P->N[2];
	s->rc = mc33hip_property_upload_rows(s->ctx, (const void *const *const *)(P->F + lo), lo, hi - lo + 1u);
	return 0;
}

static int coloured(const mc33_private *p) { return (p->prop != 0 || p->color_source != MC33_COLOR_PROPERTY) && p->has_map; }

int MC33_set_property_grid(MC33 *M, _GRD *P) {
	mc33_private *p = priv(M);
	if (!p || !mc33hip_property_upload_rows || !mc33hip_property_drop || !mc33hip_color_vertices || !mc33hip_download_enqueue)
		return -1;
	if (!P) {
		for (int k = 0; k != p->nslab; k++) (void)mc33hip_property_drop(p->slab[k].ctx);
		p->prop = 0;
		return 0;
	}
	if (p->inclined || !P->F || P->N[0] != M->nx || P->N[1] != M->ny || P->N[2] != M->nz)
		return -1;
#ifndef GRD_ORTHOGONAL
	if (P->nonortho)
		return -1;
#endif
	p->prop = P;
	if (run_slabs(p, slab_property) != MC33HIP_OK) { /* a slab without its planes: no colours from any */
		for (int q = 0; q != p->nslab; q++) (void)mc33hip_property_drop(p->slab[q].ctx);
		p->prop = 0;
		return -1;
	}
	return 0;
}

int MC33_set_color_map(MC33 *M, const int *palette, unsigned n, double lo, double hi) {
	mc33_private *p = priv(M);
	if (!p)
		return -1;
	if (!palette) {
		p->has_map = 0;
		return 0;
	}
	if (n < 2u || n > 256u || !(lo < hi))
		return -1;
	memcpy(p->map, palette, n * sizeof(int));
	p->map_n = n; p->map_lo = lo; p->map_hi = hi;
	p->has_map = 1;
	return 0;
}

int MC33_set_color_source(MC33 *M, int source) {
	mc33_private *p = priv(M);
	if (!p || source < MC33_COLOR_PROPERTY || source > MC33_COLOR_K2)
		return -1;
	if (source != MC33_COLOR_PROPERTY &&
	    (!mc33hip_curvature_vertices || !mc33hip_color_values || p->inclined || p->nslab != 1 || M->nx < 2u || M->ny < 2u || M->nz < 2u))
		return -1;
	p->color_source = source;
	return 0;
}

/* the colour kernel over the nV vertices in g->dV, behind whatever wrote them on the context's stream (enqueues only; with a
 * curvature for its source the curvature pass has been waited for, the colour kernel is enqueued) */
static int enqueue_colors(mc33_slab *s, struct staging *g, unsigned long long nV) {
	mc33_private *p = s->owner;
	if (dev_room(s->ctx, &g->dC, &g->capC, nV, sizeof(int))) return MC33HIP_ENOMEM;
	if (p->color_source != MC33_COLOR_PROPERTY) { /* the chosen curvature into p->dP (one slab: MC33_set_color_source), the map over it */
		mc33hip_curvature a;
		if (dev_room(s->ctx, &p->dP, &p->capP, nV, sizeof(float))) return MC33HIP_ENOMEM;
		memset(&a, 0, sizeof a);
		a.dV = g->dV; a.nV = nV; a.sign = MC33_NORMAL_NEG ? -1 : 1;
		*(p->color_source == MC33_COLOR_MEAN ? &a.oMean : p->color_source == MC33_COLOR_GAUSS ? &a.oGauss : p->color_source == MC33_COLOR_K1 ? &a.oK1 : &a.oK2) = (float *)p->dP;
		const int rc = mc33hip_curvature_vertices(s->ctx, &a);
		return rc != MC33HIP_OK ? rc : mc33hip_color_values(s->ctx, (const float *)p->dP, nV, p->map, p->map_n, p->map_lo, p->map_hi, p->nan_color, (int *)g->dC);
	}
	return mc33hip_color_vertices(s->ctx, g->dV, nV, p->map, p->map_n, p->map_lo, p->map_hi, p->nan_color, (int *)g->dC);
}

/* count pass of one slab (blocks until its counters are on the host) */
static void *slab_count(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	mc33hip_range r;
	r.z_begin = s->z_begin; r.z_end = s->z_end; r.ghost_below = s->ghost; r.id_base = 0;
	memset(&s->cnt, 0, sizeof s->cnt);
	s->rc = mc33hip_count(s->ctx, (double)s->iso, &r, &s->cnt);
	return 0;
}

/* Counts of every slab, side by side; the totals in *tot.  Vertex ids and triangle slots of slab k begin at the sums over the
 * slabs below it (the reference numbers vertices in sweep order, so z-slabs concatenate). */
static int count_slabs(mc33_private *p, MC33_real iso, mc33hip_counts *tot) {
	memset(tot, 0, sizeof *tot);
	int rc = refresh_grid(p);
	if (rc != MC33HIP_OK)
		return rc;
	for (int k = 0; k != p->nslab; k++) p->slab[k].iso = iso;
	if ((rc = run_slabs(p, slab_count)) != MC33HIP_OK)
		return rc;
	for (int k = 0; k != p->nslab; k++) {
		tot->nV += p->slab[k].cnt.nV; tot->nT += p->slab[k].cnt.nT; tot->active_cells += p->slab[k].cnt.active_cells;
	}
	return (tot->nV > 0xFFFFFFFFull || tot->nT > 0xFFFFFFFFull) ? MC33HIP_EOVERFLOW : MC33HIP_OK;
}

unsigned long long size_of_isosurface(MC33 *M, MC33_real iso, unsigned int *nV, unsigned int *nT) {
	mc33_private *p = priv(M);
	mc33hip_counts cnt;
	memset(&cnt, 0, sizeof cnt);
	if (p) {
		M->iso = iso;
		if (count_slabs(p, iso, &cnt) != MC33HIP_OK)
			memset(&cnt, 0, sizeof cnt);
	}
	if (nV) *nV = (unsigned int)cnt.nV;
	if (nT) *nT = (unsigned int)cnt.nT;
	/* MC:1939 */
	return cnt.nV * (6 * sizeof(MC33_real) + sizeof(int)) + cnt.nT * (3 * sizeof(int)) + sizeof(surface);
}

/* room for nV vertices and nT triangles in staging set g.  V and N grow together, under the one capacity capV: both go before
 * either is made anew, and capV stands only when both are there */
static int staging_room(mc33_slab *s, struct staging *g, unsigned long long nV, unsigned long long nT) {
	if (g->capV < nV) {
		unsigned long long capN = 0;
		dev_release(s->ctx, &g->dV, &g->capV); dev_release(s->ctx, &g->dN, &capN);
		if (dev_room(s->ctx, &g->dV, &g->capV, nV, 3 * sizeof(MC33_real))) return -1;
		if (dev_room(s->ctx, &g->dN, &capN, nV, 12)) { g->capV = 0; return -1; }
	}
	return g->capT < nT ? dev_room(s->ctx, &g->dT, &g->capT, nT, 12) : 0;
}

/* count, grow, emit (one slab: the whole grid): V, N, T of the surface of `iso` into staging set g (device memory), its sizes
 * into *cnt */
static int extract_geometry(mc33_private *p, struct staging *g, MC33_real iso, mc33hip_counts *cnt) {
	mc33_slab *s = &p->slab[0];
	mc33hip_range r;
	r.z_begin = 0; r.z_end = p->pub.nz; r.ghost_below = 0; r.id_base = 0;
	memset(cnt, 0, sizeof *cnt);
	int rc = refresh_grid(p);
	if (rc != MC33HIP_OK)
		return rc;
	/* one pass with the staging buffers of an earlier call; if they are too small the counts come back
	 * anyway, the buffers grow and only the emit pass is repeated */
	rc = mc33hip_extract(s->ctx, iso, &r, g->dV, g->dN, g->dT, g->capV, g->capT, cnt);
	if (rc == MC33HIP_ECAPACITY) {
		rc = staging_room(s, g, cnt->nV, cnt->nT) ? MC33HIP_ENOMEM : mc33hip_emit(s->ctx, g->dV, g->dN, g->dT, g->capV, g->capT);
		/* mc33hip_emit only enqueues: the set must be complete before anybody reads it - the helper thread of
		 * calculate_isosurfaces copies on a stream of its own, which is not ordered after this one */
		if (rc == MC33HIP_OK)
			rc = mc33hip_synchronize(s->ctx);
	}
	return rc;
}

/* extract_geometry, and behind it the colours of the vertices into the set where they come from the device (enqueued only): the
 * grey for a NaN is the DefaultColorMC of this moment */
static int extract_coloured(mc33_private *p, struct staging *g, MC33_real iso, mc33hip_counts *cnt) {
	int rc = extract_geometry(p, g, iso, cnt);
	if (rc == MC33HIP_OK && coloured(p) && cnt->nV) {
		p->nan_color = DefaultColorMC;
		rc = enqueue_colors(&p->slab[0], g, cnt->nV);
	}
	return rc;
}

/* GPU part of one surface of calculate_isosurfaces: extract_coloured, the colours complete like the set's other arrays */
static int extract_to_staging(mc33_private *p, struct staging *g, MC33_real iso, mc33hip_counts *cnt) {
	int rc = extract_coloured(p, g, iso, cnt);
	if (rc == MC33HIP_OK && coloured(p) && cnt->nV)
		rc = mc33hip_synchronize(p->slab[0].ctx);
	return rc;
}

/* One array of a caller-owned surface: plain free() releases it (MC:84-92).  Large ones start on a 2 MiB boundary and
 * ask for transparent huge pages: a 1024^3 surface is 200 MB, and touching it for the first time in 4 KiB pages (the
 * copy from the GPU, the colour fill, the munmap in free) cost more than the extraction itself - measured on the GPU box
 * (tools/d2h_probe.hip, profiles/r05_d2h_probe.txt): a 94 MB array arrives in 1.76 ms (56 GB/s, the rate of the link - pinning
 * the block with hipHostRegister first gains nothing) when its pages are mapped, in 4 - 5 ms when they are fresh, and giving
 * them back to the kernel costs another 4 - 6 ms; the 15 MB colour fill 0.16 against 3.0 ms.
 *
 * So free_surface_memory keeps large blocks for the next surface instead of releasing them.  How much it keeps: as much as the
 * surface it is releasing holds (an unmodified viewer loop - calculate_isosurface, draw, free_surface_memory, next isovalue:
 * reference GLUT_example/TestMC33_glut.c:421-458 - then always finds the blocks of the surface before), and at least 64 MB.
 * Blocks of earlier, larger surfaces that do not fit under that bound any more are freed, and when the last MC33 object is
 * destroyed everything beyond 64 MB goes back.  MC33_HOST_CACHE_MB in the environment replaces the rule by a fixed bound
 * (0 = keep nothing).
 *
 * Only blocks this library allocated are ever looked at: every large block handed out is entered in a small table
 * (address, size); free_surface_memory looks the pointer up there, and an address it does not know is simply passed to
 * free().  A table hit is double-checked with the allocator (a caller may have freed our block and got the same
 * address back for a smaller one of its own): it counts as ours only if the allocator still holds at least the
 * recorded size there.  The blocks are ordinary malloc blocks at all times. */
#define HUGE_PAGE ((size_t)2 << 20)
#define CACHE_MIN_BLOCK (2 * HUGE_PAGE)
#define CACHE_SLOTS 16
#define LIVE_SLOTS 256
#define CACHE_DEFAULT ((size_t)64 << 20)
static struct {
	void *p;
	size_t cap;
	unsigned long long age; /* (cache only) when it was put back: the oldest goes first */
} g_cache[CACHE_SLOTS], g_live[LIVE_SLOTS]; /* kept for reuse / handed out and still with the caller */
static size_t g_cache_bytes;
static unsigned long long g_cache_clock;
static pthread_mutex_t g_cache_lock = PTHREAD_MUTEX_INITIALIZER;

/* the plain bound: MC33_HOST_CACHE_MB, 64 MB when it is not set (*is_set says which) */
static size_t cache_limit(int *is_set) {
	const char *e = getenv("MC33_HOST_CACHE_MB");
	if (is_set) *is_set = e && *e;
	return e && *e ? (size_t)strtoull(e, 0, 10) << 20 : CACHE_DEFAULT;
}

/* (lock held) frees kept blocks, oldest first, until at most `keep` bytes are left */
static void cache_trim_locked(size_t keep) {
	while (g_cache_bytes > keep) {
		int old = -1;
		for (int k = 0; k != CACHE_SLOTS; k++)
			if (g_cache[k].p && (old < 0 || g_cache[k].age < g_cache[old].age))
				old = k;
		if (old < 0)
			break;
		free(g_cache[old].p);
		g_cache_bytes -= g_cache[old].cap;
		g_cache[old].p = 0;
	}
}
static void cache_trim(size_t keep) {
	pthread_mutex_lock(&g_cache_lock);
	cache_trim_locked(keep);
	pthread_mutex_unlock(&g_cache_lock);
}

/* (lock held) remember a large block that goes to the caller; when the table is full the block is simply not known
 * later and will be freed like a foreign one */
static void live_add(void *p, size_t cap) {
	for (int k = 0; k != LIVE_SLOTS; k++)
		if (!g_live[k].p || g_live[k].p == p) {
			g_live[k].p = p;
			g_live[k].cap = cap;
			return;
		}
}

/* Fresh large blocks - pages the process has never touched - are populated by several threads at once before the copies from the
 * GPU are started (populate_fresh).  The reference's own viewers KEEP every surface they make (GLUT_example/TestMC33_glut.c:421-458
 * appends to a list), so for them every call lands in fresh pages: populated by the copy itself, one fault after the other, a
 * 1024^3 surface costs 8 ms of page faults; profiles/r05_capi_walls.txt. */
struct fresh_block { char *p; size_t n; };
static __thread struct fresh_block t_fresh[4];
static __thread int t_nfresh;

/* a block of at least `bytes` bytes; *cap = what it can really hold */
static void *surface_block(size_t bytes, size_t *cap) {
	void *p = 0;
	if (bytes >= CACHE_MIN_BLOCK) {
		int best = -1;
		pthread_mutex_lock(&g_cache_lock);
		for (int k = 0; k != CACHE_SLOTS; k++) /* best fit, never more than twice the need */
			if (g_cache[k].p && g_cache[k].cap >= bytes && g_cache[k].cap <= 2 * bytes && (best < 0 || g_cache[k].cap < g_cache[best].cap))
				best = k;
		if (best >= 0) {
			p = g_cache[best].p;
			*cap = g_cache[best].cap;
			g_cache[best].p = 0;
			g_cache_bytes -= *cap;
			live_add(p, *cap);
		}
		pthread_mutex_unlock(&g_cache_lock);
		if (p)
			return p;
		const size_t rounded = (bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1);
		if (posix_memalign(&p, HUGE_PAGE, rounded) == 0) {
			(void)madvise(p, rounded, MADV_HUGEPAGE);
			*cap = rounded;
			if (t_nfresh < 4) { t_fresh[t_nfresh].p = (char *)p; t_fresh[t_nfresh].n = bytes; t_nfresh++; }
			pthread_mutex_lock(&g_cache_lock);
			live_add(p, rounded);
			pthread_mutex_unlock(&g_cache_lock);
			return p;
		}
	}
	p = malloc(bytes ? bytes : 1);
	*cap = bytes;
	return p;
}

/* (lock held) is p a large block of ours that the allocator still holds?  Its capacity, and the table entry is given up */
static size_t live_take(void *p) {
	if (!p)
		return 0;
	for (int k = 0; k != LIVE_SLOTS; k++)
		if (g_live[k].p == p) {
			const size_t cap = g_live[k].cap;
			g_live[k].p = 0;
			return malloc_usable_size(p) >= cap ? cap : 0;
		}
	return 0;
}

/* The counterpart used by free_surface_memory and adjustvectorlenght_s: the n arrays of ONE surface go back together.  Those
 * that are large blocks of ours are kept for the next surface as far as the bound allows - the bound being what these very
 * blocks hold, or 64 MB if that is more (MC33_HOST_CACHE_MB, when set, instead) - the others are freed. */
static void surface_blocks_release(void **blk, int n) {
	size_t cap[8], mine = 0;
	int is_set = 0;
	size_t limit = cache_limit(&is_set);
	pthread_mutex_lock(&g_cache_lock);
	for (int k = 0; k != n; k++) {
		cap[k] = live_take(blk[k]);
		mine += cap[k];
	}
	if (!is_set && mine > limit)
		limit = mine;
	cache_trim_locked(limit > mine ? limit - mine : 0); /* older blocks make room for these */
	for (int k = 0; k != n; k++) {
		if (!cap[k] || g_cache_bytes + cap[k] > limit)
			continue;
		for (int q = 0; q != CACHE_SLOTS; q++)
			if (!g_cache[q].p) {
				g_cache[q].p = blk[k];
				g_cache[q].cap = cap[k];
				g_cache[q].age = ++g_cache_clock;
				g_cache_bytes += cap[k];
				blk[k] = 0;
				break;
			}
	}
	pthread_mutex_unlock(&g_cache_lock);
	for (int k = 0; k != n; k++)
		free(blk[k]);
}
static void surface_block_release(void *p) { surface_blocks_release(&p, 1); }

/* the four arrays of a surface with nV vertices and nT triangles (caller-owned malloc blocks, MC:84-92); 0 when memory is short */
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23 /* Linux 5.14 */
#endif
static void *populate_thread(void *arg) {
	struct fresh_block *b = (struct fresh_block *)arg;
	if (madvise(b->p, b->n, MADV_POPULATE_WRITE) != 0) /* (older kernels: touch every page - nothing has been written into the block yet) */
		for (size_t off = 0; off < b->n; off += 4096) ((volatile char *)b->p)[off] = 0;
	return 0;
}
/* the fresh blocks surface_alloc has just made (this thread's list), in pieces of at most 32 MB, a thread per piece (16 at most) */
static void populate_fresh(void) {
	struct fresh_block piece[16];
	pthread_t th[16];
	int n = 0;
	for (int k = 0; k != t_nfresh; k++)
		for (size_t off = 0; off < t_fresh[k].n && n != 16; off += (size_t)32 << 20) {
			piece[n].p = t_fresh[k].p + off;
			piece[n].n = t_fresh[k].n - off < ((size_t)32 << 20) ? t_fresh[k].n - off : (size_t)32 << 20;
			n++;
		}
	t_nfresh = 0;
	int started[16];
	for (int k = 1; k < n; k++) started[k] = pthread_create(&th[k], 0, populate_thread, &piece[k]) == 0;
	if (n) populate_thread(&piece[0]);
	for (int k = 1; k < n; k++) {
		if (started[k]) pthread_join(th[k], 0);
		else populate_thread(&piece[k]);
	}
}

static surface *surface_alloc(size_t nV, size_t nT, MC33_real iso) {
	surface *S = (surface *)malloc(sizeof(surface));
	if (!S)
		return 0;
	t_nfresh = 0;
	memset(S, 0, sizeof(surface)); /* (an empty surface is exactly this, MC:1880-1883) */
	if (!nV)
		return S;
	size_t capV = 0, capN = 0, capT = 0, capC = 0;
	S->V = (MC33_real(*)[3])surface_block(nV * 3 * sizeof(MC33_real), &capV);
	S->N = (float(*)[3])surface_block(nV * 3 * sizeof(float), &capN);
	S->T = (unsigned int(*)[3])surface_block((nT ? nT : 1) * 3 * sizeof(int), &capT);
	const int fresh_vnt = t_nfresh; /* (the colour block is populated by whoever fills it) */
	S->color = (int *)surface_block(nV * sizeof(int), &capC);
	t_nfresh = fresh_vnt;
	if (!S->V || !S->N || !S->T || !S->color) {
		t_nfresh = 0;
		free_surface_memory(S);
		return 0;
	}
	S->nV = (unsigned int)nV; S->nT = (unsigned int)nT;
	/* capacities in elements, as the reference keeps them (MC:94-127 shrinks arrays whose cap exceeds the count) */
	size_t cv = capV / (3 * sizeof(MC33_real)), ct = capT / (3 * sizeof(int));
	if (capN / (3 * sizeof(float)) < cv) cv = capN / (3 * sizeof(float));
	if (capC / sizeof(int) < cv) cv = capC / sizeof(int);
	S->capv = (unsigned int)(cv > 0xFFFFFFFFu ? 0xFFFFFFFFu : cv);
	S->capt = (unsigned int)(ct > 0xFFFFFFFFu ? 0xFFFFFFFFu : ct);
	S->iso = iso;
	return S;
}

static void fill_color(surface *S) { /* MC:1875-1877 */
	const int col = DefaultColorMC;
	int *c = S->color;
	for (size_t k = 0, n = S->nV; k != n; k++)
		c[k] = col;
}
static void *fill_color_thread(void *arg) {
	fill_color((surface *)arg);
	return 0;
}

/* host part of calculate_isosurfaces: a caller-owned `surface` filled from staging set g.
 * concurrent: copy on the side stream, beside whatever the context is computing */
static surface *surface_from_staging(mc33_private *p, const struct staging *g, const mc33hip_counts *cnt, MC33_real iso, int concurrent) {
	surface *S = surface_alloc((size_t)cnt->nV, (size_t)cnt->nT, iso);
	if (!S || !S->nV)
		return S;
	populate_fresh();
	const int col = coloured(p); /* (extract_to_staging has left the colours in the set then) */
	void *const dst[4] = {S->V, S->N, S->T, S->color};
	const void *const src[4] = {g->dV, g->dN, g->dT, g->dC};
	const size_t bytes[4] = {(size_t)S->nV * 3 * sizeof(MC33_real), (size_t)S->nV * 12, (size_t)S->nT * 12, (size_t)S->nV * sizeof(int)};
	if (mc33hip_download_many(p->slab[0].ctx, col ? 4 : 3, dst, src, bytes, concurrent) != MC33HIP_OK) {
		free_surface_memory(S);
		return 0;
	}
	if (!col)
		fill_color(S);
	return S;
}

/* emit of one slab at its global base, its arrays copied straight to their place in the caller's blocks */
static void *slab_emit(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	struct staging *g = &s->set[0];
	surface *S = s->out;
	s->rc = MC33HIP_OK;
	if (!s->cnt.nV && !s->cnt.nT)
		return 0;
	if (staging_room(s, g, s->cnt.nV, s->cnt.nT)) { s->rc = MC33HIP_ENOMEM; return 0; }
	if ((s->rc = mc33hip_set_id_base(s->ctx, (unsigned int)s->vbase)) != MC33HIP_OK) return 0;
	s->rc = mc33hip_emit_download(s->ctx, g->dV, g->dN, g->dT, g->capV, g->capT, S->V + s->vbase, S->N + s->vbase, S->T + s->tbase);
	if (s->rc == MC33HIP_OK && coloured(s->owner) && s->cnt.nV) { /* the colour kernel behind the vertex pass, its array behind the other copies */
		s->rc = enqueue_colors(s, g, s->cnt.nV);
		if (s->rc == MC33HIP_OK)
			s->rc = mc33hip_download_enqueue(s->ctx, S->color + s->vbase, g->dC, (size_t)s->cnt.nV * sizeof(int));
	}
	const int w = mc33hip_download_wait(s->ctx); /* (also after a failure: nothing may still be writing into the blocks when they are released) */
	if (s->rc == MC33HIP_OK) s->rc = w;
	return 0;
}

/* mirror of the copy MC:1873 makes into the MC33 object's public prefix; an empty surface leaves the prefix as it is */
static surface *publish(MC33 *M, surface *S) {
	if (S->nV) {
		M->T = S->T; M->V = S->V; M->N = S->N; M->color = S->color;
		M->nT = S->nT; M->capt = S->capt; M->capv = S->capv;
	}
	return S;
}

/* MC:1816-1889.  Count on every slab (one, unless MC33_HIP_DEVICES names several devices) -> the sizes of the surface and where
 * each slab's part begins -> the caller's arrays (recycled blocks, see above) -> every slab emits its vertices and triangles at
 * its global base and copies them straight to their place in those arrays, each array as soon as the passes that write it are
 * through, over its own device's link: no device-to-device exchange, nothing to concatenate -> the colours are filled in by a
 * helper thread while the copies run. */
static double now_ms(void) {
	struct timespec t;
	clock_gettime(CLOCK_MONOTONIC, &t);
	return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

surface *calculate_isosurface(MC33 *M, MC33_real iso) {
	mc33_private *p = priv(M);
	if (!p)
		return 0;
	M->nT = M->nV = 0;
	M->memoryfault = 0;
	M->iso = iso;
	mc33hip_counts tot;
	static int trace = -1; /* MC33_CAPI_TRACE=1: where the wall time of a call goes (stderr) */
	if (trace < 0) trace = getenv("MC33_CAPI_TRACE") != 0;
	double t[6] = {0, 0, 0, 0, 0, 0};
	if (trace) t[0] = now_ms();
	const int crc = count_slabs(p, iso, &tot);
	if (trace) t[1] = now_ms();
	surface *S = crc == MC33HIP_OK ? surface_alloc((size_t)tot.nV, (size_t)tot.nT, iso) : 0;
	if (trace) t[2] = now_ms();
	if (S && S->nV) {
		unsigned long long vb = 0, tb = 0;
		for (int k = 0; k != p->nslab; k++) {
			mc33_slab *s = &p->slab[k];
			s->out = S; s->vbase = vb; s->tbase = tb;
			vb += s->cnt.nV; tb += s->cnt.nT;
		}
		pthread_t ct;
		const int col = coloured(p); /* the colours come from the device with the other arrays: nothing to fill */
		p->nan_color = DefaultColorMC;
		const int helper = !col && S->nV >= 65536u && pthread_create(&ct, 0, fill_color_thread, S) == 0; /* 16 MB at 1024^3: 0.8 ms beside 3.4 ms of copies */
		populate_fresh(); /* (blocks that did not come from the cache: their pages, before the copies need them) */
		if (trace) t[3] = now_ms();
		const int ok = run_slabs(p, slab_emit) == MC33HIP_OK;
		if (trace) t[4] = now_ms();
		if (helper) pthread_join(ct, 0);
		else if (!col) fill_color(S);
		if (trace) {
			t[5] = now_ms();
			fprintf(stderr, "[mc33 capi] count %.3f  blocks %.3f  helper + fresh pages %.3f  emit + copies %.3f  colours joined %.3f  total %.3f ms\n", t[1] - t[0], t[2] - t[1],
			        t[3] - t[2], t[4] - t[3], t[5] - t[4], t[5] - t[0]);
		}
		if (!ok) {
			free_surface_memory(S);
			S = 0;
		}
	}
	if (!S) {
		M->memoryfault = 1;
		return 0;
	}
	return publish(M, S);
}

/* --- extension: several isovalues of the resident grid ---------------------------------------------------- */
/* the sweeps of the next m (up to 8) isovalues in one or two passes over the grid */
static void sweep_ahead(mc33_private *p, const MC33_real *iso, unsigned m) {
	double many[8];
	mc33hip_range r;
	r.z_begin = 0; r.z_end = p->pub.nz; r.ghost_below = 0; r.id_base = 0;
	for (unsigned q = 0; q != m; q++) many[q] = iso[q];
	if (!p->reupload) /* (the re-upload of every call would drop the sweeps made ahead) */
		(void)mc33hip_sweep_many(p->slab[0].ctx, many, (int)m, &r); /* (on failure the single calls sweep for themselves) */
}

struct download_job {
	mc33_private *p;
	const struct staging *g;
	mc33hip_counts cnt;
	MC33_real iso;
	surface *S;
};

static void *download_thread(void *arg) {
	struct download_job *j = (struct download_job *)arg;
	j->S = surface_from_staging(j->p, j->g, &j->cnt, j->iso, 1);
	return 0;
}

unsigned int calculate_isosurfaces(MC33 *M, const MC33_real *iso, unsigned int n, surface **out) {
	mc33_private *p = priv(M);
	unsigned int done = 0;
	if (!out)
		return 0;
	for (unsigned int k = 0; k != n; k++)
		out[k] = 0;
	if (!p || !iso)
		return 0;
	M->memoryfault = 0;
	if (p->nslab > 1) { /* several devices: every surface by itself (each call already runs its slabs side by side) */
		for (unsigned int k = 0; k != n; k++)
			if ((out[k] = calculate_isosurface(M, iso[k])) != 0)
				done++;
		M->memoryfault = done != n;
		return done;
	}
	if (refresh_grid(p) != MC33HIP_OK)
		return 0;
	struct download_job job;
	pthread_t th;
	int running = 0;
	unsigned int running_k = 0;
	for (unsigned int k = 0; k != n; k++) {
		if (k % 8 == 0 && n - k > 1)
			sweep_ahead(p, iso + k, n - k < 8 ? n - k : 8);
		/* surface k is computed into set k&1 while the helper thread copies surface k-1 out of the other set */
		struct staging *g = &p->slab[0].set[k & 1];
		mc33hip_counts cnt;
		M->iso = iso[k];
		const int rc = extract_to_staging(p, g, iso[k], &cnt);
		if (running) {
			pthread_join(th, 0);
			running = 0;
			out[running_k] = job.S;
		}
		if (rc != MC33HIP_OK)
			continue;
		job.p = p; job.g = g; job.cnt = cnt; job.iso = iso[k]; job.S = 0;
		if (pthread_create(&th, 0, download_thread, &job) == 0) {
			running = 1;
			running_k = k;
		} else
			out[k] = surface_from_staging(p, g, &cnt, iso[k], 0);
	}
	if (running) {
		pthread_join(th, 0);
		out[running_k] = job.S;
	}
	for (unsigned int k = 0; k != n; k++) {
		if (out[k]) done++;
		else M->memoryfault = 1;
	}
	return done;
}

/* --- the extensions that work on an extracted surface: what they share -----------------------------------------------------------
 * The gate of every one of them: M's private object when it is live and on one slab and `have` - the caller's own "the device
 * layer has these weak entry points" - holds; otherwise null, and the caller refuses without having touched M or the device. */
static mc33_private *one_slab(MC33 *M, int have) {
	mc33_private *p = priv(M);
	return p && p->nslab == 1 && have ? p : 0;
}
#define MEASURE_ENTRIES (mc33hip_measure_surface && mc33hip_label_components && mc33hip_measure_components && mc33hip_sample_property)
#define TOPOLOGY_ENTRIES (mc33hip_surface_topology && mc33hip_component_topology && mc33hip_label_components)

/* The frame of a call that returns a derived surface, once its arguments have passed: the public counts reset as calculate_isosurface
 * resets them, the part's worker, then memoryfault for a NULL or the public prefix for a surface. */
typedef surface *derived_worker(mc33_private *p, MC33_real iso, const void *arg);
static surface *derived_call(mc33_private *p, MC33_real iso, derived_worker *worker, const void *arg) {
	MC33 *M = &p->pub;
	M->nT = M->nV = 0;
	M->memoryfault = 0;
	M->iso = iso;
	surface *S = worker(p, iso, arg);
	if (!S) {
		M->memoryfault = 1;
		return 0;
	}
	return publish(M, S);
}

/* A mesh pass that writes a new V, N, T - `call`, whose argument struct `a` names its outputs as the other two do - into staging
 * set h: first with the set as it stands, and when that is refused for room, once more with the set grown to the sizes that came
 * back (MC33HIP_ENOMEM when it cannot grow).  Where an attribute rides along the colour array grows too, and the vertex capacity
 * is the smaller of capV and capC.  (oAttr[0] is set for every pass; the device layer reads n_attr of them.) */
#define INTO_STAGING(rc, call, s, h, a) \
	do { \
		(rc) = MC33HIP_ECAPACITY; \
		for (int attempt = 0; attempt != 2 && (rc) == MC33HIP_ECAPACITY; attempt++) { \
			if (attempt && (staging_room(s, h, (a).nV_out, (a).nT_out) || ((a).n_attr && dev_room((s)->ctx, &(h)->dC, &(h)->capC, (a).nV_out, sizeof(int))))) { \
				(rc) = MC33HIP_ENOMEM; \
				break; \
			} \
			(a).oV = (h)->dV; (a).oN = (h)->dN; (a).oT = (h)->dT; (a).oAttr[0] = (h)->dC; \
			(a).capV = (a).n_attr && (h)->capC < (h)->capV ? (h)->capC : (h)->capV; \
			(a).capT = (h)->capT; \
			(rc) = call((s)->ctx, &(a)); \
		} \
	} while (0)

/* nV vertices and nT triangles of staging set g into a caller-owned surface */
static surface *surface_of_rows(mc33_private *p, const struct staging *g, unsigned long long nV, unsigned long long nT, MC33_real iso) {
	mc33hip_counts out;
	memset(&out, 0, sizeof out);
	out.nV = nV; out.nT = nT;
	return surface_from_staging(p, g, &out, iso, 0);
}

/* The surface of `iso` into staging set 0 - with its colours, when `colours` - and the component labels of its vertices into p->dL:
 * the sizes in *cnt, the components in *nc, the vertices no triangle names in *nu.  0, or -1. */
static int extract_labelled(mc33_private *p, MC33_real iso, int colours, mc33hip_counts *cnt, unsigned long long *nc, unsigned long long *nu) {
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	*nc = *nu = 0;
	if ((colours ? extract_coloured(p, g, iso, cnt) : extract_geometry(p, g, iso, cnt)) != MC33HIP_OK)
		return -1;
	if (dev_room(s->ctx, &p->dL, &p->capL, cnt->nV, sizeof(unsigned)))
		return -1;
	return mc33hip_label_components(s->ctx, g->dT, cnt->nT, cnt->nV, (unsigned *)p->dL, nc, nu) == MC33HIP_OK ? 0 : -1;
}

/* ... for a call that fills a table of `capacity` rows: the counts reported where asked for.  Positive: the rows are to be made.
 * Zero or negative: the call is over and returns this (0: no component, -1: failed, -2: the table is too small). */
static int labelled_for_table(mc33_private *p, MC33_real iso, unsigned capacity, unsigned *components, unsigned *unreferenced, mc33hip_counts *cnt,
                              unsigned long long *nc) {
	unsigned long long nu;
	p->pub.iso = iso;
	if (extract_labelled(p, iso, 0, cnt, nc, &nu))
		return -1;
	if (components) *components = (unsigned)*nc;
	if (unreferenced) *unreferenced = (unsigned)nu;
	if (capacity < *nc)
		return -2;
	return *nc != 0;
}

/* --- extension: measures of an isosurface, taken on the device ----------------------------------------------------------------
 * The surface goes into staging set 0 - count, grow, emit, without the colour pass - and is measured there. */
static int measure_one(mc33_private *p, MC33_real iso, mc33_measure *out) {
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	mc33hip_measures m;
	memset(out, 0, sizeof *out);
	p->pub.iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
		return -1;
	const float *dP = 0;
	if (p->prop) { /* the property at the vertices first, into a float array of its own */
		if (dev_room(s->ctx, &p->dP, &p->capP, cnt.nV, sizeof(float)) || mc33hip_sample_property(s->ctx, g->dV, cnt.nV, (float *)p->dP) != MC33HIP_OK)
			return -1;
		dP = (const float *)p->dP;
	}
	if (mc33hip_measure_surface(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, dP, &m) != MC33HIP_OK)
		return -1;
	out->nV = (unsigned)m.nV; out->nT = (unsigned)m.nT;
	out->area = m.area; out->volume = m.volume;
	for (int a = 0; a != 3; a++) {
		out->moment[a] = m.moment[a]; out->origin[a] = m.origin[a];
		out->bbox_min[a] = m.bbox_min[a]; out->bbox_max[a] = m.bbox_max[a];
	}
	out->property_integral = m.property_integral;
	out->has_property = m.has_property;
	return 0;
}

/* --- extension: curvature of an isosurface, taken on the device ------------------------------------------------------------------
 * The surface goes into staging set 0 like measure_one's; mean and Gaussian curvature at its vertices into p->dP and p->dG, and
 * each through mc33hip_measure_surface as its dP. */
int MC33_isosurface_curvature(MC33 *M, MC33_real iso, mc33_curvature *out) {
	mc33_private *p = one_slab(M, mc33hip_curvature_vertices && mc33hip_measure_surface);
	if (!p || !out || p->inclined || M->nx < 2u || M->ny < 2u || M->nz < 2u)
		return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	mc33hip_curvature a;
	mc33hip_measures m[2];
	memset(out, 0, sizeof *out);
	p->pub.iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
		return -1;
	if (dev_room(s->ctx, &p->dP, &p->capP, cnt.nV, sizeof(float)) || dev_room(s->ctx, &p->dG, &p->capG, cnt.nV, sizeof(float)))
		return -1;
	memset(&a, 0, sizeof a);
	a.dV = g->dV; a.nV = cnt.nV; a.sign = MC33_NORMAL_NEG ? -1 : 1;
	a.oMean = (float *)p->dP; a.oGauss = (float *)p->dG;
	if (mc33hip_curvature_vertices(s->ctx, &a) != MC33HIP_OK ||
	    mc33hip_measure_surface(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, (const float *)p->dP, &m[0]) != MC33HIP_OK ||
	    mc33hip_measure_surface(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, (const float *)p->dG, &m[1]) != MC33HIP_OK)
		return -1;
	out->nV = (unsigned)cnt.nV; out->nT = (unsigned)cnt.nT;
	for (int q = 0; q != 4; q++) { out->lo[q] = a.lo[q]; out->hi[q] = a.hi[q]; }
	out->finite = a.finite; out->undefined = a.undefined;
	out->total_mean = a.undefined ? (double)NAN : m[0].property_integral;
	out->total_gauss = a.undefined ? (double)NAN : m[1].property_integral;
	return 0;
}

int MC33_measure_isosurface(MC33 *M, MC33_real iso, mc33_measure *out) {
	mc33_private *p = one_slab(M, MEASURE_ENTRIES);
	if (!p || !out)
		return -1;
	return measure_one(p, iso, out);
}

unsigned MC33_measure_isosurfaces(MC33 *M, const MC33_real *iso, unsigned count, mc33_measure *out) {
	mc33_private *p = one_slab(M, MEASURE_ENTRIES);
	unsigned done = 0;
	if (!out)
		return 0;
	memset(out, 0, (size_t)count * sizeof *out);
	if (!p || !iso)
		return 0;
	if (refresh_grid(p) != MC33HIP_OK)
		return 0;
	for (unsigned k = 0; k != count; k++) {
		if (k % 8 == 0 && count - k > 1)
			sweep_ahead(p, iso + k, count - k < 8 ? count - k : 8);
		if (measure_one(p, iso[k], &out[k]) == 0)
			done++;
		else
			memset(&out[k], 0, sizeof out[k]);
	}
	return done;
}

int MC33_measure_components(MC33 *M, MC33_real iso, mc33_component *table, unsigned capacity, unsigned *components, unsigned *unreferenced) {
	mc33_private *p = one_slab(M, MEASURE_ENTRIES);
	if (components) *components = 0;
	if (unreferenced) *unreferenced = 0;
	if (!p || (capacity && !table))
		return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	unsigned long long nc;
	const int r = labelled_for_table(p, iso, capacity, components, unreferenced, &cnt, &nc);
	if (r <= 0) /* the call's own result: failed, table too small, or no component */
		return r;
	return mc33hip_measure_components(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, (const unsigned *)p->dL, (mc33hip_component *)table, capacity, &nc) == MC33HIP_OK ? 0 : -1;
}

/* --- extension: topology of an isosurface, from its triangle list in staging set 0 ------------------------------------------ */
int MC33_isosurface_topology(MC33 *M, MC33_real iso, mc33_topology *out) {
	mc33_private *p = one_slab(M, TOPOLOGY_ENTRIES);
	if (!p || !out)
		return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	mc33hip_topology t;
	memset(out, 0, sizeof *out);
	M->iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK || mc33hip_surface_topology(s->ctx, g->dT, cnt.nT, cnt.nV, &t) != MC33HIP_OK)
		return -1;
	out->nV = (unsigned)t.nV; out->nT = (unsigned)t.nT;
	out->referenced_vertices = t.referenced_vertices; out->edges = t.edges; out->boundary_edges = t.boundary_edges;
	out->nonmanifold_edges = t.nonmanifold_edges; out->misoriented_edges = t.misoriented_edges;
	out->degenerate_triangles = t.degenerate_triangles; out->boundary_loops = t.boundary_loops; out->components = t.components;
	out->closed_components = t.closed_components; out->genus_sum = t.genus_sum; out->euler = t.euler;
	out->closed = t.closed; out->manifold = t.manifold; out->oriented = t.oriented; out->genus_defined = t.genus_defined;
	return 0;
}

int MC33_component_topology(MC33 *M, MC33_real iso, mc33_component_topology *table, unsigned capacity, unsigned *components) {
	mc33_private *p = one_slab(M, TOPOLOGY_ENTRIES);
	if (components) *components = 0;
	if (!p || (capacity && !table))
		return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	unsigned long long nc;
	const int r = labelled_for_table(p, iso, capacity, components, 0, &cnt, &nc);
	if (r <= 0) /* the call's own result: failed, table too small, or no component */
		return r;
	/* (mc33_component_topology has the members of struct mc33hip_component_topology, in its order) */
	return mc33hip_component_topology(s->ctx, g->dT, cnt.nT, cnt.nV, (const unsigned *)p->dL, (struct mc33hip_component_topology *)table, capacity, &nc) == MC33HIP_OK ? 0 : -1;
}

/* --- extension: keep or drop components of an isosurface ------------------------------------------------------------------------
 * The one selection rule (include/marching_cubes_33.h): host C, no GPU. */
struct sel_row { unsigned nT, root; };
static int sel_by_size(const void *a, const void *b) { /* most triangles first, ties to the smaller root */
	const struct sel_row *x = (const struct sel_row *)a, *y = (const struct sel_row *)b;
	if (x->nT != y->nT) return x->nT > y->nT ? -1 : 1;
	return x->root < y->root ? -1 : x->root > y->root;
}
static int sel_by_root(const void *a, const void *b) {
	const unsigned x = *(const unsigned *)a, y = *(const unsigned *)b;
	return x < y ? -1 : x > y;
}

int MC33_select_components(const mc33_component *table, const mc33_component_topology *topo, unsigned n, const mc33_component_filter *f, unsigned *roots) {
	if (!f || (n && (!table || !roots)) || (f->closed_only && !topo))
		return -1;
	unsigned m = 0;
	for (unsigned k = 0; k != n; k++) {
		const double w = table[k].volume < 0 ? -table[k].volume : table[k].volume;
		if (table[k].nT >= f->min_triangles && table[k].area >= f->min_area && w >= f->min_abs_volume && (!f->closed_only || topo[k].boundary_edges == 0))
			roots[m++] = k; /* (the row for now) */
	}
	if (f->largest && m > f->largest) {
		struct sel_row *r = (struct sel_row *)malloc((size_t)m * sizeof *r);
		if (!r)
			return -1;
		for (unsigned k = 0; k != m; k++) { r[k].nT = table[roots[k]].nT; r[k].root = table[roots[k]].root; }
		qsort(r, m, sizeof *r, sel_by_size);
		m = f->largest;
		for (unsigned k = 0; k != m; k++) roots[k] = r[k].root;
		free(r);
	} else
		for (unsigned k = 0; k != m; k++) roots[k] = table[roots[k]].root;
	if (m > 1) /* (n == 0 may come with roots == NULL) */
		qsort(roots, m, sizeof *roots, sel_by_root);
	return (int)m;
}

/* the surface of `iso` into staging set 0, its colours, labels, tables -> the roots to keep -> compacted into staging set 1 ->
 * the kept rows into a caller-owned surface */
struct filter_call {
	const mc33_component_filter *f;
	unsigned *kept, *dropped;
};
static surface *filtered_surface(mc33_private *p, MC33_real iso, const void *arg) {
	const struct filter_call *fc = (const struct filter_call *)arg;
	const mc33_component_filter *f = fc->f;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0], *h = &s->set[1];
	mc33hip_counts cnt;
	unsigned long long nc, nu;
	if (extract_labelled(p, iso, 1, &cnt, &nc, &nu))
		return 0;
	mc33_component *table = (mc33_component *)malloc((size_t)(nc ? nc : 1) * sizeof *table);
	mc33_component_topology *topo = f->closed_only ? (mc33_component_topology *)malloc((size_t)(nc ? nc : 1) * sizeof *topo) : 0;
	unsigned *roots = (unsigned *)malloc((size_t)(nc ? nc : 1) * sizeof *roots);
	surface *S = 0;
	int nk = -1;
	unsigned long long n2 = nc;
	if (table && roots && (topo || !f->closed_only) &&
	    (!nc || mc33hip_measure_components(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, (const unsigned *)p->dL, (mc33hip_component *)table, nc, &n2) == MC33HIP_OK) &&
	    (!nc || !topo ||
	     mc33hip_component_topology(s->ctx, g->dT, cnt.nT, cnt.nV, (const unsigned *)p->dL, (struct mc33hip_component_topology *)topo, nc, &n2) == MC33HIP_OK))
		nk = MC33_select_components(table, topo, (unsigned)nc, f, roots);
	if (nk >= 0) {
		mc33hip_compaction a;
		memset(&a, 0, sizeof a);
		a.V = g->dV; a.N = g->dN; a.T = g->dT; a.label = (const unsigned *)p->dL;
		a.nV = cnt.nV; a.nT = cnt.nT;
		a.roots = roots; a.n_roots = (unsigned long long)nk;
		if (coloured(p) && cnt.nV) { a.attr[0] = g->dC; a.n_attr = 1; }
		int rc;
		INTO_STAGING(rc, mc33hip_compact_components, s, h, a);
		if (rc == MC33HIP_OK && (S = surface_of_rows(p, h, a.nV_out, a.nT_out, iso)) != 0) {
			if (fc->kept) *fc->kept = (unsigned)a.components_kept;
			if (fc->dropped) *fc->dropped = (unsigned)(nc - a.components_kept);
		}
	}
	free(table); free(topo); free(roots);
	return S;
}

surface *MC33_calculate_filtered_isosurface(MC33 *M, MC33_real iso, const mc33_component_filter *f, unsigned *kept, unsigned *dropped) {
	mc33_private *p = one_slab(M, mc33hip_compact_components && mc33hip_label_components && mc33hip_measure_components && mc33hip_component_topology &&
	                                  mc33hip_color_vertices);
	if (kept) *kept = 0;
	if (dropped) *dropped = 0;
	if (!p || !f)
		return 0;
	const struct filter_call fc = {f, kept, dropped};
	return derived_call(p, iso, filtered_surface, &fc);
}

/* --- extension: a smoothed isosurface -----------------------------------------------------------------------------------------
 * The surface of `iso` into staging set 0, its colours from the vertices as they were extracted, the Taubin passes in place,
 * the normals from the smoothed positions, then the download: T, nV and nT are those of calculate_isosurface. */
static surface *smoothed_surface(mc33_private *p, MC33_real iso, const void *arg) {
	const mc33_smoothing *sm = (const mc33_smoothing *)arg;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	int rc = extract_coloured(p, g, iso, &cnt);
	if (rc == MC33HIP_OK && cnt.nV) {
		mc33hip_smoothing a;
		memset(&a, 0, sizeof a);
		a.V = g->dV; a.T = g->dT; a.nV = cnt.nV; a.nT = cnt.nT;
		a.iterations = sm->iterations; a.lambda = sm->lambda; a.mu = sm->mu; a.pin_boundary = sm->pin_boundary;
		a.oV = g->dV; a.oN = (float *)g->dN;
		rc = mc33hip_smooth_surface(s->ctx, &a);
	}
	return rc == MC33HIP_OK ? surface_from_staging(p, g, &cnt, iso, 0) : 0;
}

surface *MC33_calculate_smoothed_isosurface(MC33 *M, MC33_real iso, const mc33_smoothing *sm) {
	mc33_private *p = one_slab(M, mc33hip_smooth_surface && mc33hip_color_vertices);
	if (!p || !sm)
		return 0;
	if (!(sm->lambda > 0.0 && sm->lambda <= 1.0) || !(sm->mu >= -1.0 && sm->mu <= 0.0) || sm->iterations > 1000u)
		return 0; /* (what mc33hip_smooth_surface refuses, before anything is extracted) */
	return derived_call(p, iso, smoothed_surface, sm);
}

/* --- extension: a simplified isosurface ------------------------------------------------------------------------------------------
 * The surface of `iso` into staging set 0, its colours from the extracted vertices (attribute 0), clustered on the lattice
 * (r0, cell x d) into staging set 1 with the normals of the output, then the kept rows into a caller-owned surface. */
static int simplification_ok(const mc33_simplification *sp) {
	for (int j = 0; j != 3; j++)
		if (!(sp->cell[j] > 0.0 && sp->cell[j] <= DBL_MAX))
			return 0;
	return sp->mode == MC33HIP_SIMPLIFY_MEAN || sp->mode == MC33HIP_SIMPLIFY_FIRST;
}

static surface *simplified_surface(mc33_private *p, MC33_real iso, const void *arg) {
	const mc33_simplification *sp = (const mc33_simplification *)arg;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0], *h = &s->set[1];
	mc33hip_counts cnt;
	if (extract_coloured(p, g, iso, &cnt) != MC33HIP_OK)
		return 0;
	mc33hip_simplification a;
	memset(&a, 0, sizeof a);
	a.V = g->dV; a.T = g->dT; a.nV = cnt.nV; a.nT = cnt.nT;
	if (coloured(p) && cnt.nV) { a.attr[0] = g->dC; a.n_attr = 1; }
	for (int j = 0; j != 3; j++) { a.origin[j] = p->grd_r0[j]; a.cell[j] = sp->cell[j] * p->grd_d[j]; }
	a.mode = sp->mode; a.drop_duplicates = sp->drop_duplicates;
	int rc;
	INTO_STAGING(rc, mc33hip_simplify_surface, s, h, a);
	return rc == MC33HIP_OK ? surface_of_rows(p, h, a.nV_out, a.nT_out, iso) : 0;
}

surface *MC33_calculate_simplified_isosurface(MC33 *M, MC33_real iso, const mc33_simplification *sp) {
	mc33_private *p = one_slab(M, mc33hip_simplify_surface && mc33hip_color_vertices);
	if (!p || !sp || p->inclined)
		return 0;
	if (!simplification_ok(sp))
		return 0; /* (what mc33hip_simplify_surface refuses, before anything is extracted) */
	return derived_call(p, iso, simplified_surface, sp);
}

/* --- extension: the distance between two surfaces, taken on the device ------------------------------------------------------------
 * Both surfaces in the two staging sets of the one slab; the vertices of one against the triangles of the other. */
#define DISTANCE_ENTRIES (mc33hip_surface_distance != 0)

static int distance_one(mc33_slab *s, const void *dP, unsigned long long nP, const struct staging *target, unsigned long long nV, unsigned long long nT,
                        mc33_distance *out) {
	mc33hip_distance a;
	memset(&a, 0, sizeof a);
	a.P = dP; a.nP = nP; a.V = target->dV; a.T = target->dT; a.nV = nV; a.nT = nT;
	if (mc33hip_surface_distance(s->ctx, &a) != MC33HIP_OK)
		return -1;
	out->points = a.matched_points; out->unmatched = a.unmatched_points;
	out->max = a.max; out->min = a.min;
	out->mean = a.matched_points ? a.sum / (double)a.matched_points : 0.0;
	out->rms = a.matched_points ? sqrt(a.sum_sq / (double)a.matched_points) : 0.0;
	out->argmax = (unsigned)a.argmax;
	return 0;
}

int MC33_isosurface_distance(MC33 *M, MC33_real iso_from, MC33_real iso_to, mc33_distance *out) {
	mc33_private *p = one_slab(M, DISTANCE_ENTRIES);
	if (!p || !out)
		return -1;
	mc33_slab *s = &p->slab[0];
	mc33hip_counts from, to;
	memset(out, 0, sizeof *out);
	p->pub.iso = iso_to;
	if (extract_geometry(p, &s->set[0], iso_from, &from) != MC33HIP_OK || extract_geometry(p, &s->set[1], iso_to, &to) != MC33HIP_OK)
		return -1;
	if (!from.nV || !from.nT || !to.nV || !to.nT)
		return -2;
	return distance_one(s, s->set[0].dV, from.nV, &s->set[1], to.nV, to.nT, out);
}

int MC33_simplification_error(MC33 *M, MC33_real iso, const mc33_simplification *sp, mc33_distance out[2]) {
	mc33_private *p = one_slab(M, DISTANCE_ENTRIES && mc33hip_simplify_surface);
	if (!p || !sp || !out || p->inclined || !simplification_ok(sp))
		return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0], *h = &s->set[1];
	mc33hip_counts cnt;
	memset(out, 0, 2 * sizeof *out);
	p->pub.iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
		return -1;
	mc33hip_simplification a;
	memset(&a, 0, sizeof a);
	a.V = g->dV; a.T = g->dT; a.nV = cnt.nV; a.nT = cnt.nT;
	for (int j = 0; j != 3; j++) { a.origin[j] = p->grd_r0[j]; a.cell[j] = sp->cell[j] * p->grd_d[j]; }
	a.mode = sp->mode; a.drop_duplicates = sp->drop_duplicates;
	int rc;
	INTO_STAGING(rc, mc33hip_simplify_surface, s, h, a);
	if (rc != MC33HIP_OK)
		return -1;
	if (!cnt.nV || !cnt.nT || !a.nV_out || !a.nT_out)
		return -2;
	if (distance_one(s, h->dV, a.nV_out, g, cnt.nV, cnt.nT, &out[0]) || distance_one(s, g->dV, cnt.nV, h, a.nV_out, a.nT_out, &out[1])) {
		memset(out, 0, 2 * sizeof *out);
		return -1;
	}
	return 0;
}

/* --- extension: an isosurface clipped by planes --------------------------------------------------------------------------------
 * MC33_clip_box is host C.  The surface of `iso` into staging set 0, then plane after plane from one staging set into the other
 * (each grown to the sizes a refused call reports), the colours of the FINAL vertices from the property grid, then the kept
 * rows into a caller-owned surface. */
static int clip_finite(double x) { return x >= -DBL_MAX && x <= DBL_MAX; } /* (false for a NaN) */

static int clip_plane_ok(const double *pl) {
	for (int j = 0; j != 4; j++)
		if (!clip_finite(pl[j]))
			return 0;
	return pl[0] != 0.0 || pl[1] != 0.0 || pl[2] != 0.0;
}

int MC33_clip_box(const double lo[3], const double hi[3], mc33_clip *out) {
	if (!lo || !hi || !out)
		return -1;
	for (int j = 0; j != 3; j++)
		if (!clip_finite(lo[j]) || !clip_finite(hi[j]) || !(lo[j] < hi[j]))
			return -1;
	memset(out, 0, sizeof *out);
	out->n = 6;
	for (int j = 0; j != 3; j++) { /* x - lo0, hi0 - x, y - lo1, hi1 - y, z - lo2, hi2 - z */
		out->plane[2 * j][j] = 1.0; out->plane[2 * j][3] = -lo[j];
		out->plane[2 * j + 1][j] = -1.0; out->plane[2 * j + 1][3] = hi[j];
	}
	return 0;
}

static surface *clipped_surface(mc33_private *p, MC33_real iso, const void *arg) {
	const mc33_clip *cl = (const mc33_clip *)arg;
	mc33_slab *s = &p->slab[0];
	mc33hip_counts cnt;
	int cur = 0;
	if (extract_geometry(p, &s->set[0], iso, &cnt) != MC33HIP_OK)
		return 0;
	for (unsigned k = 0; k != cl->n && cnt.nT; k++) {
		struct staging *g = &s->set[cur], *h = &s->set[cur ^ 1];
		mc33hip_clipping a;
		memset(&a, 0, sizeof a);
		a.V = g->dV; a.N = g->dN; a.T = g->dT; a.nV = cnt.nV; a.nT = cnt.nT;
		for (int j = 0; j != 4; j++) a.plane[j] = cl->plane[k][j];
		int rc;
		INTO_STAGING(rc, mc33hip_clip_surface, s, h, a);
		if (rc != MC33HIP_OK)
			return 0;
		cnt.nV = a.nV_out; cnt.nT = a.nT_out;
		cur ^= 1;
	}
	if (!cnt.nT)
		cnt.nV = 0; /* (a plane that removes everything leaves no vertex either) */
	if (coloured(p) && cnt.nV) { /* a new vertex gets the colour of its own position */
		p->nan_color = DefaultColorMC;
		if (enqueue_colors(s, &s->set[cur], cnt.nV) != MC33HIP_OK)
			return 0;
	}
	return surface_from_staging(p, &s->set[cur], &cnt, iso, 0);
}

surface *MC33_calculate_clipped_isosurface(MC33 *M, MC33_real iso, const mc33_clip *cl) {
	mc33_private *p = one_slab(M, mc33hip_clip_surface && mc33hip_color_vertices);
	if (!p || !cl)
		return 0;
	if (cl->n > 6u)
		return 0;
	for (unsigned k = 0; k != cl->n; k++)
		if (!clip_plane_ok(cl->plane[k]))
			return 0; /* (what mc33hip_clip_surface refuses, before anything is extracted) */
	return derived_call(p, iso, clipped_surface, cl);
}

/* --- extension: an isosurface closed at the faces of the grid ------------------------------------------------------------------
 * The surface of `iso` into staging set 0 and the caps behind it, in place: first with the set as it stands (an extraction leaves an
 * eighth to spare), and when that is refused for room, the set grown to the sizes that came back, the surface extracted into it
 * again - what a set held does not survive its growth - and capped there.  Then the colours of the FINAL vertices and one download. */
struct cap_job { const mc33_cap *options; mc33_cap_info *info; };

static void cap_box(const MC33 *M, const mc33_cap *o, unsigned lo[3], unsigned hi[3]) {
	const unsigned N[3] = {M->nx, M->ny, M->nz};
	const int whole = !o || (o->hi[0] == 0u && o->hi[1] == 0u && o->hi[2] == 0u);
	for (int a = 0; a != 3; a++) {
		lo[a] = whole ? 0u : o->lo[a];
		hi[a] = whole ? N[a] : o->hi[a];
	}
}

static surface *capped_surface(mc33_private *p, MC33_real iso, const void *arg) {
	const struct cap_job *job = (const struct cap_job *)arg;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	mc33hip_capping a;
	int rc = MC33HIP_ECAPACITY;
	memset(&a, 0, sizeof a);
	for (int attempt = 0; attempt != 2 && rc == MC33HIP_ECAPACITY; attempt++) {
		if (attempt && staging_room(s, g, a.nV_out, a.nT_out))
			return 0;
		if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
			return 0;
		memset(&a, 0, sizeof a);
		a.V = g->dV; a.N = g->dN; a.T = g->dT; a.nV = cnt.nV; a.nT = cnt.nT;
		a.capV = g->capV; a.capT = g->capT;
		a.iso = (double)iso;
		cap_box(&p->pub, job->options, a.lo, a.hi);
		a.invert = job->options ? job->options->invert : 0;
		rc = mc33hip_cap_surface(s->ctx, &a);
	}
	if (rc != MC33HIP_OK)
		return 0;
	cnt.nV = a.nV_out; cnt.nT = a.nT_out;
	if (coloured(p) && cnt.nV) { /* a new vertex gets the colour of its own position */
		p->nan_color = DefaultColorMC;
		if (enqueue_colors(s, g, cnt.nV) != MC33HIP_OK)
			return 0;
	}
	if (job->info) {
		mc33_cap_info *q = job->info;
		q->nV = (unsigned)a.nV_out; q->nT = (unsigned)a.nT_out;
		q->cap_vertices = (unsigned)a.cap_vertices; q->cap_triangles = (unsigned)a.cap_triangles; q->rim_segments = (unsigned)a.rim_segments;
		q->capped_cells = (unsigned)a.capped_cells; q->skipped_cells = (unsigned)a.skipped_cells; q->off_face_edges = (unsigned)a.off_face_edges;
		q->solid_above = a.solid_above; q->closed = a.closed;
	}
	return surface_from_staging(p, g, &cnt, iso, 0);
}

surface *MC33_calculate_capped_isosurface(MC33 *M, MC33_real iso, const mc33_cap *options, mc33_cap_info *info) {
	mc33_private *p = one_slab(M, mc33hip_cap_surface && mc33hip_color_vertices);
	if (!p || p->inclined || iso != iso)
		return 0;
	unsigned lo[3], hi[3];
	cap_box(M, options, lo, hi);
	const unsigned N[3] = {M->nx, M->ny, M->nz};
	for (int a = 0; a != 3; a++)
		if (!(lo[a] < hi[a] && hi[a] <= N[a]))
			return 0; /* (what mc33hip_cap_surface refuses, before anything is extracted) */
	struct cap_job job = {options, info};
	if (info) memset(info, 0, sizeof *info);
	return derived_call(p, iso, capped_surface, &job);
}

/* --- extension: pictures of an isosurface ------------------------------------------------------------------------------------
 * The surface of `iso` with its colours into staging set 0, once; every view drawn from there into p->dImg and only the arrays the
 * caller wants brought to the host.  The images are collected beside `out` and copied there when all views are done. */
static int view_ok(const mc33_view *v) { /* what mc33hip_render_surface refuses, before anything is extracted */
	int finite = isfinite(v->ambient) && isfinite(v->diffuse);
	for (int k = 0; k != 16; k++) finite = finite && isfinite(v->m[k]);
	for (int k = 0; k != 3; k++) finite = finite && isfinite(v->light[k]);
	if (!finite || v->width == 0u || v->width > 4096u || v->height == 0u || v->height > 4096u || v->cull < 0 || v->cull > 2)
		return 0;
	const double len = sqrt((v->light[0] * v->light[0] + v->light[1] * v->light[1]) + v->light[2] * v->light[2]);
	return len > 0.0 && isfinite(len);
}

void MC33_free_image(mc33_image *image) {
	if (!image)
		return;
	free(image->rgba); free(image->depth); free(image->triangle);
	image->rgba = 0; image->depth = 0; image->triangle = 0;
}

static int render_view(mc33_private *p, const struct staging *g, const mc33hip_counts *cnt, const mc33_view *v, unsigned want, mc33_image *img) {
	mc33_slab *s = &p->slab[0];
	const unsigned long long pixels = (unsigned long long)v->width * v->height;
	mc33hip_rendering a;
	memset(&a, 0, sizeof a);
	for (int b = 0; b != 3; b++)
		if ((want >> b & 1u) && dev_room(s->ctx, &p->dImg[b], &p->capImg[b], pixels, 4))
			return -1;
	a.V = g->dV; a.N = g->dN; a.T = g->dT; a.nV = cnt->nV; a.nT = cnt->nT;
	a.C = coloured(p) && cnt->nV ? g->dC : 0;
	a.base_color = (unsigned)DefaultColorMC;
	memcpy(a.m, v->m, sizeof a.m);
	a.width = v->width; a.height = v->height; a.cull = v->cull; a.two_sided = v->two_sided;
	memcpy(a.light, v->light, sizeof a.light);
	a.ambient = v->ambient; a.diffuse = v->diffuse; a.background = v->background;
	a.oRGBA = want & MC33_IMAGE_RGBA ? p->dImg[0] : 0;
	a.oDepth = want & MC33_IMAGE_DEPTH ? p->dImg[1] : 0;
	a.oTri = want & MC33_IMAGE_IDS ? p->dImg[2] : 0;
	if (mc33hip_render_surface(s->ctx, &a) != MC33HIP_OK)
		return -1;
	void **host[3] = {(void **)&img->rgba, (void **)&img->depth, (void **)&img->triangle};
	for (int b = 0; b != 3; b++) {
		if (!(want >> b & 1u))
			continue;
		if (!(*host[b] = malloc((size_t)pixels * 4)) || mc33hip_download(s->ctx, *host[b], p->dImg[b], (size_t)pixels * 4) != MC33HIP_OK)
			return -1;
	}
	img->width = v->width; img->height = v->height;
	img->drawn = (unsigned)a.drawn; img->culled = (unsigned)a.culled; img->degenerate = (unsigned)a.degenerate; img->rejected = (unsigned)a.rejected;
	img->offscreen = (unsigned)a.offscreen; img->invalid_triangles = (unsigned)a.invalid_triangles;
	img->fragments = a.fragments; img->covered = a.covered;
	img->nV = (unsigned)cnt->nV; img->nT = (unsigned)cnt->nT;
	return 0;
}

int MC33_render_isosurface(MC33 *M, MC33_real iso, const mc33_view *views, unsigned n, unsigned want, mc33_image *out) {
	mc33_private *p = one_slab(M, mc33hip_render_surface != 0);
	if (!p || !views || !out || n == 0u || !(want & (MC33_IMAGE_RGBA | MC33_IMAGE_DEPTH | MC33_IMAGE_IDS)))
		return -1;
	for (unsigned k = 0; k != n; k++)
		if (!view_ok(&views[k]))
			return -1;
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	M->iso = iso;
	mc33_image *img = (mc33_image *)calloc(n, sizeof *img);
	if (!img)
		return -1;
	int ok = extract_coloured(p, g, iso, &cnt) == MC33HIP_OK;
	for (unsigned k = 0; ok && k != n; k++) ok = render_view(p, g, &cnt, &views[k], want, &img[k]) == 0;
	if (ok)
		memcpy(out, img, n * sizeof *img);
	else
		for (unsigned k = 0; k != n; k++) MC33_free_image(&img[k]);
	free(img);
	return ok ? (int)n : -1;
}

/* the eight corners of the grid's box in the coordinates of the vertices: r0 + A (i d0, j d1, k d2), A the identity unless the grid
 * is inclined (MC:608-610) */
static void box_corners(const mc33_private *p, double c[8][3]) {
	const unsigned N[3] = {p->pub.nx, p->pub.ny, p->pub.nz};
	for (int q = 0; q != 8; q++) {
		double g[3];
		for (int a = 0; a != 3; a++) g[a] = (q >> a & 1) ? (double)N[a] * p->grd_d[a] : 0.0;
		for (int a = 0; a != 3; a++)
			c[q][a] = p->grd_r0[a] + (p->inclined ? (p->grd_A[3 * a] * g[0] + p->grd_A[3 * a + 1] * g[1]) + p->grd_A[3 * a + 2] * g[2] : g[a]);
	}
}

static double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

int MC33_view_fit(MC33 *M, const double dir[3], const double up[3], double fov_degrees, unsigned width, unsigned height, mc33_view *out) {
	const mc33_private *p = priv(M);
	if (!p || !dir || !up || !out || !(fov_degrees >= 0.0 && fov_degrees <= 170.0) || width == 0u || width > 4096u || height == 0u || height > 4096u)
		return -1;
	for (int a = 0; a != 3; a++)
		if (!isfinite(dir[a]) || !isfinite(up[a]))
			return -1;
	/* f: the viewing direction, r: to the right, u: upwards in the image; the vectors are scaled by their largest component first
	 * so that no square overflows */
	double f[3], r[3], u[3], w[3];
	const double dm = fmax(fabs(dir[0]), fmax(fabs(dir[1]), fabs(dir[2]))), um = fmax(fabs(up[0]), fmax(fabs(up[1]), fabs(up[2])));
	if (!(dm > 0.0) || !(um > 0.0))
		return -1;
	for (int a = 0; a != 3; a++) { f[a] = dir[a] / dm; w[a] = up[a] / um; }
	const double fl = sqrt(dot3(f, f)), wl = sqrt(dot3(w, w));
	for (int a = 0; a != 3; a++) { f[a] /= fl; w[a] /= wl; }
	r[0] = f[1] * w[2] - f[2] * w[1]; r[1] = f[2] * w[0] - f[0] * w[2]; r[2] = f[0] * w[1] - f[1] * w[0];
	const double rl = sqrt(dot3(r, r));
	if (!(rl > 1e-7)) /* up (anti)parallel to dir, as far as doubles can tell */
		return -1;
	for (int a = 0; a != 3; a++) r[a] /= rl;
	u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
	double c[8][3], mid[3] = {0.0, 0.0, 0.0};
	box_corners(p, c);
	for (int q = 0; q != 8; q++)
		for (int a = 0; a != 3; a++) mid[a] += 0.125 * c[q][a];
	/* the corners about the middle of the box, in the view's axes */
	double e[8][3], zmin = DBL_MAX, zmax = -DBL_MAX, hx = 0.0, hy = 0.0;
	for (int q = 0; q != 8; q++) {
		const double d[3] = {c[q][0] - mid[0], c[q][1] - mid[1], c[q][2] - mid[2]};
		e[q][0] = dot3(r, d); e[q][1] = dot3(u, d); e[q][2] = dot3(f, d);
		hx = fmax(hx, fabs(e[q][0])); hy = fmax(hy, fabs(e[q][1]));
		zmin = fmin(zmin, e[q][2]); zmax = fmax(zmax, e[q][2]);
	}
	const double span = zmax - zmin, aspect = (double)width / (double)height, margin = 1.02, zpad = span * 0x1p-10;
	if (!(span > 0.0) || !isfinite(span))
		return -1;
	mc33_view v;
	memset(&v, 0, sizeof v);
	double row[4][3], off[4]; /* clip row = row . (p - mid) + off */
	if (fov_degrees == 0.0) {
		const double a = margin * fmax(hx / (double)width, hy / (double)height); /* half a pixel's worth ... x width, x height: the half extents */
		const double zn = zmin - zpad, zf = zmax + zpad;
		for (int k = 0; k != 3; k++) { row[0][k] = r[k] / (a * (double)width); row[1][k] = u[k] / (a * (double)height); row[2][k] = f[k] / (zf - zn); row[3][k] = 0.0; }
		off[0] = 0.0; off[1] = 0.0; off[2] = -zn / (zf - zn); off[3] = 1.0;
	} else {
		const double th = tan(fov_degrees * (3.14159265358979323846 / 360.0));
		double D = 0.0; /* the eye sits D behind the middle of the box: every corner inside the pyramid */
		for (int q = 0; q != 8; q++) D = fmax(D, fmax(fabs(e[q][0]) / (th * aspect), fabs(e[q][1]) / th) - e[q][2]);
		D = fmax(margin * D, 0.05 * span - zmin);
		const double zn = D + zmin - 0x1p-10 * fmin(span, D + zmin), zf = D + zmax + zpad, A = zf / (zf - zn), B = -(zf * zn) / (zf - zn);
		for (int k = 0; k != 3; k++) { row[0][k] = r[k] / (th * aspect); row[1][k] = u[k] / th; row[3][k] = f[k]; row[2][k] = A * f[k]; }
		off[0] = 0.0; off[1] = 0.0; off[3] = D; off[2] = A * D + B;
	}
	for (int j = 0; j != 4; j++) {
		for (int k = 0; k != 3; k++) v.m[4 * j + k] = row[j][k];
		v.m[4 * j + 3] = off[j] - dot3(row[j], mid);
	}
	for (int k = 0; k != 16; k++)
		if (!isfinite(v.m[k]))
			return -1;
	v.width = width; v.height = height; v.cull = 0; v.two_sided = 1;
	for (int a = 0; a != 3; a++) v.light[a] = -f[a];
	v.ambient = 0.2; v.diffuse = 0.8; v.background = 0xFF000000u;
	*out = v;
	return 0;
}

/* --- extension: the section of an isosurface by a plane ------------------------------------------------------------------------
 * The surface goes into staging set 0, its section into the arrays of set 1 under other names - the points in dV, the segments
 * in dT (12 bytes a row there: capT rows hold capT segments and more), the contour words and the next words side by side in dN
 * (three words a row there), the colours in dC - first with the set as it stands and, when that is refused for room, once more
 * with the set grown to the sizes that came back. */
#define SECTION_ENTRIES (mc33hip_section_surface && mc33hip_section_contours && mc33hip_section_ladder && mc33hip_color_vertices && mc33hip_download)
_Static_assert(sizeof(mc33_contour) == sizeof(mc33hip_contour) && offsetof(mc33_contour, length) == offsetof(mc33hip_contour, length),
               "mc33_contour and mc33hip_contour are one layout");

static int section_to_staging(mc33_private *p, MC33_real iso, const double plane[4], mc33hip_section *a) {
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0], *h = &s->set[1];
	mc33hip_counts cnt;
	p->pub.iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
		return -1;
	memset(a, 0, sizeof *a);
	a->V = g->dV; a->T = g->dT; a->nV = cnt.nV; a->nT = cnt.nT;
	for (int j = 0; j != 4; j++) a->plane[j] = plane[j];
	int rc = MC33HIP_ECAPACITY;
	for (int attempt = 0; attempt != 2 && rc == MC33HIP_ECAPACITY; attempt++) {
		if (attempt && staging_room(s, h, a->nP_out, a->nS_out))
			return -1;
		a->oP = h->dV; a->oS = h->dT; a->capP = h->capV; a->capS = h->capT;
		a->oLabel = (unsigned *)h->dN; a->oNext = h->dN ? (unsigned *)h->dN + h->capV : 0;
		rc = mc33hip_section_surface(s->ctx, a);
	}
	return rc == MC33HIP_OK ? 0 : -1;
}

void MC33_free_section(mc33_section *S) {
	if (S) {
		free(S->P); free(S->S); free(S->contour); free(S->next); free(S->color);
		free(S);
	}
}

mc33_section *MC33_section_isosurface(MC33 *M, MC33_real iso, const double plane[4]) {
	mc33_private *p = one_slab(M, SECTION_ENTRIES);
	if (!p || !plane || !clip_plane_ok(plane))
		return 0;
	mc33_slab *s = &p->slab[0];
	struct staging *h = &s->set[1];
	mc33hip_section a;
	if (section_to_staging(p, iso, plane, &a))
		return 0;
	const size_t nP = (size_t)a.nP_out, nS = (size_t)a.nS_out;
	const int paint = coloured(p) && nP;
	if (paint) { /* a point gets the colour of its own position */
		p->nan_color = DefaultColorMC;
		if (enqueue_colors(s, h, nP) != MC33HIP_OK)
			return 0;
	}
	mc33_section *S = (mc33_section *)calloc(1, sizeof *S);
	if (!S)
		return 0;
	S->P = malloc((nP ? nP : 1) * sizeof *S->P); S->S = malloc((nS ? nS : 1) * sizeof *S->S);
	S->contour = (unsigned *)malloc((nP ? nP : 1) * sizeof(unsigned)); S->next = (unsigned *)malloc((nP ? nP : 1) * sizeof(unsigned));
	S->color = (int *)malloc((nP ? nP : 1) * sizeof(int));
	int ok = S->P && S->S && S->contour && S->next && S->color;
	if (ok && nP)
		ok = mc33hip_download(s->ctx, S->P, h->dV, nP * sizeof *S->P) == MC33HIP_OK && mc33hip_download(s->ctx, S->contour, a.oLabel, nP * sizeof(unsigned)) == MC33HIP_OK &&
		     mc33hip_download(s->ctx, S->next, a.oNext, nP * sizeof(unsigned)) == MC33HIP_OK;
	if (ok && nS)
		ok = mc33hip_download(s->ctx, S->S, h->dT, nS * sizeof *S->S) == MC33HIP_OK;
	if (ok && paint)
		ok = mc33hip_download(s->ctx, S->color, h->dC, nP * sizeof(int)) == MC33HIP_OK;
	if (!ok) {
		MC33_free_section(S);
		return 0;
	}
	if (!paint)
		for (size_t k = 0; k != nP; k++) S->color[k] = DefaultColorMC;
	S->nP = (unsigned)nP; S->nS = (unsigned)nS;
	S->on_points = (unsigned)a.on_points; S->cut_points = (unsigned)a.cut_points; S->contours = (unsigned)a.contours;
	S->closed_contours = (unsigned)a.closed_contours; S->open_ends = (unsigned)a.open_ends; S->branch_points = (unsigned)a.branch_points;
	S->degenerate_segments = (unsigned)a.degenerate_segments;
	S->length = a.length; S->area = a.area;
	for (int j = 0; j != 4; j++) S->plane[j] = plane[j];
	return S;
}

int MC33_section_contours(MC33 *M, MC33_real iso, const double plane[4], mc33_contour *table, unsigned capacity, unsigned *contours) {
	mc33_private *p = one_slab(M, SECTION_ENTRIES);
	if (contours) *contours = 0;
	if (!p || !plane || !clip_plane_ok(plane) || (capacity && !table))
		return -1;
	mc33_slab *s = &p->slab[0];
	mc33hip_section a;
	if (section_to_staging(p, iso, plane, &a))
		return -1;
	if (contours) *contours = (unsigned)a.contours;
	if (capacity < a.contours)
		return -2;
	if (!a.contours)
		return 0;
	unsigned long long n = 0;
	return mc33hip_section_contours(s->ctx, a.oP, a.nP_out, a.oS, a.nS_out, a.oLabel, plane, (mc33hip_contour *)table, capacity, &n) == MC33HIP_OK ? 0 : -1;
}

int MC33_section_profile(MC33 *M, MC33_real iso, const double normal[3], const double *offsets, unsigned n, mc33_section_level *out) {
	mc33_private *p = one_slab(M, SECTION_ENTRIES);
	if (!p || !normal || n > 255u || (n && (!offsets || !out)))
		return -1;
	const double pl[4] = {normal[0], normal[1], normal[2], 0.0};
	if (!clip_plane_ok(pl))
		return -1;
	for (unsigned k = 0; k != n; k++)
		if (!clip_finite(offsets[k]) || (k && !(offsets[k] > offsets[k - 1])))
			return -1; /* (what mc33hip_section_ladder refuses, before anything is extracted) */
	mc33_slab *s = &p->slab[0];
	struct staging *g = &s->set[0];
	mc33hip_counts cnt;
	unsigned long long seg[255], bad = 0;
	double len[255], area[255];
	p->pub.iso = iso;
	if (extract_geometry(p, g, iso, &cnt) != MC33HIP_OK)
		return -1;
	if (mc33hip_section_ladder(s->ctx, g->dV, cnt.nV, g->dT, cnt.nT, normal, offsets, n, seg, len, area, &bad) != MC33HIP_OK)
		return -1;
	for (unsigned k = 0; k != n; k++) { out[k].segments = seg[k]; out[k].length = len[k]; out[k].area = area[k]; }
	return 0;
}

void free_surface_memory(surface *S) { /* MC:84-92 */
	if (S) {
		void *blk[4] = {S->T, S->V, S->N, S->color};
		surface_blocks_release(blk, 4);
		free(S);
	}
}

void adjustvectorlenght_s(surface *S) { /* MC:94-127: shrink the four arrays to nV / nT elements */
	if (!S)
		return;
	if (S->capv > S->nV) {
		void *c = malloc(sizeof(int) * (size_t)S->nV), *n = malloc(3 * sizeof(float) * (size_t)S->nV),
		     *v = malloc(3 * sizeof(MC33_real) * (size_t)S->nV);
		if (!c || !n || !v) { free(c); free(n); free(v); return; }
		memcpy(c, S->color, sizeof(int) * (size_t)S->nV);
		memcpy(n, S->N, 3 * sizeof(float) * (size_t)S->nV);
		memcpy(v, S->V, 3 * sizeof(MC33_real) * (size_t)S->nV);
		surface_block_release(S->color); surface_block_release(S->N); surface_block_release(S->V);
		S->color = (int *)c; S->N = (float(*)[3])n; S->V = (MC33_real(*)[3])v;
		S->capv = S->nV;
	}
	if (S->capt > S->nT) {
		void *t = malloc(3 * sizeof(int) * (size_t)S->nT);
		if (!t) return;
		memcpy(t, S->T, 3 * sizeof(int) * (size_t)S->nT);
		surface_block_release(S->T);
		S->T = (unsigned int(*)[3])t;
		S->capt = S->nT;
	}
}

/* ---- grid container helpers (UTIL:125-169, 585-686), needed by callers that build grids ---------- */
/* cell angles 90 degrees, identity cell matrices (the members do not exist in GRD_ORTHOGONAL builds) */
static void set_orthogonal(_GRD *Z) {
#ifndef GRD_ORTHOGONAL
	Z->nonortho = 0;
	memset(Z->_A, 0, sizeof Z->_A);
	memset(Z->A_, 0, sizeof Z->A_);
	for (int i = 0; i != 3; i++) {
		Z->Ang[i] = 90.0f;
		Z->_A[i][i] = Z->A_[i][i] = 1.0;
	}
#else
	(void)Z;
#endif
}

void free_memory_grd(_GRD *Z) { /* UTIL:125-145 */
	if (!Z)
		return;
	if (Z->F) {
		for (unsigned int k = 0; k <= Z->N[2] && Z->F[k]; k++) {
			if (Z->internal_data)
				for (unsigned int j = 0; j <= Z->N[1]; j++)
					free(Z->F[k][j]);
			free(Z->F[k]);
		}
		free(Z->F);
	}
	free(Z);
}

int alloc_F(_GRD *Z) { /* UTIL:147-169: every row is its own allocation */
	const size_t np = (size_t)Z->N[2] + 1, nr = (size_t)Z->N[1] + 1, nc = (size_t)Z->N[0] + 1;
	Z->F = (GRD_data_type ***)calloc(np + 1, sizeof(void *)); /* one spare NULL terminates partial grids */
	if (!Z->F)
		return -1;
	Z->internal_data = 1;
	for (size_t k = 0; k != np; k++) {
		Z->F[k] = (GRD_data_type **)calloc(nr, sizeof(void *));
		if (!Z->F[k])
			return -1;
		for (size_t j = 0; j != nr; j++)
			if (!(Z->F[k][j] = (GRD_data_type *)malloc(nc * sizeof(GRD_data_type))))
				return -1;
	}
	return 0;
}

_GRD *grid_from_data_pointer(unsigned int Nx, unsigned int Ny, unsigned int Nz, GRD_data_type *data) { /* UTIL:585-627 */
	if (!data || !Nx || !Ny || !Nz)
		return 0;
	_GRD *Z = (_GRD *)calloc(1, sizeof(_GRD));
	if (!Z)
		return 0;
	Z->F = (GRD_data_type ***)calloc((size_t)Nz + 1, sizeof(void *));
	if (!Z->F) { free(Z); return 0; }
	Z->N[0] = Nx - 1; Z->N[1] = Ny - 1; Z->N[2] = Nz - 1;
	for (unsigned int k = 0; k != Nz; k++) {
		Z->F[k] = (GRD_data_type **)malloc((size_t)Ny * sizeof(void *));
		if (!Z->F[k]) { free_memory_grd(Z); return 0; }
		for (unsigned int j = 0; j != Ny; j++)
			Z->F[k][j] = data + ((size_t)k * Ny + j) * Nx;
	}
	for (int i = 0; i != 3; i++) {
		Z->L[i] = (float)Z->N[i];
		Z->d[i] = 1.0;
		Z->r0[i] = 0.0;
	}
	set_orthogonal(Z);
	return Z;
}

_GRD *generate_grid_from_fn(double xi, double yi, double zi, double xf, double yf, double zf, double dx, double dy,
                            double dz, double (*fn)(double x, double y, double z)) { /* UTIL:630-686 */
	if (dx <= 0 || dy <= 0 || dz <= 0 || xi == xf || yi == yf || zi == zf)
		return 0;
	double lo[3] = {xi, yi, zi}, hi[3] = {xf, yf, zf}, st[3] = {dx, dy, dz};
	_GRD *Z = (_GRD *)calloc(1, sizeof(_GRD));
	if (!Z)
		return 0;
	for (int i = 0; i != 3; i++) {
		if (lo[i] > hi[i]) { double t = lo[i]; lo[i] = hi[i]; hi[i] = t; }
		if (hi[i] - lo[i] < st[i]) st[i] = hi[i] - lo[i];
		Z->N[i] = (unsigned int)(int)((hi[i] - lo[i]) / st[i] + 0.5); /* intervals, UTIL:649-651 */
		Z->d[i] = st[i];
		Z->r0[i] = lo[i];
	}
	if (alloc_F(Z)) { free_memory_grd(Z); return 0; }
	if (fn) { /* coordinates advance by repeated addition, UTIL:660-672 */
		double z = lo[2];
		for (unsigned int k = 0; k <= Z->N[2]; k++, z += st[2]) {
			double y = lo[1];
			for (unsigned int j = 0; j <= Z->N[1]; j++, y += st[1]) {
				double x = lo[0];
				GRD_data_type *row = Z->F[k][j];
				for (unsigned int i = 0; i <= Z->N[0]; i++, x += st[0])
					row[i] = (GRD_data_type)fn(x, y, z);
			}
		}
	}
	for (int i = 0; i != 3; i++) {
		Z->L[i] = (float)(Z->N[i] * Z->d[i]);
	}
	set_orthogonal(Z);
	return Z;
}

/* --- extension: the grid resampled on the device before extraction -------------------------------------------------------------- */
int MC33_gaussian_taps(double sigma, unsigned radius, double *taps) {
	if (!taps || !(sigma >= 0.0 && sigma <= DBL_MAX))
		return -1;
	if (sigma == 0.0) {
		taps[0] = 1.0;
		return 0;
	}
	if (radius > 8u || (!radius && 3.0 * sigma > 8.0)) /* (before the cast: ceil(3 sigma) may be beyond an unsigned) */
		return -1;
	unsigned r = radius;
	if (!r) {
		r = (unsigned)ceil(3.0 * sigma);
		if (r < 1u) r = 1u;
	}
	double e[9];
	for (unsigned i = 0; i <= r; i++)
		e[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma));
	double S = e[0];
	for (unsigned i = 1; i <= r; i++)
		S = S + (e[i] + e[i]);
	for (unsigned i = 0; i <= r; i++)
		taps[r - i] = taps[r + i] = e[i] / S;
	return (int)r;
}

/* the row pitch of a grid this library allocates: rows on 16-byte boundaries (the rule of the device layer's own copy) */
static size_t resampled_pitch(size_t npx) {
	const size_t unit = sizeof(GRD_data_type) >= 4 ? 4 : 16 / sizeof(GRD_data_type);
	return (npx + unit - 1) / unit * unit;
}

/* What MC33_create_resampled and MC33_create_ranked share: the new object of npo points per axis and spacing `step` beside source
 * object sp (whose inclined matrices it takes over), its context on the source's device, the grid allocated through that context at
 * a 16-byte row pitch, written ONCE by `write` - a call of the device layer on the source's context that waits -, adopted and
 * declared stable.  free_MC33 releases the grid through the context (own_grid) in every outcome; NULL after any failure. */
typedef int grid_writer(mc33hip_ctx *source, const void *arg, void *dst, size_t pitch, size_t slice);
static MC33 *create_device_grid_object(mc33_private *sp, const unsigned npo[3], const double step[3], grid_writer *write, const void *arg) {
	mc33_slab *ss = &sp->slab[0];
	/* (an inclined source: the matrices of its _GRD, scaled by the new spacing) */
	mc33_private *p = new_object(npo[0] - 1u, npo[1] - 1u, npo[2] - 1u, sp->grd_r0, step, sp->inclined ? sp->grd_A : 0, sp->inclined ? sp->grd_Ai : 0);
	if (!p)
		return 0;
	MC33 *M = &p->pub;
	p->nslab = 1;
	mc33_slab *s = &p->slab[0];
	s->owner = p;
	s->device = mc33hip_context_device(ss->ctx); /* (the ordinal the source's context resolved: -1 would mean today's current device) */
	s->z_begin = 0; s->z_end = M->nz; s->ghost = 0; s->p_lo = 0; s->p_hi = M->nz;
	mc33hip_grid_desc d;
	memset(&d, 0, sizeof d);
	d.npx = npo[0]; d.npy = npo[1]; d.npz_resident = npo[2];
	d.plane0 = 0; d.nz_total = M->nz;
	for (int j = 0; j != 3; j++) { d.r0[j] = p->grd_r0[j]; d.d[j] = p->grd_d[j]; }
	d.sample_bytes = (int)sizeof(GRD_data_type);
	d.device = s->device;
	p->own_pitch = resampled_pitch(npo[0]);
	p->own_slice = p->own_pitch * npo[1];
	int rc = mc33hip_create(&s->ctx, &d);
	if (rc == MC33HIP_OK) rc = mc33hip_set_normal_neg(s->ctx, MC33_NORMAL_NEG);
	if (rc == MC33HIP_OK) rc = refresh_grid(sp); /* (samples the caller said it rewrote: uploaded first, as before an extraction) */
	if (rc == MC33HIP_OK) /* (64 samples to spare behind the last row, like the device layer's own copy) */
		rc = mc33hip_device_alloc(s->ctx, &p->own_grid, (p->own_slice * npo[2] + 64) * sizeof(GRD_data_type));
	if (rc == MC33HIP_OK) rc = write(ss->ctx, arg, p->own_grid, p->own_pitch, p->own_slice); /* (waits) */
	if (rc == MC33HIP_OK) rc = mc33hip_adopt_device(s->ctx, p->own_grid, p->own_pitch, p->own_slice);
	if (rc == MC33HIP_OK && mc33hip_grid_stable) /* (own_grid is written by the call above and never again: the sweeps may keep a range table over it) */
		rc = mc33hip_grid_stable(s->ctx, 1);
	if (rc != MC33HIP_OK) {
		free_MC33(M);
		return 0;
	}
	return M;
}

static int write_resampled(mc33hip_ctx *source, const void *arg, void *dst, size_t pitch, size_t slice) {
	return mc33hip_resample_grid(source, (const mc33hip_resampling *)arg, dst, pitch, slice);
}

MC33 *MC33_create_resampled(MC33 *source, const mc33_resampling *r) {
	mc33_private *sp = one_slab(source, mc33hip_resampled_size && mc33hip_resample_grid && mc33hip_context_device && mc33hip_adopt_device);
	if (!sp || !r)
		return 0;
	double w[3][17];
	mc33hip_resampling hr;
	unsigned npo[3];
	for (int a = 0; a != 3; a++) {
		const int rad = MC33_gaussian_taps(r->sigma[a], r->radius[a], w[a]);
		if (rad < 0 || !r->stride[a])
			return 0;
		hr.taps[a] = w[a]; hr.ntaps[a] = 2u * (unsigned)rad + 1u; hr.stride[a] = r->stride[a];
	}
	if (mc33hip_resampled_size(sp->slab[0].ctx, &hr, npo) != MC33HIP_OK) /* (fewer than 2 points left on an axis) */
		return 0;
	double step[3];
	for (int j = 0; j != 3; j++) step[j] = sp->grd_d[j] * (double)r->stride[j];
	return create_device_grid_object(sp, npo, step, write_resampled, &hr);
}

/* --- extension: the grid rank-filtered on the device before extraction ------------------------------------------------------------ */
static int write_ranked(mc33hip_ctx *source, const void *arg, void *dst, size_t pitch, size_t slice) {
	return mc33hip_rank_grid(source, (const mc33hip_ranking *)arg, dst, pitch, slice);
}

MC33 *MC33_create_ranked(MC33 *source, const mc33_ranking *r) {
	mc33_private *sp = one_slab(source, mc33hip_rank_grid && mc33hip_context_device && mc33hip_adopt_device);
	if (!sp || !r)
		return 0;
	/* (refused here, before anything is made: the limits of mc33hip_rank_grid) */
	if (r->rank != MC33_RANK_MIN && r->rank != MC33_RANK_MEDIAN && r->rank != MC33_RANK_MAX)
		return 0;
	mc33hip_ranking hr;
	for (int a = 0; a != 3; a++) {
		if (r->radius[a] > (r->rank == MC33_RANK_MEDIAN ? 1u : 8u))
			return 0;
		hr.radius[a] = r->radius[a];
	}
	hr.rank = r->rank; /* (MC33_RANK_* are MC33HIP_RANK_*) */
	const unsigned npo[3] = {source->nx + 1u, source->ny + 1u, source->nz + 1u};
	return create_device_grid_object(sp, npo, sp->grd_d, write_ranked, &hr);
}

_GRD *MC33_resampled_grid(MC33 *M) {
	mc33_private *p = priv(M);
	if (!p || !p->own_grid)
		return 0;
	_GRD *Z = (_GRD *)calloc(1, sizeof(_GRD));
	if (!Z)
		return 0;
	Z->N[0] = M->nx; Z->N[1] = M->ny; Z->N[2] = M->nz;
	for (int i = 0; i != 3; i++) {
		Z->r0[i] = p->grd_r0[i];
		Z->d[i] = p->grd_d[i];
		Z->L[i] = (float)(Z->N[i] * Z->d[i]);
	}
	set_orthogonal(Z);
#ifndef GRD_ORTHOGONAL
	if (p->inclined) {
		Z->nonortho = 1;
		memcpy(Z->_A, p->grd_A, sizeof Z->_A);
		memcpy(Z->A_, p->grd_Ai, sizeof Z->A_);
	}
#endif
	const size_t npx = (size_t)M->nx + 1, npy = (size_t)M->ny + 1, npz = (size_t)M->nz + 1;
	const size_t plane = (npy - 1) * p->own_pitch + npx; /* samples from a plane's first to its last grid point */
	GRD_data_type *stage = (GRD_data_type *)malloc(plane * sizeof(GRD_data_type));
	int ok = stage && alloc_F(Z) == 0;
	for (size_t k = 0; ok && k != npz; k++) { /* a plane at a time through one block, its rows into the rows of alloc_F */
		void *const to = stage;
		const void *const from = (const GRD_data_type *)p->own_grid + k * p->own_slice;
		const size_t bytes = plane * sizeof(GRD_data_type);
		ok = mc33hip_download_many(p->slab[0].ctx, 1, &to, &from, &bytes, 0) == MC33HIP_OK;
		for (size_t j = 0; ok && j != npy; j++)
			memcpy(Z->F[k][j], stage + j * p->own_pitch, npx * sizeof(GRD_data_type));
	}
	free(stage);
	if (!ok) {
		free_memory_grd(Z);
		return 0;
	}
	return Z;
}

/* --- extension: the contour spectrum of the grid, one pass per slab ------------------------------------------------------------------ */
int MC33_isovalue_ladder(double lo, double hi, unsigned n, MC33_real *out) {
	if (!out || n > 255u || !(lo >= -DBL_MAX && lo <= DBL_MAX) || !(hi >= -DBL_MAX && hi <= DBL_MAX) || !(lo < hi))
		return -1;
	for (unsigned k = 0; k != n; k++) {
		out[k] = (MC33_real)(lo + (hi - lo) * ((double)(k + 1u) / (double)(n + 1u)));
		if (k && !(out[k - 1u] < out[k])) /* (steps closer than MC33_real resolves) */
			return -1;
	}
	return (int)n;
}

static void *slab_spectrum(void *arg) {
	mc33_slab *s = (mc33_slab *)arg;
	mc33hip_range r;
	r.z_begin = s->z_begin; r.z_end = s->z_end; r.ghost_below = 0; r.id_base = 0;
	s->rc = mc33hip_grid_spectrum(s->ctx, &r, s->spectrum);
	return 0;
}

int MC33_grid_spectrum(MC33 *M, const MC33_real *isovalues, unsigned count, unsigned long long *cut_cells, unsigned long long *histogram,
                       mc33_spectrum_info *info) {
	mc33_private *p = priv(M);
	if (!p || !mc33hip_grid_spectrum || count > 255u || !histogram || (count && (!isovalues || !cut_cells)))
		return -1;
	/* every slab's struct, the isovalues as doubles and every slab's two arrays in one block */
	const size_t ns = (size_t)p->nslab, words = 2u * (size_t)count + 1u;
	char *blk = (char *)malloc(ns * sizeof(mc33hip_spectrum) + 256u * sizeof(double) + ns * words * sizeof(unsigned long long));
	if (!blk)
		return -1;
	mc33hip_spectrum *sp = (mc33hip_spectrum *)blk;
	double *iso = (double *)(sp + ns);
	unsigned long long *w = (unsigned long long *)(iso + 256);
	for (unsigned k = 0; k != count; k++) iso[k] = (double)isovalues[k];
	for (size_t k = 0; k != ns; k++) {
		memset(&sp[k], 0, sizeof sp[k]);
		sp[k].isos = iso; sp[k].n = count;
		sp[k].cut_cells = w + k * words; sp[k].histogram = w + k * words + count;
		p->slab[k].spectrum = &sp[k];
	}
	int rc = refresh_grid(p); /* (samples the caller said it rewrote: uploaded first, as before a count) */
	if (rc == MC33HIP_OK) rc = run_slabs(p, slab_spectrum);
	for (size_t k = 0; k != ns; k++) p->slab[k].spectrum = 0;
	if (rc == MC33HIP_OK) { /* integers add, extremes combine; nothing is written on failure */
		mc33_spectrum_info t;
		memset(&t, 0, sizeof t);
		t.sample_min = sp[0].sample_min; t.sample_max = sp[0].sample_max;
		for (unsigned j = 0; j != count; j++) cut_cells[j] = 0;
		for (unsigned j = 0; j <= count; j++) histogram[j] = 0;
		for (size_t k = 0; k != ns; k++) {
			for (unsigned j = 0; j != count; j++) cut_cells[j] += sp[k].cut_cells[j];
			for (unsigned j = 0; j <= count; j++) histogram[j] += sp[k].histogram[j];
			t.points += sp[k].points; t.cells += sp[k].cells; t.nan_samples += sp[k].nan_samples;
			if (sp[k].sample_min < t.sample_min) t.sample_min = sp[k].sample_min;
			if (sp[k].sample_max > t.sample_max) t.sample_max = sp[k].sample_max;
		}
		if (info) *info = t;
	}
	free(blk);
	return rc == MC33HIP_OK ? 0 : -1;
}
