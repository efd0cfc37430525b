/* MC33_grid_spectrum of csrc/mc33_capi.c - the host layer as it ships - on a stub device layer whose "device memory" is the heap,
 * with the grid spread over THREE slabs (MC33_HIP_DEVICES=0,0,0): that the slabs' ranges tile the grid, that the integers are
 * added and the extremes combined, that a grid marked as changed is uploaded first, and that a failing slab gives -1, writes
 * nothing and leaves nothing allocated.  Test infrastructure (tests/test_spectrum_cpu.py builds and runs it); a stand-alone
 * program, so that it can also be built with -fsanitize=address,undefined.
 *
 * mc33hip_grid_spectrum of the stub is the definition of include/mc33_hip.h written out cell by cell and point by point - a
 * linear scan for the rank, nothing of the kernel's - over the planes the context holds; it refuses a range whose planes are not
 * resident, records every range it is asked for, and fails on the call whose number is g_fail_call. */
#define _POSIX_C_SOURCE 200809L /* setenv */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/marching_cubes_33.h"
#include "../include/mc33_hip.h"

struct mc33hip_ctx {
	mc33hip_grid_desc desc;
	GRD_data_type *grid;
	size_t pitch, slice;
	int uploads;
};

#define MAXN 64
static mc33hip_ctx *g_live[MAXN];
static void *g_alloc[MAXN];
static mc33hip_range g_asked[MAXN];
static int g_calls, g_fail_call = -1;

static void die(const char *what) {
	fprintf(stderr, "stub device layer: %s\n", what);
	exit(3);
}
static void alive(mc33hip_ctx *c, const char *fn) {
	for (int k = 0; k != MAXN; k++)
		if (c && g_live[k] == c) return;
	fprintf(stderr, "stub device layer: %s called with a context that is not alive\n", fn);
	exit(3);
}

const char *mc33hip_last_error(void) { return ""; }
int mc33hip_device_count(void) { return 1; }
int mc33hip_create(mc33hip_ctx **out, const mc33hip_grid_desc *d) {
	mc33hip_ctx *c = (mc33hip_ctx *)calloc(1, sizeof *c);
	c->desc = *d;
	for (int k = 0; k != MAXN; k++)
		if (!g_live[k]) { g_live[k] = c; *out = c; return 0; }
	die("too many contexts");
	return -1;
}
void mc33hip_destroy(mc33hip_ctx *c) {
	if (!c) return;
	alive(c, "mc33hip_destroy");
	free(c->grid);
	for (int k = 0; k != MAXN; k++)
		if (g_live[k] == c) g_live[k] = 0;
	free(c);
}
int mc33hip_set_normal_neg(mc33hip_ctx *c, int on) { (void)on; alive(c, "mc33hip_set_normal_neg"); return 0; }
int mc33hip_own_stream(mc33hip_ctx *c) { alive(c, "mc33hip_own_stream"); return 0; }
int mc33hip_set_inclined(mc33hip_ctx *c, const double *A, const double *Ai, int t) { (void)A; (void)Ai; (void)t; alive(c, "mc33hip_set_inclined"); return 0; }
int mc33hip_synchronize(mc33hip_ctx *c) { alive(c, "mc33hip_synchronize"); return 0; }
int mc33hip_download_wait(mc33hip_ctx *c) { alive(c, "mc33hip_download_wait"); return 0; }
int mc33hip_set_id_base(mc33hip_ctx *c, unsigned b) { (void)b; alive(c, "mc33hip_set_id_base"); return 0; }
int mc33hip_upload_rows(mc33hip_ctx *c, const void *const *const *F) {
	alive(c, "mc33hip_upload_rows");
	const size_t npx = c->desc.npx, npy = c->desc.npy, npz = c->desc.npz_resident;
	if (!c->grid) c->grid = (GRD_data_type *)malloc(npx * npy * npz * sizeof(GRD_data_type));
	c->pitch = npx; c->slice = npx * npy;
	for (size_t k = 0; k != npz; k++)
		for (size_t j = 0; j != npy; j++) memcpy(c->grid + k * c->slice + j * c->pitch, F[k][j], npx * sizeof(GRD_data_type));
	c->uploads++;
	return 0;
}
/* (no surface on this layer: an extraction is an empty one) */
int mc33hip_count(mc33hip_ctx *c, double iso, const mc33hip_range *r, mc33hip_counts *out) { (void)iso; (void)r; alive(c, "mc33hip_count"); memset(out, 0, sizeof *out); return 0; }
int mc33hip_extract(mc33hip_ctx *c, double iso, const mc33hip_range *r, void *V, void *N, void *T, unsigned long long cv, unsigned long long ct, mc33hip_counts *out) {
	(void)iso; (void)r; (void)V; (void)N; (void)T; (void)cv; (void)ct;
	alive(c, "mc33hip_extract"); memset(out, 0, sizeof *out); return 0;
}
int mc33hip_emit(mc33hip_ctx *c, void *V, void *N, void *T, unsigned long long cv, unsigned long long ct) { (void)V; (void)N; (void)T; (void)cv; (void)ct; alive(c, "mc33hip_emit"); return 0; }
int mc33hip_emit_download(mc33hip_ctx *c, void *V, void *N, void *T, unsigned long long cv, unsigned long long ct, void *hV, void *hN, void *hT) {
	(void)V; (void)N; (void)T; (void)cv; (void)ct; (void)hV; (void)hN; (void)hT;
	alive(c, "mc33hip_emit_download"); return 0;
}
int mc33hip_sweep_many(mc33hip_ctx *c, const double *isos, int n, const mc33hip_range *r) { (void)isos; (void)n; (void)r; alive(c, "mc33hip_sweep_many"); return 0; }
int mc33hip_download_many(mc33hip_ctx *c, int n, void *const *dst, const void *const *src, const size_t *bytes, int concurrent) {
	(void)concurrent;
	alive(c, "mc33hip_download_many");
	for (int k = 0; k != n; k++) memcpy(dst[k], src[k], bytes[k]);
	return 0;
}
int mc33hip_device_alloc(mc33hip_ctx *c, void **p, size_t bytes) {
	alive(c, "mc33hip_device_alloc");
	for (int k = 0; k != MAXN; k++)
		if (!g_alloc[k]) { g_alloc[k] = *p = malloc(bytes); return 0; }
	return MC33HIP_ENOMEM;
}
int mc33hip_device_free(mc33hip_ctx *c, void *p) {
	alive(c, "mc33hip_device_free");
	for (int k = 0; k != MAXN; k++)
		if (g_alloc[k] == p) { free(p); g_alloc[k] = 0; return 0; }
	die("mc33hip_device_free of a pointer that is not allocated");
	return -1;
}

static unsigned rank_of(const MC33_real *iso, unsigned n, MC33_real r) {
	if (r != r) return signbit(r) ? n : 0u;
	unsigned k = 0;
	while (k != n && iso[k] < r) k++;
	return k;
}
static unsigned rank_at(const mc33hip_ctx *c, const MC33_real *iso, unsigned n, unsigned x, unsigned y, unsigned z) {
	return rank_of(iso, n, (MC33_real)c->grid[(size_t)(z - c->desc.plane0) * c->slice + (size_t)y * c->pitch + x]);
}
int mc33hip_grid_spectrum(mc33hip_ctx *c, const mc33hip_range *r, mc33hip_spectrum *s) {
	alive(c, "mc33hip_grid_spectrum");
	if (g_calls < MAXN) g_asked[g_calls] = *r;
	if (g_calls++ == g_fail_call) return MC33HIP_ERUNTIME;
	const mc33hip_grid_desc *d = &c->desc;
	if (!s || s->n > 255u || !s->histogram || !(r->z_begin < r->z_end) || r->z_end > d->nz_total || r->z_begin < d->plane0 ||
	    r->z_end > d->plane0 + d->npz_resident - 1u || !c->grid)
		return MC33HIP_EINVAL;
	MC33_real iso[255];
	for (unsigned k = 0; k != s->n; k++) {
		iso[k] = (MC33_real)s->isos[k];
		if (iso[k] != iso[k] || (k && !(iso[k - 1] < iso[k]))) return MC33HIP_EINVAL;
	}
	for (unsigned k = 0; k != s->n; k++) s->cut_cells[k] = 0;
	for (unsigned k = 0; k <= s->n; k++) s->histogram[k] = 0;
	s->points = s->cells = s->nan_samples = 0;
	s->sample_min = INFINITY; s->sample_max = -INFINITY;
	const unsigned top = r->z_end == d->nz_total ? r->z_end + 1u : r->z_end;
	for (unsigned z = r->z_begin; z != top; z++)
		for (unsigned y = 0; y != d->npy; y++)
			for (unsigned x = 0; x != d->npx; x++) {
				const MC33_real v = (MC33_real)c->grid[(size_t)(z - d->plane0) * c->slice + (size_t)y * c->pitch + x];
				s->histogram[rank_of(iso, s->n, v)]++;
				s->points++;
				if (v != v) s->nan_samples++;
				else {
					if ((double)v < s->sample_min) s->sample_min = (double)v;
					if ((double)v > s->sample_max) s->sample_max = (double)v;
				}
			}
	for (unsigned z = r->z_begin; z != r->z_end; z++)
		for (unsigned y = 0; y + 1u != d->npy; y++)
			for (unsigned x = 0; x + 1u != d->npx; x++) {
				unsigned mn = 255u, mx = 0u;
				for (unsigned q = 0; q != 8u; q++) {
					const unsigned k = rank_at(c, iso, s->n, x + (q & 1u), y + ((q >> 1) & 1u), z + (q >> 2));
					if (k < mn) mn = k;
					if (k > mx) mx = k;
				}
				for (unsigned k = mn; k < mx; k++) s->cut_cells[k]++;
				s->cells++;
			}
	return 0;
}

/* ---- the program ------------------------------------------------------------------------------------------------------------------ */
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)
enum { NX = 7, NY = 5, NZ = 11, NISO = 4 };

static GRD_data_type sample(int k) {
#ifdef INTEGER_GRD
	return (GRD_data_type)((k * 37 + (k / 7) * 11) % 200);
#else
	if (k % 29 == 3) return (GRD_data_type)NAN;
	if (k % 31 == 5) return (GRD_data_type)-NAN;
	return (GRD_data_type)(((k * 37 + (k / 7) * 11) % 200) - 100) / (GRD_data_type)4;
#endif
}

int main(void) {
	static GRD_data_type data[NZ * NY * NX];
	for (int k = 0; k != NZ * NY * NX; k++) data[k] = sample(k);
	_GRD *G = grid_from_data_pointer(NX, NY, NZ, data);
	CHECK(G);
#ifdef INTEGER_GRD
	const MC33_real iso[NISO] = {10, 50, 100, 150};
#else
	const MC33_real iso[NISO] = {-20, -5, 0, 12.5f};
#endif
	/* the whole grid on one slab: the answer */
	MC33 *M1 = create_MC33(G);
	CHECK(M1);
	unsigned long long cut1[NISO], hist1[NISO + 1];
	mc33_spectrum_info i1;
	CHECK(MC33_grid_spectrum(M1, iso, NISO, cut1, hist1, &i1) == 0);
	CHECK(g_calls == 1 && g_asked[0].z_begin == 0 && g_asked[0].z_end == NZ - 1);
	CHECK(i1.points == (unsigned long long)NX * NY * NZ && i1.cells == (unsigned long long)(NX - 1) * (NY - 1) * (NZ - 1));
	unsigned long long sum = 0;
	for (int k = 0; k <= NISO; k++) sum += hist1[k];
	CHECK(sum == i1.points);
	free_MC33(M1);

	/* three slabs */
	setenv("MC33_HIP_DEVICES", "0,0,0", 1);
	MC33 *M = create_MC33(G);
	CHECK(M);
	int contexts = 0;
	for (int k = 0; k != MAXN; k++) contexts += g_live[k] != 0;
	CHECK(contexts == 3);
	MC33 before;
	memcpy(&before, M, sizeof before);
	unsigned long long cut[NISO], hist[NISO + 1];
	mc33_spectrum_info info;
	g_calls = 0;
	CHECK(MC33_grid_spectrum(M, iso, NISO, cut, hist, &info) == 0);
	CHECK(g_calls == 3);
	unsigned covered[NZ - 1] = {0}; /* the ranges tile the cell slices: each slice once */
	for (int k = 0; k != 3; k++) {
		CHECK(g_asked[k].z_begin < g_asked[k].z_end && g_asked[k].z_end <= NZ - 1);
		for (unsigned z = g_asked[k].z_begin; z != g_asked[k].z_end; z++) covered[z]++;
	}
	for (int z = 0; z != NZ - 1; z++) CHECK(covered[z] == 1);
	CHECK(!memcmp(cut, cut1, sizeof cut) && !memcmp(hist, hist1, sizeof hist));
	CHECK(info.points == i1.points && info.cells == i1.cells && info.nan_samples == i1.nan_samples);
	CHECK(info.sample_min == i1.sample_min && info.sample_max == i1.sample_max);
	CHECK(!memcmp(&before, M, sizeof before)); /* iso, nV, nT, memoryfault: as they were */
	/* count == 0, info NULL */
	unsigned long long h0 = 7;
	CHECK(MC33_grid_spectrum(M, 0, 0, 0, &h0, 0) == 0 && h0 == i1.points);
	/* a changed grid is uploaded first, on every slab, once */
	int uploads = 0;
	for (int k = 0; k != MAXN; k++) if (g_live[k]) uploads += g_live[k]->uploads;
	data[0] = (GRD_data_type)250;
	data[NZ * NY * NX - 1] = (GRD_data_type)251;
	MC33_grid_changed(M);
	CHECK(MC33_grid_spectrum(M, iso, NISO, cut, hist, &info) == 0);
	int uploads2 = 0;
	for (int k = 0; k != MAXN; k++) if (g_live[k]) uploads2 += g_live[k]->uploads;
	CHECK(uploads2 == uploads + 3 && info.sample_max == 251.0);
	CHECK(MC33_grid_spectrum(M, iso, NISO, cut, hist, &info) == 0);
	for (int k = 0, u = 0; k != MAXN; k++) if (g_live[k]) { u += g_live[k]->uploads; CHECK(u <= uploads2); }
	/* refusals of the host layer: nothing reaches the device layer */
	g_calls = 0;
	const MC33_real down[2] = {2, 1};
	CHECK(MC33_grid_spectrum(0, iso, NISO, cut, hist, &info) == -1 && MC33_grid_spectrum(M, 0, NISO, cut, hist, &info) == -1);
	CHECK(MC33_grid_spectrum(M, iso, NISO, 0, hist, &info) == -1 && MC33_grid_spectrum(M, iso, NISO, cut, 0, &info) == -1);
	CHECK(MC33_grid_spectrum(M, iso, 256, cut, hist, &info) == -1 && g_calls == 0);
	CHECK(MC33_grid_spectrum(M, down, 2, cut, hist, &info) == -1); /* (refused by the device layer, on every slab) */
	/* a failing slab: -1, the outputs as they were, nothing left allocated */
	for (int fail = 0; fail != 3; fail++) {
		unsigned long long cutx[NISO], histx[NISO + 1];
		mc33_spectrum_info infox;
		memset(cutx, 0xAB, sizeof cutx); memset(histx, 0xAB, sizeof histx); memset(&infox, 0xAB, sizeof infox);
		g_calls = 0; g_fail_call = fail;
		CHECK(MC33_grid_spectrum(M, iso, NISO, cutx, histx, &infox) == -1);
		g_fail_call = -1;
		for (size_t k = 0; k != sizeof cutx; k++) CHECK(((unsigned char *)cutx)[k] == 0xAB);
		for (size_t k = 0; k != sizeof histx; k++) CHECK(((unsigned char *)histx)[k] == 0xAB);
		for (size_t k = 0; k != sizeof infox; k++) CHECK(((unsigned char *)&infox)[k] == 0xAB);
		for (int k = 0; k != MAXN; k++) CHECK(!g_alloc[k]);
	}
	CHECK(MC33_grid_spectrum(M, iso, NISO, cut, hist, &info) == 0); /* ... and the object still works */
	CHECK(!memcmp(&before, M, sizeof before));
	free_MC33(M);
	free_memory_grd(G);
	for (int k = 0; k != MAXN; k++) CHECK(!g_live[k] && !g_alloc[k]);
	/* MC33_isovalue_ladder: host C */
	MC33_real out[255];
	CHECK(MC33_isovalue_ladder(0.0, 1.0, 3, out) == 3 && out[0] == (MC33_real)0.25 && out[1] == (MC33_real)0.5 && out[2] == (MC33_real)0.75);
	CHECK(MC33_isovalue_ladder(0.0, 1.0, 0, out) == 0 && MC33_isovalue_ladder(0.0, 1.0, 256, out) == -1 && MC33_isovalue_ladder(1.0, 1.0, 3, out) == -1);
	CHECK(MC33_isovalue_ladder(0.0, (double)INFINITY, 3, out) == -1 && MC33_isovalue_ladder((double)NAN, 1.0, 3, out) == -1 && MC33_isovalue_ladder(0.0, 1.0, 3, 0) == -1);
	puts("ok");
	return 0;
}
