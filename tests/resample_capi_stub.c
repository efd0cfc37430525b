/* MC33_create_resampled / MC33_resampled_grid / free_MC33 of csrc/mc33_capi.c - the host layer as it ships - on a stub device layer
 * whose "device memory" is the heap: what the host layer does with contexts and with the grid it owns, checked without a GPU.
 * Test infrastructure (tests/test_resample_cpu.py builds and runs it); a stand-alone program, so that it can also be built with
 * -fsanitize=address,undefined by hand.
 *
 * The stub keeps a table of live contexts and of live allocations.  Every entry point that takes a context refuses a dead one
 * loudly (exit 3) - under a sanitizer the freed block is caught before that -, mc33hip_destroy of a context that still has the
 * program's resampled grid allocated through it, or an allocation left at the end, fails the run.  mc33hip_resample_grid of the
 * stub ignores the taps and keeps every stride-th sample: enough to see that the right buffers, pitches and sizes travel. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/marching_cubes_33.h"
#include "../include/mc33_hip.h"

struct mc33hip_ctx {
	mc33hip_grid_desc desc;
	int device;
	GRD_data_type *grid; /* own copy (upload_rows) or adopted */
	int owns;
	size_t pitch, slice;
};

#define MAXN 64
static mc33hip_ctx *g_live[MAXN];
static void *g_alloc[MAXN];
static mc33hip_ctx *g_alloc_ctx[MAXN];
static int g_current_device = 0; /* what "-1" resolves to */

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
int mc33hip_device_count(void) { return 4; }
int mc33hip_create(mc33hip_ctx **out, const mc33hip_grid_desc *d) {
	mc33hip_ctx *c = (mc33hip_ctx *)calloc(1, sizeof *c);
	c->desc = *d;
	c->device = d->device >= 0 ? d->device : g_current_device;
	for (int k = 0; k != MAXN; k++)
		if (!g_live[k]) { g_live[k] = c; *out = c; return 0; }
	die("too many contexts");
	return -1;
}
void mc33hip_destroy(mc33hip_ctx *c) {
	if (!c) return;
	alive(c, "mc33hip_destroy");
	for (int k = 0; k != MAXN; k++)
		if (g_alloc[k] && g_alloc_ctx[k] == c) die("mc33hip_destroy of a context that still has an allocation made through it");
	if (c->owns) free(c->grid);
	for (int k = 0; k != MAXN; k++)
		if (g_live[k] == c) g_live[k] = 0;
	memset(c, 0xDD, sizeof *c);
	free(c);
}
int mc33hip_context_device(mc33hip_ctx *c) { alive(c, "mc33hip_context_device"); return c->device; }
int mc33hip_set_normal_neg(mc33hip_ctx *c, int on) { (void)on; alive(c, "mc33hip_set_normal_neg"); return 0; }
int mc33hip_own_stream(mc33hip_ctx *c) { alive(c, "mc33hip_own_stream"); return 0; }
int mc33hip_set_inclined(mc33hip_ctx *c, const double *A, const double *Ai, int t) { (void)A; (void)Ai; (void)t; alive(c, "mc33hip_set_inclined"); return 0; }
int mc33hip_synchronize(mc33hip_ctx *c) { alive(c, "mc33hip_synchronize"); return 0; }
int mc33hip_download_wait(mc33hip_ctx *c) { alive(c, "mc33hip_download_wait"); return 0; }
int mc33hip_set_id_base(mc33hip_ctx *c, unsigned b) { (void)b; alive(c, "mc33hip_set_id_base"); return 0; }
int mc33hip_upload_rows(mc33hip_ctx *c, const void *const *const *F) {
	alive(c, "mc33hip_upload_rows");
	const size_t npx = c->desc.npx, npy = c->desc.npy, npz = c->desc.npz_resident;
	if (!c->owns) { c->grid = (GRD_data_type *)malloc(npx * npy * npz * sizeof(GRD_data_type)); c->owns = 1; }
	c->pitch = npx; c->slice = npx * npy;
	for (size_t k = 0; k != npz; k++)
		for (size_t j = 0; j != npy; j++) memcpy(c->grid + k * c->slice + j * c->pitch, F[k][j], npx * sizeof(GRD_data_type));
	return 0;
}
int mc33hip_adopt_device(mc33hip_ctx *c, const void *p, size_t pitch, size_t slice) {
	alive(c, "mc33hip_adopt_device");
	if (c->owns) free(c->grid);
	c->grid = (GRD_data_type *)p; c->owns = 0; c->pitch = pitch; c->slice = slice;
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
		if (!g_alloc[k]) { g_alloc[k] = *p = malloc(bytes); memset(*p, 0xEE, bytes); g_alloc_ctx[k] = c; return 0; }
	return MC33HIP_ENOMEM;
}
int mc33hip_device_free(mc33hip_ctx *c, void *p) {
	alive(c, "mc33hip_device_free");
	for (int k = 0; k != MAXN; k++)
		if (g_alloc[k] == p) { free(p); g_alloc[k] = 0; return 0; }
	die("mc33hip_device_free of a pointer that is not allocated");
	return -1;
}
int mc33hip_resampled_size(mc33hip_ctx *c, const mc33hip_resampling *r, unsigned np_out[3]) {
	alive(c, "mc33hip_resampled_size");
	const unsigned np[3] = {c->desc.npx, c->desc.npy, c->desc.npz_resident};
	for (int a = 0; a != 3; a++) {
		if (!r->stride[a] || (r->taps[a] && (!(r->ntaps[a] & 1u) || r->ntaps[a] > 17u))) return MC33HIP_EINVAL;
		np_out[a] = (np[a] - 1u) / r->stride[a] + 1u;
		if (np_out[a] < 2u) return MC33HIP_EINVAL;
	}
	return 0;
}
int mc33hip_resample_grid(mc33hip_ctx *c, const mc33hip_resampling *r, void *dst, size_t pitch, size_t slice) {
	unsigned n[3];
	if (mc33hip_resampled_size(c, r, n)) return MC33HIP_EINVAL;
	if (!c->grid || !dst || pitch < n[0] || slice < pitch * n[1]) return MC33HIP_EINVAL;
	GRD_data_type *o = (GRD_data_type *)dst;
	for (size_t z = 0; z != n[2]; z++)
		for (size_t y = 0; y != n[1]; y++)
			for (size_t x = 0; x != n[0]; x++)
				o[z * slice + y * pitch + x] = c->grid[z * r->stride[2] * c->slice + y * r->stride[1] * c->pitch + x * r->stride[0]];
	return 0;
}

/* ---- the program ------------------------------------------------------------------------------------------------------------------ */
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static int same_as_strided(const _GRD *Z, const GRD_data_type *data, unsigned nx, unsigned ny, const unsigned s[3]) {
	for (unsigned k = 0; k <= Z->N[2]; k++)
		for (unsigned j = 0; j <= Z->N[1]; j++)
			for (unsigned i = 0; i <= Z->N[0]; i++)
				if (Z->F[k][j][i] != data[((size_t)k * s[2] * ny + (size_t)j * s[1]) * nx + (size_t)i * s[0]]) return 0;
	return 1;
}

int main(void) {
	enum { NX = 11, NY = 9, NZ = 7 };
	static GRD_data_type data[NZ * NY * NX];
	for (int k = 0; k != NZ * NY * NX; k++) data[k] = (GRD_data_type)(k % 251);
	_GRD *G = grid_from_data_pointer(NX, NY, NZ, data);
	CHECK(G);
	G->d[0] = 0.5; G->d[1] = 0.25; G->d[2] = 2.0; G->r0[0] = 1.0;
	g_current_device = 2;
	MC33 *M = create_MC33(G);
	CHECK(M);
	g_current_device = 0; /* the caller has moved on to another device since */
	mc33_resampling rs = {{0.0, 1.0, 0.0}, {0, 0, 0}, {2, 1, 3}};
	MC33 *R = MC33_create_resampled(M, &rs);
	CHECK(R && R->nx == 5 && R->ny == 8 && R->nz == 2 && !R->F);
	CHECK(R->O[0] == (MC33_real)1.0 && R->D[0] == (MC33_real)1.0 && R->D[1] == (MC33_real)0.25 && R->D[2] == (MC33_real)6.0);
	for (int k = 0, seen = 0; k != MAXN; k++) /* both contexts on the device the source's context resolved */
		if (g_live[k]) { CHECK(g_live[k]->device == 2); CHECK(++seen <= 2); }
	/* refused structs: NULL, nothing allocated, the source as it was */
	mc33_resampling bad[4] = {{{-1.0, 0, 0}, {0, 0, 0}, {1, 1, 1}}, {{3.0, 0, 0}, {0, 0, 0}, {1, 1, 1}}, {{0, 0, 0}, {0, 0, 0}, {1, 0, 1}}, {{0, 0, 0}, {0, 0, 0}, {NX, 1, 1}}};
	for (int k = 0; k != 4; k++) CHECK(!MC33_create_resampled(M, &bad[k]));
	CHECK(!MC33_create_resampled(M, 0) && !MC33_resampled_grid(M));
	free_MC33(M); /* the source goes first */
	free_memory_grd(G);
	_GRD *Z = MC33_resampled_grid(R);
	CHECK(Z && Z->N[0] == 5 && Z->N[1] == 8 && Z->N[2] == 2 && Z->r0[0] == 1.0 && Z->d[0] == 1.0 && Z->d[2] == 6.0 && Z->internal_data == 1);
	const unsigned s1[3] = {2, 1, 3};
	CHECK(same_as_strided(Z, data, NX, NY, s1));
	free_memory_grd(Z);
	mc33_resampling rs2 = {{0.0, 0.0, 0.0}, {0, 0, 0}, {1, 2, 1}};
	MC33 *R2 = MC33_create_resampled(R, &rs2); /* a resampled object resampled again */
	CHECK(R2 && R2->ny == 4 && R2->D[1] == (MC33_real)0.5);
	MC33_grid_changed(R); /* nothing to upload: no host grid */
	surface *S = calculate_isosurface(R, (MC33_real)10);
	CHECK(S && S->nV == 0);
	free_surface_memory(S);
	free_MC33(R);
	Z = MC33_resampled_grid(R2);
	const unsigned s2[3] = {2, 2, 3};
	CHECK(Z && same_as_strided(Z, data, NX, NY, s2));
	free_memory_grd(Z);
	free_MC33(R2);
	for (int k = 0; k != MAXN; k++) CHECK(!g_live[k] && !g_alloc[k]); /* every context destroyed, every allocation released */
	puts("ok");
	return 0;
}
