// mc33_property.hip.h -- part of the ONE translation unit mc33_kernels.hip (included there, last; not a header to include elsewhere):
// a second scalar grid ("property grid": the potential painted on a density's isosurface) sampled at the vertices of a finished V
// array - k_property, a pass of its own behind the vertex pass - and the entry points around it (include/mc33_hip.h:
// mc33hip_property_*, mc33hip_sample_property, mc33hip_color_vertices, mc33hip_download_enqueue).  DESIGN.md 9.
//
// The definition (orthogonal grids; everything in IEEE double, no a*b+c fused: -ffp-contract=off), for a vertex v:
//   g[a] = ((double)v[a] - r0[a]) / d[a];  i[a] = floor(g[a]) clamped to [0, N[a]];  f[a] = g[a] - i[a] clamped to [0, 1],
//   0 where i[a] == N[a];  lerp(p, q, f) = f == 0 ? p : p * (1 - f) + q * f, along x on the four rows, then y, then z;
//   the value is that double rounded to float.  Colour: s = ((double)value - lo) / (hi - lo) clamped to [0, 1],
//   palette[(int)floor(s * (n - 1) + 0.5)], a NaN value gets nan_color.
// A vertex on a grid plane does not invert to an integer (a third of them land below their plane), hence the clamps, and hence a
// z-slab's property window reaches one plane beyond each end of its cell slices.

struct PropArgs {
	const sample_t *p;        // first resident plane of the property grid
	uint64_t slice;           // samples per plane / per row
	uint32_t pitch;
	uint32_t plane0, nplanes; // resident window, global plane numbers
	uint32_t N[3];            // cells per axis of the WHOLE grid
	double r0[3], d[3];
	const uint32_t *palette;  // (colours only) n words in device memory
	uint32_t n, nan_color;
	double lo, hi;
	unsigned long long *violations;  // vertices whose sampling needed a plane outside the window
};

__device__ __forceinline__ double prop_lerp(double p, double q, double f) { return f == 0.0 ? p : p * (1.0 - f) + q * f; }

// One lane per vertex, grid stride.  A wave reads 64 rows of V - 768 (1 536) contiguous bytes - with three strided loads per lane:
// every line the wave touches is used whole, by the three loads between them.  The eight samples are loaded unconditionally, all
// in flight together: where the definition does not read a sample (f == 0, which includes i == N) its address is the address of
// the lerp's first operand, so nothing outside the grid or the window is ever touched and no branch separates the loads.  A vertex
// that needs a plane the window lacks is counted, its addresses folded into the window, its result NaN / nan_color.
template <typename R, bool COLOR>
__global__ __launch_bounds__(256) void k_property(PropArgs a, const R *__restrict__ V, uint64_t nV, uint32_t *__restrict__ out) {
	__shared__ uint32_t pal[256];
	if (COLOR) {
		pal[threadIdx.x] = threadIdx.x < a.n ? a.palette[threadIdx.x] : 0u;
		__syncthreads();
	}
	uint32_t bad = 0u;
	for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nV; v += (uint64_t)gridDim.x * 256u) {
		const R *row = V + v * 3u;
		const double x[3] = {(double)row[0], (double)row[1], (double)row[2]};
		uint32_t i[3];
		double f[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const double g = (x[k] - a.r0[k]) / a.d[k];
			const double fl = floor(g), top = (double)a.N[k];
			const double ic = !(fl >= 0.0) ? 0.0 : (fl > top ? top : fl);  // (a NaN coordinate: cell 0, f stays NaN, so does the value)
			double fr = g - ic;
			fr = fr < 0.0 ? 0.0 : (fr > 1.0 ? 1.0 : fr);
			i[k] = (uint32_t)ic;
			f[k] = i[k] == a.N[k] ? 0.0 : fr;
		}
		const uint32_t dx = f[0] != 0.0 ? 1u : 0u, dy = f[1] != 0.0 ? 1u : 0u, dz = f[2] != 0.0 ? 1u : 0u;
		uint32_t k0 = i[2], k1 = i[2] + dz;
		const bool outside = k0 < a.plane0 || k1 >= a.plane0 + a.nplanes;
		if (outside) { bad++; k0 = k1 = a.plane0; }
		const sample_t *r00 = a.p + ((uint64_t)(k0 - a.plane0) * a.slice + (uint64_t)i[1] * a.pitch + i[0]);
		const sample_t *r01 = r00 + (uint64_t)dy * a.pitch;
		const sample_t *r10 = r00 + (uint64_t)(k1 - k0) * a.slice;
		const sample_t *r11 = r10 + (uint64_t)dy * a.pitch;
		const double s000 = (double)r00[0], s001 = (double)r00[dx], s010 = (double)r01[0], s011 = (double)r01[dx];
		const double s100 = (double)r10[0], s101 = (double)r10[dx], s110 = (double)r11[0], s111 = (double)r11[dx];
		const double y00 = prop_lerp(s000, s001, f[0]), y01 = prop_lerp(s010, s011, f[0]);
		const double y10 = prop_lerp(s100, s101, f[0]), y11 = prop_lerp(s110, s111, f[0]);
		const double z0 = prop_lerp(y00, y01, f[1]), z1 = prop_lerp(y10, y11, f[1]);
		const float val = outside ? __builtin_nanf("") : (float)prop_lerp(z0, z1, f[2]);
		if (COLOR) {
			uint32_t col = a.nan_color;
			if (val == val) {
				double s = ((double)val - a.lo) / (a.hi - a.lo);
				s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
				col = pal[(uint32_t)floor(s * (double)(a.n - 1u) + 0.5)];
			}
			out[v] = col;
		} else
			out[v] = __float_as_uint(val);
	}
	if (bad) atomicAdd(a.violations, (unsigned long long)bad);
}

// --- host side ----------------------------------------------------------------------------------------------------------

static void prop_release(mc33hip_ctx *c) {  // (a caller's buffer is let go of, the library's copy released)
	if (c->prop_owned) dev_release(&c->d_prop);
	c->d_prop = nullptr;
	c->prop_owned = false;
	c->prop_cap = 0;
}

static void prop_destroy(mc33hip_ctx *c) {
	prop_release(c);
	dev_release(&c->d_prop_pal); dev_release(&c->d_prop_viol);
	if (c->h_prop_viol) (void)hipHostFree(c->h_prop_viol);
	if (c->ev_prop) (void)hipEventDestroy(c->ev_prop);
}

static int prop_window(mc33hip_ctx *c, unsigned plane0, unsigned nplanes) {
	if (nplanes < 1u || (uint64_t)plane0 + nplanes > (uint64_t)c->desc.nz_total + 1u) { set_err("property planes [%u, %u) exceed the grid", plane0, plane0 + nplanes); return MC33HIP_EINVAL; }
	return 0;
}

// the library's own pitched copy of the window, rows on 16-byte boundaries like the sample grid's (own_pitch)
static int prop_ensure_own(mc33hip_ctx *c, unsigned plane0, unsigned nplanes) {
	const size_t pitch = own_pitch(c->desc.npx), slice = pitch * c->desc.npy, need = slice * nplanes;
	HIP_TRY(hipStreamSynchronize(c->stream));  // (nothing enqueued earlier may still be sampling the old copy)
	if (!c->prop_owned) prop_release(c);
	c->prop_owned = false;
	if (int rc = dev_room("property grid", &c->d_prop, &c->prop_cap, need)) return rc;
	c->prop_owned = true;
	c->prop_pitch = pitch; c->prop_slice = slice;
	c->prop_plane0 = plane0; c->prop_nplanes = nplanes;
	return 0;
}

extern "C" int mc33hip_property_upload_contiguous(mc33hip_ctx *c, const void *host, unsigned int plane0, unsigned int nplanes) {
	if (!c || !host) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = prop_window(c, plane0, nplanes))) return rc;
	if ((rc = prop_ensure_own(c, plane0, nplanes))) return rc;
	const size_t rowb = (size_t)c->desc.npx * sizeof(sample_t);
	if (c->prop_pitch != c->desc.npx && rowb % 4 != 0) {  // (odd-length narrow rows: packed by ourselves, see mc33hip_upload_contiguous)
		const char *h = (const char *)host;
		const size_t npy = c->desc.npy;
		rc = upload_staged(c, [=](uint32_t k, uint32_t j) { return h + ((size_t)k * npy + j) * rowb; }, c->d_prop, nplanes, c->prop_pitch);
		if (rc) prop_release(c);
		return rc;
	}
	const hipError_t e = hipMemcpy2D(c->d_prop, c->prop_pitch * sizeof(sample_t), host, rowb, rowb, (size_t)c->desc.npy * nplanes, hipMemcpyHostToDevice);
	if (e != hipSuccess) { prop_release(c); set_err("property upload failed: %s", hipGetErrorString(e)); return MC33HIP_ERUNTIME; }
	return MC33HIP_OK;
}

extern "C" int mc33hip_property_upload_rows(mc33hip_ctx *c, const void *const *const *F, unsigned int plane0, unsigned int nplanes) {
	if (!c || !F) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = prop_window(c, plane0, nplanes))) return rc;
	const uint32_t npy = c->desc.npy;
	const size_t rowb = (size_t)c->desc.npx * sizeof(sample_t);
	bool contiguous = true;  // (rows back to back: grid_from_data_pointer)
	const char *expect = (const char *)F[0][0];
	for (uint32_t k = 0; k < nplanes && contiguous; k++)
		for (uint32_t j = 0; j < npy; j++, expect += rowb)
			if ((const char *)F[k][j] != expect) { contiguous = false; break; }
	if (contiguous) return mc33hip_property_upload_contiguous(c, F[0][0], plane0, nplanes);
	if ((rc = prop_ensure_own(c, plane0, nplanes))) return rc;
	rc = upload_staged(c, [=](uint32_t k, uint32_t j) { return (const char *)F[k][j]; }, c->d_prop, nplanes, c->prop_pitch);
	if (rc) prop_release(c);
	return rc;
}

extern "C" int mc33hip_property_adopt_device(mc33hip_ctx *c, const void *dptr, size_t pitch, size_t slice, unsigned int plane0, unsigned int nplanes) {
	if (!c || !dptr || pitch < c->desc.npx || slice < pitch * c->desc.npy || pitch > 0xFFFFFFFFull) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if ((rc = prop_window(c, plane0, nplanes))) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	prop_release(c);
	c->d_prop = (sample_t *)dptr;
	c->prop_pitch = pitch; c->prop_slice = slice;
	c->prop_plane0 = plane0; c->prop_nplanes = nplanes;
	return MC33HIP_OK;
}

extern "C" int mc33hip_property_drop(mc33hip_ctx *c) {
	if (!c) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	HIP_TRY(hipStreamSynchronize(c->stream));
	prop_release(c);
	return MC33HIP_OK;
}

// What a synchronising entry point does once the stream has been waited for: the word k_property counts window violations in
// arrives in pinned memory right behind every launch.
static int prop_check(mc33hip_ctx *c) {
	if (!c->prop_pending) return 0;
	c->prop_pending = false;
	const unsigned long long n = *c->h_prop_viol;
	if (!n) return 0;
	*c->h_prop_viol = 0ull;
	HIP_TRY(hipMemsetAsync(c->d_prop_viol, 0, sizeof(unsigned long long), c->stream));
	set_err("property sampling: %llu vertices need a plane outside the attached window [%u, %u)", n, c->prop_plane0, c->prop_plane0 + c->prop_nplanes);
	return MC33HIP_ERUNTIME;
}

// the violation counter with its pinned twin and the palette's 256 words in device memory (mc33hip_color_values stages its palette
// there too): made by the first call that needs them, freed with the context
static int prop_scratch(mc33hip_ctx *c) {
	if (!c->d_prop_viol) {
		HIP_TRY(hipMalloc(&c->d_prop_viol, sizeof(unsigned long long)));
		HIP_TRY(hipMemset(c->d_prop_viol, 0, sizeof(unsigned long long)));
		HIP_TRY(hipHostMalloc(&c->h_prop_viol, sizeof(unsigned long long), hipHostMallocDefault));
		*c->h_prop_viol = 0ull;
		HIP_TRY(hipMalloc(&c->d_prop_pal, 256 * sizeof(uint32_t)));
	}
	return 0;
}

static int prop_enqueue(mc33hip_ctx *c, const void *dV, unsigned long long nV, const int *palette, unsigned n, double lo, double hi, int nan_color, void *out) {
	if (!c || (nV && (!dV || !out))) return MC33HIP_EINVAL;
	if (!c->d_prop) { set_err("no property grid attached"); return MC33HIP_EINVAL; }
	if (c->inclined) { set_err("property sampling is defined for orthogonal grids only"); return MC33HIP_EINVAL; }
	if (palette && (n < 2u || n > 256u || !(lo < hi))) { set_err("colour map needs 2..256 colours and lo < hi"); return MC33HIP_EINVAL; }
	int rc = use_device(c);
	if (rc || (rc = prop_scratch(c))) return rc;
	if (!nV) return MC33HIP_OK;
	PropArgs a;
	a.p = c->d_prop; a.slice = c->prop_slice; a.pitch = (uint32_t)c->prop_pitch;
	a.plane0 = c->prop_plane0; a.nplanes = c->prop_nplanes;
	a.N[0] = c->desc.npx - 1u; a.N[1] = c->desc.npy - 1u; a.N[2] = c->desc.nz_total;
	for (int k = 0; k < 3; k++) { a.r0[k] = c->desc.r0[k]; a.d[k] = c->desc.d[k]; }
	a.palette = c->d_prop_pal; a.n = n; a.nan_color = (uint32_t)nan_color; a.lo = lo; a.hi = hi;
	a.violations = c->d_prop_viol;
	if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
	// A lane per vertex up to 64 blocks per CU, a grid stride beyond.  (With only the eight blocks a CU holds at once - seven or
	// eight vertices per lane at 1024^3 - the kernel took 73 instead of 66 us: the blocks of the last round leave a CU idle one by
	// one, while the dispatcher keeps every CU full of short blocks until the end.  profiles/r07_property.txt)
	const uint32_t grid = (uint32_t)std::min<uint64_t>((nV + 255u) / 256u, (uint64_t)std::max(1, c->cus) * 64u);
	if (palette) {
		HIP_TRY(hipMemcpyAsync(c->d_prop_pal, palette, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL((k_property<real_t, true>), dim3(grid), dim3(256), 0, c->stream, a, (const real_t *)dV, (uint64_t)nV, (uint32_t *)out);
	} else
		hipLaunchKernelGGL((k_property<real_t, false>), dim3(grid), dim3(256), 0, c->stream, a, (const real_t *)dV, (uint64_t)nV, (uint32_t *)out);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(c->h_prop_viol, c->d_prop_viol, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	c->prop_pending = true;
	return MC33HIP_OK;
}

extern "C" int mc33hip_sample_property(mc33hip_ctx *c, const void *dV, unsigned long long nV, float *dP) {
	return prop_enqueue(c, dV, nV, nullptr, 0u, 0.0, 1.0, 0, dP);
}

extern "C" int mc33hip_color_vertices(mc33hip_ctx *c, const void *dV, unsigned long long nV, const int *palette, unsigned int n, double lo, double hi,
                                      int nan_color, int *dC) {
	if (!palette) return MC33HIP_EINVAL;
	return prop_enqueue(c, dV, nV, palette, n, lo, hi, nan_color, dC);
}

extern "C" int mc33hip_download_enqueue(mc33hip_ctx *c, void *host_dst, const void *device_src, size_t bytes) {
	if (!c || (bytes && (!host_dst || !device_src))) return MC33HIP_EINVAL;
	int rc = use_device(c);
	if (rc) return rc;
	if (!bytes) return MC33HIP_OK;
	if (!c->ev_prop) HIP_TRY(hipEventCreateWithFlags(&c->ev_prop, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(c->ev_prop, c->stream));
	HIP_TRY(hipStreamWaitEvent(c->copy, c->ev_prop, 0));
	HIP_TRY(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, c->copy));
	return MC33HIP_OK;
}
