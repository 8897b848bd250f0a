// rt0_kernels.hip -- ahead-of-time kernel instances for gfx950.
//
// The integrator itself is rt0_integrator.h.  These instances read the scene
// from HBM (DynScene) and the flags/constants from kernel arguments (DynCfg);
// the scene-specialised instance is compiled at run time by rt0_jit.cpp.
// Five instances: Cornell-class, +SDF, +volumetrics/spectral, +ReSTIR, and the
// event-counting instance used for the FLOP model; each is its own translation
// unit (rt0_pass_inst.hip, built once per RT0_VARIANT) so they compile in
// parallel.  This file holds the small kernels and the launcher table.
#include "rt0_integrator.h"

using namespace rt0;


// frame-chunked launches: ordered sum of the per-frame samples (HBM-bound,
// 16 B/sample read + 32 B/pixel)
__global__ __launch_bounds__(256) void rt0_sum_kernel(const LaunchParams P) { sum_body(P); }

// Display epilogue, written to an RGBA8 canvas.  mode 0 = the reference's
// tonemapper.glsl:28-33, pow(acc * u_cont, 1/2.2).  Modes 1/2 are not used by
// the reference (parity unpinned): 1 = its unused ACESFilm (17-26) on
// exposure 1.5 (12), 2 = the Reinhard curve the README claims (README:22).
__global__ __launch_bounds__(256) void rt0_tonemap_kernel(const float4 *__restrict__ acc, uchar4 *__restrict__ out,
                                                          int n, float cont, int mode) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 a = acc[i];
  auto g = [&](float x) {
    x = x * cont;
    if (mode == 1) {
      x *= 1.5f;
      x = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    } else if (mode == 2) {
      x = x / (1.0f + x);
    }
    float v = __powf(fmaxf(x, 0.0f), 1.0f / 2.2f);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (unsigned char)(v * 255.0f + 0.5f);
  };
  out[i] = make_uchar4(g(a.x), g(a.y), g(a.z), 255);
}

// Ray queries of the triangle path (rt0_trace_rays, a test hook): one lane
// per ray in blocks of 256 (BvhStack's stride).  mode 0 = bvh_closest, 1 =
// bvh_closest<true> (occlusion), 2 = every triangle in leaf order through the
// same tri_test with no boxes: what the walk has to reproduce.  1/d as the
// integrator's call sites take it (frcp per component).
__global__ __launch_bounds__(256) void rt0_trace_kernel(const LaunchParams P, int n, const float *__restrict__ org,
                                                        const float *__restrict__ dir,
                                                        const float *__restrict__ tmax, int mode,
                                                        float *__restrict__ t_out, int32_t *__restrict__ tri_out) {
  treelet_load(P);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const v3 o = mk(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
  const v3 d = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
  float tmin = tmax ? tmax[i] : INF_T;
  int best = -1;
  if (mode == 2) {
    for (int k = 0; k < P.n_tris; k++) {
      float t;
      if (tri_test(P.tris[k], o, d, tmin, t)) {
        tmin = t;
        best = k;
      }
    }
  } else {
    const v3 m = mk(frcp(d.x), frcp(d.y), frcp(d.z));
    best = mode == 1 ? bvh_closest<true>(P, o, d, m, tmin) : bvh_closest<false>(P, o, d, m, tmin);
  }
  t_out[i] = tmin;
  tri_out[i] = best;
}

// ------------------------------------------------------------ launchers
extern "C" hipError_t rt0_launch_pass_v0(const LaunchParams *, dim3, hipStream_t);
extern "C" hipError_t rt0_launch_pass_v1(const LaunchParams *, dim3, hipStream_t);
extern "C" hipError_t rt0_launch_pass_v2(const LaunchParams *, dim3, hipStream_t);
extern "C" hipError_t rt0_launch_pass_v3(const LaunchParams *, dim3, hipStream_t);
extern "C" hipError_t rt0_launch_pass_v4(const LaunchParams *, dim3, hipStream_t);

extern "C" hipError_t rt0_launch_pass(int variant, const LaunchParams *p, dim3 grid, hipStream_t stream) {
  switch (variant) {
    case 0: return rt0_launch_pass_v0(p, grid, stream);
    case 1: return rt0_launch_pass_v1(p, grid, stream);
    case 2: return rt0_launch_pass_v2(p, grid, stream);
    case 3: return rt0_launch_pass_v3(p, grid, stream);
    case 4: return rt0_launch_pass_v4(p, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

extern "C" hipError_t rt0_launch_sum(const LaunchParams *p, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(rt0_sum_kernel, dim3(grid.x, grid.y), dim3(256), 0, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt0_launch_trace(const LaunchParams *p, int n, const float *org, const float *dir,
                                       const float *tmax, int mode, float *t_out, int32_t *tri_out,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(rt0_trace_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *p, n, org, dir, tmax, mode, t_out,
                     tri_out);
  return hipGetLastError();
}

extern "C" hipError_t rt0_launch_tonemap(const float4 *acc, uchar4 *out, int n, float cont, int mode,
                                         hipStream_t stream) {
  hipLaunchKernelGGL(rt0_tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, acc, out, n, cont, mode);
  return hipGetLastError();
}
