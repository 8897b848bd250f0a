// rt0_refit.hip -- BVH refit on gfx950: new vertex positions into the same tree.
//
// rt0_update_model* (rt0_host.cpp) keeps the tree's links and leaf order and
// recomputes, from the resident object-space positions (RefitDev),
//   pass 1  k_refit_tris   one lane per leaf-order triangle: its TriDev, formed
//                          as bvh_build_sah and k_pack (rt0_bvh.hip) form it;
//   pass 2  k_refit_nodes  one lane per inner node of one height: the box of a
//                          leaf child is the min/max of that triangle's three
//                          world vertices, the box of an inner child the union
//                          of that child's two boxes.  A lane writes the three
//                          box quads of its own 64-B record and reads records
//                          of smaller height only, written by earlier launches:
//                          the kernel boundary is the only synchronisation, no
//                          counter, no fence, no hand-off inside a launch.
// World vertex = pos + scale * p with the product and the sum rounded
// separately (a contract(off) block), which is what the host's gather in
// build_bvh computes: a refit with unchanged positions rewrites the bytes a
// build wrote.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt0_refit.h"

namespace {

struct WorldTri {
  float v[9];
};

__device__ __forceinline__ WorldTri world_tri(const RefitDev &r, int leaf, RefitInst &inst, int32_t &model) {
  // two roundings, as the host's `pos + scale * p`: written as plain * and +
  // in a contract(off) block (__fmul_rn / __fadd_rn are plain operators in the
  // HIP headers, outside this block's reach, and -ffp-contract fuses them)
#pragma clang fp contract(off)
  const int2 src = r.leaf[leaf];
  model = src.x;
  inst = r.inst[src.x];
  const int32_t *t = r.idx + 3 * (size_t)src.y;
  WorldTri w;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float *p = r.pos + 3 * (size_t)t[j];
    const float sx = inst.scale * p[0], sy = inst.scale * p[1], sz = inst.scale * p[2];
    w.v[3 * j + 0] = inst.px + sx;
    w.v[3 * j + 1] = inst.py + sy;
    w.v[3 * j + 2] = inst.pz + sz;
  }
  return w;
}

// TriDev::eps as the tree's builder rounds it, so that a refit of unchanged
// positions is a no-op on these bytes too: k_pack's expression under the
// build's contraction (the device LBVH), or bvh_build_sah's on the host, which
// has no FMA -- the two differ by up to 2 ulp
__device__ __forceinline__ float eps_as_k_pack(const TriDev &d) {
  return 0.001f * sqrtf(d.e0x * d.e0x + d.e0y * d.e0y + d.e0z * d.e0z) *
         sqrtf(d.e1x * d.e1x + d.e1y * d.e1y + d.e1z * d.e1z);
}
__device__ __forceinline__ float eps_as_host(const TriDev &d) {
#pragma clang fp contract(off)
  const float a = d.e0x * d.e0x + d.e0y * d.e0y + d.e0z * d.e0z;
  const float b = d.e1x * d.e1x + d.e1y * d.e1y + d.e1z * d.e1z;
  return 0.001f * sqrtf(a) * sqrtf(b);  // (sqrtf is correctly rounded on both sides)
}

template <bool kHostEps>
__global__ void k_refit_tris(RefitDev r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.n_tris) return;
  RefitInst inst;
  int32_t model;
  const WorldTri w = world_tri(r, i, inst, model);
  const float *t = w.v;
  TriDev d;
  d.v0x = t[0];
  d.v0y = t[1];
  d.v0z = t[2];
  d.model = model;
  d.e0x = t[3] - t[0];
  d.e0y = t[4] - t[1];
  d.e0z = t[5] - t[2];
  d.cull = inst.cull;
  d.e1x = t[6] - t[0];
  d.e1y = t[7] - t[1];
  d.e1z = t[8] - t[2];
  d.eps = kHostEps ? eps_as_host(d) : eps_as_k_pack(d);
  float4 *out = reinterpret_cast<float4 *>(r.tris + i);  // 48 B: three 16-B stores
  out[0] = make_float4(d.v0x, d.v0y, d.v0z, __int_as_float(d.model));
  out[1] = make_float4(d.e0x, d.e0y, d.e0z, __int_as_float(d.cull));
  out[2] = make_float4(d.e1x, d.e1y, d.e1z, d.eps);
}

struct Box {
  float x0, y0, z0, x1, y1, z1;
};

__device__ __forceinline__ Box child_box(const RefitDev &r, int32_t link) {
  Box b;
  if (link < 0) {  // a leaf: the triangle's own vertices (not v0 + e0, which rounds again)
    RefitInst inst;
    int32_t model;
    const WorldTri w = world_tri(r, ~link, inst, model);
    const float *t = w.v;
    b.x0 = fminf(t[0], fminf(t[3], t[6]));
    b.y0 = fminf(t[1], fminf(t[4], t[7]));
    b.z0 = fminf(t[2], fminf(t[5], t[8]));
    b.x1 = fmaxf(t[0], fmaxf(t[3], t[6]));
    b.y1 = fmaxf(t[1], fmaxf(t[4], t[7]));
    b.z1 = fmaxf(t[2], fmaxf(t[5], t[8]));
  } else {  // an inner node of smaller height: an earlier launch wrote its record
    const float4 *c = reinterpret_cast<const float4 *>(r.nodes + link);
    const float4 c0 = c[0], c1 = c[1], c2 = c[2];  // lx0 ly0 lz0 rx0 | lx1 ly1 lz1 ry0 | rz0 rx1 ry1 rz1
    b.x0 = fminf(c0.x, c0.w);
    b.y0 = fminf(c0.y, c1.w);
    b.z0 = fminf(c0.z, c2.x);
    b.x1 = fmaxf(c1.x, c2.y);
    b.y1 = fmaxf(c1.y, c2.z);
    b.z1 = fmaxf(c1.z, c2.w);
  }
  return b;
}

// the nodes order[first, first + count): one height
__global__ void k_refit_nodes(RefitDev r, int first, int count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const int32_t node = r.order[first + j];
  float4 *rec = reinterpret_cast<float4 *>(r.nodes + node);
  const int4 links = reinterpret_cast<const int4 *>(rec)[3];  // left, right, pad, pad: not rewritten
  const Box l = child_box(r, links.x), q = child_box(r, links.y);
  rec[0] = make_float4(l.x0, l.y0, l.z0, q.x0);
  rec[1] = make_float4(l.x1, l.y1, l.z1, q.y0);
  rec[2] = make_float4(q.z0, q.x1, q.y1, q.z1);
}

}  // namespace

extern "C" hipError_t rt0_refit_launch(const RefitDev *r, const int32_t *group_off, int n_groups, hipStream_t s) {
  if (!r || !group_off || r->n_tris <= 0 || n_groups <= 0) return hipErrorInvalidValue;
  const int B = 256;
  if (r->host_eps)
    hipLaunchKernelGGL(k_refit_tris<true>, dim3((r->n_tris + B - 1) / B), dim3(B), 0, s, *r);
  else
    hipLaunchKernelGGL(k_refit_tris<false>, dim3((r->n_tris + B - 1) / B), dim3(B), 0, s, *r);
  hipError_t e = hipGetLastError();
  for (int g = 0; g < n_groups && e == hipSuccess; g++) {
    const int first = group_off[g], count = group_off[g + 1] - first;
    if (count <= 0) continue;
    hipLaunchKernelGGL(k_refit_nodes, dim3((count + B - 1) / B), dim3(B), 0, s, *r, first, count);
    e = hipGetLastError();
  }
  return e;
}
