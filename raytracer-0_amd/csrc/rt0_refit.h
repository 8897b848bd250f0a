// rt0_refit.h -- what the BVH refit keeps on the device (rt0_refit.hip) and
// the host-side height order it runs in (rt0_refit_order.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "rt0_device.h"

// One TRIANGLE instance as build_bvh (rt0_host.cpp) reads it: world vertex =
// pos + scale * p, two roundings.  32 B.
struct RefitInst {
  float px, py, pz, scale;  // Mesh.pos, joker.x
  int32_t cull;             // Material.opts[3]
  int32_t pad0, pad1, pad2;
};

// The resident inputs of a refit, all device pointers.  Passed to the kernels
// by value.
struct RefitDev {
  const float *pos;       // object-space positions of every instanced model, one after the other (3 floats each)
  const int32_t *idx;     // their triangles: 3 indices into pos each (the model's first vertex added)
  const int2 *leaf;       // per leaf-order triangle: x = model k, y = triangle in idx
  const RefitInst *inst;  // per model k
  const int32_t *order;   // inner nodes grouped by height (bvh_height_order)
  BvhNode *nodes;
  TriDev *tris;
  int32_t n_tris;
  int32_t host_eps;  // TriDev::eps as the host builder rounds it (no FMA), not as k_pack does
};

// Pass 1 (every TriDev from the resident positions) and pass 2 (the boxes,
// one launch per height group: group g is order[group_off[g], group_off[g + 1]))
// on stream s.  Nothing is allocated, nothing waits.
extern "C" hipError_t rt0_refit_launch(const RefitDev *r, const int32_t *group_off, int n_groups, hipStream_t s);

namespace rt0h {
// Heights of a finished tree of n_tris leaves (max(1, n_tris - 1) BvhNodes,
// either builder, any numbering): a node whose children are both leaves has
// height 0, any other 1 + its higher inner child.  order = the nodes sorted
// by height (by index within one height), group_off[h] = where height h
// starts in it (group_off.back() = the node count); parent[i] = the node
// holding the link to i (-1 for the root), height[i] as above.  Returns false
// for anything that is not one tree rooted at node 0 with every leaf linked
// once (a one-triangle tree: twice, by the root): a link out of range, a node
// or leaf linked twice or never, a cycle.
bool bvh_height_order(const BvhNode *nodes, int n_tris, std::vector<int32_t> &order, std::vector<int32_t> &group_off,
                      std::vector<int32_t> &parent, std::vector<int32_t> &height);
}  // namespace rt0h
