// rt0_refit_order.cpp -- the order a BVH refit visits the inner nodes in.
//
// A refit (rt0_refit.hip) recomputes every box bottom-up.  A node's boxes
// depend on its children's records only, so nodes of one height are
// independent of each other and may run in one launch, heights in ascending
// order.  Parents and heights are derived here from the finished BvhNode array
// -- the form both builders end in, after the treelet renumbering -- so the
// refit knows nothing of how the tree was built.  Host only, no device call.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rt0_internal.h"
#include "rt0_refit.h"

namespace rt0h {

bool bvh_height_order(const BvhNode *nodes, int n_tris, std::vector<int32_t> &order, std::vector<int32_t> &group_off,
                      std::vector<int32_t> &parent, std::vector<int32_t> &height) {
  order.clear();
  group_off.clear();
  parent.clear();
  height.clear();
  if (!nodes || n_tris <= 0) return false;
  const int n = n_tris > 1 ? n_tris - 1 : 1;
  parent.assign((size_t)n, -1);
  height.assign((size_t)n, -1);
  std::vector<uint8_t> leaf_links((size_t)n_tris, 0);
  for (int i = 0; i < n; i++)
    for (int32_t ch : {nodes[i].left, nodes[i].right}) {
      if (ch >= 0) {
        if (ch == 0 || ch >= n || parent[(size_t)ch] >= 0) return false;  // the root, out of range, or a second parent
        parent[(size_t)ch] = i;
      } else {
        const int32_t t = ~ch;
        if (t >= n_tris || leaf_links[(size_t)t] == 2) return false;
        leaf_links[(size_t)t]++;
      }
    }
  for (int t = 0; t < n_tris; t++)
    if (leaf_links[(size_t)t] != (n_tris == 1 ? 2 : 1)) return false;
  // post-order from the root on an explicit stack (a chain is n deep); a node
  // in a cycle has a parent but is never reached from the root
  std::vector<int32_t> stack{0};
  int reached = 0, top = 0;
  while (!stack.empty()) {
    const int32_t i = stack.back();
    const int32_t l = nodes[i].left, r = nodes[i].right;
    if (height[(size_t)i] == -1) {  // first visit: children first
      height[(size_t)i] = -2;
      reached++;
      if (l >= 0) stack.push_back(l);
      if (r >= 0) stack.push_back(r);
      continue;
    }
    stack.pop_back();
    int h = 0;
    if (l >= 0) h = std::max(h, 1 + height[(size_t)l]);
    if (r >= 0) h = std::max(h, 1 + height[(size_t)r]);
    height[(size_t)i] = h;
    top = std::max(top, h);
  }
  if (reached != n) return false;
  group_off.assign((size_t)top + 2, 0);
  for (int i = 0; i < n; i++) group_off[(size_t)height[(size_t)i] + 1]++;
  for (size_t h = 1; h < group_off.size(); h++) group_off[h] += group_off[h - 1];
  order.resize((size_t)n);
  std::vector<int32_t> at(group_off.begin(), group_off.end() - 1);
  for (int i = 0; i < n; i++) order[(size_t)at[(size_t)height[(size_t)i]]++] = i;
  return true;
}

}  // namespace rt0h

extern "C" int rt0_bvh_height_order(const void *nodes, int n_triangles, int32_t *order_out, int32_t *group_out,
                                    int *n_groups, int32_t *parent_out, int32_t *height_out) {
  if (!nodes || n_triangles <= 0) return RT0_E_ARG;
  std::vector<int32_t> order, off, parent, height;
  if (!rt0h::bvh_height_order(static_cast<const BvhNode *>(nodes), n_triangles, order, off, parent, height))
    return RT0_E_ARG;
  const size_t n = order.size();
  for (size_t i = 0; i < n; i++) {
    if (order_out) order_out[i] = order[i];
    if (parent_out) parent_out[i] = parent[i];
    if (height_out) height_out[i] = height[i];
  }
  if (group_out)
    for (size_t h = 0; h < off.size(); h++) group_out[h] = off[h];
  if (n_groups) *n_groups = (int)off.size() - 1;
  return RT0_OK;
}
