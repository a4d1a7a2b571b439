// The decision tree's walks, one thread per feature row (tree_kernel.hip's
// window and row kernels, stream_tree_kernel.hip's ring kernel).  The rule is
// sklearn's (tree_kernel.hip's header): left iff x[feature] <= threshold, a
// NaN feature following the node's nan_left.
#pragma once

#include "vad_common.h"

namespace vad {

__device__ __forceinline__ int tree_walk(const TreeNode* __restrict__ nodes, int n_nodes,
                                         const float* __restrict__ x, int x_step) {
  int node = 0;
  // every root-to-leaf path has < n_nodes edges; the bound only guards a
  // malformed table against looping forever
  for (int it = 0; it < n_nodes; ++it) {
    const TreeNode nd = nodes[node];
    if (nd.feature < 0) return nd.leaf;
    const float xv = x[nd.feature * x_step];
    const bool left = xv != xv ? nd.nan_left != 0 : (double)xv <= nd.threshold;
    node = left ? nd.left : nd.right;
  }
  return 0;
}

__device__ __forceinline__ int tree_walk_c(const TreeNodeC* nodes, int n_nodes, const float* x) {
  int node = 0;
  for (int it = 0; it < n_nodes; ++it) {
    const TreeNodeC nd = nodes[node];
    if (nd.feature < 0) return -1 - nd.feature;
    const float xv = x[nd.feature & 0xffff];
    const bool left = xv != xv ? (nd.feature >> 30) != 0 : xv <= nd.thr;
    node = left ? nd.left : nd.right;
  }
  return 0;
}

// The same two walks ending in the leaf's NODE index (score_kernel.hip looks
// the leaf's score up by it); 0, the root, for a malformed table.
__device__ __forceinline__ int tree_walk_node(const TreeNode* __restrict__ nodes, int n_nodes,
                                              const float* __restrict__ x, int x_step) {
  int node = 0;
  for (int it = 0; it < n_nodes; ++it) {
    const TreeNode nd = nodes[node];
    if (nd.feature < 0) return node;
    const float xv = x[nd.feature * x_step];
    const bool left = xv != xv ? nd.nan_left != 0 : (double)xv <= nd.threshold;
    node = left ? nd.left : nd.right;
  }
  return 0;
}

__device__ __forceinline__ int tree_walk_c_node(const TreeNodeC* nodes, int n_nodes, const float* x) {
  int node = 0;
  for (int it = 0; it < n_nodes; ++it) {
    const TreeNodeC nd = nodes[node];
    if (nd.feature < 0) return node;
    const float xv = x[nd.feature & 0xffff];
    const bool left = xv != xv ? (nd.feature >> 30) != 0 : xv <= nd.thr;
    node = left ? nd.left : nd.right;
  }
  return 0;
}

}  // namespace vad
