// The lock-free union-find on keypoint rows that gh_link_tracks_dev (track_link.hip) and gh_extend_tracks_dev (track_extend.hip)
// share: parent[] by node id, linking by index, labels = the smallest node id of a component, and the run bounds of the
// components on the sorted (label, node) list.  THE INVARIANT comment of track_link.hip covers every line here: after
// link_init the only writes to parent[] are atomic operations that lower the value, every read of parent[] while it changes is
// an agent-scope relaxed atomic load.
//
// `live` (may be NULL) restricts the graph to a subset of the existing nodes: a node takes part when live[n] == kUfLive.  The
// bytes are written by an earlier launch and are constant while these kernels run.  link_union tests both ends' byte BEFORE it
// touches parent[], so a node outside the subset stays the root of itself and is never read through; link_label gives it the
// extra bin N.  With live == NULL every existing node takes part (gh_link_tracks_dev).
//
// The edge rule, the clamp of a frame's row count and kBlock are gh_map's (map_dev.h); gh_merge_points_dev (track_merge.hip) runs
// uf_unite on its own elements.
#pragma once
#include "map_dev.h"

namespace gh_uf {
namespace {  // (internal linkage: every translation unit that includes this header gets its own kernels)

using namespace gh_map;

constexpr int kMaxUnionBlocks = 1 << 16;  // grid-stride beyond this many workgroups
constexpr uint8_t kUfLive = 1;

__device__ __forceinline__ int link_load(const int32_t* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x as far as this lane can see it, p = parent[x] as just read; every step taken also lowers parent[x] to its
// grandparent (path halving)
__device__ __forceinline__ int link_find_halve(int32_t* parent, int x, int p) {
  while (p != x) {  // p < x
    const int g = link_load(parent, p);
    if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ int link_find(const int32_t* parent, int x) {
  int p = link_load(parent, x);
  while (p != x) {
    x = p;
    p = link_load(parent, x);
  }
  return x;
}

// Joins the trees of u and v: find with path halving on both ends, hook the larger root under the smaller, retry from the new
// roots when the compare-and-swap fails.  The loop ends: a failed compare-and-swap means that parent[hi] was lowered by somebody
// else (THE INVARIANT: nothing ever raises it), so the root found from `old` is strictly smaller than hi, and the larger of the
// two roots strictly descends from one round to the next; it is bounded below by 0.  No lane waits for another lane's store.
__device__ __forceinline__ void uf_unite(int32_t* parent, int u, int v) {
  const int pu = link_load(parent, u), pv = link_load(parent, v);
  if (pu == pv) return;  // one tree already: in a flat component this spares the root's hot word two reads per edge
  int a = link_find_halve(parent, u, pu), b = link_find_halve(parent, v, pv);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) break;
    a = link_find_halve(parent, old, link_load(parent, old));  // < hi
    b = link_find_halve(parent, lo, link_load(parent, lo));
  }
}

__global__ __launch_bounds__(kBlock) void link_init_kernel(int32_t* __restrict__ parent, int N) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g < N) parent[g] = (int32_t)g;
}

__global__ __launch_bounds__(kBlock) void link_union_kernel(const int32_t* __restrict__ counts, int n_frames, int cap,
                                                            const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_t,
                                                            long long rows, const int32_t* __restrict__ idx1,
                                                            const uint8_t* __restrict__ inlier, const uint8_t* __restrict__ live,
                                                            int32_t* parent) {
  const PairRows e = {counts, n_frames, cap, pair_q, pair_t, idx1, inlier};
  const long long step = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < rows; r += step) {
    int u, v;
    if (!pair_edge(e, r, &u, &v)) continue;
    if (live && (live[u] != kUfLive || live[v] != kUfLive)) continue;
    uf_unite(parent, u, v);
  }
}

__global__ __launch_bounds__(kBlock) void link_label_kernel(const int32_t* __restrict__ counts, int cap, int N,
                                                            const uint8_t* __restrict__ live, const int32_t* parent,
                                                            int32_t* __restrict__ key, int32_t* __restrict__ item) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int n = (int)g;
  const int f = n / cap, i = n - f * cap;
  const bool in = live ? live[n] == kUfLive : i < row_count(counts, f, cap);
  key[n] = in ? link_find(parent, n) : N;
  item[n] = n;
}

__global__ __launch_bounds__(kBlock) void link_runs_kernel(const int32_t* __restrict__ skey, const int32_t* __restrict__ list, int cap,
                                                           int N, int32_t* __restrict__ begin, int32_t* __restrict__ end,
                                                           uint8_t* __restrict__ conflict) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int s = (int)g;
  const int l = skey[s];
  if (l == N) return;  // (the nodes that take no part come last)
  const int prev = s > 0 ? skey[s - 1] : -1, next = s + 1 < N ? skey[s + 1] : N;
  if (prev != l) begin[l] = s;
  if (next != l) end[l] = s + 1;
  else if (list[s] / cap == list[s + 1] / cap) conflict[l] = 1;
}

}  // namespace
}  // namespace gh_uf
