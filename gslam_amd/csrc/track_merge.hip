// Merging map points that the matches show to be one, device-resident: gh_merge_points_dev.  A track that broke comes back
// under a second point id; a later frame whose rows are matched to holders of both ids (or a chain of matches through rows
// without a point) shows that the two are one.  This call finds those groups, keeps the smallest id of each (the oldest, so what
// hangs on old ids stays valid longest), and renames the others in node_point and in the observation list.  The contract is in
// include/gslam_hip.h; tests/track_merge_restate.py restates it on dicts and sets and the device is held to it byte for byte.
// Everything is integer work except the distance gate, which is six IEEE operations rounded once each (__dsub_rn, __dmul_rn,
// __dadd_rn: nothing the compiler may fuse), so the result is the same bits on every run.
//
// WHY THE VERDICTS DO NOT DEPEND ON A RACE.  elem[n] (the point a node holds, the node's own element when it is a BRIDGE, or "takes
// no part") is a function of the node's own inputs: mrg_init has one lane per element and one writer per word.  The components
// come from the union-find of track_link.hip on n_points + N elements (track_uf.h, THE INVARIANT there: after mrg_init parent[]
// is only ever lowered, by atomics); the points come first, so the root of a component that contains a point is its smallest
// point, whatever the order of the pairs, the launch geometry or the outcome of any race.  mrg_union compares the two ends'
// elements BEFORE it touches parent[], so an edge inside one point, an edge at an OUT node and an unusable point never reach it:
// an unusable point stays the root of itself.  mrg_label runs after mrg_union has returned and writes nothing to parent[]; root[p]
// has one writer, group[r] and far[r] get the byte 1 from every writer (the same value from all of them) on bytes one memset
// zeroed.  CONFLICT is decided on the list sorted by (label, node): the sort is stable and the items go in ascending, so the
// holders of one group come in ascending node id and those of one frame are neighbours; a position looks at its right
// neighbour and stores the byte 1 to conflict[label].  mrg_points has one lane and one writer per point and reads only bytes that
// earlier launches completed.  point_len and the totals are integer atomic adds on words the call zeroed -- commutative and
// exact -- after a reduction inside the wave (gh_map::add_runs) or the workgroup (gh_map::block_counts_add).  No float atomic
// anywhere.
// mrg_emit has one writer per entry and reads its input entry before it writes the same index, which is what makes
// node_point_dev == node_point_in_dev (and the same for obs_point) safe; every earlier launch that read node_point_in has
// completed by then (one stream).
//
// CDNA4 mapping (the shared pieces are gh_map's, map_dev.h, and the union-find's, track_uf.h):
//   * mrg_init    one lane per element: parent[g] = g; the lanes of the nodes also write elem[n];
//   * mrg_union   one lane per (pair, query row), grid-stride; pair_edge, the ends taken through elem[], uf_unite;
//   * mrg_label   one lane per point: root[p] = find(p) without any write to parent[]; root != p marks the root's group byte and,
//                 with the gate on, its far byte when the point fails the gate against the root (the root itself is at
//                 distance 0 of itself unless a coordinate is not finite, and then every other point of the group fails);
//   * mrg_key     one lane per node: the label of a HOLDER of a grouped point, the extra bin n_points otherwise; item[n] = n;
//   * sort        rocPRIM's stable radix sort of (key, node) over the bits of n_points + 1 values;
//   * mrg_runs    over that list: neighbours with one label and one frame -> conflict[label] = 1;
//   * mrg_points  one lane per point: remap, state and select, and five of the totals;
//   * mrg_emit    one lane per node: node_point, obs_point, point_len (add_runs) and the changed total.
// Without an edge (npairs == 0 or cap == 0) nothing can be in a group: union, key, sort and runs are skipped.
#include <climits>

#include "dev_prims.h"
#include "track_uf.h"

namespace {

using namespace gh_uf;

constexpr int kNoElem = -1;  // elem[] of an existing node that is OUT, and of a node that does not exist

__global__ __launch_bounds__(kBlock) void mrg_init_kernel(const int32_t* __restrict__ counts, int cap, int N,
                                                          const int32_t* __restrict__ node_point_in, int n_points,
                                                          const int32_t* __restrict__ status, int bridge, int32_t* __restrict__ parent,
                                                          int32_t* __restrict__ elem) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (long long)n_points + N) return;
  parent[g] = (int32_t)g;
  if (g < n_points) return;
  const int n = (int)(g - n_points);
  const int f = n / cap, i = n - f * cap;
  int e = kNoElem;
  if (i < row_count(counts, f, cap)) {
    const int v = node_point_in[n];
    if (v >= 0 && v < n_points) {
      if (!status || status[v] == GH_TRACK_OK) e = v;  // HOLDER
    } else if (bridge) {
      e = (int)g;  // BRIDGE: the element n_points + n
    }
  }
  elem[n] = e;
}

// (the loop inside uf_unite ends: the argument is stated there, track_uf.h)
__global__ __launch_bounds__(kBlock) void mrg_union_kernel(const int32_t* __restrict__ counts, int n_frames, int cap,
                                                           const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_t,
                                                           long long rows, const int32_t* __restrict__ idx1,
                                                           const uint8_t* __restrict__ inlier, const int32_t* __restrict__ elem,
                                                           int32_t* parent) {
  const PairRows e = {counts, n_frames, cap, pair_q, pair_t, idx1, inlier};
  const long long step = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < rows; r += step) {
    int nu, nv;
    if (!pair_edge(e, r, &nu, &nv)) continue;
    const int u = elem[nu], v = elem[nv];
    if (u < 0 || v < 0 || u == v) continue;  // an OUT end; or both ends hold one point: nearly every edge of a healthy map
    uf_unite(parent, u, v);
  }
}

// the gate: (dx * dx + dy * dy) + dz * dz <= max2, every operation rounded once and none fused; a NaN fails
__device__ __forceinline__ bool mrg_near(const double* __restrict__ xyz, int p, int q, double max2) {
  const double dx = __dsub_rn(xyz[3 * (size_t)p], xyz[3 * (size_t)q]);
  const double dy = __dsub_rn(xyz[3 * (size_t)p + 1], xyz[3 * (size_t)q + 1]);
  const double dz = __dsub_rn(xyz[3 * (size_t)p + 2], xyz[3 * (size_t)q + 2]);
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)) <= max2;
}

__global__ __launch_bounds__(kBlock) void mrg_label_kernel(const int32_t* parent, int n_points, const double* __restrict__ xyz,
                                                           double max2, int32_t* __restrict__ root, uint8_t* group, uint8_t* far) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_points) return;
  const int p = (int)g;
  const int r = link_find(parent, p);  // <= p: a point
  root[p] = r;
  if (r == p) return;
  group[r] = 1;
  if (!xyz) return;
  // the label against itself too: a coordinate of it that is not finite fails the group whatever max_dist is
  if (!mrg_near(xyz, p, r, max2) || !mrg_near(xyz, r, r, max2)) far[r] = 1;
}

__global__ __launch_bounds__(kBlock) void mrg_key_kernel(const int32_t* __restrict__ elem, const int32_t* __restrict__ root,
                                                         const uint8_t* __restrict__ group, int N, int n_points,
                                                         int32_t* __restrict__ key, int32_t* __restrict__ item) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int n = (int)g;
  const int e = elem[n];
  int k = n_points;
  if (e >= 0 && e < n_points) {
    const int l = root[e];
    if (group[l]) k = l;
  }
  key[n] = k;
  item[n] = n;
}

__global__ __launch_bounds__(kBlock) void mrg_runs_kernel(const int32_t* __restrict__ skey, const int32_t* __restrict__ list, int cap,
                                                          int N, int n_points, uint8_t* conflict) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int s = (int)g;
  const int l = skey[s];
  if (l == n_points) return;  // (the nodes that hold no point of a group come last)
  if (s + 1 < N && skey[s + 1] == l && list[s] / cap == list[s + 1] / cap) conflict[l] = 1;
}

// totals [0] MERGED groups, [1] ABSORBED points, [2] CONFLICT groups, [3] FAR groups, [5] points of CONFLICT or FAR groups
__global__ __launch_bounds__(kBlock) void mrg_points_kernel(const int32_t* __restrict__ root, const uint8_t* __restrict__ group,
                                                            const uint8_t* __restrict__ conflict, const uint8_t* __restrict__ far,
                                                            int n_points, int32_t* __restrict__ remap, uint8_t* __restrict__ state,
                                                            uint8_t* __restrict__ select, int32_t* totals) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool merged = false, absorbed = false, is_conflict = false, is_far = false, apart = false;
  if (g < n_points) {
    const int p = (int)g;
    const int l = root[p];
    uint8_t s = GH_MERGE_NONE;
    if (group[l]) {
      s = conflict[l] ? GH_MERGE_CONFLICT : far[l] ? GH_MERGE_FAR : p == l ? GH_MERGE_SURVIVOR : GH_MERGE_ABSORBED;
      apart = s == GH_MERGE_CONFLICT || s == GH_MERGE_FAR;
      merged = s == GH_MERGE_SURVIVOR;
      absorbed = s == GH_MERGE_ABSORBED;
      is_conflict = s == GH_MERGE_CONFLICT && p == l;
      is_far = s == GH_MERGE_FAR && p == l;
    }
    remap[p] = absorbed ? l : p;
    state[p] = s;
    select[p] = merged ? 1 : 0;
  }
  block_counts_add<5>({wave_count(merged), wave_count(absorbed), wave_count(is_conflict), wave_count(is_far), wave_count(apart)},
                      [totals](int k) { return totals + (k < 4 ? k : 5); });
}

// node_point / obs_point may be their inputs: no __restrict__ on the four, and each lane reads entry n before it writes entry n
__global__ __launch_bounds__(kBlock) void mrg_emit_kernel(const int32_t* __restrict__ counts, int cap, int N, int n_points,
                                                          const int32_t* __restrict__ remap, const int32_t* node_point_in,
                                                          const int32_t* obs_point_in, int32_t* node_point, int32_t* obs_point,
                                                          int32_t* point_len, int32_t* totals) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool counted = false, changed = false;
  int out = 0;
  if (g < N) {
    const int n = (int)g;
    const int v = node_point_in[n];
    const bool id = v >= 0 && v < n_points;
    out = id ? remap[v] : v;
    node_point[n] = out;
    if (obs_point_in) {
      const int o = obs_point_in[n];
      obs_point[n] = (o >= 0 && o < n_points) ? remap[o] : o;
    }
    const int f = n / cap, i = n - f * cap;
    counted = id && i < row_count(counts, f, cap);
    changed = counted && out != v;
  }
  add_runs(point_len, out, counted);
  block_counts_add<1>({wave_count(changed)}, totals + 4);
}

}  // namespace

extern "C" gh_status gh_merge_points_dev(gh_ctx* ctx, const int32_t* counts_dev, int n_frames, int cap, const int32_t* pair_q_dev,
                                         const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev, const uint8_t* inlier_dev,
                                         const int32_t* node_point_in_dev, int n_points, const int32_t* point_status_dev,
                                         const double* point_xyz_dev, double max_dist, int bridge, const int32_t* obs_point_in_dev,
                                         int32_t* point_remap_dev, uint8_t* point_state_dev, uint8_t* point_select_dev,
                                         int32_t* node_point_dev, int32_t* obs_point_dev, int32_t* point_len_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n_frames >= 0 && cap >= 0 && npairs >= 0 && n_points >= 0 && cap <= 65535);
  GH_CHECK_ARG(ctx, (long long)n_points + (long long)n_frames * cap <= (long long)INT32_MAX - 1);
  GH_CHECK_ARG(ctx, counts_dev && node_point_in_dev);
  GH_CHECK_ARG(ctx, point_remap_dev && point_state_dev && point_select_dev && node_point_dev && point_len_dev && totals_dev);
  GH_CHECK_ARG(ctx, (obs_point_in_dev == nullptr) == (obs_point_dev == nullptr));
  GH_CHECK_ARG(ctx, npairs == 0 || (pair_q_dev && pair_t_dev && idx1_dev));
  GH_CHECK_ARG(ctx, !point_xyz_dev || max_dist >= 0.0);  // (a NaN fails)
  const int N = n_frames * cap;
  const double max2 = max_dist * max_dist;  // formed once, one double product
  const long long rows = (long long)npairs * cap;
  const bool edges = rows > 0 && N > 0 && n_points > 0;

  GH_HIP(ctx, hipMemsetAsync(totals_dev, 0, 6 * sizeof(int32_t), ctx->stream));
  if (n_points > 0) GH_HIP(ctx, hipMemsetAsync(point_len_dev, 0, (size_t)n_points * sizeof(int32_t), ctx->stream));
  if (N == 0 && n_points == 0) return GH_OK;

  // The scratch block.  group, conflict and far are neighbours: one memset clears them.
  const size_t n = (size_t)N, np = (size_t)n_points;
  const int bits = gh_key_bits(n_points);
  const size_t tmp_bytes = edges ? gh_sort_pairs_bytes(ctx, n, bits) : 0;
  if (edges && !tmp_bytes) return gh_set_error(ctx, GH_ERR_HIP, "gh_merge_points_dev: rocPRIM size query failed");
  gh_carve c;
  const size_t o_parent = c.take((np + n) * 4), o_elem = c.take(n * 4), o_root = c.take(np * 4), o_key = c.take(n * 4);
  const size_t o_item = c.take(n * 4), o_skey = c.take(n * 4), o_list = c.take(n * 4);
  const size_t o_group = c.take(np), o_conflict = c.take(np), o_far = c.take(np), o_tmp = c.take(tmp_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* parent = (int32_t*)(base + o_parent);
  int32_t* elem = (int32_t*)(base + o_elem);
  int32_t* root = (int32_t*)(base + o_root);
  int32_t* key = (int32_t*)(base + o_key);
  int32_t* item = (int32_t*)(base + o_item);
  int32_t* skey = (int32_t*)(base + o_skey);
  int32_t* list = (int32_t*)(base + o_list);
  uint8_t* group = (uint8_t*)(base + o_group);
  uint8_t* conflict = (uint8_t*)(base + o_conflict);
  uint8_t* far = (uint8_t*)(base + o_far);

  const dim3 block(kBlock), node_grid(gh_div_up(N, kBlock)), point_grid(gh_div_up(n_points, kBlock));
  if (n_points > 0) GH_HIP(ctx, hipMemsetAsync(group, 0, o_tmp - o_group, ctx->stream));
  GH_LAUNCH(ctx, "mrg_init", mrg_init_kernel, dim3(gh_div_up((long long)n_points + N, kBlock)), block, 0, counts_dev, cap, N,
            node_point_in_dev, n_points, point_status_dev, bridge, parent, elem);
  if (edges) {
    const long long want = (rows + kBlock - 1) / kBlock;
    GH_LAUNCH(ctx, "mrg_union", mrg_union_kernel, dim3((unsigned)(want < kMaxUnionBlocks ? want : kMaxUnionBlocks)), block, 0, counts_dev,
              n_frames, cap, pair_q_dev, pair_t_dev, rows, idx1_dev, inlier_dev, (const int32_t*)elem, parent);
  }
  if (n_points > 0)
    GH_LAUNCH(ctx, "mrg_label", mrg_label_kernel, point_grid, block, 0, (const int32_t*)parent, n_points, point_xyz_dev, max2, root, group,
              far);
  if (edges) {
    GH_LAUNCH(ctx, "mrg_key", mrg_key_kernel, node_grid, block, 0, (const int32_t*)elem, (const int32_t*)root, (const uint8_t*)group, N,
              n_points, key, item);
    GH_TRY(gh_sort_pairs_i32(ctx, "mrg_sort", "gh_merge_points_dev: sort", base + o_tmp, tmp_bytes, key, skey, item, list, n, bits));
    GH_LAUNCH(ctx, "mrg_runs", mrg_runs_kernel, node_grid, block, 0, (const int32_t*)skey, (const int32_t*)list, cap, N, n_points,
              conflict);
  }
  if (n_points > 0)
    GH_LAUNCH(ctx, "mrg_points", mrg_points_kernel, point_grid, block, 0, (const int32_t*)root, (const uint8_t*)group,
              (const uint8_t*)conflict, (const uint8_t*)far, n_points, point_remap_dev, point_state_dev, point_select_dev, totals_dev);
  if (N > 0)
    GH_LAUNCH(ctx, "mrg_emit", mrg_emit_kernel, node_grid, block, 0, counts_dev, cap, N, n_points, (const int32_t*)point_remap_dev,
              node_point_in_dev, obs_point_in_dev, node_point_dev, obs_point_dev, point_len_dev, totals_dev);
  return GH_OK;
}
