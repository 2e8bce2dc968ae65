// Multi-view tracks from pair matches, device-resident: gh_link_tracks_dev.  The inlier rows of every matched frame pair are the
// edges of a graph on the keypoint rows (node = frame * cap + row); its connected components are the tracks.  The contract is in
// include/gslam_hip.h; tests/track_link_restate.py restates it with a textbook union-find and the device is held to it byte for
// byte.  Everything is integer work except the two divisions per observation, so the result is the same bits on every run.
//
// THE INVARIANT.  parent[] is written by link_init (parent[n] = n) and, after that launch, ONLY by atomic operations that lower
// the value: the compare-and-swap that hooks a root under a smaller node and the atomic minimum of the halving step.  Hence
// parent[x] <= x at every moment, every parent chain strictly descends, the structure is acyclic under any interleaving and find
// terminates on whatever mix of fresh and stale values it reads.  Both writes put an ancestor (or a node of the tree that is
// being joined) in the place of an ancestor, so a tree never splits; a root is the smallest node of its tree because every other
// node of the tree has a chain that descends to it.  When link_union has returned every edge joins two nodes of one tree, so the
// root of a node is the smallest id of its connected component: the label, whatever the order of the pairs, the launch geometry
// or the outcome of any race.  A stale root only makes a compare-and-swap fail (then somebody else's succeeded: global progress)
// or hooks under an ancestor of the true root; no lane ever waits for another lane's store, there is no lock.
// Every read of parent[] while it changes is an agent-scope relaxed atomic load: a CU's L1 is never refreshed by another CU's
// stores and the L2s of the XCDs are not coherent with each other, the atomics are served past both.
//
// CDNA4 mapping (this is the Jayanti-Tarjan / ECL-CC scheme; linking by index is what makes the root the minimum):
//   * link_init     parent[n] = n;
//   * link_union    one lane per (pair, query row), grid-stride; gh_map::pair_edge (map_dev.h) decides whether the row is an edge,
//                   uf_unite (track_uf.h) joins the two trees;
//   * link_label    a launch of its own: key[n] = find(n) without any write for an existing node, the extra bin N otherwise.  The
//                   labels do not depend on how far link_union compressed the paths;
//   * sort          rocPRIM's stable radix sort of (key, node) pairs lists a component in ascending node id, so two nodes of one
//                   frame are neighbours in the list.  Not gh_csr_index_dev (csr_sort.hip), which was measured here first: its
//                   histogram is one atomic add per item on the item's bin, and wrong matches chain tracks into very large
//                   components -- one hot word: 2.4 / 9.7 / 15.2 ms of a 2.9 / 10.5 / 16.2 ms call at 2 M nodes;
//   * link_runs     over the sorted list: a position whose left neighbour has another key stores begin[label], one whose right
//                   neighbour has another key end[label] (so end - begin is the size of the component, without any atomic);
//                   neighbours with one label and one frame store the byte 1 to the label's flag (the same value from every writer);
//   * link_flags    per node: observation? (low word) and, at the label itself, track? (high word) packed into one uint64, so that
//                   ONE rocPRIM exclusive scan numbers the observations and the points; grid-stride over at most 1024 workgroups,
//                   the CONFLICT and SHORT components (gh_map::component_verdict) counted in registers, then
//                   gh_map::block_counts_add: LDS, one integer atomic per workgroup;
//   * link_emit     writes every entry of every output: node_point, the observation of a track node at its rank (gh_map::emit_obs),
//                   the padding past n_obs (pad_obs), point_len at the labels and zeros past n_points, totals.
// The sort and the scan are dev_prims.h's; the work space comes from the context's scratch.
#include <algorithm>
#include <climits>

#include "dev_prims.h"
#include "track_uf.h"

namespace {

// the union-find, its labels and the run bounds (link_init / link_union / link_label / link_runs): track_uf.h, shared with
// track_extend.hip; the edge rule, the verdict on a component, the observation writers and the counter tail: map_dev.h
using namespace gh_uf;

struct LinkArgs {
  const gh_keypoint* kps;
  int cap, N;
  int min_views;
  Pinhole pin;
  const int32_t* key;        // N: label, or N for a node that does not exist
  const int32_t* begin;      // N, by label: the component's range in the sorted list
  const int32_t* end;
  const uint8_t* conflict;   // N, by label
  const uint64_t* rank;      // N + 1: exclusive scan of the flags; [N] = the totals
  const int32_t* counters;   // CONFLICT components, SHORT components of two nodes or more
  int32_t* node_point;
  ObsOut obs;
  int32_t* point_len;
  int32_t* totals;
};

__global__ __launch_bounds__(kBlock) void link_flags_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ begin,
                                                            const int32_t* __restrict__ end, const uint8_t* __restrict__ conflict, int N,
                                                            int min_views, uint64_t* __restrict__ flags, int32_t* __restrict__ counters) {
  int nc = 0, ns = 0;  // the same in every lane of a wave
  const long long step = (long long)gridDim.x * kBlock;
  for (long long base = (long long)blockIdx.x * kBlock; base <= N; base += step) {  // (entry N is the scan's room for the totals)
    const long long g = base + threadIdx.x;
    bool is_conflict = false, is_short = false;
    if (g <= N) {
      const int n = (int)g;
      uint64_t f = 0;
      const int l = n < N ? key[n] : N;
      if (l != N) {
        const Component c = component_verdict(l, begin, end, conflict, min_views);
        const bool track = c.verdict == kTrack;
        f = track ? 1u : 0u;
        if (n == l) {
          if (track) f |= 1ull << 32;
          is_conflict = c.verdict == kConflict;
          is_short = c.counted_short();
        }
      }
      flags[n] = f;
    }
    nc += wave_count(is_conflict);
    ns += wave_count(is_short);
  }
  block_counts_add<2>({nc, ns}, counters);
}

__global__ __launch_bounds__(kBlock) void link_emit_kernel(LinkArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.N) return;
  const int n = (int)g;
  const uint64_t total = a.rank[a.N];
  const int n_obs = (int)(uint32_t)total, n_points = (int)(total >> 32);
  if (n == 0) {
    a.totals[0] = n_obs;
    a.totals[1] = n_points;
    a.totals[2] = a.counters[0];
    a.totals[3] = a.counters[1];
  }
  if (n >= n_obs) pad_obs(a.obs, n);
  if (n >= n_points && n < a.N / 2) a.point_len[n] = 0;
  const int l = a.key[n];
  int code = GH_LINK_NO_ROW;
  if (l != a.N) {
    const Component c = component_verdict(l, a.begin, a.end, a.conflict, a.min_views);
    if (c.verdict == kConflict) {
      code = GH_LINK_CONFLICT;
    } else if (c.verdict == kShort) {
      code = GH_LINK_SHORT;
    } else {
      code = (int)(a.rank[l] >> 32);
      emit_obs(a.obs, (int)(uint32_t)a.rank[n], n / a.cap, code, n, a.kps[n], a.pin);
      if (n == l) a.point_len[code] = c.size;
    }
  }
  a.node_point[n] = code;
}

}  // namespace

extern "C" gh_status gh_link_tracks_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                        const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                        const uint8_t* inlier_dev, double fx, double fy, double cx, double cy, int min_views,
                                        int32_t* node_point_dev, int32_t* obs_cam_dev, int32_t* obs_point_dev, double* obs_xy_dev,
                                        int32_t* obs_node_dev, int32_t* point_len_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n_frames >= 0 && cap >= 0 && npairs >= 0 && cap <= 65535);
  GH_CHECK_ARG(ctx, (long long)n_frames * cap <= (long long)INT32_MAX - 1);
  GH_CHECK_ARG(ctx, min_views >= 2);
  GH_CHECK_ARG(ctx, fx > 0.0 && fy > 0.0);  // (a NaN fails)
  GH_CHECK_ARG(ctx, kps_dev && counts_dev);
  GH_CHECK_ARG(ctx, node_point_dev && obs_cam_dev && obs_point_dev && obs_xy_dev && obs_node_dev && point_len_dev && totals_dev);
  GH_CHECK_ARG(ctx, npairs == 0 || (pair_q_dev && pair_t_dev && idx1_dev));
  const int N = n_frames * cap;
  if (N == 0) {
    GH_HIP(ctx, hipMemsetAsync(totals_dev, 0, 4 * sizeof(int32_t), ctx->stream));
    return GH_OK;
  }

  // The scratch block.  conflict and the two counters are neighbours: one memset clears both.  The rocPRIM storage serves the
  // sort of N pairs and the scan of N + 1 flags.
  const size_t n = (size_t)N;
  const int bits = gh_key_bits(N);
  const size_t sort_bytes = gh_sort_pairs_bytes(ctx, n, bits), scan_bytes = gh_scan_u64_bytes(ctx, n + 1);
  if (!sort_bytes || !scan_bytes) return gh_set_error(ctx, GH_ERR_HIP, "gh_link_tracks_dev: rocPRIM size query failed");
  const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
  gh_carve c;
  const size_t o_parent = c.take(n * 4), o_key = c.take(n * 4), o_skey = c.take(n * 4), o_item = c.take(n * 4), o_list = c.take(n * 4);
  const size_t o_conflict = c.take(n), o_counters = c.take(2 * sizeof(int32_t));
  const size_t o_flags = c.take((n + 1) * 8), o_rank = c.take((n + 1) * 8), o_tmp = c.take(tmp_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* parent = (int32_t*)(base + o_parent);
  int32_t* key = (int32_t*)(base + o_key);
  int32_t* skey = (int32_t*)(base + o_skey);
  int32_t* item = (int32_t*)(base + o_item);
  int32_t* list = (int32_t*)(base + o_list);
  int32_t* begin = parent;  // (parent is dead after link_label)
  int32_t* end = item;      // (the sort's input, dead after the sort)
  uint8_t* conflict = (uint8_t*)(base + o_conflict);
  int32_t* counters = (int32_t*)(base + o_counters);
  uint64_t* flags = (uint64_t*)(base + o_flags);
  uint64_t* rank = (uint64_t*)(base + o_rank);
  void* tmp = base + o_tmp;

  const dim3 grid(gh_div_up(N, kBlock)), block(kBlock);
  GH_HIP(ctx, hipMemsetAsync(conflict, 0, o_flags - o_conflict, ctx->stream));
  GH_LAUNCH(ctx, "link_init", link_init_kernel, grid, block, 0, parent, N);
  const long long rows = (long long)npairs * cap;
  if (rows > 0) {
    const long long want = (rows + kBlock - 1) / kBlock;
    GH_LAUNCH(ctx, "link_union", link_union_kernel, dim3((unsigned)(want < kMaxUnionBlocks ? want : kMaxUnionBlocks)), block, 0,
              counts_dev, n_frames, cap, pair_q_dev, pair_t_dev, rows, idx1_dev, inlier_dev, (const uint8_t*)nullptr, parent);
  }
  GH_LAUNCH(ctx, "link_label", link_label_kernel, grid, block, 0, counts_dev, cap, N, (const uint8_t*)nullptr, parent, key, item);
  GH_TRY(gh_sort_pairs_i32(ctx, "link_sort", "gh_link_tracks_dev: sort", tmp, tmp_bytes, key, skey, item, list, n, bits));
  GH_LAUNCH(ctx, "link_runs", link_runs_kernel, grid, block, 0, skey, list, cap, N, begin, end, conflict);
  const int flag_blocks = gh_div_up((long long)N + 1, kBlock);
  GH_LAUNCH(ctx, "link_flags", link_flags_kernel, dim3(flag_blocks < kMaxFlagBlocks ? flag_blocks : kMaxFlagBlocks), block, 0, key, begin,
            end, conflict, N, min_views, flags, counters);
  GH_TRY(gh_scan_u64(ctx, "link_scan", "gh_link_tracks_dev: scan", tmp, tmp_bytes, flags, rank, n + 1));

  const LinkArgs a = {kps_dev, cap, N, min_views, {fx, fy, cx, cy},   // the inputs
                      key, begin, end, conflict, rank, counters,      // scratch
                      node_point_dev, {obs_cam_dev, obs_point_dev, obs_xy_dev, obs_node_dev}, point_len_dev, totals_dev};
  GH_LAUNCH(ctx, "link_emit", link_emit_kernel, grid, block, 0, a);
  return GH_OK;
}
