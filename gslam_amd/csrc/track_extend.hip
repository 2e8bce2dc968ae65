// Extending the map, device-resident: gh_extend_tracks_dev.  A batch of new frames has been matched (pair entries) and
// registered (gh_localize_pairs_dev: row_point, row_inlier); this call adds the registered rows to the tracks of the map points
// they saw and links the remaining rows into NEW tracks, whose ids go on where the map's end -- so point_xyz, the point status
// and everything else that hangs on the old ids stays valid.  The contract is in include/gslam_hip.h;
// tests/track_extend_restate.py restates it on dicts and sets and the device is held to it byte for byte.  Everything is integer
// work except the two divisions per observation, so the result is the same bits on every run.
//
// WHY THE VERDICTS DO NOT DEPEND ON A RACE.  The state of a node (MAPPED, CLAIMANT, FREE, missing) is a function of the node's
// own inputs: ext_state has one lane per node and one writer per byte.  REJECTED is decided on the list sorted by (point, node):
// the sort is stable and the items go in ascending, so the nodes of one point come in ascending id and those of one frame are
// contiguous; a claimant looks at its two immediate neighbours and stores its OWN reject byte -- one writer per byte, plain
// loads of bytes a previous launch wrote.  point_grew gets the byte 1 from every adopted claimant of the point (the same value
// from every writer).  point_len of an old point is (end of its run) - (begin of its run) - (its rejected claimants): three
// kinds of integer atomic adds on a word the call zeroed, two per point plus one per rejected claimant -- commutative and
// exact, and not one per observation (a popular point would be the hot word DESIGN.md 6g measured).  New tracks come from the
// union-find of track_link.hip (track_uf.h, THE INVARIANT there) restricted to the FREE nodes: link_union tests both ends'
// state byte before it touches parent[], so a MAPPED, adopted or rejected node never joins anything and the labels are the
// smallest FREE node of each component whatever the order of the pairs.  Ids and ranks are prefix sums over node ids.
//
// CDNA4 mapping (the shared pieces are gh_map's, map_dev.h, and the union-find's, track_uf.h):
//   * ext_state   one lane per node: the state byte and the key of the first sort (the point of a MAPPED or CLAIMANT node, the
//                 extra bin n_points otherwise), item[n] = n;
//   * sort        rocPRIM's stable radix sort of (key, node) over the bits of n_points + 1 values (skipped when n_points == 0);
//   * ext_runs    over that list: run bounds into point_len, reject bytes, point_grew (above);
//   * link_init / link_union / link_label on the FREE nodes, the second sort of (label, node), link_runs: track_uf.h;
//   * ext_flags   per node: observation? (low word) and, at the label of a new track, track? (high word) of one uint64, so that
//                 ONE exclusive scan numbers the observations and the new points; ADOPTED, REJECTED, CONFLICT and SHORT
//                 (component_verdict) counted in registers, then block_counts_add: LDS, one integer atomic per workgroup of a
//                 grid of at most 1024;
//   * ext_emit    every remaining entry of every output: node_point, the observation of a node at its rank (emit_obs), the padding
//                 past n_obs (pad_obs), point_len at the labels of the new tracks, point_new, totals.
// point_len and point_grew are zeroed to their capacity by one memset each before ext_runs; what is not a count of an old point,
// a new track's length or a grown point's byte stays zero.  The sorts and the scan are dev_prims.h's; both sorts share their
// output arrays.
#include <algorithm>
#include <climits>

#include "dev_prims.h"
#include "track_uf.h"

namespace {

using namespace gh_uf;

// the state byte; FREE is the value the shared union-find takes as "takes part"
constexpr uint8_t kMissing = 0, kFree = kUfLive, kMapped = 2, kClaimant = 3;

struct ExtArgs {
  const gh_keypoint* kps;
  int cap, N, n_points, PC;
  int min_views;
  Pinhole pin;
  const uint8_t* state;      // N
  const uint8_t* reject;     // N: 1 at a rejected claimant
  const int32_t* key1;       // N: the point of a MAPPED or CLAIMANT node
  const int32_t* key2;       // N: label of a FREE node, else N
  const int32_t* begin;      // N, by label: the component's range in the second sorted list
  const int32_t* end;
  const uint8_t* conflict;   // N, by label
  const uint64_t* rank;      // N + 1: exclusive scan of the flags; [N] = the totals
  const int32_t* counters;   // ADOPTED nodes, REJECTED nodes, CONFLICT components, SHORT components of two nodes or more
  int32_t* node_point;
  ObsOut obs;
  int32_t* point_len;
  uint8_t* point_new;
  int32_t* totals;
};

__global__ __launch_bounds__(kBlock) void ext_state_kernel(const int32_t* __restrict__ counts, int cap, int N,
                                                           const int32_t* __restrict__ node_point_in, int n_points,
                                                           const int32_t* __restrict__ row_point, const uint8_t* __restrict__ row_inlier,
                                                           uint8_t* __restrict__ state, int32_t* __restrict__ key,
                                                           int32_t* __restrict__ item) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int n = (int)g;
  const int f = n / cap, i = n - f * cap;
  uint8_t s = kMissing;
  int k = n_points;
  if (i < row_count(counts, f, cap)) {
    s = kFree;
    const int m = node_point_in ? node_point_in[n] : -1;
    if (m >= 0 && m < n_points) {
      s = kMapped;
      k = m;
    } else if (row_point && row_inlier[n] != 0) {
      const int c = row_point[n];
      if (c >= 0 && c < n_points) {
        s = kClaimant;
        k = c;
      }
    }
  }
  state[n] = s;
  key[n] = k;
  item[n] = n;
}

// over the list sorted by (point, node).  point_len[k] += (s + 1 at the run's last position) - (s at its first) - (1 per
// rejected claimant): the number of observations of the old point k.
__global__ __launch_bounds__(kBlock) void ext_runs_kernel(const int32_t* __restrict__ skey, const int32_t* __restrict__ list,
                                                          const uint8_t* __restrict__ state, int cap, int N, int n_points,
                                                          uint8_t* __restrict__ reject, int32_t* point_len, uint8_t* point_grew) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int s = (int)g;
  const int k = skey[s];
  if (k == n_points) return;  // (the nodes without a point come last)
  const bool same_prev = s > 0 && skey[s - 1] == k, same_next = s + 1 < N && skey[s + 1] == k;
  if (!same_prev) atomicSub(point_len + k, s);
  if (!same_next) atomicAdd(point_len + k, s + 1);
  const int a = list[s];
  if (state[a] != kClaimant) return;
  const int f = a / cap;
  if ((same_prev && list[s - 1] / cap == f) || (same_next && list[s + 1] / cap == f)) {
    reject[a] = 1;
    atomicSub(point_len + k, 1);
  } else {
    point_grew[k] = 1;
  }
}

__global__ __launch_bounds__(kBlock) void ext_flags_kernel(const uint8_t* __restrict__ state, const uint8_t* __restrict__ reject,
                                                           const int32_t* __restrict__ key2, const int32_t* __restrict__ begin,
                                                           const int32_t* __restrict__ end, const uint8_t* __restrict__ conflict, int N,
                                                           int min_views, uint64_t* __restrict__ flags, int32_t* __restrict__ counters) {
  int na = 0, nr = 0, nc = 0, ns = 0;  // the same in every lane of a wave
  const long long step = (long long)gridDim.x * kBlock;
  for (long long base = (long long)blockIdx.x * kBlock; base <= N; base += step) {  // (entry N is the scan's room for the totals)
    const long long g = base + threadIdx.x;
    bool is_adopted = false, is_rejected = false, is_conflict = false, is_short = false;
    if (g <= N) {
      const int n = (int)g;
      uint64_t f = 0;
      const uint8_t s = n < N ? state[n] : kMissing;
      if (s == kMapped) {
        f = 1u;
      } else if (s == kClaimant) {
        is_rejected = reject[n] != 0;
        is_adopted = !is_rejected;
        f = is_adopted ? 1u : 0u;
      } else if (s == kFree) {
        const int l = key2[n];
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
    na += wave_count(is_adopted);
    nr += wave_count(is_rejected);
    nc += wave_count(is_conflict);
    ns += wave_count(is_short);
  }
  block_counts_add<4>({na, nr, nc, ns}, counters);
}

__global__ __launch_bounds__(kBlock) void ext_emit_kernel(ExtArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;  // 0 .. max(N, PC) - 1
  const uint64_t total = a.rank[a.N];
  const int n_obs = (int)(uint32_t)total, n_total = a.n_points + (int)(total >> 32);
  if (g == 0) {
    a.totals[0] = n_obs;
    a.totals[1] = n_total;
    a.totals[2] = a.counters[0];
    a.totals[3] = a.counters[1];
    a.totals[4] = a.counters[2];
    a.totals[5] = a.counters[3];
  }
  if (g < a.PC) a.point_new[g] = (g >= a.n_points && g < n_total) ? 1 : 0;
  if (g >= a.N) return;
  const int n = (int)g;
  if (n >= n_obs) pad_obs(a.obs, n);
  const uint8_t s = a.state[n];
  int code = GH_LINK_NO_ROW;
  if (s == kMapped) {
    code = a.key1[n];
  } else if (s == kClaimant) {
    code = a.reject[n] ? GH_EXT_REJECTED : a.key1[n];
  } else if (s == kFree) {
    const int l = a.key2[n];
    const Component c = component_verdict(l, a.begin, a.end, a.conflict, a.min_views);
    if (c.verdict == kConflict) {
      code = GH_LINK_CONFLICT;
    } else if (c.verdict == kShort) {
      code = GH_LINK_SHORT;
    } else {
      code = a.n_points + (int)(a.rank[l] >> 32);
      if (n == l) a.point_len[code] = c.size;
    }
  }
  if (code >= 0) emit_obs(a.obs, (int)(uint32_t)a.rank[n], n / a.cap, code, n, a.kps[n], a.pin);
  a.node_point[n] = code;
}

// N == 0: the totals of an empty frame set
__global__ __launch_bounds__(kBlock) void ext_empty_kernel(int n_points, int32_t* __restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x < 6) totals[threadIdx.x] = threadIdx.x == 1 ? n_points : 0;
}

}  // namespace

extern "C" gh_status gh_extend_tracks_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                          const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                          const uint8_t* inlier_dev, const int32_t* node_point_in_dev, int n_points,
                                          const int32_t* row_point_dev, const uint8_t* row_inlier_dev, double fx, double fy, double cx,
                                          double cy, int min_views, int32_t* node_point_dev, int32_t* obs_cam_dev, int32_t* obs_point_dev,
                                          double* obs_xy_dev, int32_t* obs_node_dev, int32_t* point_len_dev, uint8_t* point_new_dev,
                                          uint8_t* point_grew_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n_frames >= 0 && cap >= 0 && npairs >= 0 && n_points >= 0 && cap <= 65535);
  GH_CHECK_ARG(ctx, (long long)n_points + (long long)n_frames * cap <= (long long)INT32_MAX - 1);
  GH_CHECK_ARG(ctx, min_views >= 2);
  GH_CHECK_ARG(ctx, fx > 0.0 && fy > 0.0);  // (a NaN fails)
  GH_CHECK_ARG(ctx, kps_dev && counts_dev);
  GH_CHECK_ARG(ctx, node_point_dev && obs_cam_dev && obs_point_dev && obs_xy_dev && obs_node_dev && point_len_dev && point_new_dev &&
                        point_grew_dev && totals_dev);
  GH_CHECK_ARG(ctx, npairs == 0 || (pair_q_dev && pair_t_dev && idx1_dev));
  GH_CHECK_ARG(ctx, (row_point_dev == nullptr) == (row_inlier_dev == nullptr));
  const int N = n_frames * cap;
  const int PC = n_points + N / 2;
  if (PC > 0) {
    GH_HIP(ctx, hipMemsetAsync(point_len_dev, 0, (size_t)PC * sizeof(int32_t), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(point_grew_dev, 0, (size_t)PC, ctx->stream));
  }
  if (N == 0) {
    if (PC > 0) GH_HIP(ctx, hipMemsetAsync(point_new_dev, 0, (size_t)PC, ctx->stream));
    GH_LAUNCH(ctx, "ext_empty", ext_empty_kernel, dim3(1), dim3(kBlock), 0, n_points, totals_dev);
    return GH_OK;
  }

  // The scratch block.  reject, conflict and the four counters are neighbours: one memset clears them (state has one writer per
  // byte, ext_state).  The rocPRIM storage serves the two sorts of N pairs and the scan of N + 1 flags.
  const size_t n = (size_t)N;
  const int bits1 = gh_key_bits(n_points), bits2 = gh_key_bits(N);
  const size_t sort1_bytes = gh_sort_pairs_bytes(ctx, n, bits1), sort2_bytes = gh_sort_pairs_bytes(ctx, n, bits2);
  const size_t scan_bytes = gh_scan_u64_bytes(ctx, n + 1);
  if (!sort1_bytes || !sort2_bytes || !scan_bytes) return gh_set_error(ctx, GH_ERR_HIP, "gh_extend_tracks_dev: rocPRIM size query failed");
  const size_t tmp_bytes = std::max(scan_bytes, std::max(sort1_bytes, sort2_bytes));
  gh_carve c;
  const size_t o_parent = c.take(n * 4), o_key1 = c.take(n * 4), o_key2 = c.take(n * 4), o_item = c.take(n * 4);
  const size_t o_skey = c.take(n * 4), o_list = c.take(n * 4), o_state = c.take(n);
  const size_t o_reject = c.take(n), o_conflict = c.take(n), o_counters = c.take(4 * sizeof(int32_t));
  const size_t o_flags = c.take((n + 1) * 8), o_rank = c.take((n + 1) * 8), o_tmp = c.take(tmp_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* parent = (int32_t*)(base + o_parent);
  int32_t* key1 = (int32_t*)(base + o_key1);
  int32_t* key2 = (int32_t*)(base + o_key2);
  int32_t* item = (int32_t*)(base + o_item);
  int32_t* skey = (int32_t*)(base + o_skey);
  int32_t* list = (int32_t*)(base + o_list);
  int32_t* begin = parent;  // (parent is dead after link_label)
  int32_t* end = item;      // (the sorts' input, dead after the second sort)
  uint8_t* state = (uint8_t*)(base + o_state);
  uint8_t* reject = (uint8_t*)(base + o_reject);
  uint8_t* conflict = (uint8_t*)(base + o_conflict);
  int32_t* counters = (int32_t*)(base + o_counters);
  uint64_t* flags = (uint64_t*)(base + o_flags);
  uint64_t* rank = (uint64_t*)(base + o_rank);
  void* tmp = base + o_tmp;

  const dim3 grid(gh_div_up(N, kBlock)), block(kBlock);
  GH_HIP(ctx, hipMemsetAsync(reject, 0, o_flags - o_reject, ctx->stream));
  GH_LAUNCH(ctx, "ext_state", ext_state_kernel, grid, block, 0, counts_dev, cap, N, node_point_in_dev, n_points, row_point_dev,
            row_inlier_dev, state, key1, item);
  if (n_points > 0) {  // (without a map there is nothing to keep and nothing to claim: every existing node is FREE)
    GH_TRY(gh_sort_pairs_i32(ctx, "ext_sort_points", "gh_extend_tracks_dev: first sort", tmp, tmp_bytes, key1, skey, item, list, n, bits1));
    GH_LAUNCH(ctx, "ext_runs", ext_runs_kernel, grid, block, 0, skey, list, state, cap, N, n_points, reject, point_len_dev,
              point_grew_dev);
  }
  GH_LAUNCH(ctx, "link_init", link_init_kernel, grid, block, 0, parent, N);
  const long long rows = (long long)npairs * cap;
  if (rows > 0) {
    const long long want = (rows + kBlock - 1) / kBlock;
    GH_LAUNCH(ctx, "link_union", link_union_kernel, dim3((unsigned)(want < kMaxUnionBlocks ? want : kMaxUnionBlocks)), block, 0,
              counts_dev, n_frames, cap, pair_q_dev, pair_t_dev, rows, idx1_dev, inlier_dev, (const uint8_t*)state, parent);
  }
  GH_LAUNCH(ctx, "link_label", link_label_kernel, grid, block, 0, counts_dev, cap, N, (const uint8_t*)state, parent, key2, item);
  GH_TRY(gh_sort_pairs_i32(ctx, "ext_sort_labels", "gh_extend_tracks_dev: second sort", tmp, tmp_bytes, key2, skey, item, list, n, bits2));
  GH_LAUNCH(ctx, "link_runs", link_runs_kernel, grid, block, 0, skey, list, cap, N, begin, end, conflict);
  const int flag_blocks = gh_div_up((long long)N + 1, kBlock);
  GH_LAUNCH(ctx, "ext_flags", ext_flags_kernel, dim3(flag_blocks < kMaxFlagBlocks ? flag_blocks : kMaxFlagBlocks), block, 0, state, reject,
            key2, begin, end, conflict, N, min_views, flags, counters);
  GH_TRY(gh_scan_u64(ctx, "ext_scan", "gh_extend_tracks_dev: scan", tmp, tmp_bytes, flags, rank, n + 1));

  const ExtArgs a = {kps_dev, cap, N, n_points, PC, min_views, {fx, fy, cx, cy},            // the inputs
                     state, reject, key1, key2, begin, end, conflict, rank, counters,       // scratch
                     node_point_dev, {obs_cam_dev, obs_point_dev, obs_xy_dev, obs_node_dev}, point_len_dev, point_new_dev, totals_dev};
  GH_LAUNCH(ctx, "ext_emit", ext_emit_kernel, dim3(gh_div_up(N > PC ? N : PC, kBlock)), block, 0, a);
  return GH_OK;
}
