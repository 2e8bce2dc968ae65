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
// CDNA4 mapping (the skeleton of track_link.hip and localize.hip):
//   * ext_state   one lane per node: the state byte and the key of the first sort (the point of a MAPPED or CLAIMANT node, the
//                 extra bin n_points otherwise), item[n] = n;
//   * sort        rocPRIM's stable radix sort of (key, node) over the bits of n_points + 1 values (skipped when n_points == 0);
//   * ext_runs    over that list: run bounds into point_len, reject bytes, point_grew (above);
//   * link_init / link_union / link_label on the FREE nodes, the second sort of (label, node), link_runs: track_uf.h;
//   * ext_flags   per node: observation? (low word) and, at the label of a new track, track? (high word) of one uint64, so that
//                 ONE exclusive scan numbers the observations and the new points; ADOPTED, REJECTED, CONFLICT and SHORT counted in
//                 registers, then LDS, then one integer atomic per workgroup of a grid of at most 1024;
//   * ext_emit    every remaining entry of every output: node_point, the observation of a node at its rank, the padding past
//                 n_obs, point_len at the labels of the new tracks, point_new, totals.
// point_len and point_grew are zeroed to their capacity by one memset each before ext_runs; what is not a count of an old point,
// a new track's length or a grown point's byte stays zero.  One context scratch block: parent | key1 | key2 | item | sorted
// keys | list | state, reject and conflict bytes, four counters (one memset) | flags | rank | rocPRIM storage; begin lives in
// parent's place (dead after link_label), end in item's (dead after the second sort), both sorts share their output arrays.
#include <climits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "track_uf.h"

namespace {

using namespace gh_uf;

constexpr int kMaxFlagBlocks = 1024;
// the state byte; FREE is the value the shared union-find takes as "takes part"
constexpr uint8_t kMissing = 0, kFree = kUfLive, kMapped = 2, kClaimant = 3;

struct ExtArgs {
  const gh_keypoint* kps;
  int cap, N, n_points, PC;
  int min_views;
  double fx, fy, cx, cy;
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
  int32_t* obs_cam;
  int32_t* obs_point;
  double* obs_xy;
  int32_t* obs_node;
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
  if (i < link_count(counts, f, cap)) {
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
  __shared__ int s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
  __syncthreads();
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
        const int size = end[l] - begin[l];
        const bool bad = conflict[l] != 0;
        const bool track = !bad && size >= min_views;
        f = track ? 1u : 0u;
        if (n == l) {
          if (track) f |= 1ull << 32;
          is_conflict = bad;
          is_short = !bad && !track && size >= 2;
        }
      }
      flags[n] = f;
    }
    na += __popcll(__ballot(is_adopted));
    nr += __popcll(__ballot(is_rejected));
    nc += __popcll(__ballot(is_conflict));
    ns += __popcll(__ballot(is_short));
  }
  if ((threadIdx.x & 63) == 0) {
    if (na) atomicAdd(&s_count[0], na);
    if (nr) atomicAdd(&s_count[1], nr);
    if (nc) atomicAdd(&s_count[2], nc);
    if (ns) atomicAdd(&s_count[3], ns);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(counters + threadIdx.x, s_count[threadIdx.x]);
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
  if (n >= n_obs) {  // the padding; the entries below n_obs are written by the nodes that own them
    a.obs_cam[n] = -1;
    a.obs_point[n] = -1;
    a.obs_node[n] = -1;
    a.obs_xy[2 * (size_t)n] = 0.0;
    a.obs_xy[2 * (size_t)n + 1] = 0.0;
  }
  const uint8_t s = a.state[n];
  int code = GH_LINK_NO_ROW;
  if (s == kMapped) {
    code = a.key1[n];
  } else if (s == kClaimant) {
    code = a.reject[n] ? GH_EXT_REJECTED : a.key1[n];
  } else if (s == kFree) {
    const int l = a.key2[n];
    const int size = a.end[l] - a.begin[l];
    if (a.conflict[l]) {
      code = GH_LINK_CONFLICT;
    } else if (size < a.min_views) {
      code = GH_LINK_SHORT;
    } else {
      code = a.n_points + (int)(a.rank[l] >> 32);
      if (n == l) a.point_len[code] = size;
    }
  }
  if (code >= 0) {
    const int k = (int)(uint32_t)a.rank[n];
    const float x = a.kps[n].x, y = a.kps[n].y;
    a.obs_cam[k] = n / a.cap;
    a.obs_point[k] = code;
    a.obs_node[k] = n;
    a.obs_xy[2 * (size_t)k] = ((double)x - a.cx) / a.fx;
    a.obs_xy[2 * (size_t)k + 1] = ((double)y - a.cy) / a.fy;
  }
  a.node_point[n] = code;
}

// N == 0: the totals of an empty frame set
__global__ __launch_bounds__(kBlock) void ext_empty_kernel(int n_points, int32_t* __restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x < 6) totals[threadIdx.x] = threadIdx.x == 1 ? n_points : 0;
}

// temporary storage that serves the two sorts of N pairs and the scan of N + 1 flags
bool ext_rocprim_bytes(hipStream_t stream, int N, int n_points, size_t* bytes) {
  uint64_t* null_u = nullptr;
  int32_t* null_i = nullptr;
  size_t scan = 0, sort1 = 0, sort2 = 0;
  if (rocprim::exclusive_scan(nullptr, scan, null_u, null_u, (uint64_t)0, (size_t)N + 1, rocprim::plus<uint64_t>(), stream) != hipSuccess ||
      rocprim::radix_sort_pairs(nullptr, sort1, null_i, null_i, null_i, null_i, (size_t)N, 0, key_bits(n_points), stream) != hipSuccess ||
      rocprim::radix_sort_pairs(nullptr, sort2, null_i, null_i, null_i, null_i, (size_t)N, 0, key_bits(N), stream) != hipSuccess)
    return false;
  *bytes = gh_round256(std::max(std::max(scan, std::max(sort1, sort2)), (size_t)1));
  return true;
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

  const size_t n = (size_t)N;
  size_t tmp_bytes = 0;
  if (!ext_rocprim_bytes(ctx->stream, N, n_points, &tmp_bytes))
    return gh_set_error(ctx, GH_ERR_HIP, "gh_extend_tracks_dev: rocPRIM size query failed");
  const size_t ints = gh_round256(n * 4), bytes = gh_round256(n);
  const size_t o_key1 = ints, o_key2 = 2 * ints, o_item = 3 * ints, o_skey = 4 * ints, o_list = 5 * ints, o_state = 6 * ints;
  const size_t o_reject = o_state + bytes, o_conflict = o_reject + bytes, o_counters = o_conflict + bytes;
  const size_t o_flags = o_counters + 256;
  const size_t o_rank = o_flags + gh_round256((n + 1) * 8);
  const size_t o_tmp = o_rank + gh_round256((n + 1) * 8);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, o_tmp + tmp_bytes, (void**)&base));
  int32_t* parent = (int32_t*)base;
  int32_t* key1 = (int32_t*)(base + o_key1);
  int32_t* key2 = (int32_t*)(base + o_key2);
  int32_t* item = (int32_t*)(base + o_item);
  int32_t* skey = (int32_t*)(base + o_skey);
  int32_t* list = (int32_t*)(base + o_list);
  int32_t *begin = parent, *end = item;
  uint8_t* state = (uint8_t*)(base + o_state);
  uint8_t* reject = (uint8_t*)(base + o_reject);
  uint8_t* conflict = (uint8_t*)(base + o_conflict);
  int32_t* counters = (int32_t*)(base + o_counters);
  uint64_t* flags = (uint64_t*)(base + o_flags);
  uint64_t* rank = (uint64_t*)(base + o_rank);

  const dim3 grid(gh_div_up(N, kBlock)), block(kBlock);
  GH_HIP(ctx, hipMemsetAsync(reject, 0, o_flags - o_reject, ctx->stream));
  GH_LAUNCH(ctx, "ext_state", ext_state_kernel, grid, block, 0, counts_dev, cap, N, node_point_in_dev, n_points, row_point_dev,
            row_inlier_dev, state, key1, item);
  if (n_points > 0) {  // (without a map there is nothing to keep and nothing to claim: every existing node is FREE)
    {
      const int prof = gh_prof_begin(ctx, "ext_sort_points");
      size_t tb = tmp_bytes;
      const hipError_t e = rocprim::radix_sort_pairs(base + o_tmp, tb, key1, skey, item, list, n, 0, key_bits(n_points), ctx->stream);
      gh_prof_end(ctx, prof);
      if (e != hipSuccess) return gh_set_error(ctx, GH_ERR_HIP, "gh_extend_tracks_dev: first sort");
    }
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
  {
    const int prof = gh_prof_begin(ctx, "ext_sort_labels");
    size_t tb = tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(base + o_tmp, tb, key2, skey, item, list, n, 0, key_bits(N), ctx->stream);
    gh_prof_end(ctx, prof);
    if (e != hipSuccess) return gh_set_error(ctx, GH_ERR_HIP, "gh_extend_tracks_dev: second sort");
  }
  GH_LAUNCH(ctx, "link_runs", link_runs_kernel, grid, block, 0, skey, list, cap, N, begin, end, conflict);
  const int flag_blocks = gh_div_up((long long)N + 1, kBlock);
  GH_LAUNCH(ctx, "ext_flags", ext_flags_kernel, dim3(flag_blocks < kMaxFlagBlocks ? flag_blocks : kMaxFlagBlocks), block, 0, state, reject,
            key2, begin, end, conflict, N, min_views, flags, counters);
  {
    const int prof = gh_prof_begin(ctx, "ext_scan");
    size_t tb = tmp_bytes;
    const hipError_t e = rocprim::exclusive_scan(base + o_tmp, tb, flags, rank, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream);
    gh_prof_end(ctx, prof);
    if (e != hipSuccess) return gh_set_error(ctx, GH_ERR_HIP, "gh_extend_tracks_dev: scan");
  }

  ExtArgs a = {};
  a.kps = kps_dev;
  a.cap = cap;
  a.N = N;
  a.n_points = n_points;
  a.PC = PC;
  a.min_views = min_views;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.state = state;
  a.reject = reject;
  a.key1 = key1;
  a.key2 = key2;
  a.begin = begin;
  a.end = end;
  a.conflict = conflict;
  a.rank = rank;
  a.counters = counters;
  a.node_point = node_point_dev;
  a.obs_cam = obs_cam_dev;
  a.obs_point = obs_point_dev;
  a.obs_xy = obs_xy_dev;
  a.obs_node = obs_node_dev;
  a.point_len = point_len_dev;
  a.point_new = point_new_dev;
  a.totals = totals_dev;
  GH_LAUNCH(ctx, "ext_emit", ext_emit_kernel, dim3(gh_div_up(N > PC ? N : PC, kBlock)), block, 0, a);
  return GH_OK;
}
