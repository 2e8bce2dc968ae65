// New frames against the map, device-resident: gh_pnp_gather_pairs_dev (the 3D-2D gather) and gh_localize_pairs_dev (the gather,
// gh_pnp_batch_dev on its arrays, and the inlier bytes scattered back to keypoint rows).  The pair matcher has run between the
// new frames and map frames; a query row that hits a train row with a map point sees that point.  The contract is in
// include/gslam_hip.h; tests/localize_restate.py restates it on lists and dicts and the device is held to it byte for byte.
// Everything is integer work except the two divisions per correspondence, so the result is the same bits on every run.
//
// WHY THE VERDICTS DO NOT DEPEND ON A RACE.  A node is NO_POINT, AMBIGUOUS or a claimant according to min S and max S of its
// candidate set S.  loc_vote folds every candidate into lo[node] with an atomic minimum and into hi[node] with an atomic
// maximum: both are commutative, associative and idempotent, so the two words are functions of S alone, whatever the order of
// the pairs, the launch geometry or the arrival order (the same pair twice changes nothing).  Nobody reads lo / hi before the
// launch has ended: every later stage is a launch of its own on the same stream and takes plain loads.  SHARED is decided on the
// sorted list, where every writer stores the same byte 1; the counts are integer sums.
//
// CDNA4 mapping (the shared pieces are gh_map's, map_dev.h):
//   * loc_init    lo[n] = INT_MAX, hi[n] = -1;
//   * loc_vote    one lane per (pair, query row), grid-stride; pair_edge decides whether the row passes, then one read of the
//                 train node's point, the range and status tests, and the two atomics;
//   * loc_key     key[n] = lo[n] for an existing node with lo == hi, the extra bin n_points otherwise;
//   * sort        rocPRIM's stable radix sort of (key, node) over the bits of n_points + 1 values: within one point the nodes
//                 come in ascending id, so the claimants of one frame are neighbours.  No histogram per point: a popular map
//                 point would be one hot word;
//   * loc_runs    neighbours with one key below n_points and one frame both store the byte 1 to shared[node];
//   * loc_flags   per node: the code of row_point (written here), the flag "is a correspondence"; AMBIGUOUS and SHARED nodes
//                 counted in registers, then block_counts_add: LDS, one integer atomic per workgroup; grid-stride over at most
//                 1024 workgroups; entry N of the flags is the scan's room for the total;
//   * scan        one rocPRIM exclusive scan; offsets[f] is its value at node f * cap, so the offsets cost nothing extra;
//   * loc_emit    every remaining entry of every output exactly once: the correspondence of a node at its rank, the padding past
//                 n_corr, offsets, totals (the frames with a correspondence: one ballot per wave of frames, integer atomics on
//                 a word the call zeroed);
//   * loc_scatter composed call only, after a memset of row_inlier: one lane per correspondence k < n_corr (read from
//                 offsets[n_frames] on the device) stores its inlier byte at corr_node[k].
// The sort and the scan are dev_prims.h's; the work space comes from the context's scratch.  The
// composed call takes ONE scratch block: inlier bytes | n_inliers | the block of the stage that runs (the gather's is dead when
// gh_pnp_batch_dev's begins: every result of the gather lives in the caller's arrays).
#include <algorithm>
#include <climits>

#include "dev_prims.h"
#include "estimate_batch.h"
#include "map_dev.h"

namespace {

using namespace gh_map;

constexpr int kMaxVoteBlocks = 1 << 16;  // grid-stride beyond this many workgroups

struct GatherIn {
  const gh_keypoint* kps;
  const int32_t* counts;
  int n_frames, cap;
  const int32_t* pair_q;
  const int32_t* pair_t;
  int npairs;
  const int32_t* idx1;
  const uint8_t* keep;
  const int32_t* node_point;
  int n_points;
  const double* point_xyz;
  const int32_t* point_status;
  double fx, fy, cx, cy;
  int32_t* row_point;
  int32_t* offsets;
  double* xyz;
  double* xy;
  int32_t* corr_node;
  int32_t* totals;
};

struct EmitArgs {
  const gh_keypoint* kps;
  int n_frames, cap, N;
  Pinhole pin;
  const double* point_xyz;
  const int32_t* row_point;  // written by loc_flags
  const int32_t* rank;       // N + 1: exclusive scan of the flags; [N] = n_corr
  const int32_t* counters;   // AMBIGUOUS nodes, SHARED nodes
  int32_t* offsets;
  double* xyz;
  double* xy;
  int32_t* corr_node;
  int32_t* totals;           // [3] is zero when loc_emit starts
};

__global__ __launch_bounds__(kBlock) void loc_init_kernel(int32_t* __restrict__ lo, int32_t* __restrict__ hi, int N) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  lo[g] = INT_MAX;
  hi[g] = -1;
}

__global__ __launch_bounds__(kBlock) void loc_vote_kernel(const int32_t* __restrict__ counts, int n_frames, int cap,
                                                          const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_t,
                                                          long long rows, const int32_t* __restrict__ idx1,
                                                          const uint8_t* __restrict__ keep, const int32_t* __restrict__ node_point,
                                                          int n_points, const int32_t* __restrict__ point_status, int32_t* lo,
                                                          int32_t* hi) {
  const PairRows e = {counts, n_frames, cap, pair_q, pair_t, idx1, keep};
  const long long step = (long long)gridDim.x * kBlock;
  for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < rows; r += step) {
    int u, v;
    if (!pair_edge(e, r, &u, &v)) continue;
    const int c = node_point[v];
    if (c < 0 || c >= n_points) continue;
    if (point_status && point_status[c] != GH_TRACK_OK) continue;
    (void)__hip_atomic_fetch_min(lo + u, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(hi + u, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kBlock) void loc_key_kernel(const int32_t* __restrict__ counts, int cap, int N, int n_points,
                                                         const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                         int32_t* __restrict__ key, int32_t* __restrict__ item) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int n = (int)g;
  const int f = n / cap, i = n - f * cap;
  const int l = lo[n];
  key[n] = (i < row_count(counts, f, cap) && l == hi[n]) ? l : n_points;  // (no candidate: INT_MAX != -1)
  item[n] = n;
}

__global__ __launch_bounds__(kBlock) void loc_runs_kernel(const int32_t* __restrict__ skey, const int32_t* __restrict__ list, int cap,
                                                          int N, int n_points, uint8_t* __restrict__ shared) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g + 1 >= N) return;
  const int s = (int)g;
  const int l = skey[s];
  if (l == n_points || skey[s + 1] != l) return;  // (the nodes that claim nothing come last)
  const int a = list[s], b = list[s + 1];
  if (a / cap == b / cap) {
    shared[a] = 1;
    shared[b] = 1;
  }
}

__global__ __launch_bounds__(kBlock) void loc_flags_kernel(const int32_t* __restrict__ counts, int cap, int N, int n_points,
                                                           const int32_t* __restrict__ key, const int32_t* __restrict__ lo,
                                                           const int32_t* __restrict__ hi, const uint8_t* __restrict__ shared,
                                                           int32_t* __restrict__ flags, int32_t* __restrict__ row_point,
                                                           int32_t* __restrict__ counters) {
  int na = 0, ns = 0;  // the same in every lane of a wave
  const long long step = (long long)gridDim.x * kBlock;
  for (long long base = (long long)blockIdx.x * kBlock; base <= N; base += step) {  // (entry N is the scan's room for the total)
    const long long g = base + threadIdx.x;
    bool is_ambiguous = false, is_shared = false;
    if (g <= N) {
      const int n = (int)g;
      int flag = 0;
      if (n < N) {
        const int f = n / cap, i = n - f * cap;
        int code = GH_LOC_NO_ROW;
        if (i < row_count(counts, f, cap)) {
          const int k = key[n];
          if (k != n_points) {
            is_shared = shared[n] != 0;
            flag = is_shared ? 0 : 1;
            code = is_shared ? GH_LOC_SHARED : k;
          } else {
            is_ambiguous = hi[n] >= 0 && lo[n] != hi[n];
            code = is_ambiguous ? GH_LOC_AMBIGUOUS : GH_LOC_NO_POINT;
          }
        }
        row_point[n] = code;
      }
      flags[n] = flag;
    }
    na += wave_count(is_ambiguous);
    ns += wave_count(is_shared);
  }
  block_counts_add<2>({na, ns}, counters);
}

__global__ __launch_bounds__(kBlock) void loc_emit_kernel(EmitArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;  // 0 .. N: N + 1 >= n_frames + 1 lanes because cap >= 1
  const int n_corr = a.rank[a.N];
  bool frame_has = false;
  if (g <= a.n_frames) {
    const int f = (int)g;
    const int first = a.rank[f * a.cap];
    a.offsets[f] = first;
    frame_has = f < a.n_frames && a.rank[(f + 1) * a.cap] > first;
  }
  if (g <= ((long long)a.n_frames | 63)) {  // the waves that hold a frame, whole: the ballot is wave-uniform
    const int has = __popcll(__ballot(frame_has));
    if ((threadIdx.x & 63) == 0 && has) atomicAdd(a.totals + 3, has);
  }
  if (g >= a.N) return;
  const int n = (int)g;
  if (n == 0) {
    a.totals[0] = n_corr;
    a.totals[1] = a.counters[0];
    a.totals[2] = a.counters[1];
  }
  if (n >= n_corr) {  // the padding; the entries below n_corr are written by the nodes that own them
    a.xyz[3 * (size_t)n] = 0.0;
    a.xyz[3 * (size_t)n + 1] = 0.0;
    a.xyz[3 * (size_t)n + 2] = 0.0;
    a.xy[2 * (size_t)n] = 0.0;
    a.xy[2 * (size_t)n + 1] = 0.0;
    a.corr_node[n] = -1;
  }
  const int c = a.row_point[n];
  if (c < 0) return;
  const int k = a.rank[n];
  a.xyz[3 * (size_t)k] = a.point_xyz[3 * (size_t)c];
  a.xyz[3 * (size_t)k + 1] = a.point_xyz[3 * (size_t)c + 1];
  a.xyz[3 * (size_t)k + 2] = a.point_xyz[3 * (size_t)c + 2];
  normalised_xy(a.kps[n], a.pin, a.xy + 2 * (size_t)k);
  a.corr_node[k] = n;
}

__global__ __launch_bounds__(kBlock) void loc_scatter_kernel(const int32_t* __restrict__ corr_node, const int32_t* __restrict__ n_corr_dev,
                                                             const uint8_t* __restrict__ inlier, int N, uint8_t* __restrict__ row_inlier) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int n_corr = *n_corr_dev;
  if (g >= N || g >= n_corr) return;
  const int node = corr_node[g];
  if (node >= 0 && node < N && inlier[g]) row_inlier[node] = 1;
}

// The gather's scratch block: lo | hi | key | sorted keys | item | list | shared bytes, two counters (one memset) | flags | rank |
// rocPRIM storage, which serves the sort of N pairs and the scan of N + 1 flags.  (Not carved with gh_carve: six equal segments
// and five offsets are shorter this way.)
struct GatherLayout {
  int bits;  // of the sort: the keys are 0 .. n_points
  size_t ints, o_shared, o_counters, o_flags, o_rank, o_tmp, tmp_bytes, total;
};

bool gather_layout(gh_ctx* ctx, int N, int n_points, GatherLayout* L) {
  const size_t n = (size_t)N;
  L->bits = gh_key_bits(n_points);
  const size_t sort_bytes = gh_sort_pairs_bytes(ctx, n, L->bits), scan_bytes = gh_scan_i32_bytes(ctx, n + 1);
  if (!sort_bytes || !scan_bytes) return false;
  L->tmp_bytes = std::max(sort_bytes, scan_bytes);
  L->ints = gh_round256(n * 4);
  L->o_shared = 6 * L->ints;
  L->o_counters = L->o_shared + gh_round256(n);
  L->o_flags = L->o_counters + 256;
  L->o_rank = L->o_flags + gh_round256((n + 1) * 4);
  L->o_tmp = L->o_rank + gh_round256((n + 1) * 4);
  L->total = L->o_tmp + L->tmp_bytes;
  return true;
}

// 0: fine; otherwise the number of the check that failed (the entries name it)
int gather_args_bad(const GatherIn& g) {
  if (!(g.n_frames >= 0 && g.cap >= 0 && g.npairs >= 0 && g.n_points >= 0 && g.cap <= 65535)) return 1;
  if (!((long long)g.n_frames * g.cap <= (long long)INT32_MAX - 1)) return 2;
  if (!(g.fx > 0.0 && g.fy > 0.0)) return 3;  // (a NaN fails)
  if (!(g.kps && g.counts && g.node_point)) return 4;
  if (!(g.row_point && g.offsets && g.xyz && g.xy && g.corr_node && g.totals)) return 5;
  if (!(g.n_points == 0 || g.point_xyz)) return 6;
  if (!(g.npairs == 0 || (g.pair_q && g.pair_t && g.idx1))) return 7;
  return 0;
}

// The gather on `base` (gather_layout's total bytes); the arguments have been checked.
gh_status gather_on(gh_ctx* ctx, const GatherIn& g, const GatherLayout& L, char* base) {
  const int N = g.n_frames * g.cap;
  if (N == 0) {
    GH_HIP(ctx, hipMemsetAsync(g.offsets, 0, ((size_t)g.n_frames + 1) * sizeof(int32_t), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(g.totals, 0, 4 * sizeof(int32_t), ctx->stream));
    return GH_OK;
  }
  const size_t n = (size_t)N;
  int32_t* lo = (int32_t*)base;
  int32_t* hi = (int32_t*)(base + L.ints);
  int32_t* key = (int32_t*)(base + 2 * L.ints);
  int32_t* skey = (int32_t*)(base + 3 * L.ints);
  int32_t* item = (int32_t*)(base + 4 * L.ints);
  int32_t* list = (int32_t*)(base + 5 * L.ints);
  uint8_t* shared = (uint8_t*)(base + L.o_shared);
  int32_t* counters = (int32_t*)(base + L.o_counters);
  int32_t* flags = (int32_t*)(base + L.o_flags);
  int32_t* rank = (int32_t*)(base + L.o_rank);
  void* tmp = base + L.o_tmp;

  const dim3 grid(gh_div_up(N, kBlock)), block(kBlock);
  GH_HIP(ctx, hipMemsetAsync(shared, 0, L.o_flags - L.o_shared, ctx->stream));
  GH_HIP(ctx, hipMemsetAsync(g.totals + 3, 0, sizeof(int32_t), ctx->stream));
  GH_LAUNCH(ctx, "loc_init", loc_init_kernel, grid, block, 0, lo, hi, N);
  const long long rows = (long long)g.npairs * g.cap;
  if (rows > 0 && g.n_points > 0) {
    const long long want = (rows + kBlock - 1) / kBlock;
    GH_LAUNCH(ctx, "loc_vote", loc_vote_kernel, dim3((unsigned)(want < kMaxVoteBlocks ? want : kMaxVoteBlocks)), block, 0, g.counts,
              g.n_frames, g.cap, g.pair_q, g.pair_t, rows, g.idx1, g.keep, g.node_point, g.n_points, g.point_status, lo, hi);
  }
  GH_LAUNCH(ctx, "loc_key", loc_key_kernel, grid, block, 0, g.counts, g.cap, N, g.n_points, lo, hi, key, item);
  GH_TRY(gh_sort_pairs_i32(ctx, "loc_sort", "gh_pnp_gather_pairs_dev: sort", tmp, L.tmp_bytes, key, skey, item, list, n, L.bits));
  GH_LAUNCH(ctx, "loc_runs", loc_runs_kernel, grid, block, 0, skey, list, g.cap, N, g.n_points, shared);
  const int flag_blocks = gh_div_up((long long)N + 1, kBlock);
  GH_LAUNCH(ctx, "loc_flags", loc_flags_kernel, dim3(flag_blocks < kMaxFlagBlocks ? flag_blocks : kMaxFlagBlocks), block, 0, g.counts, g.cap,
            N, g.n_points, key, lo, hi, shared, flags, g.row_point, counters);
  GH_TRY(gh_scan_i32(ctx, "loc_scan", "gh_pnp_gather_pairs_dev: scan", tmp, L.tmp_bytes, flags, rank, n + 1));

  const EmitArgs a = {g.kps, g.n_frames, g.cap, N, {g.fx, g.fy, g.cx, g.cy}, g.point_xyz, g.row_point,  // the inputs
                      rank, counters,                                                               // scratch
                      g.offsets, g.xyz, g.xy, g.corr_node, g.totals};
  GH_LAUNCH(ctx, "loc_emit", loc_emit_kernel, dim3(gh_div_up((long long)N + 1, kBlock)), block, 0, a);
  return GH_OK;
}

}  // namespace

extern "C" gh_status gh_pnp_gather_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                             const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                             const uint8_t* keep_dev, const int32_t* node_point_dev, int n_points,
                                             const double* point_xyz_dev, const int32_t* point_status_dev, double fx, double fy,
                                             double cx, double cy, int32_t* row_point_dev, int32_t* offsets_dev, double* xyz_dev,
                                             double* xy_dev, int32_t* corr_node_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  const GatherIn g = {kps_dev, counts_dev, n_frames, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev, keep_dev, node_point_dev, n_points,
                      point_xyz_dev, point_status_dev, fx, fy, cx, cy, row_point_dev, offsets_dev, xyz_dev, xy_dev, corr_node_dev,
                      totals_dev};
  const int bad = gather_args_bad(g);
  if (bad) return gh_set_error(ctx, GH_ERR_ARG, "gh_pnp_gather_pairs_dev: argument check %d failed", bad);
  GatherLayout L = {};
  char* base = nullptr;
  if (n_frames * cap > 0) {
    if (!gather_layout(ctx, n_frames * cap, n_points, &L))
      return gh_set_error(ctx, GH_ERR_HIP, "gh_pnp_gather_pairs_dev: rocPRIM size query failed");
    GH_TRY(gh_scratch(ctx, L.total, (void**)&base));
  }
  return gather_on(ctx, g, L, base);
}

extern "C" gh_status gh_localize_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                           const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                           const uint8_t* keep_dev, const int32_t* node_point_dev, int n_points,
                                           const double* point_xyz_dev, const int32_t* point_status_dev, double fx, double fy,
                                           double cx, double cy, double ransac_threshold, uint64_t seed, int dof,
                                           const gh_ba_options* options, int min_rows, double inlier_threshold, int32_t* row_point_dev,
                                           int32_t* offsets_dev, double* xyz_dev, double* xy_dev, int32_t* corr_node_dev,
                                           int32_t* totals_dev, double* models_dev, int32_t* ransac_inliers_dev, double* poses_dev,
                                           double* info_dev, gh_pnp_batch_summary* summaries_dev, uint8_t* row_inlier_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  const GatherIn g = {kps_dev, counts_dev, n_frames, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev, keep_dev, node_point_dev, n_points,
                      point_xyz_dev, point_status_dev, fx, fy, cx, cy, row_point_dev, offsets_dev, xyz_dev, xy_dev, corr_node_dev,
                      totals_dev};
  const int bad = gather_args_bad(g);
  if (bad) return gh_set_error(ctx, GH_ERR_ARG, "gh_localize_pairs_dev: argument check %d failed", bad);
  const int N = n_frames * cap;
  GH_CHECK_ARG(ctx, gh_ransac::pnp_batch_args_ok(n_frames, N, ransac_threshold, min_rows, inlier_threshold));
  GH_CHECK_ARG(ctx, n_frames == 0 || (models_dev && ransac_inliers_dev && poses_dev && summaries_dev));
  GH_CHECK_ARG(ctx, row_inlier_dev);

  // ONE scratch block (gh_scratch hands out one block per context): inlier bytes | n_inliers | the stage's own block
  GatherLayout L = {};
  if (N > 0 && !gather_layout(ctx, N, n_points, &L))
    return gh_set_error(ctx, GH_ERR_HIP, "gh_localize_pairs_dev: rocPRIM size query failed");
  const size_t o_n_inliers = gh_round256((size_t)N), o_stage = o_n_inliers + gh_round256((size_t)n_frames * 4);
  const size_t stage = std::max(L.total, gh_ransac::pnp_batch_scratch_bytes(n_frames, N));
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, o_stage + stage, (void**)&base));
  uint8_t* inlier = (uint8_t*)base;
  int32_t* n_inliers = (int32_t*)(base + o_n_inliers);

  GH_TRY(gather_on(ctx, g, L, base + o_stage));
  if (n_frames == 0) return GH_OK;
  GH_TRY(gh_ransac::pnp_batch_on(ctx, xyz_dev, xy_dev, offsets_dev, n_frames, N, ransac_threshold, seed, dof, options, min_rows,
                                 inlier_threshold, models_dev, ransac_inliers_dev, poses_dev, info_dev, summaries_dev, inlier, n_inliers,
                                 base + o_stage));
  if (N == 0) return GH_OK;
  GH_HIP(ctx, hipMemsetAsync(row_inlier_dev, 0, (size_t)N, ctx->stream));
  GH_LAUNCH(ctx, "loc_scatter", loc_scatter_kernel, dim3(gh_div_up(N, kBlock)), dim3(kBlock), 0, corr_node_dev, offsets_dev + n_frames,
            inlier, N, row_inlier_dev);
  return GH_OK;
}
