// Map-point summaries, device-resident: gh_describe_points_dev.  A map point here is an id, three doubles and a status; a search
// by projection or a fusion of duplicates needs three more things per point, the ones ORB-SLAM keeps in
// MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth: the descriptor of the observation closest (by median Hamming
// distance) to the point's other observations, the mean direction from which the point was seen, and the distance range over
// which the octave of its reference keypoint predicts it can be found again.  The map's arrays go in as gh_extend_tracks_dev,
// gh_merge_points_dev and gh_triangulate_tracks_dev leave them, padding included.  The contract is in include/gslam_hip.h;
// tests/point_describe_restate.py restates it in plain Python and the device is held to it byte for byte.
//
// WHY THE BITS DO NOT DEPEND ON A RACE.  Every output entry has one writer.  The descriptor is integer work (xor, popcount, a
// selection, a minimum with the candidate index as the tie-break).  The direction is a sum of IEEE doubles in a FIXED order:
// lane j of a point's group of eight adds the unit rays of the live indices j, j + 8, ... in ascending order, and the eight
// partials meet in the __shfl_xor butterfly over 4, 2, 1 of tracks.hip, which is ((s0+s4)+(s2+s6))+((s1+s5)+(s3+s7)) in every
// lane.  The library is built with -ffp-contract=off: nothing is fused.  The four totals are integer atomic adds on words the
// call zeroed, after a reduction inside the workgroup (gh_map::block_counts_add).  No float atomic anywhere.
//
// CDNA4 mapping (the shared pieces are gh_map's, map_dev.h, and gh_csr_index_dev's, csr_sort.hip):
//   * pdsc_keys    one lane per observation: its point when the observation is USABLE, one of the spare bins from n_points on
//                  otherwise (an index out of range is never dereferenced; why the bins are many: map_dev.h, THE SPARE BINS);
//   * index        gh_csr_index_dev turns the keys into start / list: the track of a point in ascending observation index,
//                  whatever order the caller's arrays have;
//   * pdsc_narrow  one group of 8 lanes per point, 8 points per wave, 32 per 256-thread workgroup: state, views, direction, range
//                  and the totals for every point; a long track costs its group linear work.  With M <= 8 candidates it also
//                  chooses the descriptor: lane c keeps candidate c in 8 registers, eight rounds of width-8 shuffles give every
//                  lane its row of distances in registers, the median comes from counting ranks, the winner from a three-step
//                  minimum of (median, c).  No LDS beyond the counters' words;
//   * pdsc_wide    one wave per point with M > 8 (every other point leaves after three loads): lane a keeps candidate a, the loop
//                  over b broadcasts candidate b and lane a stores d(a, b) as u16 at [b][a] of its wave's 8 KB of LDS -- a lane
//                  writes and later reads only its own column, so there is no barrier -- then a nine-step value search gives the
//                  lane its median and a six-step minimum of (median, a) the winner, who writes its 32 bytes.
#include <climits>
#include <cmath>

#include "map_host.h"

namespace {

using gh_map::hamming256;
using gh_map::kBlock;
using gh_map::kMaxLevels;

constexpr int kGroupLanes = 8;                        // the group of gh_triangulate_tracks_dev: the summation order depends on it
constexpr int kPointsPerBlock = kBlock / kGroupLanes;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxViews = 64;                         // one candidate per lane of a wave
constexpr unsigned long long kQuietNaN = 0x7ff8000000000000ull;

struct DescArgs {
  const gh_keypoint* kps;
  const uint32_t* desc;  // 8 words per node
  const double* cam_pose;
  const int32_t* obs_node;
  const double* point_xyz;
  const int32_t* point_status;  // may be NULL
  const uint8_t* point_select;  // may be NULL
  const int32_t* start;         // n_points + 1 entries are read (the bins from n_points on hold what is not usable)
  const int32_t* list;
  int n_points, cap, n_levels, max_views;
  uint8_t* state;
  uint32_t* out_desc;
  int32_t* out_obs;
  int32_t* views;
  double* normal;
  double* dist;
  int32_t* totals;
};

__global__ __launch_bounds__(kBlock) void pdsc_keys_kernel(const int32_t* __restrict__ counts, int cap, int N,
                                                           const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                           const int32_t* __restrict__ obs_node, const uint8_t* __restrict__ obs_use,
                                                           int n_obs, int n_points, int spare_mask, int32_t* __restrict__ key) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n_obs) return;
  bool usable = !obs_use || obs_use[k] != 0;
  const int p = obs_point[k], n = obs_node[k];
  usable = usable && p >= 0 && p < n_points && n >= 0 && n < N;
  if (usable) {  // (N > 0 here, so cap > 0)
    const int f = n / cap;
    usable = n - f * cap < gh_map::row_count(counts, f, cap) && obs_cam[k] == f;
  }
  key[k] = usable ? p : gh_map::spare_key(n_points, k, spare_mask);
}

// the live index of candidate c of a track of L observations with M = min(L, max_views) candidates
__device__ __forceinline__ int candidate_index(int c, int L, int M) { return L == M ? c : (int)(((long long)c * L) / M); }

// a NaN leaves as the one quiet NaN with a clear sign and no payload: IEEE 754 fixes neither for a NaN that an operation makes
__device__ __forceinline__ double canonical(double x) { return x != x ? __longlong_as_double((long long)kQuietNaN) : x; }

__global__ __launch_bounds__(kBlock) void pdsc_narrow_kernel(DescArgs a, gh_map::ScalePowers pw) {
  const int tid = threadIdx.x, j = tid & (kGroupLanes - 1);
  const long long gp = (long long)blockIdx.x * kPointsPerBlock + (tid >> 3);
  const bool in_range = gp < a.n_points;
  const int p = in_range ? (int)gp : 0;
  int state = GH_PDESC_SKIPPED, first = 0, L = 0;
  if (in_range && (!a.point_select || a.point_select[p] != 0)) {
    if (a.point_status && a.point_status[p] != GH_TRACK_OK) {
      state = GH_PDESC_NOT_OK;
    } else {
      first = a.start[p];
      L = a.start[p + 1] - first;
      state = L == 0 ? GH_PDESC_EMPTY : GH_PDESC_OK;
    }
  }
  const bool ok = state == GH_PDESC_OK;
  const int32_t* list = a.list + first;  // (not dereferenced unless ok)

  // direction: this lane's partial over its live indices, then the butterfly (all lanes of the wave take part)
  double s[3] = {0.0, 0.0, 0.0};
  double r2_ref = 0.0;  // lane 0 of the group: the reference is live index 0
  int node_ref = 0, obs_ref = -1;
  if (ok) {
    const double X[3] = {a.point_xyz[3 * (size_t)p], a.point_xyz[3 * (size_t)p + 1], a.point_xyz[3 * (size_t)p + 2]};
    for (int r = j; r < L; r += kGroupLanes) {
      const int obs = list[r];
      const int n = a.obs_node[obs];  // (a listed observation has passed the range tests)
      const double* t = a.cam_pose + (size_t)(n / a.cap) * 7 + 4;
      const double v0 = X[0] - t[0], v1 = X[1] - t[1], v2 = X[2] - t[2];
      const double r2 = (v0 * v0 + v1 * v1) + v2 * v2;
      const double inv = 1.0 / sqrt(r2);
      s[0] = s[0] + v0 * inv;
      s[1] = s[1] + v1 * inv;
      s[2] = s[2] + v2 * inv;
      if (r == 0) {
        r2_ref = r2;
        node_ref = n;
        obs_ref = obs;
      }
    }
  }
#pragma unroll
  for (int m = 4; m >= 1; m >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = s[k] + __shfl_xor(s[k], m);

  // descriptor, M <= 8: candidate c in lane c, every lane's row of distances in registers
  const int M = L < a.max_views ? L : a.max_views;
  const bool narrow = ok && M <= kGroupLanes;
  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int cand_obs = -1;
  if (narrow && j < M) {
    cand_obs = list[candidate_index(j, L, M)];
    const uint32_t* src = a.desc + (size_t)a.obs_node[cand_obs] * 8;
#pragma unroll
    for (int w = 0; w < 8; ++w) d[w] = src[w];
  }
  int row[kGroupLanes];
#pragma unroll
  for (int b = 0; b < kGroupLanes; ++b) {
    uint32_t o[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = __shfl(d[w], b, kGroupLanes);
    row[b] = hamming256(d, o);
  }
  const int mid = (M - 1) / 2;
  int med = 0;
#pragma unroll
  for (int i = 0; i < kGroupLanes; ++i) {
    int lt = 0, le = 0;
#pragma unroll
    for (int k = 0; k < kGroupLanes; ++k) {
      lt += (k < M && row[k] < row[i]) ? 1 : 0;
      le += (k < M && row[k] <= row[i]) ? 1 : 0;
    }
    if (i < M && lt <= mid && mid < le) med = row[i];  // (every i that passes holds the same value)
  }
  int best = (narrow && j < M) ? (med << 3) | j : INT_MAX;  // smallest median, lowest candidate on ties
#pragma unroll
  for (int m = 4; m >= 1; m >>= 1) {
    const int o = __shfl_xor(best, m);
    best = o < best ? o : best;
  }

  if (in_range && state != GH_PDESC_SKIPPED) {
    uint32_t* out = a.out_desc + (size_t)p * 8;
    if (!ok) {
      out[j] = 0;  // eight lanes, eight words
    } else if (narrow && j == (best & (kGroupLanes - 1))) {
#pragma unroll
      for (int w = 0; w < 8; ++w) out[w] = d[w];
      a.out_obs[2 * (size_t)p] = cand_obs;
    }
    if (j == 0) {
      double nrm[3] = {0.0, 0.0, 0.0}, lo = 0.0, hi = 0.0;
      if (ok) {
        const double len = (double)L;
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = s[k] / len;
        const int oct = a.kps[node_ref].octave;
        const int level = oct < 0 ? 0 : (oct > a.n_levels - 1 ? a.n_levels - 1 : oct);
        double scale = 1.0, top = 1.0;
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) {  // (selects, not an index: the table stays in scalar registers)
          if (l == level) scale = pw.v[l];
          if (l == a.n_levels - 1) top = pw.v[l];
        }
        hi = sqrt(r2_ref) * scale;
        lo = hi / top;
      } else {
        a.out_obs[2 * (size_t)p] = -1;
      }
      a.out_obs[2 * (size_t)p + 1] = obs_ref;
      a.views[p] = ok ? L : 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) a.normal[3 * (size_t)p + k] = canonical(nrm[k]);
      a.dist[2 * (size_t)p] = canonical(lo);
      a.dist[2 * (size_t)p + 1] = canonical(hi);
    }
  }
  if (in_range && j == 0) a.state[p] = (uint8_t)state;

  const bool head = in_range && j == 0;
  gh_map::block_counts_add<4>({gh_map::wave_count(head && ok), gh_map::wave_count(head && state == GH_PDESC_EMPTY),
                               gh_map::wave_count(head && state == GH_PDESC_NOT_OK), gh_map::wave_count(head && ok && L > a.max_views)},
                              a.totals);
}

__global__ __launch_bounds__(kBlock) void pdsc_wide_kernel(DescArgs a) {
  __shared__ uint16_t s_dist[kWavesPerBlock][kMaxViews * 64];  // [b][a]: lane a owns column a
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long gp = (long long)blockIdx.x * kWavesPerBlock + wave;
  if (gp >= a.n_points) return;  // (wave-uniform, as every exit below; the kernel has no barrier)
  const int p = (int)gp;
  if (a.point_select && a.point_select[p] == 0) return;
  if (a.point_status && a.point_status[p] != GH_TRACK_OK) return;
  const int first = a.start[p];
  const int L = a.start[p + 1] - first;
  const int M = L < a.max_views ? L : a.max_views;
  if (M <= kGroupLanes) return;  // pdsc_narrow has chosen
  const int32_t* list = a.list + first;

  uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int cand_obs = -1;
  if (lane < M) {
    cand_obs = list[candidate_index(lane, L, M)];
    const uint32_t* src = a.desc + (size_t)a.obs_node[cand_obs] * 8;
#pragma unroll
    for (int w = 0; w < 8; ++w) d[w] = src[w];
  }
  uint16_t* col = &s_dist[wave][lane];
  for (int b = 0; b < M; ++b) {
    uint32_t o[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = __shfl(d[w], b);
    col[b * 64] = (uint16_t)hamming256(d, o);
  }
  // the element at index (M - 1) / 2 of the sorted column: the smallest v with at least (M - 1) / 2 + 1 values <= v
  const int need = (M - 1) / 2 + 1;
  int v = 0;  // invariant: fewer than `need` values are <= v - 1
#pragma unroll 1
  for (int bit = 256; bit >= 1; bit >>= 1) {
    const int t = v + bit - 1;
    int cnt = 0;
    for (int b = 0; b < M; ++b) cnt += col[b * 64] <= t ? 1 : 0;
    if (cnt < need) v += bit;
  }
  int best = lane < M ? (v << 6) | lane : INT_MAX;  // smallest median, lowest candidate on ties
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(best, m);
    best = o < best ? o : best;
  }
  if (lane == (best & 63)) {
    uint32_t* out = a.out_desc + (size_t)p * 8;
#pragma unroll
    for (int w = 0; w < 8; ++w) out[w] = d[w];
    a.out_obs[2 * (size_t)p] = cand_obs;
  }
}

}  // namespace

extern "C" void gh_point_desc_default_params(gh_point_desc_params* p) {
  if (!p) return;
  p->scale_factor = 1.2;
  p->n_levels = 8;
  p->max_views = kMaxViews;
}

extern "C" gh_status gh_describe_points_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const uint8_t* desc_dev, const int32_t* counts_dev,
                                            int n_frames, int cap, const double* cam_pose_dev, const int32_t* obs_cam_dev,
                                            const int32_t* obs_point_dev, const int32_t* obs_node_dev, const uint8_t* obs_use_dev,
                                            int n_obs, int n_points, const double* point_xyz_dev, const int32_t* point_status_dev,
                                            const uint8_t* point_select_dev, const gh_point_desc_params* params,
                                            uint8_t* point_state_dev, uint8_t* point_desc_dev, int32_t* point_obs_dev,
                                            int32_t* point_views_dev, double* point_normal_dev, double* point_dist_dev,
                                            int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, params != nullptr);
  GH_CHECK_ARG(ctx, n_frames >= 0 && cap >= 0 && n_obs >= 0 && n_points >= 0 && cap <= 65535);
  GH_CHECK_ARG(ctx, (long long)n_points + (long long)n_frames * cap <= (long long)INT32_MAX - 1);
  GH_CHECK_ARG(ctx, std::isfinite(params->scale_factor) && params->scale_factor >= 1.0);
  GH_CHECK_ARG(ctx, params->n_levels >= 1 && params->n_levels <= kMaxLevels && params->max_views >= 1 && params->max_views <= kMaxViews);
  GH_CHECK_ARG(ctx, kps_dev && desc_dev && counts_dev && cam_pose_dev && obs_cam_dev && obs_point_dev && obs_node_dev && point_xyz_dev);
  GH_CHECK_ARG(ctx, point_state_dev && point_desc_dev && point_obs_dev && point_views_dev && point_normal_dev && point_dist_dev &&
                        totals_dev);
  GH_CHECK_ARG(ctx, gh_map::word_aligned(desc_dev, point_desc_dev));
  const int N = n_frames * cap;

  GH_HIP(ctx, hipMemsetAsync(totals_dev, 0, 4 * sizeof(int32_t), ctx->stream));
  if (n_points == 0) return GH_OK;

  // scratch: keys | the index's work space (start and list live there)
  const int spare = gh_map::spare_bins(n_points);
  const int n_keys = n_points + spare;
  size_t work_bytes = 0;
  GH_TRY(gh_map::index_bytes(ctx, "gh_describe_points_dev", n_obs, n_keys, &work_bytes));
  gh_carve c;
  const size_t o_keys = c.take((size_t)n_obs * 4), o_work = c.take(work_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* keys = (int32_t*)(base + o_keys);
  if (n_obs > 0)
    GH_LAUNCH(ctx, "pdsc_keys", pdsc_keys_kernel, dim3(gh_div_up(n_obs, kBlock)), dim3(kBlock), 0, counts_dev, cap, N, obs_cam_dev,
              obs_point_dev, obs_node_dev, obs_use_dev, n_obs, n_points, spare - 1, keys);
  const int32_t *start = nullptr, *list = nullptr;
  GH_TRY(gh_map::build_index(ctx, "pdsc_index", keys, n_obs, n_keys, base + o_work, work_bytes, &start, &list));

  DescArgs a = {};
  a.kps = kps_dev;
  a.desc = (const uint32_t*)desc_dev;
  a.cam_pose = cam_pose_dev;
  a.obs_node = obs_node_dev;
  a.point_xyz = point_xyz_dev;
  a.point_status = point_status_dev;
  a.point_select = point_select_dev;
  a.start = start;
  a.list = list;
  a.n_points = n_points;
  a.cap = cap;
  a.n_levels = params->n_levels;
  a.max_views = params->max_views;
  a.state = point_state_dev;
  a.out_desc = (uint32_t*)point_desc_dev;
  a.out_obs = point_obs_dev;
  a.views = point_views_dev;
  a.normal = point_normal_dev;
  a.dist = point_dist_dev;
  a.totals = totals_dev;
  GH_LAUNCH(ctx, "pdsc_narrow", pdsc_narrow_kernel, dim3(gh_div_up(n_points, kPointsPerBlock)), dim3(kBlock), 0, a,
            gh_map::scale_powers(params->scale_factor));
  if (params->max_views > kGroupLanes && n_obs > kGroupLanes)  // (else no track has more than eight candidates)
    GH_LAUNCH(ctx, "pdsc_wide", pdsc_wide_kernel, dim3(gh_div_up(n_points, kWavesPerBlock)), dim3(kBlock), 0, a);
  return GH_OK;
}
