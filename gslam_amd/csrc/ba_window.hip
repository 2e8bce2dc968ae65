// The local window of a bundle adjustment, selected and compacted on the device: gh_ba_window_dev and gh_ba_window_scatter_dev.
// The map's arrays go in as gh_extend_tracks_dev and gh_triangulate_tracks_dev leave them (padded, with obs_good and the point
// status as use bytes) together with a byte per camera that marks the new frames; out come the compact arrays of a
// gh_ba_problem, the index maps back to the map and eight totals.  The contract is in include/gslam_hip.h;
// tests/ba_window_restate.py restates it on dicts and sets and the device is held to it byte for byte.  Everything is integer
// work and copies of bits, so the result is the same bytes on every run and in every order of the observations (up to that
// order itself).
//
// WHY THE VERDICTS DO NOT DEPEND ON A RACE.  Every rule is a function of sets and of integer counts, and every pass reads only
// what an EARLIER launch finished.  usable[k] has one lane and one writer per byte.  n_use[p] and shared[c] are sums of ones:
// integer atomic adds on words the call zeroed -- commutative and exact -- after the lanes of a wave that sit next to each other
// with the same key have folded their ones into the first of them (gh_map::add_runs: a ballot and a bit scan, no second
// atomic), so observations in frame-major order cost one atomic per camera and wave in baw_shared, and in track-major order
// one per point and wave in baw_count.  seen[p], window[p] and has[c] get the byte 1 from every writer (the same value from all
// of them) on bytes the call zeroed.  LOCAL is one lane per camera.  Slots are an exclusive prefix sum over ids; an
// observation's slot is its rank among the window observations in ascending index.
//
// CDNA4 mapping (add_runs and the counter tail block_counts_add are gh_map's, map_dev.h; the scan is dev_prims.h's):
//   * baw_count    one lane per observation: the USABLE byte, n_use[point] += 1, the usable total (block_counts_add: ballot,
//                  LDS, one atomic per workgroup);
//   * baw_seen     per usable observation: LIVE (n_use >= min_point_obs) and in a seed camera -> seen[point] = 1;
//   * baw_shared   per usable observation: LIVE and its point SEEN -> shared[camera] += 1;
//   * baw_local    one lane per camera: LOCAL, cam_shared_dev, and the LOCAL / held / seed totals;
//   * baw_points   per usable observation: LIVE and in a LOCAL camera -> window[point] = 1;
//   * baw_fixed    per observation: usable and of a window point -> has[camera] = 1, and the observation's flag (the LOW word of
//                  flags[k]);
//   * baw_flags    entity i of the list [cameras | points] in the window -> the HIGH word of flags[i]; ONE exclusive scan of
//                  max(n_obs, n_cams + n_points) + 1 uint64 then numbers the observations (low word, < 2^31) and the cameras and
//                  points (high word, < 2^32: a camera's slot is the word at its id, a point's the word at n_cams + id less
//                  the word at n_cams) -- three scans in one rocPRIM call at every size the arguments can take;
//   * baw_emit     every entry of every remaining output: classes, slots, the compact arrays at their slots, the padding past
//                  the totals, the totals.
#include <algorithm>

#include "dev_prims.h"
#include "map_dev.h"

namespace {

using namespace gh_map;

struct BawArgs {
  int n_cams, n_points, n_obs;
  const double* cam_pose;
  const double* point_xyz;
  const int32_t* obs_cam;
  const int32_t* obs_point;
  const double* obs_xy;
  const uint8_t* cam_hold;   // n_cams or NULL
  const uint8_t* local;      // n_cams
  const uint8_t* has;        // n_cams: the camera holds a window observation
  const uint8_t* window;     // n_points
  const uint64_t* flags;     // the low word of [k]: observation k is a window observation
  const uint64_t* rank;      // max(n_obs, n_cams + n_points) + 1: exclusive scan of the flags; the last entry = the totals
  const int32_t* counters;   // usable observations, LOCAL cameras, held LOCAL cameras, seed cameras in the window
  uint8_t* cam_class;
  int32_t* cam_slot;
  int32_t* point_slot;
  int32_t* win_cam;
  int32_t* win_cam_dof;
  double* win_cam_pose;
  int32_t* win_point;
  double* win_point_xyz;
  int32_t* win_obs_cam;
  int32_t* win_obs_point;
  int32_t* win_obs_src;
  double* win_obs_xy;
  int32_t* totals;
};

__global__ __launch_bounds__(kBlock) void baw_count_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                           const uint8_t* __restrict__ obs_use, const uint8_t* __restrict__ point_use,
                                                           int n_cams, int n_points, int n_obs, uint8_t* __restrict__ usable,
                                                           int32_t* n_use, int32_t* counters) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool u = false;
  int p = 0;
  if (g < n_obs) {
    const int c = obs_cam[g];
    p = obs_point[g];
    u = (!obs_use || obs_use[g] != 0) && c >= 0 && c < n_cams && p >= 0 && p < n_points;
    if (u && point_use) u = point_use[p] != 0;
    usable[g] = u ? 1 : 0;
  }
  add_runs(n_use, p, u);
  block_counts_add<1>({wave_count(u)}, counters);
}

__global__ __launch_bounds__(kBlock) void baw_seen_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                          const uint8_t* __restrict__ usable, const int32_t* __restrict__ n_use,
                                                          const uint8_t* __restrict__ cam_seed, int n_obs, int min_point_obs,
                                                          uint8_t* seen) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_obs || usable[g] == 0) return;
  const int p = obs_point[g];
  if (n_use[p] >= min_point_obs && cam_seed[obs_cam[g]] != 0) seen[p] = 1;
}

__global__ __launch_bounds__(kBlock) void baw_shared_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                            const uint8_t* __restrict__ usable, const int32_t* __restrict__ n_use,
                                                            const uint8_t* __restrict__ seen, int n_obs, int min_point_obs,
                                                            int32_t* shared) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool on = false;
  int c = 0;
  if (g < n_obs && usable[g] != 0) {
    const int p = obs_point[g];
    c = obs_cam[g];
    on = n_use[p] >= min_point_obs && seen[p] != 0;
  }
  add_runs(shared, c, on);
}

__global__ __launch_bounds__(kBlock) void baw_local_kernel(const int32_t* __restrict__ shared, const uint8_t* __restrict__ cam_seed,
                                                           const uint8_t* __restrict__ cam_hold, int n_cams, int min_shared,
                                                           uint8_t* __restrict__ local, int32_t* __restrict__ cam_shared,
                                                           int32_t* counters) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  bool is_local = false, is_held = false, is_seed = false;
  if (g < n_cams) {
    const int s = shared[g];
    const bool seed = cam_seed[g] != 0;
    is_local = (seed && s >= 1) || s >= (min_shared > 1 ? min_shared : 1);
    is_held = is_local && cam_hold && cam_hold[g] != 0;
    is_seed = is_local && seed;  // (a seed camera that holds a window observation holds a live one, and is LOCAL)
    local[g] = is_local ? 1 : 0;
    cam_shared[g] = s;
  }
  block_counts_add<3>({wave_count(is_local), wave_count(is_held), wave_count(is_seed)}, counters + 1);
}

__global__ __launch_bounds__(kBlock) void baw_points_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                            const uint8_t* __restrict__ usable, const int32_t* __restrict__ n_use,
                                                            const uint8_t* __restrict__ local, int n_obs, int min_point_obs,
                                                            uint8_t* window) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_obs || usable[g] == 0) return;
  const int p = obs_point[g];
  if (n_use[p] >= min_point_obs && local[obs_cam[g]] != 0) window[p] = 1;
}

// (a window point is LIVE, so its usable observations are the live ones)
__global__ __launch_bounds__(kBlock) void baw_fixed_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                           const uint8_t* __restrict__ usable, const uint8_t* __restrict__ window,
                                                           int n_obs, uint8_t* has, uint32_t* __restrict__ flag_words) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n_obs) return;
  const bool in = usable[g] != 0 && window[obs_point[g]] != 0;
  if (in) has[obs_cam[g]] = 1;
  flag_words[2 * (size_t)g] = in ? 1u : 0u;
}

// entries 0 .. last of the flags: the high word of every one, and the low word past the observations
__global__ __launch_bounds__(kBlock) void baw_flags_kernel(const uint8_t* __restrict__ local, const uint8_t* __restrict__ has,
                                                           const uint8_t* __restrict__ window, int n_cams, int n_points, int n_obs,
                                                           long long last, uint32_t* __restrict__ flag_words) {
  const long long step = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i <= last; i += step) {
    uint32_t f = 0;
    if (i < n_cams) f = (local[i] | has[i]) != 0 ? 1u : 0u;
    else if (i - n_cams < n_points) f = window[i - n_cams] != 0 ? 1u : 0u;
    flag_words[2 * (size_t)i + 1] = f;
    if (i >= n_obs) flag_words[2 * (size_t)i] = 0u;
  }
}

__device__ __forceinline__ void baw_copy_bits(double* __restrict__ dst, const double* __restrict__ src, int n) {
  for (int j = 0; j < n; ++j) ((unsigned long long*)dst)[j] = ((const unsigned long long*)src)[j];
}

__global__ __launch_bounds__(kBlock) void baw_emit_kernel(BawArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;  // 0 .. max(n_cams, n_points, n_obs, 1) - 1
  const long long cp = (long long)a.n_cams + a.n_points;
  const uint64_t total = a.rank[cp > a.n_obs ? cp : (long long)a.n_obs];
  const uint32_t cam_base = (uint32_t)(a.rank[a.n_cams] >> 32);  // = the number of window cameras
  const int n_win_cams = (int)cam_base, n_win_points = (int)((uint32_t)(total >> 32) - cam_base), n_win_obs = (int)(uint32_t)total;
  if (g == 0) {
    a.totals[0] = n_win_cams;
    a.totals[1] = a.counters[1];
    a.totals[2] = n_win_cams - a.counters[1];
    a.totals[3] = a.counters[2];
    a.totals[4] = n_win_points;
    a.totals[5] = n_win_obs;
    a.totals[6] = a.counters[3];
    a.totals[7] = a.counters[0];
  }
  if (g < a.n_cams) {
    const int c = (int)g;
    const bool is_local = a.local[c] != 0, in = is_local || a.has[c] != 0;
    const int slot = in ? (int)(a.rank[c] >> 32) : -1;
    a.cam_class[c] = is_local ? GH_WIN_LOCAL : (in ? GH_WIN_FIXED : GH_WIN_NONE);
    a.cam_slot[c] = slot;
    if (c >= n_win_cams) {  // the padding; the entries below are written by the cameras that own them
      a.win_cam[c] = -1;
      a.win_cam_dof[c] = 0;
      for (int j = 0; j < 7; ++j) a.win_cam_pose[7 * (size_t)c + j] = 0.0;
    }
    if (in) {
      a.win_cam[slot] = c;
      a.win_cam_dof[slot] = is_local && !(a.cam_hold && a.cam_hold[c] != 0) ? GH_KF_SE3 : 0;
      baw_copy_bits(a.win_cam_pose + 7 * (size_t)slot, a.cam_pose + 7 * (size_t)c, 7);
    }
  }
  if (g < a.n_points) {
    const int p = (int)g;
    const bool in = a.window[p] != 0;
    const int slot = in ? (int)((uint32_t)(a.rank[(size_t)a.n_cams + p] >> 32) - cam_base) : -1;
    a.point_slot[p] = slot;
    if (p >= n_win_points) {
      a.win_point[p] = -1;
      for (int j = 0; j < 3; ++j) a.win_point_xyz[3 * (size_t)p + j] = 0.0;
    }
    if (in) {
      a.win_point[slot] = p;
      baw_copy_bits(a.win_point_xyz + 3 * (size_t)slot, a.point_xyz + 3 * (size_t)p, 3);
    }
  }
  if (g < a.n_obs) {
    const int k = (int)g;
    if (k >= n_win_obs) {
      a.win_obs_cam[k] = -1;
      a.win_obs_point[k] = -1;
      a.win_obs_src[k] = -1;
      a.win_obs_xy[2 * (size_t)k] = 0.0;
      a.win_obs_xy[2 * (size_t)k + 1] = 0.0;
    }
    if ((uint32_t)a.flags[k] != 0) {
      const int slot = (int)(uint32_t)a.rank[k];
      a.win_obs_cam[slot] = (int)(a.rank[a.obs_cam[k]] >> 32);
      a.win_obs_point[slot] = (int)((uint32_t)(a.rank[(size_t)a.n_cams + a.obs_point[k]] >> 32) - cam_base);
      a.win_obs_src[slot] = k;
      baw_copy_bits(a.win_obs_xy + 2 * (size_t)slot, a.obs_xy + 2 * (size_t)k, 2);
    }
  }
}

__global__ __launch_bounds__(kBlock) void baw_scatter_kernel(const int32_t* __restrict__ win_cam, const int32_t* __restrict__ win_cam_dof,
                                                             int n_win_cams, const double* __restrict__ cam_pose_win,
                                                             const int32_t* __restrict__ win_point, int n_win_points,
                                                             const double* __restrict__ point_xyz_win, double* __restrict__ cam_pose,
                                                             int n_cams, double* __restrict__ point_xyz, int n_points) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g < n_win_cams && win_cam_dof[g] != 0) {
    const int c = win_cam[g];
    if (c >= 0 && c < n_cams) baw_copy_bits(cam_pose + 7 * (size_t)c, cam_pose_win + 7 * (size_t)g, 7);
  }
  if (g < n_win_points) {
    const int p = win_point[g];
    if (p >= 0 && p < n_points) baw_copy_bits(point_xyz + 3 * (size_t)p, point_xyz_win + 3 * (size_t)g, 3);
  }
}

}  // namespace

extern "C" void gh_ba_window_default_params(gh_ba_window_params* p) {
  if (!p) return;
  p->min_shared = 15;     // ORB-SLAM's co-visibility threshold
  p->min_point_obs = 2;   // a point needs two rays
}

extern "C" gh_status gh_ba_window_dev(gh_ctx* ctx, int n_cams, int n_points, int n_obs, const double* cam_pose_dev,
                                      const double* point_xyz_dev, const int32_t* obs_cam_dev, const int32_t* obs_point_dev,
                                      const double* obs_xy_dev, const uint8_t* obs_use_dev, const uint8_t* point_use_dev,
                                      const uint8_t* cam_seed_dev, const uint8_t* cam_hold_dev, const gh_ba_window_params* params,
                                      uint8_t* cam_class_dev, int32_t* cam_shared_dev, int32_t* cam_slot_dev, int32_t* point_slot_dev,
                                      int32_t* win_cam_dev, int32_t* win_cam_dof_dev, double* win_cam_pose_dev, int32_t* win_point_dev,
                                      double* win_point_xyz_dev, int32_t* win_obs_cam_dev, int32_t* win_obs_point_dev,
                                      int32_t* win_obs_src_dev, double* win_obs_xy_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, params != nullptr);
  GH_CHECK_ARG(ctx, n_cams >= 0 && n_points >= 0 && n_obs >= 0);
  GH_CHECK_ARG(ctx, params->min_shared >= 0 && params->min_point_obs >= 1);
  GH_CHECK_ARG(ctx, cam_seed_dev != nullptr);
  GH_CHECK_ARG(ctx, cam_class_dev && cam_shared_dev && cam_slot_dev && point_slot_dev && win_cam_dev && win_cam_dof_dev &&
                        win_cam_pose_dev && win_point_dev && win_point_xyz_dev && win_obs_cam_dev && win_obs_point_dev &&
                        win_obs_src_dev && win_obs_xy_dev && totals_dev);
  GH_CHECK_ARG(ctx, n_cams == 0 || cam_pose_dev);
  GH_CHECK_ARG(ctx, n_points == 0 || point_xyz_dev);
  GH_CHECK_ARG(ctx, n_obs == 0 || (obs_cam_dev && obs_point_dev && obs_xy_dev));

  const size_t nc = (size_t)n_cams, np = (size_t)n_points, no = (size_t)n_obs;
  const size_t last = std::max(no, nc + np);  // the scan covers the entries 0 .. last
  // The scratch block.  n_use, shared, seen, window, has and the four counters are neighbours: one memset clears them.
  const size_t tmp_bytes = gh_scan_u64_bytes(ctx, last + 1);
  if (!tmp_bytes) return gh_set_error(ctx, GH_ERR_HIP, "gh_ba_window_dev: rocPRIM size query failed");
  gh_carve c;
  const size_t o_n_use = c.take(np * 4), o_shared = c.take(nc * 4), o_seen = c.take(np), o_window = c.take(np), o_has = c.take(nc);
  const size_t o_counters = c.take(4 * sizeof(int32_t)), o_usable = c.take(no), o_local = c.take(nc);
  const size_t o_flags = c.take((last + 1) * 8), o_rank = c.take((last + 1) * 8), o_tmp = c.take(tmp_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* n_use = (int32_t*)(base + o_n_use);
  int32_t* shared = (int32_t*)(base + o_shared);
  uint8_t* seen = (uint8_t*)(base + o_seen);
  uint8_t* window = (uint8_t*)(base + o_window);
  uint8_t* has = (uint8_t*)(base + o_has);
  int32_t* counters = (int32_t*)(base + o_counters);
  uint8_t* usable = (uint8_t*)(base + o_usable);
  uint8_t* local = (uint8_t*)(base + o_local);
  uint64_t* flags = (uint64_t*)(base + o_flags);
  uint64_t* rank = (uint64_t*)(base + o_rank);

  const dim3 block(kBlock), obs_grid(gh_div_up(n_obs, kBlock)), cam_grid(gh_div_up(n_cams, kBlock));
  const int mpo = params->min_point_obs;
  GH_HIP(ctx, hipMemsetAsync(n_use, 0, o_usable - o_n_use, ctx->stream));
  if (n_obs > 0) {
    GH_LAUNCH(ctx, "baw_count", baw_count_kernel, obs_grid, block, 0, obs_cam_dev, obs_point_dev, obs_use_dev, point_use_dev, n_cams,
              n_points, n_obs, usable, n_use, counters);
    GH_LAUNCH(ctx, "baw_seen", baw_seen_kernel, obs_grid, block, 0, obs_cam_dev, obs_point_dev, (const uint8_t*)usable,
              (const int32_t*)n_use, cam_seed_dev, n_obs, mpo, seen);
    GH_LAUNCH(ctx, "baw_shared", baw_shared_kernel, obs_grid, block, 0, obs_cam_dev, obs_point_dev, (const uint8_t*)usable,
              (const int32_t*)n_use, (const uint8_t*)seen, n_obs, mpo, shared);
  }
  if (n_cams > 0)
    GH_LAUNCH(ctx, "baw_local", baw_local_kernel, cam_grid, block, 0, (const int32_t*)shared, cam_seed_dev, cam_hold_dev, n_cams,
              params->min_shared, local, cam_shared_dev, counters);
  if (n_obs > 0) {
    GH_LAUNCH(ctx, "baw_points", baw_points_kernel, obs_grid, block, 0, obs_cam_dev, obs_point_dev, (const uint8_t*)usable,
              (const int32_t*)n_use, (const uint8_t*)local, n_obs, mpo, window);
    GH_LAUNCH(ctx, "baw_fixed", baw_fixed_kernel, obs_grid, block, 0, obs_cam_dev, obs_point_dev, (const uint8_t*)usable,
              (const uint8_t*)window, n_obs, has, (uint32_t*)flags);
  }
  const int flag_blocks = gh_div_up((long long)last + 1, kBlock);
  GH_LAUNCH(ctx, "baw_flags", baw_flags_kernel, dim3(flag_blocks < kMaxFlagBlocks ? flag_blocks : kMaxFlagBlocks), block, 0,
            (const uint8_t*)local, (const uint8_t*)has, (const uint8_t*)window, n_cams, n_points, n_obs, (long long)last,
            (uint32_t*)flags);
  GH_TRY(gh_scan_u64(ctx, "baw_scan", "gh_ba_window_dev: scan", base + o_tmp, tmp_bytes, flags, rank, last + 1));

  const BawArgs a = {n_cams, n_points, n_obs, cam_pose_dev, point_xyz_dev, obs_cam_dev, obs_point_dev, obs_xy_dev, cam_hold_dev,  // inputs
                     local, has, window, flags, rank, counters,                                                                   // scratch
                     cam_class_dev, cam_slot_dev, point_slot_dev,                                                                 // per id
                     win_cam_dev, win_cam_dof_dev, win_cam_pose_dev, win_point_dev, win_point_xyz_dev,                            // compact
                     win_obs_cam_dev, win_obs_point_dev, win_obs_src_dev, win_obs_xy_dev, totals_dev};
  const int most = std::max(std::max(n_cams, n_points), std::max(n_obs, 1));
  GH_LAUNCH(ctx, "baw_emit", baw_emit_kernel, dim3(gh_div_up(most, kBlock)), block, 0, a);
  return GH_OK;
}

extern "C" gh_status gh_ba_window_scatter_dev(gh_ctx* ctx, const int32_t* win_cam_dev, const int32_t* win_cam_dof_dev, int n_win_cams,
                                              const double* cam_pose_win_dev, const int32_t* win_point_dev, int n_win_points,
                                              const double* point_xyz_win_dev, double* cam_pose_dev, int n_cams, double* point_xyz_dev,
                                              int n_points) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n_win_cams >= 0 && n_win_points >= 0 && n_cams >= 0 && n_points >= 0);
  GH_CHECK_ARG(ctx, n_win_cams == 0 || (win_cam_dev && win_cam_dof_dev && cam_pose_win_dev));
  GH_CHECK_ARG(ctx, n_win_points == 0 || (win_point_dev && point_xyz_win_dev));
  GH_CHECK_ARG(ctx, n_win_cams == 0 || n_cams == 0 || cam_pose_dev);
  GH_CHECK_ARG(ctx, n_win_points == 0 || n_points == 0 || point_xyz_dev);
  const int most = std::max(n_win_cams, n_win_points);
  if (most == 0) return GH_OK;
  GH_LAUNCH(ctx, "baw_scatter", baw_scatter_kernel, dim3(gh_div_up(most, kBlock)), dim3(kBlock), 0, win_cam_dev, win_cam_dof_dev,
            n_win_cams, cam_pose_win_dev, win_point_dev, n_win_points, point_xyz_win_dev, cam_pose_dev, n_cams, point_xyz_dev, n_points);
  return GH_OK;
}
