// Map points from multi-view tracks, batched and device-resident: gh_triangulate_tracks_dev.  The arrays of a gh_ba_problem go
// in as they lie on the device; every point gets a start (the least-squares intersection of its rays), a status and a verdict
// per observation, with up to max_drops gross outliers rejected.  The contract is in include/gslam_hip.h; tests/tracks_restate.py
// restates it in scalar doubles and the device is held to it bit for bit.
//
// Measured at C5 size (1 M points, 6 M observations): 728 us a call, 420 of them the index build, 274 the
// triangulation kernel, at a tenth of its byte floor: by the instruction count its bound is f64 VALU issue (a square root and
// two divisions per observation and round, six divisions of the redundant 3 x 3 solve per lane).  CDNA4 mapping:
//   * index    tracks_keys maps every observation to its point, or to the extra bin n_points when it is masked or an index is
//              out of range (such an index is never dereferenced), and writes the first obs_good: 1 = usable.  gh_csr_index_dev
//              (csr_sort.hip: rocPRIM radix sort + scan, context scratch) turns the keys into start / list: the track of a point
//              in ascending observation index, whatever order the caller's arrays have;
//   * triangulate  one group of 8 lanes per point, 8 points per wave, 32 per 256-thread workgroup.  Lane j owns the ranks
//              j, j + 8, ... of its track and keeps the 9 entries of its partial sum (6 of P, 3 of g) in registers; the eight
//              partials meet in a __shfl_xor butterfly over 4, 2, 1, which is the stated order ((s0+s4)+(s2+s6))+((s1+s5)+(s3+s7))
//              in every lane (IEEE addition commutes), so every lane of a group holds the same bits and solves, tests and
//              decides redundantly: control flow is uniform per group, nothing is broadcast, no LDS;
//   * the live set is obs_good itself: a byte per observation, read and written only by the lane that owns the rank, so no
//              fence is needed and a track may be any length.  The rank-j observation (all of a track of up to 8) also stays in
//              registers: pose, xy and ray are gathered once, not once per pass;
//   * the worst observation of a round is a three-step (key, rank) butterfly, the parallax anchor a three-step minimum of the
//              lanes' first live ranks and one shuffle of its ray from the owner;
//   * the round loop runs while any group of the wave is unfinished, so every shuffle is executed by all 64 lanes.
// A 64-lane variant for long tracks could not reproduce the summation order; a long track stalls its wave (tools/tracks_probe.py
// reports the skew: one track of 60 000 observations holds the kernel for 12 ms).  A gather of (cam, xy) into track order was
// not added: with the rank-j observation in registers a track of up to 8 reads each of its rows by index exactly once, which is
// what the gather itself would have to do before anything else, and the kernel is not bound by bytes.
#include <climits>

#include "ba_obs.h"
#include "map_host.h"

namespace {

using gh_map::kBlock;

constexpr int kGroupLanes = 8;
constexpr int kPointsPerBlock = kBlock / kGroupLanes;
constexpr double kMinPivot = 1e-12;
constexpr int kRunning = -1, kConverged = -2;  // inside the kernel only: rounds go on / all live observations good, parallax pending

struct TrackArgs {
  const double* cam_pose;
  const int32_t* obs_cam;
  const double* obs_xy;
  const uint8_t* point_select;  // may be NULL
  const int32_t* start;         // n_points + 2 (the last bin holds what is not usable)
  const int32_t* list;
  int n_points;
  int min_views, max_drops;
  double min_parallax_cos, reproj2;
  double* point_xyz;
  int32_t* status;
  int32_t* n_good;
  uint8_t* obs_good;
};

struct Ray {
  double pose[7];  // T_wc of the observing camera
  double xy[2];
  double d[3];     // unit ray in the world
};

__global__ __launch_bounds__(kBlock) void tracks_keys_kernel(const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_point,
                                                             const uint8_t* __restrict__ obs_use, int n_obs, int n_cams, int n_points,
                                                             int32_t* __restrict__ key, uint8_t* __restrict__ obs_good) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_obs) return;
  const int c = obs_cam[i], p = obs_point[i];
  const bool usable = (!obs_use || obs_use[i] != 0) && c >= 0 && c < n_cams && p >= 0 && p < n_points;
  key[i] = usable ? p : n_points;
  obs_good[i] = usable ? 1 : 0;
}

__device__ __forceinline__ void load_ray(const TrackArgs& a, int obs, Ray& o) {
  const double* pose = a.cam_pose + (size_t)a.obs_cam[obs] * 7;  // (a listed observation has passed the range test)
#pragma unroll
  for (int k = 0; k < 7; ++k) o.pose[k] = pose[k];
  o.xy[0] = a.obs_xy[2 * (size_t)obs];
  o.xy[1] = a.obs_xy[2 * (size_t)obs + 1];
  const double v[3] = {o.xy[0], o.xy[1], 1.0};
  double w[3];
  gh_ba::quat_rotate(o.pose, v, w);
  const double s = 1.0 / sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.d[k] = w[k] * s;
}

// s: A00 A01 A02 A11 A12 A22 b0 b1 b2 -> X by LDL^T without pivoting; false: a pivot fails D > 1e-12 (a NaN included)
__device__ __forceinline__ bool solve3(const double* s, double* X) {
  const double D0 = s[0];
  const double L10 = s[1] / D0, L20 = s[2] / D0;
  const double D1 = s[3] - L10 * s[1];
  const double u = s[4] - L20 * s[1];
  const double L21 = u / D1;
  const double D2 = (s[5] - L20 * s[2]) - L21 * u;
  if (!(D0 > kMinPivot) || !(D1 > kMinPivot) || !(D2 > kMinPivot)) return false;
  const double z0 = s[6];
  const double z1 = s[7] - L10 * z0;
  const double z2 = (s[8] - L20 * z0) - L21 * z1;
  const double y0 = z0 / D0, y1 = z1 / D1, y2 = z2 / D2;
  X[2] = y2;
  X[1] = y1 - L21 * X[2];
  X[0] = (y0 - L10 * X[1]) - L20 * X[2];
  return true;
}

__global__ __launch_bounds__(kBlock) void tracks_triangulate_kernel(TrackArgs a) {
  const int tid = threadIdx.x, j = tid & (kGroupLanes - 1);
  const int gshift = tid & 56;  // first lane of the group inside its wave
  const long long gp = (long long)blockIdx.x * kPointsPerBlock + (tid >> 3);
  const bool in_range = gp < a.n_points;
  const int p = in_range ? (int)gp : 0;
  int first = 0, len = 0;
  if (in_range) {
    first = a.start[p];
    len = a.start[p + 1] - first;
  }
  const int32_t* list = a.list + first;  // (not dereferenced when len = 0)
  const int need = a.min_views;

  int status = kRunning, nlive = len, drops = 0;
  if (!in_range || (a.point_select && a.point_select[p] == 0)) status = GH_TRACK_SKIPPED;
  else if (nlive < need) status = GH_TRACK_TOO_FEW;
  bool done = status != kRunning;

  // the observation of rank j stays in registers; the later ranks of a long track are gathered again in every pass
  Ray r0 = {};
  bool live0 = false;
  if (!done && j < len) {
    load_ray(a, list[j], r0);
    live0 = true;
  }
  // this lane's live observations, ascending rank
  auto for_live = [&](auto fn) {
    if (live0) fn(j, r0);
    for (int r = j + kGroupLanes; r < len; r += kGroupLanes) {
      const int obs = list[r];
      if (a.obs_good[obs] == 0) continue;
      Ray o;
      load_ray(a, obs, o);
      fn(r, o);
    }
  };

  double X[3] = {0.0, 0.0, 0.0};
  while (__any(!done)) {
    // sum: this lane's partial over its live ranks, then the butterfly (all lanes of the wave take part)
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!done)
      for_live([&](int, const Ray& o) {
        const double* d = o.d;
        const double* t = o.pose + 4;
        const double P00 = 1.0 - d[0] * d[0], P11 = 1.0 - d[1] * d[1], P22 = 1.0 - d[2] * d[2];
        const double P01 = -(d[0] * d[1]), P02 = -(d[0] * d[2]), P12 = -(d[1] * d[2]);
        s[0] = s[0] + P00;
        s[1] = s[1] + P01;
        s[2] = s[2] + P02;
        s[3] = s[3] + P11;
        s[4] = s[4] + P12;
        s[5] = s[5] + P22;
        s[6] = s[6] + ((P00 * t[0] + P01 * t[1]) + P02 * t[2]);
        s[7] = s[7] + ((P01 * t[0] + P11 * t[1]) + P12 * t[2]);
        s[8] = s[8] + ((P02 * t[0] + P12 * t[1]) + P22 * t[2]);
      });
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1)
#pragma unroll
      for (int k = 0; k < 9; ++k) s[k] = s[k] + __shfl_xor(s[k], m);
    double Xr[3] = {0.0, 0.0, 0.0};
    const bool solved = solve3(s, Xr);

    // classify at Xr: all good?  else the worst live observation (largest key, lowest rank on ties)
    bool bad = false;
    double key = -1.0;  // (below every key: a lane without a live observation never wins)
    int krank = INT_MAX;
    if (!done && solved)
      for_live([&](int r, const Ray& o) {
        gh_ba::Obs lin;
        double k = __builtin_inf();
        bool good = false;
        if (gh_ba::linearize<false>(o.pose, 0, Xr, 0, o.xy, nullptr, 0.0, lin)) {
          const double e = lin.r[0] * lin.r[0] + lin.r[1] * lin.r[1];
          good = e <= a.reproj2;
          if (e == e) k = e;
        }
        if (!good) bad = true;
        if (k > key) {
          key = k;
          krank = r;
        }
      });
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) {
      const double ok = __shfl_xor(key, m);
      const int orank = __shfl_xor(krank, m);
      if (ok > key || (ok == key && orank < krank)) {
        key = ok;
        krank = orank;
      }
    }
    const unsigned any_bad = (unsigned)(__ballot(bad) >> gshift) & 0xffu;
    if (!done) {
      if (!solved) {
        status = GH_TRACK_DEGENERATE;
        done = true;
      } else if (!any_bad) {
        X[0] = Xr[0];
        X[1] = Xr[1];
        X[2] = Xr[2];
        status = kConverged;
        done = true;
      } else if (drops == a.max_drops || nlive == need) {
        status = GH_TRACK_INCONSISTENT;
        done = true;
      } else {
        if (krank < len && (krank & (kGroupLanes - 1)) == j) {  // the owner of the rank takes it out of the live set
          if (krank == j) live0 = false;
          a.obs_good[list[krank]] = 0;
        }
        --nlive;
        ++drops;
      }
    }
  }

  // parallax against the live observation of lowest rank
  int frank = INT_MAX;
  double fd[3] = {0.0, 0.0, 0.0};
  if (status == kConverged) {
    if (live0) {
      frank = j;
      fd[0] = r0.d[0];
      fd[1] = r0.d[1];
      fd[2] = r0.d[2];
    } else {
      for (int r = j + kGroupLanes; r < len; r += kGroupLanes) {
        const int obs = list[r];
        if (a.obs_good[obs] == 0) continue;
        Ray o;
        load_ray(a, obs, o);
        frank = r;
        fd[0] = o.d[0];
        fd[1] = o.d[1];
        fd[2] = o.d[2];
        break;
      }
    }
  }
  int fmin = frank;
#pragma unroll
  for (int m = 4; m >= 1; m >>= 1) {
    const int o = __shfl_xor(fmin, m);
    fmin = o < fmin ? o : fmin;
  }
  const int owner = fmin & (kGroupLanes - 1);
  const double df0 = __shfl(fd[0], owner, kGroupLanes), df1 = __shfl(fd[1], owner, kGroupLanes), df2 = __shfl(fd[2], owner, kGroupLanes);
  bool wide = false;
  if (status == kConverged)
    for_live([&](int r, const Ray& o) {
      if (r == fmin) return;
      const double c = (df0 * o.d[0] + df1 * o.d[1]) + df2 * o.d[2];
      if (c < a.min_parallax_cos) wide = true;
    });
  const unsigned any_wide = (unsigned)(__ballot(wide) >> gshift) & 0xffu;
  if (status == kConverged) status = any_wide ? GH_TRACK_OK : GH_TRACK_LOW_PARALLAX;

  if (!in_range) return;
  if (status != GH_TRACK_OK)  // the dropped observations of an OK point are cleared already, its live ones hold 1
    for (int r = j; r < len; r += kGroupLanes) a.obs_good[list[r]] = 0;
  if (j == 0) {
    a.status[p] = status;
    a.n_good[p] = status == GH_TRACK_OK ? nlive : 0;
    if (status != GH_TRACK_SKIPPED) {
      const bool ok = status == GH_TRACK_OK;
      a.point_xyz[3 * (size_t)p] = ok ? X[0] : 0.0;
      a.point_xyz[3 * (size_t)p + 1] = ok ? X[1] : 0.0;
      a.point_xyz[3 * (size_t)p + 2] = ok ? X[2] : 0.0;
    }
  }
}

}  // namespace

extern "C" void gh_track_default_params(gh_track_params* p) {
  if (!p) return;
  p->min_parallax_cos = 0.9998;
  p->max_reproj = 0.004;
  p->min_views = 2;
  p->max_drops = 2;
}

extern "C" int gh_track_group_lanes(void) { return kGroupLanes; }

extern "C" gh_status gh_triangulate_tracks_dev(gh_ctx* ctx, const double* cam_pose_dev, int n_cams, const int32_t* obs_cam_dev,
                                               const int32_t* obs_point_dev, const double* obs_xy_dev, int n_obs, int n_points,
                                               const uint8_t* obs_use_dev, const uint8_t* point_select_dev,
                                               const gh_track_params* params, double* point_xyz_dev, int32_t* status_dev,
                                               int32_t* n_good_dev, uint8_t* obs_good_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, params != nullptr);
  GH_CHECK_ARG(ctx, n_cams >= 0 && n_obs >= 0 && n_points >= 0 && n_points <= INT_MAX - 2);
  GH_CHECK_ARG(ctx, params->min_parallax_cos > 0.0 && params->min_parallax_cos <= 1.0 && params->max_reproj >= 0.0);  // (a NaN fails)
  GH_CHECK_ARG(ctx, params->min_views >= 2 && params->max_drops >= 0);
  if (n_points == 0) return GH_OK;
  GH_CHECK_ARG(ctx, cam_pose_dev && obs_cam_dev && obs_point_dev && obs_xy_dev);
  GH_CHECK_ARG(ctx, point_xyz_dev && status_dev && n_good_dev && obs_good_dev);

  // scratch: keys | the index's work space (start and list live there).  One spare bin, not gh_map::spare_bins: DESIGN.md 6
  const int n_keys = n_points + 1;
  size_t work_bytes = 0;
  GH_TRY(gh_map::index_bytes(ctx, "gh_triangulate_tracks_dev", n_obs, n_keys, &work_bytes));
  gh_carve c;
  const size_t o_keys = c.take((size_t)n_obs * 4), o_work = c.take(work_bytes);
  char* base = nullptr;
  GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
  int32_t* keys = (int32_t*)(base + o_keys);
  if (n_obs > 0)
    GH_LAUNCH(ctx, "tracks_keys", tracks_keys_kernel, dim3(gh_div_up(n_obs, kBlock)), dim3(kBlock), 0, obs_cam_dev, obs_point_dev,
              obs_use_dev, n_obs, n_cams, n_points, keys, obs_good_dev);
  const int32_t *start = nullptr, *list = nullptr;
  GH_TRY(gh_map::build_index(ctx, "tracks_index", keys, n_obs, n_keys, base + o_work, work_bytes, &start, &list));

  TrackArgs a = {};
  a.cam_pose = cam_pose_dev;
  a.obs_cam = obs_cam_dev;
  a.obs_xy = obs_xy_dev;
  a.point_select = point_select_dev;
  a.start = start;
  a.list = list;
  a.n_points = n_points;
  a.min_views = params->min_views;
  a.max_drops = params->max_drops;
  a.min_parallax_cos = params->min_parallax_cos;
  a.reproj2 = params->max_reproj * params->max_reproj;
  a.point_xyz = point_xyz_dev;
  a.status = status_dev;
  a.n_good = n_good_dev;
  a.obs_good = obs_good_dev;
  GH_LAUNCH(ctx, "tracks_triangulate", tracks_triangulate_kernel, dim3(gh_div_up(n_points, kPointsPerBlock)), dim3(kBlock), 0, a);
  return GH_OK;
}
