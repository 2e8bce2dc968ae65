// Search by projection, device-resident: gh_search_projection_dev.  The consumer of gh_describe_points_dev's summaries: the points
// of the map are projected into the frames whose pose is known, gated by distance range and viewing angle, compared with the
// OPEN keypoints in a window around the projection, and the winners leave as claims in the two arrays gh_extend_tracks_dev takes
// from gh_localize_pairs_dev.  The contract is in include/gslam_hip.h; tests/search_projection_restate.py restates it in plain
// Python and the device is held to it byte for byte.
//
// WHY THE BYTES DO NOT DEPEND ON A RACE.  Every gate is IEEE double arithmetic in a written order (the library is built with
// -ffp-contract=off).  The best and second candidate of a window are minima of the unique key (h, row): whatever order the lanes
// meet the candidates in, the two smallest keys are the same.  A node keeps the proposal with the smallest (h, p) through one
// 64-bit integer atomicMin.  The HELD set is an open-addressed table whose CONTENT as a set does not depend on insertion order,
// and only membership is asked.  The counters are integer atomic adds on words the call zeroed.  No float atomic anywhere.
//
// CDNA4 mapping (the shared pieces are gh_map's, map_dev.h, gh_ba::quat_rotate, ba_obs.h, and gh_csr_index_dev's, csr_sort.hip):
//   * sproj_frames   one workgroup: the searched frames, compacted in ascending order with ballots; their number stays on the
//                    device (totals[10]);
//   * sproj_grid     one lane per node of a searched frame: a TAKEN node puts its point into its frame's table of 2 * cap
//                    words (atomicCAS, linear probing, at most half full), an OPEN node gets the key frame * stride + cell of a
//                    grid of gh_search_cell_pixels() pixels; every other node goes to one of the spare bins (map_dev.h,
//                    THE SPARE BINS).  The cell of a coordinate is a CLAMP into the grid,
//                    monotone in the coordinate, NaN and negatives to cell 0: no coordinate becomes an index unclamped, and a
//                    window's clamped cell range holds every keypoint that can pass the strict comparisons, out of image or not;
//   * index          gh_csr_index_dev: per cell the OPEN nodes in ascending node order; the cells of one grid row are neighbours;
//   * sproj_search   a lane holds one point (xyz, normal, range: read once) and loops over the searched frames, whose pose and
//                    table base are wave-uniform.  Gates 0 - 4 run per lane; a ballot hands the survivors, eight at a time, to
//                    the wave's eight groups of 8 lanes: the point's descriptor sits in 8 VGPRs per lane, the lanes stride over
//                    the candidates of each grid row's contiguous list range, keep their own (best, second) keys
//                    (h << 16 | row) and merge them with width-8 shuffles.  Lane 0 of the group judges and proposes with one
//                    64-bit atomicMin.  The nine verdict counts of a (wave, frame) leave as ONE atomic instruction, lane k
//                    carrying counter k, none for a zero;
//   * sproj_resolve  a lane per node: the three node outputs (a lane reads its own claim before it writes it: in place is
//                    safe) and WON per frame through gh_map::add_runs;
//   * sproj_finish   a lane per frame: LOST = PROPOSED - WON, and the ten column sums through gh_map::block_counts_add.
#include <climits>
#include <cmath>

#include "ba_obs.h"
#include "map_host.h"

namespace {

using gh_map::kBlock;
using gh_map::kMaxLevels;

constexpr int kCellPixels = 32;
constexpr int kMaxGridSide = 64;   // at most 64 x 64 cells per frame, and never more cells than the frame has rows
constexpr int kGroupLanes = 8;
constexpr int kVerdicts = 10;      // HELD BEHIND OUTSIDE RANGE ANGLE NO_CANDIDATE WEAK RATIO LOST WON
constexpr int kProposed = 8;       // the LOST column counts the proposals until sproj_finish subtracts WON
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr unsigned long long kNoProposal = ~0ull;

struct Grid {
  int gx, gy, stride;  // gx * gy <= stride cells of a frame are in use; the keys of frame f start at f * stride
};

struct SearchArgs {
  const gh_keypoint* kps;
  const uint32_t* desc;  // 8 words per node
  const int32_t* counts;
  const double* cam_pose;
  const uint8_t* frame_search;
  const int32_t* node_point_in;  // may be NULL
  const int32_t* row_point_in;   // may be NULL (then row_inlier_in is NULL too)
  const uint8_t* row_inlier_in;
  const double* point_xyz;
  const int32_t* point_status;  // may be NULL
  const uint8_t* point_select;  // may be NULL
  const int32_t* point_views;
  const uint32_t* point_desc;
  const double* point_normal;
  const double* point_dist;
  int n_frames, cap, N, n_points;
  gh_map::Pinhole pin;
  double width, height;
  gh_search_params prm;
  Grid grid;
  int spare_mask;
  // scratch
  int32_t* flist;                // the searched frames, ascending
  int32_t* held;                 // n_frames tables of 2 * cap words, -1 = empty
  unsigned long long* proposal;  // per node: (h << 32) | p, all ones = none
  int32_t* key;
  const int32_t* start;
  const int32_t* list;
  // outputs
  int32_t* row_point;
  uint8_t* row_inlier;
  uint16_t* row_dist;
  int32_t* frame_totals;
  int32_t* totals;
};

// the grid cell of a coordinate along an axis of g cells: a clamp, monotone in x; NaN and everything below 0 go to cell 0
__device__ __forceinline__ int clamp_cell(double x, int g) {
  if (!(x >= 0.0)) return 0;
  const double c = x * (1.0 / kCellPixels);  // (exact: a power of two)
  return c >= (double)g ? g - 1 : (int)c;
}

__device__ __forceinline__ uint32_t held_slot(int p, uint32_t size) {
  return (uint32_t)(((unsigned long long)((uint32_t)p * 0x9E3779B1u) * size) >> 32);
}

// the point of node n when the node is TAKEN, -1 otherwise (the node exists)
__device__ __forceinline__ int taken_point(const SearchArgs& a, int n) {
  if (a.node_point_in) {
    const int p = a.node_point_in[n];
    if (p >= 0 && p < a.n_points) return p;
  }
  if (a.row_point_in && a.row_inlier_in[n] != 0) {
    const int p = a.row_point_in[n];
    if (p >= 0 && p < a.n_points) return p;
  }
  return -1;
}

__global__ __launch_bounds__(kBlock) void sproj_frames_kernel(const uint8_t* __restrict__ frame_search, int n_frames,
                                                              int32_t* __restrict__ flist, int32_t* __restrict__ totals) {
  __shared__ int s_wave[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int f0 = 0; f0 < n_frames; f0 += kBlock) {  // (uniform: n_frames is)
    const int f = f0 + threadIdx.x;
    const bool on = f < n_frames && frame_search[f] != 0;
    const unsigned long long m = __ballot(on);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      before += w < wave ? s_wave[w] : 0;
      all += s_wave[w];
    }
    if (on) flist[base + before + __popcll(m & ((1ull << lane) - 1ull))] = f;
    base += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[10] = base;
}

__global__ __launch_bounds__(kBlock) void sproj_grid_kernel(SearchArgs a) {
  const int n = blockIdx.x * kBlock + threadIdx.x;
  if (n >= a.N) return;
  a.proposal[n] = kNoProposal;
  const int f = n / a.cap, i = n - f * a.cap;
  int key = gh_map::spare_key(a.n_frames * a.grid.stride, n, a.spare_mask);
  if (a.frame_search[f] != 0 && i < gh_map::row_count(a.counts, f, a.cap)) {
    const int p = taken_point(a, n);
    if (p >= 0) {
      const uint32_t size = 2u * (uint32_t)a.cap;
      int32_t* tab = a.held + (size_t)f * size;
      uint32_t s = held_slot(p, size);
      for (;;) {  // (at most cap distinct points in 2 * cap slots: an empty one is always met)
        const int old = atomicCAS(&tab[s], -1, p);
        if (old == -1 || old == p) break;
        s = s + 1 == size ? 0 : s + 1;
      }
    } else {
      const gh_keypoint& kp = a.kps[n];
      key = f * a.grid.stride + clamp_cell((double)kp.y, a.grid.gy) * a.grid.gx + clamp_cell((double)kp.x, a.grid.gx);
    }
  }
  a.key[n] = key;
}

// the two smallest of {best, second, key}, as selects: written with branches, the compiler kept the pair in scratch memory
__device__ __forceinline__ void keep_two(uint32_t key, uint32_t& best, uint32_t& second) {
  const uint32_t larger = key < best ? best : key;
  best = key < best ? key : best;
  second = larger < second ? larger : second;
}

__global__ __launch_bounds__(kBlock) void sproj_search_kernel(SearchArgs a, gh_map::ScalePowers pw) {
  __shared__ double s_pow[kMaxLevels];
  if (threadIdx.x < kMaxLevels) s_pow[threadIdx.x] = pw.v[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & (kGroupLanes - 1), group = lane >> 3;
  const long long gp = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int p = gp < a.n_points ? (int)gp : 0;
  bool searchable = gp < a.n_points && (!a.point_select || a.point_select[p] != 0);
  searchable = searchable && (!a.point_status || a.point_status[p] == GH_TRACK_OK);
  searchable = searchable && a.point_views[p] > 0;
  double X[3] = {0.0, 0.0, 0.0}, nrm[3] = {0.0, 0.0, 0.0}, min_dist = 0.0, max_dist = 0.0;
  if (searchable) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      X[k] = a.point_xyz[3 * (size_t)p + k];
      nrm[k] = a.point_normal[3 * (size_t)p + k];
    }
    min_dist = a.point_dist[2 * (size_t)p];
    max_dist = a.point_dist[2 * (size_t)p + 1];
  }
  const int n_searched = a.totals[10];  // (sproj_frames wrote it)
  const uint32_t tab_size = 2u * (uint32_t)a.cap;

  for (int s = blockIdx.y; s < n_searched; s += gridDim.y) {  // (wave-uniform)
    const int f = a.flist[s];
    const double* pose = a.cam_pose + (size_t)f * 7;
    int verdict = -1;  // this lane's pair; -1: no pair, or a survivor whose group will judge
    bool survivor = false;
    double u = 0.0, v = 0.0, radius = 0.0;
    int level = 0;
    if (searchable) {
      const int32_t* tab = a.held + (size_t)f * tab_size;
      uint32_t slot = held_slot(p, tab_size);
      bool held = false;
      for (;;) {
        const int t = tab[slot];
        if (t == p) held = true;
        if (t == p || t == -1) break;
        slot = slot + 1 == tab_size ? 0 : slot + 1;
      }
      const double qc[4] = {-pose[0], -pose[1], -pose[2], pose[3]};
      const double d[3] = {X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]};
      double Xc[3];
      gh_ba::quat_rotate(qc, d, Xc);
      if (held) {
        verdict = 0;
      } else if (!(Xc[2] > gh_ba::kMinDepth)) {
        verdict = 1;
      } else {
        const double iz = 1.0 / Xc[2];
        u = a.pin.fx * (Xc[0] * iz) + a.pin.cx;
        v = a.pin.fy * (Xc[1] * iz) + a.pin.cy;
        if (!(0.0 <= u && u < a.width && 0.0 <= v && v < a.height)) {
          verdict = 2;
        } else {
          const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
          const double dist = sqrt(r2);
          if (!(dist >= a.prm.range_lo * min_dist && dist <= a.prm.range_hi * max_dist)) {
            verdict = 3;
          } else {
            const double c = ((d[0] * nrm[0] + d[1] * nrm[1]) + d[2] * nrm[2]) / dist;
            if (!(c >= a.prm.min_view_cos)) {
              verdict = 4;
            } else {
              for (int l = 0; l <= a.prm.n_levels - 2; ++l) level += s_pow[l] * dist < max_dist ? 1 : 0;
              radius = (a.prm.radius_scale * (c > a.prm.near_cos ? a.prm.radius_near : a.prm.radius_far)) * s_pow[level];
              survivor = true;
            }
          }
        }
      }
    }
    int cnt[9];
#pragma unroll
    for (int k = 0; k < 5; ++k) cnt[k] = gh_map::wave_count(verdict == k);
    cnt[5] = cnt[6] = cnt[7] = cnt[8] = 0;

    // the survivors, eight at a time: group g takes the g-th of the round
    unsigned long long todo = __ballot(survivor);
    while (todo) {  // (wave-uniform)
      unsigned long long m = todo;
      int src = -1;
#pragma unroll
      for (int g = 0; g < 64 / kGroupLanes; ++g) {
        const int bit = m ? __ffsll((long long)m) - 1 : -1;
        if (g == group) src = bit;
        if (m) m &= m - 1;
      }
      todo = m;
      const bool active = src >= 0;
      const int from = active ? src : lane;
      const int sp = __shfl(p, from);
      const double su = __shfl(u, from), sv = __shfl(v, from), sr = __shfl(radius, from);
      const int sl = __shfl(level, from);
      uint32_t best = kNoKey, second = kNoKey;
      if (active) {
        uint32_t pd[8];
        const uint32_t* src_desc = a.point_desc + (size_t)sp * 8;
#pragma unroll
        for (int w = 0; w < 8; ++w) pd[w] = src_desc[w];
        const int cx_lo = clamp_cell(su - sr, a.grid.gx), cx_hi = clamp_cell(su + sr, a.grid.gx);
        const int cy_lo = clamp_cell(sv - sr, a.grid.gy), cy_hi = clamp_cell(sv + sr, a.grid.gy);
        const int32_t* start = a.start + (size_t)f * a.grid.stride;
        for (int cy = cy_lo; cy <= cy_hi; ++cy) {
          const int b = start[cy * a.grid.gx + cx_lo], e = start[cy * a.grid.gx + cx_hi + 1];
          for (int k = b + j; k < e; k += kGroupLanes) {
            const int n = a.list[k];
            const gh_keypoint& kp = a.kps[n];
            const int oct = kp.octave;
            if (!(sl - 1 <= oct && oct <= sl)) continue;
            if (!(fabs((double)kp.x - su) < sr && fabs((double)kp.y - sv) < sr)) continue;
            const uint32_t(&dn)[8] = *(const uint32_t(*)[8])(a.desc + (size_t)n * 8);  // (read in place, word by word)
            const int h = gh_map::hamming256(dn, pd);
            keep_two(((uint32_t)h << 16) | (uint32_t)(n - f * a.cap), best, second);
          }
        }
      }
#pragma unroll
      for (int x = kGroupLanes / 2; x >= 1; x >>= 1) {
        const uint32_t ob = __shfl_xor(best, x), os = __shfl_xor(second, x);
        keep_two(ob, best, second);
        keep_two(os, best, second);
      }
      int gv = -1;
      if (active && j == 0) {
        if (best == kNoKey) {
          gv = 5;
        } else {
          const int hb = (int)(best >> 16), ib = (int)(best & 0xFFFFu);
          const int hs = second == kNoKey ? 256 : (int)(second >> 16);
          if (hb > a.prm.max_hamming) {
            gv = 6;
          } else {
            const int ob = a.kps[f * a.cap + ib].octave;
            const int os = second == kNoKey ? -1 : a.kps[f * a.cap + (int)(second & 0xFFFFu)].octave;
            if (ob == os && (double)hb > a.prm.nn_ratio * (double)hs) {
              gv = 7;
            } else {
              gv = 8;
              atomicMin(&a.proposal[f * a.cap + ib], ((unsigned long long)hb << 32) | (unsigned long long)(uint32_t)sp);
            }
          }
        }
      }
#pragma unroll
      for (int k = 5; k < 9; ++k) cnt[k] += gh_map::wave_count(gv == k);
    }

    int mine = 0;  // lane k carries counter k: one atomic instruction per (wave, frame)
#pragma unroll
    for (int k = 0; k < 9; ++k) mine = lane == k ? cnt[k] : mine;
    if (lane < 9 && mine) atomicAdd(&a.frame_totals[(size_t)f * kVerdicts + lane], mine);
  }

  gh_map::block_counts_add<1>({gh_map::wave_count(searchable && blockIdx.y == 0 && n_searched > 0)}, a.totals + 11);
}

__global__ __launch_bounds__(kBlock) void sproj_resolve_kernel(SearchArgs a) {
  const long long gn = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool in_range = gn < a.N;
  const int n = in_range ? (int)gn : 0;
  const int f = in_range ? n / a.cap : 0;
  bool won = false;
  if (in_range) {
    const unsigned long long w = a.proposal ? a.proposal[n] : kNoProposal;
    won = w != kNoProposal;
    int point;
    uint8_t inlier;
    if (won) {
      point = (int)(uint32_t)(w & 0xFFFFFFFFull);
      inlier = 1;
    } else if (a.row_point_in) {
      point = a.row_point_in[n];
      inlier = a.row_inlier_in[n] != 0 ? 1 : 0;
    } else {
      point = n - f * a.cap < gh_map::row_count(a.counts, f, a.cap) ? GH_LOC_NO_POINT : GH_LOC_NO_ROW;
      inlier = 0;
    }
    a.row_point[n] = point;
    a.row_inlier[n] = inlier;
    a.row_dist[n] = won ? (uint16_t)(w >> 32) : (uint16_t)0xFFFF;
  }
  gh_map::add_runs(a.frame_totals, f * kVerdicts + (kVerdicts - 1), won);
}

__global__ __launch_bounds__(kBlock) void sproj_finish_kernel(int32_t* __restrict__ frame_totals, int n_frames,
                                                              int32_t* __restrict__ totals) {
  const int f = blockIdx.x * kBlock + threadIdx.x;
  int c[kVerdicts];
#pragma unroll
  for (int k = 0; k < kVerdicts; ++k) c[k] = 0;
  if (f < n_frames) {
    int32_t* row = frame_totals + (size_t)f * kVerdicts;
#pragma unroll
    for (int k = 0; k < kVerdicts; ++k) c[k] = row[k];
    c[kProposed] -= c[kVerdicts - 1];  // LOST = PROPOSED - WON
    row[kProposed] = c[kProposed];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int k = 0; k < kVerdicts; ++k) c[k] += __shfl_xor(c[k], m);
  gh_map::block_counts_add<5>({c[0], c[1], c[2], c[3], c[4]}, totals);
  gh_map::block_counts_add<5>({c[5], c[6], c[7], c[8], c[9]}, totals + 5);
}

Grid make_grid(int width, int height, int cap) {
  long long gx = ((long long)width + kCellPixels - 1) / kCellPixels, gy = ((long long)height + kCellPixels - 1) / kCellPixels;
  if (gx > kMaxGridSide) gx = kMaxGridSide;
  if (gy > kMaxGridSide) gy = kMaxGridSide;
  const int stride = cap < kMaxGridSide * kMaxGridSide ? (cap < 1 ? 1 : cap) : kMaxGridSide * kMaxGridSide;
  while (gx * gy > stride) {  // (the last cell of an axis then takes what lies beyond it: the clamp)
    if (gx >= gy)
      gx = (gx + 1) / 2;
    else
      gy = (gy + 1) / 2;
  }
  return {(int)gx, (int)gy, stride};
}

}  // namespace

extern "C" void gh_search_default_params(gh_search_params* p) {
  if (!p) return;
  p->scale_factor = 1.2;
  p->radius_near = 2.5;
  p->radius_far = 4.0;
  p->near_cos = 0.998;
  p->radius_scale = 1.0;
  p->min_view_cos = 0.5;
  p->range_lo = 0.8;
  p->range_hi = 1.2;
  p->nn_ratio = 0.8;
  p->n_levels = 8;
  p->max_hamming = 100;
}

extern "C" int gh_search_cell_pixels(void) { return kCellPixels; }

extern "C" gh_status gh_search_projection_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const uint8_t* desc_dev, const int32_t* counts_dev,
                                              int n_frames, int cap, const double* cam_pose_dev, const uint8_t* frame_search_dev,
                                              const int32_t* node_point_in_dev, const int32_t* row_point_in_dev,
                                              const uint8_t* row_inlier_in_dev, int n_points, const double* point_xyz_dev,
                                              const int32_t* point_status_dev, const uint8_t* point_select_dev,
                                              const int32_t* point_views_dev, const uint8_t* point_desc_dev,
                                              const double* point_normal_dev, const double* point_dist_dev, double fx, double fy,
                                              double cx, double cy, int width, int height, const gh_search_params* params,
                                              int32_t* row_point_dev, uint8_t* row_inlier_dev, uint16_t* row_dist_dev,
                                              int32_t* frame_totals_dev, int32_t* totals_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, params != nullptr);
  GH_CHECK_ARG(ctx, n_frames >= 0 && cap >= 0 && n_points >= 0 && cap <= 65535);
  GH_CHECK_ARG(ctx, (long long)n_points + (long long)n_frames * cap <= (long long)INT32_MAX - 1);
  GH_CHECK_ARG(ctx, width >= 1 && height >= 1 && fx > 0.0 && fy > 0.0);
  GH_CHECK_ARG(ctx, std::isfinite(params->scale_factor) && params->scale_factor >= 1.0);
  GH_CHECK_ARG(ctx, params->n_levels >= 1 && params->n_levels <= kMaxLevels && params->max_hamming >= 0 && params->max_hamming <= 256);
  GH_CHECK_ARG(ctx, params->radius_near >= 0.0 && params->radius_far >= 0.0 && params->radius_scale >= 0.0);  // (a NaN fails too)
  GH_CHECK_ARG(ctx, !std::isnan(params->near_cos) && !std::isnan(params->min_view_cos) && !std::isnan(params->range_lo) &&
                        !std::isnan(params->range_hi) && !std::isnan(params->nn_ratio));
  GH_CHECK_ARG(ctx, kps_dev && desc_dev && counts_dev && cam_pose_dev && frame_search_dev);
  GH_CHECK_ARG(ctx, row_point_dev && row_inlier_dev && row_dist_dev && frame_totals_dev && totals_dev);
  GH_CHECK_ARG(ctx, n_points == 0 || (point_xyz_dev && point_views_dev && point_desc_dev && point_normal_dev && point_dist_dev));
  GH_CHECK_ARG(ctx, (row_point_in_dev == nullptr) == (row_inlier_in_dev == nullptr));
  GH_CHECK_ARG(ctx, gh_map::word_aligned(desc_dev, point_desc_dev));
  const int N = n_frames * cap;

  GH_HIP(ctx, hipMemsetAsync(totals_dev, 0, 12 * sizeof(int32_t), ctx->stream));
  if (N == 0) return GH_OK;
  GH_HIP(ctx, hipMemsetAsync(frame_totals_dev, 0, (size_t)n_frames * kVerdicts * sizeof(int32_t), ctx->stream));

  SearchArgs a = {};
  a.kps = kps_dev;
  a.desc = (const uint32_t*)desc_dev;
  a.counts = counts_dev;
  a.cam_pose = cam_pose_dev;
  a.frame_search = frame_search_dev;
  a.node_point_in = node_point_in_dev;
  a.row_point_in = row_point_in_dev;
  a.row_inlier_in = row_inlier_in_dev;
  a.point_xyz = point_xyz_dev;
  a.point_status = point_status_dev;
  a.point_select = point_select_dev;
  a.point_views = point_views_dev;
  a.point_desc = (const uint32_t*)point_desc_dev;
  a.point_normal = point_normal_dev;
  a.point_dist = point_dist_dev;
  a.n_frames = n_frames;
  a.cap = cap;
  a.N = N;
  a.n_points = n_points;
  a.pin = {fx, fy, cx, cy};
  a.width = (double)width;
  a.height = (double)height;
  a.prm = *params;
  a.grid = make_grid(width, height, cap);
  a.row_point = row_point_dev;
  a.row_inlier = row_inlier_dev;
  a.row_dist = row_dist_dev;
  a.frame_totals = frame_totals_dev;
  a.totals = totals_dev;

  // scratch: searched frames | HELD tables | proposals | keys | the index's work space.  The stride of a frame's keys depends
  // on cap = N / n_frames alone, so the size is a function of N, n_points and n_frames whatever the image is.
  const long long frame_keys = (long long)n_frames * a.grid.stride;  // (<= N)
  const int spare = gh_map::spare_bins(frame_keys);
  const int n_keys = (int)frame_keys + spare;
  a.spare_mask = spare - 1;
  gh_carve c;
  const size_t o_flist = c.take((size_t)n_frames * 4);
  char* base = nullptr;
  if (n_points > 0) {
    size_t work_bytes = 0;
    GH_TRY(gh_map::index_bytes(ctx, "gh_search_projection_dev", N, n_keys, &work_bytes));
    const size_t o_held = c.take((size_t)N * 2 * 4), o_prop = c.take((size_t)N * 8), o_keys = c.take((size_t)N * 4),
                 o_work = c.take(work_bytes);
    GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
    a.flist = (int32_t*)(base + o_flist);
    a.held = (int32_t*)(base + o_held);
    a.proposal = (unsigned long long*)(base + o_prop);
    a.key = (int32_t*)(base + o_keys);
    GH_LAUNCH(ctx, "sproj_frames", sproj_frames_kernel, dim3(1), dim3(kBlock), 0, frame_search_dev, n_frames, a.flist, totals_dev);
    GH_HIP(ctx, hipMemsetAsync(a.held, 0xFF, (size_t)N * 2 * 4, ctx->stream));
    GH_LAUNCH(ctx, "sproj_grid", sproj_grid_kernel, dim3(gh_div_up(N, kBlock)), dim3(kBlock), 0, a);
    GH_TRY(gh_map::build_index(ctx, "sproj_index", a.key, N, n_keys, base + o_work, work_bytes, &a.start, &a.list));  // (N > 0)

    // the frames of a call are spread over the y dimension where the points alone do not fill the device
    const int bx = gh_div_up(n_points, kBlock);
    int by = 2048 / bx;
    by = by < 1 ? 1 : (by > n_frames ? n_frames : by);
    GH_LAUNCH(ctx, "sproj_search", sproj_search_kernel, dim3(bx, by), dim3(kBlock), 0, a,
              gh_map::scale_powers(params->scale_factor));
  } else {
    GH_TRY(gh_scratch(ctx, c.at, (void**)&base));
    a.flist = (int32_t*)(base + o_flist);
    GH_LAUNCH(ctx, "sproj_frames", sproj_frames_kernel, dim3(1), dim3(kBlock), 0, frame_search_dev, n_frames, a.flist, totals_dev);
  }
  GH_LAUNCH(ctx, "sproj_resolve", sproj_resolve_kernel, dim3(gh_div_up(N, kBlock)), dim3(kBlock), 0, a);
  GH_LAUNCH(ctx, "sproj_finish", sproj_finish_kernel, dim3(gh_div_up(n_frames, kBlock)), dim3(kBlock), 0, frame_totals_dev, n_frames,
            totals_dev);
  return GH_OK;
}
