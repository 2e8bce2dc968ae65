// Two-view reconstruction, batched and device-resident (gh_two_view_batch_dev; the pair entry gh_two_view_pairs_dev sits
// with its gather in ransac_batch.hip): the relative pose and the 3-D points of an essential matrix and its inliers.
//
// Per problem this is a 3 x 3 eigen-decomposition and four midpoint triangulations per row: a few hundred f64 operations
// per row, nothing a roofline would notice.  What it replaces is, per frame pair, an SVD on the host, four gh_triangulate
// round trips (upload, launch, download, synchronise each) and a vote; the kernel is designed against that launch latency.
// CDNA4 mapping:
//   * one 256-thread workgroup per problem, like ransac_batch_finish_kernel;
//   * every lane runs the decomposition redundantly in registers: control flow stays uniform, nothing is broadcast;
//   * rows go tid, tid + 256, ...; a lane evaluates the four candidates on its row;
//   * the four counts (and the number of rows that take part) are INTEGER sums: __popcll(__ballot(good)) per wave, kept in a
//     wave-uniform register over the row loop, the four waves combined through 4 x 5 ints of LDS.  No floating-point
//     reduction anywhere: the result does not depend on any order and is the same bits on every run;
//   * after the vote a second pass over the rows computes the winner's points again with the same function (the same
//     bits) and writes point and good for every row, the zeros included.
// Any n takes this one path.  Row ranges are clamped to the arrays before they address anything.
#include "estimate_batch.h"

namespace gh_ransac {

namespace {

__global__ __launch_bounds__(256) void two_view_kernel(TwoViewArgs a) {
  __shared__ int wave_sum[4][5];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int first;
  const int n = problem_rows(a.range, p, &first);
  const double* P = a.src + (size_t)first * 2;   // (not dereferenced when n = 0)
  const double* Q = a.dst + (size_t)first * 2;
  // pair entry: mask / good / points of the problem start at its row of the npairs x map_stride arrays
  const size_t out0 = a.row_map ? (size_t)p * a.map_stride : (size_t)first;
  const int32_t* map = a.row_map ? a.row_map + first : nullptr;

  double E[9], Ra[9], Rb[9], th[3], tn[3];
  for (int k = 0; k < 9; ++k) E[k] = a.E[(size_t)p * a.e_stride + k];
  const bool have = two_view_decompose(E, Ra, Rb, th);
  for (int k = 0; k < 3; ++k) tn[k] = -th[k];
  const double c2 = a.prm.min_parallax_cos * a.prm.min_parallax_cos, r2 = a.prm.max_reproj * a.prm.max_reproj;

  int cnt[5] = {0, 0, 0, 0, 0};  // good under candidates 0 .. 3, rows that take part: the sums of this lane's WAVE
  for (int i0 = 0; i0 < n; i0 += 256) {  // (every lane makes every trip: the ballots below are whole-wave)
    const int i = i0 + tid;
    bool use = false, g0 = false, g1 = false, g2 = false, g3 = false;
    if (i < n) use = !a.mask || a.mask[out0 + (map ? map[i] : i)] != 0;
    if (use && have) {
      const double x = P[2 * (size_t)i], y = P[2 * (size_t)i + 1], u = Q[2 * (size_t)i], v = Q[2 * (size_t)i + 1];
      double X[3];
      g0 = two_view_row(Ra, th, x, y, u, v, c2, r2, X);
      g1 = two_view_row(Ra, tn, x, y, u, v, c2, r2, X);
      g2 = two_view_row(Rb, th, x, y, u, v, c2, r2, X);
      g3 = two_view_row(Rb, tn, x, y, u, v, c2, r2, X);
    }
    cnt[0] += __popcll(__ballot(g0));
    cnt[1] += __popcll(__ballot(g1));
    cnt[2] += __popcll(__ballot(g2));
    cnt[3] += __popcll(__ballot(g3));
    cnt[4] += __popcll(__ballot(use));
  }
  if (lane == 0)
    for (int k = 0; k < 5; ++k) wave_sum[w][k] = cnt[k];
  __syncthreads();
  long long good[4], used;  // every lane adds the four waves: the vote is uniform
  for (int k = 0; k < 4; ++k) good[k] = (long long)wave_sum[0][k] + wave_sum[1][k] + wave_sum[2][k] + wave_sum[3][k];
  used = (long long)wave_sum[0][4] + wave_sum[1][4] + wave_sum[2][4] + wave_sum[3][4];

  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (good[k] > good[best]) best = k;
  int status = GH_TWO_VIEW_OK;
  if (!have || used == 0) {
    status = GH_TWO_VIEW_NO_MODEL;
  } else if (good[best] < (long long)a.prm.min_good || 1000 * good[best] < (long long)a.prm.min_good_permille * used) {
    status = GH_TWO_VIEW_TOO_FEW;
  } else {
    for (int k = 0; k < 4; ++k)
      if (k != best && 10 * good[k] > 7 * good[best]) status = GH_TWO_VIEW_AMBIGUOUS;
  }
  const double* R = best < 2 ? Ra : Rb;
  const double* t = (best & 1) ? tn : th;
  if (tid == 0) {
    a.status[p] = status;
    for (int k = 0; k < 4; ++k) a.counts[(size_t)p * 4 + k] = status == GH_TWO_VIEW_NO_MODEL ? 0 : (int32_t)good[k];
    if (a.n_used) a.n_used[p] = (int32_t)used;
    double pose[7] = {0, 0, 0, 0, 0, 0, 0};
    if (status == GH_TWO_VIEW_OK) {
      two_view_quat(R, pose);
      for (int k = 0; k < 3; ++k) pose[4 + k] = t[k];
    }
    for (int k = 0; k < 7; ++k) a.poses[(size_t)p * 7 + k] = pose[k];
  }

  // second pass: the winner's points again (the same function on the same row: the same bits), zeros everywhere else
  if (map) {  // pair entry: rows of the pair that were not gathered are cleared as well
    for (int i = tid; i < a.map_stride; i += 256) {
      a.good[out0 + i] = 0;
      for (int k = 0; k < 3; ++k) a.points[3 * (out0 + i) + k] = 0.0;
    }
    __syncthreads();  // the zeros are in place before another lane writes a gathered row (`map` is uniform)
  }
  for (int i = tid; i < n; i += 256) {
    const size_t o = out0 + (map ? map[i] : i);
    double X[3] = {0.0, 0.0, 0.0};
    bool g = false;
    if (status == GH_TWO_VIEW_OK && (!a.mask || a.mask[o] != 0)) {
      g = two_view_row(R, t, P[2 * (size_t)i], P[2 * (size_t)i + 1], Q[2 * (size_t)i], Q[2 * (size_t)i + 1], c2, r2, X);
      if (!g) X[0] = X[1] = X[2] = 0.0;
    }
    if (map && !g) continue;
    a.good[o] = g ? 1 : 0;
    for (int k = 0; k < 3; ++k) a.points[3 * o + k] = X[k];
  }
}

}  // namespace

bool two_view_params_ok(const gh_two_view_params* prm) {
  return prm && prm->min_parallax_cos > 0.0 && prm->min_parallax_cos <= 1.0 && prm->max_reproj >= 0.0;
}

gh_status two_view_launch(gh_ctx* ctx, const TwoViewArgs& a) {
  GH_LAUNCH(ctx, "two_view", two_view_kernel, dim3(a.nproblems), dim3(256), 0, a);
  return GH_OK;
}

}  // namespace gh_ransac

extern "C" void gh_two_view_default_params(gh_two_view_params* p) {
  if (!p) return;
  p->min_parallax_cos = 0.99998;
  p->max_reproj = 0.004;
  p->min_good = 50;
  p->min_good_permille = 900;
}

extern "C" gh_status gh_two_view_batch_dev(gh_ctx* ctx, const double* E_dev, int e_stride, const double* src_dev,
                                           const double* dst_dev, const int32_t* offsets_dev, int nproblems,
                                           const uint8_t* mask_dev, const gh_two_view_params* params, double* poses_dev,
                                           double* points_dev, uint8_t* good_dev, int32_t* counts_dev, int32_t* n_used_dev,
                                           int32_t* status_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, nproblems >= 0 && nproblems <= (1 << 27) && e_stride >= 9);
  GH_CHECK_ARG(ctx, gh_ransac::two_view_params_ok(params));
  if (nproblems == 0) return GH_OK;
  GH_CHECK_ARG(ctx, E_dev && src_dev && dst_dev && offsets_dev && poses_dev && points_dev && good_dev && counts_dev &&
                        n_used_dev && status_dev);
  gh_ransac::TwoViewArgs a = {};
  a.E = E_dev;
  a.e_stride = e_stride;
  a.src = src_dev;
  a.dst = dst_dev;
  a.range = {offsets_dev, offsets_dev + 1, offsets_dev + nproblems, INT_MAX};  // the arrays hold offsets[nproblems] rows
  a.nproblems = nproblems;
  a.mask = mask_dev;
  a.prm = *params;
  a.poses = poses_dev;
  a.points = points_dev;
  a.good = good_dev;
  a.counts = counts_dev;
  a.n_used = n_used_dev;
  a.status = status_dev;
  return gh_ransac::two_view_launch(ctx, a);
}
