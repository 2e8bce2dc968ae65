// Batched, device-resident RANSAC: many independent problems per launch (gh_ransac_batch_dev) and the frame-pair entry in
// front of it (gh_ransac_pairs_dev).  Problem p is, bit for bit, one gh_ransac_estimate call on its rows: the sampler, the
// minimal solvers, the error and the essential projection are the functions of ransac_models.h that the single call runs.
//
// One call of gh_ransac_estimate is ~1e8 f64 operations behind four launches, two DMAs and a stream synchronise; verifying
// the 999 frame pairs of a benchmark step that way is latency, not work.  CDNA4 mapping of the batch:
//   * norm    (F / E only) Hartley normalisation, ONE LANE per problem, sums taken sequentially in index order as the host
//             loop of the single call takes them (a tree reduction would round differently);
//   * score   one LANE per hypothesis, 2048 lanes = eight 256-thread workgroups per problem.  The lane solves its minimal
//             sample, keeps the model in registers and a private integer count; the problem's correspondences pass through
//             LDS in tiles of kTileRows rows.  Every lane reads the same LDS address (a broadcast, no bank conflict), the row
//             goes to registers before model_error sees it, and no reduction is needed.  Any n takes this one path;
//   * finish  one workgroup per problem: argmax of the 2048 counts (lowest index on ties), the winner's model solved again
//             from its index (the same function on the same rows: the same bits; 2048 x 12 doubles per problem never travel
//             through memory), its mask, and for E the projection onto the essential manifold, on the device;
//   * gather  (pair entry) order-preserving compaction of a pair's kept matches into src / dst rows, one workgroup per pair.
// gh_two_view_pairs_dev (the calibrated pair entry: gather with normalisation, the E batch, then two_view.hip's kernel on the
// inliers) lives here because it is this file's gather and this file's batch_run on one scratch block.
// gh_pnp_batch_dev (pnp_batch.hip) chains the GH_MODEL_PNP batch with its own kernels through ransac_batch_ranges below.
// A problem with fewer rows than the sample, or a threshold that is negative or NaN, is skipped by every kernel BEFORE the
// sampler (whose rejection loop does not end for n < s): it is "no model".  Row ranges are clamped to the arrays before
// they address anything.
#include "estimate_batch.h"
#include "map_dev.h"

namespace {

using namespace gh_ransac;
using gh_map::Pinhole;

constexpr int kTileRows = 512;         // correspondences staged per tile: 512 x (3 + 3) doubles = 24 KB of LDS at the most
constexpr int kParts = kHyp / 256;     // workgroups per problem in the scoring kernel
constexpr int kChunk = 8192;           // problems per launch: bounds the counts block (kChunk x 2048 ints = 64 MB)

struct BatchArgs {
  const double* src;
  const double* dst;
  RowRanges range;
  int nproblems;
  double threshold;
  const double* thresholds;   // per problem, or NULL
  uint64_t seed;
  const uint64_t* seeds;      // per problem, or NULL
  Norm* norms;                // scratch, F / E
  int* counts;                // scratch, nproblems x kHyp
  const int32_t* row_map;     // pair entry: compacted row -> query row (then `mask` is npairs x map_stride, zeroed already)
  int map_stride;
  double* models;
  uint8_t* mask;
  int32_t* inliers;
};

__device__ inline double problem_threshold(const BatchArgs& a, int p) { return a.thresholds ? a.thresholds[p] : a.threshold; }
__device__ inline uint64_t problem_seed(const BatchArgs& a, int p) { return a.seeds ? a.seeds[p] : a.seed; }

// Hartley normalisation of F / E, one lane per problem: hartley_norm is what the single call runs on the host.
__global__ __launch_bounds__(64) void ransac_batch_norm_kernel(BatchArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.nproblems) return;
  int first;
  const int n = problem_rows(a.range, p, &first);
  Norm nm = {0, 0, 1, 0, 0, 1};
  if (n >= 8) nm = hartley_norm(a.src + (size_t)first * 2, a.dst + (size_t)first * 2, n);  // (fewer rows: no model, nothing reads it)
  a.norms[p] = nm;
}

template <int MODEL>
__global__ __launch_bounds__(256) void ransac_batch_score_kernel(BatchArgs a) {
  constexpr int DP = dim_p(MODEL), DQ = dim_q(MODEL);
  __shared__ double sp[kTileRows * DP];
  __shared__ double sq[kTileRows * DQ];
  const int p = blockIdx.x / kParts, tid = threadIdx.x;
  const int h = (blockIdx.x % kParts) * 256 + tid;
  int first;
  const int n = problem_rows(a.range, p, &first);
  const double thr = problem_threshold(a, p);
  if (n < sample_size(MODEL) || !(thr >= 0)) return;  // no model (the whole workgroup leaves: the finish kernel reads no count)
  const double thr2 = thr * thr;
  const double* P = a.src + (size_t)first * DP;
  const double* Q = a.dst + (size_t)first * DQ;
  Norm nm = {0, 0, 1, 0, 0, 1};
  if (MODEL == kModelF || MODEL == kModelE) nm = a.norms[p];
  double m[12];
  const bool ok = solve_hypothesis(MODEL, P, Q, n, problem_seed(a, p), nm, h, m);
  int c = 0;
  for (int t0 = 0; t0 < n; t0 += kTileRows) {
    const int rows = n - t0 < kTileRows ? n - t0 : kTileRows;
    __syncthreads();  // the previous tile has been read by every lane
    for (int k = tid; k < rows * DP; k += 256) sp[k] = P[(size_t)t0 * DP + k];
    if (MODEL != kModelPlane)  // (the plane reads src only)
      for (int k = tid; k < rows * DQ; k += 256) sq[k] = Q[(size_t)t0 * DQ + k];
    __syncthreads();
    if (ok)
      for (int i = 0; i < rows; ++i) {
        double pr[DP], qr[DQ];  // the row in registers: model_error never sees an LDS address
        for (int e = 0; e < DP; ++e) pr[e] = sp[i * DP + e];
        for (int e = 0; e < DQ; ++e) qr[e] = MODEL != kModelPlane ? sq[i * DQ + e] : 0.0;
        double err;
        if (model_error(MODEL, m, pr, qr, 0, &err) && err <= thr2) ++c;
      }
  }
  a.counts[(size_t)p * kHyp + h] = ok ? c : -1;
}

template <int MODEL>
__global__ __launch_bounds__(256) void ransac_batch_finish_kernel(BatchArgs a) {
  constexpr int DP = dim_p(MODEL), DQ = dim_q(MODEL);
  __shared__ long long red[256];
  const int p = blockIdx.x, tid = threadIdx.x;
  int first;
  const int n = problem_rows(a.range, p, &first);
  const double thr = problem_threshold(a, p);
  const double thr2 = thr * thr;
  const double* P = a.src + (size_t)first * DP;
  const double* Q = a.dst + (size_t)first * DQ;
  long long best = -1;
  if (n >= sample_size(MODEL) && thr >= 0) best = winner_key(a.counts + (size_t)p * kHyp, red);
  // every lane solves the winner again: uniform control flow, and the mask below needs the model in each lane's registers
  double m[12], out[12];
  bool have = false;
  if (best >= 0) {
    Norm nm = {0, 0, 1, 0, 0, 1};
    if (MODEL == kModelF || MODEL == kModelE) nm = a.norms[p];
    have = solve_hypothesis(MODEL, P, Q, n, problem_seed(a, p), nm, winner_index(best), m);
  }
  const int ms = model_size(MODEL);
  for (int k = 0; k < 12; ++k) out[k] = have && k < ms ? m[k] : 0.0;
  // (E: the mask is the scored estimate's, the model its projection; a failed projection is no model, mask included)
  if (MODEL == kModelE && have) have = project_essential(out);
  if (tid == 0) {
    for (int k = 0; k < 12; ++k) a.models[(size_t)p * 12 + k] = have ? out[k] : 0.0;
    a.inliers[p] = have ? winner_count(best) : 0;
  }
  if (!a.mask) return;
  if (a.row_map) {  // pair entry: the gather kernel has zeroed the pair's row of the mask
    if (!have) return;
    uint8_t* mask = a.mask + (size_t)p * a.map_stride;
    for (int i = tid; i < n; i += 256) {
      double e;
      if (model_error(MODEL, m, P, Q, i, &e) && e <= thr2) mask[a.row_map[first + i]] = 1;
    }
    return;
  }
  for (int i = tid; i < n; i += 256) {
    double e;
    a.mask[(size_t)first + i] = (have && model_error(MODEL, m, P, Q, i, &e) && e <= thr2) ? 1 : 0;
  }
}

// Pair p's correspondences: the query rows i < counts[pair_q[p]], ascending, with keep[i] (if given) and
// 0 <= idx1[i] < counts[pair_t[p]].  Written to rows p * cap ... of src / dst (float -> double is exact) with the query row of
// each in row_map; the pair's row of the inlier mask is cleared here.  NORMALISE (gh_two_view_pairs_dev): pinhole intrinsics
// k turn the pixels into normalised coordinates in double (gh_map::normalised_xy, map_dev.h).
template <bool NORMALISE>
__global__ __launch_bounds__(256) void ransac_pairs_gather_kernel(Pinhole k, const gh_keypoint* __restrict__ kps,
                                                                  const int32_t* __restrict__ counts,
                                                                  int cap, const int32_t* __restrict__ pair_q,
                                                                  const int32_t* __restrict__ pair_t, const int32_t* __restrict__ idx1,
                                                                  const uint8_t* __restrict__ keep, double* __restrict__ src,
                                                                  double* __restrict__ dst, int32_t* __restrict__ row_map,
                                                                  int32_t* __restrict__ row_begin, int32_t* __restrict__ row_end,
                                                                  int32_t* __restrict__ n_corr, uint8_t* __restrict__ inlier) {
  __shared__ int wave_total[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int fq = pair_q[p], ft = pair_t[p];
  int cq = counts[fq], ct = counts[ft];
  cq = cq < 0 ? 0 : (cq > cap ? cap : cq);
  ct = ct < 0 ? 0 : (ct > cap ? cap : ct);
  const size_t row0 = (size_t)p * cap;
  int base = 0;
  for (int i0 = 0; i0 < cap; i0 += 256) {
    const int i = i0 + tid;
    int j = -1;
    bool take = false;
    if (i < cap) inlier[row0 + i] = 0;
    if (i < cq) {
      j = idx1[row0 + i];
      take = (!keep || keep[row0 + i]) && j >= 0 && j < ct;
    }
    compact_trip(take, &base, wave_total, [&](int at) {
      const gh_keypoint* kq = kps + (size_t)fq * cap + i;
      const gh_keypoint* kt = kps + (size_t)ft * cap + j;
      const size_t r = row0 + at;
      if (NORMALISE) {
        gh_map::normalised_xy(*kq, k, src + 2 * r);
        gh_map::normalised_xy(*kt, k, dst + 2 * r);
      } else {
        src[2 * r] = (double)kq->x;
        src[2 * r + 1] = (double)kq->y;
        dst[2 * r] = (double)kt->x;
        dst[2 * r + 1] = (double)kt->y;
      }
      row_map[r] = i;
    });
  }
  if (tid == 0) {
    row_begin[p] = (int32_t)row0;
    row_end[p] = (int32_t)row0 + base;
    n_corr[p] = base;
  }
}

template <int MODEL>
gh_status batch_launch(gh_ctx* ctx, const BatchArgs& a) {
  if (MODEL == kModelF || MODEL == kModelE)
    GH_LAUNCH(ctx, "ransac_batch_norm", ransac_batch_norm_kernel, dim3(gh_div_up(a.nproblems, 64)), dim3(64), 0, a);
  GH_LAUNCH(ctx, "ransac_batch_score", ransac_batch_score_kernel<MODEL>, dim3(a.nproblems * kParts), dim3(256), 0, a);
  GH_LAUNCH(ctx, "ransac_batch_finish", ransac_batch_finish_kernel<MODEL>, dim3(a.nproblems), dim3(256), 0, a);
  return GH_OK;
}

// `work`: ransac_batch_scratch_bytes(nproblems) bytes of device scratch.  Problems go kChunk at a time (stream order keeps the
// shared scratch safe); every per-problem array of `all` moves with the chunk, rows stay absolute.
gh_status batch_run(gh_ctx* ctx, int model, const BatchArgs& all, void* work) {
  for (int p0 = 0; p0 < all.nproblems; p0 += kChunk) {
    BatchArgs a = all;
    a.nproblems = all.nproblems - p0 < kChunk ? all.nproblems - p0 : kChunk;
    a.range.row_begin += p0;
    a.range.row_end += p0;
    if (a.thresholds) a.thresholds += p0;
    if (a.seeds) a.seeds += p0;
    a.models += (size_t)p0 * 12;
    a.inliers += p0;
    if (a.row_map && a.mask) a.mask += (size_t)p0 * a.map_stride;
    a.norms = (Norm*)work;
    a.counts = (int*)((uint8_t*)work + gh_round256((size_t)a.nproblems * sizeof(Norm)));
    switch (model) {
      case kModelH: GH_TRY(batch_launch<kModelH>(ctx, a)); break;
      case kModelA2: GH_TRY(batch_launch<kModelA2>(ctx, a)); break;
      case kModelF: GH_TRY(batch_launch<kModelF>(ctx, a)); break;
      case kModelA3: GH_TRY(batch_launch<kModelA3>(ctx, a)); break;
      case kModelE: GH_TRY(batch_launch<kModelE>(ctx, a)); break;
      case kModelSim3: GH_TRY(batch_launch<kModelSim3>(ctx, a)); break;
      case kModelPlane: GH_TRY(batch_launch<kModelPlane>(ctx, a)); break;
      default: GH_TRY(batch_launch<kModelPnP>(ctx, a)); break;
    }
  }
  return GH_OK;
}

// The scratch block of a pair entry: src | dst (npairs x cap x 2 doubles each) | row_map | row_begin | row_end | the core's
// own block.  ONE block for every stage of the call (gh_scratch hands out one block per context).
struct PairScratch {
  size_t rows, dst, map, begin, end, work, total;  // (src is at 0)
  PairScratch(int npairs, int cap)
      : rows((size_t)npairs * cap), dst(gh_round256(rows * 16)), map(2 * dst), begin(map + gh_round256(rows * 4)),
        end(begin + gh_round256((size_t)npairs * 4)), work(end + gh_round256((size_t)npairs * 4)),
        total(work + ransac_batch_scratch_bytes(npairs)) {}
};

// What both pair entries do once their own arguments are in order: refuse a bad shape or a NULL array, take the scratch,
// gather every pair's correspondences (NORMALISE: to the normalised coordinates of pinhole k) and describe them to the core.
// *a and *work are what batch_run takes; a->nproblems = 0 (and nothing launched) when there are no pairs.
template <bool NORMALISE>
gh_status pairs_front(gh_ctx* ctx, Pinhole k, const gh_keypoint* kps_dev, const int32_t* counts_dev, int cap,
                      const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                      const uint8_t* keep_dev, double threshold, uint64_t seed, double* models_dev, uint8_t* inlier_dev,
                      int32_t* n_corr_dev, int32_t* inliers_dev, BatchArgs* a, void** work) {
  *a = {};
  GH_CHECK_ARG(ctx, cap >= 0 && cap <= 65535 && npairs >= 0);
  GH_CHECK_ARG(ctx, threshold >= 0 && (long long)npairs * (cap > 0 ? cap : 1) <= 0x7FFFFFFFll && npairs <= (1 << 27));
  if (npairs == 0) return GH_OK;
  GH_CHECK_ARG(ctx, kps_dev && counts_dev && pair_q_dev && pair_t_dev && idx1_dev && models_dev && inlier_dev && n_corr_dev &&
                        inliers_dev);
  const PairScratch at(npairs, cap);
  void* base = nullptr;
  GH_TRY(gh_scratch(ctx, at.total, &base));
  uint8_t* b = (uint8_t*)base;
  double *src = (double*)b, *dst = (double*)(b + at.dst);
  int32_t *row_map = (int32_t*)(b + at.map), *row_begin = (int32_t*)(b + at.begin), *row_end = (int32_t*)(b + at.end);
  GH_LAUNCH(ctx, NORMALISE ? "two_view_pairs_gather" : "ransac_pairs_gather", ransac_pairs_gather_kernel<NORMALISE>, dim3(npairs),
            dim3(256), 0, k, kps_dev, counts_dev, cap, pair_q_dev, pair_t_dev, idx1_dev, keep_dev, src, dst, row_map, row_begin,
            row_end, n_corr_dev, inlier_dev);
  a->src = src;
  a->dst = dst;
  a->range = {row_begin, row_end, nullptr, (int)at.rows};
  a->nproblems = npairs;
  a->threshold = threshold;
  a->seed = seed;
  a->row_map = row_map;
  a->map_stride = cap;
  a->models = models_dev;
  a->mask = inlier_dev;
  a->inliers = inliers_dev;
  *work = b + at.work;
  return GH_OK;
}

}  // namespace

namespace gh_ransac {

size_t ransac_batch_scratch_bytes(int nproblems) {
  const size_t np = nproblems < kChunk ? nproblems : kChunk;
  return gh_round256(np * sizeof(Norm)) + gh_round256(np * kHyp * sizeof(int));
}

gh_status ransac_batch_ranges(gh_ctx* ctx, int model, const double* src, const double* dst, const RowRanges& range,
                              int nproblems, double threshold, const double* thresholds, uint64_t seed, const uint64_t* seeds,
                              double* models, uint8_t* mask, int32_t* inliers, void* work) {
  BatchArgs a = {};
  a.src = src;
  a.dst = dst;
  a.range = range;
  a.nproblems = nproblems;
  a.threshold = threshold;
  a.thresholds = thresholds;
  a.seed = seed;
  a.seeds = seeds;
  a.models = models;
  a.mask = mask;
  a.inliers = inliers;
  return batch_run(ctx, model, a, work);
}

}  // namespace gh_ransac

extern "C" int gh_ransac_batch_tile_rows(int model) { return model >= 0 && model <= 7 ? kTileRows : 0; }

extern "C" gh_status gh_ransac_batch_dev(gh_ctx* ctx, int model, const double* src_dev, const double* dst_dev,
                                         const int32_t* offsets_dev, int nproblems, double threshold,
                                         const double* thresholds_dev, uint64_t seed, const uint64_t* seeds_dev,
                                         double* models_dev, uint8_t* mask_dev, int32_t* inliers_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, model >= 0 && model <= 7 && nproblems >= 0 && nproblems <= (1 << 27));
  GH_CHECK_ARG(ctx, thresholds_dev || threshold >= 0);
  if (nproblems == 0) return GH_OK;
  GH_CHECK_ARG(ctx, src_dev && dst_dev && offsets_dev && models_dev && inliers_dev);
  void* work = nullptr;
  GH_TRY(gh_scratch(ctx, ransac_batch_scratch_bytes(nproblems), &work));
  const RowRanges range = {offsets_dev, offsets_dev + 1, offsets_dev + nproblems, INT_MAX};  // the arrays hold offsets[nproblems] rows
  return ransac_batch_ranges(ctx, model, src_dev, dst_dev, range, nproblems, threshold, thresholds_dev, seed, seeds_dev, models_dev,
                             mask_dev, inliers_dev, work);
}

extern "C" gh_status gh_ransac_pairs_dev(gh_ctx* ctx, int model, const gh_keypoint* kps_dev, const int32_t* counts_dev, int cap,
                                         const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs,
                                         const int32_t* idx1_dev, const uint8_t* keep_dev, double threshold, uint64_t seed,
                                         double* models_dev, uint8_t* inlier_dev, int32_t* n_corr_dev, int32_t* inliers_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, model == kModelH || model == kModelA2 || model == kModelF);
  BatchArgs a;
  void* work = nullptr;
  GH_TRY(pairs_front<false>(ctx, Pinhole{1, 1, 0, 0}, kps_dev, counts_dev, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev, keep_dev,
                            threshold, seed, models_dev, inlier_dev, n_corr_dev, inliers_dev, &a, &work));
  return batch_run(ctx, model, a, work);
}

extern "C" gh_status gh_two_view_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int cap,
                                           const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs,
                                           const int32_t* idx1_dev, const uint8_t* keep_dev, double fx, double fy, double cx,
                                           double cy, double threshold, uint64_t seed, const gh_two_view_params* params,
                                           double* models_dev, uint8_t* inlier_dev, int32_t* n_corr_dev, int32_t* inliers_dev,
                                           double* poses_dev, double* points_dev, uint8_t* good_dev, int32_t* votes_dev,
                                           int32_t* status_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, fx > 0 && fy > 0 && cx == cx && cy == cy);
  GH_CHECK_ARG(ctx, two_view_params_ok(params));
  // (every refusal comes before the first launch; no pairs is nothing to do, whatever the pointers)
  GH_CHECK_ARG(ctx, npairs <= 0 || (poses_dev && points_dev && good_dev && votes_dev && status_dev));
  BatchArgs a;
  void* work = nullptr;
  GH_TRY(pairs_front<true>(ctx, Pinhole{fx, fy, cx, cy}, kps_dev, counts_dev, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev,
                           keep_dev, threshold, seed, models_dev, inlier_dev, n_corr_dev, inliers_dev, &a, &work));
  if (npairs == 0) return GH_OK;
  GH_TRY(batch_run(ctx, kModelE, a, work));
  TwoViewArgs t = {};  // the two-view kernel reads the gathered rows and the row map again
  t.E = models_dev;
  t.e_stride = 12;
  t.src = a.src;
  t.dst = a.dst;
  t.range = a.range;
  t.nproblems = npairs;
  t.mask = inlier_dev;
  t.row_map = a.row_map;
  t.map_stride = cap;
  t.prm = *params;
  t.poses = poses_dev;
  t.points = points_dev;
  t.good = good_dev;
  t.counts = votes_dev;
  t.status = status_dev;
  return two_view_launch(ctx, t);
}
