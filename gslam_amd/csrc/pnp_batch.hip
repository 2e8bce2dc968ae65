// Pose refinement after the PnP RANSAC, batched and device-resident: gh_pnp_refine_batch_dev (many independent pose-only LM
// problems per launch) and gh_pnp_batch_dev (RANSAC fit, Huber refinement on its inliers, refit on the rows within
// `inlier_threshold`: the two rounds a tracking front end runs per frame, for every problem in one call).
//
// gh_ba_pnp is one upload, one launch on a grid of ONE workgroup, one download and a stream synchronise per problem; whoever
// holds N fits on the device pays N round trips plus the host's conversion and compaction.  The LM loop already runs inside
// one workgroup (pnp_lm.h), so the batch is a grid over problems.  CDNA4 mapping:
//   * one 256-thread workgroup per problem, p = blockIdx.x; the mapping of the single call, which is what keeps the sums
//     (and so every bit of the result) those of gh_ba_pnp.  One wave per problem would be another order of additions;
//   * start    every lane reads the start and converts it redundantly in registers (uniform control flow, no broadcast);
//   * compact  the participating rows (mask != 0), ascending, go to an int32 list in context scratch, the problem's segment
//              at its first row: chunks of 256 rows, __ballot / __popcll prefix counts per wave, the four waves combined
//              through LDS.  Thread j of the LM body then sees the j-th participating row, exactly as it would in a
//              gh_ba_pnp call on the compacted rows: every block sum adds the same numbers in the same order;
//   * refine   pnp_lm_body<indexed, no trace>;
//   * classify a last pass over ALL rows of the range at the final pose, counts by ballot (integer sums).
// Row ranges are clamped to the arrays before they address anything; every list entry is a row of the problem's own range.
#include "pnp_lm.h"
#include "estimate_batch.h"

namespace {

using namespace gh_ba;
using namespace gh_ransac;

struct PnpBatchArgs {
  const double* xyz;
  const double* xy;
  RowRanges range;
  int nproblems;
  const uint8_t* mask;        // rows that take part, or NULL: all
  const double* start;        // per problem: start_stride doubles
  int start_stride;           // 7: a T_wc pose; 12: a GH_MODEL_PNP model
  int dof;
  gh_ba_options opt;
  int min_rows;
  double inlier_threshold;    // < 0: nothing is classified
  int32_t* rows;              // scratch: `limit` ints, the list of problem p at its first row
  double* poses;
  double* info;               // may be NULL
  gh_pnp_batch_summary* summaries;
  int summary_stride;         // summaries of problem p at p * summary_stride (the chain interleaves its two rounds)
  uint8_t* inlier;            // may be NULL
  int32_t* n_inliers;         // may be NULL
};

// Two waves per SIMD (two problems per CU): without the bound the compiler takes 256 VGPRs plus AGPRs for the body's 36
// accumulators and one problem fills a CU; with it, 256 VGPRs and 20 bytes of scratch.  Measured on 999 x 300 rows: 234 -> 139 us.
// It is a register budget only: the arithmetic and its order are untouched.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pnp_refine_batch_kernel(PnpBatchArgs a) {
  __shared__ PnpLmShared S;
  __shared__ int wave_cnt[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // problem_rows (estimate_batch.h), spelled out: through the call the compiler settles on another polarity of the test, and
  // under the two-wave register bound below that costs 8 more spilled registers (36 instead of 20 bytes of scratch)
  int limit = a.range.limit;
  if (a.range.limit_dev && *a.range.limit_dev < limit) limit = *a.range.limit_dev;
  const int first = a.range.row_begin[p], end = a.range.row_end[p];
  const int n = (first < 0 || end > limit || end <= first) ? 0 : end - first;

  double pose[7];
  bool have;
  if (a.start_stride == 12) {
    double m[12];
    for (int k = 0; k < 12; ++k) m[k] = a.start[(size_t)p * 12 + k];
    have = pnp_pose_from_model(m, pose);
  } else {
    for (int k = 0; k < 7; ++k) pose[k] = a.start[(size_t)p * 7 + k];
    have = pnp_start_ok(pose);
    if (!have)
      for (int k = 0; k < 7; ++k) pose[k] = 0.0;
  }

  // compaction: the participating rows, ascending (every lane makes every trip: the ballots are whole-wave)
  int32_t* list = a.rows + (n > 0 ? first : 0);  // (not dereferenced when n = 0)
  int n_used = 0;
  if (have) {
    for (int i0 = 0; i0 < n; i0 += 256) {
      const int i = i0 + tid;
      const bool use = i < n && (!a.mask || a.mask[(size_t)first + i] != 0);
      compact_trip(use, &n_used, wave_cnt, [&](int at) { list[at] = first + i; });
    }
  }

  gh_pnp_batch_summary* sum = a.summaries + (size_t)p * a.summary_stride;
  double* info = a.info ? a.info + (size_t)p * 36 : nullptr;
  if (!have || n_used < a.min_rows) {  // GH_PNP_NO_START (pose: zeros) / GH_PNP_TOO_FEW (pose: the start), not optimised
    if (tid < 7) a.poses[(size_t)p * 7 + tid] = pose[tid];
    if (info && tid < 36) info[tid] = 0.0;
    if (tid == 0) {
      sum->iterations = 0;
      sum->accepted = 0;
      sum->termination = have ? GH_PNP_TOO_FEW : GH_PNP_NO_START;
      sum->n_used = n_used;
      sum->initial_cost = 0.0;
      sum->final_cost = 0.0;
    }
  } else {
    if (tid < 7) S.pose[tid] = pose[tid];
    __syncthreads();
    PnpLmResult res;
    pnp_lm_body<true, false>(S, a.xyz, a.xy, list, n_used, a.dof, a.opt, info, nullptr, res);
    __syncthreads();
    for (int k = 0; k < 7; ++k) pose[k] = S.pose[k];
    if (tid < 7) a.poses[(size_t)p * 7 + tid] = pose[tid];
    if (tid == 0) {
      sum->iterations = res.iterations;
      sum->accepted = res.accepted;
      sum->termination = res.termination;
      sum->n_used = n_used;
      sum->initial_cost = res.initial_cost;
      sum->final_cost = res.final_cost;
    }
  }

  // classification of ALL rows of the range, masked or not, at the pose just written (zeros without a start or a threshold)
  const bool classify = have && a.inlier_threshold >= 0;
  const double t2 = a.inlier_threshold * a.inlier_threshold;
  int cnt = 0;  // the sum of this lane's WAVE
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    bool in = false;
    if (classify && i < n) {
      const size_t r = (size_t)first + i;
      Obs o;
      if (linearize<false>(pose, 0, a.xyz + 3 * r, 0, a.xy + 2 * r, nullptr, 0.0, o)) in = o.r[0] * o.r[0] + o.r[1] * o.r[1] <= t2;
    }
    if (a.inlier && i < n) a.inlier[(size_t)first + i] = in ? 1 : 0;
    cnt += __popcll(__ballot(in));
  }
  if (a.n_inliers) {
    __syncthreads();  // (wave_cnt: the last trip of the compaction has been read)
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (tid == 0) a.n_inliers[p] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  }
}

// The chain's ranges: problem p's own when it has rows, else (0, 0) -- every stage of the chain then sees the same rows,
// and the masks of nrows bytes hold them.
__global__ __launch_bounds__(256) void pnp_batch_ranges_kernel(RowRanges offsets, int nproblems, int32_t* __restrict__ row_begin,
                                                               int32_t* __restrict__ row_end) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nproblems) return;
  int first;
  const int n = problem_rows(offsets, p, &first);
  if (n == 0) first = 0;
  row_begin[p] = first;
  row_end[p] = first + n;
}

gh_status refine_launch(gh_ctx* ctx, const PnpBatchArgs& a) {
  GH_LAUNCH(ctx, "pnp_refine_batch", pnp_refine_batch_kernel, dim3(a.nproblems), dim3(256), 0, a);
  return GH_OK;
}

gh_ba_options options_or_default(const gh_ba_options* options) {
  gh_ba_options o;
  gh_ba_default_options(&o);
  if (options) o = *options;
  return o;
}

}  // namespace

extern "C" int gh_pnp_pose_from_model(const double* model12, double* pose7) {
  if (!model12 || !pose7) return 0;
  return gh_ransac::pnp_pose_from_model(model12, pose7) ? 1 : 0;
}

extern "C" gh_status gh_pnp_refine_batch_dev(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev,
                                             int nproblems, int nrows, const uint8_t* mask_dev, const double* start_dev,
                                             int start_stride, int dof, const gh_ba_options* options, int min_rows,
                                             double inlier_threshold, double* poses_dev, double* info_dev,
                                             gh_pnp_batch_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, nproblems >= 0 && nproblems <= (1 << 27) && nrows >= 0);
  GH_CHECK_ARG(ctx, (start_stride == 7 || start_stride == 12) && min_rows >= 0 && inlier_threshold == inlier_threshold);
  if (nproblems == 0) return GH_OK;
  GH_CHECK_ARG(ctx, xyz_dev && xy_dev && offsets_dev && start_dev && poses_dev && summaries_dev);
  void* rows = nullptr;
  GH_TRY(gh_scratch(ctx, gh_round256((size_t)nrows * 4), &rows));
  PnpBatchArgs a = {};
  a.xyz = xyz_dev;
  a.xy = xy_dev;
  a.range = {offsets_dev, offsets_dev + 1, offsets_dev + nproblems, nrows};
  a.nproblems = nproblems;
  a.mask = mask_dev;
  a.start = start_dev;
  a.start_stride = start_stride;
  a.dof = dof;
  a.opt = options_or_default(options);
  a.min_rows = min_rows;
  a.inlier_threshold = inlier_threshold;
  a.rows = (int32_t*)rows;
  a.poses = poses_dev;
  a.info = info_dev;
  a.summaries = summaries_dev;
  a.summary_stride = 1;
  a.inlier = inlier_dev;
  a.n_inliers = n_inliers_dev;
  return refine_launch(ctx, a);
}

namespace gh_ransac {

bool pnp_batch_args_ok(int nproblems, int nrows, double ransac_threshold, int min_rows, double inlier_threshold) {
  return nproblems >= 0 && nproblems <= (1 << 27) && nrows >= 0 && min_rows >= 0 && ransac_threshold >= 0 &&
         inlier_threshold >= 0;  // (a NaN fails both)
}

// row list | RANSAC mask | round-1 inliers | round-1 poses | row_begin | row_end | the RANSAC core's own block
struct PnpChainLayout {
  size_t o_mask, o_in1, o_pose1, o_begin, o_end, o_work;
};

static PnpChainLayout pnp_chain_layout(int nproblems, int nrows) {
  const size_t np = (size_t)nproblems;
  PnpChainLayout L;
  L.o_mask = gh_round256((size_t)nrows * 4);
  L.o_in1 = L.o_mask + gh_round256((size_t)nrows);
  L.o_pose1 = L.o_in1 + gh_round256((size_t)nrows);
  L.o_begin = L.o_pose1 + gh_round256(np * 56);
  L.o_end = L.o_begin + gh_round256(np * 4);
  L.o_work = L.o_end + gh_round256(np * 4);
  return L;
}

size_t pnp_batch_scratch_bytes(int nproblems, int nrows) {
  return pnp_chain_layout(nproblems, nrows).o_work + ransac_batch_scratch_bytes(nproblems);
}

gh_status pnp_batch_on(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev, int nproblems, int nrows,
                       double ransac_threshold, uint64_t seed, int dof, const gh_ba_options* options, int min_rows,
                       double inlier_threshold, double* models_dev, int32_t* ransac_inliers_dev, double* poses_dev, double* info_dev,
                       gh_pnp_batch_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, void* work) {
  const PnpChainLayout L = pnp_chain_layout(nproblems, nrows);
  uint8_t* b = (uint8_t*)work;
  int32_t* row_begin = (int32_t*)(b + L.o_begin);
  int32_t* row_end = (int32_t*)(b + L.o_end);
  GH_LAUNCH(ctx, "pnp_batch_ranges", pnp_batch_ranges_kernel, dim3(gh_div_up(nproblems, 256)), dim3(256), 0,
            RowRanges{offsets_dev, offsets_dev + 1, offsets_dev + nproblems, nrows}, nproblems, row_begin, row_end);
  const RowRanges range = {row_begin, row_end, nullptr, nrows};
  GH_TRY(ransac_batch_ranges(ctx, kModelPnP, xyz_dev, xy_dev, range, nproblems, ransac_threshold, nullptr, seed, nullptr, models_dev,
                             b + L.o_mask, ransac_inliers_dev, b + L.o_work));
  PnpBatchArgs a = {};
  a.xyz = xyz_dev;
  a.xy = xy_dev;
  a.range = range;
  a.nproblems = nproblems;
  a.dof = dof;
  a.opt = options_or_default(options);
  a.min_rows = min_rows;
  a.inlier_threshold = inlier_threshold;
  a.rows = (int32_t*)b;
  a.summary_stride = 2;
  // round 1: the fit's inliers from the fit's model (the Huber fit)
  a.mask = b + L.o_mask;
  a.start = models_dev;
  a.start_stride = 12;
  a.poses = (double*)(b + L.o_pose1);
  a.info = nullptr;
  a.summaries = summaries_dev;
  a.inlier = b + L.o_in1;
  a.n_inliers = nullptr;
  GH_TRY(refine_launch(ctx, a));
  // round 2: the rows within `inlier_threshold` of round 1, from round 1's pose
  a.mask = b + L.o_in1;
  a.start = (const double*)(b + L.o_pose1);
  a.start_stride = 7;
  a.poses = poses_dev;
  a.info = info_dev;
  a.summaries = summaries_dev + 1;
  a.inlier = inlier_dev;
  a.n_inliers = n_inliers_dev;
  return refine_launch(ctx, a);
}

}  // namespace gh_ransac

extern "C" gh_status gh_pnp_batch_dev(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev,
                                      int nproblems, int nrows, double ransac_threshold, uint64_t seed, int dof,
                                      const gh_ba_options* options, int min_rows, double inlier_threshold, double* models_dev,
                                      int32_t* ransac_inliers_dev, double* poses_dev, double* info_dev,
                                      gh_pnp_batch_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, pnp_batch_args_ok(nproblems, nrows, ransac_threshold, min_rows, inlier_threshold));
  if (nproblems == 0) return GH_OK;
  GH_CHECK_ARG(ctx, xyz_dev && xy_dev && offsets_dev && models_dev && ransac_inliers_dev && poses_dev && summaries_dev);
  // ONE scratch block for all stages (gh_scratch hands out one block per context)
  void* base = nullptr;
  GH_TRY(gh_scratch(ctx, pnp_batch_scratch_bytes(nproblems, nrows), &base));
  return pnp_batch_on(ctx, xyz_dev, xy_dev, offsets_dev, nproblems, nrows, ransac_threshold, seed, dof, options, min_rows,
                      inlier_threshold, models_dev, ransac_inliers_dev, poses_dev, info_dev, summaries_dev, inlier_dev, n_inliers_dev,
                      base);
}
