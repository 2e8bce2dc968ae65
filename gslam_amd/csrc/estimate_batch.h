// Plumbing of the estimator entries (ransac.hip, ransac_batch.hip, two_view.hip, pnp_batch.hip): the row range of a problem,
// the order-preserving compaction of a workgroup, the winner among the hypothesis counts, and the calls with which one file
// chains another's stage on its own scratch block.  The mathematics is ransac_models.h.
#pragma once
#include <limits.h>

#include "ransac_models.h"

namespace gh_ransac {

// Which rows of the arrays each problem owns.
struct RowRanges {
  const int32_t* row_begin;   // per problem: first row ...
  const int32_t* row_end;     // ... and one past the last
  const int32_t* limit_dev;   // rows the arrays hold as a device word (offsets[nproblems]), or NULL
  int limit;                  // rows the arrays hold as the host knows them; INT_MAX where only the device word says
};

// The row count of problem p, its first row in *first.  ONE rule for every kernel and every entry: a range that is empty,
// reversed, or not inside `limit` and (where given) *limit_dev is 0 rows, and nothing of it is addressed.
__device__ __forceinline__ int problem_rows(const RowRanges& r, int p, int* first) {
  int limit = r.limit;
  if (r.limit_dev && *r.limit_dev < limit) limit = *r.limit_dev;
  const int b = r.row_begin[p], e = r.row_end[p];
  *first = b;
  return (b < 0 || e > limit || e <= b) ? 0 : e - b;
}

// One trip of an order-preserving compaction by a 256-thread workgroup: the lanes with `take`, in thread order, get the
// slots *base, *base + 1, ...; a lane with `take` calls emit(slot), and *base moves past the trip.  Per-wave ballot and
// popcount prefix, the four wave totals through `wave_total` (4 ints of LDS).  Every lane makes every trip (whole-wave
// ballots, two barriers); afterwards `wave_total` is free again and what emit wrote is visible to the whole workgroup.
template <class Emit>
__device__ __forceinline__ void compact_trip(bool take, int* base, int* wave_total, Emit emit) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(take);
  if (lane == 0) wave_total[w] = __popcll(b);
  __syncthreads();
  int at = *base + __popcll(b & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) at += wave_total[k];
  if (take) emit(at);
  *base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
  __syncthreads();
}

// The winner among the kHyp counts of a problem (-1: not a regular hypothesis), by a 256-thread workgroup with `red`
// (256 long long of LDS).  Key = count << 32 | (kHyp - 1 - h), largest wins: the most inliers, then the lowest index.
// Every lane gets the key; < 0: no hypothesis is regular.
__device__ __forceinline__ long long winner_key(const int* counts, long long* red) {
  const int tid = threadIdx.x;
  long long key = -1;
  for (int h = tid; h < kHyp; h += 256)
    if (counts[h] >= 0) {
      const long long k = ((long long)counts[h] << 32) | (long long)(kHyp - 1 - h);
      key = k > key ? k : key;
    }
  red[tid] = key;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ int winner_index(long long key) { return kHyp - 1 - (int)(key & 0xFFFFFFFFll); }
__device__ __forceinline__ int winner_count(long long key) { return (int)(key >> 32); }

// What two_view_kernel works on (two_view.hip).  The batch entry addresses mask / good / points by row; the pair entry
// (ransac_batch.hip) hands it the compacted rows of its gather with row_map, and then mask / good / points are
// nproblems x map_stride, addressed by the query row of each compacted row.
struct TwoViewArgs {
  const double* E;            // problem p: 9 doubles at p * e_stride
  int e_stride;
  const double* src;
  const double* dst;
  RowRanges range;
  int nproblems;
  const uint8_t* mask;        // rows that take part, or NULL: all
  const int32_t* row_map;     // pair entry only
  int map_stride;
  gh_two_view_params prm;
  double* poses;
  double* points;
  uint8_t* good;
  int32_t* counts;
  int32_t* n_used;            // may be NULL
  int32_t* status;
};
bool two_view_params_ok(const gh_two_view_params* prm);
gh_status two_view_launch(gh_ctx* ctx, const TwoViewArgs& a);

// gh_ransac_batch_dev on a scratch block the caller owns (ransac_batch.hip), for entries that chain the batch with their
// own kernels on ONE context scratch block: ransac_batch_scratch_bytes(nproblems) bytes at `work`.
size_t ransac_batch_scratch_bytes(int nproblems);
gh_status ransac_batch_ranges(gh_ctx* ctx, int model, const double* src, const double* dst, const RowRanges& range,
                              int nproblems, double threshold, const double* thresholds, uint64_t seed, const uint64_t* seeds,
                              double* models, uint8_t* mask, int32_t* inliers, void* work);

// gh_pnp_batch_dev on a scratch block the caller owns (pnp_batch.hip), for localize.hip: pnp_batch_scratch_bytes(nproblems,
// nrows) bytes at `work`.  pnp_batch_args_ok is the entry's check of its scalars; the caller has checked the pointers.
bool pnp_batch_args_ok(int nproblems, int nrows, double ransac_threshold, int min_rows, double inlier_threshold);
size_t pnp_batch_scratch_bytes(int nproblems, int nrows);
gh_status pnp_batch_on(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev, int nproblems, int nrows,
                       double ransac_threshold, uint64_t seed, int dof, const gh_ba_options* options, int min_rows,
                       double inlier_threshold, double* models_dev, int32_t* ransac_inliers_dev, double* poses_dev, double* info_dev,
                       gh_pnp_batch_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, void* work);

}  // namespace gh_ransac
