// The host-side pieces that the map stages share, beside the device-side ones of map_dev.h: the index over a stage's keys
// (gh_triangulate_tracks_dev, gh_describe_points_dev, gh_search_projection_dev), the number of spare bins, the scale table and the
// alignment the descriptor words need.
#pragma once
#include <cstdint>

#include "dense_solve.h"
#include "map_dev.h"

namespace gh_map {

// how many spare bins follow n_real_keys real ones (map_dev.h: THE SPARE BINS): kSpareBins, or one where the key range of an
// int32 has no room for them
inline int spare_bins(long long n_real_keys) { return n_real_keys <= (long long)INT32_MAX - 1 - kSpareBins ? kSpareBins : 1; }

// by repeated multiplication, not pow(): the bits of what a kernel computes from the table depend on how it was built
inline ScalePowers scale_powers(double scale_factor) {
  ScalePowers pw;
  pw.v[0] = 1.0;
  for (int l = 1; l < kMaxLevels; ++l) pw.v[l] = pw.v[l - 1] * scale_factor;
  return pw;
}

// descriptors move as 32-bit words
inline bool word_aligned(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 3) == 0; }

// KEYS TO INDEX, in two steps around the stage's own scratch block.  index_bytes: the bytes of work space that the index of
// n_items keys in [0, n_keys) needs; without items only an all-zero start of n_keys + 1 entries.
inline gh_status index_bytes(gh_ctx* ctx, const char* entry, int n_items, int n_keys, size_t* bytes) {
  *bytes = gh_round256(((size_t)n_keys + 1) * 4);
  if (n_items > 0) {
    *bytes = gh_csr_index_bytes(ctx, n_items, n_keys);
    if (!*bytes) return gh_set_error(ctx, GH_ERR_HIP, "%s: rocPRIM size query failed", entry);
  }
  return GH_OK;
}

// build_index: start / list of the keys (gh_csr_index_dev, timed under `label`) in `work`, 256-byte aligned and index_bytes(..)
// long; without items the zeroed start and no list.  The keys are read only when there are items.
inline gh_status build_index(gh_ctx* ctx, const char* label, const int32_t* keys, int n_items, int n_keys, void* work,
                             size_t work_bytes, const int32_t** start, const int32_t** list) {
  if (n_items == 0) {
    GH_HIP(ctx, hipMemsetAsync(work, 0, work_bytes, ctx->stream));
    *start = (const int32_t*)work;
    *list = nullptr;
    return GH_OK;
  }
  const int prof = gh_prof_begin(ctx, label);
  const gh_status st = gh_csr_index_dev(ctx, keys, n_items, n_keys, work, work_bytes, start, list, nullptr);
  gh_prof_end(ctx, prof);
  return st;
}

}  // namespace gh_map
