// rocPRIM's radix sort and exclusive scans, instantiated once for the whole library: dev_prims.h.
#include "dev_prims.h"

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

// rocPRIM's kernels are templates on the iterator types as well: every caller goes through int32_t* / uint64_t* so that one
// kernel of each kind is instantiated (the inputs are only read).
hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const int32_t* key_in, int32_t* key_out, const int32_t* item_in, int32_t* item_out,
                      size_t n, int bits, hipStream_t stream) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, const_cast<int32_t*>(key_in), key_out, const_cast<int32_t*>(item_in), item_out, n, 0,
                                   bits, stream);
}

template <class T>
hipError_t scan(void* tmp, size_t& tmp_bytes, const T* in, T* out, size_t n, hipStream_t stream) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, const_cast<T*>(in), out, (T)0, n, rocprim::plus<T>(), stream);
}

size_t rounded(hipError_t e, size_t bytes) { return e == hipSuccess ? gh_round256(std::max(bytes, (size_t)1)) : 0; }

// the call between its profiling events, and the error text when it fails
template <class Call>
gh_status timed(gh_ctx* ctx, const char* label, const char* what, Call call) {
  const int prof = label ? gh_prof_begin(ctx, label) : -1;
  const hipError_t e = call();
  gh_prof_end(ctx, prof);
  return e == hipSuccess ? GH_OK : gh_set_error(ctx, GH_ERR_HIP, "%s", what);
}

}  // namespace

int gh_key_bits(int max_key) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) <= max_key) ++bits;
  return bits;
}

size_t gh_sort_pairs_bytes(gh_ctx* ctx, size_t n, int bits) {
  size_t bytes = 0;
  return rounded(sort_pairs(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n, bits, ctx->stream), bytes);
}

size_t gh_scan_u64_bytes(gh_ctx* ctx, size_t n) {
  size_t bytes = 0;
  return rounded(scan<uint64_t>(nullptr, bytes, nullptr, nullptr, n, ctx->stream), bytes);
}

size_t gh_scan_i32_bytes(gh_ctx* ctx, size_t n) {
  size_t bytes = 0;
  return rounded(scan<int32_t>(nullptr, bytes, nullptr, nullptr, n, ctx->stream), bytes);
}

gh_status gh_sort_pairs_i32(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const int32_t* key_in,
                            int32_t* key_out, const int32_t* item_in, int32_t* item_out, size_t n, int bits) {
  return timed(ctx, label, what, [&] { return sort_pairs(tmp, tmp_bytes, key_in, key_out, item_in, item_out, n, bits, ctx->stream); });
}

gh_status gh_scan_u64(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const uint64_t* in, uint64_t* out,
                      size_t n) {
  return timed(ctx, label, what, [&] { return scan<uint64_t>(tmp, tmp_bytes, in, out, n, ctx->stream); });
}

gh_status gh_scan_i32(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const int32_t* in, int32_t* out,
                      size_t n) {
  return timed(ctx, label, what, [&] { return scan<int32_t>(tmp, tmp_bytes, in, out, n, ctx->stream); });
}
