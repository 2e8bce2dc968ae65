// Index lists (CSR) of a large graph built on the GPU: items sorted by key, ascending item index inside a key -- what
// build_csr (ba.hip) does on the host with a counting sort.  For the 6 M observations of BASELINE configs[2] (C5) the host
// teams take ~60 ms per solve, a stable LSD radix sort of (key, item) pairs on the device ~1 ms plus the transfers.
// The sort and the scan are rocPRIM's, behind dev_prims.h (track_link.hip sorts and scans for itself: its keys have one hot bin,
// which the histogram below would serialise).
// gh_csr_index_dev is the device-side core (keys on the device in, start and list on the device out, work space passed in, nothing
// synchronised); gh_csr_build_dev wraps it for host arrays, tracks.hip calls it on the stream with context scratch.
#include <algorithm>
#include <cstring>

#include "dense_solve.h"
#include "dev_prims.h"

namespace {

__global__ __launch_bounds__(256) void csr_prepare_kernel(const int32_t* __restrict__ key, int n, int n_keys, int32_t* __restrict__ item,
                                                          int32_t* __restrict__ count, int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  item[i] = i;
  const int k = key[i];
  if (k < 0 || k >= n_keys) {
    *bad = 1;
    return;
  }
  atomicAdd(&count[k], 1);
}

// work space: key_out | item | item_out | count | start | bad flag | rocPRIM temporary storage, segments on 256-byte boundaries
struct CsrLayout {
  int bits;  // of the sort: the keys are 0 .. n_keys - 1
  size_t o_item, o_item_out, o_count, o_start, o_bad, o_tmp, tmp_bytes, total;
};

bool csr_layout(gh_ctx* ctx, int n_items, int n_keys, CsrLayout* L) {
  const size_t N = (size_t)n_items, K = (size_t)n_keys + 1;
  L->bits = gh_key_bits(n_keys - 1);
  const size_t sort_bytes = gh_sort_pairs_bytes(ctx, N, L->bits), scan_bytes = gh_scan_i32_bytes(ctx, K);
  if (!sort_bytes || !scan_bytes) return false;
  L->tmp_bytes = std::max(sort_bytes, scan_bytes);
  L->o_item = gh_round256(N * 4);
  L->o_item_out = L->o_item + gh_round256(N * 4);
  L->o_count = L->o_item_out + gh_round256(N * 4);
  L->o_start = L->o_count + gh_round256(K * 4);
  L->o_bad = L->o_start + gh_round256(K * 4);
  L->o_tmp = L->o_bad + 256;
  L->total = L->o_tmp + L->tmp_bytes;
  return true;
}

}  // namespace

size_t gh_csr_index_bytes(gh_ctx* ctx, int n_items, int n_keys) {
  CsrLayout L;
  if (n_items <= 0 || n_keys <= 0 || !csr_layout(ctx, n_items, n_keys, &L)) return 0;
  return L.total;
}

gh_status gh_csr_index_dev(gh_ctx* ctx, const int32_t* keys_dev, int n_items, int n_keys, void* work, size_t work_bytes,
                           const int32_t** start_dev, const int32_t** list_dev, const int** bad_dev) {
  CsrLayout L;
  if (n_items <= 0 || n_keys <= 0) return gh_set_error(ctx, GH_ERR_ARG, "gh_csr_index_dev: empty input");
  if (!csr_layout(ctx, n_items, n_keys, &L)) return gh_set_error(ctx, GH_ERR_HIP, "gh_csr_index_dev: rocPRIM size query failed");
  if (!work || work_bytes < L.total || ((uintptr_t)work & 255)) return gh_set_error(ctx, GH_ERR_ARG, "gh_csr_index_dev: work space");
  const size_t N = (size_t)n_items, K = (size_t)n_keys + 1;
  char* base = (char*)work;
  int32_t* d_key_out = (int32_t*)base;
  int32_t* d_item = (int32_t*)(base + L.o_item);
  int32_t* d_item_out = (int32_t*)(base + L.o_item_out);
  int32_t* d_count = (int32_t*)(base + L.o_count);
  int32_t* d_start = (int32_t*)(base + L.o_start);
  int* d_bad = (int*)(base + L.o_bad);
  void* d_tmp = base + L.o_tmp;
  if (hipMemsetAsync(d_count, 0, L.o_tmp - L.o_count, ctx->stream) != hipSuccess)  // count, start and the flag
    return gh_set_error(ctx, GH_ERR_HIP, "gh_csr_index_dev: memset");
  hipLaunchKernelGGL(csr_prepare_kernel, dim3(gh_div_up(n_items, 256)), dim3(256), 0, ctx->stream, keys_dev, n_items, n_keys, d_item,
                     d_count, d_bad);
  // (not timed one by one: the caller times the index as a whole)
  GH_TRY(gh_scan_i32(ctx, nullptr, "gh_csr_index_dev: scan", d_tmp, L.tmp_bytes, d_count, d_start, K));
  GH_TRY(gh_sort_pairs_i32(ctx, nullptr, "gh_csr_index_dev: sort", d_tmp, L.tmp_bytes, keys_dev, d_key_out, d_item, d_item_out, N, L.bits));
  *start_dev = d_start;
  *list_dev = d_item_out;
  if (bad_dev) *bad_dev = d_bad;
  return GH_OK;
}

gh_status gh_csr_build_dev(gh_ctx* ctx, const int32_t* keys_host, int n_items, int n_keys, int32_t* start_host, int32_t* list_host) {
  if (n_items <= 0 || n_keys <= 0) return gh_set_error(ctx, GH_ERR_ARG, "gh_csr_build_dev: empty input");
  const size_t N = (size_t)n_items, K = (size_t)n_keys + 1;
  const size_t index_bytes = gh_csr_index_bytes(ctx, n_items, n_keys);
  if (!index_bytes) return gh_set_error(ctx, GH_ERR_HIP, "gh_csr_build_dev: rocPRIM size query failed");
  char* base = nullptr;
  const size_t total = gh_round256(N * 4) + index_bytes;
  if (hipMalloc((void**)&base, total) != hipSuccess) return gh_set_error(ctx, GH_ERR_NOMEM, "gh_csr_build_dev: hipMalloc(%zu)", total);
  int32_t* d_key = (int32_t*)base;
  auto fail = [&](const char* what) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(base);
    return gh_set_error(ctx, GH_ERR_HIP, "gh_csr_build_dev: %s", what);
  };
  if (hipMemcpyAsync(d_key, keys_host, N * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("upload");
  const int32_t *d_start = nullptr, *d_list = nullptr;
  const int* d_bad = nullptr;
  if (gh_csr_index_dev(ctx, d_key, n_items, n_keys, base + gh_round256(N * 4), index_bytes, &d_start, &d_list, &d_bad) != GH_OK)
    return fail("index");
  int bad = 0;
  if (hipMemcpyAsync(list_host, d_list, N * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(start_host, d_start, K * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail("download");
  (void)hipFree(base);
  if (bad) return gh_set_error(ctx, GH_ERR_ARG, "gh_csr_build_dev: a key is outside [0, %d)", n_keys);
  return GH_OK;
}
