// rocPRIM behind plain functions: the stable radix sort of (int32 key, int32 item) pairs and the exclusive scans that
// csr_sort.hip and the map stages use.  dev_prims.hip is the only translation unit that includes rocPRIM, so the library holds
// each of these device kernels once.  rocPRIM is plumbing here, like the runtime's memcpy.
//
// Every call runs on the context's stream with temporary storage that the caller carved from its scratch block.  `label` is the
// profiling label of the call (NULL: not timed, for a caller that is timed as a whole); `what` names the caller and the step,
// "<entry point>: <step>", and is the text of the error when rocPRIM refuses.
#pragma once
#include "common.h"

// bits of a radix sort whose keys are 0 .. max_key
int gh_key_bits(int max_key);

// Temporary storage in bytes: 0 when the size query fails, otherwise rounded up to 256 and at least 256.
size_t gh_sort_pairs_bytes(gh_ctx* ctx, size_t n, int bits);
size_t gh_scan_u64_bytes(gh_ctx* ctx, size_t n);
size_t gh_scan_i32_bytes(gh_ctx* ctx, size_t n);

// stable sort of n (key, item) pairs by the key bits 0 .. bits - 1
gh_status gh_sort_pairs_i32(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const int32_t* key_in,
                            int32_t* key_out, const int32_t* item_in, int32_t* item_out, size_t n, int bits);
// out[i] = in[0] + ... + in[i - 1], out[0] = 0
gh_status gh_scan_u64(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const uint64_t* in, uint64_t* out,
                      size_t n);
gh_status gh_scan_i32(gh_ctx* ctx, const char* label, const char* what, void* tmp, size_t tmp_bytes, const int32_t* in, int32_t* out,
                      size_t n);
