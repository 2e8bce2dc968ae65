// The internal header of the solver layer: the workspace of one dense solve (chol.hip) as ONE layout for every caller, the
// "state ready" protocol of its single-launch kernels, and the contracts of the functions the solver files call in each other.
// The layout part is plain host C++ (tools/dense_layout_check.cpp builds it with g++).
#pragma once
#include "common.h"

constexpr int kDenseNB = 64;   // columns of a diagonal block of the dense factorisation
constexpr int kFlowMaxT = 6;   // tiles per worker workgroup of the single-launch factorisation (chol.hip: FL_MAXT)
// bwd_chain_kernel's "not yet written": a NaN no computation produces, two equal 32-bit halves (so a 32-bit fill sets it)
constexpr unsigned kXSentinelWord = 0xFFF8BEEFu;
constexpr unsigned long long kXSentinel = ((unsigned long long)kXSentinelWord << 32) | kXSentinelWord;

// ---------------------------------------------------------------- workspace of one dense solve
// n unknowns, extra_rows in {0, 1} rows below the matrix (the right-hand side riding through the factorisation as row n).
struct DenseWork {
  int* info;             // 0 = ok; first bad block column + 1; > n: a hand-off wait of a single-launch kernel expired
  double* dinv;          // ceil(n / 64) * 4096: the inverted diagonal blocks (only the lower triangle of each is defined)
  double* work;          // n: running right-hand side of the launch-per-step substitutions
  double* xwork;         // 2 * 64 * (n + extra_rows): X rows of the one-launch panel steps, two buffers used in turn
  double* xh;            // ceil(n / 64) * 64: hand-off of the single-launch back-substitution; null = launch per step
  unsigned* flow_state;  // flags + hand-over tiles of the single-launch factorisation; null = shape not eligible / switched off
  unsigned n_flow_flag_words;  // u32 words at the start of flow_state that are ZERO when the launch starts
  unsigned n_xh_words;         // u32 words of xh that hold the sentinel when the launch starts
};

// Byte offsets from a 128-byte aligned base (in this order, every segment on a line of its own: the single-launch kernels
// touch a line with plain loads only in the one workgroup that owns it), and the sizes they were cut for.
struct DenseLayout {
  size_t info, dinv, work, xwork, xh, flow_state, bytes;
  size_t dinv_doubles, work_doubles, xwork_doubles, xh_doubles, flow_words;
  unsigned n_flow_flag_words, n_xh_words;
  int flow_workers;  // worker workgroups of the single-launch factorisation, -1 = the shape does not fit the GPU
};

// The dataflow launch needs every workgroup resident, one per CU (its LDS request admits no second one): the chain workgroup,
// an accumulator workgroup per tile row below the first, and the workers (ceil((i - 1) / kFlowMaxT) for tile row i >= 2).
inline DenseLayout dense_layout(int n, int extra_rows, int cu_count) {
  DenseLayout L{};
  const size_t nb = (size_t)gh_div_up(n, kDenseNB), ntr = (size_t)gh_div_up(n + extra_rows, kDenseNB);
  int workers = 0;
  for (int i = 2; i < (int)ntr; ++i) workers += gh_div_up(i - 1, kFlowMaxT);
  const int wgs = 1 + (ntr > 1 ? (int)ntr - 1 : 0) + workers;
  const bool fits = n >= 1 && extra_rows >= 0 && extra_rows <= 1 && wgs <= (cu_count > 0 ? cu_count : 256);
  L.flow_workers = fits ? workers : -1;
  L.dinv_doubles = nb * kDenseNB * kDenseNB;
  L.work_doubles = (size_t)n;
  L.xwork_doubles = 2 * (size_t)kDenseNB * (size_t)(n + extra_rows);
  L.xh_doubles = nb * kDenseNB;
  L.n_xh_words = (unsigned)(2 * L.xh_doubles);
  if (fits) {  // tile flags, block flags, hand-over flags, abort word; then the hand-over tiles (8192 doubles per tile row)
    L.n_flow_flag_words = (unsigned)((ntr * nb + nb + ntr + 16 + 31) & ~(size_t)31);
    L.flow_words = L.n_flow_flag_words + ntr * 8192 * 2;
  }
  size_t at = 0;
  auto segment = [&at](size_t bytes) { const size_t off = at; at += (bytes + 127) & ~(size_t)127; return off; };
  L.info = segment(sizeof(int));
  L.dinv = segment(L.dinv_doubles * sizeof(double));
  L.work = segment(L.work_doubles * sizeof(double));
  L.xwork = segment(L.xwork_doubles * sizeof(double));
  L.xh = segment(L.xh_doubles * sizeof(double));
  L.flow_state = segment(L.flow_words * sizeof(unsigned));
  L.bytes = at;
  return L;
}

inline DenseWork dense_carve(void* base, const DenseLayout& L) {
  char* p = static_cast<char*>(base);
  return DenseWork{reinterpret_cast<int*>(p + L.info),     reinterpret_cast<double*>(p + L.dinv),
                   reinterpret_cast<double*>(p + L.work),  reinterpret_cast<double*>(p + L.xwork),
                   reinterpret_cast<double*>(p + L.xh),    L.flow_words ? reinterpret_cast<unsigned*>(p + L.flow_state) : nullptr,
                   L.n_flow_flag_words,                    L.n_xh_words};
}

// ---------------------------------------------------------------- the ready protocol
// What the two single-launch kernels need before they start: info cleared, the flag words zero, the sentinel in every word of
// xh.  A caller whose previous kernel has spare workgroups lets them do it (dense_ready_word for i < words()) and passes
// `ready` = true to the two functions below: three memset nodes less in the stream.
struct DenseReady {
  unsigned* flow_flags;  // zero
  unsigned n_flow;
  unsigned* xh_words;    // the sentinel of bwd_chain_kernel in every 32-bit word
  unsigned n_xh;
  int* info;             // zero
  __host__ __device__ unsigned words() const { return n_flow > n_xh ? n_flow : n_xh; }
};
inline DenseReady dense_ready(const DenseWork& w) {
  return DenseReady{w.flow_state, w.flow_state ? w.n_flow_flag_words : 0u, reinterpret_cast<unsigned*>(w.xh),
                    w.xh ? w.n_xh_words : 0u, w.info};
}
__device__ __forceinline__ void dense_ready_word(const DenseReady& r, unsigned i) {
  if (i < r.n_flow) r.flow_flags[i] = 0u;
  if (i < r.n_xh) r.xh_words[i] = kXSentinelWord;
  if (i == 0 && r.info) *r.info = 0;
}

// ---------------------------------------------------------------- chol.hip
// Factor (lower, in place); asynchronous on the ctx stream.  `extra_rows` rows below the n x n matrix (lda >= n + extra_rows)
// ride along through trsm / syrk: with the right-hand side stored as row n, the factorisation leaves y = L^-1 b there (forward
// substitution for free).  w.xwork: full panel steps of the small-matrix regime run as one launch each (panel_step_kernel) with
// their X rows parked there until a later launch copies them home.  w.flow_state: when given (and GSLAM_HIP_CHOL_FLOW != 0, A
// and lda on 128-byte lines) the whole factorisation is the single dataflow launch (potrf_flow_kernel); `store_diag` = false lets
// it leave the diagonal blocks of L unwritten (a caller that only solves never reads them: the triangular solves use w.dinv).
// `ready`: the caller's previous kernel ran the ready protocol on `w`.
gh_status gh_potrf_dev_impl(gh_ctx* ctx, double* A, int n, int lda, int extra_rows, const DenseWork& w, bool store_diag, bool ready);
// Backward substitution only: y[i] = yv[i * ystride] on entry, x is written to b.  With w.xh (and w.info, n <= 8192 columns per
// launch, GSLAM_HIP_BWD_CHAIN != 0) one launch per 8192 columns; *w.info receives n + 1 + block if a hand-off wait expired.
gh_status gh_potrs_bwd_dev_impl(gh_ctx* ctx, const double* L, int n, int lda, const DenseWork& w, double* b, const double* yv,
                                long long ystride, bool ready);
// Two dataflow launches in flight on one GPU could each hold part of the CUs and wait for the rest for ever (until their
// bounded waits expire): callers in this process take this lock from the launch to their next stream synchronisation.
std::mutex& gh_potrf_flow_mutex(int device);

// ---------------------------------------------------------------- chol_cr.hip: band / arrowhead solver (block cyclic reduction)
// Tiles per superblock for a half-bandwidth of `hbw` scalars (A[r][c] = 0 for r - c > hbw), 0 = the band is too wide for
// this solver (or the matrix too small to gain from it): the caller stays on the dense factorisation.
int gh_cr_tiles(int n, int hbw);
size_t gh_cr_dinv_doubles(int n, int T);
size_t gh_cr_panel_doubles(int n, int T);  // workspace of the panels: W and G (two sides each), W3, yh
int gh_cr_top(int nbr);                    // superblocks the dense top takes (GSLAM_HIP_CR_TOP)
// border workspace of an arrowhead solve (doubles): the corner update's partial tiles, the dense system of the surviving
// superblocks + border and the DenseWork of its solve, the backward pass's t vector
size_t gh_arrow_ws_doubles(const gh_ctx* ctx, int n_band, int T, int nbr);
// Rows of a column of the COMPACT layout (cr_map.h) for this system as the solver will reduce it; *brow = local row of the first
// border row / of the right-hand side when there is no border.  Only systems solved WITH the border workspace (dense top).
int gh_cr_compact_lda(int n_band, int T, int nbr, int* brow);
// Arrowhead solve: A holds n_band + nbr unknowns (band first, border last; nbr = 0: a band) and the right-hand side in row
// n_band + nbr; the lower triangle of the band part must be ZERO outside the band (the fill lands there), the border rows are
// dense.  x_dev: n_band + nbr doubles.  *info_dev: 0 or the first column + 1 of a diagonal tile that is not positive definite.
// border_nz (device, may be null = E dense): the structure gh_cr_border_symbolic computed for this system, N * (nbs + ntr) bytes.
// allow_flow = false: the dense top stays off chol.hip's single-launch kernels (the caller saw one of their bounded waits expire:
// *info_dev > n_band + nbr).
gh_status gh_arrow_solve_dev_impl(gh_ctx* ctx, double* A, int n_band, int nbr, int lda, int T, double* dinv, double* W, double* bws,
                                  double* x_dev, int* info_dev, bool info_ready, bool allow_flow, const uint8_t* border_nz, bool compact);
// Structure of the border through the reduction (host, once per topology).  init[i * nbs + strip] != 0 iff the 16-row strip
// of the border rows has a structural non-zero among the band columns of superblock i (a border camera and a band camera that
// see a common point).  Eliminating i at level s fills the strips of i into i - s and i + s (E_u -= Y_i W_u^T); out receives
// nzY [N][nbs] -- the strips of E_i when i is eliminated, all set for the survivors of the dense top -- then nzT [N][ntr]: per
// 64-row tile of the corner, with the tile that holds the right-hand-side row (it rides along as row nbr) always set.
// Conservative by construction: a block marked zero is never written by any kernel and was cleared by the assembly.
size_t gh_cr_border_symbolic_bytes(int n_band, int T, int nbr);
void gh_cr_border_symbolic(int n_band, int T, int nbr, const uint8_t* init, uint8_t* out);

// ---------------------------------------------------------------- ba_order.hip, csr_sort.hip
// perm[new] = old camera (empty: the caller's order stands), returns the number of border cameras at the end of the order.
// *reordered (may be null): 1 when the bandwidth-reducing order was applied.  `allow_reorder` = false: rounds 4-5 (A/B runs).
// *band_span (may be null): the camera span of the order that results when this function has measured it (no camera border), else -1
// *border_points (may be null = never): filled when the long-range POINTS form the border (the return value is then 0)
int gh_ba_order_cameras(const gh_ba_problem* pr, std::vector<int32_t>& perm, int* reordered, bool allow_reorder, int* band_span,
                        std::vector<int32_t>* border_points);
// keys_host: n_items keys in [0, n_keys); start_host: n_keys + 1 offsets; list_host: n_items item indices, grouped by key in
// ascending key order, ascending inside a key.  Device memory comes from (and goes back to) hipMalloc: a setup-time call.
gh_status gh_csr_build_dev(gh_ctx* ctx, const int32_t* keys_host, int n_items, int n_keys, int32_t* start_host, int32_t* list_host);
// The device-side core of it, asynchronous on the context's stream: keys_dev as above but on the device (left unchanged);
// *start_dev / *list_dev point into `work` (256-byte aligned, at least gh_csr_index_bytes(ctx, n_items, n_keys) bytes; 0 = the
// size query failed), valid until the work space is reused.  *bad_dev (may be null): an int on the device, non-zero when a key
// was outside [0, n_keys) -- start and list are then unspecified.  No allocation, no synchronisation.
size_t gh_csr_index_bytes(gh_ctx* ctx, int n_items, int n_keys);
gh_status gh_csr_index_dev(gh_ctx* ctx, const int32_t* keys_dev, int n_items, int n_keys, void* work, size_t work_bytes,
                           const int32_t** start_dev, const int32_t** list_dev, const int** bad_dev);
