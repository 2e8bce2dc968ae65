// RANSAC model estimation with inlier masks on gfx950 — SURVEY.md 8 f3, the step right after matching.
//
// Fills in behind GSLAM::Estimator (GSLAM/core/Estimator.h:92-169: findHomography / findAffine2D / findFundamental /
// findAffine3D with `std::vector<uchar>* mask`).  The reference ships the INTERFACE only (the estimator plugin is
// commented out of the build, CMakeLists.txt:45), so the algorithm is specified here and restated in
// oracle/ransac_oracle.c; GPU and oracle agree bit for bit (models and masks):
//   * a fixed budget of 2048 hypotheses; hypothesis h draws its minimal sample with splitmix64(seed, h) (duplicates
//     rejected), solves the minimal problem in f64 by Gaussian elimination (no library calls, no FMA contraction),
//   * every hypothesis is scored against all N correspondences (squared error <= threshold^2), integer inlier counts,
//   * winner = most inliers, lowest hypothesis index on ties; its model and inlier mask are returned.
//   * no model = 0 inliers, model all zero, mask all zero: fewer rows than the sample, no regular hypothesis, an LMedS
//     median that is undefined, a NOSAMPLE fit that is singular or not finite (NaN / Inf input: the eigenvector fits never
//     refuse by themselves), or (E) a winner whose projection onto the essential manifold fails.
// Models: H (4 pairs, 8x8 system, h33 = 1, forward transfer error), A2 (3 pairs, 2x3 affine), F (8 pairs, Hartley-
// normalised 8x9 nullspace by full pivoting, Sampson error; rank 2 is not enforced), A3 (4 pairs, 3x4 affine, 3D).
// CDNA4 mapping: one lane per hypothesis for the tiny dense solves, one workgroup per hypothesis for scoring
// (coalesced point reads, integer block reduction), everything in one stream; the work is small and latency-bound.
#include "estimate_batch.h"

namespace {

using namespace gh_ransac;

__global__ __launch_bounds__(64) void ransac_solve_kernel(int model, const double* __restrict__ p,
                                                          const double* __restrict__ q, int n, uint64_t seed, Norm nm,
                                                          double* __restrict__ models, int* __restrict__ valid) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= kHyp) return;
  valid[h] = solve_hypothesis(model, p, q, n, seed, nm, h, models + (size_t)h * 12) ? 1 : 0;
}

__global__ __launch_bounds__(256) void ransac_score_kernel(int model, const double* __restrict__ p,
                                                           const double* __restrict__ q, int n, double thr2,
                                                           const double* __restrict__ models,
                                                           const int* __restrict__ valid, int* __restrict__ counts) {
  __shared__ int red[256];
  const int h = blockIdx.x;
  int c = 0;
  if (valid[h]) {
    double m[12];
    const int ms = model_size(model);
    for (int k = 0; k < ms; ++k) m[k] = models[(size_t)h * 12 + k];
    for (int i = threadIdx.x; i < n; i += 256) {
      double e;
      if (model_error(model, m, p, q, i, &e) && e <= thr2) ++c;
    }
  }
  red[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[h] = valid[h] ? red[0] : -1;
}

__global__ __launch_bounds__(256) void ransac_best_kernel(const int* __restrict__ counts, int* __restrict__ best) {
  __shared__ long long red[256];
  const long long key = winner_key(counts, red);
  if (threadIdx.x == 0) {
    best[0] = key < 0 ? -1 : winner_index(key);
    best[1] = key < 0 ? 0 : winner_count(key);
  }
}

__global__ __launch_bounds__(256) void ransac_mask_kernel(int model, const double* __restrict__ p,
                                                          const double* __restrict__ q, int n, double thr2,
                                                          const double* __restrict__ models,
                                                          const int* __restrict__ best, uint8_t* __restrict__ mask,
                                                          double* __restrict__ model_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int h = best[0];
  if (h < 0) {
    if (i < n) mask[i] = 0;
    return;
  }
  double m[12];
  const int ms = model_size(model);
  for (int k = 0; k < ms; ++k) m[k] = models[(size_t)h * 12 + k];
  if (i < 12) model_out[i] = i < ms ? m[i] : 0.0;
  if (i < n) {
    double e;
    mask[i] = (model_error(model, m, p, q, i, &e) && e <= thr2) ? 1 : 0;
  }
}

// LMedS score of a hypothesis: the element of rank n / 2 (ascending, 0-based) of its squared errors; a correspondence whose
// error is undefined counts as +inf.  Squared errors are non-negative doubles, whose bit patterns order as the values do:
// an exact radix select, 8 bits per pass, one workgroup per hypothesis (the errors are recomputed in every pass: ~50 flops each).
__global__ __launch_bounds__(256) void ransac_median_kernel(int model, const double* __restrict__ p,
                                                            const double* __restrict__ q, int n,
                                                            const double* __restrict__ models,
                                                            const int* __restrict__ valid,
                                                            unsigned long long* __restrict__ med) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_rank;
  const int h = blockIdx.x, tid = threadIdx.x;
  if (!valid[h]) {
    if (tid == 0) med[h] = ~0ull;
    return;
  }
  double m[12];
  const int ms = model_size(model);
  for (int k = 0; k < ms; ++k) m[k] = models[(size_t)h * 12 + k];
  unsigned long long prefix = 0ull;
  unsigned rank = (unsigned)(n / 2);
  for (int pass = 7; pass >= 0; --pass) {
    hist[tid] = 0u;
    __syncthreads();
    const unsigned long long hi_mask = pass == 7 ? 0ull : (~0ull << (8 * (pass + 1)));
    for (int i = tid; i < n; i += 256) {
      double e;
      // (`e == e` states the rule "a NaN error counts as +inf" and matches the oracle line for line; it changes no result:
      // errors carry no sign, so a NaN's bits are a key above 0x7FF0... as +inf's are, and the host refuses both alike)
      const unsigned long long b = (model_error(model, m, p, q, i, &e) && e == e) ? (unsigned long long)__double_as_longlong(e)
                                                                                 : 0x7FF0000000000000ull;
      if ((b & hi_mask) == prefix) atomicAdd(&hist[(unsigned)(b >> (8 * pass)) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned acc = 0u;
      int d = 0;
      for (; d < 255; ++d) {
        if (acc + hist[d] > rank) break;
        acc += hist[d];
      }
      s_prefix = prefix | ((unsigned long long)d << (8 * pass));
      s_rank = rank - acc;
    }
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    __syncthreads();
  }
  if (tid == 0) med[h] = prefix;
}

// NOSAMPLE (GSLAM/core/Estimator.h:89): the model from ALL correspondences, no hypotheses -- the algebraic least-squares
// counterpart of each minimal solver, sums taken sequentially in index order (host side: n x a few dozen flops; the oracle
// adds in the same order).  H, A2, A3: normal equations of the minimal solver's rows, Gaussian elimination.  F / E, PnP:
// eigenvector of the smallest eigenvalue of A^T A (cyclic Jacobi), then the minimal solver's own post-processing.  SIM3:
// Horn's closed form over all pairs.  Plane: normal = eigenvector of the smallest eigenvalue of the covariance.
template <int N>
static int smallest_eig_vector(double (*A)[N], double* vec) {
  double V[N][N];
  jacobi_eig<N>(A, V);
  int best = 0;
  for (int k = 1; k < N; ++k)
    if (A[k][k] < A[best][best]) best = k;
  for (int k = 0; k < N; ++k) vec[k] = V[k][best];
  return best;
}

static bool fit_all(int model, const double* p, const double* q, int n, const Norm& nm, double* out) {
  for (int k = 0; k < 12; ++k) out[k] = 0.0;
  if (model == kModelH || model == kModelA2 || model == kModelA3) {
    const int nu = model == kModelH ? 8 : (model == kModelA2 ? 3 : 4), nr = model == kModelH ? 1 : (model == kModelA2 ? 2 : 3);
    double N[8][12];
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 12; ++c) N[r][c] = 0.0;
    auto add_row = [&](const double* r) {
      for (int a = 0; a < nu; ++a)
        for (int b = 0; b < nu + nr; ++b) N[a][b] = N[a][b] + r[a] * r[b];
    };
    for (int i = 0; i < n; ++i) {
      if (model == kModelH) {
        const double x = p[2 * i], y = p[2 * i + 1], u = q[2 * i], v = q[2 * i + 1];
        const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
        add_row(r0);
        add_row(r1);
      } else if (model == kModelA2) {
        const double r[5] = {p[2 * i], p[2 * i + 1], 1, q[2 * i], q[2 * i + 1]};
        add_row(r);
      } else {
        const double r[7] = {p[3 * i], p[3 * i + 1], p[3 * i + 2], 1, q[3 * i], q[3 * i + 1], q[3 * i + 2]};
        add_row(r);
      }
    }
    if (!ge_solve(N, nu, nr)) return false;
    if (model == kModelH) {
      for (int k = 0; k < 8; ++k) out[k] = N[k][8];
      out[8] = 1.0;
    } else if (model == kModelA2) {
      for (int k = 0; k < 3; ++k) {
        out[k] = N[k][3];
        out[3 + k] = N[k][4];
      }
    } else {
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = N[c][4 + r];
    }
    return true;
  }
  if (model == kModelSim3) return solve_sim3(p, q, nullptr, out, n);
  if (model == kModelPlane) {
    double c[3] = {0, 0, 0}, C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, nv[3];
    for (int i = 0; i < n; ++i)
      for (int e = 0; e < 3; ++e) c[e] = c[e] + p[3 * i + e];
    for (int e = 0; e < 3; ++e) c[e] = c[e] / (double)n;
    for (int i = 0; i < n; ++i) {
      const double d[3] = {p[3 * i] - c[0], p[3 * i + 1] - c[1], p[3 * i + 2] - c[2]};
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[a][b] = C[a][b] + d[a] * d[b];
    }
    smallest_eig_vector<3>(C, nv);
    const double len = sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
    if (!(len > kTiny)) return false;
    for (int e = 0; e < 3; ++e) out[e] = nv[e] / len;
    out[3] = -(out[0] * c[0] + out[1] * c[1] + out[2] * c[2]);
    return true;
  }
  if (model == kModelPnP) {
    double A[12][12];
    for (int r = 0; r < 12; ++r)
      for (int c = 0; c < 12; ++c) A[r][c] = 0.0;
    for (int i = 0; i < n; ++i) {
      const double X = p[3 * i], Y = p[3 * i + 1], Z = p[3 * i + 2], u = q[2 * i], v = q[2 * i + 1];
      const double r0[12] = {X, Y, Z, 1, 0, 0, 0, 0, -u * X, -u * Y, -u * Z, -u}, r1[12] = {0, 0, 0, 0, X, Y, Z, 1, -v * X, -v * Y, -v * Z, -v};
      for (int a = 0; a < 12; ++a)
        for (int b = 0; b < 12; ++b) A[a][b] = A[a][b] + (r0[a] * r0[b] + r1[a] * r1[b]);
    }
    double P[12];
    smallest_eig_vector<12>(A, P);
    return pnp_from_projection(P, p, out);
  }
  // fundamental / essential
  double A[9][9];
  for (int r = 0; r < 9; ++r)
    for (int c = 0; c < 9; ++c) A[r][c] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = (p[2 * i] - nm.m1x) * nm.s1, y = (p[2 * i + 1] - nm.m1y) * nm.s1;
    const double u = (q[2 * i] - nm.m2x) * nm.s2, v = (q[2 * i + 1] - nm.m2y) * nm.s2;
    const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1};
    for (int a = 0; a < 9; ++a)
      for (int b = 0; b < 9; ++b) A[a][b] = A[a][b] + r[a] * r[b];
  }
  double fh[9];
  smallest_eig_vector<9>(A, fh);
  const double T1[9] = {nm.s1, 0, -nm.s1 * nm.m1x, 0, nm.s1, -nm.s1 * nm.m1y, 0, 0, 1};
  const double T2[9] = {nm.s2, 0, -nm.s2 * nm.m2x, 0, nm.s2, -nm.s2 * nm.m2y, 0, 0, 1};
  double tmp[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + fh[3 * r + k] * T1[3 * k + c];
      tmp[3 * r + c] = acc;
    }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + T2[3 * k + r] * tmp[3 * k + c];
      out[3 * r + c] = acc;
    }
  return true;
}

}  // namespace

// The adaptive stopping rule of sequential RANSAC (Fischler & Bolles; the rule behind a `confidence` argument): walking the
// hypotheses in index order, after every strict improvement of the best inlier count c the number of hypotheses needed is
// N = ceil(log(1 - confidence) / log(1 - (c / n)^s)), and the walk stops once h + 1 >= N.  All kHyp hypotheses are scored
// in parallel anyway; the rule only decides WHICH prefix of them a sequential run would have looked at, so the result is
// the one a CPU implementation with the same draws returns.  Evaluated on the host with libm (the oracle makes the same
// calls), never on the device.  confidence outside (0, 1): every hypothesis counts.
static int adaptive_prefix_best(const int* counts, int n, int s, double confidence, int* best_count, int* used) {
  int best_h = -1, best_c = -1, limit = kHyp;
  const bool adaptive = confidence > 0.0 && confidence < 1.0;
  int h = 0;
  for (; h < limit; ++h) {
    if (counts[h] > best_c) {
      best_c = counts[h];
      best_h = h;
      if (adaptive && best_c > 0) {
        const double pg = pow((double)best_c / (double)n, (double)s);
        int need = kHyp;
        if (pg >= 1.0) need = h + 1;
        else if (pg > 0.0) {
          const double v = ceil(log(1.0 - confidence) / log(1.0 - pg));
          need = v < 1.0 ? 1 : (v > (double)kHyp ? kHyp : (int)v);
        }
        if (need < limit) limit = need < h + 1 ? h + 1 : need;
      }
    }
  }
  *best_count = best_c < 0 ? 0 : best_c;
  *used = h;
  return best_c < 0 ? -1 : best_h;
}

extern "C" gh_status gh_ransac_estimate(gh_ctx* ctx, int model, const double* src, const double* dst, int n,
                                        double threshold, uint64_t seed, double* model_out, uint8_t* mask_out,
                                        int* inliers_out) {
  return gh_ransac_estimate_conf(ctx, model, src, dst, n, threshold, 1.0, seed, model_out, mask_out, inliers_out, nullptr);
}

extern "C" gh_status gh_ransac_estimate_conf(gh_ctx* ctx, int model, const double* src, const double* dst, int n,
                                             double threshold, double confidence, uint64_t seed, double* model_out,
                                             uint8_t* mask_out, int* inliers_out, int* hypotheses_used_out) {
  return gh_ransac_estimate_ex(ctx, model, src, dst, n, threshold, confidence, seed, GH_SAMPLE_RANSAC, model_out, mask_out,
                               inliers_out, hypotheses_used_out);
}

namespace {

// The device scratch of one gh_ransac_estimate_ex call: p | q | models | valid | counts | best | model | mask.  The pinned
// host block mirrors it offset for offset, so that every phase moves its data with one DMA per direction.
struct EstimateLayout {
  // (p is at 0; q: sized for the wider of the two point sets; counts: 8 bytes per hypothesis, LMedS stores its medians there
  // as 64-bit keys; best | model | mask lie back to back: one download)
  size_t q, models, valid, counts, best, mout, mask, total;
  explicit EstimateLayout(int n)
      : q(gh_round256((size_t)n * 3 * 8)), models(2 * q), valid(models + (size_t)kHyp * 12 * 8), counts(valid + kHyp * 4),
        best(counts + kHyp * 8), mout(best + 256), mask(mout + 256), total(mask + gh_round256((size_t)n)) {}
};

// One call on its way through the phases below.
struct EstimateRun {
  int model, n, s;
  double threshold, thr2;   // thr2: the squared inlier radius of the mask (LMedS replaces it with its own)
  uint64_t seed;
  Norm nm;
  EstimateLayout at;
  uint8_t *b, *hb;          // the device block and its pinned mirror
  int best[2];              // the winner as the host knows it: hypothesis (-1: none), inlier count
  int used;                 // hypotheses looked at: what hypotheses_used_out reports
  bool count_from_mask;     // the inlier count is the population of the mask (no device count: NOSAMPLE, LMedS)
  double* p() const { return (double*)b; }
  double* q() const { return (double*)(b + at.q); }
  double* models() const { return (double*)(b + at.models); }
  int* valid() const { return (int*)(b + at.valid); }
  int* counts() const { return (int*)(b + at.counts); }
  int* d_best() const { return (int*)(b + at.best); }
};

// Both point sets to the device through the pinned mirror.
// (a per-frame caller -- Estimator::findFundamental / findHomography / findPnPRansac -- paid two pageable uploads and
// three to five pageable downloads of ~30-50 us each around ~100 us of kernels)
gh_status estimate_upload_points(gh_ctx* ctx, const EstimateRun& R, const double* src, const double* dst) {
  const size_t qbytes = (size_t)R.n * dim_q(R.model) * 8;
  memcpy(R.hb, src, (size_t)R.n * dim_p(R.model) * 8);
  memcpy(R.hb + R.at.q, dst, qbytes);
  GH_HIP(ctx, hipMemcpyAsync(R.b, R.hb, R.at.q + qbytes, hipMemcpyHostToDevice, ctx->stream));
  return GH_OK;
}

// The host's choice of the winner (two ints) to the device; the download at the end into the same words of the pinned mirror
// is ordered behind it by the stream.
gh_status estimate_send_best(gh_ctx* ctx, const EstimateRun& R) {
  memcpy(R.hb + R.at.best, R.best, 8);
  GH_HIP(ctx, hipMemcpyAsync(R.d_best(), R.hb + R.at.best, 8, hipMemcpyHostToDevice, ctx->stream));
  return GH_OK;
}

// NOSAMPLE: the all-point fit is hypothesis 0; the device evaluates it against every correspondence (mask + inlier count).
// *have = false: a degenerate fit, the outputs stay as they were cleared.
gh_status estimate_choose_fit_all(gh_ctx* ctx, EstimateRun& R, const double* src, const double* dst, bool* have) {
  double m[12];
  // (the eigenvector fits never refuse; on NaN / Inf input they hand back a model that is not finite, whose NaN payloads
  // are the compiler's choice of operand order: such a fit is no model)
  bool ok = fit_all(R.model, src, dst, R.n, R.nm, m);
  for (int k = 0; k < 12; ++k) ok = ok && fabs(m[k]) <= 1.7976931348623157e308;
  R.used = ok ? 1 : 0;
  R.count_from_mask = true;
  *have = ok;
  if (!ok) {  // the upload from the pinned block must not outlive the call
    GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GH_OK;
  }
  memcpy(R.hb + R.at.models, m, sizeof(m));
  GH_HIP(ctx, hipMemcpyAsync(R.models(), R.hb + R.at.models, sizeof(m), hipMemcpyHostToDevice, ctx->stream));
  R.best[0] = 0;
  return estimate_send_best(ctx, R);
}

// Least median of squares (Rousseeuw; OpenCV's LMEDS): the hypothesis with the smallest median squared error wins
// (lowest index on ties); inlier radius = max(threshold, 2.5 * 1.4826 * (1 + 5 / (n - s)) * sqrt(median)).
// *have = false: no hypothesis explains half of the correspondences.
gh_status estimate_choose_lmeds(gh_ctx* ctx, EstimateRun& R, bool* have) {
  GH_LAUNCH(ctx, "ransac_solve", ransac_solve_kernel, dim3(kHyp / 64), dim3(64), 0, R.model, R.p(), R.q(), R.n, R.seed, R.nm,
            R.models(), R.valid());
  unsigned long long* d_med = (unsigned long long*)R.counts();
  GH_LAUNCH(ctx, "ransac_median", ransac_median_kernel, dim3(kHyp), dim3(256), 0, R.model, R.p(), R.q(), R.n, R.models(), R.valid(),
            d_med);
  const unsigned long long* h_med = (const unsigned long long*)(R.hb + R.at.counts);
  GH_HIP(ctx, hipMemcpyAsync(R.hb + R.at.counts, d_med, kHyp * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long bm = ~0ull;
  for (int h = 0; h < kHyp; ++h)
    if (h_med[h] < bm) {
      bm = h_med[h];
      R.best[0] = h;
    }
  R.used = kHyp;
  R.count_from_mask = true;
  *have = R.best[0] >= 0 && bm < 0x7FF0000000000000ull;
  if (!*have) return GH_OK;
  double med;
  memcpy(&med, &bm, 8);
  const double sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (double)(R.n - R.s > 0 ? R.n - R.s : 1)) * sqrt(med);
  const double radius = sigma > R.threshold ? sigma : R.threshold;
  R.thr2 = radius * radius;
  return estimate_send_best(ctx, R);
}

// RANSAC: every hypothesis scored on the device; the winner by the adaptive prefix rule on the host (confidence inside
// (0, 1)) or by the device's argmax.  Either way the device holds winner and count afterwards ("none" included).
gh_status estimate_choose_ransac(gh_ctx* ctx, EstimateRun& R, double confidence) {
  GH_LAUNCH(ctx, "ransac_solve", ransac_solve_kernel, dim3(kHyp / 64), dim3(64), 0, R.model, R.p(), R.q(), R.n, R.seed, R.nm,
            R.models(), R.valid());
  GH_LAUNCH(ctx, "ransac_score", ransac_score_kernel, dim3(kHyp), dim3(256), 0, R.model, R.p(), R.q(), R.n, R.thr2, R.models(),
            R.valid(), R.counts());
  R.count_from_mask = false;
  if (confidence > 0.0 && confidence < 1.0) {
    // the prefix rule needs the counts on the host: 8 KB back, the choice forth
    const int* h_counts = (const int*)(R.hb + R.at.counts);
    GH_HIP(ctx, hipMemcpyAsync(R.hb + R.at.counts, R.counts(), kHyp * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    R.best[0] = adaptive_prefix_best(h_counts, R.n, R.s, confidence, &R.best[1], &R.used);
    return estimate_send_best(ctx, R);
  }
  GH_LAUNCH(ctx, "ransac_best", ransac_best_kernel, dim3(1), dim3(256), 0, R.counts(), R.d_best());
  R.used = kHyp;
  return GH_OK;
}

// The winner's mask and model on the device, ONE download, and the outputs.  No winner: the cleared outputs stay.
gh_status estimate_finish(gh_ctx* ctx, EstimateRun& R, double* model_out, uint8_t* mask_out, int* inliers_out) {
  const int n = R.n;
  const EstimateLayout& at = R.at;
  GH_LAUNCH(ctx, "ransac_mask", ransac_mask_kernel, dim3(gh_div_up(n > 12 ? n : 12, 256)), dim3(256), 0, R.model, R.p(), R.q(), n,
            R.thr2, R.models(), R.d_best(), R.b + at.mask, (double*)(R.b + at.mout));
  GH_HIP(ctx, hipMemcpyAsync(R.hb + at.best, R.d_best(), (at.mask - at.best) + ((mask_out || R.count_from_mask) ? (size_t)n : 0),
                             hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!R.count_from_mask) memcpy(R.best, R.hb + at.best, 8);
  memcpy(model_out, R.hb + at.mout, 12 * 8);
  if (mask_out) memcpy(mask_out, R.hb + at.mask, (size_t)n);
  if (R.best[0] < 0) {
    for (int k = 0; k < 12; ++k) model_out[k] = 0.0;
    return GH_OK;
  }
  if (R.count_from_mask) {
    R.best[1] = 0;
    const uint8_t* hm = R.hb + at.mask;
    for (int i = 0; i < n; ++i) R.best[1] += hm[i] ? 1 : 0;
  }
  *inliers_out = R.best[1];
  if (R.model == kModelE && !project_essential(model_out)) {
    // the scored 8-point estimate has no essential matrix near it (rank 1, or not finite): no model, and like every
    // other no-model exit neither an inlier count nor a mask (the one copied out above belonged to the rejected estimate)
    for (int k = 0; k < 12; ++k) model_out[k] = 0.0;
    if (mask_out)
      for (int i = 0; i < n; ++i) mask_out[i] = 0;
    *inliers_out = 0;
  }
  return GH_OK;
}

}  // namespace

extern "C" gh_status gh_ransac_estimate_ex(gh_ctx* ctx, int model, const double* src, const double* dst, int n,
                                           double threshold, double confidence, uint64_t seed, int sampling, double* model_out,
                                           uint8_t* mask_out, int* inliers_out, int* hypotheses_used_out) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, model >= 0 && model <= 7 && src && dst && model_out && inliers_out && threshold >= 0);
  GH_CHECK_ARG(ctx, sampling == GH_SAMPLE_RANSAC || sampling == GH_SAMPLE_LMEDS || sampling == GH_SAMPLE_NONE);
  *inliers_out = 0;
  if (hypotheses_used_out) *hypotheses_used_out = 0;
  for (int k = 0; k < 12; ++k) model_out[k] = 0.0;
  if (mask_out)
    for (int i = 0; i < n; ++i) mask_out[i] = 0;
  if (n < sample_size(model)) return GH_OK;  // not enough correspondences: no model (inliers 0)
  GH_HIP(ctx, hipSetDevice(ctx->device));
  EstimateRun R = {model, n, sample_size(model), threshold, threshold * threshold, seed, {0, 0, 1, 0, 0, 1}, EstimateLayout(n)};
  if (model == kModelF || model == kModelE) R.nm = hartley_norm(src, dst, n);
  R.best[0] = -1;
  void *base = nullptr, *hbase = nullptr;
  GH_TRY(gh_scratch(ctx, R.at.total, &base));
  GH_TRY(gh_pinned(ctx, R.at.total, &hbase));
  R.b = (uint8_t*)base;
  R.hb = (uint8_t*)hbase;
  GH_TRY(estimate_upload_points(ctx, R, src, dst));
  bool have = true;
  if (sampling == GH_SAMPLE_NONE) GH_TRY(estimate_choose_fit_all(ctx, R, src, dst, &have));
  else if (sampling == GH_SAMPLE_LMEDS) GH_TRY(estimate_choose_lmeds(ctx, R, &have));
  else GH_TRY(estimate_choose_ransac(ctx, R, confidence));
  if (hypotheses_used_out) *hypotheses_used_out = R.used;
  if (!have) return GH_OK;
  return estimate_finish(ctx, R, model_out, mask_out, inliers_out);
}

namespace {

// Midpoint triangulation of one correspondence per thread (GSLAM::Estimator::trianglate, Estimator.h:164-168): the point
// of the REFERENCE frame closest to both rays, X_cur = R X_ref + t.  ok = 0 when the rays are parallel or the point lies
// behind either camera.
__global__ __launch_bounds__(256) void triangulate_kernel(const double* __restrict__ pose, int pose_stride,
                                                          const double* __restrict__ dref, const double* __restrict__ dcur,
                                                          int n, double* __restrict__ out, uint8_t* __restrict__ ok) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* T = pose + (size_t)i * pose_stride;  // [qx qy qz qw tx ty tz], ref -> cur
  const double qx = T[0], qy = T[1], qz = T[2], qw = T[3];
  const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                       2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                       2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)};
  const double* d1 = dref + 3 * (size_t)i;
  const double* b = dcur + 3 * (size_t)i;
  double a[3];
  for (int r = 0; r < 3; ++r) a[r] = R[3 * r] * d1[0] + R[3 * r + 1] * d1[1] + R[3 * r + 2] * d1[2];
  const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double at = a[0] * T[4] + a[1] * T[5] + a[2] * T[6], bt = b[0] * T[4] + b[1] * T[5] + b[2] * T[6];
  const double det = aa * bb - ab * ab;
  bool good = det > 1e-12 * aa * bb;
  double l1 = 0.0, l2 = 0.0;
  if (good) {
    l1 = (ab * bt - bb * at) / det;  // min |l1 a + t - l2 b|^2
    l2 = (aa * bt - ab * at) / det;
    good = l1 > 0.0 && l2 > 0.0;
  }
  double xr[3] = {0, 0, 0};
  if (good) {
    double mc[3];
    for (int r = 0; r < 3; ++r) mc[r] = ((l1 * a[r] + T[4 + r]) + l2 * b[r]) / 2.0 - T[4 + r];  // midpoint - t, cur frame
    for (int r = 0; r < 3; ++r) xr[r] = R[r] * mc[0] + R[3 + r] * mc[1] + R[6 + r] * mc[2];      // R^T (.)
  }
  for (int r = 0; r < 3; ++r) out[3 * (size_t)i + r] = xr[r];
  ok[i] = good ? 1 : 0;
}

}  // namespace

extern "C" gh_status gh_triangulate(gh_ctx* ctx, const double* ref2cur_pose, int pose_stride, const double* ref_dir,
                                    const double* cur_dir, int n, double* ref_points, uint8_t* ok) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n >= 0 && (pose_stride == 0 || pose_stride == 7));
  if (n == 0) return GH_OK;
  GH_CHECK_ARG(ctx, ref2cur_pose && ref_dir && cur_dir && ref_points && ok);
  const size_t np_ = pose_stride == 0 ? 1 : (size_t)n;
  const size_t a = ((np_ * 56) + 255) & ~(size_t)255, b = (((size_t)n * 24) + 255) & ~(size_t)255;
  void *base = nullptr, *hbase = nullptr;
  const size_t total = a + 3 * b + (((size_t)n + 255) & ~(size_t)255);
  GH_TRY(gh_scratch(ctx, total, &base));
  GH_TRY(gh_pinned(ctx, total, &hbase));
  uint8_t *d = (uint8_t*)base, *hd = (uint8_t*)hbase;
  // [pose | ref_dir | cur_dir] up and [points | ok] down: one DMA each way through the pinned mirror of the layout
  memcpy(hd, ref2cur_pose, np_ * 56);
  memcpy(hd + a, ref_dir, (size_t)n * 24);
  memcpy(hd + a + b, cur_dir, (size_t)n * 24);
  GH_HIP(ctx, hipMemcpyAsync(d, hd, a + b + (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  GH_LAUNCH(ctx, "triangulate", triangulate_kernel, dim3(gh_div_up(n, 256)), dim3(256), 0, (const double*)d, pose_stride,
            (const double*)(d + a), (const double*)(d + a + b), n, (double*)(d + a + 2 * b), d + a + 3 * b);
  GH_HIP(ctx, hipMemcpyAsync(hd + a + 2 * b, d + a + 2 * b, b + (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(ref_points, hd + a + 2 * b, (size_t)n * 24);
  memcpy(ok, hd + a + 3 * b, (size_t)n);
  return GH_OK;
}
