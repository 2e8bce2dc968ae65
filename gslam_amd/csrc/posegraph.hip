// Pose-graph optimisation and 3-D alignment behind GSLAM::Optimizer (the part of the boundary that round 2 answered
// `false` to):
//   gh_pg_solve      Optimizer::optimize(BundleGraph&) with se3Graph / sim3Graph / gpsGraph edges
//                    (GSLAM/core/Optimizer.h:127-148,162-167,229): LM over SIM3 keyframes, UPDATE_KF_SCALE included
//   gh_align_sim3    Optimizer::optimizeICP (:210-217) and Optimizer::fitSim3 (:220-225): dst ~ s R src + t in closed form
// Specification = header of oracle/pg_oracle.c (the reference defines the data, not the solvers); the SIM3 algebra mirrors
// GSLAM/core/SIM3.h:114-270 / SE3.h:205-287 and is pinned to the reference through the oracle.
//
// CDNA4 mapping.  A pose graph is small next to a bundle adjustment (thousands of keyframes, tens of thousands of edges):
//   pg_edge      one THREAD per edge: residual + central-difference Jacobians (28 SIM3 log evaluations, ~30 k flop, no
//                memory traffic to speak of) -> per-edge blocks J_i^T L J_i, J_j^T L J_j, J_j^T L J_i, J^T L r, cost
//   pg_assemble  deterministic assembly of the dense normal equations: one wave per diagonal block (vertex) and per
//                distinct off-diagonal block (frame pair) sums the contributions of its edges in edge order (lists built
//                once on the host) -- no atomics, bitwise reproducible
//   solve        the dense SPD solver of the bundle adjustment (gh_potrf_solve_dev: MFMA f64, single-launch dataflow
//                factorisation for n <= ~3300).  Dense on purpose: 7 n_frames squared doubles is 1.6 GB at 2000 keyframes
//                and 157 GB at 20 000 -- the 288 GB of HBM hold what a CPU back end needs a sparse factorisation for
//   gr_model / pg_update / pg_cost   per-edge terms + fixed-order reductions (shared with the general graph solver below,
//                which gh_pg_solve is the landmark-free case of)
#include <math.h>

#include <algorithm>
#include <new>
#include <vector>

#include "bsparse.h"
#include "common.h"
#include "lm_rule.h"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kFdStep = 1e-6;

// ---------------------------------------------------------------- SIM3 algebra (qx qy qz qw tx ty tz s), as pg_oracle.c
__device__ __host__ inline void q_rot(const double* q, const double* p, double* o) {
  double uvx = q[1] * p[2] - q[2] * p[1], uvy = q[2] * p[0] - q[0] * p[2], uvz = q[0] * p[1] - q[1] * p[0];
  uvx += uvx; uvy += uvy; uvz += uvz;
  o[0] = p[0] + q[3] * uvx + (q[1] * uvz - q[2] * uvy);
  o[1] = p[1] + q[3] * uvy + (q[2] * uvx - q[0] * uvz);
  o[2] = p[2] + q[3] * uvz + (q[0] * uvy - q[1] * uvx);
}
__device__ __host__ inline void q_mul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__device__ __host__ inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __host__ inline void sim3_mul(const double* a, const double* b, double* o) {
  double q[4], t[3], st[3] = {a[7] * b[4], a[7] * b[5], a[7] * b[6]};
  q_mul(a, b, q);
  q_rot(a, st, t);
  for (int e = 0; e < 4; ++e) o[e] = q[e];
  for (int e = 0; e < 3; ++e) o[4 + e] = a[4 + e] + t[e];
  o[7] = a[7] * b[7];
}
__device__ __host__ inline void sim3_inv(const double* a, double* o) {
  double qc[4] = {-a[0], -a[1], -a[2], a[3]}, t[3];
  q_rot(qc, a + 4, t);
  const double is = 1.0 / a[7];
  for (int e = 0; e < 4; ++e) o[e] = qc[e];
  for (int e = 0; e < 3; ++e) o[4 + e] = -is * t[e];
  o[7] = is;
}
__device__ __host__ inline double rot_log(const double* q, double* r) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  double A_inv;
  if (n < 1e-10) {
    const double w2 = q[3] * q[3];
    A_inv = 2.0 / q[3] - 2.0 * (1.0 - w2) / (q[3] * w2);
  } else if (fabs(q[3]) < 1e-10) {
    A_inv = (q[3] > 0 ? kPi : -kPi) / n;
  } else {
    A_inv = 2.0 * atan(n / q[3]) / n;
  }
  r[0] = q[0] * A_inv;
  r[1] = q[1] * A_inv;
  r[2] = q[2] * A_inv;
  return A_inv * n;
}
__device__ __host__ inline void sim3_abc(double theta, double sigma, double* A, double* B, double* C) {
  const double th = fabs(theta), th2 = th * th, scale = exp(sigma);
  *C = fabs(sigma) < 1e-12 ? 1.0 + 0.5 * sigma : expm1(sigma) / sigma;
  if (th < 1e-5) {
    if (fabs(sigma) < 1e-3) {
      *A = 0.5 + sigma * (1.0 / 3.0 + sigma * (1.0 / 8.0 + sigma / 30.0));
      *B = 1.0 / 6.0 + sigma * (1.0 / 8.0 + sigma * (1.0 / 20.0 + sigma / 72.0));
    } else {
      const double s2 = sigma * sigma;
      *A = ((sigma - 1.0) * scale + 1.0) / s2;
      *B = ((0.5 * s2 - sigma + 1.0) * scale - 1.0) / (s2 * sigma);
    }
    return;
  }
  const double a = scale * sin(th), b = scale * cos(th), c = th2 + sigma * sigma;
  *A = (a * sigma + (1.0 - b) * th) / (th * c);
  *B = (*C - ((b - 1.0) * sigma + a * th) / c) / th2;
}
__device__ __host__ inline void sim3_exp(const double* mu, double* S) {
  const double* p = mu;
  const double* r = mu + 3;
  const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = sqrt(th2);
  double imag, real;
  if (th < 1e-5) {
    const double th4 = th2 * th2;
    imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
    real = 1.0 - th2 / 8.0 + th4 / 384.0;
  } else {
    imag = sin(0.5 * th) / th;
    real = cos(0.5 * th);
  }
  double A, B, C;
  sim3_abc(th, mu[6], &A, &B, &C);
  S[0] = imag * r[0];
  S[1] = imag * r[1];
  S[2] = imag * r[2];
  S[3] = real;
  double c1[3], c2[3];
  cross3(r, p, c1);
  cross3(r, c1, c2);
  for (int e = 0; e < 3; ++e) S[4 + e] = A * c1[e] + B * c2[e] + C * p[e];
  S[7] = exp(mu[6]);
}
__device__ __host__ inline void sim3_log(const double* S, double* mu) {
  double r[3];
  const double theta = rot_log(S, r);
  const double sigma = log(S[7]);
  double A, B, C;
  sim3_abc(theta, sigma, &A, &B, &C);
  const double th2 = theta * theta, x = C - B * th2, d = x * x + A * A * th2;
  const double ci = 1.0 / C, ai = -A / d, bi = (A * A - B * x) / (C * d);
  const double* t = S + 4;
  double c1[3], c2[3];
  cross3(r, t, c1);
  cross3(r, c1, c2);
  for (int e = 0; e < 3; ++e) {
    mu[e] = ci * t[e] + ai * c1[e] + bi * c2[e];
    mu[3 + e] = r[e];
  }
  mu[6] = sigma;
}
__device__ __host__ inline void sim3_retract(const double* S, const double* delta, double* out) {
  double E[8];
  sim3_exp(delta, E);
  sim3_mul(S, E, out);
  const double n = 1.0 / sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2] + out[3] * out[3]);
  for (int e = 0; e < 4; ++e) out[e] *= n;
}

// type 0 SE3 edge, 1 SIM3 edge, 2 GPS edge; returns the residual dimension
__device__ inline int edge_residual(int type, const double* Si, const double* Sj, const double* meas, double* r) {
  if (type == 1) {
    double Mi[8], Sii[8], E1[8], E2[8];
    sim3_inv(meas, Mi);
    sim3_inv(Si, Sii);
    sim3_mul(Sii, Sj, E1);
    sim3_mul(Mi, E1, E2);
    sim3_log(E2, r);
    return 7;
  }
  double M[8] = {meas[0], meas[1], meas[2], meas[3], meas[4], meas[5], meas[6], 1.0}, Mi[8];
  double Ti[8] = {Si[0], Si[1], Si[2], Si[3], Si[4], Si[5], Si[6], 1.0}, E2[8], mu[7];
  sim3_inv(M, Mi);
  if (type == 0) {
    double Tj[8] = {Sj[0], Sj[1], Sj[2], Sj[3], Sj[4], Sj[5], Sj[6], 1.0}, Tii[8], E1[8];
    sim3_inv(Ti, Tii);
    sim3_mul(Tii, Tj, E1);
    sim3_mul(Mi, E1, E2);
  } else {
    sim3_mul(Mi, Ti, E2);
  }
  sim3_log(E2, mu);
  for (int a = 0; a < 6; ++a) r[a] = mu[a];
  return 6;
}

struct PgGraph {
  int n_frames, n_edges;
  const int32_t* dof;
  const int32_t *etype, *ei, *ej;
  const double* meas;  // n_edges x 8
  const double* info;  // n_edges x 49 or null
};

// per-edge record (doubles): [0..48] A_ii, [49..97] A_jj, [98..146] A_ji, [147..153] b_i, [154..160] b_j, [161..209] J_i,
// [210..258] J_j, [259..265] L r, then padding to kEdgeRec
constexpr int kEdgeRec = 272;

__device__ inline void load_info(const PgGraph& G, int e, int dim, double* L) {
  if (G.info) {
    for (int k = 0; k < 49; ++k) L[k] = G.info[(size_t)49 * e + k];
    return;
  }
  for (int k = 0; k < 49; ++k) L[k] = 0.0;
  for (int a = 0; a < dim; ++a) L[7 * a + a] = 1.0;
}

// 16 lanes per edge (4 edges per 64-thread block): lanes 0..13 each take ONE Jacobian column (endpoint = lane / 7,
// component = lane % 7: two retractions + two SIM3 logs), lane 14 the residual itself; the products are then dealt over the
// 16 lanes.  Every sum keeps the loop order of the oracle, so the record is bit-identical to a one-thread-per-edge evaluation
// -- 14 times less latency, which is what a few hundred edges are bound by.
__global__ __launch_bounds__(64) void pg_edge_kernel(PgGraph G, const double* __restrict__ S, double* __restrict__ rec,
                                                     double* __restrict__ cost_e) {
  __shared__ double sJ[4][2][49], sL[4][49], sLr[4][7], sLJ[4][2][49];
  const int slot = threadIdx.x >> 4, t = threadIdx.x & 15;
  const int e = blockIdx.x * 4 + slot;
  const bool live = e < G.n_edges;
  int type = 0, i = 0, j = -1, dim = 0;
  double Si[8], Sj[8], meas[8];
  if (live) {
    type = G.etype[e];
    i = G.ei[e];
    j = G.ej[e];
    for (int k = 0; k < 8; ++k) {
      Si[k] = S[8 * (size_t)i + k];
      Sj[k] = j >= 0 ? S[8 * (size_t)j + k] : Si[k];
      meas[k] = G.meas[8 * (size_t)e + k];
    }
    dim = type == 1 ? 7 : 6;
    if (t < 14) {
      const int which = t / 7, k = t - 7 * which;
      const int dof = which == 0 ? G.dof[i] : (j >= 0 ? G.dof[j] : 0);
      double col[7] = {0, 0, 0, 0, 0, 0, 0};
      if ((which == 0 || j >= 0) && ((dof >> k) & 1)) {
        double dp[7] = {0, 0, 0, 0, 0, 0, 0}, Sp[8], Sm[8], rp[7], rm[7];
        dp[k] = kFdStep;
        sim3_retract(which == 0 ? Si : Sj, dp, Sp);
        dp[k] = -kFdStep;
        sim3_retract(which == 0 ? Si : Sj, dp, Sm);
        edge_residual(type, which == 0 ? Sp : Si, which == 0 ? Sj : Sp, meas, rp);
        edge_residual(type, which == 0 ? Sm : Si, which == 0 ? Sj : Sm, meas, rm);
        for (int a = 0; a < dim; ++a) col[a] = (rp[a] - rm[a]) / (2.0 * kFdStep);
      }
      for (int a = 0; a < 7; ++a) sJ[slot][which][7 * a + k] = col[a];
    } else if (t == 14) {
      double r[7], L[49], q = 0;
      edge_residual(type, Si, Sj, meas, r);
      load_info(G, e, dim, L);
      for (int k = 0; k < 49; ++k) sL[slot][k] = L[k];
      for (int a = 0; a < 7; ++a) {
        double s = 0;
        if (a < dim) {
          for (int b = 0; b < dim; ++b) s += L[7 * a + b] * r[b];
          q += r[a] * s;
        }
        sLr[slot][a] = s;
      }
      cost_e[e] = 0.5 * q;
    }
  }
  __syncthreads();
  // L J (dim x 7) for both endpoints: 98 entries over the 16 lanes
  if (live)
    for (int idx = t; idx < 98; idx += 16) {
      const int which = idx / 49, ak = idx - 49 * which, a = ak / 7, k = ak - 7 * a;
      double s = 0;
      if (a < dim)
        for (int b = 0; b < dim; ++b) s += sL[slot][7 * a + b] * sJ[slot][which][7 * b + k];
      sLJ[slot][which][ak] = s;
    }
  __syncthreads();
  if (!live) return;
  double* o = rec + (size_t)kEdgeRec * e;
  const double(*J)[49] = sJ[slot];
  const double(*LJ)[49] = sLJ[slot];
  // the three 7 x 7 blocks (147 entries), the two gradient pieces (14), the Jacobians (98) and L r (7)
  for (int idx = t; idx < 147; idx += 16) {
    const int blk = idx / 49, pq = idx - 49 * blk, p = pq / 7, q2 = pq - 7 * p;
    double h = 0;
    for (int a = 0; a < dim; ++a)
      h += blk == 0 ? J[0][7 * a + p] * LJ[0][7 * a + q2] : blk == 1 ? J[1][7 * a + p] * LJ[1][7 * a + q2] : J[1][7 * a + p] * LJ[0][7 * a + q2];
    o[49 * blk + 7 * p + q2] = h;  // A_ii, A_jj, A_ji (row index in frame j, column index in frame i)
  }
  if (t < 14) {
    const int which = t / 7, p = t - 7 * which;
    double g = 0;
    for (int a = 0; a < dim; ++a) g += J[which][7 * a + p] * sLr[slot][a];
    o[147 + 7 * which + p] = g;
  }
  for (int idx = t; idx < 98; idx += 16) o[161 + idx] = idx < 49 ? J[0][idx] : J[1][idx - 49];
  if (t < 7) o[259 + t] = sLr[slot][t];
}

// residual-only pass at a candidate state
__global__ __launch_bounds__(64) void pg_cost_kernel(PgGraph G, const double* __restrict__ S, double* __restrict__ cost_e) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= G.n_edges) return;
  const int type = G.etype[e], i = G.ei[e], j = G.ej[e];
  double Si[8], Sj[8], meas[8], r[7], L[49];
  for (int k = 0; k < 8; ++k) {
    Si[k] = S[8 * (size_t)i + k];
    Sj[k] = j >= 0 ? S[8 * (size_t)j + k] : Si[k];
    meas[k] = G.meas[8 * (size_t)e + k];
  }
  const int dim = edge_residual(type, Si, Sj, meas, r);
  load_info(G, e, dim, L);
  double q = 0;
  for (int a = 0; a < dim; ++a) {
    double s = 0;
    for (int b = 0; b < dim; ++b) s += L[7 * a + b] * r[b];
    q += r[a] * s;
  }
  cost_e[e] = 0.5 * q;
}

// Sequential (edge-order) sum by ONE thread per output word: the sums are short (edges per vertex / per frame pair) and
// the order is the oracle's, so H and g are reproducible bit for bit from run to run.
//   block b < n_frames: diagonal block of frame b (+ gradient); contributions (edge, role) from vlist[vstart[b] ..]
//   block b >= n_frames: off-diagonal block of frame pair b - n_frames; contributions (edge, flip) from plist[pstart[..] ..]
struct PgLists {
  const int32_t *vstart, *vlist;  // vlist entry = edge << 1 | role (0: the frame is the edge's i, 1: its j)
  const int32_t *pstart, *plist;  // plist entry = edge << 1 | flip (0: block row = frame j of the edge, 1: transposed)
  const int32_t *prow, *pcol;     // pair -> (row frame, column frame), row > column
  int n_pairs;
};

__global__ __launch_bounds__(64) void pg_assemble_kernel(PgGraph G, PgLists Ls, const double* __restrict__ rec,
                                                         double* __restrict__ H, int lda, double* __restrict__ g,
                                                         unsigned long long* __restrict__ gmax_bits) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < G.n_frames) {
    if (t < 49) {
      const int p = t / 7, q = t - 7 * p;
      double s = 0;
      for (int k = Ls.vstart[b]; k < Ls.vstart[b + 1]; ++k) {
        const int v = Ls.vlist[k];
        s += rec[(size_t)kEdgeRec * (v >> 1) + ((v & 1) ? 49 : 0) + 7 * p + q];
      }
      H[(size_t)(7 * b + q) * lda + 7 * b + p] = s;  // column-major, whole diagonal block
    } else if (t < 56) {
      const int p = t - 49;
      double s = 0;
      for (int k = Ls.vstart[b]; k < Ls.vstart[b + 1]; ++k) {
        const int v = Ls.vlist[k];
        s += rec[(size_t)kEdgeRec * (v >> 1) + ((v & 1) ? 154 : 147) + p];
      }
      g[7 * b + p] = s;
      atomicMax(gmax_bits, (unsigned long long)__double_as_longlong(fabs(s)));  // |s| >= 0: the bit pattern orders like the value
    }
    return;
  }
  const int pr = b - G.n_frames;
  if (pr >= Ls.n_pairs || t >= 49) return;
  const int p = t / 7, q = t - 7 * p;  // element (p, q) of the block: row in the ROW frame, column in the COLUMN frame
  double s = 0;
  for (int k = Ls.pstart[pr]; k < Ls.pstart[pr + 1]; ++k) {
    const int v = Ls.plist[k];
    // A_ji is stored with rows in the edge's frame j: if the edge's j is this pair's column frame, read it transposed
    s += rec[(size_t)kEdgeRec * (v >> 1) + 98 + ((v & 1) ? 7 * q + p : 7 * p + q)];
  }
  const int rf = Ls.prow[pr], cf = Ls.pcol[pr];
  H[(size_t)(7 * cf + q) * lda + 7 * rf + p] = s;  // lower triangle (row frame > column frame)
}

// The same sums stored into the block-sparse layout of bsparse.h: block b (frames first, then pairs) goes to
// V[off[b] + p * sp[b] + q * sq[b]] (sp / sq swap when the elimination order puts the pair's row frame first).
struct BsDest {
  const int64_t* off;
  const int32_t *sp, *sq;
};
__global__ __launch_bounds__(64) void pg_assemble_bs_kernel(PgGraph G, PgLists Ls, const double* __restrict__ rec,
                                                            double* __restrict__ V, BsDest D, double* __restrict__ g) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < G.n_frames) {
    if (t < 49) {
      const int p = t / 7, q = t - 7 * p;
      double s = 0;
      for (int k = Ls.vstart[b]; k < Ls.vstart[b + 1]; ++k) {
        const int v = Ls.vlist[k];
        s += rec[(size_t)kEdgeRec * (v >> 1) + ((v & 1) ? 49 : 0) + 7 * p + q];
      }
      V[D.off[b] + p * D.sp[b] + q * D.sq[b]] = s;
    } else if (t < 56) {
      const int p = t - 49;
      double s = 0;
      for (int k = Ls.vstart[b]; k < Ls.vstart[b + 1]; ++k) {
        const int v = Ls.vlist[k];
        s += rec[(size_t)kEdgeRec * (v >> 1) + ((v & 1) ? 154 : 147) + p];
      }
      g[7 * b + p] = s;
    }
    return;
  }
  const int pr = b - G.n_frames;
  if (pr >= Ls.n_pairs || t >= 49) return;
  const int p = t / 7, q = t - 7 * p;
  double s = 0;
  for (int k = Ls.pstart[pr]; k < Ls.pstart[pr + 1]; ++k) {
    const int v = Ls.plist[k];
    s += rec[(size_t)kEdgeRec * (v >> 1) + 98 + ((v & 1) ? 7 * q + p : 7 * p + q)];
  }
  V[D.off[b] + p * D.sp[b] + q * D.sq[b]] = s;
}

// Hd = H (lower blocks incl. the diagonal) + clamp(H_kk, 1e-6, 1e32) / radius on the diagonal; d = -g
__global__ __launch_bounds__(256) void pg_damp_kernel(const double* __restrict__ H, double* __restrict__ Hd, int n, int lda,
                                                      const double* __restrict__ g, double* __restrict__ d, double radius) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)n * lda;
  if (idx < total) {
    const size_t col = idx / lda, row = idx - col * lda;
    double v = H[idx];
    if (row == col && row < (size_t)n) {
      const double c = v < 1e-6 ? 1e-6 : (v > 1e32 ? 1e32 : v);
      v += c / radius;
    }
    Hd[idx] = v;
  }
  if (idx < (size_t)n) d[idx] = -g[idx];
}

__global__ __launch_bounds__(256) void pg_update_kernel(int n_frames, const int32_t* __restrict__ dof, const double* __restrict__ S,
                                                        const double* __restrict__ d, double* __restrict__ Snew) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frames) return;
  double s[8], o[8], dl[7];
  for (int k = 0; k < 8; ++k) s[k] = S[8 * (size_t)f + k];
  if ((dof[f] & 127) == 0) {
    for (int k = 0; k < 8; ++k) Snew[8 * (size_t)f + k] = s[k];
    return;
  }
  for (int k = 0; k < 7; ++k) dl[k] = d[7 * (size_t)f + k];
  sim3_retract(s, dl, o);
  for (int k = 0; k < 8; ++k) Snew[8 * (size_t)f + k] = o[k];
}

// out[0] = sum of v[0..n) in index order (one thread: the sums are a few thousand terms and the order is the contract)
__global__ void pg_sum_kernel(const double* __restrict__ v, int n, double* __restrict__ out, int slot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0;
  for (int k = 0; k < n; ++k) s += v[k];
  out[slot] = s;
}

double now_ms_pg() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// Host side of the pose-graph part of a problem: the three edge lists flattened (order: SE3, SIM3, GPS -- the oracle's)
// and the assembly lists of pg_assemble_kernel.
struct PoseHost {
  int ne = 0, n_pairs = 0;
  bool any_info = false;
  std::vector<int32_t> etype, ei, ej, vstart, vlist, pstart, plist, prow, pcol;
  std::vector<double> meas, info;
  gh_status build(gh_ctx* ctx, const gh_pg_problem* pr);
};

gh_status PoseHost::build(gh_ctx* ctx, const gh_pg_problem* pr) {
  const int nf = pr->n_frames;
  ne = pr->n_se3 + pr->n_sim3 + pr->n_gps;
  etype.assign((size_t)(ne > 0 ? ne : 1), 0);
  ei.assign(etype.size(), 0);
  ej.assign(etype.size(), 0);
  meas.assign((size_t)8 * etype.size(), 1.0);
  any_info = pr->se3_info || pr->sim3_info || pr->gps_info;
  if (any_info) info.assign((size_t)49 * etype.size(), 0.0);
  int e = 0;
  auto put = [&](int type, int i, int j, const double* m, int mlen, const double* inf, int dim) -> bool {
    if (i < 0 || i >= nf || (type != 2 && (j < 0 || j >= nf || j == i))) return false;
    etype[e] = type;
    ei[e] = i;
    ej[e] = type == 2 ? -1 : j;
    for (int k = 0; k < mlen; ++k) meas[8 * (size_t)e + k] = m[k];
    if (any_info)
      for (int a = 0; a < dim; ++a)
        for (int b = 0; b < dim; ++b) info[49 * (size_t)e + 7 * a + b] = inf ? inf[dim * a + b] : (a == b ? 1.0 : 0.0);
    ++e;
    return true;
  };
  for (int k = 0; k < pr->n_se3; ++k)
    GH_CHECK_ARG(ctx, put(0, pr->se3_first[k], pr->se3_second[k], pr->se3_meas + 7 * (size_t)k, 7,
                          pr->se3_info ? pr->se3_info + 36 * (size_t)k : nullptr, 6));
  for (int k = 0; k < pr->n_sim3; ++k) {
    GH_CHECK_ARG(ctx, pr->sim3_meas[8 * (size_t)k + 7] > 0);
    GH_CHECK_ARG(ctx, put(1, pr->sim3_first[k], pr->sim3_second[k], pr->sim3_meas + 8 * (size_t)k, 8,
                          pr->sim3_info ? pr->sim3_info + 49 * (size_t)k : nullptr, 7));
  }
  for (int k = 0; k < pr->n_gps; ++k)
    GH_CHECK_ARG(ctx, put(2, pr->gps_frame[k], -1, pr->gps_meas + 7 * (size_t)k, 7,
                          pr->gps_info ? pr->gps_info + 36 * (size_t)k : nullptr, 6));
  vstart.assign((size_t)nf + 1, 0);
  for (int k = 0; k < ne; ++k) {
    vstart[ei[k] + 1]++;
    if (ej[k] >= 0) vstart[ej[k] + 1]++;
  }
  for (int f = 0; f < nf; ++f) vstart[f + 1] += vstart[f];
  vlist.resize((size_t)std::max(1, vstart[nf]));
  {
    std::vector<int32_t> fill(vstart.begin(), vstart.end() - 1);
    for (int k = 0; k < ne; ++k) {
      vlist[fill[ei[k]]++] = (k << 1) | 0;
      if (ej[k] >= 0) vlist[fill[ej[k]]++] = (k << 1) | 1;
    }
  }
  // distinct frame pairs (row > column), edges of a pair in edge order
  std::vector<std::pair<long long, int32_t>> keyed;  // (pair key, edge << 1 | flip)
  for (int k = 0; k < ne; ++k) {
    if (ej[k] < 0) continue;
    const int rf = std::max(ei[k], ej[k]), cf = std::min(ei[k], ej[k]);
    // A_ji has its rows in frame j: transposed read when j is the column frame
    keyed.push_back({(long long)rf * nf + cf, (k << 1) | (ej[k] == rf ? 0 : 1)});
  }
  std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  pstart.assign(1, 0);
  for (size_t k = 0; k < keyed.size(); ++k) {
    if (k == 0 || keyed[k].first != keyed[k - 1].first) {
      if (k) pstart.push_back((int32_t)plist.size());
      prow.push_back((int32_t)(keyed[k].first / nf));
      pcol.push_back((int32_t)(keyed[k].first % nf));
    }
    plist.push_back(keyed[k].second);
  }
  pstart.push_back((int32_t)plist.size());
  n_pairs = (int)prow.size();
  if (plist.empty()) plist.push_back(0);
  if (prow.empty()) { prow.push_back(0); pcol.push_back(0); }

  return GH_OK;
}

}  // namespace

// ---------------------------------------------------------------- general BundleGraph: landmarks on top of the pose graph
// gh_graph_solve: SIM3 keyframes + pose-graph edges + XYZ and inverse-depth landmarks with pinhole observations in ONE
// graph (GSLAM/core/Optimizer.h:150-172) -- what the specialised bundle adjustment of ba.hip (SE3 cameras, XYZ points
// only) does not cover: inverse-depth points, keyframe scale, pose-graph edges mixed with observations.  Specification =
// header of oracle/graph_oracle.c.  Same LM loop as gh_pg_solve; the landmarks (3 x 3 / 1 x 1 blocks) are eliminated by a
// Schur complement into the dense keyframe system:
//   gr_obs_lin     one thread per observation: residual, Huber weight, analytic Jacobians w.r.t. the observing keyframe,
//                  the host keyframe (inverse depth) and the landmark -> record; J^T L J / J^T L r added to the keyframe
//                  blocks of H, to g and to the landmark's H_pp / g_p with f64 atomics (the sums are short; their order,
//                  hence the last bits, varies from run to run -- the parity tests carry that in their tolerance)
//   gr_lm_prepare  one thread per landmark: (H_pp + D)^-1 in closed form
//   gr_schur       one thread per (observation, keyframe) slot a: U_a = W_a (H_pp + D)^-1; rhs += U_a g_p; for every slot b
//                  of the same landmark with frame(b) <= frame(a): block(frame a, frame b) -= U_a W_b^T
//   gr_backsub     one thread per landmark: d_p = -(H_pp + D)^-1 (g_p + sum W^T d_f)
//   gr_model / gr_cost / gr_reduce   per-item terms and a fixed-order two-level sum
namespace {

constexpr double kMinDepthG = 1e-9;
constexpr int kObsRec = 40;     // r(2) L(4) Jj(14) Jh(14) Jp(6)
constexpr int kCamPart = 54;    // per wave of gr_obs_lin: g_c (9) and the lower triangle of block(c, c) (45), row by row
constexpr int kObsRecCam = 58;  // ... + Jc(18): the record of a graph with a camera (GrLandmarks::rec is one of the two)

struct GrLandmarks {
  int n_xyz, n_idp, n_obs;
  const uint8_t* xyz_free;
  const int32_t* idp_host;
  const double* idp_anchor;
  const uint8_t* idp_free;
  const int32_t *obs_kind, *obs_point, *obs_frame;
  const double* obs_xy;
  const double* obs_info;  // may be null
  const int32_t *lstart, *llist;  // observations by landmark (XYZ points first, then inverse-depth points)
  double huber;
  int projection;             // 0 pinhole (obs_xy n x 2), 1 sphere (obs_xy n x 3 unit bearings)
  // BundleGraph::camera + cameraDOF (Optimizer.h:86-100,169-171): with_cam = the observations are pixels of the camera
  // c = fx fy cx cy k1 k2 p1 p2 k3 (the current / candidate value is a kernel argument), cam_free = which of the nine are
  // unknowns; they sit behind the keyframes in the reduced system: rows 7 n_frames .. 7 n_frames + 8
  int with_cam, cam_free, n_frames, rec;
};

// pixel coordinates of the normalised point (x, y), A = d(U, V)/d(x, y), Jc = d(U, V)/dc (2 x 9): GSLAM's OpenCV camera
// model (GSLAM/core/Camera.h:396-406; the pinhole model is k = p = 0), same operation order as oracle_cam_project
__device__ inline void cam_project(const double* c, double x, double y, double* UV, double* A, double* Jc) {
  const double fx = c[0], fy = c[1], k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, r4 = r2 * r2, r6 = r2 * r4, xy2 = x * y * 2.0;
  const double rad = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
  const double X1 = x * rad + xy2 * p1 + p2 * (r2 + 2.0 * x2);
  const double Y1 = y * rad + xy2 * p2 + p1 * (r2 + 2.0 * y2);
  UV[0] = c[2] + fx * X1;
  UV[1] = c[3] + fy * Y1;
  if (A) {
    const double radp = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4;
    A[0] = fx * (rad + 2.0 * x2 * radp + 2.0 * p1 * y + 6.0 * p2 * x);
    A[1] = fx * (2.0 * x * y * radp + 2.0 * p1 * x + 2.0 * p2 * y);
    A[2] = fy * (2.0 * x * y * radp + 2.0 * p2 * y + 2.0 * p1 * x);
    A[3] = fy * (rad + 2.0 * y2 * radp + 2.0 * p2 * x + 6.0 * p1 * y);
  }
  if (Jc) {
    for (int e = 0; e < 18; ++e) Jc[e] = 0.0;
    Jc[0] = X1;                   Jc[9 + 1] = Y1;
    Jc[2] = 1.0;                  Jc[9 + 3] = 1.0;
    Jc[4] = fx * x * r2;          Jc[9 + 4] = fy * y * r2;
    Jc[5] = fx * x * r4;          Jc[9 + 5] = fy * y * r4;
    Jc[6] = fx * xy2;             Jc[9 + 6] = fy * (r2 + 2.0 * y2);
    Jc[7] = fx * (r2 + 2.0 * x2); Jc[9 + 7] = fy * xy2;
    Jc[8] = fx * x * r6;          Jc[9 + 8] = fy * y * r6;
  }
}

__device__ inline void q_matrix(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// tangent plane of a unit bearing: e1 = normalise(b x k), e2 = b x e1, k = the axis b is least aligned with
__device__ inline void tangent_basis(const double* b, double* e1, double* e2) {
  const double ax = fabs(b[0]), ay = fabs(b[1]), az = fabs(b[2]);
  double k[3] = {0, 0, 0};
  if (ax <= ay && ax <= az) k[0] = 1;
  else if (ay <= az) k[1] = 1;
  else k[2] = 1;
  e1[0] = b[1] * k[2] - b[2] * k[1];
  e1[1] = b[2] * k[0] - b[0] * k[2];
  e1[2] = b[0] * k[1] - b[1] * k[0];
  const double n = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
  for (int e = 0; e < 3; ++e) e1[e] *= n;
  e2[0] = b[1] * e1[2] - b[2] * e1[1];
  e2[1] = b[2] * e1[0] - b[0] * e1[2];
  e2[2] = b[0] * e1[1] - b[1] * e1[0];
}

// residual r, quadratic form s = r^T Lambda r, Huber weight; optionally the Jacobians.  false: not in front of the camera
// (pinhole) / on the opposite hemisphere (sphere)
template <bool WITH_J>
__device__ inline bool graph_obs(int kind, const double* Sj, int dof_j, const double* Sh, int dof_h, bool same_host,
                                 const double* lm, bool lm_free, const double* anchor, const double* m, const double* info,
                                 double huber, double* r, double* wgt, double* s_out, double* Jj, double* Jh, double* Jp,
                                 int projection, const double* cam = nullptr, int cam_free = 0, double* Jc = nullptr) {
  double Z[3], Y[3], Ra[3] = {0, 0, 0}, dth[3] = {0, 0, 0};
  if (kind == 0) {
    for (int e = 0; e < 3; ++e) Z[e] = lm[e] - Sj[4 + e];
  } else {
    q_rot(Sh, anchor, Ra);
    for (int e = 0; e < 3; ++e) {
      dth[e] = Sh[4 + e] - Sj[4 + e];
      Z[e] = Sh[7] * Ra[e] + lm[0] * dth[e];
    }
  }
  const double qc[4] = {-Sj[0], -Sj[1], -Sj[2], Sj[3]};
  q_rot(qc, Z, Y);
  double P[6];
  if (projection == 0) {
    if (!(Y[2] > kMinDepthG)) return false;
    const double iz = 1.0 / Y[2], u = Y[0] * iz, v = Y[1] * iz;
    P[0] = iz; P[1] = 0; P[2] = -u * iz; P[3] = 0; P[4] = iz; P[5] = -v * iz;
    if (cam) {
      double UV[2], A[4], Jcf[18];
      cam_project(cam, u, v, UV, WITH_J ? A : nullptr, WITH_J ? Jcf : nullptr);
      r[0] = UV[0] - m[0];
      r[1] = UV[1] - m[1];
      if (WITH_J) {
        const double P0[6] = {P[0], P[1], P[2], P[3], P[4], P[5]};
        for (int e = 0; e < 3; ++e) {
          P[e] = A[0] * P0[e] + A[1] * P0[3 + e];
          P[3 + e] = A[2] * P0[e] + A[3] * P0[3 + e];
        }
        for (int a = 0; a < 2; ++a)
          for (int k = 0; k < 9; ++k) Jc[9 * a + k] = ((cam_free >> k) & 1) ? Jcf[9 * a + k] : 0.0;
      }
    } else {
      r[0] = u - m[0];
      r[1] = v - m[1];
    }
  } else {
    const double nY = sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
    if (!(nY > kMinDepthG)) return false;
    const double in = 1.0 / nY, y[3] = {Y[0] * in, Y[1] * in, Y[2] * in};
    if (!(y[0] * m[0] + y[1] * m[1] + y[2] * m[2] > 0)) return false;
    double e1[3], e2[3];
    tangent_basis(m, e1, e2);
    r[0] = e1[0] * y[0] + e1[1] * y[1] + e1[2] * y[2];
    r[1] = e2[0] * y[0] + e2[1] * y[1] + e2[2] * y[2];
    for (int e = 0; e < 3; ++e) {  // E (I - y y^T) / |Y|
      P[e] = (e1[e] - r[0] * y[e]) * in;
      P[3 + e] = (e2[e] - r[1] * y[e]) * in;
    }
  }
  double L00 = 1, L01 = 0, L10 = 0, L11 = 1;
  if (info) { L00 = info[0]; L01 = info[1]; L10 = info[2]; L11 = info[3]; }
  const double s = r[0] * (L00 * r[0] + L01 * r[1]) + r[1] * (L10 * r[0] + L11 * r[1]);
  double w = 1.0;
  if (huber > 0 && s > huber * huber) w = huber / sqrt(s);
  *wgt = w;
  *s_out = s;
  if (!WITH_J) return true;
  for (int k = 0; k < 14; ++k) Jj[k] = Jh[k] = 0.0;
  for (int k = 0; k < 6; ++k) Jp[k] = 0.0;
  if (kind == 1 && same_host) return true;
  const double c = kind == 0 ? 1.0 : lm[0];
  const double Dj[21] = {-c * Sj[7], 0, 0, 0, -Y[2], Y[1], 0,
                         0, -c * Sj[7], 0, Y[2], 0, -Y[0], 0,
                         0, 0, -c * Sj[7], -Y[1], Y[0], 0, 0};
  for (int a = 0; a < 2; ++a)
    for (int k = 0; k < 7; ++k) {
      double acc = 0;
      for (int e = 0; e < 3; ++e) acc += P[3 * a + e] * Dj[7 * e + k];
      Jj[7 * a + k] = ((dof_j >> k) & 1) ? acc : 0.0;
    }
  double Rj[9];
  q_matrix(Sj, Rj);
  if (kind == 0) {
    for (int a = 0; a < 2; ++a)
      for (int k = 0; k < 3; ++k) {
        double acc = 0;
        for (int e = 0; e < 3; ++e) acc += P[3 * a + e] * Rj[3 * k + e];
        Jp[3 * a + k] = lm_free ? acc : 0.0;
      }
    return true;
  }
  double Rh[9], M[9];
  q_matrix(Sh, Rh);
  for (int e = 0; e < 3; ++e)
    for (int f = 0; f < 3; ++f) {
      double acc = 0;
      for (int k = 0; k < 3; ++k) acc += Rj[3 * k + e] * Rh[3 * k + f];
      M[3 * e + f] = acc;
    }
  const double nax[9] = {0, anchor[2], -anchor[1], -anchor[2], 0, anchor[0], anchor[1], -anchor[0], 0};
  double Dh[21];
  for (int e = 0; e < 3; ++e) {
    for (int k = 0; k < 3; ++k) {
      Dh[7 * e + k] = lm[0] * Sh[7] * M[3 * e + k];
      double acc = 0;
      for (int f = 0; f < 3; ++f) acc += M[3 * e + f] * nax[3 * f + k];
      Dh[7 * e + 3 + k] = Sh[7] * acc;
    }
    Dh[7 * e + 6] = Sh[7] * (M[3 * e] * anchor[0] + M[3 * e + 1] * anchor[1] + M[3 * e + 2] * anchor[2]);
  }
  for (int a = 0; a < 2; ++a)
    for (int k = 0; k < 7; ++k) {
      double acc = 0;
      for (int e = 0; e < 3; ++e) acc += P[3 * a + e] * Dh[7 * e + k];
      Jh[7 * a + k] = ((dof_h >> k) & 1) ? acc : 0.0;
    }
  double dr[3];
  q_rot(qc, dth, dr);
  for (int a = 0; a < 2; ++a) Jp[3 * a] = lm_free ? P[3 * a] * dr[0] + P[3 * a + 1] * dr[1] + P[3 * a + 2] * dr[2] : 0.0;
  return true;
}

// REPRODUCIBLE ACCUMULATION (gh_ba_options.deterministic, the default).  The landmark part of the normal equations is summed
// with f64 atomics, whose order changes from run to run -- and with it the last bits of H, the step, and now and then an LM
// decision taken within rounding of a threshold.  Floating-point addition is exact, hence order-independent,
// when every summand is a multiple of a common quantum q and every partial sum stays below 2^52 q.  So each contribution v is
// split against two constants,  h = (v + M1) - M1,  l = ((v - h) + M2) - M2  (M = 1.5 * 2^E: the classic pre-rounding of
// reproducible summation), and h / l are added -- with the same atomics -- into two ZEROED accumulators shaped like the target;
// a fold kernel adds hi + lo to the target afterwards.  With |v| <= B and at most 2^K contributions per word,
// E1 = log2 B + K + 1 keeps 51 - K bits of the largest contributions in h, and l (quantum 2^(E1 - 104 + K)) the next 51 - K:
// what is dropped is below 2^(2K - 103) B -- beyond double precision of a word of size B for the K <= 20 of any real graph.
// B is a bound PER BLOCK of the reduced system, not one for the whole of it: a word far below the bound keeps only
// 103 - 2K - log2(B / |word|) bits, and one observation with large Jacobians (a keyframe of scale 1e3, a point 2e-9 in front
// of a camera) must not set the quantum of blocks it does not add to.  gr_obs_lin_kernel takes, per keyframe f (and for
// the intrinsics), B_f = the maximum over the observations with a slot in f of 16 |L| |J_f|^2 (an atomicMax: order-
// independent by itself); a word of block (f, g) uses max(B_f, B_g).  Every contribution to that block is an entry of
// J_f^T L J_g, or of a Schur product W_f V^-1 W_g^T, which the positive semi-definite per-landmark Hessian bounds by the
// geometric mean of the landmark's J_f^T L J_f and J_g^T L J_g -- the landmark's own Jacobian J_p does not enter (it cancels
// in W V^-1 W^T), so it is not part of the bound.  The right-hand sides (J_f^T L r, U g_p) couple a keyframe to the
// residuals of every observation of its landmarks: their words use one bound for all, the maximum of 16 |L| max(|J_f|, |r|)^2.
// 2^8 of head room.  Twice the atomics of the plain mode, bit-identical results run to run.
struct DetAcc {
  double* hi;   // matrix-shaped accumulators (null: plain atomics straight into the target)
  double* lo;
  double* vhi;  // vector-shaped ones (right-hand side)
  double* vlo;
  const unsigned long long* bound_bits;  // bits of the bounds (non-negative doubles): [f] keyframe f, [n_frames] intrinsics, [n_frames + 1] vectors
  int K;
  int n_frames;
};
struct DetConst { double M1, M2; };
__device__ inline DetConst det_consts_of(const DetAcc& A, double B) {
  DetConst c{0.0, 0.0};
  if (A.hi == nullptr) return c;
  int e = B > 0.0 ? ilogb(B) + 1 : -900;   // |v| <= B < 2^e
  e += 8;                                  // head room
  if (e < -900) e = -900;
  if (e > 900) e = 900;
  const int E1 = e + A.K + 1, E2 = E1 - 53 + A.K + 1;
  c.M1 = ldexp(1.5, E1);
  c.M2 = ldexp(1.5, E2);
  return c;
}
// the constants of the right-hand-side words ...
__device__ inline DetConst det_consts_vec(const DetAcc& A) {
  if (A.hi == nullptr) return DetConst{0.0, 0.0};
  return det_consts_of(A, __longlong_as_double((long long)A.bound_bits[A.n_frames + 1]));
}
// ... and of the words of block (fa, fb); the intrinsics are block index n_frames
__device__ inline DetConst det_consts_block(const DetAcc& A, int fa, int fb) {
  if (A.hi == nullptr) return DetConst{0.0, 0.0};
  return det_consts_of(A, fmax(__longlong_as_double((long long)A.bound_bits[fa]), __longlong_as_double((long long)A.bound_bits[fb])));
}
// *word = max(*word, bits of B) for a bound B (non-negative doubles order like their bit patterns).  Most observations do not
// raise the maximum: the word is read first (any stale value is a smaller one, and then the atomic decides), so that the
// observations of a keyframe do not queue on one address.
__device__ __forceinline__ void bound_max(unsigned long long* word, double B) {
  if (!(B > 0.0 && B < 1e300)) return;
  const unsigned long long b = (unsigned long long)__double_as_longlong(B);
  if (b > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, b);
}
// target[off] += v: plain atomic, or the two pre-rounded parts into the accumulators
__device__ __forceinline__ void acc_add(double* target, double* hi, double* lo, size_t off, double v, const DetConst& c) {
  if (hi == nullptr) {
    atomicAdd(target + off, v);
  } else {
    const double h = (v + c.M1) - c.M1;
    const double l = ((v - h) + c.M2) - c.M2;
    if (h != 0.0) atomicAdd(hi + off, h);
    if (l != 0.0) atomicAdd(lo + off, l);
  }
}
// target += hi + lo (matrix: n columns of lda; vector: nv words), one fixed expression per word
__global__ __launch_bounds__(256) void gr_det_fold_kernel(double* __restrict__ M, const double* __restrict__ hi, const double* __restrict__ lo,
                                                          int n, int lda, double* __restrict__ v, const double* __restrict__ vhi,
                                                          const double* __restrict__ vlo, int nv) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)n * lda;
  if (i < total) {
    const double a = hi[i] + lo[i];
    if (a != 0.0) M[i] += a;
  } else if (i - total < (size_t)nv) {
    const size_t k = i - total;
    const double a = vhi[k] + vlo[k];
    if (a != 0.0) v[k] += a;
  }
}

// frames / landmark of observation k; returns its kind
struct ObsRef {
  int kind, p, fj, fh, lm, dp;  // fh = -1 unless an inverse-depth point seen from another keyframe than its host
  bool same_host, lm_free;
};
__device__ inline ObsRef obs_ref(const GrLandmarks& G, int k) {
  ObsRef o;
  o.kind = G.obs_kind[k];
  o.p = G.obs_point[k];
  o.fj = G.obs_frame[k];
  const int h = o.kind == 1 ? G.idp_host[o.p] : o.fj;
  o.same_host = o.kind == 1 && h == o.fj;
  o.fh = (o.kind == 1 && h != o.fj) ? h : -1;
  o.lm = o.kind == 0 ? o.p : G.n_xyz + o.p;
  o.lm_free = o.kind == 0 ? (G.xyz_free ? G.xyz_free[o.p] != 0 : true) : (G.idp_free ? G.idp_free[o.p] != 0 : true);
  o.dp = o.lm_free ? (o.kind == 0 ? 3 : 1) : 0;
  return o;
}

template <bool WITH_J>
__device__ inline bool obs_eval(const GrLandmarks& G, const int32_t* dof, int k, const ObsRef& o, const double* S, const double* xyz,
                                const double* rho, double* r, double* w, double* s, double* Jj, double* Jh, double* Jp,
                                const double* cam_dev = nullptr, double* Jc = nullptr) {
  double Sj[8], Sh[8], lm[3] = {0, 0, 0}, anchor[3] = {0, 0, 0}, info[4];
  const int h = o.kind == 1 ? G.idp_host[o.p] : o.fj;
  for (int e = 0; e < 8; ++e) {
    Sj[e] = S[8 * (size_t)o.fj + e];
    Sh[e] = S[8 * (size_t)h + e];
  }
  if (o.kind == 0) {
    for (int e = 0; e < 3; ++e) lm[e] = xyz[3 * (size_t)o.p + e];
  } else {
    lm[0] = rho[o.p];
    for (int e = 0; e < 3; ++e) anchor[e] = G.idp_anchor[3 * (size_t)o.p + e];
  }
  if (G.obs_info)
    for (int e = 0; e < 4; ++e) info[e] = G.obs_info[4 * (size_t)k + e];
  const int ms = G.projection ? 3 : 2;
  const double m[3] = {G.obs_xy[ms * (size_t)k], G.obs_xy[ms * (size_t)k + 1], G.projection ? G.obs_xy[ms * (size_t)k + 2] : 1.0};
  double cam[9];
  if (G.with_cam)
    for (int e = 0; e < 9; ++e) cam[e] = cam_dev[e];
  return graph_obs<WITH_J>(o.kind, Sj, dof[o.fj], Sh, dof[h], o.same_host, lm, o.lm_free, anchor, m, G.obs_info ? info : nullptr,
                           G.huber, r, w, s, Jj, Jh, Jp, G.projection, G.with_cam ? cam : nullptr, G.cam_free, Jc);
}

// sum of one double per lane over the wave (every lane must take part), returned in every lane
__device__ inline double wave_add_f64(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(128) void gr_obs_lin_kernel(GrLandmarks G, const int32_t* __restrict__ dof, const double* __restrict__ S,
                                                         const double* __restrict__ xyz, const double* __restrict__ rho,
                                                         const double* __restrict__ cam, double* __restrict__ orec,
                                                         uint8_t* __restrict__ valid, double* __restrict__ H,
                                                         int lda, double* __restrict__ g, double* __restrict__ Hpp,
                                                         double* __restrict__ gp, double* __restrict__ cam_part,
                                                         unsigned long long* __restrict__ bound_bits) {
  const int k = blockIdx.x * 128 + threadIdx.x;
  const bool in_range = k < G.n_obs;
  if (!in_range && !G.with_cam) return;  // (with a camera every lane stays for the wave sums of the intrinsics block)
  double r[2] = {0, 0}, w = 0, s = 0, Jj[14], Jh[14], Jp[6], Jc[18], L[4] = {0, 0, 0, 0}, Lr[2] = {0, 0};
  for (int e = 0; e < 18; ++e) Jc[e] = 0.0;
  bool ok = false;
  ObsRef o;
  if (in_range) {
    o = obs_ref(G, k);
    ok = obs_eval<true>(G, dof, k, o, S, xyz, rho, r, &w, &s, Jj, Jh, Jp, cam, Jc);
    valid[k] = ok ? 1 : 0;
    double* R = orec + (size_t)G.rec * k;
    if (!ok) {
      for (int e = 0; e < G.rec; ++e) R[e] = 0.0;
      for (int e = 0; e < 18; ++e) Jc[e] = 0.0;
    } else {
      L[0] = L[3] = w;
      if (G.obs_info)
        for (int e = 0; e < 4; ++e) L[e] = w * G.obs_info[4 * (size_t)k + e];
      R[0] = r[0]; R[1] = r[1];
      for (int e = 0; e < 4; ++e) R[2 + e] = L[e];
      for (int e = 0; e < 14; ++e) { R[6 + e] = Jj[e]; R[20 + e] = Jh[e]; }
      for (int e = 0; e < 6; ++e) R[34 + e] = Jp[e];
      if (G.with_cam)
        for (int e = 0; e < 18; ++e) R[40 + e] = Jc[e];
      Lr[0] = L[0] * r[0] + L[1] * r[1];
      Lr[1] = L[2] * r[0] + L[3] * r[1];
      if (bound_bits != nullptr) {
        // reproducible mode: the bounds of the contributions this observation will make, per block it has a slot in and for
        // the right-hand sides (see DetAcc), and the landmark sums are left to gr_lm_sum_kernel (one thread per landmark, its
        // observations in list order)
        double jj = 0.0, jh = 0.0, jc = 0.0, lm = 0.0;
        for (int e = 0; e < 14; ++e) { jj = fmax(jj, fabs(Jj[e])); jh = fmax(jh, fabs(Jh[e])); }
        if (G.with_cam)
          for (int e = 0; e < 18; ++e) jc = fmax(jc, fabs(Jc[e]));
        for (int e = 0; e < 4; ++e) lm = fmax(lm, fabs(L[e]));
        bound_max(bound_bits + o.fj, 16.0 * lm * jj * jj);
        if (o.fh >= 0) bound_max(bound_bits + o.fh, 16.0 * lm * jh * jh);
        if (G.with_cam) bound_max(bound_bits + G.n_frames, 16.0 * lm * jc * jc);
        const double mx = fmax(fmax(jj, fmax(jh, jc)), fmax(fabs(r[0]), fabs(r[1])));
        bound_max(bound_bits + G.n_frames + 1, 16.0 * lm * mx * mx);
      }
      // (the keyframe rows of g and H are summed from the records by gr_frame_rows_kernel, seven consecutive words at a time)
      for (int a = 0; bound_bits == nullptr && a < o.dp; ++a) {
        atomicAdd(&gp[3 * (size_t)o.lm + a], Jp[a] * Lr[0] + Jp[3 + a] * Lr[1]);
        for (int b = 0; b < o.dp; ++b) {
          const double LJ0 = L[0] * Jp[b] + L[1] * Jp[3 + b], LJ1 = L[2] * Jp[b] + L[3] * Jp[3 + b];
          atomicAdd(&Hpp[9 * (size_t)o.lm + 3 * a + b], Jp[a] * LJ0 + Jp[3 + a] * LJ1);
        }
      }
    }
  }
  if (!G.with_cam) return;
  // intrinsics block: every observation adds to the same 9 + 45 words -> summed over the wave, the wave's 54 sums stored (no
  // atomics: from ~1000 waves the same-address atomics took twice as long as the rest of the kernel); gr_cam_fold_kernel adds
  // the partial sums up in wave order
  const bool lead = (threadIdx.x & 63) == 0;
  double* part = cam_part + (size_t)kCamPart * (blockIdx.x * 2 + (threadIdx.x >> 6));
  int slot = 0;
#pragma unroll
  for (int p = 0; p < 9; ++p) {
    const double gv = wave_add_f64(Jc[p] * Lr[0] + Jc[9 + p] * Lr[1]);  // (columns of fixed parameters are zero in the record)
    if (lead) part[slot] = gv;
    ++slot;
#pragma unroll
    for (int q = 0; q <= p; ++q) {
      const double LJ0 = L[0] * Jc[q] + L[1] * Jc[9 + q], LJ1 = L[2] * Jc[q] + L[3] * Jc[9 + q];
      const double hv = wave_add_f64(Jc[p] * LJ0 + Jc[9 + p] * LJ1);
      if (lead) part[slot] = hv;
      ++slot;
    }
  }
}

// g_c += sum of the waves' partial sums, block(c, c) += likewise: 16 threads per word, each over every 16th wave, then the 16
// partial sums of a word in order (a fixed order: reproducible)
__global__ __launch_bounds__(1024) void gr_cam_fold_kernel(const double* __restrict__ cam_part, int n_waves, int n_frames,
                                                           double* __restrict__ H, int lda, double* __restrict__ g) {
  __shared__ double sh[16][kCamPart];
  const int t = threadIdx.x;
  if (t < 16 * kCamPart) {
    const int j = t / kCamPart, w = t - j * kCamPart;
    double s = 0;
    for (int k = j; k < n_waves; k += 16) s += cam_part[(size_t)kCamPart * k + w];
    sh[j][w] = s;
  }
  __syncthreads();
  if (t >= kCamPart) return;
  double s = 0;
  for (int j = 0; j < 16; ++j) s += sh[j][t];
  // word t: the rows p = 0..8 one after the other, g_p first, then the columns q = 0..p of row p
  int p = 0, base = 0;
  while (base + p + 2 <= t) {
    base += p + 2;
    ++p;
  }
  const int cb = 7 * n_frames, q = t - base - 1;
  if (q < 0) g[cb + p] += s;
  else H[(size_t)(cb + q) * lda + cb + p] += s;
}

// Reproducible mode: H_pp and g_p of a landmark from the records of its observations, in list order, by one thread.
__global__ __launch_bounds__(256) void gr_lm_sum_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ orec,
                                                        double* __restrict__ Hpp, double* __restrict__ gp) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= G.n_xyz + G.n_idp) return;
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gv[3] = {0, 0, 0};
  for (int q = G.lstart[p]; q < G.lstart[p + 1]; ++q) {
    const int k = G.llist[q];
    if (!valid[k]) continue;
    const ObsRef o = obs_ref(G, k);
    const double* R = orec + (size_t)G.rec * k;
    const double* L = R + 2;
    const double* Jp = R + 34;
    const double Lr0 = L[0] * R[0] + L[1] * R[1], Lr1 = L[2] * R[0] + L[3] * R[1];
    for (int a = 0; a < o.dp; ++a) {
      gv[a] += Jp[a] * Lr0 + Jp[3 + a] * Lr1;
      for (int b = 0; b < o.dp; ++b) {
        const double LJ0 = L[0] * Jp[b] + L[1] * Jp[3 + b], LJ1 = L[2] * Jp[b] + L[3] * Jp[3 + b];
        h[3 * a + b] += Jp[a] * LJ0 + Jp[3 + a] * LJ1;
      }
    }
  }
  for (int e = 0; e < 9; ++e) Hpp[9 * (size_t)p + e] = h[e];
  for (int e = 0; e < 3; ++e) gp[3 * (size_t)p + e] = gv[e];
}

// Keyframe part of the normal equations from the observation records, EIGHT lanes per (observation, keyframe slot x), lane r
// = row r of the slot's blocks: g(f_x) += J_x^T L r, block(f_x, f_y) += J_x^T L J_y for the observation's slots with f_y <= f_x
// (lower triangle of blocks; inside a diagonal block rows r >= q: the solver reads nothing else), and with a camera the
// intrinsics rows x this keyframe's columns (the intrinsics block comes last: always the lower triangle).  Seven (nine)
// consecutive words per atomic instruction and slot: see gr_schur_kernel.
__global__ __launch_bounds__(256) void gr_frame_rows_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ orec,
                                                            double* __restrict__ H, int lda, double* __restrict__ g, DetAcc DA) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int sa = t >> 3, r = t & 7;
  const int k = sa >> 1, x = sa & 1;
  if (k >= G.n_obs || !valid[k]) return;
  const ObsRef o = obs_ref(G, k);
  const int fx = x == 0 ? o.fj : o.fh;
  if (fx < 0) return;
  const double* R = orec + (size_t)G.rec * k;
  const double L0 = R[2], L1 = R[3], L2 = R[4], L3 = R[5];
  const double* Jx = R + (x == 0 ? 6 : 20);
  if (r < 7) {
    const double j0 = Jx[r], j1 = Jx[7 + r];
    const double gv = j0 * (L0 * R[0] + L1 * R[1]) + j1 * (L2 * R[0] + L3 * R[1]);
    if (gv != 0.0) acc_add(g, DA.vhi, DA.vlo, (size_t)(7 * fx + r), gv, det_consts_vec(DA));
    for (int y = 0; y < 2; ++y) {
      const int fy = y == 0 ? o.fj : o.fh;
      if (fy < 0 || fy > fx) continue;
      const DetConst dc = det_consts_block(DA, fx, fy);
      const double* Jy = R + (y == 0 ? 6 : 20);
      const size_t col = (size_t)(7 * fy) * lda + 7 * fx + r;
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const double LJ0 = L0 * Jy[q] + L1 * Jy[7 + q], LJ1 = L2 * Jy[q] + L3 * Jy[7 + q];
        const double hv = j0 * LJ0 + j1 * LJ1;
        if (hv != 0.0 && (fy != fx || r >= q)) acc_add(H, DA.hi, DA.lo, col + (size_t)q * lda, hv, dc);
      }
    }
  }
  if (G.with_cam) {  // rows 0..7 of the intrinsics block by the eight lanes, row 8 by lane 0 again
    const double* Jc = R + 40;
    const double c0 = Jc[r], c1 = Jc[9 + r];
    const size_t col = (size_t)(7 * fx) * lda + 7 * G.n_frames;
    const DetConst dc = det_consts_block(DA, G.n_frames, fx);
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const double LJ0 = L0 * Jx[q] + L1 * Jx[7 + q], LJ1 = L2 * Jx[q] + L3 * Jx[7 + q];
      const double hv = c0 * LJ0 + c1 * LJ1;
      if (hv != 0.0) acc_add(H, DA.hi, DA.lo, col + (size_t)q * lda + r, hv, dc);
      if (r == 0) {
        const double h8 = Jc[8] * LJ0 + Jc[17] * LJ1;
        if (h8 != 0.0) acc_add(H, DA.hi, DA.lo, col + (size_t)q * lda + 8, h8, dc);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gr_gmax_kernel(const double* __restrict__ g, int n, const double* __restrict__ gp, int m,
                                                      unsigned long long* __restrict__ gmax_bits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v = 0;
  if (i < n) v = fabs(g[i]);
  else if (i < n + m) v = fabs(gp[i - n]);
  if (v > 0) atomicMax(gmax_bits, (unsigned long long)__double_as_longlong(v));
}

// (H_pp + D)^-1 per landmark; lmdim = 0 for a landmark that is fixed or has no valid observation
// Also, for an inverse-depth landmark: every observation from another keyframe has a slot in the HOST keyframe; those
// are summed into one (Wh = sum of their W, a 7-vector since the landmark is a scalar) represented by the first of them
// (hrep), so that the Schur product sees one host slot per landmark instead of one per observation.
__global__ __launch_bounds__(256) void gr_lm_prepare_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ Hpp,
                                                            const double* __restrict__ orec, double radius, double* __restrict__ Hinv,
                                                            int32_t* __restrict__ lmdim, double* __restrict__ Wh,
                                                            int32_t* __restrict__ hrep, double* __restrict__ Wc) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= G.n_xyz + G.n_idp) return;
  int dp = 0, rep = -1;
  double wh[7] = {0, 0, 0, 0, 0, 0, 0};
  // with a camera: the landmark's coupling to the intrinsics, W_c = sum over its observations of J_c^T L J_p (9 x 3) --
  // one slot per landmark in the Schur product (gr_schur_cam_kernel)
  double wc[27];
  for (int e = 0; e < 27; ++e) wc[e] = 0.0;
  for (int q = G.lstart[p]; q < G.lstart[p + 1]; ++q) {
    const int k = G.llist[q];
    if (valid[k]) {
      const ObsRef o = obs_ref(G, k);
      dp = o.dp > dp ? o.dp : dp;
      if (o.fh >= 0 && o.dp == 1) {
        if (rep < 0) rep = k;
        const double* R = orec + (size_t)G.rec * k;
        const double* L = R + 2;
        const double LJ0 = L[0] * R[34] + L[1] * R[37], LJ1 = L[2] * R[34] + L[3] * R[37];
        for (int r7 = 0; r7 < 7; ++r7) wh[r7] += R[20 + r7] * LJ0 + R[27 + r7] * LJ1;
      }
      if (G.with_cam && o.dp > 0) {
        const double* R = orec + (size_t)G.rec * k;
        const double* L = R + 2;
        for (int b = 0; b < o.dp; ++b) {
          const double LJ0 = L[0] * R[34 + b] + L[1] * R[37 + b], LJ1 = L[2] * R[34 + b] + L[3] * R[37 + b];
          for (int r9 = 0; r9 < 9; ++r9) wc[3 * r9 + b] += R[40 + r9] * LJ0 + R[49 + r9] * LJ1;
        }
      }
    }
  }
  if (G.with_cam)
    for (int e = 0; e < 27; ++e) Wc[27 * (size_t)p + e] = wc[e];
  lmdim[p] = dp;
  hrep[p] = rep;
  for (int r7 = 0; r7 < 7; ++r7) Wh[7 * (size_t)p + r7] = wh[r7];
  double Hi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (dp) {
    double Hp[9];
    for (int e = 0; e < 9; ++e) Hp[e] = Hpp[9 * (size_t)p + e];
    for (int a = 0; a < dp; ++a) {
      const double v = Hp[4 * a];
      Hp[4 * a] += (v < 1e-6 ? 1e-6 : (v > 1e32 ? 1e32 : v)) / radius;
    }
    if (dp == 1) {
      Hi[0] = 1.0 / Hp[0];
    } else {
      const double a = Hp[0], b = Hp[1], c = Hp[2], d = Hp[4], e = Hp[5], f = Hp[8];
      const double A = d * f - e * e, B = c * e - b * f, C = b * e - c * d;
      const double id = 1.0 / (a * A + b * B + c * C);
      Hi[0] = A * id; Hi[1] = B * id; Hi[2] = C * id;
      Hi[3] = B * id; Hi[4] = (a * f - c * c) * id; Hi[5] = (b * c - a * e) * id;
      Hi[6] = C * id; Hi[7] = Hi[5]; Hi[8] = (a * d - b * b) * id;
    }
  }
  for (int e = 0; e < 9; ++e) Hinv[9 * (size_t)p + e] = Hi[e];
}

// W = J_f^T L J_p (7 x 3, columns >= dp zero) of slot x (0: observing keyframe, 1: host) of a recorded observation
__device__ inline void slot_W(const double* R, int x, int dp, double* W) {
  const double* L = R + 2;
  const double* Jf = R + (x == 0 ? 6 : 20);
  const double* Jp = R + 34;
  for (int b = 0; b < 3; ++b) {
    const double LJ0 = L[0] * Jp[b] + L[1] * Jp[3 + b], LJ1 = L[2] * Jp[b] + L[3] * Jp[3 + b];
    for (int r7 = 0; r7 < 7; ++r7) W[3 * r7 + b] = b < dp ? Jf[r7] * LJ0 + Jf[7 + r7] * LJ1 : 0.0;
  }
}

// Row r7 of W = J_f^T L J_p (columns >= dp zero) of slot x of a recorded observation, straight from the record
__device__ __forceinline__ void slot_W_row(const double* R, int x, int dp, int r7, double* w) {
  const double* L = R + 2;
  const double* Jf = R + (x == 0 ? 6 : 20);
  const double* Jp = R + 34;
  const double j0 = Jf[r7], j1 = Jf[7 + r7];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const double LJ0 = L[0] * Jp[b] + L[1] * Jp[3 + b], LJ1 = L[2] * Jp[b] + L[3] * Jp[3 + b];
    w[b] = b < dp ? j0 * LJ0 + j1 * LJ1 : 0.0;
  }
}

// EIGHT lanes per (observation, keyframe) slot a, lane r < 7 = row r of U_a = W_a (H_pp + D)^-1: an atomic instruction then
// adds seven CONSECUTIVE words of a block column per slot.  f64 atomics resolve at the memory side and are bound by 64-byte
// sector requests, not by lanes (tools/atomic_probe.hip: 23.6 G lane-atomics/s scattered, 160 G/s in runs of seven), so the
// 7 x 7 block of a slot pair costs 7 requests instead of 49.  No local arrays: everything is read from the records by index.
__global__ __launch_bounds__(256) void gr_schur_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ orec,
                                                       const double* __restrict__ Hinv, const int32_t* __restrict__ lmdim,
                                                       const double* __restrict__ Wh, const int32_t* __restrict__ hrep,
                                                       const double* __restrict__ gp, double* __restrict__ Hd, int lda,
                                                       double* __restrict__ d, DetAcc DA) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int sa = t >> 3, r = t & 7;
  const int ka = sa >> 1, x = sa & 1;
  if (r == 7 || ka >= G.n_obs || !valid[ka]) return;
  const ObsRef oa = obs_ref(G, ka);
  const int fa = x == 0 ? oa.fj : oa.fh;
  if (fa < 0) return;
  const int dp = lmdim[oa.lm];
  if (!dp) return;
  const int rep = hrep[oa.lm];
  if (x == 1 && ka != rep) return;  // the landmark's host slots are one slot, carried by their first observation
  double wa[3], ua[3];
  if (x == 1) {
    wa[0] = Wh[7 * (size_t)oa.lm + r];
    wa[1] = wa[2] = 0.0;
  } else {
    slot_W_row(orec + (size_t)G.rec * ka, x, dp, r, wa);
  }
  const double* Hi = Hinv + 9 * (size_t)oa.lm;
#pragma unroll
  for (int b = 0; b < 3; ++b) ua[b] = wa[0] * Hi[b] + wa[1] * Hi[3 + b] + wa[2] * Hi[6 + b];
  {
    const double v = ua[0] * gp[3 * (size_t)oa.lm] + ua[1] * gp[3 * (size_t)oa.lm + 1] + ua[2] * gp[3 * (size_t)oa.lm + 2];
    if (v != 0.0) acc_add(d, DA.vhi, DA.vlo, (size_t)(7 * fa + r), v, det_consts_vec(DA));
  }
  for (int q = G.lstart[oa.lm]; q < G.lstart[oa.lm + 1]; ++q) {
    const int kb = G.llist[q];
    if (!valid[kb]) continue;
    const ObsRef ob = obs_ref(G, kb);
    for (int y = 0; y < 2; ++y) {
      const int fb = y == 0 ? ob.fj : ob.fh;
      if (fb < 0 || fb > fa || (y == 1 && kb != rep)) continue;  // lower triangle of blocks
      // (equal frames: the two orders (a, b) and (b, a) are transposes of each other, so their lower triangles add up to the
      //  lower triangle of the symmetric sum -- the solver reads nothing else)
      const double* Rb = orec + (size_t)G.rec * kb;
      const size_t col = (size_t)(7 * fb) * lda + 7 * fa + r;
      const DetConst dc = det_consts_block(DA, fa, fb);
#pragma unroll
      for (int c7 = 0; c7 < 7; ++c7) {
        double wb[3];
        if (y == 1) {
          wb[0] = Wh[7 * (size_t)oa.lm + c7];
          wb[1] = wb[2] = 0.0;
        } else {
          slot_W_row(Rb, 0, dp, c7, wb);
        }
        const double v = ua[0] * wb[0] + ua[1] * wb[1] + ua[2] * wb[2];
        if (v != 0.0 && (fb != fa || r >= c7)) acc_add(Hd, DA.hi, DA.lo, col + (size_t)c7 * lda, -v, dc);
      }
    }
  }
}

// The intrinsics' slot of the Schur product, SIXTEEN lanes per observation, lane r < 9 = row r of U_c = W_c (H_pp + D)^-1
// (9 x 3) of the observation's landmark: block(c, f) -= U_c W_f^T for the observation's keyframe slots (the intrinsics rows are
// the last rows: always the lower triangle), nine consecutive words per slot and atomic instruction (see gr_schur_kernel).
__global__ __launch_bounds__(256) void gr_schur_cam_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ orec,
                                                           const double* __restrict__ Hinv, const int32_t* __restrict__ lmdim,
                                                           const double* __restrict__ Wh, const int32_t* __restrict__ hrep,
                                                           const double* __restrict__ Wc, double* __restrict__ Hd, int lda, DetAcc DA) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int kb = t >> 4, r = t & 15;
  double ua[3];
  const int cb = 7 * G.n_frames;
  if (kb < G.n_obs && r < 9 && valid[kb]) {
    const ObsRef ob = obs_ref(G, kb);
    const int p = ob.lm, dp = lmdim[p];
    if (dp) {
      const double* Hi = Hinv + 9 * (size_t)p;
      const double* Wp = Wc + 27 * (size_t)p;
      const double w0 = Wp[3 * r], w1 = Wp[3 * r + 1], w2 = Wp[3 * r + 2];
#pragma unroll
      for (int b = 0; b < 3; ++b) ua[b] = w0 * Hi[b] + w1 * Hi[3 + b] + w2 * Hi[6 + b];
      const int rep = hrep[p];
      for (int y = 0; y < 2; ++y) {
        const int fb = y == 0 ? ob.fj : ob.fh;
        if (fb < 0 || (y == 1 && kb != rep)) continue;
        const double* Rb = orec + (size_t)G.rec * kb;
        const size_t col = (size_t)(7 * fb) * lda + cb + r;
        const DetConst dc = det_consts_block(DA, G.n_frames, fb);
#pragma unroll
        for (int c7 = 0; c7 < 7; ++c7) {
          double wb[3];
          if (y == 1) {
            wb[0] = Wh[7 * (size_t)p + c7];
            wb[1] = wb[2] = 0.0;
          } else {
            slot_W_row(Rb, 0, dp, c7, wb);
          }
          const double v = ua[0] * wb[0] + ua[1] * wb[1] + ua[2] * wb[2];
          if (v != 0.0) acc_add(Hd, DA.hi, DA.lo, col + (size_t)c7 * lda, -v, dc);
        }
      }
    }
  }
}

// ... and the landmark's own part, one thread per landmark: rhs_c += U_c g_p, block(c, c) -= U_c W_c^T.  Every landmark adds to
// the same 9 + 45 words: summed over the wave first, one atomic per wave and word (188 waves for 12 000 landmarks; issued
// from the per-observation kernel above, the same-address atomics of 15 000 waves took 0.9 ms).
__global__ __launch_bounds__(128) void gr_schur_cam_cc_kernel(GrLandmarks G, const double* __restrict__ Hinv, const int32_t* __restrict__ lmdim,
                                                              const double* __restrict__ Wc, const double* __restrict__ gp,
                                                              double* __restrict__ Hd, int lda, double* __restrict__ d, DetAcc DA) {
  const int p = blockIdx.x * 128 + threadIdx.x;
  const int nlm = G.n_xyz + G.n_idp;
  const DetConst dc = det_consts_block(DA, G.n_frames, G.n_frames), dv = det_consts_vec(DA);
  double W[27], U[27];
#pragma unroll
  for (int e = 0; e < 27; ++e) W[e] = U[e] = 0.0;
  double g0 = 0, g1 = 0, g2 = 0;
  if (p < nlm && lmdim[p] != 0) {
    double Hi[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Hi[e] = Hinv[9 * (size_t)p + e];
#pragma unroll
    for (int e = 0; e < 27; ++e) W[e] = Wc[27 * (size_t)p + e];
#pragma unroll
    for (int r9 = 0; r9 < 9; ++r9)
#pragma unroll
      for (int b = 0; b < 3; ++b) U[3 * r9 + b] = W[3 * r9] * Hi[b] + W[3 * r9 + 1] * Hi[3 + b] + W[3 * r9 + 2] * Hi[6 + b];
    g0 = gp[3 * (size_t)p]; g1 = gp[3 * (size_t)p + 1]; g2 = gp[3 * (size_t)p + 2];
  }
  const int cb = 7 * G.n_frames;
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int r9 = 0; r9 < 9; ++r9) {
    if (!((G.cam_free >> r9) & 1)) continue;
    const double v = wave_add_f64(U[3 * r9] * g0 + U[3 * r9 + 1] * g1 + U[3 * r9 + 2] * g2);
    if (lead && v != 0.0) acc_add(d, DA.vhi, DA.vlo, (size_t)(cb + r9), v, dv);
#pragma unroll
    for (int c9 = 0; c9 <= r9; ++c9) {
      if (!((G.cam_free >> c9) & 1)) continue;
      const double h = wave_add_f64(U[3 * r9] * W[3 * c9] + U[3 * r9 + 1] * W[3 * c9 + 1] + U[3 * r9 + 2] * W[3 * c9 + 2]);
      if (lead && h != 0.0) acc_add(Hd, DA.hi, DA.lo, (size_t)(cb + c9) * lda + cb + r9, -h, dc);
    }
  }
}

__global__ __launch_bounds__(256) void gr_backsub_kernel(GrLandmarks G, const uint8_t* __restrict__ valid, const double* __restrict__ orec,
                                                         const double* __restrict__ Hinv, const int32_t* __restrict__ lmdim,
                                                         const double* __restrict__ gp, const double* __restrict__ d,
                                                         double* __restrict__ dlm) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= G.n_xyz + G.n_idp) return;
  const int dp = lmdim[p];
  double out[3] = {0, 0, 0};
  if (dp) {
    double t[3] = {gp[3 * (size_t)p], gp[3 * (size_t)p + 1], gp[3 * (size_t)p + 2]};
    for (int q = G.lstart[p]; q < G.lstart[p + 1]; ++q) {
      const int k = G.llist[q];
      if (!valid[k]) continue;
      const ObsRef o = obs_ref(G, k);
      const double* R = orec + (size_t)G.rec * k;
      const double* L = R + 2;
      const double* Jp = R + 34;
      for (int x = 0; x < 2; ++x) {
        const int f = x == 0 ? o.fj : o.fh;
        if (f < 0) continue;
        const double* Jf = R + (x == 0 ? 6 : 20);
        double Jd0 = 0, Jd1 = 0;
        for (int c = 0; c < 7; ++c) {
          Jd0 += Jf[c] * d[7 * f + c];
          Jd1 += Jf[7 + c] * d[7 * f + c];
        }
        const double LJd0 = L[0] * Jd0 + L[1] * Jd1, LJd1 = L[2] * Jd0 + L[3] * Jd1;
        for (int b = 0; b < o.dp; ++b) t[b] += Jp[b] * LJd0 + Jp[3 + b] * LJd1;
      }
      if (G.with_cam) {
        double Jd0 = 0, Jd1 = 0;
        for (int c = 0; c < 9; ++c) {
          Jd0 += R[40 + c] * d[7 * G.n_frames + c];
          Jd1 += R[49 + c] * d[7 * G.n_frames + c];
        }
        const double LJd0 = L[0] * Jd0 + L[1] * Jd1, LJd1 = L[2] * Jd0 + L[3] * Jd1;
        for (int b = 0; b < o.dp; ++b) t[b] += Jp[b] * LJd0 + Jp[3 + b] * LJd1;
      }
    }
    const double* Hi = Hinv + 9 * (size_t)p;
    for (int a = 0; a < dp; ++a) out[a] = -(Hi[3 * a] * t[0] + Hi[3 * a + 1] * t[1] + Hi[3 * a + 2] * t[2]);
  }
  for (int a = 0; a < 3; ++a) dlm[3 * (size_t)p + a] = out[a];
}

// model-decrease terms: items [0, n_edges) pose edges (from the pg_edge record), then the observations
__global__ __launch_bounds__(256) void gr_model_kernel(PgGraph P, GrLandmarks G, const double* __restrict__ erec, const uint8_t* __restrict__ valid,
                                                       const double* __restrict__ orec, const double* __restrict__ d,
                                                       const double* __restrict__ dlm, double* __restrict__ term) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < P.n_edges) {
    const double* R = erec + (size_t)kEdgeRec * i;
    const int fi = P.ei[i], fj = P.ej[i];
    double lin = 0, quad = 0;
    for (int p = 0; p < 7; ++p) {
      const double dip = d[7 * fi + p], djp = fj >= 0 ? d[7 * fj + p] : 0.0;
      lin += R[147 + p] * dip + (fj >= 0 ? R[154 + p] * djp : 0.0);
      for (int q = 0; q < 7; ++q) {
        const double diq = d[7 * fi + q];
        quad += dip * R[7 * p + q] * diq;
        if (fj >= 0) quad += djp * R[49 + 7 * p + q] * d[7 * fj + q] + 2.0 * djp * R[98 + 7 * p + q] * diq;
      }
    }
    term[i] = -(lin + 0.5 * quad);
    return;
  }
  const int k = i - P.n_edges;
  if (k >= G.n_obs) return;
  double out = 0;
  if (valid[k]) {
    const ObsRef o = obs_ref(G, k);
    const double* R = orec + (size_t)G.rec * k;
    const double* L = R + 2;
    double Jd0 = 0, Jd1 = 0;
    for (int q = 0; q < 7; ++q) {
      Jd0 += R[6 + q] * d[7 * o.fj + q];
      Jd1 += R[13 + q] * d[7 * o.fj + q];
      if (o.fh >= 0) {
        Jd0 += R[20 + q] * d[7 * o.fh + q];
        Jd1 += R[27 + q] * d[7 * o.fh + q];
      }
    }
    if (G.with_cam)
      for (int q = 0; q < 9; ++q) {
        Jd0 += R[40 + q] * d[7 * G.n_frames + q];
        Jd1 += R[49 + q] * d[7 * G.n_frames + q];
      }
    for (int b = 0; b < o.dp; ++b) {
      Jd0 += R[34 + b] * dlm[3 * (size_t)o.lm + b];
      Jd1 += R[37 + b] * dlm[3 * (size_t)o.lm + b];
    }
    const double LJd0 = L[0] * Jd0 + L[1] * Jd1, LJd1 = L[2] * Jd0 + L[3] * Jd1;
    const double Lr0 = L[0] * R[0] + L[1] * R[1], Lr1 = L[2] * R[0] + L[3] * R[1];
    out = -((Jd0 * Lr0 + Jd1 * Lr1) + 0.5 * (Jd0 * LJd0 + Jd1 * LJd1));
  }
  term[i] = out;
}

__global__ __launch_bounds__(256) void gr_update_kernel(int n_xyz, int n_idp, const double* __restrict__ xyz, const double* __restrict__ rho,
                                                        const double* __restrict__ dlm, double* __restrict__ xyz_new,
                                                        double* __restrict__ rho_new, const double* __restrict__ cam,
                                                        const double* __restrict__ d_cam, int cam_free, double* __restrict__ cam_new) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (cam != nullptr && p < 9) cam_new[p] = cam[p] + (((cam_free >> p) & 1) ? d_cam[p] : 0.0);  // (d_cam = the step's intrinsics rows)
  if (p < n_xyz) {
    for (int a = 0; a < 3; ++a) xyz_new[3 * (size_t)p + a] = xyz[3 * (size_t)p + a] + dlm[3 * (size_t)p + a];
  } else if (p < n_xyz + n_idp) {
    const double v = rho[p - n_xyz] + dlm[3 * (size_t)p];
    rho_new[p - n_xyz] = v > 1e-9 ? v : 1e-9;
  }
}

// robust cost of every observation at a candidate (1/2 rho(s)); an observation that was valid at the linearisation point
// (was_valid) and is not any more makes the candidate infinitely bad
__global__ __launch_bounds__(128) void gr_cost_kernel(GrLandmarks G, const int32_t* __restrict__ dof, const double* __restrict__ S,
                                                      const double* __restrict__ xyz, const double* __restrict__ rho,
                                                      const double* __restrict__ cam, const uint8_t* __restrict__ was_valid,
                                                      double* __restrict__ cost_o) {
  const int k = blockIdx.x * 128 + threadIdx.x;
  if (k >= G.n_obs) return;
  const ObsRef o = obs_ref(G, k);
  double r[2], w, s;
  double c = 0;
  if (obs_eval<false>(G, dof, k, o, S, xyz, rho, r, &w, &s, nullptr, nullptr, nullptr, cam)) {
    c = 0.5 * ((G.huber > 0 && s > G.huber * G.huber) ? 2.0 * G.huber * sqrt(s) - G.huber * G.huber : s);
  } else if (was_valid && was_valid[k]) {
    c = INFINITY;
  }
  cost_o[k] = c;
}

// fixed-order sum: each block adds 1024 consecutive values (thread t: 4 in order, then a fixed tree), one partial per block
__global__ __launch_bounds__(256) void gr_reduce_kernel(const double* __restrict__ v, int n, double* __restrict__ partial) {
  __shared__ double sh[256];
  const int base = blockIdx.x * 1024 + threadIdx.x * 4;
  double s = 0;
  for (int e = 0; e < 4; ++e)
    if (base + e < n) s += v[base + e];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// ---------------------------------------------------------------- gh_graph_solve: the host side, phase by phase
// Sizes and switches of one solve.
struct GraphShape {
  int nf = 0, nx = 0, ni = 0, no = 0, nlm = 0, ms = 2;  // keyframes, XYZ / inverse-depth points, observations; doubles per measurement
  bool with_cam = false;                                // free intrinsics: they follow the keyframes in the reduced system
  int n = 0, lda = 0, rec = kObsRec;
  int ne = 0, n_pairs = 0;  // pose edges and their distinct frame pairs (PoseHost)
  bool sparse = false;      // block-sparse linear solver (graph_plan_sparse)
  bool det = false;         // reproducible accumulation of the landmark part (DetAcc)
  explicit GraphShape(const gh_graph_problem* gpr)
      : nf(gpr->pg.n_frames), nx(gpr->n_xyz), ni(gpr->n_idp), no(gpr->n_obs), nlm(nx + ni), ms(gpr->projection ? 3 : 2),
        with_cam(gpr->intrinsics != nullptr && no > 0), n(7 * nf + (with_cam ? 9 : 0)),
        lda((n + 1 + 15) & ~15),  // one spare row: the right-hand side rides through the factorisation (gh_potrf_solve_dev)
        rec(with_cam ? kObsRecCam : kObsRec) {}
  size_t nlm1() const { return (size_t)std::max(nlm, 1); }
  size_t no1() const { return (size_t)std::max(no, 1); }
  size_t nx1() const { return (size_t)std::max(nx, 1); }
  size_t ni1() const { return (size_t)std::max(ni, 1); }
  int n_items() const { return ne + no; }  // terms of the model decrease: pose edges, then observations
  int n_part() const { return gh_div_up(std::max(n_items(), std::max(no, 1)), 1024); }
  int eb() const { return gh_div_up(ne > 0 ? ne : 1, 64); }
  int eb4() const { return gh_div_up(ne > 0 ? ne : 1, 4); }
  int ob() const { return gh_div_up(no > 0 ? no : 1, 128); }  // workgroups of gr_obs_lin (two waves each)
};

// What the host builds from the problem before anything is allocated.
struct GraphHost {
  PoseHost PH;
  std::vector<int32_t> lstart, llist;  // observations grouped by landmark (XYZ points first), in observation order
  std::vector<int64_t> bs_off;         // block-sparse address tables: where pg_assemble_bs stores each block (BsDest)
  std::vector<int32_t> bs_sp, bs_sq;
};

// Everything the host reads back inside the loop lands in the context's pinned block: plain DMAs, no staged copies into
// pageable memory.
struct GraphReadback {
  double out4[4];
  unsigned long long gmax_bits;
  int info;
  int32_t bs_flag;
};

// The device arrays of one solve.  The arena places each array by the ORDER of alloc(): the uploaded arrays first, so
// that they form one run of the arena and travel in one DMA; then the lists of the block-sparse solver (the same way),
// then the work arrays.
struct GraphDev {
  // uploaded: pose graph
  double *S = nullptr, *meas = nullptr, *info = nullptr;
  int32_t *dof = nullptr, *etype = nullptr, *ei = nullptr, *ej = nullptr, *vstart = nullptr, *vlist = nullptr, *pstart = nullptr,
          *plist = nullptr, *prow = nullptr, *pcol = nullptr;
  // uploaded: landmarks
  double *xyz = nullptr, *rho = nullptr, *anchor = nullptr, *oxy = nullptr, *oinfo = nullptr, *cam = nullptr;
  int32_t *host = nullptr, *okind = nullptr, *opoint = nullptr, *oframe = nullptr, *lstart = nullptr, *llist = nullptr;
  uint8_t *xfree = nullptr, *ifree = nullptr;
  // uploaded: block-sparse address tables
  int64_t* bs_off = nullptr;
  int32_t *bs_sp = nullptr, *bs_sq = nullptr;
  // work arrays
  double *Snew = nullptr, *rec = nullptr, *cost_e = nullptr, *g = nullptr, *d = nullptr, *out = nullptr, *xyz_new = nullptr,
         *rho_new = nullptr, *orec = nullptr, *Hpp = nullptr, *gp = nullptr, *Hinv = nullptr, *dlm = nullptr, *term = nullptr,
         *part = nullptr, *Wh = nullptr, *cam_new = nullptr, *Wc = nullptr, *cam_part = nullptr, *H = nullptr, *Hd = nullptr;
  unsigned long long* gmax = nullptr;
  int32_t *lmdim = nullptr, *hrep = nullptr;
  uint8_t* valid = nullptr;
  // DetAcc: two matrix-shaped and two vector-shaped accumulators, the bound
  double *acc_hi = nullptr, *acc_lo = nullptr, *vacc = nullptr;
  unsigned long long* bound = nullptr;

  // Run twice (graph_arena.h): once measuring, once for real.  An uploaded array is allocated and its upload noted (real
  // pass) in ONE statement, so the order of the uploads is the order of the allocations by construction.
  bool alloc(GraphArena& A, const GraphShape& Z, const gh_graph_problem* gpr, const GraphHost& Hh, BsSolver& BS) {
    const gh_pg_problem* pr = &gpr->pg;
    const PoseHost& PH = Hh.PH;
    const size_t nf = (size_t)Z.nf, nx = (size_t)Z.nx, ni = (size_t)Z.ni, no = (size_t)Z.no, n = (size_t)Z.n;
    const size_t nx1 = Z.nx1(), ni1 = Z.ni1(), no1 = Z.no1(), nlm1 = Z.nlm1(), ne1 = PH.etype.size(), nn = n * Z.lda;
    // room elements of *arr, the first `count` of them uploaded from src
    auto up = [&A](auto** arr, size_t room, const void* src, size_t count) -> bool {
      if (!A.alloc(arr, room)) return false;
      if (!A.measuring) A.upload(*arr, src, count * sizeof(**arr));
      return true;
    };
    auto upv = [&up](auto** arr, const auto& v) -> bool { return up(arr, v.size(), v.data(), v.size()); };
    // the block-sparse solver's own lists: allocated there, their uploads noted behind the tables' (real pass)
    auto bs_lists = [&A, &BS]() -> bool {
      if (!BS.alloc_dev(A)) return false;
      if (!A.measuring) BS.note_uploads(A);
      return true;
    };
    return up(&S, nf * 8, pr->frame_sim3, nf * 8) && up(&dof, nf, pr->frame_dof, nf) && upv(&meas, PH.meas) &&
           (!PH.any_info || upv(&info, PH.info)) && upv(&etype, PH.etype) && upv(&ei, PH.ei) && upv(&ej, PH.ej) &&
           upv(&vstart, PH.vstart) && upv(&vlist, PH.vlist) && upv(&pstart, PH.pstart) && upv(&plist, PH.plist) &&
           upv(&prow, PH.prow) && upv(&pcol, PH.pcol) &&
           // landmarks
           up(&xyz, nx1 * 3, gpr->xyz, nx * 3) && up(&rho, ni1, gpr->idp_rho, ni) && up(&anchor, ni1 * 3, gpr->idp_anchor, ni * 3) &&
           up(&host, ni1, gpr->idp_host, ni) && up(&oxy, no1 * 3, gpr->projection ? gpr->obs_bearing : gpr->obs_xy, no * Z.ms) &&
           (!gpr->obs_info || up(&oinfo, no1 * 4, gpr->obs_info, no * 4)) && up(&okind, no1, gpr->obs_kind, no) &&
           up(&opoint, no1, gpr->obs_point, no) && up(&oframe, no1, gpr->obs_frame, no) && upv(&lstart, Hh.lstart) &&
           upv(&llist, Hh.llist) && (!gpr->xyz_free || up(&xfree, nx1, gpr->xyz_free, nx)) &&
           (!gpr->idp_free || up(&ifree, ni1, gpr->idp_free, ni)) && (!Z.with_cam || up(&cam, 9, gpr->intrinsics, 9)) &&
           // block-sparse tables, then the solver's own lists
           (!Z.sparse || (upv(&bs_off, Hh.bs_off) && upv(&bs_sp, Hh.bs_sp) && upv(&bs_sq, Hh.bs_sq) && bs_lists())) &&
           // work arrays
           A.alloc(&Snew, nf * 8) && A.alloc(&rec, (size_t)kEdgeRec * ne1) && A.alloc(&cost_e, ne1) && A.alloc(&g, n) &&
           A.alloc(&d, n) && A.alloc(&out, 4) && A.alloc(&gmax, 1) && A.alloc(&xyz_new, nx1 * 3) && A.alloc(&rho_new, ni1) &&
           A.alloc(&orec, no1 * Z.rec) && A.alloc(&Hpp, nlm1 * 9) && A.alloc(&gp, nlm1 * 3) && A.alloc(&Hinv, nlm1 * 9) &&
           A.alloc(&dlm, nlm1 * 3) && A.alloc(&term, (size_t)std::max(Z.n_items(), 1)) && A.alloc(&part, (size_t)Z.n_part()) &&
           A.alloc(&lmdim, nlm1) && A.alloc(&hrep, nlm1) && A.alloc(&Wh, nlm1 * 7) && A.alloc(&valid, no1) &&
           (!Z.with_cam || (A.alloc(&cam_new, 9) && A.alloc(&Wc, nlm1 * 27) && A.alloc(&cam_part, (size_t)kCamPart * 2 * Z.ob()))) &&
           (Z.sparse || (A.alloc(&H, nn) && A.alloc(&Hd, nn))) &&
           // DetAcc
           (!Z.det || (A.alloc(&acc_hi, nn) && A.alloc(&acc_lo, nn) && A.alloc(&vacc, 2 * n) && A.alloc(&bound, nf + 2)));
  }
};

// One solve: what its phases share.
struct GraphRun {
  GraphShape Z;
  GraphDev D;
  BsSolver BS;
  PgGraph G;
  PgLists Ls;
  GrLandmarks LM;
  DetAcc DA{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  GraphReadback* rb = nullptr;
  explicit GraphRun(const gh_graph_problem* gpr) : Z(gpr) {}
};

// State of the LM loop across iterations (cost, radius, decrease, term: lm_rule.h).
struct GraphLoop : LmRule {
  bool need_lin = true;
  bool fresh_gmax = false;  // a gradient maximum is on its way to the host: tested behind the solve's synchronisation
};

gh_status graph_check_problem(gh_ctx* ctx, const gh_graph_problem* gpr, const GraphShape& Z) {
  const gh_pg_problem* pr = &gpr->pg;
  const int nf = Z.nf, nx = Z.nx, ni = Z.ni, no = Z.no;
  GH_CHECK_ARG(ctx, nf >= 1 && nf <= (1 << 20) && pr->frame_sim3 && pr->frame_dof && pr->n_se3 >= 0 && pr->n_sim3 >= 0 && pr->n_gps >= 0);
  GH_CHECK_ARG(ctx, pr->n_se3 == 0 || (pr->se3_first && pr->se3_second && pr->se3_meas));
  GH_CHECK_ARG(ctx, pr->n_sim3 == 0 || (pr->sim3_first && pr->sim3_second && pr->sim3_meas));
  GH_CHECK_ARG(ctx, pr->n_gps == 0 || (pr->gps_frame && pr->gps_meas));
  GH_CHECK_ARG(ctx, no <= (1 << 26));  // (sixteen lanes per observation in the Schur kernels: 32-bit thread indices)
  GH_CHECK_ARG(ctx, nx >= 0 && ni >= 0 && no >= 0 && (nx == 0 || gpr->xyz) && (ni == 0 || (gpr->idp_host && gpr->idp_anchor && gpr->idp_rho)));
  GH_CHECK_ARG(ctx, gpr->projection == 0 || gpr->projection == 1);
  // camera self-calibration (BundleGraph::camera + cameraDOF): pixels through the camera model, pinhole projection only
  if (gpr->intrinsics) {
    if (gpr->projection != 0) return gh_set_error(ctx, GH_ERR_ARG, "gh_graph_solve: intrinsics need the pinhole projection");
    GH_CHECK_ARG(ctx, gpr->intrinsics[0] != 0.0 && gpr->intrinsics[1] != 0.0 && (gpr->intrinsics_free & ~0x1FF) == 0);
  }
  GH_CHECK_ARG(ctx, no == 0 || (gpr->obs_kind && gpr->obs_point && gpr->obs_frame && (gpr->projection ? gpr->obs_bearing : gpr->obs_xy)));
  for (int f = 0; f < nf; ++f) GH_CHECK_ARG(ctx, pr->frame_sim3[8 * (size_t)f + 7] > 0);
  for (int p = 0; p < ni; ++p) GH_CHECK_ARG(ctx, gpr->idp_host[p] >= 0 && gpr->idp_host[p] < nf && gpr->idp_rho[p] > 0);
  return GH_OK;
}

// The per-observation range check.  It runs after the pose-edge lists are built, where it always ran: an input with a bad edge
// and a bad observation is refused for the edge, and total_ms covers this loop.
gh_status graph_check_observations(gh_ctx* ctx, const gh_graph_problem* gpr, const GraphShape& Z) {
  for (int k = 0; k < Z.no; ++k) {
    const int kind = gpr->obs_kind[k], p = gpr->obs_point[k], f = gpr->obs_frame[k];
    GH_CHECK_ARG(ctx, (kind == 0 || kind == 1) && p >= 0 && p < (kind == 0 ? Z.nx : Z.ni) && f >= 0 && f < Z.nf);
  }
  return GH_OK;
}

void graph_landmark_lists(const gh_graph_problem* gpr, const GraphShape& Z, GraphHost& Hh) {
  const int nx = Z.nx, no = Z.no;
  Hh.lstart.assign((size_t)Z.nlm + 2, 0);
  Hh.llist.assign((size_t)(no ? no : 1), 0);
  auto landmark = [&](int k) { return gpr->obs_kind[k] == 0 ? gpr->obs_point[k] : nx + gpr->obs_point[k]; };
  for (int k = 0; k < no; ++k) Hh.lstart[landmark(k) + 1]++;
  for (int p = 0; p < Z.nlm; ++p) Hh.lstart[p + 1] += Hh.lstart[p];
  std::vector<int32_t> fill(Hh.lstart.begin(), Hh.lstart.end() - 1);
  for (int k = 0; k < no; ++k) Hh.llist[fill[landmark(k)]++] = k;
}

// A large pose graph (no landmarks) is solved block-sparse: bsparse.h.  GSLAM_HIP_PG_SPARSE_MIN = keyframes from which
// it is used (0: always; default 384 -- below it the dense system is a single-launch factorisation and bitwise
// reproducible), GSLAM_HIP_PG_ROOT = keyframes kept for the dense root.  Sets Z.sparse; then the elimination order, the
// solver's lists and the address of every block pg_assemble_bs stores.
gh_status graph_plan_sparse(gh_ctx* ctx, GraphShape& Z, GraphHost& Hh, BsSolver& BS, bool verbose) {
  int sparse_min = 384, root_min = 128;
  if (const char* e = getenv("GSLAM_HIP_PG_SPARSE_MIN")) sparse_min = atoi(e);
  if (const char* e = getenv("GSLAM_HIP_PG_ROOT")) root_min = std::max(1, atoi(e));
  Z.sparse = Z.nlm == 0 && Z.nf >= sparse_min && sparse_min >= 0;
  if (!Z.sparse) return GH_OK;
  const PoseHost& PH = Hh.PH;
  const int nf = Z.nf;
  BS.P.build(nf, PH.n_pairs, PH.prow.data(), PH.pcol.data(), root_min, 64);
  GH_TRY(BS.prepare_host(ctx));
  const size_t nb = (size_t)nf + PH.n_pairs;
  Hh.bs_off.resize(nb);
  Hh.bs_sp.resize(nb);
  Hh.bs_sq.resize(nb);
  for (int f = 0; f < nf; ++f) {
    size_t o = 0;
    int cs = 7;
    GH_CHECK_ARG(ctx, BS.block_addr(BS.P.pos[f], BS.P.pos[f], &o, &cs));
    Hh.bs_off[f] = (int64_t)o;
    Hh.bs_sp[f] = 1;
    Hh.bs_sq[f] = cs;
  }
  for (int k = 0; k < PH.n_pairs; ++k) {
    const int pa = BS.P.pos[PH.prow[k]], pb = BS.P.pos[PH.pcol[k]];
    size_t o = 0;
    int cs = 7;
    GH_CHECK_ARG(ctx, BS.block_addr(std::max(pa, pb), std::min(pa, pb), &o, &cs));
    Hh.bs_off[nf + k] = (int64_t)o;
    Hh.bs_sp[nf + k] = pa > pb ? 1 : cs;  // p indexes the pair's ROW frame: the block's row when that frame comes later in the order
    Hh.bs_sq[nf + k] = pa > pb ? cs : 1;
  }
  if (verbose)
    fprintf(stderr, "[gh_graph] block-sparse: %d keyframes -> %d sparse columns in %d rounds, %d blocks, root %d\n", nf, BS.P.ns,
            BS.P.n_rounds, BS.P.n_slots, BS.P.nr);
  return GH_OK;
}

// Bit budget K of the reproducible accumulation.  Contributions to one word: a keyframe's diagonal block takes one per
// observation slot in gr_frame_rows and one per slot pair of a landmark in gr_schur (<= slots x the landmark's slots in that
// keyframe, usually 1); the intrinsics block one per wave of landmarks.
// K = ceil(log2(4 x the busiest keyframe's slots + waves + 16))
int graph_det_budget(const gh_graph_problem* gpr, const GraphShape& Z) {
  const int nf = Z.nf, ni = Z.ni;
  std::vector<int> slots((size_t)nf, 0);
  for (int k = 0; k < Z.no; ++k) {
    const int fj = gpr->obs_frame[k];
    if (fj >= 0 && fj < nf) ++slots[fj];
    if (gpr->obs_kind[k] == 1) {
      const int p = gpr->obs_point[k];
      const int h = (p >= 0 && p < ni) ? gpr->idp_host[p] : -1;
      if (h >= 0 && h < nf && h != fj) ++slots[h];
    }
  }
  long long most = 16;
  for (int f = 0; f < nf; ++f) most = std::max<long long>(most, slots[f]);
  most = 4 * most + Z.nlm / 64 + 16;
  int K = 0;
  while ((1ll << K) < most) ++K;
  return K;
}

// sum of v[0..count) into D.out[slot]: fixed order (1024 per block, then the partials one after the other)
gh_status graph_reduce_to(gh_ctx* ctx, GraphRun& R, const double* v, int count, int slot) {
  const int nb = gh_div_up(count > 0 ? count : 1, 1024);
  GH_LAUNCH(ctx, "gr_reduce", gr_reduce_kernel, dim3(nb), dim3(256), 0, v, count, R.D.part);
  GH_LAUNCH(ctx, "pg_sum", pg_sum_kernel, dim3(1), dim3(64), 0, (const double*)R.D.part, nb, R.D.out, slot);
  return GH_OK;
}

// D.out[0] = cost of the pose edges, D.out[2] = cost of the observations at (S, xyz, rho)
gh_status graph_enqueue_cost(gh_ctx* ctx, GraphRun& R, const double* S_dev, const double* xyz_dev, const double* rho_dev,
                             const double* cam_dev, const uint8_t* was_valid) {
  const GraphShape& Z = R.Z;
  GraphDev& D = R.D;
  if (Z.ne > 0) GH_LAUNCH(ctx, "pg_cost", pg_cost_kernel, dim3(Z.eb()), dim3(64), 0, R.G, S_dev, D.cost_e);
  GH_TRY(graph_reduce_to(ctx, R, D.cost_e, Z.ne, 0));
  if (Z.no > 0)
    GH_LAUNCH(ctx, "gr_cost", gr_cost_kernel, dim3(Z.ob()), dim3(128), 0, R.LM, (const int32_t*)D.dof, S_dev, xyz_dev, rho_dev, cam_dev,
              was_valid, D.term);
  GH_TRY(graph_reduce_to(ctx, R, D.term, Z.no, 2));
  return GH_OK;
}

// Linearise at the current state: H, g, the landmarks' H_pp / g_p, the observation records; the gradient maximum is
// read back asynchronously.
gh_status graph_enqueue_linearise(gh_ctx* ctx, GraphRun& R, GraphLoop& L) {
  const GraphShape& Z = R.Z;
  GraphDev& D = R.D;
  const int nf = Z.nf, no = Z.no, nlm = Z.nlm, n = Z.n, lda = Z.lda;
  if (Z.sparse) GH_HIP(ctx, hipMemsetAsync(R.BS.d_H, 0, R.BS.n_vals * sizeof(double), ctx->stream));
  else GH_HIP(ctx, hipMemsetAsync(D.H, 0, (size_t)n * lda * sizeof(double), ctx->stream));
  GH_HIP(ctx, hipMemsetAsync(D.gmax, 0, 8, ctx->stream));
  GH_HIP(ctx, hipMemsetAsync(D.Hpp, 0, Z.nlm1() * 72, ctx->stream));
  GH_HIP(ctx, hipMemsetAsync(D.gp, 0, Z.nlm1() * 24, ctx->stream));
  if (Z.det) {
    GH_HIP(ctx, hipMemsetAsync(D.acc_hi, 0, (size_t)n * lda * sizeof(double), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(D.acc_lo, 0, (size_t)n * lda * sizeof(double), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(D.vacc, 0, (size_t)2 * n * sizeof(double), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(D.bound, 0, (size_t)(nf + 2) * 8, ctx->stream));
  }
  if (Z.ne > 0) GH_LAUNCH(ctx, "pg_edge", pg_edge_kernel, dim3(Z.eb4()), dim3(64), 0, R.G, (const double*)D.S, D.rec, D.cost_e);
  // stores the pose-edge sums into every diagonal block, every edge pair block and g (zeros where there is no edge)
  if (Z.sparse)
    GH_LAUNCH(ctx, "pg_assemble_bs", pg_assemble_bs_kernel, dim3(nf + Z.n_pairs), dim3(64), 0, R.G, R.Ls, (const double*)D.rec, R.BS.d_H,
              BsDest{D.bs_off, D.bs_sp, D.bs_sq}, D.g);
  else
    GH_LAUNCH(ctx, "pg_assemble", pg_assemble_kernel, dim3(nf + Z.n_pairs), dim3(64), 0, R.G, R.Ls, (const double*)D.rec, D.H, lda, D.g,
              D.gmax);
  if (Z.with_cam) GH_HIP(ctx, hipMemsetAsync(D.g + 7 * nf, 0, 72, ctx->stream));  // (pg_assemble stores the keyframe rows only)
  if (no > 0)
    GH_LAUNCH(ctx, "gr_obs_lin", gr_obs_lin_kernel, dim3(Z.ob()), dim3(128), 0, R.LM, (const int32_t*)D.dof, (const double*)D.S,
              (const double*)D.xyz, (const double*)D.rho, (const double*)D.cam, D.orec, D.valid, D.H, lda, D.g, D.Hpp, D.gp, D.cam_part,
              D.bound);
  if (Z.det && nlm > 0)
    GH_LAUNCH(ctx, "gr_lm_sum", gr_lm_sum_kernel, dim3(gh_div_up(nlm, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
              (const double*)D.orec, D.Hpp, D.gp);
  if (Z.with_cam)
    GH_LAUNCH(ctx, "gr_cam_fold", gr_cam_fold_kernel, dim3(1), dim3(1024), 0, (const double*)D.cam_part, 2 * Z.ob(), nf, D.H, lda, D.g);
  if (no > 0)
    GH_LAUNCH(ctx, "gr_frame_rows", gr_frame_rows_kernel, dim3(gh_div_up(16 * no, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
              (const double*)D.orec, D.H, lda, D.g, R.DA);
  if (Z.det)  // H += hi + lo, g likewise; the accumulators are cleared again for the Schur products of the iterations
    GH_LAUNCH(ctx, "gr_det_fold", gr_det_fold_kernel, dim3(gh_div_up((long long)n * lda + n, 256)), dim3(256), 0, D.H,
              (const double*)D.acc_hi, (const double*)D.acc_lo, n, lda, D.g, (const double*)D.vacc, (const double*)(D.vacc + n), n);
  GH_HIP(ctx, hipMemsetAsync(D.gmax, 0, 8, ctx->stream));
  GH_LAUNCH(ctx, "gr_gmax", gr_gmax_kernel, dim3(gh_div_up(n + 3 * nlm, 256)), dim3(256), 0, (const double*)D.g, n, (const double*)D.gp,
            3 * nlm, D.gmax);
  // (read behind the linear solve, which synchronises anyway: if the gradient test fires, the step computed meanwhile is
  //  simply dropped -- same decisions, one host round trip less per iteration)
  GH_HIP(ctx, hipMemcpyAsync(&R.rb->gmax_bits, D.gmax, 8, hipMemcpyDeviceToHost, ctx->stream));
  L.fresh_gmax = true;
  L.need_lin = false;
  return GH_OK;
}

// The damped reduced system of this radius: Hd = H + D / radius, d = g; then the landmarks are eliminated into it.
gh_status graph_enqueue_system(gh_ctx* ctx, GraphRun& R, double radius) {
  const GraphShape& Z = R.Z;
  GraphDev& D = R.D;
  const int no = Z.no, nlm = Z.nlm, n = Z.n, lda = Z.lda;
  if (!Z.sparse)
    GH_LAUNCH(ctx, "pg_damp", pg_damp_kernel, dim3(gh_div_up((long long)n * lda, 256)), dim3(256), 0, (const double*)D.H, D.Hd, n, lda,
              (const double*)D.g, D.d, radius);
  if (nlm == 0) return GH_OK;
  if (Z.det) {
    GH_HIP(ctx, hipMemsetAsync(D.acc_hi, 0, (size_t)n * lda * sizeof(double), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(D.acc_lo, 0, (size_t)n * lda * sizeof(double), ctx->stream));
    GH_HIP(ctx, hipMemsetAsync(D.vacc, 0, (size_t)2 * n * sizeof(double), ctx->stream));
  }
  GH_LAUNCH(ctx, "gr_lm_prepare", gr_lm_prepare_kernel, dim3(gh_div_up(nlm, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
            (const double*)D.Hpp, (const double*)D.orec, radius, D.Hinv, D.lmdim, D.Wh, D.hrep, D.Wc);
  if (no > 0)
    GH_LAUNCH(ctx, "gr_schur", gr_schur_kernel, dim3(gh_div_up(16 * no, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
              (const double*)D.orec, (const double*)D.Hinv, (const int32_t*)D.lmdim, (const double*)D.Wh, (const int32_t*)D.hrep,
              (const double*)D.gp, D.Hd, lda, D.d, R.DA);
  if (Z.with_cam)
    GH_LAUNCH(ctx, "gr_schur_cam", gr_schur_cam_kernel, dim3(gh_div_up(16 * no, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
              (const double*)D.orec, (const double*)D.Hinv, (const int32_t*)D.lmdim, (const double*)D.Wh, (const int32_t*)D.hrep,
              (const double*)D.Wc, D.Hd, lda, R.DA);
  if (Z.with_cam)
    GH_LAUNCH(ctx, "gr_schur_cam_cc", gr_schur_cam_cc_kernel, dim3(gh_div_up(nlm, 128)), dim3(128), 0, R.LM, (const double*)D.Hinv,
              (const int32_t*)D.lmdim, (const double*)D.Wc, (const double*)D.gp, D.Hd, lda, D.d, R.DA);
  if (Z.det)
    GH_LAUNCH(ctx, "gr_det_fold", gr_det_fold_kernel, dim3(gh_div_up((long long)n * lda + n, 256)), dim3(256), 0, D.Hd,
              (const double*)D.acc_hi, (const double*)D.acc_lo, n, lda, D.d, (const double*)D.vacc, (const double*)(D.vacc + n), n);
  return GH_OK;
}

// Factorise and solve, block-sparse or dense; both end with a stream synchronisation.  *info != 0: the system was not
// positive definite at this radius.
gh_status graph_linear_solve(gh_ctx* ctx, GraphRun& R, double radius, int* info) {
  if (R.Z.sparse) return R.BS.factor_solve(ctx, radius, R.D.g, R.D.d, info);
  R.rb->info = 0;
  GH_TRY(gh_potrf_solve_dev(ctx, R.D.Hd, R.Z.n, R.Z.lda, R.D.d, &R.rb->info));
  *info = R.rb->info;
  return GH_OK;
}

// The trial step: back-substitution of the landmarks, model decrease (D.out[1]), the candidate state and its cost; the
// three sums come back in one 32-byte copy.  Waits for the device.
gh_status graph_enqueue_trial(gh_ctx* ctx, GraphRun& R, int cam_free) {
  const GraphShape& Z = R.Z;
  GraphDev& D = R.D;
  const int nf = Z.nf, nlm = Z.nlm, n_items = Z.n_items();
  if (nlm > 0)
    GH_LAUNCH(ctx, "gr_backsub", gr_backsub_kernel, dim3(gh_div_up(nlm, 256)), dim3(256), 0, R.LM, (const uint8_t*)D.valid,
              (const double*)D.orec, (const double*)D.Hinv, (const int32_t*)D.lmdim, (const double*)D.gp, (const double*)D.d, D.dlm);
  if (n_items > 0)
    GH_LAUNCH(ctx, "gr_model", gr_model_kernel, dim3(gh_div_up(n_items, 256)), dim3(256), 0, R.G, R.LM, (const double*)D.rec,
              (const uint8_t*)D.valid, (const double*)D.orec, (const double*)D.d, (const double*)D.dlm, D.term);
  GH_TRY(graph_reduce_to(ctx, R, D.term, n_items, 1));
  GH_LAUNCH(ctx, "pg_update", pg_update_kernel, dim3(gh_div_up(nf, 256)), dim3(256), 0, nf, (const int32_t*)D.dof, (const double*)D.S,
            (const double*)D.d, D.Snew);
  if (nlm > 0)
    GH_LAUNCH(ctx, "gr_update", gr_update_kernel, dim3(gh_div_up(nlm, 256)), dim3(256), 0, Z.nx, Z.ni, (const double*)D.xyz,
              (const double*)D.rho, (const double*)D.dlm, D.xyz_new, D.rho_new, (const double*)D.cam, (const double*)(D.d + 7 * nf),
              cam_free, D.cam_new);
  GH_TRY(graph_enqueue_cost(ctx, R, D.Snew, D.xyz_new, D.rho_new, D.cam_new, D.valid));
  GH_HIP(ctx, hipMemcpyAsync(R.rb->out4, D.out, 32, hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GH_OK;
}

// Accept or reject the trial the read-back block speaks of (ok: there was one), and update the trust region.  true: the
// solve has terminated (L.term says why).
bool graph_decide(GraphRun& R, const gh_ba_options& opt, gh_ba_summary* sum, GraphLoop& L, bool ok, int it) {
  if (L.step(opt, sum, "gh_graph", it, ok, R.rb->out4[0] + R.rb->out4[2], R.rb->out4[1])) {
    std::swap(R.D.S, R.D.Snew);
    std::swap(R.D.xyz, R.D.xyz_new);
    std::swap(R.D.rho, R.D.rho_new);
    std::swap(R.D.cam, R.D.cam_new);
    L.need_lin = true;
  }
  return L.term != 0;
}

// results: through the pinned block too (the read-back words are not needed any more)
gh_status graph_download(gh_ctx* ctx, const GraphRun& R, gh_graph_problem* gpr) {
  const GraphShape& Z = R.Z;
  const GraphDev& D = R.D;
  const size_t bS = (size_t)Z.nf * 64, bX = (size_t)Z.nx * 24, bR = (size_t)Z.ni * 8;
  const size_t oX = (bS + 255) & ~(size_t)255, oR = oX + ((bX + 255) & ~(size_t)255), oC = oR + ((bR + 255) & ~(size_t)255);
  void* hp = nullptr;
  GH_TRY(gh_pinned(ctx, oC + 72 + 256, &hp));
  char* h = static_cast<char*>(hp);
  GH_HIP(ctx, hipMemcpyAsync(h, D.S, bS, hipMemcpyDeviceToHost, ctx->stream));
  if (Z.nx) GH_HIP(ctx, hipMemcpyAsync(h + oX, D.xyz, bX, hipMemcpyDeviceToHost, ctx->stream));
  if (Z.ni) GH_HIP(ctx, hipMemcpyAsync(h + oR, D.rho, bR, hipMemcpyDeviceToHost, ctx->stream));
  if (Z.with_cam) GH_HIP(ctx, hipMemcpyAsync(h + oC, D.cam, 72, hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(gpr->pg.frame_sim3, h, bS);
  if (Z.nx) memcpy(gpr->xyz, h + oX, bX);
  if (Z.ni) memcpy(gpr->idp_rho, h + oR, bR);
  if (Z.with_cam) memcpy(gpr->intrinsics, h + oC, 72);
  return GH_OK;
}

}  // namespace

extern "C" gh_status gh_graph_solve(gh_ctx* ctx, gh_graph_problem* gpr, const gh_ba_options* opt_in, gh_ba_summary* sum_out) {
  if (!ctx || !gpr) return GH_ERR_ARG;
  GH_ENTER(ctx);
  gh_ba_options opt;
  gh_ba_default_options(&opt);
  if (opt_in) opt = *opt_in;
  gh_ba_summary local;
  gh_ba_summary* sum = sum_out ? sum_out : &local;
  memset(sum, 0, sizeof(*sum));
  GraphRun R(gpr);
  GraphShape& Z = R.Z;
  GraphDev& D = R.D;
  GH_TRY(graph_check_problem(ctx, gpr, Z));
  const double t_begin = now_ms_pg();
  // plan: edge and landmark lists, the linear solver, the accumulation mode
  GraphHost Hh;
  GH_TRY(Hh.PH.build(ctx, &gpr->pg));
  Z.ne = Hh.PH.ne;
  Z.n_pairs = Hh.PH.n_pairs;
  GH_TRY(graph_check_observations(ctx, gpr, Z));
  graph_landmark_lists(gpr, Z, Hh);
  GH_TRY(graph_plan_sparse(ctx, Z, Hh, R.BS, opt.verbose != 0));
  Z.det = opt.deterministic != 0 && !Z.sparse && Z.no > 0;
  // allocate and upload
  GraphArena A(ctx);
  D.alloc(A, Z, gpr, Hh, R.BS);  // measuring pass
  GH_TRY(A.reserve());
  if (!D.alloc(A, Z, gpr, Hh, R.BS))
    return gh_set_error(ctx, GH_ERR_NOMEM, "gh_graph_solve: device allocation failed (dense keyframe system: %d x %d doubles)", Z.n, Z.lda);
  GH_TRY(A.flush());
  if (Z.sparse) GH_TRY(R.BS.clear_values(ctx));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  {  // (the pinned block is free again after the synchronisation above; nothing below asks for it before the download)
    void* hp = nullptr;
    GH_TRY(gh_readback_block(ctx, sizeof(GraphReadback), &hp));  // (its own block: later gh_pinned requests cannot move it)
    R.rb = static_cast<GraphReadback*>(hp);
    memset(R.rb, 0, sizeof(*R.rb));
  }
  if (Z.sparse) R.BS.h_flag = &R.rb->bs_flag;
  const int cam_free = Z.with_cam ? gpr->intrinsics_free : 0;
  if (Z.det) R.DA = DetAcc{D.acc_hi, D.acc_lo, D.vacc, D.vacc + Z.n, D.bound, graph_det_budget(gpr, Z), Z.nf};
  R.G = PgGraph{Z.nf, Z.ne, D.dof, D.etype, D.ei, D.ej, D.meas, D.info};
  R.Ls = PgLists{D.vstart, D.vlist, D.pstart, D.plist, D.prow, D.pcol, Z.n_pairs};
  R.LM = GrLandmarks{Z.nx, Z.ni, Z.no, D.xfree, D.host, D.anchor, D.ifree, D.okind, D.opoint, D.oframe, D.oxy, D.oinfo, D.lstart, D.llist,
                     opt.huber_delta, gpr->projection, Z.with_cam ? 1 : 0, cam_free, Z.nf, Z.rec};
  // first cost
  GH_TRY(graph_enqueue_cost(ctx, R, D.S, D.xyz, D.rho, D.cam, nullptr));
  GH_HIP(ctx, hipMemcpyAsync(R.rb->out4, D.out, 32, hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  GraphLoop L;
  L.cost = sum->initial_cost = R.rb->out4[0] + R.rb->out4[2];
  L.radius = opt.initial_radius;
  int it = 0;
  for (it = 0; it < opt.max_iterations; ++it) {
    if (L.need_lin) GH_TRY(graph_enqueue_linearise(ctx, R, L));
    GH_TRY(graph_enqueue_system(ctx, R, L.radius));
    int info = 0;
    const double t_s0 = now_ms_pg();
    GH_TRY(graph_linear_solve(ctx, R, L.radius, &info));
    sum->solve_ms_total += now_ms_pg() - t_s0;
    if (L.fresh_gmax) {  // (both solve paths end with a stream synchronisation: the gradient maximum is on the host)
      L.fresh_gmax = false;
      double gmax;
      memcpy(&gmax, &R.rb->gmax_bits, 8);
      if (gmax <= opt.gradient_tolerance) {
        L.term = 2;
        break;
      }
    }
    if (info == 0) GH_TRY(graph_enqueue_trial(ctx, R, cam_free));
    if (graph_decide(R, opt, sum, L, info == 0, it)) {
      ++it;
      break;
    }
  }
  sum->iterations = it;
  sum->termination = L.term;
  sum->final_cost = L.cost;
  GH_TRY(graph_download(ctx, R, gpr));
  sum->total_ms = now_ms_pg() - t_begin;
  return L.term == 3 ? GH_ERR_NUMERIC : GH_OK;
}

// The pose graph alone is the general graph without landmarks (no atomics are involved then: the assembly is the
// deterministic pg_assemble, the sums are fixed-order -- bitwise reproducible from run to run).
extern "C" gh_status gh_pg_solve(gh_ctx* ctx, gh_pg_problem* pr, const gh_ba_options* opt_in, gh_ba_summary* sum_out) {
  if (!ctx || !pr) return GH_ERR_ARG;
  gh_graph_problem g;
  memset(&g, 0, sizeof(g));
  g.pg = *pr;
  gh_ba_options opt;
  gh_ba_default_options(&opt);
  if (opt_in) opt = *opt_in;
  opt.huber_delta = 0.0;  // (the projection Huber threshold has no meaning without observations)
  return gh_graph_solve(ctx, &g, &opt, sum_out);
}

// ---------------------------------------------------------------- 3-D alignment
namespace {

// 17 sums per correspondence block of 256, then a fixed-order fold: {sum a, sum b, sum a b^T, sum |a|^2, sum |b|^2}, with
// a = src - src[0] and b = dst - dst[0].  About that pivot the centred moments cancel at the size of the cloud, not at the
// size of its coordinates (a trajectory in GPS coordinates: 1e6 m away, metres across), so the result is translation-
// invariant to rounding; every thread reads the pivot itself (one cached line), no extra launch.
__global__ __launch_bounds__(256) void align_sums_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n,
                                                         double* __restrict__ partial) {
  __shared__ double sh[256];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double v[17];
  for (int q = 0; q < 17; ++q) v[q] = 0.0;
  if (k < n) {
    const double a[3] = {src[3 * (size_t)k] - src[0], src[3 * (size_t)k + 1] - src[1], src[3 * (size_t)k + 2] - src[2]};
    const double b[3] = {dst[3 * (size_t)k] - dst[0], dst[3 * (size_t)k + 1] - dst[1], dst[3 * (size_t)k + 2] - dst[2]};
    for (int e = 0; e < 3; ++e) {
      v[e] = a[e];
      v[3 + e] = b[e];
      for (int f = 0; f < 3; ++f) v[6 + 3 * e + f] = a[e] * b[f];
    }
    v[15] = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    v[16] = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  }
  for (int q = 0; q < 17; ++q) {
    sh[threadIdx.x] = v[q];
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 17 + q] = sh[0];
    __syncthreads();
  }
}

// residual sum of squares and the 7 x 7 information at the solution: 50 values per block of 256, same fold.  S8 = the
// transform followed by its translation in pivot coordinates tp (11 doubles): the residual is taken as
// (b - b0) - (s R (a - a0) + tp), the same residual as dst - S src without the rounding of coordinates that are large
// against it.  The information is built from the uncentred a (the Jacobian of a right-multiplied delta).
__global__ __launch_bounds__(256) void align_info_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n,
                                                         const double* __restrict__ S8, int dof, double* __restrict__ partial) {
  __shared__ double sh[256];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double S[11];
  for (int e = 0; e < 11; ++e) S[e] = S8[e];
  double a[3] = {0, 0, 0}, ssq = 0.0;
  const bool on = k < n;
  if (on) {
    for (int e = 0; e < 3; ++e) a[e] = src[3 * (size_t)k + e];
    const double ap[3] = {a[0] - src[0], a[1] - src[1], a[2] - src[2]};
    double Ra[3];
    q_rot(S, ap, Ra);
    for (int e = 0; e < 3; ++e) {
      const double r = (dst[3 * (size_t)k + e] - dst[e]) - (S[7] * Ra[e] + S[8 + e]);
      ssq += r * r;
    }
  }
  const double D[3][7] = {{1, 0, 0, 0, a[2], -a[1], a[0]}, {0, 1, 0, -a[2], 0, a[0], a[1]}, {0, 0, 1, a[1], -a[0], 0, a[2]}};
  for (int q = 0; q < 50; ++q) {
    double v = 0.0;
    if (on) {
      if (q == 49) v = ssq;
      else {
        const int p = q / 7, c = q - 7 * p;
        if (((dof >> p) & 1) && ((dof >> c) & 1)) {
          double s = 0;
          for (int e = 0; e < 3; ++e) s += D[e][p] * D[e][c];
          v = S[7] * S[7] * s;
        }
      }
    }
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 50 + q] = sh[0];
    __syncthreads();
  }
}

void jacobi4(double a[4][4], double v[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (!(fabs(apq) > 1e-300)) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - sn * akq;
          a[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - sn * aqk;
          a[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - sn * vkq;
          v[k][q] = sn * vkp + c * vkq;
        }
      }
}

// Horn's closed form from the 17 sums about the pivot (a0, b0) (host: a 4 x 4 eigenproblem) -- pg_oracle.c
// oracle_align_from_sums.  The centroids are a0 + mean, b0 + mean.
// tp: the translation in pivot coordinates, mb - s R ma.
bool align_from_sums(const double* sums, const double* a0, const double* b0, int n, bool with_scale, double* out8, double* tp) {
  if (n < 3) return false;
  const double inv = 1.0 / n;
  double ma[3], mb[3], ca[3], cb[3], M[3][3];
  for (int e = 0; e < 3; ++e) {
    ma[e] = sums[e] * inv;
    mb[e] = sums[3 + e] * inv;
    ca[e] = a0[e] + ma[e];
    cb[e] = b0[e] + mb[e];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[r][c] = sums[6 + 3 * r + c] - n * ma[r] * mb[c];
  const double na = sums[15] - n * (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]);
  const double nb = sums[16] - n * (mb[0] * mb[0] + mb[1] * mb[1] + mb[2] * mb[2]);
  if (!(na > 1e-300) || !(nb > 1e-300)) return false;
  double N[4][4] = {{M[0][0] + M[1][1] + M[2][2], M[1][2] - M[2][1], M[2][0] - M[0][2], M[0][1] - M[1][0]},
                    {0, M[0][0] - M[1][1] - M[2][2], M[0][1] + M[1][0], M[2][0] + M[0][2]},
                    {0, 0, -M[0][0] + M[1][1] - M[2][2], M[1][2] + M[2][1]},
                    {0, 0, 0, -M[0][0] - M[1][1] + M[2][2]}};
  for (int r = 1; r < 4; ++r)
    for (int c = 0; c < r; ++c) N[r][c] = N[c][r];
  double V[4][4];
  jacobi4(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > N[best][best]) best = k;
  double qw = V[0][best], qx = V[1][best], qy = V[2][best], qz = V[3][best];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  if (!(qn > 1e-300)) return false;
  if (qw < 0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  const double sc = with_scale ? sqrt(nb / na) : 1.0;
  const double q[4] = {qx, qy, qz, qw};
  double Rca[3], Rma[3];
  q_rot(q, ca, Rca);
  q_rot(q, ma, Rma);
  out8[0] = qx; out8[1] = qy; out8[2] = qz; out8[3] = qw;
  for (int e = 0; e < 3; ++e) out8[4 + e] = cb[e] - sc * Rca[e];
  out8[7] = sc;
  for (int e = 0; e < 3; ++e) tp[e] = mb[e] - sc * Rma[e];
  return true;
}

}  // namespace

extern "C" gh_status gh_align_sim3(gh_ctx* ctx, const double* src, const double* dst, int n, int dof, double* sim3_out,
                                   double* information_out, double* ssq_out, int* ok_out) {
  if (!ctx) return GH_ERR_ARG;
  GH_ENTER(ctx);
  GH_CHECK_ARG(ctx, n >= 0 && sim3_out && ok_out && (n == 0 || (src && dst)));
  *ok_out = 0;
  for (int e = 0; e < 8; ++e) sim3_out[e] = e == 3 || e == 7 ? 1.0 : 0.0;
  if (information_out)
    for (int e = 0; e < 49; ++e) information_out[e] = 0.0;
  if (ssq_out) *ssq_out = 0.0;
  if (n < 3) return GH_OK;
  const int nb = gh_div_up(n, 256);
  const size_t pts = (((size_t)n * 24) + 255) & ~(size_t)255, part = (((size_t)nb * 50 * 8) + 255) & ~(size_t)255;
  void *base = nullptr, *hbase = nullptr;
  GH_TRY(gh_scratch(ctx, 2 * pts + part + 256, &base));
  GH_TRY(gh_pinned(ctx, 2 * pts + part + 256, &hbase));  // host mirror of the layout: every copy is one DMA from / to pinned memory
  double* d_src = (double*)base;
  double* d_dst = (double*)((char*)base + pts);
  double* d_part = (double*)((char*)base + 2 * pts);
  double* d_S = (double*)((char*)base + 2 * pts + part);
  char* hb = (char*)hbase;
  double* hp = (double*)(hb + 2 * pts);
  memcpy(hb, src, (size_t)n * 24);
  memcpy(hb + pts, dst, (size_t)n * 24);
  GH_HIP(ctx, hipMemcpyAsync(d_src, hb, pts + (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
  GH_LAUNCH(ctx, "align_sums", align_sums_kernel, dim3(nb), dim3(256), 0, (const double*)d_src, (const double*)d_dst, n, d_part);
  GH_HIP(ctx, hipMemcpyAsync(hp, d_part, (size_t)nb * 17 * 8, hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double sums[17];
  for (int q = 0; q < 17; ++q) {
    double s = 0;
    for (int b = 0; b < nb; ++b) s += hp[(size_t)b * 17 + q];  // block order
    sums[q] = s;
  }
  double tp[3];
  if (!align_from_sums(sums, src, dst, n, ((dof >> 6) & 1) != 0, sim3_out, tp)) {
    for (int e = 0; e < 8; ++e) sim3_out[e] = e == 3 || e == 7 ? 1.0 : 0.0;
    return GH_OK;  // degenerate set: *ok_out stays 0
  }
  *ok_out = 1;
  if (information_out || ssq_out) {
    memcpy(hb + 2 * pts + part, sim3_out, 64);
    memcpy(hb + 2 * pts + part + 64, tp, 24);
    GH_HIP(ctx, hipMemcpyAsync(d_S, hb + 2 * pts + part, 88, hipMemcpyHostToDevice, ctx->stream));
    GH_LAUNCH(ctx, "align_info", align_info_kernel, dim3(nb), dim3(256), 0, (const double*)d_src, (const double*)d_dst, n,
              (const double*)d_S, dof, d_part);
    GH_HIP(ctx, hipMemcpyAsync(hp, d_part, (size_t)nb * 50 * 8, hipMemcpyDeviceToHost, ctx->stream));
    GH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < 50; ++q) {
      double s = 0;
      for (int b = 0; b < nb; ++b) s += hp[(size_t)b * 50 + q];
      if (q == 49) {
        if (ssq_out) *ssq_out = s;
      } else if (information_out) {
        information_out[q] = s;
      }
    }
  }
  return GH_OK;
}
