// Shared pieces of the RANSAC estimator (ransac.hip: one problem per call; ransac_batch.hip: many problems per launch):
// the sampler, the minimal solvers, the error of one correspondence and the essential projection.  Both translation units
// run exactly this code, which is what keeps the batched entries bit-identical to gh_ransac_estimate.
#pragma once
#include "common.h"

namespace gh_ransac {

enum { kModelH = 0, kModelA2 = 1, kModelF = 2, kModelA3 = 3, kModelE = 4, kModelSim3 = 5, kModelPlane = 6, kModelPnP = 7 };
constexpr int kHyp = 2048;
constexpr double kTiny = 1e-12;

__host__ __device__ inline uint64_t sm64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ inline int sample_size(int model) {
  switch (model) {
    case kModelH: return 4;
    case kModelA2: return 3;
    case kModelF: case kModelE: return 8;
    case kModelA3: return 4;
    case kModelSim3: case kModelPlane: return 3;
    default: return 6;  // PnP: 6-point DLT
  }
}
__host__ __device__ inline int model_size(int model) {
  switch (model) {
    case kModelH: case kModelF: case kModelE: return 9;
    case kModelA2: return 6;
    case kModelSim3: return 8;
    case kModelPlane: return 4;
    default: return 12;  // A3 (3 x 4) and PnP ([R | t], world -> camera)
  }
}
__host__ __device__ constexpr inline int dim_p(int model) { return (model == kModelA3 || model == kModelSim3 || model == kModelPlane || model == kModelPnP) ? 3 : 2; }
__host__ __device__ constexpr inline int dim_q(int model) { return (model == kModelA3 || model == kModelSim3 || model == kModelPlane) ? 3 : 2; }

// Cyclic Jacobi eigen-decomposition of a symmetric N x N matrix (a is destroyed, v receives the eigenvectors as columns):
// a fixed number of sweeps of the classical rotation, written with + - * / sqrt only, so that the device and the CPU
// checker produce the same bits.
template <int N>
__host__ __device__ inline void jacobi_eig(double (*a)[N], double (*v)[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 12; ++sweep)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        if (!(fabs(apq) > 1e-300)) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < N; ++k) {  // A <- A J
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - sn * akq;
          a[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {  // A <- J^T A
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - sn * aqk;
          a[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - sn * vkq;
          v[k][q] = sn * vkp + c * vkq;
        }
      }
}

// Horn's closed-form absolute orientation with scale (Horn 1987; GSLAM::Estimator::findSIM3, method S3_Horn) from three
// point pairs: b ~ s R a + t.  out = [qx qy qz qw tx ty tz s] (GSLAM's SIM3 field order).
// (m pairs: the three of a RANSAC sample through idx, or all n in index order with idx = nullptr -- the NOSAMPLE fit)
__host__ __device__ inline bool solve_sim3(const double* p, const double* q, const int* idx, double* out, int m = 3) {
  double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
  for (int j = 0; j < m; ++j) {
    const int ij = idx ? idx[j] : j;
    for (int e = 0; e < 3; ++e) {
      ca[e] = ca[e] + p[3 * ij + e];
      cb[e] = cb[e] + q[3 * ij + e];
    }
  }
  for (int e = 0; e < 3; ++e) {
    ca[e] = ca[e] / (double)m;
    cb[e] = cb[e] / (double)m;
  }
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, na = 0.0, nb = 0.0;
  for (int j = 0; j < m; ++j) {
    const int ij = idx ? idx[j] : j;
    double a[3], b[3];
    for (int e = 0; e < 3; ++e) {
      a[e] = p[3 * ij + e] - ca[e];
      b[e] = q[3 * ij + e] - cb[e];
      na = na + a[e] * a[e];
      nb = nb + b[e] * b[e];
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S[r][c] = S[r][c] + a[r] * b[c];
  }
  if (!(na > kTiny) || !(nb > kTiny)) return false;
  double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                    {0, S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                    {0, 0, -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                    {0, 0, 0, -S[0][0] - S[1][1] + S[2][2]}};
  for (int r = 1; r < 4; ++r)
    for (int c = 0; c < r; ++c) N[r][c] = N[c][r];
  double V[4][4];
  jacobi_eig<4>(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > N[best][best]) best = k;
  double qw = V[0][best], qx = V[1][best], qy = V[2][best], qz = V[3][best];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  if (!(qn > kTiny)) return false;
  if (qw < 0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
  qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
  const double sc = sqrt(nb / na);
  const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                       2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                       2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)};
  out[0] = qx; out[1] = qy; out[2] = qz; out[3] = qw;
  for (int r = 0; r < 3; ++r) out[4 + r] = cb[r] - sc * (R[3 * r] * ca[0] + R[3 * r + 1] * ca[1] + R[3 * r + 2] * ca[2]);
  out[7] = sc;
  return true;
}

// Plane through three points: out = [nx ny nz d], n unit, n . x + d = 0.
__device__ inline bool solve_plane(const double* p, const int* idx, double* out) {
  const double* p0 = p + 3 * idx[0];
  const double* p1 = p + 3 * idx[1];
  const double* p2 = p + 3 * idx[2];
  const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, v[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (!(len > kTiny)) return false;
  for (int e = 0; e < 3; ++e) n[e] = n[e] / len;
  out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
  out[3] = -(n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2]);
  return true;
}

// Perspective-n-point from six 3D-2D pairs by the direct linear transform: 12 x 12 homogeneous system, nullspace by
// elimination with full pivoting (as for F), scaled to |r3| = 1 with positive depth, rotation made orthonormal by
// Gram-Schmidt on its rows.  out = [R (row-major 9) | t (3)], X_c = R X_w + t.  Coplanar object points are degenerate.
__host__ __device__ inline bool pnp_from_projection(double* P, const double* X0, double* out);
__device__ inline bool solve_pnp_dlt(const double* p, const double* q, const int* idx, double* out) {
  double a[12][12];
  for (int j = 0; j < 6; ++j) {
    const double X = p[3 * idx[j]], Y = p[3 * idx[j] + 1], Z = p[3 * idx[j] + 2], u = q[2 * idx[j]], v = q[2 * idx[j] + 1];
    double* r0 = a[2 * j];
    double* r1 = a[2 * j + 1];
    r0[0] = X; r0[1] = Y; r0[2] = Z; r0[3] = 1; r0[4] = 0; r0[5] = 0; r0[6] = 0; r0[7] = 0;
    r0[8] = -u * X; r0[9] = -u * Y; r0[10] = -u * Z; r0[11] = -u;
    r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = 0; r1[4] = X; r1[5] = Y; r1[6] = Z; r1[7] = 1;
    r1[8] = -v * X; r1[9] = -v * Y; r1[10] = -v * Z; r1[11] = -v;
  }
  int perm[12];
  for (int c = 0; c < 12; ++c) perm[c] = c;
  for (int k = 0; k < 11; ++k) {
    int pr = k, pc = k;
    double best = -1.0;
    for (int r = k; r < 12; ++r)
      for (int c = k; c < 12; ++c) {
        const double v = fabs(a[r][c]);
        if (v > best) {
          best = v;
          pr = r;
          pc = c;
        }
      }
    if (!(best > kTiny)) return false;
    if (pr != k)
      for (int c = 0; c < 12; ++c) {
        const double t = a[k][c];
        a[k][c] = a[pr][c];
        a[pr][c] = t;
      }
    if (pc != k) {
      for (int r = 0; r < 12; ++r) {
        const double t = a[r][k];
        a[r][k] = a[r][pc];
        a[r][pc] = t;
      }
      const int t = perm[k];
      perm[k] = perm[pc];
      perm[pc] = t;
    }
    const double inv = 1.0 / a[k][k];
    for (int r = k + 1; r < 12; ++r) {
      const double f = a[r][k] * inv;
      for (int c = k; c < 12; ++c) a[r][c] = a[r][c] - f * a[k][c];
    }
  }
  double z[12], P[12];
  z[11] = 1.0;
  for (int r = 10; r >= 0; --r) {
    double sres = 0.0;
    for (int c = r + 1; c < 12; ++c) sres = sres + a[r][c] * z[c];
    z[r] = -sres / a[r][r];
  }
  for (int c = 0; c < 12; ++c) P[perm[c]] = z[c];
  return pnp_from_projection(P, p + 3 * idx[0], out);
}

// [R | t] from a 3 x 4 projection known up to scale: scaled to |r3| = 1 with X0 in front of the camera, rotation made
// orthonormal by Gram-Schmidt on its rows.
__host__ __device__ inline bool pnp_from_projection(double* P, const double* X0, double* out) {
  const double n3 = sqrt(P[8] * P[8] + P[9] * P[9] + P[10] * P[10]);
  if (!(n3 > kTiny)) return false;
  double lam = 1.0 / n3;
  if ((P[8] * X0[0] + P[9] * X0[1] + P[10] * X0[2] + P[11]) * lam < 0) lam = -lam;  // the sample lies in front of the camera
  for (int c = 0; c < 12; ++c) P[c] = P[c] * lam;
  double r1[3] = {P[0], P[1], P[2]}, r2[3] = {P[4], P[5], P[6]};
  const double n1 = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
  if (!(n1 > kTiny)) return false;
  for (int e = 0; e < 3; ++e) r1[e] = r1[e] / n1;
  const double d12 = r2[0] * r1[0] + r2[1] * r1[1] + r2[2] * r1[2];
  for (int e = 0; e < 3; ++e) r2[e] = r2[e] - d12 * r1[e];
  const double n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
  if (!(n2 > kTiny)) return false;
  for (int e = 0; e < 3; ++e) r2[e] = r2[e] / n2;
  const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
  if (!(r3[0] * P[8] + r3[1] * P[9] + r3[2] * P[10] > 0)) return false;  // a reflection, not a rotation
  for (int e = 0; e < 3; ++e) {
    out[e] = r1[e];
    out[3 + e] = r2[e];
    out[6 + e] = r3[e];
  }
  out[9] = P[3] / n1;  // each translation component carries the scale of its own row of the raw estimate
  out[10] = P[7] / n2;
  out[11] = P[11];
  return true;
}

// Solve A x = b (n <= 8, nrhs <= 3) in place, partial pivoting (first maximum).  a: n x (n + nrhs) row-major, ld = 12.
__host__ __device__ inline bool ge_solve(double (*a)[12], int n, int nrhs) {
  for (int k = 0; k < n; ++k) {
    int piv = k;
    double best = fabs(a[k][k]);
    for (int r = k + 1; r < n; ++r) {
      const double v = fabs(a[r][k]);
      if (v > best) {
        best = v;
        piv = r;
      }
    }
    if (!(best > kTiny)) return false;
    if (piv != k)
      for (int c = 0; c < n + nrhs; ++c) {
        const double t = a[k][c];
        a[k][c] = a[piv][c];
        a[piv][c] = t;
      }
    const double inv = 1.0 / a[k][k];
    for (int r = k + 1; r < n; ++r) {
      const double f = a[r][k] * inv;
      for (int c = k; c < n + nrhs; ++c) a[r][c] = a[r][c] - f * a[k][c];
    }
  }
  for (int j = 0; j < nrhs; ++j)
    for (int r = n - 1; r >= 0; --r) {
      double s = a[r][n + j];
      for (int c = r + 1; c < n; ++c) s = s - a[r][c] * a[c][n + j];
      a[r][n + j] = s / a[r][r];
    }
  return true;
}

struct Norm {  // Hartley normalisation of both point sets, over ALL points of a problem
  double m1x, m1y, s1, m2x, m2y, s2;
};

// The normalisation of n >= 1 correspondences (F / E): centroid, and sqrt(2) over the mean distance from it.  The sums are
// taken sequentially in index order, on the host (gh_ransac_estimate_ex) and on the device (one lane per problem of the
// batch) alike, as the oracle takes them: a tree reduction would round differently.
__host__ __device__ inline Norm hartley_norm(const double* src, const double* dst, int n) {
  Norm nm;
  double ax = 0, ay = 0, bx = 0, by = 0;
  for (int i = 0; i < n; ++i) {
    ax += src[2 * i]; ay += src[2 * i + 1];
    bx += dst[2 * i]; by += dst[2 * i + 1];
  }
  nm.m1x = ax / n; nm.m1y = ay / n; nm.m2x = bx / n; nm.m2y = by / n;
  double d1 = 0, d2 = 0;
  for (int i = 0; i < n; ++i) {
    const double x = src[2 * i] - nm.m1x, y = src[2 * i + 1] - nm.m1y;
    const double u = dst[2 * i] - nm.m2x, v = dst[2 * i + 1] - nm.m2y;
    d1 += sqrt(x * x + y * y);
    d2 += sqrt(u * u + v * v);
  }
  d1 /= n; d2 /= n;
  nm.s1 = d1 > 0 ? 1.4142135623730951 / d1 : 1.0;
  nm.s2 = d2 > 0 ? 1.4142135623730951 / d2 : 1.0;
  return nm;
}

// Hypothesis h of a problem: draws its minimal sample with splitmix64(seed, h) (duplicates rejected; n >= sample_size(model)
// is the caller's business: the rejection loop does not end otherwise) and solves it into out (model_size(model) doubles).
// p: N x dim doubles (src), q: N x dim doubles (dst)
__device__ inline bool solve_hypothesis(int model, const double* __restrict__ p, const double* __restrict__ q, int n,
                                        uint64_t seed, const Norm& nm, int h, double* __restrict__ out) {
  const int s = sample_size(model);
  int idx[8];
  uint64_t st = sm64(seed ^ ((uint64_t)h * 0xD1B54A32D192ED03ull));
  for (int j = 0; j < s; ++j) {
    for (;;) {
      st = sm64(st);
      const int c = (int)(st % (uint64_t)n);
      bool dup = false;
      for (int t = 0; t < j; ++t) dup = dup || idx[t] == c;
      if (!dup) {
        idx[j] = c;
        break;
      }
    }
  }
  double a[8][12];
  bool ok = false;
  if (model == kModelH) {
    for (int j = 0; j < 4; ++j) {
      const double x = p[2 * idx[j]], y = p[2 * idx[j] + 1], u = q[2 * idx[j]], v = q[2 * idx[j] + 1];
      double* r0 = a[2 * j];
      double* r1 = a[2 * j + 1];
      r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = u;
      r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -v * x; r1[7] = -v * y; r1[8] = v;
    }
    ok = ge_solve(a, 8, 1);
    if (ok) {
      for (int i = 0; i < 8; ++i) out[i] = a[i][8];
      out[8] = 1.0;
    }
  } else if (model == kModelA2) {
    for (int j = 0; j < 3; ++j) {
      a[j][0] = p[2 * idx[j]]; a[j][1] = p[2 * idx[j] + 1]; a[j][2] = 1;
      a[j][3] = q[2 * idx[j]]; a[j][4] = q[2 * idx[j] + 1];
    }
    ok = ge_solve(a, 3, 2);
    if (ok)
      for (int i = 0; i < 3; ++i) {
        out[i] = a[i][3];
        out[3 + i] = a[i][4];
      }
  } else if (model == kModelA3) {
    for (int j = 0; j < 4; ++j) {
      a[j][0] = p[3 * idx[j]]; a[j][1] = p[3 * idx[j] + 1]; a[j][2] = p[3 * idx[j] + 2]; a[j][3] = 1;
      a[j][4] = q[3 * idx[j]]; a[j][5] = q[3 * idx[j] + 1]; a[j][6] = q[3 * idx[j] + 2];
    }
    ok = ge_solve(a, 4, 3);
    if (ok)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = a[c][4 + r];
  } else if (model == kModelSim3) {
    ok = solve_sim3(p, q, idx, out);
  } else if (model == kModelPlane) {
    ok = solve_plane(p, idx, out);
  } else if (model == kModelPnP) {
    ok = solve_pnp_dlt(p, q, idx, out);
  } else {  // fundamental / essential: 8 x 9 nullspace with full pivoting
    for (int j = 0; j < 8; ++j) {
      const double x = (p[2 * idx[j]] - nm.m1x) * nm.s1, y = (p[2 * idx[j] + 1] - nm.m1y) * nm.s1;
      const double u = (q[2 * idx[j]] - nm.m2x) * nm.s2, v = (q[2 * idx[j] + 1] - nm.m2y) * nm.s2;
      double* r = a[j];
      r[0] = u * x; r[1] = u * y; r[2] = u; r[3] = v * x; r[4] = v * y; r[5] = v; r[6] = x; r[7] = y; r[8] = 1;
    }
    int perm[9];
    for (int c = 0; c < 9; ++c) perm[c] = c;
    ok = true;
    for (int k = 0; k < 8 && ok; ++k) {
      int pr = k, pc = k;
      double best = -1.0;
      for (int r = k; r < 8; ++r)
        for (int c = k; c < 9; ++c) {
          const double v = fabs(a[r][c]);
          if (v > best) {
            best = v;
            pr = r;
            pc = c;
          }
        }
      if (!(best > kTiny)) {
        ok = false;
        break;
      }
      if (pr != k)
        for (int c = 0; c < 9; ++c) {
          const double t = a[k][c];
          a[k][c] = a[pr][c];
          a[pr][c] = t;
        }
      if (pc != k) {
        for (int r = 0; r < 8; ++r) {
          const double t = a[r][k];
          a[r][k] = a[r][pc];
          a[r][pc] = t;
        }
        const int t = perm[k];
        perm[k] = perm[pc];
        perm[pc] = t;
      }
      const double inv = 1.0 / a[k][k];
      for (int r = k + 1; r < 8; ++r) {
        const double f = a[r][k] * inv;
        for (int c = k; c < 9; ++c) a[r][c] = a[r][c] - f * a[k][c];
      }
    }
    if (ok) {
      double z[9];
      z[8] = 1.0;
      for (int r = 7; r >= 0; --r) {
        double sres = 0.0;
        for (int c = r + 1; c < 9; ++c) sres = sres + a[r][c] * z[c];
        z[r] = -sres / a[r][r];
      }
      double fh[9];
      for (int c = 0; c < 9; ++c) fh[perm[c]] = z[c];
      // F = T2^T * Fh * T1, T = [s 0 -s m_x; 0 s -s m_y; 0 0 1]
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
    }
  }
  return ok;
}

// squared error of correspondence i under model m; returns false if undefined
__device__ inline bool model_error(int model, const double* m, const double* p, const double* q, int i, double* err) {
  if (model == kModelH) {
    const double x = p[2 * i], y = p[2 * i + 1];
    const double w = m[6] * x + m[7] * y + m[8];
    if (!(fabs(w) > kTiny)) return false;
    const double px = (m[0] * x + m[1] * y + m[2]) / w, py = (m[3] * x + m[4] * y + m[5]) / w;
    const double dx = px - q[2 * i], dy = py - q[2 * i + 1];
    *err = dx * dx + dy * dy;
    return true;
  }
  if (model == kModelA2) {
    const double x = p[2 * i], y = p[2 * i + 1];
    const double dx = (m[0] * x + m[1] * y + m[2]) - q[2 * i], dy = (m[3] * x + m[4] * y + m[5]) - q[2 * i + 1];
    *err = dx * dx + dy * dy;
    return true;
  }
  if (model == kModelA3) {
    const double X = p[3 * i], Y = p[3 * i + 1], Z = p[3 * i + 2];
    double e = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double d = (m[4 * r] * X + m[4 * r + 1] * Y + m[4 * r + 2] * Z + m[4 * r + 3]) - q[3 * i + r];
      e = e + d * d;
    }
    *err = e;
    return true;
  }
  if (model == kModelSim3) {
    const double qx = m[0], qy = m[1], qz = m[2], qw = m[3], sc = m[7];
    const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                         2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                         2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)};
    const double X = p[3 * i], Y = p[3 * i + 1], Z = p[3 * i + 2];
    double e = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double d = (sc * (R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * Z) + m[4 + r]) - q[3 * i + r];
      e = e + d * d;
    }
    *err = e;
    return true;
  }
  if (model == kModelPlane) {
    const double d = m[0] * p[3 * i] + m[1] * p[3 * i + 1] + m[2] * p[3 * i + 2] + m[3];
    *err = d * d;
    return true;
  }
  if (model == kModelPnP) {
    const double X = p[3 * i], Y = p[3 * i + 1], Z = p[3 * i + 2];
    const double zc = m[6] * X + m[7] * Y + m[8] * Z + m[11];
    if (!(zc > kTiny)) return false;
    const double dx = (m[0] * X + m[1] * Y + m[2] * Z + m[9]) / zc - q[2 * i];
    const double dy = (m[3] * X + m[4] * Y + m[5] * Z + m[10]) / zc - q[2 * i + 1];
    *err = dx * dx + dy * dy;
    return true;
  }
  const double x = p[2 * i], y = p[2 * i + 1], u = q[2 * i], v = q[2 * i + 1];
  const double fx0 = m[0] * x + m[1] * y + m[2], fx1 = m[3] * x + m[4] * y + m[5], fx2 = m[6] * x + m[7] * y + m[8];
  const double ft0 = m[0] * u + m[3] * v + m[6], ft1 = m[1] * u + m[4] * v + m[7];
  const double num = u * fx0 + v * fx1 + fx2;
  const double den = fx0 * fx0 + fx1 * fx1 + ft0 * ft0 + ft1 * ft1;
  if (!(den > 1e-300)) return false;
  *err = (num * num) / den;
  return true;
}

// Projection of the winning 8-point estimate onto the essential manifold (two equal singular values, one zero):
// E = U diag(s, s, 0) V^T with s = (s1 + s2) / 2, through the Jacobi eigen-decomposition of E^T E.
__host__ __device__ inline bool project_essential(double* E) {
  double B[3][3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + E[3 * k + r] * E[3 * k + c];
      B[r][c] = acc;
    }
  jacobi_eig<3>(B, V);
  int o[3] = {0, 1, 2};  // eigenvalues in descending order (stable selection)
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (B[o[b]][o[b]] > B[o[a]][o[a]]) {
        const int t = o[a];
        o[a] = o[b];
        o[b] = t;
      }
  const double l1 = B[o[0]][o[0]], l2 = B[o[1]][o[1]];
  if (!(l2 > 1e-300)) return false;
  const double s1 = sqrt(l1), s2 = sqrt(l2), sm = (s1 + s2) / 2.0;
  double u[2][3];
  for (int a = 0; a < 2; ++a) {
    const double sv = a == 0 ? s1 : s2;
    for (int r = 0; r < 3; ++r) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + E[3 * r + k] * V[k][o[a]];
      u[a][r] = acc / sv;
    }
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) E[3 * r + c] = sm * (u[0][r] * V[c][o[0]] + u[1][r] * V[c][o[1]]);
  return true;
}

// ---- two-view reconstruction (two_view.hip): pose candidates of an essential matrix and the rule for one correspondence.
// tests/two_view_restate.py restates both in scalar doubles and the device is held to it bit for bit: + - * / sqrt and
// comparisons only, every sum in the order written here.

// E (row-major, dst^T E src = 0, E ~ [t]x R with X_cur = R X_ref + t) -> the two rotations and the unit baseline of its
// four candidates (Ra, +th), (Ra, -th), (Rb, +th), (Rb, -th).  Eigenvectors of E^T E ordered as project_essential orders
// them; u_a = E v_a / s_a, u3 = u1 x u2, v3 = v1 x v2 (det U = det V = +1 by construction), Ra = U W V^T, Rb = U W^T V^T.
// false: no second singular value (NaN, all zero, rank 1) or no u3.  A matrix that is not exactly essential is decomposed
// all the same.
__host__ __device__ inline bool two_view_decompose(const double* E, double* Ra, double* Rb, double* th) {
  double B[3][3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + E[3 * k + r] * E[3 * k + c];
      B[r][c] = acc;
    }
  jacobi_eig<3>(B, V);
  int o[3] = {0, 1, 2};  // eigenvalues in descending order (stable selection)
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (B[o[b]][o[b]] > B[o[a]][o[a]]) {
        const int t = o[a];
        o[a] = o[b];
        o[b] = t;
      }
  const double l1 = B[o[0]][o[0]], l2 = B[o[1]][o[1]];
  if (!(l2 > 1e-300)) return false;
  double u[3][3], v[3][3];
  for (int a = 0; a < 2; ++a) {
    const double sv = sqrt(a == 0 ? l1 : l2);
    for (int r = 0; r < 3; ++r) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = acc + E[3 * r + k] * V[k][o[a]];
      u[a][r] = acc / sv;
      v[a][r] = V[r][o[a]];
    }
  }
  for (int r = 0; r < 3; ++r) {
    const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
    u[2][r] = u[0][r1] * u[1][r2] - u[0][r2] * u[1][r1];
    v[2][r] = v[0][r1] * v[1][r2] - v[0][r2] * v[1][r1];
  }
  const double n3 = sqrt(u[2][0] * u[2][0] + u[2][1] * u[2][1] + u[2][2] * u[2][2]);
  if (!(n3 > 0.0)) return false;
  for (int r = 0; r < 3; ++r) {
    th[r] = u[2][r] / n3;
    for (int c = 0; c < 3; ++c) {
      Ra[3 * r + c] = (u[1][r] * v[0][c] - u[0][r] * v[1][c]) + u[2][r] * v[2][c];
      Rb[3 * r + c] = (u[0][r] * v[1][c] - u[1][r] * v[0][c]) + u[2][r] * v[2][c];
    }
  }
  return true;
}

// One correspondence (x, y) <-> (u, v), normalised coordinates, under the candidate (R, t): the midpoint rule of
// triangulate_kernel on the rays (x, y, 1) and (u, v, 1), then the tests a map point has to pass -- rays not parallel, both
// ray parameters positive, parallax (cos^2 of the ray angle below c2), positive depth in both views, squared reprojection
// error at most r2 in both views.  Every test is written as "not (condition)": a NaN anywhere is never good.  X: the point
// in the reference frame (defined when the result is true).
__host__ __device__ inline bool two_view_row(const double* R, const double* t, double x, double y, double u, double v, double c2,
                                             double r2, double* X) {
  const double b[3] = {u, v, 1.0};
  double a[3];
  for (int r = 0; r < 3; ++r) a[r] = R[3 * r] * x + R[3 * r + 1] * y + R[3 * r + 2] * 1.0;
  const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double at = a[0] * t[0] + a[1] * t[1] + a[2] * t[2], bt = b[0] * t[0] + b[1] * t[1] + b[2] * t[2];
  const double det = aa * bb - ab * ab;
  if (!(det > 1e-12 * aa * bb)) return false;
  const double l1 = (ab * bt - bb * at) / det, l2 = (aa * bt - ab * at) / det;
  if (!(l1 > 0.0) || !(l2 > 0.0)) return false;
  if (ab > 0.0 && ab * ab >= c2 * aa * bb) return false;
  double mc[3], xc[3];
  for (int r = 0; r < 3; ++r) mc[r] = ((l1 * a[r] + t[r]) + l2 * b[r]) / 2.0 - t[r];        // midpoint - t, cur frame
  for (int r = 0; r < 3; ++r) X[r] = R[r] * mc[0] + R[3 + r] * mc[1] + R[6 + r] * mc[2];    // R^T (.)
  for (int r = 0; r < 3; ++r) xc[r] = (R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]) + t[r];
  if (!(X[2] > 0.0) || !(xc[2] > 0.0)) return false;
  const double ex = X[0] / X[2] - x, ey = X[1] / X[2] - y, fx = xc[0] / xc[2] - u, fy = xc[1] / xc[2] - v;
  if (!(ex * ex + ey * ey <= r2) || !(fx * fx + fy * fy <= r2)) return false;
  return true;
}

// Unit quaternion [qx qy qz qw], qw >= 0, of a rotation matrix by Shepperd's rule: the largest of (trace, R00, R11, R22),
// the first on ties, picks the column of the symmetric 4 x 4 form that is built; it is normalised afterwards, so no
// square root of a pivot is needed.
__host__ __device__ inline void two_view_quat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  int pick = 0;
  double best = tr;
  if (R[0] > best) { best = R[0]; pick = 1; }
  if (R[4] > best) { best = R[4]; pick = 2; }
  if (R[8] > best) { best = R[8]; pick = 3; }
  double qx, qy, qz, qw;
  if (pick == 0) {
    qx = R[7] - R[5]; qy = R[2] - R[6]; qz = R[3] - R[1]; qw = 1.0 + tr;
  } else if (pick == 1) {
    qx = ((1.0 + R[0]) - R[4]) - R[8]; qy = R[1] + R[3]; qz = R[2] + R[6]; qw = R[7] - R[5];
  } else if (pick == 2) {
    qx = R[1] + R[3]; qy = ((1.0 - R[0]) + R[4]) - R[8]; qz = R[5] + R[7]; qw = R[2] - R[6];
  } else {
    qx = R[2] + R[6]; qy = R[5] + R[7]; qz = ((1.0 - R[0]) - R[4]) + R[8]; qw = R[3] - R[1];
  }
  const double n = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  if (qw < 0.0) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
  q[0] = qx / n; q[1] = qy / n; q[2] = qz / n; q[3] = qw / n;
}

// A 7-double T_wc pose [qx qy qz qw tx ty tz] is a usable start of the pose refinement when every value is finite and the
// quaternion's sum of squares is > 0 (gh_ba_pnp does not renormalise a start, so neither is it done here).
__host__ __device__ inline bool pnp_start_ok(const double* pose) {
  for (int k = 0; k < 7; ++k)
    if (!(pose[k] - pose[k] == 0.0)) return false;  // NaN and +-Inf fail
  return pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3] > 0.0;
}

// The model of GH_MODEL_PNP ([R row-major | t], X_cam = R X + t) as the T_wc pose gh_ba_pnp starts from: q = the quaternion
// of R^T by two_view_quat, t_wc = -R^T t.  false (pose7 all zero) when a value of the model is not finite, when R is all
// zero (the estimator's "no model" is 12 zeros; Shepperd's column of a zero matrix would be the identity quaternion) or when
// the converted pose fails pnp_start_ok.
__host__ __device__ inline bool pnp_pose_from_model(const double* m, double* pose) {
  bool finite = true, zero = true;
  for (int k = 0; k < 12; ++k)
    if (!(m[k] - m[k] == 0.0)) finite = false;
  for (int k = 0; k < 9; ++k)
    if (m[k] != 0.0) zero = false;
  const double Rt[9] = {m[0], m[3], m[6], m[1], m[4], m[7], m[2], m[5], m[8]};
  const double* t = m + 9;
  double out[7];
  two_view_quat(Rt, out);
  for (int i = 0; i < 3; ++i) out[4 + i] = -((m[i] * t[0] + m[3 + i] * t[1]) + m[6 + i] * t[2]);
  const bool ok = finite && !zero && pnp_start_ok(out);
  for (int k = 0; k < 7; ++k) pose[k] = ok ? out[k] : 0.0;
  return ok;
}

}  // namespace gh_ransac
