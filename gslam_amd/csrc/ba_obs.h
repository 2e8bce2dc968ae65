// Per-observation arithmetic of the bundle adjustment kernels: the residual, its Huber weight and its Jacobians for one
// pinhole observation of a world point by a T_wc pose, and the SE3 retraction the LM step applies.  Shared by ba.hip (the
// general solver, gh_ba_pnp, gh_ba_marginalize) and pnp_batch.hip (the batched pose refinement): one text, so the same bits.
// Compile every file that includes this with -ffp-contract=off (the project's flags): the oracle rounds that way.
#pragma once
#include "common.h"

namespace gh_ba {

constexpr double kMinDepth = 1e-9;

struct Obs {
  double r[2], w, s;
  double Jc[12], Jp[6];
};

__device__ __forceinline__ void quat_rotate(const double* q, const double* p, double* o) {
  double uvx = q[1] * p[2] - q[2] * p[1], uvy = q[2] * p[0] - q[0] * p[2], uvz = q[0] * p[1] - q[1] * p[0];
  uvx += uvx; uvy += uvy; uvz += uvz;
  o[0] = p[0] + q[3] * uvx + (q[1] * uvz - q[2] * uvy);
  o[1] = p[1] + q[3] * uvy + (q[2] * uvx - q[0] * uvz);
  o[2] = p[2] + q[3] * uvz + (q[0] * uvy - q[1] * uvx);
}

__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// T <- T * exp([v, w]) with guarded coefficients (the reference's SE3::exp is NaN at w == 0)
__device__ inline void se3_retract(const double* pose, const double* xi, double* out) {
  const double* v = xi;
  const double* w = xi + 3;
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double th = sqrt(th2);
  double imag, real, A, B;
  if (th < 1e-5) {
    const double th4 = th2 * th2;
    imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
    real = 1.0 - th2 / 8.0 + th4 / 384.0;
    A = 0.5 - th2 / 24.0 + th4 / 720.0;
    B = 1.0 / 6.0 - th2 / 120.0 + th4 / 5040.0;
  } else {
    imag = sin(0.5 * th) / th;
    real = cos(0.5 * th);
    A = (1.0 - cos(th)) / th2;
    B = (th - sin(th)) / (th2 * th);
  }
  double e[7];
  e[0] = imag * w[0]; e[1] = imag * w[1]; e[2] = imag * w[2]; e[3] = real;
  const double c1[3] = {w[1] * v[2] - w[2] * v[1], w[2] * v[0] - w[0] * v[2], w[0] * v[1] - w[1] * v[0]};
  const double c2[3] = {w[1] * c1[2] - w[2] * c1[1], w[2] * c1[0] - w[0] * c1[2], w[0] * c1[1] - w[1] * c1[0]};
  for (int i = 0; i < 3; ++i) e[4 + i] = v[i] + A * c1[i] + B * c2[i];
  double q[4], t[3];
  quat_mul(pose, e, q);
  quat_rotate(pose, e + 4, t);
  const double nrm = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) out[i] = q[i] * nrm;
  for (int i = 0; i < 3; ++i) out[4 + i] = pose[4 + i] + t[i];
}

// residual / weight / Jacobians of one observation; false if the point is not in front of the camera
template <bool WITH_J>
__device__ __forceinline__ bool linearize(const double* pose, int dof, const double* X, int pfree, const double* m,
                                          const double* info, double huber, Obs& o) {
  const double qc[4] = {-pose[0], -pose[1], -pose[2], pose[3]};
  const double d[3] = {X[0] - pose[4], X[1] - pose[5], X[2] - pose[6]};
  double Xc[3];
  quat_rotate(qc, d, Xc);
  if (!(Xc[2] > kMinDepth)) return false;
  const double iz = 1.0 / Xc[2];
  const double u = Xc[0] * iz, v = Xc[1] * iz;
  o.r[0] = u - m[0];
  o.r[1] = v - m[1];
  double L00 = 1, L01 = 0, L10 = 0, L11 = 1;
  if (info) { L00 = info[0]; L01 = info[1]; L10 = info[2]; L11 = info[3]; }
  const double s = o.r[0] * (L00 * o.r[0] + L01 * o.r[1]) + o.r[1] * (L10 * o.r[0] + L11 * o.r[1]);
  double w = 1.0;
  if (huber > 0 && s > huber * huber) w = huber / sqrt(s);
  o.w = w;
  o.s = s;
  if (!WITH_J) return true;
  const double P[6] = {iz, 0, -u * iz, 0, iz, -v * iz};
  const double D[18] = {-1, 0, 0, 0, -Xc[2], Xc[1],
                        0, -1, 0, Xc[2], 0, -Xc[0],
                        0, 0, -1, -Xc[1], Xc[0], 0};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double acc = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) acc += P[a * 3 + j] * D[j * 6 + k];
      o.Jc[a * 6 + k] = ((dof >> k) & 1) ? acc : 0.0;
    }
  const double x = pose[0], y = pose[1], z = pose[2], qw = pose[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - qw * z), 2 * (x * z + qw * y),
                       2 * (x * y + qw * z), 1 - 2 * (x * x + z * z), 2 * (y * z - qw * x),
                       2 * (x * z - qw * y), 2 * (y * z + qw * x), 1 - 2 * (x * x + y * y)};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double acc = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) acc += P[a * 3 + j] * R[k * 3 + j];  // R^T[j][k] = R[k][j]
      o.Jp[a * 3 + k] = pfree ? acc : 0.0;
    }
  return true;
}

__device__ __forceinline__ void weighted_info(const double* info, double w, double* L) {
  L[0] = w; L[1] = 0; L[2] = 0; L[3] = w;
  if (info) { L[0] = w * info[0]; L[1] = w * info[1]; L[2] = w * info[2]; L[3] = w * info[3]; }
}

}  // namespace gh_ba
