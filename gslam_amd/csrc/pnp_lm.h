// Pose-only Levenberg-Marquardt inside ONE 256-thread workgroup: the body of gh_ba_pnp's single-launch kernel (ba.hip) and
// of the batched refinement (pnp_batch.hip).  Linearisation, the damped 6 x 6 solve on thread 0, candidate cost, accept /
// reject and the trust-region update, with fixed-shape block reductions: thread j adds observations j, j + 256, ... in that
// order, a wave adds its 64 lanes by the xor butterfly, the four waves are added in index order.  The sums therefore depend
// on the observations and their order alone -- which is what lets a batched problem equal, bit for bit, the single call on
// its compacted rows.
//   INDEXED  observation k is row rows[k] of X / M (a compacted list); otherwise row k.
//   TRACE    record the per-iteration trace of gh_ba_summary (the single call); otherwise nothing is traced.
#pragma once
#include "ba_obs.h"

namespace gh_ba {

struct PnpLmShared {
  double pose[7], dc[6], red[4][36], tot[36];
  double cost, radius, decrease;
  int ctl[4];  // [0] stop, [1] solve ok, [2] need_lin
};

struct PnpLmResult {  // valid on thread 0
  int iterations, accepted, termination;
  double initial_cost, final_cost;
};

// v[0..N) summed over the 256 threads of the block in a fixed order; the totals land in tot[0..N) (valid after return)
template <int N>
__device__ inline void pnp_block_sum(double* v, double (*red)[36], double* tot) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = v[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    if (lane == 0) red[wv][i] = x;
  }
  __syncthreads();
  if (threadIdx.x < N) tot[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  __syncthreads();
}

// S.pose holds the start (written and synchronised by the caller) and the result afterwards (visible to every thread).
// info_out (36 doubles, may be NULL): J^T W J at the solution.  trace: the summary whose trace_* fields TRACE fills.
// Every thread of the block must call this (it synchronises).
template <bool INDEXED, bool TRACE>
__device__ __forceinline__ void pnp_lm_body(PnpLmShared& S, const double* __restrict__ X, const double* __restrict__ M,
                                            const int32_t* rows, int n, int dof, const gh_ba_options& opt,
                                            double* __restrict__ info_out, gh_ba_summary* __restrict__ trace, PnpLmResult& res) {
  const int tid = threadIdx.x;
  const double huber = opt.huber_delta;
  auto row_of = [&](int k) -> size_t { return INDEXED ? (size_t)rows[k] : (size_t)k; };
  auto rho_of = [&](double s) { return (huber > 0 && s > huber * huber) ? 2.0 * huber * sqrt(s) - huber * huber : s; };
  // robust cost at `pose` (sum of rho, not yet halved); with `old`: infinite if an observation valid at `old` is lost
  auto cost_pass = [&](const double* pose, const double* old) {
    double c = 0;
    for (int k = tid; k < n; k += 256) {
      const size_t r = row_of(k);
      Obs o;
      const bool in_front = linearize<false>(pose, 0, X + 3 * r, 0, M + 2 * r, nullptr, huber, o);
      double ck = in_front ? rho_of(o.s) : 0.0;
      if (old != nullptr && !in_front && linearize<false>(old, 0, X + 3 * r, 0, M + 2 * r, nullptr, huber, o)) ck = __builtin_inf();
      c += ck;
    }
    return c;
  };
  double v[36];
  v[0] = cost_pass(S.pose, nullptr);
  pnp_block_sum<1>(v, S.red, S.tot);
  int accepted = 0, trace_len = 0;  // thread 0 keeps them
  if (tid == 0) {
    S.cost = 0.5 * S.tot[0];
    S.radius = opt.initial_radius;
    S.decrease = 2.0;
    S.ctl[0] = 0;
    S.ctl[2] = 1;
    res.initial_cost = S.cost;
  }
  __syncthreads();
  double H[21], g[6];  // lower triangle of J^T L J (row a >= column b at a (a + 1) / 2 + b) and J^T L r: thread 0 keeps them
  int it = 0, term = 0;
  for (it = 0; it < opt.max_iterations; ++it) {
    if (S.ctl[2]) {
      for (int i = 0; i < 27; ++i) v[i] = 0;
      for (int k = tid; k < n; k += 256) {
        const size_t r = row_of(k);
        Obs o;
        if (!linearize<true>(S.pose, dof, X + 3 * r, 0, M + 2 * r, nullptr, huber, o)) continue;
        double L[4];
        weighted_info(nullptr, o.w, L);
        const double Lr[2] = {L[0] * o.r[0] + L[1] * o.r[1], L[2] * o.r[0] + L[3] * o.r[1]};
        double LJ[12];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          LJ[j] = L[0] * o.Jc[j] + L[1] * o.Jc[6 + j];
          LJ[6 + j] = L[2] * o.Jc[j] + L[3] * o.Jc[6 + j];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          v[21 + a] += o.Jc[a] * Lr[0] + o.Jc[6 + a] * Lr[1];
#pragma unroll
          for (int b = 0; b <= a; ++b) v[a * (a + 1) / 2 + b] += o.Jc[a] * LJ[b] + o.Jc[6 + a] * LJ[6 + b];
        }
      }
      pnp_block_sum<27>(v, S.red, S.tot);
      if (tid == 0) {
        double gmax = 0;
        for (int i = 0; i < 21; ++i) H[i] = S.tot[i];
        for (int a = 0; a < 6; ++a) {
          g[a] = S.tot[21 + a];
          gmax = fmax(gmax, fabs(g[a]));
        }
        if (gmax <= opt.gradient_tolerance) S.ctl[0] = 2;  // termination 2, nothing recorded for this iteration
        S.ctl[2] = 0;
      }
      __syncthreads();
      if (S.ctl[0] == 2) {
        term = 2;
        break;
      }
    }
    if (tid == 0) {  // damped 6 x 6 system, Cholesky, dc = -(H + D)^-1 g
      const double radius = S.radius;
      double Lc[21];
      bool ok = true;
      for (int j = 0; j < 6 && ok; ++j) {
        const double hjj = H[j * (j + 1) / 2 + j];
        double d = hjj + (hjj < 1e-6 ? 1e-6 : (hjj > 1e32 ? 1e32 : hjj)) / radius;
        for (int k = 0; k < j; ++k) d -= Lc[j * (j + 1) / 2 + k] * Lc[j * (j + 1) / 2 + k];
        if (!(d > 0.0)) {
          ok = false;
          break;
        }
        const double ljj = sqrt(d);
        Lc[j * (j + 1) / 2 + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
          double x = H[i * (i + 1) / 2 + j];
          for (int k = 0; k < j; ++k) x -= Lc[i * (i + 1) / 2 + k] * Lc[j * (j + 1) / 2 + k];
          Lc[i * (i + 1) / 2 + j] = x / ljj;
        }
      }
      if (ok) {
        double y[6];
        for (int i = 0; i < 6; ++i) {
          double x = -g[i];
          for (int k = 0; k < i; ++k) x -= Lc[i * (i + 1) / 2 + k] * y[k];
          y[i] = x / Lc[i * (i + 1) / 2 + i];
        }
        for (int i = 5; i >= 0; --i) {
          double x = y[i];
          for (int k = i + 1; k < 6; ++k) x -= Lc[k * (k + 1) / 2 + i] * y[k];
          y[i] = x / Lc[i * (i + 1) / 2 + i];
        }
        for (int i = 0; i < 6; ++i) S.dc[i] = y[i];
      }
      S.ctl[1] = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = S.ctl[1] != 0;
    double pnew[7];
    if (ok) {
      double dc[6];
      for (int a = 0; a < 6; ++a) dc[a] = S.dc[a];
      if ((dof & 63) == 0) {
        for (int i = 0; i < 7; ++i) pnew[i] = S.pose[i];
      } else {
        double cur[7];
        for (int i = 0; i < 7; ++i) cur[i] = S.pose[i];
        se3_retract(cur, dc, pnew);
      }
      double model = 0;
      for (int k = tid; k < n; k += 256) {
        const size_t r = row_of(k);
        Obs o;
        if (!linearize<true>(S.pose, dof, X + 3 * r, 0, M + 2 * r, nullptr, huber, o)) continue;
        double L[4];
        weighted_info(nullptr, o.w, L);
        double Jd[2] = {0, 0};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          Jd[0] += o.Jc[a] * dc[a];
          Jd[1] += o.Jc[6 + a] * dc[a];
        }
        const double LJd[2] = {L[0] * Jd[0] + L[1] * Jd[1], L[2] * Jd[0] + L[3] * Jd[1]};
        const double Lr[2] = {L[0] * o.r[0] + L[1] * o.r[1], L[2] * o.r[0] + L[3] * o.r[1]};
        model -= Jd[0] * Lr[0] + Jd[1] * Lr[1] + 0.5 * (Jd[0] * LJd[0] + Jd[1] * LJd[1]);
      }
      v[0] = cost_pass(pnew, S.pose);
      v[1] = model;
      pnp_block_sum<2>(v, S.red, S.tot);
    }
    if (tid == 0) {  // the step rule of lm_rule.h (LmRule::step), restated for the device: keep the two alike
      const double cost = S.cost, radius = S.radius;
      double new_cost = cost, model = 0, rho = -1;
      if (ok) {
        new_cost = 0.5 * S.tot[0];
        model = S.tot[1];
        rho = model > 0 ? (cost - new_cost) / model : -1;
        if (!(new_cost == new_cost)) rho = -1;
      }
      const bool acc = ok && rho > opt.min_relative_decrease;
      if (TRACE && trace_len < GH_BA_MAX_TRACE) {
        trace->trace_cost[trace_len] = new_cost;
        trace->trace_radius[trace_len] = radius;
        trace->trace_accepted[trace_len] = (uint8_t)acc;
        ++trace_len;
      }
      if (acc) {
        const double dcost = cost - new_cost;
        for (int i = 0; i < 7; ++i) S.pose[i] = pnew[i];
        const double t = 2.0 * rho - 1.0;
        double r2 = radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
        if (r2 > 1e16) r2 = 1e16;
        S.radius = r2;
        S.decrease = 2.0;
        ++accepted;
        S.ctl[2] = 1;
        S.cost = new_cost;
        if (fabs(dcost) <= opt.function_tolerance * cost) S.ctl[0] = 1;
      } else {
        S.radius = radius / S.decrease;
        S.decrease = S.decrease * 2.0;
        if (S.radius < 1e-32) S.ctl[0] = 3;
      }
    }
    __syncthreads();
    if (S.ctl[0] != 0) {
      term = S.ctl[0];
      ++it;
      break;
    }
  }
  if (info_out) {  // J^T W J at the solution (columns masked by dof), W = the Huber IRLS weight
    for (int i = 0; i < 36; ++i) v[i] = 0;
    for (int k = tid; k < n; k += 256) {
      const size_t r = row_of(k);
      Obs o;
      if (!linearize<true>(S.pose, dof, X + 3 * r, 0, M + 2 * r, nullptr, huber, o)) continue;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) v[6 * a + b] += o.w * (o.Jc[a] * o.Jc[b] + o.Jc[6 + a] * o.Jc[6 + b]);
    }
    pnp_block_sum<36>(v, S.red, S.tot);
    if (tid < 36) info_out[tid] = S.tot[tid];
  }
  if (tid == 0) {
    res.iterations = it;
    res.accepted = accepted;
    res.termination = term;
    res.final_cost = S.cost;
    if (TRACE) trace->trace_len = trace_len;
  }
}

}  // namespace gh_ba
