// The Levenberg-Marquardt step rule of gh_ba_solve (ba.hip) and gh_graph_solve (posegraph.hip): gain ratio, accept /
// reject, trace, trust-region radius, termination.  The tests hold both solvers to the oracle's accept / reject sequence,
// so the rule exists once on the host (the single-launch PnP kernel of ba.hip carries its own device-side copy: keep the
// two alike).  Host code only (no HIP, no context): the arithmetic, the trace entry and the verbose line.  The expressions
// and their order are the oracle's, and every file that includes this is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gslam_hip.h"

struct LmRule {
  double cost = 0, radius = 0, decrease = 2.0;
  int term = 0;  // 0: go on; 1: function tolerance; 3: the radius fell below its floor (2, the gradient test, is the caller's)

  // Judge one trial step.  ok: the linear solve succeeded and the trial was evaluated (otherwise trial_cost and
  // model_decrease are ignored: callers may pass whatever the read-back block holds).  true: accepted -- `cost` is the
  // trial's now and the caller adopts the trial state.  `term` says whether the solve ends here.  tag: the solver's name
  // on the verbose line.
  bool step(const gh_ba_options& opt, gh_ba_summary* sum, const char* tag, int it, bool ok, double trial_cost, double model_decrease) {
    double new_cost = cost, model = 0, rho = -1;
    if (ok) {
      new_cost = trial_cost;
      model = model_decrease;
      rho = model > 0 ? (cost - new_cost) / model : -1;
      if (!(new_cost == new_cost)) rho = -1;  // NaN guard
    }
    const bool acc = ok && rho > opt.min_relative_decrease;
    if (sum->trace_len < GH_BA_MAX_TRACE) {
      sum->trace_cost[sum->trace_len] = new_cost;
      sum->trace_radius[sum->trace_len] = radius;
      sum->trace_accepted[sum->trace_len] = (uint8_t)acc;
      sum->trace_len++;
    }
    if (opt.verbose)
      fprintf(stderr, "[%s] it %3d cost %.9e -> %.9e model %.3e rho %.3f radius %.3e %s\n", tag, it, cost, new_cost, model, rho,
              radius, acc ? "accepted" : (ok ? "rejected" : "solve failed"));
    if (!acc) {
      radius = radius / decrease;
      decrease *= 2.0;
      if (radius < 1e-32) term = 3;
      return false;
    }
    const double dcost = cost - new_cost;
    const double t = 2.0 * rho - 1.0;
    radius = radius / fmax(1.0 / 3.0, 1.0 - t * t * t);
    if (radius > 1e16) radius = 1e16;
    decrease = 2.0;
    sum->accepted++;
    const double prev = cost;
    cost = new_cost;
    if (fabs(dcost) <= opt.function_tolerance * prev) term = 1;
    return true;
  }
};
