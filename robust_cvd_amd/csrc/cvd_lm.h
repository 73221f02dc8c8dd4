// cvd_lm.h -- the two host-side policies of the Levenberg-Marquardt driver (cvd_solve.hip: solve) as plain arithmetic on a handful
// of ints and doubles: Ceres' trust-region radius rule and the schedule that decides when the preconditioner's levels are rebuilt.
// No HIP header and no handle: tests/test_lm_policy.py compiles this file alone with the host compiler.
// (The oracle's own LM loop, oracle/cvd_oracle.cpp, is an independent restatement and shares no code with this file.)
#pragma once

#include <algorithm>
#include <cmath>

namespace cvd {

struct Ceres {  // ceres::Solver::Options defaults used on this path
  static constexpr double initial_radius = 1e4, max_radius = 1e16, min_radius = 1e-32;
  static constexpr double min_relative_decrease = 1e-3;
  static constexpr double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  static constexpr int max_consecutive_invalid = 5;
};

// LevenbergMarquardtStrategy's radius (StepAccepted / StepRejected / StepIsInvalid) and TrustRegionMinimizer's stop tests.
struct TrustRegion {
  double radius = Ceres::initial_radius;
  double decrease = 2.0;
  int invalid = 0;  // consecutive steps whose model decrease was not a positive finite number

  bool belowMinRadius() const { return radius < Ceres::min_radius; }
  void accept(double q) {  // q: the step's relative decrease (> min_relative_decrease)
    radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * q - 1.0, 3));
    radius = std::min(Ceres::max_radius, radius);
    decrease = 2.0;
  }
  void reject() {
    radius /= decrease;
    decrease *= 2.0;
  }
  // false: too many in a row, the solve gives up (the radius stays); true: the step counts as rejected
  bool invalidStep() {
    if (++invalid >= Ceres::max_consecutive_invalid) return false;
    reject();
    return true;
  }
  void validStep() { invalid = 0; }
  static bool parameterToleranceReached(double stepNorm, double xNorm) {
    return stepNorm <= Ceres::parameter_tolerance * (xNorm + Ceres::parameter_tolerance);
  }
  static bool functionToleranceReached(double xCost, double candCost) {
    return std::abs(xCost - candCost) <= Ceres::function_tolerance * xCost;
  }
};

// Rebuild threshold of the DENSE coarse level (built in line) in PCG iterations.  excessDense = the option
// coarse_rebuild_excess_dense: > 0 fixes it; 0 (default) = 32, a constant: identical inputs must take identical rebuild decisions on
// every run and every rank (the wall-clock-derived threshold made PCG counts and end states depend on host jitter).
// -1 opts into pricing a rebuild at what THIS handle measured -- 1.5 x (the rebuild's duration / the duration of a PCG iteration of
// the running solves), in steps of 8 (the PCG counts of an LM run grow by themselves as the trust region opens: a threshold equal
// to the bare cost ratio, 22 at 300 frames, rebuilt every second LM iteration to save 0.6 iterations per LM iteration; 1.5 x = 32
// there).  Sharded runs ignore -1: every rank must decide alike.
inline int denseRebuildThreshold(int excessDense, bool dist, double rebuildMs, double pcgIterMs) {
  if (excessDense > 0) return excessDense;
  if (excessDense == 0 || dist || rebuildMs <= 0.0 || pcgIterMs <= 0.0) return 32;
  const double ratio = 1.5 * rebuildMs / pcgIterMs;
  return std::min(256, std::max(8, 8 * static_cast<int>(ratio / 8.0 + 0.5)));
}

// When the pose-graph level (coarse) and the depth-grid level (temporal) of the preconditioner are rebuilt.  Either is only a
// preconditioner: any SPD approximation serves, so a factor is kept across LM iterations (lagged lam and linearisation point).  A
// rebuild costs about as much as `threshold` PCG iterations; it is done once the iterations spent beyond the count observed right
// after the last rebuild add up to that (level 2: every LM iteration).
struct LevelSchedule {
  struct Config {           // fixed for one solve
    int coarseLevel;        // options coarse_level, temporal_level
    int temporalLevel;
    int threshold;          // PCG iterations: max(0, coarse_rebuild_excess), the dense form max(0, denseRebuildThreshold())
    bool coarseOn;          // this solve has a pose-graph level
    bool temporalOn;        // ... a depth-grid level
    bool denseMode;         // the pose-graph level in its dense form (one persistent kernel that wants every CU: always in line)
    bool dist;              // pair-sharded run
    bool stream3;           // a third stream exists
    bool smallBlock;        // frame block <= 256 unknowns
  };
  enum Rebuild { KEEP = 0, IN_LINE = 1, SIDE_STREAM = 2 };
  struct Decision {
    Rebuild coarse = KEEP;       // SIDE_STREAM: concurrently with this iteration's PCG (which keeps the old factor), for the next one
    bool inverseAside = false;   // the frames' block inverses on a stream of their own beside an in-line rebuild
    bool temporalOnly = false;   // the depth-grid level alone (no pose-graph level, or that level is kept)
  };
  // a side-stream rebuild only in the slowly changing regime: while the iterates still move a lot a factor that is one iteration
  // late costs more PCG iterations than the overlap saves
  static constexpr double asyncMaxChange = 1e-3;

  bool built = false;          // a factor of this solve exists
  bool pending = false;        // a rebuild is running on the side stream
  bool fresh = false;          // the factor was installed right before this iteration's PCG
  int cgAfterRefresh = 0;      // PCG iterations of the first solve with the factor in use
  int cgExcess = 0;            // ... spent beyond that count since
  double lastRelChange = 1.0;  // relative cost change of the last accepted step

  Decision decide(const Config& k) {  // once per LM iteration, before its PCG
    Decision d;
    const bool due = !built || cgExcess >= k.threshold;
    if (k.coarseOn) {
      const bool refresh = !pending && (k.coarseLevel == 2 || due);
      const bool aside = lastRelChange < asyncMaxChange && !k.denseMode && k.coarseLevel != 2 && !k.dist;
      if (refresh) d.coarse = aside ? SIDE_STREAM : IN_LINE;
      d.inverseAside = d.coarse == IN_LINE && !k.dist && k.stream3 && k.smallBlock;
      d.temporalOnly = !refresh && k.temporalOn && k.temporalLevel == 2;
    } else if (k.temporalOn) {
      d.temporalOnly = k.temporalLevel == 2 || due;
    }
    if (d.coarse == SIDE_STREAM) {
      pending = true;
      cgExcess = 0;
    } else if (d.coarse == IN_LINE || (!k.coarseOn && d.temporalOnly)) {
      built = true;
      fresh = true;
      cgExcess = 0;
    }
    return d;
  }
  void afterPcg(int cgIters) {
    if (fresh) cgAfterRefresh = cgIters;
    else cgExcess += std::max(0, cgIters - cgAfterRefresh);
    fresh = false;
  }
  void installed() {  // the side stream's factor was swapped in: the next PCG is its first
    pending = false;
    built = true;
    fresh = true;
    cgExcess = 0;
  }
  void accepted(double relChange) { lastRelChange = relChange; }
};

}  // namespace cvd
