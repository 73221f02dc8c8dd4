// Driver of tests/test_lm_policy.py: includes cvd_lm.h alone (host compiler, no HIP), reads a script of events from stdin and prints
// what the two policies answer -- doubles as hex floats, so that the test compares bits.
//   tr                      new TrustRegion                              -> R radius belowMin
//   accept Q | reject       StepAccepted(q) / StepRejected               -> R radius belowMin
//   invalid | valid         invalid step (G 1: give up) / valid step     -> G gaveUp, then R radius belowMin
//   ptol STEP X | ftol C CC the two stop tests                           -> B reached
//   thr OPT DIST RB PCG     denseRebuildThreshold                        -> T iterations
//   sched CL TL THR COARSE TEMPORAL DENSE DIST STREAM3 SMALLB            new LevelSchedule with this Config
//   rel X | pcg N | installed    accepted(x) / afterPcg(n) / installed() -> S built pending fresh cgAfterRefresh cgExcess
//   decide                  one LM iteration's decision                  -> D coarse inverseAside temporalOnly, then S ...
#include "../robust_cvd_amd/csrc/cvd_lm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main() {
  cvd::TrustRegion tr;
  cvd::LevelSchedule sched;
  cvd::LevelSchedule::Config cfg{};
  char line[512], cmd[32];
  auto printR = [&]() { std::printf("R %a %d\n", tr.radius, tr.belowMinRadius() ? 1 : 0); };
  auto printS = [&]() {
    std::printf("S %d %d %d %d %d\n", sched.built ? 1 : 0, sched.pending ? 1 : 0, sched.fresh ? 1 : 0, sched.cgAfterRefresh, sched.cgExcess);
  };
  while (std::fgets(line, sizeof(line), stdin)) {
    char a[64] = "", b[64] = "", c[64] = "", d[64] = "";
    int v[9] = {0}, n = 0;
    if (std::sscanf(line, "%31s%n", cmd, &n) != 1) continue;
    const char* rest = line + n;
    if (!std::strcmp(cmd, "tr")) { tr = cvd::TrustRegion(); printR(); }
    else if (!std::strcmp(cmd, "accept") && std::sscanf(rest, "%63s", a) == 1) { tr.accept(std::strtod(a, nullptr)); printR(); }
    else if (!std::strcmp(cmd, "reject")) { tr.reject(); printR(); }
    else if (!std::strcmp(cmd, "invalid")) { std::printf("G %d\n", tr.invalidStep() ? 0 : 1); printR(); }
    else if (!std::strcmp(cmd, "valid")) { tr.validStep(); std::printf("G 0\n"); printR(); }
    else if (!std::strcmp(cmd, "ptol") && std::sscanf(rest, "%63s %63s", a, b) == 2)
      std::printf("B %d\n", cvd::TrustRegion::parameterToleranceReached(std::strtod(a, nullptr), std::strtod(b, nullptr)) ? 1 : 0);
    else if (!std::strcmp(cmd, "ftol") && std::sscanf(rest, "%63s %63s", a, b) == 2)
      std::printf("B %d\n", cvd::TrustRegion::functionToleranceReached(std::strtod(a, nullptr), std::strtod(b, nullptr)) ? 1 : 0);
    else if (!std::strcmp(cmd, "thr") && std::sscanf(rest, "%63s %63s %63s %63s", a, b, c, d) == 4)
      std::printf("T %d\n", cvd::denseRebuildThreshold(std::atoi(a), std::atoi(b) != 0, std::strtod(c, nullptr), std::strtod(d, nullptr)));
    else if (!std::strcmp(cmd, "sched") &&
             std::sscanf(rest, "%d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
      sched = cvd::LevelSchedule();
      cfg = cvd::LevelSchedule::Config{v[0], v[1], v[2], v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0};
    }
    else if (!std::strcmp(cmd, "rel") && std::sscanf(rest, "%63s", a) == 1) { sched.accepted(std::strtod(a, nullptr)); printS(); }
    else if (!std::strcmp(cmd, "pcg") && std::sscanf(rest, "%d", v) == 1) { sched.afterPcg(v[0]); printS(); }
    else if (!std::strcmp(cmd, "installed")) { sched.installed(); printS(); }
    else if (!std::strcmp(cmd, "decide")) {
      const cvd::LevelSchedule::Decision dec = sched.decide(cfg);
      std::printf("D %d %d %d\n", static_cast<int>(dec.coarse), dec.inverseAside ? 1 : 0, dec.temporalOnly ? 1 : 0);
      printS();
    }
    else { std::fprintf(stderr, "bad script line: %s", line); return 2; }
  }
  return 0;
}
