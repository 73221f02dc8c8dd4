// Stand-alone driver of cutAsmSegments (robust_cvd_amd/csrc/cvd_asm_segments.h, included alone) for tests/test_assembly_segments_host.py.
// stdin:  waves unitSize P U Q, then P lines "a b count" (the pair list; offsets are the running sum), U lines "code offset" (units),
//         Q lines "u0 u1" (parts in launch order).
// stdout: "W off..." (the (part, wave) offsets), then one line "S other side first count last" per segment.
#include <cstdio>
#include <vector>

#include "../robust_cvd_amd/csrc/cvd_asm_segments.h"

int main() {
  int waves = 0, unitSize = 0, P = 0, U = 0, Q = 0;
  if (std::scanf("%d %d %d %d %d", &waves, &unitSize, &P, &U, &Q) != 5) return 1;
  std::vector<int32_t> pairA(P), pairB(P);
  std::vector<long long> pairOff(P + 1, 0);
  for (int p = 0; p < P; ++p) {
    long long n = 0;
    if (std::scanf("%d %d %lld", &pairA[p], &pairB[p], &n) != 3) return 1;
    pairOff[p + 1] = pairOff[p] + n;
  }
  std::vector<cvd::AsmUnitDesc> units(U);
  for (int u = 0; u < U; ++u)
    if (std::scanf("%d %d", &units[u].code, &units[u].offset) != 2) return 1;
  std::vector<cvd::AsmUnitRange> parts(Q);
  for (int q = 0; q < Q; ++q)
    if (std::scanf("%d %d", &parts[q].u0, &parts[q].u1) != 2) return 1;
  std::vector<cvd::AsmSegment> seg;
  std::vector<int32_t> waveOff;
  cvd::cutAsmSegments(parts, units, pairA.data(), pairB.data(), pairOff.data(), waves, unitSize, seg, waveOff);
  std::printf("W");
  for (const int32_t o : waveOff) std::printf(" %d", o);
  std::printf("\n");
  for (const cvd::AsmSegment& s : seg) std::printf("S %d %d %lld %d %d\n", s.other, s.side, s.first, s.count, s.last);
  return 0;
}
