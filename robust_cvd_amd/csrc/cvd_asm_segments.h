// cvd_asm_segments.h -- the segment list of k_assemble_fast's specialised list-mode walk (plain C++: host and device units include
// it, and tests/asm_segments_main.cpp includes it alone).
//
// The work list gives a part (one workgroup) a range of units, a unit being at most `unitSize` consecutive constraints of one
// (pair, side) entry of the part's frame.  The unit loop deals a part's units to the workgroup's waves round-robin, so a wave pays
// the header chase of a unit (descriptor -> pair -> other frame's constants and parameters) for every 128 constraints, and the units
// of one entry land on different waves.  Here a part's range is cut into one CONTIGUOUS run of units per wave (unit counts within
// one of each other), and a wave's run into SEGMENTS: maximal runs of constraints of one entry.  Whatever a wave needs to walk a
// segment is in its 32-byte record, so nothing is chased: the other frame, the own frame's role, the absolute first constraint, the
// count, and whether the wave's run ends with it.
#pragma once

#include <cstdint>
#include <vector>

namespace cvd {

struct alignas(32) AsmSegment {
  int32_t other;   // the other frame of the pair
  int32_t side;    // 0: the part's frame is the source of the pair, 1: the target
  long long first; // absolute index of the first constraint (table order)
  int32_t count;   // constraints, > 0
  int32_t last;    // 1: the last segment of its wave
  int32_t pad[2];
};
static_assert(sizeof(AsmSegment) == 32, "one scalar load per segment");

// Segment list of a launch: the segments of (part, wave) are seg[waveOff[part * waves + wave] .. waveOff[part * waves + wave + 1]);
// a wave without units has none.  depth: staging rows per wave the launch uses (cvd_eval.hip).
struct AsmSegs {
  const AsmSegment* seg;
  const int32_t* waveOff;
  int32_t depth;
};

struct AsmUnitRange { int32_t u0, u1; };   // a part's units [u0, u1)
struct AsmUnitDesc { int32_t code, offset; };  // pair * 2 + side, first constraint relative to the pair's offset

// parts: in launch order (the index of waveOff follows it).  pairA / pairB / pairOff: the table's pair list.
inline void cutAsmSegments(const std::vector<AsmUnitRange>& parts, const std::vector<AsmUnitDesc>& units, const int32_t* pairA,
                           const int32_t* pairB, const long long* pairOff, int waves, int unitSize, std::vector<AsmSegment>& seg,
                           std::vector<int32_t>& waveOff) {
  seg.clear();
  waveOff.assign(parts.size() * static_cast<size_t>(waves) + 1, 0);
  for (size_t q = 0; q < parts.size(); ++q) {
    const int nu = parts[q].u1 - parts[q].u0;
    const int base = nu / waves, rem = nu % waves;
    int u = parts[q].u0;
    for (int w = 0; w < waves; ++w) {
      const int uEnd = u + base + (w < rem ? 1 : 0);
      const size_t segBegin = seg.size();
      int lastCode = -1;
      for (; u < uEnd; ++u) {
        const int p = units[u].code >> 1, side = units[u].code & 1;
        const long long first = pairOff[p] + units[u].offset;
        const long long left = pairOff[p + 1] - first;
        const int32_t n = static_cast<int32_t>(left < unitSize ? left : unitSize);
        if (units[u].code == lastCode && seg.back().first + seg.back().count == first) {  // the same entry goes on
          seg.back().count += n;
          continue;
        }
        lastCode = units[u].code;
        AsmSegment s{};
        s.other = side ? pairA[p] : pairB[p];
        s.side = side;
        s.first = first;
        s.count = n;
        seg.push_back(s);
      }
      if (seg.size() > segBegin) seg.back().last = 1;
      waveOff[q * waves + w + 1] = static_cast<int32_t>(seg.size());
    }
  }
}

}  // namespace cvd
