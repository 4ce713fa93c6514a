// MapCloser::validatePartitions of the C++ mirror against what the Python mirror wrote to a file: the poses of two partitions, the relations
// that join them with their counters, and per validation the store, the decisions and the counters afterwards.  Prints " N differences";
// exit status 0 = none.
//
// File (little endian): int32 nCurrent, nOther, nRelations, consistent, minTimesChecked, validations; float32 translational, rotational
// threshold; nCurrent + nOther poses (16 doubles, row-major); per relation: int32 nodes[0] is in current (1) or in other (0), int32 index of
// nodes[0], of nodes[1] (in the other set), 16 doubles transform (row-major), int32 consensusTimeChecked, consensusCumInlier,
// consensusCumOutlierTimes; per validation: int32 n relations in the store before it, then per such relation, in store order: int32 its index,
// decision (0 skipped, 1 committed, 2 removed), the three counters after the call.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

static FILE* f;
template <typename T> static T rd() { T v; if (std::fread(&v, sizeof(T), 1, f) != 1) { std::fprintf(stderr, "short file\n"); std::exit(2); } return v; }
static Isometry3d rdIso() { Isometry3d T; for (int i = 0; i < 16; ++i) T.m[i] = rd<double>(); return T; }

int main(int argc, char** argv) {
  if (argc < 2 || !(f = std::fopen(argv[1], "rb"))) { std::fprintf(stderr, "usage: %s file\n", argv[0]); return 2; }
  const int nCur = rd<int>(), nOth = rd<int>(), nRel = rd<int>(), consistent = rd<int>(), minTimes = rd<int>(), validations = rd<int>();
  const float thrT = rd<float>(), thrR = rd<float>();
  std::vector<MapNode> cur(nCur), oth(nOth);
  for (int i = 0; i < nCur; ++i) { cur[i].key = i; cur[i].transform = rdIso(); }
  for (int i = 0; i < nOth; ++i) { oth[i].key = nCur + i; oth[i].transform = rdIso(); }
  int differences = 0;
  try {
    Context ctx(0, 120, 160, 1);
    MapCloser closer(&ctx, consistent != 0);
    closer.setConsensusInlierTranslationalThreshold(thrT); closer.setConsensusInlierRotationalThreshold(thrR); closer.setConsensusMinTimesCheckedThreshold(minTimes);
    std::vector<MapCloser::Relation*> byIndex(nRel);
    for (int k = 0; k < nRel; ++k) {
      const int firstInCurrent = rd<int>(), i0 = rd<int>(), i1 = rd<int>();
      MapCloser::Relation r;
      r.nodes[0] = firstInCurrent ? &cur[i0] : &oth[i0]; r.nodes[1] = firstInCurrent ? &oth[i1] : &cur[i1];
      r.transform = rdIso();
      for (double& v : r.informationMatrix) v = 0.0;
      r.consensusTimeChecked = rd<int>(); r.consensusCumInlier = rd<int>(); r.consensusCumOutlierTimes = rd<int>();
      byIndex[k] = closer.addRelation(r);
    }
    std::vector<const MapNode*> current, other;
    for (const MapNode& n : cur) current.push_back(&n);
    for (const MapNode& n : oth) other.push_back(&n);
    for (int v = 0; v < validations; ++v) {
      const int n = rd<int>();
      if (n != (int)closer.relations().size()) { ++differences; std::printf("validation %d: %zu relations in the store, the file has %d\n", v, closer.relations().size(), n); }
      std::vector<MapCloser::Relation*> live;
      for (const MapCloser::Relation& r : closer.relations()) live.push_back(const_cast<MapCloser::Relation*>(&r));
      MapCloser::Validation res = closer.validatePartitions(other, current);
      size_t removedSeen = 0;
      for (int k = 0; k < n; ++k) {
        const int index = rd<int>(), decision = rd<int>(), tcheck = rd<int>(), cin = rd<int>(), cout = rd<int>();
        if (k >= (int)live.size()) continue;
        if (index < 0 || index >= nRel || byIndex[index] != live[k]) { ++differences; std::printf("validation %d: store position %d holds another relation\n", v, k); continue; }
        bool committed = false;
        for (MapCloser::Relation* c : res.committed) committed = committed || c == live[k];
        // a removed relation has left the store: its counters are those of the copy handed back, in order
        const MapCloser::Relation* r = live[k];
        int mine = committed ? 1 : 0;
        if (decision == 2) {
          if (removedSeen < res.removed.size()) { r = &res.removed[removedSeen++]; mine = 2; } else { ++differences; std::printf("validation %d: relation %d was not removed\n", v, index); continue; }
        }
        if (mine != decision || r->consensusTimeChecked != tcheck || r->consensusCumInlier != cin || r->consensusCumOutlierTimes != cout) {
          ++differences;
          std::printf("validation %d relation %d: decision %d counters %d %d %d, the file has %d, %d %d %d\n", v, index, mine, r->consensusTimeChecked,
                      r->consensusCumInlier, r->consensusCumOutlierTimes, decision, tcheck, cin, cout);
        }
      }
      if (removedSeen != res.removed.size()) { ++differences; std::printf("validation %d: %zu relations removed, the file has %zu\n", v, res.removed.size(), removedSeen); }
    }
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 3;
  }
  std::printf(" %d differences\n", differences);
  return differences ? 1 : 0;
}
