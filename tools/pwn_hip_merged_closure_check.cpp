// pwn_hip_merged_closure_check -- PwnCloserWithMerger::processPartition of the C++ host mirror against the relations the Python mirror
// returned on the same input (tests/test_gpu_merged_partition.py writes the file).  Frame 0 is `current`, the others the other partition.
// The accepted / rejected decision, the number of relations, their nodes and image counts must be equal, the transforms equal to 1e-12
// (both mirrors run the same double loops on bitwise equal alignments).  Exits 0 when nothing differs, 1 on a difference, 2 on an error.
//
//   pwn_hip_merged_closure_check closure.bin
//
// File (little endian): int32 rows, cols, frames, frameMinNonZeroThreshold; float64 K[4] (fx fy cx cy); per frame float64 pose[16] (row-major)
// and float32 depth[rows*cols]; int32 accepted (1 / 0 / -1), relations; per relation int32 key of nodes[0], nodes[1], float64 transform[16]
// (row-major), int32 image_nonZeros, image_outliers, image_inliers.
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_merged_closure_check.cpp -o tools/pwn_hip_merged_closure_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

template <typename T> static bool get(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_merged_closure_check closure.bin" << std::endl; return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
  int head[4]; double Kd[4];
  if (!get(f, head, 4) || !get(f, Kd, 4) || head[0] <= 0 || head[1] <= 0 || head[2] < 2) { std::cerr << "bad header" << std::endl; return 2; }
  const int rows = head[0], cols = head[1], n = head[2];
  std::vector<MapNode> nodes((size_t)n);
  std::vector<DepthImage> frames((size_t)n);
  for (int k = 0; k < n; ++k) {
    nodes[k].key = k;
    frames[k].create(rows, cols);
    if (!get(f, nodes[k].transform.m, 16) || !get(f, frames[k].data.data(), frames[k].data.size())) { std::cerr << "short file" << std::endl; return 2; }
  }
  int tail[2];
  if (!get(f, tail, 2) || tail[1] < 0) { std::cerr << "short file" << std::endl; return 2; }
  struct Expected { int keys[2]; double T[16]; int counts[3]; };
  std::vector<Expected> expected((size_t)tail[1]);
  for (Expected& e : expected)
    if (!get(f, e.keys, 2) || !get(f, e.T, 16) || !get(f, e.counts, 3)) { std::cerr << "short file" << std::endl; return 2; }
  std::fclose(f);

  try {
    Context ctx(0, rows, cols, 16);
    ctx.setOmegaStorage(PWN_HIP_OMEGA_EXACT9);
    // the 120 x 160 configuration of the tests (pwn_core/conf/pwn_aligner_1_4.conf), projector range (0.01, 6), matcher at scale 1
    PinholePointProjector projector;
    Matrix3f K; K(0,0) = (float)Kd[0]; K(1,1) = (float)Kd[1]; K(0,2) = (float)Kd[2]; K(1,2) = (float)Kd[3]; K(2,2) = 1.f;
    projector.setCameraMatrix(K); projector.setMinDistance(0.01f); projector.setMaxDistance(6.0f); projector.setImageSize(rows, cols);
    StatsCalculatorIntegralImage stats;
    stats.setWorldRadius(0.1f); stats.setMinImageRadius(3); stats.setMaxImageRadius(6); stats.setMinPoints(10); stats.setCurvatureThreshold(0.2f);
    PointInformationMatrixCalculator pinfo; NormalInformationMatrixCalculator ninfo;
    pinfo.setCurvatureThreshold(0.02f); ninfo.setCurvatureThreshold(0.02f);
    DepthImageConverterIntegralImage converter(&ctx, &projector, &stats, &pinfo, &ninfo);
    CorrespondenceFinder finder;
    finder.setInlierDistanceThreshold(0.5f); finder.setInlierNormalAngularThreshold(0.95f); finder.setFlatCurvatureThreshold(0.02f);
    finder.setInlierCurvatureRatioThreshold(1.3f); finder.setImageSize(rows, cols);
    Linearizer linearizer; linearizer.setInlierMaxChi2(9000.f); linearizer.setRobustKernel(true);
    Aligner aligner(&ctx);
    aligner.setProjector(&projector); aligner.setLinearizer(&linearizer); aligner.setCorrespondenceFinder(&finder);
    aligner.setOuterIterations(10); aligner.setInnerIterations(1);
    PwnMatcherBase matcher(&ctx, &aligner, &converter);
    matcher.setScale(1);
    CloudCache cache(&matcher, 16);
    for (int k = 0; k < n; ++k) cache.addFrame(k, frames[k], K, Isometry3f::Identity());
    Merger2 merger(&ctx, &converter, &matcher);
    PwnCloserWithMerger closer(&ctx, &merger, &cache);
    closer.frameMinNonZeroThreshold = head[3];

    std::vector<const MapNode*> others;
    for (int k = 1; k < n; ++k) others.push_back(&nodes[k]);
    const std::vector<PwnCloserWithMerger::Relation> relations = closer.processPartition(others, &nodes[0]);

    int bad = 0;
    if (closer.accepted != tail[0]) { std::cerr << "accepted = " << closer.accepted << ", expected " << tail[0] << std::endl; ++bad; }
    if (relations.size() != expected.size()) { std::cerr << relations.size() << " relations, expected " << expected.size() << std::endl; ++bad; }
    double worst = 0.0;
    for (size_t i = 0; i < relations.size() && i < expected.size(); ++i) {
      const PwnCloserWithMerger::Relation& r = relations[i]; const Expected& e = expected[i];
      if (r.nodes[0]->key != e.keys[0] || r.nodes[1]->key != e.keys[1]) { std::cerr << "relation " << i << ": nodes differ" << std::endl; ++bad; }
      if (r.result.image_nonZeros != e.counts[0] || r.result.image_outliers != e.counts[1] || r.result.image_inliers != e.counts[2]) {
        std::cerr << "relation " << i << ": image counts " << r.result.image_nonZeros << " " << r.result.image_outliers << " " << r.result.image_inliers << " differ" << std::endl; ++bad;
      }
      double d = 0.0;
      for (int k = 0; k < 16; ++k) d = std::fmax(d, std::fabs(r.transform.m[k] - e.T[k]));
      if (!(d <= 1e-12)) { std::cerr << "relation " << i << ": transform differs by " << d << std::endl; ++bad; }
      worst = std::fmax(worst, d);
      for (int k = 0; k < 36; ++k) if (r.informationMatrix[k] != ((k % 7 == 0) ? (k < 21 ? 100.0 : 1000.0) : 0.0)) { std::cerr << "relation " << i << ": information matrix" << std::endl; ++bad; break; }
    }
    std::cout << n << " frames " << rows << "x" << cols << ": accepted " << closer.accepted << ", " << relations.size() << " relations, largest transform difference "
              << worst << ", " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
