// pwn_hip_scaled_batch_check -- PwnMatcherBase::makeCloudBatch of the C++ host mirror against makeCloud called per frame: the same
// synthetic depth images go through both, every array of every cloud is downloaded and compared bit for bit.  Exits 0 when nothing
// differs, 1 on a difference, 2 on an error of the library.
//
//   pwn_hip_scaled_batch_check [rows cols scale frames]        (default 121 163 2 5)
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_scaled_batch_check.cpp -o tools/pwn_hip_scaled_batch_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

// a tilted floor, a back wall and a box in front of it, with 3 % dropouts; frame k looks at it from a little further to the right
static void synthetic_depth(DepthImage& img, int rows, int cols, int k) {
  img.create(rows, cols);
  uint32_t s = 12345u + 977u * (uint32_t)k;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      const float u = (c + 0.5f) / cols - 0.5f + 0.02f * k, v = (r + 0.5f) / rows - 0.5f;
      float d = 3.0f + 0.8f * u;                                        // wall
      if (v > 0.15f) d = std::min(d, 0.9f / (v + 0.15f));               // floor
      if (u > -0.2f && u < 0.1f && v > -0.2f && v < 0.2f) d = 1.6f + 0.3f * u;      // box
      s = s * 1664525u + 1013904223u;
      if ((s >> 8) % 100u < 3u) d = 0.f;
      img.data[(size_t)r * cols + c] = d;
    }
}

static int differing(const char* what, int frame, const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0)) return 0;
  std::cerr << "frame " << frame << ": " << what << " differ (" << a.size() << " / " << b.size() << " floats)" << std::endl;
  return 1;
}

int main(int argc, char** argv) {
  const int rows = argc > 1 ? std::atoi(argv[1]) : 121, cols = argc > 2 ? std::atoi(argv[2]) : 163;
  const int scale = argc > 3 ? std::atoi(argv[3]) : 2, n = argc > 4 ? std::atoi(argv[4]) : 5;
  if (rows <= 0 || cols <= 0 || scale <= 0 || n <= 0) { std::cerr << "USAGE: pwn_hip_scaled_batch_check [rows cols scale frames]" << std::endl; return 2; }
  try {
    Context ctx(0, rows, cols, 8);
    PinholePointProjector projector;
    projector.setMinDistance(0.5f); projector.setMaxDistance(4.5f);
    StatsCalculatorIntegralImage stats;
    stats.setMinImageRadius(3); stats.setMaxImageRadius(6); stats.setMinPoints(10); stats.setCurvatureThreshold(0.2f); stats.setWorldRadius(0.1f);
    PointInformationMatrixCalculator pinfo; NormalInformationMatrixCalculator ninfo;
    DepthImageConverterIntegralImage converter(&ctx, &projector, &stats, &pinfo, &ninfo);
    CorrespondenceFinder finder; Linearizer linearizer;
    Aligner aligner(&ctx);
    aligner.setProjector(&projector); aligner.setLinearizer(&linearizer); aligner.setCorrespondenceFinder(&finder);
    PwnMatcherBase matcher(&ctx, &aligner, &converter);
    matcher.setScale(scale);
    Matrix3f K; K(0,0) = 525.f * cols / 640.f; K(1,1) = 525.f * cols / 640.f; K(0,2) = (cols - 1) * 0.5f; K(1,2) = (rows - 1) * 0.5f; K(2,2) = 1.f;
    const Isometry3f sensorOffset;

    std::vector<DepthImage> frames((size_t)n);
    std::vector<const DepthImage*> ptrs((size_t)n);
    for (int k = 0; k < n; ++k) { synthetic_depth(frames[k], rows, cols, k); ptrs[k] = &frames[k]; }

    int r1 = 0, c1 = 0, rb = 0, cb = 0;
    std::vector<std::unique_ptr<Cloud>> single;
    Matrix3f K1;
    for (int k = 0; k < n; ++k) { K1 = K; single.emplace_back(matcher.makeCloud(r1, c1, K1, sensorOffset, frames[k])); }
    Matrix3f Kb = K;
    std::vector<std::unique_ptr<Cloud>> batch;
    for (Cloud* cl : matcher.makeCloudBatch(rb, cb, Kb, sensorOffset, ptrs)) batch.emplace_back(cl);

    int bad = 0;
    if (r1 != rb || c1 != cb || std::memcmp(K1.data(), Kb.data(), 9 * sizeof(float)) != 0) { std::cerr << "scaled size / camera matrix differ" << std::endl; ++bad; }
    if (matcher.numCalls != 2 * n) { std::cerr << "numCalls = " << matcher.numCalls << ", expected " << 2 * n << std::endl; ++bad; }
    if ((int)batch.size() != n) { std::cerr << "makeCloudBatch returned " << batch.size() << " clouds" << std::endl; return 1; }
    size_t points = 0;
    for (int k = 0; k < n; ++k) {
      const Cloud& a = *single[k]; const Cloud& b = *batch[k];
      points += b.size();
      bad += differing("points", k, a.points(), b.points());
      bad += differing("normals", k, a.normals(), b.normals());
      bad += differing("curvatures", k, a.curvatures(), b.curvatures());
      bad += differing("point information matrices", k, a.pointInformationMatrix(), b.pointInformationMatrix());
      bad += differing("normal information matrices", k, a.normalInformationMatrix(), b.normalInformationMatrix());
    }
    // DepthImage_scale of the run of images against the single-image form
    std::vector<DepthImage> scaledAll;
    DepthImage_scale(ctx, scaledAll, frames, scale);
    for (int k = 0; k < n; ++k) {
      DepthImage one; DepthImage_scale(ctx, one, frames[k], scale);
      bad += differing("scaled images", k, one.data, scaledAll[k].data);
    }
    if (points == 0) { std::cerr << "the synthetic frames gave no points" << std::endl; ++bad; }
    std::cout << n << " frames " << rows << "x" << cols << " at 1/" << scale << ": " << points << " points, " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
