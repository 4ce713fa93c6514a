// pwn_hip_scene_step_check -- SceneAligner of the C++ host mirror against what the Python mirror returned for the same frames
// (tests/test_scene_step_harness.py writes the file).  Per frame the aligner's transform, the scene pose, the global pose and the four counts,
// at the end the scene's size, its Gaussian count and six of its arrays must be equal byte for byte (both mirrors make the same call on the
// same device).  Exits 0 when nothing differs, 1 on a difference, 2 on an error.
//
//   pwn_hip_scene_step_check step.bin
//
// File (little endian): int32 rows, cols, frames; float64 K[4] (fx fy cx cy), min_distance, max_distance, inlier_distance_threshold; int32
// min_image_radius, max_image_radius, min_points; per frame float32 depth[rows*cols]; per frame float32 T[16], sceneT[16], globalT[16]
// (column-major) and int32 n_cloud, n_subscene, size_after_add, size_after_merge; int32 points and Gaussians of the scene; then six arrays, each
// int64 bytes + the bytes: points, normals, curvature, omega_p, omega_n, stats.
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_scene_step_check.cpp -o tools/pwn_hip_scene_step_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

template <typename T> static bool get(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }
struct FrameResult { float T[16], sceneT[16], globalT[16]; int counts[4]; };

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_scene_step_check step.bin" << std::endl; return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
  int head[3]; double Kd[4], conf[3]; int radii[3];
  if (!get(f, head, 3) || !get(f, Kd, 4) || !get(f, conf, 3) || !get(f, radii, 3) || head[0] <= 0 || head[1] <= 0 || head[2] < 1) { std::cerr << "bad header" << std::endl; return 2; }
  const int rows = head[0], cols = head[1], n = head[2];
  std::vector<DepthImage> frames((size_t)n);
  for (int k = 0; k < n; ++k) {
    frames[k].create(rows, cols);
    if (!get(f, frames[k].data.data(), frames[k].data.size())) { std::cerr << "short file" << std::endl; return 2; }
  }
  std::vector<FrameResult> expected((size_t)n);
  for (int k = 0; k < n; ++k)
    if (!get(f, expected[k].T, 16) || !get(f, expected[k].sceneT, 16) || !get(f, expected[k].globalT, 16) || !get(f, expected[k].counts, 4)) { std::cerr << "short file" << std::endl; return 2; }
  int sizes[2];
  if (!get(f, sizes, 2)) { std::cerr << "short file" << std::endl; return 2; }
  static const char* names[6] = { "points", "normals", "curvature", "omega_p", "omega_n", "stats" };
  std::vector<std::vector<char> > arrays(6);
  for (int a = 0; a < 6; ++a) {
    long long bytes = 0;
    if (!get(f, &bytes) || bytes < 0) { std::cerr << "short file" << std::endl; return 2; }
    arrays[a].resize((size_t)bytes);
    if (bytes && !get(f, arrays[a].data(), (size_t)bytes)) { std::cerr << "short file" << std::endl; return 2; }
  }
  std::fclose(f);

  try {
    Context ctx(0, rows, cols, 2);
    PinholePointProjector projector;
    Matrix3f K; K(0,0) = (float)Kd[0]; K(1,1) = (float)Kd[1]; K(0,2) = (float)Kd[2]; K(1,2) = (float)Kd[3]; K(2,2) = 1.f;
    projector.setCameraMatrix(K); projector.setMinDistance((float)conf[0]); projector.setMaxDistance((float)conf[1]); projector.setImageSize(rows, cols);
    StatsCalculatorIntegralImage stats;
    stats.setWorldRadius(0.1f); stats.setMinImageRadius(radii[0]); stats.setMaxImageRadius(radii[1]); stats.setMinPoints(radii[2]); stats.setCurvatureThreshold(0.2f);
    PointInformationMatrixCalculator pinfo; NormalInformationMatrixCalculator ninfo;
    pinfo.setCurvatureThreshold(0.02f); ninfo.setCurvatureThreshold(0.02f);
    DepthImageConverterIntegralImage converter(&ctx, &projector, &stats, &pinfo, &ninfo);
    CorrespondenceFinder finder;
    finder.setInlierDistanceThreshold((float)conf[2]); finder.setInlierNormalAngularThreshold(0.95f); finder.setFlatCurvatureThreshold(0.02f);
    finder.setInlierCurvatureRatioThreshold(1.3f); finder.setImageSize(rows, cols);
    Linearizer linearizer; linearizer.setInlierMaxChi2(9e3f); linearizer.setRobustKernel(true);
    Aligner aligner(&ctx);
    aligner.setProjector(&projector); aligner.setLinearizer(&linearizer); aligner.setCorrespondenceFinder(&finder);
    aligner.setOuterIterations(10); aligner.setInnerIterations(1);
    Merger merger; merger.setDepthImageConverter(&converter); merger.setImageSize(rows, cols);
    SceneAligner mapper(&ctx, &converter, &aligner, &merger, (n + 1) * rows * cols);
    int differences = 0;
    for (int k = 0; k < n; ++k) {
      const Isometry3f T = mapper.processFrame(frames[k]);
      const pwn_hip_scene_step_result& r = mapper.result();
      const int counts[4] = { r.n_cloud, r.n_subscene, r.size_after_add, r.size_after_merge };
      if (std::memcmp(T.data(), expected[k].T, 64) || std::memcmp(mapper.sceneT().data(), expected[k].sceneT, 64) ||
          std::memcmp(mapper.globalT().data(), expected[k].globalT, 64) || std::memcmp(counts, expected[k].counts, sizeof(counts))) {
        std::cerr << "frame " << k << " differs" << std::endl; ++differences;
      }
    }
    Cloud* scene = mapper.scene();
    if ((int)scene->size() != sizes[0] || (int)scene->numGaussians() != sizes[1]) { std::cerr << "scene size or Gaussian count differs" << std::endl; ++differences; }
    const std::vector<float> got[6] = { scene->points(), scene->normals(), scene->curvatures(), scene->pointInformationMatrix(), scene->normalInformationMatrix(), scene->stats() };
    for (int a = 0; a < 6; ++a)
      if (got[a].size() * sizeof(float) != arrays[a].size() || (arrays[a].size() && std::memcmp(got[a].data(), arrays[a].data(), arrays[a].size()))) {
        std::cerr << "scene array " << names[a] << " differs" << std::endl; ++differences;
      }
    std::cout << n << " frames, " << scene->size() << " points, " << differences << " differences" << std::endl;
    return differences ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
