// pwn_hip_early_stop_check -- "stop when converged" (include/pwn_hip.h: pwn_hip_ctx_set_convergence) through the C++ host mirror against what the
// Python mirror wrote to a file: the same raw frames are converted and aligned as one batch under the same setting (Context::setConvergence,
// Aligner::alignBatch, Aligner::lastSteps), and every pair's transform, iteration count, error, inliers and both step traces are compared bit for
// bit.  Exits 0 when nothing differs, 1 on a difference, 2 on an error of the library or of the file.
//
//   pwn_hip_early_stop_check FILE
//
// FILE (little-endian, written by tests/test_gpu_early_stop.py):
//   int32 n, rows, cols, outer_iterations, inner_iterations, min_iterations; float translation_epsilon, rotation_epsilon; float fx, fy, cx, cy
//   n x { uint16 reference frame [rows * cols] (millimetres), uint16 current frame [rows * cols] }
//   n x float guess[16] (column-major)
//   n x { float T[16]; int32 iterations; float error; int32 inliers; int32 outer_executed; int32 converged; float step_translation[64], step_rotation[64] }
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_early_stop_check.cpp -o tools/pwn_hip_early_stop_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

struct Header { int32_t n, rows, cols, outer, inner, minIterations; float epsT, epsR; float fx, fy, cx, cy; };
struct Expected { float T[16]; int32_t iterations; float error; int32_t inliers; int32_t outerExecuted; int32_t converged; float stepT[PWN_HIP_MAX_ITERATIONS], stepR[PWN_HIP_MAX_ITERATIONS]; };

template <typename T> static bool get(std::ifstream& f, T* dst, size_t count) { return (bool)f.read(reinterpret_cast<char*>(dst), (std::streamsize)(sizeof(T) * count)); }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_early_stop_check FILE" << std::endl; return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  Header h;
  if (!f || !get(f, &h, 1) || h.n <= 0 || h.rows <= 0 || h.cols <= 0) { std::cerr << "cannot read " << argv[1] << std::endl; return 2; }
  const size_t N = (size_t)h.rows * h.cols;
  std::vector<std::vector<uint16_t>> ref((size_t)h.n, std::vector<uint16_t>(N)), cur((size_t)h.n, std::vector<uint16_t>(N));
  for (int i = 0; i < h.n; ++i) if (!get(f, ref[i].data(), N) || !get(f, cur[i].data(), N)) { std::cerr << "short file (frames)" << std::endl; return 2; }
  std::vector<Isometry3f> guesses((size_t)h.n);
  for (int i = 0; i < h.n; ++i) { float g[16]; if (!get(f, g, 16)) { std::cerr << "short file (guesses)" << std::endl; return 2; } guesses[i] = Isometry3f(g); }
  std::vector<Expected> want((size_t)h.n);
  if (!get(f, want.data(), want.size())) { std::cerr << "short file (results)" << std::endl; return 2; }
  try {
    Context ctx(0, h.rows, h.cols, h.n);
    PinholePointProjector projector;
    Matrix3f K; K(0,0) = h.fx; K(1,1) = h.fy; K(0,2) = h.cx; K(1,2) = h.cy; K(2,2) = 1.f;
    projector.setCameraMatrix(K); projector.setMinDistance(0.5f); projector.setMaxDistance(4.5f); projector.setImageSize(h.rows, h.cols);
    StatsCalculatorIntegralImage stats;       // pwn_core/conf/pwn_aligner_1_4.conf
    stats.setMinImageRadius(3); stats.setMaxImageRadius(6); stats.setMinPoints(10); stats.setCurvatureThreshold(0.2f); stats.setWorldRadius(0.1f);
    PointInformationMatrixCalculator pinfo; NormalInformationMatrixCalculator ninfo;
    pinfo.setCurvatureThreshold(0.02f); ninfo.setCurvatureThreshold(0.02f);
    DepthImageConverterIntegralImage converter(&ctx, &projector, &stats, &pinfo, &ninfo);
    CorrespondenceFinder finder;
    finder.setInlierDistanceThreshold(0.5f); finder.setInlierNormalAngularThreshold(0.95f); finder.setFlatCurvatureThreshold(0.02f);
    finder.setInlierCurvatureRatioThreshold(1.3f); finder.setImageSize(h.rows, h.cols);
    Linearizer linearizer; linearizer.setInlierMaxChi2(9000.f); linearizer.setRobustKernel(true);
    Aligner aligner(&ctx);
    aligner.setProjector(&projector); aligner.setLinearizer(&linearizer); aligner.setCorrespondenceFinder(&finder);
    aligner.setOuterIterations(h.outer); aligner.setInnerIterations(h.inner);

    std::vector<std::unique_ptr<Cloud>> own;
    std::vector<Cloud*> refs, curs, all;
    std::vector<const uint16_t*> frames;
    for (int i = 0; i < h.n; ++i) { own.emplace_back(new Cloud(ctx, (int)N)); refs.push_back(own.back().get()); frames.push_back(ref[i].data()); }
    for (int i = 0; i < h.n; ++i) { own.emplace_back(new Cloud(ctx, (int)N)); curs.push_back(own.back().get()); frames.push_back(cur[i].data()); }
    all = refs; all.insert(all.end(), curs.begin(), curs.end());
    converter.computeBatchRaw(all, frames, 0.001f, h.rows, h.cols);

    int bad = 0;
    if (ctx.convergence().enabled) { std::cerr << "the setting is not off by default" << std::endl; ++bad; }
    ctx.setConvergence(h.epsT, h.epsR, h.minIterations);
    const pwn_hip_convergence s = ctx.convergence();
    if (!s.enabled || s.translation_epsilon != h.epsT || s.rotation_epsilon != h.epsR || s.min_iterations != h.minIterations) { std::cerr << "the setting does not read back" << std::endl; ++bad; }
    const std::vector<pwn_hip_align_result> got = aligner.alignBatch(refs, curs, guesses);
    const std::vector<pwn_hip_align_steps> steps = aligner.lastSteps(0, h.n);
    int stopped = 0;
    for (int i = 0; i < h.n; ++i) {
      const Expected& w = want[i]; const pwn_hip_align_result& g = got[i]; const pwn_hip_align_steps& st = steps[i];
      const bool same = std::memcmp(g.T, w.T, sizeof(w.T)) == 0 && g.iterations == w.iterations && std::memcmp(&g.error, &w.error, 4) == 0 && g.inliers == w.inliers &&
                        st.iterations == w.outerExecuted && st.converged == w.converged &&
                        std::memcmp(st.step_translation, w.stepT, sizeof(w.stepT)) == 0 && std::memcmp(st.step_rotation, w.stepR, sizeof(w.stepR)) == 0;
      if (!same) { std::cerr << "pair " << i << " differs: " << g.iterations << " / " << w.iterations << " iterations, " << st.iterations << " / " << w.outerExecuted << " steps" << std::endl; ++bad; }
      stopped += st.converged;
    }
    ctx.clearConvergence();
    if (ctx.convergence().enabled) { std::cerr << "clearConvergence left the setting on" << std::endl; ++bad; }
    std::cout << h.n << " pairs " << h.rows << "x" << h.cols << ", " << stopped << " converged, " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
