// pwn_hip_batch_priors_check -- batch alignment with SE(3) priors (include/pwn_hip.h: pwn_hip_align_batch_priors) through the C++ host mirror
// against the bytes the Python mirror wrote to a file: the same raw frames are converted as one batch, Aligner::alignBatchRecords with the
// file's prior lists must reproduce every record byte for byte, and Aligner::alignBatch with the same lists must return the records'
// transforms and traces.  Exits 0 when nothing differs, 1 on a difference, 2 on an error of the library or of the file.
//
//   pwn_hip_batch_priors_check FILE
//
// FILE (little-endian, written by tests/test_gpu_batch_priors.py):
//   int32 n, rows, cols, outer_iterations, inner_iterations, first_pair_id; float fx, fy, cx, cy
//   n x { uint16 reference frame [rows * cols] (millimetres), uint16 current frame [rows * cols] }
//   n x float guess[16] (column-major)
//   int32 first[n + 1]; first[n] x pwn_hip_prior (int32 kind, float mean[16], reference_transform[16], information[36])
//   n x float record[PWN_HIP_RECORD_FLOATS]
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_batch_priors_check.cpp -o tools/pwn_hip_batch_priors_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

struct Header { int32_t n, rows, cols, outer, inner, firstPairId; float fx, fy, cx, cy; };

template <typename T> static bool get(std::ifstream& f, T* dst, size_t count) { return (bool)f.read(reinterpret_cast<char*>(dst), (std::streamsize)(sizeof(T) * count)); }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_batch_priors_check FILE" << std::endl; return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  Header h;
  if (!f || !get(f, &h, 1) || h.n <= 0 || h.rows <= 0 || h.cols <= 0) { std::cerr << "cannot read " << argv[1] << std::endl; return 2; }
  const size_t N = (size_t)h.rows * h.cols, R = PWN_HIP_RECORD_FLOATS;
  std::vector<std::vector<uint16_t>> ref((size_t)h.n, std::vector<uint16_t>(N)), cur((size_t)h.n, std::vector<uint16_t>(N));
  for (int i = 0; i < h.n; ++i) if (!get(f, ref[i].data(), N) || !get(f, cur[i].data(), N)) { std::cerr << "short file (frames)" << std::endl; return 2; }
  std::vector<Isometry3f> guesses((size_t)h.n);
  for (int i = 0; i < h.n; ++i) { float g[16]; if (!get(f, g, 16)) { std::cerr << "short file (guesses)" << std::endl; return 2; } guesses[i] = Isometry3f(g); }
  std::vector<int32_t> first((size_t)h.n + 1);
  if (!get(f, first.data(), first.size()) || first[0] != 0) { std::cerr << "short file (prior lists)" << std::endl; return 2; }
  Aligner::PairPriors priors((size_t)h.n);
  int total = 0;
  for (int i = 0; i < h.n; ++i) {
    if (first[i + 1] < first[i]) { std::cerr << "bad prior list" << std::endl; return 2; }
    priors[i].resize((size_t)(first[i + 1] - first[i]));
    if (!priors[i].empty() && !get(f, priors[i].data(), priors[i].size())) { std::cerr << "short file (priors)" << std::endl; return 2; }
    total += (int)priors[i].size();
  }
  std::vector<float> want((size_t)h.n * R);
  if (!get(f, want.data(), want.size())) { std::cerr << "short file (records)" << std::endl; return 2; }
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

    std::vector<float> got((size_t)h.n * R, -7.f);
    const std::vector<pwn_hip_align_result> viaRecords = aligner.alignBatchRecords(refs, curs, got.data(), guesses, priors, std::vector<int>(), h.firstPairId);
    const std::vector<pwn_hip_align_result> plain = aligner.alignBatch(refs, curs, guesses, priors);
    int bad = 0;
    for (int i = 0; i < h.n; ++i) {
      const float* g = &got[(size_t)i * R]; const float* w = &want[(size_t)i * R];
      if (std::memcmp(g, w, R * sizeof(float)) != 0) {
        int k = 0; while (k < (int)R && std::memcmp(g + k, w + k, sizeof(float)) == 0) ++k;
        std::cerr << "record " << i << " differs from word " << k << ": " << g[k] << " / " << w[k] << std::endl; ++bad;
      }
      for (const pwn_hip_align_result* r : { &viaRecords[(size_t)i], &plain[(size_t)i] }) {
        if (std::memcmp(r->T, g, sizeof(r->T)) != 0 || (float)r->iterations != g[18]) { std::cerr << "result " << i << ": transform or iterations" << std::endl; ++bad; }
        for (int k = 0; k < r->iterations && k < 10; ++k)
          if (std::memcmp(&r->chi2[k], g + 20 + k, sizeof(float)) != 0 || (float)r->iter_inliers[k] != g[30 + k]) { std::cerr << "result " << i << ": traces" << std::endl; ++bad; break; }
      }
    }
    const std::vector<pwn_hip_align_steps> steps = aligner.lastSteps(0, h.n);
    for (int i = 0; i < h.n; ++i) if (steps[(size_t)i].iterations != h.outer) { std::cerr << "pair " << i << ": step traces" << std::endl; ++bad; }
    std::cout << h.n << " pairs " << h.rows << "x" << h.cols << ", " << total << " priors, " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
