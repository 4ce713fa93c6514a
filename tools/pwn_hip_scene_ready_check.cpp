// pwn_hip_scene_ready_check -- the two host mirrors held together on the flow a lean cache broke: CloudCache(matcher, capacity, sceneReady = true)
// -> PwnMerger::mergeNodeList of the C++ mirror against the fused cloud the Python mirror made from the same input
// (tests/test_gpu_scene_ready_batch.py writes the file).  Frame 0 is the big node, the list is every frame, frame 0 included.  The point count,
// the Gaussian count, the per-cloud counters and every array of the fused cloud -- Stats and Gaussians included -- and its weights must be equal
// byte for byte (the C++ cache converts its misses one by one, the Python cache in one batch call: same bits).  Exits 0 when nothing differs, 1 on a
// difference, 2 on an error.
//
//   pwn_hip_scene_ready_check scene.bin
//
// File (little endian): int32 rows, cols, frames; float64 K[4] (fx fy cx cy), min_distance, max_distance; int32 min_image_radius,
// max_image_radius, min_points; per frame float64 pose[16] (row-major) and float32 depth[rows*cols]; int32 points and int32 Gaussians of the
// fused cloud; then sixteen arrays, each int64 bytes + the bytes: points, normals, curvature, omega_p, omega_n, stats, eigenvalues, npoints,
// weights, appended, fused, and the Gaussians' mean, cov, info_vec, info, flags.
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_scene_ready_check.cpp -o tools/pwn_hip_scene_ready_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

template <typename T> static bool get(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_scene_ready_check scene.bin" << std::endl; return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
  int head[3]; double Kd[4], range[2]; int conf[3];
  if (!get(f, head, 3) || !get(f, Kd, 4) || !get(f, range, 2) || !get(f, conf, 3) || head[0] <= 0 || head[1] <= 0 || head[2] < 1) { std::cerr << "bad header" << std::endl; return 2; }
  const int rows = head[0], cols = head[1], n = head[2];
  std::vector<MapNode> nodes((size_t)n);
  std::vector<DepthImage> frames((size_t)n);
  for (int k = 0; k < n; ++k) {
    nodes[k].key = k;
    frames[k].create(rows, cols);
    if (!get(f, nodes[k].transform.m, 16) || !get(f, frames[k].data.data(), frames[k].data.size())) { std::cerr << "short file" << std::endl; return 2; }
  }
  int expectedPoints = 0, expectedGaussians = 0;
  if (!get(f, &expectedPoints) || !get(f, &expectedGaussians)) { std::cerr << "short file" << std::endl; return 2; }
  const int kArrays = 16;
  static const char* names[kArrays] = { "points", "normals", "curvature", "omega_p", "omega_n", "stats", "eigenvalues", "npoints", "weights", "appended", "fused",
                                        "gaussian mean", "gaussian cov", "gaussian info_vec", "gaussian info", "gaussian flags" };
  std::vector<std::vector<char> > expected(kArrays);
  for (int a = 0; a < kArrays; ++a) {
    long long bytes = 0;
    if (!get(f, &bytes) || bytes < 0) { std::cerr << "short file" << std::endl; return 2; }
    expected[a].resize((size_t)bytes);
    if (bytes && !get(f, expected[a].data(), (size_t)bytes)) { std::cerr << "short file" << std::endl; return 2; }
  }
  std::fclose(f);

  try {
    Context ctx(0, rows, cols, 16);
    ctx.setOmegaStorage(PWN_HIP_OMEGA_EXACT9);
    // the converter's projector is the merger's; matcher at scale 1 (the cache makes the clouds)
    PinholePointProjector projector;
    Matrix3f K; K(0,0) = (float)Kd[0]; K(1,1) = (float)Kd[1]; K(0,2) = (float)Kd[2]; K(1,2) = (float)Kd[3]; K(2,2) = 1.f;
    projector.setCameraMatrix(K); projector.setMinDistance((float)range[0]); projector.setMaxDistance((float)range[1]); projector.setImageSize(rows, cols);
    StatsCalculatorIntegralImage stats;
    stats.setWorldRadius(0.1f); stats.setMinImageRadius(conf[0]); stats.setMaxImageRadius(conf[1]); stats.setMinPoints(conf[2]); stats.setCurvatureThreshold(0.2f);
    PointInformationMatrixCalculator pinfo; NormalInformationMatrixCalculator ninfo;
    pinfo.setCurvatureThreshold(0.02f); ninfo.setCurvatureThreshold(0.02f);
    DepthImageConverterIntegralImage converter(&ctx, &projector, &stats, &pinfo, &ninfo);
    Aligner aligner(&ctx);
    aligner.setProjector(&projector);
    PwnMatcherBase matcher(&ctx, &aligner, &converter);
    matcher.setScale(1);
    CloudCache cache(&matcher, 16, true);
    for (int k = 0; k < n; ++k) cache.addFrame(k, frames[k], K, Isometry3f::Identity());
    Merger2 merger(&ctx, &converter, &matcher);
    PwnMerger pm(&ctx, &merger, &cache);

    std::vector<const MapNode*> list;
    for (int k = 0; k < n; ++k) list.push_back(&nodes[k]);
    const Cloud* fused = pm.mergeNodeList(&nodes[0], list);

    int bad = 0;
    const size_t m = fused->size();
    if ((int)m != expectedPoints) { std::cerr << m << " points, expected " << expectedPoints << std::endl; ++bad; }
    if (cache.get(0) != fused) { std::cerr << "the cache does not hold the fused cloud under the big node's key" << std::endl; ++bad; }
    const size_t ng = fused->numGaussians();
    if ((int)ng != expectedGaussians || ng != m) { std::cerr << ng << " Gaussians for " << m << " points, expected " << expectedGaussians << std::endl; ++bad; }
    std::vector<std::vector<char> > got(kArrays);
    auto put = [&](int a, const void* p, size_t bytes) { got[a].assign((const char*)p, (const char*)p + bytes); };
    { const std::vector<float> v = fused->points(); put(0, v.data(), v.size() * 4); }
    { const std::vector<float> v = fused->normals(); put(1, v.data(), v.size() * 4); }
    { const std::vector<float> v = fused->curvatures(); put(2, v.data(), v.size() * 4); }
    { const std::vector<float> v = fused->pointInformationMatrix(); put(3, v.data(), v.size() * 4); }
    { const std::vector<float> v = fused->normalInformationMatrix(); put(4, v.data(), v.size() * 4); }
    { std::vector<float> st(m * 16), ev(m * 3); std::vector<int> np(m);
      ctx.check(pwn_hip_cloud_download_stats(ctx.handle(), fused->handle(), st.data(), ev.data(), np.data()));
      put(5, st.data(), st.size() * 4); put(6, ev.data(), ev.size() * 4); put(7, np.data(), np.size() * 4); }
    { const std::vector<float> v = merger.pesiTot(); put(8, v.data(), v.size() * 4); }
    put(9, merger.appended.data(), merger.appended.size() * sizeof(int));
    put(10, merger.fused.data(), merger.fused.size() * sizeof(int));
    { std::vector<float> mean(ng * 3), cov(ng * 9), iv(ng * 3), info(ng * 9); std::vector<int> flags(ng);
      ctx.check(pwn_hip_cloud_download_gaussians(ctx.handle(), fused->handle(), mean.data(), cov.data(), iv.data(), info.data(), flags.data()));
      put(11, mean.data(), mean.size() * 4); put(12, cov.data(), cov.size() * 4); put(13, iv.data(), iv.size() * 4); put(14, info.data(), info.size() * 4);
      put(15, flags.data(), flags.size() * sizeof(int)); }
    for (int a = 0; a < kArrays; ++a)
      if (got[a].size() != expected[a].size() || (!got[a].empty() && std::memcmp(got[a].data(), expected[a].data(), got[a].size()) != 0)) {
        std::cerr << names[a] << ": " << got[a].size() << " bytes against " << expected[a].size() << ", or their content differs" << std::endl; ++bad;
      }
    std::cout << n << " frames " << rows << "x" << cols << ": " << m << " points, " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
