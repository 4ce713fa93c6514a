// pwn_hip_manifold_check -- ManifoldVoronoiExtractor::process of the C++ host mirror against the images the Python mirror made from the same
// input (tests/test_gpu_manifold_image.py writes the file).  Every frame is a key node, pushed in order; after each push the image and the
// per-cloud counts of points inside the grid must be equal byte for byte (both mirrors make the same calls on the same device).  Exits 0 when
// nothing differs, 1 on a difference, 2 on an error.
//
//   pwn_hip_manifold_check manifold.bin
//
// File (little endian): int32 rows, cols, frames; float64 K[4] (fx fy cx cy), min_distance, max_distance; int32 min_image_radius,
// max_image_radius, min_points; float32 sensor offset[16] (row-major); int32 xSize, ySize, dequeSize; float32 resolution, normalThreshold;
// per frame float64 pose[16] (row-major) and float32 depth[rows*cols]; then per frame int32 m (clouds in the deque), int32 inside[m],
// uint16 image[xSize*ySize].
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_manifold_check.cpp -o tools/pwn_hip_manifold_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

template <typename T> static bool get(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_manifold_check manifold.bin" << std::endl; return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::cerr << "cannot open " << argv[1] << std::endl; return 2; }
  int head[3]; double Kd[4], range[2]; int conf[3]; float off[16]; int grid[3]; float par[2];
  if (!get(f, head, 3) || !get(f, Kd, 4) || !get(f, range, 2) || !get(f, conf, 3) || !get(f, off, 16) || !get(f, grid, 3) || !get(f, par, 2) || head[0] <= 0 ||
      head[1] <= 0 || head[2] < 1 || grid[0] <= 0 || grid[1] <= 0 || grid[2] < 1) { std::cerr << "bad header" << std::endl; return 2; }
  const int rows = head[0], cols = head[1], n = head[2];
  std::vector<MapNode> nodes((size_t)n);
  std::vector<DepthImage> frames((size_t)n);
  for (int k = 0; k < n; ++k) {
    nodes[k].key = k;
    frames[k].create(rows, cols);
    if (!get(f, nodes[k].transform.m, 16) || !get(f, frames[k].data.data(), frames[k].data.size())) { std::cerr << "short file" << std::endl; return 2; }
  }
  std::vector<std::vector<int> > wantInside((size_t)n);
  std::vector<std::vector<uint16_t> > wantImage((size_t)n);
  for (int k = 0; k < n; ++k) {
    int m = 0;
    if (!get(f, &m) || m < 0 || m > n) { std::cerr << "short file" << std::endl; return 2; }
    wantInside[k].resize((size_t)m); wantImage[k].resize((size_t)grid[0] * grid[1]);
    if ((m && !get(f, wantInside[k].data(), (size_t)m)) || !get(f, wantImage[k].data(), wantImage[k].size())) { std::cerr << "short file" << std::endl; return 2; }
  }
  std::fclose(f);

  try {
    Context ctx(0, rows, cols, 16);
    ctx.setOmegaStorage(PWN_HIP_OMEGA_EXACT9);
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
    CloudCache cache(&matcher, 16);
    Isometry3f offset;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) offset(r,c) = off[4 * r + c];
    for (int k = 0; k < n; ++k) cache.addFrame(k, frames[k], K, offset);
    ManifoldVoronoiExtractor extractor(&ctx, &cache);
    extractor.xSize = grid[0]; extractor.ySize = grid[1]; extractor.setQueueSize((size_t)grid[2]);
    extractor.setResolution(par[0]); extractor.normalThreshold = par[1];

    int bad = 0;
    for (int k = 0; k < n; ++k) {
      const ManifoldVoronoiData d = extractor.process(&nodes[k]);
      if (d.node != &nodes[k] || d.resolution != par[0] || d.rows != grid[0] || d.cols != grid[1]) { std::cerr << "node " << k << ": record fields differ" << std::endl; ++bad; }
      if (extractor.inside != wantInside[k]) { std::cerr << "node " << k << ": counts of points inside the grid differ" << std::endl; ++bad; }
      if (d.image != wantImage[k]) { std::cerr << "node " << k << ": image differs" << std::endl; ++bad; }
    }
    std::cout << n << " key nodes " << rows << "x" << cols << " into " << grid[0] << "x" << grid[1] << ": " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
