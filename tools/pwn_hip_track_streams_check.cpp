// pwn_hip_track_streams_check -- the multi-stream tracker (include/pwn_hip.h: pwn_hip_track_frames) through the C++ host mirror
// (PwnTrackerBatch::processFrames) against what the Python mirror (api.PwnTrackerBatch) wrote to a file: the same raw frames in the same calls,
// every frame's result record, every stream's final state and the points of its final key cloud compared bit for bit.  Exits 0 when nothing
// differs, 1 on a difference, 2 on an error of the library or of the file.
//
//   pwn_hip_track_streams_check FILE
//
// FILE (little-endian, written by tests/test_gpu_track_streams_harness.py):
//   int32 streams, frames, rows, cols, scale, calls; float threshold; float fx, fy, cx, cy; float sensor_offset[16] (column-major)
//   int32 frames_of_call[calls]                       (their sum is `frames`)
//   int32 present[frames * streams]                   (step-major; 0 = the stream idles in that step)
//   per present (step, stream): uint16 frame[rows * cols] (millimetres)
//   pwn_hip_track_result expected[frames * streams]   (all zero where the stream idled)
//   per stream: float globalT[16], previous_cloud_transform[16]; int32 counter, num_keyframes, key_points; float points[key_points * 4]
//
//   g++ -O2 -std=c++17 -I. tools/pwn_hip_track_streams_check.cpp -o tools/pwn_hip_track_streams_check -Lg2o_frontend_amd -lpwn_hip -Wl,-rpath,$ORIGIN/../g2o_frontend_amd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>

#include "g2o_frontend_amd/host/pwn_hip.hpp"

using namespace pwn_hip;

struct Header { int32_t streams, frames, rows, cols, scale, calls; float threshold; float fx, fy, cx, cy; float offset[16]; };
struct FinalState { float globalT[16], previousCloudTransform[16]; int32_t counter, numKeyframes, keyPoints; };

template <typename T> static bool get(std::ifstream& f, T* dst, size_t count) { return (bool)f.read(reinterpret_cast<char*>(dst), (std::streamsize)(sizeof(T) * count)); }

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "USAGE: pwn_hip_track_streams_check FILE" << std::endl; return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  Header h;
  if (!f || !get(f, &h, 1) || h.streams <= 0 || h.frames <= 0 || h.rows <= 0 || h.cols <= 0 || h.calls <= 0) { std::cerr << "cannot read " << argv[1] << std::endl; return 2; }
  const int S = h.streams; const size_t N = (size_t)h.rows * h.cols, FS = (size_t)h.frames * S;
  std::vector<int32_t> callF((size_t)h.calls), present(FS);
  if (!get(f, callF.data(), callF.size()) || !get(f, present.data(), FS)) { std::cerr << "short file (plan)" << std::endl; return 2; }
  int total = 0, maxF = 0;
  for (int32_t n : callF) { total += n; maxF = n > maxF ? n : maxF; }
  if (total != h.frames) { std::cerr << "the calls do not add up to the frames" << std::endl; return 2; }
  std::vector<std::unique_ptr<RawDepthImage>> images(FS);
  for (size_t i = 0; i < FS; ++i) {
    if (!present[i]) continue;
    images[i].reset(new RawDepthImage()); images[i]->rows = h.rows; images[i]->cols = h.cols; images[i]->data.resize(N);
    if (!get(f, images[i]->data.data(), N)) { std::cerr << "short file (frames)" << std::endl; return 2; }
  }
  std::vector<pwn_hip_track_result> want(FS);
  if (!get(f, want.data(), FS)) { std::cerr << "short file (results)" << std::endl; return 2; }
  std::vector<FinalState> finals((size_t)S); std::vector<std::vector<float>> keyPoints((size_t)S);
  for (int s = 0; s < S; ++s) {
    if (!get(f, &finals[s], 1) || finals[s].keyPoints < 0) { std::cerr << "short file (states)" << std::endl; return 2; }
    keyPoints[s].resize((size_t)finals[s].keyPoints * 4);
    if (!keyPoints[s].empty() && !get(f, keyPoints[s].data(), keyPoints[s].size())) { std::cerr << "short file (key clouds)" << std::endl; return 2; }
  }
  try {
    Context ctx(0, h.rows, h.cols, S > 2 ? S : 2);
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
    finder.setInlierCurvatureRatioThreshold(1.3f); finder.setImageSize(h.rows / h.scale, h.cols / h.scale);
    Linearizer linearizer; linearizer.setInlierMaxChi2(9000.f); linearizer.setRobustKernel(true);
    Aligner aligner(&ctx);
    aligner.setProjector(&projector); aligner.setLinearizer(&linearizer); aligner.setCorrespondenceFinder(&finder);
    aligner.setOuterIterations(10); aligner.setInnerIterations(1);

    int bad = 0, switches = 0;
    {
      PwnTrackerBatch tracker(&ctx, &aligner, &converter, S, maxF, h.rows, h.cols, h.scale);
      tracker.setNewFrameInliersFraction(h.threshold);
      const Isometry3f offset(h.offset);
      int f0 = 0;
      for (int32_t n : callF) {
        std::vector<std::vector<const RawDepthImage*>> frames((size_t)n, std::vector<const RawDepthImage*>((size_t)S, nullptr));
        for (int k = 0; k < n; ++k) for (int s = 0; s < S; ++s) frames[k][s] = images[(size_t)(f0 + k) * S + s].get();
        const auto got = tracker.processFrames(frames, offset, K);
        for (int k = 0; k < n; ++k)
          for (int s = 0; s < S; ++s) {
            const pwn_hip_track_result& w = want[(size_t)(f0 + k) * S + s]; const PwnTrackerBatch::StreamFrame& g = got[k][s];
            bool same = g.present == (present[(size_t)(f0 + k) * S + s] != 0);
            if (same && g.present) {
              const PwnTrackerBatch::FrameResult& r = g.result;
              same = r.newFrame == (w.new_frame != 0) && r.aligned == (w.aligned != 0) && r.inliers == w.inliers && std::memcmp(&r.error, &w.error, 4) == 0 &&
                     std::memcmp(&r.inliersFraction, &w.inliers_fraction, 4) == 0 && std::memcmp(r.T.data(), w.T, sizeof(w.T)) == 0 &&
                     std::memcmp(r.globalT.data(), w.globalT, sizeof(w.globalT)) == 0 && g.nPoints == w.n_points;
              switches += r.newFrame && r.aligned ? 1 : 0;
            }
            if (!same) { std::cerr << "frame " << f0 + k << " of stream " << s << " differs" << std::endl; ++bad; }
          }
        f0 += n;
      }
      for (int s = 0; s < S; ++s) {
        const pwn_hip_tracker_state st = tracker.state(s); const FinalState& w = finals[s];
        if (std::memcmp(st.globalT, w.globalT, sizeof(w.globalT)) != 0 || std::memcmp(st.previous_cloud_transform, w.previousCloudTransform, sizeof(w.previousCloudTransform)) != 0 ||
            st.counter != w.counter || st.num_keyframes != w.numKeyframes || tracker.numKeyframes(s) != w.numKeyframes) { std::cerr << "final state of stream " << s << " differs" << std::endl; ++bad; }
        pwn_hip_cloud* key = tracker.keyCloud(s);
        int n = 0;
        if (key) ctx.check(pwn_hip_cloud_size(ctx.handle(), key, &n));
        std::vector<float> pts((size_t)n * 4);
        if (n > 0) ctx.check(pwn_hip_cloud_download(ctx.handle(), key, pts.data(), nullptr, nullptr, nullptr, nullptr));
        if (n != w.keyPoints || (n > 0 && std::memcmp(pts.data(), keyPoints[s].data(), pts.size() * sizeof(float)) != 0)) { std::cerr << "key cloud of stream " << s << " differs" << std::endl; ++bad; }
      }
    }
    std::cout << S << " streams, " << h.frames << " frames in " << h.calls << " calls, " << switches << " key switches, " << bad << " differences" << std::endl;
    return bad ? 1 : 0;
  } catch (const Error& e) {
    std::cerr << "pwn_hip error: " << e.what() << std::endl;
    return 2;
  }
}
