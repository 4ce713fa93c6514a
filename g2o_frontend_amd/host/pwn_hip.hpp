// pwn_hip.hpp -- header-only C++ host mirror of the reference's pwn_core operator interface over the C-ABI
// (include/pwn_hip.h).  Class / method names and argument meaning follow g2o_frontend/pwn_core so that a caller
// such as PwnMatcherBase (pwn_tracker/pwn_matcher_base.cpp:57-183) or pwn_simple_aligner.cpp compiles against
// these classes with a namespace switch; the heavy methods are one call into libpwn_hip.so each.
//
// Differences a maintainer has to know about:
//   * no Eigen here: Matrix3f / Isometry3f are plain column-major float arrays with Eigen's memory layout, so
//     `Isometry3f(eigenIso.matrix().data())` / `std::memcpy(eigen.data(), m.data(), ...)` convert both ways;
//   * Cloud lives in device memory (pwn_hip_cloud); points()/normals()/... download on demand;
//   * errors: the reference asserts (UB in Release); these classes throw pwn_hip::Error carrying the ABI status.
#pragma once

#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pwn_hip.h"

namespace pwn_hip {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error("pwn_hip status " + std::to_string(c) + ": " + m), code(c) {}
};

struct Matrix3f {
  float m[9];
  Matrix3f() { std::memset(m, 0, sizeof(m)); m[0] = m[4] = m[8] = 1.f; }
  float& operator()(int r, int c) { return m[r + 3 * c]; }
  float operator()(int r, int c) const { return m[r + 3 * c]; }
  const float* data() const { return m; }
  float* data() { return m; }
};
struct Isometry3f {
  float m[16];
  Isometry3f() { setIdentity(); }
  explicit Isometry3f(const float* colmajor16) { std::memcpy(m, colmajor16, sizeof(m)); }
  static Isometry3f Identity() { return Isometry3f(); }
  void setIdentity() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = m[15] = 1.f; }
  float& operator()(int r, int c) { return m[r + 4 * c]; }
  float operator()(int r, int c) const { return m[r + 4 * c]; }
  const float* data() const { return m; }
  float* data() { return m; }
  void forceLastRow() { m[3] = 0.f; m[7] = 0.f; m[11] = 0.f; m[15] = 1.f; }
  Isometry3f inverse() const { Isometry3f r; pwn_hip_iso_inverse(m, r.m); return r; }       // Isometry3f::inverse(): R^T, -R^T t
  // Isometry3f * Isometry3f (linear = Ra*Rb, translation = Ra*tb + ta), float, left-to-right sums
  Isometry3f operator*(const Isometry3f& b) const {
    Isometry3f r;
    for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) { float s = (*this)(i,0) * b(0,j); s = s + (*this)(i,1) * b(1,j); s = s + (*this)(i,2) * b(2,j); r(i,j) = s; }
    for (int i = 0; i < 3; ++i) { float s = (*this)(i,0) * b(0,3); s = s + (*this)(i,1) * b(1,3); s = s + (*this)(i,2) * b(2,3); r(i,3) = s + (*this)(i,3); }
    r.forceLastRow();
    return r;
  }
};
struct DepthImage {                       // pwn_typedefs.h:57-62: float metres, row-major
  int rows = 0, cols = 0;
  std::vector<float> data;
  void create(int r, int c) { rows = r; cols = c; data.assign((size_t)r * c, 0.f); }
  float& operator()(int r, int c) { return data[(size_t)r * cols + c]; }
};
struct RawDepthImage { int rows = 0, cols = 0; std::vector<uint16_t> data; };
struct IntImage { int rows = 0, cols = 0; std::vector<int> data; void create(int r, int c) { rows = r; cols = c; data.assign((size_t)r * c, -1); } };

inline Isometry3f v2t(const float v[6]) { Isometry3f T; pwn_hip_v2t(v, T.data()); return T; }      // bm_se3.h:37-43
inline void t2v(const Isometry3f& T, float v[6]) { pwn_hip_t2v(T.data(), v); }                     // bm_se3.h:45-52
// Isometry3f * Isometry3f with the evaluation order of the CPU path (the library's host helper; what the device-side pose chaining uses)
inline Isometry3f iso_mul(const Isometry3f& a, const Isometry3f& b) { Isometry3f r; pwn_hip_iso_mul(a.data(), b.data(), r.data()); return r; }
struct Matrix6f {                          // bm_defs.h:11, column-major
  float m[36];
  Matrix6f() { std::memset(m, 0, sizeof(m)); }
  static Matrix6f Identity() { Matrix6f r; for (int i = 0; i < 6; ++i) r.m[7 * i] = 1.f; return r; }
  float& operator()(int r, int c) { return m[r + 6 * c]; }
  float operator()(int r, int c) const { return m[r + 6 * c]; }
  const float* data() const { return m; }
  float* data() { return m; }
};
struct Vector6f { float v[6] = { 0, 0, 0, 0, 0, 0 }; float& operator[](int i) { return v[i]; } float operator[](int i) const { return v[i]; } };

// One per (GPU, host thread); every object below borrows it (non-owning raw pointer, like the reference's
// collaborator pointers: aligner.h:381-386).
class Context {
 public:
  Context(int device, int maxRows, int maxCols, int maxBatch = 1) {
    int rc = pwn_hip_ctx_create(&_ctx, device, maxRows, maxCols, maxBatch);
    if (rc) throw Error(rc, pwn_hip_last_error_string(nullptr));
  }
  ~Context() { pwn_hip_ctx_destroy(_ctx); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  pwn_hip_ctx* handle() const { return _ctx; }
  void check(int rc) const { if (rc) throw Error(rc, pwn_hip_last_error_string(_ctx)); }
  // batch calls: frames / pairs per kernel launch and the number of HIP streams the sub-batches are dealt over (include/pwn_hip.h)
  void setSubbatch(int frames, int pairs) { check(pwn_hip_ctx_set_subbatch(_ctx, frames, pairs)); }
  void setConcurrency(int streams) { check(pwn_hip_ctx_set_concurrency(_ctx, streams)); }
  // PWN_HIP_OMEGA_SYM6 (default) / PWN_HIP_OMEGA_EXACT9 (every entry of Omega_p bit-identical to pwn_core's): storage of the point information matrices of clouds created from now on
  void setOmegaStorage(int mode) { check(pwn_hip_ctx_set_omega_storage(_ctx, mode)); }
  // "stop when converged" for every alignment call of the context (include/pwn_hip.h: pwn_hip_ctx_set_convergence; opt-in, a deviation from the
  // reference's fixed outerIterations): a pair's loop ends on the device after the first outer iteration i with i + 1 >= minIterations whose last
  // step is no longer than the two epsilons; its results are those of outerIterations = i + 1, bit for bit
  void setConvergence(float translation, float rotation, int minIterations = 0) {
    const pwn_hip_convergence s = { 1, translation, rotation, minIterations };
    check(pwn_hip_ctx_set_convergence(_ctx, &s));
  }
  void clearConvergence() { check(pwn_hip_ctx_set_convergence(_ctx, nullptr)); }
  pwn_hip_convergence convergence() const { pwn_hip_convergence s; check(pwn_hip_ctx_get_convergence(_ctx, &s)); return s; }      // enabled == 0: off
  // the step norms of the pairs [first, first + n) of the last alignment call
  std::vector<pwn_hip_align_steps> lastAlignSteps(int first = 0, int n = 1) {
    std::vector<pwn_hip_align_steps> out((size_t)(n > 0 ? n : 0));
    check(pwn_hip_last_align_steps(_ctx, first, n, out.data()));
    return out;
  }
  void synchronize() { check(pwn_hip_ctx_synchronize(_ctx)); }
  void waitStream(void* hipStream) { check(pwn_hip_ctx_wait_stream(_ctx, hipStream)); }      // what the context queues from now on runs after that stream's work
  void signalStream(void* hipStream) { check(pwn_hip_ctx_signal_stream(_ctx, hipStream)); }  // what that stream gets from now on runs after everything the context has queued
  // fn(user) runs inside every alignment batch call, after its device work is queued and before the call waits (include/pwn_hip.h); nullptr = off
  void setEnqueuedCallback(void (*fn)(void*), void* user) { check(pwn_hip_ctx_set_enqueued_callback(_ctx, fn, user)); }
 private:
  pwn_hip_ctx* _ctx = nullptr;
};

// pwn_static.cpp:54-68 / :5-36
inline void DepthImage_convert_16UC1_to_32FC1(Context& ctx, DepthImage& dest, const RawDepthImage& src, float scale = 0.001f) {
  dest.create(src.rows, src.cols);
  ctx.check(pwn_hip_depth_u16_to_f32(ctx.handle(), src.data.data(), dest.data.data(), src.rows * src.cols, scale));
}
inline void DepthImage_scale(Context& ctx, DepthImage& dest, const DepthImage& src, int step, float maxDepthCov = 0.01f) {
  dest.create(src.rows / step, src.cols / step);
  ctx.check(pwn_hip_depth_scale(ctx.handle(), src.data.data(), src.rows, src.cols, step, maxDepthCov, dest.data.data()));
}
// the same for a run of images of one size, in one call (pwn_hip_depth_scale_batch)
inline void DepthImage_scale(Context& ctx, std::vector<DepthImage>& dest, const std::vector<DepthImage>& src, int step, float maxDepthCov = 0.01f) {
  dest.resize(src.size());
  if (src.empty()) return;
  std::vector<const float*> s(src.size()); std::vector<float*> d(src.size());
  for (size_t i = 0; i < src.size(); ++i) {
    if (src[i].rows != src[0].rows || src[i].cols != src[0].cols) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImage_scale: images of one call share one size");
    dest[i].create(src[i].rows / (step > 0 ? step : 1), src[i].cols / (step > 0 ? step : 1));
    s[i] = src[i].data.data(); d[i] = dest[i].data.data();
  }
  ctx.check(pwn_hip_depth_scale_batch(ctx.handle(), s.data(), (int)src.size(), src[0].rows, src[0].cols, step, maxDepthCov, d.data()));
}

// cloud.h:20-187
class Cloud {
 public:
  Cloud(Context& ctx, int capacity) : _ctx(&ctx) { ctx.check(pwn_hip_cloud_create(ctx.handle(), capacity, &_h)); }
  ~Cloud() { pwn_hip_cloud_destroy(_ctx->handle(), _h); }
  Cloud(const Cloud&) = delete;
  Cloud& operator=(const Cloud&) = delete;
  pwn_hip_cloud* handle() const { return _h; }
  size_t size() const { int n = 0; _ctx->check(pwn_hip_cloud_size(_ctx->handle(), _h, &n)); return (size_t)n; }
  // n*4 floats each (Point w = 1, Normal w = 0)
  std::vector<float> points() const { std::vector<float> v(size() * 4); _ctx->check(pwn_hip_cloud_download(_ctx->handle(), _h, v.data(), nullptr, nullptr, nullptr, nullptr)); return v; }
  std::vector<float> normals() const { std::vector<float> v(size() * 4); _ctx->check(pwn_hip_cloud_download(_ctx->handle(), _h, nullptr, v.data(), nullptr, nullptr, nullptr)); return v; }
  std::vector<float> curvatures() const { std::vector<float> v(size()); _ctx->check(pwn_hip_cloud_download(_ctx->handle(), _h, nullptr, nullptr, v.data(), nullptr, nullptr)); return v; }
  std::vector<float> pointInformationMatrix() const { std::vector<float> v(size() * 16); _ctx->check(pwn_hip_cloud_download(_ctx->handle(), _h, nullptr, nullptr, nullptr, v.data(), nullptr)); return v; }
  std::vector<float> normalInformationMatrix() const { std::vector<float> v(size() * 16); _ctx->check(pwn_hip_cloud_download(_ctx->handle(), _h, nullptr, nullptr, nullptr, nullptr, v.data())); return v; }
  // n*16 floats: eigenvectors + mean as a column-major 4x4 per point (Stats, stats.h:13); needs a conversion that kept them (scene clouds)
  std::vector<float> stats() const { std::vector<float> v(size() * 16); _ctx->check(pwn_hip_cloud_download_stats(_ctx->handle(), _h, v.data(), nullptr, nullptr)); return v; }
  std::vector<int> traversabilityVector() const { return std::vector<int>(); }      // cloud.h:99: never written on this path
  size_t gaussians() const { return numGaussians(); }                              // cloud.h:131: the sensor-noise Gaussians live on the device (pwn_hip_cloud_download_gaussians)
  void transformInPlace(const Isometry3f& T) { _ctx->check(pwn_hip_cloud_transform_in_place(_ctx->handle(), _h, T.data())); }   // cloud.cpp:173-186
  // scene maintenance (cloud.cpp:11-171)
  void add(const Cloud& cloud, const Isometry3f& T = Isometry3f::Identity()) { _ctx->check(pwn_hip_cloud_add(_ctx->handle(), _h, cloud.handle(), T.data())); }
  bool save(const char* filename, const Isometry3f& T = Isometry3f::Identity(), int step = 1, bool binary = false) const {
    return pwn_hip_cloud_save(_ctx->handle(), _h, filename, T.data(), step, binary ? 1 : 0) == PWN_HIP_OK;
  }
  bool load(Isometry3f& T, const char* filename) { return pwn_hip_cloud_load(_ctx->handle(), _h, filename, T.data()) == PWN_HIP_OK; }
  // the cloud as one flat buffer, host or device (replication to the other GPUs of a node: pwn_closer.cpp:85-111; include/pwn_hip.h)
  size_t flatSize() const { size_t w = 0; _ctx->check(pwn_hip_cloud_export(_ctx->handle(), _h, nullptr, 0, &w)); return w; }
  size_t exportFlat(void* dst, size_t bytes) const { size_t w = 0; _ctx->check(pwn_hip_cloud_export(_ctx->handle(), _h, dst, bytes, &w)); return w; }
  void importFlat(const void* src, size_t bytes) { _ctx->check(pwn_hip_cloud_import(_ctx->handle(), _h, src, bytes)); }
  size_t numGaussians() const { int n = 0; _ctx->check(pwn_hip_cloud_num_gaussians(_ctx->handle(), _h, &n)); return (size_t)n; }
  Context* context() const { return _ctx; }
 private:
  Context* _ctx; pwn_hip_cloud* _h = nullptr;
};

// pointprojector.{h,cpp} + pinholepointprojector.{h,cpp}
class PinholePointProjector {
 public:
  PinholePointProjector() { _cameraMatrix(0,2) = 0.5f; _cameraMatrix(1,2) = 0.5f; }                      // pinholepointprojector.cpp:6-9
  const Matrix3f& cameraMatrix() const { return _cameraMatrix; }
  void setCameraMatrix(const Matrix3f& K) { _cameraMatrix = K; }
  const Isometry3f& transform() const { return _transform; }
  void setTransform(const Isometry3f& T) { _transform = T; }
  float minDistance() const { return _minDistance; }  void setMinDistance(float v) { _minDistance = v; }
  float maxDistance() const { return _maxDistance; }  void setMaxDistance(float v) { _maxDistance = v; }
  int imageRows() const { return _imageRows; }  int imageCols() const { return _imageCols; }
  void setImageSize(int r, int c) { _imageRows = r; _imageCols = c; }
  float baseline() const { return _baseline; }  void setBaseline(float v) { _baseline = v; }        // sensor-noise model of unProject's Gaussians
  float alpha() const { return _alpha; }        void setAlpha(float v) { _alpha = v; }
  void scale(float s) {                                                                                  // pinholepointprojector.cpp:149-154
    for (int c = 0; c < 3; ++c) { _cameraMatrix(0,c) *= s; _cameraMatrix(1,c) *= s; }
    _imageRows = (int)(_imageRows * s); _imageCols = (int)(_imageCols * s);
  }
  // unProject(points, indexImage, depthImage) (.cpp:68-91 / :93-133 without the Gaussians): fills the cloud's points with this projector's
  // transform, the other fields are reset to "invalid"
  Matrix3f inverseCameraMatrix() const { Matrix3f iK; float a[16], b[16]; pwn_hip_projector_matrices(_cameraMatrix.data(), _transform.data(), a, b, iK.data()); return iK; }   // :61
  // the single-point forms (pinholepointprojector.h:174,187,200): host code, the kernels' own expressions
  bool project(int& x, int& y, float& f, const float p[3]) const { return pwn_hip_project_point(_cameraMatrix.data(), _transform.data(), _minDistance, _maxDistance, p, &x, &y, &f) != 0; }
  bool unProject(float p[3], int x, int y, float d) const { return pwn_hip_unproject_pixel(_cameraMatrix.data(), _transform.data(), _minDistance, _maxDistance, x, y, d, p) != 0; }
  int projectInterval(int, int, float d, float worldRadius) const { return pwn_hip_project_interval(_cameraMatrix.data(), _minDistance, _maxDistance, d, worldRadius); }
  void unProject(Context& ctx, Cloud& cloud, IntImage& indexImage, const DepthImage& depthImage) const {
    indexImage.create(depthImage.rows, depthImage.cols);
    const pwn_hip_converter_params p = stageParams(0.1f);
    ctx.check(pwn_hip_unproject(ctx.handle(), &p, _transform.data(), depthImage.data.data(), depthImage.rows, depthImage.cols, cloud.handle(), indexImage.data.data()));
  }
  // projectIntervals(intervalImage, depthImage, worldRadius) (.cpp:135-147)
  void projectIntervals(Context& ctx, IntImage& intervalImage, const DepthImage& depthImage, float worldRadius) const {
    intervalImage.create(depthImage.rows, depthImage.cols);
    const pwn_hip_converter_params p = stageParams(worldRadius);
    ctx.check(pwn_hip_project_intervals(ctx.handle(), &p, depthImage.data.data(), depthImage.rows, depthImage.cols, intervalImage.data.data()));
  }
  void project(Context& ctx, IntImage& indexImage, DepthImage& depthImage, const Cloud& cloud) const {  // .cpp:33-66
    indexImage.create(_imageRows, _imageCols); depthImage.create(_imageRows, _imageCols);
    ctx.check(pwn_hip_project(ctx.handle(), _cameraMatrix.data(), _transform.data(), _minDistance, _maxDistance, _imageRows, _imageCols,
                              cloud.handle(), indexImage.data.data(), depthImage.data.data()));
  }
 private:
  pwn_hip_converter_params stageParams(float worldRadius) const {
    pwn_hip_converter_params p; pwn_hip_default_converter_params(&p);
    std::memcpy(p.K, _cameraMatrix.data(), sizeof(p.K));
    p.min_distance = _minDistance; p.max_distance = _maxDistance; p.world_radius = worldRadius;
    return p;
  }
  Matrix3f _cameraMatrix; Isometry3f _transform;
  float _minDistance = 0.01f, _maxDistance = 6.0f;                                                        // pointprojector.cpp:9-10
  float _baseline = 0.075f, _alpha = 0.1f;                                                                // pinholepointprojector.cpp:10-11
  int _imageRows = 0, _imageCols = 0;
};

// statscalculatorintegralimage.{h,cpp} (defaults .cpp:6-12)
class StatsCalculatorIntegralImage {
 public:
  float worldRadius() const { return _worldRadius; }            void setWorldRadius(float v) { _worldRadius = v; }
  int maxImageRadius() const { return _maxImageRadius; }        void setMaxImageRadius(int v) { _maxImageRadius = v; }
  int minImageRadius() const { return _minImageRadius; }        void setMinImageRadius(int v) { _minImageRadius = v; }
  int minPoints() const { return _minPoints; }                  void setMinPoints(int v) { _minPoints = v; }
  float curvatureThreshold() const { return _curvatureThreshold; } void setCurvatureThreshold(float v) { _curvatureThreshold = v; }
 private:
  float _worldRadius = 0.1f; int _maxImageRadius = 30, _minImageRadius = 10, _minPoints = 50; float _curvatureThreshold = 0.02f;
};
// informationmatrixcalculator.h:95-153
class InformationMatrixCalculator {
 public:
  InformationMatrixCalculator(float f0, float f1, float f2) { _flat[0] = f0; _flat[1] = f1; _flat[2] = f2; _nonFlat[0] = _nonFlat[1] = _nonFlat[2] = 1.f; }
  float curvatureThreshold() const { return _curvatureThreshold; } void setCurvatureThreshold(float v) { _curvatureThreshold = v; }
  const float* flatDiagonal() const { return _flat; }  const float* nonFlatDiagonal() const { return _nonFlat; }
  Matrix3f flatInformationMatrix() const { Matrix3f m; std::memset(m.m, 0, sizeof(m.m)); m(0,0) = _flat[0]; m(1,1) = _flat[1]; m(2,2) = _flat[2]; return m; }        // informationmatrixcalculator.h:58
  Matrix3f nonFlatInformationMatrix() const { Matrix3f m; std::memset(m.m, 0, sizeof(m.m)); m(0,0) = _nonFlat[0]; m(1,1) = _nonFlat[1]; m(2,2) = _nonFlat[2]; return m; }   // :74
  void setFlatInformationMatrix(float a, float b, float c) { _flat[0] = a; _flat[1] = b; _flat[2] = c; }
  void setNonFlatInformationMatrix(float a, float b, float c) { _nonFlat[0] = a; _nonFlat[1] = b; _nonFlat[2] = c; }
 protected:
  float _curvatureThreshold = 0.02f, _flat[3], _nonFlat[3];
};
struct PointInformationMatrixCalculator : InformationMatrixCalculator { PointInformationMatrixCalculator() : InformationMatrixCalculator(1000.f, 1.f, 1.f) {} };
struct NormalInformationMatrixCalculator : InformationMatrixCalculator { NormalInformationMatrixCalculator() : InformationMatrixCalculator(100.f, 100.f, 100.f) {} };

// depthimageconverter.{h,cpp} + depthimageconverterintegralimage.{h,cpp}
class DepthImageConverter {
 public:
  DepthImageConverter(Context* ctx, PinholePointProjector* projector, StatsCalculatorIntegralImage* statsCalculator,
                      PointInformationMatrixCalculator* pointInfo, NormalInformationMatrixCalculator* normalInfo)
      : _ctx(ctx), _projector(projector), _statsCalculator(statsCalculator), _pointInformationMatrixCalculator(pointInfo),
        _normalInformationMatrixCalculator(normalInfo) {}
  virtual ~DepthImageConverter() {}
  PinholePointProjector* projector() { return _projector; }                               void setProjector(PinholePointProjector* p) { _projector = p; }
  StatsCalculatorIntegralImage* statsCalculator() { return _statsCalculator; }            void setStatsCalculator(StatsCalculatorIntegralImage* s) { _statsCalculator = s; }      // depthimageconverter.h:63-104
  PointInformationMatrixCalculator* pointInformationMatrixCalculator() { return _pointInformationMatrixCalculator; }
  void setPointInformationMatrixCalculator(PointInformationMatrixCalculator* c) { _pointInformationMatrixCalculator = c; }
  NormalInformationMatrixCalculator* normalInformationMatrixCalculator() { return _normalInformationMatrixCalculator; }
  void setNormalInformationMatrixCalculator(NormalInformationMatrixCalculator* c) { _normalInformationMatrixCalculator = c; }
  IntImage& indexImage() { return _indexImage; }
  // The reference fills Cloud::gaussians() inside every compute() (depthimageconverterintegralimage.cpp:39); only Merger::merge reads
  // them, so here they are produced when asked for (clouds that will enter a scene).
  bool computeGaussians() const { return _computeGaussians; }  void setComputeGaussians(bool v) { _computeGaussians = v; }
  // The batch calls make lean clouds; with either flag they make scene-ready ones inside the same submission (pwn_hip_convert_batch_ex): the Stats
  // Cloud::save writes and PwnMerger copies (compute() keeps them whenever it computes Gaussians), and the Gaussians
  bool keepStats() const { return _keepStats; }  void setKeepStats(bool v) { _keepStats = v; }
  // the extras of a batch conversion with the two options given; false when both are off (the lean call)
  bool extras(pwn_hip_convert_extras& e, bool keepStats, bool gaussians) const {
    pwn_hip_default_convert_extras(&e);
    e.keep_stats = keepStats ? 1 : 0; e.gaussians = gaussians ? 1 : 0;
    e.baseline = _projector->baseline(); e.alpha = _projector->alpha();
    return keepStats || gaussians;
  }
  virtual void compute(Cloud& cloud, const DepthImage& depthImage, const Isometry3f& sensorOffset = Isometry3f::Identity()) = 0;
  pwn_hip_converter_params params(const Isometry3f& sensorOffset) const {
    if (!_projector || !_statsCalculator || !_pointInformationMatrixCalculator || !_normalInformationMatrixCalculator)
      throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImageConverter: missing collaborator");          // depthimageconverterintegralimage.cpp:18-21
    pwn_hip_converter_params p; pwn_hip_default_converter_params(&p);
    std::memcpy(p.K, _projector->cameraMatrix().data(), sizeof(p.K));
    p.min_distance = _projector->minDistance(); p.max_distance = _projector->maxDistance();
    p.world_radius = _statsCalculator->worldRadius(); p.min_image_radius = _statsCalculator->minImageRadius();
    p.max_image_radius = _statsCalculator->maxImageRadius(); p.min_points = _statsCalculator->minPoints();
    p.stats_curvature_threshold = _statsCalculator->curvatureThreshold();
    p.point_info_curvature_threshold = _pointInformationMatrixCalculator->curvatureThreshold();
    p.normal_info_curvature_threshold = _normalInformationMatrixCalculator->curvatureThreshold();
    for (int i = 0; i < 3; ++i) {
      p.point_flat_diag[i] = _pointInformationMatrixCalculator->flatDiagonal()[i]; p.point_nonflat_diag[i] = _pointInformationMatrixCalculator->nonFlatDiagonal()[i];
      p.normal_flat_diag[i] = _normalInformationMatrixCalculator->flatDiagonal()[i]; p.normal_nonflat_diag[i] = _normalInformationMatrixCalculator->nonFlatDiagonal()[i];
    }
    std::memcpy(p.sensor_offset, sensorOffset.data(), sizeof(p.sensor_offset));
    return p;
  }
 protected:
  Context* _ctx; PinholePointProjector* _projector; StatsCalculatorIntegralImage* _statsCalculator;
  PointInformationMatrixCalculator* _pointInformationMatrixCalculator; NormalInformationMatrixCalculator* _normalInformationMatrixCalculator;
  IntImage _indexImage;
  bool _computeGaussians = false, _keepStats = false;
};
class DepthImageConverterIntegralImage : public DepthImageConverter {
 public:
  using DepthImageConverter::DepthImageConverter;
  // n independent frames of equal size in one call (what a closure batch or a cache refill converts at once): depthFrames[i] -> *clouds[i].
  // The frame pointers may be host or device memory; the raw variant takes uint16 millimetre frames and fuses
  // DepthImage_convert_16UC1_to_32FC1(depthScale) in front.  Side effects on the projector as in compute().
  void computeBatch(const std::vector<Cloud*>& clouds, const std::vector<const float*>& depthFrames, int rows, int cols,
                    const Isometry3f& sensorOffset = Isometry3f::Identity()) {
    if (clouds.size() != depthFrames.size()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "computeBatch: list sizes differ");
    const pwn_hip_converter_params p = params(sensorOffset);
    _projector->setImageSize(rows, cols); _projector->setTransform(Isometry3f::Identity());
    std::vector<pwn_hip_cloud*> h(clouds.size());
    for (size_t i = 0; i < h.size(); ++i) h[i] = clouds[i]->handle();
    pwn_hip_convert_extras e;
    if (extras(e, _keepStats, _computeGaussians))
      _ctx->check(pwn_hip_convert_batch_ex(_ctx->handle(), &p, reinterpret_cast<const void* const*>(depthFrames.data()), 0, 0.f, (int)h.size(), rows, cols, 0, 0.f, &e, h.data()));
    else _ctx->check(pwn_hip_convert_batch(_ctx->handle(), &p, depthFrames.data(), (int)h.size(), rows, cols, h.data()));
  }
  void computeBatchRaw(const std::vector<Cloud*>& clouds, const std::vector<const uint16_t*>& rawFrames, float depthScale, int rows, int cols,
                       const Isometry3f& sensorOffset = Isometry3f::Identity()) {
    if (clouds.size() != rawFrames.size()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "computeBatchRaw: list sizes differ");
    const pwn_hip_converter_params p = params(sensorOffset);
    _projector->setImageSize(rows, cols); _projector->setTransform(Isometry3f::Identity());
    std::vector<pwn_hip_cloud*> h(clouds.size());
    for (size_t i = 0; i < h.size(); ++i) h[i] = clouds[i]->handle();
    pwn_hip_convert_extras e;
    if (extras(e, _keepStats, _computeGaussians))
      _ctx->check(pwn_hip_convert_batch_ex(_ctx->handle(), &p, reinterpret_cast<const void* const*>(rawFrames.data()), 1, depthScale, (int)h.size(), rows, cols, 0, 0.f, &e,
                                           h.data()));
    else _ctx->check(pwn_hip_convert_batch_u16(_ctx->handle(), &p, rawFrames.data(), depthScale, (int)h.size(), rows, cols, h.data()));
  }
  // the look-ahead of a sharded PwnCloser::processPartition (pwn_hip_convert_export_begin / _end): returns at once; the helper thread converts the raw
  // frame into `cloud` and then writes the cloud's flat form into flatDst (may be nullptr); computeExportEnd waits and returns the bytes written
  void computeExportBegin(Cloud& cloud, const uint16_t* rawFrame, float depthScale, int rows, int cols, void* flatDst, size_t flatBytes,
                          const Isometry3f& sensorOffset = Isometry3f::Identity()) {
    const pwn_hip_converter_params p = params(sensorOffset);
    _ctx->check(pwn_hip_convert_export_begin(_ctx->handle(), &p, rawFrame, depthScale, rows, cols, cloud.handle(), flatDst, flatBytes));
  }
  size_t computeExportEnd(Cloud& cloud, float* jobMs = nullptr) {
    size_t w = 0;
    _ctx->check(pwn_hip_convert_export_end(_ctx->handle(), cloud.handle(), &w, jobMs));
    return w;
  }
  void compute(Cloud& cloud, const DepthImage& depthImage, const Isometry3f& sensorOffset = Isometry3f::Identity()) override {
    if (depthImage.rows <= 0 || depthImage.cols <= 0) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImageConverterIntegralImage: depthImage has zero size");
    const pwn_hip_converter_params p = params(sensorOffset);
    _projector->setImageSize(depthImage.rows, depthImage.cols);                 // depthimageconverterintegralimage.cpp:30
    _projector->setTransform(Isometry3f::Identity());                           // :38
    _indexImage.create(depthImage.rows, depthImage.cols);
    _ctx->check(pwn_hip_convert(_ctx->handle(), &p, depthImage.data.data(), depthImage.rows, depthImage.cols, cloud.handle(),
                                _indexImage.data.data(), nullptr, _computeGaussians ? 1 : 0));      // scene clouds keep their Stats (Cloud::save)
    if (_computeGaussians)
      _ctx->check(pwn_hip_cloud_gaussians(_ctx->handle(), &p, depthImage.data.data(), depthImage.rows, depthImage.cols, cloud.handle(),
                                          _projector->baseline(), _projector->alpha()));
  }
};

// merger.{h,cpp} (defaults merger.cpp:6-8)
class Merger {
 public:
  float distanceThreshold() const { return _distanceThreshold; }  void setDistanceThreshold(float v) { _distanceThreshold = v; }
  float normalThreshold() const { return _normalThreshold; }      void setNormalThreshold(float v) { _normalThreshold = v; }
  float maxPointDepth() const { return _maxPointDepth; }          void setMaxPointDepth(float v) { _maxPointDepth = v; }
  DepthImageConverter* depthImageConverter() const { return _depthImageConverter; }
  void setDepthImageConverter(DepthImageConverter* c) { _depthImageConverter = c; }
  void setImageSize(int r, int c) { _rows = r; _cols = c; }
  void imageSize(int& r, int& c) const { r = _rows; c = _cols; }                // merger.h: the size of the merger's index / depth images
  const std::vector<int>& collapsedIndices() const { return _collapsedIndices; }
  // needs the cloud's sensor-noise Gaussians (pwn_hip_cloud_gaussians after every convert that feeds the scene)
  void merge(Cloud* cloud, Isometry3f transform = Isometry3f::Identity()) {
    if (_rows <= 0 || _cols <= 0) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Merger: _indexImage has zero size");
    if (!_depthImageConverter || !_depthImageConverter->projector()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Merger: missing _depthImageConverter / projector");
    PinholePointProjector* pp = _depthImageConverter->projector();
    pp->setTransform(transform);                                                 // merger.cpp:20-21
    _collapsedIndices.assign(cloud->size(), -1);
    int k = 0;
    Context* ctx = cloud->context();
    ctx->check(pwn_hip_merge(ctx->handle(), cloud->handle(), pp->cameraMatrix().data(), transform.data(), pp->minDistance(), pp->maxDistance(), _rows, _cols,
                             _distanceThreshold, _normalThreshold, _maxPointDepth, &k, _collapsedIndices.empty() ? nullptr : _collapsedIndices.data()));
  }
 protected:
  float _distanceThreshold = 0.1f, _normalThreshold = std::cos(10 * (float)M_PI / 180.0f), _maxPointDepth = 10.0f;
  DepthImageConverter* _depthImageConverter = nullptr;
  int _rows = 0, _cols = 0;
  std::vector<int> _collapsedIndices;
};

// voxelcalculator.{h,cpp}
class VoxelCalculator {
 public:
  float resolution() const { return _resolution; }  void setResolution(float r) { _resolution = r; }
  void compute(Cloud& cloud, float res) { const float old = _resolution; _resolution = res; compute(cloud); _resolution = old; }
  void compute(Cloud& cloud) { int k = 0; Context* ctx = cloud.context(); ctx->check(pwn_hip_voxelize(ctx->handle(), cloud.handle(), _resolution, &k, nullptr)); }
 protected:
  float _resolution = 0.01f;
};

// correspondencefinder.{h,cpp} (defaults .cpp:9-18)
class CorrespondenceFinder {
 public:
  float inlierDistanceThreshold() const { return _inlierDistanceThreshold; }            void setInlierDistanceThreshold(float v) { _inlierDistanceThreshold = v; }
  float inlierNormalAngularThreshold() const { return _inlierNormalAngularThreshold; }  void setInlierNormalAngularThreshold(float v) { _inlierNormalAngularThreshold = v; }
  float flatCurvatureThreshold() const { return _flatCurvatureThreshold; }              void setFlatCurvatureThreshold(float v) { _flatCurvatureThreshold = v; }
  float inlierCurvatureRatioThreshold() const { return _inlierCurvatureRatioThreshold; } void setInlierCurvatureRatioThreshold(float v) { _inlierCurvatureRatioThreshold = v; }
  float squaredThreshold() const { return _inlierDistanceThreshold * _inlierDistanceThreshold; }                          // correspondencefinder.h:133
  void setImageSize(int r, int c) { _rows = r; _cols = c; }
  int imageRows() const { return _rows; }  int imageCols() const { return _cols; }
  int numCorrespondences() const { return _numCorrespondences; }
  // (referenceIndex, currentIndex) pairs of the last Aligner::computeCorrespondences: the first numCorrespondences() are valid, in
  // row-major pixel order, the rest are (-1,-1) (correspondencefinder.cpp:116-117)
  const std::vector<int>& correspondences() const { return _correspondences; }
  int numCandidates() const { return _numCandidates; }
  IntImage& referenceIndexImage() { return _referenceIndexImage; }  IntImage& currentIndexImage() { return _currentIndexImage; }
  DepthImage& referenceDepthImage() { return _referenceDepthImage; }  DepthImage& currentDepthImage() { return _currentDepthImage; }
 private:
  friend class Aligner;
  float _inlierDistanceThreshold = 0.5f, _inlierNormalAngularThreshold = (float)std::cos(M_PI / 6), _flatCurvatureThreshold = 0.02f,
        _inlierCurvatureRatioThreshold = 1.3f;
  int _rows = 0, _cols = 0, _numCorrespondences = 0, _numCandidates = 0;
  std::vector<int> _correspondences;
  IntImage _referenceIndexImage, _currentIndexImage; DepthImage _referenceDepthImage, _currentDepthImage;
};
class Aligner;
// linearizer.{h,cpp} (defaults .cpp:9-15)
class Linearizer {
 public:
  void setAligner(Aligner* a) { _aligner = a; }  Aligner* aligner() { return _aligner; }
  Isometry3f T() const { return _T; }  void setT(Isometry3f T) { T.forceLastRow(); _T = T; }                         // linearizer.h:55,62-65
  float inlierMaxChi2() const { return _inlierMaxChi2; }  void setInlierMaxChi2(float v) { _inlierMaxChi2 = v; }
  bool robustKernel() const { return _robustKernel; }      void setRobustKernel(bool v) { _robustKernel = v; }
  float error() const { return _error; }  int inliers() const { return _inliers; }
  const Matrix6f& H() const { return _H; }  const Vector6f& b() const { return _b; }       // filled by Aligner::align when statistics are computed
 private:
  friend class Aligner;
  Aligner* _aligner = nullptr; float _inlierMaxChi2 = 9e3f; bool _robustKernel = true; float _error = 0.f; int _inliers = 0;
  Matrix6f _H; Vector6f _b; Isometry3f _T;
};

// aligner.{h,cpp}
class Aligner {
 public:
  explicit Aligner(Context* ctx) : _ctx(ctx) {}
  virtual ~Aligner() {}
  void setProjector(PinholePointProjector* p) { _projector = p; }            PinholePointProjector* projector() { return _projector; }
  void setLinearizer(Linearizer* l) { _linearizer = l; if (l) l->setAligner(this); }  Linearizer* linearizer() { return _linearizer; }
  void setCorrespondenceFinder(CorrespondenceFinder* f) { _correspondenceFinder = f; } CorrespondenceFinder* correspondenceFinder() { return _correspondenceFinder; }
  Cloud* referenceCloud() { return _referenceCloud; }  Cloud* currentCloud() { return _currentCloud; }
  const Isometry3f& initialGuess() const { return _initialGuess; }
  const Isometry3f& sensorOffset() const { return _referenceSensorOffset; }                                           // aligner.h:141
  const Isometry3f& referenceSensorOffset() const { return _referenceSensorOffset; }  const Isometry3f& currentSensorOffset() const { return _currentSensorOffset; }
  // aligner.h:216-239: _debug only switches the reference's terminal output on, _minInliers is never read (aligner.cpp:28): inert state, kept for configuration code
  bool debug() const { return _debug; }  void setDebug(bool v) { _debug = v; }  int minInliers() const { return _minInliers; }  void setMinInliers(int v) { _minInliers = v; }
  void setReferenceCloud(Cloud* c) { _referenceCloud = c; clearPriors(); }                                           // aligner.h:60-63: setting a cloud clears the priors
  void setCurrentCloud(Cloud* c) { _currentCloud = c; clearPriors(); }                                               // aligner.h:77-80
  // aligner.cpp:34-47, se3_prior.h
  void addRelativePrior(const Isometry3f& mean, const Matrix6f& informationMatrix) { _priors.push_back(makePrior(0, mean, Isometry3f::Identity(), informationMatrix)); }
  void addAbsolutePrior(const Isometry3f& referenceTransform, const Isometry3f& mean, const Matrix6f& informationMatrix) {
    _priors.push_back(makePrior(1, mean, referenceTransform, informationMatrix));
  }
  void clearPriors() { _priors.clear(); }
  size_t numPriors() const { return _priors.size(); }
  // Aligner::_computeStatistics (aligner.cpp:127,152-199) costs one more linearizer pass and 6x6 host math; the reference always runs it,
  // here it is run when asked for (the tracker and the closer never read its outputs)
  bool computeStatistics() const { return _computeStatistics; }  void setComputeStatistics(bool v) { _computeStatistics = v; }
  const Matrix6f& omega() const { return _omega; }                                                                    // aligner.h:314
  const Vector6f& mean() const { return _mean; }
  float translationalEigenRatio() const { return _translationalEigenRatio; }  float rotationalEigenRatio() const { return _rotationalEigenRatio; }
  float translationalMinEigenRatio() const { return _translationalMinEigenRatio; }  void setTranslationalMinEigenRatio(float v) { _translationalMinEigenRatio = v; }
  float rotationalMinEigenRatio() const { return _rotationalMinEigenRatio; }        void setRotationalMinEigenRatio(float v) { _rotationalMinEigenRatio = v; }
  bool solutionValid() const {                                                                                         // aligner.cpp:128-129
    return !(_rotationalEigenRatio > _rotationalMinEigenRatio || _translationalEigenRatio > _translationalMinEigenRatio);
  }
  int outerIterations() const { return _outerIterations; }  void setOuterIterations(int n) { _outerIterations = n; }
  int innerIterations() const { return _innerIterations; }  void setInnerIterations(int n) { _innerIterations = n; }
  const Isometry3f& T() const { return _T; }
  void setInitialGuess(Isometry3f g) { g.forceLastRow(); _initialGuess = g; }                                        // aligner.h:130-133
  void setSensorOffset(Isometry3f o) { o.forceLastRow(); _referenceSensorOffset = o; _currentSensorOffset = o; }     // :149-153
  void setReferenceSensorOffset(Isometry3f o) { o.forceLastRow(); _referenceSensorOffset = o; }
  void setCurrentSensorOffset(Isometry3f o) { o.forceLastRow(); _currentSensorOffset = o; }
  float error() const { return _error; }  int inliers() const { return _inliers; }  double totalTime() const { return _totalTime; }
  const pwn_hip_align_result& result() const { return _result; }
  // the step norms of the pairs [first, first + n) of the context's last alignment call (Context::lastAlignSteps)
  std::vector<pwn_hip_align_steps> lastSteps(int first = 0, int n = 1) { return _ctx->lastAlignSteps(first, n); }
  pwn_hip_aligner_params params() const {
    if (!_projector || !_linearizer || !_correspondenceFinder) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner: missing collaborator");   // aligner.cpp:50-52
    pwn_hip_aligner_params p; pwn_hip_default_aligner_params(&p);
    std::memcpy(p.K, _projector->cameraMatrix().data(), sizeof(p.K));
    p.min_distance = _projector->minDistance(); p.max_distance = _projector->maxDistance();
    p.rows = _projector->imageRows(); p.cols = _projector->imageCols();
    p.inlier_distance_threshold = _correspondenceFinder->inlierDistanceThreshold();
    p.inlier_normal_angular_threshold = _correspondenceFinder->inlierNormalAngularThreshold();
    p.flat_curvature_threshold = _correspondenceFinder->flatCurvatureThreshold();
    p.inlier_curvature_ratio_threshold = _correspondenceFinder->inlierCurvatureRatioThreshold();
    p.inlier_max_chi2 = _linearizer->inlierMaxChi2(); p.robust_kernel = _linearizer->robustKernel() ? 1 : 0;
    p.outer_iterations = _outerIterations; p.inner_iterations = _innerIterations;
    std::memcpy(p.reference_sensor_offset, _referenceSensorOffset.data(), 64);
    std::memcpy(p.current_sensor_offset, _currentSensorOffset.data(), 64);
    std::memcpy(p.initial_guess, _initialGuess.data(), 64);
    return p;
  }
  // aligner.cpp:49-125 ; fetchImages: also fill the finder's index / depth images (read by matchClouds)
  virtual void align(bool fetchImages = false) {
    if (!_referenceCloud || !_currentCloud) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner: missing cloud");
    const pwn_hip_aligner_params p = params();
    pwn_hip_align_statistics q;
    // the call the binding makes: the prior terms in every iteration (aligner.cpp:96-108), _computeStatistics after the loop as always (:127);
    // without priors it is pwn_hip_align_batch_ex for one pair
    _ctx->check(pwn_hip_align_with_priors_ex(_ctx->handle(), &p, _referenceCloud->handle(), _currentCloud->handle(), (int)_priors.size(),
                                             _priors.empty() ? nullptr : _priors.data(), &_result, _computeStatistics ? &q : nullptr));
    if (_computeStatistics) {
      std::memcpy(_omega.m, q.omega, sizeof(q.omega)); std::memcpy(_mean.v, q.mean, sizeof(q.mean));
      _translationalEigenRatio = q.translational_eigen_ratio; _rotationalEigenRatio = q.rotational_eigen_ratio;
      std::memcpy(_linearizer->_H.m, q.H, sizeof(q.H)); std::memcpy(_linearizer->_b.v, q.b, sizeof(q.b));
    }
    _T = Isometry3f(_result.T); _error = _result.error; _inliers = _result.inliers; _totalTime = _result.total_time_ms;
    _linearizer->_error = _error; _linearizer->_inliers = _inliers;
    _linearizer->setT(_T.inverse());      // what the reference leaves there: _linearizer->setT(_T.inverse()) in _computeStatistics (aligner.cpp:165-167)
    _correspondenceFinder->_numCorrespondences = _result.iterations > 0 ? _result.iter_correspondences[_result.iterations - 1] : 0;
    if (fetchImages) {
      CorrespondenceFinder& f = *_correspondenceFinder;
      f._referenceIndexImage.create(p.rows, p.cols); f._currentIndexImage.create(p.rows, p.cols);
      f._referenceDepthImage.create(p.rows, p.cols); f._currentDepthImage.create(p.rows, p.cols);
      _ctx->check(pwn_hip_align_images(_ctx->handle(), f._referenceIndexImage.data.data(), f._referenceDepthImage.data.data(),
                                       f._currentIndexImage.data.data(), f._currentDepthImage.data.data()));
    }
  }
  // n independent alignments with this aligner's parameters (the candidate loop of PwnCloser::processPartition, pwn_closer.cpp:92-111);
  // initialGuesses: n isometries or empty (= this aligner's initial guess for all); scores: optional depth-agreement scores of matchClouds
  std::vector<pwn_hip_align_result> alignBatch(const std::vector<Cloud*>& references, const std::vector<Cloud*>& currents,
                                               const std::vector<Isometry3f>& initialGuesses = std::vector<Isometry3f>(),
                                               std::vector<pwn_hip_match_result>* scores = nullptr, float frameInlierDepthThreshold = 50.f) {
    const size_t n = references.size();
    if (currents.size() != n || (!initialGuesses.empty() && initialGuesses.size() != n)) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::alignBatch: list sizes differ");
    std::vector<pwn_hip_align_result> results(n);
    if (n == 0) return results;
    const pwn_hip_aligner_params p = params();
    std::vector<pwn_hip_cloud*> r(n), c(n);
    for (size_t i = 0; i < n; ++i) {
      if (!references[i] || !currents[i]) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::alignBatch: null cloud");
      r[i] = references[i]->handle(); c[i] = currents[i]->handle();
    }
    std::vector<float> g;
    for (const Isometry3f& T : initialGuesses) { Isometry3f t = T; t.forceLastRow(); g.insert(g.end(), t.m, t.m + 16); }
    if (scores) scores->resize(n);
    _ctx->check(pwn_hip_align_batch_ex(_ctx->handle(), &p, (int)n, r.data(), c.data(), g.empty() ? nullptr : g.data(), results.data(),
                                       frameInlierDepthThreshold, scores ? scores->data() : nullptr, nullptr));
    return results;
  }
  // The same with SE(3) priors per pair, the loop on the device (pwn_hip_align_batch_priors; aligner.cpp:96-108): priors[i] is the list
  // addRelativePrior / addAbsolutePrior would have queued for pair i (relativePrior / absolutePrior below make the records), in that order.
  // This aligner's own list belongs to align() and is not used.
  typedef std::vector<std::vector<pwn_hip_prior>> PairPriors;
  static pwn_hip_prior relativePrior(const Isometry3f& mean, const Matrix6f& informationMatrix) { return makePrior(0, mean, Isometry3f::Identity(), informationMatrix); }
  static pwn_hip_prior absolutePrior(const Isometry3f& referenceTransform, const Isometry3f& mean, const Matrix6f& informationMatrix) {
    return makePrior(1, mean, referenceTransform, informationMatrix);
  }
  std::vector<pwn_hip_align_result> alignBatch(const std::vector<Cloud*>& references, const std::vector<Cloud*>& currents, const std::vector<Isometry3f>& initialGuesses,
                                               const PairPriors& priors, std::vector<pwn_hip_match_result>* scores = nullptr, float frameInlierDepthThreshold = 50.f) {
    return alignBatchPriors(references, currents, initialGuesses, priors, scores, frameInlierDepthThreshold, nullptr, 0, std::vector<int>(), 0);
  }
  // alignBatch whose results also leave as fixed-size records written on the device (PWN_HIP_RECORD_FLOATS floats each, device or host buffer;
  // pair id = pairIds[i], else firstPairId + i); priors: empty, or one list per pair as above
  std::vector<pwn_hip_align_result> alignBatchRecords(const std::vector<Cloud*>& references, const std::vector<Cloud*>& currents, float* records,
                                                      const std::vector<Isometry3f>& initialGuesses = std::vector<Isometry3f>(),
                                                      const PairPriors& priors = PairPriors(), const std::vector<int>& pairIds = std::vector<int>(),
                                                      int firstPairId = 0) {
    if (!records) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::alignBatchRecords: null records");
    return alignBatchPriors(references, currents, initialGuesses, priors, nullptr, 0.f, records, PWN_HIP_RECORD_FLOATS, pairIds, firstPairId);
  }
  // One candidate batch from raw uint16 frames as one submission (pwn_hip_convert_align_batch_u16): per pair PwnMatcherBase::makeCloud of both
  // frames (pwn_matcher_base.cpp:77-85), then align; `records` (optional): device or host buffer of n * PWN_HIP_RECORD_FLOATS floats that
  // receives the fixed-size result records (pair id = firstPairId + i) straight from the device.
  std::vector<pwn_hip_align_result> convertAlignBatch(DepthImageConverter& converter, const std::vector<Cloud*>& references, const std::vector<Cloud*>& currents,
                                                      const std::vector<const uint16_t*>& refFrames, const std::vector<const uint16_t*>& curFrames,
                                                      float depthScale, int rows, int cols, float* records = nullptr, int firstPairId = 0) {
    const size_t n = references.size();
    if (currents.size() != n || refFrames.size() != n || curFrames.size() != n) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::convertAlignBatch: list sizes differ");
    std::vector<pwn_hip_align_result> results(n);
    if (n == 0) return results;
    const pwn_hip_converter_params cp = converter.params(Isometry3f::Identity());
    converter.projector()->setImageSize(rows, cols); converter.projector()->setTransform(Isometry3f::Identity());      // side effects of compute() (depthimageconverterintegralimage.cpp:30,38)
    const pwn_hip_aligner_params p = params();
    std::vector<pwn_hip_cloud*> r(n), c(n);
    for (size_t i = 0; i < n; ++i) {
      if (!references[i] || !currents[i]) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::convertAlignBatch: null cloud");
      r[i] = references[i]->handle(); c[i] = currents[i]->handle();
    }
    _ctx->check(pwn_hip_convert_align_batch_u16(_ctx->handle(), &cp, &p, (int)n, refFrames.data(), curFrames.data(), depthScale, rows, cols, r.data(), c.data(),
                                                nullptr, nullptr, firstPairId, results.data(), records));
    return results;
  }
  // stage-level entry points with explicit inputs: CorrespondenceFinder::compute(reference, current, T) on two index images
  // (correspondencefinder.cpp:20-118) and Linearizer::update() with _T = T on the finder's correspondences (linearizer.cpp:17-115)
  void computeCorrespondences(const IntImage& referenceIndexImage, const IntImage& currentIndexImage, const Isometry3f& T) {
    if (!_referenceCloud || !_currentCloud) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner: missing cloud");
    const pwn_hip_aligner_params p = params();
    CorrespondenceFinder& f = *_correspondenceFinder;
    f._correspondences.assign((size_t)p.rows * p.cols * 2, -1);
    _ctx->check(pwn_hip_correspondences(_ctx->handle(), &p, _referenceCloud->handle(), _currentCloud->handle(), referenceIndexImage.data.data(),
                                        currentIndexImage.data.data(), T.data(), f._correspondences.data(), &f._numCorrespondences, &f._numCandidates));
  }
  void linearize(const Isometry3f& T) {
    if (!_referenceCloud || !_currentCloud) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner: missing cloud");
    const pwn_hip_aligner_params p = params();
    CorrespondenceFinder& f = *_correspondenceFinder;
    _ctx->check(pwn_hip_linearize(_ctx->handle(), &p, _referenceCloud->handle(), _currentCloud->handle(), f._correspondences.data(), f._numCorrespondences,
                                  T.data(), _linearizer->_H.m, _linearizer->_b.v, &_linearizer->_error, &_linearizer->_inliers));
  }
  Context* context() const { return _ctx; }
 protected:
  static pwn_hip_prior makePrior(int kind, const Isometry3f& mean, const Isometry3f& referenceTransform, const Matrix6f& info) {
    pwn_hip_prior q; q.kind = kind;
    std::memcpy(q.mean, mean.data(), sizeof(q.mean)); std::memcpy(q.reference_transform, referenceTransform.data(), sizeof(q.reference_transform));
    std::memcpy(q.information, info.data(), sizeof(q.information));
    return q;
  }
  // what the two batch calls with priors share: the handle, guess and prior arrays, and the one call (priors empty: no list is passed, the
  // launches of the call without priors)
  std::vector<pwn_hip_align_result> alignBatchPriors(const std::vector<Cloud*>& references, const std::vector<Cloud*>& currents, const std::vector<Isometry3f>& initialGuesses,
                                                     const PairPriors& priors, std::vector<pwn_hip_match_result>* scores, float frameInlierDepthThreshold,
                                                     float* records, int recordFloats, const std::vector<int>& pairIds, int firstPairId) {
    const size_t n = references.size();
    if (currents.size() != n || (!initialGuesses.empty() && initialGuesses.size() != n) || (!priors.empty() && priors.size() != n) ||
        (!pairIds.empty() && pairIds.size() < n))
      throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::alignBatch: list sizes differ");
    std::vector<pwn_hip_align_result> results(n);
    if (n == 0) return results;
    const pwn_hip_aligner_params p = params();
    std::vector<pwn_hip_cloud*> r(n), c(n);
    for (size_t i = 0; i < n; ++i) {
      if (!references[i] || !currents[i]) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "Aligner::alignBatch: null cloud");
      r[i] = references[i]->handle(); c[i] = currents[i]->handle();
    }
    std::vector<float> g;
    for (const Isometry3f& T : initialGuesses) { Isometry3f t = T; t.forceLastRow(); g.insert(g.end(), t.m, t.m + 16); }
    std::vector<int> first(n + 1, 0);
    std::vector<pwn_hip_prior> flat;
    for (size_t i = 0; i < priors.size(); ++i) { flat.insert(flat.end(), priors[i].begin(), priors[i].end()); first[i + 1] = (int)flat.size(); }
    const pwn_hip_pair_priors pp = { first.data(), flat.data() };
    if (scores) scores->resize(n);
    _ctx->check(pwn_hip_align_batch_priors(_ctx->handle(), &p, (int)n, r.data(), c.data(), g.empty() ? nullptr : g.data(), priors.empty() ? nullptr : &pp,
                                           frameInlierDepthThreshold, pairIds.empty() ? nullptr : pairIds.data(), firstPairId, results.data(),
                                           scores ? scores->data() : nullptr, nullptr, records, recordFloats));
    return results;
  }
  Context* _ctx;
  PinholePointProjector* _projector = nullptr; Linearizer* _linearizer = nullptr; CorrespondenceFinder* _correspondenceFinder = nullptr;
  Cloud* _referenceCloud = nullptr; Cloud* _currentCloud = nullptr; bool _debug = false; int _minInliers = 100;
  std::vector<pwn_hip_prior> _priors;
  bool _computeStatistics = false;
  Matrix6f _omega; Vector6f _mean;
  float _translationalEigenRatio = 3.402823466e+38f, _rotationalEigenRatio = 3.402823466e+38f;
  float _translationalMinEigenRatio = 50.f, _rotationalMinEigenRatio = 50.f;                                          // aligner.cpp:29-30
  int _outerIterations = 10, _innerIterations = 1;                                                                    // aligner.cpp:19-20
  Isometry3f _T, _initialGuess, _referenceSensorOffset, _currentSensorOffset;
  float _error = 0.f; int _inliers = 0; double _totalTime = 0.0;
  pwn_hip_align_result _result;
};

// The mapping loop of pwn_aligner.cpp:166-209 (pwn_odometry_sequential_controller.cpp:124-171), a frame per processFrame and a submission per
// frame (pwn_hip_scene_step): the frame is converted, tracked against the rendering of the scene and fused into it.  The chunk's Cloud::save is
// the caller's: save scene() under sceneT().inverse() * globalT(), then newChunk().
class SceneAligner {
 public:
  SceneAligner(Context* ctx, DepthImageConverter* converter, Aligner* aligner, Merger* merger, int capacity, const Isometry3f& sensorOffset = Isometry3f::Identity(),
               int imageScale = 0, float maxDepthCov = 0.01f)
      : _ctx(ctx), _converter(converter), _aligner(aligner), _merger(merger), _capacity(capacity), _sensorOffset(sensorOffset), _imageScale(imageScale),
        _maxDepthCov(maxDepthCov), _scene(new Cloud(*ctx, capacity)) { _sensorOffset.forceLastRow(); }
  Cloud* scene() { return _scene.get(); }
  Cloud* cloud() { return _cloud.get(); }            // the last frame's cloud, scene-ready
  Cloud* subscene() { return _subscene.get(); }      // what it was tracked against
  const Isometry3f& sceneT() const { return _sceneT; }
  const Isometry3f& globalT() const { return _globalT; }
  const pwn_hip_scene_step_result& result() const { return _result; }
  const std::vector<int>& collapsedIndices() const { return _collapsedIndices; }
  pwn_hip_scene_step_params stepParams() const {
    pwn_hip_scene_step_params sp; pwn_hip_default_scene_step_params(&sp);
    sp.distance_threshold = _merger->distanceThreshold(); sp.normal_threshold = _merger->normalThreshold(); sp.max_point_depth = _merger->maxPointDepth();
    sp.baseline = _converter->projector()->baseline(); sp.alpha = _converter->projector()->alpha();
    sp.step = _imageScale; sp.max_depth_cov = _maxDepthCov;
    return sp;
  }
  // one frame -> Aligner::T() of its alignment against the scene (the identity for the first frame of a chunk)
  Isometry3f processFrame(const DepthImage& depth) { return step(depth.data.data(), 0, 0.f, depth.rows, depth.cols); }
  Isometry3f processFrame(const RawDepthImage& raw, float depthScale) { return step(raw.data.data(), 1, depthScale, raw.rows, raw.cols); }
  // pwn_aligner.cpp:188-199: a new scene that holds the last frame's cloud at the identity; the one it replaces is returned (it holds that
  // frame too: the reference saves its chunk before the frame is added)
  std::unique_ptr<Cloud> newChunk() {
    std::unique_ptr<Cloud> old(new Cloud(*_ctx, _capacity));
    old.swap(_scene);
    _sceneT.setIdentity();
    if (_cloud) {
      _scene->add(*_cloud, _sceneT);
      _merger->merge(_scene.get(), _sceneT * _sensorOffset);
      _converter->projector()->setTransform(Isometry3f::Identity());
    }
    return old;
  }
 private:
  Isometry3f step(const void* frame, int raw, float depthScale, int rows, int cols) {
    const int vrows = _imageScale ? rows / _imageScale : rows, vcols = _imageScale ? cols / _imageScale : cols;
    if (!_cloud || _pixels < vrows * vcols) { _cloud.reset(new Cloud(*_ctx, vrows * vcols)); _subscene.reset(new Cloud(*_ctx, vrows * vcols)); _pixels = vrows * vcols; }
    _aligner->projector()->setImageSize(vrows, vcols);
    _merger->setImageSize(vrows, vcols);
    _aligner->setInitialGuess(Isometry3f::Identity()); _aligner->setSensorOffset(_sensorOffset);      // pwn_aligner.cpp:183-184
    const pwn_hip_converter_params cp = _converter->params(_sensorOffset);
    const pwn_hip_aligner_params ap = _aligner->params();
    const pwn_hip_scene_step_params sp = stepParams();
    _collapsedIndices.assign(_scene->size() + (size_t)vrows * vcols, -1);
    _ctx->check(pwn_hip_scene_step(_ctx->handle(), &cp, &ap, &sp, frame, raw, depthScale, rows, cols, _sceneT.data(), _scene->handle(), _cloud->handle(),
                                   _subscene->handle(), &_result, _collapsedIndices.data()));
    _collapsedIndices.resize((size_t)_result.size_after_add);
    const Isometry3f T(_result.align.T);
    _globalT = _globalT * T; _globalT.forceLastRow();
    _sceneT = Isometry3f(_result.scene_T);
    return T;
  }
  Context* _ctx; DepthImageConverter* _converter; Aligner* _aligner; Merger* _merger;
  int _capacity; Isometry3f _sensorOffset; int _imageScale; float _maxDepthCov; int _pixels = 0;
  std::unique_ptr<Cloud> _scene, _cloud, _subscene;
  Isometry3f _sceneT, _globalT;
  pwn_hip_scene_step_result _result;
  std::vector<int> _collapsedIndices;
};

// pwn_tracker/pwn_matcher_base.{h,cpp}: makeCloud + matchClouds with the reference's quirks kept (guess z zeroed :114,
// projector re-configured and scaled per call :117-119, information matrix = 100*I :147-148).
struct PwnMatcherBase {
  struct MatcherResult {
    double transform[16];            // column-major, Aligner::T() widened to double (convertScalar, .h:66-71)
    double informationMatrix[36];
    int cloud_inliers, image_nonZeros, image_outliers, image_inliers;
    float image_reprojectionDistance;
  };
  PwnMatcherBase(Context* ctx, Aligner* aligner, DepthImageConverter* converter) : _ctx(ctx), _aligner(aligner), _converter(converter) {}
  virtual ~PwnMatcherBase() { try { makeCloudDrop(); } catch (...) {} }
  int scale() const { return _scale; }  void setScale(int s) { _scale = s; }
  float frameInlierDepthThreshold() const { return _frameInlierDepthThreshold; }  void setFrameInlierDepthThreshold(float v) { _frameInlierDepthThreshold = v; }
  Aligner* aligner() { return _aligner; }  DepthImageConverter* converter() { return _converter; }
  void setAligner(Aligner* a) { _aligner = a; }  void setConverter(DepthImageConverter* c) { _converter = c; }      // pwn_matcher_base.h:30,33

  // .cpp:57-86: returns a new Cloud owned by the caller; r, c, cameraMatrix receive the scaled values.  DepthImage_scale (:72) and
  // converter->compute (:79) run as one device-side call (no scaled image on the host); same side effects on the converter's projector.
  // keepStats / gaussians: a scene-ready cloud (makeCloudBatch of the one image).
  Cloud* makeCloud(int& r, int& c, Matrix3f& cameraMatrix, const Isometry3f& sensorOffset, const DepthImage& depthImage, bool keepStats = false,
                   bool gaussians = false) {
    if (keepStats || gaussians) return makeCloudBatch(r, c, cameraMatrix, sensorOffset, { &depthImage }, keepStats, gaussians)[0];
    PinholePointProjector* projector = _converter->projector();
    const float invScale = 1.0f / _scale;
    Matrix3f scaled = cameraMatrix;
    for (int i = 0; i < 9; ++i) scaled.m[i] = scaled.m[i] * invScale;
    scaled(2,2) = 1.0f;
    projector->setCameraMatrix(scaled);
    projector->setImageSize(depthImage.rows / _scale, depthImage.cols / _scale);
    projector->setTransform(Isometry3f::Identity());
    cameraMatrix = projector->cameraMatrix(); r = projector->imageRows(); c = projector->imageCols();
    Cloud* cloud = new Cloud(*_ctx, r * c > 0 ? r * c : 1);
    const pwn_hip_converter_params p = _converter->params(sensorOffset);
    const int rc = pwn_hip_convert_scaled(_ctx->handle(), &p, depthImage.data.data(), depthImage.rows, depthImage.cols, _scale, 0.01f, cloud->handle());
    if (rc) { delete cloud; _ctx->check(rc); }
    ++numCalls;
    return cloud;
  }
  // makeCloud of n depth images of one size, camera matrix and sensor offset in one call (pwn_hip_convert_batch_scaled; not in the reference):
  // the clouds are new and owned by the caller, the same bits as n makeCloud calls; r, c, cameraMatrix and the projector as those leave them.
  // keepStats / gaussians: the clouds carry the Stats and the sensor-noise Gaussians the reference's converter always leaves (pwn_hip_convert_batch_ex).
  std::vector<Cloud*> makeCloudBatch(int& r, int& c, Matrix3f& cameraMatrix, const Isometry3f& sensorOffset, const std::vector<const DepthImage*>& depthImages,
                                     bool keepStats = false, bool gaussians = false) {
    std::vector<Cloud*> clouds;
    if (depthImages.empty()) return clouds;
    const int rows = depthImages[0]->rows, cols = depthImages[0]->cols;
    std::vector<const float*> frames(depthImages.size());
    for (size_t i = 0; i < depthImages.size(); ++i) {
      if (depthImages[i]->rows != rows || depthImages[i]->cols != cols) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "makeCloudBatch: images of one call share one size");
      frames[i] = depthImages[i]->data.data();
    }
    PinholePointProjector* projector = _converter->projector();
    const float invScale = 1.0f / _scale;
    Matrix3f scaled = cameraMatrix;
    for (int i = 0; i < 9; ++i) scaled.m[i] = scaled.m[i] * invScale;
    scaled(2,2) = 1.0f;
    projector->setCameraMatrix(scaled);
    projector->setImageSize(rows / _scale, cols / _scale);
    projector->setTransform(Isometry3f::Identity());
    cameraMatrix = projector->cameraMatrix(); r = projector->imageRows(); c = projector->imageCols();
    std::vector<pwn_hip_cloud*> h(frames.size());
    for (size_t i = 0; i < frames.size(); ++i) { clouds.push_back(new Cloud(*_ctx, r * c > 0 ? r * c : 1)); h[i] = clouds.back()->handle(); }
    const pwn_hip_converter_params p = _converter->params(sensorOffset);
    pwn_hip_convert_extras e;
    const int rc = _converter->extras(e, keepStats, gaussians)
        ? pwn_hip_convert_batch_ex(_ctx->handle(), &p, reinterpret_cast<const void* const*>(frames.data()), 0, 0.f, (int)frames.size(), rows, cols, _scale, 0.01f, &e, h.data())
        : pwn_hip_convert_batch_scaled(_ctx->handle(), &p, frames.data(), (int)frames.size(), rows, cols, _scale, 0.01f, h.data());
    if (rc) { for (Cloud* cl : clouds) delete cl; _ctx->check(rc); }
    numCalls += (int)frames.size();
    return clouds;
  }
  // makeCloud in two halves (pwn_hip_convert_scaled_begin / _end; not in the reference): makeCloudBegin returns at once, the frame is
  // converted by the library's helper thread next to whatever runs on the context meanwhile; makeCloudEnd returns the cloud makeCloud would
  // have returned, bit for bit.  One at a time per context; depthImage must stay alive and unchanged in between.
  void makeCloudBegin(Matrix3f cameraMatrix, const Isometry3f& sensorOffset, const DepthImage& depthImage) {
    makeCloudDrop();
    PinholePointProjector* projector = _converter->projector();
    const float invScale = 1.0f / _scale;
    for (int i = 0; i < 9; ++i) cameraMatrix.m[i] = cameraMatrix.m[i] * invScale;
    cameraMatrix(2,2) = 1.0f;
    projector->setCameraMatrix(cameraMatrix);
    projector->setImageSize(depthImage.rows / _scale, depthImage.cols / _scale);
    projector->setTransform(Isometry3f::Identity());
    _pendingK = projector->cameraMatrix(); _pendingR = projector->imageRows(); _pendingC = projector->imageCols();
    Cloud* cloud = new Cloud(*_ctx, _pendingR * _pendingC > 0 ? _pendingR * _pendingC : 1);
    const pwn_hip_converter_params p = _converter->params(sensorOffset);
    const int rc = pwn_hip_convert_scaled_begin(_ctx->handle(), &p, depthImage.data.data(), depthImage.rows, depthImage.cols, _scale, 0.01f, cloud->handle());
    if (rc) { delete cloud; _ctx->check(rc); }
    _pending = cloud; _pendingImage = &depthImage;
  }
  bool makeCloudPending(const DepthImage& depthImage) const { return _pending && _pendingImage == &depthImage; }
  Cloud* makeCloudEnd(int& r, int& c, Matrix3f& cameraMatrix) {
    if (!_pending) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "makeCloudEnd without makeCloudBegin");
    Cloud* cloud = _pending; _pending = nullptr; _pendingImage = nullptr;
    const int rc = pwn_hip_convert_end(_ctx->handle(), cloud->handle());
    if (rc) { delete cloud; _ctx->check(rc); }
    r = _pendingR; c = _pendingC; cameraMatrix = _pendingK;
    ++numCalls;
    return cloud;
  }
  void makeCloudDrop() { if (_pending) { int r, c; Matrix3f K; delete makeCloudEnd(r, c, K); } }
  // .cpp:88-183
  void matchClouds(MatcherResult& result, Cloud* fromCloud, Cloud* toCloud, const Isometry3f& fromOffset, const Isometry3f& toOffset,
                   const Matrix3f& toCameraMatrix, int toRows, int toCols, const Isometry3f& initialGuess = Isometry3f::Identity()) {
    configure(fromOffset, toOffset, toCameraMatrix, toRows, toCols, initialGuess);
    _aligner->setReferenceCloud(fromCloud);
    _aligner->setCurrentCloud(toCloud);
    _aligner->align();
    pwn_hip_match_result m;
    _ctx->check(pwn_hip_match_score(_ctx->handle(), _frameInlierDepthThreshold, &m));
    fill(result, _aligner->result(), m);
  }
  // the candidate loop of PwnCloser::processPartition (pwn_closer.cpp:92-111) as one batched call: results[i] = matchClouds(from[i], to[i])
  void matchCloudsBatch(std::vector<MatcherResult>& results, const std::vector<Cloud*>& fromClouds, const std::vector<Cloud*>& toClouds,
                        const Isometry3f& fromOffset, const Isometry3f& toOffset, const Matrix3f& toCameraMatrix, int toRows, int toCols,
                        const std::vector<Isometry3f>& initialGuesses = std::vector<Isometry3f>()) {
    configure(fromOffset, toOffset, toCameraMatrix, toRows, toCols, Isometry3f::Identity());
    std::vector<Isometry3f> g(fromClouds.size());
    for (size_t i = 0; i < g.size(); ++i) { if (!initialGuesses.empty()) g[i] = initialGuesses[i]; g[i](2,3) = 0.f; g[i].forceLastRow(); }
    std::vector<pwn_hip_match_result> scores;
    const std::vector<pwn_hip_align_result> r = _aligner->alignBatch(fromClouds, toClouds, g, &scores, _frameInlierDepthThreshold);
    results.resize(r.size());
    for (size_t i = 0; i < r.size(); ++i) fill(results[i], r[i], scores[i]);
  }
  // the same call with the results (also) leaving as PWN_HIP_MATCH_RECORD_FLOATS-float records, device or host: what the ranks of a sharded
  // processPartition exchange.  pairIds may be empty (record i then carries firstPairId + i).
  void matchCloudsBatchRecords(float* records, const std::vector<Cloud*>& fromClouds, const std::vector<Cloud*>& toClouds,
                               const Isometry3f& fromOffset, const Isometry3f& toOffset, const Matrix3f& toCameraMatrix, int toRows, int toCols,
                               const std::vector<Isometry3f>& initialGuesses = std::vector<Isometry3f>(), const std::vector<int>& pairIds = std::vector<int>(),
                               int firstPairId = 0, std::vector<MatcherResult>* results = nullptr) {
    configure(fromOffset, toOffset, toCameraMatrix, toRows, toCols, Isometry3f::Identity());
    const int n = (int)fromClouds.size();
    std::vector<float> g((size_t)n * 16);
    for (int i = 0; i < n; ++i) {
      Isometry3f t; if (!initialGuesses.empty()) t = initialGuesses[(size_t)i];
      t(2,3) = 0.f; t.forceLastRow();
      std::memcpy(&g[(size_t)i * 16], t.data(), 16 * sizeof(float));
    }
    std::vector<pwn_hip_cloud*> r((size_t)n), c((size_t)n);
    for (int i = 0; i < n; ++i) { r[(size_t)i] = fromClouds[(size_t)i]->handle(); c[(size_t)i] = toClouds[(size_t)i]->handle(); }
    std::vector<pwn_hip_align_result> res(results ? (size_t)n : 0);
    std::vector<pwn_hip_match_result> sc(results ? (size_t)n : 0);
    const pwn_hip_aligner_params p = _aligner->params();
    _ctx->check(pwn_hip_match_batch_records(_ctx->handle(), &p, n, r.data(), c.data(), g.data(), _frameInlierDepthThreshold,
                                            pairIds.empty() ? nullptr : pairIds.data(), firstPairId, results ? res.data() : nullptr,
                                            results ? sc.data() : nullptr, records));
    if (results) { results->resize((size_t)n); for (int i = 0; i < n; ++i) fill((*results)[(size_t)i], res[(size_t)i], sc[(size_t)i]); }
  }
  // the same with PWN_HIP_CLOSURE_RECORD_FLOATS-float records, which also carry Aligner::omega() computed on the device: a result's
  // informationMatrix is then that omega cast to double (pwn_tracker2/pwn_matcher_base.cpp:158-163), not v1's 100 * I
  void matchCloudsBatchClosureRecords(float* records, const std::vector<Cloud*>& fromClouds, const std::vector<Cloud*>& toClouds,
                                      const Isometry3f& fromOffset, const Isometry3f& toOffset, const Matrix3f& toCameraMatrix, int toRows, int toCols,
                                      const std::vector<Isometry3f>& initialGuesses = std::vector<Isometry3f>(), const std::vector<int>& pairIds = std::vector<int>(),
                                      int firstPairId = 0, std::vector<MatcherResult>* results = nullptr) {
    configure(fromOffset, toOffset, toCameraMatrix, toRows, toCols, Isometry3f::Identity());
    const int n = (int)fromClouds.size();
    std::vector<float> g((size_t)n * 16);
    for (int i = 0; i < n; ++i) {
      Isometry3f t; if (!initialGuesses.empty()) t = initialGuesses[(size_t)i];
      t(2,3) = 0.f; t.forceLastRow();
      std::memcpy(&g[(size_t)i * 16], t.data(), 16 * sizeof(float));
    }
    std::vector<pwn_hip_cloud*> r((size_t)n), c((size_t)n);
    for (int i = 0; i < n; ++i) { r[(size_t)i] = fromClouds[(size_t)i]->handle(); c[(size_t)i] = toClouds[(size_t)i]->handle(); }
    std::vector<pwn_hip_align_result> res(results ? (size_t)n : 0);
    std::vector<pwn_hip_match_result> sc(results ? (size_t)n : 0);
    std::vector<pwn_hip_align_statistics> st(results ? (size_t)n : 0);
    const pwn_hip_aligner_params p = _aligner->params();
    _ctx->check(pwn_hip_closure_batch_records(_ctx->handle(), &p, n, r.data(), c.data(), g.data(), _frameInlierDepthThreshold,
                                              pairIds.empty() ? nullptr : pairIds.data(), firstPairId, results ? res.data() : nullptr,
                                              results ? sc.data() : nullptr, results ? st.data() : nullptr, records));
    if (results) {
      results->resize((size_t)n);
      for (int i = 0; i < n; ++i) {
        fill((*results)[(size_t)i], res[(size_t)i], sc[(size_t)i]);
        for (int k = 0; k < 36; ++k) (*results)[(size_t)i].informationMatrix[k] = (double)st[(size_t)i].omega[k];
      }
    }
  }
  int numCalls = 0;
 protected:
  void configure(const Isometry3f& fromOffset, const Isometry3f& toOffset, const Matrix3f& toCameraMatrix, int toRows, int toCols, const Isometry3f& initialGuess) {
    PinholePointProjector* projector = _aligner->projector();
    _aligner->setReferenceSensorOffset(fromOffset);
    _aligner->setCurrentSensorOffset(toOffset);
    Isometry3f ig = initialGuess;
    ig(2,3) = 0.f;                                                               // :114
    _aligner->setInitialGuess(ig);
    projector->setCameraMatrix(toCameraMatrix);
    projector->setImageSize(toRows, toCols);
    projector->scale((float)(1. / _scale));                                      // :117-119
    _aligner->correspondenceFinder()->setImageSize(projector->imageRows(), projector->imageCols());
  }
  static void fill(MatcherResult& result, const pwn_hip_align_result& a, const pwn_hip_match_result& m) {
    for (int i = 0; i < 16; ++i) result.transform[i] = a.T[i];
    for (int i = 0; i < 36; ++i) result.informationMatrix[i] = (i % 7 == 0) ? 100.0 : 0.0;     // :147-148 HACK kept
    result.cloud_inliers = a.inliers;
    result.image_reprojectionDistance = m.image_reprojection_distance;
    result.image_nonZeros = m.image_non_zeros; result.image_outliers = m.image_outliers; result.image_inliers = m.image_inliers;
  }
  Context* _ctx; Aligner* _aligner; DepthImageConverter* _converter;
  Cloud* _pending = nullptr; const DepthImage* _pendingImage = nullptr; Matrix3f _pendingK; int _pendingR = 0, _pendingC = 0;      // makeCloudBegin
  float _frameInlierDepthThreshold = 50.f;   // .cpp:13
  int _scale = 2;                            // .cpp:12
};

// acceptance rule of PwnCloser::matchFrames (pwn_tracker/pwn_closer.cpp:56-58,138-141)
struct PwnCloserAcceptance {
  int frameMinNonZeroThreshold = 3000, frameMaxOutliersThreshold = 100, frameMinInliersThreshold = 1000;
  bool accept(const PwnMatcherBase::MatcherResult& r) const {
    return !(r.image_nonZeros < frameMinNonZeroThreshold || r.image_outliers > frameMaxOutliersThreshold || r.image_inliers < frameMinInliersThreshold);
  }
};

// pwn_tracker/pwn_tracker_cache.cpp:24-51 (+ boss_map_building cache.hpp): device-resident LRU of clouds keyed by frame; a miss re-runs the
// converter on the frame's stored depth image (PwnCache::loadFrame), so closure batches do not re-convert frames still resident in HBM.
// sceneReady: a miss makes its cloud with Stats and sensor-noise Gaussians, as the reference's converter always does -- what PwnMerger needs of
// its cache (the fused cloud copies both, pwn_merger.cpp:56-61); clouds handed to addFrame stay as they are.
class CloudCache {
 public:
  CloudCache(PwnMatcherBase* matcher, size_t capacity = 64, bool sceneReady = false) : _matcher(matcher), _capacity(capacity), _sceneReady(sceneReady) {}
  ~CloudCache() { for (auto& e : _lru) delete e.second; }
  // the cache takes ownership of `cloud` (may be nullptr: the cloud is then made on the first get)
  void addFrame(int key, const DepthImage& depthImage, const Matrix3f& cameraMatrix, const Isometry3f& sensorOffset, Cloud* cloud = nullptr) {
    _frames[key] = Frame{ depthImage, cameraMatrix, sensorOffset };
    if (cloud) insert(key, cloud);
  }
  Cloud* get(int key) {
    for (auto it = _lru.begin(); it != _lru.end(); ++it)
      if (it->first == key) { ++hits; _lru.splice(_lru.end(), _lru, it); return _lru.back().second; }
    ++misses;
    auto f = _frames.find(key);
    if (f == _frames.end()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "CloudCache: unknown frame");
    int r, c; Matrix3f K = f->second.cameraMatrix;
    Cloud* cloud = _matcher->makeCloud(r, c, K, f->second.sensorOffset, f->second.depth, _sceneReady, _sceneReady);      // pwn_tracker_cache.cpp:38-44
    insert(key, cloud);
    return cloud;
  }
  // `cloud` becomes the cloud of `key` (the cache takes ownership and deletes the one it held): PwnMerger::mergeNodeList, pwn_merger.cpp:56-61
  void put(int key, Cloud* cloud) { insert(key, cloud); }
  size_t resident() const { return _lru.size(); }  size_t capacity() const { return _capacity; }
  int hits = 0, misses = 0;
 private:
  struct Frame { DepthImage depth; Matrix3f cameraMatrix; Isometry3f sensorOffset; };
  void insert(int key, Cloud* cloud) {
    for (auto it = _lru.begin(); it != _lru.end(); ++it) if (it->first == key) { delete it->second; _lru.erase(it); break; }
    _lru.emplace_back(key, cloud);
    while (_lru.size() > _capacity) { delete _lru.front().second; _lru.pop_front(); }          // least recently used
  }
  PwnMatcherBase* _matcher; size_t _capacity; bool _sceneReady;
  std::list<std::pair<int, Cloud*> > _lru;       // front = least recently used
  std::map<int, Frame> _frames;
};

// pwn_tracker/pwn_tracker.{h,cpp}: sequential odometry with key-cloud switching (processFrame, .cpp:106-215).  The BOSS map bookkeeping of
// the reference (frames / relations handed to the map manager, :217-281) is reported through FrameResult instead.
class PwnTracker : public PwnMatcherBase {
 public:
  struct FrameResult { bool newFrame = false, aligned = false; int inliers = 0; float error = 0.f, inliersFraction = 0.f; Isometry3f T, globalT; };
  using PwnMatcherBase::PwnMatcherBase;
  ~PwnTracker() { delete _previousCloud; if (_currentCloud != _previousCloud) delete _currentCloud; }
  const Isometry3f& globalT() const { return _globalT; }
  int numKeyframes() const { return _numKeyframes; }
  float newFrameInliersFraction() const { return _newFrameInliersFraction; }  void setNewFrameInliersFraction(float v) { _newFrameInliersFraction = v; }
  void init() {                                                                  // pwn_tracker.cpp:38-49
    makeCloudDrop();
    delete _previousCloud; if (_currentCloud != _previousCloud) delete _currentCloud;
    _previousCloud = _currentCloud = nullptr;
    _globalT.setIdentity(); _previousCloudTransform.setIdentity(); _counter = 0; _numKeyframes = 0;
  }
  // Not in the reference: hand over the NEXT frame of a recorded / buffered stream (same sensor offset and camera matrix as the call that
  // will process it) before processFrame of the current one; its makeCloud (:115, independent of the alignments before it) then runs next
  // to that alignment, and processFrame of the same DepthImage object picks the cloud up.  Same results, bit for bit.
  void prefetch(const DepthImage& depthImage, const Isometry3f& sensorOffset, const Matrix3f& cameraMatrix) { makeCloudBegin(cameraMatrix, sensorOffset, depthImage); }
  // pwn_tracker.cpp:106-215; nextDepthImage (not in the reference): prefetch()ed as soon as this frame's cloud exists
  FrameResult processFrame(const DepthImage& depthImage, const Isometry3f& sensorOffset, const Matrix3f& cameraMatrix, const Isometry3f& initialGuess = Isometry3f::Identity(),
                           const DepthImage* nextDepthImage = nullptr) {
    FrameResult out;
    int r, c; Matrix3f scaledCameraMatrix = cameraMatrix;
    Cloud* currentCloud;
    if (makeCloudPending(depthImage)) currentCloud = makeCloudEnd(r, c, scaledCameraMatrix);
    else { makeCloudDrop(); currentCloud = makeCloud(r, c, scaledCameraMatrix, sensorOffset, depthImage); }     // :115
    if (nextDepthImage) prefetch(*nextDepthImage, sensorOffset, cameraMatrix);
    if (_currentCloud != _previousCloud) delete _currentCloud;                                                   // the last non-key cloud
    _currentCloud = currentCloud;
    if (_previousCloud) {
      _aligner->setCurrentSensorOffset(sensorOffset); _aligner->setCurrentCloud(currentCloud);
      _aligner->setReferenceSensorOffset(_previousCloudOffset); _aligner->setReferenceCloud(_previousCloud);
      _aligner->correspondenceFinder()->setImageSize(r, c);
      _aligner->projector()->setCameraMatrix(scaledCameraMatrix); _aligner->projector()->setImageSize(r, c);
      const Isometry3f guess = iso_mul(iso_mul(_previousCloudTransform.inverse(), _globalT), initialGuess);     // :132
      _aligner->setInitialGuess(guess);
      _aligner->align();                                                                                         // :136
      if (_aligner->inliers() > 0) _globalT = iso_mul(_previousCloudTransform, _aligner->T());                   // :147
      else _globalT = iso_mul(_globalT, guess);                                                                  // :150
      if (!(_counter % 50)) {                                                                                    // :154-159: R <- R - 0.5 R (R^T R - I)
        float R[9], Rt[9], E[9], hR[9], D[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { R[i + 3 * j] = _globalT(i,j); Rt[j + 3 * i] = _globalT(i,j); hR[i + 3 * j] = 0.5f * _globalT(i,j); }
        mul3(Rt, R, E); E[0] -= 1.f; E[4] -= 1.f; E[8] -= 1.f;
        mul3(hR, E, D);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) _globalT(i,j) = R[i + 3 * j] - D[i + 3 * j];
      }
      _globalT.forceLastRow();
      out.aligned = true; out.inliers = _aligner->inliers(); out.error = _aligner->error(); out.T = _aligner->T();
      out.inliersFraction = (float)_aligner->inliers() / (float)(r * c);
      if (out.inliersFraction < _newFrameInliersFraction) {                                                      // :164-185
        out.newFrame = true; ++_numKeyframes;
        delete _previousCloud;
        _previousCloud = currentCloud; _previousCloudTransform = _globalT;
      }
    } else {                                                                                                     // :194-200
      out.newFrame = true; ++_numKeyframes;
      _previousCloud = currentCloud; _previousCloudTransform = _globalT; _previousCloudOffset = sensorOffset;
    }
    ++_counter;
    out.globalT = _globalT;
    return out;
  }
  Cloud* previousCloud() const { return _previousCloud; }  Cloud* currentCloud() const { return _currentCloud; }
 private:
  static void mul3(const float* A, const float* B, float* C) {      // 3x3 float product, left-to-right inner products (no FMA: build without -ffast-math)
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { float s = A[i] * B[3 * j]; s = s + A[i + 3] * B[1 + 3 * j]; s = s + A[i + 6] * B[2 + 3 * j]; C[i + 3 * j] = s; }
  }
  Cloud* _previousCloud = nullptr; Cloud* _currentCloud = nullptr;
  Isometry3f _globalT, _previousCloudTransform, _previousCloudOffset;
  float _newFrameInliersFraction = 0.4f;     // pwn_tracker.cpp:36
  int _counter = 0, _numKeyframes = 0;
};

// S PwnTrackers that advance in lock-step (pwn_hip_tracker / pwn_hip_track_frames; not in the reference): processFrames runs processFrame
// (pwn_tracker.cpp:106-215) for frame 0 of every stream, then frame 1 of every stream, ... as one submission with one host wait; guess, pose chain,
// key-cloud decision and the switch of the reference cloud happen on the device.  Per stream the results, globalT and the key cloud are PwnTracker's,
// bit for bit.  The streams share camera matrix, image size, parameters and one sensor offset; frames are raw uint16 images (depth = rawScale * raw).
class PwnTrackerBatch : public PwnMatcherBase {
 public:
  using FrameResult = PwnTracker::FrameResult;
  struct StreamFrame { bool present = false; FrameResult result; int nPoints = 0; };
  PwnTrackerBatch(Context* ctx, Aligner* aligner, DepthImageConverter* converter, int streams, int framesPerCallMax, int rows, int cols, int scale = 2)
      : PwnMatcherBase(ctx, aligner, converter), _streams(streams), _framesPerCallMax(framesPerCallMax), _rows(rows), _cols(cols) {
    setScale(scale);
    ctx->check(pwn_hip_tracker_create(ctx->handle(), streams, framesPerCallMax, rows, cols, scale, &_h));
  }
  ~PwnTrackerBatch() { pwn_hip_tracker_destroy(_h); }      // before or after its context: a context that goes first leaves the handle valid for this call
  PwnTrackerBatch(const PwnTrackerBatch&) = delete;
  PwnTrackerBatch& operator=(const PwnTrackerBatch&) = delete;
  pwn_hip_tracker* handle() const { return _h; }
  int streams() const { return _streams; }  int framesPerCallMax() const { return _framesPerCallMax; }
  float newFrameInliersFraction() const { return _newFrameInliersFraction; }  void setNewFrameInliersFraction(float v) { _newFrameInliersFraction = v; }
  pwn_hip_tracker_state state(int s) const { pwn_hip_tracker_state st; _ctx->check(pwn_hip_tracker_get_state(_h, s, 1, &st)); return st; }
  void setState(int s, const pwn_hip_tracker_state& st) { _ctx->check(pwn_hip_tracker_set_state(_h, s, 1, &st)); }
  void init() { for (int s = 0; s < _streams; ++s) init(s); }                                         // pwn_tracker.cpp:38-49, every stream
  void init(int s) {
    pwn_hip_tracker_state st = pwn_hip_tracker_state();
    const Isometry3f I = Isometry3f::Identity();
    for (int q = 0; q < 16; ++q) st.globalT[q] = st.previous_cloud_transform[q] = st.sensor_offset[q] = I.data()[q];
    st.key_slot = -1;
    setState(s, st);
  }
  Isometry3f globalT(int s) const { const pwn_hip_tracker_state st = state(s); Isometry3f T; for (int q = 0; q < 16; ++q) T.data()[q] = st.globalT[q]; return T; }
  int numKeyframes(int s) const { return state(s).num_keyframes; }
  // the stream's key cloud after the last call: a borrowed handle (the next call may overwrite it), nullptr while the stream has none
  pwn_hip_cloud* keyCloud(int s) const { pwn_hip_cloud* c = nullptr; _ctx->check(pwn_hip_tracker_key_cloud(_h, s, &c)); return c; }
  // frames[f][s]: frame f of stream s, nullptr = the stream idles in that step; guesses (optional): [f][s] -> result[f][s]
  std::vector<std::vector<StreamFrame>> processFrames(const std::vector<std::vector<const RawDepthImage*>>& frames, const Isometry3f& sensorOffset, const Matrix3f& cameraMatrix,
                                                      const std::vector<std::vector<Isometry3f>>* guesses = nullptr, float rawScale = 0.001f, float maxDepthCov = 0.01f) {
    const int F = (int)frames.size(), S = _streams;
    std::vector<const uint16_t*> ptrs((size_t)F * S, nullptr);
    for (int f = 0; f < F; ++f) {
      if ((int)frames[f].size() != S) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "processFrames: one frame (or null) per stream in every step");
      for (int s = 0; s < S; ++s) {
        const RawDepthImage* d = frames[f][s];
        if (d && (d->rows != _rows || d->cols != _cols)) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "processFrames: a frame of another size than the tracker's");
        ptrs[(size_t)f * S + s] = d ? d->data.data() : nullptr;
      }
    }
    // the side effects of makeCloud (pwn_matcher_base.cpp:57-86) and of processFrame's aligner set-up (pwn_tracker.cpp:120-130) on the collaborators
    PinholePointProjector* projector = _converter->projector();
    const float invScale = 1.0f / _scale;
    Matrix3f scaled = cameraMatrix;
    for (int i = 0; i < 9; ++i) scaled.m[i] = scaled.m[i] * invScale;
    scaled(2,2) = 1.0f;
    const int r = _rows / _scale, c = _cols / _scale;
    projector->setCameraMatrix(scaled); projector->setImageSize(r, c); projector->setTransform(Isometry3f::Identity());
    const pwn_hip_converter_params cp = _converter->params(sensorOffset);
    _aligner->setCurrentSensorOffset(sensorOffset); _aligner->setReferenceSensorOffset(sensorOffset);
    _aligner->correspondenceFinder()->setImageSize(r, c);
    _aligner->projector()->setCameraMatrix(scaled); _aligner->projector()->setImageSize(r, c);
    const pwn_hip_aligner_params ap = _aligner->params();
    std::vector<float> g;
    if (guesses) {
      g.resize((size_t)F * S * 16);
      for (int f = 0; f < F; ++f) for (int s = 0; s < S; ++s) { Isometry3f T = (*guesses)[f][s]; T.forceLastRow(); for (int q = 0; q < 16; ++q) g[((size_t)f * S + s) * 16 + q] = T.data()[q]; }
    }
    std::vector<pwn_hip_track_result> res((size_t)F * S);
    _ctx->check(pwn_hip_track_frames(_ctx->handle(), _h, &cp, &ap, F, ptrs.data(), rawScale, maxDepthCov, guesses ? g.data() : nullptr, _newFrameInliersFraction, res.data()));
    std::vector<std::vector<StreamFrame>> out((size_t)F, std::vector<StreamFrame>((size_t)S));
    for (int f = 0; f < F; ++f)
      for (int s = 0; s < S; ++s) {
        if (!ptrs[(size_t)f * S + s]) continue;
        const pwn_hip_track_result& q = res[(size_t)f * S + s];
        StreamFrame& o = out[f][s];
        o.present = true; o.nPoints = q.n_points; ++numCalls;
        o.result.newFrame = q.new_frame != 0; o.result.aligned = q.aligned != 0; o.result.inliers = q.inliers; o.result.error = q.error;
        o.result.inliersFraction = q.inliers_fraction;
        for (int k = 0; k < 16; ++k) { o.result.T.data()[k] = q.T[k]; o.result.globalT.data()[k] = q.globalT[k]; }
      }
    return out;
  }
 private:
  pwn_hip_tracker* _h = nullptr;
  int _streams, _framesPerCallMax, _rows, _cols;
  float _newFrameInliersFraction = 0.4f;     // pwn_tracker.cpp:36
};

// ---- the merged closure (pwn_tracker2) --------------------------------------------------------------------------------------------------
// Eigen::Isometry3d as the closers compose it: row-major 4x4 doubles, products and inverse as plain loops in a fixed order (api.py runs the
// same loops: the two mirrors arrive at the same bits before the cast to float)
struct Isometry3d {
  double m[16];                                    // row-major
  Isometry3d() { for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0; }
  double& operator()(int r, int c) { return m[4 * r + c]; }
  double operator()(int r, int c) const { return m[4 * r + c]; }
  Isometry3d operator*(const Isometry3d& b) const {
    Isometry3d o;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) {
        double s = (*this)(i,0) * b(0,j); s = s + (*this)(i,1) * b(1,j); s = s + (*this)(i,2) * b(2,j);
        o(i,j) = (j == 3) ? s + (*this)(i,3) : s;
      }
    return o;
  }
  Isometry3d inverse() const {
    Isometry3d o;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) o(i,j) = (*this)(j,i);
      double s = (*this)(0,i) * (*this)(0,3); s = s + (*this)(1,i) * (*this)(1,3); s = s + (*this)(2,i) * (*this)(2,3);
      o(i,3) = -s;
    }
    return o;
  }
  Isometry3f toFloat() const { Isometry3f f; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) f(r,c) = (float)(*this)(r,c); return f; }      // convertScalar
  static Isometry3d fromColumnMajor(const double* a) { Isometry3d o; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) o(r,c) = a[r + 4 * c]; return o; }
};

// a depth image in device memory (pwn_hip_device_alloc): what the merged closure fuses into and converts from
class DeviceImage {
 public:
  DeviceImage(Context& ctx, int rows, int cols) : _ctx(&ctx), _rows(rows), _cols(cols) {
    ctx.check(pwn_hip_device_alloc(ctx.handle(), (void**)&_p, sizeof(float) * (size_t)(rows * cols > 0 ? rows * cols : 1)));
    try { setZero(); } catch (...) { pwn_hip_device_free(ctx.handle(), _p); throw; }
  }
  ~DeviceImage() { pwn_hip_device_free(_ctx->handle(), _p); }
  DeviceImage(const DeviceImage&) = delete;
  DeviceImage& operator=(const DeviceImage&) = delete;
  void setZero() { _ctx->check(pwn_hip_device_memset(_ctx->handle(), _p, 0, sizeof(float) * (size_t)_rows * _cols)); }      // on the device
  void download(DepthImage& out) const { out.create(_rows, _cols); if (!out.data.empty()) _ctx->check(pwn_hip_copy(_ctx->handle(), out.data.data(), _p, out.data.size() * sizeof(float))); }
  float* data() const { return _p; }
  int rows() const { return _rows; }  int cols() const { return _cols; }
 private:
  Context* _ctx; int _rows, _cols; float* _p = nullptr;
};

// pwn_tracker2/merger2.{h,cpp}: the depth-image half of the merger -- clear (:36-43), mergeDepthImage (:75-101), matchWithPartition (:185-203) --
// and the cloud-level one: clearCloud (:30-34) and merge (:106-183), the fusion of a node list's clouds into _cloud_tot with the weights
// _pesi_tot.  The fused image, the weight image (_image_pesi), the projected planes, _cloud_tot and _pesi_tot stay on the device.  Not
// mirrored: init and scale (:45-73), which nothing in the reference calls.
class Merger2 {
 public:
  Merger2(Context* ctx, DepthImageConverterIntegralImage* converter, PwnMatcherBase* matcher)
      : _r(converter->projector()->imageRows()), _c(converter->projector()->imageCols()), _ctx(ctx), _depthImageConverter(converter), _matcher(matcher),
        _image_pesi(*ctx, _r, _c), _bigCloud(*ctx, _r * _c > 0 ? _r * _c : 1), _currentBigCloud(*ctx, _r * _c > 0 ? _r * _c : 1) {}      // deserialize, :216-217
  DepthImageConverterIntegralImage* depthImageConverter() { return _depthImageConverter; }
  void clear() { _image_points_count = 0; _image_overlapping_points_count = 0; _image_pesi.setZero(); }        // :36-43
  // mergeDepthImage(out, image) (:75-101) for a run of images (host or device pointers, _r x _c floats each) in order; overlaps receives
  // _image_overlapping_points_count after each
  void mergeDepthImage(DeviceImage& out, const std::vector<const float*>& images) {
    overlaps.assign(images.size(), 0);
    _ctx->check(pwn_hip_merge_depth_images(_ctx->handle(), (int)images.size(), images.data(), _r, _c, out.data(), _image_pesi.data(), overlaps.data(), &_image_points_count));
    if (!overlaps.empty()) _image_overlapping_points_count = overlaps.back();
  }
  // PwnCloserWithMerger::mergeNode (pwn_closer_with_merger.cpp:210-224) for n clouds in one submission (pwn_hip_project_merge_batch)
  void projectMerge(DeviceImage& out, const std::vector<Cloud*>& clouds, const std::vector<Isometry3f>& transforms, float* planes = nullptr) {
    if (clouds.size() != transforms.size()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "projectMerge: list sizes differ");
    PinholePointProjector* pp = _depthImageConverter->projector();
    std::vector<pwn_hip_cloud*> h(clouds.size()); std::vector<float> tr(clouds.size() * 16);
    for (size_t i = 0; i < h.size(); ++i) { h[i] = clouds[i]->handle(); std::memcpy(&tr[16 * i], transforms[i].data(), 16 * sizeof(float)); }
    overlaps.assign(clouds.size(), 0);
    _ctx->check(pwn_hip_project_merge_batch(_ctx->handle(), pp->cameraMatrix().data(), (int)h.size(), h.data(), tr.data(), pp->minDistance(), pp->maxDistance(), _r, _c,
                                            out.data(), _image_pesi.data(), overlaps.data(), &_image_points_count, planes));
    if (!overlaps.empty()) _image_overlapping_points_count = overlaps.back();
  }
  // :185-203: both images converted by one pwn_hip_convert_batch of the two device frames, then matchClouds(from = the cloud of
  // currentPartitionImage, to = the cloud of partitionMerged, offset, offset, K, rows, cols, identity)
  void matchWithPartition(const DeviceImage& currentPartitionImage, const Isometry3f& offset, const DeviceImage& partitionMerged) {
    PinholePointProjector* pp = _depthImageConverter->projector();
    _depthImageConverter->computeBatch({ &_bigCloud, &_currentBigCloud }, { partitionMerged.data(), currentPartitionImage.data() }, _r, _c, offset);
    _matcher->aligner()->clearPriors();
    const Matrix3f K = pp->cameraMatrix();
    _matcher->matchClouds(_result, &_currentBigCloud, &_bigCloud, offset, offset, K, pp->imageRows(), pp->imageCols(), Isometry3f::Identity());
  }
  // ---- the cloud-level fusion
  void clearCloud() { _cloud_tot.reset(); _pesi_tot.reset(); }                                               // :30-34
  Cloud* cloudTot() const { return _cloud_tot.get(); }
  // _pesi_tot on the host: one weight per point of _cloud_tot
  std::vector<float> pesiTot() const {
    std::vector<float> w(_cloud_tot ? _cloud_tot->size() : 0);
    if (!w.empty()) _ctx->check(pwn_hip_copy(_ctx->handle(), w.data(), _pesi_tot->data(), w.size() * sizeof(float)));
    return w;
  }
  void merge(const Isometry3f& transform, const Isometry3f& offset, Cloud* cloud) { mergeBatch({ transform }, offset, { cloud }); }      // :106-183
  // merge for a list of clouds in order, one submission (pwn_hip_merge_clouds): cloud i comes under transforms[i] (its robot frame -> the frame
  // of _cloud_tot), `offset` is the sensor offset; appended / fused receive the pixels that took each action, per cloud
  void mergeBatch(const std::vector<Isometry3f>& transforms, const Isometry3f& offset, const std::vector<Cloud*>& clouds) {
    if (clouds.size() != transforms.size()) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "mergeBatch: list sizes differ");
    PinholePointProjector* pp = _depthImageConverter->projector();
    size_t points = _cloud_tot ? _cloud_tot->size() : 0;
    for (const Cloud* c : clouds) points += c->size();
    reserve(points);
    std::vector<pwn_hip_cloud*> h(clouds.size()); std::vector<float> tr(clouds.size() * 16);
    for (size_t i = 0; i < h.size(); ++i) { h[i] = clouds[i]->handle(); std::memcpy(&tr[16 * i], transforms[i].data(), 16 * sizeof(float)); }
    appended.assign(clouds.size(), 0); fused.assign(clouds.size(), 0);
    _ctx->check(pwn_hip_merge_clouds(_ctx->handle(), pp->cameraMatrix().data(), offset.data(), (int)h.size(), h.data(), tr.data(), pp->minDistance(), pp->maxDistance(),
                                     pp->imageRows(), pp->imageCols(), _cloud_tot->handle(), _pesi_tot->data(), appended.data(), fused.data()));
  }
  int _r, _c;
  int _image_points_count = 0, _image_overlapping_points_count = 0;
  std::vector<int> overlaps;
  std::vector<int> appended, fused;
  PwnMatcherBase::MatcherResult _result;
 private:
  // _cloud_tot / _pesi_tot with room for `points` points; what they hold is kept (Cloud::add under the identity is a copy)
  void reserve(size_t points) {
    if (_cloud_tot && _cloud_capacity >= points) return;
    const int cap = (int)(points > 0 ? points : 1);
    std::unique_ptr<Cloud> grown(new Cloud(*_ctx, cap));
    std::unique_ptr<DeviceImage> pesi(new DeviceImage(*_ctx, 1, cap));
    if (_cloud_tot && _cloud_tot->size() > 0) {
      grown->add(*_cloud_tot);
      _ctx->check(pwn_hip_copy(_ctx->handle(), pesi->data(), _pesi_tot->data(), _cloud_tot->size() * sizeof(float)));
    }
    _cloud_tot = std::move(grown); _pesi_tot = std::move(pesi); _cloud_capacity = (size_t)cap;
  }
  Context* _ctx; DepthImageConverterIntegralImage* _depthImageConverter; PwnMatcherBase* _matcher;
  DeviceImage _image_pesi;
  Cloud _bigCloud, _currentBigCloud;
  std::unique_ptr<Cloud> _cloud_tot; std::unique_ptr<DeviceImage> _pesi_tot; size_t _cloud_capacity = 0;
};

// what the merged closer needs of a SyncSensorDataNode: its transform, the sensor offset of its depth camera, the key of its frame in the cache
struct MapNode { int key = 0; Isometry3d transform; Isometry3d sensorOffset; };

// pwn_tracker2/pwn_closer_with_merger.{h,cpp}: one alignment per partition (see api.py, PwnCloserWithMerger, for the quirks kept).  The
// reference walks a std::set of pointers, whose order is not defined; here the order is the caller's vector.
class PwnCloserWithMerger {
 public:
  // the last four fields are ClosureInfo's (boss_map_building/map_closer.h): what MapCloser::validatePartitions counts and decides
  struct Relation {
    const MapNode* nodes[2]; Isometry3d transform; double informationMatrix[36]; PwnMatcherBase::MatcherResult result;
    int consensusTimeChecked = 0, consensusCumInlier = 0, consensusCumOutlierTimes = 0; bool accepted = false;
  };
  PwnCloserWithMerger(Context* ctx, Merger2* merger, CloudCache* cache) : _ctx(ctx), _merger(merger), _cache(cache) {}
  int frameMinNonZeroThreshold = 3000, frameMaxOutliersThreshold = 100, frameMinInliersThreshold = 1000;
  static int som(size_t size) { const int s = (int)(size / 8); return s == 0 ? 1 : s; }                     // :134-135
  bool rejects(const PwnMatcherBase::MatcherResult& r) const {                                            // :167-169
    return r.image_nonZeros < frameMinNonZeroThreshold / 2 || r.image_outliers > r.image_inliers / 8 || r.image_inliers < frameMinInliersThreshold / 2;
  }
  void mergeNodes(DeviceImage& out, const std::vector<const MapNode*>& others, const std::vector<Isometry3f>& transforms) {      // :210-224, n nodes
    // the cache deletes what it evicts: every cloud of the run has to stay resident until the call has used it
    if (_cache->capacity() < others.size()) throw Error(PWN_HIP_ERR_CAPACITY, "PwnCloserWithMerger: the cloud cache holds fewer clouds than one merge visits");
    std::vector<Cloud*> clouds;
    for (const MapNode* o : others) clouds.push_back(_cache->get(o->key));
    _merger->projectMerge(out, clouds, transforms);
  }
  void processCurrentPartition(const MapNode* current) {                                                  // :70-106
    _merger->clear();
    zeroed(_currentPartitionImage);
    mergeNodes(*_currentPartitionImage, { current }, { current->sensorOffset.toFloat() });
    _currentPartitionActive.push_back(current);
  }
  // :108-208; accepted: -1 = the match was not reached, 0 = rejected, 1 = accepted
  std::vector<Relation> processPartition(const std::vector<const MapNode*>& otherPartition, const MapNode* current) {
    std::vector<Relation> relations;
    accepted = -1;
    for (const MapNode* o : otherPartition) if (o == current) return relations;                           // :113-114
    if (_current != current) { _current = current; _currentPartitionActive.clear(); processCurrentPartition(current); }      // :123-127
    _merger->clear();
    zeroed(_otherPartitionImage);
    _nodeList.clear();
    const int s = som(otherPartition.size());
    std::vector<const MapNode*> visited; std::vector<Isometry3f> trs;
    for (size_t it = 0; it < otherPartition.size(); ++it) {                                               // :137-149
      if ((int)it % s != 0 || otherPartition[it] == current) continue;
      const MapNode* other = otherPartition[it];
      visited.push_back(other);
      trs.push_back((other->transform.inverse() * current->transform * other->sensorOffset).toFloat());
    }
    if (visited.empty()) return relations;
    mergeNodes(*_otherPartitionImage, visited, trs);
    for (size_t i = 0; i < visited.size(); ++i) if (_merger->overlaps[i] > 4000) _nodeList.push_back(visited[i]);      // :151-153
    if (_nodeList.empty()) return relations;                                                              // :160
    _merger->matchWithPartition(*_currentPartitionImage, visited.back()->sensorOffset.toFloat(), *_otherPartitionImage);      // :163-165
    const PwnMatcherBase::MatcherResult& result = _merger->_result;
    accepted = rejects(result) ? 0 : 1;
    if (!accepted) return relations;
    const Isometry3d current_ris_iT = current->transform * Isometry3d::fromColumnMajor(result.transform) * current->transform.inverse();      // :175
    for (const MapNode* nodo : _nodeList)                                                                 // :178-203
      for (const MapNode* nodo2 : _currentPartitionActive) {
        Relation r; r.nodes[0] = nodo2; r.nodes[1] = nodo; r.result = result;
        r.transform = nodo2->transform.inverse() * (current_ris_iT * nodo->transform);
        for (int i = 0; i < 36; ++i) r.informationMatrix[i] = (i % 7 == 0) ? (i < 21 ? 100.0 : 1000.0) : 0.0;      // :196-198
        relations.push_back(r);
      }
    return relations;
  }
  int accepted = -1;
  const std::vector<const MapNode*>& nodeList() const { return _nodeList; }
  const DeviceImage* otherPartitionImage() const { return _otherPartitionImage.get(); }
  const DeviceImage* currentPartitionImage() const { return _currentPartitionImage.get(); }
 private:
  // DepthImage::zeros(_r, _c) (:72, :129): allocated once, cleared on the device from then on
  void zeroed(std::unique_ptr<DeviceImage>& image) { if (image) image->setZero(); else image.reset(new DeviceImage(*_ctx, _merger->_r, _merger->_c)); }
  Context* _ctx; Merger2* _merger; CloudCache* _cache;
  const MapNode* _current = nullptr;
  std::vector<const MapNode*> _currentPartitionActive, _nodeList;
  std::unique_ptr<DeviceImage> _currentPartitionImage, _otherPartitionImage;
};

// The part of boss_map_building::MapCloser (map_closer.{h,cpp}) behind processPartition: the pool of relations and validatePartitions
// (:286-417), the consensus vote that commits or removes the relations joining two partitions (pwn_hip_validate_relations; without a context
// the host call: the same bits).  The reference walks std::sets of pointers, whose order is not defined; here the relations of a call come in
// the order they were added.  consistent (not in the reference, off by default): every transform is inverted before use -- the closers store
// nodes[0]^-1 * nodes[1] with nodes[0] in the current partition, and validateRelation's rule is a consistency check only for the inverse of
// that (docs/parity.md).
class MapCloser {
 public:
  typedef PwnCloserWithMerger::Relation Relation;
  explicit MapCloser(Context* ctx = nullptr, bool consistent_ = false) : consistent(consistent_), _ctx(ctx) { pwn_hip_default_consensus_params(&_params); }
  bool consistent;
  void setConsensusInlierTranslationalThreshold(float v) { _params.inlier_translational_threshold = v; }
  void setConsensusInlierRotationalThreshold(float v) { _params.inlier_rotational_threshold = v; }
  void setConsensusMinTimesCheckedThreshold(int v) { _params.min_times_checked = v; }
  const pwn_hip_consensus_params& params() const { return _params; }
  Relation* addRelation(const Relation& r) { _relations.push_back(r); return &_relations.back(); }      // :111-112
  const std::list<Relation>& relations() const { return _relations; }
  struct Validation { std::vector<Relation*> committed; std::vector<Relation> removed; };
  // :286-417.  records (optional, host or device): the records a closer call wrote for exactly the joining relations, in their order; the
  // transforms are then words [0:16] of them.  The removed relations leave the store (returned by value); "no inliers" (:362) throws Error.
  Validation validatePartitions(const std::vector<const MapNode*>& other, const std::vector<const MapNode*>& current, const float* records = nullptr,
                                int record_floats = 0) {
    auto in = [](const std::vector<const MapNode*>& s, const MapNode* n) { for (const MapNode* o : s) if (o == n) return true; return false; };
    std::vector<Relation*> rels; std::vector<int> flags;
    for (Relation& r : _relations)                                                                        // :289-306
      if ((in(other, r.nodes[0]) || in(other, r.nodes[1])) && (in(current, r.nodes[0]) || in(current, r.nodes[1]))) {
        rels.push_back(&r); flags.push_back(in(current, r.nodes[0]) ? 0 : 1);                             // :206-214
      }
    Validation v;
    const int n = (int)rels.size();
    if (n == 0) return v;
    std::vector<double> tc((size_t)16 * n), to((size_t)16 * n), tr((size_t)16 * n);
    std::vector<int> fl(n), cnt[3], dec(n, 0);
    for (auto& c : cnt) c.resize(n);
    for (int k = 0; k < n; ++k) {
      const Relation& r = *rels[k];
      for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) {
          tc[(size_t)16 * k + row + 4 * col] = r.nodes[flags[k]]->transform(row, col);
          to[(size_t)16 * k + row + 4 * col] = r.nodes[1 - flags[k]]->transform(row, col);
          tr[(size_t)16 * k + row + 4 * col] = r.transform(row, col);
        }
      fl[k] = flags[k] ^ (consistent ? 1 : 0);
      cnt[0][k] = r.consensusTimeChecked; cnt[1][k] = r.consensusCumInlier; cnt[2][k] = r.consensusCumOutlierTimes;
    }
    if (_ctx)
      _ctx->check(pwn_hip_validate_relations(_ctx->handle(), &_params, n, tc.data(), to.data(), records ? nullptr : tr.data(), records, record_floats, fl.data(),
                                             cnt[0].data(), cnt[1].data(), cnt[2].data(), dec.data(), nullptr, nullptr));
    else {
      if (records) throw Error(PWN_HIP_ERR_INVALID_ARGUMENT, "MapCloser: records need a context");
      int empty = -1;
      const int rc = pwn_hip_validate_relations_host(&_params, n, tc.data(), to.data(), tr.data(), fl.data(), cnt[0].data(), cnt[1].data(), cnt[2].data(),
                                                     dec.data(), nullptr, nullptr, &empty);
      if (rc) throw Error(rc, pwn_hip_last_error_string(nullptr));
    }
    for (int k = 0; k < n; ++k) {
      Relation& r = *rels[k];
      r.consensusTimeChecked = cnt[0][k]; r.consensusCumInlier = cnt[1][k]; r.consensusCumOutlierTimes = cnt[2][k];
      if (dec[k] == 1) { r.accepted = true; v.committed.push_back(&r); }
    }
    for (int k = 0; k < n; ++k)
      if (dec[k] == 2) {
        v.removed.push_back(*rels[k]);
        for (auto it = _relations.begin(); it != _relations.end(); ++it) if (&*it == rels[k]) { _relations.erase(it); break; }
      }
    return v;
  }
 private:
  Context* _ctx; pwn_hip_consensus_params _params; std::list<Relation> _relations;
};

// pwn_tracker2/pwn_merger.{h,cpp}: mergeNodeList (:28-62), what MapMerger::process (boss_map_building/map_merger.cpp:43-82) calls every
// listSize + 1 key nodes -- the cached clouds of the list fused, one after the other, into one local-map cloud in the frame of the first
// ("big") node, which then becomes that node's cloud in the cache.  The cache must be a CloudCache(matcher, capacity, true): only from scene-ready
// clouds does the fused cloud get real Stats and its Gaussians, and only then can it be handed to Merger::merge.
class PwnMerger {
 public:
  PwnMerger(Context* ctx, Merger2* merger, CloudCache* cache) : _ctx(ctx), _merger(merger), _cache(cache) {}
  // T = big.transform()^-1 * node.transform() in double (:36, :49), then convertScalar to float (:51)
  static Isometry3f nodeTransform(const MapNode& big, const MapNode& node) { return (big.transform.inverse() * node.transform).toFloat(); }
  // :28-62 -> the fused cloud (owned by the cache, where it replaces the big node's cloud).  The sensor offset is the big node's (:39-41).
  Cloud* mergeNodeList(const MapNode* big, const std::vector<const MapNode*>& nodes) {
    // the cache deletes what it evicts: every cloud of the list has to stay resident until the call has used it
    if (_cache->capacity() < nodes.size() + 1) throw Error(PWN_HIP_ERR_CAPACITY, "PwnMerger: the cloud cache holds fewer clouds than the node list visits");
    _merger->clearCloud();
    _cache->get(big->key);                                                                                // :34
    std::vector<Cloud*> clouds; std::vector<Isometry3f> trs;
    for (const MapNode* o : nodes) { clouds.push_back(_cache->get(o->key)); trs.push_back(nodeTransform(*big, *o)); }      // :46-51
    _merger->mergeBatch(trs, big->sensorOffset.toFloat(), clouds);
    const Cloud* tot = _merger->cloudTot();
    Cloud* fused = new Cloud(*_ctx, (int)(tot->size() > 0 ? tot->size() : 1));                            // :56-61: a cloud of the fused size
    try { fused->add(*tot); } catch (...) { delete fused; throw; }
    _cache->put(big->key, fused);
    return fused;
  }
 private:
  Context* _ctx; Merger2* _merger; CloudCache* _cache;
};

// pwn_tracker2/manifold_voronoi_extractor.h: the record ManifoldVoronoiExtractor::process puts on its stream -- the image (xSize rows by ySize
// columns of uint16: 30000 untouched, 65535 obstacle, else 10000 - 1000 z), its resolution and the key node it is centred on
struct ManifoldVoronoiData { std::vector<uint16_t> image; int rows = 0, cols = 0; float resolution = 0.2f; const MapNode* node = nullptr; };

// pwn_tracker2/manifold_voronoi_extractor.{h,cpp}: on every new key node the cached clouds of the last dequeSize key nodes, each moved into the new
// node's frame, splatted into one traversability image (process, :50-127) -- one pwn_hip_manifold_image call on clouds that stay on the device.
// The reference's deque holds cache handles, which pin the clouds; this cache owns its clouds and deletes what it evicts, so the deque holds the
// nodes and every call takes their clouds from the cache (which therefore has to hold dequeSize clouds).  Not mirrored: ManifoldVoronoi (distance
// map, Voronoi diagram and graph: pointer-keyed priority queues over a 100 x 100 image, read by the viewer only) and the BOSS serialisation.
class ManifoldVoronoiExtractor {
 public:
  ManifoldVoronoiExtractor(Context* ctx, CloudCache* cache) : _ctx(ctx), _cache(cache) {}
  void setQueueSize(size_t v) { _dequeSize = v; }   size_t dequeSize() const { return _dequeSize; }
  void setResolution(float v) { _resolution = v; }  float resolution() const { return _resolution; }
  int xSize = 100, ySize = 100;                                                                       // :41-45
  float normalThreshold = 0.64f;
  std::vector<int> inside;                           // points of each cloud of the last call that fell inside the grid
  // inT * cn->transform() in double (:66, :81), then convertScalar to float (:83-84)
  static Isometry3f nodeTransform(const MapNode& keyNode, const MapNode& cn) { return PwnMerger::nodeTransform(keyNode, cn); }
  ManifoldVoronoiData process(const MapNode* keyNode) {                                               // :50-127 for a NewKeyNodeMessage
    _deque.push_back(keyNode);                                                                        // :59-60
    while (_deque.size() > _dequeSize) _deque.erase(_deque.begin());                                  // :61-64
    if (_cache->capacity() < _deque.size()) throw Error(PWN_HIP_ERR_CAPACITY, "ManifoldVoronoiExtractor: the cloud cache holds fewer clouds than the deque");
    std::vector<pwn_hip_cloud*> h; std::vector<float> tr(_deque.size() * 16);
    for (const MapNode* o : _deque) _cache->get(o->key);                                              // misses are made first: a get may evict
    for (size_t i = 0; i < _deque.size(); ++i) {
      h.push_back(_cache->get(_deque[i]->key)->handle());
      const Isometry3f T = nodeTransform(*keyNode, *_deque[i]);
      std::memcpy(&tr[16 * i], T.data(), 16 * sizeof(float));
    }
    ManifoldVoronoiData out;
    out.rows = xSize; out.cols = ySize; out.resolution = _resolution; out.node = keyNode;             // :68-69, :124
    out.image.assign((size_t)(xSize > 0 && ySize > 0 ? xSize * ySize : 0), 0);
    inside.assign(h.size(), 0);
    _ctx->check(pwn_hip_manifold_image(_ctx->handle(), (int)h.size(), h.data(), tr.data(), _resolution, xSize, ySize, normalThreshold, 0, out.image.data(),
                                       inside.data()));
    return out;
  }
 private:
  Context* _ctx; CloudCache* _cache;
  float _resolution = 0.2f;
  size_t _dequeSize = 30;
  std::vector<const MapNode*> _deque;                // oldest first
};

}  // namespace pwn_hip
