// pwn_scene_kernels.h -- gfx950 kernels of the scene-maintenance stage that follows the registration path
// (SURVEY.md section 8(f) row 4): the per-point sensor-noise Gaussians of PinholePointProjector::unProject, Cloud::add,
// Merger::merge and VoxelCalculator::compute.  Reference: g2o_frontend/pwn_core/{pinholepointprojector.cpp:93-133, gaussian3.h,
// cloud.cpp:145-186, merger.cpp:15-119, voxelcalculator.cpp:15-73} and g2o_frontend/basemath/gaussian.h.
//
// Layout: a Gaussian is 24 floats per point, AoS (it is always read and written whole, by the thread that owns the point):
//   mean[3] cov[9] infoVec[3] info[9], 3x3 blocks column-major like Eigen's; a separate int per point holds the reference's two
//   lazy-evaluation flags (1 = moments valid, 2 = information form valid; gaussian.h:89-94).  Both forms are kept because the
//   reference caches both and fp32 inverse(inverse(A)) != A.
#pragma once

#include "pwn_kernels.h"

namespace pwnhip {

constexpr int kGaussFloats = 24;
struct GaussD { float mean[3]; float cov[9]; float infoVec[3]; float info[9]; };
constexpr int kGaussMoments = 1, kGaussInfo = 2;

struct SceneBuffers {        // optional per-cloud arrays of the scene stage
  GaussD* G;                 // [capacity]
  int* Gf;                   // [capacity] flags
};

__device__ __forceinline__ Mat3 mat3_of(const float* m) { Mat3 r; for (int k = 0; k < 9; ++k) r.m[k] = m[k]; return r; }
__device__ __forceinline__ Mat3 mat3_transpose(const Mat3& a) { Mat3 r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r(i,j) = a(j,i); return r; }
// Gaussian::_updateInfo / _updateMoments (basemath/gaussian.h:73-87)
__device__ __forceinline__ void gauss_update_info(GaussD& g, int& flags) {
  if (flags & kGaussInfo) return;
  const Mat3 I = mat3_inverse(mat3_of(g.cov));
  for (int k = 0; k < 9; ++k) g.info[k] = I.m[k];
  const Vec3 mu = { g.mean[0], g.mean[1], g.mean[2] };
  const Vec3 v = mat3_mul_vec(I, mu);
  g.infoVec[0] = v.x; g.infoVec[1] = v.y; g.infoVec[2] = v.z;
  flags |= kGaussInfo;
}
__device__ __forceinline__ void gauss_update_moments(GaussD& g, int& flags) {
  if (flags & kGaussMoments) return;
  const Mat3 C = mat3_inverse(mat3_of(g.info));
  for (int k = 0; k < 9; ++k) g.cov[k] = C.m[k];
  const Vec3 iv = { g.infoVec[0], g.infoVec[1], g.infoVec[2] };
  const Vec3 v = mat3_mul_vec(C, iv);
  g.mean[0] = v.x; g.mean[1] = v.y; g.mean[2] = v.z;
  flags |= kGaussMoments;
}
// Gaussian3fVector::transformInPlace (gaussian3.h:65-73): Gaussian3f(R*mean + t, R*cov*R^T, false)
__device__ __forceinline__ void gauss_transform(GaussD& g, int& flags, const Mat4& m) {
  gauss_update_moments(g, flags);
  const Mat3 R = iso_linear(m);
  const Vec3 mu = { g.mean[0], g.mean[1], g.mean[2] };
  Vec3 v = mat3_mul_vec(R, mu);
  g.mean[0] = v.x + m(0,3); g.mean[1] = v.y + m(1,3); g.mean[2] = v.z + m(2,3);
  const Mat3 C = mat3_mul(mat3_mul(R, mat3_of(g.cov)), mat3_transpose(R));
  for (int k = 0; k < 9; ++k) { g.cov[k] = C.m[k]; g.info[k] = 0.f; }
  g.infoVec[0] = g.infoVec[1] = g.infoVec[2] = 0.f;
  flags = kGaussMoments;
}

// ------------------------------------------------------------------------------------------------------------------
// The sensor-noise Gaussian of one valid pixel (c, r) of depth d (pinholepointprojector.cpp:104-123), moved by the sensor offset as
// Cloud::transformInPlace moves it (cloud.cpp:180).  The one definition of that arithmetic: k_gaussians and k_gaussians_batch both call it.
__device__ __forceinline__ void gauss_of_pixel(const ConvertParams& cp, const Mat3& iK, float fB, float alpha, int c, int r, float d, GaussD& g, int& flags) {
  const Vec3 mean = unproject_pixel(cp.iKRt, c, r, d);
  g.mean[0] = mean.x; g.mean[1] = mean.y; g.mean[2] = mean.z;
  const float z = d;
  const float zVariation = (alpha * z * z) / (fB + z * alpha);
  Mat3 J;
  J(0,0) = z;   J(0,1) = 0.f; J(0,2) = (float)c;
  J(1,0) = 0.f; J(1,1) = z;   J(1,2) = (float)r;
  J(2,0) = 0.f; J(2,1) = 0.f; J(2,2) = 1.f;
  J = mat3_mul(iK, J);
  const float dg[3] = { 3.0f, 3.0f, zVariation };
  Mat3 JD;
  for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) JD(i,k) = J(i,k) * dg[k];
  const Mat3 C = mat3_mul(JD, mat3_transpose(J));
  for (int k = 0; k < 9; ++k) { g.cov[k] = C.m[k]; g.info[k] = 0.f; }
  g.infoVec[0] = g.infoVec[1] = g.infoVec[2] = 0.f;
  flags = kGaussMoments;
  if (cp.hasOffset) gauss_transform(g, flags, cp.offset);
}

// The Gaussian half of PinholePointProjector::unProject(points, gaussians, index, depth) (pinholepointprojector.cpp:104-123)
// followed by Cloud::transformInPlace(sensorOffset) on the Gaussians (cloud.cpp:180).  Same ordered compaction as k_unproject
// (the point index is the row-major rank of the valid pixel); f.rowoff holds the exclusive row offsets (k_row_count + k_row_offsets).
// grid = (rows, 1), block = 256.
__global__ void __launch_bounds__(256) k_gaussians(const FrameDesc* __restrict__ frames, ConvertParams cp, Mat3 iK, float fB, float alpha,
                                                   SceneBuffers sb) {
  const FrameDesc& f = frames[blockIdx.y];
  const int r = blockIdx.x;
  __shared__ int wcount[4];
  int base = f.rowoff[r];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  for (int c0 = 0; c0 < cp.cols; c0 += 256) {
    const int c = c0 + threadIdx.x;
    const bool in = c < cp.cols;
    const float d = in ? frame_depth(f, (size_t)r * cp.cols + c) : 0.f;
    const bool valid = in && depth_in_range(d, cp.minD, cp.maxD);
    int tot;
    const int idx = row_compact(valid, wcount, wave, lane, base, tot);
    if (valid) {
      if (idx < f.cloud.capacity) {
        GaussD g;
        int flags;
        gauss_of_pixel(cp, iK, fB, alpha, c, r, d, g, flags);
        sb.G[idx] = g;
        sb.Gf[idx] = flags;
      }
    }
    base += tot;
    __syncthreads();
  }
}

// The same records for the frames of a converter sub-batch, queued behind their front end on its stream: the front end has written the cloud's index
// image (FrameDesc::index: the point of a valid pixel, -1 elsewhere), so the point index is read, not recounted; the depth is the one the front end
// read (frame_depth: a float frame, a raw frame with its scale, the slot's down-sampled frame).  sbs[frame]: the Gaussian arrays of the frame's
// cloud; records at or beyond the cloud's capacity are not written.  One thread per pixel; grid = (ceil(rows * cols / 256), frames), block = 256.
//
// STAGED = false: every lane stores its own 96-byte record and its flag word (six 16-byte stores at a 96-byte stride across the wave).
// STAGED = true: the valid pixels of a block are consecutive points (the index is the row-major rank), so the block's records are one contiguous
// run of 24 * count floats: they are staged in LDS (25 floats apart: an odd stride keeps the lanes' writes on different banks) and leave as
// consecutive dwords, lane after lane.  Same records, same bits.
constexpr int kGaussStage = kGaussFloats + 1;
constexpr int kGaussStagedDefault = 1;      // the form the library uses (DESIGN.md section 5 has both forms' times)
template <bool STAGED>
__global__ void __launch_bounds__(256) k_gaussians_batch(const FrameDesc* __restrict__ frames, const SceneBuffers* __restrict__ sbs, ConvertParams cp,
                                                         Mat3 iK, float fB, float alpha) {
  const FrameDesc& f = frames[blockIdx.y];
  const SceneBuffers sb = sbs[blockIdx.y];
  const unsigned N = (unsigned)cp.rows * (unsigned)cp.cols;
  const unsigned pix = blockIdx.x * 256u + threadIdx.x;
  const int cap = f.cloud.capacity;
  int idx = -1;
  if (pix < N) idx = f.index[pix];
  const bool valid = idx >= 0 && idx < cap;
  GaussD g;
  int flags = 0;
  if (valid) {
    const int r = (int)(pix / (unsigned)cp.cols), c = (int)(pix - (unsigned)r * (unsigned)cp.cols);
    gauss_of_pixel(cp, iK, fB, alpha, c, r, frame_depth(f, pix), g, flags);
  }
  if (!STAGED) {
    if (valid) { sb.G[idx] = g; sb.Gf[idx] = flags; }
    return;
  }
  __shared__ float stage[256 * kGaussStage];
  __shared__ int first, count;
  if (threadIdx.x == 0) { first = 0x7fffffff; count = 0; }
  __syncthreads();
  if (valid) { atomicMin(&first, idx); atomicAdd(&count, 1); }
  __syncthreads();
  const int i0 = first, cnt = count;
  if (valid) {
    float* s = stage + (idx - i0) * kGaussStage;      // idx - i0 < cnt <= 256: the block's valid pixels are consecutive points
    for (int k = 0; k < 3; ++k) { s[k] = g.mean[k]; s[12 + k] = g.infoVec[k]; }
    for (int k = 0; k < 9; ++k) { s[3 + k] = g.cov[k]; s[15 + k] = g.info[k]; }
    sb.Gf[idx] = flags;                               // one dword per lane, consecutive already
  }
  __syncthreads();
  float* out = (float*)(sb.G + i0);
  for (int j = threadIdx.x; j < cnt * kGaussFloats; j += 256) out[j] = stage[(j / kGaussFloats) * kGaussStage + j % kGaussFloats];
}

// ------------------------------------------------------------------------------------------------------------------
// The scene record.  Cloud::add and Merger::merge run on sizes that the device holds (CloudDev::count) and on a transform and a view that they read
// from this record, which lies in device memory in front of their kernels: written by the host (pwn_hip_merge) or by k_scene_pose
// (the mapping step, pwn_aligner.cpp:166-209; pwn_hip_scene_step: what the host does between pwn_hip_align, pwn_hip_cloud_add and pwn_hip_merge).
// The grids are sized by the host's upper bound of the sizes; every kernel reads the sizes itself and clamps them to the capacities.  A skipped step
// (the converter timed out, or a projection of the alignment gave up on a pixel: the host repeats or reports it) touches nothing of the scene.
// Every dependency is a kernel boundary.
struct SceneStepRecord {
  Mat4 sceneT;             // scene_T' = scene_T * Aligner::T(), last row forced: the transform of Cloud::add (pwn_aligner.cpp:199, :205)
  Mat4 mergeKRt;           // the projector matrix of scene_T' * sensor offset: the view of Merger::merge (pwn_aligner.cpp:206-208)
  int identity;            // Cloud::add's test of scene_T' (cloud.cpp:176)
  int skipped;
  int sizeAdd, sizeMerge;  // the cloud's size after Cloud::add and after Merger::merge (a skipped step: the size it had)
  int gaussLen;            // the length of the cloud's Gaussian vector, which Merger::merge does not resize (merger.cpp:108-112)
};
__device__ __forceinline__ int clamped_count(const int* count, int capacity) { return max(0, min(*count, capacity)); }
// one thread.  state: the pair's final state (PairState::T is the aligner's result); convFault: the converter's time-out word (device memory);
// alignFault: the projections' give-up word (page-locked host memory).  The record is written twice: for the kernels behind, and for the host.
__global__ void k_scene_pose(const PairState* __restrict__ state, Mat4 sceneT, Mat3 K, Mat4 offset, const int* __restrict__ convFault,
                             const int* alignFault, const int* __restrict__ sceneCount, int sceneCapacity, SceneStepRecord* __restrict__ rec,
                             SceneStepRecord* host) {
  SceneStepRecord r;
  r.sceneT = iso_mul(sceneT, state->T);
  set_last_row(r.sceneT);
  Mat4 iKRt; Mat3 iK;
  projector_matrices(K, iso_mul(r.sceneT, offset), r.mergeKRt, iKRt, iK);
  const Mat4 I = mat4_identity();
  r.identity = 1;
  for (int q = 0; q < 16; ++q) if (r.sceneT.m[q] != I.m[q]) r.identity = 0;
  r.skipped = (*convFault != 0 || *(const volatile int*)alignFault != 0) ? 1 : 0;
  r.sizeAdd = r.sizeMerge = r.gaussLen = clamped_count(sceneCount, sceneCapacity);
  *rec = r;
  *host = r;
}

// ------------------------------------------------------------------------------------------------------------------
// Cloud::add (cloud.cpp:145-171): dst[k + i] = transformInPlace(T)(src[i]).  The scene cloud keeps per-point normal information
// matrices (9 planes): clouds appended with different transforms have different class matrices.
__device__ __forceinline__ void omega_transform(const Mat4& m, float* om /* row-major 3x3, in place */) {
  float t1[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) t1[3 * a + b] = dot3seq(m(a,0), om[0 + b], m(a,1), om[3 + b], m(a,2), om[6 + b]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) om[3 * a + b] = dot3seq(t1[3 * a], m(b,0), t1[3 * a + 1], m(b,1), t1[3 * a + 2], m(b,2));
}
// StatsVector::transformInPlace on one Stats record (CloudDev::St: the 3x3 block column-major at 0..8, the translation at 12..14): m * S (stats.h:125-131)
__device__ __forceinline__ void stats_transform(const Mat4& m, float* st) {
  Mat4 S = mat4_identity();
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) S(a,b) = st[a + 3 * b];
  S(0,3) = st[12]; S(1,3) = st[13]; S(2,3) = st[14];
  const Mat4 R = mat4_mul(m, S);
  for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) st[a + 3 * b] = R(a,b);
  st[12] = R(0,3); st[13] = R(1,3); st[14] = R(2,3);
}
// the default Gaussian, all zero and neither form valid (gaussian.h:16-21), as record o
__device__ __forceinline__ void gauss_store_default(const SceneBuffers& sb, int o) {
  GaussD g;
  for (int k = 0; k < 3; ++k) g.mean[k] = g.infoVec[k] = 0.f;
  for (int k = 0; k < 9; ++k) g.cov[k] = g.info[k] = 0.f;
  sb.G[o] = g; sb.Gf[o] = 0;
}
// Point i of src, transformed by m (not at all when `identity`), stored as point o of dst: every per-point array Cloud::add carries.  The one
// definition of that arithmetic: k_cloud_append / k_scene_append (Cloud::add) and k_merge_clouds_append (Merger2::merge's push_backs) both call it.
__device__ __forceinline__ void cloud_append_point(const CloudDev& dst, const SceneBuffers& dsb, const CloudDev& src, const SceneBuffers& ssb, int i, int o,
                                                   int ngauss, const Mat4& m, int identity) {
  float4 P, Nm;                    // old-format view: (x, y, z, curvature), (normal, class word)
  cloud_get(src, i, P, Nm);
  float omP[9], omN[9];
  const int cls = __float_as_int(Nm.w) & kClsMask;
#pragma unroll
  for (int q = 0; q < 9; ++q) omP[q] = src.Om[omp_at(src.capacity, i, q, src.omSym)];
  if (src.OmN) {
#pragma unroll
    for (int q = 0; q < 9; ++q) omN[q] = src.OmN[om_at(src.capacity, i, q)];
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) omN[q] = (cls == 1) ? src.omN[0][q] : ((cls == 2) ? src.omN[1][q] : 0.f);
  }
  if (!identity) {       // Cloud::transformInPlace (cloud.cpp:173-186)
    const float px = dot4seq(m(0,0), P.x, m(0,1), P.y, m(0,2), P.z, m(0,3), 1.0f);
    const float py = dot4seq(m(1,0), P.x, m(1,1), P.y, m(1,2), P.z, m(1,3), 1.0f);
    const float pz = dot4seq(m(2,0), P.x, m(2,1), P.y, m(2,2), P.z, m(2,3), 1.0f);
    P.x = px; P.y = py; P.z = pz;
    const float tx = dot4seq(m(0,0), Nm.x, m(0,1), Nm.y, m(0,2), Nm.z, m(0,3), 0.0f);
    const float ty = dot4seq(m(1,0), Nm.x, m(1,1), Nm.y, m(1,2), Nm.z, m(1,3), 0.0f);
    const float tz = dot4seq(m(2,0), Nm.x, m(2,1), Nm.y, m(2,2), Nm.z, m(2,3), 0.0f);
    Nm.x = tx; Nm.y = ty; Nm.z = tz;
    omega_transform(m, omP);
    omega_transform(m, omN);
  }
  cloud_put(dst, o, P, Nm);
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    if (!(dst.omSym && om_is_lower(q))) dst.Om[omp_at(dst.capacity, o, q, dst.omSym)] = omP[q];
    dst.OmN[om_at(dst.capacity, o, q)] = omN[q];
  }
  if (dst.St) {
    float st[16];
    if (src.St) {
#pragma unroll
      for (int q = 0; q < 16; ++q) st[q] = src.St[(size_t)i * 16 + q];
    } else {          // default Stats(): identity, eigenvalues 0, n 0 (stats.h:21-27)
#pragma unroll
      for (int q = 0; q < 16; ++q) st[q] = 0.f;
      st[0] = st[4] = st[8] = 1.f;
    }
    if (!identity) stats_transform(m, st);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst.St[(size_t)o * 16 + q] = st[q];
  }
  if (dsb.G && ssb.G && i < ngauss) {
    GaussD g = ssb.G[i]; int flags = ssb.Gf[i];
    if (!identity) gauss_transform(g, flags, m);
    dsb.G[o] = g; dsb.Gf[o] = flags;
  }
}
// sizes, Gaussian count and transform from the host (pwn_hip_cloud_add; the record form costs that call a copy and a launch more: measured 0.056 ms
// against 0.051 ms per VGA frame, profiles/one_merge_chain_ab.txt).  grid = ceil(n / 256), block = 256
__global__ void __launch_bounds__(256) k_cloud_append(CloudDev dst, SceneBuffers dsb, CloudDev src, SceneBuffers ssb, int k, int n, int ngauss,
                                                      Mat4 m, int identity) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || k + i >= dst.capacity) return;
  cloud_append_point(dst, dsb, src, ssb, i, k + i, ngauss, m, identity);
}
// the same at sizes the device holds: src appended at *dst.count under the record's transform.  grid = ceil(pixels of the frame / 256), block = 256
__global__ void __launch_bounds__(256) k_scene_append(CloudDev dst, SceneBuffers dsb, CloudDev src, SceneBuffers ssb, const SceneStepRecord* __restrict__ rec) {
  if (*as_global(&rec->skipped)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int m = clamped_count(src.count, src.capacity), k = clamped_count(dst.count, dst.capacity);
  if (i >= m || i >= dst.capacity - k) return;
  const Mat4 T = uniform_iso_global(as_global((const float*)rec->sceneT.m));
  cloud_append_point(dst, dsb, src, ssb, i, k + i, m, T, *as_global(&rec->identity));
}
// one thread: the destination's size word follows (the append read it), and with it the length of its Gaussian vector
__global__ void k_scene_grow(CloudDev dst, CloudDev src, SceneStepRecord* __restrict__ rec, SceneStepRecord* host) {
  if (rec->skipped) return;
  const int k = clamped_count(dst.count, dst.capacity);
  const int n = k + min(clamped_count(src.count, src.capacity), dst.capacity - k);
  *dst.count = n;
  rec->sizeAdd = rec->gaussLen = n; host->sizeAdd = host->gaussLen = n;
}
// Cloud::transformInPlace on the Gaussians and Stats of an existing cloud (k_cloud_transform handles the other arrays)
__global__ void __launch_bounds__(256) k_scene_transform(CloudDev cl, SceneBuffers sb, int n, int ngauss, Mat4 m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < ngauss && sb.G) { GaussD g = sb.G[i]; int flags = sb.Gf[i]; gauss_transform(g, flags, m); sb.G[i] = g; sb.Gf[i] = flags; }
  if (i < n && cl.St) stats_transform(m, cl.St + (size_t)i * 16);
}
// class-coded normal information -> 9 explicit planes (a cloud that becomes a scene)
__global__ void __launch_bounds__(256) k_expand_omega_n(CloudDev cl, float* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 nc = cl.Nc[i];
  const int cls = normal_class(nc.x, nc.y, nc.z, nc.w, cl.clsThr);
#pragma unroll
  for (int q = 0; q < 9; ++q) out[om_at(cl.capacity, i, q)] = (cls == 1) ? cl.omN[0][q] : ((cls == 2) ? cl.omN[1][q] : 0.f);
}

// ------------------------------------------------------------------------------------------------------------------
// Merger::merge (merger.cpp:15-119) on the size the device holds (*cl.count), with the view of the scene record.
// 1. k_scene_merge_project: z-buffer of the whole cloud (index + depth image of merger.cpp:21-23).
// 2. k_scene_merge_classify: the per-point tests of merger.cpp:42-76 -> _collapsedIndices; a point that merges into target t is pushed on
//    t's list (head/next, order of arrival).
// 3. k_scene_merge_accumulate: one thread per target walks its list in ASCENDING point index -- the order in which the reference's
//    sequential loop calls addInformation, so the fp32 sums carry the same bits -- then mean() moves the point (merger.cpp:91-93).
// 4. k_scene_merge_keep_flags, exclusive scan of the keep flags over the host's bound + k_scene_merge_compact: stable compaction of every
//    per-point array (merger.cpp:88-104); k_scene_gauss_tail: what the Gaussian vector, never resized, keeps behind the survivors
//    (merger.cpp:108-112); k_scene_merge_count: the new size.
// grids = ceil(bound / 256), block = 256.
// The merger's thresholds and view as the classification reads them (merger.cpp:6-8, :20-23)
struct MergeView { float minD, maxD, maxPointDepth; int rows, cols; float distanceThreshold, normalThreshold; };
// Point i of the merge: step 2 for one point
__device__ __forceinline__ void merge_classify_point(const CloudDev& cl, int i, const Mat4& KRt, float minD, float maxD, float maxPointDepth, int rows, int cols,
                                                     const unsigned long long* __restrict__ z, unsigned tag, float distanceThreshold, float normalThreshold,
                                                     int* __restrict__ collapsed, int* __restrict__ head, int* __restrict__ next) {
  const float4 p = load_xyz(cl.P3, i);
  int res = -1;
  // PinholePointProjector::_project: x, y stay -1 when the depth is out of the projector's range
  const Vec3 ip = project_plane(KRt, p.x, p.y, p.z);
  const float d = ip.z;
  const bool ok = depth_in_range(d, minD, maxD);
  float fx = -1.f, fy = -1.f;
  if (ok) round_to_pixel(ip, fx, fy);
  // merger.cpp:49-54
  if (ok && !(d < 0 || d > maxPointDepth) && in_image(fx, fy, rows, cols)) {
    const int x = (int)fx, y = (int)fy;
    const unsigned long long key = z[(size_t)y * cols + x];
    const int targetIndex = zkey_index(key, tag);
    if (targetIndex >= 0) {
      if (targetIndex == i) res = i;
      else {
        const float targetZ = zkey_depth(key, tag);
        const float4 cn = cl.Nc[i], tn = cl.Nc[targetIndex];
        if (fabsf(d - targetZ) < distanceThreshold && dot4seq(cn.x, tn.x, cn.y, tn.y, cn.z, tn.z, 0.f, 0.f) > normalThreshold) {
          res = targetIndex;
          next[i] = atomicExch(&head[targetIndex], i);
        }
      }
    }
  }
  collapsed[i] = res;
}
__global__ void __launch_bounds__(256) k_scene_merge_project(CloudDev cl, const SceneStepRecord* __restrict__ rec, float minD, float maxD, int rows, int cols,
                                                             unsigned long long* z, unsigned tag) {
  if (*as_global(&rec->skipped)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= clamped_count(cl.count, cl.capacity)) return;
  const Mat4 KRt = uniform_iso_global(as_global((const float*)rec->mergeKRt.m));
  project_point(KRt, minD, maxD, rows, cols, load_xyz(cl.P3, i), i, z, tag);
}
__global__ void __launch_bounds__(256) k_scene_merge_classify(CloudDev cl, const SceneStepRecord* __restrict__ rec, MergeView v,
                                                              const unsigned long long* __restrict__ z, unsigned tag, int* __restrict__ collapsed,
                                                              int* __restrict__ head, int* __restrict__ next) {
  if (*as_global(&rec->skipped)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= clamped_count(cl.count, cl.capacity)) return;
  const Mat4 KRt = uniform_iso_global(as_global((const float*)rec->mergeKRt.m));
  merge_classify_point(cl, i, KRt, v.minD, v.maxD, v.maxPointDepth, v.rows, v.cols, z, tag, v.distanceThreshold, v.normalThreshold, collapsed, head, next);
}
// target t (collapsed[t] == t) takes the points on its list
__device__ __forceinline__ void merge_accumulate_target(const CloudDev& cl, const SceneBuffers& sb, int t, const int* __restrict__ head, const int* __restrict__ next) {
  GaussD g = sb.G[t]; int flags = sb.Gf[t];
  const int h = head[t];
  if (h >= 0) {
    int last = -1;
    for (;;) {                                    // next merged point in ascending index order
      int best = 0x7fffffff;
      for (int j = h; j >= 0; j = next[j]) if (j > last && j < best) best = j;
      if (best == 0x7fffffff) break;
      GaussD o = sb.G[best]; int of = sb.Gf[best];
      gauss_update_info(g, flags);                // Gaussian::addInformation (gaussian.h:47-53)
      if (!(of & kGaussInfo)) {                  // g.informationMatrix() caches the information form in the merged point's own Gaussian;
        gauss_update_info(o, of);                // it survives in the tail of the (never resized) Gaussian vector
        sb.G[best] = o; sb.Gf[best] = of;
      }
      for (int k = 0; k < 9; ++k) g.info[k] = g.info[k] + o.info[k];
      for (int k = 0; k < 3; ++k) g.infoVec[k] = g.infoVec[k] + o.infoVec[k];
      flags &= ~kGaussMoments;
      last = best;
    }
  }
  gauss_update_moments(g, flags);                 // gaussians()[i].mean()  (merger.cpp:92)
  sb.G[t] = g; sb.Gf[t] = flags;
  store_xyz(cl.P3, t, g.mean[0], g.mean[1], g.mean[2]);
}
__global__ void __launch_bounds__(256) k_scene_merge_accumulate(CloudDev cl, SceneBuffers sb, const SceneStepRecord* __restrict__ rec,
                                                                const int* __restrict__ collapsed, const int* __restrict__ head, const int* __restrict__ next) {
  if (*as_global(&rec->skipped)) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= clamped_count(cl.count, cl.capacity) || collapsed[t] != t) return;
  merge_accumulate_target(cl, sb, t, head, next);
}
// the keep flags of the n points, and 0 for every index of [n, bound): the scan runs over the bound.  collapsed gets -1 there (what the host copies back)
__global__ void __launch_bounds__(256) k_scene_merge_keep_flags(CloudDev cl, const SceneStepRecord* __restrict__ rec, int* __restrict__ collapsed, int bound,
                                                                int* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= bound) return;
  const int n = *as_global(&rec->skipped) ? 0 : clamped_count(cl.count, cl.capacity);
  if (i < n) { const int c = collapsed[i]; keep[i] = (c < 0 || c == i) ? 1 : 0; }
  else { keep[i] = 0; collapsed[i] = -1; }
}
// Record i of one array set becomes record o of another, unchanged: the optional arrays where both sets have them, the Gaussian when `gauss`.
// What the compaction of a merge and the gather of a voxelization do to a point.
__device__ __forceinline__ void cloud_move_point(const CloudDev& src, const SceneBuffers& ssb, int i, const CloudDev& dst, const SceneBuffers& dsb, int o,
                                                 bool gauss) {
  { const float4 p = load_xyz(src.P3, i); store_xyz(dst.P3, o, p.x, p.y, p.z); dst.Nc[o] = src.Nc[i]; }
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    if (!(dst.omSym && om_is_lower(q))) dst.Om[omp_at(dst.capacity, o, q, dst.omSym)] = src.Om[omp_at(src.capacity, i, q, src.omSym)];
    if (src.OmN && dst.OmN) dst.OmN[om_at(dst.capacity, o, q)] = src.OmN[om_at(src.capacity, i, q)];
  }
  if (src.St && dst.St) {
#pragma unroll
    for (int q = 0; q < 16; ++q) dst.St[(size_t)o * 16 + q] = src.St[(size_t)i * 16 + q];
  }
  if (gauss) { dsb.G[o] = ssb.G[i]; dsb.Gf[o] = ssb.Gf[i]; }
}
// stable compaction: point i with keep[i] moves to offs[i] in the destination arrays
__global__ void __launch_bounds__(256) k_scene_merge_compact(CloudDev src, SceneBuffers ssb, CloudDev dst, SceneBuffers dsb, const SceneStepRecord* __restrict__ rec,
                                                             const int* __restrict__ keep, const int* __restrict__ offs) {
  if (*as_global(&rec->skipped)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= clamped_count(src.count, src.capacity) || !keep[i]) return;
  const int o = offs[i];
  if (o < 0 || o > i) return;        // a compaction only moves a point down
  cloud_move_point(src, ssb, i, dst, dsb, o, ssb.G && dsb.G);
}
// the Gaussian tail [k, gaussLen), k = *total: the reference does not resize the Gaussian vector after a merge (merger.cpp:108-112), so these entries keep
// their old values.  After a Cloud::add the vector has the cloud's size; a cloud that was merged before holds more.  grid = ceil(bound of gaussLen / 256)
__global__ void __launch_bounds__(256) k_scene_gauss_tail(CloudDev cl, SceneBuffers ssb, SceneBuffers dsb, const SceneStepRecord* __restrict__ rec,
                                                          const int* __restrict__ total) {
  if (*as_global(&rec->skipped)) return;
  const int n = clamped_count(&rec->gaussLen, cl.capacity);
  const int i = clamped_count(total, clamped_count(cl.count, cl.capacity)) + blockIdx.x * 256 + threadIdx.x;
  if (i < n) { dsb.G[i] = ssb.G[i]; dsb.Gf[i] = ssb.Gf[i]; }
}
// one thread: the merged size becomes the cloud's
__global__ void k_scene_merge_count(CloudDev cl, const int* __restrict__ total, SceneStepRecord* __restrict__ rec, SceneStepRecord* host) {
  if (rec->skipped) return;
  const int k = clamped_count(total, clamped_count(cl.count, cl.capacity));
  *cl.count = k;
  rec->sizeMerge = k; host->sizeMerge = k;
}

// ------------------------------------------------------------------------------------------------------------------
// exclusive scan of n ints: 1024 per block, block totals scanned by one block, then added back
__global__ void __launch_bounds__(1024) k_scan_blocks(const int* __restrict__ in, int* __restrict__ out, int n, int* __restrict__ sums) {
  __shared__ int s[1024];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const int v = (i < n) ? in[i] : 0;
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int add = (threadIdx.x >= (unsigned)off) ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  if (i < n) out[i] = s[threadIdx.x] - v;
  if (threadIdx.x == 1023) sums[blockIdx.x] = s[1023];
}
__global__ void __launch_bounds__(1024) k_scan_sums(int* __restrict__ sums, int nb, int* __restrict__ total) {
  __shared__ int s[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    const int r = base + threadIdx.x;
    const int v = (r < nb) ? sums[r] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int add = (threadIdx.x >= (unsigned)off) ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    const int incl = s[threadIdx.x];
    const int c0 = carry;
    if (r < nb) sums[r] = c0 + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c0 + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(1024) k_scan_add(int* __restrict__ out, int n, const int* __restrict__ sums) {
  const int i = blockIdx.x * 1024 + threadIdx.x;
  if (i < n) out[i] += sums[blockIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------
// Merger2::merge (pwn_tracker2/merger2.cpp:106-183): one cloud fused into the total cloud (_cloud_tot, weights _pesi_tot).
// 1. k_project_single twice: the cloud under `offset` (idx_current / scaledImage_current, :113-116) and the total under transform * offset
//    (:121-127; an empty total projects nothing, so every index stays -1 as :118 leaves it).  The total's size is read on the device.
// 2. k_merge_clouds_classify: the pixel loop's decisions (:131-179).  A fuse (:153-162) rewrites point and weight of the total in place -- every
//    index of the total sits in at most one pixel -- an append (:134-149, :164-177) only raises the pixel's flag: indexImage_tot was made before
//    the loop, so what the loop appends does not change what it decides.
// 3. exclusive_scan of the flags: the raster-order rank of every appended pixel, the order of the reference's push_backs.
// 4. k_merge_clouds_append: the push_backs, with Cloud::add's per-point arithmetic (cloud_append_point, never the identity shortcut), at
//    count + rank; weight 1 / d (:132, :148).  The Stats block is transform * the source point's own block, as Cloud::add stores it: the
//    reference multiplies a member that every earlier append has left its product in (:139-143) -- docs/parity.md.
// 5. k_merge_clouds_count: count += appended, for the next cloud of the list to read.
// The comparisons are made as the reference makes them: a float against a double literal, in double.
__global__ void __launch_bounds__(256) k_merge_clouds_classify(CloudDev tot, float* __restrict__ weights, const unsigned long long* __restrict__ zcur,
                                                               const unsigned long long* __restrict__ ztot, unsigned tag, int rows, int cols, Mat4 iKRt,
                                                               float minD, float maxD, int* __restrict__ flags, int* __restrict__ fused) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  bool fuse = false;
  if (pix < rows * cols) {
    int flag = 0;
    const float d = zkey_depth(zcur[pix], tag);                  // FLT_MAX where nothing landed
    if ((double)d > 0.2 && (double)d < 100) {                    // :131
      const unsigned long long kt = ztot[pix];
      const int it = zkey_index(kt, tag);
      if (it < 0) flag = 1;                                      // :134
      else {
        const float delta = d - zkey_depth(kt, tag);
        if ((double)fabsf(delta) < .15) {                        // :153
          // PinholePointProjector::unProject(p, j, i, d) (:154): false outside the projector's range, else p = iKRt * (j d, i d, d, 1)
          if (depth_in_range(d, minD, maxD) && it < tot.capacity) {
            const int r = pix / cols, c = pix - r * cols;
            const Vec3 p = unproject_pixel(iKRt, c, r, d);
            const float peso_current = 1.0f / d;
            const float peso_tot = weights[it];
            const float somma_pesi = peso_tot + peso_current;
            const float4 q = load_xyz(tot.P3, it);
            store_xyz(tot.P3, it, (q.x * peso_tot + p.x * peso_current) / somma_pesi, (q.y * peso_tot + p.y * peso_current) / somma_pesi,
                      (q.z * peso_tot + p.z * peso_current) / somma_pesi);
            weights[it] = somma_pesi;
            fuse = true;
          }
        } else if ((double)delta < -.3) flag = 1;                // :164
      }
    }
    flags[pix] = flag;
  }
  const unsigned long long b = __ballot(fuse);
  if (lane_id() == 0 && b) atomicAdd(fused, __popcll(b));
}
__global__ void __launch_bounds__(256) k_merge_clouds_append(CloudDev tot, SceneBuffers tsb, float* __restrict__ weights, CloudDev src, SceneBuffers ssb,
                                                             int ngauss, Mat4 m, const unsigned long long* __restrict__ zcur, unsigned tag, int N,
                                                             const int* __restrict__ flags, const int* __restrict__ offs) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= N || !flags[pix]) return;
  const int o = *tot.count + offs[pix];
  if (o < 0 || o >= tot.capacity) return;
  const unsigned long long kc = zcur[pix];
  const int i = zkey_index(kc, tag);
  if (i < 0 || i >= src.capacity) return;
  cloud_append_point(tot, tsb, src, ssb, i, o, ngauss, m, 0);
  if (tsb.G && !(ssb.G && i < ngauss)) gauss_store_default(tsb, o);       // a source without Gaussians
  weights[o] = 1.0f / zkey_depth(kc, tag);
}
__global__ void k_merge_clouds_count(int* count, const int* total, int* appended) { *count += *total; *appended = *total; }

// ------------------------------------------------------------------------------------------------------------------
// VoxelCalculator::compute (voxelcalculator.cpp:15-73), canonical semantics (the intended lexicographic order of the voxel
// indices; the reference's IndexComparator, voxelcalculator.h:41-48, is not a strict weak ordering -- DESIGN.md): the FIRST point
// (lowest index) of every voxel survives; survivors come out sorted by (ix, iy, iz).
// Keys: the three truncated indices biased into 21 bits each -> one 63-bit word, so integer order == lexicographic order.
constexpr int kVoxelBits = 21, kVoxelBias = 1 << 20;
__device__ __forceinline__ bool voxel_key(const float4 p, float inverseResolution, unsigned long long& key) {
  const float fx = p.x * inverseResolution, fy = p.y * inverseResolution, fz = p.z * inverseResolution;
  if (!(fabsf(fx) < (float)kVoxelBias && fabsf(fy) < (float)kVoxelBias && fabsf(fz) < (float)kVoxelBias)) return false;
  const unsigned long long ix = (unsigned long long)((int)fx + kVoxelBias), iy = (unsigned long long)((int)fy + kVoxelBias),
                           iz = (unsigned long long)((int)fz + kVoxelBias);
  key = (ix << (2 * kVoxelBits)) | (iy << kVoxelBits) | iz;
  return true;
}
__device__ __forceinline__ unsigned long long voxel_hash(unsigned long long k) {      // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 27; k *= 0x94d049bb133111ebull; k ^= k >> 31; return k;
}
// open-addressing table of (key, lowest point index): slot claimed by atomicCAS on the key, index by atomicMin.  tableSize = power of 2.
__global__ void __launch_bounds__(256) k_voxel_insert(CloudDev cl, int n, float inverseResolution, unsigned long long* __restrict__ keys,
                                                      int* __restrict__ first, unsigned tableMask, int* __restrict__ slotOf, int* __restrict__ fault) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned long long key;
  if (!voxel_key(load_xyz(cl.P3, i), inverseResolution, key)) { atomicExch(fault, 1); slotOf[i] = -1; return; }
  unsigned slot = (unsigned)voxel_hash(key) & tableMask;
  for (unsigned probe = 0; probe <= tableMask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[slot], ~0ull, key);
    if (prev == ~0ull || prev == key) { atomicMin(&first[slot], i); slotOf[i] = (int)slot; return; }
    slot = (slot + 1) & tableMask;
  }
  atomicExch(fault, 2); slotOf[i] = -1;
}
__global__ void __launch_bounds__(256) k_voxel_survivors(int n, const int* __restrict__ slotOf, const int* __restrict__ first, int* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) { const int s = slotOf[i]; keep[i] = (s >= 0 && first[s] == i) ? 1 : 0; }
}
// survivors -> (key, index) records in index order (stable compaction), sorted afterwards by key
__global__ void __launch_bounds__(256) k_voxel_records(CloudDev cl, int n, float inverseResolution, const int* __restrict__ keep, const int* __restrict__ offs,
                                                       unsigned long long* __restrict__ rkeys, int* __restrict__ ridx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !keep[i]) return;
  unsigned long long key = 0; (void)voxel_key(load_xyz(cl.P3, i), inverseResolution, key);
  rkeys[offs[i]] = key; ridx[offs[i]] = i;
}
// LSD radix sort, 8 bits per pass, of m (key, index) records: histogram per block -> scan -> stable scatter.
// One block handles 2048 consecutive records; inside a block the scatter keeps input order (a single wave walks the chunk), so every
// pass is stable.  The scene sizes this runs on (<= 2^21 survivors) make 8 passes of this simple kernel cheap next to the merge.
constexpr int kSortChunk = 2048;
__global__ void __launch_bounds__(256) k_sort_hist(const unsigned long long* __restrict__ keys, int m, int shift, int* __restrict__ hist /*[256][nblocks]*/, int nblocks) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * kSortChunk;
  for (int j = threadIdx.x; j < kSortChunk; j += 256) { const int i = base + j; if (i < m) atomicAdd(&h[(int)((keys[i] >> shift) & 255ull)], 1); }
  __syncthreads();
  hist[threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}
__global__ void __launch_bounds__(64) k_sort_scatter(const unsigned long long* __restrict__ keys, const int* __restrict__ idx, int m, int shift,
                                                     const int* __restrict__ offs /*[256][nblocks] exclusive*/, int nblocks,
                                                     unsigned long long* __restrict__ okeys, int* __restrict__ oidx) {
  __shared__ int pos[256];
  for (int d = threadIdx.x; d < 256; d += 64) pos[d] = offs[d * nblocks + blockIdx.x];
  __syncthreads();
  const int base = blockIdx.x * kSortChunk;
  const int lane = threadIdx.x;
  for (int j0 = 0; j0 < kSortChunk; j0 += 64) {
    const int i = base + j0 + lane;
    const bool in = i < m;
    const unsigned long long key = in ? keys[i] : 0ull;
    const int digit = (int)((key >> shift) & 255ull);
    // rank of this lane among the lanes of the wave with the same digit (lower lanes first): stable
    unsigned long long same = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; ++b) { const unsigned long long bal = __ballot((digit >> b) & 1); same &= ((digit >> b) & 1) ? bal : ~bal; }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (in) { const int o = pos[digit] + rank; okeys[o] = key; oidx[o] = idx[i]; }
    __syncthreads();
    if (in && rank == __popcll(same) - 1) pos[digit] += __popcll(same);      // the last lane of each digit group advances the cursor
    __syncthreads();
  }
}
// gather the survivors' arrays in sorted order
__global__ void __launch_bounds__(256) k_voxel_gather(CloudDev src, SceneBuffers ssb, CloudDev dst, SceneBuffers dsb, int m, int withGauss,
                                                      const int* __restrict__ order) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= m) return;
  cloud_move_point(src, ssb, order[o], dst, dsb, o, withGauss != 0);
}

// ------------------------------------------------------------------------------------------------------------------
// ManifoldVoronoiExtractor::process (pwn_tracker2/manifold_voronoi_extractor.cpp:50-127): the clouds of the last key nodes, each under its own
// transform, splatted into an xSize x ySize uint16 grid.  Per cell the reference walks the points in list order, then in index order (:76-121);
// the state of a cell depends on that order, so the splat is not one per-point kernel:
// 1. k_manifold_events: one thread per point.  Its order number is the base of its cloud + its index.  An event that can ever change a cell
//    (inside the grid, :93-98, and squared normal not below 0.1, :109) gets the sort key (bad << 32 | cell) and the value pz; every other point
//    gets the key of the cell one past the grid.  Dropping on the normal test before the height test is safe: both only skip.
// 2. k_sort_hist / k_sort_scatter on the bytes of the cell field only (at most four, the key's low word; the flag lies above every sorted byte): the
//    sort is stable, so a cell's events stay in order.
// 3. k_manifold_starts: where every cell's run begins.
// 4. k_manifold_cells: one wave per cell takes its run from the image's current value, 64 events at a time, and stops at the first obstacle.
// Every dependency is a kernel boundary.
constexpr int kManifoldBadBit = 32;                   // the key's low word is the cell id, 0 .. x_size * y_size <= 2^24, the last one for the points that
                                                      // make no event; a radix pass takes a whole byte, so the flag stays out of the low word
constexpr int kManifoldUntouched = 30000, kManifoldObstacle = 65535;
struct ManifoldCloud { const float* P3; const float4* Nc; int n; int base; Mat4 T; };
struct ManifoldGrid { int xSize, ySize, cx, cy; float ires, normalThreshold; };
// The arithmetic of :91-113 for one point, stated once.  The point and the normal under T as Cloud::transformInPlace computes them; products and
// sums rounded one by one; the conversions truncate toward zero (a sum in (-1, 0) lands in row / column 0).
struct ManifoldEvent { int x, y, pz; bool inside, normal, bad; };
__device__ __forceinline__ ManifoldEvent manifold_event(const ManifoldGrid& g, const Mat4& T, const float4 P, const float4 N) {
  const float3 p = iso_point(T, P), n = iso_normal(T, N);
  ManifoldEvent e;
  e.x = (int)dot2seq((float)g.cx, 1.0f, p.x, g.ires);                                   // :91, indexes rows
  e.y = (int)dot2seq((float)g.cy, 1.0f, p.y, g.ires);                                   // :92, indexes columns
  e.inside = !(e.x < 0 || e.x >= g.xSize || e.y < 0 || e.y >= g.ySize);                 // :93-98
  e.pz = (int)dot2seq(10000.f, 1.0f, -1000.f, p.z);                                     // :100
  e.normal = !((double)dot4seq(n.x, n.x, n.y, n.y, n.z, n.z, 0.f, 0.f) < 0.1);          // :109, a float against a double literal
  e.bad = n.z < g.normalThreshold;                                                      // :113
  return e;
}
// :101-120 for one event on the state s of its cell
__device__ __forceinline__ int manifold_step(int s, int pz, bool bad) {
  if (s == kManifoldObstacle || s < pz) return s;
  return bad ? kManifoldObstacle : (int)(uint16_t)pz;
}
// grid = (ceil(largest cloud / 256), clouds of the chunk), block = 256.  inside[c] += the points of cloud c that fell inside the grid.
__global__ void __launch_bounds__(256) k_manifold_events(const ManifoldCloud* __restrict__ clouds, ManifoldGrid g, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ vals, int* __restrict__ inside) {
  const ManifoldCloud& c = clouds[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  bool in = false;
  if (i < c.n) {
    const float4 nc = c.Nc[i];
    const ManifoldEvent e = manifold_event(g, c.T, load_xyz(c.P3, i), nc);
    in = e.inside;
    const unsigned cell = (in && e.normal) ? (unsigned)(e.x * g.ySize + e.y) : (unsigned)(g.xSize * g.ySize);
    keys[c.base + i] = (unsigned long long)cell | (e.bad ? 1ull << kManifoldBadBit : 0ull);
    vals[c.base + i] = e.pz;
  }
  const unsigned long long b = __ballot(in);
  if (lane_id() == 0 && b) atomicAdd(&cnt, __popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(inside + blockIdx.y, cnt);
}
// start[cell] = the first sorted event of the cell (start holds -1 elsewhere)
__global__ void __launch_bounds__(256) k_manifold_starts(const unsigned long long* __restrict__ keys, int m, int cells, int* __restrict__ start) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const unsigned cell = (unsigned)keys[j];
  if (cell < (unsigned)cells && (j == 0 || (unsigned)keys[j - 1] != cell)) start[cell] = j;
}
// One wave per cell, four cells per workgroup: with a lane per cell the call takes 20 ms for 30 VGA clouds, 17 times this form (DESIGN.md section 5;
// the fullest cell holds 105 646 events, nearly all good points, so the walk never ends early).  The wave takes the run in trips of 64 events, four trips loaded at once.  For events with 0 <= pz <= 65534
// the per-event state functions compose as the monoid (T, M) -- s >= T gives obstacle, else min(s, M); good = (inf, pz), bad = (pz, inf);
// (T1, M1) o (T2, M2) = (M1 >= T2 ? min(T1, T2) : T1, min(M1, M2)) -- which a trip evaluates as: the state before event j is the minimum of the
// state before the trip and the good heights of the trip's earlier events (an exclusive prefix minimum over the lanes); the cell is an obstacle
// when any bad event lies at or below its minimum; otherwise the state is the minimum of all.  A trip that holds a wrapped height (pz < 0 stores
// a larger value, :119) is walked event by event instead (manifold_step), in order, by every lane alike.
constexpr int kManifoldTrips = 4;
__device__ __forceinline__ int manifold_trip(int s, bool in, int pz, bool bad, int lane) {
  const unsigned long long members = __ballot(in);
  if (__ballot(in && (pz < 0 || pz > 65534))) {
    const int n = __popcll(members);                  // the members are the first n lanes: the run is contiguous
    for (int t = 0; t < n && s != kManifoldObstacle; ++t) s = manifold_step(s, __shfl(pz, t), __shfl((int)bad, t) != 0);
    return s;
  }
  int lowest = (in && !bad) ? pz : 0x7fffffff;        // inclusive prefix minimum of the good heights
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(lowest, off); if (lane >= off) lowest = min(lowest, o); }
  int before = __shfl_up(lowest, 1);
  before = min(s, lane == 0 ? 0x7fffffff : before);
  if (__ballot(in && bad && pz <= before)) return kManifoldObstacle;
  return min(s, __shfl(lowest, 63));
}
__global__ void __launch_bounds__(256) k_manifold_cells(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, int m, int cells,
                                                       const int* __restrict__ start, uint16_t* __restrict__ image) {
  const int lane = lane_id();
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const int first = start[cell];
  if (first < 0) return;
  int s = image[cell];
  for (long long base = first; base < m && s != kManifoldObstacle; base += 64 * kManifoldTrips) {
    bool in[kManifoldTrips], bad[kManifoldTrips]; int pz[kManifoldTrips];
#pragma unroll
    for (int t = 0; t < kManifoldTrips; ++t) {        // all loads first
      const long long j = base + 64 * t + lane;
      const unsigned long long k = j < m ? keys[j] : ~0ull;
      in[t] = (unsigned)k == (unsigned)cell;
      bad[t] = (k >> kManifoldBadBit) & 1u;
      pz[t] = j < m ? vals[j] : 0;
    }
    bool more = true;
#pragma unroll
    for (int t = 0; t < kManifoldTrips; ++t) {
      if (!more || s == kManifoldObstacle) break;
      s = manifold_trip(s, in[t], pz[t], bad[t], lane);
      more = __ballot(in[t]) == ~0ull;                // a trip that is not full ends the run
    }
    if (!more) break;
  }
  if (lane == 0) image[cell] = (uint16_t)s;
}
__global__ void __launch_bounds__(256) k_manifold_fill(uint16_t* __restrict__ image, int cells) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cells) image[i] = (uint16_t)kManifoldUntouched;
}

}  // namespace pwnhip
