// pwn_scene_capi.h -- C-ABI entry points of the scene-maintenance stage; included by
// pwn_hip_capi.hip (same translation unit: it uses that file's context, cloud handle and helpers).
// Reference: pwn_core/{cloud.cpp:11-186, merger.cpp:15-119, voxelcalculator.cpp:15-73, gaussian3.h, pinholepointprojector.cpp:93-133}.
#pragma once

#include <fstream>
#include <sstream>

namespace {

// Gaussians of a cloud (24 floats + flags per point); new flags start at zero
int ensure_gauss(pwn_hip_ctx* ctx, pwn_hip_cloud* c) {
  const bool had_flags = c->sb.Gf != nullptr;
  if (int rc = cloud_own(ctx, c, kArrGauss)) return rc;
  if (!had_flags) HIPCHK(ctx, hipMemsetAsync(c->sb.Gf, 0, c->front.Gf.cap * sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// records [from, to) become default Gaussians, all zero and neither form valid (gaussian.h:16-21; what std::vector::resize appends, cloud.cpp:153):
// whoever lets a record into [0, n_gauss) without writing it calls this -- the buffer holds what hipMalloc or an earlier content left there
int default_gaussians(pwn_hip_ctx* ctx, pwn_hip_cloud* c, int from, int to) {
  if (to <= from) return PWN_HIP_OK;
  HIPCHK(ctx, hipMemsetAsync(c->sb.G + from, 0, sizeof(GaussD) * (size_t)(to - from), ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(c->sb.Gf + from, 0, sizeof(int) * (size_t)(to - from), ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// a cloud that receives appended clouds keeps explicit normal information matrices and Stats
int ensure_scene(pwn_hip_ctx* ctx, pwn_hip_cloud* c, bool with_gauss) {
  if (!c->d.OmN) {            // the kernel reads normals, curvatures and the two class matrices, not the planes it writes
    if (int rc = cloud_own(ctx, c, kArrOmN)) return rc;
    if (c->content.n > 0) hipLaunchKernelGGL(k_expand_omega_n, dim3((c->content.n + 255) / 256), dim3(256), 0, ctx->stream, c->d, c->d.OmN, c->content.n);
  }
  if (int rc = cloud_own(ctx, c, kArrSt)) return rc;
  if (!c->content.stats) {    // default Stats() for whatever the cloud already holds
    if (c->content.n > 0) {
      const std::vector<float> st = default_stats(c->content.n);
      HIPCHK(ctx, hipMemcpyAsync(c->d.St, st.data(), st.size() * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
      HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_COPY);
    }
    c->content.set_stats();
  }
  if (with_gauss) { if (int rc = ensure_gauss(ctx, c)) return rc; }
  return PWN_HIP_OK;
}
// context scratch of the scene stage: int arrays of n entries and 64-bit arrays
int scene_scratch(pwn_hip_ctx* ctx, size_t n_int, size_t n_u64) {
  if (n_int + 1024 > ctx->scene_i[0].cap || n_u64 > ctx->scene_k[0].cap) HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  for (auto& b : ctx->scene_i) HIPCHK(ctx, b.ensure(n_int + 1024), PWN_HIP_ERR_ALLOCATION);
  for (auto& b : ctx->scene_k) HIPCHK(ctx, b.ensure(n_u64), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->scene_total.ensure(4), PWN_HIP_ERR_ALLOCATION);
  return PWN_HIP_OK;
}
// the int arrays of that scratch as Merger::merge uses them
struct MergeScratch { int* collapsed; int* head; int* next; int* keep; int* offs; int* sums; };
MergeScratch merge_scratch(pwn_hip_ctx* ctx) { return { ctx->scene_i[0], ctx->scene_i[1], ctx->scene_i[2], ctx->scene_i[3], ctx->scene_i[4], ctx->scene_i[5] }; }
// out[i] = sum of in[0..i), *total = sum of all; sums: scratch of >= n/1024 + 1 ints
int exclusive_scan(pwn_hip_ctx* ctx, const int* in, int* out, int n, int* sums, int* total) {
  const int nb = (n + 1023) / 1024;
  if (n <= 0) { HIPCHK(ctx, hipMemsetAsync(total, 0, sizeof(int), ctx->stream), PWN_HIP_ERR_COPY); return PWN_HIP_OK; }
  hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(1024), 0, ctx->stream, in, out, n, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, sums, nb, total);
  hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(1024), 0, ctx->stream, out, n, (const int*)sums);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// The scene record of a stand-alone call (pwn_scene_kernels.h): the host fills it and sends it to the device in front of the call's kernels, through
// the page-locked copy that the kernels write their sizes back to
int record_send(pwn_hip_ctx* ctx, const SceneStepRecord& r) {
  HIPCHK(ctx, ctx->step_dev.ensure(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->step_host.ensure(1), PWN_HIP_ERR_ALLOCATION);
  *ctx->step_host.p = r;
  HIPCHK(ctx, hipMemcpyAsync(ctx->step_dev.p, ctx->step_host.p, sizeof(SceneStepRecord), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// Merger::merge queued on st, steps 1-4 of pwn_scene_kernels.h on the size the device holds with the record's view; the survivors go to the back
// set, the new size into the device's word and both copies of the record.  bound / gaussBound: the host's upper bounds of the cloud's size and of
// its Gaussian vector's length (grids, fill, scan); scene_scratch has been made for the bound.  collapsed[0, bound) is ready for the host behind it.
int merge_enqueue(pwn_hip_ctx* ctx, hipStream_t st, const pwn_hip_cloud* cloud, const CloudDev& back, const SceneBuffers& sback, SceneStepRecord* rec,
                  SceneStepRecord* host, const MergeView& v, size_t bound, size_t gaussBound, unsigned tag) {
  const MergeScratch s = merge_scratch(ctx);
  const SceneStepRecord* r = rec;
  const dim3 nb((unsigned)((bound + 255) / 256));
  hipLaunchKernelGGL(k_scene_merge_project, nb, dim3(256), 0, st, cloud->d, r, v.minD, v.maxD, v.rows, v.cols, ctx->zref_ws, tag);
  HIPCHK(ctx, hipMemsetAsync(s.head, 0xFF, sizeof(int) * bound, st), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_scene_merge_classify, nb, dim3(256), 0, st, cloud->d, r, v, (const unsigned long long*)ctx->zref_ws, tag, s.collapsed, s.head, s.next);
  hipLaunchKernelGGL(k_scene_merge_accumulate, nb, dim3(256), 0, st, cloud->d, cloud->sb, r, (const int*)s.collapsed, (const int*)s.head, (const int*)s.next);
  hipLaunchKernelGGL(k_scene_merge_keep_flags, nb, dim3(256), 0, st, cloud->d, r, s.collapsed, (int)bound, s.keep);
  if (int rc = exclusive_scan(ctx, s.keep, s.offs, (int)bound, s.sums, ctx->scene_total)) return rc;
  hipLaunchKernelGGL(k_scene_merge_compact, nb, dim3(256), 0, st, cloud->d, cloud->sb, back, sback, r, (const int*)s.keep, (const int*)s.offs);
  hipLaunchKernelGGL(k_scene_gauss_tail, dim3((unsigned)((gaussBound + 255) / 256)), dim3(256), 0, st, cloud->d, cloud->sb, sback, r, (const int*)ctx->scene_total);
  hipLaunchKernelGGL(k_scene_merge_count, dim3(1), dim3(1), 0, st, cloud->d, (const int*)ctx->scene_total, rec, host);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// after the wait: a merge of `before` points has left `after` of them in the back set, which becomes the front (an empty cloud moved nothing), and
// has set the device's word
int merge_commit(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, int before, int after) {
  if (before > 0) cloud->swap_sides();
  return cloud_edit(ctx, cloud, after, false);
}
// Stable LSD radix sort of m (key, value) records by the low `bits` bits of the key, 8 bits per pass (k_sort_hist, the scan of the histogram,
// k_sort_scatter), from (key[0], val[0]) to and fro between the two pairs; *in says which pair holds the result.  hist: 256 ints per block of
// kSortChunk records, sums: the scan's scratch.
int radix_sort(pwn_hip_ctx* ctx, unsigned long long* const key[2], int* const val[2], int m, int bits, int* hist, int* sums, int* in) {
  const int sb_ = (m + kSortChunk - 1) / kSortChunk;
  int a = 0;
  for (int pass = 0; 8 * pass < bits && m > 1; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(k_sort_hist, dim3(sb_), dim3(256), 0, ctx->stream, (const unsigned long long*)key[a], m, shift, hist, sb_);
    if (int rc = exclusive_scan(ctx, hist, hist, 256 * sb_, sums, ctx->scene_total + 2)) return rc;
    hipLaunchKernelGGL(k_sort_scatter, dim3(sb_), dim3(64), 0, ctx->stream, (const unsigned long long*)key[a], (const int*)val[a], m, shift, (const int*)hist, sb_,
                       key[a ^ 1], val[a ^ 1]);
    a ^= 1;
  }
  *in = a;
  return PWN_HIP_OK;
}

}  // namespace

extern "C" {

// The Gaussian half of PinholePointProjector::unProject (pinholepointprojector.cpp:104-123) for a cloud that pwn_hip_convert made
// from the same depth image with the same parameters (incl. Cloud::transformInPlace(sensorOffset) on them, cloud.cpp:180).
int pwn_hip_cloud_gaussians(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, pwn_hip_cloud* cloud,
                            float baseline, float alpha) {
  if (!ctx || !p || !depth || !cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (int rc = ensure_gauss(ctx, cloud)) return rc;
  if (int rc = ensure_desc(ctx, 1)) return rc;
  if (int rc = absorb_copies(ctx)) return rc;      // caller pointers may be the destination of a queued pwn_hip_copy_async
  const size_t N = (size_t)rows * cols;
  const ConvertParams cp = make_convert_params(ctx, p, nullptr, rows, cols, 0);
  Mat4 KRt, iKRt; Mat3 iK;
  projector_matrices(mat3_from(p->K), mat4_identity(), KRt, iKRt, iK);
  const float* d = nullptr;
  if (int rc = stage_depth(ctx, depth, N, &d)) return rc;
  fill_frame(ctx, 0, 0, d, cloud->d);
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev, ctx->frames_host, sizeof(FrameDesc), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_row_count, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp);
  hipLaunchKernelGGL(k_row_offsets, dim3(1), dim3(1024), 0, ctx->stream, ctx->frames_dev, rows);
  hipLaunchKernelGGL(k_gaussians, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp, iK, baseline * p->K[0], alpha, cloud->sb);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  pwn_hip_cloud* cl[1] = { cloud };
  if (int rc = sync_and_counts(ctx, cl, 1)) return rc;
  cloud->content.set_gaussians(cloud->content.n);
  return PWN_HIP_OK;
}
// Test-only (include/pwn_hip_testing.h): the store form of k_gaussians_batch
int pwn_hip_debug_set_gaussian_stores(pwn_hip_ctx* ctx, int staged) {
  if (!ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  ctx->gauss_staged = (staged == 0 || staged == 1) ? staged : kGaussStagedDefault;
  return PWN_HIP_OK;
}
int pwn_hip_cloud_num_gaussians(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, int* n) {
  if (!c || !n) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *n = c->view().gauss;
  return PWN_HIP_OK;
}
// mean n*3, cov n*9 (column-major 3x3), info_vec n*3, info n*9, flags n (1 = moments valid, 2 = information form valid); host pointers
int pwn_hip_cloud_download_gaussians(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, float* mean, float* cov, float* info_vec, float* info, int* flags) {
  if (!ctx || !c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int n = c->view().gauss;
  if (n == 0) return PWN_HIP_OK;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  std::vector<GaussD> g(n); std::vector<int> f(n);
  HIPCHK(ctx, hipMemcpy(g.data(), c->sb.G, sizeof(GaussD) * (size_t)n, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpy(f.data(), c->sb.Gf, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
  for (int i = 0; i < n; ++i) {
    if (mean) std::memcpy(mean + 3 * (size_t)i, g[i].mean, 12);
    if (cov) std::memcpy(cov + 9 * (size_t)i, g[i].cov, 36);
    if (info_vec) std::memcpy(info_vec + 3 * (size_t)i, g[i].infoVec, 12);
    if (info) std::memcpy(info + 9 * (size_t)i, g[i].info, 36);
    if (flags) flags[i] = f[i];
  }
  return PWN_HIP_OK;
}
// Test-only (include/pwn_hip_testing.h): the cloud's Gaussian vector becomes the n records given, in the layout pwn_hip_cloud_download_gaussians
// returns.  n need not be the cloud's size.  Everything is checked before anything is written.
int pwn_hip_debug_cloud_set_gaussians(pwn_hip_ctx* ctx, pwn_hip_cloud* c, int n, const float* mean, const float* cov, const float* info_vec,
                                      const float* info, const int* flags) {
  if (!ctx || !c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (c->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
  if (n < 0 || n > c->d.capacity) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "number of Gaussians outside [0, capacity]");
  if (n > 0 && (!mean || !cov || !info_vec || !info || !flags)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < n; ++i)
    if (flags[i] & ~(kGaussMoments | kGaussInfo)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "Gaussian flags outside 0..3");
  if (int rc = ensure_gauss(ctx, c)) return rc;
  if (n > 0) {
    std::vector<GaussD> g(n);
    for (int i = 0; i < n; ++i) {
      std::memcpy(g[i].mean, mean + 3 * (size_t)i, 12); std::memcpy(g[i].cov, cov + 9 * (size_t)i, 36);
      std::memcpy(g[i].infoVec, info_vec + 3 * (size_t)i, 12); std::memcpy(g[i].info, info + 9 * (size_t)i, 36);
    }
    HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
    HIPCHK(ctx, hipMemcpy(c->sb.G, g.data(), sizeof(GaussD) * (size_t)n, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemcpy(c->sb.Gf, flags, sizeof(int) * (size_t)n, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  }
  c->content.set_gaussians(n);
  return PWN_HIP_OK;
}
// Test-only (include/pwn_hip_testing.h): the vector's length alone
int pwn_hip_debug_cloud_expose_gaussians(pwn_hip_ctx* ctx, pwn_hip_cloud* c, int n) {
  if (!ctx || !c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (c->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
  if (n < 0 || n > c->d.capacity || !c->sb.G || !c->sb.Gf) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "number of Gaussians outside [0, capacity], or no Gaussian arrays");
  c->content.set_gaussians(n);
  return PWN_HIP_OK;
}

// Cloud::add (cloud.cpp:145-171): dst gets a copy of src transformed by T appended; src is not modified.
int pwn_hip_cloud_add(pwn_hip_ctx* ctx, pwn_hip_cloud* dst, const pwn_hip_cloud* src, const float T[16]) {
  if (!ctx || !dst || !src || !T) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (dst == src) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cannot add a cloud to itself");
  cloud_changes(ctx, dst);
  const CloudView s = src->view();
  const int k = dst->content.n, n = s.n;
  if ((size_t)k + (size_t)n > (size_t)dst->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "destination cloud capacity too small for Cloud::add");
  if (int rc = ensure_scene(ctx, dst, s.gauss > 0 || dst->sb.G)) return rc;
  const Mat4 m = forced(T);
  const int ident = is_identity(m) ? 1 : 0;                                  // cloud.cpp:176
  const int ng = s.point_gauss();
  if (n > 0) hipLaunchKernelGGL(k_cloud_append, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dst->d, dst->sb, s.d, s.sb, k, n, ng, m, ident);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  // _gaussians.resize(k + cloud.gaussians().size()) (cloud.cpp:153): records the vector had stay, the kernel wrote [k, k + ng), every other
  // record of the new size is a default Gaussian -- the destination's own points up to k, and what a source with more Gaussians than points adds
  const int newg = dst->sb.G ? std::min(k + s.gauss, dst->d.capacity) : 0;
  if (dst->sb.G) {
    if (int rc = default_gaussians(ctx, dst, dst->content.n_gauss, std::min(k, newg))) return rc;
    if (int rc = default_gaussians(ctx, dst, std::max(dst->content.n_gauss, k + ng), newg)) return rc;
    dst->content.set_gaussians(newg);
  }
  if (int rc = cloud_edit(ctx, dst, k + n, true)) return rc;      // edit: the host decides the new size
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}

// Merger::merge (merger.cpp:15-119).  K / min_distance / max_distance: the projector of the merger's DepthImageConverter; T: its pose.
// collapsed (optional, host, size of the cloud before the call) receives _collapsedIndices.
int pwn_hip_merge(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, const float K[9], const float T[16], float min_distance, float max_distance, int rows, int cols,
                  float distance_threshold, float normal_threshold, float max_point_depth, int* new_size, int* collapsed) {
  if (!ctx || !cloud || !K || !T) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  cloud_changes(ctx, cloud);
  const int n = cloud->content.n, ngauss = cloud->content.n_gauss;
  if (n > kMaxCloudPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud has more points than the z-buffer index field holds (2^25)");
  if (!cloud->sb.G || ngauss < n) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "Merger::merge needs the cloud's Gaussians (pwn_hip_cloud_gaussians)");
  if (n == 0) { if (new_size) *new_size = 0; return PWN_HIP_OK; }
  CloudDev back; SceneBuffers sback;      // the second array set: the stable compaction / reordering writes there, then the two sets change places
  HIPCHK(ctx, cloud->own_back(back, sback), PWN_HIP_ERR_ALLOCATION);
  if (int rc = scene_scratch(ctx, (size_t)n, 0)) return rc;
  unsigned tag = kZTag0;
  if (int rc = take_tags(ctx, 1, &tag)) return rc;
  SceneStepRecord r;                      // nothing skipped, no add in front: the sizes as the host knows them
  r.sceneT = mat4_identity(); r.identity = 1; r.skipped = 0; r.sizeAdd = r.sizeMerge = n; r.gaussLen = ngauss;
  { Mat4 iKRt; Mat3 iK; projector_matrices(mat3_from(K), mat4_from(T), r.mergeKRt, iKRt, iK); }
  if (int rc = record_send(ctx, r)) return rc;
  SceneStepRecord* host = ctx->step_host;
  hipStream_t st = ctx->stream;
  const MergeView view = { min_distance, max_distance, max_point_depth, rows, cols, distance_threshold, normal_threshold };
  if (int rc = merge_enqueue(ctx, st, cloud, back, sback, ctx->step_dev, host, view, (size_t)n, (size_t)ngauss, tag)) return rc;
  if (collapsed) HIPCHK(ctx, hipMemcpyAsync(collapsed, merge_scratch(ctx).collapsed, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  const int k = host->sizeMerge;
  if (int rc = merge_commit(ctx, cloud, n, k)) return rc;
  ctx->img.invalidate();                  // slot 0 of the z-buffer was used
  if (new_size) *new_size = k;
  return PWN_HIP_OK;
}

void pwn_hip_default_scene_step_params(pwn_hip_scene_step_params* p) {
  if (!p) return;
  p->distance_threshold = 0.1f; p->normal_threshold = std::cos(10 * (float)M_PI / 180.0f); p->max_point_depth = 10.0f;      // merger.cpp:6-8
  p->baseline = 0.075f; p->alpha = 0.1f;                                                                                     // pinholepointprojector.cpp:10-11
  p->step = 0; p->max_depth_cov = 0.01f;
}
// The mapping step (pwn_aligner.cpp:166-209) in one submission: the two conversions and the rendering go in front of the alignment's kernels on its
// stream (AlignHooks::pre_sub), k_scene_pose, the add and the merge behind them (before_sync); the host waits once (align_batch_once) and does the
// bookkeeping of pwn_hip_cloud_add / pwn_hip_merge afterwards.  Everything that can refuse the call is looked at before a cloud is touched.
int pwn_hip_scene_step(pwn_hip_ctx* ctx, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, const pwn_hip_scene_step_params* sp,
                       const void* frame, int raw_u16, float depth_scale, int rows, int cols, const float scene_T[16], pwn_hip_cloud* scene,
                       pwn_hip_cloud* cloud, pwn_hip_cloud* subscene, pwn_hip_scene_step_result* result, int* collapsed) {
  if (!ctx || !cp || !ap || !sp || !frame || !scene_T || !scene || !cloud || !subscene || !result) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (scene == cloud || scene == subscene || cloud == subscene) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "the three clouds of a mapping step must be distinct");
  if (scene->owner != ctx || cloud->owner != ctx || subscene->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
  if (scene->d.omSym != cloud->d.omSym || scene->d.omSym != subscene->d.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "clouds with different omega storages");
  if (sp->step < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImage_scale: step < 0");
  if (!std::isfinite(sp->baseline) || !std::isfinite(sp->alpha)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "baseline or alpha is not finite");
  if (cp->min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  ConvertCall frameCall; frameCall.p = cp; frameCall.n = 1; frameCall.rows = rows; frameCall.cols = cols;
  frameCall.raw = raw_u16 != 0; frameCall.depth_scale = frameCall.raw ? depth_scale : 0.f; frameCall.keep_stats = 1;
  if (sp->step) {
    if (int rc = make_scale_spec(ctx, rows, cols, sp->step, sp->max_depth_cov, frameCall.scale)) return rc;
    frameCall.rows = frameCall.scale.orows; frameCall.cols = frameCall.scale.ocols;
  }
  const int vrows = frameCall.rows, vcols = frameCall.cols;      // the view: what is converted, rendered, aligned and merged
  if (int rc = check_image(ctx, vrows, vcols)) return rc;
  if (ap->rows != vrows || ap->cols != vcols) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "aligner image size differs from the converted frame's");
  if (int rc = check_align_params(ctx, ap)) return rc;
  const int pixels = vrows * vcols;
  if (pixels > kMaxAlignerPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "Aligner::align: frames of more than 2^21 pixels (index field of the aligner's z-buffer word)");
  const int k0 = scene->content.n;
  if (!(scene->sb.G ? scene->content.n_gauss >= k0 : k0 == 0)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "Merger::merge needs the scene's Gaussians (fewer Gaussians than points)");
  const size_t bound = (size_t)k0 + (size_t)pixels;              // what the scene can hold after the add
  if (bound > (size_t)scene->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "scene capacity smaller than its size plus the pixels of the frame");
  if (bound > (size_t)kMaxCloudPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "the scene could exceed what the z-buffer index field holds (2^25)");
  if (cloud->d.capacity < pixels || subscene->d.capacity < pixels) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity smaller than the pixels of the converted frame");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;      // caller pointers may be the destination of a queued pwn_hip_copy_async
  // ---- allocations and whatever waits for the stream: before anything of the step is queued
  if (int rc = ensure_desc(ctx, 2)) return rc;
  if (sp->step) { if (int rc = ensure_scale(ctx, 2)) return rc; }
  HIPCHK(ctx, ctx->scene_depth_ws.ensure(ctx->N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->step_dev.ensure(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->step_host.ensure(1), PWN_HIP_ERR_ALLOCATION);
  cloud_changes(ctx, scene);
  if (int rc = ensure_scene(ctx, scene, true)) return rc;
  CloudDev back; SceneBuffers sback;
  HIPCHK(ctx, scene->own_back(back, sback), PWN_HIP_ERR_ALLOCATION);
  // the scene grows by a frame per call: when the scratch is too small it is made for twice the bound (within the capacity), so that growing it --
  // a wait for the stream, a free and an allocation per array -- happens once in a while, not once per frame
  size_t scratch = bound;
  for (const auto& b : ctx->scene_i) if (b.cap < bound + 1024) scratch = std::min((size_t)scene->d.capacity, 2 * bound);
  if (int rc = scene_scratch(ctx, scratch, 0)) return rc;
  // ---- the two conversions: entries 0 and 1 of the descriptor arrays, both in workspace slot 0 (they follow each other on one stream)
  const void* frames[1] = { frame }; pwn_hip_cloud* frameCloud[1] = { cloud };
  frameCall.frames = frames; frameCall.clouds = frameCloud;
  { Mat4 KRt, iKRt; projector_matrices(mat3_from(cp->K), mat4_identity(), KRt, iKRt, frameCall.gauss.iK); }
  frameCall.gauss.on = true; frameCall.gauss.fB = sp->baseline * cp->K[0]; frameCall.gauss.alpha = sp->alpha;
  const float* rendering[1] = { ctx->scene_depth_ws }; pwn_hip_cloud* subCloud[1] = { subscene };
  ConvertCall subCall = convert_call(cp, rendering, 0.f, 1, vrows, vcols, subCloud);
  subCall.first_entry = 1;
  const std::vector<int> slot(1, 0);
  ConvertJob frameJob, subJob;
  if (int rc = convert_prepare(ctx, frameCall, slot, true, frameJob)) return rc;
  if (int rc = convert_prepare(ctx, subCall, slot, true, subJob)) return rc;
  int* faultWord = ctx->counts_host + 2;           // behind the two counts: what counts_check reads for a call of two frames
  const Mat3 K = mat3_from(cp->K);
  const Mat4 sceneT0 = mat4_from(scene_T), offset = forced(cp->sensor_offset);
  Mat4 renderKRt;
  { Mat4 iKRt; Mat3 iK; projector_matrices(K, iso_mul(sceneT0, offset), renderKRt, iKRt, iK); }
  const MergeView view = { cp->min_distance, cp->max_distance, sp->max_point_depth, vrows, vcols, sp->distance_threshold, sp->normal_threshold };
  SceneStepRecord* rec = ctx->step_dev; SceneStepRecord* host = ctx->step_host;
  AlignHooks hooks;
  hooks.pre_sub = [&](int, int, int, hipStream_t st) -> int {
    *faultWord = 0;
    if (frameJob.host_input) { if (int rc = convert_stage_frames(ctx, frameJob, 0, 1, st)) return rc; }
    if (int rc = convert_enqueue(ctx, frameJob, 0, 1, st, faultWord)) return rc;
    { StageTimer t(ctx, "scene_render", st);      // pwn_hip_project's commands, the depth image alone, on the size the device holds
      if (int rc = render_enqueue(ctx, st, scene->d, k0, renderKRt, cp->min_distance, cp->max_distance, vrows, vcols, nullptr, ctx->scene_depth_ws)) return rc; }
    return convert_enqueue(ctx, subJob, 0, 1, st, faultWord);
  };
  hooks.before_sync = [&]() -> int {
    hipStream_t st = ctx->stream;
    { StageTimer t(ctx, "scene_pose");
      hipLaunchKernelGGL(k_scene_pose, dim3(1), dim3(1), 0, st, (const PairState*)ctx->state_ws, sceneT0, K, offset, (const int*)ctx->fault_dev,
                         (const int*)ctx->align_fault_host, (const int*)scene->d.count, scene->d.capacity, rec, host); }
    { StageTimer t(ctx, "scene_add");
      hipLaunchKernelGGL(k_scene_append, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, scene->d, scene->sb, cloud->d, cloud->sb, (const SceneStepRecord*)rec);
      hipLaunchKernelGGL(k_scene_grow, dim3(1), dim3(1), 0, st, scene->d, cloud->d, rec, host); }
    unsigned tag = kZTag0;
    if (int rc = take_tags(ctx, 1, &tag)) return rc;
    { StageTimer t(ctx, "scene_merge");
      if (int rc = merge_enqueue(ctx, st, scene, back, sback, rec, host, view, bound, bound, tag)) return rc; }
    if (collapsed) HIPCHK(ctx, hipMemcpyAsync(collapsed, merge_scratch(ctx).collapsed, sizeof(int) * bound, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
    return PWN_HIP_OK;
  };
  // after the wait: an attempt whose projection gave up commits nothing (align_finish digests the fault word, the repeat converts again); else
  // the two conversions end as a batch of two frames ends
  hooks.after_sync = [&]() -> int {
    if (*(volatile int*)ctx->align_fault_host != 0) return PWN_HIP_OK;
    pwn_hip_cloud* both[2] = { cloud, subscene };
    if (int rc = counts_check(ctx, both, 2)) return rc;
    cloud_commit_with_gaussians(cloud, ctx->counts_host[0]); frameJob.committed = true;
    cloud_commit(subscene, ctx->counts_host[1]); subJob.committed = true;
    return PWN_HIP_OK;
  };
  pwn_hip_cloud* refs[1] = { subscene }; pwn_hip_cloud* curs[1] = { cloud };
  const Mat4 I = mat4_identity();
  AlignCall call = align_call(ap, 1, refs, curs, I.m, &result->align);
  call.hooks = &hooks;
  if (int rc = align_batch_impl(ctx, call)) return rc;
  ctx->img.invalidate();                  // slot 0 of the z-buffer was used
  if (host->skipped) return fail(ctx, PWN_HIP_ERR_LAUNCH, "mapping step: skipped on the device without a fault on the host");
  // ---- the bookkeeping of pwn_hip_cloud_add and pwn_hip_merge
  const int nAdd = host->sizeAdd, nMerge = host->sizeMerge;
  scene->content.set_gaussians(nAdd);     // _gaussians.resize(k + cloud.gaussians().size()) (cloud.cpp:153); the merge does not resize it
  if (int rc = merge_commit(ctx, scene, nAdd, nMerge)) return rc;
  std::memcpy(result->scene_T, host->sceneT.m, sizeof(result->scene_T));
  result->n_cloud = cloud->content.n; result->n_subscene = subscene->content.n;
  result->size_after_add = nAdd; result->size_after_merge = nMerge;
  return PWN_HIP_OK;
}

// Merger2::merge (pwn_tracker2/merger2.cpp:106-183) for the clouds of a node list (PwnMerger::mergeNodeList, pwn_tracker2/pwn_merger.cpp:44-54) in one
// submission: per cloud the two projections, the pixel loop's decisions and in-place fuses, the ordered compaction of the appended pixels and the
// appends (pwn_scene_kernels.h).  The total's size stays on the device between the clouds (CloudDev::count); the grids are sized by the host's upper
// bound, size + the sizes of the sources so far, and the host waits once, at the end.  Everything is checked before anything is written.
int pwn_hip_merge_clouds(pwn_hip_ctx* ctx, const float K[9], const float offset[16], int n, pwn_hip_cloud* const* clouds, const float* transforms,
                         float min_distance, float max_distance, int rows, int cols, pwn_hip_cloud* total, float* weights, int* appended, int* fused) {
  if (!ctx || !K || !offset || !total || !weights) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative number of clouds");
  if (n > 0 && (!clouds || !transforms)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (total->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
  const int k0 = total->content.n;
  size_t bound = (size_t)k0;
  bool anyGauss = false;
  for (int i = 0; i < n; ++i) {
    const pwn_hip_cloud* c = clouds[i];
    if (!c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null cloud");
    if (c->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
    if (c == total) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "the total cloud is among the clouds merged into it");
    if (c->d.omSym != total->d.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "clouds with different omega storages");
    bound += (size_t)c->content.n;
    anyGauss = anyGauss || c->view().gauss > 0;
  }
  if (n == 0) return PWN_HIP_OK;
  if (bound > (size_t)total->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "total cloud capacity smaller than its size plus the sizes of the merged clouds");
  if (bound > (size_t)kMaxCloudPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "the total cloud could exceed what the z-buffer index field holds (2^25)");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;      // `weights` may be the destination of a queued pwn_hip_copy_async
  cloud_changes(ctx, total);
  const int N = rows * cols;
  if (int rc = scene_scratch(ctx, (size_t)N, (size_t)N)) return rc;
  HIPCHK(ctx, ctx->merge_counts_dev.ensure(2 * (size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->merge_counts_host.ensure(2 * (size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  float* w = weights;
  if (!is_device_ptr(weights)) { HIPCHK(ctx, ctx->cloud_weights_ws.ensure((size_t)total->d.capacity), PWN_HIP_ERR_ALLOCATION); w = ctx->cloud_weights_ws; }
  if (int rc = ensure_scene(ctx, total, anyGauss || total->sb.G)) return rc;
  hipStream_t st = ctx->stream;
  if (w != weights && k0 > 0) HIPCHK(ctx, hipMemcpyAsync(w, weights, sizeof(float) * (size_t)k0, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  // Gaussians the total has not got for the points it already holds are default Gaussians (as pwn_hip_cloud_add leaves them)
  if (total->sb.G) { if (int rc = default_gaussians(ctx, total, total->content.n_gauss, k0)) return rc; }
  int* d_counts = ctx->merge_counts_dev;             // appended[n], fused[n]
  HIPCHK(ctx, hipMemsetAsync(d_counts, 0, sizeof(int) * 2 * (size_t)n, st), PWN_HIP_ERR_COPY);
  unsigned long long* zcur = ctx->scene_k[0]; unsigned long long* ztot = ctx->scene_k[1];
  int* d_flags = ctx->scene_i[0]; int* d_offs = ctx->scene_i[1]; int* d_sums = ctx->scene_i[2];
  const Mat3 Km = mat3_from(K);
  const Mat4 off = mat4_from(offset);
  Mat4 KRtOff, iKRtOff; Mat3 iK;
  projector_matrices(Km, off, KRtOff, iKRtOff, iK);                                        // setTransform(offset), :113
  const int nbp = (N + 255) / 256;
  size_t upper = (size_t)k0;                         // what the total can hold when cloud i is merged
  for (int i = 0; i < n; ++i) {
    const pwn_hip_cloud* c = clouds[i];
    const Mat4 T = mat4_from(transforms + 16 * (size_t)i);
    Mat4 KRtTot, iKRtTot;
    projector_matrices(Km, iso_mul(T, off), KRtTot, iKRtTot, iK);                          // setTransform(transform * offset), :121
    HIPCHK(ctx, hipMemsetAsync(zcur, 0xFF, sizeof(unsigned long long) * (size_t)N, st), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemsetAsync(ztot, 0xFF, sizeof(unsigned long long) * (size_t)N, st), PWN_HIP_ERR_COPY);
    if (c->content.n > 0)
      hipLaunchKernelGGL(k_project_single, dim3((c->content.n + 255) / 256), dim3(256), 0, st, c->d, KRtOff, min_distance, max_distance, rows, cols, zcur, kZTag0);
    if (upper > 0)
      hipLaunchKernelGGL(k_project_single, dim3((unsigned)((upper + 255) / 256)), dim3(256), 0, st, total->d, KRtTot, min_distance, max_distance, rows, cols, ztot, kZTag0);
    hipLaunchKernelGGL(k_merge_clouds_classify, dim3(nbp), dim3(256), 0, st, total->d, w, (const unsigned long long*)zcur, (const unsigned long long*)ztot, kZTag0,
                       rows, cols, iKRtTot, min_distance, max_distance, d_flags, d_counts + n + i);
    if (int rc = exclusive_scan(ctx, d_flags, d_offs, N, d_sums, ctx->scene_total)) return rc;
    const CloudView s = c->view();
    hipLaunchKernelGGL(k_merge_clouds_append, dim3(nbp), dim3(256), 0, st, total->d, total->sb, w, s.d, s.sb, s.point_gauss(), forced(transforms + 16 * (size_t)i),
                       (const unsigned long long*)zcur, kZTag0, N, (const int*)d_flags, (const int*)d_offs);
    hipLaunchKernelGGL(k_merge_clouds_count, dim3(1), dim3(1), 0, st, total->d.count, (const int*)ctx->scene_total, d_counts + i);
    HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
    upper += (size_t)c->content.n;
  }
  int* h = ctx->merge_counts_host;
  HIPCHK(ctx, hipMemcpyAsync(h, d_counts, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(h + 2 * n, total->d.count, sizeof(int), hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  const int k1 = h[2 * n];
  if (w != weights && k1 > 0) HIPCHK(ctx, hipMemcpy(weights, w, sizeof(float) * (size_t)k1, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
  if (appended) std::copy(h, h + n, appended);
  if (fused) std::copy(h + n, h + 2 * n, fused);
  if (total->sb.G) total->content.set_gaussians(k1);
  return cloud_edit(ctx, total, k1, false);      // edit: k_merge_clouds_count kept the device's word
}

// ManifoldVoronoiExtractor::process (pwn_tracker2/manifold_voronoi_extractor.cpp:50-127): the traversability image of clouds[0..n), cloud i under
// transforms[i], in one submission (pwn_scene_kernels.h).  Clouds are taken in chunks of whole clouds with at most ctx->manifold_chunk points; the
// image carries the state from chunk to chunk, so the bits do not depend on the chunking.  Scratch is sized by the largest chunk's point count, which
// the host knows; the host waits once, at the end.  Everything is checked before anything is written.
int pwn_hip_manifold_image(pwn_hip_ctx* ctx, int n, pwn_hip_cloud* const* clouds, const float* transforms, float resolution, int x_size, int y_size,
                           float normal_threshold, int accumulate, uint16_t* image, int* inside) {
  if (!ctx || !image) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative number of clouds");
  if (n > 0 && (!clouds || !transforms)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (x_size <= 0 || y_size <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "grid has zero size");
  if ((long long)x_size * y_size > (1ll << 24)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "grid has more than 2^24 cells");
  if (!std::isfinite(resolution) || !(resolution > 0.f)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "resolution must be finite and positive");
  // chunks of whole clouds: [first, last), points, largest cloud
  struct Chunk { int first, last; size_t points; int largest; };
  std::vector<Chunk> chunks;
  size_t most = 0;
  for (int i = 0; i < n; ++i) {
    const pwn_hip_cloud* c = clouds[i];
    if (!c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null cloud");
    if (c->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
    if (c->content.n > ctx->manifold_chunk)
      return fail(ctx, PWN_HIP_ERR_CAPACITY, "a cloud has more points than one chunk holds (" + std::to_string(ctx->manifold_chunk) + ")");
    if (chunks.empty() || chunks.back().points + (size_t)c->content.n > (size_t)ctx->manifold_chunk || chunks.back().last - chunks.back().first >= 65535)
      chunks.push_back({ i, i, 0, 0 });
    Chunk& k = chunks.back();
    k.last = i + 1; k.points += (size_t)c->content.n; k.largest = std::max(k.largest, c->content.n);
    most = std::max(most, k.points);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;      // `image` may be the destination of a queued pwn_hip_copy_async
  const int cells = x_size * y_size;
  const size_t sortBlocks = (most + kSortChunk - 1) / kSortChunk;
  if (int rc = scene_scratch(ctx, std::max(std::max(most, (size_t)cells), 256 * sortBlocks + 1024), most)) return rc;
  HIPCHK(ctx, ctx->manifold_dev.ensure((size_t)std::max(n, 1)), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->manifold_host.ensure((size_t)std::max(n, 1)), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->merge_counts_dev.ensure((size_t)std::max(n, 1)), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->merge_counts_host.ensure((size_t)std::max(n, 1)), PWN_HIP_ERR_ALLOCATION);
  hipStream_t st = ctx->stream;
  uint16_t* img = image;
  if (!is_device_ptr(image)) {
    HIPCHK(ctx, ctx->manifold_img_dev.ensure((size_t)cells), PWN_HIP_ERR_ALLOCATION);
    HIPCHK(ctx, ctx->manifold_img_host.ensure((size_t)cells), PWN_HIP_ERR_ALLOCATION);
    img = ctx->manifold_img_dev;
    if (accumulate) {
      std::memcpy(ctx->manifold_img_host.p, image, sizeof(uint16_t) * (size_t)cells);
      HIPCHK(ctx, hipMemcpyAsync(img, ctx->manifold_img_host.p, sizeof(uint16_t) * (size_t)cells, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
    }
  }
  if (!accumulate) hipLaunchKernelGGL(k_manifold_fill, dim3((cells + 255) / 256), dim3(256), 0, st, img, cells);      // setTo(30000), :72
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  ManifoldGrid g;
  g.xSize = x_size; g.ySize = y_size;
  g.cx = (int)(x_size * 0.5); g.cy = (int)(y_size * 0.5);                      // :54-55
  g.ires = (float)(1. / (double)resolution);                                  // :56
  g.normalThreshold = normal_threshold;
  int* d_inside = ctx->merge_counts_dev;
  if (n > 0) {
    HIPCHK(ctx, hipMemsetAsync(d_inside, 0, sizeof(int) * (size_t)n, st), PWN_HIP_ERR_COPY);
    for (const Chunk& k : chunks) {
      int base = 0;
      for (int i = k.first; i < k.last; ++i) {
        ManifoldCloud& m = ctx->manifold_host.p[i];
        m.P3 = clouds[i]->d.P3; m.Nc = clouds[i]->d.Nc; m.n = clouds[i]->content.n; m.base = base; m.T = mat4_from(transforms + 16 * (size_t)i);
        base += m.n;
      }
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->manifold_dev.p, ctx->manifold_host.p, sizeof(ManifoldCloud) * (size_t)n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  }
  unsigned long long* const d_key[2] = { ctx->scene_k[0], ctx->scene_k[1] };
  int* const d_val[2] = { ctx->scene_i[0], ctx->scene_i[1] }; int* d_hist = ctx->scene_i[2]; int* d_sums = ctx->scene_i[3]; int* d_start = ctx->scene_i[4];
  int cellBits = 0;                                  // bits of the largest cell id, x_size * y_size (the cell of the points that make no event): at most 25,
                                                     // so at most four passes, all within the key's low word, below the flag (kManifoldBadBit)
  while ((cells >> cellBits) != 0) ++cellBits;
  for (const Chunk& k : chunks) {
    const int m = (int)k.points;
    if (m == 0) continue;
    hipLaunchKernelGGL(k_manifold_events, dim3((k.largest + 255) / 256, k.last - k.first), dim3(256), 0, st, (const ManifoldCloud*)(ctx->manifold_dev.p + k.first), g,
                       d_key[0], d_val[0], d_inside + k.first);
    // sorted by cell, stable: a cell's events stay in cloud order, then index order
    int s = 0;
    if (int rc = radix_sort(ctx, d_key, d_val, m, cellBits, d_hist, d_sums, &s)) return rc;
    HIPCHK(ctx, hipMemsetAsync(d_start, 0xFF, sizeof(int) * (size_t)cells, st), PWN_HIP_ERR_COPY);
    hipLaunchKernelGGL(k_manifold_starts, dim3((m + 255) / 256), dim3(256), 0, st, (const unsigned long long*)d_key[s], m, cells, d_start);
    hipLaunchKernelGGL(k_manifold_cells, dim3((cells + 3) / 4), dim3(256), 0, st, (const unsigned long long*)d_key[s], (const int*)d_val[s], m, cells, (const int*)d_start, img);
    HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  }
  if (img != image) HIPCHK(ctx, hipMemcpyAsync(ctx->manifold_img_host.p, img, sizeof(uint16_t) * (size_t)cells, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  if (inside && n > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->merge_counts_host.p, d_inside, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  if (img != image) std::memcpy(image, ctx->manifold_img_host.p, sizeof(uint16_t) * (size_t)cells);
  if (inside && n > 0) std::copy(ctx->merge_counts_host.p, ctx->merge_counts_host.p + n, inside);
  return PWN_HIP_OK;
}
// Test-only (include/pwn_hip_testing.h): the most points one chunk of pwn_hip_manifold_image holds; points <= 0 restores 2^25
int pwn_hip_debug_set_manifold_chunk(pwn_hip_ctx* ctx, int points) {
  if (!ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  ctx->manifold_chunk = (points <= 0 || points > kMaxCloudPoints) ? kMaxCloudPoints : points;
  return PWN_HIP_OK;
}

// VoxelCalculator::compute (voxelcalculator.cpp:15-73) with the intended ordering of the voxel keys (see pwn_scene_kernels.h).
// kept (optional, host) receives the original indices of the survivors in output order.
int pwn_hip_voxelize(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, float resolution, int* new_size, int* kept) {
  if (!ctx || !cloud || !(resolution > 0.f)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  cloud_changes(ctx, cloud);
  const int n = cloud->content.n;
  if (n == 0) { if (new_size) *new_size = 0; return PWN_HIP_OK; }
  CloudDev back; SceneBuffers sback;      // the second array set: the stable compaction / reordering writes there, then the two sets change places
  HIPCHK(ctx, cloud->own_back(back, sback), PWN_HIP_ERR_ALLOCATION);
  size_t table = 1024; while (table < 2 * (size_t)n) table <<= 1;
  const int nblocksSort = (n + kSortChunk - 1) / kSortChunk;
  if (int rc = scene_scratch(ctx, std::max(table, (size_t)256 * nblocksSort + 1024), std::max(table, (size_t)n))) return rc;
  int* d_first = ctx->scene_i[0]; int* d_slot = ctx->scene_i[1]; int* d_keep = ctx->scene_i[2]; int* d_offs = ctx->scene_i[3]; int* d_sums = ctx->scene_i[4];
  int* const d_idx[2] = { ctx->scene_i[5], ctx->scene_i[6] }; int* d_hist = ctx->scene_i[7];
  unsigned long long* d_table = ctx->scene_k[0]; unsigned long long* const d_key[2] = { ctx->scene_k[1], ctx->scene_k[2] };
  hipStream_t st = ctx->stream;
  const float inverseResolution = 1.0f / resolution;
  const int nb = (n + 255) / 256;
  int* d_fault = ctx->scene_total + 1;
  HIPCHK(ctx, hipMemsetAsync(d_table, 0xFF, table * 8, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(d_first, 0x7F, table * 4, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(d_fault, 0, sizeof(int), st), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_voxel_insert, dim3(nb), dim3(256), 0, st, cloud->d, n, inverseResolution, d_table, d_first, (unsigned)(table - 1), d_slot, d_fault);
  hipLaunchKernelGGL(k_voxel_survivors, dim3(nb), dim3(256), 0, st, n, (const int*)d_slot, (const int*)d_first, d_keep);
  if (int rc = exclusive_scan(ctx, d_keep, d_offs, n, d_sums, ctx->scene_total)) return rc;
  hipLaunchKernelGGL(k_voxel_records, dim3(nb), dim3(256), 0, st, cloud->d, n, inverseResolution, (const int*)d_keep, (const int*)d_offs, d_key[0], d_idx[0]);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  int hostv[2] = { 0, 0 };
  HIPCHK(ctx, hipMemcpyAsync(hostv, ctx->scene_total, 2 * sizeof(int), hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  if (hostv[1] != 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, hostv[1] == 1 ? "voxel index outside +-2^20 (or NaN point)" : "voxel table full");
  const int m = hostv[0];
  // the survivors sorted by their 63-bit voxel key (8 passes of 8 bits), stable -> lexicographic (ix, iy, iz) order
  int s = 0;
  if (int rc = radix_sort(ctx, d_key, d_idx, m, 64, d_hist, d_sums, &s)) return rc;
  const int* d_order = d_idx[s];
  const bool withGauss = cloud->sb.G && cloud->content.n_gauss == n;          // voxelcalculator.cpp:62-64
  if (m > 0) hipLaunchKernelGGL(k_voxel_gather, dim3((m + 255) / 256), dim3(256), 0, st, cloud->d, cloud->sb, back, sback, m, withGauss ? 1 : 0, d_order);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (int rc = cloud_edit(ctx, cloud, m, true)) return rc;      // edit: the host decides the new size
  cloud->content.set_gaussians(withGauss ? m : 0);
  if (kept && m > 0) HIPCHK(ctx, hipMemcpyAsync(kept, d_order, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  cloud->swap_sides();
  if (new_size) *new_size = m;
  return PWN_HIP_OK;
}

// Cloud::save (cloud.cpp:84-136).  Text records are the reference's, token for token (operator<< on floats).  Binary records keep the
// reference's object layout on x86-64 (Point 32 B, Normal 32 B, Stats 112 B: vptr, padding, data) with the non-data bytes zeroed.
int pwn_hip_cloud_save(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, const char* filename, const float T[16], int step, int binary) {
  if (!ctx || !c || !filename || !T || step <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  const int n = c->content.n;
  std::vector<float> P, Nm, St;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  if (int rc = cloud_fetch_records(ctx, c->d, n, P, Nm)) return rc;
  if (n > 0) {
    if (c->content.stats && c->d.St) { St.resize((size_t)n * 16); HIPCHK(ctx, hipMemcpy(St.data(), c->d.St, St.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY); }
  }
  std::ofstream os(filename);
  if (!os) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, std::string("cannot open ") + filename);
  os << "PWNCLOUD " << (size_t)n / (size_t)step << " " << (binary ? true : false) << std::endl;
  float tv[6]; t2v(mat4_from(T), tv);
  os << tv[0] << " " << tv[1] << " " << tv[2] << " " << tv[3] << " " << tv[4] << " " << tv[5] << " " << std::endl;
  for (int i = 0; i < n; i += step) {
    float S[16] = { 0.f };                           // Stats as a row/column-indexed 4x4 (column-major here); all zero for a cloud without Stats
    int npts = 0; float ev[3] = { 0.f, 0.f, 0.f };
    if (!St.empty()) stats_unpack(&St[(size_t)16 * i], S, ev, &npts);
    const float* p = &P[(size_t)4 * i]; const float* nm = &Nm[(size_t)4 * i];
    if (!binary) {
      os << "POINTWITHSTATS ";
      for (int k = 0; k < 3; ++k) os << p[k] << " ";
      for (int k = 0; k < 3; ++k) os << nm[k] << " ";
      for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) os << S[r + 4 * q] << " ";
      os << std::endl;
    } else {
      char rec[176]; std::memset(rec, 0, sizeof(rec));
      const float pw[4] = { p[0], p[1], p[2], 1.0f }, nw[4] = { nm[0], nm[1], nm[2], 0.0f };
      std::memcpy(rec + 16, pw, 16); std::memcpy(rec + 32 + 16, nw, 16);
      char* st = rec + 64;
      std::memcpy(st + 16, S, 64); std::memcpy(st + 80, &npts, 4); std::memcpy(st + 84, ev, 12);
      // Stats::_curvatureComputed / _curvature as DepthImageConverter::compute leaves them: cached where the stats calculator
      // evaluated curvature() (statscalculatorintegralimage.cpp:72), the Stats() defaults (false, 1.0f) where it skipped the pixel;
      // a cloud without Stats (uploaded) carries curvatures set by setCurvature()
      const bool cached = St.empty() || npts > 0;
      st[96] = cached ? 1 : 0; const float curv = cached ? p[3] : 1.0f; std::memcpy(st + 100, &curv, 4);
      os.write(rec, sizeof(rec));
    }
  }
  if (!os.good()) return fail(ctx, PWN_HIP_ERR_COPY, std::string("write error on ") + filename);
  return PWN_HIP_OK;
}
// Cloud::load (cloud.cpp:25-82): points, normals and Stats; the information matrices are not part of the format (they stay zero) and
// the curvature comes from the stored eigenvalues (binary) or is the Stats default (text: eigenvalues are not stored -> 0/(0+1e-9) = 0).
int pwn_hip_cloud_load(pwn_hip_ctx* ctx, pwn_hip_cloud* c, const char* filename, float T_out[16]) {
  if (!ctx || !c || !filename || !T_out) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  std::ifstream is(filename);
  if (!is) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, std::string("cannot open ") + filename);
  char buf[1024];
  is.getline(buf, 1024);
  std::istringstream ls(buf);
  std::string tag; size_t numPoints = 0; bool binary = false;
  ls >> tag;
  if (tag != "PWNCLOUD") return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "not a PWNCLOUD file");
  ls >> numPoints >> binary;
  if (numPoints > (size_t)c->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity smaller than the file's point count");
  is.getline(buf, 1024);
  std::istringstream lst(buf);
  float tv[6] = { 0, 0, 0, 0, 0, 0 };
  lst >> tv[0] >> tv[1] >> tv[2] >> tv[3] >> tv[4] >> tv[5];
  const Mat4 T = v2t(tv); std::memcpy(T_out, T.m, sizeof(T.m));
  const int n = (int)numPoints;
  std::vector<float> P((size_t)n * 4, 0.f), Nm((size_t)n * 4, 0.f), St = default_stats(n);
  size_t k = 0;
  while (k < (size_t)n && is.good()) {
    float S[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    float ev[3] = { 0.f, 0.f, 0.f }; int npts = 0; float curv = 0.f; bool haveCurv = false;
    float* p = &P[4 * k]; float* nm = &Nm[4 * k];
    if (!binary) {
      is.getline(buf, 1024);
      std::istringstream l2(buf);
      std::string s2; l2 >> s2;
      if (s2 != "POINTWITHSTATS") continue;
      for (int i = 0; i < 3 && l2; ++i) l2 >> p[i];
      for (int i = 0; i < 3 && l2; ++i) l2 >> nm[i];
      for (int r = 0; r < 4 && l2; ++r) for (int q = 0; q < 4 && l2; ++q) l2 >> S[r + 4 * q];
    } else {
      char rec[176];
      is.read(rec, sizeof(rec));
      std::memcpy(p, rec + 16, 12); std::memcpy(nm, rec + 32 + 16, 12);
      const char* st = rec + 64;
      std::memcpy(S, st + 16, 64); std::memcpy(&npts, st + 80, 4); std::memcpy(ev, st + 84, 12);
      haveCurv = st[96] != 0; std::memcpy(&curv, st + 100, 4);
    }
    if (!haveCurv) curv = (float)((double)ev[0] / ((double)(ev[0] + ev[1] + ev[2]) + 1e-9));     // stats.h:98-103
    p[3] = curv;
    const int cls = 0; std::memcpy(&nm[3], &cls, 4);
    stats_pack(S, ev, npts, &St[16 * k]);
    ++k;
  }
  const bool ok = is.good();
  // replace: points with Stats.  Cloud::load leaves both information-matrix vectors empty (cloud.cpp:25-82): zero matrices for every point.  The
  // class of the normal information matrix is derived from normal and curvature on the device, so a loaded cloud says "zero" with explicit planes.
  if (int rc = cloud_replace(ctx, c, true, true, nullptr)) return rc;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  if (n > 0) {
    if (int rc = cloud_store_records(ctx, c->d, n, P, Nm)) return rc;
    HIPCHK(ctx, hipMemcpy(c->d.St, St.data(), St.size() * 4, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemset(c->d.Om, 0, c->front.Om.cap * sizeof(float)), PWN_HIP_ERR_COPY);
  }
  HIPCHK(ctx, hipMemset(c->d.OmN, 0, (size_t)c->d.capacity * 9 * sizeof(float)), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpy(c->d.count, &n, sizeof(int), hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  cloud_commit(c, n);
  if (!ok) return fail(ctx, PWN_HIP_ERR_COPY, "read error / truncated PWNCLOUD file");
  return PWN_HIP_OK;
}

}  // extern "C"
