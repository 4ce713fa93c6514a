// pwn_hip_capi.hip -- implementation of include/pwn_hip.h: context, device clouds and the launch
// sequences that replace the reference's DepthImageConverterIntegralImage::compute
// (pwn_core/depthimageconverterintegralimage.cpp:15-55) and Aligner::align (pwn_core/aligner.cpp:49-125).
//
// Host code only orchestrates: every per-pixel / per-point / per-correspondence loop of the reference runs
// in a kernel of pwn_kernels.h, and the Gauss-Newton loop runs without host round trips (the 6x6 solve and
// the SE(3) update are a one-wave kernel).  There is no CPU fallback: without a HIP device every entry point
// returns PWN_HIP_ERR_NO_DEVICE.
#include <cstdlib>
#include "../../include/pwn_hip.h"
#include "../../include/pwn_hip_testing.h"
#include "pwn_buffers.h"
#include "pwn_kernels.h"
#include "pwn_scene_kernels.h"
#include "pwn_stats.h"
#include "pwn_consensus.h"
#include "pwn_track.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

using namespace pwnhip;

namespace {

thread_local std::string g_err = "";

struct StageAcc { float ms = 0.f; int launches = 0; };
struct EventRec { std::string stage; hipEvent_t a, b; };

// pwn_hip_convert_scaled_begin / _end: a helper context (streams and workspaces of its own) driven by a helper thread, so that a frame
// is converted next to whatever the caller runs on the context meanwhile
struct AsyncConvert {
  pwn_hip_ctx* helper = nullptr;           // default-priority streams: the tracker's look-ahead (a frame converted beside ONE alignment's short kernels)
  pwn_hip_ctx* helper_hi = nullptr;        // high-priority streams, created on first use: a frame converted beside a BATCH call (pwn_hip_convert_export_begin)
  pwn_hip_ctx* job_ctx = nullptr;          // the one the current job runs on
  std::thread worker;
  std::mutex m;
  std::condition_variable cv;
  bool has_job = false, done = true, quit = false;
  pwn_hip_converter_params p;
  const float* depth = nullptr; int rows = 0, cols = 0, step = 1; float max_depth_cov = 0.f;
  const uint16_t* raw = nullptr; float raw_scale = 0.f;      // pwn_hip_convert_export_begin: a raw uint16 frame instead of `depth`
  void* flat_dst = nullptr; size_t flat_bytes = 0, flat_written = 0;      // ... and the cloud's flat form written behind the conversion
  float job_ms = 0.f;                                        // wall time of the job on the helper thread (conversion + export, waits included)
  pwn_hip_cloud* cloud = nullptr;
  int rc = 0; std::string err;
};

// What an index image was made with.  Projecting a cloud returns the index image the converter kept for it exactly when the projector's key equals the
// image's (and the pose is the identity): the aligner's shortcut compares keys, so a field the projection depends on is added here and nowhere else.
struct IndexKey {
  int rows = 0, cols = 0; float K[9] = { 0 }; float minD = 0.f, maxD = 0.f;
  IndexKey() = default;
  IndexKey(int r, int c, const float* k, float mn, float mx) : rows(r), cols(c), minD(mn), maxD(mx) { std::memcpy(K, k, sizeof(K)); }
  bool operator==(const IndexKey& o) const { return rows == o.rows && cols == o.cols && minD == o.minD && maxD == o.maxD && std::memcmp(K, o.K, sizeof(K)) == 0; }
};
IndexKey index_key(const pwn_hip_converter_params* p, int rows, int cols) { return IndexKey(rows, cols, p->K, p->min_distance, p->max_distance); }
IndexKey index_key(const pwn_hip_aligner_params* p) { return IndexKey(p->rows, p->cols, p->K, p->min_distance, p->max_distance); }
// The pair whose images sit in workspace slot 0 after an alignment: its descriptor (pairs_host / pairs_dev entry), its clouds (the depth images are
// recomputed from their points) and the z-buffer epochs of its last reference projection and of its current projection
struct Slot0Pair {
  int pair = 0; const pwn_hip_cloud* ref_cloud = nullptr; const pwn_hip_cloud* cur_cloud = nullptr; unsigned ref_tag = kZ32Tag0, cur_tag = kZ32Tag0;
};
// The finder's images of the last alignment, as pwn_hip_align_images / pwn_hip_match_score read them.  Written by its own functions only: set()
// after a finished call, invalidate() by whatever touches slot 0 or the descriptors, drop_clouds() when one of its clouds changes or goes.
struct FinderImages : Slot0Pair {
  bool valid = false;
  AlignParams ap = {};                       // of the call (the images are ap.rows x ap.cols)
  // A single alignment whose current cloud carries its own index image (pwn_hip_cloud::idximg) does not project that cloud at all; its
  // z-buffer is filled in only when pwn_hip_align_images asks for the finder's current images (pwn_hip_match_score reads the depths off the cloud)
  bool cur_lazy = false;
  void invalidate() { valid = false; }
  void drop_clouds() { valid = false; ref_cloud = nullptr; cur_cloud = nullptr; }
  void set(const AlignParams& a, const Slot0Pair& s, bool is_valid, bool lazy) { Slot0Pair::operator=(s); ap = a; valid = is_valid; cur_lazy = lazy; }
  void cur_projected() { cur_lazy = false; }      // pwn_hip_align_images has made the projection the alignment skipped
};

// One side of a cloud's per-point arrays, and their only owner: the core arrays every cloud has, and three optional groups -- explicit normal
// information matrices (uploaded, imported and scene clouds), Stats (keep_stats conversions, scenes, loaded clouds), the sensor-noise Gaussians
// with their flags (scene stage).  The elements per point are written here and nowhere else; everything else names groups.
enum : unsigned { kArrCore = 1, kArrOmN = 2, kArrSt = 4, kArrGauss = 8 };
struct CloudArrays {
  DevBuf<float> P3; DevBuf<float4> Nc; DevBuf<float> Om, OmN, St; DevBuf<GaussD> G; DevBuf<int> Gf;
  // the arrays of the groups `which` for `cap` points; an array that is there stays as it is
  hipError_t ensure(unsigned which, size_t cap, int sym) {
    hipError_t e = hipSuccess;
    auto need = [&](unsigned group, auto& buf, size_t per_point) { if ((which & group) && e == hipSuccess) e = buf.ensure(cap * per_point); };
    need(kArrCore, P3, 3); need(kArrCore, Nc, 1); need(kArrCore, Om, 3 * (size_t)om_planes(sym));
    need(kArrOmN, OmN, 9); need(kArrSt, St, 16); need(kArrGauss, G, 1); need(kArrGauss, Gf, 1);
    return e;
  }
  // the groups this side holds anything of
  unsigned held() const { return ((P3 || Nc || Om) ? kArrCore : 0u) | (OmN ? kArrOmN : 0u) | (St ? kArrSt : 0u) | ((G || Gf) ? kArrGauss : 0u); }
  size_t core_bytes() const { return P3.cap * sizeof(float) + Nc.cap * sizeof(float4) + Om.cap * sizeof(float); }
  // The two sides change places after a compaction wrote the other one: the core arrays always, an optional group only where both sides hold it.  A side
  // without a group stays without: a scene cloud imported from a class-coded one has lost its front OmN and must not get the back's stale planes.
  void swap(CloudArrays& o) {
    std::swap(P3, o.P3); std::swap(Nc, o.Nc); std::swap(Om, o.Om);
    if (OmN && o.OmN) std::swap(OmN, o.OmN);
    if (St && o.St) std::swap(St, o.St);
    if (G && o.G) { std::swap(G, o.G); std::swap(Gf, o.Gf); }
  }
  void view(CloudDev& d, SceneBuffers& s) const { d.P3 = P3; d.Nc = Nc; d.Om = Om; d.OmN = OmN; d.St = St; s.G = G; s.Gf = Gf; }
};

// What a cloud's arrays hold at this moment.  The fields are assigned in this struct and nowhere else (tests/test_capi_cpu.py); its functions are
// called by the three transitions of a cloud's content -- cloud_replace, cloud_commit, cloud_edit -- by a conversion job that ends without a commit,
// or whose kernels wrote the Gaussians of the points they counted (commit_with_gaussians),
// and by the two setters' callers (the Gaussian calls, ensure_scene).  Everything else reads.
struct CloudContent {
  int n = 0;                     // points, as the host knows them (pwn_hip_cloud_size); the device keeps a word of its own (pwn_hip_cloud::count)
  bool stats = false;            // St holds the Stats of these points (St may be allocated while this is false: see pwn_hip_cloud::view)
  int n_gauss = 0;               // Cloud::gaussians().size(): the records [0, n_gauss) of G / Gf
  // idximg is what projecting these points with idx_key's projector under the identity pose gives (see pwn_hip_cloud::idximg).  Between the replace
  // and the commit of a conversion it is a promise: the fused step describes its pairs, shortcut included, before its conversions have run.
  bool idx_valid = false; IndexKey idx_key;
  void replace(bool keep_stats, const IndexKey* key, bool promised) { n = 0; stats = keep_stats; n_gauss = 0; idx_valid = promised; if (key) idx_key = *key; }
  void commit(int points) { n = points; }                                                        // a promised index key stands
  void commit(int points, const IndexKey& key) { n = points; idx_valid = true; idx_key = key; }  // the index image arrived with the points
  void commit_with_gaussians(int points) { n = points; n_gauss = points; }                       // ... and a sensor-noise Gaussian with every point
  void withdraw() { n = 0; stats = false; n_gauss = 0; idx_valid = false; }                      // the new content did not arrive: an empty cloud
  void edit(int points) { n = points; idx_valid = false; }
  void set_gaussians(int count) { n_gauss = count; }
  void set_stats() { stats = true; }
};
// What a kernel gets of a cloud it only reads: the by-value records with St only where the content has Stats, the size, and the Gaussians a
// consumer may read -- `gauss` of the vector, point_gauss() of them for the cloud's points
struct CloudView { CloudDev d; SceneBuffers sb; int n, gauss; int point_gauss() const { return std::min(gauss, n); } };

}  // namespace

struct pwn_hip_cloud {
  // The owners: the front arrays, the second set the scene stage's compactions / reorderings write before the two change places
  // (pwn_scene_capi.h), and the size word.  `delete` frees them all.
  CloudArrays front, back; DevBuf<int> count;
  // What kernels and descriptors receive by value: the front's pointers beside the cloud's scalar fields, which live here and nowhere else
  // (capacity, omSym, omN, clsThr).  The pointers are refreshed by the three functions below that change what the front owns, and by nothing else.
  CloudDev d = {};
  SceneBuffers sb = { nullptr, nullptr };
  void refresh() { front.view(d, sb); d.count = count; }
  hipError_t own(unsigned which) {
    hipError_t e = count.ensure(1);
    if (e == hipSuccess) e = front.ensure(which, (size_t)d.capacity, d.omSym);
    refresh();
    return e;
  }
  void drop_omega_n() { front.OmN.release(); refresh(); }      // for a caller that knows no stream still reads the planes
  void swap_sides() { front.swap(back); refresh(); }
  // the back set gets the core arrays and whatever optional groups the front holds; bd / bs: its views
  hipError_t own_back(CloudDev& bd, SceneBuffers& bs) {
    const hipError_t e = back.ensure(kArrCore | front.held(), (size_t)d.capacity, d.omSym);
    bd = d; back.view(bd, bs);
    return e;
  }
  // the whole core, the size word and nothing else (but the index image): such a cloud may retire into the context's pool
  bool plain() const { return front.P3 && front.Nc && front.Om && count && front.held() == kArrCore && back.held() == 0; }
  size_t core_bytes() const { return front.core_bytes() + (idximg.cap + stripoff.cap) * sizeof(int); }      // what the pool's budget counts
  // What the arrays mean right now; the owners above say nothing about that
  CloudContent content;
  CloudView view() const { CloudView v = { d, sb, content.n, sb.G ? content.n_gauss : 0 }; if (!content.stats) v.d.St = nullptr; return v; }
  // The index image DepthImageConverter::compute produced for this cloud (written here directly instead of into a workspace); what it was
  // made from is content.idx_key.  Projecting a cloud with the very projector it was unprojected with (same K, size, range, identity pose)
  // returns this image: every point falls back on its own pixel (the round trip moves it by < 0.01 pixel and its depth not at all), so batch
  // alignments take it as the current index image and skip that projection.  Anything that changes the points invalidates it.
  DevBuf<int> idximg;
  // The strip offsets that index image was counted from: [rows][cols / 64] words, entry (r, s) = the index of the first valid pixel of columns
  // [64 s, 64 s + 64) of row r.  The converter's single-pass front end writes them here (FrameDesc::rowoff) instead of into its workspace when
  // cols is a multiple of 64 and the cloud receives its own index image; with them an index is a table word plus a rank among 64 depths
  // (CurDepthSrc::strips).  stripoff_filled: the conversion that is making (or made) the index image fills the table -- set by convert_prepare,
  // taken back by a launch that runs the three-kernel front end, cleared by every replace.  The table is no part of the flat form: an imported
  // cloud has none.
  DevBuf<int> stripoff; bool stripoff_filled = false;
  bool strip_table() const { return content.idx_valid && stripoff_filled && stripoff; }      // valid exactly as long as the index image it belongs to
  const pwn_hip_ctx* owner = nullptr;    // the context it was created on (pwn_hip_project_merge_batch refuses another context's cloud)
};

struct pwn_hip_tracker;
void tracker_orphan(pwn_hip_tracker* tr);      // pwn_track_capi.h: the context goes, the handle stays valid for pwn_hip_tracker_destroy alone
struct pwn_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  hipStream_t stream2 = nullptr;           // batch calls deal sub-batches round-robin over `stream`, `stream2` and `extra` (own streams only)
  hipStream_t extra[2] = { nullptr, nullptr };
  hipEvent_t fork_ev = nullptr, join_ev = nullptr, join_extra[2] = { nullptr, nullptr };
  hipStream_t copy_stream = nullptr;       // host frames of a batch call are copied on their own stream, one sub-batch ahead of the kernels
  std::vector<hipEvent_t> sync_events;     // ordering events of that hand-over (copied[k], converted[k]); grown on demand
  hipEvent_t copy_ev = nullptr;            // pwn_hip_copy_async: the next call that reads frames waits for the copies issued so far
  hipEvent_t foreign_ev = nullptr;         // pwn_hip_ctx_wait_stream: marks the caller's stream
  bool copy_pending = false;
  int max_rows = 0, max_cols = 0, max_batch = 0;
  int num_cus = 256;                       // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  size_t N = 0;
  int sub_frames = 64, sub_pairs = 64;
  int concurrency = 4;
  int omega_sym = 1;                       // pwn_hip_ctx_set_omega_storage: storage of the point information matrices of clouds created from now on (default: sym6)
  // convert workspaces (per slot)
  DevBuf<float> depth_ws; DevBuf<int> index_ws, interval_ws; DevBuf<float> integral_ws; DevBuf<int> rowoff_ws;
  DevBuf<uint16_t> raw_ws;
  // the *_scaled batch calls (allocated by the first of them): the down-sampled frame of every slot, which its front end reads, and the box
  // kernel's descriptors (one per frame of a call)
  DevBuf<float> scaled_ws; DevBuf<ScaleDesc> scale_dev; HostBuf<ScaleDesc> scale_host;
  // pwn_hip_convert_batch_ex with Gaussians (allocated by the first such call): the Gaussian arrays of every frame's cloud, beside frames_dev
  DevBuf<SceneBuffers> gauss_dev; HostBuf<SceneBuffers> gauss_host;
  int gauss_staged = kGaussStagedDefault;                    // pwn_hip_debug_set_gaussian_stores (test hook): how k_gaussians_batch stores its records
  DevBuf<unsigned long long> carry_ws; size_t carry_slot = 0; size_t rowoff_slot = 0;   // single-pass integral image: hand-over words, strip offsets
  unsigned convert_epoch = 0; DevBuf<int> fault_dev;
  int last_convert_fault = 0;              // fault word of the last converter launch of the CURRENT call (1 = a bounded poll timed out); reset when a call starts
  int spin_limit = kSpinLimit; int dbg_withhold = -1;        // pwn_hip_debug_withhold_carry (test hook)
  int dbg_withhold_once = 0;                                 // the hook switches itself off after the first launch that timed out
  int convert_retries = 0;                                   // conversions repeated after a hand-over time-out (pwn_hip_debug_convert_retries)
  // align workspaces (per slot)
  DevBuf<unsigned long long> zref_ws;           // 64-bit z-buffer of the stand-alone projection and of Merger::merge (one image)
  DevBuf<unsigned> z32ref_ws, z32cur_ws;        // the aligner's 32-bit z-buffers (tag | index), one image per slot
  DevBuf<int> curidx_ws; DevBuf<double> partials_ws; DevBuf<PairState> state_ws;
  int nblocks_max = 0;
  // descriptors (one entry per frame / pair of a batch call; grown on demand)
  int desc_cap = 0;
  DevBuf<FrameDesc> frames_dev; DevBuf<PairDesc> pairs_dev; DevBuf<RawDesc> raw_dev; DevBuf<int> counts_dev;
  HostBuf<FrameDesc> frames_host; HostBuf<PairDesc> pairs_host; HostBuf<RawDesc> raw_host; HostBuf<PairState> state_host; HostBuf<int> counts_host;
  DevBuf<MatchAcc> match_dev; HostBuf<MatchAcc> match_host;
  DevBuf<SolveOut> stats_dev; HostBuf<SolveOut> stats_host;
  DevBuf<PairStats> pairstats_dev; HostBuf<PairStats> pairstats_host;      // k_pair_statistics: Aligner::_computeStatistics' result per pair
  // misc scratch
  DevBuf<SolveOut> solve_dev; DevBuf<int> counters_dev; DevBuf<int2> corr_ws; DevBuf<int> scratch_count;
  DevBuf<float> io_ws;      // N*16 floats staging for cloud up/download
  FinderImages img;                         // images of the last alignment
  int index_shortcut = 1;                   // pwn_hip_debug_set_index_shortcut (test hook): 0 = always project
  StopRule stop = { 0, 0.f, 0.f, 0 };       // pwn_hip_ctx_set_convergence: when a pair's loop ends on the device before outer_iterations (off by default)
  // pwn_hip_last_align_steps: the pairs of the last alignment call, and whether their final states are in state_host already (a call that
  // returned records only leaves them in state_ws until somebody asks)
  int last_pairs = 0; bool last_states_on_host = false;
  // z-buffer epoch tags are handed out in descending order ACROSS batch calls (a smaller tag wins, so whatever earlier calls left in
  // the buffers reads as empty): the buffers are cleared only when the 12-bit tag space is used up, not once per alignment
  unsigned ztag_next = 0;                   // 64-bit buffer (scene stage)
  unsigned z32tag_next = 0;                 // 32-bit buffers (aligner)
  std::string err;
  bool profiling = false;
  std::map<std::string, StageAcc> stages;
  std::vector<EventRec> pending;
  std::vector<hipEvent_t> event_pool;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  // scene-stage scratch (grown on demand)
  DevBuf<int> scene_i[8];
  DevBuf<unsigned long long> scene_k[3];
  DevBuf<int> scene_total;
  // Retired clouds kept for reuse: pwn_hip_cloud_create / _destroy are called once per frame by makeCloud-style callers (the reference
  // returns a `new Cloud` per depth image, pwn_matcher_base.cpp:77-85), and hipMalloc / hipFree of the point arrays cost more than the
  // conversion of a frame.  Bounded by kCloudPoolBytes.
  std::vector<pwn_hip_cloud*> cloud_pool; size_t cloud_pool_bytes = 0;
  AsyncConvert* async = nullptr;           // pwn_hip_convert_scaled_begin: created on first use
  HostBuf<char> flat_hdr_host;             // page-locked staging of a flat cloud's 256-byte header (pwn_hip_cloud_export / _import)
  DevBuf<float> records_ws;                              // result records of a batch on their way to host memory (k_pack_records)
  DevBuf<int> ids_dev;                                   // the caller's pair ids of those records
  // pwn_hip_align_batch_priors: the call's prior list (pair i: [first[i], first[i + 1])), the device copies of the priors and one record of
  // terms per prior (k_prior_terms); they grow with the call
  DevBuf<int> prior_first_dev; HostBuf<int> prior_first_host;
  DevBuf<PriorHost> priors_dev; HostBuf<PriorHost> priors_host;
  DevBuf<PriorTerms> prior_terms_dev;
  // Projection fault path (z32_settle): a page-locked word the projection kernels raise when a pixel's settle loop gave up; the call is then
  // repeated with the two-pass projection (k_project_robust) and its depth images (allocated on first use)
  void (*enqueued_cb)(void*) = nullptr; void* enqueued_user = nullptr;      // pwn_hip_ctx_set_enqueued_callback
  HostBuf<int> align_fault_host;
  DevBuf<unsigned> zdepth_ws;
  int settle_guard = kSettleGuard;                       // pwn_hip_debug_set_settle_guard (test hook)
  int last_align_fault = 0;                              // the last alignment call ended with the fault word raised
  int host_waits = 0;                                    // waits of the calling thread for one of the context's streams so far (pwn_hip_debug_host_waits)
  int projection_fallbacks = 0;                          // calls repeated with the two-pass projection so far (pwn_hip_debug_projection_fallbacks)
  // the frames of a step's current clouds, per pair (CurDepthSrc::raw), and how many sub-batches of the last batch alignment ran the fused pass
  // on them (pwn_hip_debug_cur_depth_sub_batches)
  DevBuf<const uint16_t*> cur_raw_dev; HostBuf<const uint16_t*> cur_raw_host;
  int cur_depth_subs = 0;
  // the strip offsets of those clouds, per pair (CurDepthSrc::strips), and how many of those sub-batches ranked the current index from them
  // (pwn_hip_debug_strip_index_sub_batches)
  DevBuf<const int*> cur_strip_dev; HostBuf<const int*> cur_strip_host;
  int strip_index_subs = 0;
  // The merged closure (pwn_hip_merge_depth_images, pwn_hip_project_merge_batch), allocated by the first such call: the staging images of
  // host-side `merged` / `weights` ([0, N) and [N, 2N)) and behind them merge_planes = min(max_batch, kMergePlanesMax) depth planes of N words;
  // a call with more images runs in chunks of that many.  Per image of a call: its plane's address, its cloud, its projector matrix; the
  // counters (overlap[n], then points) on their way to the host.
  DevBuf<float> merge_ws; int merge_planes = 0;
  DevBuf<const float*> plane_ptrs_dev; HostBuf<const float*> plane_ptrs_host;
  DevBuf<DepthCloudDesc> depth_clouds_dev; HostBuf<DepthCloudDesc> depth_clouds_host;
  DevBuf<Mat4> krt_dev; HostBuf<Mat4> krt_host;
  DevBuf<int> merge_counts_dev; HostBuf<int> merge_counts_host;
  DevBuf<float> cloud_weights_ws;            // pwn_hip_merge_clouds: the staging of host-side `weights` (the total cloud's capacity)
  // pwn_hip_manifold_image: one descriptor per cloud of a call, the staging of a host-side `image`, and the most points a chunk of clouds holds
  // (pwn_hip_debug_set_manifold_chunk lowers it)
  DevBuf<ManifoldCloud> manifold_dev; HostBuf<ManifoldCloud> manifold_host;
  DevBuf<uint16_t> manifold_img_dev; HostBuf<uint16_t> manifold_img_host;
  int manifold_chunk = kMaxCloudPoints;
  // pwn_hip_scene_step (allocated by the first such call): the rendering of the scene, the step record on the device and its page-locked copy
  DevBuf<float> scene_depth_ws; DevBuf<SceneStepRecord> step_dev; HostBuf<SceneStepRecord> step_host;
  // pwn_hip_validate_relations (they grow with the call): per relation its four transforms, the isIn bit matrix, the column counts and behind
  // them the empty-column word, the staging of the call's host-side arrays, and the page-locked copy of the empty-column word
  DevBuf<ConsensusRel> consensus_rel; DevBuf<unsigned long long> consensus_bits; DevBuf<int> consensus_counts;
  DevBuf<char> consensus_stage; HostBuf<int> consensus_flag_host;
  // the multi-stream trackers created on the context (pwn_hip_tracker_create): their clouds and device records go with the context; a handle that outlives it is only good for pwn_hip_tracker_destroy
  std::vector<pwn_hip_tracker*> trackers;
};

namespace {

constexpr size_t kCloudPoolBytes = 1ull << 30;

// What the aligner's launches for one sub-batch share: the call's parameters and grid (nb workgroups per pair; sym: storage of the current clouds' point
// information matrices, CloudDev::omSym, the same for every pair), the m consecutive pair descriptors, their stream, and -- when the call runs the
// two-pass projection, else nullptr -- the depth images of their workspace slots (contiguous, ctx->N words each)
// cd: the depth source of the pairs' current side (CurDepthSrc, raw already that of the launch's first pair), nullptr = the stored points
struct PairLaunch { const AlignParams* ap; int nb, sym; int m; hipStream_t st; const PairDesc* pr; unsigned* zd; const CurDepthSrc* cd; };
// the fused correspondence + linearize pass: the throughput shape, or the latency shape (same sums bit for bit, see k_corr_linearize_lat)
// when all workgroups of the launch find a CU of their own -- its 1024-thread workgroups fit one per CU, a second round costs more than
// the shape saves: one VGA pair is 150 workgroups, two pairs or one 1280x960 pair are not worth it on 256 CUs
bool latency_shape(const pwn_hip_ctx* ctx, int nb, int m) { return (long long)nb * m <= ctx->num_cus; }
// The depth source is a trade of bytes, so it belongs to the throughput shape: the latency shape keeps the stored points.
template <bool SAME_T, bool FULL_H, bool SYM>
void launch_corr_linearize_s(const pwn_hip_ctx* ctx, const PairLaunch& L, unsigned tag, int usePrevTc, int ownRef) {
  if (latency_shape(ctx, L.nb, L.m)) hipLaunchKernelGGL((k_corr_linearize_lat<SAME_T, FULL_H, SYM>), dim3(L.nb, L.m), dim3(kLatBlock), 0, L.st, L.pr, *L.ap, tag, usePrevTc, ownRef);
  else if (L.cd && L.cd->strips) hipLaunchKernelGGL((k_corr_linearize<SAME_T, FULL_H, SYM, kPixPerThread, true, true>), dim3(L.nb, L.m), dim3(kAlignBlock), 0, L.st, L.pr, *L.ap, tag, usePrevTc, ownRef, *L.cd);
  else if (L.cd) hipLaunchKernelGGL((k_corr_linearize<SAME_T, FULL_H, SYM, kPixPerThread, true>),dim3(L.nb, L.m), dim3(kAlignBlock), 0, L.st, L.pr, *L.ap, tag, usePrevTc, ownRef, *L.cd);
  else hipLaunchKernelGGL((k_corr_linearize<SAME_T, FULL_H, SYM>), dim3(L.nb, L.m), dim3(kAlignBlock), 0, L.st, L.pr, *L.ap, tag, usePrevTc, ownRef, NoCurDepthSrc());
}
template <bool SAME_T, bool FULL_H>
void launch_corr_linearize(const pwn_hip_ctx* ctx, const PairLaunch& L, unsigned tag, int usePrevTc, int ownRef) {
  if (L.sym) launch_corr_linearize_s<SAME_T, FULL_H, true>(ctx, L, tag, usePrevTc, ownRef);
  else launch_corr_linearize_s<SAME_T, FULL_H, false>(ctx, L, tag, usePrevTc, ownRef);
}

// every wait of the calling thread for a stream goes through here, so that a test can count the waits of a call
hipError_t host_wait(pwn_hip_ctx* ctx, hipStream_t st) { if (ctx) ++ctx->host_waits; return hipStreamSynchronize(st); }
int fail(pwn_hip_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}
// The finder's depth images of the last alignment are recomputed from the clouds' points (the z-buffer keeps indices only): anything
// that changes or frees one of those clouds ends the validity of pwn_hip_align_images / pwn_hip_match_score for that alignment.
void cloud_changes(pwn_hip_ctx* ctx, const pwn_hip_cloud* c) {
  if (ctx && c && (c == ctx->img.ref_cloud || c == ctx->img.cur_cloud)) ctx->img.drop_clouds();
}
#define HIPCHK(ctx, call, code)                                                                               \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) return fail(ctx, code, std::string(#call) + ": " + hipGetErrorString(e_));           \
  } while (0)

// projection of one cloud of each of the launch's pairs (which: 0 = reference, 1 = current; capacity: the largest of those clouds): four
// points per thread when the launch is large
constexpr int kProjectPPT = 4;
int launch_project(pwn_hip_ctx* ctx, const PairLaunch& L, int capacity, int which, unsigned tag) {
  if (L.zd) {
    HIPCHK(ctx, hipMemsetAsync(L.zd, 0xFF, (size_t)L.m * ctx->N * sizeof(unsigned), L.st), PWN_HIP_ERR_COPY);
    for (int pass = 0; pass < 2; ++pass)
      hipLaunchKernelGGL(k_project_robust, dim3((capacity + 255) / 256, L.m), dim3(256), 0, L.st, L.pr, *L.ap, which, tag, pass);
    return PWN_HIP_OK;
  }
  if (L.m >= 8) hipLaunchKernelGGL((k_project<kProjectPPT>), dim3((capacity + 256 * kProjectPPT - 1) / (256 * kProjectPPT), L.m), dim3(256), 0, L.st, L.pr, *L.ap, which, tag);
  else hipLaunchKernelGGL((k_project<1>), dim3((capacity + 255) / 256, L.m), dim3(256), 0, L.st, L.pr, *L.ap, which, tag);
  return PWN_HIP_OK;
}
// the current clouds projected with epoch `tag` and resolved into the pairs' current index images
int launch_project_cur(pwn_hip_ctx* ctx, const PairLaunch& L, int capacity, unsigned tag) {
  if (int rc = launch_project(ctx, L, capacity, 1, tag)) return rc;
  const int N = L.ap->rows * L.ap->cols;
  hipLaunchKernelGGL(k_resolve_cur, dim3(std::min((N + 255) / 256, 1024), L.m), dim3(256), 0, L.st, L.pr, N, tag);
  return PWN_HIP_OK;
}
// Aligner::_computeStatistics' extra Linearizer::update: the finder's correspondences of the last outer iteration (epoch lastRefTag, tests with
// that iteration's transform) re-linearized at the final transform with the full H (aligner.cpp:165-170), and its sums reduced into out[0..m)
void launch_statistics(const pwn_hip_ctx* ctx, const PairLaunch& L, unsigned lastRefTag, SolveOut* out) {
  launch_corr_linearize<false, true>(ctx, L, lastRefTag, 1, 0);
  hipLaunchKernelGGL(k_reduce_pairs, dim3(L.m), dim3(256), 0, L.st, L.pr, L.nb, out);
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}
// copy helper: any combination of host/device
hipError_t copy_any(void* dst, const void* src, size_t bytes, hipStream_t s) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s);
}

// device-to-device section copies of the flat cloud: a kernel (hipMemcpyAsync between device buffers is a blit kernel of the runtime's with a
// launch of its own per call: 0.3 ms per 17 MB cloud measured, against ~10 us); sizes and offsets are multiples of 4 bytes.
// The grid is SMALL on purpose (at most kCopyBlocks workgroups, four independent 16-byte accesses in flight per thread: ~2 TB/s alone, a 5 MB
// section in a few microseconds): these copies run beside a batch alignment (export in the look-ahead job, import on a second context), where a
// grid that fills the device (2048 workgroups until round 6) displaced the batch's own workgroups for ~80 us per section -- measured as +2.5 % on the
// sum of the batch's kernel times for 0.25 % more bytes.
constexpr unsigned kCopyBlocks = 96;
template <typename V> __global__ void __launch_bounds__(256) k_copy_words(const V* __restrict__ src, V* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const V a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
  }
  for (; i < n; i += stride) dst[i] = src[i];
}
hipError_t copy_section(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return hipSuccess;
  if (!is_device_ptr(dst) || !is_device_ptr(src) || (bytes & 3) || (((uintptr_t)dst | (uintptr_t)src) & 3)) return copy_any(dst, src, bytes, st);
  if (((((uintptr_t)dst | (uintptr_t)src) | bytes) & 15) == 0) {
    const size_t n = bytes / 16;
    hipLaunchKernelGGL(k_copy_words<uint4>, dim3((unsigned)std::min<size_t>((n + 1023) / 1024, kCopyBlocks)), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, n);
  } else {
    const size_t n = bytes / 4;
    hipLaunchKernelGGL(k_copy_words<unsigned>, dim3((unsigned)std::min<size_t>((n + 1023) / 1024, 2 * kCopyBlocks)), dim3(256), 0, st, (const unsigned*)src, (unsigned*)dst, n);
  }
  return hipGetLastError();
}

hipEvent_t get_event(pwn_hip_ctx* ctx) {
  if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
  // timing-only events: no system-scope fence (no cache write-back / invalidate between the kernels they bracket)
  hipEvent_t e; (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence); return e;
}
struct StageTimer {
  pwn_hip_ctx* ctx; EventRec rec; bool on; hipStream_t st;
  StageTimer(pwn_hip_ctx* c, const char* stage, hipStream_t s = nullptr) : ctx(c), on(c->profiling), st(s ? s : c->stream) {
    if (on) { rec.stage = stage; rec.a = get_event(ctx); rec.b = get_event(ctx); (void)hipEventRecord(rec.a, st); }
  }
  ~StageTimer() { if (on) { (void)hipEventRecord(rec.b, st); ctx->pending.push_back(rec); } }
};
// Two-stream mode: only with the context's own streams and when the workspaces hold two sub-batches.
struct StreamPlan {
  int sub; int ns; hipStream_t s[4];
  bool dual() const { return ns > 1; }
  hipStream_t stream(int k) const { return s[k % ns]; }
  int slot0(int k) const { return (k % ns) * sub; }
};
StreamPlan make_plan(pwn_hip_ctx* ctx, int want_sub, int n) {
  StreamPlan p;
  p.sub = std::max(1, std::min(want_sub, ctx->max_batch));
  // A batch is cut into a multiple of `streams` sub-batches of equal size (not larger than asked for), so that no stream idles while the other
  // works: the short dependent kernels of one sub-batch (projection, 6x6 step) fill the gaps of the other's large ones.  Measured on MI355X
  // (one-submission step, two streams): 64 VGA pairs as 2 x 32 instead of 1 x 64: 11 340 -> 12 170 alignments/s; 32 pairs as 2 x 16: 10 620 ->
  // 11 440; 32 pairs of 1280x960 as 2 x 16: 2 900 -> 3 090 (docs/experiments.md, round 4).  A call is only cut when every part keeps at least 16
  // items (the converter's single-pass kernels start there: kSinglePassMinFrames); smaller calls stay one launch sequence.
  if (ctx->stream == ctx->own_stream && ctx->stream2 && ctx->concurrency >= 2) {
    const int kmax = std::min(std::min(ctx->concurrency, 4), (!ctx->extra[0] ? 2 : (!ctx->extra[1] ? 3 : 4)));
    for (int k = kmax; k >= 2; --k) {      // as many streams as leave every part 16 items
      const int nsub_even = k * ((n + k * p.sub - 1) / (k * p.sub));
      if (nsub_even > 0 && n / nsub_even >= 16) { p.sub = (n + nsub_even - 1) / nsub_even; break; }
    }
  }
  const int nsub = (n + p.sub - 1) / p.sub;
  int ns = 1;
  if (ctx->stream == ctx->own_stream && ctx->stream2)
    ns = std::max(1, std::min(std::min(ctx->concurrency, 4), std::min(nsub, ctx->max_batch / p.sub)));
  if (ns > 2 && (!ctx->extra[0] || (ns > 3 && !ctx->extra[1]))) ns = 2;
  p.ns = ns;
  p.s[0] = ctx->stream; p.s[1] = ctx->stream2; p.s[2] = ctx->extra[0]; p.s[3] = ctx->extra[1];
  return p;
}
int plan_fork(pwn_hip_ctx* ctx, const StreamPlan& p) {      // the other streams start after everything enqueued so far on `stream`
  if (!p.dual()) return PWN_HIP_OK;
  HIPCHK(ctx, hipEventRecord(ctx->fork_ev, p.s[0]), PWN_HIP_ERR_LAUNCH);
  for (int k = 1; k < p.ns; ++k) HIPCHK(ctx, hipStreamWaitEvent(p.s[k], ctx->fork_ev, 0), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int plan_join(pwn_hip_ctx* ctx, const StreamPlan& p) {      // `stream` continues after the other streams' work
  if (!p.dual()) return PWN_HIP_OK;
  for (int k = 1; k < p.ns; ++k) {
    hipEvent_t ev = k == 1 ? ctx->join_ev : ctx->join_extra[k - 2];
    HIPCHK(ctx, hipEventRecord(ev, p.s[k]), PWN_HIP_ERR_LAUNCH);
    HIPCHK(ctx, hipStreamWaitEvent(p.s[0], ev, 0), PWN_HIP_ERR_LAUNCH);
  }
  return PWN_HIP_OK;
}
// pwn_hip_copy_async: everything queued on the context's stream from here on runs after the copies issued so far (the other streams of a
// batch call fork from that stream)
int absorb_copies(pwn_hip_ctx* ctx) {
  if (!ctx->copy_pending) return PWN_HIP_OK;
  HIPCHK(ctx, hipEventRecord(ctx->copy_ev, ctx->copy_stream), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->copy_ev, 0), PWN_HIP_ERR_LAUNCH);
  ctx->copy_pending = false;
  return PWN_HIP_OK;
}
void collect_stage_times(pwn_hip_ctx* ctx) {
  for (auto& r : ctx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { auto& s = ctx->stages[r.stage]; s.ms += ms; s.launches += 1; }
    ctx->event_pool.push_back(r.a); ctx->event_pool.push_back(r.b);
  }
  ctx->pending.clear();
}

Mat4 forced(const float* T) { Mat4 m = mat4_from(T); set_last_row(m); return m; }
bool is_identity(const Mat4& m) { const Mat4 I = mat4_identity(); for (int i = 0; i < 16; ++i) if (m.m[i] != I.m[i]) return false; return true; }

ConvertParams make_convert_params(const pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* T, int rows, int cols, int keep_stats) {
  ConvertParams cp;
  cp.spinLimit = ctx ? ctx->spin_limit : kSpinLimit; cp.dbgWithhold = ctx ? ctx->dbg_withhold : -1;
  cp.rows = rows; cp.cols = cols;
  const Mat3 K = mat3_from(p->K);
  Mat4 KRt; Mat3 iK;
  projector_matrices(K, T ? mat4_from(T) : mat4_identity(), KRt, cp.iKRt, iK);
  interval_scale(K, p->world_radius, cp.ivx, cp.ivy);
  cp.minD = p->min_distance; cp.maxD = p->max_distance;
  cp.minRadius = p->min_image_radius; cp.maxRadius = p->max_image_radius; cp.minPoints = p->min_points;
  cp.statsCurvThr = p->stats_curvature_threshold;
  cp.pointInfoCurvThr = p->point_info_curvature_threshold; cp.normalInfoCurvThr = p->normal_info_curvature_threshold;
  for (int i = 0; i < 3; ++i) { cp.pFlat[i] = p->point_flat_diag[i]; cp.pNonFlat[i] = p->point_nonflat_diag[i]; }
  cp.offset = forced(p->sensor_offset);
  cp.hasOffset = is_identity(cp.offset) ? 0 : 1;
  cp.keepStats = keep_stats;
  cp.lean = 0;
  cp.omSym = 0;        // set per call from the clouds being written (convert_batch_impl)
  return cp;
}
// T * Omega * T^t of a row-major 3x3 under the rotation of m, in place (informationmatrix.h:111-121)
void transform_omega(const Mat4& m, float om[9]) {
  float t1[9], o2[9];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) t1[3 * i + j] = dot3seq(m(i,0), om[0 + j], m(i,1), om[3 + j], m(i,2), om[6 + j]);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o2[3 * i + j] = dot3seq(t1[3 * i], m(j,0), t1[3 * i + 1], m(j,1), t1[3 * i + 2], m(j,2));
  std::memcpy(om, o2, sizeof(o2));
}
// The two class matrices that stand for a cloud's normal information matrices where it keeps no explicit planes (CloudDev::omN, clsThr)
struct OmegaNClasses { float omN[2][9]; float clsThr; };
// ... of a conversion: the calculator's diagonals after Cloud::transformInPlace(sensorOffset)
OmegaNClasses make_omega_n_classes(const pwn_hip_converter_params* p) {
  OmegaNClasses o;
  const Mat4 m = forced(p->sensor_offset);
  const bool ident = is_identity(m);
  for (int c = 0; c < 2; ++c) {
    const float* dg = c == 0 ? p->normal_flat_diag : p->normal_nonflat_diag;
    const float om[9] = { dg[0], 0, 0, 0, dg[1], 0, 0, 0, dg[2] };
    std::memcpy(o.omN[c], om, sizeof(om));
    if (!ident) transform_omega(m, o.omN[c]);
  }
  o.clsThr = p->normal_info_curvature_threshold;      // what normal_class() needs to tell flat from non-flat
  return o;
}
// Host staging in the records the rest of the host code was written for: P = (x, y, z, curvature), Nm = (nx, ny, nz, class word), n
// points each; the device keeps 12-byte points and (normal, curvature) records (pwn_kernels.h).
int cloud_fetch_records(pwn_hip_ctx* ctx, const CloudDev& d, int n, std::vector<float>& P, std::vector<float>& Nm) {
  std::vector<float> p3((size_t)n * 3), nc((size_t)n * 4);
  if (n > 0) {
    HIPCHK(ctx, hipMemcpy(p3.data(), d.P3, p3.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemcpy(nc.data(), d.Nc, nc.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
  }
  P.resize((size_t)n * 4); Nm.resize((size_t)n * 4);
  for (int i = 0; i < n; ++i) {
    P[4 * i] = p3[3 * i]; P[4 * i + 1] = p3[3 * i + 1]; P[4 * i + 2] = p3[3 * i + 2]; P[4 * i + 3] = nc[4 * i + 3];
    Nm[4 * i] = nc[4 * i]; Nm[4 * i + 1] = nc[4 * i + 1]; Nm[4 * i + 2] = nc[4 * i + 2];
    const int cls = normal_class(nc[4 * i], nc[4 * i + 1], nc[4 * i + 2], nc[4 * i + 3], d.clsThr);
    std::memcpy(&Nm[4 * i + 3], &cls, 4);
  }
  return PWN_HIP_OK;
}
int cloud_store_records(pwn_hip_ctx* ctx, const CloudDev& d, int n, const std::vector<float>& P, const std::vector<float>& Nm) {
  if (n <= 0) return PWN_HIP_OK;
  std::vector<float> p3((size_t)n * 3), nc((size_t)n * 4);
  for (int i = 0; i < n; ++i) {
    p3[3 * i] = P[4 * i]; p3[3 * i + 1] = P[4 * i + 1]; p3[3 * i + 2] = P[4 * i + 2];
    nc[4 * i] = Nm[4 * i]; nc[4 * i + 1] = Nm[4 * i + 1]; nc[4 * i + 2] = Nm[4 * i + 2]; nc[4 * i + 3] = P[4 * i + 3];
  }
  HIPCHK(ctx, hipMemcpy(d.P3, p3.data(), p3.size() * 4, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpy(d.Nc, nc.data(), nc.size() * 4, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
AlignParams make_align_params(const pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p) {
  AlignParams ap;
  ap.settleGuard = ctx ? ctx->settle_guard : kSettleGuard;
  ap.mayFreeze = ctx ? ctx->stop.enabled : 0;
  ap.rows = p->rows; ap.cols = p->cols;
  ap.K = mat3_from(p->K);
  ap.refOffset = mat4_from(p->reference_sensor_offset);
  ap.minD = p->min_distance; ap.maxD = p->max_distance;
  ap.sqDist = p->inlier_distance_threshold * p->inlier_distance_threshold;
  ap.normalThr = p->inlier_normal_angular_threshold;
  ap.flatThr = p->flat_curvature_threshold;
  ap.minRatio = 1.0f / p->inlier_curvature_ratio_threshold;
  ap.maxRatio = p->inlier_curvature_ratio_threshold;
  ap.maxChi2 = p->inlier_max_chi2;
  ap.robust = p->robust_kernel;
  return ap;
}

int check_image(pwn_hip_ctx* ctx, int rows, int cols) {
  if (rows <= 0 || cols <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "image has zero size");
  // both sides are bounded: the hand-over / offset workspaces (rowoff_slot, carry_slot in pwn_hip_ctx_create) are sized for
  // rows, cols <= max(max_rows, max_cols); a wide, short image with rows*cols <= N would overrun them
  const int M = std::max(ctx->max_rows, ctx->max_cols);
  if ((size_t)rows * cols > ctx->N || rows > M || cols > M)
    return fail(ctx, PWN_HIP_ERR_CAPACITY, "image larger than the context was created for");
  return PWN_HIP_OK;
}
// first (largest) of `need` consecutive descending tags of the 64-bit z-buffer (scene stage); clears it when the tag space is used up
int take_tags(pwn_hip_ctx* ctx, unsigned need, unsigned* first) {
  if (need > kZTag0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "more projections than z-buffer epoch tags");
  if (ctx->ztag_next < need) {
    HIPCHK(ctx, hipMemsetAsync(ctx->zref_ws, 0xFF, ctx->N * 8, ctx->stream), PWN_HIP_ERR_COPY);
    ctx->ztag_next = kZTag0;
  }
  *first = ctx->ztag_next;
  ctx->ztag_next -= need;
  return PWN_HIP_OK;
}
// the same for the aligner's 32-bit z-buffers (11-bit tags): clears every slot of both when the tag space is used up
int take_tags32(pwn_hip_ctx* ctx, unsigned need, unsigned* first) {
  if (need > kZ32Tag0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "more projections per alignment than z-buffer epoch tags");
  if (ctx->z32tag_next < need) {
    HIPCHK(ctx, hipMemsetAsync(ctx->z32ref_ws, 0xFF, (size_t)ctx->max_batch * ctx->N * 4, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemsetAsync(ctx->z32cur_ws, 0xFF, (size_t)ctx->max_batch * ctx->N * 4, ctx->stream), PWN_HIP_ERR_COPY);
    ctx->z32tag_next = kZ32Tag0;
  }
  *first = ctx->z32tag_next;
  ctx->z32tag_next -= need;
  return PWN_HIP_OK;
}
// the two-pass projection's depth images: one per workspace slot, allocated when a call first needs them
int ensure_zdepth(pwn_hip_ctx* ctx) {
  HIPCHK(ctx, ctx->zdepth_ws.ensure((size_t)ctx->max_batch * ctx->N), PWN_HIP_ERR_ALLOCATION);
  return PWN_HIP_OK;
}
// An alignment attempt starts here and ends in take_align_fault; a robust one (the repeat) runs every projection with the two-pass kernels
int start_align_attempt(pwn_hip_ctx* ctx, bool robust) {
  ctx->last_align_fault = 0;
  return robust ? ensure_zdepth(ctx) : PWN_HIP_OK;
}
const char* const kSettleMessage = "projection: a pixel's z-buffer settle loop gave up (too many points of one cloud in one pixel)";
// after the attempt's final wait: did a projection of it give up on a pixel?  (the word is host memory the kernels store to)
int take_align_fault(pwn_hip_ctx* ctx) {
  const bool f = ctx->align_fault_host && *(volatile int*)ctx->align_fault_host != 0;
  if (f) *(volatile int*)ctx->align_fault_host = 0;
  ctx->last_align_fault = f ? 1 : 0;
  return f ? fail(ctx, PWN_HIP_ERR_LAUNCH, kSettleMessage) : PWN_HIP_OK;
}
// attempt(false); if it failed with the given fault (a projection's settle loop gave up, or a converter strip's hand-over timed out), the
// repeat is counted and attempt(true) runs.  Once only: a second fault is reported.
enum RepeatOn { kSettleFault, kHandoverTimeout };
template <typename Attempt>
int repeat_once(pwn_hip_ctx* ctx, RepeatOn on, Attempt attempt) {
  const int rc = attempt(false);
  if (rc != PWN_HIP_ERR_LAUNCH || !ctx || (on == kSettleFault ? ctx->last_align_fault : ctx->last_convert_fault) != 1) return rc;
  if (on == kSettleFault) ++ctx->projection_fallbacks;
  else ++ctx->convert_retries;
  return attempt(true);
}
int align_nblocks(int N) { return (N + kAlignBlock * kPixPerThread - 1) / (kAlignBlock * kPixPerThread); }

// descriptor / state arrays for a batch of n items
int ensure_desc(pwn_hip_ctx* ctx, int n) {
  if (n <= ctx->desc_cap) return PWN_HIP_OK;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  ctx->desc_cap = 0;
  ctx->img.invalidate();                     // the descriptor of the last alignment's pair goes with the old arrays
  const size_t B = (size_t)std::max(n, 16);
  HIPCHK(ctx, ctx->frames_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->pairs_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->raw_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->counts_dev.ensure(B + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->state_ws.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->frames_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->pairs_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->raw_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->state_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->counts_host.ensure(B + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->cur_raw_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->cur_raw_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->cur_strip_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->cur_strip_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->match_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->match_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->stats_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->stats_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->pairstats_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->pairstats_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  ctx->desc_cap = (int)B;
  return PWN_HIP_OK;
}

// launch sequence of the converter for the frames [base, base+n) of the uploaded descriptor array
// fault_out: page-locked host word for the launch's time-out flag (latency path only; nullptr = the caller copies ctx->fault_dev itself)
// launches of at least this many frames take the single-pass strip kernel; measured on MI355X at VGA, three kernels vs single pass: 8 frames 0.20 vs
// 0.27 ms, 16 frames 0.38 vs 0.35, 32 frames 0.74 vs 0.58
constexpr int kSinglePassMinFrames = 16;
bool single_pass_launch(int n) { return n >= kSinglePassMinFrames; }
// the stats pass over n frames
void launch_stats(const ConvertParams& cp, const FrameDesc* fr, int n, hipStream_t st) {
  const unsigned perFrame = (unsigned)cp.rows * (unsigned)((cp.cols + 255) / 256);
  const unsigned nblk = (n >= 8 ? 8u * (unsigned)((n + 7) / 8) : (unsigned)n) * perFrame;      // see k_stats: XCD-aware placement from 8 frames on
  hipLaunchKernelGGL(k_stats, dim3(nblk), dim3(256), 0, st, fr, cp, n);
}
// the front end of a convert call (everything before the stats pass): counts, offsets, points, index / interval images, integral planes
int launch_front_end(pwn_hip_ctx* ctx, const ConvertParams& cp, int base, int n, hipStream_t st, bool single_pass, int* fault_out) {
  const FrameDesc* fr = ctx->frames_dev + base;
  if (single_pass) {
    // throughput path: the integral planes are written once; a frame is a chain of strips * bands hand-over steps, so it
    // needs several frames in flight to fill the device
    { StageTimer t(ctx, "unproject", st);          // ordered compaction: valid pixels per (row, strip) and their offsets
      // frames of one call are all raw uint16 or all float (convert_batch_impl); 16-byte loads need 16-byte aligned rows
      const bool raw = ctx->frames_host[base].raw != nullptr;
      bool aligned = cp.cols % (raw ? 8 : 4) == 0;
      for (int i = 0; i < n && aligned; ++i) {
        const FrameDesc& fd = ctx->frames_host[base + i];
        aligned = ((uintptr_t)(raw ? (const void*)fd.raw : (const void*)fd.depth) & 15u) == 0;
      }
      if (aligned && raw) hipLaunchKernelGGL(k_strip_count<true>, dim3((cp.rows + 3) / 4, n), dim3(256), 0, st, fr, cp);
      else if (aligned) hipLaunchKernelGGL(k_strip_count<false>, dim3((cp.rows + 3) / 4, n), dim3(256), 0, st, fr, cp);
      else hipLaunchKernelGGL(k_strip_count_any, dim3(cp.rows, n), dim3(256), 0, st, fr, cp);
      hipLaunchKernelGGL(k_row_offsets, dim3(n), dim3(1024), 0, st, fr, cp.rows * strips_of(cp.cols)); }
    { StageTimer t(ctx, "integral", st);           // unProject + intervals + the three integral-image passes
      const unsigned epoch = ++ctx->convert_epoch;
      if (epoch == 0) return fail(ctx, PWN_HIP_ERR_LAUNCH, "convert epoch wrapped: recreate the context");
      const dim3 grid(8u * (unsigned)((n + 7) / 8) * (unsigned)strips_of(cp.cols));
      if (cp.lean == kLeanGrouped) hipLaunchKernelGGL(k_unproject_integral_grouped, grid, dim3(kII_Threads), 0, st, fr, cp, n, epoch, ctx->fault_dev);
      else hipLaunchKernelGGL(k_unproject_integral, grid, dim3(kII_Threads), 0, st, fr, cp, n, epoch, ctx->fault_dev); }
  } else {
    // latency path (single frames: tracker, makeCloud): three short, fully parallel kernels
    { StageTimer t(ctx, "unproject", st);          // ordered compaction: per-row counts and offsets
      hipLaunchKernelGGL(k_row_count, dim3(cp.rows, n), dim3(256), 0, st, fr, cp);
      hipLaunchKernelGGL(k_row_offsets, dim3(n), dim3(1024), 0, st, fr, cp.rows); }
    { StageTimer t(ctx, "integral_rows", st);      // unProject + intervals + accumulate + row prefix, one pass over the depth
      const unsigned epoch = ++ctx->convert_epoch;
      if (epoch == 0) return fail(ctx, PWN_HIP_ERR_LAUNCH, "convert epoch wrapped: recreate the context");
      hipLaunchKernelGGL(k_unproject_integral_rows, dim3(8u * (unsigned)((bands_of(cp.rows) + 7) / 8) * (unsigned)strips_of(cp.cols), n), dim3(256), 0, st, fr, cp,
                         epoch, ctx->fault_dev); }
    { StageTimer t(ctx, "integral_cols", st);
      const bool grouped = cp.lean == kLeanGrouped;
      const dim3 grid = grouped ? dim3((ig_width(0) * cp.cols + kIC_Block - 1) / kIC_Block, kIG_Groups, n)
                                   : dim3((cp.cols + kIC_Block - 1) / kIC_Block, kIntegralChannels, n);
      hipLaunchKernelGGL(k_integral_cols, grid, dim3(kIC_Block), 0, st, fr, cp.rows, cp.cols, (const int*)ctx->fault_dev, fault_out, grouped ? 1 : 0); }
  }
  return PWN_HIP_OK;
}
int launch_convert(pwn_hip_ctx* ctx, const ConvertParams& cp, int base, int n, hipStream_t st, int* fault_out = nullptr) {
  if (int rc = launch_front_end(ctx, cp, base, n, st, single_pass_launch(n), fault_out)) return rc;
  { StageTimer t(ctx, "stats", st);
    launch_stats(cp, ctx->frames_dev + base, n, st); }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
void fill_frame(pwn_hip_ctx* ctx, int entry, int slot, const float* depth_dev, const CloudDev& cl) {
  FrameDesc& f = ctx->frames_host[entry];
  f.depth = depth_dev; f.raw = nullptr; f.raw_scale = 0.f;
  f.index = ctx->index_ws + (size_t)slot * ctx->N;
  f.interval = ctx->interval_ws + (size_t)slot * ctx->N;
  f.integral = ctx->integral_ws + (size_t)slot * ctx->N * kIntegralChannels;
  f.rowoff = ctx->rowoff_ws + (size_t)slot * ctx->rowoff_slot;
  f.carry = ctx->carry_ws + (size_t)slot * ctx->carry_slot;
  f.cloud = cl;
  f.count_out = nullptr;
}
// the cloud's front gets the arrays of the groups `which` (kArrSt: keep_stats; kArrOmN: explicit Omega_n planes -- converted clouds keep the two
// class matrices only; kArrGauss: the scene stage)
int cloud_own(pwn_hip_ctx* ctx, pwn_hip_cloud* c, unsigned which) {
  HIPCHK(ctx, c->own(which), PWN_HIP_ERR_ALLOCATION);
  return PWN_HIP_OK;
}
// ---- the three transitions of a cloud's content (CloudContent); every entry point that writes a cloud says which one it is ----
// Replace: the cloud is about to receive new points from outside.  What it held is gone from here on -- it reads as empty, without Gaussians and,
// unless the caller promises that the points will arrive with the index image of `key`, without an index image -- and the arrays of what is coming
// are there: St when Stats are kept; for the normal information matrices the explicit planes (`planes`), or no planes and the class matrices
// `cls` (nullptr: as they are); the Gaussian arrays when the conversion will write Gaussians (`gauss`; the count stays 0 until its commit).  Planes are dropped after a wait for the stream, which may still read them; the wait happens only then.
// (`key` without the promise: what the index image is being made with, kept beside an image that is not valid -- the flat form carries it.)
int cloud_replace(pwn_hip_ctx* ctx, pwn_hip_cloud* c, bool keep_stats, bool planes, const OmegaNClasses* cls, const IndexKey* key = nullptr, bool promised = false,
                  bool gauss = false) {
  cloud_changes(ctx, c);
  if (const unsigned which = (keep_stats ? kArrSt : 0u) | (planes ? kArrOmN : 0u) | (gauss ? kArrGauss : 0u)) { if (int rc = cloud_own(ctx, c, which)) return rc; }
  if (!planes && c->d.OmN) { HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH); c->drop_omega_n(); }
  if (cls) { std::memcpy(c->d.omN, cls->omN, sizeof(cls->omN)); c->d.clsThr = cls->clsThr; }
  c->content.replace(keep_stats, key, promised);
  c->stripoff_filled = false;      // the table went with the index image it belonged to; a conversion that fills it says so after this (convert_prepare)
  return PWN_HIP_OK;
}
// Commit: the new content has arrived, `n` points of it; with `key` the index image came with them, without it a promised one stands.  (The
// device's size word is the kernels' or the caller's copy.)
void cloud_commit(pwn_hip_cloud* c, int n, const IndexKey* key = nullptr) { if (key) c->content.commit(n, *key); else c->content.commit(n); }
void cloud_commit_with_gaussians(pwn_hip_cloud* c, int n) { c->content.commit_with_gaussians(n); }      // a promised index key stands here too
// Edit: the points changed in place, or their number did: no index image, `n` points.  device_word: the host decided the size, and the device's
// word follows on the stream, as a fill value, so that nothing is read from host memory after the call returned.
int cloud_edit(pwn_hip_ctx* ctx, pwn_hip_cloud* c, int n, bool device_word) {
  c->content.edit(n);
  if (device_word) HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)c->d.count, n, 1, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// The Stats record of a point (CloudDev::St, 16 floats) on the host: the 3x3 block of the matrix column-major at 0..8, the eigenvalues at 9..11, the
// translation at 12..14, the point count at 15.  To and from Stats as a column-major 4x4 with its eigenvalues and count (stats.h:13-27); the
// default Stats() is the identity with eigenvalues and count zero.
void stats_unpack(const float* s, float S[16], float ev[3], int* npts) {
  for (int q = 0; q < 16; ++q) S[q] = 0.f;
  for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) S[r + 4 * q] = s[r + 3 * q];
  S[12] = s[12]; S[13] = s[13]; S[14] = s[14]; S[15] = 1.0f;
  ev[0] = s[9]; ev[1] = s[10]; ev[2] = s[11]; *npts = (int)s[15];
}
void stats_pack(const float S[16], const float ev[3], int npts, float* s) {
  for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) s[r + 3 * q] = S[r + 4 * q];
  s[12] = S[12]; s[13] = S[13]; s[14] = S[14]; s[9] = ev[0]; s[10] = ev[1]; s[11] = ev[2]; s[15] = (float)npts;
}
std::vector<float> default_stats(int n) {
  std::vector<float> st((size_t)n * 16, 0.f);
  for (int i = 0; i < n; ++i) { st[(size_t)16 * i] = 1.f; st[(size_t)16 * i + 4] = 1.f; st[(size_t)16 * i + 8] = 1.f; }
  return st;
}
// direct: the kernels of the call have written counts and fault flag into counts_host themselves (FrameDesc::count_out, launch_convert's fault_out)
// the two halves of sync_and_counts for callers that wait for the stream themselves: queue the copy back of counts + fault flag; digest them
int counts_enqueue(pwn_hip_ctx* ctx, int n) {
  if (n <= 0) return PWN_HIP_OK;
  hipLaunchKernelGGL(k_gather_counts, dim3((n + 256) / 256), dim3(256), 0, ctx->stream, ctx->frames_dev, n, ctx->counts_dev, ctx->fault_dev);
  HIPCHK(ctx, hipMemcpyAsync(ctx->counts_host, ctx->counts_dev, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// the fault flag and the counts against the clouds' capacities; nothing is committed
int counts_check(pwn_hip_ctx* ctx, pwn_hip_cloud* const* clouds, int n) {
  if (n > 0 && ctx->counts_host[n] != 0) {
    const int code = ctx->counts_host[n];
    (void)hipMemset(ctx->fault_dev, 0, sizeof(int));
    ctx->last_convert_fault = code;
    if (ctx->dbg_withhold_once) { ctx->dbg_withhold = -1; ctx->spin_limit = kSpinLimit; ctx->dbg_withhold_once = 0; }
    return fail(ctx, PWN_HIP_ERR_LAUNCH, "integral image: strip hand-over timed out (results invalid)");
  }
  ctx->last_convert_fault = 0;
  for (int i = 0; i < n; ++i)
    if (ctx->counts_host[i] > clouds[i]->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity smaller than the number of valid depth pixels");
  return PWN_HIP_OK;
}
// commit: the counts are the clouds' sizes, if the check lets all of them pass
int counts_apply(pwn_hip_ctx* ctx, pwn_hip_cloud* const* clouds, int n, bool gauss = false) {
  if (int rc = counts_check(ctx, clouds, n)) return rc;
  for (int i = 0; i < n; ++i) { if (gauss) cloud_commit_with_gaussians(clouds[i], ctx->counts_host[i]); else cloud_commit(clouds[i], ctx->counts_host[i]); }
  return PWN_HIP_OK;
}
// frames_dev[0..n) must describe clouds[0..n): the counts and the fault flag back (direct: the kernels stored them in counts_host themselves), the wait
int sync_counts(pwn_hip_ctx* ctx, int n, bool direct = false) {
  if (n > 0 && !direct) { if (int rc = counts_enqueue(ctx, n)) return rc; }
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}
int sync_and_counts(pwn_hip_ctx* ctx, pwn_hip_cloud* const* clouds, int n) {
  if (int rc = sync_counts(ctx, n)) return rc;
  return counts_apply(ctx, clouds, n);
}

// One converter call.  What the caller asks for is one record (ConvertCall, below); the work is cut into the pieces a caller can interleave with
// other work on the same streams: convert_prepare (descriptors of all frames, uploaded on ctx->stream), convert_stage_frames (host frames
// [base, base + m) into their slots), convert_enqueue (the kernels of those frames on one stream) and convert_finish (counts and fault flag back,
// clouds' host-side sizes).  A batch call runs them phase by phase (convert_batch_once); the one-call step weaves them into an alignment.
// slot[i] = workspace slot of frame i: frames that are in flight at the same time on different streams must not share one; a stream reuses its
// slots from launch to launch (stream order serialises the reuse).
// DepthImage_scale in front of a conversion (PwnMatcherBase::makeCloud, pwn_matcher_base.cpp:57-86): the source size, the step and what it leaves
struct ScaleSpec {
  int step = 0;                          // 0: the frames are converted as they are
  int srows = 0, scols = 0, orows = 0, ocols = 0; float maxCov = 0.f;
};
// the argument checks the *_scaled calls share: the step, a source frame the context holds, a scaled image that is not empty
int make_scale_spec(pwn_hip_ctx* ctx, int rows, int cols, int step, float max_depth_cov, ScaleSpec& sc) {
  if (step < 1) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImage_scale: step < 1");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  sc.step = step; sc.srows = rows; sc.scols = cols; sc.orows = rows / step; sc.ocols = cols / step; sc.maxCov = max_depth_cov;
  if (sc.orows <= 0 || sc.ocols <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "scaled image has zero size");
  return PWN_HIP_OK;
}
// the scaled frames' workspace (one frame per slot, as depth_ws) and box descriptors for n frames (grown after a wait for the stream, as
// ensure_desc grows its arrays)
int ensure_scale(pwn_hip_ctx* ctx, int n) {
  HIPCHK(ctx, ctx->scaled_ws.ensure((size_t)ctx->max_batch * ctx->N), PWN_HIP_ERR_ALLOCATION);
  if ((size_t)n > ctx->scale_dev.cap) HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  const size_t B = (size_t)std::max(n, 16);
  HIPCHK(ctx, ctx->scale_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->scale_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  return PWN_HIP_OK;
}
// DepthImage_scale of the frames [base, base + n) of the uploaded box descriptors (scale_host / scale_dev) on st.  The 16-byte form for the
// three (type, step) pairs it exists for, when every frame and every source row starts 16-byte aligned; else one thread per pixel.
int launch_depth_scale(pwn_hip_ctx* ctx, const ScaleSpec& sc, bool raw, float raw_scale, int base, int n, hipStream_t st) {
  if (n <= 0) return PWN_HIP_OK;
  StageTimer t(ctx, "depth_scale", st);
  const ScaleDesc* fr = ctx->scale_dev + base;
  bool aligned = ((size_t)sc.scols * (raw ? sizeof(uint16_t) : sizeof(float))) % 16 == 0 && (raw ? (sc.step == 2 || sc.step == 4) : sc.step == 2);
  for (int i = 0; i < n && aligned; ++i) aligned = ((uintptr_t)ctx->scale_host[base + i].src & 15u) == 0;
  if (aligned) {
    const int dpl = (raw ? 8 : 4) / sc.step;
    const dim3 grid((unsigned)(((size_t)sc.orows * (size_t)((sc.ocols + dpl - 1) / dpl) + 255) / 256), (unsigned)n);
    if (!raw) hipLaunchKernelGGL((k_depth_scale_batch<float, 2>), grid, dim3(256), 0, st, fr, sc.srows, sc.scols, raw_scale, sc.maxCov);
    else if (sc.step == 2) hipLaunchKernelGGL((k_depth_scale_batch<uint16_t, 2>), grid, dim3(256), 0, st, fr, sc.srows, sc.scols, raw_scale, sc.maxCov);
    else hipLaunchKernelGGL((k_depth_scale_batch<uint16_t, 4>), grid, dim3(256), 0, st, fr, sc.srows, sc.scols, raw_scale, sc.maxCov);
  } else {
    const dim3 grid((unsigned)(((size_t)sc.orows * sc.ocols + 255) / 256), (unsigned)n);
    if (raw) hipLaunchKernelGGL(k_depth_scale_batch_any<uint16_t>, grid, dim3(256), 0, st, fr, sc.srows, sc.scols, sc.step, raw_scale, sc.maxCov);
    else hipLaunchKernelGGL(k_depth_scale_batch_any<float>, grid, dim3(256), 0, st, fr, sc.srows, sc.scols, sc.step, raw_scale, sc.maxCov);
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// The sensor-noise Gaussians a conversion writes beside its points (pwn_hip_convert_batch_ex): the arguments k_gaussians takes
struct GaussSpec {
  bool on = false;
  Mat3 iK; float fB = 0.f, alpha = 0.f;
};
// the per-frame Gaussian arrays of a call of n frames (grown after a wait for the stream, as ensure_desc grows its arrays)
int ensure_gauss_desc(pwn_hip_ctx* ctx, int n) {
  if ((size_t)n > ctx->gauss_dev.cap) HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  const size_t B = (size_t)std::max(n, 16);
  HIPCHK(ctx, ctx->gauss_dev.ensure(B), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->gauss_host.ensure(B), PWN_HIP_ERR_ALLOCATION);
  return PWN_HIP_OK;
}
// What a caller asks of a conversion; every member defaults to "not asked for", an entry point names the ones it uses (on its stack; handed down by reference).
struct ConvertCall {
  const pwn_hip_converter_params* p = nullptr;
  int n = 0;                                                   // frames: frames[i] into clouds[i]
  const void* const* frames = nullptr;                         // device or host, all of one kind; all float (metres), or
  bool raw = false; float depth_scale = 0.f;                   // all uint16 with their scale
  int rows = 0, cols = 0;                                      // the size that is converted (scale.step != 0: of the down-sampled image)
  pwn_hip_cloud* const* clouds = nullptr;
  int keep_stats = 0; bool want_interval = false;              // the interval image stays readable (pwn_hip_convert(..., interval_image))
  ScaleSpec scale; GaussSpec gauss;                            // DepthImage_scale in front of every conversion; the sensor-noise Gaussians beside the points
  int first_entry = 0;                                         // the job's descriptors are entries [first_entry, first_entry + n) of the context's arrays: a call
                                                               // that holds two jobs of different kinds at once (the mapping step) puts the second behind the first
};
// The members every entry point fills, and where the typed ones hand their frame arrays over: behind it the frame type is ConvertCall::raw
template <typename T>
ConvertCall convert_call(const pwn_hip_converter_params* p, const T* const* frames, float depth_scale, int n, int rows, int cols, pwn_hip_cloud* const* clouds) {
  static_assert(std::is_same<T, float>::value || std::is_same<T, uint16_t>::value, "depth frames are float or uint16");
  ConvertCall c; c.p = p; c.n = n; c.rows = rows; c.cols = cols; c.clouds = clouds;
  c.frames = reinterpret_cast<const void* const*>(frames); c.raw = std::is_same<T, uint16_t>::value; c.depth_scale = c.raw ? depth_scale : 0.f;
  return c;
}
struct ConvertJob {
  ConvertParams cp;
  GaussSpec gauss;
  int n = 0, rows = 0, cols = 0;
  int entry0 = 0;                        // ConvertCall::first_entry: frame i of the job is entry entry0 + i of frames_dev / gauss_dev / scale_dev / counts_host
  size_t N = 0;
  size_t srcN = 0;                       // pixels of a frame as the caller hands it over (= N unless the job down-samples)
  ScaleSpec scale;
  bool raw = false, host_input = false, direct = false;      // raw: the caller's frames are uint16
  float depth_scale = 0.f;
  std::vector<const void*> src;          // the caller's frame pointers (host frames are staged by convert_enqueue)
  std::vector<int> slot;
  // The clouds convert_prepare has replaced the content of.  A job that ends any other way than through convert_commit -- an error return, the first
  // attempt of a repeated call, a front end that stores no points -- leaves them empty and takes the index promise back.
  std::vector<pwn_hip_cloud*> clouds; bool committed = false;
  ~ConvertJob() { if (!committed) for (pwn_hip_cloud* c : clouds) c->content.withdraw(); }
};
int convert_prepare(pwn_hip_ctx* ctx, const ConvertCall& c, const std::vector<int>& slot, bool direct, ConvertJob& job) {
  const int n = c.n; const bool raw = c.raw; const ScaleSpec& sc = c.scale; const GaussSpec& gs = c.gauss;
  const size_t N = (size_t)c.rows * c.cols;
  ctx->last_convert_fault = 0;            // the fault word belongs to this call from here on (a stale 1 would make an unrelated failure look like a time-out)
  ConvertParams cp = make_convert_params(ctx, c.p, nullptr, c.rows, c.cols, c.keep_stats);
  // the interval image leaves the converter only through pwn_hip_convert(..., interval_image); nothing outside the library sees a lean call's
  // integral image: grouped storage (ig_at)
  cp.lean = c.want_interval ? 0 : kLeanGrouped;
  const int e0 = c.first_entry;
  if (int rc = ensure_desc(ctx, e0 + n)) return rc;
  if (gs.on) { if (int rc = ensure_gauss_desc(ctx, e0 + n)) return rc; }
  job.gauss = gs; job.entry0 = e0;
  job.n = n; job.rows = c.rows; job.cols = c.cols; job.N = N; job.raw = raw; job.depth_scale = c.depth_scale; job.slot = slot; job.direct = direct;
  job.scale = sc; job.srcN = sc.step ? (size_t)sc.srows * sc.scols : N;
  job.src.assign(n, nullptr);
  cp.omSym = n > 0 ? c.clouds[0]->d.omSym : 0;      // one storage for all of them: check_frames_and_clouds
  const OmegaNClasses cls = make_omega_n_classes(c.p);
  // the index image stays with the cloud, promised for the points this conversion will store (a sensor offset moves them off their pixels)
  const IndexKey key = index_key(c.p, c.rows, c.cols);
  job.host_input = n > 0 && !is_device_ptr(c.frames[0]);      // host frames are staged per launch, in their slots; device frames are read in place
  // every frame gets a descriptor; workspace slots are reused round-robin (stream order serialises the reuse)
  for (int i = 0; i < n; ++i) {
    pwn_hip_cloud* cl = c.clouds[i];
    if (int rc = cloud_replace(ctx, cl, c.keep_stats != 0, false, &cls, &key, cp.hasOffset == 0, gs.on)) return rc;
    job.clouds.push_back(cl);
    if (gs.on) ctx->gauss_host[e0 + i] = cl->sb;
    job.src[i] = c.frames[i];
    const void* src = c.frames[i];      // where the kernels find the frame
    if (job.host_input) src = raw ? (const void*)(ctx->raw_ws + (size_t)slot[i] * ctx->N) : (const void*)(ctx->depth_ws + (size_t)slot[i] * ctx->N);
    float* scaled = sc.step ? ctx->scaled_ws + (size_t)slot[i] * ctx->N : nullptr;      // a down-sampling job: the box kernel writes, the front end reads the slot's frame
    fill_frame(ctx, e0 + i, slot[i], sc.step ? scaled : raw ? nullptr : static_cast<const float*>(src), cl->d);
    if (cl->idximg.cap < N) {
      HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
      HIPCHK(ctx, cl->idximg.ensure(N), PWN_HIP_ERR_ALLOCATION);
    }
    ctx->frames_host[e0 + i].index = cl->idximg;
    // ... and so do the strip offsets it is counted from, where a single-pass launch will leave a table of 64-column strips that line up with
    // the rows: the front end's kernels get the cloud's buffer for their workspace slot, and run the code they ran (a three-kernel launch
    // writes its [rows] offsets there and takes the promise back: convert_enqueue)
    if (cp.hasOffset == 0 && c.cols % kIR_Cols == 0) {
      const size_t words = (size_t)c.rows * (size_t)strips_of(c.cols);
      if (cl->stripoff.cap < words) {
        HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
        HIPCHK(ctx, cl->stripoff.ensure(words), PWN_HIP_ERR_ALLOCATION);
      }
      ctx->frames_host[e0 + i].rowoff = cl->stripoff;
      cl->stripoff_filled = true;
    }
    if (sc.step) { ctx->scale_host[e0 + i].src = src; ctx->scale_host[e0 + i].dst = scaled; }
    else if (raw) { ctx->frames_host[e0 + i].raw = static_cast<const uint16_t*>(src); ctx->frames_host[e0 + i].raw_scale = c.depth_scale; }      // converted on the fly by the kernels
  }
  if (sc.step) HIPCHK(ctx, hipMemcpyAsync(ctx->scale_dev + e0, ctx->scale_host + e0, sizeof(ScaleDesc) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  if (gs.on && n > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->gauss_dev + e0, ctx->gauss_host + e0, sizeof(SceneBuffers) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  // a call of a few frames (latency path, one launch): counts and fault flag land in page-locked host words straight from the kernels
  if (direct) for (int i = 0; i < n; ++i) ctx->frames_host[e0 + i].count_out = ctx->counts_host + e0 + i;
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev + e0, ctx->frames_host + e0, sizeof(FrameDesc) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  job.cp = cp;
  return PWN_HIP_OK;
}
// frames [base, base + m) of the job: their host frames (if any) copied on `cs`, their kernels launched on `st`.  The frames' slots must be
// consecutive (slot[base + i] = slot[base] + i).
int convert_stage_frames(pwn_hip_ctx* ctx, const ConvertJob& job, int base, int m, hipStream_t cs) {
  // frames that follow each other in host memory (a ring buffer, one block for the batch) go in one transfer -- only when the frame
  // fills its staging slot (N == ctx->N), so that the slots are contiguous too
  const size_t fbytes = job.srcN * (job.raw ? sizeof(uint16_t) : sizeof(float));
  const int s0 = job.slot[base];
  for (int i = 0; i < m;) {
    int run = 1;
    if (job.srcN == ctx->N)
      while (i + run < m && (const char*)job.src[base + i + run] == (const char*)job.src[base + i] + (size_t)run * fbytes) ++run;
    void* dst = job.raw ? (void*)(ctx->raw_ws + (size_t)(s0 + i) * ctx->N) : (void*)(ctx->depth_ws + (size_t)(s0 + i) * ctx->N);
    HIPCHK(ctx, hipMemcpyAsync(dst, job.src[base + i], fbytes * run, hipMemcpyHostToDevice, cs), PWN_HIP_ERR_COPY);
    i += run;
  }
  return PWN_HIP_OK;
}
// what convert_prepare relies on, looked at by every caller before it touches a cloud (a refused call leaves the clouds as they were)
int check_frames_and_clouds(pwn_hip_ctx* ctx, const void* const* frames, pwn_hip_cloud* const* clouds, int n) {
  for (int i = 0; i < n; ++i) {
    if (!clouds[i] || !frames[i]) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null frame or cloud");
    if (clouds[i]->d.omSym != clouds[0]->d.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "clouds of one convert batch must share one omega storage (exact9 / sym6)");
  }
  return PWN_HIP_OK;
}
// the Gaussians of frames [base, base + m) on st, behind the front end that wrote their index images (and on its stream: the kernel reads the depth
// the front end read, which for a down-sampling job is the slot's frame, and stream order keeps the slot's next user behind it)
int launch_gaussians(pwn_hip_ctx* ctx, const ConvertJob& job, int base, int m, hipStream_t st) {
  if (m <= 0) return PWN_HIP_OK;
  StageTimer t(ctx, "gaussians", st);
  const dim3 grid((unsigned)((job.N + 255) / 256), (unsigned)m);
  const FrameDesc* fr = ctx->frames_dev + job.entry0 + base; const SceneBuffers* sbs = ctx->gauss_dev + job.entry0 + base;
  if (ctx->gauss_staged) hipLaunchKernelGGL(k_gaussians_batch<true>, grid, dim3(256), 0, st, fr, sbs, job.cp, job.gauss.iK, job.gauss.fB, job.gauss.alpha);
  else hipLaunchKernelGGL(k_gaussians_batch<false>, grid, dim3(256), 0, st, fr, sbs, job.cp, job.gauss.iK, job.gauss.fB, job.gauss.alpha);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// the kernels of frames [base, base + m) of the job on st: the box mean into the frames' slots first when the job down-samples, the Gaussians last
// when it makes them
// the clouds of frames [base, base + m) get no strip table after all: their launch runs the three-kernel front end, whose offsets are per row
void no_strip_tables(const ConvertJob& job, int base, int m) { for (int i = 0; i < m; ++i) job.clouds[(size_t)(base + i)]->stripoff_filled = false; }
int convert_enqueue(pwn_hip_ctx* ctx, const ConvertJob& job, int base, int m, hipStream_t st, int* fault_out = nullptr) {
  if (!single_pass_launch(m)) no_strip_tables(job, base, m);
  if (job.scale.step) { if (int rc = launch_depth_scale(ctx, job.scale, job.raw, job.depth_scale, job.entry0 + base, m, st)) return rc; }
  if (int rc = launch_convert(ctx, job.cp, job.entry0 + base, m, st, fault_out)) return rc;
  if (job.gauss.on) return launch_gaussians(ctx, job, base, m, st);
  return PWN_HIP_OK;
}
// commit: the job's clouds hold what its kernels counted (after the wait that brought counts and fault flag back)
int convert_commit(pwn_hip_ctx* ctx, ConvertJob& job) {
  if (int rc = counts_apply(ctx, job.clouds.data(), job.n, job.gauss.on)) return rc;
  job.committed = true;
  return PWN_HIP_OK;
}
int convert_finish(pwn_hip_ctx* ctx, ConvertJob& job) {
  if (int rc = sync_counts(ctx, job.n, job.direct)) return rc;
  return convert_commit(ctx, job);
}

// What the phases of one attempt at a conversion share (on convert_batch_once's stack)
struct ConvertRun {
  StreamPlan plan;
  std::vector<int> slot;                 // workspace slot of every frame
  bool direct = false;                   // a few frames in one launch (latency path): counts and fault flag arrive in host words, no copy back
  bool ahead = false;                    // host frames travel on the copy stream, ahead of the kernels
  ConvertJob job;
};
// ---- one attempt at a batch conversion, phase by phase (convert_batch_once calls them in this order) ----
// Check: what can refuse the call before a cloud is touched.  Once per call, in front of the attempts; on the streams: nothing (queued copies absorbed).
int convert_check(pwn_hip_ctx* ctx, const ConvertCall& c) {
  if (!ctx || !c.p || !c.frames || !c.clouds || c.n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, c.rows, c.cols)) return rc;
  if (int rc = check_frames_and_clouds(ctx, c.frames, c.clouds, c.n)) return rc;
  return absorb_copies(ctx);
}
// Plan and slots.  On the streams: nothing.  Sub-batch k takes the slots of its stream's block, frame by frame.
void convert_plan_slots(pwn_hip_ctx* ctx, const ConvertCall& c, ConvertRun& run) {
  ctx->stages.clear();
  run.plan = make_plan(ctx, ctx->sub_frames, c.n);
  const int sub = run.plan.sub;
  run.slot.resize((size_t)std::max(c.n, 0));
  for (int i = 0; i < c.n; ++i) run.slot[i] = run.plan.slot0(i / sub) + i % sub;
  run.direct = c.n > 0 && c.n < kSinglePassMinFrames && c.n <= sub;
}
// Set the copy-ahead up (prepare has found out whether the frames are host memory).  On the copy stream: the wait for everything queued before this call.
// Host frames travel on the copy stream, ahead of the kernels: the frames of sub-batch k are copied while sub-batches k-1, k-2 ... are
// being converted (with the copies on the sub-batch's own stream the two streams copy at the same time and then compute at the same
// time: 7.5 ms per 256 VGA frames against 5).  copied[k] (sync_events[2 k]) orders convert k after its copies; converted[k]
// (sync_events[2 k + 1]) orders the copies into a staging block after the kernels that read its previous content.
int convert_copy_ahead(pwn_hip_ctx* ctx, const ConvertCall& c, ConvertRun& run) {
  run.ahead = run.job.host_input && ctx->copy_stream && run.plan.dual();
  if (!run.ahead) return PWN_HIP_OK;
  const int nsub = (c.n + run.plan.sub - 1) / run.plan.sub;
  while ((int)ctx->sync_events.size() < 2 * nsub) {
    hipEvent_t e = nullptr;
    HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), PWN_HIP_ERR_ALLOCATION);
    ctx->sync_events.push_back(e);
  }
  HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->fork_ev, 0), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// Enqueue sub-batch k, the frames [base, base + m).  On its stream: its kernels, behind its host frames' copies (on the copy stream when they travel ahead).
int convert_enqueue_sub(pwn_hip_ctx* ctx, const ConvertCall& c, ConvertRun& run, int base, int k) {
  const ConvertJob& job = run.job;
  const int m = std::min(run.plan.sub, c.n - base), ns = run.plan.ns;
  hipStream_t st = run.plan.stream(k);
  if (job.host_input) {
    hipStream_t cs = run.ahead ? ctx->copy_stream : st;
    if (run.ahead && k >= ns) HIPCHK(ctx, hipStreamWaitEvent(cs, ctx->sync_events[2 * (k - ns) + 1], 0), PWN_HIP_ERR_LAUNCH);
    if (int rc = convert_stage_frames(ctx, job, base, m, cs)) return rc;
    if (run.ahead) {
      HIPCHK(ctx, hipEventRecord(ctx->sync_events[2 * k], cs), PWN_HIP_ERR_LAUNCH);
      HIPCHK(ctx, hipStreamWaitEvent(st, ctx->sync_events[2 * k], 0), PWN_HIP_ERR_LAUNCH);
    }
  }
  if (int rc = convert_enqueue(ctx, job, base, m, st, run.direct ? ctx->counts_host + c.n : nullptr)) return rc;
  if (run.ahead) HIPCHK(ctx, hipEventRecord(ctx->sync_events[2 * k + 1], st), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// One attempt at the call.  Prepare leaves the descriptor uploads on ctx->stream and the clouds replaced (the job withdraws them unless it
// commits); after the join everything is on ctx->stream again, and finish waits for it and commits.
int convert_batch_once(pwn_hip_ctx* ctx, const ConvertCall& call) {
  ConvertRun run;
  convert_plan_slots(ctx, call, run);
  if (int rc = convert_prepare(ctx, call, run.slot, run.direct, run.job)) return rc;
  if (int rc = plan_fork(ctx, run.plan)) return rc;
  if (int rc = convert_copy_ahead(ctx, call, run)) return rc;
  for (int base = 0, k = 0; base < call.n; base += run.plan.sub, ++k) { if (int rc = convert_enqueue_sub(ctx, call, run, base, k)) return rc; }
  if (int rc = plan_join(ctx, run.plan)) return rc;
  return convert_finish(ctx, run.job);
}
// The call; and once more after a hand-over time-out.  A strip waited for its left neighbour longer than the poll bound (~1 s): the neighbour's
// workgroup was not dispatched in time -- a device shared with another process's long kernels -- and the planes of this call are invalid.
// Nothing is left behind (epoch-tagged words), so the call is simply made again, once; a second time-out is reported.
int convert_batch_impl(pwn_hip_ctx* ctx, const ConvertCall& call) {
  if (int rc = convert_check(ctx, call)) return rc;
  return repeat_once(ctx, kHandoverTimeout, [&](bool) { return convert_batch_once(ctx, call); });
}

// pwn_hip_debug_front_end: one launch of launch_front_end over n frames prepared as a convert call prepares them (frame i in workspace slot i),
// and what it wrote copied back per frame.  No stats pass, no repeat after a time-out.
int debug_front_end_impl(pwn_hip_ctx* ctx, const ConvertCall& call, bool single_pass, int lean, float* integral_out, int* index_out, int* interval_out,
                         int* rowoff_out) {
  const int n = call.n, rows = call.rows, cols = call.cols; pwn_hip_cloud* const* clouds = call.clouds;
  if (int rc = check_frames_and_clouds(ctx, call.frames, clouds, n)) return rc;
  ctx->stages.clear();
  std::vector<int> slot((size_t)n);
  for (int i = 0; i < n; ++i) slot[i] = i;
  const bool direct = !single_pass && n < kSinglePassMinFrames;      // as convert_plan_slots decides for a call of n frames in one launch
  ConvertJob job;
  if (int rc = convert_prepare(ctx, call, slot, direct, job)) return rc;
  if (job.host_input) { if (int rc = convert_stage_frames(ctx, job, 0, n, ctx->stream)) return rc; }
  if (!single_pass) no_strip_tables(job, 0, n);
  if (lean == PWN_HIP_FRONT_END_LEAN_PLANES) job.cp.lean = 1;      // ten planes; PWN_HIP_FRONT_END_LEAN_GROUPED keeps convert_prepare's kLeanGrouped and
                                                                   // integral_out receives the slot as stored (three arrays of records, ig_at)
  // The one thing queued here that a convert call does not queue (there k_stats writes normals and matrices): with lean = 0 the clouds get points
  // only, so their previous normals and matrices are cleared instead of staying readable next to the new points.  Two memsets per cloud ahead of
  // the kernels; the kernels, their grids and their arguments are the convert call's.
  if (!lean) for (int i = 0; i < n; ++i) {
    HIPCHK(ctx, hipMemsetAsync(clouds[i]->d.Nc, 0, sizeof(float4) * (size_t)clouds[i]->d.capacity, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemsetAsync(clouds[i]->d.Om, 0, sizeof(float) * clouds[i]->front.Om.cap, ctx->stream), PWN_HIP_ERR_COPY);
  }
  if (int rc = launch_front_end(ctx, job.cp, 0, n, ctx->stream, single_pass, direct ? ctx->counts_host + n : nullptr)) return rc;
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  const size_t N = job.N, noff = (size_t)rows * (size_t)(single_pass ? strips_of(cols) : 1);
  for (int i = 0; i < n; ++i) {
    const FrameDesc& f = ctx->frames_host[i];
    HIPCHK(ctx, copy_any(integral_out + (size_t)i * N * kIntegralChannels, f.integral, N * kIntegralChannels * sizeof(float), ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, copy_any(index_out + (size_t)i * N, f.index, N * sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, copy_any(rowoff_out + (size_t)i * noff, f.rowoff, noff * sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);
    if (!lean) HIPCHK(ctx, copy_any(interval_out + (size_t)i * N, f.interval, N * sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);
  }
  if (!lean) return convert_finish(ctx, job);
  // a lean front end stores no points: counts and fault flag are digested and the job ends without a commit, its clouds empty
  if (int rc = sync_counts(ctx, n, direct)) return rc;
  return counts_check(ctx, clouds, n);
}

// DepthImage_scale of the call's n equal-sized frames (frames, raw, depth_scale, n and scale of `c`; its rows, cols and clouds are not looked at):
// chunks of at most max_batch frames, one box launch each; host sources are staged in the slots' source-size workspaces, host destinations leave
// through the slots' scaled frames.  dst == nullptr (check_scaled_capacities): the images stay in the slots and only valid[i], the pixels of
// image i inside the converter's [min_distance, max_distance], comes back.
int depth_scale_batch_impl(pwn_hip_ctx* ctx, const ConvertCall& c, float* const* dst, int* valid = nullptr) {
  const void* const* src = c.frames; const int n = c.n; const bool raw = c.raw; const ScaleSpec& sc = c.scale;
  for (int i = 0; i < n; ++i) if (!src[i] || (dst && !dst[i])) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null frame");
  if (int rc = absorb_copies(ctx)) return rc;
  if (int rc = ensure_scale(ctx, std::min(n, ctx->max_batch))) return rc;
  ctx->stages.clear();
  const float min_d = valid ? c.p->min_distance : 0.f, max_d = valid ? c.p->max_distance : 0.f;
  const size_t sbytes = (size_t)sc.srows * sc.scols * (raw ? sizeof(uint16_t) : sizeof(float)), obytes = (size_t)sc.orows * sc.ocols * sizeof(float);
  for (int base = 0; base < n; base += ctx->max_batch) {
    const int m = std::min(ctx->max_batch, n - base);
    for (int j = 0; j < m; ++j) {
      ScaleDesc& d = ctx->scale_host[j];
      d.src = src[base + j]; d.dst = dst ? dst[base + j] : nullptr;
      if (!is_device_ptr(d.src)) {
        void* ws = raw ? (void*)(ctx->raw_ws + (size_t)j * ctx->N) : (void*)(ctx->depth_ws + (size_t)j * ctx->N);
        HIPCHK(ctx, hipMemcpyAsync(ws, d.src, sbytes, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
        d.src = ws;
      }
      if (!is_device_ptr(d.dst)) d.dst = ctx->scaled_ws + (size_t)j * ctx->N;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->scale_dev, ctx->scale_host, sizeof(ScaleDesc) * m, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    if (int rc = launch_depth_scale(ctx, sc, raw, c.depth_scale, 0, m, ctx->stream)) return rc;
    for (int j = 0; j < m && dst; ++j)
      if (ctx->scale_host[j].dst != dst[base + j]) HIPCHK(ctx, hipMemcpyAsync(dst[base + j], ctx->scale_host[j].dst, obytes, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
    if (valid) {
      HIPCHK(ctx, hipMemsetAsync(ctx->counts_dev, 0, sizeof(int) * m, ctx->stream), PWN_HIP_ERR_COPY);
      const int on = sc.orows * sc.ocols;
      hipLaunchKernelGGL(k_count_in_range, dim3((unsigned)std::min((on + 255) / 256, 1024), (unsigned)m), dim3(256), 0, ctx->stream, ctx->scale_dev, on, min_d, max_d,
                         ctx->counts_dev);
      HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
      HIPCHK(ctx, hipMemcpyAsync(ctx->counts_host, ctx->counts_dev, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
    }
    HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);      // the descriptors and the slots are reused by the next chunk
    if (valid) std::copy(ctx->counts_host.p, ctx->counts_host.p + m, valid + base);
  }
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}
// A cloud too small for its frame's valid pixels is otherwise found when the kernels have written into it.  The *_scaled calls refuse before they
// touch a cloud: where a cloud holds fewer points than the scaled image has pixels, the frames are down-sampled and counted first (a pass of its
// own, only then).
int check_scaled_capacities(pwn_hip_ctx* ctx, const ConvertCall& c) {
  const ScaleSpec& sc = c.scale;
  bool tight = false;
  for (int i = 0; i < c.n; ++i) tight = tight || (size_t)c.clouds[i]->d.capacity < (size_t)sc.orows * sc.ocols;
  if (!tight) return PWN_HIP_OK;
  std::vector<int> valid((size_t)c.n);
  if (int rc = depth_scale_batch_impl(ctx, c, nullptr, valid.data())) return rc;
  for (int i = 0; i < c.n; ++i)
    if (valid[i] > c.clouds[i]->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity smaller than the number of valid depth pixels");
  return PWN_HIP_OK;
}
// n x makeCloud's data path (DepthImage_scale, then the conversion of the small image) inside the batch plan: the extra checks in front of
// convert_batch_impl.  `src` carries the size of the frames as the caller holds them; everything that can refuse the call is looked at before a
// cloud is touched.
int convert_batch_scaled_impl(pwn_hip_ctx* ctx, const ConvertCall& src, int step, float max_depth_cov) {
  if (!ctx || !src.p || !src.frames || !src.clouds || src.n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  ConvertCall call = src;
  if (int rc = make_scale_spec(ctx, src.rows, src.cols, step, max_depth_cov, call.scale)) return rc;
  call.rows = call.scale.orows; call.cols = call.scale.ocols;
  if (int rc = check_frames_and_clouds(ctx, call.frames, call.clouds, call.n)) return rc;
  if (int rc = check_scaled_capacities(ctx, call)) return rc;
  if (int rc = ensure_scale(ctx, call.n)) return rc;
  return convert_batch_impl(ctx, call);
}

// pwn_hip_debug_stats_from_integral and its lean form (`frames` given): the stats pass, launched as launch_convert launches it, on windows the
// caller supplies.  The clouds are replaced as a conversion replaces them; they end with the points they held (the index image must stay
// inside them), or lean, where k_stats writes the points, with max(index image) + 1 points inside their capacity.
int debug_stats_impl(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, int rows, int cols, int nframes, const float* integral, const int* index_image,
                     const int* interval_image, const void* const* frames, float depth_scale, pwn_hip_cloud* const* clouds, int keep_stats) {
  const bool lean = frames != nullptr, raw = depth_scale > 0.f;
  if (nframes < 1 || nframes > ctx->max_batch) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "nframes must be 1..max_batch");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (int rc = absorb_copies(ctx)) return rc;
  if (int rc = ensure_desc(ctx, nframes)) return rc;
  const size_t N = (size_t)rows * cols;
  ConvertParams cp = make_convert_params(ctx, p, nullptr, rows, cols, keep_stats);
  cp.lean = lean ? kLeanGrouped : 0;
  std::vector<int> npoints((size_t)nframes, 0);
  for (int i = 0; i < nframes; ++i) {
    const pwn_hip_cloud* c = clouds[i];
    if (!c || (lean && !frames[i])) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, lean ? "null frame or cloud" : "null cloud");
    if (c->d.omSym != clouds[0]->d.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "clouds of one call must share one omega storage (exact9 / sym6)");
    const int* idx = index_image + (size_t)i * N;
    const int limit = lean ? c->d.capacity : c->content.n;
    if (!lean) npoints[i] = c->content.n;
    for (size_t k = 0; k < N; ++k) {
      if (idx[k] >= limit)
        return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, lean ? "index image refers to a point beyond the cloud's capacity" : "index image refers to a point the cloud does not hold");
      if (lean && idx[k] >= npoints[i]) npoints[i] = idx[k] + 1;
    }
  }
  cp.omSym = clouds[0]->d.omSym;
  const OmegaNClasses cls = make_omega_n_classes(p);
  for (int i = 0; i < nframes; ++i) {
    pwn_hip_cloud* c = clouds[i];
    if (int rc = cloud_replace(ctx, c, keep_stats != 0, false, &cls)) return rc;
    fill_frame(ctx, i, i, nullptr, c->d);
    FrameDesc& f = ctx->frames_host[i];
    if (lean) {      // k_stats recomputes point and interval of every pixel from the staged frame, raw or float
      if (raw) { f.raw = ctx->raw_ws + (size_t)i * ctx->N; f.raw_scale = depth_scale; } else f.depth = ctx->depth_ws + (size_t)i * ctx->N;
      HIPCHK(ctx, hipMemcpyAsync(raw ? (void*)f.raw : (void*)f.depth, frames[i], N * (raw ? sizeof(uint16_t) : sizeof(float)), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    }
    HIPCHK(ctx, hipMemcpyAsync(f.index, index_image + (size_t)i * N, N * sizeof(int), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    if (!lean) HIPCHK(ctx, hipMemcpyAsync(f.interval, interval_image + (size_t)i * N, N * sizeof(int), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemcpyAsync(f.integral, integral + (size_t)i * N * kIntegralChannels, N * kIntegralChannels * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream), PWN_HIP_ERR_COPY);
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev, ctx->frames_host, sizeof(FrameDesc) * nframes, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  launch_stats(cp, ctx->frames_dev, nframes, ctx->stream);      // launch_convert's grid
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  for (int i = 0; i < nframes; ++i) cloud_commit(clouds[i], npoints[i]);
  return PWN_HIP_OK;
}

}  // namespace

// ================================================================================================================
extern "C" {

int pwn_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}
const char* pwn_hip_last_error_string(const pwn_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int pwn_hip_host_alloc(void** ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "bad host_alloc argument");
  *ptr = nullptr;
  hipError_t e = hipHostMalloc(ptr, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); *ptr = nullptr; return fail(nullptr, PWN_HIP_ERR_ALLOCATION, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
  return PWN_HIP_OK;
}
int pwn_hip_host_free(void* ptr) {
  if (!ptr) return PWN_HIP_OK;
  hipError_t e = hipHostFree(ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, std::string("hipHostFree: ") + hipGetErrorString(e)); }
  return PWN_HIP_OK;
}

int pwn_hip_device_alloc(pwn_hip_ctx* ctx, void** ptr, size_t bytes) {
  if (!ctx || !ptr || bytes == 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad device_alloc argument");
  *ptr = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  hipError_t e = hipMalloc(ptr, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); *ptr = nullptr; return fail(ctx, PWN_HIP_ERR_ALLOCATION, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  return PWN_HIP_OK;
}
int pwn_hip_device_free(pwn_hip_ctx* ctx, void* ptr) {
  if (!ptr) return PWN_HIP_OK;
  if (!ctx) {      // the context that allocated it is gone (and with it everything that could still use the buffer): plain hipFree, which
    hipError_t e = hipFree(ptr);      // waits for the device by itself
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, std::string("hipFree: ") + hipGetErrorString(e)); }
    return PWN_HIP_OK;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);       // nothing queued may still read or write it
  HIPCHK(ctx, hipFree(ptr), PWN_HIP_ERR_INVALID_ARGUMENT);
  return PWN_HIP_OK;
}
int pwn_hip_copy(pwn_hip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx || !dst || !src) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad copy argument");
  if (bytes == 0) return PWN_HIP_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;
  HIPCHK(ctx, copy_any(dst, src, bytes, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
int pwn_hip_device_memset(pwn_hip_ctx* ctx, void* ptr, int value, size_t bytes) {
  if (!ctx || (!ptr && bytes)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!bytes) return PWN_HIP_OK;
  if (!is_device_ptr(ptr)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "pwn_hip_device_memset: not a device pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  HIPCHK(ctx, hipMemsetAsync(ptr, value, bytes, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
int pwn_hip_copy_async(pwn_hip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx || !dst || !src) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad copy argument");
  if (bytes == 0) return PWN_HIP_OK;
  if (!ctx->copy_stream || !ctx->copy_ev) return pwn_hip_copy(ctx, dst, src, bytes);
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  HIPCHK(ctx, copy_any(dst, src, bytes, ctx->copy_stream), PWN_HIP_ERR_COPY);
  ctx->copy_pending = true;
  return PWN_HIP_OK;
}

void pwn_hip_default_converter_params(pwn_hip_converter_params* p) {
  std::memset(p, 0, sizeof(*p));
  const float K[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.5f, 0.5f, 1.f };   // pinholepointprojector.cpp:6-9
  std::memcpy(p->K, K, sizeof(K));
  p->min_distance = 0.01f; p->max_distance = 6.0f;
  p->world_radius = 0.1f; p->min_image_radius = 10; p->max_image_radius = 30; p->min_points = 50;
  p->stats_curvature_threshold = 0.02f; p->point_info_curvature_threshold = 0.02f; p->normal_info_curvature_threshold = 0.02f;
  p->point_flat_diag[0] = 1000.f; p->point_flat_diag[1] = 1.f; p->point_flat_diag[2] = 1.f;
  for (int i = 0; i < 3; ++i) { p->point_nonflat_diag[i] = 1.f; p->normal_flat_diag[i] = 100.f; p->normal_nonflat_diag[i] = 1.f; }
  const Mat4 I = mat4_identity();
  std::memcpy(p->sensor_offset, I.m, sizeof(I.m));
}
void pwn_hip_default_aligner_params(pwn_hip_aligner_params* p) {
  std::memset(p, 0, sizeof(*p));
  const float K[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.5f, 0.5f, 1.f };
  std::memcpy(p->K, K, sizeof(K));
  p->min_distance = 0.01f; p->max_distance = 6.0f;
  p->rows = 0; p->cols = 0;
  p->inlier_distance_threshold = 0.5f;
  p->inlier_normal_angular_threshold = (float)cos(M_PI / 6);
  p->flat_curvature_threshold = 0.02f; p->inlier_curvature_ratio_threshold = 1.3f;
  p->inlier_max_chi2 = 9e3f; p->robust_kernel = 1; p->outer_iterations = 10; p->inner_iterations = 1;
  const Mat4 I = mat4_identity();
  std::memcpy(p->reference_sensor_offset, I.m, sizeof(I.m));
  std::memcpy(p->current_sensor_offset, I.m, sizeof(I.m));
  std::memcpy(p->initial_guess, I.m, sizeof(I.m));
}

// high_priority: the streams of the look-ahead helper context that works beside BATCH calls (AsyncConvert::helper_hi).  Its one-frame jobs run beside
// streams that hold hundreds of queued launches; on the default priority a stream of the helper can share a hardware queue with one of those and is
// then served when that queue has drained -- at the end of the batch instead of beside it.  (Only for a context whose streams do not wait on other streams' events: a
// high-priority context used for the partition step's imports, which wait for a broadcast, made the whole step 8-13 % slower -- docs/experiments.md, round 6.)
static int ctx_create(pwn_hip_ctx** out, int device, int max_rows, int max_cols, int max_batch, bool high_priority);
int pwn_hip_ctx_create(pwn_hip_ctx** out, int device, int max_rows, int max_cols, int max_batch) { return ctx_create(out, device, max_rows, max_cols, max_batch, false); }
static hipError_t make_stream(hipStream_t* s, bool high_priority) {
  if (high_priority) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least && hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
// the workspaces of a context for max_batch images of N pixels; a failure leaves a half-built context that pwn_hip_ctx_destroy takes as it is
static int ctx_alloc(pwn_hip_ctx* ctx) {
  const size_t N = ctx->N, B = (size_t)ctx->max_batch;
  HIPCHK(ctx, ctx->depth_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->raw_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->index_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->interval_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->integral_ws.alloc(B * N * kIntegralChannels), PWN_HIP_ERR_ALLOCATION);
  {   // any rows x cols image with rows*cols <= N and rows, cols <= M: rows*strips <= N/64 + M, strips*bands <= N/1024 + M/64 + M/16 + 1
    const size_t M = (size_t)std::max(ctx->max_rows, ctx->max_cols);
    ctx->rowoff_slot = N / 64 + M + 64;
    ctx->carry_slot = (N / ((size_t)kIR_Cols * kIR_Rows) + M / kIR_Cols + M / kIR_Rows + 2) * (size_t)kII_Chains;
  }
  HIPCHK(ctx, ctx->rowoff_ws.alloc(B * ctx->rowoff_slot), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->carry_ws.alloc(B * ctx->carry_slot), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->fault_dev.alloc(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->align_fault_host.alloc(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->flat_hdr_host.alloc(256), PWN_HIP_ERR_ALLOCATION);
  *ctx->align_fault_host = 0;
  if (hipMemset(ctx->carry_ws, 0, B * ctx->carry_slot * sizeof(unsigned long long)) != hipSuccess || hipMemset(ctx->fault_dev, 0, sizeof(int)) != hipSuccess)
    return fail(ctx, PWN_HIP_ERR_ALLOCATION, "hipMemset of the hand-over workspace failed");
  HIPCHK(ctx, ctx->zref_ws.alloc(N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->z32ref_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->z32cur_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->curidx_ws.alloc(B * N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->partials_ws.alloc(B * (size_t)ctx->nblocks_max * kAccN), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->solve_dev.alloc(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->counters_dev.alloc(16), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->corr_ws.alloc(N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->scratch_count.alloc(1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->io_ws.alloc(N * 16), PWN_HIP_ERR_ALLOCATION);
  return ensure_desc(ctx, std::max(16, ctx->max_batch));
}
static int ctx_create(pwn_hip_ctx** out, int device, int max_rows, int max_cols, int max_batch, bool high_priority) {
  if (!out || max_rows <= 0 || max_cols <= 0 || max_batch <= 0) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "bad ctx_create argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(nullptr, PWN_HIP_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)"); }
  if (device < 0 || device >= ndev) return fail(nullptr, PWN_HIP_ERR_NO_DEVICE, "device index out of range");
  HIPCHK(nullptr, hipSetDevice(device), PWN_HIP_ERR_NO_DEVICE);
  pwn_hip_ctx* ctx = new pwn_hip_ctx();
  ctx->device = device; ctx->max_rows = max_rows; ctx->max_cols = max_cols; ctx->max_batch = max_batch;
  ctx->N = (size_t)max_rows * max_cols;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->num_cus = cus; }
  ctx->nblocks_max = align_nblocks((int)ctx->N);
  if (make_stream(&ctx->own_stream, high_priority) != hipSuccess) { delete ctx; return fail(nullptr, PWN_HIP_ERR_ALLOCATION, "hipStreamCreate failed"); }
  ctx->stream = ctx->own_stream;
  (void)make_stream(&ctx->stream2, high_priority);
  for (int k = 0; k < 2; ++k) { (void)make_stream(&ctx->extra[k], high_priority); (void)hipEventCreateWithFlags(&ctx->join_extra[k], hipEventDisableTiming); }
  (void)hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming); (void)hipEventCreateWithFlags(&ctx->join_ev, hipEventDisableTiming);
  (void)hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
  (void)hipEventCreateWithFlags(&ctx->copy_ev, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&ctx->foreign_ev, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&ctx->t0, hipEventDisableSystemFence); (void)hipEventCreateWithFlags(&ctx->t1, hipEventDisableSystemFence);
  if (int rc = ctx_alloc(ctx)) { std::string m = ctx->err; pwn_hip_ctx_destroy(ctx); return fail(nullptr, rc, m); }
  *out = ctx;
  return PWN_HIP_OK;
}
int pwn_hip_ctx_destroy(pwn_hip_ctx* ctx) {
  if (!ctx) return PWN_HIP_OK;
  (void)hipSetDevice(ctx->device);
  for (pwn_hip_tracker* tr : ctx->trackers) tracker_orphan(tr);
  ctx->trackers.clear();
  if (AsyncConvert* a = ctx->async) {       // a conversion still in flight finishes first; its result is dropped
    { std::unique_lock<std::mutex> lk(a->m); a->quit = true; }
    a->cv.notify_all();
    if (a->worker.joinable()) a->worker.join();
    if (a->helper) pwn_hip_ctx_destroy(a->helper);
    if (a->helper_hi) pwn_hip_ctx_destroy(a->helper_hi);
    delete a; ctx->async = nullptr;
  }
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);      // pwn_hip_copy_async transfers still in flight
  if (ctx->stream) (void)host_wait(ctx, ctx->stream);
  collect_stage_times(ctx);
  for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
  if (ctx->t0) (void)hipEventDestroy(ctx->t0);
  if (ctx->t1) (void)hipEventDestroy(ctx->t1);
  for (pwn_hip_cloud* r : ctx->cloud_pool) delete r;
  ctx->cloud_pool.clear();
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  for (int k = 0; k < 2; ++k) { if (ctx->extra[k]) (void)hipStreamDestroy(ctx->extra[k]); if (ctx->join_extra[k]) (void)hipEventDestroy(ctx->join_extra[k]); }
  if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
  if (ctx->copy_ev) (void)hipEventDestroy(ctx->copy_ev);
  if (ctx->foreign_ev) (void)hipEventDestroy(ctx->foreign_ev);
  for (hipEvent_t e : ctx->sync_events) (void)hipEventDestroy(e);
  ctx->sync_events.clear();
  if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
  if (ctx->join_ev) (void)hipEventDestroy(ctx->join_ev);
  // every workspace, descriptor array and mirror is a member that frees itself here: the context's device is current (set above; the helper
  // contexts live on the same one) and both streams were synchronised above, so nothing queued still uses them
  delete ctx;
  return PWN_HIP_OK;
}
int pwn_hip_ctx_set_stream(pwn_hip_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return PWN_HIP_OK;
}
int pwn_hip_ctx_wait_stream(pwn_hip_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (!ctx->foreign_ev) return fail(ctx, PWN_HIP_ERR_ALLOCATION, "no event");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  // everything the context queues from now on (its other streams fork from ctx->stream) runs after what the caller's stream holds now
  HIPCHK(ctx, hipEventRecord(ctx->foreign_ev, (hipStream_t)hip_stream), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->foreign_ev, 0), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_ctx_signal_stream(pwn_hip_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (!ctx->foreign_ev) return fail(ctx, PWN_HIP_ERR_ALLOCATION, "no event");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  // the mirror image of pwn_hip_ctx_wait_stream: what the caller queues on its stream from now on runs after everything the context has queued
  // so far (every batch call joins its streams back into ctx->stream before it packs its records)
  HIPCHK(ctx, hipEventRecord(ctx->foreign_ev, ctx->stream), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipStreamWaitEvent((hipStream_t)hip_stream, ctx->foreign_ev, 0), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_ctx_set_enqueued_callback(pwn_hip_ctx* ctx, void (*fn)(void*), void* user) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  ctx->enqueued_cb = fn; ctx->enqueued_user = fn ? user : nullptr;
  return PWN_HIP_OK;
}
int pwn_hip_ctx_synchronize(pwn_hip_ctx* ctx) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (int rc = absorb_copies(ctx)) return rc;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_ctx_set_subbatch(pwn_hip_ctx* ctx, int frames, int pairs) {
  if (!ctx || frames <= 0 || pairs <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad subbatch");
  ctx->sub_frames = std::min(frames, ctx->max_batch); ctx->sub_pairs = std::min(pairs, ctx->max_batch);
  return PWN_HIP_OK;
}
int pwn_hip_ctx_set_omega_storage(pwn_hip_ctx* ctx, int mode) {
  if (!ctx || (mode != PWN_HIP_OMEGA_EXACT9 && mode != PWN_HIP_OMEGA_SYM6)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "omega storage must be PWN_HIP_OMEGA_EXACT9 or PWN_HIP_OMEGA_SYM6");
  ctx->omega_sym = mode == PWN_HIP_OMEGA_SYM6 ? 1 : 0;
  return PWN_HIP_OK;
}
int pwn_hip_cloud_omega_storage(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, int* mode) {
  if (!c || !mode) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *mode = c->d.omSym ? PWN_HIP_OMEGA_SYM6 : PWN_HIP_OMEGA_EXACT9;
  return PWN_HIP_OK;
}
int pwn_hip_ctx_set_concurrency(pwn_hip_ctx* ctx, int streams) {
  if (!ctx || streams < 1 || streams > 4) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "streams must be 1..4");
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  ctx->concurrency = streams;
  return PWN_HIP_OK;
}
// Test hook for the strip hand-over of the converter's integral-image kernels: one hand-over word (strip, band, chain) of every
// frame is not written, so the chain to its right times out after `spin_limit` polls (0 = the default, ~1 s), the launch raises
// its fault flag and the convert call returns PWN_HIP_ERR_LAUNCH instead of hanging.  strip < 0 switches the hook off.
int pwn_hip_debug_withhold_carry(pwn_hip_ctx* ctx, int strip, int band, int chain, int rows, int spin_limit) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (strip < 0) { ctx->dbg_withhold = -1; ctx->spin_limit = kSpinLimit; ctx->dbg_withhold_once = 0; return PWN_HIP_OK; }
  if (band < 0 || chain < 0 || chain >= kII_Chains || rows <= 0 || band >= bands_of(rows)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad hand-over word");
  ctx->dbg_withhold = (strip * bands_of(rows) + band) * kII_Chains + chain;
  ctx->dbg_withhold_once = spin_limit < 0 ? 1 : 0;                  // negative: |spin_limit| polls, and only the next launch is disturbed
  ctx->spin_limit = spin_limit > 0 ? spin_limit : (spin_limit < 0 ? -spin_limit : kSpinLimit);
  return PWN_HIP_OK;
}
int pwn_hip_debug_convert_retries(pwn_hip_ctx* ctx, int* retries) {
  if (!ctx || !retries) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *retries = ctx->convert_retries;
  return PWN_HIP_OK;
}
// Test hook: 0 makes every alignment project both clouds in every iteration, also where a cloud's own index image is known to be that
// projection's result (the shortcut of align_describe_pairs) -- so that tests can hold the shortcut against the projection it replaces.
int pwn_hip_debug_set_index_shortcut(pwn_hip_ctx* ctx, int enabled) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  ctx->index_shortcut = enabled ? 1 : 0;
  return PWN_HIP_OK;
}
// Test hooks of the projection's fault path: the rounds a thread of k_project spends on a contended pixel before it gives up (0 = every
// collision gives up at once; < 0 = the default), and how many alignment calls were repeated with the two-pass projection so far.
int pwn_hip_debug_set_settle_guard(pwn_hip_ctx* ctx, int rounds) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  ctx->settle_guard = rounds < 0 ? kSettleGuard : rounds;
  return PWN_HIP_OK;
}
int pwn_hip_debug_host_waits(pwn_hip_ctx* ctx, int* waits) {
  if (!ctx || !waits) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *waits = ctx->host_waits;
  return PWN_HIP_OK;
}
int pwn_hip_debug_projection_fallbacks(pwn_hip_ctx* ctx, int* calls) {
  if (!ctx || !calls) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *calls = ctx->projection_fallbacks;
  return PWN_HIP_OK;
}
// Test hook: sub-batches of the last batch alignment whose fused pass took the current points from the depth frames (CurDepthSrc)
int pwn_hip_debug_cur_depth_sub_batches(pwn_hip_ctx* ctx, int* sub_batches) {
  if (!ctx || !sub_batches) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *sub_batches = ctx->cur_depth_subs;
  return PWN_HIP_OK;
}
// Test hook: those of them that also ranked the current indices from the clouds' strip offsets (CurDepthSrc::strips)
int pwn_hip_debug_strip_index_sub_batches(pwn_hip_ctx* ctx, int* sub_batches) {
  if (!ctx || !sub_batches) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *sub_batches = ctx->strip_index_subs;
  return PWN_HIP_OK;
}
// Test hook: the converter's stats pass (k_stats, launched as launch_convert launches it) on caller-supplied integral planes, index and
// interval images -- windows that no depth frame produces.  The clouds hold the points the index images refer to (pwn_hip_cloud_upload).
int pwn_hip_debug_stats_from_integral(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, int rows, int cols, int nframes, const float* integral,
                                      const int* index_image, const int* interval_image, pwn_hip_cloud* const* clouds, int keep_stats) {
  if (!ctx || !p || !integral || !index_image || !interval_image || !clouds) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  return debug_stats_impl(ctx, p, rows, cols, nframes, integral, index_image, interval_image, nullptr, 0.f, clouds, keep_stats);
}
// Test hook: the stats pass of a lean convert call (cp.lean = kLeanGrouped) on caller-supplied windows: the integral image arrives in the grouped
// form (ig_at: three arrays of records per slot), and k_stats recomputes point and interval of every pixel from the staged depth frame, float or
// raw, as it does behind the grouped front end.  The clouds give capacity only; k_stats writes their points.
int pwn_hip_debug_stats_from_integral_lean(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, int rows, int cols, int nframes, const float* integral,
                                           const int* index_image, const void* const* frames, float depth_scale, pwn_hip_cloud* const* clouds, int keep_stats) {
  if (!ctx || !p || !integral || !index_image || !frames || !clouds) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (depth_scale < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative depth scale");
  return debug_stats_impl(ctx, p, rows, cols, nframes, integral, index_image, nullptr, frames, depth_scale, clouds, keep_stats);
}
// Test hook: the front end of a convert call (launch_front_end, the function launch_convert itself calls) on the caller's frames, the path chosen
// by the caller instead of by the frame count, and everything it wrote handed back: planes, index images, offsets, and with lean = 0 the
// interval images and (in the clouds) the points.  k_stats is not launched.
int pwn_hip_debug_front_end(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const void* const* frames, float depth_scale, int nframes, int rows, int cols,
                            int path, int lean, pwn_hip_cloud* const* clouds, float* integral_out, int* index_out, int* interval_out, int* rowoff_out) {
  if (!ctx || !p || !frames || !clouds || !integral_out || !index_out || !rowoff_out) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (nframes < 1 || nframes > ctx->max_batch) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "nframes must be 1..max_batch");
  if (path != PWN_HIP_FRONT_END_LATENCY && path != PWN_HIP_FRONT_END_SINGLE_PASS) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "path must be 0 (latency) or 1 (single pass)");
  if (lean != PWN_HIP_FRONT_END_LEAN_OFF && lean != PWN_HIP_FRONT_END_LEAN_PLANES && lean != PWN_HIP_FRONT_END_LEAN_GROUPED)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "lean must be 0 (off), 1 (ten planes) or 2 (grouped records)");
  if (lean ? interval_out != nullptr : interval_out == nullptr)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, lean ? "a lean front end writes no interval image (and no points): interval_out must be null" : "null argument");
  if (depth_scale < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative depth scale");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (int rc = absorb_copies(ctx)) return rc;
  ConvertCall call; call.p = p; call.n = nframes; call.rows = rows; call.cols = cols; call.clouds = clouds;
  call.frames = frames; call.raw = depth_scale > 0.f; call.depth_scale = depth_scale; call.want_interval = lean == 0;
  return debug_front_end_impl(ctx, call, path == PWN_HIP_FRONT_END_SINGLE_PASS, lean, integral_out, index_out, interval_out, rowoff_out);
}
__global__ void __launch_bounds__(256) k_debug_trig(int n, const float* __restrict__ y, const float* __restrict__ x, float* __restrict__ theta,
                                                    float* __restrict__ c, float* __restrict__ s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  PWN_EIG3_TRIG(y[i], x[i], t, ct, st);      // the text eig3_direct expands
  theta[i] = t; c[i] = ct; s[i] = st;
}
// Test hook: PWN_EIG3_TRIG (the eigensolver's three trig values, as eig3_direct computes them) on the device for n host arguments
int pwn_hip_debug_trig_eval(pwn_hip_ctx* ctx, int n, const float* y, const float* x, float* theta, float* cos_theta, float* sin_theta) {
  if (!ctx || n < 0 || (n > 0 && (!y || !x || !theta || !cos_theta || !sin_theta))) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n == 0) return PWN_HIP_OK;
  DevBuf<float> d;
  const size_t bytes = (size_t)n * sizeof(float);
  HIPCHK(ctx, d.alloc(5 * (size_t)n), PWN_HIP_ERR_ALLOCATION);
  hipError_t e = hipMemcpy(d, y, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_trig, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, d + 4 * (size_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(theta, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cos_theta, d + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(sin_theta, d + 4 * (size_t)n, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(ctx, PWN_HIP_ERR_LAUNCH, std::string("trig eval: ") + hipGetErrorString(e));
  return PWN_HIP_OK;
}
// Test hook: the shipped k_pair_statistics on n injected systems (H: n x 36 column-major, T: n x 16 column-major) through the context's own pair
// arrays; out: n x 44 = omega[36], mean[6], the translational and the rotational eigen ratio
int pwn_hip_debug_statistics_eval(pwn_hip_ctx* ctx, int n, const float* H, const float* T, float* out) {
  if (!ctx || n < 0 || (n > 0 && (!H || !T || !out))) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n == 0) return PWN_HIP_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = ensure_desc(ctx, n)) return rc;
  ctx->img.invalidate(); ctx->last_pairs = 0;      // the pair arrays of the last alignment are overwritten
  for (int i = 0; i < n; ++i) {
    std::memset(&ctx->pairs_host[i], 0, sizeof(PairDesc));
    ctx->pairs_host[i].state = ctx->state_ws + i;
    std::memset(&ctx->state_host[i], 0, sizeof(PairState));
    std::memcpy(ctx->state_host[i].T.m, T + 16 * (size_t)i, sizeof(float) * 16);
    std::memset(&ctx->stats_host[i], 0, sizeof(SolveOut));
    std::memcpy(ctx->stats_host[i].H, H + 36 * (size_t)i, sizeof(float) * 36);
  }
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(ctx->pairs_dev, ctx->pairs_host, sizeof(PairDesc) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->state_ws, ctx->state_host, sizeof(PairState) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->stats_dev, ctx->stats_host, sizeof(SolveOut) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_pair_statistics, dim3(n), dim3(64), 0, st, ctx->pairs_dev, (const SolveOut*)ctx->stats_dev, ctx->pairstats_dev);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipMemcpyAsync(ctx->pairstats_host, ctx->pairstats_dev, sizeof(PairStats) * n, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  for (int i = 0; i < n; ++i) std::memcpy(out + 44 * (size_t)i, &ctx->pairstats_host[i], sizeof(float) * 44);
  return PWN_HIP_OK;
}
int pwn_hip_set_profiling(pwn_hip_ctx* ctx, int enabled) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  ctx->profiling = enabled != 0;
  return PWN_HIP_OK;
}
// ---- what the box's HBM delivers (the measured figure next to the 8 TB/s spec) ---------------------------------
// float4 streaming kernels, 2048 workgroups x 256 threads, grid-stride with four independent loads in flight per thread
__global__ void __launch_bounds__(256) k_probe_read(const v4f* __restrict__ src, size_t n4, float* __restrict__ sink) {
  const size_t stride = (size_t)gridDim.x * 256;
  v4f a = { 0.f, 0.f, 0.f, 0.f }, b = a, c = a, d = a;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const v4f x0 = __builtin_nontemporal_load(src + i), x1 = __builtin_nontemporal_load(src + i + stride);
    const v4f x2 = __builtin_nontemporal_load(src + i + 2 * stride), x3 = __builtin_nontemporal_load(src + i + 3 * stride);
    a.x += x0.x; a.y += x0.y; a.z += x0.z; a.w += x0.w; b.x += x1.x; b.y += x1.y; b.z += x1.z; b.w += x1.w;
    c.x += x2.x; c.y += x2.y; c.z += x2.z; c.w += x2.w; d.x += x3.x; d.y += x3.y; d.z += x3.z; d.w += x3.w;
  }
  for (; i < n4; i += stride) { const v4f x0 = src[i]; a.x += x0.x; a.y += x0.y; a.z += x0.z; a.w += x0.w; }
  const float s = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w));
  if (s == 123456.789f) sink[0] = s;          // never true for the zero-filled buffer: keeps the loads alive
}
__global__ void __launch_bounds__(256) k_probe_copy(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 x0 = src[i], x1 = src[i + stride], x2 = src[i + 2 * stride], x3 = src[i + 3 * stride];
    dst[i] = x0; dst[i + stride] = x1; dst[i + 2 * stride] = x2; dst[i + 3 * stride] = x3;
  }
  for (; i < n4; i += stride) dst[i] = src[i];
}
int pwn_hip_measure_hbm(pwn_hip_ctx* ctx, size_t bytes, float* read_gbps, float* copy_gbps) {
  if (!ctx || bytes < (1u << 20)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx or fewer than 1 MiB");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  const size_t n4 = bytes / sizeof(float4);
  DevBuf<float4> src, dst;
  HIPCHK(ctx, src.alloc(n4), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, dst.alloc(n4), PWN_HIP_ERR_ALLOCATION);
  hipStream_t st = ctx->stream;
  (void)hipMemsetAsync(src, 0, n4 * sizeof(float4), st); (void)hipMemsetAsync(dst, 0, n4 * sizeof(float4), st);
  float best_r = 1e30f, best_c = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {
    float ms = 0.f;
    (void)hipEventRecord(ctx->t0, st);
    hipLaunchKernelGGL(k_probe_read, dim3(2048), dim3(256), 0, st, (const v4f*)src.p, n4, (float*)dst.p);
    (void)hipEventRecord(ctx->t1, st); (void)hipEventSynchronize(ctx->t1); (void)hipEventElapsedTime(&ms, ctx->t0, ctx->t1);
    if (rep > 0 && ms < best_r) best_r = ms;
    (void)hipEventRecord(ctx->t0, st);
    hipLaunchKernelGGL(k_probe_copy, dim3(2048), dim3(256), 0, st, src, dst, n4);
    (void)hipEventRecord(ctx->t1, st); (void)hipEventSynchronize(ctx->t1); (void)hipEventElapsedTime(&ms, ctx->t0, ctx->t1);
    if (rep > 0 && ms < best_c) best_c = ms;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, PWN_HIP_ERR_LAUNCH, hipGetErrorString(e));
  const double b = (double)n4 * sizeof(float4);
  if (read_gbps) *read_gbps = (float)(b / (best_r * 1e-3) / 1e9);
  if (copy_gbps) *copy_gbps = (float)(2.0 * b / (best_c * 1e-3) / 1e9);
  return PWN_HIP_OK;
}
int pwn_hip_last_stage_ms(pwn_hip_ctx* ctx, const char* stage, float* ms, int* launches) {
  if (!ctx || !stage) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  auto it = ctx->stages.find(stage);
  if (ms) *ms = it == ctx->stages.end() ? 0.f : it->second.ms;
  if (launches) *launches = it == ctx->stages.end() ? 0 : it->second.launches;
  return PWN_HIP_OK;
}

// ---------------------------------------------------------------------------------------------------- clouds
int pwn_hip_cloud_create(pwn_hip_ctx* ctx, int capacity, pwn_hip_cloud** out) {
  if (!ctx || !out || capacity <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad cloud_create argument");
  if (capacity > kMaxCloudPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "a cloud holds at most 2^25 points (index field of the scene stage's z-buffer word)");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  for (size_t k = 0; k < ctx->cloud_pool.size(); ++k) {
    pwn_hip_cloud* r = ctx->cloud_pool[k];
    if (r->d.capacity != capacity || r->d.omSym != ctx->omega_sym) continue;
    ctx->cloud_pool.erase(ctx->cloud_pool.begin() + (long)k);
    ctx->cloud_pool_bytes -= r->core_bytes();
    HIPCHK(ctx, hipMemsetAsync(r->d.count, 0, sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);      // stream order: after whatever used the retired cloud
    r->owner = ctx;
    *out = r;
    return PWN_HIP_OK;
  }
  pwn_hip_cloud* c = new pwn_hip_cloud();
  c->d.capacity = capacity;
  c->d.omSym = ctx->omega_sym;
  c->owner = ctx;
  hipError_t e = c->own(kArrCore);
  if (e == hipSuccess) e = hipMemsetAsync(c->d.count, 0, sizeof(int), ctx->stream);
  if (e != hipSuccess) { pwn_hip_cloud_destroy(ctx, c); return fail(ctx, PWN_HIP_ERR_ALLOCATION, std::string("cloud allocation: ") + hipGetErrorString(e)); }
  *out = c;
  return PWN_HIP_OK;
}
int pwn_hip_cloud_destroy(pwn_hip_ctx* ctx, pwn_hip_cloud* c) {
  if (!c) return PWN_HIP_OK;
  if (ctx && ctx->async && ctx->async->cloud == c) (void)pwn_hip_convert_end(ctx, c);      // a conversion into this cloud is still in flight
  cloud_changes(ctx, c);
  // plain clouds (no scene-stage or uploaded extras) retire into the context's pool: every call that used them has joined its streams
  // back into ctx->stream before returning, and a reuse is enqueued on that stream
  if (ctx && c->plain() && ctx->cloud_pool_bytes + c->core_bytes() <= kCloudPoolBytes) {
    (void)cloud_replace(ctx, c, false, false, nullptr);      // a plain cloud: nothing to allocate, no planes to wait for
    ctx->cloud_pool.push_back(c);
    ctx->cloud_pool_bytes += c->core_bytes();
    return PWN_HIP_OK;
  }
  if (ctx) (void)host_wait(ctx, ctx->stream);
  delete c;
  return PWN_HIP_OK;
}
int pwn_hip_cloud_size(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, int* n) {
  if (!c || !n) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *n = c->content.n;
  return PWN_HIP_OK;
}
int pwn_hip_cloud_upload(pwn_hip_ctx* ctx, pwn_hip_cloud* c, int n, const float* points, const float* normals, const float* curvature,
                         const float* omega_p, const float* omega_n) {
  if (!ctx || !c || n < 0 || !points || !normals || !curvature || !omega_p || !omega_n) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n > c->d.capacity) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity too small");
  if (int rc = absorb_copies(ctx)) return rc;     // caller pointers may be the destination of a queued pwn_hip_copy_async
  // repack on the host into the device layout (upload is not on the hot path)
  std::vector<float> hp((size_t)n * 4), hn((size_t)n * 4), hc(n), hop((size_t)n * 16), hon((size_t)n * 16);
  HIPCHK(ctx, copy_any(hp.data(), points, hp.size() * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(hn.data(), normals, hn.size() * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(hc.data(), curvature, hc.size() * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(hop.data(), omega_p, hop.size() * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(hon.data(), omega_n, hon.size() * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_COPY);
  const size_t cap = (size_t)c->d.capacity;
  const int sym = c->d.omSym;
  std::vector<float> P((size_t)n * 4), Nm((size_t)n * 4), Om(c->front.Om.cap, 0.f), OmN(cap * 9, 0.f);
  for (int i = 0; i < n; ++i) {
    P[4 * i] = hp[4 * i]; P[4 * i + 1] = hp[4 * i + 1]; P[4 * i + 2] = hp[4 * i + 2]; P[4 * i + 3] = hc[i];
    Nm[4 * i] = hn[4 * i]; Nm[4 * i + 1] = hn[4 * i + 1]; Nm[4 * i + 2] = hn[4 * i + 2];
    const int one = 1; std::memcpy(&Nm[4 * i + 3], &one, 4);
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) {
      if (!(sym && om_is_lower(3 * r + q))) Om[omp_at(cap, i, 3 * r + q, sym)] = hop[(size_t)16 * i + r + 4 * q];      // column-major 4x4 -> entry (r,q); sym6 keeps the upper triangle
      OmN[om_at(cap, i, 3 * r + q)] = hon[(size_t)16 * i + r + 4 * q];
    }
  }
  if (int rc = cloud_replace(ctx, c, false, true, nullptr)) return rc;      // replace: points with explicit Omega_n planes, no Stats
  if (int rc = cloud_store_records(ctx, c->d, n, P, Nm)) return rc;
  HIPCHK(ctx, hipMemcpy(c->d.Om, Om.data(), Om.size() * 4, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpy(c->d.OmN, OmN.data(), OmN.size() * 4, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpy(c->d.count, &n, sizeof(int), hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  cloud_commit(c, n);
  return PWN_HIP_OK;
}
int pwn_hip_cloud_download(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, float* points, float* normals, float* curvature, float* omega_p, float* omega_n) {
  if (!ctx || !c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int n = c->content.n; const size_t cap = (size_t)c->d.capacity;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  std::vector<float> P, Nm;
  if (int rc = cloud_fetch_records(ctx, c->d, n, P, Nm)) return rc;
  std::vector<float> hp, hn, hc, hop, hon;
  if (points) { hp.resize((size_t)n * 4); for (int i = 0; i < n; ++i) { hp[4*i] = P[4*i]; hp[4*i+1] = P[4*i+1]; hp[4*i+2] = P[4*i+2]; hp[4*i+3] = 1.0f; } }
  if (normals) { hn.resize((size_t)n * 4); for (int i = 0; i < n; ++i) { hn[4*i] = Nm[4*i]; hn[4*i+1] = Nm[4*i+1]; hn[4*i+2] = Nm[4*i+2]; hn[4*i+3] = 0.0f; } }
  if (curvature) { hc.resize(n); for (int i = 0; i < n; ++i) hc[i] = P[4*i+3]; }
  if (omega_p || omega_n) {
    std::vector<float> Om(c->front.Om.cap), OmN;
    HIPCHK(ctx, hipMemcpy(Om.data(), c->d.Om, Om.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
    if (c->d.OmN) { OmN.resize(cap * 9); HIPCHK(ctx, hipMemcpy(OmN.data(), c->d.OmN, OmN.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY); }
    if (omega_p) hop.assign((size_t)n * 16, 0.f);
    if (omega_n) hon.assign((size_t)n * 16, 0.f);
    for (int i = 0; i < n; ++i) {
      int cls; std::memcpy(&cls, &Nm[4 * i + 3], 4); cls &= kClsMask;
      for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) {
        if (omega_p) hop[(size_t)16 * i + r + 4 * q] = Om[omp_at(cap, i, 3 * r + q, c->d.omSym)];      // sym6: the stored upper triangle, mirrored
        if (omega_n) {
          float v = 0.f;
          if (c->d.OmN) v = OmN[om_at(cap, i, 3 * r + q)];
          else if (cls == 1) v = c->d.omN[0][3 * r + q];
          else if (cls == 2) v = c->d.omN[1][3 * r + q];
          hon[(size_t)16 * i + r + 4 * q] = v;
        }
      }
    }
  }
  if (points) HIPCHK(ctx, hipMemcpy(points, hp.data(), hp.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (normals) HIPCHK(ctx, hipMemcpy(normals, hn.data(), hn.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (curvature) HIPCHK(ctx, hipMemcpy(curvature, hc.data(), hc.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (omega_p) HIPCHK(ctx, hipMemcpy(omega_p, hop.data(), hop.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (omega_n) HIPCHK(ctx, hipMemcpy(omega_n, hon.data(), hon.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
int pwn_hip_cloud_download_stats(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, float* stats, float* eigenvalues, int* npoints) {
  if (!ctx || !c) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!c->content.stats || !c->d.St) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud was not converted with keep_stats");
  const int n = c->content.n;
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  std::vector<float> St((size_t)n * 16);
  HIPCHK(ctx, hipMemcpy(St.data(), c->d.St, St.size() * 4, hipMemcpyDeviceToHost), PWN_HIP_ERR_COPY);
  std::vector<float> hs, he; std::vector<int> hn;
  if (stats) hs.assign((size_t)n * 16, 0.f);
  if (eigenvalues) he.resize((size_t)n * 3);
  if (npoints) hn.resize(n);
  for (int i = 0; i < n; ++i) {
    float S[16], ev[3]; int npts;
    stats_unpack(&St[(size_t)16 * i], S, ev, &npts);
    if (stats) std::memcpy(&hs[(size_t)16 * i], S, sizeof(S));
    if (eigenvalues) std::memcpy(&he[(size_t)3 * i], ev, sizeof(ev));
    if (npoints) hn[i] = npts;
  }
  if (stats) HIPCHK(ctx, hipMemcpy(stats, hs.data(), hs.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (eigenvalues) HIPCHK(ctx, hipMemcpy(eigenvalues, he.data(), he.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (npoints) HIPCHK(ctx, hipMemcpy(npoints, hn.data(), hn.size() * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
int pwn_hip_cloud_transform_in_place(pwn_hip_ctx* ctx, pwn_hip_cloud* c, const float T[16]) {
  if (!ctx || !c || !T) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const Mat4 m = forced(T);
  if (is_identity(m)) return PWN_HIP_OK;                       // cloud.cpp:176
  cloud_changes(ctx, c);
  if (!c->d.OmN) for (int k = 0; k < 2; ++k) transform_omega(m, c->d.omN[k]);      // class matrices transform with the cloud
  if (int rc = cloud_edit(ctx, c, c->content.n, false)) return rc;                 // edit: the same points, moved
  hipLaunchKernelGGL(k_cloud_transform, dim3((c->d.capacity + 255) / 256), dim3(256), 0, ctx->stream, c->d, m);
  {   // StatsVector / Gaussian3fVector::transformInPlace (stats.h:125-131, gaussian3.h:65-73)
    const CloudView v = c->view();
    const int cnt = std::max(v.n, v.gauss);
    if (cnt > 0 && (v.d.St || v.gauss > 0)) hipLaunchKernelGGL(k_scene_transform, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, v.d, v.sb, v.n, v.gauss, m);
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}

// ---- a cloud as ONE flat buffer (replication of a cloud to the other GPUs of a node: PwnCloser::processPartition matches one `current` cloud
// against every cloud of the other partition, pwn_tracker/pwn_closer.cpp:85-111; SURVEY.md 8(e): "replicate current's cloud to all GPUs") ----
namespace {
struct CloudFlatHeader {            // 256 bytes; sections start at multiples of 256 bytes
  uint32_t magic, version;
  int32_t n, omSym, hasOmN, idxValid, idxRows, idxCols;
  float clsThr, idxMinD, idxMaxD;
  float omN[2][9];
  float idxK[9];
  uint64_t offP3, offNc, offOm, offOmN, offIdx, total;
  unsigned char pad[256 - (8 * 4 + 3 * 4 + 18 * 4 + 9 * 4 + 6 * 8)];
};
static_assert(sizeof(CloudFlatHeader) == 256, "flat cloud header");
constexpr uint32_t kFlatMagic = 0x464E5750u;      // "PWNF"
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
// section offsets for n points (plane stride inside the flat buffer = n points, not the cloud's capacity)
void flat_layout(CloudFlatHeader& h, size_t n, int omSym, bool omN, size_t idxPixels) {
  size_t o = sizeof(CloudFlatHeader);
  h.offP3 = o; o += up256(n * 12);
  h.offNc = o; o += up256(n * 16);
  h.offOm = o; o += (size_t)om_planes(omSym) * up256(n * 12);
  h.offOmN = o; if (omN) o += 3 * up256(n * 12);
  h.offIdx = o; o += up256(idxPixels * 4);
  h.total = o;
}
}  // namespace
size_t pwn_hip_cloud_export_bound(int capacity, int omega_storage, int index_pixels, int with_omega_n) {
  if (capacity < 0 || index_pixels < 0) return 0;
  CloudFlatHeader h;
  flat_layout(h, (size_t)capacity, omega_storage == PWN_HIP_OMEGA_SYM6 ? 1 : 0, with_omega_n != 0, (size_t)index_pixels);
  return (size_t)h.total;
}
int pwn_hip_cloud_export(pwn_hip_ctx* ctx, const pwn_hip_cloud* c, void* dst, size_t dst_bytes, size_t* written) {
  if (!ctx || !c || (!dst && !written)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  const size_t n = (size_t)std::min(c->content.n, c->d.capacity), cap = (size_t)c->d.capacity;
  // the header is staged in page-locked memory of the context: the copy below is asynchronous, and an error return further down must not
  // leave it reading a dead stack frame
  CloudFlatHeader& h = *(CloudFlatHeader*)ctx->flat_hdr_host.p; std::memset(&h, 0, sizeof(h));
  h.magic = kFlatMagic; h.version = 1; h.n = (int32_t)n; h.omSym = c->d.omSym; h.hasOmN = c->d.OmN ? 1 : 0;
  h.clsThr = c->d.clsThr; std::memcpy(h.omN, c->d.omN, sizeof(h.omN));
  const IndexKey& key = c->content.idx_key;
  const bool idx = c->content.idx_valid && c->idximg && (size_t)key.rows * key.cols <= c->idximg.cap;
  h.idxValid = idx ? 1 : 0; h.idxRows = idx ? key.rows : 0; h.idxCols = idx ? key.cols : 0;
  h.idxMinD = key.minD; h.idxMaxD = key.maxD; std::memcpy(h.idxK, key.K, sizeof(h.idxK));
  const size_t npx = idx ? (size_t)key.rows * key.cols : 0;
  flat_layout(h, n, c->d.omSym, c->d.OmN != nullptr, npx);
  if (written) *written = (size_t)h.total;
  if (!dst) return PWN_HIP_OK;                                   // size query
  if (dst_bytes < h.total) return fail(ctx, PWN_HIP_ERR_CAPACITY, "flat cloud buffer too small (pwn_hip_cloud_export_bound)");
  char* out = (char*)dst; hipStream_t st = ctx->stream;
  HIPCHK(ctx, copy_any(out, &h, sizeof(h), st), PWN_HIP_ERR_COPY);
  if (n > 0) {
    HIPCHK(ctx, copy_section(out + h.offP3, c->d.P3, n * 12, st), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, copy_section(out + h.offNc, c->d.Nc, n * 16, st), PWN_HIP_ERR_COPY);
    for (int r = 0; r < om_planes(c->d.omSym); ++r)
      HIPCHK(ctx, copy_section(out + h.offOm + (size_t)r * up256(n * 12), c->d.Om + (size_t)r * cap * 3, n * 12, st), PWN_HIP_ERR_COPY);
    if (c->d.OmN) for (int r = 0; r < 3; ++r)
      HIPCHK(ctx, copy_section(out + h.offOmN + (size_t)r * up256(n * 12), c->d.OmN + (size_t)r * cap * 3, n * 12, st), PWN_HIP_ERR_COPY);
  }
  if (npx > 0) HIPCHK(ctx, copy_section(out + h.offIdx, c->idximg, npx * 4, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_COPY);      // the buffer is complete on return
  return PWN_HIP_OK;
}
int pwn_hip_cloud_import(pwn_hip_ctx* ctx, pwn_hip_cloud* c, const void* src, size_t src_bytes) {
  if (!ctx || !c || !src) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (src_bytes < sizeof(CloudFlatHeader)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "flat cloud buffer shorter than its header");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;
  hipStream_t st = ctx->stream;
  CloudFlatHeader h;
  HIPCHK(ctx, copy_any(&h, src, sizeof(h), st), PWN_HIP_ERR_COPY);      // on the context's stream: ordered after pwn_hip_ctx_wait_stream
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_COPY);
  if (h.magic != kFlatMagic || h.version != 1 || h.n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "not a flat cloud buffer (pwn_hip_cloud_export)");
  CloudFlatHeader want; std::memset(&want, 0, sizeof(want));
  const bool idx = h.idxValid != 0 && h.idxRows > 0 && h.idxCols > 0;
  const size_t n = (size_t)h.n, npx = idx ? (size_t)h.idxRows * h.idxCols : 0, cap = (size_t)c->d.capacity;
  flat_layout(want, n, h.omSym ? 1 : 0, h.hasOmN != 0, npx);
  if (want.offP3 != h.offP3 || want.offNc != h.offNc || want.offOm != h.offOm || want.offOmN != h.offOmN || want.offIdx != h.offIdx || want.total != h.total)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "flat cloud buffer: inconsistent header");
  if (src_bytes < h.total) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "flat cloud buffer shorter than its header says");
  if (n > cap) return fail(ctx, PWN_HIP_ERR_CAPACITY, "cloud capacity smaller than the flat cloud");
  if ((h.omSym ? 1 : 0) != c->d.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "flat cloud and destination cloud differ in omega storage (exact9 / sym6)");
  // replace: from here on the destination's previous content is being overwritten and it reads as EMPTY (host size and device count) until every
  // section has arrived, so that a copy that fails half way leaves an empty cloud behind, not a mixture with the old sizes
  OmegaNClasses cls; std::memcpy(cls.omN, h.omN, sizeof(h.omN)); cls.clsThr = h.clsThr;
  if (int rc = cloud_replace(ctx, c, false, h.hasOmN != 0, &cls)) return rc;
  HIPCHK(ctx, hipMemsetAsync(c->d.count, 0, sizeof(int), st), PWN_HIP_ERR_COPY);
  CloudFlatHeader& hp = *(CloudFlatHeader*)ctx->flat_hdr_host.p; hp = h;      // page-locked copy: source of the asynchronous count copy below
  if (idx) HIPCHK(ctx, c->idximg.ensure(npx), PWN_HIP_ERR_ALLOCATION);
  const char* in = (const char*)src;
  if (n > 0) {
    HIPCHK(ctx, copy_section(c->d.P3, in + h.offP3, n * 12, st), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, copy_section(c->d.Nc, in + h.offNc, n * 16, st), PWN_HIP_ERR_COPY);
    for (int r = 0; r < om_planes(c->d.omSym); ++r)
      HIPCHK(ctx, copy_section(c->d.Om + (size_t)r * cap * 3, in + h.offOm + (size_t)r * up256(n * 12), n * 12, st), PWN_HIP_ERR_COPY);
    if (h.hasOmN) for (int r = 0; r < 3; ++r)
      HIPCHK(ctx, copy_section(c->d.OmN + (size_t)r * cap * 3, in + h.offOmN + (size_t)r * up256(n * 12), n * 12, st), PWN_HIP_ERR_COPY);
  }
  if (idx) HIPCHK(ctx, copy_section(c->idximg, in + h.offIdx, npx * 4, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(c->d.count, &hp.n, sizeof(int), st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_COPY);
  const IndexKey key(h.idxRows, h.idxCols, h.idxK, h.idxMinD, h.idxMaxD);
  cloud_commit(c, h.n, idx ? &key : nullptr);
  return PWN_HIP_OK;
}

// ------------------------------------------------------------------------------------------ input conditioning
int pwn_hip_depth_u16_to_f32(pwn_hip_ctx* ctx, const uint16_t* src, float* dst, int n, float scale) {
  if (!ctx || !src || !dst || n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if ((size_t)n > ctx->N * ctx->max_batch) return fail(ctx, PWN_HIP_ERR_CAPACITY, "image larger than the context workspaces");
  if (int rc = absorb_copies(ctx)) return rc;
  const uint16_t* s = src; float* d = dst;
  if (!is_device_ptr(src)) { HIPCHK(ctx, hipMemcpyAsync(ctx->raw_ws, src, (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY); s = ctx->raw_ws; }
  if (!is_device_ptr(dst)) d = ctx->depth_ws;
  ctx->raw_host[0].src = s; ctx->raw_host[0].dst = d;
  HIPCHK(ctx, hipMemcpyAsync(ctx->raw_dev, ctx->raw_host, sizeof(RawDesc), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_u16_to_f32, dim3(std::min((n + 255) / 256, 2048), 1), dim3(256), 0, ctx->stream, ctx->raw_dev, n, scale);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (d != dst) HIPCHK(ctx, hipMemcpyAsync(dst, d, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_depth_f32_to_u16(pwn_hip_ctx* ctx, const float* src, uint16_t* dst, int n, float scale) {
  if (!ctx || !src || !dst || n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if ((size_t)n > ctx->N * ctx->max_batch) return fail(ctx, PWN_HIP_ERR_CAPACITY, "image larger than the context workspaces");
  if (int rc = absorb_copies(ctx)) return rc;
  const float* s = src; uint16_t* d = dst;
  if (!is_device_ptr(src)) { HIPCHK(ctx, hipMemcpyAsync(ctx->depth_ws, src, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY); s = ctx->depth_ws; }
  if (!is_device_ptr(dst)) d = ctx->raw_ws;
  hipLaunchKernelGGL(k_f32_to_u16, dim3(std::min((n + 255) / 256, 2048)), dim3(256), 0, ctx->stream, s, d, n, scale);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (d != dst) HIPCHK(ctx, hipMemcpyAsync(dst, d, (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_depth_scale(pwn_hip_ctx* ctx, const float* src, int rows, int cols, int step, float max_depth_cov, float* dst) {
  if (!ctx || !src || !dst || step <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  const size_t n = (size_t)rows * cols; const int orows = rows / step, ocols = cols / step; const size_t on = (size_t)orows * ocols;
  if (int rc = absorb_copies(ctx)) return rc;
  const float* s = src; float* d = dst;
  if (!is_device_ptr(src)) { HIPCHK(ctx, hipMemcpyAsync(ctx->depth_ws, src, n * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY); s = ctx->depth_ws; }
  if (!is_device_ptr(dst)) d = ctx->io_ws;
  if (on > 0) hipLaunchKernelGGL(k_depth_scale, dim3((unsigned)((on + 255) / 256)), dim3(256), 0, ctx->stream, s, rows, cols, step, max_depth_cov, d);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (d != dst) HIPCHK(ctx, hipMemcpyAsync(dst, d, on * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// the two typed forms' argument checks, then the frames of `c` down-sampled into dst
static int depth_scale_batch_checked(pwn_hip_ctx* ctx, ConvertCall c, int step, float max_depth_cov, float* const* dst) {
  if (!ctx || !c.frames || !dst || c.n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = make_scale_spec(ctx, c.rows, c.cols, step, max_depth_cov, c.scale)) return rc;
  return depth_scale_batch_impl(ctx, c, dst);
}
int pwn_hip_depth_scale_batch(pwn_hip_ctx* ctx, const float* const* src, int n, int rows, int cols, int step, float max_depth_cov, float* const* dst) {
  return depth_scale_batch_checked(ctx, convert_call(nullptr, src, 0.f, n, rows, cols, nullptr), step, max_depth_cov, dst);
}
int pwn_hip_depth_scale_batch_u16(pwn_hip_ctx* ctx, const uint16_t* const* src, float depth_scale, int n, int rows, int cols, int step, float max_depth_cov,
                                  float* const* dst) {
  return depth_scale_batch_checked(ctx, convert_call(nullptr, src, depth_scale, n, rows, cols, nullptr), step, max_depth_cov, dst);
}

// ---------------------------------------------------------------------------------------------- converter stages
static int stage_depth(pwn_hip_ctx* ctx, const float* depth, size_t N, const float** out) {
  if (int rc = absorb_copies(ctx)) return rc;
  if (is_device_ptr(depth)) { *out = depth; return PWN_HIP_OK; }
  HIPCHK(ctx, hipMemcpyAsync(ctx->depth_ws, depth, N * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  *out = ctx->depth_ws;
  return PWN_HIP_OK;
}
int pwn_hip_unproject(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float T[16], const float* depth, int rows, int cols,
                      pwn_hip_cloud* cloud, int* index_image) {
  if (!ctx || !p || !depth || !cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  const size_t N = (size_t)rows * cols;
  // replace: points only.  Normals and point information are zeroed below; the normal information is the two class matrices, which give zero for a
  // zero normal, so nothing of the previous content's (Stats, Gaussians, explicit planes) is read beside the new points
  const OmegaNClasses cls = make_omega_n_classes(p);
  if (int rc = cloud_replace(ctx, cloud, false, false, &cls)) return rc;
  const ConvertParams cp = make_convert_params(ctx, p, T, rows, cols, 0);
  const float* d = nullptr;
  if (int rc = stage_depth(ctx, depth, N, &d)) return rc;
  HIPCHK(ctx, hipMemsetAsync(cloud->d.Nc, 0, sizeof(float4) * (size_t)cloud->d.capacity, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(cloud->d.Om, 0, sizeof(float) * cloud->front.Om.cap, ctx->stream), PWN_HIP_ERR_COPY);
  fill_frame(ctx, 0, 0, d, cloud->d);
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev, ctx->frames_host, sizeof(FrameDesc), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_row_count, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp);
  hipLaunchKernelGGL(k_row_offsets, dim3(1), dim3(1024), 0, ctx->stream, ctx->frames_dev, rows);
  hipLaunchKernelGGL(k_unproject, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (index_image) HIPCHK(ctx, copy_any(index_image, ctx->frames_host[0].index, N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  pwn_hip_cloud* arr[1] = { cloud };
  return sync_and_counts(ctx, arr, 1);      // commit
}
int pwn_hip_project_intervals(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, int* interval_image) {
  if (!ctx || !p || !depth || !interval_image) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  const size_t N = (size_t)rows * cols;
  const ConvertParams cp = make_convert_params(ctx, p, nullptr, rows, cols, 0);
  const float* d = nullptr;
  if (int rc = stage_depth(ctx, depth, N, &d)) return rc;
  CloudDev none; std::memset(&none, 0, sizeof(none)); none.count = ctx->scratch_count; none.capacity = 0;
  fill_frame(ctx, 0, 0, d, none);
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev, ctx->frames_host, sizeof(FrameDesc), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_row_count, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp);
  hipLaunchKernelGGL(k_row_offsets, dim3(1), dim3(1024), 0, ctx->stream, ctx->frames_dev, rows);
  hipLaunchKernelGGL(k_unproject, dim3(rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, cp);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, copy_any(interval_image, ctx->frames_host[0].interval, N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_integral_image(pwn_hip_ctx* ctx, const int* index_image, const pwn_hip_cloud* cloud, int rows, int cols, float* out) {
  if (!ctx || !index_image || !cloud || !out) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (int rc = absorb_copies(ctx)) return rc;      // caller pointers may be the destination of a queued pwn_hip_copy_async
  const size_t N = (size_t)rows * cols;
  fill_frame(ctx, 0, 0, nullptr, cloud->d);
  HIPCHK(ctx, copy_any(ctx->frames_host[0].index, index_image, N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->frames_dev, ctx->frames_host, sizeof(FrameDesc), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_integral_rows, dim3((rows + kIR_Rows - 1) / kIR_Rows, 1), dim3(256), 0, ctx->stream, ctx->frames_dev, rows, cols);
  hipLaunchKernelGGL(k_integral_cols, dim3((cols + kIC_Block - 1) / kIC_Block, kIntegralChannels, 1), dim3(kIC_Block), 0, ctx->stream, ctx->frames_dev, rows, cols, (const int*)nullptr, (int*)nullptr, 0);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, copy_any(out, ctx->frames_host[0].integral, N * kIntegralChannels * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_convert(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, pwn_hip_cloud* cloud,
                    int* index_image, int* interval_image, int keep_stats) {
  const float* frames[1] = { depth };
  pwn_hip_cloud* clouds[1] = { cloud };
  ConvertCall call = convert_call(p, frames, 0.f, 1, rows, cols, clouds);
  call.keep_stats = keep_stats; call.want_interval = interval_image != nullptr;
  if (int rc = convert_batch_impl(ctx, call)) return rc;
  const size_t N = (size_t)rows * cols;
  if (index_image) HIPCHK(ctx, hipMemcpy(index_image, ctx->frames_host[0].index, N * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  if (interval_image) HIPCHK(ctx, hipMemcpy(interval_image, ctx->frames_host[0].interval, N * 4, hipMemcpyDefault), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
int pwn_hip_convert_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, int step, float max_depth_cov,
                           pwn_hip_cloud* cloud) {
  if (!ctx || !p || !depth || !cloud || step <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  const int orows = rows / step, ocols = cols / step;
  if (orows <= 0 || ocols <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "scaled image has zero size");
  const size_t on = (size_t)orows * ocols;
  const float* src = nullptr;
  if (int rc = stage_depth(ctx, depth, (size_t)rows * cols, &src)) return rc;
  float* scaled = ctx->io_ws;                                        // device scratch (N*16 floats)
  hipLaunchKernelGGL(k_depth_scale, dim3((unsigned)((on + 255) / 256)), dim3(256), 0, ctx->stream, src, rows, cols, step, max_depth_cov, scaled);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  const float* frames[1] = { scaled };
  pwn_hip_cloud* clouds[1] = { cloud };
  return convert_batch_impl(ctx, convert_call(p, frames, 0.f, 1, orows, ocols, clouds));
}
static void async_convert_loop(AsyncConvert* a, int device) {
  (void)hipSetDevice(device);
  for (;;) {
    std::unique_lock<std::mutex> lk(a->m);
    a->cv.wait(lk, [a] { return a->has_job || a->quit; });
    if (!a->has_job) return;                                    // quit, nothing pending
    lk.unlock();
    const auto t_begin = std::chrono::steady_clock::now();
    int rc;
    if (a->raw) {
      const uint16_t* frames[1] = { a->raw }; pwn_hip_cloud* clouds[1] = { a->cloud };
      rc = convert_batch_impl(a->job_ctx, convert_call(&a->p, frames, a->raw_scale, 1, a->rows, a->cols, clouds));
    } else {
      rc = pwn_hip_convert_scaled(a->job_ctx, &a->p, a->depth, a->rows, a->cols, a->step, a->max_depth_cov, a->cloud);
    }
    size_t written = 0;
    if (rc == PWN_HIP_OK && a->flat_dst) rc = pwn_hip_cloud_export(a->job_ctx, a->cloud, a->flat_dst, a->flat_bytes, &written);
    const float job_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    lk.lock();
    a->flat_written = written; a->job_ms = job_ms;
    a->rc = rc; a->err = rc == PWN_HIP_OK ? std::string() : a->job_ctx->err;
    a->has_job = false; a->done = true;
    lk.unlock();
    a->cv.notify_all();
  }
}
// one job for the helper thread: a float frame through DepthImage_scale + the converter, or a raw uint16 frame through the converter; then
// (flat_dst != nullptr) the cloud's flat form
static int async_convert_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, const uint16_t* raw, float raw_scale, int rows, int cols,
                               int step, float max_depth_cov, pwn_hip_cloud* cloud, void* flat_dst, size_t flat_bytes);
int pwn_hip_convert_scaled_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, int step, float max_depth_cov,
                                 pwn_hip_cloud* cloud) {
  if (!ctx || !p || !depth || !cloud || step <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  return async_convert_begin(ctx, p, depth, nullptr, 0.f, rows, cols, step, max_depth_cov, cloud, nullptr, 0);
}
int pwn_hip_convert_export_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* raw_frame, float depth_scale, int rows, int cols,
                                 pwn_hip_cloud* cloud, void* flat_dst, size_t flat_bytes) {
  if (!ctx || !p || !raw_frame || !cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad argument");
  if (flat_dst) {      // checked here, where the caller can still act on it: the largest flat form this frame can have must fit
    const size_t need = pwn_hip_cloud_export_bound(std::min(cloud->d.capacity, rows * cols), cloud->d.omSym ? PWN_HIP_OMEGA_SYM6 : PWN_HIP_OMEGA_EXACT9, rows * cols, 0);
    if (flat_bytes < need) return fail(ctx, PWN_HIP_ERR_CAPACITY, "flat cloud buffer too small for a frame of this size (pwn_hip_cloud_export_bound)");
  }
  return async_convert_begin(ctx, p, nullptr, raw_frame, depth_scale, rows, cols, 1, 0.f, cloud, flat_dst, flat_bytes);
}
int pwn_hip_convert_export_end(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, size_t* written, float* job_ms) {
  if (written) *written = 0;
  if (job_ms) *job_ms = 0.f;
  const int rc = pwn_hip_convert_end(ctx, cloud);
  if (ctx && ctx->async) {
    if (written) *written = rc == PWN_HIP_OK ? ctx->async->flat_written : 0;
    if (job_ms) *job_ms = ctx->async->job_ms;
  }
  return rc;
}
static int async_convert_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, const uint16_t* raw, float raw_scale, int rows, int cols,
                               int step, float max_depth_cov, pwn_hip_cloud* cloud, void* flat_dst, size_t flat_bytes) {
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (rows / step <= 0 || cols / step <= 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "scaled image has zero size");
  if (!ctx->async) {
    AsyncConvert* a = new AsyncConvert();
    if (int rc = ctx_create(&a->helper, ctx->device, ctx->max_rows, ctx->max_cols, 1, false)) { const std::string m = g_err; delete a; return fail(ctx, rc, "helper context: " + m); }
    a->worker = std::thread(async_convert_loop, a, ctx->device);
    ctx->async = a;
  }
  AsyncConvert* a = ctx->async;
  {
    std::unique_lock<std::mutex> lk(a->m);
    if (a->cloud || !a->done) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "a conversion is already in flight on this context (pwn_hip_convert_end first)");
    // Which helper: the raw-frame form runs beside a batch whose streams hold hundreds of queued launches -- on default priority the one-frame job is
    // served when a hardware queue it shares with the batch has drained (5.8 ms of wall time instead of 0.5); beside a single alignment (the tracker's
    // look-ahead) high priority is the wrong way round: it delays the alignment's short dependent kernels (3 070 -> 2 300 frames/s measured).
    if (raw && !a->helper_hi) {
      if (int rc = ctx_create(&a->helper_hi, ctx->device, ctx->max_rows, ctx->max_cols, 1, true)) return fail(ctx, rc, "helper context: " + g_err);
    }
    a->job_ctx = raw ? a->helper_hi : a->helper;
    // the caller's copies (pwn_hip_copy_async into a device frame) must have landed before the helper's stream reads the frame
    if (int rc = absorb_copies(ctx)) return rc;
    // a device frame the context's own stream may still be writing (pwn_hip_copy_async above): wait for it.  The raw-frame form does not wait --
    // it is what a caller queues from inside pwn_hip_ctx_set_enqueued_callback while the context's stream is busy with a batch -- and asks for a
    // frame that is complete when the call is made (include/pwn_hip.h)
    if (depth && is_device_ptr(depth)) HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
    cloud_changes(ctx, cloud);
    a->raw = raw; a->raw_scale = raw_scale; a->flat_dst = flat_dst; a->flat_bytes = flat_bytes; a->flat_written = 0; a->job_ms = 0.f;
    a->p = *p; a->depth = depth; a->rows = rows; a->cols = cols; a->step = step; a->max_depth_cov = max_depth_cov; a->cloud = cloud;
    a->rc = PWN_HIP_OK; a->err.clear();
    a->done = false; a->has_job = true;
  }
  a->cv.notify_all();
  return PWN_HIP_OK;
}
int pwn_hip_convert_end(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud) {
  if (!ctx || !cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  AsyncConvert* a = ctx->async;
  if (!a || a->cloud != cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "no conversion of this cloud was begun on this context");
  std::unique_lock<std::mutex> lk(a->m);
  a->cv.wait(lk, [a] { return a->done; });
  a->cloud = nullptr;
  if (a->rc != PWN_HIP_OK) return fail(ctx, a->rc, a->err);
  return PWN_HIP_OK;
}
int pwn_hip_convert_batch(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* const* depth_frames, int n, int rows, int cols,
                          pwn_hip_cloud* const* clouds) {
  return convert_batch_impl(ctx, convert_call(p, depth_frames, 0.f, n, rows, cols, clouds));
}
int pwn_hip_convert_batch_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* const* depth_frames, int n, int rows, int cols, int step,
                                 float max_depth_cov, pwn_hip_cloud* const* clouds) {
  return convert_batch_scaled_impl(ctx, convert_call(p, depth_frames, 0.f, n, rows, cols, clouds), step, max_depth_cov);
}
int pwn_hip_convert_batch_u16_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* const* raw_frames, float depth_scale, int n,
                                     int rows, int cols, int step, float max_depth_cov, pwn_hip_cloud* const* clouds) {
  return convert_batch_scaled_impl(ctx, convert_call(p, raw_frames, depth_scale, n, rows, cols, clouds), step, max_depth_cov);
}
int pwn_hip_convert_batch_u16(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* const* raw_frames, float depth_scale, int n,
                              int rows, int cols, pwn_hip_cloud* const* clouds) {
  return convert_batch_impl(ctx, convert_call(p, raw_frames, depth_scale, n, rows, cols, clouds));
}
void pwn_hip_default_convert_extras(pwn_hip_convert_extras* e) {
  if (!e) return;
  e->keep_stats = 0; e->gaussians = 0; e->baseline = 0.075f; e->alpha = 0.1f;      // pinholepointprojector.cpp:10-11
}
// The four batch forms with the extras.  What the extras can be refused for is looked at here; everything else by the form's own implementation,
// before it touches a cloud.
int pwn_hip_convert_batch_ex(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const void* const* frames, int raw_u16, float depth_scale, int n, int rows,
                             int cols, int step, float max_depth_cov, const pwn_hip_convert_extras* extras, pwn_hip_cloud* const* clouds) {
  if (!ctx || !p || !frames || !clouds || n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (step < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "DepthImage_scale: step < 0");
  ConvertCall call; call.p = p; call.n = n; call.rows = rows; call.cols = cols; call.clouds = clouds;
  call.frames = frames; call.raw = raw_u16 != 0; call.depth_scale = call.raw ? depth_scale : 0.f;
  if (extras) {
    GaussSpec& gs = call.gauss;
    if ((extras->keep_stats != 0 && extras->keep_stats != 1) || (extras->gaussians != 0 && extras->gaussians != 1))
      return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "convert extras: keep_stats and gaussians must be 0 or 1");
    if (!std::isfinite(extras->baseline) || !std::isfinite(extras->alpha)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "convert extras: baseline or alpha is not finite");
    call.keep_stats = extras->keep_stats;
    if (extras->gaussians) {
      Mat4 KRt, iKRt;
      projector_matrices(mat3_from(p->K), mat4_identity(), KRt, iKRt, gs.iK);
      gs.on = true; gs.fB = extras->baseline * p->K[0]; gs.alpha = extras->alpha;
    }
  }
  return step == 0 ? convert_batch_impl(ctx, call) : convert_batch_scaled_impl(ctx, call, step, max_depth_cov);
}

// ------------------------------------------------------------------------------------------------ aligner stages
// A cloud rendered into index and / or depth image (either may be null; device pointers): the z-buffer cleared, the cloud's points projected -- the
// kernel reads the size; bound: what the grid covers -- and the winners resolved.  pwn_hip_project and the mapping step's rendering of the scene.
static int render_enqueue(pwn_hip_ctx* ctx, hipStream_t st, const CloudDev& cl, int bound, const Mat4& KRt, float min_distance, float max_distance, int rows, int cols,
                          int* index, float* depth) {
  const size_t N = (size_t)rows * cols;
  HIPCHK(ctx, hipMemsetAsync(ctx->zref_ws, 0xFF, N * 8, st), PWN_HIP_ERR_COPY);
  if (bound > 0) hipLaunchKernelGGL(k_project_single, dim3((unsigned)((bound + 255) / 256)), dim3(256), 0, st, cl, KRt, min_distance, max_distance, rows, cols, ctx->zref_ws, kZTag0);
  hipLaunchKernelGGL(k_zbuf_resolve, dim3((unsigned)std::min<size_t>((N + 255) / 256, 2048)), dim3(256), 0, st, ctx->zref_ws, (int)N, index, depth, kZTag0);
  return PWN_HIP_OK;
}
int pwn_hip_project(pwn_hip_ctx* ctx, const float K[9], const float T[16], float min_distance, float max_distance, int rows, int cols,
                    const pwn_hip_cloud* cloud, int* index_image, float* depth_image) {
  if (!ctx || !K || !T || !cloud) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  if (int rc = check_image(ctx, rows, cols)) return rc;
  const size_t N = (size_t)rows * cols;
  Mat4 KRt, iKRt; Mat3 iK;
  projector_matrices(mat3_from(K), mat4_from(T), KRt, iKRt, iK);
  int* di = index_image ? (is_device_ptr(index_image) ? index_image : ctx->index_ws) : nullptr;
  float* dd = depth_image ? (is_device_ptr(depth_image) ? depth_image : ctx->depth_ws) : nullptr;
  { StageTimer t(ctx, "project");
    if (int rc = render_enqueue(ctx, ctx->stream, cloud->d, cloud->d.capacity, KRt, min_distance, max_distance, rows, cols, di, dd)) return rc; }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (index_image && di != index_image) HIPCHK(ctx, hipMemcpyAsync(index_image, di, N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  if (depth_image && dd != depth_image) HIPCHK(ctx, hipMemcpyAsync(depth_image, dd, N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  ctx->img.invalidate();
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}
// ------------------------------------------------------------------------------------------------ merged closure
// What the two entry points of the merged closure share.  A call is checked completely before anything is written; then: the caller's `merged`
// and weight image are used in place (device) or staged (host), the counters cleared, the images fused in chunks of ctx->merge_planes in call
// order on the context's stream -- the per-pixel chain of a later chunk continues from what the earlier one left in `merged` / `weights`, so the
// chunking does not show in the bits -- and everything that has to reach the host copied back before the one wait of the call.
struct MergeRun { float* merged; float* weights; float* planes; int N; };
static int merge_check(pwn_hip_ctx* ctx, int n, int rows, int cols, const float* merged, const float* weights) {
  if (!ctx || !merged || !weights) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative number of images");
  if (merged == weights) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "merged and weights are the same image");
  return check_image(ctx, rows, cols);
}
static int merge_begin(pwn_hip_ctx* ctx, int n, int rows, int cols, float* merged, float* weights, MergeRun& r) {
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;
  if (!ctx->merge_planes) ctx->merge_planes = std::min(ctx->max_batch, kMergePlanesMax);
  HIPCHK(ctx, ctx->merge_ws.ensure((size_t)(ctx->merge_planes + 2) * ctx->N), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->plane_ptrs_dev.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->plane_ptrs_host.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->merge_counts_dev.ensure((size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->merge_counts_host.ensure((size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  ctx->stages.clear();
  r.N = rows * cols;
  r.planes = ctx->merge_ws + 2 * ctx->N;
  r.merged = is_device_ptr(merged) ? merged : ctx->merge_ws.p;
  r.weights = is_device_ptr(weights) ? weights : ctx->merge_ws + ctx->N;
  if (r.merged != merged) HIPCHK(ctx, hipMemcpyAsync(r.merged, merged, (size_t)r.N * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  if (r.weights != weights) HIPCHK(ctx, hipMemcpyAsync(r.weights, weights, (size_t)r.N * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(ctx->merge_counts_dev, 0, sizeof(int) * ((size_t)n + 1), ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// images [base, base + m) of the call, whose addresses sit in plane_ptrs_dev
static int merge_chunk(pwn_hip_ctx* ctx, const MergeRun& r, int n, int base, int m) {
  StageTimer t(ctx, "merge_depth_images");
  hipLaunchKernelGGL(k_merge_depth_images, dim3((unsigned)((r.N + 255) / 256)), dim3(256), 0, ctx->stream, ctx->plane_ptrs_dev + base, m, r.N, r.merged, r.weights,
                     ctx->merge_counts_dev + base, ctx->merge_counts_dev + n);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
static int merge_end(pwn_hip_ctx* ctx, const MergeRun& r, int n, float* merged, float* weights, int* overlap, int* points) {
  if (r.merged != merged) HIPCHK(ctx, hipMemcpyAsync(merged, r.merged, (size_t)r.N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  if (r.weights != weights) HIPCHK(ctx, hipMemcpyAsync(weights, r.weights, (size_t)r.N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->merge_counts_host, ctx->merge_counts_dev, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  if (overlap) std::copy(ctx->merge_counts_host.p, ctx->merge_counts_host.p + n, overlap);
  if (points) *points += ctx->merge_counts_host[n];
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}
int pwn_hip_merge_depth_images(pwn_hip_ctx* ctx, int n, const float* const* depth_images, int rows, int cols, float* merged, float* weights, int* overlap,
                               int* points) {
  if (int rc = merge_check(ctx, n, rows, cols, merged, weights)) return rc;
  if (n > 0 && !depth_images) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < n; ++i) if (!depth_images[i]) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (n == 0) return PWN_HIP_OK;
  MergeRun r;
  if (int rc = merge_begin(ctx, n, rows, cols, merged, weights, r)) return rc;
  const int P = ctx->merge_planes;
  std::vector<char> staged((size_t)n);                 // host images pass through the plane of their place in the chunk
  for (int i = 0; i < n; ++i) {
    staged[i] = !is_device_ptr(depth_images[i]);
    ctx->plane_ptrs_host[i] = staged[i] ? r.planes + (size_t)(i % P) * r.N : depth_images[i];
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->plane_ptrs_dev, ctx->plane_ptrs_host, sizeof(float*) * (size_t)n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  for (int base = 0; base < n; base += P) {
    const int m = std::min(P, n - base);
    for (int j = 0; j < m; ++j)
      if (staged[base + j]) HIPCHK(ctx, hipMemcpyAsync(r.planes + (size_t)j * r.N, depth_images[base + j], (size_t)r.N * 4, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    if (int rc = merge_chunk(ctx, r, n, base, m)) return rc;
  }
  return merge_end(ctx, r, n, merged, weights, overlap, points);
}
int pwn_hip_project_merge_batch(pwn_hip_ctx* ctx, const float K[9], int n, pwn_hip_cloud* const* clouds, const float* transforms, float min_distance,
                                float max_distance, int rows, int cols, float* merged, float* weights, int* overlap, int* points, float* planes) {
  if (int rc = merge_check(ctx, n, rows, cols, merged, weights)) return rc;
  if (!K || (n > 0 && (!clouds || !transforms))) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  for (int i = 0; i < n; ++i) {
    if (!clouds[i]) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null cloud");
    if (clouds[i]->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
  }
  if (n == 0) return PWN_HIP_OK;
  MergeRun r;
  if (int rc = merge_begin(ctx, n, rows, cols, merged, weights, r)) return rc;
  HIPCHK(ctx, ctx->depth_clouds_dev.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->depth_clouds_host.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->krt_dev.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->krt_host.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  const int P = ctx->merge_planes;
  const Mat3 Km = mat3_from(K);
  for (int i = 0; i < n; ++i) {
    Mat4 iKRt; Mat3 iK;
    projector_matrices(Km, mat4_from(transforms + 16 * (size_t)i), ctx->krt_host[i], iKRt, iK);      // as pwn_hip_project builds its KRt
    DepthCloudDesc& d = ctx->depth_clouds_host[i];
    d.P3 = clouds[i]->d.P3; d.count = clouds[i]->d.count; d.capacity = clouds[i]->d.capacity;
    ctx->plane_ptrs_host[i] = r.planes + (size_t)(i % P) * r.N;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->plane_ptrs_dev, ctx->plane_ptrs_host, sizeof(float*) * (size_t)n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->depth_clouds_dev, ctx->depth_clouds_host, sizeof(DepthCloudDesc) * (size_t)n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->krt_dev, ctx->krt_host, sizeof(Mat4) * (size_t)n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
  for (int base = 0; base < n; base += P) {
    const int m = std::min(P, n - base);
    int capacity = 1;
    for (int j = 0; j < m; ++j) capacity = std::max(capacity, clouds[base + j]->d.capacity);
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)r.planes, (int)kDepthPlaneEmpty, (size_t)m * r.N, ctx->stream), PWN_HIP_ERR_COPY);
    // one point per thread: the atomics return nothing, so a thread has nothing to wait for between its points (what k_project's four points per
    // thread buy); more points per thread stay unbuilt until a measurement asks for them
    { StageTimer t(ctx, "project_depth_batch");
      hipLaunchKernelGGL((k_project_depth_batch<1>), dim3((unsigned)((capacity + 255) / 256), (unsigned)m), dim3(256), 0, ctx->stream, ctx->depth_clouds_dev + base,
                         ctx->krt_dev + base, min_distance, max_distance, rows, cols, (unsigned*)r.planes); }
    HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
    if (int rc = merge_chunk(ctx, r, n, base, m)) return rc;
    if (planes) HIPCHK(ctx, copy_any(planes + (size_t)base * r.N, r.planes, (size_t)m * r.N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  }
  return merge_end(ctx, r, n, merged, weights, overlap, points);
}
int pwn_hip_correspondences(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur,
                            const int* ref_index, const int* cur_index, const float T[16], int* corr, int* n_corr, int* n_cand) {
  if (!ctx || !p || !ref || !cur || !ref_index || !cur_index || !T || !corr || !n_corr) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, p->rows, p->cols)) return rc;
  const size_t N = (size_t)p->rows * p->cols;
  const AlignParams ap = make_align_params(ctx, p);
  int* ri = ctx->index_ws; int* ci = ctx->interval_ws;
  if (int rc = absorb_copies(ctx)) return rc;      // caller pointers may be the destination of a queued pwn_hip_copy_async
  HIPCHK(ctx, copy_any(ri, ref_index, N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, copy_any(ci, cur_index, N * 4, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemsetAsync(ctx->counters_dev, 0, 16 * sizeof(int), ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_correspondence_image, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, ref->d, cur->d, ri, ci, ap, forced(T), ctx->corr_ws, ctx->counters_dev);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  std::vector<int2> img(N); int cand = 0;
  HIPCHK(ctx, hipMemcpyAsync(img.data(), ctx->corr_ws, N * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(&cand, ctx->counters_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  std::vector<int> out(2 * N, -1);
  int C = 0;
  for (size_t i = 0; i < N; ++i) if (img[i].x >= 0) { out[2 * C] = img[i].x; out[2 * C + 1] = img[i].y; ++C; }   // row-major order
  HIPCHK(ctx, hipMemcpy(corr, out.data(), 2 * N * sizeof(int), hipMemcpyDefault), PWN_HIP_ERR_COPY);
  *n_corr = C;
  if (n_cand) *n_cand = cand;
  return PWN_HIP_OK;
}
int pwn_hip_linearize(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, const int* corr,
                      int C, const float T[16], float* H, float* b, float* error, int* inliers) {
  if (!ctx || !p || !ref || !cur || (!corr && C > 0) || !T || C < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if ((size_t)C > ctx->N) return fail(ctx, PWN_HIP_ERR_CAPACITY, "more correspondences than pixels");
  const AlignParams ap = make_align_params(ctx, p);
  if (int rc = absorb_copies(ctx)) return rc;      // caller pointers may be the destination of a queued pwn_hip_copy_async
  if (C > 0) HIPCHK(ctx, copy_any(ctx->corr_ws, corr, (size_t)C * sizeof(int2), ctx->stream), PWN_HIP_ERR_COPY);
  const int nb = std::max(1, align_nblocks(C));
  { StageTimer t(ctx, "corr_linearize");
    hipLaunchKernelGGL(k_linearize_list, dim3(nb), dim3(kAlignBlock), 0, ctx->stream, ref->d, cur->d, ctx->corr_ws, C, ap, forced(T), ctx->partials_ws); }
  hipLaunchKernelGGL(k_reduce_only, dim3(1), dim3(256), 0, ctx->stream, ctx->partials_ws, nb, ctx->solve_dev);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  SolveOut so;
  HIPCHK(ctx, hipMemcpyAsync(&so, ctx->solve_dev, sizeof(so), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  if (H) std::memcpy(H, so.H, sizeof(so.H));
  if (b) std::memcpy(b, so.b, sizeof(so.b));
  if (error) *error = so.chi2;
  if (inliers) *inliers = so.inliers;
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}

// What a caller may weave into a batch alignment (pwn_hip_convert_align_batch_u16: the conversion of a sub-batch's frames goes in front of its
// alignment on the same stream, so that one sub-batch converts while the other aligns and nothing waits for the host in between).
struct AlignHooks {
  std::function<int(int base, int m, int k, hipStream_t st)> pre_sub;      // before the kernels of pairs [base, base + m) (sub-batch k) are enqueued on st
  std::function<int()> before_sync;                                        // on ctx->stream, after the streams have joined
  std::function<int()> after_sync;                                         // after the final wait, before the results are filled in
};
// The resident full-resolution uint16 frames the current clouds of a call are converted from in front of their alignment, with that conversion's
// parameters: a sub-batch whose pairs all take the current cloud's own index image runs the fused pass on them (CurDepthSrc)
struct CurDepthFrames { const void* const* frames; float scale; const ConvertParams* cp; };
// What a caller asks of a batch alignment; every member defaults to "not asked for", an entry point names the ones it uses.
struct AlignCall {
  const pwn_hip_aligner_params* p = nullptr;
  int n = 0;                                                   // pairs: refs[i] against curs[i]
  pwn_hip_cloud* const* refs = nullptr; pwn_hip_cloud* const* curs = nullptr;
  const float* guesses = nullptr;                              // n initial transforms (16 floats each); nullptr: p->initial_guess for every pair
  pwn_hip_align_result* results = nullptr;                     // may be nullptr when records are asked for
  pwn_hip_match_result* scores = nullptr; float match_threshold = 0.f;      // the matchClouds score of every pair
  pwn_hip_align_statistics* statistics = nullptr;              // Aligner::_computeStatistics of every pair
  const AlignHooks* hooks = nullptr;
  float* records = nullptr;                                    // n records, device or host, written by k_pack_records: PWN_HIP_RECORD_FLOATS floats each,
  bool match_records = false;                                  // or the long form with the score words
  bool closure_records = false;                                // or the closure form: the score words and Aligner::_computeStatistics, computed on the device
  const int* pair_ids = nullptr; int first_pair_id = 0;        // record word 19: pair_ids[i] (host), else first_pair_id + i
  const CurDepthFrames* cur_depth = nullptr;                   // the one-call step: the frames curs[i] are being converted from
  const pwn_hip_pair_priors* priors = nullptr;                 // SE(3) priors per pair (checked by the entry point); nullptr or an empty list: none
};
// What the phases of one attempt at a call share (on align_batch_once's stack)
struct AlignRun {
  bool robust = false;                   // every projection by the two-pass kernels (the repeat of a call whose k_project gave up on a pixel)
  bool want_scores = false;              // the score accumulators are needed: for `scores`, or for the score words of the long records
  bool direct_state = false;             // a few pairs: k_solve_update keeps state_host up to date itself, no copy back
  StreamPlan plan;
  AlignParams ap;
  int N = 0, nb = 0, omSym = 0;          // pixels; workgroups per pair of the linearize pass; storage of the current clouds' information matrices
  std::vector<char> sub_own, sub_ownref; // per sub-batch: every pair of it takes the current cloud's own index image / the reference cloud's in iteration 0
  bool any_own = false;
  bool priors = false;                   // the call holds at least one prior: its list is on the device (align_describe_pairs)
  bool rolling = false; unsigned tagBase = kZ32Tag0, tagsPerSub = 1;      // sub-batch k draws the tags tagBase - k * tagsPerSub downwards; fixed tags: kZ32Tag0 for all
  Slot0Pair slot0;                       // the sub-batch that owns workspace slot 0 (what the finder's images will show)
};
// the parameter checks of every alignment call (each entry point checks its own pointer arguments first)
static int check_align_params(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p) {
  if (int rc = check_image(ctx, p->rows, p->cols)) return rc;
  if (p->min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  const int nit = p->outer_iterations * p->inner_iterations;
  if (p->outer_iterations < 0 || p->inner_iterations < 0 || nit > PWN_HIP_MAX_ITERATIONS)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "outer*inner iterations exceeds PWN_HIP_MAX_ITERATIONS");
  return PWN_HIP_OK;
}
// the aligner's 32-bit z-buffer word indexes 2^21 points (every frame up to 1448 x 1448 pixels); larger clouds are scenes (merge, voxelize)
static int check_pair_points(pwn_hip_ctx* ctx, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur) {
  if (std::min(ref->content.n, ref->d.capacity) > kMaxAlignerPoints || std::min(cur->content.n, cur->d.capacity) > kMaxAlignerPoints)
    return fail(ctx, PWN_HIP_ERR_CAPACITY, "Aligner::align: a cloud holds more than 2^21 points (index field of the aligner's z-buffer word)");
  return PWN_HIP_OK;
}
// descriptor `entry` of a call (its state: state_ws[entry]): the pair's clouds and the buffers of workspace slot `slot`
static void fill_pair(pwn_hip_ctx* ctx, int entry, int slot, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, PairState* state_out, bool robust) {
  PairDesc& pd = ctx->pairs_host[entry];
  pd.ref = ref->d; pd.cur = cur->d;
  pd.zref = ctx->z32ref_ws + (size_t)slot * ctx->N;
  pd.zcur = ctx->z32cur_ws + (size_t)slot * ctx->N;
  pd.curidx = ctx->curidx_ws + (size_t)slot * ctx->N;
  pd.refidx0 = nullptr;
  pd.partials = ctx->partials_ws + (size_t)slot * ctx->nblocks_max * kAccN;
  pd.state = ctx->state_ws + entry;
  pd.state_out = state_out;
  pd.fault = ctx->align_fault_host;
  pd.zdepth = robust ? ctx->zdepth_ws + (size_t)slot * ctx->N : nullptr;
}
// the pose part of a pair's state at the start of an outer iteration with transform T (aligner.cpp:72-73,84)
static void set_pose(PairState& st, const Mat4& T, const AlignParams& ap, const Mat4& KRtCur) {
  st.T = T;
  st.invTcorr = iso_inverse(T);
  st.invT = st.invTcorr; set_last_row(st.invT);
  Mat4 iKRt; Mat3 iK;
  projector_matrices(ap.K, iso_mul(T, ap.refOffset), st.KRt, iKRt, iK);
  st.KRtLast = st.KRt;
  st.KRtCur = KRtCur;
}

// the record the prior terms are computed from (pwn_stats.h): the inverse reference transform is taken here, once (se3_prior.h)
static PriorHost prior_host_from(const pwn_hip_prior& q) {
  PriorHost pr;
  pr.kind = q.kind; pr.mean = mat4_from(q.mean);
  pr.invReference = q.kind == 1 ? iso_inverse(mat4_from(q.reference_transform)) : mat4_identity();
  std::memcpy(pr.information, q.information, sizeof(pr.information));
  return pr;
}
// a prior list as pwn_hip_pair_priors describes it: first[0] = 0, non-decreasing, every kind 0 or 1
static bool prior_list_ok(int n, const int* first, const pwn_hip_prior* priors) {
  if (n < 0 || !first || first[0] != 0) return false;
  for (int i = 0; i < n; ++i) if (first[i + 1] < first[i]) return false;
  if (first[n] > 0 && !priors) return false;
  for (int j = 0; j < first[n]; ++j) if (priors[j].kind != 0 && priors[j].kind != 1) return false;
  return true;
}
// The list of a call on the device, queued on st: first[0 .. n] and the first[n] records; the terms get room.  The buffers grow with the call
// (nothing of an earlier call is in flight: every call ends with a wait).
static int upload_priors(pwn_hip_ctx* ctx, int n, const int* first, const pwn_hip_prior* priors, hipStream_t st) {
  const size_t np = (size_t)first[n];
  HIPCHK(ctx, ctx->prior_first_dev.ensure((size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->prior_first_host.ensure((size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->priors_dev.ensure(std::max<size_t>(np, 64)), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->priors_host.ensure(std::max<size_t>(np, 64)), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->prior_terms_dev.ensure(std::max<size_t>(np, 64)), PWN_HIP_ERR_ALLOCATION);
  std::memcpy(ctx->prior_first_host.p, first, sizeof(int) * ((size_t)n + 1));
  for (size_t j = 0; j < np; ++j) ctx->priors_host[j] = prior_host_from(priors[j]);
  HIPCHK(ctx, hipMemcpyAsync(ctx->prior_first_dev, ctx->prior_first_host, sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  if (np > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->priors_dev, ctx->priors_host, sizeof(PriorHost) * np, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}

// ---- one attempt at a batch alignment, phase by phase (align_batch_once calls them in this order) ----
// Check and plan.  On the streams: the start event.  A call refused for its image size keeps the last alignment's images; from there on they are gone.
static int align_check_and_plan(pwn_hip_ctx* ctx, const AlignCall& c, AlignRun& run) {
  if (!ctx || !c.p || !c.refs || !c.curs || (!c.results && !c.records) || c.n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_image(ctx, c.p->rows, c.p->cols)) return rc;
  ctx->img.invalidate();                  // whatever happens below (set again on success)
  ctx->last_pairs = 0; ctx->cur_depth_subs = 0; ctx->strip_index_subs = 0;
  if (int rc = check_align_params(ctx, c.p)) return rc;
  if (int rc = start_align_attempt(ctx, run.robust)) return rc;
  run.want_scores = c.scores != nullptr || (c.records && (c.match_records || c.closure_records));
  run.ap = make_align_params(ctx, c.p); run.N = c.p->rows * c.p->cols; run.nb = align_nblocks(run.N);
  ctx->stages.clear();
  run.plan = make_plan(ctx, ctx->sub_pairs, c.n);
  if (int rc = ensure_desc(ctx, c.n)) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->t0, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// Describe the pairs.  On ctx->stream: the uploads of all descriptors and initial states, and the score accumulators cleared.
static int align_describe_pairs(pwn_hip_ctx* ctx, const AlignCall& c, AlignRun& run) {
  const pwn_hip_aligner_params* p = c.p;
  const int n = c.n, sub = run.plan.sub;
  // A cloud's own index image (the converter's) is what projecting it with these parameters and an identity pose would give (see
  // pwn_hip_cloud::idximg): the current cloud's projection is skipped, and the matchClouds score then reads the current depth image off the
  // cloud itself (k_match_score, curOwn); a single alignment's current z-buffer is made on demand (FinderImages::cur_lazy).  The reference
  // cloud's FIRST projection is skipped when guess and reference offset are the identity too; later iterations (and the last one, whose
  // z-buffer the statistics pass re-reads) project as usual.
  const IndexKey key = index_key(p);
  const bool shortcut = n >= 1 && ctx->index_shortcut && is_identity(forced(p->current_sensor_offset));
  // the first outer iteration may be a pair's last under the convergence setting: then its z-buffer is read afterwards too, so the shortcut is decided
  // as for a call of the fewest outer iterations a pair can run
  const int min_outer = ctx->stop.enabled ? std::min(p->outer_iterations, std::max(1, ctx->stop.minIterations)) : p->outer_iterations;
  const bool shortcut_ref = shortcut && min_outer > 1 && is_identity(forced(p->reference_sensor_offset));
  // a few pairs (latency path): k_solve_update writes the pose and the traces into the page-locked host copy itself, no copy back at the end;
  // batches copy the states back in one transfer (64 workgroups storing across PCIe in every solve launch cost more than that: 16 against 11 us per launch)
  run.direct_state = n <= 4;
  run.omSym = (n > 0 && c.curs[0]) ? c.curs[0]->d.omSym : 0;      // the linearizer reads the CURRENT cloud's information matrices (linearizer.cpp:52-53)
  // The loop runs with the device idle (the call's first launch comes after it): what does not depend on the pair is computed once, and only the
  // head of a state is cleared (the traces behind `it` are written before they are read: k_solve_update stores entry `it`, every reader stops at `it`).
  // Workspace slots are reused round-robin across sub-batches; a sub-batch skips the projection kernels only if every pair of it can.
  run.sub_own.assign((size_t)(n + sub - 1) / sub + 1, 1); run.sub_ownref.assign(run.sub_own.size(), 1);
  Mat4 KRtCur0;
  { Mat4 iKRt0; Mat3 iK0; projector_matrices(run.ap.K, mat4_from(p->current_sensor_offset), KRtCur0, iKRt0, iK0); }
  for (int i = 0; i < n; ++i) {
    const pwn_hip_cloud* r = c.refs[i]; const pwn_hip_cloud* cu = c.curs[i];
    if (!r || !cu) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null cloud in batch");
    if (cu->d.omSym != run.omSym) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "current clouds of one batch must share one omega storage (exact9 / sym6)");
    if (int rc = check_pair_points(ctx, r, cu)) return rc;
    fill_pair(ctx, i, run.plan.slot0(i / sub) + i % sub, r, cu, run.direct_state ? ctx->state_host + i : nullptr, run.robust);
    // initial state: aligner.cpp:60-64,72-73,79,84
    PairState& st = ctx->state_host[i];
    std::memset(&st, 0, offsetof(PairState, chi2));
    Mat4 T = mat4_from(c.guesses ? c.guesses + 16 * (size_t)i : p->initial_guess);
    set_last_row(T);
    if (!(shortcut && cu->content.idx_valid && cu->content.idx_key == key)) run.sub_own[i / sub] = 0;
    if (!(shortcut_ref && is_identity(T) && r->content.idx_valid && r->content.idx_key == key)) run.sub_ownref[i / sub] = 0;
    set_pose(st, T, run.ap, KRtCur0);
  }
  for (int i = 0; i < n; ++i) {
    if (run.sub_own[i / sub]) { ctx->pairs_host[i].curidx = c.curs[i]->idximg; run.any_own = true; }
    if (run.sub_ownref[i / sub]) ctx->pairs_host[i].refidx0 = c.refs[i]->idximg;
  }
  if (n > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->pairs_dev, ctx->pairs_host, sizeof(PairDesc) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemcpyAsync(ctx->state_ws, ctx->state_host, sizeof(PairState) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    if (c.cur_depth && run.any_own) {
      for (int i = 0; i < n; ++i) ctx->cur_raw_host[i] = static_cast<const uint16_t*>(c.cur_depth->frames[i]);
      HIPCHK(ctx, hipMemcpyAsync(ctx->cur_raw_dev, ctx->cur_raw_host, sizeof(const uint16_t*) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
      // the strip offsets beside them (whether a sub-batch reads them is decided when its conversions have been queued: align_enqueue_sub)
      for (int i = 0; i < n; ++i) ctx->cur_strip_host[i] = c.curs[i]->stripoff;
      HIPCHK(ctx, hipMemcpyAsync(ctx->cur_strip_dev, ctx->cur_strip_host, sizeof(const int*) * n, hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    }
    if (run.want_scores) HIPCHK(ctx, hipMemsetAsync(ctx->match_dev, 0, sizeof(MatchAcc) * n, ctx->stream), PWN_HIP_ERR_COPY);
  }
  run.priors = n > 0 && c.priors && c.priors->first[n] > 0;
  if (run.priors) { if (int rc = upload_priors(ctx, n, c.priors->first, c.priors->priors, ctx->stream)) return rc; }
  return PWN_HIP_OK;
}
// Draw the tags.  On ctx->stream: the clearing of all z-buffer slots if the tag space had to start over, else nothing.
// Every sub-batch takes its own block of tags (workspace slots are reused from sub-batch to sub-batch): its first for the current-cloud
// projection (its own buffer) and that minus i for the reference projection of outer iteration i.  A call with more sub-batches than the tag
// space holds falls back to the fixed tags and clears the slots of every sub-batch.
static int align_draw_tags(pwn_hip_ctx* ctx, const AlignCall& c, AlignRun& run) {
  run.tagsPerSub = (unsigned)std::max(1, c.p->outer_iterations);
  const unsigned nsub = (unsigned)((c.n + run.plan.sub - 1) / run.plan.sub);
  if (run.tagsPerSub > kZ32Tag0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "more projections per alignment than z-buffer epoch tags");
  run.rolling = (unsigned long long)nsub * run.tagsPerSub <= kZ32Tag0;
  if (run.rolling && nsub > 0) { if (int rc = take_tags32(ctx, nsub * run.tagsPerSub, &run.tagBase)) return rc; }
  // fixed tags leave words in the buffers that could beat (smaller tag wins) the tags a later rolling call draws: make that call clear first
  if (!run.rolling) ctx->z32tag_next = 0;
  run.slot0.cur_tag = run.tagBase; run.slot0.ref_tag = run.tagBase - (run.tagsPerSub - 1);
  return PWN_HIP_OK;
}
// Enqueue sub-batch k, the pairs [base, base + m).  On its stream: what the pre_sub hook put there, then all its kernels up to the final states, statistics sums and scores.
static int align_enqueue_sub(pwn_hip_ctx* ctx, const AlignCall& c, AlignRun& run, int base, int k) {
  const pwn_hip_aligner_params* p = c.p;
  const int m = std::min(run.plan.sub, c.n - base), N = run.N;
  hipStream_t st = run.plan.stream(k);
  const size_t s0 = (size_t)run.plan.slot0(k);
  // the current points from the frames: every pair of the sub-batch reads the index image its frame's conversion wrote, in the throughput shape
  CurDepthSrc cd;
  const bool cur_depth = c.cur_depth && run.sub_own[k] && !latency_shape(ctx, run.nb, m);
  if (cur_depth) {
    const ConvertParams& cp = *c.cur_depth->cp;
    cd.raw = ctx->cur_raw_dev + base; cd.scale = c.cur_depth->scale; cd.iKRt = cp.iKRt; cd.hasOffset = cp.hasOffset; cd.offset = cp.offset;
    cd.strips = nullptr; cd.minD = cp.minD; cd.maxD = cp.maxD;
    ++ctx->cur_depth_subs;
  }
  const PairLaunch L = { &run.ap, run.nb, run.omSym, m, st, ctx->pairs_dev + base, run.robust ? ctx->zdepth_ws + s0 * ctx->N : nullptr, cur_depth ? &cd : nullptr };
  int maxcap_ref = 0, maxcap_cur = 0;
  for (int i = 0; i < m; ++i) { maxcap_ref = std::max(maxcap_ref, c.refs[base + i]->d.capacity); maxcap_cur = std::max(maxcap_cur, c.curs[base + i]->d.capacity); }
  const unsigned tag0 = run.rolling ? run.tagBase - (unsigned)k * run.tagsPerSub : kZ32Tag0, lastRefTag = tag0 - (run.tagsPerSub - 1);
  if (!run.rolling) {      // z-buffers start empty; slots are contiguous
    HIPCHK(ctx, hipMemsetAsync(ctx->z32ref_ws + s0 * ctx->N, 0xFF, (size_t)m * ctx->N * 4, st), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, hipMemsetAsync(ctx->z32cur_ws + s0 * ctx->N, 0xFF, (size_t)m * ctx->N * 4, st), PWN_HIP_ERR_COPY);
  }
  if (s0 == 0 || k == 0) {      // slot 0: what pwn_hip_align_images / pwn_hip_match_score read
    run.slot0.pair = base; run.slot0.ref_cloud = c.refs[base]; run.slot0.cur_cloud = c.curs[base];
    run.slot0.cur_tag = tag0; run.slot0.ref_tag = lastRefTag;
  }
  if (c.hooks && c.hooks->pre_sub) { if (int rc = c.hooks->pre_sub(base, m, k, st)) return rc; }
  // ... and the current indices from the strip offsets, when every current cloud's conversion -- queued by the hook above, which knows how it
  // launched them -- leaves the table of its index image (L.cd points to cd)
  if (cur_depth) {
    bool tables = true;
    for (int i = 0; i < m && tables; ++i) tables = c.curs[base + i]->strip_table();
    if (tables) { cd.strips = ctx->cur_strip_dev + base; ++ctx->strip_index_subs; }
  }
  // a sub-batch that holds a prior takes the priors form of the step, with the terms of this iteration's transforms in front of it
  const bool subPriors = run.priors && c.priors->first[base + m] > c.priors->first[base];
  const PairPriors pp = { ctx->prior_first_dev + base, ctx->prior_terms_dev };
  if (!run.sub_own[k]) {
    StageTimer t(ctx, "project_cur", st);
    if (int rc = launch_project_cur(ctx, L, maxcap_cur, tag0)) return rc; }
  for (int i = 0; i < p->outer_iterations; ++i) {
    const unsigned tag = tag0 - (unsigned)i;      // epoch of this outer iteration's reference projection
    const int ownRef = (i == 0 && run.sub_ownref[k]) ? 1 : 0;
    if (!ownRef) { StageTimer t(ctx, "project_ref", st);
      if (int rc = launch_project(ctx, L, maxcap_ref, 0, tag)) return rc; }
    for (int j = 0; j < p->inner_iterations; ++j) {
      const bool lastInner = (j == p->inner_iterations - 1);
      { StageTimer t(ctx, "corr_linearize", st);
        // first inner pass: the linearizer's transform is bitwise the finder's (aligner.cpp:79,84)
        if (j == 0) launch_corr_linearize<true, false>(ctx, L, tag, 0, ownRef);
        else launch_corr_linearize<false, false>(ctx, L, tag, 0, ownRef); }
      if (subPriors) { StageTimer t(ctx, "prior_terms", st);
        hipLaunchKernelGGL(k_prior_terms, dim3(m), dim3(64), 0, st, L.pr, pp.first, (const PriorHost*)ctx->priors_dev, (PriorTerms*)ctx->prior_terms_dev,
                           (const Mat4*)nullptr, ctx->stop); }
      { StageTimer t(ctx, "solve", st);
        const int last = (lastInner && i == p->outer_iterations - 1) ? 1 : 0;
        if (subPriors) hipLaunchKernelGGL(k_solve_update_priors, dim3(m), dim3(256), 0, st, L.pr, run.ap, run.nb, lastInner ? 1 : 0, last, tag, ctx->stop, pp);
        else hipLaunchKernelGGL(k_solve_update, dim3(m), dim3(256), 0, st, L.pr, run.ap, run.nb, lastInner ? 1 : 0, last, tag, ctx->stop); }
    }
  }
  if ((c.statistics || c.closure_records) && p->outer_iterations > 0) {
    StageTimer t(ctx, "statistics", st);
    launch_statistics(ctx, L, lastRefTag, ctx->stats_dev + base);
  }
  if (c.closure_records && p->outer_iterations > 0) {
    StageTimer t(ctx, "pair_statistics", st);
    hipLaunchKernelGGL(k_pair_statistics, dim3(m), dim3(64), 0, st, L.pr, (const SolveOut*)(ctx->stats_dev + base), ctx->pairstats_dev + base);
  }
  if (run.want_scores && p->outer_iterations > 0) {
    StageTimer t(ctx, "match_score", st);     // the z-buffers of this sub-batch still hold the finder's last depth images
    // blocks per pair: enough to fill the device together with the other pairs of the launch, few enough that the per-block atomics on the
    // pair's one record stay rare
    hipLaunchKernelGGL(k_match_score, dim3(std::min((N + 255) / 256, m >= 8 ? 64 : 256), m), dim3(256), 0, st, L.pr, N, lastRefTag, tag0, 1000.0f,
                       c.match_threshold, ctx->match_dev + base, run.sub_own[k] ? 1 : 0);
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
// Enqueue the records.  On ctx->stream (the streams have joined): the pair ids up, k_pack_records, and the records on their way to the caller -- as the kernel
// wrote them: straight into the caller's device buffer (what an all-gather sends), or through the context's own buffer into host memory.
static int align_enqueue_records(pwn_hip_ctx* ctx, const AlignCall& c) {
  const int n = c.n;
  if (n <= 0 || !c.records) return PWN_HIP_OK;
  const bool dev = is_device_ptr(c.records);
  const int rlen = c.closure_records ? kClosureRecordFloats : c.match_records ? kMatchRecordFloats : kRecordFloats;
  if (!dev) HIPCHK(ctx, ctx->records_ws.ensure((size_t)std::max(n, 64) * (c.closure_records ? kClosureRecordFloats : kMatchRecordFloats)), PWN_HIP_ERR_ALLOCATION);
  if (c.pair_ids) {
    HIPCHK(ctx, ctx->ids_dev.ensure((size_t)std::max(n, 64)), PWN_HIP_ERR_ALLOCATION);
    HIPCHK(ctx, copy_any(ctx->ids_dev, c.pair_ids, sizeof(int) * n, ctx->stream), PWN_HIP_ERR_COPY);
  }
  float* dst = dev ? c.records : ctx->records_ws;
  if (c.closure_records)
    hipLaunchKernelGGL(k_pack_closure_records, dim3(n), dim3(kClosureRecordFloats), 0, ctx->stream, ctx->pairs_dev, c.pair_ids ? (const int*)ctx->ids_dev : nullptr, c.first_pair_id, dst,
                       (const MatchAcc*)ctx->match_dev, c.p->outer_iterations > 0 ? (const PairStats*)ctx->pairstats_dev : nullptr);
  else
    hipLaunchKernelGGL(k_pack_records, dim3(n), dim3(c.match_records ? 128 : 64), 0, ctx->stream, ctx->pairs_dev, c.pair_ids ? (const int*)ctx->ids_dev : nullptr, c.first_pair_id, dst,
                       c.match_records ? (const MatchAcc*)ctx->match_dev : nullptr);
  if (!dev) HIPCHK(ctx, hipMemcpyAsync(c.records, ctx->records_ws, sizeof(float) * rlen * n, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}
// Enqueue the copy-backs and the end event.  On ctx->stream: everything of the call; nothing has been waited for.
static int align_enqueue_copybacks(pwn_hip_ctx* ctx, const AlignCall& c, const AlignRun& run) {
  const int n = c.n;
  if (n > 0 && c.scores) HIPCHK(ctx, hipMemcpyAsync(ctx->match_host, ctx->match_dev, sizeof(MatchAcc) * n, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  if (n > 0 && c.statistics) HIPCHK(ctx, hipMemcpyAsync(ctx->stats_host, ctx->stats_dev, sizeof(SolveOut) * n, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  if (n > 0 && c.statistics && c.closure_records && c.p->outer_iterations > 0)
    HIPCHK(ctx, hipMemcpyAsync(ctx->pairstats_host, ctx->pairstats_dev, sizeof(PairStats) * n, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  // direct_state: T, it and the traces of state_host[i] were written by the last k_solve_update of each pair (PairDesc::state_out); with no
  // iterations it still holds the initial state
  if (n > 0 && !run.direct_state && c.results) HIPCHK(ctx, hipMemcpyAsync(ctx->state_host, ctx->state_ws, sizeof(PairState) * n, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipEventRecord(ctx->t1, ctx->stream), PWN_HIP_ERR_LAUNCH);      // before the wait: recording it afterwards costs a second round trip per call
  return PWN_HIP_OK;
}

static void finish_match(const MatchAcc& a, pwn_hip_match_result* r) {
  r->image_non_zeros = (int)a.nonZeros;
  r->image_inliers = (int)a.inliers;
  r->image_outliers = (int)a.nonZeros - (int)a.inliers;
  r->image_reprojection_distance = match_reprojection_distance(a);               // the expression k_pack_records evaluates for the score words of a record
}
// a pair's result from its final state (transform, iterations, traces)
static void fill_result(pwn_hip_align_result& r, const PairState& st, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, float ms) {
  std::memset(&r, 0, sizeof(r));
  std::memcpy(r.T, st.T.m, sizeof(r.T));
  r.iterations = st.it;
  for (int k = 0; k < st.it && k < PWN_HIP_MAX_ITERATIONS; ++k) {
    r.chi2[k] = st.chi2[k]; r.iter_inliers[k] = st.inliers[k]; r.iter_correspondences[k] = st.ncorr[k]; r.iter_candidates[k] = st.ncand[k];
  }
  if (st.it > 0) { r.error = st.chi2[st.it - 1]; r.inliers = st.inliers[st.it - 1]; }
  r.n_reference = ref->content.n; r.n_current = cur->content.n;
  r.total_time_ms = ms;
}
// Aligner::_computeStatistics from the re-linearization at the final transform T (so: its sums; nullptr when the call ran no iteration)
static void fill_statistics(pwn_hip_align_statistics& q, const SolveOut* so, const Mat4& T) {
  std::memset(&q, 0, sizeof(q));
  if (!so) return;
  std::memcpy(q.H, so->H, sizeof(q.H)); std::memcpy(q.b, so->b, sizeof(q.b)); q.error = so->chi2; q.inliers = so->inliers;
  compute_statistics(so->H, T, q.mean, q.omega, &q.translational_eigen_ratio, &q.rotational_eigen_ratio);
}
// the same from the record k_pair_statistics wrote for the pair (the closure records: no 6x6 math on the host)
static void fill_statistics_from_device(pwn_hip_align_statistics& q, const SolveOut* so, const PairStats* ps) {
  std::memset(&q, 0, sizeof(q));
  if (!so) return;
  std::memcpy(q.H, so->H, sizeof(q.H)); std::memcpy(q.b, so->b, sizeof(q.b)); q.error = so->chi2; q.inliers = so->inliers;
  std::memcpy(q.mean, ps->mean, sizeof(q.mean)); std::memcpy(q.omega, ps->omega, sizeof(q.omega));
  q.translational_eigen_ratio = ps->translationalRatio; q.rotational_eigen_ratio = ps->rotationalRatio;
}
// Finish after the wait.  The streams are idle: the fault word is digested, scores, results and statistics are filled in, the finder's images are this call's.
static int align_finish(pwn_hip_ctx* ctx, const AlignCall& c, const AlignRun& run) {
  const int n = c.n;
  if (c.hooks && c.hooks->after_sync) { if (int rc = c.hooks->after_sync()) return rc; }
  if (int rc = take_align_fault(ctx)) return rc;
  for (int i = 0; i < n && c.scores; ++i) finish_match(ctx->match_host[i], &c.scores[i]);      // with or without `results` (pwn_hip_match_batch_records)
  float ms = 0.f; (void)hipEventElapsedTime(&ms, ctx->t0, ctx->t1);
  for (int i = 0; i < n && c.results; ++i) {
    fill_result(c.results[i], ctx->state_host[i], c.refs[i], c.curs[i], ms / n);
    if (c.statistics && !c.closure_records) fill_statistics(c.statistics[i], c.p->outer_iterations > 0 ? ctx->stats_host + i : nullptr, ctx->state_host[i].T);
  }
  for (int i = 0; i < n && c.statistics && c.closure_records; ++i)      // with or without `results`
    fill_statistics_from_device(c.statistics[i], c.p->outer_iterations > 0 ? ctx->stats_host + i : nullptr, ctx->pairstats_host + i);
  // batches: no current z-buffer after a skipped projection; a single alignment makes it on demand
  ctx->img.set(run.ap, run.slot0, n > 0 && (!run.any_own || n == 1), n == 1 && run.any_own);
  ctx->last_pairs = n; ctx->last_states_on_host = run.direct_state || c.results != nullptr;
  collect_stage_times(ctx);
  return PWN_HIP_OK;
}
// One attempt at the call; robust: every projection by the two-pass kernels
static int align_batch_once(pwn_hip_ctx* ctx, const AlignCall& call, bool robust) {
  AlignRun run; run.robust = robust;
  if (int rc = align_check_and_plan(ctx, call, run)) return rc;
  if (int rc = align_describe_pairs(ctx, call, run)) return rc;
  if (int rc = align_draw_tags(ctx, call, run)) return rc;
  if (int rc = plan_fork(ctx, run.plan)) return rc;
  for (int base = 0, k = 0; base < call.n; base += run.plan.sub, ++k) { if (int rc = align_enqueue_sub(ctx, call, run, base, k)) return rc; }
  if (int rc = plan_join(ctx, run.plan)) return rc;
  if (int rc = align_enqueue_records(ctx, call)) return rc;
  if (call.hooks && call.hooks->before_sync) { if (int rc = call.hooks->before_sync()) return rc; }
  if (int rc = align_enqueue_copybacks(ctx, call, run)) return rc;
  // everything of the call is queued, nothing has been waited for: the caller's moment to queue what depends on it on other streams, or to prepare
  // the next call, while the device works (pwn_hip_ctx_set_enqueued_callback)
  if (ctx->enqueued_cb && call.n > 0) ctx->enqueued_cb(ctx->enqueued_user);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  return align_finish(ctx, call, run);
}
// The call; and once more with the two-pass projection if one of its projections gave up on a pixel (z32_settle): nothing of the failed
// attempt is kept (states and descriptors are rebuilt, z-buffer tags move on; the hooks of a fused step convert the same frames into the same
// clouds again).  A fault in the repeat cannot happen (k_project_robust has no loop) and would be reported.
static int align_batch_impl(pwn_hip_ctx* ctx, const AlignCall& call) {
  return repeat_once(ctx, kSettleFault, [&](bool robust) { return align_batch_once(ctx, call, robust); });
}
// the members every batch entry point fills
static AlignCall align_call(const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs, const float* guesses,
                            pwn_hip_align_result* results) {
  AlignCall c; c.p = p; c.n = n; c.refs = refs; c.curs = curs; c.guesses = guesses; c.results = results;
  return c;
}
int pwn_hip_align_batch(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                        const float* guesses, pwn_hip_align_result* results) {
  return align_batch_impl(ctx, align_call(p, n, refs, curs, guesses, results));
}
int pwn_hip_match_batch(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                        const float* guesses, float threshold, pwn_hip_align_result* results, pwn_hip_match_result* scores) {
  if (!scores) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null scores");
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.scores = scores; call.match_threshold = threshold;
  return align_batch_impl(ctx, call);
}
int pwn_hip_align_with_priors(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, int n_priors,
                              const pwn_hip_prior* priors, pwn_hip_align_result* result) {
  return pwn_hip_align_with_priors_ex(ctx, p, ref, cur, n_priors, priors, result, nullptr);
}
// One pair of pwn_hip_align_batch_priors: the caller's n_priors records are the pair's list.  With priors the call is refused while the convergence
// setting is on (include/pwn_hip.h: a stated limit of this entry point) and for the null arguments it always refused, nothing touched.
int pwn_hip_align_with_priors_ex(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, int n_priors,
                                 const pwn_hip_prior* priors, pwn_hip_align_result* result, pwn_hip_align_statistics* statistics) {
  if (n_priors > 0 && ctx && ctx->stop.enabled) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "a single call with priors runs a fixed iteration count: switch the convergence setting off");
  pwn_hip_cloud* r[1] = { const_cast<pwn_hip_cloud*>(ref) };
  pwn_hip_cloud* c[1] = { const_cast<pwn_hip_cloud*>(cur) };
  AlignCall call = align_call(p, 1, r, c, nullptr, result);
  call.statistics = statistics;
  if (n_priors <= 0) return align_batch_impl(ctx, call);
  if (!ctx || !p || !ref || !cur || !priors || !result) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int first[2] = { 0, n_priors };
  pwn_hip_pair_priors list; list.first = first; list.priors = priors;
  if (!prior_list_ok(1, list.first, list.priors)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad prior list: n_priors records of kind 0 or 1");
  call.priors = &list;
  return align_batch_impl(ctx, call);
}
int pwn_hip_align_batch_ex(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                           const float* guesses, pwn_hip_align_result* results, float threshold, pwn_hip_match_result* scores,
                           pwn_hip_align_statistics* statistics) {
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.scores = scores; call.match_threshold = threshold; call.statistics = statistics;
  return align_batch_impl(ctx, call);
}
int pwn_hip_align_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                                const float* guesses, const int* pair_ids, int first_pair_id, pwn_hip_align_result* results, float* records) {
  if (!records) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null records");
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.records = records; call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return align_batch_impl(ctx, call);
}
int pwn_hip_match_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                                const float* guesses, float threshold, const int* pair_ids, int first_pair_id, pwn_hip_align_result* results,
                                pwn_hip_match_result* scores, float* records) {
  if (!records) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null records");
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.scores = scores; call.match_threshold = threshold; call.records = records; call.match_records = true; call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return align_batch_impl(ctx, call);
}
int pwn_hip_closure_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                                  const float* guesses, float threshold, const int* pair_ids, int first_pair_id, pwn_hip_align_result* results,
                                  pwn_hip_match_result* scores, pwn_hip_align_statistics* statistics, float* records) {
  if (!records) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null records");
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.scores = scores; call.match_threshold = threshold; call.statistics = statistics;
  call.records = records; call.closure_records = true; call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return align_batch_impl(ctx, call);
}
int pwn_hip_align_batch_priors(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs,
                               const float* guesses, const pwn_hip_pair_priors* pair_priors, float threshold, const int* pair_ids, int first_pair_id,
                               pwn_hip_align_result* results, pwn_hip_match_result* scores, pwn_hip_align_statistics* statistics, float* records,
                               int record_floats) {
  if (record_floats != 0 && record_floats != kRecordFloats && record_floats != kMatchRecordFloats && record_floats != kClosureRecordFloats)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "record_floats is none of 0 and the three record lengths");
  if ((record_floats != 0) != (records != nullptr)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "records and record_floats must be given together");
  if (pair_priors && !prior_list_ok(n, pair_priors->first, pair_priors->priors))
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "bad prior list: first[0] = 0, first non-decreasing, first[n] records of kind 0 or 1");
  AlignCall call = align_call(p, n, refs, curs, guesses, results);
  call.scores = scores; call.match_threshold = threshold; call.statistics = statistics; call.priors = pair_priors;
  call.records = records; call.match_records = record_floats == kMatchRecordFloats; call.closure_records = record_floats == kClosureRecordFloats;
  call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return align_batch_impl(ctx, call);
}
// The one-submission step: the reference frames (`ref`) and the current frames (`cur`, the same request but for frames and clouds) converted in
// front of the alignment `align` asks for, whose pairs are their clouds.  scale.step != 0: every frame is down-sampled in front of its
// conversion (rows, cols: the size that is converted and aligned)
static int convert_align_batch_impl(pwn_hip_ctx* ctx, const ConvertCall& ref, const ConvertCall& cur, const AlignCall& align) {
  const int n = align.n, rows = ref.rows, cols = ref.cols;
  if (int rc = check_image(ctx, rows, cols)) return rc;
  if (align.p->rows != rows || align.p->cols != cols) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "aligner image size differs from the frames'");
  // the clouds' host-side sizes are those of their PREVIOUS content while the step is being queued: bound what the conversion can produce instead
  if ((size_t)rows * cols > (size_t)kMaxAlignerPoints)
    return fail(ctx, PWN_HIP_ERR_CAPACITY, "Aligner::align: frames of more than 2^21 pixels (index field of the aligner's z-buffer word)");
  {   // sub-batches run on different streams: a cloud that appears twice would be written by two of them at once
    std::vector<const pwn_hip_cloud*> all; all.reserve((size_t)2 * std::max(n, 0));
    for (int i = 0; i < n; ++i) { all.push_back(align.refs[i]); all.push_back(align.curs[i]); }
    std::sort(all.begin(), all.end());
    if (std::adjacent_find(all.begin(), all.end()) != all.end()) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "the 2 n clouds of a step must be distinct");
  }
  // a hand-over time-out (see convert_batch_impl): the step once more, its conversions included
  return repeat_once(ctx, kHandoverTimeout, [&](bool) -> int {
    if (int rc = absorb_copies(ctx)) return rc;
    if (int rc = ensure_desc(ctx, 2 * n)) return rc;       // before anything of the step is queued: growing the descriptor arrays waits for the stream
    // the sub-batches and streams the alignment will use (align_batch_impl makes the same plan); the frames of sub-batch k -- its reference
    // frames, then its current frames -- are converted on k's stream in front of k's alignment, in launches of at most sub_frames frames that
    // reuse the stream's own block of frame slots
    const StreamPlan plan = make_plan(ctx, ctx->sub_pairs, n);
    const int sub = plan.sub;
    const int fslots = std::max(1, std::min(ctx->sub_frames, ctx->max_batch / plan.ns));
    std::vector<const void*> frames((size_t)2 * std::max(n, 0));
    std::vector<pwn_hip_cloud*> clouds((size_t)2 * std::max(n, 0));
    std::vector<int> slot((size_t)2 * std::max(n, 0));
    for (int base = 0, k = 0; base < n; base += sub, ++k) {
      const int m = std::min(sub, n - base);
      for (int j = 0; j < m; ++j) {
        frames[2 * base + j] = ref.frames[base + j]; clouds[2 * base + j] = ref.clouds[base + j];
        frames[2 * base + m + j] = cur.frames[base + j]; clouds[2 * base + m + j] = cur.clouds[base + j];
      }
      for (int f = 0; f < 2 * m; ++f) slot[2 * base + f] = (k % plan.ns) * fslots + f % fslots;
    }
    ConvertCall both = ref;                // one job for the 2 n frames, in the order they are converted
    both.n = 2 * n; both.frames = frames.data(); both.clouds = clouds.data();
    ConvertJob job;
    if (int rc = convert_prepare(ctx, both, slot, false, job)) return rc;
    AlignHooks hooks;
    hooks.pre_sub = [&](int base, int m, int, hipStream_t st) -> int {
      for (int f = 0; f < 2 * m; f += fslots) {
        const int cnt = std::min(fslots, 2 * m - f);
        if (job.host_input) { if (int rc = convert_stage_frames(ctx, job, 2 * base + f, cnt, st)) return rc; }
        if (int rc = convert_enqueue(ctx, job, 2 * base + f, cnt, st)) return rc;
      }
      return PWN_HIP_OK;
    };
    hooks.before_sync = [&]() -> int { return counts_enqueue(ctx, 2 * n); };
    hooks.after_sync = [&]() -> int { return convert_commit(ctx, job); };
    AlignCall call = align;
    call.hooks = &hooks;
    // the current frames as a depth source: the caller's own resident frames only -- a staged host frame or a down-sampled one lives in a workspace
    // slot that the next launch of conversions reuses
    const CurDepthFrames cur_depth = { cur.frames, cur.depth_scale, &job.cp };
    if (job.raw && !job.host_input && !both.scale.step) call.cur_depth = &cur_depth;
    return align_batch_impl(ctx, call);
  });
}
// what the step's conversions rely on (check_frames_and_clouds, for the 2 n frames and clouds), before a cloud is touched
static int check_step_clouds(pwn_hip_ctx* ctx, const ConvertCall& ref, const ConvertCall& cur) {
  if (int rc = check_frames_and_clouds(ctx, ref.frames, ref.clouds, ref.n)) return rc;
  if (int rc = check_frames_and_clouds(ctx, cur.frames, cur.clouds, cur.n)) return rc;
  if (ref.n > 0 && ref.clouds[0]->d.omSym != cur.clouds[0]->d.omSym)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "clouds of one convert batch must share one omega storage (exact9 / sym6)");
  return PWN_HIP_OK;
}
int pwn_hip_convert_align_batch_u16(pwn_hip_ctx* ctx, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, int n,
                                    const uint16_t* const* ref_frames, const uint16_t* const* cur_frames, float depth_scale, int rows, int cols,
                                    pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs, const float* guesses, const int* pair_ids, int first_pair_id,
                                    pwn_hip_align_result* results, float* records) {
  if (!ctx || !cp || !ap || !ref_frames || !cur_frames || !refs || !curs || (!results && !records) || n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const ConvertCall ref = convert_call(cp, ref_frames, depth_scale, n, rows, cols, refs), cur = convert_call(cp, cur_frames, depth_scale, n, rows, cols, curs);
  if (int rc = check_step_clouds(ctx, ref, cur)) return rc;
  AlignCall call = align_call(ap, n, refs, curs, guesses, results);
  call.records = records; call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return convert_align_batch_impl(ctx, ref, cur, call);
}
int pwn_hip_convert_align_batch_u16_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, int n,
                                           const uint16_t* const* ref_frames, const uint16_t* const* cur_frames, float depth_scale, int rows, int cols,
                                           pwn_hip_cloud* const* refs, pwn_hip_cloud* const* curs, const float* guesses, const int* pair_ids, int first_pair_id,
                                           pwn_hip_align_result* results, float* records, int step, float max_depth_cov) {
  if (!ctx || !cp || !ap || !ref_frames || !cur_frames || !refs || !curs || (!results && !records) || n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  ScaleSpec sc;
  if (int rc = make_scale_spec(ctx, rows, cols, step, max_depth_cov, sc)) return rc;
  ConvertCall ref = convert_call(cp, ref_frames, depth_scale, n, sc.orows, sc.ocols, refs), cur = convert_call(cp, cur_frames, depth_scale, n, sc.orows, sc.ocols, curs);
  ref.scale = cur.scale = sc;
  if (int rc = check_step_clouds(ctx, ref, cur)) return rc;
  if (int rc = check_scaled_capacities(ctx, ref)) return rc;
  if (int rc = check_scaled_capacities(ctx, cur)) return rc;
  if (int rc = ensure_scale(ctx, 2 * n)) return rc;
  AlignCall call = align_call(ap, n, refs, curs, guesses, results);
  call.records = records; call.pair_ids = pair_ids; call.first_pair_id = first_pair_id;
  return convert_align_batch_impl(ctx, ref, cur, call);
}
int pwn_hip_ctx_set_convergence(pwn_hip_ctx* ctx, const pwn_hip_convergence* s) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (!s || !s->enabled) { ctx->stop = StopRule{ 0, 0.f, 0.f, 0 }; return PWN_HIP_OK; }
  if (!std::isfinite(s->translation_epsilon) || !std::isfinite(s->rotation_epsilon) || s->translation_epsilon < 0.f || s->rotation_epsilon < 0.f)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "convergence epsilons must be finite and >= 0");
  if (s->min_iterations < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_iterations must be >= 0");
  ctx->stop = StopRule{ 1, s->translation_epsilon, s->rotation_epsilon, s->min_iterations };
  return PWN_HIP_OK;
}
int pwn_hip_ctx_get_convergence(const pwn_hip_ctx* ctx, pwn_hip_convergence* s) {
  if (!ctx || !s) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  s->enabled = ctx->stop.enabled; s->translation_epsilon = ctx->stop.epsT; s->rotation_epsilon = ctx->stop.epsR; s->min_iterations = ctx->stop.minIterations;
  return PWN_HIP_OK;
}
int pwn_hip_last_align_steps(pwn_hip_ctx* ctx, int first, int n, pwn_hip_align_steps* out) {
  if (!ctx || (!out && n > 0)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (first < 0 || n < 0 || (long long)first + n > ctx->last_pairs) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "pairs outside the last alignment call");
  if (n > 0 && !ctx->last_states_on_host) {      // the call returned records only: its final states are still in state_ws
    HIPCHK(ctx, hipMemcpyAsync(ctx->state_host, ctx->state_ws, sizeof(PairState) * ctx->last_pairs, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
    ctx->last_states_on_host = true;
  }
  for (int i = 0; i < n; ++i) {
    const PairState& st = ctx->state_host[first + i];
    pwn_hip_align_steps& o = out[i];
    std::memset(&o, 0, sizeof(o));
    o.iterations = st.outer; o.converged = st.frozen;
    for (int k = 0; k < st.outer && k < PWN_HIP_MAX_ITERATIONS; ++k) { o.step_translation[k] = st.stepT[k]; o.step_rotation[k] = st.stepR[k]; }
  }
  return PWN_HIP_OK;
}
void pwn_hip_compute_statistics(const float H[36], const float T[16], float mean[6], float omega[36], float* tr, float* rr) {
  compute_statistics(H, mat4_from(T), mean, omega, tr, rr);
}
void pwn_hip_prior_terms(const float invT[16], const pwn_hip_prior* prior, float Hp[36], float bp[6], int* valid) {
  PriorWork ws;
  const bool ok = prior_terms(SerialTeam(), prior_host_from(*prior), mat4_from(invT), Hp, bp, ws);
  if (!ok) { std::memset(Hp, 0, sizeof(float) * 36); std::memset(bp, 0, sizeof(float) * 6); }
  if (valid) *valid = ok ? 1 : 0;
}
// Test hook: the shipped k_prior_terms on n injected transforms with their prior lists, through the context's own prior arrays
int pwn_hip_debug_prior_terms_eval(pwn_hip_ctx* ctx, int n, const float* invT, const int* first, const pwn_hip_prior* priors, float* out) {
  if (!ctx || n < 0 || !prior_list_ok(n, first, priors) || (n > 0 && !invT) || (n > 0 && first[n] > 0 && !out))
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument or bad prior list");
  if (n == 0 || first[n] == 0) return PWN_HIP_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  static_assert(sizeof(Mat4) == 16 * sizeof(float), "a transform is 16 floats");
  DevBuf<Mat4> T;
  HIPCHK(ctx, T.alloc((size_t)n), PWN_HIP_ERR_ALLOCATION);
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(T, invT, sizeof(Mat4) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  if (int rc = upload_priors(ctx, n, first, priors, st)) return rc;
  const StopRule off = { 0, 0.f, 0.f, 0 };
  hipLaunchKernelGGL(k_prior_terms, dim3(n), dim3(64), 0, st, (const PairDesc*)nullptr, (const int*)ctx->prior_first_dev, (const PriorHost*)ctx->priors_dev,
                     (PriorTerms*)ctx->prior_terms_dev, (const Mat4*)T, off);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->prior_terms_dev, sizeof(PriorTerms) * (size_t)first[n], hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  return PWN_HIP_OK;
}
int pwn_hip_match_score(pwn_hip_ctx* ctx, float threshold, pwn_hip_match_result* out) {
  if (!ctx || !out) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!ctx->img.valid) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "no alignment has run on this context");
  const int N = ctx->img.ap.rows * ctx->img.ap.cols;
  // the descriptor of the pair in slot 0 is still in pairs_dev (clouds, z-buffers, state with the projection matrices)
  HIPCHK(ctx, hipMemsetAsync(ctx->match_dev, 0, sizeof(MatchAcc), ctx->stream), PWN_HIP_ERR_COPY);
  hipLaunchKernelGGL(k_match_score, dim3(std::min((N + 255) / 256, 256), 1), dim3(256), 0, ctx->stream, ctx->pairs_dev + ctx->img.pair, N, ctx->img.ref_tag,
                     ctx->img.cur_tag, 1000.0f, threshold, ctx->match_dev, ctx->img.cur_lazy ? 1 : 0);
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipMemcpyAsync(ctx->match_host, ctx->match_dev, sizeof(MatchAcc), hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  finish_match(ctx->match_host[0], out);
  return PWN_HIP_OK;
}
int pwn_hip_align(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* ref, const pwn_hip_cloud* cur, pwn_hip_align_result* result) {
  pwn_hip_cloud* r[1] = { const_cast<pwn_hip_cloud*>(ref) };
  pwn_hip_cloud* c[1] = { const_cast<pwn_hip_cloud*>(cur) };
  return pwn_hip_align_batch(ctx, p, 1, r, c, nullptr, result);
}
int pwn_hip_align_images(pwn_hip_ctx* ctx, int* ref_index, float* ref_depth, int* cur_index, float* cur_depth) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (!ctx->img.valid) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "no alignment has run on this context");
  const size_t N = (size_t)ctx->img.ap.rows * ctx->img.ap.cols;
  if (ctx->img.cur_lazy && (cur_index || cur_depth)) {      // the projection the alignment skipped, with the tag it had reserved for it
    // two-pass form straight away: one projection of one cloud, off the hot path, and no repeat to arrange (the pair's descriptor on the device
    // gets the depth image's address first)
    if (int rc = ensure_zdepth(ctx)) return rc;
    ctx->pairs_host[ctx->img.pair].zdepth = ctx->zdepth_ws;
    HIPCHK(ctx, hipMemcpyAsync(&ctx->pairs_dev[ctx->img.pair].zdepth, &ctx->pairs_host[ctx->img.pair].zdepth, sizeof(unsigned*), hipMemcpyHostToDevice, ctx->stream), PWN_HIP_ERR_COPY);
    const PairLaunch L = { &ctx->img.ap, 0, 0, 1, ctx->stream, ctx->pairs_dev + ctx->img.pair, ctx->zdepth_ws };
    if (int rc = launch_project(ctx, L, ctx->img.cur_cloud->d.capacity, 1, ctx->img.cur_tag)) return rc;
    HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
    ctx->img.cur_projected();
  }
  for (int pass = 0; pass < 2; ++pass) {
    int* oi = pass == 0 ? ref_index : cur_index; float* od = pass == 0 ? ref_depth : cur_depth;
    if (!oi && !od) continue;
    int* di = oi ? (is_device_ptr(oi) ? oi : ctx->index_ws) : nullptr;
    float* dd = od ? (is_device_ptr(od) ? od : ctx->depth_ws) : nullptr;
    hipLaunchKernelGGL(k_pair_images, dim3((unsigned)std::min<size_t>((N + 255) / 256, 2048)), dim3(256), 0, ctx->stream, ctx->pairs_dev + ctx->img.pair, pass,
                       pass == 0 ? ctx->img.ref_tag : ctx->img.cur_tag, (int)N, di, dd);
    HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
    if (oi && di != oi) HIPCHK(ctx, hipMemcpyAsync(oi, di, N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
    if (od && dd != od) HIPCHK(ctx, hipMemcpyAsync(od, dd, N * 4, hipMemcpyDeviceToHost, ctx->stream), PWN_HIP_ERR_COPY);
    HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  }
  return PWN_HIP_OK;
}
// Test hook: the aligner's projection launch (launch_project: its grid, its choice of kernel by n, its AlignParams with the context's settle guard)
// on n injected clouds, each under its own projector transform, through the context's own pair descriptors, states and z-buffer slots (pair i:
// slot i), with a tag from the running supply (the slots are not cleared), and every pair's images as k_pair_images reads them back.  No repeat:
// *gave_up is the call's settle word.  Everything is checked before anything is written.
int pwn_hip_debug_project_pairs(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* clouds, const float* transforms, int which,
                                int form, int* index_out, float* depth_out, int* gave_up) {
  if (!ctx || !p || !clouds || !transforms || !gave_up) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 1 || n > ctx->max_batch) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "pairs outside 1 .. max_batch");
  if ((which != 0 && which != 1) || (form != 0 && form != 1)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "which and form must be 0 or 1");
  if (p->min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  if (int rc = check_image(ctx, p->rows, p->cols)) return rc;
  int capacity = 0;
  for (int i = 0; i < n; ++i) {
    if (!clouds[i]) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null cloud");
    if (clouds[i]->owner != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "cloud of another context");
    if (std::min(clouds[i]->content.n, clouds[i]->d.capacity) > kMaxAlignerPoints)
      return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "a cloud holds more than 2^21 points (index field of the aligner's z-buffer word)");
    capacity = std::max(capacity, clouds[i]->d.capacity);
  }
  if (int rc = absorb_copies(ctx)) return rc;
  if (int rc = ensure_desc(ctx, n)) return rc;
  const bool robust = form == 1;
  if (int rc = start_align_attempt(ctx, robust)) return rc;
  ctx->img.invalidate();
  ctx->last_pairs = 0;
  const AlignParams ap = make_align_params(ctx, p);
  const size_t N = (size_t)p->rows * p->cols;
  hipStream_t st = ctx->stream;
  for (int i = 0; i < n; ++i) {
    fill_pair(ctx, i, i, clouds[i], clouds[i], nullptr, robust);
    PairState& hs = ctx->state_host[i];
    std::memset(&hs, 0, sizeof(hs));
    Mat4 iKRt; Mat3 iK;
    projector_matrices(ap.K, mat4_from(transforms + 16 * (size_t)i), hs.KRt, iKRt, iK);
    hs.KRtLast = hs.KRt; hs.KRtCur = hs.KRt;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->pairs_dev, ctx->pairs_host, sizeof(PairDesc) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->state_ws, ctx->state_host, sizeof(PairState) * n, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  unsigned tag = kZ32Tag0;
  if (int rc = take_tags32(ctx, 1, &tag)) return rc;
  const PairLaunch L = { &ap, align_nblocks((int)N), clouds[0]->d.omSym, n, st, ctx->pairs_dev, robust ? (unsigned*)ctx->zdepth_ws : nullptr, nullptr };
  if (int rc = launch_project(ctx, L, capacity, which, tag)) return rc;
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  for (int i = 0; i < n && (index_out || depth_out); ++i) {
    int* di = index_out ? ctx->index_ws + (size_t)i * N : nullptr;
    float* dd = depth_out ? ctx->depth_ws + (size_t)i * N : nullptr;
    hipLaunchKernelGGL(k_pair_images, dim3((unsigned)std::min<size_t>((N + 255) / 256, 2048)), dim3(256), 0, st, ctx->pairs_dev + i, which, tag, (int)N, di, dd);
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (index_out) HIPCHK(ctx, copy_any(index_out, ctx->index_ws, (size_t)n * N * 4, st), PWN_HIP_ERR_COPY);
  if (depth_out) HIPCHK(ctx, copy_any(depth_out, ctx->depth_ws, (size_t)n * N * 4, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  // the settle word, read and cleared here: a give-up is this call's result, not an error (take_align_fault would leave its message behind an OK)
  *gave_up = *(volatile int*)ctx->align_fault_host != 0 ? 1 : 0;
  *(volatile int*)ctx->align_fault_host = 0;
  return PWN_HIP_OK;
}

// ------------------------------------------------------------------------------------------------------- helpers
void pwn_hip_projector_matrices(const float K[9], const float T[16], float KRt[16], float iKRt[16], float iK[9]) {
  Mat4 a, b; Mat3 c;
  projector_matrices(mat3_from(K), mat4_from(T), a, b, c);
  if (KRt) std::memcpy(KRt, a.m, sizeof(a.m));
  if (iKRt) std::memcpy(iKRt, b.m, sizeof(b.m));
  if (iK) std::memcpy(iK, c.m, sizeof(c.m));
}
int pwn_hip_project_point(const float K[9], const float T[16], float min_distance, float max_distance, const float p[3], int* x, int* y, float* d) {
  if (!K || !T || !p) return 0;
  Mat4 KRt, iKRt; Mat3 iK;
  projector_matrices(mat3_from(K), mat4_from(T), KRt, iKRt, iK);
  const Vec3 ip = project_plane(KRt, p[0], p[1], p[2]);
  if (d) *d = ip.z;
  if (!depth_in_range(ip.z, min_distance, max_distance)) return 0;
  float fx, fy;
  round_to_pixel(ip, fx, fy);
  // the reference converts whatever comes out to int (undefined for values an int cannot hold); saturate instead, and give a NaN the
  // smallest int (the conversion of a NaN is as undefined as that of a large value: no pixel of any image either way)
  const float lim = 2147483520.0f;
  const auto to_int = [lim](float f) { return f != f ? -2147483647 - 1 : (int)(f > lim ? lim : (f < -lim ? -lim : f)); };
  if (x) *x = to_int(fx);
  if (y) *y = to_int(fy);
  return 1;
}
int pwn_hip_unproject_pixel(const float K[9], const float T[16], float min_distance, float max_distance, int x, int y, float d, float p[3]) {
  if (!K || !T || !p) return 0;
  if (!depth_in_range(d, min_distance, max_distance)) return 0;
  Mat4 KRt, iKRt; Mat3 iK;
  projector_matrices(mat3_from(K), mat4_from(T), KRt, iKRt, iK);
  const Vec3 q = unproject_pixel(iKRt, x, y, d);
  p[0] = q.x; p[1] = q.y; p[2] = q.z;
  return 1;
}
// Test hook, host code: converter_point -- the expression the stats pass stores and the fused pass's depth source recomputes -- of every pixel
// of a uint16 frame whose index is >= 0, written to points[3 * index]
int pwn_hip_debug_converter_points(const pwn_hip_converter_params* p, int rows, int cols, const uint16_t* raw, float depth_scale, const int* index_image,
                                   int capacity, float* points) {
  if (!p || !raw || !index_image || !points || rows <= 0 || cols <= 0) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const ConvertParams cp = make_convert_params(nullptr, p, nullptr, rows, cols, 0);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      const size_t pix = (size_t)r * cols + c;
      const int idx = index_image[pix];
      if (idx < 0 || idx >= capacity) continue;
      const Vec3 q = converter_point(cp.iKRt, cp.hasOffset, cp.offset, c, r, raw_to_metres(raw[pix], depth_scale));
      points[3 * (size_t)idx] = q.x; points[3 * (size_t)idx + 1] = q.y; points[3 * (size_t)idx + 2] = q.z;
    }
  return PWN_HIP_OK;
}
int pwn_hip_project_interval(const float K[9], float min_distance, float max_distance, float d, float world_radius) {
  if (!K) return -1;
  if (!depth_in_range(d, min_distance, max_distance)) return -1;
  float ivx, ivy;
  interval_scale(mat3_from(K), world_radius, ivx, ivy);
  return depth_interval(ivx, ivy, d);
}
void pwn_hip_iso_inverse(const float T[16], float out[16]) { const Mat4 r = iso_inverse(mat4_from(T)); std::memcpy(out, r.m, sizeof(r.m)); }
void pwn_hip_iso_mul(const float A[16], const float B[16], float out[16]) { const Mat4 r = iso_mul(mat4_from(A), mat4_from(B)); std::memcpy(out, r.m, sizeof(r.m)); }
void pwn_hip_v2t(const float v[6], float T[16]) { const Mat4 t = v2t(v); std::memcpy(T, t.m, sizeof(t.m)); }
void pwn_hip_t2v(const float T[16], float v[6]) { t2v(mat4_from(T), v); }
void pwn_hip_ldlt_solve6(const float H[36], const float b[6], float x[6]) { ldlt_solve6(H, b, x); }

// ---------------------------------------------------------------------------------------------------- consensus validation of closures
void pwn_hip_default_consensus_params(pwn_hip_consensus_params* p) {
  if (!p) return;
  p->inlier_translational_threshold = 0.5 * 0.5;                             // map_closer.cpp:63
  p->inlier_rotational_threshold = (float)(15.0f * M_PI / 180.0f);           // :64
  p->min_times_checked = 5;                                                  // :65
}
static const char* consensus_params_refused(const pwn_hip_consensus_params* p) {
  if (!p) return "null params";
  if (!(p->inlier_translational_threshold > 0.f)) return "the translational threshold must be positive";
  if (!(p->inlier_rotational_threshold > 0.f && (double)p->inlier_rotational_threshold <= kConsensusMaxRotThreshold))
    return "the rotational threshold must lie in (0, 2 pi / 3]: beyond it the decision depends on the Eigen version";
  return nullptr;
}
static ConsensusRel consensus_rel_host(const double* tc, const double* to, const double* tr, const int* flags, int i) {
  ConsensusRel r;
  consensus_prepare(tc + (size_t)16 * i, to + (size_t)16 * i, tr + (size_t)16 * i, nullptr, flags ? flags[i] : 0, r);
  return r;
}
void pwn_hip_validate_relation(int n, const double* tc, const double* to, const double* tr, const int* flags, int i, float* translational_errors,
                               float* rotational_errors) {
  if (n <= 0 || !tc || !to || !tr || i < 0 || i >= n || !translational_errors || !rotational_errors) return;
  const ConsensusRel ri = consensus_rel_host(tc, to, tr, flags, i);
  for (int j = 0; j < n; ++j) {
    const ConsensusRel rj = consensus_rel_host(tc, to, tr, flags, j);
    consensus_pair(ri.tfix, rj.tc, rj.toInv, rj.trInv, translational_errors[j], rotational_errors[j]);
  }
}
int pwn_hip_validate_relations_host(const pwn_hip_consensus_params* p, int n, const double* tc, const double* to, const double* tr, const int* flags,
                                    int* times_checked, int* cum_inlier, int* cum_outlier_times, int* decisions, float* translational_errors,
                                    float* rotational_errors, int* empty_column) {
  if (empty_column) *empty_column = -1;
  if (const char* why = consensus_params_refused(p)) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, why);
  if (n < 0) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "negative n");
  if (n > PWN_HIP_CONSENSUS_MAX_RELATIONS) return fail(nullptr, PWN_HIP_ERR_CAPACITY, "more than PWN_HIP_CONSENSUS_MAX_RELATIONS relations");
  if (n == 0) return PWN_HIP_OK;
  if (!tc || !to || !tr || !times_checked || !cum_inlier || !cum_outlier_times || !decisions)
    return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const float thrT = p->inlier_translational_threshold, thrR = p->inlier_rotational_threshold;
  std::vector<ConsensusRel> rel((size_t)n);
  for (int i = 0; i < n; ++i) rel[i] = consensus_rel_host(tc, to, tr, flags, i);
  const int W = (n + kConsensusTile - 1) / kConsensusTile;
  std::vector<unsigned long long> bits((size_t)W * n, 0ull);               // the device's layout: word (tile row a, column i) at a * n + i
  std::vector<int> counts((size_t)n, 0);
  int empty = -1;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      float te, re;
      consensus_pair(rel[i].tfix, rel[j].tc, rel[j].toInv, rel[j].trInv, te, re);
      if (translational_errors) translational_errors[(size_t)j + (size_t)n * i] = te;
      if (rotational_errors) rotational_errors[(size_t)j + (size_t)n * i] = re;
      if (consensus_is_in(te, re, thrT, thrR)) { bits[(size_t)(j / kConsensusTile) * n + i] |= 1ull << (j % kConsensusTile); counts[i] += 1; }
    }
    if (counts[i] == 0 && empty < 0) empty = i;
  }
  if (empty >= 0) {
    if (empty_column) *empty_column = empty;
    return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "no inliers in column " + std::to_string(empty));
  }
  for (int j = 0; j < n; ++j) {
    int in = 0, out = 0;
    for (int i = 0; i < n; ++i) { if ((bits[(size_t)(j / kConsensusTile) * n + i] >> (j % kConsensusTile)) & 1ull) in += counts[i]; else out += 1; }
    times_checked[j] += 1; cum_inlier[j] += in; cum_outlier_times[j] += out;
    decisions[j] = consensus_decision(times_checked[j], cum_inlier[j], cum_outlier_times[j], p->min_times_checked);
  }
  return PWN_HIP_OK;
}
int pwn_hip_validate_relations(pwn_hip_ctx* ctx, const pwn_hip_consensus_params* p, int n, const double* tc, const double* to, const double* tr,
                               const float* records, int record_floats, const int* flags, int* times_checked, int* cum_inlier,
                               int* cum_outlier_times, int* decisions, float* translational_errors, float* rotational_errors) {
  if (!ctx) return fail(nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null ctx");
  if (const char* why = consensus_params_refused(p)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, why);
  if (n < 0) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "negative n");
  if (n > PWN_HIP_CONSENSUS_MAX_RELATIONS) return fail(ctx, PWN_HIP_ERR_CAPACITY, "more than PWN_HIP_CONSENSUS_MAX_RELATIONS relations");
  if ((tr != nullptr) == (records != nullptr)) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "exactly one of tr and records must be given");
  if (records && record_floats != PWN_HIP_RECORD_FLOATS && record_floats != PWN_HIP_MATCH_RECORD_FLOATS && record_floats != PWN_HIP_CLOSURE_RECORD_FLOATS)
    return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "record_floats is not one of the three record sizes");
  if (n == 0) return PWN_HIP_OK;
  if (!tc || !to || !times_checked || !cum_inlier || !cum_outlier_times || !decisions) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  if (int rc = absorb_copies(ctx)) return rc;
  hipStream_t st = ctx->stream;
  const int W = (n + kConsensusTile - 1) / kConsensusTile;
  const size_t nn = (size_t)n * n;
  // host-side arrays pass through the staging block: inputs go up in front of the kernels, outputs come down behind them
  // (tc, to, tr, records, flags: up; the three counters and decisions: up and down; the two matrices, up to 256 MB each: down)
  struct Staged { void* user; size_t bytes; bool up, down; bool staged; size_t off; void* dev; };
  auto arg = [](const void* user, size_t bytes, bool up, bool down) { return Staged{ const_cast<void*>(user), bytes, up, down, false, 0, const_cast<void*>(user) }; };
  Staged a[11] = { arg(tc, sizeof(double) * 16 * n, true, false), arg(to, sizeof(double) * 16 * n, true, false), arg(tr, sizeof(double) * 16 * n, true, false),
                   arg(records, sizeof(float) * (size_t)record_floats * n, true, false), arg(flags, sizeof(int) * n, true, false),
                   arg(times_checked, sizeof(int) * n, true, true), arg(cum_inlier, sizeof(int) * n, true, true),
                   arg(cum_outlier_times, sizeof(int) * n, true, true), arg(decisions, sizeof(int) * n, true, true),
                   arg(translational_errors, sizeof(float) * nn, false, true), arg(rotational_errors, sizeof(float) * nn, false, true) };
  size_t need = 256;
  for (Staged& s : a)
    if (s.user && !is_device_ptr(s.user)) { s.staged = true; s.off = need; need += (s.bytes + 255) & ~(size_t)255; }
  HIPCHK(ctx, ctx->consensus_stage.ensure(need), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->consensus_rel.ensure((size_t)n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->consensus_bits.ensure((size_t)W * n), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->consensus_counts.ensure((size_t)n + 1), PWN_HIP_ERR_ALLOCATION);
  HIPCHK(ctx, ctx->consensus_flag_host.ensure(1), PWN_HIP_ERR_ALLOCATION);
  for (Staged& s : a) {
    if (!s.staged) continue;
    s.dev = ctx->consensus_stage.p + s.off;
    if (s.up) HIPCHK(ctx, hipMemcpyAsync(s.dev, s.user, s.bytes, hipMemcpyHostToDevice, st), PWN_HIP_ERR_COPY);
  }
  ctx->stages.clear();
  int* emptyDev = ctx->consensus_counts + n;
  {
    StageTimer t(ctx, "consensus_prepare");
    hipLaunchKernelGGL(k_consensus_prepare, dim3((n + 63) / 64), dim3(64), 0, st, n, (const double*)a[0].dev, (const double*)a[1].dev, (const double*)a[2].dev,
                       (const float*)a[3].dev, record_floats, (const int*)a[4].dev, (ConsensusRel*)ctx->consensus_rel, emptyDev);
  }
  {
    StageTimer t(ctx, "consensus_errors");
    hipLaunchKernelGGL(k_consensus_errors, dim3(W, W), dim3(kConsensusTile), 0, st, (const ConsensusRel*)ctx->consensus_rel, n, p->inlier_translational_threshold,
                       p->inlier_rotational_threshold, (unsigned long long*)ctx->consensus_bits, (float*)a[9].dev, (float*)a[10].dev);
  }
  {
    StageTimer t(ctx, "consensus_count");
    hipLaunchKernelGGL(k_consensus_count, dim3((n + 255) / 256), dim3(256), 0, st, (const unsigned long long*)ctx->consensus_bits, n, W, (int*)ctx->consensus_counts, emptyDev);
  }
  {
    StageTimer t(ctx, "consensus_commit");
    hipLaunchKernelGGL(k_consensus_commit, dim3(W), dim3(kConsensusTile), 0, st, (const unsigned long long*)ctx->consensus_bits, (const int*)ctx->consensus_counts,
                       (const int*)emptyDev, n, p->min_times_checked, (int*)a[5].dev, (int*)a[6].dev, (int*)a[7].dev, (int*)a[8].dev);
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  // a call that found an empty column committed nothing: its staged counters come back as they went up
  for (Staged& s : a)
    if (s.staged && s.down) HIPCHK(ctx, hipMemcpyAsync(s.user, s.dev, s.bytes, hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->consensus_flag_host, emptyDev, sizeof(int), hipMemcpyDeviceToHost, st), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, host_wait(ctx, st), PWN_HIP_ERR_LAUNCH);
  collect_stage_times(ctx);
  const int empty = ctx->consensus_flag_host[0];
  if (empty != kConsensusNoEmptyColumn) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "no inliers in column " + std::to_string(empty));
  return PWN_HIP_OK;
}

}  // extern "C"

#include "pwn_scene_capi.h"
#include "pwn_track_capi.h"
