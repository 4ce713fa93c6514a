// pwn_track_capi.h -- C-ABI entry points of the multi-stream tracker (include/pwn_hip.h: pwn_hip_tracker, pwn_hip_track_frames); included by
// pwn_hip_capi.hip (same translation unit: it uses that file's context, cloud handle, conversion job and alignment phases).
// Reference: pwn_tracker/pwn_tracker.cpp:38-49 (init), :106-215 (processFrame).  The arithmetic and the two kernels: pwn_track.h.
#pragma once

// S streams, a ring of F + 1 clouds per stream, the S state records on the device and their page-locked mirror.  The mirror is the state after the
// last successful call (or set_state): what get_state returns, what an attempt that has to be made again starts from, and where the host reads which
// streams have no key cloud yet.
struct pwn_hip_tracker {
  pwn_hip_ctx* ctx = nullptr;
  int S = 0, F = 0, slots = 0;              // streams, frames per call at most, F + 1
  int rows = 0, cols = 0, step = 1;         // the SOURCE frames and DepthImage_scale's step
  int vrows = 0, vcols = 0;                 // the view: what is converted and aligned
  std::vector<pwn_hip_cloud*> ring;         // [S][slots]
  std::vector<char> converted;              // [S][slots]: a successful call has converted a frame into the slot (its cloud may still be empty)
  DevBuf<TrackState> state_dev; HostBuf<TrackState> state_host, state_back;      // state_back: where a call's final states arrive
  DevBuf<TrackItem> items_dev; HostBuf<TrackItem> items_host;                    // [F][S]: step f owns [f S, f S + S)
  DevBuf<CloudDev> ring_dev; HostBuf<CloudDev> ring_host;
  DevBuf<float> guesses_dev; DevBuf<Mat4> guess_dev;                             // the caller's initial guesses; the guesses k_track_begin formed
  HostBuf<TrackResult> results_host;
};

static_assert(sizeof(TrackState) == sizeof(pwn_hip_tracker_state) && offsetof(TrackState, keySlot) == offsetof(pwn_hip_tracker_state, key_slot), "state record layout");
static_assert(sizeof(TrackResult) == sizeof(pwn_hip_track_result) && offsetof(TrackResult, nPoints) == offsetof(pwn_hip_track_result, n_points), "result record layout");

namespace {

TrackState track_initial_state() {
  TrackState s; std::memset(&s, 0, sizeof(s));
  const Mat4 I = mat4_identity();
  std::memcpy(s.globalT, I.m, sizeof(I.m)); std::memcpy(s.previousCloudTransform, I.m, sizeof(I.m)); std::memcpy(s.sensorOffset, I.m, sizeof(I.m));
  s.keySlot = -1;
  return s;
}

// What one call of pwn_hip_track_frames asks for (every pointer checked by the entry point)
struct TrackCall {
  pwn_hip_tracker* tr; const pwn_hip_converter_params* cp; const pwn_hip_aligner_params* ap;
  int F; const uint16_t* const* frames; float depth_scale, max_depth_cov; const float* guesses; float threshold; pwn_hip_track_result* results;
};

// One attempt at the call: everything is queued -- the F S conversions on the conversion stream, per step k_track_begin, the sub-batches of the
// step's alignment and k_track_end on the context's streams -- and the host waits once.  robust: every projection by the two-pass kernels.
// Frame f of stream s goes into the f-th slot of the stream's ring that is not the key slot the stream ENTERED the call with: such a slot is
// written once per call, and the key during the call is either the one at entry or a slot written earlier in the call, so no conversion overwrites a
// key cloud.  No cloud is copied: a key switch is TrackState::keySlot.
int track_frames_once(pwn_hip_ctx* ctx, const TrackCall& c, bool robust, bool restore) {
  pwn_hip_tracker* tr = c.tr;
  const int S = tr->S, F = c.F, slots = tr->slots;
  if (int rc = absorb_copies(ctx)) return rc;
  if (int rc = ensure_desc(ctx, F * S)) return rc;
  if (int rc = ensure_scale(ctx, F * S)) return rc;
  ctx->img.invalidate(); ctx->last_pairs = 0; ctx->last_states_on_host = false; ctx->cur_depth_subs = 0; ctx->strip_index_subs = 0;
  if (int rc = start_align_attempt(ctx, robust)) return rc;
  ctx->stages.clear();
  hipStream_t st0 = ctx->stream;
  if (restore) HIPCHK(ctx, hipMemcpyAsync(tr->state_dev, tr->state_host, sizeof(TrackState) * S, hipMemcpyHostToDevice, st0), PWN_HIP_ERR_COPY);
  // ---- the items of every step, and the frames to convert in step order
  std::vector<const void*> frames; std::vector<pwn_hip_cloud*> clouds; std::vector<int> cslot;
  std::vector<int> conv0((size_t)F + 1, 0), npairs((size_t)F, 0), nitems((size_t)F, 0);
  std::vector<pwn_hip_cloud*> refs((size_t)F * S, nullptr), curs((size_t)F * S, nullptr);
  std::vector<char> has_key((size_t)S);
  const int fslots = std::max(1, std::min(ctx->sub_frames, ctx->max_batch));
  for (int s = 0; s < S; ++s) has_key[s] = tr->state_host[s].keySlot >= 0;
  for (int f = 0; f < F; ++f) {
    conv0[f] = (int)frames.size();
    TrackItem* items = tr->items_host + (size_t)f * S;
    auto item_of = [&](int s) {
      const int k0 = tr->state_host[s].keySlot;
      TrackItem it; it.stream = s; it.slot = (k0 >= 0 && f >= k0) ? f + 1 : f; it.result = f * S + s; it.pair = -1;      // the f-th slot that is not k0
      return it;
    };
    // the pairs first: the streams that hold a key cloud when the step begins
    int np = 0;
    for (int s = 0; s < S; ++s) {
      if (!c.frames[(size_t)f * S + s] || !has_key[s]) continue;
      TrackItem it = item_of(s);
      it.pair = f * S + np;
      refs[(size_t)it.pair] = tr->ring[(size_t)s * slots];      // the reference is the device's choice: any slot stands for its capacity
      curs[(size_t)it.pair] = tr->ring[(size_t)s * slots + it.slot];
      items[np++] = it;
    }
    // behind them the streams that take this frame as their first key cloud, without an alignment
    int ni = np;
    for (int s = 0; s < S; ++s) {
      if (!c.frames[(size_t)f * S + s] || has_key[s]) continue;
      items[ni++] = item_of(s);
    }
    for (int i = np; i < ni; ++i) has_key[items[i].stream] = 1;
    npairs[f] = np; nitems[f] = ni;
    for (int i = 0; i < nitems[f]; ++i) {
      const TrackItem& it = items[i];
      cslot.push_back((int)(frames.size() - (size_t)conv0[f]) % fslots);
      frames.push_back(c.frames[(size_t)it.result]); clouds.push_back(tr->ring[(size_t)it.stream * slots + it.slot]);
    }
  }
  conv0[F] = (int)frames.size();
  const int nconv = conv0[F];
  // ---- the conversions: one job, prepared on the context's stream (descriptor uploads)
  ConvertCall cc = convert_call(c.cp, reinterpret_cast<const uint16_t* const*>(frames.data()), c.depth_scale, nconv, tr->vrows, tr->vcols, clouds.data());
  if (int rc = make_scale_spec(ctx, tr->rows, tr->cols, tr->step, c.max_depth_cov, cc.scale)) return rc;
  for (int f = 0; f < F; ++f)      // what the slots held goes with the replace: until the call has succeeded they hold nothing
    for (int i = 0; i < nitems[f]; ++i) { const TrackItem& it = tr->items_host[(size_t)f * S + i]; tr->converted[(size_t)it.stream * slots + it.slot] = 0; }
  ConvertJob job;
  if (int rc = convert_prepare(ctx, cc, cslot, false, job)) return rc;
  // ---- the alignment's parameters, plan and tags
  AlignRun run; run.robust = robust;
  run.ap = make_align_params(ctx, c.ap); run.N = c.ap->rows * c.ap->cols; run.nb = align_nblocks(run.N);
  run.plan = make_plan(ctx, ctx->sub_pairs, S);
  const int sub = run.plan.sub;
  int nsub = 0;
  for (int f = 0; f < F; ++f) nsub += (npairs[f] + sub - 1) / sub;
  run.omSym = tr->ring[0]->d.omSym;
  run.sub_own.assign((size_t)nsub + 1, 1); run.sub_ownref.assign((size_t)nsub + 1, 0);
  const IndexKey key = index_key(c.ap);
  const bool shortcut = ctx->index_shortcut && is_identity(forced(c.ap->current_sensor_offset));
  Mat4 KRtCur0;
  { Mat4 iKRt0; Mat3 iK0; projector_matrices(run.ap.K, mat4_from(c.ap->current_sensor_offset), KRtCur0, iKRt0, iK0); }
  for (int f = 0, kk = 0; f < F; ++f)
    for (int base = 0; base < npairs[f]; base += sub, ++kk)
      for (int i = base; i < std::min(base + sub, npairs[f]); ++i) {
        const int e = f * S + i;
        const pwn_hip_cloud* cu = curs[(size_t)e];
        fill_pair(ctx, e, run.plan.slot0(kk) + (i - base), refs[(size_t)e], cu, nullptr, robust);
        if (!(shortcut && cu->content.idx_valid && cu->content.idx_key == key)) run.sub_own[(size_t)kk] = 0;
      }
  for (int f = 0, kk = 0; f < F; ++f)
    for (int base = 0; base < npairs[f]; base += sub, ++kk)
      for (int i = base; i < std::min(base + sub, npairs[f]); ++i)
        if (run.sub_own[(size_t)kk]) { ctx->pairs_host[f * S + i].curidx = curs[(size_t)(f * S + i)]->idximg; run.any_own = true; }
  { AlignCall tags; tags.p = c.ap; tags.n = nsub * sub;
    if (int rc = align_draw_tags(ctx, tags, run)) return rc; }
  for (int s = 0; s < S; ++s) for (int k = 0; k < slots; ++k) tr->ring_host[(size_t)s * slots + k] = tr->ring[(size_t)s * slots + k]->d;
  HIPCHK(ctx, hipEventRecord(ctx->t0, st0), PWN_HIP_ERR_LAUNCH);
  HIPCHK(ctx, hipMemcpyAsync(tr->ring_dev, tr->ring_host, sizeof(CloudDev) * (size_t)S * slots, hipMemcpyHostToDevice, st0), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(tr->items_dev, tr->items_host, sizeof(TrackItem) * (size_t)F * S, hipMemcpyHostToDevice, st0), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipMemcpyAsync(ctx->pairs_dev, ctx->pairs_host, sizeof(PairDesc) * (size_t)F * S, hipMemcpyHostToDevice, st0), PWN_HIP_ERR_COPY);
  if (c.guesses) HIPCHK(ctx, copy_any(tr->guesses_dev, c.guesses, sizeof(float) * 16 * (size_t)F * S, st0), PWN_HIP_ERR_COPY);
  // ---- the conversions of all steps on the conversion stream, behind the uploads: they depend on no alignment, so step f + 1 converts beside
  // step f's alignment.  done[f] (sync_events[f]) orders step f behind its frames' clouds.
  hipStream_t cvs = (ctx->copy_stream && ctx->stream == ctx->own_stream) ? ctx->copy_stream : st0;
  while ((int)ctx->sync_events.size() < F) {
    hipEvent_t e = nullptr;
    HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), PWN_HIP_ERR_ALLOCATION);
    ctx->sync_events.push_back(e);
  }
  if (cvs != st0) {
    HIPCHK(ctx, hipEventRecord(ctx->fork_ev, st0), PWN_HIP_ERR_LAUNCH);
    HIPCHK(ctx, hipStreamWaitEvent(cvs, ctx->fork_ev, 0), PWN_HIP_ERR_LAUNCH);
  }
  auto convert_step = [&](int f) -> int {
    for (int b = conv0[f]; b < conv0[f + 1]; b += fslots) {
      const int cnt = std::min(fslots, conv0[f + 1] - b);
      if (job.host_input) { if (int rc = convert_stage_frames(ctx, job, b, cnt, cvs)) return rc; }
      if (int rc = convert_enqueue(ctx, job, b, cnt, cvs)) return rc;
    }
    if (cvs != st0) HIPCHK(ctx, hipEventRecord(ctx->sync_events[(size_t)f], cvs), PWN_HIP_ERR_LAUNCH);
    return PWN_HIP_OK;
  };
  if (cvs != st0) for (int f = 0; f < F; ++f) { if (int rc = convert_step(f)) return rc; }
  // ---- the steps
  const Mat4 offset = forced(c.ap->current_sensor_offset);
  const float* guesses = c.guesses ? (const float*)tr->guesses_dev : nullptr;
  for (int f = 0, kk = 0; f < F; ++f) {
    if (nitems[f] == 0) continue;
    if (cvs == st0) { if (int rc = convert_step(f)) return rc; }
    else HIPCHK(ctx, hipStreamWaitEvent(st0, ctx->sync_events[(size_t)f], 0), PWN_HIP_ERR_LAUNCH);
    const TrackItem* items = tr->items_dev + (size_t)f * S;
    if (npairs[f] > 0) {
      { StageTimer t(ctx, "track_begin", st0);
        hipLaunchKernelGGL(k_track_begin, dim3((npairs[f] + 63) / 64), dim3(64), 0, st0, items, npairs[f], (const TrackState*)tr->state_dev, guesses,
                           (const CloudDev*)tr->ring_dev, slots, (PairDesc*)ctx->pairs_dev, run.ap, KRtCur0, (Mat4*)tr->guess_dev); }
      if (int rc = plan_fork(ctx, run.plan)) return rc;
      AlignCall step; step.p = c.ap; step.refs = refs.data(); step.curs = curs.data(); step.n = f * S + npairs[f];
      for (int base = 0; base < npairs[f]; base += sub, ++kk) { if (int rc = align_enqueue_sub(ctx, step, run, f * S + base, kk)) return rc; }
      if (int rc = plan_join(ctx, run.plan)) return rc;
    }
    { StageTimer t(ctx, "track_end", st0);
      hipLaunchKernelGGL(k_track_end, dim3((nitems[f] + 63) / 64), dim3(64), 0, st0, items, nitems[f], (TrackState*)tr->state_dev, (const PairDesc*)ctx->pairs_dev,
                         (const Mat4*)tr->guess_dev, (const CloudDev*)tr->ring_dev, slots, run.N, c.threshold, offset, (TrackResult*)tr->results_host); }
  }
  HIPCHK(ctx, hipGetLastError(), PWN_HIP_ERR_LAUNCH);
  if (int rc = counts_enqueue(ctx, nconv)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(tr->state_back, tr->state_dev, sizeof(TrackState) * S, hipMemcpyDeviceToHost, st0), PWN_HIP_ERR_COPY);
  HIPCHK(ctx, hipEventRecord(ctx->t1, st0), PWN_HIP_ERR_LAUNCH);
  // ---- the one wait
  HIPCHK(ctx, host_wait(ctx, st0), PWN_HIP_ERR_LAUNCH);
  collect_stage_times(ctx);
  if (int rc = take_align_fault(ctx)) return rc;      // the job withdraws its clouds; the repeat converts again
  if (int rc = convert_commit(ctx, job)) return rc;
  // ---- the call is done: the mirror moves on, the results leave
  std::memcpy(tr->state_host, tr->state_back, sizeof(TrackState) * S);
  for (int f = 0; f < F; ++f)
    for (int i = 0; i < nitems[f]; ++i) { const TrackItem& it = tr->items_host[(size_t)f * S + i]; tr->converted[(size_t)it.stream * slots + it.slot] = 1; }
  std::memset(c.results, 0, sizeof(pwn_hip_track_result) * (size_t)F * S);
  for (int f = 0; f < F; ++f)
    for (int i = 0; i < nitems[f]; ++i) {
      const int r = tr->items_host[(size_t)f * S + i].result;
      std::memcpy(&c.results[r], &tr->results_host[r], sizeof(TrackResult));
    }
  return PWN_HIP_OK;
}

}  // namespace

// What a tracker holds of its context is released; the handle stays valid for pwn_hip_tracker_destroy, every other entry point refuses it.
// (pwn_hip_ctx_destroy calls this for the trackers that are left, so that neither mirror frees anything twice.)
void tracker_orphan(pwn_hip_tracker* tr) {
  pwn_hip_ctx* ctx = tr->ctx;
  if (!ctx) return;
  (void)host_wait(ctx, ctx->stream);
  for (pwn_hip_cloud* cl : tr->ring) (void)pwn_hip_cloud_destroy(ctx, cl);
  tr->ring.clear(); tr->converted.clear();
  tr->state_dev.release(); tr->items_dev.release(); tr->ring_dev.release(); tr->guesses_dev.release(); tr->guess_dev.release();
  tr->state_host.release(); tr->state_back.release(); tr->items_host.release(); tr->ring_host.release(); tr->results_host.release();
  tr->ctx = nullptr;
}

extern "C" {

int pwn_hip_tracker_create(pwn_hip_ctx* ctx, int streams, int frames_per_call_max, int rows, int cols, int step, pwn_hip_tracker** out) {
  if (!ctx || !out) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (streams < 1 || frames_per_call_max < 1) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "a tracker has at least one stream and one frame per call");
  if (streams > ctx->max_batch) return fail(ctx, PWN_HIP_ERR_CAPACITY, "more streams than the context's max_batch");
  if ((long long)streams * frames_per_call_max > (1 << 20)) return fail(ctx, PWN_HIP_ERR_CAPACITY, "streams x frames per call exceeds 2^20");
  ScaleSpec sc;
  if (int rc = make_scale_spec(ctx, rows, cols, step, 0.f, sc)) return rc;
  if ((size_t)sc.orows * sc.ocols > (size_t)kMaxAlignerPoints) return fail(ctx, PWN_HIP_ERR_CAPACITY, "Aligner::align: frames of more than 2^21 pixels");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  pwn_hip_tracker* tr = new pwn_hip_tracker();
  tr->ctx = ctx; tr->S = streams; tr->F = frames_per_call_max; tr->slots = frames_per_call_max + 1;
  tr->rows = rows; tr->cols = cols; tr->step = step; tr->vrows = sc.orows; tr->vcols = sc.ocols;
  ctx->trackers.push_back(tr);
  const size_t S = (size_t)streams, FS = S * (size_t)frames_per_call_max, R = S * (size_t)tr->slots;
  hipError_t e = tr->state_dev.alloc(S);
  if (e == hipSuccess) e = tr->state_host.alloc(S);
  if (e == hipSuccess) e = tr->state_back.alloc(S);
  if (e == hipSuccess) e = tr->items_dev.alloc(FS);
  if (e == hipSuccess) e = tr->items_host.alloc(FS);
  if (e == hipSuccess) e = tr->ring_dev.alloc(R);
  if (e == hipSuccess) e = tr->ring_host.alloc(R);
  if (e == hipSuccess) e = tr->guesses_dev.alloc(FS * 16);
  if (e == hipSuccess) e = tr->guess_dev.alloc(FS);
  if (e == hipSuccess) e = tr->results_host.alloc(FS);
  if (e != hipSuccess) { pwn_hip_tracker_destroy(tr); return fail(ctx, PWN_HIP_ERR_ALLOCATION, std::string("tracker allocation: ") + hipGetErrorString(e)); }
  for (size_t i = 0; i < R; ++i) {
    pwn_hip_cloud* cl = nullptr;
    if (int rc = pwn_hip_cloud_create(ctx, sc.orows * sc.ocols, &cl)) { pwn_hip_tracker_destroy(tr); return rc; }
    tr->ring.push_back(cl);
    // what a conversion would otherwise make on first use, behind a wait for the stream (convert_prepare): the cloud's own index image and,
    // where the single-pass front end leaves one, its table of strip offsets
    hipError_t ea = cl->idximg.ensure((size_t)sc.orows * sc.ocols);
    if (ea == hipSuccess && sc.ocols % kIR_Cols == 0) ea = cl->stripoff.ensure((size_t)sc.orows * (size_t)strips_of(sc.ocols));
    if (ea != hipSuccess) { pwn_hip_tracker_destroy(tr); return fail(ctx, PWN_HIP_ERR_ALLOCATION, std::string("tracker allocation: ") + hipGetErrorString(ea)); }
  }
  tr->converted.assign(R, 0);
  for (size_t s = 0; s < S; ++s) tr->state_host[s] = track_initial_state();
  if (int rc = ensure_desc(ctx, (int)FS)) { pwn_hip_tracker_destroy(tr); return rc; }
  if (int rc = ensure_scale(ctx, (int)FS)) { pwn_hip_tracker_destroy(tr); return rc; }
  if (hipMemcpy(tr->state_dev, tr->state_host, sizeof(TrackState) * S, hipMemcpyHostToDevice) != hipSuccess) {
    pwn_hip_tracker_destroy(tr); return fail(ctx, PWN_HIP_ERR_COPY, "tracker: upload of the initial states failed");
  }
  *out = tr;
  return PWN_HIP_OK;
}

int pwn_hip_tracker_destroy(pwn_hip_tracker* tr) {
  if (!tr) return PWN_HIP_OK;
  if (pwn_hip_ctx* ctx = tr->ctx) {      // else: the context went first and took the clouds and the device records along
    (void)hipSetDevice(ctx->device);
    tracker_orphan(tr);
    ctx->trackers.erase(std::remove(ctx->trackers.begin(), ctx->trackers.end(), tr), ctx->trackers.end());
  }
  delete tr;
  return PWN_HIP_OK;
}

int pwn_hip_tracker_get_state(pwn_hip_tracker* tr, int first, int n, pwn_hip_tracker_state* out) {
  if (!tr || !out || !tr->ctx) return fail(tr ? tr->ctx : nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument, or a tracker whose context is gone");
  if (first < 0 || n < 0 || first + n > tr->S) return fail(tr->ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "streams outside the tracker's");
  std::memcpy(out, tr->state_host + first, sizeof(TrackState) * (size_t)n);
  return PWN_HIP_OK;
}

int pwn_hip_tracker_set_state(pwn_hip_tracker* tr, int first, int n, const pwn_hip_tracker_state* in) {
  if (!tr || !in || !tr->ctx) return fail(tr ? tr->ctx : nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument, or a tracker whose context is gone");
  pwn_hip_ctx* ctx = tr->ctx;
  if (first < 0 || n < 0 || first + n > tr->S) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "streams outside the tracker's");
  for (int i = 0; i < n; ++i) {
    const int k = in[i].key_slot;
    if (k < -1 || k >= tr->slots) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "key_slot outside -1 .. frames_per_call_max");
    if (k >= 0 && !tr->converted[(size_t)(first + i) * tr->slots + k]) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "key_slot names a slot that no frame has been converted into");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  HIPCHK(ctx, host_wait(ctx, ctx->stream), PWN_HIP_ERR_LAUNCH);
  std::memcpy(tr->state_host + first, in, sizeof(TrackState) * (size_t)n);
  HIPCHK(ctx, hipMemcpy(tr->state_dev + first, tr->state_host + first, sizeof(TrackState) * (size_t)n, hipMemcpyHostToDevice), PWN_HIP_ERR_COPY);
  return PWN_HIP_OK;
}

int pwn_hip_tracker_key_cloud(pwn_hip_tracker* tr, int s, pwn_hip_cloud** cloud) {
  if (!tr || !cloud || !tr->ctx) return fail(tr ? tr->ctx : nullptr, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument, or a tracker whose context is gone");
  if (s < 0 || s >= tr->S) return fail(tr->ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "stream outside the tracker's");
  const int k = tr->state_host[s].keySlot;
  *cloud = k >= 0 ? tr->ring[(size_t)s * tr->slots + k] : nullptr;
  return PWN_HIP_OK;
}

void pwn_hip_track_pose_update(pwn_hip_tracker_state* state, const float initial_guess[16], const float T[16], int inliers, int pixels, float threshold, int slot,
                               pwn_hip_track_result* result) {
  if (!state || !T || !result) return;
  TrackState s; std::memcpy(&s, state, sizeof(s));
  const Mat4 guess = track_guess(mat4_from(s.previousCloudTransform), mat4_from(s.globalT), initial_guess ? mat4_from(initial_guess) : mat4_identity());
  TrackResult r; std::memset(&r, 0, sizeof(r));
  r.aligned = 1; r.inliers = inliers;
  std::memcpy(r.T, T, sizeof(r.T));
  track_pose_update(s, guess, mat4_from(T), inliers, pixels, threshold, slot, &r.newFrame, &r.inliersFraction);
  std::memcpy(r.globalT, s.globalT, sizeof(r.globalT));
  std::memcpy(state, &s, sizeof(s)); std::memcpy(result, &r, sizeof(r));
}

int pwn_hip_track_frames(pwn_hip_ctx* ctx, pwn_hip_tracker* tr, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, int F,
                         const uint16_t* const* frames, float depth_scale, float max_depth_cov, const float* initial_guesses, float new_frame_inliers_fraction,
                         pwn_hip_track_result* results) {
  if (!ctx || !tr || !cp || !ap || !frames || !results) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (tr->ctx != ctx) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "tracker of another context");
  if (F < 1 || F > tr->F) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "frames per call outside 1 .. frames_per_call_max");
  if (tr->S > ctx->max_batch) return fail(ctx, PWN_HIP_ERR_CAPACITY, "more streams than the context's max_batch");
  if (ap->rows != tr->vrows || ap->cols != tr->vcols) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "aligner image size differs from the tracker's scaled frames'");
  if (int rc = check_image(ctx, tr->rows, tr->cols)) return rc;
  if (int rc = check_align_params(ctx, ap)) return rc;
  if (cp->min_distance < 0.f) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "min_distance must be >= 0");
  HIPCHK(ctx, hipSetDevice(ctx->device), PWN_HIP_ERR_NO_DEVICE);
  int kind = -1;      // the frames of a call are all host or all device memory (the conversion job stages host frames)
  for (size_t i = 0; i < (size_t)F * tr->S; ++i) {
    if (!frames[i]) continue;
    const int k = is_device_ptr(frames[i]) ? 1 : 0;
    if (kind >= 0 && k != kind) return fail(ctx, PWN_HIP_ERR_INVALID_ARGUMENT, "the frames of one call must be all host or all device memory");
    kind = k;
  }
  const TrackCall call = { tr, cp, ap, F, frames, depth_scale, max_depth_cov, initial_guesses, new_frame_inliers_fraction, results };
  // A projection that gave up on a pixel, or a converter strip whose hand-over timed out: the whole call once more, from the states it started with
  // (the mirror has not moved).  Any other failure leaves the device's records as the mirror has them, too.
  int attempts = 0;
  auto attempt = [&](bool robust) { return track_frames_once(ctx, call, robust, attempts++ > 0); };
  int rc = repeat_once(ctx, kSettleFault, attempt);
  if (rc == PWN_HIP_ERR_LAUNCH && attempts == 1 && ctx->last_convert_fault == 1) { ++ctx->convert_retries; rc = attempt(false); }
  if (rc != PWN_HIP_OK) {
    const std::string msg = ctx->err;
    (void)host_wait(ctx, ctx->stream);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipMemcpy(tr->state_dev, tr->state_host, sizeof(TrackState) * (size_t)tr->S, hipMemcpyHostToDevice);
    return fail(ctx, rc, msg);
  }
  return PWN_HIP_OK;
}

}  // extern "C"
