// pwn_track.h -- PwnTracker::processFrame (pwn_tracker/pwn_tracker.cpp:106-215) for S independent streams that advance in lock-step: the part
// of the tracker that sits between two alignments -- the guess, the pose chain, the key-cloud decision and the switch of the reference cloud --
// as one arithmetic text for host and device, and the two kernels that run it in front of and behind a step's batch alignment.
//
// The records (TrackState, TrackResult) have the layout of pwn_hip_tracker_state / pwn_hip_track_result (include/pwn_hip.h).  The 4x4 / 3x3
// arithmetic is pwn_math.h's: inner products left to right, no FMA (this file is compiled with -ffp-contract=off like the rest), so that host,
// device and the Python mirror (api._mul3, api.iso_mul) arrive at the same bits.
#pragma once

#include "pwn_kernels.h"

namespace pwnhip {

struct TrackState {
  float globalT[16];                    // PwnTracker::_globalT
  float previousCloudTransform[16];     // _previousCloudTransform
  float sensorOffset[16];               // _previousCloudOffset, recorded when the stream takes its first key cloud (pwn_tracker.cpp:194-200)
  int counter, numKeyframes;            // _counter, _numKeyframes
  int keySlot;                          // slot of the stream's ring that holds _previousCloud; -1: none (PwnTracker::init)
  int reserved;
};
struct TrackResult {
  int newFrame, aligned, inliers;
  float error;
  float T[16], globalT[16];
  float inliersFraction;
  int nPoints;                          // points of the frame's cloud
};
// One frame of one stream inside a step.  pair: the entry of the step's alignment that tracks it (descriptor pairs[pair], state pairs[pair].state),
// -1 = the stream has no key cloud yet and takes this frame as its key without an alignment.  slot: where the frame's cloud was converted to.
struct TrackItem { int stream, pair, slot, result; };

// Eigen::Isometry3f guess = _previousCloudTransform.inverse() * _globalT * initialGuess (pwn_tracker.cpp:132)
PWN_HD Mat4 track_guess(const Mat4& prevT, const Mat4& globalT, const Mat4& initialGuess) {
  return iso_mul(iso_mul(iso_inverse(prevT), globalT), initialGuess);
}
// R - (0.5 R)(R^T R - I) (pwn_tracker.cpp:154-159)
PWN_HD void track_reorthonormalize(Mat4& G) {
  const Mat3 R = iso_linear(G);
  Mat3 Rt, H;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { Rt(i,j) = R(j,i); H(i,j) = 0.5f * R(i,j); }
  Mat3 E = mat3_mul(Rt, R);
  for (int i = 0; i < 3; ++i) E(i,i) = E(i,i) - 1.0f;
  const Mat3 C = mat3_mul(H, E);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) G(i,j) = R(i,j) - C(i,j);
}
// What processFrame does with an alignment's result (pwn_tracker.cpp:146-185, 211): the pose chain, the re-orthonormalisation of every 50th frame,
// the forced last row, the key-cloud decision -- the fraction and the threshold compared as floats, as the reference's members are
// (pwn_tracker.h:98) -- and the counters.  slot: where this frame's cloud lies (the key slot after a switch).
PWN_HD void track_pose_update(TrackState& s, const Mat4& guess, const Mat4& T, int inliers, int pixels, float threshold, int slot,
                              int* newFrame, float* inliersFraction) {
  Mat4 G = inliers > 0 ? iso_mul(mat4_from(s.previousCloudTransform), T) : iso_mul(mat4_from(s.globalT), guess);
  if (!(s.counter % 50)) track_reorthonormalize(G);
  set_last_row(G);
  const float fraction = (float)inliers / (float)pixels;
  const int sw = fraction < threshold ? 1 : 0;
  for (int q = 0; q < 16; ++q) s.globalT[q] = G.m[q];
  if (sw) {
    s.numKeyframes = s.numKeyframes + 1;
    s.keySlot = slot;
    for (int q = 0; q < 16; ++q) s.previousCloudTransform[q] = G.m[q];
  }
  s.counter = s.counter + 1;
  *newFrame = sw; *inliersFraction = fraction;
}
// the first frame of a stream (pwn_tracker.cpp:194-200, 211): it is the key cloud, nothing is aligned
PWN_HD void track_first_frame(TrackState& s, int slot, const Mat4& offset) {
  s.keySlot = slot;
  for (int q = 0; q < 16; ++q) { s.previousCloudTransform[q] = s.globalT[q]; s.sensorOffset[q] = offset.m[q]; }
  s.numKeyframes = s.numKeyframes + 1;
  s.counter = s.counter + 1;
}

// In front of a step's alignment kernels, one thread per item of the step.  For an item with a pair: the guess from the stream's state and the
// caller's initial guess (guesses: one 4x4 per result index, nullptr = identity), the pair's initial state exactly as the host writes it for a batch
// call (set_pose: T, both inverses, the projector matrix of T * reference offset; the head of the state cleared), and the stream's key cloud as the pair's
// reference (ring: slots CloudDev records per stream).  The reference's own index image is never taken (PairDesc::refidx0 stays null): the host
// does not know the guess.  guessOut[pair]: the guess, for k_track_end.
__global__ void k_track_begin(const TrackItem* __restrict__ items, int n, const TrackState* __restrict__ states, const float* __restrict__ guesses,
                              const CloudDev* __restrict__ ring, int slots, PairDesc* __restrict__ pairs, AlignParams ap, Mat4 KRtCur, Mat4* __restrict__ guessOut) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const TrackItem it = items[i];
  if (it.pair < 0) return;
  const TrackState& s = states[it.stream];
  const Mat4 init = guesses ? mat4_from(guesses + 16 * (size_t)it.result) : mat4_identity();
  Mat4 T = track_guess(mat4_from(s.previousCloudTransform), mat4_from(s.globalT), init);
  guessOut[it.pair] = T;
  set_last_row(T);
  PairDesc& pd = pairs[it.pair];
  const int key = min(max(s.keySlot, 0), slots - 1);
  pd.ref = ring[(size_t)it.stream * slots + key];
  PairState* st = pd.state;
  st->T = T;
  st->invTcorr = iso_inverse(T);
  Mat4 invT = st->invTcorr; set_last_row(invT);
  st->invT = invT;
  Mat4 zero; for (int q = 0; q < 16; ++q) zero.m[q] = 0.f;
  st->invTcorrPrev = zero;
  Mat4 KRt, iKRt; Mat3 iK;
  projector_matrices(ap.K, iso_mul(T, ap.refOffset), KRt, iKRt, iK);
  st->KRt = KRt; st->KRtLast = KRt; st->KRtCur = KRtCur;
  st->it = 0; st->frozen = 0; st->refTag = 0u; st->outer = 0;
}

// Behind the step's last solve, one thread per item: the pose chain and the key-cloud decision of the item's stream from the pair's final state,
// or the first frame's bookkeeping; the result record goes to the host's page-locked array.
__global__ void k_track_end(const TrackItem* __restrict__ items, int n, TrackState* __restrict__ states, const PairDesc* __restrict__ pairs,
                            const Mat4* __restrict__ guessIn, const CloudDev* __restrict__ ring, int slots, int pixels, float threshold, Mat4 offset,
                            TrackResult* results) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const TrackItem it = items[i];
  TrackState s = states[it.stream];
  TrackResult r;
  r.newFrame = 1; r.aligned = 0; r.inliers = 0; r.error = 0.f; r.inliersFraction = 0.f;
  for (int q = 0; q < 16; ++q) r.T[q] = 0.f;
  const CloudDev& cl = ring[(size_t)it.stream * slots + it.slot];
  r.nPoints = max(0, min(*cl.count, cl.capacity));
  if (it.pair >= 0) {
    const PairState* st = pairs[it.pair].state;
    const int nit = st->it;
    r.aligned = 1;
    if (nit > 0) { r.error = st->chi2[nit - 1]; r.inliers = st->inliers[nit - 1]; }
    for (int q = 0; q < 16; ++q) r.T[q] = st->T.m[q];
    track_pose_update(s, guessIn[it.pair], st->T, r.inliers, pixels, threshold, it.slot, &r.newFrame, &r.inliersFraction);
  } else {
    track_first_frame(s, it.slot, offset);
  }
  for (int q = 0; q < 16; ++q) r.globalT[q] = s.globalT[q];
  states[it.stream] = s;
  results[it.result] = r;
}

}  // namespace pwnhip
