// pwn_consensus.h -- the consensus vote of MapCloser::validatePartitions (reference boss_map_building/map_closer.cpp:200-253, :286-417):
// for the n relations that join two partitions, the n x n pose errors of validateRelation, the two integer votes over them, and the decision
// per relation.  One text for the host (pwn_hip_validate_relation, pwn_hip_validate_relations_host) and the device (the kernels at the end):
// everything is double arithmetic in a fixed order (products ((a0 b0 + a1 b1) + a2 b2), no FMA: -ffp-contract=off), the square roots and
// divisions are IEEE operations, the one transcendental is pwn_atan2_pos (+ - * / only), so both sides produce the same bits.
//
// Relation i is a triple (tc_i, to_i, tr_i): the pose of its node in the current partition, of its node in the other partition, and its
// transform, which is inverted first when bit 0 of its flag is set (the reference's `else` branch, :211-214 / :231-234).
//   TR_i   = tr_i or tr_i^-1
//   tfix_i = (to_i * TR_i) * tc_i^-1                                         (:220-221)
//   pair (j, i):  tcp = tfix_i * tc_j,  trp = to_j^-1 * tcp,  te = TR_j^-1 * trp   (:239-244)
//   transErr = (float)((tx^2 + ty^2) + tz^2),  rotErr = (float)AngleAxisd(te.linear()).angle()   (:247-249)
//   isIn(j, i) = transErr < thrT && fabs(rotErr) < thrR                      (:349-351)
// The angle is Eigen 3.3's: Quaternion(Matrix3) without normalisation, n = |vec|, angle = n != 0 ? 2 atan2(n, |w|) : 0.  Eigen <= 3.2 returns
// 2 acos(w) instead, which differs only where w < 0 (it is then beyond pi, and 3.3 reports 2 pi minus it).  A negative w can only leave the
// three `trace <= 0` branches of the conversion, where |w| <= 0.5: there 3.3's angle is at least 2 acos(0.5) = 2 pi / 3 and 3.2's at least pi.
// So for every rotational threshold up to 2 pi / 3 both Eigen versions take the same decision, and the library refuses a larger threshold
// (kConsensusMaxRotThreshold) instead of choosing one of the two.
#pragma once
#include <cmath>
#include "pwn_math.h"

namespace pwnhip {

constexpr double kConsensusMaxRotThreshold = 2.0943951023931953;      // 2 pi / 3
constexpr int kConsensusNoEmptyColumn = 0x7fffffff;

// Isometry3d: linear part column-major, then the translation
struct IsoD {
  double r[9]; double t[3];
  PWN_HD double& operator()(int i, int j) { return r[i + 3 * j]; }
  PWN_HD double operator()(int i, int j) const { return r[i + 3 * j]; }
};
// what a pair evaluation reads of a relation: 48 doubles
struct ConsensusRel { IsoD tfix, tc, toInv, trInv; };

// the loops of api._iso_mul_d / _iso_inverse_d (and their twins in host/pwn_hip.hpp)
PWN_HD IsoD iso_mul_d(const IsoD& A, const IsoD& B) {
  IsoD R;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) { double s = A(i,0) * B(0,j); s = s + A(i,1) * B(1,j); s = s + A(i,2) * B(2,j); R(i,j) = s; }
    double s = A(i,0) * B.t[0]; s = s + A(i,1) * B.t[1]; s = s + A(i,2) * B.t[2];
    R.t[i] = s + A.t[i];
  }
  return R;
}
PWN_HD IsoD iso_inverse_d(const IsoD& T) {
  IsoD R;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R(i,j) = T(j,i);
    double s = T(0,i) * T.t[0]; s = s + T(1,i) * T.t[1]; s = s + T(2,i) * T.t[2];
    R.t[i] = -s;
  }
  return R;
}
// a 4x4 column-major matrix; the last row is not read (it is (0, 0, 0, 1) by definition)
PWN_HD IsoD iso_from_d(const double* m) {
  IsoD R;
  for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) R(i,j) = m[i + 4 * j];
  for (int i = 0; i < 3; ++i) R.t[i] = m[i + 12];
  return R;
}
// words [0:16] of a result record: float, column-major; convertScalar of the twelve upper entries
PWN_HD IsoD iso_from_f(const float* m) {
  IsoD R;
  for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) R(i,j) = (double)m[i + 4 * j];
  for (int i = 0; i < 3; ++i) R.t[i] = (double)m[i + 12];
  return R;
}

// AngleAxisd(Matrix3d).angle(), Eigen 3.3: Quaternion(Matrix3) -- the text of mat2quat (pwn_math.h) in double, WITHOUT its normalisation and
// sign fix -- then AngleAxis(Quaternion)
PWN_HD double rotation_angle_d(const IsoD& R) {
  double x, y, z, w;
  double t = (R(0,0) + R(1,1)) + R(2,2);
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    x = (R(2,1) - R(1,2)) * t;
    y = (R(0,2) - R(2,0)) * t;
    z = (R(1,0) - R(0,1)) * t;
  } else {
    int i = 0;
    if (R(1,1) > R(0,0)) i = 1;
    if (R(2,2) > (i == 0 ? R(0,0) : R(1,1))) i = 2;
    if (i == 0) {
      t = sqrt(R(0,0) - R(1,1) - R(2,2) + 1.0);
      x = 0.5 * t; t = 0.5 / t;
      w = (R(2,1) - R(1,2)) * t; y = (R(1,0) + R(0,1)) * t; z = (R(2,0) + R(0,2)) * t;
    } else if (i == 1) {
      t = sqrt(R(1,1) - R(2,2) - R(0,0) + 1.0);
      y = 0.5 * t; t = 0.5 / t;
      w = (R(0,2) - R(2,0)) * t; z = (R(2,1) + R(1,2)) * t; x = (R(0,1) + R(1,0)) * t;
    } else {
      t = sqrt(R(2,2) - R(0,0) - R(1,1) + 1.0);
      z = 0.5 * t; t = 0.5 / t;
      w = (R(1,0) - R(0,1)) * t; x = (R(0,2) + R(2,0)) * t; y = (R(1,2) + R(2,1)) * t;
    }
  }
  const double n = sqrt((x * x + y * y) + z * z);
  return n != 0.0 ? 2.0 * pwn_atan2_pos(n, w < 0.0 ? -w : w) : 0.0;
}

// relation i, from its three poses (tr: 16 doubles, or NULL and rec: the 16 floats of its record)
PWN_HD void consensus_prepare(const double* tc, const double* to, const double* tr, const float* rec, int flag, ConsensusRel& out) {
  const IsoD TC = iso_from_d(tc), TO = iso_from_d(to);
  const IsoD T0 = tr ? iso_from_d(tr) : iso_from_f(rec);
  const IsoD TR = (flag & 1) ? iso_inverse_d(T0) : T0;
  out.tfix = iso_mul_d(iso_mul_d(TO, TR), iso_inverse_d(TC));
  out.tc = TC;
  out.toInv = iso_inverse_d(TO);
  out.trInv = iso_inverse_d(TR);
}
// pair (j, i): the reference relation's tfix_i against relation j
PWN_HD void consensus_pair(const IsoD& tfix, const IsoD& tc, const IsoD& toInv, const IsoD& trInv, float& transErr, float& rotErr) {
  const IsoD tcp = iso_mul_d(tfix, tc);
  const IsoD trp = iso_mul_d(toInv, tcp);
  const IsoD te = iso_mul_d(trInv, trp);
  transErr = (float)((te.t[0] * te.t[0] + te.t[1] * te.t[1]) + te.t[2] * te.t[2]);
  rotErr = (float)rotation_angle_d(te);
}
PWN_HD bool consensus_is_in(float transErr, float rotErr, float thrT, float thrR) { return transErr < thrT && fabsf(rotErr) < thrR; }
// 0 skipped, 1 accepted, 2 removed (:385-414)
PWN_HD int consensus_decision(int timesChecked, int cumInlier, int cumOutlierTimes, int minTimesChecked) {
  return timesChecked < minTimesChecked ? 0 : (cumInlier > cumOutlierTimes ? 1 : 2);
}

// ---- the device side -------------------------------------------------------------------------------------------------------------------
// Four launches on one stream.  The n x n isIn matrix is kept as bits: word (tile row a, column i) = isIn(64 a .. 64 a + 63, i), stored at
// bits[a * n + i], so that the wave that produced it stores consecutive words and the wave that commits rows 64 a .. reads consecutive ones.
// No kernel waits for another workgroup, the only atomic is an integer minimum, every sum is an integer sum: the results do not depend on
// the launch geometry or on which workgroup arrives first.
constexpr int kConsensusTile = 64;

// one thread per relation; thread 0 lowers the empty-column word
__global__ void __launch_bounds__(64) k_consensus_prepare(int n, const double* __restrict__ tc, const double* __restrict__ to, const double* __restrict__ tr,
                                                          const float* __restrict__ records, int recordFloats, const int* __restrict__ flags,
                                                          ConsensusRel* __restrict__ rel, int* __restrict__ emptyColumn) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i == 0) *emptyColumn = kConsensusNoEmptyColumn;
  if (i >= n) return;
  ConsensusRel r;
  consensus_prepare(tc + (size_t)16 * i, to + (size_t)16 * i, tr ? tr + (size_t)16 * i : nullptr, records ? records + (size_t)recordFloats * i : nullptr,
                    flags ? flags[i] : 0, r);
  rel[i] = r;
}
// One wave per 64 x 64 tile: lane l owns row j = 64 blockIdx.x + l and keeps its (tc_j, to_j^-1, TR_j^-1) in registers, the tile's tfix_i sit
// in LDS, where every lane reads the same address (a broadcast, no bank conflict), and the wave walks the tile's columns together: the ballot
// of isIn over the lanes is the tile's word of column i.  The loop count is the same for every lane (the ballot needs them all); a lane
// beyond n votes 0 and stores nothing.
__global__ void __launch_bounds__(kConsensusTile) k_consensus_errors(const ConsensusRel* __restrict__ rel, int n, float thrT, float thrR,
                                                                     unsigned long long* __restrict__ bits, float* __restrict__ transErrs,
                                                                     float* __restrict__ rotErrs) {
  __shared__ IsoD fix[kConsensusTile];
  const int lane = threadIdx.x;
  const int j = blockIdx.x * kConsensusTile + lane, i0 = blockIdx.y * kConsensusTile;
  const int cols = min(kConsensusTile, n - i0);
  for (int e = lane; e < cols * 12; e += kConsensusTile) {
    const int c = e / 12, k = e % 12;
    ((double*)&fix[c])[k] = ((const double*)&rel[i0 + c].tfix)[k];
  }
  __syncthreads();
  const bool live = j < n;
  const ConsensusRel& mine = rel[live ? j : 0];
  const IsoD tc = mine.tc, toInv = mine.toInv, trInv = mine.trInv;
  for (int c = 0; c < cols; ++c) {
    float te, re;
    consensus_pair(fix[c], tc, toInv, trInv, te, re);
    const unsigned long long word = __ballot(live && consensus_is_in(te, re, thrT, thrR));
    if (lane == 0) bits[(size_t)blockIdx.x * n + i0 + c] = word;
    if (live && transErrs) transErrs[(size_t)j + (size_t)n * (i0 + c)] = te;
    if (live && rotErrs) rotErrs[(size_t)j + (size_t)n * (i0 + c)] = re;
  }
}
// c_i = the inliers of column i, over its W = ceil(n / 64) words; a column without one is the reference's "no inliers": the smallest such
// column ends up in *emptyColumn
__global__ void __launch_bounds__(256) k_consensus_count(const unsigned long long* __restrict__ bits, int n, int W, int* __restrict__ counts,
                                                         int* __restrict__ emptyColumn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int s = 0;
  for (int a = 0; a < W; ++a) s += __popcll(bits[(size_t)a * n + i]);
  counts[i] = s;
  if (s == 0) atomicMin(emptyColumn, i);
}
// one thread per relation j (a block is one tile row: its 64 lanes read the same word): the votes of every column added into its three
// counters, then its decision.  Nothing is written when a column was empty.
__global__ void __launch_bounds__(kConsensusTile) k_consensus_commit(const unsigned long long* __restrict__ bits, const int* __restrict__ counts,
                                                                     const int* __restrict__ emptyColumn, int n, int minTimesChecked,
                                                                     int* __restrict__ timesChecked, int* __restrict__ cumInlier,
                                                                     int* __restrict__ cumOutlierTimes, int* __restrict__ decisions) {
  if (*emptyColumn != kConsensusNoEmptyColumn) return;
  const int j = blockIdx.x * kConsensusTile + threadIdx.x;
  if (j >= n) return;
  const unsigned long long* row = bits + (size_t)blockIdx.x * n;
  const int b = threadIdx.x;
  int in = 0, out = 0;
  for (int i = 0; i < n; ++i) {
    if ((row[i] >> b) & 1ull) in += counts[i]; else out += 1;
  }
  const int t = timesChecked[j] + 1, ci = cumInlier[j] + in, co = cumOutlierTimes[j] + out;
  timesChecked[j] = t; cumInlier[j] = ci; cumOutlierTimes[j] = co;
  decisions[j] = consensus_decision(t, ci, co, minTimesChecked);
}

}  // namespace pwnhip
