// pwn_stats.h -- the 6x6 math of Aligner::_computeStatistics (reference pwn_core/aligner.cpp:152-199,
// pwn_core/unscented.h:23-65): covariance of the estimate from the final normal equations, unscented remap into the
// (t, q) chart of the solution, information matrix and the translational / rotational eigen-ratios.
// The reference uses Eigen's JacobiSVD / LLT / Matrix6f::inverse; symmetric cyclic Jacobi, Cholesky and Gauss-Jordan
// stand in for them here (results agree to fp32 round-off).
// One text for the host (pwn_hip_compute_statistics, fill_statistics) and the device (k_pair_statistics).  It is written for a TEAM: the loops
// whose turns do not depend on each other (the k loops of a Jacobi rotation, the rows of an elimination step, the 13 sigma points, the elements
// of a 6x6 sum) are dealt over the team's lanes and closed by team.sync(); everything else -- the rotation's angle, the pivot search, a
// Cholesky diagonal -- every lane computes for itself from the same stored values, so every branch is uniform.  On the host the team is one
// thread (SerialTeam: the loops are the plain loops, sync does nothing); on the device it is the 64 lanes of a workgroup (LaneTeam,
// pwn_kernels.h).  Every ELEMENT sees the same operations in the same order either way: the bits do not depend on the team.  Every array lives
// in a StatsWork the caller provides -- the stack on the host, LDS on the device, where the run-time indices of the pivot search and of the
// rotations would otherwise turn register arrays into scratch.  The SE(3) prior terms below are the same kind of text (PriorWork).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include "pwn_math.h"

namespace pwnhip {

struct SerialTeam {
  PWN_HD int lane() const { return 0; }
  PWN_HD int size() const { return 1; }
  PWN_HD void sync() const {}
};

// the arrays of compute_statistics and of the two solvers it calls (1.9 KB)
struct StatsWork {
  double wI[13], wP[13];
  float H[36], V[36], sigma[36], L[36], C[36], cov[36], ga[36], gb[36];
  float samples[13][6];
  float w[6], gf[6];
  float B[9], BtB[9], Vb[9], eb[3];
};

// eigen-decomposition of a symmetric n x n matrix (column-major, n <= 6) by cyclic Jacobi rotations; A must be in place for every lane (synced)
template <class Team>
PWN_HD void sym_eigen(const Team& tm, int n, float* A, float* V, float* w) {
  for (int i = tm.lane(); i < n * n; i += tm.size()) V[i] = 0.f;
  tm.sync();
  for (int i = tm.lane(); i < n; i += tm.size()) V[i + n * i] = 1.f;
  tm.sync();
  for (int sweep = 0; sweep < 30; ++sweep) {
    float off = 0.f;
    for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) off += A[p + n * q] * A[p + n * q];
    if (off < 1e-30f) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const float apq = A[p + n * q];
        if (std::fabs(apq) < 1e-30f) continue;
        const float theta = (A[q + n * q] - A[p + n * p]) / (2.f * apq);
        const float t = (theta >= 0.f ? 1.f : -1.f) / (std::fabs(theta) + std::sqrt(theta * theta + 1.f));
        const float c = 1.f / std::sqrt(t * t + 1.f), s = t * c;
        tm.sync();      // every lane has read the three entries (and the sweep's sum) before one of them changes
        for (int k = tm.lane(); k < n; k += tm.size()) { const float x = A[k + n * p], y = A[k + n * q]; A[k + n * p] = c * x - s * y; A[k + n * q] = s * x + c * y; }
        tm.sync();
        for (int k = tm.lane(); k < n; k += tm.size()) { const float x = A[p + n * k], y = A[q + n * k]; A[p + n * k] = c * x - s * y; A[q + n * k] = s * x + c * y; }
        for (int k = tm.lane(); k < n; k += tm.size()) { const float x = V[k + n * p], y = V[k + n * q]; V[k + n * p] = c * x - s * y; V[k + n * q] = s * x + c * y; }
        tm.sync();
      }
  }
  for (int i = tm.lane(); i < n; i += tm.size()) w[i] = A[i + n * i];
  tm.sync();
}
// a, b: n * n floats of work space each, f: n floats; Ain must be in place for every lane
template <class Team>
PWN_HD bool gauss_jordan_inverse(const Team& tm, int n, const float* Ain, float* out, float* a, float* b, float* f) {
  for (int i = tm.lane(); i < n * n; i += tm.size()) { a[i] = Ain[i]; b[i] = 0.f; }
  tm.sync();
  for (int i = tm.lane(); i < n; i += tm.size()) b[i + n * i] = 1.f;
  tm.sync();
  for (int c = 0; c < n; ++c) {
    int piv = c; float best = std::fabs(a[c + n * c]);
    for (int r = c + 1; r < n; ++r) if (std::fabs(a[r + n * c]) > best) { best = std::fabs(a[r + n * c]); piv = r; }
    if (best == 0.f) return false;
    tm.sync();      // the search is over for every lane
    if (piv != c) {
      for (int k = tm.lane(); k < n; k += tm.size()) {
        const float ta = a[c + n * k]; a[c + n * k] = a[piv + n * k]; a[piv + n * k] = ta;
        const float tb = b[c + n * k]; b[c + n * k] = b[piv + n * k]; b[piv + n * k] = tb;
      }
      tm.sync();
    }
    const float d = a[c + n * c];
    for (int r = tm.lane(); r < n; r += tm.size()) f[r] = a[r + n * c];      // the factors of the rows below and above, before column c is cleared
    tm.sync();
    for (int k = tm.lane(); k < n; k += tm.size()) { a[c + n * k] /= d; b[c + n * k] /= d; }
    tm.sync();
    for (int e = tm.lane(); e < n * n; e += tm.size()) {
      const int r = e % n, k = e / n;
      if (r != c && f[r] != 0.f) { a[r + n * k] -= f[r] * a[c + n * k]; b[r + n * k] -= f[r] * b[c + n * k]; }
    }
    tm.sync();
  }
  for (int i = tm.lane(); i < n * n; i += tm.size()) out[i] = b[i];
  tm.sync();
  return true;
}
inline bool gauss_jordan_inverse(int n, const float* Ain, float* out) {
  float a[36], b[36], f[6];
  return gauss_jordan_inverse(SerialTeam(), n, Ain, out, a, b, f);
}

// H: Linearizer::H() at the final transform (no damping), column-major; T: Aligner::_T.  mean, omega and the two ratios are written for the
// whole team to read (mean and omega by the lanes their elements were dealt to, a ratio by lane 0).
template <class Team>
PWN_HD void compute_statistics(const Team& tm, const float Hin[36], const Mat4& T, float mean[6], float omega[36], float* translationalRatio,
                               float* rotationalRatio, StatsWork& ws) {
  const int n = 6;
  float* H = ws.H; float* V = ws.V; float* w = ws.w;
  for (int i = tm.lane(); i < 36; i += tm.size()) H[i] = Hin[i];
  tm.sync();
  for (int i = tm.lane(); i < n; i += tm.size()) H[i + n * i] += 1.0f;    // aligner.cpp:169
  tm.sync();
  sym_eigen(tm, n, H, V, w);                                              // :172 (JacobiSVD of a symmetric PSD matrix)
  float smax = 0.f;
  for (int i = 0; i < n; ++i) smax = std::max(smax, std::fabs(w[i]));
  float* sigma = ws.sigma;
  for (int e = tm.lane(); e < 36; e += tm.size()) {                       // :173 svd.solve(Identity): pseudo-inverse
    const int i = e % n, j = e / n;
    float sg = 0.f;
    for (int k = 0; k < n; ++k) {
      if (std::fabs(w[k]) <= FLT_EPSILON * n * smax) continue;
      const float inv = 1.0f / w[k];
      sg += V[i + n * k] * inv * V[j + n * k];
    }
    sigma[e] = sg;
  }
  tm.sync();
  // unscented.h:23-50
  const double alpha = 1e-3, beta = 2., lambda = alpha * alpha * n;
  const double wi = 1. / (2. * (n + lambda));
  float* L = ws.L; float* C = ws.C;
  for (int i = tm.lane(); i < 36; i += tm.size()) { L[i] = 0.f; C[i] = sigma[i] * (float)(n + lambda); }
  tm.sync();
  for (int j = 0; j < n; ++j) {
    float d = C[j + n * j];
    for (int k = 0; k < j; ++k) d -= L[j + n * k] * L[j + n * k];
    d = std::sqrt(d);
    if (tm.lane() == 0) L[j + n * j] = d;
    for (int i = j + 1 + tm.lane(); i < n; i += tm.size()) { float v = C[i + n * j]; for (int k = 0; k < j; ++k) v -= L[i + n * k] * L[j + n * k]; L[i + n * j] = v / d; }
    tm.sync();
  }
  float (*samples)[6] = ws.samples; double* wI = ws.wI; double* wP = ws.wP;
  for (int k = tm.lane(); k < 13; k += tm.size()) {                       // sigma point k: 0 the mean, 2 i + 1 and 2 i + 2 = +- column i of L
    if (k == 0) {
      for (int r = 0; r < n; ++r) samples[0][r] = 0.f;
      wI[0] = lambda / (n + lambda); wP[0] = lambda / (n + lambda) + (1. - alpha * alpha + beta);
    } else {
      const int i = (k - 1) / 2;
      for (int r = 0; r < n; ++r) samples[k][r] = ((k - 1) & 1) ? -L[r + n * i] : L[r + n * i];
      wI[k] = wP[k] = wi;
    }
    const Mat4 X = iso_mul(T, iso_inverse(v2t(samples[k])));              // aligner.cpp:182-185
    t2v(X, samples[k]);
  }
  tm.sync();
  float* cov = ws.cov;                                                    // unscented.h:52-65
  for (int r = tm.lane(); r < n; r += tm.size()) {
    float m = 0.f;
    for (int k = 0; k < 13; ++k) m += (float)wI[k] * samples[k][r];
    mean[r] = m;
  }
  tm.sync();
  for (int e = tm.lane(); e < 36; e += tm.size()) {
    const int i = e % n, j = e / n;
    float cv = 0.f;
    for (int k = 0; k < 13; ++k) {
      const float di = samples[k][i] - mean[i], dj = samples[k][j] - mean[j];
      cv += (float)wP[k] * (di * dj);
    }
    cov[e] = cv;
  }
  tm.sync();
  if (!gauss_jordan_inverse(tm, n, cov, omega, ws.ga, ws.gb, ws.gf)) {    // aligner.cpp:190
    for (int i = tm.lane(); i < 36; i += tm.size()) omega[i] = 0.f;
    tm.sync();
  }
  for (int blk = 0; blk < 2; ++blk) {                                     // :193-198
    float* B = ws.B; float* BtB = ws.BtB; float* Vb = ws.Vb; float* eb = ws.eb;
    for (int e = tm.lane(); e < 9; e += tm.size()) { const int i = e % 3, j = e / 3; B[i + 3 * j] = omega[(i + 3 * blk) + n * (j + 3 * blk)]; }
    tm.sync();
    for (int e = tm.lane(); e < 9; e += tm.size()) {
      const int i = e % 3, j = e / 3;
      float acc = 0.f;
      for (int k = 0; k < 3; ++k) acc += B[k + 3 * i] * B[k + 3 * j];
      BtB[e] = acc;
    }
    tm.sync();
    sym_eigen(tm, 3, BtB, Vb, eb);
    float s0 = 0.f, s2 = FLT_MAX;
    for (int i = 0; i < 3; ++i) { const float sv = std::sqrt(std::max(eb[i], 0.f)); s0 = std::max(s0, sv); s2 = std::min(s2, sv); }
    if (tm.lane() == 0) (blk == 0 ? *translationalRatio : *rotationalRatio) = s0 / s2;
    tm.sync();
  }
}
inline void compute_statistics(const float Hin[36], const Mat4& T, float mean[6], float omega[36], float* translationalRatio, float* rotationalRatio) {
  StatsWork ws;
  compute_statistics(SerialTeam(), Hin, T, mean, omega, translationalRatio, rotationalRatio, ws);
}

// ---- SE(3) priors (reference pwn_core/se3_prior.{h,cpp}, consumed by aligner.cpp:96-108) ---------------------------
// One text again: prior_terms is what pwn_hip_prior_terms and prior_accumulate expand through SerialTeam and k_prior_terms through LaneTeam.  The prior is the device copy too (the arrays of a batch call hold PriorHost records).
struct PriorHost {
  int kind;            // 0: SE3RelativePrior (error = t2v(invT * mean)), 1: SE3AbsolutePrior (error = t2v(invT * ref^-1 * mean))
  Mat4 mean;           // _priorMean
  Mat4 invReference;   // _inverseReferenceTransform (identity for relative priors)
  float information[36];
};
// the arrays of prior_terms and of the inverse it calls (2.2 KB)
struct PriorWork {
  float ev[24][6];     // error 4 i + q of the numeric Jacobians: q = 0, 1 the +- steps of column i of J, q = 2, 3 those of Jz
  float e[6];
  float J[36], Jz[36], iJz[36], iJzT[36], t1[36], Om[36], Jt[36], t2[36];
  float ga[36], gb[36], gf[6];
};
PWN_HD void prior_error(const PriorHost& pr, const Mat4& mean, const Mat4& invT, float e[6]) {      // se3_prior.cpp:58-60,69-71
  const Mat4 X = pr.kind == 0 ? iso_mul(invT, mean) : iso_mul(iso_mul(invT, pr.invReference), mean);
  t2v(X, e);
}
// element e of the column-major product A * B, the inner product left to right
PWN_HD float mat6_mul_at(const float* A, const float* B, int e) {
  const int i = e % 6, j = e / 6;
  float s = A[i] * B[6 * j];
  for (int k = 1; k < 6; ++k) s = s + A[i + 6 * k] * B[k + 6 * j];
  return s;
}
template <class Team> PWN_HD void mat6_mul(const Team& tm, const float* A, const float* B, float* R) {
  for (int e = tm.lane(); e < 36; e += tm.size()) R[e] = mat6_mul_at(A, B, e);
  tm.sync();
}
template <class Team> PWN_HD void mat6_transpose(const Team& tm, const float* A, float* R) {
  for (int e = tm.lane(); e < 36; e += tm.size()) { const int i = e % 6, j = e / 6; R[i + 6 * j] = A[j + 6 * i]; }
  tm.sync();
}
// The terms one prior adds to the normal equations at Linearizer::_T = invT (aligner.cpp:99-107, the numeric Jacobians of se3_prior.cpp:8-52):
// Hp = J^T Omega' J and bp = J^T Omega' e, for the whole team to read.  false: the inverse of Jz was refused, the reference's `return` skips the
// prior, Hp and bp are not written.  pr and invT must be in place for every lane.
template <class Team>
PWN_HD bool prior_terms(const Team& tm, const PriorHost& pr, const Mat4& invT, float Hp[36], float bp[6], PriorWork& ws) {
  const float epsilon = 1e-3f, iEpsilon = 0.5f / epsilon;
  tm.sync();      // whoever read ws for the prior before this one is done
  for (int t = tm.lane(); t < 25; t += tm.size()) {
    if (t == 24) { prior_error(pr, pr.mean, invT, ws.e); continue; }
    const int i = t / 4, q = t % 4;
    float dv[6];
    for (int k = 0; k < 6; ++k) dv[k] = k != i ? 0.f : (q & 1) ? -epsilon : epsilon;
    if (q < 2) prior_error(pr, pr.mean, iso_mul(v2t(dv), invT), ws.ev[t]);      // jacobian
    else prior_error(pr, iso_mul(pr.mean, v2t(dv)), invT, ws.ev[t]);            // jacobianZ
  }
  tm.sync();
  for (int el = tm.lane(); el < 36; el += tm.size()) {
    const int r = el % 6, i = el / 6;
    ws.J[el] = iEpsilon * (ws.ev[4 * i][r] - ws.ev[4 * i + 1][r]);
    ws.Jz[el] = iEpsilon * (ws.ev[4 * i + 2][r] - ws.ev[4 * i + 3][r]);
  }
  tm.sync();
  if (!gauss_jordan_inverse(tm, 6, ws.Jz, ws.iJz, ws.ga, ws.gb, ws.gf)) return false;
  mat6_transpose(tm, ws.iJz, ws.iJzT); mat6_mul(tm, ws.iJzT, pr.information, ws.t1); mat6_mul(tm, ws.t1, ws.iJz, ws.Om);      // errorInformation
  mat6_transpose(tm, ws.J, ws.Jt); mat6_mul(tm, ws.Jt, ws.Om, ws.t2); mat6_mul(tm, ws.t2, ws.J, Hp);
  for (int i = tm.lane(); i < 6; i += tm.size()) { float sacc = ws.t2[i] * ws.e[0]; for (int k = 1; k < 6; ++k) sacc = sacc + ws.t2[i + 6 * k] * ws.e[k]; bp[i] = sacc; }
  tm.sync();
  return true;
}
// Adds the terms of one prior to H and b: the host statement of "terms, then add in list order", which the step on the device
// (k_solve_update_priors) is held against (tests/test_prior_terms_cpu.py); no alignment call runs it
inline void prior_accumulate(const PriorHost& pr, const Mat4& invT, float H[36], float b[6]) {
  PriorWork ws; float Hp[36], bp[6];
  if (!prior_terms(SerialTeam(), pr, invT, Hp, bp, ws)) return;
  for (int i = 0; i < 36; ++i) H[i] = H[i] + Hp[i];
  for (int i = 0; i < 6; ++i) b[i] = b[i] + bp[i];
}

}  // namespace pwnhip
