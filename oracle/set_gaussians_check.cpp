/* Stand-alone check of orc_cloud_set_gaussians (test infrastructure): set, read back, refuse, then drive the calls that read the
 * Gaussian vector (add, transform, merge with a tail, voxel grid with matching and non-matching sizes).  Meant to be built together with
 * pwn_oracle.cpp under -fsanitize=address,undefined (make -C oracle set_gaussians_check_asan) and run once; exit status 0 = all held. */
#include "pwn_oracle.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

int main() {
  const int n = 300, ng = n + 5;
  std::vector<float> P(4 * n), N(4 * n), C(n), OP(16 * n, 0.f), ON(16 * n, 0.f);
  for (int i = 0; i < n; ++i) {
    const float z = 1.0f + 0.001f * (float)(i % 7);
    P[4 * i] = 0.01f * (float)(i % 5 - 2) * z; P[4 * i + 1] = 0.01f * (float)(i % 3 - 1) * z; P[4 * i + 2] = z; P[4 * i + 3] = 1.f;
    N[4 * i] = 0.f; N[4 * i + 1] = 0.f; N[4 * i + 2] = -1.f; N[4 * i + 3] = 0.f;
    C[i] = 0.01f;
    for (int a = 0; a < 3; ++a) { OP[16 * i + 5 * a] = 1.f + (float)a; ON[16 * i + 5 * a] = 100.f; }
  }
  std::vector<float> mean(3 * ng), cov(9 * ng, 0.f), iv(3 * ng), info(9 * ng, 0.f);
  std::vector<int> flags(ng);
  for (int i = 0; i < ng; ++i) {
    for (int a = 0; a < 3; ++a) {
      mean[3 * i + a] = (i < n ? P[4 * i + a] : 7.f) + 0.001f * (float)(a + 1);
      cov[9 * i + 4 * a] = 0.01f * (float)(a + 1); info[9 * i + 4 * a] = 1.f / cov[9 * i + 4 * a];
      iv[3 * i + a] = info[9 * i + 4 * a] * mean[3 * i + a];
    }
    flags[i] = 1 + i % 3;
  }
  orc_cloud* c = orc_cloud_create();
  orc_cloud_set(c, n, P.data(), N.data(), C.data(), OP.data(), ON.data());
  CHECK(orc_cloud_set_gaussians(c, ng, mean.data(), cov.data(), iv.data(), info.data(), flags.data()) == 0);
  CHECK(orc_cloud_num_gaussians(c) == ng);
  {
    std::vector<float> m2(3 * ng), c2(9 * ng), v2(3 * ng), i2(9 * ng); std::vector<int> f2(ng);
    orc_cloud_get_gaussians(c, m2.data(), c2.data(), v2.data(), i2.data(), f2.data());
    CHECK(!std::memcmp(m2.data(), mean.data(), 12 * ng) && !std::memcmp(c2.data(), cov.data(), 36 * ng));
    CHECK(!std::memcmp(v2.data(), iv.data(), 12 * ng) && !std::memcmp(i2.data(), info.data(), 36 * ng) && f2 == flags);
  }
  /* refusals leave the vector alone */
  CHECK(orc_cloud_set_gaussians(c, -1, mean.data(), cov.data(), iv.data(), info.data(), flags.data()) == 1);
  CHECK(orc_cloud_set_gaussians(c, 3, nullptr, cov.data(), iv.data(), info.data(), flags.data()) == 1);
  { std::vector<int> bad(flags); bad[2] = 4; CHECK(orc_cloud_set_gaussians(c, 3, mean.data(), cov.data(), iv.data(), info.data(), bad.data()) == 1); }
  CHECK(orc_cloud_num_gaussians(c) == ng);
  /* Cloud::add, transformInPlace, Merger::merge (tail of 5 kept), VoxelCalculator (sizes differ: no Gaussians; equal: gathered) */
  const float T[16] = { 0, 1, 0, 0,  -1, 0, 0, 0,  0, 0, 1, 0,  0.1f, 0.2f, 0.3f, 1 };
  const float I[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
  orc_cloud* s = orc_cloud_create();
  orc_cloud_add(s, c, T);
  CHECK(orc_cloud_size(s) == n && orc_cloud_num_gaussians(s) == ng);
  orc_cloud_transform_in_place(s, T);
  /* a source with fewer Gaussians than points: the destination gets the entries there are (size + n - 3 in all) */
  CHECK(orc_cloud_set_gaussians(c, n - 3, mean.data(), cov.data(), iv.data(), info.data(), flags.data()) == 0);
  orc_cloud_add(s, c, T);
  CHECK(orc_cloud_size(s) == 2 * n && orc_cloud_num_gaussians(s) == 2 * n - 3);
  CHECK(orc_cloud_set_gaussians(c, ng, mean.data(), cov.data(), iv.data(), info.data(), flags.data()) == 0);
  const float K[9] = { 50, 0, 0,  0, 50, 0,  31.5f, 23.5f, 1 };
  std::vector<int> collapsed(n);
  const int k = orc_merge(c, K, I, 0.5f, 5.f, 48, 64, 0.1f, 0.9f, 10.f, collapsed.data());
  CHECK(k > 0 && k < n && orc_cloud_size(c) == k && orc_cloud_num_gaussians(c) == ng);
  std::vector<int> kept(n);
  const int m = orc_voxelize(c, 0.01f, 0, kept.data());
  CHECK(m > 0 && m <= k && orc_cloud_num_gaussians(c) == 0);
  CHECK(orc_cloud_set_gaussians(c, m, mean.data(), cov.data(), iv.data(), info.data(), flags.data()) == 0);
  const int m2 = orc_voxelize(c, 0.02f, 0, kept.data());
  CHECK(m2 > 0 && orc_cloud_num_gaussians(c) == m2);
  CHECK(orc_cloud_set_gaussians(c, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 && orc_cloud_num_gaussians(c) == 0);
  orc_cloud_destroy(s); orc_cloud_destroy(c);
  std::printf(failures ? "set_gaussians_check: %d failures\n" : "set_gaussians_check: ok\n", failures);
  return failures ? 1 : 0;
}
