// pwn_kernels.h -- hand-written gfx950 kernels of the PWN dense-registration path.
//
// One kernel per stage of the reference's CPU path (g2o_frontend/pwn_core/, cited per kernel).
// All kernels are batched: blockIdx.y selects the frame / pair, whose buffers are described by a
// FrameDesc / PairDesc record in device memory.  Layout in HBM is SoA:
//   cloud:  P3[3*i .. 3*i+2] = x, y, z                     (Point: 12 bytes -- the projection reads nothing else)
//           Nc[i] = float4(nx, ny, nz, curvature)          (Normal + Stats::curvature(); the class of the normal information matrix --
//                   0 = zero, 1 = flat, 2 = non-flat -- is not stored: normal_class() derives it from this record and the threshold the
//                   cloud was converted with)
//           Om[((r*cap + i)*3 + c]                         (point information matrix: three planes of 12-byte rows, om_at(); nine dword
//                   planes until round 2: k_stats stores three 12-byte rows per point instead of nine dwords, -9 % of its time)
//           64 bytes per point; until round 2 the point carried the curvature and the normal a class word (68 bytes): the fused pass
//           fetches 8 bytes less per candidate (-7.5 % of its time), the projection 4 of 16 bytes less per point
//   images: row-major int32 / float32, lanes along image x (row-coalesced loads)
//   integral image: 10 planes [ch][rows][cols] (x y z n xx xy xz yy yz zz)
//   z-buffer of the aligner: uint32 per pixel = epoch tag (11 b) | point index (21 b), empty = ~0 (kZ32Tag0);
//   z-buffer of the stand-alone projection / Merger: uint64 = epoch tag (8 b) | float_bits(depth) (31 b) | point index (25 b)
// Arithmetic follows the reference's evaluation order (left-to-right inner products, no FMA:
// compiled with -ffp-contract=off) so integer outputs are bit-exact and fp32 outputs differ from
// the CPU path only through libm-vs-ocml trig and summation order of the H/b reduction.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "pwn_math.h"
#include "pwn_stats.h"

namespace pwnhip {

constexpr int kMaxIter = 64;
constexpr int kIntegralChannels = 10;
// The H/b sum record, one per thread, per block (fp64 partials) and per pair: the column-major 3x3 blocks Htt, Htr, Hrr of H, the halves bt, br
// of b and chi2 -- what linearize_term adds to (kAccTerms slots) -- then the counts: inliers, correspondences C, candidates K.
constexpr int kAccHtt = 0, kAccHtr = 9, kAccHrr = 18, kAccBt = 27, kAccBr = 30, kAccChi2 = 33, kAccTerms = kAccChi2 + 1;
constexpr int kAccInliers = kAccTerms, kAccCorr = kAccInliers + 1, kAccCand = kAccCorr + 1, kAccN = kAccCand + 1;
constexpr int kPixPerThread = 8;
constexpr int kAlignBlock = 256;
constexpr unsigned long long kZEmpty = ~0ull;
// 64-bit z-buffer word (stand-alone projection, Merger::merge: the scene stage) = epoch tag (8 bits) | depth bits (31, depth >= 0) |
// point index (25 bits).  Call number j uses tag kZTag0 - j: a smaller tag wins atomicMin, so words left by earlier projections behave
// as "empty" and the buffer is cleared only when the tag space is used up (take_tags).  The reference's clouds have no size limit; a scene
// grows by a frame per step (pwn_aligner.cpp:205-208: 1.2 M points per 1280x960 frame), so the index field is 25 bits wide here -- until
// round 4 it was 21 (tag 12), the width the ALIGNER's 32-bit word still has (kZIndexBits below).
constexpr unsigned kZTag0 = 0xFEu;
constexpr int kZ64IndexBits = 25, kZ64TagShift = 56;
constexpr int kMaxCloudPoints = 1 << kZ64IndexBits;      // 33 554 432 points per cloud
constexpr int kZIndexBits = 21;                           // index field of the aligner's 32-bit word (kZ32Tag0)
constexpr int kMaxAlignerPoints = 1 << kZIndexBits;       // 2 097 152: what a cloud handed to Aligner::align may hold
__host__ __device__ __forceinline__ unsigned long long zkey(unsigned tag, float d, int i) {
  return ((unsigned long long)tag << kZ64TagShift) | ((unsigned long long)(__builtin_bit_cast(unsigned, d) & 0x7fffffffu) << kZ64IndexBits) | (unsigned)i;
}
__host__ __device__ __forceinline__ int zkey_index(unsigned long long k, unsigned tag) {
  return ((unsigned)(k >> kZ64TagShift) == tag) ? (int)(k & ((1u << kZ64IndexBits) - 1u)) : -1;
}
__host__ __device__ __forceinline__ float zkey_depth(unsigned long long k, unsigned tag) {
  return ((unsigned)(k >> kZ64TagShift) == tag) ? __builtin_bit_cast(float, (unsigned)((k >> kZ64IndexBits) & 0x7fffffffu)) : FLT_MAX;
}

// Z-buffer of the ALIGNER (round 2): 32 bits per pixel = epoch tag (11 b) | point index (21 b), empty = ~0.  The depth is not stored:
// a pixel's first point under the current tag arrives by one atomicMin (a smaller tag beats whatever older projections left, like
// in the 64-bit form); only when two points of the SAME projection meet in a pixel -- a few per cent -- does the later one compare
// depths (it recomputes the other's from the cloud) and install the nearer one, ties to the lower index, with a compare-and-swap loop
// (project_point32).  Same winner as the reference's sequential `>` test (pinholepointprojector.cpp:61), half the atomic bytes (the
// projection runs at the memory-side atomic rate: tools/micro/zbuf_atomics.hip, 78 us against 122 us for the bare scatter), half the
// z-buffer bytes in the fused pass.  Depth images (matchClouds score, CorrespondenceFinder::*DepthImage()) are recomputed from the
// winning point with the projection's own matrix: the same expression, the same bits.
constexpr unsigned kZ32Tag0 = 0x7FEu;       // 0x7FF is the tag of the empty word
constexpr unsigned kZ32IndexMask = (1u << kZIndexBits) - 1u;
__host__ __device__ __forceinline__ unsigned z32key(unsigned tag, int i) { return (tag << kZIndexBits) | (unsigned)i; }
__host__ __device__ __forceinline__ int z32_index(unsigned w, unsigned tag) { return ((w >> kZIndexBits) == tag) ? (int)(w & kZ32IndexMask) : -1; }

constexpr int kClsMask = 3;      // class of the normal information matrix (0 zero, 1 flat, 2 non-flat) as a word in the old-format view (cloud_get)

struct CloudDev {
  float*  P3;        // [capacity][3] x y z
  float4* Nc;        // [capacity] (nx, ny, nz, curvature)
  float*  Om;        // [3][capacity][3]: row r of point i at (r * capacity + i) * 3 (om_at)
  float*  OmN;       // optional, same layout: full normal information matrices (uploaded clouds, scenes), else nullptr
  float*  St;        // optional [capacity][16] stats: U(9, column-major) eigenvalues(3) mean(3) n(1)
  int*    count;
  int     capacity;
  float   omN[2][9]; // class matrices (row-major 3x3): [0] flat, [1] non-flat
  float   clsThr;    // NormalInformationMatrixCalculator::_curvatureThreshold the cloud was converted with (informationmatrixcalculator.cpp:47-52)
  int     omSym;     // storage of Om: 0 = exact9 (three planes of 12-byte rows, all nine entries as computed), 1 = sym6 (two planes:
                     // (xx xy xz) and (yy yz zz), the upper triangle as computed; readers mirror it).  OmN is always nine entries.
};
// NormalInformationMatrixCalculator::compute (informationmatrixcalculator.cpp:38-58): zero normal -> zero matrix, else flat / non-flat by
// the curvature.  The converter decides on the normal before the sensor offset is applied; a rotation does not turn a non-zero normal
// into the zero vector, and a candidate with a zero normal is rejected before its class is looked at (correspondencefinder.cpp:69).
// information matrices (Om, OmN): entry k = 3 r + c of point i
__host__ __device__ __forceinline__ size_t om_at(size_t cap, size_t i, int k) { return ((size_t)(k / 3) * cap + i) * 3 + (size_t)(k % 3); }
// sym6 storage of the POINT information matrix (PWN_HIP_OMEGA_SYM6): U diag U^t is symmetric up to the rounding of its nine separately
// evaluated entries (informationmatrixcalculator.cpp:26-30), and SURVEY.md 8(d) counts it as 24 bytes.  Entry k = 3 r + c lives in slot
// sym_slot(k) of the six stored values (row-major upper triangle), i.e. at om_at(cap, i, sym_slot(k)): slots 0-2 are plane 0, 3-5 plane 1.
// Writers store the upper triangle only (om_is_lower entries are dropped), readers get the mirrored value.
__host__ __device__ constexpr int sym_slot(int k) { return k == 0 ? 0 : (k == 1 || k == 3) ? 1 : (k == 2 || k == 6) ? 2 : k == 4 ? 3 : (k == 5 || k == 7) ? 4 : 5; }
__host__ __device__ constexpr bool om_is_lower(int k) { return k == 3 || k == 6 || k == 7; }
__host__ __device__ __forceinline__ size_t omp_at(size_t cap, size_t i, int k, int sym) { return om_at(cap, i, sym ? sym_slot(k) : k); }
__host__ __device__ __forceinline__ int om_planes(int sym) { return sym ? 2 : 3; }
// The reference tests squaredNorm() > 0 (informationmatrixcalculator.cpp:46): a normal whose squares all underflow (components near 1e-30,
// which only an imported or a scene cloud can carry) is a zero normal.  The sum is formed as correspondence_test forms it.
__host__ __device__ __forceinline__ int normal_class(float nx, float ny, float nz, float curvature, float thr) {
  return (dot4seq(nx, nx, ny, ny, nz, nz, 0.f, 0.f) > 0.0f) ? ((curvature < thr) ? 1 : 2) : 0;
}

struct FrameDesc {
  const float* depth;        // float32 metres, or nullptr when `raw` is used
  const uint16_t* raw;       // optional uint16 source (DepthImage_convert_16UC1_to_32FC1 fused in: d = raw ? scale*raw : 0)
  float raw_scale;
  int* index;
  int* interval;
  float* integral;   // [10][rows*cols]
  int* rowoff;       // [rows] (stand-alone unProject) or [rows][strips] (converter fast path)
  unsigned long long* carry; // [strips][bands][160] strip-to-strip hand-over words of k_unproject_integral
  CloudDev cloud;
  int* count_out;    // optional: page-locked host word that receives the point count as well (single-frame calls: no gather kernel, no copy back)
};

struct ConvertParams {
  int rows, cols;
  Mat4 iKRt;
  float ivx, ivy;            // K*(R,R,0): pixels-per-metre of the world radius at unit depth
  float minD, maxD;
  int minRadius, maxRadius, minPoints;
  float statsCurvThr, pointInfoCurvThr, normalInfoCurvThr;
  float pFlat[3], pNonFlat[3];
  int hasOffset;
  Mat4 offset;               // sensor offset with last row forced
  int keepStats;
  int spinLimit;             // polls of a strip hand-over word before a waiting lane gives up and raises the fault flag (kSpinLimit)
  int dbgWithhold;           // test hook (pwn_hip_debug_withhold_carry): index of one hand-over word that is NOT written, -1 = none
  int omSym;                 // storage of the clouds' point information matrices (CloudDev::omSym): 1 = k_stats stores the upper triangle as two 12-byte rows
  int lean;                  // 1 = the front end (k_unproject_integral*) stores neither the points nor the interval image and k_stats recomputes
                             // both from the depth (the same expressions, the same bits): 20 bytes per pixel less written and 18 less read back
                             // kLeanGrouped (2) = lean, and the integral image of a slot is stored as three interleaved arrays (ig_at) instead of ten planes
};
constexpr int kLeanGrouped = 2;
// Grouped storage of the integral image (ConvertParams::lean == kLeanGrouped: the batch and tracker paths, where the image is a temporary between the
// front end and k_stats): the slot's 10 N floats hold three arrays [rows][cols] of records instead of ten planes [ch][rows][cols] --
//   group 0: (x, y, z, n)   group 1: (xx, xy, xz, yy)   group 2: (yz, zz)
// so channel k is component k % 4 of group k / 4, a producer stores one 16-byte (8-byte) record per pixel and group, and k_stats reads a
// window corner with three loads instead of ten.  Same bytes, same values.  A slot starts 8-byte aligned (40 N bytes per slot), and so
// does every group (16 N and 32 N bytes in): the record types carry alignment 8.
constexpr int kIG_Groups = 3;
__host__ __device__ constexpr int ig_width(int g) { return g < 2 ? 4 : 2; }
// float offset, inside a slot, of component 0 of pixel pix (= row * cols + col) in group g
__host__ __device__ __forceinline__ size_t ig_at(size_t N, int g, size_t pix) { return (size_t)4 * (size_t)g * N + pix * (size_t)ig_width(g); }

struct PairState {
  Mat4 T;          // Aligner::_T
  Mat4 invTcorr;   // _T.inverse() handed to CorrespondenceFinder::compute
  Mat4 invTcorrPrev; // the one of the last executed outer iteration (the finder's correspondences that _computeStatistics reuses)
  Mat4 invT;       // Linearizer::_T
  Mat4 KRt;        // projector matrix of the next reference projection
  Mat4 KRtLast;    // projector matrix of the reference projection executed last (its depth image is recomputed with it)
  Mat4 KRtCur;     // projector matrix of the current-cloud projection
  int   it;
  int   frozen;    // 1 = the pair met the context's convergence rule (StopRule) at the end of outer iteration `outer` - 1: every later launch of the
                   // call's loop returns for its workgroups, so this state and the pair's z-buffer words stay those of that iteration
  unsigned refTag; // z-buffer epoch of the reference projection executed last (what the readers after the loop take for a frozen pair)
  int   outer;     // outer iterations executed = entries of the two step traces
  float chi2[kMaxIter];
  int   inliers[kMaxIter];
  int   ncorr[kMaxIter];
  int   ncand[kMaxIter];
  float stepT[kMaxIter];   // per outer iteration: norm of the translation part of the last inner step dx, and of its rotation part as v2t reads it
  float stepR[kMaxIter];   // (pwn_hip.h: pwn_hip_align_steps)
};
// "Stop when converged" (pwn_hip_ctx_set_convergence): after outer iteration i (0-based) a pair freezes iff
// i + 1 >= minIterations && stepT[i] <= epsT && stepR[i] <= epsR (a NaN never passes).  enabled == 0: nobody freezes.
struct StopRule { int enabled; float epsT, epsR; int minIterations; };


struct PairDesc {
  CloudDev ref, cur;
  unsigned* zref;          // 32-bit z-buffers (tag | index), one word per pixel
  unsigned* zcur;
  int* curidx;             // index image of the current cloud (resolved once from zcur, or the converter's own image)
  const int* refidx0;      // optional: index image of the reference cloud for the FIRST outer iteration (the converter's own image when the
                           // initial guess is the identity: that projection returns it), else nullptr
  double* partials;        // [nblocks][kAccN]
  PairState* state;
  PairState* state_out;    // optional: page-locked host copy that k_solve_update keeps up to date in what the host reads back (T, it, the traces)
  int* fault;              // page-locked host word of the call: k_project stores 1 when a pixel's settle loop gave up (z32_settle)
  unsigned* zdepth;        // depth image of the two-pass projection (k_project_robust), nullptr unless the call runs in that mode
};

struct AlignParams {
  int rows, cols;
  Mat3 K;
  Mat4 refOffset;
  float minD, maxD;
  float sqDist, normalThr, flatThr, minRatio, maxRatio;
  float maxChi2;
  int robust;
  int settleGuard;         // rounds of z32_settle's compare-and-swap loop before a thread gives up (kSettleGuard)
  int mayFreeze;           // the call runs under an enabled StopRule: the loop's kernels look at the pairs' convergence flags.  0 (the default setting): nobody
                           // can freeze and no kernel of the loop loads a flag -- the launches are the ones of a library without the feature
};

// A depth source for the current side of a sub-batch's pairs (k_corr_linearize<..., CUR_DEPTH = true>): the one-call step aligns clouds it has
// just converted from frames that are still resident, and where a pair takes the current cloud's own index image (PairDesc::curidx = the
// converter's), candidate pixel pix with ci = curidx[pix] is the pixel point ci was unprojected from.  The fused pass then reads the pixel's
// 2-byte raw depth, coalesced, instead of gathering the 12-byte point, and evaluates the converter's own expression (converter_point: the bits
// k_stats stored).  raw[y] belongs to pair y of the launch, like pairs[y]; the other members are those of the step's conversions.  It sits next to
// the descriptors, not in them: PairDesc and AlignParams keep their layout, and every other kernel its code.
// STRIP_IDX: the index goes the same way.  The single-pass front end gave valid pixel (row, col) the index rowoff[row][col / 64] + (valid pixels of
// the strip to its left), with cols a multiple of 64 (unproject_integral_body), and a cloud keeps that table of strip offsets beside its index
// image.  A wave of the fused pass covers the 64 pixels of one (row, strip), entry pix >> 6 of the table, and holds their raw depths: one table
// word, the converter's range test and one ballot stand for the 4-byte-per-pixel index stream.
struct CurDepthSrc {
  const uint16_t* const* raw;   // per pair of the launch: the uint16 frame the current cloud was converted from (rows x cols, the aligner's size)
  float scale;                  // metres per raw unit
  Mat4 iKRt;                    // ConvertParams::iKRt
  int hasOffset; Mat4 offset;   // ConvertParams::hasOffset / offset
  const int* const* strips;     // per pair of the launch: the current cloud's strip offsets [rows][cols / 64]; nullptr: the launch reads the index images
  float minD, maxD;             // ConvertParams::minD / maxD: the range the converter counted a pixel valid in
};
struct NoCurDepthSrc {};        // what the other instantiations take in its place

// ------------------------------------------------------------------------------------------------------------------
// small device helpers
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// Butterfly sum of the 64 lanes in the order xor 1, 2, 4, 8, 16, 32 with DPP operands instead of ds_bpermute (no LDS crossbar, no
// lgkmcnt waits): after each step all lanes of a group hold the group's sum, so quad_perm / row_half_mirror / row_mirror bring
// "the other half's sum" exactly like an xor shuffle would, and row_bcast15 / row_bcast31 add the neighbouring rows' sums
// (a + b == b + a bitwise): the fixed tree ((..(l0+l1)+(l2+l3)..)) of a wave, so results stay bitwise reproducible.
// The total is valid in lane 63 only.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_sum_dpp_lane63(float v) {
  v += dpp_f32<0xB1, 0xF>(v);       // quad_perm [1,0,3,2]  (xor 1)
  v += dpp_f32<0x4E, 0xF>(v);       // quad_perm [2,3,0,1]  (xor 2)
  v += dpp_f32<0x141, 0xF>(v);      // row_half_mirror      (the other quad of the 8)
  v += dpp_f32<0x140, 0xF>(v);      // row_mirror           (the other 8 of the row)
  v += dpp_f32<0x142, 0xA>(v);      // row_bcast15 -> rows 1 and 3
  v += dpp_f32<0x143, 0xC>(v);      // row_bcast31 -> rows 2 and 3
  return v;
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// Pointers that reach a kernel inside a descriptor struct are generic to the compiler (flat_* instructions, 64-bit VALU address
// arithmetic, and flat traffic ties the LDS counter to the vector-memory one).  They all point to hipMalloc'ed memory: as_global()
// says so, which gives global_* instructions with a scalar base + 32-bit lane offset.
template <typename T> using gptr = T __attribute__((address_space(1)))*;
template <typename T> __device__ __forceinline__ gptr<T> as_global(T* p) { return (gptr<T>)(uintptr_t)p; }
// a pair's convergence flag (workgroup-uniform: every thread reads the same word)
__device__ __forceinline__ int pair_frozen(const PairState* st) { return *as_global(&st->frozen); }
// The epoch of a pair's last reference projection for the readers after the loop: the launch's, or a frozen pair's own older one
__device__ __forceinline__ unsigned pair_ref_tag(const PairState* st, unsigned launchTag) { return pair_frozen(st) ? *as_global(&st->refTag) : launchTag; }
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load4(gptr<const v4f> p) { const v4f v = *p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void store4(gptr<v4f> p, const float4 v) { v4f t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w; *p = t; }
// three packed floats: a clang ext_vector_type(3) has sizeof = alignof = 16, but the xyz records and the information-matrix rows sit at
// 12-byte strides -- the access type therefore carries alignment 4 (still one global_load/store_dwordx3; an `align 16` access at a 4-byte
// aligned address would be undefined behaviour and licenses the compiler to widen it to 16 bytes, over the next record;
// tests/test_capi_cpu.py disassembles the library and checks that k_stats / k_unproject_integral contain no dwordx4 store)
typedef float v3f_raw __attribute__((ext_vector_type(3)));
typedef v3f_raw v3f __attribute__((aligned(4)));
// records of the grouped integral image (ig_at): 16 and 8 bytes at 8-byte aligned addresses
typedef v4f ig4 __attribute__((aligned(8)));
typedef float ig2 __attribute__((ext_vector_type(2)));
// point i of a packed xyz array as (x, y, z, 0): one 12-byte load
__device__ __forceinline__ float4 load_xyz(gptr<const float> p3, unsigned i) { const v3f_raw v = *(gptr<const v3f>)(p3 + 3u * i); return make_float4(v.x, v.y, v.z, 0.f); }
__device__ __forceinline__ float4 load_xyz(const float* p3, int i) { return load_xyz(as_global(p3), (unsigned)i); }
__device__ __forceinline__ void store_xyz(float* p3, int i, float x, float y, float z) { v3f_raw v; v.x = x; v.y = y; v.z = z; *(gptr<v3f>)(as_global(p3) + 3u * (unsigned)i) = v; }
// Old-format view of point i for the code that is not hot (scene stage, stand-alone stages): P = (x, y, z, curvature),
// Nm = (nx, ny, nz, class word); cloud_put stores the same view back (the class word is derived data and is dropped).
__device__ __forceinline__ void cloud_get(const CloudDev& c, int i, float4& P, float4& Nm) {
  P = load_xyz(c.P3, i);
  const float4 nc = c.Nc[i];
  P.w = nc.w;
  Nm = make_float4(nc.x, nc.y, nc.z, __int_as_float(normal_class(nc.x, nc.y, nc.z, nc.w, c.clsThr)));
}
__device__ __forceinline__ void cloud_put(const CloudDev& c, int i, const float4 P, const float4 Nm) {
  store_xyz(c.P3, i, P.x, P.y, P.z);
  c.Nc[i] = make_float4(Nm.x, Nm.y, Nm.z, P.w);
}
// force a wave-uniform value into a scalar register
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ Mat4 uniform_iso(const Mat4& T) {
  Mat4 r;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r(0,c) = uniform(T(0,c)); r(1,c) = uniform(T(1,c)); r(2,c) = uniform(T(2,c));
  }
  r(3,0) = 0.f; r(3,1) = 0.f; r(3,2) = 0.f; r(3,3) = 1.f;
  return r;
}

__device__ __forceinline__ Mat4 uniform_iso_global(gptr<const float> m) {      // column-major 4x4 in global memory -> SGPRs
  Mat4 r;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r(0,c) = uniform(m[4 * c]); r(1,c) = uniform(m[4 * c + 1]); r(2,c) = uniform(m[4 * c + 2]);
  }
  r(3,0) = 0.f; r(3,1) = 0.f; r(3,2) = 0.f; r(3,3) = 1.f;
  return r;
}

// ------------------------------------------------------------------------------------------------------------------
// DepthImage_convert_16UC1_to_32FC1 (pwn_core/pwn_static.cpp:54-68).  grid.y = frame
struct RawDesc { const uint16_t* src; float* dst; };
__global__ void k_u16_to_f32(const RawDesc* __restrict__ d, int n, float scale) {
  const RawDesc rd = d[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    rd.dst[i] = raw_to_metres(rd.src[i], scale);
  }
}
// DepthImage_convert_32FC1_to_16UC1 (pwn_core/pwn_static.cpp:38-52)
__global__ void k_f32_to_u16(const float* __restrict__ src, uint16_t* __restrict__ dst, int n, float scale) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float f = src[i];
    dst[i] = (f < FLT_MAX) ? (uint16_t)(scale * f) : (uint16_t)0;
  }
}
// DepthImage_scale (pwn_core/pwn_static.cpp:5-36), the arithmetic of one destination pixel, stated once: the sums over its step x step block
// in the loop's order (block row outer, block column inner); every pixel enters the sums, the positive ones are counted; the pixel is the
// mean unless nothing was counted or the variance exceeds maxCov
struct BoxAcc {
  float acc = 0.f, acc2 = 0.f; int np = 0;
  __device__ __forceinline__ void add(float f) { acc += f; acc2 += f * f; np += f > 0; }
  __device__ __forceinline__ float pixel(float maxCov) const {
    if (!np) return 0.f;
    const float mu = acc / np;
    const float sigma = acc2 / np - mu * mu;
    return (sigma > maxCov) ? 0.f : mu;
  }
};
// a source pixel in metres: float frames as they are, raw uint16 as DepthImage_convert_16UC1_to_32FC1 makes them (pwn_static.cpp:54-68)
__device__ __forceinline__ float metres_of(float v, float) { return v; }
__device__ __forceinline__ float metres_of(uint16_t v, float scale) { return raw_to_metres(v, scale); }
// the destination pixel whose block starts at p (rows `pitch` elements apart)
template <typename SRC> __device__ __forceinline__ float box_pixel(gptr<const SRC> p, int pitch, int step, float rawScale, float maxCov) {
  BoxAcc s;
  for (int a = 0; a < step; ++a)
    for (int b = 0; b < step; ++b) s.add(metres_of(p[(size_t)a * pitch + b], rawScale));
  return s.pixel(maxCov);
}
// one frame, one thread per destination pixel (pwn_hip_depth_scale, pwn_hip_convert_scaled)
__global__ void k_depth_scale(const float* __restrict__ src, int srows, int scols, int step, float maxCov, float* __restrict__ dst) {
  const int rows = srows / step, cols = scols / step;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i % cols;
  dst[i] = box_pixel(as_global(src) + ((size_t)r * step * scols + (size_t)c * step), scols, step, 0.f, maxCov);
}
// DepthImage_scale of the frames of a sub-batch in one launch (grid.y = frame), float or raw uint16 source.  The kernel only streams -- 2 or 4
// bytes in per source pixel, 4 / step^2 out -- so a lane owns DPL adjacent destination pixels and reads one 16-byte word per source row of
// their blocks: uint16 step 2: 4 pixels, uint16 step 4: 2, float step 2: 2.  Every destination pixel keeps sums of its own, filled in the
// reference's order.  Needs frames and source rows that start 16-byte aligned; the last lane of a destination row takes the pixels that do
// not fill a word with box_pixel.  Source rows and columns past rows * STEP, cols * STEP are not read.
// grid = (ceil(rows * ceil(cols / DPL) / 256), frames), block = 256
struct ScaleDesc { const void* src; float* dst; };
__device__ __forceinline__ void unpack_word(const v4u w, float (&f)[8], float scale) {
  const unsigned u[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[2 * k] = raw_to_metres(u[k] & 0xFFFFu, scale); f[2 * k + 1] = raw_to_metres(u[k] >> 16, scale); }
}
__device__ __forceinline__ void unpack_word(const v4u w, float (&f)[4], float) {
  f[0] = __uint_as_float(w.x); f[1] = __uint_as_float(w.y); f[2] = __uint_as_float(w.z); f[3] = __uint_as_float(w.w);
}
template <typename SRC, int STEP>
__global__ void __launch_bounds__(256) k_depth_scale_batch(const ScaleDesc* __restrict__ frames, int srows, int scols, float rawScale, float maxCov) {
  constexpr int PX = 16 / (int)sizeof(SRC);            // source pixels per 16-byte word
  constexpr int DPL = PX / STEP;                       // destination pixels per lane
  static_assert(DPL >= 1 && DPL * STEP == PX, "a word holds whole blocks");
  const ScaleDesc sd = frames[blockIdx.y];
  const int rows = srows / STEP, cols = scols / STEP;
  const int full = cols / DPL, slots = (cols + DPL - 1) / DPL;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)rows * (unsigned)slots) return;
  const int r = (int)(t / (unsigned)slots), s = (int)(t % (unsigned)slots);
  const gptr<const SRC> src = as_global((const SRC*)sd.src) + ((size_t)r * STEP * scols + (size_t)s * PX);
  const gptr<float> dst = as_global(sd.dst) + ((size_t)r * cols + (size_t)s * DPL);
  if (s < full) {
    v4u w[STEP];
#pragma unroll
    for (int a = 0; a < STEP; ++a) w[a] = *(gptr<const v4u>)(src + (size_t)a * scols);
    BoxAcc acc[DPL];
#pragma unroll
    for (int a = 0; a < STEP; ++a) {
      float f[PX];
      unpack_word(w[a], f, rawScale);
#pragma unroll
      for (int j = 0; j < DPL; ++j)
#pragma unroll
        for (int b = 0; b < STEP; ++b) acc[j].add(f[j * STEP + b]);
    }
#pragma unroll
    for (int j = 0; j < DPL; ++j) dst[j] = acc[j].pixel(maxCov);
  } else {
    for (int j = 0; j < cols - full * DPL; ++j) dst[j] = box_pixel(src + j * STEP, scols, STEP, rawScale, maxCov);
  }
}
// any step, any alignment: one thread per destination pixel.  grid = (ceil(rows * cols / 256), frames), block = 256
template <typename SRC>
__global__ void __launch_bounds__(256) k_depth_scale_batch_any(const ScaleDesc* __restrict__ frames, int srows, int scols, int step, float rawScale, float maxCov) {
  const ScaleDesc sd = frames[blockIdx.y];
  const int rows = srows / step, cols = scols / step;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)rows * (unsigned)cols) return;
  const int r = (int)(i / (unsigned)cols), c = (int)(i % (unsigned)cols);
  as_global(sd.dst)[i] = box_pixel(as_global((const SRC*)sd.src) + ((size_t)r * step * scols + (size_t)c * step), scols, step, rawScale, maxCov);
}

// valid pixels (the range test of PinholePointProjector::_unProject, pinholepointprojector.h:246-248) of each frame's down-sampled image: the
// points a conversion of it will ask of its cloud.  out[frame] starts at 0.  grid = (<= 1024, frames), block = 256
__global__ void __launch_bounds__(256) k_count_in_range(const ScaleDesc* __restrict__ frames, int n, float minD, float maxD, int* __restrict__ out) {
  const gptr<const float> d = as_global((const float*)frames[blockIdx.y].dst);
  int cnt = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) cnt += depth_in_range(d[i], minD, maxD);
  const int t = (int)wave_sum((float)cnt);      // small integers: exact in fp32
  if (lane_id() == 0 && t) atomicAdd(out + blockIdx.y, t);
}
// depth of pixel i of a frame: the float image, or the raw uint16 image converted on the fly
__device__ __forceinline__ float frame_depth(const FrameDesc& f, size_t i) {
  if (f.raw) return raw_to_metres(f.raw[i], f.raw_scale);
  return f.depth[i];
}
// ------------------------------------------------------------------------------------------------------------------
// Ordered compaction, step 1: valid pixels per image row.  grid = (rows, frames), block = 256.
// validity test = PinholePointProjector::_unProject (pwn_core/pinholepointprojector.h:246-248)
__global__ void __launch_bounds__(256) k_row_count(const FrameDesc* __restrict__ frames, ConvertParams cp) {
  const FrameDesc& f = frames[blockIdx.y];
  const int r = blockIdx.x;
  int cnt = 0;
  for (int c = threadIdx.x; c < cp.cols; c += 256) {
    const float d = frame_depth(f, (size_t)r * cp.cols + c);
    cnt += depth_in_range(d, cp.minD, cp.maxD);
  }
  __shared__ int s[4];
  float t = wave_sum((float)cnt);           // <= 64*N small ints: exact in fp32
  if (lane_id() == 0) s[threadIdx.x >> 6] = (int)t;
  __syncthreads();
  if (threadIdx.x == 0) f.rowoff[r] = s[0] + s[1] + s[2] + s[3];
}
// step 2: exclusive scan of the row counts (in place) + total.  grid = frames, block = 1024
__global__ void __launch_bounds__(1024) k_row_offsets(const FrameDesc* __restrict__ frames, int rows) {
  const FrameDesc& f = frames[blockIdx.x];
  __shared__ int s[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < rows; base += 1024) {
    const int r = base + threadIdx.x;
    const int v = (r < rows) ? f.rowoff[r] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int add = (threadIdx.x >= off) ? s[threadIdx.x - off] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    const int incl = s[threadIdx.x];
    const int c0 = carry;
    if (r < rows) f.rowoff[r] = c0 + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c0 + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) { *f.cloud.count = carry; if (f.count_out) *f.count_out = carry; }
}
// per-frame point counts -> one contiguous array (single D2H copy per batch)
__global__ void k_gather_counts(const FrameDesc* __restrict__ frames, int n, int* __restrict__ out, const int* __restrict__ fault) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = *frames[i].cloud.count;
  if (i == n) out[n] = *fault;      // time-out flag of k_unproject_integral rides along with the counts
}
// Ordered compaction of one 256-pixel step of an image row, block = 256: the point index of this thread's pixel = base + valid pixels
// left of it in the step (meaningful when `valid`); tot = the step's valid pixels.  wcount: the block's 4 per-wave counts, free again after
// the caller's next __syncthreads().
__device__ __forceinline__ int row_compact(bool valid, int (&wcount)[4], int wave, int lane, int base, int& tot) {
  const unsigned long long bal = __ballot(valid);
  const int rank = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcount[wave] = __popcll(bal);
  __syncthreads();
  int woff = 0;
  tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { const int n = wcount[w]; if (w < wave) woff += n; tot += n; }
  return base + woff + rank;
}
// step 3: PinholePointProjector::unProject (pwn_core/pinholepointprojector.cpp:93-133) + projectIntervals (:135-147).
// Point index = row-major rank of the valid pixel.  grid = (rows, frames), block = 256.
__global__ void __launch_bounds__(256) k_unproject(const FrameDesc* __restrict__ frames, ConvertParams cp) {
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
    const int slot = row_compact(valid, wcount, wave, lane, base, tot);
    if (in) {
      const size_t pix = (size_t)r * cp.cols + c;
      int idx = -1, itv = -1;
      if (valid) {
        idx = slot;
        const Vec3 p = unproject_pixel(cp.iKRt, c, r, d);
        if (f.cloud.P3 && idx < f.cloud.capacity) store_xyz(f.cloud.P3, idx, p.x, p.y, p.z);
        itv = depth_interval(cp.ivx, cp.ivy, d);
      }
      f.index[pix] = idx;
      f.interval[pix] = itv;
    }
    base += tot;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// PointIntegralImage::compute, passes 1+2 (pwn_core/pointintegralimage.cpp:16-35): scatter the points into the
// accumulators and prefix-sum along image x inside each image row.  fp32 addition is not associative and
// the covariance downstream differences these sums, so every chain keeps the reference's strictly sequential
// left-to-right order: one thread per (row, channel) chain, tiles staged through LDS so that all global
// traffic is row-coalesced.  grid = (ceil(rows/16), frames), block = 256.
// band height of the integral-image kernels (a multiple of 4: one row per compute wave and step); measured on MI355X: the hand-over
// wavefront of the strip kernel fills and drains in half the time with 8-row bands: -7 % against 16
constexpr int kIR_Rows = 8, kIR_Cols = 64, kIR_Stride = kIR_Cols + 1;
static_assert(kIR_Rows % 4 == 0 && (kIR_Rows & (kIR_Rows - 1)) == 0 && kIR_Rows <= 64, "band height");
// the ten integral-image channel values of a point (PointAccumulator::operator+=(Point), pointaccumulator.h:56-59): p, 1, the upper triangle of p p^T
__device__ __forceinline__ void point_channels(float (&v)[kIntegralChannels], float x, float y, float z) {
  v[0] = x; v[1] = y; v[2] = z; v[3] = 1.0f;
  v[4] = x * x; v[5] = x * y; v[6] = x * z;
  v[7] = y * y; v[8] = y * z; v[9] = z * z;
}
__global__ void __launch_bounds__(256) k_integral_rows(const FrameDesc* __restrict__ frames, int rows, int cols) {
  const FrameDesc& f = frames[blockIdx.y];
  const int r0 = blockIdx.x * kIR_Rows;
  __shared__ float tile[kIntegralChannels * kIR_Rows * kIR_Stride];   // 41.6 KB
  const int tid = threadIdx.x;
  const size_t N = (size_t)rows * cols;
  // scan role: thread t < 160 owns chain (row = t % 16, ch = t / 16)
  const int srow = tid % kIR_Rows, sch = tid / kIR_Rows;
  float carry = 0.f;
  for (int x0 = 0; x0 < cols; x0 += kIR_Cols) {
    // phase 1: 1024 pixels, 4 per thread, lanes along x
#pragma unroll
    for (int j = 0; j < kIR_Rows / 4; ++j) {
      const int q = tid + 256 * j;
      const int lr = q / kIR_Cols, lc = q % kIR_Cols;
      const int r = r0 + lr, c = x0 + lc;
      float v[kIntegralChannels];
#pragma unroll
      for (int k = 0; k < kIntegralChannels; ++k) v[k] = 0.f;
      if (r < rows && c < cols) {
        const int idx = f.index[(size_t)r * cols + c];
        if (idx >= 0 && idx < f.cloud.capacity) {
          const float4 p = load_xyz(f.cloud.P3, idx);
          point_channels(v, p.x, p.y, p.z);
        }
      }
#pragma unroll
      for (int k = 0; k < kIntegralChannels; ++k) tile[(k * kIR_Rows + lr) * kIR_Stride + lc] = v[k];
    }
    __syncthreads();
    // phase 2: sequential scan of 64 columns per chain
    if (tid < kIntegralChannels * kIR_Rows) {
      float* t = &tile[(sch * kIR_Rows + srow) * kIR_Stride];
      float vals[kIR_Cols];
#pragma unroll
      for (int c = 0; c < kIR_Cols; ++c) vals[c] = t[c];
#pragma unroll
      for (int c = 0; c < kIR_Cols; ++c) { carry = vals[c] + carry; vals[c] = carry; }
#pragma unroll
      for (int c = 0; c < kIR_Cols; ++c) t[c] = vals[c];
    }
    __syncthreads();
    // phase 3: coalesced write-back, plane by plane
#pragma unroll
    for (int j = 0; j < kIR_Rows / 4; ++j) {
      const int q = tid + 256 * j;
      const int lr = q / kIR_Cols, lc = q % kIR_Cols;
      const int r = r0 + lr, c = x0 + lc;
      if (r < rows && c < cols) {
#pragma unroll
        for (int k = 0; k < kIntegralChannels; ++k)
          f.integral[k * N + (size_t)r * cols + c] = tile[(k * kIR_Rows + lr) * kIR_Stride + lc];
      }
    }
    __syncthreads();
  }
}
// Converter latency path (a few frames: tracker, makeCloud): unProject + projectIntervals fused into the row scan.  Depth is read once;
// the kernel writes the points, the index and interval images AND the row-prefixed integral planes (k_integral_cols finishes them).
// One workgroup per 16-row x 64-column tile, so a VGA frame is 300 workgroups instead of 30 walking ten tiles each: unprojecting and
// storing a tile does not depend on its left neighbour, only the 160 (channel, row) chains do -- they continue from the neighbour's
// carry, handed over as in k_unproject_integral (one 64-bit word per chain = launch epoch << 32 | float bits, written once per launch;
// a tile waits only for a lower-numbered workgroup; bounded poll that raises *fault instead of hanging).  All tiles of a band sit on
// one XCD (workgroup ids are dealt round-robin over the 8 XCDs), so the hand-over words stay in that XCD's L2.  Wave w owns rows
// r0 + w + 4j (j = 0..3): one wave instruction covers the 64 columns of one row, the point index of a valid pixel = row offset +
// valid pixels of the row left of the tile (counted here) + popcount(ballot below the lane).
// grid = (8 * ceil(bands/8) * strips, frames), block = 256.
constexpr int kII_Chains = kIntegralChannels * kIR_Rows;     // 160 (channel, row) chains of a band
__global__ void __launch_bounds__(256) k_unproject_integral_rows(const FrameDesc* __restrict__ frames, ConvertParams cp, unsigned epoch, int* __restrict__ fault) {
  const FrameDesc& f = frames[blockIdx.y];
  const int rows = cp.rows, cols = cp.cols;
  const int S = (cols + kIR_Cols - 1) / kIR_Cols, NB = (rows + kIR_Rows - 1) / kIR_Rows;
  const unsigned kk = blockIdx.x >> 3;
  const int band = 8 * (int)(kk / (unsigned)S) + (int)(blockIdx.x & 7u), s = (int)(kk % (unsigned)S);
  if (band >= NB) return;
  const int r0 = band * kIR_Rows, x0 = s * kIR_Cols;
  __shared__ float tile[kIntegralChannels * kIR_Rows * kIR_Stride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t N = (size_t)rows * cols;
  // 1. unproject the tile
#pragma unroll
  for (int j = 0; j < kIR_Rows / 4; ++j) {
    const int lr = wave + 4 * j, lc = lane;
    const int r = r0 + lr, c = x0 + lc;
    const bool in = r < rows && c < cols;
    int base = 0;
    if (r < rows) {                                           // wave-uniform
      base = f.rowoff[r];
      for (int t = 0; t < s; ++t) {                           // full strips left of this one
        const float dl = frame_depth(f, (size_t)r * cols + t * kIR_Cols + lane);
        base += __popcll(__ballot(depth_in_range(dl, cp.minD, cp.maxD)));
      }
    }
    const float d = in ? frame_depth(f, (size_t)r * cols + c) : 0.f;
    const bool valid = in && depth_in_range(d, cp.minD, cp.maxD);
    const unsigned long long bal = __ballot(valid);
    float v[kIntegralChannels];
#pragma unroll
    for (int k = 0; k < kIntegralChannels; ++k) v[k] = 0.f;
    if (in) {
      int idx = -1, itv = -1;
      if (valid) {
        idx = base + __popcll(bal & ((1ull << lane) - 1ull));
        const Vec3 p = unproject_pixel(cp.iKRt, c, r, d);
        if (idx < f.cloud.capacity) {
          if (!cp.lean) store_xyz(f.cloud.P3, idx, p.x, p.y, p.z);
          point_channels(v, p.x, p.y, p.z);
        }
        if (!cp.lean) itv = depth_interval(cp.ivx, cp.ivy, d);
      }
      f.index[(size_t)r * cols + c] = idx;
      if (!cp.lean) f.interval[(size_t)r * cols + c] = itv;
    }
#pragma unroll
    for (int k = 0; k < kIntegralChannels; ++k) tile[(k * kIR_Rows + lr) * kIR_Stride + lc] = v[k];
  }
  __syncthreads();
  // 2. the 160 (channel, row) chains of the tile, continued from the tile to the left
  if (tid < kII_Chains) {
    float carry = 0.f;
    if (s > 0) {
      const unsigned long long* src = f.carry + ((size_t)(s - 1) * NB + band) * kII_Chains + tid;
      unsigned long long w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int spins = 0;
      while ((unsigned)(w >> 32) != epoch) {
        if (++spins >= cp.spinLimit) { atomicOr(fault, 1); break; }    // a starved chain finishes with garbage instead of hanging the device
        __builtin_amdgcn_s_sleep(1);
        w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      carry = __uint_as_float((unsigned)w);
    }
    const int srow = tid % kIR_Rows, sch = tid / kIR_Rows;
    float* t = &tile[(sch * kIR_Rows + srow) * kIR_Stride];
#pragma unroll 1
    for (int c0 = 0; c0 < kIR_Cols; c0 += 16) {          // 16 LDS reads in flight, then the sequential adds
      float vals[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) vals[c] = t[c0 + c];
#pragma unroll
      for (int c = 0; c < 16; ++c) { carry = vals[c] + carry; vals[c] = carry; }
#pragma unroll
      for (int c = 0; c < 16; ++c) t[c0 + c] = vals[c];
    }
    if (s + 1 < S && (s * NB + band) * kII_Chains + tid != cp.dbgWithhold)
      __hip_atomic_store(f.carry + ((size_t)s * NB + band) * kII_Chains + tid,
                         ((unsigned long long)epoch << 32) | (unsigned long long)__float_as_uint(carry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  // 3. the row-prefixed planes
  if (cp.lean == kLeanGrouped) {
    // grouped storage: the tile's 64 columns of a row are 64 * width consecutive floats of a group (column, component): lanes along them
    for (int g = 0; g < kIG_Groups; ++g) {
      const int w = ig_width(g), rowlen = kIR_Cols * w;
      for (int j = tid; j < kIR_Rows * rowlen; j += 256) {
        const int lr = j / rowlen, e = j % rowlen;
        const int lc = e / w, k = e % w;
        const int r = r0 + lr, c = x0 + lc;
        if (r < rows && c < cols) f.integral[ig_at(N, g, (size_t)r * cols + c) + k] = tile[((4 * g + k) * kIR_Rows + lr) * kIR_Stride + lc];
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kIR_Rows / 4; ++j) {
    const int lr = wave + 4 * j, lc = lane;
    const int r = r0 + lr, c = x0 + lc;
    if (r < rows && c < cols) {
#pragma unroll
      for (int k = 0; k < kIntegralChannels; ++k)
        f.integral[k * N + (size_t)r * cols + c] = tile[(k * kIR_Rows + lr) * kIR_Stride + lc];
    }
  }
}
// ------------------------------------------------------------------------------------------------------------------
// Converter fast path, single pass: unProject + projectIntervals + PointIntegralImage::compute (all three passes of
// pwn_core/pointintegralimage.cpp:16-43) with ONE write of the integral planes and no read of them.
//
// A workgroup owns one 64-column strip of one frame and walks it top to bottom in bands of 16 rows.  Per band:
//   1. unproject the 16x64 pixels (as k_unproject; the point index comes from per-(row, strip) offsets, k_strip_count),
//      10 channel values per pixel into LDS;
//   2. x pass: 160 threads own the (channel, row) chains, continue them from the carry of the strip to the LEFT and hand the
//      carry on to the strip to the right;
//   3. y pass: 640 (channel, column) chains whose running sums live in registers from band to band; coalesced store.
// Every chain is the reference's strictly sequential fp32 sum, so the planes are bit-identical to the three-kernel path.
//
// The strip-to-strip hand-over is one 64-bit word per (strip, band, chain) = launch epoch << 32 | float bits: value and
// "ready" flag travel in the same single-copy-atomic store, so no fence is needed; a word is written once per launch (no
// slot reuse inside a launch, hence no back-pressure), stale words carry an older epoch.  Forward progress: strip s waits
// only for strip s-1 of the same frame, which has a smaller workgroup id and is therefore dispatched before it; the poll is
// bounded (kSpinLimit), a starved chain raises *fault and finishes with garbage instead of hanging the device.
// Workgroup -> (frame, strip) puts all strips of a frame on one XCD (ids are dealt round-robin over the 8 XCDs), so the
// hand-over words stay in that XCD's L2.  grid = 8 * ceil(frames/8) * strips, block = 256.
constexpr int kSpinLimit = 1 << 20;      // polls of >= 64 cycles + one L2 round trip each: ~1 s, against hand-over waits of microseconds
__host__ __device__ __forceinline__ int strips_of(int cols) { return (cols + kIR_Cols - 1) / kIR_Cols; }
__host__ __device__ __forceinline__ int bands_of(int rows) { return (rows + kIR_Rows - 1) / kIR_Rows; }

// valid pixels per (row, 64-column strip); k_row_offsets over rows*strips entries turns them into point-index offsets.
// One wave per image row, 16 bytes per lane and load (8 uint16 or 4 float pixels), so a 640-pixel row is two (five) wave loads instead
// of ten dependent 128-byte ones; the per-lane counts are summed over the 8 (16) lanes of a strip with xor shuffles (small integers:
// exact).  Needs rows that start 16-byte aligned (cols % 8 == 0 resp. cols % 4 == 0), else k_strip_count_any.
// grid = (ceil(rows / 4), frames), block = 256
template <bool RAW>
__global__ void __launch_bounds__(256) k_strip_count(const FrameDesc* __restrict__ frames, ConvertParams cp) {
  const FrameDesc& f = frames[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int r = blockIdx.x * 4 + wave, S = strips_of(cp.cols);
  if (r >= cp.rows) return;
  constexpr int PX = RAW ? 8 : 4;                      // pixels per lane and load
  constexpr int LPS = kIR_Cols / PX;                   // lanes per strip
  const float scale = f.raw_scale;
  for (int c0 = 0; c0 < cp.cols; c0 += 64 * PX) {
    const int c = c0 + lane * PX;
    int cnt = 0;
    if (c < cp.cols) {                                 // cols % PX == 0: a lane's pixels are all inside or all outside the row
      float d[PX];
      if (RAW) {
        const v4u w = *(gptr<const v4u>)(as_global(f.raw) + ((size_t)r * cp.cols + c));
        const unsigned u[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned lo = u[k] & 0xFFFFu, hi = u[k] >> 16;
          d[2 * k] = raw_to_metres(lo, scale); d[2 * k + 1] = raw_to_metres(hi, scale);
        }
      } else {
        const v4f w = *(gptr<const v4f>)(as_global(f.depth) + ((size_t)r * cp.cols + c));
        d[0] = w.x; d[1] = w.y; d[2] = w.z; d[3] = w.w;
      }
#pragma unroll
      for (int k = 0; k < PX; ++k) cnt += depth_in_range(d[k], cp.minD, cp.maxD);
    }
#pragma unroll
    for (int off = 1; off < LPS; off <<= 1) cnt += __shfl_xor(cnt, off, 64);
    const int s = c / kIR_Cols;
    if ((lane & (LPS - 1)) == 0 && c < cp.cols) f.rowoff[r * S + s] = cnt;
  }
}
// any width / alignment.  grid = (rows, frames), block = 256
__global__ void __launch_bounds__(256) k_strip_count_any(const FrameDesc* __restrict__ frames, ConvertParams cp) {
  const FrameDesc& f = frames[blockIdx.y];
  const int r = blockIdx.x, S = strips_of(cp.cols);
  const int wave = threadIdx.x >> 6, lane = lane_id();
  for (int s = wave; s < S; s += 4) {
    const int c = s * kIR_Cols + lane;
    const float d = (c < cp.cols) ? frame_depth(f, (size_t)r * cp.cols + c) : 0.f;
    const bool valid = c < cp.cols && depth_in_range(d, cp.minD, cp.maxD);
    const unsigned long long bal = __ballot(valid);
    if (lane == 0) f.rowoff[r * S + s] = __popcll(bal);
  }
}

// workgroup barrier that orders LDS traffic only: global stores stay in flight across it (a __syncthreads() would drain them)
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// Block = 4 compute waves + 1 loader wave.  gfx950 counts vector loads and stores in ONE in-order counter (vmcnt), so a wave that
// waits for a load also waits for every store it issued before it; the compute waves issue ~60 KB of stores per band and must not
// wait for memory at all.  The loader wave therefore does every global read of the block (depth and strip offsets of the NEXT
// band, hand-over words of the current one) and passes the values on through LDS; it never stores to global memory.
// Plane, index and interval stores are non-temporal (measured: strip kernel -5 %, k_stats after it -4 %).
constexpr int kII_Threads = 320;
// y pass of one group of the grouped integral image: the thread owns column `lane` of the strip and the W chains of the group's channels
// ch0 .. ch0 + W - 1, continues them over the band's rows and stores one W-float record per row (a wave store covers 64 W floats in a row).
// Rows go in batches of kIG_RowBatch: W * kIG_RowBatch values in registers at a time.
constexpr int kIG_RowBatch = 4;
static_assert(kIR_Rows % kIG_RowBatch == 0, "row batch");
template <int W>
__device__ __forceinline__ void ypass_group(const float* tile, const int ch0, const int lane, float (&vc)[4], const bool incol, const gptr<float> dst,
                                            const unsigned rowFloats, const int r0, const int rows) {
#pragma unroll
  for (int rb = 0; rb < kIR_Rows; rb += kIG_RowBatch) {
    float vals[kIG_RowBatch][W];
#pragma unroll
    for (int r = 0; r < kIG_RowBatch; ++r)
#pragma unroll
      for (int k = 0; k < W; ++k) vals[r][k] = tile[((ch0 + k) * kIR_Rows + rb + r) * kIR_Stride + lane];
#pragma unroll
    for (int r = 0; r < kIG_RowBatch; ++r)
#pragma unroll
      for (int k = 0; k < W; ++k) { vc[k] = vals[r][k] + vc[k]; vals[r][k] = vc[k]; }
    if (incol) {
#pragma unroll
      for (int r = 0; r < kIG_RowBatch; ++r) if (r0 + rb + r < rows) {
        const gptr<float> q = dst + (unsigned)(rb + r) * rowFloats;
        if (W == 4) { v4f v; v.x = vals[r][0]; v.y = vals[r][1]; v.z = vals[r][2]; v.w = vals[r][3]; __builtin_nontemporal_store(v, (gptr<ig4>)q); }
        else { ig2 v; v.x = vals[r][0]; v.y = vals[r][W - 1]; __builtin_nontemporal_store(v, (gptr<ig2>)q); }
      }
    }
  }
}
// Body of the single-pass front end for strip s of frame f.  GROUPED = false: planes [10][rows][cols] (lean or not, cp.lean); GROUPED = true:
// the lean front end with the grouped integral image (ig_at), the form k_stats reads back in the batch and tracker paths.
template <bool GROUPED>
__device__ __forceinline__ void unproject_integral_body(const FrameDesc& f, const ConvertParams& cp, const int s, const unsigned epoch, int* __restrict__ fault) {
  const int rows = cp.rows, cols = cp.cols;
  const int S = strips_of(cols), NB = bands_of(rows);
  __shared__ float tile[kIntegralChannels * kIR_Rows * kIR_Stride];
  __shared__ float stage[2][kIR_Rows * kIR_Cols];     // depth of the band (metres; 0 outside the image), double-buffered
  __shared__ int sbase[2][kIR_Rows];                  // point-index offset of (row, strip)
  __shared__ float cin[kII_Chains];                   // x-pass carries handed over by the strip to the left
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the role branches below are wave-uniform
  const size_t N = (size_t)rows * cols;
  const int x0 = s * kIR_Cols, c = x0 + lane;
  const bool loader = wave == 4;
  const bool chain = tid < kII_Chains;
  const gptr<const float> gdepth = as_global(f.depth);
  const gptr<const uint16_t> graw = as_global(f.raw);
  const bool is_raw = f.raw != nullptr;
  const float raw_scale = f.raw_scale;
  const gptr<const int> growoff = as_global((const int*)f.rowoff);
  const gptr<int> gindex = as_global(f.index), ginterval = as_global(f.interval);
  const gptr<float> gintegral = as_global(f.integral);
  float* const gP3 = f.cloud.P3;
  const gptr<unsigned long long> gcarry = as_global(f.carry);
  const int capacity = f.cloud.capacity;
  const bool lean = GROUPED || cp.lean != 0;
  float vcarry[GROUPED ? 4 : 3] = {};      // y-pass running sums: chains tid + 256 jj (planes), the group's channels (grouped)
  bool starved = false;

  // loader: request depth + offsets of band b (all loads unconditional and in flight together; pixels outside the image read
  // element 0 and are zeroed when staged), later convert and put them into stage[b & 1]
  unsigned bits[kIR_Rows]; int off = 0;
  auto request_band = [&](int b) {
    const int r0 = b * kIR_Rows;
    if (is_raw) {
#pragma unroll
      for (int i = 0; i < kIR_Rows; ++i) {
        const int r = r0 + i;
        const unsigned pix = (r < rows && c < cols) ? (unsigned)(r * cols + c) : 0u;
        bits[i] = graw[pix];
      }
    } else {
#pragma unroll
      for (int i = 0; i < kIR_Rows; ++i) {
        const int r = r0 + i;
        const unsigned pix = (r < rows && c < cols) ? (unsigned)(r * cols + c) : 0u;
        bits[i] = __float_as_uint(gdepth[pix]);
      }
    }
    const int rr = r0 + (lane & (kIR_Rows - 1));
    off = growoff[(rr < rows ? rr : 0) * S + s];
  };
  auto stage_band = [&](int b) {
    const int r0 = b * kIR_Rows;
#pragma unroll
    for (int i = 0; i < kIR_Rows; ++i) {
      float d;
      if (is_raw) d = raw_to_metres(bits[i], raw_scale);
      else d = __uint_as_float(bits[i]);
      stage[b & 1][i * kIR_Cols + lane] = (r0 + i < rows && c < cols) ? d : 0.f;
    }
    sbase[b & 1][lane & (kIR_Rows - 1)] = off;       // 4 lanes write the same value
  };
  if (loader) { request_band(0); stage_band(0); }
  lds_barrier();

  for (int band = 0; band < NB; ++band) {
    const int r0 = band * kIR_Rows;
    if (loader) {
      const int nb = (band + 1 < NB) ? band + 1 : band;        // the last band re-reads itself (unconditional loads, result unused)
      request_band(nb);
      if (s > 0) {
        const gptr<unsigned long long> src = gcarry + ((size_t)(s - 1) * NB + band) * kII_Chains;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const int k = lane + 64 * m;
          if (k < kII_Chains) {
            unsigned long long w = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int spins = 0;
            while ((unsigned)(w >> 32) != epoch && !starved) {    // after one time-out this lane stops waiting: the launch is lost anyway
              if (++spins >= cp.spinLimit) { atomicOr(fault, 1); starved = true; break; }
              __builtin_amdgcn_s_sleep(1);
              w = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            cin[k] = __uint_as_float((unsigned)w);
          }
        }
      }
      stage_band(band + 1);
    } else {
      // 1. unproject: wave w owns rows r0 + w + 4j
#pragma unroll
      for (int jj = 0; jj < kIR_Rows / 4; ++jj) {
        const int lr = wave + 4 * jj;
        const int r = r0 + lr;
        const bool in = r < rows && c < cols;
        const float dd = stage[band & 1][lr * kIR_Cols + lane];
        const bool valid = in && depth_in_range(dd, cp.minD, cp.maxD);
        const unsigned long long bal = __ballot(valid);
        float v[kIntegralChannels];
#pragma unroll
        for (int k = 0; k < kIntegralChannels; ++k) v[k] = 0.f;
        if (in) {
          int idx = -1, itv = -1;
          if (valid) {
            idx = sbase[band & 1][lr] + __popcll(bal & ((1ull << lane) - 1ull));
            const Vec3 p = unproject_pixel(cp.iKRt, c, r, dd);
            if (idx < capacity) {
              if (!lean) store_xyz(gP3, idx, p.x, p.y, p.z);
              point_channels(v, p.x, p.y, p.z);
            }
            if (!lean) itv = depth_interval(cp.ivx, cp.ivy, dd);
          }
          __builtin_nontemporal_store(idx, gindex + (unsigned)(r * cols + c));
          if (!lean) __builtin_nontemporal_store(itv, ginterval + (unsigned)(r * cols + c));
        }
#pragma unroll
        for (int k = 0; k < kIntegralChannels; ++k) tile[(k * kIR_Rows + lr) * kIR_Stride + lane] = v[k];
      }
    }
    lds_barrier();
    // 2. x pass, chain (channel = tid / 16, row = tid % 16)
    if (chain) {
      float carry = (s > 0) ? cin[tid] : 0.f;
      float* t = &tile[tid * kIR_Stride];
#pragma unroll 1
      for (int c0 = 0; c0 < kIR_Cols; c0 += 16) {
        float vals[16];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) vals[cc] = t[c0 + cc];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) { carry = vals[cc] + carry; vals[cc] = carry; }
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) t[c0 + cc] = vals[cc];
      }
      if (s + 1 < S && (s * NB + band) * kII_Chains + tid != cp.dbgWithhold)
        __hip_atomic_store(gcarry + ((size_t)s * NB + band) * kII_Chains + tid,
                           ((unsigned long long)epoch << 32) | (unsigned long long)__float_as_uint(carry),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    lds_barrier();
    // 3. y pass.  Grouped: compute wave g owns group g (wave 3 has no chain), 64 columns each; one 16-byte (8-byte) store per row.
    // Planes: chain q = (channel = q / 64, column = q % 64)
    if constexpr (GROUPED) {
      if (wave < kIG_Groups) {
        const gptr<float> dst = gintegral + ig_at(N, wave, (size_t)r0 * cols + c);
        if (wave < 2) ypass_group<4>(tile, 4 * wave, lane, vcarry, c < cols, dst, 4u * (unsigned)cols, r0, rows);
        else ypass_group<2>(tile, 8, lane, vcarry, c < cols, dst, 2u * (unsigned)cols, r0, rows);
      }
    } else if (!loader) {
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) {
        const int q = tid + 256 * jj;
        if (q < kIntegralChannels * kIR_Cols) {
          const int ch = q >> 6;
          float vals[kIR_Rows];
#pragma unroll
          for (int r = 0; r < kIR_Rows; ++r) vals[r] = tile[(ch * kIR_Rows + r) * kIR_Stride + lane];
          float vc = vcarry[jj];
#pragma unroll
          for (int r = 0; r < kIR_Rows; ++r) { vc = vals[r] + vc; vals[r] = vc; }
          vcarry[jj] = vc;
          if (c < cols) {
            const gptr<float> dst = gintegral + ((size_t)ch * N + (size_t)r0 * cols + c);
#pragma unroll
            for (int r = 0; r < kIR_Rows; ++r) if (r0 + r < rows) __builtin_nontemporal_store(vals[r], dst + (unsigned)(r * cols));
          }
        }
      }
    }
    lds_barrier();
  }
}
__global__ void __launch_bounds__(kII_Threads) k_unproject_integral(const FrameDesc* __restrict__ frames, ConvertParams cp, int nframes,
                                                                    unsigned epoch, int* __restrict__ fault) {
  const int S = strips_of(cp.cols);
  const unsigned j = blockIdx.x >> 3;
  const int fi = 8 * (int)(j / (unsigned)S) + (int)(blockIdx.x & 7u), s = (int)(j % (unsigned)S);
  if (fi >= nframes) return;
  unproject_integral_body<false>(frames[fi], cp, s, epoch, fault);
}
// the same launch for ConvertParams::lean == kLeanGrouped: a kernel of its own, because it stores 16-byte records where the kernel above must not hold a
// 16-byte store (its 12-byte point records: see v3f)
__global__ void __launch_bounds__(kII_Threads) k_unproject_integral_grouped(const FrameDesc* __restrict__ frames, ConvertParams cp, int nframes,
                                                                            unsigned epoch, int* __restrict__ fault) {
  const int S = strips_of(cp.cols);
  const unsigned j = blockIdx.x >> 3;
  const int fi = 8 * (int)(j / (unsigned)S) + (int)(blockIdx.x & 7u), s = (int)(j % (unsigned)S);
  if (fi >= nframes) return;
  unproject_integral_body<true>(frames[fi], cp, s, epoch, fault);
}
// pass 3 (pwn_core/pointintegralimage.cpp:38-43): prefix-sum along image y inside each image column, sequential.
// one thread per (column, channel) chain, lanes along x.  grid = (ceil(cols/64), 10, frames), block = 64: this kernel only runs on the
// latency path (a few frames), where one-wave workgroups spread a frame's 6400 chains over 100 CUs instead of 30.
constexpr int kIC_Block = 64;
// fault / fault_out: the time-out flag of k_unproject_integral_rows (the launch before this one, complete by now) forwarded to a page-locked
// host word, so that the host reads it without a copy of its own (fault_out may be nullptr).
// grouped (ConvertParams::lean == kLeanGrouped): blockIdx.y is a group instead of a plane and a thread owns one float of the group's row -- (column, component),
// ig_width(group) * cols chains per group; grid = (ceil(4 * cols / 64), 3, frames).
__global__ void __launch_bounds__(kIC_Block) k_integral_cols(const FrameDesc* __restrict__ frames, int rows, int cols_, const int* __restrict__ fault,
                                                             int* __restrict__ fault_out, int grouped) {
  if (fault_out && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *fault_out = *fault;
  const FrameDesc& f = frames[blockIdx.z];
  const size_t N = (size_t)rows * cols_;
  const int cols = grouped ? ig_width((int)blockIdx.y) * cols_ : cols_;      // floats per row of the array this thread works in
  const int c = blockIdx.x * kIC_Block + threadIdx.x;
  if (c >= cols) return;
  float* p = f.integral + (grouped ? ig_at(N, (int)blockIdx.y, 0) : (size_t)blockIdx.y * N) + c;
  float carry = 0.f;
  int r = 0;
  constexpr int U = 16;
  for (; r + U <= rows; r += U) {
    float v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = p[(size_t)(r + k) * cols];
#pragma unroll
    for (int k = 0; k < U; ++k) { carry = v[k] + carry; v[k] = carry; }
#pragma unroll
    for (int k = 0; k < U; ++k) p[(size_t)(r + k) * cols] = v[k];
  }
  for (; r < rows; ++r) { carry = p[(size_t)r * cols] + carry; p[(size_t)r * cols] = carry; }
}

// ------------------------------------------------------------------------------------------------------------------
// StatsCalculatorIntegralImage::compute per-pixel loop (pwn_core/statscalculatorintegralimage.cpp:33-80) fused with
// PointInformationMatrixCalculator / NormalInformationMatrixCalculator::compute (informationmatrixcalculator.cpp:9-58)
// and Cloud::transformInPlace (cloud.cpp:173-186).  One thread per pixel, lanes along x.
// XCD-aware 1-D grid: workgroups are dealt round-robin over the 8 XCDs (block b and b+8 share an XCD and its 4 MiB L2), so
// block b works on frame 8*(k / blocksPerFrame) + (b % 8), k = b / 8, walking that frame's rows in order: every frame lives on
// one XCD and the four corner reads of neighbouring rows (2*radius rows apart, ~1.6 MB of planes) are L2 hits instead of one
// L2 fill per XCD.  Placement only affects speed.  grid = 8 * ceil(frames/8) * rows * ceil(cols/256) (frames >= 8; else frames * rows *
// ceil(cols/256), frame-major), block = 256.
__device__ __forceinline__ int clampi(int v, int lo, int hi) { v = (v < lo) ? lo : v; v = (v > hi) ? hi : v; return v; }
// streamed-once data of k_stats (index / interval / point in, cloud out) uses non-temporal accesses so that it does not evict the
// integral-image lines, which are the only data with reuse (each value is read by ~4 pixels)
template <typename PTR> __device__ __forceinline__ auto stream_load(PTR p) -> std::remove_cv_t<std::remove_reference_t<decltype(*p)>> {
  return __builtin_nontemporal_load(p);
}
template <typename PTR, typename T> __device__ __forceinline__ void stream_store(PTR p, T v) { __builtin_nontemporal_store(v, p); }
// the 12-byte records: not through the templates above (template argument deduction drops the typedef's alignment attribute and the access
// would be emitted with the vector type's natural `align 16`)
__device__ __forceinline__ v3f_raw stream_load3(gptr<const float> p) { return __builtin_nontemporal_load((gptr<const v3f>)p); }
__device__ __forceinline__ void stream_store3(gptr<float> p, v3f_raw v) { __builtin_nontemporal_store(v, (gptr<v3f>)p); }

// One pixel of the stats pass (everything after the thread has found its pixel): planes [10][rows][cols], point index from the index image.
__device__ __forceinline__ void stats_pixel(const FrameDesc& f, const ConvertParams& cp, const int r, const int c) {
  const int rows = cp.rows, cols = cp.cols;
  const size_t N = (size_t)rows * cols;
  // descriptor pointers are generic to the compiler; they all point to hipMalloc'ed memory: global_* instructions with a scalar
  // base and a 32-bit lane offset instead of flat_* with 64-bit VALU address arithmetic (the kernel is VALU-bound)
  const gptr<const int> gindex = as_global((const int*)f.index), ginterval = as_global((const int*)f.interval);
  const gptr<const float> gintegral = as_global((const float*)f.integral);
  const gptr<float> gP = as_global(f.cloud.P3), gN = as_global((float*)f.cloud.Nc), gOm = as_global(f.cloud.Om);
  const int cap = f.cloud.capacity;
  const unsigned upix = (unsigned)(r * cols + c);
  const int idx = stream_load(gindex + upix);
  if (idx < 0 || idx >= cap) return;
  int itv;
  float4 P;
  if (cp.lean) {
    // the front end kept the point and the interval to itself: recomputed from the same depth by the same helpers
    float d;
    if (f.raw) d = raw_to_metres(stream_load(as_global(f.raw) + upix), f.raw_scale);
    else d = stream_load(as_global(f.depth) + upix);
    const Vec3 p = unproject_pixel(cp.iKRt, c, r, d);
    P.x = p.x; P.y = p.y; P.z = p.z; P.w = 0.f;
    itv = depth_interval(cp.ivx, cp.ivy, d);
  } else {
    itv = stream_load(ginterval + upix);
    const v3f_raw pv = stream_load3((gptr<const float>)gP + 3u * (unsigned)idx); P.x = pv.x; P.y = pv.y; P.z = pv.z; P.w = 0.f;      // one 12-byte load
  }
  float nx = 0.f, ny = 0.f, nz = 0.f;
  float curvature = 0.f;          // Stats() default: eigenvalues 0 -> curvature() = 0/(0+1e-9) = 0  (stats.h:21-27,98-103)
  int cls = 0;
  float om[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) om[k] = 0.f;
  float U[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f };   // column-major
  float ev[3] = { 0.f, 0.f, 0.f };
  float mean[3] = { 0.f, 0.f, 0.f };
  int npts = 0;
  if (itv >= 0) {
    int rad = itv;
    if (rad < cp.minRadius) rad = cp.minRadius;
    if (rad > cp.maxRadius) rad = cp.maxRadius;
    // PointIntegralImage::getRegion (pointintegralimage.cpp:53-66)
    const int xmin = clampi(c - rad - 1, 0, cols - 1), xmax = clampi(c + rad - 1, 0, cols - 1);
    const int ymin = clampi(r - rad - 1, 0, rows - 1), ymax = clampi(r + rad - 1, 0, rows - 1);
    const unsigned oA = (unsigned)(ymax * cols + xmax), oB = (unsigned)(ymin * cols + xmin);
    const unsigned oC = (unsigned)(ymax * cols + xmin), oD = (unsigned)(ymin * cols + xmax);
    float a[kIntegralChannels];
    // group bases of the grouped storage: scalar; lane offsets: 32-bit bytes
    const gptr<const char> g0 = (gptr<const char>)gintegral, g1 = (gptr<const char>)(gintegral + ig_at(N, 1, 0)), g2 = (gptr<const char>)(gintegral + ig_at(N, 2, 0));
    if (cp.lean == kLeanGrouped) {
      // one record per corner holds (x, y, z, n): four loads decide whether the pixel needs the other eight
      const v4f A = *(gptr<const ig4>)(g0 + 16u * oA), B = *(gptr<const ig4>)(g0 + 16u * oB);
      const v4f C = *(gptr<const ig4>)(g0 + 16u * oC), D = *(gptr<const ig4>)(g0 + 16u * oD);
      a[0] = ((A.x + B.x) - C.x) - D.x; a[1] = ((A.y + B.y) - C.y) - D.y; a[2] = ((A.z + B.z) - C.z) - D.z; a[3] = ((A.w + B.w) - C.w) - D.w;
#pragma unroll
      for (int k = 4; k < kIntegralChannels; ++k) a[k] = 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < kIntegralChannels; ++k) {
        const gptr<const char> pl = (gptr<const char>)(gintegral + (size_t)k * N);      // plane base: scalar; lane offsets: 32-bit bytes
        float v;
        v = *(gptr<const float>)(pl + 4u * oA);
        v = v + *(gptr<const float>)(pl + 4u * oB);
        v = v - *(gptr<const float>)(pl + 4u * oC);
        v = v - *(gptr<const float>)(pl + 4u * oD);
        a[k] = v;
      }
    }
    const int n = (int)a[3];
    if (n >= cp.minPoints) {
      if (cp.lean == kLeanGrouped) {
        const v4f A = *(gptr<const ig4>)(g1 + 16u * oA), B = *(gptr<const ig4>)(g1 + 16u * oB);
        const v4f C = *(gptr<const ig4>)(g1 + 16u * oC), D = *(gptr<const ig4>)(g1 + 16u * oD);
        const ig2 E = *(gptr<const ig2>)(g2 + 8u * oA), F = *(gptr<const ig2>)(g2 + 8u * oB);
        const ig2 G = *(gptr<const ig2>)(g2 + 8u * oC), H = *(gptr<const ig2>)(g2 + 8u * oD);
        a[4] = ((A.x + B.x) - C.x) - D.x; a[5] = ((A.y + B.y) - C.y) - D.y; a[6] = ((A.z + B.z) - C.z) - D.z; a[7] = ((A.w + B.w) - C.w) - D.w;
        a[8] = ((E.x + F.x) - G.x) - H.x; a[9] = ((E.y + F.y) - G.y) - H.y;
      }
      npts = n;
      // PointAccumulator::mean / covariance (pointaccumulator.h:66-86)
      float d = a[3];
      float c00 = 0, c10 = 0, c20 = 0, c11 = 0, c21 = 0, c22 = 0;
      if (d != 0.f) {
        d = 1.0f / d;
        mean[0] = a[0] * d; mean[1] = a[1] * d; mean[2] = a[2] * d;
        c00 = a[4] * d - mean[0] * mean[0];
        c10 = a[5] * d - mean[1] * mean[0];
        c20 = a[6] * d - mean[2] * mean[0];
        c11 = a[7] * d - mean[1] * mean[1];
        c21 = a[8] * d - mean[2] * mean[1];
        c22 = a[9] * d - mean[2] * mean[2];
      }
      Vec3 v0, v1, v2;
      eig3_direct(c00, c10, c20, c11, c21, c22, ev, v0, v1, v2);
      if (ev[0] < 0.0f) ev[0] = 0.0f;
      U[0] = v0.x; U[1] = v0.y; U[2] = v0.z; U[3] = v1.x; U[4] = v1.y; U[5] = v1.z; U[6] = v2.x; U[7] = v2.y; U[8] = v2.z;
      // Stats::curvature (stats.h:98-103): fp32 sum, double +1e-9 and divide
      curvature = (float)((double)ev[0] / ((double)(ev[0] + ev[1] + ev[2]) + 1e-9));
      if (curvature < cp.statsCurvThr) {
        nx = v0.x; ny = v0.y; nz = v0.z;
        // normal.dot(point) > 0 -> flip (4-vector dot, w term 0*1)
        const float dp = dot4seq(nx, P.x, ny, P.y, nz, P.z, 0.f, 1.f);
        if (dp > 0) { nx = -nx; ny = -ny; nz = -nz; }
      }
    }
  }
  // information matrices
  const float sq = dot4seq(nx, nx, ny, ny, nz, nz, 0.f, 0.f);
  if (sq > 0) {
    float dg[3];
    if (curvature < cp.pointInfoCurvThr) { dg[0] = cp.pFlat[0]; dg[1] = cp.pFlat[1]; dg[2] = cp.pFlat[2]; }
    else { dg[0] = 1.0f / ev[0]; dg[1] = 1.0f / ev[1]; dg[2] = 1.0f / ev[2]; }
    // (U * D) * U^T, U(i,k) = U[i + 3k]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        om[3 * i + j] = dot3seq(U[i] * dg[0], U[j], U[i + 3] * dg[1], U[j + 3], U[i + 6] * dg[2], U[j + 6]);
    cls = (curvature < cp.normalInfoCurvThr) ? 1 : 2;
  }
  if (cp.keepStats && f.cloud.St) {
    float* st = f.cloud.St + (size_t)idx * 16;
    // Stats 4x4 after the optional sensor-offset left-multiplication (stats.h:125-131)
    if (cp.hasOffset) {
      Mat4 S = mat4_identity();
      if (npts > 0) {
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) S(i,j) = U[i + 3 * j];
        S(0,3) = mean[0]; S(1,3) = mean[1]; S(2,3) = mean[2]; S(3,3) = 1.f;
      }
      const Mat4 R = mat4_mul(cp.offset, S);
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) st[i + 3 * j] = R(i,j);
      st[12] = R(0,3); st[13] = R(1,3); st[14] = R(2,3);
    } else {
      for (int k = 0; k < 9; ++k) st[k] = U[k];
      st[12] = mean[0]; st[13] = mean[1]; st[14] = mean[2];
    }
    st[9] = ev[0]; st[10] = ev[1]; st[11] = ev[2];
    st[15] = (float)npts;
  }
  if (cp.hasOffset) {
    // Cloud::transformInPlace: p = m*p, n = m*n, Omega = T*Omega*T^t with T = m without last row/col
    const Mat4& m = cp.offset;
    // the point: the second half of converter_point (pwn_math.h); the first is the lean path's unproject_pixel above -- the normal's
    // orientation test in between wants the point in the sensor's frame
    const Vec3 po = offset_point(m, P.x, P.y, P.z);
    P.x = po.x; P.y = po.y; P.z = po.z;
    const float tx = dot4seq(m(0,0), nx, m(0,1), ny, m(0,2), nz, m(0,3), 0.0f);
    const float ty = dot4seq(m(1,0), nx, m(1,1), ny, m(1,2), nz, m(1,3), 0.0f);
    const float tz = dot4seq(m(2,0), nx, m(2,1), ny, m(2,2), nz, m(2,3), 0.0f);
    nx = tx; ny = ty; nz = tz;
    float t1[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) t1[3 * i + j] = dot3seq(m(i,0), om[0 + j], m(i,1), om[3 + j], m(i,2), om[6 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) om[3 * i + j] = dot3seq(t1[3 * i], m(j,0), t1[3 * i + 1], m(j,1), t1[3 * i + 2], m(j,2));
  }
  (void)cls;      // not stored: normal_class(normal, curvature, normalInfoCurvThr) gives it back
  {
    // one 12-byte and one 16-byte store (dword stores per lane would write every 1 KiB segment of the wave several times at a fraction of the density)
    v3f_raw pv; pv.x = P.x; pv.y = P.y; pv.z = P.z;
    v4f nv; nv.x = nx; nv.y = ny; nv.z = nz; nv.w = curvature;
    stream_store3(gP + 3u * (unsigned)idx, pv);
    stream_store((gptr<v4f>)(gN + 4u * (unsigned)idx), nv);
  }
  if (cp.omSym) {                        // sym6: (xx xy xz) (yy yz zz), the upper triangle as computed -- 24 bytes per point instead of 36
    v3f_raw r0, r1; r0.x = om[0]; r0.y = om[1]; r0.z = om[2]; r1.x = om[4]; r1.y = om[5]; r1.z = om[8];
    stream_store3(gOm + 3u * (unsigned)idx, r0);
    stream_store3(gOm + 3u * (size_t)cap + 3u * (unsigned)idx, r1);
    return;
  }
#pragma unroll
  for (int r3 = 0; r3 < 3; ++r3) {      // three 12-byte rows (nine dword stores per point cost k_stats 9 % more time)
    v3f_raw rw; rw.x = om[3 * r3]; rw.y = om[3 * r3 + 1]; rw.z = om[3 * r3 + 2];
    stream_store3(gOm + (size_t)r3 * 3u * (size_t)cap + 3u * (unsigned)idx, rw);
  }
}

__global__ void __launch_bounds__(256) k_stats(const FrameDesc* __restrict__ frames, ConvertParams cp, int nframes) {
  const int nxb = (cp.cols + 255) / 256;
  const int perFrame = nxb * cp.rows;
  int frame, rem;
  if (nframes >= 8) {
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    frame = (k / perFrame) * 8 + xcd;
    rem = k % perFrame;
  } else {                                   // fewer frames than XCDs (tracker, makeCloud): a frame per XCD would idle the others; grid = nframes * perFrame
    frame = blockIdx.x / perFrame;
    rem = blockIdx.x % perFrame;
  }
  if (frame >= nframes) return;
  const FrameDesc& f = frames[frame];
  const int r = rem / nxb;
  const int c = (rem % nxb) * 256 + threadIdx.x;
  if (c >= cp.cols) return;
  stats_pixel(f, cp, r, c);
}

// Cloud::transformInPlace on an existing device cloud (cloud.cpp:173-186); grid = ceil(cap/256)
__global__ void __launch_bounds__(256) k_cloud_transform(CloudDev cl, Mat4 m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= *cl.count || i >= cl.capacity) return;
  float4 P, Nm;
  cloud_get(cl, i, P, Nm);
  const float px = dot4seq(m(0,0), P.x, m(0,1), P.y, m(0,2), P.z, m(0,3), 1.0f);
  const float py = dot4seq(m(1,0), P.x, m(1,1), P.y, m(1,2), P.z, m(1,3), 1.0f);
  const float pz = dot4seq(m(2,0), P.x, m(2,1), P.y, m(2,2), P.z, m(2,3), 1.0f);
  P.x = px; P.y = py; P.z = pz;
  const float tx = dot4seq(m(0,0), Nm.x, m(0,1), Nm.y, m(0,2), Nm.z, m(0,3), 0.0f);
  const float ty = dot4seq(m(1,0), Nm.x, m(1,1), Nm.y, m(1,2), Nm.z, m(1,3), 0.0f);
  const float tz = dot4seq(m(2,0), Nm.x, m(2,1), Nm.y, m(2,2), Nm.z, m(2,3), 0.0f);
  Nm.x = tx; Nm.y = ty; Nm.z = tz;
  for (int pass = 0; pass < 2; ++pass) {
    float* base = pass == 0 ? cl.Om : cl.OmN;
    if (!base) continue;
    float om[9], t1[9];
    const int sym = pass == 0 ? cl.omSym : 0;
    for (int k = 0; k < 9; ++k) om[k] = base[omp_at(cl.capacity, i, k, sym)];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) t1[3 * a + b] = dot3seq(m(a,0), om[0 + b], m(a,1), om[3 + b], m(a,2), om[6 + b]);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) om[3 * a + b] = dot3seq(t1[3 * a], m(b,0), t1[3 * a + 1], m(b,1), t1[3 * a + 2], m(b,2));
    for (int k = 0; k < 9; ++k) if (!(sym && om_is_lower(k))) base[omp_at(cl.capacity, i, k, sym)] = om[k];
  }
  cloud_put(cl, i, P, Nm);
}

// ------------------------------------------------------------------------------------------------------------------
// PinholePointProjector::project (pwn_core/pinholepointprojector.cpp:33-66): z-buffer by 64-bit atomicMin on
// (depth bits, point index): nearest point wins, ties keep the lowest index (the reference's strict '>' in a
// sequential loop).  grid = (ceil(capacity/256), pairs), block = 256.  which: 0 = reference cloud, 1 = current.
// _project of the aligner's projections: false when the depth is out of range or the pixel (x, y) outside the image
__device__ __forceinline__ bool project_to_pixel(const Mat4& KRt, float minD, float maxD, int rows, int cols, const float4 p, float& d, int& x, int& y) {
  const Vec3 ip = project_plane(KRt, p.x, p.y, p.z);
  d = ip.z;
  if (!depth_in_range(d, minD, maxD)) return false;
  float fx, fy;
  round_to_pixel(ip, fx, fy);
  if (!in_image(fx, fy, rows, cols)) return false;
  x = (int)fx; y = (int)fy;
  return true;
}
__device__ __forceinline__ void project_point(const Mat4& KRt, float minD, float maxD, int rows, int cols,
                                              const float4 p, int i, unsigned long long* z, unsigned tag) {
  float d; int x, y;
  if (project_to_pixel(KRt, minD, maxD, rows, cols, p, d, x, y)) atomicMin(&z[(size_t)y * cols + x], zkey(tag, d, i));
}
// depth of a point under a projector matrix: the third row of _project
__device__ __forceinline__ float point_depth(const Mat4& KRt, const float4 p) { return affine_row(KRt, 2, p.x, p.y, p.z); }
// 32-bit z-buffer insert (see kZ32Tag0) in two steps, so that a thread with several points has all its atomics in flight before it
// looks at the first returned word.  z32_insert: the projection and the atomicMin; w = nullptr when the point is rejected.
struct Z32Pending { unsigned* w; unsigned key, old; float d; };
__device__ __forceinline__ Z32Pending z32_insert(const Mat4& KRt, float minD, float maxD, int rows, int cols, const float4 p, int i, unsigned* z, unsigned tag) {
  Z32Pending r; r.w = nullptr; r.key = 0u; r.old = ~0u; r.d = 0.f;
  float d; int x, y;
  if (!project_to_pixel(KRt, minD, maxD, rows, cols, p, d, x, y)) return r;
  r.w = &z[(size_t)y * cols + x];
  r.key = z32key(tag, i); r.d = d;
  r.old = atomicMin(r.w, r.key);
  return r;
}
// z32_settle: nothing to do for the first point of this projection in its pixel (older tags and the empty word are larger than any key of
// the current tag); otherwise make sure the word ends up with the nearest of every point this thread gets to see, ties to the lower index.
// P: the cloud's points (to evaluate the depth of a point met in the pixel).
// The loop is lock-free (a failed compare-and-swap means another thread's write went through, and the word only changes a bounded number of
// times: one insert per point, and every successful swap installs a strictly nearer point), but its length has no useful bound when tens of
// thousands of points of one projection share a pixel.  A thread that has not settled after guardLimit rounds gives up and raises the
// call's fault word (page-locked host memory, PairDesc::fault): the host then repeats the call with the two-pass projection below, so a
// pixel is never silently left with the wrong point (pinholepointprojector.cpp:54-63).
constexpr int kSettleGuard = 4096;
__device__ __forceinline__ bool z32_settle(const Z32Pending& q, const Mat4& KRt, const float* __restrict__ P3, unsigned tag, int guardLimit) {
  if (!q.w || (q.old >> kZIndexBits) != tag) return true;
  int best = (int)(q.key & kZ32IndexMask); float dbest = q.d;
  unsigned cur = q.old < q.key ? q.old : q.key;       // what the word holds after the atomicMin, unless someone changed it since
  unsigned seen = q.old;
  for (int guard = 0; guard < guardLimit; ++guard) {
    const int j = (int)(seen & kZ32IndexMask);
    if (j != best) {
      const float dj = point_depth(KRt, load_xyz(P3, j));
      if (dj < dbest || (dj == dbest && j < best)) { best = j; dbest = dj; }
    }
    const unsigned want = z32key(tag, best);
    if (cur == want) return true;
    const unsigned r = atomicCAS(q.w, cur, want);
    if (r == cur) return true;                        // installed
    seen = r; cur = r;                                // somebody else wrote (same tag): weigh its point too and try again
  }
  return false;
}
// PPT points per thread: all loads first, then all atomicMin's, then the (rare) collisions -- with one point per thread the wave waits
// for every returned word before it does anything else (measured per 64-pair launch: 134 us with 1 point per thread, 104 with 2, 101
// with 4; the 64-bit no-return atomicMin it replaces: 131).  Small launches (single alignments) keep 1: they need the workgroups.
// grid.x = ceil(capacity / (256 * PPT))
template <int PPT>
__global__ void __launch_bounds__(256) k_project(const PairDesc* __restrict__ pairs, AlignParams ap, int which, unsigned tag) {
  constexpr int kProjectPointsPerThread = PPT;
  const PairDesc& pd = pairs[blockIdx.y];
  if (!which && ap.mayFreeze && pair_frozen(pd.state)) return;      // a converged pair keeps the z-buffer words of its last iteration: nothing is inserted (workgroup-uniform)
  const CloudDev& cl = which ? pd.cur : pd.ref;
  const int n = min(*cl.count, cl.capacity);
  const int i0 = blockIdx.x * 256 * kProjectPointsPerThread + threadIdx.x;
  if (i0 >= n) return;
  const Mat4 KRt = uniform_iso(which ? pd.state->KRtCur : pd.state->KRt);
  unsigned* z = which ? pd.zcur : pd.zref;
  float4 p[kProjectPointsPerThread];
#pragma unroll
  for (int j = 0; j < kProjectPointsPerThread; ++j) { const int i = i0 + 256 * j; if (i < n) p[j] = load_xyz(cl.P3, i); }      // loads first (12 bytes per point)
  Z32Pending q[kProjectPointsPerThread];
#pragma unroll
  for (int j = 0; j < kProjectPointsPerThread; ++j) {
    const int i = i0 + 256 * j;
    if (i < n) q[j] = z32_insert(KRt, ap.minD, ap.maxD, ap.rows, ap.cols, p[j], i, z, tag); else q[j].w = nullptr;
  }
  bool settled = true;
#pragma unroll
  for (int j = 0; j < kProjectPointsPerThread; ++j) settled = z32_settle(q[j], KRt, cl.P3, tag, ap.settleGuard) && settled;
  if (!settled) __hip_atomic_store(pd.fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The same projection without a retry loop, for calls whose k_project gave up (and for nothing else: it reads the points twice and clears a
// depth image per projection).  Pass 1: the nearest depth per pixel by atomicMin on the depth's bit pattern (depths are >= 0: min_distance >= 0
// is checked by the host, so the patterns order like the values; -0 counts as 0) in the pair's own depth image PairDesc::zdepth, cleared to ~0
// by the host before the launch.  Pass 2: every point that has its pixel's nearest depth enters the 32-bit word by atomicMin on tag | index:
// the nearest point, ties to the lowest index -- the reference's sequential strict '>' (pinholepointprojector.cpp:61), the word k_project leaves.
__global__ void __launch_bounds__(256) k_project_robust(const PairDesc* __restrict__ pairs, AlignParams ap, int which, unsigned tag, int pass) {
  const PairDesc& pd = pairs[blockIdx.y];
  if (!which && ap.mayFreeze && pair_frozen(pd.state)) return;      // as in k_project: neither the pair's depth image nor its z-buffer words are touched
  const CloudDev& cl = which ? pd.cur : pd.ref;
  const int n = min(*cl.count, cl.capacity);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Mat4 KRt = uniform_iso(which ? pd.state->KRtCur : pd.state->KRt);
  float d; int x, y;
  if (!project_to_pixel(KRt, ap.minD, ap.maxD, ap.rows, ap.cols, load_xyz(cl.P3, i), d, x, y)) return;
  const int pix = y * ap.cols + x;
  const unsigned dbits = __float_as_uint(d) & 0x7fffffffu;
  if (pass == 0) atomicMin(&pd.zdepth[pix], dbits);
  else if (pd.zdepth[pix] == dbits) atomicMin(&(which ? pd.zcur : pd.zref)[pix], z32key(tag, i));
}
// current-cloud z-buffer -> int index image, once per alignment.  grid = (blocks, pairs)
__global__ void k_resolve_cur(const PairDesc* __restrict__ pairs, int n, unsigned tag) {
  const PairDesc& pd = pairs[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    pd.curidx[i] = z32_index(pd.zcur[i], tag);
}
// CorrespondenceFinder::{reference,current}{Index,Depth}Image() of a pair after its alignment: index from the 32-bit z-buffer, depth
// recomputed from the winning point with the matrix its projection used; empty pixels -1 / FLT_MAX (pinholepointprojector.cpp:41-42)
__global__ void k_pair_images(const PairDesc* __restrict__ pairs, int which, unsigned tag, int n, int* __restrict__ index, float* __restrict__ depth) {
  const PairDesc& pd = pairs[0];
  const CloudDev& cl = which ? pd.cur : pd.ref;
  const unsigned* z = which ? pd.zcur : pd.zref;
  const Mat4 KRt = which ? pd.state->KRtCur : pd.state->KRtLast;
  const int np = min(*cl.count, cl.capacity);
  if (!which) tag = pair_ref_tag(pd.state, tag);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int k = z32_index(z[i], tag);
    if (index) index[i] = k;
    if (depth) depth[i] = (k >= 0 && k < np) ? point_depth(KRt, load_xyz(cl.P3, k)) : FLT_MAX;
  }
}
// stand-alone projection with an explicit matrix (pwn_hip_project)
__global__ void __launch_bounds__(256) k_project_single(CloudDev cl, Mat4 KRt, float minD, float maxD, int rows, int cols,
                                                        unsigned long long* z, unsigned tag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = min(*cl.count, cl.capacity);
  if (i >= n) return;
  project_point(KRt, minD, maxD, rows, cols, load_xyz(cl.P3, i), i, z, tag);
}
// z-buffer -> (index image, depth image): empty pixels -1 / FLT_MAX (pinholepointprojector.cpp:41-42)
__global__ void k_zbuf_resolve(const unsigned long long* __restrict__ z, int n, int* __restrict__ index, float* __restrict__ depth, unsigned tag) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned long long k = z[i];
    if (index) index[i] = zkey_index(k, tag);
    if (depth) depth[i] = zkey_depth(k, tag);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// PwnCloserWithMerger::mergeNode (pwn_tracker2/pwn_closer_with_merger.cpp:210-224) for the nodes of a partition in one launch: the depth
// images of n clouds, each under its own projector, and their pixel-wise fusion (Merger2::mergeDepthImage, pwn_tracker2/merger2.cpp:75-101).
//
// k_project_depth_batch: PinholePointProjector::project's depth image (pinholepointprojector.cpp:33-66) of cloud blockIdx.y under
// KRt[blockIdx.y] into plane blockIdx.y (rows * cols words).  Only the depths are wanted, so a point that passes _project does one atomicMin
// on its depth's bit pattern (the sign bit masked as in k_project_robust: min_distance >= 0 is the host's check, so the patterns order like
// the values) and nothing else: no index, no settle loop, no second pass.  The planes are cleared to the bit pattern of FLT_MAX; afterwards
// a plane read as floats is the projector's depth image: FLT_MAX where nothing landed (:41-42), else the nearest depth.
// grid = (ceil(largest capacity / (256 * PPT)), n), block = 256
struct DepthCloudDesc { const float* P3; const int* count; int capacity; };
constexpr unsigned kDepthPlaneEmpty = 0x7f7fffffu;      // FLT_MAX
template <int PPT>
__global__ void __launch_bounds__(256) k_project_depth_batch(const DepthCloudDesc* __restrict__ clouds, const Mat4* __restrict__ KRts, float minD, float maxD,
                                                             int rows, int cols, unsigned* __restrict__ planes) {
  const DepthCloudDesc cl = clouds[blockIdx.y];
  const int n = min(*cl.count, cl.capacity);
  const int i0 = blockIdx.x * 256 * PPT + threadIdx.x;
  if (i0 >= n) return;
  const Mat4 KRt = uniform_iso_global(as_global((const float*)(KRts + blockIdx.y)));
  unsigned* plane = planes + (size_t)blockIdx.y * ((size_t)rows * cols);
  float4 p[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) { const int i = i0 + 256 * j; if (i < n) p[j] = load_xyz(cl.P3, i); }
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    float d; int x, y;
    if (i0 + 256 * j < n && project_to_pixel(KRt, minD, maxD, rows, cols, p[j], d, x, y))
      atomicMin(&plane[(size_t)y * cols + x], __float_as_uint(d) & 0x7fffffffu);
  }
}
// k_merge_depth_images: one thread per pixel walks the m planes in call order with Merger2::mergeDepthImage's arithmetic, literally: the
// range test and the two thresholds in double against the double literals, the weight an IEEE division, the weighted mean from separately
// rounded products (dot2seq), `out` and the weight image in / out -- m planes in one launch are m successive mergeDepthImage calls.
// overlap[k] += pixels of plane k inside (0.1, 10000) (_image_overlapping_points_count, which the reference resets per image: the host
// clears the words), *points += pixels replaced (_image_points_count): a ballot per wave, an LDS word per counter, one global atomic per
// workgroup and non-zero counter.  grid = ceil(N / 256), block = 256, m <= kMergePlanesMax
constexpr int kMergePlanesMax = 256;
__global__ void __launch_bounds__(256) k_merge_depth_images(const float* const* __restrict__ planes, int m, int N, float* __restrict__ out,
                                                            float* __restrict__ weights, int* __restrict__ overlap, int* __restrict__ points) {
  __shared__ int s_cnt[kMergePlanesMax + 1];
  for (int t = threadIdx.x; t <= m; t += 256) s_cnt[t] = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool live = i < (unsigned)N;
  float o = 0.f, w = 0.f;
  if (live) { o = out[i]; w = weights[i]; }
  int replaced = 0;
  for (int k = 0; k < m; ++k) {
    bool selected = false;
    if (live) {
      const float d = as_global(planes[k])[i];
      selected = (double)d > 0.1 && (double)d < 10000;                   // merger2.cpp:80
      if (selected) {
        const float peso = 1.0f / d;                                     // :82
        if (o == 0.f || (double)(d - o) < -.00003) {                     // :84
          ++replaced; o = d; w = peso;                                   // :86-89
        } else if ((double)fabsf(d - o) < .2) {                          // :91
          const float somma = w + peso;                                  // :93
          o = dot2seq(o, w, d, peso) / somma;                            // :94
          w = somma;                                                     // :95
        }
      }
    }
    const int c = __popcll(__ballot(selected));
    if (lane_id() == 0 && c) atomicAdd(&s_cnt[k], c);
  }
  if (live) { out[i] = o; weights[i] = w; }
  const int r = (int)wave_sum((float)replaced);      // <= 64 * kMergePlanesMax: exact in fp32
  if (lane_id() == 0 && r) atomicAdd(&s_cnt[m], r);
  __syncthreads();
  for (int t = threadIdx.x; t <= m; t += 256)
    if (s_cnt[t]) atomicAdd(t < m ? overlap + t : points, s_cnt[t]);
}

// ------------------------------------------------------------------------------------------------------------------
// One correspondence's contribution to the normal equations: Linearizer::update loop body
// (pwn_core/linearizer.cpp:57-88).  oP / oN: row-major 3x3 information matrices of the CURRENT point.
// The 4x4 products of the reference are written out for the non-zero 3x3 part; dropped terms are exact zeros.
__device__ __forceinline__ void skewT_mul(float tx, float ty, float tz, const float* m /*row-major 3x3*/, float* out) {
  // out = S^T * m with S = skew(v) = -2[v]x, (tx,ty,tz) = 2v   (bm_se3.h:54-66)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    out[0 + j] = (-tz) * m[3 + j] + ty * m[6 + j];
    out[3 + j] = tz * m[0 + j] + (-tx) * m[6 + j];
    out[6 + j] = (-ty) * m[0 + j] + tx * m[3 + j];
  }
}
__device__ __forceinline__ void mul_skew(const float* a /*row-major 3x3*/, float tx, float ty, float tz, float* out) {
  // out = a * S
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out[3 * i + 0] = a[3 * i + 1] * (-tz) + a[3 * i + 2] * ty;
    out[3 * i + 1] = a[3 * i + 0] * tz + a[3 * i + 2] * (-tx);
    out[3 * i + 2] = a[3 * i + 0] * (-ty) + a[3 * i + 1] * tx;
  }
}
// Accumulator policies of linearize_term: registers (RegAcc) or one private LDS column per thread (LdsAcc; frees ~34 VGPRs,
// which is what limits the occupancy of the fused kernel).  LdsAcc::add is a plain read-add-write of the thread's own slot.
struct RegAcc {
  float* a;
  __device__ __forceinline__ void add(int k, float v) const { a[k] += v; }
};
// The Gauss-Newton step solves with Matrix6f::ldlt(), which reads the LOWER triangle of H only (aligner.cpp:112; Eigen's LDLT
// default): the strictly upper entries of the Htt and Hrr blocks (acc_is_upper) are never looked at, so the iteration kernels
// do not accumulate them (FULL = false) and their LDS columns have no slot for them (acc_slot_lower).  Aligner::_computeStatistics
// inverts the full H, the pass that feeds it runs with FULL = true (all kAccTerms sums).
__host__ __device__ constexpr bool acc_block_upper(int k, int base) { return k >= base && k < base + 9 && (k - base) % 3 < (k - base) / 3; }   // row < column
__host__ __device__ constexpr bool acc_is_upper(int k) { return acc_block_upper(k, kAccHtt) || acc_block_upper(k, kAccHrr); }
__host__ __device__ constexpr int acc_upper_below(int k) { int n = 0; for (int j = 0; j < k; ++j) n += acc_is_upper(j); return n; }
__host__ __device__ constexpr int acc_slot_lower(int k) { return k - acc_upper_below(k); }
template <bool FULL> struct LdsAcc {
  static constexpr int kSlots = kAccTerms - (FULL ? 0 : acc_upper_below(kAccTerms));
  float* base;      // &lds[threadIdx.x], stride kAlignBlock
  __device__ __forceinline__ void add(int k, float v) const {
    if (!FULL && acc_is_upper(k)) return;
    base[(FULL ? k : acc_slot_lower(k)) * kAlignBlock] += v;
  }
};
static_assert(kAccN == 37 && LdsAcc<true>::kSlots == 34 && LdsAcc<false>::kSlots == 28 && acc_slot_lower(kAccChi2) == 27, "the sum record's sizes");
static_assert(acc_is_upper(3) && acc_is_upper(6) && acc_is_upper(7) && acc_is_upper(21) && acc_is_upper(24) && acc_is_upper(25) &&
              acc_upper_below(kAccN) == 6, "the strictly upper entries of Htt and Hrr, and no other slot");
// a*b + c*d of the H / b products: two roundings of the products and one of the sum, as the CPU path evaluates them (no FMA)
#define MAD2(a, b, c, d) ((a) * (b) + (c) * (d))
// returns false if the term is rejected (non-robust kernel and chi2 above threshold)
template <typename ACC>
__device__ __forceinline__ bool linearize_term(const float3 rp, const float3 rn, const float3 cp, const float3 cn,
                                               const float* oP, const float* oN, float maxChi2, int robust, const ACC acc) {
  const float pe0 = rp.x - cp.x, pe1 = rp.y - cp.y, pe2 = rp.z - cp.z;
  const float ne0 = rn.x - cn.x, ne1 = rn.y - cn.y, ne2 = rn.z - cn.z;
  float ep[3], en[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ep[i] = dot3seq(oP[3 * i], pe0, oP[3 * i + 1], pe1, oP[3 * i + 2], pe2);
    en[i] = dot3seq(oN[3 * i], ne0, oN[3 * i + 1], ne1, oN[3 * i + 2], ne2);
  }
  const float localError = dot3seq(pe0, ep[0], pe1, ep[1], pe2, ep[2]) + dot3seq(ne0, en[0], ne1, en[1], ne2, en[2]);
  float kscale = 1.f;
  if (localError > maxChi2) {
    if (robust) kscale = sqrtf(maxChi2 / localError);
    else return false;
  }
  const float ptx = 2 * rp.x, pty = 2 * rp.y, ptz = 2 * rp.z;
  const float ntx = 2 * rn.x, nty = 2 * rn.y, ntz = 2 * rn.z;
  // Sp^T ep + Sn^T en
  const float s0 = (MAD2((-ptz), ep[1], pty, ep[2])) + (MAD2((-ntz), en[1], nty, en[2]));
  const float s1 = (MAD2(ptz, ep[0], (-ptx), ep[2])) + (MAD2(ntz, en[0], (-ntx), en[2]));
  const float s2 = (MAD2((-pty), ep[0], ptx, ep[1])) + (MAD2((-nty), en[0], ntx, en[1]));
  // Row by row (keeps few values live): Htt += omegaP ; Htr += omegaP*Sp ; Hrr += (Sp^T omegaP Sp + Sn^T omegaN Sn).
  // accumulators are column-major 3x3 blocks: acc[kAccH.. + i + 3*j]
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float a0 = oP[3 * i], a1 = oP[3 * i + 1], a2 = oP[3 * i + 2];
    acc.add(kAccHtt + i, a0); acc.add(kAccHtt + i + 3, a1); acc.add(kAccHtt + i + 6, a2);
    acc.add(kAccHtr + i, MAD2(a1, (-ptz), a2, pty));                    // (omegaP * Sp)(i, 0..2)
    acc.add(kAccHtr + i + 3, MAD2(a0, ptz, a2, (-ptx)));
    acc.add(kAccHtr + i + 6, MAD2(a0, (-pty), a1, ptx));
    // row i of Sp^T*omegaP and of Sn^T*omegaN
    float p0, p1, p2, q0, q1, q2;
    if (i == 0) {
      p0 = MAD2((-ptz), oP[3], pty, oP[6]); p1 = MAD2((-ptz), oP[4], pty, oP[7]); p2 = MAD2((-ptz), oP[5], pty, oP[8]);
      q0 = MAD2((-ntz), oN[3], nty, oN[6]); q1 = MAD2((-ntz), oN[4], nty, oN[7]); q2 = MAD2((-ntz), oN[5], nty, oN[8]);
    } else if (i == 1) {
      p0 = MAD2(ptz, oP[0], (-ptx), oP[6]); p1 = MAD2(ptz, oP[1], (-ptx), oP[7]); p2 = MAD2(ptz, oP[2], (-ptx), oP[8]);
      q0 = MAD2(ntz, oN[0], (-ntx), oN[6]); q1 = MAD2(ntz, oN[1], (-ntx), oN[7]); q2 = MAD2(ntz, oN[2], (-ntx), oN[8]);
    } else {
      p0 = MAD2((-pty), oP[0], ptx, oP[3]); p1 = MAD2((-pty), oP[1], ptx, oP[4]); p2 = MAD2((-pty), oP[2], ptx, oP[5]);
      q0 = MAD2((-nty), oN[0], ntx, oN[3]); q1 = MAD2((-nty), oN[1], ntx, oN[4]); q2 = MAD2((-nty), oN[2], ntx, oN[5]);
    }
    acc.add(kAccHrr + i, (MAD2(p1, (-ptz), p2, pty)) + (MAD2(q1, (-ntz), q2, nty)));
    acc.add(kAccHrr + i + 3, (MAD2(p0, ptz, p2, (-ptx))) + (MAD2(q0, ntz, q2, (-ntx))));
    acc.add(kAccHrr + i + 6, (MAD2(p0, (-pty), p1, ptx)) + (MAD2(q0, (-nty), q1, ntx)));
  }
  acc.add(kAccBt, kscale * ep[0]); acc.add(kAccBt + 1, kscale * ep[1]); acc.add(kAccBt + 2, kscale * ep[2]);
  acc.add(kAccBr, kscale * s0); acc.add(kAccBr + 1, kscale * s1); acc.add(kAccBr + 2, kscale * s2);
  acc.add(kAccChi2, kscale * localError);
  return true;
}
__device__ __forceinline__ void load_omegas(const CloudDev& cur, int ci, int cls, float* oP, float* oN) {
  const size_t cap = (size_t)cur.capacity;
#pragma unroll
  for (int k = 0; k < 9; ++k) oP[k] = cur.Om[omp_at(cap, ci, k, cur.omSym)];
  if (cur.OmN) {
#pragma unroll
    for (int k = 0; k < 9; ++k) oN[k] = cur.OmN[om_at(cap, ci, k)];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) oN[k] = (cls == 1) ? cur.omN[0][k] : ((cls == 2) ? cur.omN[1][k] : 0.f);
  }
}
__device__ __forceinline__ float3 iso_point(const Mat4& T, const float4 p) {
  float3 r;
  r.x = dot4seq(T(0,0), p.x, T(0,1), p.y, T(0,2), p.z, T(0,3), 1.0f);
  r.y = dot4seq(T(1,0), p.x, T(1,1), p.y, T(1,2), p.z, T(1,3), 1.0f);
  r.z = dot4seq(T(2,0), p.x, T(2,1), p.y, T(2,2), p.z, T(2,3), 1.0f);
  return r;
}
__device__ __forceinline__ float3 iso_normal(const Mat4& T, const float4 n) {
  float3 r;
  r.x = dot4seq(T(0,0), n.x, T(0,1), n.y, T(0,2), n.z, T(0,3), 0.0f);
  r.y = dot4seq(T(1,0), n.x, T(1,1), n.y, T(1,2), n.z, T(1,3), 0.0f);
  r.z = dot4seq(T(2,0), n.x, T(2,1), n.y, T(2,2), n.z, T(2,3), 0.0f);
  return r;
}
// CorrespondenceFinder::compute acceptance tests (pwn_core/correspondencefinder.cpp:60-99) for one pixel.
// rp / rn return the reference point / normal remapped by Tc (reused by the linearizer when its transform is the same).
__device__ __forceinline__ bool correspondence_test(const AlignParams& ap, const Mat4& Tc, const float4 rP, const float4 rN,
                                                    const float4 cP, const float4 cN, float3& rp, float3& rn) {
  if (dot4seq(cN.x, cN.x, cN.y, cN.y, cN.z, cN.z, 0.f, 0.f) == 0.0f || dot4seq(rN.x, rN.x, rN.y, rN.y, rN.z, rN.z, 0.f, 0.f) == 0.0f)
    return false;
  rp = iso_point(Tc, rP);
  rn = iso_normal(Tc, rN);
  if (dot4seq(cN.x, rn.x, cN.y, rn.y, cN.z, rn.z, 0.f, 0.f) < ap.normalThr) return false;
  const float dx = cP.x - rp.x, dy = cP.y - rp.y, dz = cP.z - rp.z;
  if (dot4seq(dx, dx, dy, dy, dz, dz, 0.f, 0.f) > ap.sqDist) return false;
  float rc = rP.w, cc = cP.w;
  if (rc < ap.flatThr) rc = ap.flatThr;
  if (cc < ap.flatThr) cc = ap.flatThr;
  // The reference evaluates (rc + 1e-5) / (cc + 1e-5) in double and compares the float-rounded ratio with the bounds
  // (correspondencefinder.cpp:96-99).  An fp32 estimate (relative error < 1e-6) decides every case that is not within
  // 1e-5 of a bound; only those run the exact double computation, so the decision is always the reference's.
  const float est = (rc + 1e-5f) / (cc + 1e-5f);
  if (est < ap.minRatio * (1.0f - 1e-5f) || est > ap.maxRatio * (1.0f + 1e-5f)) return false;
  if (est > ap.minRatio * (1.0f + 1e-5f) && est < ap.maxRatio * (1.0f - 1e-5f)) return true;
  const float ratio = (float)(((double)rc + 1e-5) / ((double)cc + 1e-5));
  if (ratio < ap.minRatio || ratio > ap.maxRatio) return false;
  return true;
}

// the record of the thread that owns column `col` of the LDS sums (LdsAcc<FULL>) and counted K candidates, C correspondences and the inliers
template <bool FULL>
__device__ __forceinline__ void acc_from_lds(const float* lds, int col, float K, float C, float inliers, float* acc) {
#pragma unroll
  for (int k = 0; k < kAccTerms; ++k)
    acc[k] = (FULL || !acc_is_upper(k)) ? lds[(FULL ? k : acc_slot_lower(k)) * kAlignBlock + col] : 0.f;
  acc[kAccCand] = K; acc[kAccCorr] = C; acc[kAccInliers] = inliers;
}
// block-level reduction of kAccN fp32 accumulators -> fp64 partial record of the block: a wave tree per sum, the kAlignBlock / 64 wave sums in
// order, in double.  contributes: this thread is one of the block's first kAlignBlock and acc is its record (whole waves; the rest only meet the barrier)
template <bool FULL = true>
__device__ __forceinline__ void block_reduce_store(const float* acc, double* out_generic, bool contributes) {
  const gptr<double> out = as_global(out_generic);
  __shared__ float red[kAlignBlock / 64][kAccN];
  if (contributes) {
#pragma unroll
    for (int k = 0; k < kAccN; ++k) {
      if (!FULL && acc_is_upper(k)) {            // sums the lower-triangle passes do not accumulate: exact zeros, no reduction
        if (lane_id() == 63) red[threadIdx.x >> 6][k] = 0.f;
        continue;
      }
      const float v = wave_sum_dpp_lane63(acc[k]);
      if (lane_id() == 63) red[threadIdx.x >> 6][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < kAccN) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kAlignBlock / 64; ++w) s += (double)red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// Fused CorrespondenceFinder::compute + Linearizer::update (correspondencefinder.cpp:45-106, linearizer.cpp:33-90):
// one pass over the pixels, no correspondence list is materialised; the z-buffer is epoch-tagged, nothing is written back.
// The kernel is latency-bound (index -> point/normal gathers -> information-matrix gathers are dependent loads), so it
// is software-pipelined by hand as a rolling three-stage loop: indices of pixel j+2, point/normal gathers of pixel j+1,
// tests + arithmetic of pixel j.  Measured on MI355X: prefetching the 9 information-matrix planes as well costs more
// in occupancy (174 VGPRs -> 2 waves/SIMD) than it hides (13.2 ms vs 9.8 ms per 128x10 pair-iterations; docs/experiments.md).
// grid = (ceil(N / (256*kPixPerThread)), pairs), block = 256.
struct Candidate {
  float4 rP, rN, cP, cN;
  int ci;
  bool valid;
  unsigned craw;      // CUR_DEPTH: the pixel's raw depth (STRIP_IDX: its depth in metres, as bits) stands for cP.xyz (CurDepthSrc), one register instead of three
};
// The descriptor's pointers are generic to the compiler: flat_* loads, which count on BOTH the vector-memory and the LDS counter, so
// every wait for an LDS accumulator update would also wait for the gathers of the next pixel that are meant to stay in flight.
// They all point to hipMalloc'ed memory: as_global() -> global_* loads (vmcnt only).
struct PairPtrs {
  gptr<const float> refP, curP;      // packed xyz
  gptr<const v4f> refN, curN;        // (normal, curvature)
  gptr<const float> curOm, curOmN;
  gptr<const unsigned> zref;
  gptr<const int> curidx, refidx0;
  unsigned cap;      // capacity of the current cloud (plane stride)
};
__device__ __forceinline__ PairPtrs pair_ptrs(const PairDesc& pd) {
  PairPtrs q;
  q.refP = as_global((const float*)pd.ref.P3); q.refN = as_global((const v4f*)pd.ref.Nc);
  q.curP = as_global((const float*)pd.cur.P3); q.curN = as_global((const v4f*)pd.cur.Nc);
  q.curOm = as_global((const float*)pd.cur.Om); q.curOmN = as_global((const float*)pd.cur.OmN);
  q.zref = as_global((const unsigned*)pd.zref); q.curidx = as_global((const int*)pd.curidx);
  q.refidx0 = as_global(pd.refidx0);
  q.cap = (unsigned)pd.cur.capacity;
  return q;
}
// CUR_DEPTH: without the load of the current point: craw, the raw depth of the candidate's pixel (it arrived with the indices), is kept in its place
template <bool CUR_DEPTH = false>
__device__ __forceinline__ void candidate_load(const PairPtrs& q, int ri, int ci, int nref, int ncur, Candidate& c, unsigned craw = 0u) {
  c.valid = !(ri < 0 || ci < 0 || ri >= nref || ci >= ncur);
  c.ci = ci;
  if constexpr (CUR_DEPTH) c.craw = craw;
  if (c.valid) {
    // 12 + 16 bytes per side; the rest of the pass keeps the (point, curvature) / (normal, -) records it was written for
    c.rP = load_xyz(q.refP, (unsigned)ri);
    if constexpr (!CUR_DEPTH) c.cP = load_xyz(q.curP, (unsigned)ci);
    c.cN = load4(q.curN + (unsigned)ci);
    c.rN = load4(q.refN + (unsigned)ri);
    c.rP.w = c.rN.w; c.cP.w = c.cN.w;
  }
}
template <bool SAME_T, bool SYM, typename ACC>
__device__ __forceinline__ void candidate_consume(const PairDesc& pd, const PairPtrs& q, const AlignParams& ap, const Mat4& Tc, const Mat4& Tl,
                                                  const Candidate& c, const ACC acc, float* cnt /* K, C, inliers */, const float* omNtab /* LDS [3][9] */) {
  if (!c.valid) return;
  cnt[0] += 1.f;
  float3 rp, rn;
  if (!correspondence_test(ap, Tc, c.rP, c.rN, c.cP, c.cN, rp, rn)) return;
  cnt[1] += 1.f;
  float oN[9];
  const int cls = (c.cP.w < pd.cur.clsThr) ? 1 : 2;      // normal_class(): the normal is not zero here (correspondence_test)
  if (pd.cur.OmN) {
#pragma unroll
    for (int k = 0; k < 9; ++k) oN[k] = q.curOmN[om_at(q.cap, (unsigned)c.ci, k)];
  } else {
    // class -> matrix through a 27-float LDS table (row 0 = zero matrix): one broadcast read per entry.  Selecting from the descriptor
    // compiled into a tree of exec-masked branches with a scalar load and a wait inside each, 18 of them per correspondence.
    const float* t = omNtab + 9 * (cls > 2 ? 0 : cls);
#pragma unroll
    for (int k = 0; k < 9; ++k) oN[k] = t[k];
  }
  if (!SAME_T) { rp = iso_point(Tl, c.rP); rn = iso_normal(Tl, c.rN); }   // inner iterations > 0: the linearizer's transform moved on
  float oP[9];
  {
    const size_t cap = (size_t)q.cap;
    const unsigned ci = (unsigned)c.ci;
    if (SYM) {                            // sym6 storage: two 12-byte loads, the lower triangle mirrored in registers (no extra VALU)
      const v3f_raw r0 = *(gptr<const v3f>)(q.curOm + 3u * ci);
      const v3f_raw r1 = *(gptr<const v3f>)(q.curOm + 3u * cap + 3u * ci);
      oP[0] = r0.x; oP[1] = r0.y; oP[2] = r0.z; oP[3] = r0.y; oP[4] = r1.x; oP[5] = r1.y; oP[6] = r0.z; oP[7] = r1.y; oP[8] = r1.z;
    } else {
#pragma unroll
      for (int r3 = 0; r3 < 3; ++r3) {      // three 12-byte loads
        const v3f_raw rw = *(gptr<const v3f>)(q.curOm + (size_t)r3 * 3u * cap + 3u * ci);
        oP[3 * r3] = rw.x; oP[3 * r3 + 1] = rw.y; oP[3 * r3 + 2] = rw.z;
      }
    }
  }
  if (linearize_term(rp, rn, make_float3(c.cP.x, c.cP.y, c.cP.z), make_float3(c.cN.x, c.cN.y, c.cN.z), oP, oN, ap.maxChi2, ap.robust, acc))
    cnt[2] += 1.f;
}
// usePrevTc: the acceptance tests run with the previous outer iteration's transform (Aligner::_computeStatistics re-linearizes
// the finder's existing correspondences at the final transform, aligner.cpp:165-170).
// CUR_DEPTH: the pairs' current clouds own their index images (curidx) and their frames are at hand (cd, CurDepthSrc): the current point is
// recomputed from the pixel's depth instead of loaded -- 2 coalesced bytes per pixel in place of a 12-byte gather per candidate, the same bits.
// STRIP_IDX (with CUR_DEPTH): the current index is ranked from the depths the wave holds and the cloud's strip offsets (cd.strips), curidx is not read.
template <bool SAME_T, bool FULL_H, bool SYM = false, int PPT = kPixPerThread, bool CUR_DEPTH = false, bool STRIP_IDX = false>
__global__ void __launch_bounds__(kAlignBlock, 1) k_corr_linearize(const PairDesc* __restrict__ pairs, AlignParams ap, unsigned tag, int usePrevTc, int ownRefIndex,
                                                                   std::conditional_t<CUR_DEPTH, CurDepthSrc, NoCurDepthSrc> cd) {
  const PairDesc& pd = pairs[blockIdx.y];
  const int N = ap.rows * ap.cols;
  const PairState* stp = pd.state;
  // a converged pair: the loop's passes return (workgroup-uniform, in front of the first barrier); the statistics pass reads its own last epoch
  if (ap.mayFreeze && pair_frozen(stp)) { if (!usePrevTc) return; tag = *as_global(&stp->refTag); }
  const Mat4 Tc = uniform_iso_global(as_global((const float*)(usePrevTc ? stp->invTcorrPrev.m : stp->invTcorr.m)));
  const Mat4 Tl = uniform_iso_global(as_global((const float*)stp->invT.m));
  constexpr int kSlots = LdsAcc<FULL_H>::kSlots;
  __shared__ float lacc[kSlots * kAlignBlock];        // float sums of the thread in column threadIdx.x (bank-conflict free)
#pragma unroll
  for (int k = 0; k < kSlots; ++k) lacc[k * kAlignBlock + threadIdx.x] = 0.f;
  const LdsAcc<FULL_H> sums = { &lacc[threadIdx.x] };
  __shared__ float omNtab[27];
  if (threadIdx.x < 27) omNtab[threadIdx.x] = threadIdx.x < 9 ? 0.f : pd.cur.omN[(threadIdx.x - 9) / 9][(threadIdx.x - 9) % 9];
  __syncthreads();
  float cnt[3] = { 0.f, 0.f, 0.f };
  const int nref = min(*as_global((const int*)pd.ref.count), pd.ref.capacity), ncur = min(*as_global((const int*)pd.cur.count), pd.cur.capacity);
  const int pix0 = blockIdx.x * PPT * kAlignBlock + threadIdx.x;
  const PairPtrs q = pair_ptrs(pd);
  gptr<const uint16_t> craw = nullptr;                    // CUR_DEPTH: the pair's current frame
  int row = 0, col = 0;                                   // CUR_DEPTH: row and column of pixel j
  if constexpr (CUR_DEPTH) { craw = as_global(as_global(cd.raw)[blockIdx.y]); row = pix0 / ap.cols; col = pix0 - row * ap.cols; }
  static_assert(CUR_DEPTH || !STRIP_IDX, "the strip ranks are counted on the depths of the depth source");
  // STRIP_IDX: the offsets of the tile's PPT * 4 strips, one per lane -- lane 4 j + w holds the offset (>= 0) of the strip wave w covers in turn j; the
  // lanes behind them and the strips behind the image hold -1.  One 128-byte load per wave stands for the index stream of its 512 pixels.
  constexpr int kWaves = kAlignBlock / 64;
  static_assert((PPT + 1) * kWaves <= 64, "the strips of a tile and of the turn of look-ahead behind it are lanes of one wave");
  int tileoff = -1;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (STRIP_IDX) {
    const unsigned lane = lane_id(), strip = blockIdx.x * (PPT * kWaves) + lane;
    if (lane < (unsigned)(PPT * kWaves) && strip < ((unsigned)N >> 6)) tileoff = as_global(as_global(cd.strips)[blockIdx.y])[strip];
  }
  auto load_indices = [&](int j, int& ri, int& ci, unsigned& cr) {
    const int pix = pix0 + j * kAlignBlock;
    ri = -1; ci = -1;
    if (j < PPT && pix < N) {
      ri = ownRefIndex ? q.refidx0[(unsigned)pix] : z32_index(q.zref[(unsigned)pix], tag);      // wave-uniform choice
      if constexpr (!STRIP_IDX) ci = q.curidx[(unsigned)pix];
      if constexpr (CUR_DEPTH) cr = craw[(unsigned)pix];    // 2 bytes per pixel, coalesced: what the 12-byte gather of the current point is traded for
    }
  };
  // STRIP_IDX: the index of pixel j, whose raw depth has arrived -- the front end's expression (unproject_integral_body: the strip's offset + the valid
  // pixels of the strip in the lanes below, -1 for a pixel out of range).  Every lane of the wave votes; a turn without pixels (offset -1) votes false.
  // The depth in metres is handed on in cr (its bits): the point of the pixel is computed from it a turn later.
  auto cur_index = [&](int j, int ci, unsigned& cr) {
    if constexpr (STRIP_IDX) {
      const int off = __builtin_amdgcn_readlane(tileoff, kWaves * j + wave);      // wave-uniform
      const float d = raw_to_metres(cr, cd.scale);
      const bool valid = off >= 0 && depth_in_range(d, cd.minD, cd.maxD);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid);
      const int idx = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, (unsigned)off));
      cr = __float_as_uint(d);
      return valid ? idx : -1;
    } else {
      return ci;
    }
  };
  int ri1, ci1, ri2, ci2;
  unsigned cr1 = 0u, cr2 = 0u;
  load_indices(0, ri1, ci1, cr1);
  load_indices(1, ri2, ci2, cr2);
  Candidate nxt;
  ci1 = cur_index(0, ci1, cr1);
  candidate_load<CUR_DEPTH>(q, ri1, ci1, nref, ncur, nxt, cr1);
#pragma unroll 1
  for (int j = 0; j < PPT; ++j) {
    Candidate cur = nxt;
    ci2 = cur_index(j + 1, ci2, cr2);
    candidate_load<CUR_DEPTH>(q, ri2, ci2, nref, ncur, nxt, cr2);      // gathers of pixel j+1: in flight during the arithmetic below
    load_indices(j + 2, ri2, ci2, cr2);                   // indices of pixel j+2
    if constexpr (CUR_DEPTH) {                            // the current point of pixel j = (row, col), as the converter stored it
      if (cur.valid) {
        const float d = STRIP_IDX ? __uint_as_float(cur.craw) : raw_to_metres(cur.craw, cd.scale);
        const Vec3 p = converter_point(cd.iKRt, cd.hasOffset, cd.offset, col, row, d);
        cur.cP.x = p.x; cur.cP.y = p.y; cur.cP.z = p.z;
      }
    }
    candidate_consume<SAME_T, SYM>(pd, q, ap, Tc, Tl, cur, sums, cnt, omNtab);
    if constexpr (CUR_DEPTH) {                            // pixel j + 1 lies 256 pixels on: no division; cols may be below 256, so the wrap is a loop
      col += kAlignBlock;
      while (col >= ap.cols) { col -= ap.cols; ++row; }
    }
  }
  float acc[kAccN];
  acc_from_lds<FULL_H>(lacc, threadIdx.x, cnt[0], cnt[1], cnt[2], acc);
  block_reduce_store<FULL_H>(acc, pd.partials + (size_t)blockIdx.x * kAccN, true);
}

// Latency shape of the fused pass for small launches (sequential odometry: PwnTracker::processFrame aligns one pair at a time).  A pair is
// only 150 workgroups of k_corr_linearize, one wave per SIMD, so the launch lasts as long as one thread's chain of 8 dependent pixels.  Here
// a workgroup has 1024 threads for the same 2048-pixel tile: thread (q, col) = (tid / 256, tid % 256) takes pixels q and q + 4 of column col, so
// the gathers and the arithmetic of all eight pixels of a column run side by side.  The sums stay bit-identical to k_corr_linearize: the
// per-pixel terms are added to the column's LDS accumulator in the same order, pixel 0, 1, ... 7 -- eight ordered turns, a workgroup barrier
// between turns -- and the block reduction is block_reduce_store on the same 256 columns.  (Putting the four threads of a column into one wave
// needs no barriers but makes every wave walk all eight turns and quarters the gathers' coalescing: measured 19 vs 16 us per launch.)
// grid = (ceil(N / 2048), pairs), block = 1024.
constexpr int kLatBlock = 4 * kAlignBlock;
template <bool SAME_T, bool FULL_H, bool SYM = false>
__global__ void __launch_bounds__(kLatBlock) k_corr_linearize_lat(const PairDesc* __restrict__ pairs, AlignParams ap, unsigned tag, int usePrevTc, int ownRefIndex) {
  static_assert(kPixPerThread == 8, "two rounds of four turns");
  const PairDesc& pd = pairs[blockIdx.y];
  const int N = ap.rows * ap.cols;
  const PairState* stp = pd.state;
  // a converged pair: the loop's passes return (workgroup-uniform, in front of the first barrier); the statistics pass reads its own last epoch
  if (ap.mayFreeze && pair_frozen(stp)) { if (!usePrevTc) return; tag = *as_global(&stp->refTag); }
  const Mat4 Tc = uniform_iso_global(as_global((const float*)(usePrevTc ? stp->invTcorrPrev.m : stp->invTcorr.m)));
  const Mat4 Tl = uniform_iso_global(as_global((const float*)stp->invT.m));
  constexpr int kSlots = LdsAcc<FULL_H>::kSlots;
  __shared__ float lacc[kSlots * kAlignBlock];
  __shared__ float lcnt[3 * kAlignBlock];
  __shared__ float omNtab[27];
  const int tid = threadIdx.x, col = tid & (kAlignBlock - 1), q = tid >> 8;
  for (int i = tid; i < kSlots * kAlignBlock; i += kLatBlock) lacc[i] = 0.f;
  if (tid < 3 * kAlignBlock) lcnt[tid] = 0.f;
  if (tid < 27) omNtab[tid] = tid < 9 ? 0.f : pd.cur.omN[(tid - 9) / 9][(tid - 9) % 9];
  const int nref = min(*as_global((const int*)pd.ref.count), pd.ref.capacity), ncur = min(*as_global((const int*)pd.cur.count), pd.cur.capacity);
  const int pix0 = blockIdx.x * kPixPerThread * kAlignBlock + col;
  const PairPtrs pp = pair_ptrs(pd);
  // both pixels' indices, then both pixels' gathers, then both pixels' terms: every load is in flight before the first ordered turn
  int ri[2], ci[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int pix = pix0 + (q + 4 * r) * kAlignBlock;
    ri[r] = -1; ci[r] = -1;
    if (pix < N) {
      ri[r] = ownRefIndex ? pp.refidx0[(unsigned)pix] : z32_index(pp.zref[(unsigned)pix], tag);
      ci[r] = pp.curidx[(unsigned)pix];
    }
  }
  Candidate cand[2];
  candidate_load(pp, ri[0], ci[0], nref, ncur, cand[0]);
  candidate_load(pp, ri[1], ci[1], nref, ncur, cand[1]);
  __syncthreads();                                   // accumulators zeroed, class table written
  float t[2][kAccN], c3[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int k = 0; k < kAccN; ++k) t[r][k] = 0.f;
    c3[r][0] = c3[r][1] = c3[r][2] = 0.f;
    candidate_consume<SAME_T, SYM>(pd, pp, ap, Tc, Tl, cand[r], RegAcc{ t[r] }, c3[r], omNtab);
  }
  const LdsAcc<FULL_H> sums = { &lacc[col] };
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const bool has = c3[r][2] > 0.f;              // linearize_term added this pixel's terms
#pragma unroll 1
    for (int turn = 0; turn < 4; ++turn) {
      if (q == turn) {
        if (has) {
#pragma unroll
          for (int k = 0; k < kAccTerms; ++k) sums.add(k, t[r][k]);
        }
        lcnt[col] += c3[r][0]; lcnt[kAlignBlock + col] += c3[r][1]; lcnt[2 * kAlignBlock + col] += c3[r][2];     // counts: integers, exact in any order
      }
      __syncthreads();
    }
  }
  // the records of the 256 columns (waves 0..3) into the block's
  const bool owns_column = tid < kAlignBlock;
  float acc[kAccN];
  if (owns_column) acc_from_lds<FULL_H>(lacc, tid, lcnt[tid], lcnt[kAlignBlock + tid], lcnt[2 * kAlignBlock + tid], acc);
  block_reduce_store<FULL_H>(acc, pd.partials + (size_t)blockIdx.x * kAccN, owns_column);
}

// CorrespondenceFinder::compute as a per-pixel pair image (compacted on the host in row-major order).
__global__ void __launch_bounds__(256) k_correspondence_image(CloudDev ref, CloudDev cur, const int* __restrict__ refIndex,
                                                              const int* __restrict__ curIndex, AlignParams ap, Mat4 Tc,
                                                              int2* __restrict__ out, int* __restrict__ counters) {
  const int N = ap.rows * ap.cols;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= N) return;
  int2 res = make_int2(-1, -1);
  const int ri = refIndex[pix], ci = curIndex[pix];
  const int nref = min(*ref.count, ref.capacity), ncur = min(*cur.count, cur.capacity);
  if (ri >= 0 && ci >= 0 && ri < nref && ci < ncur) {
    atomicAdd(&counters[0], 1);
    float3 rp, rn;
    float4 rP, rN, cP, cN;
    cloud_get(ref, ri, rP, rN); cloud_get(cur, ci, cP, cN);
    if (correspondence_test(ap, Tc, rP, rN, cP, cN, rp, rn)) res = make_int2(ri, ci);
  }
  out[pix] = res;
}
// Linearizer::update on an explicit list.  grid = ceil(C/(256*4)), block 256.
__global__ void __launch_bounds__(kAlignBlock) k_linearize_list(CloudDev ref, CloudDev cur, const int2* __restrict__ corr, int C,
                                                                AlignParams ap, Mat4 Tl, double* __restrict__ partials) {
  float acc[kAccN];
#pragma unroll
  for (int k = 0; k < kAccN; ++k) acc[k] = 0.f;
  const int nref = min(*ref.count, ref.capacity), ncur = min(*cur.count, cur.capacity);
#pragma unroll
  for (int j = 0; j < kPixPerThread; ++j) {
    const int i = (blockIdx.x * kPixPerThread + j) * kAlignBlock + threadIdx.x;
    if (i >= C) continue;
    const int2 c = corr[i];
    if (c.x < 0 || c.y < 0 || c.x >= nref || c.y >= ncur) continue;
    acc[kAccCorr] += 1.f;
    float4 rP, rN, cP, cN;
    cloud_get(ref, c.x, rP, rN); cloud_get(cur, c.y, cP, cN);
    float oP[9], oN[9];
    load_omegas(cur, c.y, __float_as_int(cN.w) & kClsMask, oP, oN);
    const float3 rp = iso_point(Tl, rP), rn = iso_normal(Tl, rN);
    if (linearize_term(rp, rn, make_float3(cP.x, cP.y, cP.z), make_float3(cN.x, cN.y, cN.z), oP, oN, ap.maxChi2, ap.robust, RegAcc{ acc })) acc[kAccInliers] += 1.f;
  }
  block_reduce_store(acc, partials + (size_t)blockIdx.x * kAccN, true);
}

// ------------------------------------------------------------------------------------------------------------------
// PwnMatcherBase::matchClouds post-alignment score (pwn_tracker/pwn_matcher_base.cpp:153-182): both finder depth images
// -> uint16 millimetres (DepthImage_convert_32FC1_to_16UC1, FLT_MAX -> 0), mask = both > 0, diff = |cur - ref| as float
// BITWISE-ANDed with the float mask 255.0f (that is what cv::Mat `abs(a-b) & mask` does on CV_32F data), inliers =
// mask && diff < threshold, sum of diff.  Every surviving diff is a multiple of 1/64 (or < 2^-120), so the sum is kept
// exactly in 1/64 fixed point with integer atomics -> bitwise reproducible.  out[pair] = {nonZeros, inliers, sum64, tiny}.
struct MatchAcc { unsigned long long nonZeros, inliers; long long sum64; unsigned long long tiny; };
// sum of the masked differences / nonZeros (pwn_matcher_base.cpp:179; 0/0 = NaN like the reference): the float nearest to the exact sum.  That
// sum is exact in 1/64 units; a `tiny` pixel (a difference of 1 mm: bits(1.0f) & bits(255.0f) = 0x03000000) adds 2^-121, which shows when
// nothing else was added, and where the rest lies exactly half-way between two floats (it then rounds up instead of to even).  One expression
// for the host (pwn_hip_match_result) and the device (result records).
__host__ __device__ __forceinline__ float match_reprojection_distance(const MatchAcc& a) {
  long long s64 = a.sum64;
  if (a.tiny && s64 >= (1ll << 24)) {
    const int sh = 40 - __builtin_clzll((unsigned long long)s64);      // bits of s64 below the float's 24
    if ((s64 & ((1ll << sh) - 1)) == (1ll << (sh - 1))) s64 += 1;
  }
  const double sum = s64 ? (double)s64 / 64.0 : (double)a.tiny * 0x1p-121;
  return (float)sum / (float)(int)a.nonZeros;
}
__device__ __forceinline__ unsigned short depth_to_u16(float d, float scale) { return (d < FLT_MAX) ? (unsigned short)(scale * d) : (unsigned short)0; }
// curOwn: the current cloud was not projected (batch path, identity current offset): its depth image is read off the cloud through its
// own index image -- pixel -> point -> z.  With an identity offset the projector's depth is the point's z bit for bit (row 2 of K*R
// is (0, 0, 1), K*t is 0: d = ((0*x + 0*y) + 1*z) + 0*1), and every point lands on its own pixel (see pwn_hip_cloud::idximg).
__global__ void __launch_bounds__(256) k_match_score(const PairDesc* __restrict__ pairs, int n, unsigned refTag, unsigned curTag, float scale,
                                                     float threshold, MatchAcc* __restrict__ out, int curOwn) {
  const PairDesc& pd = pairs[blockIdx.y];
  refTag = pair_ref_tag(pd.state, refTag);
  int nz = 0, inl = 0; long long sum = 0; int tiny = 0;
  const int ncur = min(*pd.cur.count, pd.cur.capacity), nref = min(*pd.ref.count, pd.ref.capacity);
  const Mat4 KRtRef = uniform_iso(pd.state->KRtLast), KRtCur = uniform_iso(pd.state->KRtCur);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float dc = FLT_MAX, dr = FLT_MAX;
    if (curOwn) { const int ci = pd.curidx[i]; if (ci >= 0 && ci < ncur) dc = load_xyz(pd.cur.P3, ci).z; }
    else { const int ci = z32_index(pd.zcur[i], curTag); if (ci >= 0 && ci < ncur) dc = point_depth(KRtCur, load_xyz(pd.cur.P3, ci)); }
    { const int ri = z32_index(pd.zref[i], refTag); if (ri >= 0 && ri < nref) dr = point_depth(KRtRef, load_xyz(pd.ref.P3, ri)); }
    const unsigned short c = depth_to_u16(dc, scale);
    const unsigned short r = depth_to_u16(dr, scale);
    if (c > 0 && r > 0) {
      ++nz;
      const float ad = fabsf((float)c - (float)r);
      const unsigned bits = __float_as_uint(ad) & 0x437F0000u;            // & bits(255.0f)
      const float d = __uint_as_float(bits);
      if (d < threshold) ++inl;
      const unsigned e = bits >> 23;
      if (e >= 128u) sum += (long long)(128u + ((bits >> 16) & 0x7Fu)) << ((e - 128u));   // d * 64 = (128+m7) * 2^(e-128)
      else if (bits) ++tiny;                                               // d < 2^-120: cannot change a float sum >= 1/64
    }
  }
  // wave reduction of the integers, the four waves of the block combined through LDS, then ONE set of atomics per block: the record of a pair is
  // a single 32-byte target, and memory-side atomics on one address serialise (one set per wave from 256 blocks per pair cost a 64-pair launch
  // 0.68 ms -- 5 x what its reads take; integer sums: any order gives the same bits)
  for (int off = 32; off > 0; off >>= 1) {
    nz += __shfl_xor(nz, off, 64); inl += __shfl_xor(inl, off, 64); tiny += __shfl_xor(tiny, off, 64);
    sum += __shfl_xor(sum, off, 64);
  }
  __shared__ long long part[4][4];
  if (lane_id() == 0) { long long* q = part[threadIdx.x >> 6]; q[0] = nz; q[1] = inl; q[2] = sum; q[3] = tiny; }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = part[0][k] + part[1][k] + part[2][k] + part[3][k];
    MatchAcc* o = out + blockIdx.y;
    if (t[0]) atomicAdd(&o->nonZeros, (unsigned long long)t[0]);
    if (t[1]) atomicAdd(&o->inliers, (unsigned long long)t[1]);
    if (t[2]) atomicAdd((unsigned long long*)&o->sum64, (unsigned long long)t[2]);
    if (t[3]) atomicAdd(&o->tiny, (unsigned long long)t[3]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Deterministic final reduction (fixed block order, fp64) + the Gauss-Newton step of Aligner::align
// (pwn_core/aligner.cpp:86-117): H = H_lin + I + 1000 I, dx = ldlt(H) \ (-b), invT = v2t(dx) * invT, and at the
// end of an outer iteration _T = v2t(t2v(invT^-1)) plus the projector matrix of the next reference projection.
// grid = pairs, block = 256.
struct SolveOut { float H[36]; float b[6]; float chi2; int inliers, ncorr, ncand; };
// fixed partition: lane c < kAccN of wave s sums blocks s, s+4, s+8, ... in order; the four wave sums are
// combined in a fixed order -> bitwise reproducible.  blockDim.x must be 256.
__device__ __forceinline__ void reduce_partials(const double* partials, int nblocks, double* sums /*shared[kAccN]*/) {
  __shared__ double part[4][kAccN];
  const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
  if (c < kAccN) {
    double acc = 0.0;
    int b = s;
    // up to kRW independent loads in flight, then the adds in block order (one pair at VGA: 150 records, 38 per wave: ONE memory round trip;
    // with 32 + a remainder loop it was three).  Records past the end are neither loaded nor added: the sum is the same chain as before.
    constexpr int kRW = 40;
    for (; b < nblocks; b += 4 * kRW) {
      double v[kRW];
#pragma unroll
      for (int i = 0; i < kRW; ++i) { const int bb = b + 4 * i; v[i] = (bb < nblocks) ? partials[(size_t)bb * kAccN + c] : 0.0; }
#pragma unroll
      for (int i = 0; i < kRW; ++i) if (b + 4 * i < nblocks) acc += v[i];
    }
    part[s][c] = acc;
  }
  __syncthreads();
  if (threadIdx.x < kAccN) sums[threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
  __syncthreads();
}
__device__ __forceinline__ void assemble_Hb(const double* s, float* H, float* b) {
  // Linearizer.cpp:109-114
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      H[i + 6 * j] = (float)s[kAccHtt + i + 3 * j];
      H[i + 6 * (j + 3)] = (float)s[kAccHtr + i + 3 * j];
      H[(i + 3) + 6 * (j + 3)] = (float)s[kAccHrr + i + 3 * j];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[(i + 3) + 6 * j] = H[j + 6 * (i + 3)];
#pragma unroll
  for (int i = 0; i < 3; ++i) { b[i] = (float)s[kAccBt + i]; b[i + 3] = (float)s[kAccBr + i]; }
}
// the four trace entries of iteration `it`
__device__ __forceinline__ void trace_put(PairState& s, int it, const double* sums) {
  s.chi2[it] = (float)sums[kAccChi2]; s.inliers[it] = (int)sums[kAccInliers]; s.ncorr[it] = (int)sums[kAccCorr]; s.ncand[it] = (int)sums[kAccCand];
}
// reduction only: the block records of one pair -> its H, b and the four scalars.  blockDim.x must be 256
__device__ __forceinline__ void reduce_to_solve_out(const double* partials, int nblocks, SolveOut* o) {
  __shared__ double sums[kAccN];
  reduce_partials(partials, nblocks, sums);
  if (threadIdx.x != 0) return;
  assemble_Hb(sums, o->H, o->b);
  o->chi2 = (float)sums[kAccChi2]; o->inliers = (int)sums[kAccInliers]; o->ncorr = (int)sums[kAccCorr]; o->ncand = (int)sums[kAccCand];
}
// The step is written out in the kernel, on registers with constant indices only.  (Round 3 had it as a pure function returning the new state in a
// struct, for two experiments that evaluated it inside other kernels: the struct cost the kernel 29 VGPRs, 68 bytes of scratch and a 16 KB
// LDS-promoted array, and a 64-pair launch 18 us instead of 10.5 -- found in the v14 kernel trace and undone.)
// last: this is the alignment's final step -- with pd.state_out set (a few pairs: latency path), the pose goes to the page-locked host copy of
// the state as well (the traces go there step by step), and the host needs no copy back of the state.
// tag: the epoch of this outer iteration's reference projection.  At the end of an outer iteration the norms of the step just solved are recorded
// (stepT / stepR, entry `outer`), and under an enabled StopRule the pair may freeze: its update is applied as usual, and with pd.state_out set the
// pose goes to the host copy now, because the launch with `last` set will return for this pair like every other one.
// The terms of one prior at one pair's Linearizer::_T (k_prior_terms writes them, the priors form of the step adds them); valid = 0: the inverse
// of the prior's Jz was refused, the prior is skipped (se3_prior.cpp's `return`), Hp and bp are zeros
constexpr int kPriorTermsWords = 44;
struct PriorTerms { float Hp[36]; float bp[6]; int valid; int pad; };
// What a call with priors hands the step next to the descriptors (PairDesc, PairState and AlignParams keep their layout): pair y of the launch
// carries the records terms[first[y] .. first[y + 1]), in list order.  NoPairPriors is what the plain step takes in its place.
struct PairPriors { const int* first; const PriorTerms* terms; };
struct NoPairPriors {};
// One body for the two kernels below: PRIORS = false is k_solve_update as it was (the priors argument is an empty struct, nothing of it is compiled)
template <bool PRIORS, class Priors>
// (arguments by value, as the kernel takes them: by reference the compiler commuted a dozen additions of k_solve_update)
__device__ __forceinline__ void solve_update(const PairDesc* __restrict__ pairs, AlignParams ap, int nblocks, int outerEnd, int last, unsigned tag,
                                             StopRule stop, Priors priors) {
  const PairDesc& pd = pairs[blockIdx.x];
  if (stop.enabled && pair_frozen(pd.state)) return;      // workgroup-uniform, in front of reduce_partials' barriers
  __shared__ double sums[kAccN];
  reduce_partials(pd.partials, nblocks, sums);
  if (threadIdx.x != 0) return;
  PairState& st = *pd.state;
  PairState* const so = pd.state_out;
  float H[36], b[6];                                                     // registers: every index below is a constant
  assemble_Hb(sums, H, b);
  const int it = st.it;
  if (it < kMaxIter) {
    trace_put(st, it, sums);
    if (so) trace_put(*so, it, sums);
  }
  st.it = it + 1;
#pragma unroll
  for (int d = 0; d < 6; ++d) H[d + 6 * d] = H[d + 6 * d] + 1.0f;        // aligner.cpp:92
#pragma unroll
  for (int d = 0; d < 6; ++d) H[d + 6 * d] = H[d + 6 * d] + 1000.0f;     // aligner.cpp:94
  if constexpr (PRIORS) {                                                // aligner.cpp:97-108, the valid terms in list order
    const int j1 = priors.first[blockIdx.x + 1];
    for (int j = priors.first[blockIdx.x]; j < j1; ++j) {
      const PriorTerms& pt = priors.terms[j];
      if (!pt.valid) continue;
#pragma unroll
      for (int i = 0; i < 36; ++i) H[i] = H[i] + pt.Hp[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] = b[i] + pt.bp[i];
    }
  }
  float nb[6], dx[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) nb[d] = -b[d];
  ldlt_solve6(H, nb, dx);
  Mat4 invT = st.invT;
  set_last_row(invT);
  invT = iso_mul(v2t(dx), invT);
  if (outerEnd) {
    Mat4 T = iso_inverse(invT);
    float v[6];
    t2v(T, v);
    T = v2t(v);
    set_last_row(T);
    st.T = T;
    // fp32, every product and sum rounded on its own, left to right
    const float sT = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx[0], dx[0]), __fmul_rn(dx[1], dx[1])), __fmul_rn(dx[2], dx[2])));
    const float sR = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx[3], dx[3]), __fmul_rn(dx[4], dx[4])), __fmul_rn(dx[5], dx[5])));
    const int oi = st.outer;
    if (oi < kMaxIter) {
      st.stepT[oi] = sT; st.stepR[oi] = sR;
      if (so) { so->stepT[oi] = sT; so->stepR[oi] = sR; }
    }
    st.outer = oi + 1;
    st.refTag = tag;
    const bool freeze = stop.enabled && oi + 1 >= stop.minIterations && sT <= stop.epsT && sR <= stop.epsR;      // false for a NaN
    if (freeze) st.frozen = 1;
    if (so && (last || freeze)) { so->T = T; so->it = it + 1; so->outer = oi + 1; so->frozen = freeze ? 1 : 0; }
    const Mat4 Tinv = iso_inverse(T);
    st.invTcorrPrev = st.invTcorr;
    st.invTcorr = Tinv;
    invT = Tinv;
    Mat4 KRt, iKRt; Mat3 iK;
    projector_matrices(ap.K, iso_mul(T, ap.refOffset), KRt, iKRt, iK);
    st.KRtLast = st.KRt;        // the reference projection of this outer iteration (what the finder's depth image belongs to)
    st.KRt = KRt;
  }
  set_last_row(invT);
  st.invT = invT;
}
__global__ void __launch_bounds__(256) k_solve_update(const PairDesc* __restrict__ pairs, AlignParams ap, int nblocks, int outerEnd, int last, unsigned tag,
                                                      StopRule stop) {
  solve_update<false>(pairs, ap, nblocks, outerEnd, last, tag, stop, NoPairPriors());
}
// The priors form of the step (pwn_hip_align_batch_priors, a sub-batch that holds at least one prior): after the two damping additions it adds the
// valid records k_prior_terms wrote for the pair at this iteration's st.invT, then solves and updates as k_solve_update does
__global__ void __launch_bounds__(256) k_solve_update_priors(const PairDesc* __restrict__ pairs, AlignParams ap, int nblocks, int outerEnd, int last, unsigned tag,
                                                             StopRule stop, PairPriors priors) {
  solve_update<true>(pairs, ap, nblocks, outerEnd, last, tag, stop, priors);
}
// The result record of a pair as it travels between ranks (include/pwn_hip.h: PWN_HIP_RECORD_FLOATS): 64 floats =
//   [0:16] T column-major  [16] chi2 of the last iteration  [17] its inliers  [18] iterations  [19] the caller's pair id
//   [20:30] chi2_i  [30:40] inliers_i  [40:50] C_i  [50:60] K_i (first 10 iterations)  [60] M_ref  [61] M_cur  [62] iterations in the traces
//   [63] 0, or 1 when a projection of the call gave up on a pixel (z32_settle): the library repeats such a call and the records it returns are the
//        repeat's, but a reader that takes the records off the device BEFORE the call has returned (pwn_hip_ctx_set_enqueued_callback) sees the
//        first attempt's and must drop them
// written on the device from the pair's state, so that a gather of records needs no trip through the host.  Counts travel as float
// (exact below 2^24).  grid = pairs, block = 64
// match != nullptr: a record has kMatchRecordFloats words, [64:68] = PwnMatcherBase::MatcherResult's image fields of the pair (nonZeros, outliers,
// inliers, reprojection distance: pwn_matcher_base.cpp:175-181) from its MatchAcc, [68:72] = 0.  block = 64, or 128 for the long records.
constexpr int kRecordFloats = 64, kRecordTrace = 10, kMatchRecordFloats = 72;
// word t < kMatchRecordFloats of pair `pair`'s record (match: its score accumulators, read for t >= kRecordFloats only)
__device__ __forceinline__ float record_word(const PairDesc& pd, int pair, int t, const int* __restrict__ pair_ids, int first_id, const MatchAcc* __restrict__ match) {
  const PairState& st = *pd.state;
  const int it = st.it, m = it < kRecordTrace ? it : kRecordTrace;
  float v = 0.f;
  if (t >= kRecordFloats) {
    const MatchAcc a = match[pair];
    if (t == 64) v = (float)(int)a.nonZeros;
    else if (t == 65) v = (float)((int)a.nonZeros - (int)a.inliers);
    else if (t == 66) v = (float)(int)a.inliers;
    else if (t == 67) v = match_reprojection_distance(a);
  }
  else if (t < 16) v = st.T.m[t];
  else if (t == 16) v = it > 0 ? st.chi2[it - 1] : 0.f;
  else if (t == 17) v = it > 0 ? (float)st.inliers[it - 1] : 0.f;
  else if (t == 18) v = (float)it;
  else if (t == 19) v = (float)(pair_ids ? pair_ids[pair] : first_id + pair);
  else if (t < 30) v = (t - 20 < m) ? st.chi2[t - 20] : 0.f;
  else if (t < 40) v = (t - 30 < m) ? (float)st.inliers[t - 30] : 0.f;
  else if (t < 50) v = (t - 40 < m) ? (float)st.ncorr[t - 40] : 0.f;
  else if (t < 60) v = (t - 50 < m) ? (float)st.ncand[t - 50] : 0.f;
  else if (t == 60) v = (float)*pd.ref.count;
  else if (t == 61) v = (float)*pd.cur.count;
  else if (t == 62) v = (float)m;
  else if (t == 63) v = (float)__hip_atomic_load(pd.fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // 1 = the call's fault word is up (see the layout above)
  return v;
}
__global__ void __launch_bounds__(128) k_pack_records(const PairDesc* __restrict__ pairs, const int* __restrict__ pair_ids, int first_id, float* __restrict__ out,
                                                      const MatchAcc* __restrict__ match) {
  const int t = threadIdx.x, len = match ? kMatchRecordFloats : kRecordFloats;
  if (t >= len) return;
  out[(size_t)blockIdx.x * len + t] = record_word(pairs[blockIdx.x], (int)blockIdx.x, t, pair_ids, first_id, match);
}
// Aligner::_computeStatistics' 6x6 math of one pair per workgroup (pwn_stats.h: the text the host entry points expand), from the H of the extra
// update (so[pair], k_reduce_pairs) and the pair's final transform.  The team of that text is the workgroup's one wave: the independent turns of
// its loops (at most 36) go to lanes, what is serial every lane computes for itself, every array is in LDS (StatsWork): no scratch, and every
// element sees the host's operations in the host's order.  grid = pairs, block = 64
//   record (kPairStatsFloats words): omega[36] column-major, mean[6], translational and rotational eigen ratio, error and inliers of the extra
//   update (the count as float), 1 = computed, 0
struct LaneTeam {
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int size() const { return 64; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};
constexpr int kPairStatsFloats = 48;
struct PairStats { float omega[36]; float mean[6]; float translationalRatio, rotationalRatio; float error, inliers; float computed, pad; };
__global__ void __launch_bounds__(64) k_pair_statistics(const PairDesc* __restrict__ pairs, const SolveOut* __restrict__ so, PairStats* __restrict__ out) {
  __shared__ StatsWork ws;
  __shared__ PairStats rec;
  const SolveOut& s = so[blockIdx.x];
  const Mat4 T = pairs[blockIdx.x].state->T;
  compute_statistics(LaneTeam(), s.H, T, rec.mean, rec.omega, &rec.translationalRatio, &rec.rotationalRatio, ws);
  if (threadIdx.x == 0) { rec.error = s.chi2; rec.inliers = (float)s.inliers; rec.computed = 1.f; rec.pad = 0.f; }
  __syncthreads();
  if (threadIdx.x < kPairStatsFloats) reinterpret_cast<float*>(out + blockIdx.x)[threadIdx.x] = reinterpret_cast<const float*>(&rec)[threadIdx.x];
}
// The prior terms of one pair per workgroup (pwn_stats.h: prior_terms, the text pwn_hip_prior_terms and prior_accumulate expand on the host), for each
// prior of the pair in list order, at the pair's Linearizer::_T as the last step stored it (after set_last_row, aligner.cpp:86).  The
// 24 error evaluations of the numeric Jacobians, the rows of the elimination and the 36 elements of each product go to lanes; every array is in
// LDS (PriorWork).  A pair without priors, and a frozen pair under an enabled StopRule, returns at once.  grid = pairs, block = 64
//   first: per pair of the launch, as for PairPriors; priors: the device copies; terms: one record per prior
//   invT != nullptr (pwn_hip_debug_prior_terms_eval): pair y takes invT[y] and `pairs` is not read
// The team is LaneTeam under a name of its own: with one team type for both kernels the two shared gauss_jordan_inverse<LaneTeam>, and the
// compiler then laid out k_pair_statistics' blocks differently (same operations, other code).  A type of its own keeps that kernel's code as it was.
struct PriorLaneTeam : LaneTeam {};
__global__ void __launch_bounds__(64) k_prior_terms(const PairDesc* __restrict__ pairs, const int* __restrict__ first, const PriorHost* __restrict__ priors,
                                                    PriorTerms* __restrict__ terms, const Mat4* __restrict__ invT, StopRule stop) {
  const int j0 = first[blockIdx.x], j1 = first[blockIdx.x + 1];
  if (j0 >= j1) return;
  if (!invT && stop.enabled && pair_frozen(pairs[blockIdx.x].state)) return;      // workgroup-uniform
  __shared__ PriorWork ws;
  __shared__ PriorHost pr;
  __shared__ Mat4 T;
  __shared__ PriorTerms rec;
  static_assert(sizeof(PriorHost) % 4 == 0 && sizeof(PriorTerms) == 4 * kPriorTermsWords, "records are copied word by word");
  constexpr int kPriorWords = (int)(sizeof(PriorHost) / 4);
  const float* Tsrc = invT ? invT[blockIdx.x].m : pairs[blockIdx.x].state->invT.m;
  if (threadIdx.x < 16) T.m[threadIdx.x] = Tsrc[threadIdx.x];
  for (int j = j0; j < j1; ++j) {
    __syncthreads();      // the record of the prior before this one is out, T is in
    for (int w = threadIdx.x; w < kPriorWords; w += 64) reinterpret_cast<unsigned*>(&pr)[w] = reinterpret_cast<const unsigned*>(priors + j)[w];
    __syncthreads();
    const bool valid = prior_terms(PriorLaneTeam(), pr, T, rec.Hp, rec.bp, ws);
    if (!valid && threadIdx.x < 42) reinterpret_cast<float*>(&rec)[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) { rec.valid = valid ? 1 : 0; rec.pad = 0; }
    __syncthreads();
    if (threadIdx.x < kPriorTermsWords) reinterpret_cast<unsigned*>(terms + j)[threadIdx.x] = reinterpret_cast<const unsigned*>(&rec)[threadIdx.x];
  }
}
// The closure record (include/pwn_hip.h: PWN_HIP_CLOSURE_RECORD_FLOATS): [0:72] the match record word for word, [72:119] the pair's PairStats
// up to its "computed" word (stats == nullptr: the call ran no iteration, zeros), [119:128] 0.  grid = pairs, block = 128
constexpr int kClosureRecordFloats = 128, kClosureStatsWords = 47;
__global__ void __launch_bounds__(128) k_pack_closure_records(const PairDesc* __restrict__ pairs, const int* __restrict__ pair_ids, int first_id, float* __restrict__ out,
                                                              const MatchAcc* __restrict__ match, const PairStats* __restrict__ stats) {
  const int t = threadIdx.x;
  float v = 0.f;
  if (t < kMatchRecordFloats) v = record_word(pairs[blockIdx.x], (int)blockIdx.x, t, pair_ids, first_id, match);
  else if (stats && t < kMatchRecordFloats + kClosureStatsWords) v = reinterpret_cast<const float*>(stats + blockIdx.x)[t - kMatchRecordFloats];
  out[(size_t)blockIdx.x * kClosureRecordFloats + t] = v;
}
// one record per pair (Aligner::_computeStatistics' 11th update).  grid = pairs, block = 256
__global__ void __launch_bounds__(256) k_reduce_pairs(const PairDesc* __restrict__ pairs, int nblocks, SolveOut* __restrict__ out) {
  reduce_to_solve_out(pairs[blockIdx.x].partials, nblocks, out + blockIdx.x);
}
// one record (pwn_hip_linearize).  grid = 1, block = 256
__global__ void __launch_bounds__(256) k_reduce_only(const double* __restrict__ partials, int nblocks, SolveOut* __restrict__ out) {
  reduce_to_solve_out(partials, nblocks, out);
}

}  // namespace pwnhip
