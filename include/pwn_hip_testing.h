/* pwn_hip_testing.h -- entry points that exist for the test suite only.  NOT part of the drop-in boundary (include/pwn_hip.h): a
 * reference-side binding never calls them.  They are exported by the same library so that the tests exercise the product build. */
#ifndef PWN_HIP_TESTING_H
#define PWN_HIP_TESTING_H
#include "pwn_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The converter's integral-image kernels hand the running sums of a strip to the strip on its right through tagged words,
 * polled with a bound: a word that never arrives raises a fault flag and the convert call returns PWN_HIP_ERR_LAUNCH ("strip hand-over
 * timed out") instead of hanging the device.  This call makes that happen on purpose: the word (strip, band, chain) of every frame of
 * rows x * images is withheld and the poll bound is lowered to spin_limit polls (0 = the default).  strip < 0 switches the hook off.
 * While the hook is on every convert call of the context fails; the word index is the same in both kernels that hand over
 * (k_unproject_integral, k_unproject_integral_rows: 10 planes x band rows chains per (strip, band)). */
int pwn_hip_debug_withhold_carry(pwn_hip_ctx* ctx, int strip, int band, int chain, int rows, int spin_limit);
/* spin_limit < 0: |spin_limit| polls and ONE disturbed launch only -- the hook switches itself off when that launch has timed out, so
 * that the library's own recovery can be watched: a convert call (and the one-submission step) whose launch timed out is made again, once,
 * before an error is reported (the words are epoch-tagged: a failed launch leaves nothing behind).  Number of such repeats so far: */
int pwn_hip_debug_convert_retries(pwn_hip_ctx* ctx, int* retries);

/* An alignment does not project a cloud where the cloud's own index image (the one DepthImageConverter::compute produced for it) is known
 * to be what that projection returns: same camera matrix, image size and range, identity pose (the current cloud always; the reference cloud
 * in the first outer iteration of an identity guess).  enabled = 0 makes every alignment of the context project everything, so that tests can
 * hold the shortcut against the projection it replaces; 1 (the default) switches it back on. */
int pwn_hip_debug_set_index_shortcut(pwn_hip_ctx* ctx, int enabled);

/* PinholePointProjector::project (pinholepointprojector.cpp:54-63) keeps the nearest point per pixel, ties to the lowest index.  The aligner's
 * projection kernel settles two points of one projection that meet in a pixel with a compare-and-swap loop; a thread that has not settled after
 * `rounds` rounds (default 4096: tens of thousands of points in one pixel) raises the call's fault word, and the library repeats the whole call
 * with a two-pass projection (nearest depth per pixel, then the lowest index among the points that have it) that needs no loop -- the images are
 * the reference's either way.  rounds = 0 makes every collision give up, so that the repeat can be watched; rounds < 0 restores the default.
 * Number of calls repeated so far: */
int pwn_hip_debug_set_settle_guard(pwn_hip_ctx* ctx, int rounds);
int pwn_hip_debug_projection_fallbacks(pwn_hip_ctx* ctx, int* calls);
/* How often the calling thread has waited for one of the context's streams so far (every such wait of the library is counted, whatever the
 * reason: the end of a call, a workspace or descriptor array that has to grow, a cloud's planes that are dropped).  The difference across a call
 * is the number of host waits of that call: what "one submission, one wait" means for the one-call entry points. */
int pwn_hip_debug_host_waits(pwn_hip_ctx* ctx, int* waits);
/* The aligner's projection launch on injected clouds: clouds[i], i < n, projected under the projector transform transforms[16 i ..] (column-major,
 * what pwn_hip_project takes); camera matrix, image size and range from p, as an alignment takes them.  The launch is the function an alignment
 * calls, with its grid, its choice of kernel by n (fewer than 8 pairs: one point per thread; from 8 on: four) and the context's settle guard,
 * through the context's own pair descriptors, states and z-buffer slots (pair i uses slot i).  which = 0: the reference side (its buffers, its
 * matrix); which = 1: the current side.  The epoch tag comes from the context's running supply, so the slots are NOT cleared first.  form = 0:
 * what an alignment of n pairs launches; form = 1: the two-pass projection of a repeated call.  index_out / depth_out (host or device, either
 * may be NULL) receive every pair's images, n x rows x cols, read from the pair's words and points as pwn_hip_align_images reads slot 0's:
 * empty pixels -1 / FLT_MAX.  *gave_up = 1 if a thread's settle loop ran out of rounds (the images are then not the reference's; the call is
 * not repeated), else 0.  The images of the context's last alignment are no longer available afterwards.  Refused with
 * PWN_HIP_ERR_INVALID_ARGUMENT, nothing written: a null ctx, p, clouds, transforms, gave_up or cloud; n outside 1 .. max_batch; which or form
 * outside {0, 1}; min_distance < 0; a cloud of another context or of more than 2^21 points; with PWN_HIP_ERR_CAPACITY: an image larger than
 * the context's. */
int pwn_hip_debug_project_pairs(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* clouds, const float* transforms,
                                int which, int form, int* index_out, float* depth_out, int* gave_up);

/* The one-call step (pwn_hip_convert_align_batch_u16) aligns clouds it has just converted from frames that are still on the device.  Where every
 * pair of a sub-batch takes the current cloud's own index image (see pwn_hip_debug_set_index_shortcut), the frames are the caller's resident
 * uint16 frames, and the sub-batch is large enough for the throughput shape of the fused correspondence + linearize pass (more workgroups than
 * compute units), that pass does not load the current points: it recomputes each from its pixel's raw depth, the converter's expression, the same
 * bits.  Number of sub-batches of the context's last batch alignment that ran this way (0 after every other alignment call, after the _scaled
 * step, and after a step on host frames): */
int pwn_hip_debug_cur_depth_sub_batches(pwn_hip_ctx* ctx, int* sub_batches);
/* Of those sub-batches, the ones whose fused pass did not load the current clouds' index images either: where cols is a multiple of 64 and the
 * conversions of the sub-batch's current frames ran the single-pass strip front end (launches of at least 16 frames), every current cloud keeps
 * that front end's table of strip offsets, and a pixel's index is the table word of its 64-column strip plus its rank among the strip's valid
 * depths -- the converter's expression, the same bits.  0 wherever the hook above reads 0, for other widths and for smaller launches: */
int pwn_hip_debug_strip_index_sub_batches(pwn_hip_ctx* ctx, int* sub_batches);
/* The expression that pass evaluates, on the host (no GPU, no context): for every pixel (r, c) of a rows x cols uint16 frame with
 * 0 <= index_image[r][c] < capacity, points[3 * index] = the point the converter stores for that pixel -- PinholePointProjector::unProject of
 * (c, r, depth_scale * raw), then p's sensor offset if it is not the identity.  Other entries of points are left alone. */
int pwn_hip_debug_converter_points(const pwn_hip_converter_params* p, int rows, int cols, const uint16_t* raw, float depth_scale, const int* index_image,
                                   int capacity, float* points);

/* The converter's stats pass (the kernel DepthImageConverter::compute runs after its integral image) on windows the caller supplies:
 * integral = nframes x [10][rows][cols] planes (x, y, z, n, xx, xy, xz, yy, yz, zz), index_image / interval_image = nframes x [rows][cols];
 * clouds[i] holds the points (pwn_hip_cloud_upload) index image i refers to.  Normals, curvature, information matrices (and stats with
 * keep_stats) are written as a convert call writes them; read them back with pwn_hip_cloud_download / pwn_hip_cloud_download_stats.
 * 1 <= nframes <= max_batch; from 8 frames on the kernel takes its XCD-aware placement, as in a convert call. */
int pwn_hip_debug_stats_from_integral(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, int rows, int cols, int nframes, const float* integral,
                                      const int* index_image, const int* interval_image, pwn_hip_cloud* const* clouds, int keep_stats);
/* The same pass as a lean convert call runs it (the batch calls, the tracker, the fused step): the integral image in the grouped form and
 * no interval image and no points -- the kernel recomputes both from the depth frame.  integral = nframes x 10 N floats, N = rows * cols of
 * this call (not of the context), per frame three arrays of records: (x y z n) at float 0, (xx xy xz yy) at float 4 N, (yz zz) at float 8 N,
 * one record per pixel in each array, pixels in row-major order.  frames[i] = rows x cols host image, float32 metres (depth_scale == 0) or
 * uint16 raw values (depth_scale > 0: metres = depth_scale * raw, raw 0 = 0 metres), as pwn_hip_debug_front_end takes them.  A pixel with
 * index >= 0 must hold a depth the front end would have accepted: the kernel does not repeat the range test.  The clouds need capacity only
 * (every index < capacity, else the call is refused); afterwards cloud i reports max(index image i) + 1 points, written by the kernel. */
int pwn_hip_debug_stats_from_integral_lean(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, int rows, int cols, int nframes, const float* integral,
                                           const int* index_image, const void* const* frames, float depth_scale, pwn_hip_cloud* const* clouds,
                                           int keep_stats);
/* The converter's front end (everything a convert call launches before its stats pass) on the caller's frames, and what it wrote:
 * frames[i] = rows x cols float32 metres (depth_scale == 0) or uint16 raw values (depth_scale > 0: metres = depth_scale * raw), host or device
 * pointers, all of one kind.  path chooses the launch sequence whatever nframes is: PWN_HIP_FRONT_END_LATENCY (k_row_count, k_row_offsets,
 * k_unproject_integral_rows, k_integral_cols: what a call of fewer than 16 frames per launch takes) or PWN_HIP_FRONT_END_SINGLE_PASS (k_strip_count
 * or k_strip_count_any, k_row_offsets, k_unproject_integral) -- the function a convert call runs, with its grids, its choice of the counting
 * kernel by width and pointer alignment and its hand-over epoch; the stats pass is not launched.  1 <= nframes <= max_batch (frame i uses
 * workspace slot i).  Per frame: integral_out nframes x [10][rows][cols], index_out nframes x [rows][cols], rowoff_out nframes x [rows]
 * (latency: first point index of every row) or nframes x [rows][strips of 64 columns] (single pass: of every (row, strip)).  lean = 0: the
 * interval images go to interval_out and clouds[i] holds the points (normals, curvature and matrices zero).  lean = 1: the front end stores
 * neither; interval_out must be NULL and the clouds hold 0 points afterwards; the planes are written as with lean = 0 (a configuration no
 * shipped call uses any more: it exists for the tests).  lean = 2 (PWN_HIP_FRONT_END_LEAN_GROUPED), the setting of every lean convert call:
 * as lean = 1, but the launches are the grouped ones (k_unproject_integral_grouped; the grouped write-out of k_unproject_integral_rows and the
 * grouped mode of k_integral_cols) and integral_out receives each frame's 10 N floats as the slot stores them, nothing rearranged, N = rows *
 * cols of this call (not of the context): three arrays of records, (x y z n) at float 0, (xx xy xz yy) at float 4 N, (yz zz) at float 8 N,
 * one record per pixel in each array, pixels in row-major order.  Any other value of lean is refused and the outputs stay untouched.  A
 * hand-over time-out returns PWN_HIP_ERR_LAUNCH with a convert call's message (the call is not repeated). */
enum { PWN_HIP_FRONT_END_LATENCY = 0, PWN_HIP_FRONT_END_SINGLE_PASS = 1 };
enum { PWN_HIP_FRONT_END_LEAN_OFF = 0, PWN_HIP_FRONT_END_LEAN_PLANES = 1, PWN_HIP_FRONT_END_LEAN_GROUPED = 2 };
int pwn_hip_debug_front_end(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const void* const* frames, float depth_scale, int nframes, int rows,
                            int cols, int path, int lean, pwn_hip_cloud* const* clouds, float* integral_out, int* index_out, int* interval_out,
                            int* rowoff_out);
/* The eigensolver's three trig values (theta = atan2(y, x) / 3, cos theta, sin theta as floats) evaluated on the device for n host arguments
 * y = sqrt(q) >= 0, x = half_b: the lines of the stats kernel's eigensolver that compute them (one macro, expanded in both places). */
int pwn_hip_debug_trig_eval(pwn_hip_ctx* ctx, int n, const float* y, const float* x, float* theta, float* cos_theta, float* sin_theta);
/* The kernel behind pwn_hip_closure_batch_records' statistics words (k_pair_statistics, as shipped, one system per workgroup, through the
 * context's own pair arrays, which grow to n) on n injected systems: H n x 36 (column-major Linearizer::H() without damping), T n x 16
 * (column-major Aligner::T()); out n x 44 = omega[36] column-major, mean[6], the translational and the rotational eigen ratio -- what
 * pwn_hip_compute_statistics returns for the same system on the host. */
int pwn_hip_debug_statistics_eval(pwn_hip_ctx* ctx, int n, const float* H, const float* T, float* out);
/* The kernel behind pwn_hip_align_batch_priors' prior terms (k_prior_terms, as shipped, one pair per workgroup) on n injected pairs: invT
 * n x 16 (column-major Linearizer::_T), pair i carries priors[first[i] .. first[i + 1]) (first: n + 1 ints as in pwn_hip_pair_priors); out
 * first[n] x 44 words = Hp[36] column-major, bp[6], valid (an int), 0 -- per prior what pwn_hip_prior_terms returns for (invT[i], prior) on
 * the host. */
int pwn_hip_debug_prior_terms_eval(pwn_hip_ctx* ctx, int n, const float* invT, const int* first, const pwn_hip_prior* priors, float* out);

/* A cloud's Gaussian vector (Cloud::gaussians()) set from host arrays in the layout pwn_hip_cloud_download_gaussians returns: mean n x 3,
 * cov n x 9 (column-major 3x3), info_vec n x 3, info n x 9, flags n (1 = moments valid, 2 = information form valid; any of 0..3).  The
 * records and flags are stored as given -- a field its flag does not declare valid is carried along, never read.  0 <= n <= capacity; n need
 * not be the cloud's size (Cloud::add's shorter Gaussian vector, Merger::merge's tail, VoxelCalculator's "sizes must match" rule).  Bad
 * arguments (null pointers with n > 0, n outside the range, flags outside 0..3, a cloud of another context) are refused with
 * PWN_HIP_ERR_INVALID_ARGUMENT and nothing is written.  A later upload or conversion into the cloud does not keep them in step: set them after. */
int pwn_hip_debug_cloud_set_gaussians(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, int n, const float* mean, const float* cov, const float* info_vec,
                                      const float* info, const int* flags);

/* The Gaussian vector becomes the first n records of the cloud's Gaussian arrays as they are, nothing written (0 <= n <= capacity; the arrays
 * must exist: a cloud that has had Gaussians).  Lets a test read records beyond the vector's end, to see that a call left them alone. */
int pwn_hip_debug_cloud_expose_gaussians(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, int n);

/* pwn_hip_manifold_image takes its clouds in chunks of whole clouds with at most 2^25 points and carries the image from chunk to chunk.  This
 * sets the bound to `points` (<= 0: back to 2^25), so that a small list runs as several chunks; a cloud above the bound is refused as a cloud
 * above 2^25 is (PWN_HIP_ERR_CAPACITY). */
int pwn_hip_debug_set_manifold_chunk(pwn_hip_ctx* ctx, int points);

/* How k_gaussians_batch (pwn_hip_convert_batch_ex with Gaussians) stores its records: 0 = every lane its own 96-byte record, 1 = staged in LDS
 * and written as consecutive dwords, anything else = back to the library's choice.  Same bits either way; for the timing tool and the test that
 * says so. */
int pwn_hip_debug_set_gaussian_stores(pwn_hip_ctx* ctx, int staged);

#ifdef __cplusplus
}
#endif
#endif
