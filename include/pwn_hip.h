/*
 * pwn_hip.h -- C-ABI of the MI355X (gfx950) PWN dense-registration path.
 *
 * This is the drop-in boundary behind the reference's pwn_core C++ API
 * (grisetti/g2o_frontend, g2o_frontend/pwn_core/).  Every entry point names the reference
 * method it replaces (file:line relative to g2o_frontend/pwn_core/ unless a directory is given).
 * The in-tree precedent for a C-style device boundary is pwn_cuda/cudaaligner.h:59-80
 * (createContext / initComputation / simpleIteration / getHb); the shape below follows it:
 * opaque context, plain pointers and sizes, int status codes, nothing thrown across the ABI.
 *
 * Conventions
 *   - matrices: COLUMN-MAJOR float (Eigen default, as pwn_cuda/cualigner.cpp:56-67 passes them);
 *     3x3 = 9 floats, 4x4 isometries = 16 floats, 6x6 = 36 floats.
 *   - images: row-major [rows][cols]; index images are int32 (-1 = empty), depth images float32
 *     metres (pwn_typedefs.h:57-62).
 *   - data pointers may be HOST or DEVICE memory; the library detects which
 *     (hipPointerGetAttributes) and copies accordingly.  Parameter structs, result structs and
 *     handle arrays are always host memory.
 *   - a context is bound to one GPU; calls on one context must be serialised by the caller
 *     (the reference objects are not re-entrant either: aligner.cpp:60-76 mutates the shared
 *     projector).  Use one context per (GPU, host thread).
 *   - all calls are synchronous with respect to the host unless noted: outputs are valid on return.
 *   - status: 0 = ok; otherwise one of pwn_hip_status; pwn_hip_last_error_string() gives detail.
 */
#ifndef PWN_HIP_H
#define PWN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PWN_HIP_MAX_ITERATIONS 64

typedef enum pwn_hip_status {
  PWN_HIP_OK = 0,
  PWN_HIP_ERR_INVALID_ARGUMENT = 1,
  PWN_HIP_ERR_NO_DEVICE = 2,
  PWN_HIP_ERR_ALLOCATION = 3,      /* cf. pwn_cuda Operation::Allocation      (cudaaligner.h:11) */
  PWN_HIP_ERR_COPY = 4,            /* cf. CopyToDevice / CopyFromDevice        (:13-14) */
  PWN_HIP_ERR_LAUNCH = 5,          /* cf. KernelLaunch                          (:15) */
  PWN_HIP_ERR_CAPACITY = 6         /* image / batch / cloud larger than the context or handle allows */
} pwn_hip_status;

typedef struct pwn_hip_ctx pwn_hip_ctx;       /* one per (GPU, host thread) */
typedef struct pwn_hip_cloud pwn_hip_cloud;   /* device-resident pwn::Cloud (cloud.h:20-187) */

/* Parameters of DepthImageConverterIntegralImage and its four collaborators
 * (depthimageconverter.h:29-32).  Defaults = the class defaults of the reference. */
typedef struct pwn_hip_converter_params {
  float K[9];                            /* PinholePointProjector::setCameraMatrix (pinholepointprojector.h:51) */
  float min_distance;                    /* PointProjector::setMinDistance (pointprojector.h:62), default 0.01 (pointprojector.cpp:9) */
  float max_distance;                    /* setMaxDistance (:76), default 6.0 (pointprojector.cpp:10) */
  float world_radius;                    /* StatsCalculatorIntegralImage::setWorldRadius, 0.1 (statscalculatorintegralimage.cpp:7) */
  int   min_image_radius;                /* setMinImageRadius, 10 (:9) */
  int   max_image_radius;                /* setMaxImageRadius, 30 (:8) */
  int   min_points;                      /* setMinPoints, 50 (:10) */
  float stats_curvature_threshold;       /* setCurvatureThreshold, 0.02 (:11) */
  float point_info_curvature_threshold;  /* PointInformationMatrixCalculator::setCurvatureThreshold, 0.02 (informationmatrixcalculator.h:109) */
  float normal_info_curvature_threshold; /* NormalInformationMatrixCalculator, 0.02 (informationmatrixcalculator.h:144) */
  float point_flat_diag[3];              /* diag(1000,1,1) (informationmatrixcalculator.h:107) */
  float point_nonflat_diag[3];           /* diag(1,1,1) (:108); replaced by 1/eigenvalues at use (.cpp:27-29) */
  float normal_flat_diag[3];             /* diag(100,100,100) (:142) */
  float normal_nonflat_diag[3];          /* diag(1,1,1) (:143) */
  float sensor_offset[16];               /* third argument of DepthImageConverter::compute (depthimageconverter.h:47) */
} pwn_hip_converter_params;

/* Parameters of PinholePointProjector + CorrespondenceFinder + Linearizer + Aligner as the
 * callers set them before Aligner::align() (pwn_simple_aligner.cpp:214-269, pwn_matcher_base.cpp:107-135). */
typedef struct pwn_hip_aligner_params {
  float K[9];                             /* projector camera matrix */
  float min_distance, max_distance;       /* projector range */
  int   rows, cols;                       /* PointProjector::setImageSize / CorrespondenceFinder::setImageSize (correspondencefinder.h:211-218) */
  float inlier_distance_threshold;        /* 0.5  (correspondencefinder.cpp:10) */
  float inlier_normal_angular_threshold;  /* cos(pi/6) (:12) */
  float flat_curvature_threshold;         /* 0.02 (:13) */
  float inlier_curvature_ratio_threshold; /* 1.3  (:14) */
  float inlier_max_chi2;                  /* 9e3  (linearizer.cpp:13) */
  int   robust_kernel;                    /* 1    (linearizer.cpp:14) */
  int   outer_iterations;                 /* 10   (aligner.cpp:19) */
  int   inner_iterations;                 /* 1    (aligner.cpp:20) */
  float reference_sensor_offset[16];      /* Aligner::setReferenceSensorOffset (aligner.h:168-171) */
  float current_sensor_offset[16];        /* Aligner::setCurrentSensorOffset (aligner.h:187-190) */
  float initial_guess[16];                /* Aligner::setInitialGuess (aligner.h:130-133) */
} pwn_hip_aligner_params;

/* What Aligner exposes after align(): T() (aligner.h:115), error() (:320), inliers() (:326),
 * totalTime() (:332), plus the per-iteration counters SURVEY.md §8(d) asks the kernels to emit. */
typedef struct pwn_hip_align_result {
  float T[16];                                 /* Aligner::T(): current -> reference frame */
  float error;                                 /* value of the LAST in-loop Linearizer::update (aligner.cpp:124) */
  int   inliers;                               /* aligner.cpp:125 */
  int   iterations;                            /* outer*inner linearizer updates executed */
  float total_time_ms;                         /* GPU time of this alignment (batch: batch time / n) */
  float chi2[PWN_HIP_MAX_ITERATIONS];          /* Linearizer::error() after each update */
  int   iter_inliers[PWN_HIP_MAX_ITERATIONS];  /* Linearizer::inliers() */
  int   iter_correspondences[PWN_HIP_MAX_ITERATIONS]; /* C_i: CorrespondenceFinder::numCorrespondences() */
  int   iter_candidates[PWN_HIP_MAX_ITERATIONS];      /* K_i: pixels with both index images >= 0 */
  int   n_reference, n_current;                /* M_r, M_c */
} pwn_hip_align_result;

/* PwnMatcherBase::MatcherResult image fields (pwn_tracker/pwn_matcher_base.h:13-22), what PwnCloser::matchFrames
 * thresholds (pwn_tracker/pwn_closer.cpp:56-58,138-141). */
typedef struct pwn_hip_match_result {
  int   image_non_zeros;               /* pixels where both finder depth images are > 0 after the uint16-mm conversion */
  int   image_outliers;                /* non_zeros - inliers */
  int   image_inliers;                 /* masked pixels whose (bit-masked) |depth difference| < threshold */
  float image_reprojection_distance;   /* sum of the differences / non_zeros */
} pwn_hip_match_result;

/* What Aligner::_computeStatistics leaves behind (aligner.cpp:127,152-199): omega() (aligner.h:314), the eigen-ratio
 * validity measures compared with rotational/translationalMinEigenRatio (aligner.cpp:128-129), the remapped mean. */
typedef struct pwn_hip_align_statistics {
  float mean[6];                       /* (t, q) of the solution as reconstructed from the sigma points */
  float omega[36];                     /* column-major 6x6 information matrix of the estimate */
  float translational_eigen_ratio;
  float rotational_eigen_ratio;
  float H[36];                         /* Linearizer::H() of the extra update at the final transform (what the statistics start from) */
  float b[6];
  float error;                         /* Linearizer::error() / inliers() of that extra update (aligner.cpp:168 overwrites the */
  int   inliers;                       /* linearizer's values, not the Aligner's cached ones) */
} pwn_hip_align_statistics;

/* Aligner::addRelativePrior / addAbsolutePrior (aligner.h:342-361, se3_prior.h) */
typedef struct pwn_hip_prior {
  int   kind;                     /* 0 = SE3RelativePrior, 1 = SE3AbsolutePrior */
  float mean[16];                 /* prior mean (column-major isometry) */
  float reference_transform[16];  /* SE3AbsolutePrior::referenceTransform; ignored for relative priors */
  float information[36];          /* column-major 6x6 */
} pwn_hip_prior;

/* ------------------------------------------------------------------ context ------------------ */
/* cf. pwn_cuda createContext(AlignerContext**, maxRef, maxCur, rows, cols) (cudaaligner.h:59).
 * max_batch = largest number of frames (convert_batch) / pairs (align_batch) per call. */
int pwn_hip_ctx_create(pwn_hip_ctx** ctx, int device, int max_rows, int max_cols, int max_batch);
int pwn_hip_ctx_destroy(pwn_hip_ctx* ctx);                       /* cf. destroyContext (cudaaligner.h:61) */
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the context's own stream */
int pwn_hip_ctx_set_stream(pwn_hip_ctx* ctx, void* hip_stream);
int pwn_hip_ctx_synchronize(pwn_hip_ctx* ctx);
/* Ordering against a stream of the caller (hip_stream: a hipStream_t, NULL = the legacy default stream): everything the context queues from
 * now on runs after the work that stream holds now.  The context runs its kernels on non-blocking streams of its own, so device buffers that
 * the caller's streams touch are NOT ordered against it by themselves.  Two cases need this call:
 *   - a device buffer the context WRITES call after call (the `records` of the *_records entry points) is still being READ on the caller's
 *     stream (an all-gather of step k while step k+1 packs its records): call it after queueing the reader, before the next writing call;
 *   - a device buffer the caller's stream WRITES (a broadcast that receives a flat cloud, a kernel that fills frames) is READ by the next call
 *     (pwn_hip_cloud_import, convert*): call it after queueing the writer.
 * The other direction needs nothing: every call is complete on return (outputs valid), pwn_hip_copy_async excepted (see there). */
int pwn_hip_ctx_wait_stream(pwn_hip_ctx* ctx, void* hip_stream);
/* The other direction: what the caller queues on `hip_stream` from now on runs after everything the context has queued so far.  With
 * pwn_hip_ctx_set_enqueued_callback this lets a collective that sends a call's device `records` be queued while the call's kernels still run. */
int pwn_hip_ctx_signal_stream(pwn_hip_ctx* ctx, void* hip_stream);
/* fn(user) is called on the calling thread by every alignment call of the context (pwn_hip_align_batch*, pwn_hip_match_batch*,
 * pwn_hip_convert_align_batch_u16 with n > 0; pwn_hip_align and pwn_hip_align_with_priors*, with priors or without) after ALL device work
 * of the call has been queued -- records packed, copies back queued -- and before the call waits for it.  The reference's closer loop (pwn_tracker/pwn_closer.cpp:85-111) is sequential; on a GPU the host's share of a step
 * (queueing the exchange of the results, fetching and replicating the next `current` cloud) would otherwise run with the device idle between two
 * calls.  Inside fn: other streams and other contexts freely; on THIS context only pwn_hip_ctx_signal_stream, pwn_hip_ctx_wait_stream,
 * pwn_hip_convert_export_begin / _end, pwn_hip_convert_scaled_begin / pwn_hip_convert_end -- no call that converts, aligns or waits on it.  The
 * results the call returns (and host `records`) are not valid inside fn; device `records` are valid for work ordered with
 * pwn_hip_ctx_signal_stream.  If the call has to be repeated (word 63 of the records, PWN_HIP_RECORD_FLOATS) fn runs again for the repeat.
 * fn = NULL switches it off. */
int pwn_hip_ctx_set_enqueued_callback(pwn_hip_ctx* ctx, void (*fn)(void* user), void* user);
/* Batch calls are executed in sub-batches of at most this many frames / pairs (default 64, capped by
 * max_batch), which bounds the workspace the temporaries (integral images, z-buffers) need.  Measured on
 * MI355X: larger sub-batches are faster (fewer, fuller launches) -- as long as every stream has one: a call of
 * 32 items or more is cut into a multiple of `streams` (below) equal sub-batches of at least 16 and no more than this many items (64 pairs
 * run as 2 x 32 on two streams: +7 % over 1 x 64).  Results do not depend on it. */
int pwn_hip_ctx_set_subbatch(pwn_hip_ctx* ctx, int frames, int pairs);
/* streams = 4 (default): batch calls deal their sub-batches round-robin over up to `streams` (1..4) HIP streams of the context when the
 * workspaces hold one sub-batch per stream: the short dependent kernels of one sub-batch (projection, 6x6 solve) fill the gaps of the
 * others' large ones.  Measured on MI355X, 128 VGA pairs per call: 2 streams +12 % over 1; with the one-submission step
 * (pwn_hip_convert_align_batch_u16) 4 streams x 32 pairs another +2 % over 2 x 64 (10.04-10.09 against 10.19-10.35 ms; round 2 had measured
 * 3 and 4 no better than 2 on the two-call sequence).  streams = 1: strictly serial launches (use it when profiling per-kernel durations).
 * Results are identical. */
int pwn_hip_ctx_set_concurrency(pwn_hip_ctx* ctx, int streams);
/* Storage of the point information matrices (InformationMatrix, informationmatrix.h:13; PointInformationMatrixCalculator::compute,
 * informationmatrixcalculator.cpp:9-36) of the clouds created on the context FROM NOW ON (existing clouds keep theirs;
 * pwn_hip_cloud_omega_storage tells).  The clouds of one convert batch and the current clouds of one align batch must share one.
 *   PWN_HIP_OMEGA_SYM6 (the default since round 6): the upper triangle as the reference evaluates it, 24 bytes per point (the size
 *     SURVEY.md 8(d) counts); readers -- the Linearizer (linearizer.cpp:66-67,84-88), cloud_download, the scene stage -- mirror it.  The
 *     reference's nine entries are symmetric only up to the rounding of each entry's own products, so the lower triangle differs from it by
 *     <= 1 ulp of the entry's largest term: Omega_p within 1e-6 |Omega_p| (measured 1.7e-7), chi2 / H / b within 1e-5 (measured 6e-8 from the
 *     same iterate), every other converter output bit-identical.  12 of the 30 bytes the fused correspondence + linearize pass gathers per
 *     correspondence and 12 of k_stats' 64 stored bytes less: the 128-pair step runs 11-13 % faster than with exact9.
 *   PWN_HIP_OMEGA_EXACT9: all nine entries of U diag U^t as the reference evaluates them, 36 bytes per point; EVERY converter output,
 *     the lower triangle of Omega_p included, is bit-identical to the CPU path.  The mode to select when a caller compares clouds bit for
 *     bit with pwn_core's (the parity tests do), at the cost above. */
#define PWN_HIP_OMEGA_EXACT9 0
#define PWN_HIP_OMEGA_SYM6 1
int pwn_hip_ctx_set_omega_storage(pwn_hip_ctx* ctx, int mode);
int pwn_hip_cloud_omega_storage(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, int* mode);
/* "Stop when converged": a deviation from the reference, whose Aligner::align always runs outerIterations (aligner.cpp:70); opt-in and off by
 * default, and a context with the default setting computes bit for bit what it computed without it.
 *   Let dx be the Gauss-Newton step solved in the LAST inner iteration of outer iteration i (0-based): dx[0:3] the translation, dx[3:6] the
 *   rotation part as v2t reads it, and
 *     s_t = sqrt((dx0*dx0 + dx1*dx1) + dx2*dx2)      s_r = sqrt((dx3*dx3 + dx4*dx4) + dx5*dx5)
 *   in fp32, every product rounded on its own, the sums left to right, the square root correctly rounded.  Both are recorded per pair at index i,
 *   whether or not the setting is enabled (pwn_hip_last_align_steps).
 *   Enabled, a pair is converged after outer iteration i iff  i + 1 >= min_iterations && s_t <= translation_epsilon && s_r <= rotation_epsilon
 *   (a NaN never converges).  The update of iteration i is applied as usual; from then on the pair is frozen: the remaining launches of the call
 *   return for it on the device (no host round trip; the launches themselves still happen, so this saves time in batches whose pairs converge
 *   at different iterations, not in the latency of a single pair).
 *   Contract: everything the call returns for a pair frozen after iteration i -- its pwn_hip_align_result (T, error, inliers, iterations, the
 *   traces), its record words, its matchClouds score, its statistics, and for the pair of slot 0 pwn_hip_align_images / pwn_hip_match_score -- equals
 *   bit for bit what the same call returns with outer_iterations = i + 1.  total_time_ms is exempt.
 * Every alignment entry point honours the setting.  The one exception is a stated limit of one entry point: pwn_hip_align_with_priors* with
 * n_priors > 0 returns PWN_HIP_ERR_INVALID_ARGUMENT while the setting is enabled, and touches nothing.  The loop it runs is the one of
 * pwn_hip_align_batch_priors, which honours the setting (n = 1 of that call is the way to a single pair with priors under it); lifting the
 * refusal is left to a change of its own.
 * set: NULL or enabled == 0 switches it off; enabling is refused (INVALID_ARGUMENT, setting unchanged) unless both epsilons are finite and >= 0
 * and min_iterations >= 0. */
typedef struct pwn_hip_convergence {
  int   enabled;
  float translation_epsilon;      /* metres */
  float rotation_epsilon;         /* norm of the rotation part of the step (about half the angle in radians) */
  int   min_iterations;           /* outer iterations every pair runs at least */
} pwn_hip_convergence;
int pwn_hip_ctx_set_convergence(pwn_hip_ctx* ctx, const pwn_hip_convergence* setting);
int pwn_hip_ctx_get_convergence(const pwn_hip_ctx* ctx, pwn_hip_convergence* setting);
/* The step norms of the pairs [first, first + n) of the context's last alignment call: `iterations` OUTER iterations were executed (the entries
 * [0, iterations) of both traces, zeros behind them), `converged` = 1 when the pair froze under the setting above.  Reads what the call left
 * behind (a call that returned records only fetches the states from the device on the first such request); INVALID_ARGUMENT when the range
 * is not inside the last call's pairs.  Every alignment call fills them, pwn_hip_align_with_priors* with n_priors > 0 included (the traces
 * pwn_hip_align_batch_priors leaves for that pair). */
typedef struct pwn_hip_align_steps {
  int   iterations;
  int   converged;
  float step_translation[PWN_HIP_MAX_ITERATIONS];
  float step_rotation[PWN_HIP_MAX_ITERATIONS];
} pwn_hip_align_steps;
int pwn_hip_last_align_steps(pwn_hip_ctx* ctx, int first, int n, pwn_hip_align_steps* out);
/* ctx may be NULL (errors of ctx_create). Never returns NULL. cf. AlignerStatus::toString (cudaaligner.h:54) */
const char* pwn_hip_last_error_string(const pwn_hip_ctx* ctx);
/* number of HIP devices visible; does not initialise a device */
int pwn_hip_device_count(void);

/* Page-locked host memory for depth frames handed to the convert calls from the host (a grabber's ring buffer): copies from it are
 * asynchronous DMA transfers that overlap the kernels of the other stream; from ordinary (pageable) memory every frame goes through the
 * runtime's bounce buffer and blocks the calling thread.  Does not need a context.  The reference has no counterpart (its images are
 * cv::Mat on the host, depthimageconverter.h:47); any host pointer is accepted by every entry point, this is the fast kind. */
int pwn_hip_host_alloc(void** ptr, size_t bytes);
int pwn_hip_host_free(void* ptr);
/* Device buffers for callers that do not link the HIP runtime themselves (the binding of INTEGRATION.md is plain C++): frames uploaded ahead
 * of time with pwn_hip_copy are used in place by the convert calls (no staging copy).  pwn_hip_copy: any direction, ordered after the work
 * already queued on the context, complete on return. */
int pwn_hip_device_alloc(pwn_hip_ctx* ctx, void** ptr, size_t bytes);
int pwn_hip_device_free(pwn_hip_ctx* ctx, void* ptr);      /* waits for the context's queued work first; ctx may be NULL once the context that
                                                             * allocated the buffer has been destroyed (the buffer is then simply released) */
int pwn_hip_copy(pwn_hip_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Fills `bytes` bytes of a device buffer with the byte `value` (0: a DepthImage::zeros that never leaves the device), queued on the context's
 * stream: every later call on the context sees it; returns at once. */
int pwn_hip_device_memset(pwn_hip_ctx* ctx, void* ptr, int value, size_t bytes);
/* The same copy queued on the context's copy stream; returns at once (for page-locked host memory -- pageable memory makes it wait).  The
 * next call on the context that reads data through a caller-supplied pointer -- convert*, unproject, project_intervals, the depth-image
 * helpers, cloud_gaussians, cloud_upload, integral_image, correspondences, linearize -- and pwn_hip_copy, ctx_synchronize, device_free
 * run after every copy issued so far.  The calls that take cloud handles only (align*, match*, project, merge, voxelize, cloud_add,
 * cloud_download*) do NOT wait: that is what lets a transfer overlap an alignment.  Pattern: upload the frames of batch k+1 into a second set of device
 * buffers, align batch k meanwhile, convert batch k+1 -- the transfers disappear behind the alignment.  The caller keeps source and
 * destination untouched until one of those calls has returned. */
int pwn_hip_copy_async(pwn_hip_ctx* ctx, void* dst, const void* src, size_t bytes);

void pwn_hip_default_converter_params(pwn_hip_converter_params* p);
void pwn_hip_default_aligner_params(pwn_hip_aligner_params* p);

/* ------------------------------------------------------------------ clouds ------------------- */
/* capacity = maximum number of points (rows*cols of the images it will be converted from; for a scene that grows by Cloud::add,
 * pwn_aligner.cpp:205-208, the sum of its frames): at most 2^25 = 33 554 432 (index field of the scene stage's 64-bit z-buffer word).
 * The clouds handed to the align / match calls may hold at most 2^21 = 2 097 152 points (index field of the aligner's 32-bit z-buffer
 * word: every frame up to 1448 x 1448 pixels) -- PWN_HIP_ERR_CAPACITY beyond that; merge, voxelize, cloud_add, save / load,
 * transform_in_place and project take the large ones. */
int pwn_hip_cloud_create(pwn_hip_ctx* ctx, int capacity, pwn_hip_cloud** cloud);
int pwn_hip_cloud_destroy(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud);
int pwn_hip_cloud_size(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, int* n);    /* Cloud::points().size() */
/* Upload a host/device pwn::Cloud: points/normals n*4 floats (Point/Normal, homogeneousvector4f.h:78-93),
 * curvature n floats (Stats::curvature(), stats.h:98-103), omega_p/omega_n n*16 floats
 * (InformationMatrix 4x4, informationmatrix.h:13).  cf. pwn_cuda initComputation (cudaaligner.h:63-75).  The cloud's previous content is
 * replaced whole: no Stats, no Gaussians, no index image afterwards. */
int pwn_hip_cloud_upload(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, int n, const float* points, const float* normals,
                         const float* curvature, const float* omega_p, const float* omega_n);
/* Any output may be NULL.  Same layouts as upload. */
int pwn_hip_cloud_download(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, float* points, float* normals,
                           float* curvature, float* omega_p, float* omega_n);
/* Stats of the last convert of this cloud (only if the convert ran with keep_stats != 0): per point
 * eigenvectors+mean as a column-major 4x4 (Stats, stats.h:13), eigenvalues[3], n (stats.h:30). */
int pwn_hip_cloud_download_stats(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, float* stats, float* eigenvalues, int* npoints);
/* Cloud::transformInPlace (cloud.cpp:173-186): points, normals, both information matrices (T Omega T^t, informationmatrix.h:111-121), the
 * Stats when the cloud carries them (m * S, stats.h:125-131) and the Gaussians (gaussian3.h:65-73); skipped when T is the identity (:176) */
int pwn_hip_cloud_transform_in_place(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, const float T[16]);
/* A cloud as ONE flat buffer, host or device: what replicates a cloud to the other GPUs of a node.  PwnCloser::processPartition
 * (pwn_tracker/pwn_closer.cpp:85-111) matches the cloud of ONE `current` frame against every cached cloud of the other partition; sharded over
 * GPUs, the others stay where they were converted and `current` travels ("replicate current's cloud to all GPUs; one
 * broadcast") -- export on the rank that converted it, one broadcast of the buffer, import on every rank.  The reference's own whole-cloud
 * form is Cloud::save / load (cloud.cpp:11-136; pwn_hip_cloud_save / _load), which goes through a file and drops the information matrices.
 * Content: 256-byte header, points (12 B), normal + curvature (16 B), the point information matrices as stored (exact9 / sym6), the class
 * matrices of the normal information matrix (or its full planes for uploaded clouds), and the converter's index image with the projector it
 * belongs to when the cloud carries one (so that an imported cloud takes the same projection shortcuts as the original: bitwise the same
 * alignments).  Not carried: Stats, Gaussians (the scene stage's data; Aligner::align reads neither).
 * export_bound: buffer size that holds any cloud of that capacity.  export: *written (optional) = bytes used; PWN_HIP_ERR_CAPACITY when
 * dst_bytes is too small (*written then = bytes needed); dst = NULL: size query only.  import: the destination cloud must have been created with
 * the same omega storage and capacity >= the flat cloud's points.  Both are complete on return; with device buffers that another stream
 * produces / consumes see pwn_hip_ctx_wait_stream. */
size_t pwn_hip_cloud_export_bound(int capacity, int omega_storage, int index_pixels, int with_omega_n);
int pwn_hip_cloud_export(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, void* dst, size_t dst_bytes, size_t* written);
int pwn_hip_cloud_import(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, const void* src, size_t src_bytes);

/* ------------------------------------------------------------------ input conditioning ------- */
/* DepthImage_convert_16UC1_to_32FC1 (pwn_static.cpp:54-68) */
int pwn_hip_depth_u16_to_f32(pwn_hip_ctx* ctx, const uint16_t* src, float* dst, int n, float scale);
/* DepthImage_convert_32FC1_to_16UC1 (pwn_static.cpp:38-52) */
int pwn_hip_depth_f32_to_u16(pwn_hip_ctx* ctx, const float* src, uint16_t* dst, int n, float scale);
/* DepthImage_scale (pwn_static.cpp:5-36); dst holds (rows/step)*(cols/step) floats */
int pwn_hip_depth_scale(pwn_hip_ctx* ctx, const float* src, int rows, int cols, int step, float max_depth_cov, float* dst);
/* DepthImage_scale (pwn_static.cpp:5-36) of n frames of equal size in one call: src[i] (rows*cols floats) -> dst[i] ((rows/step)*(cols/step)
 * floats); src / dst: n pointers (host arrays), each frame host or device.  step = 1 is the reference's copy that zeroes non-positive pixels.
 * Waits for the results. */
int pwn_hip_depth_scale_batch(pwn_hip_ctx* ctx, const float* const* src, int n, int rows, int cols, int step, float max_depth_cov,
                              float* const* dst);
/* Same, from raw uint16 frames: DepthImage_convert_16UC1_to_32FC1 (pwn_static.cpp:54-68, depth = depth_scale * raw) fused in front. */
int pwn_hip_depth_scale_batch_u16(pwn_hip_ctx* ctx, const uint16_t* const* src, float depth_scale, int n, int rows, int cols, int step,
                                  float max_depth_cov, float* const* dst);

/* ------------------------------------------------------------------ converter stages --------- */
/* PinholePointProjector::unProject(points, gaussians, indexImage, depthImage) (pinholepointprojector.cpp:93-133)
 * with the projector transform T (identity inside the converter).  Fills cloud points (normals etc. are
 * reset to "invalid").  The per-point sensor Gaussians are not produced (only Merger consumes them); the cloud's previous content is replaced
 * whole: no Stats, no Gaussians, zero normal information for the zero normals. */
int pwn_hip_unproject(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float T[16], const float* depth,
                      int rows, int cols, pwn_hip_cloud* cloud, int* index_image);
/* PinholePointProjector::projectIntervals (pinholepointprojector.cpp:135-147) */
int pwn_hip_project_intervals(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols,
                              int* interval_image);
/* PointIntegralImage::compute (pointintegralimage.cpp:7-44): the 10 unique channels
 * (x,y,z,n,xx,xy,xz,yy,yz,zz) as planes out[10][rows][cols]. Diagnostic / parity entry point. */
int pwn_hip_integral_image(pwn_hip_ctx* ctx, const int* index_image, const pwn_hip_cloud* cloud, int rows, int cols, float* out);
/* DepthImageConverterIntegralImage::compute(cloud, depthImage, sensorOffset)
 * (depthimageconverterintegralimage.cpp:15-55).  index_image / interval_image: optional outputs
 * (DepthImageConverter::indexImage(), depthimageconverter.h:111). keep_stats: also keep per-point Stats.
 * Every conversion call (this one, the batch and scaled forms, the one-submission steps) that returns an error after it has begun to write
 * leaves its clouds empty: size 0, no Stats, no Gaussians, no index image. */
int pwn_hip_convert(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols,
                    pwn_hip_cloud* cloud, int* index_image, int* interval_image, int keep_stats);
/* PwnMatcherBase::makeCloud's data path in one call (pwn_tracker/pwn_matcher_base.cpp:71-79): DepthImage_scale(depth, step,
 * max_depth_cov) followed by the converter on the (rows/step) x (cols/step) image, without leaving the device.
 * p->K must already be the scaled camera matrix. */
int pwn_hip_convert_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, int step,
                           float max_depth_cov, pwn_hip_cloud* cloud);
/* The same conversion in two halves, for callers that know their next frame before they are done with the current one (a recorded or
 * buffered stream through PwnTracker::processFrame, pwn_tracker/pwn_tracker.cpp:115: makeCloud of frame k+1 does not depend on the
 * alignment of frame k).  _begin returns at once: the frame is converted by a helper thread on streams and workspaces of its own (created
 * on first use: one more set of single-frame workspaces), next to whatever the caller runs on `ctx` meanwhile.  _end waits for it and
 * returns what pwn_hip_convert_scaled would have returned; the cloud then holds the same bits.  Between the two calls `depth` must stay
 * valid and unchanged and `cloud` must not be passed to any other entry point (pwn_hip_cloud_destroy and pwn_hip_ctx_destroy wait for a
 * conversion in flight).  One conversion in flight per context. */
int pwn_hip_convert_scaled_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols, int step,
                                 float max_depth_cov, pwn_hip_cloud* cloud);
int pwn_hip_convert_end(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud);
/* The look-ahead of a sharded PwnCloser::processPartition (pwn_tracker/pwn_closer.cpp:85-111): the outer loop hands the closer one `current`
 * keyframe after the other, and _cache->get(current) of keyframe k+1 (:92-93; PwnCache::makeCloud, pwn_tracker_cache.cpp:24-51) depends on nothing
 * keyframe k's matches produce.  _begin returns at once; a helper thread converts the raw uint16 frame (depth = depth_scale * raw, as
 * pwn_hip_convert_batch_u16) into `cloud` and then, with flat_dst != NULL, writes the cloud's flat form (pwn_hip_cloud_export) into flat_dst (device
 * or host; at least pwn_hip_cloud_export_bound(min(capacity, rows*cols), storage, rows*cols, 0) bytes, checked by _begin) -- what the rank that owns
 * `current` broadcasts while every rank still matches the previous keyframe.  _end waits for the job, returns its status and reports the bytes
 * written (what to broadcast) and the job's wall time on the helper thread in milliseconds; both optional.  Same rules as
 * pwn_hip_convert_scaled_begin between the two calls (frame, cloud AND flat_dst belong to the job; one job in flight per context); the cloud holds
 * the bits pwn_hip_convert_batch_u16 gives, the buffer the bytes pwn_hip_cloud_export gives. */
int pwn_hip_convert_export_begin(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* raw_frame, float depth_scale, int rows, int cols,
                                 pwn_hip_cloud* cloud, void* flat_dst, size_t flat_bytes);
int pwn_hip_convert_export_end(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, size_t* written, float* job_ms);
/* n independent frames of equal size in one call.  depth[i] -> clouds[i].
 * depth_frames: n pointers (host array) to rows*cols floats each (each host or device).  A call refused for a null frame or cloud, or for
 * clouds of mixed omega storages, leaves every cloud as it was. */
int pwn_hip_convert_batch(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* const* depth_frames,
                          int n, int rows, int cols, pwn_hip_cloud* const* clouds);
/* Same, from raw uint16 millimetre frames: fuses DepthImage_convert_16UC1_to_32FC1 (scale) in front. */
int pwn_hip_convert_batch_u16(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* const* raw_frames,
                              float depth_scale, int n, int rows, int cols, pwn_hip_cloud* const* clouds);
/* n x PwnMatcherBase::makeCloud's data path (pwn_tracker/pwn_matcher_base.cpp:57-86) in one call: DepthImage_scale(frame i, step,
 * max_depth_cov) and the converter on the (rows/step) x (cols/step) image -> clouds[i], inside the batch plan (the box mean of a
 * sub-batch's frames is queued on its stream in front of its conversion).  rows, cols: the SOURCE size; p->K must already be the scaled
 * camera matrix.  clouds[i] holds the bits pwn_hip_convert_scaled gives for frame i, index image included.  A refused call leaves the
 * clouds as they were: PWN_HIP_ERR_INVALID_ARGUMENT for step < 1, an empty scaled image, a null frame or cloud, mixed omega storages;
 * PWN_HIP_ERR_CAPACITY for a context smaller than the source frame or a cloud smaller than its number of valid scaled pixels. */
int pwn_hip_convert_batch_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* const* depth_frames, int n, int rows,
                                 int cols, int step, float max_depth_cov, pwn_hip_cloud* const* clouds);
/* Same, from raw uint16 frames (DepthImage_convert_16UC1_to_32FC1, pwn_static.cpp:54-68, in front of DepthImage_scale, :5-36). */
int pwn_hip_convert_batch_u16_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const uint16_t* const* raw_frames,
                                     float depth_scale, int n, int rows, int cols, int step, float max_depth_cov,
                                     pwn_hip_cloud* const* clouds);
/* What a cloud that leaves DepthImageConverter::compute carries besides points, normals and matrices (depthimageconverterintegralimage.cpp:39,
 * pinholepointprojector.cpp:104-123), and the scene stage needs: Merger::merge reads the Gaussians, Cloud::save writes the Stats, PwnMerger::
 * mergeNodeList copies both.  The batch calls above make lean clouds; pwn_hip_convert_batch_ex makes scene-ready ones on request. */
typedef struct pwn_hip_convert_extras {
  int keep_stats;                 /* 1: cloud i holds the Stats pwn_hip_convert(..., keep_stats = 1) gives for the image the front end read */
  int gaussians;                  /* 1: cloud i holds, for every point, the record pwn_hip_cloud_gaussians writes (sensor offset included) */
  float baseline, alpha;          /* PinholePointProjector::_baseline, _alpha (pinholepointprojector.cpp:10-11) */
} pwn_hip_convert_extras;
void pwn_hip_default_convert_extras(pwn_hip_convert_extras* e);   /* 0, 0, 0.075, 0.1 */
/* The four batch calls above behind one entry point, with the extras.  raw_u16 != 0: frames are uint16 with depth_scale (the _u16 forms), else
 * floats (depth_scale is ignored).  step == 0: the unscaled call on rows x cols frames; step >= 1: the _scaled form (rows, cols: the SOURCE
 * size, p->K already scaled, max_depth_cov as there).  extras == NULL or all flags zero: the launches and the clouds of the matching call
 * above, bit for bit.  With extras->gaussians the image the Gaussians are made from is the one the front end read (depth_scale * raw, the
 * box-averaged image, or both) and pwn_hip_cloud_num_gaussians equals the cloud's size afterwards; without, the clouds have none.  Everything is
 * queued inside the batch plan, one kernel per sub-batch behind its conversion, and the host waits once.  Refused, every cloud as it was: what
 * the matching call above refuses; a non-finite baseline or alpha; keep_stats or gaussians outside {0, 1} (PWN_HIP_ERR_INVALID_ARGUMENT).  A call
 * that fails later leaves its clouds empty, without Stats and Gaussians. */
int pwn_hip_convert_batch_ex(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const void* const* frames, int raw_u16, float depth_scale,
                             int n, int rows, int cols, int step, float max_depth_cov, const pwn_hip_convert_extras* extras,
                             pwn_hip_cloud* const* clouds);

/* ------------------------------------------------------------------ aligner stages ----------- */
/* PinholePointProjector::project(indexImage, depthImage, points) (pinholepointprojector.cpp:33-66) with
 * projector transform T.  Untouched depth pixels are FLT_MAX, index -1; ties keep the lowest index. */
int pwn_hip_project(pwn_hip_ctx* ctx, const float K[9], const float T[16], float min_distance, float max_distance,
                    int rows, int cols, const pwn_hip_cloud* cloud, int* index_image, float* depth_image);
/* ---- the merged closure (pwn_tracker2/pwn_closer_with_merger.cpp:108-224): the clouds of a partition fused into ONE depth image in the view of
 * `current`, one alignment per partition instead of one per candidate.  merged / weights (rows*cols floats each, in / out), the images and
 * `planes` may be host or device memory; overlap and points are host memory.  A refused call -- a null argument, n < 0, an image larger than
 * the context's, min_distance < 0, a cloud of another context -- returns its status and leaves merged, weights and the counters untouched;
 * n == 0 is a no-op that returns PWN_HIP_OK.  merged, weights, the images and `planes` must not overlap one another (merged == weights is refused; other
 * overlaps are the caller's to avoid: the kernels read and write them as distinct arrays).  The context keeps min(max_batch, 256) depth planes of max_rows*max_cols words (allocated by the
 * first call); a call with more images runs in chunks of that many, in order, with the same bits. */
/* Merger2::mergeDepthImage(out, image) (pwn_tracker2/merger2.cpp:75-101) for depth_images[0..n) in call order: a pixel d inside (0.1, 10000)
 * replaces `merged` where that is 0 or more than 3e-5 behind d (weight 1/d), else is averaged in with inverse-depth weights when within 0.2
 * (:84-96); `weights` is Merger2::_image_pesi.  overlap[i] (n ints, may be NULL) = _image_overlapping_points_count after image i (the reference
 * resets it per image, :77); *points (may be NULL) += the pixels replaced, _image_points_count (:86; Merger2::clear zeroes it, :40). */
int pwn_hip_merge_depth_images(pwn_hip_ctx* ctx, int n, const float* const* depth_images, int rows, int cols, float* merged, float* weights,
                               int* overlap, int* points);
/* PwnCloserWithMerger::mergeNode (pwn_tracker2/pwn_closer_with_merger.cpp:210-224) for n nodes in one submission on the context's stream:
 * PinholePointProjector::project's depth image (pinholepointprojector.cpp:33-66) of clouds[i] under the projector transform
 * transforms[16 i .. 16 i + 16) (column-major; camera matrix K, range, image size shared), then Merger2::mergeDepthImage of the n images in
 * order, without leaving the device.  planes (optional, n*rows*cols floats) receives the projected depth images (FLT_MAX where nothing
 * landed): what n pwn_hip_project calls return as depth_image, bit for bit. */
int pwn_hip_project_merge_batch(pwn_hip_ctx* ctx, const float K[9], int n, pwn_hip_cloud* const* clouds, const float* transforms,
                                float min_distance, float max_distance, int rows, int cols, float* merged, float* weights, int* overlap,
                                int* points, float* planes);
/* CorrespondenceFinder::compute (correspondencefinder.cpp:20-118, single-thread canonical order).
 * correspondences: rows*cols pairs (referenceIndex,currentIndex) -- the first *n_correspondences are
 * valid, in row-major pixel order, the rest are (-1,-1) (correspondencefinder.cpp:116-117). */
int pwn_hip_correspondences(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* reference,
                            const pwn_hip_cloud* current, const int* reference_index_image, const int* current_index_image,
                            const float T[16], int* correspondences, int* n_correspondences, int* n_candidates);
/* Linearizer::update (linearizer.cpp:17-115) on an explicit correspondence list with transform T (= invT).
 * H: column-major 6x6 (Linearizer::H()), b: 6 (Linearizer::b()). cf. pwn_cuda getHb (cudaaligner.h:79). */
int pwn_hip_linearize(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* reference,
                      const pwn_hip_cloud* current, const int* correspondences, int n_correspondences, const float T[16],
                      float* H, float* b, float* error, int* inliers);
/* Aligner::align (aligner.cpp:49-125): project current once, then outer x inner Gauss-Newton
 * iterations of {project reference, find correspondences, linearize, damped LDLT solve, update}.
 * The whole loop runs on the device without host round trips. Priors and _computeStatistics
 * (aligner.cpp:96-108,127) are not part of this entry point. */
int pwn_hip_align(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* reference,
                  const pwn_hip_cloud* current, pwn_hip_align_result* result);
/* CorrespondenceFinder::{reference,current}{Index,Depth}Image() after the last pwn_hip_align
 * (correspondencefinder.h:99-117; read by pwn_tracker/pwn_matcher_base.cpp:153-155). Any may be NULL.
 * The aligner's z-buffers keep point indices only; the depth images are recomputed from the two clouds' points, so this call (and
 * pwn_hip_match_score) is valid until either cloud of that alignment is destroyed or gets new content (then: INVALID_ARGUMENT). */
int pwn_hip_align_images(pwn_hip_ctx* ctx, int* reference_index, float* reference_depth, int* current_index, float* current_depth);
/* n independent alignments (the loop-closure candidate batch, pwn_tracker/pwn_closer.cpp:92-111).
 * p is shared by all pairs; initial_guesses: n*16 floats or NULL (= p->initial_guess for all). */
int pwn_hip_align_batch(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                        pwn_hip_cloud* const* currents, const float* initial_guesses, pwn_hip_align_result* results);

/* ------------------------------------------------------------------ matcher ---------- */
/* Post-alignment depth-agreement score of PwnMatcherBase::matchClouds (pwn_tracker/pwn_matcher_base.cpp:153-182) on the
 * finder depth images of the last pwn_hip_align: DepthImage_convert_32FC1_to_16UC1 of both (scale 1000, FLT_MAX -> 0),
 * mask, |difference|, counts.  frame_inlier_depth_threshold: _frameInlierDepthThreshold (50, pwn_matcher_base.cpp:13). */
int pwn_hip_match_score(pwn_hip_ctx* ctx, float frame_inlier_depth_threshold, pwn_hip_match_result* out);
/* pwn_hip_align_batch + the score of every pair (the loop-closure check of PwnCloser::processPartition,
 * pwn_tracker/pwn_closer.cpp:92-111, without the host loop).  scores: n records. */
int pwn_hip_match_batch(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                        pwn_hip_cloud* const* currents, const float* initial_guesses, float frame_inlier_depth_threshold,
                        pwn_hip_align_result* results, pwn_hip_match_result* scores);

/* Everything Aligner::align() does for n pairs in one call: the Gauss-Newton loop, optionally the matcher's depth-agreement
 * score (scores != NULL) and optionally Aligner::_computeStatistics (statistics != NULL; aligner.cpp:127,152-199: one more
 * linearizer update at the final transform on the finder's last correspondences, then the 6x6 covariance / unscented math
 * on the host; pwn_hip_closure_batch_records runs that math on the device and returns it in the pair's record).
 * pwn_hip_align_batch / pwn_hip_match_batch are this call with the optional outputs left NULL. */
int pwn_hip_align_batch_ex(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                           pwn_hip_cloud* const* currents, const float* initial_guesses, pwn_hip_align_result* results,
                           float frame_inlier_depth_threshold, pwn_hip_match_result* scores, pwn_hip_align_statistics* statistics);
/* The result of a pair as ONE fixed-size record of PWN_HIP_RECORD_FLOATS floats (256 bytes) -- what the ranks of a sharded candidate batch
 * exchange (the reference runs the candidates of PwnCloser::process one after the other on one Aligner and keeps MatcherResult per pair,
 * pwn_tracker/pwn_closer.cpp:92-111):
 *   [0:16] T (column-major)   [16] chi2 of the last iteration   [17] its inliers   [18] iterations   [19] pair id
 *   [20:30] chi2_i   [30:40] inliers_i   [40:50] correspondences C_i   [50:60] candidates K_i   (first 10 iterations; 0 beyond the last)
 *   [60] points of the reference cloud   [61] of the current cloud   [62] iterations carried in the traces
 *   [63] 0; 1 = a projection of the call gave up on a pixel and the call is being repeated (the records a call RETURNS always carry 0: only a reader
 *        that takes device records inside pwn_hip_ctx_set_enqueued_callback can meet a 1, and drops those records)
 * Counts travel as float (exact below 2^24).  The records are written by a kernel from the pairs' device state: `records` may be a DEVICE
 * buffer (n * PWN_HIP_RECORD_FLOATS floats; e.g. the tensor an all-gather sends -- no trip through the host) or host memory.
 * pair_ids (host, may be NULL: then record i carries first_pair_id + i).  results may be NULL when only the records are wanted.
 * ORDERING: the kernel writes a device `records` buffer on the context's own stream.  If a stream of the caller still reads the buffer from
 * the previous call (an all-gather queued after it), call pwn_hip_ctx_wait_stream(ctx, that stream) before this call -- or alternate two buffers. */
#define PWN_HIP_RECORD_FLOATS 64
int pwn_hip_align_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                                pwn_hip_cloud* const* currents, const float* initial_guesses, const int* pair_ids, int first_pair_id,
                                pwn_hip_align_result* results, float* records);
/* pwn_hip_match_batch whose results (also) leave as records of PWN_HIP_MATCH_RECORD_FLOATS floats (288 bytes): the 64 words of the alignment
 * record, then PwnMatcherBase::MatcherResult's image fields (pwn_tracker/pwn_matcher_base.cpp:175-181)
 *   [64] image_nonZeros   [65] image_outliers   [66] image_inliers   [67] image_reprojectionDistance   [68:72] 0
 * -- everything PwnCloser::matchFrames thresholds and stores in a PwnCloserRelation (pwn_closer.cpp:138-151), written on the device.  `records`:
 * device or host, n * PWN_HIP_MATCH_RECORD_FLOATS floats; results and scores may be NULL.  A device `records` buffer that another stream still
 * reads from the previous call: pwn_hip_ctx_wait_stream. */
#define PWN_HIP_MATCH_RECORD_FLOATS 72
int pwn_hip_match_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                                pwn_hip_cloud* const* currents, const float* initial_guesses, float frame_inlier_depth_threshold,
                                const int* pair_ids, int first_pair_id, pwn_hip_align_result* results, pwn_hip_match_result* scores,
                                float* records);
/* pwn_hip_match_batch_records whose records carry the one field of a closure relation the match record lacks: MatcherResult::informationMatrix =
 * Aligner::omega() (pwn_tracker2/pwn_matcher_base.cpp:158-163, stored in the PwnCloserRelation by pwn_closer.cpp).  The extra linearizer update of
 * Aligner::_computeStatistics runs on the device as for pwn_hip_align_batch_ex, and so does its 6x6 math (k_pair_statistics, one pair per
 * workgroup, directly behind that update on the sub-batch's stream): the same bits as pwn_hip_compute_statistics, no per-pair host math.
 * A record has PWN_HIP_CLOSURE_RECORD_FLOATS floats (512 bytes):
 *   [0:72]    the record of pwn_hip_match_batch_records, word for word
 *   [72:108]  Aligner::omega(), column-major   [108:114] the remapped mean   [114] translational, [115] rotational eigen ratio
 *   [116] error, [117] inliers of the extra update (the count as float)
 *   [118]     1 = the statistics were computed; 0 when outer_iterations == 0, and then [72:118] are 0 (as pwn_hip_align_batch_ex leaves them)
 *   [119:128] 0
 * H and b of the extra update are not in the record: a caller who wants them passes `statistics` (host, n entries, may be NULL), which is filled
 * from the device's record and sums.  `records`: device or host, n * PWN_HIP_CLOSURE_RECORD_FLOATS floats; results and scores may be NULL.
 * Ordering, the enqueued callback and word 63 as for the other record calls. */
#define PWN_HIP_CLOSURE_RECORD_FLOATS 128
int pwn_hip_closure_batch_records(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                                  pwn_hip_cloud* const* currents, const float* initial_guesses, float frame_inlier_depth_threshold,
                                  const int* pair_ids, int first_pair_id, pwn_hip_align_result* results, pwn_hip_match_result* scores,
                                  pwn_hip_align_statistics* statistics, float* records);

/* ---- consensus validation of closures (boss_map_building/map_closer.cpp:200-253, :286-417) -----------------------------------
 * What MapCloser::process runs after every processPartition: validatePartitions(other, current).  For the n relations that join the two
 * partitions, reference relation i predicts where every relation j should land; the n x n pose errors of validateRelation become two integer
 * votes, and the votes decide which relations are committed (ClosureFoundMessage) and which are removed.
 *   relation i = (tc_i, to_i, tr_i): the pose of its node in the current partition, of its node in the other partition, and its transform
 *   TR_i = tr_i, or tr_i^-1 when bit 0 of flags[i] is set (the reference's `else` branch, :211-214 / :231-234);  tfix_i = (to_i TR_i) tc_i^-1
 *   pair (j, i): te = TR_j^-1 (to_j^-1 (tfix_i tc_j));  transErr = (float)|te.translation|^2;  rotErr = (float)AngleAxisd(te.linear()).angle()
 *   isIn(j, i) = transErr < inlier_translational_threshold && fabs(rotErr) < inlier_rotational_threshold
 * Order of effects: every times_checked goes up by one; for each column i with c_i = sum_j isIn(j, i): cum_inlier[j] += c_i where isIn(j, i),
 * else cum_outlier_times[j] += 1; then decisions[j] = 0 (skipped: times_checked[j] < min_times_checked), 1 (accepted: cum_inlier[j] >
 * cum_outlier_times[j]) or 2 (removed).  The three counters are ClosureInfo::consensusTimeChecked / consensusCumInlier /
 * consensusCumOutlierTimes, in / out.
 * All arithmetic is double in a fixed order, one text for the host and the device: the device call returns the host call's bits.  The angle is
 * Eigen 3.3's (2 atan2(|vec|, |w|) of the unnormalised quaternion); Eigen <= 3.2 (2 acos(w)) takes the same decision for every rotational
 * threshold up to 2 pi / 3, and a larger threshold is refused.
 * tc, to: n x 16 doubles, column-major.  The transforms: tr (n x 16 doubles), or the records a closer call wrote (record_floats = 64, 72 or 128;
 * T = words [0:16], each of the twelve upper entries converted to double, the last row forced) -- exactly one of the two.  flags may be NULL.
 * The error matrices are optional: n x n floats, column-major, element (j, i) at j + n i (translationalErrors.col(i)).  Every array of the
 * device call is host or device memory.
 * A column without an inlier is the reference's throw "no inliers" (a NaN pose produces one): PWN_HIP_ERR_INVALID_ARGUMENT, the column named in
 * pwn_hip_last_error_string (and in *empty_column by the host call, else -1), counters and decisions exactly as they were.  n == 0 is a
 * no-op; n > PWN_HIP_CONSENSUS_MAX_RELATIONS returns PWN_HIP_ERR_CAPACITY; a NULL required argument, both or neither of tr and records,
 * another record_floats, a translational threshold that is not positive or a rotational one outside (0, 2 pi / 3] return
 * PWN_HIP_ERR_INVALID_ARGUMENT with nothing written. */
typedef struct pwn_hip_consensus_params {
  float inlier_translational_threshold;   /* 0.5*0.5, squared metres           map_closer.cpp:63 */
  float inlier_rotational_threshold;      /* (float)(15.0f*M_PI/180.0f)        :64; must lie in (0, 2*pi/3] */
  int   min_times_checked;                /* 5                                 :65 */
} pwn_hip_consensus_params;
void pwn_hip_default_consensus_params(pwn_hip_consensus_params* p);
#define PWN_HIP_CONSENSUS_MAX_RELATIONS 8192
/* host, no context: column i of both error matrices (n floats each), what validateRelation(..., rels[i], ...) writes */
void pwn_hip_validate_relation(int n, const double* tc, const double* to, const double* tr, const int* flags, int i,
                               float* translational_errors, float* rotational_errors);
/* host, no context: all of validatePartitions from the same text, serially */
int pwn_hip_validate_relations_host(const pwn_hip_consensus_params* p, int n, const double* tc, const double* to, const double* tr,
                                    const int* flags, int* times_checked, int* cum_inlier, int* cum_outlier_times, int* decisions,
                                    float* translational_errors, float* rotational_errors, int* empty_column);
/* device: four launches on the context's stream and one host wait (stages consensus_prepare, consensus_errors, consensus_count,
 * consensus_commit in pwn_hip_last_stage_ms); the empty-column condition is a word a kernel writes and the committing kernel reads */
int pwn_hip_validate_relations(pwn_hip_ctx* ctx, const pwn_hip_consensus_params* p, int n, const double* tc, const double* to,
                               const double* tr, const float* records, int record_floats, const int* flags,
                               int* times_checked, int* cum_inlier, int* cum_outlier_times, int* decisions,
                               float* translational_errors, float* rotational_errors);

/* One candidate batch from raw frames as ONE submission: per pair i, DepthImageConverter::compute of ref_frames[i] -> references[i] and
 * cur_frames[i] -> currents[i] (PwnMatcherBase::makeCloud, pwn_matcher_base.cpp:77-85), then Aligner::align of the pair
 * (pwn_matcher_base.cpp:120-128).  The conversion of a sub-batch's frames is queued in front of its alignment on the same stream, so one
 * sub-batch converts while the other aligns and nothing waits for the host between the two halves.  Results are bit for bit those of
 * pwn_hip_convert_batch_u16 followed by pwn_hip_align_batch.  The 2 n clouds must be distinct; frames: uint16 millimetres, host or device.
 * A call refused for a null frame or cloud, or for clouds of mixed omega storages, leaves every cloud as it was. */
int pwn_hip_convert_align_batch_u16(pwn_hip_ctx* ctx, const pwn_hip_converter_params* converter, const pwn_hip_aligner_params* aligner, int n,
                                    const uint16_t* const* ref_frames, const uint16_t* const* cur_frames, float depth_scale, int rows, int cols,
                                    pwn_hip_cloud* const* references, pwn_hip_cloud* const* currents, const float* initial_guesses,
                                    const int* pair_ids, int first_pair_id, pwn_hip_align_result* results, float* records);
/* The same step at 1/step resolution, as the reference's callers run it (PwnMatcherBase::makeCloud, pwn_matcher_base.cpp:57-86: _scale is 2
 * by default, :12): every frame goes through DepthImage_scale(frame, step, max_depth_cov) in front of its conversion.  rows, cols: the
 * SOURCE size; converter->K and aligner->K the scaled camera matrix; aligner->rows / cols must equal rows/step, cols/step.  Results are bit
 * for bit those of pwn_hip_convert_batch_u16_scaled followed by pwn_hip_align_batch_records. */
int pwn_hip_convert_align_batch_u16_scaled(pwn_hip_ctx* ctx, const pwn_hip_converter_params* converter, const pwn_hip_aligner_params* aligner,
                                           int n, const uint16_t* const* ref_frames, const uint16_t* const* cur_frames, float depth_scale,
                                           int rows, int cols, pwn_hip_cloud* const* references, pwn_hip_cloud* const* currents,
                                           const float* initial_guesses, const int* pair_ids, int first_pair_id,
                                           pwn_hip_align_result* results, float* records, int step, float max_depth_cov);
/* Aligner::align with priors (aligner.cpp:96-108), one pair: one pair of pwn_hip_align_batch_priors (below), the loop on the device.  The
 * prior terms (numeric Jacobians, se3_prior.cpp:8-52) change the normal equations of every iteration; the initial guess is p->initial_guess,
 * the pair's list the n_priors records of `priors` in that order.  n_priors <= 0 is pwn_hip_align.  Like every alignment call it leaves the
 * step traces (pwn_hip_last_align_steps), with profiling on the stage times (pwn_hip_last_stage_ms), the finder's images of the pair
 * (pwn_hip_align_images, pwn_hip_match_score), runs a set enqueued callback, takes the current cloud's own index image where it may, and waits
 * for the device once.  Result, statistics, a following score and the following images are bit for bit those of the loop the host once
 * drove behind this entry point (one wait per iteration, no traces, no stage times, no callback), for every call that loop accepted.
 * Refused with PWN_HIP_ERR_INVALID_ARGUMENT, nothing touched: a NULL ctx, p, cloud or result; with n_priors > 0 also NULL priors, a kind
 * outside {0, 1} (never defined; it used to be read half as a relative, half as an absolute prior), and the convergence setting enabled
 * (see pwn_hip_ctx_set_convergence). */
int pwn_hip_align_with_priors(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* reference,
                              const pwn_hip_cloud* current, int n_priors, const pwn_hip_prior* priors, pwn_hip_align_result* result);
/* The same with Aligner::_computeStatistics (aligner.cpp:127): the reference runs it after every align(), priors or not, on
 * Linearizer::H() + I at the final transform -- the prior terms are not part of that H (aligner.cpp:165-170).  statistics may
 * be NULL (= pwn_hip_align_with_priors); n_priors = 0 is pwn_hip_align_batch_ex for one pair. */
int pwn_hip_align_with_priors_ex(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, const pwn_hip_cloud* reference,
                                 const pwn_hip_cloud* current, int n_priors, const pwn_hip_prior* priors, pwn_hip_align_result* result,
                                 pwn_hip_align_statistics* statistics);
/* the host-side part alone: H = Linearizer::H() at the final transform, T = Aligner::T() */
void pwn_hip_compute_statistics(const float H[36], const float T[16], float mean[6], float omega[36],
                                float* translational_eigen_ratio, float* rotational_eigen_ratio);
/* The terms one prior adds to the normal equations of an inner iteration (aligner.cpp:99-107), the host side alone: invT = Linearizer::_T of
 * that iteration (column-major, last row 0 0 0 1), Hp = J^T Omega' J (column-major), bp = J^T Omega' e, with the numeric Jacobians of
 * se3_prior.cpp:8-52.  *valid = 0: the inverse of the prior's Jz was refused, the reference skips such a prior, Hp and bp are zeros.  The
 * text every alignment call with priors expands, on the host and on the device (the same bits). */
void pwn_hip_prior_terms(const float invT[16], const pwn_hip_prior* prior, float Hp[36], float bp[6], int* valid);
/* Batch alignment with SE(3) priors, device-resident: pwn_hip_align_batch_ex (records == NULL, record_floats == 0) or one of the three
 * record calls (record_floats == PWN_HIP_RECORD_FLOATS, PWN_HIP_MATCH_RECORD_FLOATS or PWN_HIP_CLOSURE_RECORD_FLOATS; layouts unchanged)
 * in which pair i carries the priors pair_priors->priors[first[i] .. first[i + 1]) in that order, as Aligner::addRelativePrior /
 * addAbsolutePrior queued them.  Once per inner iteration a sub-batch that holds at least one prior runs a small kernel that computes the
 * terms of its pairs' priors at the pair's Linearizer::_T, and its solve step adds the valid ones behind the two damping additions
 * (aligner.cpp:92-108); the loop stays on the device, and so do traces, step norms and the convergence setting (honoured as everywhere: a
 * stopped pair returns the result of that many outer iterations).  Statistics and omega come from the linearizer's H alone
 * (aligner.cpp:165-170).  A batch of n equals n single calls: pwn_hip_align_with_priors_ex is one pair of this call.  pair_priors == NULL or first[n] == 0:
 * the launches and the bits of the matching call without priors.  scores, statistics and results may be NULL as in those calls (results
 * only when records are asked for).  Refused with PWN_HIP_ERR_INVALID_ARGUMENT, nothing touched: first == NULL, first[0] != 0, a decreasing
 * first, priors == NULL with first[n] > 0, a kind outside {0, 1}, a record_floats outside the four values, records == NULL with
 * record_floats != 0 (or the reverse). */
typedef struct pwn_hip_pair_priors {   /* pair i carries priors[first[i] .. first[i+1]) in that order */
  const int* first;                    /* n + 1 host ints, first[0] = 0, non-decreasing */
  const pwn_hip_prior* priors;         /* first[n] host records */
} pwn_hip_pair_priors;
int pwn_hip_align_batch_priors(pwn_hip_ctx* ctx, const pwn_hip_aligner_params* p, int n, pwn_hip_cloud* const* references,
                               pwn_hip_cloud* const* currents, const float* initial_guesses, const pwn_hip_pair_priors* pair_priors,
                               float frame_inlier_depth_threshold, const int* pair_ids, int first_pair_id, pwn_hip_align_result* results,
                               pwn_hip_match_result* scores, pwn_hip_align_statistics* statistics, float* records, int record_floats);

/* ---- scene maintenance (what follows the registration path in pwn_aligner.cpp:205-208 / pwn_merger.cpp:91-94) ---------------- */
/* The Gaussian half of PinholePointProjector::unProject(points, gaussians, index, depth) (pinholepointprojector.cpp:104-123; baseline
 * and alpha defaults :10-11) for a cloud made by pwn_hip_convert from the same depth image and parameters, followed by
 * Gaussian3fVector::transformInPlace(sensor_offset) (cloud.cpp:180).  The reference computes them inside every
 * DepthImageConverter::compute; only Merger::merge consumes them, so here they are produced on request. */
int pwn_hip_cloud_gaussians(pwn_hip_ctx* ctx, const pwn_hip_converter_params* p, const float* depth, int rows, int cols,
                            pwn_hip_cloud* cloud, float baseline, float alpha);
int pwn_hip_cloud_num_gaussians(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, int* n);       /* Cloud::gaussians().size() */
/* host arrays: mean n*3, cov n*9 (column-major 3x3), info_vec n*3, info n*9, flags n (1 = moments valid, 2 = information form valid:
 * the two lazily evaluated forms of basemath/gaussian.h:9-94); any pointer may be NULL */
int pwn_hip_cloud_download_gaussians(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, float* mean, float* cov, float* info_vec, float* info,
                                     int* flags);
/* Cloud::add (cloud.cpp:145-171): append a copy of `src` transformed by T (Cloud::transformInPlace) to `dst` */
int pwn_hip_cloud_add(pwn_hip_ctx* ctx, pwn_hip_cloud* dst, const pwn_hip_cloud* src, const float T[16]);
/* Merger::merge (merger.cpp:15-119).  K, min/max_distance: the projector of the merger's DepthImageConverter (merger.cpp:20-23),
 * T: its pose; thresholds: merger.cpp:6-8.  collapsed (optional, host, old size) receives Merger::_collapsedIndices. */
int pwn_hip_merge(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, const float K[9], const float T[16], float min_distance, float max_distance,
                  int rows, int cols, float distance_threshold, float normal_threshold, float max_point_depth, int* new_size,
                  int* collapsed);
/* Merger2::merge (pwn_tracker2/merger2.cpp:106-183) for clouds[0..n) in call order, as PwnMerger::mergeNodeList (pwn_tracker2/pwn_merger.cpp:28-62)
 * calls it for the nodes of a list: one submission on the context's stream, the host waits once at the end.  Cloud i is projected under the sensor
 * `offset` (:113-116) and `total` (Merger2::_cloud_tot) under transforms[16 i .. 16 i + 16) * offset (:121-127; the product is Isometry3f *
 * Isometry3f in float, pwn_hip_iso_mul; K, range and image size are the projector's).  A pixel whose depth d lies in (0.2, 100) appends the
 * cloud's point, transformed by transforms[i] with Cloud::add's per-point arithmetic and never its identity shortcut, with weight 1 / d where
 * `total` shows nothing (:134-149) or lies more than 0.3 behind (:164-177); where |d - depth of total| < 0.15 and d is inside the projector's range it
 * moves the total's point to the weighted mean with the pixel's unprojection (:153-162); the appended points follow in raster order of their
 * pixels.  `weights` (Merger2::_pesi_tot): one float per point of `total`, capacity-of-total floats, host or device memory, in / out.
 * appended / fused (host, n ints each, may be NULL): the pixels that took each action per cloud.  `total` gets explicit normal information
 * matrices, Stats (the default Stats() for a source without) and, when it or a source has them, Gaussians (the default Gaussian for a source
 * without), as pwn_hip_cloud_add gives them.  One deviation: the Stats block of an appended point is transforms[i] * the source point's own
 * block, what Cloud::add stores; the reference multiplies a member that holds the product of every earlier append (:139-143, :167-171).
 * Refused with `total`, `weights` and the counters untouched: a null argument, n < 0, a cloud of another context, `total` among the clouds,
 * clouds of different omega storages, an image larger than the context's, min_distance < 0, and -- PWN_HIP_ERR_CAPACITY, tested on the upper
 * bound size(total) + sum of size(clouds[i]) before any work -- a bound above the capacity of `total` or above 2^25.  n == 0 is a no-op. */
int pwn_hip_merge_clouds(pwn_hip_ctx* ctx, const float K[9], const float offset[16], int n, pwn_hip_cloud* const* clouds, const float* transforms,
                         float min_distance, float max_distance, int rows, int cols, pwn_hip_cloud* total, float* weights, int* appended,
                         int* fused);
/* ManifoldVoronoiExtractor::process (pwn_tracker2/manifold_voronoi_extractor.cpp:50-127): the traversability image of the last key clouds.
 * clouds[0..n) in call order (the deque, :76), cloud i under transforms[16 i .. 16 i + 16) (inT * cn->transform() as a float isometry, :81-85; the
 * per-point arithmetic of Cloud::transformInPlace, never its identity shortcut, which changes no integer computed here), are splatted into `image`,
 * x_size rows by y_size columns of uint16, host or device memory at any 2-byte alignment.  The image is filled with 30000 first (:72) unless
 * `accumulate` is not 0; the walk starts from the image's contents either way, so a list may be split over calls.  Per point, in list order and
 * then in index order (:87-121): cx = (int)(x_size * 0.5), cy likewise, ires = (float)(1. / resolution) (:54-56); x = (int)(cx + p.x * ires) is
 * the row and y = (int)(cy + p.y * ires) the column (:91-92, :99; product and sum rounded one by one, the conversion truncates toward zero);
 * outside the grid the point is skipped (:93-98); pz = (int)(10000 - 1000 * p.z) (:100); a cell that holds 65535 or a value below pz keeps it
 * (:101-108, an int comparison); so does every cell for a normal whose squared norm is below 0.1 (:109, compared in double); otherwise the cell
 * becomes 65535 where n.z < normal_threshold and (uint16)pz elsewhere (:113-120; the store is modular: a point above 10 m wraps, pz = -1 makes
 * an obstacle).  A float to int conversion of a NaN or of a magnitude >= 2^31 is undefined in the reference; such a coordinate gives no defined
 * cell or height here either.  inside (optional, host, n ints): the points of cloud i that fell inside the grid.  One submission on the
 * context's stream; the host waits once, at the end.  A list above 2^25 points runs as successive chunks of whole clouds that carry the image;
 * the bits are the same.  Refused with `image` and `inside` untouched: a null argument, n < 0, a cloud of another context, x_size or y_size <= 0,
 * x_size * y_size > 2^24, a resolution that is not finite or not positive, and -- PWN_HIP_ERR_CAPACITY -- a single cloud above 2^25 points.
 * n == 0 fills the image (unless `accumulate`) and returns. */
int pwn_hip_manifold_image(pwn_hip_ctx* ctx, int n, pwn_hip_cloud* const* clouds, const float* transforms /* n x 16 */,
                           float resolution, int x_size, int y_size, float normal_threshold,
                           int accumulate, uint16_t* image /* x_size rows x y_size cols, host or device */,
                           int* inside /* optional, host, n ints: points of cloud i that fell inside the grid */);
/* VoxelCalculator::compute (voxelcalculator.cpp:15-73): the first point of every voxel survives, output sorted by voxel indices
 * (the intended lexicographic order; the reference's IndexComparator, voxelcalculator.h:41-48, is not a strict weak ordering).
 * kept (optional, host) receives the original indices of the survivors in output order. */
int pwn_hip_voxelize(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, float resolution, int* new_size, int* kept);
/* Cloud::save / Cloud::load (cloud.cpp:11-136): "PWNCLOUD n binary" header, t2v(T) line, POINTWITHSTATS text records or the
 * reference's 176-byte binary records (object layout of Point / Normal / Stats, non-data bytes zeroed) */
int pwn_hip_cloud_save(pwn_hip_ctx* ctx, const pwn_hip_cloud* cloud, const char* filename, const float T[16], int step, int binary);
int pwn_hip_cloud_load(pwn_hip_ctx* ctx, pwn_hip_cloud* cloud, const char* filename, float T_out[16]);

/* ---- the mapping step (pwn_aligner.cpp:166-209, pwn_odometry_sequential_controller.cpp:124-171) ------------------------------ */
/* One frame of the mapping loop in one submission: the host queues everything on the context's stream and waits once.  In stream order:
 *   1. the frame is converted into `cloud`, scene-ready (Stats and sensor-noise Gaussians: pwn_hip_convert_batch_ex with both extras), behind
 *      DepthImage_scale when sp->step != 0 (step and max_depth_cov as in pwn_hip_convert_batch_ex);
 *   2. `scene` is rendered under scene_T * cp->sensor_offset (pwn_hip_iso_mul) into a depth image on the device (pwn_hip_project);
 *   3. that image is converted into `subscene` (pwn_hip_convert_batch);
 *   4. `subscene` (reference) is aligned against `cloud` (current) from the identity, as pwn_hip_align does it with the context's settings;
 *   5. one thread forms scene_T' = scene_T * Aligner::T() with the last row forced, the projector matrices of scene_T' * cp->sensor_offset and
 *      Cloud::add's identity test;
 *   6. Cloud::add(cloud, scene_T') on `scene` (pwn_hip_cloud_add) with the size of `cloud` read on the device;
 *   7. Merger::merge on `scene` (pwn_hip_merge) under scene_T' * cp->sensor_offset, with the projector of cp, the image size that was converted
 *      and sp's thresholds, on the size the add left.
 * The result is, byte for byte, what those seven calls give one after the other (total_time_ms apart).  rows, cols: the frame as the caller
 * holds it; ap->rows, ap->cols must be the size that is converted (rows / step, cols / step).  frame: float metres, or uint16 with depth_scale
 * when raw_u16 != 0; host or device memory.  scene_T: host, the scene pose before the frame.  collapsed (optional, host,
 * size(scene) + converted pixels ints): Merger::_collapsedIndices for the size the add left, -1 behind it.
 * A scene of size 0 is allowed (the reference's first frame: nothing is rendered, the pose stays the identity of the alignment).  If a
 * projection of the alignment gave up on a pixel the step leaves `scene` alone on the device and the call runs once more with the two-pass
 * projection, as pwn_hip_align does; after a converter time-out `scene` is untouched as well and the call returns PWN_HIP_ERR_LAUNCH.
 * Refused, the three clouds untouched: PWN_HIP_ERR_INVALID_ARGUMENT for a null argument, a scene that has fewer Gaussians than points, two
 * equal handles, a cloud of another context, clouds of different omega storages, an aligner image size that is not the converted one;
 * PWN_HIP_ERR_CAPACITY when size(scene) + converted pixels exceeds the scene's capacity or 2^25, or `cloud` / `subscene` hold fewer points
 * than the converted image has pixels. */
typedef struct pwn_hip_scene_step_params {
  float distance_threshold, normal_threshold, max_point_depth;   /* Merger (merger.cpp:6-8) */
  float baseline, alpha;                                         /* the Gaussians of `cloud`, as in pwn_hip_convert_extras */
  int step; float max_depth_cov;                                 /* DepthImage_scale in front of the conversion; step 0: the frame as it is */
} pwn_hip_scene_step_params;
typedef struct pwn_hip_scene_step_result {
  pwn_hip_align_result align;
  float scene_T[16];                                             /* the scene pose after the frame */
  int n_cloud, n_subscene;                                       /* points of `cloud` and `subscene` */
  int size_after_add, size_after_merge;                          /* points of `scene` */
} pwn_hip_scene_step_result;
void pwn_hip_default_scene_step_params(pwn_hip_scene_step_params* p);
int pwn_hip_scene_step(pwn_hip_ctx* ctx, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, const pwn_hip_scene_step_params* sp,
                       const void* frame, int raw_u16, float depth_scale, int rows, int cols, const float scene_T[16], pwn_hip_cloud* scene,
                       pwn_hip_cloud* cloud, pwn_hip_cloud* subscene, pwn_hip_scene_step_result* result, int* collapsed);

/* ------------------------------------------------------------------ multi-stream tracker ------ */
/* PwnTracker::processFrame (pwn_tracker/pwn_tracker.cpp:106-215) for S independent depth streams that advance in lock-step: frame f of every
 * stream, then frame f + 1 of every stream -- each step one batch of up to S (key cloud, frame) pairs -- and a run of F frames per stream in ONE
 * submission with ONE host wait.  What the tracker does between two alignments runs on the device: the guess _previousCloudTransform^-1 * _globalT *
 * initialGuess (:132) and the pairs' initial states in front of a step's alignment kernels, the pose chain (:147-150), the re-orthonormalisation
 * of every 50th frame (:154-159), the key-cloud decision (:164-185) and the switch of the reference cloud behind them.
 * The tracker belongs to its context: pwn_hip_ctx_destroy releases the clouds and device records of the trackers that are left, and such a handle is
 * then good for pwn_hip_tracker_destroy alone (every other call refuses it), so either order of destruction is safe.  It owns, per stream, a ring of frames_per_call_max + 1 clouds of
 * (rows / step) * (cols / step) points -- ordinary lean clouds of the context, as pwn_hip_convert_batch_u16_scaled fills them -- and one state
 * record on the device.  A key switch moves no cloud: the state names the slot.  rows, cols: the size of the frames; step: DepthImage_scale's
 * (>= 1; PwnMatcherBase::_scale).  Refused: streams < 1 or above the context's max_batch (PWN_HIP_ERR_CAPACITY), frames_per_call_max < 1, a
 * frame larger than the context's, an empty scaled image. */
typedef struct pwn_hip_tracker pwn_hip_tracker;
/* The state of one stream: what PwnTracker keeps between two frames.  key_slot = -1: no key cloud (PwnTracker::init(), :38-49, with the other
 * fields at their initial values: identities and zeros).  sensor_offset is _previousCloudOffset as the stream recorded it with its first key cloud
 * (:194-200); it is kept for the caller and not read by the alignment (see pwn_hip_track_frames). */
typedef struct pwn_hip_tracker_state {
  float globalT[16];
  float previous_cloud_transform[16];
  float sensor_offset[16];
  int   counter;
  int   num_keyframes;
  int   key_slot;                  /* slot of the stream's ring that holds the key cloud, 0 .. frames_per_call_max; -1: none */
  int   reserved;
} pwn_hip_tracker_state;
/* What processFrame reports for one frame of one stream.  A first frame (no key cloud before it): new_frame = 1, aligned = 0, the rest of the
 * alignment's fields zero.  A stream that idled in a step (NULL frame): all zero. */
typedef struct pwn_hip_track_result {
  int   new_frame;                 /* the frame became the stream's key cloud */
  int   aligned;
  int   inliers;                   /* Aligner::inliers() */
  float error;                     /* Aligner::error() */
  float T[16];                     /* Aligner::T() */
  float globalT[16];               /* _globalT after the frame */
  float inliers_fraction;          /* (float) inliers / (float) (view rows * view cols) (:163) */
  int   n_points;                  /* points of the frame's cloud */
} pwn_hip_track_result;
int pwn_hip_tracker_create(pwn_hip_ctx* ctx, int streams, int frames_per_call_max, int rows, int cols, int step, pwn_hip_tracker** tracker);
int pwn_hip_tracker_destroy(pwn_hip_tracker* tracker);
/* The states of the streams [first, first + n), as the last call (or set_state) left them.  set_state with key_slot >= 0 is refused unless that
 * slot of the stream's ring holds a cloud; a refused call changes nothing.  set_state waits for the context's queued work. */
int pwn_hip_tracker_get_state(pwn_hip_tracker* tracker, int first, int n, pwn_hip_tracker_state* states);
int pwn_hip_tracker_set_state(pwn_hip_tracker* tracker, int first, int n, const pwn_hip_tracker_state* states);
/* The cloud that is stream s's key cloud after the last call: a borrowed handle (the tracker owns it and a later call may overwrite it), for
 * pwn_hip_cloud_download and tests; NULL while the stream has none. */
int pwn_hip_tracker_key_cloud(pwn_hip_tracker* tracker, int s, pwn_hip_cloud** cloud);
/* processFrame for frame 0 of every stream, then frame 1 of every stream, ... frame F - 1: frames[f * S + s] (raw uint16, rows x cols, ALL host or ALL
 * device memory) is frame f of stream s; NULL = the stream has no frame in that step and idles (its state, counter included, does not move).
 * Per frame: makeCloud's data path as pwn_hip_convert_batch_u16_scaled runs it (depth = depth_scale * raw, DepthImage_scale(step, max_depth_cov), the
 * converter) into a free slot of the stream's ring; then the alignment against the stream's key cloud and the tracker's bookkeeping, or, for a
 * stream without a key cloud, the frame's cloud taken as the key without an alignment (:194-200).  initial_guesses: F * S column-major 4x4, or NULL
 * (identities).  new_frame_inliers_fraction: PwnTracker::_newFrameInliersFraction (0.4, :36); the fraction is compared with it in float, as the
 * reference's float members are.  results: F * S records, results[f * S + s].
 * K, image size, converter and aligner parameters are the call's, as everywhere in this ABI, and so is the SENSOR OFFSET: the aligner's kernels take
 * one reference offset per call, so a tracker tracks streams of ONE sensor offset -- cp->sensor_offset for the conversions,
 * ap->reference_sensor_offset and ap->current_sensor_offset (the same matrix for PwnTracker's use, :194-200) for the alignments.
 * ap->initial_guess is not read.  The convergence setting (pwn_hip_ctx_set_convergence) is honoured as in every batch call.
 * The conversions of all steps are queued on a stream of their own, so step f + 1 converts beside step f's alignment; a step's pairs run in the
 * sub-batches and on the streams of a batch alignment (pwn_hip_ctx_set_subbatch, _set_concurrency); results do not depend on either.
 * A projection that gives up on a pixel (see pwn_hip_align_batch_records, word 63) or a converter strip whose hand-over times out makes the
 * library run the whole call once more from the states it started with.  Bit for bit, every stream's results, state and key cloud are those
 * of pwn_hip_convert_scaled + pwn_hip_align per frame with the host-side bookkeeping in between (what api.PwnTracker does).
 * Refused, nothing touched (states, clouds, results): a null argument (initial_guesses apart), a tracker of another context, F outside
 * 1 .. frames_per_call_max, more streams than the context's max_batch, ap->rows x ap->cols other than (rows / step) x (cols / step), what every
 * alignment call refuses in ap, frames of mixed host and device memory. */
int pwn_hip_track_frames(pwn_hip_ctx* ctx, pwn_hip_tracker* tracker, const pwn_hip_converter_params* cp, const pwn_hip_aligner_params* ap, int F,
                         const uint16_t* const* frames, float depth_scale, float max_depth_cov, const float* initial_guesses,
                         float new_frame_inliers_fraction, pwn_hip_track_result* results);
/* The host compilation of what the device does with one alignment's result (no context): from *state and initial_guess (NULL: identity) the
 * guess of :132, then with the aligner's T and inliers the pose chain, the re-orthonormalisation when counter % 50 == 0, the forced last row, the
 * key-cloud decision against `threshold` (on a switch key_slot = slot, previous_cloud_transform = globalT, num_keyframes + 1) and counter + 1.
 * *state is updated, *result filled (error and n_points are left zero). */
void pwn_hip_track_pose_update(pwn_hip_tracker_state* state, const float initial_guess[16], const float T[16], int inliers, int pixels,
                               float threshold, int slot, pwn_hip_track_result* result);

/* ------------------------------------------------------------------ helpers ------------------ */
/* PinholePointProjector::_updateMatrices (pinholepointprojector.cpp:17-31): KRt, iKRt (4x4), iK (3x3) */
void pwn_hip_projector_matrices(const float K[9], const float T[16], float KRt[16], float iKRt[16], float iK[9]);
/* The single-point forms of the projector (host code; the very expressions the kernels evaluate, so a point projected here lands on the pixel
 * pwn_hip_project gives it):
 *   PinholePointProjector::project(x, y, f, p)      (pinholepointprojector.h:174, _project :224-233): 1 = valid (depth inside [min, max]); the image
 *                                                   bounds are the caller's test, as in the reference (pinholepointprojector.cpp:51-55);
 *                                                   a rounded coordinate an int cannot hold is returned as +-2147483520, a NaN as INT_MIN
 *   PinholePointProjector::unProject(p, x, y, d)    (:187, _unProject :246-251): 1 = valid; x = column, y = row (pinholepointprojector.cpp:112)
 *   PinholePointProjector::projectInterval(x,y,d,R) (:200, _projectInterval :264-274): -1 for a depth outside [min, max] */
int pwn_hip_project_point(const float K[9], const float T[16], float min_distance, float max_distance, const float p[3], int* x, int* y, float* d);
int pwn_hip_unproject_pixel(const float K[9], const float T[16], float min_distance, float max_distance, int x, int y, float d, float p[3]);
int pwn_hip_project_interval(const float K[9], float min_distance, float max_distance, float d, float world_radius);
/* Eigen::Isometry3f::inverse() and Isometry3f * Isometry3f with the evaluation order the CPU path has (host code) */
void pwn_hip_iso_inverse(const float T[16], float out[16]);
void pwn_hip_iso_mul(const float A[16], const float B[16], float out[16]);
/* bm_se3.h:37-52 */
void pwn_hip_v2t(const float v[6], float T[16]);
void pwn_hip_t2v(const float T[16], float v[6]);
/* Matrix6f::ldlt().solve(b) as aligner.cpp:110 calls it (column-major H, lower triangle read): the host compilation of the
 * function k_solve_update runs on the device */
void pwn_hip_ldlt_solve6(const float H[36], const float b[6], float x[6]);
/* per-kernel device time (ms) of the stages of the last batch/single call, for bench.py:
 * names: "unproject","integral","integral_rows","integral_cols","stats","project_cur","project_ref","corr_linearize","solve",
 * "statistics","match_score" ("project": the stand-alone pwn_hip_project; "project_depth_batch","merge_depth_images": the merged closure).  launches = timed launch groups (one per sub-batch). */
int pwn_hip_last_stage_ms(pwn_hip_ctx* ctx, const char* stage, float* ms, int* launches);
/* what this GPU's HBM delivers, for the roofline report (SURVEY 8(d) asks for the measured figure next to the 8 TB/s spec):
 * float4 streaming read and device-to-device copy of `bytes` (use >= 1 GiB: the Infinity Cache holds 256 MiB), best of 5,
 * GB/s; the copy counts bytes read + written.  Allocates and frees 2 x bytes. */
int pwn_hip_measure_hbm(pwn_hip_ctx* ctx, size_t bytes, float* read_gbps, float* copy_gbps);
/* enable/disable hipEvent timing around every kernel launch (adds host overhead; default off) */
int pwn_hip_set_profiling(pwn_hip_ctx* ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif
