/*
 * gslam_hip.h — plain-C ABI of libgslam_hip.so: the MI355X (gfx950) hot path of GSLAM.
 *
 * This is the drop-in boundary underneath the GSLAM plugin shims (libgslam_optimizer.so,
 * libgslam_featuredetector.so).  Everything here is `extern "C"`, plain pointers + sizes,
 * POD structs, int status codes, no exceptions, no torch / C++ types.
 *
 * Reference interfaces each entry point stands in for (paths relative to the GSLAM tree):
 *   gh_bf_*      GSLAM/core/Vocabulary.h:485-491  (DistanceFactory::hamming32: 4 x u64 XOR + popcount)
 *                GSLAM/core/Vocabulary.h:1712-1725 (first strict minimum wins ties -> lowest index)
 *                GSLAM/core/Map.h:252-258         (FrameConnection::getMatches vector<pair<int,int>>)
 *   gh_orb_*     GSLAM/core/Map.h:122-195         (KeyPoint, 28-byte POD == gh_keypoint)
 *                GSLAM/core/Map.h:309-321         (MapFrame::setKeyPoints(kps, N x 32 8UC1 GImage))
 *                GSLAM/core/GImage.h:160-190,378-382 (dense row-major u8 image / descriptor matrix)
 *   gh_ba_*      GSLAM/core/Optimizer.h:102-182   (BundleGraph, BundleEdge, KeyFrameEstimzation,
 *                                                  MapPointEstimation, OptimzeConfig)
 *                GSLAM/core/Optimizer.h:229       (Optimizer::optimize(BundleGraph&))
 *                GSLAM/core/Optimizer.h:202-207   (Optimizer::optimizePnP)
 *                GSLAM/core/SE3.h:100-103,257-287 (inverse / exp used by the pose update)
 *
 * Conventions
 *   - `*_dev` pointers are DEVICE (HBM) addresses; everything else is host memory.
 *   - Every call enqueues on the context's stream; `gh_ctx_sync` waits for it.  Host-buffer
 *     convenience entry points (`*_host`) synchronise before returning.
 *   - One gh_ctx per host thread; a ctx may be created on one thread and used on another
 *     (GSLAM constructs optimizers on one thread and calls them on Messenger workers).
 *   - No CPU fallback exists: every entry point fails with GH_ERR_HIP if the device is absent.
 */
#ifndef GSLAM_HIP_H_
#define GSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_ctx gh_ctx;

typedef enum gh_status {
  GH_OK = 0,
  GH_ERR_ARG = 1,      /* bad argument (null pointer, negative size, capacity overflow) */
  GH_ERR_HIP = 2,      /* a HIP runtime call failed; see gh_last_error */
  GH_ERR_NOMEM = 3,    /* device or host allocation failed */
  GH_ERR_NUMERIC = 4,  /* BA: reduced system not positive definite even at maximum damping */
  GH_ERR_UNSUPPORTED = 5
} gh_status;

/* ------------------------------------------------------------------ context ---------- */
int gh_abi_version(void); /* bumps when a struct in this header changes layout or entry points change meaning; 2 since round 5
                             (GH_ABI_VERSION below is what this header describes: a host compares the two at start-up) */
#define GH_ABI_VERSION 2
gh_status gh_ctx_create(int device, gh_ctx** out);
void gh_ctx_destroy(gh_ctx* ctx);
const char* gh_last_error(const gh_ctx* ctx);
/* Use an externally owned hipStream_t (e.g. the caller's current stream).  NULL is the legacy
 * default stream (what torch's default stream is); gh_ctx_use_own_stream restores the private one. */
gh_status gh_ctx_set_stream(gh_ctx* ctx, void* hip_stream);
/* Frees what the context has grown for past calls (device scratch, pinned staging, the arenas of gh_ba_solve and of the
 * graph solvers): a single large graph would otherwise pin its high-water mark for the life of the context.  Waits for the
 * context's stream; everything is re-grown on demand; gh_ba_graph objects own their memory and are not touched. */
gh_status gh_ctx_trim(gh_ctx* ctx);
/* Linear solver of the reduced camera system in gh_ba_solve / gh_ba_graph_solve: GH_BA_SOLVER_AUTO (default) takes the
 * band solver (block cyclic reduction, chol_cr.hip) when every point is seen from cameras at most 31 indices apart, the
 * system has at least four superblocks of 64 * ceil((6 span + 5) / 64) columns, else the
 * dense MFMA factorisation; _DENSE forces the dense path (what BASELINE's C5 names); _BAND asks for the band solver and
 * falls back to dense when the graph is not a band.  The test is made on the solver's own camera order (gh_ba_camera_order),
 * not on the caller's.  LOOP CLOSURES: under _AUTO / _BAND the cameras that long-range points
 * tie to far-away cameras (at most 1024 of them) are numbered last inside the solver, and the system is solved as a band +
 * dense border (GH_BA_SOLVER_ARROW in gh_ctx_last_ba_solver; gh_arrow_solve_dev) instead of falling to the dense path.
 * The environment variable GSLAM_HIP_BA_SOLVER=dense|band|auto overrides it (A/B measurements). */
#define GH_BA_SOLVER_AUTO 0
#define GH_BA_SOLVER_DENSE 1
#define GH_BA_SOLVER_BAND 2
#define GH_BA_SOLVER_ARROW 3 /* reported only: band + dense border */
gh_status gh_ctx_set_ba_solver(gh_ctx* ctx, int solver);
/* What the last gh_ba_solve / gh_ba_graph_solve on this context used: GH_BA_SOLVER_DENSE or _BAND (0 before the first
 * solve); *band_tiles = 64-column tiles per superblock of the band solver (0 for dense), *cam_span = the largest distance
 * in camera indices between two observers of one point -- border cameras of the arrow ordering left out -- (the
 * half-bandwidth of the band part is 6 * span + 5).
 * Either pointer may be NULL. */
int gh_ctx_last_ba_solver(gh_ctx* ctx, int* band_tiles, int* cam_span);
/* The camera order behind that solve (round 6): *border_cams = cameras of the arrowhead border (0 for band / dense),
 * *reordered = 1 when the solver replaced the caller's camera order by its own bandwidth-reducing order (gh_ba_camera_order).
 * Returns 1 after a solve, 0 before the first.  Either pointer may be NULL. */
int gh_ctx_last_ba_order(gh_ctx* ctx, int* border_cams, int* reordered);
int gh_ctx_last_ba_border_points(gh_ctx* ctx); /* long-range points in the border of that solve (0: a camera border or none) */
gh_status gh_ctx_use_own_stream(gh_ctx* ctx);
void* gh_ctx_stream(gh_ctx* ctx);
gh_status gh_ctx_sync(gh_ctx* ctx);
/* Device facts as the runtime reports them. */
gh_status gh_device_info(gh_ctx* ctx, int* cu_count, int* clock_khz, size_t* hbm_bytes, char* name, int name_cap);

/* Raw device memory helpers, so C/C++ hosts need no HIP headers. */
gh_status gh_dev_alloc(gh_ctx* ctx, size_t bytes, void** out_dev);
gh_status gh_dev_free(gh_ctx* ctx, void* dev);
gh_status gh_dev_upload(gh_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
gh_status gh_dev_download(gh_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
gh_status gh_dev_memset(gh_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* Live per-kernel timing with HIP events on the context's stream (bench.py's roofline). */
typedef struct gh_prof_entry {
  char name[48];
  uint64_t launches;
  double total_ms;
} gh_prof_entry;
gh_status gh_prof_enable(gh_ctx* ctx, int on); /* on=1 also clears accumulated entries */
/* Resolves pending events (synchronises), writes up to cap entries, returns count in *n. */
gh_status gh_prof_collect(gh_ctx* ctx, gh_prof_entry* out, int cap, int* n);

/* ------------------------------------------------------------------ BF matcher ------- */
/* 256-bit descriptors, 32 bytes each, dense rows (GImage N x 32, 8UC1).
 * For query i:  idx1[i] = argmin_j hamming(q_i, t_j), first minimum (lowest j) on ties;
 *               d1[i]   = that distance; d2[i] = min over j != idx1[i] (65535 if nt < 2).
 * nt == 0  ->  idx1 = -1, d1 = d2 = 65535.   Any nt: train sets beyond 65535 rows (a frame against a local map) are swept
 * in chunks and folded with the same strict '<', so the result is the one of a single sweep.  (The batched pair entries
 * below keep cap <= 65535: their rows are frames.) */
gh_status gh_bf_match_dev(gh_ctx* ctx, const uint8_t* q_dev, int nq, const uint8_t* t_dev, int nt,
                          int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);
gh_status gh_bf_match_host(gh_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                           int32_t* idx1, uint16_t* d1, uint16_t* d2);

/* Batched over frame pairs.  desc_dev: F frames x cap rows x 32 B; counts_dev[f] <= cap valid rows.
 * Pair p matches frame pair_q[p] (queries) against frame pair_t[p] (train).
 * Outputs are P x cap (rows >= counts[pair_q[p]] get idx1 = -1, d = 65535).
 * Dispatches on the amount of pair work: small batches run the popcount kernel (gh_bf_match_pairs_popc_dev), batches
 * that fill the chip the exact MFMA formulation (gh_bf_match_pairs_mfma_dev); the results are bit-identical. */
gh_status gh_bf_match_pairs_dev(gh_ctx* ctx, const uint8_t* desc_dev, const int32_t* counts_dev, int cap,
                                const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs,
                                int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);

/* The same matchers for descriptors of ANY width that is a multiple of 8 bytes (8 .. 256): the reference chooses its distance
 * by the descriptor's width -- GSLAM/core/Vocabulary.h:565-567: hamming32 for 32 bytes, hamming64 (:493-500) for 64,
 * hamming8x (:502-513) for other multiples of 8 -- and so do these entries (32 bytes run the kernels above, MFMA formulation
 * included).  Same outputs, same first-minimum rule; train sets beyond 65535 rows are swept in chunks for every width (round 6). */
gh_status gh_bf_match_bytes_dev(gh_ctx* ctx, const uint8_t* q_dev, int nq, const uint8_t* t_dev, int nt, int desc_bytes,
                                int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);
gh_status gh_bf_match_bytes_host(gh_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int desc_bytes, int32_t* idx1,
                                 uint16_t* d1, uint16_t* d2); /* host arrays in and out, like gh_bf_match_host */
gh_status gh_bf_match_pairs_bytes_dev(gh_ctx* ctx, const uint8_t* desc_dev, const int32_t* counts_dev, int cap, int desc_bytes,
                                      const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, int32_t* idx1_dev,
                                      uint16_t* d1_dev, uint16_t* d2_dev);

/* The popcount formulation, always (north_star's contract kernel: v_xor + v_bcnt, GSLAM/core/Vocabulary.h:485-491 as
 * written; the kernel bench.py prices against the VALU issue ceiling). */
gh_status gh_bf_match_pairs_popc_dev(gh_ctx* ctx, const uint8_t* desc_dev, const int32_t* counts_dev, int cap,
                                     const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs,
                                     int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);

/* The same contract through an exact integer MFMA formulation, always: hamming = |a| + |b| - 2 |a & b| with |a & b| as a
 * dot product of the descriptors expanded to one byte per bit on v_mfma_i32_16x16x64_i8; three VALU instructions per
 * pair instead of nineteen.  Results are bit-identical to gh_bf_match_pairs_popc_dev. */
gh_status gh_bf_match_pairs_mfma_dev(gh_ctx* ctx, const uint8_t* desc_dev, const int32_t* counts_dev, int cap,
                                     const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs,
                                     int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);

/* Match masks (integer only):  keep[i] = d1 <= max_dist  &&  d1 * ratio_den < ratio_num * d2
 *                                        && (!cross_check || back_idx1[idx1[i]] == i).
 * ratio_num <= 0 disables the ratio test.  back_idx1_dev may be NULL when cross_check == 0. */
gh_status gh_match_mask_dev(gh_ctx* ctx, const int32_t* idx1_dev, const uint16_t* d1_dev,
                            const uint16_t* d2_dev, int nq, const int32_t* back_idx1_dev, int nt,
                            int max_dist, int ratio_num, int ratio_den, int cross_check,
                            uint8_t* keep_dev);

/* VALU ceiling probe: runs a register-resident xor+popcount chain and reports the measured
 * rate in 256-bit pair-equivalents per second (16 VALU ops each). */
gh_status gh_bf_valu_probe(gh_ctx* ctx, double* pairs_per_s);

/* Issue-rate probes per VALU instruction class of the ORB / matcher inner loops (register-only chains, 8 waves per
 * SIMD): wave-instructions per second over the whole device for op = 0, 1, ... ; GH_ERR_ARG past the last op.  name (may
 * be NULL) receives the instruction class.  bench.py reports them as the MEASURED issue ceiling of the VALU-bound
 * kernels instead of an assumed cycles-per-instruction figure. */
gh_status gh_valu_issue_probe(gh_ctx* ctx, int op, double* wave_insts_per_s, char* name, int name_cap);

/* Host only (no GPU needed): the 32-bit multiplier m with (n * m) >> 32 == n / d for EVERY n <= n_max, or 0 when no such
 * constant is guaranteed (the kernels then divide).  orb_fast_cells turns its tile id into (frame, tile row, tile column)
 * with two of these instead of two integer divisions per wave; exported so that the guarantee can be tested exhaustively. */
uint32_t gh_magic_div(uint32_t d, uint32_t n_max);

/* ------------------------------------------------------------------ ORB front end ---- */
/* Layout-identical to GSLAM::KeyPoint (GSLAM/core/Map.h:122-195, sizeof == 28). */
typedef struct gh_keypoint {
  float x, y;     /* level-0 pixel coordinates */
  float size;     /* 31 * scale^octave */
  float angle;    /* degrees, [0,360]: a multiple of 12 (30 orientation bins), or continuous (gh_orb_plan_set_steering) */
  float response; /* FAST corner score */
  int32_t octave;
  int32_t class_id; /* -1 */
} gh_keypoint;

/* Row-band restricted variant for stereo left-right matching (BASELINE configs[2]): train row j is a
 * candidate of query i only if |kps[i].y - kps[j].y| <= kps[i].size * band_per_size (single fp32 multiply).
 * kps_dev: F x cap gh_keypoint records parallel to desc_dev.  Outputs as gh_bf_match_pairs_dev. */
gh_status gh_bf_match_band_pairs_dev(gh_ctx* ctx, const uint8_t* desc_dev, const gh_keypoint* kps_dev,
                                     const int32_t* counts_dev, int cap, const int32_t* pair_q_dev,
                                     const int32_t* pair_t_dev, int npairs, float band_per_size,
                                     int32_t* idx1_dev, uint16_t* d1_dev, uint16_t* d2_dev);

typedef struct gh_orb_params {
  int32_t n_features;   /* K: total keypoint quota per frame (default 1000) */
  int32_t n_levels;     /* pyramid levels, 1..8 (default 8); scale factor fixed at 1.2 */
  int32_t ini_th_fast;  /* default 20 */
  int32_t min_th_fast;  /* default 7 */
} gh_orb_params;
void gh_orb_default_params(gh_orb_params* p);

typedef struct gh_orb_plan gh_orb_plan; /* owns pyramid + workspace for (w, h, batch) */
gh_status gh_orb_plan_create(gh_ctx* ctx, int width, int height, int max_batch,
                             const gh_orb_params* params, gh_orb_plan** out);
void gh_orb_plan_destroy(gh_orb_plan* plan);
/* Replace the plan's BRIEF test pattern: 256 tests x (ax, ay, bx, by) int8, relative to the keypoint, unrotated.  The
 * 30-bin steered look-up table is rebuilt from it (12-degree steps, round half away from zero).  Lets a deployer load
 * the canonical ORB / ORB-SLAM `bit_pattern_31_` (after gh_orb_plan_set_steering(plan, 1): it has points of radius 18.4) so
 * that descriptors are compatible with existing ORB vocabularies; the built-in default is a seeded pattern of this
 * repository (the canonical table is not available offline).  In the 30-bin mode every rotated point must stay inside the
 * +-13 px blurred patch (radius <= 13.49), in the continuous mode inside radius 19.49; otherwise GH_ERR_ARG. */
gh_status gh_orb_plan_set_pattern(gh_orb_plan* plan, const int8_t* pattern_256x4);
/* Orientation / steering mode.  0 (default): 30 orientation bins of 12 degrees with a precomputed rotated pattern per
 * bin, KeyPoint.angle a multiple of 12.  1: continuous -- angle = the fp32 polynomial arctangent of OpenCV's fastAtan2
 * (what ORB-SLAM's IC_Angle calls) on the same integer moments, every test point rotated by that angle and rounded to the
 * nearest pixel (ties to even, as cvRound): the steering of OpenCV / ORB-SLAM's computeOrbDescriptor.  In this mode
 * gh_orb_plan_set_pattern takes points up to radius 19.49 (the canonical ORB `bit_pattern_31_` reaches (-13, -13)), the
 * 7x7 blur reads up to 22 px from the keypoint and pixels beyond the image border are mirrored (BORDER_REFLECT_101, what
 * ORB-SLAM's padded pyramid holds there).  With the canonical pattern installed the descriptors are the ones ORB
 * vocabularies were trained on up to the image arithmetic (integer pyramid / FAST score / blur here, float there). */
gh_status gh_orb_plan_set_steering(gh_orb_plan* plan, int mode);
/* Keypoint distribution.  0 (default): 32 x 32 cells, in-cell rank, per-level quota by rank order (oracle steps 3-5; the
 * throughput path).  1: what ORB-SLAM's ORBextractor does (ComputeKeyPointsOctTree + DistributeOctTree) -- FAST per ~30 x 30
 * cell (W' = w - 32: nCols = W' / 30, wCell = ceil(W' / nCols)) with non-maximum suppression INSIDE the cell and the
 * cell's own fall-back from ini_th_fast to min_th_fast, every surviving corner a candidate (no per-cell cap), then per
 * (frame, level) the quadtree: nodes split into four until there are n_l of them (largest first in the last stage), the
 * strongest corner of each node kept.  Specification: oracle/orb_oracle.c steps 4' and 5' (bit-exact; ties that ORB-SLAM
 * leaves to heap addresses are fixed there).  Output rows per level are in (y, x) order.  Limits: levels up to 4096 x 4096,
 * per-level quota <= 2045.  The candidate lists hold the exact worst case (one strict maximum per 2 x 2 pixels of a cell) while
 * that fits 4 GB over max_batch frames (1080p: up to ~400 frames per call) and calls are asynchronous like the default mode's;
 * a plan whose budget had to cut the lists makes every call wait for its kernels, and a frame with more FAST maxima than a
 * list holds fails with GH_ERR_NOMEM, never silently.
 * Together with gh_orb_plan_set_steering(plan, 1) and the canonical pattern this is the ORB-SLAM extraction up to the image
 * arithmetic (integer pyramid and blur here, float resize there; KeyPoint.response = FAST score, OpenCV's is score - 1). */
gh_status gh_orb_plan_set_distribution(gh_orb_plan* plan, int mode);
/* The threshold hint of large calls (the per-level schedule with ini_th_fast > min_th_fast; every other call ignores it).
 * The detector may score a (level, frame) at any threshold T >= ini_th_fast first: where at least `quota` cells hold a
 * corner above T the output does not depend on T, and where they do not the level is redone from min_th_fast.  So T is
 * advice: it changes the time a call takes and not one output byte.
 *   GH_ORB_HINT_ADAPTIVE (default)  per (level, batch slot) the plan keeps a T that every call derives from the score at
 *                                   its quota cut, for the next call on that slot: good while a slot sees similar images
 *                                   call after call (a camera).  A redo is slow (one workgroup per level and frame), so
 *                                   after one the whole plan stays at ini_th_fast for 2, 4, .. 64 calls, and then goes
 *                                   above it in every other call only until calls that hold have worked the penalty off
 *   GH_ORB_HINT_OFF                 always ini_th_fast (also: GSLAM_HIP_ORB_HINT=0 in the environment)
 *   GH_ORB_HINT_FORCED              every level and slot at max(value, ini_th_fast), value <= 255; nothing is updated */
#define GH_ORB_HINT_ADAPTIVE 0
#define GH_ORB_HINT_OFF 1
#define GH_ORB_HINT_FORCED 2
gh_status gh_orb_plan_set_threshold_hint(gh_orb_plan* plan, int mode, int value);
/* Test access: the adaptive T of every (batch slot, level), max_batch x 8 bytes to host; waits for the plan's stream. */
gh_status gh_orb_plan_debug_hints(gh_orb_plan* plan, uint8_t* out_host);
/* Level geometry of the plan, for tests. */
gh_status gh_orb_plan_level(const gh_orb_plan* plan, int level, int* w, int* h, int* quota);
size_t gh_orb_plan_device_bytes(const gh_orb_plan* plan);

/* Extract from `batch` gray u8 frames resident in HBM (frame f at gray_dev + f*frame_stride,
 * rows `row_stride` bytes apart).  Outputs, each with capacity K = params.n_features per frame:
 *   kps_dev  batch x K gh_keypoint, desc_dev batch x K x 32 B, counts_dev batch int32.
 * A 16-byte aligned buffer (pointer, row_stride, frame_stride) is read in place, in 16-byte windows over the whole
 * row_stride x height extent of every frame: the padding of the rows must be allocated.  For a single frame whose
 * allocation ends at (height-1) * row_stride + width (an ROI view) pass batch = 1 and frame_stride = 0: the frame
 * is then copied row by row into the plan's own pyramid slab first. */
gh_status gh_orb_extract_dev(gh_orb_plan* plan, const uint8_t* gray_dev, int batch, size_t frame_stride,
                             int row_stride, gh_keypoint* kps_dev, uint8_t* desc_dev, int32_t* counts_dev);
/* Single host frame convenience (uploads, extracts, downloads, synchronises). */
gh_status gh_orb_extract_host(gh_orb_plan* plan, const uint8_t* gray, int row_stride, gh_keypoint* kps,
                              uint8_t* desc, int32_t* count);
/* Fixed-point luma (B*1868 + G*9617 + R*4899 + 8192) >> 14 for 3- or 4-channel BGR(A) input. */
gh_status gh_bgr_to_gray_dev(gh_ctx* ctx, const uint8_t* bgr_dev, int width, int height, int channels,
                             int src_row_stride, uint8_t* gray_dev, int dst_row_stride);
/* The same for n_frames frames laid out src_frame_stride / dst_frame_stride bytes apart (one launch). */
gh_status gh_bgr_to_gray_batch_dev(gh_ctx* ctx, const uint8_t* bgr_dev, int width, int height, int channels,
                                   int src_row_stride, size_t src_frame_stride, int n_frames, uint8_t* gray_dev,
                                   int dst_row_stride, size_t dst_frame_stride);

/* ---- Host-fed streaming extraction: frames arrive in HOST memory, results are wanted in HOST memory -------------------
 * What a GSLAM process sees: a dataset / camera thread hands over frames one by one (GSLAM/plugins/play/main.cpp:99-155)
 * and MapFrame::setKeyPoints wants std::vector<KeyPoint> + an N x 32 descriptor matrix on the host (GSLAM/core/Map.h:
 * 309-321).  A ring of `depth` slots of up to `chunk_frames` frames each; per submit ONE flat host-to-device DMA, the
 * extraction, and a pack kernel that writes per-frame offsets + only the valid records straight into pinned host memory --
 * on three HIP streams chained by events, so the copies of neighbouring chunks run under the kernels of this one.  No
 * torch, no Python: this is the entry a C++ host uses.  Frame layout is fixed per stream: `channels` interleaved u8
 * (1 gray, 3 BGR, 4 BGRA: luma as gh_bgr_to_gray_dev), rows row_stride bytes apart, frames frame_stride bytes apart.
 *   gh_orb_stream_staging  pinned staging block (chunk_frames x frame_stride bytes) of the slot the NEXT submit uses: a
 *                          producer that decodes / captures straight into it saves the host copy (submit with NULL).
 *   gh_orb_stream_submit   frames_host = NULL (the staging block) or the caller's own buffer (pinned: DMA in place;
 *                          pageable: the runtime stages it and the call returns when that is done).  Returns at once
 *                          otherwise; blocks only while the slot's previous ticket (ticket - depth) is still running.
 *                          The results of ticket t are overwritten by ticket t + depth: collect before that.
 *   gh_orb_stream_collect  waits for the ticket; *out points into the slot's pinned result block (valid until the slot
 *                          is reused): frame f owns records offsets[f] .. offsets[f + 1] - 1 of kps / desc.
 *                          Thread-safe against a concurrent submit (producer / consumer threads).
 *   gh_orb_stream_poll     *ready = 1 when collect would not block. */
typedef struct gh_orb_stream gh_orb_stream;
typedef struct gh_orb_stream_result {
  int32_t n_frames;
  const int32_t* offsets;   /* n_frames + 1 */
  const gh_keypoint* kps;   /* offsets[n_frames] records, frame after frame */
  const uint8_t* desc;      /* offsets[n_frames] x 32 B */
  float gpu_ms;             /* first byte on the link -> last result byte in host memory, for this ticket */
} gh_orb_stream_result;
gh_status gh_orb_stream_create(gh_ctx* ctx, int width, int height, int channels, int row_stride, size_t frame_stride,
                               int chunk_frames, int depth, const gh_orb_params* params, gh_orb_stream** out);
void gh_orb_stream_destroy(gh_orb_stream* stream);
/* The extraction plan behind the stream (owned by it), for gh_orb_plan_set_pattern / gh_orb_plan_set_steering: call them
 * while no ticket is outstanding. */
gh_orb_plan* gh_orb_stream_plan(gh_orb_stream* stream);
gh_status gh_orb_stream_staging(gh_orb_stream* stream, uint8_t** host_pinned);
gh_status gh_orb_stream_submit(gh_orb_stream* stream, const uint8_t* frames_host, int n_frames, int64_t* ticket);
gh_status gh_orb_stream_poll(gh_orb_stream* stream, int64_t ticket, int* ready);
gh_status gh_orb_stream_collect(gh_orb_stream* stream, int64_t ticket, gh_orb_stream_result* out);
/* Pinned (page-locked, DMA-able) host memory for callers without HIP headers. */
gh_status gh_host_alloc_pinned(gh_ctx* ctx, size_t bytes, void** out_host);
gh_status gh_host_free_pinned(gh_ctx* ctx, void* host);

/* Test-only branch census.  enable != 0 makes the following extractions of this plan count how often the rarely taken
 * paths run; out16 (may be NULL) receives and clears the 16 counters accumulated so far:
 *   [0] cells processed  [1] cells with > 64 scored pixels (list branch)  [2] cells that wrote overflow entries (8th..)
 *   [3] cells at the 32-entry cap  [4] cells with > 32 candidates (ranks dropped)  [5] cells where a strong corner
 *   silenced weaker ones  [6] longest pass-1 queue  [7] most scored pixels in a cell  [8] level selections cut by the
 *   quota  [9] ... with the cut-off bin split among ties  [10] cells whose overflow entries the selection read
 *   [11] streaming selection variant used  [12] zero-filled output rows  [13] level selections below quota.
 * tests/test_orb_adversarial_gpu.py uses it to prove that its inputs reach those branches. */
gh_status gh_orb_plan_debug_counters(gh_orb_plan* plan, int enable, uint32_t* out16);
/* Debug/test access: copy pyramid level `level` of batch slot `slot` to host (w*h bytes, dense). */
gh_status gh_orb_debug_level(gh_orb_plan* plan, int slot, int level, uint8_t* out_host);

/* Deterministic synthetic frames (integer procedural texture, seed = base_seed + frame index);
 * bit-identical to oracle/synth.c.  Test/bench input generator, resident in HBM. */
gh_status gh_synth_frames_dev(gh_ctx* ctx, uint8_t* gray_dev, int width, int height, int row_stride,
                              size_t frame_stride, int first_frame, int n_frames, uint32_t base_seed);

/* ------------------------------------------------------------------ multi-GPU exchange */
/* Frames shard over the GPUs of one node (one process per GPU); the only data-path exchange is an
 * all-gather of the per-frame records after extraction and, optionally, of the match rows after matching.  The
 * reference has no transport (GSLAM's Messenger is in-process, GSLAM/core/Messenger.h:455-468,687-715), so these entry
 * points are what a multi-GPU C++ host adds; no Python / torch is involved.
 *   RCCL transport: rank 0 calls gh_comm_unique_id and hands the 128 bytes to the other ranks by any out-of-band means
 *     (file, socket, MPI, torch.distributed broadcast), then every rank calls gh_comm_create_rccl.  ncclAllGather over
 *     xGMI on the communicator's own stream.
 *   IPC transport (same node): every rank calls gh_comm_create_ipc with the same rendezvous name; peers' gathered
 *     buffers are mapped through HIP IPC and each rank pushes its slice into all of them.  Also works when several ranks
 *     share one GPU (RCCL refuses that).  Asynchronous like RCCL: the ranks' streams order themselves through flags in
 *     the rendezvous segment that bounded one-wave kernels set and poll; no host thread waits during an exchange.
 * A gather is ordered after the work already enqueued on the context's stream and runs beside it; gh_comm_wait orders
 * the context's stream after the gather and returns at once.  A rank that gave up waiting for a peer (timeout
 * GSLAM_HIP_COMM_TIMEOUT_S, default 60) shows in gh_comm_status and in the next gh_allgather* call of every rank.
 * Gathered buffers must come from gh_comm_buffer (a collective call). */
typedef struct gh_comm gh_comm;
gh_status gh_comm_unique_id(uint8_t id_out[128]);
gh_status gh_comm_create_rccl(gh_ctx* ctx, int rank, int world, const uint8_t unique_id[128], gh_comm** out);
gh_status gh_comm_create_ipc(gh_ctx* ctx, int rank, int world, const char* rendezvous_name, gh_comm** out);
void gh_comm_destroy(gh_comm* comm);
int gh_comm_rank(const gh_comm* comm);
int gh_comm_world(const gh_comm* comm);
gh_status gh_comm_buffer(gh_comm* comm, size_t bytes_per_rank, void** gathered_dev); /* world x bytes_per_rank */
gh_status gh_allgather(gh_comm* comm, const void* send_dev, void* gathered_dev, size_t bytes_per_rank);
/* This rank's `frames` frames of gh_orb_extract_dev output into slot `rank` of the gathered arrays
 * (world x frames x cap records).  kps_dev / g_kps_dev may both be NULL when only descriptors are needed. */
gh_status gh_allgather_features(gh_comm* comm, int frames, int cap, const gh_keypoint* kps_dev, const uint8_t* desc_dev,
                                const int32_t* counts_dev, gh_keypoint* g_kps_dev, uint8_t* g_desc_dev,
                                int32_t* g_counts_dev);
/* `rows` match rows of this rank (cap entries each) into slot `rank`; d1 / d2 (and their gathered arrays) may be NULL. */
gh_status gh_allgather_matches(gh_comm* comm, int rows, int cap, const int32_t* idx1_dev, const uint16_t* d1_dev,
                               const uint16_t* d2_dev, int32_t* g_idx1_dev, uint16_t* g_d1_dev, uint16_t* g_d2_dev);
gh_status gh_comm_wait(gh_comm* comm);
gh_status gh_comm_status(gh_comm* comm); /* GH_OK, or GH_ERR_HIP once any rank abandoned an exchange */

/* ------------------------------------------------------------------ BoW transform ---- */
/* GSLAM::Vocabulary image -> BoW vector (GSLAM/core/Vocabulary.h:1558-1621, per-feature descent :1695-1736,
 * normalisation :386-408), for 32-byte binary descriptors.  The vocabulary is given in the in-memory layout of the
 * reference's .gbow file (:1843-1932): nodes = {uint32 childNum; float weight}[nnodes], node_desc = nnodes x 32 B,
 * children of node p at p*k+1 .. p*k+childNum.  weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY;
 * scoring: 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT (enum order of the reference). */
typedef struct gh_bow_vocab gh_bow_vocab;
gh_status gh_bow_vocab_create(gh_ctx* ctx, int k, int L, int weighting, int scoring, uint32_t nnodes,
                              const void* nodes, const uint8_t* node_desc, gh_bow_vocab** out);
/* Binary descriptors of any multiple of 8 bytes (Vocabulary.h:560-568: 32 -> hamming32, 64 -> hamming64, others ->
 * hamming8x); gh_bow_vocab_create is desc_bytes = 32.  The transforms take descriptors of the vocabulary's width. */
gh_status gh_bow_vocab_create_bytes(gh_ctx* ctx, int k, int L, int weighting, int scoring, uint32_t nnodes,
                                    const void* nodes, const uint8_t* node_desc, int desc_bytes, gh_bow_vocab** out);
/* Float vocabularies (SIFT / SURF style): node_desc n_nodes x dims floats, dims a multiple of 8 -- the dimensions for which
 * the reference's DistanceFactory picks l2generic whatever ISA it was built for (Vocabulary.h:550-560,569-578): squared L2,
 * float accumulation in index order, no fused multiply-add.  The transforms then take descriptors of dims floats. */
gh_status gh_bow_vocab_create_f32(gh_ctx* ctx, int k, int L, int weighting, int scoring, uint32_t nnodes, const void* nodes,
                                  const float* node_desc, int dims, gh_bow_vocab** out);
void gh_bow_vocab_destroy(gh_bow_vocab* vocab);
/* Batched over images: desc_dev n_images x cap x 32 B, counts_dev (may be NULL = cap rows each).  Per feature:
 * word id, word weight, node id at level L - levelsup (0xFFFFFFFF / 0 / 0xFFFFFFFF for rows >= count).  Per image:
 * bow_word (ascending, 0xFFFFFFFF padded) / bow_val (normalised as the reference does) / bow_n.  cap <= 16384.
 * Shallow leaves: a tree may end above level L (childNum == 0 on a higher level).  Where a feature's descent ends above
 * level L - levelsup (> 0), the node id is 0, the root.  The reference leaves its `nid` unwritten there
 * (Vocabulary.h:1728 is never reached, the caller's local at :1579 is uninitialised), so 0 is this library's own
 * contract; word id, weight and the BoW vector are the reference's.  Level L - levelsup <= 0 gives 0 as upstream.
 * A float descent in which no child compares below FLT_MAX (NaN / inf / overflowing input) stops at the node it is on;
 * the reference does not terminate on such input.  counts_dev entries are clamped to [.., cap]; <= 0 is an empty image. */
gh_status gh_bow_transform_dev(gh_bow_vocab* vocab, const uint8_t* desc_dev, const int32_t* counts_dev, int cap,
                               int n_images, int levelsup, uint32_t* word_dev, float* weight_dev, uint32_t* node_dev,
                               uint32_t* bow_word_dev, float* bow_val_dev, int32_t* bow_n_dev);
gh_status gh_bow_transform_host(gh_bow_vocab* vocab, const uint8_t* desc, int n, int levelsup, uint32_t* word,
                                float* weight, uint32_t* node, uint32_t* bow_word, float* bow_val, int32_t* bow_n);

/* Batched GSLAM::Vocabulary::score(a, b) = m_scoring_object->score(a, b) (GSLAM/core/Vocabulary.h:691-979, one class
 * per ScoringType): every query BowVector against every database BowVector, scores_dev[q * n_db + j] = score(query q,
 * database j) as the reference's double.  Vectors are in the padded layout gh_bow_transform_dev writes (word ids
 * ascending, *_n valid entries of a row of capacity cap_*), so a block of images transformed on the GPU is scored with
 * no host copy.  L1 / L2 / chi-square / Bhattacharyya / dot product are bit-identical to the reference (same float
 * terms, same ascending-id double accumulation); KL goes through logf and matches to 1e-6 relative. */
gh_status gh_bow_score_dev(gh_ctx* ctx, int scoring, const uint32_t* q_word_dev, const float* q_val_dev,
                           const int32_t* q_n_dev, int n_q, int cap_q, const uint32_t* db_word_dev,
                           const float* db_val_dev, const int32_t* db_n_dev, int n_db, int cap_db, double* scores_dev);
/* One query against n_db host vectors in CSR form (db_off[n_db + 1] offsets into db_word / db_val): the loop-closure
 * candidate scan of a detector that keeps std::map BowVectors on the host. */
gh_status gh_bow_score_host(gh_ctx* ctx, int scoring, const uint32_t* q_word, const float* q_val, int q_n,
                            const uint32_t* db_word, const float* db_val, const int64_t* db_off, int n_db,
                            double* scores);

/* ------------------------------------------------------------------ undistortion ----- */
/* GSLAM::Undistorter::undistort / undistortFast (GSLAM/core/Undistorter.h:206-348) with the remap tables its
 * prepareReMap builds on the host (:120-203): per output pixel remapX, remapFast, remapIdx[4], remapCoef[4].
 * u8 images, 1 / 3 (/ 4 for `fast`) interleaved channels, dense rows.  Pixels the reference leaves unwritten are 0.
 * Table contract (anything else is GH_ERR_ARG): remapFast < w_in * h_in, and remapFast >= 0 wherever remapX > 0;
 * 0 <= remapIdx <= w_in * h_in + w_in (the reference's step past the last row / column, clamped to the last pixel). */
typedef struct gh_undist_plan gh_undist_plan;
gh_status gh_undist_plan_create(gh_ctx* ctx, int w_in, int h_in, int w_out, int h_out, const float* remapX,
                                const int32_t* remapFast, const int32_t* remapIdx, const float* remapCoef,
                                gh_undist_plan** out);
void gh_undist_plan_destroy(gh_undist_plan* plan);
gh_status gh_undistort_dev(gh_undist_plan* plan, const uint8_t* img_dev, int channels, int batch,
                           size_t in_frame_stride, uint8_t* out_dev, size_t out_frame_stride, int fast);
gh_status gh_undistort_host(gh_undist_plan* plan, const uint8_t* img, int channels, uint8_t* out, int fast);

/* ------------------------------------------------------------------ RANSAC estimation - */
/* Robust model fitting with an inlier mask, behind GSLAM::Estimator (GSLAM/core/Estimator.h:100-169; interface only in
 * the reference).  Deterministic: 2048 hypotheses drawn from `seed` (gh_ransac_estimate_conf: the prefix of them that
 * the requested confidence asks for); winner = most correspondences with squared error
 * <= threshold^2, lowest hypothesis index on ties.  model_out must hold 12 doubles; mask_out (n bytes, may be NULL) gets
 * 1 for inliers; *inliers_out = 0 means no model.
 *   0 homography   findHomography      src, dst n x 2; model 9 row-major, h33 = 1; forward transfer error
 *   1 affine 2D    findAffine2D        src, dst n x 2; model 6 = 2 x 3
 *   2 fundamental  findFundamental     src, dst n x 2; dst^T F src = 0; model 9; Sampson error; rank not enforced
 *   3 affine 3D    findAffine3D        src, dst n x 3; model 12 = 3 x 4
 *   4 essential    findEssentialMatrix src, dst n x 2 NORMALISED image coordinates; hypotheses as (2), the winner is
 *                                      projected onto the essential manifold (singular values s, s, 0); model 9
 *   5 SIM3         findSIM3            src, dst n x 3; dst ~ s R src + t by Horn's closed form on 3 pairs;
 *                                      model 8 = [qx qy qz qw tx ty tz s]
 *   6 plane        findPlane           src n x 3 (dst ignored, pass src); model 4 = [nx ny nz d], n . x + d = 0, |n| = 1
 *   7 PnP          findPnP             src n x 3 object points, dst n x 2 normalised image points; 6-point DLT
 *                                      hypotheses (coplanar object points are degenerate); model 12 = [R row-major | t],
 *                                      X_cam = R X + t.  Refine on the inliers with gh_ba_pnp (one problem, host arrays)
 *                                      or gh_pnp_refine_batch_dev / gh_pnp_batch_dev (batched, device-resident). */
#define GH_MODEL_HOMOGRAPHY 0
#define GH_MODEL_AFFINE2D 1
#define GH_MODEL_FUNDAMENTAL 2
#define GH_MODEL_AFFINE3D 3
#define GH_MODEL_ESSENTIAL 4
#define GH_MODEL_SIM3 5
#define GH_MODEL_PLANE 6
#define GH_MODEL_PNP 7
gh_status gh_ransac_estimate(gh_ctx* ctx, int model, const double* src, const double* dst, int n, double threshold,
                             uint64_t seed, double* model_out, uint8_t* mask_out, int* inliers_out);
/* The same with GSLAM::Estimator's `confidence` argument honoured (Estimator.h:100-169 pass threshold AND confidence):
 * the winner is the best among the hypotheses a SEQUENTIAL adaptive RANSAC with the same draws would have examined -- in
 * index order, after every strict improvement of the best inlier count c the needed number of hypotheses becomes
 * ceil(log(1 - confidence) / log(1 - (c / n)^s)) (s = sample size of the model), and the walk ends when it is reached.
 * *hypotheses_used_out (may be NULL) reports that number.  confidence <= 0 or >= 1: all 2048 (== gh_ransac_estimate). */
gh_status gh_ransac_estimate_conf(gh_ctx* ctx, int model, const double* src, const double* dst, int n, double threshold,
                                  double confidence, uint64_t seed, double* model_out, uint8_t* mask_out,
                                  int* inliers_out, int* hypotheses_used_out);
/* The same with GSLAM::EstimatorMethod's sampling flag (Estimator.h:86-89):
 *   GH_SAMPLE_RANSAC  as gh_ransac_estimate_conf.
 *   GH_SAMPLE_LMEDS   least median of squares over the same 2048 hypotheses: the winner has the smallest MEDIAN squared error
 *                     (the element of rank n / 2, ascending; lowest hypothesis index on ties), `confidence` is not used; the
 *                     mask holds the correspondences within max(threshold, 2.5 * 1.4826 * (1 + 5 / (n - s)) * sqrt(median))
 *                     (Rousseeuw's robust standard deviation, the rule of OpenCV's LMEDS); no model when even the best
 *                     median is undefined.
 *   GH_SAMPLE_NONE    NOSAMPLE: no hypotheses -- the algebraic least-squares model of ALL correspondences (normal equations of
 *                     the minimal solver's rows for H / affine, smallest eigenvector of A^T A for F / E / PnP, Horn over all
 *                     pairs for SIM3, principal plane); mask / inliers by `threshold`; *hypotheses_used_out = 1.  A fit that
 *                     is singular or not finite (NaN / Inf coordinates) is no model: zeros, *hypotheses_used_out = 0.
 * In every mode "no model" means *inliers_out = 0, model_out all zero and mask_out all zero, also for GH_MODEL_ESSENTIAL when
 * the winning estimate has no essential matrix near it (its projection fails). */
#define GH_SAMPLE_RANSAC 0
#define GH_SAMPLE_LMEDS 1
#define GH_SAMPLE_NONE 2
gh_status gh_ransac_estimate_ex(gh_ctx* ctx, int model, const double* src, const double* dst, int n, double threshold,
                                double confidence, uint64_t seed, int sampling, double* model_out, uint8_t* mask_out,
                                int* inliers_out, int* hypotheses_used_out);
/* Batched and device-resident: geometric verification of many frame pairs in one call.  Every pointer is a DEVICE pointer,
 * nothing is copied to the host and the call is asynchronous on the context's stream, like the other _dev entries.
 * Problem p owns rows offsets[p] .. offsets[p + 1] - 1 of src / dst (row widths per model as above; offsets_dev holds
 * nproblems + 1 entries, offsets[nproblems] = the rows the arrays hold).  Its result is, bit for bit, what
 * gh_ransac_estimate(ctx, model, src_p, dst_p, n_p, threshold_p, seed_p, ...) returns: GH_SAMPLE_RANSAC over all 2048
 * hypotheses, most inliers, lowest index on ties; all eight models (GH_MODEL_ESSENTIAL is projected on the device).
 *   thresholds_dev  one threshold per problem, or NULL: `threshold` for all.  seeds_dev likewise with `seed`.
 *   models_dev      nproblems x 12 doubles; inliers_dev nproblems counts; mask_dev offsets[nproblems] bytes or NULL, the
 *                   mask of problem p at offsets[p].  Every output is written for every problem (dirty buffers never show).
 * "No model" holds per problem (12 zeros, an all-zero mask segment, 0 inliers): n_p < sample size -- a range that is empty,
 * reversed (offsets not monotone) or not inside 0 .. offsets[nproblems] counts as 0 rows and nothing of it is addressed --,
 * no regular hypothesis, a failed essential projection, a per-problem threshold that is negative or NaN.
 * NOT offered here: `confidence`, GH_SAMPLE_LMEDS and GH_SAMPLE_NONE.  Their selection rules run on the host with libm by
 * design (the prefix rule, the LMedS radius, the all-point fits); gh_ransac_estimate_ex remains the way to get them.
 * GH_ERR_ARG: model outside 0..7, nproblems < 0, a NULL among src / dst / offsets / models / inliers, `threshold` negative
 * or NaN while thresholds_dev is NULL.  nproblems == 0: GH_OK, nothing is launched. */
gh_status gh_ransac_batch_dev(gh_ctx* ctx, int model, const double* src_dev, const double* dst_dev,
                              const int32_t* offsets_dev, int nproblems, double threshold, const double* thresholds_dev,
                              uint64_t seed, const uint64_t* seeds_dev, double* models_dev, uint8_t* mask_dev,
                              int32_t* inliers_dev);
/* The call a pipeline makes after gh_bf_match_pairs_dev / gh_match_mask_dev: a gather in front of gh_ransac_batch_dev.
 * kps_dev, counts_dev, cap, pair_q_dev, pair_t_dev, idx1_dev (npairs x cap) as the pair matchers take and return them;
 * keep_dev (npairs x cap, may be NULL) as gh_match_mask_dev writes it.  The correspondences of pair p are the query rows
 * i < counts[pair_q[p]], in ascending i, with (keep == NULL || keep[p * cap + i]) and 0 <= idx1[p * cap + i] < counts[pair_t[p]]
 * (an index outside that range drops the row, it is never dereferenced; counts are clamped to 0 .. cap): src = the query
 * keypoint's (x, y), dst = the matched train keypoint's (x, y), widened float -> double.  Pair p then equals one
 * gh_ransac_estimate call with `threshold` and `seed` on those rows: models_dev npairs x 12, inliers_dev npairs,
 * n_corr_dev npairs (the rows gathered), inlier_dev npairs x cap with 1 exactly at the query rows that are inliers of the
 * winner and 0 everywhere else.  model: GH_MODEL_HOMOGRAPHY, GH_MODEL_AFFINE2D or GH_MODEL_FUNDAMENTAL only (E needs
 * intrinsics, PnP 3D points: gather them yourself and call gh_ransac_batch_dev); cap <= 65535.  GH_ERR_ARG otherwise. */
gh_status gh_ransac_pairs_dev(gh_ctx* ctx, int model, const gh_keypoint* kps_dev, const int32_t* counts_dev, int cap,
                              const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                              const uint8_t* keep_dev, double threshold, uint64_t seed, double* models_dev,
                              uint8_t* inlier_dev, int32_t* n_corr_dev, int32_t* inliers_dev);
/* Host only (no GPU needed): the number of correspondences of `model` the batched scoring kernel stages through LDS at a
 * time; <= 0 for an unknown model.  Exported so that tests can sit exactly on the kernel's own tile boundary. */
int gh_ransac_batch_tile_rows(int model);
/* Midpoint triangulation, one correspondence per thread (GSLAM::Estimator::trianglate, Estimator.h:164-168): the point of
 * the REFERENCE frame closest to the two rays ref_dir and cur_dir (camera.UnProject of the two pixels), with
 * X_cur = T_ref2cur X_ref, pose = [qx qy qz qw tx ty tz].  pose_stride = 7: one pose per correspondence; 0: one pose for
 * all.  ok[i] = 0 when the rays are parallel or the point lies behind either camera. */
gh_status gh_triangulate(gh_ctx* ctx, const double* ref2cur_pose, int pose_stride, const double* ref_dir,
                         const double* cur_dir, int n, double* ref_points, uint8_t* ok);
/* Two-view reconstruction, batched and device-resident: from an essential matrix and its correspondences to the relative
 * pose and the 3-D points a bundle adjustment starts from (the step between gh_ransac_batch_dev(GH_MODEL_ESSENTIAL) and
 * gh_ba_graph_create).  Every pointer is a DEVICE pointer, nothing is copied to the host, the call is asynchronous on
 * the context's stream.
 * Problem p reads E = E_dev[p * e_stride .. + 8] (row-major; e_stride >= 9 doubles, 12 reads models_dev of
 * gh_ransac_batch_dev in place; the estimator's convention dst^T E src = 0, E ~ [t]x R with X_cur = R X_ref + t) and rows
 * offsets[p] .. offsets[p + 1] - 1 of src (x, y: reference view) and dst (u, v: current view), both in NORMALISED image
 * coordinates as for GH_MODEL_ESSENTIAL; offsets_dev holds nproblems + 1 entries and a range that is empty, reversed or not
 * inside 0 .. offsets[nproblems] counts as 0 rows, nothing of it is addressed.  mask_dev (offsets[nproblems] bytes, may be
 * NULL: all rows) says which rows take part -- the inlier mask of the fit.
 *   decomposition  eigenvectors v1, v2 of E^T E for its two largest eigenvalues l1 >= l2 (cyclic Jacobi), u_a = E v_a / sqrt(l_a),
 *                  u3 = u1 x u2, v3 = v1 x v2, t^ = u3 / |u3|, Ra = u2 v1^T - u1 v2^T + u3 v3^T, Rb = u1 v2^T - u2 v1^T + u3 v3^T;
 *                  candidates 0 (Ra, +t^), 1 (Ra, -t^), 2 (Rb, +t^), 3 (Rb, -t^).  None when l2 > 1e-300 or |u3| > 0 fails.
 *   one row        midpoint triangulation of the rays (x, y, 1), (u, v, 1) as gh_triangulate does it; the row is GOOD under a
 *                  candidate when the rays are not parallel, both ray parameters are positive, the cosine of the angle between
 *                  the rays is below min_parallax_cos, the point has positive depth in both views and its squared reprojection
 *                  error is at most max_reproj^2 in both views.  A NaN anywhere is never good.
 *   vote           counts[k] = participating rows good under candidate k; the winner has the largest count, lowest k on ties.
 *   status         checked in this order:  GH_TWO_VIEW_NO_MODEL   no decomposition, or no participating row;
 *                                          GH_TWO_VIEW_TOO_FEW    counts[best] < min_good or 1000 counts[best] < min_good_permille n_used;
 *                                          GH_TWO_VIEW_AMBIGUOUS  some other candidate has 10 counts[j] > 7 counts[best];
 *                                          GH_TWO_VIEW_OK.
 * Outputs, ALL written for every problem (dirty buffers never show): status_dev nproblems; counts_dev nproblems x 4 (zeros
 * for NO_MODEL); n_used_dev nproblems (participating rows); poses_dev nproblems x 7 [qx qy qz qw tx ty tz], ref -> cur, the
 * layout gh_triangulate takes, |t| = 1, qw >= 0, zeros unless the status is OK; points_dev 3 doubles and good_dev one byte
 * per row of src: the winner's point in the REFERENCE frame and 1 for its good rows, zeros for every other row of a problem
 * and for every row of a problem that is not OK.  The scale is the baseline's: |t| = 1.
 * All counts are integer sums, so the result is the same bits on every run; the arithmetic is + - * / sqrt only and
 * tests/two_view_restate.py restates it.
 * GH_ERR_ARG: nproblems < 0, e_stride < 9, params NULL, min_parallax_cos outside (0, 1], max_reproj negative or NaN, a NULL
 * among the other pointers (mask_dev excepted).  nproblems == 0: GH_OK, nothing is launched. */
#define GH_TWO_VIEW_OK 0
#define GH_TWO_VIEW_NO_MODEL 1
#define GH_TWO_VIEW_TOO_FEW 2
#define GH_TWO_VIEW_AMBIGUOUS 3
typedef struct gh_two_view_params {
  double min_parallax_cos;   /* 0.99998: ORB-SLAM's initialiser asks for a ray angle of about 0.36 degrees */
  double max_reproj;         /* 0.004 normalised units: 2 px at f = 500 */
  int32_t min_good;          /* 50 */
  int32_t min_good_permille; /* 900: ORB-SLAM's 0.9 of the rows */
} gh_two_view_params;
void gh_two_view_default_params(gh_two_view_params* p);
gh_status gh_two_view_batch_dev(gh_ctx* ctx, const double* E_dev, int e_stride, const double* src_dev, const double* dst_dev,
                                const int32_t* offsets_dev, int nproblems, const uint8_t* mask_dev,
                                const gh_two_view_params* params, double* poses_dev, double* points_dev, uint8_t* good_dev,
                                int32_t* counts_dev, int32_t* n_used_dev, int32_t* status_dev);
/* The call a pipeline makes after the pair matcher when the camera is calibrated: gather, essential fit and two-view
 * reconstruction of every pair in one call.  kps_dev .. keep_dev as gh_ransac_pairs_dev takes them and the same gather
 * rule; the rows are normalised with the pinhole intrinsics as ((double)x - cx) / fx, ((double)y - cy) / fy, fitted with
 * GH_MODEL_ESSENTIAL (`threshold` in normalised units, `seed`) and the two-view kernel runs on the inliers of that fit.
 * The result equals, bit for bit, the composition of the public pieces: the gather, that normalisation in double,
 * gh_ransac_batch_dev(GH_MODEL_ESSENTIAL) and gh_two_view_batch_dev with its mask.
 * Per pair: models_dev npairs x 12, inliers_dev, n_corr_dev, poses_dev npairs x 7, votes_dev npairs x 4 (the four counts),
 * status_dev.  Per query row, as gh_ransac_pairs_dev indexes its mask: inlier_dev npairs x cap, good_dev npairs x cap,
 * points_dev npairs x cap x 3 (zeros where good is 0).  Limits as gh_ransac_pairs_dev (cap <= 65535); fx, fy > 0. */
gh_status gh_two_view_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int cap,
                                const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                const uint8_t* keep_dev, double fx, double fy, double cx, double cy, double threshold,
                                uint64_t seed, const gh_two_view_params* params, double* models_dev, uint8_t* inlier_dev,
                                int32_t* n_corr_dev, int32_t* inliers_dev, double* poses_dev, double* points_dev,
                                uint8_t* good_dev, int32_t* votes_dev, int32_t* status_dev);

/* ------------------------------------------------------------------ bundle adjustment - */
/* DOF bits follow GSLAM::KeyFrameEstimzationDOF (GSLAM/core/Optimizer.h:70-84). */
#define GH_KF_X 1
#define GH_KF_Y 2
#define GH_KF_Z 4
#define GH_KF_RX 8
#define GH_KF_RY 16
#define GH_KF_RZ 32
#define GH_KF_SE3 63
#define GH_KF_SCALE 64 /* UPDATE_KF_SCALE: only the pose-graph solver and gh_align_sim3 have a scale to update */
#define GH_KF_SIM3 127

/* Values the solvers take as they are given:
 *   cam_pose   the quaternion is used AS IT STANDS, not normalised on the way in: X_c = M(q)^T (X - t) with
 *              M(q) = I + 2 qw [v]x + 2 [v]x^2, which is the rotation only for a unit q (q and -q are the same pose).  The first
 *              accepted step renormalises the quaternion of every camera that is not fixed; a fixed camera keeps its bits.
 *   obs_info   must be symmetric positive semi-definite.  Rank-deficient and all-zero matrices are allowed (a zero matrix
 *              removes the observation from the cost); an indefinite matrix is unspecified.
 *   cam_dof    only the bits GH_KF_X .. GH_KF_RZ count; GH_KF_SCALE and higher bits are ignored.
 * An observation whose camera-frame depth is not above 1e-9 does not exist for that evaluation (a NaN depth included). */
typedef struct gh_ba_problem {
  int32_t n_cams, n_points, n_obs;
  /* T_wc (camera -> world) per keyframe: 7 doubles [qx,qy,qz,qw,tx,ty,tz]  (in/out) */
  double* cam_pose;
  const int32_t* cam_dof; /* GH_KF_* bitmask per camera; 0 = fixed */
  double* point_xyz;      /* 3 doubles per point, world frame  (in/out) */
  const uint8_t* point_free; /* 1 = optimise, 0 = fixed; NULL = all free */
  const int32_t* obs_cam;
  const int32_t* obs_point;
  const double* obs_xy;   /* 2 doubles per observation: normalised (x,y) on the z=1 plane */
  const double* obs_info; /* 4 doubles (row-major 2x2) per observation or NULL = identity */
} gh_ba_problem;

typedef struct gh_ba_options {
  double huber_delta;        /* OptimzeConfig::projectErrorHuberThreshold; <= 0 disables */
  int32_t max_iterations;    /* OptimzeConfig::maxIterations */
  double initial_radius;     /* 1e4 */
  double function_tolerance; /* 1e-6 */
  double gradient_tolerance; /* 1e-10 */
  double min_relative_decrease; /* 1e-3 */
  int32_t verbose;
  int32_t deterministic;     /* 1 (default): reproducible sums -- gh_ba_solve: ordered segmented Schur accumulation; gh_graph_solve:
                                the landmark part pre-rounded so that its atomics add exactly (bit-identical from run to run) on
                                the DENSE path (two more n x lda accumulators, one fold pass per iteration); graphs large enough
                                for the block-sparse Cholesky (gh_graph_summary: sparse) keep plain atomics -- the option is
                                IGNORED there and the last bits vary between runs;
                                0: plain f64 atomics (faster assembly, last bits vary between runs) */
} gh_ba_options;
void gh_ba_default_options(gh_ba_options* o);

#define GH_BA_MAX_TRACE 512
typedef struct gh_ba_summary {
  int32_t iterations;      /* LM iterations executed (accepted + rejected) */
  int32_t accepted;
  int32_t termination;     /* 0 max_iterations, 1 function_tolerance, 2 gradient_tolerance, 3 failure */
  double initial_cost, final_cost;
  double solve_ms_total;   /* host time from the dense reduced-camera solve to the candidate cost (per-iteration sync) */
  double total_ms;
  int32_t trace_len;
  double trace_cost[GH_BA_MAX_TRACE];   /* candidate cost evaluated at each iteration */
  double trace_radius[GH_BA_MAX_TRACE]; /* trust-region radius used at each iteration */
  uint8_t trace_accepted[GH_BA_MAX_TRACE];
} gh_ba_summary;

/* Host-struct entry point (what the Optimizer plugin calls): uploads, runs LM on the GPU,
 * writes cam_pose / point_xyz back in place. */
gh_status gh_ba_solve(gh_ctx* ctx, gh_ba_problem* problem, const gh_ba_options* options,
                      gh_ba_summary* summary);

/* Device-resident graph across solves.  A windowed SLAM back end calls Optimizer::optimize (GSLAM/core/Optimizer.h:229)
 * every few keyframes on a graph whose TOPOLOGY (which camera observes which point) changes far less often than its
 * values; gh_ba_solve rebuilds the index lists, the Schur pair lists and the chunk tables and uploads every array each
 * time (1.1-2.4 ms at C4 against 12 x 1.0 ms of iterations).  A gh_ba_graph keeps all of that in HBM:
 *   gh_ba_graph_create   validates + uploads the problem, builds the lists and tables (what gh_ba_solve does before its
 *                        first iteration).  options->deterministic is fixed here (it decides whether pair lists exist).
 *   gh_ba_graph_update   new VALUES for the same topology; any pointer may be NULL = unchanged.  obs_info / point_free
 *                        can only be updated if the graph was created with them.
 *   gh_ba_graph_solve    LM iterations on the resident state (same algorithm, same results as gh_ba_solve on the same
 *                        values); the state stays on the device: consecutive solves continue from the last accepted one.
 *   gh_ba_graph_read     cam_pose (n_cams x 7) / point_xyz (n_points x 3) back to the host; either may be NULL.
 * The Optimizer plugin caches one graph keyed on the topology of the BundleGraph it is given. */
typedef struct gh_ba_graph gh_ba_graph;
gh_status gh_ba_graph_create(gh_ctx* ctx, const gh_ba_problem* problem, const gh_ba_options* options, gh_ba_graph** out);
void gh_ba_graph_destroy(gh_ba_graph* graph);
gh_status gh_ba_graph_update(gh_ba_graph* graph, const double* cam_pose, const double* point_xyz, const double* obs_xy,
                             const double* obs_info, const int32_t* cam_dof, const uint8_t* point_free);
gh_status gh_ba_graph_solve(gh_ba_graph* graph, const gh_ba_options* options, gh_ba_summary* summary);
gh_status gh_ba_graph_read(gh_ba_graph* graph, double* cam_pose, double* point_xyz);

/* Pose-only (motion-only BA) on 3D-2D matches: pose = T_wc 7 doubles in/out;
 * information_out (36 doubles, row-major 6x6 J^T J at the solution) may be NULL. */
gh_status gh_ba_pnp(gh_ctx* ctx, const double* points_xyz, const double* obs_xy, int n, double* pose,
                    int dof, const gh_ba_options* options, double* information_out, gh_ba_summary* summary);

/* Pose refinement after the PnP RANSAC, batched and device-resident: many independent gh_ba_pnp problems in one launch.
 * Every pointer is a DEVICE pointer, nothing is copied to the host, the call is asynchronous on the context's stream.
 * Problem p owns rows offsets[p] .. offsets[p + 1] - 1 of xyz_dev (3 doubles: world point) and xy_dev (2 doubles: normalised
 * image point); offsets_dev holds nproblems + 1 entries.  nrows = the rows the arrays hold (what a caller stores in
 * offsets[nproblems]): the host sizes its index scratch by it, and a range that is empty, reversed or not inside BOTH
 * 0 .. nrows and 0 .. offsets[nproblems] counts as 0 rows, nothing of it is addressed.  Ranges of different problems must
 * not overlap (offsets that are not monotone can make them): such problems get unspecified values, still inside the arrays.
 *   rows         the PARTICIPATING rows of a problem are those of its range with mask_dev == NULL || mask_dev[row] != 0, in
 *                ascending order (mask_dev: nrows bytes -- the inlier mask of the fit).
 *   start        start_stride == 7: start_dev[7 p ..] is a T_wc pose [qx qy qz qw tx ty tz], taken as it stands (not
 *                renormalised: gh_ba_pnp does not either).  start_stride == 12: start_dev[12 p ..] is a model of
 *                gh_ransac_batch_dev(GH_MODEL_PNP), converted as gh_pnp_pose_from_model does.  No start: a value read that
 *                is not finite, a quaternion whose sum of squares fails > 0, for stride 12 an all-zero R ("no model").
 *   refinement   dof, options as gh_ba_pnp takes them (NULL: the defaults; `verbose` is ignored, `deterministic` plays no
 *                part).  A problem that is optimised equals, BIT FOR BIT, gh_ba_pnp (its default single-launch path) on the
 *                participating rows with the same start, dof and options: pose, information, iterations, accepted,
 *                termination, initial_cost and final_cost.
 *   termination  GH_PNP_NO_START  no start: pose, information, costs, counts and the inlier segment are zero;
 *                GH_PNP_TOO_FEW   fewer than min_rows participating rows: pose = the (converted) start, costs 0, information
 *                                 zeros, not optimised;
 *                0 .. 3           the codes of gh_ba_summary.termination.
 *   classify     with inlier_threshold >= 0, a last pass over ALL rows of the range, masked or not, at the pose written:
 *                inlier_dev[row] = 1 when the point's depth in the camera is > 1e-9 and dx * dx + dy * dy <=
 *                inlier_threshold^2 (the residual of gh_ba_pnp's linearisation), else 0; n_inliers_dev[p] their number (an
 *                integer sum: the same bits on every run).  Zeros for NO_START; a TOO_FEW problem is classified under its
 *                start.  With inlier_threshold < 0 nothing is classified: inlier_dev / n_inliers_dev are zero-filled.
 * Outputs, ALL written for every problem (dirty buffers never show): poses_dev nproblems x 7, summaries_dev nproblems,
 * info_dev nproblems x 36 (row-major J^T W J, as gh_ba_pnp's information_out), inlier_dev one byte per row of a valid range
 * (rows no range owns are not touched), n_inliers_dev nproblems.  mask_dev, info_dev, inlier_dev, n_inliers_dev may be NULL.
 * GH_ERR_ARG: nproblems < 0, nrows < 0, start_stride not 7 or 12, min_rows < 0, inlier_threshold NaN, a NULL among the
 * other pointers.  nproblems == 0: GH_OK, nothing is launched. */
#define GH_PNP_NO_START 4
#define GH_PNP_TOO_FEW 5
typedef struct gh_pnp_batch_summary { /* 32 bytes */
  int32_t iterations, accepted, termination, n_used; /* n_used: participating rows */
  double initial_cost, final_cost;
} gh_pnp_batch_summary;
/* Host only (no GPU needed): model12 = [R row-major | t] with X_cam = R X + t  ->  pose7 = T_wc [qx qy qz qw tx ty tz]:
 * q = the quaternion of R^T by Shepperd's rule (qw >= 0, normalised), t_wc[i] = -((R[i] t[0] + R[3 + i] t[1]) + R[6 + i] t[2]).
 * Returns 1 with a pose, 0 with pose7 all zero when there is no start (see above).  tests/pnp_restate.py restates it. */
int gh_pnp_pose_from_model(const double* model12, double* pose7);
gh_status gh_pnp_refine_batch_dev(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev,
                                  int nproblems, int nrows, const uint8_t* mask_dev, const double* start_dev, int start_stride,
                                  int dof, const gh_ba_options* options, int min_rows, double inlier_threshold,
                                  double* poses_dev, double* info_dev, gh_pnp_batch_summary* summaries_dev,
                                  uint8_t* inlier_dev, int32_t* n_inliers_dev);
/* The call after a 3D-2D gather: fit, refine, refit, for every problem in one call.  It equals, bit for bit, the composition
 * of the public pieces:
 *   1. gh_ransac_batch_dev(GH_MODEL_PNP, src = xyz, dst = xy, ransac_threshold, seed) -> models_dev (nproblems x 12), its
 *      mask, ransac_inliers_dev (nproblems);
 *   2. gh_pnp_refine_batch_dev with that mask, start = the models (stride 12), classification by inlier_threshold;
 *   3. gh_pnp_refine_batch_dev with mask = the inliers of (2), start = the poses of (2) (stride 7), the same classification.
 * poses_dev, info_dev, inlier_dev, n_inliers_dev are those of (3); summaries_dev is nproblems x 2: [2 p] round (2),
 * [2 p + 1] round (3).  A problem whose round-(2) inliers number fewer than min_rows keeps its first fit (TOO_FEW);
 * NO_START carries through both rounds.  Ranges as above (inside both nrows and offsets[nproblems], for every stage).
 * GH_ERR_ARG as above, and: ransac_threshold negative or NaN, inlier_threshold negative (round (3) needs the classification),
 * models_dev or ransac_inliers_dev NULL.  info_dev, inlier_dev, n_inliers_dev may be NULL. */
gh_status gh_pnp_batch_dev(gh_ctx* ctx, const double* xyz_dev, const double* xy_dev, const int32_t* offsets_dev,
                           int nproblems, int nrows, double ransac_threshold, uint64_t seed, int dof,
                           const gh_ba_options* options, int min_rows, double inlier_threshold, double* models_dev,
                           int32_t* ransac_inliers_dev, double* poses_dev, double* info_dev,
                           gh_pnp_batch_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev);

/* Map points from multi-view tracks, batched and device-resident: the step between gh_pnp_batch_dev (cameras registered) and
 * gh_ba_graph_create (gh_ba_problem.point_xyz needs a start for every point).  Every pointer is a DEVICE pointer, the call is
 * asynchronous on the context's stream, nothing is synchronised or allocated per call (scratch comes from the context).
 * Inputs are laid out as in gh_ba_problem: cam_pose_dev n_cams x 7 T_wc [qx qy qz qw tx ty tz], taken as it stands (not
 * renormalised); obs_cam_dev / obs_point_dev n_obs; obs_xy_dev n_obs x 2 on the z = 1 plane; obs_use_dev n_obs bytes or NULL = all
 * observations; point_select_dev n_points bytes or NULL = all points.
 *   track      of point p: the observations with obs_point == p in ascending observation index (the caller need not group or
 *              sort them); the RANK of an observation is its position in that list.  Only USABLE observations are listed:
 *              obs_use NULL or non-zero, 0 <= obs_cam < n_cams, 0 <= obs_point < n_points.  An index outside its range drops the
 *              observation; it is never dereferenced.
 *   arithmetic + - * / and sqrt in IEEE doubles, nothing fused, in the order written here.
 *   ray        w = quat_rotate(q, (x, y, 1)):  uv = q.xyz X p, uv += uv, w_i = (p_i + qw * uv_i) + (q.xyz X uv)_i, with
 *              (a X b)_0 = a1 * b2 - a2 * b1, (a X b)_1 = a2 * b0 - a0 * b2, (a X b)_2 = a0 * b1 - a1 * b0;
 *              d = w * (1 / sqrt((w0 * w0 + w1 * w1) + w2 * w2));  P = I - d d^T: Pii = 1 - di * di, Pij = -(di * dj);
 *              g_i = (Pi0 * t0 + Pi1 * t1) + Pi2 * t2.
 *   sums       gh_track_group_lanes() = 8 partial sums, each from +0.0: partial j adds the (P, g) of the LIVE observations with
 *              rank % 8 == j in ascending rank; total = ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7)) entry by entry: A (the
 *              sum of P, six entries) and b (the sum of g).  Every round sums anew over the live set; nothing is subtracted.
 *   solve      A X = b by LDL^T without pivoting: D0 = A00; L10 = A01 / D0; L20 = A02 / D0; D1 = A11 - L10 * A01;
 *              u = A12 - L20 * A01; L21 = u / D1; D2 = (A22 - L20 * A02) - L21 * u; every pivot must satisfy D > 1e-12 (a NaN does
 *              not), else DEGENERATE; z0 = b0; z1 = b1 - L10 * z0; z2 = (b2 - L20 * z0) - L21 * z1; y_i = z_i / D_i; X2 = y2;
 *              X1 = y1 - L21 * X2; X0 = (y0 - L10 * X1) - L20 * X2.
 *   classify   a live observation at X, with the residual of gh_ba_solve's linearisation: Xc = quat_rotate((-qx, -qy, -qz, qw),
 *              X - t); not good unless Xc[2] > 1e-9; iz = 1 / Xc[2]; r = (Xc[0] * iz - x, Xc[1] * iz - y); e = r0 * r0 + r1 * r1;
 *              good when e <= max_reproj * max_reproj.  Drop key: e when the depth test passed and e is not a NaN, else +inf.
 *              (A NaN that reaches only b, from a camera translation, leaves the pivots regular: X is NaN, no observation is
 *              good, every key is +inf and the drop rule removes the lowest rank.)
 *   per point  (selected)  1. live = its usable observations; fewer than min_views: TOO_FEW.
 *              2. loop: sum and solve (failure: DEGENERATE); classify; all live observations good: leave the loop; drops ==
 *                 max_drops or the live set has min_views members: INCONSISTENT; else drop the live observation with the largest
 *                 key (lowest rank on ties), ++drops.
 *              3. parallax on the final live set: f = the live observation of lowest rank; cos_k = (df0 * dk0 + df1 * dk1) +
 *                 df2 * dk2 for every other live k; no cos_k < min_parallax_cos: LOW_PARALLAX (all rays within theta of the
 *                 first: every pair within 2 theta).  4. else OK.
 * Outputs, ALL written for every point and observation (dirty buffers never show): status_dev n_points (GH_TRACK_*);
 * point_xyz_dev n_points x 3: X for OK points, zeros for every other selected point, NOT written for SKIPPED points (in/out:
 * existing map points survive); n_good_dev n_points: the size of the final live set for OK points, else 0; obs_good_dev n_obs
 * bytes: 1 exactly at the final live observations of OK points, 0 everywhere else (a bad index included).  Counts are integer
 * and the floating-point order is fixed: the same bits on every run.  tests/tracks_restate.py restates all of it.
 * GH_ERR_ARG: ctx or params NULL; n_cams, n_obs or n_points negative; min_parallax_cos outside (0, 1]; max_reproj negative or
 * NaN; min_views < 2; max_drops < 0; a NULL among cam_pose, obs_cam, obs_point, obs_xy or the four outputs.  n_points == 0:
 * GH_OK, nothing is launched.  n_obs == 0 with n_points > 0: every selected point is TOO_FEW. */
#define GH_TRACK_OK 0
#define GH_TRACK_TOO_FEW 1        /* fewer than min_views usable observations */
#define GH_TRACK_DEGENERATE 2     /* the 3 x 3 system has no regular solution (parallel rays, a NaN) */
#define GH_TRACK_INCONSISTENT 3   /* some live observation still fails after the allowed drops */
#define GH_TRACK_LOW_PARALLAX 4
#define GH_TRACK_SKIPPED 5        /* point_select says: not this point */
typedef struct gh_track_params {  /* 24 bytes */
  double min_parallax_cos;  /* 0.9998: ORB-SLAM's bound when it creates map points */
  double max_reproj;        /* 0.004 normalised units, as gh_two_view_params */
  int32_t min_views;        /* 2 */
  int32_t max_drops;        /* 2 */
} gh_track_params;
void gh_track_default_params(gh_track_params* p);
int gh_track_group_lanes(void);   /* host only: 8, the number of partial sums (above); lets tests sit on the boundary */
gh_status gh_triangulate_tracks_dev(gh_ctx* ctx, const double* cam_pose_dev, int n_cams, const int32_t* obs_cam_dev,
                                    const int32_t* obs_point_dev, const double* obs_xy_dev, int n_obs, int n_points,
                                    const uint8_t* obs_use_dev, const uint8_t* point_select_dev,
                                    const gh_track_params* params, double* point_xyz_dev, int32_t* status_dev,
                                    int32_t* n_good_dev, uint8_t* obs_good_dev);
/* Multi-view tracks from pair matches, device-resident: the step between the pair entries (gh_match_mask_dev,
 * gh_ransac_pairs_dev, gh_two_view_pairs_dev: idx1 and a byte per query row of every frame pair) and the per-point arrays
 * gh_triangulate_tracks_dev and a gh_ba_problem take (obs_cam, obs_point, obs_xy).  Every pointer is a DEVICE pointer, nothing
 * is copied to the host, the call is asynchronous on the context's stream.  kps_dev n_frames x cap records, counts_dev
 * n_frames, pair_q_dev / pair_t_dev npairs, idx1_dev npairs x cap as the pair entries take and return them; inlier_dev
 * npairs x cap or NULL (all rows): `keep` of gh_match_mask_dev, `inlier` of gh_ransac_pairs_dev, `inlier` / `good` of
 * gh_two_view_pairs_dev.
 *   nodes      N = n_frames * cap; the node of (frame f, row i) is f * cap + i; it EXISTS when 0 <= i < clamp(counts[f], 0, cap).
 *   edges      pair p is read only when 0 <= pair_q[p], pair_t[p] < n_frames and pair_q[p] != pair_t[p]; otherwise the whole
 *              pair is ignored and nothing of it is addressed beyond pair_q[p] / pair_t[p].  Query row i of the pair gives the
 *              edge (pair_q[p], i) -- (pair_t[p], j), j = idx1[p * cap + i], when i < clamp(counts[pair_q[p]], 0, cap),
 *              (inlier_dev == NULL || inlier_dev[p * cap + i] != 0) and 0 <= j < clamp(counts[pair_t[p]], 0, cap): the gather
 *              rule of gh_ransac_pairs_dev.  An index outside its range drops the row; it is never dereferenced.  The same edge
 *              may occur any number of times and in both directions.
 *   components the connected components of the undirected graph on the existing nodes; the LABEL of a component is its
 *              smallest node id, whatever the order of the pairs, the launch geometry or the outcome of any race.
 *   class      of a component, checked in this order: CONFLICT two of its nodes lie in the same frame -- the whole component
 *              is dropped, as OpenMVG's track filter does (a many-to-one match produces exactly this); SHORT fewer than
 *              min_views nodes (an existing node without any edge is a component of one); otherwise it is a TRACK.
 *   numbering  tracks get the point ids 0, 1, ... in ascending label; the observations are the nodes of tracks in ascending
 *              node id (frame-major, then row), the observation index is the rank in that list.
 * Outputs, ALL written for their full capacity on every call (dirty buffers never show): node_point_dev N: the point id
 * (>= 0), GH_LINK_SHORT, GH_LINK_CONFLICT or GH_LINK_NO_ROW (the node does not exist); obs_cam_dev, obs_point_dev,
 * obs_node_dev N each and obs_xy_dev N x 2: for observation k < n_obs the frame, the point id, the node id and
 * (((double)x - cx) / fx, ((double)y - cy) / fy) of that keypoint (the normalisation of gh_two_view_pairs_dev: two IEEE
 * operations each, nothing fused); for k >= n_obs obs_cam = obs_point = obs_node = -1 and obs_xy = (0, 0); point_len_dev
 * N / 2 (enough because min_views >= 2): the number of observations of point p, 0 for p >= n_points; totals_dev 4: n_obs,
 * n_points, the number of CONFLICT components, the number of SHORT components with at least two nodes.
 * The padding is the point of the layout: the arrays go to gh_triangulate_tracks_dev as they are, with n_cams = n_frames,
 * n_obs = N and n_points = N / 2, without a count being read back -- that contract drops an observation whose index is out
 * of range and reports a point without observations as GH_TRACK_TOO_FEW.  Everything is integer work except the two
 * divisions: the same bits on every run.  tests/track_link_restate.py restates all of it.
 * GH_ERR_ARG, and then nothing is written: ctx NULL; n_frames, cap or npairs negative; cap > 65535; n_frames * cap >
 * INT32_MAX - 1; min_views < 2; fx or fy not > 0 (a NaN included); a NULL among kps, counts or the seven outputs; with
 * npairs > 0 a NULL among pair_q, pair_t, idx1.  N == 0: GH_OK, only totals_dev (zeros) is written.  npairs == 0 with
 * N > 0: every existing node is SHORT, everything else is padding. */
#define GH_LINK_SHORT (-1)
#define GH_LINK_CONFLICT (-2)
#define GH_LINK_NO_ROW (-3)
gh_status gh_link_tracks_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                             const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                             const uint8_t* inlier_dev, double fx, double fy, double cx, double cy, int min_views,
                             int32_t* node_point_dev, int32_t* obs_cam_dev, int32_t* obs_point_dev, double* obs_xy_dev,
                             int32_t* obs_node_dev, int32_t* point_len_dev, int32_t* totals_dev);
/* The 3D-2D gather: new frames matched against map frames, read through the map -- the step between gh_link_tracks_dev /
 * gh_triangulate_tracks_dev (a map exists) and gh_pnp_batch_dev (xyz, xy, offsets of one problem per frame).  Every pointer is a
 * DEVICE pointer, nothing is copied to the host, the call is asynchronous on the context's stream, scratch comes from the
 * context.  kps_dev, counts_dev, n_frames, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev as gh_link_tracks_dev takes them;
 * keep_dev npairs x cap or NULL (all rows).  The map: node_point_dev N = n_frames * cap entries as gh_link_tracks_dev writes them
 * (>= 0: a point id, anything negative: no point), point_xyz_dev n_points x 3, point_status_dev n_points or NULL -- a point is
 * USABLE when point_status_dev is NULL or its status equals GH_TRACK_OK.
 *   candidates pair p is read under the rule of gh_link_tracks_dev (both frame indices in range and different, else nothing of
 *              it is addressed).  Query row i of the pair passes when i < clamp(counts[pair_q[p]], 0, cap), (keep_dev == NULL ||
 *              keep_dev[p * cap + i] != 0) and 0 <= j = idx1[p * cap + i] < clamp(counts[pair_t[p]], 0, cap): the gather rule of
 *              gh_ransac_pairs_dev.  A passing row gives the candidate c = node_point[pair_t[p] * cap + j] to the node
 *              (pair_q[p], i) when 0 <= c < n_points and point c is usable; a value outside that range drops the candidate, it is
 *              never used as an index.  The node_point entries of a frame are read only where the frame is the TRAIN frame of a
 *              pair: what a query node itself holds plays no part.  The same pair may occur any number of times.
 *   per node   S = the set of its candidates over all pairs.  The node does not exist: GH_LOC_NO_ROW.  S empty: GH_LOC_NO_POINT.
 *              min S != max S: GH_LOC_AMBIGUOUS -- two map frames disagree about what this keypoint is; the row is dropped, not
 *              voted on.  Otherwise the node CLAIMS the one point of S.
 *   per (frame, point)  two or more nodes of one frame claim the same point: all of them are GH_LOC_SHARED (a many-to-one
 *              match, as the CONFLICT rule of gh_link_tracks_dev).  A node that is the only one of its frame to claim its point
 *              is a CORRESPONDENCE; nodes of different frames may claim one point, each stays.
 *   numbering  correspondences are numbered in ascending node id (frame-major, then row); problem f (one per frame) owns
 *              offsets[f] .. offsets[f + 1] - 1, offsets[n_frames] = n_corr; a frame without correspondences has an empty range.
 * Outputs, ALL written for their full capacity on every call (dirty buffers never show): row_point_dev N: the point id or a
 * GH_LOC_* code; offsets_dev n_frames + 1; xyz_dev N x 3: for k < n_corr an exact copy of the point's three doubles; xy_dev
 * N x 2: (((double)x - cx) / fx, ((double)y - cy) / fy) of the keypoint (two IEEE operations each, nothing fused: the
 * normalisation of gh_link_tracks_dev); corr_node_dev N: the node of correspondence k; for k >= n_corr xyz = xy = zeros and
 * corr_node = -1; totals_dev 4: n_corr, the AMBIGUOUS nodes, the SHARED nodes, the frames with at least one correspondence.
 * xyz_dev, xy_dev, offsets_dev go to gh_pnp_batch_dev as they are, with nproblems = n_frames and nrows = N.  Everything is integer
 * work except the two divisions: the same bits on every run.  tests/localize_restate.py restates all of it.
 * GH_ERR_ARG, and then nothing is written: ctx NULL; n_frames, cap, npairs or n_points negative; cap > 65535; n_frames * cap >
 * INT32_MAX - 1; fx or fy not > 0 (a NaN included); a NULL among kps, counts, node_point or the six outputs; with n_points > 0 a
 * NULL point_xyz; with npairs > 0 a NULL among pair_q, pair_t, idx1.  N == 0: GH_OK, only offsets_dev (zeros) and totals_dev
 * (zeros) are written.  npairs == 0 or n_points == 0 with N > 0: every existing node is NO_POINT. */
#define GH_LOC_NO_POINT (-1)
#define GH_LOC_AMBIGUOUS (-2)
#define GH_LOC_NO_ROW (-3)
#define GH_LOC_SHARED (-4)
gh_status gh_pnp_gather_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                  const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                  const uint8_t* keep_dev, const int32_t* node_point_dev, int n_points, const double* point_xyz_dev,
                                  const int32_t* point_status_dev, double fx, double fy, double cx, double cy,
                                  int32_t* row_point_dev, int32_t* offsets_dev, double* xyz_dev, double* xy_dev,
                                  int32_t* corr_node_dev, int32_t* totals_dev);
/* Register every frame against the map in one call.  It equals, bit for bit, the composition of the public pieces:
 *   1. gh_pnp_gather_pairs_dev -> row_point_dev, offsets_dev, xyz_dev, xy_dev, corr_node_dev, totals_dev (outputs of this call
 *      too, the caller supplies the arrays);
 *   2. gh_pnp_batch_dev(xyz_dev, xy_dev, offsets_dev, nproblems = n_frames, nrows = N, ransac_threshold, seed, dof, options,
 *      min_rows, inlier_threshold) -> models_dev n_frames x 12, ransac_inliers_dev n_frames, poses_dev n_frames x 7, info_dev
 *      n_frames x 36 or NULL, summaries_dev n_frames x 2; its inlier bytes per correspondence and n_inliers stay in scratch;
 *   3. a scatter -> row_inlier_dev N bytes: 1 exactly at the nodes whose correspondence is an inlier of the last round, 0
 *      everywhere else.
 * row_point_dev and row_inlier_dev together are what gh_extend_tracks_dev needs to add the new observations to the tracks.  A frame
 * without correspondences is an empty range of gh_pnp_batch_dev and comes out as that contract says.  GH_ERR_ARG: whatever
 * either stage rejects, and row_inlier_dev NULL -- checked before anything is launched, and then nothing is written.
 * N == 0: GH_OK, only offsets_dev and totals_dev are written, and with n_frames > 0 what gh_pnp_batch_dev writes for empty
 * ranges. */
gh_status gh_localize_pairs_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                                const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                                const uint8_t* keep_dev, const int32_t* node_point_dev, int n_points, const double* point_xyz_dev,
                                const int32_t* point_status_dev, double fx, double fy, double cx, double cy,
                                double ransac_threshold, uint64_t seed, int dof, const gh_ba_options* options, int min_rows,
                                double inlier_threshold, int32_t* row_point_dev, int32_t* offsets_dev, double* xyz_dev,
                                double* xy_dev, int32_t* corr_node_dev, int32_t* totals_dev, double* models_dev,
                                int32_t* ransac_inliers_dev, double* poses_dev, double* info_dev,
                                gh_pnp_batch_summary* summaries_dev, uint8_t* row_inlier_dev);
/* Extending the map: the rows of new frames that gh_localize_pairs_dev registered are added to the tracks of the points they
 * saw, and the remaining rows are linked into NEW tracks whose ids go on where the map's end -- gh_link_tracks_dev cannot do
 * this, it numbers every track from scratch.  Every pointer is a DEVICE pointer, nothing is copied to the host, the call is
 * asynchronous on the context's stream, scratch comes from the context.  kps_dev, counts_dev, n_frames, cap, pair_q_dev,
 * pair_t_dev, npairs, idx1_dev, inlier_dev, the intrinsics and min_views as gh_link_tracks_dev takes them.  The map:
 * node_point_in_dev N entries or NULL (no map), n_points.  The claims: row_point_dev N and row_inlier_dev N bytes as
 * gh_localize_pairs_dev writes them, or both NULL (no claims).
 *   sizes      N = n_frames * cap, PC = n_points + N / 2: a new track uses up at least two nodes that had no point, so PC point
 *              entries are always enough and no count is read back.
 *   nodes, pairs, edges  exactly the rules of gh_link_tracks_dev: node (f, i) EXISTS when 0 <= i < clamp(counts[f], 0, cap); a pair
 *              is read only when both frame indices are in range and different; query row i of a pair is an edge under the
 *              gather rule of gh_ransac_pairs_dev; an index outside its range drops the row, it is never dereferenced.
 *   state      of an existing node n, checked in this order.  MAPPED: node_point_in_dev != NULL and 0 <= node_point_in[n] <
 *              n_points -- the node keeps that point; any other value (negative, >= n_points) means "no point" and is never
 *              used as an index; two MAPPED nodes of one frame that hold one point are the caller's map and are emitted as they
 *              stand.  CLAIMANT: not MAPPED, the claim arrays given, row_inlier[n] != 0 and 0 <= c = row_point[n] < n_points.  A
 *              claimant is REJECTED (GH_EXT_REJECTED) when its frame holds a MAPPED node of point c or another CLAIMANT of point
 *              c -- every such claimant of that (frame, point) is, and a rejected node takes no further part in anything; in
 *              every other case it is ADOPTED: node_point[n] = c.  Nodes of different frames may adopt one point: that is what
 *              a track is.  FREE: every other existing node.
 *   new tracks an edge counts only when BOTH of its ends are FREE (an edge between a FREE node and a node with a point would
 *              merge or re-assign map points: it is ignored).  Components, the label (the smallest node id), the classes
 *              CONFLICT / SHORT / TRACK and their order of checking are those of gh_link_tracks_dev on the graph of the FREE
 *              nodes; tracks get the ids n_points, n_points + 1, ... in ascending label.
 *   observations  the nodes whose final node_point is >= 0 (MAPPED, ADOPTED, nodes of new tracks) in ascending node id; the
 *              observation index is the rank in that list.
 * Outputs, ALL written for their full capacity on every call (dirty buffers never show): node_point_dev N: the point id,
 * GH_LINK_SHORT, GH_LINK_CONFLICT, GH_EXT_REJECTED or GH_LINK_NO_ROW; obs_cam_dev, obs_point_dev, obs_node_dev N each and
 * obs_xy_dev N x 2 as gh_link_tracks_dev writes them (-1 and (0, 0) past n_obs, ((double)x - cx) / fx: two IEEE operations each);
 * point_len_dev PC: the number of observations of point p, 0 for p >= n_points_total; point_new_dev PC bytes: 1 exactly for
 * n_points <= p < n_points_total; point_grew_dev PC bytes: 1 exactly for the old points with at least one ADOPTED node;
 * totals_dev 6: n_obs, n_points_total, the ADOPTED nodes, the REJECTED nodes, the CONFLICT components, the SHORT components
 * with at least two nodes.  node_point_dev must not overlap node_point_in_dev.
 * The arrays go to gh_triangulate_tracks_dev as they are, with n_cams = n_frames, n_obs = N, n_points = PC and
 * point_select_dev = point_new_dev: only the new points are triangulated, the old points are GH_TRACK_SKIPPED and keep their
 * coordinates, the padding is SKIPPED too.  That call OVERWRITES the status of the skipped points with GH_TRACK_SKIPPED, so a
 * caller keeps the map's status array apart from the one it passes there.
 * Everything is integer work except the two divisions: the same bits on every run.  tests/track_extend_restate.py restates all
 * of it.  With node_point_in_dev NULL (or n_points == 0) and no claim arrays, node_point, the four observation arrays and the
 * first N / 2 entries of point_len equal those of gh_link_tracks_dev on the same inputs byte for byte, and totals [0], [1],
 * [4], [5] equal its totals [0], [1], [2], [3].
 * GH_ERR_ARG, and then nothing is written: ctx NULL; n_frames, cap, npairs or n_points negative; cap > 65535; n_points +
 * n_frames * cap > INT32_MAX - 1; min_views < 2; fx or fy not > 0 (a NaN included); a NULL among kps, counts or the nine
 * outputs; with npairs > 0 a NULL among pair_q, pair_t, idx1; exactly one of row_point_dev / row_inlier_dev NULL.  N == 0:
 * GH_OK, totals_dev is zeros except [1] = n_points and the PC = n_points entries of the three point arrays are zeros.
 * npairs == 0: no new tracks.  Both claim arrays NULL: no adoptions. */
#define GH_EXT_REJECTED (-4)   /* beside GH_LINK_SHORT -1, GH_LINK_CONFLICT -2, GH_LINK_NO_ROW -3 */
gh_status gh_extend_tracks_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const int32_t* counts_dev, int n_frames, int cap,
                               const int32_t* pair_q_dev, const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev,
                               const uint8_t* inlier_dev,
                               const int32_t* node_point_in_dev, int n_points,
                               const int32_t* row_point_dev, const uint8_t* row_inlier_dev,
                               double fx, double fy, double cx, double cy, int min_views,
                               int32_t* node_point_dev, int32_t* obs_cam_dev, int32_t* obs_point_dev, double* obs_xy_dev,
                               int32_t* obs_node_dev, int32_t* point_len_dev, uint8_t* point_new_dev, uint8_t* point_grew_dev,
                               int32_t* totals_dev);
/* Merging map points that the matches show to be one: a track that broke comes back under a second point id, and until the two
 * ids are merged gh_extend_tracks_dev ignores every edge between them and gh_pnp_gather_pairs_dev turns a keypoint that both
 * answer into GH_LOC_AMBIGUOUS.  This call finds the groups of points that the pair matches join, keeps the smallest id of each
 * and renames the others in node_point and in the observation list; no observation moves.  Every pointer is a DEVICE pointer,
 * nothing is copied to the host, the call is asynchronous on the context's stream, scratch comes from the context.  counts_dev,
 * n_frames, cap, pair_q_dev, pair_t_dev, npairs, idx1_dev, inlier_dev (or NULL) as gh_link_tracks_dev takes them.  The map:
 * node_point_in_dev N = n_frames * cap entries as gh_extend_tracks_dev leaves them; n_points is a CAPACITY (the PC of
 * gh_extend_tracks_dev goes in as it is); point_status_dev n_points or NULL; point_xyz_dev n_points x 3 or NULL (no gate);
 * max_dist; bridge; obs_point_in_dev N entries or NULL.
 *   nodes, pairs, edges  exactly the rules of gh_link_tracks_dev: node (f, i) EXISTS when 0 <= i < clamp(counts[f], 0, cap); a pair
 *              is read only when both frame indices are in range and different; query row i of a pair is an edge under the
 *              gather rule of gh_ransac_pairs_dev; an index outside its range drops the row, it is never dereferenced.
 *   classes    point p is USABLE when point_status_dev is NULL or status[p] == GH_TRACK_OK.  An existing node n with 0 <=
 *              node_point_in[n] < n_points is a HOLDER of that point when the point is usable and OUT when it is not.  Any other
 *              existing node (a negative code, a value >= n_points) is a BRIDGE when bridge != 0 and OUT when bridge == 0.  An
 *              edge that touches an OUT node is ignored; a value that is not a valid id is never used as an index.
 *   graph      the elements are the usable points and the BRIDGE nodes; an edge (u, v) links e(u) and e(v), where e(HOLDER) is
 *              its point and e(BRIDGE) the node itself; an edge whose two ends hold the same point links nothing.  A GROUP is a
 *              connected component that contains at least two points, its LABEL the smallest point id in it -- the oldest id
 *              survives -- whatever the order of the pairs.  A component with one point or with none is left exactly as it
 *              is (new tracks are the business of gh_extend_tracks_dev).
 *   verdict    of a group, checked in this order.  CONFLICT: two HOLDER nodes of its points lie in one frame (the merged point
 *              would be seen twice there); two holders of the SAME point that the caller's map already had in one frame count
 *              too; the whole group is left apart, as gh_link_tracks_dev drops a conflicting component.  FAR: point_xyz_dev !=
 *              NULL and some point p of the group fails d2(p, label) <= max_dist * max_dist, with d2 = (dx * dx + dy * dy) +
 *              dz * dz, every difference, product and sum rounded once and nothing fused, max_dist * max_dist one double
 *              product; a NaN fails.  MERGED: otherwise; every point of the group is renamed to the label.
 * Outputs, ALL written for their full capacity on every call (dirty buffers never show): point_remap_dev n_points: the label for
 * the points of MERGED groups, p itself for every other p; point_state_dev n_points bytes: GH_MERGE_NONE, GH_MERGE_SURVIVOR (the
 * label of a MERGED group), GH_MERGE_ABSORBED (its other points), GH_MERGE_CONFLICT / GH_MERGE_FAR (every point of such a group);
 * point_select_dev n_points bytes: 1 exactly at the survivors -- it goes to gh_triangulate_tracks_dev as point_select_dev, as
 * point_new_dev of gh_extend_tracks_dev does, and a survivor keeps its old coordinates until then; node_point_dev N: remap[v]
 * where 0 <= v = node_point_in[n] < n_points, otherwise v copied -- a function of that entry and the remap table alone, for
 * existing and non-existing nodes alike; obs_point_dev N: the same function of obs_point_in_dev (both NULL or both given; the
 * observation list keeps its order and length, obs_cam, obs_xy and obs_node stay valid as they are); point_len_dev n_points: the
 * number of existing nodes whose output node_point equals p, so an absorbed point ends at 0, drops out of gh_ba_window_dev and
 * is unreachable through node_point; totals_dev 6: the MERGED groups, the ABSORBED points, the CONFLICT groups, the FAR groups,
 * the existing nodes whose node_point changed, the points in CONFLICT or FAR groups.  node_point_dev may be node_point_in_dev
 * and obs_point_dev may be obs_point_in_dev (identical or disjoint): the map is updated in place.
 * Everything is integer work except the gate: the same bits on every run.  tests/track_merge_restate.py restates all of it.
 * GH_ERR_ARG, and then nothing is written: ctx NULL; n_frames, cap, npairs or n_points negative; cap > 65535; n_points +
 * n_frames * cap > INT32_MAX - 1; a NULL among counts, node_point_in, point_remap, point_state, point_select, node_point,
 * point_len, totals; exactly one of obs_point_in_dev / obs_point_dev NULL; with npairs > 0 a NULL among pair_q, pair_t, idx1;
 * with point_xyz_dev given, max_dist negative or NaN.  N == 0 or npairs == 0: GH_OK, the identity remap, states and selects 0,
 * totals zeros, node_point and obs_point copied and point_len counted as above. */
#define GH_MERGE_NONE 0
#define GH_MERGE_SURVIVOR 1
#define GH_MERGE_ABSORBED 2
#define GH_MERGE_CONFLICT 3
#define GH_MERGE_FAR 4
gh_status gh_merge_points_dev(gh_ctx* ctx, const int32_t* counts_dev, int n_frames, int cap, const int32_t* pair_q_dev,
                              const int32_t* pair_t_dev, int npairs, const int32_t* idx1_dev, const uint8_t* inlier_dev,
                              const int32_t* node_point_in_dev, int n_points, const int32_t* point_status_dev,
                              const double* point_xyz_dev, double max_dist, int bridge, const int32_t* obs_point_in_dev,
                              int32_t* point_remap_dev, uint8_t* point_state_dev, uint8_t* point_select_dev,
                              int32_t* node_point_dev, int32_t* obs_point_dev, int32_t* point_len_dev, int32_t* totals_dev);
/* Map-point summaries: what a search by projection or a fusion of duplicate points needs per point and the map did not have --
 * the three things ORB-SLAM keeps in MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth: the descriptor of the
 * observation closest, by median Hamming distance, to the point's other observations; the mean direction from which the point
 * was seen; the distance range over which the octave of its reference keypoint predicts it can be found again.  Every pointer
 * is a DEVICE pointer, nothing is copied to the host, the call is asynchronous on the context's stream, scratch comes from the
 * context, nothing is allocated or synchronised per call.  The inputs are the map's arrays as gh_extend_tracks_dev,
 * gh_merge_points_dev and gh_triangulate_tracks_dev leave them, padding included; no count is read back.
 * Inputs: kps_dev n_frames x cap records; desc_dev n_frames x cap x 32 bytes, the descriptors of the same rows (4-byte aligned);
 * counts_dev n_frames; cam_pose_dev n_frames x 7 T_wc, taken as it stands; obs_cam_dev, obs_point_dev, obs_node_dev n_obs each
 * (the N of gh_extend_tracks_dev goes in as it is); obs_use_dev n_obs bytes or NULL (this is where obs_good goes); n_points is a
 * CAPACITY (PC goes in as it is); point_xyz_dev n_points x 3; point_status_dev n_points or NULL: a point is USABLE when
 * point_status_dev is NULL or its status equals GH_TRACK_OK; point_select_dev n_points bytes or NULL (all points); params:
 * gh_point_desc_default_params gives scale_factor 1.2, n_levels 8 (the ORB pyramid) and max_views 64.
 *   nodes      N = n_frames * cap; node n is (frame n / cap, row n % cap) and EXISTS when n % cap < clamp(counts[n / cap], 0, cap).
 *   usable     observation k is usable when (obs_use_dev == NULL || obs_use[k] != 0), 0 <= p = obs_point[k] < n_points,
 *              0 <= n = obs_node[k] < N, node n exists and obs_cam[k] == n / cap.  An index outside its range drops the
 *              observation; it is never dereferenced.
 *   track      of point p: its usable observations in ascending observation index, whatever order the arrays have; the LIVE INDEX
 *              of an observation is its position in that list, L the length of the list.
 *   state      one byte per point, checked in this order: GH_PDESC_SKIPPED point_select_dev is given and point_select[p] == 0;
 *              GH_PDESC_NOT_OK the point is not usable; GH_PDESC_EMPTY L == 0; GH_PDESC_OK otherwise.
 *   descriptor M = min(L, max_views) candidates; candidate c is the observation at live index c when L <= max_views and at
 *              (c * L) / M otherwise (a 64-bit product, integer division: strictly increasing in c).  d(a, b) = the popcount of
 *              the xor of the two 256-bit descriptors; row a holds the M values d(a, .), its own 0 included; med(a) = the
 *              element at index (M - 1) / 2 of the sorted row (ORB-SLAM's vDists[0.5 * (N - 1)]).  Chosen: the candidate with the
 *              smallest med, the lowest c on ties.
 *   direction  IEEE doubles, every operation rounded once, nothing fused.  For each live observation: t = the last three
 *              entries of the pose of frame obs_node / cap; v = X - t entry by entry; r2 = (v0 * v0 + v1 * v1) + v2 * v2;
 *              u = v * (1 / sqrt(r2)).  gh_track_group_lanes() = 8 partial sums, each from +0.0: partial j adds the u of the live
 *              indices with index % 8 == j in ascending order; total = ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7)) entry
 *              by entry, the order of gh_triangulate_tracks_dev; normal = total / (double)L entry by entry.
 *   range      the REFERENCE is live index 0; dist = sqrt(r2 of the reference); level = clamp(kps[its node].octave, 0,
 *              n_levels - 1); max_dist = dist * pow[level]; min_dist = max_dist / pow[n_levels - 1], with pow[0] = 1 and
 *              pow[l] = pow[l - 1] * scale_factor formed on the host in doubles.
 *   NaN        a point that coincides with a camera centre gives 0 * inf: the direction is NaN.  IEEE 754 fixes neither the
 *              sign nor the payload of a NaN that an operation makes (x86 sets the sign, gfx950 does not), so every NaN among the
 *              five doubles is written as the quiet NaN 0x7ff8000000000000.
 * Outputs: point_state_dev n_points bytes, written for EVERY point; point_desc_dev n_points x 32 bytes (4-byte aligned): the
 * chosen descriptor; point_obs_dev n_points x 2: the observation index of the chosen candidate and of the reference;
 * point_views_dev n_points: L; point_normal_dev n_points x 3; point_dist_dev n_points x 2: min_dist, max_dist; totals_dev 4: the
 * OK points, the EMPTY points, the NOT_OK points, the OK points with L > max_views (whose descriptor saw a sample of the track).
 * Everything except the state byte and the totals is IN/OUT: written as above for an OK point; zeros, with -1 in both entries
 * of point_obs, for an EMPTY or NOT_OK point; NOT written for a SKIPPED point -- a caller refreshes only what changed with
 * point_select = point_new | point_grew | the survivors of a merge.  The same inputs give the same bits on every run.
 * tests/point_describe_restate.py restates all of it.
 * GH_ERR_ARG, and then nothing is written: ctx or params NULL; n_frames, cap, n_obs or n_points negative; cap > 65535; n_points +
 * n_frames * cap > INT32_MAX - 1; scale_factor not finite or < 1; n_levels outside 1 .. 32; max_views outside 1 .. 64; a NULL
 * among kps, desc, counts, cam_pose, obs_cam, obs_point, obs_node, point_xyz or the seven outputs; desc_dev or point_desc_dev
 * not 4-byte aligned.  n_points == 0: GH_OK, only totals_dev (zeros) is written.  n_obs == 0 with n_points > 0: every selected
 * usable point is EMPTY. */
#define GH_PDESC_OK 0
#define GH_PDESC_EMPTY 1      /* usable, but no usable observation */
#define GH_PDESC_NOT_OK 2     /* point_status says: not a map point */
#define GH_PDESC_SKIPPED 3    /* point_select says: not this point */
typedef struct gh_point_desc_params {  /* 16 bytes */
  double scale_factor;  /* 1.2 */
  int32_t n_levels;     /* 8 */
  int32_t max_views;    /* 64: the candidates of the descriptor choice, at most 64 */
} gh_point_desc_params;
void gh_point_desc_default_params(gh_point_desc_params* p);
gh_status gh_describe_points_dev(gh_ctx* ctx, const gh_keypoint* kps_dev, const uint8_t* desc_dev, const int32_t* counts_dev,
                                 int n_frames, int cap, const double* cam_pose_dev, const int32_t* obs_cam_dev,
                                 const int32_t* obs_point_dev, const int32_t* obs_node_dev, const uint8_t* obs_use_dev, int n_obs,
                                 int n_points, const double* point_xyz_dev, const int32_t* point_status_dev,
                                 const uint8_t* point_select_dev, const gh_point_desc_params* params, uint8_t* point_state_dev,
                                 uint8_t* point_desc_dev, int32_t* point_obs_dev, int32_t* point_views_dev,
                                 double* point_normal_dev, double* point_dist_dev, int32_t* totals_dev);
/* Search by projection: the consumer of the summaries above.  The searchable points of the map are projected into the frames
 * marked in frame_search_dev (their pose is known: gh_localize_pairs_dev's poses go in as they are), gated by point_dist and by
 * the angle to point_normal, compared with the OPEN keypoints in a window around the projection, and the winners leave as claims
 * in the form gh_extend_tracks_dev takes.  The order of calls is localize -> search -> extend -> triangulate ->
 * describe(point_new | point_grew).  Every pointer is a DEVICE pointer, the call is asynchronous on the context's stream, scratch
 * comes from the context (a function of N = n_frames * cap, n_points and n_frames only, linear in each), nothing is allocated,
 * synchronised or read back per call.
 * Inputs: kps_dev, desc_dev, counts_dev, cam_pose_dev (T_wc, taken as it stands), n_points (a CAPACITY), point_xyz_dev,
 * point_status_dev (NULL, or compared with GH_TRACK_OK) and point_select_dev (NULL: all) as gh_describe_points_dev takes them;
 * point_views_dev, point_desc_dev, point_normal_dev, point_dist_dev as it writes them; frame_search_dev n_frames bytes, non-zero:
 * search this frame; node_point_in_dev N entries or NULL: the map; row_point_in_dev / row_inlier_in_dev N entries each, both or
 * neither: the claims of gh_localize_pairs_dev; fx, fy, cx, cy, width, height: the pinhole and the image; params:
 * gh_search_default_params gives the values noted at the fields.
 *   nodes      node n = f * cap + i EXISTS when i < clamp(counts[f], 0, cap).  An existing node is TAKEN when it is MAPPED
 *              (node_point_in given and 0 <= node_point_in[n] < n_points) or else CLAIMED (claims given, row_inlier_in[n] != 0 and
 *              0 <= row_point_in[n] < n_points); its point is that value.  HELD(f, p): some TAKEN node of frame f has point p.
 *              Every other existing node is OPEN.  A value outside its range is never used as an index.
 *   points     p is SEARCHABLE when point_select is NULL or non-zero at p, point_status is NULL or GH_TRACK_OK at p, and
 *              point_views[p] > 0.
 *   pairs      every (searched frame f, searchable point p) gets exactly one verdict, checked in this order, in IEEE doubles
 *              with + - * / and sqrt, every operation rounded once, nothing fused, in the order written; a comparison with a
 *              NaN fails.  pow[0] = 1, pow[l] = pow[l - 1] * scale_factor, formed on the host.  q, t = the pose of f.
 *              0 HELD          HELD(f, p).
 *              1 BEHIND        d = X - t entry by entry; Xc = quat_rotate((-qx, -qy, -qz, qw), d), the formula under
 *                              gh_triangulate_tracks_dev; BEHIND unless Xc[2] > 1e-9.
 *              2 OUTSIDE       iz = 1 / Xc[2]; u = fx * (Xc[0] * iz) + cx; v = fy * (Xc[1] * iz) + cy; OUTSIDE unless
 *                              0 <= u && u < (double)width && 0 <= v && v < (double)height.
 *              3 RANGE         r2 = (d0 * d0 + d1 * d1) + d2 * d2; dist = sqrt(r2); (min_dist, max_dist) = point_dist[p]; RANGE
 *                              unless dist >= range_lo * min_dist && dist <= range_hi * max_dist.
 *              4 ANGLE         c = ((d0 * n0 + d1 * n1) + d2 * n2) / dist with n = point_normal[p], not renormalised
 *                              (ORB-SLAM's isInFrustum); ANGLE unless c >= min_view_cos.
 *              5 NO_CANDIDATE  level = the number of l in 0 .. n_levels - 2 with pow[l] * dist < max_dist; radius =
 *                              (radius_scale * (c > near_cos ? radius_near : radius_far)) * pow[level].  The CANDIDATES are the
 *                              OPEN nodes i of frame f with level - 1 <= kps[i].octave <= level, fabs((double)kps[i].x - u) <
 *                              radius and fabs((double)kps[i].y - v) < radius: strict, on the widened floats, and nothing else
 *                              decides -- a keypoint with NaN, infinite or out-of-image coordinates obeys the same three
 *                              comparisons.  NO_CANDIDATE when there is none.
 *              6 WEAK          h(i) = popcount(desc[i] xor point_desc[p]) over 256 bits; the candidates are ordered by the key
 *                              (h, i); best is the smallest key, second the next (one candidate: h_second = 256, octave -1).
 *                              WEAK when h_best > max_hamming.
 *              7 RATIO         octave(best) == octave(second) and (double)h_best > nn_ratio * (double)h_second.
 *              otherwise (f, p) PROPOSES node best with distance h_best.  A node takes the proposal with the smallest (h, p):
 *              that pair is 9 WON, every other proposal to the node is 8 LOST.  The result is a function of sets.
 * Outputs, all written for their full capacity on every call: for a node that won p with distance h, row_point[n] = p,
 * row_inlier[n] = 1, row_dist[n] = h.  For every other node row_dist = 0xFFFF, and row_point[n] = row_point_in[n], row_inlier[n]
 * = (row_inlier_in[n] != 0) when the claims were given; otherwise row_point = GH_LOC_NO_POINT for an existing node, GH_LOC_NO_ROW
 * for the others, and row_inlier = 0.  row_point_dev / row_inlier_dev may BE the claim inputs (identical or disjoint); the pair
 * then goes to gh_extend_tracks_dev as it is: no two claimants of a frame share a point and no claimant's point is MAPPED in its
 * frame, so extend's REJECTED rule never fires on what this call adds.  frame_totals_dev n_frames x 10: the pairs of the frame per
 * verdict in the order of the numbers above (zeros for a frame that was not searched); totals_dev 12: the ten column sums, the
 * searched frames, the searchable points (counted when a frame is searched).  The same inputs give the same bytes on every run.
 * tests/search_projection_restate.py restates all of it.
 * GH_ERR_ARG, and then nothing is written: ctx or params NULL; n_frames, cap or n_points negative; cap > 65535; n_points +
 * n_frames * cap > INT32_MAX - 1; width or height < 1; fx or fy not > 0; scale_factor not finite or < 1; n_levels outside 1 .. 32;
 * max_hamming outside 0 .. 256; a NaN among the eight other doubles of params; radius_near, radius_far or radius_scale negative; a
 * NULL among kps, desc, counts, cam_pose, frame_search or the five outputs; with n_points > 0 a NULL among point_xyz and the four
 * summaries; exactly one of the two claim inputs NULL; desc_dev or point_desc_dev not 4-byte aligned.  N == 0: GH_OK, only
 * totals_dev (zeros) is written.  n_points == 0, or no searched frame: GH_OK, the node outputs fall through as above and every
 * count is zero except the searched frames. */
typedef struct gh_search_params {   /* 80 bytes */
  double scale_factor;   /* 1.2 */
  double radius_near;    /* 2.5   window half-width at level 0 when the view is close to the mean direction */
  double radius_far;     /* 4.0 */
  double near_cos;       /* 0.998 */
  double radius_scale;   /* 1.0   ORB-SLAM's th */
  double min_view_cos;   /* 0.5 */
  double range_lo;       /* 0.8 */
  double range_hi;       /* 1.2 */
  double nn_ratio;       /* 0.8 */
  int32_t n_levels;      /* 8 */
  int32_t max_hamming;   /* 100 */
} gh_search_params;
void gh_search_default_params(gh_search_params* p);
int  gh_search_cell_pixels(void);   /* host only: the side of the keypoint grid's cells, so tests can sit on its boundaries */
gh_status gh_search_projection_dev(gh_ctx* ctx,
    const gh_keypoint* kps_dev, const uint8_t* desc_dev, const int32_t* counts_dev, int n_frames, int cap,
    const double* cam_pose_dev, const uint8_t* frame_search_dev,
    const int32_t* node_point_in_dev, const int32_t* row_point_in_dev, const uint8_t* row_inlier_in_dev,
    int n_points, const double* point_xyz_dev, const int32_t* point_status_dev, const uint8_t* point_select_dev,
    const int32_t* point_views_dev, const uint8_t* point_desc_dev, const double* point_normal_dev, const double* point_dist_dev,
    double fx, double fy, double cx, double cy, int width, int height, const gh_search_params* params,
    int32_t* row_point_dev, uint8_t* row_inlier_dev, uint16_t* row_dist_dev, int32_t* frame_totals_dev, int32_t* totals_dev);

/* The local window of a bundle adjustment, selected and compacted on the device: the last arrow of match -> localize -> extend ->
 * triangulate the new points -> BA.  The map's arrays go in as gh_extend_tracks_dev and gh_triangulate_tracks_dev leave them,
 * padding included, with a byte per camera that marks the new frames; out come the compact arrays of a gh_ba_problem (cam_pose,
 * cam_dof, point_xyz, obs_cam, obs_point, obs_xy), the index maps back to the map and eight totals.  The host reads the 32
 * bytes of totals and the compact prefixes and calls gh_ba_solve or gh_ba_graph_create unchanged.  Every pointer is a DEVICE
 * pointer, the call is asynchronous on the context's stream, scratch comes from the context, nothing is synchronised or
 * allocated per call.
 * Inputs: n_cams, n_points, n_obs are CAPACITIES (the N and PC of gh_extend_tracks_dev go in as they are); cam_pose_dev
 * n_cams x 7, point_xyz_dev n_points x 3; obs_cam_dev, obs_point_dev n_obs each and obs_xy_dev n_obs x 2 as
 * gh_triangulate_tracks_dev takes them; obs_use_dev n_obs bytes or NULL (this is where obs_good goes); point_use_dev n_points
 * bytes or NULL: non-zero = the point is in the map (status == GH_TRACK_OK, merged over the caller's calls); cam_seed_dev n_cams
 * bytes: non-zero marks a new frame; cam_hold_dev n_cams bytes or NULL: non-zero = the camera enters the problem with dof 0
 * even if it is LOCAL (frame 0 as the gauge, for instance); params: gh_ba_window_default_params gives min_shared 15
 * (ORB-SLAM's co-visibility threshold) and min_point_obs 2 (a point needs two rays).
 * The rules, each a function of sets and integer counts, never of arrival order:
 *   USABLE     observation k: obs_use is NULL or non-zero at k, 0 <= obs_cam[k] < n_cams, 0 <= obs_point[k] < n_points, and
 *              point_use is NULL or non-zero at that point.  An index outside its range drops the observation and is never
 *              dereferenced.
 *   n_use[p]   the number of usable observations of p.  The same (camera, point) pair given twice counts twice, here and
 *              everywhere below.
 *   LIVE       point p when n_use[p] >= min_point_obs; an observation when it is usable and its point is LIVE.
 *   SEEN[p]    p is LIVE and a live observation of p lies in a seed camera.
 *   shared[c]  the number of live observations of camera c whose point is SEEN.
 *   LOCAL[c]   (cam_seed[c] != 0 and shared[c] >= 1) or shared[c] >= max(min_shared, 1).  A seed camera without a live observation
 *              is not in the window: a camera without observations is a singular block.
 *   window point  p is LIVE and a live observation of p lies in a LOCAL camera.  Every usable observation of a window point is a
 *              WINDOW OBSERVATION.
 *   FIXED[c]   c is not LOCAL and holds a window observation.  Every other camera is NONE.
 *   dof        GH_KF_SE3 for a LOCAL camera with cam_hold NULL or zero; 0 for a held LOCAL camera; 0 for a FIXED camera.
 *   numbering  window cameras (LOCAL and FIXED together) get 0, 1, ... in ascending camera id; window points get 0, 1, ... in
 *              ascending point id; window observations are emitted in ascending observation index.
 * Outputs, ALL written for their full capacity on every call (dirty buffers never show): cam_class_dev n_cams bytes: GH_WIN_NONE,
 * GH_WIN_LOCAL or GH_WIN_FIXED; cam_shared_dev n_cams: shared[c]; cam_slot_dev n_cams and point_slot_dev n_points: the compact id
 * or -1; win_cam_dev n_cams: the original camera id, pad -1; win_cam_dof_dev n_cams: the dof, pad 0; win_cam_pose_dev n_cams x
 * 7: the seven doubles copied bit for bit, pad 0.0; win_point_dev n_points: the original point id, pad -1; win_point_xyz_dev
 * n_points x 3: copied bits, pad 0.0; win_obs_cam_dev, win_obs_point_dev n_obs each: the compact ids, pad -1; win_obs_src_dev
 * n_obs: the original observation index, pad -1; win_obs_xy_dev n_obs x 2: copied bits, pad (0, 0).  totals_dev 8: window
 * cameras, LOCAL cameras, FIXED cameras, LOCAL cameras held at dof 0, window points, window observations, seed cameras in the
 * window, usable observations.
 * GH_ERR_ARG, and then nothing is written: ctx or params NULL; a negative count; min_shared < 0; min_point_obs < 1; a NULL among
 * cam_seed or the fourteen outputs; a NULL among cam_pose, point_xyz or the three observation arrays while the count that sizes
 * it is positive.  n_cams == 0: GH_OK, the totals are zeros and the point and observation outputs are padding.  No seed, or
 * n_obs == 0: an empty window -- everything is padding or NONE and the totals are zeros except the last.
 * tests/ba_window_restate.py restates all of it; the device gives the same bytes on every run and in every order of the
 * observations (the observation outputs up to that order: map them through win_obs_src). */
#define GH_WIN_NONE 0
#define GH_WIN_LOCAL 1
#define GH_WIN_FIXED 2
typedef struct gh_ba_window_params {
  int32_t min_shared;    /* 15 */
  int32_t min_point_obs; /* 2 */
} gh_ba_window_params;
void gh_ba_window_default_params(gh_ba_window_params* p);
gh_status gh_ba_window_dev(gh_ctx* ctx, int n_cams, int n_points, int n_obs, const double* cam_pose_dev,
                           const double* point_xyz_dev, const int32_t* obs_cam_dev, const int32_t* obs_point_dev,
                           const double* obs_xy_dev, const uint8_t* obs_use_dev, const uint8_t* point_use_dev,
                           const uint8_t* cam_seed_dev, const uint8_t* cam_hold_dev, const gh_ba_window_params* params,
                           uint8_t* cam_class_dev, int32_t* cam_shared_dev, int32_t* cam_slot_dev, int32_t* point_slot_dev,
                           int32_t* win_cam_dev, int32_t* win_cam_dof_dev, double* win_cam_pose_dev, int32_t* win_point_dev,
                           double* win_point_xyz_dev, int32_t* win_obs_cam_dev, int32_t* win_obs_point_dev,
                           int32_t* win_obs_src_dev, double* win_obs_xy_dev, int32_t* totals_dev);
/* The way back: the solved poses and points of a window into the map's device arrays.  win_cam_dev, win_cam_dof_dev and
 * win_point_dev as gh_ba_window_dev wrote them; cam_pose_win_dev n_win_cams x 7 and point_xyz_win_dev n_win_points x 3 hold the
 * solved values (DEVICE pointers); n_win_cams and n_win_points are host integers, which the caller has after the solve.  For
 * i < n_win_cams with win_cam_dof[i] != 0 and 0 <= win_cam[i] < n_cams the seven doubles of row i go to row win_cam[i] of
 * cam_pose_dev; for j < n_win_points with 0 <= win_point[j] < n_points the three doubles go to row win_point[j] of
 * point_xyz_dev: copies of bits.  Fixed and held cameras, every camera and point outside the window and padding keep their bits.
 * The ids of one list must be distinct; with duplicates the row that lands is unspecified.  Asynchronous on the context's
 * stream.  GH_ERR_ARG, and then nothing is written: ctx NULL; a negative count; a NULL among the arrays a positive count sizes. */
gh_status gh_ba_window_scatter_dev(gh_ctx* ctx, const int32_t* win_cam_dev, const int32_t* win_cam_dof_dev, int n_win_cams,
                                   const double* cam_pose_win_dev, const int32_t* win_point_dev, int n_win_points,
                                   const double* point_xyz_win_dev, double* cam_pose_dev, int n_cams, double* point_xyz_dev,
                                   int n_points);

/* Optimizer::magin(GSLAM/core/Optimizer.h:230-232, "Convert bundle graph to pose graph"; the reference ships the
 * declaration only): one SE3 edge per pair of cameras (first < second) that share at least min_shared points, with the 6x6
 * information (row-major, [v, w] order of SE3::exp) of the second camera's pose relative to the first held fixed -- the
 * Schur complement of the two-view problem over the shared points at the current estimate, Huber-weighted like
 * gh_ba_solve (specification: oracle_ba_marginalize in oracle/ba_oracle.c).  The measurement of the edge is
 * T_first^-1 T_second of the current poses (the caller forms it).  Edges come sorted by (first, second); *n_edges is
 * always the number found; with max_edges == 0 nothing else is written (size query), with 0 < max_edges < *n_edges the
 * call fails.  edge_shared (may be NULL) = shared points per edge. */
/* The camera order gh_ba_solve / gh_ba_graph_create would use INSIDE the solver for this graph -- host code, no device work, the
 * context plays no part (tests, tools, a caller that wants to know whether its graph reaches the band solver).  BundleGraph::keyframes
 * is a plain vector (GSLAM/core/Optimizer.h:116-119,150-157): nothing says a caller fills it in trajectory order, so the solver
 * orders the reduced camera system for itself, as Ceres' SPARSE_SCHUR does behind Optimizer::optimize (Optimizer.h:229):
 *   the caller's order when it is a band (every point's observers at most 31 camera indices apart) or a band + border as it stands;
 *   otherwise a weighted maximum-adjacency order of the camera co-visibility graph (from a sample of the points), refined by two
 *   barycentre sweeps, then the border of the cameras that long-range points tie to far-away ones.
 * perm_out[n_cams]: old camera of every new position (the identity when the caller's order stands); *n_border: cameras of the dense
 * border at the end of the order; *cam_span: largest distance in new positions between two band observers of one point (the solver
 * takes the band / arrowhead path when 6 * span + 5 <= 192 and at least four superblocks remain); *reordered: 1 when the
 * bandwidth-reducing order was applied.  *n_border_points (NULL: the camera-border choice only): when the long-range POINTS make
 * the smaller border (3 unknowns each against 6 per far camera) they are kept out of the Schur complement and solved for together
 * with the cameras -- then *n_border = 0, no camera moves for them, and *cam_span leaves them out.
 * problem: only n_cams, n_points, n_obs, obs_cam, obs_point are read.
 * GH_ERR_ARG for null pointers or indices out of range.  The environment variable GSLAM_HIP_BA_REORDER=0 keeps gh_ba_solve on the
 * caller's order (A/B measurements); this function always reports the order the default would choose. */
gh_status gh_ba_camera_order(const gh_ba_problem* problem, int32_t* perm_out, int32_t* n_border, int32_t* cam_span,
                             int32_t* reordered, int32_t* n_border_points);

gh_status gh_ba_marginalize(gh_ctx* ctx, const gh_ba_problem* problem, double huber_delta, int32_t min_shared,
                            int32_t max_edges, int32_t* edge_first, int32_t* edge_second, int32_t* edge_shared,
                            double* edge_info, int32_t* n_edges);

/* ---- Pose graph: Optimizer::optimize(BundleGraph&) with se3Graph / sim3Graph / gpsGraph edges ---------------------------
 * Data contract GSLAM/core/Optimizer.h:127-148,162-167: SE3Edge {firstId, secondId, measurement SE3_12 := SE3_1^-1 SE3_2,
 * information 6x6}, SIM3Edge {.., SIM3_12 := SIM3_1^-1 SIM3_2, 7x7}, GPSEdge {frameId, SE3_gps := SE3_frame, 6x6};
 * keyframes are SIM3 T_wc with KeyFrameEstimzationDOF masks incl. UPDATE_KF_SCALE.  The reference ships no solver; the
 * specification is the header of oracle/pg_oracle.c: residual = log(M^-1 * S_first^-1 * S_second) (SE3 edges on the (R, t)
 * part, GPS edges log(M^-1 * T_frame)), cost 1/2 sum r^T Lambda r, update S <- S * SIM3::exp(delta) restricted to the dof
 * mask, central-difference Jacobians, Levenberg-Marquardt on the dense normal equations with the trust-region strategy of
 * gh_ba_solve (options / summary are shared; huber_delta and deterministic are not used: the assembly is always
 * deterministic).  Arrays: frame_sim3 n_frames x 8 [qx qy qz qw tx ty tz s] (in/out); *_meas n x 7 (SE3, GPS:
 * [qx qy qz qw tx ty tz]) or n x 8 (SIM3); *_info row-major 6x6 / 7x7 per edge, NULL = identity. */
typedef struct gh_pg_problem {
  int32_t n_frames;
  double* frame_sim3;
  const int32_t* frame_dof; /* GH_KF_* bits; 0 = fixed (at least one frame should be: the gauge) */
  int32_t n_se3;
  const int32_t *se3_first, *se3_second;
  const double *se3_meas, *se3_info;
  int32_t n_sim3;
  const int32_t *sim3_first, *sim3_second;
  const double *sim3_meas, *sim3_info;
  int32_t n_gps;
  const int32_t* gps_frame;
  const double *gps_meas, *gps_info;
} gh_pg_problem;
gh_status gh_pg_solve(gh_ctx* ctx, gh_pg_problem* problem, const gh_ba_options* options, gh_ba_summary* summary);

/* The GENERAL BundleGraph of Optimizer::optimize (GSLAM/core/Optimizer.h:150-172,229): the keyframes and pose-graph edges
 * of gh_pg_problem PLUS landmarks -- XYZ map points (mappoints, :113-114,155) and inverse-depth points (invDepths,
 * :106-111,152-153: host keyframe, anchor in the host camera, idepth) -- with their pinhole observations (BundleEdge,
 * :121-125,160-161).  This is the path for what gh_ba_solve (SE3 cameras + XYZ points only, the fast path) does not take:
 * inverse-depth points, keyframes with a free scale, pose-graph edges mixed with observations.  The reference holds no
 * implementation: specification and cross-checks in oracle/graph_oracle.c (parity unpinned).  options->huber_delta is
 * OptimzeConfig::projectErrorHuberThreshold (0 = no robust kernel).  Landmarks are eliminated by a Schur complement, the
 * keyframe system (7 n_frames square) is dense.  In/out: pg.frame_sim3, xyz, idp_rho.
 *   xyz n_xyz x 3 world points, xyz_free NULL = all free;  idp_host / idp_anchor (n x 3, pinhole anchors (x, y, 1)) /
 *   idp_rho > 0 / idp_free;  obs_kind 0 = XYZ point, 1 = inverse-depth point; obs_point indexes the respective array;
 *   obs_xy n_obs x 2 normalised image coordinates; obs_info n_obs x 4 row-major 2x2 or NULL.
 * Sphere projection: the residual is the predicted bearing in the tangent plane of the measured one (2-vector, same
 * information / Huber), dropped on the opposite hemisphere. */
typedef struct gh_graph_problem {
  gh_pg_problem pg;
  int32_t n_xyz;
  double* xyz;
  const uint8_t* xyz_free;
  int32_t n_idp;
  const int32_t* idp_host;
  const double* idp_anchor;
  double* idp_rho;
  const uint8_t* idp_free;
  int32_t n_obs;
  const int32_t *obs_kind, *obs_point, *obs_frame;
  const double *obs_xy, *obs_info;
  int32_t projection;        /* 0 = PROJECTION_PINHOLE (obs_xy), 1 = PROJECTION_SPHERE (obs_bearing; Optimizer.h:58-61,175) */
  const double* obs_bearing; /* n_obs x 3 unit bearings, sphere only: anchors are unit bearings too, idepth = 1 / range */
  /* Camera self-calibration -- BundleGraph::camera + cameraDOF (Optimizer.h:86-100,169-171: "Invalid camera indicates idea
   * camera").  intrinsics = fx fy cx cy k1 k2 p1 p2 k3 of GSLAM's OpenCV camera model (GSLAM/core/Camera.h:386-407; a
   * pinhole camera :213-227 has k = p = 0), in / out; NULL = ideal camera.  With intrinsics, obs_xy are PIXELS, the residual
   * is Project(Y) - obs_xy (Huber threshold and obs_info in pixel units), and the parameters whose bit is set in
   * intrinsics_free (bit i = parameter i; CameraEstimationDOF: FOCAL -> bits 0-1, CENTER -> 2-3, K1 4, K2 5, P1 6, P2 7,
   * K3 8) are unknowns of the same Levenberg-Marquardt problem (a 9-row block behind the keyframes in the reduced system).
   * Anchors of inverse-depth points stay normalised.  Pinhole projection only (GH_ERR_ARG with projection = 1). */
  double* intrinsics;
  int32_t intrinsics_free;
} gh_graph_problem;
gh_status gh_graph_solve(gh_ctx* ctx, gh_graph_problem* problem, const gh_ba_options* options, gh_ba_summary* summary);

/* 3-D alignment dst_k ~ s R src_k + t over n correspondences (n x 3 doubles each), Horn's closed form: what
 * Optimizer::optimizeICP (3D-3D correspondences, Optimizer.h:210-217) and Optimizer::fitSim3 (translations of two
 * synchronised trajectories, :220-225) compute.  dof & GH_KF_SCALE decides whether s is estimated (else s = 1).
 * sim3_out 8 doubles [qx qy qz qw tx ty tz s]; information_out (49 doubles, may be NULL) = J^T J of the residuals
 * dst - S exp(delta) src at the solution, rows / columns of masked dof zero; ssq_out (may be NULL) = sum of squared
 * residuals; *ok_out = 0 for fewer than 3 or degenerate (coincident) correspondences.
 * Translation-invariant: the moments are accumulated about the first correspondence (src[0], dst[0]) and the centroids
 * formed as pivot + mean, so R and s come out the same to rounding wherever the two clouds sit (a trajectory in GPS
 * coordinates, 1e6 m from the origin and metres across, loses nothing) and t is exact to the rounding of the centroids.
 * information_out keeps its definition: it is built from the uncentred src, as the Jacobian of a right-multiplied
 * delta is. */
gh_status gh_align_sim3(gh_ctx* ctx, const double* src, const double* dst, int n, int dof, double* sim3_out,
                        double* information_out, double* ssq_out, int* ok_out);

/* Dense SPD solve used by the reduced camera system, exposed for tests and the C5 bench:
 * A_dev is n x n column-major/symmetric (lower triangle read, overwritten by L), b_dev in, x out.
 * *info: 0 = ok; 1 .. n = the matrix is not positive definite (first bad 64-column block, 1-based first column);
 * > n = a single-launch kernel (n <= ~3300 with lda % 16 == 0: factorisation; n <= 8192: back-substitution) could not
 * get all its workgroups resident in bounded time -- rebuild A and retry with GSLAM_HIP_CHOL_FLOW=0 / GSLAM_HIP_BWD_CHAIN=0
 * in the environment (gh_ba_solve does this by itself). */
/* With lda > n the right-hand side rides through the factorisation as row n of A (one launch less per solve, as in the
 * bundle adjustment): the padding rows n .. lda - 1 are scratch then. */
gh_status gh_potrf_solve_dev(gh_ctx* ctx, double* A_dev, int n, int lda, double* b_dev, int* info);

/* The same solve for a BAND matrix by block cyclic reduction (gslam_amd/csrc/chol_cr.hip): what gh_ba_solve uses for the
 * reduced camera system when the cameras only share points with their neighbours along the trajectory (the SPARSE_SCHUR
 * case of the Ceres solve behind GSLAM/core/Optimizer.h:229).  A_dev n x n column-major, lower triangle read and
 * overwritten, A[r][c] = 0 (stored zeros) for r - c > half_bandwidth; lda > n (row n is scratch for the right-hand side);
 * b_dev in, x out.  half_bandwidth <= 192 and n >= 4 superblocks of 64 * ceil(half_bandwidth / 64) columns, else
 * GH_ERR_ARG.  The result equals gh_potrf_solve_dev's up to rounding (a Cholesky factorisation of the odd-even permuted
 * matrix).  The reduction stops when two superblocks survive (four with a border: gh_arrow_solve_dev) and hands the system they
 * form to the dense path (GSLAM_HIP_CR_TOP = 1 .. 16 survivors; 1 = reduce down to the first superblock).
 * *info: 0 = ok; 1 .. n = first column + 1 of a diagonal tile that is not positive definite; > n = a bounded wait inside the dense
 * path's single-launch kernels expired (as gh_potrf_solve_dev reports it; A is overwritten either way). */
gh_status gh_band_solve_dev(gh_ctx* ctx, double* A_dev, int n, int lda, int half_bandwidth, double* b_dev, int* info);

/* ... and for an ARROWHEAD matrix, a band with a dense border: the reduced camera system of a trajectory with a few loop
 * closures once the cameras that long-range points tie to far-away ones are numbered last (what gh_ba_solve does by itself:
 * gh_ba_options.solver / the arrow ordering of gslam_amd/csrc/ba.hip; the graphs global BA exists for,
 * GSLAM/core/Optimizer.h:127-148,229).  The first n_band unknowns form the band (A[r][c] = 0 for r - c > half_bandwidth,
 * r < n_band), rows n_band .. n - 1 are dense.  Block cyclic reduction on the band with the border rows riding along as extra
 * rows of every eliminated superblock, then the dense system of the surviving superblocks + the border through the dense
 * factorisation.  Same limits on the band as gh_band_solve_dev; the result equals gh_potrf_solve_dev's up to rounding. */
gh_status gh_arrow_solve_dev(gh_ctx* ctx, double* A_dev, int n, int lda, int n_band, int half_bandwidth, double* b_dev,
                             int* info);
/* The COMPACT storage gh_ba_solve keeps its reduced camera system in when the band / arrowhead solver runs (round 6): a column
 * holds the rows block cyclic reduction ever touches -- 0.93 GB instead of the 28.8 GB of the dense lower triangle at C5.
 * gh_cr_compact_layout: for n_band band unknowns of `half_bandwidth` and nbr border unknowns, *lda = doubles per column, *m =
 * superblock columns, *brow = local row of the first border row.  Element (r, c), r >= c (plus the strictly upper part of a
 * column's own 64 x 64 diagonal tile, which is never read as data), at A[c * lda + local(r, c)]:
 *     r >= n_band                          brow + (r - n_band)        border rows; the right-hand side is local row brow + nbr
 *     I - J <= 1  (I = r / m, J = c / m)    r - J * m                  the band
 *     I - J = 2^k, k >= 1                   (1 + k) * m + (r - I * m)  the fill of the reduction: ZERO on entry
 * Returns 0 when the band does not fit the solver (more than 192 wide or fewer than four superblocks).
 * gh_arrow_solve_compact_dev: gh_arrow_solve_dev on such a matrix (n_band == n: a band without a border); A_dev is overwritten,
 * b_dev (n doubles) receives x.  Test / tool entries: gh_ba_solve builds the layout itself. */
int gh_cr_compact_layout(int n_band, int half_bandwidth, int nbr, int* lda, int* m, int* brow);
gh_status gh_arrow_solve_compact_dev(gh_ctx* ctx, double* A_dev, int n, int lda, int n_band, int half_bandwidth, double* b_dev,
                                     int* info);

/* Structure of the border through the reduction (host only, no GPU; what gh_ba_solve computes once per topology when the
 * border block has 4 M entries or more, so that the border kernels of the arrowhead solver skip what stays zero).
 * tiles = 64-column tiles per superblock (1 .. 3, as the solver picks them for the half-bandwidth); with m = 64 tiles,
 * N = ceil(n_band / m), nbs = ceil(nbr / 16), ntr = ceil((nbr + 1) / 64):
 *   init[i * nbs + t] != 0  iff  the 16-row strip t of the border rows has a structural non-zero among the band columns of
 *                                superblock i (a border camera and a band camera that see a common point);
 *   out: N * nbs bytes -- the strips that can be non-zero in superblock i at the moment the reduction eliminates it (all set
 *        for the superblocks that survive into the dense system) -- then N * ntr bytes, the same per 64-row tile of the
 *        corner (the tile that holds the right-hand-side row always set).
 * Returns the bytes `out` needs (0 = bad arguments); fills `out` when it is non-NULL and out_bytes suffices. */
size_t gh_cr_border_structure(int n_band, int tiles, int nbr, const uint8_t* init, uint8_t* out, size_t out_bytes);

/* Block-sparse Cholesky with a dense root: the linear solver gh_pg_solve uses for LARGE pose graphs
 * (GSLAM/core/Optimizer.h:127-148,162-167 -- se3Graph / sim3Graph / gpsGraph over thousands of keyframes; the system has
 * one 7 x 7 block per keyframe and one per edge).  Exposed for tests and tools:
 * gh_bs_symbolic (host only, no GPU): the elimination order of the keyframe graph given its distinct frame pairs --
 *   rounds of independent low-degree keyframes (cyclic reduction on an odometry chain), the rest is the dense root.
 *   counts_out[5] = {sparse columns, root keyframes, rounds, below-diagonal blocks incl. fill, 7 x 7 block products};
 *   pos_out[n_frames] frame -> position; round_ptr_out[rounds + 1]; colptr_out[sparse columns + 1]; rows_out = row
 *   positions of the blocks of each sparse column, ascending (any of the arrays may be NULL).
 * gh_bs_solve_host: (H + clamp(diag H, 1e-6, 1e32) / radius) x = -g for a symmetric positive definite H given by its
 *   diagonal blocks diag[n_frames][49] and off-diagonal blocks off[n_pairs][49] (block (row frame prow[k], column frame
 *   pcol[k]), both column-major); g, x_out[7 n_frames].  *info: 0 ok, > 0 a non-positive pivot.
 * root_min: keyframes kept for the dense root at least; max_rounds: bound on the elimination rounds. */
gh_status gh_bs_symbolic(int n_frames, int n_pairs, const int32_t* prow, const int32_t* pcol, int root_min, int max_rounds,
                         int32_t* pos_out, int64_t* counts_out, int32_t* round_ptr_out, int round_cap, int32_t* colptr_out,
                         int32_t* rows_out, int rows_cap);
gh_status gh_bs_solve_host(gh_ctx* ctx, int n_frames, int n_pairs, const int32_t* prow, const int32_t* pcol, const double* diag,
                           const double* off, const double* g, double radius, int root_min, int max_rounds, double* x_out,
                           int* info);

#ifdef __cplusplus
}
#endif
#endif /* GSLAM_HIP_H_ */
