/*
 * gem_hip.h -- C ABI of the MI355X (gfx950) window optimiser for GlobalEgoMocap's hot path.
 *
 * The reference has no FFI of its own: its boundary for this path is two Python call signatures
 * (optimizer.py:311-314 `main`, optimizer.py:242-276 `optimize_pose_seq_pytorch_LBFGS`) plus the
 * checkpoint / pickle / camera-json schemas.  This header is what a Python
 * (ctypes) binding of those two calls binds to; `globalegomocap_amd/_capi.py` is that binding and
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every entry point returns 0 on success, non-zero on failure; `gem_last_error()` gives the text
 *     (thread-local).  Nothing is printed, nothing aborts.
 *   - `d_*` arguments are DEVICE pointers owned by the caller (e.g. torch tensors); the library never
 *     frees or keeps them beyond the call.  `h_*` are host pointers.
 *   - `stream` is a hipStream_t passed as void*; all work of a call is enqueued on it, no call
 *     synchronises the device (except gem_create / gem_load_vae / gem_destroy, which allocate).
 *   - one handle per device; a handle is not thread-safe; no hidden RNG (eps is an input, D5).
 *   - windows are independent: `B` windows per call, each T frames x J joints (T=10, J=15).
 */
#ifndef GEM_HIP_H
#define GEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEM_MAX_HIDDEN 8
#define GEM_MAX_POLY 16
#define GEM_MAX_JOINTS 16

typedef struct gem_handle gem_handle;

/* Geometry of the path.  Replaces the constructor arguments of BodyPoseOptimizer
 * (optimizer.py:36-71), ConvVAE (networks/models/SeqConvVAE.py:11-30) and
 * FishEyeCameraCalibrated (utils/fisheye/FishEyeCalibrated.py:7-15). */
typedef struct gem_config {
    int32_t seq_len;                    /* T, frames per window (10) */
    int32_t n_joints;                   /* J (15) */
    int32_t latent_dim;                 /* D (2048) */
    int32_t n_hidden;                   /* number of encoder conv blocks (5) */
    int32_t hidden[GEM_MAX_HIDDEN];     /* encoder channel widths (64,64,128,256,512) */
    int32_t heat_h, heat_w;             /* heat-map size (64,64) */
    int32_t n_poly;                     /* number of polynomialW2C coefficients (11 or 14) */
    double  poly[GEM_MAX_POLY];         /* rho(theta) = sum poly[i] theta^i */
    double  cx, cy;                     /* image centre = intrinsic[0][2], intrinsic[1][2] */
    int32_t parents[GEM_MAX_JOINTS];    /* kinematic parents (optimizer.py:34) */
    int32_t max_windows;                /* capacity: largest B any call will pass */
    int32_t device;                     /* HIP device ordinal */
} gem_config;

/* Energy weights = BodyPoseOptimizer.set_weights (optimizer.py:73-79); gmm_weight is accepted by the
 * Python mirror and ignored exactly as the reference ignores it (D4). */
typedef struct gem_energy_weights {
    double w3d, smooth, bone, vae, reproj;
} gem_energy_weights;

/* torch.optim.LBFGS arguments as used at optimizer.py:261-262 (+ _strong_wolfe's constants). */
typedef struct gem_lbfgs_opts {
    double  lr;             /* 2 */
    int32_t max_iter;       /* 25 */
    int32_t max_eval;       /* max_iter*5/4 = 31 */
    int32_t history;        /* 100 (never reached: at most max_iter-1 pairs) */
    int32_t reserved;
    double  tol_grad;       /* 1e-7 */
    double  tol_change;     /* 1e-6 */
    double  c1, c2;         /* 1e-4, 0.9 */
    double  ls_tol_change;  /* 1e-9 */
} gem_lbfgs_opts;

typedef struct gem_window_stats {
    int32_t n_iter;         /* state['n_iter'] */
    int32_t func_evals;     /* state['func_evals'] */
    float   final_loss;
    int32_t status;         /* bit 0: finished (0 = still running: a bug); bit 1: a closure value was NaN -- a joint exactly on
                             * the optical axis, where the reference raises Exception("norm is zero!") (FishEyeCalibrated.py:124-127) */
} gem_window_stats;

enum { GEM_STAGE_LOCAL = 0, GEM_STAGE_GLOBAL = 1 };

const char* gem_last_error(void);
int gem_version(void);

/* BodyPoseOptimizer.__init__ minus checkpoint loading. */
int  gem_create(const gem_config* cfg, gem_handle** out);
void gem_destroy(gem_handle* h);

/* Accepted for compatibility and otherwise ignored: every gem_optimize_windows call runs as one lane.  (The two-lane schedule it
 * used to switch on -- two half-batches on two streams, shifted by half an evaluation round -- measured slower than one lane,
 * 247-259 k vs 289 k windows/s at 8192 windows, and is no longer in the library: DESIGN.md section 2.)  min_windows must be >= 0. */
int gem_set_lanes(gem_handle* h, int min_windows);

/* Arithmetic of the decoder / encoder products (every energy term is always fp32 arithmetic on the fp32 decoded pose):
 *   0 = fp32 MFMA everywhere (default, BASELINE configs[1]);
 *   1 = "bf16x3": operands of the wide products split into bf16 hi+lo, three bf16 MFMAs per product, fp32 accumulate
 *       (error ~2^-16 relative, i.e. fp32-grade, at ~1.5x the fp32 rate); the narrow tail layers stay fp32;
 *   2 = bf16 operands, fp32 accumulate (BASELINE configs[2..4] "bf16 VAE decoder / fp32 energy"): the wide products always; the
 *       narrow tail layers too, at every batch size (csrc/tail_bf16.hip: bf16 weights and bf16 activations between the layers;
 *       1..8 windows per workgroup, chosen from the batch size, every choice bitwise the same (asserted by the tests; the library
 *       is compiled with -ffp-contract=on so that no template instantiation fuses multiply-adds differently from another) -- so the
 *       tail's part of a window's bf16 result does not depend on the size of the batch it arrives in.  It is the fp32 result plus zero-mean noise of the order of 2^-9 per decoded
 *       coordinate (tests/test_hip_full_size.py::test_bf16_on_fitted_vae_against_the_oracle: ~1.3 mm per window on fitted
 *       weights, 0.06 mm on a sequence's MPJPE).
 * May be switched at any time between calls. */
enum { GEM_PRECISION_F32 = 0, GEM_PRECISION_BF16X3 = 1, GEM_PRECISION_BF16 = 2 };
int gem_set_precision(gem_handle* h, int mode);

/* network.load_state_dict(torch.load(path)['state_dict']) (optimizer.py:59-63).  `h_blobs[i]` is the
 * i-th float32 tensor of the state_dict in the order of globalegomocap_amd.vae.VAEShape.schema(),
 * `n_elem[i]` its element count (checked).  BatchNorm (eval) is folded into the convolutions and the
 * weights are re-packed for the MFMA kernels inside. */
int gem_load_vae(gem_handle* h, int stage, int n_blobs, const float* const* h_blobs, const int64_t* n_elem);

/* mean_bone_length of a chunk (optimizer.py:42-43,89-94): d_pose [n_frames,J,3] f32 -> d_out [J] f32. */
int gem_mean_bone_length(gem_handle* h, const float* d_pose, int n_frames, float* d_out, void* stream);

/* ConvVAE.get_latent_space (SeqConvVAE.py:184-189): d_pose [B,T,J*3] f32, d_eps [B,D] f32 (may be
 * NULL: z = mu).  Any of d_mu/d_logvar/d_z may be NULL. */
int gem_encode(gem_handle* h, int stage, int B, const float* d_pose, const float* d_eps,
               float* d_mu, float* d_logvar, float* d_z, void* stream);

/* ConvVAE.decode_to_bodypose (SeqConvVAE.py:131-140): d_z [B,D] -> d_pose [B,T,J,3] f32. */
int gem_decode(gem_handle* h, int stage, int B, const float* d_z, float* d_pose, void* stream);

/* total_loss + backward at fixed z (optimizer.py:226-240, 264-268), for parity tests:
 * d_pose_init [B,T,J,3] f32 (the stage's input pose), d_heat [n_frames,H,W,J] f32 (pickle layout,
 * may be NULL when reproj == 0), d_frame0 [B] int32 first frame of each window, d_mean_bone [B,J] f32.
 * Outputs (each may be NULL): d_energy [B] f64, d_parts [B,5] f64 (E_3d,E_smooth,E_bone,E_vae,E_reproj),
 * d_dz [B,D] f32, d_pose [B,T,J,3] f32 (decoded pose). */
int gem_energy_grad(gem_handle* h, int stage, int B, const float* d_z, const float* d_pose_init,
                    const float* d_heat, const int32_t* d_frame0, const float* d_mean_bone,
                    const gem_energy_weights* w, double* d_energy, double* d_parts, float* d_dz,
                    float* d_pose, void* stream);

/* BodyPoseOptimizer.optimize_pose_seq_pytorch_LBFGS for B windows at once (optimizer.py:242-276):
 * encode -> L-BFGS/strong-Wolfe over z through decoder + energies -> decode.
 * d_pose_in [B,T,J,3] f32, d_eps [B,D] f32, d_pose_out [B,T,J,3] f32, d_stats [B] (may be NULL). */
int gem_optimize_stage(gem_handle* h, int stage, int B, const float* d_pose_in, const float* d_heat,
                       const int32_t* d_frame0, const float* d_mean_bone, const float* d_eps,
                       const gem_energy_weights* w, const gem_lbfgs_opts* opt, float* d_pose_out,
                       gem_window_stats* d_stats, void* stream);

/* Closure values of the LAST stage run on this handle (the `total_loss` values torch.optim.LBFGS.step's closure returned,
 * optimizer.py:263-268): d_out [n_rounds][B] f64, row r = the value window b's optimiser consumed in evaluation round r,
 * NaN once the window had finished (a window's evaluations are rounds 0..func_evals-1).  n_rounds <= 64.  For parity
 * tests against the reference's closure traces; after gem_optimize_windows it holds the global stage's values. */
int gem_read_trace(gem_handle* h, int B, int n_rounds, double* d_out, void* stream);

/* ---- For parity tests: the L-BFGS / strong-Wolfe state machine (csrc/lbfgs.hip) stepped alone -------------------------------
 * These three calls launch the kernels of the evaluation rounds exactly as a stage does (same launchers, same arguments),
 * but the caller plays the decoder and the energy: it reads the trial points, evaluates whatever objective it likes and hands
 * (f, g) back.  They need no VAE weights.  They are test hooks, not part of the reference's surface.
 *
 * gem_lbfgs_debug_begin: d_x0 [B,D] f32 becomes the trial point of every window (padded to pad64(D) with zeros; in bf16
 * precision the bf16 copy is written too), the states are reset and the identity compaction runs, as at the start of a stage.
 * `slots` selects how the later rounds address gradient rows:
 *   0  no slot table (slot_of == nullptr in the kernel): row b belongs to window b;
 *   1  compact_kernel runs between the rounds: windows still iterating take slots [0, count) in window order;
 *   2  lbfgs_advance hands out the next round's slots itself (two alternating perm / slot_of sets and one zeroed counter per
 *      round, as a stage with atomic slots arranges them): slots [0, count) in arrival order.
 *
 * gem_lbfgs_debug_advance: one evaluation round.  d_f [B] f64 is indexed by window.  d_g is [max(n_slabs,1)][B][D] f32: row
 * slot_of[b] (gem_lbfgs_debug_read) belongs to window b, and the slabs sum to the gradient.  n_slabs == 0: the rows are the
 * finished gradient (the kernel reads them where the decoder's backward product leaves dE/dz); n_slabs >= 1: the rows go to the
 * split-K scratch as that many slabs with a STATIC cut (slab z at z * B * pad64(D)) and the kernel sums them, in slab order.
 * The device-adaptive cut of the stage rounds (a slab count computed on the device from the live row count) is out of scope
 * here.  `opt` is checked as gem_optimize_stage checks it; B must be the B of the begin call; n_slabs * B * pad64(D) must fit
 * the scratch.  At most max_eval + 1 calls are ever needed; a call for a finished window changes nothing.
 *
 * gem_lbfgs_debug_read: every pointer may be NULL.  d_state [B] gem_lbfgs_debug_state; d_x, d_d, d_trial [B,D] f32 (unpadded).
 * In bf16 precision the kernel writes only the bf16 trial point: d_trial then holds those bf16 values widened to f32.
 * d_slot_of [B] int32 and d_count [1] int32: the slot table and the live count of the NEXT advance call (slots == 0: the
 * identity and B; entries of finished windows are meaningless).
 *
 * A stage call after a debug run behaves as on a fresh handle. */
typedef struct gem_lbfgs_debug_state {
    int32_t phase;          /* 0 INIT, 1 BRACKET, 2 ZOOM, 3 DONE */
    int32_t n_iter, evals, ls_iter, ls_evals, hist_count, hist_start, low, high, insuf, nan_seen;
    int32_t pad_nonzero;    /* padding columns D..pad64(D)-1 of x, d and the trial point (bf16 precision: the bf16 one) that are not zero */
    double  t, loss, gtd, d_norm, H_diag;
} gem_lbfgs_debug_state;
int gem_lbfgs_debug_begin(gem_handle* h, int B, const float* d_x0, int slots, void* stream);
int gem_lbfgs_debug_advance(gem_handle* h, int B, const gem_lbfgs_opts* opt, const double* d_f, const float* d_g, int n_slabs,
                            void* stream);
int gem_lbfgs_debug_read(gem_handle* h, int B, gem_lbfgs_debug_state* d_state, float* d_x, float* d_d, float* d_trial,
                         int32_t* d_slot_of, int32_t* d_count, void* stream);

/* ---- For parity tests: ONE layer through one of the two GEMM dispatch functions -------------------------------------------
 *   C[M,N] = epi( sum_tap shift_tap(A)[M,K] . W[tap][N][K]^T + bias ),  row = window * T + frame, lda = K, ldc = N
 * launch_gemm (csrc/gemm_f32.hip, forwards to launch_gemm_bf16 in the bf16x3 / bf16 precision modes) or gemm_bf16a
 * (csrc/decoder_bf16.hip).  The entry adds no kernel and changes no dispatch rule: which kernel runs is decided by the
 * dispatch function from the shape, the epilogue, the handle's precision mode and compute-unit count and the options below,
 * as in a stage.  A test hook, not part of the reference's surface; it needs no VAE weights.
 *
 * gem_gemm_debug_layer_create: taps 1 | 3, N % 64 == 0, K % 32 == 0 (already padded), h_w [taps][N][K] and h_bias [N] host
 * fp32.  The fp32 image and the bf16 hi / lo images are made and uploaded by the code gem_load_vae uses.  The layer lives until
 * gem_gemm_debug_layer_destroy or gem_destroy.
 *
 * gem_gemm_debug_run is synchronous.  Every argument is checked before anything is launched (the row map and the device row
 * count are read back for that); a bad argument is an error return.  When a.defer is set and the dispatch function leaves
 * split-K slabs to its consumer, the entry plays the consumer with the library's own reduce pass (epilogue included), which
 * writes fp32.  names gets the launched kernels' names ("; " separated, as gem_profile_kernels prints them; the reduce passes
 * are not listed), info[0..3] = {slabs left to the consumer (0: none), workgroup count of a device-side cut (0: static cut),
 * 1 when d_C holds bf16 / 0 for fp32, 0}. */
typedef struct gem_gemm_debug_layer gem_gemm_debug_layer;
typedef struct gem_gemm_debug_args {
    int32_t route;           /* 0 launch_gemm, 1 gemm_bf16a */
    int32_t epi;             /* 0 bias, 1 bias + LeakyReLU, 2 mask (conv layers only; needs d_aux), 3 none */
    int32_t M, T;            /* rows; frames per window (conv layers: M % T == 0; gemm_bf16a: T == seq_len) */
    int32_t a_rows;          /* rows of d_A (>= M unless a row map gathers them) */
    int32_t family;          /* profiling family of the call site, -1 .. 3 (0 = the front products: picks some instantiations) */
    int32_t out_bf16;        /* gemm_bf16a: d_C bf16 (unless slabs are left to the consumer, see above) */
    int32_t allow_split;     /* gemm_bf16a */
    int32_t defer;           /* "the consumer takes slabs" (gemm_bf16a: only with allow_split) */
    int32_t reserved;
    const float* d_A;        /* [a_rows, K] fp32; gemm_bf16a: converted to bf16 first */
    const float* d_aux;      /* [M, N] fp32 or NULL (same conversion) */
    void* d_C;               /* [M, N] fp32 or bf16 */
    const int32_t* d_rows;   /* NULL or device {m, m * T}, 0 <= m <= M: the row count of an evaluation round */
    const int32_t* d_row_map;/* NULL or device [M] rows of d_A (linear layers only) */
} gem_gemm_debug_args;
int gem_gemm_debug_layer_create(gem_handle* h, int taps, int N, int K, const float* h_w, const float* h_bias,
                                gem_gemm_debug_layer** out);
int gem_gemm_debug_layer_destroy(gem_handle* h, gem_gemm_debug_layer* layer);
int gem_gemm_debug_run(gem_handle* h, const gem_gemm_debug_layer* layer, const gem_gemm_debug_args* a, char* names, int names_len,
                       int32_t* info, void* stream);

/* The window loop body of main() (optimizer.py:370-423) for B windows at once: local stage,
 * relative-global transform X_rel[t] = C0^-1 C_t X_loc[t] in float64 (utils/utils.py:99-112), global
 * stage, X_glob = C0 X_rel (optimizer.py:302-308).
 *   d_local_pose [n_frames,J,3] f32   estimated_local_skeleton, frames stored once
 *   d_cams       [n_frames,4,4] f64   camera_pose_list
 *   d_heat       [n_frames,H,W,J] f32 heatmap_list
 *   d_frame0     [B] int32            first frame of each window
 *   d_mean_bone  [B,J] f32
 *   d_eps_local / d_eps_global [B,D] f32
 * Outputs: d_mid_local [B,T,J,3] f32 (stage-A result, may be NULL), d_global [B,T,J,3] f64
 * (refined global pose), d_stats [2*B] (local stats then global stats, may be NULL). */
int gem_optimize_windows(gem_handle* h, int B, const float* d_local_pose, const double* d_cams,
                         const float* d_heat, const int32_t* d_frame0, const float* d_mean_bone,
                         const float* d_eps_local, const float* d_eps_global,
                         const gem_energy_weights* w_local, const gem_energy_weights* w_global,
                         const gem_lbfgs_opts* opt, float* d_mid_local, double* d_global,
                         gem_window_stats* d_stats, void* stream);

/* The reprojection term (optimizer.py:139-149) keeps the four heat-map texels under every joint from one evaluation of a
 * stage to the next and re-reads them as one record while the joint stays inside the same texel block (same values, bit for
 * bit; fewer scattered cache lines).  On by default; this switch exists so that a test can prove "bit for bit". */
int gem_set_texel_cache(gem_handle* h, int on);

/* hipGraph replay of whole optimisation calls (BASELINE configs[4] "hipGraph-captured inner step"; the loop being captured
 * replaces optimizer.py:261-270 for every window of the call).  With graphs on, gem_optimize_stage / gem_optimize_windows
 * run eagerly the first time they see a given signature (batch size, precision, every pointer argument, weights, options,
 * stream), capture the second call into a hipGraph and replay that graph from then on: one hipGraphLaunch instead of ~700
 * kernel launches per call.  Results are bitwise those of the eager path.  Needs a non-default stream (the legacy default
 * stream cannot be captured: such calls stay eager) and profiling off.  The caller must pass the SAME buffers to get
 * replays; a call with other pointers is a new signature (at most 16 are cached per handle).
 * A captured call holds the ADDRESSES of the caller's buffers.  A caller that frees buffers a captured call used must call
 * gem_graph_enable(h, 0) first -- it synchronises the device and drops every cached graph (gem_graph_enable(h, 1) switches replay
 * on again) -- so that no graph can be replayed on whatever is allocated at those addresses next (ROCm 7.2: such a replay ended in
 * a GPU memory access fault even with equally sized new buffers at the same addresses).
 * gem_graph_stats: number of captures and replays so far. */
int gem_graph_enable(gem_handle* h, int on);
int gem_graph_stats(gem_handle* h, int64_t* n_captures, int64_t* n_replays);

/* ---- sequence post-processing: the reporting side of the path, on the same stream ----
 * Both calls may grow an internal scratch buffer (hipMalloc, synchronous) the first time a larger sequence is seen. */

/* merge_batches (optimizer.py:425-437) per chunk, then optionally gaussian_filter1d(sigma=1, axis=0) per chunk
 * (optimizer.py:448-450).  d_windows [n_chunks*windows_per_chunk, T, J, 3] f64 (e.g. d_global of
 * gem_optimize_windows) -> d_out [n_chunks*frames_per_chunk, J, 3] f64 with
 * frames_per_chunk = windows_per_chunk*(T-overlap)+overlap. */
int gem_merge_windows(gem_handle* h, const double* d_windows, int n_chunks, int windows_per_chunk, int overlap,
                      int smooth, double* d_out, void* stream);

/* calculate_errors (calculate_errors.py:114-179): d_est / d_mid / d_opt / d_gt [n_frames,J,3] f64 (metres),
 * h_bone_mm [J] reference bone lengths in mm (utils/skeleton.py:102-110).  d_out [17+J] f64 in the order of
 * the reference's result dict: original/mid/optimized_global_mpjpe, original/optimized_camera_pos_error,
 * original/mid/optimized aligned camera error, original/mid/optimized sequence-aligned mpjpe,
 * per-frame-Procrustes mpjpe x3, bone-length-normalised mpjpe x3, joints_error[J].
 * Includes the batched 3x3 SVD Umeyama (utils/rigid_transform_with_scale.py:18-43) and the skeleton
 * re-growth (utils/skeleton.py:124-136).  Needs n_joints >= 12 (hip joints 7 and 11). */
int gem_calculate_errors(gem_handle* h, const double* d_est, const double* d_mid, const double* d_opt,
                         const double* d_gt, int n_frames, const double* h_bone_mm, double* d_out, void* stream);

/* gem_calculate_errors for each of n_chunks equally long sequences laid end to end (d_* [n_chunks*frames_per_chunk,J,3] f64) in ONE
 * call: the per-chunk `main()` reports that optimize_whole_sequence.py:55-104 collects.  d_out [n_chunks][17+J] f64. */
int gem_calculate_errors_chunks(gem_handle* h, const double* d_est, const double* d_mid, const double* d_opt, const double* d_gt,
                                int n_chunks, int frames_per_chunk, const double* h_bone_mm, double* d_out, void* stream);

/* A per-chunk report that needs no ground truth: what the reference's energy terms (optimizer.py:139-149,
 * 172-177,202-213) say about merged sequences.  For n_chunks chunks of frames_per_chunk merged frames each (merged frame f of a
 * chunk is the chunk's frame f):
 *   d_seq       [n_chunks*frames_per_chunk,J,3] f64   the sequences in their chunks' global frames (e.g. what gem_merge_windows wrote)
 *   d_cams      [n_frames,4,4] f64, d_heat [n_frames,H,W,J] f32   the frame buffers the optimiser was given
 *   d_frame0    [n_chunks] i64    each chunk's first frame in those buffers; a frame outside [0, n_frames) is not read and
 *                                 makes column 0 NaN
 *   d_mean_bone [n_chunks,J] f32  the chunks' mean bone lengths (gem_mean_bone_length)
 *   d_ref       like d_seq, or NULL
 * d_out [n_chunks][4] f64:
 *   0 heatmap_response  mean over frames and joints of the bilinear heat-map sample (zeros outside, align_corners=True) at the
 *                       projection of X_cam = C_f^-1 X (rigid inverse in f64, rounded once to f32; projection, heat-map coordinates
 *                       and sample in the fp32 arithmetic of the optimiser's reprojection term); NaN when a joint lies exactly on
 *                       the optical axis
 *   1 bone_length_rms   sqrt(mean over frames and the bones j with parent(j) != j of (|X_j - X_parent(j)| - mean_bone_j)^2), metres
 *   2 acceleration      mean over frames 1 .. frames_per_chunk-2 and joints of |X[f-1] - 2 X[f] + X[f+1]|
 *   3 displacement      mean over frames and joints of |X - ref|; NaN when d_ref is NULL
 * Sums are f64 in a fixed order: two calls give the same bits.  Two launches whatever n_chunks; may grow the scratch buffer. */
int gem_sequence_quality(gem_handle* h, const double* d_seq, const double* d_cams, const float* d_heat, int64_t n_frames,
                         const int64_t* d_frame0, const float* d_mean_bone, const double* d_ref, int n_chunks, int frames_per_chunk,
                         double* d_out, void* stream);

/* ---- input lifting: raw network outputs -> estimated_local_skeleton ----
 * Skeleton.set_skeleton_from_file + set_skeleton + get_max_preds (utils/skeleton.py:74-90,32-45,176-204) followed by
 * FishEyeCameraCalibrated.camera2world (utils/fisheye/FishEyeCalibrated.py:18-33), without the bone-length resize
 * (the reference's data preparation passes bone_length_file=None, MakeDataForOptimization/process_test_data.py:59-62).
 *   d_heat   [n_frames,H,W,J] f32   heat-maps as stored in the .mat files / the pickle
 *   d_depth  [n_frames,J] f64       predicted joint distances
 *   h_poly_c2w                      the calibration's polynomialC2W (ascending powers)
 *   upscale, pad_x, pad_y           16, 128, 0: cv2.resize(64 -> 1024, INTER_NEAREST) + np.pad 128 columns each side
 * Outputs (either may be NULL): d_out64 [n_frames,J,3] f64 (what the reference pickles), d_out32 the same as f32
 * (what gem_optimize_windows consumes).  Family 3 of the profiling hook times this kernel (bytes instead of flops). */
int gem_lift_skeleton(gem_handle* h, const float* d_heat, const double* d_depth, int n_frames, const double* h_poly_c2w,
                      int n_poly_c2w, int upscale, int pad_x, int pad_y, double* d_out64, float* d_out32, void* stream);

/* ---- chunk files: `<chunk>/test_data.pkl` as the reference writes and reads it ----
 * The file is a pickled dict of lists of numpy arrays (written at MakeDataForOptimization/process_test_data.py:149-157, read at
 * optimizer.py:315-324); its heat-maps are what scipy.io.loadmat returned (process_test_data.py:65-67): [H,W,J] arrays in
 * FORTRAN order, float32 or float64.  These calls take such a file to the device without building a Python object per array.
 * None of them needs a gem_handle; the host-side ones need no GPU. */
enum { GEM_DT_F32 = 0, GEM_DT_F64 = 1 };
enum { GEM_PICKLE_UNSUPPORTED = 2 };     /* return code: a well-formed call on a file outside the subset -- un-pickle it the ordinary way */

typedef struct gem_pickle_array {
    int64_t offset;         /* of the array's raw data, in bytes from the start of the file */
    int64_t nbytes;
    int32_t dtype;          /* GEM_DT_F32 / GEM_DT_F64 (little-endian) */
    int32_t ndim;           /* 0..4 */
    int32_t fortran;        /* 1: the data are in Fortran order (ndarray.flags.f_contiguous and not c_contiguous) */
    int32_t key;            /* index into the `keys` the scan was given */
    int64_t shape[4];       /* unused trailing dimensions are 1 */
} gem_pickle_array;

/* Interprets the pickle in h_image[0, len) (protocols 2-5; the opcodes a dict of lists of ndarrays consists of) WITHOUT constructing
 * or calling anything it names, and reports where the arrays of the dict's entries `keys[0 .. n_keys)` lie: `out` receives the
 * arrays key by key in list order (at most `cap`), counts[k] the number of arrays under keys[k], or -1 when the dict has no such
 * key.  Returns GEM_PICKLE_UNSUPPORTED (text in gem_last_error) for anything else: other opcodes, an entry that is not a list of
 * float32 / float64 ndarrays, protocol-2 arrays (their bytes are stored as text), big-endian data. */
int gem_pickle_scan(const void* h_image, int64_t len, const char* const* keys, int n_keys, gem_pickle_array* out, int64_t cap,
                    int64_t* counts);

/* n equally shaped arrays found by gem_pickle_scan -> h_out [n][shape] float64, C order (np.asarray(list_of_arrays) as at
 * optimizer.py:318-323 for the skeleton / camera lists). */
int gem_pickle_gather_f64(const void* h_image, int64_t len, const gem_pickle_array* arrays, int64_t n, double* h_out);

/* Heat-maps out of a DEVICE image of (part of) the file: d_image[0, image_len) holds file bytes, d_offsets [n] the byte position of
 * every frame's raw data in it (any alignment); dtype / fortran as gem_pickle_scan reported them (all frames alike).
 * d_out [n, heat_h, heat_w, n_joints] f32 = what `torch.from_numpy(np.asarray(heatmap_list)).float()` holds (optimizer.py:324,248):
 * the Fortran order undone, float64 rounded to nearest even.  d_image must be 4-byte aligned and readable up to image_len rounded
 * UP to a multiple of 4; d_out 16-byte aligned; n <= 65535. */
int gem_heat_gather(const void* d_image, int64_t image_len, const int64_t* d_offsets, int64_t n, int heat_h, int heat_w,
                    int n_joints, int dtype, int fortran, float* d_out, void* stream);

/* One chunk file as an object: gem_chunk_open opens and maps `path`, scans it for `keys` (gem_pickle_scan) and keeps the table.
 * gem_chunk_count: arrays under keys[key] (-1: no such key); gem_chunk_bytes: size of the file.
 * gem_chunk_info: info[8] = { count, ndim, dtype, fortran, shape[0..3] } of the arrays under keys[key]; ndim = -1 when they are not
 * all of one shape, type and order.  gem_chunk_offsets: the byte offset of every array's raw data in the file (h_out [count]).
 * gem_chunk_gather_f64: gem_pickle_gather_f64 on the key's arrays (n_out = capacity of h_out in doubles). */
typedef struct gem_chunk gem_chunk;
int     gem_chunk_open(const char* path, const char* const* keys, int n_keys, gem_chunk** out);
void    gem_chunk_close(gem_chunk* c);
int64_t gem_chunk_bytes(const gem_chunk* c);
int64_t gem_chunk_count(const gem_chunk* c, int key);
int     gem_chunk_info(const gem_chunk* c, int key, int64_t* info);
int     gem_chunk_offsets(const gem_chunk* c, int key, int64_t* h_out, int64_t cap);
int     gem_chunk_gather_f64(const gem_chunk* c, int key, double* h_out, int64_t n_out);

/* A file on its way to the device: `path` is read (pread, `slice_bytes` at a time) into the caller's PINNED buffer h_pinned and sent
 * on to d_image slice by slice (hipMemcpyAsync on `stream` of `device`: the next slice is read while the last one crosses PCIe), so
 * that d_image[0, *file_bytes) is an image of the file once the stream has passed the call's work -- what gem_heat_gather reads, with
 * the offsets gem_chunk_offsets reports.  Both buffers must hold buffer_bytes >= file size + 8; h_pinned must stay untouched until the
 * stream has passed.  Nothing synchronises; needs no scan of the file, so it can run beside gem_chunk_open on another thread.
 * Calls on different files may run concurrently from different threads (one stream and one pair of buffers each). */
int gem_file_stage(const char* path, int device, void* h_pinned, void* d_image, int64_t buffer_bytes, int64_t slice_bytes,
                   int64_t* file_bytes, void* stream);

/* ---- recordings as the pose network writes them: one `heatmap` .mat and one `depth` .mat per frame ----
 * What MakeDataForOptimization/process_test_data.py:52-68 reads with scipy.io.loadmat, frame by frame.  The host-side calls need no
 * GPU and no gem_handle. */
enum { GEM_MAT_UNSUPPORTED = 2, GEM_MAT_NOT_FOUND = 3 };  /* return codes: outside the subset -- use scipy.io.loadmat; no such variable */
enum { GEM_MAT_HEAT_F64 = 1, GEM_MAT_DEPTH_F32 = 2 };     /* bits of gem_mat_frames' per-frame `kinds` */

typedef struct gem_mat_array {
    int64_t offset;         /* out: of the real part's raw data in the image (compressed = 1: of the zlib stream) */
    int64_t nbytes;         /* out: its length = product of dims * item size (compressed = 1: of the zlib stream) */
    int64_t next;           /* out: where the element after the reported one starts */
    int64_t start;          /* IN:  where to resume (0: at the first element) */
    int32_t bare;           /* IN:  1 = the image is a run of data elements without the 128-byte file header (an inflated element) */
    int32_t compressed;     /* out: 1 = an miCOMPRESSED element was met before the variable was found */
    int32_t mat_class;      /* out: 6 = mxDOUBLE_CLASS, 7 = mxSINGLE_CLASS */
    int32_t storage;        /* out: 7 = miSINGLE, 9 = miDOUBLE */
    int32_t ndim;           /* out: 1..4 */
    int32_t reserved;
    int64_t dims[4];        /* out: unused trailing dimensions are 1; the data are column-major */
} gem_mat_array;

/* Interprets the Level-5 MAT file in h_image[0, len) and LOCATES the numeric array called `name`; copies nothing.  Accepted:
 * little-endian files of version 0x0100; class single stored as miSINGLE, class double stored as miDOUBLE; small data elements;
 * other variables in front (of several variables of that name the last one is reported, as loadmat's dict keeps it).  When an
 * miCOMPRESSED element is met first, it is reported instead (compressed = 1, offset / nbytes of its zlib stream): the caller
 * inflates it, scans the result with bare = 1 and, on GEM_MAT_NOT_FOUND, resumes in the file with start = next.
 * GEM_MAT_UNSUPPORTED, always with a reason in gem_last_error: big-endian, v4 and v7.3 (HDF5) files, complex, sparse, logical,
 * character, cell, struct and object arrays, integer classes, a double array stored in a narrower type (loadmat returns that one in
 * its storage type), more than four dimensions, and any length or offset that does not fit its container. */
int gem_mat_scan(const void* h_image, int64_t len, const char* name, gem_mat_array* out);

/* sizes[i] = size of paths[i] in bytes (one stat each; fails on the first missing file). */
int gem_files_sizes(const char* const* paths, int64_t n, int64_t* sizes);

/* n files into one block of host memory (pinned, for the copy that follows): paths[i] is read to h_block + at[i] (sizes[i] bytes, as
 * gem_files_sizes reported them) and scanned for `name` there: out[i] as gem_mat_scan fills it (offsets relative to the file's own
 * start), rc_out[i] its return code.  Returns non-zero only when a file cannot be read.  Holds no lock: call it from several threads
 * on disjoint ranges of one block. */
int gem_mat_read(const char* const* paths, int64_t n, const int64_t* at, const int64_t* sizes, const char* name, void* h_block,
                 int64_t block_bytes, gem_mat_array* out, int32_t* rc_out);

/* ONE launch: the device image d_image[0, image_len) of such a block -> d_heat [n,heat_h,heat_w,n_joints] f32, bit for bit
 * `torch.from_numpy(loadmat(f)['heatmap']).float()`, and d_depth [n,n_joints] f64 = `loadmat(f)['depth'][0]`.  d_heat_offsets /
 * d_depth_offsets [n]: byte position of every frame's payloads in the image (any alignment; bytes outside the image read as zero);
 * d_kinds [n]: GEM_MAT_HEAT_F64 when the frame's heat-map is stored as double (rounded to nearest even), GEM_MAT_DEPTH_F32 when its
 * depths are stored as single (widened exactly).  d_depth_offsets and d_depth both NULL: a recording without depth files, the
 * heat-maps alone.  Alignment requirements as gem_heat_gather. */
int gem_mat_frames(const void* d_image, int64_t image_len, const int64_t* d_heat_offsets, const int64_t* d_depth_offsets,
                   const int32_t* d_kinds, int64_t n, int heat_h, int heat_w, int n_joints, float* d_heat, double* d_depth, void* stream);

/* process_test_data.py:70-79 for all frames of a batch of chunks: d_est_global [n,J,3] = R_f . d_est_local[f] + t_f with
 * d_cams [n,4,4] (row-major camera-to-world, the SCALED trajectory), float64, no fused multiply-adds; d_frame_error [n] (may be
 * NULL) = mean_j |d_gt - d_est_global| per frame, the terms of main()'s "initial mpjpe" (:160-165). */
int gem_prepare_global(const double* d_est_local, const double* d_cams, const double* d_gt, int64_t n_frames, int n_joints,
                       double* d_est_global, double* d_frame_error, void* stream);

/* ---- Skeleton meshes as PLY files: what the reference's --save writes with open3d, frame by frame ----
 * One file per frame: 15 spheres (radius 0.02 m, 762 vertices, 1520 triangles) on the joints, then 15 cylinders (radius 0.005 m, 102
 * vertices, 200 triangles) along Skeleton.lines -- binary little-endian PLY as open3d's writer lays it out: a text header, 12 960
 * vertex records of 27 bytes (3 x float64 position + 3 x uint8 colour, no padding), 25 800 face records of 13 bytes (uint8 3 + 3 x
 * uint32).  Header and face block are the same for every frame; only the vertex block is made on the device.
 * gem_skeleton_mesh_layout: out[6] = vertices, triangles, header bytes, vertex-block bytes, face-block bytes, file bytes.
 * gem_skeleton_mesh_constant: fills h_header (header bytes) and h_faces (face-block bytes).  Both need no GPU. */
int gem_skeleton_mesh_layout(int64_t* out);
int gem_skeleton_mesh_constant(void* h_header, void* h_faces);

/* The similarity of calculate_errors.global_align_skeleton_seq: Umeyama (with the reflection fix) of d_src [n_points,3] onto d_dst
 * [n_points,3], float64 -> d_crt [13] = c, R (row-major), t with dst ~ c * (src . R) + t for row vectors.  One workgroup, sums in a
 * fixed order, no floating-point atomics: the same bits on every call. */
int gem_sequence_align(const double* d_src, const double* d_dst, int64_t n_points, double* d_crt, void* stream);

/* The vertex blocks of n_frames meshes: d_seq [n_frames,15,3] float64; d_crt [13] from gem_sequence_align (every joint p becomes
 * c * (p . R) + t first) or NULL; frame f's block is written at d_vertex_blocks + f * frame_stride_bytes.  The stride must be at
 * least the block (349 920 bytes) and a multiple of 16, the base 16-byte aligned: anything else is refused before the launch.  A
 * bone along -z (1 + b_z <= 2^-40) is turned by diag(1,-1,-1), a bone of length zero is not turned (the reference gives NaN for
 * both); a NaN joint gives NaN vertices in its sphere and its bones only.  Works on the current device. */
int gem_skeleton_mesh(const double* d_seq, int64_t n_frames, const double* d_crt, void* d_vertex_blocks, int64_t frame_stride_bytes,
                      void* stream);

/* ---- Skeleton sequences as PNG frames: `render=DIR` / `--render DIR` ----
 * A scene is a list of capsules -- all points within r of a segment [a, b] -- each with one colour 0x00BBGGRR.  An image draws a
 * contiguous range of the list through one orthographic view: pixel (px, py) looks along `forward` through
 * centre + u right + v down with u = (px + 0.5 - W/2) s, v = (py + 0.5 - H/2) s, s = 2 half_width / W; one sample per pixel; the
 * nearest entry into a capsule wins (the lower index on equal depth), shaded 0.3 + 0.7 max(0, -n . forward); background white.
 * All arithmetic float64. */
typedef struct gem_view {
    double right[3], down[3], forward[3];       /* orthonormal (checked to 1e-9) */
    double centre[3];
    double half_width;                          /* metres from the image's centre to its left and right edge */
    int32_t width, height;                      /* pixels; width at most 1024 */
} gem_view;

/* out[3] = bytes of one scanline (1 + 3 width: PNG filter byte 0, then RGB), bytes of one image (height scanlines: what the file's
 * IDAT holds before deflate), and the distance of two images in gem_render_capsules' output (the image's bytes rounded up to 16).
 * Needs no GPU. */
int gem_render_layout(int width, int height, int64_t* out);

/* The 30 capsules of every frame of d_seq [n_frames,15,3] float64, moved by d_crt [13] (gem_sequence_align) first unless NULL: the
 * 15 joints (a == b, r = 0.02 m, rgb_joint), then the 15 lines of Skeleton.lines (r = 0.005 m, rgb_line), in the meshes' order.
 * d_geom [n_frames*30,7] float64 = a, b, r in world coordinates; d_rgb [n_frames*30] uint32. */
int gem_skeleton_capsules(const double* d_seq, int64_t n_frames, const double* d_crt, uint32_t rgb_joint, uint32_t rgb_line,
                          double* d_geom, uint32_t* d_rgb, void* stream);

/* n_images images of view->width x view->height pixels: image i draws the capsules d_first[i] .. d_first[i+1] (int32, device) of
 * d_geom [n_capsules,7] / d_rgb [n_capsules] and is written at d_out + i * image_stride_bytes as its PNG scanline stream.
 * d_ids [n_images,H,W] int32 (may be NULL): the winning capsule's index within the image's range, -1 where nothing is hit;
 * d_depth [n_images,H,W] float64 (may be NULL): the hit's t along `forward` from the plane through the centre, +inf where nothing
 * is hit.  A capsule with a NaN is never hit.  Refused before any launch, with the reason in gem_last_error: d_out not 16-byte
 * aligned; a stride below the image's bytes or no multiple of 16; d_first not ascending or leaving [0, n_capsules] (the call reads
 * d_first back for this: it waits for the stream); a view that is not orthonormal; width or height below 1, width above 1024.
 * One workgroup per band of 16 rows; no floating-point atomics: the same bytes on every call.  Works on the current device. */
int gem_render_capsules(const double* d_geom, const uint32_t* d_rgb, int64_t n_capsules, const int32_t* d_first, int n_images,
                        const gem_view* view, void* d_out, int64_t image_stride_bytes, int32_t* d_ids, double* d_depth, void* stream);

/* ---- The camera's view: `render_camera=DIR` / `--render_camera DIR` ----
 * The fisheye image points of a sequence, and images of the 1024 x 1024 crop of the 1280 x 1024 fisheye image that the heat-maps
 * cover (columns 128 .. 1152): the heat-maps as a tinted background, the reprojected skeletons flat on top. */

/* d_seq [n_frames,J,3] float64 -> d_uv [n_frames,J,2] float32, pixels of the 1280 x 1024 image.  d_crt [13] (gem_sequence_align) or
 * NULL: every joint p becomes c * (p . R) + t first, exactly as in gem_skeleton_capsules.  d_cams [n_frames,4,4] float64, rigid
 * camera-to-world, or NULL when the points are in the camera's frame already: X_cam = R^T (X - t) in float64, rounded once to
 * float32, then the fp32 projection of the optimiser's reprojection term with the handle's polynomial, cx and cy -- the arithmetic
 * of gem_sequence_quality's column 0.  A joint on the optical axis gives a pair that is not finite, and no error. */
int gem_project_sequence(gem_handle* h, const double* d_seq, const double* d_crt, const double* d_cams, int64_t n_frames, float* d_uv,
                         void* stream);

typedef struct gem_camera_view {
    int32_t  size;          /* N: N x N pixels over the 1024 x 1024 crop the heat-maps cover; 1 .. 1024 */
    uint32_t joint_mask;    /* bit j set: heat-map j takes part in the background */
    uint32_t rgb_heat;      /* 0x00BBGGRR */
    uint32_t reserved;
    double   joint_radius, line_radius;   /* in pixels of the 1280 x 1024 image */
} gem_camera_view;

/* n_images images of N x N pixels, image i written at d_out + i * image_stride_bytes as its PNG scanline stream, in the layout of
 * gem_render_layout(N, N).  d_heat [n_images,H,W,J] float32 (NULL: a white background, response 0); d_uv [n_sequences,n_images,J,2]
 * float32 (gem_project_sequence); d_rgb [n_sequences] 0x00BBGGRR; d_ids [n_images,N,N] int32 and d_response [n_images,N,N] float32
 * may be NULL.  Pixel (px, py) stands at u = 128 + (px + 0.5) (1024 / N), v = (py + 0.5) (1024 / N), in fp32 for the background and
 * in float64 for the overlay (the same numbers when N is a power of two).
 *   Background: m = the largest, over the joints of joint_mask, of the bilinear heat-map sample at (u, v) (zeros outside, the fp32
 *   arithmetic of the reprojection term), clamped to [0, 1] -- d_response receives it; every colour byte is
 *   floor(255 + (c - 255) m + 0.5) in float64 with c that byte of rgb_heat.
 *   Overlay: sequence s has 30 primitives in gem_skeleton_capsules' order: the 15 joints as discs of joint_radius about their
 *   (u, v), then the 15 lines as all points within line_radius of the straight segment between their joints' (u, v).  A primitive
 *   covers a pixel whose centre lies within its radius (<=, float64 on the widened fp32 points).  Of the covering primitives the
 *   higher s wins, within a sequence a joint beats a line, within a class the lower index; the pixel takes d_rgb[s] flat and d_ids
 *   receives s * 30 + c (-1: none).  A primitive with a coordinate that is not finite is never drawn.
 * Refused before any launch, with the reason in gem_last_error: a handle whose n_joints is not 15; size outside 1 .. 1024;
 * joint_mask bits at or above 15; a radius that is negative or not finite; n_sequences outside 0 .. 8; n_images outside 0 .. 65535;
 * d_out not 16-byte aligned, a stride below the image's bytes or no multiple of 16; NULL where data are needed.  n_images == 0
 * returns 0.  One workgroup per band of 16 rows; no atomics: the same bytes on every call. */
int gem_render_camera(gem_handle* h, const float* d_heat, const float* d_uv, const uint32_t* d_rgb, int n_sequences, int n_images,
                      const gem_camera_view* view, void* d_out, int64_t image_stride_bytes, int32_t* d_ids, float* d_response,
                      void* stream);

/* Timing hook for bench.py's roofline: average device time (ms) of the launches of the dominant
 * kernel family since the last reset, measured with HIP events on the launch stream.
 * family: 0 = decoder_input GEMMs (forward + backward-data), 1 = fused tail / energy kernel, 2 = L-BFGS advance,
 *         3 = input lifting (`flops` then returns algorithmic bytes).
 * `gem_profile_enable(h, 1)` turns event recording on (off by default: events cost launches). */
int gem_profile_enable(gem_handle* h, int on);
int gem_profile_read(gem_handle* h, int family, double* total_ms, int64_t* n_launches, double* flops);
/* Names of the kernels launched for `family` while event recording was on, since the last call (a "; "-separated list of
 * demangled names without parameter lists, i.e. as rocprofv3 --kernel-trace --stats prints them), written to buf (truncated to
 * buf_len - 1 characters).  bench.py labels its roofline objects with this, so that the label is the kernel that actually ran. */
int gem_profile_kernels(gem_handle* h, int family, char* buf, int buf_len);

/* ---- VAE training on the device: the loop body of networks/train.py:65-108 ----
 * One gem_trainer_step = model.train() forward (BatchNorm1d batch statistics; running statistics updated with `bn_momentum`,
 * unbiased variance), ConvVAE.loss_function (networks/models/SeqConvVAE.py:191-219: F.mse_loss(recons, input) + kld_weight *
 * mean_b(-0.5 * sum_d(1 + logvar - mu^2 - exp(logvar))), `kld_weight` being train.py:89's M_N), loss.backward() and -- when
 * `update` is non-zero -- one torch.optim.Adam step (train.py:60: lr, betas, eps, L2 weight_decay added to the gradient).
 * update = 1 leaves every gradient in the gradient arena (p.grad after the step).  update = 2 is the training loop's mode: the two
 * linear layers (fc_mu | fc_var, decoder_input: 97 % of the parameters) form their weight gradient INSIDE their Adam step and do
 * not write it to the arena (afterwards gem_trainer_download(what = 1) returns NaN in those two ranges, and gem_trainer_arena(what = 1)
 * / gem_trainer_apply fail until a step with update = 0 or 1 has filled the arena again); parameters, moments, statistics and losses are the same
 * up to summation order (at batches of at most 64 windows the same pass over the weights also forms the layers' backward-data
 * products; what Adam's eps makes of last-bit differences: tests/test_hip_train.py::test_training_loop_mode_steps_like_the_default_mode).
 *
 * Parameters, gradients and both Adam moments are fp32 arenas of `n_params` floats in the packed device layout; running
 * statistics an arena of `n_stats` floats.  Arena order (every width padded to a multiple of 64, padding zero):
 *   encoder block i:  W [3][N][K] (Conv1d weight[n][k][tap] at [tap][n][k]), bias [N], BN gamma [N], BN beta [N]
 *   fc_mu | fc_var:   W [2*Dp][T*topp] (row d = fc_mu d, row Dp + d = fc_var d; column t*topp + c = flattened feature c*T + t),
 *                     bias [2*Dp]
 *   decoder_input:    W [T*topp][Dp] (row t*topp + c = output feature c*T + t), bias [T*topp]
 *   decoder block i:  W [3][N][K] = the equivalent Conv1d taps of ConvTranspose1d(k=3,s=1,p=1): weight[k][n][2-tap] at
 *                     [tap][n][k]; bias, gamma, beta (the final Conv1d has no BatchNorm: W, bias only)
 *   statistics:       per BatchNorm layer in the same order: running_mean [N], running_var [N]
 * globalegomocap_amd/vae_train.py converts between this and the checkpoint schema of the reference.
 *
 *   d_pose    [B,T,3J] f32 device   the batch (train.py:82 after the float() cast)
 *   d_eps     [B,D]    f32 device   the reparameterisation noise (torch.randn_like at SeqConvVAE.py:167)
 *   d_losses  [3]      f64 device   loss, Reconstruction_Loss, KLD (may be NULL)
 * 2 <= B <= cfg.max_windows; update must be 0, 1 or 2.  Everything is enqueued on `stream`; nothing synchronises. */
typedef struct gem_trainer gem_trainer;
typedef struct gem_train_opts {
    double  lr, beta1, beta2, eps, weight_decay;   /* torch.optim.Adam: 1e-3, 0.9, 0.999, 1e-8, train.py's --weight_decay */
    double  kld_weight;                            /* M_N = kl_weight * batch / len(dataset) (train.py:89) */
    double  bn_momentum;                           /* 0.1 */
    int32_t recon_sum;                             /* 0: F.mse_loss mean (the reference); 1: summed squared error */
    int32_t reserved;
} gem_train_opts;
int  gem_trainer_create(const gem_config* cfg, gem_trainer** out);
void gem_trainer_destroy(gem_trainer* t);
int  gem_trainer_sizes(gem_trainer* t, int64_t* n_params, int64_t* n_stats);
/* what: 0 parameters (resets the Adam step count), 1 gradients (download only), 2 running statistics, 3 / 4 Adam moments */
int  gem_trainer_upload(gem_trainer* t, int what, const float* h_src, int64_t n);
int  gem_trainer_download(gem_trainer* t, int what, float* h_dst, int64_t n);
int  gem_trainer_set_step(gem_trainer* t, int64_t step);
int  gem_trainer_step(gem_trainer* t, int B, const float* d_pose, const float* d_eps, const gem_train_opts* opts, int update,
                      double* d_losses, void* stream);
/* Data-parallel training (one process per GPU, every rank its own batch; the reference trains on one device, networks/train.py:58):
 * gem_trainer_step(..., update = 0, ...) leaves the rank's gradients in the gradient arena; the caller all-reduces that ONE flat
 * buffer (gem_trainer_arena returns the device address of arena `what` and its length in floats; RCCL through torch.distributed
 * in vae_train.py) and applies the Adam step with gem_trainer_apply, which scales the gradients by grad_scale (1 / world size)
 * on the fly.  BatchNorm statistics stay per rank, as under torch's DistributedDataParallel without SyncBatchNorm. */
int  gem_trainer_arena(gem_trainer* t, int what, void** d_ptr, int64_t* n);
int  gem_trainer_apply(gem_trainer* t, const gem_train_opts* opts, double grad_scale, void* stream);
/* Two read-only views for tests and tools.
 * gem_trainer_route: the decisions a step of B windows takes -- the very record gem_trainer_step fills at its top and consults
 * -- as int32 (cap >= 12 + 2 * (number of conv layers); nothing is launched):
 *   [0]  BatchNorm forward: 0 = sums from the producing conv's epilogue, 1 = register-resident kernel, 2 = row-block kernels
 *   [1]  BatchNorm backward where no dz arrives from a conv's epilogue: 1 = register-resident, 2 = row-block kernels
 *   [2]  update = 2: the encoder's last block gets dz (and its sums) from the fc layer's backward
 *   [3], [4]  update = 2: strip length (n tiles per workgroup) of the fused backward of decoder_input, of fc; 0 = separate kernels
 *   [5], [6]  the separate backward-data product of decoder_input, of fc: slabs summed behind it; 1 = none, the product writes dX
 *        itself (batch a multiple of 64); -1 = one slab copied out of the slab buffer (any other batch)
 *   [7], [8]  weight-gradient slabs of the conv layers, of the linear layers (update < 2)
 *   [9], [10] conv layers of the encoder, of the decoder;  [11] compute units the decisions were made for
 *   [12 + 2 l], [13 + 2 l]  conv layer l (encoder, then decoder): waves per workgroup of its forward product, of its backward-data
 *        product (0: the first encoder conv has none)
 * gem_trainer_layer_output: which = 0 encoder / 1 decoder, block `index`: the device address of the block's output [rows, *ld]
 * (after LeakyReLU; the decoder's last index is the final conv = the reconstructed pose), valid after a step until the next one. */
int  gem_trainer_route(gem_trainer* t, int B, int32_t* out, int cap);
int  gem_trainer_layer_output(gem_trainer* t, int which, int index, void** d_ptr, int* ld);

/* ---- Training windows of the motion VAEs cut on the device ----
 * gem_motion_cameras: d_loc [n,3], d_quat [n,4] (x, y, z, w; any non-zero norm) float64 -> d_cam34 [n,3,4] float64 = [R | loc] with
 * R = scipy's Rotation.from_quat(quat).as_matrix() (normalised first; utils/utils.py:33-42 of the reference).
 * gem_motion_windows: S sequences packed in one frame arena: d_pose [F,15,3] float64; d_cam34 [F,3,4] from gem_motion_cameras for
 * global windows or NULL for local (camera-frame) ones; d_seq_frame0 [S] the first arena frame of every sequence, d_seq_window0
 * [S+1] the prefix of the windows per sequence (window0[S] = n_windows), d_seq_timer [S] its frame-rate timer.  For every id of
 * d_ids [B] (int64, device), window w = id - window0[s] of sequence s starts at arena frame frame0[s] + w * interval (interval 0:
 * w * frame_num * windows_size * timer[s], the reference's windows without sliding) and
 * d_out [B,T,45] float32 receives
 *   global (T = frame_num):              inv(C_start) . C_f . [x; 1] for f = start + t * windows_size * timer (float64, rounded once)
 *   local  (T = frame_num * windows_size): the pose of frame f = start + t * timer
 * An id outside [0, n_windows) gives NaN rows.  The host builds the prefix arrays; the kernel trusts them.  Nothing synchronises. */
int gem_motion_cameras(const double* d_loc, const double* d_quat, int64_t n_frames, double* d_cam34, void* stream);
int gem_motion_windows(const double* d_pose, const double* d_cam34, const int64_t* d_seq_frame0, const int64_t* d_seq_window0,
                       const int32_t* d_seq_timer, int n_seq, int64_t interval, int frame_num, int windows_size,
                       const int64_t* d_ids, int64_t B, float* d_out, void* stream);

/* ---- Looking at a trained motion VAE ----
 * Neither function takes a handle: the batch is not limited by a handle's max_windows.  Caller-owned device pointers, nothing
 * synchronises, sums are f64 in a fixed order (two calls give the same bits), no atomics.
 *
 * gem_latent_paths: for each of n_pairs pairs, n_steps >= 2 latent points from d_za [n_pairs,D] to d_zb [n_pairs,D] into
 * d_out [n_pairs,n_steps,D], all f32.  Step 0 is za and step n_steps-1 is zb, copied.  Interior step i, t = i / (n_steps-1):
 *   GEM_PATH_LINEAR     numpy's float32 arithmetic of `first_z + (i / (S - 1.)) * (second_z - first_z)` (the reference's
 *                       networks/interpolant.py:126): t rounded to f32, then the difference, the product and the sum rounded once each
 *   GEM_PATH_SPHERICAL  w = acos(clamp(<a,b> / (|a| |b|), -1, 1)) from f64 sums; (sin((1-t) w) a + sin(t w) b) / sin w in f64,
 *                       rounded once to f32.  A pair with |a| = 0, |b| = 0 or sin w < 1e-6 takes the linear formula.
 *
 * gem_latent_report: d_mu, d_logvar [n_windows,D] f32 (what the encoder returns); d_x, d_rec [n_windows,n_coords] f32 with
 * n_coords = frames * n_joints * 3 (a window and its reconstruction), or NULL.  d_rows [n_windows][5] f64 per window:
 *   0 mu_error         sum_d mu^2                                  (networks/get_latent.py:57)
 *   1 std_error        sum_d (exp(logvar / 2) - 1)^2               (get_latent.py:58)
 *   2 kld              -1/2 sum_d (1 + logvar - mu^2 - exp(logvar))  (the summand of SeqConvVAE.loss_function's batch mean)
 *   3 mpjpe            mean over frames and joints of |rec - x|     (networks/train.py:127-129); NaN without d_x / d_rec
 *   4 max_joint_error  the largest of those distances; NaN without d_x / d_rec
 * f64 arithmetic on the f32 inputs.  d_cols [3][D] f64 (or NULL) are accumulators the caller zeroes once; every call adds the
 * batch's sum_n mu_d, sum_n mu_d^2 and sum_n exp(logvar_d), summed in an order that depends on a row's index in the batch only.
 * d_count (or NULL): *d_count += n_windows. */
enum { GEM_PATH_LINEAR = 0, GEM_PATH_SPHERICAL = 1 };
int gem_latent_paths(const float* d_za, const float* d_zb, int64_t n_pairs, int latent_dim, int n_steps, int mode, float* d_out,
                     void* stream);
int gem_latent_report(const float* d_mu, const float* d_logvar, const float* d_x, const float* d_rec, int64_t n_windows, int latent_dim,
                      int n_coords, int n_joints, double* d_rows, double* d_cols, int64_t* d_count, void* stream);

/* ---- Live mode: a stream optimised window by window as its frames arrive ----
 * Frames are numbered n = 0, 1, 2, ... in arrival order; window w covers the frames [8w, 8w + 10) (seq_len 10, overlap 2: the
 * handle must have been made with seq_len = GEM_LIVE_WINDOW).  All memory is the caller's: the frame rings of GEM_LIVE_RING frames
 * (frame n lives in slot n mod GEM_LIVE_RING) and one block of GEM_LIVE_STATE_DOUBLES doubles that the caller zeroes once:
 *     0..15   sum over the pushed frames of every joint's bone length (the f32 length, added in frame order)
 *     16      the number of frames in those sums      17  frames pushed      18  windows emitted      19  frames emitted
 *     20      t_prev of the filter                     21  1 once the filter has seen a frame
 *     22..23  the timestamps of the two held frames    24  1 while two frames are held
 *     32..79  x_prev [48]     80..127  dx_prev [48]     128..223  held optimised frames [2][48]     224..319  held estimated frames [2][48]
 * The four launch functions allocate nothing, copy nothing to the host and never synchronise; the host passes the stream position
 * (first_frame, n_pushed, window) because it knows it, and the functions check it against the ring before they launch.
 *
 * gem_live_push: k <= GEM_LIVE_PUSH_MAX frames (d_heat [k,H,W,J] f32, d_pose [k,J,3] f32 the lifted local skeleton, d_cams [k,4,4] f64,
 * d_times [k] f64) become the frames first_frame .. first_frame + k - 1 of the rings, and their bone lengths are added to the sums.
 * oldest_needed: the oldest frame a window still to come reads; a push that would overwrite it is refused.
 *
 * gem_live_window: the frames of window `window` from the rings into the buffers of fixed address that the optimiser's call reads
 * (d_win_pose [10,J,3] f32, d_win_cams [10,4,4] f64, d_win_heat [10,H,W,J] f32), and d_mean_bone [J] f32: d_bone_fixed when given, else
 * the running mean (f64 sum / count, rounded once).  n_pushed: frames pushed so far; the window must be complete and still in the rings.
 *
 * gem_live_emit: d_global [10,J,3] f64 is the window's result (gem_optimize_windows with B = 1 on the window buffers).  Writes
 * d_out [2][8][J*3] f64: the 8 frames [8w, 8w + 8) of the optimised sequence -- its first two (w > 0) the held frames plus the
 * window's, halved -- and of the estimated one, cams . pose in f64; holds the window's last two frames.  final != 0: writes the two
 * held frames to d_out [2][0..1] instead and releases them (d_global, d_win_pose, d_win_cams are not read).  h_one_euro (host, 3
 * doubles: min_cutoff, beta, d_cutoff; or NULL: off): the optimised frames pass the One-Euro filter in frame order, per coordinate,
 * with the frames' own timestamps; its state lives in the state block.
 *
 * gem_one_euro: the same filter over whole sequences.  d_seq [n_chunks*frames_per_chunk, n_coords] f64, d_times [n_chunks*frames_per_chunk]
 * f64 -> d_out of d_seq's shape; every chunk starts with fresh state (its first frame passes through).  The arithmetic is the
 * reference's utils/one_euro_filter.py in f64, operation by operation:
 *     t_e = t - t_prev;  a_d = r / (r + 1) with r = 2 pi d_cutoff t_e;  dx = (x - x_prev) / t_e;  dx_hat = a_d dx + (1 - a_d) dx_prev;
 *     cutoff = min_cutoff + beta |dx_hat|;  a likewise from cutoff;  x_hat = a x + (1 - a) x_prev.
 * Timestamps must increase strictly (the caller checks: the device never reports). */
#define GEM_LIVE_WINDOW 10
#define GEM_LIVE_STRIDE 8
#define GEM_LIVE_RING 32
#define GEM_LIVE_PUSH_MAX 8
#define GEM_LIVE_STATE_DOUBLES 320
typedef struct gem_live_buffers {
    float* ring_pose;      /* [GEM_LIVE_RING,J,3] */
    double* ring_cams;     /* [GEM_LIVE_RING,4,4] */
    double* ring_times;    /* [GEM_LIVE_RING] */
    float* ring_heat;      /* [GEM_LIVE_RING,H,W,J] */
    double* state;         /* [GEM_LIVE_STATE_DOUBLES] */
} gem_live_buffers;
int gem_live_push(gem_handle* h, const gem_live_buffers* b, int64_t first_frame, int k, int64_t oldest_needed, const float* d_heat,
                  const float* d_pose, const double* d_cams, const double* d_times, void* stream);
int gem_live_window(gem_handle* h, const gem_live_buffers* b, int64_t window, int64_t n_pushed, const float* d_bone_fixed,
                    float* d_win_pose, double* d_win_cams, float* d_win_heat, float* d_mean_bone, void* stream);
int gem_live_emit(gem_handle* h, const gem_live_buffers* b, int64_t window, int final, const double* d_global, const float* d_win_pose,
                  const double* d_win_cams, const double* h_one_euro, double* d_out, void* stream);
int gem_one_euro(const double* d_seq, const double* d_times, int n_chunks, int64_t frames_per_chunk, int n_coords, const double* h_params,
                 double* d_out, void* stream);
/* Live mode at a stride below 8 with a zero-look-ahead stream, and the dense merge of recorded windows: their declarations and the
 * layout of their state block are in the header of their own, next to this one. */
#include "gem_live_dense.h"

/* ---- Skeleton sequences as BVH animation: `bvh=DIR` / `--bvh DIR` ----
 * The file's skeleton has 19 nodes on the 15 joints (node: parent, rest direction, joint; Y up, Z forward, +X the character's left):
 *    0 Hips            -   -   midpoint of joints 7 and 11      1 Spine          0   0  (helper, zero offset)       2 Neck  1  +Y  joint 0
 *    3 Right_collar    2   0   (helper)                         7 Left_collar    2   0  (helper)
 *    4 Right_shoulder  3  -X   joint 1                          8 Left_shoulder  7  +X  joint 4
 *    5 Right_elbow     4  -X   joint 2                          9 Left_elbow     8  +X  joint 5
 *    6 Right_wrist     5  -X   joint 3                         10 Left_wrist     9  +X  joint 6
 *   11 Right_hip       0  -X   joint 7                         15 Left_hip       0  +X  joint 11
 *   12 Right_knee     11  -Y   joint 8                         16 Left_knee     15  -Y  joint 12
 *   13 Right_ankle    12  -Y   joint 9                         17 Left_ankle    16  -Y  joint 13
 *   14 Right_foot     13  +Z   joint 10                        18 Left_foot     17  +Z  joint 14
 * A helper sits on its parent.  A frame has 60 channels: Hips' Xposition Yposition Zposition, then Zrotation Xrotation Yrotation of every
 * node in the order above; a node's local rotation is Rz(a) Rx(b) Ry(c), degrees.  In the text every channel is one 16-byte field,
 * "%15.6f" and a space (a newline after the 60th): a frame is 960 bytes.
 * gem_bvh_layout: out[4] = nodes, channels per frame, bytes per field, bytes per frame.
 * gem_bvh_tables: parents [19] (-1: the root), joint_of_node [19] (-1: Hips and the helpers), rest_dirs [19,3].  Both need no GPU. */
int gem_bvh_layout(int64_t* out);
int gem_bvh_tables(int32_t* parents, int32_t* joint_of_node, double* rest_dirs);

/* The rest lengths: d_rest [19] float64 = for every node with a rest direction the mean over the n_frames (>= 1) frames of d_seq
 * [n_frames,15,3] float64 of |pos(node) - pos(parent)|, 0 for the others; every joint is first moved by d_crt [13] (gem_sequence_align:
 * c * (p . R) + t) unless NULL.  One workgroup, sums in a fixed order, no floating-point atomics: the same bits on every call.  Works
 * on the current device. */
int gem_bvh_rest(const double* d_seq, int64_t n_frames, const double* d_crt, double* d_rest, void* stream);

/* The channels: d_channels [n_frames,60] float64 from d_seq and d_crt as above, float64 without fused multiply-adds.  With X_j joint j,
 * P = (X7 + X11) / 2 and unit(v) = v / |v|: the position channels are P * unit_scale.  The root's frame G0 has the columns
 * x = unit(X11 - X7), z = unit(x cross (X0 - P)), y = z cross x; the Neck's is built the same way from unit(X4 - X1) and the Spine's y
 * column.  Every other node with one child that has a rest direction r gets G = G_parent S, S the shortest-arc rotation from r to
 * l = G_parent^T unit(pos(child) - pos(node)): Rodrigues about r cross l by atan2(|r cross l|, r . l).  The wrists and feet inherit
 * their parent's frame (three zeros).  A node's local rotation is G_parent^T G, and from it b = asin(R21), a = atan2(-R01, R11),
 * c = atan2(-R20, R22); where |R21| > 1 - 1e-10: b = +-90, a = atan2(R10, R00), c = 0.
 * Defined corners: |r cross l| < 1e-12 is the identity where r . l >= 0 and else a half turn about unit(r cross X), about
 * unit(r cross Y) where |r_x| >= 0.9; a bone of length zero is the identity; where the root's or the Neck's x or x cross hint is
 * shorter than 1e-12 the node takes its parent's frame (the root: the identity).  A NaN joint gives NaN channels in its frame.
 * d_rest [19] (gem_bvh_rest) is the skeleton the channels are for; it must not be NULL, and no formula reads it: the rotations
 * reproduce directions, the file's OFFSET lines the lengths.  Works on the current device. */
int gem_bvh_channels(const double* d_seq, int64_t n_frames, const double* d_crt, const double* d_rest, double unit_scale,
                     double* d_channels, void* stream);

/* d_values [n_values] float64 -> d_text [n_values * 16] bytes: field i is "%15.6f" of value i as C and Python print it -- rounded to
 * the nearest millionth, ties to even, on the value's exact binary expansion; "-0.000000" for a negative value that rounds to zero --
 * and one separator: a newline after every values_per_line-th value, else a space.  nan, inf and -inf are written as such.  They, and
 * a value that rounds to more than 9999999.999999 in magnitude (its field is filled with asterisks), add one to d_bad[0] and lower
 * d_bad[1] to their line's index i / values_per_line: the caller sets d_bad to {0, -1} beforehand; nothing synchronises or reads
 * back.  d_text must be 16-byte aligned: anything else is refused before the launch.  Works on the current device. */
int gem_format_fields(const double* d_values, int64_t n_values, int64_t values_per_line, void* d_text, int64_t* d_bad, void* stream);

/* ---- Results as one glTF 2.0 binary file: skinned, animated skeletons: `gltf=DIR` / `--gltf DIR` ----
 * The file's skeleton is the BVH route's tree of 19 nodes above; its 15 rotating nodes are the root and every node with a child (all but
 * the wrists and feet).  The mesh is the geometry of gem_skeleton_mesh: 12 960 vertices, 25 800 triangles.
 * gem_gltf_layout: out[40] = nodes (19), rotating nodes (15), vertices, triangles, bytes per vertex (32), bytes of a vertex block
 * (414 720); the 15 rotating nodes in node order; the byte offsets of the 17 arrays of an animation block of n_frames frames --
 * times [F] f32, translation [F,3] f32, one rotation [F,4] f32 (x, y, z, w) per rotating node; every array tightly packed, every start
 * a multiple of 16 --; the block's size; the payload per frame (256 bytes).  Needs no GPU. */
int gem_gltf_layout(int64_t n_frames, int64_t* out);

/* The animation block of d_seq [n_frames,15,3] float64 behind d_crt [13] (or NULL), as in gem_bvh_channels, into d_block (16-byte aligned,
 * the size gem_gltf_layout gives): times[f] = (double)f / fps, translation[f] = the Hips' position P in metres, and per rotating node the
 * local rotation matrix R that gem_bvh_channels turns into angles, with the same defined corners, as a quaternion:
 *   1. Shepperd's method on the largest of (trace, R00, R11, R22), the first on ties: with r = sqrt(1 + trace), w = r / 2 and
 *      (x, y, z) = (R21 - R12, R02 - R20, R10 - R01) / (2 r); with r = sqrt(1 + R00 - R11 - R22), x = r / 2 and
 *      (w, y, z) = (R21 - R12, R01 + R10, R02 + R20) / (2 r); the other two likewise;
 *   2. the canonical sign c: the first non-zero of (w, x, y, z) is positive;
 *   3. the sign from key to key: s[0] = +1, s[f] = -s[f-1] where c[f] . c[f-1] < 0 and else s[f-1] (a dot of 0 or NaN does not flip);
 *      s[f] c[f] is written.
 * float64 without fused multiply-adds; every number is rounded once, to float32; nothing is renormalised.  The bytes are the same on
 * every call.  Every frame with a number that is not finite adds one to d_bad[0] and lowers d_bad[1] to its index: the caller sets
 * d_bad to {0, -1} beforehand.  Three launches on `stream`; no read-back, no synchronisation, no scratch memory.  n_frames < 0, an fps
 * that is not finite and positive, a misaligned block and (with n_frames > 0) null pointers are refused before the launch;
 * n_frames = 0 returns 0.  Works on the current device. */
int gem_gltf_animation(const double* d_seq, int64_t n_frames, const double* d_crt, double fps, void* d_block, int64_t* d_bad, void* stream);

/* The rest-pose mesh of the skeleton with the rest lengths d_rest [19] (gem_bvh_rest): the rest joints are the rest directions times
 * the lengths, Hips at the origin; on them the 15 spheres and the 15 cylinders of gem_skeleton_mesh, same tables, same vertex order.
 * d_vertices (16-byte aligned) takes 12 960 records of 32 bytes: position f32 x 3, normal f32 x 3 (a sphere's and a cylinder ring's
 * radial, a cap centre's + or - the bone), JOINTS_0 u8 x 4, WEIGHTS_0 u8 x 4 (of 255).  A sphere is bound to its joint's node.  A
 * cylinder is bound to the node its bone turns with: the parent of its second joint's node, Hips for the hip line (7, 11).  The torso
 * lines (1, 7) and (4, 11) join two branches: their ring k of 5, counted from the line's SECOND joint as the vertices are, is bound to
 * (the second joint's node, the first joint's node) with the weights (255 - w, w), w = 0, 64, 128, 191, 255, and each cap centre to its
 * own end; a weight of 0 names node 0.  d_bounds [6] = the minimum (x, y, z) and the maximum of the float32 positions written.  One
 * workgroup, the same bytes on every call.  Works on the current device. */
int gem_gltf_rest_mesh(const double* d_rest, void* d_vertices, float* d_bounds, void* stream);

/* ---- Rendered frames as baseline JPEG images and Motion-JPEG chunks: `video=PATH` / `--video DIR` ----
 * The format is fixed: 8-bit YCbCr (JFIF, full range), 4:4:4, one restart segment per MCU row, the Annex K quantisation tables scaled
 * by the IJG quality rule and the Annex K Huffman tables; integer arithmetic throughout, so the bytes are a function of the pixels
 * and the quality alone (6j, "The format").
 * gem_jpeg_header: the 629 bytes in front of the entropy data -- SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, DRI,
 * SOS -- into buf (cap >= 629); returns 629, or -1 with the reason in gem_last_error.  gem_jpeg_bound: the most bytes one image's
 * file can take, 629 + ceil(H / 8) * (2 * ceil(3 * ceil(W / 8) * 1660 / 8) + 2); -1 for a size out of range.  Both need no GPU. */
int gem_jpeg_header(int width, int height, int quality, void* buf, int64_t cap);
int64_t gem_jpeg_bound(int width, int height);

/* d_scan: n_images images as gem_render_capsules / gem_render_camera write them, `height` rows of 1 + 3 * width bytes each (byte 0 of
 * a row, the PNG filter byte, is ignored), in_stride bytes apart.  Image i's bytes go to d_out[d_offsets[i] .. d_offsets[i+1]):
 * with avi_chunks = 0 a complete JPEG file, with avi_chunks = 1 an AVI chunk -- '00dc', the file's length as uint32, the file, one
 * zero byte behind an odd length -- so that the whole run can be appended to a 'movi' list verbatim.  d_offsets [n_images + 1] int64 is
 * always complete; an image with d_offsets[i+1] > out_capacity is not written at all, and nothing at or behind d_offsets[n_images] or
 * out_capacity is touched.  d_coef, unless NULL (16-byte aligned): int16 [n_images, 3, ceil(H/8), ceil(W/8), 64], the quantised
 * coefficients of Y, Cb, Cr in zigzag order.  1 <= width <= 1024, 1 <= height <= 16384, 1 <= quality <= 100, 0 <= n_images <= 65535,
 * in_stride >= height * (1 + 3 * width): anything else is refused before any launch.  Asynchronous on `stream` (it waits for the
 * device only when the handle's scratch buffer has to grow); two calls give the same bytes. */
int gem_jpeg_encode(gem_handle* h, const void* d_scan, int n_images, int width, int height, int64_t in_stride, int quality, int avi_chunks,
                    void* d_out, int64_t out_capacity, int64_t* d_offsets, int16_t* d_coef, void* stream);

/* ---- Recordings given as 2-D joint detections ----
 * A detection is (u, v, confidence): u, v in pixels of the fisheye image (the 1280 x 1024 image the calibration describes).  It is
 * USABLE when confidence > 0 (NaN is not) and u and v are finite.
 *
 * gem_keypoint_heatmaps: d_kp [n_frames,n_joints,3] f64 -> d_heat [n_frames,heat_h,heat_w,n_joints] f32, the layout every consumer
 * takes.  Joint j of frame f becomes a * exp(-((x - ix)^2 + (y - iy)^2) / (2 sigma^2)) with a = min(max(confidence, 0), 1) and
 * (ix, iy) = ((u - 128) (heat_w - 1) / 1024, v (heat_h - 1) / 1024): the heat-map coordinate at which the reprojection term samples
 * image point (u, v) (optimizer.py:143-147), so that the energy's maximum sits on the detection.  An unusable joint gets an all-zero
 * map.  The value is the float64 expression rounded to float32.  2 <= n_joints <= 16, heat_w >= 2, n_joints (heat_h + heat_w) <= 8192;
 * d_heat needs no more than a float's alignment (16-byte stores wherever the frame's run allows).  Works on the current device. */
int gem_keypoint_heatmaps(const double* d_kp, int64_t n_frames, int n_joints, int heat_h, int heat_w, double sigma, float* d_heat,
                          void* stream);

/* FishEyeCameraCalibrated.camera2world (utils/fisheye/FishEyeCalibrated.py:18-33) at the detection itself, in float64, with the
 * handle's image centre and h_poly_c2w (polynomialC2W, ascending powers): the un-projection of gem_lift_skeleton without its argmax
 * and its 16-pixel grid -- for the same image point the same bits.  d_kp [n_frames,J,3] f64, d_depth [n_frames,J] f64; outputs (each
 * may be NULL, not all) d_out64 / d_out32 [n_frames,J,3] and d_valid [n_frames,J] u8: 1 where the detection was usable.
 * d_prev NULL: frames are independent, an unusable joint is written as zeros (gem_fill_missing replaces it).
 * d_prev [J,3] f64: the frames are taken in order; an unusable joint takes d_prev's value, every usable one updates it, and d_prev
 * holds the last values afterwards -- the causal "hold the last one" of a stream, carried from call to call. */
int gem_lift_keypoints(gem_handle* h, const double* d_kp, const double* d_depth, int64_t n_frames, const double* h_poly_c2w, int n_poly,
                       double* d_prev, double* d_out64, float* d_out32, unsigned char* d_valid, void* stream);

/* In place on d_seq [n_chunks * frames_per_chunk, n_joints, 3] f64 with d_valid [n_chunks * frames_per_chunk, n_joints] u8: per chunk
 * and joint, a frame with valid = 0 between valid frames lo < f < hi becomes seq[lo] + (seq[hi] - seq[lo]) (f - lo) / (hi - lo); in
 * front of the chunk's first valid frame it takes that frame's value, behind the last valid frame that one's.  A joint with no valid
 * frame in a chunk is left untouched (the caller refuses such a recording).  Works on the current device. */
int gem_fill_missing(double* d_seq, const unsigned char* d_valid, int n_chunks, int frames_per_chunk, int n_joints, void* stream);

/* ---- Depths from bone lengths: 2-D detections without a depth network ----
 * A head-mounted camera fixes the joints' depths: the calibration makes every detection a unit ray r_j (camera2world at depth 1, the
 * expressions of gem_lift_keypoints, so that depth * ray there has the bits of d_j r_j here), the wearer's bone lengths L_j are
 * constant, and the neck sits at a nearly fixed distance from the camera.  Per frame, independently, the depths d_0 .. d_14 minimise
 *     sum_bones (|d_j r_j - d_p r_p| - L_j)^2 + w_n (d_0 - neck_depth)^2 + w_m sum_j (d_j - dbar_j)^2,        p = parent of j,
 * by Levenberg-Marquardt: `iters` iterations from d = dbar; a step solves (A + lambda diag A) delta = -g for the normal matrix A, whose
 * graph is the skeleton's tree (eliminated leaf to root without fill, O(15)); the trial point max(d + delta, 0.01) is taken when it
 * lowers the cost, lambda (1e-3 at first) then falls tenfold, else rises tenfold.  A bone of zero extent has a zero Jacobian row.
 * A joint is SOLVED when it and every joint on its path to the neck are USABLE (above).  Only solved joints and the bones between
 * them take part; every other joint keeps dbar_j, and a frame whose neck is unusable keeps every dbar_j.
 * d_kp [n_frames,15,3] f64; h_poly_c2w as gem_lift_keypoints takes it; outputs (each may be NULL, not all) d_depth [n_frames,15] f64,
 * d_solved [n_frames,15] u8, d_rms [n_frames] f64: sqrt of the mean squared bone residual, in metres, at the depths returned, over the
 * bones that took part (0 without any) -- a large value says the detections contradict the skeleton.  The handle must have been
 * created with the 15-joint egocentric tree.  bone[0] = 0, bone[j] >= 0, dbar[j] >= 0.01, neck_depth > 0, w_n >= 0, w_m > 0,
 * 1 <= iters <= 1000, all finite: anything else is refused before any launch.  float64 without fused multiply-adds, every sum in a
 * fixed order: two calls give the same bytes, and a frame's bytes do not depend on the other frames of its call.  Asynchronous on
 * `stream`. */
typedef struct gem_bone_depth_opts {
    double bone[GEM_MAX_JOINTS];      /* L_j, metres; entries 0 and 15 unused (0) */
    double dbar[GEM_MAX_JOINTS];      /* the prior depths and the start */
    double neck_depth, w_n, w_m;
    int32_t iters, reserved;
} gem_bone_depth_opts;
int gem_bone_depths(gem_handle* h, const double* d_kp, int64_t n_frames, const double* h_poly_c2w, int n_poly, const gem_bone_depth_opts* opts,
                    double* d_depth, unsigned char* d_solved, double* d_rms, void* stream);

/* ---- Heat-maps without a depth network: the maps' peaks as sub-pixel detections ----
 * d_heat [n_frames,H,W,J] f32 with the handle's heat_h, heat_w and J (float alignment is enough: 16-byte non-temporal loads when the
 * tensor starts on a 16-byte boundary and a frame is a whole number of 16-byte words, a scalar scan otherwise) -> d_kp [n_frames,J,3]
 * f64, detections (u, v, confidence) in the convention above, and d_arg [n_frames,J] int32, the flat row-major index sy W + sx of the
 * map's integer maximum under numpy's argmax rule (NaN is maximal, the first occurrence wins).  Either output may be NULL, not both.
 * From m = (sx, sy), eight iterations of m <- sum w k x / sum w k over the texels within 4 of (sx, sy) that lie inside the map, with
 * w = max(value, 0) (a NaN texel weighs nothing) and k = exp(-(x - m_x)^2 / 2 tau^2) exp(-(y - m_y)^2 / 2 tau^2), tau = 1.5: a
 * Gaussian-windowed mean shift, whose fixed point is the centre of a Gaussian blob whatever the blob's own width.  Then
 * u = pad_x + m_x upscale W / (W - 1), v = pad_y + m_y upscale H / (H - 1) -- with upscale 16 and pads 128, 0 on a 64 x 64 map the
 * inverse of the map at which the reprojection term samples and gem_keypoint_heatmaps splats -- and confidence = min(peak, 1), the
 * float32 maximum widened.  A joint whose maximum is NaN, not positive or below min_peak is UNUSABLE and written as (0, 0, 0).
 * n_frames >= 0, upscale >= 1, pads >= 0, min_peak finite and >= 0, at most 16 joints, maps of at least 2 x 2: anything else is
 * refused before any launch.  One workgroup per frame; float64 without fused multiply-adds, every sum in a fixed order, no atomics:
 * two calls give the same bytes, and a frame's bytes do not depend on the other frames of its call.  Asynchronous on `stream`. */
int gem_heatmap_peaks(gem_handle* h, const float* d_heat, int64_t n_frames, int upscale, int pad_x, int pad_y, double min_peak,
                      double* d_kp, int32_t* d_arg, void* stream);

/* ---- The SLAM scale of a recording without ground truth, from foot contacts: `--scale auto` ----
 * A monocular SLAM gives the camera's rotation R_t and its translation c_t up to one factor s; the lifted poses x_t are metric.  A
 * foot that stands does not move in the world, so R_t x_t,foot + s c_t is constant over a stance phase.  With q[t,side] =
 * R_t (x[t,ankle] + x[t,foot]) / 2, a[p,side] = q[t+lag,side] - q[t,side] and b[p] = c[t+lag] - c[t] for every t with
 * ids[t+lag] - ids[t] = lag: s_ref = sqrt(sum |a|^2 / (2 sum |b|^2)); the cost C(s) = sum_p min(min_side |a + s b|^2, tau^2) at the
 * 513 candidates s_ref 2^(g/32), g = -256 .. 256; s0 the candidate of the smallest cost (the smallest g of equal ones); four rounds
 * of: every pair takes the side of the smaller residual (a tie: the right foot), is an inlier when that residual is < tau^2, and
 * s <- -sum_inl <a,b> / sum_inl <b,b>.  Everything is float64 without fused multiply-adds and every sum has a fixed order: two calls
 * give the same bits.
 *
 * The report: a gem_scale_report and behind it [n_chunks][3] doubles -- numerator, denominator and scale of the inlier pairs whose
 * first frame lies in the chunk.  `informative`: inliers with s |b| > tau (the camera moved further than a swinging foot is allowed
 * to); stance_right / stance_left: the inliers' shares of the two sides.  status is 0 or why no scale can be given. */
#define GEM_SCALE_CANDIDATES 513
#define GEM_SCALE_TILE 256          /* pairs per workgroup of the cost kernel */
#define GEM_SCALE_REPORT_DOUBLES 16
#define GEM_SCALE_NO_PAIRS 2        /* no two frames lag apart, or the camera never moved (sum |b|^2 = 0) */
#define GEM_SCALE_TOO_FEW 3         /* fewer than min_pairs informative pairs: the wearer did not walk enough */
#define GEM_SCALE_BAD_SCALE 4       /* the fitted scale is not a finite positive number */
typedef struct gem_scale_report {
    double scale, s0, s_ref, g0;                    /* g0: index 0 .. 512 of s0 among the candidates */
    double pairs, inliers, informative;             /* counts */
    double residual_rms, path_length;               /* metres: RMS of the inliers' residuals; scale * sum |b| / lag */
    double stance_right, stance_left;
    double status;                                  /* 0, GEM_SCALE_NO_PAIRS, GEM_SCALE_TOO_FEW or GEM_SCALE_BAD_SCALE */
    double lag, tau, min_pairs, n_chunks;           /* the call's parameters */
} gem_scale_report;

/* Bytes of d_work a call with these sizes needs; -1 with the reason in gem_last_error for sizes out of range.  Needs no GPU. */
int64_t gem_slam_scale_work(int64_t n_frames, int lag, int n_chunks);

/* h_chunks (host) and d_chunks (the same numbers on the device): [n_chunks] device addresses of the chunks' poses, each its own
 * [n,n_joints,3] f64 allocation, then [n_chunks + 1] first rows, rising from 0 to n_frames (a chunk may be empty; the chunks are
 * also the partition of the per-chunk sums).  h_feet [4]: right ankle, right foot, left ankle, left foot.  d_rot [n_frames,3,3],
 * d_trans [n_frames,3]: the unscaled SLAM poses relative to the first frame; d_ids [n_frames] int64 frame ids.  d_work: scratch;
 * d_report [16 + 3 n_chunks]; d_costs [513] or NULL: the candidates' costs.  Arguments are checked before any launch; n_frames <= lag
 * returns GEM_SCALE_NO_PAIRS and launches nothing.  h_report NULL: everything is enqueued on `stream`, the return value says only
 * whether that worked and the verdict is the report's status.  h_report [16 + 3 n_chunks] (host): the report is copied there, the
 * stream is waited for, and a status other than 0 is the return value, its text with the counts in gem_last_error.  Inputs must be
 * finite.  Works on the current device. */
int gem_slam_scale(const int64_t* h_chunks, const int64_t* d_chunks, int n_chunks, int n_joints, const int* h_feet, const double* d_rot,
                   const double* d_trans, const int64_t* d_ids, int64_t n_frames, int lag, double tau, int min_pairs, void* d_work,
                   int64_t work_bytes, double* d_report, double* d_costs, double* h_report, void* stream);

/* ---- A SLAM scale that drifts within a recording, and the camera track in metres: `--scale drift` ----
 * The scale is a piecewise-linear curve over K = max(2, ceil((last_id - first_id) / knot) + 1) knots at frame ids first_id + k knot.
 * A pair whose first row is t lives at ids[t] + lag / 2, in interval k_p = min(floor((that - first_id) / knot), K - 2) with the fraction
 * u_p inside it.  Start: s_k = gem_slam_scale's estimate, whose refusals are this call's.  Four rounds of: with the current curve every
 * pair takes the side of the smaller residual |a + s(tau_p) b|^2 (a tie: the right foot) and is an inlier when that is < tau^2; then
 * minimise sum_inl |a_p + ((1 - u_p) s_k + u_p s_k+1) b_p|^2 + lambda sum_{k=1..K-2} (s_k-1 - 2 s_k + s_k+1)^2 with
 * lambda = stiffness sum_inl <b,b> / (K - 1): a symmetric pentadiagonal system, factored L D L^T in index order.  A pivot that is not
 * positive and finite, or (K > 2) fewer than two intervals whose inliers have sum <b,b> > 0 -- one interval's pairs fix a line, which
 * the penalty would only extrapolate over the whole recording -- keeps the curve of the round before and gives GEM_DRIFT_NOT_SOLVED.
 * The metric track: C_0 = 0, C_i = C_i-1 + s((ids[i-1] + ids[i]) / 2) (c_i - c_i-1), summed as an inclusive scan within blocks of 256
 * rows plus the blocks' totals in order, so the bytes up to row i do not depend on rows behind the block that holds i.  Everything is
 * float64 without fused multiply-adds, every sum has a fixed order, there are no floating-point atomics: two calls give the same bytes. */
#define GEM_DRIFT_MAX_KNOTS 2048
#define GEM_DRIFT_REPORT_DOUBLES 16
#define GEM_DRIFT_NOT_SOLVED 5      /* the recording does not fix the curve */
typedef struct gem_drift_report {
    double status;                                  /* 0, a GEM_SCALE_* refusal of the global estimate, or GEM_DRIFT_NOT_SOLVED */
    double n_knots, knot, stiffness;                /* K and the call's parameters */
    double inliers, informative, residual_rms;      /* under the last curve; informative: s(tau_p) |b| > tau */
    double scale_min, scale_max, scale_mean;        /* over the knots; scale_mean = metric_length / slam_length */
    double metric_length, slam_length;              /* sum of the scaled steps' lengths, metres; sum of the steps' lengths, SLAM units */
    double lam;                                     /* the last round's lambda */
    double first_id;
    double bad_pivot, informed;                     /* index of the first failed pivot or -1; intervals with inlier sum <b,b> > 0 */
} gem_drift_report;

/* Bytes of d_work a call with these sizes needs; -1 with the reason in gem_last_error for sizes out of range.  Needs no GPU. */
int64_t gem_slam_drift_work(int64_t n_frames, int lag, int n_knots);

/* gem_slam_scale's inputs (which see), the first and the last of the frame ids (d_ids must rise), `knot` >= lag + 1 frames between
 * knots and `stiffness` >= 0.  d_scale_report [16 + 3 n_chunks] and d_costs [513] or NULL: gem_slam_scale's outputs, computed once
 * here by its own kernels.  d_knots [K][4]: value, inlier count and inlier sum <b,b> of the interval to the knot's right (0 for the
 * last knot), reserved; d_metric [n_frames,3]; d_report: a gem_drift_report.  All arguments are checked before any launch (more than
 * GEM_DRIFT_MAX_KNOTS knots, knot < lag + 1, a stiffness that is negative or not finite, a null output, d_work too small: return 1
 * with the reason in gem_last_error and nothing written).  A refusal of the global estimate writes the two reports and leaves
 * d_knots and d_metric untouched; GEM_DRIFT_NOT_SOLVED writes d_knots too (the counts tell which intervals held no inliers).
 * h_report NULL: everything is enqueued on `stream` and the verdict is the report's status.  h_report [16] (host): the stream is
 * waited for, h_scale_report, h_knots and h_metric are filled where given (they need h_report), and a status other than 0 is the
 * return value with its text in gem_last_error.  Works on the current device. */
int gem_slam_drift(const int64_t* h_chunks, const int64_t* d_chunks, int n_chunks, int n_joints, const int* h_feet, const double* d_rot,
                   const double* d_trans, const int64_t* d_ids, int64_t n_frames, int64_t first_id, int64_t last_id, int lag, double tau,
                   int min_pairs, int knot, double stiffness, void* d_work, int64_t work_bytes, double* d_scale_report, double* d_costs,
                   double* d_knots, double* d_metric, double* d_report, double* h_scale_report, double* h_knots, double* h_metric,
                   double* h_report, void* stream);

/* ---- The ground plane of a pose sequence from its foot contacts, and the upright frame: `--upright` ----
 * A foot that stands does not move, and the places where the feet stand lie on the floor.  With q[f,side] = (x[f,ankle] + x[f,foot]) / 2
 * (right: joints 9 and 10, left: 13 and 14), foot point (f, side) is a candidate when f + lag < n_frames and
 * |q[f+lag,side] - q[f,side]| < tau_v.  Body up u0 = normalise(sum_f (x[f,0] - (q[f,0] + q[f,1]) / 2)).  The plane n . p = d: centroid
 * and scatter of the candidates, n the singular vector of the scatter's smallest singular value with n . u0 >= 0, d = n . centroid;
 * four rounds of refit on the candidates with |n . p - d| < tau_h; a round with fewer than min_points of them ends the fit.
 * source PLANE: every round had min_points inliers and sqrt(middle eigenvalue of the last scatter) >= min_spread.  BODY_NORMAL: the
 * candidates span no plane: n = u0, d the candidates' height along u0, from their lower median by four rounds of refit within tau_h.
 * BODY: fewer than min_points candidates: n = u0, d the lowest foot point's height.  The foot figures at the final (n, d), over all
 * frames: h = n . q - d; a foot point is in contact when it is a candidate and |h| < tau_h; skate: the mean displacement, without its
 * part along n, between frames f and f + 1 of a foot in contact in both (metres per frame, 0 without such a pair); penetration =
 * max(0, -min h); lift_max = max h.  The upright transform crt = (c = 1, R row-major, t), p -> c * (p . R) + t for row vectors as
 * gem_sequence_align writes it: the columns of R are X (left hip - right hip of frame 0, made level; the most nearly level world
 * axis if that is shorter than 1e-6), Y = n and Z = X x Y ("forward"), det R = +1; t puts frame 0's hip midpoint on x = z = 0 and
 * the plane n . p = d - foot_height on y = 0.  Everything is float64, every sum has a fixed order, there are no floating-point
 * atomics: two calls give the same bytes. */
#define GEM_GROUND_RECORD_DOUBLES 48
#define GEM_GROUND_LDS_FRAMES 1024        /* a longer sequence keeps its foot points in d_work */
#define GEM_GROUND_NO_BODY 2              /* |sum_f (neck - feet)| < 1e-6 n_frames, or a joint that is no number */
#define GEM_GROUND_BAD_SEQUENCE 3         /* the table's row: no or a misaligned address, frames outside 1 .. 2^24 */
#define GEM_GROUND_SOURCE_PLANE 0
#define GEM_GROUND_SOURCE_BODY_NORMAL 1
#define GEM_GROUND_SOURCE_BODY 2
typedef struct gem_ground_record {
    double status, source;                          /* 0 or GEM_GROUND_NO_BODY / GEM_GROUND_BAD_SEQUENCE; GEM_GROUND_SOURCE_* */
    double n[3], d, u0[3], tilt_cos;                /* the plane, body up, n . u0 */
    double points, inliers, rms, spread, extent;    /* candidates; inliers and their residual RMS at the final plane; sqrt of the last scatter's middle and largest eigenvalue */
    double contact_right, contact_left;             /* frames in contact */
    double skate, penetration, lift_max, skate_pairs;
    double frames, lag;
    double crt[13];
    double reserved[12];
} gem_ground_record;

/* h_frames [n_sequences] -> h_offsets [n_sequences] (or NULL): where in d_work, in doubles, a sequence of more than
 * GEM_GROUND_LDS_FRAMES frames keeps its foot points, -1 for the others.  Returns the bytes of d_work a call needs (0: none), -1 with the
 * reason in gem_last_error for a bad argument.  Needs no GPU. */
int64_t gem_ground_plane_work(const int64_t* h_frames, int n_sequences, int64_t* h_offsets);

/* h_table (host) and d_table (the same numbers on the device), [4 n_sequences] int64: the device addresses of the sequences, each a
 * [frames,15,3] float64 array of its own; their frame counts; per sequence the device address of a (c, R, t) [13] that is applied to
 * the joints first, or 0; the work offsets of gem_ground_plane_work.  d_records [n_sequences] gem_ground_record.  The call's own
 * arguments are checked before the launch -- an empty table is an error, no grid of zero workgroups is launched --; a row of the
 * table that cannot be used sets its own record's status and leaves the other rows alone.  One launch on `stream`, no
 * synchronisation.  Works on the current device. */
int gem_ground_plane(const int64_t* h_table, const int64_t* d_table, int n_sequences, int lag, double tau_v, double tau_h, double min_spread,
                     int min_points, double foot_height, double* d_work, int64_t work_bytes, double* d_records, void* stream);

/* n records (c, R, t) [13] each: d_out = a, then b, that is c = c_a c_b, R = R_a R_b, t = c_b (t_a . R_b) + t_b.  d_out may be d_a or
 * d_b. */
int gem_similarity_compose(const double* d_a, const double* d_b, double* d_out, int64_t n, void* stream);

/* ---- Foot-skate clean-up: standing feet pinned to the floor, legs by two-bone inverse kinematics: `--foot_lock` ----
 * With the foot points q and the contact rule of gem_ground_plane (a candidate within tau_h of the plane n . p = d, both read from the
 * sequence's gem_ground_record on the device): a RUN is a maximal stretch of at least min_run consecutive contact frames of one foot.
 * Its anchor a = q[s] + mean_f (q[f] - q[s]) over its frames s .. e, and with `snap` a -= (n . a - d) n unless |n . a - d| < 1e-12.
 * The correction of a foot point: a - q[f] inside a run; outside, with k(u) = 1 - u^2 (3 - 2 u) for u < 1 and 0 beyond,
 * (a1 - q[e]) k((f - e) / B) + (a2 - q[s]) k((s - f) / B) for the run before (last frame e, anchor a1) and the run after (first frame
 * s, anchor a2), either of which may be absent; B = min(blend, (s - e) / 2) between two runs, blend at the sequence's ends.  A leg
 * whose correction is not zero is re-solved from its unmoved hip h: l1 = |knee - h|, l2 = |ankle - knee|, target a' = ankle +
 * correction, D = |a' - h|, u = (a' - h) / D.  |l1 - l2| < D < l1 + l2: c = (l1^2 - l2^2 + D^2) / (2 D), knee' = h + c u +
 * sqrt(max(l1^2 - c^2, 0)) b and ankle' = a', b the unit part of knee - h across u (shorter than 1e-9: that of foot - ankle; that
 * too: of the world axis most nearly across u).  D >= l1 + l2: the leg straight and lengthened by g = min(D / (l1 + l2), 1 + stretch),
 * knee' = h + g l1 u, ankle' = h + g (l1 + l2) u; the pin is missed where D / (l1 + l2) > 1 + stretch (`unreachable`).
 * D <= |l1 - l2|: folded on the axis, knee' = h +- l1 u, ankle' = h + |l1 - l2| u (`unreachable`).  foot' = foot + (ankle' - ankle).
 * Only joints 8, 9, 10, 12, 13, 14 change; every other joint, and every leg whose correction is exactly zero, is copied bit for bit.
 * Everything is float64, every sum has a fixed order, there are no floating-point atomics: two calls give the same bytes. */
#define GEM_FOOT_LOCK_RECORD_DOUBLES 24
#define GEM_FOOT_LOCK_NO_CONTACT 2        /* no run in the sequence: it is copied bit for bit (a result, not an error) */
#define GEM_FOOT_LOCK_BAD_GROUND 3        /* the sequence's ground record has a status other than 0: copied */
#define GEM_FOOT_LOCK_BAD_SEQUENCE 4      /* the table's row: no or a misaligned address, in place, frames outside 1 .. 2^24: nothing is written */
typedef struct gem_foot_lock_record {
    double status;                                  /* 0 or GEM_FOOT_LOCK_* */
    double runs_right, runs_left;                   /* runs per foot */
    double pinned_right, pinned_left;               /* frames inside a run */
    double changed;                                 /* frames with a leg that moved */
    double lengthened, unreachable;                 /* legs (frame and side) made straight and longer; legs whose target was missed */
    double delta_max, delta_mean;                   /* the correction's length over the pinned foot points, metres */
    double knee_max;                                /* the largest displacement of a knee */
    double stretch_max;                             /* the largest g (1: no leg was lengthened) */
    double slide_before, slide_after;               /* mean in-plane movement per frame of a foot point over the consecutive frame pairs of one run */
    double slide_pairs, frames;
    double reserved[8];
} gem_foot_lock_record;

/* h_frames [n_sequences] -> h_offsets [n_sequences] (or NULL): where in d_work, in doubles, a sequence keeps its run table (and, beyond
 * GEM_GROUND_LDS_FRAMES frames, its foot points), -1 for a frame count outside 1 .. 2^24.  Returns the bytes of d_work a call needs, -1
 * with the reason in gem_last_error for a bad argument.  Needs no GPU. */
int64_t gem_foot_lock_work(const int64_t* h_frames, int n_sequences, int64_t* h_offsets);

/* h_table (host) and d_table (the same numbers on the device), [4 n_sequences] int64: the device addresses of the sequences, each a
 * [frames,15,3] float64 array; their frame counts; the device addresses of the outputs, arrays of the same size that do not overlap
 * their inputs; the work offsets of gem_foot_lock_work.  d_ground_records [n_sequences] gem_ground_record, as gem_ground_plane wrote
 * them for the same sequences with the same lag, tau_v and tau_h (no read-back in between).  d_records [n_sequences]
 * gem_foot_lock_record.  blend: frames over which a correction is eased in and out.  The call's own arguments are checked before the
 * launch, the argument at fault named in gem_last_error; a row that cannot be used sets its own record's status and leaves the other
 * rows alone.  One launch on `stream`, no synchronisation.  Works on the current device. */
int gem_foot_lock(const int64_t* h_table, const int64_t* d_table, int n_sequences, const double* d_ground_records, int lag, double tau_v,
                  double tau_h, int min_run, int blend, int snap, double stretch, double* d_work, int64_t work_bytes, double* d_records,
                  void* stream);

/* ---- Bridging the frames on which SLAM lost tracking: `--bridge` ----
 * The n frames of a recording's span carry metric poses relative to the first frame (t xyz, q xyzw); a frame whose byte in `tracked`
 * is 0 has none.  A GAP is a maximal run of lost frames with tracked neighbours e and s.  Rotation of a lost frame t: slerp between
 * the unit quaternions of e and s (the second negated where their dot product is negative) at u = (t - e) / (s - e), the normalised
 * linear blend where the angle between them is below 1e-8; every matrix is made from the normalised quaternion.  Translation: the
 * unknown c_t minimise the sum of |c_{t-1} - 2 c_t + c_{t+1}|^2 over every t in [e, s] whose three frames lie in the span and hold a
 * lost frame; gaps with fewer than two tracked frames between them couple and form ONE system, given as (first lost frame, frames up
 * to and including its last lost frame).  A system's normal equations (symmetric positive definite, pentadiagonal, one matrix for the
 * three axes, at most GEM_BRIDGE_MAX_GAP unknowns) are solved by Cholesky in a fixed order, for the offset from the straight line
 * between the system's tracked neighbours.  Then G[f] is frame f's 4x4 matrix, cams[f] = inv(G[a]) G[f] with a the first frame of f's
 * chunk and the rigid inverse (R^T, -R^T c), origins[k] = G[a_k], bridged[f] = 1 for a lost frame.  Everything is float64, there
 * are no floating-point atomics: two calls give the same bytes.  tests/bridge_twin.py is the specification. */
#define GEM_BRIDGE_MAX_GAP 64             /* lost frames of one gap, and unknowns of one system */
#define GEM_BRIDGE_MAX_SPAN 127           /* frames of one system: 64 lost ones with single tracked frames between them */
#define GEM_BRIDGE_RECORD_DOUBLES 16
#define GEM_BRIDGE_NOT_SOLVED 2           /* a pivot of a system was not positive (poses that are not finite): status of the record */
typedef struct gem_bridge_record {
    double status;                                  /* 0 or GEM_BRIDGE_NOT_SOLVED */
    double frames, lost, gaps, systems;
    double longest_gap;                             /* lost frames */
    double offset_max;                              /* largest |c_t - straight line between the gap's neighbours|, metres */
    double angle_max;                               /* largest rotation bridged across one gap, radians */
    double translation_max;                         /* largest |c_s - c_e| bridged across one gap, metres */
    double reserved[7];
} gem_bridge_record;

/* The bytes of d_work a call on n frames needs; -1 with the reason in gem_last_error unless n lies in 1 .. 2^20.  Needs no GPU. */
int64_t gem_slam_bridge_work(int64_t n);

/* d_poses [n,7] float64; h_tracked / d_tracked [n] bytes (the same on the host and on the device, like the tables that follow);
 * h_systems / d_systems [n_systems,2] int32 (may be NULL for none); h_chunk_starts / d_chunk_starts [n_chunks] int32, ascending from
 * 0.  Outputs: d_G [n,4,4], d_cams [n,4,4], d_origins [n_chunks,4,4] float64, d_bridged [n] bytes, d_record one gem_bridge_record.
 * The host tables are checked before the launch and the argument at fault named in gem_last_error: null pointers, n outside
 * 1 .. 2^20, alignment, a first or last frame that is not tracked, chunk starts out of order, and a system table that is not the
 * one of the mask (a system out of place, longer than GEM_BRIDGE_MAX_SPAN frames or with more than GEM_BRIDGE_MAX_GAP unknowns, a
 * lost frame outside every system).  Two launches on `stream` (one workgroup of 256 per system, then the per-chunk rebase), no
 * synchronisation.  Works on the current device. */
int gem_slam_bridge(const double* d_poses, const unsigned char* h_tracked, const unsigned char* d_tracked, const int32_t* h_systems,
                    const int32_t* d_systems, int n_systems, const int32_t* h_chunk_starts, const int32_t* d_chunk_starts, int n_chunks,
                    int64_t n, double* d_G, double* d_cams, double* d_origins, unsigned char* d_bridged, double* d_work, int64_t work_bytes,
                    double* d_record, void* stream);

/* ---- A recording optimised as one continuous motion: merging windows that are not equally spaced ----
 * d_windows [n_windows,T,n_joints,3] float64, d_starts [n_windows] the windows' first frames, ascending.  d_merged [n_frames,n_joints,3]:
 * every frame the mean of ALL windows that cover it, ((G_a + G_b) + ...) / count over the covering windows oldest first, a frame's
 * first window taken as it is (a -0.0 survives); at equally spaced starts these are the bits of gem_merge_windows (smoothing off) and
 * of gem_merge_dense.  d_count [n_frames] (may be NULL): the number of covering windows.  d_spread [n_frames] (may be NULL): the
 * largest Euclidean distance, over joints and covering windows, between a window's joint and the merged joint, 0 where count is 1.
 * d_smooth (may be NULL; the shape of d_merged, another buffer): gaussian_filter1d(sigma=1, mode='reflect', truncate=4) of d_merged along
 * the frames, by the kernel gem_merge_windows smooths with, in a second launch.  A frame no window covers gets NaN, count 0 and spread
 * NaN.  The kernel is safe whatever the table holds (every read is guarded, a frame looks at no more than T windows); that the table
 * covers the frames without a hole is the caller's to check (sequence.check_cover).  Refused before any launch, with the reason in
 * gem_last_error: NULL d_windows, d_starts or d_merged, T < 1, n_joints outside 1 .. GEM_MAX_JOINTS, a negative size, more than 2^40
 * / (3 T n_joints) windows, more than 2^33 frames (2^30 with d_smooth).  One wavefront per frame, no atomics: a frame's bytes do not
 * depend on the launch.  Asynchronous on `stream`; works on the current device. */
int gem_merge_cover(const double* d_windows, const int32_t* d_starts, int64_t n_windows, int T, int n_joints, int64_t n_frames,
                    double* d_merged, double* d_smooth, int32_t* d_count, double* d_spread, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEM_HIP_H */
