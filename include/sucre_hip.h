/*
 * sucre_hip.h -- C ABI of libsucre_hip.so, the MI355X (gfx950) engine for the SUCRe hot path.
 *
 * The reference (clementinboittiaux/sucre) is pure Python and has no FFI layer; its boundary for this path is
 * the Python surface   sfm.Image.match_images (sfm.py:127-138),  loader.MatchesFile.prepare_matches /
 * load_matches (loader.py:78-118),  sucre.SUCRe.__init__/update_J/forward (sucre.py:36-82)  and
 * sucre.adam (sucre.py:124-157).  A drop-in therefore binds these entry points with ctypes (INTEGRATION.md shows
 * the stub); sucre_amd/{sfm,loader,sucre}.py is that binding, mirroring the reference's names and arguments.
 *
 * Conventions
 *   - Plain C: pointers and sizes only.  Every `*_dev` / device pointer is HIP device memory owned by the
 *     caller (e.g. a PyTorch-ROCm allocation); the library allocates no persistent device memory, performs no
 *     host<->device copy of bulk data and never synchronises: every call only enqueues kernels on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream) and returns.
 *   - Return value: 0 = OK, negative = error; sucre_last_error() gives the message for the calling thread.
 *     No C++ exception crosses the ABI.  All arguments are validated before anything is launched.
 *   - Re-entrant; no global mutable state except the thread-local error string and the host copies of the light
 *     groups' image tables (sucre_light_group_init, behind a lock).  One host thread / process
 *     per GPU; concurrent calls on different streams or devices are safe.
 *   - All state of one restoration lives in ONE caller-allocated workspace of sucre_workspace_bytes() bytes,
 *     256-byte aligned.  Its internal layout (observation store, Adam state, ...) is private; the few regions a
 *     host needs to read back are located with sucre_ws_offset().
 *   - A workspace, an extension workspace (`lws`), a group buffer, a batch table and a scratch buffer may hold anything when
 *     they are handed in -- the library clears nothing wholesale, every region is written by the call that owns it before
 *     another reads it -- and the same bytes may be laid out again for another `n_views` (or mode) between images.
 *
 * Data layout in HBM: the target image is cut into 16x16-pixel tiles.  Matching writes,
 * for every (tile, view) pair, one 1792-byte chunk = 256 float32 ranges z=||cP|| (0 = no observation) + 256 x 3
 * uint8 colours (7 B/observation instead of the reference's 28-byte (u,v,cP,I) records, loader.py:33-53,103-118,
 * and its HDF5 spill); sucre_finalize_matches then compacts them per pixel, sorted by observation count, into the
 * store the fit streams: the sorted pixels are cut into strips of 64 (one pixel per lane of the wave that fits the
 * strip), a strip's observations are stored as chunks of 64 pixels x 4 levels, and finalize also writes every fit
 * wave's list of items to stream (the plan).  J and the Adam moments are float32 planes per strip in that sorted order.
 */
#ifndef SUCRE_HIP_H
#define SUCRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUCRE_ABI_VERSION 2

/* error codes */
#define SUCRE_OK 0
#define SUCRE_ERR_ARG (-1)      /* NULL / misaligned pointer, bad size            */
#define SUCRE_ERR_RANGE (-2)    /* view index, iteration count ... out of range    */
#define SUCRE_ERR_LAUNCH (-3)   /* HIP reported a launch error                     */

/* fit flags */
#define SUCRE_FIT_CLOSED_FORM 1u /* --use-closed-form: J is a closed-form buffer, sucre.py:66-77,141 */
#define SUCRE_FIT_OBS_U16MM 2u   /* the store was finalised with SUCRE_OBS_U16MM (must match, see below) */
#define SUCRE_FIT_KEEP_J 8u      /* with SUCRE_FIT_CLOSED_FORM: do not append the final update_J (sucre.py:156), i.e. leave
                                    J = J(theta_k) of the last iteration k next to theta_{k+1} -- the pair the reference
                                    plots at a --save-interval stop (sucre.py:141,153-154) */
#define SUCRE_FIT_UNPAIRED 32u   /* sucre_fit_run without SUCRE_FIT_CLOSED_FORM: one launch per iteration, as before the
                                    iterations were taken in pairs of launches that touch a pixel's Adam moments once per pair.
                                    Either way every result bit is the same (tests, A/B measurements) */

/*
 * Observation formats of the store the fit streams.  SUCRE_OBS_F32: float32 range + 3 uint8
 * colours = 7 B/observation, lossless for the reference's data (default).  How the library keeps those float32 ranges is
 * its own business as long as every bit comes back: when all ranges of an image lie within 2^24 - 2 float32 bit patterns
 * of the smallest one (a span of about a factor of four) and nothing rides along in extension planes, the finalize step
 * stores them as 24-bit offsets from it (6 B/observation, decided on the device, no host synchronisation); an image whose
 * ranges span more keeps the float32 words.  SUCRE_OBS_F32_Z26 asks for 26-bit offsets instead (6.25 B/observation) whenever
 * the ranges lie within 2^26 - 2 bit patterns (a factor of up to 256 between the nearest and the farthest range) -- an
 * opt-in: measured, the fit reads the words faster than it decodes these.  Results are bit-identical
 * whichever form the store takes.  SUCRE_OBS_F32_PLAIN asks for the float32 words themselves (A/B measurements, tests).
 * SUCRE_OBS_U16MM: the range as uint16 millimetres, rint(1000 z) clamped to [1, 65535] = 5 B/observation (BASELINE
 * config 5) -- lossy by at most 0.5 mm of range; every sum is still accumulated in float32/float64 exactly as with
 * SUCRE_OBS_F32.  A store finalised with SUCRE_OBS_F32 or SUCRE_OBS_F32_PLAIN is fitted WITHOUT SUCRE_FIT_OBS_U16MM.
 */
#define SUCRE_OBS_F32 0
#define SUCRE_OBS_U16MM 1
#define SUCRE_OBS_F32_PLAIN 2
#define SUCRE_OBS_F32_Z26 3   /* float32 ranges as 26-bit offsets when they fit, else as words (never the 24-bit form) */

/*
 * What the three float32 extension planes of the second workspace (`lws`, see the *_light entry points) carry per
 * observation.  SUCRE_EXT_POINTS: the camera-frame point cP (artificial-light model).  SUCRE_EXT_COLOUR: the colour I
 * as float32 -- for inputs that are not k/255 (the reference's --image-scale resizes colours in float64,
 * loader.py:156-163), with the plain water model; the uint8 colours of the main store are then unused.
 */
#define SUCRE_EXT_POINTS 1
#define SUCRE_EXT_COLOUR 2
#define SUCRE_EXT_POINTS_COLOUR 3 /* both, in two sets of planes: the light model on inputs whose colours are not k/255
                                     (--light-model with --image-scale); needs sucre_light_workspace_bytes_ext(.., 3) */
#define SUCRE_FIT_EXT_COLOUR 4u  /* flag of sucre_fit_run_light / sucre_update_J_ext: lws was matched with SUCRE_EXT_COLOUR */
#define SUCRE_FIT_EXT_BOTH 16u   /* ... with SUCRE_EXT_POINTS_COLOUR: the light model on float32 colours (excludes the former) */

/*
 * One view of the scene = the arguments the reference reads from an sfm.Image (sfm.py:81-88): depth map,
 * colour image, camera, pose.  The 3x3 matrices are row-major float32 and must be computed by the caller the
 * way the reference computes them (Kinv = K.inverse(), sfm.py:92; Rinv/tinv = Pose.inverse() = (R.T, -R.T@t),
 * sfm.py:42-47) so that match sets are bit-identical to the reference's.
 */
typedef struct sucre_view {
    const float *depth;   /* device, (H,W) float32 metres, <=0 = invalid   loader.py:166-170 */
    const uint8_t *rgb;   /* device, (H,W,3) uint8                         loader.py:156-163
                             NULL in a NEIGHBOUR view of sucre_match_views / sucre_match_views_light / sucre_match_map:
                             `depth` then points to the view's sucre_pack_view records (depth and colour in one gather) */
    int32_t H, W;
    float K[9];
    float Kinv[9];
    float R[9];           /* world-from-camera                              sfm.py:32-40      */
    float t[3];
    float Rinv[9];
    float tinv[3];
} sucre_view_t;

/* workspace regions a host may read back (all written by the library) */
enum {
    SUCRE_WS_VIEW_COUNT = 0, /* uint64[n_views]  matches per view (before the min_cover rule), sfm.py:136 */
    SUCRE_WS_VIEW_KEEP = 1,  /* uint32[n_views]  1 = view passed min_cover                                */
    SUCRE_WS_N_OBS = 2,      /* uint64[1]        len(matches_data), sucre.py:135,202                       */
    SUCRE_WS_PARAMS = 3,     /* float32[9]       B[3], beta[3], gamma[3], sucre.py:41-43                  */
    SUCRE_WS_SUMS = 4,       /* float64[12]      reduced gradient sums of the last sucre_fit_grad (multi-GPU) */
    SUCRE_WS_N_OBS_TOTAL = 5,/* uint64[1]        n_obs used for the 1/(3 n_obs) scale (shared-water: summed over ranks) */
    SUCRE_WS_STORE_FORMAT = 6,/* uint32[4]       how sucre_finalize_matches* laid the observations out: 0 = float32 ranges,
                                                 1 = uint16 millimetres, 2 = 24-bit, 3 = 26-bit offsets of the float32 bit
                                                 patterns; the offset; the smallest and the largest float32 bit pattern among
                                                 the ranges */
    SUCRE_WS_STATE = 7,      /* float32[4 tiles][9][64]  J, exp_avg, exp_avg_sq (three channel planes each) of every strip of 64
                                                 count-sorted pixels, tiles = ceil(H/16) ceil(W/16): the fit's per-pixel state */
    SUCRE_WS_PAIR_GRADIENT = 8 /* float32[4 tiles][3][64]  scratch of a sucre_fit_run call that pairs its iterations: the only
                                                 bytes of a workspace that depend on SUCRE_FIT_UNPAIRED; runs to the workspace's end
                                                 together with the paired launches' item lists */
};

int sucre_version(void);
const char *sucre_last_error(void);

/* Bytes of the workspace for an HxW target fitted against n_views views (0 on invalid arguments). */
size_t sucre_workspace_bytes(int H, int W, int n_views);
/* Byte offset of a SUCRE_WS_* region inside the workspace (-1 on invalid arguments). */
int64_t sucre_ws_offset(int H, int W, int n_views, int region);

/*
 * Replaces Image.match_images (sfm.py:127-138) + MatchesFile.prepare_matches/load_matches (loader.py:78-118)
 * for views k0 <= k < k1 of `views_dev` (a device array of n_views sucre_view_t): two-way depth-map matching
 * (sfm.py:90-125, 154-175), d = depth2[v2,u2], cP = K2^-1 d [u2+.5, v2+.5, 1], z = ||cP|| (sucre.py:53),
 * I = rgb2[v2,u2]; results go to the observation store of `ws`.  `target` is a HOST struct whose depth/rgb
 * point to device memory.
 */
int sucre_match_views(void *ws, int H, int W, int n_views, const sucre_view_t *target,
                      const sucre_view_t *views_dev, int k0, int k1, void *stream);

/*
 * Image.match_two_way (sfm.py:121-125) of the target against view k in dense form: map_dev[(v1,u1)] = v2*W2 + u2
 * of the matched pixel, or -1 (H*W int32).  The (u1,v1,u2,v2) lists of sfm.Matches (sfm.py:145-152) are its
 * non-negative entries in row-major order.  Needs no workspace.  Used by the sfm.Matches compatibility API,
 * the HDF5 shim of loader.MatchesFile.save_matches (loader.py:68-76) and the parity tests.
 */
int sucre_match_map(int H, int W, int n_views, const sucre_view_t *target, const sucre_view_t *views_dev, int k,
                    int32_t *map_dev, void *stream);

/*
 * Optional, per neighbour view and once per scene: depth map and uint8 colour image interleaved into H*W 8-byte records
 * {float32 depth, r, g, b, 0} at packed_dev (8-byte aligned, H*W*8 bytes).  A view of `views_dev` whose `rgb` is NULL and
 * whose `depth` points to such records is matched with ONE gather per landing pixel instead of two (the match kernel is
 * bound by its gathers); the values are the same, so are the results.  The target keeps the plain form (its depth map and
 * colour image are read as such: sfm.py:129, sucre.py:47).  Not for float32 colour images (SUCRE_EXT_COLOUR modes).
 */
int sucre_pack_view(const float *depth_dev, const uint8_t *rgb_dev, int H, int W, void *packed_dev, void *stream);
/*
 * The same for n views of one size in as few launches as possible (sixteen views per launch): depth_dev[k], rgb_dev[k],
 * packed_dev[k] are HOST arrays of device pointers.  A target's image_list (sfm.py:127-138) is packed with five launches
 * instead of 65.
 */
int sucre_pack_views(const float *const *depth_dev, const uint8_t *const *rgb_dev, void *const *packed_dev, int n, int H, int W,
                     void *stream);

/*
 * Image.project_to_view + the truncation and bound test of Image.match_one_way (sfm.py:103-107, 115-117) for an
 * explicit list of world points: wP_dev is (3, n) float32 row-major (x[n], y[n], z[n], as sfm.py lays points out),
 * pix_dev[i] = v2 * W + u2 of the pixel of `view` that point i truncates into, or -1 when it falls outside the
 * sensor (NaN / inf included; like the reference, nothing tests that the point is in front of the camera).  Same
 * float32 operation order as the fused match kernel, i.e. bit-identical to the reference's torch CPU arithmetic.
 * `view` is a HOST struct (only its camera and pose are read).  This is the building block behind
 * sfm.Image.match_one_way / match_two_way when a caller passes its own point sets.
 */
int sucre_project_points(const sucre_view_t *view, const float *wP_dev, int64_t n, int32_t *pix_dev, void *stream);

/*
 * Alternative to sucre_match_views for one view: loads an explicit match list -- one group of a matches file
 * written by the reference (loader.py:68-76: u1, v1 int16; the ranges z = ||K2^-1 d [u2+.5, v2+.5, 1]|| of
 * loader.py:113 + sucre.py:53 and the colours I*255 as uint8, n x 3) -- into view k of the observation store,
 * replacing whatever the view held.  This is how a kept matches file (--keep-matches, sucre.py:185) is consumed
 * without re-matching.  Follow with sucre_finalize_matches as usual.
 */
int sucre_import_view(void *ws, int H, int W, int n_views, int k, const int16_t *u1_dev, const int16_t *v1_dev,
                      const float *z_dev, const uint8_t *rgb_dev, int64_t n, void *stream);

/*
 * The `len(matches) / (W*H) > min_cover` rule (sfm.py:136) for every view, n_obs, and the count-sorted per-pixel
 * compaction of the kept observations that the fit iterates over.  Call once after all sucre_match_views calls.
 */
int sucre_finalize_matches(void *ws, int H, int W, int n_views, double min_cover, void *stream);
/*
 * Same with an explicit observation format.  A store finalised with SUCRE_OBS_U16MM must be fitted with
 * SUCRE_FIT_OBS_U16MM in the flags of sucre_fit_run / sucre_fit_grad (and sucre_update_J_fmt); a mismatch is
 * detected on the device and poisons the logged cost with NaN instead of reading the store wrongly.
 */
int sucre_finalize_matches_fmt(void *ws, int H, int W, int n_views, double min_cover, int obs_format, void *stream);

/*
 * SUCRe.__init__ (sucre.py:36-50): B, beta, gamma <- params0 (host, 9 floats; the reference uses 0.1),
 * J <- rgb1/255 with NaN where depth1 <= 0, Adam moments <- 0.  If J0_dev != NULL it is an (H,W,3) float32
 * warm start replacing rgb1/255 (--params-path, sucre.py:206-207).
 */
int sucre_fit_init(void *ws, int H, int W, int n_views, const uint8_t *rgb1_dev, const float *depth1_dev,
                   const float *params0, const float *J0_dev, void *stream);

/*
 * sucre.adam (sucre.py:124-157): iterations t0+1 .. t0+T of torch.optim.Adam(lr, betas, eps) on {B,beta,gamma,J}
 * (or {B,beta,gamma} with SUCRE_FIT_CLOSED_FORM), all enqueued without a host sync.  trace_dev (nullable) gets
 * T x 10 float64: the cost sum r^2 the reference logs (sucre.py:146,150) and the nine parameters after the step.
 * With SUCRE_FIT_CLOSED_FORM the final update_J of sucre.py:156 is included (unless SUCRE_FIT_KEEP_J), and a run that
 * starts at t0 = 0 first solves J once from the initial parameters, so that the one-pass kernel measures its
 * residuals from a J that is already close (accuracy only: iteration 0 re-solves J from the observations anyway).
 * Without SUCRE_FIT_CLOSED_FORM the T iterations run as T / 2 pairs of launches (and one single launch if T is odd) unless
 * SUCRE_FIT_UNPAIRED: nothing is pending when the call returns, and the workspace holds what T single launches leave.
 */
int sucre_fit_run(void *ws, int H, int W, int n_views, int t0, int T, double lr, double beta1, double beta2,
                  double eps, unsigned flags, double *trace_dev, void *stream);

/*
 * The two halves of one iteration, for data-parallel runs where several GPUs share the water parameters:
 * sucre_fit_grad leaves the reduced sums at SUCRE_WS_SUMS (float64[12]) so the host can all-reduce them
 * (RCCL) before sucre_fit_step applies Adam to B, beta, gamma.  sucre_fit_run == T x (grad, step).
 */
int sucre_fit_grad(void *ws, int H, int W, int n_views, int step, double lr, double beta1, double beta2,
                   double eps, unsigned flags, void *stream);
int sucre_fit_step(void *ws, int H, int W, int n_views, int step, double lr, double beta1, double beta2,
                   double eps, double *trace_row_dev, void *stream);
/* Overrides the observation count used in the 1/(3 n_obs) gradient scale (sum over ranks). */
int sucre_set_n_obs_total(void *ws, int H, int W, int n_views, uint64_t n_obs_total, void *stream);

/*
 * Shared water parameters over SEVERAL images (all the images of one rank; BASELINE config 4): one launch and one
 * collective per iteration.  `group_dev`: sucre_group_bytes(n_images) bytes of device memory, 256-byte aligned, set
 * up once by sucre_group_init from the images' workspaces (each matched, finalised and fit_init-ed; `images` is a host
 * array) and the nine start parameters.  sucre_group_iter(step), step = 1, 2, ...: first takes the Adam step on B,
 * beta, gamma that the sums left by the previous call -- all-reduced over the ranks by the host in between -- call
 * for (and logs it in row step-2 of trace_dev, T x 10 float64, nullable), then runs the gradient pass of iteration
 * `step` over every image (J steps stay local, sucre.py:142-148) and leaves this rank's ten float64 sums at
 * sucre_group_sums_offset() inside the buffer.  sucre_group_finish(step) takes the last pending step and copies the
 * final parameters into every image's workspace (SUCRE_WS_PARAMS).  n_obs_total: observations over all images of all
 * ranks, the n_obs of the 1/(3 n_obs) scale.
 */
typedef struct sucre_group_image {
    void *ws;              /* the image's workspace */
    int32_t H, W, n_views; /* its geometry */
    int32_t reserved;
} sucre_group_image_t;
size_t sucre_group_bytes(int n_images);
int64_t sucre_group_sums_offset(void);
int sucre_group_init(void *group_dev, int n_images, const sucre_group_image_t *images, const float *params0, void *stream);
int sucre_group_iter(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps, unsigned flags,
                     uint64_t n_obs_total, double *trace_dev, void *stream);
int sucre_group_finish(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                       uint64_t n_obs_total, double *trace_dev, void *stream);

/*
 * Independent images, ONE launch per iteration: the loop over the images of a scene (sucre.py:243-261, one SUCRe module and one
 * sucre.adam call per image, nothing shared) with the iterations of n_images images advancing together.  Every image keeps
 * its own B, beta, gamma, J, Adam state and log; its results are bit for bit those of sucre_fit_run on it alone -- the
 * launch only spares small images the per-launch cost they are dominated by (BASELINE config 1) and fills the end of one
 * image's pass with the next image's beginning.  All images have one size (H, W: one launch grid); their view counts may
 * differ (n_views[i] = what image i's workspace was laid out for).  They must have been matched / imported, finalized and
 * initialised (sucre_fit_init) and stand at the same step t0.
 * ws / trace_dev / n_views: HOST arrays of n_images entries (trace_dev itself or any of its entries may be NULL; an entry is
 * that image's (T, 10) float64 device log as in sucre_fit_run); batch_dev: sucre_batch_bytes(n_images) bytes of device memory,
 * 256-byte aligned, that the call fills (the image table the launches read) and that must stay untouched until they have run.
 * flags as in sucre_fit_run.
 */
size_t sucre_batch_bytes(int n_images);
int sucre_fit_run_batch(void *batch_dev, int n_images, void *const *ws, double *const *trace_dev, int H, int W, const int *n_views,
                        int t0, int T, double lr, double beta1, double beta2, double eps, unsigned flags, void *stream);

/* SUCRe.update_J(force_update=True) (sucre.py:66-77): closed-form J from the current parameters. */
int sucre_update_J(void *ws, int H, int W, int n_views, void *stream);
int sucre_update_J_fmt(void *ws, int H, int W, int n_views, int obs_format, void *stream);

/* J as the reference lays it out: (H,W,3) float32 (sucre.py:213-215). */
int sucre_export_J(const void *ws, int H, int W, int n_views, float *J_dev, void *stream);

/*
 * Output stage, SUCRe.plot_J (sucre.py:84-95): exact order statistics of the restored image without moving it.  For
 * every channel of J_dev ((H,W,3) float32) the values at the given 0-based ranks among the VALID pixels (no NaN in any
 * channel, sucre.py:87), ascending: out_dev[c * n_ranks + r].  `ranks` is a host array of n_ranks <= 8 entries, each
 * below the number of valid pixels; scratch_dev: sucre_select_scratch_bytes() bytes, 8-byte aligned.  numpy's percentile
 * is a linear interpolation between two such values; the caller does that part (in numpy's arithmetic).
 */
size_t sucre_select_scratch_bytes(void);
int sucre_select_ranks(const float *J_dev, int H, int W, int n_ranks, const uint64_t *ranks, float *out_dev, void *scratch_dev,
                       void *stream);

/* Number of valid pixels of J_dev (no NaN in any channel: `valid`, sucre.py:86-87) -> *count_dev (uint64, device). */
int sucre_count_valid(const float *J_dev, int H, int W, uint64_t *count_dev, void *stream);

/*
 * The remainder of SUCRe.plot_J (sucre.py:88-94) in one pass over J_dev: clip every channel to [lo[c], hi[c]] (the
 * two percentiles; host arrays of 3), subtract the minimum, divide by the maximum, multiply by 255 and truncate to
 * uint8 -> out_dev ((H,W,3) uint8); pixels with a NaN come out black.  After the clip the minimum is lo[c] and the
 * maximum of the shifted values is the float32 difference hi[c] - lo[c], so no reduction is involved and the result
 * equals numpy's bit for bit.
 */
int sucre_plot_stretch(const float *J_dev, int H, int W, const float *lo, const float *hi, uint8_t *out_dev, void *stream);

/*
 * ---- pooled radix select: order statistics of the valid pixels of MANY images ------------------------------------------
 * The select above for a POOL of images -- of any sizes, in any number of chunks, possibly on several ranks -- without
 * concatenating or moving them: for every channel the values at given 0-based ranks among the valid pixels (no NaN in any
 * channel) of all the images together.  It is split into its phases so that the caller can add histograms between them:
 *     begin;  for pass = 0..3: { pass (once per chunk of images) ...;  [all-reduce the histograms over the ranks];  locate }
 * `state_dev`: sucre_pool_select_bytes() bytes of device memory, 8-byte aligned.  It BEGINS with uint64_t hist[3][8][256]
 * ([channel][rank][byte]; this placement is part of the contract: the caller may sum these 6144 words over processes between
 * the pass calls and locate); what follows (prefix, remaining rank per channel and rank) is private.
 * sucre_pool_select_begin zeroes the state.
 * sucre_pool_select_pass ADDS to hist the histogram of key byte 3 - pass over the valid pixels of the chunk's images whose
 * higher key bytes equal the rank's prefix (the key is the order-preserving integer image of the float32 bits); it may be
 * called any number of times per pass.  Pass 0 has no prefix, does not depend on the ranks and fills hist[c][0] only: the sum
 * of hist[0][0][0..255] after the pass-0 calls IS the number of valid pixels of the pool, from which the caller forms the
 * ranks -- there is no separate counting pass.  `images`: HOST array of n_images entries, 0 <= n_images <= 4096; J: device,
 * (n_px, 3) float32, 16-byte aligned; n_px >= 0 (an image with n_px == 0, whose J may be NULL, or with NaN in every pixel is
 * legal and contributes nothing); the images of one call may hold 2^45 pixels together.  `table_dev`:
 * sucre_pool_table_bytes(n_images) bytes of device memory (0 on an invalid count), 8-byte aligned, that the call fills -- by
 * value through small kernels -- and that must stay untouched until the launch has run; it may be NULL when n_images == 0.
 * sucre_pool_select_locate consumes hist: finds the byte under which each rank falls, updates prefix and remaining rank and
 * zeroes hist.  `ranks`: HOST array of n_ranks 0-based pooled ranks, each below the pooled valid count, read at pass 0 only
 * (may be NULL later).  After pass 3 it writes out_dev[c * n_ranks + r] (device, 3 * n_ranks float32; may be NULL before).
 * 1 <= n_ranks <= 8, the same in every call of a select; pass = 0..3; anything else, a NULL or misaligned pointer and a
 * negative count give SUCRE_ERR_ARG without a launch.  The calls only enqueue.
 */
typedef struct sucre_pool_image {
    const float *J;
    int64_t n_px;
} sucre_pool_image_t;
size_t sucre_pool_select_bytes(void);
size_t sucre_pool_table_bytes(int n_images);
int sucre_pool_select_begin(void *state_dev, void *stream);
int sucre_pool_select_pass(void *state_dev, int pass, void *table_dev, int n_images, const sucre_pool_image_t *images, int n_ranks,
                           void *stream);
int sucre_pool_select_locate(void *state_dev, int pass, int n_ranks, const uint64_t *ranks, float *out_dev, void *stream);

/*
 * MatchesFile.check_integrity (loader.py:89-101) over the whole store in one launch: verdict_dev[k] (uint32, one per
 * view) gets bit 0 if a stored range of view k is not finite, bit 1 if one is negative, bit 2 if the number of
 * stored ranges > 0 differs from the view's match count; 0 = sound.  scratch_dev: n_views uint64 of scratch.
 */
int sucre_check_store(const void *ws, int H, int W, int n_views, uint32_t *verdict_dev, uint64_t *scratch_dev,
                      void *stream);

/*
 * One view of the observation store as dense planes (inverse of the tiling): z (H,W) float32, 0 = no match,
 * and rgb (H,W,3) uint8.  Either output may be NULL.  Used by tests and by the MatchesData compatibility shim.
 */
int sucre_export_view(const void *ws, int H, int W, int n_views, int k, float *z_dev, uint8_t *rgb_dev,
                      void *stream);

/*
 * ---- artificial-light model: --light-model, SUCRe.compute_l_z with se3.exp (sucre.py:54-61, se3.py:22-27) ------------
 * The model needs the camera-frame point cP of every observation (loader.py:113), which the 7-byte store does not
 * keep, so this mode uses a second caller-owned buffer `lws` of sucre_light_workspace_bytes() bytes (256-byte
 * aligned) next to `ws`: three float32 planes per chunk + the 19 parameters B[3], beta[3], gamma[3],
 * cam2light[6], sigma[4] (row-major 2x2; sucre.py:41-46) and their Adam state.  The *_light entry points replace
 * their namesakes; J, sucre_export_J, sucre_export_view, sucre_match_map and SUCRE_WS_* work unchanged on `ws`.
 * params0: 19 host floats (the reference starts from 0.1 x 9, 0 x 6, identity).  trace_dev: T x 20 float64
 * (cost, then the 19 parameters after the step).  The parameters live at sucre_light_params_offset() in `lws`.
 */
size_t sucre_light_workspace_bytes(int H, int W, int n_views);
int64_t sucre_light_params_offset(int H, int W, int n_views);
int sucre_match_views_light(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                            const sucre_view_t *views_dev, int k0, int k1, void *stream);
/* Same with float32 colour images: every view's `rgb` points to (H,W,3) float32 instead of uint8 (SUCRE_EXT_COLOUR). */
int sucre_match_views_fcolour(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                              const sucre_view_t *views_dev, int k0, int k1, void *stream);
/*
 * Both at once -- the reference accepts --light-model together with --image-scale (sfm.py:193-199, sucre.py:54-61): the
 * views' `rgb` are (H,W,3) float32 images, the camera points go to the first set of planes and the float32 colours to
 * a second one (SUCRE_EXT_POINTS_COLOUR).  `lws` must then be sucre_light_workspace_bytes_ext(H, W, n_views,
 * SUCRE_EXT_POINTS_COLOUR) bytes (the second set sits behind everything else, so all other offsets are unchanged);
 * finalise with sucre_finalize_matches_ext(.., SUCRE_EXT_POINTS_COLOUR, ..) and pass SUCRE_FIT_EXT_BOTH to
 * sucre_fit_run_light / sucre_update_J_ext.  sucre_finalize_matches_ext with SUCRE_EXT_POINTS or SUCRE_EXT_COLOUR equals
 * sucre_finalize_matches_light.
 */
size_t sucre_light_workspace_bytes_ext(int H, int W, int n_views, int ext_mode);
int sucre_match_views_light_fcolour(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                                    const sucre_view_t *views_dev, int k0, int k1, void *stream);
int sucre_finalize_matches_ext(void *ws, void *lws, int H, int W, int n_views, double min_cover, int ext_mode, void *stream);
/*
 * sucre_import_view with extension planes: ext_dev holds three float32 planes [3][n] -- the camera points cP of the
 * list (loader.py:113; ext_mode SUCRE_EXT_POINTS, rgb_dev required) or its colours I (loader.py:87; SUCRE_EXT_COLOUR,
 * for colours that are not k/255; rgb_dev may be NULL), or both as six planes [6][n], cP first (SUCRE_EXT_POINTS_COLOUR;
 * rgb_dev may be NULL).  This is how a caller-built MatchesData (loader.py:36-53)
 * enters the engine; sucre_export_view_ext returns the planes of view k as (3, H, W), zero where nothing was observed.
 * With the light model the range of an observation IS the norm of its camera point (sucre.py:53, compute_l_z): the
 * J-parameter light kernel forms it from the point instead of reading the stored range, and takes a non-zero cP.z (the
 * depth) as the mark of a real observation.
 * sucre_export_view_ext2 returns the SECOND set of planes of view k the same way: the float32 colours of a store that keeps
 * both sets.  It is valid only for an `lws` of sucre_light_workspace_bytes_ext(.., SUCRE_EXT_POINTS_COLOUR) bytes: a smaller
 * extension workspace has no second set, and the call would read past its end.
 */
int sucre_import_view_ext(void *ws, void *lws, int H, int W, int n_views, int k, const int16_t *u1_dev, const int16_t *v1_dev,
                          const float *z_dev, const uint8_t *rgb_dev, const float *ext_dev, int64_t n, int ext_mode, void *stream);
int sucre_export_view_ext(const void *ws, const void *lws, int H, int W, int n_views, int k, float *planes_dev, void *stream);
int sucre_export_view_ext2(const void *ws, const void *lws, int H, int W, int n_views, int k, float *planes_dev, void *stream);
int sucre_finalize_matches_light(void *ws, void *lws, int H, int W, int n_views, double min_cover, void *stream);
int sucre_fit_init_light(void *ws, void *lws, int H, int W, int n_views, const uint8_t *rgb1_dev, const float *depth1_dev,
                         const float *params0, const float *J0_dev, void *stream);
/* closed-form J with the illumination factor in absorption and backscatter (sucre.py:66-77 with light_model) */
int sucre_update_J_light(void *ws, void *lws, int H, int W, int n_views, void *stream);
int sucre_update_J_ext(void *ws, void *lws, int H, int W, int n_views, unsigned flags, void *stream);
int sucre_fit_run_light(void *ws, void *lws, int H, int W, int n_views, int t0, int T, double lr, double beta1,
                        double beta2, double eps, unsigned flags /* SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_KEEP_J | SUCRE_FIT_EXT_COLOUR or SUCRE_FIT_EXT_BOTH */, double *trace_dev,
                        void *stream);

/*
 * ---- fit residuals per pixel and per view ------------------------------------------------------------------------------
 * Where the fitted model can be trusted, and which view hurts it: one streaming pass over the DENSE store of a matched (or
 * imported), finalised and fitted workspace that evaluates the residual of sucre.adam's objective (sucre.py:144),
 *     r = I - l (J exp(-beta z) + B (1 - exp(-gamma z)))        SUCRe.forward, sucre.py:79-82; l, z: sucre.py:52-64,
 * for every observation of every KEPT view (SUCRE_WS_VIEW_KEEP, sfm.py:136) at the workspace's CURRENT parameters and CURRENT
 * J (the J sucre_export_J would return), and keeps two kinds of sums -- what a caller otherwise rebuilds on the host from
 * MatchesData.iter (loader.py:120-130) to write a --filter-images-path list (sucre.py:227-232):
 *   count_dev       int32   (H,W)        observations of the pixel over the kept views
 *   ssr_dev         float32 (H,W,3)      sum of r^2 per channel over those observations (0 where count is 0)
 *   view_stats_dev  float64 (n_views,4)  per view: observations, then sum of r^2 for R, G, B; zeros for a view that is not kept
 * The workspaces are only read.  scratch_dev: sucre_residual_scratch_bytes() bytes of caller-owned device memory, 16-byte
 * aligned, that must stay untouched until the pass has run; every sum is formed in a fixed order (no atomics), so two calls
 * give the same bits.  obs_format: the format the store was finalised with -- with SUCRE_OBS_U16MM the range of an observation
 * is the one that store's fit reads, 0.001f * clamp(rint(1000 z), 1, 65535); the three float32 forms read the same number.
 * sucre_fit_residuals_ext: the same for a workspace with extension planes.  flags = SUCRE_FIT_EXT_COLOUR: float32 colours from
 * the dense extension planes, plain water model (its nine parameters are the first nine of `lws`); flags = 0: the light model
 * (SUCRE_EXT_POINTS), flags = SUCRE_FIT_EXT_BOTH: the light model on float32 colours.  With the light model l and z come from
 * the camera point cP and R, t, Sigma^-1 of the parameters as they stand in `lws` (derived anew, as sucre_update_J_ext does, so a
 * caller may have written them); the range that enters z = range + ||lP|| is the STORED one of the dense store -- ||cP|| as the
 * match kernel wrote it, or an imported list's own z -- as in the closed-form kernel, not the ||cP|| the J-parameter kernel
 * re-forms from the point.
 */
size_t sucre_residual_scratch_bytes(int H, int W, int n_views);
int sucre_fit_residuals(const void *ws, int H, int W, int n_views, int obs_format, int32_t *count_dev, float *ssr_dev,
                        double *view_stats_dev, void *scratch_dev, void *stream);
int sucre_fit_residuals_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags /* 0 | SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH */,
                            int32_t *count_dev, float *ssr_dev, double *view_stats_dev, void *scratch_dev, void *stream);

/*
 * ---- outlier-trimmed refit: sigma-clip observations out of the dense store -------------------------------------------------
 * The fit is a least-squares mean over every view that sees a pixel, so one fish or diver in one view is averaged into J.  These
 * calls drop the offending OBSERVATIONS (not whole views, as a --filter-images-path list does) from the dense store of a matched
 * (or imported), finalised and fitted workspace.  One round, for a multiple k_sigma > 0:
 *  1 Scale.  view_stats_dev is the table sucre_fit_residuals* has just left (the caller runs that pass; it is only read).  Over
 *    the KEPT views, in view order, in float64: N = sum view_stats[v][0], S_c = sum view_stats[v][1+c]; per channel
 *    tau^2_c = float32(k_sigma^2 S_c / N), formed on the device.  N = 0: nothing is dropped (tau^2 = +inf).
 *  2 Decision.  For every stored observation (match count > 0, z > 0) of every kept view the residual r_c of sucre.adam's
 *    objective (sucre.py:144) is evaluated exactly as sucre_fit_residuals* evaluates it -- one device function serves both: the
 *    SUCRE_OBS_U16MM range, float32 colours, the light model's l, z from the parameters as they stand with the stored range.
 *    The observation is an OUTLIER iff r_c^2 > tau^2_c for any channel, compared in float32; a NaN compares false and stays.
 *  3 Guard.  A pixel whose observations over the kept views would all be outliers keeps all of them.
 *  4 Drop.  A dropped observation's range in the dense store becomes 0; colours and extension planes stay as they are, behind
 *    z > 0.  For every (tile, kept view) pair the match count, the four pixel-bit words and the range pair end up as a recount
 *    of the chunk would leave them (sucre_import_view's last step), the neutral pair where nothing is left.  Views that are
 *    not kept keep their observations, counts and bits; their range pairs are restated as their chunks' own (a matched store
 *    keeps the ranges of several views in the pair of one of them, through which a dropped range could stay in the span).
 *  5 Outputs, on the device, every sum in a fixed order without atomics (two calls give the same bits):
 *      dropped_dev       int32   (H,W)      observations dropped from the pixel
 *      view_dropped_dev  int64   (n_views)  observations dropped from the view (0 for a view that is not kept)
 *      thresholds_dev    float32 [3]        tau^2_c
 *  6 Re-finalise.  The CALLER then runs sucre_finalize_matches_fmt / _ext with the min_cover and format of the first time: view
 *    totals, the min_cover rule (a view that falls below it drops out, as in a plain run on the survivors), n_obs, the range
 *    span, the store format, the compaction and the plans are redone; then sucre_fit_init* and the fit start over, and the
 *    result is bit for bit that of a plain run on a store into which only the survivors were imported.  sucre_match_map is
 *    geometry and keeps returning the untrimmed matches.
 * Nothing in 1-6 waits on the host.  scratch_dev: sucre_trim_scratch_bytes() bytes of caller-owned device memory, 16-byte
 * aligned, untouched until the launches have run.  obs_format / flags: as for sucre_fit_residuals / sucre_fit_residuals_ext.
 * Arguments are checked before anything is launched: k_sigma not finite or <= 0, NULL or misaligned pointers and a bad geometry
 * give SUCRE_ERR_ARG.
 */
size_t sucre_trim_scratch_bytes(int H, int W, int n_views);
int sucre_trim_outliers(void *ws, int H, int W, int n_views, int obs_format, double k_sigma, const double *view_stats_dev,
                        int32_t *dropped_dev, int64_t *view_dropped_dev, float *thresholds_dev, void *scratch_dev, void *stream);
int sucre_trim_outliers_ext(void *ws, const void *lws, int H, int W, int n_views, unsigned flags /* 0 | SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH */,
                            double k_sigma, const double *view_stats_dev, int32_t *dropped_dev, int64_t *view_dropped_dev,
                            float *thresholds_dev, void *scratch_dev, void *stream);

/*
 * ---- per-view gain compensation: estimate, divide out of the dense store ---------------------------------------------------
 * The fit assumes that every view saw the scene with one camera response; auto-exposure, a strobe that has not recharged or a
 * white-balance step makes ONE view brighter or darker than the rest in every pixel.  These calls estimate one multiplicative
 * gain per kept view and channel at the fit as it stands, and divide it out of the dense store of a matched (or imported),
 * finalised and fitted workspace.  One round:
 *  1 Estimate (sucre_view_gains*; the workspaces are only read).  With the modelled intensity of sucre.adam's objective,
 *        Ihat = l (J exp(-beta z) + B (1 - exp(-gamma z)))        SUCRe.forward, sucre.py:79-82, 144 (l, z: sucre.py:52-64),
 *    evaluated exactly as sucre_fit_residuals* evaluates it (one device function serves both: the SUCRE_OBS_U16MM range, float32
 *    colours, the light model's l, z from the parameters as they stand with the stored range), the gain of view k in channel c
 *    is the least-squares answer to I = g Ihat over the view's observations at the CURRENT J and parameters:
 *        g = S_IIhat / S_IhatIhat,   S_IIhat = sum I_c Ihat_c,   S_IhatIhat = sum Ihat_c^2.
 *    The sums are float32 FMAs per (tile, view), then float64 over the view's tiles, all in a fixed order without atomics (two
 *    calls give the same bits); a term whose Ihat is not finite contributes to neither sum.
 *      sums_dev   float64 (n_views,7)  per view: observations, S_IIhat R, G, B, S_IhatIhat R, G, B; zeros for a view not kept
 *      gains_dev  float64 (n_views,3)  g
 *      inv_dev    float32 (n_views,3)  float32(1 / g)
 *    g = 1 and inv = 1 exactly where there is nothing to estimate from: the view is not kept (SUCRE_WS_VIEW_KEEP), it has no
 *    observation, or S_IhatIhat or the quotient is not finite and positive.  Otherwise g is clamped to [1 / limit, limit].
 *    Gains are not normalised: at a converged fit the pooled gain is 1 by the optimality condition.
 *  2 Apply (sucre_apply_view_gains*).  In every slot with z > 0 of every kept view with a match count, the three colours are
 *    multiplied by the view's inv_c (positive and finite, as step 1 leaves them):
 *      uint8 colours    k' = min(255, rintf(float(k) * inv_c)) -- one correctly rounded float32 multiply, then round half to even;
 *      float32 colours  I' = I * inv_c, one float32 multiply, no clamp (SUCRE_FIT_EXT_COLOUR / SUCRE_FIT_EXT_BOTH: the planes of
 *                       `lws` the colours live in; the uint8 colours of such a store are not read by anything and stay).
 *    Empty slots, ranges, match counts, pixel bits, range pairs and views that are not kept are not touched.
 *      view_clipped_dev  int64 (n_views)  uint8 values of the view that met the 255 clamp (0 for a view not kept, and for
 *                                          float32 colours)
 *  3 Re-finalise.  The CALLER then runs sucre_finalize_matches_fmt / _ext with the min_cover and format of the first time -- the
 *    compacted store the fit reads is rebuilt from the dense one; nothing else changes, no view is gained or lost -- and then
 *    sucre_fit_init* and the fit start over: the result is bit for bit that of a plain run on a store into which the corrected
 *    colours were imported.  A uint8 store is re-rounded once per round; a float32-colour store is not rounded at all.
 * Nothing in 1-3 waits on the host.  scratch_dev: sucre_gain_scratch_bytes() bytes of caller-owned device memory (one size for
 * both calls), 16-byte aligned, untouched until the launches have run.  obs_format / flags: as for sucre_fit_residuals /
 * sucre_fit_residuals_ext (the apply needs no range format).  Arguments are checked before anything is launched: NULL or
 * misaligned pointers, a bad geometry and a limit that is not finite or is < 1 give SUCRE_ERR_ARG.
 */
size_t sucre_gain_scratch_bytes(int H, int W, int n_views);
int sucre_view_gains(const void *ws, int H, int W, int n_views, int obs_format, double limit, double *gains_dev, float *inv_dev,
                     double *sums_dev, void *scratch_dev, void *stream);
int sucre_view_gains_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags /* 0 | SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH */,
                         double limit, double *gains_dev, float *inv_dev, double *sums_dev, void *scratch_dev, void *stream);
int sucre_apply_view_gains(void *ws, int H, int W, int n_views, const float *inv_dev, int64_t *view_clipped_dev, void *scratch_dev,
                           void *stream);
int sucre_apply_view_gains_ext(void *ws, void *lws, int H, int W, int n_views, unsigned flags /* 0 | SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH */,
                               const float *inv_dev, int64_t *view_clipped_dev, void *scratch_dev, void *stream);

/*
 * ---- single-view inversion: a fitted water (and light) model applied to any image -------------------------------------------
 * With ONE observation per pixel -- the image itself, through its own depth map -- SUCRe.update_J (sucre.py:66-77) is
 *     J = (I - l B (1 - exp(-gamma z))) a / a^2,   a = l exp(-beta z),   cP = Kinv d [u+.5, v+.5, 1] (loader.py:113),
 *     z = ||cP|| (sucre.py:53), l = 1 -- or l, z = ||cP|| + ||lP|| of SUCRe.compute_l_z (sucre.py:54-61) with SUCRE_INVERT_LIGHT,
 * per pixel, and NaN in all three channels where depth <= 0 (sucre.py:48).  This is what update_J returns on a matches file
 * that holds only the image matched against itself, and the call gives the very bits sucre_update_J / sucre_update_J_ext leave
 * for such a store -- wherever the two-way match of the image with itself keeps every pixel with depth > 0, which a depth map
 * consistent with its camera does -- without matching, without a workspace and without a neighbour view: the way to restore
 * the images of a survey that were not part of the fit with the parameters of those that were.
 * `images`: HOST array of n_images entries, 1 <= n_images <= 4096 (SUCRE_ERR_RANGE otherwise); the images of one call may differ
 * in size.  depth: device, (H,W) float32, 16-byte aligned; rgb: device, (H,W,3) uint8, 4-byte aligned -- or float32, 16-byte
 * aligned, with SUCRE_INVERT_FLOAT_COLOUR (all images of a call alike); J: device, (H,W,3) float32, 16-byte aligned, caller-owned,
 * written in full; Kinv: row-major K.inverse() (sfm.py:92), as in sucre_view_t; reserved: ignored.  1 <= H, W <= 32767.
 * `params`: HOST, B[3], beta[3], gamma[3], and with SUCRE_INVERT_LIGHT cam2light[6], sigma[4] behind them (the geometry is
 * derived anew from them, as sucre_update_J_ext does).  `table_dev`: sucre_invert_bytes(n_images) bytes of device memory (0 on an
 * invalid count), 256-byte aligned, that the call fills -- by value through small kernels, no host-to-device copy -- and that must
 * stay untouched until the launches have run; it may hold anything before.  The call only enqueues, all images in one launch.
 */
#define SUCRE_INVERT_LIGHT 1u          /* params: 19 floats, else 9 */
#define SUCRE_INVERT_FLOAT_COLOUR 2u   /* rgb: (H,W,3) float32, else uint8 */
typedef struct sucre_invert_image {
    const float *depth;
    const void *rgb;
    float *J;
    int32_t H, W;
    float Kinv[9];
    int32_t reserved;
} sucre_invert_image_t;
size_t sucre_invert_bytes(int n_images);
int sucre_invert_images(void *table_dev, int n_images, const sucre_invert_image_t *images, const float *params, unsigned flags,
                        void *stream);

/*
 * ---- cross-view colour consistency of restored images -----------------------------------------------------------------------
 * SUCRe's premise is that one point of the seabed has one restored colour whichever camera saw it.  This call measures it, with
 * no fit and no workspace, from depth maps, poses and the J images a run wrote: for every view k of `views_dev` and every target
 * pixel the match is the one sucre_match_map returns for (target, view k) -- the same device function -- and no map is written.
 * A matched pair is VALID when neither a = J_target[v1,u1,:] nor b = J_k[v2,u2,:] holds a NaN in any channel (plot_J's rule,
 * sucre.py:86-87).  Over the valid pairs:
 *   count_dev  int32   (H,W)          views with a valid pair at the pixel
 *   ssd_dev    float32 (H,W,3)        sum over k, ascending, of (a_c - b_c)^2, accumulated as fmaf(d, d, acc); 0 where count is 0
 *   stats_dev  float64 (n_views,26)   per view: [0] matches (the map's entries >= 0: len(matches) of sfm.py:136, whatever J holds),
 *                                     [1] valid pairs, [2:14] sum d^2, sum a^2, sum b^2, sum a b of J (R, G, B each), [14:26] the same
 *                                     four sums of the raw colours (float)k / 255.0f of the same pixels of the same valid pairs
 * all written in full.  `target`: HOST struct, `views_dev`: device table of n_views entries, as for sucre_match_map; the views may
 * differ in size from the target and from each other and are in PLAIN form (depth map, uint8 rgb -- no sucre_pack_view records).  A
 * view's rgb may be NULL: it is then not read and the view's raw sums are zero (all raw sums, when the target's is); its J sums are
 * formed all the same.  J_target_dev: (H,W,3) float32.  J_views_dev: DEVICE array of n_views device pointers to (H_k,W_k,3) float32;
 * a NULL entry means the view takes no part -- its stats row is zero, it adds nothing to any pixel.  Every sum is formed in float32
 * per (16x16 tile, view), then in float64 over the tiles in a fixed order; no atomics: two calls give the same bits.
 * scratch_dev: sucre_consistency_scratch_bytes() bytes (0 on invalid arguments) of caller-owned device memory that must stay
 * untouched until the launches have run; it may hold anything before.  Checked before any launch: NULL target, views_dev, J_*,
 * outputs or scratch, outputs or scratch not 16-byte aligned, H or W outside 1..32767, a target of another size (SUCRE_ERR_ARG);
 * n_views outside 1..4096 (SUCRE_ERR_RANGE).  The call only enqueues: two launches, no allocation, nothing copied from the host.
 */
size_t sucre_consistency_scratch_bytes(int H, int W, int n_views);
int sucre_view_consistency(int H, int W, int n_views, const sucre_view_t *target, const sucre_view_t *views_dev,
                           const float *J_target_dev, const float *const *J_views_dev, int32_t *count_dev, float *ssd_dev,
                           double *stats_dev, void *scratch_dev, void *stream);

/*
 * ---- seabed mosaic of restored images: best-view ortho splat -------------------------------------------------------------------
 * Every pixel of every image is dropped onto a plane grid and the pixel seen through the least water wins its cell; nothing is
 * blended here (the blend: below) and no hole is filled (sucre_mosaic_fill_*, further below).  Image i of the request (its
 * ORDINAL: first_ordinal + its index in the call) has a depth map, a camera, a world-from-camera pose, its restored J (H,W,3)
 * float32 and its raw uint8 colours.  Pixel p = v W + u TAKES PART when depth > 0 and J[p] holds no NaN in any channel (plot_J's
 * rule, sucre.py:86-87).  In float32, every FMA explicit:
 *   cP = Kinv (d [u+.5, v+.5, 1])                     sfm.py:90-93 (Image.unproject_depth), the match kernels' chain
 *   z  = sqrt(cP.x cP.x + cP.y cP.y + cP.z cP.z)       the range, as sucre_invert_images forms it
 *   wP = R cP + t                                      sfm.py:49-55 (Pose.transform)
 *   a_s = e1 . wP, a_t = e2 . wP                       e1, e2: rows 0 and 1 of `axes` (row-major 3x3), x*e[0], fma(e[1], y, .), fma(e[2], z, .)
 *   q_s = (a_s - lo_s) / gsd, q_t = (a_t - lo_t) / gsd (IEEE); dropped unless 0 <= q_s < Wm and 0 <= q_t < Hm;
 *   cell = (int)q_t * Wm + (int)q_s
 * The winner of a cell is the pixel with the lexicographically smallest (bits of z, ordinal, p); the result does not depend on
 * the order of arrival, so two runs give the same bits.  Four phases, each one call per batch of images, each call one launch per
 * 32 images (plus the table's) on `stream`; nothing is copied from the host, nothing allocated, nothing waited for:
 *   sucre_mosaic_bounds   bounds_dev[0..3] (uint32) = min a_s, min a_t, max a_s, max a_t over the pixels that take part, as
 *                         order-preserving keys: key(x) = bits(x) ^ (bits(x) >> 31 ? 0xffffffff : 0x80000000).  The call
 *                         ACCUMULATES: the caller starts the two min words at 0xffffffff and the two max words at 0
 *   sucre_mosaic_splat    key_dev[cell] (uint64) = min over the pixels of the cell of bits(z) << 32 | ordinal; the caller starts
 *                         every word at all ones (an empty cell keeps that).  z > 0, so a key stays below 2^63.
 *                         flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- issue the 64-bit atomic min for every pixel instead of loading the
 *                         word first and skipping the atomic when it is already smaller (same result; for measurements)
 *   sucre_mosaic_resolve  pix_dev[cell] (uint32) = min p over the pixels whose key equals key_dev[cell]; starts at all ones
 *   sucre_mosaic_gather   the one pixel per filled cell with the cell's key and pix_dev[cell] == p writes J_out (Hm,Wm,3)
 *                         float32 bit for bit, raw_out (Hm,Wm,3) uint8, source_out (Hm,Wm) int32 its ordinal, pixel_out (Hm,Wm)
 *                         int32 p, range_out (Hm,Wm) float32 z.  Empty cells are not touched: the caller fills the outputs first
 * All calls of one mosaic get the same images with the same ordinals, and splat / resolve / gather the same grid.
 * `images`: HOST array; `table_dev`: sucre_mosaic_table_bytes(n_images) bytes of device memory, 256-byte aligned, that must stay
 * untouched until the call's launches have run.  Checked before any launch (SUCRE_ERR_ARG): a NULL or misaligned pointer,
 * n_images or first_ordinal + n_images outside 1..4096, an image size outside 1..32767, gsd or a bound that is not finite, gsd <= 0,
 * Hm or Wm outside 1..2^24, unknown flags.
 *
 * The blend: a range-weighted mean of all the pixels of a cell, next to the best-view outputs, summed in FIXED POINT so that
 * the result has the same bits in any order of arrival and any split into calls.  Once sucre_mosaic_splat has seen every image,
 * key_dev[cell] >> 32 holds the bits of zmin, the cell's smallest range.  For every pixel that takes part and has a cell, with
 * range z, in float32, one IEEE operation per step, inv_h = 1 / H for a blend depth of H metres:
 *   d = z - zmin;  t = max(1 - d inv_h, 0) (product rounded, then the difference);  wq = (int)rintf((t t) 4096), 0..4096, 4096
 *   for the winner and its ties;  Jq_c = (int64)rintf(min(max(J_c, -1024), 1024) 1048576), |Jq_c| <= 2^30 (infinities clamped)
 *   sucre_mosaic_accumulate  a pixel with wq > 0 adds to the SUCRE_MOSAIC_ACC_WORDS = 8 int64 words of its cell, cell-major
 *                         (acc_dev[8 cell + k]; Hm Wm 64 bytes, 8-byte aligned, the caller starts every word at 0):
 *                         k = 0..2: wq Jq_c;  k = 3..5: wq rgb_c (raw uint8);  k = 6: wq;  k = 7: 1, the sample count.
 *                         64-bit integer atomic adds.  THE BOUND: with fewer than 2^20 samples in a cell every sum stays below
 *                         2^62.  Word 7 counts on its own, so a cell that reached 2^20 samples is detected there (any count
 *                         below 2^32): the caller checks samples_out after sucre_mosaic_normalize and discards the blend then.
 *                         flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- eight atomics per pixel instead of eight per run of adjacent
 *                         pixels of a wave that share a cell (same words; for measurements)
 *   sucre_mosaic_normalize   one pass over the cells, no image read; for a cell with word 7 > 0:
 *                         J_out (Hm,Wm,3) float32 = (float)(((double)acc_c / (double)wsum) 2^-20), raw_out (Hm,Wm,3) uint8 =
 *                         (2 racc_c + wsum) / (2 wsum) in integers, weight_out (Hm,Wm) float32 = (float)((double)wsum 2^-12),
 *                         samples_out (Hm,Wm) int32 = the count (2^31 - 1 when above).  Empty cells are not touched: the caller
 *                         fills the outputs first.  A filled cell has wsum >= 4096.
 * Checked before any launch as above, and: inv_h not finite or <= 0, a NULL or misaligned acc_dev or output, Hm Wm above 2^39.
 *
 * The feather: one more factor in the blend's weight, which falls to nothing towards the edge of an image's footprint -- its
 * frame, a NaN patch of J, a hole of the depth map.  A pixel that takes part is a MEMBER of its image.  For a member (u, v) and a
 * feather width of feather_px = F source pixels, 1..SUCRE_MOSAIC_FEATHER_MAX = 1024, in exact integers:
 *   D2 = min over integer (u', v') that are non-members or lie outside [0,W) x [0,H) of (u - u')^2 + (v - v')^2
 *   dist2 = min(D2, F^2), uint32; 0 for a non-member, >= 1 for a member (the frame just outside the image counts)
 *   sucre_mosaic_feather_bytes  the bytes of feather_dev for these images (only H and W are read; 0 and an error for bad sizes):
 *                         image i's dist2, row-major (H,W) uint32, starts at WORD 256 sum_(j<i) ceil(H_j W_j / 256); behind all the
 *                         words, 4 bytes each, sits a uint16 scratch of as many entries: 6 bytes per pixel, images rounded up to 256
 *   sucre_mosaic_feather  writes every image's dist2 (the words between two images are not written); two launches per 32
 *                         images.  feather_dev: 4-byte aligned
 *   sucre_mosaic_accumulate_feathered  sucre_mosaic_accumulate with, in float32, one IEEE operation per step,
 *                         f = dist2 >= F^2 ? 1 : sqrtf((float)dist2) inv_F (inv_F = 1.0f / (float)F) and
 *                         wq = (int)rintf(((t t) f) 4096), 0..4096; everything else as there, flags included.  The images are
 *                         those of the sucre_mosaic_feather call that wrote feather_dev, in the same order, with this F or a
 *                         larger one (dist2 = min(D2, F'^2) with F' >= F gives the same dist2 >= F^2 and the same root below it).
 *                         A cell's winner has wq >= 4 (f >= 1/1024), so a filled cell has wsum >= 4 and a count >= 1; with
 *                         F = 1 the words equal sucre_mosaic_accumulate's to the bit (every member has dist2 >= 1 = F^2).
 * Checked before any launch as above, and: feather_px outside 1..1024, a NULL or misaligned feather_dev.
 *
 * The bands: a multi-band blend.  Every image is split, in source space, into K detail bands D_0 .. D_(K-1) and a residual S_K,
 * K in 1..SUCRE_MOSAIC_BANDS_MAX = 6; the caller accumulates every band with sucre_mosaic_accumulate(_feathered) -- the band as the
 * images' J, signed values included -- into an accumulator of its own, the finer the band the smaller its blend depth, and one
 * pass over the cells adds the blended bands.  The members of an image are the pixels that take part.  Float32, one IEEE
 * operation per step:
 *   S_0 = min(max(J, -1024), 1024) at members (the accumulate's clamp; an infinity becomes finite)
 *   level j -> j+1, s = 2^j, with a(u,v) = S_j at a member and +0.0f elsewhere and outside the image, m the same with 1 and 0:
 *     Nh(u,v) = (a(u-s,v) + 2 a(u,v)) + a(u+s,v),  N(u,v) = (Nh(u,v-s) + 2 Nh(u,v)) + Nh(u,v+s);  Ah, A likewise in integers (A: 0..16)
 *     S_(j+1) = N / (float)A (a member has A >= 4);  D_j = S_j - S_(j+1)
 *   at a non-member every S and D is the NaN 0x7fc00000 in all three channels: the members of every band are the members of J.
 *   sucre_mosaic_band_bytes  the bytes of ONE band buffer for these images (only H and W are read; 0 and an error for bad sizes):
 *                         image i's (H,W,3) float32 block starts at PIXEL 256 sum_(j<i) ceil(H_j W_j / 256), 12 bytes per pixel
 *                         (the feather map's placement); the pixels between two images are not written
 *   sucre_mosaic_band_split  one level: writes S_(level+1) to S_out and D_level to D_out.  level = 0: S_in is NULL and the images'
 *                         depth and J are read; level >= 1: S_in is the S_out of the level before (a NaN marks a non-member;
 *                         depth and J are not read).  S_in, S_out and D_out are three buffers of sucre_mosaic_band_bytes that do
 *                         not overlap.  One launch per 32 images (plus the table's); only enqueues: nothing is allocated, nothing
 *                         copied from the host
 *   sucre_mosaic_band_combine  acc_bands_dev: n_bands = K + 1 accumulators of sucre_mosaic_accumulate's layout, (n_bands, Hm Wm, 8)
 *                         int64, band j at slice j and the residual last.  One pass over the cells, no image read; for a cell
 *                         whose residual has word 7 > 0: B_j = (float)(((double)acc_j,c / (double)wsum_j) 2^-20), the quotient of
 *                         sucre_mosaic_normalize, and J_out (Hm,Wm,3) float32 = (..((B_K + B_(K-1)) + B_(K-2)) ..) + B_0, coarse
 *                         to fine.  Empty cells are not touched.  Every filled cell has wsum_j >= 4 in every band: its winner
 *                         has d = 0, so t = 1 whatever the band's blend depth, and f >= 1/1024.
 * Checked before any launch as above, and: level outside 0..5, S_in given at level 0 or NULL above it, a NULL or misaligned S_out
 * or D_out, buffers that overlap, n_bands outside 2..7, a NULL or misaligned acc_bands_dev or J_out, Hm Wm above 2^39.
 *
 * The surface test: a per-cell top height along e3 (row 2 of the axes; it looks the way the cameras look, so smaller is higher),
 * and the samples too far below it taken out of every later phase.  For a pixel that takes part and has a cell, a_n = dot3(e3, wP)
 * with the wP its plane coordinates are formed from; top[cell] is the smallest a_n of the cell, kept as the order-preserving
 * uint32 image of its bits (k = bits ^ 0x80000000 for a_n >= +0, ~bits below; -0.0 lies below +0.0; all ones: empty).
 *   sucre_mosaic_surface  top_dev[cell] (uint32) = min k over the pixels of the cell; the caller starts it at all ones.  One pass
 *                         over ALL images, any split into calls, before sucre_mosaic_cull.  flags: SUCRE_MOSAIC_PLAIN_ATOMIC --
 *                         the atomic min for every pixel instead of loading the word first (the same top_dev)
 *   sucre_mosaic_cull     J_out: a buffer of sucre_mosaic_band_bytes for these images, in that layout.  A pixel that takes part and
 *                         is not culled -- culled: it has a cell, the cell's top is not all ones and a_n - top > tol, one float32
 *                         subtraction and one comparison -- gets its J copied bit for bit; every other pixel of an image gets
 *                         the NaN 0x7fc00000 in all three channels; the pixels between two images are not written.  The caller
 *                         hands the other entries J_out's blocks as the images' J: a culled pixel takes part in nothing.
 *                         culled_dev (uint32 per cell, or NULL): a culled sample adds 1 to its cell.  counts_dev (uint64 x 2, or
 *                         NULL): adds the culled samples and the samples with a cell.  Only enqueues
 * Checked before any launch as above, and: a NULL or misaligned top_dev or J_out, a misaligned culled_dev or counts_dev, tol not
 * finite or <= 0, a J_out that overlaps an image's J, unknown flags.
 *
 * The supported surface (csrc/support.h): the top above is a plain minimum, so one spurious high sample owns its cell.  Here the top
 * of a cell is the highest level that at least M different images reach.  key64 = (uint64)k << 32 | ordinal, k as above; level 0 of
 * a cell is the smallest key64 of its samples, level r the smallest among the samples whose ordinal is not the low word of one of
 * its levels 0..r-1 (a view listed twice has two ordinals and counts twice; a height tie goes to the earlier image); a level that
 * finds no sample stays all ones.  With n the levels of a cell that hold something and m = min(n_levels, n): top = the high word
 * of level m-1 (all ones for n = 0), support = n, source = the low word of level m-1 (-1 for n = 0): a cell that fewer than
 * n_levels images see rests on the lowest of its per-image tops.
 *   sucre_mosaic_support         level `level` of rank_dev ((n_levels, Hm Wm) uint64; the caller starts it at all ones): one pass
 *                                over ALL images, any split into calls, after level - 1 has seen them all.  flags:
 *                                SUCRE_MOSAIC_PLAIN_ATOMIC -- the atomic min for every pixel (the same rank_dev)
 *   sucre_mosaic_support_top     top_dev (uint32, the key format of sucre_mosaic_surface), support_out and source_out (int32, or
 *                                NULL) of every cell from its n_levels words; reads no image
 *   sucre_mosaic_cull_supported  sucre_mosaic_cull with a second side: with d = a_n - top (one float32 subtraction) a sample is
 *                                culled below when d > tol and above when d < -tol; J_out as there.  culled_dev counts the
 *                                samples culled below per cell, culled_above_dev those culled above (uint32, or NULL);
 *                                counts_dev (uint64 x 3, or NULL): culled below, culled above, samples with a cell
 * All three only enqueue.  Checked before any launch as above, and: n_levels outside 1..SUCRE_MOSAIC_SUPPORT_MAX, level outside
 * 0..n_levels-1, a NULL or misaligned rank_dev or top_dev, misaligned support_out, source_out, culled_above_dev, Hm Wm above 2^39.
 *
 * Per-image gain compensation (csrc/gains_mosaic.h): one gain per image and channel from the cells that two or more images share,
 * by rounds of exact block-coordinate descent on sum (g_i J - m_cell)^2; the host solves between the passes.  The images' J are
 * those the phases after the surface test see.  gains_dev: (n_ordinals, 3) float32, row = ordinal; sums_dev: (n_ordinals, 16) int64,
 * row = ordinal, SUCRE_MOSAIC_GAIN_WORDS = 10 words used (rows padded to 128 bytes); the caller starts the sums at zero.
 *   sucre_mosaic_gain_span   span_dev ((Hm Wm, 2) uint32; the caller starts every pair at all ones, 0): per cell the min and the max of
 *                            the ordinals of the pixels that take part and have a cell; a cell is SHARED when min < max.  Once,
 *                            over ALL images, any split into calls.  flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- both atomics for every
 *                            pixel instead of loading the words first (the same span_dev)
 *   sucre_mosaic_gain_apply  J_out (sucre_mosaic_band_bytes for these images, that layout): J_c x gains[ordinal][c], one float32
 *                            multiply, for every pixel of every image; a NaN stays a NaN.  An image's J may be its own block of
 *                            J_out; it may not overlap J_out otherwise
 *   sucre_mosaic_gain_sums   acc_dev: an accumulator of sucre_mosaic_accumulate over the gained images with inv_h = 0x1p-126f (every
 *                            wq = 4096: the per-sample mean), complete for ALL images.  For a pixel that takes part, whose cell is
 *                            shared, with q(x) = (int64)rintf(fminf(fmaxf(x, -8), 8) 16384), m_c = the quotient of
 *                            sucre_mosaic_normalize of words c and 6: Xq = q(J_c), Mq = q(m_c), Rq = q(J_c gains[ordinal][c]) - Mq,
 *                            and the image's row takes 1, Xq Mq x 3, Xq Xq x 3, Rq Rq x 3 (integer adds: any order, the same words).
 *                            flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- ten atomics per 256 pixels instead of ten per 8192 of an image
 * All three only enqueue.  Checked before any launch as above, and: a NULL or misaligned span_dev (8 bytes), gains_dev, J_out, acc_dev
 * or sums_dev (128 bytes), n_ordinals outside 1..4096 or below first_ordinal + n_images, an image of more than 2^26 pixels (its sums
 * could pass 2^62), a J_out that overlaps an image's J without being it, unknown flags.
 *
 * The direct solve of the gain compensation (csrc/gains_direct.h): the rounds' objective solved exactly, once.  Integer state only.
 * slot_ord_dev: (Hm Wm, SUCRE_MOSAIC_GAIN_SLOTS = 8) uint32, the caller starts every word at all ones (free); slot_sum_dev:
 * (Hm Wm, 8, 4) int64 -- n, sum Xq x 3 --, slot_over_dev: (Hm Wm) uint32, pairs_dev: (n_ordinals, n_ordinals, 4) int64, diag_dev:
 * (n_ordinals, 16) int64, 4 words used; the caller starts all of these at zero.
 *   sucre_mosaic_gain_slots  after the span, over ALL images, any split into calls: a sample of a shared cell takes the cell's slot
 *                            that holds its ordinal, or claims the first free one, and adds 1 and Xq_c = q(J_c); a sample that finds
 *                            all eight held by other images sets slot_over[cell] = 1.  Which slot an image holds depends on
 *                            arrival (sort a cell's slots by ordinal); the slots of a cell with slot_over set hold nothing to read.
 *                            flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- every sample for itself, without the run sums of a wave's lanes
 *   sucre_mosaic_gain_pairs  once, after the slots: for every shared cell with slot_over 0, N = sum n_a, and for every pair of held
 *                            slots a <= b with i = min, j = max of their ordinals: pairs[i][j][c] += llrint(((double)S_a,c
 *                            (double)S_b,c) / (double)N) for c in 0..2, pairs[i][j][3] += 1.  table_entries: the size of a
 *                            workgroup's LDS table of pair sums, a power of two up to 512, 0 for 512 (any size: the same words).
 *                            flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- global atomics per cell and pair, no table
 *   sucre_mosaic_gain_diag   after the slots, over ALL images: the image's row takes 1 and Xq Xq x 3 for every sample in a shared
 *                            cell with slot_over 0.  flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- four atomics per 256 pixels
 * All three only enqueue.  Checked before any launch as above, and: a NULL or misaligned span_dev (8 bytes), slot_ord_dev (4),
 * slot_sum_dev (8), slot_over_dev (4), pairs_dev (8) or diag_dev (128), n_ordinals outside 1..4096, a table_entries that is no such
 * power of two, a grid of 2^43 cells or more (pairs: its workgroups of 4096 cells must fit a launch), an image of more than 2^26
 * pixels (diag), unknown flags.
 *
 * The colour consensus across views (csrc/reject.h): the samples whose colour differs from what the median image of their cell saw,
 * taken out ahead of the splat.  Integer state, or one IEEE operation per step: the same bits in any order, split and atomic form.
 * slot_ord_dev: (Hm Wm, SUCRE_MOSAIC_REJECT_SLOTS = 8) uint32, the caller starts every word at all ones (free); slot_over_dev:
 * (Hm Wm) uint32 and slot_sum_dev: (Hm Wm, 8, 4) int64 -- n, sum Xq x 3 --, both started at zero.
 *   sucre_mosaic_reject_claim      over ALL images, any split into calls: afterwards a cell's words hold the 8 smallest distinct
 *                                  ordinals that reach it, ascending, free words last (a chain of atomic minima that carries the
 *                                  displaced value on), and slot_over[cell] = 1 exactly when a ninth reaches it.
 *                                  flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- every sample walks the whole chain, without the load of the
 *                                  cell's words ahead of it and without the runs of a wave's lanes
 *   sucre_mosaic_reject_sums       after the claim has seen ALL images, over ALL images: a sample whose ordinal is one of its
 *                                  cell's eight adds 1 and Xq_c = q(J_c) to that slot; any other sample adds nothing.
 *                                  flags: SUCRE_MOSAIC_PLAIN_ATOMIC -- every sample for itself, without the run sums
 *   sucre_mosaic_reject_consensus  once, after the sums: per cell views_out = k, the occupied slots; with k >= SUCRE_MOSAIC_REJECT_
 *                                  MIN_VIEWS = 3 the slots are ordered by Y / n (Y = S_0 + S_1 + S_2; exactly, Y_a n_b < Y_b n_a,
 *                                  ties by ordinal), the slot at index (k - 1) / 2 is the reference: source_out its ordinal,
 *                                  ref_out[c] = (float)(((double)S_c / (double)n) 2^-14); otherwise source_out -1 and ref_out NaN.
 *                                  big_dev (one uint64, started at zero): the slots with n >= 2^20, whose cells get no reference --
 *                                  a caller stops on a count above 0
 *   sucre_mosaic_reject_cull       sucre_mosaic_cull with the colour test: J_out gets NaN in every channel of a pixel that does not
 *                                  take part, or whose cell has a reference, whose ordinal is not source[cell] and for which
 *                                  fabsf(J_c - ref_c) > tol in any channel.  rejected_dev (uint32 per cell, or NULL): the rejected
 *                                  samples per cell; counts_dev ((n_ordinals, 16) int64, two words used, or NULL): per image the
 *                                  samples in cells that have a reference and the samples rejected
 * All four only enqueue.  Checked before any launch as above, and: a NULL or misaligned slot_ord_dev (32 bytes), slot_over_dev (4),
 * slot_sum_dev (8), ref_dev / ref_out (4), source (4), views_out (4) or big_dev (8), a misaligned rejected_dev (4) or counts_dev
 * (128), n_ordinals outside 1..4096 or below first_ordinal + n_images when counts_dev is given, a tol that is not finite and > 0, a
 * J_out that overlaps an image's J, a grid of more than 2^39 cells (consensus), unknown flags.
 */
#define SUCRE_MOSAIC_PLAIN_ATOMIC 1u
#define SUCRE_MOSAIC_GAIN_WORDS 10
#define SUCRE_MOSAIC_GAIN_SLOTS 8
#define SUCRE_MOSAIC_REJECT_SLOTS 8
#define SUCRE_MOSAIC_REJECT_MIN_VIEWS 3
#define SUCRE_MOSAIC_SUPPORT_MAX 4
#define SUCRE_MOSAIC_ACC_WORDS 8
#define SUCRE_MOSAIC_FEATHER_MAX 1024
#define SUCRE_MOSAIC_BANDS_MAX 6
typedef struct sucre_mosaic_image {
    const float *depth;   /* (H,W) float32 */
    const uint8_t *rgb;   /* (H,W,3) uint8 */
    const float *J;       /* (H,W,3) float32 */
    int32_t H, W;
    float Kinv[9], R[9], t[3];
    int32_t reserved[3];
} sucre_mosaic_image_t;
typedef struct sucre_mosaic_grid {
    float axes[9];        /* rows e1, e2, e3 */
    float gsd, lo_s, lo_t;
    int32_t Hm, Wm;
} sucre_mosaic_grid_t;
size_t sucre_mosaic_table_bytes(int n_images);
int sucre_mosaic_bounds(void *table_dev, int n_images, const sucre_mosaic_image_t *images, const float *axes, uint32_t *bounds_dev,
                        void *stream);
int sucre_mosaic_splat(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                       const sucre_mosaic_grid_t *grid, uint64_t *key_dev, unsigned flags, void *stream);
int sucre_mosaic_resolve(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, uint32_t *pix_dev, void *stream);
int sucre_mosaic_gather(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                        const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, const uint32_t *pix_dev, float *J_out,
                        uint8_t *raw_out, int32_t *source_out, int32_t *pixel_out, float *range_out, void *stream);
int sucre_mosaic_accumulate(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                            const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, float inv_h, int64_t *acc_dev, unsigned flags,
                            void *stream);
int sucre_mosaic_normalize(const sucre_mosaic_grid_t *grid, const int64_t *acc_dev, float *J_out, uint8_t *raw_out, float *weight_out,
                           int32_t *samples_out, void *stream);
size_t sucre_mosaic_feather_bytes(int n_images, const sucre_mosaic_image_t *images);
int sucre_mosaic_feather(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int feather_px, void *feather_dev,
                         void *stream);
int sucre_mosaic_accumulate_feathered(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                      const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, float inv_h, int feather_px,
                                      const void *feather_dev, int64_t *acc_dev, unsigned flags, void *stream);
size_t sucre_mosaic_band_bytes(int n_images, const sucre_mosaic_image_t *images);
int sucre_mosaic_band_split(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int level, const float *S_in, float *S_out,
                            float *D_out, void *stream);
int sucre_mosaic_band_combine(const sucre_mosaic_grid_t *grid, int n_bands, const int64_t *acc_bands_dev, float *J_out, void *stream);
int sucre_mosaic_surface(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, uint32_t *top_dev, unsigned flags, void *stream);
int sucre_mosaic_cull(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                      const sucre_mosaic_grid_t *grid, const uint32_t *top_dev, float tol, float *J_out, uint32_t *culled_dev,
                      uint64_t *counts_dev, void *stream);
int sucre_mosaic_support(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, int n_levels, int level, uint64_t *rank_dev, unsigned flags, void *stream);
int sucre_mosaic_support_top(const sucre_mosaic_grid_t *grid, int n_levels, const uint64_t *rank_dev, uint32_t *top_dev,
                             int32_t *support_out, int32_t *source_out, void *stream);
int sucre_mosaic_cull_supported(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                const sucre_mosaic_grid_t *grid, const uint32_t *top_dev, float tol, float *J_out,
                                uint32_t *culled_dev, uint32_t *culled_above_dev, uint64_t *counts_dev, void *stream);
int sucre_mosaic_gain_span(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, uint32_t *span_dev, unsigned flags, void *stream);
int sucre_mosaic_gain_apply(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const float *gains_dev,
                            int n_ordinals, float *J_out, void *stream);
int sucre_mosaic_gain_sums(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const int64_t *acc_dev, const float *gains_dev,
                           int n_ordinals, int64_t *sums_dev, unsigned flags, void *stream);
int sucre_mosaic_gain_slots(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                            const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, uint32_t *slot_ord_dev, int64_t *slot_sum_dev,
                            uint32_t *slot_over_dev, unsigned flags, void *stream);
int sucre_mosaic_gain_pairs(const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const uint32_t *slot_ord_dev,
                            const int64_t *slot_sum_dev, const uint32_t *slot_over_dev, int n_ordinals, int64_t *pairs_dev, int table_entries,
                            unsigned flags, void *stream);
int sucre_mosaic_gain_diag(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const uint32_t *slot_over_dev, int n_ordinals,
                           int64_t *diag_dev, unsigned flags, void *stream);
int sucre_mosaic_reject_claim(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                              const sucre_mosaic_grid_t *grid, uint32_t *slot_ord_dev, uint32_t *slot_over_dev, unsigned flags,
                              void *stream);
int sucre_mosaic_reject_sums(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                             const sucre_mosaic_grid_t *grid, const uint32_t *slot_ord_dev, int64_t *slot_sum_dev, unsigned flags,
                             void *stream);
int sucre_mosaic_reject_consensus(const sucre_mosaic_grid_t *grid, const uint32_t *slot_ord_dev, const int64_t *slot_sum_dev,
                                  float *ref_out, int32_t *source_out, int32_t *views_out, uint64_t *big_dev, void *stream);
int sucre_mosaic_reject_cull(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                             const sucre_mosaic_grid_t *grid, const float *ref_dev, const int32_t *source_dev, float tol, float *J_out,
                             uint32_t *rejected_dev, int n_ordinals, int64_t *counts_dev, void *stream);

/*
 * ---- hole filling of the finished mosaic: a bounded push-pull over a pyramid of the grid ------------------------------------------
 * A pure grid operation on the outputs of sucre_mosaic_gather (or of sucre_mosaic_normalize with the same source): no image is
 * read, no atomic issued, every number is a fixed chain of float32 operations, one IEEE operation per step -- the same bits on
 * every run.  Level 0 is the mosaic (Hm x Wm), level l+1 has ((H_l + 1) >> 1) x ((W_l + 1) >> 1) cells; `levels` = L in 1..24.  A
 * record is 8 float32 (32 bytes): c[0..2] for J, c[3..5] for the raw colour as float, w, g.  Level 0 is read in place: a cell is
 * valid (w = 1, c its J and raw values) when source >= 0 and its three J channels are finite, otherwise w = 0 and every c counts
 * as +0.0f.
 *   sucre_mosaic_fill_bytes  the bytes of levels 1..L, each level row-major and 256-byte aligned (0 and an error for bad sizes)
 *   sucre_mosaic_fill_pull   levels 1..L, one launch each: with the children (2y+dy, 2x+dx) in the order (0,0), (0,1), (1,0), (1,1),
 *                         one outside the level a record of zeros, Wt = ((w0 + w1) + w2) + w3 and S_k = ((w0 c0_k + w1 c1_k) +
 *                         w2 c2_k) + w3 c3_k, every product rounded before its add.  Wt > 0: c_k = S_k / Wt, w = Wt 0.25f,
 *                         g = l+1; otherwise the record is all +0.0f.  Every record of the pyramid is written.
 *   sucre_mosaic_fill_push   l = L-1 .. 0, one launch each, in place: a cell with w > 0 is untouched; for a cell (y, x) with
 *                         w == 0, py = y >> 1, ny = clamp(py + (y & 1 ? 1 : -1), 0, H_(l+1) - 1), px and nx likewise, the taps
 *                         (py,px), (py,nx), (ny,px), (ny,nx) of level l+1 have a_i = 9/16, 3/16, 3/16, 1/16 where the tap's w > 0 and
 *                         0 elsewhere; A and S_k are summed as Wt and S_k above.  A > 0: c_k = S_k / A, w = 1, g = the largest g of
 *                         the taps with a_i > 0; otherwise the cell stays empty.  Level 0 writes, for EVERY cell: J_filled
 *                         (Hm,Wm,3) float32 -- a measured cell (source >= 0) its J bit for bit, finite or not, a filled cell
 *                         c[0..2], an unfilled one the NaN 0x7fc00000 --, raw_filled (Hm,Wm,3) uint8 -- raw, (uint8)rintf(min(max(
 *                         c[3+k], 0), 255)), 0 -- and level_out (Hm,Wm) int32 -- 0, g in 1..L, -1.
 * Every empty cell within 2^(L-1) cells (Chebyshev) of a valid cell is filled; none at 3 x 2^L cells or more from every valid one.
 * Push comes after pull with the same sizes, inputs and pyramid.  Checked before any launch (SUCRE_ERR_ARG): Hm or Wm outside
 * 1..2^24, Hm Wm above 2^39, levels outside 1..24, a NULL pointer, J / source / J_filled / level_out not 4-byte aligned, pyramid_dev
 * not 256-byte aligned.
 */
size_t sucre_mosaic_fill_bytes(int Hm, int Wm, int levels);
int sucre_mosaic_fill_pull(int Hm, int Wm, int levels, const float *J, const uint8_t *raw, const int32_t *source, void *pyramid_dev,
                           void *stream);
int sucre_mosaic_fill_push(int Hm, int Wm, int levels, const float *J, const uint8_t *raw, const int32_t *source, void *pyramid_dev,
                           float *J_filled, uint8_t *raw_filled, int32_t *level_out, void *stream);

/*
 * Shared water AND light over several light-model images (the group above for the 19-parameter model; sucre.py:54-61 with
 * the objective of sucre.py:124-157 summed over the images: one B, beta, gamma, cam2light, sigma, every image its own J, one
 * n_obs).  `group_dev`: sucre_light_group_bytes(n_images) bytes of device memory, 256-byte aligned; `images` (host array)
 * names every image's matched, finalised (f32 store, camera points only) and fit_init_light-ed workspaces; images may differ
 * in size and view count.  sucre_light_group_init sets the shared parameters from params0 (19 host floats; the reference
 * starts from 0.1 x 9, 0 x 6 and identity) and keeps a host copy of the table, keyed by group_dev, until the next init there.
 * sucre_light_group_iter(step), step = 1, 2, ... in order (SUCRE_ERR_RANGE otherwise): takes the Adam step the sums left by
 * the previous call -- all-reduced over the ranks by the host in between -- call for (trace row step-2 of trace_dev, T x 20
 * float64, nullable: cost, then the 19 parameters after the step), then runs every image's gradient pass on the shared
 * parameters (J steps and closed-form solves stay per image, scaled by n_obs_total, the observations of all images of all
 * ranks) and leaves this rank's 19 float64 sums at sucre_light_group_sums_offset(), the images added in table order.
 * sucre_light_group_finish(step) takes the last step, copies the final parameters into every image's `lws`
 * (sucre_light_params_offset) and, with SUCRE_FIT_CLOSED_FORM, solves every image's final J (sucre.py:155-156).
 * flags: SUCRE_FIT_CLOSED_FORM only (float32 colours, SUCRE_FIT_EXT_*, and other stores are refused).
 */
typedef struct sucre_light_group_image {
    void *ws;              /* the image's workspace */
    void *lws;             /* its light workspace (sucre_light_workspace_bytes) */
    int32_t H, W, n_views; /* its geometry */
    int32_t reserved;
} sucre_light_group_image_t;
size_t sucre_light_group_bytes(int n_images);
int64_t sucre_light_group_sums_offset(void);
int sucre_light_group_init(void *group_dev, int n_images, const sucre_light_group_image_t *images, const float *params0,
                           void *stream);
int sucre_light_group_iter(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                           unsigned flags, uint64_t n_obs_total, double *trace_dev, void *stream);
int sucre_light_group_finish(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                             unsigned flags, uint64_t n_obs_total, double *trace_dev, void *stream);

/*
 * ---- standard errors of the water parameters and of J --------------------------------------------------------------------
 * How well the observations determine what the fit reports: one float64 streaming pass over the DENSE store of a matched (or
 * imported), finalised and fitted workspace that forms, for every observation of every KEPT view at the workspace's CURRENT
 * parameters and CURRENT J (as sucre_fit_residuals* reads them), per channel c -- channels do not couple --
 *     a = exp(-beta z),  g = exp(-gamma z)                                      SUCRe.forward, sucre.py:79-82; z: sucre.py:52-53
 *     dJ = a,  dB = 1 - g,  dbeta = -J z a,  dgamma = B z g,  r = I - (J a + B dB)       the Jacobian of sucre.py:144's residual
 * and sums the Gauss-Newton normal equations with every pixel's own J eliminated:
 *     per pixel p:  A_p = sum dJ^2,  b_p = sum dJ (dB, dbeta, dgamma),  k_p = b_p / A_p
 *     H = sum_obs d d^T - sum_p b_p b_p^T / A_p   with d = (dB, dbeta, dgamma),   SSR = sum r^2
 * from which  s^2 = SSR / (N - P - 3),  cov(B, beta, gamma) = s^2 H^-1  and  sigma_J(p)^2 = s^2 (1 / A_p + k_p^T H^-1 k_p)
 * follow on the host.  z, J, B, beta, gamma and I are the float32 numbers of the residual pass (with SUCRE_OBS_U16MM the range
 * 0.001f * clamp(rint(1000 z), 1, 65535); uint8 colours as float32(k / 255)) promoted to float64; everything behind is float64,
 * one IEEE operation per step: the elimination is a 30-65x cancellation in a matrix of scaled condition number 1e3 - 3e4, and
 * float32 sums leave H wrong by 5e-4 - 9e-4 relative.
 *   count_dev   int32   (H,W)       observations of the pixel over the kept views
 *   jterms_dev  float32 (H,W,3,4)   per channel {1 / A_p, k_B, k_beta, k_gamma}; 0 where count is 0
 *   sums_dev    float64 [SUCRE_UNCERTAINTY_WORDS]
 *                 word 0  N, the observations           word 1  P, the pixels with at least one
 *                 word 2  pixels that have observations but no finite positive A_p in some channel: nothing is eliminated for
 *                         them and their jterms are 0 (their observations still stand in N, SSR and sum d d^T, so a caller
 *                         must not trust the sums of an image where this word is not 0)
 *                 words 3 + 7 c ..: H_BB, H_Bbeta, H_Bgamma, H_betabeta, H_betagamma, H_gammagamma, SSR of channel c
 * The workspaces are only read.  scratch_dev: sucre_uncertainty_scratch_bytes() bytes of caller-owned device memory, 16-byte
 * aligned, that must stay untouched until the pass has run; every sum is formed in a fixed order (no atomics), so two calls
 * give the same bits.  obs_format: as for sucre_fit_residuals.  sucre_fit_uncertainty_ext: the same for a workspace with
 * float32 colours, flags = SUCRE_FIT_EXT_COLOUR (the nine parameters are the first nine of `lws`).  The light model is not
 * built: flags = 0 and SUCRE_FIT_EXT_BOTH are refused -- the lamp's ten parameters would have to join (B, beta, gamma), and
 * errors conditional on a fixed lamp would understate.  Arguments are checked before anything is launched: NULL or misaligned
 * pointers, a bad geometry, an unknown format or such flags give SUCRE_ERR_ARG and a message that names the reason.
 * Limits: Gauss-Newton at the current point, not necessarily at the minimum; observations are taken as independent with one
 * variance per channel, so errors shared by views (depth maps, poses) are not in it.
 */
#define SUCRE_UNCERTAINTY_WORDS 24
size_t sucre_uncertainty_scratch_bytes(int H, int W, int n_views);
int sucre_fit_uncertainty(const void *ws, int H, int W, int n_views, int obs_format, int32_t *count_dev, float *jterms_dev,
                          double *sums_dev, void *scratch_dev, void *stream);
int sucre_fit_uncertainty_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags /* SUCRE_FIT_EXT_COLOUR */,
                              int32_t *count_dev, float *jterms_dev, double *sums_dev, void *scratch_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SUCRE_HIP_H */
