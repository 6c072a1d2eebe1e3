// extern "C" surface of libsucre_hip.so (include/sucre_hip.h): argument validation, error strings, launch order.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "consist.h"
#include "fill.h"
#include "invert.h"
#include "launch.h"
#include "mosaic.h"
#include "bands.h"
#include "pool.h"
#include "surface.h"
#include "support.h"
#include "gains_mosaic.h"
#include "gains_direct.h"
#include "reject.h"

namespace sucre {

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return SUCRE_OK;
    return fail(SUCRE_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

static bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

static int check_ws(const void *ws, int H, int W, int n_views, Layout *L) {
    if (!make_layout(H, W, n_views, L))
        return fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d (need 1..32767, 1..%d views)", H, W, n_views,
                    kMaxViews);
    if (!ws) return fail(SUCRE_ERR_ARG, "workspace is NULL");
    if (!aligned(ws, 256)) return fail(SUCRE_ERR_ARG, "workspace must be 256-byte aligned");
    return SUCRE_OK;
}

// torch/optim/adam.py: bias_correction1 = 1 - beta1 ** step; step_size = lr / bias_correction1;
// bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5  -- Python floats (double), cast to float32 at use.
AdamCoef adam_coef(int step, double lr, double beta1, double beta2, double eps) {
    AdamCoef c;
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    c.w1 = (float)(1.0 - beta1);
    c.beta2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.step_size_neg = (float)(-(lr / bc1));
    c.bc2_sqrt = (float)std::sqrt(bc2);
    c.eps = (float)eps;
    return c;
}

static int check_adam(int step, double lr, double beta1, double beta2, double eps) {
    if (step < 1) return fail(SUCRE_ERR_RANGE, "Adam step must be >= 1 (got %d)", step);
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return fail(SUCRE_ERR_ARG, "invalid Adam hyper-parameters lr=%g betas=(%g,%g) eps=%g", lr, beta1, beta2, eps);
    return SUCRE_OK;
}

}  // namespace sucre

using namespace sucre;

extern "C" {

int sucre_version(void) { return SUCRE_ABI_VERSION; }

const char *sucre_last_error(void) { return g_err; }

size_t sucre_workspace_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) {
        fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
        return 0;
    }
    return L.total;
}

int64_t sucre_ws_offset(int H, int W, int n_views, int region) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) return fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
    switch (region) {
        case SUCRE_WS_VIEW_COUNT: return (int64_t)L.off_view_count;
        case SUCRE_WS_VIEW_KEEP: return (int64_t)L.off_view_keep;
        case SUCRE_WS_N_OBS: return (int64_t)L.off_n_obs;
        case SUCRE_WS_PARAMS: return (int64_t)L.off_params;
        case SUCRE_WS_SUMS: return (int64_t)L.off_sums;
        case SUCRE_WS_N_OBS_TOTAL: return (int64_t)L.off_n_obs_total;
        case SUCRE_WS_STORE_FORMAT: return (int64_t)off_store_format(L);
        case SUCRE_WS_STATE: return (int64_t)L.off_state;
        case SUCRE_WS_PAIR_GRADIENT: return (int64_t)L.off_gplane;
        default: return fail(SUCRE_ERR_RANGE, "unknown workspace region %d", region);
    }
}

int sucre_match_views(void *ws, int H, int W, int n_views, const sucre_view_t *target,
                      const sucre_view_t *views_dev, int k0, int k1, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (!target || !views_dev) return fail(SUCRE_ERR_ARG, "target / views_dev is NULL");
    if (!target->depth) return fail(SUCRE_ERR_ARG, "target depth map is NULL");
    if (target->H != H || target->W != W)
        return fail(SUCRE_ERR_ARG, "target is %dx%d but the workspace is laid out for %dx%d", target->W, target->H, W, H);
    if (!aligned(views_dev, 8)) return fail(SUCRE_ERR_ARG, "views_dev must be 8-byte aligned");
    if (k0 < 0 || k1 > n_views || k0 >= k1) return fail(SUCRE_ERR_RANGE, "view range [%d,%d) outside [0,%d)", k0, k1, n_views);
    return check_hip(launch_match(L, static_cast<uint8_t *>(ws), *target, views_dev, k0, k1,
                                  static_cast<hipStream_t>(stream)), "sucre_match_views");
}

int sucre_match_map(int H, int W, int n_views, const sucre_view_t *target, const sucre_view_t *views_dev, int k,
                    int32_t *map_dev, void *stream) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) return fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
    if (!target || !views_dev || !map_dev) return fail(SUCRE_ERR_ARG, "target / views_dev / map_dev is NULL");
    if (!target->depth) return fail(SUCRE_ERR_ARG, "target depth map is NULL");
    if (target->H != H || target->W != W) return fail(SUCRE_ERR_ARG, "target is %dx%d, expected %dx%d", target->W, target->H, W, H);
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    return check_hip(launch_match_map(L, *target, views_dev, k, map_dev, static_cast<hipStream_t>(stream)), "sucre_match_map");
}

int sucre_pack_view(const float *depth_dev, const uint8_t *rgb_dev, int H, int W, void *packed_dev, void *stream) {
    if (H <= 0 || W <= 0 || H > 32767 || W > 32767) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d", W, H);
    if (!depth_dev || !rgb_dev || !packed_dev) return fail(SUCRE_ERR_ARG, "depth_dev / rgb_dev / packed_dev is NULL");
    if (!aligned(packed_dev, 8)) return fail(SUCRE_ERR_ARG, "packed_dev must be 8-byte aligned");
    return check_hip(launch_pack_view(depth_dev, rgb_dev, H, W, packed_dev, static_cast<hipStream_t>(stream)), "sucre_pack_view");
}

int sucre_pack_views(const float *const *depth_dev, const uint8_t *const *rgb_dev, void *const *packed_dev, int n, int H, int W,
                     void *stream) {
    if (H <= 0 || W <= 0 || H > 32767 || W > 32767) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d", W, H);
    if (n < 0) return fail(SUCRE_ERR_RANGE, "negative view count %d", n);
    if (n == 0) return SUCRE_OK;
    if (!depth_dev || !rgb_dev || !packed_dev) return fail(SUCRE_ERR_ARG, "depth_dev / rgb_dev / packed_dev is NULL");
    for (int k = 0; k < n; ++k) {
        if (!depth_dev[k] || !rgb_dev[k] || !packed_dev[k]) return fail(SUCRE_ERR_ARG, "view %d: depth / rgb / packed pointer is NULL", k);
        if (!aligned(packed_dev[k], 8)) return fail(SUCRE_ERR_ARG, "view %d: packed_dev must be 8-byte aligned", k);
    }
    return check_hip(launch_pack_views(depth_dev, rgb_dev, packed_dev, n, H, W, static_cast<hipStream_t>(stream)), "sucre_pack_views");
}

int sucre_project_points(const sucre_view_t *view, const float *wP_dev, int64_t n, int32_t *pix_dev, void *stream) {
    if (!view) return fail(SUCRE_ERR_ARG, "view is NULL");
    if (view->H <= 0 || view->W <= 0 || view->H > 32767 || view->W > 32767)
        return fail(SUCRE_ERR_ARG, "invalid sensor size %dx%d", view->W, view->H);
    if (n < 0) return fail(SUCRE_ERR_RANGE, "negative point count %lld", (long long)n);
    if (n == 0) return SUCRE_OK;   // nothing to launch
    if (!wP_dev || !pix_dev) return fail(SUCRE_ERR_ARG, "wP_dev / pix_dev is NULL");
    return check_hip(launch_project_points(*view, wP_dev, (long long)n, pix_dev, static_cast<hipStream_t>(stream)),
                     "sucre_project_points");
}

int sucre_import_view(void *ws, int H, int W, int n_views, int k, const int16_t *u1_dev, const int16_t *v1_dev,
                      const float *z_dev, const uint8_t *rgb_dev, int64_t n, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    if (n < 0) return fail(SUCRE_ERR_RANGE, "negative observation count %lld", (long long)n);
    if (n > 0 && (!u1_dev || !v1_dev || !z_dev || !rgb_dev)) return fail(SUCRE_ERR_ARG, "NULL match list");
    return check_hip(launch_import_view(L, static_cast<uint8_t *>(ws), k, u1_dev, v1_dev, z_dev, rgb_dev, (long long)n,
                                        static_cast<hipStream_t>(stream)), "sucre_import_view");
}

int sucre_finalize_matches(void *ws, int H, int W, int n_views, double min_cover, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (std::isnan(min_cover)) return fail(SUCRE_ERR_ARG, "min_cover is NaN");
    return check_hip(launch_finalize(L, static_cast<uint8_t *>(ws), min_cover, static_cast<hipStream_t>(stream)),
                     "sucre_finalize_matches");
}

int sucre_finalize_matches_fmt(void *ws, int H, int W, int n_views, double min_cover, int obs_format, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (std::isnan(min_cover)) return fail(SUCRE_ERR_ARG, "min_cover is NaN");
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    return check_hip(launch_finalize(L, static_cast<uint8_t *>(ws), min_cover, static_cast<hipStream_t>(stream),
                                     nullptr, nullptr, obs_format), "sucre_finalize_matches_fmt");
}

int sucre_fit_init(void *ws, int H, int W, int n_views, const uint8_t *rgb1_dev, const float *depth1_dev,
                   const float *params0, const float *J0_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (!depth1_dev || !params0) return fail(SUCRE_ERR_ARG, "depth1_dev / params0 is NULL");
    if (!rgb1_dev && !J0_dev) return fail(SUCRE_ERR_ARG, "need rgb1_dev or J0_dev");
    return check_hip(launch_fit_init(L, static_cast<uint8_t *>(ws), rgb1_dev, depth1_dev, params0, J0_dev,
                                     static_cast<hipStream_t>(stream)), "sucre_fit_init");
}

int sucre_fit_grad(void *ws, int H, int W, int n_views, int step, double lr, double beta1, double beta2,
                   double eps, unsigned flags, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (flags & ~(SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_OBS_U16MM)) return fail(SUCRE_ERR_ARG, "unknown fit flags 0x%x", flags);
    if ((flags & SUCRE_FIT_CLOSED_FORM) && step == 1)  // see sucre_fit_run: start the one-pass kernel from a solved J
        if (int rc = check_hip(launch_update_J(L, static_cast<uint8_t *>(ws), (flags & SUCRE_FIT_OBS_U16MM) ? SUCRE_OBS_U16MM : SUCRE_OBS_F32,
                                               static_cast<hipStream_t>(stream)), "sucre_fit_grad/update_J")) return rc;
    return check_hip(launch_fit_grad(L, static_cast<uint8_t *>(ws), adam_coef(step, lr, beta1, beta2, eps), flags,
                                     static_cast<hipStream_t>(stream)), "sucre_fit_grad");
}

int sucre_fit_step(void *ws, int H, int W, int n_views, int step, double lr, double beta1, double beta2,
                   double eps, double *trace_row_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (trace_row_dev && !aligned(trace_row_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    return check_hip(launch_fit_step(L, static_cast<uint8_t *>(ws), adam_coef(step, lr, beta1, beta2, eps),
                                     trace_row_dev, static_cast<hipStream_t>(stream)), "sucre_fit_step");
}

int sucre_fit_run(void *ws, int H, int W, int n_views, int t0, int T, double lr, double beta1, double beta2,
                  double eps, unsigned flags, double *trace_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (t0 < 0 || T < 0) return fail(SUCRE_ERR_RANGE, "t0=%d T=%d must be >= 0", t0, T);
    if (int rc = check_adam(t0 + 1, lr, beta1, beta2, eps)) return rc;
    if (flags & ~(SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_OBS_U16MM | SUCRE_FIT_KEEP_J | SUCRE_FIT_UNPAIRED)) return fail(SUCRE_ERR_ARG, "unknown fit flags 0x%x", flags);
    if (trace_dev && !aligned(trace_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    auto *w = static_cast<uint8_t *>(ws);
    auto s = static_cast<hipStream_t>(stream);
    const int fmt = (flags & SUCRE_FIT_OBS_U16MM) ? SUCRE_OBS_U16MM : SUCRE_OBS_F32;
    // J-parameter iterations go in pairs of launches (fit.hip, 'Paired iterations'); an odd one out runs alone, behind them
    const bool paired = fit_pair_built() && !(flags & (SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_UNPAIRED));
    flags &= ~SUCRE_FIT_UNPAIRED;
    // The one-pass closed-form kernel forms its sums relative to the previous J (fit.hip, AccOne): at t0 = 0 that is
    // the initial image, far from the solved J, and the differences S - dJ S' cancel digits in iteration 0 (seen as
    // 2.6e-5 relative on the logged cost at 4K x 25 views).  One plain update_J first makes dJ small from the start.
    if ((flags & SUCRE_FIT_CLOSED_FORM) && t0 == 0 && T > 0)
        if (int rc = check_hip(launch_update_J(L, w, fmt, s), "sucre_fit_run/initial update_J")) return rc;
    int it = 0;
    for (; paired && it + 1 < T; it += 2) {
        const AdamCoef co0 = adam_coef(t0 + it + 1, lr, beta1, beta2, eps), co1 = adam_coef(t0 + it + 2, lr, beta1, beta2, eps);
        if (int rc = check_hip(launch_fit_pair_fused(L, w, co0, co1, flags, trace_dev ? trace_dev + (size_t)it * 10 : nullptr,
                                                     trace_dev ? trace_dev + (size_t)(it + 1) * 10 : nullptr, s), "sucre_fit_run")) return rc;
    }
    for (; it < T; ++it) {
        const AdamCoef co = adam_coef(t0 + it + 1, lr, beta1, beta2, eps);
        if (int rc = check_hip(launch_fit_iter_fused(L, w, co, flags, trace_dev ? trace_dev + (size_t)it * 10 : nullptr, s),
                               "sucre_fit_run")) return rc;
    }
    if ((flags & SUCRE_FIT_CLOSED_FORM) && !(flags & SUCRE_FIT_KEEP_J))
        return check_hip(launch_update_J(L, w, fmt, s), "sucre_fit_run/update_J");
    return SUCRE_OK;
}

int sucre_set_n_obs_total(void *ws, int H, int W, int n_views, uint64_t n_obs_total, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (n_obs_total == 0) return fail(SUCRE_ERR_RANGE, "n_obs_total must be > 0");
    return check_hip(launch_set_n_obs_total(L, static_cast<uint8_t *>(ws), n_obs_total,
                                            static_cast<hipStream_t>(stream)), "sucre_set_n_obs_total");
}

int sucre_update_J(void *ws, int H, int W, int n_views, void *stream) {
    return sucre_update_J_fmt(ws, H, W, n_views, SUCRE_OBS_F32, stream);
}

int sucre_update_J_fmt(void *ws, int H, int W, int n_views, int obs_format, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    return check_hip(launch_update_J(L, static_cast<uint8_t *>(ws), obs_format == SUCRE_OBS_U16MM ? SUCRE_OBS_U16MM : SUCRE_OBS_F32,
                                     static_cast<hipStream_t>(stream)),
                     "sucre_update_J");
}

int sucre_export_J(const void *ws, int H, int W, int n_views, float *J_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (!J_dev) return fail(SUCRE_ERR_ARG, "J_dev is NULL");
    return check_hip(launch_export_J(L, static_cast<const uint8_t *>(ws), J_dev, static_cast<hipStream_t>(stream)),
                     "sucre_export_J");
}

int sucre_export_view(const void *ws, int H, int W, int n_views, int k, float *z_dev, uint8_t *rgb_dev,
                      void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    if (!z_dev && !rgb_dev) return fail(SUCRE_ERR_ARG, "both outputs are NULL");
    return check_hip(launch_export_view(L, static_cast<const uint8_t *>(ws), k, z_dev, rgb_dev,
                                        static_cast<hipStream_t>(stream)), "sucre_export_view");
}

int sucre_check_store(const void *ws, int H, int W, int n_views, uint32_t *verdict_dev, uint64_t *scratch_dev,
                      void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (!verdict_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "verdict_dev / scratch_dev is NULL");
    if (!aligned(verdict_dev, 4) || !aligned(scratch_dev, 8)) return fail(SUCRE_ERR_ARG, "outputs must be 4 / 8-byte aligned");
    return check_hip(launch_check_store(L, static_cast<const uint8_t *>(ws), verdict_dev, scratch_dev,
                                        static_cast<hipStream_t>(stream)), "sucre_check_store");
}

/* ---- shared water parameters over the images of a rank: one launch + one collective per iteration -------------- */

size_t sucre_group_bytes(int n_images) { return n_images > 0 ? group_bytes(n_images) : 0; }

int64_t sucre_group_sums_offset(void) { return group_sums_offset(); }

int sucre_group_init(void *group_dev, int n_images, const sucre_group_image_t *images, const float *params0, void *stream) {
    if (!group_dev || !aligned(group_dev, 256)) return fail(SUCRE_ERR_ARG, "group buffer is NULL or not 256-byte aligned");
    if (n_images < 1 || !images || !params0) return fail(SUCRE_ERR_ARG, "need at least one image and params0");
    auto s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(launch_group_init(group_dev, params0, s), "sucre_group_init")) return rc;
    for (int i = 0; i < n_images; ++i) {
        Layout L;
        if (int rc = check_ws(images[i].ws, images[i].H, images[i].W, images[i].n_views, &L)) return rc;
        if (int rc = check_hip(launch_group_set_image(group_dev, i, L, static_cast<uint8_t *>(images[i].ws), s), "sucre_group_init")) return rc;
    }
    return SUCRE_OK;
}

int sucre_group_iter(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps, unsigned flags,
                     uint64_t n_obs_total, double *trace_dev, void *stream) {
    if (!group_dev || n_images < 1) return fail(SUCRE_ERR_ARG, "group buffer is NULL / no image");
    if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (flags & ~(SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_OBS_U16MM)) return fail(SUCRE_ERR_ARG, "unknown fit flags 0x%x", flags);
    if (n_obs_total == 0) return fail(SUCRE_ERR_RANGE, "n_obs_total must be > 0");
    if (trace_dev && !aligned(trace_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    const AdamCoef co_prev = adam_coef(step > 1 ? step - 1 : 1, lr, beta1, beta2, eps);
    double *row = (trace_dev && step > 1) ? trace_dev + (size_t)(step - 2) * 10 : nullptr;
    return check_hip(launch_group_iter(group_dev, n_images, step, co_prev, adam_coef(step, lr, beta1, beta2, eps), flags, n_obs_total,
                                       row, static_cast<hipStream_t>(stream)), "sucre_group_iter");
}

int sucre_group_finish(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                       uint64_t n_obs_total, double *trace_dev, void *stream) {
    if (!group_dev || n_images < 1) return fail(SUCRE_ERR_ARG, "group buffer is NULL / no image");
    if (step < 0) return fail(SUCRE_ERR_RANGE, "step=%d must be >= 0", step);
    if (step >= 1) if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (n_obs_total == 0) return fail(SUCRE_ERR_RANGE, "n_obs_total must be > 0");
    double *row = (trace_dev && step >= 1) ? trace_dev + (size_t)(step - 1) * 10 : nullptr;
    return check_hip(launch_group_finish(group_dev, n_images, step, adam_coef(step >= 1 ? step : 1, lr, beta1, beta2, eps), n_obs_total,
                                         row, static_cast<hipStream_t>(stream)), "sucre_group_finish");
}

/* ---- independent images, one launch per iteration ---------------------------------------------------------------- */

size_t sucre_batch_bytes(int n_images) { return n_images > 0 ? batch_bytes(n_images) : 0; }

int sucre_fit_run_batch(void *batch_dev, int n_images, void *const *ws, double *const *trace_dev, int H, int W, const int *n_views,
                        int t0, int T, double lr, double beta1, double beta2, double eps, unsigned flags, void *stream) {
    if (!batch_dev || !aligned(batch_dev, 256)) return fail(SUCRE_ERR_ARG, "batch buffer is NULL or not 256-byte aligned");
    if (n_images < 1 || !ws || !n_views) return fail(SUCRE_ERR_ARG, "need at least one image (ws and n_views arrays)");
    if (n_images > 4096) return fail(SUCRE_ERR_RANGE, "n_images=%d: at most 4096 images per batch", n_images);
    std::vector<Layout> layouts((size_t)n_images);
    for (int i = 0; i < n_images; ++i) {
        if (int rc = check_ws(ws[i], H, W, n_views[i], &layouts[(size_t)i])) return rc;
        for (int j = 0; j < i; ++j)
            if (ws[j] == ws[i]) return fail(SUCRE_ERR_ARG, "images %d and %d share a workspace", j, i);
        if (trace_dev && trace_dev[i] && !aligned(trace_dev[i], 8)) return fail(SUCRE_ERR_ARG, "trace of image %d must be 8-byte aligned", i);
    }
    if (t0 < 0 || T < 0) return fail(SUCRE_ERR_RANGE, "t0=%d T=%d must be >= 0", t0, T);
    if (int rc = check_adam(t0 + 1, lr, beta1, beta2, eps)) return rc;
    if (flags & ~(SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_OBS_U16MM | SUCRE_FIT_KEEP_J)) return fail(SUCRE_ERR_ARG, "unknown fit flags 0x%x", flags);
    auto s = static_cast<hipStream_t>(stream);
    const int fmt = (flags & SUCRE_FIT_OBS_U16MM) ? SUCRE_OBS_U16MM : SUCRE_OBS_F32;
    if (int rc = check_hip(launch_batch_set(batch_dev, n_images, reinterpret_cast<uint8_t *const *>(ws), trace_dev, layouts.data(), flags, s),
                           "sucre_fit_run_batch/table")) return rc;
    if ((flags & SUCRE_FIT_CLOSED_FORM) && t0 == 0 && T > 0)   // as sucre_fit_run: the one-pass kernel starts from a solved J
        for (int i = 0; i < n_images; ++i)
            if (int rc = check_hip(launch_update_J(layouts[(size_t)i], static_cast<uint8_t *>(ws[i]), fmt, s), "sucre_fit_run_batch/initial update_J")) return rc;
    for (int it = 0; it < T; ++it)
        if (int rc = check_hip(launch_batch_iter(layouts[0], batch_dev, n_images, adam_coef(t0 + it + 1, lr, beta1, beta2, eps), flags, it, s),
                               "sucre_fit_run_batch")) return rc;
    if ((flags & SUCRE_FIT_CLOSED_FORM) && !(flags & SUCRE_FIT_KEEP_J))
        for (int i = 0; i < n_images; ++i)
            if (int rc = check_hip(launch_update_J(layouts[(size_t)i], static_cast<uint8_t *>(ws[i]), fmt, s), "sucre_fit_run_batch/update_J")) return rc;
    return SUCRE_OK;
}

size_t sucre_select_scratch_bytes(void) { return select_scratch_bytes(); }

int sucre_select_ranks(const float *J_dev, int H, int W, int n_ranks, const uint64_t *ranks, float *out_dev, void *scratch_dev,
                       void *stream) {
    if (H <= 0 || W <= 0) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d", W, H);
    if (!J_dev || !ranks || !out_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "J_dev / ranks / out_dev / scratch_dev is NULL");
    if (n_ranks < 1 || n_ranks > 8) return fail(SUCRE_ERR_RANGE, "n_ranks=%d outside [1,8]", n_ranks);
    if (!aligned(scratch_dev, 8) || !aligned(J_dev, 4) || !aligned(out_dev, 4)) return fail(SUCRE_ERR_ARG, "misaligned pointer");
    return check_hip(launch_select_ranks(J_dev, H, W, n_ranks, ranks, out_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_select_ranks");
}

int sucre_count_valid(const float *J_dev, int H, int W, uint64_t *count_dev, void *stream) {
    if (H <= 0 || W <= 0) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d", W, H);
    if (!J_dev || !count_dev) return fail(SUCRE_ERR_ARG, "J_dev / count_dev is NULL");
    if (!aligned(J_dev, 4) || !aligned(count_dev, 8)) return fail(SUCRE_ERR_ARG, "misaligned pointer");
    return check_hip(launch_count_valid(J_dev, H, W, count_dev, static_cast<hipStream_t>(stream)), "sucre_count_valid");
}

int sucre_plot_stretch(const float *J_dev, int H, int W, const float *lo, const float *hi, uint8_t *out_dev, void *stream) {
    if (H <= 0 || W <= 0) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d", W, H);
    if (!J_dev || !lo || !hi || !out_dev) return fail(SUCRE_ERR_ARG, "J_dev / lo / hi / out_dev is NULL");
    if (!aligned(J_dev, 4)) return fail(SUCRE_ERR_ARG, "misaligned pointer");
    return check_hip(launch_plot_stretch(J_dev, H, W, lo, hi, out_dev, static_cast<hipStream_t>(stream)), "sucre_plot_stretch");
}

/* ---- pooled radix select: order statistics of the valid pixels of many images ---------------------------------------- */

size_t sucre_pool_select_bytes(void) { return pool_state_bytes(); }

size_t sucre_pool_table_bytes(int n_images) {
    if (n_images < 0 || n_images > kPoolMaxImages) {
        fail(SUCRE_ERR_ARG, "n_images=%d outside [0,%d]", n_images, kPoolMaxImages);
        return 0;
    }
    return pool_table_bytes(n_images);
}

int sucre_pool_select_begin(void *state_dev, void *stream) {
    if (!state_dev || !aligned(state_dev, 8)) return fail(SUCRE_ERR_ARG, "pool select state is NULL or not 8-byte aligned");
    return check_hip(launch_pool_begin(state_dev, static_cast<hipStream_t>(stream)), "sucre_pool_select_begin");
}

int sucre_pool_select_pass(void *state_dev, int pass, void *table_dev, int n_images, const sucre_pool_image_t *images, int n_ranks,
                           void *stream) {
    if (!state_dev || !aligned(state_dev, 8)) return fail(SUCRE_ERR_ARG, "pool select state is NULL or not 8-byte aligned");
    if (pass < 0 || pass > 3) return fail(SUCRE_ERR_ARG, "pass=%d outside [0,3]", pass);
    if (n_ranks < 1 || n_ranks > kPoolMaxRanks) return fail(SUCRE_ERR_ARG, "n_ranks=%d outside [1,%d]", n_ranks, kPoolMaxRanks);
    if (n_images < 0 || n_images > kPoolMaxImages) return fail(SUCRE_ERR_ARG, "n_images=%d outside [0,%d]", n_images, kPoolMaxImages);
    if (n_images == 0) return SUCRE_OK;   // nothing to add, nothing launched
    if (!images) return fail(SUCRE_ERR_ARG, "images is NULL");
    if (!table_dev || !aligned(table_dev, 8)) return fail(SUCRE_ERR_ARG, "pool table is NULL or not 8-byte aligned");
    uint64_t blocks = 0;
    for (int i = 0; i < n_images; ++i) {
        if (images[i].n_px < 0) return fail(SUCRE_ERR_ARG, "image %d: negative pixel count %lld", i, (long long)images[i].n_px);
        if (images[i].n_px > 0 && (!images[i].J || !aligned(images[i].J, 16)))
            return fail(SUCRE_ERR_ARG, "image %d: J is NULL or not 16-byte aligned", i);
        blocks += pool_blocks(images[i].n_px);
        if (blocks > 0x7fffffffull) return fail(SUCRE_ERR_ARG, "the images of one call may hold 2^45 pixels together (image %d passes that)", i);
    }
    return check_hip(launch_pool_pass(state_dev, pass, table_dev, n_images, images, n_ranks, static_cast<hipStream_t>(stream)),
                     "sucre_pool_select_pass");
}

int sucre_pool_select_locate(void *state_dev, int pass, int n_ranks, const uint64_t *ranks, float *out_dev, void *stream) {
    if (!state_dev || !aligned(state_dev, 8)) return fail(SUCRE_ERR_ARG, "pool select state is NULL or not 8-byte aligned");
    if (pass < 0 || pass > 3) return fail(SUCRE_ERR_ARG, "pass=%d outside [0,3]", pass);
    if (n_ranks < 1 || n_ranks > kPoolMaxRanks) return fail(SUCRE_ERR_ARG, "n_ranks=%d outside [1,%d]", n_ranks, kPoolMaxRanks);
    if (pass == 0 && !ranks) return fail(SUCRE_ERR_ARG, "ranks is NULL at pass 0");
    if (pass == 3 && (!out_dev || !aligned(out_dev, 4))) return fail(SUCRE_ERR_ARG, "out_dev is NULL or misaligned at pass 3");
    return check_hip(launch_pool_locate(state_dev, pass, n_ranks, ranks, out_dev, static_cast<hipStream_t>(stream)),
                     "sucre_pool_select_locate");
}

/* ---- artificial-light model (--light-model) ------------------------------------------------------------------ */

size_t sucre_light_workspace_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) { fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views); return 0; }
    return light_workspace_bytes(L);
}

size_t sucre_light_workspace_bytes_ext(int H, int W, int n_views, int ext_mode) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) { fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views); return 0; }
    if (ext_mode < SUCRE_EXT_POINTS || ext_mode > SUCRE_EXT_POINTS_COLOUR) { fail(SUCRE_ERR_ARG, "unknown extension mode %d", ext_mode); return 0; }
    return light_workspace_bytes(L, ext_mode == SUCRE_EXT_POINTS_COLOUR ? 2 : 1);
}

int64_t sucre_light_params_offset(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) return fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
    return light_params_offset(L);
}

static int check_lws(const void *lws) {
    if (!lws) return fail(SUCRE_ERR_ARG, "light workspace is NULL");
    if (!aligned(lws, 256)) return fail(SUCRE_ERR_ARG, "light workspace must be 256-byte aligned");
    return SUCRE_OK;
}

int sucre_match_views_light(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                            const sucre_view_t *views_dev, int k0, int k1, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (!target || !views_dev || !target->depth) return fail(SUCRE_ERR_ARG, "target / views_dev / target depth is NULL");
    if (target->H != H || target->W != W) return fail(SUCRE_ERR_ARG, "target is %dx%d, expected %dx%d", target->W, target->H, W, H);
    if (k0 < 0 || k1 > n_views || k0 >= k1) return fail(SUCRE_ERR_RANGE, "view range [%d,%d) outside [0,%d)", k0, k1, n_views);
    return check_hip(launch_match(L, static_cast<uint8_t *>(ws), *target, views_dev, k0, k1, static_cast<hipStream_t>(stream),
                                  light_ext_dense(L, static_cast<uint8_t *>(lws))), "sucre_match_views_light");
}

int sucre_match_views_fcolour(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                              const sucre_view_t *views_dev, int k0, int k1, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (!target || !views_dev || !target->depth) return fail(SUCRE_ERR_ARG, "target / views_dev / target depth is NULL");
    if (target->H != H || target->W != W) return fail(SUCRE_ERR_ARG, "target is %dx%d, expected %dx%d", target->W, target->H, W, H);
    if (k0 < 0 || k1 > n_views || k0 >= k1) return fail(SUCRE_ERR_RANGE, "view range [%d,%d) outside [0,%d)", k0, k1, n_views);
    return check_hip(launch_match(L, static_cast<uint8_t *>(ws), *target, views_dev, k0, k1, static_cast<hipStream_t>(stream),
                                  light_ext_dense(L, static_cast<uint8_t *>(lws)), SUCRE_EXT_COLOUR), "sucre_match_views_fcolour");
}

int sucre_match_views_light_fcolour(void *ws, void *lws, int H, int W, int n_views, const sucre_view_t *target,
                                    const sucre_view_t *views_dev, int k0, int k1, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (!target || !views_dev || !target->depth) return fail(SUCRE_ERR_ARG, "target / views_dev / target depth is NULL");
    if (target->H != H || target->W != W) return fail(SUCRE_ERR_ARG, "target is %dx%d, expected %dx%d", target->W, target->H, W, H);
    if (k0 < 0 || k1 > n_views || k0 >= k1) return fail(SUCRE_ERR_RANGE, "view range [%d,%d) outside [0,%d)", k0, k1, n_views);
    auto *l = static_cast<uint8_t *>(lws);
    return check_hip(launch_match(L, static_cast<uint8_t *>(ws), *target, views_dev, k0, k1, static_cast<hipStream_t>(stream),
                                  light_ext_dense(L, l), SUCRE_EXT_POINTS_COLOUR, light_ext2_dense(L, l)),
                     "sucre_match_views_light_fcolour");
}

int sucre_finalize_matches_ext(void *ws, void *lws, int H, int W, int n_views, double min_cover, int ext_mode, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (std::isnan(min_cover)) return fail(SUCRE_ERR_ARG, "min_cover is NaN");
    if (ext_mode < SUCRE_EXT_POINTS || ext_mode > SUCRE_EXT_POINTS_COLOUR) return fail(SUCRE_ERR_ARG, "unknown extension mode %d", ext_mode);
    auto *l = static_cast<uint8_t *>(lws);
    const bool both = ext_mode == SUCRE_EXT_POINTS_COLOUR;
    return check_hip(launch_finalize(L, static_cast<uint8_t *>(ws), min_cover, static_cast<hipStream_t>(stream),
                                     light_ext_dense(L, l), light_ext_comp(L, l), SUCRE_OBS_F32,
                                     both ? light_ext2_dense(L, l) : nullptr, both ? light_ext2_comp(L, l) : nullptr),
                     "sucre_finalize_matches_ext");
}

int sucre_import_view_ext(void *ws, void *lws, int H, int W, int n_views, int k, const int16_t *u1_dev, const int16_t *v1_dev,
                          const float *z_dev, const uint8_t *rgb_dev, const float *ext_dev, int64_t n, int ext_mode, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    if (n < 0) return fail(SUCRE_ERR_RANGE, "negative observation count %lld", (long long)n);
    if (ext_mode < SUCRE_EXT_POINTS || ext_mode > SUCRE_EXT_POINTS_COLOUR) return fail(SUCRE_ERR_ARG, "unknown extension mode %d", ext_mode);
    if (n > 0 && (!u1_dev || !v1_dev || !z_dev || !ext_dev)) return fail(SUCRE_ERR_ARG, "NULL match list");
    if (n > 0 && ext_mode == SUCRE_EXT_POINTS && !rgb_dev) return fail(SUCRE_ERR_ARG, "camera-point lists need uint8 colours too");
    auto *l = static_cast<uint8_t *>(lws);
    return check_hip(launch_import_view(L, static_cast<uint8_t *>(ws), k, u1_dev, v1_dev, z_dev, rgb_dev, (long long)n,
                                        static_cast<hipStream_t>(stream), light_ext_dense(L, l), ext_dev,
                                        ext_mode == SUCRE_EXT_POINTS_COLOUR ? light_ext2_dense(L, l) : nullptr),
                     "sucre_import_view_ext");
}

int sucre_export_view_ext(const void *ws, const void *lws, int H, int W, int n_views, int k, float *planes_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    if (!planes_dev) return fail(SUCRE_ERR_ARG, "planes_dev is NULL");
    return check_hip(launch_export_view_ext(L, static_cast<const uint8_t *>(ws),
                                            light_ext_dense(L, const_cast<uint8_t *>(static_cast<const uint8_t *>(lws))), k,
                                            planes_dev, static_cast<hipStream_t>(stream)), "sucre_export_view_ext");
}

int sucre_export_view_ext2(const void *ws, const void *lws, int H, int W, int n_views, int k, float *planes_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (k < 0 || k >= n_views) return fail(SUCRE_ERR_RANGE, "view %d outside [0,%d)", k, n_views);
    if (!planes_dev) return fail(SUCRE_ERR_ARG, "planes_dev is NULL");
    return check_hip(launch_export_view_ext(L, static_cast<const uint8_t *>(ws),
                                            light_ext2_dense(L, const_cast<uint8_t *>(static_cast<const uint8_t *>(lws))), k,
                                            planes_dev, static_cast<hipStream_t>(stream)), "sucre_export_view_ext2");
}

int sucre_finalize_matches_light(void *ws, void *lws, int H, int W, int n_views, double min_cover, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (std::isnan(min_cover)) return fail(SUCRE_ERR_ARG, "min_cover is NaN");
    auto *l = static_cast<uint8_t *>(lws);
    return check_hip(launch_finalize(L, static_cast<uint8_t *>(ws), min_cover, static_cast<hipStream_t>(stream),
                                     light_ext_dense(L, l), light_ext_comp(L, l)), "sucre_finalize_matches_light");
}

int sucre_fit_init_light(void *ws, void *lws, int H, int W, int n_views, const uint8_t *rgb1_dev, const float *depth1_dev,
                         const float *params0, const float *J0_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (!depth1_dev || !params0) return fail(SUCRE_ERR_ARG, "depth1_dev / params0 is NULL");
    if (!rgb1_dev && !J0_dev) return fail(SUCRE_ERR_ARG, "need rgb1_dev or J0_dev");
    auto s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(launch_fit_init(L, static_cast<uint8_t *>(ws), rgb1_dev, depth1_dev, params0, J0_dev, s),
                           "sucre_fit_init_light/J")) return rc;
    return check_hip(launch_light_init(L, static_cast<uint8_t *>(lws), params0, s), "sucre_fit_init_light");
}

int sucre_update_J_light(void *ws, void *lws, int H, int W, int n_views, void *stream) {
    return sucre_update_J_ext(ws, lws, H, W, n_views, 0u, stream);
}

int sucre_update_J_ext(void *ws, void *lws, int H, int W, int n_views, unsigned flags, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (flags & ~(SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & SUCRE_FIT_EXT_COLOUR) && (flags & SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "SUCRE_FIT_EXT_COLOUR and SUCRE_FIT_EXT_BOTH exclude each other");
    return check_hip(launch_light_update_J(L, static_cast<uint8_t *>(ws), static_cast<uint8_t *>(lws), flags,
                                           static_cast<hipStream_t>(stream)), "sucre_update_J_ext");
}

int sucre_fit_run_light(void *ws, void *lws, int H, int W, int n_views, int t0, int T, double lr, double beta1,
                        double beta2, double eps, unsigned flags, double *trace_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (t0 < 0 || T < 0) return fail(SUCRE_ERR_RANGE, "t0=%d T=%d must be >= 0", t0, T);
    if (int rc = check_adam(t0 + 1, lr, beta1, beta2, eps)) return rc;
    if (trace_dev && !aligned(trace_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    if (flags & ~(SUCRE_FIT_CLOSED_FORM | SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_KEEP_J | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown fit flags 0x%x", flags);
    if ((flags & SUCRE_FIT_EXT_COLOUR) && (flags & SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "SUCRE_FIT_EXT_COLOUR and SUCRE_FIT_EXT_BOTH exclude each other");
    if (T > 0)   // which strips every wave of the gradient launches works on (layout.h, the deal): written once per call
        if (int rc = check_hip(launch_light_deal(L, static_cast<uint8_t *>(ws), static_cast<uint8_t *>(lws), flags,
                                                 static_cast<hipStream_t>(stream)), "sucre_fit_run_light/deal")) return rc;
    for (int it = 0; it < T; ++it) {
        const AdamCoef co = adam_coef(t0 + it + 1, lr, beta1, beta2, eps);
        if (int rc = check_hip(launch_light_iter(L, static_cast<uint8_t *>(ws), static_cast<uint8_t *>(lws), co, flags,
                                                 trace_dev ? trace_dev + (size_t)it * 20 : nullptr,
                                                 static_cast<hipStream_t>(stream)), "sucre_fit_run_light")) return rc;
    }
    if ((flags & SUCRE_FIT_CLOSED_FORM) && !(flags & SUCRE_FIT_KEEP_J))  // the final update_J of sucre.py:156
        return check_hip(launch_light_update_J(L, static_cast<uint8_t *>(ws), static_cast<uint8_t *>(lws),
                                               flags & (SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH), static_cast<hipStream_t>(stream)),
                         "sucre_fit_run_light/update_J");
    return SUCRE_OK;
}

/* ---- fit residuals per pixel and per view ------------------------------------------------------------------------ */

size_t sucre_residual_scratch_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) {
        fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
        return 0;
    }
    return residual_scratch_bytes(L);
}

}  // extern "C"

namespace sucre {
static int check_residual_outputs(const int32_t *count_dev, const float *ssr_dev, const double *view_stats_dev, const void *scratch_dev) {
    if (!count_dev || !ssr_dev || !view_stats_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "count_dev / ssr_dev / view_stats_dev / scratch_dev is NULL");
    if (!aligned(count_dev, 4) || !aligned(ssr_dev, 4) || !aligned(view_stats_dev, 8)) return fail(SUCRE_ERR_ARG, "outputs must be 4 / 4 / 8-byte aligned");
    if (!aligned(scratch_dev, 16)) return fail(SUCRE_ERR_ARG, "scratch_dev must be 16-byte aligned");
    return SUCRE_OK;
}
}  // namespace sucre

extern "C" {

int sucre_fit_residuals(const void *ws, int H, int W, int n_views, int obs_format, int32_t *count_dev, float *ssr_dev,
                        double *view_stats_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    if (int rc = check_residual_outputs(count_dev, ssr_dev, view_stats_dev, scratch_dev)) return rc;
    return check_hip(launch_residuals(L, static_cast<const uint8_t *>(ws), obs_format == SUCRE_OBS_U16MM ? SUCRE_OBS_U16MM : SUCRE_OBS_F32,
                                      count_dev, ssr_dev, view_stats_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_fit_residuals");
}

int sucre_fit_residuals_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags, int32_t *count_dev,
                            float *ssr_dev, double *view_stats_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (flags & ~(SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & SUCRE_FIT_EXT_COLOUR) && (flags & SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "SUCRE_FIT_EXT_COLOUR and SUCRE_FIT_EXT_BOTH exclude each other");
    if (int rc = check_residual_outputs(count_dev, ssr_dev, view_stats_dev, scratch_dev)) return rc;
    return check_hip(launch_residuals_ext(L, static_cast<const uint8_t *>(ws), static_cast<const uint8_t *>(lws), flags, count_dev,
                                          ssr_dev, view_stats_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_fit_residuals_ext");
}

/* ---- outlier-trimmed refit: sigma-clip observations out of the dense store ---------------------------------------------- */

size_t sucre_trim_scratch_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) {
        fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
        return 0;
    }
    return trim_scratch_bytes(L);
}

}  // extern "C"

namespace sucre {
static int check_trim_args(double k_sigma, const double *view_stats_dev, const int32_t *dropped_dev, const int64_t *view_dropped_dev,
                           const float *thresholds_dev, const void *scratch_dev) {
    if (!std::isfinite(k_sigma) || !(k_sigma > 0.0)) return fail(SUCRE_ERR_ARG, "k_sigma must be finite and > 0 (got %g)", k_sigma);
    if (!view_stats_dev || !dropped_dev || !view_dropped_dev || !thresholds_dev || !scratch_dev)
        return fail(SUCRE_ERR_ARG, "view_stats_dev / dropped_dev / view_dropped_dev / thresholds_dev / scratch_dev is NULL");
    if (!aligned(view_stats_dev, 8) || !aligned(dropped_dev, 4) || !aligned(view_dropped_dev, 8) || !aligned(thresholds_dev, 4))
        return fail(SUCRE_ERR_ARG, "view_stats_dev / dropped_dev / view_dropped_dev / thresholds_dev must be 8 / 4 / 8 / 4-byte aligned");
    if (!aligned(scratch_dev, 16)) return fail(SUCRE_ERR_ARG, "scratch_dev must be 16-byte aligned");
    return SUCRE_OK;
}
}  // namespace sucre

extern "C" {

int sucre_trim_outliers(void *ws, int H, int W, int n_views, int obs_format, double k_sigma, const double *view_stats_dev,
                        int32_t *dropped_dev, int64_t *view_dropped_dev, float *thresholds_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    if (int rc = check_trim_args(k_sigma, view_stats_dev, dropped_dev, view_dropped_dev, thresholds_dev, scratch_dev)) return rc;
    return check_hip(launch_trim(L, static_cast<uint8_t *>(ws), obs_format == SUCRE_OBS_U16MM ? SUCRE_OBS_U16MM : SUCRE_OBS_F32, k_sigma,
                                 view_stats_dev, dropped_dev, view_dropped_dev, thresholds_dev, scratch_dev,
                                 static_cast<hipStream_t>(stream)), "sucre_trim_outliers");
}

int sucre_trim_outliers_ext(void *ws, const void *lws, int H, int W, int n_views, unsigned flags, double k_sigma,
                            const double *view_stats_dev, int32_t *dropped_dev, int64_t *view_dropped_dev, float *thresholds_dev,
                            void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (flags & ~(SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & SUCRE_FIT_EXT_COLOUR) && (flags & SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "SUCRE_FIT_EXT_COLOUR and SUCRE_FIT_EXT_BOTH exclude each other");
    if (int rc = check_trim_args(k_sigma, view_stats_dev, dropped_dev, view_dropped_dev, thresholds_dev, scratch_dev)) return rc;
    return check_hip(launch_trim_ext(L, static_cast<uint8_t *>(ws), static_cast<const uint8_t *>(lws), flags, k_sigma, view_stats_dev,
                                     dropped_dev, view_dropped_dev, thresholds_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_trim_outliers_ext");
}

/* ---- per-view gain compensation: estimate at the fit as it stands, divide out of the dense store ------------------------- */

size_t sucre_gain_scratch_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) {
        fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
        return 0;
    }
    return gain_scratch_bytes(L);
}

}  // extern "C"

namespace sucre {
static int check_gain_args(double limit, const double *gains_dev, const float *inv_dev, const double *sums_dev, const void *scratch_dev) {
    if (!std::isfinite(limit) || !(limit >= 1.0)) return fail(SUCRE_ERR_ARG, "limit must be finite and >= 1 (got %g)", limit);
    if (!gains_dev || !inv_dev || !sums_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "gains_dev / inv_dev / sums_dev / scratch_dev is NULL");
    if (!aligned(gains_dev, 8) || !aligned(inv_dev, 4) || !aligned(sums_dev, 8))
        return fail(SUCRE_ERR_ARG, "gains_dev / inv_dev / sums_dev must be 8 / 4 / 8-byte aligned");
    if (!aligned(scratch_dev, 16)) return fail(SUCRE_ERR_ARG, "scratch_dev must be 16-byte aligned");
    return SUCRE_OK;
}

static int check_gain_apply_args(const float *inv_dev, const int64_t *view_clipped_dev, const void *scratch_dev) {
    if (!inv_dev || !view_clipped_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "inv_dev / view_clipped_dev / scratch_dev is NULL");
    if (!aligned(inv_dev, 4) || !aligned(view_clipped_dev, 8)) return fail(SUCRE_ERR_ARG, "inv_dev / view_clipped_dev must be 4 / 8-byte aligned");
    if (!aligned(scratch_dev, 16)) return fail(SUCRE_ERR_ARG, "scratch_dev must be 16-byte aligned");
    return SUCRE_OK;
}

static int check_ext_flags(unsigned flags) {
    if (flags & ~(SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown flags 0x%x", flags);
    if ((flags & SUCRE_FIT_EXT_COLOUR) && (flags & SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "SUCRE_FIT_EXT_COLOUR and SUCRE_FIT_EXT_BOTH exclude each other");
    return SUCRE_OK;
}
}  // namespace sucre

extern "C" {

int sucre_view_gains(const void *ws, int H, int W, int n_views, int obs_format, double limit, double *gains_dev, float *inv_dev,
                     double *sums_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    if (int rc = check_gain_args(limit, gains_dev, inv_dev, sums_dev, scratch_dev)) return rc;
    return check_hip(launch_view_gains(L, static_cast<const uint8_t *>(ws), obs_format == SUCRE_OBS_U16MM ? SUCRE_OBS_U16MM : SUCRE_OBS_F32,
                                       limit, gains_dev, inv_dev, sums_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_view_gains");
}

int sucre_view_gains_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags, double limit, double *gains_dev,
                         float *inv_dev, double *sums_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (int rc = check_ext_flags(flags)) return rc;
    if (int rc = check_gain_args(limit, gains_dev, inv_dev, sums_dev, scratch_dev)) return rc;
    return check_hip(launch_view_gains_ext(L, static_cast<const uint8_t *>(ws), static_cast<const uint8_t *>(lws), flags, limit, gains_dev,
                                           inv_dev, sums_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_view_gains_ext");
}

int sucre_apply_view_gains(void *ws, int H, int W, int n_views, const float *inv_dev, int64_t *view_clipped_dev, void *scratch_dev,
                           void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_gain_apply_args(inv_dev, view_clipped_dev, scratch_dev)) return rc;
    return check_hip(launch_apply_view_gains(L, static_cast<uint8_t *>(ws), inv_dev, view_clipped_dev, scratch_dev,
                                             static_cast<hipStream_t>(stream)), "sucre_apply_view_gains");
}

int sucre_apply_view_gains_ext(void *ws, void *lws, int H, int W, int n_views, unsigned flags, const float *inv_dev,
                               int64_t *view_clipped_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (int rc = check_ext_flags(flags)) return rc;
    if (int rc = check_gain_apply_args(inv_dev, view_clipped_dev, scratch_dev)) return rc;
    return check_hip(launch_apply_view_gains_ext(L, static_cast<uint8_t *>(ws), static_cast<uint8_t *>(lws), flags, inv_dev,
                                                 view_clipped_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_apply_view_gains_ext");
}

/* ---- single-view inversion (sucre.py:66-77 with one observation per pixel: the image itself) ---------------------------- */

size_t sucre_invert_bytes(int n_images) {
    if (n_images < 1 || n_images > kInvertMaxImages) {
        fail(SUCRE_ERR_RANGE, "n_images=%d outside [1,%d]", n_images, kInvertMaxImages);
        return 0;
    }
    return invert_bytes(n_images);
}

int sucre_invert_images(void *table_dev, int n_images, const sucre_invert_image_t *images, const float *params, unsigned flags,
                        void *stream) {
    if (!table_dev || !aligned(table_dev, 256)) return fail(SUCRE_ERR_ARG, "invert table is NULL or not 256-byte aligned");
    if (n_images < 1 || n_images > kInvertMaxImages) return fail(SUCRE_ERR_RANGE, "n_images=%d outside [1,%d]", n_images, kInvertMaxImages);
    if (!images || !params) return fail(SUCRE_ERR_ARG, "images / params is NULL");
    if (flags & ~(SUCRE_INVERT_LIGHT | SUCRE_INVERT_FLOAT_COLOUR)) return fail(SUCRE_ERR_ARG, "unknown invert flags 0x%x", flags);
    const size_t rgb_align = (flags & SUCRE_INVERT_FLOAT_COLOUR) ? 16 : 4;
    uint64_t blocks = 0;
    for (int i = 0; i < n_images; ++i) {
        const sucre_invert_image_t &im = images[i];
        if (im.H < 1 || im.W < 1 || im.H > 32767 || im.W > 32767) return fail(SUCRE_ERR_ARG, "image %d: invalid size %dx%d (need 1..32767)", i, im.W, im.H);
        if (!im.depth || !im.rgb || !im.J) return fail(SUCRE_ERR_ARG, "image %d: depth / rgb / J is NULL", i);
        if (!aligned(im.depth, 16) || !aligned(im.J, 16) || !aligned(im.rgb, rgb_align))
            return fail(SUCRE_ERR_ARG, "image %d: depth / J must be 16-byte aligned, rgb %d-byte aligned", i, (int)rgb_align);
        blocks += invert_blocks(im.H, im.W);
    }
    if (blocks > 0x7fffffffull) return fail(SUCRE_ERR_RANGE, "%llu workgroups: the images of one call may hold 2^41 pixels together", (unsigned long long)blocks);
    return check_hip(launch_invert(table_dev, n_images, images, params, flags, static_cast<hipStream_t>(stream)), "sucre_invert_images");
}

/* ---- cross-view colour consistency of restored images (plot_J's valid rule, sucre.py:86-87, over sfm.py:121-125's matches) -- */

}  // extern "C"

namespace sucre {
static int check_consistency_geometry(int H, int W, int n_views) {
    if (H < 1 || W < 1 || H > 32767 || W > 32767) return fail(SUCRE_ERR_ARG, "invalid image size %dx%d (need 1..32767)", W, H);
    if (n_views < 1 || n_views > kMaxViews) return fail(SUCRE_ERR_RANGE, "n_views=%d outside [1,%d]", n_views, kMaxViews);
    return SUCRE_OK;
}
}  // namespace sucre

extern "C" {

size_t sucre_consistency_scratch_bytes(int H, int W, int n_views) {
    if (check_consistency_geometry(H, W, n_views)) return 0;
    return consist_scratch_bytes(((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile), n_views);
}

int sucre_view_consistency(int H, int W, int n_views, const sucre_view_t *target, const sucre_view_t *views_dev,
                           const float *J_target_dev, const float *const *J_views_dev, int32_t *count_dev, float *ssd_dev,
                           double *stats_dev, void *scratch_dev, void *stream) {
    if (int rc = check_consistency_geometry(H, W, n_views)) return rc;
    if (!target || !views_dev || !J_target_dev || !J_views_dev) return fail(SUCRE_ERR_ARG, "target / views_dev / J_target_dev / J_views_dev is NULL");
    if (!count_dev || !ssd_dev || !stats_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "count_dev / ssd_dev / stats_dev / scratch_dev is NULL");
    if (!aligned(count_dev, 16) || !aligned(ssd_dev, 16) || !aligned(stats_dev, 16) || !aligned(scratch_dev, 16))
        return fail(SUCRE_ERR_ARG, "count_dev / ssd_dev / stats_dev / scratch_dev must be 16-byte aligned");
    if (!target->depth) return fail(SUCRE_ERR_ARG, "target depth map is NULL");
    if (target->H != H || target->W != W) return fail(SUCRE_ERR_ARG, "target is %dx%d, expected %dx%d", target->W, target->H, W, H);
    if (!aligned(views_dev, 8) || !aligned(J_views_dev, 8) || !aligned(J_target_dev, 4))
        return fail(SUCRE_ERR_ARG, "views_dev / J_views_dev must be 8-byte aligned, J_target_dev 4-byte aligned");
    return check_hip(launch_consistency(H, W, n_views, *target, views_dev, J_target_dev, J_views_dev, count_dev, ssd_dev, stats_dev,
                                        scratch_dev, static_cast<hipStream_t>(stream)), "sucre_view_consistency");
}

/* ---- seabed mosaic of restored images: best-view ortho splat (sfm.py:90-93, 49-55; plot_J's valid rule, sucre.py:86-87) ---- */

}  // extern "C"

namespace sucre {

static int check_mosaic_images(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal) {
    if (!table_dev || !aligned(table_dev, 256)) return fail(SUCRE_ERR_ARG, "mosaic table is NULL or not 256-byte aligned");
    if (n_images < 1 || n_images > kMaxViews) return fail(SUCRE_ERR_ARG, "n_images=%d outside [1,%d]", n_images, kMaxViews);
    if (first_ordinal < 0 || first_ordinal > kMaxViews - n_images)
        return fail(SUCRE_ERR_ARG, "ordinals %d..%d outside [0,%d)", first_ordinal, first_ordinal + n_images - 1, kMaxViews);
    if (!images) return fail(SUCRE_ERR_ARG, "images is NULL");
    uint64_t blocks = 0;
    for (int i = 0; i < n_images; ++i) {
        const sucre_mosaic_image_t &im = images[i];
        if (im.H < 1 || im.W < 1 || im.H > 32767 || im.W > 32767) return fail(SUCRE_ERR_ARG, "image %d: invalid size %dx%d (need 1..32767)", i, im.W, im.H);
        if (!im.depth || !im.rgb || !im.J) return fail(SUCRE_ERR_ARG, "image %d: depth / rgb / J is NULL", i);
        if (!aligned(im.depth, 4) || !aligned(im.J, 4)) return fail(SUCRE_ERR_ARG, "image %d: depth / J must be 4-byte aligned", i);
        if (i % kMosaicLaunch == 0) blocks = 0;
        blocks += mosaic_blocks(im.H, im.W);
        if (blocks > 0x7fffffffull) return fail(SUCRE_ERR_ARG, "image %d: the 32 images of one launch may hold 2^39 pixels together", i);
    }
    return SUCRE_OK;
}

static int check_mosaic_grid(const sucre_mosaic_grid_t *g, MosaicGrid *out) {
    if (!g) return fail(SUCRE_ERR_ARG, "grid is NULL");
    for (int i = 0; i < 9; ++i) if (!std::isfinite(g->axes[i])) return fail(SUCRE_ERR_ARG, "axes[%d] is not finite", i);
    if (!std::isfinite(g->gsd) || !(g->gsd > 0.0f)) return fail(SUCRE_ERR_ARG, "gsd=%g must be finite and > 0", (double)g->gsd);
    if (!std::isfinite(g->lo_s) || !std::isfinite(g->lo_t)) return fail(SUCRE_ERR_ARG, "lo=(%g, %g) is not finite", (double)g->lo_s, (double)g->lo_t);
    if (g->Hm < 1 || g->Wm < 1 || g->Hm > (1 << 24) || g->Wm > (1 << 24))
        return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells (need 1..2^24 each way)", g->Wm, g->Hm);
    for (int i = 0; i < 9; ++i) out->axes[i] = g->axes[i];
    out->gsd = g->gsd; out->lo_s = g->lo_s; out->lo_t = g->lo_t; out->Hm = g->Hm; out->Wm = g->Wm;
    return SUCRE_OK;
}

}  // namespace sucre

extern "C" {

size_t sucre_mosaic_table_bytes(int n_images) {
    if (n_images < 1 || n_images > kMaxViews) {
        fail(SUCRE_ERR_ARG, "n_images=%d outside [1,%d]", n_images, kMaxViews);
        return 0;
    }
    return mosaic_table_bytes(n_images);
}

int sucre_mosaic_bounds(void *table_dev, int n_images, const sucre_mosaic_image_t *images, const float *axes, uint32_t *bounds_dev,
                        void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, 0)) return rc;
    if (!axes) return fail(SUCRE_ERR_ARG, "axes is NULL");
    if (!bounds_dev || !aligned(bounds_dev, 4)) return fail(SUCRE_ERR_ARG, "bounds_dev is NULL or misaligned");
    MosaicGrid g = {};
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(axes[i])) return fail(SUCRE_ERR_ARG, "axes[%d] is not finite", i);
        g.axes[i] = axes[i];
    }
    return check_hip(launch_mosaic(kMosaicBounds, table_dev, n_images, images, 0, g, bounds_dev, nullptr, nullptr, MosaicOut{},
                                   static_cast<hipStream_t>(stream)), "sucre_mosaic_bounds");
}


// The one flag a mosaic phase takes.
static int check_mosaic_flags(unsigned flags) {
    if (flags & ~SUCRE_MOSAIC_PLAIN_ATOMIC) return fail(SUCRE_ERR_ARG, "unknown mosaic flags 0x%x", flags);
    return SUCRE_OK;
}

// J_out, the copy of every image's J that a cull or the gains write in the band buffers' layout, against the images' own J: a
// buffer of its own -- a lane reads its pixel of an image's J and writes it somewhere else in J_out --, unless allow_in_place and an
// image's J is its very block of J_out (a lane then reads and writes its own pixel alone).
static int check_copy_out(const float *J_out, int n_images, const sucre_mosaic_image_t *images, bool allow_in_place) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(J_out), o1 = o0 + band_bytes(n_images, images);
    uint64_t at = 0;   // pixels ahead of the image's block
    for (int i = 0; i < n_images; ++i) {
        const uintptr_t j0 = reinterpret_cast<uintptr_t>(images[i].J), j1 = j0 + (size_t)images[i].H * (size_t)images[i].W * 12;
        if (!(allow_in_place && j0 == o0 + at * 12) && j0 < o1 && o0 < j1)
            return fail(SUCRE_ERR_ARG, allow_in_place ? "image %d: J_out overlaps the image's J without being it" : "image %d: J_out overlaps the image's J", i);
        at += mosaic_blocks(images[i].H, images[i].W) * kMosaicBlockPx;
    }
    return SUCRE_OK;
}

int sucre_mosaic_splat(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                       const sucre_mosaic_grid_t *grid, uint64_t *key_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!key_dev || !aligned(key_dev, 8)) return fail(SUCRE_ERR_ARG, "key_dev is NULL or not 8-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) ? kMosaicSplatPlain : kMosaicSplat, table_dev, n_images, images,
                                   first_ordinal, g, nullptr, reinterpret_cast<unsigned long long *>(key_dev), nullptr, MosaicOut{},
                                   static_cast<hipStream_t>(stream)), "sucre_mosaic_splat");
}

int sucre_mosaic_resolve(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, uint32_t *pix_dev, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!key_dev || !aligned(key_dev, 8)) return fail(SUCRE_ERR_ARG, "key_dev is NULL or not 8-byte aligned");
    if (!pix_dev || !aligned(pix_dev, 4)) return fail(SUCRE_ERR_ARG, "pix_dev is NULL or misaligned");
    return check_hip(launch_mosaic(kMosaicResolve, table_dev, n_images, images, first_ordinal, g, nullptr,
                                   reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(key_dev)), pix_dev, MosaicOut{},
                                   static_cast<hipStream_t>(stream)), "sucre_mosaic_resolve");
}

int sucre_mosaic_gather(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                        const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, const uint32_t *pix_dev, float *J_out,
                        uint8_t *raw_out, int32_t *source_out, int32_t *pixel_out, float *range_out, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!key_dev || !aligned(key_dev, 8)) return fail(SUCRE_ERR_ARG, "key_dev is NULL or not 8-byte aligned");
    if (!pix_dev || !aligned(pix_dev, 4)) return fail(SUCRE_ERR_ARG, "pix_dev is NULL or misaligned");
    if (!J_out || !raw_out || !source_out || !pixel_out || !range_out)
        return fail(SUCRE_ERR_ARG, "J_out / raw_out / source_out / pixel_out / range_out is NULL");
    if (!aligned(J_out, 4) || !aligned(source_out, 4) || !aligned(pixel_out, 4) || !aligned(range_out, 4))
        return fail(SUCRE_ERR_ARG, "J_out / source_out / pixel_out / range_out must be 4-byte aligned");
    MosaicOut out = {J_out, raw_out, source_out, pixel_out, range_out};
    return check_hip(launch_mosaic(kMosaicGather, table_dev, n_images, images, first_ordinal, g, nullptr,
                                   reinterpret_cast<unsigned long long *>(const_cast<uint64_t *>(key_dev)),
                                   const_cast<uint32_t *>(pix_dev), out, static_cast<hipStream_t>(stream)), "sucre_mosaic_gather");
}

static int check_feather_px(int feather_px) {
    if (feather_px < 1 || feather_px > kFeatherMax) return fail(SUCRE_ERR_ARG, "feather_px=%d outside [1,%d]", feather_px, kFeatherMax);
    return SUCRE_OK;
}

// What the two accumulate entries check, in this order, and launch; `feathered`: feather_px and feather_dev are read.
static int mosaic_accumulate(const char *entry, bool feathered, void *table_dev, int n_images, const sucre_mosaic_image_t *images,
                             int first_ordinal, const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, float inv_h, int feather_px,
                             const void *feather_dev, int64_t *acc_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!key_dev || !aligned(key_dev, 8)) return fail(SUCRE_ERR_ARG, "key_dev is NULL or not 8-byte aligned");
    if (!std::isfinite(inv_h) || !(inv_h > 0.0f)) return fail(SUCRE_ERR_ARG, "inv_h=%g must be finite and > 0", (double)inv_h);
    MosaicFeather f = {};
    if (feathered) {
        if (int rc = check_feather_px(feather_px)) return rc;
        if (!feather_dev || !aligned(feather_dev, 4)) return fail(SUCRE_ERR_ARG, "feather_dev is NULL or not 4-byte aligned");
        f = {static_cast<const uint32_t *>(feather_dev), (uint32_t)feather_px * (uint32_t)feather_px, 1.0f / (float)feather_px};
    }
    if (!acc_dev || !aligned(acc_dev, 8)) return fail(SUCRE_ERR_ARG, "acc_dev is NULL or not 8-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_accumulate((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g,
                                              reinterpret_cast<const unsigned long long *>(key_dev), inv_h, feathered ? &f : nullptr,
                                              reinterpret_cast<unsigned long long *>(acc_dev), static_cast<hipStream_t>(stream)), entry);
}

int sucre_mosaic_accumulate(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                            const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, float inv_h, int64_t *acc_dev, unsigned flags,
                            void *stream) {
    return mosaic_accumulate("sucre_mosaic_accumulate", false, table_dev, n_images, images, first_ordinal, grid, key_dev, inv_h, 0, nullptr,
                             acc_dev, flags, stream);
}

size_t sucre_mosaic_feather_bytes(int n_images, const sucre_mosaic_image_t *images) {
    if (n_images < 1 || n_images > kMaxViews || !images) {
        fail(SUCRE_ERR_ARG, "n_images=%d outside [1,%d], or images is NULL", n_images, kMaxViews);
        return 0;
    }
    for (int i = 0; i < n_images; ++i) {
        if (images[i].H < 1 || images[i].W < 1 || images[i].H > 32767 || images[i].W > 32767) {
            fail(SUCRE_ERR_ARG, "image %d: invalid size %dx%d (need 1..32767)", i, images[i].W, images[i].H);
            return 0;
        }
    }
    return feather_bytes(n_images, images);
}

int sucre_mosaic_feather(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int feather_px, void *feather_dev,
                         void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, 0)) return rc;
    if (int rc = check_feather_px(feather_px)) return rc;
    if (!feather_dev || !aligned(feather_dev, 4)) return fail(SUCRE_ERR_ARG, "feather_dev is NULL or not 4-byte aligned");
    return check_hip(launch_mosaic_feather(table_dev, n_images, images, feather_px, feather_dev, static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_feather");
}

int sucre_mosaic_accumulate_feathered(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                      const sucre_mosaic_grid_t *grid, const uint64_t *key_dev, float inv_h, int feather_px,
                                      const void *feather_dev, int64_t *acc_dev, unsigned flags, void *stream) {
    return mosaic_accumulate("sucre_mosaic_accumulate_feathered", true, table_dev, n_images, images, first_ordinal, grid, key_dev, inv_h,
                             feather_px, feather_dev, acc_dev, flags, stream);
}

int sucre_mosaic_normalize(const sucre_mosaic_grid_t *grid, const int64_t *acc_dev, float *J_out, uint8_t *raw_out, float *weight_out,
                           int32_t *samples_out, void *stream) {
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if ((uint64_t)g.Hm * (uint64_t)g.Wm > (1ull << 39)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: one pass takes 2^39 cells", g.Wm, g.Hm);
    if (!acc_dev || !aligned(acc_dev, 8)) return fail(SUCRE_ERR_ARG, "acc_dev is NULL or not 8-byte aligned");
    if (!J_out || !raw_out || !weight_out || !samples_out) return fail(SUCRE_ERR_ARG, "J_out / raw_out / weight_out / samples_out is NULL");
    if (!aligned(J_out, 4) || !aligned(weight_out, 4) || !aligned(samples_out, 4))
        return fail(SUCRE_ERR_ARG, "J_out / weight_out / samples_out must be 4-byte aligned");
    MosaicBlend out = {J_out, raw_out, weight_out, samples_out};
    return check_hip(launch_mosaic_normalize(g, reinterpret_cast<const long long *>(acc_dev), out, static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_normalize");
}

/* ---- multi-band blend: the band stack of every image and the per-cell sum of the blended bands (bands.h) ---- */

size_t sucre_mosaic_band_bytes(int n_images, const sucre_mosaic_image_t *images) {
    if (n_images < 1 || n_images > kMaxViews || !images) {
        fail(SUCRE_ERR_ARG, "n_images=%d outside [1,%d], or images is NULL", n_images, kMaxViews);
        return 0;
    }
    for (int i = 0; i < n_images; ++i) {
        if (images[i].H < 1 || images[i].W < 1 || images[i].H > 32767 || images[i].W > 32767) {
            fail(SUCRE_ERR_ARG, "image %d: invalid size %dx%d (need 1..32767)", i, images[i].W, images[i].H);
            return 0;
        }
    }
    return band_bytes(n_images, images);
}

int sucre_mosaic_band_split(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int level, const float *S_in, float *S_out,
                            float *D_out, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, 0)) return rc;
    if (level < 0 || level >= kBandsMax) return fail(SUCRE_ERR_ARG, "level=%d outside [0,%d]", level, kBandsMax - 1);
    if (level == 0 && S_in) return fail(SUCRE_ERR_ARG, "level 0 reads the images: S_in must be NULL");
    if (level > 0 && (!S_in || !aligned(S_in, 4))) return fail(SUCRE_ERR_ARG, "S_in is NULL or not 4-byte aligned");
    if (!S_out || !D_out || !aligned(S_out, 4) || !aligned(D_out, 4)) return fail(SUCRE_ERR_ARG, "S_out / D_out is NULL or not 4-byte aligned");
    // three different buffers of band_bytes each: no two of them may overlap
    const size_t n_bytes = band_bytes(n_images, images);
    const auto overlap = [n_bytes](const void *a, const void *b) {
        const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
        return a && b && x < y + n_bytes && y < x + n_bytes;
    };
    if (overlap(S_in, S_out) || overlap(S_in, D_out) || overlap(S_out, D_out))
        return fail(SUCRE_ERR_ARG, "S_in / S_out / D_out overlap: a level reads its neighbours' S_in while it writes");
    return check_hip(launch_band_split(table_dev, n_images, images, level, S_in, S_out, D_out, static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_band_split");
}

int sucre_mosaic_band_combine(const sucre_mosaic_grid_t *grid, int n_bands, const int64_t *acc_bands_dev, float *J_out, void *stream) {
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if ((uint64_t)g.Hm * (uint64_t)g.Wm > (1ull << 39)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: one pass takes 2^39 cells", g.Wm, g.Hm);
    if (n_bands < 2 || n_bands > kBandsMax + 1) return fail(SUCRE_ERR_ARG, "n_bands=%d outside [2,%d]", n_bands, kBandsMax + 1);
    if (!acc_bands_dev || !aligned(acc_bands_dev, 8)) return fail(SUCRE_ERR_ARG, "acc_bands_dev is NULL or not 8-byte aligned");
    if (!J_out || !aligned(J_out, 4)) return fail(SUCRE_ERR_ARG, "J_out is NULL or not 4-byte aligned");
    return check_hip(launch_band_combine(g, n_bands, reinterpret_cast<const long long *>(acc_bands_dev), J_out,
                                         static_cast<hipStream_t>(stream)), "sucre_mosaic_band_combine");
}

/* ---- surface test of the mosaic: the per-cell top height along e3 and the samples too far below it (surface.h) ---- */

int sucre_mosaic_surface(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, uint32_t *top_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!top_dev || !aligned(top_dev, 4)) return fail(SUCRE_ERR_ARG, "top_dev is NULL or not 4-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_surface((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, top_dev,
                                           static_cast<hipStream_t>(stream)), "sucre_mosaic_surface");
}

// Both culls: sucre_mosaic_cull (culled_above_dev NULL, two counters) and sucre_mosaic_cull_supported (three).
static int mosaic_cull(bool two_sided, const char *what, void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                       const sucre_mosaic_grid_t *grid, const uint32_t *top_dev, float tol, float *J_out, uint32_t *culled_dev,
                       uint32_t *culled_above_dev, uint64_t *counts_dev, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!top_dev || !aligned(top_dev, 4)) return fail(SUCRE_ERR_ARG, "top_dev is NULL or not 4-byte aligned");
    if (!std::isfinite(tol) || !(tol > 0.0f)) return fail(SUCRE_ERR_ARG, "tol=%g must be finite and > 0", (double)tol);
    if (!J_out || !aligned(J_out, 4)) return fail(SUCRE_ERR_ARG, "J_out is NULL or not 4-byte aligned");
    if (culled_dev && !aligned(culled_dev, 4)) return fail(SUCRE_ERR_ARG, "culled_dev is not 4-byte aligned");
    if (culled_above_dev && !aligned(culled_above_dev, 4)) return fail(SUCRE_ERR_ARG, "culled_above_dev is not 4-byte aligned");
    if (counts_dev && !aligned(counts_dev, 8)) return fail(SUCRE_ERR_ARG, "counts_dev is not 8-byte aligned");
    if (int rc = check_copy_out(J_out, n_images, images, false)) return rc;
    const MosaicCull out = {culled_dev, culled_above_dev, reinterpret_cast<unsigned long long *>(counts_dev)};
    return check_hip(launch_mosaic_cull(two_sided, table_dev, n_images, images, first_ordinal, g, top_dev, tol, J_out, out,
                                        static_cast<hipStream_t>(stream)), what);
}

int sucre_mosaic_cull(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                      const sucre_mosaic_grid_t *grid, const uint32_t *top_dev, float tol, float *J_out, uint32_t *culled_dev,
                      uint64_t *counts_dev, void *stream) {
    return mosaic_cull(false, "sucre_mosaic_cull", table_dev, n_images, images, first_ordinal, grid, top_dev, tol, J_out, culled_dev, nullptr,
                       counts_dev, stream);
}

/* ---- view-supported surface: per-cell ranks of the per-image tops, the supported top, the two-sided cull (support.h) ---- */

static int check_support_levels(int n_levels, const MosaicGrid &g) {
    if (n_levels < 1 || n_levels > kSupportMax) return fail(SUCRE_ERR_ARG, "n_levels=%d outside [1,%d]", n_levels, kSupportMax);
    if ((uint64_t)g.Hm * (uint64_t)g.Wm > (1ull << 39)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: one pass takes 2^39 cells", g.Wm, g.Hm);
    return SUCRE_OK;
}

int sucre_mosaic_support(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                         const sucre_mosaic_grid_t *grid, int n_levels, int level, uint64_t *rank_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (int rc = check_support_levels(n_levels, g)) return rc;
    if (level < 0 || level >= n_levels) return fail(SUCRE_ERR_ARG, "level=%d outside [0,%d)", level, n_levels);
    if (!rank_dev || !aligned(rank_dev, 8)) return fail(SUCRE_ERR_ARG, "rank_dev is NULL or not 8-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_support((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, level,
                                           reinterpret_cast<unsigned long long *>(rank_dev), static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_support");
}

int sucre_mosaic_support_top(const sucre_mosaic_grid_t *grid, int n_levels, const uint64_t *rank_dev, uint32_t *top_dev,
                             int32_t *support_out, int32_t *source_out, void *stream) {
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (int rc = check_support_levels(n_levels, g)) return rc;
    if (!rank_dev || !aligned(rank_dev, 8)) return fail(SUCRE_ERR_ARG, "rank_dev is NULL or not 8-byte aligned");
    if (!top_dev || !aligned(top_dev, 4)) return fail(SUCRE_ERR_ARG, "top_dev is NULL or not 4-byte aligned");
    if (!aligned(support_out, 4) || !aligned(source_out, 4)) return fail(SUCRE_ERR_ARG, "support_out / source_out must be 4-byte aligned");
    return check_hip(launch_mosaic_support_top(g, n_levels, reinterpret_cast<const unsigned long long *>(rank_dev), top_dev, support_out,
                                               source_out, static_cast<hipStream_t>(stream)), "sucre_mosaic_support_top");
}

int sucre_mosaic_cull_supported(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                                const sucre_mosaic_grid_t *grid, const uint32_t *top_dev, float tol, float *J_out,
                                uint32_t *culled_dev, uint32_t *culled_above_dev, uint64_t *counts_dev, void *stream) {
    return mosaic_cull(true, "sucre_mosaic_cull_supported", table_dev, n_images, images, first_ordinal, grid, top_dev, tol, J_out, culled_dev,
                       culled_above_dev, counts_dev, stream);
}

/* ---- per-image gain compensation of the mosaic: the span of ordinals per cell, J x gain, the ten sums per image (gains_mosaic.h) ---- */

// The rows of gains_dev (and sums_dev) the call's ordinals index: all of them must exist.
static int check_gain_rows(int n_images, int first_ordinal, int n_ordinals) {
    if (n_ordinals < 1 || n_ordinals > kMaxViews) return fail(SUCRE_ERR_ARG, "n_ordinals=%d outside [1,%d]", n_ordinals, kMaxViews);
    if (first_ordinal + n_images > n_ordinals)
        return fail(SUCRE_ERR_ARG, "ordinals %d..%d outside the %d rows of the gain table", first_ordinal, first_ordinal + n_images - 1, n_ordinals);
    return SUCRE_OK;
}

int sucre_mosaic_gain_span(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, uint32_t *span_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!span_dev || !aligned(span_dev, 8)) return fail(SUCRE_ERR_ARG, "span_dev is NULL or not 8-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_gain_span((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, span_dev,
                                             static_cast<hipStream_t>(stream)), "sucre_mosaic_gain_span");
}

int sucre_mosaic_gain_apply(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal, const float *gains_dev,
                            int n_ordinals, float *J_out, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    if (int rc = check_gain_rows(n_images, first_ordinal, n_ordinals)) return rc;
    if (!gains_dev || !aligned(gains_dev, 4)) return fail(SUCRE_ERR_ARG, "gains_dev is NULL or not 4-byte aligned");
    if (!J_out || !aligned(J_out, 4)) return fail(SUCRE_ERR_ARG, "J_out is NULL or not 4-byte aligned");
    if (int rc = check_copy_out(J_out, n_images, images, true)) return rc;   // an image's J may be its own block of J_out
    return check_hip(launch_mosaic_gain_apply(table_dev, n_images, images, first_ordinal, gains_dev, J_out, static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_gain_apply");
}

int sucre_mosaic_gain_sums(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const int64_t *acc_dev, const float *gains_dev,
                           int n_ordinals, int64_t *sums_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (int rc = check_gain_rows(n_images, first_ordinal, n_ordinals)) return rc;
    for (int i = 0; i < n_images; ++i)
        if ((uint64_t)images[i].H * (uint64_t)images[i].W > kGainMaxPixels)
            return fail(SUCRE_ERR_ARG, "image %d: %dx%d pixels, more than the 2^26 whose sums stay below 2^62", i, images[i].W, images[i].H);
    if (!span_dev || !aligned(span_dev, 8)) return fail(SUCRE_ERR_ARG, "span_dev is NULL or not 8-byte aligned");
    if (!acc_dev || !aligned(acc_dev, 8)) return fail(SUCRE_ERR_ARG, "acc_dev is NULL or not 8-byte aligned");
    if (!gains_dev || !aligned(gains_dev, 4)) return fail(SUCRE_ERR_ARG, "gains_dev is NULL or not 4-byte aligned");
    if (!sums_dev || !aligned(sums_dev, 128)) return fail(SUCRE_ERR_ARG, "sums_dev is NULL or not 128-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_gain_sums((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, span_dev,
                                             reinterpret_cast<const long long *>(acc_dev), gains_dev,
                                             reinterpret_cast<unsigned long long *>(sums_dev), static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_gain_sums");
}

/* ---- the direct solve of the gain compensation: a cell's slots, the pair sums, the diag (gains_direct.h) ---- */

static int check_gain_slot_state(const uint32_t *span_dev, const void *slot_ord_dev, const void *slot_sum_dev, const void *slot_over_dev,
                                 bool need_slots) {
    if (!span_dev || !aligned(span_dev, 8)) return fail(SUCRE_ERR_ARG, "span_dev is NULL or not 8-byte aligned");
    if (need_slots && (!slot_ord_dev || !aligned(slot_ord_dev, 4))) return fail(SUCRE_ERR_ARG, "slot_ord_dev is NULL or not 4-byte aligned");
    if (need_slots && (!slot_sum_dev || !aligned(slot_sum_dev, 8))) return fail(SUCRE_ERR_ARG, "slot_sum_dev is NULL or not 8-byte aligned");
    if (!slot_over_dev || !aligned(slot_over_dev, 4)) return fail(SUCRE_ERR_ARG, "slot_over_dev is NULL or not 4-byte aligned");
    return SUCRE_OK;
}

int sucre_mosaic_gain_slots(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                            const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, uint32_t *slot_ord_dev, int64_t *slot_sum_dev,
                            uint32_t *slot_over_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (int rc = check_gain_slot_state(span_dev, slot_ord_dev, slot_sum_dev, slot_over_dev, true)) return rc;
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_gain_slots((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, span_dev,
                                              slot_ord_dev, reinterpret_cast<unsigned long long *>(slot_sum_dev), slot_over_dev,
                                              static_cast<hipStream_t>(stream)), "sucre_mosaic_gain_slots");
}

int sucre_mosaic_gain_pairs(const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const uint32_t *slot_ord_dev,
                            const int64_t *slot_sum_dev, const uint32_t *slot_over_dev, int n_ordinals, int64_t *pairs_dev, int table_entries,
                            unsigned flags, void *stream) {
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    // ceil(cells / kPairTileCells) workgroups must stay within the 2^31 - 1 of a launch
    if ((uint64_t)g.Hm * (uint64_t)g.Wm >= (1ull << 43)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: the pairs take fewer than 2^43", g.Wm, g.Hm);
    if (int rc = check_gain_slot_state(span_dev, slot_ord_dev, slot_sum_dev, slot_over_dev, true)) return rc;
    if (n_ordinals < 1 || n_ordinals > kMaxViews) return fail(SUCRE_ERR_ARG, "n_ordinals=%d outside [1,%d]", n_ordinals, kMaxViews);
    if (!pairs_dev || !aligned(pairs_dev, 8)) return fail(SUCRE_ERR_ARG, "pairs_dev is NULL or not 8-byte aligned");
    if (table_entries == 0) table_entries = kPairTableMax;
    if (table_entries < 1 || table_entries > kPairTableMax || (table_entries & (table_entries - 1)))
        return fail(SUCRE_ERR_ARG, "table_entries=%d is not 0 or a power of two within [1,%d]", table_entries, kPairTableMax);
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_gain_pairs((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, g, span_dev, slot_ord_dev,
                                              reinterpret_cast<const long long *>(slot_sum_dev), slot_over_dev, n_ordinals,
                                              reinterpret_cast<unsigned long long *>(pairs_dev), table_entries, static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_gain_pairs");
}

int sucre_mosaic_gain_diag(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                           const sucre_mosaic_grid_t *grid, const uint32_t *span_dev, const uint32_t *slot_over_dev, int n_ordinals,
                           int64_t *diag_dev, unsigned flags, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (int rc = check_gain_rows(n_images, first_ordinal, n_ordinals)) return rc;
    for (int i = 0; i < n_images; ++i)
        if ((uint64_t)images[i].H * (uint64_t)images[i].W > kGainMaxPixels)
            return fail(SUCRE_ERR_ARG, "image %d: %dx%d pixels, more than the 2^26 whose sums stay below 2^62", i, images[i].W, images[i].H);
    if (int rc = check_gain_slot_state(span_dev, nullptr, nullptr, slot_over_dev, false)) return rc;
    if (!diag_dev || !aligned(diag_dev, 128)) return fail(SUCRE_ERR_ARG, "diag_dev is NULL or not 128-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_gain_diag((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g, span_dev,
                                             slot_over_dev, reinterpret_cast<unsigned long long *>(diag_dev), static_cast<hipStream_t>(stream)),
                     "sucre_mosaic_gain_diag");
}

/* ---- colour consensus across views: a cell's eight smallest ordinals, their sums, the median image, the cull (reject.h) ---- */

int sucre_mosaic_reject_claim(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                              const sucre_mosaic_grid_t *grid, uint32_t *slot_ord_dev, uint32_t *slot_over_dev, unsigned flags,
                              void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!slot_ord_dev || !aligned(slot_ord_dev, 32)) return fail(SUCRE_ERR_ARG, "slot_ord_dev is NULL or not 32-byte aligned");
    if (!slot_over_dev || !aligned(slot_over_dev, 4)) return fail(SUCRE_ERR_ARG, "slot_over_dev is NULL or not 4-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_reject_claim((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g,
                                                slot_ord_dev, slot_over_dev, static_cast<hipStream_t>(stream)), "sucre_mosaic_reject_claim");
}

int sucre_mosaic_reject_sums(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                             const sucre_mosaic_grid_t *grid, const uint32_t *slot_ord_dev, int64_t *slot_sum_dev, unsigned flags,
                             void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!slot_ord_dev || !aligned(slot_ord_dev, 32)) return fail(SUCRE_ERR_ARG, "slot_ord_dev is NULL or not 32-byte aligned");
    if (!slot_sum_dev || !aligned(slot_sum_dev, 8)) return fail(SUCRE_ERR_ARG, "slot_sum_dev is NULL or not 8-byte aligned");
    if (int rc = check_mosaic_flags(flags)) return rc;
    return check_hip(launch_mosaic_reject_sums((flags & SUCRE_MOSAIC_PLAIN_ATOMIC) != 0, table_dev, n_images, images, first_ordinal, g,
                                               slot_ord_dev, reinterpret_cast<unsigned long long *>(slot_sum_dev),
                                               static_cast<hipStream_t>(stream)), "sucre_mosaic_reject_sums");
}

int sucre_mosaic_reject_consensus(const sucre_mosaic_grid_t *grid, const uint32_t *slot_ord_dev, const int64_t *slot_sum_dev,
                                  float *ref_out, int32_t *source_out, int32_t *views_out, uint64_t *big_dev, void *stream) {
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if ((uint64_t)g.Hm * (uint64_t)g.Wm > (1ull << 39)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: one pass takes 2^39 cells", g.Wm, g.Hm);
    if (!slot_ord_dev || !aligned(slot_ord_dev, 32)) return fail(SUCRE_ERR_ARG, "slot_ord_dev is NULL or not 32-byte aligned");
    if (!slot_sum_dev || !aligned(slot_sum_dev, 8)) return fail(SUCRE_ERR_ARG, "slot_sum_dev is NULL or not 8-byte aligned");
    if (!ref_out || !aligned(ref_out, 4)) return fail(SUCRE_ERR_ARG, "ref_out is NULL or not 4-byte aligned");
    if (!source_out || !aligned(source_out, 4)) return fail(SUCRE_ERR_ARG, "source_out is NULL or not 4-byte aligned");
    if (!views_out || !aligned(views_out, 4)) return fail(SUCRE_ERR_ARG, "views_out is NULL or not 4-byte aligned");
    if (!big_dev || !aligned(big_dev, 8)) return fail(SUCRE_ERR_ARG, "big_dev is NULL or not 8-byte aligned");
    return check_hip(launch_mosaic_reject_consensus(g, slot_ord_dev, reinterpret_cast<const long long *>(slot_sum_dev), ref_out, source_out,
                                                    views_out, reinterpret_cast<unsigned long long *>(big_dev),
                                                    static_cast<hipStream_t>(stream)), "sucre_mosaic_reject_consensus");
}

int sucre_mosaic_reject_cull(void *table_dev, int n_images, const sucre_mosaic_image_t *images, int first_ordinal,
                             const sucre_mosaic_grid_t *grid, const float *ref_dev, const int32_t *source_dev, float tol, float *J_out,
                             uint32_t *rejected_dev, int n_ordinals, int64_t *counts_dev, void *stream) {
    if (int rc = check_mosaic_images(table_dev, n_images, images, first_ordinal)) return rc;
    MosaicGrid g;
    if (int rc = check_mosaic_grid(grid, &g)) return rc;
    if (!ref_dev || !aligned(ref_dev, 4)) return fail(SUCRE_ERR_ARG, "ref_dev is NULL or not 4-byte aligned");
    if (!source_dev || !aligned(source_dev, 4)) return fail(SUCRE_ERR_ARG, "source_dev is NULL or not 4-byte aligned");
    if (!std::isfinite(tol) || !(tol > 0.0f)) return fail(SUCRE_ERR_ARG, "tol=%g must be finite and > 0", (double)tol);
    if (!J_out || !aligned(J_out, 4)) return fail(SUCRE_ERR_ARG, "J_out is NULL or not 4-byte aligned");
    if (rejected_dev && !aligned(rejected_dev, 4)) return fail(SUCRE_ERR_ARG, "rejected_dev is not 4-byte aligned");
    if (counts_dev) {   // every ordinal of the call has a row
        if (!aligned(counts_dev, 128)) return fail(SUCRE_ERR_ARG, "counts_dev is not 128-byte aligned");
        if (int rc = check_gain_rows(n_images, first_ordinal, n_ordinals)) return rc;
    }
    if (int rc = check_copy_out(J_out, n_images, images, false)) return rc;
    const MosaicReject out = {rejected_dev, reinterpret_cast<unsigned long long *>(counts_dev)};
    return check_hip(launch_mosaic_reject_cull(table_dev, n_images, images, first_ordinal, g, ref_dev, source_dev, tol, J_out, out,
                                               static_cast<hipStream_t>(stream)), "sucre_mosaic_reject_cull");
}

/* ---- hole filling of the finished mosaic: a bounded push-pull over a pyramid of the grid (fill.h) ---- */

}  // extern "C"

namespace sucre {

static int check_fill_geometry(int Hm, int Wm, int levels) {
    if (Hm < 1 || Wm < 1 || Hm > (1 << 24) || Wm > (1 << 24)) return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells (need 1..2^24 each way)", Wm, Hm);
    if ((uint64_t)Hm * (uint64_t)Wm > (1ull << 39) || fill_blocks(Hm, Wm) > 0x7fffffffull)
        return fail(SUCRE_ERR_ARG, "mosaic of %dx%d cells: one pass takes 2^39 cells", Wm, Hm);
    if (levels < 1 || levels > kFillMaxLevels) return fail(SUCRE_ERR_ARG, "levels=%d outside [1,%d]", levels, kFillMaxLevels);
    return SUCRE_OK;
}

static int check_fill_base(const float *J, const uint8_t *raw, const int32_t *source, const void *pyramid_dev) {
    if (!J || !aligned(J, 4)) return fail(SUCRE_ERR_ARG, "J is NULL or not 4-byte aligned");
    if (!raw) return fail(SUCRE_ERR_ARG, "raw is NULL");
    if (!source || !aligned(source, 4)) return fail(SUCRE_ERR_ARG, "source is NULL or not 4-byte aligned");
    if (!pyramid_dev || !aligned(pyramid_dev, 256)) return fail(SUCRE_ERR_ARG, "pyramid_dev is NULL or not 256-byte aligned");
    return SUCRE_OK;
}

}  // namespace sucre

extern "C" {

size_t sucre_mosaic_fill_bytes(int Hm, int Wm, int levels) {
    if (check_fill_geometry(Hm, Wm, levels)) return 0;
    return fill_pyramid_bytes(Hm, Wm, levels);
}

int sucre_mosaic_fill_pull(int Hm, int Wm, int levels, const float *J, const uint8_t *raw, const int32_t *source, void *pyramid_dev,
                           void *stream) {
    if (int rc = check_fill_geometry(Hm, Wm, levels)) return rc;
    if (int rc = check_fill_base(J, raw, source, pyramid_dev)) return rc;
    const FillBase base = {reinterpret_cast<const uint32_t *>(J), raw, source};
    return check_hip(launch_fill_pull(Hm, Wm, levels, base, pyramid_dev, static_cast<hipStream_t>(stream)), "sucre_mosaic_fill_pull");
}

int sucre_mosaic_fill_push(int Hm, int Wm, int levels, const float *J, const uint8_t *raw, const int32_t *source, void *pyramid_dev,
                           float *J_filled, uint8_t *raw_filled, int32_t *level_out, void *stream) {
    if (int rc = check_fill_geometry(Hm, Wm, levels)) return rc;
    if (int rc = check_fill_base(J, raw, source, pyramid_dev)) return rc;
    if (!J_filled || !aligned(J_filled, 4)) return fail(SUCRE_ERR_ARG, "J_filled is NULL or not 4-byte aligned");
    if (!raw_filled) return fail(SUCRE_ERR_ARG, "raw_filled is NULL");
    if (!level_out || !aligned(level_out, 4)) return fail(SUCRE_ERR_ARG, "level_out is NULL or not 4-byte aligned");
    const FillBase base = {reinterpret_cast<const uint32_t *>(J), raw, source};
    const FillOut out = {reinterpret_cast<uint32_t *>(J_filled), raw_filled, level_out};
    return check_hip(launch_fill_push(Hm, Wm, levels, base, pyramid_dev, out, static_cast<hipStream_t>(stream)), "sucre_mosaic_fill_push");
}

/* ---- shared water and light over the light-model images of a rank (sucre.py:54-61, 124-157) ------------------------ */

}  // extern "C"

namespace sucre {

// What the iterations of a light group need on the host -- every image's layout and buffers, which iteration is next, which
// mode the gradient launches' deals in the light workspaces were written for -- kept from sucre_light_group_init on,
// keyed by the group buffer (the device buffer itself is never read back: the loop has no host synchronisation).
struct LightGroupHost {
    std::vector<Layout> L;
    std::vector<uint8_t *> ws, lws;
    int steps_done = 0;
    int deal_mode = -1;   // -1: no deal written yet, else the SUCRE_FIT_CLOSED_FORM bit of the launches it was written for
};
static std::mutex g_light_groups_lock;
static std::map<const void *, LightGroupHost> g_light_groups;

static int check_light_group_flags(unsigned flags) {
    if (flags & (SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH))
        return fail(SUCRE_ERR_ARG, "light groups run on uint8 colours: SUCRE_FIT_EXT_COLOUR / SUCRE_FIT_EXT_BOTH are not supported");
    if (flags & SUCRE_FIT_OBS_U16MM) return fail(SUCRE_ERR_ARG, "light groups need the f32 store (SUCRE_FIT_OBS_U16MM given)");
    if (flags & ~SUCRE_FIT_CLOSED_FORM) return fail(SUCRE_ERR_ARG, "unknown light group flags 0x%x", flags);
    return SUCRE_OK;
}

// The group's host table (under the lock), after the checks every iter / finish call makes.
static int light_group_of(void *group_dev, int n_images, LightGroupHost **out) {
    if (!group_dev || n_images < 1) return fail(SUCRE_ERR_ARG, "light group buffer is NULL / no image");
    auto it = g_light_groups.find(group_dev);
    if (it == g_light_groups.end()) return fail(SUCRE_ERR_ARG, "light group buffer was not set up by sucre_light_group_init");
    if ((int)it->second.L.size() != n_images)
        return fail(SUCRE_ERR_ARG, "light group holds %d images, not %d", (int)it->second.L.size(), n_images);
    *out = &it->second;
    return SUCRE_OK;
}

}  // namespace sucre

extern "C" {

size_t sucre_light_group_bytes(int n_images) { return n_images > 0 ? light_group_bytes(n_images) : 0; }

int64_t sucre_light_group_sums_offset(void) { return light_group_sums_offset(); }

int sucre_light_group_init(void *group_dev, int n_images, const sucre_light_group_image_t *images, const float *params0, void *stream) {
    if (!group_dev || !aligned(group_dev, 256)) return fail(SUCRE_ERR_ARG, "light group buffer is NULL or not 256-byte aligned");
    if (n_images < 1 || !images || !params0) return fail(SUCRE_ERR_ARG, "need at least one image and params0");
    LightGroupHost h;
    for (int i = 0; i < n_images; ++i) {
        Layout L;
        if (int rc = check_ws(images[i].ws, images[i].H, images[i].W, images[i].n_views, &L)) return rc;
        if (int rc = check_lws(images[i].lws)) return rc;
        h.L.push_back(L);
        h.ws.push_back(static_cast<uint8_t *>(images[i].ws));
        h.lws.push_back(static_cast<uint8_t *>(images[i].lws));
    }
    std::lock_guard<std::mutex> hold(g_light_groups_lock);
    LightGroupHost &g = g_light_groups[group_dev] = std::move(h);
    return check_hip(launch_light_group_init(group_dev, n_images, g.L.data(), g.ws.data(), g.lws.data(), params0,
                                             static_cast<hipStream_t>(stream)), "sucre_light_group_init");
}

int sucre_light_group_iter(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                           unsigned flags, uint64_t n_obs_total, double *trace_dev, void *stream) {
    if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (int rc = check_light_group_flags(flags)) return rc;
    if (n_obs_total == 0) return fail(SUCRE_ERR_RANGE, "n_obs_total must be > 0");
    if (trace_dev && !aligned(trace_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    std::lock_guard<std::mutex> hold(g_light_groups_lock);
    LightGroupHost *g;
    if (int rc = light_group_of(group_dev, n_images, &g)) return rc;
    if (step != g->steps_done + 1)
        return fail(SUCRE_ERR_RANGE, "light group: iteration %d asked after %d done -- iterations run in order, once "
                                     "(sucre_light_group_init starts over)", step, g->steps_done);
    const int mode = (flags & SUCRE_FIT_CLOSED_FORM) ? 1 : 0;
    const AdamCoef co_prev = adam_coef(step > 1 ? step - 1 : 1, lr, beta1, beta2, eps);
    double *row = (trace_dev && step > 1) ? trace_dev + (size_t)(step - 2) * 20 : nullptr;
    if (int rc = check_hip(launch_light_group_iter(group_dev, n_images, g->L.data(), g->ws.data(), g->lws.data(), step, co_prev,
                                                   adam_coef(step, lr, beta1, beta2, eps), flags, n_obs_total, row,
                                                   g->deal_mode != mode, static_cast<hipStream_t>(stream)),
                           "sucre_light_group_iter")) return rc;
    g->deal_mode = mode;
    g->steps_done = step;
    return SUCRE_OK;
}

int sucre_light_group_finish(void *group_dev, int n_images, int step, double lr, double beta1, double beta2, double eps,
                             unsigned flags, uint64_t n_obs_total, double *trace_dev, void *stream) {
    if (step < 0) return fail(SUCRE_ERR_RANGE, "step=%d must be >= 0", step);
    if (step >= 1) if (int rc = check_adam(step, lr, beta1, beta2, eps)) return rc;
    if (int rc = check_light_group_flags(flags)) return rc;
    if (n_obs_total == 0) return fail(SUCRE_ERR_RANGE, "n_obs_total must be > 0");
    if (trace_dev && !aligned(trace_dev, 8)) return fail(SUCRE_ERR_ARG, "trace must be 8-byte aligned");
    std::lock_guard<std::mutex> hold(g_light_groups_lock);
    LightGroupHost *g;
    if (int rc = light_group_of(group_dev, n_images, &g)) return rc;
    if (step != g->steps_done)
        return fail(SUCRE_ERR_RANGE, "light group: finish after iteration %d, but %d ran -- iterations run in order", step, g->steps_done);
    double *row = (trace_dev && step >= 1) ? trace_dev + (size_t)(step - 1) * 20 : nullptr;
    return check_hip(launch_light_group_finish(group_dev, n_images, g->L.data(), g->ws.data(), g->lws.data(), step,
                                               adam_coef(step >= 1 ? step : 1, lr, beta1, beta2, eps), flags, n_obs_total, row,
                                               static_cast<hipStream_t>(stream)), "sucre_light_group_finish");
}

}  // extern "C"

/* ---- standard errors of the water parameters and of J ------------------------------------------------------------------- */

namespace sucre {
static int check_uncertainty_outputs(const int32_t *count_dev, const float *jterms_dev, const double *sums_dev, const void *scratch_dev) {
    if (!count_dev || !jterms_dev || !sums_dev || !scratch_dev) return fail(SUCRE_ERR_ARG, "count_dev / jterms_dev / sums_dev / scratch_dev is NULL");
    if (!aligned(count_dev, 4) || !aligned(jterms_dev, 16) || !aligned(sums_dev, 8)) return fail(SUCRE_ERR_ARG, "outputs must be 4 / 16 / 8-byte aligned");
    if (!aligned(scratch_dev, 16)) return fail(SUCRE_ERR_ARG, "scratch_dev must be 16-byte aligned");
    return SUCRE_OK;
}
}  // namespace sucre

extern "C" {

size_t sucre_uncertainty_scratch_bytes(int H, int W, int n_views) {
    Layout L;
    if (!make_layout(H, W, n_views, &L)) {
        fail(SUCRE_ERR_ARG, "invalid geometry H=%d W=%d n_views=%d", H, W, n_views);
        return 0;
    }
    return uncertainty_scratch_bytes(L);
}

int sucre_fit_uncertainty(const void *ws, int H, int W, int n_views, int obs_format, int32_t *count_dev, float *jterms_dev,
                          double *sums_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (obs_format != SUCRE_OBS_F32 && obs_format != SUCRE_OBS_U16MM && obs_format != SUCRE_OBS_F32_PLAIN && obs_format != SUCRE_OBS_F32_Z26)
        return fail(SUCRE_ERR_ARG, "unknown observation format %d", obs_format);
    if (int rc = check_uncertainty_outputs(count_dev, jterms_dev, sums_dev, scratch_dev)) return rc;
    return check_hip(launch_uncertainty(L, static_cast<const uint8_t *>(ws), obs_format == SUCRE_OBS_U16MM ? SUCRE_OBS_U16MM : SUCRE_OBS_F32,
                                        count_dev, jterms_dev, sums_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_fit_uncertainty");
}

int sucre_fit_uncertainty_ext(const void *ws, const void *lws, int H, int W, int n_views, unsigned flags, int32_t *count_dev,
                              float *jterms_dev, double *sums_dev, void *scratch_dev, void *stream) {
    Layout L;
    if (int rc = check_ws(ws, H, W, n_views, &L)) return rc;
    if (int rc = check_lws(lws)) return rc;
    if (flags & ~(SUCRE_FIT_EXT_COLOUR | SUCRE_FIT_EXT_BOTH)) return fail(SUCRE_ERR_ARG, "unknown flags 0x%x", flags);
    if (flags != SUCRE_FIT_EXT_COLOUR)
        return fail(SUCRE_ERR_ARG, "flags 0x%x name the light model, whose uncertainty is not built: the lamp's parameters would have to "
                                   "join B, beta, gamma (only SUCRE_FIT_EXT_COLOUR is taken)", flags);
    if (int rc = check_uncertainty_outputs(count_dev, jterms_dev, sums_dev, scratch_dev)) return rc;
    return check_hip(launch_uncertainty_colour(L, static_cast<const uint8_t *>(ws), static_cast<const uint8_t *>(lws), count_dev,
                                               jterms_dev, sums_dev, scratch_dev, static_cast<hipStream_t>(stream)),
                     "sucre_fit_uncertainty_ext");
}

}  // extern "C"
