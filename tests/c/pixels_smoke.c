/* nwe_render_pixels and nwe_set_adaptive_pixel_lists from plain C on a host-only context: every refusal that needs no device, by
 * code, text and order, the switch, the path decision and the report of a context that has rendered no pixel list.  Built and run by
 * `make asan` beside adaptive_smoke.c, host code only; no GPU needed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nwe.h"

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)
#define REFUSED(call, code, text) CHECK((call) == (code) && strcmp(nwe_last_error(ctx), (text)) == 0)

static float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static int32_t list[3] = {0, 7, 19};   /* never read: every call refuses */

/* the call with a good camera but for H and far, which the cases vary */
static int pixels(nwe_ctx *ctx, int H, float far, const int32_t *px, int64_t n, int precision, const nwe_pixel_outputs *out) {
    return nwe_render_pixels(ctx, pose, 1, H, 5, 2.f, 2.f, 2.f, 1.5f, 0.1f, far, 0, H > 0 ? H : 0, px, n, precision, out, NULL);
}

static int set_network(nwe_ctx *ctx, int which) {
    enum { D = 2, W = 8, IN_XYZ = 63, IN_DIR = 27 };
    const int ins[D + 4] = {IN_XYZ, W, W + IN_DIR, W, W, W / 2};
    const int outs[D + 4] = {W, W, W / 2, W, 1, 3};
    float *w[D + 4], *b[D + 4];
    for (int l = 0; l < D + 4; ++l) {
        w[l] = (float *)calloc((size_t)ins[l] * outs[l], sizeof(float));
        b[l] = (float *)calloc((size_t)outs[l], sizeof(float));
    }
    const int rc = nwe_set_network(ctx, which, D, W, IN_XYZ, IN_DIR, -1, (const float *const *)w, (const float *const *)b);
    for (int l = 0; l < D + 4; ++l) {
        free(w[l]);
        free(b[l]);
    }
    return rc;
}

int main(void) {
    nwe_ctx *ctx = NULL;
    CHECK(nwe_create(&ctx, -1) == NWE_OK && ctx);
    float rgb[3 * 3];
    memset(rgb, 0x5a, sizeof(rgb));
    nwe_pixel_outputs good = {0}, none = {0}, stale = {0};
    uint32_t flags = 0;
    good.struct_bytes = none.struct_bytes = sizeof(nwe_pixel_outputs);
    stale.struct_bytes = sizeof(nwe_pixel_outputs) - 8;
    good.rgb = stale.rgb = rgb;
    good.flags = none.flags = &flags;
    const int64_t too_many = (int64_t)1 << 31;
    /* each call is wrong in everything behind the refusal it expects as well */
    CHECK(pixels(NULL, 0, 0.f, NULL, -1, 9, NULL) == NWE_ERR_INVALID);
    REFUSED(pixels(ctx, 0, 0.f, NULL, -1, 9, NULL), NWE_ERR_INVALID, "null outputs");
    CHECK(pixels(ctx, 0, 0.f, NULL, -1, 9, &stale) == NWE_ERR_INVALID && strstr(nwe_last_error(ctx), "nwe_pixel_outputs.struct_bytes") != NULL);
    REFUSED(pixels(ctx, 0, 0.f, NULL, -1, 9, &none), NWE_ERR_INVALID, "none of rgb / depth / acc requested");
    REFUSED(pixels(ctx, 0, 0.f, NULL, -1, 9, &good), NWE_ERR_INVALID, "bad pose / image / row range");
    REFUSED(pixels(ctx, 4, 0.f, NULL, -1, 9, &good), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths");
    REFUSED(pixels(ctx, 4, 5.f, list, -1, 9, &good), NWE_ERR_INVALID, "bad pixels (null, a negative count, or more than 2^31 - 1)");
    REFUSED(pixels(ctx, 4, 5.f, list, too_many, 9, &good), NWE_ERR_INVALID, "bad pixels (null, a negative count, or more than 2^31 - 1)");
    REFUSED(pixels(ctx, 4, 5.f, NULL, 3, 9, &good), NWE_ERR_INVALID, "bad pixels (null, a negative count, or more than 2^31 - 1)");
    REFUSED(pixels(ctx, 4, 5.f, list, too_many - 1, 9, &good), NWE_ERR_INVALID, "unknown precision");
    REFUSED(pixels(ctx, 4, 5.f, NULL, 0, 9, &good), NWE_ERR_INVALID, "unknown precision");
    REFUSED(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good), NWE_ERR_STATE, "nwe_set_sampling has not been called");
    {
        float t[4] = {0.f, 1.f / 3, 2.f / 3, 1.f}, omt[4] = {1.f, 2.f / 3, 1.f / 3, 0.f}, u[2] = {0.f, 1.f};
        CHECK(nwe_set_sampling(ctx, t, omt, 4, u, 2) == NWE_OK);
    }
    REFUSED(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good), NWE_ERR_STATE, "coarse network not set");
    CHECK(nwe_debug_pixels_path(ctx, NWE_PREC_F16X3) == 0);
    CHECK(set_network(ctx, NWE_NET_COARSE) == NWE_OK);
    REFUSED(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good), NWE_ERR_STATE, "fine network not set but n_importance > 0");
    CHECK(set_network(ctx, NWE_NET_FINE) == NWE_OK);
    /* a 2x8 network has no MFMA kernel: refused for the MFMA precisions in front of the host-only refusal, and no list kernel serves it */
    CHECK(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F16X3, &good) == NWE_ERR_UNSUPPORTED &&
          strstr(nwe_last_error(ctx), "no MFMA kernel for this network shape") == nwe_last_error(ctx));
    CHECK(nwe_debug_pixels_path(ctx, NWE_PREC_F16X3) == 0 && nwe_debug_pixels_path(ctx, NWE_PREC_F16X1) == 0 && nwe_debug_pixels_path(ctx, NWE_PREC_F32) == 0);
    CHECK(nwe_debug_pixels_path(ctx, 9) == -1 && nwe_debug_pixels_path(NULL, NWE_PREC_F32) == -1);
    /* a mode the call cannot serve, in nwe_render_rays' words */
    CHECK(nwe_set_early_termination(ctx, 0.01f) == NWE_OK);
    CHECK(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good) == NWE_ERR_UNSUPPORTED && strstr(nwe_last_error(ctx), "early termination is on") == nwe_last_error(ctx));
    CHECK(nwe_set_early_termination(ctx, 0.f) == NWE_OK);
    CHECK(nwe_set_shared_coarse(ctx, 2) == NWE_OK);
    CHECK(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good) == NWE_ERR_UNSUPPORTED && strstr(nwe_last_error(ctx), "the shared coarse pass is on") == nwe_last_error(ctx));
    CHECK(nwe_set_shared_coarse(ctx, 1) == NWE_OK);
    /* the last refusal a host-only context can give, no pixels included */
    REFUSED(pixels(ctx, 4, 5.f, list, 3, NWE_PREC_F32, &good), NWE_ERR_STATE, "host-only context cannot render");
    REFUSED(pixels(ctx, 4, 5.f, NULL, 0, NWE_PREC_F32, &good), NWE_ERR_STATE, "host-only context cannot render");
    /* a refused call writes nothing and there is no report of a call that never ran */
    for (size_t i = 0; i < sizeof(rgb); ++i) CHECK(((unsigned char *)rgb)[i] == 0x5a);
    CHECK(flags == 0);
    int64_t n = -7;
    int path = -7;
    CHECK(nwe_last_pixels(ctx, &n, &path) == NWE_ERR_STATE && n == -7 && path == -7);
    CHECK(nwe_last_pixels(ctx, NULL, &path) == NWE_ERR_INVALID && nwe_last_pixels(ctx, &n, NULL) == NWE_ERR_INVALID && nwe_last_pixels(NULL, &n, &path) == NWE_ERR_INVALID);
    CHECK(nwe_last_kernel_ms(ctx) < 0.f && nwe_debug_last_plan(ctx) == -1);
    /* the switch: host-side, 0 or 1 */
    CHECK(nwe_get_adaptive_pixel_lists(NULL) == -1 && nwe_set_adaptive_pixel_lists(NULL, 1) == NWE_ERR_INVALID);
    CHECK(nwe_get_adaptive_pixel_lists(ctx) == 0);
    REFUSED(nwe_set_adaptive_pixel_lists(ctx, 2), NWE_ERR_INVALID, "adaptive_pixel_lists must be 0 or 1 (0 = off)");
    REFUSED(nwe_set_adaptive_pixel_lists(ctx, -1), NWE_ERR_INVALID, "adaptive_pixel_lists must be 0 or 1 (0 = off)");
    CHECK(nwe_get_adaptive_pixel_lists(ctx) == 0);
    CHECK(nwe_set_adaptive_pixel_lists(ctx, 1) == NWE_OK && nwe_get_adaptive_pixel_lists(ctx) == 1);
    CHECK(nwe_set_adaptive_pixel_lists(ctx, 0) == NWE_OK && nwe_get_adaptive_pixel_lists(ctx) == 0);
    nwe_destroy(ctx);
    printf("pixels_smoke ok\n");
    return 0;
}
