/* nwe_render_adaptive from plain C on a host-only context: every refusal in front of the host-only one, by code, text and order, the
 * lattice call and the report of a context that has rendered no adaptive frame.  Built and run by `make asan` beside abi_smoke.c,
 * host code only; no GPU needed. */
#include <math.h>
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

/* the call with a good camera but for H, W and far, which the cases vary */
static int adaptive(nwe_ctx *ctx, int H, int W, float far, int precision, int k, float tol_rgb, float tol_depth, const nwe_adaptive_outputs *out) {
    return nwe_render_adaptive(ctx, pose, 1, H, W, 2.f, 2.f, 2.f, 1.5f, 0.1f, far, 0, H > 0 ? H : 0, precision, k, tol_rgb, tol_depth, out, NULL);
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
    float rgb[4 * 5 * 3];
    memset(rgb, 0x5a, sizeof(rgb));
    nwe_adaptive_outputs good = {0}, none = {0}, stale = {0};
    uint8_t kind[4 * 5];
    uint32_t flags = 0;
    memset(kind, 0x5a, sizeof(kind));
    good.struct_bytes = none.struct_bytes = sizeof(nwe_adaptive_outputs);
    stale.struct_bytes = sizeof(nwe_adaptive_outputs) - 8;
    good.rgb = stale.rgb = rgb;
    good.kind = none.kind = kind;
    good.flags = none.flags = &flags;
    const float nan = nanf("");
    /* each call is wrong in everything behind the refusal it expects as well */
    CHECK(adaptive(NULL, 0, 5, 0.f, 9, 0, nan, nan, NULL) == NWE_ERR_INVALID);
    REFUSED(adaptive(ctx, 0, 5, 0.f, 9, 0, nan, nan, NULL), NWE_ERR_INVALID, "null outputs");
    CHECK(adaptive(ctx, 0, 5, 0.f, 9, 0, nan, nan, &stale) == NWE_ERR_INVALID && strstr(nwe_last_error(ctx), "nwe_adaptive_outputs.struct_bytes") != NULL);
    REFUSED(adaptive(ctx, 0, 5, 0.f, 9, 0, nan, nan, &none), NWE_ERR_INVALID, "none of rgb / depth / acc requested");
    REFUSED(adaptive(ctx, 0, 5, 0.f, 9, 0, nan, nan, &good), NWE_ERR_INVALID, "bad pose / image / row range");
    REFUSED(adaptive(ctx, 4, 5, 0.f, 9, 0, nan, nan, &good), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths");
    REFUSED(adaptive(ctx, 4097, 4096, 5.f, 9, 0, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: more than 2^24 rays in one call");
    REFUSED(adaptive(ctx, 4096, 4096, 5.f, 9, 0, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: k must be in 1..64");
    REFUSED(adaptive(ctx, 4, 5, 5.f, 9, 65, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: k must be in 1..64");
    REFUSED(adaptive(ctx, 4, 5, 5.f, 9, 64, nan, 0.f, &good), NWE_ERR_INVALID, "adaptive frame: the tolerances must not be NaN");
    REFUSED(adaptive(ctx, 4, 5, 5.f, 9, 1, 0.f, nan, &good), NWE_ERR_INVALID, "adaptive frame: the tolerances must not be NaN");
    REFUSED(adaptive(ctx, 4, 5, 5.f, 9, 1, -INFINITY, INFINITY, &good), NWE_ERR_INVALID, "unknown precision");
    REFUSED(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "nwe_set_sampling has not been called");
    {
        float t[4] = {0.f, 1.f / 3, 2.f / 3, 1.f}, omt[4] = {1.f, 2.f / 3, 1.f / 3, 0.f}, u[2] = {0.f, 1.f};
        CHECK(nwe_set_sampling(ctx, t, omt, 4, u, 2) == NWE_OK);
    }
    REFUSED(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "coarse network not set");
    CHECK(set_network(ctx, NWE_NET_COARSE) == NWE_OK);
    REFUSED(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "fine network not set but n_importance > 0");
    CHECK(set_network(ctx, NWE_NET_FINE) == NWE_OK);
    /* a 2x8 network has no MFMA kernel: refused for the MFMA precisions in front of the host-only refusal, as nwe_render_rays plans it */
    CHECK(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F16X3, 2, 0.01f, 0.05f, &good) == NWE_ERR_UNSUPPORTED &&
          strstr(nwe_last_error(ctx), "no MFMA kernel for this network shape") == nwe_last_error(ctx));
    /* a mode the call cannot serve, in nwe_render_rays' words */
    CHECK(nwe_set_early_termination(ctx, 0.01f) == NWE_OK);
    CHECK(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 0.01f, 0.05f, &good) == NWE_ERR_UNSUPPORTED &&
          strstr(nwe_last_error(ctx), "early termination is on") == nwe_last_error(ctx));
    CHECK(nwe_set_early_termination(ctx, 0.f) == NWE_OK);
    /* the last refusal a host-only context can give, zero rays included */
    REFUSED(adaptive(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "host-only context cannot render");
    REFUSED(nwe_render_adaptive(ctx, pose, 1, 4, 5, 2.f, 2.f, 2.f, 1.5f, 0.1f, 5.f, 2, 2, NWE_PREC_F32, 64, -1.f, INFINITY, &good, NULL), NWE_ERR_STATE,
            "host-only context cannot render");
    /* a refused call writes nothing and there is no report of a call that never ran */
    for (size_t i = 0; i < sizeof(rgb); ++i) CHECK(((unsigned char *)rgb)[i] == 0x5a);
    for (size_t i = 0; i < sizeof(kind); ++i) CHECK(kind[i] == 0x5a);
    CHECK(flags == 0);
    int64_t counts[4] = {-7, -7, -7, -7};
    float ms = -7.f;
    CHECK(nwe_last_adaptive(ctx, counts, &ms) == NWE_ERR_STATE && counts[0] == -7 && counts[3] == -7 && ms == -7.f);
    CHECK(nwe_last_adaptive(ctx, NULL, &ms) == NWE_ERR_INVALID && nwe_last_adaptive(NULL, counts, NULL) == NWE_ERR_INVALID);
    CHECK(nwe_last_kernel_ms(ctx) < 0.f && nwe_debug_last_plan(ctx) == -1);
    /* the lattice call: needs no context */
    int32_t lat[64];
    CHECK(nwe_debug_adaptive_lattice(0, 37, 5, lat, 64) == 9 && lat[0] == 0 && lat[1] == 5 && lat[7] == 35 && lat[8] == 36);
    CHECK(nwe_debug_adaptive_lattice(5, 30, 5, lat, 64) == 6 && lat[0] == 5 && lat[4] == 25 && lat[5] == 29);
    CHECK(nwe_debug_adaptive_lattice(0, 45, 4, lat, 12) == 12 && lat[11] == 44);
    CHECK(nwe_debug_adaptive_lattice(7, 8, 64, lat, 1) == 1 && lat[0] == 7);
    CHECK(nwe_debug_adaptive_lattice(0, 37, 64, lat, 2) == 2 && lat[0] == 0 && lat[1] == 36);
    CHECK(nwe_debug_adaptive_lattice(0, 45, 4, lat, 11) == -1 && nwe_debug_adaptive_lattice(0, 45, 0, lat, 64) == -1);
    CHECK(nwe_debug_adaptive_lattice(0, 45, 65, lat, 64) == -1 && nwe_debug_adaptive_lattice(3, 3, 2, lat, 64) == -1);
    CHECK(nwe_debug_adaptive_lattice(0, 45, 2, NULL, 64) == -1 && nwe_debug_adaptive_lattice(0, 2147483647, 64, lat, 64) == -1);
    nwe_destroy(ctx);
    printf("adaptive_smoke ok\n");
    return 0;
}
