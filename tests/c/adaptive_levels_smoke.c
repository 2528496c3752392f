/* nwe_render_adaptive_levels from plain C on a host-only context: every refusal in front of the host-only one, by code, text and
 * order - the one-level call's, with the levels refusal directly behind k -, the lattice and the plan call and the report of a
 * context that has rendered no such frame.  Built and run by `make asan` beside adaptive_smoke.c, host code only; no GPU needed. */
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
#define LEVELS_TEXT "adaptive frame: levels must be in 1..4 and k * 2^(levels - 1) at most 64"

static float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

/* the call with a good camera but for H, W and far, which the cases vary */
static int levels(nwe_ctx *ctx, int H, int W, float far, int precision, int k, int n, float tol_rgb, float tol_depth,
                  const nwe_adaptive_levels_outputs *out) {
    return nwe_render_adaptive_levels(ctx, pose, 1, H, W, 2.f, 2.f, 2.f, 1.5f, 0.1f, far, 0, H > 0 ? H : 0, precision, k, n, tol_rgb, tol_depth, out,
                                      NULL);
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
    nwe_adaptive_levels_outputs good = {0}, none = {0}, stale = {0};
    uint8_t kind[4 * 5], level[4 * 5];
    uint32_t flags = 0;
    memset(kind, 0x5a, sizeof(kind));
    memset(level, 0x5a, sizeof(level));
    good.struct_bytes = none.struct_bytes = sizeof(nwe_adaptive_levels_outputs);
    stale.struct_bytes = sizeof(nwe_adaptive_outputs); /* the one-level call's struct is another */
    CHECK(sizeof(nwe_adaptive_levels_outputs) == sizeof(nwe_adaptive_outputs) + sizeof(uint8_t *));
    good.rgb = stale.rgb = rgb;
    good.kind = none.kind = kind;
    good.level = none.level = level;
    good.flags = none.flags = &flags;
    const float nan = nanf("");
    /* each call is wrong in everything behind the refusal it expects as well */
    CHECK(levels(NULL, 0, 5, 0.f, 9, 0, 0, nan, nan, NULL) == NWE_ERR_INVALID);
    REFUSED(levels(ctx, 0, 5, 0.f, 9, 0, 0, nan, nan, NULL), NWE_ERR_INVALID, "null outputs");
    CHECK(levels(ctx, 0, 5, 0.f, 9, 0, 0, nan, nan, &stale) == NWE_ERR_INVALID &&
          strstr(nwe_last_error(ctx), "nwe_adaptive_levels_outputs.struct_bytes") != NULL);
    REFUSED(levels(ctx, 0, 5, 0.f, 9, 0, 0, nan, nan, &none), NWE_ERR_INVALID, "none of rgb / depth / acc requested");
    REFUSED(levels(ctx, 0, 5, 0.f, 9, 0, 0, nan, nan, &good), NWE_ERR_INVALID, "bad pose / image / row range");
    REFUSED(levels(ctx, 4, 5, 0.f, 9, 0, 0, nan, nan, &good), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths");
    REFUSED(levels(ctx, 4097, 4096, 5.f, 9, 0, 0, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: more than 2^24 rays in one call");
    REFUSED(levels(ctx, 4096, 4096, 5.f, 9, 0, 0, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: k must be in 1..64");
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 65, 0, nan, nan, &good), NWE_ERR_INVALID, "adaptive frame: k must be in 1..64");
    /* the levels, directly behind k */
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 2, 0, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 2, 5, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 2, -2147483647 - 1, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 2, 2147483647, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 33, 2, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 9, 4, nan, nan, &good), NWE_ERR_INVALID, LEVELS_TEXT);
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 8, 4, nan, 0.f, &good), NWE_ERR_INVALID, "adaptive frame: the tolerances must not be NaN");
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 64, 1, 0.f, nan, &good), NWE_ERR_INVALID, "adaptive frame: the tolerances must not be NaN");
    REFUSED(levels(ctx, 4, 5, 5.f, 9, 1, 4, -INFINITY, INFINITY, &good), NWE_ERR_INVALID, "unknown precision");
    REFUSED(levels(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "nwe_set_sampling has not been called");
    {
        float t[4] = {0.f, 1.f / 3, 2.f / 3, 1.f}, omt[4] = {1.f, 2.f / 3, 1.f / 3, 0.f}, u[2] = {0.f, 1.f};
        CHECK(nwe_set_sampling(ctx, t, omt, 4, u, 2) == NWE_OK);
    }
    REFUSED(levels(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "coarse network not set");
    CHECK(set_network(ctx, NWE_NET_COARSE) == NWE_OK);
    REFUSED(levels(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 2, 0.01f, 0.05f, &good), NWE_ERR_STATE, "fine network not set but n_importance > 0");
    CHECK(set_network(ctx, NWE_NET_FINE) == NWE_OK);
    /* a 2x8 network has no MFMA kernel: refused for the MFMA precisions in front of the host-only refusal */
    CHECK(levels(ctx, 4, 5, 5.f, NWE_PREC_F16X3, 2, 2, 0.01f, 0.05f, &good) == NWE_ERR_UNSUPPORTED &&
          strstr(nwe_last_error(ctx), "no MFMA kernel for this network shape") == nwe_last_error(ctx));
    /* a mode the call cannot serve, in nwe_render_rays' words */
    CHECK(nwe_set_early_termination(ctx, 0.01f) == NWE_OK);
    CHECK(levels(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 2, 0.01f, 0.05f, &good) == NWE_ERR_UNSUPPORTED &&
          strstr(nwe_last_error(ctx), "early termination is on") == nwe_last_error(ctx));
    CHECK(nwe_set_early_termination(ctx, 0.f) == NWE_OK);
    /* the last refusal a host-only context can give, zero rays included */
    REFUSED(levels(ctx, 4, 5, 5.f, NWE_PREC_F32, 2, 3, 0.01f, 0.05f, &good), NWE_ERR_STATE, "host-only context cannot render");
    REFUSED(nwe_render_adaptive_levels(ctx, pose, 1, 4, 5, 2.f, 2.f, 2.f, 1.5f, 0.1f, 5.f, 2, 2, NWE_PREC_F32, 8, 4, -1.f, INFINITY, &good, NULL),
            NWE_ERR_STATE, "host-only context cannot render");
    /* a refused call writes nothing and there is no report of a call that never ran */
    for (size_t i = 0; i < sizeof(rgb); ++i) CHECK(((unsigned char *)rgb)[i] == 0x5a);
    for (size_t i = 0; i < sizeof(kind); ++i) CHECK(kind[i] == 0x5a && level[i] == 0x5a);
    CHECK(flags == 0);
    int64_t counts[12];
    for (int i = 0; i < 12; ++i) counts[i] = -7;
    float ms = -7.f;
    CHECK(nwe_last_adaptive_levels(ctx, counts, 12, &ms) == NWE_ERR_STATE && counts[0] == -7 && counts[11] == -7 && ms == -7.f);
    CHECK(nwe_last_adaptive_levels(ctx, NULL, 12, &ms) == NWE_ERR_INVALID && nwe_last_adaptive_levels(NULL, counts, 12, NULL) == NWE_ERR_INVALID);
    CHECK(nwe_last_adaptive(ctx, counts, &ms) == NWE_ERR_STATE && nwe_last_kernel_ms(ctx) < 0.f && nwe_debug_last_plan(ctx) == -1);
    /* the lattice call: needs no context.  37 rows at k = 2 on three levels: spacings 8, 4, 2 */
    int32_t lat[64], one[64];
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 0, lat, 64) == 6 && lat[0] == 0 && lat[4] == 32 && lat[5] == 36);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 1, lat, 64) == 10 && lat[8] == 32 && lat[9] == 36);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 2, lat, 64) == 19 && nwe_debug_adaptive_lattice(0, 37, 2, one, 64) == 19);
    CHECK(memcmp(lat, one, 19 * sizeof(int32_t)) == 0);
    CHECK(nwe_debug_adaptive_levels_lattice(5, 30, 3, 2, 0, lat, 64) == 5 && lat[0] == 5 && lat[1] == 11 && lat[4] == 29);
    CHECK(nwe_debug_adaptive_levels_lattice(7, 8, 8, 4, 0, lat, 1) == 1 && lat[0] == 7);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 3, lat, 64) == -1 && nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, -1, lat, 64) == -1);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 33, 2, 0, lat, 64) == -1 && nwe_debug_adaptive_levels_lattice(0, 37, 2, 0, 0, lat, 64) == -1);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 5, 0, lat, 64) == -1 && nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 1, lat, 9) == -1);
    CHECK(nwe_debug_adaptive_levels_lattice(0, 37, 2, 3, 0, NULL, 64) == -1 && nwe_debug_adaptive_levels_lattice(3, 3, 2, 2, 0, lat, 64) == -1);
    /* the plan call: 37 x 45 at k = 2 on three levels - lattices of 6 x 7, 10 x 12 and 19 x 23 pixels */
    int64_t plan[16];
    CHECK(nwe_debug_adaptive_levels_plan(1, 37, 45, 2, 3, 11, plan, 16) == 11);
    CHECK(plan[0] == 1665 && plan[1] == 42 && plan[2] == 1228 && plan[3] > 1665 * 28 && plan[3] % 256 == 0);
    CHECK(plan[4] == 5 * 6 && plan[5] == 9 * 11 && plan[6] == 18 * 22);
    CHECK(plan[7] == 42 && plan[8] == 120 - 42 && plan[9] == 437 - 120 && plan[10] == 1228);
    CHECK(nwe_debug_adaptive_levels_plan(1, 37, 45, 2, 3, 11, plan, 10) == -1 && nwe_debug_adaptive_levels_plan(1, 37, 45, 2, 3, 9, plan, 16) == -1);
    CHECK(nwe_debug_adaptive_levels_plan(0, 37, 45, 2, 3, 11, plan, 16) == -1 && nwe_debug_adaptive_levels_plan(1, 4097, 4096, 2, 3, 8, plan, 16) == -1);
    CHECK(nwe_debug_adaptive_levels_plan(1, 37, 45, 33, 2, 11, plan, 16) == -1 && nwe_debug_adaptive_levels_plan(1, 37, 45, 2, 3, 11, NULL, 16) == -1);
    CHECK(nwe_debug_adaptive_levels_plan(1, 4096, 4096, 8, 4, 11, plan, 16) == 13 && plan[0] == 16777216);
    nwe_destroy(ctx);
    printf("adaptive_levels_smoke ok\n");
    return 0;
}
