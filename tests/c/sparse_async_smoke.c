/* nwe_render_sparse_async from plain C on a host-only context: every refusal in front of the host-only one, by code, text and order -
 * the list of nwe_render_sparse (tests/c/sparse_smoke.c), which shares its check - the reports and the host-wait hook of a context
 * that has rendered no sparse frame, and the counted grid rule, which needs no context.  Built and run by `make asan` beside
 * sparse_smoke.c, host code only; no GPU needed. */
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

/* the call with a good camera but for H and far, which the cases vary */
static int sparse(nwe_ctx *ctx, int H, float far, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs *out) {
    return nwe_render_sparse_async(ctx, pose, 1, H, 5, 2.f, 2.f, 2.f, 1.5f, 0.1f, far, 0, H > 0 ? H : 0, which, precision, min_weight, dilate, out, NULL);
}

int main(void) {
    nwe_ctx *ctx = NULL;
    CHECK(nwe_create(&ctx, -1) == NWE_OK && ctx);
    float rgb[4 * 5 * 3];
    memset(rgb, 0x5a, sizeof(rgb));
    nwe_sparse_outputs good = {0}, none = {0}, stale = {0};
    uint32_t flags = 0;
    good.struct_bytes = none.struct_bytes = sizeof(nwe_sparse_outputs);
    stale.struct_bytes = sizeof(nwe_sparse_outputs) - 8;
    good.rgb = stale.rgb = rgb;
    none.flags = &flags;
    const float nan = nanf("");
    /* each call is wrong in everything behind the refusal it expects as well */
    CHECK(sparse(NULL, 0, 0.f, 2, 9, nan, 9, NULL) == NWE_ERR_INVALID);
    REFUSED(sparse(ctx, 0, 0.f, 2, 9, nan, 9, NULL), NWE_ERR_INVALID, "null outputs");
    CHECK(sparse(ctx, 0, 0.f, 2, 9, nan, 9, &stale) == NWE_ERR_INVALID && strstr(nwe_last_error(ctx), "nwe_sparse_outputs.struct_bytes") != NULL);
    REFUSED(sparse(ctx, 0, 0.f, 2, 9, nan, 9, &none), NWE_ERR_INVALID,
            "none of rgb / depth / acc / weights_coarse / z_fine / weights_grid / selected / raw_fine requested");
    REFUSED(sparse(ctx, 0, 0.f, 2, 9, nan, 9, &good), NWE_ERR_INVALID, "bad pose / image / row range");
    REFUSED(sparse(ctx, 4, 0.f, 2, 9, nan, 9, &good), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths");
    REFUSED(sparse(ctx, 4, 5.f, 2, 9, nan, 9, &good), NWE_ERR_INVALID, "which must be 0 or 1");
    REFUSED(sparse(ctx, 4, 5.f, 1, 9, nan, 9, &good), NWE_ERR_INVALID, "unknown precision");
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, nan, 9, &good), NWE_ERR_INVALID, "sparse frame: min_weight must not be NaN");
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, 9, &good), NWE_ERR_INVALID, "sparse frame: dilate must be in 0..8");
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, -1, &good), NWE_ERR_INVALID, "sparse frame: dilate must be in 0..8");
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, -INFINITY, 8, &good), NWE_ERR_STATE,
            "sparse frame: no radiance grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)");
    {
        const float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
        const int res[3] = {1, 2, 1};
        const float rows[8] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 2.f};
        CHECK(nwe_set_radiance_grid(ctx, lo, hi, res, rows, 0) == NWE_OK);
    }
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, 0, &good), NWE_ERR_STATE, "nwe_set_sampling has not been called");
    {
        float t[4] = {0.f, 1.f / 3, 2.f / 3, 1.f}, omt[4] = {1.f, 2.f / 3, 1.f / 3, 0.f};
        CHECK(nwe_set_sampling(ctx, t, omt, 4, NULL, 0) == NWE_OK);
    }
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, 0, &good), NWE_ERR_STATE, "sparse frame: the fine network is not set");
    REFUSED(sparse(ctx, 4, 5.f, 0, NWE_PREC_F32, 1e-3f, 0, &good), NWE_ERR_STATE, "sparse frame: the coarse network is not set");
    /* a network (which clears the grid: set it again behind it), and the last refusal a host-only context can give */
    {
        enum { D = 2, W = 8, IN_XYZ = 63, IN_DIR = 27 };
        const int ins[D + 4] = {IN_XYZ, W, W + IN_DIR, W, W, W / 2};
        const int outs[D + 4] = {W, W, W / 2, W, 1, 3};
        float *w[D + 4], *b[D + 4];
        for (int l = 0; l < D + 4; ++l) {
            w[l] = (float *)calloc((size_t)ins[l] * outs[l], sizeof(float));
            b[l] = (float *)calloc((size_t)outs[l], sizeof(float));
        }
        CHECK(nwe_set_network(ctx, NWE_NET_FINE, D, W, IN_XYZ, IN_DIR, -1, (const float *const *)w, (const float *const *)b) == NWE_OK);
        for (int l = 0; l < D + 4; ++l) {
            free(w[l]);
            free(b[l]);
        }
        const float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
        const int res[3] = {1, 1, 1};
        const float rows[4] = {0.f, 0.f, 0.f, 1.f};
        REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, 0, &good), NWE_ERR_STATE,
                "sparse frame: no radiance grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)");
        CHECK(nwe_set_radiance_grid(ctx, lo, hi, res, rows, 0) == NWE_OK);
    }
    /* a 2x8 network has no MFMA kernel, but the host-only refusal stands in front of that one */
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F16X3, 1e-3f, 0, &good), NWE_ERR_STATE, "needs a device context");
    REFUSED(sparse(ctx, 4, 5.f, 1, NWE_PREC_F32, -1.f, 8, &good), NWE_ERR_STATE, "needs a device context");
    /* a refused call writes nothing and moves no report */
    for (size_t i = 0; i < sizeof(rgb); ++i) CHECK(((unsigned char *)rgb)[i] == 0x5a);
    CHECK(flags == 0);
    int64_t counts[2] = {-7, -7};
    CHECK(nwe_last_sparse_samples(ctx, counts) == NWE_ERR_STATE && counts[0] == -7 && counts[1] == -7);
    CHECK(nwe_last_sparse_samples(ctx, NULL) == NWE_ERR_INVALID && nwe_last_sparse_samples(NULL, counts) == NWE_ERR_INVALID);
    CHECK(nwe_last_sparse_ms(ctx) < 0.f && nwe_last_sparse_ms(NULL) < 0.f);
    CHECK(nwe_last_kernel_ms(ctx) < 0.f && nwe_last_query_ms(ctx) < 0.f && nwe_last_grid_ms(ctx) < 0.f && nwe_debug_last_plan(ctx) == -1);
    CHECK(nwe_debug_last_sparse_host_waits(ctx) == -1 && nwe_debug_last_sparse_host_waits(NULL) == -1);
    /* the counted grid: min(ceil(capacity / packet), 8 cus), or ceil(ceil(capacity / packet) / steps) when forced */
    CHECK(nwe_debug_query_counted_grid(0, 128, 0, 256) == 0 && nwe_debug_query_counted_grid(1, 128, 0, 256) == 1);
    CHECK(nwe_debug_query_counted_grid(128, 128, 0, 256) == 1 && nwe_debug_query_counted_grid(129, 128, 0, 256) == 2);
    CHECK(nwe_debug_query_counted_grid((int64_t)1 << 21, 128, 0, 256) == 2048 && nwe_debug_query_counted_grid((int64_t)1 << 21, 16, 0, 4) == 32);
    CHECK(nwe_debug_query_counted_grid(10240, 128, 3, 256) == 27 && nwe_debug_query_counted_grid(1920, 16, 7, 256) == 18);
    nwe_destroy(ctx);
    printf("sparse_async_smoke ok\n");
    return 0;
}
