// csrc/nwe_check.cpp asked directly, without the library: the refusals that the ABI reaches only with a device context, so that
// no host-only context can be made to say them.  Built with the host compiler and run by tests/test_refusals_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "nwe_check.h"

using namespace nwe;

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static bool is(const Refusal& r, int code, const char* text) {
    if (r.code == code && r.text == text) return true;
    fprintf(stderr, "got %d \"%s\"\n", r.code, r.text.c_str());
    return false;
}

static const char* kNoMfma =
    "no MFMA kernel for this network shape (have widths 128 and 256 with depth 6 or 8 and the skip after layer 4, or depth 4 without, 63 + 27 or, "
    "without view directions, 63 inputs); use NWE_PREC_F32";

int main() {
    const float pose[16] = {};
    // the camera: image, intrinsics, depth range, in this order, and the two texts that are the entry point's own
    const Camera ok{pose, 1, 4, 8, 1.f, 1.f, 0.f, 0.f, 0.1f, 10.f, 0, 4};
    CHECK(is(check_camera(ok), NWE_OK, ""));
    Camera m = ok;
    m.W = 0; m.fx = 0.f; m.far = 0.f;
    CHECK(is(check_camera(m), NWE_ERR_INVALID, "bad pose / image / row range"));
    CHECK(is(check_camera(m, kCameraOfTiled), NWE_ERR_INVALID, "bad pose / image"));
    CHECK(is(check_camera(m, kCameraOfCreateRays), NWE_ERR_INVALID, "bad pose / image / row range"));
    m.W = 8;
    for (CameraOf entry : {kCameraOfRender, kCameraOfTiled, kCameraOfCreateRays}) CHECK(is(check_camera(m, entry), NWE_ERR_INVALID, "fx and fy must be non-zero"));
    m.fx = -0.f;
    CHECK(is(check_camera(m), NWE_ERR_INVALID, "fx and fy must be non-zero"));
    m.fx = 1.f; m.fy = 0.f;
    CHECK(is(check_camera(m), NWE_ERR_INVALID, "fx and fy must be non-zero"));
    m.fy = 1.f;
    CHECK(is(check_camera(m), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths"));
    CHECK(is(check_camera(m, kCameraOfTiled), NWE_ERR_INVALID, "far < near: the sorted merge of the fine pass needs ascending depths"));
    CHECK(is(check_camera(m, kCameraOfCreateRays), NWE_ERR_INVALID, "far < near: nwe_render_rays needs near <= far on every ray"));
    m.far = m.near;
    CHECK(is(check_camera(m), NWE_OK, ""));
    CHECK(is(check_on_device(false), NWE_ERR_STATE, "needs a device context") && is(check_on_device(true), NWE_OK, ""));

    // a device context with a 4x128 coarse network that has MFMA kernels and a fine network without view directions that has none
    ContextDesc d;
    d.net[0].set = true; d.net[0].D = 4; d.net[0].W = 128; d.net[0].in_xyz = 63; d.net[0].in_dir = 27; d.net[0].mfma_ok = true;
    ContextDesc host = d;
    host.host_only = true;
    const float points[3] = {};
    nwe_point_outputs out;
    memset(&out, 0, sizeof out);
    out.struct_bytes = sizeof out;
    float sink = 0.f;
    out.sigma = &sink;

    // nwe_query_points, in the order of include/nwe.h
    const auto query = [&](const ContextDesc* c, int which, const float* p, int64_t n, const float* dirs, int64_t per_dir, int precision,
                           const nwe_point_outputs* o) { return check_query(c, which, p, n, dirs, per_dir, precision, o); };
    CHECK(is(query(nullptr, 0, points, 1, nullptr, 1, 0, &out), NWE_ERR_STATE, "needs a device context"));
    CHECK(is(query(&host, 0, points, 1, nullptr, 1, 0, &out), NWE_ERR_STATE, "needs a device context"));
    CHECK(is(query(&d, 0, points, 1, nullptr, 1, 0, nullptr), NWE_ERR_INVALID, "null outputs"));
    nwe_point_outputs older = out;
    older.struct_bytes -= 8;
    CHECK(is(query(&d, 7, points, 1, nullptr, 1, 0, &older), NWE_ERR_INVALID,
             "nwe_point_outputs.struct_bytes != sizeof(nwe_point_outputs): the caller was built against another version of include/nwe.h"));
    CHECK(is(query(&d, 2, points, -1, nullptr, 1, 0, &out), NWE_ERR_INVALID, "which must be 0 or 1"));
    CHECK(is(query(&d, 0, points, -1, nullptr, 0, 0, &out), NWE_ERR_INVALID, "bad n_points (negative, or more than 2^31 - 1)"));
    CHECK(is(query(&d, 0, points, (int64_t)1 << 31, nullptr, 0, 0, &out), NWE_ERR_INVALID, "bad n_points (negative, or more than 2^31 - 1)"));
    CHECK(is(query(&d, 0, nullptr, 1, nullptr, 0, 0, &out), NWE_ERR_INVALID, "points_per_dir must be at least 1"));
    CHECK(is(query(&d, 0, nullptr, 1, nullptr, 1, 7, &out), NWE_ERR_INVALID, "null points"));
    CHECK(is(query(&d, 0, nullptr, 0, nullptr, 1, 0, &out), NWE_OK, ""));
    nwe_point_outputs nothing = out;
    nothing.sigma = nullptr;
    CHECK(is(query(&d, 0, points, 1, nullptr, 1, 7, &nothing), NWE_ERR_INVALID, "neither raw nor sigma requested"));
    CHECK(is(query(&d, 1, points, 1, nullptr, 1, 7, &out), NWE_ERR_INVALID, "unknown precision"));
    CHECK(is(query(&d, 1, points, 1, nullptr, 1, 0, &out), NWE_ERR_STATE, "fine network not set"));
    ContextDesc none = d;
    none.net[0].set = false;
    CHECK(is(query(&none, 0, points, 1, nullptr, 1, 0, &out), NWE_ERR_STATE, "coarse network not set"));
    d.net[1].set = true; d.net[1].D = 4; d.net[1].W = 64; d.net[1].in_xyz = 63; d.net[1].in_dir = 0; d.net[1].out_ch = 5;
    CHECK(is(query(&d, 1, points, 1, points, 1, 0, &out), NWE_ERR_INVALID,
             "the network takes no view directions (nwe_set_network_no_view_dirs): dirs_dev must be null"));
    nwe_point_outputs raw = out;
    raw.raw = &sink;
    CHECK(is(query(&d, 0, points, 1, nullptr, 1, 0, &raw), NWE_ERR_INVALID,
             "raw output of a network with view directions needs dirs_dev (only sigma does not depend on the direction)"));
    CHECK(is(query(&d, 0, points, 1, nullptr, 1, 0, &out), NWE_OK, "") && is(query(&d, 0, points, 1, points, 1, 1, &raw), NWE_OK, ""));
    CHECK(is(query(&d, 1, points, 1, nullptr, 1, 1, &raw), NWE_ERR_UNSUPPORTED, kNoMfma) && is(query(&d, 1, points, 1, nullptr, 1, 2, &raw), NWE_OK, ""));

    // nwe_build_occupancy and nwe_bake_coarse_grid in front of their device: the box, their own arguments, the networks
    const float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
    const float zero[3] = {0.f, 0.f, 0.f}, denormal[3] = {1.f, 1e-45f, 1.f};   // a box whose fp32 resolution / (hi - lo) is infinite
    const int res[3] = {2, 3, 4}, big[3] = {2, 3, 513}, bigger[3] = {1025, 3, 4}, fine[3] = {2, 3, 512};
    CHECK(is(check_build_occupancy(&host, lo, hi, res, 2, 0.f, 1, 0), NWE_ERR_STATE, "needs a device context"));
    CHECK(is(check_build_occupancy(&d, lo, nullptr, res, 9, 0.f, 1, 0), NWE_ERR_INVALID, "occupancy: null lo, hi or resolution"));
    CHECK(is(check_build_occupancy(&d, hi, lo, res, 9, 0.f, 1, 0), NWE_ERR_INVALID, "occupancy: the box must have lo < hi on every axis"));
    CHECK(is(check_build_occupancy(&d, lo, hi, bigger, 9, 0.f, 1, 0), NWE_ERR_INVALID, "occupancy: the resolution must be in 1..1024 on every axis"));
    CHECK(is(check_build_occupancy(&d, lo, hi, big, 0, 0.f, 3, 0), NWE_ERR_INVALID, "occupancy: probes must be in 1..4"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 5, 0.f, 3, 0), NWE_ERR_INVALID, "occupancy: probes must be in 1..4"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 4, NAN, 3, 0), NWE_ERR_INVALID, "occupancy: dilate must be in 0..2"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 4, NAN, -1, 0), NWE_ERR_INVALID, "occupancy: dilate must be in 0..2"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 4, NAN, 2, 7), NWE_ERR_INVALID, "occupancy: the threshold must not be NaN"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 1, INFINITY, 0, 7), NWE_ERR_INVALID, "unknown precision"));
    ContextDesc unset;
    CHECK(is(check_build_occupancy(&unset, lo, hi, res, 1, 0.f, 0, 0), NWE_ERR_STATE, "occupancy: no network is set"));
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 1, 0.f, 0, 1), NWE_ERR_UNSUPPORTED, kNoMfma));   // either network without a kernel
    CHECK(is(check_build_occupancy(&d, lo, hi, res, 1, 0.f, 0, 2), NWE_OK, ""));
    CHECK(is(check_build_occupancy(&d, zero, denormal, res, 1, 0.f, 0, 2), NWE_OK, ""));   // only the coarse grid asks for a finite inv
    CHECK(is(check_bake_coarse_grid(nullptr, lo, hi, res, 0), NWE_ERR_STATE, "needs a device context"));
    CHECK(is(check_bake_coarse_grid(&d, lo, hi, big, 7), NWE_ERR_INVALID, "coarse grid: the resolution must be in 1..512 on every axis"));
    CHECK(is(check_bake_coarse_grid(&d, zero, denormal, res, 7), NWE_ERR_INVALID, "coarse grid: the box must be finite (resolution / (hi - lo) is not, in fp32)"));
    CHECK(is(check_bake_coarse_grid(&d, lo, hi, fine, 7), NWE_ERR_INVALID, "unknown precision"));
    CHECK(is(check_bake_coarse_grid(&none, lo, hi, res, 0), NWE_ERR_STATE, "coarse grid: the coarse network is not set"));
    CHECK(is(check_bake_coarse_grid(&d, lo, hi, res, 0), NWE_OK, ""));   // the fine network's shape does not matter to a bake
    d.net[0].mfma_ok = false;
    CHECK(is(check_bake_coarse_grid(&d, lo, hi, res, 1), NWE_ERR_UNSUPPORTED, kNoMfma) && is(check_bake_coarse_grid(&d, lo, hi, res, 2), NWE_OK, ""));
    printf("check_smoke ok\n");
    return 0;
}
