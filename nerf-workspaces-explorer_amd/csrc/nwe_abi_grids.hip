// C ABI of libnwe_hip.so (include/nwe.h), the grids of a context: the occupancy grid, the coarse density grid and the radiance grid -
// set, clear, read, build or bake over the probe lattice of a box - nwe_coarse_grid_weights and the grid frame (nwe_render_grid).
// Host code only: the kernels are in nwe_occupancy.hip, nwe_coarse_grid.hip and nwe_radiance_grid.hip.
#include <algorithm>

#include "nwe_ctx.h"

namespace nwe {

// The context's coarse density grid as the producer kernel takes it, its radiance grid as the grid frame's and the sparse frames' do.
CoarseGrid coarse_grid_args(const nwe_ctx* ctx) {
    CoarseGrid g = ctx->cgrid.box.args<CoarseGrid>();
    g.sigma = ctx->d_cgrid.get();
    return g;
}
RadianceGrid radiance_grid_args(const nwe_ctx* ctx) {
    RadianceGrid g = ctx->rgrid.box.args<RadianceGrid>();
    g.rows = reinterpret_cast<const float4*>(ctx->d_rgrid.get());
    return g;
}

}  // namespace nwe

namespace {

// ---- occupancy grid (nwe_set_occupancy, nwe_build_occupancy) ----

int64_t occ_words(int64_t cells) { return (cells + 31) / 32; }

// Makes `words` (host, occ_words(cells) of them) the context's grid.  The bits behind the last cell are cleared; on a device
// context the words and the descriptor go to the context's own buffers, which no launch reads any more (the caller has waited).
int install_occupancy(nwe_ctx* c, const GridBox& box, std::vector<uint32_t>&& words) {
    Occupancy g;
    g.box = box;
    if (box.cells & 31) words.back() &= (1u << (box.cells & 31)) - 1u;
    for (const uint32_t w : words) g.occupied += __builtin_popcount(w);
    g.bits = std::move(words);
    if (!c->host_only) {
        c->occ.set = false;   // a failing upload leaves no grid rather than the old one's descriptor over new words
        HIPCHK(c, c->d_occ_bits.reserve(g.bits.size()));
        HIPCHK(c, c->d_occ.reserve(1));
        HIPCHK(c, hipMemcpy(c->d_occ_bits.get(), g.bits.data(), g.bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        OccGrid d = box.args<OccGrid>();
        d.bits = c->d_occ_bits.get();
        HIPCHK(c, hipMemcpy(c->d_occ.get(), &d, sizeof(d), hipMemcpyHostToDevice));
    }
    g.set = true;
    c->occ = std::move(g);
    return NWE_OK;
}

// ---- coarse density grid (nwe_set_coarse_grid, nwe_bake_coarse_grid) ----

// The box, the resolution and inv of a new grid of values - the coarse density grid or the radiance grid; the values are in place
// (the grid's device buffer or g.host) when this is called.
void install_grid(CoarseGridState& slot, const GridBox& box, std::vector<float>&& host) { slot = CoarseGridState{true, box, std::move(host)}; }

// nwe_set_* of a grid of values, `per_cell` floats a cell, behind its checks: the one path of both such grids.
int set_values_grid(nwe_ctx* c, CoarseGridState& slot, DevBuf<float>& dev, const GridBox& box, int per_cell, const float* values, bool on_device) {
    const size_t count = (size_t)box.cells * per_cell;
    if (c->host_only) {
        install_grid(slot, box, std::vector<float>(values, values + count));
        return NWE_OK;
    }
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // a queued launch still reads the old grid
    slot = CoarseGridState{};    // a failing allocation or upload leaves no grid rather than the old box over new values
    HIPCHK(c, dev.reserve(count));
    HIPCHK(c, hipMemcpy(dev.get(), values, count * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    install_grid(slot, box, {});
    return NWE_OK;
}
// nwe_clear_* of any of the three grids: a queued launch may still read the one that goes
template <class Grid>
int clear_grid(nwe_ctx* c, Grid& grid) {
    if (!c->host_only && grid.set) {
        ON_DEVICE(c);
        TRY(wait_for_launches(c));
    }
    grid = Grid{};
    return NWE_OK;
}
// nwe_get_* and nwe_*_copy of such a grid, `per_cell` floats a cell again; no grid is set: the outputs stay untouched (and so does the
// error text of a const context)
int get_values_grid(const CoarseGridState& slot, float* lo, float* hi, int* res, float* inv) {
    if (!slot.set) return NWE_ERR_STATE;
    slot.box.read(lo, hi, res, inv);
    return NWE_OK;
}
int copy_values_grid(nwe_ctx* c, const CoarseGridState& slot, const DevBuf<float>& dev, int per_cell, const char* needs, float* host_values, int64_t n_values) {
    if (!slot.set) return NWE_ERR_STATE;
    if (!host_values || n_values != per_cell * slot.box.cells) return fail(c, NWE_ERR_INVALID, needs);
    if (c->host_only) return copy_out(&slot.host, host_values, n_values);
    ON_DEVICE(c);
    HIPCHK(c, hipMemcpy(host_values, dev.get(), (size_t)n_values * sizeof(float), hipMemcpyDeviceToHost));
    return NWE_OK;
}

// ---- the probe lattice of a box: what nwe_build_occupancy asks the networks at, and - probes = 1, the cells' centres - what
// nwe_bake_coarse_grid does ----

struct Lattice {
    OccBuild b;
    int per_cell;       // probes^3
    int chunk_cells;    // the cells whose probes go through the scratch buffer at a time: 2^20 points at the most
};

Lattice probe_lattice(const GridBox& box, int probes) {
    Lattice l = {};
    for (int i = 0; i < 3; ++i) {
        l.b.lo[i] = box.lo[i]; l.b.res[i] = box.res[i];
        l.b.step[i] = (float)(((double)box.hi[i] - (double)box.lo[i]) / (double)box.res[i]);
    }
    l.b.probes = probes;
    l.per_cell = probes * probes * probes;
    l.chunk_cells = (int)std::min<int64_t>(box.cells, std::max(1, (1 << 20) / l.per_cell));
    return l;
}

// Chunk by chunk on `stream`: the probe points of the chunk's cells into `points`, a query of network n at them, then
// done(first cell, cells), which queues what the caller makes of the answers.  fill(q, first cell, cells) says where the answers go:
// it finds the sigma-only query of nwe_query_points - no directions, the density trunk alone where it is built - and sets q.sigma,
// or makes it the raw query of one direction (nwe_bake_radiance_grid).
template <class Fill, class Done>
int query_lattice(nwe_ctx* c, const NetState& n, const Lattice& l, int64_t cells, float* points, int precision, hipStream_t stream,
                  Fill&& fill, Done&& done) {
    for (int64_t first = 0; first < cells; first += l.chunk_cells) {
        const int count = (int)std::min<int64_t>(l.chunk_cells, cells - first);
        launch_occ_probe_points(l.b, first, count, points, stream);
        QueryArgs q = {};
        q.points = points; q.n_points = count * l.per_cell; q.points_per_dir = 1; q.density_only = 1;
        fill(q, first, count);
        TRY(run_query(c, n, q, precision, stream));
        done(first, count);
    }
    return NWE_OK;
}

// nwe_bake_* of a grid of values behind its checks, the one path of both such grids: the cells' centres, a chunk of them in the
// scratch buffer (12 MB at the most; the radiance grid's direction behind them), and network n's answers straight into the grid -
// sigma, or (raw) the rows of the raw query with one direction for all of a chunk's points.
int bake_values_grid(nwe_ctx* c, CoarseGridState& slot, DevBuf<float>& dev, const NetState& n, const GridBox& box, bool raw, const float* dir3_host,
                     int precision, hipStream_t stream) {
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // the bake ends in a new grid: a queued launch still reads the old one
    slot = CoarseGridState{};    // a failing bake leaves no grid
    const Lattice l = probe_lattice(box, 1);
    HIPCHK(c, c->d_occ_scratch.reserve((size_t)l.chunk_cells * 3 + (raw ? 3 : 0)));
    HIPCHK(c, dev.reserve((size_t)box.cells * (raw ? 4 : 1)));
    float* points = c->d_occ_scratch.get();
    float* dir = dir3_host ? points + (size_t)l.chunk_cells * 3 : nullptr;
    if (dir) HIPCHK(c, hipMemcpyAsync(dir, dir3_host, 3 * sizeof(float), hipMemcpyHostToDevice, stream));
    float* grid = dev.get();
    TRY(query_lattice(c, n, l, box.cells, points, precision, stream, [&](QueryArgs& q, int64_t first, int count) {
        if (!raw) { q.sigma = grid + first; return; }
        q.dirs = dir; q.raw = grid + first * 4; q.points_per_dir = count; q.density_only = 0;
    }, [](int64_t, int) {}));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(stream));
    install_grid(slot, box, {});
    return NWE_OK;
}

}  // namespace

extern "C" {

int nwe_set_occupancy(nwe_ctx* c, const float* lo, const float* hi, const int* res, const uint32_t* bits, int bits_on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kOccupancyGrid, lo, hi, res, bits, bits_on_device != 0, c->host_only));
    const GridBox box(lo, hi, res);
    std::vector<uint32_t> words((size_t)occ_words(box.cells));
    if (c->host_only) {
        std::memcpy(words.data(), bits, words.size() * sizeof(uint32_t));
        return install_occupancy(c, box, std::move(words));
    }
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // a queued launch still reads the old grid
    if (bits_on_device) HIPCHK(c, hipMemcpy(words.data(), bits, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    else std::memcpy(words.data(), bits, words.size() * sizeof(uint32_t));
    return install_occupancy(c, box, std::move(words));
}

int nwe_clear_occupancy(nwe_ctx* c) { return c ? clear_grid(c, c->occ) : NWE_ERR_INVALID; }

int nwe_get_occupancy(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv, int64_t* occupied_cells) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->occ.set) return NWE_ERR_STATE;   // no grid is set: the outputs stay untouched (and so does the error text of a const context)
    c->occ.box.read(lo, hi, res, inv);
    if (occupied_cells) *occupied_cells = c->occ.occupied;
    return NWE_OK;
}

int nwe_occupancy_copy(const nwe_ctx* c, uint32_t* host_words, int64_t n_words) {
    if (!c) return NWE_ERR_INVALID;
    if (!c->occ.set) return NWE_ERR_STATE;
    return copy_out(&c->occ.bits, host_words, n_words);
}

int nwe_build_occupancy(nwe_ctx* c, const float* lo, const float* hi, const int* res, int probes, float threshold, int dilate,
                        int precision, void* stream_) {
    CHECK(c, check_build_occupancy(MaybeContext(c).p, lo, hi, res, probes, threshold, dilate, precision));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    TRY(wait_for_launches(c));   // the build ends in a new grid: a queued launch still reads the old one
    const GridBox box(lo, hi, res);
    const Lattice l = probe_lattice(box, probes);
    const int64_t words = occ_words(box.cells);
    // the probes of a chunk of cells and their sigma in a scratch buffer the context keeps: 2^20 points (16 MB) at the most
    HIPCHK(c, c->d_occ_scratch.reserve((size_t)l.chunk_cells * l.per_cell * 4));
    HIPCHK(c, c->d_occ_tmp.reserve((size_t)words * 2));
    float* points = c->d_occ_scratch.get();
    float* sigma = points + (size_t)l.chunk_cells * l.per_cell * 3;
    uint32_t* buf[2] = {c->d_occ_tmp.get(), c->d_occ_tmp.get() + words};
    HIPCHK(c, hipMemsetAsync(buf[0], 0, (size_t)words * sizeof(uint32_t), stream));
    for (const NetState& n : c->net)   // a cell is occupied where either network says so
        if (n.set)
            TRY(query_lattice(c, n, l, box.cells, points, precision, stream, [&](QueryArgs& q, int64_t, int) { q.sigma = sigma; }, [&](int64_t first, int count) {
                launch_occ_reduce_bits(sigma, first, count, l.per_cell, threshold, buf[0], stream);
            }));
    int cur = 0;
    for (int d = 0; d < dilate; ++d, cur ^= 1)
        launch_occ_dilate(buf[cur], buf[cur ^ 1], res, stream);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> host((size_t)words);
    HIPCHK(c, hipMemcpyAsync(host.data(), buf[cur], (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    return install_occupancy(c, box, std::move(host));
}

int nwe_set_coarse_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, const float* sigma, int on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kCoarseGrid, lo, hi, res, sigma, on_device != 0, c->host_only));
    return set_values_grid(c, c->cgrid, c->d_cgrid, GridBox(lo, hi, res), 1, sigma, on_device != 0);
}

int nwe_clear_coarse_grid(nwe_ctx* c) { return c ? clear_grid(c, c->cgrid) : NWE_ERR_INVALID; }

int nwe_get_coarse_grid(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv) { return c ? get_values_grid(c->cgrid, lo, hi, res, inv) : NWE_ERR_INVALID; }

int nwe_coarse_grid_copy(nwe_ctx* c, float* host_values, int64_t n_values) {
    return c ? copy_values_grid(c, c->cgrid, c->d_cgrid, 1, "coarse grid: the copy needs rx * ry * rz values", host_values, n_values) : NWE_ERR_INVALID;
}

int nwe_bake_coarse_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, int precision, void* stream_) {
    CHECK(c, check_bake_coarse_grid(MaybeContext(c).p, lo, hi, res, precision));
    return bake_values_grid(c, c->cgrid, c->d_cgrid, c->net[NWE_NET_COARSE], GridBox(lo, hi, res), false, nullptr, precision, (hipStream_t)stream_);
}

int nwe_coarse_grid_weights(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near,
                            float far, int row_begin, int row_end, float* sigma_out_dev, float* weights_out_dev, void* stream_) {
    CHECK(c, check_on_device(c && !c->host_only));
    if (!c->cgrid.set) return fail(c, NWE_ERR_STATE, "coarse grid: no grid is set (nwe_set_coarse_grid, nwe_bake_coarse_grid)");
    if (c->ns <= 0) return fail(c, NWE_ERR_STATE, "nwe_set_sampling has not been called");
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_camera(m));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->rays_slot;   // not a slot of the ring, like nwe_create_rays: the timing calls keep describing the last render
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = camera_args(m, slot.poses.get());
    CHECK(c, check_ray_count(a.n_rays, false));
    context_args(c, a);
    if (a.n_rays == 0 || (!sigma_out_dev && !weights_out_dev)) return NWE_OK;
    return record_launch(c, slot, stream, [&]() -> int {
        launch_coarse_grid_weights(a, coarse_grid_args(c), nullptr, sigma_out_dev, weights_out_dev, stream);
        return NWE_OK;
    });
}

int nwe_set_radiance_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, const float* raw, int on_device) {
    if (!c) return NWE_ERR_INVALID;
    CHECK(c, check_set_grid(kRadianceGrid, lo, hi, res, raw, on_device != 0, c->host_only));
    return set_values_grid(c, c->rgrid, c->d_rgrid, GridBox(lo, hi, res), 4, raw, on_device != 0);
}

int nwe_clear_radiance_grid(nwe_ctx* c) { return c ? clear_grid(c, c->rgrid) : NWE_ERR_INVALID; }

int nwe_get_radiance_grid(const nwe_ctx* c, float* lo, float* hi, int* res, float* inv) { return c ? get_values_grid(c->rgrid, lo, hi, res, inv) : NWE_ERR_INVALID; }

int nwe_radiance_grid_copy(nwe_ctx* c, float* host_values, int64_t n_values) {
    return c ? copy_values_grid(c, c->rgrid, c->d_rgrid, 4, "radiance grid: the copy needs 4 * rx * ry * rz values", host_values, n_values) : NWE_ERR_INVALID;
}

int nwe_bake_radiance_grid(nwe_ctx* c, const float* lo, const float* hi, const int* res, int which, const float* dir3_host, int precision,
                           void* stream_) {
    CHECK(c, check_bake_radiance_grid(MaybeContext(c).p, lo, hi, res, which, dir3_host, precision));
    return bake_values_grid(c, c->rgrid, c->d_rgrid, c->net[which], GridBox(lo, hi, res), true, dir3_host, precision, (hipStream_t)stream_);
}

int nwe_render_grid(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                    int row_begin, int row_end, const nwe_grid_outputs* out, void* stream_) {
    const Camera m{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end};
    CHECK(c, check_render_grid(MaybeContext(c).p, out, m));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(c);
    Slot& slot = c->grid.next();   // not a slot of the render ring (see nwe_create_rays)
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, c2w, n_poses, stream));
    RenderArgs a = frame_args(c, m, slot.poses.get(), out->rgb, out->depth, out->acc, out->flags);
    if (a.n_rays == 0) return NWE_OK;
    a.out.weights_coarse = out->weights_coarse; a.out.z_fine = out->z_fine; a.out.raw_fine = out->raw_fine;
    TRY(record_launch(c, slot, stream, [&]() -> int {
        launch_radiance_grid_render(a, radiance_grid_args(c), stream);
        return NWE_OK;
    }));
    c->grid.commit(slot);
    return NWE_OK;
}

float nwe_last_grid_ms(nwe_ctx* c) { return elapsed_ms(c, c ? c->grid.last() : nullptr, "nwe_last_grid_ms"); }

}  // extern "C"
