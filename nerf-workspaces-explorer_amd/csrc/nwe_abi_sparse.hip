// C ABI of libnwe_hip.so (include/nwe.h), the sparse frames: nwe_render_sparse and nwe_render_sparse_async, one body for both,
// their reports and their hooks.  Host code only: the kernels are in nwe_sparse.hip, nwe_sparse_async.hip and the query units.
#include <algorithm>

#include "nwe_ctx.h"

namespace {

// What the host waits for in front of a call, until its slot, the scratch and the poses are ready.
// The synchronous call: every sparse call in flight - an asynchronous one still uses the scratch - and an unconditional reserve
// (grow-only; nothing of an earlier call still reads it), with the pinned word the chunks' totals are read back through.
int ready_sync(nwe_ctx* c, const SparsePlan& p, SparseSlot& slot, const Camera& m, hipStream_t stream) {
    TRY(wait_for_sparse(c, nullptr));
    TRY(prepare_slot(c, slot));
    TRY(upload_poses(c, slot, m.c2w, m.n_poses, stream));
    HIPCHK(c, c->d_sparse_scratch.reserve((size_t)p.bytes));
    if (!c->sparse_word) HIPCHK(c, hipHostMalloc(&c->sparse_word.h, sizeof(uint32_t), hipHostMallocDefault));
    return NWE_OK;
}
// The asynchronous call: the host waits only here - for every sparse call in flight if the scratch has to grow (growing drops it),
// and for the call that used this slot of the ring four calls ago, normally long finished.  On the device the call goes behind the
// previous sparse call of either kind, whose chunks use the same scratch, on whatever stream it ran.
int ready_async(nwe_ctx* c, const SparsePlan& p, SparseSlot& slot, const Camera& m, hipStream_t stream, int* host_waits) {
    if ((size_t)p.bytes > c->d_sparse_scratch.cap) {
        TRY(wait_for_sparse(c, host_waits));
        HIPCHK(c, c->d_sparse_scratch.reserve((size_t)p.bytes));
    }
    if (slot.used && hipEventQuery(slot.ev1) != hipSuccess) { ++*host_waits; (void)hipGetLastError(); }
    TRY(prepare_slot(c, slot));
    HIPCHK(c, slot.tally.reserve(1));
    if (!slot.word) HIPCHK(c, hipHostMalloc(&slot.word.h, sizeof(unsigned long long), hipHostMallocDefault));
    if (const SparseSlot* last = c->sparse.last()) HIPCHK(c, hipStreamWaitEvent(stream, last->ev1, 0));
    return upload_poses(c, slot, m.c2w, m.n_poses, stream);
}

// Both kinds of sparse frame: the checks, the plan (plan_sparse, nwe_plan.h), the kernel arguments and the chunk loop are one; the
// kinds differ in what the host waits for beforehand (ready_*), in the step between emit and composite, and in the epilogue.
int render_sparse(nwe_ctx* c, bool async, const Camera& m, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs* out,
                  hipStream_t stream) {
    CHECK(c, check_render_sparse(MaybeContext(c).p, out, m, which, precision, min_weight, dilate));
    const int64_t n_rays = (int64_t)m.n_poses * (m.row_end - m.row_begin) * m.W;
    if (n_rays == 0) return NWE_OK;
    ON_DEVICE(c);
    const NetState& net = c->net[which];
    const int S = c->ns + c->ni;
    const SparsePlan p = plan_sparse(n_rays, S, c->sparse_chunk);   // the rays of a chunk, and the scratch laid out for that many
    SparseSlot& slot = c->sparse.next();   // not a slot of the render ring (see nwe_create_rays)
    int host_waits = 0;
    TRY(async ? ready_async(c, p, slot, m, stream, &host_waits) : ready_sync(c, p, slot, m, stream));
    const RenderArgs a = frame_args(c, m, slot.poses.get(), out->rgb, out->depth, out->acc, out->flags);
    uint8_t* const base = c->d_sparse_scratch.get();
    SparseChunk k = {};
    k.S = S; k.min_weight = min_weight; k.dilate = dilate;
    k.row_grid = reinterpret_cast<float4*>(base + p.at_grid); k.rows = reinterpret_cast<const float4*>(base + p.at_rows);
    k.z = reinterpret_cast<float*>(base + p.at_z); k.points = reinterpret_cast<float*>(base + p.at_points);
    k.dirs = net.in_dir != 0 ? reinterpret_cast<float*>(base + p.at_dirs) : nullptr;
    k.offsets = reinterpret_cast<uint32_t*>(base + p.at_offsets); k.total = reinterpret_cast<uint32_t*>(base + p.at_total);
    k.mask = base + p.at_mask;
    k.weights_coarse = out->weights_coarse; k.z_fine = out->z_fine; k.weights_grid = out->weights_grid; k.raw_fine = out->raw_fine;
    k.selected = out->selected;
    const RadianceGrid grid = radiance_grid_args(c);
    QueryArgs q = {};   // the raw path of nwe_query_points, one direction per point, the rows into the scratch
    q.points = k.points; q.dirs = k.dirs; q.raw = reinterpret_cast<float*>(base + p.at_rows); q.points_per_dir = 1;
    volatile uint32_t* const word = static_cast<uint32_t*>(c->sparse_word.h);
    unsigned long long* const tally = slot.tally.get();
    int64_t selected = 0;
    const int rc = record_launch(c, slot, stream, [&]() -> int {
        if (async) HIPCHK(c, hipMemsetAsync(tally, 0, sizeof(unsigned long long), stream));
        for (int64_t first = 0; first < n_rays; first += p.cap) {   // the one buffer is reused in stream order
            k.first = first; k.count = (int)std::min<int64_t>(p.cap, n_rays - first);
            launch_sparse_mark(a, grid, k, stream);
            launch_sparse_scan(k, stream);
            launch_sparse_emit(a, k, stream);
            if (async) {   // the count stays on the device: one add to the tally, and the counted query, sized for all of the chunk's samples
                launch_sparse_tally(k, tally, stream);
                q.n_points = k.count * S;
                TRY(run_query(c, net, q, precision, stream, k.total));
            } else {       // the one read-back of the chunk: the query's launch needs its n_points on the host
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipMemcpyAsync(c->sparse_word.h, k.total, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
                HIPCHK(c, hipStreamSynchronize(stream));
                ++host_waits;
                const uint32_t n_points = *word;
                if ((uint64_t)n_points > (uint64_t)k.count * S) return fail(c, NWE_ERR_HIP, "sparse frame: the chunk's point count is out of range");
                selected += n_points;
                q.n_points = (int)n_points;
                if (n_points > 0) TRY(run_query(c, net, q, precision, stream));   // a chunk with nothing selected launches no query
            }
            launch_sparse_composite(a, k, stream);
            if (async) HIPCHK(c, hipGetLastError());
        }
        if (async) HIPCHK(c, hipMemcpyAsync(slot.word.h, tally, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        return NWE_OK;
    });
    // nothing of a synchronous call may still run, or read the scratch, when it returns; nor may anything of one that failed half way
    const hipError_t waited = !async || rc ? hipStreamSynchronize(stream) : hipSuccess;
    if (rc) return rc;
    HIPCHK(c, waited);
    c->sparse.commit(slot);
    c->sparse_total = n_rays * S;
    if (!async) c->sparse_selected = selected;   // an asynchronous call's are in the slot's pinned word (nwe_last_sparse_samples)
    c->sparse_async = async; c->sparse_host_waits = async ? host_waits : host_waits + 1;
    return NWE_OK;
}

}  // namespace

extern "C" {

int nwe_render_sparse(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                      int row_begin, int row_end, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs* out,
                      void* stream) {
    return render_sparse(c, false, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, which, precision, min_weight, dilate, out,
                         (hipStream_t)stream);
}

int nwe_render_sparse_async(nwe_ctx* c, const float* c2w, int n_poses, int H, int W, float fx, float fy, float cx, float cy, float near, float far,
                            int row_begin, int row_end, int which, int precision, float min_weight, int dilate, const nwe_sparse_outputs* out,
                            void* stream) {
    return render_sparse(c, true, Camera{c2w, n_poses, H, W, fx, fy, cx, cy, near, far, row_begin, row_end}, which, precision, min_weight, dilate, out,
                         (hipStream_t)stream);
}

int nwe_debug_last_sparse_host_waits(nwe_ctx* c) { return c && c->sparse.last_slot >= 0 ? c->sparse_host_waits : -1; }
unsigned nwe_debug_query_counted_grid(int64_t capacity, int packet, int forced_steps, int cus) {
    return query_counted_grid(capacity, packet, forced_steps, cus);
}

int nwe_debug_set_sparse_chunk(nwe_ctx* c, int rays) { return set_on(rays < 0 ? nullptr : c, [&] { c->sparse_chunk = rays; }); }

float nwe_last_sparse_ms(nwe_ctx* c) { return elapsed_ms(c, c ? c->sparse.last() : nullptr, "nwe_last_sparse_ms"); }

int nwe_last_sparse_samples(nwe_ctx* c, int64_t* out2) {
    if (!c || !out2) return NWE_ERR_INVALID;
    if (c->sparse.last_slot < 0) return NWE_ERR_STATE;
    if (c->sparse_async) {   // the tally is in the slot's pinned word once the call's end event has passed
        const SparseSlot& slot = c->sparse.slots[c->sparse.last_slot];
        ON_DEVICE(c);
        HIPCHK(c, hipEventSynchronize(slot.ev1));
        c->sparse_selected = (int64_t)*static_cast<volatile unsigned long long*>(slot.word.h);
        c->sparse_async = false;   // read once
    }
    out2[0] = c->sparse_selected; out2[1] = c->sparse_total;
    return NWE_OK;
}

}  // extern "C"
