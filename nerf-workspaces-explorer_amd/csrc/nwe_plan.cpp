// Launch planning (nwe_plan.h): plain C++ without HIP.
#include "nwe_plan.h"

namespace nwe {

// The plan of a launch group: 0 = all packets, 1 = all sample-split, 2 = hybrid; *full_out = the rays of the hybrid plan's first launch.
static int plan_launch(const PassDesc& a, int cus, int64_t* full_out) {
    // One workgroup per CU at a time, so a launch costs (rounds of workgroups) x (sample iterations per workgroup).  Three
    // plans, same arithmetic: all packets; all sample-split (finer units, ~6 % overhead: redundant sequential part and
    // exchange); or the full rounds as packets and the ragged last round sample-split in a second launch behind it.
    const int64_t rays_wg = kWaves * kRaysPerWave;
    // the sample iterations this launch runs: both passes, or - shared coarse pass - the producer's coarse pass alone, the
    // consumer's fine pass alone
    const int s_coarse = a.role == kShareConsumer ? 0 : a.n_samples;
    const int s_fine = a.role == kShareProducer || a.n_importance <= 0 ? 0 : a.n_samples + a.n_importance;
    const double its = (double)(s_coarse + s_fine);
    const double its_split = 1.06 * (double)((s_coarse + 3) / 4 + (s_fine + 3) / 4);
    const auto rounds = [&](int64_t rays, int64_t per_wg) { return (double)(((rays + per_wg - 1) / per_wg + cus - 1) / cus); };
    const int64_t full = (a.n_rays / rays_wg / cus) * cus * rays_wg;            // rays in complete rounds of packet workgroups
    const double t_packet = rounds(a.n_rays, rays_wg) * its;
    const double t_split = rounds(a.n_rays, kRaysPerWave) * its_split;
    const double t_hybrid = full > 0 && full < a.n_rays ? (double)(full / rays_wg / cus) * its + rounds(a.n_rays - full, kRaysPerWave) * its_split : 1e300;
    // two launches when the model promises at least 0.8 %: the 800x800 frame (19 full rounds + 136 workgroups) is 1.0 % by the
    // model and measures -0.4 % (368.4 vs 370.0 ms, alternating, tools/plan_ab.py); a second launch costs a few microseconds
    const double t_single = t_packet <= t_split ? t_packet : t_split;
    int plan = t_hybrid < 0.992 * t_single ? 2 : (t_packet <= t_split ? 0 : 1);
    if (a.decomposition >= 0) plan = a.decomposition;   // nwe_debug_set_decomposition: tests force one
    if (a.n_samples > kPacketMaxSamples) plan = 1;      // only the single-packet workgroup has LDS for that many coarse weights
    *full_out = full;
    return plan;
}

PassPlan plan_pass(const PassDesc& d, int cus) {
    PassPlan p;
    if (d.variant < 0) return p;
    p.ok = true;
    p.variant = d.variant;
    int64_t full = 0;
    p.plan = plan_launch(d, cus, &full);
    // Dealing: the hardware hands workgroup b of a launch to XCD (b + c) mod 8, an eighth of the launch each
    // whatever pace an XCD runs at.  A queued launch deals tickets instead (render_mfma_kernel), from a counter of its own.
    const auto deal = [&](LaunchPlan& l, int64_t ray_first, int64_t rays, bool split) {
        l.ray_first = ray_first; l.rays = rays; l.split = split;
        l.items = mfma_workgroups(rays, split);
        if (d.may_queue && rays > 0 && (d.queue_mode == 1 || l.items > (unsigned)cus)) l.grid = queue_grid(l.items);
    };
    if (p.plan != 2) {
        p.n_launches = 1;
        deal(p.launch[0], 0, d.n_rays, p.plan == 1);
        return p;
    }
    p.n_launches = 2;
    deal(p.launch[0], 0, full, false);
    deal(p.launch[1], full, d.n_rays - full, true);
    if (!d.side || !p.queued()) return p;   // both launches on the caller's stream, the second behind the first
    // The tail path: the surplus workgroups of the queued packets launch render the split items, one ticket each from the
    // call's third counter, and the second launch - the same kernel, behind the first on the device - renders what they
    // left, which is nothing when the surplus covers every item; only then is the path taken.  Otherwise nothing changes:
    // the second launch backfills the first from the side stream, whose low priority keeps its items behind the packets.
    const bool lean = d.lean && (d.stamped_build || !d.stamps);
    p.tail = p.launch[0].grid && d.tail && lean && d.tail_built && d.n_rays > full &&
             p.launch[0].grid - p.launch[0].items >= p.launch[1].items;
    p.tail_items = p.tail ? p.launch[1].items : 0;
    p.fork = p.tail ? kForkBehind : kForkFront;
    return p;
}

// The kernels that serve a stage, or -1: the terminating, the sharing and the occupancy kernels are lean only, and exclude one another; a
// stage that carries a role without being lean (separate passes through the full kernels) is a single-pass render for the
// producer and reads the coarse weights through the hook for the consumer.
static int stage_variant(const CallDesc& c, int role, bool lean, int n_importance, bool w_in, int net) {
    const bool share = role != kShareOff && lean;
    int v = kVariantPlain;
    if (c.list) v = lean && role == kShareOff && !c.term && !c.occ ? kVariantList : -1;
    else if (c.occ) v = lean && role == kShareOff && !c.term ? kVariantOcc : -1;
    else if (c.term) v = lean && !share ? kVariantTerm : -1;
    else if (share) v = n_importance > 0 ? kVariantShare : -1;
    else if (role != kShareOff && (role == kShareProducer ? n_importance != 0 : !w_in)) v = -1;
    return v >= 0 && c.built[net][v] ? v : -1;
}

CallPlan plan_call(const CallDesc& c, int cus) {
    CallPlan p;
    const bool lean = c.lean && !c.stamps;   // what picks the kernels: a stamped launch is not lean
    // Shared coarse pass: with importance samples the call is two launches, the producer over the representatives of the blocks
    // its rows touch (everything but lean pinhole calls has been refused), then the consumer over its rays.
    // Separate passes (MFMA precisions): the same two launches for every call with importance samples, each with the kernel of
    // its own network's shape and with that network in both descriptor slots, so that a kernel copies bias tables of its own
    // shape only.  A lean call takes the sharing kernels, at k = 1 every pixel its own representative; every other call the
    // full kernels: the coarse launch is their single-pass render (n_importance = 0) whose weights_coarse output is the table,
    // the fine launch reads the table through the coarse-weights hook, which takes the place of pass 0.
    // Baked coarse pass (a lean pinhole call - everything else has been refused - with importance samples): the same two
    // stages at k = 1, but the producer fills the table from the context's density grid and is no MFMA launch group; the consumer
    // takes the fine network's sharing kernels with that network in both descriptor slots, so the coarse network's shape is free.
    p.baked = c.baked && c.n_importance > 0;
    p.separate = c.separate && c.mfma && c.n_importance > 0;
    p.share = c.n_importance > 0 && (p.baked || c.share_k > 1 || (p.separate && lean && c.built[0][kVariantShare] && c.built[1][kVariantShare]));
    p.full = p.separate && !p.share;
    p.coarse_launch = p.share || (p.full && !c.w_in);   // with the coarse-weights hook armed there is no coarse pass
    p.share_k = p.share ? c.share_k : 1;
    p.occ = c.occ;
    p.need_evals = c.term || c.occ;
    // the table between the two launches: [n_samples][n_rep] of the sharing kernels, [n_rays][n_samples] of the full ones, which
    // may be the caller's own
    if (p.baked) p.table_elems = c.n_rays * c.n_samples;
    else if (p.share) p.table_elems = c.n_rep * c.n_samples;
    else if (p.full && p.coarse_launch && !c.want_weights_coarse) p.table_elems = c.n_rays * c.n_samples;
    p.coarse_flags = p.full && p.coarse_launch && c.want_flags;

    StagePlan& m = p.main;
    m.active = true;
    m.role = p.share || p.full ? kShareConsumer : kShareOff;
    m.n_rays = c.n_rays; m.n_importance = c.n_importance;
    m.net = p.separate || p.baked ? 1 : -1;
    StagePlan& k = p.coarse;
    if (p.coarse_launch) {
        k.active = true;
        k.role = kShareProducer;
        k.n_rays = p.share && !p.baked ? c.n_rep : c.n_rays;
        k.n_importance = p.share && !p.baked ? c.n_importance : 0;
        k.net = p.separate || p.baked ? 0 : -1;
    }
    p.evals_full = c.n_rays * (int64_t)(c.n_samples + (c.n_importance > 0 ? c.n_samples + c.n_importance : 0));
    if (p.baked) p.evals_run = c.n_rays * (int64_t)(c.n_samples + c.n_importance);   // no coarse evaluation is run
    else p.evals_run = p.coarse_launch ? k.n_rays * c.n_samples + c.n_rays * (int64_t)(c.n_samples + c.n_importance) : p.evals_full;
    p.share_rays = p.coarse_launch ? k.n_rays : 0;
    if (!c.mfma) return p;

    // Work queue: a call that is one fused plain MFMA kernel - plain kernels (and the list kernels, which take the plain kernel's
    // tickets) only: early termination, the occupancy grid, the
    // shared coarse pass and separate passes keep their launches as they are - may deal its workgroups from the slot's counters,
    // and its hybrid plan's second launch may backfill the first from the slot's own stream.
    const bool plain_only = !p.separate && !p.share && !c.term && !c.occ;
    const auto describe = [&](const StagePlan& s, bool stage_lean, bool w_in) {
        PassDesc d;
        d.n_rays = s.n_rays; d.n_samples = c.n_samples; d.n_importance = s.n_importance;
        d.role = s.role;
        d.lean = stage_lean && c.lean; d.stamps = c.stamps; d.stamped_build = c.stamped_build;
        d.variant = stage_variant(c, s.role, stage_lean && lean, s.n_importance, w_in, s.net > 0 ? 1 : 0);
        d.tail_built = c.built[s.net > 0 ? 1 : 0][kVariantTail];
        d.decomposition = c.decomposition; d.queue_mode = c.queue_mode;
        return d;
    };
    // the launches through the full kernels are not lean: the coarse one writes the table, the fine one reads it
    if (k.active && !p.baked) k.pass = plan_pass(describe(k, !p.full, false), cus);
    PassDesc d = describe(m, !p.full, p.full || c.w_in);
    d.may_queue = plain_only && c.queue_mode != 0;
    d.side = c.backfill; d.tail = c.tail && !c.list;   // a pixel list has no tail path: it is planned as the ray list it replaces
    m.pass = plan_pass(d, cus);
    p.may_queue = m.pass.queued();   // a call that queues nothing pays nothing
    p.need_side = p.may_queue && c.backfill;
    // Packets of 8x4 pixel blocks (nwe_packet_blocks.h): a lean pinhole frame that is one fused launch group of the plain kernels
    // (the tail kernel with them) - the terminating, sharing and occupancy kernels and the baked consumer keep their linear
    // packets - whose rows per pose are whole bands and whose width is whole blocks.  Then n_rays, the hybrid plan's first ray
    // of the second launch (whole rounds of 128-ray workgroups) and the tail kernel's split part all are multiples of 32: no
    // packet is ragged, and every packet is one block.
    p.blocks = c.packet_blocks && lean && plain_only && m.pass.ok && m.pass.variant == kVariantPlain && packet_blocks_fit(c.rows, c.width);
    return p;
}

int query_steps(int64_t packets, int forced, int cus) {
    if (forced > 0) return forced < kQueryMaxSteps ? forced : kQueryMaxSteps;
    const int64_t steps = packets / (8 * (int64_t)cus);   // the rule: nwe_plan.h
    return (int)(steps < 1 ? 1 : (steps > kQueryMaxSteps ? kQueryMaxSteps : steps));
}

unsigned query_counted_grid(int64_t capacity, int packet, int forced, int cus) {
    if (capacity <= 0 || packet <= 0) return 0;
    const int64_t packets = (capacity + packet - 1) / packet;
    if (forced > 0) {
        const int64_t steps = forced < kQueryMaxSteps ? forced : kQueryMaxSteps;
        return (unsigned)((packets + steps - 1) / steps);
    }
    const int64_t most = 8 * (int64_t)(cus > 0 ? cus : 1);
    return (unsigned)(packets < most ? packets : most);
}

SparsePlan plan_sparse(int64_t n_rays, int S, int chunk_hook) {
    SparsePlan p;
    p.cap = kSparseChunkSamples / S;
    if (p.cap < 1) p.cap = 1;
    if (chunk_hook > 0 && chunk_hook < p.cap) p.cap = chunk_hook;
    if (n_rays < p.cap) p.cap = n_rays;
    p.chunks = (n_rays + p.cap - 1) / p.cap;
    p.M = p.cap * S;
    const auto take = [&](int64_t n) { const int64_t at = p.bytes; p.bytes += (n + 255) / 256 * 256; return at; };
    p.at_grid = take(p.M * 16); p.at_rows = take(p.M * 16); p.at_z = take(p.M * 4); p.at_points = take(p.M * 12); p.at_dirs = take(p.M * 12);
    p.at_offsets = take(p.cap * 4); p.at_total = take(4); p.at_mask = take(p.M);
    return p;
}

AdaptivePlan plan_adaptive(int n_poses, int rows, int width, int k, int ray_cols) {
    AdaptivePlan p;
    p.h = adaptive_axis(rows, k); p.w = adaptive_axis(width, k);
    p.n_poses = n_poses; p.cols = ray_cols;
    p.pixels = (int64_t)n_poses * rows * width;
    p.lattice = (int64_t)n_poses * p.h.n * p.w.n;
    p.cells = (int64_t)n_poses * p.h.cells * p.w.cells;
    p.list = p.lattice > p.pixels - p.lattice ? p.lattice : p.pixels - p.lattice;
    const auto take = [&](int64_t n) { const int64_t at = p.bytes; p.bytes += (n + 255) / 256 * 256; return at; };
    p.at_list = take(p.list * 4); p.at_rays = take(p.list * ray_cols * 4);
    p.at_rgb = take(p.pixels * 12); p.at_depth = take(p.pixels * 4); p.at_acc = take(p.pixels * 4);
    p.at_kind = take(p.pixels); p.at_counts = take(p.pixels * 4); p.at_busy = take(p.cells);
    p.at_total = take(4); p.at_flags = take(4);
    return p;
}

int adaptive_lattice(int first, int last_excl, int k, int32_t* out, int cap) {
    if (first >= last_excl || (int64_t)last_excl - first > INT32_MAX - kAdaptiveMaxK || k < 1 || k > kAdaptiveMaxK || !out) return -1;
    const AdaptiveAxis x = adaptive_axis(last_excl - first, k);
    if (x.n > cap) return -1;
    for (int i = 0; i < x.n; ++i) out[i] = first + adaptive_entry(x, i);
    return x.n;
}

AdaptiveLevelsPlan plan_adaptive_levels(int n_poses, int rows, int width, int k, int levels, int ray_cols) {
    AdaptiveLevelsPlan p;
    p.levels = levels; p.n_poses = n_poses; p.cols = ray_cols;
    p.pixels = (int64_t)n_poses * rows * width;
    int64_t on_lattice = 0;   // the pixels of the level before
    for (int l = 0; l < levels; ++l) {
        p.h[l] = adaptive_axis(rows, adaptive_level_spacing(k, levels, l)); p.w[l] = adaptive_axis(width, adaptive_level_spacing(k, levels, l));
        p.cells[l] = (int64_t)n_poses * p.h[l].cells * p.w[l].cells;
        const int64_t now = (int64_t)n_poses * p.h[l].n * p.w[l].n;
        p.pass_max[l] = now - on_lattice;   // the lattices are nested
        on_lattice = now;
    }
    p.pass_max[levels] = p.pixels - on_lattice;
    p.lattice = p.pass_max[0];
    for (int i = 0; i <= levels; ++i) p.list = p.pass_max[i] > p.list ? p.pass_max[i] : p.list;
    const auto take = [&](int64_t n) { const int64_t at = p.bytes; p.bytes += (n + 255) / 256 * 256; return at; };
    p.at_list = take(p.list * 4); p.at_rays = take(p.list * ray_cols * 4);
    p.at_rgb = take(p.pixels * 12); p.at_depth = take(p.pixels * 4); p.at_acc = take(p.pixels * 4);
    p.at_slot = take(p.pixels * 4); p.at_counts = take(p.pixels * 4);
    for (int l = 0; l < levels; ++l) p.at_state[l] = take(p.cells[l]);
    p.at_words = take(2 * kAdaptiveMaxLevels * 4); p.at_interp = take(kAdaptiveMaxLevels * 4); p.at_flags = take(4);
    return p;
}

int adaptive_levels_lattice(int first, int last_excl, int k, int levels, int level, int32_t* out, int cap) {
    if (!adaptive_levels_ok(k, levels) || level < 0 || level >= levels) return -1;
    return adaptive_lattice(first, last_excl, adaptive_level_spacing(k, levels, level), out, cap);
}

}  // namespace nwe
