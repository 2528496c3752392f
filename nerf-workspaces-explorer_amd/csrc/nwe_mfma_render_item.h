// NOT a header of its own (no include guard: it is included up to three times, inside function bodies).
// The body of a render kernel behind its work item: everything a workgroup does once it knows which item is its own.  Included
// as text, not called (nwe_mfma_render.h: render_mfma_kernel once, render_mfma_tail_kernel once per decomposition): the
// kernel's register allocation does not survive the body as a function, not even a force-inlined one with one call site - the
// headline kernel then spills scalar registers.  The including scope provides
//   W, D, SKIP, X3, SPLIT, FORM, LEAN, TERM, SHARE  compile-time constants (template parameters or constexpr locals)
//   S = Shape<W, D>, SM = Smem<W, D, SPLIT>
//   a (RenderArgs, the kernel's own copy: a.ray_first is the first ray of the item's launch), nc, nf, smem, item
//   NWE_ITEM_OCC, defined by render_mfma_occ_kernel alone, with occ (const OccGrid*: the occupancy grid; that kernel's comment
//   holds the argument).  The occupancy code is under the preprocessor, not under `if constexpr`, so that every other kernel
//   compiles the very tokens it compiled before: their device code is the same to the byte (tools/device_code_digest.py).
//   NWE_ITEM_LIST, defined by render_mfma_list_kernel alone, with list (const int32_t*: the call's pixel list), under the
//   preprocessor for the same reason: the seed comes from the listed pixel, and there are no packet blocks.
//   stamp_item (diagnostic builds only): the item's row group in the stamp buffer
// and NWE_PRIME_STREAM / NWE_EVAL_POINT.  The first word of smem may hold a queued launch's ticket up to the barrier behind the
// table copies.
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5;
    const int ns = a.n_samples, ni = a.n_importance;

    float* s_t = reinterpret_cast<float*>(smem + SM::TOFF);
    float* s_omt = s_t + kMaxSamples;
    float* s_u = s_omt + kMaxSamples;
    for (int i = threadIdx.x; i < ns; i += 256) { s_t[i] = a.t_vals[i]; s_omt[i] = a.omt_vals[i]; }
    for (int i = threadIdx.x; i < ni; i += 256) s_u[i] = a.u_vals[i];
    float* s_bias = reinterpret_cast<float*>(smem + SM::BOFF);
    constexpr int NCH = S::n_chunks(FORM);       // the launcher checks n_chunks of both networks against it
    constexpr int NROWS = S::n_bias_rows(FORM);  // kFormFolded: the alpha layer's weights and bias ride behind the bias rows
    static_assert(NROWS * 32 * 4 <= SM::BIAS_BYTES, "bias table too small for the dot rows");
    for (int i = threadIdx.x; i < NROWS * 32; i += 256) {
        s_bias[i] = nc.bias[i];
        if (ni > 0) s_bias[SM::BIAS_BYTES / 4 + i] = nf.bias[i];
    }

    const int64_t packet = SPLIT ? (int64_t)item : (int64_t)item * kWaves + wave;
    const int64_t ridx64 = a.ray_first + packet * kRaysPerWave + (lane & 31);
    const bool lane_live = ridx64 < a.n_rays && half == 0;    // this lane stores per-sample outputs of its ray
    const bool live = lane_live && (!SPLIT || wave == 0);      // ... and the per-ray results (every wave holds them in SPLIT mode)
    const bool gone = ridx64 >= a.n_rays;                      // TERM: a lane past the call's rays computes along and has no say
    // One 32-bit row index per lane (the ABI keeps n_rays below 2^31): the ray's own index, or the call's last ray for the
    // lanes of a ragged last packet, which compute along and store nothing.  64-bit only where an offset is formed.
    int row_of = (int)(ridx64 < a.n_rays ? ridx64 : a.n_rays - 1);
#if !defined(NWE_ITEM_OCC) && !defined(NWE_ITEM_LIST)
    // A blocked call (nwe_packet_blocks.h; the lean plain and tail kernels, by plan_call's decision): the index names pixel pi(j),
    // so that the packet is an 8x4 block.  Everything from here on - the seed, the tables' rows, every store - sees the pixel; gone,
    // lane_live and live above are the index's, and such a call has no ragged packet.
    if constexpr (LEAN && !TERM && !SHARE) {
        if (a.ray_cols & kPacketBlocksBit) row_of = packet_block_pixel(row_of, a.W);
    }
#endif
    const int row = row_of;
    const int64_t ridx = row, rclamp = row;
    // The ray is kept as its three-register seed and expanded at the top of every sample iteration (bit-identical by
    // construction): nothing of it but |d| stays in registers across an MLP evaluation.  The empty asm hides the seed from
    // loop-invariant code motion, which would otherwise hoist the expansion and spill its results.
    const bool producer = SHARE && share_role(a) == kShareProducer, consumer = SHARE && share_role(a) == kShareConsumer;
#ifdef NWE_ITEM_LIST
    // The seed of the listed pixel: one 4-byte load per lane, here and nowhere else, so the pointer and the pixel are dead before
    // the sample loop.  Clamped into the rays of the camera's own nwe_render call (a.ray_cols poses): whatever the list holds, the
    // pose index make_ray reads with lies in the pose table.  `row` stays the index within the list.
    const RaySeed seed = seed_ray(a, min(max(list[row], 0), a.ray_cols * a.rows * a.W - 1));
#else
    const RaySeed seed = seed_of<SHARE>(a, rclamp);
#endif
    auto fresh_ray = [&]() __attribute__((always_inline)) {
        RaySeed sd = seed;
        asm volatile("" : "+v"(sd.pose), "+v"(sd.x), "+v"(sd.y));
        return make_ray<false>(a, sd);
    };

    Walker<S::CHUNK_BYTES, X3> wk;
    wk.buf0 = smem; wk.lds_chunks = (uint32_t)(uintptr_t)(LDS_AS char*)smem;
    wk.tail0 = smem + SM::LOFF; wk.lds_tail = wk.lds_chunks + SM::LOFF; wk.t3 = 0;
    wk.b = 0; wk.wave = wave; wk.lane_off = lane * 16;

    // gamma(d): once per ray (model_utils.py:23-25 re-embeds the same direction for every sample), parked in LDS
    char* gd_lds = smem + SM::GOFF + wave * (2 * S::KD * kTileBytes) + lane * 16;
    if constexpr (FORM != kFormNoViewDirs) {
        const Ray rv = make_ray<true>(a, seed);
        h8 GDhi[S::KD], GDlo[S::KD];
        encode<2, S::KD, X3>(rv.vx, rv.vy, rv.vz, half, GDhi, GDlo);
#pragma unroll
        for (int k = 0; k < S::KD; ++k) {
            *reinterpret_cast<h8*>(gd_lds + (2 * k) * kTileBytes) = GDhi[k];
            *reinterpret_cast<h8*>(gd_lds + (2 * k + 1) * kTileBytes) = GDlo[k];
        }
    }

    // The hollow path of mlp_eval (colour_skip_built; lean kernels): one word per wave says whether the evaluations of the pass
    // that produces the outputs may leave out the colour layers where no ray of the wave has density.  Set if the launch allows it
    // for that pass's network (NetMfma::colour_skip) and gamma(d) as the view tiles multiply with it is finite for every ray of the
    // wave: a zero or NaN rotation gives NaN there while the sample points, and so sigma, stay finite.  Written and read by the
    // same wave, so it needs no barrier; it costs the sample loop no register (mlp_eval reads it with the gamma(d) fragments).
    constexpr bool CSKIP = LEAN && colour_skip_built<D, SKIP>(FORM);
    const int* skip_word = reinterpret_cast<const int*>(smem + SM::KOFF) + wave;
    if constexpr (CSKIP) {
        bool gd_ok = true;
        const h8* gdh = reinterpret_cast<const h8*>(gd_lds);
#pragma unroll
        for (int k = 0; k < S::KD; ++k) {
            const h8 g = gdh[(2 * k) * (kTileBytes / 16)];
#pragma unroll
            for (int j = 0; j < 8; ++j) gd_ok = gd_ok && __builtin_fabsf((float)g[j]) <= 65504.f;   // lo = v - hi is finite where hi is
        }
        const int allow = (ni > 0 ? nf : nc).colour_skip != 0 && __all(gd_ok);
        if (lane == 0) *reinterpret_cast<int*>(smem + SM::KOFF + wave * 4) = allow;
    }

    FineSampler fs;
    // coarse weights, then the cdf: one buffer per wave (= per packet), or ONE for the workgroup's single packet (SPLIT), which
    // wave 0 alone writes - all four waves compute the same values - and everyone reads behind a workgroup barrier
    fs.wc = reinterpret_cast<float*>(smem + SM::WOFF) + (SPLIT ? 0 : wave * (kPacketMaxSamples * kRaysPerWave)) + (lane & 31);
    const bool wc_writer = !SPLIT || wave == 0;
    fs.stride = kRaysPerWave; fs.u_tab = s_u; fs.ns = ns; fs.ni = ni;
    fs.cd.t_tab = s_t; fs.cd.omt_tab = s_omt; fs.cd.ns = ns;
    fs.cd.jitter = a.t_rand; fs.cd.row = row;                         // training-mode forward: host-drawn random rows
    fs.u_rand = a.u_rand;
    // Up to this barrier nothing may write the chunk buffers (no LDS-DMA piece, no priming): their first word carries a queued
    // launch's ticket until every wave has read it, which this barrier is the first to guarantee.
    __syncthreads();

    Composite comp;
    uint32_t flags = 0;
#ifdef NWE_ITEM_OCC
    int occ_evals = 0;   // the samples of the iterations this workgroup evaluated, both passes
#endif
#ifdef NWE_STAMPS
    unsigned long long st_enc = 0, st_sync = 0, st_mlp = 0, st_comp = 0;
    const unsigned long long st_begin = __builtin_amdgcn_s_memtime();
    const unsigned long long st_real = __builtin_amdgcn_s_memrealtime();   // 100 MHz: the in-kernel clock is d(memtime) / d(memrealtime) x 100 MHz
#endif
    for (int pass = 0; pass < (ni > 0 ? 2 : 1); ++pass) {
        const NetMfma& net = pass == 0 ? nc : nf;
        const float* bias = s_bias + (pass == 0 ? 0 : SM::BIAS_BYTES / 4);
        const float* dot_tab = bias + NCH * 32;
        const int Stot = pass == 0 ? ns : ns + ni;
        // a lean frame with importance sampling reads nothing of the coarse pass but its weights, which depend on sigma alone
        // (mlp_eval: density_only); with ni == 0 the coarse colour is the frame's colour
        const bool density_only = LEAN && density_only_built<D, SKIP>(FORM) && pass == 0 && ni > 0;
        const float* noise = pass == 0 ? a.noise_c : a.noise_f;
        const float* raw_in = pass == 0 ? a.raw_in_c : a.raw_in_f;   // test hook: network outputs from the caller (uniform)
        if (pass == 0 && a.w_in) {                                   // test hook: coarse weights from the caller, no coarse pass
            if (wc_writer) for (int s = 0; s < ns; ++s) fs.wc[s * kRaysPerWave] = a.w_in[rclamp * ns + s];
            continue;
        }
        if constexpr (SHARE) {
            if (pass == 0 && consumer) {                             // the representative's coarse weights instead of a coarse pass
                const float* col = a.share_w + share_rep_of(a, rclamp);
                const int n_rep = share_n_rep(a, share_grid(a));
                if (wc_writer) for (int s = 0; s < ns; ++s) fs.wc[s * kRaysPerWave] = col[(int64_t)s * n_rep];
                continue;
            }
        }
        comp.reset();
        const bool stops = TERM && (pass == 1 || ni == 0);          // the pass that produces the outputs
        const float eps = stops ? a.min_trans : 0.f;                // 0: nothing is ever below
        if constexpr (SPLIT) {
            // depths are produced strictly in order: zq[0..3] = this iteration's four samples, zq[4] = the first of the next
            int produced = 0;
            auto gen = [&](const Ray& ray) -> float {
                const int i = produced++;
                if (i >= Stot) return 0.f;
                if (pass == 0) return fs.cd.z(ray, i);
                return a.z_fine_in ? a.z_fine_in[rclamp * Stot + i] : fs.next(ray);
            };
            float zq[5], zp[4];
            {
                const Ray ray = fresh_ray();
                if (pass == 1) {
                    if (wc_writer) fs.build_cdf();     // in place: one wave, then everyone reads
                    __syncthreads();
                    fs.start(ray);
                    if (wants_survey(a.out)) {
                        const SampleSurvey sv = fs.survey(ray);
                        if (live) flags |= store_survey(a.out, ridx, sv);
                    }
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) zq[k] = gen(ray);
            }
            float4* xch = reinterpret_cast<float4*>(smem + SM::XOFF);
            const int n_it = (Stot + 3) / 4;
            // composite the (up to four) samples of iteration `it`, shaded by the four waves, in sample order
            auto drain = [&](int it) {
                const float4* x = xch + (it & 1) * (kWaves * kRaysPerWave) + (lane & 31);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int si = 4 * it + k;
                    if (si < Stot) {
                        const float w = TERM ? comp.accumulate_above(x[k * kRaysPerWave], zp[k], eps) : comp.accumulate(x[k * kRaysPerWave], zp[k]);
                        if (pass == 0) {
                            if (wc_writer) fs.wc[si * kRaysPerWave] = w;
                            if constexpr (SHARE) { if (producer && live) a.share_w[si * a.n_rays + row] = w; }   // n_rays = n_rep
                            if (live && a.out.weights_coarse) a.out.weights_coarse[ridx * ns + si] = w;
                        }
                    }
                }
            };
            [[maybe_unused]] int it_end = n_it;   // TERM: the iterations that ran
            for (int it = 0; it < n_it; ++it) {
                if constexpr (TERM) {
                    // comp holds the samples of iterations 0 .. it - 2: iteration it - 1 is composited behind this one's barrier
                    if (stops && it > 0 && __all(gone || comp.below(eps))) { it_end = it; break; }
                }
#ifdef NWE_ITEM_OCC
                // the vote on this iteration's four samples, one per wave
                unsigned long long occ_mask = 0;   // the lanes whose sample lies in an empty cell
                bool occ_skip = false;             // workgroup-uniform: nothing is evaluated
                {
                    const OccGrid* g = occ;
                    asm volatile("" : "+s"(g));   // read again every iteration: nothing of the grid stays in registers across an evaluation
                    const Ray ray = fresh_ray();
                    float zo = zq[0];
                    if (wave == 1) zo = zq[1];
                    if (wave == 2) zo = zq[2];
                    if (wave == 3) zo = zq[3];
                    float px, py, pz;
                    point_at(ray, zo, px, py, pz);
                    const bool empty = occ_empty(g, px, py, pz);
                    occ_mask = __ballot(empty);
                    const int mine = __all(gone || 4 * it + wave >= Stot || empty);
                    int* vote = reinterpret_cast<int*>(smem + SM::TOTAL);
                    if (lane == 0) vote[(it & 1) * kWaves + wave] = mine;
                    __syncthreads();
                    const int* v = vote + (it & 1) * kWaves;
                    occ_skip = __builtin_amdgcn_readfirstlane(v[0] & v[1] & v[2] & v[3]) != 0;
                    if (!occ_skip) occ_evals += Stot - 4 * it < 4 ? Stot - 4 * it : 4;
                }
#endif
                NWE_STAMP(const unsigned long long t0 = __builtin_amdgcn_s_memtime();)
#ifdef NWE_ITEM_OCC
                if (!occ_skip)
#endif
                if (!raw_in) NWE_PRIME_STREAM();
                const Ray ray = fresh_ray();
                const int s_own = 4 * it + wave;
                const bool own_valid = s_own < Stot;
                float z_own = zq[0], z_nxt = zq[1];
                if (wave == 1) { z_own = zq[1]; z_nxt = zq[2]; }
                if (wave == 2) { z_own = zq[2]; z_nxt = zq[3]; }
                if (wave == 3) { z_own = zq[3]; z_nxt = zq[4]; }
                float nz[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) nz[k] = gen(ray);
                float rr, rg, rb, rs;
                if (raw_in) {
                    __syncthreads();             // publishes the previous iteration's shaded samples
                    if (it > 0) drain(it - 1);
#pragma unroll
                    for (int k = 0; k < 4; ++k) zp[k] = zq[k];
                    read_raw(raw_in, rclamp * Stot + (own_valid ? s_own : Stot - 1), rr, rg, rb, rs);
#ifdef NWE_ITEM_OCC
                } else if (occ_skip) {
                    // the vote's barrier has published the previous iteration's shaded samples
                    if (it > 0) drain(it - 1);
#pragma unroll
                    for (int k = 0; k < 4; ++k) zp[k] = zq[k];
                    rr = rg = rb = rs = 0.f;
#endif
                } else {
                    // its barrier also publishes the previous iteration's shaded samples; they are composited behind the fragment
                    // reads, whose latency that covers
                    NWE_EVAL_POINT(z_own, if (it > 0) drain(it - 1); _Pragma("unroll") for (int k = 0; k < 4; ++k) zp[k] = zq[k];);
#ifdef NWE_ITEM_OCC
                    if ((occ_mask >> lane) & 1) rr = rg = rb = rs = 0.f;   // all four channels (include/nwe.h)
#endif
                }
                NWE_STAMP(const unsigned long long t3 = __builtin_amdgcn_s_memtime();)
                if (own_valid) {
                    xch[(it & 1) * (kWaves * kRaysPerWave) + wave * kRaysPerWave + (lane & 31)] =
                        Composite::shade(rr, rg, rb, rs, z_own, z_nxt, s_own + 1 == Stot, ray.dnorm, noise ? noise[rclamp * Stot + s_own] : 0.f);
                    if (lane_live) {
                        float* raw = pass == 0 ? a.out.raw_coarse : a.out.raw_fine;
                        if (raw && store_raw(raw + (ridx * Stot + s_own) * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
                        if (pass == 1 && a.out.z_fine) a.out.z_fine[ridx * Stot + s_own] = z_own;
                    }
                }
                zq[0] = zq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) zq[k + 1] = nz[k];
                NWE_STAMP(st_comp += __builtin_amdgcn_s_memtime() - t3;)
            }
            __syncthreads();
            drain(TERM ? it_end - 1 : n_it - 1);   // TERM: the last iteration that ran (it_end >= 1)
            __syncthreads();   // the exchange buffers are free again for the next pass
            if constexpr (TERM) {
                if (stops) {
                    const unsigned long long mine = __popcll(__ballot(lane_live));
                    const int walked = (ni > 0 ? ns : 0) + (4 * it_end < Stot ? 4 * it_end : Stot);
                    if (wave == 0 && lane == 0) atomicAdd(a.evals, mine * (unsigned long long)walked);
                }
            }
        } else {
            float z_cur, z_next = 0.f;
            {
                const Ray ray = fresh_ray();
                if (pass == 0) z_cur = fs.cd.z(ray, 0);
                else {
                    fs.prepare(ray);
                    if (wants_survey(a.out)) {
                        const SampleSurvey sv = fs.survey(ray);
                        if (live) flags |= store_survey(a.out, ridx, sv);
                    }
                    z_cur = a.z_fine_in ? a.z_fine_in[rclamp * Stot] : fs.next(ray);
                }
            }
            [[maybe_unused]] int s_end = Stot;   // TERM: the iterations that ran
            for (int s = 0; s < Stot; ++s) {
                if constexpr (TERM) {
                    if (stops) {
                        int* vote = reinterpret_cast<int*>(smem + SM::TOTAL);
                        const int mine = __all(gone || comp.below(eps));
                        if (lane == 0) vote[(s & 1) * kWaves + wave] = mine;
                        if (s > 0) {
                            const int* v = vote + ((s - 1) & 1) * kWaves;
                            if (__builtin_amdgcn_readfirstlane(v[0] & v[1] & v[2] & v[3])) { s_end = s; break; }
                        }
                    }
                }
#ifdef NWE_ITEM_OCC
                // the vote on this iteration's sample of the workgroup's four packets
                unsigned long long occ_mask = 0;   // the lanes whose sample lies in an empty cell
                bool occ_skip = false;             // workgroup-uniform: nothing is evaluated
                {
                    const OccGrid* g = occ;
                    asm volatile("" : "+s"(g));   // read again every iteration: nothing of the grid stays in registers across an evaluation
                    const Ray ray = fresh_ray();
                    float px, py, pz;
                    point_at(ray, z_cur, px, py, pz);
                    const bool empty = occ_empty(g, px, py, pz);
                    occ_mask = __ballot(empty);
                    const int mine = __all(gone || empty);
                    const int n = pass == 0 ? s : ns + s;   // the iteration's number over both passes: no barrier separates them
                    int* vote = reinterpret_cast<int*>(smem + SM::TOTAL);
                    if (lane == 0) vote[(n & 1) * kWaves + wave] = mine;
                    __syncthreads();
                    const int* v = vote + (n & 1) * kWaves;
                    occ_skip = __builtin_amdgcn_readfirstlane(v[0] & v[1] & v[2] & v[3]) != 0;
                    if (!occ_skip) ++occ_evals;
                }
#endif
                NWE_STAMP(const unsigned long long t0 = __builtin_amdgcn_s_memtime();)
#ifdef NWE_ITEM_OCC
                if (!occ_skip)
#endif
                if (!raw_in) NWE_PRIME_STREAM();
                const Ray ray = fresh_ray();
                if (s + 1 < Stot) {
                    if (pass == 0) z_next = fs.cd.z(ray, s + 1);
                    else z_next = a.z_fine_in ? a.z_fine_in[rclamp * Stot + s + 1] : fs.next(ray);
                }
                float rr, rg, rb, rs;
                if (raw_in) {
                    read_raw(raw_in, rclamp * Stot + s, rr, rg, rb, rs);
#ifdef NWE_ITEM_OCC
                } else if (occ_skip) {
                    rr = rg = rb = rs = 0.f;
#endif
                } else {
                    NWE_EVAL_POINT(z_cur, );
#ifdef NWE_ITEM_OCC
                    if ((occ_mask >> lane) & 1) rr = rg = rb = rs = 0.f;   // all four channels (include/nwe.h)
#endif
                }
                NWE_STAMP(const unsigned long long t3 = __builtin_amdgcn_s_memtime();)
                const float4 shaded = Composite::shade(rr, rg, rb, rs, z_cur, z_next, s + 1 == Stot, ray.dnorm, noise ? noise[rclamp * Stot + s] : 0.f);
                const float w = TERM ? comp.accumulate_above(shaded, z_cur, eps) : comp.accumulate(shaded, z_cur);
                if (pass == 0) fs.wc[s * kRaysPerWave] = w;
                if constexpr (SHARE) { if (producer && lane_live) a.share_w[s * a.n_rays + row] = w; }   // n_rays = n_rep
                if (lane_live) {
                    if (pass == 0 && a.out.weights_coarse) a.out.weights_coarse[ridx * ns + s] = w;
                    float* raw = pass == 0 ? a.out.raw_coarse : a.out.raw_fine;
                    if (raw && store_raw(raw + (ridx * Stot + s) * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
                    if (pass == 1 && a.out.z_fine) a.out.z_fine[ridx * Stot + s] = z_cur;
                }
                z_cur = z_next;
                NWE_STAMP(st_comp += __builtin_amdgcn_s_memtime() - t3;)
            }
            if constexpr (TERM) {
                if (stops) {
                    const unsigned long long mine = __popcll(__ballot(lane_live));
                    if (lane == 0 && mine) atomicAdd(a.evals, mine * (unsigned long long)((ni > 0 ? ns : 0) + s_end));
                }
            }
        }
        if (live) {
            // density-only coarse pass: there is no coarse colour whose flag could be raised (include/nwe.h)
            flags |= store_ray(a.out, ridx, comp, pass == 1, a.white_bkgd != 0) & (density_only ? ~(uint32_t)NWE_FLAG_RGB_COARSE : ~0u);
            if (ni == 0) flags |= store_ray(a.out, ridx, comp, true, a.white_bkgd != 0);
        }
        // the table is the producer's only result; its coarse flag bits reach a flag word only where the launcher gave it one
        // (separate passes at k = 1, where every ray runs its own coarse pass: nwe_abi.hip)
        if (producer) break;
    }
#ifdef NWE_ITEM_OCC
    {   // every wave of a sample-split workgroup holds the same 32 rays: wave 0 counts them
        const unsigned long long mine = __popcll(__ballot(lane_live));
        if (lane == 0 && mine && (!SPLIT || wave == 0)) atomicAdd(a.evals, mine * (unsigned long long)occ_evals);
    }
#endif
    if (flags && a.out.flags) atomicOr(a.out.flags, flags);
#ifdef NWE_STAMPS
    if (a.stamps && lane == 0) {   // diagnostic build only: a buffer no other code reads
        unsigned long long* o = a.stamps + ((size_t)stamp_item * kWaves + wave) * kStampWords;   // by work item: however it was dealt
        o[0] = st_enc; o[1] = st_sync; o[2] = st_mlp; o[3] = st_comp; o[4] = __builtin_amdgcn_s_memtime() - st_begin;
        o[5] = wk.st_pre; o[6] = wk.st_wait; o[7] = wk.st_post;
        const unsigned long long st_real_end = __builtin_amdgcn_s_memrealtime();
        o[8] = st_real_end - st_real; o[9] = st_begin;
        // where and when the wave ran: HW_REG_XCC_ID (register 20; the XCD is its low four bits) with HW_REG_HW_ID (register 4:
        // wave, SIMD, CU, shader array and engine) above it, the work item, and the wave's span on the 100 MHz clock
        o[10] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) | (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 32;
        o[11] = stamp_item; o[12] = st_real; o[13] = st_real_end;
    }
#endif
