// NOT a header of its own (no include guard: it is included once per render kernel of nwe_kernel_f32.hip, inside the function body).
// The body of the fp32 render kernel.  Included as text so that the occupancy kernel, which has a name of its own, shares it
// with render_f32_kernel without a line of the latter's device code changing.  The including scope provides
//   TERM, SHARE, OCC  compile-time constants (template parameters or constexpr locals)
//   a (RenderArgs), nc, nf (NetF32), occ (const OccGrid*, null unless OCC)
    __shared__ __attribute__((aligned(16))) float s_gx[96 * kRP];
    __shared__ __attribute__((aligned(16))) float s_gd[64 * kRP];
    __shared__ __attribute__((aligned(16))) float s_ha[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_hb[256 * kRP];
    __shared__ __attribute__((aligned(16))) float s_pt[3 * kRP];
    __shared__ __attribute__((aligned(16))) float s_raw[4 * kRP];
    __shared__ float s_wcur[kRP];   // endpoint_feat: the weight of the current sample, per ray of the packet
    __shared__ float s_w[kMaxSamples * kRP];
    __shared__ float s_t[kMaxSamples], s_omt[kMaxSamples], s_u[kMaxImportance];

    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kRP;
    const bool owner = tid < kRP;
    const int64_t ridx = base + tid;
    const bool live = owner && ridx < a.n_rays;
    const int ns = a.n_samples, ni = a.n_importance;

    for (int i = tid; i < ns; i += 256) { s_t[i] = a.t_vals[i]; s_omt[i] = a.omt_vals[i]; }
    for (int i = tid; i < ni; i += 256) s_u[i] = a.u_vals[i];

    const bool producer = SHARE && share_role(a) == kShareProducer, consumer = SHARE && share_role(a) == kShareConsumer;
    Ray ray = {};
    if (owner) {
        const int64_t at = live ? ridx : a.n_rays - 1;
        ray = make_ray<true>(a, seed_of<SHARE>(a, at));
        s_pt[0 * kRP + tid] = ray.vx; s_pt[1 * kRP + tid] = ray.vy; s_pt[2 * kRP + tid] = ray.vz;
    }
    __syncthreads();
    encode16(s_gd, s_pt, nc.in_dir, 1.f);   // handler.py:101 scalar_factor = 1; same for every sample (model_utils.py:23-25)
    __syncthreads();

    Composite comp; comp.reset();
    FineSampler fs;
    fs.wc = s_w + tid; fs.stride = kRP; fs.u_tab = s_u; fs.ns = ns; fs.ni = ni;
    fs.cd.t_tab = s_t; fs.cd.omt_tab = s_omt; fs.cd.ns = ns;
    const int64_t rrow = live ? ridx : a.n_rays - 1;
    fs.cd.jitter = a.t_rand; fs.cd.row = (int)rrow;
    fs.u_rand = a.u_rand;
    uint32_t flags = 0;
    [[maybe_unused]] int occ_evals = 0;   // OCC: the sample iterations this workgroup evaluated, both passes

    for (int pass = 0; pass < (ni > 0 ? 2 : 1); ++pass) {
        const NetF32& net = pass == 0 ? nc : nf;
        const int S = pass == 0 ? ns : ns + ni;
        const float* raw_in = pass == 0 ? a.raw_in_c : a.raw_in_f;          // test hook: network outputs from the caller
        if (pass == 0 && a.w_in) {                                          // test hook: coarse weights from the caller
            if (owner) for (int s = 0; s < ns; ++s) s_w[s * kRP + tid] = a.w_in[rrow * ns + s];
            continue;
        }
        if constexpr (SHARE) {
            if (pass == 0 && consumer) {                                    // the representative's coarse weights
                if (owner) {
                    const float* col = a.share_w + share_rep_of(a, rrow);
                    const int n_rep = share_n_rep(a, share_grid(a));
                    for (int s = 0; s < ns; ++s) s_w[s * kRP + tid] = col[(int64_t)s * n_rep];
                }
                continue;
            }
        }
        const bool want_feat = pass == 1 && a.out.feat_map != nullptr && !raw_in;   // uniform
        float facc[kRP];
#pragma unroll
        for (int p = 0; p < kRP; ++p) facc[p] = 0.f;
        const float* s_feat = s_ha;
        const bool stops = TERM && (pass == 1 || ni == 0);   // the pass that produces the outputs
        const float eps = stops ? a.min_trans : 0.f;
        float z_cur = 0.f, z_next = 0.f;
        if (owner) {
            comp.reset();
            if (pass == 0) { z_cur = fs.cd.z(ray, 0); }
            else {
                fs.prepare(ray);
                if (wants_survey(a.out)) {
                    const SampleSurvey sv = fs.survey(ray);
                    if (live) flags |= store_survey(a.out, ridx, sv);
                }
                z_cur = a.z_fine_in ? a.z_fine_in[(live ? ridx : a.n_rays - 1) * S] : fs.next(ray);
            }
        }
        int s = 0;
        for (; s < S; ++s) {
            if constexpr (TERM) {
                // uniform: every thread gets the same answer from the one barrier (a thread that owns no ray agrees)
                if (stops && __syncthreads_and(!live || comp.below(eps))) break;
            }
            [[maybe_unused]] bool empty = false, skip_eval = false;
            if constexpr (OCC) {
                if (owner) {
                    float px, py, pz; point_at(ray, z_cur, px, py, pz);
                    empty = occ_empty(occ, px, py, pz);
                }
                // uniform: every thread gets the same answer from the one barrier (a thread that owns no live ray agrees)
                skip_eval = __syncthreads_and(!live || empty);
                if (!skip_eval) ++occ_evals;
            }
            if (owner) {
                if (s + 1 < S) {
                    if (pass == 0) z_next = fs.cd.z(ray, s + 1);
                    else z_next = a.z_fine_in ? a.z_fine_in[(live ? ridx : a.n_rays - 1) * S + s + 1] : fs.next(ray);
                }
                float px, py, pz; point_at(ray, z_cur, px, py, pz);
                s_pt[0 * kRP + tid] = px; s_pt[1 * kRP + tid] = py; s_pt[2 * kRP + tid] = pz;
            }
            __syncthreads();
            if (raw_in) {
                if (owner) {
                    const float4 v = *reinterpret_cast<const float4*>(raw_in + (rrow * S + s) * 4);
                    s_raw[0 * kRP + tid] = v.x; s_raw[1 * kRP + tid] = v.y; s_raw[2 * kRP + tid] = v.z; s_raw[3 * kRP + tid] = v.w;
                }
            } else if (OCC && skip_eval) {
                // every live ray's sample lies in an empty cell: nothing is evaluated (s_raw is stale and not read below)
            } else {
            encode16(s_gx, s_pt, net.in_xyz, 10.f);   // handler.py:93 scalar_factor = 10
            __syncthreads();
            // trunk: nerf_model.py:53-59
            float* cur = s_ha; float* nxt = s_hb;
            dense16(net.blob, net.pts[0], s_gx, net.in_xyz, nullptr, 0, cur, true);
            for (int i = 1; i < net.D; ++i) {
                if (i == net.skip + 1) dense16(net.blob, net.pts[i], s_gx, net.in_xyz, cur, net.W, nxt, true);
                else dense16(net.blob, net.pts[i], cur, net.W, nullptr, 0, nxt, true);
                float* t = cur; cur = nxt; nxt = t;
            }
            if (net.in_dir == 0) {
                // use_view_dirs=False, nerf_model.py:82-83: outputs = _output_linear(h); channels 0..2 rgb_raw, 3 sigma_raw
                // (model_utils.py:62,71), the rest unused.  out_ch rows land in nxt, the four that matter are copied.
                dense16(net.blob, net.output, cur, net.W, nullptr, 0, nxt, false);
                if (tid < 4 * kRP) s_raw[tid] = nxt[tid];
                __syncthreads();
            } else {
            // heads: nerf_model.py:63-74.  alpha (1 row) goes to s_raw row 3, feature to nxt, views to cur, rgb to s_raw rows 0..2
            dense16(net.blob, net.alpha, cur, net.W, nullptr, 0, s_raw + 3 * kRP, false);
            dense16(net.blob, net.feature, cur, net.W, nullptr, 0, nxt, false);
            dense16(net.blob, net.views, nxt, net.W, s_gd, net.in_dir, cur, true);
            dense16(net.blob, net.rgb, cur, net.W / 2, nullptr, 0, s_raw, false);
            s_feat = cur;                         // the view layer's output [W/2][16]: the endpoint feature (nerf_model.py:72-73)
            }
            }
            if (owner) {
                float rr = s_raw[0 * kRP + tid], rg = s_raw[1 * kRP + tid], rb = s_raw[2 * kRP + tid],
                      rs = s_raw[3 * kRP + tid];
                if constexpr (OCC) { if (empty || skip_eval) rr = rg = rb = rs = 0.f; }   // all four channels (include/nwe.h)
                const float* nz = pass == 0 ? a.noise_c : a.noise_f;
                const float4 shaded = Composite::shade(rr, rg, rb, rs, z_cur, z_next, s + 1 == S, ray.dnorm, nz ? nz[rrow * S + s] : 0.f);
                const float w = TERM ? comp.accumulate_above(shaded, z_cur, eps) : comp.accumulate(shaded, z_cur);
                if (pass == 0) s_w[s * kRP + tid] = w;
                if constexpr (SHARE) { if (producer && live) a.share_w[s * a.n_rays + ridx] = w; }   // n_rays = n_rep
                if (want_feat) s_wcur[tid] = w;
                if (live) {
                    if (pass == 0 && a.out.weights_coarse) a.out.weights_coarse[ridx * S + s] = w;
                    float* raw = pass == 0 ? a.out.raw_coarse : a.out.raw_fine;
                    if (raw) {
                        float4* dst = reinterpret_cast<float4*>(raw + (ridx * S + s) * 4);
                        *dst = make_float4(rr, rg, rb, rs);
                        if (bad(rr) || bad(rg) || bad(rb) || bad(rs)) flags |= NWE_FLAG_RAW;
                    }
                    if (pass == 1 && a.out.z_fine) a.out.z_fine[ridx * S + s] = z_cur;
                }
                z_cur = z_next;
            }
            if (want_feat) {
                // feat_map = sum_s weights * feat (model_utils.py:87-89): thread n owns channel n for the 16 rays of the packet.
                // s_feat is rewritten by the next sample's trunk only behind a barrier every thread passes after this.
                __syncthreads();
                if (tid < net.W / 2) {
#pragma unroll
                    for (int p = 0; p < kRP; ++p) facc[p] = __fadd_rn(facc[p], __fmul_rn(s_wcur[p], s_feat[tid * kRP + p]));
                }
            }
            // s_pt / s_raw are rewritten only after the next barrier pair; the owners' reads above are
            // ordered before their own writes at the top of the next iteration.
        }
        if constexpr (TERM) {
            if (stops && tid == 0) {
                const int64_t mine = a.n_rays - base < kRP ? a.n_rays - base : kRP;
                atomicAdd(a.evals, (unsigned long long)mine * (unsigned long long)((ni > 0 ? ns : 0) + s));
            }
        }
        if (want_feat && tid < net.W / 2) {
            for (int p = 0; p < kRP; ++p)
                if (base + p < a.n_rays) a.out.feat_map[(base + p) * (net.W / 2) + tid] = facc[p];
        }
        if (producer) break;   // the table is the producer's only result
        if (live) {
            flags |= store_ray(a.out, ridx, comp, pass == 1, a.white_bkgd != 0);
            if (ni == 0) flags |= store_ray(a.out, ridx, comp, true, a.white_bkgd != 0);   // coarse-only: fill the "fine" slots too
        }
    }
    if constexpr (OCC) {
        if (tid == 0) {
            const int64_t mine = a.n_rays - base < kRP ? a.n_rays - base : kRP;
            atomicAdd(a.evals, (unsigned long long)mine * (unsigned long long)occ_evals);
        }
    }
    if (flags && a.out.flags) atomicOr(a.out.flags, flags);
