// One step of the fp32 point query, as text: included at the one place in the step loop of query_f32_kernel and of
// query_f32_counted_kernel (nwe_kernel_f32.hip), so that both hold the same statements in the same order.  No include guard.
// Reads from the including scope: a (QueryArgs), net (NetF32), n (points of the call, > 0), first (int64_t: the first point of this
// step's packet, < n), tid, owner, the s_* buffers and the template argument VIEW.  Writes: flags.
        const int64_t idx = first + tid;
        if (owner) {
            const int row = (int)(idx < n ? idx : n - 1);
            const float* p = a.points + (int64_t)row * 3;
            s_pt[0 * kRP + tid] = p[0]; s_pt[1 * kRP + tid] = p[1]; s_pt[2 * kRP + tid] = p[2];
            if constexpr (VIEW) {
                float vx = 0.f, vy = 0.f, vz = 0.f;      // no directions given: sigma does not depend on them
                if (a.dirs) {
                    const float* d = a.dirs + (int64_t)(row / a.points_per_dir) * 3;
                    vx = d[0]; vy = d[1]; vz = d[2];
                }
                s_dir[0 * kRP + tid] = vx; s_dir[1 * kRP + tid] = vy; s_dir[2 * kRP + tid] = vz;
            }
        }
        __syncthreads();
        if constexpr (VIEW) encode16(s_gd, s_dir, net.in_dir, 1.f);   // handler.py:101 scalar_factor = 1
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
        if constexpr (!VIEW) {
            // use_view_dirs=False, nerf_model.py:82-83: channels 0..2 rgb_raw, 3 sigma_raw of _output_linear(h)
            dense16(net.blob, net.output, cur, net.W, nullptr, 0, nxt, false);
            if (tid < 4 * kRP) s_raw[tid] = nxt[tid];
            __syncthreads();
        } else {
            // heads: nerf_model.py:63-74
            dense16(net.blob, net.alpha, cur, net.W, nullptr, 0, s_raw + 3 * kRP, false);
            dense16(net.blob, net.feature, cur, net.W, nullptr, 0, nxt, false);
            dense16(net.blob, net.views, nxt, net.W, s_gd, net.in_dir, cur, true);
            dense16(net.blob, net.rgb, cur, net.W / 2, nullptr, 0, s_raw, false);
        }
        if (owner && idx < n) {
            const float rr = s_raw[0 * kRP + tid], rg = s_raw[1 * kRP + tid], rb = s_raw[2 * kRP + tid], rs = s_raw[3 * kRP + tid];
            if (a.raw) {
                *reinterpret_cast<float4*>(a.raw + idx * 4) = make_float4(rr, rg, rb, rs);
                if (bad(rr) || bad(rg) || bad(rb) || bad(rs)) flags |= NWE_FLAG_RAW;
            }
            if (a.sigma) {
                a.sigma[idx] = rs;
                if (bad(rs)) flags |= NWE_FLAG_RAW;
            }
        }
        // s_pt / s_dir are rewritten at the top of the next step, behind the barrier every thread passed after encode16 read
        // them; s_raw only behind the next step's barriers, which an owner reaches after its reads above.
