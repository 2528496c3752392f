// One step of a query workgroup (nwe_mfma_query.h), as text: included at the one place in the step loop of query_mfma_kernel and
// of query_mfma_counted_kernel (the nwe_mfma_render_item.h precedent), so that both kernels hold the same statements in the
// same order and no call boundary stands between the step and the registers of its loop.  No include guard: it is text.
// Reads from the including scope:  a (QueryArgs), net (NetMfma), n (points of the call, > 0), first (int64_t: the first point of
// this step's packet, < n), wk, bias, dot_tab, gd_lds, lane, wave, half, density_only; the template arguments W, D, SKIP, X3,
// FORM and the aliases S, SM.  Writes: flags.
        {   // start streaming chunks 0 and 1 (layer 0, tiles 0 and 1): they fly while the point is loaded and encoded
            wk.start(net.stream, bias);
            wk.begin(S::N_L0, 0, 0);
#pragma unroll
            for (int i = 0; i < S::N_L0; ++i) wk.piece(i);
            wk.begin(S::N_L0, 1, 1);
#pragma unroll
            for (int i = 0; i < S::N_L0; ++i) wk.piece(i);
        }
        const int64_t idx = first + wave * kRaysPerWave + (lane & 31);
        const bool live = idx < n && half == 0;          // this lane stores the outputs of its point
        const int row = (int)(idx < n ? idx : n - 1);    // a lane past the call's points computes the last one along
        const float* p = a.points + (int64_t)row * 3;
        const float px = p[0], py = p[1], pz = p[2];
        if constexpr (FORM != kFormNoViewDirs) {
            // gamma(d) of this step's points into the wave's OWN slots (model_utils.py:23-25 embeds the direction of every
            // point).  No barrier guards the write: the slots are private to the wave - slot address = f(wave, lane) - so the only
            // earlier accesses are this wave's own reads in the previous step's mlp_eval, and LDS serves the accesses of one
            // wave in the order it issued them; the reads of this step's mlp_eval are issued behind the write likewise (and
            // behind the lgkmcnt(0) of the barrier below).  LDS-DMA pieces never land here (chunk buffers and tail slots only).
            float vx = 0.f, vy = 0.f, vz = 0.f;          // no directions given: sigma does not depend on them
            if (a.dirs) {
                const float* d = a.dirs + (int64_t)(row / a.points_per_dir) * 3;
                vx = d[0]; vy = d[1]; vz = d[2];
            }
            h8 GDhi[S::KD], GDlo[S::KD];
            encode<2, S::KD, X3>(vx, vy, vz, half, GDhi, GDlo);
#pragma unroll
            for (int k = 0; k < S::KD; ++k) {
                *reinterpret_cast<h8*>(gd_lds + (2 * k) * kTileBytes) = GDhi[k];
                *reinterpret_cast<h8*>(gd_lds + (2 * k + 1) * kTileBytes) = GDlo[k];
            }
        }
        float rr, rg, rb, rs;
        {
            h8 Ghi[S::KG], Glo[S::KG];
            // handler.py:93: scalar_factor = 10, a true division (embedding.py:48)
            encode<5, S::KG, X3>(__fdiv_rn(px, 10.f), __fdiv_rn(py, 10.f), __fdiv_rn(pz, 10.f), half, Ghi, Glo);
            wk.template sync<false>();   // publishes chunk 0
            Frags F;
#pragma unroll
            for (int k = 0; k < PD; ++k) {
                F.hi[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k) * kTileBytes);
                if (X3) F.lo[k] = *reinterpret_cast<const h8*>(wk.cur() + lane * 16 + (2 * k + 1) * kTileBytes);
            }
            mlp_eval<W, D, SKIP, X3, FORM>(wk, F, lane, net.inv_scale, Ghi, Glo, gd_lds, dot_tab, density_only, rr, rg, rb, rs);
        }
        if (live) {
            if (a.raw && store_raw(a.raw + idx * 4, rr, rg, rb, rs)) flags |= NWE_FLAG_RAW;
            if (a.sigma) {
                a.sigma[idx] = rs;
                if (bad(rs)) flags |= NWE_FLAG_RAW;
            }
        }
