"""The occupancy grid on the GPU (include/nwe.h: nwe_set_occupancy; the kernels' part: csrc/nwe_mfma_render.h, nwe_kernel_f32_occ.hip).

The reference is the oracle with the raw rows of empty-cell samples replaced by zero in both passes (tests/occupancy.py); scenes
are a few hundred rays.  Tolerances are the project's parity tolerances (rgb 1e-4, depth 1e-4 * far, acc 1e-4; 1e-3 for f16x1)
on the rays whose every sample is further than 1e-3 of a cell from a cell face; the identities - all bits set, the slab
network's exact grid, the decompositions among themselves - hold to the bit on every ray.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import occupancy as G

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
PRECISIONS = ("f16x3", "f16x1", "f32")
TOL = {"rgb": 1e-4, "depth": 1e-4 * G.FAR, "acc": 1e-4}
TOL_X1 = {"rgb": 1e-3, "depth": 1e-3 * G.FAR, "acc": 1e-3}
DISP_BITS = (1 << 3) | (1 << 7)      # NWE_FLAG_DISP | NWE_FLAG_DISP_COARSE


def _renderer(sd_c, sd_f, cfg, devices=None):
    r = nwe_amd.TiledRenderer(devices) if devices else nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    if cfg.n_importance > 0:
        r.set_network(1, sd_f)
    r.set_sampling(cfg.n_samples, cfg.n_importance)
    return r


def _scene_renderer(name, kind=None, devices=None, n_poses=1):
    sd_c, sd_f, cfg = G.scene(name, n_poses)[:3]
    r = _renderer(sd_c, sd_f, cfg, devices)
    if kind is not None:
        _set(r, G.grid(kind))
    return r


def _set(r, g):
    r.set_occupancy(g["bits"], g["lo"], g["hi"], g["res"])


def _frame(r, poses, H, W, precision, rows=None, outputs=LEAN):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return r.render(poses.numpy(), H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=G.NEAR, far=G.FAR, rows=rows, precision=precision, outputs=outputs)


def _scene_frame(r, name, precision, n_poses=1, **kw):
    _, _, _, poses, _, H, W = G.scene(name, n_poses)
    return _frame(r, poses, H, W, precision, **kw)


def _same(a, b, ctx):
    for k in LEAN:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _modes(precision):
    """(decomposition to force, the helper's kind of group)"""
    return ((-1, "f32"),) if precision == "f32" else ((0, "packets"), (1, "split"))


# ---- 1. all bits set -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fog192", "fog128", "novd"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_bits_set_renders_the_bits_of_no_grid(name, precision):
    cfg = G.scene(name)[2]
    r, plain = _scene_renderer(name, "full"), _scene_renderer(name)
    try:
        n_rays = G.scene(name)[4].shape[0]
        for mode, _ in _modes(precision):
            if mode == 0 and cfg.n_samples > 64:
                continue                      # more than 64 coarse samples: the single-packet workgroup whatever is forced
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            _same(_scene_frame(r, name, precision), _scene_frame(plain, name, precision), (name, precision, mode))
            assert r.last_ray_evaluations() == (G.full_evaluations(cfg, n_rays),) * 2
            if precision != "f32":
                assert r.debug_last_plan() == plain.debug_last_plan()
    finally:
        r.close(); plain.close()


# ---- 2. no bit set ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_bit_set_renders_nothing_and_evaluates_nothing(precision, white):
    """rgb 0 (1 with a white background), depth 0, acc 0, nothing evaluated.  The flag word is the masked oracle's: none of the
    rgb / depth / acc bits, and the two disp bits, because raw2outputs' disp of a ray without weight is 1 / max(1e-10, 0 / 0) =
    NaN in the reference too (model_utils.py:94) and the bits report the reference's pattern whether or not disp is requested
    (include/nwe.h) - as for a ray of zero weight in a call without a grid."""
    r = _scene_renderer("fog7", "none")
    try:
        r.set_white_background(white)
        for mode, _ in _modes(precision):
            r.debug_set_decomposition(mode)
            out = _scene_frame(r, "fog7", precision)
            assert (out["rgb"] == (1.0 if white else 0.0)).all() and (out["depth"] == 0).all() and (out["acc"] == 0).all()
            assert int(out["flags"].item()) == DISP_BITS
            assert r.last_ray_evaluations() == (0, G.full_evaluations(G.scene("fog7")[2], 133))
    finally:
        r.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_outside_a_small_empty_box_everything_is_evaluated(precision):
    """A box smaller than the scene with no bit set: executed equals the helper's count, the frame the masked oracle's."""
    r = _scene_renderer("fog7", "small_none")
    try:
        ref = G.reference("fog7", "small_none")
        decided = ref["decided"]
        assert float(decided.float().mean()) >= 0.85
        for mode, kind in _modes(precision):
            r.debug_set_decomposition(mode)
            out = _scene_frame(r, "fog7", precision)
            lo, hi = G.executed_interval(ref, kind)
            ran = r.last_ray_evaluations()[0]
            print(f"small box {precision} {kind}: executed {ran}, helper [{lo}, {hi}]")
            assert 0 < lo and hi < G.full_evaluations(G.scene("fog7")[2], 133) and lo <= ran <= hi, (precision, kind)
            tol = TOL_X1 if precision == "f16x1" else TOL
            for k in LEAN:
                err = (out[k].cpu() - ref[k]).abs()
                err = err.max(-1).values if err.dim() == 2 else err
                assert float(err[decided].max()) <= tol[k], (precision, k)
            assert float(out["acc"].max()) > 0.05          # the samples outside the box are there
    finally:
        r.close()


# ---- 3. the slab network with its exact grid ----------------------------------------------------------------------------------

@pytest.mark.parametrize("vd", [True, False], ids=["folded", "novd"])
@pytest.mark.parametrize("samples", [(64, 128), (32, 0)], ids=["64+128", "32+0"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_slab_network_with_its_exact_grid(precision, samples, vd):
    """sigma_raw is exactly +0 in every cell the grid marks empty: every output bit-identical to the call without a grid,
    executed < full and inside the helper's interval."""
    sd_c, sd_f = G.slab_state_dict(2000, 4, 128, vd), G.slab_state_dict(2001, 4, 128, vd)
    cfg = O.RenderConfig(n_samples=samples[0], n_importance=samples[1])
    H, W = 12, 64
    poses, rays = G.E.frame_rays(H, W)
    g = G.slab_grid()
    ref = G.masked_render(rays if vd else rays[:, :8].contiguous(), sd_c, sd_f, cfg, g)
    r, plain = _renderer(sd_c, sd_f, cfg), _renderer(sd_c, sd_f, cfg)
    try:
        _set(r, g)
        for mode, kind in _modes(precision):
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            a, b = _frame(r, poses, H, W, precision), _frame(plain, poses, H, W, precision)
            _same(a, b, (precision, samples, vd, mode))
            assert float(a["acc"].max()) > 0.5
            ran, full = r.last_ray_evaluations()
            lo, hi = G.executed_interval(ref, kind)
            print(f"slab {precision} {samples} vd={vd} {kind}: executed {ran} of {full}, helper [{lo}, {hi}]")
            assert full == G.full_evaluations(cfg, H * W) and ran < full and lo <= ran <= hi
    finally:
        r.close(); plain.close()


# ---- 4. parity with the masked oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", G.PARITY_GRIDS)
@pytest.mark.parametrize("name", G.PARITY_SCENES)
def test_parity_with_the_masked_oracle(name, kind):
    """Decided rays within the parity tolerances in every precision (that they are 95 % of the frame and that the reference
    reproduces itself there: tests/test_occupancy_host.py); the undecided rays' errors are printed; and the MFMA frames
    equal the f32 frame within the same tolerances on EVERY ray.
    The checkerboard of the scenes with importance samples (7 + 6) lies over the near box, so that sample_pdf's last bin keeps its
    weight (tests/occupancy.py: NEAR_LO): a checkerboard over the whole scene box masks that bin on some rays, and there one ulp
    of the cdf moves the u = 1 sample by 8e-3 units, across the decided margin."""
    kind = G.parity_kind(name, kind)
    ref = G.reference(name, kind)
    decided = ref["decided"].numpy()
    r = _scene_renderer(name, kind)
    frames = {}
    try:
        for precision in PRECISIONS:
            for mode, _ in _modes(precision):
                r.debug_set_decomposition(mode)
                frames[precision] = out = _scene_frame(r, name, precision)
                tol = TOL_X1 if precision == "f16x1" else TOL
                for k in LEAN:
                    err = np.abs(out[k].cpu().numpy() - ref[k].numpy())
                    err = err.max(-1) if err.ndim == 2 else err
                    und = err[~decided]
                    print(f"{name} {kind} {precision} mode {mode} {k}: max err decided {err[decided].max():.2e} (tol {tol[k]:.0e}), "
                          f"undecided {und.max() if und.size else 0.0:.2e} of {und.size} rays")
                    assert err[decided].max() <= tol[k], (name, kind, precision, mode, k)
        for precision in ("f16x3", "f16x1"):
            tol = TOL_X1 if precision == "f16x1" else TOL
            for k in LEAN:
                err = float((frames[precision][k] - frames["f32"][k]).abs().max())
                print(f"{name} {kind} {precision} vs f32 {k}: {err:.2e}")
                assert err <= tol[k], (name, kind, precision, k)
    finally:
        r.close()


# ---- 5. decompositions, hybrid plan, row tiles, pose batches, TiledRenderer --------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1"])
def test_decompositions_and_the_hybrid_plan_agree_bit_for_bit(precision):
    r = _scene_renderer("fog192", "checker")
    try:
        r.debug_set_decomposition(0)
        base = _scene_frame(r, "fog192", precision)
        assert r.debug_last_plan() == 0
        for mode in (1, 2, -1):
            r.debug_set_decomposition(mode)
            _same(_scene_frame(r, "fog192", precision), base, (precision, mode))
            assert mode < 0 or r.debug_last_plan() == mode
            assert r.debug_last_queue()["grid"] == (0, 0)             # never queued
    finally:
        r.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_row_tiles_pose_batches_and_tiled_renderer_agree_bit_for_bit(precision):
    """fog7 at two poses, 7 x 19: ragged packets everywhere."""
    r = _scene_renderer("fog7", "half", n_poses=2)
    t = _scene_renderer("fog7", "half", devices=[0, 0, 0], n_poses=2)
    try:
        _, _, _, poses, _, H, W = G.scene("fog7", 2)
        whole = _frame(r, poses, H, W, precision)
        singles = [_frame(r, poses[p:p + 1], H, W, precision) for p in range(2)]
        tiles = [[_frame(r, poses[p:p + 1], H, W, precision, rows=rows) for rows in ((0, 3), (3, 4), (4, 7))] for p in range(2)]
        tiled = _frame(t, poses, H, W, precision)
        assert t.last_tiled
        for k in LEAN:
            assert torch.equal(whole[k], torch.cat([s[k] for s in singles])), (precision, k)
            assert torch.equal(whole[k], torch.cat([x[k] for p in tiles for x in p])), (precision, k)
            assert torch.equal(whole[k], tiled[k]), (precision, k)
        ref = G.reference("fog7", "half", n_poses=2)
        assert float((whole["rgb"].cpu() - ref["rgb"]).abs().max(-1).values[ref["decided"]].max()) <= (1e-3 if precision == "f16x1" else 1e-4)
    finally:
        r.close(); t.close()


# ---- 6. executed evaluations ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("fog192", "half"), ("fog192", "checker"), ("fog7", "half")])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_executed_evaluations_lie_in_the_helpers_interval(name, kind, precision):
    ref = G.reference(name, kind)
    cfg, n_rays = G.scene(name)[2], G.scene(name)[4].shape[0]
    r = _scene_renderer(name, kind)
    try:
        for mode, group in _modes(precision):
            r.debug_set_decomposition(mode)
            _scene_frame(r, name, precision)
            ran, full = r.last_ray_evaluations()
            lo, hi = G.executed_interval(ref, group)
            print(f"{name} {kind} {precision} {group}: executed {ran} of {full}, helper [{lo}, {hi}]")
            assert full == G.full_evaluations(cfg, n_rays) and lo <= ran <= hi, (name, kind, precision, group)
    finally:
        r.close()


# ---- 7. build_occupancy ------------------------------------------------------------------------------------------------------

def _probe_points(lo, hi, res, probes):
    """The probe lattice of nwe_build_occupancy restated: [cells, probes^3, 3] float32."""
    cols = []
    for c in range(3):
        step = np.float32((float(hi[c]) - float(lo[c])) / res[c])
        j = (np.arange(probes, dtype=np.float32) + np.float32(0.5)) / np.float32(probes)
        f = np.arange(res[c], dtype=np.float32)[:, None] + j[None, :]
        cols.append(f * step + np.float32(lo[c]))               # [r, probes], every operation in fp32
    X, Y, Z = cols
    shape = (res[0], res[1], res[2], probes, probes, probes, 3)
    pts = np.empty(shape, np.float32)
    pts[..., 0] = X[:, None, None, :, None, None]
    pts[..., 1] = Y[None, :, None, None, :, None]
    pts[..., 2] = Z[None, None, :, None, None, :]
    return pts.reshape(res[0] * res[1] * res[2], probes ** 3, 3)


def _dilate(bits):
    out = np.zeros_like(bits)
    p = np.pad(bits, 1)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= p[dx:dx + bits.shape[0], dy:dy + bits.shape[1], dz:dz + bits.shape[2]]
    return out


@pytest.mark.parametrize("both", [False, True], ids=["one_network", "both_networks"])
@pytest.mark.parametrize("res,probes", [((5, 7, 9), 2), ((16, 16, 16), 1), ((5, 7, 9), 3), ((17, 31, 33), 4)])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_build_occupancy_equals_its_numpy_restatement(precision, res, probes, both):
    """query_points sigma at the same probe points, threshold, NaN -> occupied, dilation 0 / 1 / 2: exact, since a query row
    depends on its point alone.  The threshold is the median of the cells' largest sigma, so that both kinds of cell exist.
    17 x 31 x 33 at probes 4: 17 391 cells of 64 probes, which the build walks as one full chunk of 16 384 cells (2^20 points) and
    a ragged one of 1 007."""
    sd_c, sd_f, cfg = G.scene("fog192")[:3]
    sd_f = dict(sd_f)
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(1, sd_f)
        if both:
            r.set_network(0, nwe_amd.synthetic.dense_fog(nwe_amd.synthetic.make_state_dict(1000, 4, 128), 0.5, 3.0))
        lo, hi = (-3.0, -1.0, -2.0), (9.0, 11.0, 3.0)
        pts = torch.from_numpy(_probe_points(lo, hi, res, probes)).cuda()
        sig = [r.query_points(pts, None, which=w, precision=precision, outputs=("sigma",))["sigma"].cpu().numpy() for w in ((0, 1) if both else (1,))]
        # a cell is occupied by its largest probe over the networks, so it is the median of those maxima that halves the cells
        thr = float(np.median(np.max([x.reshape(pts.shape[0], -1).max(-1) for x in sig], axis=0)))
        occ = np.zeros(pts.shape[0], bool)
        for s in sig:
            occ |= ((s > np.float32(thr)) | ~np.isfinite(s)).any(-1)
        expect = occ.reshape(res)
        assert expect.any() and not expect.all()
        for dilate in (0, 1, 2):
            r.build_occupancy(lo, hi, res, probes=probes, threshold=thr, dilate=dilate, precision=precision)
            got = r.occupancy_bits()
            assert got.shape == tuple(res) and (got == expect).all(), (precision, res, probes, both, dilate, int((got != expect).sum()))
            assert r.occupancy["occupied_cells"] == int(expect.sum())
            expect = _dilate(expect)
        r.build_occupancy(lo, hi, res, probes=probes, threshold=float("inf"), dilate=2, precision=precision)
        assert r.occupancy["occupied_cells"] == 0
        r.build_occupancy(lo, hi, res, probes=probes, threshold=-float("inf"), dilate=0, precision=precision)
        assert r.occupancy["occupied"] == 1.0
    finally:
        r.close()


def test_build_occupancy_nan_is_occupied_and_its_refusals():
    sd = nwe_amd.synthetic.make_state_dict(1001, 4, 128)
    sd["_alpha_linear.bias"][:] = np.nan
    r = nwe_amd.Renderer(0)
    try:
        with pytest.raises(RuntimeError, match="no network is set"):
            r.build_occupancy((0, 0, 0), (1, 1, 1), 4)
        r.set_network(1, sd)
        r.build_occupancy((0, 0, 0), (1, 1, 1), (3, 4, 5), probes=1, threshold=1e30, dilate=0)
        assert r.occupancy["occupied"] == 1.0
        for kw, text in ((dict(probes=0), "probes"), (dict(probes=5), "probes"), (dict(dilate=-1), "dilate"), (dict(dilate=3), "dilate"),
                         (dict(threshold=float("nan")), "threshold")):
            with pytest.raises(ValueError, match=text):
                r.build_occupancy((0, 0, 0), (1, 1, 1), 4, **kw)
        with pytest.raises(ValueError, match="lo < hi"):
            r.build_occupancy((0, 0, 0), (1, 0, 1), 4)
        assert r.occupancy["resolution"] == (3, 4, 5)            # a refused build leaves the grid
        r.set_network(0, nwe_amd.synthetic.make_state_dict(5, 3, 64, skips=()))
        with pytest.raises(NotImplementedError, match="no MFMA kernel for this network shape"):
            r.build_occupancy((0, 0, 0), (1, 1, 1), 4)
        r.build_occupancy((0, 0, 0), (1, 1, 1), 4, precision="f32")
        assert r.occupancy["occupied"] == 1.0
    finally:
        r.close()


def test_handler_renders_with_a_built_grid_and_reports_the_refusals(monkeypatch):
    sd_c, sd_f, cfg, poses, rays, H, W = G.scene("fog192")
    monkeypatch.setenv("NWE_OCCUPANCY", "16,1,0")
    h = nwe_amd.NeRFReplicaInferenceHandler("office_geneve", "x.ckpt", occupancy={"lo": G.BOX_LO, "hi": G.BOX_HI, "threshold": 0.5})
    h.set_sampling(cfg.n_samples, cfg.n_importance)
    h.initialize_models((sd_c, sd_f))
    try:
        g = h.occupancy
        assert g["resolution"] == (16, 16, 16) and 0 < g["occupied"] < 1
        bits = h.renderer.occupancy_bits()
        out = h.render(poses[0].numpy(), H, W)
        ran, full = h.renderer.last_ray_evaluations()
        assert ran < full
        # the same frame from a plain renderer under the same bits
        r = _renderer(sd_c, sd_f, cfg)
        r.set_occupancy(bits, g["lo"], g["hi"], g["resolution"])
        fx, fy, cx, cy = nwe_amd.handler.pinhole_intrinsics(H, W)
        ref = r.render(poses.numpy(), H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=h._depth_close_bound, far=h._depth_far_bound)
        assert torch.equal(out["rgb"].reshape(-1, 3), ref["rgb"])
        r.close()
        with pytest.raises(NotImplementedError, match="nwe_set_occupancy"):
            h._render_rays(rays.cuda())
        with pytest.raises(NotImplementedError, match="only rgb / depth / acc / flags"):
            h.render(poses[0].numpy(), H, W, outputs=("rgb", "z_std"))
        h.clear_occupancy()
        assert h.occupancy is None
        h._render_rays(rays.cuda())
        h.build_occupancy(G.BOX_LO, G.BOX_HI, 8, probes=1, dilate=0)
        assert h.occupancy["resolution"] == (8, 8, 8)
    finally:
        h.renderer.close()
    with pytest.raises(ValueError, match="occupancy"):
        nwe_amd.NeRFReplicaInferenceHandler("office_geneve", "x.ckpt", occupancy={"lo": G.BOX_LO, "hi": G.BOX_HI}, early_termination=1e-2)
    with pytest.raises(ValueError, match="occupancy"):
        nwe_amd.NeRFReplicaInferenceHandler("office_geneve", "x.ckpt", occupancy={"lo": G.BOX_LO})


# ---- 8. every built shape ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vd", [True, False], ids=["folded", "novd"])
@pytest.mark.parametrize("D,W,skips", [(4, 128, ()), (6, 128, (4,)), (8, 128, (4,)), (4, 256, ()), (6, 256, (4,)), (8, 256, (4,))])
def test_every_built_shape_against_the_f32_kernel(D, W, skips, vd):
    """One small frame (7 x 19, 32 + 0: without importance samples every ray's cells are the f32 kernel's, so every ray is
    compared) under the half-space grid, both MFMA precisions and both decompositions against the f32 kernel at the parity
    tolerances, and the executed counts equal to the helper's.  The fog's spread is the one at which f16x1 meets its tolerance
    on every shape with no grid set (tests/occupancy.py: X1_SPREAD)."""
    S = nwe_amd.synthetic
    fog = S.thin_fog if vd else S.thin_fog_output
    sd_c = fog(S.make_state_dict(1001, D, W, skips=skips, use_view_dirs=vd), 0.5, G.X1_SPREAD)
    sd_f = sd_c
    cfg = O.RenderConfig(n_samples=32, n_importance=0)
    H, Wd = 7, 19
    poses, rays = G.E.frame_rays(H, Wd)
    g = G.grid("half")
    ref = G.masked_render(rays if vd else rays[:, :8].contiguous(), sd_c, sd_f, cfg, g)
    r = _renderer(sd_c, sd_f, cfg)
    try:
        _set(r, g)
        base = _frame(r, poses, H, Wd, "f32")
        for precision in ("f16x3", "f16x1"):
            tol = TOL_X1 if precision == "f16x1" else TOL
            first = None
            for mode, kind in _modes(precision):
                r.debug_set_decomposition(mode)
                out = _frame(r, poses, H, Wd, precision)
                for k in LEAN:
                    assert float((out[k] - base[k]).abs().max()) <= tol[k], (D, W, vd, precision, mode, k)
                lo, hi = G.executed_interval(ref, kind)
                assert lo <= r.last_ray_evaluations()[0] <= hi and hi < G.full_evaluations(cfg, 133)
                if first is None:
                    first = out
                else:
                    _same(out, first, (D, W, vd, precision))
    finally:
        r.close()


# ---- 9. sequences on one context ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_sequences_on_one_context_equal_fresh_contexts(precision):
    """grid -> clear -> grid, and set_network in between, equal fresh contexts; a refused call leaves nwe_last_kernel_ms
    describing the last launch."""
    sd_c, sd_f, cfg = G.scene("fog7")[:3]
    r = _scene_renderer("fog7", "half")
    fresh_half, fresh_plain, fresh_checker = _scene_renderer("fog7", "half"), _scene_renderer("fog7"), _scene_renderer("fog7", "checker")
    try:
        a = _scene_frame(r, "fog7", precision)
        _same(a, _scene_frame(fresh_half, "fog7", precision), "first")
        ms, evals = r.last_kernel_ms(), r.last_ray_evaluations()
        with pytest.raises(NotImplementedError, match="nwe_set_occupancy"):
            _scene_frame(r, "fog7", precision, outputs=("rgb", "z_fine"))
        with pytest.raises(NotImplementedError, match="nwe_set_occupancy"):
            r.render_rays(G.scene("fog7")[4].cuda(), precision=precision)
        r.set_early_termination(1e-2)
        with pytest.raises(NotImplementedError, match="early termination"):
            _scene_frame(r, "fog7", precision)
        r.set_early_termination(0.0)
        assert r.last_kernel_ms() == ms and r.last_ray_evaluations() == evals
        r.clear_occupancy()
        _same(_scene_frame(r, "fog7", precision), _scene_frame(fresh_plain, "fog7", precision), "cleared")
        assert r.last_ray_evaluations() == (G.full_evaluations(cfg, 133),) * 2
        _set(r, G.grid("checker"))
        _same(_scene_frame(r, "fog7", precision), _scene_frame(fresh_checker, "fog7", precision), "second grid")
        r.set_network(1, sd_f)                                   # clears the grid
        assert r.occupancy is None
        _same(_scene_frame(r, "fog7", precision), _scene_frame(fresh_plain, "fog7", precision), "set_network")
        _set(r, G.grid("half"))
        _same(_scene_frame(r, "fog7", precision), a, "grid again")
        # a query ignores the grid
        pts = torch.rand(64, 3).cuda()
        q = r.query_points(pts, None, precision=precision, outputs=("sigma",))["sigma"]
        assert torch.equal(q, fresh_plain.query_points(pts, None, precision=precision, outputs=("sigma",))["sigma"])
    finally:
        for x in (r, fresh_half, fresh_plain, fresh_checker):
            x.close()


# ---- 10. a NaN weight --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_nan_keeps_the_references_pattern_on_unmasked_samples_and_masked_samples_stay_finite(precision):
    """A NaN bias in the fine network's density head: every ray with an unmasked sample is NaN, with the flags; under a grid
    with no bit set every sample is masked and the frame is finite - the NaN colour under a zero weight does not leak."""
    sd_c, sd_f, cfg, poses, rays, H, W = G.scene("fog7")
    bad = {k: v.copy() for k, v in sd_f.items()}
    bad["_alpha_linear.bias"][:] = np.nan
    bad["_rgb_linear.bias"][:] = np.nan
    g = G.grid("half")
    ref = G.masked_render(rays, sd_c, bad, cfg, g)
    r = _renderer(sd_c, bad, cfg)
    try:
        _set(r, g)
        for mode, _ in _modes(precision):
            r.debug_set_decomposition(mode)
            out = _frame(r, poses, H, W, precision)
            for k in LEAN:
                assert (torch.isnan(out[k].cpu()) == torch.isnan(ref[k])).all(), (precision, mode, k)
            assert torch.isnan(ref["rgb"]).any()
            assert int(out["flags"].item()) & 7 == 7
        _set(r, G.grid("none"))
        out = _frame(r, poses, H, W, precision)
        assert all(torch.isfinite(out[k]).all() for k in LEAN) and int(out["flags"].item()) == DISP_BITS   # 0 / 0 disp, as above
    finally:
        r.close()
