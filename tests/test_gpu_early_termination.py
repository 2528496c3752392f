"""Early ray termination on the GPU (include/nwe.h: nwe_set_early_termination; the kernels' part: csrc/nwe_mfma_render.h).

The reference is the oracle's own output with the weights of samples whose transmittance is below eps set to 0
(tests/early_termination.py); the scenes are fogs dense enough to end rays, at frames of a few hundred rays.  Tolerances are
the project's parity tolerances (rgb 1e-4, depth 1e-4 * far, acc 1e-4) for rays whose every transmittance is further than
1e-3 relative from eps, and those plus eps (eps * far for depth) for the others, which may stop one sample apart.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import early_termination as E

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
EPS = 1e-2
TOL = {"rgb": 1e-4, "depth": 1e-4 * E.FAR, "acc": 1e-4}
# include/nwe.h: NWE_PREC_F16X1 is ~1e-3 absolute on rgb; the same relative error on the weights gives depth and acc
TOL_X1 = {"rgb": 1e-3, "depth": 1e-3 * E.FAR, "acc": 1e-3}
# iterations a workgroup may run past the one in which its last ray is masked (csrc/nwe_mfma_render.h, nwe_kernel_f32.hip)
LAG = {"packets": 1, "split": 1, "f32": 0}


def _renderer(name, eps=0.0, devices=None, **kw):
    sd_c, sd_f, cfg, _, _, _ = E.scene(name, **kw)
    r = nwe_amd.TiledRenderer(devices) if devices else nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    if cfg.n_importance > 0:
        r.set_network(1, sd_f)
    r.set_sampling(cfg.n_samples, cfg.n_importance)
    r.set_early_termination(eps)
    return r


def _frame(r, name, precision, rows=None, outputs=LEAN, **kw):
    H, W = kw.get("H") or E.SCENES[name][6], kw.get("W") or E.SCENES[name][7]
    poses = E.scene(name, **kw)[3]
    fx, fy, cx, cy = O.intrinsics(H, W)
    return r.render(poses.numpy(), H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=E.NEAR, far=E.FAR, rows=rows, precision=precision, outputs=outputs)


def _full(name, n_rays):
    cfg = E.scene(name)[2]
    return n_rays * (cfg.n_samples + (cfg.n_samples + cfg.n_importance if cfg.n_importance > 0 else 0))


def _same(a, b, ctx):
    for k in LEAN:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _check_against_masked(out, ref, eps, tol, ctx):
    """Decided rays within tol, undecided rays within tol + eps (eps * far for depth); prints each figure first."""
    decided = ref["decided"].numpy()
    mx = lambda e: float(e.max()) if e.size else 0.0
    for k in LEAN:
        err = np.abs(out[k].cpu().numpy() - ref[k].numpy())
        err = err.max(-1) if err.ndim == 2 else err
        wide = tol[k] + eps * (E.FAR if k == "depth" else 1.0)
        print(f"{ctx} {k}: max err decided {mx(err[decided]):.2e} (tol {tol[k]:.0e}), undecided {mx(err[~decided]):.2e} of "
              f"{int((~decided).sum())} rays (tol {wide:.1e})")
        assert mx(err[decided]) <= tol[k], (ctx, k)
        assert mx(err[~decided]) <= wide, (ctx, k)


# ---- 1. off is off ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_back_to_zero_is_a_fresh_context(precision):
    """A context that had eps > 0 and went back to 0 renders the bits of a context that never had it, and reports the full
    evaluation count."""
    r, fresh = _renderer("allstop", EPS), _renderer("allstop")
    try:
        on = _frame(r, "allstop", precision)
        assert r.last_ray_evaluations()[0] < _full("allstop", 133)
        r.set_early_termination(0.0)
        assert r.early_termination == 0.0
        off, ref = _frame(r, "allstop", precision), _frame(fresh, "allstop", precision)
        _same(off, ref, precision)
        assert not torch.equal(on["rgb"], off["rgb"])
        assert r.last_ray_evaluations() == fresh.last_ray_evaluations() == (_full("allstop", 133),) * 2
    finally:
        r.close(); fresh.close()


@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_terminating_kernel_gives_the_plain_bits_where_nothing_gets_that_low(precision):
    """Thin fog (sigma 0.08): no ray's transmittance reaches 1e-4 (tests/test_early_termination_host.py), so the terminating
    kernels mask nothing, run every iteration and must give the bits of the plain ones - both decompositions."""
    r, plain = _renderer("thin", 1e-4), _renderer("thin")
    try:
        for mode in ((0, 1) if precision != "f32" else (-1,)):
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            _same(_frame(r, "thin", precision), _frame(plain, "thin", precision), (precision, mode))
            assert r.last_ray_evaluations() == (_full("thin", 133),) * 2
    finally:
        r.close(); plain.close()


# ---- 2. / 3. parity with the masked oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "allstop", "coarse_only", "ragged_samples"])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_parity_with_the_masked_oracle(name, precision):
    """eps = 1e-2.  That the masked reference is far from the unmasked one on these scenes (so that a renderer which ignored
    eps fails here) and that at most 5 % of the rays are undecided is checked in tests/test_early_termination_host.py."""
    ref = E.masked_reference(name, EPS)
    assert float((~ref["decided"]).float().mean()) <= 0.05
    r = _renderer(name, EPS)
    try:
        out = _frame(r, name, precision)
        assert int(out["flags"].item()) & 0x7 == 0      # rgb / depth / acc finite (a ray without density has a NaN disparity)
        _check_against_masked(out, ref, EPS, TOL, (name, precision))
    finally:
        r.close()


@pytest.mark.parametrize("name", ["mixed", "allstop", "coarse_only"])
def test_single_product_precision_within_its_tolerance_plus_eps(name):
    """f16x1: within its documented tolerance plus eps of the masked oracle, and - the bound that holds by construction in
    every precision - within eps (eps * far) of its own unterminated frame."""
    ref = E.masked_reference(name, EPS)
    r = _renderer(name, EPS)
    try:
        out = _frame(r, name, "f16x1")
        r.set_early_termination(0.0)
        plain = _frame(r, name, "f16x1")
        for k in LEAN:
            wide = EPS * (E.FAR if k == "depth" else 1.0)
            err = float((out[k].cpu() - ref[k]).abs().max())
            own = float((out[k] - plain[k]).abs().max())
            print(f"{name} f16x1 {k}: vs masked oracle {err:.2e} (tol {TOL_X1[k] + wide:.1e}), vs its own unterminated frame {own:.2e} (bound {wide:.0e})")
            assert err <= TOL_X1[k] + wide, (name, k)
            assert own <= wide + 1e-6 * (E.FAR if k == "depth" else 1.0), (name, k)
    finally:
        r.close()


# ---- 4. bit-identity under termination -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "ragged_samples", "coarse_only"])
@pytest.mark.parametrize("precision", ["f16x3", "f16x1"])
def test_decompositions_agree_bit_for_bit(name, precision):
    """Packets, sample split and the hybrid plan: the same outputs, whichever rays share a workgroup and however late it leaves."""
    r = _renderer(name, EPS)
    try:
        res = {}
        for mode in (0, 1, 2):
            r.debug_set_decomposition(mode)
            res[mode] = _frame(r, name, precision)
            assert r.debug_last_plan() == mode
        _same(res[0], res[1], (name, precision, "0 vs 1"))
        _same(res[0], res[2], (name, precision, "0 vs 2"))
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_row_tiles_pose_batches_and_context_tiles_equal_the_frame(precision):
    """The rule is per ray: rows rendered apart, poses rendered apart and the tiles of TiledRenderer([0, 0, 0]) give the bits of
    the one launch, although every one of them groups the rays differently."""
    name, kw = "mixed", dict(H=9, W=20, n_poses=2)
    r, tiled = _renderer(name, EPS, **kw), _renderer(name, EPS, devices=[0, 0, 0], **kw)
    try:
        whole = _frame(r, name, precision, **kw)
        n = 9 * 20
        parts = [_frame(r, name, precision, rows=rows, **kw) for rows in ((0, 4), (4, 5), (5, 9))]
        for k in LEAN:
            w = whole[k].reshape((2, 9, 20) + tuple(whole[k].shape[1:]))
            rows = torch.cat([p[k].reshape((2, -1, 20) + tuple(p[k].shape[1:])) for p in parts], 1)
            assert torch.equal(w, rows), (precision, k, "row tiles")
        poses = E.scene(name, **kw)[3]
        fx, fy, cx, cy = O.intrinsics(9, 20)
        for p in range(2):
            one = r.render(poses[p].numpy(), 9, 20, fx=fx, fy=fy, cx=cx, cy=cy, near=E.NEAR, far=E.FAR, precision=precision, outputs=LEAN)
            for k in LEAN:
                assert torch.equal(one[k], whole[k][p * n:(p + 1) * n]), (precision, k, "pose", p)
        t = _frame(tiled, name, precision, **kw)
        assert tiled.last_tiled and all(p.early_termination == np.float32(EPS) for p in tiled.parts)
        _same(t, whole, (precision, "context tiles"))
    finally:
        r.close(); tiled.close()


# ---- 5. the counter --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "allstop", "coarse_only", "ragged_samples"])
def test_executed_evaluations_lie_in_the_interval_the_stop_indices_give(name):
    """Packets (groups of 128 rays, one sample per iteration), sample split (groups of 32, four samples per iteration) and the
    fp32 kernel (groups of 16, one sample, no lag): executed = per group its rays x (the coarse pass in full + the samples up
    to the group's largest stop index, in whole iterations, plus at most the documented lag).  Where every ray stops,
    executed < full."""
    cfg = E.scene(name)[2]
    ref = E.masked_reference(name, EPS)
    S = ref["trans"].shape[1]
    coarse = cfg.n_samples if cfg.n_importance > 0 else 0
    n_rays = len(ref["stop"])
    r = _renderer(name, EPS)
    try:
        # the fp32-grade precisions: their transmittance agrees with the oracle's well inside the margin that makes a ray decided
        for plan, precision, mode, group, per_it in (("packets", "f16x3", 0, 128, 1), ("split", "f16x3", 1, 32, 4), ("f32", "f32", -1, 16, 1)):
            if plan == "packets" and cfg.n_samples > 64:
                continue
            r.debug_set_decomposition(mode)
            _frame(r, name, precision)
            ran, full = r.last_ray_evaluations()
            lo, hi = E.executed_interval(ref["stop"], ref["decided"], group, per_it, LAG[plan], S, coarse)
            print(f"{name} {plan} {precision}: executed {ran} of {full}, interval [{lo}, {hi}]")
            assert full == _full(name, n_rays) and lo <= ran <= hi, (name, plan, precision)
            if name in ("allstop", "ragged_samples"):
                assert ran < full
            assert r.last_ray_evaluations() == (ran, full)
    finally:
        r.close()


# ---- 6. shapes that can break it ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (4, 8), (7, 19)])
@pytest.mark.parametrize("name", ["allstop", "ragged_samples", "coarse_only"])
def test_small_and_ragged_frames(name, H, W):
    """1 ray, 32 rays (one packet exactly) and 133 rays (a full 128-ray group plus a ragged packet) in every precision and
    decomposition against the masked oracle; 7 + 6 samples leave the sample-split plan's last iteration ragged."""
    kw = dict(H=H, W=W)
    ref = E.masked_reference(name, EPS, **kw)
    r = _renderer(name, EPS, **kw)
    try:
        first = None
        for precision, mode in (("f16x3", 0), ("f16x3", 1), ("f32", -1)):
            r.debug_set_decomposition(mode)
            out = _frame(r, name, precision, **kw)
            _check_against_masked(out, ref, EPS, TOL, (name, H, W, precision, mode))
            ran, full = r.last_ray_evaluations()
            assert 0 < ran <= full == _full(name, H * W)
            if precision == "f16x3":
                first = first or out
                _same(first, out, (name, H, W, mode))
    finally:
        r.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_every_other_call_is_refused_by_name_and_leaves_the_last_launch_alone():
    name = "allstop"
    r = _renderer(name, EPS)
    sd_c, sd_f, cfg, poses, rays, _ = E.scene(name)
    try:
        good = _frame(r, name, "f16x3")
        ms, parts, evals = r.last_kernel_ms(), r.last_launch_parts(), r.last_ray_evaluations()
        dev_rays = rays.cuda()

        def refused(call):
            with pytest.raises(NotImplementedError, match="min_transmittance"):
                call()
            assert (r.last_kernel_ms(), r.last_launch_parts(), r.last_ray_evaluations()) == (ms, parts, evals)

        for extra in ("disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "raw_fine", "raw_coarse", "z_fine", "weights_coarse",
                      "sample_cond"):
            for precision in ("f16x3", "f32"):
                refused(lambda: _frame(r, name, precision, outputs=LEAN + (extra,)))
        refused(lambda: _frame(r, name, "f32", outputs=LEAN + ("feat_map",)))
        for precision in ("f16x3", "f16x1", "f32"):
            refused(lambda: r.render_rays(dev_rays, precision=precision))
        S = cfg.n_samples + cfg.n_importance
        refused(lambda: r.render_rays(dev_rays, debug_fine_depths=torch.zeros(len(rays), S)))
        refused(lambda: r.render_rays(dev_rays, debug_raw=(None, torch.zeros(len(rays), S, 4))))
        refused(lambda: r.render_rays(dev_rays, debug_coarse_weights=torch.zeros(len(rays), cfg.n_samples)))
        refused(lambda: r.render_rays(dev_rays, train={"t_rand": torch.rand(len(rays), cfg.n_samples)}))
        # the refusals that exist without it come first and keep their text
        with pytest.raises(NotImplementedError, match="feat_map .* NWE_PREC_F32 kernel only"):
            _frame(r, name, "f16x3", outputs=LEAN + ("feat_map",))
        # the next legal render is unaffected (and no hook stayed armed)
        _same(_frame(r, name, "f16x3"), good, "after the refusals")
        r.set_early_termination(0.0)
        assert "rgb" in r.render_rays(dev_rays, outputs=LEAN + ("z_fine",))
    finally:
        r.close()


def test_unfolded_networks_and_unbuilt_shapes_are_refused_under_the_mfma_precisions():
    """nwe_debug_set_fold(0) packs the reference formulation, a comparison path that has no terminating kernel: refused by
    name under f16x3 / f16x1, rendered by the fp32 kernel, and rendered again once eps is back to 0."""
    name = "allstop"
    sd_c, sd_f, cfg, _, _, _ = E.scene(name)
    r = nwe_amd.Renderer(0)
    try:
        r.debug_set_fold(False)
        r.set_network(0, sd_c); r.set_network(1, sd_f)
        r.set_sampling(cfg.n_samples, cfg.n_importance)
        plain = _frame(r, name, "f16x3")
        ms = r.last_kernel_ms()
        r.set_early_termination(EPS)
        for precision in ("f16x3", "f16x1"):
            with pytest.raises(NotImplementedError, match=r"min_transmittance.*nwe_debug_set_fold\(0\)"):
                _frame(r, name, precision)
            assert r.last_kernel_ms() == ms
        _check_against_masked(_frame(r, name, "f32"), E.masked_reference(name, EPS), EPS, TOL, "unfolded f32")
        r.set_early_termination(0.0)
        _same(_frame(r, name, "f16x3"), plain, "unfolded, eps back to 0")
    finally:
        r.close()


# ---- 8. white background, NaN, the handler ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_white_background_uses_the_masked_acc(precision):
    ref = E.masked_reference("allstop", EPS, white_bkgd=True)
    r = _renderer("allstop", EPS)
    try:
        r.set_white_background(True)
        out = _frame(r, "allstop", precision)
        _check_against_masked(out, ref, EPS, TOL, ("white", precision))
        assert float((out["rgb"].cpu() - E.masked_reference("allstop", EPS)["rgb"]).abs().max()) > 1e-3   # the background shows
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_nan_weight_keeps_the_nan_pattern_and_flags(precision):
    """A NaN in the fine network's density head: every transmittance behind the first sample is NaN, which is not below eps, so
    the frame has the NaN pattern and the flags it has with eps = 0 - and every iteration runs."""
    sd_c, sd_f, cfg, _, _, _ = E.scene("allstop")
    bad = {k: v.copy() for k, v in sd_f.items()}
    bad["_alpha_linear.bias"] = np.full_like(bad["_alpha_linear.bias"], np.nan)
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, sd_c); r.set_network(1, bad)
        r.set_sampling(cfg.n_samples, cfg.n_importance)
        plain = _frame(r, "allstop", precision)
        r.set_early_termination(EPS)
        for mode in ((0, 1) if precision != "f32" else (-1,)):
            r.debug_set_decomposition(mode)
            out = _frame(r, "allstop", precision)
            for k in LEAN:
                assert torch.equal(torch.isnan(out[k]), torch.isnan(plain[k])), (precision, mode, k)
            assert torch.isnan(out["acc"]).all()
            assert int(out["flags"].item()) == int(plain["flags"].item()) != 0
            assert r.last_ray_evaluations() == (_full("allstop", 133),) * 2
    finally:
        r.close()


def test_handler_applies_the_setting_and_raises_what_the_abi_says(monkeypatch):
    sd_c, sd_f, cfg, _, rays, _ = E.scene("allstop")
    monkeypatch.setenv("NWE_EARLY_TERMINATION", str(EPS))
    h = nwe_amd.NeRFReplicaInferenceHandler("office_geneve", "unused.ckpt")
    h.set_sampling(cfg.n_samples, cfg.n_importance)
    h.initialize_models((sd_c, sd_f))
    try:
        assert h.renderer.early_termination == np.float32(EPS)
        pose = E.scene("allstop")[3][0].numpy()
        out = h.render(pose, 7, 19)
        ran, full = h.renderer.last_ray_evaluations()
        assert ran < full and torch.isfinite(out["rgb"]).all()
        with pytest.raises(NotImplementedError, match="min_transmittance"):
            h._render_rays(rays.cuda())
    finally:
        h.renderer.close()
