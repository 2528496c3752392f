"""The baked coarse pass on the GPU (include/nwe.h: nwe_set_coarse_grid; the producer kernel: csrc/nwe_coarse_grid.hip).

The two halves of the rule are checked separately through nwe_coarse_grid_weights: the grid's sigma_raw per coarse sample against
the numpy restatement (tests/coarse_grid.py), bit for bit, and the weights against the render kernels' own compositing of that
sigma, bit for bit.  The frame is then the ordinary call fed those weights, bit for bit, in every precision, decomposition,
tiling and pose batch.  Parity with the oracle composed with the restated grid holds on every ray of the scene that
tests/test_coarse_grid_host.py vetted, at the project's parity tolerances (rgb 1e-4, depth 1e-4 * far, acc 1e-4; 1e-3 for
f16x1).  "Bit for bit" lets a NaN equal a NaN whatever its sign and payload: an inf - inf of the host and of the GPU differ there.
The last test bakes across the border of the bake's chunks of 2^20 cells; tests/test_gpu_grid_sizes.py bakes beyond 2^20 cells too,
beside the radiance bake and with the query run whole and split, and looks the grid up along an axis of 512 cells, which no grid
that is looked up here has. The same file covers the sparse frame's chunks beyond one scan tile and its default chunk.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd.handler import NeRFReplicaInferenceHandler
from oracle import nerf_oracle as O
from tests import coarse_grid as B

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
PRECISIONS = ("f16x3", "f16x1", "f32")
TOL = {"rgb": 1e-4, "depth": 1e-4 * B.FAR, "acc": 1e-4}           # tests/test_gpu_occupancy.py
TOL_X1 = {"rgb": 1e-3, "depth": 1e-3 * B.FAR, "acc": 1e-3}


def _renderer(sd_c, sd_f, cfg, devices=None):
    r = nwe_amd.TiledRenderer(devices) if devices else nwe_amd.Renderer(0)
    r.set_network(0, sd_c)
    if sd_f is not None:
        r.set_network(1, sd_f)
    r.set_sampling(cfg.n_samples, cfg.n_importance)
    return r


def _scene_renderer(name, kind=None, devices=None):
    sd_c, sd_f, cfg = B.scene(name)[:3]
    r = _renderer(sd_c, sd_f, cfg, devices)
    if kind is not None:
        _set(r, B.grid(kind))
    return r


def _set(r, g):
    r.set_coarse_grid(g["values"], g["lo"], g["hi"])


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=B.NEAR, far=B.FAR)


def _frame(r, poses, H, W, precision, rows=None, outputs=LEAN):
    return r.render(poses.numpy(), H, W, rows=rows, precision=precision, outputs=outputs, **_camera(H, W))


def _same(a, b, ctx):
    for k in LEAN:
        assert torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _modes(precision, n_samples):
    if precision == "f32":
        return (-1,)
    return (1,) if n_samples > 64 else (0, 1, 2)      # more than 64 coarse samples: the sample-split plan only


# ---- 1. interpolation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns", [("random", 7), ("small", 64), ("small_nonfinite", 96)])
def test_sigma_equals_the_numpy_restatement_bit_for_bit(kind, ns):
    """Random grid values of both signs; points inside the box, within half a cell of its faces and outside it (the small box
    ends inside the frame's depth range), and - the second and third pose - points with a NaN and with an infinite coordinate."""
    g = B.grid(kind)
    H, W = B.H2, B.W2
    poses, _ = B.G.E.frame_rays(H, W, 3)
    poses = poses.clone()
    poses[1, 0, 3] = float("nan")
    poses[2, 1, 3] = float("inf")
    r = nwe_amd.Renderer(0)
    try:
        r.set_sampling(ns, 0)           # no network: the producer needs none
        _set(r, g)
        rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W)).cpu().numpy()
        _, pts = B.coarse_points(rays, ns)
        want = B.grid_sigma(pts, g)
        out = r.coarse_grid_weights(poses.numpy(), H, W, **_camera(H, W))
        got = out["sigma"].cpu().numpy()
        assert got.shape == (3 * H * W, ns)
        assert B.same_bits(got, want)
        # the cases are there
        lo, hi, cell = g["lo"], g["hi"], (g["hi"] - g["lo"]) / np.array(g["res"], np.float32)
        first = pts[:H * W]
        inside = ((first >= lo) & (first <= hi)).all(-1)
        near_face = inside & (((first - lo) < 0.5 * cell) | ((hi - first) < 0.5 * cell)).any(-1)
        assert near_face.any() and (want[:H * W][inside] != 0).any()
        if kind != "random":
            assert (~inside).any() and (want[:H * W][~inside] == 0).all()
        assert not np.isfinite(pts[H * W:]).all(-1).any() and (want[H * W:] == 0).all()
        if kind == "small_nonfinite":
            assert np.isnan(want).any()
        # rows of a frame are the frame's rows; one output alone
        part = r.coarse_grid_weights(poses.numpy(), H, W, rows=(2, 7), outputs=("sigma",), **_camera(H, W))
        assert set(part) == {"sigma"}
        assert B.same_bits(part["sigma"].cpu().numpy(), got.reshape(3, H, W, ns)[:, 2:7].reshape(-1, ns))
    finally:
        r.close()


# ---- 2. weights -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("s7", "small"), ("s192", "random"), ("s128", "small"), ("novd", "random")])
def test_weights_are_the_render_kernels_compositing_of_the_grids_sigma(name, kind):
    """weights_out == weights_coarse of nwe_render_rays on nwe_create_rays' rays with raw_coarse = (0, 0, 0, sigma_out): both from
    the GPU, so no tolerance."""
    sd_c, sd_f, cfg, poses, _, H, W = B.scene(name)
    r = _scene_renderer(name)
    try:
        rays = r.create_rays(poses.numpy(), H, W, use_view_dirs=r.ray_columns == 11, **_camera(H, W))
        _set(r, B.grid(kind))
        out = r.coarse_grid_weights(poses.numpy(), H, W, **_camera(H, W))
        r.clear_coarse_grid()
        raw = torch.zeros(rays.shape[0], cfg.n_samples, 4, device=rays.device)
        raw[..., 3] = out["sigma"]
        for precision in ("f16x3", "f32"):
            ref = r.render_rays(rays, precision=precision, outputs=("weights_coarse",), debug_raw=(raw, None))
            assert torch.equal(out["weights"], ref["weights_coarse"]), (name, precision)
        assert float(out["weights"].max()) > 0.01 and (out["sigma"] < 0).any()
    finally:
        r.close()


# ---- 3. frame -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("s7", "small"), ("s192", "random"), ("s128", "random"), ("big7", "random"), ("novd", "small")])
def test_baked_frame_is_the_ordinary_call_fed_the_grids_weights(name, kind):
    """rgb / depth / acc of a baked nwe_render == nwe_render_rays on the same rays with nwe_debug_set_coarse_weights(weights_out),
    in all three precisions and under every decomposition; rows and the coarse flag bits as well."""
    sd_c, sd_f, cfg, poses, _, H, W = B.scene(name)
    r, plain = _scene_renderer(name, kind), _scene_renderer(name)
    try:
        rays = plain.create_rays(poses.numpy(), H, W, use_view_dirs=plain.ray_columns == 11, **_camera(H, W))
        weights = r.coarse_grid_weights(poses.numpy(), H, W, outputs=("weights",), **_camera(H, W))["weights"]
        for precision in PRECISIONS:
            ref = plain.render_rays(rays, precision=precision, outputs=LEAN, debug_coarse_weights=weights)
            for mode in _modes(precision, cfg.n_samples):
                r.debug_set_decomposition(mode)
                out = _frame(r, poses, H, W, precision)
                _same(out, ref, (name, precision, mode))
                assert int(out["flags"].item()) & 0xF0 == 0          # the coarse flag bits are never raised
                if precision != "f32":
                    assert r.debug_last_plan() == mode
            r.debug_set_decomposition(-1)
            whole = _frame(r, poses, H, W, precision)
            _same(whole, ref, (name, precision, "auto"))
            tiles = [_frame(r, poses, H, W, precision, rows=rows) for rows in ((0, 5), (5, 6), (6, H))]
            for k in LEAN:
                assert torch.equal(torch.cat([t[k] for t in tiles]), whole[k]), (name, precision, k, "row tiles")
        assert float(whole["acc"].max()) > 0.05
    finally:
        r.close(); plain.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pose_batches_and_tiled_renderer(precision):
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7", True)
    g = B.grid("small")
    r, tiled = _renderer(sd_c, sd_f, cfg), _renderer(sd_c, sd_f, cfg, [0, 0, 0])
    try:
        _set(r, g); _set(tiled, g)
        assert all(p.coarse_grid["resolution"] == g["res"] for p in tiled.parts)
        both = _frame(r, poses, H, W, precision)
        each = [_frame(r, poses[p:p + 1], H, W, precision) for p in range(2)]
        for k in LEAN:
            assert torch.equal(torch.cat([e[k] for e in each]), both[k]), (precision, k, "pose batch")
        out = _frame(tiled, poses, H, W, precision)
        assert tiled.last_tiled
        _same(out, both, (precision, "tiled"))
        tiled.clear_coarse_grid()
        assert all(p.coarse_grid is None for p in tiled.parts)
    finally:
        r.close(); tiled.close()


# ---- 4. constant fog ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s192", "s128", "novd"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_fog_baked_equals_the_frame_without_a_grid(name, precision):
    """A coarse network whose density head has zero weights and bias c: sigma_raw = c everywhere, the interpolation of equal values
    is exact and the k = 1 consumer is bit-identical to the fused kernel, so the baked frame is the ordinary frame."""
    sd_c, sd_f, cfg, poses, _, H, W = B.scene(name)
    c = np.float32(0.25)
    fog = {k: v.copy() for k, v in sd_c.items()}
    if "_alpha_linear.weight" in fog:
        fog["_alpha_linear.weight"][:] = 0.0
        fog["_alpha_linear.bias"][:] = c
    else:
        fog["_output_linear.weight"][3] = 0.0
        fog["_output_linear.bias"][3] = c
    r, plain = _renderer(fog, sd_f, cfg), _renderer(fog, sd_f, cfg)
    try:
        r.bake_coarse_grid(B.BOX_LO, B.BOX_HI, B.BOX_RES, precision=precision)
        assert (r.coarse_grid_values() == c).all()
        for mode in _modes(precision, cfg.n_samples):
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            a, b = _frame(r, poses, H, W, precision), _frame(plain, poses, H, W, precision)
            _same({**a, "flags": a["flags"] & 0x0F}, {**b, "flags": b["flags"] & 0x0F}, (name, precision, mode))
        assert float(a["acc"].max()) > 0.05
    finally:
        r.close(); plain.close()


# ---- 5. bake --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_bake_equals_the_density_grid_of_the_coarse_network(precision):
    """nwe_bake_coarse_grid == handler.density_grid(which="coarse"), bit for bit, under a 4x128 coarse / 8x256 fine pair - which
    then renders under the MFMA precisions without separate passes."""
    S = nwe_amd.synthetic
    sd_c = S.thin_fog(S.make_state_dict(1000, 4, 128), 0.3, 1.0)
    sd_f = S.dense_fog(S.make_state_dict(1001, 8, 256), 0.5, 1.0)
    lo, hi, res = B.SMALL_LO, B.SMALL_HI, (5, 7, 9)
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision=precision)
    h.set_sampling(7, 6)
    h.initialize_models(state_dicts=(sd_c, sd_f))
    r = h.renderer
    try:
        want = h.density_grid(lo, hi, res, which="coarse", precision=precision)
        h.bake_coarse_grid(lo, hi, res)
        g = h.coarse_grid
        assert g["resolution"] == res
        got = r.coarse_grid_values()
        assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32))
        assert float(np.std(got)) > 1e-3
        poses, _ = B.G.E.frame_rays(B.H2, B.W2)
        out = _frame(r, poses, B.H2, B.W2, precision)
        assert all(torch.isfinite(out[k]).all() for k in LEAN) and float(out["acc"].max()) > 0.05
        # the device-to-device path of nwe_set_coarse_grid: the same grid from the tensor density_grid returned
        r.set_coarse_grid(want, lo, hi)
        _same(_frame(r, poses, B.H2, B.W2, precision), out, "set from a device tensor")
        h.clear_coarse_grid()
        if precision != "f32":
            with pytest.raises(NotImplementedError, match="same shape"):
                _frame(r, poses, B.H2, B.W2, precision)
        # refusals of the bake, as nwe_build_occupancy's
        with pytest.raises(ValueError, match="lo < hi"):
            r.bake_coarse_grid((0, 0, 0), (1, 0, 1), 4)
        with pytest.raises(ValueError, match="1..512"):
            r.bake_coarse_grid((0, 0, 0), (1, 1, 1), 513)
        r.set_network(0, S.make_state_dict(5, 3, 64, skips=()))
        with pytest.raises(NotImplementedError, match="no MFMA kernel for this network shape"):
            r.bake_coarse_grid((0, 0, 0), (1, 1, 1), 4)
        r.bake_coarse_grid((0, 0, 0), (1, 1, 1), 4, precision="f32")
        assert r.coarse_grid["resolution"] == (4, 4, 4)
        # a coarse network of any shape under an MFMA fine network
        out = _frame(r, poses, B.H2, B.W2, precision)
        assert all(torch.isfinite(out[k]).all() for k in LEAN)
    finally:
        r.close()
    fresh = nwe_amd.Renderer(0)
    try:
        with pytest.raises(RuntimeError, match="coarse network is not set"):
            fresh.bake_coarse_grid((0, 0, 0), (1, 1, 1), 4)
    finally:
        fresh.close()


# ---- 6. parity ------------------------------------------------------------------------------------------------------------------

def test_parity_with_the_composed_oracle_on_every_ray():
    """z_vals -> grid sigma -> raw2outputs -> sample_pdf -> fine run_network -> raw2outputs, from the oracle's own functions
    (tests/coarse_grid.py); every ray, every precision, every decomposition."""
    name, kind = B.PARITY_SCENE, B.PARITY_GRID
    _, _, cfg, poses, _, H, W = B.scene(name)
    ref = B.parity_reference()
    r = _scene_renderer(name, kind)
    try:
        got = r.coarse_grid_weights(poses.numpy(), H, W, **_camera(H, W))
        assert B.same_bits(got["sigma"].cpu().numpy(), ref["sigma"].numpy())
        assert float((got["weights"].cpu() - ref["weights"]).abs().max()) < 1e-6
        for precision in PRECISIONS:
            tol = TOL_X1 if precision == "f16x1" else TOL
            for mode in _modes(precision, cfg.n_samples):
                r.debug_set_decomposition(mode)
                out = _frame(r, poses, H, W, precision)
                for k in LEAN:
                    err = float((out[k].cpu() - ref[k]).abs().max())
                    print(f"baked parity {precision} mode {mode} {k}: max err {err:.2e} (tol {tol[k]:.0e})")
                    assert err <= tol[k], (precision, mode, k)
    finally:
        r.close()


# ---- 7. reports -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_reports(precision):
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s192")
    n, ns, ni = H * W, cfg.n_samples, cfg.n_importance
    r, plain = _scene_renderer("s192", "random"), _scene_renderer("s192")
    try:
        _frame(r, poses, H, W, precision)
        assert r.last_ray_evaluations() == (n * (ns + ni), n * (2 * ns + ni))
        ms, rays = r.last_coarse_launch()
        assert rays == n and ms > 0
        parts = r.last_launch_parts()
        total = r.last_kernel_ms()
        assert sum(rays for _, rays in parts) == n
        assert abs(ms + sum(t for t, _ in parts) - total) <= 1e-3 + 1e-3 * total, (ms, parts, total)
        # the producer alone moves none of the render reports
        r.coarse_grid_weights(poses.numpy(), H, W, **_camera(H, W))
        assert r.last_kernel_ms() == total and r.last_coarse_launch() == (ms, rays)
        # n_importance == 0: a grid changes no bit and nothing is reported
        r.set_sampling(ns, 0); plain.set_sampling(ns, 0)
        _same(_frame(r, poses, H, W, precision), _frame(plain, poses, H, W, precision), (precision, "coarse only"))
        assert r.last_coarse_launch() is None and r.last_ray_evaluations() == (n * ns, n * ns)
        if precision != "f32":
            assert r.debug_last_plan() == plain.debug_last_plan()
    finally:
        r.close(); plain.close()


# ---- 8. refusals and a sequence -------------------------------------------------------------------------------------------------

def test_refusals_of_the_real_calls():
    sd_c, sd_f, cfg, poses, rays, H, W = B.scene("s7")
    r = _scene_renderer("s7", "random")
    try:
        base = _frame(r, poses, H, W, "f16x3")
        ms, evals = r.last_kernel_ms(), r.last_ray_evaluations()
        with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*only rgb / depth / acc / flags"):
            _frame(r, poses, H, W, "f16x3", outputs=("rgb", "z_fine"))
        with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*nwe_render_rays"):
            r.render_rays(rays.cuda())
        with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*nwe_render_rays"):
            r.render_rays(rays.cuda(), precision="f32", debug_coarse_weights=torch.ones(rays.shape[0], cfg.n_samples))
        for setter, on, off, text in ((r.set_early_termination, 1e-2, 0.0, "early termination"), (r.set_shared_coarse, 2, 1, "shared coarse pass"),
                                      (r.set_separate_passes, True, False, "separate passes")):
            setter(on)
            for precision in ("f16x3", "f32"):
                with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*not built together with.*" + text):
                    _frame(r, poses, H, W, precision)
            setter(off)
        r.set_occupancy(np.ones((2, 2, 2), bool), (0, 0, 0), (1, 1, 1), (2, 2, 2))
        with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*occupancy grid"):
            _frame(r, poses, H, W, "f16x3")
        r.clear_occupancy()
        assert r.last_kernel_ms() == ms and r.last_ray_evaluations() == evals      # a refused call moves no report
        _same(_frame(r, poses, H, W, "f16x3"), base, "after the refusals")
        # nwe_coarse_grid_weights: what it needs
        with pytest.raises(ValueError, match="far < near"):
            r.coarse_grid_weights(poses.numpy(), H, W, **dict(_camera(H, W), near=2.0, far=1.0))
        r.clear_coarse_grid()
        with pytest.raises(RuntimeError, match="no grid is set"):
            r.coarse_grid_weights(poses.numpy(), H, W, **_camera(H, W))
        # a query ignores the grid
        _set(r, B.grid("random"))
        pts = torch.rand(64, 3).cuda()
        plain = _scene_renderer("s7")
        assert torch.equal(r.query_points(pts, None, which=0, outputs=("sigma",))["sigma"], plain.query_points(pts, None, which=0, outputs=("sigma",))["sigma"])
        plain.close()
    finally:
        r.close()
    # a fine network packed unfolded: refused by name under the MFMA precisions, rendered by NWE_PREC_F32
    r = nwe_amd.Renderer(0)
    try:
        r.debug_set_fold(False)
        r.set_network(0, sd_c); r.set_network(1, sd_f); r.set_sampling(cfg.n_samples, cfg.n_importance)
        _set(r, B.grid("random"))
        with pytest.raises(NotImplementedError, match="nwe_set_coarse_grid.*packed unfolded"):
            _frame(r, poses, H, W, "f16x3")
        _frame(r, poses, H, W, "f32")
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_a_sequence_on_one_context(precision):
    """bake -> frame -> set fine network -> frame -> set coarse network (the grid is gone: the ordinary frame) -> clear."""
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7")
    r, plain = _scene_renderer("s7"), _scene_renderer("s7")
    try:
        ordinary = _frame(plain, poses, H, W, precision)
        r.bake_coarse_grid(B.BOX_LO, B.BOX_HI, (22, 18, 10), precision=precision)
        values = r.coarse_grid_values()
        a = _frame(r, poses, H, W, precision)
        assert r.last_coarse_launch() is not None
        for k in LEAN:                       # an approximation of the ordinary frame, and not the same frame
            assert float((a[k] - ordinary[k]).abs().max()) < 0.05 * (B.FAR if k == "depth" else 1.0)
        r.set_network(1, sd_f)
        assert np.array_equal(r.coarse_grid_values(), values)
        _same(_frame(r, poses, H, W, precision), a, "fine network set again")
        r.set_network(0, sd_c)
        assert r.coarse_grid is None
        _same(_frame(r, poses, H, W, precision), ordinary, "coarse network set: the grid is gone")
        assert r.last_coarse_launch() is None
        n = H * W
        assert r.last_ray_evaluations() == (n * (2 * cfg.n_samples + cfg.n_importance),) * 2
        r.set_coarse_grid(values, B.BOX_LO, B.BOX_HI)
        _same(_frame(r, poses, H, W, precision), a, "the same grid set from the host")
        r.clear_coarse_grid()
        _same(_frame(r, poses, H, W, precision), ordinary, "cleared")
    finally:
        r.close(); plain.close()


# ---- 9. the bake across a chunk boundary --------------------------------------------------------------------------------------
# Last in the file on purpose.  test_reports reads one pair of events twice and asks for the same float; the runtime converts GPU ticks
# to nanoseconds with a fit that it renews now and then, and a renewal between the two readings moves the answer by 1 ns.  With this
# test in front of test_reports that happened in 2 of 10 runs of the file (4 of 10 on the commit before this test existed, with the
# test added to it), with it here or left out in none of 10.

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bake_across_a_chunk_boundary(precision):
    """101 x 103 x 102 = 1 061 106 cells: the bake walks them as one full chunk of 2^20 cells and a ragged one of 12 530.  The grid is
    query_points' sigma at the cells' centres (the probes = 1 lattice of nwe_build_occupancy, restated in tests/test_gpu_occupancy.py),
    bit for bit, since a query row depends on its point alone."""
    from tests.test_gpu_occupancy import _probe_points
    S = nwe_amd.synthetic
    lo, hi, res = (-3.0, -1.0, -2.0), (9.0, 11.0, 3.0), (101, 103, 102)
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, S.dense_fog(S.make_state_dict(1000, 4, 128), 0.5, 3.0))
        pts = torch.from_numpy(_probe_points(lo, hi, res, 1)).cuda()
        want = r.query_points(pts, None, which=0, precision=precision, outputs=("sigma",))["sigma"].cpu().numpy().reshape(res)
        r.bake_coarse_grid(lo, hi, res, precision=precision)
        got = r.coarse_grid_values()
        assert got.shape == want.shape and float(np.std(want[np.isfinite(want)])) > 1e-3
        nan = np.isnan(got) & np.isnan(want)
        differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not differ.any(), (precision, int(differ.sum()), np.argwhere(differ)[:3].tolist())
    finally:
        r.close()
