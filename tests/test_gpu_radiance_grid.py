"""The radiance grid on the GPU (include/nwe.h: nwe_render_grid; the kernel: csrc/nwe_radiance_grid.hip).

The steps of the rule are checked one by one through the call's diagnostics: the interpolated rows against the numpy restatement
(tests/radiance_grid.py), bit for bit; the coarse weights against the baked coarse pass's producer on the sigma channel, bit for
bit; the frame against the ordinary machinery (nwe_render_rays under f32) fed the call's own weights and rows, bit for bit.  Row
tiles, pose batches and streams give the whole call's bits.  Parity with the oracle composed with the restated grid holds on every
ray of the scene that tests/test_radiance_grid_host.py vetted, at the project's parity tolerances (rgb 1e-4, depth 1e-4 * far,
acc 1e-4).  "Bit for bit" lets a NaN equal a NaN whatever its sign and payload: an inf - inf of the host and of the GPU differ there.
The grids here are small: 13 824 cells at the most.  A bake beyond 2^20 cells - nwe_bake_radiance_grid walks the
cells in chunks of that many - and the lookup along an axis of 512 cells are covered by tests/test_gpu_grid_sizes.py, which also
covers the sparse frame's chunks beyond one scan tile and its default chunk.
"""
import math

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from nwe_amd.handler import NeRFReplicaInferenceHandler
from oracle import nerf_oracle as O
from tests import coarse_grid as B
from tests import radiance_grid as R

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
DIAG = ("weights_coarse", "z_fine", "raw_fine")
TOL = {"rgb": 1e-4, "depth": 1e-4 * R.FAR, "acc": 1e-4}           # tests/test_gpu_occupancy.py


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=R.NEAR, far=R.FAR)


def _set(r, g):
    r.set_radiance_grid(g["values"], g["lo"], g["hi"])


def _grid_renderer(kind, ns, ni):
    """No network: a grid frame needs none."""
    r = nwe_amd.Renderer(0)
    r.set_sampling(ns, ni)
    _set(r, R.grid(kind))
    return r


def _frame(r, poses, H, W, rows=None, outputs=LEAN):
    return r.render_grid(poses.numpy(), H, W, rows=rows, outputs=outputs, **_camera(H, W))


def _eq(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _same(a, b, ctx, keys=LEAN):
    for k in keys:
        assert _eq(a[k], b[k]), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


# ---- 1. interpolation -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns", [("random", 7), ("small_nonfinite", 96), ("smooth", 2), ("one", 7), ("flat", 2)])
def test_rows_equal_the_numpy_restatement_bit_for_bit(kind, ns):
    """n_importance = 0: the only pass walks the coarse depths, and raw_fine holds the row of every one of them.  Points inside the
    box, within half a cell of its faces and outside it, and - the second and third pose - with a NaN and an infinite coordinate."""
    g = R.grid(kind)
    H, W = R.H2, R.W2
    poses, _ = B.G.E.frame_rays(H, W, 3)
    poses = poses.clone()
    poses[1, 0, 3] = float("nan")
    poses[2, 1, 3] = float("inf")
    r = _grid_renderer(kind, ns, 0)
    try:
        rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W)).cpu().numpy()
        z, pts = R.coarse_points(rays, ns)
        want = R.grid_rows(pts, g)
        out = _frame(r, poses, H, W, outputs=("raw_fine", "z_fine"))
        got = out["raw_fine"].cpu().numpy()
        assert got.shape == (3 * H * W, ns, 4)
        assert R.same_bits(got, want)
        assert R.same_bits(out["z_fine"].cpu().numpy(), z)
        # the bits say what the composite holds, whichever outputs were asked for: the NaN of the grid reaches the colour alone
        assert int(out["flags"].item()) == (1 if kind == "small_nonfinite" else 0)
        # the cases are there
        first = pts[:H * W]
        inside = ((first >= g["lo"]) & (first <= g["hi"])).all(-1)
        assert inside.any() and (want[:H * W][inside] != 0).any()
        if kind in ("small_nonfinite", "one"):
            assert (~inside).any() and (want[:H * W][~inside] == 0).all()
        assert not np.isfinite(pts[H * W:]).all(-1).any() and (want[H * W:] == 0).all()
        if kind == "small_nonfinite":
            nan = np.isnan(want)
            assert nan[..., 0].any() and not nan[..., 1].any()      # the NaN stays in its channel
        # rows of a frame are the frame's rows
        part = _frame(r, poses, H, W, rows=(2, 7), outputs=("raw_fine",))
        assert R.same_bits(part["raw_fine"].cpu().numpy(), got.reshape(3, H, W, ns, 4)[:, 2:7].reshape(-1, ns, 4))
    finally:
        r.close()


# ---- 2. coarse weights ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("random", 7, 6), ("small_nonfinite", 64, 128), ("smooth", 96, 0), ("flat", 3, 1)])
def test_coarse_weights_are_the_baked_coarse_producers(kind, ns, ni):
    """weights_coarse == nwe_coarse_grid_weights for a coarse grid holding the sigma channel over the same box: colours do not enter
    a weight."""
    g = R.grid(kind)
    r = _grid_renderer(kind, ns, ni)
    try:
        r.set_coarse_grid(np.ascontiguousarray(g["values"][..., 3]), g["lo"], g["hi"])
        poses = R.scene("s7")[1]
        got = _frame(r, poses, R.H, R.W, outputs=("weights_coarse",))["weights_coarse"]
        ref = r.coarse_grid_weights(poses.numpy(), R.H, R.W, outputs=("weights",), **_camera(R.H, R.W))["weights"]
        assert tuple(got.shape) == (R.H * R.W, ns) and _eq(got, ref)
        assert float(torch.nan_to_num(got).max()) > 0.01
    finally:
        r.close()


# ---- 3. the frame ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kind,ns,ni,hw", [("random", 3, 1, None), ("small_nonfinite", 7, 6, None), ("random", 64, 128, None),
                                           ("smooth", 128, 256, (4, 4))])
def test_the_frame_is_the_ordinary_machinery_fed_the_grid(kind, ns, ni, hw, white):
    """nwe_render_rays under f32 on nwe_create_rays' rays, armed with the call's weights_coarse (nwe_debug_set_coarse_weights) and
    raw_fine (nwe_debug_set_raw), returns the call's z_fine, rgb, depth and acc: both run the same Composite and FineSampler code."""
    sd_c, sd_f = B.scene("s7")[:2]                            # any network: the hooks stand where it would run
    H, W = hw or (R.H, R.W)
    poses, _ = B.G.E.frame_rays(H, W, 1)
    r, plain = _grid_renderer(kind, ns, ni), nwe_amd.Renderer(0)
    try:
        plain.set_network(0, sd_c); plain.set_network(1, sd_f)
        plain.set_sampling(ns, ni)
        r.set_white_background(white); plain.set_white_background(white)
        out = _frame(r, poses, H, W, outputs=LEAN + DIAG)
        assert tuple(out["z_fine"].shape) == (H * W, ns + ni) and tuple(out["raw_fine"].shape) == (H * W, ns + ni, 4)
        rays = plain.create_rays(poses.numpy(), H, W, **_camera(H, W))
        ref = plain.render_rays(rays, precision="f32", outputs=LEAN + ("z_fine",), debug_coarse_weights=out["weights_coarse"],
                                debug_raw=(None, out["raw_fine"]))
        for k in LEAN + ("z_fine",):
            assert _eq(out[k], ref[k]), (kind, ns, ni, white, k)
        assert int(out["flags"].item()) == int(ref["flags"].item()) & 0x7     # the rgb / depth / acc bits, and no other
        if kind != "small_nonfinite":
            assert int(out["flags"].item()) == 0 and float(out["acc"].max()) > 0.05
            assert bool((out["z_fine"][:, 1:] >= out["z_fine"][:, :-1]).all())
        else:
            assert int(out["flags"].item()) != 0 and bool(torch.isfinite(out["rgb"]).any())
    finally:
        r.close(); plain.close()


# ---- 4. tiling ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("random", 7, 6), ("small_nonfinite", 64, 32)])
def test_row_tiles_pose_batches_and_streams_give_the_whole_calls_bits(kind, ns, ni):
    keys = LEAN + DIAG
    r = _grid_renderer(kind, ns, ni)
    try:
        poses = R.scene("s7")[1]
        H, W = R.H, R.W
        whole = _frame(r, poses, H, W, outputs=keys)
        tiles = [_frame(r, poses, H, W, rows=rows, outputs=keys) for rows in ((0, 5), (5, 6), (6, H))]
        for k in keys:
            assert _eq(torch.cat([t[k] for t in tiles]), whole[k]), (k, "row tiles")
        flags = 0
        for t in tiles:
            flags |= int(t["flags"].item())
        assert flags == int(whole["flags"].item())
        empty = _frame(r, poses, H, W, rows=(5, 5))
        assert tuple(empty["rgb"].shape) == (0, 3) and int(empty["flags"].item()) == 0
        poses2 = R.scene("s7", True)[1]
        both = _frame(r, poses2, R.H2, R.W2, outputs=keys)
        each = [_frame(r, poses2[p:p + 1], R.H2, R.W2, outputs=keys) for p in range(2)]
        for k in keys:
            assert _eq(torch.cat([e[k] for e in each]), both[k]), (k, "pose batch")
        # two streams back to back: a slot of the ring each, a pose table each
        streams = [torch.cuda.Stream(device=r.device) for _ in range(2)]
        outs = []
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(_frame(r, poses, H, W, outputs=keys))
        for s in streams:
            s.synchronize()
        for o in outs:
            _same(o, whole, "streams", keys)
    finally:
        r.close()


# ---- 5. parity ------------------------------------------------------------------------------------------------------------------

def test_parity_with_the_composed_oracle_on_every_ray():
    cfg, poses, _, H, W = R.scene(R.PARITY_SCENE)
    ref = R.parity_reference()
    r = _grid_renderer(R.PARITY_GRID, cfg.n_samples, cfg.n_importance)
    try:
        out = _frame(r, poses, H, W)
        for k in LEAN:
            err = (out[k].cpu() - ref[k]).abs()
            print(f"radiance grid parity {k}: {float(err.max()):.2e} (tol {TOL[k]:.0e})")
            assert float(err.max()) <= TOL[k], k
        assert int(out["flags"].item()) == 0
    finally:
        r.close()


# ---- 6. the bake ----------------------------------------------------------------------------------------------------------------

def _handler(precision, sds, ns=7, ni=6):
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision=precision)
    h.set_sampling(ns, ni)
    h.initialize_models(state_dicts=sds)
    return h


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bake_stores_run_network_at_the_cell_centres(precision):
    S = nwe_amd.synthetic
    sd_c = S.thin_fog(S.make_state_dict(1000, 4, 128), 0.3, 1.0)
    sd_f = S.dense_fog(S.make_state_dict(1001, 4, 128), 0.5, 1.0)
    lo, hi, res = R.SMALL_LO, R.SMALL_HI, (5, 7, 9)
    h = _handler(precision, (sd_c, sd_f))
    r = h.renderer
    try:
        centres = h.grid_centres(lo, hi, res, device=r.device)[None]
        for which, d in (("fine", (0.6, 0.0, -0.8)), ("coarse", (0.0, 2.0, 0.0))):      # used as given, not normalised
            want = h.run_network(centres, torch.tensor([d], device=r.device), which=which, precision=precision)[0]
            h.bake_radiance_grid(lo, hi, res, which=which, view_dir=d)
            assert h.radiance_grid["resolution"] == res
            got = r.radiance_grid_values()
            assert got.shape == res + (4,) and np.array_equal(got.reshape(-1, 4).view(np.uint32), want.cpu().numpy().view(np.uint32))
            assert float(np.std(got[..., 3])) > 1e-3 and float(np.std(got[..., :3])) > 1e-3
        # the six-direction default: its own torch restatement
        h.bake_radiance_grid(lo, hi, res, chunk=100)
        acc = None
        for d in h._AXIS_DIRECTIONS:
            row = h.run_network(centres, torch.tensor([d], device=r.device), precision=precision)[0]
            acc = row if acc is None else acc + row
        want6 = (acc / 6.0).cpu().numpy()
        got = r.radiance_grid_values().reshape(-1, 4)
        assert np.array_equal(got.view(np.uint32), want6.view(np.uint32))
        one = h.run_network(centres, torch.tensor([[1., 0., 0.]], device=r.device), precision=precision)[0].cpu().numpy()
        assert np.abs(got[:, 3] - one[:, 3]).max() <= 1e-6 * np.abs(one[:, 3]).max()    # sigma_raw does not depend on the direction
        # the device-to-device path of nwe_set_radiance_grid rendered a frame; so does the bake's own buffer
        poses, _ = B.G.E.frame_rays(R.H2, R.W2)
        out = h.render_grid(poses[0].numpy(), R.H2, R.W2)
        assert tuple(out["rgb"].shape) == (R.H2, R.W2, 3) and all(bool(torch.isfinite(out[k]).all()) for k in LEAN)
        # refusals of the bake that need a device context
        with pytest.raises(ValueError, match="lo < hi"):
            r.bake_radiance_grid((0, 0, 0), (1, 0, 1), 4, view_dir=(0, 0, 1))
        with pytest.raises(ValueError, match="1..512"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 513, view_dir=(0, 0, 1))
        with pytest.raises(ValueError, match="which must be 0 or 1"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, which=2, view_dir=(0, 0, 1))
        with pytest.raises(ValueError, match="need dir3_host"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4)
        assert r.radiance_grid["resolution"] == res          # a refused bake leaves the grid
        r.set_network(0, S.make_state_dict(5, 3, 64, skips=()))
        assert r.radiance_grid is None                       # an upload of either network clears it
        with pytest.raises(NotImplementedError, match="no MFMA kernel for this network shape"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, which=0, view_dir=(0, 0, 1))
        r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, which=0, view_dir=(0, 0, 1), precision="f32")
        assert r.radiance_grid["resolution"] == (4, 4, 4)
    finally:
        r.close()
    fresh = nwe_amd.Renderer(0)
    try:
        with pytest.raises(RuntimeError, match="fine network is not set"):
            fresh.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, view_dir=(0, 0, 1))
    finally:
        fresh.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bake_of_a_network_without_view_directions(precision):
    sd_c, sd_f, cfg = B.scene("novd")[:3]
    lo, hi, res = R.SMALL_LO, R.SMALL_HI, (4, 3, 6)
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, sd_c); r.set_network(1, sd_f)
        r.set_sampling(cfg.n_samples, cfg.n_importance)
        centres = NeRFReplicaInferenceHandler.grid_centres(lo, hi, res, device=r.device)
        want = r.query_points(centres, None, which=1, precision=precision, outputs=("raw",))["raw"]
        r.bake_radiance_grid(lo, hi, res, which=1, view_dir=None, precision=precision)
        got = r.radiance_grid_values().reshape(-1, 4)
        assert np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32)) and float(np.std(got)) > 1e-3
        with pytest.raises(ValueError, match="dir3_host must be null"):
            r.bake_radiance_grid(lo, hi, res, which=1, view_dir=(0, 0, 1), precision=precision)
    finally:
        r.close()


def test_a_baked_frame_resembles_the_networks_own():
    """Loosely: a 24^3 grid (1-unit cells) of dense_fog(0.15, 1.0), a fog whose raw density changes sign over the frame.  Where it is
    positive at a ray's last sample the opacity is 1 whatever lies in front (the last interval is 1e10 long), so only a scene with
    empty regions has an opacity to compare at all: this one has acc from 0.34 to 1.  A random network's density has structure far
    below the cell size - the worst case for a grid - so the frames agree loosely.  The quality numbers belong to
    tools/radiance_grid_ab.py; here the PSNR is printed and asserted only to be finite, and the opacity to correlate with the
    network's: r > 3 / sqrt(rays), three standard deviations of the r of as many uncorrelated rays (0.137 for 481)."""
    S = nwe_amd.synthetic
    _, _, cfg, poses, _, H, W = B.scene("s7")
    sds = (S.thin_fog(S.make_state_dict(1000, 4, 128)), S.dense_fog(S.make_state_dict(1001, 4, 128), 0.15, 1.0))
    h = _handler("f16x3", sds, cfg.n_samples, cfg.n_importance)
    try:
        ref = h.render(poses[0].numpy(), H, W)
        h.bake_radiance_grid(R.BOX_LO, R.BOX_HI, 24)
        out = h.render_grid(poses[0].numpy(), H, W)
        mse = float(((out["rgb"] - ref["rgb"]) ** 2).mean())
        psnr = -10.0 * math.log10(mse) if mse > 0 else float("inf")
        corr = float(torch.corrcoef(torch.stack([out["acc"].reshape(-1), ref["acc"].reshape(-1)]))[0, 1])
        print(f"24^3 grid frame against the network's: PSNR {psnr:.1f} dB, acc correlation {corr:.3f}, "
              f"acc {float(ref['acc'].min()):.3f} .. {float(ref['acc'].max()):.3f}")
        assert math.isfinite(mse) and not math.isnan(psnr) and all(bool(torch.isfinite(out[k]).all()) for k in LEAN)
        assert float(ref["acc"].std()) > 0.01 and corr > 3.0 / math.sqrt(H * W)
    finally:
        h.renderer.close()


# ---- 7. sequences ---------------------------------------------------------------------------------------------------------------

def test_a_grid_frame_between_two_renders_moves_nothing_of_theirs():
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7")
    g = R.grid("random")
    r, fresh = nwe_amd.Renderer(0), _grid_renderer("random", cfg.n_samples, cfg.n_importance)
    try:
        r.set_network(0, sd_c); r.set_network(1, sd_f)
        r.set_sampling(cfg.n_samples, cfg.n_importance)
        cam = _camera(H, W)
        assert r.last_grid_ms() is None
        first = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        r.query_points(torch.zeros(5, 3, device=r.device), None, outputs=("sigma",))
        reports = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_plan(), r.last_ray_evaluations(), r.last_coarse_launch(),
                           r.last_query_ms())
        before = reports()
        _set(r, g)                                              # behind the networks: an upload clears the grid
        want = _frame(fresh, poses, H, W)
        got = _frame(r, poses, H, W)
        _same(got, want, "a context with networks and a context without")
        ms = r.last_grid_ms()
        assert ms is not None and ms > 0 and reports() == before
        assert _frame(r, poses, H, W, rows=(3, 3))["rgb"].numel() == 0 and r.last_grid_ms() == ms   # zero rays: nothing launched
        second = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        _same(first, second, "the render after a grid frame")
        assert r.last_grid_ms() == ms                           # a render moves nothing of the grid's
        # none of the modes is read: the grid frame keeps its bits under every one of them
        r.set_early_termination(0.05)
        _same(_frame(r, poses, H, W), want, "early termination")
        r.set_early_termination(0.0)
        r.set_shared_coarse(4); r.set_separate_passes(True)
        _same(_frame(r, poses, H, W), want, "shared coarse, separate passes")
        r.set_shared_coarse(1); r.set_separate_passes(False)
        r.set_occupancy(np.zeros((2, 2, 2), bool), R.BOX_LO, R.BOX_HI, (2, 2, 2))
        r.set_coarse_grid(np.zeros((2, 2, 2), np.float32), R.BOX_LO, R.BOX_HI)
        r.debug_set_decomposition(1); r.debug_set_packet_blocks(False)
        _same(_frame(r, poses, H, W), want, "occupancy grid, coarse grid, decomposition")
        assert r.occupancy is not None and r.coarse_grid is not None      # and nothing of them was cleared
        r.clear_occupancy(); r.clear_coarse_grid(); r.debug_set_decomposition(-1); r.debug_set_packet_blocks(True)
        # an armed hook stays armed over a grid frame: it is the next nwe_render_rays that consumes it
        rays = r.create_rays(poses.numpy(), H, W, **cam)
        z = torch.linspace(R.NEAR, R.FAR, cfg.n_samples + cfg.n_importance, device=r.device).expand(rays.shape[0], -1).contiguous()
        hooked = r.render_rays(rays, precision="f32", debug_fine_depths=z, outputs=("z_fine",))
        _lib.load().nwe_debug_set_fine_depths(r._ctx, z.data_ptr())
        _same(_frame(r, poses, H, W), want, "an armed hook")
        again = r.render_rays(rays, precision="f32", outputs=("z_fine",))
        assert torch.equal(again["z_fine"], hooked["z_fine"]) and torch.equal(again["z_fine"], z)
        # the sampling tables are the grid frame's own input, and the white background
        r.set_sampling(cfg.n_samples, 0); fresh.set_sampling(cfg.n_samples, 0)
        _same(_frame(r, poses, H, W), _frame(fresh, poses, H, W), "n_importance = 0")
        r.set_white_background(True)
        white = _frame(r, poses, H, W)
        assert not torch.equal(white["rgb"], _frame(fresh, poses, H, W)["rgb"])
        fresh.set_white_background(True)
        _same(white, _frame(fresh, poses, H, W), "white background")
        # a new grid replaces the old one; clearing refuses the next frame by name
        _set(r, R.grid("small_nonfinite")); _set(fresh, R.grid("small_nonfinite"))
        _same(_frame(r, poses, H, W), _frame(fresh, poses, H, W), "a second grid")
        r.clear_radiance_grid()
        with pytest.raises(RuntimeError, match="no grid is set"):
            _frame(r, poses, H, W)
        third = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        assert not torch.equal(third["rgb"], first["rgb"])     # white background, n_importance = 0: the context's own state
    finally:
        r.close(); fresh.close()
