"""The sparse frame on the GPU (include/nwe.h: nwe_render_sparse; the kernels: csrc/nwe_sparse.hip).

The steps of the rule are checked one by one through the call's diagnostics, bit for bit unless said otherwise: the proposal against
nwe_render_grid's own diagnostics; the mask against the numpy rule (tests/sparse_fine.py) on the call's own weights; the rows
against nwe_query_points at the helper's points where selected and against the grid's rows elsewhere; the frame against the ordinary
machinery (nwe_render_rays under f32) fed the call's weights, rows and depths.  At min_weight = 2 the frame is the grid's, at
min_weight = -1 it is nwe_render's under a baked coarse pass.  Chunks, row tiles, pose batches and streams give the whole call's
bits, and the call moves nothing of the other calls' reports.  Parity with the composed oracle holds on the room scene at the
project's tolerances.  "Bit for bit" lets a NaN equal a NaN whatever its sign and payload.
The frames here have at most 481 rays a chunk (700 under the hook).  Chunks beyond one scan tile of 1024 rays, the default chunk
of 2^22 / S rays that splits a call, the scratch buffer grown and reused, and a grid axis of 512 cells under the proposal's
lookup are covered by tests/test_gpu_grid_sizes.py; so are the bakes beyond 2^20 cells.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd.handler import NeRFReplicaInferenceHandler
from oracle import nerf_oracle as O
from tests import coarse_grid as B
from tests import radiance_grid as R
from tests import sparse_fine as SF

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
DIAG = ("weights_coarse", "z_fine", "weights_grid", "selected", "raw_fine")
TOL = {"rgb": 1e-4, "depth": 1e-4 * R.FAR, "acc": 1e-4}           # tests/test_gpu_radiance_grid.py


def _camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=R.NEAR, far=R.FAR)


def _renderer(grid, ns, ni, sds=None):
    """Both networks of a scene (s7's by default) and the grid behind them: an upload clears a grid."""
    sd_c, sd_f = sds or B.scene("s7")[:2]
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    if grid is not None:
        r.set_radiance_grid(grid["values"], grid["lo"], grid["hi"])
    return r


def _sparse(r, poses, H, W, rows=None, outputs=LEAN, **kw):
    return r.render_sparse(poses.numpy(), H, W, rows=rows, outputs=outputs, **_camera(H, W), **kw)


def _grid_frame(r, poses, H, W, outputs=LEAN):
    return r.render_grid(poses.numpy(), H, W, outputs=outputs, **_camera(H, W))


def _eq(a, b):
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _same(a, b, ctx, keys=LEAN):
    for k in keys:
        assert _eq(a[k], b[k]), (ctx, k)
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _far_pose(poses):
    """A second pose a hundred units away: every sample of its rays lies outside every box of the tests."""
    far = poses[:1].clone()
    far[0, 0, 3] += 100.0
    return torch.cat([poses[:1], far])


# ---- 1. the proposal ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("random", 7, 6), ("small_nonfinite", 64, 128), ("smooth", 3, 1), ("smooth", 7, 0)])
def test_the_proposal_is_the_grid_frames_own(kind, ns, ni):
    poses = R.scene("s7")[1]
    H, W = R.H, R.W
    r = _renderer(R.grid(kind), ns, ni)
    try:
        got = _sparse(r, poses, H, W, outputs=DIAG)
        ref = _grid_frame(r, poses, H, W, outputs=("weights_coarse", "z_fine", "raw_fine"))
        assert _eq(got["weights_coarse"], ref["weights_coarse"]) and _eq(got["z_fine"], ref["z_fine"])
        assert tuple(got["weights_grid"].shape) == (H * W, ns + ni) and got["selected"].dtype == torch.uint8
        if ni == 0:
            assert _eq(got["weights_grid"], got["weights_coarse"])
            return
        rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W)).cpu()
        with torch.no_grad():
            want = O.raw2outputs(ref["raw_fine"].cpu(), ref["z_fine"].cpu(), rays[:, 3:6], False)[3]
        w = got["weights_grid"].cpu()
        assert torch.equal(torch.isnan(w), torch.isnan(want))
        err = float((w - want).abs().nan_to_num(0.0).max())
        print(f"weights_grid against raw2outputs on the grid frame's rows, {kind} {ns}+{ni}: {err:.2e} (tol 1e-06)")
        assert err <= 1e-6            # the tolerance tests/test_gpu_coarse_grid.py holds weights to
        assert float(w.nan_to_num(0.0).max()) > 0.01
    finally:
        r.close()


# ---- 2. the selection -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("smooth", 64, 128), ("small_nonfinite", 7, 6), ("random", 3, 1), ("smooth", 7, 0)])
def test_the_mask_is_the_numpy_rule_on_the_calls_own_weights(kind, ns, ni):
    H, W = R.H2, R.W2
    poses = _far_pose(R.scene("s7", True)[1])
    r = _renderer(R.grid(kind), ns, ni)
    try:
        for min_weight, dilate in ((1e-3, 0), (1e-3, 1), (0.05, 8), (-1.0, 0), (2.0, 3)):
            out = _sparse(r, poses, H, W, outputs=("weights_grid", "selected"), min_weight=min_weight, dilate=dilate)
            w, sel = out["weights_grid"].cpu().numpy(), out["selected"].cpu().numpy()
            want = SF.select(w, min_weight, dilate)
            assert sel.dtype == np.uint8 and set(np.unique(sel)) <= {0, 1}
            assert np.array_equal(sel.astype(bool), want), (kind, min_weight, dilate)
            assert r.last_sparse_samples() == (int(want.sum()), 2 * H * W * (ns + ni))
            if min_weight < 0:
                assert want.all()
            if min_weight == 2.0:
                assert not want[~np.isnan(w).any(-1)].any()       # no weight is above 1, so only a NaN is a hit there
            if kind == "smooth" and ni > 0 and min_weight == 1e-3:
                per_ray = want.sum(-1)
                mixed = (per_ray > 0) & (per_ray < ns + ni)
                print(f"smooth grid {ns}+{ni}, min_weight 1e-3, dilate {dilate}: {int(mixed.sum())} rays with both values, "
                      f"{int((per_ray == 0).sum())} with none, share {want.mean():.3f}")
                assert mixed.any() and (per_ray == 0).any()       # the cases are there
    finally:
        r.close()


# ---- 3. the rows ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,precision", [("s7", "f32"), ("s7", "f16x3"), ("novd", "f32"), ("novd", "f16x3"), ("big7", "f16x3")])
def test_rows_are_the_querys_where_selected_and_the_grids_elsewhere(scene, precision):
    sd_c, sd_f, cfg, poses, _, H, W = B.scene(scene)
    r = _renderer(R.grid("smooth"), cfg.n_samples, cfg.n_importance, (sd_c, sd_f))
    try:
        out = _sparse(r, poses, H, W, outputs=("z_fine", "selected", "raw_fine"), precision=precision, min_weight=0.06, dilate=1)
        sel = out["selected"].bool()
        assert bool(sel.any()) and bool((~sel).any())
        rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W))
        pts = torch.from_numpy(SF.points(rays.cpu().numpy(), out["z_fine"].cpu().numpy())).to(r.device)
        dirs = rays[:, 8:11].contiguous() if scene != "novd" else None
        q = r.query_points(pts, dirs, which=1, precision=precision, outputs=("raw",))["raw"]
        grid_rows = _grid_frame(r, poses, H, W, outputs=("raw_fine",))["raw_fine"]
        assert _eq(out["raw_fine"][sel], q[sel]), "selected rows"
        assert _eq(out["raw_fine"][~sel], grid_rows[~sel]), "the other rows"
        assert not _eq(q[sel], grid_rows[sel])
    finally:
        r.close()


# ---- 4. the frame ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kind,ns,ni,hw", [("random", 3, 1, None), ("small_nonfinite", 7, 6, None), ("random", 64, 128, None),
                                           ("smooth", 128, 256, (4, 4))])
def test_the_frame_is_the_ordinary_machinery_fed_the_mix(kind, ns, ni, hw, white):
    H, W = hw or (R.H, R.W)
    poses, _ = B.G.E.frame_rays(H, W, 1)
    r = _renderer(R.grid(kind), ns, ni)
    try:
        r.set_white_background(white)
        out = _sparse(r, poses, H, W, outputs=LEAN + DIAG, precision="f32", min_weight=0.02, dilate=1)
        sel = out["selected"].bool()
        assert bool(sel.any()) and bool((~sel).any())
        rays = r.create_rays(poses.numpy(), H, W, **_camera(H, W))
        ref = r.render_rays(rays, precision="f32", outputs=LEAN + ("z_fine",), debug_coarse_weights=out["weights_coarse"],
                            debug_raw=(None, out["raw_fine"]), debug_fine_depths=out["z_fine"])
        for k in LEAN + ("z_fine",):
            assert _eq(out[k], ref[k]), (kind, ns, ni, white, k)
        assert int(out["flags"].item()) == int(ref["flags"].item()) & 0x7     # the rgb / depth / acc bits, and no other
    finally:
        r.close()


# ---- 5. the ends of the range ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("random", 7, 6), ("smooth", 64, 128), ("random", 7, 0)])
def test_nothing_selected_is_the_grid_frame(kind, ns, ni):
    poses = R.scene("s7")[1]
    r = _renderer(R.grid(kind), ns, ni)
    try:
        out = _sparse(r, poses, R.H, R.W, outputs=LEAN + ("selected", "raw_fine"), min_weight=2.0, dilate=0)
        ref = _grid_frame(r, poses, R.H, R.W, outputs=LEAN + ("raw_fine",))
        assert int(out["selected"].sum()) == 0 and r.last_sparse_samples() == (0, R.H * R.W * (ns + ni))
        _same(out, ref, "min_weight 2", LEAN + ("raw_fine",))
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("net", ["room", "s7"])
def test_everything_selected_is_the_render_under_a_baked_coarse_pass(net, precision):
    """The coarse grid holds the radiance grid's sigma channel over the same box, so both calls draw the same fine depths; the
    render kernels evaluate the fine network at them, the sparse frame the point query - bit-identical by the query's contract."""
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7")
    if net == "room":
        sd_f = SF.room_net()
    g = R.grid("smooth")
    r = _renderer(g, cfg.n_samples, cfg.n_importance, (sd_c, sd_f))
    try:
        out = _sparse(r, poses, H, W, outputs=LEAN + ("selected",), precision=precision, min_weight=-1.0, dilate=0)
        assert bool(out["selected"].bool().all())
        r.set_coarse_grid(np.ascontiguousarray(g["values"][..., 3]), g["lo"], g["hi"])
        ref = r.render(poses.numpy(), H, W, precision=precision, outputs=LEAN, **_camera(H, W))
        for k in LEAN:
            diff = float((out[k] - ref[k]).abs().nan_to_num(0.0).max())
            print(f"min_weight -1 against the baked coarse render, {net} {precision} {k}: max |diff| {diff:.2e}")
        _same(out, ref, (net, precision))
    finally:
        r.close()


# ---- 6. chunks, tiles, batches --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,ns,ni", [("small_nonfinite", 7, 6), ("smooth", 64, 32)])
def test_chunks_row_tiles_pose_batches_and_streams_give_the_whole_calls_bits(kind, ns, ni):
    keys = LEAN + DIAG
    H, W = SF.H3, SF.W3
    poses, _ = B.G.E.frame_rays(H, W, 3)
    kw = dict(min_weight=0.03, dilate=2, outputs=keys)
    r = _renderer(R.grid(kind), ns, ni)
    try:
        whole = _sparse(r, poses[:1], H, W, **kw)
        count = r.last_sparse_samples()
        sel = whole["selected"].bool()
        assert bool(sel.any()) and bool((~sel).any()) and count == (int(sel.sum()), H * W * (ns + ni))
        nan = torch.isnan(whole["weights_grid"])
        if kind == "small_nonfinite":                               # a NaN weight is a hit: the rule's own comparison
            assert bool(nan.any()) and bool(sel[nan].all())
        for chunk in (64, 1, 100):
            r.debug_set_sparse_chunk(chunk)
            _same(_sparse(r, poses[:1], H, W, **kw), whole, ("chunk", chunk), keys)
            assert r.last_sparse_samples() == count
        r.debug_set_sparse_chunk(0)
        with pytest.raises(ValueError):
            r.debug_set_sparse_chunk(-1)
        tiles = [_sparse(r, poses[:1], H, W, rows=rows, **kw) for rows in ((0, 2), (2, 7), (7, H))]
        for k in keys:
            assert _eq(torch.cat([t[k] for t in tiles]), whole[k]), (k, "row tiles")
        flags = 0
        for t in tiles:
            flags |= int(t["flags"].item())
        assert flags == int(whole["flags"].item())
        ms = r.last_sparse_ms()
        empty = _sparse(r, poses[:1], H, W, rows=(5, 5))
        assert tuple(empty["rgb"].shape) == (0, 3) and int(empty["flags"].item()) == 0 and r.last_sparse_ms() == ms
        r.debug_set_sparse_chunk(700)                               # a chunk border inside the second pose
        both = _sparse(r, poses, H, W, **kw)
        r.debug_set_sparse_chunk(0)
        each = [_sparse(r, poses[p:p + 1], H, W, **kw) for p in range(3)]
        for k in keys:
            assert _eq(torch.cat([e[k] for e in each]), both[k]), (k, "pose batch")
        assert _eq(each[0]["rgb"], whole["rgb"])
        streams = [torch.cuda.Stream(device=r.device) for _ in range(2)]
        outs = []
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(_sparse(r, poses[:1], H, W, **kw))
        for s in streams:
            s.synchronize()
        for o in outs:
            _same(o, whole, "streams", keys)
    finally:
        r.close()


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------------

def test_a_sparse_frame_between_two_renders_moves_nothing_of_theirs():
    sd_c, sd_f, cfg, poses, _, H, W = B.scene("s7")
    g = R.grid("random")
    r, fresh = _renderer(None, cfg.n_samples, cfg.n_importance), _renderer(g, cfg.n_samples, cfg.n_importance)
    kw = dict(min_weight=0.02, dilate=1)
    try:
        cam = _camera(H, W)
        assert r.last_sparse_ms() is None and r.last_sparse_samples() is None
        first = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        r.query_points(torch.zeros(5, 3, device=r.device), None, outputs=("sigma",))
        r.set_radiance_grid(g["values"], g["lo"], g["hi"])
        r.render_grid(poses.numpy(), H, W, **cam)
        reports = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_plan(), r.last_ray_evaluations(), r.last_coarse_launch(),
                           r.last_query_ms(), r.last_grid_ms())
        before = reports()
        want = _sparse(fresh, poses, H, W, **kw)
        got = _sparse(r, poses, H, W, **kw)
        _same(got, want, "two contexts")
        ms = r.last_sparse_ms()
        assert ms is not None and ms > 0 and reports() == before and before[0] > 0
        second = r.render(poses.numpy(), H, W, precision="f16x3", **cam)
        _same(first, second, "the render after a sparse frame")
        assert r.last_sparse_ms() == ms
        # none of the modes is read: the sparse frame keeps its bits under every one of them
        r.set_early_termination(0.05)
        _same(_sparse(r, poses, H, W, **kw), want, "early termination")
        r.set_early_termination(0.0)
        r.set_shared_coarse(4); r.set_separate_passes(True)
        _same(_sparse(r, poses, H, W, **kw), want, "shared coarse, separate passes")
        r.set_shared_coarse(1); r.set_separate_passes(False)
        r.set_occupancy(np.zeros((2, 2, 2), bool), R.BOX_LO, R.BOX_HI, (2, 2, 2))
        r.set_coarse_grid(np.zeros((2, 2, 2), np.float32), R.BOX_LO, R.BOX_HI)
        r.debug_set_decomposition(1); r.debug_set_packet_blocks(False); r.debug_set_work_queue(1); r.debug_set_colour_skip(0)
        _same(_sparse(r, poses, H, W, **kw), want, "occupancy grid, coarse grid, decomposition, queue, colour skip")
        assert r.occupancy is not None and r.coarse_grid is not None      # and nothing of them was cleared
    finally:
        r.close(); fresh.close()


def test_the_refusals_that_need_a_device():
    """The last refusal of the order (tests/test_sparse_fine_host.py walks the others): an MFMA precision for a shape without a query
    kernel, with the query's own message, behind everything else - and nothing is launched or reported."""
    S = nwe_amd.synthetic
    g = R.grid("random")
    r = _renderer(None, 7, 6, (S.make_state_dict(5, 3, 64, skips=()), B.scene("s7")[1]))
    try:
        poses = R.scene("s7")[1]
        with pytest.raises(RuntimeError, match="no radiance grid is set"):
            _sparse(r, poses, R.H, R.W, which=0)
        r.set_radiance_grid(g["values"], g["lo"], g["hi"])
        with pytest.raises(NotImplementedError, match="no MFMA kernel for this network shape"):
            _sparse(r, poses, R.H, R.W, which=0)
        with pytest.raises(ValueError, match="dilate must be in 0..8"):
            _sparse(r, poses, R.H, R.W, which=0, dilate=9)          # in front of the shape
        assert r.last_sparse_ms() is None and r.last_sparse_samples() is None
        out = _sparse(r, poses, R.H, R.W, which=0, precision="f32")   # the fp32 query serves every shape
        assert bool(torch.isfinite(out["rgb"]).all()) and r.last_sparse_samples()[1] == R.H * R.W * 13
        assert _sparse(r, poses, R.H, R.W, which=1)["rgb"].shape == (R.H * R.W, 3)
    finally:
        r.close()


# ---- 8. parity ------------------------------------------------------------------------------------------------------------------

def test_parity_with_the_composed_oracle_on_the_room():
    """Every ray of the room at 64 + 128 with a 32^3 grid; left out are only rays whose selection may differ for a rounding's sake:
    an oracle weight within 1e-6 of min_weight (tests/test_sparse_fine_host.py holds them to 1 % of the rays)."""
    cfg, poses, _, sd, grid = SF.parity_scene()
    ref = SF.parity_reference()
    keep = ref["margin"] >= SF.PARITY_MARGIN
    assert float((~keep).float().mean()) <= SF.PARITY_CAP
    r = _renderer(grid, cfg.n_samples, cfg.n_importance, (B.scene("s7")[0], sd))
    try:
        out = _sparse(r, poses, R.H, R.W, outputs=LEAN + ("selected",), min_weight=SF.PARITY_MIN_WEIGHT, dilate=SF.PARITY_DILATE)
        same_mask = (out["selected"].cpu().bool() == ref["selected"]).all(-1)
        print(f"sparse parity: {int((~keep).sum())} rays left out, {int((~same_mask & keep).sum())} kept rays with another mask, "
              f"selected share {float(out['selected'].float().mean()):.3f}")
        for k in LEAN:
            err = (out[k].cpu() - ref[k]).abs()[keep]
            print(f"sparse parity {k}: {float(err.max()):.2e} (tol {TOL[k]:.0e})")
            assert float(err.max()) <= TOL[k], k
        assert int(out["flags"].item()) == 0
        share = r.last_sparse_samples()
        assert 0 < share[0] < share[1]
    finally:
        r.close()


# ---- 9. the handler -------------------------------------------------------------------------------------------------------------

def test_the_handler_draws_its_frame_through_the_sparse_call():
    sd_c = B.scene("s7")[0]
    opt = {"min_weight": 1e-3, "dilate": 1}
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3", sparse_fine=opt,
                                    radiance_grid={"lo": SF.ROOM_LO, "hi": SF.ROOM_HI, "resolution": 16, "view_dir": (0.0, 0.0, 1.0)})
    h.set_sampling(7, 6)
    h.initialize_models(state_dicts=(sd_c, SF.room_net()))
    try:
        assert h.last_sparse_samples() is None
        init, coord = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
        img = h.render_coordinates(init, coord)
        selected, total = h.last_sparse_samples()
        Hh, Wh = h.image_size
        assert total == Hh * Wh * 13 and 0 < selected < total
        pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [coord])
        want = h.renderer.to8b(h.render_sparse(pose[0].numpy(), **opt)["rgb"]).cpu().numpy()
        assert img.shape == (Hh, Wh, 3) and img.dtype == np.uint8 and np.array_equal(img, want.reshape(Hh, Wh, 3))
        # preview frames stay what they were
        h.render_coordinates(init, coord, preview="grid")
        assert h.last_sparse_samples() == (selected, total)
    finally:
        h.renderer.close()
