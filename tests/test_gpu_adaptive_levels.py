"""The multi-level adaptive frame on the GPU (include/nwe.h: nwe_render_adaptive_levels; the kernels: csrc/nwe_adaptive_levels.hip).

The reference of every comparison is the frame nwe_render draws on the same context, put through the numpy restatement of the rule
(tests/adaptive_levels.py; for levels = 1 also tests/adaptive.py) - never the call under test.  Everything is compared bit for bit
("bit for bit" lets a NaN equal a NaN whatever its sign and payload).
The shapes are those of tests/test_gpu_adaptive.py - the 4 x 128 network with 16 + 16 samples, the room scene, the same pose - on
frames of 37 x 45 (36 and 44 are multiples of 4, not of 8) and 33 x 41 (32 and 40 are multiples of 8): ragged and aligned last
cells occur at every level.  37 x 45 is 1665 pixels, more than one scan tile of 1024."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler, pinhole_intrinsics
from oracle import nerf_oracle as O
from tests import adaptive as A
from tests import adaptive_levels as L

pytestmark = pytest.mark.gpu

H, W = 37, 45
NS, NI = 16, 16
NEAR, FAR = 0.1, 8.0
ALL = ("rgb", "depth", "acc", "kind", "level")
MASK = A.FLAG_RGB | A.FLAG_DEPTH | A.FLAG_ACC
INF = float("inf")
REPORT = ("pixels", "lattice", "levels", "render_launches", "rendered", "interpolated")


def _pose(x=0.3, y=-0.2, z=0.1):
    p = np.eye(4, dtype=np.float32)
    p[:3, 3] = (x, y, z)
    return p[None]


def _two_poses():
    poses = np.concatenate([_pose(), _pose(-0.8, 0.4, -0.3)])
    poses[1, :3, :3] = O.camera_pose((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0, 0, 0, 40.0, 10.0, 0.0))[0, :3, :3].numpy()
    return poses


def _room(seed=7, D=4, Wn=128, skips=()):
    return synthetic.room(synthetic.make_state_dict(seed, D, Wn, skips=skips))


def _camera(h, w):
    fx, fy, cx, cy = O.intrinsics(h, w)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def _renderer(sd_c=None, sd_f=None):
    sd_c = _room() if sd_c is None else sd_c
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_c if sd_f is None else sd_f)
    r.set_sampling(NS, NI)
    return r


@pytest.fixture(scope="module")
def room():
    """One context for the tests that change nothing of it (or put back what they change)."""
    r = _renderer()
    yield r
    r.close()


def _stack(out, n, h, w):
    return torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy().reshape(n, h, w, 5)


def _full(r, poses, h=H, w=W, rows=None, precision="f16x3"):
    """nwe_render's frame [P, rows, w, 5] (r, g, b, depth, acc) and its rgb / depth / acc flag bits."""
    out = r.render(poses, h, w, rows=rows, precision=precision, outputs=("rgb", "depth", "acc"), **_camera(h, w))
    r0, r1 = rows or (0, h)
    return _stack(out, len(poses), r1 - r0, w), int(out["flags"].item()) & MASK


def _levels(r, poses, h=H, w=W, rows=None, precision="f16x3", **kw):
    """The call under test: frame, kinds, levels, flags, report."""
    out = r.render_adaptive(poses, h, w, rows=rows, precision=precision, outputs=ALL, **_camera(h, w), **kw)
    r0, r1 = rows or (0, h)
    shape = (len(poses), r1 - r0, w)
    rep = r.last_adaptive_levels()
    assert rep["ms"] > 0.0
    return (_stack(out, *shape), out["kind"].cpu().numpy().reshape(shape), out["level"].cpu().numpy().reshape(shape), int(out["flags"].item()),
            {key: rep[key] for key in REPORT})


def _want(full, first_row, k, levels, tol_rgb, tol_depth):
    """The restatement on every pose of nwe_render's frame: frame, kinds, levels, the call's counts, the interpolation's flag bits."""
    parts = [L.apply(f, first_row, k, levels, tol_rgb, tol_depth) for f in full]
    flags = 0
    for out, kind, _, _ in parts:
        flags |= A.interpolation_flags(out, kind)
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]), L.add_counts([p[3] for p in parts]), flags


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _check(r, poses, k, levels, tol_rgb, tol_depth, h=H, w=W, rows=None, precision="f16x3", full=None):
    """One call against the restatement on the context's own nwe_render frame; returns the restatement's counts."""
    full, full_flags = _full(r, poses, h, w, rows, precision) if full is None else full
    got, kind, level, flags, report = _levels(r, poses, h, w, rows, precision, k=k, levels=levels, tol_rgb=tol_rgb, tol_depth=tol_depth)
    want, want_kind, want_level, counts, interp_flags = _want(full, (rows or (0, h))[0], k, levels, tol_rgb, tol_depth)
    ctx = (h, w, rows, precision, k, levels, tol_rgb)
    print(ctx, counts)
    assert np.array_equal(kind, want_kind), ctx
    assert np.array_equal(level, want_level), ctx
    assert _same_bits(got, want), ctx
    assert report == counts, ctx
    assert flags == full_flags | interp_flags, ctx
    return counts


# ---- 1. one level is the adaptive frame -----------------------------------------------------------------------------------------

def test_one_level_is_nwe_render_adaptive(room):
    r, poses = room, _pose()
    full = _full(r, poses)
    for k in (1, 2, 3, 5):
        old = r.render_adaptive(poses, H, W, outputs=("rgb", "depth", "acc", "kind"), k=k, tol_rgb=0.05, tol_depth=0.05, **_camera(H, W))
        old_counts = r.last_adaptive()
        got, kind, level, flags, report = _levels(r, poses, k=k, levels=1, tol_rgb=0.05, tol_depth=0.05)
        assert _same_bits(got, _stack(old, 1, H, W)) and np.array_equal(kind.reshape(-1), old["kind"].cpu().numpy()), k
        assert flags == int(old["flags"].item())
        assert (report["pixels"], report["lattice"], report["rendered"], report["interpolated"]) == \
            (old_counts["pixels"], old_counts["lattice"], [old_counts["rendered"]], [old_counts["interpolated"]]), k
        assert report["render_launches"] == (2 if old_counts["rendered"] else 1)
        want = A.apply(full[0][0], 0, k, 0.05, 0.05)                 # ... and both are tests/adaptive.py on nwe_render's frame
        assert _same_bits(got[0], want[0]) and np.array_equal(kind[0], want[1]), k
        _check(r, poses, k, 1, 0.05, 0.05, full=full)


# ---- 2. the exact regime --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_a_negative_tolerance_renders_every_pixel_with_nwe_renders_bits(room, precision):
    r, poses = room, _pose()
    full, full_flags = _full(r, poses, precision=precision)
    assert np.isfinite(full).all() and float(np.ptp(full[..., :3])) > 0.05          # a frame with something in it
    for k, levels in ((2, 2), (2, 3), (1, 3), (3, 2), (1, 4)):
        got, kind, level, flags, report = _levels(r, poses, precision=precision, k=k, levels=levels, tol_rgb=-1.0, tol_depth=-1.0)
        assert _same_bits(got, full), (precision, k, levels)
        assert flags == full_flags and not (kind == A.KIND_INTERPOLATED).any()
        plan = L.plan(1, H, W, k, levels)                                           # every pass is full
        assert report == {"pixels": H * W, "lattice": plan["lattice"], "levels": levels, "rendered": plan["pass_max"][1:],
                          "interpolated": [0] * levels, "render_launches": 1 + sum(1 for n in plan["pass_max"][1:] if n)}
        assert [int((level == i).sum()) for i in range(levels + 1)] == plan["pass_max"]
        if k == 2:
            assert plan["pass_max"][-1] == 1228                                     # the last pass: more than one scan tile
        else:
            assert (plan["pass_max"][-1] == 0) == (k == 1)                          # k = 1: the last pass is empty


# ---- 3. the mixed regime --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,k,levels,tol_rgb", [(37, 45, 2, 3, 16 / 255), (33, 41, 2, 3, 20 / 255)])
def test_the_frame_the_kinds_the_levels_and_the_counts_are_the_restatements(room, h, w, k, levels, tol_rgb):
    counts = _check(room, _pose(), k, levels, tol_rgb, 0.5, h=h, w=w)
    # the condition the inputs are chosen for, on the restatement's own counts: every pass and every level is populated
    assert all(n > 0 for n in counts["rendered"]) and all(n > 0 for n in counts["interpolated"]), counts
    assert counts["render_launches"] == levels + 1


def test_an_odd_finest_spacing(room):
    _check(room, _pose(), 3, 2, 16 / 255, 0.5)


# ---- 4. the all-flat and the all-busy regime ------------------------------------------------------------------------------------

def test_an_infinite_tolerance_makes_one_render_launch(room):
    r = room
    for k, levels in ((2, 3), (3, 2)):
        counts = _check(r, _pose(), k, levels, INF, INF)
        assert counts["render_launches"] == 1 and counts["rendered"] == [0] * levels
        assert counts["interpolated"] == [H * W - counts["lattice"]] + [0] * (levels - 1)
        # the last render launch made is pass 0, and there was no other
        assert r.last_ray_evaluations() == (counts["lattice"] * (2 * NS + NI),) * 2


def test_a_nan_colour_makes_the_cells_busy_at_every_level():
    sd_f = _room()
    sd_f["_rgb_linear.bias"] = np.full_like(sd_f["_rgb_linear.bias"], np.nan)
    r = _renderer(sd_f=sd_f)
    try:
        poses = _pose()
        full = _full(r, poses)
        assert np.isnan(full[0][..., :3]).all() and np.isfinite(full[0][..., 3:]).all() and full[1] == A.FLAG_RGB
        for k, levels in ((2, 3), (3, 2)):
            counts = _check(r, poses, k, levels, INF, INF, full=full)
            assert counts["interpolated"] == [0] * levels and counts["rendered"] == L.plan(1, H, W, k, levels)["pass_max"][1:]
    finally:
        r.close()


# ---- 5. shapes and calls --------------------------------------------------------------------------------------------------------

def test_two_poses_are_two_single_pose_calls(room):
    r, poses = room, _two_poses()
    k, levels, tol = 2, 3, 16 / 255
    both = _levels(r, poses, k=k, levels=levels, tol_rgb=tol, tol_depth=0.5)
    singles = [_levels(r, poses[i:i + 1], k=k, levels=levels, tol_rgb=tol, tol_depth=0.5) for i in range(2)]
    for i in range(2):
        assert _same_bits(both[0][i], singles[i][0][0]) and np.array_equal(both[1][i], singles[i][1][0]) and np.array_equal(both[2][i], singles[i][2][0])
    assert both[3] == singles[0][3] | singles[1][3]
    assert both[4] == L.add_counts([singles[0][4], singles[1][4]])
    assert not np.array_equal(both[1][0], both[1][1])           # two different views
    _check(r, poses, k, levels, tol, 0.5)


def test_a_row_tile_has_its_own_lattices(room):
    for k, levels in ((2, 3), (3, 2)):
        _check(room, _pose(), k, levels, 16 / 255, 0.5, rows=(5, 30))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (9, 1), (2, 3)])
def test_degenerate_frames(room, h, w):
    for k, levels in ((1, 1), (2, 2), (1, 4), (8, 4)):
        for tol in (-1.0, 0.05, INF):
            _check(room, _pose(), k, levels, tol, tol, h=h, w=w)


def test_the_list_switch_changes_no_bit(room):
    r, poses = room, _pose()
    assert not r.adaptive_pixel_lists
    off = _levels(r, poses, k=2, levels=3, tol_rgb=16 / 255, tol_depth=0.5)
    r.set_adaptive_pixel_lists(True)
    try:
        on = _levels(r, poses, k=2, levels=3, tol_rgb=16 / 255, tol_depth=0.5)
        assert r.last_pixels() == {"n": off[4]["rendered"][-1], "path": "list"}      # the last pass went through the list kernels
        _check(r, poses, 2, 3, 16 / 255, 0.5)
        _check(r, poses, 2, 2, -1.0, -1.0, precision="f32")                                 # no list kernels: the ray table, as without the switch
    finally:
        r.set_adaptive_pixel_lists(False)
    assert _same_bits(on[0], off[0]) and np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2]) and on[3:] == off[3:]


def test_the_white_background_is_honoured():
    r = _renderer()
    try:
        plain = _full(r, _pose())[0]
        r.set_white_background(True)
        assert not _same_bits(_full(r, _pose())[0], plain)
        _check(r, _pose(), 2, 3, 16 / 255, 0.5)
    finally:
        r.close()


def test_separate_passes_keep_two_shapes_on_the_mfma_kernels():
    r = _renderer(sd_c=_room(7, 4, 128, ()), sd_f=_room(8, 8, 256, (4,)))
    try:
        r.set_separate_passes(True)
        for precision in ("f16x3", "f16x1"):
            _check(r, _pose(), 2, 3, 16 / 255, 0.5, precision=precision)
    finally:
        r.close()


# ---- 6. the modes and the reports -----------------------------------------------------------------------------------------------

def _raw_call(r, out, k=2, levels=2, precision=_lib.PREC_F16X3):
    cam = _camera(H, W)
    pose = _pose()
    return r._lib.nwe_render_adaptive_levels(r._ctx, pose.ctypes.data, 1, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], NEAR, FAR, 0, H, precision,
                                             k, levels, 0.05, 0.05, C.byref(out), torch.cuda.current_stream().cuda_stream)


def test_the_other_modes_refuse_the_call_in_nwe_render_rays_words():
    r = _renderer()
    try:
        rays = r.create_rays(_pose(), 2, 2, **_camera(2, 2))
        bufs = {name: torch.full((H * W * n,), 123.0, device=r.device) for name, n in (("rgb", 3), ("depth", 1), ("acc", 1))}
        maps = {name: torch.full((H * W,), 9, dtype=torch.uint8, device=r.device) for name in ("kind", "level")}
        flags = torch.zeros(1, dtype=torch.int32, device=r.device)
        out = _lib.AdaptiveLevelsOutputs(flags=flags.data_ptr(), **{name: t.data_ptr() for name, t in {**bufs, **maps}.items()})
        assert _raw_call(r, out) == _lib.NWE_OK                     # the call runs while no mode is on ...
        torch.cuda.synchronize()
        ran = r.last_adaptive_levels()
        assert not (bufs["rgb"] == 123.0).any() and int(maps["kind"].max()) <= 2 and int(maps["level"].max()) <= 2
        for t in bufs.values():
            t.fill_(123.0)
        for t in maps.values():
            t.fill_(9)
        box = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))
        modes = ((lambda: r.set_early_termination(0.01), lambda: r.set_early_termination(0.0), "early termination"),
                 (lambda: r.set_shared_coarse(2), lambda: r.set_shared_coarse(1), "the shared coarse pass"),
                 (lambda: r.set_occupancy(np.ones((4, 4, 4), bool), *box, 4), r.clear_occupancy, "an occupancy grid"),
                 (lambda: r.set_coarse_grid(np.zeros((4, 4, 4), np.float32), *box), r.clear_coarse_grid, "a coarse density grid"))
        for on, off, name in modes:
            on()
            with pytest.raises(NotImplementedError) as of_rays:
                r.render_rays(rays, outputs=("rgb",))
            text = str(of_rays.value).split(": ", 1)[1]
            assert text.startswith(name)
            assert _raw_call(r, out) == _lib.NWE_ERR_UNSUPPORTED and r._lib.nwe_last_error(r._ctx).decode() == text
            with pytest.raises(NotImplementedError) as of_call:
                r.render_adaptive(_pose(), H, W, levels=2, **_camera(H, W))
            assert str(of_call.value) == "nwe_render_adaptive_levels: " + text
            off()
        assert _raw_call(r, out, k=33) == _lib.NWE_ERR_INVALID and _raw_call(r, out, levels=5) == _lib.NWE_ERR_INVALID
        torch.cuda.synchronize()
        assert all(bool((t == 123.0).all()) for t in bufs.values()) and all(bool((t == 9).all()) for t in maps.values()) and int(flags.item()) == 0
        assert r.last_adaptive_levels() == ran                      # ... and a refused call moves no report
        _check(r, _pose(), 2, 2, 0.05, 0.05)                        # the modes are off again
    finally:
        r.close()


def test_the_reports():
    """Neither adaptive call moves the other's report; the render reports describe the last render launch made; the cap of the
    report call."""
    r = _renderer()
    try:
        poses = _pose()
        assert r.last_adaptive_levels() is None and r.last_adaptive() is None
        got = _levels(r, poses, k=2, levels=3, tol_rgb=16 / 255, tol_depth=0.5)
        report = got[4]
        assert r.last_adaptive() is None                            # nwe_last_adaptive is not moved
        assert report["rendered"][-1] > 0 and r.last_ray_evaluations() == (report["rendered"][-1] * (2 * NS + NI),) * 2
        assert [int((got[2][got[1] == A.KIND_RENDERED] == i + 1).sum()) for i in range(3)] == report["rendered"]
        assert [int((got[2][got[1] == A.KIND_INTERPOLATED] == i).sum()) for i in range(3)] == report["interpolated"]
        before = r.last_adaptive_levels()
        r.render_adaptive(poses, H, W, k=2, tol_rgb=16 / 255, tol_depth=0.5, **_camera(H, W))
        assert r.last_adaptive()["pixels"] == H * W and r.last_adaptive_levels() == before      # ... nor this report by that call
        out, ms = (C.c_int64 * 12)(*([-7] * 12)), C.c_float(-7.0)
        assert r._lib.nwe_last_adaptive_levels(r._ctx, out, 9, C.byref(ms)) == _lib.NWE_ERR_INVALID and tuple(out) == (-7,) * 12
        assert r._lib.nwe_last_adaptive_levels(r._ctx, out, 10, None) == _lib.NWE_OK
        assert list(out[:10]) == [H * W, report["lattice"], 3, report["render_launches"]] + report["rendered"] + report["interpolated"]
        assert tuple(out[10:]) == (-7, -7)
        _levels(r, poses, k=2, levels=1, tol_rgb=INF, tol_depth=INF)                            # a shorter report replaces it
        assert r.last_adaptive_levels()["levels"] == 1 and r.last_adaptive_levels()["render_launches"] == 1
    finally:
        r.close()


# ---- 7. the handler -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by", ["argument", "environment"])
def test_the_handler_draws_its_frame_through_the_multi_level_call(by, monkeypatch):
    opt = {"k": 2, "tol_rgb": 0.02, "tol_depth": 0.1}
    for name in ("NWE_ADAPTIVE", "NWE_ADAPTIVE_LEVELS", "NWE_ADAPTIVE_LISTS"):
        monkeypatch.delenv(name, raising=False)
    if by == "environment":
        monkeypatch.setenv("NWE_ADAPTIVE_LEVELS", "3")
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3", adaptive=opt, **({"adaptive_levels": 3} if by == "argument" else {}))
    h.set_sampling(NS, NI)
    sd = _room()
    h.initialize_models(state_dicts=(sd, sd))
    try:
        assert h.last_adaptive_levels() is None
        init, coord = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
        img = h.render_coordinates(init, coord)
        Hh, Wh = h.image_size
        rep = h.last_adaptive_levels()
        assert h.last_adaptive() is None and rep["levels"] == 3 and rep["pixels"] == Hh * Wh
        assert rep["lattice"] == len(A.lattice(0, Hh, 8)) * len(A.lattice(0, Wh, 8))
        assert rep["lattice"] + sum(rep["rendered"]) + sum(rep["interpolated"]) == rep["pixels"] and sum(rep["interpolated"]) > 0
        pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [coord])
        cam = dict(zip(("fx", "fy", "cx", "cy"), pinhole_intrinsics(Hh, Wh)))
        near, far = h._depth_close_bound, h._depth_far_bound
        want = h.renderer.to8b(h.renderer.render_adaptive(pose.numpy(), Hh, Wh, near=near, far=far, levels=3, **cam, **opt)["rgb"]).cpu().numpy()
        assert img.shape == (Hh, Wh, 3) and img.dtype == np.uint8 and np.array_equal(img, want.reshape(Hh, Wh, 3))
        # levels= on the handler's own calls: None is the one-level call, an integer the multi-level one
        one = h.render_adaptive(pose.numpy()[0], 9, 11, outputs=("rgb", "kind"), **opt)
        assert h.last_adaptive()["pixels"] == 99 and h.last_adaptive_levels()["pixels"] == Hh * Wh
        two = h.render_adaptive(pose.numpy()[0], 9, 11, outputs=("rgb", "kind", "level"), levels=1, **opt)
        assert h.last_adaptive_levels()["pixels"] == 99 and tuple(two["level"].shape) == (9, 11)
        assert torch.equal(one["rgb"], two["rgb"]) and torch.equal(one["kind"], two["kind"])
        batch = h.render_adaptive_batch(pose.numpy(), 9, 11, outputs=("rgb", "level"), levels=2, **opt)
        assert tuple(batch["rgb"].shape) == (1, 9, 11, 3) and h.last_adaptive_levels()["levels"] == 2
    finally:
        h.renderer.close()
