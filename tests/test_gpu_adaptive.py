"""The adaptive frame on the GPU (include/nwe.h: nwe_render_adaptive; the kernels: csrc/nwe_adaptive.hip).

The reference of every comparison is the frame nwe_render draws on the same context, and the numpy restatement of the rule
(tests/adaptive.py) applied to that frame - never the call under test.  Everything is compared bit for bit ("bit for bit" lets a
NaN equal a NaN whatever its sign and payload): a rendered pixel has nwe_render's bits, an interpolated one those of three
separately rounded fp32 operations per step.
The shapes: the 4 x 128 network with 16 + 16 samples, the room scene of nwe_amd.synthetic, frames of 37 x 45 - 36 is a multiple of
2, 3 and 4 but not of 5, 44 of 2 and 4 but not of 3 and 5, so the last lattice row and column both coincide with a multiple of k
and stand extra - which is 1665 pixels a pose, more than one scan tile of 1024."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler, pinhole_intrinsics
from oracle import nerf_oracle as O
from tests import adaptive as A

pytestmark = pytest.mark.gpu

H, W = 37, 45
NS, NI = 16, 16
NEAR, FAR = 0.1, 8.0
ALL = ("rgb", "depth", "acc", "kind")
MASK = A.FLAG_RGB | A.FLAG_DEPTH | A.FLAG_ACC
INF = float("inf")


def _pose(x=0.3, y=-0.2, z=0.1):
    p = np.eye(4, dtype=np.float32)
    p[:3, 3] = (x, y, z)
    return p[None]


def _room(seed=7, D=4, Wn=128, skips=()):
    return synthetic.room(synthetic.make_state_dict(seed, D, Wn, skips=skips))


def _camera(h, w):
    fx, fy, cx, cy = O.intrinsics(h, w)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def _renderer(sd_c=None, sd_f=None, ns=NS, ni=NI):
    sd_c = _room() if sd_c is None else sd_c
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_c if sd_f is None else sd_f)
    r.set_sampling(ns, ni)
    return r


def _full(r, poses, h=H, w=W, rows=None, precision="f16x3"):
    """nwe_render's frame [P, rows, w, 5] (r, g, b, depth, acc) and its rgb / depth / acc flag bits."""
    out = r.render(poses, h, w, rows=rows, precision=precision, outputs=("rgb", "depth", "acc"), **_camera(h, w))
    r0, r1 = rows or (0, h)
    frame = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy().reshape(len(poses), r1 - r0, w, 5)
    return frame, int(out["flags"].item()) & MASK


def _adaptive(r, poses, h=H, w=W, rows=None, precision="f16x3", **kw):
    out = r.render_adaptive(poses, h, w, rows=rows, precision=precision, outputs=ALL, **_camera(h, w), **kw)
    r0, r1 = rows or (0, h)
    frame = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy().reshape(len(poses), r1 - r0, w, 5)
    return frame, out["kind"].cpu().numpy().reshape(len(poses), r1 - r0, w), int(out["flags"].item())


def _want(full, first_row, k, tol_rgb, tol_depth):
    """The restatement on every pose of nwe_render's frame: frame, kinds, counts of the call, the interpolation's flag bits."""
    parts = [A.apply(f, first_row, k, tol_rgb, tol_depth) for f in full]
    frame, kind = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    counts = {key: sum(p[2][key] for p in parts) for key in parts[0][2]}
    flags = 0
    for out, kd, _ in parts:
        flags |= A.interpolation_flags(out, kd)
    return frame, kind, counts, flags


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _counts(r):
    rep = r.last_adaptive()
    assert rep["ms"] > 0.0
    return {key: rep[key] for key in ("pixels", "lattice", "rendered", "interpolated")}


def _check(r, poses, k, tol_rgb, tol_depth, h=H, w=W, rows=None, precision="f16x3", ctx=None):
    """One call against the restatement on the context's own nwe_render frame; returns the restatement's counts."""
    full, full_flags = _full(r, poses, h, w, rows, precision)
    got, kind, flags = _adaptive(r, poses, h, w, rows, precision, k=k, tol_rgb=tol_rgb, tol_depth=tol_depth)
    want, want_kind, counts, interp_flags = _want(full, (rows or (0, h))[0], k, tol_rgb, tol_depth)
    ctx = (ctx, h, w, rows, precision, k, tol_rgb)
    assert np.array_equal(kind, want_kind), ctx
    assert _same_bits(got, want), ctx
    assert _counts(r) == counts, ctx
    assert flags == full_flags | interp_flags, ctx
    return counts


# ---- 1. the exact regime --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_a_negative_tolerance_renders_every_pixel_with_nwe_renders_bits(precision):
    r = _renderer()
    try:
        poses = _pose()
        full, full_flags = _full(r, poses, precision=precision)
        assert np.isfinite(full).all() and float(np.ptp(full[..., :3])) > 0.05          # a frame with something in it
        for k in (1, 2, 3, 5):
            got, kind, flags = _adaptive(r, poses, precision=precision, k=k, tol_rgb=-1.0, tol_depth=-1.0)
            assert _same_bits(got, full), (precision, k)
            assert flags == full_flags and not (kind == A.KIND_INTERPOLATED).any()
            n_lattice = len(A.lattice(0, H, k)) * len(A.lattice(0, W, k))
            assert int((kind == A.KIND_LATTICE).sum()) == n_lattice
            assert _counts(r) == {"pixels": H * W, "lattice": n_lattice, "rendered": H * W - n_lattice, "interpolated": 0}
    finally:
        r.close()


# ---- 2. the general regime ------------------------------------------------------------------------------------------------------

def test_the_frame_the_kinds_and_the_counts_are_the_restatements():
    r = _renderer()
    try:
        for k in (2, 3, 5, 16, 64):                      # 64 exceeds both edges: the lattice is the four corners
            counts = _check(r, _pose(), k, 0.05, 0.05)
            rest = counts["pixels"] - counts["lattice"]
            print(f"k = {k}: lattice {counts['lattice']}, rendered {counts['rendered']} ({counts['rendered'] / rest:.0%}), "
                  f"interpolated {counts['interpolated']} ({counts['interpolated'] / rest:.0%}) of {rest}")
            if k in (2, 3):      # the condition of the case, on the restatement's output: both regimes are well populated
                assert counts["rendered"] >= 0.1 * rest and counts["interpolated"] >= 0.1 * rest, (k, counts)
        assert _counts(r)["lattice"] == 4
    finally:
        r.close()


# ---- 3. the all-flat regime -----------------------------------------------------------------------------------------------------

def test_an_infinite_tolerance_makes_one_render_launch():
    r = _renderer()
    try:
        for k in (2, 5):
            counts = _check(r, _pose(), k, INF, INF)
            assert counts["rendered"] == 0 and counts["interpolated"] == H * W - counts["lattice"]
            # the last render launch made is the lattice's, and there was no other
            assert r.last_ray_evaluations() == (counts["lattice"] * (2 * NS + NI),) * 2
    finally:
        r.close()


def test_a_nan_colour_makes_every_cell_busy():
    sd_f = _room()
    sd_f["_rgb_linear.bias"] = np.full_like(sd_f["_rgb_linear.bias"], np.nan)
    r = _renderer(sd_f=sd_f)
    try:
        poses = _pose()
        full, full_flags = _full(r, poses)
        assert np.isnan(full[..., :3]).all() and np.isfinite(full[..., 3:]).all() and full_flags == A.FLAG_RGB
        for k in (2, 3):
            got, kind, flags = _adaptive(r, poses, k=k, tol_rgb=INF, tol_depth=INF)
            assert not (kind == A.KIND_INTERPOLATED).any() and flags == full_flags
            assert np.array_equal(np.isnan(got), np.isnan(full)) and _same_bits(got, full)
            assert _counts(r)["rendered"] == H * W - _counts(r)["lattice"]
    finally:
        r.close()


# ---- 4. shapes and calls --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(1, 45), (37, 1), (2, 2), (1, 1)])
def test_degenerate_frames(h, w):
    r = _renderer()
    try:
        for k in (1, 2, 3, 64):
            for tol in (-1.0, 0.05, INF):
                _check(r, _pose(), k, tol, tol, h=h, w=w)
    finally:
        r.close()


def test_two_poses_are_two_single_pose_calls():
    r = _renderer()
    try:
        poses = np.concatenate([_pose(), _pose(-0.8, 0.4, -0.3)])
        poses[1, :3, :3] = O.camera_pose((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0, 0, 0, 40.0, 10.0, 0.0))[0, :3, :3].numpy()
        for k in (2, 3):
            both = _adaptive(r, poses, k=k, tol_rgb=0.05, tol_depth=0.05)
            both_counts = _counts(r)
            singles = [_adaptive(r, poses[i:i + 1], k=k, tol_rgb=0.05, tol_depth=0.05) + (_counts(r),) for i in range(2)]
            for i in range(2):
                assert _same_bits(both[0][i], singles[i][0][0]) and np.array_equal(both[1][i], singles[i][1][0]), (k, i)
            assert both[2] == singles[0][2] | singles[1][2]
            assert both_counts == {key: singles[0][3][key] + singles[1][3][key] for key in both_counts}
            assert not np.array_equal(both[1][0], both[1][1])           # two different views
            _check(r, poses, k, 0.05, 0.05)
    finally:
        r.close()


def test_a_row_tile_has_its_own_lattice():
    r = _renderer()
    try:
        for k in (2, 3, 5):
            _check(r, _pose(), k, 0.05, 0.05, rows=(5, 30))
            _check(r, np.concatenate([_pose(), _pose(0.0, 0.0, 0.0)]), k, 0.05, 0.05, rows=(36, 37))
    finally:
        r.close()


def test_networks_without_view_directions():
    sd = synthetic.room_output(synthetic.make_state_dict(7, 4, 128, skips=(), use_view_dirs=False))
    r = _renderer(sd_c=sd)
    try:
        assert r.ray_columns == 8
        for k, tol in ((2, 0.05), (3, -1.0), (5, INF)):
            _check(r, _pose(), k, tol, tol)
    finally:
        r.close()


def test_the_white_background_is_honoured():
    r = _renderer()
    try:
        plain = _full(r, _pose())[0]
        r.set_white_background(True)
        assert not _same_bits(_full(r, _pose())[0], plain)
        for k, tol in ((2, 0.05), (3, 0.05), (2, -1.0)):
            _check(r, _pose(), k, tol, tol)
    finally:
        r.close()


# ---- 5. the modes ---------------------------------------------------------------------------------------------------------------

def test_separate_passes_keep_two_shapes_on_the_mfma_kernels():
    r = _renderer(sd_c=_room(7, 4, 128, ()), sd_f=_room(8, 8, 256, (4,)))
    try:
        r.set_separate_passes(True)
        for precision in ("f16x3", "f16x1"):
            for k, tol in ((2, 0.05), (3, -1.0)):
                _check(r, _pose(), k, tol, tol, precision=precision)
    finally:
        r.close()


def _raw_call(r, out, k=2, precision=_lib.PREC_F16X3):
    cam = _camera(H, W)
    pose = _pose()
    return r._lib.nwe_render_adaptive(r._ctx, pose.ctypes.data, 1, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], NEAR, FAR, 0, H, precision, k,
                                      0.05, 0.05, C.byref(out), torch.cuda.current_stream().cuda_stream)


def test_the_other_modes_refuse_the_call_in_nwe_render_rays_words():
    r = _renderer()
    try:
        rays = r.create_rays(_pose(), 2, 2, **_camera(2, 2))
        bufs = {name: torch.full((H * W * n,), 123.0, device=r.device) for name, n in (("rgb", 3), ("depth", 1), ("acc", 1))}
        kind, flags = torch.full((H * W,), 9, dtype=torch.uint8, device=r.device), torch.zeros(1, dtype=torch.int32, device=r.device)
        out = _lib.AdaptiveOutputs(rgb=bufs["rgb"].data_ptr(), depth=bufs["depth"].data_ptr(), acc=bufs["acc"].data_ptr(), kind=kind.data_ptr(),
                                   flags=flags.data_ptr())
        assert _raw_call(r, out) == _lib.NWE_OK                     # the call runs while no mode is on ...
        torch.cuda.synchronize()
        ran = _counts(r)
        assert not (bufs["rgb"] == 123.0).any() and int(kind.max()) <= 2
        for b in bufs.values():
            b.fill_(123.0)
        kind.fill_(9)
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
                r.render_adaptive(_pose(), H, W, **_camera(H, W))
            assert str(of_call.value) == "nwe_render_adaptive: " + text
            off()
        torch.cuda.synchronize()
        assert all(bool((b == 123.0).all()) for b in bufs.values()) and bool((kind == 9).all()) and int(flags.item()) == 0
        assert _counts(r) == ran                                    # ... and a refused call moves no report
        _check(r, _pose(), 2, 0.05, 0.05)                           # the modes are off again
    finally:
        r.close()


def test_an_armed_hook_stays_armed():
    """The call neither uses nor clears the one-shot hooks: a coarse-weights hook armed in front of it serves the next
    nwe_render_rays, unlike a hook armed in front of a nwe_render_rays call, which that call consumes."""
    r = _renderer()
    try:
        rays = r.create_rays(_pose(), 4, 5, **_camera(4, 5))
        weights = torch.linspace(0.0, 1.0, 20 * NS, device=r.device).reshape(20, NS).contiguous()
        plain = r.render_rays(rays, outputs=("rgb",))["rgb"].cpu().numpy()
        hooked = r.render_rays(rays, outputs=("rgb",), debug_coarse_weights=weights)["rgb"].cpu().numpy()
        assert not _same_bits(plain, hooked)
        assert _same_bits(r.render_rays(rays, outputs=("rgb",))["rgb"].cpu().numpy(), plain)         # consumed
        r._lib.nwe_debug_set_coarse_weights(r._ctx, weights.data_ptr())
        _check(r, _pose(), 2, 0.05, 0.05)                                                           # not used ...
        assert _same_bits(r.render_rays(rays, outputs=("rgb",))["rgb"].cpu().numpy(), hooked)        # ... and not cleared
        assert _same_bits(r.render_rays(rays, outputs=("rgb",))["rgb"].cpu().numpy(), plain)
    finally:
        r.close()


# ---- 6. sequences ---------------------------------------------------------------------------------------------------------------

def test_a_long_lived_context_gives_the_bits_of_fresh_ones():
    """Growing, then shrinking calls with a changing k on one context - the scratch grows and is reused, the pixel list of a
    smaller call lies in front of a larger one's leftovers - with nwe_render and nwe_render_sparse calls in between."""
    steps = ((5, 9, 2, 0.05, 1), (20, 33, 5, 0.05, 1), (37, 45, 3, 0.05, 2), (37, 45, 2, INF, 1), (37, 45, 2, 0.02, 1), (12, 7, 4, 0.05, 2),
             (2, 2, 2, -1.0, 1), (37, 45, 64, 0.05, 1))
    rng = np.random.default_rng(3)
    grid = rng.uniform(-1.0, 1.0, (4, 5, 3, 4)).astype(np.float32)
    box = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))

    def poses_of(n):
        return np.concatenate([_pose(), _pose(-0.5, 0.6, 0.2)])[:n]

    def call(r, h, w, k, tol, n):
        got = _adaptive(r, poses_of(n), h, w, k=k, tol_rgb=tol, tol_depth=tol)
        return got + (_counts(r),)

    long_lived = _renderer()
    try:
        long_lived.set_radiance_grid(grid, *box)
        results = []
        for i, (h, w, k, tol, n) in enumerate(steps):
            results.append(call(long_lived, h, w, k, tol, n))
            if i % 2 == 0:
                long_lived.render(_pose(), 9, 11, outputs=("rgb",), **_camera(9, 11))
            else:
                long_lived.render_sparse(_pose(), 9, 11, outputs=("rgb",), **_camera(9, 11))
    finally:
        long_lived.close()
    for step, got in zip(steps, results):
        fresh = _renderer()
        try:
            want = call(fresh, *step)
        finally:
            fresh.close()
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], step


# ---- 7. the handler -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by", ["argument", "environment"])
def test_the_handler_draws_its_frame_through_the_adaptive_call(by, monkeypatch):
    opt = {"k": 3, "tol_rgb": 0.02, "tol_depth": 0.1}
    monkeypatch.delenv("NWE_ADAPTIVE", raising=False)
    if by == "environment":
        monkeypatch.setenv("NWE_ADAPTIVE", "3,0.02,0.1")
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3", **({"adaptive": opt} if by == "argument" else {}))
    h.set_sampling(NS, NI)
    sd = _room()
    h.initialize_models(state_dicts=(sd, sd))
    try:
        assert h.last_adaptive() is None
        init, coord = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
        img = h.render_coordinates(init, coord)
        Hh, Wh = h.image_size
        rep = h.last_adaptive()
        assert rep["pixels"] == Hh * Wh and rep["lattice"] == len(A.lattice(0, Hh, 3)) * len(A.lattice(0, Wh, 3))
        assert rep["lattice"] + rep["rendered"] + rep["interpolated"] == rep["pixels"] and rep["interpolated"] > 0
        pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [coord])
        cam = dict(zip(("fx", "fy", "cx", "cy"), pinhole_intrinsics(Hh, Wh)))
        near, far = h._depth_close_bound, h._depth_far_bound
        want = h.renderer.to8b(h.renderer.render_adaptive(pose.numpy(), Hh, Wh, near=near, far=far, **cam, **opt)["rgb"]).cpu().numpy()
        assert img.shape == (Hh, Wh, 3) and img.dtype == np.uint8 and np.array_equal(img, want.reshape(Hh, Wh, 3))
        assert h.last_adaptive()["rendered"] == rep["rendered"]
        # previews stay what they were: the coarse pass alone through nwe_render, no adaptive call
        before = h.last_adaptive()
        h.render_coordinates(init, coord, preview=True)
        assert h.last_adaptive() == before
    finally:
        h.renderer.close()
