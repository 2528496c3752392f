"""The pixel list on the GPU (include/nwe.h: nwe_render_pixels; the kernels: csrc/nwe_mfma_render.h, render_mfma_list_kernel) and the
adaptive frame on it (nwe_set_adaptive_pixel_lists).

The reference of every comparison is the frame nwe_render draws on the same context, gathered at the list - never the call under
test.  Everything is compared bit for bit ("same bits" lets a NaN equal a NaN whatever its sign and payload).
The shapes are those of tests/test_gpu_adaptive.py: the 4 x 128 network with 16 + 16 samples, the room scene of nwe_amd.synthetic,
frames of 37 x 45 - 1665 pixels a pose: 13 workgroups of four packets and a ragged last packet of one ray, 53 of one packet."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler
from oracle import nerf_oracle as O
from tests import lean_domain as L

pytestmark = pytest.mark.gpu

H, W = 37, 45
N = H * W
NS, NI = 16, 16
NEAR, FAR = 0.1, 8.0
ALL = ("rgb", "depth", "acc")
MASK = _lib.FLAG_RGB | _lib.FLAG_DEPTH | _lib.FLAG_ACC
MFMA = ("f16x3", "f16x1")


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


def _camera(h, w, near=NEAR, far=FAR):
    fx, fy, cx, cy = O.intrinsics(h, w)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=near, far=far)


def _renderer(sd_c=None, sd_f=None, ns=NS, ni=NI, fold=True):
    sd_c = _room() if sd_c is None else sd_c
    r = nwe_amd.Renderer(0)
    r.debug_set_fold(fold)
    r.set_network(0, sd_c); r.set_network(1, sd_c if sd_f is None else sd_f)
    r.set_sampling(ns, ni)
    return r


def _full(r, poses, h=H, w=W, rows=None, precision="f16x3", cam=None):
    """nwe_render's frame [rays, 5] (r, g, b, depth, acc) and its rgb / depth / acc flag bits."""
    out = r.render(poses, h, w, rows=rows, precision=precision, outputs=ALL, **(cam or _camera(h, w)))
    frame = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy()
    return frame, int(out["flags"].item()) & MASK


def _dev(r, pixels):
    return torch.as_tensor(np.asarray(pixels, dtype=np.int64).astype(np.int32), device=r.device)


def _pixels(r, poses, pixels, h=H, w=W, rows=None, precision="f16x3", cam=None):
    """The call under test: [n, 5] and the flag word."""
    out = r.render_pixels(poses, h, w, _dev(r, pixels), rows=rows, precision=precision, outputs=ALL, **(cam or _camera(h, w)))
    got = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy()
    return got, int(out["flags"].item())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _path(precision):
    return "rays" if precision == "f32" else "list"


def _perm(n, seed=11):
    return np.random.default_rng(seed).permutation(n)


# ---- 1. the identity list -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f16x1", "f32"])
def test_the_identity_list_is_the_frame(precision):
    r = _renderer()
    try:
        for poses, rows in ((_pose(), None), (_pose(), (5, 29)), (_two_poses(), None)):
            full, full_flags = _full(r, poses, rows=rows, precision=precision)
            assert np.isfinite(full).all() and float(np.ptp(full[:, :3])) > 0.05          # a frame with something in it
            got, flags = _pixels(r, poses, np.arange(len(full)), rows=rows, precision=precision)
            assert _same_bits(got, full), (precision, rows, len(poses))
            assert flags == full_flags
            assert r.last_pixels() == {"n": len(full), "path": _path(precision)}
            # an ordinary launch on the render ring: its reports describe it
            evals = len(full) * (2 * NS + NI)
            assert r.last_ray_evaluations() == (evals, evals) and r.last_kernel_ms() > 0.0
    finally:
        r.close()


# ---- 2. packet and workgroup edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", MFMA)
def test_lengths_around_a_packet_and_a_workgroup_under_every_plan(precision):
    r = _renderer()
    try:
        full, _ = _full(r, _pose(), precision=precision)
        perm = _perm(N)
        for n in (1, 31, 32, 33, 127, 128, 129, N):
            want = full[perm[:n]]
            for decomposition, queues in ((0, (-1,)), (1, (-1,)), (2, (0, 1))):
                r.debug_set_decomposition(decomposition)
                for queue in queues:
                    r.debug_set_work_queue(queue)
                    got, _ = _pixels(r, _pose(), perm[:n], precision=precision)
                    ctx = (precision, n, decomposition, queue)
                    assert _same_bits(got, want), ctx
                    assert r.debug_last_plan() == decomposition and r.last_pixels() == {"n": n, "path": "list"}, ctx
                    grid = r.debug_last_queue()["grid"]
                    if queue == 0:
                        assert grid == (0, 0), ctx
                    elif queue == 1:                       # every launch that has rays takes tickets
                        cus = torch.cuda.get_device_properties(0).multi_processor_count
                        first = n // 128 // cus * cus * 128     # the hybrid plan: whole rounds of packets, then the split rest
                        assert (grid[0] > 0) == (first > 0) and (grid[1] > 0) == (n > first), (ctx, grid)
            r.debug_set_decomposition(-1); r.debug_set_work_queue(-1)
    finally:
        r.close()


# ---- 3. order and out-of-range values -------------------------------------------------------------------------------------------

def test_order_duplicates_and_values_outside_the_frame():
    r = _renderer()
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            for poses in (_pose(), _two_poses()):
                full, _ = _full(r, poses, precision=precision)
                n = len(full)
                lists = {"reversed": np.arange(n)[::-1], "twice": np.repeat(np.arange(n), 2),
                         "outside": np.array([-1, n, 2**31 - 1, -2**31, 0, n - 1, 7, n // 2, -5, n + 5, 1000], dtype=np.int64)}
                for name, px in lists.items():
                    got, _ = _pixels(r, poses, px, precision=precision)
                    want = full[np.clip(px, 0, n - 1)]
                    assert _same_bits(got, want), (precision, len(poses), name)
                    assert r.last_pixels() == {"n": len(px), "path": _path(precision)}
                # ... which is what the list of the clamped values gives
                clamped, _ = _pixels(r, poses, np.clip(lists["outside"], 0, n - 1), precision=precision)
                assert _same_bits(clamped, full[np.clip(lists["outside"], 0, n - 1)])
    finally:
        r.close()


# ---- 4. every shape and formulation ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,Wn,form", L.SHAPES, ids=L.IDS)
def test_every_shape_with_list_kernels(D, Wn, form):
    """Every shape of csrc/nwe_mfma_shapes.h in the formulation tests/lean_domain.py packs it in (debug_set_fold): the list kernels
    exist for the product formulations, and the library says so; the reference formulation goes through a ray table."""
    h, w, n = 16, 24, 200
    r = nwe_amd.Renderer(0)
    try:
        r.debug_set_fold(L.fold(form))
        sd_c, sd_f = L.nets(D, Wn, form)
        r.set_network(0, sd_c); r.set_network(1, sd_f)
        r.set_sampling(8, 8)
        built = form != "reference"
        px = _perm(h * w, seed=D * 1000 + Wn)[:n]
        cam = L.camera(h, w)
        for precision in MFMA:
            assert r.pixels_path(precision) == ("list" if built else "rays")
            full, full_flags = _full(r, L.pose()[None], h, w, precision=precision, cam=cam)
            got, flags = _pixels(r, L.pose()[None], px, h, w, precision=precision, cam=cam)
            assert _same_bits(got, full[px]), (D, Wn, form, precision)
            assert flags & ~MASK == 0 and flags | full_flags == full_flags
            assert r.last_pixels() == {"n": n, "path": "list" if built else "rays"}
    finally:
        r.close()


# ---- 5. other settings ----------------------------------------------------------------------------------------------------------

def test_the_white_background_and_the_hollow_path():
    r = _renderer()
    try:
        px = _perm(N, seed=5)[:700]
        plain, _ = _full(r, _pose())
        r.set_white_background(True)
        white, _ = _full(r, _pose())
        assert not _same_bits(white, plain)
        assert _same_bits(_pixels(r, _pose(), px)[0], white[px])
        r.set_white_background(False)
        # the room has an empty interior: with the hollow path allowed (1, the default; 2: whatever the weights hold) and without
        # it (0) the bits are the frame's, which do not depend on it either
        for precision in MFMA:
            frames = []
            for mode in (0, 1, 2):
                r.debug_set_colour_skip(mode)
                full, _ = _full(r, _pose(), precision=precision)
                assert _same_bits(_pixels(r, _pose(), px, precision=precision)[0], full[px]), (precision, mode)
                assert r.last_pixels()["path"] == "list"
                frames.append(full)
            assert _same_bits(frames[0], frames[1]) and _same_bits(frames[0], frames[2])
            r.debug_set_colour_skip(1)
    finally:
        r.close()


def test_separate_passes_and_unfolded_networks_go_through_a_ray_table():
    px = _perm(N, seed=6)[:333]
    r = _renderer()
    try:
        r.set_separate_passes(True)
        for precision in ("f16x3", "f16x1", "f32"):
            full, full_flags = _full(r, _pose(), precision=precision)
            got, flags = _pixels(r, _pose(), px, precision=precision)
            assert _same_bits(got, full[px]) and flags == full_flags and r.last_pixels() == {"n": 333, "path": "rays"}, precision
        r.set_separate_passes(False)
        assert _pixels(r, _pose(), px)[1] == 0 and r.last_pixels()["path"] == "list"
    finally:
        r.close()
    r = _renderer(fold=False)
    try:
        for precision in MFMA:
            full, _ = _full(r, _pose(), precision=precision)
            got, _ = _pixels(r, _pose(), px, precision=precision)
            assert _same_bits(got, full[px]) and r.last_pixels() == {"n": 333, "path": "rays"}, precision
    finally:
        r.close()


# ---- 6. flags -------------------------------------------------------------------------------------------------------------------

def test_only_the_rgb_depth_and_acc_bits_are_reported():
    px = _perm(N, seed=8)[:500]
    # a fine network whose colour layers hold a NaN: every colour is NaN, depth and acc are finite
    sd_f = _room()
    sd_f["_rgb_linear.bias"] = np.full_like(sd_f["_rgb_linear.bias"], np.nan)
    r = _renderer(sd_f=sd_f)
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            full, full_flags = _full(r, _pose(), precision=precision)
            assert np.isnan(full[:, :3]).all() and np.isfinite(full[:, 3:]).all() and full_flags == _lib.FLAG_RGB
            got, flags = _pixels(r, _pose(), px, precision=precision)
            assert _same_bits(got, full[px]) and flags == _lib.FLAG_RGB == full_flags, precision
    finally:
        r.close()
    # a coarse network with NaN colour weights and a finite density: its colour reaches no output of the call, and no coarse bit the
    # flag word - on the list kernels, whose coarse pass is density only, and through a ray table, whose coarse pass computes it
    sd_c = _room()
    sd_c["_rgb_linear.weight"] = np.full_like(sd_c["_rgb_linear.weight"], np.nan)
    r = _renderer(sd_c=sd_c, sd_f=_room())
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            whole = r.render(_pose(), H, W, precision=precision, outputs=ALL, **_camera(H, W))
            full, full_flags = _full(r, _pose(), precision=precision)
            assert np.isfinite(full).all() and full_flags == 0
            got, flags = _pixels(r, _pose(), px, precision=precision)
            assert _same_bits(got, full[px]) and flags == 0 == int(whole["flags"].item()) & MASK, precision
        r.set_separate_passes(True)                       # the ray table under an MFMA precision: the full kernels' coarse launch
        rays = r.create_rays(_pose(), 4, 5, **_camera(4, 5))
        assert int(r.render_rays(rays, outputs=("rgb", "rgb_coarse"))["flags"].item()) & ~MASK != 0     # there is a coarse bit to mask
        full, full_flags = _full(r, _pose())
        got, flags = _pixels(r, _pose(), px)
        assert _same_bits(got, full[px]) and flags == 0 == full_flags and r.last_pixels()["path"] == "rays"
    finally:
        r.close()


# ---- 7. refusals on the device --------------------------------------------------------------------------------------------------

def _raw_call(r, out, pixels, n, precision=_lib.PREC_F16X3):
    cam = _camera(H, W)
    pose = _pose()
    return r._lib.nwe_render_pixels(r._ctx, pose.ctypes.data, 1, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], NEAR, FAR, 0, H,
                                    pixels.data_ptr(), n, precision, C.byref(out), torch.cuda.current_stream().cuda_stream)


def test_the_other_modes_refuse_the_call_in_nwe_render_rays_words():
    r = _renderer()
    try:
        rays = r.create_rays(_pose(), 2, 2, **_camera(2, 2))
        n = 300
        px = _dev(r, _perm(N, seed=9)[:n])
        bufs = {name: torch.full((n * k,), 123.0, device=r.device) for name, k in (("rgb", 3), ("depth", 1), ("acc", 1))}
        flags = torch.zeros(1, dtype=torch.int32, device=r.device)
        out = _lib.PixelOutputs(rgb=bufs["rgb"].data_ptr(), depth=bufs["depth"].data_ptr(), acc=bufs["acc"].data_ptr(), flags=flags.data_ptr())
        assert _raw_call(r, out, px, n) == _lib.NWE_OK              # the call runs while no mode is on ...
        torch.cuda.synchronize()
        assert not (bufs["rgb"] == 123.0).any() and r.last_pixels() == {"n": n, "path": "list"}
        ran_ms, ran_evals = r.last_kernel_ms(), r.last_ray_evaluations()
        assert ran_ms > 0.0 and ran_evals == (n * (2 * NS + NI),) * 2
        for b in bufs.values():
            b.fill_(123.0)
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
            for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
                assert _raw_call(r, out, px, n, precision) == _lib.NWE_ERR_UNSUPPORTED, name
                if precision == _lib.PREC_F16X3:
                    assert r._lib.nwe_last_error(r._ctx).decode() == text
            with pytest.raises(NotImplementedError) as of_call:
                r.render_pixels(_pose(), H, W, px, **_camera(H, W))
            assert str(of_call.value) == "nwe_render_pixels: " + text
            off()
        # no pixels: NWE_OK, nothing launched
        assert _raw_call(r, out, px, 0) == _lib.NWE_OK
        assert r.render_pixels(_pose(), H, W, px[:0], **_camera(H, W))["rgb"].shape == (0, 3)
        torch.cuda.synchronize()
        assert all(bool((b == 123.0).all()) for b in bufs.values()) and int(flags.item()) == 0
        # ... and neither a refused call nor an empty one moves a report
        assert r.last_kernel_ms() == ran_ms and r.last_ray_evaluations() == ran_evals and r.last_pixels() == {"n": n, "path": "list"}
    finally:
        r.close()


# ---- 8. asynchrony --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_six_calls_back_to_back_keep_their_own_lists(precision):
    """Six calls on one stream with nothing between them: the ring has four slots, so the fifth waits for the first - and every
    call still reads its own list, poses and, on the ray-table path, its own slot's table."""
    r = _renderer()
    try:
        full = [_full(r, p, precision=precision)[0] for p in (_pose(), _pose(-0.5, 0.6, 0.2))]
        lists = [_perm(N, seed=20 + i)[:n] for i, n in enumerate((700, 33, N, 128, 1, 900))]
        torch.cuda.synchronize()
        outs = []
        for i, px in enumerate(lists):
            pose = (_pose(), _pose(-0.5, 0.6, 0.2))[i % 2]
            outs.append(r.render_pixels(pose, H, W, _dev(r, px), precision=precision, outputs=ALL, **_camera(H, W)))
        torch.cuda.synchronize()
        for i, (px, out) in enumerate(zip(lists, outs)):
            got = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy()
            assert _same_bits(got, full[i % 2][px]), (precision, i)
        assert r.last_pixels() == {"n": 900, "path": _path(precision)}
    finally:
        r.close()


# ---- 9. the adaptive switch -----------------------------------------------------------------------------------------------------

def _adaptive(r, precision, k, tol_rgb, tol_depth):
    out = r.render_adaptive(_two_poses(), H, W, precision=precision, outputs=ALL + ("kind",), k=k, tol_rgb=tol_rgb, tol_depth=tol_depth,
                            **_camera(H, W))
    frame = torch.cat([out["rgb"], out["depth"][:, None], out["acc"][:, None]], 1).cpu().numpy()
    rep = r.last_adaptive()
    return frame, out["kind"].cpu().numpy(), int(out["flags"].item()), {key: rep[key] for key in ("pixels", "lattice", "rendered", "interpolated")}


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_the_adaptive_frame_is_the_same_with_the_switch_on_and_off(precision):
    r = _renderer()
    try:
        full, _ = _full(r, _two_poses(), precision=precision)
        for k in (2, 3):
            for tol_rgb, tol_depth in ((2 / 255, 0.05), (-1.0, -1.0)):
                r.set_adaptive_pixel_lists(False)
                off = _adaptive(r, precision, k, tol_rgb, tol_depth)
                before = r.last_pixels()
                r.set_adaptive_pixel_lists(True)
                on = _adaptive(r, precision, k, tol_rgb, tol_depth)
                ctx = (precision, k, tol_rgb)
                assert _same_bits(on[0], off[0]) and np.array_equal(on[1], off[1]) and on[2:] == off[2:], ctx
                if tol_rgb < 0:                              # every pixel rendered: nwe_render's frame, the reference of it all
                    assert _same_bits(on[0], full) and on[3]["interpolated"] == 0, ctx
                else:                                        # a second render launch was made (on this frame few cells are that flat)
                    assert on[3]["rendered"] > 0 and on[3]["lattice"] + on[3]["rendered"] + on[3]["interpolated"] == 2 * N, ctx
                if precision == "f16x3":                     # the second render launch was the last one
                    assert r.last_pixels() == {"n": on[3]["rendered"], "path": "list"}, ctx
                    assert r.last_ray_evaluations() == (on[3]["rendered"] * (2 * NS + NI),) * 2
                else:                                        # not eligible: the call runs as without the switch
                    assert r.last_pixels() == before, ctx
        r.set_adaptive_pixel_lists(False)
    finally:
        r.close()


# ---- 10. the handler ------------------------------------------------------------------------------------------------------------

def test_the_handler_renders_regions_and_pixel_lists():
    h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3")
    h.set_sampling(NS, NI)
    sd = _room()
    h.initialize_models(state_dicts=(sd, sd))
    try:
        init, coord = nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)
        img = h.render_coordinates(init, coord)
        Hh, Wh = h.image_size
        for top, left, height, width in ((0, 0, Hh, Wh), (3, 5, 17, 31), (Hh - 1, Wh - 1, 1, 1), (0, Wh - 9, Hh, 9)):
            region = h.render_region(init, coord, top, left, height, width)
            assert region.dtype == np.uint8 and region.shape == (height, width, 3) and region.flags.c_contiguous
            assert np.array_equal(region, img[top:top + height, left:left + width]), (top, left, height, width)
            assert h.renderer.last_pixels() == {"n": height * width, "path": "list"}
        with pytest.raises(ValueError, match="the region must be"):
            h.render_region(init, coord, 0, 0, Hh + 1, 4)
        pose = nwe_amd.get_camera_poses_from_list_of_coordinates(init, [coord])
        frame = h.render(pose.numpy()[0], outputs=("rgb",))["rgb"].reshape(-1, 3).cpu().numpy()
        px = _perm(Hh * Wh, seed=4)[:1000]
        got = h.render_pixels(init, coord, px.astype(np.int32))
        assert got.shape == (1000, 3) and got.dtype == torch.float32 and _same_bits(got.cpu().numpy(), frame[px])
        assert np.array_equal(h.render_coordinates(init, coord), img)          # the frame's staging buffer is the frame's again
    finally:
        h.renderer.close()


def test_the_handlers_switch(monkeypatch):
    monkeypatch.delenv("NWE_ADAPTIVE", raising=False)
    monkeypatch.setenv("NWE_ADAPTIVE_LISTS", "1")
    opt = {"k": 3, "tol_rgb": 0.02, "tol_depth": 0.1}
    sd = _room()
    imgs = []
    for lists in (False, None):                 # the argument switches it off, the environment on
        h = NeRFReplicaInferenceHandler("office_tokyo", "unused", precision="f16x3", adaptive=opt, adaptive_lists=lists)
        h.set_sampling(NS, NI)
        h.initialize_models(state_dicts=(sd, sd))
        try:
            assert h.renderer.adaptive_pixel_lists is (lists is None)
            imgs.append(h.render_coordinates(nwe_amd.COORD(x=0.0, y=-0.5, z=-0.76, pitch=-90.0), nwe_amd.COORD(yaw=-30.0)))
            last = h.renderer.last_pixels()
            rep = h.last_adaptive()             # the last render launch: the kind 1 pixels', or the lattice's where there are none
            assert (last is None) if lists is False else (last["path"] == "list" and last["n"] == (rep["rendered"] or rep["lattice"]) > 0)
        finally:
            h.renderer.close()
    assert np.array_equal(imgs[0], imgs[1])
