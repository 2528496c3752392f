"""The pixel list without a GPU (include/nwe.h: nwe_render_pixels, nwe_set_adaptive_pixel_lists): every refusal on a host-only
context by code, text and order; the switch's domain; the path decision of the HIP-free code (csrc/nwe_check.cpp:
pixel_list_path, asked through nwe_debug_pixels_path as tests/test_adaptive_host.py asks the planner); the handler's option."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler as Handler

I, S, U = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE, _lib.NWE_ERR_UNSUPPORTED
SOMEWHERE = 1      # a pixel list "on the device": never read, every call here refuses or launches nothing


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _render_pixels(r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4),
                   pixels=SOMEWHERE, n=3, precision=_lib.PREC_F16X3):
    ptr = None if poses is None else poses.ctypes.data
    return _lib.load().nwe_render_pixels(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0], rows[1],
                                         pixels, n, precision, None if out is None else C.byref(out), None)


def _last(r):
    n, path = C.c_int64(-7), C.c_int(-7)
    return _lib.load().nwe_last_pixels(r._ctx, C.byref(n), C.byref(path)), n.value, path.value


def test_every_refusal_in_front_of_the_host_only_one():
    """Code, text and order: each call below is wrong in everything behind the refusal it expects as well."""
    r = nwe_amd.Renderer(host_only=True)
    bad = dict(n=-1, precision=9)                 # 4. and 5. wrong
    try:
        buf = np.full(60, 123.0, np.float32)
        flags = np.zeros(1, np.uint32)
        good = _lib.PixelOutputs(rgb=buf.ctypes.data, flags=flags.ctypes.data)
        stale = _lib.PixelOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.PixelOutputs) - 8
        # 1. the context - whatever else is wrong
        assert _render_pixels(None, None, poses=None, **bad) == I
        # 2. the outputs, in front of the camera (H = 0)
        assert _render_pixels(r, None, H=0, **bad) == I and _error(r) == "null outputs"
        assert _render_pixels(r, stale, H=0, **bad) == I and _error(r).startswith("nwe_pixel_outputs.struct_bytes != sizeof(nwe_pixel_outputs)")
        assert _render_pixels(r, _lib.PixelOutputs(flags=1), H=0, **bad) == I and _error(r) == "none of rgb / depth / acc requested"
        for name in ("rgb", "depth", "acc"):      # any one of them is a request
            assert _render_pixels(r, _lib.PixelOutputs(**{name: 1}), H=0, **bad) == I and _error(r) == "bad pose / image / row range", name
        # 3. the camera and its ray count, with nwe_render's texts
        for kw in (dict(poses=None), dict(n_poses=0), dict(H=0), dict(W=0), dict(rows=(-1, 4)), dict(rows=(0, 5)), dict(rows=(3, 2))):
            assert _render_pixels(r, good, **kw, **bad) == I and _error(r) == "bad pose / image / row range", kw
        for kw in (dict(fx=0.), dict(fy=-0.)):
            assert _render_pixels(r, good, **kw, **bad) == I and _error(r) == "fx and fy must be non-zero", kw
        assert _render_pixels(r, good, near=2., far=1., **bad) == I
        assert _error(r) == "far < near: the sorted merge of the fine pass needs ascending depths"
        assert _render_pixels(r, good, n_poses=3, H=30000, W=30000, rows=(0, 30000), **bad) == I
        assert _error(r) == "more than 2^31 - 1 rays in one call"
        # 4. the list: a negative count, 2^31 or more, no list; 2^31 - 1 pixels are let through to the next refusal
        text = "bad pixels (null, a negative count, or more than 2^31 - 1)"
        for kw in (dict(n=-1), dict(n=2**31), dict(n=2**40), dict(n=1, pixels=None)):
            assert _render_pixels(r, good, **dict(bad, **kw)) == I and _error(r) == text, kw
        assert _render_pixels(r, good, n=2**31 - 1, precision=9) == I and _error(r) == "unknown precision"
        # 5. the precision; no list at all is fine for no pixels
        assert _render_pixels(r, good, n=0, pixels=None, precision=9) == I and _error(r) == "unknown precision"
        # 6. what nwe_render_rays refuses of the context for lean outputs, in its words; no pixels do not come first
        for n in (3, 0):
            assert _render_pixels(r, good, n=n) == S and _error(r) == "nwe_set_sampling has not been called"
        r.set_sampling(8, 8)
        assert _render_pixels(r, good) == S and _error(r) == "coarse network not set"
        r.set_network(0, synthetic.make_state_dict(5, 3, 64, skips=()))          # a shape without an MFMA kernel
        assert _render_pixels(r, good) == S and _error(r) == "fine network not set but n_importance > 0"
        r.set_network(1, synthetic.make_state_dict(6, 3, 64, skips=()))
        assert _render_pixels(r, good) == U and _error(r).startswith("no MFMA kernel for this network shape")
        sd = synthetic.make_state_dict(7, 4, 128, skips=())
        r.set_network(0, sd); r.set_network(1, sd)
        lib = _lib.load()
        rays_out, report = _lib.Outputs(rgb=1), _lib.PlanReport()

        def rays_refusal():      # of a ray list of four with lean outputs, asked of the planner: a host-only context serves that
            rc = lib.nwe_debug_plan(r._ctx, 1, 1, 4, 0, 1, 4, C.byref(rays_out), 0, _lib.PREC_F16X3, 256, C.byref(report))
            return rc, _error(r)

        r.set_early_termination(0.01)
        want = rays_refusal()
        assert want[0] == U and "early termination" in want[1] and (_render_pixels(r, good), _error(r)) == want
        r.set_early_termination(0.0); r.set_shared_coarse(2)
        want = rays_refusal()
        assert want[0] == U and "shared coarse pass" in want[1] and (_render_pixels(r, good), _error(r)) == want
        r.set_shared_coarse(1)
        r.set_occupancy(np.ones((2, 2, 2), bool), (-1, -1, -1), (1, 1, 1), 2)
        want = rays_refusal()
        assert want[0] == U and "occupancy grid" in want[1] and (_render_pixels(r, good), _error(r)) == want
        r.clear_occupancy()
        r.set_coarse_grid(np.zeros((2, 2, 2), np.float32), (-1, -1, -1), (1, 1, 1))
        want = rays_refusal()
        assert want[0] == U and "coarse density grid" in want[1] and (_render_pixels(r, good), _error(r)) == want
        r.clear_coarse_grid()
        # 7. last, the device - on either path, separate passes honoured
        for separate in (False, True):
            r.set_separate_passes(separate)
            for precision in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32):
                assert _render_pixels(r, good, precision=precision) == S and _error(r) == "host-only context cannot render"
                # no pixels do not come first either: NWE_OK is what a device context answers behind every refusal
                assert _render_pixels(r, good, precision=precision, n=0, pixels=None) == S and _error(r) == "host-only context cannot render"
        with pytest.raises(RuntimeError, match="nwe_render_pixels: host-only context cannot render"):
            r.render_pixels(np.eye(4), 4, 5, torch.zeros(3, dtype=torch.int32), fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5.)
        with pytest.raises(ValueError, match="unknown pixel outputs"):
            r.render_pixels(np.eye(4), 4, 5, torch.zeros(3, dtype=torch.int32), fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., outputs=("rgb", "disp"))
        with pytest.raises(ValueError, match="int32 tensor"):
            r.render_pixels(np.eye(4), 4, 5, torch.zeros(3, dtype=torch.int64), fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5.)
        # a refused call leaves the outputs untouched, and there is no report of a call that never ran
        assert (buf == 123.0).all() and flags[0] == 0
        assert _last(r) == (S, -7, -7) and r.last_pixels() is None
        assert lib.nwe_last_pixels(None, None, None) == I
    finally:
        r.close()


def test_a_stale_struct_is_refused_whatever_it_points_to():
    r = nwe_amd.Renderer(host_only=True)
    try:
        for delta in (-8, 8, -C.sizeof(_lib.PixelOutputs)):
            out = _lib.PixelOutputs(rgb=1, depth=1, acc=1, flags=1)
            out.struct_bytes = C.sizeof(_lib.PixelOutputs) + delta
            assert _render_pixels(r, out) == I and "the caller was built against another version of include/nwe.h" in _error(r), delta
        assert C.sizeof(_lib.PixelOutputs) == 8 + 4 * C.sizeof(C.c_void_p)
    finally:
        r.close()


def test_the_switch():
    lib = _lib.load()
    assert lib.nwe_get_adaptive_pixel_lists(None) == -1 and lib.nwe_set_adaptive_pixel_lists(None, 1) == I
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert r.adaptive_pixel_lists is False                      # off by default
        for on in (2, -1, 7, 256):
            assert lib.nwe_set_adaptive_pixel_lists(r._ctx, on) == I and _error(r) == "adaptive_pixel_lists must be 0 or 1 (0 = off)"
            assert lib.nwe_get_adaptive_pixel_lists(r._ctx) == 0
        r.set_adaptive_pixel_lists(True)
        assert r.adaptive_pixel_lists is True and lib.nwe_get_adaptive_pixel_lists(r._ctx) == 1
        assert lib.nwe_set_adaptive_pixel_lists(r._ctx, 3) == I and r.adaptive_pixel_lists is True      # a refused value changes nothing
        r.set_adaptive_pixel_lists(False)
        assert r.adaptive_pixel_lists is False
    finally:
        r.close()


def test_the_path_decision():
    """list: an MFMA precision, one shape with list kernels for both networks - so both in a product formulation - no separate
    passes.  Everything else that is legal: a ray table."""
    lib = _lib.load()
    assert lib.nwe_debug_pixels_path(None, _lib.PREC_F16X3) == -1
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert lib.nwe_debug_pixels_path(r._ctx, 9) == -1
        assert r.pixels_path() == "rays"                            # no network yet: nothing for the list kernels to run
        r.set_sampling(8, 8)
        sd = synthetic.make_state_dict(7, 4, 128, skips=())
        r.set_network(0, sd); r.set_network(1, sd)
        assert [r.pixels_path(p) for p in ("f16x3", "f16x1", "f32")] == ["list", "list", "rays"]
        r.set_separate_passes(True)
        assert [r.pixels_path(p) for p in ("f16x3", "f16x1", "f32")] == ["rays"] * 3
        r.set_separate_passes(False)
        assert r.pixels_path() == "list"
        # packed unfolded: the reference formulation has no list kernels - one network is enough
        r.debug_set_fold(False)
        r.set_network(1, sd)
        assert [r.pixels_path(p) for p in ("f16x3", "f16x1")] == ["rays"] * 2
        r.set_network(0, sd)
        assert r.pixels_path() == "rays"
        r.debug_set_fold(True)
        r.set_network(0, sd); r.set_network(1, sd)
        assert r.pixels_path() == "list"
        # a shape in the fp32 domain only (3 x 64): no MFMA kernel, so no list kernel
        small = synthetic.make_state_dict(5, 3, 64, skips=())
        r.set_network(0, small); r.set_network(1, small)
        assert [r.pixels_path(p) for p in ("f16x3", "f16x1", "f32")] == ["rays"] * 3
        # two MFMA shapes (legal under separate passes only): not one shared shape
        r.set_network(0, sd); r.set_network(1, synthetic.make_state_dict(8, 8, 256, skips=(4,)))
        assert r.pixels_path() == "rays"
        # without importance samples the fine network does not run: the coarse network's shape decides
        r.set_sampling(8, 0)
        assert r.pixels_path() == "list"
        # networks without view directions have list kernels
        nv = synthetic.make_state_dict(7, 4, 128, skips=(), use_view_dirs=False)
        r.set_sampling(8, 8)
        r.set_network(0, nv); r.set_network(1, nv)
        assert [r.pixels_path(p) for p in ("f16x3", "f16x1", "f32")] == ["list", "list", "rays"]
    finally:
        r.close()


def test_the_handlers_option(monkeypatch):
    monkeypatch.delenv("NWE_ADAPTIVE", raising=False)
    monkeypatch.delenv("NWE_ADAPTIVE_LISTS", raising=False)
    assert Handler("office_geneve", "none.ckpt")._adaptive_lists is False
    assert Handler("office_geneve", "none.ckpt", adaptive={})._adaptive_lists is False
    assert Handler("office_geneve", "none.ckpt", adaptive={}, adaptive_lists=True)._adaptive_lists is True
    with pytest.raises(ValueError, match="adaptive_lists is an option of the adaptive frame"):
        Handler("office_geneve", "none.ckpt", adaptive_lists=True)
    monkeypatch.setenv("NWE_ADAPTIVE_LISTS", "1")
    with pytest.raises(ValueError, match="adaptive_lists is an option of the adaptive frame"):
        Handler("office_geneve", "none.ckpt")
    assert Handler("office_geneve", "none.ckpt", adaptive={"k": 3})._adaptive_lists is True
    assert Handler("office_geneve", "none.ckpt", adaptive={"k": 3}, adaptive_lists=False)._adaptive_lists is False
    monkeypatch.setenv("NWE_ADAPTIVE", "2,0.01")
    assert Handler("office_geneve", "none.ckpt")._adaptive_lists is True
    monkeypatch.setenv("NWE_ADAPTIVE_LISTS", "yes")
    with pytest.raises(ValueError, match="NWE_ADAPTIVE_LISTS must be 0 or 1"):
        Handler("office_geneve", "none.ckpt")
