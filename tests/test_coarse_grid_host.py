"""The baked coarse pass without a GPU (include/nwe.h: nwe_set_coarse_grid): the numpy restatement of the interpolation rule, the
grid calls on a host-only context, the plan and the refusals of a baked call (nwe_debug_plan), the handler's arguments, and the
conditioning of the parity scene of tests/test_gpu_coarse_grid.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from tests import coarse_grid as B

PRODUCER, CONSUMER, SHARE = 1, 2, 2
TOL = {"rgb": 1e-4, "depth": 1e-4 * B.FAR, "acc": 1e-4}     # the project's parity tolerances (tests/test_gpu_occupancy.py)


def _renderer(nets=("4x128", "4x128"), ns=8, ni=8, fold=True):
    r = nwe_amd.Renderer(host_only=True)
    r.debug_set_fold(fold)
    shapes = {"4x128": dict(D=4, W=128), "8x256": dict(D=8, W=256), "3x64": dict(D=3, W=64, skips=())}
    for which, net in enumerate(nets):
        r.set_network(which, synthetic.make_state_dict(1000 + which, **shapes[net]))
    r.set_sampling(ns, ni)
    return r


def _set(r, kind="random"):
    g = B.grid(kind)
    r.set_coarse_grid(g["values"], g["lo"], g["hi"])


def _plan(r, n_rays, outputs=("rgb",), cus=256, pinhole=True, precision=_lib.PREC_F16X3):
    report = _lib.PlanReport()
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, 1, n_rays, 0, 1, -1 if pinhole else n_rays, C.byref(_lib.Outputs(**{k: 1 for k in outputs})), 0,
                                    precision, cus, C.byref(report))
    return rc, report


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def test_restatement_of_the_interpolation_rule():
    g = B.grid("random")
    lo, hi, res, v = g["lo"].astype(np.float64), g["hi"].astype(np.float64), np.array(g["res"]), g["values"]
    cell = (hi - lo) / res
    # at the cell centres the value is the cell's (f is 0 to rounding)
    centres = B.G.cell_centres(lo, hi, g["res"]).astype(np.float32)
    assert np.abs(B.grid_sigma(centres, g) - v).max() < 1e-4
    # within half a cell of a face the value is the face cell's: the same along the axis
    for axis in range(3):
        a, b = centres[1, 2, 3].copy(), centres[1, 2, 3].copy()
        a[axis] = lo[axis] + 0.05 * cell[axis]; b[axis] = lo[axis] + 0.45 * cell[axis]
        assert B.grid_sigma(a, g) == B.grid_sigma(b, g)
        a[axis] = hi[axis] - 0.05 * cell[axis]; b[axis] = hi[axis] - 0.45 * cell[axis]
        assert B.grid_sigma(a, g) == B.grid_sigma(b, g)
    # outside the box, and where a coordinate is not finite: 0; the faces themselves are inside
    inside = centres[1, 2, 3]
    for axis in range(3):
        for value in (lo[axis] - 0.01, hi[axis] + 0.01, np.nan, np.inf, -np.inf, 3e38):
            p = inside.copy(); p[axis] = value
            assert B.grid_sigma(p, g) == 0.0, (axis, value)
        for value in (lo[axis], hi[axis]):
            p = inside.copy(); p[axis] = value
            assert B.grid_sigma(p, g) != 0.0
    # equal values interpolate exactly; a non-finite value propagates to the points whose taps include it and to no other
    const = B.make_grid(np.full((3, 4, 5), 0.3, np.float32), (0, 0, 0), (1, 2, 3))
    rng = np.random.default_rng(1)
    pts = (rng.random((500, 3)) * np.array([1, 2, 3])).astype(np.float32)
    assert (B.grid_sigma(pts, const) == np.float32(0.3)).all()
    bad = B.grid("small_nonfinite")
    c = B.G.cell_centres(bad["lo"].astype(np.float64), bad["hi"].astype(np.float64), bad["res"]).astype(np.float32)
    assert np.isnan(B.grid_sigma(c[2, 3, 4], bad)) and np.isfinite(B.grid_sigma(c[0, 0, 0], bad))
    # fp32 and fp64 agree to fp32 rounding on points inside
    pts = (lo + rng.random((2000, 3)) * (hi - lo)).astype(np.float32)
    assert np.abs(B.grid_sigma(pts, g).astype(np.float64) - B.grid_sigma(pts, g, np.float64)).max() < 2e-5
    # the order of the interpolations is z, then y, then x: restated with scalars for one point
    p = np.array([1.3, 5.1, -0.4], np.float32)
    gc = (p - g["lo"]) * g["inv"] - np.float32(0.5)
    i0 = np.floor(gc).astype(int); f = gc - np.floor(gc)
    assert f.dtype == np.float32
    i1 = np.minimum(i0 + 1, res - 1); i0 = np.maximum(i0, 0)
    L = lambda a, b, t: np.float32(a + np.float32(np.float32(b - a) * t))
    cz = [[L(v[x, y, i0[2]], v[x, y, i1[2]], f[2]) for y in (i0[1], i1[1])] for x in (i0[0], i1[0])]
    want = L(L(cz[0][0], cz[0][1], f[1]), L(cz[1][0], cz[1][1], f[1]), f[0])
    assert B.grid_sigma(p, g).view(np.uint32) == want.view(np.uint32)


def test_coarse_points_are_the_oracles_fp32_points():
    _, _, cfg, _, rays, _, _ = B.scene("s192")
    z, pts = B.coarse_points(rays.numpy(), cfg.n_samples)
    t = torch.linspace(0., 1., steps=cfg.n_samples)
    z_ref = rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t
    p_ref = rays[:, None, 0:3] + rays[:, None, 3:6] * z_ref[..., None]
    assert np.array_equal(z, z_ref.numpy()) and np.array_equal(pts, p_ref.numpy())


# ---- the grid calls on a host-only context --------------------------------------------------------------------------------------

def test_set_get_copy_clear_on_a_host_only_context():
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert r.coarse_grid is None and r.coarse_grid_values() is None
        v = B.random_values((3, 4, 5))
        r.set_coarse_grid(v, (-1.0, 0.0, 2.0), (1.0, 3.0, 2.5))
        g = r.coarse_grid
        assert g["resolution"] == (3, 4, 5) and g["lo"] == (-1.0, 0.0, 2.0) and g["hi"] == (1.0, 3.0, 2.5)
        want = np.array([3, 4, 5], np.float32) / (np.array(g["hi"], np.float32) - np.array(g["lo"], np.float32))
        assert g["inv"].dtype == np.float32 and np.array_equal(g["inv"], want)
        assert np.array_equal(r.coarse_grid_values(), v)
        # a flat array with a resolution, and a torch tensor
        r.set_coarse_grid(torch.from_numpy(v).reshape(-1), (0, 0, 0), (1, 1, 1), (3, 4, 5))
        assert np.array_equal(r.coarse_grid_values(), v) and r.coarse_grid["hi"] == (1.0, 1.0, 1.0)
        lib = _lib.load()
        buf = np.empty(60, np.float32)
        assert lib.nwe_coarse_grid_copy(r._ctx, buf.ctypes.data, 59) == _lib.NWE_ERR_INVALID
        assert lib.nwe_coarse_grid_copy(r._ctx, None, 60) == _lib.NWE_ERR_INVALID
        r.clear_coarse_grid()
        assert r.coarse_grid is None
        assert lib.nwe_get_coarse_grid(r._ctx, None, None, None, None) == _lib.NWE_ERR_STATE
        assert lib.nwe_coarse_grid_copy(r._ctx, buf.ctypes.data, 60) == _lib.NWE_ERR_STATE
        r.clear_coarse_grid()     # clearing nothing is fine
        assert lib.nwe_clear_coarse_grid(None) == _lib.NWE_ERR_INVALID and lib.nwe_get_coarse_grid(None, None, None, None, None) == _lib.NWE_ERR_INVALID
        # the device-side calls say what they need
        with pytest.raises(RuntimeError, match="needs a device context"):
            r.bake_coarse_grid((0, 0, 0), (1, 1, 1), 4)
        with pytest.raises(RuntimeError, match="needs a device context"):
            r.coarse_grid_weights(np.eye(4, dtype=np.float32), 2, 2, fx=1., fy=1., cx=0., cy=0., near=0.1, far=1.)
    finally:
        r.close()


def test_every_refusal_of_set_coarse_grid_by_name():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    F3, I3 = C.c_float * 3, C.c_int * 3
    v = np.zeros(8, np.float32)
    try:
        r.set_coarse_grid(np.ones((1, 1, 1), np.float32), (0, 0, 0), (1, 1, 1))
        ok = (F3(0, 0, 0), F3(1, 1, 1), I3(2, 2, 2))
        for args, text in (((None, ok[1], ok[2]), "null lo, hi or resolution"), ((ok[0], None, ok[2]), "null lo, hi or resolution"),
                           ((ok[0], ok[1], None), "null lo, hi or resolution")):
            assert lib.nwe_set_coarse_grid(r._ctx, *args, v.ctypes.data, 0) == _lib.NWE_ERR_INVALID and text in _error(r)
        assert lib.nwe_set_coarse_grid(r._ctx, *ok, None, 0) == _lib.NWE_ERR_INVALID and "null sigma" in _error(r)
        assert lib.nwe_set_coarse_grid(r._ctx, *ok, v.ctypes.data, 1) == _lib.NWE_ERR_INVALID and "host-only" in _error(r)
        assert lib.nwe_set_coarse_grid(None, *ok, v.ctypes.data, 0) == _lib.NWE_ERR_INVALID
        for lo, hi, text in (((0, 0, 0), (1, 0, 1), "lo < hi"), ((0, 2, 0), (1, 1, 1), "lo < hi"), ((0, 0, float("nan")), (1, 1, 1), "finite"),
                             ((0, 0, 0), (float("inf"), 1, 1), "finite"), ((-3e38, 0, 0), (3e38, 1, 1), "finite"),
                             ((0, 0, 0), (1, 1e-44, 1), "finite")):
            with pytest.raises(ValueError, match=text):
                r.set_coarse_grid(v.reshape(2, 2, 2), lo, hi)
        for res in ((0, 2, 2), (2, 513, 2), (2, 2, -1)):
            with pytest.raises(ValueError, match="1..512"):
                r.set_coarse_grid(np.zeros(max(int(np.prod(res)), 8), np.float32), (0, 0, 0), (1, 1, 1), res)
        with pytest.raises(ValueError, match="values for resolution"):
            r.set_coarse_grid(v, (0, 0, 0), (1, 1, 1), (2, 2, 3))
        assert r.coarse_grid["resolution"] == (1, 1, 1)        # a refused call leaves the grid
        r.set_coarse_grid(np.zeros((512, 1, 2), np.float32), (0, 0, 0), (1, 1, 1))
        assert r.coarse_grid["resolution"] == (512, 1, 2)
    finally:
        r.close()


def test_the_coarse_network_clears_the_grid_and_the_fine_network_does_not():
    r = _renderer()
    try:
        _set(r)
        r.set_network(1, synthetic.make_state_dict(5, 8, 256))
        assert r.coarse_grid["resolution"] == B.BOX_RES
        with pytest.raises(NotImplementedError):                # a refused call leaves it
            r.set_network(0, synthetic.make_state_dict(5, 17, 256))
        assert r.coarse_grid is not None
        r.set_network(0, synthetic.make_state_dict(6, 4, 128))
        assert r.coarse_grid is None
        _set(r)
        r.set_network(0, synthetic.make_state_dict(6, 4, 128, use_view_dirs=False))
        assert r.coarse_grid is None
    finally:
        r.close()


# ---- the plan of a baked call ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32])
@pytest.mark.parametrize("nets", [("4x128", "4x128"), ("4x128", "8x256"), ("3x64", "8x256")])
def test_the_plan_of_a_baked_call(nets, precision):
    """Two stages: the grid producer over the call's rays, which is no MFMA launch group (variant = plan = -1), and the sharing
    consumer at k = 1 with the fine network in both descriptor slots - so a 4x128, or a shape without any MFMA kernel, plans
    under an 8x256 fine network without separate passes."""
    ns, ni, n = 8, 8, 1000
    r = _renderer(nets, ns, ni)
    try:
        if nets[0] != nets[1] and precision != _lib.PREC_F32:
            rc, _ = _plan(r, n, precision=precision)
            assert rc == _lib.NWE_ERR_UNSUPPORTED          # without a grid the pair has no fused kernel
        _set(r)
        rc, p = _plan(r, n, precision=precision)
        assert rc == _lib.NWE_OK, _error(r)
        assert (p.separate, p.share, p.full, p.coarse_launch, p.share_k) == (0, 1, 0, 1, 1)
        assert (p.may_queue, p.need_side, p.need_evals, p.coarse_flags) == (0, 0, 0, 0)
        assert p.table_elems == n * ns
        assert p.evals_full == n * (2 * ns + ni) and p.evals_run == n * (ns + ni) and p.share_rays == n
        c = p.coarse
        assert (c.active, c.role, c.n_rays, c.variant, c.plan, c.n_launches) == (1, PRODUCER, n, -1, -1, 1)
        assert (c.n_importance, c.net, c.fork, c.tail, c.tail_items) == (0, 0, 0, 0, 0)
        assert list(c.ray_first) + list(c.rays) + list(c.split) + list(c.items) + list(c.grid) == [0] * 10
        m = p.main
        assert (m.active, m.role, m.n_rays, m.n_importance, m.net) == (1, CONSUMER, n, ni, 1)
        if precision != _lib.PREC_F32:
            assert m.variant == SHARE and m.n_launches >= 1 and sum(m.rays) == n and list(m.grid) == [0, 0]
        # more than 64 coarse samples: the sample-split plan only
        r.set_sampling(96, 32)
        rc, p = _plan(r, n, precision=precision)
        assert rc == _lib.NWE_OK and p.table_elems == n * 96
        if precision != _lib.PREC_F32:
            assert p.main.plan == 1
        # n_importance == 0: the ordinary call, nothing of the grid in the plan
        r.set_sampling(ns, 0)
        if nets[0] != "3x64" or precision == _lib.PREC_F32:
            rc, p = _plan(r, n, precision=precision)
            assert rc == _lib.NWE_OK and (p.share, p.coarse_launch, p.table_elems, p.coarse.active) == (0, 0, 0, 0)
            assert p.evals_run == p.evals_full == n * ns and p.main.role == 0 and p.main.net == -1
    finally:
        r.close()


def test_all_refusals_of_the_baked_call_by_name(monkeypatch):
    r = _renderer()
    grid = "a coarse density grid is set (nwe_set_coarse_grid, 11 x 9 x 5): "
    try:
        _set(r)
        for ni in (8, 0):
            r.set_sampling(8, ni)
            assert _plan(r, 100)[0] == _lib.NWE_OK
            for outputs in (("rgb", "z_std"), ("rgb", "weights_coarse"), ("rgb", "disp"), ("raw_fine",)):
                assert _plan(r, 100, outputs)[0] == _lib.NWE_ERR_UNSUPPORTED
                assert _error(r) == grid + "only rgb / depth / acc / flags can be requested; call nwe_clear_coarse_grid for this call"
            for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
                assert _plan(r, 100, pinhole=False, precision=precision)[0] == _lib.NWE_ERR_UNSUPPORTED
                assert _error(r).startswith(grid + "nwe_render_rays, its hooks and its training tables do not read the grid")
        r.set_sampling(8, 8)
        for setter, off, text in ((r.set_early_termination, (1e-2, 0.0), "early termination (nwe_set_early_termination"),
                                  (r.set_shared_coarse, (2, 1), "the shared coarse pass (nwe_set_shared_coarse"),
                                  (r.set_separate_passes, (True, False), "separate passes (nwe_set_separate_passes)")):
            setter(off[0])
            for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
                assert _plan(r, 100, precision=precision)[0] == _lib.NWE_ERR_UNSUPPORTED
                assert "not built together with " + text in _error(r)
            setter(off[1])
        r.set_occupancy(np.ones((2, 2, 2), bool), (0, 0, 0), (1, 1, 1), (2, 2, 2))
        assert _plan(r, 100)[0] == _lib.NWE_ERR_UNSUPPORTED
        assert _error(r).startswith(grid + "it is not built together with an occupancy grid (nwe_set_occupancy)")
        r.clear_occupancy()
        # a stamped launch
        assert _lib.load().nwe_debug_set_stamps(r._ctx, 8) == _lib.NWE_OK
        assert _plan(r, 100)[0] == _lib.NWE_ERR_UNSUPPORTED and "a stamped launch (nwe_debug_set_stamps)" in _error(r)
        _lib.load().nwe_debug_set_stamps(r._ctx, None)
        assert _plan(r, 100)[0] == _lib.NWE_OK
        # behind the call's own refusals
        assert _plan(r, 100, ("rgb", "feat_map"))[0] == _lib.NWE_ERR_UNSUPPORTED and "feat_map" in _error(r) and "grid" not in _error(r)
    finally:
        r.close()
    # a fine network packed unfolded has no sharing kernel; NWE_PREC_F32 renders it
    r = _renderer(fold=False)
    try:
        _set(r)
        assert _plan(r, 100)[0] == _lib.NWE_ERR_UNSUPPORTED
        assert _error(r).startswith(grid + "a network packed unfolded (nwe_debug_set_fold(0)) has no sharing MFMA kernel; use NWE_PREC_F32")
        assert _plan(r, 100, precision=_lib.PREC_F32)[0] == _lib.NWE_OK
        r.set_sampling(8, 0)
        assert _plan(r, 100)[0] == _lib.NWE_OK       # one pass: the ordinary call
    finally:
        r.close()
    # a fine network without any MFMA kernel keeps the call's own refusal
    r = _renderer(("4x128", "3x64"))
    try:
        _set(r)
        assert _plan(r, 100)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r).startswith("no MFMA kernel for this network shape")
    finally:
        r.close()


# ---- the handler ----------------------------------------------------------------------------------------------------------------

def test_handler_arguments_and_environment(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    box = {"lo": B.BOX_LO, "hi": B.BOX_HI}
    monkeypatch.delenv("NWE_BAKED_COARSE", raising=False)
    assert H("office_geneve", "x.ckpt")._baked_coarse is None
    assert H("office_geneve", "x.ckpt", baked_coarse=box)._baked_coarse == {"lo": B.BOX_LO, "hi": B.BOX_HI, "resolution": 128}
    assert H("office_geneve", "x.ckpt", baked_coarse=dict(box, resolution=(8, 9, 10)))._baked_coarse["resolution"] == (8, 9, 10)
    monkeypatch.setenv("NWE_BAKED_COARSE", "64")
    assert H("office_geneve", "x.ckpt", baked_coarse=box)._baked_coarse["resolution"] == 64
    assert H("office_geneve", "x.ckpt")._baked_coarse is None          # without a box there is no grid
    monkeypatch.setenv("NWE_BAKED_COARSE", "64,2")
    with pytest.raises(ValueError, match="NWE_BAKED_COARSE"):
        H("office_geneve", "x.ckpt", baked_coarse=box)
    monkeypatch.delenv("NWE_BAKED_COARSE")
    for kw in ({"lo": B.BOX_LO}, {"hi": B.BOX_HI}, dict(box, probes=2)):
        with pytest.raises(ValueError, match="baked_coarse"):
            H("office_geneve", "x.ckpt", baked_coarse=kw)
    for other in (dict(early_termination=1e-2), dict(shared_coarse=2), dict(separate_passes=True), dict(occupancy=box)):
        with pytest.raises(ValueError, match="baked coarse pass"):
            H("office_geneve", "x.ckpt", baked_coarse=box, **other)
    h = H("office_geneve", "x.ckpt", baked_coarse=box)
    with pytest.raises(RuntimeError, match="initialize_models"):
        h.bake_coarse_grid(B.BOX_LO, B.BOX_HI, 8)
    with pytest.raises(RuntimeError, match="initialize_models"):
        h.clear_coarse_grid()


# ---- the parity scene -----------------------------------------------------------------------------------------------------------

def test_the_parity_scene_is_well_conditioned():
    """The oracle composed with the restated grid in fp32 and in fp64 agree within the parity tolerance on EVERY ray: the scene's
    reference reproduces itself, so a kernel can be held to it on every ray.  Every sample lies inside the box (the rule is
    discontinuous at its faces) and every coarse bin carries weight."""
    _, _, cfg, _, rays, _, _ = B.scene(B.PARITY_SCENE)
    g = B.grid(B.PARITY_GRID)
    a, b = B.parity_reference(), B.parity_reference(fp64=True)
    for k in ("rgb", "depth", "acc"):
        err = (a[k].double() - b[k]).abs()
        print(f"parity scene, fp32 against fp64 {k}: {float(err.max()):.2e} (tol {TOL[k]:.0e})")
        assert float(err.max()) <= TOL[k], k
    lo, hi = g["lo"].astype(np.float64), g["hi"].astype(np.float64)
    for z in (a["z_fine"].numpy(), b["z_fine"].numpy()):
        pts = rays[:, None, 0:3].numpy() + rays[:, None, 3:6].numpy() * z[..., None]
        assert (pts > lo + 1e-3).all() and (pts < hi - 1e-3).all()
    assert float(a["weights"][:, 1:-1].min()) > 1e-3 and float(a["acc"].min()) > 0.05
    assert float((a["sigma"] - b["sigma"].float()).abs().max()) < 1e-5
