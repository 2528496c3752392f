"""The radiance grid without a GPU (include/nwe.h: nwe_set_radiance_grid, nwe_render_grid): the numpy restatement of the lookup, the
grid calls on a host-only context, every refusal of nwe_render_grid in front of the host-only one and of the bake, that a grid
moves no plan of a render call, the handler's arguments, and the conditioning of the parity scene of
tests/test_gpu_radiance_grid.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from tests import coarse_grid as B
from tests import radiance_grid as R

TOL = {"rgb": 1e-4, "depth": 1e-4 * R.FAR, "acc": 1e-4}     # the project's parity tolerances (tests/test_gpu_occupancy.py)
F3, I3 = C.c_float * 3, C.c_int * 3


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _set(r, kind="random"):
    g = R.grid(kind)
    r.set_radiance_grid(g["values"], g["lo"], g["hi"])


def _networks(r, nets=("4x128", "4x128")):
    shapes = {"4x128": dict(D=4, W=128), "8x256": dict(D=8, W=256), "3x64": dict(D=3, W=64, skips=())}
    for which, net in enumerate(nets):
        r.set_network(which, synthetic.make_state_dict(1000 + which, **shapes[net]))


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def test_rows_are_the_coarse_grids_sigma_per_channel():
    rng = np.random.default_rng(3)
    for kind in R.GRIDS:
        g = R.grid(kind)
        lo, hi = g["lo"].astype(np.float64), g["hi"].astype(np.float64)
        cell = (hi - lo) / np.array(g["res"])
        inside = lo + rng.random((400, 3)) * (hi - lo)
        faces = inside.copy()                      # within half a cell of a face, either side of it
        axis = rng.integers(0, 3, 400)
        faces[np.arange(400), axis] = np.where(rng.random(400) < 0.5, lo[axis], hi[axis]) + (rng.random(400) - 0.5) * cell[axis]
        outside = lo - 0.1 - rng.random((100, 3)) * 5.0
        nonfinite = inside[:60].copy()
        nonfinite[np.arange(60), np.arange(60) % 3] = np.tile([np.nan, np.inf, -np.inf, 3.4e38], 15)
        pts = np.concatenate([inside, faces, outside, nonfinite]).astype(np.float32)
        rows = R.grid_rows(pts, g)
        assert rows.shape == (960, 4) and rows.dtype == np.float32
        for c in range(4):
            assert R.same_bits(rows[:, c], B.grid_sigma(pts, R.channel(g, c))), (kind, c)
        # the sigma channel is what a coarse grid of the same values over the same box gives
        as_coarse = B.make_grid(g["values"][..., 3], g["lo"], g["hi"])
        assert np.array_equal(as_coarse["inv"], g["inv"])
        assert R.same_bits(rows[:, 3], B.grid_sigma(pts, as_coarse)), kind
        assert (rows[800:] == 0).all() and (R.grid_rows(pts[800:], g, np.float64) == 0).all()   # rows of zeros outside
        assert (rows[:400] != 0).any()


def test_rows_at_the_cell_centres_are_the_stored_rows():
    """A box whose cells are half a unit wide: inv = 2 and the centres (i + 0.5) / 2 are exact, so the fraction is exactly 0."""
    v = R.random_rows((3, 4, 5), seed=21)
    g = R.make_grid(v, (0, 0, 0), (1.5, 2.0, 2.5))
    assert np.array_equal(g["inv"], np.float32([2, 2, 2]))
    centres = B.G.cell_centres((0, 0, 0), (1.5, 2.0, 2.5), (3, 4, 5)).astype(np.float32)
    assert np.array_equal(R.grid_rows(centres, g).view(np.uint32), v.view(np.uint32))
    # a non-finite value propagates in its channel and in no other
    bad = R.grid("small_nonfinite")
    c = B.G.cell_centres(bad["lo"].astype(np.float64), bad["hi"].astype(np.float64), bad["res"]).astype(np.float32)
    row = R.grid_rows(c[2, 3, 4], bad)
    assert np.isnan(row[0]) and np.isfinite(row[1:]).all()
    # one cell on an axis: both taps clamp to it, the rows do not depend on that coordinate
    flat = R.grid("flat")
    p = np.float32([[-7.0, 3.3, 1.1], [13.0, 3.3, 1.1]])
    rows = R.grid_rows(p, flat)
    assert np.array_equal(rows[0], rows[1]) and (rows[0] != 0).all()
    one = R.grid("one")
    assert np.array_equal(R.grid_rows(np.float32([1.0, 2.0, 3.0]), one), one["values"][0, 0, 0])


# ---- the grid calls on a host-only context --------------------------------------------------------------------------------------

def test_set_get_copy_clear_on_a_host_only_context():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    try:
        assert r.radiance_grid is None and r.radiance_grid_values() is None and r.last_grid_ms() is None
        v = R.random_rows((3, 4, 5))
        v[1, 2, 3, 1] = np.nan
        r.set_radiance_grid(v, (-1.0, 0.0, 2.0), (1.0, 3.0, 2.5))
        g = r.radiance_grid
        assert g["resolution"] == (3, 4, 5) and g["lo"] == (-1.0, 0.0, 2.0) and g["hi"] == (1.0, 3.0, 2.5)
        want = np.array([3, 4, 5], np.float32) / (np.array(g["hi"], np.float32) - np.array(g["lo"], np.float32))
        assert g["inv"].dtype == np.float32 and np.array_equal(g["inv"], want)
        assert np.array_equal(r.radiance_grid_values().view(np.uint32), v.view(np.uint32))
        # a flat array with a resolution, and a torch tensor
        r.set_radiance_grid(torch.from_numpy(v).reshape(-1), (0, 0, 0), (1, 1, 1), (3, 4, 5))
        assert np.array_equal(r.radiance_grid_values().view(np.uint32), v.view(np.uint32)) and r.radiance_grid["hi"] == (1.0, 1.0, 1.0)
        with pytest.raises(ValueError, match=r"\[rx, ry, rz, 4\]"):
            r.set_radiance_grid(v[..., 0], (0, 0, 0), (1, 1, 1))
        buf = np.empty(240, np.float32)
        assert lib.nwe_radiance_grid_copy(r._ctx, buf.ctypes.data, 60) == _lib.NWE_ERR_INVALID and "4 * rx * ry * rz" in _error(r)
        assert lib.nwe_radiance_grid_copy(r._ctx, None, 240) == _lib.NWE_ERR_INVALID
        # the other grids and the radiance grid do not know of each other
        assert r.coarse_grid is None and r.occupancy is None
        r.set_coarse_grid(v[..., 3], (0, 0, 0), (1, 1, 1))
        r.clear_coarse_grid()
        assert r.radiance_grid["resolution"] == (3, 4, 5)
        r.clear_radiance_grid()
        assert r.radiance_grid is None
        lo, res = F3(7, 7, 7), I3(9, 9, 9)
        assert lib.nwe_get_radiance_grid(r._ctx, lo, None, res, None) == _lib.NWE_ERR_STATE
        assert tuple(lo) == (7, 7, 7) and tuple(res) == (9, 9, 9)       # nothing written
        assert lib.nwe_radiance_grid_copy(r._ctx, buf.ctypes.data, 240) == _lib.NWE_ERR_STATE
        r.clear_radiance_grid()     # clearing nothing is fine
        assert lib.nwe_clear_radiance_grid(None) == _lib.NWE_ERR_INVALID
        assert lib.nwe_get_radiance_grid(None, None, None, None, None) == _lib.NWE_ERR_INVALID
        assert lib.nwe_radiance_grid_copy(None, buf.ctypes.data, 240) == _lib.NWE_ERR_INVALID
        assert lib.nwe_last_grid_ms(None) < 0 and lib.nwe_last_grid_ms(r._ctx) < 0
    finally:
        r.close()


def test_either_network_clears_the_grid_and_a_refused_upload_does_not():
    r = nwe_amd.Renderer(host_only=True)
    try:
        for which in (0, 1):
            _set(r)
            with pytest.raises(NotImplementedError):                # a refused call leaves it
                r.set_network(which, synthetic.make_state_dict(5, 17, 256))
            assert r.radiance_grid["resolution"] == R.BOX_RES
            r.set_network(which, synthetic.make_state_dict(6, 4, 128))
            assert r.radiance_grid is None
            _set(r)
            r.set_network(which, synthetic.make_state_dict(6, 4, 128, use_view_dirs=False))
            assert r.radiance_grid is None
        _set(r)
        r.set_sampling(8, 8); r.set_white_background(True); r.set_early_termination(0.01)
        assert r.radiance_grid is not None                          # no other setter touches it
    finally:
        r.close()


def test_every_refusal_of_set_radiance_grid_by_name():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    v = np.zeros(32, np.float32)
    try:
        r.set_radiance_grid(np.ones((1, 1, 1, 4), np.float32), (0, 0, 0), (1, 1, 1))
        ok = (F3(0, 0, 0), F3(1, 1, 1), I3(2, 2, 2))
        for args in ((None, ok[1], ok[2]), (ok[0], None, ok[2]), (ok[0], ok[1], None)):
            assert lib.nwe_set_radiance_grid(r._ctx, *args, v.ctypes.data, 0) == _lib.NWE_ERR_INVALID
            assert _error(r) == "radiance grid: null lo, hi or resolution"
        assert lib.nwe_set_radiance_grid(r._ctx, *ok, None, 0) == _lib.NWE_ERR_INVALID and _error(r) == "radiance grid: null rows"
        assert lib.nwe_set_radiance_grid(r._ctx, *ok, v.ctypes.data, 1) == _lib.NWE_ERR_INVALID
        assert _error(r) == "radiance grid: a host-only context takes its rows from the host"
        assert lib.nwe_set_radiance_grid(None, *ok, v.ctypes.data, 0) == _lib.NWE_ERR_INVALID
        # the box in front of the array
        assert lib.nwe_set_radiance_grid(r._ctx, ok[0], F3(1, 0, 1), ok[2], None, 1) == _lib.NWE_ERR_INVALID and "lo < hi" in _error(r)
        for lo, hi, text in (((0, 0, 0), (1, 0, 1), "radiance grid: the box must have lo < hi on every axis"),
                             ((0, 2, 0), (1, 1, 1), "lo < hi"), ((0, 0, float("nan")), (1, 1, 1), "radiance grid: the box must be finite"),
                             ((0, 0, 0), (float("inf"), 1, 1), "finite"), ((-3e38, 0, 0), (3e38, 1, 1), "finite"),
                             ((0, 0, 0), (1, 1e-44, 1), r"resolution / \(hi - lo\) is not, in fp32")):
            with pytest.raises(ValueError, match=text):
                r.set_radiance_grid(v.reshape(2, 2, 2, 4), lo, hi)
        for res in ((0, 2, 2), (2, 513, 2), (2, 2, -1)):
            with pytest.raises(ValueError, match=r"radiance grid: the resolution must be in 1\.\.512 on every axis"):
                r.set_radiance_grid(np.zeros(4 * max(int(np.prod(res)), 8), np.float32), (0, 0, 0), (1, 1, 1), res)
        with pytest.raises(ValueError, match="values for resolution"):
            r.set_radiance_grid(v, (0, 0, 0), (1, 1, 1), (2, 2, 3))
        assert r.radiance_grid["resolution"] == (1, 1, 1)        # a refused call leaves the grid
        r.set_radiance_grid(np.zeros((512, 1, 2, 4), np.float32), (0, 0, 0), (1, 1, 1))
        assert r.radiance_grid["resolution"] == (512, 1, 2)
    finally:
        r.close()


def _render_grid(r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4)):
    ptr = None if poses is None else poses.ctypes.data
    return _lib.load().nwe_render_grid(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0], rows[1],
                                       None if out is None else C.byref(out), None)


def test_every_refusal_of_render_grid_in_front_of_the_host_only_one():
    """Code, text and order: each call below is wrong in everything behind the refusal it expects as well."""
    r = nwe_amd.Renderer(host_only=True)
    I, S = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE
    try:
        good = _lib.GridOutputs(rgb=1)
        none = _lib.GridOutputs(flags=1)
        stale = _lib.GridOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.GridOutputs) - 8
        # 1. the context - whatever else is wrong
        assert _render_grid(None, None, poses=None) == I
        # 2. the outputs, in front of the camera (H = 0), the state (no grid, no sampling) and the device
        assert _render_grid(r, None, H=0) == I and _error(r) == "null outputs"
        assert _render_grid(r, stale, H=0) == I and _error(r).startswith("nwe_grid_outputs.struct_bytes != sizeof(nwe_grid_outputs)")
        assert _render_grid(r, none, H=0) == I and _error(r) == "none of rgb / depth / acc / weights_coarse / z_fine / raw_fine requested"
        for name in _lib.GRID_OUTPUT_FIELDS[:-1]:       # any one of them is a request
            assert _render_grid(r, _lib.GridOutputs(**{name: 1}), H=0) == I and _error(r) == "bad pose / image / row range", name
        # 3. the camera, with nwe_render's texts, in front of the state
        for kw in (dict(poses=None), dict(n_poses=0), dict(H=0), dict(W=0), dict(rows=(-1, 4)), dict(rows=(0, 5)), dict(rows=(3, 2))):
            assert _render_grid(r, good, **kw) == I and _error(r) == "bad pose / image / row range", kw
        for kw in (dict(fx=0.), dict(fy=-0.)):
            assert _render_grid(r, good, **kw) == I and _error(r) == "fx and fy must be non-zero", kw
        assert _render_grid(r, good, near=2., far=1.) == I and _error(r) == "far < near: the sorted merge of the fine pass needs ascending depths"
        # 4. the ray count
        assert _render_grid(r, good, n_poses=3, H=30000, W=30000, rows=(0, 30000)) == I and _error(r) == "more than 2^31 - 1 rays in one call"
        # 5. the state: the grid, then the sampling; zero rays and a host-only context do not come first
        for rows in ((0, 4), (2, 2)):
            assert _render_grid(r, good, rows=rows) == S
            assert _error(r) == "radiance grid: no grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)"
        _set(r)
        assert _render_grid(r, good) == S and _error(r) == "nwe_set_sampling has not been called"
        # 6. last, the device
        r.set_sampling(8, 8)
        for rows in ((0, 4), (2, 2)):
            assert _render_grid(r, good, rows=rows) == S and _error(r) == "needs a device context"
        with pytest.raises(RuntimeError, match="nwe_render_grid: needs a device context"):
            r.render_grid(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5.)
        with pytest.raises(ValueError, match="unknown grid outputs"):
            r.render_grid(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., outputs=("rgb", "disp"))
        r.clear_radiance_grid()
        assert _render_grid(r, good) == S and "no grid is set" in _error(r)
    finally:
        r.close()


def test_the_host_side_refusals_of_the_bake():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    try:
        # a host-only context comes first, whatever else is wrong
        assert lib.nwe_bake_radiance_grid(r._ctx, None, None, None, 7, None, 9, None) == _lib.NWE_ERR_STATE and _error(r) == "needs a device context"
        assert lib.nwe_bake_radiance_grid(None, None, None, None, 7, None, 9, None) == _lib.NWE_ERR_STATE
        with pytest.raises(RuntimeError, match="needs a device context"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4)
        with pytest.raises(ValueError, match="unknown precision"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, precision="f64")
        with pytest.raises(ValueError, match="three coordinates"):
            r.bake_radiance_grid((0, 0, 0), (1, 1, 1), 4, view_dir=(1, 0))
    finally:
        r.close()


# ---- the grid changes nothing else ----------------------------------------------------------------------------------------------

def _plan(r, n_rays, outputs=("rgb",), cus=256, pinhole=True, precision=_lib.PREC_F16X3):
    report = _lib.PlanReport()
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, 1, n_rays, 0, 1, -1 if pinhole else n_rays, C.byref(_lib.Outputs(**{k: 1 for k in outputs})), 0,
                                    precision, cus, C.byref(report))
    return rc, bytes(report), _error(r) if rc else ""


@pytest.mark.parametrize("ni", [8, 0])
def test_a_radiance_grid_moves_no_plan_of_a_render_call(ni):
    r = nwe_amd.Renderer(host_only=True)
    try:
        _networks(r)
        r.set_sampling(8, ni)
        calls = [dict(n_rays=n, pinhole=pinhole, precision=precision, outputs=outputs)
                 for n in (481, 100000) for pinhole in (True, False) for precision in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32)
                 for outputs in (("rgb", "depth", "acc"),)]
        calls.append(dict(n_rays=481, outputs=("rgb", "weights_coarse")))
        before = [_plan(r, **kw) for kw in calls]
        assert all(rc == _lib.NWE_OK for rc, _, _ in before)
        _set(r)
        assert [_plan(r, **kw) for kw in calls] == before
        # nor a refusal: a mode's refusal reads as it read
        r.set_early_termination(0.01)
        refused = _plan(r, 481, ("rgb", "z_std"))
        r.clear_radiance_grid()
        assert refused[0] == _lib.NWE_ERR_UNSUPPORTED and _plan(r, 481, ("rgb", "z_std")) == refused and "radiance" not in refused[2]
    finally:
        r.close()


# ---- the handler ----------------------------------------------------------------------------------------------------------------

def test_handler_arguments_and_environment(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    box = {"lo": R.BOX_LO, "hi": R.BOX_HI}
    monkeypatch.delenv("NWE_RADIANCE_GRID", raising=False)
    assert H("office_geneve", "x.ckpt")._radiance_grid is None
    assert H("office_geneve", "x.ckpt", radiance_grid=box)._radiance_grid == dict(box, resolution=128, which="fine", view_dir=None)
    h = H("office_geneve", "x.ckpt", radiance_grid=dict(box, resolution=(8, 9, 10), which="coarse", view_dir=(0, 0, 1)))
    assert (h._radiance_grid["resolution"], h._radiance_grid["which"], h._radiance_grid["view_dir"]) == ((8, 9, 10), "coarse", (0, 0, 1))
    monkeypatch.setenv("NWE_RADIANCE_GRID", "64")
    assert H("office_geneve", "x.ckpt", radiance_grid=box)._radiance_grid["resolution"] == 64
    assert H("office_geneve", "x.ckpt")._radiance_grid is None          # without a box there is no grid
    monkeypatch.setenv("NWE_RADIANCE_GRID", "64,2")
    with pytest.raises(ValueError, match="NWE_RADIANCE_GRID"):
        H("office_geneve", "x.ckpt", radiance_grid=box)
    monkeypatch.delenv("NWE_RADIANCE_GRID")
    for kw in ({"lo": R.BOX_LO}, {"hi": R.BOX_HI}, dict(box, probes=2)):
        with pytest.raises(ValueError, match="radiance_grid"):
            H("office_geneve", "x.ckpt", radiance_grid=kw)
    from nwe_amd import handler as Hm
    with pytest.raises(ValueError, match="one device"):
        H("office_geneve", "x.ckpt", radiance_grid=box, devices=[0, 0])
    # it is no mode of a frame: every other option goes with it
    H("office_geneve", "x.ckpt", radiance_grid=box, early_termination=1e-2)
    H("office_geneve", "x.ckpt", radiance_grid=box, baked_coarse=box)
    h = H("office_geneve", "x.ckpt", radiance_grid=box)
    for call in (lambda: h.bake_radiance_grid(R.BOX_LO, R.BOX_HI, 8), h.clear_radiance_grid, lambda: h.radiance_grid,
                 lambda: h.render_grid(np.eye(4)), lambda: h.render_coordinates(Hm.COORD(), Hm.COORD(), preview="grid")):
        with pytest.raises(RuntimeError, match="initialize_models"):
            call()


class _FakeRenderer:
    """The Renderer boundary of the handler's grid calls: records them, renders zeros."""

    def __init__(self, device=0, host_only=False):
        self.calls, self.radiance_grid, self.device = [], None, torch.device("cpu")
        self.n_samples = self.n_importance = 0

    def __getattr__(self, name):
        if name.startswith("set_") or name.startswith("debug_set_"):
            return lambda *a, **k: self.calls.append((name,) + a)
        raise AttributeError(name)

    def mfma_supported(self, which):
        return True

    shapes = {0: (4, 128, 63, 27, -1), 1: (4, 128, 63, 27, -1)}

    def bake_radiance_grid(self, lo, hi, resolution, which, view_dir, precision):
        self.calls.append(("bake_radiance_grid", tuple(lo), tuple(hi), resolution, which, view_dir, precision))
        self.radiance_grid = {"lo": tuple(lo), "hi": tuple(hi), "resolution": resolution}

    def clear_radiance_grid(self):
        self.calls.append(("clear_radiance_grid",))
        self.radiance_grid = None

    def _frame(self, name, poses, H, W, rows, outputs):
        self.calls.append((name, H, W, rows, tuple(outputs)))
        n = len(poses) * ((rows[1] - rows[0]) if rows else H) * W
        return {"rgb": torch.full((n, 3), 0.5), "flags": torch.zeros(1, dtype=torch.int32)}

    def render_grid(self, poses, H, W, *, fx, fy, cx, cy, near, far, rows=None, outputs=()):
        return self._frame("render_grid", poses, H, W, rows, outputs)

    def render(self, poses, H, W, *, fx, fy, cx, cy, near, far, rows=None, precision="f16x3", outputs=()):
        return self._frame("render", poses, H, W, rows, outputs)

    def to8b(self, rgb):
        return (255 * rgb.clamp(0, 1)).to(torch.uint8)


def test_handler_renders_previews_from_the_grid(monkeypatch):
    from nwe_amd import handler as Hm
    monkeypatch.setattr(Hm, "Renderer", _FakeRenderer)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"synchronize": lambda self: None})())
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, _e=torch.empty, **k: _e(*a, **k))
    monkeypatch.delenv("NWE_RADIANCE_GRID", raising=False)
    sd = synthetic.make_state_dict(1, 4, 128)
    h = Hm.NeRFReplicaInferenceHandler("office_geneve", "x.ckpt", radiance_grid={"lo": R.BOX_LO, "hi": R.BOX_HI, "resolution": 16, "view_dir": (0, 1, 0)})
    h.initialize_models(state_dicts=(sd, sd))
    r = h.renderer
    assert ("bake_radiance_grid", R.BOX_LO, R.BOX_HI, 16, _lib.NET_FINE, (0, 1, 0), "f16x3") in r.calls and h.radiance_grid is not None
    Himg, Wimg = h.image_size
    coords = Hm.COORD()
    # preview="grid" renders from the grid; preview=True and False take the paths they took
    r.calls.clear()
    img = h.render_coordinates(coords, coords, preview="grid")
    assert img.shape == (Himg, Wimg, 3) and img.dtype == np.uint8 and (img == 127).all()
    assert [c[0] for c in r.calls] == ["render_grid"] and r.calls[0][1:] == (Himg, Wimg, (0, Himg), ("rgb",))
    r.calls.clear()
    h.render_coordinates(coords, coords, preview=True)
    assert [c[0] for c in r.calls] == ["set_sampling", "render", "set_sampling"] and r.calls[0][1:] == (h._n_samples, 0)
    r.calls.clear()
    h.render_coordinates(coords, coords)
    assert [c[0] for c in r.calls] == ["render"]
    r.calls.clear()
    out = h.render_grid(np.eye(4), 6, 8, rows=(1, 4), outputs=("rgb",))
    assert r.calls == [("render_grid", 6, 8, (1, 4), ("rgb",))] and tuple(out["rgb"].shape) == (3, 8, 3)
    assert tuple(h.render_grid_batch(np.stack([np.eye(4)] * 2), 6, 8, outputs=("rgb",))["rgb"].shape) == (2, 6, 8, 3)
    with pytest.raises(ValueError, match="preview must be"):
        h.render_coordinates(coords, coords, preview="fast")
    # without a grid preview="grid" raises by name, and renders nothing
    h.clear_radiance_grid()
    r.calls.clear()
    with pytest.raises(RuntimeError, match="bake_radiance_grid"):
        h.render_coordinates(coords, coords, preview="grid")
    assert r.calls == []


# ---- the parity scene -----------------------------------------------------------------------------------------------------------

def test_the_parity_scene_is_well_conditioned():
    """grid_render in fp32 and in fp64 agree within the parity tolerance on EVERY ray: the scene's reference reproduces itself, so the
    kernel can be held to it on every ray.  Every sample lies inside the box (the rule is discontinuous at its faces) and every
    coarse bin carries weight."""
    cfg, _, rays, _, _ = R.scene(R.PARITY_SCENE)
    g = R.grid(R.PARITY_GRID)
    a, b = R.parity_reference(), R.parity_reference(fp64=True)
    for k in ("rgb", "depth", "acc"):
        err = (a[k].double() - b[k]).abs()
        print(f"radiance grid parity scene, fp32 against fp64 {k}: {float(err.max()):.2e} (tol {TOL[k]:.0e})")
        assert float(err.max()) <= TOL[k], k
    lo, hi = g["lo"].astype(np.float64), g["hi"].astype(np.float64)
    for z in (a["z_fine"].numpy(), b["z_fine"].numpy()):
        pts = rays[:, None, 0:3].numpy() + rays[:, None, 3:6].numpy() * z[..., None]
        assert (pts > lo + 1e-3).all() and (pts < hi - 1e-3).all()
    assert float(a["weights"][:, 1:-1].min()) > 1e-3 and float(a["acc"].min()) > 0.05
    assert float(a["rgb"].std()) > 0.01          # the colour varies over the frame
    # with n_importance == 0 the only pass is the output: the coarse composite
    cfg0 = type(cfg)(n_samples=cfg.n_samples, n_importance=0)
    single = R.grid_render(rays, cfg0, g)
    assert torch.equal(single["weights"], a["weights"]) and tuple(single["raw_fine"].shape) == (rays.shape[0], cfg.n_samples, 4)
