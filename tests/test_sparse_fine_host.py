"""The sparse frame without a GPU (include/nwe.h: nwe_render_sparse): every refusal in front of the host-only one, by code, text and
order; that a refused call writes nothing and moves no report; that nothing sparse moves a plan of a render call; the numpy
selection rule of tests/sparse_fine.py against a slow loop; the handler's arguments; the room scene of nwe_amd.synthetic against
the oracle; and the conditioning of the parity scene of tests/test_gpu_sparse_fine.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from tests import radiance_grid as R
from tests import sparse_fine as SF

TOL = {"rgb": 1e-4, "depth": 1e-4 * R.FAR, "acc": 1e-4}     # the project's parity tolerances (tests/test_gpu_radiance_grid.py)
NAN = float("nan")


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _set(r, kind="random"):
    g = R.grid(kind)
    r.set_radiance_grid(g["values"], g["lo"], g["hi"])


def _render_sparse(r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4), which=1,
                   precision=_lib.PREC_F16X3, min_weight=1e-3, dilate=1):
    ptr = None if poses is None else poses.ctypes.data
    return _lib.load().nwe_render_sparse(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0], rows[1],
                                         which, precision, min_weight, dilate, None if out is None else C.byref(out), None)


def _reports(r):
    lib = _lib.load()
    counts = (C.c_int64 * 2)(-7, -7)
    return (lib.nwe_last_kernel_ms(r._ctx), lib.nwe_debug_last_plan(r._ctx), lib.nwe_last_query_ms(r._ctx), lib.nwe_last_grid_ms(r._ctx),
            lib.nwe_last_sparse_ms(r._ctx), lib.nwe_last_sparse_samples(r._ctx, counts), tuple(counts))


def test_every_refusal_in_front_of_the_host_only_one():
    """Code, text and order: each call below is wrong in everything behind the refusal it expects as well."""
    r = nwe_amd.Renderer(host_only=True)
    I, S = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE
    bad = dict(which=2, precision=9, min_weight=NAN, dilate=9)       # 4. to 7. all wrong
    try:
        buf = np.full(60, 123.0, np.float32)
        good = _lib.SparseOutputs(rgb=buf.ctypes.data)
        none = _lib.SparseOutputs(flags=1)
        stale = _lib.SparseOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.SparseOutputs) - 8
        before = _reports(r)
        # 1. the context - whatever else is wrong
        assert _render_sparse(None, None, poses=None, **bad) == I
        # 2. the outputs, in front of the camera (H = 0)
        assert _render_sparse(r, None, H=0, **bad) == I and _error(r) == "null outputs"
        assert _render_sparse(r, stale, H=0, **bad) == I and _error(r).startswith("nwe_sparse_outputs.struct_bytes != sizeof(nwe_sparse_outputs)")
        assert _render_sparse(r, none, H=0, **bad) == I
        assert _error(r) == "none of rgb / depth / acc / weights_coarse / z_fine / weights_grid / selected / raw_fine requested"
        for name in _lib.SPARSE_OUTPUT_FIELDS[:-1]:       # any one of them is a request
            assert _render_sparse(r, _lib.SparseOutputs(**{name: 1}), H=0, **bad) == I and _error(r) == "bad pose / image / row range", name
        # 3. the camera and the ray count, with nwe_render's texts
        for kw in (dict(poses=None), dict(n_poses=0), dict(H=0), dict(W=0), dict(rows=(-1, 4)), dict(rows=(0, 5)), dict(rows=(3, 2))):
            assert _render_sparse(r, good, **kw, **bad) == I and _error(r) == "bad pose / image / row range", kw
        for kw in (dict(fx=0.), dict(fy=-0.)):
            assert _render_sparse(r, good, **kw, **bad) == I and _error(r) == "fx and fy must be non-zero", kw
        assert _render_sparse(r, good, near=2., far=1., **bad) == I
        assert _error(r) == "far < near: the sorted merge of the fine pass needs ascending depths"
        assert _render_sparse(r, good, n_poses=3, H=30000, W=30000, rows=(0, 30000), **bad) == I
        assert _error(r) == "more than 2^31 - 1 rays in one call"
        # 4. to 7. the arguments of the call, each in front of the next
        for which in (2, -1):
            assert _render_sparse(r, good, **dict(bad, which=which)) == I and _error(r) == "which must be 0 or 1"
        assert _render_sparse(r, good, **dict(bad, which=0)) == I and _error(r) == "unknown precision"
        assert _render_sparse(r, good, **dict(bad, which=1, precision=_lib.PREC_F32)) == I and _error(r) == "sparse frame: min_weight must not be NaN"
        for dilate in (9, -1):
            assert _render_sparse(r, good, dilate=dilate) == I and _error(r) == "sparse frame: dilate must be in 0..8"
        # 8. to 10. the state: the grid, the sampling, the network; zero rays and a host-only context do not come first
        for kw in (dict(rows=(0, 4)), dict(rows=(2, 2)), dict(dilate=0, min_weight=-np.inf), dict(dilate=8, min_weight=np.inf)):
            assert _render_sparse(r, good, **kw) == S
            assert _error(r) == "sparse frame: no radiance grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)"
        _set(r)
        assert _render_sparse(r, good) == S and _error(r) == "nwe_set_sampling has not been called"
        r.set_sampling(8, 8)
        assert _render_sparse(r, good) == S and _error(r) == "sparse frame: the fine network is not set"
        assert _render_sparse(r, good, which=0) == S and _error(r) == "sparse frame: the coarse network is not set"
        r.set_network(0, synthetic.make_state_dict(5, 3, 64, skips=()))     # a shape without an MFMA kernel; the upload clears the grid
        assert _render_sparse(r, good, which=0) == S and "no radiance grid is set" in _error(r)
        _set(r)
        assert _render_sparse(r, good, which=1) == S and _error(r) == "sparse frame: the fine network is not set"
        # 11. the device, in front of 12. the shape without a query kernel - which a host-only context therefore never reports
        for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
            for rows in ((0, 4), (2, 2)):
                assert _render_sparse(r, good, which=0, precision=precision, rows=rows) == S and _error(r) == "needs a device context"
        with pytest.raises(RuntimeError, match="nwe_render_sparse: needs a device context"):
            r.render_sparse(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., which=0)
        with pytest.raises(ValueError, match="unknown sparse outputs"):
            r.render_sparse(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., outputs=("rgb", "disp"))
        # a refused call leaves the outputs and all reports untouched
        assert (buf == 123.0).all() and _reports(r) == before
        assert before[4] < 0 and before[5] == _lib.NWE_ERR_STATE and before[6] == (-7, -7)
        assert r.last_sparse_ms() is None and r.last_sparse_samples() is None
    finally:
        r.close()


def _plan(r, n_rays, outputs=("rgb",), cus=256, pinhole=True, precision=_lib.PREC_F16X3):
    report = _lib.PlanReport()
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, 1, n_rays, 0, 1, -1 if pinhole else n_rays, C.byref(_lib.Outputs(**{k: 1 for k in outputs})), 0,
                                    precision, cus, C.byref(report))
    return rc, bytes(report), _error(r) if rc else ""


def test_nothing_sparse_moves_a_plan_of_a_render_call():
    r = nwe_amd.Renderer(host_only=True)
    try:
        for which in (0, 1):
            r.set_network(which, synthetic.make_state_dict(1000 + which, 4, 128))
        r.set_sampling(8, 8)
        calls = [dict(n_rays=n, pinhole=pinhole, precision=p) for n in (481, 100000) for pinhole in (True, False)
                 for p in (_lib.PREC_F16X3, _lib.PREC_F32)]
        before = [_plan(r, **kw) for kw in calls]
        assert all(rc == _lib.NWE_OK for rc, _, _ in before)
        r.debug_set_sparse_chunk(64)
        assert [_plan(r, **kw) for kw in calls] == before
        _set(r)
        _render_sparse(r, _lib.SparseOutputs(rgb=1))         # refused by the device alone
        assert _error(r) == "needs a device context" and [_plan(r, **kw) for kw in calls] == before
        r.debug_set_sparse_chunk(0)
        for bad in (-1, -100):
            with pytest.raises(ValueError):
                r.debug_set_sparse_chunk(bad)
        assert [_plan(r, **kw) for kw in calls] == before
    finally:
        r.close()


# ---- the selection rule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dilate", [0, 1, 8])
@pytest.mark.parametrize("min_weight", [-1.0, 0.0, 1e-3, 2.0])
def test_the_selection_helper_against_a_slow_loop(min_weight, dilate):
    rng = np.random.default_rng(11)
    for S in (2, 4, 13, 40):
        w = (rng.random((60, S)) ** 6 * 0.02).astype(np.float32)
        w[rng.random((60, S)) < 0.5] = 0.0
        w[0] = 0.0
        w[1], w[2] = 0.0, 0.0
        w[1, 0], w[2, -1] = 0.5, 0.5                   # a hit at either end
        w[3] = 0.0
        w[3, S // 2] = NAN                             # a NaN weight is a hit
        w[4] = 1e-3                                    # equal to the threshold is no hit
        got, want = SF.select(w, min_weight, dilate), SF.select_slow(w, min_weight, dilate)
        assert got.dtype == bool and np.array_equal(got, want), (S, min_weight, dilate)
        if min_weight < 0:
            assert got.all()
        elif min_weight == 2.0:
            assert got[3].any() and not np.delete(got, 3, 0).any()
        else:
            assert not got[0].any() and got[3, S // 2]
            assert got[1, :dilate + 1].all() and not got[1, dilate + 1:].any()
            assert got[2, S - 1 - dilate:].all() and not got[2, :max(S - 1 - dilate, 0)].any()
            assert got[4].any() == (min_weight < 1e-3)


def test_points_round_the_product_and_the_sum_separately():
    rays = np.float32([[0.1, 0.2, 0.3, 0.7, -0.3, 1.0 / 3, 0, 0]])
    z = np.float32([[1.0 / 3, 7.7]])
    p = SF.points(rays, z)
    want = np.float32([[[np.float32(0.1) + np.float32(np.float32(d) * np.float32(zz)) for o, d in ((0.1, 0.7),)] for zz in z[0]]])
    assert p.dtype == np.float32 and p.shape == (1, 2, 3) and np.array_equal(p[..., :1], want)


# ---- the handler ----------------------------------------------------------------------------------------------------------------

def test_handler_arguments_and_environment(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    box = {"lo": R.BOX_LO, "hi": R.BOX_HI}
    monkeypatch.delenv("NWE_SPARSE_FINE", raising=False)
    monkeypatch.delenv("NWE_RADIANCE_GRID", raising=False)
    assert H("office_geneve", "x.ckpt")._sparse_fine is None and H("office_geneve", "x.ckpt", radiance_grid=box)._sparse_fine is None
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={})._sparse_fine == {"min_weight": 1e-3, "dilate": 1, "which": "fine"}
    h = H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={"min_weight": 0.01, "dilate": 3, "which": "coarse"})
    assert h._sparse_fine == {"min_weight": 0.01, "dilate": 3, "which": "coarse"}
    with pytest.raises(ValueError, match="needs a radiance grid"):
        H("office_geneve", "x.ckpt", sparse_fine={})
    with pytest.raises(ValueError, match="one device"):
        H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={}, devices=[0, 0])
    for opt in ({"threshold": 1}, {"dilate": 9}, {"dilate": -1}, {"dilate": 1.5}, {"dilate": True}, {"min_weight": NAN}, {"min_weight": "x"},
                {"which": "both"}):
        with pytest.raises(ValueError, match="sparse_fine"):
            H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine=opt)
    monkeypatch.setenv("NWE_SPARSE_FINE", "0.02")
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={"dilate": 2})._sparse_fine == {"min_weight": 0.02, "dilate": 2, "which": "fine"}
    monkeypatch.setenv("NWE_SPARSE_FINE", "1e-4, 0")
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={"dilate": 2})._sparse_fine == {"min_weight": 1e-4, "dilate": 0, "which": "fine"}
    assert H("office_geneve", "x.ckpt", radiance_grid=box)._sparse_fine == {"min_weight": 1e-4, "dilate": 0, "which": "fine"}
    for env in ("1,2,3", "x", "0.1,y", "0.1,9", "nan"):
        monkeypatch.setenv("NWE_SPARSE_FINE", env)
        with pytest.raises(ValueError, match="NWE_SPARSE_FINE|sparse_fine"):
            H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={})
    monkeypatch.delenv("NWE_SPARSE_FINE")
    from nwe_amd import handler as Hm
    h = H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={})
    for call in (lambda: h.render_sparse(np.eye(4)), lambda: h.render_sparse_batch(np.eye(4)[None]), h.last_sparse_samples,
                 lambda: h.render_coordinates(Hm.COORD(), Hm.COORD())):
        with pytest.raises(RuntimeError, match="initialize_models"):
            call()
    # preview values and their error text stay as they are
    with pytest.raises((ValueError, RuntimeError), match="initialize_models|preview must be False, True or 'grid'"):
        h.render_coordinates(Hm.COORD(), Hm.COORD(), preview="sparse")


# ---- the room -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,width,view_dirs", [(4, 128, True), (8, 256, True), (4, 128, False)])
def test_the_room_is_empty_inside_and_dense_behind_its_walls(depth, width, view_dirs):
    """Against the oracle's restatement of NeRFModel: sigma_raw < 0 at 1 000 interior points, > 0 half a unit behind each wall."""
    sd = SF.room_net(depth, width, view_dirs)
    rng = np.random.default_rng(5)
    inside = rng.uniform(-2.95, 2.95, (1000, 1, 3)).astype(np.float32)
    dirs = None
    if view_dirs:
        d = rng.normal(size=(1000, 3))
        dirs = torch.from_numpy((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))
    sigma = SF.oracle_rows(sd, inside, dirs)[..., 3]
    assert tuple(sigma.shape) == (1000, 1) and float(sigma.max()) < 0.0
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = rng.uniform(-2.5, 2.5, (100, 1, 3)).astype(np.float32)
            p[..., axis] = sign * 3.5
            behind = SF.oracle_rows(sd, p, None if dirs is None else dirs[:100])[..., 3]
            assert float(behind.min()) > 0.0, (axis, sign)
    # the copy shares nothing with the state it was made from, and the colours are still a network's
    base = synthetic.make_state_dict(1001, depth, width, use_view_dirs=view_dirs)
    again = synthetic.make_state_dict(1001, depth, width, use_view_dirs=view_dirs)
    (synthetic.room if view_dirs else synthetic.room_output)(base)
    assert all(np.array_equal(base[k], again[k]) for k in base)
    assert float(SF.oracle_rows(sd, inside, dirs)[..., :3].std()) > 1e-3


# ---- the parity scene -----------------------------------------------------------------------------------------------------------

def test_the_parity_scene_is_well_conditioned():
    """The oracle alone: its float32 and float64 evaluations agree to a tenth of the parity tolerance on the rays that are kept, and the
    rays left out - a weight within 1e-6 of min_weight - are at most 1 % of the frame; both values of the mask occur."""
    a, b = SF.parity_reference(), SF.parity_reference(True)
    keep = a["margin"] >= SF.PARITY_MARGIN
    left_out = float((~keep).float().mean())
    print(f"parity scene: {left_out:.4f} of the rays left out, selected share {float(a['selected'].float().mean()):.3f}")
    assert left_out <= SF.PARITY_CAP
    assert bool((a["selected"][keep] == b["selected"][keep]).all())
    for k in ("rgb", "depth", "acc"):
        err = float((a[k] - b[k].float()).abs()[keep].max())
        print(f"parity scene {k}: fp32 against fp64 {err:.2e}")
        assert err <= 0.1 * TOL[k], k
    sel = a["selected"]
    assert bool(sel.any()) and bool((~sel).any()) and 0.05 < float(sel.float().mean()) < 0.95


# ---- the stand-alone program ----------------------------------------------------------------------------------------------------

def test_sparse_smoke_builds_and_runs_from_plain_c(tmp_path):
    """tests/c/sparse_smoke.c against the product library, without sanitizers (`make asan` runs it with them)."""
    cc = "gcc"                                          # as tests/test_abi.py builds abi_smoke.c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "sparse_smoke")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "sparse_smoke.c"),
                    "-o", exe, "-L", lib_dir, "-lnwe_hip", "-lm", f"-Wl,-rpath,{lib_dir}"], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "sparse_smoke ok" in res.stdout, res.stderr
