"""The point query on the GPU (include/nwe.h: nwe_query_points; run_network of nerf/models/model_utils.py:13-30): every
comparison but the first is bitwise.  The yardstick is "the ray trick" of tests/test_gpu_parity.py: one ray per point with
o = p, near = far = 0 and n_samples = 2, whose raw_coarse[:, 0] is the network at p with the ray's view-direction columns -
the only way to ask a network about a point before the query existed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from tests import mode_domain as M

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16x3", "f16x1", "f32")
# every built shape: the list the mode-domain tests iterate, and the two of the reference formulation (debug_set_fold(False))
SHAPES = [(M.kind(D, W, form), D, W, form != "no_view_dirs", True) for D, W, form in M.SHAPES] + \
         [("8x256-unfolded", 8, 256, True, False), ("4x128-unfolded", 4, 128, True, False)]
COUNTS = (1, 31, 32, 33, 127, 128, 129, 257, 300)
STEPS = (1, 2, 3, 0)          # forced, and automatic


def _sd(seed, D, W, view=True):
    return nwe_amd.synthetic.make_state_dict(seed, D, W, use_view_dirs=view)


def _renderer(nets, fold=True, sampling=(2, 0)):
    """nets: {which: state dict}."""
    r = nwe_amd.Renderer(0)
    if not fold:
        r.debug_set_fold(False)
    for which, sd in nets.items():
        r.set_network(which, sd)
    if sampling:
        r.set_sampling(*sampling)
    return r


def _cloud(seed, n):
    """n points in a scene-sized box and n unit directions; no negative zero (the trick's o + d * 0 would turn it into +0)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    dirs = rng.normal(size=(n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    assert not np.signbit(pts[pts == 0]).any()
    return pts, dirs


def _trick(r, pts, dirs, precision):
    """raw [n,4] through nwe_render_rays on network 0 of a context with set_sampling(2, 0); the ray direction is `dirs` too
    (it is multiplied by z = 0)."""
    n = pts.shape[0]
    cols = [pts, dirs, np.zeros((n, 2), np.float32)] + ([dirs] if r.ray_columns == 11 else [])
    rays = torch.from_numpy(np.concatenate(cols, 1).astype(np.float32)).cuda()
    raw = r.render_rays(rays, precision=precision, outputs=("raw_coarse",))["raw_coarse"]
    assert torch.equal(raw[:, 0], raw[:, 1])
    return raw[:, 0].cpu().numpy()


def _query(r, pts, dirs, precision, which=0, outputs=("raw",)):
    res = r.query_points(torch.from_numpy(pts).cuda(), None if dirs is None else torch.from_numpy(dirs).cuda(), which=which,
                         precision=precision, outputs=outputs)
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


def _query_abi(r, pts, dirs, ppd, precision, which=0):
    """raw [n,4] and the flag word through the C ABI itself: any points_per_dir."""
    p = torch.from_numpy(pts).cuda()
    d = torch.from_numpy(dirs).cuda()
    raw = torch.empty((pts.shape[0], 4), dtype=torch.float32, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    o = _lib.PointOutputs(raw=raw.data_ptr(), flags=flags.data_ptr())
    rc = r._lib.nwe_query_points(r._ctx, which, p.data_ptr(), pts.shape[0], d.data_ptr(), ppd, _lib.PRECISIONS[precision], C.byref(o),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, r._lib.nwe_last_error(r._ctx)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), int(flags.item())


def _same(a, b):
    """Bitwise, NaN included."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the reference's own vectors ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag,D,Wn,seed", [("4x128", 4, 128, 1000), ("8x256", 8, 256, 1001)])
def test_reference_mlp_vectors_through_the_query(golden_dir, precision, tag, D, Wn, seed):
    """tests/golden/mlp.npz - the reference's NeRFModel on gamma of embed.npz's points and directions (|x| ~ 20, -0.0, 1e-8
    among them) - through query_points: within the 5e-6 that test_reference_mlp_vectors_through_the_kernels applies to these
    very vectors, and the bits of the ray trick on the same context."""
    ge, gm = np.load(os.path.join(golden_dir, "embed.npz")), np.load(os.path.join(golden_dir, "mlp.npz"))
    y = gm[f"y_{tag}"]
    pts, dirs = np.concatenate([ge["pts"]] * 2, 0), np.concatenate([ge["dirs"]] * 2, 0)
    r = _renderer({0: _sd(seed, D, Wn)})
    try:
        got = _query(r, pts, dirs, precision)
        err = np.abs(got["raw"] - y)
        print(f"[{precision} {tag}] query vs reference NeRFModel: max {err.max():.2e}")
        assert got["flags"][0] == 0
        assert err.max() <= 5e-6
        assert np.array_equal(got["raw"], _trick(r, pts, dirs, precision))
    finally:
        r.close()


# ---- 2. every built shape ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,D,Wn,view,fold", SHAPES, ids=[s[0] for s in SHAPES])
def test_query_equals_the_ray_trick_on_every_built_shape(name, D, Wn, view, fold, precision):
    """Point counts around the wave (32), the packet (128) and two packets, with the steps per workgroup forced to 1, 2 and 3
    and automatic: one workgroup walking several packets, several workgroups, ragged last packets and waves without a point."""
    pts, dirs = _cloud(D * 1000 + Wn, max(COUNTS))
    r = _renderer({0: _sd(1000, D, Wn, view)}, fold=fold)
    try:
        assert r.mfma_supported(0)
        for n in COUNTS:
            want = _trick(r, pts[:n], dirs[:n], precision)
            assert np.isfinite(want).all()
            for steps in STEPS:
                r.debug_set_query_steps(steps)
                got = _query(r, pts[:n], dirs[:n] if view else None, precision)
                assert got["flags"][0] == 0 and got["raw"].shape == (n, 4)
                assert np.array_equal(got["raw"], want), (n, steps)
    finally:
        r.close()


# ---- 3. sigma only ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D,Wn,view", [(8, 256, True), (6, 256, True), (8, 256, False), (4, 128, False)],
                         ids=["8x256-density-only-built", "6x256-full-evaluation", "8x256-noview", "4x128-noview"])
def test_sigma_alone_has_the_bits_of_the_full_query(D, Wn, view, precision):
    """outputs=("sigma",) against raw[..., 3]: where the density-only evaluation is built (8x256 folded) and where the full
    evaluation runs and drops the colour (6x256 folded: its skip input enters the last trunk layer), with and without a
    direction, on networks without view directions, and beside raw in one call."""
    assert M.density_only(8, 256, "folded") and not M.density_only(6, 256, "folded")
    pts, dirs = _cloud(77, 300)
    r = _renderer({0: _sd(1002, D, Wn, view)}, sampling=None)       # a query needs no sampling tables
    try:
        r.debug_set_query_steps(2)
        d = dirs if view else None
        full = _query(r, pts, d, precision)["raw"]
        both = _query(r, pts, d, precision, outputs=("raw", "sigma"))
        assert np.array_equal(both["raw"], full) and np.array_equal(both["sigma"], full[:, 3])
        assert np.array_equal(_query(r, pts, d, precision, outputs=("sigma",))["sigma"], full[:, 3])
        if view:
            assert np.array_equal(_query(r, pts, None, precision, outputs=("sigma",))["sigma"], full[:, 3])
            assert np.array_equal(_query(r, pts, dirs[::-1].copy(), precision, outputs=("sigma",))["sigma"], full[:, 3])
    finally:
        r.close()


# ---- 4. direction indexing --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_points_per_dir_equals_the_expanded_directions(precision):
    """Point i takes direction i / points_per_dir: 1, 3, 7 (divides neither a wave nor a packet), 64 (spans waves), n and more
    than n, each against the same query with one direction per point, at n = 300 with two steps per workgroup."""
    n = 300
    pts, dirs = _cloud(5, n)
    r = _renderer({0: _sd(1003, 4, 128)}, sampling=None)
    try:
        r.debug_set_query_steps(2)
        for ppd in (1, 3, 7, 64, n, n + 11):
            rows = -(-n // ppd)
            expanded = np.ascontiguousarray(dirs[np.arange(n) // ppd])
            want, _ = _query_abi(r, pts, expanded, 1, precision)
            got, flags = _query_abi(r, pts, np.ascontiguousarray(dirs[:rows]), ppd, precision)
            assert flags == 0 and np.array_equal(got, want), ppd
        # the layout run_network has: [N,S,3] against [N,3]
        N, S = 20, 15
        got = _query(r, pts.reshape(N, S, 3), dirs[:N], precision)["raw"]
        assert got.shape == (N, S, 4)
        assert np.array_equal(got.reshape(n, 4), _query_abi(r, pts, np.ascontiguousarray(np.repeat(dirs[:N], S, 0)), 1, precision)[0])
    finally:
        r.close()


# ---- 5. locality ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D,Wn,view", [(4, 128, True), (8, 256, False)], ids=["4x128", "8x256-noview"])
def test_rows_do_not_depend_on_the_rows_around_them(D, Wn, view, precision):
    pts, dirs = _cloud(6, 300)
    r = _renderer({0: _sd(1004, D, Wn, view)}, sampling=None)
    try:
        whole = _query(r, pts, dirs if view else None, precision, outputs=("raw", "sigma"))
        for a, b, steps in ((37, 203, 0), (1, 300, 2), (131, 132, 0), (95, 290, 1)):
            r.debug_set_query_steps(steps)
            part = _query(r, pts[a:b], dirs[a:b] if view else None, precision, outputs=("raw", "sigma"))
            assert np.array_equal(part["raw"], whole["raw"][a:b]) and np.array_equal(part["sigma"], whole["sigma"][a:b]), (a, b)
    finally:
        r.close()


# ---- 6. two shapes in one context -------------------------------------------------------------------------------------------

def test_two_mfma_shapes_in_one_context_answer_queries_and_still_refuse_to_render():
    sd_c, sd_f = _sd(1005, 4, 128), _sd(1006, 8, 256)
    pts, dirs = _cloud(8, 300)
    both = _renderer({0: sd_c, 1: sd_f}, sampling=(8, 8))
    only_c, only_f = _renderer({0: sd_c, 1: sd_c}, sampling=None), _renderer({0: sd_f, 1: sd_f}, sampling=None)
    try:
        assert not both.separate_passes
        for precision in ("f16x3", "f16x1"):
            for which, alone in ((0, only_c), (1, only_f)):
                got = _query(both, pts, dirs, precision, which=which)
                assert got["flags"][0] == 0 and np.isfinite(got["raw"]).all()
                assert np.array_equal(got["raw"], _query(alone, pts, dirs, precision, which=which)["raw"])
                assert np.array_equal(got["raw"], _query(alone, pts, dirs, precision, which=1 - which)["raw"])
        rays = torch.from_numpy(np.concatenate([pts, dirs, np.full((300, 1), 0.1, np.float32), np.full((300, 1), 6.0, np.float32), dirs], 1)).cuda()
        with pytest.raises(NotImplementedError, match="same shape"):
            both.render_rays(rays, precision="f16x3")
        assert both.render_rays(rays, precision="f32")["rgb"].shape == (300, 3)
    finally:
        for r in (both, only_c, only_f):
            r.close()


# ---- 7. a long-lived context ------------------------------------------------------------------------------------------------

def _frame(r, precision="f16x3"):
    from oracle import nerf_oracle as O
    H, W = 12, 20
    fx, fy, cx, cy = O.intrinsics(H, W)
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    return r.render(pose[0].numpy(), H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=6.0, precision=precision)


def test_a_query_moves_nothing_a_render_reports_and_keeps_armed_hooks():
    r = _renderer({0: nwe_amd.synthetic.thin_fog(_sd(1000, 4, 128)), 1: _sd(1001, 4, 128)}, sampling=(8, 8))
    pts, dirs = _cloud(9, 300)
    try:
        assert r.last_query_ms() < 0
        rgb = _frame(r)["rgb"].clone()
        report = lambda: (r.last_kernel_ms(), r.last_launch_parts(), r.debug_last_plan(), r.last_ray_evaluations(), r.debug_last_queue())
        before = report()
        assert before[0] > 0
        q = _query(r, pts, dirs, "f16x3", which=1, outputs=("raw", "sigma"))
        ms = r.last_query_ms()
        assert ms > 0 and report() == before
        # an empty query is no launch: the timing stays
        assert _query(r, pts[:0], dirs[:0], "f16x3", which=1)["raw"].shape == (0, 4) and r.last_query_ms() == ms
        # a render moves no query report, and renders what it rendered
        assert torch.equal(_frame(r)["rgb"], rgb) and r.last_query_ms() == ms
        # a hook armed before a query is still armed behind it, and the next render_rays consumes it
        n = 40
        rays = torch.from_numpy(np.concatenate([pts[:n], dirs[:n], np.full((n, 1), 0.1, np.float32), np.full((n, 1), 6.0, np.float32), dirs[:n]], 1)).cuda()
        table = torch.from_numpy(np.random.default_rng(3).normal(size=(n, 8, 4)).astype(np.float32)).cuda()
        assert r._lib.nwe_debug_set_raw(r._ctx, table.data_ptr(), None) == 0
        again = _query(r, pts, dirs, "f16x3", which=1, outputs=("raw", "sigma"))
        assert np.array_equal(again["raw"], q["raw"]) and np.array_equal(again["sigma"], q["sigma"])
        hooked = r.render_rays(rays, precision="f16x3", outputs=("raw_coarse",))["raw_coarse"]
        assert torch.equal(hooked, table)
        plain = r.render_rays(rays, precision="f16x3", outputs=("raw_coarse",))["raw_coarse"]
        assert not torch.equal(plain, table)
    finally:
        r.close()


def test_set_network_waits_for_a_query_in_flight():
    """65 536 points of the 8x256 network, and at once - no synchronise - other weights for the same network: the query returns
    the old network's values, the ones a synchronised query returned before the swap."""
    n = 65536
    pts, dirs = _cloud(10, n)
    p, d = torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()
    old, new = _sd(1001, 8, 256), _sd(1007, 8, 256)
    r = _renderer({1: old}, sampling=None)
    try:
        first = r.query_points(p, d, which=1)
        torch.cuda.synchronize()
        want = first["raw"].cpu().numpy()
        second = r.query_points(p, d, which=1)
        r.set_network(1, new)                       # repacks and uploads: must wait for `second`
        torch.cuda.synchronize()
        assert np.array_equal(second["raw"].cpu().numpy(), want)
        third = r.query_points(p, d, which=1)["raw"].cpu().numpy()
        assert not np.array_equal(third, want)
        assert r.last_query_ms() > 0
    finally:
        r.close()


# ---- 8. range, and the refusals behind the context check --------------------------------------------------------------------

@pytest.mark.parametrize("D,Wn,view", [(4, 128, True), (4, 128, False)], ids=["4x128", "4x128-noview"])
def test_a_coordinate_out_of_range_is_nan_in_its_row_alone(D, Wn, view):
    """A coordinate of 1e6 (beyond the 5e5 of include/nwe.h): NaN and NWE_FLAG_RAW under f16x3, finite and no flag under f32,
    and the rows around it are those of the query without it."""
    pts, dirs = _cloud(11, 200)
    bad = 77
    hit = pts.copy()
    hit[bad, 1] = 1e6
    keep = np.arange(200) != bad
    r = _renderer({0: _sd(1008, D, Wn, view)}, sampling=None)
    try:
        r.debug_set_query_steps(2)
        for precision in PRECISIONS:
            dd = (lambda a: a) if view else (lambda a: None)
            without = _query(r, pts[keep], dd(dirs[keep]), precision, outputs=("raw", "sigma"))
            got = _query(r, hit, dd(dirs), precision, outputs=("raw", "sigma"))
            assert without["flags"][0] == 0
            assert np.array_equal(got["raw"][keep], without["raw"]) and np.array_equal(got["sigma"][keep], without["sigma"])
            if precision == "f32":
                assert np.isfinite(got["raw"][bad]).all() and got["flags"][0] == 0
            else:
                assert np.isnan(got["raw"][bad]).all() and np.isnan(got["sigma"][bad]) and got["flags"][0] == _lib.NWE_FLAG_RAW
                only_sigma = _query(r, hit, dd(dirs), precision, outputs=("sigma",))
                assert only_sigma["flags"][0] == _lib.NWE_FLAG_RAW and _same(only_sigma["sigma"], got["sigma"])
    finally:
        r.close()


def test_refusals_in_their_order():
    """Behind the context check (tests/test_query_host.py): arguments, precision, network, directions, shape - each refusal
    comes before the ones listed after it, nothing is launched and last_query_ms stays unset."""
    lib = _lib.load()
    r = _renderer({0: _sd(1, 4, 128), 1: _sd(2, 6, 64, False)}, sampling=None)      # 6x64 without view directions: no MFMA kernel
    pts = torch.zeros(4, 3, device="cuda")
    dirs = torch.zeros(4, 3, device="cuda")
    raw = torch.empty(4, 4, device="cuda")
    good = _lib.PointOutputs(raw=raw.data_ptr())
    short = _lib.PointOutputs(raw=raw.data_ptr())
    short.struct_bytes -= 8
    none = _lib.PointOutputs()
    P, D = pts.data_ptr(), dirs.data_ptr()

    def call(which=0, p=P, n=4, d=D, ppd=1, prec=0, out=good):
        rc = lib.nwe_query_points(r._ctx, which, p, n, d, ppd, prec, C.byref(out) if out is not None else None, None)
        return rc, lib.nwe_last_error(r._ctx)
    try:
        INV, UNS, STA = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_UNSUPPORTED, _lib.NWE_ERR_STATE
        # 2. arguments - with an unknown precision and an unset network behind them
        assert call(out=None, prec=9)[0] == INV
        rc, msg = call(out=short, prec=9)
        assert rc == INV and b"struct_bytes" in msg
        for kw in (dict(which=2), dict(which=-1), dict(n=-1), dict(n=1 << 31), dict(ppd=0), dict(p=None), dict(out=none)):
            assert call(prec=9, **kw)[0] == INV, kw
        assert call(n=(1 << 31) - 1, p=None)[0] == INV
        # 3. precision, in front of 4. the network
        empty = nwe_amd.Renderer(0)
        assert lib.nwe_query_points(empty._ctx, 0, P, 4, D, 1, 9, C.byref(good), None) == INV
        assert lib.nwe_query_points(empty._ctx, 0, P, 4, D, 1, 0, C.byref(good), None) == STA
        assert b"network not set" in lib.nwe_last_error(empty._ctx)
        assert lib.nwe_query_points(empty._ctx, 0, P, 0, D, 1, 0, C.byref(good), None) == STA      # also with no points
        empty.close()
        # 5. directions, in front of 6. the shape
        rc, msg = call(which=1, prec=0)                          # no view directions, a pointer given; and no MFMA kernel
        assert rc == INV and b"no view directions" in msg
        rc, msg = call(which=0, d=None)                          # view directions, raw asked for, none given
        assert rc == INV and b"dirs_dev" in msg
        rc, msg = call(which=1, d=None, prec=0)
        assert rc == UNS and b"use NWE_PREC_F32" in msg
        assert call(which=1, d=None, prec=1)[0] == UNS
        assert r.last_query_ms() < 0                              # nothing was launched so far
        assert call(n=0)[0] == 0 and call(n=0, p=None)[0] == 0 and r.last_query_ms() < 0
        # and the calls that are fine
        assert call(which=1, d=None, prec=2)[0] == 0             # the fp32 kernel serves the shape
        assert call(which=0)[0] == 0
        torch.cuda.synchronize()
        assert r.last_query_ms() > 0
        with pytest.raises(NotImplementedError, match="use NWE_PREC_F32"):
            r.query_points(pts, None, which=1)
        with pytest.raises(ValueError, match="dirs_dev"):
            r.query_points(pts, None, which=0)
    finally:
        r.close()


def test_the_fp32_query_serves_shapes_without_an_mfma_kernel():
    """Width 64, depth 5, skip after layer 2: the fp32 domain's query against the fp32 ray trick."""
    sd = nwe_amd.synthetic.make_state_dict(12, 5, 64, skips=(2,))
    pts, dirs = _cloud(12, 100)
    r = _renderer({0: sd})
    try:
        assert not r.mfma_supported(0)
        for steps in (0, 1, 3):
            r.debug_set_query_steps(steps)
            for n in (1, 15, 16, 17, 100):
                assert np.array_equal(_query(r, pts[:n], dirs[:n], "f32")["raw"], _trick(r, pts[:n], dirs[:n], "f32")), (steps, n)
    finally:
        r.close()


# ---- 9. the handler ---------------------------------------------------------------------------------------------------------

def test_handler_run_network_and_density_grid(capsys):
    """run_network([N,S,3], [N,3]) is query_points with points_per_dir = S; "auto" keeps a 4x128 coarse and an 8x256 fine
    network on the MFMA kernels for queries (frames of the pair fall back to fp32); density_grid is the sigma-only query of the
    cell centres, whatever the chunk."""
    sd_c, sd_f = _sd(1005, 4, 128), _sd(1006, 8, 256)
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")
    h.initialize_models(state_dicts=(sd_c, sd_f))
    assert h._precision == "f32"
    r = h.renderer
    try:
        pts, dirs = _cloud(13, 21 * 9)
        inputs, viewdirs = torch.from_numpy(pts.reshape(21, 9, 3)).cuda(), torch.from_numpy(dirs[:21]).cuda()
        for which, idx in (("fine", 1), ("coarse", 0)):
            raw = h.run_network(inputs, viewdirs, which=which)
            assert raw.shape == (21, 9, 4)
            want = r.query_points(inputs, viewdirs, which=idx, precision="f16x3")["raw"]
            assert torch.equal(raw, want)
            expanded = viewdirs[:, None].expand(inputs.shape).contiguous()         # model_utils.py:24
            assert torch.equal(raw, r.query_points(inputs, expanded, which=idx, precision="f16x3")["raw"])
            assert not torch.equal(raw, h.run_network(inputs, viewdirs, which=which, precision="f32"))
        assert torch.equal(h.run_network(inputs, viewdirs), h.run_network(inputs, viewdirs, which="fine"))
        with pytest.raises(ValueError):
            h.run_network(inputs, viewdirs[:5])
        with pytest.raises(ValueError):
            h.run_network(inputs, viewdirs, which="both")
        # density_grid: a resolution no chunk divides
        lo, hi, res = (-1.0, -2.0, 0.5), (1.0, 2.5, 0.75), (3, 5, 7)
        axes = [(np.arange(n).astype(np.float32) + np.float32(0.5)) * np.float32((b - a) / n) + np.float32(a) for a, b, n in zip(lo, hi, res)]
        centres = np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(np.float32)
        want = r.query_points(torch.from_numpy(centres).cuda(), None, which=1, precision="f16x3", outputs=("sigma",))["sigma"]
        for chunk in (1 << 20, 16, 104, 105):
            grid = h.density_grid(lo, hi, res, chunk=chunk)
            assert grid.shape == res and torch.equal(grid, want), chunk
        assert torch.equal(h.density_grid(lo, hi, res, which="coarse", chunk=50),
                           r.query_points(torch.from_numpy(centres).cuda(), None, which=0, outputs=("sigma",))["sigma"])
        cube = h.density_grid((-1, -1, -1), (1, 1, 1), 4, chunk=10)
        assert cube.shape == (4, 4, 4)
    finally:
        r.close()


def test_handler_run_network_without_view_dirs(tmp_path, monkeypatch):
    import yaml
    cfg = {k: dict(v) for k, v in nwe_amd.config.INFERENCE_DEFAULTS.items()}
    cfg["rendering"].update(use_view_dirs=False, n_samples=8, n_importance=8)
    with open(tmp_path / "office_tokyo_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setenv("NWE_CONFIG_DIR", str(tmp_path))
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "synthetic")
    sd_c, sd_f = _sd(1009, 4, 128, False), _sd(1010, 4, 128, False)
    h.initialize_models(state_dicts=(sd_c, sd_f))
    r = h.renderer
    try:
        pts, dirs = _cloud(14, 6 * 50)
        inputs = torch.from_numpy(pts.reshape(6, 50, 3)).cuda()
        raw = h.run_network(inputs, None)
        assert raw.shape == (6, 50, 4) and torch.equal(raw, r.query_points(inputs, None, which=1, precision="f16x3")["raw"])
        alone = _renderer({0: sd_f})
        assert np.array_equal(raw.reshape(-1, 4).cpu().numpy(), _trick(alone, pts, dirs, "f16x3"))
        alone.close()
        with pytest.raises(ValueError, match="no view directions"):
            h.run_network(inputs, torch.from_numpy(dirs[:6]).cuda())
        assert h.density_grid((-1, -1, -1), (1, 1, 1), (2, 3, 4)).shape == (2, 3, 4)
    finally:
        r.close()
