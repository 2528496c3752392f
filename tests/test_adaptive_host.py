"""The adaptive frame without a GPU (include/nwe.h: nwe_render_adaptive): the numpy restatement of tests/adaptive.py against
nwe_debug_adaptive_lattice and against itself in the regimes the rule names; every refusal on a host-only context by code, text and
order; NWE_ADAPTIVE and the handler's arguments."""
import ctypes as C

import numpy as np
import pytest

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler as Handler
from tests import adaptive as A

NAN, INF = float("nan"), float("inf")


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _lattice(first, last_excl, k, cap=None):
    cap = max(last_excl - first, 1) if cap is None else cap
    out = (C.c_int32 * max(cap, 1))()
    n = _lib.load().nwe_debug_adaptive_lattice(first, last_excl, k, out, cap)
    return n, list(out[:max(n, 0)])


def test_the_lattice_call_is_the_restatement():
    for first in (0, 5, 29):
        for length in list(range(1, 70)) + [128, 129, 130, 800]:
            for k in list(range(1, 65)):
                n, got = _lattice(first, first + length, k)
                want = A.lattice(first, first + length, k)
                assert n == len(want) and got == want.tolist(), (first, length, k)
                assert got[0] == first and got[-1] == first + length - 1 and all(b > a for a, b in zip(got, got[1:]))
    assert _lattice(3, 4, 7) == (1, [3]) and _lattice(0, 37, 64) == (2, [0, 36]) and _lattice(0, 45, 1)[0] == 45
    assert nwe_amd.Renderer.adaptive_lattice(5, 30, 5).tolist() == [5, 10, 15, 20, 25, 29]


def test_the_lattice_call_refuses():
    for first, last, k, cap in ((3, 3, 2, 4), (4, 3, 2, 4), (0, 10, 0, 16), (0, 10, 65, 16), (0, 10, -1, 16), (0, 10, 3, 3), (0, 2**31 - 1, 2, 4)):
        assert _lattice(first, last, k, cap)[0] == -1, (first, last, k, cap)
    assert _lib.load().nwe_debug_adaptive_lattice(0, 10, 2, None, 16) == -1
    assert _lattice(0, 10, 3, 4) == (4, [0, 3, 6, 9]) and _lattice(0, 11, 3, 5) == (5, [0, 3, 6, 9, 10])
    with pytest.raises(ValueError, match="adaptive lattice"):
        nwe_amd.Renderer.adaptive_lattice(0, 10, 65)


def _frame(h, W, seed=0, smooth=False):
    rng = np.random.default_rng(seed)
    if smooth:
        y, x = np.mgrid[0:h, 0:W].astype(np.float32)
        base = np.stack([0.01 * x, 0.02 * y, 0.005 * (x + y), 1.0 + 0.03 * x, 1.0 - 0.001 * y], -1)
        return (base + rng.uniform(-1e-3, 1e-3, base.shape)).astype(np.float32)
    return rng.uniform(0, 1, (h, W, 5)).astype(np.float32)


SHAPES = ((37, 45), (1, 45), (37, 1), (2, 2), (1, 1), (5, 9), (9, 4))


@pytest.mark.parametrize("h,W", SHAPES)
def test_the_regimes_of_the_restatement(h, W):
    frame = _frame(h, W, seed=h * 100 + W)
    for k in (1, 2, 3, 4, 5, 16, 64):
        for first in (0, 5):
            n_lattice = len(A.lattice(first, first + h, k)) * len(A.lattice(0, W, k))
            # a tolerance below 0: nothing is interpolated, and the frame is the full frame
            out, kind, counts = A.apply(frame, first, k, -1.0, -1.0)
            assert not (kind == A.KIND_INTERPOLATED).any() and np.array_equal(out, frame)
            assert counts == {"pixels": h * W, "lattice": n_lattice, "rendered": h * W - n_lattice, "interpolated": 0}
            # +inf on a finite frame: nothing is rendered beyond the lattice
            out, kind, counts = A.apply(frame, first, k, INF, INF)
            assert not (kind == A.KIND_RENDERED).any()
            assert counts == {"pixels": h * W, "lattice": n_lattice, "rendered": 0, "interpolated": h * W - n_lattice}
            assert np.array_equal(out[kind == 0], frame[kind == 0]) and np.isfinite(out).all()
            if k == 1:
                assert (kind == A.KIND_LATTICE).all()
            # in between: every pixel has exactly one kind, the counts add up, and only interpolated pixels moved
            out, kind, counts = A.apply(_frame(h, W, seed=k, smooth=True), first, k, 0.05, 0.05)
            assert set(np.unique(kind)) <= {0, 1, 2} and counts["lattice"] == n_lattice
            assert counts["lattice"] + counts["rendered"] + counts["interpolated"] == counts["pixels"] == h * W


def test_the_rule_by_hand():
    """A 5 x 5 frame at k = 4 is one cell: flat, the centre is the mean of the corners; one corner off by more than the tolerance
    makes it busy.  A NaN corner makes the cell busy whatever the tolerance; a pixel on the lattice row between a flat and a busy
    cell is rendered."""
    frame = np.zeros((5, 5, 5), np.float32)
    frame[0, 0], frame[0, 4], frame[4, 0], frame[4, 4] = 0.0, 0.02, 0.04, 0.06
    frame[2, 2] = 9.0                        # a feature narrower than k inside a flat cell is not seen: the stated limitation
    out, kind, counts = A.apply(frame, 0, 4, 0.07, 0.07)
    assert counts == {"pixels": 25, "lattice": 4, "rendered": 0, "interpolated": 21}
    assert np.allclose(out[2, 2], 0.03, atol=1e-7) and np.allclose(out[0, 1], 0.005, atol=1e-7)
    out, kind, counts = A.apply(frame, 0, 4, 0.05, 0.07)
    assert counts["rendered"] == 21 and out[2, 2, 0] == 9.0
    frame[0, 0, 3] = NAN
    assert A.apply(frame, 0, 4, INF, INF)[2]["rendered"] == 21
    # two cells side by side (W = 9, k = 4 -> columns 0, 4, 8), a single lattice row pair (h = 2 -> rows 0, 1)
    frame = np.zeros((2, 9, 5), np.float32)
    frame[:, 8] = 1.0                        # the right cell is busy, the left one flat
    out, kind, _ = A.apply(frame, 0, 4, 0.5, 0.5)
    assert kind[0].tolist() == [0, 2, 2, 2, 0, 1, 1, 1, 0] and kind[1].tolist() == kind[0].tolist()
    frame = np.zeros((9, 2, 5), np.float32)  # the same, turned: rows 0, 4, 8; the pixels of row 4 are lattice pixels
    frame[8] = 1.0
    assert A.apply(frame, 0, 4, 0.5, 0.5)[1][:, 0].tolist() == [0, 2, 2, 2, 0, 1, 1, 1, 0]
    # a pixel on the lattice row between a flat cell (above) and a busy one (below) is rendered: W = 3, k = 2 -> one cell column
    frame = np.zeros((5, 3, 5), np.float32)
    frame[4] = 1.0
    assert A.apply(frame, 0, 2, 0.5, 0.5)[1][:, 1].tolist() == [2, 2, 1, 1, 1]


def _render_adaptive(r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4),
                     precision=_lib.PREC_F16X3, k=2, tol_rgb=0.01, tol_depth=0.05):
    ptr = None if poses is None else poses.ctypes.data
    return _lib.load().nwe_render_adaptive(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0], rows[1],
                                           precision, k, tol_rgb, tol_depth, None if out is None else C.byref(out), None)


def _report(r):
    counts, ms = (C.c_int64 * 4)(-7, -7, -7, -7), C.c_float(-7.0)
    return _lib.load().nwe_last_adaptive(r._ctx, counts, C.byref(ms)), tuple(counts), ms.value


def test_every_refusal_in_front_of_the_host_only_one():
    """Code, text and order: each call below is wrong in everything behind the refusal it expects as well."""
    r = nwe_amd.Renderer(host_only=True)
    I, S, U = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE, _lib.NWE_ERR_UNSUPPORTED
    bad = dict(k=0, tol_rgb=NAN, precision=9)             # 5. and 6. wrong
    try:
        buf = np.full(60, 123.0, np.float32)
        good = _lib.AdaptiveOutputs(rgb=buf.ctypes.data)
        stale = _lib.AdaptiveOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.AdaptiveOutputs) - 8
        # 1. the context - whatever else is wrong
        assert _render_adaptive(None, None, poses=None, **bad) == I
        # 2. the outputs, in front of the camera (H = 0)
        assert _render_adaptive(r, None, H=0, **bad) == I and _error(r) == "null outputs"
        assert _render_adaptive(r, stale, H=0, **bad) == I and _error(r).startswith("nwe_adaptive_outputs.struct_bytes != sizeof(nwe_adaptive_outputs)")
        assert _render_adaptive(r, _lib.AdaptiveOutputs(kind=1, flags=1), H=0, **bad) == I and _error(r) == "none of rgb / depth / acc requested"
        for name in ("rgb", "depth", "acc"):      # any one of them is a request
            assert _render_adaptive(r, _lib.AdaptiveOutputs(**{name: 1}), H=0, **bad) == I and _error(r) == "bad pose / image / row range", name
        # 3. the camera and the ray count, with nwe_render's texts
        for kw in (dict(poses=None), dict(n_poses=0), dict(H=0), dict(W=0), dict(rows=(-1, 4)), dict(rows=(0, 5)), dict(rows=(3, 2))):
            assert _render_adaptive(r, good, **kw, **bad) == I and _error(r) == "bad pose / image / row range", kw
        for kw in (dict(fx=0.), dict(fy=-0.)):
            assert _render_adaptive(r, good, **kw, **bad) == I and _error(r) == "fx and fy must be non-zero", kw
        assert _render_adaptive(r, good, near=2., far=1., **bad) == I
        assert _error(r) == "far < near: the sorted merge of the fine pass needs ascending depths"
        assert _render_adaptive(r, good, n_poses=3, H=30000, W=30000, rows=(0, 30000), **bad) == I
        assert _error(r) == "more than 2^31 - 1 rays in one call"
        # 4. the call's own bound: 2^24 rays are let through to the next refusal, one more is not
        assert _render_adaptive(r, good, H=4096, W=4096, rows=(0, 4096), **bad) == I and _error(r) == "adaptive frame: k must be in 1..64"
        assert _render_adaptive(r, good, H=4097, W=4096, rows=(0, 4097), **bad) == I
        assert _error(r) == "adaptive frame: more than 2^24 rays in one call"
        # 5. k and the tolerances, 6. the precision
        for k in (0, 65, -2):
            assert _render_adaptive(r, good, **dict(bad, k=k)) == I and _error(r) == "adaptive frame: k must be in 1..64"
        for kw in (dict(tol_rgb=NAN), dict(tol_rgb=0.1, tol_depth=NAN)):
            assert _render_adaptive(r, good, **dict(bad, k=64, **kw)) == I and _error(r) == "adaptive frame: the tolerances must not be NaN"
        assert _render_adaptive(r, good, k=1, tol_rgb=-INF, tol_depth=INF, precision=9) == I and _error(r) == "unknown precision"
        # 7. what nwe_render_rays refuses of the context for lean outputs, in its words; zero rays do not come first
        for rows in ((0, 4), (2, 2)):
            assert _render_adaptive(r, good, rows=rows) == S and _error(r) == "nwe_set_sampling has not been called"
        r.set_sampling(8, 8)
        assert _render_adaptive(r, good) == S and _error(r) == "coarse network not set"
        r.set_network(0, synthetic.make_state_dict(5, 3, 64, skips=()))          # a shape without an MFMA kernel
        assert _render_adaptive(r, good) == S and _error(r) == "fine network not set but n_importance > 0"
        r.set_network(1, synthetic.make_state_dict(6, 3, 64, skips=()))
        assert _render_adaptive(r, good) == U and _error(r).startswith("no MFMA kernel for this network shape")
        sd = synthetic.make_state_dict(7, 4, 128, skips=())
        r.set_network(0, sd); r.set_network(1, sd)
        lib = _lib.load()
        rays_out, report = _lib.Outputs(rgb=1), _lib.PlanReport()

        def rays_refusal():      # of a ray list of four with lean outputs, asked of the planner: a host-only context serves that
            rc = lib.nwe_debug_plan(r._ctx, 1, 1, 4, 0, 1, 4, C.byref(rays_out), 0, _lib.PREC_F16X3, 256, C.byref(report))
            return rc, _error(r)

        # the modes: nwe_render_rays' own code and text, on this very context
        r.set_early_termination(0.01)
        want = rays_refusal()
        assert want[0] == U and "early termination" in want[1] and (_render_adaptive(r, good), _error(r)) == want
        r.set_early_termination(0.0); r.set_shared_coarse(2)
        want = rays_refusal()
        assert want[0] == U and "shared coarse pass" in want[1] and (_render_adaptive(r, good), _error(r)) == want
        r.set_shared_coarse(1)
        r.set_occupancy(np.ones((2, 2, 2), bool), (-1, -1, -1), (1, 1, 1), 2)
        want = rays_refusal()
        assert want[0] == U and "occupancy grid" in want[1] and (_render_adaptive(r, good), _error(r)) == want
        r.clear_occupancy()
        r.set_coarse_grid(np.zeros((2, 2, 2), np.float32), (-1, -1, -1), (1, 1, 1))
        want = rays_refusal()
        assert want[0] == U and "coarse density grid" in want[1] and (_render_adaptive(r, good), _error(r)) == want
        r.clear_coarse_grid()
        r.set_separate_passes(True)          # separate passes are honoured: the call comes through to the last refusal
        # 8. last, the device
        for precision in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32):
            for rows in ((0, 4), (2, 2)):
                assert _render_adaptive(r, good, precision=precision, rows=rows, k=64, tol_rgb=-1.0, tol_depth=INF) == S
                assert _error(r) == "host-only context cannot render"
        with pytest.raises(RuntimeError, match="nwe_render_adaptive: host-only context cannot render"):
            r.render_adaptive(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5.)
        with pytest.raises(ValueError, match="unknown adaptive outputs"):
            r.render_adaptive(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., outputs=("rgb", "disp"))
        # a refused call leaves the outputs untouched, and there is no report of a call that never ran
        assert (buf == 123.0).all()
        assert _report(r) == (S, (-7, -7, -7, -7), -7.0) and r.last_adaptive() is None
        assert lib.nwe_last_adaptive(None, None, None) == I
    finally:
        r.close()


def test_the_handlers_option(monkeypatch):
    parse = Handler.parse_adaptive
    assert parse(None, "") is None and parse(None, " ") is None
    assert parse({}, "") == {"k": 2, "tol_rgb": 2 / 255, "tol_depth": 0.05}
    assert parse({"k": 4, "tol_depth": 1}, "") == {"k": 4, "tol_rgb": 2 / 255, "tol_depth": 1.0}
    assert parse(None, "3,0.01") == {"k": 3, "tol_rgb": 0.01, "tol_depth": 0.05}
    assert parse({"k": 4, "tol_rgb": 0.5}, " 5 , 0.02 , 0.1 ") == {"k": 5, "tol_rgb": 0.02, "tol_depth": 0.1}
    assert parse(None, "2,-1,inf") == {"k": 2, "tol_rgb": -1.0, "tol_depth": INF}
    for env in ("3", "3,0.1,0.2,0.3", "x,0.1", "2.5,0.1", "3,abc"):
        with pytest.raises(ValueError, match="NWE_ADAPTIVE must be k,tol_rgb"):
            parse(None, env)
    for opt, text in (({"k": 0}, "k must be an integer in 1..64"), ({"k": 65}, "k must be"), ({"k": True}, "k must be"), ({"k": 2.0}, "k must be"),
                      ({"tol_rgb": NAN}, "tol_rgb must be a number"), ({"tol_depth": "1"}, "tol_depth must be a number"),
                      ({"tolerance": 1}, "adaptive may hold k, tol_rgb, tol_depth")):
        with pytest.raises(ValueError, match=text):
            parse(opt, "")
    with pytest.raises(ValueError, match="k must be"):
        parse(None, "65,0.1")
    # the constructor: off by default, on by argument or by environment, refused by name together with what it cannot serve
    box = {"lo": (-1, -1, -1), "hi": (1, 1, 1)}
    monkeypatch.delenv("NWE_ADAPTIVE", raising=False)
    assert Handler("office_geneve", "none.ckpt")._adaptive is None
    assert Handler("office_geneve", "none.ckpt", adaptive={"k": 3})._adaptive == {"k": 3, "tol_rgb": 2 / 255, "tol_depth": 0.05}
    assert Handler("office_geneve", "none.ckpt", adaptive={}, separate_passes=True)._adaptive["k"] == 2
    for kw, other in ((dict(sparse_fine={}, radiance_grid=box), "sparse_fine"), (dict(early_termination=0.01), "early_termination > 0"),
                      (dict(shared_coarse=2), "shared_coarse > 1"), (dict(occupancy=box), "occupancy"), (dict(baked_coarse=box), "baked_coarse"),
                      (dict(devices=[0, 0]), "devices")):
        with pytest.raises(ValueError) as exc:
            Handler("office_geneve", "none.ckpt", adaptive={"k": 2}, **kw)
        assert "adaptive" in str(exc.value) and other in str(exc.value), kw
    monkeypatch.setenv("NWE_ADAPTIVE", "4,0.02")
    assert Handler("office_geneve", "none.ckpt")._adaptive == {"k": 4, "tol_rgb": 0.02, "tol_depth": 0.05}
    with pytest.raises(ValueError, match="adaptive .* devices"):
        Handler("office_geneve", "none.ckpt", devices=[0, 1])
    monkeypatch.setenv("NWE_ADAPTIVE", "4")
    with pytest.raises(ValueError, match="NWE_ADAPTIVE must be"):
        Handler("office_geneve", "none.ckpt")
