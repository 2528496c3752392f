"""The multi-level adaptive frame without a GPU (include/nwe.h: nwe_render_adaptive_levels): the numpy restatement of
tests/adaptive_levels.py against tests/adaptive.py and against itself in the regimes the rule names; the lattice and the plan calls
against it; every refusal on a host-only context by code, text and order; NWE_ADAPTIVE_LEVELS and the handler's arguments."""
import ctypes as C

import numpy as np
import pytest

import nwe_amd
from nwe_amd import _lib, synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler as Handler
from tests import adaptive as A
from tests import adaptive_levels as L

NAN, INF = float("nan"), float("inf")
LEGAL = [(k, n) for n in range(1, 5) for k in range(1, 65) if L.levels_ok(k, n)]


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _frame(h, W, seed=0):
    """Smooth ramps, a step edge and a little noise: at tolerances around 0.05 cells of every kind at every level."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:W].astype(np.float32)
    base = np.stack([0.004 * x, 0.006 * y, 0.002 * (x + y), 1.0 + 0.01 * x, 1.0 - 0.001 * y], -1)
    base[(x + 2 * y) > 0.9 * (W + h)] += 0.5
    return (base + rng.uniform(-1e-3, 1e-3, base.shape)).astype(np.float32)


SHAPES = ((37, 45), (33, 41), (1, 1), (1, 7), (9, 1), (2, 3))


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,W", SHAPES)
def test_one_level_is_the_adaptive_frame_bit_for_bit(h, W):
    frame = _frame(h, W, seed=h + W)
    for k in (1, 2, 3, 5, 64):
        for first in (0, 5):
            for tol in (-1.0, 0.02, INF):
                want, want_kind, want_counts = A.apply(frame, first, k, tol, tol)
                out, kind, level, counts = L.apply(frame, first, k, 1, tol, tol)
                assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(kind, want_kind), (k, first, tol)
                assert counts["lattice"] == want_counts["lattice"] and counts["rendered"] == [want_counts["rendered"]]
                assert counts["interpolated"] == [want_counts["interpolated"]]
                assert np.array_equal(level, (kind == A.KIND_RENDERED).astype(np.uint8))


@pytest.mark.parametrize("h,W", SHAPES)
def test_the_regimes_of_the_restatement(h, W):
    """apply() itself asserts that the rule is well defined - rendered corners, parents that hold their children, a flat own cell
    for every pixel left - on ragged and aligned lattices and on row tiles (first = 5)."""
    frame = _frame(h, W, seed=3)
    for k, levels in ((2, 2), (2, 3), (1, 3), (3, 2), (1, 4), (8, 4), (5, 3)):
        for first in (0, 5):
            n0 = len(A.lattice(first, first + h, L.spacing(k, levels, 0))) * len(A.lattice(0, W, L.spacing(k, levels, 0)))
            out, kind, level, counts = L.apply(frame, first, k, levels, -1.0, -1.0)     # every cell busy: every pixel rendered
            assert np.array_equal(out, frame) and not (kind == A.KIND_INTERPOLATED).any() and counts["interpolated"] == [0] * levels
            assert counts["lattice"] == n0 and counts["rendered"] == L.plan(1, h, W, k, levels)["pass_max"][1:]
            assert np.array_equal(level > 0, kind == A.KIND_RENDERED) and int(level.max()) <= levels
            out, kind, level, counts = L.apply(frame, first, k, levels, INF, INF)       # every cell flat: one launch, all at level 0
            assert counts["render_launches"] == 1 and counts["rendered"] == [0] * levels
            assert counts["interpolated"] == [h * W - n0] + [0] * (levels - 1) and not level.any()
            for tol in (0.01, 0.05):
                out, kind, level, counts = L.apply(frame, first, k, levels, tol, tol)
                moved = out.view(np.uint32) != frame.view(np.uint32)
                assert not moved[kind != A.KIND_INTERPOLATED].any()
                assert [int((level[kind == A.KIND_INTERPOLATED] == l).sum()) for l in range(levels)] == counts["interpolated"]
                assert [int((level[kind == A.KIND_RENDERED] == l + 1).sum()) for l in range(levels)] == counts["rendered"]


def test_the_rule_by_hand():
    """9 x 9 at k = 4, levels = 2: level 0 is one cell of spacing 8, level 1 four cells of spacing 4."""
    frame = np.zeros((9, 9, 5), np.float32)
    frame[4, 4] = 9.0                        # on the level 1 lattice, inside the flat level 0 cell: not seen, the stated limitation
    out, kind, level, counts = L.apply(frame, 0, 4, 2, 0.5, 0.5)
    assert counts == {"pixels": 81, "lattice": 4, "levels": 2, "render_launches": 1, "rendered": [0, 0], "interpolated": [77, 0]}
    assert out[4, 4, 0] == 0.0
    frame[8, 8] = 1.0                        # one corner off: the level 0 cell is busy, pass 1 renders the other five level 1 lattice pixels
    out, kind, level, counts = L.apply(frame, 0, 4, 2, 0.5, 0.5)
    assert counts["rendered"][0] == 5 and counts["render_launches"] == 3 and out[4, 4, 0] == 9.0
    # now every level 1 cell has the corner (4, 4) at 9: all four are busy, and pass 2 renders the rest
    assert counts["rendered"][1] == 81 - 9 and counts["interpolated"] == [0, 0]
    frame[4, 4] = 0.0                        # only the lower right level 1 cell is busy now: its closed rectangle is rendered
    out, kind, level, counts = L.apply(frame, 0, 4, 2, 0.5, 0.5)
    assert counts["rendered"] == [5, 25 - 4] and counts["interpolated"] == [0, 81 - 9 - 21]
    assert (kind[4:, 4:] != A.KIND_INTERPOLATED).all() and (kind[:4, :] != A.KIND_RENDERED)[:, [1, 2, 3, 5, 6, 7]].all()
    assert level[5, 5] == 2 and level[4, 8] == 1 and level[0, 0] == 0 and level[1, 1] == 1 and kind[1, 1] == A.KIND_INTERPOLATED


# ---- the debug calls ------------------------------------------------------------------------------------------------------------

def _lattice(first, last_excl, k, levels, level, cap=None):
    cap = max(last_excl - first, 1) if cap is None else cap
    out = (C.c_int32 * max(cap, 1))()
    n = _lib.load().nwe_debug_adaptive_levels_lattice(first, last_excl, k, levels, level, out, cap)
    return n, list(out[:max(n, 0)])


def _one_level_lattice(first, last_excl, k):
    out = (C.c_int32 * max(last_excl - first, 1))()
    n = _lib.load().nwe_debug_adaptive_lattice(first, last_excl, k, out, max(last_excl - first, 1))
    return n, list(out[:max(n, 0)])


def test_the_lattice_call_nests_and_ends_in_the_one_level_lattice():
    for first in (0, 5):
        for length in list(range(1, 40)) + [45, 64, 65, 129, 800]:
            for k, levels in LEGAL:
                if k > 9 and k not in (16, 21, 32, 64):
                    continue
                got = [_lattice(first, first + length, k, levels, l) for l in range(levels)]
                want = L.lattices(first, first + length, k, levels)
                for l in range(levels):
                    assert got[l] == (len(want[l]), (want[l] + first).tolist()), (first, length, k, levels, l)
                    if l:
                        assert set(got[l - 1][1]) <= set(got[l][1])
                assert got[-1] == _one_level_lattice(first, first + length, k)
    assert nwe_amd.Renderer.adaptive_levels_lattice(5, 30, 2, 3, 0).tolist() == [5, 13, 21, 29]


def test_the_lattice_call_refuses():
    for args in ((3, 3, 2, 2, 0), (0, 10, 0, 1, 0), (0, 10, 65, 1, 0), (0, 10, 2, 0, 0), (0, 10, 2, 5, 0), (0, 10, 33, 2, 0), (0, 10, 9, 4, 0),
                 (0, 10, 2, 2, 2), (0, 10, 2, 2, -1)):
        assert _lattice(*args, cap=16)[0] == -1, args
    assert _lattice(0, 10, 2, 2, 1, cap=4)[0] == -1 and _lattice(0, 10, 2, 2, 0, cap=4) == (4, [0, 4, 8, 9])
    assert _lib.load().nwe_debug_adaptive_levels_lattice(0, 10, 2, 2, 0, None, 16) == -1
    assert _lattice(0, 100, 32, 2, 0) == (3, [0, 64, 99]) and _lattice(0, 100, 8, 4, 0) == (3, [0, 64, 99])
    with pytest.raises(ValueError, match="adaptive lattice"):
        nwe_amd.Renderer.adaptive_levels_lattice(0, 10, 33, 2, 0)


def _plan(n_poses, rows, width, k, levels, cols=11, cap=16):
    out = (C.c_int64 * 16)()
    n = _lib.load().nwe_debug_adaptive_levels_plan(n_poses, rows, width, k, levels, cols, out, cap)
    return n, list(out[:max(n, 0)])


def test_the_plan_is_the_restatements():
    for n_poses, rows, width in ((1, 37, 45), (2, 33, 41), (1, 1, 1), (1, 1, 7), (3, 9, 1), (1, 2, 3), (1, 800, 800)):
        for k, levels in ((2, 1), (2, 2), (2, 3), (1, 3), (3, 2), (1, 4), (8, 4), (64, 1), (5, 3)):
            want = L.plan(n_poses, rows, width, k, levels)
            n, got = _plan(n_poses, rows, width, k, levels)
            assert n == 5 + 2 * levels, (n_poses, rows, width, k, levels)
            assert got[:3] == [want["pixels"], want["lattice"], want["list"]] and got[4:4 + levels] == want["cells"]
            assert got[4 + levels:] == want["pass_max"] and sum(want["pass_max"]) == want["pixels"]
            # the scratch holds its regions: list and rays of the largest pass, 28 bytes per pixel of outputs, slots and counts, the cells
            floor = want["list"] * 4 * (1 + 11) + want["pixels"] * 28 + sum(want["cells"]) + 4 * (2 * 4 + 4 + 1)
            assert floor <= got[3] <= floor + 256 * (11 + levels) and got[3] % 256 == 0
            assert _plan(n_poses, rows, width, k, levels, cols=8)[1][3] < got[3] or want["list"] * 12 < 256
    for args in ((0, 4, 4, 2, 2), (1, 0, 4, 2, 2), (1, 4, 0, 2, 2), (1, 4097, 4096, 2, 2), (1, 4, 4, 0, 2), (1, 4, 4, 2, 0), (1, 4, 4, 2, 5),
                 (1, 4, 4, 33, 2)):
        assert _plan(*args)[0] == -1, args
    assert _plan(1, 4, 4, 2, 2, cols=9)[0] == -1 and _plan(1, 4, 4, 2, 2, cap=8)[0] == -1 and _plan(1, 4, 4, 2, 2, cap=9)[0] == 9
    assert _lib.load().nwe_debug_adaptive_levels_plan(1, 4, 4, 2, 2, 11, None, 16) == -1


# ---- the refusals ---------------------------------------------------------------------------------------------------------------

def _call(r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4),
          precision=_lib.PREC_F16X3, k=2, levels=2, tol_rgb=0.01, tol_depth=0.05):
    ptr = None if poses is None else poses.ctypes.data
    return _lib.load().nwe_render_adaptive_levels(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0],
                                                  rows[1], precision, k, levels, tol_rgb, tol_depth, None if out is None else C.byref(out), None)


def _report(r, cap=12):
    counts, ms = (C.c_int64 * 12)(*([-7] * 12)), C.c_float(-7.0)
    return _lib.load().nwe_last_adaptive_levels(r._ctx, counts, cap, C.byref(ms)), tuple(counts), ms.value


def test_every_refusal_in_front_of_the_host_only_one():
    """Code, text and order: each call below is wrong in everything behind the refusal it expects as well."""
    r = nwe_amd.Renderer(host_only=True)
    I, S, U = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE, _lib.NWE_ERR_UNSUPPORTED
    bad = dict(k=0, levels=0, tol_rgb=NAN, precision=9)
    levels_text = "adaptive frame: levels must be in 1..4 and k * 2^(levels - 1) at most 64"
    try:
        buf = np.full(60, 123.0, np.float32)
        good = _lib.AdaptiveLevelsOutputs(rgb=buf.ctypes.data)
        stale = _lib.AdaptiveLevelsOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.AdaptiveOutputs)           # the one-level call's struct is another
        assert C.sizeof(_lib.AdaptiveLevelsOutputs) == C.sizeof(_lib.AdaptiveOutputs) + 8
        # 1. the context, 2. the outputs, in front of the camera (H = 0)
        assert _call(None, None, poses=None, **bad) == I
        assert _call(r, None, H=0, **bad) == I and _error(r) == "null outputs"
        assert _call(r, stale, H=0, **bad) == I
        assert _error(r).startswith("nwe_adaptive_levels_outputs.struct_bytes != sizeof(nwe_adaptive_levels_outputs)")
        assert _call(r, _lib.AdaptiveLevelsOutputs(kind=1, level=1, flags=1), H=0, **bad) == I and _error(r) == "none of rgb / depth / acc requested"
        for name in ("rgb", "depth", "acc"):
            assert _call(r, _lib.AdaptiveLevelsOutputs(**{name: 1}), H=0, **bad) == I and _error(r) == "bad pose / image / row range", name
        # 3. the camera and the ray count, 4. the call's own bound
        for kw in (dict(poses=None), dict(n_poses=0), dict(W=0), dict(rows=(0, 5)), dict(rows=(3, 2))):
            assert _call(r, good, **kw, **bad) == I and _error(r) == "bad pose / image / row range", kw
        assert _call(r, good, fx=0., **bad) == I and _error(r) == "fx and fy must be non-zero"
        assert _call(r, good, near=2., far=1., **bad) == I and _error(r).startswith("far < near")
        assert _call(r, good, n_poses=3, H=30000, W=30000, rows=(0, 30000), **bad) == I and _error(r) == "more than 2^31 - 1 rays in one call"
        assert _call(r, good, H=4097, W=4096, rows=(0, 4097), **bad) == I and _error(r) == "adaptive frame: more than 2^24 rays in one call"
        assert _call(r, good, H=4096, W=4096, rows=(0, 4096), **bad) == I and _error(r) == "adaptive frame: k must be in 1..64"
        # 5. k, then directly behind it the levels, then the tolerances; 6. the precision
        for k in (0, 65, -2):
            assert _call(r, good, **dict(bad, k=k)) == I and _error(r) == "adaptive frame: k must be in 1..64"
        for k, levels in ((2, 0), (2, 5), (2, -1), (33, 2), (17, 3), (9, 4), (64, 2)):
            assert _call(r, good, **dict(bad, k=k, levels=levels)) == I and _error(r) == levels_text, (k, levels)
        for k, levels in ((64, 1), (32, 2), (16, 3), (8, 4), (1, 4)):         # the largest legal ones come through to the tolerances
            assert _call(r, good, **dict(bad, k=k, levels=levels)) == I and _error(r) == "adaptive frame: the tolerances must not be NaN"
        assert _call(r, good, tol_rgb=0.1, tol_depth=NAN, precision=9) == I and _error(r) == "adaptive frame: the tolerances must not be NaN"
        assert _call(r, good, tol_rgb=-INF, tol_depth=INF, precision=9) == I and _error(r) == "unknown precision"
        # 7. what nwe_render_rays refuses of the context for lean outputs, in its words; zero rays do not come first
        for rows in ((0, 4), (2, 2)):
            assert _call(r, good, rows=rows) == S and _error(r) == "nwe_set_sampling has not been called"
        r.set_sampling(8, 8)
        assert _call(r, good) == S and _error(r) == "coarse network not set"
        sd = synthetic.make_state_dict(7, 4, 128, skips=())
        r.set_network(0, sd); r.set_network(1, sd)
        lib = _lib.load()
        rays_out, report = _lib.Outputs(rgb=1), _lib.PlanReport()

        def rays_refusal():      # of a ray list of four with lean outputs, asked of the planner: a host-only context serves that
            rc = lib.nwe_debug_plan(r._ctx, 1, 1, 4, 0, 1, 4, C.byref(rays_out), 0, _lib.PREC_F16X3, 256, C.byref(report))
            return rc, _error(r)

        modes = ((lambda: r.set_early_termination(0.01), lambda: r.set_early_termination(0.0), "early termination"),
                 (lambda: r.set_shared_coarse(2), lambda: r.set_shared_coarse(1), "shared coarse pass"),
                 (lambda: r.set_occupancy(np.ones((2, 2, 2), bool), (-1, -1, -1), (1, 1, 1), 2), r.clear_occupancy, "occupancy grid"),
                 (lambda: r.set_coarse_grid(np.zeros((2, 2, 2), np.float32), (-1, -1, -1), (1, 1, 1)), r.clear_coarse_grid, "coarse density grid"))
        for on, off, name in modes:
            on()
            want = rays_refusal()
            assert want[0] == U and name in want[1] and (_call(r, good), _error(r)) == want, name
            off()
        r.set_separate_passes(True)          # separate passes are honoured: the call comes through to the last refusal
        # 8. last, the device
        for precision in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32):
            for rows in ((0, 4), (2, 2)):
                assert _call(r, good, precision=precision, rows=rows, k=8, levels=4, tol_rgb=-1.0, tol_depth=INF) == S
                assert _error(r) == "host-only context cannot render"
        cam = dict(fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5.)
        with pytest.raises(RuntimeError, match="nwe_render_adaptive_levels: host-only context cannot render"):
            r.render_adaptive(np.eye(4), 4, 5, levels=2, **cam)
        with pytest.raises(ValueError, match="nwe_render_adaptive_levels: adaptive frame: levels must be"):
            r.render_adaptive(np.eye(4), 4, 5, levels=5, **cam)
        with pytest.raises(RuntimeError, match="nwe_render_adaptive: host-only context cannot render"):     # None stays the one-level call
            r.render_adaptive(np.eye(4), 4, 5, **cam)
        with pytest.raises(ValueError, match="unknown adaptive outputs"):                                     # ... which has no level map
            r.render_adaptive(np.eye(4), 4, 5, outputs=("rgb", "level"), **cam)
        with pytest.raises(ValueError, match="unknown adaptive outputs"):
            r.render_adaptive(np.eye(4), 4, 5, outputs=("rgb", "disp"), levels=2, **cam)
        # a refused call leaves the outputs untouched, and there is no report of a call that never ran
        assert (buf == 123.0).all()
        assert _report(r) == (S, (-7,) * 12, -7.0) and r.last_adaptive_levels() is None and r.last_adaptive() is None
        assert lib.nwe_last_adaptive_levels(None, None, 12, None) == I
    finally:
        r.close()


# ---- the handler ----------------------------------------------------------------------------------------------------------------

def test_the_handlers_option(monkeypatch):
    parse = Handler.parse_adaptive_levels
    assert parse(None, "", 2) is None and parse(None, " ", None) is None
    assert parse(3, "", 2) == 3 and parse(None, " 2 ", 2) == 2 and parse(1, "4", 64) == 1 and parse(4, "", 8) == 4
    for env in ("x", "2.5", "1,2"):
        with pytest.raises(ValueError, match="NWE_ADAPTIVE_LEVELS must be an integer in 1..4"):
            parse(None, env, 2)
    for levels in (0, 5, True, 2.0, "2"):
        with pytest.raises(ValueError, match="adaptive_levels must be an integer in 1..4"):
            parse(levels, "", 2)
    with pytest.raises(ValueError, match="adaptive_levels must be an integer in 1..4"):
        parse(None, "7", 2)
    with pytest.raises(ValueError, match="is an option of the adaptive frame"):
        parse(2, "", None)
    for k, levels in ((33, 2), (9, 4), (64, 2)):
        with pytest.raises(ValueError, match="must be at most 64"):
            parse(levels, "", k)
    for name in ("NWE_ADAPTIVE", "NWE_ADAPTIVE_LEVELS", "NWE_ADAPTIVE_LISTS"):
        monkeypatch.delenv(name, raising=False)
    assert Handler("office_geneve", "none.ckpt")._adaptive_levels is None
    assert Handler("office_geneve", "none.ckpt", adaptive={"k": 3})._adaptive_levels is None          # off unless asked for
    h = Handler("office_geneve", "none.ckpt", adaptive={"k": 3}, adaptive_levels=3)
    assert h._adaptive_levels == 3 and h._adaptive == {"k": 3, "tol_rgb": 2 / 255, "tol_depth": 0.05}
    with pytest.raises(ValueError, match="adaptive_levels is an option of the adaptive frame"):
        Handler("office_geneve", "none.ckpt", adaptive_levels=2)
    with pytest.raises(ValueError, match="must be at most 64"):
        Handler("office_geneve", "none.ckpt", adaptive={"k": 33}, adaptive_levels=2)
    monkeypatch.setenv("NWE_ADAPTIVE_LEVELS", "2")
    assert Handler("office_geneve", "none.ckpt", adaptive={})._adaptive_levels == 2
    assert Handler("office_geneve", "none.ckpt", adaptive={}, adaptive_levels=4)._adaptive_levels == 4   # the argument wins
    with pytest.raises(ValueError, match="adaptive_levels is an option of the adaptive frame"):
        Handler("office_geneve", "none.ckpt")
    monkeypatch.setenv("NWE_ADAPTIVE", "4,0.02")                    # the string format of NWE_ADAPTIVE is what it was
    h = Handler("office_geneve", "none.ckpt")
    assert h._adaptive == {"k": 4, "tol_rgb": 0.02, "tol_depth": 0.05} and h._adaptive_levels == 2
