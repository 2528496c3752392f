"""tests/opt_in_sequences.py without a GPU: the walks are deterministic and cover their table; the whole state machine - every
setter, clear and getter, the three clearing rules, every refusal in front of "host-only context" - is walked on a host-only
long-lived context against fresh host-only contexts; and the generator's own bookkeeping (which calls render, which weight table
they take, which slot of the render ring) is held to nwe_debug_plan, so that the coverage counts mean what they say."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from tests import opt_in_sequences as S


def test_the_walks_are_deterministic_and_cover_the_table():
    union = {}
    for i in range(S.N_WALKS):
        steps, cover = S.make_walk(i)
        assert len(steps) >= S.WALKS[i][1] and steps == list(S._make_walk.__wrapped__(S.WALKS[i][0], S.WALKS[i][1], (i, S.N_WALKS))[0]), i
        assert not S.coverage_gaps(cover, (i, S.N_WALKS)), (i, S.coverage_gaps(cover, (i, S.N_WALKS)))     # its share ...
        assert steps[-1][0] in ("render", "render_rays") and S.expect(_state_before_last(steps), steps[-1]) is None, i
        for k, n in cover.items():
            union[k] = union.get(k, 0) + n
    assert union == S.union_coverage()
    assert not S.coverage_gaps(union), S.coverage_gaps(union)                                             # ... and all of it
    print(f"{S.N_WALKS} walks, {sum(len(S.make_walk(i)[0]) for i in range(S.N_WALKS))} steps; coverage:")
    for k, n in S.MUST_COVER:
        print(f"  {union[k]:4d} (>= {n})  {k}")
    # the frames are what the issue asks for: below a wave, ragged against 128, past one scan tile
    rays = [h * w for h, w in S.FRAMES]
    assert rays[0] < 32 and rays[1] % 128 and rays[2] > 2 * 1024


def _state_before_last(steps):
    st = S.State()
    for s in steps[:-1]:
        if not s[0].startswith("refused_"):
            st.apply(s)
    return st


# ---- the walk on host-only contexts ---------------------------------------------------------------------------------------------

_PLAN = None


def _plan(r, call, hook):
    """nwe_debug_plan for a render / render_rays call -> (code, text, the report's bytes)."""
    global _PLAN
    lib = _lib.load()
    if _PLAN is None:
        _PLAN = lib["nwe_debug_plan"]
        _PLAN.restype, _PLAN.argtypes = C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_int64, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    op, prec, outk, frame, n_poses = call
    H, W = S.FRAMES[frame]
    out = _lib.Outputs(flags=1, **{k: 1 for k in (S.LEAN if outk == "lean" else S.FULL)})
    report = _lib.PlanReport()
    hooks = 0 if hook is None else (_lib.PLAN_HOOK_COARSE_WEIGHTS if hook == "coarse_weights" else _lib.PLAN_HOOK_OTHER)
    if op == "render":
        rc = _PLAN(r._ctx, n_poses, H, W, 0, H, -1, C.addressof(out), 0, _lib.PRECISIONS[prec], 256, C.addressof(report))
    else:
        rc = _PLAN(r._ctx, 1, 1, 1, 0, 1, H * W * n_poses, C.addressof(out), hooks, _lib.PRECISIONS[prec], 256, C.addressof(report))
    return rc, (lib.nwe_last_error(r._ctx).decode() if rc else ""), (bytes(report) if rc == 0 else b""), report.table_elems


def _raised(call):
    try:
        call()
    except (RuntimeError, ValueError, NotImplementedError) as e:        # NotImplementedError is a RuntimeError; named for the reader
        return type(e), str(e)
    return None


def _host_call(r, st, call):
    """A render-like call that is no render / render_rays on a host-only context: the wrapper's exception, entry name removed."""
    op = call[0]
    cam = S.camera_of(*S.FRAMES[call[-2]]) if op != "query" else None
    if op == "render_grid":
        return _raised(lambda: r.render_grid(S.poses_of(call[-1]), *S.FRAMES[call[-2]], outputs=S.GRID_OUT[call[1]], **cam))
    if op == "render_sparse":
        got = []
        for asynchronous in (False, True):
            e = _raised(lambda: r.render_sparse(S.poses_of(call[-1]), *S.FRAMES[call[-2]], which=call[3], precision=call[2], min_weight=call[4],
                                                dilate=call[5], outputs=S.SPARSE_OUT[call[6]], asynchronous=asynchronous, **cam))
            assert e is not None
            got.append((e[0], e[1].split(": ", 1)[1]))
        assert got[0] == got[1], (call, got)                  # the two entry points agree
        return got[0]
    if op == "query":
        pts = torch.zeros(call[4], 3)
        dirs = None if st.noview(call[1]) or call[3] == "sigma" else torch.zeros(call[4], 3)
        return _raised(lambda: r.query_points(pts, dirs, which=call[1], precision=call[2], outputs=(call[3],)))
    if op == "cgrid_weights":
        return _raised(lambda: r.coarse_grid_weights(S.poses_of(call[-1]), *S.FRAMES[call[-2]], **cam))
    return None                                               # create_rays: nothing of it is reachable without a device


def _fake_build(step):
    """A host-only context cannot build: the grid a build step leaves is stood in for by one set from the host, of the step's size."""
    rng = np.random.Generator(np.random.Philox(key=[sum(step[1].encode()), 11]))
    res = tuple(step[2])
    if step[0] == "build_occ":
        values = rng.uniform(size=res) < 0.6
    else:
        values = rng.uniform(-1.0, 2.0, size=res + ((4,) if step[0] == "bake_rgrid" else ())).astype(np.float32)
    return {"values": values, "lo": S.BOX_LO, "hi": S.BOX_HI, "res": res}


@functools.lru_cache(maxsize=None)
def _walk_on_the_host(index):
    """Walks walk `index`; returns per step whether each of its render / render_rays calls was planned (not refused)."""
    steps, _ = S.make_walk(index)
    grids = S.Grids()
    r, st = nwe_amd.Renderer(host_only=True), S.State()
    S.configure(r, st, grids)
    fresh = {"key": None, "ctx": None}
    planned, compared = [], 0

    def fresh_context():
        if fresh["key"] != st.key():
            if fresh["ctx"] is not None:
                fresh["ctx"].close()
            fresh["ctx"] = nwe_amd.Renderer(host_only=True)
            S.configure(fresh["ctx"], st, grids)
            fresh["key"] = st.key()
        return fresh["ctx"]

    @functools.lru_cache(maxsize=None)
    def expected_grids(occ, cgrid, rgrid):
        """The getters of a context that was given these grids and nothing else."""
        f = nwe_amd.Renderer(host_only=True)
        try:
            for g, name in (("occ", occ), ("cgrid", cgrid), ("rgrid", rgrid)):
                if name is not None:
                    S.do_setter(f, ("set_" + g, name), grids)
            return S.grid_state(f)
        finally:
            f.close()

    def one_call(call, hook, ctx):
        nonlocal compared
        why = S.expect(st, call, hook)
        if call[0] in ("render", "render_rays"):
            got, want = _plan(r, call, hook), _plan(fresh_context(), call, hook)
            assert got == want, (ctx, call, got[:2], want[:2])
            assert (got[0] == 0) == (why is None), (ctx, call, why, got[:2])          # the generator's refusal bookkeeping
            if got[0] == 0:
                assert got[3] == S.table_use(st, call, hook)[1], (ctx, call, got[3], S.table_use(st, call, hook))
            compared += 1
            return got[0] == 0
        got = _host_call(r, st, call)
        if call[0] != "create_rays":
            want = _host_call(fresh_context(), st, call)
            assert got is not None and got == want, (ctx, call, got, want)
            # every refusal in front of "needs a device context" is reachable; a call the generator says renders gets as far as that
            if call[0] in ("render_grid", "render_sparse"):
                assert got[1].endswith("needs a device context") == (why is None or why == ("no_mfma_kernel",)), (ctx, call, why, got)
            compared += 1
        return None

    try:
        for i, step in enumerate(steps):
            ctx, op = (index, i, step), step[0]
            flags = []
            if op == "burst":               # its switches take effect between its calls
                for item in step[1] + ((step[2],) if step[2] is not None else ()):
                    if item[0] in S.RENDER_LIKE:
                        flags.append(one_call(item, None, ctx))
                    else:
                        S.do_setter(r, item, grids)
                        st.apply(item)
            elif op in S.RENDER_LIKE or op == "hooked":
                for call, hook in S.calls_of(step):
                    flags.append(one_call(call, hook, ctx))
            elif op in S.SCRATCH_USERS:
                grids[step[1]] = _fake_build(step)
                S.do_setter(r, ("set_" + {"build_occ": "occ", "bake_cgrid": "cgrid", "bake_rgrid": "rgrid"}[op], step[1]), grids)
                st.apply(step)
            elif op.startswith("refused_"):
                got = _raised(lambda: S.do_setter(r, step, grids))
                want = _raised(lambda: S.do_setter(fresh_context(), step, grids))
                assert got is not None and got == want, (ctx, got, want)
                assert (r.early_termination, r.shared_coarse) == (pytest.approx(st.eps), st.share_k), ctx
                compared += 1
            else:
                S.do_setter(r, step, grids)
                st.apply(step)
            planned.append(flags)
            assert S.grid_state(r) == expected_grids(st.occ, st.cgrid, st.rgrid), (ctx, "the grids after the step")
            assert (r.early_termination, r.shared_coarse, r.separate_passes) == (pytest.approx(st.eps), st.share_k, st.separate), ctx
            assert (r.debug_get_work_queue(), r.debug_get_colour_skip()) == (st.wq, st.cskip), ctx
            for w in (0, 1):
                assert r.mfma_supported(w) == st.mfma_ok(w), ctx
    finally:
        r.close()
        if fresh["ctx"] is not None:
            fresh["ctx"].close()
    return steps, planned, compared


@pytest.mark.parametrize("index", range(S.N_WALKS))
def test_the_walk_on_a_host_only_context_against_fresh_host_only_contexts(index):
    steps, _, compared = _walk_on_the_host(index)
    print(f"walk {index}: {len(steps)} steps, {compared} calls compared with a fresh host-only context")
    assert compared >= 40


@pytest.mark.parametrize("index", range(S.N_WALKS))
def test_the_generators_ring_model_is_the_count_of_recorded_launches(index):
    """The slot the generator predicts for every step is (launches recorded before it) mod 4, where a launch is a render / render_rays
    call that nwe_debug_plan planned on the fresh context - counted here from the step list, not by the generator."""
    steps, planned, _ = _walk_on_the_host(index)
    slots = S.predicted_slots(index)
    assert len(slots) == len(steps) == len(planned)
    launches, seen = 0, set()
    for i, flags in enumerate(planned):
        assert slots[i] == launches % 4, (index, i, steps[i])
        seen.add(slots[i])
        launches += sum(1 for f in flags if f)
    assert seen == {0, 1, 2, 3} and launches >= 16
