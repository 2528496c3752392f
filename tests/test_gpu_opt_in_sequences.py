"""The walks of tests/opt_in_sequences.py on the GPU, and the counted query kernels on every built shape.

1. Every call of a walk on ONE long-lived context gives what a FRESH context gives that was configured from `State` alone: every
   requested output and the flags word bit for bit (NaN equal to NaN), or the same exception with the same text.  No tolerance.
   After every step every report that the step's kind of call must not move is what it was; the reports a step does move that are
   no timings equal the fresh context's.  Grids made on the device are read back and equal the fresh context's build bit for bit.
2. The counted query (nwe_render_sparse_async's kernels) in all 28 MFMA instantiations and once in fp32, against the synchronous
   twin and against query_points.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib as L
from tests import coarse_grid as B
from tests import opt_in_sequences as S
from tests import radiance_grid as R
from tests import test_gpu_query as TQ
from tests import test_gpu_sparse_async as TA

pytestmark = pytest.mark.gpu

# ---- 1. the walks ---------------------------------------------------------------------------------------------------------------

TIMINGS = ("kernel_ms", "parts", "query_ms", "grid_ms", "sparse_ms", "coarse_ms")
_RENDER_MOVES = {"kernel_ms", "parts", "evals", "plan", "coarse_ms", "coarse_rays", "coarse_none"}
MOVES = {"render": _RENDER_MOVES, "render_rays": _RENDER_MOVES,
         "query": {"query_ms"}, "render_grid": {"grid_ms"}, "render_sparse": {"sparse_ms", "sparse_samples"}, "cgrid_weights": set(), "create_rays": set()}


def _or_none(call):
    try:
        return call()
    except RuntimeError:
        return None


def reports(r):
    """The nine reports; each blocks until the launch it describes has finished.  nwe_last_coarse_launch through the ABI itself: a
    launch without a coarse stage reports exactly -1 / 0 (include/nwe.h), which the wrapper would fold together with any negative
    time."""
    ms, rays = C.c_float(), C.c_int64()
    coarse = (ms.value, rays.value) if r._lib.nwe_last_coarse_launch(r._ctx, C.byref(ms), C.byref(rays)) == 0 else None
    return {"kernel_ms": r.last_kernel_ms(), "parts": _or_none(lambda: tuple(r.last_launch_parts())), "query_ms": r.last_query_ms(),
            "grid_ms": r.last_grid_ms(), "sparse_ms": r.last_sparse_ms(), "sparse_samples": r.last_sparse_samples(),
            "evals": _or_none(r.last_ray_evaluations), "plan": r.debug_last_plan(), "coarse_ms": coarse and coarse[0], "coarse_rays": coarse and coarse[1],
            "coarse_none": coarse and coarse[0] == -1.0}


TIMER_STEP_MS = 1e-5        # the 10 ns step of the event timer (include/nwe.h: nwe_last_launch_parts; kMinPartMs in csrc/nwe_abi.hip)


@functools.lru_cache(maxsize=None)
def _cloud(n):
    pts, dirs = TQ._cloud(n, n)
    return torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()


def do_call(r, st, call):
    """A render-like call on context r -> the wrapper's result dict."""
    op = call[0]
    if op == "query":
        pts, dirs = _cloud(call[4])
        return r.query_points(pts, None if st.noview(call[1]) else dirs, which=call[1], precision=call[2], outputs=(call[3],))
    (H, W), poses = S.FRAMES[call[-2]], S.poses_of(call[-1])
    cam = S.camera_of(H, W)
    if op == "render":
        return r.render(poses, H, W, precision=call[1], outputs=S.LEAN if call[2] == "lean" else S.FULL, **cam)
    if op == "render_rays":
        rays = r.create_rays(poses, H, W, use_view_dirs=not st.noview(0), **cam)
        return r.render_rays(rays, precision=call[1], outputs=S.LEAN if call[2] == "lean" else S.FULL)
    if op == "render_grid":
        return r.render_grid(poses, H, W, outputs=S.GRID_OUT[call[1]], **cam)
    if op == "render_sparse":
        return r.render_sparse(poses, H, W, which=call[3], precision=call[2], min_weight=call[4], dilate=call[5], outputs=S.SPARSE_OUT[call[6]],
                               asynchronous=call[1], **cam)
    if op == "cgrid_weights":
        return r.coarse_grid_weights(poses, H, W, **cam)
    if op == "create_rays":
        return {"rays": r.create_rays(poses, H, W, **cam)}
    raise AssertionError(call)


def attempt(r, st, call):
    """The result dict, or (exception type, text) of a refused call."""
    try:
        return do_call(r, st, call)
    except (RuntimeError, ValueError) as e:
        return type(e), str(e)


def same_result(got, want, ctx):
    assert isinstance(got, tuple) == isinstance(want, tuple), (ctx, got if isinstance(got, tuple) else "rendered", want if isinstance(want, tuple) else "rendered")
    if isinstance(got, tuple):
        assert got == want, (ctx, got, want)                # the exception type and the whole text
        return 0
    keys = [k for k in want if not k.startswith("_")]
    assert sorted(keys) == sorted(k for k in got if not k.startswith("_")), ctx
    for k in keys:
        a, b = got[k], want[k]
        if a.dtype == torch.float32:
            assert S.bits_equal(a, b), (ctx, k)
        else:
            assert a.shape == b.shape and torch.equal(a, b), (ctx, k)
    return len(keys)


def untouched_by_the_refused_call(r, st, call, ctx):
    """The refused render / render_rays / render_grid / render_sparse call again, through the ABI with buffers that hold a sentinel:
    it writes nothing."""
    op, (H, W), poses = call[0], S.FRAMES[call[-2]], S.poses_of(call[-1]).astype(np.float32)
    n = H * W * call[-1]
    cam = S.camera_of(H, W)
    if op in ("render_grid", "render_sparse"):
        sparse = op == "render_sparse"
        names = (S.SPARSE_OUT[call[6]] if sparse else S.GRID_OUT[call[1]]) + ("flags",)
        with torch.cuda.device(r.device):
            # each buffer as large as its output would be, in floats (`selected` is bytes: more than enough)
            s = st.ns + st.ni
            size = {"rgb": 3 * n, "depth": n, "acc": n, "weights_coarse": n * st.ns, "z_fine": n * s, "weights_grid": n * s, "selected": n * s,
                    "raw_fine": 4 * n * s, "flags": 1}
            res = {k: torch.full((size[k],), 123.0, device=r.device) for k in names}
            o = (L.SparseOutputs if sparse else L.GridOutputs)(**{k: v.data_ptr() for k, v in res.items()})
            head = (r._ctx, poses.ctypes.data, call[-1], H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"], cam["far"], 0, H)
            if sparse:
                entry = r._lib.nwe_render_sparse_async if call[1] else r._lib.nwe_render_sparse
                rc = entry(*head, call[3], L.PRECISIONS[call[2]], call[4], call[5], C.byref(o), None)
            else:
                rc = r._lib.nwe_render_grid(*head, C.byref(o), None)
            torch.cuda.synchronize()
        assert rc != 0, ctx
        for k, v in res.items():
            assert bool((v == 123.0).all()), (ctx, k, "written by a refused call")
        return
    outputs = S.LEAN if call[2] == "lean" else S.FULL
    with torch.cuda.device(r.device):
        o, res = r._alloc(n, outputs)
        for k, v in res.items():
            v.fill_(7 if k == "flags" else 123.0)
        if op == "render":
            rc = r._lib.nwe_render(r._ctx, poses.ctypes.data, call[-1], H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"], cam["far"], 0, H,
                                   L.PRECISIONS[call[1]], C.byref(o), None)
        else:
            rays = torch.zeros(n, r.ray_columns, device=r.device)
            rc = r._lib.nwe_render_rays(r._ctx, rays.data_ptr(), n, L.PRECISIONS[call[1]], C.byref(o), None)
        torch.cuda.synchronize()
    assert rc != 0, ctx
    for k, v in res.items():
        assert bool((v == (7 if k == "flags" else 123.0)).all()), (ctx, k, "written by a refused call")


class HookBuffers:
    """One live buffer set for the hooks, sized for the largest call any walk makes (two poses of 40 x 64 rays at 64 + 128 samples)
    though a hooked step has 133 rays at the most: every later call of the walk finds the buffers alive and large enough, so a hook
    that stayed armed shows as a value difference, never as a fault."""
    R, NS, S = 2 * 40 * 64, 64, 192

    def __init__(self):
        assert 2 * max(h * w for h, w in S.FRAMES) <= self.R and max(ns for ns, _ in S.SAMPLINGS) <= self.NS and max(map(sum, S.SAMPLINGS)) <= self.S
        z = lambda n: torch.zeros(n, device="cuda")
        self.buf = {"z": z(self.R * self.S), "raw_c": z(self.R * self.NS * 4), "raw_f": z(self.R * self.S * 4), "w": z(self.R * self.NS),
                    "t_rand": z(self.R * self.NS), "noise_c": z(self.R * self.NS), "noise_f": z(self.R * self.S), "u": z(self.R * self.S)}

    def fill(self, n_rays, ns, ni):
        """Contents that depend on (rays, sampling) only, so that a fresh context's result can be kept."""
        assert n_rays <= self.R and ns <= self.NS and ns + ni <= self.S
        g = torch.Generator().manual_seed(n_rays * 1000003 + ns * 1009 + ni)
        s = ns + ni
        rows = {"z": torch.sort(S.Q.NEAR + (S.Q.FAR - S.Q.NEAR) * torch.rand(n_rays, s, generator=g), dim=-1).values,
                "raw_c": torch.randn(n_rays, ns, 4, generator=g), "raw_f": torch.randn(n_rays, s, 4, generator=g),
                "w": torch.rand(n_rays, ns, generator=g), "t_rand": torch.rand(n_rays, ns, generator=g),
                "noise_c": torch.randn(n_rays, ns, generator=g), "noise_f": torch.randn(n_rays, s, generator=g),
                "u": torch.sort(torch.rand(n_rays, ni, generator=g), dim=-1).values}
        for k, v in rows.items():
            self.buf[k][:v.numel()] = v.reshape(-1).cuda()

    def arm(self, r, hook):
        p = lambda k: self.buf[k].data_ptr()
        lib, ctx = r._lib, r._ctx
        if hook == "fine_depths":
            assert lib.nwe_debug_set_fine_depths(ctx, p("z")) == 0
        elif hook == "raw":
            assert lib.nwe_debug_set_raw(ctx, p("raw_c"), p("raw_f")) == 0
        elif hook == "coarse_weights":
            assert lib.nwe_debug_set_coarse_weights(ctx, p("w")) == 0
        else:
            assert lib.nwe_set_train_tables(ctx, p("t_rand"), p("noise_c"), p("noise_f"), p("u")) == 0


class Walk:
    def __init__(self, index):
        self.index = index
        self.steps, self.cover = S.make_walk(index)
        self.grids = S.Grids()
        self.st = S.State()
        self.r = nwe_amd.Renderer(0)
        S.configure(self.r, self.st, self.grids)
        self.hooks = HookBuffers()
        self.cache = {}
        self.compared = self.refused = self.outputs = self.fresh_made = 0

    def fresh(self, call, hook=None, st=None):
        """(result or refusal, the reports that are no timings) of `call` on a context made for it; kept by (state, call, hook)."""
        st = st or self.st
        key = (st.key(), call, hook)
        if key not in self.cache:
            f = nwe_amd.Renderer(0)
            try:
                S.configure(f, st, self.grids)
                if hook:
                    self.hooks.arm(f, hook)
                res = attempt(f, st, call)
                torch.cuda.synchronize()
                self.cache[key] = (res, reports(f))
                self.fresh_made += 1
            finally:
                f.close()
        return self.cache[key]

    def compare(self, call, got, ctx, hook=None, st=None):
        want, want_reports = self.fresh(call, hook, st)
        n = same_result(got, want, ctx)
        self.compared += 1
        self.refused += isinstance(got, tuple)
        self.outputs += n
        return want, want_reports

    def reports_after(self, before, moved, ctx):
        after = reports(self.r)
        for k, v in before.items():
            if k not in moved:
                assert after[k] == v, (ctx, k, "moved by a step that must not move it", v, after[k])       # times too: exactly
        return after

    def single(self, call, ctx, hook=None):
        """One call, compared at once; -> the reports it may move."""
        got = attempt(self.r, self.st, call)
        torch.cuda.synchronize()
        want, want_reports = self.compare(call, got, ctx, hook)
        if isinstance(got, tuple):
            if call[0] in ("render", "render_rays", "render_grid", "render_sparse"):
                untouched_by_the_refused_call(self.r, self.st, call, ctx)
            return set(), None
        return MOVES[call[0]], (call, want_reports)

    def run(self):
        r, st = self.r, self.st
        for i, step in enumerate(self.steps):
            ctx, op = (self.index, i, step), step[0]
            before = reports(r)
            moved, last = set(), None
            if op in S.RENDER_LIKE:
                moved, last = self.single(step, ctx)
            elif op == "hooked":
                _, hook, between, rays_call = step
                self.hooks.fill(S.n_rays_of(rays_call), st.ns, st.ni)
                self.hooks.arm(r, hook)
                m1, _ = self.single(between, ctx + ("between",))         # neither uses nor clears the hook
                m2, last = self.single(rays_call, ctx + ("hooked",), hook)
                moved = m1 | m2
            elif op == "burst":
                moved = self.burst(step, ctx)
            elif op in S.SCRATCH_USERS:
                S.do_build(r, st, step)
                made = S.read_grid(r, op)
                f = nwe_amd.Renderer(0)
                try:
                    S.configure(f, st, self.grids)
                    S.do_build(f, st, step)
                    want = S.read_grid(f, op)
                finally:
                    f.close()
                for k in ("lo", "hi", "res"):
                    assert tuple(made[k]) == tuple(want[k]), (ctx, k)
                assert made["values"].shape == want["values"].shape and made["values"].tobytes() == want["values"].tobytes(), (ctx, "the grid made on the device")
                self.grids[step[1]] = made
                self.compared += 1
            elif op.startswith("refused_"):
                got = _refusal(lambda: S.do_setter(r, step, self.grids))
                f = nwe_amd.Renderer(0)
                try:
                    S.configure(f, st, self.grids)
                    want = _refusal(lambda: S.do_setter(f, step, self.grids))
                finally:
                    f.close()
                assert got is not None and got == want, (ctx, got, want)
            else:
                S.do_setter(r, step, self.grids)
            if not op.startswith("refused_"):
                st.apply(step)
            after = self.reports_after(before, moved, ctx)
            if last is not None:            # the reports the call moved that are no timings are the fresh context's
                call, want = last
                for k in MOVES[call[0]] - set(TIMINGS):
                    if k == "plan" and call[1] == "f32":
                        continue            # the fp32 launcher has no plan: the report keeps the last MFMA launch's
                    assert after[k] == want[k], (ctx, k, after[k], want[k])
                if call[0] in ("render", "render_rays"):
                    # include/nwe.h: nwe_last_kernel_ms spans the call's launches; the parts describe the main stage's and add up to
                    # its time to within the timer's step (a part below it is reported as the step); nwe_last_coarse_launch is the
                    # producer's time in front of them - whatever slot of the ring the launch took and whatever used that slot before
                    total, ms = sum(p[0] for p in after["parts"]) + (0.0 if after["coarse_none"] else after["coarse_ms"]), after["kernel_ms"]
                    assert ms > 0 and abs(total - ms) <= 3 * TIMER_STEP_MS + 4.0 * float(np.spacing(np.float32(ms))), (ctx, "parts", after["parts"], after["coarse_ms"], ms)
                    assert sum(p[1] for p in after["parts"]) == S.n_rays_of(call), (ctx, after["parts"])
            assert ((r.occupancy is None), (r.coarse_grid is None), (r.radiance_grid is None)) == ((st.occ is None), (st.cgrid is None), (st.rgrid is None)), ctx

    def burst(self, step, ctx):
        """The calls queued behind some tens of milliseconds of other work with no host synchronisation between them - host-side
        switches flipped in between reach the calls behind them only - then, perhaps, a setter that must wait for them; each call
        is compared afterwards, against a fresh context in the state the call was made in."""
        r, now = self.r, self.st.copy()
        _, items, setter = step
        TA._busy(r.device)
        made = []
        for item in items:
            if item[0] in S.RENDER_LIKE:
                made.append((item, attempt(r, now, item), now.copy()))
            else:
                S.do_setter(r, item, self.grids)
                now.apply(item)
        if setter is not None:
            S.do_setter(r, setter, self.grids)
        torch.cuda.synchronize()
        moved = set()
        for j, (call, res, st) in enumerate(made):
            self.compare(call, res, ctx + (j, call), st=st)
            if not isinstance(res, tuple):
                moved |= MOVES[call[0]]
            elif setter is None and st.key() == now.key() and call[0] in ("render", "render_rays", "render_grid", "render_sparse"):
                untouched_by_the_refused_call(r, st, call, ctx + (j, call))      # the context is still in the state that refused it
        return moved

    def close(self):
        self.r.close()


def _refusal(call):
    try:
        call()
    except (RuntimeError, ValueError) as e:
        return type(e), str(e)
    return None


@pytest.mark.parametrize("index", range(S.N_WALKS))
def test_seeded_walk_over_the_opt_in_state(index):
    t0 = time.perf_counter()
    w = Walk(index)
    try:
        w.run()
    finally:
        w.close()
    print(f"\nwalk {index} (seed {S.WALKS[index][0]}): {len(w.steps)} steps, {w.compared} comparisons with {w.fresh_made} fresh contexts "
          f"({w.refused} refusals, {w.outputs} outputs compared bit for bit), {time.perf_counter() - t0:.2f} s")
    assert w.compared >= 40 and w.compared - w.refused >= 20 and w.refused >= 5
    gaps = S.coverage_gaps(w.cover, (index, S.N_WALKS))
    assert not gaps, gaps                                       # this walk's share of the table ...
    assert not S.coverage_gaps(S.union_coverage())              # ... and the table


# ---- 2. the counted query on every built shape ----------------------------------------------------------------------------------

def _counted(r, view, precision, packet):
    """An asynchronous sparse frame of 5 x 9 rays at 3 + 1 in one chunk: everything selected - 180 points, one full packet of 128 and
    a ragged one - then a threshold from the call's own weights_grid that selects fewer than 128 and more than none."""
    H, W = 5, 9
    poses, _ = B.G.E.frame_rays(H, W, 1)
    got, count = TA._twin(r, poses, H, W, "all", precision=precision, min_weight=-1.0, dilate=0)
    assert count == (180, 180) and bool(got["selected"].bool().all())
    TA._rows_are_the_querys(r, poses, H, W, got, precision, view)
    min_weight, k = TA._threshold_for(got["weights_grid"].cpu().numpy(), 33, 128, packet)      # more than a wave, less than a packet
    got, count = TA._twin(r, poses, H, W, "ragged", precision=precision, min_weight=min_weight, dilate=0)
    assert count == (k, 180) and 0 < k < 128 and int(got["selected"].sum()) == k
    TA._rows_are_the_querys(r, poses, H, W, got, precision, view)
    return k


def _shape_renderer(D, Wn, view, fold, seed=1000):
    g = R.grid("smooth")
    r = nwe_amd.Renderer(0)
    r.debug_set_fold(fold)
    for which in (0, 1):
        r.set_network(which, nwe_amd.synthetic.make_state_dict(seed + which, D, Wn, use_view_dirs=view))
    r.set_sampling(3, 1)
    r.set_radiance_grid(g["values"], g["lo"], g["hi"])
    return r


@pytest.mark.parametrize("precision", ["f16x3", "f16x1"])
@pytest.mark.parametrize("name,D,Wn,view,fold", TQ.SHAPES, ids=[s[0] for s in TQ.SHAPES])
def test_the_counted_query_on_every_built_shape(name, D, Wn, view, fold, precision):
    """The 14 instantiations and the two reference-formulation shapes, in two precisions: DESIGN.md 5.9's 28 counted kernels, each
    through its dispatcher row, its LDS layout and its n_chunks check."""
    r = _shape_renderer(D, Wn, view, fold)
    try:
        assert r.mfma_supported(1)
        k = _counted(r, view, precision, 128)
        print(f"counted query, {name} {precision}: 180 of 180, then {k} of 180")
    finally:
        r.close()


def test_the_fp32_counted_query_on_a_shape_without_an_mfma_kernel():
    """Width 64, depth 5, skip after layer 2 (tests/test_gpu_query.py's fp32 shape): packets of 16 points."""
    g = R.grid("smooth")
    r = nwe_amd.Renderer(0)
    try:
        for which in (0, 1):
            r.set_network(which, nwe_amd.synthetic.make_state_dict(12 + which, 5, 64, skips=(2,)))
        r.set_sampling(3, 1)
        r.set_radiance_grid(g["values"], g["lo"], g["hi"])
        assert not r.mfma_supported(1)
        k = _counted(r, True, "f32", 16)
        print(f"counted query, 5x64 f32: 180 of 180, then {k} of 180")
    finally:
        r.close()
