"""Call sequences on ONE long-lived context against fresh contexts (include/nwe.h: what a context carries from call to call).

The application keeps one context for the life of the GUI: it reloads models, changes the sampling, toggles options and
renders from whatever stream torch hands it.  The yardstick here is a FRESH context: the same call on a context created for
that one call and configured with only the state that is current must give every requested output and the flags word bit
for bit (the kernels are deterministic: test_repeated_renders_are_bit_identical, test_gpu_coarse_density_only.py), so there
is no tolerance anywhere in this file except the one comparison against fp64 at the end, which is tests/accuracy.py's.

1. a seeded walk of 121 steps over one context (reconfiguration, toggles, every precision, every kind of call, refused
   calls), compared with a fresh context after every rendering step;
2. the one-shot hooks of nwe_render_rays and calls that fail: a refused call consumes them, nwe_render leaves them alone;
3. the timing calls (nwe_last_kernel_ms, nwe_last_launch_parts) describe the last launch that was MADE;
4. reconfiguring while a launch is in flight on a side stream;
5. the white background on every path the product runs (lean frames, render_rays, the f32 kernel, tiles, ni = 0).

One refusal that the render entry points document cannot be reached through the ABI: "n_samples above the MFMA limit" - the
limit equals nwe_set_sampling's own bound (128), which refuses first.  The walk therefore makes THAT refusal
(nwe_set_sampling with 129 samples, NWE_ERR_UNSUPPORTED) and checks that it leaves the tables and counts alone.

Every buffer handed to a hook stays referenced by the test for as long as the context lives and is sized for every call
that follows, so that a stale hook would read live memory and show up as a value difference, never as a fault.
"""
import ctypes as C
import functools
import random
import time

import pytest
import torch

import nwe_amd
from nwe_amd import _lib as L
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import accuracy as A
from tests.test_gpu_coarse_density_only import FULL, LEAN, _assert_lean_equals_full

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.1, 10.0
WALK_FULL = ("rgb", "depth", "acc", "disp", "rgb_coarse", "depth_coarse", "acc_coarse")   # coarse slots are written with ni = 0 too
FRAMES = ((7, 19), (3, 9))                 # 133 rays (not a multiple of 128) and 27 rays (below 32)
PRECISIONS = ("f16x3", "f16x1", "f32")


def _pose(yaw=-30.0):
    return O.camera_pose((0.0, -0.5, -0.77, 0.0, -90.0, 0.0), (0, 0, 0, yaw, 0.0, 0.0))[0].numpy()


def _kw(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


def bits_equal(a, b):
    """Bit for bit (NaN included: a disparity of 1/0 is NaN in both or in neither)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_same(got, want, outputs, ctx):
    for k in tuple(outputs) + ("flags",):
        assert bits_equal(got[k], want[k]), (ctx, k)


# ------------------------------------------------------------------------------------------------------------------------
# 1. the walk
# ------------------------------------------------------------------------------------------------------------------------

KINDS = {
    "8x256": dict(D=8, W=256),
    "4x128": dict(D=4, W=128),
    "6x256": dict(D=6, W=256),                       # its lean frames keep the coarse colour
    "generic": dict(D=6, W=64, skips=(2,)),          # no MFMA instantiation: the f32 kernel only
    "noview": dict(D=4, W=128, use_view_dirs=False),
}
UNFOLDABLE = ("8x256", "4x128")                      # debug_set_fold(False) has an MFMA kernel for these two only
SAMPLINGS = ((64, 128), (37, 17), (16, 0), (8, 5), (24, 40))
WALK_SEED, WALK_STEPS = 39, 120          # the first seed whose walk meets WALK_MUST_COVER at this length (checked on the CPU)


@functools.lru_cache(maxsize=None)
def _sd(kind, seed):
    return synthetic.make_state_dict(seed, **KINDS[kind])


class State:
    """What a context holds after the steps so far (and all a fresh context is configured with)."""

    def __init__(self):
        self.nets = [("8x256", 100, True), ("8x256", 101, True)]     # (kind, seed, folded at upload)
        self.ns, self.ni = 64, 128
        self.white, self.decomp = False, -1

    def copy(self):
        s = State()
        s.nets, s.ns, s.ni, s.white, s.decomp = list(self.nets), self.ns, self.ni, self.white, self.decomp
        return s

    def mfma_ok(self, which):
        kind, _, fold = self.nets[which]
        return kind != "generic" and (kind == "noview" or fold or kind in UNFOLDABLE)

    def form(self, which):
        kind, _, fold = self.nets[which]
        return (KINDS[kind]["D"], KINDS[kind]["W"], "noview" if kind == "noview" else ("folded" if fold else "reference"))

    def noview(self, which):
        return self.nets[which][0] == "noview"

    def expect(self, precision, feat_map=False):
        """(NWE_ERR_* or 0, reason) of a render call in this state: the order of check_ready and launch() in csrc/nwe_abi.hip."""
        if self.ni > 0 and self.noview(0) != self.noview(1):
            return L.NWE_ERR_STATE, "view_dirs"
        if feat_map:
            if self.ni <= 0 or self.noview(1):
                return L.NWE_ERR_INVALID, "feat_map_needs_fine"
            if precision != "f32":
                return L.NWE_ERR_UNSUPPORTED, "feat_map_mfma"
        if precision != "f32":
            if not self.mfma_ok(0) or (self.ni > 0 and not self.mfma_ok(1)):
                return L.NWE_ERR_UNSUPPORTED, "no_mfma_kernel"
            if self.ni > 0 and self.form(0) != self.form(1):
                return L.NWE_ERR_UNSUPPORTED, "same_shape"          # refused inside launch()
        return 0, "ok"

    def apply(self, step):
        op = step[0]
        if op == "sampling":
            self.ns, self.ni = step[1], step[2]
        elif op == "net":
            _, which, kind, seed, fold = step
            for w in ((0, 1) if which == 2 else (which,)):
                self.nets[w] = (kind, seed + w, fold)
        elif op == "white":
            self.white = step[1]
        elif op == "decomp":
            self.decomp = step[1]


def make_walk(seed=WALK_SEED, n_steps=WALK_STEPS):
    """The step list (>= n_steps steps) and its coverage counts; pure Python, so the coverage can be checked without a GPU
    (tests/test_host_logic.py does).  Macro choices emit several steps: a refusal that needs a particular state first moves
    the context into it with ordinary set_network steps."""
    rng = random.Random(seed)
    st, steps, cover = State(), [], {}
    next_seed = [200]

    def count(key):
        cover[key] = cover.get(key, 0) + 1

    def emit(step):
        steps.append(step)
        op = step[0]
        if op in ("render", "render_rays"):
            code, reason = st.expect(step[1])
            if code:
                count(("refused", reason))
            else:
                count(("op", op)); count(("pair", step[1], step[2])); count(("frame", step[3]))
        elif op == "sampling":
            if step[2] == 0:
                count(("sampling", "to_ni_0"))
            elif st.ni == 0:
                count(("sampling", "back_from_ni_0"))
            if step[1] < st.ns and step[2] < st.ni:
                count(("sampling", "shrinks_both"))
            count(("op", op))
        elif op == "net":
            count(("op", "net_both" if step[1] == 2 else ("net_coarse_only", "net_fine_only")[step[1]]))
            count(("kind", step[2]))
            if not step[4]:
                count(("op", "unfolded_upload"))
        elif op == "refuse_feat_map":
            count(("refused", st.expect(step[1], True)[1]))
        elif op.startswith("refuse_"):
            count(("refused", op[len("refuse_"):]))
        else:
            count(("op", op))
        st.apply(step)

    def new_seed():
        next_seed[0] += 2
        return next_seed[0]

    def render_step(prec=None):
        prec = prec or rng.choice(PRECISIONS)
        return (rng.choice(("render", "render_rays")), prec, rng.choice(("lean", "full")), rng.randrange(len(FRAMES)))

    def valid_precisions():
        return [p for p in PRECISIONS if st.expect(p)[0] == 0]

    while True:
        c = rng.choices(("render", "sampling", "net_both", "net_one", "refold", "white", "decomp", "create_rays", "to8b", "refuse_struct",
                         "refuse_feat_map", "refuse_sampling", "refuse_no_kernel", "refuse_view_dirs", "refuse_same_shape"),
                        weights=(14, 4, 3, 3, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1))[0]
        if c == "render":
            ok = valid_precisions()
            if ok:
                emit(render_step(rng.choice(ok)))
        elif c == "sampling":
            emit(("sampling",) + rng.choice([s for s in SAMPLINGS if s != (st.ns, st.ni)]))
        elif c == "net_both":
            emit(("net", 2, rng.choice(tuple(KINDS)), new_seed(), True))
        elif c == "net_one":        # only the coarse or only the fine network, same kind and form, other weights
            which = rng.randrange(2)
            kind, _, fold = st.nets[which]
            emit(("net", which, kind, new_seed() - which, fold))
        elif c == "refold":         # debug_set_fold(False) and a re-upload (or back)
            if st.nets[0][0] in UNFOLDABLE and st.nets[0][0] == st.nets[1][0]:
                emit(("net", 2, st.nets[0][0], new_seed(), not st.nets[0][2]))
        elif c == "white":
            emit(("white", not st.white))
        elif c == "decomp":
            emit(("decomp", rng.choice([m for m in (-1, 0, 1, 2) if m != st.decomp])))
        elif c in ("create_rays", "to8b"):
            emit((c, rng.randrange(len(FRAMES))))
        elif c == "refuse_struct":
            emit(("refuse_struct", rng.choice(PRECISIONS)))
        elif c == "refuse_feat_map":
            emit(("refuse_feat_map", rng.choice(("f16x3", "f16x1"))))
        elif c == "refuse_sampling":
            emit(("refuse_sampling", 129, rng.choice((0, 64))))
        elif c == "refuse_no_kernel":      # an MFMA precision on a shape without MFMA kernel, then the f32 kernel on it
            emit(("net", 2, "generic", new_seed(), True))
            emit(render_step(rng.choice(("f16x3", "f16x1"))))
            emit(render_step("f32"))
        elif c == "refuse_view_dirs":      # one network with, one without view directions (refused only with a fine pass)
            if st.ni > 0:
                which = rng.randrange(2)
                back = st.nets[which]
                emit(("net", which, "8x256" if st.noview(which) else "noview", new_seed() - which, True))
                emit(render_step())
                emit(("net", which, back[0], back[1] - which, back[2]))
        elif c == "refuse_same_shape":     # both have an MFMA kernel but not the same one: refused inside launch(); f32 takes it
            if st.ni > 0 and not st.noview(0) and not st.noview(1) and st.mfma_ok(1):
                emit(("net", 0, "4x128" if st.nets[1][0] != "4x128" else "8x256", new_seed(), True))
                emit(render_step(rng.choice(("f16x3", "f16x1"))))
                emit(render_step("f32"))
        if len(steps) >= n_steps and valid_precisions():
            emit(render_step(rng.choice(valid_precisions())))      # the walk ends on a comparison
            return steps, cover


WALK_MUST_COVER = (
    [("op", o) for o in ("render", "render_rays", "sampling", "net_both", "net_coarse_only", "net_fine_only", "unfolded_upload", "white", "decomp",
                         "create_rays", "to8b")] +
    [("kind", k) for k in KINDS] +
    [("pair", p, o) for p in PRECISIONS for o in ("lean", "full")] +
    [("frame", i) for i in range(len(FRAMES))] +
    [("sampling", s) for s in ("to_ni_0", "back_from_ni_0", "shrinks_both")] +
    [("refused", r) for r in ("struct", "feat_map_mfma", "sampling", "no_mfma_kernel", "view_dirs", "same_shape")])


def walk_coverage_gaps(cover):
    """Every operation class, every (precision, lean | full) pair and every refusal at least twice."""
    return [k for k in WALK_MUST_COVER if cover.get(k, 0) < 2]


def _configure(r, st):
    for which in (0, 1):
        kind, seed, fold = st.nets[which]
        r.debug_set_fold(fold)
        r.set_network(which, _sd(kind, seed))
    r.set_sampling(st.ns, st.ni)
    r.set_white_background(st.white)
    r.debug_set_decomposition(st.decomp)


def _upload(r, step):
    _, which, kind, seed, fold = step
    r.debug_set_fold(fold)
    for w in ((0, 1) if which == 2 else (which,)):
        r.set_network(w, _sd(kind, seed + w))


def _call(r, st, step):
    """A render / render_rays step on context r -> the wrapper's result dict and the outputs asked for."""
    op, prec, which, frame = step
    H, W = FRAMES[frame]
    outputs = LEAN if which == "lean" else WALK_FULL
    if op == "render":
        return r.render(_pose(), H, W, precision=prec, outputs=outputs, **_kw(H, W)), outputs
    rays = r.create_rays(_pose(), H, W, use_view_dirs=not st.noview(0), **_kw(H, W))
    return r.render_rays(rays, precision=prec, outputs=outputs), outputs


def _fresh_call(st, step, white=None):
    f = nwe_amd.Renderer(0)
    try:
        _configure(f, st)
        if white is not None:
            f.set_white_background(white)
        res, _ = _call(f, st, step)
        torch.cuda.synchronize()
        return res
    finally:
        f.close()


def _raw_render_rays(r, rays, precision, outputs, struct_bytes=None, null_rays=False):
    """nwe_render_rays through ctypes without the wrapper's own checks -> (return code, result dict)."""
    with torch.cuda.device(r.device):
        o, res = r._alloc(rays.shape[0], outputs)
        if struct_bytes is not None:
            o.struct_bytes = struct_bytes
        code = precision if isinstance(precision, int) else L.PRECISIONS[precision]
        rc = r._lib.nwe_render_rays(r._ctx, None if null_rays else rays.data_ptr(), rays.shape[0], code, C.byref(o),
                                    torch.cuda.current_stream(r.device).cuda_stream)
    res["_rays"] = rays
    return rc, res


def _assert_refused(r, rc, code, ctx):
    assert rc == code, (ctx, rc, code)
    assert r._lib.nwe_last_error(r._ctx).decode() != "", ctx


_EXC = {L.NWE_ERR_UNSUPPORTED: NotImplementedError, L.NWE_ERR_INVALID: ValueError, L.NWE_ERR_STATE: RuntimeError}


def test_seeded_walk_over_one_context():
    steps, cover = make_walk()
    for i, s in enumerate(steps):
        print(f"step {i:3d}: {s}")
    assert len(steps) >= 60
    r, st = nwe_amd.Renderer(0), State()
    _configure(r, st)
    compared = 0
    try:
        for i, step in enumerate(steps):
            op, ctx = step[0], (i, step)
            if op in ("render", "render_rays"):
                code, reason = st.expect(step[1])
                if code:
                    with pytest.raises(_EXC[code]) as e:
                        _call(r, st, step)
                    assert type(e.value) is _EXC[code] and str(e.value).split(": ", 1)[1] != "", ctx
                else:
                    got, outputs = _call(r, st, step)
                    assert_same(got, _fresh_call(st, step), outputs, ctx)
                    if st.white:          # the identity the existing white-background test asserts, against a context without it
                        off = _fresh_call(st, (step[0], step[1], "full", step[3]), white=False)
                        assert bits_equal(got["rgb"], off["rgb"] + (1.0 - off["acc"])[..., None]), ctx
                        assert bits_equal(got["acc"], off["acc"]) and bits_equal(got["depth"], off["depth"]), ctx
                    compared += 1
            elif op == "sampling":
                r.set_sampling(step[1], step[2])
            elif op == "net":
                _upload(r, step)
                after = st.copy()
                after.apply(step)
                for w in (0, 1):
                    assert r.mfma_supported(w) == after.mfma_ok(w), ctx
            elif op == "white":
                r.set_white_background(step[1])
            elif op == "decomp":
                r.debug_set_decomposition(step[1])
            elif op == "create_rays":
                H, W = FRAMES[step[1]]
                f = nwe_amd.Renderer(0)
                try:
                    assert bits_equal(r.create_rays(_pose(), H, W, **_kw(H, W)), f.create_rays(_pose(), H, W, **_kw(H, W))), ctx
                finally:
                    f.close()
            elif op == "to8b":
                x = torch.linspace(-0.25, 1.25, 3 * FRAMES[step[1]][0] * FRAMES[step[1]][1], device="cuda").reshape(-1, 3)
                want = (255.0 * x.clamp(0.0, 1.0)).to(torch.uint8)           # model_utils.py:9, truncation
                assert torch.equal(r.to8b(x), want), ctx
            elif op == "refuse_struct":
                rays = torch.zeros(5, r.ray_columns, device="cuda")
                rc, _ = _raw_render_rays(r, rays, step[1], LEAN, struct_bytes=C.sizeof(L.Outputs) - 8)
                _assert_refused(r, rc, L.NWE_ERR_INVALID, ctx)
            elif op == "refuse_feat_map":
                code, _ = st.expect(step[1], feat_map=True)
                rays = torch.zeros(5, r.ray_columns, device="cuda")
                o, res = r._alloc(5, LEAN)
                keep = torch.zeros(5, 256, device="cuda")                    # never written: the call is refused
                o.feat_map = keep.data_ptr()
                rc = r._lib.nwe_render_rays(r._ctx, rays.data_ptr(), 5, L.PRECISIONS[step[1]], C.byref(o), None)
                _assert_refused(r, rc, code, ctx)
            elif op == "refuse_sampling":
                t = torch.linspace(0., 1., steps=step[1])
                omt, u = 1. - t, torch.linspace(0., 1., steps=max(step[2], 1))
                rc = r._lib.nwe_set_sampling(r._ctx, t.numpy().ctypes.data, omt.numpy().ctypes.data, step[1], u.numpy().ctypes.data, step[2])
                _assert_refused(r, rc, L.NWE_ERR_UNSUPPORTED, ctx)
            else:
                raise AssertionError(step)
            st.apply(step)
    finally:
        r.close()
    print(f"{len(steps)} steps, {compared} renders compared with a fresh context; coverage {sorted(cover.items(), key=str)}")
    assert not walk_coverage_gaps(cover), walk_coverage_gaps(cover)


# ------------------------------------------------------------------------------------------------------------------------
# 2. hooks and failed calls
# ------------------------------------------------------------------------------------------------------------------------

HNS, HNI, HR = 16, 24, 133
HOOK_OUT = ("rgb", "depth", "acc", "rgb_coarse", "z_fine")
HOOKED_OUT = ("rgb", "depth", "acc", "z_fine")        # with given coarse weights the coarse outputs are not written (include/nwe.h)
HOOKS = ("fine_depths", "raw", "coarse_weights", "train_tables")


class HookBench:
    """A 4x128 context at 16 + 24 samples, 133 rays, and one live, full-size buffer set per hook."""

    def __init__(self):
        self.sd = (synthetic.thin_fog(_sd("4x128", 300)), _sd("4x128", 301))
        self.r = self.context()
        self.rays = self.r.create_rays(_pose(), 7, 19, **_kw(7, 19))
        g = torch.Generator().manual_seed(5)
        S = HNS + HNI
        z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(HR, S, generator=g), dim=-1).values
        self.buf = {                              # float32, contiguous, on the device: .to() / .contiguous() return these very tensors
            "z": z.cuda(), "raw_c": torch.randn(HR, HNS, 4, generator=g).cuda(), "raw_f": torch.randn(HR, S, 4, generator=g).cuda(),
            "w": torch.rand(HR, HNS, generator=g).cuda(), "t_rand": torch.rand(HR, HNS, generator=g).cuda(),
            "noise_c": torch.randn(HR, HNS, generator=g).cuda(), "noise_f": torch.randn(HR, S, generator=g).cuda(),
            "u": torch.sort(torch.rand(HR, HNI, generator=g), dim=-1).values.cuda()}
        f = self.context()
        self.plain = {p: f.render_rays(self.rays, precision=p, outputs=HOOK_OUT) for p in PRECISIONS}       # hook-free, fresh context
        self.plain_pinhole = f.render(_pose(), 7, 19, precision="f16x3", outputs=LEAN, **_kw(7, 19))
        torch.cuda.synchronize()
        f.close()

    def context(self):
        r = nwe_amd.Renderer(0)
        r.set_network(0, self.sd[0])
        r.set_network(1, self.sd[1])
        r.set_sampling(HNS, HNI)
        return r

    def arm(self, r, hook):
        """Through the C setters directly, as a C caller would."""
        b, lib, ctx = self.buf, r._lib, r._ctx
        p = lambda k: b[k].data_ptr()
        if hook == "fine_depths":
            assert lib.nwe_debug_set_fine_depths(ctx, p("z")) == 0
        elif hook == "raw":
            assert lib.nwe_debug_set_raw(ctx, p("raw_c"), p("raw_f")) == 0
        elif hook == "coarse_weights":
            assert lib.nwe_debug_set_coarse_weights(ctx, p("w")) == 0
        else:
            assert lib.nwe_set_train_tables(ctx, p("t_rand"), p("noise_c"), p("noise_f"), p("u")) == 0

    def wrapper_kwargs(self, hook):
        b = self.buf
        return {"fine_depths": dict(debug_fine_depths=b["z"]), "raw": dict(debug_raw=(b["raw_c"], b["raw_f"])),
                "coarse_weights": dict(debug_coarse_weights=b["w"]),
                "train_tables": dict(train={"t_rand": b["t_rand"], "noise_coarse": b["noise_c"], "noise_fine": b["noise_f"], "u": b["u"]})}[hook]

    def close(self):
        self.r.close()


def _disarm(r):
    """NULL pointers through the C setters (whatever the library under test does on its own)."""
    r._lib.nwe_debug_set_fine_depths(r._ctx, None)
    r._lib.nwe_debug_set_raw(r._ctx, None, None)
    r._lib.nwe_debug_set_coarse_weights(r._ctx, None)
    r._lib.nwe_set_train_tables(r._ctx, None, None, None, None)


@pytest.fixture(scope="module")
def hb():
    b = HookBench()
    yield b
    b.close()


def _plain_equals(hb, r, precision, ctx):
    got = r.render_rays(hb.rays, precision=precision, outputs=HOOK_OUT)
    assert_same(got, hb.plain[precision], HOOK_OUT, ctx)


def _hooked_differs(hb, got, precision, ctx):
    """The hook has an effect on these outputs, so a hook that stayed armed could not hide."""
    assert not bits_equal(got["rgb"], hb.plain[precision]["rgb"]), ctx


REFUSALS = ("struct_bytes", "feat_map_mfma", "unknown_precision", "null_rays", "no_mfma_kernel")


def _refused_call(hb, r, how):
    """One refused nwe_render_rays on context r (which holds hb's networks): exact code, a message."""
    if how == "struct_bytes":
        rc, _ = _raw_render_rays(r, hb.rays, "f16x3", HOOK_OUT, struct_bytes=8)
        _assert_refused(r, rc, L.NWE_ERR_INVALID, how)
    elif how == "feat_map_mfma":
        rc, _ = _raw_render_rays(r, hb.rays, "f16x3", HOOK_OUT + ("feat_map",))
        _assert_refused(r, rc, L.NWE_ERR_UNSUPPORTED, how)
    elif how == "unknown_precision":
        rc, _ = _raw_render_rays(r, hb.rays, 7, HOOK_OUT)
        _assert_refused(r, rc, L.NWE_ERR_INVALID, how)
    elif how == "null_rays":            # past check_ready: nwe_render_rays' own argument check
        rc, _ = _raw_render_rays(r, hb.rays, "f16x3", HOOK_OUT, null_rays=True)
        _assert_refused(r, rc, L.NWE_ERR_INVALID, how)
    else:
        raise AssertionError(how)


@pytest.mark.parametrize("how", REFUSALS)
@pytest.mark.parametrize("hook", HOOKS)
def test_refused_call_consumes_the_hook(hb, hook, how):
    """Arm, refused nwe_render_rays, plain call: the plain call equals the hook-free render of a fresh context."""
    if how == "no_mfma_kernel":         # a context of its own: 6x64 networks, an MFMA precision is refused, f32 renders
        r = nwe_amd.Renderer(0)
        try:
            r.set_network(0, _sd("generic", 11)); r.set_network(1, _sd("generic", 12)); r.set_sampling(HNS, HNI)
            want = r.render_rays(hb.rays, precision="f32", outputs=HOOK_OUT)         # nothing armed yet on this new context
            hb.arm(r, hook)
            rc, _ = _raw_render_rays(r, hb.rays, "f16x3", HOOK_OUT)
            _assert_refused(r, rc, L.NWE_ERR_UNSUPPORTED, how)
            got = r.render_rays(hb.rays, precision="f32", outputs=HOOK_OUT)
            assert_same(got, want, HOOK_OUT, (hook, how))
        finally:
            _disarm(r)
            r.close()
        return
    try:
        hb.arm(hb.r, hook)
        _refused_call(hb, hb.r, how)
        _plain_equals(hb, hb.r, "f16x3", (hook, how))
    finally:
        _disarm(hb.r)


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("hook", HOOKS)
def test_hooks_are_one_shot(hb, hook, precision):
    """Arm, render twice: the first render is hooked, the second equals the hook-free one."""
    try:
        hb.arm(hb.r, hook)
        first = hb.r.render_rays(hb.rays, precision=precision, outputs=HOOK_OUT)
        _hooked_differs(hb, first, precision, (hook, precision))
        _plain_equals(hb, hb.r, precision, (hook, precision))
    finally:
        _disarm(hb.r)


@pytest.mark.parametrize("hook", HOOKS)
def test_pinhole_render_leaves_the_hooks_alone(hb, hook):
    """include/nwe.h: nwe_render neither uses nor clears the hooks - the next nwe_render_rays takes them."""
    try:
        hb.arm(hb.r, hook)
        want = hb.r.render_rays(hb.rays, precision="f16x3", outputs=HOOK_OUT)       # hooked
        hb.arm(hb.r, hook)
        pin = hb.r.render(_pose(), 7, 19, precision="f16x3", outputs=LEAN, **_kw(7, 19))
        assert_same(pin, hb.plain_pinhole, LEAN, hook)                              # not used by nwe_render ...
        got = hb.r.render_rays(hb.rays, precision="f16x3", outputs=HOOK_OUT)
        assert_same(got, want, HOOKED_OUT, hook)                                    # ... and still armed for nwe_render_rays
        _hooked_differs(hb, got, "f16x3", hook)
        _plain_equals(hb, hb.r, "f16x3", hook)
    finally:
        _disarm(hb.r)


@pytest.mark.parametrize("hook", HOOKS)
def test_zero_rays_consume_the_hook(hb, hook):
    try:
        hb.arm(hb.r, hook)
        rc, _ = _raw_render_rays(hb.r, hb.rays[:0], "f16x3", ("rgb",))
        assert rc == L.NWE_OK
        _plain_equals(hb, hb.r, "f16x3", hook)
    finally:
        _disarm(hb.r)


@pytest.mark.parametrize("hook", HOOKS)
def test_wrapper_arms_nothing_it_does_not_render(hb, hook):
    """Renderer.render_rays: (a) a call the library refuses, (b) a ValueError of the wrapper's own validation part-way through its
    hook arguments - after each, a plain call equals the hook-free render; (c) through the wrapper too a hook holds once."""
    kw = hb.wrapper_kwargs(hook)
    try:
        with pytest.raises(NotImplementedError):
            hb.r.render_rays(hb.rays, precision="f16x3", outputs=HOOK_OUT + ("feat_map",), **kw)
        _plain_equals(hb, hb.r, "f16x3", (hook, "refused"))
        bad = dict(kw)
        if hook == "train_tables":
            bad["train"] = dict(kw["train"], u=hb.buf["u"][:, :3])            # t_rand, noise_* valid; u of the wrong shape
        else:
            bad["train"] = {"u": hb.buf["u"][:, :3]}                           # the debug argument valid, a later one wrong
        with pytest.raises(ValueError):
            hb.r.render_rays(hb.rays, precision="f16x3", outputs=HOOK_OUT, **bad)
        _plain_equals(hb, hb.r, "f16x3", (hook, "ValueError"))
        hooked = hb.r.render_rays(hb.rays, precision="f16x3", outputs=HOOK_OUT, **kw)
        _hooked_differs(hb, hooked, "f16x3", hook)
        _plain_equals(hb, hb.r, "f16x3", (hook, "one-shot"))
    finally:
        _disarm(hb.r)


def test_wrapper_value_error_part_way_arms_nothing(hb):
    """debug_fine_depths valid, debug_raw of the wrong shape: nothing may be armed afterwards.  Likewise for every other
    way the wrapper can raise after it has looked at debug_fine_depths."""
    z, b = hb.buf["z"], hb.buf
    bad_calls = (dict(debug_raw=(b["raw_c"], b["raw_f"][:, :5])), dict(debug_coarse_weights=b["w"][:, :5]), dict(train={"no_such_key": b["u"]}),
                 dict(outputs=HOOK_OUT + ("no_such_output",)), dict(precision="fp8"))
    try:
        for bad in bad_calls:
            with pytest.raises(ValueError):
                hb.r.render_rays(hb.rays, **{**dict(precision="f16x3", outputs=HOOK_OUT, debug_fine_depths=z), **bad})
            _plain_equals(hb, hb.r, "f16x3", sorted(bad))
    finally:
        _disarm(hb.r)


# ------------------------------------------------------------------------------------------------------------------------
# 3. timing calls
# ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def r_bench():
    """The bench networks at 64 + 128."""
    r = nwe_amd.Renderer(0)
    r.set_network(0, synthetic.make_state_dict(1000, 8, 256))
    r.set_network(1, synthetic.make_state_dict(1001, 8, 256))
    r.set_sampling(64, 128)
    yield r
    r.close()


def test_timing_calls_before_any_launch():
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, _sd("4x128", 300)); r.set_network(1, _sd("4x128", 301)); r.set_sampling(HNS, HNI)
        ms, rays = (C.c_float * 2)(), (C.c_int64 * 2)()

        def nothing_yet(ctx):
            assert r.last_kernel_ms() < 0, ctx
            assert r._lib.nwe_last_launch_parts(r._ctx, ms, rays) == L.NWE_ERR_STATE, ctx
            assert r._lib.nwe_last_error(r._ctx).decode() != "", ctx

        nothing_yet("new context")
        for _ in range(5):                                   # ray generation is not a render launch
            rays0 = r.create_rays(_pose(), 7, 19, **_kw(7, 19))
        nothing_yet("after create_rays")
        assert r.render_rays(rays0[:0], outputs=("rgb",))["rgb"].shape == (0, 3)
        nothing_yet("after zero rays")
        with pytest.raises(NotImplementedError):             # a refused call is no launch either
            r.render_rays(rays0, precision="f16x3", outputs=LEAN + ("feat_map",))
        nothing_yet("after a refused call")
        r.render_rays(rays0, outputs=LEAN)
        assert r.last_kernel_ms() > 0 and r.last_launch_parts()[0][1] == rays0.shape[0]
    finally:
        r.close()


def test_create_rays_leaves_the_timing_alone(r_bench):
    """Render, read both timing calls, five nwe_create_rays, read again: equal exactly (the same event pairs).  Under plan 2,
    so that a stale ev_mid would show as well."""
    r_bench.debug_set_decomposition(2)
    try:
        r_bench.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        assert r_bench.debug_last_plan() == 2
        ms, parts = r_bench.last_kernel_ms(), r_bench.last_launch_parts()
        assert len(parts) == 2
        for i in range(5):
            r_bench.create_rays(_pose(-10.0 * i), 48, 64, **_kw(48, 64))
        assert r_bench.last_kernel_ms() == ms
        assert r_bench.last_launch_parts() == parts
    finally:
        r_bench.debug_set_decomposition(-1)


@pytest.mark.parametrize("plan", [0, 1, 2])
def test_launch_parts_of_every_plan(r_bench, plan):
    """300 x 200 = 60000 rays: plan 2 splits into a packets launch over the full rounds and a sample-split rest
    (test_hybrid_launch_plan).  A kernel cannot take longer than the call that contains it plus its synchronisation."""
    n = 200 * 300
    r_bench.debug_set_decomposition(plan)
    try:
        r_bench.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))     # warm: code objects loaded, pose table allocated
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r_bench.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert r_bench.debug_last_plan() == plan
        ms, parts = r_bench.last_kernel_ms(), r_bench.last_launch_parts()
        print(f"plan {plan}: kernel {ms:.3f} ms, call + synchronise {wall_ms:.3f} ms, parts {parts}")
        assert 0 < ms <= wall_ms
        assert sum(p[1] for p in parts) == n
        assert (len(parts) == 2 and parts[1][1] > 0) if plan == 2 else len(parts) == 1
        for part_ms, part_rays in parts:
            assert 0 < part_ms <= ms and part_rays > 0
    finally:
        r_bench.debug_set_decomposition(-1)


def test_launch_refused_inside_launch_leaves_the_timing_alone():
    """A good launch, then launches refused after the argument checks (coarse 4x128, fine 8x256, an MFMA precision): the timing
    calls still describe the good launch, and the f32 kernel, which takes two shapes, renders what a fresh context renders."""
    r, f = nwe_amd.Renderer(0), nwe_amd.Renderer(0)
    try:
        for x in (r, f):
            x.set_network(1, _sd("8x256", 101)); x.set_sampling(HNS, HNI)
        r.set_network(0, _sd("8x256", 100))
        r.debug_set_decomposition(2)
        r.render(_pose(), 200, 300, outputs=LEAN, **_kw(200, 300))
        ms, parts = r.last_kernel_ms(), r.last_launch_parts()
        assert ms > 0 and len(parts) == 2
        r.debug_set_decomposition(-1)
        r.set_network(0, _sd("4x128", 300)); f.set_network(0, _sd("4x128", 300))
        for _ in range(5):                                   # more refusals than the ring has slots
            with pytest.raises(NotImplementedError, match="same shape"):
                r.render(_pose(), 7, 19, precision="f16x3", outputs=LEAN, **_kw(7, 19))
            assert r.last_kernel_ms() == ms and r.last_launch_parts() == parts
        got = r.render(_pose(), 7, 19, precision="f32", outputs=WALK_FULL, **_kw(7, 19))
        assert_same(got, f.render(_pose(), 7, 19, precision="f32", outputs=WALK_FULL, **_kw(7, 19)), WALK_FULL, "f32 after refusals")
        assert r.last_launch_parts()[0][1] == 7 * 19 and len(r.last_launch_parts()) == 1
    finally:
        r.close(); f.close()


def test_six_launches_on_six_streams(r_bench):
    """include/nwe.h: with more than four launches queued the call blocks until the oldest has finished.  Six renders with six
    poses on six streams of one context give what they give one after the other; twice, so that every slot is reused."""
    yaws = (0.0, -25.0, -50.0, -75.0, -100.0, -125.0)
    kw = dict(outputs=LEAN, **_kw(96, 128))
    want = [{k: v.clone() for k, v in r_bench.render(_pose(y), 96, 128, **kw).items()} for y in yaws]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in yaws]
    for _ in range(2):
        got = []
        for y, st in zip(yaws, streams):
            with torch.cuda.stream(st):
                got.append(r_bench.render(_pose(y), 96, 128, **kw))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same(a, b, LEAN, i)
        assert sum(p[1] for p in r_bench.last_launch_parts()) == 96 * 128


# ------------------------------------------------------------------------------------------------------------------------
# 4. reconfiguring under a launch in flight
# ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_frame():
    """The 800 x 800 benchmark frame (many rounds of workgroups) of a fresh context at 64 + 128."""
    r = nwe_amd.Renderer(0)
    r.set_network(0, synthetic.make_state_dict(1000, 8, 256))
    r.set_network(1, synthetic.make_state_dict(1001, 8, 256))
    r.set_sampling(64, 128)
    out = r.render(_pose(), 800, 800, outputs=LEAN, **_kw(800, 800))
    torch.cuda.synchronize()
    r.close()
    return out


@pytest.mark.parametrize("what", ["set_sampling", "set_network", "set_white_background"])
def test_reconfigure_under_a_launch_in_flight(big_frame, what):
    """Queue the frame on a side stream and reconfigure at once, without synchronising: the frame is the one of the settings it
    was launched with (nwe_set_sampling / nwe_set_network wait for the context's launches; the white-background switch is host
    state copied at launch).  The next frame has the new settings.  Once each; nothing here is repeated to provoke anything."""
    r = nwe_amd.Renderer(0)
    f = nwe_amd.Renderer(0)
    try:
        for x in (r, f):
            x.set_network(0, synthetic.make_state_dict(1000, 8, 256))
            x.set_network(1, synthetic.make_state_dict(1001, 8, 256))
            x.set_sampling(64, 128)
        r.render(_pose(), 16, 16, outputs=LEAN, **_kw(16, 16))          # warm: code objects, pose table
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = r.render(_pose(), 800, 800, outputs=LEAN, **_kw(800, 800))
        for x in (r, f):
            if what == "set_sampling":
                x.set_sampling(24, 40)
            elif what == "set_network":
                x.set_network(0, _sd("4x128", 300)); x.set_network(1, _sd("4x128", 301))
            else:
                x.set_white_background(True)
        torch.cuda.synchronize()
        assert_same(got, big_frame, LEAN, what)
        after = r.render(_pose(), 13, 29, outputs=LEAN, **_kw(13, 29))
        assert_same(after, f.render(_pose(), 13, 29, outputs=LEAN, **_kw(13, 29)), LEAN, (what, "next frame"))
    finally:
        torch.cuda.synchronize()
        r.close(); f.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. white background
# ------------------------------------------------------------------------------------------------------------------------

WHITE_SHAPES = {"8x256": dict(D=8, W=256), "6x256": dict(D=6, W=256), "8x256-no_view_dirs": dict(D=8, W=256, use_view_dirs=False)}
FULL_C = FULL + ("acc_coarse",)


def _white_case(r, call, ctx):
    """call(outputs) renders on r.  White off and on, lean and full: lean == full; rgb_on == rgb_off + (1 - acc_off) in fp32, coarse
    and fine alike; depth, acc and the flags are those of the frame without the option."""
    r.set_white_background(False)
    off_lean, off_full = call(LEAN), call(FULL_C)
    r.set_white_background(True)
    try:
        on_lean, on_full = call(LEAN), call(FULL_C)
    finally:
        r.set_white_background(False)
    _assert_lean_equals_full(off_lean, off_full, ctx)
    _assert_lean_equals_full(on_lean, on_full, ctx)
    for on, off in ((on_lean, off_lean), (on_full, off_full)):
        assert bits_equal(on["rgb"], off["rgb"] + (1.0 - off["acc"])[..., None]), ctx
        assert bits_equal(on["depth"], off["depth"]) and bits_equal(on["acc"], off["acc"]), ctx
        assert int(on["flags"].item()) == int(off["flags"].item()), ctx
    assert bits_equal(on_full["rgb_coarse"], off_full["rgb_coarse"] + (1.0 - off_full["acc_coarse"])[..., None]), ctx
    assert bits_equal(on_full["acc_coarse"], off_full["acc_coarse"]), ctx
    assert float((on_lean["rgb"] - off_lean["rgb"]).abs().max()) > 0.0, ctx      # the option does something on this frame


@pytest.mark.parametrize("ni", [0, 17])
@pytest.mark.parametrize("shape", list(WHITE_SHAPES))
def test_white_background_lean_full_every_mode(shape, ni):
    """render and render_rays; f16x3 and f16x1 under decompositions 0, 1, 2 and the f32 kernel; 13 x 29 = 377 rays."""
    kind = WHITE_SHAPES[shape]
    r = nwe_amd.Renderer(0)
    try:
        r.set_network(0, synthetic.make_state_dict(2000, **kind))
        r.set_network(1, synthetic.make_state_dict(2001, **kind))
        r.set_sampling(37, ni)
        rays = r.create_rays(_pose(), 13, 29, use_view_dirs=kind.get("use_view_dirs", True), **_kw(13, 29))
        for precision, mode in [(p, m) for p in ("f16x3", "f16x1") for m in (0, 1, 2)] + [("f32", -1)]:
            r.debug_set_decomposition(mode)
            _white_case(r, lambda outs: r.render(_pose(), 13, 29, precision=precision, outputs=outs, **_kw(13, 29)), (shape, ni, precision, mode, "render"))
            _white_case(r, lambda outs: r.render_rays(rays, precision=precision, outputs=outs), (shape, ni, precision, mode, "render_rays"))
    finally:
        r.close()


@pytest.mark.parametrize("ni", [0, 17])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_white_background_two_tiles_on_one_device(precision, ni):
    """nwe_render_tiled, two contexts on one device: the tiled frame with the option on is the single context's, bit for bit."""
    t = nwe_amd.TiledRenderer([0, 0])
    try:
        t.set_network(0, synthetic.make_state_dict(2000, 8, 256))
        t.set_network(1, synthetic.make_state_dict(2001, 8, 256))
        t.set_sampling(37, ni)
        kw = dict(precision=precision, outputs=LEAN, **_kw(13, 29))
        off = t.render(_pose(), 13, 29, **kw)
        assert t.last_tiled
        t.set_white_background(True)
        on = t.render(_pose(), 13, 29, **kw)
        assert t.last_tiled
        single = t.parts[0].render(_pose(), 13, 29, **kw)
        torch.cuda.synchronize()
        assert_same(on, single, LEAN, (precision, ni))
        assert bits_equal(on["rgb"], off["rgb"] + (1.0 - off["acc"])[..., None])
        assert bits_equal(on["depth"], off["depth"]) and bits_equal(on["acc"], off["acc"])
        assert int(on["flags"].item()) == int(off["flags"].item())
    finally:
        t.close()


def test_white_background_against_fp64():
    """The fog scene of test_gpu_accuracy.test_fog_scene_end_to_end_against_fp64 (2048 rays, thin-fog 8x256, 64 + 128) with the option on,
    lean frames, under the criterion of tests/accuracy.py with that test's K32 = 1.5 (measured 1.07 without the
    option): the f32 kernel against the fp32 oracle at K32, f16x3 at FACTOR against the larger of the two fp32 paths."""
    from tests.test_gpu_accuracy import _renderer, _scene_rays, _t
    rays = _scene_rays(2048)
    sd_c, sd_f = synthetic.thin_fog(synthetic.make_state_dict(1000, 8, 256)), synthetic.make_state_dict(1001, 8, 256)
    cfg = O.RenderConfig(n_samples=64, n_importance=128, white_bkgd=True)
    ref32 = A.per_ray_outputs(O.render_rays(rays, _t(sd_c), _t(sd_f), cfg), True)
    res64 = O.render_rays(rays, _t(sd_c), _t(sd_f), cfg, dtype=torch.float64)
    ref64 = A.per_ray_outputs(res64, True)
    keep = res64["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    try:
        r.set_white_background(True)
        kf = r.render_rays(rays.cuda(), precision="f32", outputs=LEAN)
        A.e2e_report(rep, "white fog f32 lean", kf, ref32, ref64, FAR, keep=keep, keys=LEAN, factor=1.5)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            got = r.render_rays(rays.cuda(), precision="f16x3", outputs=LEAN)
            A.e2e_report(rep, f"white fog f16x3 d{mode} lean", got, ref32, ref64, FAR, keep=keep, keys=LEAN, alt=kf, alt_cap=1.5)
    finally:
        r.close()
    rep.check()
