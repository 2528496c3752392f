"""The calls whose refusals are recorded in tests/golden/refusal_table.npz, enumerated once for the recorder (tools/record_refusals.py,
run on a library built from an earlier commit) and for the replay (tests/test_refusals_host.py, run on the tree under test).  Every call
is made on a host-only context, so nothing here needs a GPU.  walk() yields (case, code, text) in a fixed order; a case is a
tuple of plain values that says what was called.

Through nwe_debug_plan, which refuses what nwe_render and nwe_render_rays refuse, the full product of
    network pairs x sampling x modes x precisions x outputs x call form and ray count,
and beside it the direct refusals of the setters, of the two grids' boxes and of the render calls on a context without a device."""
import ctypes as C
import itertools

import numpy as np

import nwe_amd
from nwe_amd import _lib, synthetic

BOX_LO, BOX_HI, BOX_RES = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (2, 3, 4)

# ---- the domain of nwe_debug_plan ----

# name -> (coarse, fine); a network is (fold, make_state_dict arguments) or None for "not set"
_FOLDED = (True, dict(D=4, W=128))
_UNFOLDED = (False, dict(D=4, W=128))
_NO_DIRS = (True, dict(D=4, W=128, use_view_dirs=False))
_W64 = (True, dict(D=4, W=64))
_BIG = (True, dict(D=8, W=256))
NET_PAIRS = {
    "folded": (_FOLDED, _FOLDED),
    "unfolded": (_UNFOLDED, _UNFOLDED),
    "folded+unfolded": (_FOLDED, _UNFOLDED),
    "no_dirs": (_NO_DIRS, _NO_DIRS),
    "dirs+no_dirs": (_FOLDED, _NO_DIRS),
    "w64": (_W64, _W64),
    "w64+folded": (_W64, _FOLDED),
    "fine_unset": (_FOLDED, None),
    "4x128+8x256": (_FOLDED, _BIG),
}
# beside the product, under the plain modes only: what the pairs above do not reach
EXTRA_NET_PAIRS = {
    "none": (None, None),                                                  # "coarse network not set"
    "other_encoding": (_FOLDED, (True, dict(D=4, W=128, in_xyz=39))),      # "... must share their encodings"
}
SAMPLINGS = ((8, 0), (8, 8), None)                       # (n_samples, n_importance); None: nwe_set_sampling was never called
# share_k, min_transmittance, separate passes, occupancy grid, coarse grid, stamps
MODES = tuple(itertools.product((1, 2), (0.0, 0.25), (0, 1), (0, 1), (0, 1), (0, 1)))
PLAIN = (1, 0.0, 0, 0, 0, 0)
PRECISIONS = (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32, 7)
OUTPUTS = ("lean", "z_fine", "feat_map", "flags", "struct_bytes")
# (form, ray count): pinhole frames of 0, 8 and 2^31 rays, ray lists of as many, bare and with each hook bit
FORMS = ("pinhole", "rays", "rays+weights_hook", "rays+other_hook")
COUNTS = (0, 8, 1 << 31)
_PINHOLE = {0: (1, 1, 8, 0, 0), 8: (1, 1, 8, 0, 1), 1 << 31: (2, 1 << 15, 1 << 15, 0, 1 << 15)}   # n_poses, H, W, row_begin, row_end
_HOOKS = {"rays": 0, "rays+weights_hook": _lib.PLAN_HOOK_COARSE_WEIGHTS, "rays+other_hook": _lib.PLAN_HOOK_OTHER}


def _outputs(name):
    lean = dict(rgb=1, depth=1, acc=1, flags=1)
    o = {"lean": lean, "z_fine": dict(lean, z_fine=1), "feat_map": dict(lean, feat_map=1), "flags": dict(flags=1), "struct_bytes": lean}[name]
    out = _lib.Outputs(**o)
    if name == "struct_bytes":
        out.struct_bytes -= 8
    return out


class _Calls:
    """The library, with handles of this walk's own that take pointers as numbers (as tests/test_plan_host.py's walk does)."""

    def __init__(self):
        self.lib = _lib.load()
        self.plan = self.lib["nwe_debug_plan"]
        self.plan.restype, self.plan.argtypes = C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_int64, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_void_p]
        self.report = _lib.PlanReport()
        self.outputs = {k: _outputs(k) for k in OUTPUTS}
        self.out_at = {k: C.addressof(v) for k, v in self.outputs.items()}

    def error(self, ctx):
        return self.lib.nwe_last_error(ctx).decode()

    def result(self, ctx, rc):
        return rc, (self.error(ctx) if rc else "")


def _context(pair, sampling):
    r = nwe_amd.Renderer(host_only=True)
    for which, net in enumerate(pair):
        if net is not None:
            r.debug_set_fold(net[0])
            r.set_network(which, synthetic.make_state_dict(1000 + which, **net[1]))
    if sampling is not None:
        r.set_sampling(*sampling)
    return r


_STAMPS = C.c_uint64(0)   # an armed stamp buffer: a host-only context never writes it


def _set_modes(calls, r, modes):
    """The grids after the networks: nwe_set_network clears them."""
    share_k, min_trans, separate, occ, cgrid, stamps = modes
    r.set_shared_coarse(share_k); r.set_early_termination(min_trans); r.set_separate_passes(bool(separate))
    if occ:
        r.set_occupancy(np.ones(BOX_RES, dtype=bool), BOX_LO, BOX_HI, BOX_RES)
    else:
        r.clear_occupancy()
    if cgrid:
        r.set_coarse_grid(np.ones(BOX_RES, dtype=np.float32), BOX_LO, BOX_HI)
    else:
        r.clear_coarse_grid()
    assert calls.lib.nwe_debug_set_stamps(r._ctx, C.addressof(_STAMPS) if stamps else None) == 0


def _plan_calls():
    """What one context state is asked: (key, arguments of nwe_debug_plan behind the context)."""
    for precision, out, form, count in itertools.product(PRECISIONS, OUTPUTS, FORMS, COUNTS):
        if form == "pinhole":
            n_poses, H, W, row_begin, row_end = _PINHOLE[count]
            yield (precision, out, form, count), (n_poses, H, W, row_begin, row_end, -1, out, 0, precision, 256)
        else:
            yield (precision, out, form, count), (1, 1, 1, 0, 1, count, out, _HOOKS[form], precision, 256)


def _walk_plans(calls):
    asked = list(_plan_calls())
    pairs = [(name, pair, SAMPLINGS, MODES) for name, pair in NET_PAIRS.items()] + \
            [(name, pair, SAMPLINGS[1:2], (PLAIN,)) for name, pair in EXTRA_NET_PAIRS.items()]
    report = C.addressof(calls.report)
    for name, pair, samplings, mode_sets in pairs:
        for sampling in samplings:
            r = _context(pair, sampling)
            try:
                for modes in mode_sets:
                    _set_modes(calls, r, modes)
                    ctx = r._ctx
                    for key, (n_poses, H, W, rb, re, n_rays, out, hooks, precision, cus) in asked:
                        rc = calls.plan(ctx, n_poses, H, W, rb, re, n_rays, calls.out_at[out], hooks, precision, cus, report)
                        yield ("plan", name, sampling, modes) + key, rc, (calls.error(ctx) if rc else "")
                # what nwe_debug_plan refuses beside the product: no outputs, a bad row range, no CUs, a report of another size
                _set_modes(calls, r, PLAIN)
                lean = calls.out_at["lean"]
                for what, args in (("null_outputs", (1, 1, 8, 0, 1, -1, None, 0, 0, 256, report)),
                                   ("bad_row_range", (1, 4, 8, 3, 2, -1, lean, 0, 0, 256, report)),
                                   ("rows_past_the_image", (1, 4, 8, 0, 5, -1, lean, 0, 0, 256, report)),
                                   ("no_poses", (0, 4, 8, 0, 4, -1, lean, 0, 0, 256, report)),
                                   ("cus_0", (1, 1, 8, 0, 1, -1, lean, 0, 0, 0, report)),
                                   ("null_report", (1, 1, 8, 0, 1, -1, lean, 0, 0, 256, None))):
                    yield ("plan", name, sampling, what), *calls.result(r._ctx, calls.plan(r._ctx, *args))
            finally:
                r.close()


# ---- the direct refusals ----

def _layers(depth, width, in_xyz, in_dir, out_ch=5):
    """Small constant weights and zero biases in the layer order of nwe_set_network (in_dir > 0) or nwe_set_network_no_view_dirs."""
    depth, width = max(depth, 1), max(width, 2)
    shapes = [(width, in_xyz)] + [(width, width)] * (depth - 1)
    shapes += [(width // 2, width + in_dir), (width, width), (1, width), (3, width // 2)] if in_dir else [(out_ch, width)]
    w = [np.full((o, max(i, 1)), 0.01, dtype=np.float32) for o, i in shapes]
    b = [np.zeros(o, dtype=np.float32) for o, _ in shapes]
    return w, b


def _pointers(arrays, null_at=None):
    return (C.c_void_p * len(arrays))(*[None if i == null_at else a.ctypes.data for i, a in enumerate(arrays)])


def _walk_setters(calls):
    lib = calls.lib
    r = nwe_amd.Renderer(host_only=True)
    ctx = r._ctx
    try:
        # nwe_set_network: which, depth, width, in_xyz, in_dir, then what is null
        for which, depth, width, in_xyz, in_dir, null in (
                (0, 4, 128, 63, 27, None), (0, 4, 128, 63, 27, "w"), (0, 4, 128, 63, 27, "b"), (2, 4, 128, 63, 27, None), (-1, 4, 128, 63, 27, None),
                (0, 0, 128, 63, 27, None), (0, 17, 128, 63, 27, None), (0, 4, 0, 63, 27, None), (0, 4, 258, 63, 27, None), (0, 4, 127, 63, 27, None),
                (0, 4, 128, 0, 27, None), (0, 4, 128, 64, 27, None), (0, 4, 128, 99, 27, None), (0, 4, 128, 63, 0, None), (0, 4, 128, 63, 28, None),
                (0, 4, 128, 63, 69, None), (1, 4, 128, 63, 27, 0), (1, 4, 128, 63, 27, 7), (1, 4, 128, 63, 27, -7)):
            w, b = _layers(depth, width, max(in_xyz, 3), max(in_dir, 3))
            wp = None if null == "w" else _pointers(w, null if isinstance(null, int) and null >= 0 else None)
            bp = None if null == "b" else _pointers(b, -null if isinstance(null, int) and null < 0 else None)
            rc = lib.nwe_set_network(ctx, which, depth, width, in_xyz, in_dir, -1, wp, bp)
            yield ("nwe_set_network", which, depth, width, in_xyz, in_dir, null), *calls.result(ctx, rc)
        # nwe_set_network_no_view_dirs: which, depth, width, in_xyz, output_ch, then what is null
        for which, depth, width, in_xyz, out_ch, null in (
                (0, 4, 128, 63, 5, None), (0, 4, 128, 63, 5, "w"), (3, 4, 128, 63, 5, None), (0, 0, 128, 63, 5, None),
                (0, 4, 258, 63, 5, None), (0, 4, 128, 62, 5, None), (0, 4, 128, 99, 5, None), (0, 4, 128, 63, 3, None), (0, 4, 128, 63, 257, None),
                (1, 4, 128, 63, 5, 4), (1, 4, 128, 63, 5, -2)):
            w, b = _layers(depth, width, max(in_xyz, 3), 0, min(max(out_ch, 1), 256))
            wp = None if null == "w" else _pointers(w, null if isinstance(null, int) and null >= 0 else None)
            bp = _pointers(b, -null if isinstance(null, int) and null < 0 else None)
            rc = lib.nwe_set_network_no_view_dirs(ctx, which, depth, width, in_xyz, -1, out_ch, wp, bp)
            yield ("nwe_set_network_no_view_dirs", which, depth, width, in_xyz, out_ch, null), *calls.result(ctx, rc)
        # nwe_set_sampling: n_samples, n_importance, then which table is null
        t = np.linspace(0.0, 1.0, 129, dtype=np.float32)
        for ns, ni, null in ((8, 8, None), (8, 0, "u"), (8, 8, "t"), (8, 8, "omt"), (1, 0, None), (129, 0, None), (8, -1, None), (8, 257, None),
                             (8, 8, "u"), (2, 8, None), (2, 0, None), (128, 256, None)):
            at = {k: (None if null == k else t.ctypes.data) for k in ("t", "omt", "u")}
            rc = lib.nwe_set_sampling(ctx, at["t"], at["omt"], ns, at["u"], ni)
            yield ("nwe_set_sampling", ns, ni, null), *calls.result(ctx, rc)
        # the three mode setters
        for eps in (0.0, 0.25, -0.1, 1.0, 1.5, float("nan")):
            yield ("nwe_set_early_termination", repr(eps)), *calls.result(ctx, lib.nwe_set_early_termination(ctx, eps))
        for k in (1, 16, 0, 17, -3):
            yield ("nwe_set_shared_coarse", k), *calls.result(ctx, lib.nwe_set_shared_coarse(ctx, k))
        for on in (0, 1, 2, -1):
            yield ("nwe_set_separate_passes", on), *calls.result(ctx, lib.nwe_set_separate_passes(ctx, on))
    finally:
        r.close()


def _walk_boxes(calls):
    """nwe_set_occupancy and nwe_set_coarse_grid over the same boxes: the coarse grid's maximum is 512 per axis, the occupancy grid's
    1024, and only the coarse grid asks that the fp32 resolution / (hi - lo) be finite."""
    lib = calls.lib
    nan, inf, tiny = float("nan"), float("inf"), 1e-45
    boxes = (("ok", (-1, -1, -1), (1, 1, 1), (2, 3, 4)), ("null_lo", None, (1, 1, 1), (2, 3, 4)), ("null_hi", (-1, -1, -1), None, (2, 3, 4)),
             ("null_res", (-1, -1, -1), (1, 1, 1), None), ("nan_lo", (-1, nan, -1), (1, 1, 1), (2, 3, 4)), ("nan_hi", (-1, -1, -1), (1, 1, nan), (2, 3, 4)),
             ("inf_hi", (-1, -1, -1), (inf, 1, 1), (2, 3, 4)), ("infinite_extent", (-3e38, -1, -1), (3e38, 1, 1), (2, 3, 4)),
             ("lo_equals_hi", (-1, 1, -1), (1, 1, 1), (2, 3, 4)), ("lo_above_hi", (-1, -1, 2), (1, 1, 1), (2, 3, 4)),
             ("res_0", (-1, -1, -1), (1, 1, 1), (2, 0, 4)), ("res_negative", (-1, -1, -1), (1, 1, 1), (2, 3, -4)),
             ("res_512", (-1, -1, -1), (1, 1, 1), (512, 1, 1)), ("res_513", (-1, -1, -1), (1, 1, 1), (1, 513, 1)),
             ("res_1024", (-1, -1, -1), (1, 1, 1), (1, 1, 1024)), ("res_1025", (-1, -1, -1), (1, 1, 1), (1025, 1, 1)),
             ("thin", (0, 0, 0), (1, tiny, 1), (2, 3, 4)))
    F3, I3 = C.c_float * 3, C.c_int * 3
    values = np.ones(1024, dtype=np.float32)
    for setter in ("nwe_set_occupancy", "nwe_set_coarse_grid"):
        r = nwe_amd.Renderer(host_only=True)
        try:
            call = getattr(lib, setter)
            for name, lo, hi, res in boxes:
                args = [F3(*lo) if lo else None, F3(*hi) if hi else None, I3(*res) if res else None]
                yield (setter, name), *calls.result(r._ctx, call(r._ctx, *args, values.ctypes.data, 0))
            ok = [F3(-1, -1, -1), F3(1, 1, 1), I3(2, 3, 4)]
            yield (setter, "null_values"), *calls.result(r._ctx, call(r._ctx, *ok, None, 0))
            yield (setter, "values_on_device"), *calls.result(r._ctx, call(r._ctx, *ok, values.ctypes.data, 1))
        finally:
            r.close()


def _walk_host_only_renders(calls):
    """nwe_render and nwe_render_rays on a context without a device: check_ready's refusal of it, behind the two in front."""
    lib = calls.lib
    pose = np.eye(4, dtype=np.float32)
    for state in ("ready", "bare"):
        r = _context(NET_PAIRS["folded"], (8, 8)) if state == "ready" else nwe_amd.Renderer(host_only=True)
        try:
            for out in ("lean", "struct_bytes", None):
                o = C.byref(calls.outputs[out]) if out else None
                rc = lib.nwe_render(r._ctx, pose.ctypes.data, 1, 1, 8, 1.0, 1.0, 0.0, 0.0, 0.1, 1.0, 0, 1, 0, o, None)
                yield ("nwe_render", state, out), *calls.result(r._ctx, rc)
                rc = lib.nwe_render_rays(r._ctx, None, 0, 0, o, None)
                yield ("nwe_render_rays", state, out), *calls.result(r._ctx, rc)
        finally:
            r.close()


def walk():
    """(case, code, text) of every call of the domain, in its fixed order; text is "" where the call was not refused."""
    calls = _Calls()
    yield from _walk_plans(calls)
    yield from _walk_setters(calls)
    yield from _walk_boxes(calls)
    yield from _walk_host_only_renders(calls)
