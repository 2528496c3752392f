"""The occupancy grid without a GPU (include/nwe.h: nwe_set_occupancy): set / get / clear / copy and every refusal on a host-only
context, what set_network does to a grid, the planner's fifth variant and the refusals of the excluded combinations, the
helper's cell rule on hand-made points, and the validity of the parity scenes (tests/occupancy.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib, synthetic
from tests import occupancy as G

F3, I3 = C.c_float * 3, C.c_int * 3


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _outputs(*names):
    o = _lib.Outputs()
    for n in names:
        setattr(o, n, 8)   # only null / non-null is read
    return o


def _plan(r, n_rays, outputs=("rgb",), pinhole=True, hooks=0, precision=_lib.PREC_F16X3, cus=256):
    report = _lib.PlanReport()
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, 1, n_rays, 0, 1, -1 if pinhole else n_rays, C.byref(_outputs(*outputs)), hooks, precision, cus,
                                    C.byref(report))
    return rc, report


def _host(ns=8, ni=8, D=4, W=128, **kw):
    r = nwe_amd.Renderer(host_only=True)
    r.set_network(0, synthetic.make_state_dict(1000, D=D, W=W, **kw))
    r.set_network(1, synthetic.make_state_dict(1001, D=D, W=W, **kw))
    r.set_sampling(ns, ni)
    return r


def test_set_get_clear_copy_on_a_host_only_context():
    """(5, 7, 9): 315 cells, no multiple of 32 - the bits behind the last cell come back as 0."""
    lib = _lib.load()
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert r.occupancy is None and r.occupancy_bits() is None
        assert lib.nwe_get_occupancy(r._ctx, None, None, None, None, None) == _lib.NWE_ERR_STATE
        assert lib.nwe_occupancy_copy(r._ctx, None, 10) == _lib.NWE_ERR_STATE
        rng = np.random.default_rng(5)
        bits = rng.random((5, 7, 9)) > 0.5
        lo, hi = (-1.0, 0.5, 2.0), (1.5, 4.0, 2.25)
        r.set_occupancy(bits, lo, hi, (5, 7, 9))
        g = r.occupancy
        assert g["resolution"] == (5, 7, 9) and g["lo"] == lo and g["hi"] == hi
        assert g["occupied_cells"] == int(bits.sum()) and g["occupied"] == bits.sum() / 315
        expect = np.array([5, 7, 9], np.float32) / (np.array(hi, np.float32) - np.array(lo, np.float32))
        assert g["inv"].dtype == np.float32 and (g["inv"] == expect).all()
        assert (r.occupancy_bits() == bits).all()
        # packed words, all ones: the ten words carry 320 bits, 315 are cells
        ones = np.full(10, 0xFFFFFFFF, np.uint32)
        r.set_occupancy(ones, lo, hi, (5, 7, 9))
        assert r.occupancy["occupied_cells"] == 315
        words = np.empty(10, np.uint32)
        assert lib.nwe_occupancy_copy(r._ctx, words.ctypes.data, 10) == _lib.NWE_OK
        assert (words[:9] == 0xFFFFFFFF).all() and words[9] == (1 << (315 - 288)) - 1
        assert lib.nwe_occupancy_copy(r._ctx, words.ctypes.data, 9) == _lib.NWE_ERR_INVALID
        # the layout: bit (ix ry + iy) rz + iz
        one = np.zeros((5, 7, 9), bool); one[3, 2, 4] = True
        r.set_occupancy(one, lo, hi, (5, 7, 9))
        assert lib.nwe_occupancy_copy(r._ctx, words.ctypes.data, 10) == _lib.NWE_OK
        cell = (3 * 7 + 2) * 9 + 4
        assert words[cell >> 5] == 1 << (cell & 31) and words.astype(bool).sum() == 1
        # a torch bool tensor, a scalar resolution
        r.set_occupancy(torch.ones(4, 4, 4, dtype=torch.bool), lo, hi, 4)
        assert r.occupancy["resolution"] == (4, 4, 4) and r.occupancy["occupied"] == 1.0
        r.clear_occupancy()
        assert r.occupancy is None
        r.clear_occupancy()                       # clearing nothing is fine
        assert lib.nwe_clear_occupancy(None) == _lib.NWE_ERR_INVALID and lib.nwe_get_occupancy(None, None, None, None, None, None) == _lib.NWE_ERR_INVALID
    finally:
        r.close()


def test_every_refusal_of_the_setter_by_message():
    lib = _lib.load()
    r = nwe_amd.Renderer(host_only=True)
    try:
        good = np.ones((2, 2, 2), bool)
        r.set_occupancy(good, (0, 0, 0), (1, 1, 1), 2)
        words = np.ones(1, np.uint32)
        lo, hi, res = F3(0, 0, 0), F3(1, 1, 1), I3(2, 2, 2)
        for args, text in (((None, hi, res, words.ctypes.data), "null lo, hi or resolution"), ((lo, None, res, words.ctypes.data), "null lo, hi or resolution"),
                           ((lo, hi, None, words.ctypes.data), "null lo, hi or resolution"), ((lo, hi, res, None), "null bits")):
            assert lib.nwe_set_occupancy(r._ctx, *args, 0) == _lib.NWE_ERR_INVALID and text in _error(r)
        assert lib.nwe_set_occupancy(r._ctx, lo, hi, res, words.ctypes.data, 1) == _lib.NWE_ERR_INVALID and "host-only" in _error(r)
        inf, nan = float("inf"), float("nan")
        for lo_, hi_, text in (((0, 0, 0), (1, nan, 1), "must be finite"), ((0, -inf, 0), (1, 1, 1), "must be finite"), ((0, 0, 0), (1, 1, inf), "must be finite"),
                               ((-3e38, 0, 0), (3e38, 1, 1), "must be finite"),     # the extent overflows fp32
                               ((0, 0, 0), (1, 0, 1), "lo < hi"), ((0, 2, 0), (1, 1, 1), "lo < hi")):
            with pytest.raises(ValueError, match=text):
                r.set_occupancy(good, lo_, hi_, 2)
        for res_ in ((0, 2, 2), (2, 2, 1025), (2, -1, 2)):
            assert lib.nwe_set_occupancy(r._ctx, lo, hi, I3(*res_), words.ctypes.data, 0) == _lib.NWE_ERR_INVALID and "1..1024" in _error(r)
        with pytest.raises(ValueError, match="shape"):
            r.set_occupancy(np.ones((2, 2, 3), bool), (0, 0, 0), (1, 1, 1), 2)
        with pytest.raises(ValueError, match="words"):
            r.set_occupancy(np.ones(2, np.uint32), (0, 0, 0), (1, 1, 1), 2)
        # a refused call leaves the grid that was set
        assert r.occupancy["resolution"] == (2, 2, 2) and r.occupancy["occupied_cells"] == 8
        # the largest legal grid's word count is what the ABI asks for: 1024^3 cells are fewer than 2^31
        for bad in ((0, 1), (5, 1), (1, -1), (1, 3)):
            with pytest.raises((ValueError, RuntimeError)):
                r.build_occupancy((0, 0, 0), (1, 1, 1), 2, probes=bad[0], dilate=bad[1])   # a host-only context builds nothing
    finally:
        r.close()


def test_set_network_clears_the_grid_and_a_refused_one_does_not():
    r = _host()
    try:
        bits = np.ones((2, 2, 2), bool)
        for setter in (lambda: r.set_network(1, synthetic.make_state_dict(7, D=4, W=128)),
                       lambda: r.set_network(0, synthetic.make_state_dict(7, D=4, W=128, use_view_dirs=False))):
            r.set_occupancy(bits, (0, 0, 0), (1, 1, 1), 2)
            setter()
            assert r.occupancy is None
        r.set_occupancy(bits, (0, 0, 0), (1, 1, 1), 2)
        with pytest.raises(NotImplementedError):
            r.set_network(0, synthetic.make_state_dict(7, D=17, W=128, skips=()))        # depth outside 1..16
        sd = synthetic.make_state_dict(7, D=4, W=128)
        ws = (C.c_void_p * 8)(*[None] * 8)
        assert _lib.load().nwe_set_network(r._ctx, 2, 4, 128, 63, 27, -1, ws, ws) == _lib.NWE_ERR_INVALID   # which
        assert r.occupancy is not None and r.occupancy["occupied_cells"] == 8
        del sd
        r.set_sampling(16, 0)                     # sampling does not touch it
        assert r.occupancy is not None
    finally:
        r.close()


def test_the_plan_reports_the_occupancy_variant_and_the_refusals():
    """A lean call while a grid is set: variant 3, never queued, no tail, the evaluation counter; every excluded combination
    and output is refused with NWE_ERR_UNSUPPORTED and a message that names the setting - without a device."""
    r = _host(ns=64, ni=128)
    try:
        rc, plain = _plan(r, 800 * 800)
        assert rc == 0 and plain.main.variant == 0 and plain.may_queue == 1 and plain.need_evals == 0
        r.set_occupancy(np.ones((4, 4, 4), bool), (0, 0, 0), (1, 1, 1), 4)
        for n_rays in (133, 40000, 800 * 800):
            for dec in (-1, 0, 1, 2):
                r.debug_set_decomposition(dec)
                rc, rep = _plan(r, n_rays)
                assert rc == 0, _error(r)
                assert rep.main.variant == 3 and rep.may_queue == 0 and rep.need_side == 0 and rep.need_evals == 1
                assert rep.main.tail == 0 and rep.main.fork == 0 and list(rep.main.grid) == [0, 0]
                assert rep.coarse_launch == 0 and rep.main.role == 0
                assert rep.main.rays[0] + rep.main.rays[1] == n_rays
        r.debug_set_decomposition(-1)
        r.debug_set_work_queue(1)
        assert _plan(r, 40000)[1].may_queue == 0
        r.debug_set_work_queue(-1)
        assert _plan(r, 133, precision=_lib.PREC_F32)[0] == 0 and _plan(r, 133, precision=_lib.PREC_F16X1)[1].main.variant == 3
        named = "an occupancy grid is set (nwe_set_occupancy, 4 x 4 x 4)"
        for out in ("disp", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse", "disp_coarse", "raw_coarse", "raw_fine", "z_fine",
                    "weights_coarse", "sample_cond", "sample_amp", "sample_switch"):
            for prec in (_lib.PREC_F16X3, _lib.PREC_F32):
                rc, _ = _plan(r, 133, outputs=("rgb", out), precision=prec)
                assert rc == _lib.NWE_ERR_UNSUPPORTED and named in _error(r) and "only rgb / depth / acc / flags" in _error(r), (out, _error(r))
        for hooks in (0, _lib.PLAN_HOOK_COARSE_WEIGHTS, _lib.PLAN_HOOK_OTHER):
            for prec in (_lib.PREC_F16X3, _lib.PREC_F32):
                rc, _ = _plan(r, 133, pinhole=False, hooks=hooks, precision=prec)
                assert rc == _lib.NWE_ERR_UNSUPPORTED and named in _error(r) and "nwe_render_rays" in _error(r)
        # the other three modes: not built together, under every precision
        for on, off, word in ((lambda: r.set_early_termination(1e-2), lambda: r.set_early_termination(0.0), "early termination"),
                              (lambda: r.set_shared_coarse(2), lambda: r.set_shared_coarse(1), "shared coarse pass"),
                              (lambda: r.set_separate_passes(True), lambda: r.set_separate_passes(False), "separate passes")):
            on()
            for prec in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32):
                rc, _ = _plan(r, 133, precision=prec)
                assert rc == _lib.NWE_ERR_UNSUPPORTED and named in _error(r) and word in _error(r) and "not built together" in _error(r), _error(r)
            off()
            assert _plan(r, 133)[0] == 0
        # behind every refusal the call has without it
        rc, _ = _plan(r, 133, outputs=("rgb", "feat_map"))
        assert rc == _lib.NWE_ERR_UNSUPPORTED and "feat_map" in _error(r) and named not in _error(r)
        r.clear_occupancy()
        assert _plan(r, 800 * 800)[1].main.variant == 0
    finally:
        r.close()


def test_unfolded_and_unbuilt_shapes_are_refused_under_the_mfma_precisions():
    r = nwe_amd.Renderer(host_only=True)
    try:
        r.debug_set_fold(False)
        r.set_network(0, synthetic.make_state_dict(1000, D=4, W=128))
        r.set_sampling(8, 0)
        r.set_occupancy(np.ones((2, 2, 2), bool), (0, 0, 0), (1, 1, 1), 2)
        rc, _ = _plan(r, 133)
        assert rc == _lib.NWE_ERR_UNSUPPORTED and "packed unfolded" in _error(r) and "occupancy MFMA kernel" in _error(r) and "nwe_set_occupancy" in _error(r)
        assert _plan(r, 133, precision=_lib.PREC_F32)[0] == 0
        # a shape without MFMA kernels: its own refusal comes first, NWE_PREC_F32 renders
        r.debug_set_fold(True)
        r.set_network(0, synthetic.make_state_dict(1000, D=3, W=64, skips=()))
        r.set_occupancy(np.ones((2, 2, 2), bool), (0, 0, 0), (1, 1, 1), 2)
        rc, _ = _plan(r, 133)
        assert rc == _lib.NWE_ERR_UNSUPPORTED and "no MFMA kernel for this network shape" in _error(r)
        assert _plan(r, 133, precision=_lib.PREC_F32)[0] == 0
    finally:
        r.close()


def test_every_built_shape_has_the_occupancy_variant():
    for vd in (True, False):
        for W in (128, 256):
            for D, skips in ((4, ()), (6, (4,)), (8, (4,))):
                r = nwe_amd.Renderer(host_only=True)
                try:
                    r.set_network(0, synthetic.make_state_dict(1, D=D, W=W, skips=skips, use_view_dirs=vd))
                    r.set_sampling(8, 0)
                    r.set_occupancy(np.ones((2, 2, 2), bool), (0, 0, 0), (1, 1, 1), 2)
                    rc, rep = _plan(r, 133)
                    assert rc == 0 and rep.main.variant == 3, (vd, W, D, _error(r))
                finally:
                    r.close()


def test_cell_rule_on_hand_made_points():
    """On a face, outside, NaN, +-inf: a point that is not finite or outside on any axis is occupied."""
    bits = np.zeros((2, 2, 2), bool)
    bits[1, 0, 0] = True
    g = G.make_grid(bits, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))
    assert (g["inv"] == 1.0).all()
    inf, nan = np.inf, np.nan
    pts = np.array([[0.5, 0.5, 0.5],      # cell (0,0,0): empty
                    [1.5, 0.5, 0.5],      # cell (1,0,0): occupied
                    [1.0, 0.5, 0.5],      # on the face between them: floor(1.0) = 1, occupied
                    [0.0, 0.0, 0.0],      # the box's lower corner is inside: cell (0,0,0)
                    [2.0, 0.5, 0.5],      # the upper face is outside: index 2
                    [-1e-6, 0.5, 0.5],    # just below: index -1
                    [0.5, 0.5, 7.0], [nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -inf],
                    [np.nextafter(np.float32(1.0), np.float32(0.0)), 1.5, 1.5]], dtype=np.float32)
    empty, decided = G.classify(pts, g)
    assert empty.tolist() == [True, False, False, True, False, False, False, False, False, False, True]
    assert decided.tolist() == [True, True, False, False, False, False, False, True, True, True, False]
    # the rule rounds in fp32: a point whose fp32 difference lands on the face differs from its fp64 reading
    g2 = G.make_grid(np.zeros((3, 1, 1), bool), (0.1, 0.0, 0.0), (0.4, 1.0, 1.0))
    p = np.array([[0.2, 0.5, 0.5]], np.float32)
    c32, c64 = G.cell_coords(p, g2), G.cell_coords(p.astype(np.float64), g2)
    assert c32.dtype == np.float32 and c64.dtype == np.float64 and c32[0, 0] == (np.float32(0.2) - np.float32(0.1)) * g2["inv"][0]


def test_masked_render_without_a_grid_is_the_oracle_and_all_set_is_too():
    sd_c, sd_f, cfg, _, rays, _, _ = G.scene("fog7")
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    from oracle import nerf_oracle as O
    ref = O.render_rays(rays, t(sd_c), t(sd_f), cfg)
    for kind in (None, "full"):
        m = G.reference("fog7", kind)
        for k, key in (("rgb", "rgb_fine"), ("depth", "depth_fine"), ("acc", "acc_fine")):
            assert torch.equal(m[k], ref[key]), (kind, k)
    none = G.reference("fog7", "none")
    assert float(none["rgb"].abs().max()) == 0 and float(none["acc"].abs().max()) == 0 and float(none["depth"].abs().max()) == 0
    assert G.executed_interval(none, "packets") == (0, 0)
    full = G.reference("fog7", "full")
    assert G.executed_interval(full, "split")[1] == G.full_evaluations(cfg, 133)


def test_executed_interval_arithmetic():
    """Two groups of 2 rays, 4 samples, iterations of 1 and of 4 (GROUP is patched for the arithmetic's sake)."""
    e = np.array([[1, 1, 0, 0], [1, 0, 0, 1], [1, 1, 1, 1], [1, 1, 1, 0]], bool)
    ref = {"coarse": {"may_empty": e.copy(), "may_occupied": ~e}}
    old = dict(G.GROUP)
    try:
        G.GROUP["packets"], G.GROUP["split"] = (2, 1), (2, 4)
        assert G.executed_interval(ref, "packets") == (2 * 3 + 2 * 1,) * 2
        assert G.executed_interval(ref, "split") == (8 + 8,) * 2
        ref["coarse"]["may_empty"][3, 3] = True          # the one occupied sample of group 1 may be empty after all
        assert G.executed_interval(ref, "packets") == (6, 8)
        assert G.executed_interval(ref, "split") == (8, 16)
    finally:
        G.GROUP.update(old)


@pytest.mark.parametrize("kind", G.PARITY_GRIDS)
@pytest.mark.parametrize("name", G.PARITY_SCENES)
def test_parity_scenes_are_valid(name, kind):
    """Per parity scene and grid: decided rays are at least 95 % of the frame by the oracle alone; on them the masked oracle in
    fp32 agrees with its own fp64 run to a tenth of the parity tolerance; and the grid bites - a renderer that ignored it
    would fail the parity test - with groups that skip and groups that do not.  With importance samples, sample_pdf's last bin
    keeps its weight on every ray (tests/occupancy.py: NEAR_LO says why), while the grid still masks coarse samples."""
    kind = G.parity_kind(name, kind)
    if G.scene(name)[2].n_importance > 0:
        empty = G.reference(name, kind)["coarse"]["empty"]
        assert not empty[:, -2].any() and empty.any()
    m, m64, plain = G.reference(name, kind), G.reference(name, kind, fp64=True), G.reference(name, None)
    decided = m["decided"] & m64["decided"]
    assert float(decided.float().mean()) >= 0.95, float(decided.float().mean())
    for k, tol in (("rgb", 1e-5), ("depth", 1e-5 * G.FAR), ("acc", 1e-5)):
        err = (m[k].double() - m64[k]).abs()
        err = err.max(-1).values if err.dim() == 2 else err
        assert float(err[decided].max()) <= tol, (name, kind, k, float(err[decided].max()))
    bites = ((m["rgb"] - plain["rgb"]).abs().max(-1).values > 1e-3) | ((m["acc"] - plain["acc"]).abs() > 1e-3)
    assert float(bites.float().mean()) >= 0.25
    cfg = G.scene(name)[2]
    for plan in ("packets", "split", "f32"):
        lo, hi = G.executed_interval(m, plan)
        assert 0 < lo <= hi <= G.full_evaluations(cfg, 133), (plan, lo, hi)
        assert kind != "half" or hi < G.full_evaluations(cfg, 133), (plan, lo, hi)      # groups that skip, and groups that do not


def test_the_slab_grid_is_exact_for_the_slab_network():
    """sigma_raw of the slab network is exactly +0 wherever the slab grid says empty, with finite colours - in the oracle's fp32
    and fp64 alike - so the masked oracle is the plain oracle bit for bit; and the grid skips: executed < full."""
    from oracle import nerf_oracle as O
    g = G.slab_grid()
    assert not g["bits"].all() and g["bits"].any()
    _, rays = G.E.frame_rays(12, 64)
    for vd, D, W in ((True, 4, 128), (False, 4, 128)):
        sd_c, sd_f = G.slab_state_dict(2000, D, W, vd), G.slab_state_dict(2001, D, W, vd)
        cfg = O.RenderConfig(n_samples=64, n_importance=128)
        rr = rays if vd else rays[:, :8].contiguous()
        for dtype in (torch.float32, torch.float64):
            plain, masked = G.masked_render(rr, sd_c, sd_f, cfg, None, dtype), G.masked_render(rr, sd_c, sd_f, cfg, g, dtype)
            for p in ("coarse", "fine"):
                e = torch.from_numpy(masked[p]["empty"])
                assert e.any() and (plain[p]["raw"][..., 3][e] == 0).all() and torch.isfinite(plain[p]["raw"][e]).all()
            for k in ("rgb", "depth", "acc"):
                assert torch.equal(plain[k], masked[k]), (vd, dtype, k)
        lo, hi = G.executed_interval(masked, "packets")
        assert hi < G.full_evaluations(cfg, 768)
        assert float(masked["acc"].max()) > 0.5          # the slab is there
