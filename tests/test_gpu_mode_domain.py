"""Early ray termination, the shared coarse pass and separate passes (include/nwe.h) on every network shape their kernels are
built for, at sample counts on both sides of the single-packet threshold, and on the degenerate and non-finite inputs of
tests/input_domain.py (tables, scenes and references: tests/mode_domain.py; their premises: tests/test_mode_domain_host.py).

Part A, 7 x 19 x 2 poses = 266 rays (two full 128-ray groups and a ragged packet), the 12 shapes:
  A1  termination that masks nothing equals the plain lean frame bit for bit;
  A2  termination that stops 45 % of the rays (and all of them, at 7 + 6) against the masked oracle, the plans bit-identical,
      the executed evaluations inside the interval the stop indices give;
  A3  the shared coarse pass against each ray's fine pass on its representative's depths, bit for bit;
  A4  separate passes on one shape against the fused call, bit for bit;
  A5  separate passes on two shapes, every ordered pair of neighbours on a ring through the six, against one-shape contexts;
  A6  the same at 96 + 32, 65 + 7 and 128 + 256 (the ABI maximum), where only the sample-split plan is legal.
Part B, 6 x 8 = 48 rays, the 16 pinhole cases on 8x256, 6x256 (the shape whose lean coarse pass keeps its colour) and 4x128
without view directions: flag words that are not zero, NaN patterns, degenerate geometry.
Tolerances are those of tests/test_gpu_early_termination.py; everything else is bit for bit.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from tests import early_termination as E
from tests import input_domain as I
from tests import mode_domain as M
from tests import shared_coarse as SC
from tests import test_gpu_early_termination as TE
from tests import test_gpu_separate_passes as TP
from tests import test_gpu_shared_coarse as TS

pytestmark = pytest.mark.gpu

LEAN = M.LEAN
MFMA = ("f16x3", "f16x1")
COUNT_IDS = [f"{M.kind(*s)}-{ns}+{ni}" for s in M.COUNT_SHAPES for ns, ni in M.BIG_COUNTS]
COUNT_PARAMS = [s + (ns, ni) for s in M.COUNT_SHAPES for ns, ni in M.BIG_COUNTS]


def _renderer(sd_c, sd_f, ns, ni, white=False, tiles=None):
    r = nwe_amd.Renderer(0) if tiles is None else nwe_amd.TiledRenderer(tiles)
    r.set_network(0, sd_c); r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    r.set_white_background(white)
    return r


def _frame(r, precision, outputs=LEAN, rows=None):
    return r.render(M.frame()[0].numpy(), M.H, M.W, rows=rows, precision=precision, outputs=outputs, **M.camera())


def _plans(precision, ns):
    """The decompositions to force: packets, sample split and the hybrid plan under the MFMA precisions - with more than 64
    coarse samples only the sample split is legal, whatever is forced."""
    if precision == "f32":
        return (-1,)
    return (0, 1) if ns > 64 else (0, 1, 2)


def _check_plan(r, precision, mode, ns):
    if precision != "f32":
        assert r.debug_last_plan() == (1 if ns > 64 else mode), (precision, mode, ns, r.debug_last_plan())


def _full(ns, ni, n_rays=M.N_RAYS):
    return n_rays * (ns + ns + ni)


# ---- A1: termination that masks nothing ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,Wd,form", M.SHAPES, ids=M.IDS)
def test_terminating_kernels_of_every_shape_give_the_plain_bits_where_nothing_stops(D, Wd, form):
    """Thin fog, eps = 1e-4: every shape's terminating MLP is the plain lean kernel's, which
    test_raw_outputs_every_instantiation_against_fp64 holds to fp64."""
    sd_c, sd_f, cfg, _, _, _ = M.scene(D, Wd, form, "thin")
    r = _renderer(sd_c, sd_f, 64, 128)
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            for mode in _plans(precision, 64):
                r.debug_set_decomposition(mode)
                r.set_early_termination(0.0)
                plain = _frame(r, precision)
                r.set_early_termination(M.SCENES["thin"][2])
                out = _frame(r, precision)
                _check_plan(r, precision, mode, 64)
                TE._same(out, plain, (M.kind(D, Wd, form), precision, mode))
                assert r.last_ray_evaluations() == (_full(64, 128),) * 2
        print(f"A1 {M.kind(D, Wd, form)}: eps {M.SCENES['thin'][2]:g} equals eps 0 bit for bit in 7 launches, executed == full == {_full(64, 128)}")
    finally:
        r.close()


# ---- A2 / A6: termination that stops rays -------------------------------------------------------------------------------------

def _check_termination(D, Wd, form, name, ns, ni):
    eps = M.SCENES[name][2]
    sd_c, sd_f, cfg, _, _, _ = M.scene(D, Wd, form, name, ns, ni)
    ref = M.masked_reference(D, Wd, form, name, ns, ni)
    S = ns + ni
    iv = M.intervals(ref["stop"], ref["decided"], ns, S, TE.LAG)
    tag = f"{name} {M.kind(D, Wd, form)} {ns}+{ni}"
    print(f"{tag}: {float((ref['stop'] < S).float().mean()):.3f} of the rays stop, {float((~ref['decided']).float().mean()):.3f} undecided")
    r = _renderer(sd_c, sd_f, ns, ni)
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            r.set_early_termination(0.0)
            r.debug_set_decomposition(-1)
            plain = _frame(r, precision)
            r.set_early_termination(eps)
            first = None
            for mode in _plans(precision, ns):
                r.debug_set_decomposition(mode)
                out = _frame(r, precision)
                _check_plan(r, precision, mode, ns)
                ran, full = r.last_ray_evaluations()
                ctx = f"{tag} {precision} d{mode}"
                assert int(out["flags"].item()) & 0x7 == 0, ctx
                if first is None:
                    first = out
                    if precision == "f16x1":
                        for k in LEAN:
                            wide = eps * (E.FAR if k == "depth" else 1.0)
                            err = float(M.per_ray((out[k].cpu() - ref[k]).abs()).max())
                            print(f"{ctx} {k}: max err {err:.2e} (tol {TE.TOL_X1[k] + wide:.1e})")
                            assert err <= TE.TOL_X1[k] + wide, (ctx, k)
                    else:
                        TE._check_against_masked(out, ref, eps, TE.TOL, ctx)
                    assert not torch.equal(out["rgb"], plain["rgb"]), (ctx, "the mode ran")
                else:
                    TE._same(first, out, ctx)
                assert full == _full(ns, ni), ctx
                if precision != "f16x1":      # the fp32-grade precisions: their transmittance is well inside the decided margin
                    lo, hi = iv["f32" if precision == "f32" else ("packets" if mode == 0 and ns <= 64 else "split")]
                    print(f"{ctx}: executed {ran} of {full}, interval [{lo}, {hi}]")
                    assert lo <= ran <= hi, ctx
                if name == "allstop":
                    assert ran < full, ctx
    finally:
        r.close()


@pytest.mark.parametrize("name,ns,ni", [("halfstop", 64, 128), ("allstop", 7, 6)])
@pytest.mark.parametrize("D,Wd,form", M.SHAPES, ids=M.IDS)
def test_termination_on_every_shape_against_the_masked_oracle(D, Wd, form, name, ns, ni):
    """`halfstop`: the image edges stop and the centre does not, in every 128-ray group; `allstop` at 7 + 6: every ray stops
    and the sample-split plan's last iteration is ragged.  Every precision against the masked oracle, the plans bit-identical,
    the executed evaluations inside the interval of the stop indices, the result not the eps = 0 frame."""
    _check_termination(D, Wd, form, name, ns, ni)


@pytest.mark.parametrize("name", ["halfstop", "allstop"])
@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNT_PARAMS, ids=COUNT_IDS)
def test_termination_with_more_than_64_coarse_samples(D, Wd, form, ns, ni, name):
    """96 + 32, 65 + 7 and the ABI maximum 128 + 256: the single-packet workgroup with its other weight layout, whatever plan
    is forced.  `halfstop` masks samples but keeps every workgroup to its last iteration (each group of 16 rays holds one that
    never stops); in `allstop` every workgroup leaves early."""
    _check_termination(D, Wd, form, name, ns, ni)


# ---- A3 / A6: the shared coarse pass ------------------------------------------------------------------------------------------

F32_SHARED = ("6x128", "8x256-noview")         # the fp32 kernel is not instantiated per shape: two of them


def _check_shared(name, ns, ni, white, precisions):
    D, Wd, view = M.NETS[name]
    poses = M.frame()[0].numpy()
    r = _renderer(synthetic.make_state_dict(1000, D, Wd, use_view_dirs=view), synthetic.make_state_dict(1001, D, Wd, use_view_dirs=view),
                  ns, ni, white)
    try:
        for precision in precisions:
            for k in (2, 3):
                r.set_shared_coarse(1)
                r.debug_set_decomposition(-1)
                want = M.expected_shared(r, poses, M.H, M.W, k, precision, view)
                plain = _frame(r, precision)
                r.set_shared_coarse(k)
                for mode in _plans(precision, ns):
                    r.debug_set_decomposition(mode)
                    got = _frame(r, precision)
                    _check_plan(r, precision, mode, ns)
                    TS._same_as_expected(got, want, (name, ns, ni, white, precision, k, mode))
                    assert r.last_coarse_launch()[1] == SC.n_rep(M.H, M.W, k, 0, M.H, M.N_POSES)
                    assert r.last_ray_evaluations() == SC.evaluations(M.H, M.W, k, 0, M.H, M.N_POSES, ns, ni)
                assert not torch.equal(got["rgb"], plain["rgb"]), "the rule changes the frame"
                print(f"A3 {name} {ns}+{ni} {precision} k {k}: the expected frame bit for bit, flags 0x{int(got['flags'].item()):x} "
                      f"(expected render 0x{int(want['flags'].item()):x}), max|shared - plain| rgb {float((got['rgb'] - plain['rgb']).abs().max()):.2e}")
    finally:
        r.close()


@pytest.mark.parametrize("name", M.IDS)
def test_shared_coarse_pass_on_every_shape_bit_for_bit(name):
    """Raw random networks, k = 2 and 3, the three plans; white background on every other shape."""
    _check_shared(name, 64, 128, M.IDS.index(name) % 2 == 1, MFMA + (("f32",) if name in F32_SHARED else ()))


@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNT_PARAMS, ids=COUNT_IDS)
def test_shared_coarse_pass_with_more_than_64_coarse_samples(D, Wd, form, ns, ni):
    _check_shared(M.kind(D, Wd, form), ns, ni, ns == 65, MFMA)


# ---- A4 / A6: separate passes, one shape --------------------------------------------------------------------------------------

def _check_separate(name, ns, ni, white):
    D, Wd, view = M.NETS[name]
    r = TP._renderer(name, name, ns, ni, white=white)
    try:
        rays = r.create_rays(M.frame()[0].numpy(), M.H, M.W, use_view_dirs=view, **M.camera())

        def calls(precision):
            return {"lean": _frame(r, precision), "full": _frame(r, precision, outputs=TP.FULL),
                    "rows": _frame(r, precision, rows=(3, 6), outputs=LEAN + ("rgb_coarse", "z_fine")),
                    "rays": r.render_rays(rays, precision=precision, outputs=TP.FULL)}

        for precision in MFMA:
            r.set_separate_passes(False)
            r.debug_set_decomposition(-1)
            off = calls(precision)
            assert r.last_coarse_launch() is None
            r.set_separate_passes(True)
            for mode in _plans(precision, ns):
                r.debug_set_decomposition(mode)
                on = calls(precision)
                _check_plan(r, precision, mode, ns)
                assert r.last_coarse_launch()[1] == M.N_RAYS
                for key in off:
                    TP._same(on[key], off[key], (name, ns, ni, precision, white, mode, key))
            print(f"A4 {name} {ns}+{ni} {precision}: on equals off bit for bit in 4 calls x {len(_plans(precision, ns))} plans, flags "
                  + ", ".join(f"{key} 0x{int(v['flags'].item()):x}" for key, v in off.items()))
    finally:
        r.close()


@pytest.mark.parametrize("name", M.IDS)
def test_separate_passes_on_every_shape_equal_the_fused_call(name):
    """A lean frame, a frame with every output, the row tile (3, 6) and render_rays with every output: mode on against off,
    outputs and flag words, under the three forced plans."""
    _check_separate(name, 64, 128, M.IDS.index(name) % 2 == 0)


@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNT_PARAMS, ids=COUNT_IDS)
def test_separate_passes_with_more_than_64_coarse_samples(D, Wd, form, ns, ni):
    _check_separate(M.kind(D, Wd, form), ns, ni, ns == 96)


# ---- A5: separate passes, two shapes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse,fine", M.PAIRS, ids=[f"c{a}-f{b}" for a, b in M.PAIRS])
def test_every_neighbouring_pair_of_shapes_equals_the_passes_of_one_shape_contexts(coarse, fine):
    """The check of test_mixed_shapes_equal_the_passes_of_one_shape_contexts - render_rays and render with every output, a lean
    frame, the three plans, against a (coarse, coarse) and a (fine, fine) context, the flag word against the fp32 kernel's -
    for each ordered pair; f16x1 on every other pair."""
    i = M.PAIRS.index((coarse, fine))
    for precision in MFMA[:1 + i % 2]:
        TP.test_mixed_shapes_equal_the_passes_of_one_shape_contexts(coarse, fine, 64, 128, precision, i % 4 < 2)
        print(f"A5 c{coarse} f{fine} {precision}: every output of render_rays and render bit for bit")


@pytest.mark.parametrize("coarse,fine", [("8x256", "6x128"), ("6x256", "4x128")])
@pytest.mark.parametrize("precision", MFMA)
def test_shared_coarse_pass_composes_with_a_pair_that_holds_a_six_deep_network(coarse, fine, precision):
    """A 6-deep consumer, and a 6-deep producer - the one whose lean coarse pass still computes its colour: k = 2."""
    TP.test_shared_coarse_pass_composes_with_a_mixed_pair(2, coarse, fine, 64, 128, precision, precision == "f16x1")


# ---- B: the input-domain table ------------------------------------------------------------------------------------------------

DOMAIN_IDS = [M.kind(*s) for s in M.DOMAIN_SHAPES]


def _cam(case):
    return dict(M.camera(I.H, I.W), near=case.near, far=case.far)


def _domain_frame(r, case, precision, outputs=LEAN):
    return r.render(case.pose, I.H, I.W, precision=precision, outputs=outputs, **_cam(case))


def _bad_rays(t):
    return I.ray_mask(~torch.isfinite(t).cpu().numpy())


@pytest.mark.parametrize("name", M.DOMAIN_CASES)
@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_separate_passes_on_degenerate_inputs_keep_the_outputs_and_raise_the_fused_flags(D, Wd, form, name):
    """B1: lean frame, full frame and a lean frame of two context tiles, mode on against off: outputs (NaN-aware) and flag
    words equal, and the word is the one include/nwe.h promises for the oracle's outputs - lean frames raise
    NWE_FLAG_RGB_COARSE exactly where the coarse colour exists (6x256, no view directions), full frames everywhere."""
    case = I.BY_NAME[name]
    _, sd_c, sd_f, res = M.domain_oracle(name, D, Wd, form)
    d_only = M.density_only(D, Wd, form)
    want = {"lean": I.expected_flags(res, I.LEAN, True, density_only=d_only), "full": I.expected_flags(res, I.FULL, True)}
    want["tiled"] = want["lean"]
    r, tiled = _renderer(sd_c, sd_f, I.NS, I.NI), _renderer(sd_c, sd_f, I.NS, I.NI, tiles=[0, 0])
    try:
        def calls(precision):
            out = {"lean": _domain_frame(r, case, precision), "full": _domain_frame(r, case, precision, I.FULL),
                   "tiled": _domain_frame(tiled, case, precision)}
            assert tiled.last_tiled
            return out

        for precision in MFMA:
            for x in (r, tiled):
                x.set_separate_passes(False)
            r.debug_set_decomposition(-1)
            off = calls(precision)
            for x in (r, tiled):
                x.set_separate_passes(True)
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                on = calls(precision)
                assert r.last_coarse_launch()[1] == I.H * I.W and all(p.last_coarse_launch() is not None for p in tiled.parts)
                for key in off:
                    ctx = (name, M.kind(D, Wd, form), precision, mode, key)
                    TP._same(on[key], off[key], ctx)
                    assert int(on[key]["flags"].item()) == want[key], (ctx, hex(int(on[key]["flags"].item())), hex(want[key]))
            print(f"B1 {name} {M.kind(D, Wd, form)} {precision}: on equals off; flags lean 0x{want['lean']:x}, full 0x{want['full']:x}")
        if name == "nan_rgb_linear_coarse":
            assert bool(want["lean"] & I.FLAG_RGB_COARSE) == (not d_only) and want["full"] & I.FLAG_RGB_COARSE
    finally:
        r.close(); tiled.close()


@pytest.mark.parametrize("spoiled", ["coarse 6x256", "coarse 8x256"])
def test_separate_passes_or_the_flags_of_two_launches_of_two_shapes(spoiled):
    """A coarse network with a NaN in its colour head under a clean fine network of another shape: the full frame's word is the
    fp32 kernel's for the same pair (the OR of both launches); a lean frame raises NWE_FLAG_RGB_COARSE from the 6-deep coarse
    network, whose lean coarse pass computes the colour, and nothing from the 8-deep one."""
    case, healthy = I.BY_NAME["nan_rgb_linear_coarse"], I.BY_NAME["healthy"]
    Dc, Df = (6, 8) if spoiled == "coarse 6x256" else (8, 6)
    sd_c, sd_f = I.nets(case, Dc, 256, "folded")[0], I.nets(healthy, Df, 256, "folded")[1]
    r = _renderer(sd_c, sd_f, I.NS, I.NI)
    try:
        r.set_separate_passes(True)
        f32 = _domain_frame(r, case, "f32", I.FULL)
        want = int(f32["flags"].item())
        assert want & I.FLAG_RGB_COARSE and want & I.FLAG_RAW and want & 0x7 == 0, hex(want)
        for precision in MFMA:
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                full, lean = _domain_frame(r, case, precision, I.FULL), _domain_frame(r, case, precision)
                print(f"B1 {spoiled} spoiled, {precision} d{mode}: full 0x{int(full['flags'].item()):x} (fp32 kernel 0x{want:x}), lean 0x{int(lean['flags'].item()):x}")
                assert int(full["flags"].item()) == want, (spoiled, precision, mode)
                for k in ("rgb_coarse", "raw_coarse"):
                    assert _bad_rays(full[k]).all(), k
                for k in LEAN + ("depth_coarse", "acc_coarse"):
                    assert torch.isfinite(full[k]).all() and torch.isfinite(f32[k]).all(), k
                assert int(lean["flags"].item()) & ~I.FLAG_DISP & ~I.FLAG_DISP_COARSE == (I.FLAG_RGB_COARSE if Dc == 6 else 0), (spoiled, precision, mode)
    finally:
        r.close()


@pytest.mark.parametrize("name", M.DOMAIN_CASES)
@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_shared_coarse_pass_on_degenerate_inputs(D, Wd, form, name):
    """B2, k = 2.  Finite coarse depths: the expected frame bit for bit with its NaN positions, the fine flag bits of the
    expected render, no coarse bit, and the non-finite rays of the oracle-side shared reference.  far_inf and nan_c2w (the order
    of non-finite depths is not specified): every ray non-finite in all three outputs, bits 0-2 set, bits 4-7 clear."""
    case = I.BY_NAME[name]
    _, sd_c, sd_f, _ = M.domain_oracle(name, D, Wd, form)
    ref = M.domain_shared_reference(name, D, Wd, form, 2)
    view = form != "no_view_dirs"
    r = _renderer(sd_c, sd_f, I.NS, I.NI)
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            r.set_shared_coarse(1)
            r.debug_set_decomposition(-1)
            want = M.expected_shared(r, case.pose, I.H, I.W, 2, precision, view, _cam(case)) if name in M.FINITE_DEPTHS else None
            r.set_shared_coarse(2)
            for mode in ((0, 1) if precision != "f32" else (-1,)):
                r.debug_set_decomposition(mode)
                got = _domain_frame(r, case, precision)
                word = int(got["flags"].item())
                ctx = (name, M.kind(D, Wd, form), precision, mode)
                assert r.last_coarse_launch()[1] == SC.n_rep(I.H, I.W, 2, 0, I.H, 1)
                assert word & 0xF0 == 0, (ctx, hex(word))
                if want is not None:
                    TS._same_as_expected(got, want, ctx)
                    for k in LEAN:
                        assert np.array_equal(_bad_rays(got[k]), _bad_rays(ref[k])), (ctx, k, int(_bad_rays(got[k]).sum()), int(_bad_rays(ref[k]).sum()))
                else:
                    assert all(_bad_rays(got[k]).all() for k in LEAN) and word & 0x7 == 0x7, (ctx, hex(word))
            print(f"B2 {name} {M.kind(D, Wd, form)} {precision}: flags 0x{word:x}, non-finite rays "
                  + ", ".join(f"{k} {int(_bad_rays(got[k]).sum())}" for k in LEAN))
    finally:
        r.close()


@pytest.mark.parametrize("name", M.DOMAIN_CASES)
@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_termination_on_degenerate_inputs(D, Wd, form, name):
    """B3, eps = 1e-2 with the fine fog (0.4, 0.01), against E.masked_outputs on the oracle's fine pass of the case: the
    non-finite rays of rgb / depth / acc and flag bits 0-2 are the reference's, bits 4-7 those of the eps = 0 lean frame, the
    finite decided rays within the parity tolerances (f16x1: its documented tolerance plus eps), the plans bit-identical."""
    case = I.BY_NAME[name]
    _, sd_c, sd_f, _ = M.domain_oracle(name, D, Wd, form, M.FINE_FOG)
    ref = M.domain_masked_reference(name, D, Wd, form)
    bad = {k: _bad_rays(ref[k]) for k in LEAN}
    want_fine = sum(bit for bit, k in ((I.FLAG_RGB, "rgb"), (I.FLAG_DEPTH, "depth"), (I.FLAG_ACC, "acc")) if bad[k].any())
    decided = ref["decided"].numpy()
    S = I.NS + I.NI
    r = _renderer(sd_c, sd_f, I.NS, I.NI)
    try:
        for precision in ("f16x3", "f16x1", "f32"):
            r.set_early_termination(0.0)
            r.debug_set_decomposition(-1)
            plain = _domain_frame(r, case, precision)
            r.set_early_termination(M.DOMAIN_EPS)
            first, worst = None, {}
            for mode in ((0, 1) if precision != "f32" else (-1,)):
                r.debug_set_decomposition(mode)
                out = _domain_frame(r, case, precision)
                word = int(out["flags"].item())
                ctx = (name, M.kind(D, Wd, form), precision, mode)
                if first is not None:
                    TE._same(first, out, ctx)
                    continue
                first = out
                assert word & 0x7 == want_fine, (ctx, hex(word), hex(want_fine))
                assert word & 0xF0 == int(plain["flags"].item()) & 0xF0, (ctx, hex(word), hex(int(plain["flags"].item())))
                for k in LEAN:
                    assert np.array_equal(_bad_rays(out[k]), bad[k]), (ctx, k, int(_bad_rays(out[k]).sum()), int(bad[k].sum()))
                    err = M.per_ray((out[k].cpu() - ref[k]).abs()).numpy()
                    wide = M.DOMAIN_EPS * (E.FAR if k == "depth" else 1.0)
                    ok = ~bad[k]
                    if precision == "f16x1":
                        tol_d = tol_u = TE.TOL_X1[k] + wide
                    else:
                        tol_d, tol_u = TE.TOL[k], TE.TOL[k] + wide
                    e_d = float(err[ok & decided].max()) if (ok & decided).any() else 0.0
                    e_u = float(err[ok & ~decided].max()) if (ok & ~decided).any() else 0.0
                    worst[k] = (e_d, e_u)
                    assert e_d <= tol_d and e_u <= tol_u, (ctx, k, e_d, e_u)
            print(f"B3 {name} {M.kind(D, Wd, form)} {precision}: {int((ref['stop'] < S).sum())} of 48 rays stop, {int((~ref['decided']).sum())} undecided, "
                  f"flags 0x{word:x}, max err decided / undecided " + ", ".join(f"{k} {a:.1e} / {b:.1e}" for k, (a, b) in worst.items()))
    finally:
        r.close()
