"""Degenerate and non-finite inputs in every kernel mode (the case table of tests/input_domain.py; its expectations are checked
against the CPU oracle by tests/test_input_domain_oracle.py).

The other GPU tests feed healthy rays and finite networks.  Here: NaN / inf / zero-length rays, near == far, far = inf, NaN poses,
NaN and inf weights and biases, coordinates from 0 to 1e12 - on the f32 kernel, on f16x3 in both decompositions, lean and full,
and on f16x1; 8x256 and 4x128 folded, one instantiation without view directions and one in the reference formulation.
  * every output's non-finite mask equals the fp32 oracle's per element and `flags` is the word include/nwe.h promises;
  * where the outputs are finite they meet the criterion of tests/accuracy.py (FACTOR, FLOOR unchanged; K32 per group, its
    measured maximum rounded up, never above 6; DESIGN.md section 6.1 tabulates the ratios);
  * raw outputs over the coordinate sweep against fp64 at the reference's fp32 points (tests/accuracy.raw_at_depths);
  * healthy rays are bit-identical with and without poisoned neighbours in their packet;
  * the conditioning diagnostics equal the oracle's on the kernel's own coarse weights, NaN positions included;
  * far < near is refused (the sorted merge needs ascending depths).
"""
import numpy as np
import pytest
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import accuracy as A
from tests import input_domain as I
from tests.test_gpu_accuracy import _emulate_x1, _same_flags

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
K32_CAP = 6.0                       # the largest K32 this project has accepted (tests/test_gpu_accuracy.py)
RAY_MODES = (("f32", -1), ("f16x3", 0), ("f16x3", 1), ("f16x1", 0))          # nwe_render_rays: never a lean launch
FRAME_MODES = tuple((p, m, lean) for p, m in RAY_MODES for lean in (False, True))
INST_IDS = [f"{D}x{W}-{f}" for D, W, f in I.INSTANTIATIONS]
DIAG = ("sample_cond", "sample_amp", "sample_switch")


def _renderer(sd_c, sd_f, form, ns=I.NS, ni=I.NI, tiles=None):
    r = nwe_amd.Renderer(0) if tiles is None else nwe_amd.TiledRenderer(tiles)
    r.debug_set_fold(form != "reference")
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    return r


def _name(prec, mode, lean=None):
    return prec + (f" d{mode}" if mode >= 0 else "") + ("" if lean is None else (" lean" if lean else " full"))


def _beyond_mfma_range(case):
    """Coordinates an MFMA mode cannot represent (fp16 hi + lo of x / 10 >= 65520, octave arguments >= 1.6e6): include/nwe.h
    promises NaN and the flags there, not the reference's finite values; test_coordinate_sweep holds them to that."""
    return case.name in [f"origin_{s:g}" for s in I.SWEEP_BEYOND]


def _check_masks(problems, tag, got, masks, outputs, z_fine=None):
    """`z_fine`: the oracle's fine depths, for the cases whose coarse depths are finite: there the kernel's z_fine equals it in
    its NaN positions (torch.sort puts NaN samples behind every depth) and has no inf."""
    if z_fine is not None and "z_fine" in outputs:
        z = got["z_fine"].cpu()
        if not torch.equal(torch.isnan(z), torch.isnan(z_fine)) or torch.isinf(z).any():
            problems.append(f"{tag} z_fine: NaN at {int(torch.isnan(z).sum())} positions (oracle {int(torch.isnan(z_fine).sum())}), "
                            f"{int((torch.isnan(z) != torch.isnan(z_fine)).sum())} of them elsewhere, inf at {int(torch.isinf(z).sum())}")
    for k in outputs:
        if k not in masks:
            continue
        m = ~torch.isfinite(got[k]).cpu().numpy()
        if not np.array_equal(m, masks[k]):
            diff = m != masks[k]
            rays = np.nonzero(I.ray_mask(diff))[0].tolist()
            problems.append(f"{tag} {k}: non-finite mask differs from the fp32 oracle's on {int(diff.sum())} elements, rays {rays[:10]} "
                            f"(kernel non-finite {int(m.sum())}, oracle {int(masks[k].sum())})")


def _frame_kw(case):
    fx, fy, cx, cy = O.intrinsics(I.H, I.W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=case.near, far=case.far)


# ------------------------------------------------------------------------------------------------------------------------
# 1. masks and flags
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in I.CASES])
@pytest.mark.parametrize("D,W,form", I.INSTANTIATIONS, ids=INST_IDS)
def test_masks_and_flags_equal_the_oracles(D, W, form, name):
    """Every output's non-finite mask per element and the flag word, through nwe_render_rays in every mode and - pinhole cases -
    through nwe_render, full and lean, and nwe_render_tiled (two tiles on one device)."""
    case = I.BY_NAME[name]
    rays, sd_c, sd_f, res = I.run_oracle(case, D, W, form)
    masks = I.oracle_masks(res, True)
    z_ref = res["z_fine"] if torch.isfinite(res["z_coarse"]).all() else None   # NaN / inf coarse depths: a merge cannot sort them
    r = _renderer(sd_c, sd_f, form)
    assert np.isfinite(r.packed_scale(0)) and np.isfinite(r.packed_scale(1)) and r.packed_scale(0) > 0 and r.packed_scale(1) > 0
    problems, flags = [], {}
    try:
        for prec, mode in RAY_MODES:
            if prec != "f32" and _beyond_mfma_range(case):
                continue
            r.debug_set_decomposition(mode)
            got = r.render_rays(rays.cuda(), precision=prec, outputs=I.FULL)
            tag = f"{name} {D}x{W} {form} rays {_name(prec, mode)}"
            _check_masks(problems, tag, got, masks, I.FULL, z_ref)
            want = I.expected_flags(res, I.FULL, True)
            flags[tag] = int(got["flags"].item())
            if flags[tag] != want:
                problems.append(f"{tag}: flags 0x{flags[tag]:x}, expected 0x{want:x}")
        if case.pose is not None:
            for prec, mode, lean in FRAME_MODES:
                r.debug_set_decomposition(mode)
                outs = I.LEAN if lean else I.FULL
                got = r.render(case.pose, I.H, I.W, precision=prec, outputs=outs, **_frame_kw(case))
                tag = f"{name} {D}x{W} {form} frame {_name(prec, mode, lean)}"
                _check_masks(problems, tag, got, masks, outs, z_ref)
                density_only = lean and prec != "f32" and form == "folded"
                want = I.expected_flags(res, outs, True, density_only=density_only)
                flags[tag] = int(got["flags"].item())
                if flags[tag] != want:
                    problems.append(f"{tag}: flags 0x{flags[tag]:x}, expected 0x{want:x}")
                if lean and case.density_only_sees_nothing and density_only:
                    assert want == 0, "a defect in the coarse colour head alone: a density-only lean frame sees nothing"
    finally:
        r.debug_set_decomposition(-1)
        r.close()
    assert not problems, "\n".join(problems)
    # the rule of test_gpu_accuracy._same_flags across modes, among the calls that requested the same outputs
    _same_flags({k: v for k, v in flags.items() if " lean" not in k})
    _same_flags({k: v & ~I.FLAG_RGB_COARSE for k, v in flags.items() if " lean" in k})


@pytest.mark.parametrize("name", ["healthy"] + I.GEOMETRY_CASES)
def test_degenerate_geometry_through_the_tiled_frame(name):
    """nwe_render_tiled, two tiles on one device: the assembled frame's masks and the OR-ed flag word."""
    case = I.BY_NAME[name]
    rays, sd_c, sd_f, res = I.run_oracle(case, 8, 256, "folded")
    masks = I.oracle_masks(res, True)
    r = _renderer(sd_c, sd_f, "folded", tiles=[0, 0])
    problems = []
    try:
        for prec in ("f32", "f16x3", "f16x1"):
            got = r.render(case.pose, I.H, I.W, precision=prec, outputs=I.LEAN, **_frame_kw(case))
            assert r.last_tiled
            _check_masks(problems, f"{name} tiled {prec}", got, masks, I.LEAN)
            want = I.expected_flags(res, I.LEAN, True, density_only=prec != "f32")
            if int(got["flags"].item()) != want:
                problems.append(f"{name} tiled {prec}: flags 0x{int(got['flags'].item()):x}, expected 0x{want:x}")
    finally:
        r.close()
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------------------------------
# 2. values where finite
# ------------------------------------------------------------------------------------------------------------------------

# K32 per case group: the measured maximum ratio of the f32 kernel's error to the fp32 reference's, rounded up
VALUE_CASES = ["healthy", "near_eq_far", "zero_direction", "underflow_direction", "poisoned_neighbours", "nan_weight_fine_trunk",
               "nan_alpha_linear_fine", "nan_rgb_linear_coarse", "nan_rgb_linear_fine"]
VALUE_K32 = {"healthy": 2.5, "near_eq_far": 1.5, "zero_direction": 1.5, "underflow_direction": 1.5, "poisoned_neighbours": 2.5,
             "nan_weight_fine_trunk": 2.5, "nan_alpha_linear_fine": 2.5, "nan_rgb_linear_coarse": 2.5, "nan_rgb_linear_fine": 2.5}
VALUE_KEYS = ("rgb", "depth", "acc", "z_std", "rgb_coarse", "depth_coarse", "acc_coarse")
DEPTH_KEYS = ("depth", "depth_coarse", "z_std", "z_fine")


# every case on the two folded shapes; the formulation without view directions and the reference form on two of them
VALUE_PARAMS = [(D, W, f, n) for D, W, f in I.INSTANTIATIONS for n in VALUE_CASES if f == "folded" or n in ("healthy", "zero_direction")]


@pytest.mark.parametrize("D,W,form,name", VALUE_PARAMS, ids=[f"{D}x{W}-{f}-{n}" for D, W, f, n in VALUE_PARAMS])
def test_values_where_finite_against_fp64(D, W, form, name):
    """On the elements that are finite (in both oracles; the kernel's mask is pinned by the test above) the criterion of
    tests/accuracy.py, unchanged.  Rays on the alpha step of the last sample (|sigma_last| < 1e-5 in fp64) are left out of the
    outputs of that pass, at most 5 % of a case's rays (asserted on the oracle alone by the CPU test for the all-finite cases).
    On the 32 x 48 frame (1542 rays of the ray table): the statistics of 48 rays are single rays (tests/input_domain.py).
    Through nwe_render_rays with every output (the full launch) and, for the pinhole cases, through nwe_render requesting
    rgb / depth / acc only (the lean launch, whose coarse pass evaluates the density alone in the folded form), under the same
    bounds.  Not here: nwe_render_tiled (it assembles tiles of the same lean launches; its masks and flags are checked above)
    and f16x1 end to end - that mode is ~1e-3 on rgb by design (include/nwe.h), there is no fp32-grade criterion to hold it to,
    and its arithmetic is compared with the emulated single product on the raw outputs of the coordinate sweep, as
    test_gpu_accuracy.py does for healthy inputs."""
    case = I.BY_NAME[name]
    k32 = VALUE_K32[name]
    assert k32 <= K32_CAP
    rays, sd_c, sd_f, res32 = I.run_oracle(case, D, W, form, big=True)
    res64 = I.run_oracle(case, D, W, form, F64, big=True)[3]
    r = _renderer(sd_c, sd_f, form)
    rep = A.Report()
    try:
        outs = {_name(p, m): None for p, m in RAY_MODES}
        for prec, mode in RAY_MODES:
            r.debug_set_decomposition(mode)
            outs[_name(prec, mode)] = r.render_rays(rays.cuda(), precision=prec, outputs=I.FULL)
        kf = outs["f32"]
        lean = {}
        if case.pose is not None:            # the same frame through nwe_render requesting rgb / depth / acc only: the LEAN launch
            fx, fy, cx, cy = O.intrinsics(I.BIG_H, I.BIG_W)
            for prec, mode in RAY_MODES[:3]:
                r.debug_set_decomposition(mode)
                lean[_name(prec, mode)] = r.render(case.pose, I.BIG_H, I.BIG_W, precision=prec, outputs=I.LEAN, fx=fx, fy=fy, cx=cx, cy=cy,
                                                   near=case.near, far=case.far)
        for key in VALUE_KEYS:
            ok = I.oracle_key(key, True)
            y32, y64 = res32[ok], res64[ok]
            sig = res64["raw_coarse" if key in I.COARSE_SIDE else "raw_fine"][:, -1, 3]
            step = (sig.abs() < 1e-5).numpy()                         # NaN compares False: a NaN sigma leaves nothing finite anyway
            fin = torch.isfinite(y32).reshape(len(rays), -1).all(-1) & torch.isfinite(y64).reshape(len(rays), -1).all(-1)
            keep = fin.numpy() & ~step
            assert step[fin.numpy()].sum() <= 0.05 * max(int(fin.sum()), 1) + 1e-9, (key, int(step.sum()), int(fin.sum()))
            if not keep.any():
                continue
            scale = case.far if key in DEPTH_KEYS and np.isfinite(case.far) else (I.FAR if key in DEPTH_KEYS else 1.0)
            for prec, mode in RAY_MODES:
                tag = f"{name} {D}x{W} {form} {_name(prec, mode)} {key}"
                if prec == "f32":
                    rep.add(tag, kf[key], y32, y64, scale=scale, keep=keep, factor=k32)
                elif prec == "f16x3":
                    rep.add(tag, outs[_name(prec, mode)][key], y32, y64, scale=scale, keep=keep, y_alt=kf[key], alt_cap=k32)
                if key in I.LEAN and _name(prec, mode) in lean:
                    got = lean[_name(prec, mode)][key]
                    if prec == "f32":
                        rep.add(tag + " (lean frame)", got, y32, y64, scale=scale, keep=keep, factor=k32)
                    else:
                        rep.add(tag + " (lean frame)", got, y32, y64, scale=scale, keep=keep, y_alt=kf[key], alt_cap=k32)
                # f16x1 is ~1e-3 on rgb by design (include/nwe.h); its arithmetic is held to the emulator in test_coordinate_sweep
    finally:
        r.debug_set_decomposition(-1)
        r.close()
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 3. coordinate sweep, raw outputs
# ------------------------------------------------------------------------------------------------------------------------

# K32 of the raw outputs per origin scale (f32 kernel against the fp32 reference at the same fp32 points, both against fp64 at
# those points): measured maximum rounded up
SWEEP_K32 = {0.0: 1.5, 1e-20: 1.5, 1.0: 1.5, 22.0: 1.5, 1e2: 1.5, 1e3: 2.0, 1e4: 2.0, 4e5: 1.5, 1e6: 2.0, 3e7: 2.0, 1e12: 2.0}


@pytest.mark.parametrize("scale", I.SWEEP_SCALES + I.SWEEP_BEYOND, ids=lambda s: f"{s:g}")
@pytest.mark.parametrize("D,W,form", I.INSTANTIATIONS, ids=INST_IDS)
def test_coordinate_sweep_raw_outputs_against_fp64_at_fp32_points(D, W, form, scale):
    """Both networks at the kernel's own sample points.  Ground truth: encoding and MLP in fp64 on the reference's fp32 points
    (at 1e4 the plain fp64 path differs from the fp32 reference by 7e-3, all of it point rounding); yardstick: the fp32 oracle
    at the same points.  Up to 4e5 every mode meets the criterion.  Beyond (1e6, 3e7, 1e12: x / 10 no longer fits fp16
    hi + lo, octave arguments beyond 1.6e6) the f32 kernel still does, and an MFMA mode must either meet it or return NaN and raise
    NWE_FLAG_RAW and the rgb / depth / acc bits: finite values outside the criterion are a bug."""
    case = I.BY_NAME[f"origin_{scale:g}"]
    k32 = SWEEP_K32[scale]
    assert k32 <= K32_CAP
    sd_c, sd_f = I.nets(case, D, W, form)
    tc, tf = I.tensors(sd_c), I.tensors(sd_f)
    rays = case.make_rays(form != "no_view_dirs")
    t = torch.linspace(0., 1., I.NS)
    z_c = rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t
    ref = lambda z, state, dtype: A.raw_at_depths(rays, z, state, dtype, fp32_points=True)
    c32, c64 = ref(z_c, tc, F32), ref(z_c, tc, F64)
    beyond = scale in I.SWEEP_BEYOND
    r = _renderer(sd_c, sd_f, form)
    rep = A.Report()
    problems = []
    outs = ("raw_coarse", "raw_fine", "z_fine", "rgb", "depth", "acc")
    try:
        kf = r.render_rays(rays.cuda(), precision="f32", outputs=outs)
        assert torch.isfinite(kf["raw_coarse"]).all() and torch.isfinite(kf["raw_fine"]).all(), "the f32 kernel has no coordinate limit"
        for prec, mode in RAY_MODES:
            r.debug_set_decomposition(mode)
            got = kf if prec == "f32" else r.render_rays(rays.cuda(), precision=prec, outputs=outs)
            tag = f"origin {scale:g} {D}x{W} {form} {_name(prec, mode)}"
            flag = int(got["flags"].item())
            fin_c = torch.isfinite(got["raw_coarse"]).reshape(len(rays), -1).all(-1).cpu().numpy()
            fin_f = torch.isfinite(got["raw_fine"]).reshape(len(rays), -1).all(-1).cpu().numpy()
            if not (fin_c.all() and fin_f.all()):
                print(f"{tag}: {int((~fin_c).sum())} / {int((~fin_f).sum())} of {len(rays)} rays with non-finite raw_coarse / raw_fine, flags 0x{flag:x}")
                if not beyond:
                    problems.append(f"{tag}: non-finite raw outputs inside the documented coordinate range")
                    continue
                need = I.FLAG_RAW | I.FLAG_RGB | I.FLAG_DEPTH | I.FLAG_ACC
                if flag & need != need:
                    problems.append(f"{tag}: non-finite raw outputs, flags 0x{flag:x} lack some of 0x{need:x}")
                bad = ~(fin_c & fin_f)
                if torch.isfinite(got["rgb"]).all(-1).cpu().numpy()[bad].any() or torch.isfinite(got["acc"]).cpu().numpy()[bad].any():
                    problems.append(f"{tag}: a ray with non-finite raw outputs has a finite rgb or acc")
            z_f = got["z_fine"].cpu()
            if not torch.isfinite(z_f).all():
                continue                                           # all NaN (asserted above with the flags): nothing to compare
            f32_, f64_ = ref(z_f, tf, F32), ref(z_f, tf, F64)
            if prec == "f32":
                rep.add(f"{tag} raw_coarse", got["raw_coarse"], c32, c64, keep=fin_c, factor=k32)
                rep.add(f"{tag} raw_fine", got["raw_fine"], f32_, f64_, keep=fin_f, factor=k32)
            elif prec == "f16x3":
                kf_fine = kf["raw_fine"]
                if not torch.equal(z_f, kf["z_fine"].cpu()):
                    kf_fine = r.render_rays(rays.cuda(), precision="f32", outputs=("raw_fine",), debug_fine_depths=z_f)["raw_fine"]
                if fin_c.any():
                    rep.add(f"{tag} raw_coarse", got["raw_coarse"], c32, c64, keep=fin_c, y_alt=kf["raw_coarse"], alt_cap=k32)
                if fin_f.any():
                    rep.add(f"{tag} raw_fine", got["raw_fine"], f32_, f64_, keep=fin_f, y_alt=kf_fine, alt_cap=k32)
            elif fin_c.all() and fin_f.all():                      # f16x1: against the emulated single-product arithmetic
                n = 16
                fold = form != "reference"
                rep.add(f"{tag} raw_coarse (vs emulated x1)", got["raw_coarse"][:n], _emulate_x1(sd_c, fold, rays[:n], z_c[:n]), c64[:n])
                rep.add(f"{tag} raw_fine (vs emulated x1)", got["raw_fine"][:n], _emulate_x1(sd_f, fold, rays[:n], z_f[:n]), f64_[:n])
    finally:
        r.debug_set_decomposition(-1)
        r.close()
    assert not problems, "\n".join(problems)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 4. poisoned neighbours
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,W,form", I.INSTANTIATIONS, ids=INST_IDS)
def test_healthy_rays_do_not_see_poisoned_neighbours(D, W, form):
    """NaN, inf and zero-direction rays inside the same 32-ray packets as healthy ones (three packets, the last ragged), plans
    0 (packets), 1 (sample split) and 2 (packets + split rest): the healthy rays' outputs are bit-identical to the same rays
    rendered without the poisoned ones in the same mode."""
    case = I.BY_NAME["poisoned_neighbours"]
    sd_c, sd_f = I.nets(case, D, W, form)
    vd = form != "no_view_dirs"
    mixed, clean = I.poisoned_rays(vd).cuda(), I.poisoned_rays(vd, healthy_only=True).cuda()
    healthy = torch.tensor([i for i in range(I.POISON_RAYS) if i not in I.POISON]).cuda()
    r = _renderer(sd_c, sd_f, form)
    problems = []
    try:
        for prec, plans in (("f32", (-1,)), ("f16x3", (0, 1, 2)), ("f16x1", (0, 1, 2))):
            for plan in plans:
                r.debug_set_decomposition(plan)
                a = r.render_rays(mixed, precision=prec, outputs=I.FULL + DIAG)
                if prec != "f32":
                    assert r.debug_last_plan() == plan
                b = r.render_rays(clean, precision=prec, outputs=I.FULL + DIAG)
                alone = r.render_rays(clean[healthy].contiguous(), precision=prec, outputs=I.FULL + DIAG)
                assert int(b["flags"].item()) == 0 and int(alone["flags"].item()) == 0
                for k in I.FULL + DIAG:
                    if not torch.equal(a[k][healthy], b[k][healthy]):
                        problems.append(f"{prec} plan {plan} {k}: healthy rays differ next to poisoned ones")
                    if not torch.equal(a[k][healthy], alone[k]):
                        problems.append(f"{prec} plan {plan} {k}: healthy rays differ from the same rays rendered alone")
    finally:
        r.debug_set_decomposition(-1)
        r.close()
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------------------------------
# 5. diagnostics on the non-finite cases
# ------------------------------------------------------------------------------------------------------------------------

def _same_with_nan(a, b, rel=0.0, abs_=0.0):
    """Equal NaN and inf positions (with sign), and the finite values within rel * |b| + abs_."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    inf = np.isinf(a) | np.isinf(b)
    if not np.array_equal(a[inf], b[inf]):
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    return bool(np.all(np.abs(a[fin] - b[fin]) <= rel * np.abs(b[fin]) + abs_))


@pytest.mark.parametrize("name", ["zero_direction", "far_inf", "nan_c2w", "poisoned_neighbours", "nan_weight_coarse_trunk",
                                  "inf_weight_coarse_trunk", "nan_alpha_linear_coarse", "nan_rgb_linear_coarse", "near_eq_far"])
@pytest.mark.parametrize("D,W,form", I.INSTANTIATIONS[:2], ids=INST_IDS[:2])
def test_sampling_diagnostics_on_non_finite_cases(D, W, form, name):
    """sample_cond / sample_amp / sample_switch = O.sample_pdf_diagnostics on the kernel's own weights_coarse, with the
    tolerances of test_gpu_parity's C3 test (1e-5 and 1e-3 relative, 1e-9 absolute) and the same NaN positions: torch's min /
    max keep a NaN and its searchsorted steps over NaN cdf entries."""
    case = I.BY_NAME[name]
    sd_c, sd_f = I.nets(case, D, W, form)
    rays = case.make_rays()
    t = torch.linspace(0., 1., I.NS)
    z_c = rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t
    z_mid = .5 * (z_c[..., 1:] + z_c[..., :-1])
    r = _renderer(sd_c, sd_f, form)
    problems = []
    try:
        for prec, mode in RAY_MODES:
            r.debug_set_decomposition(mode)
            out = r.render_rays(rays.cuda(), precision=prec, outputs=("weights_coarse", "z_std") + DIAG)
            w = out["weights_coarse"].cpu()
            dg = O.sample_pdf_diagnostics(z_mid, w[..., 1:-1], I.NI)
            for key, k, rel, abs_ in (("min_denom", "sample_cond", 1e-5, 0.0), ("amp", "sample_amp", 1e-3, 0.0), ("switch", "sample_switch", 0.0, 1e-9)):
                if not _same_with_nan(out[k].cpu().numpy(), dg[key].numpy(), rel, abs_):
                    problems.append(f"{name} {_name(prec, mode)} {k}: kernel {out[k].cpu().numpy()[:6]} oracle {dg[key].numpy()[:6]}")
            own = O.sample_pdf(z_mid, w[..., 1:-1], I.NI)
            zs = torch.std(own, dim=-1, unbiased=False).numpy()
            if not np.array_equal(np.isfinite(out["z_std"].cpu().numpy()), np.isfinite(zs)):
                problems.append(f"{name} {_name(prec, mode)} z_std: non-finite positions differ from torch.std of the oracle's samples")
    finally:
        r.debug_set_decomposition(-1)
        r.close()
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------------------------------
# 6. far < near
# ------------------------------------------------------------------------------------------------------------------------

def test_far_below_near_is_refused():
    """With far < near the coarse depths descend and the fine pass's two-way merge (which assumes two ascending lists) cannot
    reproduce the reference's torch.sort (measured: z_fine unsorted in every mode): nwe_render, nwe_create_rays
    and nwe_render_tiled refuse it with NWE_ERR_INVALID (ValueError), the timing ring keeps describing the last launch made,
    and the next valid call renders as if nothing had happened.  near == far and NaN bounds are not refused."""
    case = I.BY_NAME["healthy"]
    sd_c, sd_f = I.nets(case, 8, 256, "folded")
    kw = _frame_kw(case)
    r = _renderer(sd_c, sd_f, "folded", tiles=[0, 0])
    try:
        first = r.parts[0]
        before = first.render(case.pose, I.H, I.W, precision="f16x3", **kw)
        ms, parts = first.last_kernel_ms(), first.last_launch_parts()
        bad = dict(kw, near=6.0, far=2.0)
        for call in (lambda: first.render(case.pose, I.H, I.W, precision="f16x3", **bad),
                     lambda: first.render(case.pose, I.H, I.W, precision="f32", **bad),
                     lambda: first.create_rays(case.pose, I.H, I.W, **bad),
                     lambda: r.render(case.pose, I.H, I.W, precision="f16x3", **bad)):
            with pytest.raises(ValueError, match="far < near"):
                call()
            assert first.last_kernel_ms() == ms and first.last_launch_parts() == parts
        after = first.render(case.pose, I.H, I.W, precision="f16x3", **kw)
        for k in ("rgb", "depth", "acc", "flags"):
            assert torch.equal(before[k], after[k]), k
        first.render(case.pose, I.H, I.W, precision="f16x3", **dict(kw, near=2.0, far=2.0))
        first.render(case.pose, I.H, I.W, precision="f16x3", **dict(kw, near=float("nan")))
        first.create_rays(case.pose, I.H, I.W, **dict(kw, far=float("inf")))
        torch.cuda.synchronize()
    finally:
        r.close()
