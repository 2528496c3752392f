"""Every kernel mode against the fp64 ground truth (oracle/nerf_oracle.py, dtype=torch.float64), with the one criterion of
tests/accuracy.py: max, p99 and median of |kernel - fp64| within FACTOR x those of |fp32 reference - fp64| (+ 1e-7).

The other accuracy tests compare the kernels with another fp32 computation; these measure each mode's own error.  The f32
kernel is held to K32 x the fp32 reference's error, K32 being each test's measured maximum rounded up (1.5 for the network
arithmetic of every instantiation; up to 6 where the compositing's sequential sums, shared by every mode, meet outputs whose
reference error is a few ulps); the f16x3 modes to 1.5 x the larger of the two fp32 paths' errors, capped at K32 x the
reference's (tests/accuracy.py).  Every line printed is one (case, output) with both sides' statistics, their ratios and the
bound; DESIGN.md section 6.1 tabulates them.
"""
import os

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import accuracy as A
from tests import mfma_emulator as E

pytestmark = pytest.mark.gpu

FAR = 10.0
NWE_FLAG_RGB, NWE_FLAG_DEPTH, NWE_FLAG_ACC = 1, 2, 4             # include/nwe.h
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64 = torch.float64
F32 = torch.float32

# every (D, W, form) launch_render_mfma dispatches (nwe_mfma_shapes.h)
FOLDED = [(8, 256), (4, 128), (8, 128), (4, 256), (6, 256), (6, 128)]
REFERENCE = [(8, 256), (4, 128)]
NO_VIEW_DIRS = [(8, 256), (4, 128), (6, 256), (4, 256), (8, 128), (6, 128)]
INSTANTIATIONS = ([(D, W, "folded") for D, W in FOLDED] + [(D, W, "reference") for D, W in REFERENCE] +
                  [(D, W, "no_view_dirs") for D, W in NO_VIEW_DIRS])


def _t(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def _nets(D, W, form, seed):
    """Thin-fog coarse network (well-conditioned importance sampling) and a plain random fine network."""
    if form == "no_view_dirs":
        return (synthetic.thin_fog_output(synthetic.make_state_dict(seed, D, W, use_view_dirs=False)),
                synthetic.make_state_dict(seed + 1, D, W, use_view_dirs=False))
    return synthetic.thin_fog(synthetic.make_state_dict(seed, D, W)), synthetic.make_state_dict(seed + 1, D, W)


def _renderer(sd_c, sd_f, ns, ni, fold=True):
    r = nwe_amd.Renderer(0)
    r.debug_set_fold(fold)
    r.set_network(0, sd_c)
    if sd_f is not None:
        r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    return r


def _scene_rays(n, use_view_dirs=True, stride=1):
    """n rays of the fog scene's 800x800 hor30 frame (tests/golden/e2e_fog.npz)."""
    g = np.load(os.path.join(GOLDEN, "e2e_fog.npz"))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    full = O.create_rays(torch.from_numpy(g["pose"])[None], 800, 800, fx, fy, cx, cy, 0.1, FAR, use_view_dirs)[0]
    return full[torch.from_numpy(g["idx"][::stride][:n])].contiguous()


def _z_coarse(rays, ns):
    t = torch.linspace(0., 1., ns)
    return rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t                     # handler.py:216-218, fp32 as the kernel forms it


def _emulate_x1(sd, fold, rays, z):
    """The single-product arithmetic of the packed stream (tests/mfma_emulator.py, sums in fp64) at the points o + d z."""
    rh = nwe_amd.Renderer(host_only=True)
    rh.debug_set_fold(fold)
    shape = rh.set_network(0, sd)
    novd = "_output_linear.weight" in sd
    D, W = shape[0], shape[1]
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)      # fp32, handler.py:223
    dirs = None if novd else rays[:, None, 8:11].expand(-1, z.shape[1], -1).reshape(-1, 3).numpy()
    y = E.mlp_eval(rh.packed_stream(0), rh.packed_bias(0), rh.packed_scale(0), (pts / 10).numpy(), dirs, D, W, shape[4],
                   three_pass=False, folded=fold and not novd, no_view_dirs=novd)
    rh.close()
    return torch.from_numpy(y.reshape(z.shape[0], z.shape[1], 4))


def _bounds(prec, k32, alt):
    """compare() keywords of a mode: the f32 kernel against the reference alone at K32; f16x3 at FACTOR against the larger of
    the reference's and the f32 kernel's (`alt`) errors, capped at K32 x the reference's."""
    return {"factor": k32} if prec == "f32" else {"y_alt": alt, "alt_cap": k32}


def raw_accuracy(rep, tag, r, rays, sd_c, sd_f, ns, fold=True, modes=(("f16x3", 0), ("f16x3", 1), ("f32", -1)), x1_rays=16, k32=1.5):
    """§ raw network outputs: both oracle networks at the kernel's own sample points (coarse: the linspace depths; fine: the
    kernel's z_fine), so only the network arithmetic is compared, not the sampler."""
    tc, tf = _t(sd_c), _t(sd_f)
    z_c = _z_coarse(rays, ns)
    c32, c64 = A.raw_at_depths(rays, z_c, tc, F32), A.raw_at_depths(rays, z_c, tc, F64)
    cache, flags = {}, {}
    kf = r.render_rays(rays.cuda(), precision="f32", outputs=("raw_coarse", "raw_fine", "z_fine"))    # the fp32 kernel, a yardstick
    for prec, mode in modes:
        r.debug_set_decomposition(mode)
        out = r.render_rays(rays.cuda(), precision=prec, outputs=("raw_coarse", "raw_fine", "z_fine"))
        z_f = out["z_fine"].cpu()
        key = z_f.numpy().tobytes()
        if key not in cache:
            cache[key] = (A.raw_at_depths(rays, z_f, tf, F32), A.raw_at_depths(rays, z_f, tf, F64))
        f32_, f64_ = cache[key]
        name = f"{tag} {prec}" + (f" d{mode}" if mode >= 0 else "")
        kf_fine = kf["raw_fine"]
        if prec != "f32" and not torch.equal(z_f, kf["z_fine"].cpu()):   # the f32 kernel's network at this mode's points
            kf_fine = r.render_rays(rays.cuda(), precision="f32", outputs=("raw_fine",), debug_fine_depths=z_f)["raw_fine"]
        rep.add(f"{name} raw_coarse", out["raw_coarse"], c32, c64, **_bounds(prec, k32, kf["raw_coarse"]))
        rep.add(f"{name} raw_fine", out["raw_fine"], f32_, f64_, **_bounds(prec, k32, kf_fine))
        flags[name] = int(out["flags"].item())
    r.debug_set_decomposition(-1)
    # single product: calibrated against the emulated single-product arithmetic of the same stream at the same points
    n = x1_rays
    out = r.render_rays(rays[:n].cuda(), precision="f16x1", outputs=("raw_coarse", "raw_fine", "z_fine"))
    z_f = out["z_fine"].cpu()
    rep.add(f"{tag} f16x1 raw_coarse (vs emulated x1)", out["raw_coarse"], _emulate_x1(sd_c, fold, rays[:n], z_c[:n]), c64[:n])
    rep.add(f"{tag} f16x1 raw_fine (vs emulated x1)", out["raw_fine"], _emulate_x1(sd_f, fold, rays[:n], z_f),
            A.raw_at_depths(rays[:n], z_f, tf, F64))
    _same_flags(flags)


E2E_MODES = (("f16x3", 0, True), ("f16x3", 0, False), ("f16x3", 1, True), ("f16x3", 1, False), ("f32", -1, False))


def e2e_accuracy(rep, tag, r, rays, sd_c, sd_f, ns, ni, far=FAR, modes=E2E_MODES, k32=1.5):
    """§ end to end: rgb / depth / acc (and z_fine / z_std with importance samples) of every mode against fp64.  Lean renders
    request only rgb / depth / acc (flags are always written), so that the density-only coarse pass runs.  Rays whose last sample sits on the
    alpha step of the 1e10 interval (|sigma_last| < 1e-5 in fp64, model_utils.py:56) are counted and left out."""
    cfg = O.RenderConfig(n_samples=ns, n_importance=ni)
    tc, tf = _t(sd_c), (_t(sd_f) if ni else None)
    ref32 = A.per_ray_outputs(O.render_rays(rays, tc, tf, cfg), ni > 0)
    res64 = O.render_rays(rays, tc, tf, cfg, dtype=F64)
    ref64 = A.per_ray_outputs(res64, ni > 0)
    keep = res64["raw_fine" if ni else "raw_coarse"][:, -1, 3].abs().numpy() > 1e-5
    flags = {}
    kf = r.render_rays(rays.cuda(), precision="f32", outputs=("rgb", "depth", "acc") + (("z_fine", "z_std") if ni else ()))
    for prec, mode, lean in modes:
        r.debug_set_decomposition(mode)
        outs = ("rgb", "depth", "acc") + (() if lean or not ni else ("z_fine", "z_std"))
        got = r.render_rays(rays.cuda(), precision=prec, outputs=outs)
        name = f"{tag} {prec}" + (f" d{mode}" if mode >= 0 else "") + (" lean" if lean else "")
        b = _bounds(prec, k32, kf)
        A.e2e_report(rep, name, got, ref32, ref64, far, keep=keep, alt=b.pop("y_alt", None), **b)
        flags[name] = int(got["flags"].item())
    r.debug_set_decomposition(-1)
    print(f"{tag}: {int((~keep).sum())} of {keep.size} rays left out (last sample on the alpha step)")
    _same_flags(flags)


def _same_flags(flags):
    """Every mode raises the flags the f32 kernel raises (NWE_FLAG_DISP* on rays with acc = 0: the reference's disparity is
    NaN there too, model_utils.py:94); NWE_FLAG_RGB_COARSE is left out (a lean frame computes no coarse colour)."""
    f32 = {v & ~16 for k, v in flags.items() if " f32" in k}
    assert len(f32) <= 1 and all(v & ~16 == next(iter(f32), 0) for v in flags.values()), flags


# ------------------------------------------------------------------------------------------------------------------------
# 1. raw network outputs, every MFMA instantiation
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,W,form", INSTANTIATIONS, ids=[f"{D}x{W}-{f}" for D, W, f in INSTANTIATIONS])
def test_raw_outputs_every_instantiation_against_fp64(D, W, form):
    sd_c, sd_f = _nets(D, W, form, 300 + D + W)
    rays = _scene_rays(64, use_view_dirs=form != "no_view_dirs", stride=29)
    r = _renderer(sd_c, sd_f, 64, 128, fold=form != "reference")
    assert r.mfma_supported(0) and r.mfma_supported(1)
    rep = A.Report()
    raw_accuracy(rep, f"{D}x{W} {form}", r, rays, sd_c, sd_f, 64, fold=form != "reference")
    r.close()
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 2. end to end, well-conditioned scenes
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", ["hor0", "hor30"])
def test_thin_fog_c3_subset_end_to_end_against_fp64(pose):
    g = np.load(os.path.join(GOLDEN, "e2e_c3_subset.npz"))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    full = O.create_rays(torch.from_numpy(g[f"pose_{pose}"])[None], 800, 800, fx, fy, cx, cy, 0.1, FAR)[0]
    rays = full[torch.from_numpy(g[f"idx_{pose}"][::2])].contiguous()              # 2048 of the 4096 rays
    sd_c, sd_f = synthetic.thin_fog(synthetic.make_state_dict(1000, 8, 256)), synthetic.make_state_dict(1001, 8, 256)
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    e2e_accuracy(rep, f"thin-fog C3 {pose}", r, rays, sd_c, sd_f, 64, 128, k32=2.0)           # measured 1.65
    r.close()
    rep.check()


def test_fog_scene_end_to_end_against_fp64():
    rays = _scene_rays(2048)
    sd_c, sd_f = synthetic.thin_fog(synthetic.make_state_dict(1000, 8, 256)), synthetic.make_state_dict(1001, 8, 256)
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    e2e_accuracy(rep, "fog", r, rays, sd_c, sd_f, 64, 128)
    r.close()
    rep.check()


def test_c1_end_to_end_against_fp64():
    g = np.load(os.path.join(GOLDEN, "e2e_c1.npz"))
    fx, fy, cx, cy = O.intrinsics(64, 64)
    rays = O.create_rays(torch.from_numpy(g["pose"])[None], 64, 64, fx, fy, cx, cy, 0.1, FAR)[0].contiguous()
    sd = synthetic.make_state_dict(1000, 4, 128)
    r = _renderer(sd, None, 32, 0)
    rep = A.Report()
    e2e_accuracy(rep, "C1", r, rays, sd, None, 32, 0)
    r.close()
    rep.check()


def test_randomised_sampling_configurations_against_fp64():
    """The ten configurations of test_gpu_parity.test_randomised_sampling_configurations_against_live_oracle (same rays)."""
    rng = np.random.default_rng(20240)
    sd_c = synthetic.thin_fog(synthetic.make_state_dict(1000, 8, 256))
    sd_f = synthetic.make_state_dict(1001, 8, 256)
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    for ns, ni, near, far, n_rays in [(3, 5, 0.1, 10.0, 70), (5, 1, 0.5, 4.0, 33), (64, 256, 0.1, 10.0, 45), (17, 40, 0.05, 6.0, 129),
                                      (33, 2, 1.0, 2.0, 64), (64, 0, 0.1, 10.0, 50), (4, 0, 0.1, 10.0, 31),
                                      (128, 128, 0.1, 10.0, 61), (65, 7, 0.2, 5.0, 40), (100, 0, 0.1, 10.0, 33)]:
        r.set_sampling(ns, ni)
        o = rng.uniform(-1.0, 1.0, (n_rays, 3)).astype(np.float32)
        d = (rng.normal(size=(n_rays, 3)) * rng.uniform(0.2, 3.0, (n_rays, 1))).astype(np.float32)
        v = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays = torch.from_numpy(np.concatenate([o, d, np.full((n_rays, 1), near, np.float32), np.full((n_rays, 1), far, np.float32),
                                                v.astype(np.float32)], 1))
        e2e_accuracy(rep, f"random {ns}+{ni}", r, rays, sd_c, sd_f if ni else None, ns, ni, far=far,
                     k32=6.0 if ni == 0 else 3.0)           # measured: 64+0 acc 5.0 (median 1.2e-7 vs 3e-9); see DESIGN.md 6.1
    r.close()
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 3. the bench scene, measured both ways
# ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bench_scene():
    """The 2 x 4096 rays of e2e_c3_subset.npz with the bench networks (two unrelated random 8x256 networks, 64+128): the fp32
    and fp64 oracle once per module."""
    g = np.load(os.path.join(GOLDEN, "e2e_c3_subset.npz"))
    fx, fy, cx, cy = O.intrinsics(800, 800)
    sd_c, sd_f = synthetic.make_state_dict(1000, 8, 256), synthetic.make_state_dict(1001, 8, 256)
    rays, ref32, ref64 = [], [], []
    for pose in ("hor0", "hor30"):
        full = O.create_rays(torch.from_numpy(g[f"pose_{pose}"])[None], 800, 800, fx, fy, cx, cy, 0.1, FAR)[0]
        rr = full[torch.from_numpy(g[f"idx_{pose}"])].contiguous()
        rays.append(rr)
        keep = ("rgb_fine", "depth_fine", "raw_fine")
        ref32.append(O.render_rays(rr, _t(sd_c), _t(sd_f), O.RenderConfig(), keep=keep))
        ref64.append(O.render_rays(rr, _t(sd_c), _t(sd_f), O.RenderConfig(), keep=keep, dtype=F64))
    cat = lambda parts, k: torch.cat([p[k] for p in parts], 0)
    return {"rays": torch.cat(rays, 0), "sd_c": sd_c, "sd_f": sd_f,
            "rgb32": cat(ref32, "rgb_fine").double(), "depth32": cat(ref32, "depth_fine").double(),
            "rgb64": cat(ref64, "rgb_fine"), "depth64": cat(ref64, "depth_fine")}


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bench_scene_against_fp64(bench_scene, precision):
    """Unrelated random networks: the reference's importance sampling is ill conditioned on ~1 % of the rays, where the fp32
    reference itself is > 1e-4 from fp64.  Per ray, the kernel must not be worse than the reference:
    the count of rays > 1e-4 from fp64 at most 1.5x the reference's (+ 3), p99 at most 1.5x, and on the rays where kernel
    and reference disagree by > 1e-4, the kernel at least as close to fp64 on >= 40 % of them."""
    b = bench_scene
    r = _renderer(b["sd_c"], b["sd_f"], 64, 128)
    got = r.render_rays(b["rays"].cuda(), precision=precision, outputs=("rgb", "depth", "acc"))
    r.close()
    rows, failed = [], []
    for key, scale in (("rgb", 1.0), ("depth", FAR)):
        k = got[key].cpu().double()
        e_k = ((k - b[key + "64"]).abs() / scale).reshape(k.shape[0], -1).max(-1).values.numpy()
        e_r = ((b[key + "32"] - b[key + "64"]).abs() / scale).reshape(k.shape[0], -1).max(-1).values.numpy()
        d_kr = ((k - b[key + "32"]).abs() / scale).reshape(k.shape[0], -1).max(-1).values.numpy()
        n_k, n_r = int((e_k > 1e-4).sum()), int((e_r > 1e-4).sum())
        p_k, p_r = float(np.percentile(e_k, 99)), float(np.percentile(e_r, 99))
        disagree = d_kr > 1e-4
        closer = float((e_k[disagree] <= e_r[disagree]).mean()) if disagree.any() else 1.0
        rows.append(f"bench {precision} {key:<5s} rays > 1e-4 from fp64: kernel {n_k} ref32 {n_r} | p99 kernel {p_k:.2e} ref32 "
                    f"{p_r:.2e} | max kernel {e_k.max():.2e} ref32 {e_r.max():.2e} | |kernel - ref32| > 1e-4 on {int(disagree.sum())} "
                    f"rays, kernel at least as close to fp64 on {closer:.0%}")
        if n_k > 1.5 * n_r + 3:
            failed.append(f"{key}: {n_k} rays > 1e-4 vs the reference's {n_r}")
        if p_k > 1.5 * p_r + A.FLOOR:
            failed.append(f"{key}: p99 {p_k:.2e} vs the reference's {p_r:.2e}")
        if closer < 0.4:
            failed.append(f"{key}: kernel closer on only {closer:.0%} of the disagreeing rays")
    print("\n".join(rows))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------
# 4. trained-like weight statistics
# ------------------------------------------------------------------------------------------------------------------------

# K32 (raw, end to end) per weight set, the measured maxima over 8x256 and 4x128 rounded up: raw 2.25 for the
# layer scales (the f32 kernel's FMA chains at raw values ~0.4), end to end 5.4 for the outlier (acc of saturated rays, the
# compositing's sequential sum) and 2.6 for heavy tails
TRAINED_K32 = {"layer_scales": (2.5, 1.5), "bias300": (2.0, 1.5), "bias3000": (2.0, 1.5), "outlier": (1.5, 6.0), "student_t": (1.5, 3.0)}


@pytest.mark.parametrize("kind", A.WEIGHT_SETS)
@pytest.mark.parametrize("D,W", [(8, 256), (4, 128)])
def test_trained_like_weight_statistics_against_fp64(D, W, kind):
    sd_c = synthetic.thin_fog(A.weight_set(synthetic.make_state_dict(500 + D, D, W), kind))
    sd_f = A.weight_set(synthetic.make_state_dict(501 + D, D, W), kind)
    rays = _scene_rays(64, stride=31)
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    raw_accuracy(rep, f"{D}x{W} {kind}", r, rays, sd_c, sd_f, 64, modes=(("f16x3", 0), ("f32", -1)), k32=TRAINED_K32[kind][0])
    e2e_accuracy(rep, f"{D}x{W} {kind}", r, _scene_rays(256, stride=7), sd_c, sd_f, 64, 128,
                 modes=(("f16x3", 0, True), ("f16x3", 1, False), ("f32", -1, False)), k32=TRAINED_K32[kind][1])
    r.close()
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the fp16 range edge of the split activations
# ------------------------------------------------------------------------------------------------------------------------

def _edge(sd, value, n=4):
    """n first-layer units driven to about `value` (their pre-activation is `value` + O(1))."""
    out = {k: v.copy() for k, v in sd.items()}
    out["_pts_linears.0.bias"][5:5 + n] = np.float32(value)
    return out


@pytest.mark.parametrize("D,W", [(8, 256), (4, 128)])
def test_activations_near_the_fp16_limit_against_fp64(D, W):
    """Hidden activations in [2^15, 65504]: hi = fp16(v) is finite, lo carries the rest; the §2 criterion holds."""
    sd_c = synthetic.thin_fog(_edge(synthetic.make_state_dict(600 + D, D, W), 40000.0))
    sd_f = _edge(synthetic.make_state_dict(601 + D, D, W), 40000.0)
    rays = _scene_rays(64, stride=37)
    tf = _t(sd_f)
    with torch.no_grad():                   # the premise: the fine network's first layer does reach [2^15, 65504] here
        h0 = torch.relu(torch.nn.functional.linear(O.embed(rays[:, :3], 10, 10), tf["_pts_linears.0.weight"], tf["_pts_linears.0.bias"]))
    assert 2.0 ** 15 <= h0.max().item() <= 65504, h0.max().item()
    r = _renderer(sd_c, sd_f, 64, 128)
    rep = A.Report()
    raw_accuracy(rep, f"{D}x{W} activations ~4e4", r, rays, sd_c, sd_f, 64, modes=(("f16x3", 0), ("f16x3", 1), ("f32", -1)),
                 k32=2.0)                                                                   # measured 1.51
    e2e_accuracy(rep, f"{D}x{W} activations ~4e4", r, rays, sd_c, sd_f, 64, 128,
                 modes=(("f16x3", 0, True), ("f16x3", 1, False), ("f32", -1, False)), k32=2.0)
    r.close()
    rep.check()


@pytest.mark.parametrize("which", ["coarse", "fine", "both"])
@pytest.mark.parametrize("D,W", [(8, 256), (4, 128)])
def test_activations_beyond_fp16_range_are_never_silently_wrong(D, W, which):
    """Hidden activations >= 65520 round to hi = inf.  An f16x3 render must never return a finite, wrong result: every ray whose
    rgb / depth / acc are all finite must agree with fp64 as closely as the fp32 kernel does (the §2 criterion with the f32
    kernel as the yardstick), and if any ray is not finite the render must raise an NWE_FLAG_RGB / DEPTH / ACC bit that the
    fp32 kernel did not (include/nwe.h, "fp16 range").  Lean and full renders, both decompositions."""
    base_c, base_f = synthetic.thin_fog(synthetic.make_state_dict(700 + D, D, W)), synthetic.make_state_dict(701 + D, D, W)
    sd_c = synthetic.thin_fog(_edge(synthetic.make_state_dict(700 + D, D, W), 70000.0)) if which != "fine" else base_c
    sd_f = _edge(synthetic.make_state_dict(701 + D, D, W), 70000.0) if which != "coarse" else base_f
    rays = _scene_rays(64, stride=41)
    r = _renderer(sd_c, sd_f, 64, 128)
    res64 = O.render_rays(rays, _t(sd_c), _t(sd_f), O.RenderConfig(), dtype=F64)
    keep = res64["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    y64 = A.per_ray_outputs(res64, True)
    ref = r.render_rays(rays.cuda(), precision="f32", outputs=("rgb", "depth", "acc", "z_fine"))
    assert all(torch.isfinite(ref[k]).all().item() for k in ("rgb", "depth", "acc")), "the fp32 kernel has no fp16 range limit"
    ref_flags = int(ref["flags"].item())
    problems = []
    for mode, lean in ((0, True), (0, False), (1, True), (1, False)):
        r.debug_set_decomposition(mode)
        outs = ("rgb", "depth", "acc") + (() if lean else ("z_fine", "raw_fine"))
        got = r.render_rays(rays.cuda(), precision="f16x3", outputs=outs)
        flag = int(got["flags"].item())
        new = flag & ~ref_flags & (NWE_FLAG_RGB | NWE_FLAG_DEPTH | NWE_FLAG_ACC)
        finite = (torch.isfinite(got["rgb"]).all(-1) & torch.isfinite(got["depth"]) & torch.isfinite(got["acc"])).cpu().numpy()
        tag = f"{D}x{W} {which} > 65520 d{mode}{' lean' if lean else ''}"
        print(f"{tag}: flags 0x{flag:x} (f32 kernel 0x{ref_flags:x}), {int(finite.sum())} of {finite.size} rays finite")
        rep = A.Report()
        if (keep & finite).any():
            A.e2e_report(rep, tag + " finite rays", got, ref, y64, FAR, keep=keep & finite,
                         keys=("rgb", "depth", "acc") + (() if lean else ("z_fine",)))
        if rep.failed:
            problems.append(f"{tag}: rays with finite outputs are wrong:\n" + "\n".join(rep.failed))
        if not finite.all() and not new:
            problems.append(f"{tag}: {int((~finite).sum())} rays not finite and no NWE_FLAG_RGB / DEPTH / ACC bit of its own "
                            f"(flags 0x{flag:x}, f32 kernel 0x{ref_flags:x})")
    r.close()
    assert not problems, "\n".join(problems)
