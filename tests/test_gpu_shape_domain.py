"""The fp32 kernel (NWE_PREC_F32) over the legal network-shape domain, case by case from tests/shape_domain.py, against the fp64
oracle under the one criterion of tests/accuracy.py: it is the yardstick of every f16x3 comparison and the path of every legal
YAML whose shape the MFMA kernels have no instantiation for, so it is held to fp64 wherever nwe_set_network lets a caller go.

Per case: the raw network outputs at the kernel's own sample points, every per-ray output of a full and of a lean request, the
endpoint feature map where the case asks for it; the MFMA precisions refuse and leave the context as it was; ragged ray counts
are prefixes of one another; the handler picks "f32" for two MFMA shapes that differ; and two networks with different encodings
are refused.  Each bound starts at A.FACTOR; a case whose f32 kernel measures above it carries its own K32 below (its measured
maximum ratio rounded up to the next 0.5, never above 6), and DESIGN.md section 6.1 tabulates every ratio.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import accuracy as A
from tests import shape_domain as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
RGB_TOL = 1e-4                                    # tests/test_gpu_parity.py
FLAG_DISP, FLAG_DISP_COARSE = 8, 128              # include/nwe.h: the only bits a finite render may raise (acc = 0 on a ray)
LEAN = ("rgb", "depth", "acc")
COARSE = ("rgb_coarse", "depth_coarse", "acc_coarse")

# K32 (raw, end to end) of the cases whose f32 kernel measures above A.FACTOR = 1.5 x the fp32 reference's error on an MI355X
# (the factor a statistic needs with the 1e-7 floor taken into account, as DESIGN.md tabulates it).  All of them end to end, none
# in the network arithmetic: the compositing's sequential fp32 sums against torch's blocked ones, over 37 rays, where max and
# p99 are single rays.
K32 = {
    "7x32-skip5": (1.5, 6.0),        # measured 5.74: acc, the median ray saturates (1 + 2^-23 for the reference's 1.0; 1.17e-7 vs 3.0e-9)
    "8x256-noskip": (1.5, 2.5),      # measured 2.01: depth max (8.3e-6 vs 4.1e-6 of far)
    "4x128-skip1": (1.5, 3.0),       # measured 2.90: depth max (4.4e-6 vs 1.5e-6 of far)
    "8x256-freqs9": (1.5, 2.0),      # measured 1.89: depth max
    "2x8-128+256": (1.5, 4.0),       # measured 3.65: acc_coarse, a sequential sum of 128 weights (3.5e-7 vs 6.8e-8); rgb 3.52
}


def _k32(name):
    return K32.get(name, (A.FACTOR, A.FACTOR))


def _renderer(b):
    r = nwe_amd.Renderer(0)
    r.set_network(0, b.sd_c)
    if b.sd_f is not None:
        r.set_network(1, b.sd_f)
    r.set_sampling(b.case.ns, b.case.ni)
    r.set_white_background(b.case.white_background)
    return r


def _full(case):
    return LEAN + ((("z_fine", "z_std") + COARSE) if case.ni else COARSE) + (("feat_map",) if case.feat_map else ())


def _z_coarse(rays, ns):
    t = torch.linspace(0., 1., ns)
    return rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t                     # handler.py:216-218, fp32 as the kernel forms it


def _only_disp_flags(out):
    return int(out["flags"].item()) & ~(FLAG_DISP | FLAG_DISP_COARSE) == 0


# ------------------------------------------------------------------------------------------------------------------------
# 1. raw network outputs at the kernel's own sample points
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_raw_outputs_against_fp64(name):
    """raw_coarse at the linspace depths and raw_fine at the kernel's own z_fine, so that the network arithmetic alone is
    compared.  With more than ten frequencies (2^14 x / 10) the rounding of the point is the whole of the plain fp64
    difference, so the ground truth is fp64 at the reference's fp32 points (tests/accuracy.raw_at_depths)."""
    b, _, _ = S.reference(name)
    case, cfg = b.case, b.case.config()
    at_fp32_points = case.freqs_xyz > 10
    r = _renderer(b)
    got = r.render_rays(b.rays.cuda(), precision="f32", outputs=("raw_coarse",) + (("raw_fine", "z_fine") if case.ni else ()))
    r.close()
    rep = A.Report()
    z_c = _z_coarse(b.rays, case.ns)
    tc = S.tensors(b.sd_c)
    rep.add(f"{name} f32 raw_coarse", got["raw_coarse"], A.raw_at_depths(b.rays, z_c, tc, F32, cfg, at_fp32_points),
            A.raw_at_depths(b.rays, z_c, tc, F64, cfg, at_fp32_points), factor=_k32(name)[0])
    if case.ni:
        z_f, tf = got["z_fine"].cpu(), S.tensors(b.sd_f)
        assert (z_f[:, 1:] >= z_f[:, :-1]).all() and z_f.shape == (S.N_RAYS, case.ns + case.ni)
        rep.add(f"{name} f32 raw_fine", got["raw_fine"], A.raw_at_depths(b.rays, z_f, tf, F32, cfg, at_fp32_points),
                A.raw_at_depths(b.rays, z_f, tf, F64, cfg, at_fp32_points), factor=_k32(name)[0])
    assert _only_disp_flags(got)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 2. end to end
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_end_to_end_against_fp64(name):
    """rgb / depth / acc / z_fine / z_std and the coarse rgb / depth / acc of a full request, rgb / depth / acc of a lean one
    (the same bits), the endpoint feature map against the oracle's feat_map_fine.  Rays whose last sample sits on the alpha step
    of the 1e10 interval (|sigma_last| < 1e-5 in fp64) are left out as in tests/test_gpu_accuracy.e2e_accuracy (none here:
    tests/test_shape_domain_oracle.py).  With more than ten frequencies the fine outputs are a chaotic function of 1e-6 depth
    differences: the coarse outputs alone are compared."""
    b, res32, res64 = S.reference(name)
    case = b.case
    fine = case.ni > 0
    k32 = _k32(name)[1]
    ref32, ref64 = A.per_ray_outputs(res32, fine), A.per_ray_outputs(res64, fine)
    keep = res64["raw_fine" if fine else "raw_coarse"][:, -1, 3].abs().numpy() > 1e-5
    keep_c = res64["raw_coarse"][:, -1, 3].abs().numpy() > 1e-5
    r = _renderer(b)
    full = r.render_rays(b.rays.cuda(), precision="f32", outputs=_full(case))
    lean = r.render_rays(b.rays.cuda(), precision="f32", outputs=LEAN)
    r.close()
    rep = A.Report()
    for tag, got in (("full", full), ("lean", lean)):
        if case.freqs_xyz <= 10:
            A.e2e_report(rep, f"{name} f32 {tag}", got, ref32, ref64, S.FAR, keep=keep, factor=k32)
        for k in COARSE:
            if k in got:
                rep.add(f"{name} f32 {tag} {k}", got[k], res32[k], res64[k], scale=S.FAR if k == "depth_coarse" else 1.0, keep=keep_c,
                        factor=k32)
        if "feat_map" in got:
            half = case.fine.W // 2          # the reference composites raw[..., -128:]: for W/2 < 128 the view layer's outputs are its tail
            assert got["feat_map"].shape == (S.N_RAYS, half)
            rep.add(f"{name} f32 {tag} feat_map", got["feat_map"], res32["feat_map_fine"][:, -half:], res64["feat_map_fine"][:, -half:],
                    keep=keep, factor=k32)
        assert _only_disp_flags(got), hex(int(got["flags"].item()))
    print(f"{name}: {int((~keep).sum())} of {keep.size} rays left out (last sample on the alpha step)")
    for k in LEAN:
        assert torch.equal(full[k], lean[k]), k
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# 3. dispatch
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_mfma_precisions_refuse_and_leave_the_f32_render_alone(name):
    b = S.build(S.BY_NAME[name])
    case = b.case
    r = _renderer(b)
    assert [r.mfma_supported(w) for w in range(2 if case.ni else 1)] == list(case.mfma[:2 if case.ni else 1])
    rays = b.rays.cuda()
    before = r.render_rays(rays, precision="f32", outputs=_full(case))
    for prec in ("f16x3", "f16x1"):
        for outs in (LEAN, tuple(o for o in _full(case) if o != "feat_map")):
            with pytest.raises(NotImplementedError):
                r.render_rays(rays, precision=prec, outputs=outs)
    after = r.render_rays(rays, precision="f32", outputs=_full(case))
    r.close()
    for k in _full(case) + ("flags",):
        assert torch.equal(before[k], after[k]), k


def test_refused_configuration_leaves_the_context_rendering():
    """Networks and samplings just outside the domain (tests/test_shape_domain_oracle.py walks the borders on a host-only
    context) are refused on a device context too, and the next render is what it was."""
    b = S.build(S.BY_NAME["c8x256-f2x16"])
    r = _renderer(b)
    rays, outs = b.rays.cuda(), _full(b.case)
    before = r.render_rays(rays, precision="f32", outputs=outs)
    for which in (0, 1):
        for kw in (dict(D=17, W=8), dict(D=2, W=258), dict(D=2, W=8, in_xyz=99), dict(D=2, W=8, in_dir=69)):
            with pytest.raises(NotImplementedError):
                r.set_network(which, synthetic.make_state_dict(3, **kw))
        with pytest.raises(ValueError, match="more than one skip"):
            r.set_network(which, synthetic.make_state_dict(3, 5, 16, skips=(1, 3)))
    for ns, ni, exc in ((1, 0, NotImplementedError), (129, 0, NotImplementedError), (16, 257, NotImplementedError), (2, 4, ValueError)):
        with pytest.raises(exc):
            r.set_sampling(ns, ni)
    after = r.render_rays(rays, precision="f32", outputs=outs)
    r.close()
    for k in outs + ("flags",):
        assert torch.equal(before[k], after[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# 4. the handler
# ------------------------------------------------------------------------------------------------------------------------

def test_handler_renders_two_mfma_shapes_that_differ_with_f32(capsys):
    """net_depth / net_width 4 x 128 and net_depth_fine / net_width_fine 8 x 256 (handler.py:42-45,106-119): each has an MFMA
    instantiation, the pair has none; "auto" picks the fp32 kernel, says so, and renders the live oracle's image."""
    b = S.build(S.BY_NAME["c4x128-f8x256"])
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "unused")
    h.initialize_models(state_dicts=(b.sd_c, b.sd_f))
    said = capsys.readouterr().out
    assert h._precision == "f32" and "no MFMA instantiation" in said
    assert h.renderer.mfma_supported(0) and h.renderer.mfma_supported(1)
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    got = h.render(pose[0].numpy(), S.FRAME_H, S.FRAME_W)["rgb"].reshape(-1, 3).cpu().numpy()[:S.N_RAYS]
    ref = O.render_rays(b.rays, S.tensors(b.sd_c), S.tensors(b.sd_f), O.RenderConfig())           # the YAML's 64 + 128
    ok = ref["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    assert ok.mean() >= 0.95 and np.abs(got - ref["rgb_fine"].numpy())[ok].max() <= RGB_TOL


def test_handler_renders_two_shapes_without_view_dirs(tmp_path, monkeypatch, capsys):
    import yaml
    name = "novd-c4x128-f6x64"
    b, res32, _ = S.reference(name)
    case = b.case
    cfg = {k: dict(v) for k, v in nwe_amd.config.INFERENCE_DEFAULTS.items()}
    cfg["rendering"].update(use_view_dirs=False, n_samples=case.ns, n_importance=case.ni)
    cfg["experiment"].update(image_width=S.FRAME_W, image_height=S.FRAME_H)
    with open(tmp_path / "office_tokyo_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setenv("NWE_CONFIG_DIR", str(tmp_path))
    h = nwe_amd.NeRFReplicaInferenceHandler("office_tokyo", "synthetic")
    h.initialize_models(state_dicts=(b.sd_c, b.sd_f))
    assert h._precision == "f32" and "no MFMA instantiation" in capsys.readouterr().out
    ok = res32["raw_fine"][:, -1, 3].abs().numpy() > 1e-5
    res = h._render_rays(b.rays.cuda())
    assert np.abs(res["rgb_fine"].cpu().numpy() - res32["rgb_fine"].numpy())[ok].max() <= RGB_TOL
    assert np.abs(res["rgb_coarse"].cpu().numpy() - res32["rgb_coarse"].numpy()).max() <= RGB_TOL
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    frame = h.render(pose[0].numpy())["rgb"].reshape(-1, 3).cpu().numpy()[:S.N_RAYS]
    assert np.abs(frame - res32["rgb_fine"].numpy())[ok].max() <= RGB_TOL


# ------------------------------------------------------------------------------------------------------------------------
# 5. ragged work
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.RAGGED_CASES)
def test_ray_counts_around_the_workgroup_size_are_prefixes_of_one_another(name):
    """A workgroup owns 16 rays and pads a ragged packet with copies of the call's last ray: 1, 15, 16, 17 and 37 rays give the
    same bits for the rays they share."""
    b = S.build(S.BY_NAME[name])
    outs = _full(b.case) + ("raw_coarse", "raw_fine")
    r = _renderer(b)
    whole = r.render_rays(b.rays.cuda(), precision="f32", outputs=outs)
    for n in S.RAGGED_COUNTS:
        part = r.render_rays(b.rays[:n].cuda(), precision="f32", outputs=outs)
        for k in outs:
            assert part[k].shape[0] == n and torch.equal(part[k], whole[k][:n]), (n, k)
    r.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. the two networks share their encodings
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse,fine", [((63, 15), (63, 27)), ((63, 27), (63, 15)), ((27, 27), (63, 27)), ((63, 27), (27, 27))],
                         ids=["in_dir-15-27", "in_dir-27-15", "in_xyz-27-63", "in_xyz-63-27"])
def test_networks_with_different_encodings_are_refused(coarse, fine):
    """One Embedding serves both networks in the reference (handler.py:93-103) and the kernels encode a ray's view direction
    once, with the coarse network's in_dir: a fine network with a wider one would read encoding rows nobody wrote.  Every render
    entry point refuses the pair with NWE_ERR_STATE while importance samples are on; the coarse pass alone, and the pair once
    its encodings agree, render what a fresh context renders."""
    mk = lambda seed, enc: synthetic.make_state_dict(seed, 2, 16, in_xyz=enc[0], in_dir=enc[1], skips=())
    rays = S.frame_rays().cuda()
    r, fresh = nwe_amd.Renderer(0), nwe_amd.Renderer(0)
    r.set_network(0, synthetic.thin_fog(mk(60, coarse)))
    r.set_network(1, mk(61, fine))
    r.set_sampling(8, 8)
    fx, fy, cx, cy = O.intrinsics(S.FRAME_H, S.FRAME_W)
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))[0].numpy()
    for prec in ("f32", "f16x3"):
        with pytest.raises(RuntimeError, match=f"share their encodings: in_xyz {coarse[0]} / {fine[0]}, in_dir {coarse[1]} / {fine[1]}"):
            r.render_rays(rays, precision=prec)
        with pytest.raises(RuntimeError, match="share their encodings"):
            r.render(pose, S.FRAME_H, S.FRAME_W, fx=fx, fy=fy, cx=cx, cy=cy, near=S.NEAR, far=S.FAR, precision=prec)
    assert r.last_kernel_ms() < 0                                    # nothing was launched
    outs = LEAN + ("z_fine", "raw_fine")
    r.set_sampling(8, 0)                                             # the coarse pass alone never reads the fine network
    fresh.set_network(0, synthetic.thin_fog(mk(60, coarse)))
    fresh.set_sampling(8, 0)
    a, c = r.render_rays(rays, precision="f32", outputs=LEAN), fresh.render_rays(rays, precision="f32", outputs=LEAN)
    assert all(torch.equal(a[k], c[k]) and torch.isfinite(a[k]).all() for k in LEAN)
    r.set_network(1, mk(62, coarse))                                 # the pair with one encoding
    r.set_sampling(8, 8)
    fresh.set_network(1, mk(62, coarse))
    fresh.set_sampling(8, 8)
    a, c = r.render_rays(rays, precision="f32", outputs=outs), fresh.render_rays(rays, precision="f32", outputs=outs)
    assert all(torch.equal(a[k], c[k]) and torch.isfinite(a[k]).all() for k in outs)
    r.close(); fresh.close()
