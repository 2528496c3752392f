"""The case table of tests/input_domain.py against the CPU oracle alone (no GPU): the hand-written expectations are checked
against the reference's behaviour here, so that tests/test_gpu_input_domain.py compares the kernels with something that was
never derived from them; the fp64-at-fp32-points ground truth of tests/accuracy.raw_at_depths is pinned; and the bound of the
wide positional-encoding sweep of nwe_selftest (report[7]) is derived from the reference's own sinf.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import accuracy as A
from tests import input_domain as I

F32, F64 = torch.float32, torch.float64
MAX_LEFT_OUT = 0.05          # share of a case's rays the alpha-step rule may leave out of a value comparison


def _forms(case):
    return [(8, 256, "folded")] + ([(8, 256, "no_view_dirs")] if case.expect_novd is not None or case.spoil_novd is not None else [])


@pytest.mark.parametrize("name", [c.name for c in I.CASES])
def test_expectation_is_what_the_reference_does(name):
    case = I.BY_NAME[name]
    for D, W, form in _forms(case):
        rays, _, _, res = I.run_oracle(case, D, W, form)
        masks = I.oracle_masks(res, True)
        expect = case.expectation(form)
        assert set(expect) <= set(I.OUTPUTS)
        for k in I.OUTPUTS:
            acc = res["acc_coarse" if k in I.COARSE_SIDE else "acc_fine"]
            want = I.expected_ray_mask(expect.get(k), rays.shape[0], acc)
            got = I.ray_mask(masks[k])
            assert np.array_equal(got, want), (name, form, k, np.nonzero(got)[0].tolist(), np.nonzero(want)[0].tolist())
        res64 = I.run_oracle(case, D, W, form, F64)[3]
        masks64 = I.oracle_masks(res64, True)
        same = all(np.array_equal(masks[k], masks64[k]) for k in I.OUTPUTS)
        if case.f32_overflow:      # the fp32 product x / 10 * 2^9 is inf and sin(inf) NaN; in fp64 it is an ordinary number
            assert not same and not any(m.any() for k, m in masks64.items() if not k.startswith("disp"))
        else:
            assert same, (name, form, [k for k in I.OUTPUTS if not np.array_equal(masks[k], masks64[k])])
        # the flag word of a full and of a lean request
        full = I.expected_flags(res, I.FULL, True)
        lean = I.expected_flags(res, I.LEAN, True, density_only=form == "folded")
        assert lean == full & ~(I.FLAG_RAW | I.FLAG_ZSTD) & ~(I.FLAG_RGB_COARSE if form == "folded" else 0)
        if case.density_only_sees_nothing and form == "folded":
            assert full & I.FLAG_RGB_COARSE and lean == 0, (hex(full), hex(lean))
        if not any(v for v in expect.values() if v != I.ACC0) and not (res["acc_fine"] == 0).any() and not (res["acc_coarse"] == 0).any():
            assert full == 0
        if case.values or name in I.SWEEP_CASES:
            left_out = (res64["raw_fine"][:, -1, 3].abs() < 1e-5).float().mean().item()
            left_out_c = (res64["raw_coarse"][:, -1, 3].abs() < 1e-5).float().mean().item()
            assert max(left_out, left_out_c) <= MAX_LEFT_OUT, (name, left_out, left_out_c)


def test_poisoned_rays_leave_their_neighbours_alone():
    """The table's healthy rays are the same bits with and without the poisoned ones, and in the oracle (ray-wise by
    construction) their outputs do not change: the premise of the GPU test's bit-identity."""
    bad, good = I.poisoned_rays(), I.poisoned_rays(healthy_only=True)
    assert torch.equal(I.poisoned_rays(n=I.BIG_RAYS)[:I.POISON_RAYS][list(I.POISON)].isfinite(), bad[list(I.POISON)].isfinite())
    healthy = np.array([i for i in range(I.POISON_RAYS) if i not in I.POISON])
    assert torch.equal(bad[healthy], good[healthy]) and torch.isfinite(good).all()
    assert all(not torch.isfinite(bad[i]).all() or I.POISON[i] in ("zero_dir", "underflow_dir") for i in I.POISON)
    case = I.BY_NAME["poisoned_neighbours"]
    sd_c, sd_f = I.nets(case, 8, 256, "folded")
    cfg = O.RenderConfig(n_samples=I.NS, n_importance=I.NI)
    a = O.render_rays(bad, I.tensors(sd_c), I.tensors(sd_f), cfg)
    b = O.render_rays(good, I.tensors(sd_c), I.tensors(sd_f), cfg)
    for k in ("rgb_fine", "depth_fine", "acc_fine", "z_std", "raw_fine", "z_fine"):
        assert torch.equal(a[k][healthy], b[k][healthy]), k


def test_far_below_near_is_sorted_by_the_reference():
    """far < near: the coarse depths descend, the reference's torch.sort(cat(...)) (handler.py:243) still returns ascending
    fine depths and finite outputs.  A two-way merge of two descending lists cannot: nwe_render / nwe_create_rays /
    nwe_render_tiled refuse far < near and nwe_render_rays states near <= far as a precondition (include/nwe.h)."""
    case = I.Case("far_below_near", {}, pose=I._pose(), near=6.0, far=2.0)
    rays, _, _, res = I.run_oracle(case, 8, 256, "folded")
    assert (res["z_coarse"][:, 1:] < res["z_coarse"][:, :-1]).all()
    assert (res["z_fine"][:, 1:] >= res["z_fine"][:, :-1]).all()
    assert all(torch.isfinite(res[k]).all() for k in ("rgb_fine", "depth_fine", "acc_fine", "z_std"))


# ------------------------------------------------------------------------------------------------------------------------
# fp64 at the reference's fp32 points
# ------------------------------------------------------------------------------------------------------------------------

def _z(rays, ns=I.NS):
    t = torch.linspace(0., 1., ns)
    return rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t


def test_fp64_at_fp32_points_is_the_fp64_network_on_the_references_own_inputs():
    """raw_at_depths(fp32_points=True): bit-equal to encoding + MLP written out in fp64 on v = fp32(fp32(o + d z) / 10)."""
    case = I.BY_NAME["origin_1000"]
    sd_c, _ = I.nets(case, 8, 256, "folded")
    state = I.tensors(sd_c)
    rays = case.make_rays()
    z = _z(rays)
    got = A.raw_at_depths(rays, z, state, F64, fp32_points=True)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    v = (pts / 10.0).reshape(-1, 3)
    assert v.dtype == F32
    enc = torch.cat([O.embed(v.to(F64), 10, 1.0), O.embed(rays[:, None, 8:11].expand(pts.shape).reshape(-1, 3).to(F64), 4, 1.0)], -1)
    with torch.no_grad():
        want = O.mlp_forward(O.cast_state(state, F64), enc).reshape(got.shape)
    assert torch.equal(got, want)
    # and in fp32 the option changes nothing: the reference's own path
    assert torch.equal(A.raw_at_depths(rays, z, state, F32, fp32_points=True), A.raw_at_depths(rays, z, state, F32))


@pytest.mark.parametrize("name", ["healthy", "origin_1", "origin_22"])
def test_fp64_at_fp32_points_agrees_with_fp64_at_scene_size(name):
    """At scene-sized coordinates the two ground truths differ by the rounding of the point alone (o + d z and / 10 in fp32).
    That difference (measured on max: 6.5e-6 on the pinhole frame, 9.0e-6 and 1.9e-5 at origins of 1 and 22) is one part of
    the fp32 reference's own error, so no statistic of it exceeds 1.25 x that of
    |fp32 reference - fp64| (measured 0.77 .. 1.01 on two hosts - the reference's fp32 sums differ between hosts, so no lower
    bound is asserted), and what is left of the fp32 reference's error against the new ground truth - its arithmetic alone -
    is smaller than its error against the old one (measured 4e-7 .. 6e-7 of 7e-6 .. 2e-5 on max)."""
    case = I.BY_NAME[name]
    sd_c, _ = I.nets(case, 8, 256, "folded")
    state = I.tensors(sd_c)
    rays = case.make_rays()
    z = _z(rays)
    y64, y64p, y32 = (A.raw_at_depths(rays, z, state, F64), A.raw_at_depths(rays, z, state, F64, fp32_points=True),
                      A.raw_at_depths(rays, z, state, F32))
    d = A.stats((y64p - y64).abs().numpy())
    e = A.stats((y32.double() - y64).abs().numpy())
    e_p = A.stats((y32.double() - y64p).abs().numpy())
    print(f"{name}: |fp64@fp32pts - fp64| max {d[0]:.9e} p99 {d[1]:.9e} med {d[2]:.9e} | |ref32 - fp64| {e[0]:.2e} {e[1]:.2e} {e[2]:.2e} "
          f"| |ref32 - fp64@fp32pts| {e_p[0]:.2e} {e_p[1]:.2e} {e_p[2]:.2e}")
    assert all(a <= 1.25 * b for a, b in zip(d, e)), (d, e)
    assert all(a <= b for a, b in zip(e_p, e)), (e_p, e)


def test_fp64_is_no_ground_truth_at_large_coordinates_and_fp64_at_fp32_points_is():
    """At |x| = 1e4 the plain fp64 path sees other points than the reference (|fp32 - fp64| = 7e-3: all point rounding); against
    the fp64-at-fp32-points ground truth the fp32 reference's error is that of its arithmetic again (1.4e-4: fp32 products of
    identity inputs of 1e3)."""
    case = I.BY_NAME["origin_10000"]
    sd_c, _ = I.nets(case, 8, 256, "folded")
    state = I.tensors(sd_c)
    rays = case.make_rays()
    z = _z(rays)
    y32 = A.raw_at_depths(rays, z, state, F32).double()
    e_plain = (y32 - A.raw_at_depths(rays, z, state, F64)).abs().max().item()
    e_pts = (y32 - A.raw_at_depths(rays, z, state, F64, fp32_points=True)).abs().max().item()
    print(f"origin 1e4: |ref32 - fp64| {e_plain:.2e}, |ref32 - fp64 at fp32 points| {e_pts:.2e}")
    assert e_pts < 0.1 * e_plain


# ------------------------------------------------------------------------------------------------------------------------
# the bound of nwe_selftest report[7]
# ------------------------------------------------------------------------------------------------------------------------



def test_wide_sincos_bound_comes_from_the_references_sinf():
    """The positional encoding of the reference is torch.sin / torch.cos of the fp32 product v * 2^b (embedding.py:36).  Over the
    range octave_sincos is documented for (|v| <= 5e4 in either lane half, i.e. arguments up to 2.56e7 rad) its error against
    fp64 libm is 3.58e-8 (0.6 ulp of a value in [0.5, 1)); the bound for the kernel's routine is that plus one such ulp
    (2^-24 = 5.96e-8): 9.54e-8, rounded up to 100e-9."""
    rng = np.random.Generator(np.random.Philox(key=[5, 5]))
    v = (10.0 ** rng.uniform(-1.0, np.log10(5e4), 200000) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    worst = 0.0
    for b in range(10):
        a = torch.from_numpy(v) * float(2 ** b)
        for fn in (torch.sin, torch.cos):
            worst = max(worst, (fn(a).double() - fn(a.double())).abs().max().item())
    print(f"reference sinf / cosf: max |fp32 - fp64| = {worst:.3e} over |v| <= 5e4, ten octaves")
    assert worst <= 2.0 ** -24                              # within one ulp: nothing like a lost range reduction
    assert (worst + 2.0 ** -24) * 1e9 <= I.SINCOS_WIDE_BOUND
