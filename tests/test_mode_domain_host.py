"""tests/mode_domain.py without a GPU: the shape list against the packer, the conditions under which the scenes of part A test
anything (rays stop, few are undecided, a renderer that ignored eps would fail, the reference reproduces itself), and the flag
and mask expectations of part B against the CPU oracle.  Every test prints the figures it asserts.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import synthetic
from tests import input_domain as I
from tests import mode_domain as M


# ---- the shape list -------------------------------------------------------------------------------------------------------------

def test_shape_list_is_what_the_packer_accepts_and_what_the_accuracy_tests_list():
    """The 12 shapes are tests/test_gpu_accuracy.INSTANTIATIONS without the reference formulation, and exactly the (D, W) of
    depths 2..10 and widths 64..256 (the widest the ABI takes) that Renderer(host_only=True).mfma_supported accepts, with and without view directions."""
    from tests import test_gpu_accuracy as A
    assert sorted(M.SHAPES) == sorted(s for s in A.INSTANTIATIONS if s[2] != "reference")
    assert len(M.SHAPES) == len(set(M.SHAPES)) == 12 and sorted(M.NETS) == sorted(M.IDS)
    r = nwe_amd.Renderer(host_only=True)
    try:
        accepted = []
        for view, form in ((True, "folded"), (False, "no_view_dirs")):
            for D in range(2, 11):
                for Wd in (64, 128, 192, 256):
                    shape = r.set_network(0, synthetic.make_state_dict(7, D, Wd, use_view_dirs=view))
                    assert tuple(shape[:2]) == (D, Wd)
                    if r.mfma_supported(0):
                        accepted.append((D, Wd, form))
        print("accepted by the packer:", accepted)
        assert sorted(accepted) == sorted(M.SHAPES)
    finally:
        r.close()
    # the ring of the two-shape pairs covers every shape, each as coarse and as fine network of two different partners
    for form in ("folded", "no_view_dirs"):
        names = {M.kind(D, Wd, form) for D, Wd in M.FOLDED}
        pairs = [p for p in M.PAIRS if p[0] in names]
        assert len(pairs) == 12 and all(a != b and b in names for a, b in pairs)
        assert {a for a, _ in pairs} == {b for _, b in pairs} == names
    assert [M.density_only(*s) for s in M.DOMAIN_SHAPES] == [True, False, False]


# ---- part A: the scenes ---------------------------------------------------------------------------------------------------------

def _report(tag, f):
    print(f"{tag}: stop {f['stop']:.3f}, undecided {f['undecided']:.3f}, decided in fp32 and fp64 {f['decided_both']:.3f}, "
          f"max|masked - plain| rgb {f['bite_rgb']:.1e} depth {f['bite_depth']:.1e} acc {f['bite_acc']:.1e} "
          f"(min over stopping rays rgb {f['bite_min_rgb']:.1e}), fp32 vs fp64 rgb {f['fp64_rgb']:.1e} depth {f['fp64_depth']:.1e} "
          f"acc {f['fp64_acc']:.1e}")


def _bites(f):
    """Some ray's masked reference is further than ten times the parity tolerance from the plain one."""
    return any(f["bite_" + k] > 10 * M.TOL[k] for k in M.LEAN)


def _well_conditioned(f):
    return all(f["fp64_" + k] <= 0.1 * M.TOL[k] for k in M.LEAN)


COUNTS = [(D, Wd, form, 64, 128) for D, Wd, form in M.SHAPES] + [(D, Wd, form, ns, ni) for D, Wd, form in M.COUNT_SHAPES for ns, ni in M.BIG_COUNTS]
COUNT_IDS = [f"{M.kind(D, Wd, form)}-{ns}+{ni}" for D, Wd, form, ns, ni in COUNTS]


@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNTS, ids=COUNT_IDS)
def test_halfstop_stops_part_of_every_group_and_is_well_conditioned(D, Wd, form, ns, ni):
    """eps = 1e-2: between 20 % and 80 % of the rays stop, at most 10 % are undecided, ignoring eps would miss the parity
    tolerance tenfold on some ray, the fp32 masked reference agrees with the fp64 one to a tenth of the tolerance on the rays
    decided in both - and every 128-ray group holds rays that stop and rays that do not."""
    f = M.scene_figures(D, Wd, form, "halfstop", ns, ni)
    _report(f"halfstop {M.kind(D, Wd, form)} {ns}+{ni}", f)
    assert 0.2 <= f["stop"] <= 0.8
    assert f["undecided"] <= 0.10
    assert _bites(f)
    assert _well_conditioned(f)
    stops = (M.masked_reference(D, Wd, form, "halfstop", ns, ni)["stop"] < ns + ni).numpy()
    for g in range(0, M.N_RAYS, 128):
        assert stops[g:g + 128].any() and not stops[g:g + 128].all(), g


@pytest.mark.parametrize("D,Wd,form", M.SHAPES, ids=M.IDS)
def test_thin_never_gets_near_its_eps_and_allstop_stops_everywhere(D, Wd, form):
    """`thin` (eps = 1e-4): no transmittance below 1e-2, so the terminating kernels mask nothing.  `allstop` at 7 + 6
    (eps = 1e-2): every ray stops, none is undecided, and the reference reproduces itself."""
    m = M.masked_reference(D, Wd, form, "thin")
    print(f"thin {M.kind(D, Wd, form)}: min transmittance {float(m['trans'].min()):.3f}")
    assert float(m["trans"].min()) > 1e-2 and (m["stop"] == 192).all() and m["decided"].all()
    f = M.scene_figures(D, Wd, form, "allstop", 7, 6)
    _report(f"allstop {M.kind(D, Wd, form)} 7+6", f)
    assert f["stop"] == 1.0 and f["undecided"] == 0.0 and _bites(f) and _well_conditioned(f)


@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNTS[12:], ids=COUNT_IDS[12:])
def test_allstop_with_more_than_64_coarse_samples(D, Wd, form, ns, ni):
    """Every ray stops, at most 10 % are undecided, and the reference reproduces itself: the scene in which the workgroups of
    the single-packet plan leave early."""
    f = M.scene_figures(D, Wd, form, "allstop", ns, ni)
    _report(f"allstop {M.kind(D, Wd, form)} {ns}+{ni}", f)
    assert f["stop"] == 1.0 and f["undecided"] <= 0.10 and _bites(f) and _well_conditioned(f)


@pytest.mark.parametrize("D,Wd,form,ns,ni", COUNTS[:3] + COUNTS[12:], ids=COUNT_IDS[:3] + COUNT_IDS[12:])
def test_masked_reference_with_eps_zero_is_the_oracle(D, Wd, form, ns, ni):
    """The masked reference restates raw2outputs: at eps = 0 it is the oracle's fine outputs bit for bit, for every sample
    count and with and without view directions."""
    ref = M.scene(D, Wd, form, "halfstop", ns, ni)[5]
    plain = M.masked_reference(D, Wd, form, "halfstop", ns, ni, eps=0.0)
    for k in M.LEAN:
        assert torch.equal(plain[k], ref[k + "_fine"]), k


def test_interval_plans():
    """The three groupings of M.intervals on stops that show them apart: 256 rays of which ray 0 alone never stops."""
    stop, dec = np.full(256, 8), np.ones(256, bool)
    stop[0] = 16
    lag = {"packets": 1, "split": 1, "f32": 0}
    iv = M.intervals(stop, dec, 4, 16, lag)
    assert iv["packets"] == (256 * 4 + 128 * 16 + 128 * 8, 256 * 4 + 128 * 16 + 128 * 9)
    assert iv["split"] == (256 * 4 + 32 * 16 + 224 * 8, 256 * 4 + 32 * 16 + 224 * 12)
    assert iv["f32"] == (256 * 4 + 16 * 16 + 240 * 8,) * 2


# ---- part B: the input-domain table ---------------------------------------------------------------------------------------------

DOMAIN_IDS = [M.kind(*s) for s in M.DOMAIN_SHAPES]


def test_domain_cases_are_the_sixteen_pinhole_cases():
    assert len(M.DOMAIN_CASES) == 16 and M.DOMAIN_CASES[:6] == ["healthy", "near_eq_far", "zero_direction", "underflow_direction", "far_inf", "nan_c2w"]
    assert set(M.DOMAIN_CASES[6:]) == set(I.NETWORK_CASES) and len(I.NETWORK_CASES) == 10
    # the new argument of I.nets changes nothing for those who do not pass it, and touches the fine density head alone
    case = I.BY_NAME["nan_rgb_linear_fine"]
    for form in ("folded", "no_view_dirs"):
        a, b = I.nets(case, 6, 256, form), I.nets(case, 6, 256, form, fine_fog=None)
        c = I.nets(case, 6, 256, form, fine_fog=M.FINE_FOG)
        assert all(np.array_equal(a[i][k], b[i][k], equal_nan=True) for i in (0, 1) for k in a[i])
        assert all(np.array_equal(a[0][k], c[0][k], equal_nan=True) for k in a[0])
        changed = sorted(k for k in a[1] if not np.array_equal(a[1][k], c[1][k], equal_nan=True))
        assert changed == (["_alpha_linear.bias", "_alpha_linear.weight"] if form == "folded" else ["_output_linear.bias", "_output_linear.weight"])
        key = "_rgb_linear.weight" if form == "folded" else "_output_linear.weight"
        assert np.isnan(c[1][key][1, 3])                                # the spoil comes behind the fog


@pytest.mark.parametrize("name", M.DOMAIN_CASES)
@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_flag_expectations_of_separate_passes(D, Wd, form, name):
    """B1: the flag words the GPU test expects, against the oracle's masks: a lean frame's word is the full frame's without the
    raw / z_std bits and - density-only shapes - without NWE_FLAG_RGB_COARSE; the colour-only defect is seen by a lean frame
    exactly where the coarse colour exists."""
    res = M.domain_oracle(name, D, Wd, form)[3]
    d_only = M.density_only(D, Wd, form)
    full = I.expected_flags(res, I.FULL, True)
    lean = I.expected_flags(res, I.LEAN, True, density_only=d_only)
    print(f"{name} {M.kind(D, Wd, form)}: full 0x{full:x}, lean 0x{lean:x}")
    assert lean == full & ~(I.FLAG_RAW | I.FLAG_ZSTD) & ~(I.FLAG_RGB_COARSE if d_only else 0)
    masks = I.oracle_masks(res, True)
    for bit, key in ((I.FLAG_RGB, "rgb"), (I.FLAG_DEPTH, "depth"), (I.FLAG_ACC, "acc"), (I.FLAG_RGB_COARSE, "rgb_coarse"),
                     (I.FLAG_DEPTH_COARSE, "depth_coarse"), (I.FLAG_ACC_COARSE, "acc_coarse")):
        assert bool(full & bit) == bool(masks[key].any()), key
    if name == "nan_rgb_linear_coarse":
        assert full & I.FLAG_RGB_COARSE and bool(lean & I.FLAG_RGB_COARSE) == (not d_only)
        assert lean & ~I.FLAG_RGB_COARSE == 0


@pytest.mark.parametrize("name", M.DOMAIN_CASES)
@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_shared_reference_of_the_domain_cases(D, Wd, form, name):
    """B2, k = 2: with finite coarse depths the shared reference's non-finite rays are the representatives' (depth, acc: they
    follow the depths) joined with the ray's own (rgb: its view direction, the fine network); far_inf and nan_c2w leave no
    finite ray.  k = 1 is the oracle itself."""
    rays, _, sd_f, res = M.domain_oracle(name, D, Wd, form)
    own = M.domain_shared_reference(name, D, Wd, form, 1)
    for k, key in (("rgb", "rgb_fine"), ("depth", "depth_fine"), ("acc", "acc_fine")):
        assert torch.equal(torch.nan_to_num(own[k], nan=-7.0), torch.nan_to_num(res[key], nan=-7.0)), k
    ref = M.domain_shared_reference(name, D, Wd, form, 2)
    bad = {k: I.ray_mask(~torch.isfinite(ref[k]).numpy()) for k in M.LEAN}
    print(f"{name} {M.kind(D, Wd, form)} k 2: non-finite rays " + ", ".join(f"{k} {int(bad[k].sum())}" for k in M.LEAN))
    if name in M.FINITE_DEPTHS:
        assert torch.isfinite(res["z_coarse"]).all()
        masks = I.oracle_masks(res, True)
        for k in M.LEAN:
            # every case of the table is all rays or none
            assert bad[k].all() == I.ray_mask(masks[k]).all() and bad[k].any() == I.ray_mask(masks[k]).any(), k
    else:
        assert all(bad[k].all() for k in M.LEAN)


@pytest.mark.parametrize("D,Wd,form", M.DOMAIN_SHAPES, ids=DOMAIN_IDS)
def test_fine_fog_stops_rays_of_the_healthy_case(D, Wd, form):
    """B3: with the fine fog (0.4, 0.01) and eps = 1e-2 between 20 % and 80 % of the 48 healthy rays stop and at most 10 % are
    undecided; near_eq_far stops nowhere (its only interval with a length is the last one); a NaN transmittance is never
    below eps, so the cases with a NaN fine pass stop nowhere either."""
    m = M.domain_masked_reference("healthy", D, Wd, form)
    plain = M.domain_masked_reference("healthy", D, Wd, form, eps=0.0)
    S = I.NS + I.NI
    stop, und = float((m["stop"] < S).float().mean()), float((~m["decided"]).float().mean())
    bite = float((m["rgb"] - plain["rgb"]).abs().max())
    print(f"healthy {M.kind(D, Wd, form)} fine fog {M.FINE_FOG}: stop {stop:.3f}, undecided {und:.3f} ({int((~m['decided']).sum())} rays), "
          f"max|masked - plain| rgb {bite:.1e}")
    assert 0.2 <= stop <= 0.8 and und <= 0.10 and bite > 10 * M.TOL["rgb"]
    assert (M.domain_masked_reference("near_eq_far", D, Wd, form)["stop"] == S).all()
    for name in M.DOMAIN_CASES:
        mm = M.domain_masked_reference(name, D, Wd, form)
        nan_trans = torch.isnan(mm["trans"]).any(-1)
        print(f"{name} {M.kind(D, Wd, form)}: {int((mm['stop'] < S).sum())} rays stop, {int(nan_trans.sum())} with a NaN transmittance")
