"""The scenes of tests/test_gpu_hollow_variants.py, vetted with the CPU oracle (tests/hollow_domain.py): every condition the GPU
tests assert from the GPU's own sigma holds for the fp32 oracle's, so a GPU test that finds one violated has found a difference
between the kernels and the reference, not a scene that never had it.  Every measured share is printed."""
import numpy as np
import pytest
import torch

from tests import hollow_domain as H


def _samplings(shape):
    """The samplings the GPU file runs a shape at: 64 + 128 at 8x256 (one case per variant: the on-equals-off tests of the
    terminating, occupancy and sharing kernels) and at the two shapes whose plain kernels never ran hollow."""
    return (H.RAGGED, H.SINGLE) + ((H.LONG,) if shape != "4x128" else ())


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_hollow_share_of_every_call_lies_in_the_cap(shape):
    for sampling in _samplings(shape):
        share = H.hollow_share(H.oracle(shape, sampling)[0][..., 3])
        print(f"{shape} {sampling} shift {H.shift_of(shape, sampling)}: hollow share {share:.3f}")
        assert H.in_cap(share), (shape, sampling, share)


@pytest.mark.parametrize("shape", sorted(H.SHAPES))
def test_gain_ends_rays_and_keeps_the_hollow_set(shape):
    """Gain 100 at eps = 1e-2: the conditions of the terminating tests; the hollow set is the one of gain 1 up to the rounding of
    the scaled weights.  Gain 1: the smallest transmittance is computed here, nothing stops at 1e-2, and at half the minimum -
    the eps the GPU test takes from its own FULL frame in the same way - no ray stops and every ray is decided."""
    raw1, z1, d = H.oracle(shape)
    plain = H.term_figures(raw1, z1, d)
    half = 0.5 * plain["min_trans"]
    print(f"{shape} gain 1: smallest transmittance {plain['min_trans']:.4f}, half of it {half:.4f}, rays that stop at 1e-2 {plain['stop']:.3f}")
    assert plain["stop"] == 0.0 and H.EPS < half < 1.0
    none = H.term_figures(raw1, z1, d, half)
    assert none["stop"] == 0.0 and none["decided"] == 1.0
    for sampling in (H.RAGGED,) + ((H.LONG,) if shape == "8x256" else ()):
        raw, z, d = H.oracle(shape, sampling, H.GAIN)
        fig = H.term_figures(raw, z, d)
        share = H.hollow_share(raw[..., 3])
        print(f"{shape} {sampling} gain {H.GAIN}: hollow share {share:.3f}, rays that stop {fig['stop']:.3f}, packets in which every ray "
              f"stops {fig['packets_all_stop']:.3f}, rays decided {fig['decided']:.3f}")
        assert H.in_cap(share) and H.term_conditions(fig), (shape, sampling, share, fig["stop"], fig["packets_all_stop"], fig["decided"])
        same = float((H.hollow(raw[..., 3]) == H.hollow(H.oracle(shape, sampling)[0][..., 3])).float().mean())
        assert same >= 0.999, (shape, sampling, same)
        # where the loop exit runs: under the sample split at every shape; under the packets plan only where a group of 128 stops
        for mode in (0, 1):
            lo, hi, whole = H.executed_interval(fig, mode, sampling[0])
            print(f"{shape} {sampling} decomposition {mode}: executed in [{lo}, {hi}] of {whole}, groups that stop {H.groups_that_stop(fig, mode):.3f}")
            if mode == 1 or shape not in H.TERM_GROUP_SHIFT:
                assert hi < whole, (shape, sampling, mode)
            else:
                assert lo == whole, (shape, sampling, mode)     # what TERM_GROUP_SHIFT is there for


@pytest.mark.parametrize("shape", sorted(H.TERM_GROUP_SHIFT))
def test_the_packets_plans_own_scene_has_groups_that_stop(shape):
    shift = H.TERM_GROUP_SHIFT[shape]
    raw, z, d = H.oracle(shape, H.RAGGED, H.GAIN, shift=shift)
    fig = H.term_figures(raw, z, d)
    share = H.hollow_share(raw[..., 3])
    lo, hi, whole = H.executed_interval(fig, 0, H.RAGGED[0])
    print(f"{shape} shift {shift}: hollow share {share:.3f}, rays that stop {fig['stop']:.3f}, groups of 128 that stop "
          f"{H.groups_that_stop(fig, 0):.3f}, decided {fig['decided']:.3f}, executed in [{lo}, {hi}] of {whole}")
    assert H.in_cap(share) and H.group_conditions(fig) and hi < whole


@pytest.mark.parametrize("shape", H.PAIR)
def test_occupancy_scene_has_every_kind_of_wave(shape):
    """37 + 0 under the checkerboard: each of the six shares above 0.01, at least 0.8 of the rays decided."""
    grid = H.occupancy_grid()
    raw, _, _ = H.oracle(shape, H.SINGLE)
    empty, decided = H.cells(H.oracle_rays().numpy(), H.SINGLE[0], grid)
    shares = H.occupancy_shares(raw[..., 3], empty)
    print(shape, " ".join(f"{k} {shares[k]:.3f}" for k in H.OCC_SHARES), f"rays decided {decided.mean():.3f}")
    assert all(shares[k] > 0.01 for k in H.OCC_SHARES), (shape, shares)
    assert decided.mean() >= 0.8


@pytest.mark.parametrize("shape", H.PAIR)
def test_nan_head_scenes_have_both_kinds_of_ray(shape):
    """The three NaN-head scenes of a shape: the hollow share in the cap, and among the decided rays both those whose rgb stays
    finite and those whose rgb does not, at least 1 % each; under termination some rays stop."""
    raw, z, d = H.oracle(shape, H.RAGGED, H.GAIN, shift=H.NAN_SHIFT["term", shape])
    fig = H.term_figures(raw, z, d)
    decided = fig["masked"]["decided"]
    finite = float(H.finite_under_termination(raw[..., 3], fig["masked"]["stop"])[decided].float().mean())
    share = H.hollow_share(raw[..., 3])
    print(f"{shape} terminating, shift {H.NAN_SHIFT['term', shape]}: hollow share {share:.3f}, finite {finite:.3f}, rays that stop {fig['stop']:.3f}, "
          f"decided {fig['decided']:.3f}")
    assert H.in_cap(share) and 0.01 <= finite <= 0.99 and fig["stop"] >= 0.01 and fig["decided"] >= 0.95

    raw, _, _ = H.oracle(shape, H.SINGLE, shift=H.NAN_SHIFT["occ", shape])
    empty, decided = H.cells(H.oracle_rays().numpy(), H.SINGLE[0], H.occupancy_grid())
    finite = float(H.finite_under_occupancy(raw[..., 3], empty)[torch.from_numpy(decided)].float().mean())
    share = H.hollow_share(raw[..., 3])
    print(f"{shape} occupancy, shift {H.NAN_SHIFT['occ', shape]}: hollow share {share:.3f}, finite {finite:.3f}")
    assert H.in_cap(share) and 0.01 <= finite <= 0.99

    raw, _, _ = H.oracle(shape, H.RAGGED, shift=H.NAN_SHIFT["share", shape])
    finite = float(H.hollow(raw[..., 3]).all(dim=1).float().mean())
    share = H.hollow_share(raw[..., 3])
    print(f"{shape} sharing, shift {H.NAN_SHIFT['share', shape]}: hollow share {share:.3f}, finite {finite:.3f}")
    assert H.in_cap(share) and 0.01 <= finite <= 0.99


@pytest.mark.parametrize("shape", H.PAIR)
def test_shared_and_baked_calls_stay_in_the_cap(shape):
    """k = 4 on rows [400, 404) and the baked coarse pass change where the fine samples lie: the hollow share of their own fine
    sigma, by the oracle's composition of the two rules."""
    shared, baked = H.hollow_share(H.oracle_shared_sigma(shape)), H.hollow_share(H.oracle_baked_sigma(shape))
    print(f"{shape}: hollow share under k = {H.SHARED_K} {shared:.3f}, under the baked coarse pass {baked:.3f}")
    assert H.in_cap(shared) and H.in_cap(baked)


def test_predictions_on_hand_made_cases():
    """finite_under_termination / finite_under_occupancy / hollow on two packets written out by hand."""
    S = 4
    sigma = torch.full((64, S), -1.0)
    sigma[3, 2] = 1.0                      # packet 0: on the full path at sample 2
    sigma[40, 0] = float("-inf")           # packet 1: -inf does not pass the test, sample 0 is on the full path
    h = H.hollow(sigma)
    assert h.tolist() == [[True, True, False, True], [False, True, True, True]]
    stop = torch.full((64,), S)
    stop[5], stop[6], stop[50] = 2, 3, 0
    fin = H.finite_under_termination(sigma, stop)
    assert not fin[3] and fin[5] and not fin[6] and not fin[40] and fin[50] and not fin[51]
    empty = np.zeros((64, S), bool)
    empty[7, 2] = True                     # the lane is masked where its packet is on the full path
    empty[41, :] = True
    fin = H.finite_under_occupancy(sigma, empty)
    assert fin[7] and not fin[8] and fin[41] and not fin[40]
    ragged = H.hollow(sigma[:40])          # 8 rays of packet 1: the last ray stands for the missing lanes
    assert ragged.shape == (2, S) and ragged[1].tolist() == [True, True, True, True]
