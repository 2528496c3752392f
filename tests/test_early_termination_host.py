"""Early ray termination without a GPU: the masked reference against the bounds the rule gives by construction, the setter's
domain and the getter on a host-only context, the handler's keyword and environment variable."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from tests import early_termination as E


@pytest.mark.parametrize("name", sorted(E.SCENES))
@pytest.mark.parametrize("eps", [1e-4, 1e-2])
def test_masked_reference_meets_the_bounds_by_construction(name, eps):
    """The dropped weights sum to less than eps, so |d rgb| < eps per channel, |d acc| < eps, |d depth| < eps * z_last; eps = 0 is
    the oracle's raw2outputs bit for bit; transmittance never increases, so a masked ray stays masked."""
    _, _, cfg, _, rays, ref = E.scene(name)
    raw, z = E.terminated_pass(ref, cfg)
    plain = E.masked_outputs(raw, z, rays[:, 3:6], 0.0)
    fine = cfg.n_importance > 0
    for k, key in (("rgb", "rgb_fine" if fine else "rgb_coarse"), ("depth", "depth_fine" if fine else "depth_coarse"),
                   ("acc", "acc_fine" if fine else "acc_coarse")):
        assert torch.equal(plain[k], ref[key]), k
    m = E.masked_outputs(raw, z, rays[:, 3:6], eps)
    dropped = (plain["weights"] - m["weights"]).sum(-1)
    slack = 1e-6                                        # fp32 sums of up to 192 weights below 1
    assert (dropped >= 0).all() and float(dropped.max()) < eps + slack
    assert float((m["rgb"] - plain["rgb"]).abs().max()) < eps + slack
    assert float((m["acc"] - plain["acc"]).abs().max()) < eps + slack
    assert ((m["depth"] - plain["depth"]).abs() < eps * z[:, -1] + slack * E.FAR).all()
    trans = m["trans"]
    assert (trans[:, 1:] <= trans[:, :-1]).all()
    below = trans < eps
    assert (below[:, 1:] | ~below[:, :-1]).all()        # once below, below to the end
    S = z.shape[1]
    assert ((m["stop"] == S) == ~below.any(-1)).all()


def test_scenes_have_the_groups_the_gpu_tests_need():
    """eps = 1e-2.  `mixed`: 128-ray groups in which some rays stop and some never do, and groups in which all stop; `allstop`,
    `ragged_samples`: every ray stops; `coarse_only`: a mixed group.  At most 5 % of the rays are undecided in the scenes of
    the parity test, and the masked reference differs from the unmasked one by more than ten times the parity tolerance on a
    fair share of the rays: a renderer that ignored eps would fail it."""
    def groups(name):
        m = E.masked_reference(name, 1e-2)
        S = m["trans"].shape[1]
        never = (m["stop"] == S).numpy()
        gs = [never[g:g + 128] for g in range(0, len(never), 128)]
        return m, sum(1 for g in gs if g.any() and not g.all()), sum(1 for g in gs if not g.any())
    m, mixed, allstop = groups("mixed")
    assert mixed >= 2 and allstop >= 2
    assert groups("coarse_only")[1] >= 1
    for name in ("allstop", "ragged_samples"):
        m, mixed, allstop = groups(name)
        assert mixed == 0 and allstop == 2
    for name in ("mixed", "allstop", "coarse_only", "ragged_samples"):
        m, plain = E.masked_reference(name, 1e-2), E.masked_reference(name, 0.0)
        assert float((~m["decided"]).float().mean()) <= 0.05, name
        bites = ((m["rgb"] - plain["rgb"]).abs().max(-1).values > 1e-3) | ((m["depth"] - plain["depth"]).abs() > 1e-3 * E.FAR) | \
                ((m["acc"] - plain["acc"]).abs() > 1e-3)
        assert float(bites.float().mean()) >= 0.25, name


@pytest.mark.parametrize("name", ["mixed", "allstop", "coarse_only", "ragged_samples"])
def test_reference_is_well_conditioned_on_the_parity_scenes(name):
    """The parity tolerances (rgb 1e-4, depth 1e-4 * far, acc 1e-4) mean something only where the reference reproduces itself:
    on every decided ray the fp32 masked reference agrees with the same rule applied to the oracle's fp64 evaluation to a
    tenth of the tolerance (the importance sampling amplifies rounding where a coarse bin is nearly empty, DESIGN.md section
    6), and no ray that reaches its last sample has a density within 1e-5 of the last interval's step (the "cliff rays"
    the project's parity tests set aside)."""
    _, _, cfg, _, rays, ref = E.scene(name)
    raw, z = E.terminated_pass(ref, cfg)
    raw64, z64 = E.terminated_pass(E.reference_fp64(name), cfg)
    m, m64 = E.masked_outputs(raw, z, rays[:, 3:6], 1e-2), E.masked_outputs(raw64, z64, rays[:, 3:6].double(), 1e-2)
    decided = m["decided"] & m64["decided"]
    assert float(decided.float().mean()) >= 0.95
    for k, tol in (("rgb", 1e-5), ("depth", 1e-5 * E.FAR), ("acc", 1e-5)):
        err = (m[k].double() - m64[k]).abs()
        err = err.max(-1).values if err.dim() == 2 else err
        assert float(err[decided].max()) <= tol, (name, k, float(err[decided].max()))
    reaches_end = m["stop"] == z.shape[1]
    assert not reaches_end.any() or float(raw[reaches_end, -1, 3].abs().min()) > 1e-5


def test_thin_fog_never_gets_that_low():
    """No ray of the thin fog (sigma 0.08) reaches a transmittance of 1e-2, let alone 1e-4: termination changes nothing there."""
    m = E.masked_reference("thin", 1e-2)
    assert float(m["trans"].min()) > 1e-2 and (m["stop"] == 192).all()


def test_executed_interval_arithmetic():
    """Two groups of 4 rays, S = 16: stops (3, 5, 16, 2) never finish early; stops (3, 5, 6, 2) need 6 samples."""
    stop, dec = [3, 5, 16, 2, 3, 5, 6, 2], [True] * 8
    assert E.executed_interval(stop, dec, 4, 1, 1, 16, 10) == (4 * 26 + 4 * 16, 4 * 26 + 4 * 17)
    assert E.executed_interval(stop, dec, 4, 4, 1, 16, 0) == (4 * 16 + 4 * 8, 4 * 16 + 4 * 12)
    assert E.executed_interval(stop, dec, 4, 1, 0, 16, 0) == (4 * 16 + 4 * 6,) * 2
    dec[6] = False       # the ray that decides the second group may stop one sample apart
    assert E.executed_interval(stop, dec, 4, 1, 1, 16, 0) == (4 * 16 + 4 * 5, 4 * 16 + 4 * 8)


def test_setter_domain_and_getter_on_a_host_only_context():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    assert r.early_termination == 0.0
    r.set_early_termination(1e-2)
    assert r.early_termination == np.float32(1e-2)
    # the last one is below 1 as a double and 1 in fp32
    for bad in (float("nan"), -1e-3, 1.0, 2.0, float("inf"), -float("inf"), math.nextafter(1.0, 0.0)):
        with pytest.raises(ValueError, match="min_transmittance"):
            r.set_early_termination(bad)
        assert lib.nwe_set_early_termination(r._ctx, bad) == _lib.NWE_ERR_INVALID
        assert r.early_termination == np.float32(1e-2)            # the previous value stays
    r.set_early_termination(float(np.nextafter(np.float32(1.0), np.float32(0.0))))   # the largest float below 1 is legal
    r.set_early_termination(-0.0)
    assert r.early_termination == 0.0 and math.copysign(1.0, r.early_termination) == 1.0
    assert lib.nwe_set_early_termination(None, 0.5) == _lib.NWE_ERR_INVALID and lib.nwe_get_early_termination(None) == -1.0
    # nothing was launched on a host-only context
    out = (C.c_int64 * 2)(7, 7)
    assert lib.nwe_last_ray_evaluations(r._ctx, out) == _lib.NWE_ERR_STATE and list(out) == [0, 0]
    assert lib.nwe_last_ray_evaluations(r._ctx, None) == _lib.NWE_ERR_INVALID
    r.close()


def test_handler_keyword_and_environment_variable(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    assert H("office_geneve", "x.ckpt").early_termination == 0.0
    assert H("office_geneve", "x.ckpt", early_termination=1e-3).early_termination == 1e-3
    monkeypatch.setenv("NWE_EARLY_TERMINATION", "0.01")
    assert H("office_geneve", "x.ckpt").early_termination == 0.01
    assert H("office_geneve", "x.ckpt", early_termination=1e-3).early_termination == 1e-3   # the keyword wins
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="early_termination"):
            H("office_geneve", "x.ckpt", early_termination=bad)
    monkeypatch.setenv("NWE_EARLY_TERMINATION", "1.5")
    with pytest.raises(ValueError, match="early_termination"):
        H("office_geneve", "x.ckpt")
