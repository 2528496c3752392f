"""The training-table domain of tests/train_domain.py on the oracle alone (CPU): every condition here is one on
oracle/nerf_oracle.py, none on a kernel.  tests/test_gpu_train_domain.py compares the kernels with the same stage references,
stage by stage; this file shows that those references mean something:

  * the stages chained are the oracle's render loop, bit for bit;
  * stage by stage the fp32 and the fp64 oracle agree (A and C to 1e-5; B except on "undecided" rays, at most 10 % of a case),
    while end to end they do not - which is why the GPU file compares per stage;
  * every case composites something, every table changes what it should and nothing in front of it;
  * the edge set does what tests/train_domain.py says it does.

Measured (fp32 against fp64, worst over a network's cases; rgb / acc absolute, depths in units of far):
  4x128 5.3e-6, 8x256 5.1e-6, 6x128 without view directions 6.5e-6, 4x128 unfolded 4.2e-6, 1x2 7.8e-7, 4x128 under 8x256 7.7e-6.
  16x30 6.0e-6 with a weight gain of 2.5; with the 2.9 of tests/shape_domain.py's case it is 1.3e-4 (|raw| up to 17.5 after
  sixteen layers, fp32 raw error 2.9e-4), so the gain was lowered on the oracle alone (tests/train_domain.SHAPE_WEIGHTS).
Undecided rays of stage B on the fp32 oracle's own weights: at most 9 of 165 in any case (the cap is 16).
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import input_domain as I
from tests import train_domain as T

F32, F64 = torch.float32, torch.float64
AGREE = 1e-5


def _diff(x, y, far=1.0):
    return float((x.double() - y.double()).abs().max()) / far


def _key(name, fine):
    return "weights_coarse" if name == "weights_coarse" else I.oracle_key(name, fine)


def _oracle(b, ns, ni, tab, dtype=F32):
    return O.render_rays(b.rays, b.tc, b.tf if ni else None, T.config(b, ns, ni), train=tab, dtype=dtype)


@pytest.mark.parametrize("name,ns,ni", [("4x128", 7, 6), ("6x128-novd", 5, 3), ("16x30", 7, 6), ("8x256", 9, 0)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_stages_chained_are_the_oracle_loop(name, ns, ni, dtype):
    b = T.built(name, ni)
    tab = T.tables(ns, ni, 1.0)
    res = _oracle(b, ns, ni, tab, dtype)
    a, sb, c = T.chain(b, b.rays, ns, ni, tab, dtype)
    pairs = [("z_coarse", a["z"]), ("raw_coarse", a["raw"]), ("weights_coarse", a["weights"]), ("rgb_coarse", a["rgb"]),
             ("depth_coarse", a["depth"]), ("acc_coarse", a["acc"])]
    if ni:
        pairs += [("z_fine", sb["z_fine"]), ("z_std", sb["z_std"]), ("raw_fine", c["raw"]), ("rgb_fine", c["rgb"]),
                  ("depth_fine", c["depth"]), ("acc_fine", c["acc"])]
    for key, mine in pairs:
        want = res[key][..., :4] if key.startswith("raw") else res[key]
        assert torch.equal(mine, want), key
    if ni and dtype == F32:       # stage B on the fp32 depths and weights is the loop's own sampler
        sb32 = T.stage_b(T.z_coarse(b.rays, ns, tab["t_rand"]), a["weights"], ni, tab["u"], F32)
        assert torch.equal(sb32["z_fine"], res["z_fine"]) and torch.equal(sb32["z_std"], res["z_std"])


@pytest.mark.parametrize("name", [n.name for n in T.NETWORKS])
def test_stage_agreement(name):
    """Every (sampling, subset, std) of the network: stages A and C of the fp32 and the fp64 oracle agree to 1e-5 (rgb, acc;
    depths: of far), stage B fed the fp32 oracle's own weights agrees on all but the undecided rays, at most 10 % of the
    case; no ray sits on the alpha step of the last interval; the mean fp64 acc of at least one pass lies in 0.05 .. 0.999."""
    failed, worst, worst_und = [], 0.0, 0
    for c in [c for c in T.CASES if c.net == name]:
        b = T.built(c.net, c.ni)
        tab = T.case_tables(c)
        a32, a64 = T.stage_a(b, b.rays, c.ns, tab, F32), T.stage_a(b, b.rays, c.ns, tab, F64)
        d = {"A " + k: _diff(a32[k], a64[k], T.FAR if k == "depth" else 1.0) for k in ("rgb", "acc", "depth")}
        step = int(T.on_alpha_step(a64, tab.get("noise_coarse")).sum())
        accs = [float(a64["acc"].mean())]
        und = 0
        if c.ni:
            zc = T.z_coarse(b.rays, c.ns, tab.get("t_rand"))
            assert torch.equal(zc, a32["z"])
            b32, b64 = (T.stage_b(zc, a32["weights"], c.ni, tab.get("u"), dt) for dt in (F32, F64))
            und = int(T.undecided(b32, b64).sum())
            c32, c64 = (T.stage_c(b, b.rays, b32["z_fine"], tab.get("noise_fine"), dt) for dt in (F32, F64))
            d.update({"C " + k: _diff(c32[k], c64[k], T.FAR if k == "depth" else 1.0) for k in ("rgb", "acc", "depth")})
            step += int(T.on_alpha_step(c64, tab.get("noise_fine")).sum())
            accs.append(float(c64["acc"].mean()))
        worst, worst_und = max(worst, max(d.values())), max(worst_und, und)
        print(f"{c.id:<62s} " + " ".join(f"{k} {v:.1e}" for k, v in d.items()) + f" | undecided {und} | acc {accs}")
        bad = {k: v for k, v in d.items() if not v <= AGREE}
        if bad:
            failed.append(f"{c.id}: fp32 and fp64 stages differ by {bad}")
        if und > T.UNDECIDED_CAP * T.N_RAYS:
            failed.append(f"{c.id}: {und} of {T.N_RAYS} rays undecided in stage B")
        if step:
            failed.append(f"{c.id}: {step} rays on the alpha step")
        if not any(0.05 <= a <= 0.999 for a in accs):
            failed.append(f"{c.id}: nothing composited, mean acc {accs}")
    print(f"{name}: worst stage difference {worst:.2e}, most undecided rays {worst_und}")
    assert not failed, "\n".join(failed)


def test_end_to_end_the_two_oracles_disagree():
    """The check on the method: with noise_coarse of unit variance at 7+6 the fp32 oracle's z_fine is more than 1e-3 of far from
    the fp64 oracle's - the sampler amplifies the coarse pass's rounding - although each stage agrees to 1e-5 (above)."""
    b = T.build("4x128")
    tab = T.pick(T.tables(7, 6, 1.0), ("noise_coarse",))
    r32, r64 = _oracle(b, 7, 6, tab, F32), _oracle(b, 7, 6, tab, F64)
    d = _diff(r32["z_fine"], r64["z_fine"], T.FAR)
    print(f"end to end, noise_coarse at std 1, 7+6: z_fine differs by {d:.2e} of far, rgb by {_diff(r32['rgb_fine'], r64['rgb_fine']):.2e}")
    assert d > 1e-3


@pytest.mark.parametrize("name", ["4x128", "6x128-novd", "16x30"])
def test_each_table_changes_what_it_should_and_nothing_in_front_of_it(name):
    ns, ni = 7, 6
    b = T.build(name)
    tab = T.tables(ns, ni, 1.0)
    plain = _oracle(b, ns, ni, {}, F64)
    moved = {"t_rand": ("z_coarse", "depth_coarse", "z_fine"), "noise_coarse": ("weights_coarse", "acc_coarse", "z_fine"),
             "noise_fine": ("acc_fine", "rgb_fine"), "u": ("z_fine", "z_std")}
    for key, outs in moved.items():
        armed = _oracle(b, ns, ni, {key: tab[key]}, F64)
        for k in outs:
            assert _diff(armed[k], plain[k]) > 1e-3, (key, k)
    # a change to a table leaves the stages in front of it as they were, bit for bit (fp32, all four armed)
    base = _oracle(b, ns, ni, tab, F32)
    other = T.tables(ns, ni, 1.0, seed=9)
    coarse = ("z_coarse", "raw_coarse", "weights_coarse", "rgb_coarse", "depth_coarse", "acc_coarse")
    untouched = {"noise_coarse": ("z_coarse", "raw_coarse"), "u": coarse, "noise_fine": coarse + ("z_fine", "z_std")}
    for key, outs in untouched.items():
        res = _oracle(b, ns, ni, dict(tab, **{key: other[key]}), F32)
        for k in outs:
            assert torch.equal(res[k], base[k]), (key, k)
        assert not torch.equal(res["rgb_fine"], base["rgb_fine"]), key


@pytest.mark.parametrize("ns,ni", T.EDGE_SAMPLINGS)
def test_edge_set(ns, ni):
    b = T.built("4x128", ni)
    tab = T.edge_tables(b, ns, ni)
    E = T.EDGE_RAYS
    # depths stay inside their strata and ascending, the rays of 0 and of nextafter(1, 0) included
    z = T.z_coarse(b.rays, ns, tab["t_rand"])
    base = T.z_coarse(b.rays, ns, None)
    mids = .5 * (base[:, 1:] + base[:, :-1])
    lower, upper = torch.cat([base[:, :1], mids], -1), torch.cat([mids, base[:, -1:]], -1)
    assert bool((z >= lower).all()) and bool((z <= upper).all()) and bool((z[:, 1:] >= z[:, :-1]).all())
    assert torch.equal(z[E["t_zero"]], lower[E["t_zero"]])
    assert bool((z[E["t_one"]] > base[E["t_one"]])[:-1].all())     # at or one rounding below `upper`, never past it (above)
    res32, res64 = _oracle(b, ns, ni, tab, F32), _oracle(b, ns, ni, tab, F64)
    if ni:
        a32 = T.stage_a(b, b.rays, ns, tab, F32)
        for dt in (F32, F64):
            sb = T.stage_b(z, a32["weights"], ni, tab["u"], dt)
            zs = sb["z_samples"]
            assert bool((zs[E["u_equal"]] == zs[E["u_equal"], 0]).all())                  # an all-equal u: all samples equal
            assert float(sb["z_std"][E["u_equal"]]) == 0.0
        # the tie: u == cdf[k] in fp32 -> searchsorted(right=True) steps past the entry, t = 0, the sample IS bin edge k
        r = E["u_tie"]
        cdf = O.sample_pdf_cdf(a32["weights"][r:r + 1, 1:-1])[0]
        u = tab["u"][r]
        assert all(bool((cdf == x).any()) for x in u)
        k = torch.searchsorted(cdf, u.contiguous(), right=True) - 1
        assert bool((cdf[k] == u).all())
        zmid = .5 * (z[r, 1:] + z[r, :-1])
        sb32 = T.stage_b(z, a32["weights"], ni, tab["u"], F32)
        assert torch.equal(sb32["z_samples"][r], zmid[k])
        assert torch.equal(sb32["z_fine"].nan_to_num(-1.0), res32["z_fine"].nan_to_num(-1.0))      # ... and is the loop's
    # the non-finite rays: the hand-written expectation holds in both oracles, element masks agree between them
    outs = tuple(T.edge_expectation(ni))
    for res in (res32, res64):
        for name, rays in T.edge_expectation(ni).items():
            v = res[_key(name, ni > 0)]
            v = v[..., :4] if name.startswith("raw") else v
            got = np.nonzero(I.ray_mask(~torch.isfinite(v).numpy()))[0].tolist()
            assert got == rays, (name, got, rays)
    for name in outs:
        k = _key(name, ni > 0)
        assert np.array_equal(~torch.isfinite(res32[k]).numpy(), ~torch.isfinite(res64[k]).numpy()), name
    side = "fine" if ni else "coarse"
    assert float(res32["acc_" + side][E["noise_minus"]]) == 0.0 and bool(torch.isnan(res32["disp_" + side][E["noise_minus"]]))
    assert float(res32["weights_coarse"][E["noise_plus"], 0]) == 1.0 and float(res32["acc_coarse"][E["noise_plus"]]) == 1.0
    # the flag word the GPU test demands: every per-ray bit of both passes; NWE_FLAG_RAW and NWE_FLAG_ZSTD through the NaN depths
    word = I.expected_flags(res32, outs, ni > 0)
    assert word == I.expected_flags(res64, outs, ni > 0)
    assert word == (0x3FF if ni else 0x0FF), hex(word)
