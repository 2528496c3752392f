"""Training tables (nwe_set_train_tables) and the one-shot hooks on the GPU over the domain of tests/train_domain.py.

(a) stage accuracy against fp64: every case is rendered once per mode with everything requested, and each stage is compared with
    the stage references fed what the kernel itself produced for the stage before it (stage B on the kernel's weights_coarse,
    stage C on the kernel's z_fine) - end to end even the fp32 oracle is 8e-2 of far from the fp64 oracle here
    (tests/test_train_domain_oracle.py).  The criterion is tests/accuracy.py's: max, p99 and median within FACTOR x the fp32
    reference's own error + FLOOR; the f32 kernel at K32, the f16x3 modes against the larger of the reference's and the f32
    kernel's error, capped at K32 x the reference's.  Undecided rays of stage B (fp32 and fp64 reference more than 1e-5 of far
    apart on the kernel's weights) are left out, at most 10 % of a case.
(b) invariants that need no reference, bit for bit: prefixes and tails of a call with their table rows, plans x dealing, a true
    hybrid launch (the only place the second launch's ray_first meets a per-ray table), separate passes, no-op tables.
(c) the edge set: NaN pattern and flag word are the oracle's, finite rays meet (a), the tie and the all-equal u are torch's bits.
(d) hooks together with tables: a hook replaces its stage and nothing else.
DESIGN.md 6.1.4 holds the measured figures.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from tests import accuracy as A
from tests import input_domain as I
from tests import train_domain as T
from tests.test_gpu_accuracy import _emulate_x1

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
FAR = T.FAR
COARSE = ("raw_coarse", "weights_coarse", "rgb_coarse", "depth_coarse", "acc_coarse")
LAST = ("rgb", "depth", "acc")
FINE = ("z_fine", "z_std", "raw_fine")
DEPTHS = ("depth", "depth_coarse", "z_fine", "z_std")
COARSE_BITS = 0xF0

# K32 (tests/accuracy.py): the f32 kernel's bound against the fp32 reference's own error.  The module's default of 1.5 holds for
# every output of every pass of fewer than 64 samples (measured at most 1.45).  Where a pass composites 64 samples or more (65+7,
# 64+128) the compositing's sequential fp32 sums, which every mode shares, meet outputs whose reference error is a few ulps -
# acc of a saturated ray: the kernel's median error is one ulp of 1.0 (1.2e-7), torch's blocked sum 4e-9 - and the measured
# factor, the smallest that satisfies the criterion, max (e_kernel - FLOOR) / e_ref32, rounded up to the next half, is
# (6 at most, the project's documented worst is 5.4):
K32_DEFAULT = 1.5
K32_LONG = {"acc_coarse": 2.5,      # measured 2.14
            "rgb": 4.5,             # 4.16
            "depth": 2.0,           # 1.67
            "acc": 4.5}             # 4.34
LONG_PASS = 64


def k32(name, samples):
    return K32_LONG.get(name, K32_DEFAULT) if samples >= LONG_PASS else K32_DEFAULT


def outputs(ni, coarse=True):
    return (COARSE if coarse else ()) + LAST + (FINE if ni else ())


def modes(net, ns):
    """(precision, plan) of a network: the fp32 kernel, and where both networks share an MFMA shape f16x3 under both plans
    (above kPacketMaxSamples coarse samples only the sample split exists)."""
    m = [("f32", -1)]
    if T.NET[net].mfma:
        m += [("f16x3", p) for p in ((0, 1) if ns <= T.K_PACKET_MAX_SAMPLES else (1,))]
    return m


@pytest.fixture(scope="module")
def pool():
    """One renderer per (network, single pass, separate passes) for the module; `get` sets the sampling and restores the
    automatic plan and dealing."""
    made = {}

    def get(name, ns, ni, separate=False, sds=None):
        key = (name, ni == 0, separate, None if sds is None else id(sds[0]))
        if key not in made:
            b = T.built(name, ni)
            r = nwe_amd.Renderer(0)
            r.debug_set_fold(b.net.fold)
            sd_c, sd_f = sds if sds is not None else (b.sd_c, b.sd_f)
            r.set_network(0, sd_c)
            r.set_network(1, sd_f)
            r.set_separate_passes(separate)
            made[key] = r
        r = made[key]
        r.set_sampling(ns, ni)
        r.debug_set_decomposition(-1)
        r.debug_set_work_queue(-1)
        return r

    yield get
    for r in made.values():
        r.close()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A device fault ends the run: nothing more is started on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU faulted: {e}", returncode=3)


def render(r, rays, prec, outs, tab=None, hooks=None, plan=-1):
    h = hooks or {}
    kw = {}
    if "fine_depths" in h:
        kw["debug_fine_depths"] = h["fine_depths"]
    if "raw_coarse" in h or "raw_fine" in h:
        kw["debug_raw"] = (h.get("raw_coarse"), h.get("raw_fine"))
    if "coarse_weights" in h:
        kw["debug_coarse_weights"] = h["coarse_weights"]
    r.debug_set_decomposition(plan)
    out = r.render_rays(rays.cuda(), precision=prec, outputs=outs, train=dict(tab) if tab else None, **kw)
    return {k: v.cpu() for k, v in out.items() if not k.startswith("_")}


def rows(d, sl):
    return None if d is None else {k: v[sl] for k, v in d.items()}


def same(got, want, ctx, keys=None, flags=True):
    for k in (keys if keys is not None else [k for k in want if k != "flags"]):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (ctx, k)
    if flags:
        assert int(got["flags"]) == int(want["flags"]), (ctx, "flags", hex(int(got["flags"])), hex(int(want["flags"])))


def _bounds(prec, name, alt, samples):
    """tests/test_gpu_accuracy._bounds per output; `samples`: those of the pass that produced it."""
    k = k32(name, samples)
    return {"factor": k} if prec == "f32" or alt is None else {"y_alt": alt[name], "alt_cap": k}


def _scale(name):
    return FAR if name in DEPTHS else 1.0


def stage_check(rep, tag, r, b, rays, ns, ni, tab, got, prec, kf, hooks=None, keep=None, cache=None):
    """Holds every stage of one render to the criterion.  `got`: the render's outputs (CPU), `kf`: the f32 kernel's outputs of the
    same call (the second yardstick of an f16x3 mode), `hooks`: what the call was armed with, `keep` [R]: rays compared (default
    all).  Returns the number of undecided rays."""
    h = hooks or {}
    R = rays.shape[0]
    tag = f"{b.net.name} {ns}+{ni} {tag}"
    keep = np.ones(R, bool) if keep is None else keep
    cache = {} if cache is None else cache
    alt = None if prec == "f32" else kf
    und_n = 0
    if "coarse_weights" not in h:                                                   # stage A
        if "A" not in cache:
            cache["A"] = tuple(T.stage_a(b, rays, ns, tab, dt, raw=h.get("raw_coarse")) for dt in (F32, F64))
        a32, a64 = cache["A"]
        k_a = keep & ~T.on_alpha_step(a64, tab.get("noise_coarse"))
        names = {"raw_coarse": "raw", "weights_coarse": "weights", "rgb_coarse": "rgb", "depth_coarse": "depth", "acc_coarse": "acc"}
        if ni == 0:
            names.update(rgb="rgb", depth="depth", acc="acc")                       # the fine slots hold the coarse results
        for name, key in names.items():
            rep.add(f"{tag} A {name}", got[name], a32[key], a64[key], scale=_scale(name), keep=keep if key == "raw" else k_a,
                    **_bounds(prec, name, alt, ns))
        if "raw_coarse" in h:
            assert torch.equal(got["raw_coarse"], h["raw_coarse"]), (tag, "raw_coarse is the caller's")
    if ni == 0:
        return 0
    if "fine_depths" not in h:                                                      # stage B, on the kernel's own weights
        w = h["coarse_weights"] if "coarse_weights" in h else got["weights_coarse"]
        zc = T.z_coarse(rays, ns, tab.get("t_rand"))
        key = ("B", w.numpy().tobytes())
        if key not in cache:
            cache[key] = tuple(T.stage_b(zc, w, ni, tab.get("u"), dt) for dt in (F32, F64))
        b32, b64 = cache[key]
        und = T.undecided(b32, b64) & keep
        und_n = int(und.sum())
        assert und_n <= T.UNDECIDED_CAP * R, f"{tag}: {und_n} of {R} rays undecided in stage B on the kernel's weights"
        for name in ("z_fine", "z_std"):           # the sampler is the same fp32 code in every mode: no second yardstick
            rep.add(f"{tag} B {name} ({und_n} undecided)", got[name], b32[name], b64[name], scale=FAR, keep=keep & ~und, factor=K32_DEFAULT)
    else:
        assert torch.equal(got["z_fine"], h["fine_depths"]), (tag, "z_fine is the caller's")
    z = got["z_fine"]                                                               # stage C, at the kernel's own depths
    key = ("C", z.numpy().tobytes())
    if key not in cache:
        cache[key] = tuple(T.stage_c(b, rays, z, tab.get("noise_fine"), dt, raw=h.get("raw_fine")) for dt in (F32, F64))
    c32, c64 = cache[key]
    if alt is not None and not torch.equal(z, kf["z_fine"]):                        # the f32 kernel's fine pass at this mode's depths
        hk = {"fine_depths": z, **({"raw_fine": h["raw_fine"]} if "raw_fine" in h else {})}
        alt = render(r, rays, "f32", ("raw_fine",) + LAST, T.pick(tab, ("noise_fine",)), hk)
    k_c = keep & ~T.on_alpha_step(c64, tab.get("noise_fine")) & np.isfinite(z.numpy()).all(-1)
    for name, key in (("raw_fine", "raw"), ("rgb", "rgb"), ("depth", "depth"), ("acc", "acc")):
        rep.add(f"{tag} C {name}", got[name], c32[key], c64[key], scale=_scale(name), keep=keep & np.isfinite(z.numpy()).all(-1) if key == "raw" else k_c,
                **_bounds(prec, name, alt, ns + ni))
    if "raw_fine" in h:
        assert torch.equal(got["raw_fine"], h["raw_fine"]), (tag, "raw_fine is the caller's")
    return und_n


def same_flags(flags):
    """Every mode raises the flags the f32 kernel raises (tests/test_gpu_accuracy._same_flags)."""
    assert len({v & ~16 for v in flags.values()}) == 1, {k: hex(v) for k, v in flags.items()}


# ------------------------------------------------------------------------------------------------------------------------
# a. stage accuracy against fp64
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", T.CASES, ids=[c.id for c in T.CASES])
def test_stages_against_fp64(pool, case):
    c = case
    b = T.built(c.net, c.ni)
    tab = T.case_tables(c)
    r = pool(c.net, c.ns, c.ni)
    rep, cache, flags = A.Report(), {}, {}
    kf = None
    for prec, plan in modes(c.net, c.ns):
        got = render(r, b.rays, prec, outputs(c.ni), tab, plan=plan)
        kf = got if prec == "f32" else kf
        name = f"{prec}" + (f" d{plan}" if plan >= 0 else "")
        stage_check(rep, name, r, b, b.rays, c.ns, c.ni, tab, got, prec, kf, cache=cache)
        flags[name] = int(got["flags"])
        if plan >= 0:
            assert r.debug_last_plan() == plan
    same_flags(flags)
    rep.check()


@pytest.mark.parametrize("ns,ni", [(7, 6), (9, 0)])
def test_single_product_stages_against_the_emulator(pool, ns, ni):
    """f16x1, 4x128, 16 rays, stages A and C: the emulated single-product arithmetic of the packed stream at the kernel's own
    points (tests/mfma_emulator.py), composited by the reference with the same noise rows, is the yardstick (raw_accuracy)."""
    n = 16
    b = T.built("4x128", ni)
    rays = b.rays[:n].contiguous()
    tab = rows(T.tables(ns, ni, 1.0), slice(0, n))
    r = pool("4x128", ns, ni)
    got = render(r, rays, "f16x1", outputs(ni), tab)
    rep = A.Report()
    zc = T.z_coarse(rays, ns, tab["t_rand"])
    stages = [("A", zc, b.sd_c, tab["noise_coarse"], T.stage_a(b, rays, ns, tab, F64),
               {"raw_coarse": "raw", "weights_coarse": "weights", "rgb_coarse": "rgb", "depth_coarse": "depth", "acc_coarse": "acc"})]
    if ni:
        z = got["z_fine"]
        stages.append(("C", z, b.sd_f, tab["noise_fine"], T.stage_c(b, rays, z, tab["noise_fine"], F64),
                       {"raw_fine": "raw", "rgb": "rgb", "depth": "depth", "acc": "acc"}))
    for st, z, sd, noise, y64, names in stages:
        raw = _emulate_x1(sd, True, rays, z).to(F32)
        emu = T._composite(raw, z, rays, noise, F32)
        keep = ~T.on_alpha_step(y64, noise)
        for name, key in names.items():
            rep.add(f"f16x1 {st} {name} (vs emulated x1)", got[name], emu[key], y64[key], scale=_scale(name), keep=None if key == "raw" else keep)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# b. invariants that need no reference
# ------------------------------------------------------------------------------------------------------------------------

PREFIX_NETS = ("4x128", "16x30")
PREFIX_HOOKS = {None: (), "coarse_weights": ("coarse_weights",), "raw": ("raw_coarse", "raw_fine"), "fine_depths": ("fine_depths",)}
PREFIX_CASES = [(net, ns, ni, hook) for net in PREFIX_NETS for ns, ni in ((7, 6), (9, 0)) for hook in PREFIX_HOOKS
                if ni or hook in (None, "raw")]


@pytest.mark.parametrize("net,ns,ni,hook", PREFIX_CASES, ids=[f"{n}-{s}+{i}-{h}" for n, s, i, h in PREFIX_CASES])
def test_prefixes_and_tail_with_their_table_rows(pool, net, ns, ni, hook):
    """The first n rays with the first n table (and hook) rows are the first n rows of the 165-ray call, and rays 37.. with rows
    37.. are its tail: a row is a function of its own ray alone, wherever the ray sits in its packet, workgroup or launch.  A
    part's flag word is over fewer rays: its bits are among the whole call's."""
    b = T.built(net, ni)
    tab = T.tables(ns, ni, 1.0)
    hk = {k: v for k, v in T.hook_inputs(ns, ni).items() if k in PREFIX_HOOKS[hook] and (ni or k == "raw_coarse")}
    outs = outputs(ni, coarse=hook != "coarse_weights")
    r = pool(net, ns, ni)
    for prec, plan in modes(net, ns):
        whole = render(r, b.rays, prec, outs, tab, hk, plan)
        for sl in [slice(0, n) for n in (1, 31, 32, 33, 127, 128, 129)] + [slice(37, None)]:
            part = render(r, b.rays[sl].contiguous(), prec, outs, rows(tab, sl), rows(hk, sl), plan)
            same(part, rows({k: v for k, v in whole.items() if k != "flags"}, sl), (prec, plan, sl), flags=False)
            assert int(part["flags"]) & ~int(whole["flags"]) == 0, (prec, plan, sl)


PLAN_CASES = [("4x128", 7, 6, s) for s in T.SUBSETS] + [(n, 7, 6, T.ALL4) for n in T.MFMA_NETWORKS[1:]] + \
             [(n, 65, 7, T.ALL4) for n in T.MFMA_NETWORKS] + [("4x128", 9, 0, T.SUBSETS_NI0[-1])]


@pytest.mark.parametrize("net,ns,ni,subset", PLAN_CASES, ids=[f"{n}-{s}+{i}-{'+'.join(t)}" for n, s, i, t in PLAN_CASES])
def test_plans_and_dealing_are_bit_identical(pool, net, ns, ni, subset):
    """Plans 0, 1 and a forced 2, each dealt statically and from the queue: one result.  Above kPacketMaxSamples only plan 1 exists."""
    b = T.built(net, ni)
    tab = T.pick(T.tables(ns, ni, 1.0), subset)
    r = pool(net, ns, ni)
    want = None
    for plan in (0, 1, 2):
        for queue in (0, 1):
            r.debug_set_work_queue(queue)
            got = render(r, b.rays, "f16x3", outputs(ni), tab, plan=plan)
            assert r.debug_last_plan() == (plan if ns <= T.K_PACKET_MAX_SAMPLES else 1), (plan, queue)
            assert any(r.debug_last_queue()["grid"]) == bool(queue), (plan, queue)
            want = want or got
            same(got, want, (plan, queue))


def test_hybrid_launch_second_launch_reads_its_own_table_rows(pool):
    """cus * 128 + 165 rays under plan 2: the packets launch takes the full round, the sample-split launch starts at
    ray_first = cus * 128 and must read table row ray_first + i for its ray i.  Equal to plan 0, and its last 165 rays equal to
    those rays rendered alone with their own rows; statically dealt and queued (both launches then take tickets)."""
    ns, ni = 5, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = T.build("4x128")
    n = cus * 128 + T.N_RAYS
    rays = b.rays.repeat((n + T.N_RAYS - 1) // T.N_RAYS, 1)[:n].contiguous()
    tab = T.tables(ns, ni, 1.0, seed=3, n_rays=n)                # fresh random rows per ray: tiled rays, distinct rows
    r = pool("4x128", ns, ni)
    outs = outputs(ni)
    r.debug_set_work_queue(0)
    want = render(r, rays, "f16x3", outs, tab, plan=0)
    assert r.debug_last_plan() == 0
    tail = slice(n - T.N_RAYS, None)
    alone = render(r, rays[tail].contiguous(), "f16x3", outs, rows(tab, tail), plan=0)
    same(rows(want, tail), alone, "plan 0 tail vs alone", flags=False)
    assert not torch.equal(want["rgb"][:T.N_RAYS], want["rgb"][tail])      # the rows do differ between the tiles
    for queue in (0, 1):
        r.debug_set_work_queue(queue)
        got = render(r, rays, "f16x3", outs, tab, plan=2)
        assert r.debug_last_plan() == 2
        parts = r.last_launch_parts()
        assert [p[1] for p in parts] == [cus * 128, T.N_RAYS], parts
        q = r.debug_last_queue()
        assert (all(q["grid"]) and q["taken"] == q["grid"]) if queue else not any(q["grid"]), q
        same(got, want, ("hybrid", queue))
        same(rows(got, tail), alone, ("hybrid tail vs alone", queue), flags=False)


@pytest.mark.parametrize("subset", T.SUBSETS, ids=["+".join(s) for s in T.SUBSETS])
def test_separate_passes_one_shape(pool, subset):
    ns, ni = 7, 6
    b = T.build("4x128")
    tab = T.pick(T.tables(ns, ni, 1.0), subset)
    off, on = pool("4x128", ns, ni), pool("4x128", ns, ni, separate=True)
    for plan in (0, 1):
        same(render(on, b.rays, "f16x3", outputs(ni), tab, plan=plan), render(off, b.rays, "f16x3", outputs(ni), tab, plan=plan), (subset, plan))
        assert on.last_coarse_launch()[1] == T.N_RAYS and off.last_coarse_launch() is None


@pytest.mark.parametrize("subset", [("t_rand",), ("noise_coarse",), ("noise_fine",), T.ALL4], ids=lambda s: "+".join(s))
def test_separate_passes_two_shapes(pool, subset):
    """4x128 under 8x256 (include/nwe.h): the coarse outputs are those of a (coarse, coarse) context, everything else that of a
    (fine, fine) context fed these weights through nwe_debug_set_coarse_weights, with the same tables, bit for bit."""
    ns, ni = 7, 6
    b = T.build("c4x128-f8x256")
    tab = T.pick(T.tables(ns, ni, 1.0), subset)
    sep = pool("c4x128-f8x256", ns, ni, separate=True)
    cc = pool("c4x128-f8x256", ns, ni, sds=(b.sd_c, b.sd_c))
    ff = pool("c4x128-f8x256", ns, ni, sds=(b.sd_f, b.sd_f))
    rest = outputs(ni, coarse=False)
    for plan in (0, 1):
        got = render(sep, b.rays, "f16x3", outputs(ni), tab, plan=plan)
        c = render(cc, b.rays, "f16x3", COARSE, tab, plan=plan)
        f = render(ff, b.rays, "f16x3", rest, tab, {"coarse_weights": got["weights_coarse"]}, plan=plan)
        same(got, c, (subset, plan, "coarse"), keys=COARSE, flags=False)
        same(got, f, (subset, plan, "fine"), keys=rest, flags=False)
        assert int(got["flags"]) == (int(c["flags"]) & (COARSE_BITS | I.FLAG_RAW)) | (int(f["flags"]) & ~COARSE_BITS), (subset, plan)


@pytest.mark.parametrize("net,ns,ni", [("4x128", 7, 6), ("4x128", 9, 0), ("4x128", 65, 7), ("6x128-novd", 7, 6), ("1x2-freqs0-3+1", 7, 6)])
def test_no_op_tables_give_inference(pool, net, ns, ni):
    """Noise rows of 0.0 and u equal to the linspace table: inference, bit for bit.  (No t_rand puts every depth on its linspace
    value, so none is claimed.)"""
    b = T.built(net, ni)
    r = pool(net, ns, ni)
    noops = {"noise_coarse": torch.zeros(T.N_RAYS, ns)}
    if ni:
        noops.update(noise_fine=torch.zeros(T.N_RAYS, ns + ni), u=T.linspace_u(T.N_RAYS, ni))
    for prec, plan in modes(net, ns):
        plain = render(r, b.rays, prec, outputs(ni), plan=plan)
        for key in list(noops) + ["all"]:
            tab = noops if key == "all" else {key: noops[key]}
            same(render(r, b.rays, prec, outputs(ni), tab, plan=plan), plain, (prec, plan, key))


# ------------------------------------------------------------------------------------------------------------------------
# c. the edge set
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns,ni", T.EDGE_SAMPLINGS)
def test_edge_set(pool, ns, ni):
    b = T.built("4x128", ni)
    tab = T.edge_tables(b, ns, ni)
    E = T.EDGE_RAYS
    outs = outputs(ni)
    from oracle import nerf_oracle as O
    res32 = O.render_rays(b.rays, b.tc, b.tf if ni else None, T.config(b, ns, ni), train=tab)
    word = I.expected_flags(res32, outs, ni > 0)
    key_of = lambda name: "weights_coarse" if name == "weights_coarse" else I.oracle_key(name, ni > 0)
    keep = np.ones(T.N_RAYS, bool)
    keep[[E["noise_nan_coarse"], E["noise_nan_fine"]]] = False
    r = pool("4x128", ns, ni)
    rep, cache, kf = A.Report(), {}, None
    for prec, plan in modes("4x128", ns):
        tag = f"edge {prec}" + (f" d{plan}" if plan >= 0 else "")
        got = render(r, b.rays, prec, outs, tab, plan=plan)
        kf = got if prec == "f32" else kf
        # the NaN pattern of every output, element by element, and the flag word are the oracle's
        for name in outs:
            want = res32[key_of(name)]
            want = want[..., :4] if name.startswith("raw") else want
            assert np.array_equal(~np.isfinite(got[name].numpy()), ~np.isfinite(want.numpy())), (tag, name)
            bad = np.nonzero(I.ray_mask(~np.isfinite(got[name].numpy())))[0].tolist()
            assert bad == T.edge_expectation(ni)[name], (tag, name, bad)
        assert int(got["flags"]) == word, (tag, hex(int(got["flags"])), hex(word))
        # finite rays: the stage criterion
        stage_check(rep, tag, r, b, b.rays, ns, ni, tab, got, prec, kf, keep=keep, cache=cache)
        if ni:
            # the all-equal u and the tie (u on fp32 cdf entries): the cdf is torch's bit for bit (include/nwe.h), so the samples are
            zc = T.z_coarse(b.rays, ns, tab["t_rand"])
            own = T.stage_b(zc, got["weights_coarse"], ni, tab["u"], F32)
            for ray in (E["u_equal"], E["u_tie"]):
                assert torch.equal(got["z_fine"][ray], own["z_fine"][ray]), (tag, "own weights", ray)
                assert torch.equal(got["z_std"][ray], own["z_std"][ray]), (tag, "own weights, z_std", ray)
            # ... on the fp32 oracle's weights the numbers of the tie ray ARE entries of the kernel's cdf
            w = res32["weights_coarse"]
            hooked = render(r, b.rays, prec, ("z_fine", "z_std"), T.pick(tab, ("t_rand", "u")), {"coarse_weights": w}, plan)
            ref = T.stage_b(zc, w, ni, tab["u"], F32)
            for ray in (E["u_equal"], E["u_tie"]):
                assert torch.equal(hooked["z_fine"][ray], ref["z_fine"][ray]), (tag, "oracle weights", ray)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------------
# d. hooks together with tables
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", list(T.COMBINATIONS))
@pytest.mark.parametrize("net", ["4x128", "6x128-novd", "16x30"])
def test_hooks_with_tables(pool, net, combo):
    """tests/train_domain.COMBINATIONS: each stage that still runs meets the criterion of (a) on the references the rule gives,
    the outputs a hook supplies are the caller's bits, and what the rule says is untouched is bit-identical."""
    ns, ni = T.COMBINATION_SAMPLING
    b = T.build(net)
    hook_names, tables = T.COMBINATIONS[combo]
    tab = T.pick(T.tables(ns, ni, 1.0), tables)
    hk = {k: v for k, v in T.hook_inputs(ns, ni).items() if k in hook_names}
    outs = outputs(ni, coarse="coarse_weights" not in hk)
    r = pool(net, ns, ni)
    rep, cache, flags, kf = A.Report(), {}, {}, None
    for prec, plan in modes(net, ns):
        tag = f"{combo} {prec}" + (f" d{plan}" if plan >= 0 else "")
        got = render(r, b.rays, prec, outs, tab, hk, plan)
        kf = got if prec == "f32" else kf
        stage_check(rep, tag, r, b, b.rays, ns, ni, tab, got, prec, kf, hooks=hk, cache=cache)
        flags[tag] = int(got["flags"])
        if combo == "weights+noise_coarse":          # the noise has nothing to act on
            same(got, render(r, b.rays, prec, outs, None, hk, plan), tag)
        if combo == "depths+u":                       # the sampler feeds nothing into the fine pass, but z_std is still its own
            alone = render(r, b.rays, prec, outs, None, hk, plan)
            same(got, alone, tag, keys=[k for k in outs if k != "z_std"], flags=False)
            same(got, render(r, b.rays, prec, outs, tab, None, plan), tag, keys=["z_std"], flags=False)
            assert not torch.equal(got["z_std"], alone["z_std"])
    same_flags(flags)
    rep.check()
