"""The case table of tests/shape_domain.py without a GPU: every case tests something (liveness and conditioning on the fp64
oracle alone), the table holds every edge of the legal shape domain (asserted from the case fields), a host-only context packs
every case as the table says (shape, flops, MFMA support), and the borders of nwe_set_network / nwe_set_network_no_view_dirs /
nwe_set_sampling are refused just outside and accepted just inside.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from tests import shape_domain as S

MAX_LEFT_OUT = 0.05          # share of a case's rays the alpha-step rule (|sigma_last| < 1e-5 in fp64) may leave out


# ------------------------------------------------------------------------------------------------------------------------
# every case tests something
# ------------------------------------------------------------------------------------------------------------------------

def liveness_problems(case, res64):
    """What keeps a case from testing anything, on the fp64 oracle alone: a last pass that composites nothing (or saturates on
    every ray), a density of one sign, a raw channel that does not move."""
    acc, raw = S.last_pass(res64, case)
    acc, raw = acc.numpy(), raw.numpy().reshape(-1, 4)
    problems = []
    if not (acc.max() - acc.min() >= 0.2 or (acc.min() >= 0.2 and acc.max() <= 0.98)):
        problems.append(f"acc in [{acc.min():.3g}, {acc.max():.3g}]: spans < 0.2 and not inside [0.2, 0.98]")
    pos, neg = float((raw[:, 3] > 0).mean()), float((raw[:, 3] < 0).mean())
    if pos < 0.10 or neg < 0.01:
        problems.append(f"raw sigma positive on {pos:.1%}, negative on {neg:.1%} of the samples (need 10 % / 1 %)")
    std = raw.std(0)
    if not (std > 1e-3).all():
        problems.append(f"raw channel standard deviations {std}")
    return problems


@pytest.mark.parametrize("name", S.NAMES)
def test_case_is_alive_and_well_conditioned(name):
    b, res32, res64 = S.reference(name)
    case = b.case
    acc, raw = S.last_pass(res64, case)
    print(f"{name}: acc {acc.min().item():.3f} .. {acc.max().item():.3f}, sigma > 0 on {(raw[..., 3] > 0).float().mean().item():.1%}, "
          f"< 0 on {(raw[..., 3] < 0).float().mean().item():.1%}, raw std {raw.reshape(-1, 4).std(0).numpy()}")
    assert b.rays.shape == (S.N_RAYS, 11 if case.view_dirs else 8)
    assert not liveness_problems(case, res64), liveness_problems(case, res64)
    for res in (res32, res64):
        assert all(torch.isfinite(v).all() for k, v in res.items() if not k.startswith("disp")), name
    left_out = [(res64[k][:, -1, 3].abs() < 1e-5).float().mean().item() for k in ("raw_coarse", "raw_fine") if k in res64]
    assert max(left_out) <= MAX_LEFT_OUT, (name, left_out)
    # the thin-fog coarse pass gives every bin weight: no importance sample goes through the denom < 1e-5 replacement
    if case.ni:
        z = res64["z_coarse"]
        d = S.O.sample_pdf_diagnostics(.5 * (z[:, 1:] + z[:, :-1]).float(), res32["weights_coarse"][:, 1:-1], case.ni)
        assert d["min_denom"].min().item() > 1e-4, d["min_denom"].min().item()


def test_table_holds_every_edge_of_the_domain():
    """From the case fields, not the names."""
    cs = S.CASES
    both = lambda c: (c.coarse, c.fine)
    same = lambda c: c.coarse == c.fine
    has = lambda pred: any(pred(c) for c in cs)
    assert len(set(S.NAMES)) == len(cs)
    # depth 1, W/2 = 1, in_xyz = in_dir = 3, the smallest sampling with importance samples
    assert has(lambda c: same(c) and c.fine.D == 1 and c.fine.W == 2 and c.in_xyz == 3 and c.in_dir == 3 and (c.ns, c.ni) == (3, 1))
    # the skip after layer 0, W/2 = 3, freqs 1 / 0
    assert has(lambda c: same(c) and c.fine == S.Net(2, 6, (0,)) and (c.freqs_xyz, c.freqs_dir) == (1, 0) and c.view_dirs)
    # kMaxDepth with a width that is no multiple of 4
    assert has(lambda c: same(c) and c.fine.D == S.MAX_DEPTH and c.fine.W == 30 and c.fine.W % 4)
    # the skip input entering the last trunk layer (skip = D - 2) of 6x64, and of 7x32
    assert has(lambda c: same(c) and c.fine == S.Net(6, 64, (4,)) and c.view_dirs and not c.feat_map)
    assert has(lambda c: same(c) and c.fine == S.Net(7, 32, (5,)) and c.fine.skip == c.fine.D - 2)
    # the bounds of the encoding rows, a width just under the maximum
    assert has(lambda c: same(c) and c.fine == S.Net(3, 254, (1,)) and c.in_xyz == S.MAX_IN_XYZ and c.in_dir == S.MAX_IN_DIR)
    # two MFMA shapes that differ; wider coarse over narrower fine
    assert has(lambda c: both(c) == (S.Net(4, 128), S.Net(8, 256, (4,))) and c.mfma == (True, True) and c.view_dirs
               and (c.freqs_xyz, c.freqs_dir) == (10, 4))
    assert has(lambda c: both(c) == (S.Net(8, 256, (4,)), S.Net(2, 16)) and c.view_dirs)
    # neighbours of MFMA shapes, none of them supported
    for net, fx in ((S.Net(8, 256), 10), (S.Net(8, 256, (3,)), 10), (S.Net(4, 128, (1,)), 10), (S.Net(8, 256, (4,)), 9)):
        assert has(lambda c: same(c) and c.fine == net and (c.freqs_xyz, c.freqs_dir) == (fx, 4) and c.view_dirs
                   and c.mfma == (False, False)), (net, fx)
    # without view directions: output_ch at both bounds, and two shapes
    assert has(lambda c: not c.view_dirs and same(c) and c.fine == S.Net(5, 48, (), S.MIN_OUTPUT_CH))
    assert has(lambda c: not c.view_dirs and same(c) and c.fine == S.Net(5, 48, (), S.MAX_OUTPUT_CH) and c.freqs_xyz == 6)
    assert has(lambda c: not c.view_dirs and both(c) == (S.Net(4, 128), S.Net(6, 64, (4,))))
    # the largest and the smallest sampling
    assert has(lambda c: same(c) and c.fine == S.Net(2, 8) and (c.freqs_xyz, c.freqs_dir) == (4, 2)
               and (c.ns, c.ni) == (S.MAX_SAMPLES, S.MAX_IMPORTANCE))
    assert has(lambda c: c.coarse == S.Net(2, 8) and (c.ns, c.ni) == (2, 0))
    assert has(lambda c: c.white_background and 16 <= c.fine.W <= 128 and c.ni > 0)
    # the endpoint feature at W/2 = 1, 3, 32, each with another coarse network
    for half in (1, 3, 32):
        assert has(lambda c: c.feat_map and c.fine.W // 2 == half and not same(c) and c.view_dirs and c.ni > 0), half
    # every case is inside the domain and outside the MFMA kernels' reach
    for c in cs:
        for n in both(c):
            assert 1 <= n.D <= S.MAX_DEPTH and 2 <= n.W <= S.MAX_WIDTH and n.W % 2 == 0 and len(n.skips) <= 1
            assert all(0 <= s <= n.D - 2 for s in n.skips), c.name
            assert c.view_dirs or S.MIN_OUTPUT_CH <= n.output_ch <= S.MAX_OUTPUT_CH
        assert 3 <= c.in_xyz <= S.MAX_IN_XYZ and (not c.view_dirs or 3 <= c.in_dir <= S.MAX_IN_DIR)
        assert 2 <= c.ns <= S.MAX_SAMPLES and 0 <= c.ni <= S.MAX_IMPORTANCE and (c.ni == 0 or c.ns >= 3)
        assert not (all(c.mfma) and same(c)) and not (c.ni == 0 and c.mfma[0]), c.name
        assert c.name in S.BY_NAME
    assert all(n in S.BY_NAME and S.BY_NAME[n].ni > 0 for n in S.RAGGED_CASES)
    assert S.RAGGED_COUNTS == (1, 15, 16, 17, 37)


# ------------------------------------------------------------------------------------------------------------------------
# a host-only context packs every case
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
def test_host_only_context_packs_the_case(name):
    b = S.build(S.BY_NAME[name])
    case = b.case
    r = nwe_amd.Renderer(host_only=True)
    for which, sd in ((0, b.sd_c), (1, b.sd_f)):
        if sd is None:
            continue
        assert r.set_network(which, sd) == case.shape(which)
        assert r.flops_per_eval(which) == 2 * S.forward_weight_elements(sd)
        assert r.mfma_supported(which) == case.mfma[which]
    r.set_sampling(case.ns, case.ni)
    assert r.ray_columns == (11 if case.view_dirs else 8)
    r.close()


# ------------------------------------------------------------------------------------------------------------------------
# the borders
# ------------------------------------------------------------------------------------------------------------------------

class _Raw:
    """nwe_set_network* called with bare numbers: every layer pointer shows the same zeroed buffer, large enough for the
    largest legal layer (256 x (256 + 93)), so an accepted call reads inside it and a refused one reads nothing."""

    def __init__(self):
        self.lib = _lib.load()
        self.r = nwe_amd.Renderer(host_only=True)
        self.buf = np.zeros(S.MAX_WIDTH * (S.MAX_WIDTH + S.MAX_IN_XYZ), np.float32)
        self.ptrs = (C.c_void_p * (S.MAX_DEPTH + 4 + 1))(*([self.buf.ctypes.data] * (S.MAX_DEPTH + 4 + 1)))

    def view(self, D=4, W=64, in_xyz=63, in_dir=27, skip=-1, which=0):
        return self.lib.nwe_set_network(self.r._ctx, which, D, W, in_xyz, in_dir, skip, self.ptrs, self.ptrs)

    def noview(self, D=4, W=64, in_xyz=63, skip=-1, out_ch=5, which=0):
        return self.lib.nwe_set_network_no_view_dirs(self.r._ctx, which, D, W, in_xyz, skip, out_ch, self.ptrs, self.ptrs)

    def sampling(self, ns, ni):
        t = np.linspace(0, 1, max(ns, 2)).astype(np.float32)
        u = np.linspace(0, 1, max(ni, 1)).astype(np.float32)
        return self.lib.nwe_set_sampling(self.r._ctx, t.ctypes.data, (1 - t).ctypes.data, ns, u.ctypes.data if ni > 0 else None, ni)

    def error(self):
        return self.lib.nwe_last_error(self.r._ctx).decode()


OUTSIDE = [("view", dict(D=0)), ("view", dict(D=17)), ("view", dict(W=0)), ("view", dict(W=3)), ("view", dict(W=258)),
           ("view", dict(in_xyz=0)), ("view", dict(in_xyz=8)), ("view", dict(in_xyz=10)), ("view", dict(in_xyz=99)),
           ("view", dict(in_dir=0)), ("view", dict(in_dir=4)), ("view", dict(in_dir=69)),
           ("noview", dict(D=0)), ("noview", dict(D=17)), ("noview", dict(W=0)), ("noview", dict(W=3)), ("noview", dict(W=258)),
           ("noview", dict(in_xyz=0)), ("noview", dict(in_xyz=8)), ("noview", dict(in_xyz=99)),
           ("noview", dict(out_ch=3)), ("noview", dict(out_ch=257))]
INSIDE = [("view", dict(D=1)), ("view", dict(D=16)), ("view", dict(W=2)), ("view", dict(W=256)), ("view", dict(in_xyz=3)),
          ("view", dict(in_xyz=9)), ("view", dict(in_xyz=93)), ("view", dict(in_dir=3)), ("view", dict(in_dir=63)),
          ("view", dict(D=16, W=256, in_xyz=93, in_dir=63, skip=14)),
          ("noview", dict(D=1)), ("noview", dict(D=16)), ("noview", dict(W=2)), ("noview", dict(W=256)), ("noview", dict(in_xyz=3)),
          ("noview", dict(in_xyz=93)), ("noview", dict(out_ch=4)), ("noview", dict(out_ch=256))]


def test_network_borders_are_refused_outside_and_accepted_inside():
    """depth 1..16, even width 2..256, in_xyz = 3 + 6 k <= 93, in_dir = 3 + 6 k <= 63, output_ch 4..256: just outside is
    NWE_ERR_UNSUPPORTED with a message and leaves the network set before it as it was; just inside is accepted.  (in_xyz = 9 is
    3 + 6 x 1, one frequency: legal, and the table's skip-0 case uses it; its neighbours 8 and 10 are the refused ones.)"""
    raw = _Raw()
    sd = nwe_amd.synthetic.make_state_dict(7, 4, 128)
    for which in (0, 1):
        raw.r.set_network(which, sd)
    before = [(raw.r.flops_per_eval(w), raw.r.packed_stream(w).tobytes(), raw.r.packed_bias(w).tobytes()) for w in (0, 1)]
    for which in (0, 1):
        for fn, kw in OUTSIDE:
            assert getattr(raw, fn)(which=which, **kw) == _lib.NWE_ERR_UNSUPPORTED, (fn, kw)
            assert len(raw.error()) > 10, (fn, kw)
            now = [(raw.r.flops_per_eval(w), raw.r.packed_stream(w).tobytes(), raw.r.packed_bias(w).tobytes()) for w in (0, 1)]
            assert now == before, (fn, kw)
    assert raw.view(which=2) == _lib.NWE_ERR_INVALID and raw.noview(which=-1) == _lib.NWE_ERR_INVALID
    for fn, kw in INSIDE:
        assert getattr(raw, fn)(which=1, **kw) == _lib.NWE_OK, (fn, kw, raw.error())
        assert raw.r.flops_per_eval(1) > 0 and raw.r.flops_per_eval(0) == before[0][0]
    # a skip that feeds no layer (after the last trunk layer, or nonsense) is no skip: the flops are those without one
    assert raw.view(D=4, skip=-1, which=1) == _lib.NWE_OK
    plain = raw.r.flops_per_eval(1)
    for skip in (3, 4, 99, -7):
        assert raw.view(D=4, skip=skip, which=1) == _lib.NWE_OK and raw.r.flops_per_eval(1) == plain, skip
    assert raw.view(D=4, skip=2, which=1) == _lib.NWE_OK and raw.r.flops_per_eval(1) == plain + 2 * 63 * 64
    raw.r.close()


def test_sampling_borders():
    """n_samples 2..128 and n_importance 0..256 (NWE_ERR_UNSUPPORTED outside); importance samples need three coarse samples,
    because sample_pdf takes weights[..., 1:-1] (NWE_ERR_INVALID).  A refusal leaves the sampling set before it in place."""
    raw = _Raw()
    assert raw.sampling(64, 128) == _lib.NWE_OK
    for (ns, ni), code in (((1, 0), _lib.NWE_ERR_UNSUPPORTED), ((129, 0), _lib.NWE_ERR_UNSUPPORTED), ((0, 0), _lib.NWE_ERR_UNSUPPORTED),
                           ((64, 257), _lib.NWE_ERR_UNSUPPORTED), ((64, -1), _lib.NWE_ERR_UNSUPPORTED),
                           ((2, 1), _lib.NWE_ERR_INVALID), ((2, 256), _lib.NWE_ERR_INVALID)):
        assert raw.sampling(ns, ni) == code, (ns, ni)
        assert len(raw.error()) > 10
    for ns, ni in ((2, 0), (128, 0), (3, 1), (3, 256), (128, 256)):
        assert raw.sampling(ns, ni) == _lib.NWE_OK, (ns, ni, raw.error())
    raw.r.close()
    # the wrapper turns the codes into exceptions and keeps its own record of the sampling
    r = nwe_amd.Renderer(host_only=True)
    r.set_sampling(16, 24)
    for ns, ni, exc in ((1, 0, NotImplementedError), (129, 0, NotImplementedError), (16, 257, NotImplementedError), (2, 4, ValueError)):
        with pytest.raises(exc):
            r.set_sampling(ns, ni)
        assert (r.n_samples, r.n_importance) == (16, 24)
    r.close()


def test_wrapper_refuses_what_the_abi_cannot_express():
    """Two skip connections, and a layer whose input width is neither W nor W + in_xyz: ValueError before anything is packed."""
    r = nwe_amd.Renderer(host_only=True)
    good = nwe_amd.synthetic.make_state_dict(3, 5, 16, in_xyz=15, in_dir=9, skips=(1,))
    assert r.set_network(0, good) == (5, 16, 15, 9, 1)
    flops = r.flops_per_eval(0)
    with pytest.raises(ValueError, match="more than one skip"):
        r.set_network(0, nwe_amd.synthetic.make_state_dict(3, 5, 16, in_xyz=15, in_dir=9, skips=(1, 3)))
    bad = {k: v.copy() for k, v in good.items()}
    bad["_pts_linears.3.weight"] = np.zeros((16, 20), np.float32)
    with pytest.raises(ValueError, match="unexpected input width 20"):
        r.set_network(0, bad)
    bad = {k: v.copy() for k, v in good.items()}
    bad["_pts_linears.2.bias"] = np.zeros(15, np.float32)
    with pytest.raises(ValueError, match="_pts_linears.2"):
        r.set_network(0, bad)
    with pytest.raises(ValueError, match="no _pts_linears.0"):
        r.set_network(0, {k: v for k, v in good.items() if not k.startswith("_pts_linears")})
    # the wrapper's view of the ABI's borders: exceptions by code
    for kw in (dict(D=17, W=8), dict(D=2, W=258), dict(D=2, W=8, in_xyz=99), dict(D=2, W=8, in_dir=69)):
        with pytest.raises(NotImplementedError):
            r.set_network(0, nwe_amd.synthetic.make_state_dict(3, **kw))
    for ch in (3, 257):
        with pytest.raises(NotImplementedError, match="output_ch"):
            r.set_network(0, nwe_amd.synthetic.make_state_dict(3, 2, 8, use_view_dirs=False, output_ch=ch))
    assert r.flops_per_eval(0) == flops and r.shapes[0] == (5, 16, 15, 9, 1)
    r.close()
