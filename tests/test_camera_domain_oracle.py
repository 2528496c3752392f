"""The camera cases of tests/camera_domain.py on the CPU: the oracle reproduces the reference's recorded rays
(tests/golden/cameras.npz, written by oracle/make_goldens.py from nerf/rays/rays.py), a numpy restatement of the arithmetic
csrc/nwe_device.h documents reproduces the oracle, and the table is ALIVE: every case differs in bits from the control camera
and from the wrong twins it names, every twin is told apart by some case, and every kind of case is there.  A table that could
not tell a swap from the truth fails here, without a GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import camera_domain as CD

F = np.float32


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cameras.npz"))


def test_table_is_well_formed():
    assert len(set(CD.NAMES)) == len(CD.NAMES)
    for c in CD.CASES:
        assert c.poses.dtype == F and c.poses.shape[1:] == (4, 4) and c.poses.shape[0] >= 1, c.name
        assert np.isfinite(c.poses).all(), c.name
        assert all(np.isfinite(v) for v in (c.fx, c.fy, c.cx, c.cy, c.near, c.far)) and F(c.fx) != 0 and F(c.fy) != 0, c.name
        r0, r1 = c.window
        assert 0 <= r0 < r1 <= c.H and c.W >= 1 and c.near <= c.far, c.name
        assert c.n_rays <= CD.MAX_GOLDEN_RAYS, (c.name, c.n_rays)              # the golden holds every ray
        assert c.n_poses * c.H * c.W <= 2 * CD.MAX_GOLDEN_RAYS, c.name
        assert set(c.catches) <= set(CD.TWINS), c.name
        assert not c.tiled or c.H % 3 != 0, c.name                            # tile borders where shard_rows puts them for a remainder
    assert CD.CASES[0] is CD.CONTROL and CD.CONTROL.kind == "control"
    assert (CD.CONTROL.fx, CD.CONTROL.fy, CD.CONTROL.cx, CD.CONTROL.cy) == O.intrinsics(CD.CONTROL.H, CD.CONTROL.W)


def test_table_covers_every_kind():
    have = {c.kind for c in CD.CASES}
    assert have == set(CD.KINDS), (set(CD.KINDS) - have, have - set(CD.KINDS))
    by = {k: [c for c in CD.CASES if c.kind == k] for k in CD.KINDS}
    # what each kind promises, checked on the numbers themselves
    assert all(c.fx != c.fy and c.H == c.W and c.cx == c.cy for c in by["focal-square"])
    assert all(c.fx != c.fy and c.H != c.W for c in by["focal-nonsquare"])
    assert all(c.fx < 0 < c.fy for c in by["neg-fx"]) and all(c.fy < 0 < c.fx for c in by["neg-fy"])
    assert all(c.fx < 0 and c.fy < 0 for c in by["neg-both"])
    assert all(c.cx != int(c.cx) and c.cy != int(c.cy) and c.cx != (c.W - 1) / 2 for c in by["pp-offcentre"])
    for c in by["pp-integer-posfx"] + by["pp-integer-negfx"]:
        assert c.cx == int(c.cx) and c.cy == int(c.cy) and 0 <= c.cx < c.W and 0 <= c.cy < c.H
        assert (c.fx < 0) == (c.kind == "pp-integer-negfx")
    assert all(c.cx < 0 and c.cy > c.H for c in by["pp-outside-low"]) and all(c.cx > c.W and c.cy < 0 for c in by["pp-outside-high"])
    assert {F(c.fx) for c in by["inexact-quotient"]} | {F(c.fy) for c in by["inexact-quotient"]} >= {F(3.0), F(7.0), F(CD.F400)}
    assert all(c.fx == c.fy == 1e5 for c in by["telephoto"]) and all(c.fx == c.fy == 0.05 for c in by["wide"])
    assert [(c.H, c.W) for c in by["frame-1x1"]] == [(1, 1)]
    assert all(c.H == 1 and c.W == 37 for c in by["frame-1xW"]) and all(c.H == 37 and c.W == 1 for c in by["frame-Hx1"])
    assert all(c.H == 3 and c.W in (127, 129) for c in by["frame-wide-row"])
    for c in by["batch-window"]:
        assert c.n_poses == 5 and 0 < c.window[0] and c.window[1] < c.H
        assert all(not np.array_equal(c.poses[i], c.poses[j]) for i in range(5) for j in range(i))
    for c in by["general-linear"] + by["general-shear"]:
        R = c.poses[0, :3, :3]
        assert len(set(np.abs(R).ravel().tolist())) == 9 and (R > 0).any() and (R < 0).any()
    norms = np.linalg.norm(by["general-linear"][0].poses[0, :3, :3].astype(np.float64), axis=0)
    assert np.allclose(norms, (0.01, 1.0, 30.0), rtol=2e-2), norms
    for c in by["axis-aligned"]:
        R = c.poses[:, :3, :3]
        assert set(np.abs(R).ravel().tolist()) == {0.0, 1.0} and (np.signbit(R) & (R == 0)).any() and (~np.signbit(R) & (R == 0)).any()
        assert np.allclose(np.abs(np.linalg.det(R.astype(np.float64))), 1.0)
    g, clean = (CD.BY_NAME[n] for n in CD.GARBAGE_PAIR)
    assert g.poses[0, 3].tolist() == [7.0, 8.0, 9.0, 10.0] and clean.poses[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(g.poses[:, :3], clean.poses[:, :3]) and g.camera() == clean.camera() and (g.H, g.W) == (clean.H, clean.W)
    assert all(np.abs(c.poses[:, :3, 3]).max() == 1e4 for c in by["large-translation"])


def test_signed_zeros_are_in_the_table():
    """The integer principal point gives (w - cx) == +0 exactly; a negative fx turns it into x = -0.  With the skew pose both
    reach the direction as m0 * (+-0), whose sign the sum with the next product absorbs, so the zero sign shows in the
    camera-plane coordinate itself: asserted there, on the restated seed."""
    pos, neg = CD.BY_NAME["pp-integer-posfx"], CD.BY_NAME["pp-integer-negfx"]
    for c, negative in ((pos, False), (neg, True)):
        x = (np.arange(c.W, dtype=F) - F(c.cx)) / F(c.fx)
        i = int(c.cx)
        assert x[i] == 0 and bool(np.signbit(x[i])) == negative, (c.name, x[i])
    # and the axis-aligned poses carry products with -0.0 entries into the sums: directions with exact zeros of both signs
    d = CD.oracle_rays(CD.BY_NAME["axis-aligned"])[:, 3:6]
    assert ((d == 0) & ~np.signbit(d)).any(), "no +0 direction component in the axis-aligned case"


def test_hybrid_case_puts_the_second_launch_inside_a_row():
    for cus in (256, 304, 228, 120, 104, 64, 8):
        c = CD.hybrid_case(cus)
        first = cus * CD.RAYS_PER_WORKGROUP
        per_pose = (c.window[1] - c.window[0]) * c.W
        assert c.n_poses == 3 and 0 < c.window[0] and c.window[1] < c.H
        assert first < c.n_rays < 2 * first, (cus, c.n_rays)                   # one full round and less than one more
        assert first // per_pose == 2 and (first % per_pose) % c.W != 0, cus   # ray_first: last pose, in the middle of a row
        assert (c.cx, c.cy) != ((c.W - 1) / 2, (c.H - 1) / 2) and c.fx != c.fy
    c = CD.hybrid_case(256)
    assert (c.H, c.W, c.window, c.n_rays) == (120, 111, (10, 110), 33300)


@pytest.mark.parametrize("name", CD.NAMES)
def test_oracle_reproduces_the_reference_rays(name, gold):
    """11 columns, and 8 (use_view_dirs=False): the reference's 8-column rays are the first 8 of its 11, which
    oracle/make_goldens.py asserted when it wrote the file."""
    c = CD.BY_NAME[name]
    assert CD.same_bits(gold[f"pose_{name}"], c.poses), "the table's pose is not the recorded one"
    assert gold[f"camera_{name}"].tolist() == [c.H, c.W, c.fx, c.fy, c.cx, c.cy, c.near, c.far]
    ref = gold[f"rays_{name}"]
    assert ref.shape == (c.n_poses, c.H * c.W, 11) and np.isfinite(ref).all()
    assert (np.abs(ref[..., 3:6]).max(-1) > 0).all()                           # no zero direction (tests/input_domain.py's)
    assert CD.same_bits(CD.oracle_frames(c, True), ref)
    assert CD.same_bits(CD.oracle_frames(c, False), ref[..., :8])
    assert bool(gold["eight_columns_are_the_first_eight"])


@pytest.mark.parametrize("name", CD.NAMES)
def test_restated_device_arithmetic_reproduces_the_oracle(name):
    c = CD.BY_NAME[name]
    for vd in (True, False):
        got, ref = CD.restated_rays(c, None, vd), CD.oracle_rays(c, vd)
        bad = np.flatnonzero((CD.bits(got) != CD.bits(ref)).any(-1))
        assert bad.size == 0, (name, vd, bad[:5], got[bad[:2]], ref[bad[:2]])


def test_restated_arithmetic_on_the_hybrid_frame():
    c = CD.hybrid_case(256)
    assert CD.same_bits(CD.restated_rays(c), CD.oracle_rays(c))


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic, on operands chosen to sit on double-rounding cases and at random."""
    from fractions import Fraction
    rng = np.random.Generator(np.random.Philox(key=[77, 0]))
    a = rng.standard_normal(400).astype(F)
    b = rng.standard_normal(400).astype(F)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-9, 3, 400)).astype(F)
    # ties of the fp32 rounding that only the sticky bits of the product decide
    a[:4], b[:4] = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12)                        # product 1 + 2^-11 + 2^-24
    c[:4] = (F(2.0 ** -40), F(-2.0 ** -40), F(2.0 ** -60), F(-2.0 ** -60))
    got = CD.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F(float(exact))                                                  # a double-rounded candidate: fix it up exactly
        cands = sorted({float(np.nextafter(lo, F(-np.inf))), float(lo), float(np.nextafter(lo, F(np.inf)))})
        dist = [abs(Fraction(v) - exact) for v in cands]
        best = min(dist)
        winners = [v for v, d in zip(cands, dist) if d == best]
        if len(winners) == 2:                                                 # a true tie: to even
            winners = [v for v in winners if (np.array(v, dtype=F).view(np.int32) & 1) == 0]
        assert float(got[i]) == winners[0], (i, a[i], b[i], c[i], got[i], winners)


# ------------------------------------------------------------------------------------------------------------------------
# liveness
# ------------------------------------------------------------------------------------------------------------------------

def _control_on(c):
    """The control camera on the case's frame: the 90-degree family and the control pose, repeated per pose of the case."""
    fx, fy, cx, cy = O.intrinsics(c.H, c.W)
    poses = np.repeat(CD.CONTROL.poses, c.n_poses, axis=0)
    full = O.create_rays(torch.from_numpy(poses), c.H, c.W, fx, fy, cx, cy, c.near, c.far, True).numpy()
    return CD.window_of(full, c)


@pytest.mark.parametrize("name", CD.NAMES[1:])
def test_case_differs_from_the_control(name):
    c = CD.BY_NAME[name]
    mine, ctrl = CD.oracle_rays(c), _control_on(c)
    assert mine.shape == ctrl.shape
    # not every ray: a pixel on the principal point looks along the pose's third column whatever the focal lengths are
    differing = int((CD.bits(mine[:, 3:6]) != CD.bits(ctrl[:, 3:6])).any(-1).sum())
    assert 2 * differing > mine.shape[0], f"{differing} of {mine.shape[0]} rays differ from the control camera's"


@pytest.mark.parametrize("name", CD.NAMES)
def test_case_tells_its_twins_apart(name):
    c = CD.BY_NAME[name]
    truth = CD.restated_rays(c)
    for twin in c.catches:
        wrong = CD.restated_rays(c, twin)
        differing = int((CD.bits(wrong) != CD.bits(truth)).any(-1).sum())
        assert differing > 0, f"{name} cannot tell {twin} from the truth"


def test_every_twin_is_told_apart_by_some_case():
    seen = {t: [] for t in CD.TWINS}
    for c in CD.CASES:
        truth = CD.restated_rays(c)
        for t in CD.TWINS:
            n = int((CD.bits(CD.restated_rays(c, t)) != CD.bits(truth)).any(-1).sum())
            if n:
                seen[t].append((c.name, n))
    for t, where in seen.items():
        print(f"{t}: {len(where)} of {len(CD.CASES)} cases differ; most rays in {max(where, key=lambda x: x[1]) if where else None}")
        assert where, f"no case of the table tells {t} from the truth"
    named = {t for c in CD.CASES for t in c.catches}
    assert named == set(CD.TWINS), set(CD.TWINS) - named
    # the twins that need a particular kind of case are caught by that kind alone
    assert {n for n, _ in seen["no_row_begin"]} == {c.name for c in CD.CASES if c.rows is not None}
    assert {n for n, _ in seen["row3"]} == {"row3-garbage"}
    assert {n for n, _ in seen["no_zero_start"]} == {"axis-aligned"}


def test_reciprocal_multiply_differs_on_the_inexact_quotients():
    for c in (x for x in CD.CASES if x.kind == "inexact-quotient"):
        w, h = np.arange(c.W, dtype=F), np.arange(c.H, dtype=F)
        for v, p, f in ((w, F(c.cx), F(c.fx)), (h, F(c.cy), F(c.fy))):
            q, r = (v - p) / f, (v - p) * (F(1) / f)
            if f == F(3.0) or f == F(7.0) or f == F(CD.F400):
                assert (CD.bits(q) != CD.bits(r)).any(), (c.name, float(f))
                assert (q.astype(np.float64) * np.float64(f) != (v - p).astype(np.float64)).any(), (c.name, float(f))   # inexact


def test_garbage_bottom_row_changes_nothing():
    g, clean = (CD.BY_NAME[n] for n in CD.GARBAGE_PAIR)
    assert CD.same_bits(CD.oracle_rays(g), CD.oracle_rays(clean))
    assert CD.same_bits(CD.restated_rays(g), CD.restated_rays(clean))
