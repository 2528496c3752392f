"""tests/lean_domain.py without a GPU: the shape list against tests/test_gpu_accuracy.py and csrc/nwe_mfma_shapes.h, the frames
the rules give at 256 and 304 CUs against the planner (nwe_debug_plan on host-only contexts: plan, tail, blocks, and with the
tail taken that the tail kernels of the shape are built), and the conditions under which the judged rays test anything, from the
CPU oracle alone.  Every test prints the figures it asserts."""
import ctypes as C
import os
import re

import pytest

import nwe_amd
from nwe_amd import _lib
from tests import lean_domain as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (256, 304)


# ---- the shape list -------------------------------------------------------------------------------------------------------------

def test_shape_list_is_the_accuracy_tests_and_the_headers():
    from tests import test_gpu_accuracy as A
    from tests import mode_domain as M
    assert L.SHAPES == A.INSTANTIATIONS and len(set(L.SHAPES)) == 14 and len(set(L.IDS)) == 14
    assert [s for s in L.SHAPES if s[2] != "reference"] == M.SHAPES
    text = open(os.path.join(ROOT, "nerf-workspaces-explorer_amd", "csrc", "nwe_mfma_shapes.h")).read()
    entries = re.findall(r"\bX\((\d+), (\d+), (-?\d+), (kForm\w+)\)", text)
    print("nwe_mfma_shapes.h:", entries)
    assert len(entries) == 14
    assert sorted((int(D), int(W), L.FORM_TOKENS[form]) for W, D, _, form in entries) == sorted(L.SHAPES)
    assert all(int(skip) == (4 if int(D) > 4 else -1) for _, D, skip, _ in entries)
    assert set(L.LONG_SHAPES) <= set(L.SHAPES) and len({s[2] for s in L.LONG_SHAPES}) == 2    # the reference form has no third
    assert [L.density_only(*s) for s in L.SHAPES if s[2] != "reference"] == [M.density_only(*s) for s in M.SHAPES]


def test_frames_by_rule():
    """What the rules give at 256 CUs is what the issue names; at every CU count of the planner's table they give a frame."""
    assert L.surplus(256) == 64 and L.surplus(304) == 80
    assert L.ragged(256) == (64, 19, 1831) and 19 * 1831 == 34789
    assert L.blocked(256) == (16, 160, 208)
    assert L.one_past(256)[0] == 65 and L.one_past(304)[0] == 81
    assert L.hollow_frame(256) == (51, (379, 422))
    for cus in (8, 64, 104, 120, 228, 256, 304):
        s = L.surplus(cus)
        k, H, W = L.ragged(cus)
        assert 1 <= k <= s and H * W == cus * 128 + (k - 1) * 32 + 5 and max(H, W) < 8192 and W % 8
        kb, Hb, Wb = L.blocked(cus)
        assert 1 <= kb <= s and Hb * Wb == cus * 128 + kb * 32 and Hb % 4 == 0 and Wb % 8 == 0 and max(Hb, Wb) < 8192
        kp, Hp, Wp = L.one_past(cus)
        assert kp > s and Hp * Wp == cus * 128 + (kp - 1) * 32 + 5 and max(Hp, Wp) < 8192
        print(f"{cus} CUs: surplus {s}, ragged {H} x {W} (k {k}), blocked {Hb} x {Wb} (k {kb}), one past {Hp} x {Wp} (k {kp}), "
              f"hollow {L.hollow_frame(cus)}")
    idx = L.judged(256, 34789)
    assert len(idx) == 389 and list(idx[128:130]) == [256 * 128 - 128, 256 * 128 - 127] and idx[-1] == 34788 and idx[-69] == 34720


# ---- the planner ----------------------------------------------------------------------------------------------------------------

def _renderer(monkeypatch, D, W, form, sampling):
    for name in ("NWE_WORK_QUEUE", "NWE_WORK_QUEUE_BACKFILL", "NWE_WORK_QUEUE_TAIL", "NWE_PACKET_BLOCKS", "NWE_COLOUR_SKIP"):
        monkeypatch.delenv(name, raising=False)
    r = nwe_amd.Renderer(host_only=True)
    r.debug_set_fold(L.fold(form))
    sd_c, sd_f = L.nets(D, W, form)
    r.set_network(0, sd_c)
    r.set_network(1, sd_f)
    r.set_sampling(*sampling)
    return r


def _plan(r, H, W, outputs, precision, cus):
    report = _lib.PlanReport()
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, H, W, 0, H, -1, C.byref(_lib.Outputs(**{k: 1 for k in outputs})), 0,
                                    _lib.PRECISIONS[precision], cus, C.byref(report))
    assert rc == 0, _lib.load().nwe_last_error(r._ctx).decode()
    return report.main, r.debug_last_packet_blocks()


def _stage(m):
    return dict(plan=m.plan, n_launches=m.n_launches, rays=tuple(m.rays), split=tuple(m.split), items=tuple(m.items), grid=tuple(m.grid),
                tail=m.tail, tail_items=m.tail_items, fork=m.fork)


@pytest.mark.parametrize("D,W,form", L.SHAPES, ids=L.IDS)
def test_the_planner_takes_the_path_on_every_shape(monkeypatch, D, W, form):
    """Mode 1, hybrid plan forced, as the GPU file runs: ragged and blocked take the tail with k items - which the planner
    grants only where the shape's tail kernels are built (nwe_plan.cpp: tail_built, from mfma_variant_built) - blocks off and
    on; one past is the hybrid plan's two launches, nothing stolen; the FULL frame of the reference is neither queued onto the
    tail nor blocked."""
    for sampling in L.samplings(D, W, form):
        r = _renderer(monkeypatch, D, W, form, sampling)
        try:
            r.debug_set_decomposition(2)
            r.debug_set_work_queue(1)
            for cus in CUS:
                for precision in L.PRECISIONS:
                    ctx = (L.kind(D, W, form), sampling, cus, precision)
                    for name, (k, H, Wd), blocks in (("ragged", L.ragged(cus), 0), ("blocked", L.blocked(cus), 1)):
                        m, was = _plan(r, H, Wd, L.LEAN, precision, cus)
                        print(*ctx, name, (H, Wd), _stage(m), "blocks", was)
                        assert (m.active, m.variant, m.plan, m.n_launches, m.tail, m.tail_items, m.fork) == (1, 0, 2, 2, 1, k, 2), (ctx, name)
                        assert tuple(m.items) == (cus, k) and tuple(m.grid) == (L.grid(cus), L.grid(k)) and tuple(m.split) == (0, 1), (ctx, name)
                        assert tuple(m.rays) == (cus * 128, H * Wd - cus * 128) and was == blocks, (ctx, name)
                        full, was = _plan(r, H, Wd, L.FULL, precision, cus)
                        assert (full.plan, full.tail, full.tail_items, was) == (2, 0, 0, 0) and tuple(full.items) == (cus, k), (ctx, name)
                    k, H, Wd = L.one_past(cus)
                    m, was = _plan(r, H, Wd, L.LEAN, precision, cus)
                    print(*ctx, "one past", (H, Wd), _stage(m), "blocks", was)
                    assert (m.plan, m.n_launches, m.tail, m.tail_items, m.fork, was) == (2, 2, 0, 0, 1, 0), ctx
                    assert tuple(m.items) == (cus, k) and tuple(m.grid) == (L.grid(cus), L.grid(k)) and tuple(m.split) == (0, 1), ctx
                    assert tuple(m.rays) == (cus * 128, H * Wd - cus * 128), ctx
                    # static dealing, the reference's: no grid, no tail
                    r.debug_set_work_queue(0)
                    m, _ = _plan(r, *L.ragged(cus)[1:], L.LEAN, precision, cus)
                    assert (m.plan, m.tail, tuple(m.grid)) == (2, 0, (0, 0)), ctx
                    r.debug_set_work_queue(1)
        finally:
            r.close()


# ---- the scenes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,W,form", L.SHAPES, ids=L.IDS)
def test_the_judged_rays_can_tell(D, W, form):
    """On the 389 judged rays of the ragged frame at 256 CUs, per sampling: the project's own rule leaves out at most 2 % of them,
    the fp64 colour varies (std >= 0.01: a wrong or missing colour moves the statistics), the depth is not constant."""
    for sampling in L.samplings(D, W, form):
        f = L.scene_figures(256, D, W, form, sampling)
        print(f"{L.kind(D, W, form)} {sampling[0]}+{sampling[1]} white {L.WHITE[sampling]}: {f['left_out']} of {f['rays']} rays left out, "
              f"rgb std {f['rgb_std']:.3f}, depth spread {f['depth_spread']:.3f}, mean acc {f['acc_mean']:.3f}")
        assert f["rays"] == 389 and f["left_out"] <= 0.02 * f["rays"]
        assert f["rgb_std"] >= 0.01
        assert f["depth_spread"] > 0.0


@pytest.mark.parametrize("shape", ["4x256", "8x128", "8x256", "4x128"])
def test_the_hollow_rows_take_the_tail(monkeypatch, shape):
    """The rows of the 800-wide frame of tests/hollow_domain.py that the GPU file renders: the tail with k items at 256 and 304 CUs,
    linear packets (the row counts are no multiples of 4)."""
    from tests import hollow_domain as H
    D, W = H.SHAPES[shape]
    r = _renderer(monkeypatch, D, W, "folded", H.RAGGED)
    try:
        r.debug_set_decomposition(2)
        r.debug_set_work_queue(1)
        for cus in CUS:
            k, (row0, row1) = L.hollow_frame(cus)
            for precision in L.PRECISIONS:
                report = _lib.PlanReport()
                rc = _lib.load().nwe_debug_plan(r._ctx, 1, H.SIZE, H.SIZE, row0, row1, -1, C.byref(_lib.Outputs(rgb=1, depth=1, acc=1)), 0,
                                                _lib.PRECISIONS[precision], cus, C.byref(report))
                m = report.main
                print(shape, cus, precision, (row0, row1), _stage(m), "blocks", r.debug_last_packet_blocks())
                assert rc == 0 and (m.plan, m.tail, m.tail_items) == (2, 1, k) and tuple(m.items) == (cus, k)
                assert H.SIZE * (row1 - row0) == cus * 128 + k * 32 and r.debug_last_packet_blocks() == ((row1 - row0) % 4 == 0)
    finally:
        r.close()
