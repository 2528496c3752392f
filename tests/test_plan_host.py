"""The launch planner without a GPU (csrc/nwe_plan.cpp through nwe_debug_plan, include/nwe.h): plain C++ that compiles without
ROCm; its plans at every CU count against a recording of the arithmetic it replaced (tests/golden/plan_table.npz, whose header
says which commit's code produced it and how - a recording of this project's own earlier code, never of the code under test);
invariants of a plan over the same grid; the call-level decisions from context state; the refusals of the real calls; the chunks
and the scratch of a sparse frame (plan_sparse) against the arithmetic of the two calls that each formed them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import nwe_amd
from nwe_amd import _lib, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-workspaces-explorer_amd", "csrc")
OFF, PRODUCER, CONSUMER = 0, 1, 2
PLAIN, TERM, SHARE = 0, 1, 2
REPORT = np.dtype(_lib.PlanReport)


def _grid(n):
    return (n + (n + 3) // 4 + 7) // 8 * 8


def _items(rays, split):
    return -(-rays // (32 if split else 128))


def _renderer(monkeypatch, side=1, tail=1, fold=True, nets=("4x128", "4x128"), ns=8, ni=8):
    monkeypatch.delenv("NWE_WORK_QUEUE", raising=False)
    monkeypatch.setenv("NWE_WORK_QUEUE_BACKFILL", str(side))
    monkeypatch.setenv("NWE_WORK_QUEUE_TAIL", str(tail))
    r = nwe_amd.Renderer(host_only=True)
    r.debug_set_fold(fold)
    shapes = {"4x128": dict(D=4, W=128), "8x256": dict(D=8, W=256)}
    for which, net in enumerate(nets):
        r.set_network(which, synthetic.make_state_dict(1000 + which, **shapes[net]))
    r.set_sampling(ns, ni)
    return r


def _outputs(*names):
    """nwe_outputs of which only null / non-null is read."""
    return _lib.Outputs(**{k: 1 for k in names})


def _plan(r, n_rays, outputs=("rgb",), cus=256, pinhole=True, hooks=0, precision=_lib.PREC_F16X3, report=None):
    """(rc, report) of nwe_debug_plan for a frame of 1 x n_rays pixels, or for n_rays precomputed rays."""
    report = _lib.PlanReport() if report is None else report
    rc = _lib.load().nwe_debug_plan(r._ctx, 1, 1, n_rays, 0, 1, -1 if pinhole else n_rays, C.byref(_outputs(*outputs)), hooks, precision, cus,
                                    C.byref(report))
    return rc, report


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def test_the_planner_compiles_without_rocm(tmp_path):
    """nwe_plan.cpp is plain C++17: g++ with every warning an error and no ROCm include path (as test_abi.py compiles abi_smoke.c)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(CSRC, "nwe_plan.cpp"), "-o", str(tmp_path / "nwe_plan.o")], check=True)
    for name in ("nwe_plan.cpp", "nwe_plan.h"):
        assert "hip" not in open(os.path.join(CSRC, name)).read().replace("HIP", "").replace(".hip", ""), name
    # the sparse frame's plan is declared there, constant included, and nowhere beside it: the HIP headers take it from the planner
    header = open(os.path.join(CSRC, "nwe_plan.h")).read()
    for declared in ("constexpr int64_t kSparseChunkSamples = (int64_t)1 << 22;", "struct SparsePlan {", "SparsePlan plan_sparse(int64_t n_rays, int S, int chunk_hook);"):
        assert declared in header, declared
    assert "kSparseChunkSamples =" not in open(os.path.join(CSRC, "nwe_host.h")).read()


# plan_sparse's fields in the order tests/c/sparse_plan_smoke.cpp prints them
KEYS = ("cap", "chunks", "M", "at_grid", "at_rows", "at_z", "at_points", "at_dirs", "at_offsets", "at_total", "at_mask", "bytes")
REGIONS = KEYS[3:11]
# (n_rays, S, hook): one ray; M = 432, whose 4 M = 1 728 bytes round up to 1 792; three chunks, the last of 5 rays; one chunk against two
# at 2^22 // 192 = 21 845 rays; the largest legal S = 128 + 256; a hook above the cap; a hook of one ray
SPARSE_CASES = ((1, 1, 0), (27, 16, 0), (133, 16, 64), (21845, 192, 0), (21846, 192, 0), (2560, 384, 0), (100, 16, 1000), (100, 16, 1))


def _sparse_plan_of_the_parent(n_rays, S, hook):
    """The chunk size and the scratch layout as nwe_render_sparse and nwe_render_sparse_async of commit 4becc22 formed them, each for
    itself (csrc/nwe_abi.hip there: `cap`, the `take` lambda, at_grid .. at_mask, the loop `first += cap`), restated."""
    cap = max(1, (1 << 22) // S)
    if hook > 0:
        cap = min(cap, hook)
    cap = min(cap, n_rays)
    M = cap * S
    plan, size = {"cap": cap, "chunks": -(-n_rays // cap), "M": M}, 0
    for name, n in zip(REGIONS, (M * 16, M * 16, M * 4, M * 12, M * 12, cap * 4, 4, M)):
        plan[name] = size
        size += (n + 255) // 256 * 256
    plan["bytes"] = size
    return plan, dict(zip(REGIONS, (M * 16, M * 16, M * 4, M * 12, M * 12, cap * 4, 4, M)))


def test_the_sparse_plan_is_the_arithmetic_it_replaced(tmp_path):
    """tests/c/sparse_plan_smoke.cpp - the host compiler, every warning an error, no ROCm include path, nwe_plan.cpp alone - prints
    plan_sparse at the smallest inputs at which it can go wrong; every field against the restatement of the code it replaced."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sparse_plan_smoke")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "c", "sparse_plan_smoke.cpp"),
                    os.path.join(CSRC, "nwe_plan.cpp"), "-o", exe], check=True)
    words = [str(v) for case in SPARSE_CASES for v in case]
    done = subprocess.run([exe] + words, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    piped = subprocess.run([exe], input=" ".join(words), capture_output=True, text=True)
    assert piped.returncode == 0 and piped.stdout == done.stdout
    lines = done.stdout.splitlines()
    assert len(lines) == len(SPARSE_CASES)
    for case, line in zip(SPARSE_CASES, lines):
        got = dict(zip(KEYS, (int(v) for v in line.split())))
        want, sizes = _sparse_plan_of_the_parent(*case)
        assert len(line.split()) == len(KEYS) and got == want, (case, got, want)
        # ascending, 256-aligned, no region reaches into the next, bytes is the end of the last
        ends = [got[name] + sizes[name] for name in REGIONS]
        starts = [got[name] for name in REGIONS]
        assert starts[0] == 0 and all(s % 256 == 0 for s in starts), (case, got)
        assert all(end <= nxt and start < nxt for start, end, nxt in zip(starts, ends, starts[1:])), (case, got)
        assert ends[-1] <= got["bytes"] < ends[-1] + 256 and got["bytes"] % 256 == 0, (case, got)
    by_case = {case: dict(zip(KEYS, (int(v) for v in line.split()))) for case, line in zip(SPARSE_CASES, lines)}
    assert by_case[27, 16, 0]["M"] == 432 and by_case[27, 16, 0]["at_points"] - by_case[27, 16, 0]["at_z"] == 1792
    assert (by_case[133, 16, 64]["cap"], by_case[133, 16, 64]["chunks"], 133 - 2 * 64) == (64, 3, 5)
    assert (by_case[21845, 192, 0]["chunks"], by_case[21846, 192, 0]["chunks"], by_case[21846, 192, 0]["cap"]) == (1, 2, 21845)
    assert by_case[2560, 384, 0]["cap"] == 2560 and by_case[100, 16, 1000]["cap"] == 100 and by_case[100, 16, 1]["chunks"] == 100


@pytest.fixture(scope="module")
def table():
    t = np.load(os.path.join(ROOT, "tests", "golden", "plan_table.npz"))
    assert "5270fef" in str(t["header"])
    rows = t["rows"].astype(np.int64)
    return {name: rows[:, i] for i, name in enumerate(t["columns"])}


def _stage_columns(stage):
    """The columns of the table, from the stage records of a report array."""
    cols = {"plan": stage["plan"], "fork": stage["fork"], "tail_items": stage["tail_items"]}
    for l in (0, 1):
        cols.update({f"first{l}": stage["ray_first"][:, l], f"rays{l}": stage["rays"][:, l], f"split{l}": stage["split"][:, l],
                     f"items{l}": stage["items"][:, l], f"grid{l}": stage["grid"][:, l]})
    return cols


def _walk(monkeypatch, table):
    """Every row of the table through nwe_debug_plan: yields (rows, stage records) per group of rows that one context state serves.
    Role off: a fused call.  Producer / consumer: the two stages of separate passes, sharing kernels when lean, full kernels otherwise."""
    call = _lib.load()["nwe_debug_plan"]   # a handle of this walk's own, which takes the report's address as a number
    call.restype, call.argtypes = C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_int64, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    outs = {1: C.byref(_outputs("rgb")), 0: C.byref(_outputs("rgb", "z_fine"))}
    names = ("side_ok", "tail_ok", "n_samples", "n_importance", "decomposition", "queue_mode")
    code = np.zeros(len(table["cus"]), dtype=np.int64)
    for k in names:
        code = code * 1024 + table[k] + 1
    order = np.argsort(code, kind="stable")
    starts = np.flatnonzero(np.diff(code[order], prepend=-1))
    renderers = {}
    try:
        for group in np.split(order, starts[1:]):
            key = side, tail, ns, ni, dec, qm = tuple(int(table[k][group[0]]) for k in names)
            if (side, tail) not in renderers:
                renderers[side, tail] = _renderer(monkeypatch, side, tail)
            r = renderers[side, tail]
            r.set_sampling(ns, ni); r.debug_set_decomposition(dec); r.debug_set_work_queue(qm)
            for separate in (0, 1):
                rows = group[(table["role"][group] != OFF) == bool(separate)]
                if not len(rows):
                    continue
                r.set_separate_passes(bool(separate))
                got = np.zeros(len(rows), dtype=REPORT)
                got["struct_bytes"] = REPORT.itemsize
                at, ctx = got.ctypes.data, r._ctx
                for n, lean, cus in zip(table["n_rays"][rows].tolist(), table["lean"][rows].tolist(), table["cus"][rows].tolist()):
                    if call(ctx, 1, 1, n, 0, 1, -1, outs[lean], 0, 0, cus, at) != 0:
                        raise AssertionError((n, lean, cus, key, _error(r)))
                    at += REPORT.itemsize
                producer = table["role"][rows] == PRODUCER
                stage = np.where(producer, got["coarse"], got["main"])
                yield rows, got, stage
    finally:
        for r in renderers.values():
            r.close()


@pytest.fixture(scope="module")
def walked(table):
    """The walk, once: (row indices, reports, the row's stage) concatenated in walk order."""
    with pytest.MonkeyPatch.context() as mp:
        parts = list(_walk(mp, table))
    rows = np.concatenate([p[0] for p in parts])
    assert sorted(rows) == list(range(len(table["cus"])))
    return rows, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def test_plans_equal_the_recorded_ones_at_every_cu_count(table, walked):
    rows, _, stage = walked
    assert set(np.unique(table["cus"])) == {8, 64, 104, 120, 228, 256, 304}
    assert (stage["active"] == 1).all() and (stage["role"] == table["role"][rows]).all()
    for name, got in _stage_columns(stage).items():
        bad = np.flatnonzero(got != table[name][rows])
        assert not len(bad), (name, {k: int(v[rows[bad[0]]]) for k, v in table.items()}, int(got[bad[0]]))
    assert ((stage["tail"] == 1) == (table["tail_items"][rows] > 0)).all()


def test_invariants_of_a_plan(table, walked):
    rows, report, s = walked
    t = {k: v[rows] for k, v in table.items()}
    two = s["plan"] == 2
    assert (s["n_launches"] == np.where(two, 2, 1)).all()
    # the launches partition [0, n_rays)
    assert (s["ray_first"][:, 0] == 0).all() and (s["rays"][:, 0] + s["rays"][:, 1] == t["n_rays"]).all()
    assert (s["ray_first"][two, 1] == s["rays"][two, 0]).all() and (s["rays"][~two, 1] == 0).all() and (s["rays"] >= 0).all()
    assert (s["split"][:, 0] == (s["plan"] == 1)).all() and (s["split"][two, 1] == 1).all()
    for l in (0, 1):   # items == mfma_workgroups(rays, split); grid is 0 or queue_grid(items)
        assert (s["items"][:, l] == -(-s["rays"][:, l] // np.where(s["split"][:, l] == 1, 32, 128))).all()
        n = s["items"][:, l].astype(np.int64)
        assert ((s["grid"][:, l] == 0) | (s["grid"][:, l] == (n + (n + 3) // 4 + 7) // 8 * 8)).all()
        assert (s["grid"][s["rays"][:, l] == 0, l] == 0).all()
    # no launch of a sharing stage (nor, below, of a terminating one) is queued; nor any launch under a role
    plain = (s["variant"] == PLAIN) & (t["role"] == OFF)
    assert (s["grid"][~plain] == 0).all() and (s["variant"][(t["role"] != OFF) & (t["lean"] == 1)] == SHARE).all()
    assert (s["variant"][t["lean"] == 0] == PLAIN).all()
    assert (report["may_queue"] == ((report["main"]["grid"] != 0).any(axis=1))).all()
    assert (report["need_side"] == (report["may_queue"] & t["side_ok"])).all()
    # the tail path: lean, plain, first launch queued, side stream on offer, allowed, and the surplus covers the split items
    tail = s["tail"] == 1
    surplus = s["grid"][:, 0].astype(np.int64) - s["items"][:, 0]
    want = two & plain & (t["lean"] == 1) & (s["grid"][:, 0] > 0) & (t["side_ok"] == 1) & (t["tail_ok"] == 1) & (s["rays"][:, 1] > 0) & \
        (surplus >= s["items"][:, 1])
    assert (tail == want).all() and tail.any()
    assert (s["tail_items"] == np.where(tail, s["items"][:, 1], 0)).all()
    forks = two & (t["side_ok"] == 1) & ((s["grid"] != 0).any(axis=1))
    assert (s["fork"] == np.where(tail, 2, np.where(forks, 1, 0))).all()
    assert (s["plan"][t["n_samples"] > 64] == 1).all()               # kPacketMaxSamples
    forced = (t["decomposition"] >= 0) & (t["n_samples"] <= 64)
    assert (s["plan"][forced] == t["decomposition"][forced]).all()
    # evaluations (include/nwe.h, nwe_last_ray_evaluations)
    ns, ni, n = t["n_samples"], t["n_importance"], t["n_rays"]
    assert (report["evals_full"] == n * (ns + np.where(ni > 0, ns + ni, 0))).all()
    coarse = report["coarse_launch"] == 1
    assert (report["evals_run"] == np.where(coarse, report["share_rays"] * ns + n * (ns + ni), report["evals_full"])).all()
    assert (report["share_rays"] == np.where(coarse, n, 0)).all() and (coarse == (t["role"] != OFF)).all()


def _flags(report):
    return tuple(int(getattr(report, k)) for k in ("separate", "share", "full", "coarse_launch", "may_queue"))


def test_call_level_decisions_from_context_state(monkeypatch):
    n = 256 * 128 + 160   # at 256 CUs: one round of packets and five split items - hybrid, queued, tail path
    r = _renderer(monkeypatch)
    try:
        r.debug_set_work_queue(1)
        rc, p = _plan(r, n)
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 1) and p.need_side and not p.need_evals and not p.table_elems
        assert (p.main.plan, p.main.tail, p.main.tail_items, p.main.fork, p.main.net, p.main.role) == (2, 1, 5, 2, -1, OFF)
        assert not p.coarse.active and p.evals_run == p.evals_full == n * 24
        rc, p = _plan(r, n, ("rgb", "z_fine"))                      # not lean: backfill, no tail
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 1) and (p.main.tail, p.main.fork) == (0, 1)
        rc, p = _plan(r, n, pinhole=False)                          # nwe_render_rays: never lean
        assert rc == 0 and (p.main.tail, p.main.fork, p.main.plan) == (0, 1, 2)
        rc, p = _plan(r, n, precision=_lib.PREC_F32)                # the fp32 launcher has no plan
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 0) and p.main.active and p.main.n_launches == 0
        # early termination: its own kernels, a zeroed counter, nothing queued
        r.set_early_termination(0.01)
        rc, p = _plan(r, n)
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 0) and p.need_evals and p.main.variant == TERM and list(p.main.grid) == [0, 0]
        r.set_early_termination(0.0)
        # shared coarse pass, k = 2 on a frame of one row: ceil(n / 2) representatives
        r.set_shared_coarse(2)
        rc, p = _plan(r, n)
        rep = (n + 1) // 2
        assert rc == 0 and _flags(p) == (0, 1, 0, 1, 0) and p.share_k == 2 and p.table_elems == rep * 8 and p.share_rays == rep
        assert (p.coarse.role, p.coarse.n_rays, p.coarse.variant, p.coarse.net) == (PRODUCER, rep, SHARE, -1)
        assert (p.main.role, p.main.n_rays, p.main.variant) == (CONSUMER, n, SHARE) and p.evals_run == rep * 8 + n * 16
        rc, p = _plan(r, n, precision=_lib.PREC_F32)
        assert rc == 0 and _flags(p) == (0, 1, 0, 1, 0)
        r.set_shared_coarse(1)
        # separate passes: lean -> sharing kernels at k = 1; an output beyond the lean ones -> the full kernels and a table
        r.set_separate_passes(True)
        rc, p = _plan(r, n)
        assert rc == 0 and _flags(p) == (1, 1, 0, 1, 0) and p.share_k == 1 and p.table_elems == n * 8 and not p.coarse_flags
        assert (p.coarse.net, p.main.net, p.coarse.n_importance) == (0, 1, 8)
        rc, p = _plan(r, n, ("rgb", "z_fine", "flags"))
        assert rc == 0 and _flags(p) == (1, 0, 1, 1, 0) and p.table_elems == n * 8 and p.coarse_flags
        assert (p.coarse.variant, p.main.variant, p.coarse.n_importance, p.coarse.role, p.main.role) == (PLAIN, PLAIN, 0, PRODUCER, CONSUMER)
        rc, p = _plan(r, n, ("rgb", "weights_coarse"))              # the caller's own table serves
        assert rc == 0 and _flags(p) == (1, 0, 1, 1, 0) and p.table_elems == 0 and not p.coarse_flags
        rc, p = _plan(r, n, pinhole=False, hooks=_lib.PLAN_HOOK_COARSE_WEIGHTS)   # the hook takes the coarse pass's place
        assert rc == 0 and _flags(p) == (1, 0, 1, 0, 0) and not p.coarse.active and p.share_rays == 0 and p.evals_run == p.evals_full
        rc, p = _plan(r, n, pinhole=False, hooks=_lib.PLAN_HOOK_OTHER)
        assert rc == 0 and _flags(p) == (1, 0, 1, 1, 0)
        rc, p = _plan(r, n, precision=_lib.PREC_F32)                # fp32 has no separate passes
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 0)
        r.set_sampling(8, 0)                                        # nor has a call without importance samples
        rc, p = _plan(r, n)
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 1)
        rc, p = _plan(r, 0, pinhole=False)                          # no rays: nothing planned
        assert rc == 0 and not p.main.active
    finally:
        r.close()
    r = _renderer(monkeypatch, fold=False)   # the unfolded formulation has no sharing kernels: a lean frame takes the full ones
    try:
        r.set_separate_passes(True)
        rc, p = _plan(r, n)
        assert rc == 0 and _flags(p) == (1, 0, 1, 1, 0) and (p.coarse.variant, p.main.variant) == (PLAIN, PLAIN)
        r.set_separate_passes(False)
        r.debug_set_work_queue(1)
        rc, p = _plan(r, n)                                         # ... but the plain kernels, their queue and their tail
        assert rc == 0 and _flags(p) == (0, 0, 0, 0, 1) and p.main.tail == 1
    finally:
        r.close()


def test_refusals_are_the_real_calls(monkeypatch):
    """Code and text of what nwe_render / nwe_render_rays refuse, in their order; a host-only context's own refusal aside."""
    lib = _lib.load()
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert lib.nwe_debug_plan(None, 1, 1, 8, 0, 1, -1, C.byref(_outputs("rgb")), 0, 0, 256, C.byref(_lib.PlanReport())) == _lib.NWE_ERR_INVALID
        assert lib.nwe_debug_plan(r._ctx, 1, 1, 8, 0, 1, -1, None, 0, 0, 256, C.byref(_lib.PlanReport())) == _lib.NWE_ERR_INVALID
        assert _error(r) == "null context or outputs"
        bad = _outputs("rgb"); bad.struct_bytes -= 8
        assert lib.nwe_debug_plan(r._ctx, 1, 1, 8, 0, 1, -1, C.byref(bad), 0, 0, 256, C.byref(_lib.PlanReport())) == _lib.NWE_ERR_INVALID
        assert "nwe_outputs.struct_bytes" in _error(r)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_STATE and _error(r) == "nwe_set_sampling has not been called"
        r.set_sampling(8, 8)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_STATE and _error(r) == "coarse network not set"
        r.set_network(0, synthetic.make_state_dict(1000, D=4, W=128))
        assert _plan(r, 8)[0] == _lib.NWE_ERR_STATE and _error(r) == "fine network not set but n_importance > 0"
    finally:
        r.close()
    r = _renderer(monkeypatch)
    try:
        assert _plan(r, 8, precision=7)[0] == _lib.NWE_ERR_INVALID and _error(r) == "unknown precision"
        small = _lib.PlanReport(); small.struct_bytes -= 8
        assert _plan(r, 8, report=small)[0] == _lib.NWE_ERR_INVALID and "nwe_plan_report.struct_bytes" in _error(r)
        assert _plan(r, 8, cus=0)[0] == _lib.NWE_ERR_INVALID
        assert lib.nwe_debug_plan(r._ctx, 1, 4, 8, 3, 2, -1, C.byref(_outputs("rgb")), 0, 0, 256, C.byref(_lib.PlanReport())) == _lib.NWE_ERR_INVALID
        assert _error(r) == "bad pose / image / row range"
        assert lib.nwe_debug_plan(r._ctx, 4, 1 << 15, 1 << 15, 0, 1 << 15, -1, C.byref(_outputs("rgb")), 0, 0, 256,
                                  C.byref(_lib.PlanReport())) == _lib.NWE_ERR_INVALID
        assert _error(r) == "more than 2^31 - 1 rays in one call"
        assert _plan(r, 1 << 31, pinhole=False)[0] == _lib.NWE_ERR_INVALID and _error(r) == "bad rays (null, or more than 2^31 - 1)"
        assert _plan(r, 8, ("rgb", "feat_map"))[0] == _lib.NWE_ERR_UNSUPPORTED and "feat_map (endpoint_feat) is computed by the NWE_PREC_F32 kernel only" == _error(r)
        r.set_early_termination(0.25)
        on = "early termination is on (nwe_set_early_termination, min_transmittance = 0.250000): "
        off = "; set min_transmittance to 0 for this call"
        assert _plan(r, 8, pinhole=False)[0] == _lib.NWE_ERR_UNSUPPORTED
        assert _error(r) == on + "nwe_render_rays, its hooks and its training tables are not terminated" + off
        assert _plan(r, 8, ("rgb", "z_fine"))[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == on + "only rgb / depth / acc / flags can be requested" + off
        r.set_separate_passes(True)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r).startswith(
            "separate passes are on (nwe_set_separate_passes): they are not built together with early termination")
        assert _plan(r, 8, precision=_lib.PREC_F32)[0] == _lib.NWE_OK
        r.set_separate_passes(False)
        r.set_shared_coarse(2)
        sharing = "the shared coarse pass is on (nwe_set_shared_coarse, k = 2): "
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == sharing + \
            "it is not built together with early termination (nwe_set_early_termination, min_transmittance = 0.250000); switch one of them off"
        r.set_early_termination(0.0)
        share_off = "; set shared_coarse to 1 for this call"
        assert _plan(r, 8, pinhole=False)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == sharing + "nwe_render_rays has no pixel grid to share over" + share_off
        assert _plan(r, 8, ("rgb", "disp"))[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == sharing + "only rgb / depth / acc / flags can be requested" + share_off
    finally:
        r.close()
    r = _renderer(monkeypatch, fold=False)
    try:
        r.set_shared_coarse(2)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == "the shared coarse pass is on (nwe_set_shared_coarse, k = 2): " \
            "a network packed unfolded (nwe_debug_set_fold(0)) has no sharing MFMA kernel; use NWE_PREC_F32; set shared_coarse to 1 for this call"
        r.set_shared_coarse(1)
        r.set_early_termination(0.5)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == "early termination is on (nwe_set_early_termination, min_transmittance = 0.500000): " \
            "a network packed unfolded (nwe_debug_set_fold(0)) has no terminating MFMA kernel; use NWE_PREC_F32; set min_transmittance to 0 for this call"
        r.set_early_termination(0.0)
        r.debug_set_fold(True)
        r.set_network(1, synthetic.make_state_dict(1001, D=4, W=128))
        r.set_separate_passes(True)
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == "separate passes are on (nwe_set_separate_passes): coarse and fine " \
            "networks must be packed in the same formulation (nwe_debug_set_fold); use NWE_PREC_F32; set separate_passes to 0 for this call"
    finally:
        r.close()
    r = _renderer(monkeypatch, nets=("4x128", "8x256"))   # one fused kernel cannot serve two shapes; separate passes can
    try:
        assert _plan(r, 8)[0] == _lib.NWE_ERR_UNSUPPORTED and _error(r) == "coarse and fine networks must have the same shape for the MFMA kernel"
        r.set_separate_passes(True)
        rc, p = _plan(r, 8)
        assert rc == _lib.NWE_OK and _flags(p)[:4] == (1, 1, 0, 1)
    finally:
        r.close()
