"""The asynchronous sparse frame without a GPU (include/nwe.h: nwe_render_sparse_async): every refusal in front of the host-only one
by code, text and order - the synchronous call's list, call by call; that a refused call writes nothing and moves no report; the grid
rule of the counted query launches; a numpy model of the counted kernels' strided walk; the handler's option; and the stand-alone C
program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nwe_amd
from nwe_amd import _lib, synthetic
from tests import radiance_grid as R

NAN = float("nan")


def _error(r):
    return _lib.load().nwe_last_error(r._ctx).decode()


def _set(r, kind="random"):
    g = R.grid(kind)
    r.set_radiance_grid(g["values"], g["lo"], g["hi"])


def _call(entry, r, out, poses=np.eye(4, dtype=np.float32), n_poses=1, H=4, W=5, fx=2., fy=2., near=0.1, far=5., rows=(0, 4), which=1,
          precision=_lib.PREC_F16X3, min_weight=1e-3, dilate=1):
    ptr = None if poses is None else poses.ctypes.data
    fn = getattr(_lib.load(), entry)
    return fn(r._ctx if r is not None else None, ptr, n_poses, H, W, fx, fy, 2., 1.5, near, far, rows[0], rows[1], which, precision,
              min_weight, dilate, None if out is None else C.byref(out), None)


def _reports(r):
    lib = _lib.load()
    counts = (C.c_int64 * 2)(-7, -7)
    return (lib.nwe_last_kernel_ms(r._ctx), lib.nwe_debug_last_plan(r._ctx), lib.nwe_last_query_ms(r._ctx), lib.nwe_last_grid_ms(r._ctx),
            lib.nwe_last_sparse_ms(r._ctx), lib.nwe_last_sparse_samples(r._ctx, counts), tuple(counts),
            lib.nwe_debug_last_sparse_host_waits(r._ctx))


def test_every_refusal_is_the_synchronous_calls_by_code_text_and_order():
    """Each call is made through both entry points on the same context; each is wrong in everything behind the refusal it expects."""
    r = nwe_amd.Renderer(host_only=True)
    I, S = _lib.NWE_ERR_INVALID, _lib.NWE_ERR_STATE
    bad = dict(which=2, precision=9, min_weight=NAN, dilate=9)

    def both(out, code, text, **kw):
        got = []
        for entry in ("nwe_render_sparse", "nwe_render_sparse_async"):
            rc = _call(entry, r, out, **kw)
            got.append((rc, _error(r)))
        assert got[0] == got[1], (kw, got)
        assert got[1][0] == code and (got[1][1] == text or (text.endswith("*") and got[1][1].startswith(text[:-1]))), (kw, got)

    try:
        buf = np.full(60, 123.0, np.float32)
        good = _lib.SparseOutputs(rgb=buf.ctypes.data)
        none = _lib.SparseOutputs(flags=1)
        stale = _lib.SparseOutputs(rgb=1)
        stale.struct_bytes = C.sizeof(_lib.SparseOutputs) - 8
        before = _reports(r)
        # 1. the context
        assert _call("nwe_render_sparse_async", None, None, poses=None, **bad) == I
        # 2. the outputs, in front of the camera (H = 0)
        both(None, I, "null outputs", H=0, **bad)
        both(stale, I, "nwe_sparse_outputs.struct_bytes != sizeof(nwe_sparse_outputs)*", H=0, **bad)
        both(none, I, "none of rgb / depth / acc / weights_coarse / z_fine / weights_grid / selected / raw_fine requested", H=0, **bad)
        for name in _lib.SPARSE_OUTPUT_FIELDS[:-1]:
            both(_lib.SparseOutputs(**{name: 1}), I, "bad pose / image / row range", H=0, **bad)
        # 3. the camera and the ray count
        for kw in (dict(poses=None), dict(n_poses=0), dict(H=0), dict(W=0), dict(rows=(-1, 4)), dict(rows=(0, 5)), dict(rows=(3, 2))):
            both(good, I, "bad pose / image / row range", **kw, **bad)
        for kw in (dict(fx=0.), dict(fy=-0.)):
            both(good, I, "fx and fy must be non-zero", **kw, **bad)
        both(good, I, "far < near: the sorted merge of the fine pass needs ascending depths", near=2., far=1., **bad)
        both(good, I, "more than 2^31 - 1 rays in one call", n_poses=3, H=30000, W=30000, rows=(0, 30000), **bad)
        # 4. to 7. the arguments of the call, each in front of the next
        for which in (2, -1):
            both(good, I, "which must be 0 or 1", **dict(bad, which=which))
        both(good, I, "unknown precision", **dict(bad, which=0))
        both(good, I, "sparse frame: min_weight must not be NaN", **dict(bad, which=1, precision=_lib.PREC_F32))
        for dilate in (9, -1):
            both(good, I, "sparse frame: dilate must be in 0..8", dilate=dilate)
        # 8. to 10. the state; zero rays and a host-only context do not come first
        no_grid = "sparse frame: no radiance grid is set (nwe_set_radiance_grid, nwe_bake_radiance_grid)"
        for kw in (dict(rows=(0, 4)), dict(rows=(2, 2)), dict(dilate=0, min_weight=-np.inf), dict(dilate=8, min_weight=np.inf)):
            both(good, S, no_grid, **kw)
        _set(r)
        both(good, S, "nwe_set_sampling has not been called")
        r.set_sampling(8, 8)
        both(good, S, "sparse frame: the fine network is not set")
        both(good, S, "sparse frame: the coarse network is not set", which=0)
        r.set_network(0, synthetic.make_state_dict(5, 3, 64, skips=()))     # a shape without an MFMA kernel; the upload clears the grid
        both(good, S, no_grid, which=0)
        _set(r)
        both(good, S, "sparse frame: the fine network is not set", which=1)
        # 11. the device - also for a call of zero rays
        for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
            for rows in ((0, 4), (2, 2)):
                both(good, S, "needs a device context", which=0, precision=precision, rows=rows)
        with pytest.raises(RuntimeError, match="nwe_render_sparse_async: needs a device context"):
            r.render_sparse(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., which=0, asynchronous=True)
        with pytest.raises(ValueError, match="unknown sparse outputs"):
            r.render_sparse(np.eye(4), 4, 5, fx=2., fy=2., cx=2., cy=1.5, near=0.1, far=5., outputs=("rgb", "disp"), asynchronous=True)
        # a refused call leaves the outputs and all reports untouched
        assert (buf == 123.0).all() and _reports(r) == before
        assert before[4] < 0 and before[5] == _lib.NWE_ERR_STATE and before[6] == (-7, -7) and before[7] == -1
        assert r.last_sparse_ms() is None and r.last_sparse_samples() is None and r.debug_last_sparse_host_waits() is None
        assert _lib.load().nwe_debug_last_sparse_host_waits(None) == -1
        assert {"nwe_render_sparse_async", "nwe_debug_last_sparse_host_waits", "nwe_debug_query_counted_grid"} <= set(_lib.SYMBOLS)
    finally:
        r.close()


# ---- the counted launches -------------------------------------------------------------------------------------------------------

def _grid(capacity, packet, forced=0, cus=256):
    return int(_lib.load().nwe_debug_query_counted_grid(capacity, packet, forced, cus))


@pytest.mark.parametrize("packet", [128, 16])
def test_the_counted_grid_rule(packet):
    """min(ceil(capacity / packet), 8 CUs); forced steps s: ceil(ceil(capacity / packet) / s)."""
    assert _grid(0, packet) == 0                                   # nothing is launched
    assert _grid(1, packet) == 1
    assert _grid(packet, packet) == 1 and _grid(packet + 1, packet) == 2
    for cus in (1, 4, 256):
        most = 8 * cus
        assert _grid(most * packet, packet, cus=cus) == most                   # exactly 8 CUs packets
        assert _grid(most * packet + 1, packet, cus=cus) == most               # above: the walk takes the rest
        assert _grid((most - 1) * packet + 1, packet, cus=cus) == most
        assert _grid((most - 1) * packet, packet, cus=cus) == most - 1
        assert _grid((1 << 21), packet, cus=cus) == min((1 << 21) // packet, most)
    for forced in (1, 2, 3, 7, 256):
        for capacity in (1, packet, packet + 1, 80 * packet, 81 * packet - 1, (1 << 21)):
            packets = -(-capacity // packet)
            assert _grid(capacity, packet, forced) == -(-packets // forced), (capacity, forced)   # whatever the CUs
            assert _grid(capacity, packet, forced, cus=1) == -(-packets // forced)
    assert _grid(0, packet, 3) == 0
    # the cases of tests/test_gpu_sparse_async.py
    assert _grid(10240, 128, 3) == 27 and _grid(1920, 16, 7) == 18


def _walk(n, grid, packet):
    """The counted kernels' walk in numpy: workgroup `item` visits packets item, item + grid, ... while packet * size < n; returns the
    visits per packet and the workgroups that returned before anything else."""
    packets = -(-n // packet) if n > 0 else 0
    visits = np.zeros(max(packets, 1) + 2 * grid + 2, np.int64)
    idle = 0
    for item in range(grid):
        if item * packet >= n:                 # the early return
            idle += 1
            continue
        p = item
        while p * packet < n:                  # the test at the top of a step
            visits[p] += 1
            p += grid
    return visits, idle


@pytest.mark.parametrize("grid", [1, 3, 4, 10])
@pytest.mark.parametrize("packet", [128, 16])
def test_the_strided_walk_visits_every_packet_below_n_exactly_once(grid, packet):
    capacity = 10 * packet
    for n in range(capacity + 1):
        visits, idle = _walk(n, grid, packet)
        packets = -(-n // packet)
        assert (visits[:packets] == 1).all() and not visits[packets:].any(), (n, grid)
        assert idle == max(grid - packets, 0), (n, grid)          # exactly the workgroups without a packet return at once
    assert _walk(0, grid, packet)[1] == grid                      # n == 0 loads no point: every workgroup returns


# ---- the handler ----------------------------------------------------------------------------------------------------------------

def test_handler_option_and_environment(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    box = {"lo": R.BOX_LO, "hi": R.BOX_HI}
    for name in ("NWE_SPARSE_FINE", "NWE_SPARSE_ASYNC", "NWE_RADIANCE_GRID"):
        monkeypatch.delenv(name, raising=False)
    assert H("office_geneve", "x.ckpt")._sparse_async is False
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={})._sparse_async is False          # nothing changes without it
    h = H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={"dilate": 2}, sparse_async=True)
    assert h._sparse_async is True and h._sparse_fine == {"min_weight": 1e-3, "dilate": 2, "which": "fine"}
    for kw in (dict(), dict(radiance_grid=box)):
        with pytest.raises(ValueError, match="sparse_async is an option of the sparse frame"):
            H("office_geneve", "x.ckpt", sparse_async=True, **kw)
    with pytest.raises(ValueError, match="needs a radiance grid"):          # sparse_fine's own refusal stays in front
        H("office_geneve", "x.ckpt", sparse_fine={}, sparse_async=True)
    monkeypatch.setenv("NWE_SPARSE_ASYNC", "1")
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={})._sparse_async is True
    assert H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={}, sparse_async=False)._sparse_async is False
    with pytest.raises(ValueError, match="sparse_async is an option of the sparse frame"):
        H("office_geneve", "x.ckpt", radiance_grid=box)
    monkeypatch.setenv("NWE_SPARSE_FINE", "0.02")                           # the environment alone switches both on
    h = H("office_geneve", "x.ckpt", radiance_grid=box)
    assert h._sparse_async is True and h._sparse_fine == {"min_weight": 0.02, "dilate": 1, "which": "fine"}
    monkeypatch.setenv("NWE_SPARSE_ASYNC", "0")
    assert H("office_geneve", "x.ckpt", radiance_grid=box)._sparse_async is False
    monkeypatch.setenv("NWE_SPARSE_ASYNC", "yes")
    with pytest.raises(ValueError, match="NWE_SPARSE_ASYNC must be 0 or 1"):
        H("office_geneve", "x.ckpt", radiance_grid=box)
    monkeypatch.delenv("NWE_SPARSE_ASYNC")
    h = H("office_geneve", "x.ckpt", radiance_grid=box, sparse_fine={}, sparse_async=True)
    for call in (lambda: h.render_sparse(np.eye(4), asynchronous=True), lambda: h.render_sparse_batch(np.eye(4)[None], asynchronous=True)):
        with pytest.raises(RuntimeError, match="initialize_models"):
            call()


# ---- the stand-alone program ----------------------------------------------------------------------------------------------------

def test_sparse_async_smoke_builds_and_runs_from_plain_c(tmp_path):
    """tests/c/sparse_async_smoke.c against the product library, without sanitizers (`make asan` runs it with them)."""
    cc = "gcc"                                          # as tests/test_sparse_fine_host.py builds sparse_smoke.c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "sparse_async_smoke")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "sparse_async_smoke.c"), "-o", exe, "-L", lib_dir, "-lnwe_hip", "-lm",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "sparse_async_smoke ok" in res.stdout, res.stderr
