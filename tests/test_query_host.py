"""The point query (include/nwe.h: nwe_query_points; run_network of nerf/models/model_utils.py:13-30) as far as it is reachable
without a device: what a host-only context answers, the nwe_point_outputs layout and its size guard's premise, the shape
rules of Renderer.query_points, and the cell centres of the handler's density_grid against a numpy restatement.  The
refusals behind the context check - the C order puts it first - are in tests/test_gpu_query.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from nwe_amd.handler import NeRFReplicaInferenceHandler
from nwe_amd.renderer import Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def host():
    r = Renderer(host_only=True)
    r.set_network(1, nwe_amd.synthetic.make_state_dict(7, 4, 128))
    yield r
    r.close()


def test_host_only_and_null_contexts_are_refused_first(host):
    """Refusal 1 comes before every argument check: a host-only or a null context is NWE_ERR_STATE whatever else is wrong, and
    the timing call and the steps hook behave on it."""
    lib = _lib.load()
    good, short = _lib.PointOutputs(), _lib.PointOutputs()
    short.struct_bytes -= 8
    for ctx in (host._ctx, None):
        for out in (good, short, None):
            for which, n, ppd, prec in ((1, 0, 1, 0), (7, -1, 0, 9), (0, 1 << 31, 1, 2)):
                rc = lib.nwe_query_points(ctx, which, None, n, None, ppd, prec, C.byref(out) if out is not None else None, None)
                assert rc == _lib.NWE_ERR_STATE
    assert b"needs a device context" in lib.nwe_last_error(host._ctx)
    assert lib.nwe_last_query_ms(host._ctx) == -1.0 and lib.nwe_last_query_ms(None) == -1.0
    # the steps hook is host-side state: 0 (automatic) .. 256
    for steps, rc in ((0, 0), (1, 0), (3, 0), (256, 0), (257, _lib.NWE_ERR_INVALID), (-1, _lib.NWE_ERR_INVALID)):
        assert lib.nwe_debug_set_query_steps(host._ctx, steps) == rc, steps
    assert lib.nwe_debug_set_query_steps(None, 1) == _lib.NWE_ERR_INVALID
    host.debug_set_query_steps(2)
    with pytest.raises(ValueError):
        host.debug_set_query_steps(1000)
    assert host.last_query_ms() == -1.0


def test_point_outputs_struct_matches_the_header():
    """nwe_point_outputs carries its own size like nwe_outputs: the ctypes struct has exactly the header's fields, in order, and
    fills struct_bytes with its size (the refusal of another size needs a device context: tests/test_gpu_query.py)."""
    header = open(os.path.join(ROOT, "include", "nwe.h")).read()
    body = header[header.index("typedef struct nwe_point_outputs {"):header.index("} nwe_point_outputs;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:float|uint32_t|uint64_t)\s*\*?\s*(\w+)\s*;", body)
    assert fields == ["struct_bytes"] + list(_lib.POINT_OUTPUT_FIELDS) == ["struct_bytes", "raw", "sigma", "flags"]
    o = _lib.PointOutputs()
    assert o.struct_bytes == C.sizeof(_lib.PointOutputs) == 8 * len(fields)
    assert o.raw is None and o.sigma is None and o.flags is None
    assert [f[0] for f in _lib.PointOutputs._fields_] == fields
    assert {"nwe_query_points", "nwe_last_query_ms", "nwe_debug_set_query_steps"} <= set(_lib.SYMBOLS)


@pytest.mark.parametrize("points,dirs,expect", [
    ((5, 3), None, (5, 1)),
    ((5, 3), (5, 3), (5, 1)),
    ((4, 6, 3), (4, 6, 3), (24, 1)),
    ((4, 6, 3), (4, 3), (24, 6)),             # run_network's layout: viewdirs[:, None].expand(inputs.shape)
    ((3, 3, 3), (3, 3), (9, 3)),
    ((2, 3, 4, 3), (2, 3, 4, 3), (24, 1)),
    ((3,), None, (1, 1)),
    ((3,), (3,), (1, 1)),
    ((0, 3), None, (0, 1)),
    ((4, 0, 3), (4, 3), (0, 1)),
])
def test_query_layout_accepts(points, dirs, expect):
    assert Renderer.query_layout(points, dirs) == expect


@pytest.mark.parametrize("points,dirs", [
    ((5, 4), None),                 # not [..., 3]
    ((), None),
    ((5, 3), (4, 3)),               # neither one row per point ...
    ((4, 6, 3), (6, 3)),            # ... nor one per leading row
    ((4, 6, 3), (24, 3)),
    ((4, 6, 3), (4, 1, 3)),         # no broadcasting
    ((2, 3, 4, 3), (2, 3)),         # [N,3] only against [N,S,3]
    ((5, 3), (5, 4)),
    ((5, 3), (3,)),
])
def test_query_layout_refuses(points, dirs):
    with pytest.raises(ValueError):
        Renderer.query_layout(points, dirs)


def test_query_points_checks_its_arguments_before_the_context(host):
    """Every Python-side check raises ValueError on a host-only renderer, whose ABI would answer NWE_ERR_STATE (RuntimeError):
    the checks come first and touch no device."""
    p, d = torch.zeros(4, 6, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="dirs must be"):
        host.query_points(p, torch.zeros(6, 3))
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        host.query_points(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="float32"):
        host.query_points(p.double(), d)
    with pytest.raises(ValueError, match="float32"):
        host.query_points(p, d.half())
    for outputs in ((), ("rgb",), ("raw", "raw"), ("raw", "depth")):
        with pytest.raises(ValueError, match="outputs"):
            host.query_points(p, d, outputs=outputs)
    with pytest.raises(ValueError, match="precision"):
        host.query_points(p, d, precision="f64")
    with pytest.raises(ValueError, match="which"):
        host.query_points(p, d, which=2)
    with pytest.raises(RuntimeError, match="needs a device context"):
        host.query_points(p, d)
    with pytest.raises(RuntimeError, match="needs a device context"):
        host.query_points(p, None, outputs=("sigma",), precision="f32", which=0)


def _centres_numpy(lo, hi, res):
    """The restatement: per axis (i + 0.5) * step + lo in float32, step = (hi - lo) / r rounded to float32 once; [rx, ry, rz, 3]."""
    axes = []
    for l, h, r in zip(lo, hi, res):
        step = np.float32((float(h) - float(l)) / r)
        axes.append((np.arange(r).astype(np.float32) + np.float32(0.5)) * step + np.float32(l))
    gx, gy, gz = np.meshgrid(*axes, indexing="ij")
    return np.stack([gx, gy, gz], -1).astype(np.float32)


@pytest.mark.parametrize("lo,hi,res", [
    ((-1.0, -2.0, 0.5), (1.0, 2.5, 0.75), (3, 5, 7)),
    ((-3.3, -1.1, -2.7), (4.1, 0.3, 2.9), (4, 1, 6)),
    ((0.1, 0.2, 0.3), (0.7, 0.5, 0.4), (1, 1, 1)),
    ((-5.0, -5.0, -5.0), (5.0, 5.0, 5.0), (10, 11, 13)),
])
def test_grid_centres_match_the_numpy_restatement(lo, hi, res):
    want = _centres_numpy(lo, hi, res)
    total = res[0] * res[1] * res[2]
    whole = NeRFReplicaInferenceHandler.grid_centres(lo, hi, res)
    assert whole.dtype == torch.float32 and tuple(whole.shape) == (total, 3)
    assert np.array_equal(whole.numpy().reshape(res + (3,)), want)
    # every centre lies inside its cell, and so inside the box
    assert (want >= np.float32(lo)).all() and (want <= np.float32(hi)).all()
    # in chunks, as density_grid walks them: sizes that divide the grid and sizes that do not, one cell, more than the grid
    for chunk in (1, 4, 7, total - 1 if total > 1 else 1, total, total + 5):
        parts = [NeRFReplicaInferenceHandler.grid_centres(lo, hi, res, start, min(chunk, total - start))
                 for start in range(0, total, chunk)]
        assert all(0 < p.shape[0] <= chunk for p in parts)
        assert torch.equal(torch.cat(parts, 0), whole), chunk
