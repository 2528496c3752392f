"""Evaluation rates of the point query (nwe_query_points) beside the renderer's, in one process on one box, three alternating
repetitions each, median and range:

  (a) frame      the C3 bench frame (800x800, 64 + 128, 8x256 coarse + fine, f16x3): 163.84 M evaluations / last_kernel_ms;
  (b) query      query_points of 2^24 points of the fine 8x256 network, f16x3, raw, one direction per 192 points:
                 points / last_query_ms;
  (c) sigma      the same points, sigma only (no directions): the density-only evaluation;
  (d) trick      the ray trick (one ray per point, o = p, near = far = 0, n_samples = 2, raw_coarse) on 2^22 points:
                 points / last_kernel_ms - by construction it evaluates every point twice.

The render kernels' device code is what it was before the query existed, so (a) and (d) stand for the library without it.
Prints one line per measurement and the ratios (b)/(a), (c)/(b), (b)/(d) (DESIGN.md section 5.4 quotes them).
With a third argument `sweep` it then repeats (b) with the steps per workgroup forced to 4 .. 256 (nwe_debug_set_query_steps) and
automatic: a rate that does not move with them rules out the workgroup prologue and the ragged last round of workgroups.
Usage on the GPU box: python tools/query_rate.py [log2 of the query's points, default 24] [sweep]."""
import ctypes as C
import os
import socket
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import _lib, synthetic

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 24
N_QUERY, N_TRICK, PER_DIR = 1 << LOG2, 1 << max(LOG2 - 2, 0), 192
H = W = 800
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)

r = nwe_amd.Renderer(0)
r.set_network(0, synthetic.make_state_dict(1000, 8, 256))
r.set_network(1, synthetic.make_state_dict(1001, 8, 256))
trick = nwe_amd.Renderer(0)                       # the trick's sampling tables (2 + 0) on a context of its own
trick.set_network(0, synthetic.make_state_dict(1001, 8, 256))
trick.set_sampling(2, 0)

gen = torch.Generator(device="cuda").manual_seed(0)
pts = (torch.rand((N_QUERY, 3), generator=gen, device="cuda") * 8.0 - 4.0).contiguous()
dirs = torch.nn.functional.normalize(torch.randn((-(-N_QUERY // PER_DIR), 3), generator=gen, device="cuda"), dim=-1).contiguous()
t_dirs = dirs[torch.arange(N_TRICK, device="cuda") // PER_DIR]
q_raw = torch.empty((N_QUERY, 4), device="cuda")
q_flags = torch.zeros(1, dtype=torch.int32, device="cuda")
q_out = _lib.PointOutputs(raw=q_raw.data_ptr(), flags=q_flags.data_ptr())
rays = torch.cat([pts[:N_TRICK], t_dirs, torch.zeros((N_TRICK, 2), device="cuda"), t_dirs], 1).contiguous()


def frame():
    r.set_sampling(64, 128)
    r.render(pose, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0, outputs=("rgb", "depth", "acc"))
    return H * W * (64 + 64 + 128) / r.last_kernel_ms() * 1e-6          # G evaluations / s


def query():
    # through the ABI itself: 192 does not divide 2^24, so the [N,S,3] / [N,3] layout of Renderer.query_points does not fit
    rc = r._lib.nwe_query_points(r._ctx, 1, pts.data_ptr(), N_QUERY, dirs.data_ptr(), PER_DIR, _lib.PREC_F16X3, C.byref(q_out),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, r._lib.nwe_last_error(r._ctx)
    return N_QUERY / r.last_query_ms() * 1e-6


def sigma():
    r.query_points(pts, None, which=1, precision="f16x3", outputs=("sigma",))
    return N_QUERY / r.last_query_ms() * 1e-6


def ray_trick():
    trick.render_rays(rays, precision="f16x3", outputs=("raw_coarse",))
    return N_TRICK / trick.last_kernel_ms() * 1e-6


runs = (("frame", frame), ("query", query), ("sigma", sigma), ("trick", ray_trick))
print(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}; query 2^{LOG2} = {N_QUERY} points, trick {N_TRICK} points, "
      f"one direction per {PER_DIR} points", flush=True)
for name, fn in runs:       # one launch each to warm up
    fn()
rates = {name: [] for name, _ in runs}
for rep in range(3):
    for name, fn in runs:
        rates[name].append(fn())
        print(f"rep {rep} {name}: {rates[name][-1]:.4f} G evaluations/s" + (" (points/s: each evaluated twice)" if name == "trick" else ""), flush=True)
med = {k: statistics.median(v) for k, v in rates.items()}
for name, _ in runs:
    print(f"== {name}: median {med[name]:.4f} G/s, range {min(rates[name]):.4f} .. {max(rates[name]):.4f}")
print(f"== (b)/(a) query / frame = {med['query'] / med['frame']:.4f}   (c)/(b) sigma / query = {med['sigma'] / med['query']:.4f} "
      f"(MFMA ratio 3120 / 2880 = {3120 / 2880:.4f})   (b)/(d) query / trick = {med['query'] / med['trick']:.4f}")
if sys.argv[2:3] == ["sweep"]:
    sweep = {}
    for rep in range(3):
        for steps in (4, 8, 16, 32, 64, 128, 256, 0):
            r.debug_set_query_steps(steps)
            sweep.setdefault(steps, []).append(query())
    for steps, v in sweep.items():
        print(f"== query, steps {steps if steps else 'automatic'}: median {statistics.median(v):.4f} G/s, range {min(v):.4f} .. {max(v):.4f}")
r.close()
trick.close()
