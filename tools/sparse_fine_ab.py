"""The sparse frame on the bench frame (800x800, 8x256, 64+128): arms alternating on one box, three repetitions of two timed frames
each, on the benchmark's random networks, on a dense_fog scene and on the room (synthetic.room):

  plain          the ordinary frame
  baked 128      the baked coarse pass at 128^3: the yardstick of the sparse frame's time
  grid 128       the radiance grid's frame at 128^3: the proposal alone
  sparse 1e-2    the sparse frame (Renderer.render_sparse) on that grid, min_weight 1e-2, dilate 1
  sparse 1e-3    ... min_weight 1e-3
  sparse 1e-4    ... min_weight 1e-4

Per arm the kernel ms as median (min - max) - nwe_last_kernel_ms, nwe_last_grid_ms, nwe_last_sparse_ms - the selected share, PSNR,
max and mean |d rgb| against the plain frame of the same run, and for the sparse arms the model
t = t(grid frame) + selected * 37 ms / 2^24 (the point query's rate) next to the measured time.  The grid is baked
as the handler bakes it by default: the mean of the raw rows over the six axis directions.  DESIGN.md section 5.9 quotes it.
Usage on the GPU box: python tools/sparse_fine_ab.py [H W]."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic
from nwe_amd.handler import NeRFReplicaInferenceHandler as Handler

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
CAM = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
LO, HI = (-16.0, -16.0, -16.0), (16.0, 16.0, 16.0)      # every sample of the frame (depth 0.1 .. 10 from (0, -0.76, 0.5))
RES = 128
QUERY_MS_PER_POINT = 37.0 / 2 ** 24                     # 2^24 points in 37 ms
MIN_WEIGHTS = (1e-2, 1e-3, 1e-4)


def renderer(sds):
    r = nwe_amd.Renderer(0)
    r.set_network(0, sds[0]); r.set_network(1, sds[1])
    r.set_sampling(64, 128)
    return r


def bake_mean(r, res, chunk=1 << 20):
    """The handler's default bake on a bare Renderer: the mean of the fine network's raw rows over the six axis directions."""
    total = res ** 3
    raw = torch.empty((total, 4), dtype=torch.float32, device=r.device)
    for start in range(0, total, chunk):
        count = min(chunk, total - start)
        pts = Handler.grid_centres(LO, HI, (res,) * 3, start, count, device=r.device)[None]
        acc = None
        for d in Handler._AXIS_DIRECTIONS:
            row = r.query_points(pts, torch.tensor([d], dtype=torch.float32, device=r.device), outputs=("raw",))["raw"][0]
            acc = row if acc is None else acc + row
        raw[start:start + count] = acc / 6.0
    r.set_radiance_grid(raw.reshape(res, res, res, 4), LO, HI)


def timed(what, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    print(f"{what}: {1e3 * (time.perf_counter() - t0):.1f} ms", flush=True)


def quality(rgb, ref):
    d = (rgb - ref).abs()
    mse = float((d.double() ** 2).mean())
    psnr = "inf" if mse == 0 else f"{-10.0 * np.log10(mse):.1f}"
    return f"PSNR {psnr} dB, max |d rgb| {float(d.max()):.3f}, mean |d rgb| {float(d.mean()):.4f}"


def run(scene, sds):
    print(f"==== scene: {scene}", flush=True)
    plain, baked, grid = (renderer(sds) for _ in range(3))
    timed(f"bake coarse {RES}^3", lambda: baked.bake_coarse_grid(LO, HI, RES))
    timed(f"bake radiance {RES}^3, six directions", lambda: bake_mean(grid, RES))
    frame = lambda r: r.render(pose, H, W, outputs=("rgb", "depth", "acc"), **CAM)
    arms = [("plain", plain, frame, plain.last_kernel_ms), ("baked 128", baked, frame, baked.last_kernel_ms),
            ("grid 128", grid, lambda r: r.render_grid(pose, H, W, **CAM), grid.last_grid_ms)]
    for mw in MIN_WEIGHTS:
        arms.append((f"sparse {mw:.0e}", grid, lambda r, mw=mw: r.render_sparse(pose, H, W, min_weight=mw, dilate=1, **CAM), grid.last_sparse_ms))
    ms, rgb, share = {a[0]: [] for a in arms}, {}, {}
    for rep in range(3):
        for label, r, render, last_ms in arms:
            for i in range(3):      # one frame to warm up, two timed
                out = render(r)
                if i > 0:
                    ms[label].append(last_ms())
            rgb[label] = out["rgb"]
            if label.startswith("sparse"):
                share[label] = grid.last_sparse_samples()
            print(f"{label} rep {rep}: kernel {ms[label][-2]:.3f} / {ms[label][-1]:.3f} ms", flush=True)
    med = {a: statistics.median(v) for a, v in ms.items()}
    for label in ms:
        line = f"== {label}: median {med[label]:.3f} ms ({min(ms[label]):.3f} - {max(ms[label]):.3f}); {med['plain'] / med[label]:.2f}x the plain frame"
        if label != "plain":
            line += f", {med['baked 128'] / med[label]:.2f}x the baked-coarse frame; against plain: {quality(rgb[label], rgb['plain'])}"
        if label in share:
            selected, total = share[label]
            model = med["grid 128"] + selected * QUERY_MS_PER_POINT
            line += (f"; selected {selected} of {total} samples = {selected / total:.4f}; model t(grid) + selected * 37 ms / 2^24 = {model:.3f} ms, "
                     f"measured / model = {med[label] / model:.2f}")
        print(line, flush=True)
    for r in (plain, baked, grid):
        r.close()


def main():
    S = synthetic
    coarse = S.thin_fog(S.make_state_dict(1000, 8, 256))
    run("bench (random networks)", (S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256)))
    run("dense_fog(0.5, 3.0) fine under a thin_fog coarse network", (coarse, S.dense_fog(S.make_state_dict(1001, 8, 256), 0.5, 3.0)))
    run("room (walls at +-3, both networks)", (S.room(S.make_state_dict(1000, 8, 256)), S.room(S.make_state_dict(1001, 8, 256))))


if __name__ == "__main__":
    main()
