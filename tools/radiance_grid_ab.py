"""The radiance grid on the bench frame (800x800, 8x256, 64+128): arms alternating on one box, three repetitions each, on the
benchmark's networks and on a dense_fog scene:

  plain       the ordinary frame
  baked 128   the baked coarse pass at 128^3
  preview     the coarse-only preview: set_sampling(64, 0), what render_coordinates(preview=True) renders - the cheapest picture
              there was, and the yardstick of the grid frame's time
  grid 128    the radiance grid's frame (Renderer.render_grid) at 128^3: both passes from the grid, no network
  grid 256    ... at 256^3

Per arm the kernel ms (nwe_last_kernel_ms; the grid arms: nwe_last_grid_ms), the bake times apart.  For the grid arms the PSNR
and max |d rgb| against the plain frame, for the grid baked as the handler bakes it by default (the mean of the raw rows over the
six axis directions) and, at 128^3, for one baked with the view direction of the frame's central ray.  Prints one line per (arm,
repetition) and a summary of medians with their spread; last, the grid frame's time on a box tight around the frustum against
the 32-unit box at 128^3, 256^3 and 512^3.  DESIGN.md section 5.8 quotes it.
Usage on the GPU box: python tools/radiance_grid_ab.py [H W]."""
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
AXES = Handler._AXIS_DIRECTIONS


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
        for d in AXES:
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


def quality(label, rgb, ref):
    d = (rgb - ref).abs()
    mse = float((d.double() ** 2).mean())
    psnr = "inf" if mse == 0 else f"{-10.0 * np.log10(mse):.1f}"
    return f"{label}: PSNR {psnr} dB, max |d rgb| {float(d.max()):.3f}, mean |d rgb| {float(d.mean()):.4f}"


def run(scene, sds):
    print(f"==== scene: {scene}", flush=True)
    plain, baked, g128, g256 = (renderer(sds) for _ in range(4))
    timed("bake coarse 128^3", lambda: baked.bake_coarse_grid(LO, HI, 128))
    timed("bake radiance 128^3, six directions", lambda: bake_mean(g128, 128))
    timed("bake radiance 256^3, six directions", lambda: bake_mean(g256, 256))
    frame = lambda r: r.render(pose, H, W, outputs=("rgb", "depth", "acc"), **CAM)
    grid = lambda r: r.render_grid(pose, H, W, **CAM)

    def preview(r):
        r.set_sampling(64, 0)
        try:
            return frame(r)
        finally:
            r.set_sampling(64, 128)

    arms = (("plain", plain, frame, plain.last_kernel_ms), ("baked 128", baked, frame, baked.last_kernel_ms),
            ("preview", plain, preview, plain.last_kernel_ms), ("grid 128", g128, grid, g128.last_grid_ms),
            ("grid 256", g256, grid, g256.last_grid_ms))
    ms, rgb = {a[0]: [] for a in arms}, {}
    for rep in range(3):
        for label, r, render, last_ms in arms:
            for i in range(3):      # one launch to warm up, two timed
                out = render(r)
                if i > 0:
                    ms[label].append(last_ms())
            rgb[label] = out["rgb"]
            print(f"{label} rep {rep}: kernel {ms[label][-2]:.3f} / {ms[label][-1]:.3f} ms", flush=True)
    med = {a: statistics.median(v) for a, v in ms.items()}
    for label in ms:
        print(f"== {label}: median {med[label]:.3f} ms ({min(ms[label]):.3f} - {max(ms[label]):.3f}); "
              f"{med['plain'] / med[label]:.1f}x the plain frame, {med['preview'] / med[label]:.1f}x the preview", flush=True)
    print("== " + quality("preview against plain", rgb["preview"], rgb["plain"]))
    print("== " + quality("baked 128 against plain", rgb["baked 128"], rgb["plain"]))
    for label in ("grid 128", "grid 256"):
        print("== " + quality(f"{label} (six-direction mean) against plain", rgb[label], rgb["plain"]), flush=True)
    forward = tuple(float(v) for v in pose[:3, 2] / np.linalg.norm(pose[:3, 2]))     # the central ray's direction
    timed("bake radiance 128^3, one direction", lambda: g128.bake_radiance_grid(LO, HI, 128, view_dir=forward))
    print("== " + quality("grid 128 (central ray's direction) against plain", grid(g128)["rgb"], rgb["plain"]), flush=True)
    for r in (plain, baked, g128, g256):
        r.close()


def tight_box(sds):
    """The grid frame's time against the share of the grid its rays read: a box tight around the frame's frustum, which the rays
    cross about a third of, against the 32-unit box, at 128^3, 256^3 and 512^3 (2 GiB); one direction baked in place."""
    print("==== grid frame time by box and resolution (bench networks, one direction baked)", flush=True)
    r = renderer(sds)
    rays = r.create_rays(pose, H, W, **CAM)
    ends = torch.cat([rays[:, 0:3] + rays[:, 3:6] * CAM["near"], rays[:, 0:3] + rays[:, 3:6] * CAM["far"]])
    lo, hi = (ends.min(0).values - 0.05).cpu().tolist(), (ends.max(0).values + 0.05).cpu().tolist()
    print("tight box", [round(v, 2) for v in lo], [round(v, 2) for v in hi], flush=True)
    forward = tuple(float(v) for v in pose[:3, 2])
    for name, box in (("tight", (lo, hi)), ("32-unit", (LO, HI))):
        for res in (128, 256, 512):
            r.bake_radiance_grid(box[0], box[1], res, view_dir=forward)
            ms = []
            for i in range(7):      # two launches to warm up, five timed
                out = r.render_grid(pose, H, W, **CAM)
                if i > 1:
                    ms.append(r.last_grid_ms())
            print(f"{name} box {res}^3 ({res ** 3 * 16 / 2 ** 20:.0f} MiB): grid frame median {statistics.median(ms):.3f} ms "
                  f"({min(ms):.3f} - {max(ms):.3f}), rays with opacity {100 * float((out['acc'] > 0).float().mean()):.1f} %", flush=True)
    r.close()


def main():
    S = synthetic
    run("bench (random networks)", (S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256)))
    run("dense_fog(0.5, 3.0) fine under a thin_fog coarse network",
        (S.thin_fog(S.make_state_dict(1000, 8, 256)), S.dense_fog(S.make_state_dict(1001, 8, 256), 0.5, 3.0)))
    tight_box((S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256)))


if __name__ == "__main__":
    main()
