"""The adaptive frame on the bench frame (800x800, 8x256, 64+128, f16x3): arms alternating in one process on one box, three
repetitions of two timed frames each, on the room (synthetic.room), on a dense_fog scene and on the benchmark's random networks
(the worst case: little should be flat):

  plain            the ordinary frame (nwe_render)
  rays             nwe_render_rays on the whole frame's rays, lean outputs: the per-ray price of not being lean
  adaptive k t     the adaptive frame (Renderer.render_adaptive) for k in {2, 4} x tol_rgb in {1, 2, 4} / 255, tol_depth 0.05

Per arm the host wall time of the call (synchronised) and the device time - nwe_last_kernel_ms, or the span of nwe_last_adaptive -
as median (min - max); for the adaptive arms the four counts, PSNR and the largest |d rgb| against the plain frame of the same
run, and the expectation (lattice + rendered) / pixels x the rays arm, next to which the measured span shows the classify /
compose / read-back constant.  DESIGN.md section 5.10 quotes it.
Usage on the GPU box: python tools/adaptive_ab.py [H W [scene ...]] with scenes of room, fog, bench (default: all three)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nwe_amd
from nwe_amd import synthetic

H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (800, 800)
SCENES = sys.argv[3:] or ["room", "fog", "bench"]
pose = np.array([[0.8660254, 0, 0.5, 0], [-0.5, 0, 0.8660254, -0.76157], [0, -1, 0, 0.5], [0, 0, 0, 1]], np.float32)
fx, fy, cx, cy = nwe_amd.pinhole_intrinsics(H, W)
CAM = dict(fx=fx, fy=fy, cx=cx, cy=cy, near=0.1, far=10.0)
KS, TOLS, TOL_DEPTH = (2, 4), (1, 2, 4), 0.05


def quality(rgb, ref):
    d = (rgb - ref).abs()
    mse = float((d.double() ** 2).mean())
    psnr = "inf" if mse == 0 else f"{-10.0 * np.log10(mse):.1f}"
    return f"PSNR {psnr} dB, max |d rgb| {float(d.max()):.4f}"


def run(scene, sds):
    print(f"==== scene: {scene}", flush=True)
    r = nwe_amd.Renderer(0)
    r.set_network(0, sds[0]); r.set_network(1, sds[1])
    r.set_sampling(64, 128)
    rays = r.create_rays(pose, H, W, **CAM)
    arms = [("plain", lambda: r.render(pose, H, W, outputs=("rgb",), **CAM), r.last_kernel_ms),
            ("rays", lambda: r.render_rays(rays, outputs=("rgb",)), r.last_kernel_ms)]
    for k in KS:
        for t in TOLS:
            arms.append((f"adaptive k={k} tol={t}/255", lambda k=k, t=t: r.render_adaptive(pose, H, W, k=k, tol_rgb=t / 255, tol_depth=TOL_DEPTH, **CAM),
                         lambda: r.last_adaptive()["ms"]))
    wall, dev, rgb, counts = {a[0]: [] for a in arms}, {a[0]: [] for a in arms}, {}, {}
    for rep in range(3):
        for label, render, last_ms in arms:
            for i in range(3):      # one frame to warm up, two timed
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = render()
                torch.cuda.synchronize()
                if i > 0:
                    wall[label].append(1e3 * (time.perf_counter() - t0))
                    dev[label].append(last_ms())
            rgb[label] = out["rgb"]
            if label.startswith("adaptive"):
                counts[label] = r.last_adaptive()
            print(f"{label} rep {rep}: device {dev[label][-2]:.3f} / {dev[label][-1]:.3f} ms, wall {wall[label][-2]:.3f} / {wall[label][-1]:.3f} ms", flush=True)
    med = {a: statistics.median(v) for a, v in dev.items()}
    print(f"the rays arm's rgb equals the plain frame's bit for bit: {torch.equal(torch.nan_to_num(rgb['rays']), torch.nan_to_num(rgb['plain']))}")
    for label in dev:
        line = (f"== {label}: device median {med[label]:.3f} ms ({min(dev[label]):.3f} - {max(dev[label]):.3f}), wall median "
                f"{statistics.median(wall[label]):.3f} ms; {med['plain'] / med[label]:.2f}x the plain frame")
        if label in counts:
            c = counts[label]
            model = (c["lattice"] + c["rendered"]) / c["pixels"] * med["rays"]
            line += (f"; pixels {c['pixels']}, lattice {c['lattice']}, rendered {c['rendered']}, interpolated {c['interpolated']} "
                     f"({c['interpolated'] / c['pixels']:.3f}); against plain: {quality(rgb[label], rgb['plain'])}; model (lattice + rendered) / "
                     f"pixels x rays = {model:.3f} ms, measured - model = {med[label] - model:.3f} ms")
        print(line, flush=True)
    r.close()


def main():
    S = synthetic
    scenes = {"room": ("room (walls at +-3, both networks)", lambda: (S.room(S.make_state_dict(1000, 8, 256)), S.room(S.make_state_dict(1001, 8, 256)))),
              "fog": ("dense_fog(0.5, 3.0) fine under a thin_fog coarse network",
                      lambda: (S.thin_fog(S.make_state_dict(1000, 8, 256)), S.dense_fog(S.make_state_dict(1001, 8, 256), 0.5, 3.0))),
              "bench": ("bench (random networks)", lambda: (S.make_state_dict(1000, 8, 256), S.make_state_dict(1001, 8, 256)))}
    for name in SCENES:
        title, make = scenes[name]
        run(title, make())


if __name__ == "__main__":
    main()
