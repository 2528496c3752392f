"""The multi-level adaptive frame on the bench frame (800x800, 8x256, 64+128, f16x3): arms alternating in one process on one box,
three repetitions of two timed frames each (medians of six), on the room (synthetic.room), on a dense_fog scene and on the
benchmark's random networks (the worst case: little should be flat).  For k = 2, tol_rgb in {1, 2, 4} / 255, tol_depth 0.05, with the
adaptive frame's list switch (nwe_set_adaptive_pixel_lists) off and on:

  plain                  the ordinary frame (nwe_render)
  adaptive t             the one-level adaptive frame (Renderer.render_adaptive, levels=None): the yardstick
  levels=2 t, levels=3 t the multi-level frame (levels=2: lattices of spacing 4 and 2; levels=3: 8, 4 and 2)

Per arm the device time - nwe_last_kernel_ms, or the span of nwe_last_adaptive / nwe_last_adaptive_levels, read-back gaps included -
as median (min - max), the lattice, rendered and interpolated pixels, the render launches, PSNR and the largest |d rgb| against the
plain frame of the same run.  DESIGN.md section 5.12 quotes it.
Usage on the GPU box: python tools/adaptive_levels_ab.py [H W [scene ...]] with scenes of room, fog, bench (default: all three)."""
import os
import statistics
import sys

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
K, TOLS, TOL_DEPTH, LEVELS = 2, (1, 2, 4), 0.05, (2, 3)


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

    def one_level(t, lists):
        r.set_adaptive_pixel_lists(lists)
        out = r.render_adaptive(pose, H, W, k=K, tol_rgb=t / 255, tol_depth=TOL_DEPTH, **CAM)
        c = r.last_adaptive()
        return out, c["ms"], dict(lattice=c["lattice"], rendered=[c["rendered"]], interpolated=[c["interpolated"]],
                                  render_launches=2 if c["rendered"] else 1)

    def levelled(t, lists, levels):
        r.set_adaptive_pixel_lists(lists)
        out = r.render_adaptive(pose, H, W, k=K, levels=levels, tol_rgb=t / 255, tol_depth=TOL_DEPTH, **CAM)
        c = r.last_adaptive_levels()
        return out, c["ms"], c

    def plain():
        out = r.render(pose, H, W, outputs=("rgb",), **CAM)
        torch.cuda.synchronize()
        return out, r.last_kernel_ms(), None

    arms = [("plain", plain)]
    for lists in (False, True):
        for t in TOLS:
            tag = f"tol={t}/255 lists={'on' if lists else 'off'}"
            arms.append((f"adaptive {tag}", lambda t=t, lists=lists: one_level(t, lists)))
            for n in LEVELS:
                arms.append((f"levels={n} {tag}", lambda t=t, lists=lists, n=n: levelled(t, lists, n)))
    dev, rgb, counts = {a[0]: [] for a in arms}, {}, {}
    for rep in range(3):
        for label, render in arms:
            for i in range(3):      # one frame to warm up, two timed
                out, ms, c = render()
                if i > 0:
                    dev[label].append(ms)
            rgb[label], counts[label] = out["rgb"], c
            print(f"{label} rep {rep}: device {dev[label][-2]:.3f} / {dev[label][-1]:.3f} ms", flush=True)
    med = {a: statistics.median(v) for a, v in dev.items()}
    for label in dev:
        line = f"== {label}: device median {med[label]:.3f} ms ({min(dev[label]):.3f} - {max(dev[label]):.3f}); {med['plain'] / med[label]:.2f}x the plain frame"
        c = counts[label]
        if c is not None:
            yardstick = med["adaptive " + label.split(" ", 1)[1]]
            line += (f", {yardstick / med[label]:.2f}x the one-level frame; lattice {c['lattice']}, rendered {c['rendered']}, interpolated "
                     f"{c['interpolated']}, network pixels {(c['lattice'] + sum(c['rendered'])) / (H * W):.3f} of the frame, render launches "
                     f"{c['render_launches']}; against plain: {quality(rgb[label], rgb['plain'])}")
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
