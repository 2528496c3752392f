"""Accuracy against an fp64 ground truth: the one criterion every precision test of tests/test_gpu_accuracy.py applies.

For an output y (per-sample raw, or per-ray rgb / depth / acc / z_fine / z_std):
    e_k = |y_kernel - y_64|      the kernel's error
    e_r = |y_ref32 - y_64|       the error of the fp32 oracle (bit-equal to the reference) on the same inputs
and each of max, p99 and median of e_k must be <= FACTOR * (the same statistic of e_r) + FLOOR.  Depths are divided by `far`
first.  y_64 is oracle/nerf_oracle.py in its fp64 mode, pinned to the reference's own blocks by tests/golden/f64.npz.
The same comparison calibrates the single-product mode against tests/mfma_emulator.py (y_ref32 := the emulator).

The kernels' own fp32 arithmetic (the f32 kernel's FMA chains, the compositing's sequential sums that every mode shares) rounds
in another order than torch's blocked sums.  On outputs whose error is a few ulps it is up to 5.4x the reference's error
(DESIGN.md section 6.1).  So each test has a bound K32 of its own, its measured maximum rounded up:
  * the f32 kernel:  each statistic <= K32 x that of the fp32 reference + FLOOR  (pins the shared fp32 path to fp64);
  * the f16x3 modes: each statistic <= FACTOR x min(max(reference's, f32 kernel's), K32 x reference's) + FLOOR, i.e. against
    the larger of the two fp32 paths' errors (`y_alt`), a yardstick that can never exceed K32 x the reference's.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import nerf_oracle as O

FACTOR = 1.5       # DESIGN.md section 6 records the ratios measured on an MI355X
FLOOR = 1e-7       # absolute


def _np(y) -> np.ndarray:
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    return np.asarray(y, np.float64)


def stats(e: np.ndarray) -> Tuple[float, float, float]:
    """(max, p99, median) of an error array; NaN if any element is not finite."""
    e = np.asarray(e, np.float64).ravel()
    if e.size == 0:
        return 0.0, 0.0, 0.0
    if not np.all(np.isfinite(e)):
        return float("nan"), float("nan"), float("nan")
    return float(e.max()), float(np.percentile(e, 99)), float(np.median(e))


def compare(tag: str, y_k, y_r, y_64, scale: float = 1.0, keep: Optional[np.ndarray] = None,
            factor: float = FACTOR, floor: float = FLOOR, y_alt=None, alt_cap: Optional[float] = None) -> Tuple[bool, str]:
    """The criterion on one output.  `keep` [R] selects rays (the leading axis); `scale` divides every error (far for depths).
    `y_alt`: a second fp32 yardstick (the on-device fp32 kernel); each statistic of the yardstick is then the larger of the
    two, but at most `alt_cap` x the reference's.  Returns (passed, one report line with all three statistics of both sides and
    their ratios)."""
    y_k, y_r, y_64 = _np(y_k), _np(y_r), _np(y_64)
    assert y_k.shape == y_r.shape == y_64.shape, (tag, y_k.shape, y_r.shape, y_64.shape)
    y_a = None if y_alt is None else _np(y_alt)
    if keep is not None:
        y_k, y_r, y_64 = y_k[keep], y_r[keep], y_64[keep]
        y_a = None if y_a is None else y_a[keep]
    sk = stats(np.abs(y_k - y_64) / scale)
    sr = stats(np.abs(y_r - y_64) / scale)
    if y_a is not None:
        assert alt_cap is not None, "a second yardstick needs its cap"
        sr = tuple(min(max(r, a), alt_cap * r) for r, a in zip(sr, stats(np.abs(y_a - y_64) / scale)))
    ok = all(k <= factor * r + floor for k, r in zip(sk, sr))          # NaN compares False
    ratio = lambda k, r: k / r if r > 0 else (0.0 if k == 0 else float("inf"))
    line = (f"{tag:<58s} kernel max {sk[0]:.2e} p99 {sk[1]:.2e} med {sk[2]:.2e} | ref32 max {sr[0]:.2e} p99 {sr[1]:.2e} "
            f"med {sr[2]:.2e}{' (ref32|f32 kernel)' if y_a is not None else ''} | ratio {ratio(sk[0], sr[0]):.2f} {ratio(sk[1], sr[1]):.2f} {ratio(sk[2], sr[2]):.2f}"
            f" (bound {factor:g}x){'' if ok else '  FAIL'}")
    return ok, line


class Report:
    """Collects comparisons, prints every line, and fails once at the end with all failing lines."""

    def __init__(self):
        self.lines: List[str] = []
        self.failed: List[str] = []

    def add(self, tag: str, y_k, y_r, y_64, **kw) -> None:
        ok, line = compare(tag, y_k, y_r, y_64, **kw)
        print(line)
        self.lines.append(line)
        if not ok:
            self.failed.append(line)

    def check(self) -> None:
        assert not self.failed, "kernel error above its bound against fp64:\n" + "\n".join(self.failed)


def raw_at_depths(rays: torch.Tensor, z: torch.Tensor, state: Dict[str, torch.Tensor], dtype: torch.dtype,
                  cfg: Optional[O.RenderConfig] = None, fp32_points: bool = False) -> torch.Tensor:
    """The network of the reference at the points o + d * z of the given fp32 rays [R, 8|11] and depths [R, S] (the points
    are formed in `dtype`, as the oracle's render loop forms them, handler.py:223,246) -> raw [R, S, 4].
    `fp32_points`: the points o + d * z and their division by 10 (embedding.py:48) are formed in fp32 exactly as the reference
    forms them, and encoding and MLP run in `dtype` on those fp32 values (the view directions are fp32 values already).  With
    dtype = float64 this is the ground truth for coordinates so large that the rounding of the point dominates everything else:
    there |fp32 - fp64| of the plain fp64 path measures the point rounding and nothing of the arithmetic under test."""
    cfg = cfg or O.RenderConfig()
    viewdirs = rays[:, -3:] if rays.shape[1] > 8 else None
    if fp32_points:
        rays32, z32 = rays.to(torch.float32), z.to(torch.float32)
        pts = rays32[:, None, 0:3] + rays32[:, None, 3:6] * z32[..., None]            # handler.py:223, fp32
        # run_network divides by 10 in `dtype`: hand it 10 x (the fp32 quotient), which that division undoes exactly in fp64
        # (v * 10 is exact in fp64 for an fp32 v, and (v * 10) / 10 rounds back to v: |v * 10 / 10 - v| < ulp64(v) / 2)
        v = (pts / 10.0).to(dtype)
        pts = v * 10.0 if dtype == torch.float64 else pts
    else:
        rays, z = rays.to(dtype), z.to(dtype)
        pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    with torch.no_grad():
        raw = O.run_network(pts, viewdirs, state, cfg.freqs_xyz, cfg.freqs_dir, cfg.net_chunk, dtype=dtype)
    return raw[..., :4]


def per_ray_outputs(res: Dict[str, torch.Tensor], fine: bool) -> Dict[str, torch.Tensor]:
    """The oracle's per-ray outputs under the kernel's output names."""
    p = "fine" if fine else "coarse"
    out = {"rgb": res["rgb_" + p], "depth": res["depth_" + p], "acc": res["acc_" + p]}
    if fine:
        out.update(z_fine=res["z_fine"], z_std=res["z_std"])
    return out


def e2e_report(rep: Report, tag: str, got: Dict[str, torch.Tensor], ref32: Dict[str, torch.Tensor], ref64: Dict[str, torch.Tensor],
               far: float, keep: Optional[np.ndarray] = None, keys: Sequence[str] = ("rgb", "depth", "acc", "z_fine", "z_std"),
               alt: Optional[Dict[str, torch.Tensor]] = None, **kw) -> None:
    """`alt`: the f32 kernel's outputs as the second yardstick (pass `alt_cap`); other keywords go to compare()."""
    for k in keys:
        if k in got and k in ref32:
            rep.add(f"{tag} {k}", got[k], ref32[k], ref64[k], scale=far if k in ("depth", "z_fine", "z_std") else 1.0, keep=keep,
                    y_alt=None if alt is None or k not in alt else alt[k], **kw)


def weight_set(sd: Dict[str, np.ndarray], kind: str) -> Dict[str, np.ndarray]:
    """Weight statistics other than make_state_dict's uniform gain-2 layers (deterministic)."""
    out = {k: v.copy() for k, v in sd.items()}
    W = sd["_pts_linears.0.weight"].shape[0]
    names = sorted(k[:-len(".weight")] for k in sd if k.endswith(".weight"))
    if kind == "layer_scales":             # per-layer magnitudes 2^-4 .. 2^3 under the one stream-wide scale
        for i, n in enumerate(names):
            out[n + ".weight"] = (out[n + ".weight"] * np.float32(2.0 ** ((3 * i) % 8 - 4))).astype(np.float32)
    elif kind in ("bias300", "bias3000"):  # large first-layer activations
        out["_pts_linears.0.bias"] = (out["_pts_linears.0.bias"] + np.float32(300 if kind == "bias300" else 3000)).astype(np.float32)
    elif kind == "outlier":                # one weight of 60 sets the stream-wide scale for all others
        out["_pts_linears.2.weight"][W // 3, 7] = np.float32(60.0)
    elif kind == "student_t":              # heavy tails (t, 3 degrees of freedom), the uniform init's standard deviation
        rng = np.random.Generator(np.random.Philox(key=[77, W]))
        for n in names:
            w = out[n + ".weight"]
            std = 2.0 / np.sqrt(w.shape[1]) / np.sqrt(3.0)
            out[n + ".weight"] = (rng.standard_t(3, size=w.shape) * std / np.sqrt(3.0)).astype(np.float32)
    else:
        raise ValueError(kind)
    return out


WEIGHT_SETS = ["layer_scales", "bias300", "bias3000", "outlier", "student_t"]
