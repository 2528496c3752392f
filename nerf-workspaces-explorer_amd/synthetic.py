"""Deterministic synthetic NeRF weights in the reference's ``NeRFModel`` state-dict layout.

The trained checkpoints of the reference are not in its tree (.MISSING_LARGE_BLOBS:1-4), so the
benchmark and the parity tests use weights from a counter-based numpy generator: the same seed
gives the same tensors on every machine, so nothing large has to be committed.

Layout follows nerf/models/nerf_model.py:32-43 (``nn.Linear`` weights are ``[out, in]``, fp32):
``_pts_linears.{i}``, ``_views_linears.0``, ``_feature_linear``, ``_alpha_linear``, ``_rgb_linear``.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np


def layer_shapes(D: int, W: int, in_xyz: int = 63, in_dir: int = 27,
                 skips: Tuple[int, ...] = (4,), use_view_dirs: bool = True, output_ch: int = 5) -> Dict[str, Tuple[int, int]]:
    """name -> (out, in) for every Linear of NeRFModel(D, W, use_view_dirs=...).  use_view_dirs=False (nerf_model.py:41-43; the
    handler then passes input_ch_views = 0 and output_ch = 5, handler.py:97-110): the heads are ONE `_output_linear`; the
    module still owns a `_views_linears.0` (:37) that forward() never calls - it is part of the state dict."""
    shapes = {"_pts_linears.0": (W, in_xyz)}
    for i in range(D - 1):
        # nerf_model.py:33-35: layer i+1 takes the skip input when i is in `skips`
        shapes[f"_pts_linears.{i + 1}"] = (W, W + in_xyz if i in skips else W)
    if not use_view_dirs:
        shapes["_views_linears.0"] = (W // 2, W)
        shapes["_output_linear"] = (output_ch, W)
        return shapes
    shapes["_views_linears.0"] = (W // 2, in_dir + W)
    shapes["_feature_linear"] = (W, W)
    shapes["_alpha_linear"] = (1, W)
    shapes["_rgb_linear"] = (3, W // 2)
    return shapes


def make_state_dict(seed: int, D: int = 8, W: int = 256, in_xyz: int = 63, in_dir: int = 27,
                    skips: Tuple[int, ...] = (4,), w_gain: float = 2.0, b_gain: float = 1.0,
                    use_view_dirs: bool = True, output_ch: int = 5) -> Dict[str, np.ndarray]:
    """U(-w_gain/sqrt(fan_in), +w_gain/sqrt(fan_in)) weights, U(+-b_gain/sqrt(fan_in)) biases.

    The gain is about twice PyTorch's default init so that per-sample opacity spans 0..1 and the
    rendered image is not flat; one Philox stream per tensor keyed by (seed, index).
    """
    out: Dict[str, np.ndarray] = {}
    for idx, (name, (n_out, n_in)) in enumerate(layer_shapes(D, W, in_xyz, in_dir, skips, use_view_dirs, output_ch).items()):
        rng = np.random.Generator(np.random.Philox(key=[seed, idx]))
        kw, kb = w_gain / np.sqrt(n_in), b_gain / np.sqrt(n_in)
        out[f"{name}.weight"] = rng.uniform(-kw, kw, size=(n_out, n_in)).astype(np.float32)
        out[f"{name}.bias"] = rng.uniform(-kb, kb, size=(n_out,)).astype(np.float32)
    return out


def thin_fog(state: Dict[str, np.ndarray], sigma: float = 0.08, spread: float = 0.01) -> Dict[str, np.ndarray]:
    """Copy of `state` whose density head gives a thin, everywhere-positive fog (raw sigma ~ `sigma`).

    With such a COARSE network every coarse bin carries comparable weight, so the inverse-CDF importance
    sampling of the reference (nerf/rays/rays.py:87-119) is well conditioned and end-to-end results can be
    compared on every ray; with the raw random networks a few percent of the importance samples fall in
    nearly empty bins where the reference's own output is not reproducible to 1e-4."""
    out = {k: v.copy() for k, v in state.items()}
    out["_alpha_linear.weight"] = (out["_alpha_linear.weight"] * np.float32(spread)).astype(np.float32)
    out["_alpha_linear.bias"] = np.full_like(out["_alpha_linear.bias"], sigma)
    return out


def thin_fog_output(state: Dict[str, np.ndarray], sigma: float = 0.08, spread: float = 0.01) -> Dict[str, np.ndarray]:
    """`thin_fog` for a use_view_dirs=False network: row 3 of `_output_linear` is the density (raw[..., 3], model_utils.py:71)."""
    out = {k: v.copy() for k, v in state.items()}
    out["_output_linear.weight"][3] = (out["_output_linear.weight"][3] * np.float32(spread)).astype(np.float32)
    out["_output_linear.bias"][3] = np.float32(sigma)
    return out


def dense_fog(state: Dict[str, np.ndarray], sigma: float = 3.0, spread: float = 0.01) -> Dict[str, np.ndarray]:
    """`thin_fog` with a density that ends rays: the scenes of early ray termination (Renderer.set_early_termination).

    The defaults give a uniform fog (raw sigma ~ 3) in which every ray's transmittance falls below 1e-2 after about 1.5
    units of depth.  A large `spread` makes the density depend on the position: sigma = 0.5, spread = 3.0 leaves a quarter
    of the rays of a room-sized frame above 1e-2 to the end while their neighbours stop - workgroups in which some rays
    stop and some never do."""
    return thin_fog(state, sigma, spread)


def _room_trunk(state: Dict[str, np.ndarray], half_extent: float, slope: float) -> Dict[str, np.ndarray]:
    """The six wall units of `room` in the trunk of a copy of `state`: hidden units 0..5 of every `_pts_linears` layer."""
    out = {k: v.copy() for k, v in state.items()}
    in_xyz = out["_pts_linears.0.weight"].shape[1]
    W = out["_pts_linears.0.weight"].shape[0]
    depth = sum(1 for k in out if k.startswith("_pts_linears.") and k.endswith(".weight"))
    if W < 8:
        raise ValueError("room needs a trunk of at least 8 units: six of them are the walls")
    w0, b0 = out["_pts_linears.0.weight"], out["_pts_linears.0.bias"]
    for axis in range(3):
        for k, sign in enumerate((1.0, -1.0)):
            unit = 2 * axis + k
            w0[unit] = 0.0
            w0[unit, axis] = np.float32(sign * 10.0 * slope)      # the identity slot of gamma(x) holds x / 10
            b0[unit] = np.float32(-slope * half_extent)
    for i in range(1, depth):
        w, b = out[f"_pts_linears.{i}.weight"], out[f"_pts_linears.{i}.bias"]
        first = w.shape[1] - W          # in_xyz at the layer behind the skip (cat([input_pts, h])), else 0
        assert first in (0, in_xyz)
        w[:, first:first + 6] = 0.0     # no other unit reads the six
        w[:6] = 0.0
        b[:6] = 0.0
        for unit in range(6):
            w[unit, first + unit] = 1.0  # relu(1 * h) = h: the unit copies itself
    return out


def room(state: Dict[str, np.ndarray], half_extent: float = 3.0, slope: float = 1.0, gain: float = 8.0, floor: float = -2.0,
         spread: float = 0.01) -> Dict[str, np.ndarray]:
    """Copy of `state` with an empty interior and walls at +-`half_extent` on all three axes, built exactly, without training.

    Six hidden units, indices 0..5, are reserved.  In `_pts_linears.0` unit 2a + k reads only the identity slot a of gamma(x) and
    gives relu(slope * (+-x_a - half_extent)): the distance behind a wall.  Every later trunk layer copies the six and lets no
    other unit read them; `_feature_linear` ignores them; `_alpha_linear` weighs them with `gain` and everything else with
    `spread` times its random weights, with bias `floor`.  So sigma_raw ~ floor < 0 inside the room - empty space, where the fogs
    of this module have density everywhere - and rises linearly behind a wall.  The colours stay the random network's."""
    out = _room_trunk(state, half_extent, slope)
    out["_feature_linear.weight"][:, :6] = 0.0
    alpha = (out["_alpha_linear.weight"] * np.float32(spread)).astype(np.float32)
    alpha[0, :6] = np.float32(gain)
    out["_alpha_linear.weight"] = alpha
    out["_alpha_linear.bias"] = np.full_like(out["_alpha_linear.bias"], floor)
    return out


def room_output(state: Dict[str, np.ndarray], half_extent: float = 3.0, slope: float = 1.0, gain: float = 8.0, floor: float = -2.0,
                spread: float = 0.01) -> Dict[str, np.ndarray]:
    """`room` for a use_view_dirs=False network: row 3 of `_output_linear` is the density, the other rows ignore the six units."""
    out = _room_trunk(state, half_extent, slope)
    w = out["_output_linear.weight"]
    w[3] = (w[3] * np.float32(spread)).astype(np.float32)
    w[:, :6] = 0.0
    w[3, :6] = np.float32(gain)
    out["_output_linear.bias"][3] = np.float32(floor)
    return out
