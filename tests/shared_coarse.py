"""The coarse pass shared by k x k pixel blocks (include/nwe.h: nwe_set_shared_coarse): the block arithmetic restated without a
GPU, and the reference of the rule.

The rule, in reference terms: ray r takes the importance samples of its block's representative ray rep(r) of the same pose -
sample_pdf(z_mid, weights[rep][..., 1:-1], ...) at nerf_replica_inference_handler.py:237 - and since the coarse depths are the
frame's, z_fine[r] is the ordinary frame's z_fine[rep(r)].  Everything behind is the ray's own, so the reference is the oracle's
ordinary render followed by its fine pass on those depths (`shared_reference`).  Scenes are those of tests/early_termination.py.
"""
import functools

import numpy as np
import torch

from oracle import nerf_oracle as O
from tests import early_termination as E


def rep_index(H, W, k, row_begin, row_end, n_poses):
    """For every ray of a call over rows [row_begin, row_end) of n_poses poses, in the call's ray order (pose, row, column): the
    index of its representative among the rays of the WHOLE frames, (p * H + rh) * W + rw with the representative pixel
    (rh, rw) = (min(k (h // k) + k // 2, H - 1), min(k (w // k) + k // 2, W - 1)).  It may lie outside the call's rows."""
    h = np.arange(row_begin, row_end, dtype=np.int64)
    w = np.arange(W, dtype=np.int64)
    rh = np.minimum(h // k * k + k // 2, H - 1)
    rw = np.minimum(w // k * k + k // 2, W - 1)
    p = np.arange(n_poses, dtype=np.int64)
    return ((p[:, None, None] * H + rh[None, :, None]) * W + rw[None, None, :]).reshape(-1)


def n_rep(H, W, k, row_begin, row_end, n_poses):
    """Representatives of such a call: every block column of the block rows its rows touch, per pose."""
    if row_end <= row_begin:
        return 0
    return n_poses * ((row_end - 1) // k - row_begin // k + 1) * -(-W // k)


def evaluations(H, W, k, row_begin, row_end, n_poses, ns, ni):
    """(executed, full) ray evaluations of such a call (nwe_last_ray_evaluations)."""
    rays = n_poses * (row_end - row_begin) * W
    full = rays * (ns + (ns + ni if ni > 0 else 0))
    if k == 1 or ni == 0:
        return full, full
    return n_rep(H, W, k, row_begin, row_end, n_poses) * ns + rays * (ns + ni), full


def _tensors(sd):
    return {key: torch.from_numpy(v) for key, v in sd.items()}


@functools.lru_cache(maxsize=None)
def shared_reference(name, k, dtype=torch.float32):
    """rgb / depth / acc of scene `name` under the rule: the oracle's ordinary render, then its fine pass of every ray on the
    depths of the ray's representative.  dtype = float64: the same from the oracle's fp64 evaluation (its own error bar).
    Computed once and shared: leave it unchanged."""
    _, sd_f, cfg, poses, rays, ref = E.scene(name)
    H, W = E.SCENES[name][6:8]
    if dtype == torch.float64:
        ref = E.reference_fp64(name)
    rep = torch.from_numpy(rep_index(H, W, k, 0, H, poses.shape[0]))
    out = O.fine_pass_given_depths(rays.to(dtype), ref["z_fine"][rep], O.cast_state(_tensors(sd_f), dtype), cfg)
    return {"rgb": out["rgb_fine"], "depth": out["depth_fine"], "acc": out["acc_fine"]}
