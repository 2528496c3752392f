"""Drop-in for the reference's ``NeRFReplicaInferenceHandler`` (nerf/inference/
nerf_replica_inference_handler.py:23-277) backed by the HIP render path.

Same three public methods with the same argument types and return value as the reference:

* ``__init__(office_name, ckpt_path)``                                   (handler.py:25)
* ``initialize_models()``                                                (handler.py:88)
* ``render_coordinates(init_coordinates, coordinates) -> uint8 [H,W,3]`` (handler.py:166)

plus the call surface BASELINE.json names, ``render(camera_pose, H, W)`` / ``render_batch(poses, H, W)``,
the internal seam ``_render_rays(flat_rays)`` (handler.py:187), and the point query ``run_network(inputs, viewdirs)``
(model_utils.py:13-30) with ``density_grid(lo, hi, resolution)`` on top of it.  Python here does weight loading,
pose math and I/O only; rays, sampling, encoding, both MLPs and compositing run in libnwe_hip.so.
Dropped side effects of the reference (none affects results): ``torch.cuda.empty_cache()`` (:86),
``eval()`` on YAML strings (:42-50), the tqdm bar, the ConfigParser singleton.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .camera_poses import get_camera_poses_from_list_of_coordinates
from .config import Config, parse_product
from .data_descriptors import COORD
from .renderer import Renderer, TiledRenderer

_FLAG_KEYS = {1 << 0: "rgb_fine", 1 << 1: "depth_fine", 1 << 2: "acc_fine", 1 << 3: "disp_fine", 1 << 4: "rgb_coarse",
              1 << 5: "depth_coarse", 1 << 6: "acc_coarse", 1 << 7: "disp_coarse", 1 << 8: "raw", 1 << 9: "z_std"}


def load_checkpoint(path: str) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """(coarse, fine) state dicts of a reference checkpoint: a torch-saved dict with
    ``network_coarse_state_dict`` / ``network_fine_state_dict`` (nerf/training/
    nerf_replica_training_handler.py:404-407).  Loaded with ``weights_only=True`` (tensors only)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    return ckpt["network_coarse_state_dict"], ckpt["network_fine_state_dict"]


def pinhole_intrinsics(H: int, W: int, hfov_deg: float = 90.0) -> Tuple[float, float, float, float]:
    """handler.py:67-74: fx = fy = W/2/tan(hfov/2) (fy is derived from the WIDTH), centre of the pixel grid."""
    fx = W / 2.0 / math.tan(math.radians(hfov_deg / 2.0))
    return fx, fx, (W - 1.0) / 2.0, (H - 1.0) / 2.0


class NeRFReplicaInferenceHandler:

    def __init__(self, office_name: str, ckpt_path: str, device: int = 0, precision: str = "auto",
                 devices: Optional[Sequence[int]] = None, early_termination: float = 0.0, shared_coarse: int = 1,
                 separate_passes: Optional[bool] = None, occupancy: Optional[Mapping[str, object]] = None,
                 baked_coarse: Optional[Mapping[str, object]] = None,
                 radiance_grid: Optional[Mapping[str, object]] = None,
                 sparse_fine: Optional[Mapping[str, object]] = None, sparse_async: Optional[bool] = None,
                 adaptive: Optional[Mapping[str, object]] = None, adaptive_lists: Optional[bool] = None,
                 adaptive_levels: Optional[int] = None) -> None:
        """``adaptive_levels``: an integer 1 .. 4, or NWE_ADAPTIVE_LEVELS=n in the environment, draws the adaptive frame on that many
        nested lattices (Renderer.render_adaptive, ``levels``): ``adaptive``'s k is the finest spacing, k 2^(levels - 1) <= 64 the
        coarsest.  It is an option of ``adaptive``: given without it, a ValueError.  Off (None) by default: the one-level call.
        ``adaptive_lists``: True, or NWE_ADAPTIVE_LISTS=1 in the environment, lets the adaptive frame hand its pixel lists to
        the list kernels of ``render_pixels`` (Renderer.set_adaptive_pixel_lists): the same frame, its rendered pixels on lean
        kernels.  It is an option of ``adaptive``: given without it, a ValueError.  Off by default.
        ``adaptive``: a mapping with optional "k" (2), "tol_rgb" (2/255) and "tol_depth" (0.05): with it
        ``render_coordinates(preview=False)`` draws its frame through ``render_adaptive_batch`` - every k-th pixel and the
        pixels of the lattice cells whose corners disagree rendered by the networks, the rest interpolated
        (Renderer.render_adaptive) - an approximation, off by default.  The environment variable NWE_ADAPTIVE =
        "k,tol_rgb[,tol_depth]" overrides the three, and switches the option on for two-argument callers.  It is refused
        together with ``sparse_fine``, ``early_termination > 0``, ``shared_coarse > 1``, ``occupancy``, ``baked_coarse`` and
        ``devices``; previews are unchanged.
        ``sparse_async``: True, or NWE_SPARSE_ASYNC=1 in the environment, makes ``render_coordinates`` draw its sparse frame
        through the asynchronous call (Renderer.render_sparse(asynchronous=True)): the same frame, queued instead of waited for
        chunk by chunk.  It is an option of ``sparse_fine``: given without it, a ValueError.  Off by default.
        ``sparse_fine``: a mapping with optional "min_weight" (1e-3), "dilate" (1) and "which" ("fine"): with it
        ``render_coordinates(preview=False)`` draws its frame through ``render_sparse_batch`` - the radiance grid as a proposal,
        the network only at the samples the grid gives weight (Renderer.render_sparse) - an approximation, off by default.  It
        needs ``radiance_grid`` too (a ValueError otherwise).  The environment variable NWE_SPARSE_FINE = "min_weight[,dilate]"
        overrides the two, and switches the option on for a caller that gave a radiance grid.
        ``radiance_grid``: a mapping with the box "lo", "hi" (world coordinates) and optionally "resolution" (128, one int or
        three), "which" ("fine") and "view_dir" (None: the mean over the six axis directions): initialize_models() bakes the
        network's raw output into a radiance grid over the box (bake_radiance_grid), from which ``render_grid`` and
        ``render_coordinates(preview="grid")`` render preview frames without running a network - an approximation; no other
        frame reads the grid.  The environment variable NWE_RADIANCE_GRID = "res" overrides the resolution over the box given
        here, for the same two-argument callers; without a box there is no grid.  One device only: not with ``devices``.
        ``baked_coarse``: a mapping with the box "lo", "hi" (world coordinates) and optionally "resolution" (128, one int or
        three): initialize_models() bakes the coarse network's density into a grid over the box (Renderer.bake_coarse_grid) and
        frames take their coarse weights from it instead of running the coarse network - an approximation, off by default.
        The environment variable NWE_BAKED_COARSE = "res" overrides the resolution over the box given here, for the same
        two-argument callers; without a box there is no grid.  While a grid is set ``_render_rays`` raises what the ABI says;
        it is refused together with ``early_termination > 0``, ``shared_coarse > 1``, ``separate_passes`` and ``occupancy``.
        ``occupancy``: a mapping with the box "lo", "hi" (world coordinates) and optionally "resolution" (128), "probes" (2),
        "dilate" (1), "threshold" (0.0): initialize_models() builds an occupancy grid over the box from the networks it has
        uploaded (Renderer.build_occupancy) and frames skip the samples in cells it marks empty.  The environment variable
        NWE_OCCUPANCY = "res[,probes[,dilate]]" overrides these three over the box given here, for the same two-argument
        callers; without a box there is no grid.  While a grid is set ``_render_rays`` raises what the ABI says; it is
        refused together with ``early_termination > 0``, ``shared_coarse > 1`` and ``separate_passes``.
        ``early_termination`` (or the environment variable NWE_EARLY_TERMINATION, for the same two-argument callers):
        the minimum transmittance of Renderer.set_early_termination, applied in initialize_models(); 0 = off.  While it is on,
        frames (render, render_batch, render_coordinates) are terminated and ``_render_rays`` raises what the ABI says.
        ``shared_coarse`` (or the environment variable NWE_SHARED_COARSE): the block edge k of Renderer.set_shared_coarse,
        applied in initialize_models(); 1 = off.  While it is on, frames share their coarse pass over k x k pixel blocks and
        ``_render_rays`` raises what the ABI says.  It is refused together with ``early_termination > 0``.
        ``separate_passes`` (or the environment variable NWE_SEPARATE_PASSES = 0 / 1, read when the argument is None):
        Renderer.set_separate_passes, applied in initialize_models(); off by default.  While it is on, "auto" keeps a coarse and
        a fine network of two different MFMA shapes on the MFMA path (f16x3): the coarse and the fine pass are launched
        separately, each with the kernel of its own shape.  It is refused together with ``early_termination > 0``.
        ``devices`` (or the environment variable NWE_DEVICES, e.g. "0,1,2,3", for a caller that constructs the handler
        with the reference's two arguments, application/workspace.py:28-29): render every frame as row tiles on these
        devices from this one process (renderer.TiledRenderer); a device may be listed more than once."""
        self._office_name = office_name
        self._ckpt_path = ckpt_path
        self._device_index = device
        if devices is None and os.environ.get("NWE_DEVICES"):
            devices = [int(d) for d in os.environ["NWE_DEVICES"].split(",") if d.strip() != ""]
        self._devices = list(devices) if devices else None
        if not early_termination and os.environ.get("NWE_EARLY_TERMINATION"):
            early_termination = float(os.environ["NWE_EARLY_TERMINATION"])
        if not 0.0 <= early_termination < 1.0:      # NaN fails too
            raise ValueError("early_termination (min_transmittance) must be in [0, 1)")
        self._early_termination = float(early_termination)
        if shared_coarse is not True and shared_coarse == 1 and os.environ.get("NWE_SHARED_COARSE"):
            shared_coarse = int(os.environ["NWE_SHARED_COARSE"])
        if isinstance(shared_coarse, bool) or not isinstance(shared_coarse, int) or not 1 <= shared_coarse <= 16:
            raise ValueError("shared_coarse (block edge k) must be an integer in 1..16")
        if shared_coarse > 1 and self._early_termination > 0.0:
            raise ValueError("shared_coarse > 1 and early_termination > 0 are not supported together")
        self._shared_coarse = shared_coarse
        if separate_passes is None:
            env = os.environ.get("NWE_SEPARATE_PASSES", "0").strip()
            if env not in ("", "0", "1"):
                raise ValueError("NWE_SEPARATE_PASSES (separate_passes) must be 0 or 1")
            separate_passes = env == "1"
        if not isinstance(separate_passes, bool):
            raise ValueError("separate_passes must be True, False or None")
        if separate_passes and self._early_termination > 0.0:
            raise ValueError("separate_passes and early_termination > 0 are not supported together")
        self._separate_passes = separate_passes
        self._occupancy = None
        if occupancy is not None:
            unknown = set(occupancy) - {"lo", "hi", "resolution", "probes", "dilate", "threshold"}
            if unknown or "lo" not in occupancy or "hi" not in occupancy:
                raise ValueError(f"occupancy needs 'lo' and 'hi' and may hold resolution, probes, dilate, threshold; got {sorted(occupancy)}")
            grid = {"resolution": 128, "probes": 2, "dilate": 1, "threshold": 0.0}
            grid.update(occupancy)
            env = [v.strip() for v in os.environ.get("NWE_OCCUPANCY", "").split(",") if v.strip() != ""]
            if len(env) > 3:
                raise ValueError("NWE_OCCUPANCY must be res[,probes[,dilate]]")
            for key, value in zip(("resolution", "probes", "dilate"), env):
                grid[key] = int(value)
            if self._early_termination > 0.0 or self._shared_coarse > 1 or self._separate_passes:
                raise ValueError("an occupancy grid is not supported together with early_termination > 0, shared_coarse > 1 or separate_passes")
            self._occupancy = grid
        self._baked_coarse = None
        if baked_coarse is not None:
            unknown = set(baked_coarse) - {"lo", "hi", "resolution"}
            if unknown or "lo" not in baked_coarse or "hi" not in baked_coarse:
                raise ValueError(f"baked_coarse needs 'lo' and 'hi' and may hold resolution; got {sorted(baked_coarse)}")
            grid = {"resolution": 128}
            grid.update(baked_coarse)
            env = os.environ.get("NWE_BAKED_COARSE", "").strip()
            if env != "":
                if not env.isdigit():
                    raise ValueError("NWE_BAKED_COARSE must be a resolution (one integer)")
                grid["resolution"] = int(env)
            if self._early_termination > 0.0 or self._shared_coarse > 1 or self._separate_passes or self._occupancy is not None:
                raise ValueError("a baked coarse pass is not supported together with early_termination > 0, shared_coarse > 1, "
                                 "separate_passes or an occupancy grid")
            self._baked_coarse = grid
        self._radiance_grid = None
        if radiance_grid is not None:
            unknown = set(radiance_grid) - {"lo", "hi", "resolution", "which", "view_dir"}
            if unknown or "lo" not in radiance_grid or "hi" not in radiance_grid:
                raise ValueError(f"radiance_grid needs 'lo' and 'hi' and may hold resolution, which, view_dir; got {sorted(radiance_grid)}")
            grid = {"resolution": 128, "which": "fine", "view_dir": None}
            grid.update(radiance_grid)
            env = os.environ.get("NWE_RADIANCE_GRID", "").strip()
            if env != "":
                if not env.isdigit():
                    raise ValueError("NWE_RADIANCE_GRID must be a resolution (one integer)")
                grid["resolution"] = int(env)
            if self._devices:
                raise ValueError("a radiance grid is rendered by one device: it is not supported together with devices")
            self._radiance_grid = grid
        self._sparse_fine = self.parse_sparse_fine(sparse_fine, os.environ.get("NWE_SPARSE_FINE", ""))
        if self._sparse_fine is not None and self._radiance_grid is None:
            raise ValueError("sparse_fine needs a radiance grid as its proposal: give radiance_grid={'lo': ..., 'hi': ...} too")
        env_async = os.environ.get("NWE_SPARSE_ASYNC", "").strip()
        if env_async not in ("", "0", "1"):
            raise ValueError("NWE_SPARSE_ASYNC must be 0 or 1")
        self._sparse_async = bool(sparse_async) if sparse_async is not None else env_async == "1"
        if self._sparse_async and self._sparse_fine is None:
            raise ValueError("sparse_async is an option of the sparse frame: give sparse_fine={...} (and a radiance grid) too")
        self._adaptive = self.parse_adaptive(adaptive, os.environ.get("NWE_ADAPTIVE", ""))
        if self._adaptive is not None:
            for on, other in ((self._sparse_fine is not None, "sparse_fine"), (self._early_termination > 0.0, "early_termination > 0"),
                              (self._shared_coarse > 1, "shared_coarse > 1"), (self._occupancy is not None, "an occupancy grid (occupancy)"),
                              (self._baked_coarse is not None, "a baked coarse pass (baked_coarse)"), (bool(self._devices), "devices")):
                if on:
                    raise ValueError(f"adaptive (the adaptive frame) is not supported together with {other}")
        env_lists = os.environ.get("NWE_ADAPTIVE_LISTS", "").strip()
        if env_lists not in ("", "0", "1"):
            raise ValueError("NWE_ADAPTIVE_LISTS must be 0 or 1")
        self._adaptive_lists = bool(adaptive_lists) if adaptive_lists is not None else env_lists == "1"
        if self._adaptive_lists and self._adaptive is None:
            raise ValueError("adaptive_lists is an option of the adaptive frame: give adaptive={...} too")
        self._adaptive_levels = self.parse_adaptive_levels(adaptive_levels, os.environ.get("NWE_ADAPTIVE_LEVELS", ""),
                                                           None if self._adaptive is None else self._adaptive["k"])
        # "auto": the fp32-grade MFMA mode (f16x3) where the network shape has an MFMA instantiation (every shape the
        # reference's configs use), else the fp32 vector-ALU HIP kernel, with a notice - a legal YAML (say net_width 64) must
        # render, slowly, rather than raise.  Decided in initialize_models(), when the shapes are known.
        if precision != "auto" and precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be 'auto' or one of {sorted(_lib.PRECISIONS)}")
        self._precision = precision
        self._auto_precision = precision == "auto"

        cfg = Config.for_office(office_name)
        self._endpoint_feat = cfg.get_param(("experiment", "endpoint_feat"), bool, default=False)
        self._net_depth_coarse = parse_product(cfg.get_param(("model", "net_depth"), str))
        self._net_width_coarse = parse_product(cfg.get_param(("model", "net_width"), str))
        self._net_depth_fine = parse_product(cfg.get_param(("model", "net_depth_fine"), str))
        self._net_width_fine = parse_product(cfg.get_param(("model", "net_width_fine"), str))
        self._net_chunk = parse_product(cfg.get_param(("model", "net_chunk"), str))    # kept for reference; the fused
        self._chunk = parse_product(cfg.get_param(("inference", "chunk"), str))        # kernel needs no chunking
        self._n_samples = cfg.get_param(("rendering", "n_samples"), int)
        self._n_importance = cfg.get_param(("rendering", "n_importance"), int)
        self._num_freqs_3d = cfg.get_param(("rendering", "num_freqs_3d"), int)
        self._num_freqs_2d = cfg.get_param(("rendering", "num_freqs_2d"), int)
        self._use_view_dirs = cfg.get_param(("rendering", "use_view_dirs"), bool)
        self._white_bkgd = cfg.get_param(("rendering", "white_background"), bool)
        self._img_h = cfg.get_param(("experiment", "image_height"), int)
        self._img_w = cfg.get_param(("experiment", "image_width"), int)
        self._depth_close_bound, self._depth_far_bound = cfg.get_param(("rendering", "depth_range"), list)
        # rendering.use_view_dirs = False (nerf_model.py:41-43,82-83) and experiment.endpoint_feat = True (:72-81, handler.py:248-271)
        # are off in all four reference YAMLs; both render here: networks without view directions through the MFMA kernel's
        # own instantiations (other shapes than its six through the fp32 HIP kernel), the endpoint feature map as
        # `feat_map_fine` of _render_rays (fp32 kernel; frames, which return rgb only, keep the MFMA kernel).
        self._fx, self._fy, self._cx, self._cy = pinhole_intrinsics(self._img_h, self._img_w)
        self._renderer: Optional[Renderer] = None
        self._stage: Optional[torch.Tensor] = None   # pinned uint8 [H,W,3] staging buffer for render_coordinates

    @staticmethod
    def parse_sparse_fine(sparse_fine: Optional[Mapping[str, object]], env: str = "") -> Optional[Dict[str, object]]:
        """The ``sparse_fine`` option with its defaults, NWE_SPARSE_FINE = "min_weight[,dilate]" (``env``) laid over it; None when
        neither is given."""
        env = [v.strip() for v in env.split(",") if v.strip() != ""]
        if sparse_fine is None and not env:
            return None
        opt = {"min_weight": 1e-3, "dilate": 1, "which": "fine"}
        if sparse_fine is not None:
            unknown = set(sparse_fine) - set(opt)
            if unknown:
                raise ValueError(f"sparse_fine may hold min_weight, dilate, which; got {sorted(sparse_fine)}")
            opt.update(sparse_fine)
        if len(env) > 2:
            raise ValueError("NWE_SPARSE_FINE must be min_weight[,dilate]")
        try:
            if env:
                opt["min_weight"] = float(env[0])
            if len(env) > 1:
                opt["dilate"] = int(env[1])
        except ValueError:
            raise ValueError("NWE_SPARSE_FINE must be min_weight[,dilate]") from None
        if isinstance(opt["min_weight"], bool) or not isinstance(opt["min_weight"], (int, float)) or opt["min_weight"] != opt["min_weight"]:
            raise ValueError("sparse_fine: min_weight must be a number, not NaN")
        if isinstance(opt["dilate"], bool) or not isinstance(opt["dilate"], int) or not 0 <= opt["dilate"] <= 8:
            raise ValueError("sparse_fine: dilate must be an integer in 0..8")
        if opt["which"] not in ("coarse", "fine"):
            raise ValueError("sparse_fine: which must be 'coarse' or 'fine'")
        opt["min_weight"] = float(opt["min_weight"])
        return opt

    @staticmethod
    def parse_adaptive(adaptive: Optional[Mapping[str, object]], env: str = "") -> Optional[Dict[str, object]]:
        """The ``adaptive`` option with its defaults, NWE_ADAPTIVE = "k,tol_rgb[,tol_depth]" (``env``) laid over it; None when
        neither is given."""
        env = [v.strip() for v in env.split(",") if v.strip() != ""]
        if adaptive is None and not env:
            return None
        opt = {"k": 2, "tol_rgb": 2 / 255, "tol_depth": 0.05}
        if adaptive is not None:
            unknown = set(adaptive) - set(opt)
            if unknown:
                raise ValueError(f"adaptive may hold k, tol_rgb, tol_depth; got {sorted(adaptive)}")
            opt.update(adaptive)
        if env and not 2 <= len(env) <= 3:
            raise ValueError("NWE_ADAPTIVE must be k,tol_rgb[,tol_depth]")
        try:
            if env:
                opt["k"], opt["tol_rgb"] = int(env[0]), float(env[1])
            if len(env) > 2:
                opt["tol_depth"] = float(env[2])
        except ValueError:
            raise ValueError("NWE_ADAPTIVE must be k,tol_rgb[,tol_depth]") from None
        if isinstance(opt["k"], bool) or not isinstance(opt["k"], int) or not 1 <= opt["k"] <= _lib.ADAPTIVE_MAX_K:
            raise ValueError("adaptive: k must be an integer in 1..64")
        for key in ("tol_rgb", "tol_depth"):
            if isinstance(opt[key], bool) or not isinstance(opt[key], (int, float)) or opt[key] != opt[key]:
                raise ValueError(f"adaptive: {key} must be a number, not NaN")
            opt[key] = float(opt[key])
        return opt

    @staticmethod
    def parse_adaptive_levels(levels: Optional[int], env: str = "", k: Optional[int] = None) -> Optional[int]:
        """The ``adaptive_levels`` option, NWE_ADAPTIVE_LEVELS (``env``) where it is not given; ``k``: the adaptive frame's k, None
        without an adaptive frame.  None when neither is given."""
        env = env.strip()
        if levels is None and env == "":
            return None
        if levels is None:
            try:
                levels = int(env)
            except ValueError:
                raise ValueError("NWE_ADAPTIVE_LEVELS must be an integer in 1..4") from None
        if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= _lib.ADAPTIVE_MAX_LEVELS:
            raise ValueError("adaptive_levels must be an integer in 1..4")
        if k is None:
            raise ValueError("adaptive_levels is an option of the adaptive frame: give adaptive={...} too")
        if k << (levels - 1) > _lib.ADAPTIVE_MAX_K:
            raise ValueError("adaptive_levels: k * 2^(levels - 1) must be at most 64")
        return levels

    # ------------------------------------------------------------------------------------------------
    def set_sampling(self, n_samples: int, n_importance: int) -> None:
        """Override the YAML sample counts (BASELINE configs use 32+0, 64+0 and 64+128)."""
        self._n_samples, self._n_importance = n_samples, n_importance
        if self._renderer is not None:
            self._renderer.set_sampling(n_samples, n_importance)

    def debug_set_fold(self, on: bool) -> None:
        """Test hook (Renderer.debug_set_fold): applies to the networks the next initialize_models() uploads."""
        self._fold = bool(on)

    def initialize_models(self, state_dicts: Optional[Tuple[Mapping, Mapping]] = None) -> None:
        """Load the checkpoint and upload both networks (handler.py:88-148).  Safe to call repeatedly
        (the GUI calls it on every window open, application/app.py:116).  ``state_dicts=(coarse, fine)``
        bypasses the file for synthetic weights."""
        if state_dicts is None:
            try:
                state_dicts = load_checkpoint(self._ckpt_path)
            except FileNotFoundError as exc:
                raise RuntimeError(f"Checkpoint path: {self._ckpt_path} for model cannot be found!") from exc
        if self._renderer is None:
            self._renderer = TiledRenderer(self._devices) if self._devices else Renderer(self._device_index)
        if getattr(self, "_fold", True) is False:
            self._renderer.debug_set_fold(False)
        coarse, fine = state_dicts
        for name, sd in (("coarse", coarse), ("fine", fine)):
            if sd is not None and any(k.lstrip("_").startswith("output_linear") for k in sd) == self._use_view_dirs:
                # the reference would fail in load_state_dict(strict) (handler.py:134-141): say which side is off
                raise RuntimeError(f"{name} network {'has no' if self._use_view_dirs else 'has'} view-direction heads but "
                                   f"rendering.use_view_dirs is {self._use_view_dirs}")
        self._renderer.set_network(_lib.NET_COARSE, coarse)
        if fine is not None:
            self._renderer.set_network(_lib.NET_FINE, fine)
        self._renderer.set_sampling(self._n_samples, self._n_importance)
        self._renderer.set_white_background(self._white_bkgd)                     # handler.py:57,231,253
        self._renderer.set_early_termination(self._early_termination)
        self._renderer.set_shared_coarse(self._shared_coarse)
        self._renderer.set_separate_passes(self._separate_passes)
        if self._adaptive_lists:
            self._renderer.set_adaptive_pixel_lists(True)
        if self._auto_precision:
            nets = (_lib.NET_COARSE,) + ((_lib.NET_FINE,) if fine is not None else ())
            each = all(self._renderer.mfma_supported(w) for w in nets)
            mfma, hint = each, ""
            if mfma and fine is not None and self._renderer.shapes[_lib.NET_COARSE] != self._renderer.shapes[_lib.NET_FINE]:
                # the fused MFMA kernel runs both passes with one instantiation; separate passes launch one per network, which
                # must still share their encodings (in_xyz, in_dir)
                same_encodings = self._renderer.shapes[_lib.NET_COARSE][2:4] == self._renderer.shapes[_lib.NET_FINE][2:4]
                # ... and so does a baked coarse pass, which runs the fine network's kernels only
                mfma = (self._separate_passes or self._baked_coarse is not None) and same_encodings
                if same_encodings and not mfma:
                    hint = "; separate_passes=True or NWE_SEPARATE_PASSES=1 renders such a pair with the MFMA kernels"
            self._precision = "f16x3" if mfma else "f32"
            if not mfma:
                shapes = " / ".join(str(self._renderer.shapes.get(w)) for w in nets)
                print(f"[nwe] network shape {shapes} has no MFMA instantiation: rendering with the "
                      f"fp32 vector-ALU kernel (same results, ~25x slower){hint}")
        if self._occupancy is not None:     # behind the networks (set_network clears a grid) and the precision
            self.build_occupancy(**self._occupancy)
        if self._baked_coarse is not None:
            self.bake_coarse_grid(**self._baked_coarse)
        if self._radiance_grid is not None:
            self.bake_radiance_grid(**self._radiance_grid)

    def _need_renderer(self) -> Renderer:
        if self._renderer is None:
            raise RuntimeError("initialize_models() has not been called")
        return self._renderer

    def _report_flags(self, flags: torch.Tensor) -> None:
        bits = int(flags.item())
        for bit, key in _FLAG_KEYS.items():
            if bits & bit:
                print(f"[Numerical Error] {key} contains NaN or inf.")   # handler.py:273-275

    # ------------------------------------------------------------------------------------------------
    def render(self, camera_pose, H: Optional[int] = None, W: Optional[int] = None, *,
               rows: Optional[Tuple[int, int]] = None, outputs: Sequence[str] = ("rgb", "depth", "acc"),
               precision: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """One pinhole view: 4x4 float32 camera-to-world pose -> device tensors rgb [h,W,3], depth [h,W],
        acc [h,W] (h = rows rendered, default all H).  Intrinsics as handler.py:67-74 for (H, W)."""
        res = self.render_batch(np.asarray(camera_pose, dtype=np.float32).reshape(1, 4, 4), H, W, rows=rows,
                                outputs=outputs, precision=precision)
        return {k: v[0] for k, v in res.items()}

    def render_batch(self, poses, H: Optional[int] = None, W: Optional[int] = None, *,
                     rows: Optional[Tuple[int, int]] = None, outputs: Sequence[str] = ("rgb", "depth", "acc"),
                     precision: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """[B,4,4] poses -> tensors with leading [B, h, W]; all B views in ONE kernel launch."""
        r = self._need_renderer()
        H = self._img_h if H is None else H
        W = self._img_w if W is None else W
        fx, fy, cx, cy = pinhole_intrinsics(H, W)
        poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        r0, r1 = rows if rows is not None else (0, H)
        # rows=None stays None: "the whole frame" is what a TiledRenderer splits over its devices
        res = r.render(poses, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=self._depth_close_bound, far=self._depth_far_bound,
                       rows=None if rows is None else (r0, r1), precision=precision or self._precision, outputs=outputs)
        out = {}
        for k, v in res.items():
            if k == "flags":
                out[k] = v
            else:
                out[k] = v.reshape((poses.shape[0], r1 - r0, W) + tuple(v.shape[1:]))
        return out

    def render_coordinates(self, init_coordinates: COORD, coordinates: COORD, *, out: Optional[np.ndarray] = None,
                           preview=False) -> np.ndarray:
        """handler.py:166-185: uint8 [H,W,3], C-contiguous (Qt wraps ``image.data`` with stride 3*W,
        application/app.py:339-340).

        Frame hand-off: ``to8b`` (model_utils.py:9, truncating) runs on the device, the 3 bytes/pixel image goes through
        a pinned staging buffer kept by the handler, and lands either in a fresh array (the reference's behaviour) or in
        ``out``, a caller-owned uint8 [H,W,3] array such as the one a GUI image wraps.  ``preview=True`` renders the coarse
        pass only (Ns samples through the coarse net, a quarter of the work) for a fast first image; ``preview="grid"`` renders
        from the radiance grid (render_grid: no network runs) and raises a RuntimeError when none is set."""
        r = self._need_renderer()
        from_grid = isinstance(preview, str)
        if from_grid:
            if preview != "grid":
                raise ValueError("preview must be False, True or 'grid'")
            if getattr(r, "radiance_grid", None) is None:
                raise RuntimeError('preview="grid" needs a radiance grid: call bake_radiance_grid(lo, hi, resolution) first')
            preview = False
        camera_pose = get_camera_poses_from_list_of_coordinates(init_coordinates, [coordinates])   # :170
        H, W = self._img_h, self._img_w
        if out is not None and (out.dtype != np.uint8 or out.shape != (H, W, 3) or not out.flags.c_contiguous):
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {(H, W, 3)}")
        if preview and self._n_importance > 0:
            r.set_sampling(self._n_samples, 0)
        try:
            if from_grid:
                res = self.render_grid_batch(camera_pose.numpy(), H, W, outputs=("rgb",))
            elif self._sparse_fine is not None and not preview:
                res = self.render_sparse_batch(camera_pose.numpy(), H, W, outputs=("rgb",), asynchronous=self._sparse_async,
                                               **self._sparse_fine)
            elif self._adaptive is not None and not preview:
                res = self.render_adaptive_batch(camera_pose.numpy(), H, W, outputs=("rgb",), levels=self._adaptive_levels, **self._adaptive)
            else:
                res = self.render_batch(camera_pose.numpy(), H, W, outputs=("rgb",))
        finally:
            if preview and self._n_importance > 0:
                r.set_sampling(self._n_samples, self._n_importance)
        img = r.to8b(res["rgb"][0])                                                                 # :183
        if self._stage is None or tuple(self._stage.shape) != (H, W, 3):
            self._stage = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True)
        self._stage.copy_(img.reshape(H, W, 3), non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        self._report_flags(res["flags"])
        if out is None:
            return self._stage.numpy().copy()
        np.copyto(out, self._stage.numpy())
        return out

    def _render_rays(self, flat_rays: torch.Tensor, outputs: Optional[Sequence[str]] = None,
                     precision: Optional[str] = None,
                     train: Optional[Dict[str, Optional[torch.Tensor]]] = None) -> Dict[str, torch.Tensor]:
        """handler.py:187-201: [R,11] rays -> dict keyed like the reference's output dict.  ``train`` = the forward pass of
        the training handler's renderer (nerf_replica_training_handler.py:536-600) on caller-drawn random numbers, see
        Renderer.render_rays."""
        r = self._need_renderer()
        fine = self._n_importance > 0
        precision = precision or self._precision
        if outputs is None:
            outputs = ["rgb", "disp", "acc", "depth", "rgb_coarse", "disp_coarse", "acc_coarse", "depth_coarse"]
            if fine:
                outputs.append("z_std")
            if fine and self._endpoint_feat and self._use_view_dirs:      # handler.py:270-271
                outputs.append("feat_map")
                precision = "f32"                                         # the composited view-layer features exist in the fp32 kernel only
        res = r.render_rays(flat_rays, precision=precision, outputs=outputs, train=train)
        rename = {"rgb": "rgb_fine", "disp": "disp_fine", "acc": "acc_fine", "depth": "depth_fine", "feat_map": "feat_map_fine"}
        return {rename.get(k, k): v for k, v in res.items() if not k.startswith("_")}

    # ------------------------------------------------------------------------------------------------
    def _query_net(self, which) -> Tuple[int, str]:
        """(network index, precision) of a point query: "auto" resolves per network - a query runs one network, so a coarse
        and a fine network of two MFMA shapes both stay on the MFMA kernels."""
        names = {"coarse": _lib.NET_COARSE, "fine": _lib.NET_FINE, _lib.NET_COARSE: _lib.NET_COARSE, _lib.NET_FINE: _lib.NET_FINE}
        if isinstance(which, bool) or which not in names:
            raise ValueError("which must be 'coarse' or 'fine'")
        w = names[which]
        r = self._need_renderer()
        if not self._auto_precision:
            return w, self._precision
        return w, "f16x3" if r.mfma_supported(w) else "f32"

    def run_network(self, inputs: torch.Tensor, viewdirs: Optional[torch.Tensor], which="fine",
                    precision: Optional[str] = None) -> torch.Tensor:
        """The reference's run_network (nerf/models/model_utils.py:13-30) on the render kernels: points ``inputs`` [N,S,3] and
        view directions ``viewdirs`` [N,3] (None with rendering.use_view_dirs = False) -> raw [N,S,4] = rgb_raw, sigma_raw of
        the ``which`` network.  World coordinates; the directions are used as given."""
        if inputs.dim() != 3 or inputs.shape[-1] != 3:
            raise ValueError(f"inputs must be [N,S,3], got {tuple(inputs.shape)}")
        if viewdirs is not None and tuple(viewdirs.shape) != (inputs.shape[0], 3):
            raise ValueError(f"viewdirs must be [N,3] = [{inputs.shape[0]},3], got {tuple(viewdirs.shape)}")
        w, auto = self._query_net(which)
        return self._need_renderer().query_points(inputs, viewdirs, which=w, precision=precision or auto, outputs=("raw",))["raw"]

    @staticmethod
    def grid_centres(lo: Sequence[float], hi: Sequence[float], resolution: Sequence[int], start: int = 0,
                     count: Optional[int] = None, device=None) -> torch.Tensor:
        """Cell centres [count,3] (float32) of the axis-aligned box lo..hi cut into resolution = (rx, ry, rz) cells, for the flat
        cell indices start .. start + count - 1 of the [rx, ry, rz] grid (z fastest).  Along an axis with r cells, cell i has
        its centre at (i + 0.5) * step + lo with step = (hi - lo) / r rounded to float32 once: a float32 product, then a
        float32 sum."""
        rx, ry, rz = (int(r) for r in resolution)
        count = rx * ry * rz - start if count is None else count
        i = torch.arange(start, start + count, dtype=torch.int64, device=device)
        index = (i // (ry * rz), (i // rz) % ry, i % rz)
        cols = []
        for idx, l, h, r in zip(index, lo, hi, (rx, ry, rz)):
            step = float(np.float32((float(h) - float(l)) / r))
            cols.append((idx.to(torch.float32) + 0.5) * step + float(np.float32(l)))
        return torch.stack(cols, -1)

    def density_grid(self, lo: Sequence[float], hi: Sequence[float], resolution, which="fine", chunk: int = 1 << 20,
                     precision: Optional[str] = None) -> torch.Tensor:
        """sigma_raw of the ``which`` network at the cell centres of the box lo..hi (world coordinates), [rx, ry, rz] on the
        device; ``resolution`` = one int or (rx, ry, rz).  The centres are generated on the device (grid_centres) and
        evaluated with the sigma-only query, ``chunk`` points at a time at the most."""
        res3 = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(r) for r in resolution)
        if len(res3) != 3 or min(res3) < 1 or len(lo) != 3 or len(hi) != 3:
            raise ValueError("density_grid needs lo, hi of three coordinates and a resolution of one or three positive ints")
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        w, auto = self._query_net(which)
        r = self._need_renderer()
        total = res3[0] * res3[1] * res3[2]
        out = torch.empty(total, dtype=torch.float32, device=r.device)
        for start in range(0, total, int(chunk)):
            count = min(int(chunk), total - start)
            pts = self.grid_centres(lo, hi, res3, start, count, device=r.device)
            out[start:start + count] = r.query_points(pts, None, which=w, precision=precision or auto, outputs=("sigma",))["sigma"]
        return out.reshape(res3)

    def build_occupancy(self, lo: Sequence[float], hi: Sequence[float], resolution=128, probes: int = 2, threshold: float = 0.0,
                        dilate: int = 1, precision: Optional[str] = None) -> None:
        """Builds an occupancy grid over the box lo..hi from the uploaded networks (Renderer.build_occupancy); frames then skip
        the samples in cells it marks empty, and ``_render_rays`` raises what the ABI says until clear_occupancy()."""
        self._need_renderer().build_occupancy(lo, hi, resolution, probes, threshold, dilate, precision or self._precision)

    def clear_occupancy(self) -> None:
        self._need_renderer().clear_occupancy()

    def bake_coarse_grid(self, lo: Sequence[float], hi: Sequence[float], resolution=128, precision: Optional[str] = None) -> None:
        """Bakes the coarse network's density over the box lo..hi into the renderer's coarse grid (Renderer.bake_coarse_grid);
        frames then take their coarse weights from it, and ``_render_rays`` raises what the ABI says until clear_coarse_grid()."""
        self._need_renderer().bake_coarse_grid(lo, hi, resolution, precision or self._query_net("coarse")[1])

    def clear_coarse_grid(self) -> None:
        self._need_renderer().clear_coarse_grid()

    _AXIS_DIRECTIONS = ((1., 0., 0.), (-1., 0., 0.), (0., 1., 0.), (0., -1., 0.), (0., 0., 1.), (0., 0., -1.))

    def _grid_renderer(self) -> Renderer:
        r = self._need_renderer()
        if isinstance(r, TiledRenderer):
            raise NotImplementedError("the radiance grid is rendered by one device (a grid frame is a few milliseconds): not with devices")
        return r

    def bake_radiance_grid(self, lo: Sequence[float], hi: Sequence[float], resolution=128, which="fine",
                           view_dir: Optional[Sequence[float]] = None, precision: Optional[str] = None, chunk: int = 1 << 20) -> None:
        """Bakes the raw output of the ``which`` network at the cell centres of the box lo..hi into the renderer's radiance grid;
        ``render_grid`` and ``render_coordinates(preview="grid")`` then render from it.  A given ``view_dir`` (three floats, used as
        given) is the one direction every cell is evaluated with (Renderer.bake_radiance_grid).  ``view_dir=None`` on a network with
        view directions bakes the mean of the raw rows over the six axis directions +x, -x, +y, -y, +z, -z: six queries through
        run_network, summed in float32 in that order and divided by 6 (sigma_raw does not depend on the direction); on a network
        without view directions it is the network's row."""
        r = self._grid_renderer()
        w, auto = self._query_net(which)
        precision = precision or auto
        if view_dir is not None or not self._use_view_dirs:
            r.bake_radiance_grid(lo, hi, resolution, w, view_dir, precision)
            return
        res3 = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
        if len(res3) != 3 or min(res3) < 1 or len(lo) != 3 or len(hi) != 3:
            raise ValueError("bake_radiance_grid needs lo, hi of three coordinates and a resolution of one or three positive ints")
        total = res3[0] * res3[1] * res3[2]
        raw = torch.empty((total, 4), dtype=torch.float32, device=r.device)
        for start in range(0, total, int(chunk)):
            count = min(int(chunk), total - start)
            pts = self.grid_centres(lo, hi, res3, start, count, device=r.device)[None]      # [1, count, 3]: one direction for all
            acc = None
            for d in self._AXIS_DIRECTIONS:
                row = self.run_network(pts, torch.tensor([d], dtype=torch.float32, device=r.device), which=w, precision=precision)[0]
                acc = row if acc is None else acc + row
            raw[start:start + count] = acc / 6.0
        r.set_radiance_grid(raw.reshape(res3 + (4,)), lo, hi)

    def clear_radiance_grid(self) -> None:
        self._need_renderer().clear_radiance_grid()

    @property
    def radiance_grid(self):
        """The renderer's radiance grid (Renderer.radiance_grid), None without one."""
        return getattr(self._need_renderer(), "radiance_grid", None)

    def render_grid(self, camera_pose, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                    outputs: Sequence[str] = ("rgb", "depth", "acc")) -> Dict[str, torch.Tensor]:
        """``render`` from the radiance grid (Renderer.render_grid): no network runs."""
        res = self.render_grid_batch(np.asarray(camera_pose, dtype=np.float32).reshape(1, 4, 4), H, W, rows=rows, outputs=outputs)
        return {k: v[0] for k, v in res.items()}

    def render_grid_batch(self, poses, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                          outputs: Sequence[str] = ("rgb", "depth", "acc")) -> Dict[str, torch.Tensor]:
        """``render_batch`` from the radiance grid: [B,4,4] poses -> tensors with leading [B, h, W], one launch."""
        r = self._grid_renderer()
        H = self._img_h if H is None else H
        W = self._img_w if W is None else W
        fx, fy, cx, cy = pinhole_intrinsics(H, W)
        poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        r0, r1 = rows if rows is not None else (0, H)
        res = r.render_grid(poses, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=self._depth_close_bound, far=self._depth_far_bound,
                            rows=(r0, r1), outputs=outputs)
        return {k: v if k == "flags" else v.reshape((poses.shape[0], r1 - r0, W) + tuple(v.shape[1:])) for k, v in res.items()}

    def _sparse_renderer(self) -> Renderer:
        r = self._need_renderer()
        if isinstance(r, TiledRenderer):
            raise NotImplementedError("the sparse frame is rendered by one device (TiledRenderer has no sparse frame): not with devices")
        return r

    def render_sparse(self, camera_pose, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                      which="fine", precision: Optional[str] = None, min_weight: float = 1e-3, dilate: int = 1,
                      outputs: Sequence[str] = ("rgb", "depth", "acc"), asynchronous: bool = False) -> Dict[str, torch.Tensor]:
        """``render`` as a sparse frame (Renderer.render_sparse): the ``which`` network only where the radiance grid sees weight."""
        res = self.render_sparse_batch(np.asarray(camera_pose, dtype=np.float32).reshape(1, 4, 4), H, W, rows=rows, which=which,
                                       precision=precision, min_weight=min_weight, dilate=dilate, outputs=outputs,
                                       asynchronous=asynchronous)
        return {k: v[0] for k, v in res.items()}

    def render_sparse_batch(self, poses, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                            which="fine", precision: Optional[str] = None, min_weight: float = 1e-3, dilate: int = 1,
                            outputs: Sequence[str] = ("rgb", "depth", "acc"), asynchronous: bool = False) -> Dict[str, torch.Tensor]:
        """``render_batch`` as a sparse frame: [B,4,4] poses -> tensors with leading [B, h, W].  ``precision`` None: the
        handler's own, "auto" resolved for the ``which`` network as run_network does.  ``asynchronous``: queued on the current
        stream, not waited for (Renderer.render_sparse)."""
        r = self._sparse_renderer()
        w, auto = self._query_net(which)
        H = self._img_h if H is None else H
        W = self._img_w if W is None else W
        fx, fy, cx, cy = pinhole_intrinsics(H, W)
        poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        r0, r1 = rows if rows is not None else (0, H)
        res = r.render_sparse(poses, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=self._depth_close_bound, far=self._depth_far_bound,
                              rows=(r0, r1), which=w, precision=precision or auto, min_weight=min_weight, dilate=dilate, outputs=outputs,
                              asynchronous=asynchronous)
        return {k: v if k == "flags" else v.reshape((poses.shape[0], r1 - r0, W) + tuple(v.shape[1:])) for k, v in res.items()}

    def last_sparse_samples(self):
        """(selected, total) samples of the last sparse frame (Renderer.last_sparse_samples), None if there was none."""
        return self._sparse_renderer().last_sparse_samples()

    def render_adaptive(self, camera_pose, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                        precision: Optional[str] = None, k: int = 2, tol_rgb: float = 2 / 255, tol_depth: float = 0.05,
                        outputs: Sequence[str] = ("rgb",), levels: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``render`` as an adaptive frame (Renderer.render_adaptive): a lattice of every k-th pixel, the cells that are not flat,
        the rest interpolated; ``levels``: None, or the nested lattices of the multi-level frame."""
        res = self.render_adaptive_batch(np.asarray(camera_pose, dtype=np.float32).reshape(1, 4, 4), H, W, rows=rows, precision=precision,
                                         k=k, tol_rgb=tol_rgb, tol_depth=tol_depth, outputs=outputs, levels=levels)
        return {name: v if name == "flags" else v[0] for name, v in res.items()}

    def render_adaptive_batch(self, poses, H: Optional[int] = None, W: Optional[int] = None, *, rows: Optional[Tuple[int, int]] = None,
                              precision: Optional[str] = None, k: int = 2, tol_rgb: float = 2 / 255, tol_depth: float = 0.05,
                              outputs: Sequence[str] = ("rgb",), levels: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``render_batch`` as an adaptive frame: [B,4,4] poses -> tensors with leading [B, h, W]; each pose has its own lattice."""
        r = self._need_renderer()
        if isinstance(r, TiledRenderer):
            raise NotImplementedError("the adaptive frame is rendered by one device (its lattice belongs to the rows of a call): not with devices")
        H = self._img_h if H is None else H
        W = self._img_w if W is None else W
        fx, fy, cx, cy = pinhole_intrinsics(H, W)
        poses = np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4)
        r0, r1 = rows if rows is not None else (0, H)
        res = r.render_adaptive(poses, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=self._depth_close_bound, far=self._depth_far_bound,
                                rows=(r0, r1), precision=precision or self._precision, k=k, tol_rgb=tol_rgb, tol_depth=tol_depth,
                                outputs=outputs, levels=levels)
        return {name: v if name == "flags" else v.reshape((poses.shape[0], r1 - r0, W) + tuple(v.shape[1:])) for name, v in res.items()}

    def _single_renderer(self, what: str) -> Renderer:
        r = self._need_renderer()
        if isinstance(r, TiledRenderer):
            raise NotImplementedError(f"{what} is rendered by one device: not with devices")
        return r

    def render_pixels(self, init_coordinates: COORD, coordinates: COORD, pixels) -> torch.Tensor:
        """The listed pixels of the view ``render_coordinates`` draws: ``pixels`` holds indices h * W + w into its image (an int32
        device tensor, or anything ``torch.as_tensor`` takes), in any order; returns their float rgb [n, 3] on the device, bit
        for bit the float frame gathered at the list (Renderer.render_pixels)."""
        r = self._single_renderer("a pixel list")
        camera_pose = get_camera_poses_from_list_of_coordinates(init_coordinates, [coordinates])
        H, W = self._img_h, self._img_w
        pixels = torch.as_tensor(pixels, dtype=torch.int32).reshape(-1).to(r.device)
        res = r.render_pixels(camera_pose.numpy(), H, W, pixels, fx=self._fx, fy=self._fy, cx=self._cx, cy=self._cy,
                              near=self._depth_close_bound, far=self._depth_far_bound, precision=self._precision, outputs=("rgb",))
        self._report_flags(res["flags"])
        return res["rgb"]

    def render_region(self, init_coordinates: COORD, coordinates: COORD, top: int, left: int, height: int, width: int) -> np.ndarray:
        """The rectangle [top, top + height) x [left, left + width) of the view ``render_coordinates`` draws: uint8
        [height, width, 3], equal to that crop of its image, with only those pixels rendered (Renderer.render_pixels; ``to8b`` on
        the device and the pinned staging of ``render_coordinates``)."""
        r = self._single_renderer("a region")
        H, W = self._img_h, self._img_w
        top, left, height, width = int(top), int(left), int(height), int(width)
        if height < 1 or width < 1 or top < 0 or left < 0 or top + height > H or left + width > W:
            raise ValueError(f"the region must be a non-empty rectangle inside the {H} x {W} image")
        camera_pose = get_camera_poses_from_list_of_coordinates(init_coordinates, [coordinates])
        rows_ = torch.arange(top, top + height, dtype=torch.int32, device=r.device)
        cols_ = torch.arange(left, left + width, dtype=torch.int32, device=r.device)
        pixels = (rows_[:, None] * W + cols_[None, :]).reshape(-1)
        res = r.render_pixels(camera_pose.numpy(), H, W, pixels, fx=self._fx, fy=self._fy, cx=self._cx, cy=self._cy,
                              near=self._depth_close_bound, far=self._depth_far_bound, precision=self._precision, outputs=("rgb",))
        img = r.to8b(res["rgb"])
        if self._stage is None or tuple(self._stage.shape) != (H, W, 3):
            self._stage = torch.empty((H, W, 3), dtype=torch.uint8, pin_memory=True)
        stage = self._stage.view(-1)[:height * width * 3].view(height, width, 3)   # the head of the frame's staging buffer
        stage.copy_(img.reshape(height, width, 3), non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        self._report_flags(res["flags"])
        return stage.numpy().copy()

    def last_adaptive(self):
        """The counts and the device span of the last adaptive frame (Renderer.last_adaptive), None if there was none."""
        return self._need_renderer().last_adaptive()

    def last_adaptive_levels(self):
        """The report of the last multi-level adaptive frame (Renderer.last_adaptive_levels), None if there was none."""
        return self._need_renderer().last_adaptive_levels()

    @property
    def coarse_grid(self):
        """The renderer's coarse density grid (Renderer.coarse_grid), None without one."""
        return self._need_renderer().coarse_grid

    @property
    def occupancy(self):
        """The renderer's grid (Renderer.occupancy), None without one."""
        return self._need_renderer().occupancy

    # ------------------------------------------------------------------------------------------------
    @property
    def renderer(self) -> Renderer:
        return self._need_renderer()

    @property
    def early_termination(self) -> float:
        """The minimum transmittance initialize_models() applies (0 = off)."""
        return self._early_termination

    @property
    def shared_coarse(self) -> int:
        """The block edge initialize_models() applies (1 = off)."""
        return self._shared_coarse

    @property
    def separate_passes(self) -> bool:
        """What initialize_models() hands to Renderer.set_separate_passes."""
        return self._separate_passes

    @property
    def image_size(self) -> Tuple[int, int]:
        return self._img_h, self._img_w
