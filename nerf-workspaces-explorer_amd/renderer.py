"""Thin host wrapper over the C ABI (include/nwe.h): owns one ``nwe_ctx``, allocates the output tensors
with torch (device memory and streams only) and hands raw pointers to the HIP library.

No arithmetic of the render path happens here; if ``libnwe_hip.so`` is missing every entry point raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

LAYER_ORDER_TAIL = ("_views_linears.0", "_feature_linear", "_alpha_linear", "_rgb_linear")

_PER_RAY = {"rgb": 3, "depth": 1, "acc": 1, "disp": 1, "z_std": 1, "rgb_coarse": 3, "depth_coarse": 1,
            "acc_coarse": 1, "disp_coarse": 1, "sample_cond": 1, "sample_amp": 1, "sample_switch": 1}


def normalize_state_dict(sd: Mapping[str, object]) -> Dict[str, np.ndarray]:
    """Accept both spellings of the reference's keys: checkpoints carry ``pts_linears.0.weight``, the
    current modules ``_pts_linears.0.weight`` (nerf_replica_inference_handler.py:150-164)."""
    out = {}
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        out[k if k.startswith("_") else "_" + k] = v
    return out


def net_shape(sd: Mapping[str, np.ndarray]) -> Tuple[int, int, int, int, int]:
    """(D, W, in_xyz, in_dir, skip_layer) from the tensor shapes (nerf/models/nerf_model.py:32-43)."""
    D = 0
    while f"_pts_linears.{D}.weight" in sd:
        D += 1
    if D == 0:
        raise ValueError("state dict has no _pts_linears.0.weight")
    W, in_xyz = sd["_pts_linears.0.weight"].shape
    # use_view_dirs=False (nerf_model.py:41-43): `_output_linear` instead of the alpha / feature / rgb heads, no direction input
    in_dir = 0 if "_output_linear.weight" in sd else sd["_views_linears.0.weight"].shape[1] - W
    skip = -1
    for i in range(1, D):
        k = sd[f"_pts_linears.{i}.weight"].shape[1]
        if k == W + in_xyz:
            if skip != -1:
                raise ValueError("more than one skip connection is not supported")
            skip = i - 1
        elif k != W:
            raise ValueError(f"_pts_linears.{i}.weight has unexpected input width {k}")
    return D, int(W), int(in_xyz), int(in_dir), skip


class Renderer:
    """One HIP context on one GPU.  Not thread-safe (like the reference handler)."""

    def __init__(self, device: int = 0, host_only: bool = False):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        self.device_index = -1 if host_only else int(device)
        rc = self._lib.nwe_create(C.byref(self._ctx), self.device_index)
        if rc != _lib.NWE_OK:
            raise RuntimeError(f"nwe_create failed: {self._lib.nwe_last_error(None).decode()}")
        self.device = None if host_only else torch.device("cuda", self.device_index)
        self.n_samples = 0
        self.n_importance = 0
        self.shapes: Dict[int, Tuple[int, int, int, int, int]] = {}

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.nwe_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc != _lib.NWE_OK:
            msg = self._lib.nwe_last_error(self._ctx).decode()
            exc = NotImplementedError if rc == _lib.NWE_ERR_UNSUPPORTED else (ValueError if rc == _lib.NWE_ERR_INVALID else RuntimeError)
            raise exc(f"{what}: {msg}")

    # -- set-up -----------------------------------------------------------------------------------
    def set_network(self, which: int, state_dict: Mapping[str, object]) -> Tuple[int, int, int, int, int]:
        sd = normalize_state_dict(state_dict)
        D, W, in_xyz, in_dir, skip = net_shape(sd)
        if in_dir == 0:     # NeRFModel(use_view_dirs=False): trunk + _output_linear (nerf_model.py:41-43,82-83)
            names = [f"_pts_linears.{i}" for i in range(D)] + ["_output_linear"]
            out_ch = int(sd["_output_linear.weight"].shape[0])
            expect_in = [in_xyz] + [W + in_xyz if i - 1 == skip else W for i in range(1, D)] + [W]
            expect_out = [W] * D + [out_ch]
        else:
            names = [f"_pts_linears.{i}" for i in range(D)] + list(LAYER_ORDER_TAIL)
            expect_in = [in_xyz] + [W + in_xyz if i - 1 == skip else W for i in range(1, D)] + [W + in_dir, W, W, W // 2]
            expect_out = [W] * D + [W // 2, W, 1, 3]
        ws = [sd[n + ".weight"] for n in names]
        bs = [sd[n + ".bias"] for n in names]
        for n, w, b, ki, ko in zip(names, ws, bs, expect_in, expect_out):
            if w.shape != (ko, ki) or b.shape != (ko,):
                raise ValueError(f"{n}: expected weight [{ko},{ki}] and bias [{ko}], got {w.shape} / {b.shape}")
        wp = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
        if in_dir == 0:
            self._check(self._lib.nwe_set_network_no_view_dirs(self._ctx, which, D, W, in_xyz, skip, out_ch, wp, bp),
                        "nwe_set_network_no_view_dirs")
        else:
            self._check(self._lib.nwe_set_network(self._ctx, which, D, W, in_xyz, in_dir, skip, wp, bp), "nwe_set_network")
        self.shapes[which] = (D, W, in_xyz, in_dir, skip)
        return self.shapes[which]

    @property
    def ray_columns(self) -> int:
        """11 ([o d near far viewdir], rays.py:26-30), or 8 when the networks take no view directions (rays.py:22)."""
        return 8 if self.shapes.get(_lib.NET_COARSE, (0, 0, 0, 27, 0))[3] == 0 else 11

    def set_sampling(self, n_samples: int, n_importance: int) -> None:
        """Tables come from torch.linspace on the host, whose bits differ from i/(n-1)."""
        t = torch.linspace(0., 1., steps=n_samples)                    # handler.py:216
        omt = 1. - t                                                   # handler.py:218
        u = torch.linspace(0., 1., steps=max(n_importance, 1))         # nerf/rays/rays.py:95
        self._check(self._lib.nwe_set_sampling(self._ctx, t.numpy().ctypes.data, omt.numpy().ctypes.data, n_samples,
                                               u.numpy().ctypes.data if n_importance > 0 else None, n_importance),
                    "nwe_set_sampling")
        self.n_samples, self.n_importance = n_samples, n_importance

    # -- rendering --------------------------------------------------------------------------------
    def _alloc(self, n_rays: int, outputs: Iterable[str]) -> Tuple[_lib.Outputs, Dict[str, torch.Tensor]]:
        res: Dict[str, torch.Tensor] = {}
        S = self.n_samples + self.n_importance
        for name in outputs:
            if name in _PER_RAY:
                shape = (n_rays, 3) if _PER_RAY[name] == 3 else (n_rays,)
            elif name == "weights_coarse":
                shape = (n_rays, self.n_samples)
            elif name == "raw_coarse":
                shape = (n_rays, self.n_samples, 4)
            elif name == "raw_fine":
                shape = (n_rays, S, 4)
            elif name == "z_fine":
                shape = (n_rays, S)
            elif name == "feat_map":
                shape = (n_rays, self.shapes[_lib.NET_FINE][1] // 2)
            else:
                raise ValueError(f"unknown output {name!r}")
            res[name] = torch.empty(shape, dtype=torch.float32, device=self.device)
        res["flags"] = torch.zeros(1, dtype=torch.int32, device=self.device)
        o = _lib.Outputs()
        for name in _lib.OUTPUT_FIELDS:
            setattr(o, name, res[name].data_ptr() if name in res else None)
        return o, res

    def render(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
               rows: Optional[Tuple[int, int]] = None, precision: str = "f16x3",
               outputs: Sequence[str] = ("rgb", "depth", "acc")) -> Dict[str, torch.Tensor]:
        """Render rows [rows[0], rows[1]) of each pose.  c2w: [4,4] or [B,4,4] (numpy or CPU tensor)."""
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        n_rays = poses.shape[0] * (r1 - r0) * W
        with torch.cuda.device(self.device):
            o, res = self._alloc(n_rays, outputs)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.nwe_render(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1,
                                      _lib.PRECISIONS[precision], C.byref(o), stream)
        self._check(rc, "nwe_render")
        return res

    def create_rays(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                    rows: Optional[Tuple[int, int]] = None, use_view_dirs: bool = True) -> torch.Tensor:
        """[B*(rows)*W, 11] device rays, the layout and bits of nerf/rays/rays.py:6-32; use_view_dirs=False leaves the
        view-direction columns out ([.., 8], rays.py:22-30)."""
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        with torch.cuda.device(self.device):
            out = torch.empty((poses.shape[0] * (r1 - r0) * W, 11), dtype=torch.float32, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.nwe_create_rays(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1,
                                           out.data_ptr(), stream)
        self._check(rc, "nwe_create_rays")
        return out if use_view_dirs else out[:, :8].contiguous()

    def render_rays(self, rays: torch.Tensor, *, precision: str = "f16x3",
                    outputs: Sequence[str] = ("rgb", "depth", "acc"),
                    debug_fine_depths: Optional[torch.Tensor] = None,
                    debug_raw: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                    debug_coarse_weights: Optional[torch.Tensor] = None,
                    train: Optional[Dict[str, Optional[torch.Tensor]]] = None) -> Dict[str, torch.Tensor]:
        """rays: [R,11] fp32 on this renderer's device, the layout of nerf/rays/rays.py:26-30.
        ``debug_fine_depths`` ([R, Ns+Ni], test hook) replaces the importance sampling of the fine pass;
        ``debug_raw`` = (raw_coarse [R,Ns,4] or None, raw_fine [R,Ns+Ni,4] or None) replaces the MLP outputs;
        ``debug_coarse_weights`` [R,Ns] replaces the coarse pass (its outputs are then not written).

        ``train`` switches on the training-mode forward of nerf/training/nerf_replica_training_handler.py:553-580 with
        random numbers drawn by the caller where the reference draws them (any key may be missing / None):
        ``t_rand`` [R,Ns] = torch.rand (stratified jitter), ``noise_coarse`` [R,Ns] and ``noise_fine`` [R,Ns+Ni] =
        torch.randn * raw_noise_std (model_utils.py:64-71), ``u`` [R,Ni] = torch.rand of sample_pdf(det=False)
        (rays.py:98; sorted per ray here, which changes no output because the depths are sorted afterwards)."""
        if rays.dim() != 2 or rays.shape[1] != self.ray_columns or rays.dtype != torch.float32:
            raise ValueError(f"rays must be float32 [R,{self.ray_columns}] for these networks")
        rays = rays.to(self.device).contiguous()
        # Every hook argument is validated before any hook is armed: a ValueError leaves the context as it was.
        keep = []
        S = self.n_samples + self.n_importance
        if debug_fine_depths is not None:
            debug_fine_depths = debug_fine_depths.to(self.device, torch.float32).contiguous()
            if tuple(debug_fine_depths.shape) != (rays.shape[0], S):
                raise ValueError("debug_fine_depths must be [R, n_samples + n_importance]")
        raw_ptrs = None
        if debug_raw is not None:
            raw_ptrs = []
            for t, n in zip(debug_raw, (self.n_samples, S)):
                if t is None:
                    raw_ptrs.append(None)
                    continue
                t = t.to(self.device, torch.float32).contiguous()
                if tuple(t.shape) != (rays.shape[0], n, 4):
                    raise ValueError(f"debug_raw entries must be [R, {n}, 4]")
                keep.append(t)
                raw_ptrs.append(t.data_ptr())
        weights = None
        if debug_coarse_weights is not None:
            weights = debug_coarse_weights.to(self.device, torch.float32).contiguous()
            if tuple(weights.shape) != (rays.shape[0], self.n_samples):
                raise ValueError("debug_coarse_weights must be [R, n_samples]")
            keep.append(weights)
        train_ptrs = None
        if train:
            R, ns, ni = rays.shape[0], self.n_samples, self.n_importance
            shapes = {"t_rand": (R, ns), "noise_coarse": (R, ns), "noise_fine": (R, ns + ni), "u": (R, ni)}
            unknown = set(train) - set(shapes)
            if unknown:
                raise ValueError(f"unknown train keys {sorted(unknown)}")
            train_ptrs = []
            for key in ("t_rand", "noise_coarse", "noise_fine", "u"):
                t = train.get(key)
                if t is None:
                    train_ptrs.append(None)
                    continue
                t = t.to(self.device, torch.float32)
                if tuple(t.shape) != shapes[key]:
                    raise ValueError(f"train[{key!r}] must be {shapes[key]}")
                if key == "u":
                    t = torch.sort(t, dim=-1).values
                t = t.contiguous()
                keep.append(t)
                train_ptrs.append(t.data_ptr())
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        with torch.cuda.device(self.device):
            o, res = self._alloc(rays.shape[0], outputs)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if debug_fine_depths is not None:
                self._lib.nwe_debug_set_fine_depths(self._ctx, debug_fine_depths.data_ptr())
            if raw_ptrs is not None:
                self._lib.nwe_debug_set_raw(self._ctx, *raw_ptrs)
            if weights is not None:
                self._lib.nwe_debug_set_coarse_weights(self._ctx, weights.data_ptr())
            if train_ptrs is not None:
                self._lib.nwe_set_train_tables(self._ctx, *train_ptrs)
            rc = self._lib.nwe_render_rays(self._ctx, rays.data_ptr(), rays.shape[0], _lib.PRECISIONS[precision], C.byref(o), stream)
        if rc != _lib.NWE_OK:
            # a refused call consumes the hooks (include/nwe.h); disarmed here as well, while `keep` still holds the buffers
            self.disarm_hooks()
        self._check(rc, "nwe_render_rays")
        res["_keepalive_rays"] = rays
        if keep:
            res["_keepalive_train"] = keep
        if debug_fine_depths is not None:
            res["_keepalive_depths"] = debug_fine_depths
        return res

    def disarm_hooks(self) -> None:
        """Clears the one-shot hooks of ``render_rays`` (debug depths / raw / coarse weights, train tables)."""
        self._lib.nwe_debug_set_fine_depths(self._ctx, None)
        self._lib.nwe_debug_set_raw(self._ctx, None, None)
        self._lib.nwe_debug_set_coarse_weights(self._ctx, None)
        self._lib.nwe_set_train_tables(self._ctx, None, None, None, None)

    def debug_set_fold(self, on: bool) -> None:
        """Test hook: networks uploaded after this call are packed with (default) / without _feature_linear folded into the
        view layer (include/nwe.h)."""
        self._check(self._lib.nwe_debug_set_fold(self._ctx, 1 if on else 0), "nwe_debug_set_fold")

    def debug_set_decomposition(self, mode: int) -> None:
        """Test hook: 0 = four ray packets per workgroup, 1 = sample split, 2 = packets for the full rounds + sample split for the
        ragged last round, -1 = automatic (bit-identical results)."""
        self._check(self._lib.nwe_debug_set_decomposition(self._ctx, int(mode)), "nwe_debug_set_decomposition")

    def debug_last_plan(self) -> int:
        """Test hook: the decomposition the last MFMA launch took (0 packets, 1 sample split, 2 packets + split rest)."""
        return int(self._lib.nwe_debug_last_plan(self._ctx))

    def debug_set_work_queue(self, mode: int) -> None:
        """How a plain MFMA launch's workgroups get their work (include/nwe.h; bit-identical results): -1 = tickets from a queue
        when the launch has more workgroups than the device has CUs (the default, or what NWE_WORK_QUEUE set when the renderer
        was created), 0 = the hardware's static dealing, 1 = queue every launch."""
        self._check(self._lib.nwe_debug_set_work_queue(self._ctx, int(mode)), "nwe_debug_set_work_queue")

    def debug_get_work_queue(self) -> int:
        return int(self._lib.nwe_debug_get_work_queue(self._ctx))

    def debug_last_queue(self):
        """{"items", "grid", "taken": (first launch, second launch), "side_stream": bool} of the last render: the work items of
        each launch of its plan, its grid and the tickets taken (zeros = not queued), and whether the hybrid plan's second
        launch ran on the renderer's own low-priority stream."""
        items, grid, taken, side = (C.c_uint * 2)(), (C.c_uint * 2)(), (C.c_uint * 2)(), C.c_int(0)
        self._check(self._lib.nwe_debug_last_queue(self._ctx, items, grid, taken, C.byref(side)), "nwe_debug_last_queue")
        return {"items": tuple(items), "grid": tuple(grid), "taken": tuple(taken), "side_stream": bool(side.value)}

    def debug_last_tail(self) -> int:
        """The sample-split items that the packets launch of the last render rendered in its tail (include/nwe.h: the tail path of
        the work queue; all of the plan's split items when the path was taken), 0 when it was not."""
        stolen = C.c_uint(0)
        self._check(self._lib.nwe_debug_last_tail(self._ctx, C.byref(stolen)), "nwe_debug_last_tail")
        return int(stolen.value)

    def debug_last_tail_rest(self) -> int:
        """The split items that the SECOND launch of the last render rendered on the tail path: debug_last_tail() plus this is the
        plan's split items exactly if every item was rendered once; 0 when the path was not taken."""
        n = C.c_uint(0)
        self._check(self._lib.nwe_debug_last_tail_rest(self._ctx, C.byref(n)), "nwe_debug_last_tail_rest")
        return int(n.value)

    def debug_set_colour_skip(self, mode: int) -> None:
        """The hollow path of the lean MFMA kernels (include/nwe.h): 0 = off, 1 = on where the network's colour layers are finite as
        packed (the default, or what NWE_COLOUR_SKIP set when the renderer was created), 2 = test hook without that condition."""
        self._check(self._lib.nwe_debug_set_colour_skip(self._ctx, int(mode)), "nwe_debug_set_colour_skip")

    def debug_get_colour_skip(self) -> int:
        return int(self._lib.nwe_debug_get_colour_skip(self._ctx))

    def debug_set_packet_blocks(self, on: bool) -> None:
        """Packets of 8x4 pixel blocks in lean frames on the plain MFMA kernels (include/nwe.h); on by default, or what
        NWE_PACKET_BLOCKS set when the renderer was created.  No output depends on it."""
        self._check(self._lib.nwe_debug_set_packet_blocks(self._ctx, 1 if on else 0), "nwe_debug_set_packet_blocks")

    def debug_last_packet_blocks(self) -> int:
        """1 / 0: the call most recently planned (rendered, or asked about with nwe_debug_plan) was / was not blocked."""
        return int(self._lib.nwe_debug_last_packet_blocks(self._ctx))

    def debug_get_work_queue_tail(self) -> bool:
        """Whether this renderer may take the tail path: fixed when it was created (NWE_WORK_QUEUE_TAIL=0 in the environment then)."""
        return bool(self._lib.nwe_debug_get_work_queue_tail(self._ctx))

    def set_white_background(self, on: bool) -> None:
        """rendering.white_background (model_utils.py:97-98): rgb += 1 - acc on every rgb output."""
        self._check(self._lib.nwe_set_white_background(self._ctx, 1 if on else 0), "nwe_set_white_background")

    def set_early_termination(self, min_transmittance: float) -> None:
        """Opt-in early ray termination (include/nwe.h): in the pass that produces the outputs a sample whose transmittance is
        below ``min_transmittance`` weighs nothing, and a workgroup whose rays are all below stops evaluating.  0 = off (the
        default); |d rgb|, |d acc| < eps and |d depth| < eps * far by construction.  ``render`` honours it for rgb / depth / acc;
        every other call raises NotImplementedError while it is on."""
        self._check(self._lib.nwe_set_early_termination(self._ctx, float(min_transmittance)), "nwe_set_early_termination")

    @property
    def early_termination(self) -> float:
        return float(self._lib.nwe_get_early_termination(self._ctx))

    def set_shared_coarse(self, k: int) -> None:
        """Opt-in coarse pass shared by k x k pixel blocks (include/nwe.h): one ray per block of the whole image runs the coarse
        pass and the block's pixels draw their importance samples from its weights; everything behind is the pixel's own.
        1 = off (the default), 1..16.  An approximation.  ``render`` honours it for rgb / depth / acc when
        n_importance > 0; every other call raises NotImplementedError while it is on, and so does every call while early
        termination is on as well."""
        self._check(self._lib.nwe_set_shared_coarse(self._ctx, int(k)), "nwe_set_shared_coarse")

    @property
    def shared_coarse(self) -> int:
        return int(self._lib.nwe_get_shared_coarse(self._ctx))

    def set_separate_passes(self, on: bool) -> None:
        """Opt-in separate passes (include/nwe.h): under the MFMA precisions a call with n_importance > 0 is a coarse launch
        with the coarse network's kernels and a fine launch with the fine network's, so the two networks may differ in depth,
        width and skip.  Exact: with one shape every output is bit-identical to the fused call.  Off by default; every call
        raises NotImplementedError while early termination is on as well."""
        self._check(self._lib.nwe_set_separate_passes(self._ctx, 1 if on else 0), "nwe_set_separate_passes")

    @property
    def separate_passes(self) -> bool:
        return int(self._lib.nwe_get_separate_passes(self._ctx)) == 1

    # -- occupancy grid ---------------------------------------------------------------------------
    @staticmethod
    def _occupancy_box(lo, hi, resolution):
        res3 = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(r) for r in resolution)
        if len(res3) != 3 or len(lo) != 3 or len(hi) != 3:
            raise ValueError("occupancy needs lo, hi of three coordinates and a resolution of one or three ints")
        return (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi]), (C.c_int * 3)(*res3), res3

    @staticmethod
    def pack_occupancy(bits) -> np.ndarray:
        """uint32 words of a bool [rx, ry, rz] array (numpy or torch): bit (ix * ry + iy) * rz + iz in word >> 5 at bit & 31."""
        if isinstance(bits, torch.Tensor):
            bits = bits.detach().cpu().numpy()
        flat = np.ascontiguousarray(bits).astype(bool).reshape(-1)
        padded = np.zeros((flat.size + 31) // 32 * 32, dtype=np.uint8)
        padded[:flat.size] = flat
        shifted = padded.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :]
        return np.ascontiguousarray(np.bitwise_or.reduce(shifted, axis=1), dtype=np.uint32)

    @staticmethod
    def unpack_occupancy(words: np.ndarray, resolution) -> np.ndarray:
        """The bool [rx, ry, rz] array of packed words (pack_occupancy's inverse)."""
        rx, ry, rz = (int(r) for r in resolution)
        w = np.ascontiguousarray(words, dtype=np.uint32)
        flat = ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)
        return flat[:rx * ry * rz].reshape(rx, ry, rz)

    def set_occupancy(self, bits, lo: Sequence[float], hi: Sequence[float], resolution) -> None:
        """Opt-in occupancy grid (include/nwe.h): the box lo..hi in world coordinates cut into resolution = (rx, ry, rz) cells,
        ``bits`` a bool [rx, ry, rz] array (numpy or torch; True = occupied) or the packed uint32 words (pack_occupancy).  A
        sample in a cell marked empty counts as raw = 0 in both passes and a workgroup whose rays are all in empty cells at
        an iteration does not evaluate it; outside the box everything is evaluated.  ``render`` honours it for rgb / depth /
        acc; every other call raises NotImplementedError while a grid is set, and so does every call while early
        termination, a shared coarse pass or separate passes are on as well.  ``set_network`` clears the grid."""
        lo3, hi3, res3, res = self._occupancy_box(lo, hi, resolution)
        n_words = (res[0] * res[1] * res[2] + 31) // 32 if min(res) > 0 else 0
        if isinstance(bits, torch.Tensor) and bits.dtype != torch.bool:
            bits = bits.detach().cpu().numpy()
        arr = bits if isinstance(bits, torch.Tensor) else np.asarray(bits)
        if arr.dtype in (np.uint32, np.int32) and arr.ndim == 1:
            words = np.ascontiguousarray(arr).view(np.uint32)
        else:
            if tuple(arr.shape) != res:
                raise ValueError(f"occupancy bits must be a bool array of shape {res} or packed uint32 words, got {tuple(arr.shape)}")
            words = self.pack_occupancy(arr)
        if min(res) > 0 and words.size != n_words:
            raise ValueError(f"occupancy needs {n_words} words for resolution {res}, got {words.size}")
        self._check(self._lib.nwe_set_occupancy(self._ctx, lo3, hi3, res3, words.ctypes.data if words.size else None, 0), "nwe_set_occupancy")

    def build_occupancy(self, lo: Sequence[float], hi: Sequence[float], resolution, probes: int = 2, threshold: float = 0.0,
                        dilate: int = 1, precision: str = "f16x3") -> None:
        """Builds the grid from the networks that are set (nwe_build_occupancy): a cell is occupied if sigma_raw of any set
        network at any of its probes^3 lattice points is > threshold or not finite, then ``dilate`` steps of 3 x 3 x 3
        dilation.  An approximation unless the networks have no density in the cells it marks empty."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        lo3, hi3, res3, _ = self._occupancy_box(lo, hi, resolution)
        stream = None
        if self.device is not None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.nwe_build_occupancy(self._ctx, lo3, hi3, res3, int(probes), float(threshold), int(dilate),
                                                  _lib.PRECISIONS[precision], stream), "nwe_build_occupancy")

    def clear_occupancy(self) -> None:
        self._check(self._lib.nwe_clear_occupancy(self._ctx), "nwe_clear_occupancy")

    @property
    def occupancy(self) -> Optional[Dict[str, object]]:
        """None, or the grid: "lo", "hi", "resolution", "inv" (the fp32 factors the kernels multiply by), "occupied_cells" and
        "occupied" (their share of the cells)."""
        lo, hi, res, inv, occ = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_int * 3)(), (C.c_float * 3)(), C.c_int64(0)
        if self._lib.nwe_get_occupancy(self._ctx, lo, hi, res, inv, C.byref(occ)) != _lib.NWE_OK:
            return None
        cells = res[0] * res[1] * res[2]
        return {"lo": tuple(lo), "hi": tuple(hi), "resolution": tuple(res), "inv": np.array(list(inv), dtype=np.float32),
                "occupied_cells": int(occ.value), "occupied": occ.value / cells}

    def occupancy_bits(self) -> Optional[np.ndarray]:
        """The grid as a bool [rx, ry, rz] array, None without one."""
        g = self.occupancy
        if g is None:
            return None
        rx, ry, rz = g["resolution"]
        words = np.empty((rx * ry * rz + 31) // 32, dtype=np.uint32)
        self._check(self._lib.nwe_occupancy_copy(self._ctx, words.ctypes.data, words.size), "nwe_occupancy_copy")
        return self.unpack_occupancy(words, (rx, ry, rz))

    # -- baked coarse pass ------------------------------------------------------------------------
    def set_coarse_grid(self, sigma, lo: Sequence[float], hi: Sequence[float], resolution=None) -> None:
        """Opt-in baked coarse pass (include/nwe.h): ``sigma`` holds sigma_raw of the coarse network at the cell centres of the
        box lo..hi, a float32 [rx, ry, rz] array (numpy, or a torch tensor on any device; what handler.density_grid returns) or
        a flat array with ``resolution`` given.  While a grid is set, ``render`` of rgb / depth / acc with n_importance > 0 takes
        its coarse weights from the trilinearly interpolated grid instead of running the coarse network; every other call
        raises NotImplementedError, and so does every call while early termination, a shared coarse pass, separate passes or
        an occupancy grid are on as well.  ``set_network`` of the coarse network clears the grid."""
        if resolution is None:
            resolution = tuple(sigma.shape)
        lo3, hi3, res3, res = self._occupancy_box(lo, hi, resolution)
        on_device = isinstance(sigma, torch.Tensor) and self.device is not None and sigma.device == self.device
        if on_device:
            values = sigma.detach().to(torch.float32).contiguous()
            n, ptr = values.numel(), values.data_ptr()
        else:
            if isinstance(sigma, torch.Tensor):
                sigma = sigma.detach().cpu().numpy()
            values = np.ascontiguousarray(np.asarray(sigma, dtype=np.float32))
            n, ptr = values.size, values.ctypes.data
        if min(res) > 0 and n != res[0] * res[1] * res[2]:
            raise ValueError(f"the coarse grid needs {res[0] * res[1] * res[2]} values for resolution {res}, got {n}")
        if on_device:
            torch.cuda.current_stream(self.device).synchronize()   # the copy inside is not ordered with torch's stream
        self._check(self._lib.nwe_set_coarse_grid(self._ctx, lo3, hi3, res3, ptr if n else None, 1 if on_device else 0), "nwe_set_coarse_grid")

    def bake_coarse_grid(self, lo: Sequence[float], hi: Sequence[float], resolution, precision: str = "f16x3") -> None:
        """Bakes the grid from the coarse network that is set (nwe_bake_coarse_grid): its sigma_raw at the cell centres."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        lo3, hi3, res3, _ = self._occupancy_box(lo, hi, resolution)
        stream = None
        if self.device is not None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.nwe_bake_coarse_grid(self._ctx, lo3, hi3, res3, _lib.PRECISIONS[precision], stream), "nwe_bake_coarse_grid")

    def clear_coarse_grid(self) -> None:
        self._check(self._lib.nwe_clear_coarse_grid(self._ctx), "nwe_clear_coarse_grid")

    @property
    def coarse_grid(self) -> Optional[Dict[str, object]]:
        """None, or the grid: "lo", "hi", "resolution" and "inv" (the fp32 factors the kernel multiplies by)."""
        lo, hi, res, inv = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_int * 3)(), (C.c_float * 3)()
        if self._lib.nwe_get_coarse_grid(self._ctx, lo, hi, res, inv) != _lib.NWE_OK:
            return None
        return {"lo": tuple(lo), "hi": tuple(hi), "resolution": tuple(res), "inv": np.array(list(inv), dtype=np.float32)}

    def coarse_grid_values(self) -> Optional[np.ndarray]:
        """The grid's values as a float32 [rx, ry, rz] array on the host, None without one."""
        g = self.coarse_grid
        if g is None:
            return None
        rx, ry, rz = g["resolution"]
        values = np.empty(rx * ry * rz, dtype=np.float32)
        self._check(self._lib.nwe_coarse_grid_copy(self._ctx, values.ctypes.data, values.size), "nwe_coarse_grid_copy")
        return values.reshape(rx, ry, rz)

    def coarse_grid_weights(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                            rows: Optional[Tuple[int, int]] = None, outputs: Sequence[str] = ("sigma", "weights")) -> Dict[str, torch.Tensor]:
        """Test hook (nwe_coarse_grid_weights): the producer of the baked coarse pass alone, for the rays of ``render`` with the
        same arguments: "sigma" [R, n_samples] = the grid's sigma_raw per coarse sample, "weights" [R, n_samples] = the coarse
        weights it composites from them."""
        outputs = tuple(outputs)
        if set(outputs) - {"sigma", "weights"}:
            raise ValueError(f"outputs must be a choice of 'sigma' and 'weights', got {outputs!r}")
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        if self.device is None:   # a host-only context: the ABI's own refusal
            self._check(self._lib.nwe_coarse_grid_weights(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far,
                                                          r0, r1, None, None, None), "nwe_coarse_grid_weights")
        n_rays = poses.shape[0] * max(r1 - r0, 0) * W
        with torch.cuda.device(self.device):
            res = {k: torch.empty((n_rays, self.n_samples), dtype=torch.float32, device=self.device) for k in outputs}
            ptr = lambda k: res[k].data_ptr() if k in res else None
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.nwe_coarse_grid_weights(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1,
                                                   ptr("sigma"), ptr("weights"), stream)
        self._check(rc, "nwe_coarse_grid_weights")
        return res

    # -- radiance grid ----------------------------------------------------------------------------
    def set_radiance_grid(self, raw, lo: Sequence[float], hi: Sequence[float], resolution=None) -> None:
        """Opt-in radiance grid (include/nwe.h): ``raw`` holds the network's raw output (rgb_raw[3], sigma_raw) at the cell centres
        of the box lo..hi, a float32 [rx, ry, rz, 4] array (numpy, or a torch tensor on any device; what handler.run_network returns
        at handler.grid_centres) or a flat array with ``resolution`` given.  ``render_grid`` renders frames from it without a
        network; no other call reads it.  ``set_network`` of either network clears the grid."""
        if resolution is None:
            if len(raw.shape) != 4 or raw.shape[3] != 4:
                raise ValueError(f"the radiance grid needs an [rx, ry, rz, 4] array or a resolution, got {tuple(raw.shape)}")
            resolution = tuple(raw.shape[:3])
        lo3, hi3, res3, res = self._occupancy_box(lo, hi, resolution)
        on_device = isinstance(raw, torch.Tensor) and self.device is not None and raw.device == self.device
        if on_device:
            values = raw.detach().to(torch.float32).contiguous()
            n, ptr = values.numel(), values.data_ptr()
        else:
            if isinstance(raw, torch.Tensor):
                raw = raw.detach().cpu().numpy()
            values = np.ascontiguousarray(np.asarray(raw, dtype=np.float32))
            n, ptr = values.size, values.ctypes.data
        if min(res) > 0 and n != 4 * res[0] * res[1] * res[2]:
            raise ValueError(f"the radiance grid needs {4 * res[0] * res[1] * res[2]} values for resolution {res}, got {n}")
        if on_device:
            torch.cuda.current_stream(self.device).synchronize()   # the copy inside is not ordered with torch's stream
        self._check(self._lib.nwe_set_radiance_grid(self._ctx, lo3, hi3, res3, ptr if n else None, 1 if on_device else 0), "nwe_set_radiance_grid")

    def bake_radiance_grid(self, lo: Sequence[float], hi: Sequence[float], resolution, which: int = _lib.NET_FINE,
                           view_dir: Optional[Sequence[float]] = None, precision: str = "f16x3") -> None:
        """Bakes the grid from network ``which`` (nwe_bake_radiance_grid): its raw output at the cell centres, every cell with the one
        direction ``view_dir`` (three floats, used as given; None for networks without view directions)."""
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        lo3, hi3, res3, _ = self._occupancy_box(lo, hi, resolution)
        dir3 = None
        if view_dir is not None:
            if len(view_dir) != 3:
                raise ValueError("view_dir must hold three coordinates")
            dir3 = (C.c_float * 3)(*[float(v) for v in view_dir])
        stream = None
        if self.device is not None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.nwe_bake_radiance_grid(self._ctx, lo3, hi3, res3, int(which), dir3, _lib.PRECISIONS[precision], stream),
                    "nwe_bake_radiance_grid")

    def clear_radiance_grid(self) -> None:
        self._check(self._lib.nwe_clear_radiance_grid(self._ctx), "nwe_clear_radiance_grid")

    @property
    def radiance_grid(self) -> Optional[Dict[str, object]]:
        """None, or the grid: "lo", "hi", "resolution" and "inv" (the fp32 factors the kernel multiplies by)."""
        lo, hi, res, inv = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_int * 3)(), (C.c_float * 3)()
        if self._lib.nwe_get_radiance_grid(self._ctx, lo, hi, res, inv) != _lib.NWE_OK:
            return None
        return {"lo": tuple(lo), "hi": tuple(hi), "resolution": tuple(res), "inv": np.array(list(inv), dtype=np.float32)}

    def radiance_grid_values(self) -> Optional[np.ndarray]:
        """The grid's rows as a float32 [rx, ry, rz, 4] array on the host, None without one."""
        g = self.radiance_grid
        if g is None:
            return None
        rx, ry, rz = g["resolution"]
        values = np.empty(rx * ry * rz * 4, dtype=np.float32)
        self._check(self._lib.nwe_radiance_grid_copy(self._ctx, values.ctypes.data, values.size), "nwe_radiance_grid_copy")
        return values.reshape(rx, ry, rz, 4)

    def render_grid(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                    rows: Optional[Tuple[int, int]] = None, outputs: Sequence[str] = ("rgb", "depth", "acc")) -> Dict[str, torch.Tensor]:
        """A frame from the radiance grid (nwe_render_grid): rows [rows[0], rows[1]) of each pose, both passes of the pipeline with
        the trilinear lookup in run_network's place; no network is needed or read.  ``outputs``: a choice of "rgb", "depth", "acc"
        and the diagnostics "weights_coarse" [R, n_samples], "z_fine" [R, S] and "raw_fine" [R, S, 4] (S = n_samples +
        n_importance, the output pass); "flags" is always returned."""
        outputs = tuple(outputs)
        unknown = set(outputs) - set(_lib.GRID_OUTPUT_FIELDS[:-1])
        if unknown:
            raise ValueError(f"unknown grid outputs {sorted(unknown)}; have {_lib.GRID_OUTPUT_FIELDS[:-1]}")
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        o = _lib.GridOutputs()
        if self.device is None:   # a host-only context: the ABI's own refusals, nothing allocated
            for name in outputs:
                setattr(o, name, 1)   # never written: every path of a host-only context refuses
            self._check(self._lib.nwe_render_grid(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1,
                                                  C.byref(o), None), "nwe_render_grid")
            raise RuntimeError("nwe_render_grid: a host-only context rendered")   # not reached
        n_rays = poses.shape[0] * max(r1 - r0, 0) * W
        S = self.n_samples + self.n_importance
        shapes = {"rgb": (n_rays, 3), "depth": (n_rays,), "acc": (n_rays,), "weights_coarse": (n_rays, self.n_samples),
                  "z_fine": (n_rays, S), "raw_fine": (n_rays, S, 4)}
        with torch.cuda.device(self.device):
            # at least one element each: an empty tensor has no pointer, and a call of zero rays still says what it asks for
            bufs = {name: torch.empty(max(int(np.prod(shapes[name])), 1), dtype=torch.float32, device=self.device) for name in outputs}
            res = {name: bufs[name][:int(np.prod(shapes[name]))].view(shapes[name]) for name in outputs}
            res["flags"] = torch.zeros(1, dtype=torch.int32, device=self.device)
            for name in _lib.GRID_OUTPUT_FIELDS:
                setattr(o, name, (bufs[name] if name in bufs else res[name]).data_ptr() if name in res else None)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self._lib.nwe_render_grid(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1,
                                           C.byref(o), stream)
        self._check(rc, "nwe_render_grid")
        return res

    def last_grid_ms(self) -> Optional[float]:
        """Device time of the last ``render_grid`` launch in ms (blocks until it has finished), None if there was none."""
        ms = float(self._lib.nwe_last_grid_ms(self._ctx))
        return ms if ms >= 0 else None

    # -- sparse frame -----------------------------------------------------------------------------
    def render_sparse(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                      rows: Optional[Tuple[int, int]] = None, which: int = _lib.NET_FINE, precision: str = "f16x3",
                      min_weight: float = 1e-3, dilate: int = 1,
                      outputs: Sequence[str] = ("rgb", "depth", "acc"), asynchronous: bool = False) -> Dict[str, torch.Tensor]:
        """A sparse frame (nwe_render_sparse): the radiance grid's frame as a proposal, network ``which`` at the samples of the
        output pass whose proposed weight is above ``min_weight`` (and ``dilate`` neighbours on either side), the grid's rows at
        the others.  Synchronous, unless ``asynchronous``: then the call is queued on the current stream and returns
        (nwe_render_sparse_async), with the same bits; the tensors are valid for work queued on that stream behind it.  ``outputs``: a choice of "rgb", "depth", "acc" and the diagnostics "weights_coarse"
        [R, n_samples], "z_fine" [R, S], "weights_grid" [R, S], "selected" [R, S] (uint8) and "raw_fine" [R, S, 4] (S = n_samples +
        n_importance, the output pass); "flags" is always returned."""
        outputs = tuple(outputs)
        unknown = set(outputs) - set(_lib.SPARSE_OUTPUT_FIELDS[:-1])
        if unknown:
            raise ValueError(f"unknown sparse outputs {sorted(unknown)}; have {_lib.SPARSE_OUTPUT_FIELDS[:-1]}")
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        o = _lib.SparseOutputs()
        tail = (r0, r1, int(which), _lib.PRECISIONS[precision], float(min_weight), int(dilate))
        entry = "nwe_render_sparse_async" if asynchronous else "nwe_render_sparse"
        call = getattr(self._lib, entry)
        if self.device is None:   # a host-only context: the ABI's own refusals, nothing allocated
            for name in outputs:
                setattr(o, name, 1)   # never written: every path of a host-only context refuses
            self._check(call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, *tail, C.byref(o), None), entry)
            raise RuntimeError(f"{entry}: a host-only context rendered")   # not reached
        n_rays = poses.shape[0] * max(r1 - r0, 0) * W
        S = self.n_samples + self.n_importance
        shapes = {"rgb": (n_rays, 3), "depth": (n_rays,), "acc": (n_rays,), "weights_coarse": (n_rays, self.n_samples),
                  "z_fine": (n_rays, S), "weights_grid": (n_rays, S), "selected": (n_rays, S), "raw_fine": (n_rays, S, 4)}
        with torch.cuda.device(self.device):
            # at least one element each: an empty tensor has no pointer, and a call of zero rays still says what it asks for
            bufs = {name: torch.empty(max(int(np.prod(shapes[name])), 1), dtype=torch.uint8 if name == "selected" else torch.float32,
                                      device=self.device) for name in outputs}
            res = {name: bufs[name][:int(np.prod(shapes[name]))].view(shapes[name]) for name in outputs}
            res["flags"] = torch.zeros(1, dtype=torch.int32, device=self.device)
            for name in _lib.SPARSE_OUTPUT_FIELDS:
                setattr(o, name, (bufs[name] if name in bufs else res[name]).data_ptr() if name in res else None)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, *tail, C.byref(o), stream)
        self._check(rc, entry)
        return res

    def last_sparse_ms(self) -> Optional[float]:
        """Device span of the last ``render_sparse`` call in ms (blocks until it has finished), None if there was none."""
        ms = float(self._lib.nwe_last_sparse_ms(self._ctx))
        return ms if ms >= 0 else None

    def last_sparse_samples(self) -> Optional[Tuple[int, int]]:
        """(selected, total) samples of the last ``render_sparse`` call (blocks until an asynchronous one has finished), None if
        there was none."""
        out = (C.c_int64 * 2)()
        if self._lib.nwe_last_sparse_samples(self._ctx, out) != _lib.NWE_OK:
            return None
        return int(out[0]), int(out[1])

    def debug_last_sparse_host_waits(self) -> Optional[int]:
        """Test hook (nwe_debug_last_sparse_host_waits): how often the last ``render_sparse`` call made the host wait for the
        device - its chunks + 1 when synchronous, 0 for a warmed asynchronous call; None if there was none."""
        n = int(self._lib.nwe_debug_last_sparse_host_waits(self._ctx))
        return n if n >= 0 else None

    def debug_set_sparse_chunk(self, rays: int) -> None:
        """Test hook (nwe_debug_set_sparse_chunk): the rays of a chunk of ``render_sparse``; 0 restores the default."""
        if self._lib.nwe_debug_set_sparse_chunk(self._ctx, int(rays)) != _lib.NWE_OK:
            raise ValueError("the sparse chunk must be 0 (the default) or a number of rays of at least 1")

    # -- adaptive frame ---------------------------------------------------------------------------
    def render_adaptive(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                        rows: Optional[Tuple[int, int]] = None, precision: str = "f16x3", k: int = 2, tol_rgb: float = 2 / 255,
                        tol_depth: float = 0.05, outputs: Sequence[str] = ("rgb",), levels: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """An adaptive frame (nwe_render_adaptive): the lattice of every ``k``-th pixel and the pixels of the lattice cells whose
        corners differ by more than ``tol_rgb`` (r, g, b, acc) or ``tol_depth`` are rendered by the networks, bit for bit as
        ``render`` renders them; the pixels of the other cells are interpolated bilinearly.  Synchronous.  ``outputs``: a choice
        of "rgb", "depth", "acc" (at least one) and the diagnostic "kind" [R] (uint8: 0 lattice, 1 rendered, 2 interpolated);
        "flags" is always returned.
        ``levels``: None is that call.  An integer 1 .. 4 takes the multi-level frame (nwe_render_adaptive_levels): ``k`` is then
        the finest of ``levels`` nested lattices, the coarsest has the spacing k 2^(levels - 1) <= 64, and only the cells whose
        corners disagree are subdivided; ``outputs`` may then hold the diagnostic "level" [R] (uint8: the pass that rendered a
        pixel, or the level of the cell it was interpolated in)."""
        outputs = tuple(outputs)
        fields = _lib.ADAPTIVE_OUTPUT_FIELDS if levels is None else _lib.ADAPTIVE_LEVELS_OUTPUT_FIELDS
        have = tuple(name for name in fields if name != "flags")
        unknown = set(outputs) - set(have)
        if unknown:
            raise ValueError(f"unknown adaptive outputs {sorted(unknown)}; have {have}")
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        if levels is None:
            o, who, call = _lib.AdaptiveOutputs(), "nwe_render_adaptive", self._lib.nwe_render_adaptive
            tail = (r0, r1, _lib.PRECISIONS[precision], int(k), float(tol_rgb), float(tol_depth))
        else:
            o, who, call = _lib.AdaptiveLevelsOutputs(), "nwe_render_adaptive_levels", self._lib.nwe_render_adaptive_levels
            tail = (r0, r1, _lib.PRECISIONS[precision], int(k), int(levels), float(tol_rgb), float(tol_depth))
        if self.device is None:   # a host-only context: the ABI's own refusals, nothing allocated
            for name in outputs:
                setattr(o, name, 1)   # never written: every path of a host-only context refuses
            self._check(call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, *tail, C.byref(o), None), who)
            raise RuntimeError(f"{who}: a host-only context rendered")   # not reached
        n_rays = poses.shape[0] * max(r1 - r0, 0) * W
        shapes = {"rgb": (n_rays, 3), "depth": (n_rays,), "acc": (n_rays,), "kind": (n_rays,), "level": (n_rays,)}
        with torch.cuda.device(self.device):
            # at least one element each: an empty tensor has no pointer, and a call of zero rays still says what it asks for
            bufs = {name: torch.empty(max(int(np.prod(shapes[name])), 1), dtype=torch.uint8 if name in ("kind", "level") else torch.float32,
                                      device=self.device) for name in outputs}
            res = {name: bufs[name][:int(np.prod(shapes[name]))].view(shapes[name]) for name in outputs}
            res["flags"] = torch.zeros(1, dtype=torch.int32, device=self.device)
            for name in fields:
                setattr(o, name, (bufs[name] if name in bufs else res[name]).data_ptr() if name in res else None)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, *tail, C.byref(o), stream)
        self._check(rc, who)
        return res

    def last_adaptive_levels(self) -> Optional[Dict[str, object]]:
        """{"pixels", "lattice", "levels", "render_launches", "rendered", "interpolated", "ms"} of the last multi-level
        ``render_adaptive`` call that ran: ``rendered[i]`` the pixels of render pass i + 1, ``interpolated[l]`` the pixels
        interpolated in a cell of level l (lists of ``levels`` entries); None if there was none."""
        cap = 4 + 2 * _lib.ADAPTIVE_MAX_LEVELS
        out, ms = (C.c_int64 * cap)(), C.c_float(-1.0)
        if self._lib.nwe_last_adaptive_levels(self._ctx, out, cap, C.byref(ms)) != _lib.NWE_OK:
            return None
        n = int(out[2])
        return {"pixels": int(out[0]), "lattice": int(out[1]), "levels": n, "render_launches": int(out[3]),
                "rendered": [int(v) for v in out[4:4 + n]], "interpolated": [int(v) for v in out[4 + n:4 + 2 * n]], "ms": float(ms.value)}

    @staticmethod
    def adaptive_levels_lattice(first: int, last_excl: int, k: int, levels: int, level: int) -> np.ndarray:
        """The lattice rows (or columns) of [first, last_excl) at level ``level`` of ``levels`` over the finest spacing ``k``
        (nwe_debug_adaptive_levels_lattice; needs no context)."""
        lib = _lib.load()
        cap = max(int(last_excl) - int(first), 1)
        out = (C.c_int32 * cap)()
        n = lib.nwe_debug_adaptive_levels_lattice(int(first), int(last_excl), int(k), int(levels), int(level), out, cap)
        if n < 0:
            raise ValueError("adaptive lattice: an empty range, k outside 1..64, levels outside 1..4, k * 2^(levels - 1) > 64 or a level outside 0..levels - 1")
        return np.array(out[:n], dtype=np.int32)

    def last_adaptive(self) -> Optional[Dict[str, object]]:
        """{"pixels", "lattice", "rendered", "interpolated", "ms"} of the last ``render_adaptive`` call that ran (ms: its device
        span, the read-back between its two render launches included), None if there was none."""
        out, ms = (C.c_int64 * 4)(), C.c_float(-1.0)
        if self._lib.nwe_last_adaptive(self._ctx, out, C.byref(ms)) != _lib.NWE_OK:
            return None
        return {"pixels": int(out[0]), "lattice": int(out[1]), "rendered": int(out[2]), "interpolated": int(out[3]), "ms": float(ms.value)}

    @staticmethod
    def adaptive_lattice(first: int, last_excl: int, k: int) -> np.ndarray:
        """The lattice rows (or columns) of [first, last_excl) at ``k`` (nwe_debug_adaptive_lattice; needs no context)."""
        lib = _lib.load()
        cap = max(int(last_excl) - int(first), 1)
        out = (C.c_int32 * cap)()
        n = lib.nwe_debug_adaptive_lattice(int(first), int(last_excl), int(k), out, cap)
        if n < 0:
            raise ValueError("adaptive lattice: an empty range, or k outside 1..64")
        return np.array(out[:n], dtype=np.int32)

    def set_adaptive_pixel_lists(self, on: bool) -> None:
        """Opt-in (nwe_set_adaptive_pixel_lists): ``render_adaptive`` hands its pixel lists to the list kernels of
        ``render_pixels`` where they can serve the call, in place of ray tables.  The same bits; off by default."""
        self._check(self._lib.nwe_set_adaptive_pixel_lists(self._ctx, 1 if on else 0), "nwe_set_adaptive_pixel_lists")

    @property
    def adaptive_pixel_lists(self) -> bool:
        return int(self._lib.nwe_get_adaptive_pixel_lists(self._ctx)) == 1

    # -- pixel list -------------------------------------------------------------------------------
    def render_pixels(self, c2w, H: int, W: int, pixels: torch.Tensor, *, fx: float, fy: float, cx: float, cy: float, near: float,
                      far: float, rows: Optional[Tuple[int, int]] = None, precision: str = "f16x3",
                      outputs: Sequence[str] = ("rgb",)) -> Dict[str, torch.Tensor]:
        """The listed pixels of a pinhole view (nwe_render_pixels): ``pixels`` is an int32 tensor [n] on this renderer's device
        of ray indices of ``render`` with the same camera arguments, (p * rows + (h - rows[0])) * W + w, in any order, duplicates
        allowed; a value outside the frame renders the clamped pixel.  Row i of every output holds, bit for bit, what ``render``
        writes to row ``pixels[i]``.  Asynchronous on the current stream.  ``outputs``: a choice of "rgb", "depth", "acc" (at
        least one); "flags" (the rgb / depth / acc bits only) is always returned."""
        outputs = tuple(outputs)
        unknown = set(outputs) - set(_lib.PIXEL_OUTPUT_FIELDS[:-1])
        if unknown:
            raise ValueError(f"unknown pixel outputs {sorted(unknown)}; have {_lib.PIXEL_OUTPUT_FIELDS[:-1]}")
        if not isinstance(pixels, torch.Tensor) or pixels.dtype != torch.int32 or pixels.dim() != 1:
            raise ValueError("pixels must be an int32 tensor [n]")
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        r0, r1 = rows if rows is not None else (0, H)
        o = _lib.PixelOutputs()
        n = int(pixels.shape[0])
        call = self._lib.nwe_render_pixels
        if self.device is None:   # a host-only context: the ABI's own refusals, nothing allocated
            for name in outputs:
                setattr(o, name, 1)   # never written: every path of a host-only context refuses, or launches nothing
            self._check(call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1, 1 if n else None, n,
                             _lib.PRECISIONS[precision], C.byref(o), None), "nwe_render_pixels")
            return {}
        if pixels.device != self.device:
            raise ValueError(f"pixels must be on {self.device}")
        pixels = pixels.contiguous()
        shapes = {"rgb": (n, 3), "depth": (n,), "acc": (n,)}
        with torch.cuda.device(self.device):
            # at least one element each: an empty tensor has no pointer, and a call of no pixels still says what it asks for
            bufs = {name: torch.empty(max(int(np.prod(shapes[name])), 1), dtype=torch.float32, device=self.device) for name in outputs}
            res = {name: bufs[name][:int(np.prod(shapes[name]))].view(shapes[name]) for name in outputs}
            res["flags"] = torch.zeros(1, dtype=torch.int32, device=self.device)
            for name in _lib.PIXEL_OUTPUT_FIELDS:
                setattr(o, name, (bufs[name] if name in bufs else res[name]).data_ptr() if name in res else None)
            stream = torch.cuda.current_stream(self.device)
            rc = call(self._ctx, poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near, far, r0, r1, pixels.data_ptr() if n else None, n,
                      _lib.PRECISIONS[precision], C.byref(o), stream.cuda_stream)
            pixels.record_stream(stream)   # the launch reads the list after this call has returned
        self._check(rc, "nwe_render_pixels")
        return res

    def last_pixels(self) -> Optional[Dict[str, object]]:
        """{"n", "path"} of the last pixel-list launch that was recorded - ``render_pixels``, or a render launch of
        ``render_adaptive`` under ``set_adaptive_pixel_lists`` - path "list" (the list kernels) or "rays" (a ray table); None if
        there was none."""
        n, path = C.c_int64(), C.c_int()
        if self._lib.nwe_last_pixels(self._ctx, C.byref(n), C.byref(path)) != _lib.NWE_OK:
            return None
        return {"n": int(n.value), "path": "list" if path.value == 1 else "rays"}

    def pixels_path(self, precision: str = "f16x3") -> str:
        """The path ``render_pixels`` would take under ``precision`` as the context stands (nwe_debug_pixels_path; a host-only
        context serves it): "list" or "rays"."""
        return "list" if int(self._lib.nwe_debug_pixels_path(self._ctx, _lib.PRECISIONS[precision])) == 1 else "rays"

    def last_coarse_launch(self) -> Optional[Tuple[float, int]]:
        """(ms, rays) of the coarse (producer) launch of the last render, None if it had none (k = 1 without separate passes,
        n_importance == 0)."""
        ms, rays = C.c_float(), C.c_int64()
        self._check(self._lib.nwe_last_coarse_launch(self._ctx, C.byref(ms), C.byref(rays)), "nwe_last_coarse_launch")
        return (float(ms.value), int(rays.value)) if ms.value >= 0 else None

    def last_ray_evaluations(self) -> Tuple[int, int]:
        """(executed, full) ray evaluations of the last render launch: equal unless early termination skipped some or a
        shared coarse pass left some out."""
        out = (C.c_int64 * 2)()
        self._check(self._lib.nwe_last_ray_evaluations(self._ctx, out), "nwe_last_ray_evaluations")
        return int(out[0]), int(out[1])

    # -- point query ------------------------------------------------------------------------------
    @staticmethod
    def query_layout(points_shape: Sequence[int], dirs_shape: Optional[Sequence[int]]) -> Tuple[int, int]:
        """(n_points, points_per_dir) of a query, or ValueError: ``points`` is [..., 3]; ``dirs`` is None, or one row per
        point (the shape of ``points``), or [N,3] against ``points`` of shape [N,S,3] (run_network's layout,
        model_utils.py:23-25: points_per_dir = S)."""
        points_shape = tuple(int(d) for d in points_shape)
        if len(points_shape) < 1 or points_shape[-1] != 3:
            raise ValueError(f"points must be [..., 3], got {points_shape}")
        n = int(np.prod(points_shape[:-1], dtype=np.int64))
        if dirs_shape is None:
            return n, 1
        dirs_shape = tuple(int(d) for d in dirs_shape)
        if dirs_shape == points_shape:
            return n, 1
        if len(points_shape) == 3 and dirs_shape == (points_shape[0], 3):
            return n, max(points_shape[1], 1)
        raise ValueError(f"dirs must be one row per point {points_shape} or [N,3] against points [N,S,3], got {dirs_shape} against {points_shape}")

    def query_points(self, points: torch.Tensor, dirs: Optional[torch.Tensor] = None, *, which: int = _lib.NET_FINE,
                     precision: str = "f16x3", outputs: Sequence[str] = ("raw",)) -> Dict[str, torch.Tensor]:
        """Network ``which`` at arbitrary points (nwe_query_points; the reference's run_network, model_utils.py:13-30):
        ``points`` float32 [..., 3] world coordinates on this renderer's device, ``dirs`` float32 view directions, used as
        given (see query_layout; None for networks without view directions, and allowed when only sigma is asked for).
        ``outputs`` of "raw" ([..., 4] = rgb_raw, sigma_raw: no sigmoid, no ReLU) and "sigma" ([...] = sigma_raw); the
        result also holds "flags" (NWE_FLAG_RAW when a value written is NaN or inf).  Needs nothing but that network set."""
        n, ppd = self.query_layout(points.shape, None if dirs is None else dirs.shape)
        if points.dtype != torch.float32 or (dirs is not None and dirs.dtype != torch.float32):
            raise ValueError("points and dirs must be float32")
        outputs = tuple(outputs)
        if not outputs or set(outputs) - {"raw", "sigma"} or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs must be a non-empty choice of 'raw' and 'sigma', got {outputs!r}")
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        if which not in (_lib.NET_COARSE, _lib.NET_FINE):
            raise ValueError("which must be 0 (coarse) or 1 (fine)")
        o = _lib.PointOutputs()
        if self.device is None:   # a host-only context: the ABI's own refusal
            self._check(self._lib.nwe_query_points(self._ctx, which, None, n, None, ppd, _lib.PRECISIONS[precision], C.byref(o), None),
                        "nwe_query_points")
        points = points.to(self.device).contiguous()
        dirs = None if dirs is None else dirs.to(self.device).contiguous()
        lead = tuple(points.shape[:-1])
        with torch.cuda.device(self.device):
            res: Dict[str, torch.Tensor] = {"flags": torch.zeros(1, dtype=torch.int32, device=self.device)}
            # at least one row each, so that an empty query still hands the ABI the pointers that say what was asked for
            base = {"flags": res["flags"]}
            if "raw" in outputs:
                base["raw"] = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)
                res["raw"] = base["raw"][:n].reshape(lead + (4,))
            if "sigma" in outputs:
                base["sigma"] = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
                res["sigma"] = base["sigma"][:n].reshape(lead)
            for name in _lib.POINT_OUTPUT_FIELDS:
                setattr(o, name, base[name].data_ptr() if name in base else None)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if dirs is not None and dirs.numel() == 0:   # likewise: "directions were given"
                dirs = torch.zeros(3, dtype=torch.float32, device=self.device)
            rc = self._lib.nwe_query_points(self._ctx, which, points.data_ptr() if n else None, n, None if dirs is None else dirs.data_ptr(),
                                            ppd, _lib.PRECISIONS[precision], C.byref(o), stream)
        self._check(rc, "nwe_query_points")
        res["_keepalive_points"] = (points, dirs)
        return res

    def last_query_ms(self) -> float:
        """Time of the last query launch (events of its own: no render moves it, and it moves no render's); < 0 if none yet."""
        return float(self._lib.nwe_last_query_ms(self._ctx))

    def debug_set_query_steps(self, steps: int) -> None:
        """Test hook: the packets a query workgroup walks (1..256; 0 = automatic).  Results do not depend on it."""
        self._check(self._lib.nwe_debug_set_query_steps(self._ctx, int(steps)), "nwe_debug_set_query_steps")

    def to8b(self, rgb: torch.Tensor) -> torch.Tensor:
        rgb = rgb.contiguous()
        out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._check(self._lib.nwe_to8b(self._ctx, rgb.data_ptr(), out.data_ptr(), rgb.numel(), stream), "nwe_to8b")
        return out

    # -- introspection ----------------------------------------------------------------------------
    def last_kernel_ms(self) -> float:
        return float(self._lib.nwe_last_kernel_ms(self._ctx))

    def last_launch_parts(self):
        """[(ms, rays), ...] of the launches the last render took: one, or - under the hybrid plan - the packets launch over
        the full rounds of workgroups and the sample-split launch over the ragged rest."""
        ms, rays = (C.c_float * 2)(), (C.c_int64 * 2)()
        self._check(self._lib.nwe_last_launch_parts(self._ctx, ms, rays), "nwe_last_launch_parts")
        return [(float(ms[i]), int(rays[i])) for i in range(2) if ms[i] >= 0]

    def mfma_supported(self, which: int) -> bool:
        """True if network `which` has been packed for the MFMA kernel (its shape has an instantiation)."""
        return int(self._lib.nwe_packed_bytes(self._ctx, which)) > 0

    def flops_per_eval(self, which: int) -> int:
        return int(self._lib.nwe_flops_per_eval(self._ctx, which))

    def packed_stream(self, which: int) -> np.ndarray:
        n = int(self._lib.nwe_packed_bytes(self._ctx, which))
        buf = np.empty(n, dtype=np.uint8)
        if n:
            rc = self._lib.nwe_packed_copy(self._ctx, which, buf.ctypes.data, n)
            if rc != _lib.NWE_OK:
                raise RuntimeError("nwe_packed_copy failed")
        return buf

    def packed_bias(self, which: int) -> np.ndarray:
        n = int(self._lib.nwe_packed_bias_count(self._ctx, which))
        buf = np.empty(n, dtype=np.float32)
        if n and self._lib.nwe_packed_bias_copy(self._ctx, which, buf.ctypes.data, n) != _lib.NWE_OK:
            raise RuntimeError("nwe_packed_bias_copy failed")
        return buf.reshape(-1, 32)

    def packed_scale(self, which: int) -> float:
        return float(self._lib.nwe_packed_scale(self._ctx, which))

    def packed_colour_finite(self, which: int) -> bool:
        """Whether the colour layers of network `which` are finite as packed (include/nwe.h: nwe_packed_colour_finite)."""
        return int(self._lib.nwe_packed_colour_finite(self._ctx, which)) == 1

    def selftest(self):
        rep = (C.c_int32 * 8)()
        rc = self._lib.nwe_selftest(self._ctx, rep)
        return rc, list(rep)


class TiledRenderer:
    """Several HIP contexts in ONE process - one per device, or several on one device - that render one frame together:
    context i renders the row tile ``dist.shard_rows(H, n)[i]`` of every pose on its own stream and the tiles are copied
    into full frames on the first device (``nwe_render_tiled``: hipMemcpyPeerAsync over xGMI).  This is the multi-GPU path
    of the reference's synchronous GUI call (application/app.py:336 -> workspace.py:66 -> render_coordinates), which cannot
    be a torchrun rank; one process per GPU with an RCCL gather is ``nwe_amd.dist``.

    ``devices`` lists the device of every tile, e.g. ``[0, 1, 2, 3]`` or, for tests on a one-GPU box, ``[0, 0, 0]``.
    The first renderer doubles as the single-context surface (``render_rays``, ``to8b``, ``create_rays`` ...)."""

    def __init__(self, devices: Sequence[int]):
        if not devices:
            raise ValueError("TiledRenderer needs at least one device")
        self.parts = [Renderer(int(d)) for d in devices]
        self.devices = [int(d) for d in devices]
        self._lib = self.parts[0]._lib
        self._ctxs = (C.c_void_p * len(self.parts))(*[p._ctx for p in self.parts])
        self.last_tiled = False                 # did the last render() go through nwe_render_tiled?

    def __getattr__(self, name):            # everything else: the first context (same device as the assembled frames)
        if name in ("parts", "_lib", "_ctxs", "devices", "last_tiled"):
            raise AttributeError(name)      # not constructed yet: no delegation (and no recursion through self.parts)
        return getattr(self.parts[0], name)

    def close(self) -> None:
        for p in self.parts:
            p.close()

    def set_network(self, which: int, state_dict: Mapping[str, object]):
        return [p.set_network(which, state_dict) for p in self.parts][0]

    def set_sampling(self, n_samples: int, n_importance: int) -> None:
        for p in self.parts:
            p.set_sampling(n_samples, n_importance)

    def set_white_background(self, on: bool) -> None:
        for p in self.parts:
            p.set_white_background(on)

    def debug_set_fold(self, on: bool) -> None:
        for p in self.parts:
            p.debug_set_fold(on)

    def debug_set_work_queue(self, mode: int) -> None:
        for p in self.parts:
            p.debug_set_work_queue(mode)

    def set_early_termination(self, min_transmittance: float) -> None:
        for p in self.parts:
            p.set_early_termination(min_transmittance)

    def set_shared_coarse(self, k: int) -> None:
        for p in self.parts:
            p.set_shared_coarse(k)

    def set_separate_passes(self, on: bool) -> None:
        for p in self.parts:
            p.set_separate_passes(on)

    def set_occupancy(self, bits, lo: Sequence[float], hi: Sequence[float], resolution) -> None:
        for p in self.parts:
            p.set_occupancy(bits, lo, hi, resolution)

    def build_occupancy(self, lo: Sequence[float], hi: Sequence[float], resolution, probes: int = 2, threshold: float = 0.0,
                        dilate: int = 1, precision: str = "f16x3") -> None:
        """Built once, on the first part, and copied to the others: every tile reads the same bits."""
        first = self.parts[0]
        first.build_occupancy(lo, hi, resolution, probes, threshold, dilate, precision)
        g = first.occupancy
        for p in self.parts[1:]:
            p.set_occupancy(first.occupancy_bits(), g["lo"], g["hi"], g["resolution"])

    def clear_occupancy(self) -> None:
        for p in self.parts:
            p.clear_occupancy()

    def set_coarse_grid(self, sigma, lo: Sequence[float], hi: Sequence[float], resolution=None) -> None:
        if isinstance(sigma, torch.Tensor):   # one host copy serves every part, whatever device it is on
            sigma = sigma.detach().cpu().numpy()
        for p in self.parts:
            p.set_coarse_grid(sigma, lo, hi, resolution)

    def bake_coarse_grid(self, lo: Sequence[float], hi: Sequence[float], resolution, precision: str = "f16x3") -> None:
        """Baked once, on the first part, and copied to the others: every tile reads the same values."""
        first = self.parts[0]
        first.bake_coarse_grid(lo, hi, resolution, precision)
        g = first.coarse_grid
        values = first.coarse_grid_values() if len(self.parts) > 1 else None
        for p in self.parts[1:]:
            p.set_coarse_grid(values, g["lo"], g["hi"], g["resolution"])

    def clear_coarse_grid(self) -> None:
        for p in self.parts:
            p.clear_coarse_grid()

    def render(self, c2w, H: int, W: int, *, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
               rows: Optional[Tuple[int, int]] = None, precision: str = "f16x3",
               outputs: Sequence[str] = ("rgb", "depth", "acc")) -> Dict[str, torch.Tensor]:
        """Whole frames [B*H*W, ...] on the first device.  A caller that asks for a proper row range, or for outputs other
        than rgb / depth / acc, gets the single-context path (those are test and diagnostic surfaces); ``rows=(0, H)`` is the
        whole frame and is tiled like ``rows=None``."""
        whole = rows is None or (int(rows[0]), int(rows[1])) == (0, H)
        self.last_tiled = whole and set(outputs) <= {"rgb", "depth", "acc"}
        if not self.last_tiled:
            return self.parts[0].render(c2w, H, W, fx=fx, fy=fy, cx=cx, cy=cy, near=near, far=far, rows=rows, precision=precision,
                                        outputs=outputs)
        poses = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1, 4, 4))
        first = self.parts[0]
        n = poses.shape[0] * H * W
        with torch.cuda.device(first.device):
            res = {k: torch.empty((n, 3) if k == "rgb" else (n,), dtype=torch.float32, device=first.device) for k in outputs}
            res["flags"] = torch.zeros(1, dtype=torch.int32, device=first.device)
            ptr = lambda k: res[k].data_ptr() if k in res else None
            stream = torch.cuda.current_stream(first.device).cuda_stream
            rc = self._lib.nwe_render_tiled(self._ctxs, len(self.parts), poses.ctypes.data, poses.shape[0], H, W, fx, fy, cx, cy, near,
                                            far, _lib.PRECISIONS[precision], ptr("rgb"), ptr("depth"), ptr("acc"), ptr("flags"), stream)
        first._check(rc, "nwe_render_tiled")
        return res

    def tile_kernel_ms(self):
        """Kernel time of every tile of the last frame (HIP events on the tiles' own streams); -1 for a tile that has not
        rendered.  The calling thread's current device is left as it was."""
        return [p.last_kernel_ms() for p in self.parts]

    def last_warning(self) -> str:
        """What the last tiled frame went through without failing (peer access unavailable -> staged copies), "" if nothing."""
        return self._lib.nwe_last_warning(self.parts[0]._ctx).decode()

    def peer_access(self):
        """Per tile: 1 if its device can write the first device's memory directly (hipDeviceCanAccessPeer; same device = 1),
        0 if the copy is staged by the runtime, -1 if the query failed."""
        return [int(self._lib.nwe_debug_peer_access(self.parts[0]._ctx, p._ctx)) for p in self.parts]
