"""What the size tests of the grid and sparse kernels share (tests/test_grid_sizes_host.py, tests/test_gpu_grid_sizes.py): the
sizes at which the loops of csrc/nwe_sparse.hip and of the host code in csrc/nwe_abi_grids.hip and csrc/nwe_abi_sparse.hip take a
second turn, and the scenes there.

A. `sparse_scan_kernel` scans a chunk's per-ray counts in tiles of SCAN_TILE: a 40 x 64 frame is tiles of 1024, 1024 and 512 rays.
   `tiled_scan` restates the kernel tile by tile in numpy; `scan_premises` says what the frame's selection must hold for the
   carry, the ragged tile and the reads across a tile border to matter.
B. nwe_render_sparse cuts a call into chunks of SPARSE_CHUNK_SAMPLES // S rays: 96 x 120 rays at 128 + 256 are two chunks whose
   border lies inside image row 91.  `default_subset` names the rays whose rows are compared one by one.
C. Both bakes walk the cells in chunks of BAKE_CHUNK_CELLS: 128 x 128 x 65 cells are a full chunk and a ragged one of 16 384.
   `centres` restates the cell centres in numpy, `bake_nets` are the networks.
D. `long_axis_case` puts an axis of 512 cells, the largest nwe_set_*_grid accepts, along the depth range of a camera that looks
   down that axis; `taps` restates the lookup's coordinate and indices so that the host test can count the cases.
The constants are restated from the sources named beside them; the grids are built here and are none of tests/radiance_grid.py's
GRIDS, which its parametrisations read.
"""
import functools

import numpy as np
import torch

import nwe_amd
from oracle import nerf_oracle as O
from tests import coarse_grid as B
from tests import radiance_grid as R
from tests import sparse_fine as SF

SCAN_TILE = 1024                     # kScanThreads (csrc/nwe_sparse.hip)
SPARSE_CHUNK_SAMPLES = 1 << 22       # kSparseChunkSamples (csrc/nwe_plan.h)
BAKE_CHUNK_CELLS = 1 << 20           # probe_lattice at probes = 1 (csrc/nwe_abi_grids.hip)


def camera(H, W):
    fx, fy, cx, cy = O.intrinsics(H, W)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=R.NEAR, far=R.FAR)


# ---- A. the scan past one tile ------------------------------------------------------------------------------------------------

SCAN_SCENE, SCAN_GRID = "s7", "smooth"                    # 7 + 6 samples, 4x128 networks; the 1-unit cells over the scene box
SCAN_H, SCAN_W = 40, 64                                   # 2 560 rays
SCAN_TILES = ((0, 1024), (1024, 2048), (2048, 2560))
SCAN_MIN_WEIGHT, SCAN_DILATE = 0.15, 2                    # chosen on the CPU (tests/test_grid_sizes_host.py prints what they give)
SCAN_CHUNKS = (1023, 1024, 1025, 2047, 2048, 2049, 0)     # a border one ray before, on and one ray behind a tile's edge; the default


@functools.lru_cache(maxsize=None)
def scan_frame(n_poses=1):
    """(cfg, poses, rays) of the 40 x 64 frame on the shared camera: leave them unchanged."""
    cfg = B.scene(SCAN_SCENE)[2]
    poses, rays = B.G.E.frame_rays(SCAN_H, SCAN_W, n_poses)
    return cfg, poses, rays


def tiled_scan(counts, tile=SCAN_TILE, wave=64):
    """sparse_scan_kernel restated: counts [n] -> (exclusive offsets [n], total), uint32 as the kernel's.  Tile by tile: the
    inclusive scan within each wave of 64, the exclusive scan of the waves' sums, the tile's sum, and the running carry that every
    later tile adds; elements behind the end count as 0."""
    counts = np.asarray(counts, dtype=np.uint32)
    n = counts.size
    offsets = np.empty(n, np.uint32)
    carry = np.uint32(0)
    with np.errstate(over="ignore"):
        for base in range(0, n, tile):
            v = np.zeros(tile, np.uint32)
            m = min(tile, n - base)
            v[:m] = counts[base:base + m]
            incl = np.cumsum(v.reshape(tile // wave, wave), axis=1, dtype=np.uint32)
            w = incl[:, -1]
            wi = np.cumsum(w, dtype=np.uint32)
            s_wave, s_tile = wi - w, wi[-1]
            out = (carry + s_wave[:, None] + incl - v.reshape(tile // wave, wave)).astype(np.uint32).reshape(-1)
            offsets[base:base + m] = out[:m]
            carry = np.uint32(carry + s_tile)
    return offsets, int(carry)


def scan_premises(selected):
    """selected [2560, S] bool -> the per-ray counts, after asserting what the scan test rests on: at least four distinct counts, the
    count 0, a non-zero count in every tile, something selected on the four rays beside the two tile edges, both values of the mask."""
    sel = np.asarray(selected).astype(bool)
    assert sel.shape[0] == SCAN_H * SCAN_W
    counts = sel.sum(-1)
    assert np.unique(counts).size >= 4, np.unique(counts)
    assert (counts == 0).any()
    for a, b in SCAN_TILES:
        assert (counts[a:b] > 0).any(), (a, b)
    assert counts[[1023, 1024, 2047, 2048]].any()
    assert sel.any() and (~sel).any()
    return counts


def describe_counts(counts):
    values, n = np.unique(counts, return_counts=True)
    tiles = ", ".join(f"[{a}, {b}): {int((counts[a:b] > 0).sum())} of {b - a}" for a, b in SCAN_TILES)
    edges = ", ".join(f"{i}: {int(counts[i])}" for i in (1023, 1024, 2047, 2048))
    return (f"per-ray counts {dict(zip(values.tolist(), n.tolist()))}; rays with a non-zero count per tile {tiles}; at the tile edges {edges}; "
            f"selected {int(counts.sum())} of {counts.size * 13}")


# ---- B. the default chunk -----------------------------------------------------------------------------------------------------

DEF_NS, DEF_NI = 128, 256
DEF_H, DEF_W = 96, 120                                                   # 11 520 rays
DEF_CAP = SPARSE_CHUNK_SAMPLES // (DEF_NS + DEF_NI)                      # 10 922 rays: the border lies in row 91, behind 2 of its 120 rays
DEF_MIN_WEIGHT, DEF_DILATE = 0.0036, 1                                   # chosen on the CPU for a share between 1 % and 20 %
DEF_SHARE = (0.01, 0.20)
DEF_STRIDE = 16                                                          # rays 0, 16, 32, ... of the frame: what the host test vets
DEF_BORDER_ROWS = (89, 94)                                               # image rows 89 .. 93: the border's row and two on either side
DEF_CHUNKS = (0, 4096, DEF_CAP)


@functools.lru_cache(maxsize=None)
def default_frame():
    """(cfg, poses, rays) of the 96 x 120 frame at 128 + 256 on the shared camera: leave them unchanged."""
    cfg = O.RenderConfig(n_samples=DEF_NS, n_importance=DEF_NI)
    poses, rays = B.G.E.frame_rays(DEF_H, DEF_W, 1)
    return cfg, poses, rays


def default_subset():
    """The rays whose rows the GPU test compares one by one: every ray of image rows 89 .. 93 and every 16th ray of the frame."""
    idx = np.arange(DEF_H * DEF_W)
    row = idx // DEF_W
    return np.flatnonzero(((row >= DEF_BORDER_ROWS[0]) & (row < DEF_BORDER_ROWS[1])) | (idx % DEF_STRIDE == 0))


# ---- C. bakes past one chunk of cells -----------------------------------------------------------------------------------------

BAKE_LO, BAKE_HI, BAKE_RES = (-3.0, -1.0, -2.0), (9.0, 11.0, 3.0), (128, 128, 65)      # the box of the occupancy build's test
BAKE_CELLS = 128 * 128 * 65                                                          # 2^20 + 16 384
BAKE_DIRS = {1: (0.6, 0.0, -0.8), 0: (0.0, 2.0, 0.0)}                                # used as given, not normalised
# the cells that the fp64 yardstick is taken at: 512 cells about the chunk border, 128 in front of it and 384 behind it, and the
# 256 on either side of it
BAKE_BORDER_CELLS = {"1048448..1048959": (1048448, 1048960), "256 either side": (BAKE_CHUNK_CELLS - 256, BAKE_CHUNK_CELLS + 256)}


def centres(lo, hi, res, first=0, count=None):
    """The centres [count, 3] of the flat cells first .. first + count - 1 (z fastest) in float32: (i + 0.5) * step + lo, with the
    step rounded to float32 once, a float32 product, then a float32 sum (tests/test_gpu_occupancy.py's _probe_points at probes 1)."""
    rx, ry, rz = (int(r) for r in res)
    count = rx * ry * rz - first if count is None else count
    i = np.arange(first, first + count, dtype=np.int64)
    cols = []
    for idx, l, h, r in zip((i // (ry * rz), (i // rz) % ry, i % rz), lo, hi, (rx, ry, rz)):
        step = np.float32((float(h) - float(l)) / r)
        cols.append(((idx.astype(np.float32) + np.float32(0.5)) * step).astype(np.float32) + np.float32(l))
    return np.stack(cols, -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def bake_nets(view_dirs=True):
    """(coarse, fine) 4x128 networks: those of tests/test_gpu_radiance_grid.py's bake test, or scene `novd`'s."""
    if not view_dirs:
        return B.scene("novd")[:2]
    S = nwe_amd.synthetic
    return S.thin_fog(S.make_state_dict(1000, 4, 128), 0.3, 1.0), S.dense_fog(S.make_state_dict(1001, 4, 128), 0.5, 1.0)


# ---- D. a 512-cell axis -------------------------------------------------------------------------------------------------------

LONG = 512
LONG_RES = {0: (512, 2, 3), 1: (2, 512, 3), 2: (3, 2, 512)}
# Along the long axis the box ends inside the depth range, so that the rays leave it through the far face; across it, it holds every
# ray.  In the shared camera's own frame (it looks along +y from (0, -0.77, 0.5)) the long axis is y.
LONG_DEPTH = (-1.0, 6.0)
LONG_ACROSS = ((-12.0, 14.0), (-9.0, 10.0))      # x and z of the camera's own frame


def _turn(axis):
    """The rotation that carries y onto `axis` (a cyclic permutation of the axes: proper, and exact in floating point)."""
    m = np.zeros((4, 4), np.float32)
    m[3, 3] = 1
    for c in range(3):
        m[(c + axis - 1) % 3, c] = 1
    return m


@functools.lru_cache(maxsize=None)
def long_axis_case(axis):
    """(poses, rays, radiance grid, coarse grid) with 512 cells along `axis`: the shared 13 x 37 camera turned to look down that axis,
    a box turned with it, random values of both signs."""
    poses, _ = B.G.E.frame_rays(R.H, R.W, 1)
    m = _turn(axis)
    poses = torch.from_numpy(m[None] @ poses.numpy())
    fx, fy, cx, cy = O.intrinsics(R.H, R.W)
    rays = O.create_rays(poses, R.H, R.W, fx, fy, cx, cy, R.NEAR, R.FAR).reshape(-1, 11)
    own = (LONG_ACROSS[0], LONG_DEPTH, LONG_ACROSS[1])             # x, y, z of the camera's own frame
    lo, hi = [0.0] * 3, [0.0] * 3
    for c in range(3):
        lo[(c + axis - 1) % 3], hi[(c + axis - 1) % 3] = own[c]
    res = LONG_RES[axis]
    grid = R.make_grid(R.random_rows(res, seed=40 + axis), lo, hi)
    cgrid = B.make_grid(B.random_values(res, seed=50 + axis), lo, hi)
    return poses, rays, grid, cgrid


def taps(points, grid):
    """The lookup's coordinate and indices as tests/coarse_grid.py's grid_sigma forms them, in float32: (gc [..., 3], inside [...],
    i0 [..., 3], i1 [..., 3]); the indices mean something only where `inside`."""
    p = np.asarray(points, dtype=np.float32)
    lo, inv = grid["lo"].astype(np.float32), grid["inv"].astype(np.float32)
    res = np.array(grid["res"], dtype=np.int64)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        gc = (p - lo) * inv - half
        upper = res.astype(np.float32) - half
        inside = np.isfinite(p).all(-1) & ~(gc < -half).any(-1) & ~(gc > upper).any(-1)
        fl = np.floor(np.where(inside[..., None], gc, np.float32(0)))
    i0 = np.clip(fl.astype(np.int64), 0, res - 1)
    i1 = np.clip(fl.astype(np.int64) + 1, 0, res - 1)
    return gc, inside, i0, i1
