"""The grid and sparse kernels past one scan tile and one chunk (the sizes and scenes: tests/grid_sizes.py, vetted on the CPU by
tests/test_grid_sizes_host.py).  The other files test the rule on frames of a few hundred rays and grids of a few thousand cells;
here every loop of csrc/nwe_sparse.hip and of the host code around it takes its second turn:

A. a chunk of 2 560 rays: sparse_scan_kernel scans tiles of 1024, 1024 and 512 counts with a carry.  The rows of every selected
   sample are nwe_query_points' at that ray's own points, ray by ray - which a wrong offset anywhere would break - and the grid's
   elsewhere; chunk borders one ray before, on and behind the tile edges, everything and nothing selected over three tiles, and
   2.5 tiles of zeros behind a non-zero carry give the same bits.
B. 11 520 rays at 128 + 256: the default chunk of 2^22 // 384 = 10 922 rays splits the call inside image row 91, and the scratch
   buffer is laid out at its full size; a small call, this call and the small call again on one context give the fresh contexts' bits.
C. nwe_bake_radiance_grid and nwe_bake_coarse_grid over 128 x 128 x 65 cells: one full chunk of 2^20 cells and a ragged one.  The
   grid is nwe_query_points at the cells' centres, bit for bit, the query run whole and split at the border; 512 cells about the
   border are held to the fp64 oracle by the criterion of tests/accuracy.py; a small bake behind the large one renders a fresh
   context's frame.
D. an axis of 512 cells, the largest a grid may have, looked up on the device by nwe_render_grid, nwe_coarse_grid_weights and
   nwe_render_sparse against the numpy restatements, bit for bit.
"Bit for bit" lets a NaN equal a NaN whatever its sign and payload.
"""
import numpy as np
import pytest
import torch

import nwe_amd
from tests import accuracy as A
from tests import coarse_grid as B
from tests import grid_sizes as Z
from tests import radiance_grid as R
from tests import sparse_fine as SF

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
DIAG = ("weights_coarse", "z_fine", "weights_grid", "selected", "raw_fine")
K32 = 1.5            # tests/test_gpu_accuracy.py's bound for raw outputs of random networks; measured here: the f32 bake 1.00 x the fp32
                     # oracle's error at the most, the f16x3 bake 1.12 x its yardstick


def _renderer(grid, ns, ni, sds=None):
    """Both networks of a scene (s7's by default) and the grid behind them: an upload clears a grid."""
    sd_c, sd_f = sds or B.scene("s7")[:2]
    r = nwe_amd.Renderer(0)
    r.set_network(0, sd_c); r.set_network(1, sd_f)
    r.set_sampling(ns, ni)
    if grid is not None:
        r.set_radiance_grid(grid["values"], grid["lo"], grid["hi"])
    return r


def _sparse(r, poses, H, W, outputs=LEAN, **kw):
    return r.render_sparse(poses.numpy(), H, W, outputs=outputs, **Z.camera(H, W), **kw)


def _grid_frame(r, poses, H, W, outputs=LEAN):
    return r.render_grid(poses.numpy(), H, W, outputs=outputs, **Z.camera(H, W))


def _eq(a, b):
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _same(a, b, ctx, keys=LEAN):
    for k in keys:
        assert _eq(a[k], b[k]), (ctx, k, _first_ray(a[k], b[k]))
    assert int(a["flags"].item()) == int(b["flags"].item()), ctx


def _first_ray(a, b):
    """The first rays (leading index) at which two outputs differ: what a failure says."""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    differ = ~(((a == b) | (a.isnan() & b.isnan())) if a.dtype == torch.float32 else (a == b)).all(-1)
    rays = torch.nonzero(differ).reshape(-1)
    return f"{int(rays.numel())} rays differ, the first at {rays[:4].tolist()}"


def _far_pose(poses):
    """A second pose a hundred units away: every sample of its rays lies outside every box of the tests."""
    far = poses[:1].clone()
    far[0, 0, 3] += 100.0
    return torch.cat([poses[:1], far])


def _check_rows(r, out, poses, H, W, precision, idx=None):
    """raw_fine is nwe_query_points' row at the helper's point of the call's own depth where selected, ray by ray, and the grid
    frame's row elsewhere - on the rays `idx` (all of them by default)."""
    rays = r.create_rays(poses.numpy(), H, W, **Z.camera(H, W))
    grid_rows = _grid_frame(r, poses, H, W, outputs=("raw_fine",))["raw_fine"]
    sel, raw, z = out["selected"].bool(), out["raw_fine"], out["z_fine"]
    if idx is not None:
        at = torch.from_numpy(idx).to(r.device)
        rays, grid_rows, sel, raw, z = rays[at], grid_rows[at], sel[at], raw[at], z[at]
    pts = torch.from_numpy(SF.points(rays.cpu().numpy(), z.cpu().numpy())).to(r.device)
    q = r.query_points(pts, rays[:, 8:11].contiguous(), which=1, precision=precision, outputs=("raw",))["raw"]
    only = lambda x, m: torch.where(m[..., None], x, torch.zeros_like(x))
    assert _eq(raw[sel], q[sel]), ("selected rows", _first_ray(only(raw, sel), only(q, sel)))
    assert _eq(raw[~sel], grid_rows[~sel]), ("the other rows", _first_ray(only(raw, ~sel), only(grid_rows, ~sel)))
    assert not _eq(q[sel], grid_rows[sel])            # a frame of grid rows alone would not pass


# ---- A. the scan past one tile --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_rows_of_a_chunk_of_three_scan_tiles_are_each_rays_own(precision):
    _, poses, _ = Z.scan_frame()
    H, W = Z.SCAN_H, Z.SCAN_W
    r = _renderer(R.grid(Z.SCAN_GRID), 7, 6)
    try:
        out = _sparse(r, poses, H, W, outputs=("z_fine", "weights_grid", "selected", "raw_fine"), precision=precision,
                      min_weight=Z.SCAN_MIN_WEIGHT, dilate=Z.SCAN_DILATE)
        count = r.last_sparse_samples()
        sel = out["selected"].cpu().numpy().astype(bool)
        counts = Z.scan_premises(sel)
        print(f"scan scene on the device, {precision}: {Z.describe_counts(counts)}")
        assert np.array_equal(sel, SF.select(out["weights_grid"].cpu().numpy(), Z.SCAN_MIN_WEIGHT, Z.SCAN_DILATE))
        assert count == (int(sel.sum()), 2560 * 13)
        _check_rows(r, out, poses, H, W, precision)
    finally:
        r.close()


def test_chunk_borders_on_and_off_the_tile_edges_give_the_same_bits():
    """1024: exactly one full tile; 1025: a full tile and one ray; 2049: two full tiles and one ray; 0: the whole frame, three tiles."""
    keys = LEAN + DIAG
    _, poses, _ = Z.scan_frame()
    H, W = Z.SCAN_H, Z.SCAN_W
    kw = dict(min_weight=Z.SCAN_MIN_WEIGHT, dilate=Z.SCAN_DILATE, outputs=keys)
    r = _renderer(R.grid(Z.SCAN_GRID), 7, 6)
    try:
        first = count = None
        for chunk in Z.SCAN_CHUNKS:
            r.debug_set_sparse_chunk(chunk)
            out = _sparse(r, poses, H, W, **kw)
            if first is None:
                first, count = out, r.last_sparse_samples()
                Z.scan_premises(first["selected"].cpu().numpy())
                continue
            _same(out, first, ("chunk", chunk), keys)
            assert r.last_sparse_samples() == count, chunk
    finally:
        r.close()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_everything_and_nothing_selected_over_three_tiles(precision):
    """min_weight -1: every ray selects its 13 samples, every offset is a multiple of 13, and the frame is nwe_render's under a baked
    coarse pass (tests/test_gpu_sparse_fine.py's set-up); min_weight 2: the grid frame."""
    _, poses, _ = Z.scan_frame()
    H, W = Z.SCAN_H, Z.SCAN_W
    g = R.grid(Z.SCAN_GRID)
    r = _renderer(g, 7, 6)
    try:
        out = _sparse(r, poses, H, W, outputs=LEAN + ("selected",), precision=precision, min_weight=-1.0, dilate=0)
        assert bool(out["selected"].bool().all()) and r.last_sparse_samples() == (33280, 33280)
        none = _sparse(r, poses, H, W, outputs=LEAN + ("selected", "raw_fine"), precision=precision, min_weight=2.0, dilate=0)
        assert int(none["selected"].sum()) == 0 and r.last_sparse_samples() == (0, 33280)
        _same(none, _grid_frame(r, poses, H, W, outputs=LEAN + ("raw_fine",)), "min_weight 2", LEAN + ("raw_fine",))
        r.set_coarse_grid(np.ascontiguousarray(g["values"][..., 3]), g["lo"], g["hi"])
        ref = r.render(poses.numpy(), H, W, precision=precision, outputs=LEAN, **Z.camera(H, W))
        _same(out, ref, ("min_weight -1", precision))
        assert not _eq(out["rgb"], none["rgb"])
    finally:
        r.close()


def test_two_and_a_half_tiles_of_zeros_behind_a_carry():
    """Two poses in one call under the default chunk: one chunk of 5 120 rays, of which the second pose's 2 560 select nothing - the
    scan's last 2.5 tiles add zeros to a non-zero carry.  The call is the two single-pose calls one after the other."""
    keys = LEAN + DIAG
    _, poses, _ = Z.scan_frame()
    H, W = Z.SCAN_H, Z.SCAN_W
    both_poses = _far_pose(poses)
    kw = dict(min_weight=Z.SCAN_MIN_WEIGHT, dilate=Z.SCAN_DILATE, outputs=keys)
    r = _renderer(R.grid(Z.SCAN_GRID), 7, 6)
    try:
        both = _sparse(r, both_poses, H, W, **kw)
        count = r.last_sparse_samples()
        each = [_sparse(r, both_poses[p:p + 1], H, W, **kw) for p in range(2)]
        sel = [e["selected"].bool() for e in each]
        assert bool(sel[0].any()) and not bool(sel[1].any()) and count == (int(sel[0].sum()), 5120 * 13)
        for k in keys:
            joined = torch.cat([e[k] for e in each])
            assert _eq(joined, both[k]), (k, _first_ray(joined, both[k]))
        assert int(both["flags"].item()) == int(each[0]["flags"].item()) | int(each[1]["flags"].item())
    finally:
        r.close()


# ---- B. the default chunk -------------------------------------------------------------------------------------------------------

DEF_KEYS = LEAN + ("selected", "z_fine", "weights_grid", "raw_fine")


def _default_call(r):
    _, poses, _ = Z.default_frame()
    return _sparse(r, poses, Z.DEF_H, Z.DEF_W, outputs=DEF_KEYS, min_weight=Z.DEF_MIN_WEIGHT, dilate=Z.DEF_DILATE)


def _scan_call(r):
    _, poses, _ = Z.scan_frame()
    return _sparse(r, poses, Z.SCAN_H, Z.SCAN_W, outputs=LEAN + DIAG, min_weight=Z.SCAN_MIN_WEIGHT, dilate=Z.SCAN_DILATE)


def test_the_default_chunk_splits_a_call_inside_a_row():
    """11 520 rays at 128 + 256 under the default chunk: 10 922 rays and 598, the border behind the second ray of image row 91."""
    _, poses, _ = Z.default_frame()
    H, W = Z.DEF_H, Z.DEF_W
    r = _renderer(R.grid(Z.SCAN_GRID), Z.DEF_NS, Z.DEF_NI)
    try:
        whole = _default_call(r)
        count = r.last_sparse_samples()
        share = count[0] / count[1]
        print(f"default chunk scene on the device: {count[0]} of {count[1]} samples selected, share {share:.4f}")
        assert count[1] == H * W * 384 and Z.DEF_SHARE[0] < share < Z.DEF_SHARE[1]     # cheap, and both values there: no quality claim
        for chunk in Z.DEF_CHUNKS[1:]:
            r.debug_set_sparse_chunk(chunk)
            _same(_default_call(r), whole, ("chunk", chunk), DEF_KEYS)
            assert r.last_sparse_samples() == count, chunk
        r.debug_set_sparse_chunk(0)
        sel = whole["selected"].cpu().numpy().astype(bool)
        assert np.array_equal(sel, SF.select(whole["weights_grid"].cpu().numpy(), Z.DEF_MIN_WEIGHT, Z.DEF_DILATE))
        assert count[0] == int(sel.sum()) and sel[:Z.DEF_CAP].any() and sel[Z.DEF_CAP:].any()
        # the rows of image rows 89 .. 93 - the border with two rows on either side - and of every 16th ray
        _check_rows(r, whole, poses, H, W, "f16x3", Z.default_subset())
    finally:
        r.close()


def test_the_scratch_buffer_grown_and_reused_gives_fresh_contexts_bits():
    """A small call at 7 + 6, the default-chunk call at 128 + 256 (the scratch grows to its full layout) and the small call again
    (a small layout in the grown buffer) on one context; a context that makes only the large call; one that makes only the small."""
    g = R.grid(Z.SCAN_GRID)
    r, large_only, small_only = _renderer(g, 7, 6), _renderer(g, Z.DEF_NS, Z.DEF_NI), _renderer(g, 7, 6)
    try:
        small = _scan_call(r)
        small_count = r.last_sparse_samples()
        r.set_sampling(Z.DEF_NS, Z.DEF_NI)
        large = _default_call(r)
        large_count = r.last_sparse_samples()
        r.set_sampling(7, 6)
        again = _scan_call(r)
        assert r.last_sparse_samples() == small_count and 0 < small_count[0] < small_count[1]
        _same(again, small, "the small call behind the large one", LEAN + DIAG)
        _same(_scan_call(small_only), small, "a context of the small call alone", LEAN + DIAG)
        assert small_only.last_sparse_samples() == small_count
        _same(_default_call(large_only), large, "a context of the large call alone", DEF_KEYS)
        assert large_only.last_sparse_samples() == large_count and 0 < large_count[0] < large_count[1]
    finally:
        r.close(); large_only.close(); small_only.close()


# ---- C. bakes past one chunk of cells -------------------------------------------------------------------------------------------

def _bits_differ(got, want):
    """Where two float32 arrays differ bit for bit, a NaN equal to a NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))


def _query_whole_and_split(r, centres, d, which, precision, outputs):
    """nwe_query_points at all centres in one call, and in two calls split at the bakes' chunk border: equal, so that the query's own
    size handling is not what the comparison trusts."""
    key = outputs[0]
    dirs = None if d is None else torch.tensor([d], device=r.device)
    q = lambda p: r.query_points(p[None] if dirs is not None else p, dirs, which=which, precision=precision, outputs=outputs)[key]
    whole = q(centres).reshape((-1, 4) if key == "raw" else (-1,))
    parts = torch.cat([q(centres[:Z.BAKE_CHUNK_CELLS]).reshape(whole[:Z.BAKE_CHUNK_CELLS].shape),
                       q(centres[Z.BAKE_CHUNK_CELLS:]).reshape(whole[Z.BAKE_CHUNK_CELLS:].shape)])
    assert _eq(whole, parts), ("the query whole and split", which, precision, _first_ray(whole, parts))
    return whole.cpu().numpy()


def _sides(rows):
    return (("in front of the border", rows[:Z.BAKE_CHUNK_CELLS]), ("behind the border", rows[Z.BAKE_CHUNK_CELLS:]))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bakes_of_a_full_chunk_of_cells_and_a_ragged_one(precision):
    lo, hi, res = Z.BAKE_LO, Z.BAKE_HI, Z.BAKE_RES
    r = _renderer(None, 7, 6, Z.bake_nets())
    fresh = _renderer(None, 7, 6, Z.bake_nets())
    try:
        centres = torch.from_numpy(Z.centres(lo, hi, res)).to(r.device)
        assert centres.shape[0] == Z.BAKE_CELLS
        for which in (1, 0):
            d = Z.BAKE_DIRS[which]
            want = _query_whole_and_split(r, centres, d, which, precision, ("raw",))
            r.bake_radiance_grid(lo, hi, res, which=which, view_dir=d, precision=precision)
            assert r.radiance_grid["resolution"] == res
            got = r.radiance_grid_values().reshape(-1, 4)
            differ = _bits_differ(got, want).any(-1)
            assert not differ.any(), ("radiance bake", which, int(differ.sum()), np.flatnonzero(differ)[:4].tolist())
            for name, side in _sides(got):
                assert float(np.std(side[:, 3])) > 1e-3 and float(np.std(side[:, :3])) > 1e-3, (which, name)
        want = _query_whole_and_split(r, centres, None, 0, precision, ("sigma",))
        r.bake_coarse_grid(lo, hi, res, precision=precision)
        got = r.coarse_grid_values()
        assert got.shape == res
        differ = _bits_differ(got.reshape(-1), want)
        assert not differ.any(), ("coarse bake", int(differ.sum()), np.flatnonzero(differ)[:4].tolist())
        for name, side in _sides(got.reshape(-1)):
            assert float(np.std(side)) > 1e-3, name
        # a small bake behind the large ones: the scratch and the grid's buffer are reused after a shrink
        poses, _ = B.G.E.frame_rays(R.H, R.W, 1)
        frames = []
        for ctx in (r, fresh):
            ctx.bake_radiance_grid(lo, hi, (5, 7, 9), which=1, view_dir=Z.BAKE_DIRS[1], precision=precision)
            frames.append(_grid_frame(ctx, poses, R.H, R.W, outputs=LEAN + ("raw_fine",)))
        assert np.array_equal(r.radiance_grid_values(), fresh.radiance_grid_values(), equal_nan=True)
        _same(frames[0], frames[1], "a small bake behind a large one", LEAN + ("raw_fine",))
        assert float(frames[0]["acc"].max()) > 0.05
    finally:
        r.close(); fresh.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_bake_of_a_network_without_view_directions_past_one_chunk(precision):
    lo, hi, res = Z.BAKE_LO, Z.BAKE_HI, Z.BAKE_RES
    r = _renderer(None, 7, 6, Z.bake_nets(False))
    try:
        centres = torch.from_numpy(Z.centres(lo, hi, res)).to(r.device)
        want = _query_whole_and_split(r, centres, None, 1, precision, ("raw",))
        r.bake_radiance_grid(lo, hi, res, which=1, view_dir=None, precision=precision)
        got = r.radiance_grid_values().reshape(-1, 4)
        differ = _bits_differ(got, want).any(-1)
        assert not differ.any(), (int(differ.sum()), np.flatnonzero(differ)[:4].tolist())
        for name, side in _sides(got):
            assert float(np.std(side[:, 3])) > 1e-3 and float(np.std(side[:, :3])) > 1e-3, name
    finally:
        r.close()


def test_baked_rows_about_the_chunk_border_against_fp64():
    """The criterion of tests/accuracy.py on the baked rows of 512 cells about the border (the 128 in front of it and the 384 behind it,
    and the 256 on either side of it), the centres formed in numpy from the rule: the f32 bake within K32 x the fp32 oracle's error,
    the f16x3 bake within 1.5 x the larger of the oracle's and the f32 bake's, that one capped at K32 x the oracle's."""
    lo, hi, res = Z.BAKE_LO, Z.BAKE_HI, Z.BAKE_RES
    rep = A.Report()
    r = _renderer(None, 7, 6, Z.bake_nets())
    try:
        for which in (1, 0):
            d = Z.BAKE_DIRS[which]
            rows = {}
            for precision in ("f32", "f16x3"):
                r.bake_radiance_grid(lo, hi, res, which=which, view_dir=d, precision=precision)
                rows[precision] = r.radiance_grid_values().reshape(-1, 4)
            for name, (a, b) in Z.BAKE_BORDER_CELLS.items():
                pts = Z.centres(lo, hi, res, a, b - a)[None]
                dirs = torch.tensor([d])
                y32 = SF.oracle_rows(Z.bake_nets()[which], pts, dirs)[0]
                y64 = SF.oracle_rows(Z.bake_nets()[which], pts, dirs, dtype=torch.float64)[0]
                rep.add(f"bake, network {which}, cells {name}, f32", rows["f32"][a:b], y32, y64, factor=K32)
                rep.add(f"bake, network {which}, cells {name}, f16x3", rows["f16x3"][a:b], y32, y64, y_alt=rows["f32"][a:b], alt_cap=K32)
        rep.check()
    finally:
        r.close()


# ---- D. a 512-cell axis ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_512_cell_axis_is_looked_up_as_the_numpy_restatements_say(axis):
    poses, _, grid, cgrid = Z.long_axis_case(axis)
    H, W = R.H, R.W
    r = _renderer(grid, 7, 6)
    try:
        rays = r.create_rays(poses.numpy(), H, W, **Z.camera(H, W)).cpu().numpy()
        # the radiance grid's rows at the call's own depths
        out = _grid_frame(r, poses, H, W, outputs=("z_fine", "raw_fine"))
        pts = SF.points(rays, out["z_fine"].cpu().numpy())
        want = R.grid_rows(pts, grid, np.float32)
        got = out["raw_fine"].cpu().numpy()
        differ = _bits_differ(got, want).any(-1)
        assert not differ.any(), ("radiance grid", int(differ.sum()), np.argwhere(differ)[:4].tolist())
        gc, inside, i0, i1 = Z.taps(pts, grid)                                     # the cases are there, at the device's depths
        a = gc[..., axis]
        clamped, beyond = inside & (a > 510.5) & (a <= 511.5), ~inside & (a > 511.5)
        assert clamped.any() and beyond.any() and (want[clamped] != 0).any() and (got[beyond] == 0).all()
        # the sparse proposal's lookup: nothing selected, so every row is the grid's
        none = _sparse(r, poses, H, W, outputs=("selected", "z_fine", "raw_fine"), min_weight=2.0, dilate=0)
        assert int(none["selected"].sum()) == 0 and _eq(none["z_fine"], out["z_fine"])
        assert _eq(none["raw_fine"], out["raw_fine"]), _first_ray(none["raw_fine"], out["raw_fine"])
        # the coarse grid's sigma at the coarse depths
        r.set_coarse_grid(cgrid["values"], cgrid["lo"], cgrid["hi"])
        sigma = r.coarse_grid_weights(poses.numpy(), H, W, outputs=("sigma",), **Z.camera(H, W))["sigma"].cpu().numpy()
        cpts = B.coarse_points(rays, 7)[1]
        want = B.grid_sigma(cpts, cgrid)
        differ = _bits_differ(sigma, want)
        assert not differ.any(), ("coarse grid", int(differ.sum()), np.argwhere(differ)[:4].tolist())
        gc, inside, _, _ = Z.taps(cpts, cgrid)
        a = gc[..., axis]
        assert (inside & (a > 510.5) & (a <= 511.5)).any() and (~inside & (a > 511.5)).any() and (want[inside] != 0).any()
    finally:
        r.close()
