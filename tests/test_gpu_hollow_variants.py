"""The hollow path of mlp_eval (csrc/nwe_mfma_eval.h: CSKIP) in the terminating, occupancy and sharing render kernels, and in the
plain kernels of the two shapes tests/test_gpu_colour_skip.py leaves out (4x256, 8x128).

The path is a wave-uniform branch inside the weight-streaming loop: a hollow wave still issues its quarter of every LDS-DMA chunk
and arrives at every barrier, next to these variants' own control flow - the terminating kernels' early loop exit and lagging
vote, the occupancy kernels' vote barrier, masked lanes and skipped iterations, the sharing consumers' weights from elsewhere.
The scenes are coherent rays of which between a tenth and nine tenths of the (packet, sample) pairs are hollow
(tests/hollow_domain.py; vetted with the CPU oracle in tests/test_hollow_domain_host.py), and every condition is asserted again
from the GPU's own sigma: raw_fine / raw_coarse of a FULL instantiation, which never takes the path.

Every variant is held to the frame with the path off, bit for bit, and to a reference that never takes the path: the plain FULL
instantiation, render_rays fed a hook, or the fp64 masked reference of tests/early_termination.py.  The NaN-head tests prove
where the branch ran: with a NaN in the fine rgb head and the hook that ignores the pack-time guard (mode 2), a ray's rgb is
finite exactly where no evaluation that counts for it ran the colour layers.

Which test takes the branch where (P = proved by a NaN-head test; elsewhere the [0.1, 0.9] hollow share of the reference's sigma
stands for it).  Plain and tail kernels at 8x256 and 4x128: tests/test_gpu_colour_skip.py (P), tests/test_gpu_packet_blocks.py;
plain at 4x256 and 8x128: test_plain_lean_equals_full_and_on_equals_off (the tail kernels of these two shapes:
tests/test_gpu_lean_domain.py).  Terminating, all four shapes: test_terminating_on_equals_off,
test_terminating_kernel_with_nothing_to_stop_gives_the_plain_full_bits, at 4x128 / 8x128 under the packets plan also
test_terminating_packets_plan_leaves_its_loop_at_the_narrow_shapes; 4x128 and 8x256: test_terminating_parity_with_the_masked_reference,
test_terminating_path_runs_exactly_where_predicted (P).  Occupancy, all four: test_occupancy_on_equals_off,
test_occupancy_kernel_with_all_bits_set_gives_the_plain_full_bits; 4x128 and 8x256: test_occupancy_frame_is_the_composite_of_the_masked_full_raw,
test_occupancy_path_runs_exactly_where_predicted (P).  Sharing, all four: test_sharing_on_equals_off; 4x128 and 8x256:
test_separate_passes_with_the_path_on_give_the_plain_full_fused_bits, test_sharing_path_runs_exactly_where_predicted (P),
test_shared_coarse_frame_is_the_full_call_fed_the_representatives_weights, test_baked_coarse_frame_is_the_full_call_fed_the_grids_weights.

64 + 128 at 8x256, one case per variant: test_terminating_on_equals_off, test_occupancy_on_equals_off, test_sharing_on_equals_off.

Measured on an MI355X (f16x3; f16x1 within 0.002), hollow share at 37 + 17 / 37 + 0 / 64 + 128: 8x256 0.506 / 0.635 / 0.448, 4x128
0.533 / 0.640 / -, 4x256 0.391 / 0.466 / 0.354, 8x128 0.426 / 0.505 / 0.381; under k = 4 0.585 (4x128) and 0.576 (8x256), baked
0.639 and 0.650.  Gain 100, eps 1e-2, rays that stop / packets that stop entirely / rays decided: 4x128 0.545 / 0.22 / 0.999,
8x256 0.266 / 0.18 / 0.999 (64 + 128: 0.244 / 0.18 / 1.000), 4x256 0.825 / 0.54 / 0.999, 8x128 0.632 / 0.20 / 0.998; the packets
plan's own scenes 0.896 (4x128, 0.385 of the groups of 128 stop) and 0.936 (8x128, 0.615).  Occupancy at 37 + 0, 4x128: hollow 0.640,
every lane masked 0.298, mixed 0.325, hollow and mixed 0.191, the vote must say no 0.049, iterations skipped 0.077, rays decided
0.859 (8x256: 0.635, 0.298, 0.325, 0.189, 0.043, 0.077, 0.859).  NaN-head scenes, hollow share / finite rays: terminating 0.788 /
0.020 (4x128) and 0.877 / 0.140 (8x256), 0.086 and 0.084 of the rays stop; occupancy 0.852 / 0.122 and 0.799 / 0.098; sharing 0.868 /
0.080 and 0.877 / 0.140.  Parity under termination: at most 1.6e-7 in rgb, 1.4e-6 in depth, 1.5e-7 in acc on decided rays.
"""
import pytest
import torch

import nwe_amd
from tests import hollow_domain as H
from tests import shared_coarse as SC
from tests.test_gpu_early_termination import TOL, TOL_X1

pytestmark = pytest.mark.gpu

LEAN = ("rgb", "depth", "acc")
FLAGS_KEPT = 0x7                     # fine rgb / depth / acc: the bits a lean frame and a full frame share whatever else is asked for
PRECISIONS = ("f16x3", "f16x1")
SHAPES = sorted(H.SHAPES)


def _renderer(sd_c, sd_f, sampling):
    r = nwe_amd.Renderer(0)
    sd0, sd1 = H.slots(sd_c, sd_f, sampling)
    r.set_network(0, sd0)
    r.set_network(1, sd1)
    r.set_sampling(*sampling)
    return r


def _resample(r, sd_c, sd_f, sampling):
    sd0, _ = H.slots(sd_c, sd_f, sampling)
    r.set_network(0, sd0)
    r.set_sampling(*sampling)


def _rows(r, precision="f16x3", outputs=LEAN, rows=H.ROWS):
    return r.render(H.pose(), H.SIZE, H.SIZE, rows=rows, precision=precision, outputs=outputs, **H.camera())


def _full(r, precision="f16x3", rows=H.ROWS, extra=()):
    """The FULL instantiation of the call, and its sigma [rays, samples] in the pass that produces the outputs."""
    raw = "raw_fine" if r.n_importance > 0 else "raw_coarse"
    out = _rows(r, precision, LEAN + (raw,) + tuple(extra), rows)
    return out, out[raw][..., 3].cpu()


def _share(sigma, ctx):
    """The cap of every test, from the reference's own sigma."""
    share = H.hollow_share(sigma)
    print(*ctx, "hollow share %.3f" % share)
    assert H.in_cap(share), (ctx, share)
    return share


def _same(a, b, ctx, keys=LEAN, flags="all"):
    for k in keys:
        assert torch.equal(a[k], b[k]), (ctx, k)
    fa, fb = int(a["flags"].item()), int(b["flags"].item())
    if flags == "all":
        assert fa == fb, (ctx, hex(fa), hex(fb))
    elif flags == "kept":
        assert fa & FLAGS_KEPT == fb & FLAGS_KEPT, (ctx, hex(fa), hex(fb))


def _on_off(r, precision, ctx, rows=H.ROWS, evaluations=False):
    """The lean frame with the path on, held to the frame with the path off and to a second render with it on."""
    r.debug_set_colour_skip(0)
    off = _rows(r, precision, rows=rows)
    ev_off = r.last_ray_evaluations()
    r.debug_set_colour_skip(1)
    on = _rows(r, precision, rows=rows)
    ev_on = r.last_ray_evaluations()
    _same(on, off, ctx + ("on vs off",))
    _same(_rows(r, precision, rows=rows), on, ctx + ("on again",))
    if evaluations:
        assert ev_on == ev_off, (ctx, ev_on, ev_off)
    return on, ev_on


def _finite(out):
    return torch.isfinite(out["rgb"]).all(dim=1).cpu()


def _both_occur(got, want, decided, ctx):
    print(*ctx, "decided %.3f, finite rgb on %.3f of them" % (float(decided.float().mean()), float(want[decided].float().mean())))
    assert torch.equal(got[decided], want[decided]), ctx
    assert bool(want[decided].any()) and not bool(want[decided].all()), ctx


# ---- the plain kernels of 4x256 and 8x128 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["4x256", "8x128"])
def test_plain_lean_equals_full_and_on_equals_off(shape):
    """tests/test_gpu_colour_skip.py: test_lean_equals_full_and_mode_1_equals_mode_0 at the two shapes it leaves out: 37 + 17,
    37 + 0 and 64 + 128, decompositions 0 / 1 / 2, both precisions."""
    sd_c, sd_f = H.nets(shape)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        for sampling in (H.RAGGED, H.SINGLE, H.LONG):
            _resample(r, sd_c, sd_f, sampling)
            for precision in PRECISIONS:
                r.debug_set_decomposition(0)
                full, sigma = _full(r, precision)
                _share(sigma, (shape, sampling, precision))
                for mode in (0, 1, 2):
                    r.debug_set_decomposition(mode)
                    ctx = (shape, sampling, precision, mode)
                    r.debug_set_colour_skip(1)
                    on = _rows(r, precision)
                    r.debug_set_colour_skip(0)
                    off = _rows(r, precision)
                    _same(on, full, ctx, flags="kept")
                    _same(on, off, ctx, flags="kept")
    finally:
        r.close()


# ---- the terminating kernels ----------------------------------------------------------------------------------------------------

def _term_figures(full, r_dirs, eps=H.EPS):
    return H.term_figures(full["raw_fine"], full["z_fine"], r_dirs, eps)


def _dirs(r):
    return r.create_rays(H.pose(), H.SIZE, H.SIZE, rows=H.ROWS, **H.camera())[:, 3:6].cpu()


def _executed(fig, mode, ns, ran, whole, ctx, exit_runs):
    """The evaluations executed lie in the interval the GPU's own stop indices give; exit_runs: some workgroup of the
    decomposition stops entirely, so the count is strictly below the full one - the loop exit ran."""
    lo, hi, count = H.executed_interval(fig, mode, ns)
    print(*ctx, f"executed {ran} of {whole}, interval [{lo}, {hi}]")
    assert whole == count and lo <= ran <= hi, (ctx, ran, whole, lo, hi)
    if exit_runs:
        assert hi < whole and ran < whole, (ctx, ran, whole, hi)


@pytest.mark.parametrize("shape", SHAPES)
def test_terminating_on_equals_off(shape):
    """Gain 100, eps = 1e-2: rays stop, whole packets stop, whole packets do not.  The frame with the path on is the frame with
    it off in rgb, depth, acc and the flag word, and a second render repeats the first.  The evaluations executed are equal, lie in
    the interval the GPU's own stop indices give and are below the full count - the loop exit ran - under the sample split at every
    shape and under the packets plan at 4x256 and 8x256; at 4x128 and 8x128 every group of 128 rays of this scene holds a ray that
    never stops, the packets plan executes everything (145 600 of 145 600, as the interval says) and its exit has the test below.
    Both precisions, decompositions 0 / 1; 64 + 128 as well at 8x256."""
    r = None
    try:
        for sampling in (H.RAGGED,) + ((H.LONG,) if shape == "8x256" else ()):
            sd_c, sd_f = H.nets(shape, sampling, H.GAIN)
            if r is None:
                r = _renderer(sd_c, sd_f, sampling)
                dirs = _dirs(r)
            else:
                _resample(r, sd_c, sd_f, sampling)
            for precision in PRECISIONS:
                r.set_early_termination(0.0)
                r.debug_set_decomposition(0)
                full, sigma = _full(r, precision, extra=("z_fine",))
                _share(sigma, (shape, sampling, precision))
                fig = _term_figures(full, dirs)
                print(shape, sampling, precision, "rays that stop %.3f, packets in which every ray stops %.3f, decided %.3f"
                      % (fig["stop"], fig["packets_all_stop"], fig["decided"]))
                assert H.term_conditions(fig), (shape, sampling, precision, fig["stop"], fig["packets_all_stop"], fig["decided"])
                r.set_early_termination(H.EPS)
                for mode in (0, 1):
                    r.debug_set_decomposition(mode)
                    _, (ran, whole) = _on_off(r, precision, (shape, sampling, precision, mode), evaluations=True)
                    _executed(fig, mode, sampling[0], ran, whole, (shape, sampling, precision, mode),
                              exit_runs=mode == 1 or shape not in H.TERM_GROUP_SHIFT)
    finally:
        if r is not None:
            r.close()


@pytest.mark.parametrize("shape", sorted(H.TERM_GROUP_SHIFT))
def test_terminating_packets_plan_leaves_its_loop_at_the_narrow_shapes(shape):
    """The scene with more density (tests/hollow_domain.py: TERM_GROUP_SHIFT): whole groups of 128 rays stop, so the packets plan's
    exit runs next to hollow waves at these two shapes as well.  On = off as above, executed below the full count."""
    sd_c, sd_f = H.nets(shape, H.RAGGED, H.GAIN, shift=H.TERM_GROUP_SHIFT[shape])
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        dirs = _dirs(r)
        r.debug_set_decomposition(0)
        for precision in PRECISIONS:
            r.set_early_termination(0.0)
            full, sigma = _full(r, precision, extra=("z_fine",))
            _share(sigma, (shape, precision, "shift", H.TERM_GROUP_SHIFT[shape]))
            fig = _term_figures(full, dirs)
            print(shape, precision, "rays that stop %.3f, groups of 128 in which every ray stops %.3f, decided %.3f"
                  % (fig["stop"], H.groups_that_stop(fig, 0), fig["decided"]))
            assert H.group_conditions(fig), (shape, precision, fig["stop"], H.groups_that_stop(fig, 0), fig["decided"])
            r.set_early_termination(H.EPS)
            _, (ran, whole) = _on_off(r, precision, (shape, precision), evaluations=True)
            _executed(fig, 0, H.RAGGED[0], ran, whole, (shape, precision), exit_runs=True)
    finally:
        r.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_terminating_kernel_with_nothing_to_stop_gives_the_plain_full_bits(shape):
    """Gain 1 and half the smallest transmittance of the scene, computed from the FULL frame's own raw_fine and z_fine as
    tests/test_hollow_domain_host.py computes it from the oracle's: no ray stops and every ray is decided, so the terminating
    kernel with the path on gives the bits of the plain FULL instantiation."""
    sd_c, sd_f = H.nets(shape)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        dirs = _dirs(r)
        for precision in PRECISIONS:
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                r.set_early_termination(0.0)
                full, sigma = _full(r, precision, extra=("z_fine",))
                if mode == 0:
                    _share(sigma, (shape, precision))
                    eps = 0.5 * _term_figures(full, dirs)["min_trans"]
                    assert H.EPS < eps < 1.0, (shape, precision, eps)
                    fig = _term_figures(full, dirs, eps)
                    print(shape, precision, "eps %.3f, smallest transmittance %.4f" % (eps, fig["min_trans"]))
                    assert fig["stop"] == 0.0 and fig["decided"] == 1.0, (shape, precision, fig["stop"], fig["min_trans"])
                r.set_early_termination(eps)
                on, (ran, whole) = _on_off(r, precision, (shape, precision, mode), evaluations=True)
                assert ran == whole
                _same(on, full, (shape, precision, mode, "vs plain FULL"), flags="kept")
    finally:
        r.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_terminating_parity_with_the_masked_reference(shape):
    """eps = 1e-2: on decided rays the frame with the path on agrees with the fp64 masked reference fed the GPU's own FULL
    raw_fine, z_fine and ray directions, at the tolerances of tests/test_gpu_early_termination.py."""
    sd_c, sd_f = H.nets(shape, H.RAGGED, H.GAIN)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        dirs = _dirs(r)
        for precision in PRECISIONS:
            tol = TOL_X1 if precision == "f16x1" else TOL
            r.set_early_termination(0.0)
            r.debug_set_decomposition(0)
            full, sigma = _full(r, precision, extra=("z_fine",))
            _share(sigma, (shape, precision))
            fig = _term_figures(full, dirs)
            assert H.term_conditions(fig), (shape, precision, fig["stop"], fig["packets_all_stop"], fig["decided"])
            ref, decided = fig["masked"], fig["masked"]["decided"]
            r.set_early_termination(H.EPS)
            r.debug_set_colour_skip(1)
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                out = _rows(r, precision)
                for k in LEAN:
                    err = (out[k].cpu().double() - ref[k]).abs()
                    err = err.max(dim=-1).values if err.dim() == 2 else err
                    worst = float(err[decided].max())
                    print(f"{shape} {precision} mode {mode} {k}: max err on decided rays {worst:.2e} (tol {tol[k]:.0e})")
                    assert worst <= tol[k], (shape, precision, mode, k)
    finally:
        r.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_terminating_path_runs_exactly_where_predicted(shape):
    """A NaN in the fine rgb head under mode 2: accumulate_above masks with selects, so on decided rays rgb is finite if and only
    if the ray's packet is hollow at every sample in front of the ray's own stop index.  Both values occur; depth and acc are
    the path-off frame's.  The scene has its own shift and asks only that some rays stop (tests/hollow_domain.py: NAN_SHIFT says
    why).  What this proves is less than the prediction says: a ray that stops had density in front of its stop index, so every
    ray with stop < S is NaN already and "in front of the ray's own stop index" never decides a ray - the test shows "finite if
    and only if the packet is hollow at every sample" in the terminating kernel, next to rays that are masked from their stop on."""
    shift = H.NAN_SHIFT["term", shape]
    sd_c, sd_f = H.nets(shape, H.RAGGED, H.GAIN, nan_head=True, shift=shift)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        assert not r.packed_colour_finite(1) and r.packed_colour_finite(0)
        dirs = _dirs(r)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            r.set_early_termination(0.0)
            full, sigma = _full(r, extra=("z_fine",))
            assert torch.isnan(full["rgb"]).any(dim=1).all()
            _share(sigma, (shape, mode, "shift", shift))
            fig = _term_figures(full, dirs)
            print(shape, mode, "rays that stop %.3f" % fig["stop"])
            assert fig["stop"] >= 0.01 and fig["decided"] >= 0.95, (shape, mode, fig["stop"], fig["decided"])
            want = H.finite_under_termination(sigma, fig["masked"]["stop"])
            r.set_early_termination(H.EPS)
            r.debug_set_colour_skip(0)
            off = _rows(r)
            assert not _finite(off).any()
            r.debug_set_colour_skip(2)
            hook = _rows(r)
            _both_occur(_finite(hook), want, fig["masked"]["decided"], (shape, mode))
            _same(hook, off, (shape, mode), keys=("depth", "acc"), flags=None)
    finally:
        r.close()


# ---- the occupancy kernels --------------------------------------------------------------------------------------------------------

def _set_grid(r, g):
    r.set_occupancy(g["bits"], g["lo"], g["hi"], g["res"])


def _cells(plain, ns, g):
    rays = plain.create_rays(H.pose(), H.SIZE, H.SIZE, rows=H.ROWS, **H.camera())
    empty, decided = H.cells(rays.cpu().numpy(), ns, g)
    return rays, empty, torch.from_numpy(decided)


@pytest.mark.parametrize("shape", SHAPES)
def test_occupancy_on_equals_off(shape):
    """The checkerboard at 37 + 17 and 37 + 0, at 8x256 at 64 + 128 as well (48 iterations of the sample split, 192 of the packets
    plan): on = off in rgb, depth, acc, the flag word and the evaluations the grid left, which are fewer than all.  Both
    precisions, decompositions 0 / 1."""
    g = H.occupancy_grid()
    sd_c, sd_f = H.nets(shape)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        for sampling in (H.RAGGED, H.SINGLE) + ((H.LONG,) if shape == "8x256" else ()):
            _resample(r, sd_c, sd_f, sampling)        # clears the grid
            for precision in PRECISIONS:
                r.debug_set_decomposition(0)
                _, sigma = _full(r, precision)
                _share(sigma, (shape, sampling, precision))
            _set_grid(r, g)
            for precision in PRECISIONS:
                for mode in (0, 1):
                    r.debug_set_decomposition(mode)
                    _, (ran, whole) = _on_off(r, precision, (shape, sampling, precision, mode), evaluations=True)
                    assert 0 < ran < whole, (shape, sampling, precision, mode, ran, whole)
    finally:
        r.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_occupancy_kernel_with_all_bits_set_gives_the_plain_full_bits(shape):
    sd_c, sd_f = H.nets(shape)
    r, plain = _renderer(sd_c, sd_f, H.RAGGED), _renderer(sd_c, sd_f, H.RAGGED)
    try:
        _set_grid(r, H.occupancy_grid(full=True))
        for precision in PRECISIONS:
            for mode in (0, 1):
                r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
                full, sigma = _full(plain, precision)
                if mode == 0:
                    _share(sigma, (shape, precision))
                on, (ran, whole) = _on_off(r, precision, (shape, precision, mode), evaluations=True)
                assert ran == whole
                _same(on, full, (shape, precision, mode, "vs plain FULL"), flags="kept")
    finally:
        r.close(); plain.close()


def _occupancy_shares(sigma, empty, decided, ctx):
    shares = H.occupancy_shares(sigma, empty)
    print(*ctx, " ".join(f"{k} {shares[k]:.3f}" for k in H.OCC_SHARES), "rays decided %.3f" % float(decided.float().mean()))
    assert all(shares[k] > 0.01 for k in H.OCC_SHARES) and H.in_cap(shares["hollow"]), (ctx, shares)
    assert float(decided.float().mean()) >= 0.8, ctx


@pytest.mark.parametrize("shape", H.PAIR)
def test_occupancy_frame_is_the_composite_of_the_masked_full_raw(shape):
    """37 + 0, f16x3: the plain FULL frame's raw_coarse with all four channels of the empty-cell samples zeroed, composited by
    render_rays(precision="f32", debug_raw=...) on a context without a grid.  On decided rays the occupancy frame with the path on
    equals it in rgb, depth and acc: a hollow wave's colour 0 and the full path's finite colour under weight 0 give the same sums."""
    g = H.occupancy_grid()
    sd_c, sd_f = H.nets(shape, H.SINGLE)
    r, plain = _renderer(sd_c, sd_f, H.SINGLE), _renderer(sd_c, sd_f, H.SINGLE)
    try:
        _set_grid(r, g)
        rays, empty, decided = _cells(plain, H.SINGLE[0], g)
        full, sigma = _full(plain)
        _occupancy_shares(sigma, empty, decided, (shape,))
        ref = plain.render_rays(rays, precision="f32", outputs=LEAN, debug_raw=(H.masked_raw(full["raw_coarse"], empty), None))
        dec = decided.to(ref["rgb"].device)
        r.debug_set_colour_skip(1)
        for mode in (0, 1):
            r.debug_set_decomposition(mode)
            on = _rows(r)
            for k in LEAN:
                assert torch.equal(on[k][dec], ref[k][dec]), (shape, mode, k)
            assert float(on["acc"].max()) > 0.05
    finally:
        r.close(); plain.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_occupancy_path_runs_exactly_where_predicted(shape):
    """A NaN in the rgb head under mode 2, 37 + 0: on decided rays rgb is finite if and only if, at every sample, the ray's lane is
    masked or the packet is hollow by the network's sigma over all 32 lanes, masked ones included.  Both values occur; depth and
    acc are the path-off frame's."""
    g = H.occupancy_grid()
    shift = H.NAN_SHIFT["occ", shape]
    sd_c, sd_f = H.nets(shape, H.SINGLE, nan_head=True, shift=shift)
    r, plain = _renderer(sd_c, sd_f, H.SINGLE), _renderer(sd_c, sd_f, H.SINGLE)
    try:
        assert not r.packed_colour_finite(0)
        _set_grid(r, g)
        _, empty, decided = _cells(plain, H.SINGLE[0], g)
        for mode in (0, 1):
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            full, sigma = _full(plain)
            assert torch.isnan(full["rgb"]).any(dim=1).all()
            _share(sigma, (shape, mode, "shift", shift))
            want = H.finite_under_occupancy(sigma, empty)
            r.debug_set_colour_skip(0)
            off = _rows(r)
            r.debug_set_colour_skip(2)
            hook = _rows(r)
            _both_occur(_finite(hook), want, decided, (shape, mode))
            _same(hook, off, (shape, mode), keys=("depth", "acc"), flags=None)
            # with the path off a ray is finite only where the grid masks its every sample
            assert torch.equal(_finite(off)[decided], torch.from_numpy(empty).all(dim=1)[decided]), (shape, mode)
    finally:
        r.close(); plain.close()


# ---- the sharing consumer kernels ---------------------------------------------------------------------------------------------

def _bake(r, precision="f16x3"):
    r.bake_coarse_grid(H.OCC_LO, H.OCC_HI, H.OCC_RES, precision=precision)


@pytest.mark.parametrize("shape", SHAPES)
def test_sharing_on_equals_off(shape):
    """Separate passes at k = 1, the shared coarse pass at k = 4 and the baked coarse pass: on = off in rgb, depth, acc and the
    flag word.  Both precisions, decompositions 0 / 1; at 8x256 at 64 + 128 as well.  That the sharing launches ran is read from
    what include/nwe.h says they report: the coarse launch's rays (the call's, or its representatives) and the evaluations
    executed (all; the representatives' coarse pass and every ray's fine pass; the fine pass alone).  The separate-passes frame
    is also the plain FULL fused frame of the same call, at every shape; the hollow share is that frame's."""
    sd_c, sd_f = H.nets(shape)
    r = _renderer(sd_c, sd_f, H.RAGGED)
    try:
        for sampling in (H.RAGGED,) + ((H.LONG,) if shape == "8x256" else ()):
            ns, ni = sampling
            r.set_separate_passes(False)
            r.set_shared_coarse(1)
            _resample(r, sd_c, sd_f, sampling)        # clears the baked grid
            assert r.coarse_grid is None
            fulls = {}
            for precision in PRECISIONS:
                r.debug_set_decomposition(0)
                fulls[precision], sigma = _full(r, precision)
                _share(sigma, (shape, sampling, precision))
            for name, rows in (("separate", H.ROWS), ("shared", H.SHARED_ROWS), ("baked", H.ROWS)):
                if name == "separate":
                    r.set_separate_passes(True)
                elif name == "shared":
                    r.set_separate_passes(False)
                    r.set_shared_coarse(H.SHARED_K)
                else:
                    r.set_shared_coarse(1)
                    _bake(r)
                assert (r.separate_passes, r.shared_coarse, r.coarse_grid is not None) == \
                    {"separate": (True, 1, False), "shared": (False, H.SHARED_K, False), "baked": (False, 1, True)}[name]
                n = (rows[1] - rows[0]) * H.SIZE
                whole = n * (2 * ns + ni)
                launched, evaluated = {
                    "separate": (n, (whole, whole)),
                    "shared": (SC.n_rep(H.SIZE, H.SIZE, H.SHARED_K, rows[0], rows[1], 1),
                               SC.evaluations(H.SIZE, H.SIZE, H.SHARED_K, rows[0], rows[1], 1, ns, ni)),
                    "baked": (n, (n * (ns + ni), whole)),
                }[name]
                for precision in PRECISIONS:
                    for mode in (0, 1):
                        r.debug_set_decomposition(mode)
                        ctx = (shape, sampling, name, precision, mode)
                        on, ran = _on_off(r, precision, ctx, rows=rows)
                        coarse = r.last_coarse_launch()
                        assert coarse is not None and coarse[1] == launched and ran == evaluated, (ctx, coarse, launched, ran, evaluated)
                        assert float(on["acc"].max()) > 0.05
                        if name == "separate":
                            _same(on, fulls[precision], ctx + ("vs plain FULL",), flags="kept")
    finally:
        r.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_separate_passes_with_the_path_on_give_the_plain_full_fused_bits(shape):
    """include/nwe.h: with two networks of one shape every output of separate passes is the fused call's."""
    sd_c, sd_f = H.nets(shape)
    r, plain = _renderer(sd_c, sd_f, H.RAGGED), _renderer(sd_c, sd_f, H.RAGGED)
    try:
        r.set_separate_passes(True)
        r.debug_set_colour_skip(1)
        for precision in PRECISIONS:
            for mode in (0, 1):
                r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
                full, sigma = _full(plain, precision)
                if mode == 0:
                    _share(sigma, (shape, precision))
                on = _rows(r, precision)
                assert r.last_coarse_launch() is not None
                _same(on, full, (shape, precision, mode), flags="kept")
    finally:
        r.close(); plain.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_sharing_path_runs_exactly_where_predicted(shape):
    """A NaN in the fine rgb head under mode 2 and separate passes at k = 1: rgb is finite if and only if the ray's packet is hollow
    at every fine sample by the FULL frame's raw_fine.  Both values occur; depth and acc are the FULL frame's."""
    shift = H.NAN_SHIFT["share", shape]
    sd_c, sd_f = H.nets(shape, H.RAGGED, nan_head=True, shift=shift)
    r, plain = _renderer(sd_c, sd_f, H.RAGGED), _renderer(sd_c, sd_f, H.RAGGED)
    try:
        assert not r.packed_colour_finite(1) and r.packed_colour_finite(0)
        r.set_separate_passes(True)
        for mode in (0, 1):
            r.debug_set_decomposition(mode); plain.debug_set_decomposition(mode)
            full, sigma = _full(plain)
            assert torch.isnan(full["rgb"]).any(dim=1).all()
            _share(sigma, (shape, mode, "shift", shift))
            want = H.hollow(sigma).all(dim=1).repeat_interleave(32)[:sigma.shape[0]]
            r.debug_set_colour_skip(2)
            hook = _rows(r)
            _both_occur(_finite(hook), want, torch.ones_like(want), (shape, mode))
            _same(hook, full, (shape, mode), keys=("depth", "acc"), flags=None)
            r.debug_set_colour_skip(1)                       # the pack-time guard keeps every evaluation on the full path
            guarded = _rows(r)
            assert torch.isnan(guarded["rgb"]).any(dim=1).all(), (shape, mode)
    finally:
        r.close(); plain.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_shared_coarse_frame_is_the_full_call_fed_the_representatives_weights(shape):
    """k = 4 on rows [400, 404): the frame with the path on equals, in rgb, depth and acc, a plain context's FULL render_rays on the
    call's rays with debug_coarse_weights = the FULL frame's weights_coarse of every ray's representative
    (tests/shared_coarse.py), rendered over the row that holds them.  The hollow share is that reference call's own."""
    sd_c, sd_f = H.nets(shape)
    r, plain = _renderer(sd_c, sd_f, H.RAGGED), _renderer(sd_c, sd_f, H.RAGGED)
    try:
        r.set_shared_coarse(H.SHARED_K)
        r.debug_set_colour_skip(1)
        rep_rows, rep = H.representatives()
        rays = plain.create_rays(H.pose(), H.SIZE, H.SIZE, rows=H.SHARED_ROWS, **H.camera())
        for precision in PRECISIONS:
            weights = _rows(plain, precision, LEAN + ("weights_coarse",), rep_rows)["weights_coarse"][torch.from_numpy(rep).to(rays.device)]
            ref = plain.render_rays(rays, precision=precision, outputs=LEAN + ("raw_fine",), debug_coarse_weights=weights)
            _share(ref["raw_fine"][..., 3].cpu(), (shape, precision, "k", H.SHARED_K))
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                on = _rows(r, precision, rows=H.SHARED_ROWS)
                _same(on, ref, (shape, precision, mode), flags=None)
    finally:
        r.close(); plain.close()


@pytest.mark.parametrize("shape", H.PAIR)
def test_baked_coarse_frame_is_the_full_call_fed_the_grids_weights(shape):
    """A 16^3 grid of the coarse network's sigma over the occupancy box: the frame with the path on equals, in rgb, depth and acc,
    a plain context's FULL render_rays fed coarse_grid_weights' weights.  The hollow share is that reference call's own."""
    sd_c, sd_f = H.nets(shape)
    r, plain = _renderer(sd_c, sd_f, H.RAGGED), _renderer(sd_c, sd_f, H.RAGGED)
    try:
        _bake(r)
        r.debug_set_colour_skip(1)
        rays = plain.create_rays(H.pose(), H.SIZE, H.SIZE, rows=H.ROWS, **H.camera())
        weights = r.coarse_grid_weights(H.pose(), H.SIZE, H.SIZE, rows=H.ROWS, outputs=("weights",), **H.camera())["weights"]
        for precision in PRECISIONS:
            ref = plain.render_rays(rays, precision=precision, outputs=LEAN + ("raw_fine",), debug_coarse_weights=weights)
            _share(ref["raw_fine"][..., 3].cpu(), (shape, precision, "baked"))
            for mode in (0, 1):
                r.debug_set_decomposition(mode)
                on = _rows(r, precision)
                _same(on, ref, (shape, precision, mode), flags=None)
    finally:
        r.close(); plain.close()
