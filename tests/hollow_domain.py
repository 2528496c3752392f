"""The scenes, predictions and helpers of the hollow path's tests in the terminating, occupancy and sharing kernels
(csrc/nwe_mfma_eval.h: mlp_eval, CSKIP; tests/test_gpu_hollow_variants.py, tests/test_hollow_domain_host.py).  No GPU here.

The scene is that of tests/test_gpu_colour_skip.py: rows [400, 402) of the 800 x 800 frame under bench.sweep_pose(0, 1), near 0.1,
far 10 - 1600 coherent rays, 50 packets, 12 1/2 workgroups of four packets.  The networks are the raw random ones with the fine
network's density bias lowered by a SHIFT per shape, so that between a tenth and nine tenths of the (packet, sample) pairs are
hollow; without importance samples the fine network sits in slot 0.  Under GAIN the density head is multiplied by a positive
number: the sign of sigma, and so the hollow set, stays, and rays end.

Every helper that predicts something takes the sigma, depths and cells it predicts from as arguments: the host test feeds the
oracle's, the GPU tests the GPU's own FULL instantiation of the same call, which never takes the path.
"""
import functools

import numpy as np
import torch

import bench
from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import coarse_grid as B
from tests import early_termination as E
from tests import occupancy as G
from tests import shared_coarse as SC

NEAR, FAR = 0.1, 10.0
SIZE, ROWS = 800, (400, 402)
FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = {"8x256": (8, 256), "4x128": (4, 128), "4x256": (4, 256), "8x128": (8, 128)}
PAIR = ("4x128", "8x256")              # the shapes of the parity, NaN-head and reference-fed tests
RAGGED, SINGLE, LONG = (37, 17), (37, 0), (64, 128)   # 37: no multiple of 4, the sample-split plan's last iteration is ragged
CAP = (0.1, 0.9)                       # the hollow share of every call, from the reference's own sigma

# The amount the fine network's _alpha_linear.bias is lowered by, per shape; a (shape, sampling) entry overrides the shape's.
# Behind each: the hollow (packet, sample) share of the fp32 oracle at 37 + 17 / 37 + 0 / 64 + 128 (tests/test_hollow_domain_host.py
# prints them and holds every one the GPU file uses to CAP).
SHIFT = {
    "8x256": 0.0,      # 0.506 / 0.635 / 0.448
    "4x128": 0.3,      # 0.533 / 0.640 / - (no test runs 64 + 128 at this shape)
    "4x256": 0.1,      # 0.391 / 0.466 / 0.354
    "8x128": 0.1,      # 0.426 / 0.505 / 0.381
}

# The NaN-head tests need rays whose packet is hollow at EVERY sample that counts for them, next to rays for which it is not.
# Under the shifts above no packet is (the oracle: 0.000 of the rays at 8x256, at most 0.004 at 4x128), so these tests lower the
# bias further, per variant.  A ray that stops had density at a sample in front of its stop index, where its packet was not
# hollow: every ray with a finite rgb is one that never stops, so a scene cannot have finite rays AND meet term_conditions'
# packets that stop entirely (the oracle at every shift between: either no packet stops or no ray is finite).  The terminating NaN-
# head test therefore asks what it can: some rays stop, both values occur.  Behind each: the oracle's hollow share, the share
# of decided rays with a finite rgb, and under termination the rays that stop.
NAN_SHIFT = {
    ("term", "4x128"): 0.37,     # 0.788, 0.020, stop 0.086
    ("term", "8x256"): 0.10,     # 0.877, 0.140, stop 0.084
    ("occ", "4x128"): 0.37,      # 0.852, 0.122
    ("occ", "8x256"): 0.05,      # 0.799, 0.098
    ("share", "4x128"): 0.40,    # 0.868, 0.080
    ("share", "8x256"): 0.10,    # 0.877, 0.140
}

# Early termination: the gain on the fine network's density head, and the threshold of the tests.
GAIN, EPS = 100.0, 1e-2
# At gain 1 the networks are thin: term_figures' "min_trans", the smallest transmittance in front of any sample, is 0.58 to
# 0.76 (tests/test_hollow_domain_host.py computes it per shape), and at half of it - the GPU test takes half of the minimum of
# its own FULL raw_fine - the terminating kernel masks nothing.
# A workgroup leaves its loop once ALL its rays are below eps: 32 rays under the sample split, 128 under the packets plan.  At
# 4x128 and 8x128 every group of 128 rays of the scene holds a ray that never stops (the oracle: the packets plan executes all
# 145 600 evaluations), so there the packets plan's exit gets a scene of its own with more density.  Behind each: the oracle's
# hollow share, rays that stop, and the evaluations the packets plan executes at most, of 145 600.
TERM_GROUP_SHIFT = {
    "4x128": 0.25,     # 0.306, 0.896, 137 472
    "8x128": 0.05,     # 0.262, 0.936, 136 576
}
TERM_GROUPS = {0: (128, 1), 1: (32, 4)}     # decomposition -> (rays of a workgroup, samples of an iteration)
TERM_LAG = 1                                # iterations a workgroup may run past its last ray's stop (tests/test_gpu_early_termination.py)

# The occupancy grid: a checkerboard of single cells of 1.375 units over a box that the longest rays leave near their far end
# (outside it every sample is evaluated).
OCC_LO, OCC_HI, OCC_RES = (-11.0, -11.0, -11.0), (11.0, 11.0, 11.0), (16, 16, 16)
OCC_SHARES = ("hollow", "all_masked", "mixed", "hollow_and_mixed", "vote_must_say_no", "iterations_skipped")

# The sharing kernels at k > 1: k = 4 on rows [400, 404), a whole row of blocks.
SHARED_K, SHARED_ROWS = 4, (400, 404)


def shift_of(shape, sampling=RAGGED):
    return SHIFT.get((shape, tuple(sampling)), SHIFT[shape])


def nets(shape, sampling=RAGGED, gain=1.0, nan_head=False, shift=None):
    """(coarse, fine) of a shape: make_state_dict(1000 / 1001), the fine density bias lowered by the shift, then the fine
    density head (weights and the lowered bias) multiplied by `gain`; nan_head plants a NaN in the fine rgb head."""
    D, W = SHAPES[shape]
    sd_c, sd_f = synthetic.make_state_dict(1000, D, W), synthetic.make_state_dict(1001, D, W)
    shift = shift_of(shape, sampling) if shift is None else shift
    bias = (sd_f["_alpha_linear.bias"] - np.float32(shift)).astype(np.float32)
    sd_f["_alpha_linear.bias"] = (bias * np.float32(gain)).astype(np.float32)
    sd_f["_alpha_linear.weight"] = (sd_f["_alpha_linear.weight"] * np.float32(gain)).astype(np.float32)
    if nan_head:
        sd_f["_rgb_linear.weight"] = sd_f["_rgb_linear.weight"].copy()
        sd_f["_rgb_linear.weight"][1, 3] = np.nan
    return sd_c, sd_f


def slots(sd_c, sd_f, sampling):
    """The networks of slots 0 and 1 of a call: without importance samples the single pass runs network 0, so the fine network
    sits there and the call has the density of the others."""
    return (sd_c if sampling[1] > 0 else sd_f), sd_f


def pose():
    return np.asarray(bench.sweep_pose(0, 1), dtype=np.float32)


def camera():
    fx, fy, cx, cy = O.intrinsics(SIZE, SIZE)
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, near=NEAR, far=FAR)


@functools.lru_cache(maxsize=None)
def oracle_rays(rows=ROWS):
    """[R, 11] of the oracle for rows of the frame, shared: leave it unchanged."""
    fx, fy, cx, cy = O.intrinsics(SIZE, SIZE)
    rays = O.create_rays(torch.from_numpy(pose())[None], SIZE, SIZE, fx, fy, cx, cy, NEAR, FAR).reshape(SIZE, SIZE, 11)
    return rays[rows[0]:rows[1]].reshape(-1, 11).contiguous()


def _tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def oracle(shape, sampling=RAGGED, gain=1.0, rows=ROWS, shift=None):
    """(raw [R, S, 4], z [R, S], d [R, 3]) of the pass that produces the outputs, from the fp32 oracle; shared: leave it unchanged."""
    sd0, sd1 = slots(*nets(shape, sampling, gain, shift=shift), sampling)
    cfg = O.RenderConfig(n_samples=sampling[0], n_importance=sampling[1])
    rays = oracle_rays(rows)
    ref = O.render_rays(rays, _tensors(sd0), _tensors(sd1) if sampling[1] > 0 else None, cfg,
                        keep=("raw_fine", "z_fine", "raw_coarse", "z_coarse"))
    raw, z = E.terminated_pass(ref, cfg)
    return raw[..., :4], z, rays[:, 3:6]


# ---- the hollow set ------------------------------------------------------------------------------------------------------------

def hollow(sigma):
    """sigma [R, S] (torch) -> [packets, S] bool: no ray of the packet has density at the sample, by mlp_eval's own test.  The
    lanes of a ragged last packet compute the call's last ray along, so they add nothing to the packet's vote.
    tests/test_gpu_colour_skip.py: _hollow is the same restatement and stays where it is, with that file's assertions: a change
    of mlp_eval's test on sigma has to reach both."""
    R, S = sigma.shape
    none = (sigma <= 0) & (sigma >= -FLT_MAX)
    pad = (-R) % 32
    if pad:
        none = torch.cat([none, none[-1:].expand(pad, S)])
    return none.view(-1, 32, S).all(dim=1)


def hollow_share(sigma):
    return float(hollow(sigma).float().mean())


def in_cap(share):
    return CAP[0] <= share <= CAP[1]


def _per_ray(per_packet, n_rays):
    return per_packet.repeat_interleave(32, dim=0)[:n_rays]


# ---- early termination ---------------------------------------------------------------------------------------------------------

def term_figures(raw, z, d, eps=EPS):
    """The fp64 masked reference (tests/early_termination.py) of raw / z / d from any source, and the shares the tests'
    conditions speak of: rays that stop, packets in which every ray stops, rays decided."""
    m = E.masked_outputs(raw.detach().cpu().double(), z.detach().cpu().double(), d.detach().cpu().double(), eps)
    R, S = z.shape
    assert R % 32 == 0
    stops = m["stop"] < S
    whole = stops.view(-1, 32).all(dim=1)
    return {"masked": m, "stop": float(stops.float().mean()), "packets_all_stop": float(whole.float().mean()),
            "decided": float(m["decided"].float().mean()), "min_trans": float(m["trans"].min())}


def term_conditions(fig):
    """The conditions of the terminating tests: between 10 % and 90 % of the rays stop, at least one packet stops entirely and
    at least one does not, at least 95 % of the rays are decided."""
    return 0.1 <= fig["stop"] <= 0.9 and 0.0 < fig["packets_all_stop"] < 1.0 and fig["decided"] >= 0.95


def executed_interval(fig, mode, n_samples):
    """[lo, hi] of the evaluations a terminated 37 + 17 style call may execute under a decomposition, from term_figures' stop
    indices (tests/early_termination.py: executed_interval), and the full count."""
    m = fig["masked"]
    R, S = m["trans"].shape
    group, per_it = TERM_GROUPS[mode]
    lo, hi = E.executed_interval(m["stop"], m["decided"], group, per_it, TERM_LAG, S, n_samples)
    return lo, hi, R * (n_samples + S)


def groups_that_stop(fig, mode):
    """The share of the decomposition's workgroups whose every ray stops in front of the last sample."""
    stop = fig["masked"]["stop"]
    S = fig["masked"]["trans"].shape[1]
    group = TERM_GROUPS[mode][0]
    stop = torch.cat([stop, torch.zeros((-len(stop)) % group, dtype=stop.dtype)])     # a ragged group's missing rays have no say
    return float((stop.view(-1, group).max(dim=1).values < S).float().mean())


def group_conditions(fig):
    """The conditions of the packets plan's own scenes: rays that never stop, groups of 128 rays that stop entirely and groups
    that do not, at least 95 % of the rays decided."""
    return 0.1 <= fig["stop"] < 1.0 and 0.0 < groups_that_stop(fig, 0) < 1.0 and fig["decided"] >= 0.95


def finite_under_termination(sigma, stop):
    """Per ray: its packet is hollow at every sample in front of the ray's own stop index - where a NaN rgb head leaves the
    ray's rgb finite, since accumulate_above masks the samples from the stop index on with selects."""
    h = hollow(sigma)
    S = h.shape[1]
    idx = torch.arange(S).expand(h.shape)
    first_full = torch.where(~h, idx, torch.full_like(idx, S)).min(dim=1).values      # the packet's first sample on the full path
    return _per_ray(first_full, sigma.shape[0]) >= stop


# ---- the occupancy grid ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def occupancy_grid(full=False):
    bits = np.ones(OCC_RES, bool) if full else G.checkerboard_bits(OCC_RES, 1)
    return G.make_grid(bits, OCC_LO, OCC_HI)


def cells(rays, n_samples, grid):
    """rays [R, >= 8] (numpy float32, the call's own) -> (empty [R, S], decided [R]) of the coarse samples by the rule's
    restatement on the fp32 points (tests/occupancy.py: classify; tests/coarse_grid.py: coarse_points)."""
    _, pts = B.coarse_points(np.asarray(rays, dtype=np.float32), n_samples)
    empty, decided = G.classify(pts, grid)
    return empty, decided.all(-1)


def occupancy_shares(sigma, empty):
    """The six shares of the issue over (packet, sample) pairs - the last over (group of 128 rays, sample) - from the
    network's sigma [R, S] (torch, masked samples included) and the cells' empty [R, S] (numpy)."""
    R, S = sigma.shape
    assert R % 32 == 0
    h = hollow(sigma).numpy()
    e = empty.reshape(-1, 32, S)
    all_m, any_m = e.all(1), e.any(1)
    mixed = any_m & ~all_m
    none = ((sigma <= 0) & (sigma >= -FLT_MAX)).numpy().reshape(-1, 32, S)
    vote_no = (none | e).all(1) & ~h & ~all_m      # the unmasked lanes have no density, a masked lane has: not hollow
    groups = np.concatenate([empty, np.ones(((-R) % 128, S), bool)]).reshape(-1, 128, S).all(1)
    return {"hollow": float(h.mean()), "all_masked": float(all_m.mean()), "mixed": float(mixed.mean()),
            "hollow_and_mixed": float((h & mixed).mean()), "vote_must_say_no": float(vote_no.mean()),
            "iterations_skipped": float(groups.mean())}


def finite_under_occupancy(sigma, empty):
    """Per ray: at every sample the ray's lane is masked or the packet is hollow by the network's sigma over all 32 lanes,
    masked ones included - where a NaN rgb head leaves the ray's rgb finite."""
    h = _per_ray(hollow(sigma), sigma.shape[0])
    return (h | torch.from_numpy(empty)).all(dim=1)


def masked_raw(raw, empty):
    """raw [R, S, 4] with all four channels of the rows of empty-cell samples replaced by zero (include/nwe.h)."""
    return torch.where(torch.from_numpy(empty).to(raw.device)[..., None], torch.zeros((), dtype=raw.dtype, device=raw.device), raw)


# ---- the sharing kernels -----------------------------------------------------------------------------------------------------------

def representatives(k=SHARED_K, rows=SHARED_ROWS):
    """(the rows of the frame that hold the representatives of a call over `rows`, per ray of the call the index of its
    representative among the rays of those rows): tests/shared_coarse.py has the rule."""
    idx = SC.rep_index(SIZE, SIZE, k, rows[0], rows[1], 1)
    r0, r1 = int(idx.min()) // SIZE, int(idx.max()) // SIZE + 1
    return (r0, r1), idx - r0 * SIZE


def oracle_fine_sigma_given_weights(shape, z_fine, rows):
    """sigma [R, S] of the fine network of a shape at caller-given fine depths: the oracle's fine pass alone."""
    _, sd_f = nets(shape)
    cfg = O.RenderConfig(n_samples=RAGGED[0], n_importance=RAGGED[1])
    out = O.fine_pass_given_depths(oracle_rays(rows), z_fine, _tensors(sd_f), cfg)
    return out["raw_fine"][..., 3]


@functools.lru_cache(maxsize=None)
def oracle_shared_sigma(shape):
    """The fine sigma of the k > 1 call by the oracle: every ray's fine pass on the depths of its representative."""
    sd_c, sd_f = nets(shape)
    cfg = O.RenderConfig(n_samples=RAGGED[0], n_importance=RAGGED[1])
    rep_rows, rep = representatives()
    ref = O.render_rays(oracle_rays(rep_rows), _tensors(sd_c), _tensors(sd_f), cfg, keep=("z_fine",))
    return oracle_fine_sigma_given_weights(shape, ref["z_fine"][torch.from_numpy(rep)], SHARED_ROWS)


@functools.lru_cache(maxsize=None)
def oracle_baked_sigma(shape):
    """The fine sigma of the baked call by the oracle: a 16^3 grid of the coarse network's sigma at the cell centres of the
    occupancy box, then tests/coarse_grid.py's composition."""
    sd_c, sd_f = nets(shape)
    cfg = O.RenderConfig(n_samples=RAGGED[0], n_importance=RAGGED[1])
    centres = torch.from_numpy(G.cell_centres(OCC_LO, OCC_HI, OCC_RES).reshape(-1, 1, 3).astype(np.float32))
    dirs = torch.tensor([[0.0, 0.0, 1.0]]).expand(centres.shape[0], 3)       # sigma does not depend on the direction
    with torch.no_grad():
        values = O.run_network(centres, dirs, _tensors(sd_c), cfg.freqs_xyz, cfg.freqs_dir, cfg.net_chunk)[..., 3]
    grid = B.make_grid(values.numpy().reshape(OCC_RES), OCC_LO, OCC_HI)
    baked = B.baked_render(oracle_rays(ROWS), sd_f, cfg, grid)
    return oracle_fine_sigma_given_weights(shape, baked["z_fine"], ROWS)
