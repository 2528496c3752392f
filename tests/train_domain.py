"""Training-mode tables (nwe_set_train_tables: t_rand, noise_coarse, noise_fine, u) and the one-shot hooks over their domain:
one table of cases shared by tests/test_train_domain_oracle.py (CPU) and tests/test_gpu_train_domain.py (GPU), like
tests/shape_domain.py, tests/input_domain.py and tests/mode_domain.py are shared by their tests.  Plain data and CPU references;
nothing here touches a GPU.

Why stage by stage: with sigma noise of unit variance on a thin-fog coarse network the noise pushes sigma across the ReLU, the
weights collapse and the inverse CDF sits on its `denom < 1e-5` switch, so the fp32 oracle ITSELF is up to 8e-2 of far from
the fp64 oracle in z_fine (tests/test_train_domain_oracle.py asserts > 1e-3) and no end-to-end tolerance both passes and means
something.  Taken stage by stage on the same inputs the two oracles agree to ~1e-6, so every comparison is per stage, each
stage fed what the kernel itself produced for the stage before it:

  stage A  coarse   rays, t_rand, noise_coarse                     -> z_coarse, raw_coarse, weights_coarse, rgb / depth / acc
  stage B  sampler  z_coarse (fp32), weights_coarse [R, ns], u      -> z_fine (sorted union), z_std
  stage C  fine     rays, z_fine, noise_fine                        -> raw_fine, rgb, depth, acc

A hook replaces its stage and nothing else (include/nwe.h); `raw=` below is nwe_debug_set_raw, stage B's `weights` argument is
nwe_debug_set_coarse_weights, stage C's `z_fine` argument nwe_debug_set_fine_depths.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from nwe_amd import synthetic
from oracle import nerf_oracle as O
from tests import shape_domain as SD

NEAR, FAR = 0.1, 10.0
N_RAYS = 165                     # 128 + 32 + 5: a full packets workgroup, a full packet, a ragged one; ten 16-ray workgroups + 5
FRAME_H, FRAME_W = 12, 16
F32, F64 = torch.float32, torch.float64
ONE_BELOW = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
K_PACKET_MAX_SAMPLES = 64        # nwe_mfma_config.h: above it the launcher forces the sample split
UNDECIDED = 1e-5                 # of far: a ray whose fp32 and fp64 stage-B depths differ by more is left out of stage B
UNDECIDED_CAP = 0.10             # of a case's rays

TABLES = ("t_rand", "noise_coarse", "noise_fine", "u")
ALL4 = TABLES
SUBSETS: Tuple[Tuple[str, ...], ...] = (("t_rand",), ("noise_coarse",), ("noise_fine",), ("u",), ALL4, ("t_rand", "u"),
                                        ("noise_coarse", "noise_fine"))
SUBSETS_NI0: Tuple[Tuple[str, ...], ...] = (("t_rand",), ("noise_coarse",), ("t_rand", "noise_coarse"))

SAMPLINGS: Tuple[Tuple[int, int], ...] = (
    (3, 1),      # the smallest with importance samples
    (5, 3),
    (7, 6),      # Stot 7 and 13: no multiples of 4, the tail of the sample split runs in both passes
    (16, 24),
    (9, 0),      # one pass: noise_fine and u have no meaning
    (65, 7),     # above kPacketMaxSamples: plan 1 only
    (64, 128),   # 4x128 only: fills the packets kernel's LDS weight buffer
)


# ------------------------------------------------------------------------------------------------------------------------
# networks
# ------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Network:
    name: str
    D: int = 0
    W: int = 0
    form: str = "folded"             # "folded" | "reference" (packed unfolded) | "no_view_dirs"
    mfma: bool = True                # both networks have one MFMA shape: every precision renders it
    shape_case: Optional[str] = None  # a case of tests/shape_domain.py: NWE_PREC_F32 only (or MFMA under separate passes)
    separate: bool = False           # two MFMA shapes: the MFMA precisions render it under separate passes

    @property
    def view_dirs(self) -> bool:
        return self.form != "no_view_dirs" if self.shape_case is None else SD.BY_NAME[self.shape_case].view_dirs

    @property
    def fold(self) -> bool:
        return self.form != "reference"


NETWORKS: List[Network] = [
    Network("4x128", 4, 128),                                        # the workhorse
    Network("8x256", 8, 256),
    Network("6x128-novd", 6, 128, "no_view_dirs"),                   # 8-column rays
    Network("4x128-reference", 4, 128, "reference"),                 # packed unfolded
    Network("1x2-freqs0-3+1", mfma=False, shape_case="1x2-freqs0-3+1"),
    Network("16x30", mfma=False, shape_case="16x30"),
    Network("c4x128-f8x256", mfma=False, shape_case="c4x128-f8x256", separate=True),   # the mixed pair, and separate passes
]
NET = {n.name: n for n in NETWORKS}
# seeds of the synthetic weights where 300 + D + W (tests/test_gpu_accuracy.py) is not kept: chosen on the oracle alone, until
# the fp32 and fp64 stages of every case agree to 1e-5 (tests/test_train_domain_oracle.py)
NET_SEED: Dict[str, int] = {"4x128": 438, "4x128-reference": 438}
# (seed, w_gain, b_gain) of the random network of a tests/shape_domain.py case where the case's own are not kept, chosen on the
# oracle alone like NET_SEED.  16x30 keeps its shape, encodings and seed; with the case's gain of 2.9 its raw outputs reach 17.5
# and the fp32 oracle's own stage C is 1.3e-4 from the fp64 oracle's (2.7: 6.0e-5), with 2.5 they reach 1.9 and it is 6.0e-6,
# while every case still composites (mean acc of the 16x30 pass 0.92 .. 0.98)
SHAPE_WEIGHTS: Dict[str, Tuple[int, float, float]] = {"16x30": (56, 2.5, 1.0)}
MFMA_NETWORKS = [n.name for n in NETWORKS if n.mfma]
F32_ONLY_NETWORKS = [n.name for n in NETWORKS if not n.mfma]


@dataclass
class Built:
    net: Network
    sd_c: Dict[str, np.ndarray]
    sd_f: Dict[str, np.ndarray]
    tc: Dict[str, torch.Tensor]
    tf: Dict[str, torch.Tensor]
    freqs_xyz: int
    freqs_dir: int
    rays: torch.Tensor               # [165, 11 | 8]


def _frame_rays(use_view_dirs: bool) -> torch.Tensor:
    pose = O.camera_pose((0.0, -0.5, -0.76, 0.0, -90.0, 0.0), (0, 0, 0, -30.0, 0.0, 0.0))
    fx, fy, cx, cy = O.intrinsics(FRAME_H, FRAME_W)
    return O.create_rays(pose, FRAME_H, FRAME_W, fx, fy, cx, cy, NEAR, FAR, use_view_dirs)[0][:N_RAYS].contiguous()


@functools.lru_cache(maxsize=None)
def build(name: str, single: bool = False) -> Built:
    """Thin-fog coarse network and a plain random fine network (tests/test_gpu_accuracy._nets), or the networks of a
    tests/shape_domain.py case.  `single` (n_importance == 0): there is no sampling to condition, and a thin fog's only pass has
    acc = 1 on every ray, so the one network is the plain random one of the coarse network's shape (as tests/shape_domain.build
    does).  Shared; nobody writes to it."""
    net = NET[name]
    if net.shape_case is not None:
        case = SD.BY_NAME[net.shape_case]
        fog = synthetic.thin_fog if case.view_dirs else synthetic.thin_fog_output
        seed, w_gain, b_gain = SHAPE_WEIGHTS.get(name, (case.seed, case.w_gain, case.b_gain))
        sd_c = fog(SD.make_net(case, case.coarse, seed))
        sd_f = SD.make_net(case, case.fine, seed + 1, w_gain, b_gain)
        if single:
            sd_c = SD.make_net(case, case.coarse, seed + 1, w_gain, b_gain)
        fx, fd = case.freqs_xyz, case.freqs_dir
    else:
        seed = NET_SEED.get(name, 300 + net.D + net.W)
        if net.form == "no_view_dirs":
            sd_c = synthetic.thin_fog_output(synthetic.make_state_dict(seed, net.D, net.W, use_view_dirs=False))
            sd_f = synthetic.make_state_dict(seed + 1, net.D, net.W, use_view_dirs=False)
        else:
            sd_c = synthetic.thin_fog(synthetic.make_state_dict(seed, net.D, net.W))
            sd_f = synthetic.make_state_dict(seed + 1, net.D, net.W)
        if single:
            sd_c = sd_f
        fx, fd = 10, 4
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    return Built(net, sd_c, sd_f, t(sd_c), t(sd_f), fx, fd, _frame_rays(net.view_dirs))


def config(b: Built, ns: int, ni: int) -> O.RenderConfig:
    return O.RenderConfig(n_samples=ns, n_importance=ni, freqs_xyz=b.freqs_xyz, freqs_dir=b.freqs_dir)


# ------------------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------------------

def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def tables(ns: int, ni: int, std: float, seed: int = 0, n_rays: int = N_RAYS) -> Dict[str, torch.Tensor]:
    """All four tables as the reference draws them (torch.rand / torch.randn * raw_noise_std) from a seeded generator."""
    g = torch.Generator().manual_seed(_seed("train_domain", ns, ni, seed))
    t = {"t_rand": torch.rand(n_rays, ns, generator=g),
         "noise_coarse": torch.randn(n_rays, ns, generator=g) * std,
         "noise_fine": torch.randn(n_rays, ns + ni, generator=g) * std,
         "u": torch.rand(n_rays, ni, generator=g)}
    if ni == 0:
        del t["noise_fine"], t["u"]
    return t


def pick(tab: Dict[str, torch.Tensor], subset: Sequence[str]) -> Dict[str, torch.Tensor]:
    return {k: tab[k] for k in subset if k in tab}


@dataclass(frozen=True)
class Case:
    net: str
    ns: int
    ni: int
    subset: Tuple[str, ...]
    std: float

    @property
    def id(self) -> str:
        return f"{self.net}-{self.ns}+{self.ni}-{'+'.join(self.subset)}-std{self.std:g}"


def samplings_of(name: str) -> Tuple[Tuple[int, int], ...]:
    if name == "4x128":
        return SAMPLINGS
    if NET[name].mfma or NET[name].separate:
        return tuple(s for s in SAMPLINGS if s != (64, 128))
    return ((3, 1), (7, 6), (9, 0))


def _cases() -> Iterator[Case]:
    """The workhorse takes every (sampling, subset, std).  Every other network takes all four tables at every sampling of its
    own, and every subset at (7, 6) and (9, 0), with std = 1; 0.1 once."""
    for net in NETWORKS:
        for ns, ni in samplings_of(net.name):
            subsets = SUBSETS if ni else SUBSETS_NI0
            last = (ALL4 if ni else SUBSETS_NI0[-1])
            for subset in subsets:
                for std in (1.0, 0.1):
                    if net.name != "4x128":
                        if (ns, ni) not in ((7, 6), (9, 0)) and subset != last:
                            continue
                        if std != 1.0 and not ((ns, ni) == (7, 6) and subset == last):
                            continue
                    if std != 1.0 and not any(k.startswith("noise") for k in subset):
                        continue                     # std only scales the noise tables
                    if ns >= 64 and std == 1.0 and "noise_coarse" in subset and "u" not in subset:
                        continue                     # unit noise under the linspace u at 64 or more coarse samples: the fp32
                                                     # oracle's own stage B leaves 10 % of the rays undecided (17 of 165)
                    yield Case(net.name, ns, ni, subset, std)


CASES: List[Case] = list(_cases())


# seeds of the tables per sampling where 0 is not kept: chosen on the oracle alone, until at most UNDECIDED_CAP of a case's rays
# are undecided in stage B on the fp32 oracle's own weights (tests/test_train_domain_oracle.py)
TABLE_SEED: Dict[Tuple[int, int], int] = {(65, 7): 1}


def case_tables(c: Case, n_rays: int = N_RAYS) -> Dict[str, torch.Tensor]:
    return pick(tables(c.ns, c.ni, c.std, TABLE_SEED.get((c.ns, c.ni), 0), n_rays), c.subset)


def built(net: str, ni: int) -> Built:
    return build(net, ni == 0)


# ------------------------------------------------------------------------------------------------------------------------
# stage references
# ------------------------------------------------------------------------------------------------------------------------

def _viewdirs(rays: torch.Tensor) -> Optional[torch.Tensor]:
    return rays[:, -3:] if rays.shape[-1] > 8 else None


def z_coarse(rays: torch.Tensor, ns: int, t_rand: Optional[torch.Tensor], dtype: torch.dtype = F32) -> torch.Tensor:
    """handler.py:216-218 and, with t_rand, training_handler.py:553-562; dtype = float32 is the kernel's own arithmetic."""
    rays = rays.to(dtype)
    t = torch.linspace(0., 1., steps=ns).to(dtype)
    z = (rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t).expand(rays.shape[0], ns)
    if t_rand is not None:
        mids = .5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * t_rand.to(dtype)
    return z


def _composite(raw, z, rays, noise, dtype) -> Dict[str, torch.Tensor]:
    rgb, disp, acc, w, depth = O.raw2outputs(raw, z, rays[:, 3:6].to(dtype), False, None if noise is None else noise.to(dtype))
    return {"raw": raw[..., :4], "rgb": rgb, "disp": disp, "acc": acc, "weights": w, "depth": depth, "z": z}


def _network(b: Built, which: int, rays: torch.Tensor, z: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    r = rays.to(dtype)
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]
    with torch.no_grad():
        return O.run_network(pts, _viewdirs(rays), b.tf if which else b.tc, b.freqs_xyz, b.freqs_dir, 1024 * 32, dtype=dtype)


def stage_a(b: Built, rays: torch.Tensor, ns: int, tab: Dict[str, torch.Tensor], dtype: torch.dtype,
            raw: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The coarse pass.  `raw` [R, ns, 4]: the caller's network outputs (nwe_debug_set_raw); the noise still acts on them."""
    z = z_coarse(rays, ns, tab.get("t_rand"), dtype)
    raw = _network(b, 0, rays, z, dtype) if raw is None else raw.to(dtype)
    return _composite(raw, z, rays, tab.get("noise_coarse"), dtype)


def linspace_u(n_rays: int, ni: int) -> torch.Tensor:
    return torch.linspace(0., 1., steps=ni).expand(n_rays, ni).contiguous()


def stage_b(zc32: torch.Tensor, weights: torch.Tensor, ni: int, u: Optional[torch.Tensor], dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """The sampler on GIVEN fp32 coarse depths and weights [R, ns] (handler.py:236-243, :267); u = None: the linspace table."""
    z, w = zc32.to(dtype), weights.to(dtype)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    u = linspace_u(z.shape[0], ni) if u is None else torch.sort(u, -1).values
    with torch.no_grad():
        zs = O.sample_pdf(z_mid, w[..., 1:-1], ni, u)
    return {"z_samples": zs, "z_fine": torch.sort(torch.cat([z, zs], -1), -1).values, "z_std": torch.std(zs, dim=-1, unbiased=False)}


def stage_c(b: Built, rays: torch.Tensor, z_fine: torch.Tensor, noise_fine: Optional[torch.Tensor], dtype: torch.dtype,
            raw: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The fine pass at GIVEN depths: O.fine_pass_given_depths with the noise and with 8-column rays."""
    z = z_fine.to(dtype)
    raw = _network(b, 1, rays, z, dtype) if raw is None else raw.to(dtype)
    return _composite(raw, z, rays, noise_fine, dtype)


def undecided(b32: Dict[str, torch.Tensor], b64: Dict[str, torch.Tensor], far: float = FAR) -> np.ndarray:
    """[R] bool: the ray's fp32 and fp64 stage-B depths differ by more than 1e-5 of far (or are not finite in either)."""
    d = (b32["z_fine"].double() - b64["z_fine"]).abs().max(-1).values / far
    return ~(d <= UNDECIDED).numpy()


def on_alpha_step(c64: Dict[str, torch.Tensor], noise: Optional[torch.Tensor]) -> np.ndarray:
    """[R] bool: the last sample sits on the alpha step of the 1e10 interval (|sigma_last + noise| < 1e-5 in fp64,
    model_utils.py:56), as tests/test_gpu_accuracy.e2e_accuracy leaves such rays out."""
    s = c64["raw"][:, -1, 3] + (0. if noise is None else noise[:, -1].double())
    return (s.abs() < 1e-5).numpy()


def chain(b: Built, rays: torch.Tensor, ns: int, ni: int, tab: Dict[str, torch.Tensor], dtype: torch.dtype):
    """Stages A, B, C in `dtype`, each on the one before it: the oracle's render loop (O.render_rays with train=tab)."""
    a = stage_a(b, rays, ns, tab, dtype)
    if ni == 0:
        return a, None, None
    s = O.sample_pdf(.5 * (a["z"][..., 1:] + a["z"][..., :-1]), a["weights"][..., 1:-1], ni, tab.get("u"))
    sb = {"z_samples": s, "z_fine": torch.sort(torch.cat([a["z"], s], -1), -1).values, "z_std": torch.std(s, dim=-1, unbiased=False)}
    return a, sb, stage_c(b, rays, sb["z_fine"], tab.get("noise_fine"), dtype)


# ------------------------------------------------------------------------------------------------------------------------
# the edge set
# ------------------------------------------------------------------------------------------------------------------------

EDGE_STD = 0.1
EDGE_SAMPLINGS = ((7, 6), (9, 0), (65, 7))
EDGE_RAYS = {"t_zero": 3, "t_one": 4, "t_entries": 5, "u_equal": 6, "u_tie": 7, "u_entries": 8, "noise_minus": 9, "noise_plus": 10,
             "noise_nan_coarse": 11, "noise_nan_fine": 12}
U_EQUAL = 0.37


def edge_tables(b: Built, ns: int, ni: int) -> Dict[str, torch.Tensor]:
    """All four tables at std 0.1 with the deliberate edges of EDGE_RAYS written into them (everything else is as drawn):
      t_rand  a ray of 0, a ray of nextafter(1, 0), single entries of both;
      u       a ray of equal numbers; a ray whose numbers are fp32 cdf entries of that very ray, taken from the fp32 oracle's
              coarse weights (the tie of searchsorted(right=True)); entries 0 and nextafter(1, 0);
      noise   a ray at -1e30 in both passes (sigma = 0 everywhere: acc = 0, disp = NaN with its flag), a ray at +1e30 (alpha
              saturates), one NaN on sample 2 of one ray of noise_coarse and of another ray of noise_fine."""
    t = {k: v.clone() for k, v in tables(ns, ni, EDGE_STD, seed=1).items()}
    E = EDGE_RAYS
    t["t_rand"][E["t_zero"]] = 0.0
    t["t_rand"][E["t_one"]] = ONE_BELOW
    t["t_rand"][E["t_entries"], 0] = 0.0
    t["t_rand"][E["t_entries"], 1] = ONE_BELOW
    t["t_rand"][E["t_entries"], -1] = ONE_BELOW
    for k in ("noise_coarse", "noise_fine"):
        if k in t:
            t[k][E["noise_minus"]] = -1e30
            t[k][E["noise_plus"]] = 1e30
    t["noise_coarse"][E["noise_nan_coarse"], 2] = float("nan")
    if ni:
        t["noise_fine"][E["noise_nan_fine"], 2] = float("nan")
        t["u"][E["u_equal"]] = U_EQUAL
        t["u"][E["u_entries"], 0] = 0.0
        t["u"][E["u_entries"], -1] = ONE_BELOW
        a32 = stage_a(b, b.rays, ns, t, F32)
        cdf = O.sample_pdf_cdf(a32["weights"][E["u_tie"]:E["u_tie"] + 1, 1:-1])[0]          # [ns - 1], fp32, cdf[0] = 0
        inner = cdf[(cdf < 1.0)]                                                            # the numbers of torch.rand are below 1
        t["u"][E["u_tie"]] = torch.sort(inner[torch.arange(ni) % inner.numel()]).values
    return t


def edge_expectation(ni: int) -> Dict[str, List[int]]:
    """Hand-written: output -> the rays that hold a non-finite element (tests/test_train_domain_oracle.py checks it against both
    oracles).  The -1e30 ray meets no density (acc = 0: only its disparity is NaN), the +1e30 ray is finite everywhere; the NaN
    in noise_coarse reaches every later weight of its ray, so its samples and everything behind them; the NaN in noise_fine
    reaches the fine composite of its ray alone.  Without importance samples the fine slots hold the coarse results."""
    E = EDGE_RAYS
    c, f = [E["noise_nan_coarse"]], sorted([E["noise_nan_coarse"], E["noise_nan_fine"]])
    out = {"raw_coarse": [], "weights_coarse": c, "rgb_coarse": c, "depth_coarse": c, "acc_coarse": c}
    if ni:
        out.update(z_fine=c, z_std=c, raw_fine=c, rgb=f, depth=f, acc=f)
    else:
        out.update(rgb=c, depth=c, acc=c)
    return out


def healthy_edge_rays(n_rays: int = N_RAYS) -> np.ndarray:
    """[R] bool: the rays whose tables hold nothing but finite numbers of ordinary size."""
    m = np.ones(n_rays, bool)
    for k in ("noise_minus", "noise_plus", "noise_nan_coarse", "noise_nan_fine"):
        m[EDGE_RAYS[k]] = False
    return m


# ------------------------------------------------------------------------------------------------------------------------
# hooks together with tables: a hook replaces its stage and nothing else
# ------------------------------------------------------------------------------------------------------------------------

# name -> (hooks armed, tables armed).  What each must compute (tests/test_gpu_train_domain.py checks it, include/nwe.h says it):
#   weights+t_rand+u        stage A is skipped (no coarse output is written); the jitter still defines z_coarse and z_mid, so
#                           z_fine / z_std = stage B (z_coarse(t_rand), the caller's weights, u), then stage C as ever
#   weights+noise_coarse    the noise has nothing to act on: every output equals the call with the hook alone, bit for bit
#   raw+noise               the noise is added to the caller's sigma_raw: stage A / C with raw = the caller's
#   depths+noise_fine       stage C at the caller's depths with the noise; z_fine = the caller's depths
#   depths+u                the sampler feeds nothing into the fine pass: rgb / depth / acc / raw_fine / z_fine equal the call with
#                           the hook alone bit for bit; z_std (and sample_cond / sample_amp / sample_switch) still describe the
#                           call's own importance samples, so they equal those of the call with u alone, bit for bit
COMBINATIONS: Dict[str, Tuple[Tuple[str, ...], Tuple[str, ...]]] = {
    "weights+t_rand+u": (("coarse_weights",), ("t_rand", "u")),
    "weights+noise_coarse": (("coarse_weights",), ("noise_coarse",)),
    "raw+noise": (("raw_coarse", "raw_fine"), ("noise_coarse", "noise_fine")),
    "raw_fine+all": (("raw_fine",), ALL4),
    "depths+noise_fine": (("fine_depths",), ("noise_fine",)),
    "depths+u": (("fine_depths",), ("u",)),
}
COMBINATION_SAMPLING = (7, 6)


def hook_inputs(ns: int, ni: int, n_rays: int = N_RAYS) -> Dict[str, torch.Tensor]:
    """Caller-made inputs of the hooks, unrelated to the networks: positive weights with a few empty bins, raw outputs with
    sigma of both signs, ascending depths inside [near, far]."""
    g = torch.Generator().manual_seed(_seed("hooks", ns, ni))
    w = torch.rand(n_rays, ns, generator=g) * 0.2
    w[torch.rand(n_rays, ns, generator=g) < 0.2] = 0.0
    raw = lambda s: torch.cat([torch.randn(n_rays, s, 3, generator=g), torch.randn(n_rays, s, 1, generator=g) * 0.5 + 0.1], -1)
    z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(n_rays, ns + ni, generator=g), -1).values
    return {"coarse_weights": w, "raw_coarse": raw(ns), "raw_fine": raw(ns + ni), "fine_depths": z}
