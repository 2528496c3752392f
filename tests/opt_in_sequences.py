"""Call sequences over everything a long-lived context carries today (include/nwe.h): the opt-in modes, the three grids, the four
event rings and the buffers that features added one at a time share.  What tests/test_opt_in_sequences_host.py (CPU) and
tests/test_gpu_opt_in_sequences.py (GPU) walk; nothing here needs a GPU.

The rule is tests/test_gpu_sequences.py's: every call on ONE long-lived context gives the bits, the flags - or the refusal - of a
FRESH context that was configured from `State` alone.  That file's walk knows two networks, the sampling, the white background and
the decomposition; this one adds early termination, the shared coarse pass, separate passes, the occupancy / coarse / radiance
grids (set from the host and made on the device), work queue, colour skip, packet blocks, sparse chunk and query steps, and the
calls that came with them: render_grid, render_sparse (both kinds), query_points, coarse_grid_weights, the three builds, bursts of
calls queued without a host synchronisation, and the one-shot hooks of render_rays across calls that must leave them alone.

`State.apply` holds the three clearing rules of nwe_set_network* and nothing else clever.  `expect` restates the order of
check_ready / check_modes (csrc/nwe_check.cpp) ONLY to steer the generator and to count coverage; no test asserts a refusal
because `expect` names it - the fresh context decides (the host test does hold `expect` to nwe_debug_plan, so that the coverage
counts mean what they say).

A walk is produced, not found: walk i of N_WALKS is responsible for every N_WALKS-th key of MUST_COVER and keeps emitting the steps
that produce a key it still lacks, with random steps in between, until its share is covered; the union of the walks covers the
table whatever the seeds are.  The seeds only shuffle the filler and the arguments.
"""
import functools
import random

import numpy as np

from tests import occupancy as G
from tests import test_gpu_sequences as Q

bits_equal, pose_of, camera_of, state_dict = Q.bits_equal, Q._pose, Q._kw, Q._sd

FRAMES = ((3, 9), (7, 19), (40, 64))      # 27 rays: below a wave; 133: ragged against 128; 2 560: past one 1 024-ray scan tile
PRECISIONS = ("f16x3", "f16x1", "f32")
SAMPLINGS = ((7, 6), (16, 24), (37, 17), (16, 0), (64, 128))
KINDS = ("4x128", "8x256", "noview", "generic")     # of tests/test_gpu_sequences.KINDS; "generic" has no MFMA kernel
LEAN, FULL = ("rgb", "depth", "acc"), Q.WALK_FULL
GRID_OUT = {"lean": LEAN, "diag": LEAN + ("weights_coarse", "z_fine", "raw_fine")}
SPARSE_OUT = {"lean": LEAN, "diag": LEAN + ("weights_coarse", "z_fine", "weights_grid", "selected", "raw_fine")}
MIN_WEIGHTS, DILATES = (-1.0, 1e-3, 2.0), (0, 1)
QUERY_COUNTS = (27, 133, 300)
HOOKS = Q.HOOKS
BOX_LO, BOX_HI = G.BOX_LO, G.BOX_HI
RES_SMALL, RES_BIG = (5, 4, 3), (11, 9, 5)           # 60 and 495 cells: the build scratch grows from one to the other
MODES = ("share", "term", "separate", "occ", "baked")            # the order of kModeTable (csrc/nwe_check.cpp)
EXCLUSIONS = (("share", "term"), ("separate", "term"), ("occ", "term"), ("occ", "share"), ("occ", "separate"), ("baked", "term"),
              ("baked", "share"), ("baked", "separate"), ("baked", "occ"))
TABLE_USERS = ("share", "separate", "baked")
SCRATCH_USERS = ("build_occ", "bake_cgrid", "bake_rgrid")
MID_BURST = ("share_k", "eps", "separate", "white", "decomp")      # host-side switches a burst may flip between two of its calls
RENDER_LIKE = ("render", "render_rays", "render_grid", "render_sparse", "query", "cgrid_weights", "create_rays")

# ---- grids set from the host --------------------------------------------------------------------------------------------------

STATIC_GRIDS = {"occ": ("occ_a", "occ_b"), "cgrid": ("cg_a", "cg_b"), "rgrid": ("rg_a", "rg_b")}


@functools.lru_cache(maxsize=None)
def static_grid(name):
    """{"values", "lo", "hi", "res"} of a named grid: leave it unchanged.  Occupancy: about half the cells; coarse grid: sigma of
    both signs; radiance grid: rows whose density is positive in most cells, so that a sparse frame has samples to select."""
    rng = np.random.Generator(np.random.Philox(key=[sum(name.encode()), 7]))
    res = RES_BIG if name.endswith("_a") else (6, 7, 4)
    if name.startswith("occ"):
        values = rng.uniform(size=res) < 0.5
    elif name.startswith("cg"):
        values = rng.uniform(-1.0, 2.0, size=res).astype(np.float32)
    else:
        values = rng.uniform(-0.5, 2.0, size=res + (4,)).astype(np.float32)
    return {"values": values, "lo": BOX_LO, "hi": BOX_HI, "res": res}


class Grids(dict):
    """name -> grid: the static ones, and the read-back of every grid a walk made on the device."""

    def __missing__(self, name):
        self[name] = static_grid(name)
        return self[name]


# ---- the state ------------------------------------------------------------------------------------------------------------------

class State:
    """What a context holds after the steps so far, and all a fresh context is configured with."""
    FIELDS = ("nets", "ns", "ni", "white", "eps", "share_k", "separate", "occ", "cgrid", "rgrid", "wq", "cskip", "blocks", "decomp",
              "chunk", "qsteps")
    SETTERS = ("white", "eps", "share_k", "separate", "wq", "cskip", "blocks", "decomp", "chunk", "qsteps")

    def __init__(self):
        self.nets = (("4x128", 100, True), ("4x128", 101, True))      # (kind, seed, folded at upload)
        self.ns, self.ni = 16, 24
        self.white, self.eps, self.share_k, self.separate = False, 0.0, 1, False
        self.occ = self.cgrid = self.rgrid = None                     # the name of a grid, or none
        self.wq, self.cskip, self.blocks, self.decomp, self.chunk, self.qsteps = -1, 1, True, -1, 0, 0

    def key(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def copy(self):
        s = State()
        for f in self.FIELDS:
            setattr(s, f, getattr(self, f))
        return s

    def noview(self, which):
        return self.nets[which][0] == "noview"

    def formulation(self, which):
        kind, _, fold = self.nets[which]
        return "noview" if kind == "noview" else ("folded" if fold else "reference")

    def mfma_ok(self, which):
        return self.nets[which][0] != "generic"       # 4x128 and 8x256 have a reference-formulation kernel too

    def form(self, which):
        return (self.nets[which][0], self.formulation(which))

    def apply(self, step):
        """A step that succeeded.  The clearing rules: either upload clears the occupancy and the radiance grid, the coarse upload
        the coarse grid; a refused step changes nothing."""
        op = step[0]
        if op == "net":
            _, which, kind, seed, fold = step
            nets = list(self.nets)
            for w in ((0, 1) if which == 2 else (which,)):
                nets[w] = (kind, seed + w, fold)
            self.nets = tuple(nets)
            self.occ = self.rgrid = None
            if which != 1:
                self.cgrid = None
        elif op == "sampling":
            self.ns, self.ni = step[1], step[2]
        elif op in self.SETTERS:
            setattr(self, op, step[1])
        elif op in ("set_occ", "build_occ"):
            self.occ = step[1]
        elif op in ("set_cgrid", "bake_cgrid"):
            self.cgrid = step[1]
        elif op in ("set_rgrid", "bake_rgrid"):
            self.rgrid = step[1]
        elif op == "clear_occ":
            self.occ = None
        elif op == "clear_cgrid":
            self.cgrid = None
        elif op == "clear_rgrid":
            self.rgrid = None
        elif op == "burst":
            for item in step[1]:
                if item[0] not in RENDER_LIKE:
                    self.apply(item)
            if step[2] is not None:
                self.apply(step[2])


def n_rays_of(call):
    """Rays of a render-like call on a frame: (.., frame, n_poses) close every such call."""
    H, W = FRAMES[call[-2]]
    return H * W * call[-1]


def n_rep_of(call, k):
    H, W = FRAMES[call[-2]]
    return -(-H // k) * -(-W // k) * call[-1]


def expect(st, call, hook=None):
    """None if `call` renders in state `st`, else a tuple that names the refusal: check_ready and check_modes in their order, then
    what launch() refuses.  For steering and counting only."""
    op = call[0]
    if op in ("render", "render_rays"):
        prec, outk = call[1], call[2]
        pinhole, mfma, ni = op == "render", call[1] != "f32", st.ni
        if ni > 0 and st.noview(0) != st.noview(1):
            return ("view_dirs",)
        baked = st.cgrid is not None
        if mfma and ((not (baked and ni > 0) and not st.mfma_ok(0)) or (ni > 0 and not st.mfma_ok(1))):
            return ("no_mfma_kernel",)
        on = dict(share=st.share_k > 1, term=st.eps > 0, separate=st.separate, occ=st.occ is not None, baked=baked)
        for m in MODES:
            if not on[m] or (m == "separate" and not mfma):
                continue
            for a, b in EXCLUSIONS:
                if a == m and on[b]:
                    return ("pair", a, b)
            if m == "separate":
                if ni > 0 and st.formulation(0) != st.formulation(1):
                    return ("separate", "form")
                continue
            if not pinhole:
                return (m, "rays")
            if outk != "lean":
                return (m, "output")
            if mfma:
                for i in range(1 if m == "baked" else 0, 2 if ni > 0 else 1):
                    if st.formulation(i) == "reference":
                        return (m, "unfolded")
        if mfma and ni > 0 and not st.separate and not baked and st.form(0) != st.form(1):
            return ("same_shape",)
        return None
    if op == "render_grid":
        return None if st.rgrid else ("no_rgrid",)
    if op == "render_sparse":
        if not st.rgrid:
            return ("no_rgrid",)
        return ("no_mfma_kernel",) if call[2] != "f32" and not st.mfma_ok(call[3]) else None
    if op == "query":
        return ("no_mfma_kernel",) if call[2] != "f32" and not st.mfma_ok(call[1]) else None
    if op == "cgrid_weights":
        return None if st.cgrid else ("no_cgrid",)
    return None


def table_use(st, call, hook=None):
    """(user, floats) of the render slot's weight table in a render / render_rays call that renders, or (None, 0): plan_call's
    table_elems (csrc/nwe_plan.cpp)."""
    if call[0] not in ("render", "render_rays") or st.ni == 0:
        return None, 0
    n = n_rays_of(call)
    if st.cgrid is not None:
        return "baked", n * st.ns
    if st.share_k > 1:
        return "share", n_rep_of(call, st.share_k) * st.ns
    if st.separate and call[1] != "f32":
        lean = call[0] == "render" and call[2] == "lean"
        if not lean and hook == "coarse_weights":       # no coarse launch: the caller's weights
            return None, 0
        return "separate", n * st.ns
    return None, 0


def scratch_use(step):
    """Floats of d_occ_scratch a build step reserves (csrc/nwe_abi_grids.hip; grids this small are one chunk)."""
    cells = int(np.prod(step[2]))
    # one chunk: the builds walk at most 2^20 probe points at a time (tests/grid_sizes.py: BAKE_CHUNK_CELLS); beyond that the scratch
    # would hold a chunk, not the grid, and this model would not be the library's
    assert cells * (step[3] ** 3 if step[0] == "build_occ" else 1) <= 1 << 20, step
    if step[0] == "build_occ":
        return cells * step[3] ** 3 * 4
    return cells * 3 + (3 if step[0] == "bake_rgrid" else 0)


def build_ok(st, step):
    """Whether a build step is made in this state: the generator makes only builds that the ABI accepts."""
    if step[-1] == "f32":
        return True
    if step[0] == "build_occ":
        return st.mfma_ok(0) and st.mfma_ok(1)
    return st.mfma_ok(0 if step[0] == "bake_cgrid" else step[3])


# ---- coverage -------------------------------------------------------------------------------------------------------------------

OPS = ("render", "render_rays", "render_grid", "sparse_sync", "sparse_async", "query_raw", "query_sigma", "cgrid_weights", "create_rays",
       "build_occ", "bake_cgrid", "bake_rgrid", "sampling", "net_both", "net_coarse", "net_fine", "unfolded_upload", "white", "eps", "share_k",
       "separate", "wq", "cskip", "blocks", "decomp", "chunk", "qsteps", "set_occ", "clear_occ", "set_cgrid", "clear_cgrid", "set_rgrid",
       "clear_rgrid", "burst", "burst_setter", "hooked")
PAIRS = [(o, p) for o in ("render", "render_rays", "sparse_sync", "sparse_async", "query_raw", "query_sigma") for p in PRECISIONS] + \
        [(o, p) for o in SCRATCH_USERS for p in PRECISIONS]
MIXED = "4x128+8x256"
MUST_COVER = (
    [(("op", o), 2) for o in OPS] + [(("pair",) + p, 2) for p in PAIRS] +
    [(("frame", f, n), 2) for f in range(len(FRAMES)) for n in (1, 2)] +
    [(("kind", k), 2) for k in KINDS + (MIXED,)] + [(("sampling",) + s, 2) for s in SAMPLINGS] +
    [(("sparse_args", w, d), 2) for w in MIN_WEIGHTS for d in DILATES] + [(("hook", h), 2) for h in HOOKS] +
    [(("refused", m, a), 2) for m in ("term", "share", "occ", "baked") for a in ("rays", "output", "unfolded")] +
    [(("refused", "separate", "form"), 2), (("refused", "same_shape"), 2), (("refused", "no_mfma_kernel"), 2), (("refused", "view_dirs"), 2)] +
    [(("refused", "pair") + x, 2) for x in EXCLUSIONS] +
    [(("refused_setter", s), 2) for s in ("nan_eps", "k17", "box_occ", "box_cgrid", "box_rgrid", "net")] +
    [(("clears", how, g), 2) for how in ("coarse_upload", "fine_upload", "refused_upload") for g in ("occ", "cgrid", "rgrid")] +
    [(("table_pair", a, b), 1) for a in TABLE_USERS for b in TABLE_USERS if a != b] + [(("table_grows",), 2), (("table_to_none",), 2)] +
    [(("scratch_pair", a, b), 1) for a in SCRATCH_USERS for b in SCRATCH_USERS if a != b] + [(("scratch_grows",), 2)] +
    [(("sparse_after", "sync", "async"), 2), (("sparse_after", "async", "sync"), 2), (("sparse_grows",), 2)] +
    [(("behind_async", k), 2) for k in ("render", "query", "render_grid")] + [(("burst_setter_waits",), 2)] +
    [(("mid_burst", f), 2) for f in MID_BURST] + [(("under_async", "share_k", "render"), 2)])
N_WALKS = 8
# (seed, least number of steps) of each walk.  The first seeds there are: a walk covers its share of MUST_COVER by construction
# (see the module docstring), so no seed had to be searched for; tests/test_opt_in_sequences_host.py checks the union on the CPU.
WALKS = tuple((seed, 60) for seed in range(1, N_WALKS + 1))


def coverage_gaps(cover, share=(0, 1)):
    return [(k, n) for i, (k, n) in enumerate(MUST_COVER) if i % share[1] == share[0] and cover.get(k, 0) < n]


def union_coverage():
    total = {}
    for i in range(N_WALKS):
        for k, n in make_walk(i)[1].items():
            total[k] = total.get(k, 0) + n
    return total


# ---- the generator --------------------------------------------------------------------------------------------------------------

class Walker:
    """One walk: the steps, the coverage counts and the generator's model of the rings and scratches."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.st, self.steps, self.cover = State(), [], {}
        self.next_seed, self.next_grid = 200, 0
        self.launches = 0                                  # successful non-empty render launches: the slot is launches % 4
        self.slot_user, self.slot_cap = [None] * 4, [0] * 4
        self.slots = []                                    # per emitted step: the slot the generator says the next launch takes
        self.scratch_user, self.scratch_cap = None, 0
        self.sparse_last, self.sparse_cap = None, 0        # the kind of the last sparse call if it was the last step, the largest so far

    def count(self, *key):
        self.cover[key] = self.cover.get(key, 0) + 1

    # -- bookkeeping of one render-like call --
    def note_call(self, call, hook=None, behind=None):
        st, op = self.st, call[0]
        why = expect(st, call, hook)
        if why is not None:
            self.count("refused", *why)
            return False
        if op in ("render", "render_rays"):
            self.count("op", op); self.count("pair", op, call[1]); self.count("frame", call[-2], call[-1])
            user, elems = table_use(st, call, hook)
            slot = self.launches % 4
            prev = self.slot_user[slot]
            if user and prev and prev != user:
                self.count("table_pair", prev, user)
            if user and 0 < self.slot_cap[slot] < elems:
                self.count("table_grows")
            if not user and prev:
                self.count("table_to_none")
            self.slot_user[slot], self.slot_cap[slot] = user, max(self.slot_cap[slot], elems)
            self.launches += 1
        elif op == "render_sparse":
            kind = "async" if call[1] else "sync"
            self.count("op", "sparse_" + kind); self.count("pair", "sparse_" + kind, call[2]); self.count("sparse_args", call[4], call[5])
            self.count("frame", call[-2], call[-1])
            if self.sparse_last and self.sparse_last != kind:
                self.count("sparse_after", self.sparse_last, kind)
            size = n_rays_of(call) * (st.ns + st.ni)
            if 0 < self.sparse_cap < size:
                self.count("sparse_grows")
            self.sparse_cap = max(self.sparse_cap, size)
        elif op == "query":
            self.count("op", "query_" + call[3]); self.count("pair", "query_" + call[3], call[2])
        else:
            self.count("op", op)
            if op == "render_grid":
                self.count("frame", call[-2], call[-1])
        if behind is not None and behind[0] == "render_sparse" and behind[1] and expect(st, behind) is None and op in ("render", "query", "render_grid"):
            self.count("behind_async", op)
        return True

    def emit(self, step):
        st, op = self.st, step[0]
        self.slots.append(self.launches % 4)
        self.steps.append(step)
        sparse_before, self.sparse_last = self.sparse_last, None
        if op in RENDER_LIKE:
            if op == "render_sparse":
                self.sparse_last = sparse_before            # "directly after": the step before this one
            rendered = self.note_call(step)
            self.sparse_last = ("async" if step[1] else "sync") if rendered and op == "render_sparse" else None
        elif op == "burst":
            self.count("op", "burst")
            behind, under_async, in_flight = None, None, False
            for item in step[1]:
                if item[0] in RENDER_LIKE:
                    in_flight |= self.note_call(item, behind=behind)
                    if under_async and item[0] == "render" and expect(st, item) is None:
                        self.count("under_async", under_async, "render")     # the setter reached the render and not the sparse frame
                    behind, under_async = item, None
                else:                       # a host-side switch in the middle: copied at launch, it reaches no call queued before it
                    self.count("mid_burst", item[0])
                    if behind is not None and behind[0] == "render_sparse" and behind[1] and expect(st, behind) is None:
                        under_async = item[0]
                    self.count_setter(item)
                    st.apply(item)
            if step[2] is not None:
                self.count("op", "burst_setter")
                if in_flight:
                    self.count("burst_setter_waits")
                self.count_setter(step[2])
                st.apply(step[2])
            return
        elif op == "hooked":
            _, hook, between, rays_call = step
            self.count("op", "hooked"); self.count("hook", hook)
            self.note_call(between)
            self.note_call(rays_call, hook=hook)
        else:
            self.count_setter(step)
        st.apply(step)

    def count_setter(self, step):
        st, op = self.st, step[0]
        if op == "net":
            which = step[1]
            self.count("op", ("net_coarse", "net_fine", "net_both")[which])
            if not step[4]:
                self.count("op", "unfolded_upload")
            how = "fine_upload" if which == 1 else "coarse_upload"
            for g in ("occ", "cgrid", "rgrid"):
                if getattr(st, g) is not None:
                    self.count("clears", how, g)
            after = st.copy(); after.apply(step)
            kinds = (after.nets[0][0], after.nets[1][0])
            self.count("kind", MIXED if kinds == ("4x128", "8x256") else step[2])
        elif op == "refused_net":
            self.count("refused_setter", "net")
            for g in ("occ", "cgrid", "rgrid"):
                if getattr(st, g) is not None:
                    self.count("clears", "refused_upload", g)
        elif op.startswith("refused_"):
            self.count("refused_setter", op[len("refused_"):])
        elif op == "sampling":
            self.count("op", op); self.count("sampling", step[1], step[2])
        elif op in SCRATCH_USERS:
            self.count("op", op); self.count("pair", op, step[-1])
            need = scratch_use(step)
            if self.scratch_user and self.scratch_user != op:
                self.count("scratch_pair", self.scratch_user, op)
            if 0 < self.scratch_cap < need:
                self.count("scratch_grows")
            self.scratch_user, self.scratch_cap = op, max(self.scratch_cap, need)
        else:
            self.count("op", op)

    # -- arguments --
    def seed(self):
        self.next_seed += 2
        return self.next_seed

    def frame(self, small=False):
        return (self.rng.randrange(2 if small else len(FRAMES)), self.rng.choice((1, 1, 2)))

    def a_render(self, prec=None, outk=None, op=None, frame=None):
        return (op or self.rng.choice(("render", "render_rays")), prec or self.rng.choice(PRECISIONS), outk or self.rng.choice(("lean", "full"))) + \
               (frame or self.frame())

    def a_sparse(self, kind=None, prec=None, frame=None, args=None):
        asynchronous = self.rng.random() < 0.5 if kind is None else kind == "async"
        w, d = args or (self.rng.choice(MIN_WEIGHTS), self.rng.choice(DILATES))
        return ("render_sparse", asynchronous, prec or self.rng.choice(PRECISIONS), self.rng.randrange(2), w, d, self.rng.choice(("lean", "diag"))) + \
               (frame or self.frame())

    def a_query(self, what=None, prec=None):
        return ("query", self.rng.randrange(2), prec or self.rng.choice(PRECISIONS), what or self.rng.choice(("raw", "sigma")), self.rng.choice(QUERY_COUNTS))

    def a_grid_frame(self):
        return ("render_grid", self.rng.choice(("lean", "diag"))) + self.frame()

    def a_build(self, op, prec=None, res=None):
        self.next_grid += 1
        name, res = f"made_{op}_{self.next_grid}", res or self.rng.choice((RES_SMALL, RES_BIG))
        prec = prec or self.rng.choice(PRECISIONS)
        if op == "build_occ":
            step = (op, name, res, self.rng.choice((1, 2)), self.rng.choice((0.0, 0.5)), self.rng.choice((0, 1)), prec)
        elif op == "bake_cgrid":
            step = (op, name, res, prec)
        else:
            step = (op, name, res, self.rng.randrange(2), prec)
        return step if build_ok(self.st, step) else step[:-1] + ("f32",)

    def valid_precisions(self, call_without_prec):
        return [p for p in PRECISIONS if expect(self.st, call_without_prec(p)) is None]

    # -- moving the state --
    def set(self, field, value):
        if getattr(self.st, field) != value:
            self.emit((field, value))

    def nets(self, kind0="4x128", kind1=None, fold=(True, True)):
        kind1 = kind1 or kind0
        for which, kind, f in ((0, kind0, fold[0]), (1, kind1, fold[1])):
            have = self.st.nets[which]
            if have[0] != kind or (have[2] != f and kind != "noview"):
                self.emit(("net", which, kind, self.seed() - which, f))

    def sampling(self, importance=True):
        if importance and self.st.ni == 0:
            self.emit(("sampling",) + self.rng.choice([s for s in SAMPLINGS[:3]]))

    def grid(self, g, on=True):
        if on and getattr(self.st, g) is None:
            self.emit(("set_" + g, self.rng.choice(STATIC_GRIDS[g])))
        if not on and getattr(self.st, g) is not None:
            self.emit(("clear_" + g,))

    def mode(self, m, on):
        if m == "share":
            if on != (self.st.share_k > 1):
                self.emit(("share_k", self.rng.choice((2, 3, 5)) if on else 1))
        elif m == "term":
            self.set("eps", 0.01 if on else 0.0)
        elif m == "separate":
            self.set("separate", on)
        else:
            self.grid("occ" if m == "occ" else "cgrid", on)

    def only_modes(self, *keep):
        for m in MODES:
            self.mode(m, m in keep)

    def plain(self, kind="4x128"):
        self.only_modes()
        self.nets(kind)
        self.sampling()

    # -- producing a key of MUST_COVER --
    def produce(self, key):
        rng, st, what = self.rng, self.st, key[0]
        if what == "op":
            self.produce_op(key[1])
        elif what == "pair":
            o, prec = key[1], key[2]
            if o in SCRATCH_USERS:
                self.nets(rng.choice(KINDS[:3]))
                self.emit(self.a_build(o, prec))
                self.check_builds()
            elif o in ("render", "render_rays"):
                self.plain(rng.choice(("4x128", "8x256")))
                self.emit(self.a_render(prec, op=o))
            elif o.startswith("sparse"):
                self.nets(rng.choice(("4x128", "8x256", "noview")))
                self.grid("rgrid")
                self.emit(self.a_sparse(o[7:], prec))
            else:
                self.nets(rng.choice(("4x128", "8x256", "noview")))
                self.emit(self.a_query(o[6:], prec))
        elif what == "frame":
            self.plain()
            self.emit(self.a_render(frame=(key[1], key[2])))
        elif what == "kind":
            if key[1] == MIXED:                 # only separate passes render it under the MFMA precisions
                self.only_modes("separate")
                self.nets("4x128", "8x256")
                self.sampling()
                self.emit(self.a_render(rng.choice(("f16x3", "f16x1"))))
                self.set("separate", False)
                self.emit(self.a_render(rng.choice(("f16x3", "f16x1"))))        # refused inside launch(): "same shape"
                self.emit(self.a_render("f32"))
            else:
                self.only_modes()
                self.emit(("net", 2, key[1], self.seed(), True))
                self.emit(self.a_render("f32" if key[1] == "generic" else None))
        elif what == "sampling":
            if (st.ns, st.ni) == key[1:]:
                self.emit(("sampling",) + rng.choice([s for s in SAMPLINGS if s != key[1:]]))
            self.emit(("sampling",) + key[1:])
            self.only_modes()
            self.nets(st.nets[0][0] if st.nets[0][0] == st.nets[1][0] else "4x128")
            self.emit(self.a_render("f32" if st.nets[0][0] == "generic" else None, frame=self.frame(small=key[1:] == (64, 128))))
        elif what == "sparse_args":
            self.nets(rng.choice(("4x128", "8x256")))
            self.grid("rgrid")
            self.emit(self.a_sparse(args=key[1:]))
        elif what == "hook":
            self.hooked(key[1])
        elif what == "refused":
            self.produce_refusal(key[1:])
        elif what == "refused_setter":
            self.emit(("refused_" + key[1],))
        elif what == "clears":
            how, g = key[1], key[2]
            self.nets(rng.choice(KINDS[:3]))
            self.sampling()
            # the grid, and nothing beside it that would refuse the frame that reads it (an occupancy grid and a coarse grid exclude
            # each other; the radiance grid excludes nothing)
            self.only_modes(*{"occ": ("occ",), "cgrid": ("baked",), "rgrid": rng.choice(((), ("occ",), ("baked",)))}[g])
            self.grid(g)
            if how == "refused_upload":
                self.emit(("refused_net",))
            else:
                which = 1 if how == "fine_upload" else rng.choice((0, 2))
                kind = st.nets[which][0] if which < 2 else rng.choice(KINDS[:3])
                self.emit(("net", which, kind, self.seed() - (which == 1), True))
            # what the rule kept or dropped is seen by the calls that read it
            self.emit(self.a_render(None, "lean", "render"))
            self.emit(self.a_grid_frame())
            self.emit(self.a_sparse())
        elif what == "table_pair":
            self.table_user(key[1]); self.lean_frame()
            self.table_user(key[2])
            for _ in range(4):
                self.lean_frame()
        elif what == "table_grows":
            self.table_user(rng.choice(("separate", "baked")))      # n_rays x n_samples floats: the largest tables
            if self.slot_cap[self.launches % 4] >= 5120 * st.ns:
                self.emit(("sampling", 64, 128))
            self.lean_frame((0, 1))
            for _ in range(3):
                self.lean_frame((rng.randrange(2), 1))
            self.lean_frame((2, 2))
        elif what == "table_to_none":
            self.table_user(rng.choice(TABLE_USERS)); self.lean_frame()
            self.only_modes()
            for _ in range(4):
                self.lean_frame()
        elif what == "scratch_pair":
            self.nets(rng.choice(("4x128", "8x256")))
            self.emit(self.a_build(key[1])); self.emit(self.a_build(key[2]))
            self.check_builds()
        elif what == "scratch_grows":
            self.nets(rng.choice(("4x128", "8x256")))
            if self.scratch_cap == 0:
                self.emit(self.a_build(rng.choice(SCRATCH_USERS), res=RES_SMALL))
            for res, probes in ((RES_BIG, 2), ((12, 10, 9), 2), ((16, 12, 10), 2), ((16, 12, 10), 3), ((20, 16, 12), 3), ((24, 20, 16), 4)):
                big = self.a_build("build_occ", res=res)
                big = big[:3] + (probes,) + big[4:]
                if scratch_use(big) > self.scratch_cap:
                    self.emit(big)
                    break
            self.check_builds()
        elif what == "sparse_after":
            self.nets(rng.choice(("4x128", "8x256", "noview")))
            self.grid("rgrid")
            self.emit(self.a_sparse(key[1])); self.emit(self.a_sparse(key[2]))
        elif what == "sparse_grows":
            self.nets("4x128")
            self.grid("rgrid")
            if self.sparse_cap >= 5120 * (st.ns + st.ni):
                self.emit(("sampling", 64, 128))
            self.emit(self.a_sparse(frame=(0, 1))); self.emit(self.a_sparse(frame=(2, 2)))
        elif what == "behind_async":
            self.burst(behind=key[1])
        elif what == "burst_setter_waits":
            self.burst(setter=True)
        elif what == "mid_burst":
            self.burst(switch=key[1])
        elif what == "under_async":
            self.burst(switch=key[1], under_async=True)
        else:
            raise AssertionError(key)

    def check_builds(self):
        """The grids made on the device are read by the calls that read them."""
        st = self.st
        if st.rgrid:
            self.emit(self.a_grid_frame())
        if st.occ and st.cgrid:
            self.grid("cgrid", False)
        self.only_modes(*(m for m in ("occ", "baked") if getattr(st, "occ" if m == "occ" else "cgrid") is not None))
        self.sampling()
        self.emit(self.a_render(None, "lean", "render"))

    def table_user(self, user):
        self.nets(self.rng.choice(("4x128", "8x256")))
        self.sampling()
        self.only_modes(user)

    def lean_frame(self, frame=None):
        prec = self.rng.choice(PRECISIONS[:2]) if self.st.separate else None
        outk = self.rng.choice(("lean", "full")) if self.st.separate and self.st.share_k == 1 else "lean"
        self.emit(self.a_render(prec, outk, "render" if outk == "lean" else None, frame or self.frame(small=True)))

    def produce_op(self, o):
        rng, st = self.rng, self.st
        if o in ("render", "render_rays"):
            self.plain(); self.emit(self.a_render(op=o))
        elif o == "render_grid":
            self.grid("rgrid"); self.emit(self.a_grid_frame())
        elif o.startswith("sparse_"):
            self.produce(("pair", o, rng.choice(PRECISIONS)))
        elif o.startswith("query_"):
            self.produce(("pair", o, rng.choice(PRECISIONS)))
        elif o == "cgrid_weights":
            self.grid("cgrid"); self.emit((o,) + self.frame())
        elif o == "create_rays":
            self.emit((o,) + self.frame())
        elif o in SCRATCH_USERS:
            self.produce(("pair", o, rng.choice(PRECISIONS)))
        elif o == "sampling":
            self.produce(("sampling",) + rng.choice(SAMPLINGS))
        elif o in ("net_both", "net_coarse", "net_fine"):
            which = ("net_coarse", "net_fine", "net_both").index(o)
            kind = rng.choice(KINDS[:3]) if which == 2 else st.nets[which][0]
            self.emit(("net", which, kind, self.seed() - (which == 1), st.nets[which][2] if which < 2 else True))
        elif o == "unfolded_upload":
            self.only_modes()
            self.nets(rng.choice(("4x128", "8x256")), fold=(False, False))
            self.sampling()
            self.emit(self.a_render())
        elif o in ("set_occ", "set_cgrid", "set_rgrid"):
            self.emit((o, rng.choice(STATIC_GRIDS[o[4:]])))
        elif o in ("clear_occ", "clear_cgrid", "clear_rgrid"):
            self.grid(o[6:]); self.emit((o,))
        elif o == "burst":
            self.burst()
        elif o == "burst_setter":
            self.burst(setter=True)
        elif o == "hooked":
            self.hooked(rng.choice(HOOKS))
        else:                                   # a switch: another value, then a frame that reads it
            values = {"white": (False, True), "eps": (0.0, 0.01, 0.2), "share_k": (1, 2, 3, 5, 16), "separate": (False, True), "wq": (-1, 0, 1),
                      "cskip": (0, 1, 2), "blocks": (False, True), "decomp": (-1, 0, 1, 2), "chunk": (0, 1, 64, 100, 1000), "qsteps": (0, 1, 3)}[o]
            self.emit((o, rng.choice([v for v in values if v != getattr(st, o)])))
            if o in ("chunk", "qsteps"):
                self.nets(st.nets[1][0] if st.nets[1][0] != "generic" else "4x128")
                self.grid("rgrid")
                self.emit(self.a_sparse(frame=(rng.randrange(len(FRAMES)), 1)))
            elif o in ("wq", "cskip", "blocks", "decomp"):
                self.plain()
                self.emit(("render", rng.choice(PRECISIONS[:2]), "lean", 2, 1))     # 40 x 64: rows a multiple of 4, W of 8
            else:
                self.emit(self.a_render(op="render", outk="lean"))

    def produce_refusal(self, why):
        rng = self.rng
        mfma = rng.choice(PRECISIONS[:2])
        if why[0] == "pair":
            self.nets(rng.choice(("4x128", "8x256"))); self.sampling()        # the networks first: an upload clears the grids
            self.only_modes(why[1], why[2])
            self.emit(self.a_render(mfma if "separate" in why else None, "lean", "render"))
        elif why[0] in ("term", "share", "occ", "baked"):
            self.sampling()
            if why[1] == "unfolded":
                self.nets(rng.choice(("4x128", "8x256")), fold=(True, False) if why[0] == "baked" else (False, False))
                self.only_modes(why[0])
                self.emit(self.a_render(mfma, "lean", "render"))
                self.emit(self.a_render("f32", "lean", "render"))          # NWE_PREC_F32 renders it
            else:
                self.nets(rng.choice(("4x128", "8x256", "noview")))
                self.only_modes(why[0])
                self.emit(self.a_render(None, "lean" if why[1] == "rays" else "full", "render_rays" if why[1] == "rays" else "render"))
            self.emit(self.a_render("f32" if self.st.formulation(1) == "reference" else None, "lean", "render"))   # ... and the mode still renders
        elif why == ("separate", "form"):
            self.only_modes("separate"); self.sampling()
            self.nets("4x128", rng.choice(("4x128", "8x256")), fold=rng.choice(((True, False), (False, True))))
            self.emit(self.a_render(mfma))
            self.emit(self.a_render("f32"))
        elif why == ("same_shape",):
            self.only_modes(); self.sampling()
            self.nets(*rng.choice((("4x128", "8x256"), ("8x256", "4x128"))))
            self.emit(self.a_render(mfma)); self.emit(self.a_render("f32"))
        elif why == ("no_mfma_kernel",):
            which = rng.randrange(2)
            self.emit(("net", which, "generic", self.seed() - which, True))
            self.emit(("query", which, mfma, rng.choice(("raw", "sigma")), 27))
            self.emit(self.a_render(mfma))          # by that refusal too, unless the call does not run that network or another refusal comes first
            self.emit(self.a_render("f32"))
        elif why == ("view_dirs",):
            self.sampling()
            which = rng.randrange(2)
            self.nets(*(("noview", "4x128") if which == 0 else ("4x128", "noview")))
            self.emit(self.a_render())
            self.emit(self.a_query())
        else:
            raise AssertionError(why)

    def burst(self, behind=None, setter=False, switch=None, under_async=False):
        """Two to five render-like calls queued with nothing waited for in between - a synchronous sparse frame would wait, so the
        sparse frames of a burst are asynchronous.  `behind`: one of the calls directly behind an asynchronous sparse frame;
        `switch`: a host-side switch flipped between two calls (`under_async`: directly behind an asynchronous sparse frame and in
        front of a render, include/nwe.h: copied at launch, so it reaches the render and not the frame in flight); `setter`: ended
        by a setter that must wait for them."""
        rng, st = self.rng, self.st
        self.nets(rng.choice(("4x128", "8x256")))
        self.only_modes(*(() if switch else rng.choice(((), (), ("share",), ("separate",), ("baked",), ("occ",)))))
        self.sampling()
        self.grid("rgrid")
        small = lambda: (rng.randrange(2), 1)
        makers = {"render": lambda: self.a_render(rng.choice(PRECISIONS[:2]) if st.separate or switch == "separate" else None, "lean", "render", small()),
                  "query": lambda: self.a_query(),
                  "render_grid": lambda: ("render_grid", rng.choice(("lean", "diag"))) + small(),
                  "sparse": lambda: self.a_sparse("async", frame=small()),
                  "cgrid_weights": lambda: ("cgrid_weights",) + small(), "create_rays": lambda: ("create_rays",) + small()}
        calls = []
        if behind:
            calls += [self.a_sparse("async", frame=small()), makers[behind]()]
        if switch:
            values = {"share_k": (1, 2, 3, 5), "eps": (0.0, 0.01), "separate": (False, True), "white": (False, True), "decomp": (-1, 0, 1, 2)}[switch]
            flip = (switch, rng.choice([v for v in values if v != getattr(st, switch)]))
            calls += [self.a_sparse("async", frame=small()) if under_async else makers[rng.choice(("render", "sparse", "render_grid"))](), flip, makers["render"]()]
        while len(calls) < 2 or (len(calls) < 5 and rng.random() < 0.6):
            at = len(calls) if behind else rng.choice((0, len(calls))) if switch else rng.randrange(len(calls) + 1)
            calls.insert(at, makers[rng.choice(tuple(makers))]())
        end = None
        if setter:
            end = rng.choice((("sampling",) + rng.choice([s for s in SAMPLINGS[:3] if s != (st.ns, st.ni)]),
                              ("net", 1, st.nets[1][0], self.seed() - 1, True), ("set_rgrid", rng.choice(STATIC_GRIDS["rgrid"])), ("clear_rgrid",),
                              ("set_occ", rng.choice(STATIC_GRIDS["occ"])), ("set_cgrid", rng.choice(STATIC_GRIDS["cgrid"]))))
        self.emit(("burst", tuple(calls), end))

    def hooked(self, hook):
        """Arm, a call that by include/nwe.h neither uses nor clears the hook, then the render_rays call that consumes it."""
        rng = self.rng
        self.only_modes(*rng.choice(((), ("separate",))))
        self.nets(rng.choice(("4x128", "8x256")))
        self.sampling()
        self.grid("rgrid")
        frame = (rng.randrange(2), 1)
        between = rng.choice((self.a_grid_frame()[:2] + frame, self.a_sparse(frame=frame), self.a_query(), ("render", rng.choice(PRECISIONS), "lean") + frame))
        outk = "lean" if hook == "coarse_weights" else rng.choice(("lean", "full"))      # with given weights the coarse outputs are not written
        self.emit(("hooked", hook, between, ("render_rays", rng.choice(PRECISIONS), outk) + frame))

    def filler(self):
        """A step nobody planned: any call in whatever state the walk is in, or a switch."""
        rng, st = self.rng, self.st
        c = rng.choice(("render", "render", "render", "grid", "sparse", "query", "switch", "switch", "create_rays", "cgrid_weights", "grid_toggle"))
        if c == "render":
            self.emit(self.a_render())
        elif c == "grid":
            self.emit(self.a_grid_frame())
        elif c == "sparse":
            self.emit(self.a_sparse())
        elif c == "query":
            self.emit(self.a_query())
        elif c in ("create_rays", "cgrid_weights"):
            self.emit((c,) + self.frame())
        elif c == "grid_toggle":
            g = rng.choice(("occ", "cgrid", "rgrid"))
            self.grid(g, getattr(st, g) is None)
        else:
            o = rng.choice(("white", "eps", "share_k", "separate", "wq", "cskip", "blocks", "decomp"))
            values = {"white": (False, True), "eps": (0.0, 0.01), "share_k": (1, 2, 4), "separate": (False, True), "wq": (-1, 0, 1),
                      "cskip": (0, 1, 2), "blocks": (False, True), "decomp": (-1, 0, 1, 2)}[o]
            self.emit((o, rng.choice([v for v in values if v != getattr(st, o)])))


@functools.lru_cache(maxsize=None)
def _make_walk(seed, n_steps, share):
    w = Walker(seed)
    stuck = {}
    while True:
        gaps = coverage_gaps(w.cover, share)
        if not gaps and len(w.steps) >= n_steps:
            break
        if gaps and w.rng.random() < 0.7:
            key = w.rng.choice(gaps)[0]
            before = w.cover.get(key, 0)
            w.produce(key)
            if w.cover.get(key, 0) == before:
                stuck[key] = stuck.get(key, 0) + 1
                assert stuck[key] < 8, ("the generator does not produce", key)
        else:
            w.filler()
    w.plain()
    w.emit(w.a_render())            # the walk ends on a comparison
    return tuple(w.steps), dict(w.cover), tuple(w.slots)


def make_walk(index, seed=None, n_steps=None):
    """(steps, coverage counts) of walk `index` of N_WALKS; pure Python, so the coverage is checked without a GPU."""
    steps, cover, _ = _make_walk(seed if seed is not None else WALKS[index][0], n_steps if n_steps is not None else WALKS[index][1], (index, N_WALKS))
    return list(steps), dict(cover)


def predicted_slots(index):
    """Per step of walk `index`: the slot of the render ring the generator says the step's first launch takes."""
    return list(_make_walk(WALKS[index][0], WALKS[index][1], (index, N_WALKS))[2])


def calls_of(step):
    """The render-like calls a step makes, in order, each with the hook armed for it."""
    if step[0] in RENDER_LIKE:
        return [(step, None)]
    if step[0] == "burst":
        return [(c, None) for c in step[1] if c[0] in RENDER_LIKE]
    if step[0] == "hooked":
        return [(step[2], None), (step[3], step[1])]
    return []


# ---- carrying a step out (host-only contexts included) -------------------------------------------------------------------------

def poses_of(n_poses):
    return np.stack([pose_of(-30.0), pose_of(20.0)][:n_poses])


def configure(r, st, grids):
    """All a fresh context is given.  The grids behind the networks: an upload clears them."""
    for which in (0, 1):
        kind, seed, fold = st.nets[which]
        r.debug_set_fold(fold)
        r.set_network(which, state_dict(kind, seed))
    r.set_sampling(st.ns, st.ni)
    for field in State.SETTERS:
        do_setter(r, (field, getattr(st, field)), grids)
    for g in ("occ", "cgrid", "rgrid"):
        if getattr(st, g) is not None:
            do_setter(r, ("set_" + g, getattr(st, g)), grids)


_BAD_NET = None


def do_setter(r, step, grids):
    """A step that is no render-like call and no build, on context r; the refused ones raise the wrapper's exception."""
    op = step[0]
    if op == "net":
        _, which, kind, seed, fold = step
        r.debug_set_fold(fold)
        for w in ((0, 1) if which == 2 else (which,)):
            r.set_network(w, state_dict(kind, seed + w))
    elif op == "sampling":
        r.set_sampling(step[1], step[2])
    elif op in ("set_occ", "set_cgrid", "set_rgrid"):
        g = grids[step[1]]
        if op == "set_occ":
            r.set_occupancy(g["values"], g["lo"], g["hi"], g["res"])
        elif op == "set_cgrid":
            r.set_coarse_grid(g["values"], g["lo"], g["hi"])
        else:
            r.set_radiance_grid(g["values"], g["lo"], g["hi"])
    elif op in ("clear_occ", "clear_cgrid", "clear_rgrid"):
        {"clear_occ": r.clear_occupancy, "clear_cgrid": r.clear_coarse_grid, "clear_rgrid": r.clear_radiance_grid}[op]()
    elif op == "refused_nan_eps":
        r.set_early_termination(float("nan"))
    elif op == "refused_k17":
        r.set_shared_coarse(17)
    elif op.startswith("refused_box_"):
        lo, hi = (0.0, 1.0, 0.0), (1.0, 1.0, 1.0)                       # lo == hi on one axis
        if op.endswith("occ"):
            r.set_occupancy(np.ones((2, 2, 2), bool), lo, hi, (2, 2, 2))
        elif op.endswith("cgrid"):
            r.set_coarse_grid(np.ones((2, 2, 2), np.float32), lo, hi)
        else:
            r.set_radiance_grid(np.ones((2, 2, 2, 4), np.float32), lo, hi)
    elif op == "refused_net":                                           # depth 17: outside the ABI's domain
        global _BAD_NET
        if _BAD_NET is None:
            _BAD_NET = Q.synthetic.make_state_dict(9, 17, 8, skips=())
        r.set_network(0, _BAD_NET)
    else:
        {"white": r.set_white_background, "eps": r.set_early_termination, "share_k": r.set_shared_coarse, "separate": r.set_separate_passes,
         "wq": r.debug_set_work_queue, "cskip": r.debug_set_colour_skip, "blocks": r.debug_set_packet_blocks, "decomp": r.debug_set_decomposition,
         "chunk": r.debug_set_sparse_chunk, "qsteps": r.debug_set_query_steps}[op](step[1])


def do_build(r, st, step):
    """A build step on a device context."""
    op, res, prec = step[0], step[2], step[-1]
    if op == "build_occ":
        r.build_occupancy(BOX_LO, BOX_HI, res, probes=step[3], threshold=step[4], dilate=step[5], precision=prec)
    elif op == "bake_cgrid":
        r.bake_coarse_grid(BOX_LO, BOX_HI, res, precision=prec)
    else:
        r.bake_radiance_grid(BOX_LO, BOX_HI, res, which=step[3], view_dir=None if st.noview(step[3]) else (0.0, 0.6, 0.8), precision=prec)


def read_grid(r, op):
    """The grid a build step made, as `set_*` takes it."""
    if op == "build_occ":
        g, values = r.occupancy, r.occupancy_bits()
    elif op == "bake_cgrid":
        g, values = r.coarse_grid, r.coarse_grid_values()
    else:
        g, values = r.radiance_grid, r.radiance_grid_values()
    return {"values": values, "lo": g["lo"], "hi": g["hi"], "res": g["resolution"]}


def grid_state(r):
    """The three grids as the getters report them: descriptors and values."""
    out = []
    for g, values in ((r.occupancy, r.occupancy_bits), (r.coarse_grid, r.coarse_grid_values), (r.radiance_grid, r.radiance_grid_values)):
        if g is None:
            out.append(None)
        else:
            out.append((g["lo"], g["hi"], g["resolution"], g["inv"].tobytes(), g.get("occupied_cells"), values().tobytes()))
    return out
