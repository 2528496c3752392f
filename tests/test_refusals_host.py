"""Whether a call runs and with which words it is refused, without a GPU (csrc/nwe_check.cpp): plain C++ that compiles without
ROCm; every call of tests/refusal_domain.py against a recording of what the code it replaced answered
(tests/golden/refusal_table.npz, whose header says which commit's library produced it and how - a recording of this project's own
earlier code, never of the code under test), code and text compared with ==; what the recording must cover to mean anything; and
the checks that no host-only context reaches, asked directly by a stand-alone program."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from nwe_amd import _lib
from tests import refusal_domain as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-workspaces-explorer_amd", "csrc")
PARENT = "e6a1ff6"

MFMA_SENTENCE = ("no MFMA kernel for this network shape (have widths 128 and 256 with depth 6 or 8 and the skip after layer 4, or depth 4 without, "
                 "63 + 27 or, without view directions, 63 inputs); use NWE_PREC_F32")

# Every literal of the refusals that check_ready, check_lean_mode, check_camera, the two box checks and the network / sampling checks
# of commit e6a1ff6 spelled out (nwe_abi.hip there), whole texts and the fragments its texts were put together from.
PARENT_LITERALS = (
    # check_ready
    "null context or outputs",
    "nwe_outputs.struct_bytes != sizeof(nwe_outputs): the caller was built against another version of include/nwe.h",
    "host-only context cannot render", "nwe_set_sampling has not been called", "coarse network not set", "fine network not set but n_importance > 0",
    "unknown precision", "coarse and fine networks must both have, or both lack, view directions",
    "coarse and fine networks must share their encodings: in_xyz ", ", in_dir ", " (coarse / fine)",
    "feat_map is the fine pass's view-layer output: it needs n_importance > 0 and networks with view directions",
    "feat_map (endpoint_feat) is computed by the NWE_PREC_F32 kernel only", MFMA_SENTENCE,
    "the MFMA kernel supports n_samples <= 128; use NWE_PREC_F32",
    "the shared coarse pass is on (nwe_set_shared_coarse, k = ",
    "it is not built together with early termination (nwe_set_early_termination, min_transmittance = ", "); switch one of them off",
    "; set shared_coarse to 1 for this call", "nwe_render_rays has no pixel grid to share over",
    "early termination is on (nwe_set_early_termination, min_transmittance = ", "; set min_transmittance to 0 for this call",
    "nwe_render_rays, its hooks and its training tables are not terminated",
    "separate passes are on (nwe_set_separate_passes): ", "; set separate_passes to 0 for this call",
    "they are not built together with early termination (nwe_set_early_termination, min_transmittance = ",
    "), which would need terminating consumer kernels; switch one of them off",
    "coarse and fine networks must be packed in the same formulation (nwe_debug_set_fold); use NWE_PREC_F32",
    "an occupancy grid is set (nwe_set_occupancy, ", "; call nwe_clear_occupancy for this call",
    "it is not built together with the shared coarse pass (nwe_set_shared_coarse, k = ",
    "it is not built together with separate passes (nwe_set_separate_passes); switch one of them off",
    "nwe_render_rays, its hooks and its training tables do not read the grid",
    "a stamped launch (nwe_debug_set_stamps) has no occupancy kernel",
    "a coarse density grid is set (nwe_set_coarse_grid, ", "; call nwe_clear_coarse_grid for this call",
    "it is not built together with an occupancy grid (nwe_set_occupancy); clear one of them",
    "a stamped launch (nwe_debug_set_stamps) has no sharing kernel",
    # check_lean_mode
    "only rgb / depth / acc / flags can be requested", "a network packed unfolded (nwe_debug_set_fold(0)) has no ", " MFMA kernel",
    " MFMA kernel was built for this network shape", "; use NWE_PREC_F32",
    "sharing MFMA kernel", "terminating MFMA kernel", "occupancy MFMA kernel",
    "no sharing MFMA kernel was built", "no terminating MFMA kernel was built", "no occupancy MFMA kernel was built",
    # check_camera
    "bad pose / image / row range", "bad pose / image", "fx and fy must be non-zero",
    "far < near: the sorted merge of the fine pass needs ascending depths", "far < near: nwe_render_rays needs near <= far on every ray",
    # the ray limits of nwe_render / nwe_render_rays
    "more than 2^31 - 1 rays in one call", "bad rays (null, or more than 2^31 - 1)",
    # check_occupancy_box, check_coarse_grid_box and the setters behind them
    "occupancy: null lo, hi or resolution", "occupancy: the box must be finite", "occupancy: the box must have lo < hi on every axis",
    "occupancy: the resolution must be in 1..1024 on every axis", "occupancy: the grid must have fewer than 2^31 cells",
    "occupancy: null bits", "occupancy: a host-only context takes its bits from the host",
    "coarse grid: null lo, hi or resolution", "coarse grid: the box must be finite", "coarse grid: the box must have lo < hi on every axis",
    "coarse grid: the resolution must be in 1..512 on every axis", "coarse grid: the box must be finite (resolution / (hi - lo) is not, in fp32)",
    "coarse grid: null sigma", "coarse grid: a host-only context takes its values from the host",
    # check_network_head, nwe_set_network*, set_network, nwe_set_sampling, the mode setters
    "null argument", "which must be 0 or 1", "depth must be in 1..16", "width must be even and <= 256",
    "encoded widths must be 3 + 6*num_freqs (xyz <= 93, dir <= 63)", "encoded width must be 3 + 6*num_freqs (<= 93)",
    "output_ch must be in 4..256 (rgb_raw, sigma_raw, ignored rest)", "null weight or bias pointer",
    "n_samples must be in 2..128", "n_importance must be in 0..256", "importance sampling needs u and n_samples >= 3",
    "min_transmittance must be in [0, 1) (0 = off)", "shared_coarse k must be in 1..16 (1 = off)", "separate_passes must be 0 or 1 (0 = off)",
)

# The literals above that no call on a host-only context can be refused with, each with its reason.  The two dead ones are gone from
# the code; the camera's are asked directly below (test_the_checks_no_host_only_context_reaches).
UNREACHABLE = {
    "the MFMA kernel supports n_samples <= 128; use NWE_PREC_F32":
        "never fired: nwe_set_sampling lets at most 128 = kSplitMaxSamples samples through (static_assert in nwe_check.cpp)",
    "occupancy: the grid must have fewer than 2^31 cells":
        "never fired: the resolution check in front of it leaves at most 1024^3 = 2^30 cells",
    "bad pose / image":
        "nwe_render_tiled's word for it, which refuses host-only contexts first",
    "fx and fy must be non-zero":
        "nwe_debug_plan takes no intrinsics (it checks a camera with fx = fy = 1); every entry point that does needs a device before it checks them",
    "far < near: the sorted merge of the fine pass needs ascending depths":
        "nwe_debug_plan takes no depth range (near = far = 0); nwe_render refuses a host-only context in front of its camera",
    "far < near: nwe_render_rays needs near <= far on every ray":
        "nwe_create_rays' word for it, which needs a device context first",
}

EXCLUSIVE_PAIRS = (("share_k", "min_trans"), ("separate", "min_trans"), ("occ", "min_trans"), ("occ", "share_k"), ("occ", "separate"),
                   ("cgrid", "min_trans"), ("cgrid", "share_k"), ("cgrid", "separate"), ("cgrid", "occ"))
MODE_FIELDS = ("share_k", "min_trans", "separate", "occ", "cgrid", "stamps")


def test_the_checks_compile_without_rocm(tmp_path):
    """nwe_check.cpp is plain C++17, like the planner: g++ with every warning an error and no ROCm include path."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(CSRC, "nwe_check.cpp"), "-o", str(tmp_path / "nwe_check.o")], check=True)
    for name in ("nwe_check.cpp", "nwe_check.h", "nwe_plan.cpp", "nwe_plan.h"):
        assert "hip" not in open(os.path.join(CSRC, name)).read().replace("HIP", "").replace(".hip", ""), name


def test_the_checks_no_host_only_context_reaches(tmp_path):
    """tests/c/check_smoke.cpp asks nwe_check.cpp directly what only a device context is asked through the ABI: the camera's
    intrinsics and depth range, nwe_query_points, nwe_build_occupancy and nwe_bake_coarse_grid in front of their device."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "check_smoke")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "c", "check_smoke.cpp"),
                    os.path.join(CSRC, "nwe_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "check_smoke ok", done.stdout + done.stderr


@pytest.fixture(scope="module")
def table():
    t = np.load(os.path.join(ROOT, "tests", "golden", "refusal_table.npz"))
    assert PARENT in str(t["header"]) and "tools/record_refusals.py" in str(t["header"])
    return {"codes": t["codes"].tolist(), "texts": [str(s) for s in t["texts"]], "rows": t["rows"].astype(np.int64), "cases": str(t["cases"])}


@pytest.fixture(scope="module")
def walked():
    """The walk on the library under test, once: (cases, codes, texts)."""
    cases, codes, texts = [], [], []
    for case, code, text in D.walk():
        cases.append(case); codes.append(code); texts.append(text)
    return cases, codes, texts


def test_every_call_is_refused_as_recorded(table, walked):
    cases, codes, texts = walked
    h = hashlib.sha256()
    for case in cases:
        h.update(repr(case).encode())
    assert h.hexdigest() == table["cases"], "the walk is not the recorded one: record again from a library of the recorded commit"
    assert len(cases) == len(table["rows"])
    want_codes, want_texts = table["codes"], table["texts"]
    bad = [(case, (code, text), (want_codes[row], want_texts[row])) for case, code, text, row in zip(cases, codes, texts, table["rows"].tolist())
           if code != want_codes[row] or text != want_texts[row]]
    assert not bad, (len(bad), bad[:3])


def test_the_recording_covers_what_the_replaced_checks_said(table):
    texts = table["texts"]
    assert len(set(PARENT_LITERALS)) == len(PARENT_LITERALS) and set(UNREACHABLE) <= set(PARENT_LITERALS)
    missing = [s for s in PARENT_LITERALS if s not in UNREACHABLE and not any(s in t for t in texts)]
    assert not missing, missing
    # ... and an exception is one: "bad pose / image" is the only literal that is a prefix of a reachable one
    for s in UNREACHABLE:
        assert not any(s in t for t in texts if not (s == "bad pose / image" and t == "bad pose / image / row range")), s
    # every code occurs, and every text belongs to the calls of this domain
    assert set(table["codes"]) == {_lib.NWE_OK, _lib.NWE_ERR_INVALID, _lib.NWE_ERR_UNSUPPORTED, _lib.NWE_ERR_STATE}


def test_every_exclusive_pair_occurs_under_all_three_precisions(table, walked):
    """The two modes of a pair on and nothing else, a lean pinhole frame of networks that every mode has kernels for: refused under
    the MFMA precisions by the pair's own text, and under NWE_PREC_F32 too unless the refusing mode is separate passes."""
    cases, _, _ = walked
    index = {case: i for i, case in enumerate(cases) if case[0] == "plan" and len(case) == 8}
    on = {"share_k": 2, "min_trans": 0.25, "separate": 1, "occ": 1, "cgrid": 1}
    name = {"share_k": "the shared coarse pass", "min_trans": "early termination", "separate": "separate passes", "occ": "an occupancy grid",
            "cgrid": "a coarse density grid"}
    for mode, other in EXCLUSIVE_PAIRS:
        modes = tuple(on[f] if f in (mode, other) else D.PLAIN[i] for i, f in enumerate(MODE_FIELDS))
        for precision in (_lib.PREC_F16X3, _lib.PREC_F16X1, _lib.PREC_F32):
            row = table["rows"][index[("plan", "folded", (8, 8), modes, precision, "lean", "pinhole", 8)]]
            code, text = table["codes"][row], table["texts"][row]
            if mode == "separate" and precision == _lib.PREC_F32:
                assert (code, text) == (_lib.NWE_OK, ""), (mode, other, text)   # fp32 ignores separate passes, and terminates lean frames
                continue
            assert code == _lib.NWE_ERR_UNSUPPORTED and text.startswith(name[mode]) and " not built together with " + name[other] + " (" in text, \
                (mode, other, precision, text)
