"""The packed MFMA stream, bias table, scale and flop count of every instantiated shape, in all three forms and at four
weight magnitudes, pinned byte for byte (sha256) to tests/golden/pack_digests.json.  The json records what the library
packed BEFORE the packers moved out of the HIP translation unit into csrc/nwe_pack.cpp: any change in how the fp64 fold
sums, how (hi, lo) splits round or how the scale exponent clamps shows here without a GPU.  The fp32 blob is not readable
through the ABI; the bitwise f32 GPU tests cover it.

Regenerate (only when the packing is MEANT to change) with `python -m tests.test_pack_digests` from the repository root;
NWE_LIB selects the library that is asked."""
import hashlib
import json
import os

import numpy as np
import pytest

import nwe_amd
from nwe_amd import synthetic

JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")
SHAPES = [(256, 8, (4,)), (256, 6, (4,)), (256, 4, ()), (128, 8, (4,)), (128, 6, (4,)), (128, 4, ())]   # (W, D, skips)
FORMS = ("folded", "reference", "noview")   # reference: debug_set_fold(False); only 8x256 and 4x128 have such a stream
# x1; x2^-20 and x2^12 reach the upper (30) and lower (-14) clamp of the scale exponent; x0 takes the wmax == 0 branch
GAINS = (("plain", 1.0), ("tiny", 2.0 ** -20), ("huge", 2.0 ** 12), ("zero", 0.0))
CASES = [(W, D, skips, form, gain) for W, D, skips in SHAPES for form in FORMS for gain, _ in GAINS]


def case_id(W, D, form, gain):
    return f"{D}x{W}-{form}-{gain}"


def digest(W, D, skips, form, gain):
    sd = synthetic.make_state_dict(100 + D + W, D, W, skips=skips, use_view_dirs=form != "noview")
    mul = np.float32(dict(GAINS)[gain])
    sd = {k: (v * mul).astype(np.float32) for k, v in sd.items()}
    r = nwe_amd.Renderer(host_only=True)
    r.debug_set_fold(form != "reference")
    r.set_network(0, sd)
    stream, bias = r.packed_stream(0), r.packed_bias(0)
    h = hashlib.sha256()
    h.update(stream.tobytes())
    h.update(bias.tobytes())
    out = {"sha256": h.hexdigest(), "scale": float(r.packed_scale(0)), "flops": int(r.flops_per_eval(0)),
           "stream_bytes": int(stream.size), "bias_shape": [int(d) for d in bias.shape]}
    r.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(JSON) as f:
        return json.load(f)


def test_json_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(case_id(W, D, form, gain) for W, D, _, form, gain in CASES) and len(golden) == 72


@pytest.mark.parametrize("W,D,skips,form,gain", CASES, ids=[case_id(W, D, form, gain) for W, D, _, form, gain in CASES])
def test_packed_network_is_what_it_was(golden, W, D, skips, form, gain):
    assert digest(W, D, skips, form, gain) == golden[case_id(W, D, form, gain)]


if __name__ == "__main__":
    with open(JSON, "w") as f:
        json.dump({case_id(W, D, form, gain): digest(W, D, skips, form, gain) for W, D, skips, form, gain in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", JSON, "from", nwe_amd._lib.LIB_PATH)
