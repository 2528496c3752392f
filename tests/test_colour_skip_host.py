"""The pack-time condition of the hollow path (csrc/nwe_pack.cpp: Packed::colour_finite; include/nwe.h: nwe_packed_colour_finite),
on a host-only context: set once per set_network for a folded network whose colour layers are finite AS PACKED - the folded view
layer formed in fp64 with its view-direction columns, the rgb head, both biases.  The trunk and the density head have no say.
The flag travels neither in the packed stream nor in the bias table (tests/test_pack_digests.py pins their bytes)."""
import numpy as np
import pytest

import nwe_amd
from nwe_amd import synthetic


def _flag(sd, fold=True):
    r = nwe_amd.Renderer(host_only=True)
    try:
        r.debug_set_fold(fold)
        r.set_network(0, sd)
        return r.packed_colour_finite(0)
    finally:
        r.close()


def _spoiled(D, W, key, idx, value):
    sd = synthetic.make_state_dict(1001, D, W)
    sd[key] = sd[key].copy()
    sd[key][idx] = np.float32(value)
    return sd


@pytest.mark.parametrize("D,W", [(8, 256), (4, 128)])
def test_finite_colour_layers(D, W):
    assert _flag(synthetic.make_state_dict(1001, D, W))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("key,idx", [("_rgb_linear.weight", (1, 3)), ("_rgb_linear.bias", (2,)), ("_views_linears.0.weight", (5, 7)),
                                     ("_views_linears.0.weight", (5, 128 + 20)), ("_views_linears.0.bias", (9,)),
                                     ("_feature_linear.weight", (3, 4)), ("_feature_linear.bias", (11,))])
def test_non_finite_colour_layers(key, idx, value):
    """Every layer the colour depends on behind the trunk: the rgb head, the view layer (a trunk-feature column and a gamma(d)
    column), the feature layer that is folded into it, and their biases."""
    assert not _flag(_spoiled(4, 128, key, idx, value))


@pytest.mark.parametrize("key,idx", [("_pts_linears.2.weight", (5, 7)), ("_pts_linears.0.bias", (1,)), ("_alpha_linear.weight", (0, 9)),
                                     ("_alpha_linear.bias", (0,))])
def test_trunk_and_density_head_have_no_say(key, idx):
    """A NaN there reaches sigma, and a NaN sigma never takes the path (csrc/nwe_mfma_eval.h)."""
    assert _flag(_spoiled(4, 128, key, idx, np.nan))


def test_a_fold_that_overflows():
    """All weights finite, but their product is not what fp16 (weights) or fp32 (bias) can hold."""
    sd = synthetic.make_state_dict(1001, 4, 128)
    for k in ("_views_linears.0.weight", "_feature_linear.weight"):
        sd[k] = (sd[k] * np.float32(1e25)).astype(np.float32)
    assert all(np.isfinite(v).all() for v in sd.values())
    assert not _flag(sd)
    sd = synthetic.make_state_dict(1001, 4, 128)
    sd["_views_linears.0.weight"] = (sd["_views_linears.0.weight"] * np.float32(1e3)).astype(np.float32)
    sd["_feature_linear.bias"] = (sd["_feature_linear.bias"] + np.float32(1e37)).astype(np.float32)
    assert all(np.isfinite(v).all() for v in sd.values())
    assert not _flag(sd)   # the folded bias b_v + W_v b_f is beyond fp32


def test_a_large_but_representable_colour_layer():
    sd = synthetic.make_state_dict(1001, 4, 128)
    sd["_rgb_linear.weight"] = (sd["_rgb_linear.weight"] * np.float32(1e6)).astype(np.float32)
    assert _flag(sd)   # the scale of the stream follows the largest weight


def test_other_formulations_have_no_path():
    assert not _flag(synthetic.make_state_dict(1001, 4, 128), fold=False)
    assert not _flag(synthetic.make_state_dict(1001, 4, 128, use_view_dirs=False))
    r = nwe_amd.Renderer(host_only=True)
    try:
        assert not r.packed_colour_finite(0)   # not set
    finally:
        r.close()
