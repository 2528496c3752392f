"""The shared coarse pass without a GPU: the block arithmetic against a brute-force double loop, the setter's domain and the
getter on a host-only context, the handler's keyword and environment variable, and the conditioning of the reference the GPU
tests compare with."""
import ctypes as C

import numpy as np
import pytest
import torch

import nwe_amd
from nwe_amd import _lib
from tests import early_termination as E
from tests import shared_coarse as SC

SIZES = (1, 2, 7, 19)
KS = (1, 2, 3, 4, 16)


def _tiles(H):
    """The whole frame and unaligned row tiles: every split in two, and single rows."""
    return [(0, H)] + [(0, c) for c in range(1, H)] + [(c, H) for c in range(1, H)] + [(c, c + 1) for c in range(H)]


def _brute(H, W, k, r0, r1, n_poses):
    out = []
    for p in range(n_poses):
        for h in range(r0, r1):
            for w in range(W):
                bh, bw = h // k, w // k                           # the block, on the grid of the whole image
                rh, rw = min(k * bh + k // 2, H - 1), min(k * bw + k // 2, W - 1)
                assert rh // k == bh and rw // k == bw            # the representative is a pixel of its own block
                out.append((p * H + rh) * W + rw)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("W", SIZES)
def test_rep_index_against_a_double_loop(H, W):
    for k in KS:
        for r0, r1 in _tiles(H):
            for n_poses in (1, 2):
                got = SC.rep_index(H, W, k, r0, r1, n_poses)
                assert np.array_equal(got, _brute(H, W, k, r0, r1, n_poses)), (H, W, k, r0, r1, n_poses)
                if k == 1:                                      # every pixel is its own representative
                    assert np.array_equal(got, SC.rep_index(H, W, 1, 0, H, n_poses).reshape(n_poses, H, W)[:, r0:r1].reshape(-1))


@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("W", SIZES)
def test_n_rep_counts_the_distinct_representatives_of_a_tile(H, W):
    for k in KS:
        for r0, r1 in _tiles(H):
            for n_poses in (1, 2):
                assert SC.n_rep(H, W, k, r0, r1, n_poses) == len(np.unique(SC.rep_index(H, W, k, r0, r1, n_poses))), (H, W, k, r0, r1)
        assert SC.n_rep(H, W, k, 0, 0, 1) == 0
    # a tile's rows are the frame's rows: row tiles look up the same representatives as the frame
    whole = SC.rep_index(7, 19, 3, 0, 7, 2).reshape(2, 7, 19)
    parts = [SC.rep_index(7, 19, 3, r0, r1, 2).reshape(2, r1 - r0, 19) for r0, r1 in ((0, 3), (3, 6), (6, 7))]
    assert np.array_equal(whole, np.concatenate(parts, 1))


def test_evaluation_arithmetic():
    """7 x 19, k = 4, 64 + 128: 2 x 5 blocks; rows [3, 6) touch both block rows, rows [4, 7) only the second."""
    assert SC.n_rep(7, 19, 4, 0, 7, 1) == 10 and SC.n_rep(7, 19, 4, 3, 6, 1) == 10 and SC.n_rep(7, 19, 4, 4, 7, 1) == 5
    assert SC.evaluations(7, 19, 4, 0, 7, 1, 64, 128) == (10 * 64 + 133 * 192, 133 * 256)
    assert SC.evaluations(7, 19, 4, 4, 7, 2, 64, 128) == (10 * 64 + 114 * 192, 114 * 256)
    assert SC.evaluations(7, 19, 1, 0, 7, 1, 64, 128) == (133 * 256,) * 2
    assert SC.evaluations(7, 19, 4, 0, 7, 1, 32, 0) == (133 * 32,) * 2
    # the issue's table: an aligned frame at k = 2 / 4 loses 3/4 / 15/16 of its coarse evaluations
    for k, kept in ((2, 4), (4, 16)):
        ran, full = SC.evaluations(800, 800, k, 0, 800, 1, 64, 128)
        assert full - ran == 640000 * 64 - 640000 * 64 // kept


def test_setter_domain_and_getter_on_a_host_only_context():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    assert r.shared_coarse == 1
    for k in (2, 16, 3):
        r.set_shared_coarse(k)
        assert r.shared_coarse == k
    for bad in (0, -1, 17, 1 << 20):
        with pytest.raises(ValueError, match="shared_coarse"):
            r.set_shared_coarse(bad)
        assert lib.nwe_set_shared_coarse(r._ctx, bad) == _lib.NWE_ERR_INVALID
        assert r.shared_coarse == 3                                  # the previous value stays
    r.set_shared_coarse(1)
    assert r.shared_coarse == 1
    assert lib.nwe_set_shared_coarse(None, 2) == _lib.NWE_ERR_INVALID and lib.nwe_get_shared_coarse(None) == -1
    # the two settings are independent on the context: their combination is refused by the render calls
    r.set_early_termination(1e-2); r.set_shared_coarse(4)
    assert r.shared_coarse == 4 and r.early_termination == np.float32(1e-2)
    # nothing was launched on a host-only context
    ms, rays = C.c_float(7.0), C.c_int64(7)
    assert lib.nwe_last_coarse_launch(r._ctx, C.byref(ms), C.byref(rays)) == _lib.NWE_ERR_STATE and (ms.value, rays.value) == (-1.0, 0)
    assert lib.nwe_last_coarse_launch(r._ctx, None, C.byref(rays)) == _lib.NWE_ERR_INVALID
    with pytest.raises(RuntimeError, match="nothing has been launched"):
        r.last_coarse_launch()
    r.close()


def test_handler_keyword_and_environment_variable(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    assert H("office_geneve", "x.ckpt").shared_coarse == 1
    assert H("office_geneve", "x.ckpt", shared_coarse=4).shared_coarse == 4
    monkeypatch.setenv("NWE_SHARED_COARSE", "2")
    assert H("office_geneve", "x.ckpt").shared_coarse == 2
    assert H("office_geneve", "x.ckpt", shared_coarse=4).shared_coarse == 4      # the keyword wins
    for bad in (0, 17, -2, 2.0, True):
        with pytest.raises(ValueError, match="shared_coarse"):
            H("office_geneve", "x.ckpt", shared_coarse=bad)
    monkeypatch.setenv("NWE_SHARED_COARSE", "32")
    with pytest.raises(ValueError, match="shared_coarse"):
        H("office_geneve", "x.ckpt")
    # refused together with early termination, however either arrives
    monkeypatch.setenv("NWE_SHARED_COARSE", "2")
    with pytest.raises(ValueError, match="shared_coarse.*early_termination"):
        H("office_geneve", "x.ckpt", early_termination=1e-3)
    monkeypatch.delenv("NWE_SHARED_COARSE")
    monkeypatch.setenv("NWE_EARLY_TERMINATION", "0.01")
    with pytest.raises(ValueError, match="shared_coarse.*early_termination"):
        H("office_geneve", "x.ckpt", shared_coarse=2)
    assert H("office_geneve", "x.ckpt").shared_coarse == 1


@pytest.mark.parametrize("name", ["thin", "mixed"])
@pytest.mark.parametrize("k", [2, 4])
def test_reference_is_well_conditioned_on_the_parity_scenes(name, k):
    """The GPU tests hold the kernels to rgb 1e-4, depth 1e-4 * far, acc 1e-4 against `shared_reference`.  That means something
    only where the reference reproduces itself: in fp32 it agrees with the same rule applied to the oracle's fp64 evaluation
    to a tenth of that on every ray (both scenes keep a thin fog in their coarse network, whose importance sampling has no
    nearly empty bins: tests/early_termination.py).  And the rule bites: some rays differ from the ordinary frame."""
    ref, ref64 = SC.shared_reference(name, k), SC.shared_reference(name, k, torch.float64)
    for key, tol in (("rgb", 1e-5), ("depth", 1e-5 * E.FAR), ("acc", 1e-5)):
        err = float((ref[key].double() - ref64[key]).abs().max())
        print(f"{name} k {k} {key}: fp32 vs fp64 reference {err:.2e} (bound {tol:.0e})")
        assert err <= tol, (name, k, key, err)
    plain = E.scene(name)[5]
    rep = SC.rep_index(*E.SCENES[name][6:8], k, 0, E.SCENES[name][6], 1)
    own = rep == np.arange(len(rep))
    assert 0 < own.sum() < len(rep)
    # a representative renders the ordinary frame's bits, the others take someone else's depths
    assert torch.equal(ref["rgb"][own], plain["rgb_fine"][own])
    assert not torch.equal(ref["rgb"][~own], plain["rgb_fine"][~own])
