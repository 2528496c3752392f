"""Separate passes without a GPU (include/nwe.h: nwe_set_separate_passes): the setter's domain and the getter on a host-only
context, the place of the new refusals in the documented order, and the handler's keyword and environment variable."""
import ctypes as C

import pytest

import nwe_amd
from nwe_amd import _lib, synthetic


def test_default_setter_domain_and_getter_on_a_host_only_context():
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    try:
        assert r.separate_passes is False and lib.nwe_get_separate_passes(r._ctx) == 0
        r.set_separate_passes(True)
        assert r.separate_passes is True and lib.nwe_get_separate_passes(r._ctx) == 1
        for bad in (2, -1, 256, 1 << 20):
            assert lib.nwe_set_separate_passes(r._ctx, bad) == _lib.NWE_ERR_INVALID
            assert b"separate_passes" in lib.nwe_last_error(r._ctx)
            assert lib.nwe_get_separate_passes(r._ctx) == 1                # the previous value stays
        r.set_separate_passes(False)
        assert r.separate_passes is False
        assert lib.nwe_set_separate_passes(None, 1) == _lib.NWE_ERR_INVALID and lib.nwe_get_separate_passes(None) == -1
        # independent of the two other opt-in modes on the context: the combinations are judged by the render calls
        r.set_early_termination(1e-2); r.set_shared_coarse(4); r.set_separate_passes(True)
        assert (r.separate_passes, r.shared_coarse) == (True, 4) and r.early_termination > 0
        # nothing was launched on a host-only context
        ms, rays = C.c_float(7.0), C.c_int64(7)
        assert lib.nwe_last_coarse_launch(r._ctx, C.byref(ms), C.byref(rays)) == _lib.NWE_ERR_STATE and (ms.value, rays.value) == (-1.0, 0)
    finally:
        r.close()


def _render(r, lib, precision, outputs=None):
    """nwe_render on a host-only context: every refusal but "host-only context cannot render" needs a device, so the order is
    read off the error text of calls that fail earlier or exactly there."""
    o = outputs or _lib.Outputs()
    pose = (C.c_float * 16)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]))
    rc = lib.nwe_render(r._ctx, C.cast(pose, C.c_void_p), 1, 4, 4, 2.0, 2.0, 1.5, 1.5, 0.1, 10.0, 0, 4, precision, C.byref(o), None)
    return rc, lib.nwe_last_error(r._ctx).decode()


def test_the_refusals_every_call_has_come_before_the_modes():
    """check_ready's order: the outputs struct, the host-only context, and only then anything the modes refuse - with early
    termination, the shared coarse pass and separate passes all on, a host-only context still says the first thing wrong."""
    r = nwe_amd.Renderer(host_only=True)
    lib = _lib.load()
    try:
        r.set_network(0, synthetic.make_state_dict(1000, 4, 128)); r.set_network(1, synthetic.make_state_dict(1001, 8, 256))
        r.set_sampling(64, 128)
        r.set_early_termination(1e-2); r.set_separate_passes(True)
        bad = _lib.Outputs()
        bad.struct_bytes = 8
        rc, msg = _render(r, lib, _lib.PREC_F16X3, bad)
        assert rc == _lib.NWE_ERR_INVALID and "struct_bytes" in msg
        for precision in (_lib.PREC_F16X3, _lib.PREC_F32):
            rc, msg = _render(r, lib, precision)
            assert rc == _lib.NWE_ERR_STATE and "host-only" in msg and "separate" not in msg
        # both shapes keep their MFMA packing side by side: nothing about the pair is refused when the networks are set
        assert r.mfma_supported(0) and r.mfma_supported(1) and r.shapes[0] != r.shapes[1]
    finally:
        r.close()


def test_handler_keyword_and_environment_variable(monkeypatch):
    H = nwe_amd.NeRFReplicaInferenceHandler
    assert H("office_geneve", "x.ckpt").separate_passes is False
    assert H("office_geneve", "x.ckpt", separate_passes=True).separate_passes is True
    monkeypatch.setenv("NWE_SEPARATE_PASSES", "1")
    assert H("office_geneve", "x.ckpt").separate_passes is True
    assert H("office_geneve", "x.ckpt", separate_passes=False).separate_passes is False      # the keyword wins
    monkeypatch.setenv("NWE_SEPARATE_PASSES", "0")
    assert H("office_geneve", "x.ckpt").separate_passes is False
    assert H("office_geneve", "x.ckpt", separate_passes=True).separate_passes is True
    for bad in (2, 0, 1, "1", 1.0):
        with pytest.raises(ValueError, match="separate_passes"):
            H("office_geneve", "x.ckpt", separate_passes=bad)
    monkeypatch.setenv("NWE_SEPARATE_PASSES", "yes")
    with pytest.raises(ValueError, match="separate_passes"):
        H("office_geneve", "x.ckpt")
    # refused together with early termination, however either arrives
    monkeypatch.setenv("NWE_SEPARATE_PASSES", "1")
    with pytest.raises(ValueError, match="separate_passes.*early_termination"):
        H("office_geneve", "x.ckpt", early_termination=1e-3)
    monkeypatch.delenv("NWE_SEPARATE_PASSES")
    monkeypatch.setenv("NWE_EARLY_TERMINATION", "0.01")
    with pytest.raises(ValueError, match="separate_passes.*early_termination"):
        H("office_geneve", "x.ckpt", separate_passes=True)
    assert H("office_geneve", "x.ckpt").separate_passes is False
    # the shared coarse pass composes with it
    monkeypatch.delenv("NWE_EARLY_TERMINATION")
    h = H("office_geneve", "x.ckpt", separate_passes=True, shared_coarse=2)
    assert (h.separate_passes, h.shared_coarse) == (True, 2)
