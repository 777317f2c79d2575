"""C ABI and module surface of the opt-in input gradient (no GPU needed): seunet_net_input_grad_bytes /
seunet_net_backward_input are declared, bound and exported; the scratch size is positive for valid descriptors and 0 plus a
message for a bad one; the network workspace is unchanged; SE_UNet() keeps input_grad off and out of its state_dict."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("seunet_net_input_grad_bytes", "seunet_net_backward_input")


@pytest.fixture(scope="module")
def lib():
    from seunet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _desc(**kw):
    from seunet_amd import _lib
    from seunet_amd.SE_UNet import make_desc
    a = dict(b=2, in_channel=2, n_classes=1, d=32, h=32, w=32, width_mult=1, dtype=_lib.dtype_code("bf16"), conv_impl=0, slope=0.01)
    a.update(kw)
    return make_desc(a["b"], a["in_channel"], a["n_classes"], a["d"], a["h"], a["w"], a["width_mult"], a["dtype"], a["conv_impl"],
                     a["slope"])


def test_new_entry_points_declared_bound_and_exported(lib):
    from seunet_amd import _lib
    with open(os.path.join(ROOT, "include", "seunet_hip.h")) as f:
        header = f.read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (seunet_[a-z0-9_]+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert name in exported, name
        assert getattr(lib, name) is not None
    assert lib.seunet_version() >= 201


@pytest.mark.parametrize("kw", [{}, dict(in_channel=1), dict(in_channel=3), dict(in_channel=8, width_mult=2), dict(conv_impl=1),
                                dict(n_classes=3), dict(b=1, d=40, h=48, w=56), dict(dtype=0)])
def test_scratch_bytes_cover_the_three_level_terms(lib, kw):
    d = _desc(**kw)
    n = lib.seunet_net_input_grad_bytes(C.byref(d))
    ic, vox = d.in_channel, d.d * d.h * d.w
    need = sum(d.batch * (vox >> (3 * l)) * ic * 4 for l in range(3))        # the three per-level f32 x-branch terms
    assert need <= n < need + 3 * 256


# seunet_net_workspace_bytes of the library before the input gradient existed: the new scratch is separate, the workspace is not
# touched.  (batch, in_channel, n_classes, d, h, w, width_mult, dtype, conv_impl) -> bytes
WORKSPACE_BEFORE = {
    (2, 2, 1, 32, 32, 32, 1, 1, 0): 151843584, (2, 1, 1, 32, 32, 32, 1, 1, 0): 151843584, (2, 3, 1, 32, 32, 32, 1, 0, 0): 262159360,
    (2, 2, 1, 32, 32, 32, 2, 0, 0): 450231040, (2, 2, 3, 32, 32, 32, 1, 0, 1): 268097792, (1, 2, 1, 40, 48, 56, 1, 2, 0): 206767872,
    (4, 2, 1, 128, 128, 128, 1, 1, 0): 11276056832, (1, 8, 1, 64, 64, 64, 2, 1, 1): 845772288,
}


@pytest.mark.parametrize("key", sorted(WORKSPACE_BEFORE))
def test_workspace_bytes_unchanged(lib, key):
    from seunet_amd.SE_UNet import make_desc
    d = make_desc(*key, 0.01)
    assert lib.seunet_net_workspace_bytes(C.byref(d)) == WORKSPACE_BEFORE[key]
    assert lib.seunet_net_input_grad_bytes(C.byref(d)) > 0


@pytest.mark.parametrize("kw", [dict(d=30), dict(in_channel=9), dict(width_mult=3), dict(n_classes=0), dict(dtype=7)])
def test_scratch_bytes_zero_with_a_message_for_a_bad_descriptor(lib, kw):
    from seunet_amd import _lib
    d = _desc(**kw)
    assert lib.seunet_net_input_grad_bytes(C.byref(d)) == 0
    assert "net" in _lib.last_error()
    assert lib.seunet_net_input_grad_bytes(None) == 0
    assert "null" in _lib.last_error()


def test_module_default_is_off_and_not_state():
    import seunet_amd as A
    m = A.SE_UNet()
    assert m.input_grad is False
    on = A.SE_UNet(in_channel=2, input_grad=True)
    assert on.input_grad is True
    assert not any("input_grad" in k for k in on.state_dict())
    assert list(on.state_dict().keys()) == list(A.SE_UNet(in_channel=2).state_dict().keys())
