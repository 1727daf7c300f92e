"""CPU: the boundary of activation recomputation -- the header declares ``mdm_gn_reapply`` and the library exports it without
an ABI bump, the switch defaults to off and round-trips, the ops refuse CPU tensors, and the entry point rejects bad
arguments with a message before any launch."""
import ctypes
import re

import pytest
import torch

import recompute_cases as RC
from mdm_hip import _lib


def test_header_declares_and_library_exports_gn_reapply_without_an_abi_bump():
    protos = {name: (argtypes, argnames) for name, _, argtypes, argnames in _lib.header_prototypes()}
    assert "mdm_gn_reapply" in protos
    argtypes, argnames = protos["mdm_gn_reapply"]
    assert argnames == ["x", "coef", "y", "N", "HW", "C", "act", "p", "seed", "offset", "dtype", "stream"]
    assert argtypes[7] is ctypes.c_float and argtypes[8] is ctypes.c_ulonglong and argtypes[9] is ctypes.c_ulonglong
    L = _lib.lib()
    assert hasattr(L, "mdm_gn_reapply")
    assert _lib.ABI_VERSION == 6 and L.mdm_abi_version() == 6
    text = open(_lib.HEADER).read()
    decl = text[:text.index("int mdm_gn_reapply(")]
    comment = decl[decl.rindex("/*"):]
    assert re.search(r"unet\.py:224, 233-234", comment)   # the reference lines the entry stands for


def test_switch_defaults_to_off_and_round_trips():
    import mdm_hip
    from mdm_hip import ops

    assert mdm_hip.enable_activation_recompute is ops.enable_activation_recompute
    assert mdm_hip.activation_recompute_enabled is ops.activation_recompute_enabled
    assert ops.activation_recompute_enabled() is False
    try:
        ops.enable_activation_recompute(True)
        assert ops.activation_recompute_enabled() is True
        ops.enable_activation_recompute(0)
        assert ops.activation_recompute_enabled() is False
    finally:
        ops.enable_activation_recompute(False)


def test_ops_refuse_cpu_tensors():
    from mdm_hip import ops

    x = torch.randn(2, 4, 4, 32)
    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.gn_reapply(x, torch.zeros(2, 32, 2))
    w = torch.randn(32, 32, 3, 3, requires_grad=True)
    with pytest.raises(_lib.MdmHipError, match="no CPU fallback"):
        ops.gn_conv(x, torch.ones(32), torch.zeros(32), 8, w, torch.zeros(32))


def test_gn_conv_checks_its_arguments_on_the_host():
    from mdm_hip import ops

    x = torch.randn(2, 4, 4, 32)
    with pytest.raises(_lib.MdmHipError, match="3x3"):
        ops.gn_conv(x, torch.ones(32), torch.zeros(32), 8, torch.randn(32, 32, 1, 1))
    w = torch.randn(32, 32, 3, 3)
    with pytest.raises(_lib.MdmHipError, match="outside"):
        ops.gn_conv(x, torch.ones(32), torch.zeros(32), 8, w, p=1.0)
    with pytest.raises(_lib.MdmHipError, match="multiple of 8"):
        ops.gn_conv(torch.randn(1, 1, 3, 4), torch.ones(4), torch.zeros(4), 1, torch.randn(4, 4, 3, 3), p=0.1)


def _reapply(x=1, coef=1, y=1, N=2, HW=16, C=32, act=1, p=0.0, dtype=1):
    """the entry point with made-up non-null pointers: every call here must be rejected before anything is launched"""
    L = _lib.lib()
    rc = L.mdm_gn_reapply(x or None, coef or None, y or None, N, HW, C, act, p, 5, 0, dtype, None)
    msg = L.mdm_last_error()
    return rc, (msg.decode() if msg else "")


@pytest.mark.parametrize("kw,needle", [
    (dict(C=36, dtype=1), "C % epv"),             # bf16: not whole 16-byte chunks (8 elements)
    (dict(C=34, dtype=0), "C % epv"),             # fp32: not whole 16-byte chunks (4 elements)
    (dict(p=1.0), "p < 1.f"),
    (dict(p=1.5), "p < 1.f"),
    (dict(p=-0.1), "p >= 0.f"),
    (dict(N=1, HW=3, C=4, dtype=0, p=0.1), "% 8"),   # 12 elements: mdm_dropout's multiple-of-8 rule
    (dict(x=0), "x && coef && y"),
    (dict(coef=0), "x && coef && y"),
    (dict(act=2), "act == 0"),
    (dict(dtype=2), "dtype =="),
    (dict(N=0), "N > 0"),
    (dict(N=70000), "N <= 65535"),
])
def test_invalid_arguments_are_rejected_with_a_message(kw, needle):
    rc, msg = _reapply(**kw)
    assert rc < 0, (kw, rc)
    assert needle in msg and "norm.hip" in msg, (kw, msg)


def test_case_table_names_the_kernel_family_the_dispatch_rule_gives():
    fams = set()
    for N, H, W, C, G, fam16, fam32 in RC.KERNEL_CASES:
        assert RC.family(H * W, C, G, torch.bfloat16) == fam16, (N, H, W, C, G)
        assert RC.family(H * W, C, G, torch.float32) == fam32, (N, H, W, C, G)
        fams |= {("bf16", fam16), ("fp32", fam32)}
    assert fams == {("bf16", "split"), ("bf16", "fused"), ("fp32", "split"), ("fp32", "fused")}
    assert all((N * H * W * C) % 8 == 0 for N, H, W, C, *_ in RC.DROPOUT_CASES) and len(RC.DROPOUT_CASES) >= 4
