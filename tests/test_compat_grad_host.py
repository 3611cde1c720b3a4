"""Host-side checks of the backward of the compatibility + softmax step (phl_compat_grad.hip): the workspace size of
phl_compat_mu_grad and the kernels' machine code.  No GPU needed."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ranges(n, L):
    """The documented formula (include/phl.h): pixel ranges of phl_compat_mu_grad."""
    c = -(-L // 64)
    r = min(c, 16 // c)
    slabs = -(-L // (64 * r))
    occ = 256 * max(1, 16 // (c * r)) // slabs
    R = min(-(-n // 64), occ, (1 << 24) // (L * L))
    if slabs > 1 and R >= 8:
        R = R // 8 * 8
    return max(1, R)


def test_mu_grad_workspace_follows_its_formula():
    import phl

    lib = phl.load_library()
    for L in range(0, 530):
        for n in (0, 1, 63, 65, 511, 513, 140_003, 3_145_728):
            got = lib.phl_compat_mu_grad_workspace_bytes(n, L)
            if L % 4 or L < 4 or L > 512:
                assert got == 0, (n, L, got)
            else:
                assert got == _ranges(n, L) * L * L * 4, (n, L, got)
                assert got <= 64 << 20, (n, L, got)
    assert lib.phl_compat_mu_grad_workspace_bytes(3_145_728, 512) == 64 << 20
    assert lib.phl_compat_mu_grad_workspace_bytes(3_145_728, 256) == 64 << 20     # one slab, 256 ranges


def test_grad_kernels_machine_code():
    """tools/check_grad_isa.py: no scratch, the register budget of each launch, no float atomics, the products on the
    f32 matrix cores."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("check_grad_isa", os.path.join(ROOT, "tools", "check_grad_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main() == 0
