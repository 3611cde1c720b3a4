"""Host-side checks of the wide compatibility kernel (256 < L <= 512, phl_compat_wide.hip): the C ABI's planes size
and the kernel's machine code.  No GPU needed."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planes_bytes_cover_the_wide_label_range():
    """phl_compat_planes_bytes(L) > 0 exactly for L % 4 == 0 in (128, 512]: the split entry points take up to 512 labels.
    Above 256 the planes hold (L rounded up to 32) / 32 K chunks x ceil(Lp / 128) label quarters of 24 KiB."""
    import phl

    lib = phl.load_library()
    for L in range(0, 600):
        got = lib.phl_compat_planes_bytes(L)
        want = L % 4 == 0 and 128 < L <= 512
        assert (got > 0) == want, (L, got)
    for L in (516, 342, 0, 128, 1024):
        assert lib.phl_compat_planes_bytes(L) == 0, L
    for L, Lp in ((260, 288), (344, 352), (384, 384), (512, 512)):
        assert lib.phl_compat_planes_bytes(L) == (Lp // 32) * ((Lp + 127) // 128) * 24576, L
    assert lib.phl_compat_planes_bytes(256) == 16 * 24576          # the 256-label layout is unchanged


def test_wide_compat_kernel_machine_code():
    """tools/check_wide_isa.py: every instance of k_compat_wide compiles without scratch or AGPRs, within 256 VGPRs, with
    six DMA units and a counted wait in front of the barrier of every slot."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("check_wide_isa", os.path.join(ROOT, "tools", "check_wide_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main() == 0
