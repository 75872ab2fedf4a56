"""The test hook of the Winograd convolution's persistent grid, without a GPU: declared, bound and exported; the ABI stays."""
import os
import re

from mvdetr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvdetr_winograd_set_max_workgroups"


def test_the_hook_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    assert re.search(r"#define\s+MVDETR_OPS_ABI_VERSION\s+18\b", header) and _lib.ABI_VERSION == 18
    assert re.search(r"\bint\s+%s\s*\(\s*int\s+n\s*\)\s*;" % NAME, header)
    assert _lib.SIGNATURES[NAME] == ([_lib._i], _lib._i)
    lib = _lib.lib()                                                           # loads the library and checks every symbol
    assert lib.mvdetr_ops_abi_version() == 18
    from mvdetr_amd.ops import conv_winograd as cw
    # process-wide, 0 is the default, the previous value comes back; no launch is needed for any of it
    try:
        assert cw.set_winograd_max_workgroups(7) == 0
        assert getattr(lib, NAME)(3) == 7
        assert cw.set_winograd_max_workgroups(0) == 3
    finally:
        cw.set_winograd_max_workgroups(0)
    assert cw.set_winograd_max_workgroups(0) == 0


def test_one_kernel_and_no_work_counter():
    """The persistent kernel replaced the one-unit kernel (no second copy), and hands out units statically."""
    src = "".join(open(os.path.join(ROOT, "mvdetr_amd", "csrc", f)).read()    # the kernels and the device text they share
                  for f in ("conv_winograd.hip", "conv_winograd_device.h"))
    assert len(re.findall(r"__global__[^;{]*\bconv3x3_winograd_f32\s*\(", src)) == 1
    assert "gridDim.x" in src and not re.search(r"\batomic(Add|Inc|CAS)\b", src)
