"""fp8 weights in batched decode frames, the parts that need no GPU: the ABI addition, and the compiled gfx950 code of csrc/ua2_skinny.hip —
the fp8-weight instantiations of the weights-stationary kernel keep their working set in registers (no scratch), and the bf16
instantiations are what they were before the fp8 form was added."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# skinny2_kernel<EPI, CT, MT, CH, NWV, LA, SC, WD, RPW> of the bf16 form as the commit before the fp8 form compiled it (hipcc -O3,
# gfx950): (template arguments, .vgpr_count, .private_segment_fixed_size).  Recorded data: the fp8 form is a template flag of the same
# kernel text, and adding it must not move the bf16 kernels' registers or push them into scratch.
BF16_BEFORE = [
    ((0,1,2,4,16,2,0,0,1), 56, 0), ((0,1,2,4,16,2,1,0,1), 92, 0), ((0,1,2,8,8,2,0,0,1), 72, 0), ((0,1,2,8,8,2,1,0,1), 108, 0),
    ((0,1,2,8,12,2,0,0,1), 72, 0), ((0,1,2,8,12,2,1,0,1), 125, 0), ((0,1,2,12,8,2,0,0,1), 88, 0), ((0,1,2,12,8,2,1,0,1), 141, 0),
    ((0,1,4,4,16,1,0,0,1), 64, 0), ((0,1,4,4,16,1,1,0,1), 106, 0), ((0,1,4,4,16,2,0,0,1), 76, 0), ((0,1,4,8,8,1,0,0,1), 80, 0),
    ((0,1,4,8,8,1,1,0,1), 123, 0), ((0,1,4,8,8,2,0,0,1), 98, 0), ((0,1,4,8,8,2,1,0,1), 143, 0), ((0,1,4,8,12,1,0,0,1), 86, 0),
    ((0,1,4,8,12,1,1,0,1), 139, 0), ((0,1,4,8,12,2,0,0,1), 98, 0), ((0,1,4,8,12,2,1,0,1), 155, 0), ((0,1,4,12,8,1,0,0,1), 96, 0),
    ((0,1,4,12,8,1,1,0,1), 155, 0), ((0,1,4,12,8,2,0,0,1), 118, 0), ((0,1,4,12,8,2,1,0,1), 175, 0), ((0,2,2,4,16,2,0,0,1), 76, 0),
    ((0,2,2,8,8,2,0,0,1), 112, 0), ((0,2,2,8,8,2,1,0,1), 143, 0), ((0,2,2,8,12,2,0,0,1), 112, 0), ((0,2,2,8,12,2,1,0,1), 155, 0),
    ((0,2,2,12,8,2,0,0,1), 144, 0), ((0,2,2,12,8,2,1,0,1), 187, 0), ((0,2,4,4,16,1,0,0,1), 98, 0), ((0,2,4,4,16,2,0,0,1), 102, 0),
    ((0,2,4,8,8,1,0,0,1), 112, 0), ((0,2,4,8,8,1,1,0,1), 167, 0), ((0,2,4,8,8,2,0,0,1), 130, 0), ((0,2,4,8,8,2,1,0,1), 187, 0),
    ((0,2,4,8,12,1,0,0,1), 112, 0), ((0,2,4,8,12,2,0,0,1), 130, 0), ((0,2,4,12,8,1,0,0,1), 162, 0), ((0,2,4,12,8,1,1,0,1), 215, 0),
    ((0,2,4,12,8,2,0,0,1), 166, 0), ((0,2,4,12,8,2,1,0,1), 235, 0), ((1,1,2,4,16,2,0,0,1), 54, 0), ((1,1,2,8,12,2,0,0,1), 70, 0),
    ((1,1,2,16,16,2,0,0,1), 102, 0), ((1,1,2,16,16,4,0,0,2), 190, 0), ((1,1,4,4,16,1,0,0,1), 62, 0), ((1,1,4,4,16,2,0,0,1), 74, 0),
    ((1,1,4,8,12,1,0,0,1), 78, 0), ((1,1,4,8,12,2,0,0,1), 94, 0), ((1,1,4,16,16,1,0,0,1), 114, 0), ((1,1,4,16,16,1,0,0,2), 202, 0),
    ((1,1,4,16,16,4,0,0,2), 242, 0), ((1,2,2,4,16,2,0,0,1), 74, 0), ((1,2,2,8,12,2,0,0,1), 110, 0), ((1,2,4,4,16,1,0,0,1), 98, 0),
    ((1,2,4,4,16,2,0,0,1), 102, 0), ((1,2,4,8,12,1,0,0,1), 110, 0), ((1,2,4,8,12,2,0,0,1), 130, 0), ((2,1,2,8,8,2,0,0,1), 110, 0),
    ((2,1,2,8,8,2,1,0,1), 142, 0), ((2,1,2,12,8,2,0,0,1), 142, 0), ((2,1,2,12,8,2,1,0,1), 186, 0), ((2,1,4,8,8,1,0,0,1), 114, 0),
    ((2,1,4,8,8,1,1,0,1), 168, 0), ((2,1,4,8,8,2,0,0,1), 148, 0), ((2,1,4,8,8,2,1,0,1), 184, 0), ((2,1,4,12,8,1,0,0,1), 164, 0),
    ((2,1,4,12,8,1,1,0,1), 216, 0), ((2,1,4,12,8,2,0,0,1), 168, 0), ((2,1,4,12,8,2,1,0,1), 232, 0), ((2,2,2,8,8,2,0,0,1), 196, 0),
    ((2,2,2,8,8,2,1,0,1), 220, 0), ((2,2,4,8,8,1,0,0,1), 232, 0), ((2,2,4,8,8,1,0,4,1), 144, 0), ((2,2,4,8,8,1,1,4,1), 204, 0),
    ((2,2,4,8,8,2,0,0,1), 248, 0), ((2,2,4,12,8,1,0,3,1), 126, 0), ((2,2,4,12,8,1,0,4,1), 144, 0), ((2,2,4,12,8,1,0,6,1), 204, 0),
    ((2,2,4,12,8,1,1,3,1), 201, 0), ((2,2,4,12,8,1,1,4,1), 217, 0), ((2,2,4,12,8,1,1,6,1), 253, 0), ((2,2,4,12,8,2,0,6,1), 212, 0),
    ((2,2,4,12,8,2,1,6,1), 256, 0), ((3,1,2,4,16,2,0,0,1), 58, 0), ((3,1,2,4,16,2,1,0,1), 92, 0), ((3,1,2,8,12,2,0,0,1), 74, 0),
    ((3,1,2,8,12,2,1,0,1), 127, 0), ((3,1,2,12,8,2,0,0,1), 90, 0), ((3,1,2,12,8,2,1,0,1), 143, 0), ((3,1,4,4,16,1,0,0,1), 64, 0),
    ((3,1,4,4,16,1,1,0,1), 102, 0), ((3,1,4,4,16,2,0,0,1), 80, 0), ((3,1,4,8,12,1,0,0,1), 90, 0), ((3,1,4,8,12,1,1,0,1), 141, 0),
    ((3,1,4,8,12,2,0,0,1), 102, 0), ((3,1,4,8,12,2,1,0,1), 153, 0), ((3,1,4,12,8,1,0,0,1), 110, 0), ((3,1,4,12,8,1,1,0,1), 157, 0),
    ((3,1,4,12,8,2,0,0,1), 122, 0), ((3,1,4,12,8,2,1,0,1), 177, 0), ((3,2,2,4,16,2,0,0,1), 78, 0), ((3,2,2,8,12,2,0,0,1), 116, 0),
    ((3,2,2,8,12,2,1,0,1), 159, 0), ((3,2,2,12,8,2,0,0,1), 148, 0), ((3,2,2,12,8,2,1,0,1), 191, 0), ((3,2,4,4,16,1,0,0,1), 102, 0),
    ((3,2,4,4,16,2,0,0,1), 122, 0), ((3,2,4,8,12,1,0,0,1), 118, 0), ((3,2,4,8,12,2,0,0,1), 150, 0), ((3,2,4,12,8,1,0,0,1), 166, 0),
    ((3,2,4,12,8,1,1,0,1), 217, 0), ((3,2,4,12,8,2,0,0,1), 170, 0), ((3,2,4,12,8,2,1,0,1), 237, 0),
]


def test_abi_addition_is_declared_and_exported_and_the_version_stays():
    from uniaudio2_amd import _lib
    header = open(os.path.join(ROOT, "include", "ua2hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bua2_linear_w8_many\s*\(", header)
    assert hasattr(raw, "ua2_linear_w8_many") and "ua2_linear_w8_many" in _lib.exported_symbols()
    assert hasattr(raw, "ua2_linear_w8_many_chain_timed") and re.search(r"\bua2_linear_w8_many_chain_timed\s*\(", header)
    assert _lib.lib.ua2_version() == 10
    assert _lib.lib.ua2_debug_kernel_launches(b"skinny2_w8") >= 0        # a known family (GPU tests of the same process may have launched it)
    assert _lib.lib.ua2_debug_kernel_launches(b"skinny2_w9") == -1


def test_null_arguments_return_an_error_without_a_device():
    from uniaudio2_amd import _lib
    assert _lib.lib.ua2_linear_w8_many(None, None, None, None) != 0
    assert b"ua2_linear_w8_many" in _lib.lib.ua2_last_error()
    a = _lib.LinearArgs()
    assert _lib.lib.ua2_linear_w8_many(ctypes.byref(a), None, None, None) != 0
    assert b"ua2_linear_w8_many" in _lib.lib.ua2_last_error()


@pytest.fixture(scope="module")
def skinny_meta(tmp_path_factory):
    """{(W8, EPI, CT, MT, CH, NWV, LA, SC, WD, RPW) of skinny2_kernel: (vgpr_count, private_segment_fixed_size)} from the assembly metadata"""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "skinny.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "uniaudio2_amd", "csrc", "ua2_skinny.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", out.read_text())[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"skinny2_kernelI((?:L[ib]\d+E)+)E", name)
        if not m:
            continue
        args = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1)))
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[args] = (field("vgpr_count"), field("private_segment_fixed_size"))
    return meta


def test_fp8_instantiations_have_no_scratch(skinny_meta):
    w8 = {k: v for k, v in skinny_meta.items() if k[0] == 1}
    # the variants pick_variant can return (4 resident forms x the 12 geometries, scaled consumers where the epilogue has one, + the SwiGLU rings)
    assert len(w8) >= 60, sorted(w8)
    for k, (vgpr, scratch) in w8.items():
        assert scratch == 0, f"skinny2_kernel<{k}> (fp8) spills {scratch} B of scratch per lane"
        assert k[9] == 1 and k[8] % 2 == 0, f"{k}: the fp8 form has one range per wave and even rings"
        bf16 = skinny_meta.get((0,) + k[1:])
        # the held weights are fp8: never more registers than the bf16 form of the same variant plus the expanded fragments of one chunk
        if bf16 is not None:
            assert vgpr <= bf16[0] + 16, (k, vgpr, bf16)


def test_bf16_instantiations_are_what_they_were(skinny_meta):
    bf16 = {k[1:]: v for k, v in skinny_meta.items() if k[0] == 0}
    assert len(BF16_BEFORE) == 115
    for args, vgpr, scratch in BF16_BEFORE:
        assert args in bf16, f"skinny2_kernel<{args}> is no longer built"
        assert bf16[args] == (vgpr, scratch), f"skinny2_kernel<{args}>: (vgprs, scratch) {bf16[args]} was {(vgpr, scratch)}"
    assert set(bf16) == {a for a, _, _ in BF16_BEFORE}, "a bf16 instantiation was added"
