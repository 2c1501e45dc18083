"""fp8 (OCP e4m3fn) weight-only option, the parts that need no GPU: ABI additions, the CLI flag, the torch restatement of the quantiser
(ops.w8_exponents / quant_w8 / dequant_w8) that the GPU tests compare the HIP pack kernel against, and the compiled code of the
fp8-weight instantiations of the decode kernel."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ["ua2_pack_linear_w8", "ua2_packed_bytes_w8", "ua2_linear_w8", "ua2_stage3_set_w8"]


def test_abi_additions_are_declared_and_exported_and_the_version_stays():
    from uniaudio2_amd import _lib
    header = open(os.path.join(ROOT, "include", "ua2hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name) and name in _lib.exported_symbols(), name
    assert _lib.lib.ua2_version() == 10
    assert _lib.lib.ua2_debug_kernel_launches(b"gemv_w8") == 0          # nothing in this process has asked for fp8 weights
    assert _lib.lib.ua2_debug_kernel_launches(b"gemv_w9") == -1
    assert _lib.lib.ua2_packed_bytes_w8(5120, 3072) == 5120 * 3072        # half of the bf16 form
    assert _lib.lib.ua2_packed_bytes_w8(110, 128) == 112 * 128            # N padded to 16
    assert _lib.lib.ua2_packed_bytes_w8(16, 96) == 0                      # K % 64 != 0: no fp8 form


def test_bad_arguments_return_codes_without_a_device():
    from uniaudio2_amd import _lib
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert _lib.lib.ua2_pack_linear_w8(p, _lib.UA2_F32, 0, 16, 96, p, p, None, 0, None) != 0
    assert b"multiple of 64" in _lib.lib.ua2_last_error()
    assert _lib.lib.ua2_pack_linear_w8(p, 7, 0, 16, 64, p, p, None, 0, None) != 0
    assert _lib.lib.ua2_linear_w8(None, None, None, None) != 0
    assert _lib.lib.ua2_stage3_set_w8(None, None, 0) != 0


def test_cli_flag():
    from uniaudio2_amd import multi_task_inference as cli
    a = cli.get_parser().parse_args(["--task", "TTS"])
    assert a.weight_dtype == "none"
    a = cli.get_parser().parse_args(["--task", "TTS", "--weight_dtype", "fp8_e4m3"])
    assert a.weight_dtype == "fp8_e4m3" and a.dtype == "bf16"
    with pytest.raises(SystemExit):
        cli.get_parser().parse_args(["--task", "TTS", "--weight_dtype", "fp8_e4m3", "--dtype", "fp32"])
    with pytest.raises(SystemExit):
        cli.get_parser().parse_args(["--task", "TTS", "--weight_dtype", "int8"])


def test_model_refuses_fp8_weights_outside_bf16_before_touching_a_device():
    from helpers import build_toy_module
    m = build_toy_module()
    assert m.weight_dtype is None
    with pytest.raises(ValueError, match="bf16 plan"):                    # an fp32 plan: refused before anything looks at the device
        m.setup_caches(1, dtype=torch.float32, weight_dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="bf16 plan"):                    # the module's own dtype (fp32 parameters) counts the same way
        m.setup_caches(1, weight_dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="weight_dtype must be"):
        m.setup_caches(1, dtype=torch.bfloat16, weight_dtype=torch.int8)
    m.weight_dtype = torch.float8_e4m3fn                                  # the attribute is what setup_caches takes when the argument is left out
    with pytest.raises(ValueError, match="bf16 plan"):
        m.setup_caches(1, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="ROCm device"):                # a valid request on a CPU module: the device check, as before
        m.setup_caches(1, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):                # an explicit None overrides the attribute
        m.setup_caches(1, dtype=torch.float32, weight_dtype=None)


def test_quantiser_restatement():
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(5)
    W = torch.randn(64, 256, generator=g) * 0.02
    W[1] = 0.0                                   # zero row
    W[2] = 0.0
    W[2, 3] = -448.0 * 2.0 ** -7                 # amax exactly 448 x a power of two: the largest code, not the next exponent
    W[3] = torch.randn(256, generator=g) * 1e-30   # tiny but normal
    W[4] = torch.randn(256, generator=g) * 1e-41   # fp32 denormals: e clamps at -117, everything rounds to (signed) zero
    W[5] *= 1e30
    q, e = ops.quant_w8(W)
    Wp = ops.dequant_w8(W)
    assert q.dtype == torch.float8_e4m3fn and e.dtype == torch.int32
    qf = q.float()
    assert torch.isfinite(qf).all() and float(qf.abs().max()) == 448.0
    assert torch.equal(Wp.bfloat16().float(), Wp), "W' survives a bf16 round trip"
    assert torch.equal(Wp, ops.dequant_w8(Wp)), "quantising W' again changes nothing (same e, same q)"
    # e = ceil(log2(amax / 448)), restated in double precision
    for n in range(W.shape[0]):
        amax = float(W[n].abs().max())
        want = 0 if amax == 0.0 else min(max(math.ceil(math.log2(amax / 448.0) - 1e-12), -117), 120)
        assert int(e[n]) == want, (n, amax, int(e[n]), want)
        if want > -117 and amax > 0:
            assert float(qf[n].abs().max()) >= 224.0, "the scale is the smallest power of two that fits (amax 2^-e in (224, 448]; RNE may land on 224)"
    assert int(e[1]) == 0 and float(Wp[1].abs().max()) == 0.0
    assert int(e[2]) == -7 and float(Wp[2, 3]) == float(W[2, 3])
    assert int(e[4]) == -117 and float(Wp[4].abs().max()) == 0.0
    # the loss the documentation quotes: relative rms error of W' on N(0, 0.02) weights
    big = torch.randn(512, 1024, generator=g) * 0.02
    rel = float((ops.dequant_w8(big) - big).pow(2).mean().sqrt() / big.pow(2).mean().sqrt())
    assert 2.0e-2 < rel < 3.2e-2, rel
    # a power-of-two scale commutes with an fp32 sum: scaling after the sum == summing the scaled weights
    x = torch.randn(1024, generator=g)
    qb, eb = ops.quant_w8(big)
    assert torch.equal(torch.ldexp(qb.float() @ x, eb), torch.ldexp(qb.float(), eb.unsqueeze(1)) @ x)


def test_w8_state_dict_touches_the_linears_only():
    from helpers import load_golden_lm, toy_state_dict
    from w8_ref import is_quantised, w8_state_dict
    sd = toy_state_dict(load_golden_lm()[1])
    out = w8_state_dict(sd)
    changed = {k for k in sd if not torch.equal(sd[k], out[k])}
    assert changed == {k for k, v in sd.items() if is_quantised(k, v)}
    assert not any("wte" in k or "audio_embeddings" in k or "norm" in k or "ln_f" in k for k in changed)
    assert "audio_head" in changed and "projection.weight" in changed and "backbone.lm_head.weight" in changed


# ---- compiled code of the fp8-weight instantiations (csrc/ua2_gemv.hip gemv_w8_kernel) ---------------------------------------
@pytest.fixture(scope="module")
def gemv_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "gemv.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "uniaudio2_amd", "csrc", "ua2_gemv.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernels(asm_text):
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)s_endpgm", asm_text, re.S | re.M):
        ins = [line.split(";")[0].strip() for line in m.group(2).splitlines()]
        out[m.group(1)] = [t for t in ins if t and not t.startswith(".")]
    return out


def test_fp8_kernels_have_no_scratch_and_issue_the_burst_without_waiting(gemv_asm):
    scratch = dict(re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", gemv_asm))
    ks = {k: v for k, v in _kernels(gemv_asm).items() if "gemv_w8_kernel" in k}
    assert len(ks) >= 9 * 5, sorted(ks)          # 9 (prologue, epilogue) pairs x the geometries
    for name, ins in ks.items():
        assert int(scratch[name]) == 0, f"{name} spills {scratch[name]} B of scratch per lane"
        assert any(t.startswith("v_cvt_pk_f32_fp8") for t in ins) and any(t.startswith("v_mfma_f32_16x16x32_bf16") for t in ins), name
        assert not any("f8f6f4" in t or "fp8_fp8" in t or "bf8" in t for t in ins), f"{name}: activations are bf16, the MFMA is the bf16 one"
        nts = [i for i, t in enumerate(ins) if t.startswith("global_load_dwordx4") and t.endswith(" nt")]
        assert nts, name
        end = 0
        while end + 1 < len(nts) and nts[end + 1] - nts[end] < 16:
            end += 1
        exps = [i for i, t in enumerate(ins[:nts[0]]) if re.match(r"global_load_[su]byte", t)]
        assert exps, f"{name}: the exponent vector must be requested BEFORE the weight burst"
        if "gemv_w8_kernelILi3E" in name:
            continue                             # LOCAL_ATTN: the attention's own dependent loads (page id -> K / V) sit in front of the burst, as in the bf16 kernel
        waits = [t for t in ins[exps[0]:nts[end] + 1] if t.startswith("s_waitcnt vmcnt")]
        assert not waits, f"{name}: {waits} between the exponent load and the end of the first weight burst"
        inner = [t for t in ins[nts[0]:nts[end] + 1] if t.startswith("s_waitcnt vmcnt(0)")]
        assert not inner, name
