"""CPU tests of tests/encoder_refs.py, the references of tests/test_gpu_encoder_parity.py: each float64 helper is pinned to the torch
library function it restates (rtol 1e-12); every input generator of the GPU module is held to a narrow bar (a condition on the
inputs, so that a pass on the device means something); and deliberately wrong models fail the GPU module's own assertions, run
here on host tensors with the right model standing in for the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_refs as er
import kernel_refs as kr

F64, F32 = torch.float64, torch.float32


def _close(a, b, rtol=1e-12):
    assert a.shape == b.shape and a.dtype == b.dtype == F64
    assert float((a - b).abs().max()) <= rtol * max(float(b.abs().max()), 1.0)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- float64 helpers against the torch library ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dense", [False, True], ids=["causal", "dense"])
def test_relbias_attn_ref_vs_torch_softmax(dense):
    H, hs, lens, half = 3, 16, [5, 70], 40                                            # a table shorter than the longer sequence: both clamps
    g = _g(1)
    K = [torch.randn(L, H, hs, generator=g, dtype=F64) for L in lens]
    V = [torch.randn(L, H, hs, generator=g, dtype=F64) for L in lens]
    own = np.concatenate([np.arange(L) for L in lens])
    seq = np.concatenate([np.full(L, b) for b, L in enumerate(lens)])
    pos = np.asarray(lens)[seq] - 1 if dense else own
    R = len(own)
    q, gate, tab = torch.randn(R, H * hs, generator=g, dtype=F64), 1 + torch.rand(R, H, generator=g, dtype=F64), torch.randn(H, 2 * half + 1, generator=g, dtype=F64)
    got = er.relbias_attn_ref(q, K, V, pos, seq, own, gate, tab, half, H)
    for r in range(R):
        n = pos[r] + 1
        k, v = K[seq[r]][:n].transpose(0, 1), V[seq[r]][:n].transpose(0, 1)           # [H, n, hs]
        idx = (torch.arange(n) - own[r] + half).clamp(0, 2 * half)
        s = torch.einsum("hd,hnd->hn", q[r].view(H, hs), k) + gate[r][:, None] * tab[:, idx]
        _close(got[r], torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v).reshape(-1))


@pytest.mark.parametrize("B,T,C,groups,K", [(2, 19, 32, 2, 5), (1, 7, 64, 4, 16), (1, 3, 16, 1, 1), (1, 5, 32, 1, 2)])
def test_grouped_conv_ref_vs_conv1d(B, T, C, groups, K):
    x, w, b, r = (t.double() for t in er.gconv_case(B, T, C, groups, K, True, True, 3))
    conv = F.conv1d(x.transpose(1, 2), w, b, padding=K // 2, groups=groups)[:, :, :T].transpose(1, 2)
    _close(er.grouped_conv_ref(x, w, b, groups, False, None), conv)
    _close(er.grouped_conv_ref(x, w, None, groups, True, r), F.gelu(conv - b) + r)
    _close(er.grouped_conv_replay(x, w, b, groups, True, r).double(), (F.gelu(conv) + r), rtol=1e-5)


@pytest.mark.parametrize("Cin,Fq,T,Cout,stride", [(1, 6, 9, 3, (2, 2)), (5, 5, 9, 16, (1, 1)), (17, 4, 10, 7, (2, 1)), (16, 1, 1, 4, (1, 2))])
def test_conv2d_ref_vs_conv2d(Cin, Fq, T, Cout, stride):
    x, w, b, r = (t.double() for t in er.conv2d_case(2, Cin, Fq, T, Cout, stride, True, True, 4))
    conv = F.conv2d(x, w, b, stride=stride, padding=1)
    _close(er.conv2d_ref(x, w, b, stride), conv)
    _close(er.conv2d_ref(x, w, None, stride, r, True), torch.relu(conv - b[None, :, None, None] + r))
    _close(er.conv2d_replay(x, w, b, stride, r, True).double(), torch.relu(conv + r), rtol=1e-5)


def test_layernorm_rope_ref_vs_layer_norm():
    R, C, hs, P = 6, 96, 32, 9
    g = _g(5)
    x, w, b = (torch.randn(s, generator=g, dtype=F64) for s in ((R, C), (C,), (C,)))
    cos, sin = torch.randn(P, hs, generator=g, dtype=F64), torch.randn(P, hs, generator=g, dtype=F64)
    pos = torch.tensor([0, 3, 8, -2, 11, 5])
    got = er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs)
    n = F.layer_norm(x, (C,), w, b, 1e-5)
    p = pos.clamp(0, P - 1)
    nh = n.view(R, C // hs, hs)
    rot = nh * cos[p][:, None] + torch.cat((-nh[..., hs // 2:], nh[..., :hs // 2]), -1) * sin[p][:, None]
    _close(got, torch.cat((rot.reshape(R, C), n), 1))
    _close(er.layernorm_rope_ref(x, None, None, 1e-5, cos, sin, pos, hs)[:, C:], F.layer_norm(x, (C,), None, None, 1e-5))


@pytest.mark.parametrize("B,N,C,K,stride", [(2, 400, 8, 10, 5), (1, 17, 4, 10, 5), (1, 70, 4, 1, 1), (1, 300, 8, 16, 32)])
def test_conv0_ref_vs_conv1d_group_norm_gelu(B, N, C, K, stride):
    x = er.conv0_clip(B, N, 6).double()
    w, gw, gb = (t.double() for t in er.conv0_weights(C, K, 7))
    lib = F.gelu(F.group_norm(F.conv1d(x[:, None], w[:, None], stride=stride), C, gw, gb, 1e-5)).transpose(1, 2)
    _close(er.conv0_ref(x, w, gw, gb, stride), lib)
    assert float((er.conv0_replay(x, w, gw, gb, stride).double() - lib).abs().max()) <= 1e-5
    # one frame (F.group_norm refuses it): the variance is exactly 0 and the output GELU(gn_b)
    _close(er.conv0_ref(x[:, :K], w, gw, gb, stride), F.gelu(gb)[None, None, :].expand(B, 1, C))


def test_melspec_db_ref_vs_matmul_and_the_floor():
    B, T, nb, nm, ld = 2, 3, 33, 7, 70
    g = _g(8)
    spec = torch.randn(B * T, ld, generator=g, dtype=F64)
    spec[1] = 0.0
    fb = torch.rand(nb, nm, generator=g, dtype=F64)
    fb[:, 2] = 0.0
    got = er.melspec_db_ref(spec, fb, B, T, nb, 6.5, 18.25)
    p = (spec[:, :nb] ** 2 + spec[:, nb:2 * nb] ** 2) @ fb
    want = ((10 * torch.log10(p.clamp(min=1e-10)) - 6.5) / 18.25).view(B, T, nm).transpose(1, 2)
    _close(got, want, rtol=1e-9)                       # the floor constant is the kernel's 1e-10f, 4e-8 dB from 1e-10
    floor = (-100.0 - 6.5) / 18.25
    assert bool((got[0, :, 1] == floor).all()) and bool((got[:, 2, :] == floor).all())
    assert not torch.equal(er.melspec_db_ref(spec, fb, B, T, nb, 6.5, 18.25, dt=F32), er.melspec_db_ref(spec, fb, B, T, nb, 6.5, 18.25, dt=F32, split=nb // 2 + 1))


# ---- the generators of the GPU module: conditions on the inputs ---------------------------------------------------------------------

def _relbias_batches():
    import test_gpu_encoder_parity as gp
    return gp


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
def test_plain_attention_inputs_keep_the_bars_narrow(hs, dense):
    gp = _relbias_batches()
    for dtype, cap in ((F32, 2e-5), (torch.bfloat16, 1e-4)):
        b = gp.batch(hs, dtype, dense)
        e = b.e_ref() if dtype == F32 else b.e_model()
        print(f"hs {hs} dense {dense} {dtype}: E {e:.3e} scale {b.scale():.3f}")
        assert 4.0 * e <= cap and b.scale() <= 8.0


@pytest.mark.parametrize("kind", er.HOSTILE_KINDS)
@pytest.mark.parametrize("hs", [64, 128])
def test_hostile_attention_inputs_are_finite_and_keep_the_bars_narrow(hs, kind):
    gp = _relbias_batches()
    for dtype in (F32, torch.bfloat16):
        b = gp.hostile(kind, hs, dtype)
        assert all(bool(torch.isfinite(t).all()) for t in b.K + b.V + [b.q, b.gate, b.tab, b.cache.k.float(), b.cache.v.float()])
        e = b.e_ref() if dtype == F32 else b.e_model()
        print(f"hostile {kind} hs {hs} {dtype}: E {e:.3e}")
        assert 4.0 * e <= 1e-3


def test_bias_dominant_kind_lets_the_bias_decide():
    b = _relbias_batches().hostile("bias_dominant", 64, F32)
    s = torch.einsum("rhd,lhd->rhl", b.q.view(-1, b.H, b.hs).double(), b.K[2])
    assert float(s.abs().max()) < 10.0 and float((b.gate[:, :, None] * b.tab[None]).abs().min()) == 75.0


def test_conv_inputs_keep_the_old_bar_as_a_cap():
    gp = _relbias_batches()
    for case in gp.GCONV_CASES:
        ref, replay = gp.gconv_host(case)[-2:]
        assert 4.0 * kr.abs_err(replay, ref) <= 2e-5 * float(ref.abs().max()), case
    for case in gp.CONV2D_CASES:
        ref, replay = gp.conv2d_host(case)[-2:]
        assert 4.0 * kr.abs_err(replay, ref) <= 2e-5 * float(ref.abs().max()), case


# ---- wrong models against the GPU module's assertions ---------------------------------------------------------------------------------

def test_wrong_attention_models_fail_the_assertions():
    gp = _relbias_batches()
    b32, b16 = gp.batch(64, F32, False), gp.batch(64, torch.bfloat16, False)
    # the right models stand in for the device and pass
    assert er.check_rows_fp32(er.relbias_attn_ref(*b32.args(), dt=F32), b32)[0]
    assert er.check_flash_bf16(er.relbias_flash_model(*b16.args(), score_dt=F64), b16)[0]
    assert er.check_flash_bf16(er.relbias_flash_model(*b16.args(), keys_per_step=128), b16)[0]
    flipped = lambda keys, qp, half: (torch.as_tensor(qp).long()[:, None] - keys[None, :].long() + half).clamp(0, 2 * half)
    off_by_one = lambda keys, qp, half: er.table_index(keys, qp, half + 1).clamp(0, 2 * half)
    wrong = {"q - key": dict(index=flipped), "head h + 1": dict(head_shift=1), "gate of the next row": dict(row_shift=1),
             "tab_half + 1": dict(index=off_by_one)}
    for name, kw in wrong.items():
        assert not er.check_rows_fp32(er.relbias_attn_ref(*b32.args(), dt=F32, **kw), b32)[0], name
        assert not er.check_flash_bf16(er.relbias_flash_model(*b16.args(), **kw), b16)[0], name
    for name, kw in {"gate without log2 e": dict(gate_log2e=False), "q as one bf16": dict(mode=("bf16", "split")),
                     "weights as one bf16": dict(mode=("split", "bf16"))}.items():
        assert not er.check_flash_bf16(er.relbias_flash_model(*b16.args(), **kw), b16)[0], name
    nan = b16.model().clone()
    nan[3, 5] = float("nan")                             # an unwritten element
    assert not er.check_flash_bf16(nan, b16)[0] and not er.check_rows_fp32(nan, b32)[0]
    # the hostile bars
    for kind in ("rising_max", "bias_dominant"):
        h32, h16 = gp.hostile(kind, 64, F32), gp.hostile(kind, 64, torch.bfloat16)
        assert er.check_rows_fp32(er.relbias_attn_ref(*h32.args(), dt=F32), h32)[0]
        assert er.check_flash_bf16(er.relbias_flash_model(*h16.args(), score_dt=F64), h16)[0]
        for name in ("q - key", "head h + 1"):
            assert not er.check_rows_fp32(er.relbias_attn_ref(*h32.args(), dt=F32, **wrong[name]), h32)[0], (kind, name)
            assert not er.check_flash_bf16(er.relbias_flash_model(*h16.args(), **wrong[name]), h16)[0], (kind, name)


def test_wrong_rotation_fails_the_rope_assertion():
    gp = _relbias_batches()
    x, w, b, cos, sin, pos, C, hs = gp.lnrope_host((256, 64))
    ref = er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs)
    replay = er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs, dt=F32)
    assert er.rows_check(replay, ref, replay)[0]
    assert not er.rows_check(er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs, dt=F32, rotate=er.rotate_half_wrong), ref, replay)[0]


def test_mel_chains_split_elsewhere_differ_in_bits():
    gp = _relbias_batches()
    spec, fb, B, T, nb, nm, ld = gp.mel_host((1025, 128, 2064))
    a = er.melspec_db_ref(spec, fb, B, T, nb, gp.MEL_MEAN, gp.MEL_STD, dt=F32)
    b = er.melspec_db_ref(spec, fb, B, T, nb, gp.MEL_MEAN, gp.MEL_STD, dt=F32, split=nb // 2 + 1)
    assert not torch.equal(a, b)
