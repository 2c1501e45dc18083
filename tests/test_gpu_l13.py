"""Lossless 13-bit weight images on the device (include/ua2hip.h ua2_pack_linear_l13, ua2_linear_l13, ua2_stage3_set_lossless): the
device packer against the numpy encoder byte for byte, the decode kernel on the image against the same launch on the bf16 weights bit
for bit in every form its launcher picks, escapes, and a toy plan with the images on and off."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import build_product_model, load_golden_lm, product_decode_loop, toy_state_dict
from l13_ref import encode

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRO_SCALED = 4

# (K, N, (waves, chunks per wave, multi-round) the launcher must pick for one matrix, what the shape is here for)
SHAPES = [(128, 32, (4, 4, 0), "fall-back geometry: one chunk per wave"),
          (512, 48, (4, 4, 0), "single burst of 4 chunks"),
          (3072, 48, (12, 8, 0), "single burst of 8 chunks"),
          (8192, 32, (16, 16, 0), "single burst of 16 chunks"),
          (2048, 4112, (8, 4, 1), "more than 256 tiles: two rounds of 4"),
          (3072, 4112, (8, 4, 1), "three rounds of 4")]
ROWS = [1, 2, 5]


def _launches(name):
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(name.encode())


def _geometry(N, K, nt):
    from uniaudio2_amd._lib import UA2_BF16, lib
    w, c, mr = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.ua2_debug_gemv_geometry(UA2_BF16, N, K, nt, C.byref(w), C.byref(c), C.byref(mr)) == 0
    return w.value, c.value, mr.value


def _weight(N, K, seed, block=16):
    """N(0, 0.02) in bf16 with, in every run of 8 consecutive k (a lane's share of a chunk): +0 or -0, the top pair of the tile's window,
    a negative value of its bottom pair (q = 1) and one of that pair's upper binade.  The window alternates from one block of `block`
    rows to the next — top +-0.125 (E[7:1] = 62, base 47, bottom -2^-31) and top +-0.5 (base 48, bottom -2^-29) — so that neighbouring
    tiles have different base bytes (block = 16: a tile; a rotated q|k|v weight passes its head size, since packing permutes rows inside
    a head).  Random values below 2^-20 are lifted to it, so that the window holds every weight by construction: no escapes."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.02
    W = torch.where(W.abs() < 2.0 ** -20, torch.copysign(torch.full_like(W, 2.0 ** -20), W), W)
    top = torch.where((torch.arange(N) // block) % 2 == 0, 0.125, 0.5).unsqueeze(1)
    sgn = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0).unsqueeze(1)
    n8 = K // 8
    W[:, 0::8] = (0.0 * sgn).expand(N, n8)
    W[:, 1::8] = (top * sgn).expand(N, n8)
    W[:, 2::8] = (-top * 2.0 ** -28).expand(N, n8)
    W[:, 3::8] = (1.5 * top * 2.0 ** -27).expand(N, n8)
    return W.bfloat16()


def _bases(N, block=16):
    """base byte of every tile of a _weight(N, K, ...) matrix packed without a row permutation"""
    return [47 + (t * 16 // block) % 2 for t in range((N + 15) // 16)]


_PACKS = {}


def _pack(N, K, seed, rope_hs=0):
    """(packed bf16, image, base) of a planted weight, packed once per process."""
    from uniaudio2_amd import ops
    key = (N, K, seed, rope_hs)
    if key not in _PACKS:
        packed = ops.pack_linear(_weight(N, K, seed, rope_hs or 16).to(DEV), torch.bfloat16, rope_head_size=rope_hs)
        image, base, esc = ops.pack_linear_l13(packed, N, K)
        assert int(esc.item()) == 0 and base.cpu().tolist() == _bases(N, rope_hs or 16)
        _PACKS[key] = (packed, image, base)
    return _PACKS[key]


# ---- (a) the packer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(128, 32), (512, 48), (2048, 4112), (256, 110)])
def test_device_packer_equals_the_numpy_encoder(K, N):
    from uniaudio2_amd._lib import lib
    packed, image, base = _pack(N, K, 3)
    T = (N + 15) // 16
    assert image.numel() == lib.ua2_packed_bytes_l13(N, K) == T * (K // 128) * 3328
    ref_image, ref_base, ref_esc = encode(packed.view(torch.int16).cpu().numpy().view(np.uint16).reshape(T, K // 32, 64, 8))
    assert ref_esc == 0
    assert np.array_equal(base.cpu().numpy(), ref_base), "base bytes"
    assert ref_base.tolist() == _bases(N) and (T == 1 or len(set(ref_base.tolist())) == 2)      # neighbouring tiles differ
    assert np.array_equal(image.cpu().numpy(), ref_image), "image bytes"


def test_no_image_for_k_not_a_multiple_of_128():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    assert lib.ua2_packed_bytes_l13(64, 192) == 0 and lib.ua2_packed_bytes_l13(64, 96) == 0
    with pytest.raises(ValueError):
        ops.pack_linear_l13(ops.pack_linear(torch.zeros(64, 192, device=DEV), torch.bfloat16), 64, 192)


# ---- (c) escapes ----------------------------------------------------------------------------------------------------------------
def test_one_planted_escape_is_counted():
    from uniaudio2_amd import ops
    N, K = 48, 512
    W = _weight(N, K, 5)
    W[17, 133] = 2.0 ** -31                                        # E[7:1] = 48 = base of tile 1 (top 0.5): one pair below its window
    packed = ops.pack_linear(W.to(DEV), torch.bfloat16)
    image, base, esc = ops.pack_linear_l13(packed, N, K)
    assert int(esc.item()) == 1 and base.cpu().tolist() == [47, 48, 47]
    ref = encode(packed.view(torch.int16).cpu().numpy().view(np.uint16).reshape(3, K // 32, 64, 8))
    assert ref[2] == 1 and np.array_equal(image.cpu().numpy(), ref[0])


# ---- (b) kernel identity: ua2_linear_l13 against ua2_linear on the bf16 weights ------------------------------------------------------
def _kv(M, n_head, n_kv, hs, seed):
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(M, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV)
    v = (torch.randn(M, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV)
    pt = torch.arange(M, dtype=torch.int32, device=DEV).view(M, 1)
    return k, v, ops.kv_geom(k, v, pt, n_head, n_kv, hs), pt


def _identity(pro, epi, M, N, K, heads=None, rope_mode=0, handover=False, partmax=False):
    """The launch on the bf16 weights (ua2_linear) and on their images (ua2_linear_l13): asserts every output equal bit for bit."""
    from uniaudio2_amd import _lib, ops
    nt = 2 if epi == _lib.EPI_SWIGLU else 1
    rope_hs = heads[2] if (epi == _lib.EPI_QKV_ROPE and rope_mode == _lib.ROPE_HALF_SPLIT) else 0
    packs = [_pack(N, K, 11 + t, rope_hs) for t in range(nt)]
    outs = []
    for use_image in (False, True):
        gg = torch.Generator().manual_seed(K + N + M)
        kw = dict(dtype=torch.bfloat16, M=M, N=N, K=K, w0=packs[0][0], prologue=pro, epilogue=epi, launch=False, rope_mode=rope_mode)
        keep, hold = {}, []
        if nt == 2:
            kw["w1"] = packs[1][0]
        x = torch.randn(M, K, generator=gg)
        if pro == _lib.PRO_NORM:
            kw.update(x=x.to(DEV), norm_w=(1 + 0.1 * torch.randn(K, generator=gg)).to(DEV))
        elif pro == _lib.PRO_CAST:
            kw.update(x=x.to(DEV))
        elif pro == PRO_SCALED:
            kw.update(x_h=x.bfloat16().to(DEV), x_ssq=(x * x).view(M, K // 16, 16).sum(-1).to(DEV).contiguous(), ldh=K)
        if pro == _lib.PRO_LOCAL_ATTN or epi == _lib.EPI_QKV_ROPE:
            n_head, n_kv, hs = heads
            k, v, geom, pt = _kv(M, n_head, n_kv, hs, 7)
            hold.append(pt)
            keep["k_pool"], keep["v_pool"] = k, v
            kw.update(row_pos=torch.full((M,), 5, dtype=torch.int32, device=DEV), kv=geom)
            if pro == _lib.PRO_LOCAL_ATTN:
                kw.update(x=(torch.randn(M, K, generator=gg) * 0.5).to(DEV))
            else:
                ang = torch.rand(8, hs // 2, generator=gg)
                keep["q_out"] = torch.zeros(M, n_head * hs, device=DEV)
                kw.update(rope_cos=torch.cos(ang).to(DEV), rope_sin=torch.sin(ang).to(DEV), q_out=keep["q_out"])
        if epi == _lib.EPI_RESIDUAL:
            keep["y"] = torch.zeros(M, N, device=DEV)
            kw.update(resid=torch.randn(M, N, generator=gg).to(DEV), y=keep["y"])
        elif epi in (_lib.EPI_STORE, _lib.EPI_SWIGLU):
            keep["y"] = torch.zeros(M, N, device=DEV)
            kw.update(y=keep["y"])
        if handover:
            keep["y_h"] = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            keep["y_ssq"] = torch.zeros(M, N // 16, device=DEV)
            kw.update(y_norm_w=(1 + 0.1 * torch.randn(N, generator=gg)).to(DEV), y_h=keep["y_h"], y_ssq=keep["y_ssq"], ldh=N)
        if partmax:
            nb = (N + 15) // 16
            keep["part_max"] = torch.zeros(M, nb, device=DEV)
            keep["part_idx"] = torch.zeros(M, nb, dtype=torch.int32, device=DEV)
            kw.update(part_max=keep["part_max"], part_idx=keep["part_idx"], forbid=torch.full((M,), 24, dtype=torch.int32, device=DEV))
        hold.append(kw)
        a = ops.linear(**kw)
        n_g, n_l = _launches("gemv"), _launches("gemv_l13")
        if use_image:
            ops.linear_l13(a, packs[0][1:], packs[1][1:] if nt == 2 else None)
        else:
            _lib.check(_lib.lib.ua2_linear(C.byref(a), ops.stream()), "ua2_linear")
        torch.cuda.synchronize()
        assert (_launches("gemv") - n_g, _launches("gemv_l13") - n_l) == ((1, 1) if use_image else (1, 0)), use_image
        outs.append({k: v.cpu().clone() for k, v in keep.items()})
    ref, got = outs
    assert ref.keys() == got.keys() and ref
    for k in ref:
        p, q = ref[k], got[k]
        if p.dtype == torch.bfloat16:
            p, q = p.view(torch.int16), q.view(torch.int16)
        assert torch.equal(p, q), (pro, epi, M, N, K, k)
        assert k not in ("y", "q_out", "y_h") or float(ref[k].float().abs().max()) > 0, (k, "output never written")


def test_the_shapes_reach_the_forms_they_are_here_for():
    for K, N, geo, what in SHAPES:
        assert _geometry(N, K, 1) == geo, (K, N, what)
    assert _geometry(48, 3072, 2) == (12, 8, 0) and _geometry(48, 512, 2) == (4, 4, 0) and _geometry(4112, 2048, 2) == (8, 4, 1) and _geometry(4112, 3072, 2) == (8, 4, 1)
    assert _geometry(32, 8192, 2) == (16, 8, 0)                    # two matrices: rounds of 8 at most, two per wave, reloaded in place
    assert _geometry(96, 128, 1) == (4, 4, 0) and _geometry(96, 8192, 1) == (16, 16, 0)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", [(k, n) for k, n, _, _ in SHAPES])
def test_store_with_argmax_partials_and_forbid(K, N, M):
    from uniaudio2_amd import _lib
    _identity(_lib.PRO_CAST, _lib.EPI_STORE, M, N, K, partmax=True)
    if K <= 4096:
        _identity(PRO_SCALED, _lib.EPI_STORE, M, N, K, partmax=True)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", [(k, n) for k, n, _, _ in SHAPES])
def test_residual_with_the_scaled_handover(K, N, M):
    from uniaudio2_amd import _lib
    _identity(_lib.PRO_CAST, _lib.EPI_RESIDUAL, M, N, K, handover=(N % 32 == 0))     # the hand-over needs whole 32-column pairs of tiles


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N", [(k, n) for k, n, _, _ in SHAPES])
def test_swiglu_two_matrices(K, N, M):
    from uniaudio2_amd import _lib
    _identity(PRO_SCALED if K <= 4096 else _lib.PRO_NORM, _lib.EPI_SWIGLU, M, N, K)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K,N,heads,mode", [(128, 96, (1, 1, 32), 0), (512, 48, (1, 1, 16), 1), (3072, 48, (1, 1, 16), 1), (3072, 96, (1, 1, 32), 0),
                                            (8192, 96, (1, 1, 32), 0),
                                            (2048, 4112, (255, 1, 16), 1), (3072, 4112, (255, 1, 16), 1)])
def test_qkv_rope_q_and_cache_page(K, N, heads, mode, M):
    """N = (n_head + 2 n_kv) head_size: 16-wide heads under the interleaved rotation at the table's N, 32-wide half-split heads (the
    packer's row permutation) at N = 96 where the table's N = 32 holds no q | k | v."""
    from uniaudio2_amd import _lib
    _identity(PRO_SCALED if K <= 4096 else _lib.PRO_NORM, _lib.EPI_QKV_ROPE, M, N, K, heads=heads, rope_mode=mode)


@pytest.mark.parametrize("K,N,heads", [(128, 32, (4, 2, 32)), (512, 48, (8, 2, 64)), (3072, 48, (24, 8, 128)), (8192, 32, (64, 8, 128)),
                                       (2048, 4112, (32, 8, 64)), (3072, 4112, (24, 8, 128))])
def test_local_attention_prologue(K, N, heads):
    from uniaudio2_amd import _lib
    _identity(_lib.PRO_LOCAL_ATTN, _lib.EPI_RESIDUAL, 1, N, K, heads=heads, handover=(N % 32 == 0))


def test_refusals_name_the_entry_point_and_launch_nothing():
    from uniaudio2_amd import _lib, ops
    packed, image, base = _pack(32, 128, 3)
    n0 = _launches("gemv")
    for M, dtype, epi in [(6, torch.bfloat16, _lib.EPI_STORE), (1, torch.float32, _lib.EPI_STORE), (1, torch.bfloat16, _lib.EPI_GELU)]:
        x, y = torch.zeros(M, 128, device=DEV), torch.zeros(M, 32, device=DEV)
        a = ops.linear(dtype=dtype, M=M, N=32, K=128, w0=packed, x=x, y=y, epilogue=epi, launch=False)
        with pytest.raises(_lib.Ua2Error, match="ua2_linear_l13"):
            ops.linear_l13(a, (image, base))
    assert _launches("gemv") == n0


# ---- (d) a toy plan with the images on and off ---------------------------------------------------------------------------------------
def test_toy_plan_is_identical_with_images_on_and_off():
    d, meta = load_golden_lm()
    sd = {k: v.clone() for k, v in toy_state_dict(meta).items()}
    w = sd["decoder.transformer.h.1.mlp.proj.weight"]
    w[0, 0], w[0, 1] = 1.0, 2.0 ** -40                             # tile 0: window below 1.0 ends 30 binades down: an escape
    tokens = torch.from_numpy(d["tts1_tokens"]).long()[None]
    mask = torch.from_numpy(d["tts1_mask"]).bool()[None]
    m = build_product_model(sd, torch.bfloat16, batch=1)
    st = m.lossless_stats()
    n_mats = (3 + 2 + 2 + 2) * 5 + 1 + 8                            # five Linears per layer, projection, the audio heads
    assert st["on"] == 1 and st["with_escapes"] == 1 and st["without_image"] == 1 and st["with_image"] == n_mats - 1, st
    assert 13 / 16 < st["image_bytes_per_frame"] / st["bf16_bytes_per_frame"] < 0.84 and st["extra_device_bytes"] > 0, st

    def run(on):
        m.set_lossless(on)
        assert m.lossless_stats()["on"] == int(on)
        n0 = _launches("gemv_l13")
        out = product_decode_loop(m, tokens, mask, 6, "audio", collect_logits=True)
        torch.cuda.synchronize()
        pools = [t.cpu().clone() for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert, m.decoder)
                 for t in g.kv_cache.k + g.kv_cache.v]
        fast = product_decode_loop(m, tokens, mask, 6, "audio", fast=True)["samples"]       # the on-device loop: the frame log
        torch.cuda.synchronize()
        return out, pools, fast, _launches("gemv_l13") - n0

    off, pools_off, log_off, n_off = run(False)
    on, pools_on, log_on, n_on = run(True)
    assert n_off == 0 and n_on > 0, (n_off, n_on)
    for k in ("samples", "text_logits", "audio_logits"):
        assert torch.equal(on[k], off[k]), k
    assert torch.equal(log_on, log_off), "frame log"
    for p, q in zip(pools_on, pools_off):
        assert torch.equal(p.view(torch.int16), q.view(torch.int16)), "K / V pages"
