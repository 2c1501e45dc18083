#!/usr/bin/env python3
"""WavLM encoder at the released size (WavLM base: conv_dim 512 x 7, hidden 768, 12 heads, ffn 3072, nine layers run, taps 6 .. 9) on
seeded random weights, one 30-s segment (480 160 samples at 16 kHz -> 1 500 frames) and six (the audio2token chunk), fp32 and bf16 plans:
device-event time per stage (first layer, conv GEMMs 1 .. 6, projection, positional conv, encoder LayerNorm, the nine layers, tap mean)
and per new kernel (ua2_wavlm_conv0, ua2_conv1d_grouped, ua2_relpos_gate, ua2_attn_relbias at both precisions).

With --e2e: ReasoningTokenizer.audio2token of one 30-s clip through the released-size Whisper-medium, BEST-RQ and WavLM encoders and the
codec's encode stages at the released widths (random weights, no callable), the figure to set beside profiles/whisper_frontend.txt and
profiles/bestrq_encoder.txt.

Every figure is the median of --iters timed calls after 2 warm-up calls (device events around the call; the device is otherwise idle).
python tools/ubench/wavlm_encoder.py [--out profiles/wavlm_encoder.txt] [--iters 7] [--batches 1,6] [--e2e]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

import wavlm_ref as wr
from uniaudio2_amd import ops
from uniaudio2_amd._lib import EPI_GELU
from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models._dense import DenseKV
from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_wavlm import RELEASED_CONFIG, WavLMEncoder, _gather_taps


def median_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def e2e(say, iters):
    """audio2token of one 30-s clip: released-size Whisper-medium (bf16), BEST-RQ (fp32) and WavLM (fp32, and bf16) encoders + the codec's
    encode stages at the released widths, all on random weights, no callable."""
    import bestrq_ref as br
    import whisper_ref as whr
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models import modeling_whisper
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.PretrainedModel import BESTRQ_Model
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model import musicfm_25hz as mf
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    torch.manual_seed(3)
    m = AudioDiffusion1D(use_detokenizer=False).cuda().prepare()
    wcfg = dict(modeling_whisper.RELEASED_CONFIG)
    wenc = modeling_whisper.WhisperEncoder(wcfg)
    wenc.load_state_dict(whr.encoder_state_dict(wcfg, seed=7300), strict=True)
    mus = mf.MusicFM25Hz(dict(mf.RELEASED_CONFIG), taps=mf.TAPS)
    mus.load_state_dict(br.state_dict(dict(mf.RELEASED_CONFIG), seed=8500, n_layers=max(mf.TAPS)), strict=True)
    lenc = WavLMEncoder(dict(RELEASED_CONFIG))
    lenc.load_state_dict(wr.state_dict(dict(RELEASED_CONFIG), seed=6700, n_layers=9), strict=True)
    object.__setattr__(m, "whisper_encoder", wenc.cuda().prepare(torch.bfloat16))
    object.__setattr__(m, "bestrq_encoder", BESTRQ_Model(model=mus.cuda(), layers=mf.TAPS, dtype=torch.float32))
    tok = ReasoningTokenizer(model=m, device="cuda")
    clip = (0.1 * torch.randn(1, 30 * 24000 - 240, generator=torch.Generator().manual_seed(9))).cuda()
    for dtype in (torch.float32, torch.bfloat16):
        object.__setattr__(m, "wavlm_encoder", lenc.cuda().prepare(dtype))
        t = median_ms(lambda: tok.audio2token(clip, 24000), max(3, iters // 2))
        reason, rec = tok.audio2token(clip, 24000)
        t_w = median_ms(lambda: m.get_wavlm_feature(clip[:, None, :], 750), max(3, iters // 2))
        say(f"audio2token, one 30-s clip (one segment), Whisper bf16 + BEST-RQ fp32 + WavLM {str(dtype)}: {t:9.3f} ms end to end "
            f"-> reason {tuple(reason.shape)}, rec {tuple(rec.shape)}; get_wavlm_feature alone (resample + encoder) {t_w:8.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--batches", default="1,6")
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wavlm_encoder.py measures on the GPU; none found")
    cfg = dict(RELEASED_CONFIG)
    enc = WavLMEncoder(cfg)
    enc.load_state_dict(wr.state_dict(cfg, seed=6700, n_layers=max(enc.taps)), strict=True)
    enc = enc.cuda()
    lines = [f"WavLM encoder, released size (hidden {cfg['hidden_size']}, {cfg['num_attention_heads']} heads, ffn {cfg['intermediate_size']}, "
             f"taps {enc.taps}: {max(enc.taps)} layers run), seeded random weights; device-event ms per call, median of {a.iters} after 2 warm-up calls"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    g = torch.Generator().manual_seed(5)
    batches = [int(b) for b in a.batches.split(",")]
    wav = (0.1 * torch.randn(max(batches), 480160, generator=g)).cuda()
    d, H = cfg["hidden_size"], cfg["num_attention_heads"]
    for B in batches:
        w = wav[:B].contiguous()
        for dtype in (torch.float32, torch.bfloat16):
            enc.prepare(dtype)
            p = enc._p
            tag = f"B={B} {str(dtype):15s}"
            t_c0 = median_ms(lambda: ops.wavlm_conv0(w, p["w0"], p["gn"][0], p["gn"][1], cfg["conv_stride"][0], p["gn"][2]), a.iters)
            y = ops.wavlm_conv0(w, p["w0"], p["gn"][0], p["gn"][1], cfg["conv_stride"][0], p["gn"][2])
            gb = y.numel() * 4 / 1e9
            say(f"{tag}: ua2_wavlm_conv0 {t_c0:8.3f} ms   ({tuple(y.shape)}: {gb:.3f} GB written, {gb / (t_c0 * 1e-3):.0f} GB/s)")
            T, C = y.shape[1], y.shape[2]
            rows = y.view(B * T, C)
            del y
            t_gemm = 0.0
            for i, lin in enumerate(p["convs"], start=1):
                k, s = cfg["conv_kernel"][i], cfg["conv_stride"][i]
                src, Tin = rows, T
                t_g = median_ms(lambda: _gather_taps(src, B, Tin, C, k, s, lin.K), a.iters)
                x, T = _gather_taps(src, B, Tin, C, k, s, lin.K)
                t_l = median_ms(lambda: lin(x, epilogue=EPI_GELU), a.iters)
                fl = 2.0 * x.shape[0] * lin.K * lin.N
                say(f"{tag}: conv layer {i} [k {k}, stride {s}, {Tin} -> {T} frames] gather {t_g:7.3f} ms + GEMM {t_l:7.3f} ms ({fl / t_l / 1e9:6.1f} TFLOP/s, fp32)")
                t_gemm += t_g + t_l
                rows = lin(x, epilogue=EPI_GELU)
                del x
            t_front = median_ms(lambda: enc.front_end(w), a.iters)
            say(f"{tag}: front end {t_front:8.3f} ms   (first layer {t_c0:.3f} + conv GEMMs and gathers {t_gemm:.3f})")
            t_proj = median_ms(lambda: p["proj"](rows, norm=p["proj_ln"]), a.iters)
            h = p["proj"](rows, norm=p["proj_ln"])
            pc = enc.encoder.pos_conv_embed.conv
            K = pc.kernel_size[0]
            t_pos = median_ms(lambda: ops.conv1d_grouped(h, p["pos_w"], B, T, pc.groups, K, bias=p["pos_b"], resid=h, gelu=True), a.iters)
            fl = 2.0 * B * T * d * (d // pc.groups) * K
            say(f"{tag}: projection {t_proj:7.3f} ms; ua2_conv1d_grouped [k {K}, {pc.groups} groups, T {T}] {t_pos:8.3f} ms   ({fl / t_pos / 1e9:6.1f} TFLOP/s, exact fp32)")
            h = ops.layernorm_rows(ops.conv1d_grouped(h, p["pos_w"], B, T, pc.groups, K, bias=p["pos_b"], resid=h, gelu=True), *p["ln"])
            kv = DenseKV(B, T, H, d // H, dtype, h.device)
            tab = enc.rel_table(T, h.device)
            l0 = enc.encoder.layers[0]
            lp = l0._p
            t_gate = median_ms(lambda: ops.relpos_gate(h, lp["gate_w"], lp["gate_b"], lp["gate_c"], H), a.iters)
            gate = ops.relpos_gate(h, lp["gate_w"], lp["gate_b"], lp["gate_c"], H)
            q = torch.empty(B * T, d, device=h.device)
            from uniaudio2_amd._lib import EPI_QKV_ROPE, ROPE_NONE
            lp["qkv"](h, epilogue=EPI_QKV_ROPE, rope_mode=ROPE_NONE, row_pos=kv.row_pos, row_seq=kv.row_seq, q_out=q, kv=kv.geom)
            o = torch.empty_like(q)
            att = lambda: ops.attn_relbias(dtype=dtype, R=B * T, q=q, row_pos=kv.all_pos, row_seq=kv.row_seq, kv=kv.geom, q_pos=kv.row_pos, gate=gate,
                                           rel_tab=tab, y=o, groups=kv.groups)
            t_att = median_ms(att, a.iters)
            fl = 4.0 * B * H * T * T * (d // H)
            say(f"{tag}: ua2_relpos_gate {t_gate:7.3f} ms; ua2_attn_relbias [{H} heads x {T} keys] {t_att:8.3f} ms   ({fl / t_att / 1e9:6.1f} TFLOP/s)")
            t_layer = median_ms(lambda: l0.run(h, kv, tab), a.iters)
            t_all = median_ms(lambda: enc(w), a.iters)
            n = max(enc.taps)
            say(f"{tag}: one layer {t_layer:8.3f} ms (x {n} = {n * t_layer:8.3f}); whole forward {t_all:8.3f} ms "
                f"(front end {t_front:.3f}, projection + positional conv {t_proj + t_pos:.3f}, {n} layers + tap mean {t_all - t_front - t_proj - t_pos:.3f})")
            del rows, h, q, o, kv
            torch.cuda.empty_cache()
    if a.e2e:
        e2e(say, a.iters)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
