"""Whisper encoder of the codec's tokenizer (the heaviest of its three frozen SSL encoders), host side.

Mirror of the reference's tools/tokenizer/ReasoningCodec_film/models/modeling_whisper.py `WhisperEncoder` (:723-866) over
`WhisperEncoderLayer` / `WhisperAttention`: same class and attribute names, hence the same state-dict keys (`conv1`, `conv2`,
`embed_positions.weight`, `layers.N.self_attn.{q,k,v,out}_proj` with no bias on k_proj, `self_attn_layer_norm`, `fc1`, `fc2`,
`final_layer_norm`, `layer_norm`), so a Whisper checkpoint's `model.encoder.*` loads.  The modules only hold parameters;
`prepare()` packs them and `forward()` issues, on the device:

  conv1 (k 3, pad 1) + exact-erf GELU        ua2_linear CAST / GELU over the gathered [B T, 3 x 80] operand     :805
  conv2 (k 3, stride 2, pad 1) + GELU        ua2_linear CAST / GELU over the gathered [B P, 3 d] operand        :806
                                             (the GEMM's rows ARE the [T, C] layout: the permute of :808 vanishes)
  + embed_positions.weight                   ua2_ew_fma                                                         :809-811
  per layer  LayerNorm -> q | k | v + bias   ua2_linear NORM(LayerNorm) / QKV (no rotation)                     :386-392, 264-275
             softmax(q k^T / sqrt(hd)) v     ua2_attn, every row over all P positions (the reference scales q by
                                             hd^-0.5 after q_proj :273; the kernel scales the scores, once)
             out_proj + bias + residual      ua2_linear CAST / RESIDUAL                                         :393-394
             LayerNorm -> fc1 + erf-GELU     ua2_linear NORM / GELU                                             :397-398
             fc2 + bias + residual           ua2_linear CAST / RESIDUAL                                         :400-402
  layer_norm                                 ua2_layernorm_rows                                                 :850

The two convolutions run as GEMMs so that they reach the matrix pipe: with the activation kept as zero-padded [T + 2, C]
rows, the three taps of output step t are 3 C consecutive floats (rows s t .. s t + 2), so the operand is a strided copy
(data movement only) and the filter is the [Cout, 3 Cin] matrix with the taps outermost.  `dtype` is torch.float32 (the
parity contract) or torch.bfloat16 (speed; the reference itself runs this encoder under bf16 autocast,
reason_tokenizer.py:117).  Every GEMM keeps the row-invariant summation order: a clip's features have the same bits alone
and inside a batch.  transformers is not imported."""
import json
import os

import torch
import torch.nn as nn

from ..... import ops
from ....._lib import EPI_GELU, EPI_QKV_ROPE, EPI_RESIDUAL, ROPE_NONE
from ._dense import DenseKV, PackedLinear

RELEASED_CONFIG = dict(d_model=1024, encoder_layers=24, encoder_attention_heads=16, encoder_ffn_dim=4096, num_mel_bins=80,
                       max_source_positions=1500)           # whisper-medium, the encoder the released codec was trained on


class WhisperAttention(nn.Module):
    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        if self.head_dim * num_heads != embed_dim:
            raise ValueError(f"embed_dim must be divisible by num_heads (got `embed_dim`: {embed_dim} and `num_heads`: {num_heads}).")
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=False)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)


class WhisperEncoderLayer(nn.Module):
    def __init__(self, d_model, heads, ffn_dim):
        super().__init__()
        self.embed_dim = d_model
        self.self_attn = WhisperAttention(d_model, heads)
        self.self_attn_layer_norm = nn.LayerNorm(d_model)
        self.fc1 = nn.Linear(d_model, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, d_model)
        self.final_layer_norm = nn.LayerNorm(d_model)

    def prepare(self, dtype):
        a = self.self_attn
        f32 = lambda t: t.detach().float().contiguous()
        w = torch.cat([f32(a.q_proj.weight), f32(a.k_proj.weight), f32(a.v_proj.weight)], 0)
        b = torch.cat([f32(a.q_proj.bias), torch.zeros_like(f32(a.q_proj.bias)), f32(a.v_proj.bias)], 0)     # k_proj has no bias
        ln = lambda m: (f32(m.weight), f32(m.bias), float(m.eps))
        self._p = dict(dtype=dtype, qkv=PackedLinear(w, b, dtype), out=PackedLinear(a.out_proj.weight, a.out_proj.bias, dtype),
                       fc1=PackedLinear(self.fc1.weight, self.fc1.bias, dtype), fc2=PackedLinear(self.fc2.weight, self.fc2.bias, dtype),
                       ln1=ln(self.self_attn_layer_norm), ln2=ln(self.final_layer_norm))

    def run(self, h, kv: DenseKV):
        """h [B*P, d] fp32 rows, updated in place."""
        p, d = self._p, self.embed_dim
        M = h.shape[0]
        q = torch.empty(M, d, dtype=torch.float32, device=h.device)
        p["qkv"](h, epilogue=EPI_QKV_ROPE, norm=p["ln1"], rope_mode=ROPE_NONE, row_pos=kv.row_pos, row_seq=kv.row_seq, q_out=q, kv=kv.geom)
        if kv.groups is not None and M > 16 and d % 32 == 0 and p["fc2"].K % 32 == 0:
            # bf16 plan at many rows: attention and GELU write their consumer's operand in fragment order (the rounding the
            # consumer's own prep launch applies: identical bits, two launches less per layer)
            ws_o = ops.linear_workspace(p["dtype"], M, d, h.device)
            ws_f = ops.linear_workspace(p["dtype"], M, p["fc2"].K, h.device)
            kv.attend(q, y_packed=ws_o)
            p["out"](None, M=M, x_packed=ws_o, epilogue=EPI_RESIDUAL, resid=h, y=h)
            p["fc1"](h, epilogue=EPI_GELU, norm=p["ln2"], y_packed=ws_f)
            p["fc2"](None, M=M, x_packed=ws_f, epilogue=EPI_RESIDUAL, resid=h, y=h)
            return h
        o = kv.attend(q)
        p["out"](o, epilogue=EPI_RESIDUAL, resid=h, y=h)
        f = p["fc1"](h, epilogue=EPI_GELU, norm=p["ln2"])
        p["fc2"](f, epilogue=EPI_RESIDUAL, resid=h, y=h)
        return h


def _tap_major(conv, k_pad=1):
    """nn.Conv1d weight [Cout, Cin, k] -> [Cout, k * Cin] with the taps outermost (the order of k consecutive [Cin] rows), K
    zero-padded to a multiple of k_pad."""
    w = conv.weight.detach().float()
    w = w.permute(0, 2, 1).reshape(w.shape[0], -1)
    K = (w.shape[1] + k_pad - 1) // k_pad * k_pad
    out = torch.zeros(w.shape[0], K, dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out.contiguous()


def _gather_taps(rows, B, T, C, stride, K):
    """rows [B*T, C] -> [B*Tout, K] fp32: row (b, t) = frames stride t - 1 .. stride t + 1 of sequence b (zero beyond both ends),
    i.e. the operand of a k 3 / pad 1 convolution in tap-major order (columns past 3 C stay zero).  Data movement only."""
    xp = torch.zeros(B, T + 2, C, dtype=torch.float32, device=rows.device)
    xp[:, 1:T + 1] = rows.view(B, T, C)
    Tout = (T - 1) // stride + 1
    taps = xp.as_strided((B, Tout, 3 * C), ((T + 2) * C, stride * C, 1))
    if K == 3 * C:
        return taps.reshape(B * Tout, K).contiguous(), Tout
    out = torch.zeros(B, Tout, K, dtype=torch.float32, device=rows.device)
    out[:, :, :3 * C] = taps
    return out.view(B * Tout, K), Tout


class WhisperEncoder(nn.Module):
    def __init__(self, config=None, **kw):
        super().__init__()
        cfg = dict(RELEASED_CONFIG)
        cfg.update(config or {})
        cfg.update(kw)
        self.config = {k: cfg[k] for k in RELEASED_CONFIG}
        d = cfg["d_model"]
        self.num_mel_bins, self.max_source_positions = cfg["num_mel_bins"], cfg["max_source_positions"]
        self.d_model, self.heads = d, cfg["encoder_attention_heads"]
        if cfg.get("scale_embedding"):
            raise NotImplementedError("scale_embedding is not used by any Whisper encoder checkpoint and is not built")
        self.conv1 = nn.Conv1d(self.num_mel_bins, d, kernel_size=3, padding=1)
        self.conv2 = nn.Conv1d(d, d, kernel_size=3, stride=2, padding=1)
        self.embed_positions = nn.Embedding(self.max_source_positions, d)
        self.layers = nn.ModuleList([WhisperEncoderLayer(d, self.heads, cfg["encoder_ffn_dim"]) for _ in range(cfg["encoder_layers"])])
        self.layer_norm = nn.LayerNorm(d)
        self._p = None
        self._kvs = {}

    # ---- loading -----------------------------------------------------------------------------------------------
    @staticmethod
    def read_checkpoint(path):
        """state dict of `model.safetensors` or `pytorch_model.bin` in directory `path`."""
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            return load_file(st), st
        pt = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(pt):
            return torch.load(pt, map_location="cpu"), pt
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")

    @classmethod
    def from_pretrained(cls, path):
        """`path`: a directory with config.json + model.safetensors / pytorch_model.bin (a Whisper checkpoint, or its encoder
        alone).  `encoder.` / `model.encoder.` prefixes are stripped, decoder keys ignored; a parameter of this module tree
        that the file does not name is an error (never silently random weights)."""
        with open(os.path.join(path, "config.json"), "r", encoding="utf-8") as f:
            cfg = json.load(f)
        model = cls({k: cfg[k] for k in RELEASED_CONFIG if k in cfg})
        sd, src = cls.read_checkpoint(path)
        mine = model.state_dict()
        own = {}
        for k, v in sd.items():
            for prefix in ("model.encoder.", "encoder."):
                if k.startswith(prefix):
                    k = k[len(prefix):]
                    break
            if k in mine:
                own[k] = v
        missing = sorted(set(mine) - set(own))
        if missing:
            raise RuntimeError(f"{src}: {len(missing)} parameter(s) of the Whisper encoder are not in the checkpoint "
                               f"(first: {missing[:5]}) — a key-name mismatch between this module tree and the checkpoint")
        model.load_state_dict(own, strict=True)
        return model

    # ---- plan --------------------------------------------------------------------------------------------------
    def prepare(self, dtype=torch.bfloat16):
        dev = self.layer_norm.weight.device
        if dev.type != "cuda":
            raise RuntimeError("uniaudio2_amd runs on a ROCm device only (no CPU fallback); move the model to cuda")
        f32 = lambda t: t.detach().float().contiguous()
        for l in self.layers:
            l.prepare(dtype)
        self._p = dict(dtype=dtype, conv1=PackedLinear(_tap_major(self.conv1, 64), self.conv1.bias, dtype),
                       conv2=PackedLinear(_tap_major(self.conv2, 64), self.conv2.bias, dtype),
                       pos=f32(self.embed_positions.weight), ln=(f32(self.layer_norm.weight), f32(self.layer_norm.bias), float(self.layer_norm.eps)))
        self._kvs = {}
        return self

    def stem(self, mels):
        """mels [B, n_mels, T] -> rows [B*P, d] of gelu(conv2(gelu(conv1(mels)))) + embed_positions (:805-811), P."""
        p = self._p
        B, Cm, T = mels.shape
        if Cm != self.num_mel_bins or (T - 1) // 2 + 1 != self.max_source_positions:
            raise ValueError(f"WhisperEncoder: mels of shape {tuple(mels.shape)}; expected [B, {self.num_mel_bins}, {2 * self.max_source_positions}] "
                             "(the positional table is added whole, as in the reference)")
        x1, _ = _gather_taps(mels.float().transpose(1, 2).reshape(B * T, Cm), B, T, Cm, 1, p["conv1"].K)
        h1 = p["conv1"](x1, epilogue=EPI_GELU)
        x2, P = _gather_taps(h1, B, T, self.d_model, 2, p["conv2"].K)
        h = p["conv2"](x2, epilogue=EPI_GELU)
        return ops.ew_fma(h, c=p["pos"], out=h), P                     # + embed_pos: the modulo broadcast repeats it per batch element

    @torch.inference_mode()
    def forward(self, mels):
        """mels [B, num_mel_bins, 2 P] fp32 on the device -> last_hidden_state [B, P, d_model] fp32."""
        if self._p is None:
            self.prepare()
        B = mels.shape[0]
        h, P = self.stem(mels)
        kv = self._kvs.get((B, P))
        if kv is None:
            kv = self._kvs[(B, P)] = DenseKV(B, P, self.heads, self.d_model // self.heads, self._p["dtype"], h.device)
        for l in self.layers:
            l.run(h, kv)
        w, b, eps = self._p["ln"]
        return ops.layernorm_rows(h, w, b, eps).view(B, P, self.d_model)
