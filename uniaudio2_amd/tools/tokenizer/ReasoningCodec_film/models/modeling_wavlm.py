"""WavLM encoder of the codec's tokenizer (the third of its three frozen SSL encoders), host side.

The reference loads it with `AutoModel.from_pretrained(wav_lm_path)` and takes `hidden_states[6:10].mean` of a 16-kHz clip
(AudioDiffusion1D.py:233-234, 355-366); `wavlm_fea_dim = 768` makes that transformers' `WavLMModel` at the base size.  This is a
mirror of that class for the one call the codec makes: the same module tree, hence the same state-dict keys
(`feature_extractor.conv_layers.N.conv.weight`, `conv_layers.0.layer_norm`, `feature_projection.{layer_norm,projection}`,
`encoder.pos_conv_embed.conv.{bias, parametrizations.weight.original0/1}`, `encoder.layer_norm`,
`encoder.layers.N.attention.{q,k,v,out}_proj / gru_rel_pos_linear / gru_rel_pos_const / rel_attn_embed` (layer 0 only),
`encoder.layers.N.{layer_norm, feed_forward.intermediate_dense, feed_forward.output_dense, final_layer_norm}`), so a released
directory loads with strict=True.  The modules only hold parameters; `prepare()` packs them and `forward()` issues, on the device:

  conv layer 0 (Cin 1) + GroupNorm(C groups) + GELU      ua2_wavlm_conv0, time-major [B, T0, C] rows
  conv layers 1 .. 6 + GELU                              ua2_linear CAST / GELU over a strided view: the k taps of an output step are
                                                         k C consecutive floats of the time-major rows, the filter is [Cout, k Cin]
                                                         with the taps outermost (no padding: the feature extractor has none)
  feature projection: LayerNorm(512) -> Linear           ua2_linear NORM(LayerNorm) / STORE
  h + GELU(pos_conv(h)) (k 128, 16 groups, weight norm)  ua2_conv1d_grouped (weight norm, dim 2, folded once in prepare)
  encoder.layer_norm                                     ua2_layernorm_rows                               -> hidden_states[0]
  per layer (post-norm)
      gate of the relative-position bias                 ua2_relpos_gate on the layer's input rows
      q | k | v + bias, q scaled by hs^-0.5              ua2_linear CAST / QKV (no rotation) into the paged K/V
      softmax(q k^T + gate * rel_tab[key - query]) v     ua2_attn_relbias
      out_proj + bias + residual, LayerNorm              ua2_linear CAST / RESIDUAL, ua2_layernorm_rows
      intermediate_dense + GELU, output_dense + residual ua2_linear x 2
      final_layer_norm                                   ua2_layernorm_rows                               -> hidden_states[i + 1]
  mean of the taps, added in tap order                   ua2_ew_fma

Only layers 1 .. max(taps) run: the reference computes all twelve and reads hidden_states 6 .. 9, so the last three layers never
influence a token.  The relative-position table is built on the host once per T with transformers' bucket rule in
the same torch float operations (`bias_table`), [n_head, 2 T - 1] fp32, shared by all layers as transformers shares layer 0's
position_bias.  No attention mask: the reference passes none.  `dtype` is torch.float32 (the parity contract) or torch.bfloat16
(the projection, the layers' GEMMs and K/V in bf16; the whole feature extractor, the positional conv, the LayerNorms and the gate stay
fp32, so the front end is the same under both plans).  Every kernel keeps a
row-invariant summation order: a clip's features have the same bits alone and inside a batch.  transformers is not imported."""
import json
import math
import os

import torch
import torch.nn as nn

from ..... import ops
from ....._lib import EPI_GELU, EPI_QKV_ROPE, EPI_RESIDUAL, ROPE_NONE
from ._dense import DenseKV, PackedLinear

RELEASED_CONFIG = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12,
                       conv_dim=(512, 512, 512, 512, 512, 512, 512), conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2),
                       conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False, num_conv_pos_embeddings=128,
                       num_conv_pos_embedding_groups=16, num_buckets=320, max_bucket_distance=800, layer_norm_eps=1e-5,
                       feat_extract_activation="gelu", hidden_act="gelu")            # microsoft/wavlm-base(-plus)


def frame_count(n_samples, kernels=RELEASED_CONFIG["conv_kernel"], strides=RELEASED_CONFIG["conv_stride"]):
    """Frames the feature extractor makes of n_samples (no padding anywhere): 480 160 -> 1 500."""
    n = int(n_samples)
    for k, s in zip(kernels, strides):
        n = (n - k) // s + 1
    return n


def relative_buckets(relative_positions, num_buckets, max_distance):
    """transformers WavLMAttention._relative_positions_bucket, operation for operation (bidirectional: half the buckets per sign,
    exact below num_buckets / 4, log-spaced up to max_distance), so bucket boundaries agree exactly."""
    nb = num_buckets // 2
    buckets = (relative_positions > 0).to(torch.long) * nb
    rp = torch.abs(relative_positions)
    max_exact = nb // 2
    is_small = rp < max_exact
    large = torch.log(rp.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rp, large)


def bias_table(rel_attn_embed, T, num_buckets, max_distance):
    """rel_attn_embed [num_buckets, n_head] -> rel_tab [n_head, 2 T - 1] fp32 on the host: entry d + T - 1 is the bias of relative
    position d = key - query (transformers compute_bias: position_bias[h][q][k] = rel_tab[h][k - q + T - 1])."""
    d = torch.arange(-(T - 1), T, dtype=torch.long)
    return rel_attn_embed.detach().float().cpu()[relative_buckets(d, num_buckets, max_distance)].t().contiguous()


class _Conv(nn.Module):
    def __init__(self, cin, cout, k, s, group_norm):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size=k, stride=s, bias=False)
        if group_norm:
            self.layer_norm = nn.GroupNorm(num_groups=cout, num_channels=cout, affine=True)


class _FeatureExtractor(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        dims = (1,) + tuple(cfg["conv_dim"])
        self.conv_layers = nn.ModuleList([_Conv(dims[i], dims[i + 1], cfg["conv_kernel"][i], cfg["conv_stride"][i], i == 0)
                                          for i in range(len(cfg["conv_dim"]))])


class _FeatureProjection(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cfg["conv_dim"][-1], eps=cfg["layer_norm_eps"])
        self.projection = nn.Linear(cfg["conv_dim"][-1], cfg["hidden_size"])


class _PosConv(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d, k = cfg["hidden_size"], cfg["num_conv_pos_embeddings"]
        self.conv = nn.utils.parametrizations.weight_norm(nn.Conv1d(d, d, kernel_size=k, padding=k // 2, groups=cfg["num_conv_pos_embedding_groups"]),
                                                          name="weight", dim=2)


class WavLMAttention(nn.Module):
    def __init__(self, cfg, has_relative_position_bias):
        super().__init__()
        d, H = cfg["hidden_size"], cfg["num_attention_heads"]
        self.embed_dim, self.num_heads, self.head_dim = d, H, d // H
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))
        self.gru_rel_pos_const = nn.Parameter(torch.ones(1, H, 1, 1))
        self.gru_rel_pos_linear = nn.Linear(self.head_dim, 8)
        if has_relative_position_bias:
            self.rel_attn_embed = nn.Embedding(cfg["num_buckets"], H)


class _FeedForward(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.intermediate_dense = nn.Linear(cfg["hidden_size"], cfg["intermediate_size"])
        self.output_dense = nn.Linear(cfg["intermediate_size"], cfg["hidden_size"])


class WavLMEncoderLayer(nn.Module):
    def __init__(self, cfg, has_relative_position_bias):
        super().__init__()
        self.attention = WavLMAttention(cfg, has_relative_position_bias)
        self.layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])
        self.feed_forward = _FeedForward(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])

    def prepare(self, dtype):
        a, ff = self.attention, self.feed_forward
        f32 = lambda t: t.detach().float().contiguous()
        s = a.head_dim ** -0.5                       # F.multi_head_attention_forward scales q (weight and bias) by head_dim^-0.5
        w = torch.cat([f32(a.q_proj.weight) * s, f32(a.k_proj.weight), f32(a.v_proj.weight)], 0)
        b = torch.cat([f32(a.q_proj.bias) * s, f32(a.k_proj.bias), f32(a.v_proj.bias)], 0)
        ln = lambda m: (f32(m.weight), f32(m.bias), float(m.eps))
        self._p = dict(qkv=PackedLinear(w, b, dtype), out=PackedLinear(a.out_proj.weight, a.out_proj.bias, dtype),
                       fc1=PackedLinear(ff.intermediate_dense.weight, ff.intermediate_dense.bias, dtype),
                       fc2=PackedLinear(ff.output_dense.weight, ff.output_dense.bias, dtype), ln1=ln(self.layer_norm), ln2=ln(self.final_layer_norm),
                       gate_w=f32(a.gru_rel_pos_linear.weight), gate_b=f32(a.gru_rel_pos_linear.bias), gate_c=f32(a.gru_rel_pos_const).view(-1).contiguous())

    def run(self, h, kv: DenseKV, rel_tab):
        """h [B*T, d] fp32 rows -> the layer's output rows (a new tensor: the taps keep their inputs)."""
        p, a = self._p, self.attention
        M, d = h.shape
        gate = ops.relpos_gate(h, p["gate_w"], p["gate_b"], p["gate_c"], a.num_heads)
        q = torch.empty(M, d, dtype=torch.float32, device=h.device)
        p["qkv"](h, epilogue=EPI_QKV_ROPE, rope_mode=ROPE_NONE, row_pos=kv.row_pos, row_seq=kv.row_seq, q_out=q, kv=kv.geom)
        o = torch.empty_like(q)
        ops.attn_relbias(dtype=kv.dtype, R=M, q=q, row_pos=kv.all_pos, row_seq=kv.row_seq, kv=kv.geom, q_pos=kv.row_pos, gate=gate,
                         rel_tab=rel_tab, y=o, groups=kv.groups)
        x = p["out"](o, epilogue=EPI_RESIDUAL, resid=h)
        x = ops.layernorm_rows(x, *p["ln1"])
        f = p["fc1"](x, epilogue=EPI_GELU)
        y = p["fc2"](f, epilogue=EPI_RESIDUAL, resid=x)
        return ops.layernorm_rows(y, *p["ln2"])


class _Encoder(nn.Module):
    def __init__(self, cfg, n_layers):
        super().__init__()
        self.pos_conv_embed = _PosConv(cfg)
        self.layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])
        self.layers = nn.ModuleList([WavLMEncoderLayer(cfg, i == 0) for i in range(n_layers)])


def _tap_major(conv, k_mult=32):
    """nn.Conv1d weight [Cout, Cin, k] -> [Cout, k * Cin] with the taps outermost, zero-padded to a multiple of k_mult columns."""
    w = conv.weight.detach().float()
    w = w.permute(0, 2, 1).reshape(w.shape[0], -1)
    K = (w.shape[1] + k_mult - 1) // k_mult * k_mult
    out = torch.zeros(w.shape[0], K, dtype=torch.float32, device=w.device)
    out[:, :w.shape[1]] = w
    return out.contiguous()


def _gather_taps(rows, B, T, C, k, stride, K):
    """rows [B*T, C] -> ([B*Tout, K] fp32, Tout): row (b, t) = frames stride t .. stride t + k - 1 of sequence b, the operand of an
    un-padded convolution in tap-major order (columns past k C stay zero).  Data movement only."""
    Tout = (T - k) // stride + 1
    taps = rows.as_strided((B, Tout, k * C), (T * C, stride * C, 1))
    if K == k * C:
        return taps.reshape(B * Tout, K).contiguous(), Tout
    out = torch.zeros(B, Tout, K, dtype=torch.float32, device=rows.device)
    out[:, :, :k * C] = taps
    return out.view(B * Tout, K), Tout


class WavLMEncoder(nn.Module):
    def __init__(self, config=None, taps=(6, 7, 8, 9), **kw):
        super().__init__()
        cfg = dict(RELEASED_CONFIG)
        cfg.update({k: v for k, v in (config or {}).items() if k in RELEASED_CONFIG})
        cfg.update(kw)
        self.config = {k: cfg[k] for k in RELEASED_CONFIG}
        self.taps = tuple(int(t) for t in taps)
        d, H = cfg["hidden_size"], cfg["num_attention_heads"]
        if cfg["feat_extract_norm"] != "group":
            raise NotImplementedError(f"feat_extract_norm = {cfg['feat_extract_norm']!r}: only the 'group' feature extractor of WavLM base "
                                      "(GroupNorm after the first convolution) is built")
        if cfg["do_stable_layer_norm"]:
            raise NotImplementedError("do_stable_layer_norm = True (the pre-norm encoder of WavLM large) is not built")
        if cfg["conv_bias"]:
            raise NotImplementedError("conv_bias = True: the feature extractor of WavLM base has no convolution bias; not built")
        if cfg["feat_extract_activation"] != "gelu" or cfg["hidden_act"] != "gelu":
            raise NotImplementedError("only the erf GELU of WavLM base is built (feat_extract_activation / hidden_act = 'gelu')")
        if d % H or (d // H) % 16:
            raise NotImplementedError(f"head size {d / H:g} (hidden {d} / {H} heads) is not a multiple of 16")
        g = cfg["num_conv_pos_embedding_groups"]
        if d % g or (d // g) % 16:
            raise NotImplementedError(f"hidden / groups = {d} / {g} is not a multiple of 16 (ua2_conv1d_grouped)")
        if not self.taps or min(self.taps) < 0 or max(self.taps) > cfg["num_hidden_layers"]:
            raise ValueError(f"taps {self.taps} outside hidden_states[0 .. {cfg['num_hidden_layers']}]")
        if not (len(cfg["conv_dim"]) == len(cfg["conv_kernel"]) == len(cfg["conv_stride"])):
            raise ValueError("conv_dim, conv_kernel and conv_stride differ in length")
        self.hidden_size, self.heads = d, H
        self.feature_extractor = _FeatureExtractor(cfg)
        self.feature_projection = _FeatureProjection(cfg)
        self.encoder = _Encoder(cfg, max(self.taps))                    # layers past the last tap are never computed
        self._p = None
        self._kvs, self._tabs = {}, {}

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
            try:
                return torch.load(pt, map_location="cpu", weights_only=True), pt
            except Exception:
                return torch.load(pt, map_location="cpu", weights_only=False), pt
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")

    def filter_state_dict(self, sd):
        """A transformers WavLMModel state dict -> the keys of this module tree: a `wavlm.` prefix stripped, `masked_spec_embed` and
        the layers past the last tap dropped, the old `weight_g` / `weight_v` spelling of the positional conv's weight norm renamed."""
        n = len(self.encoder.layers)
        rename = {"encoder.pos_conv_embed.conv.weight_g": "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
                  "encoder.pos_conv_embed.conv.weight_v": "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
        own = {}
        for k, v in sd.items():
            if k.startswith("wavlm."):
                k = k[len("wavlm."):]
            k = rename.get(k, k)
            if k == "masked_spec_embed":
                continue
            if k.startswith("encoder.layers.") and int(k.split(".")[2]) >= n:
                continue
            own[k] = v
        return own

    @classmethod
    def from_pretrained(cls, path, taps=(6, 7, 8, 9)):
        """`path`: a directory with config.json + model.safetensors / pytorch_model.bin (a transformers WavLMModel).  Loads with
        strict=True after `filter_state_dict`: a parameter the file does not name, or a key this tree does not have, is an error."""
        with open(os.path.join(path, "config.json"), "r", encoding="utf-8") as f:
            cfg = json.load(f)
        model = cls({k: cfg[k] for k in RELEASED_CONFIG if k in cfg}, taps=taps)
        sd, src = cls.read_checkpoint(path)
        try:
            model.load_state_dict(model.filter_state_dict(sd), strict=True)
        except RuntimeError as e:
            raise RuntimeError(f"{src}: not the state dict of a WavLMModel of this config — {e}") from None
        return model

    # ---- plan --------------------------------------------------------------------------------------------------
    def prepare(self, dtype=torch.float32):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"WavLMEncoder.prepare: dtype {dtype}; torch.float32 (parity) or torch.bfloat16")
        dev = self.encoder.layer_norm.weight.device
        if dev.type != "cuda":
            raise RuntimeError("uniaudio2_amd runs on a ROCm device only (no CPU fallback); move the model to cuda")
        f32 = lambda t: t.detach().float().contiguous()
        ln = lambda m: (f32(m.weight), f32(m.bias), float(m.eps))
        cl = self.feature_extractor.conv_layers
        for l in self.encoder.layers:
            l.prepare(dtype)
        pc = self.encoder.pos_conv_embed.conv
        par = pc.parametrizations.weight
        w_pos = torch._weight_norm(f32(par.original1), f32(par.original0), 2)           # g * v / ||v|| over (out, in) per tap: folded once
        self._p = dict(dtype=dtype, w0=f32(cl[0].conv.weight).view(cl[0].conv.out_channels, -1).contiguous(),
                       gn=(f32(cl[0].layer_norm.weight), f32(cl[0].layer_norm.bias), float(cl[0].layer_norm.eps)),
                       convs=[PackedLinear(_tap_major(c.conv), None, torch.float32) for c in list(cl)[1:]],
                       proj=PackedLinear(self.feature_projection.projection.weight, self.feature_projection.projection.bias, dtype),
                       proj_ln=ln(self.feature_projection.layer_norm),
                       pos_w=ops.pack_conv1d_grouped_weight(w_pos, pc.groups), pos_b=f32(pc.bias), ln=ln(self.encoder.layer_norm),
                       rel=f32(self.encoder.layers[0].attention.rel_attn_embed.weight) if len(self.encoder.layers) else None)
        self._kvs, self._tabs = {}, {}
        return self

    def frames(self, n_samples):
        return frame_count(n_samples, self.config["conv_kernel"], self.config["conv_stride"])

    def front_end(self, wav):
        """wav [B, N] fp32 on the device -> (feature-extractor rows [B*T, conv_dim[-1]] fp32, T): transformers' `extract_features`
        before the projection's LayerNorm."""
        p, cfg = self._p, self.config
        B, N = wav.shape
        if self.frames(N) < 1:
            raise ValueError(f"WavLMEncoder: {N} samples make no frame")
        w0, (gw, gb, eps) = p["w0"], p["gn"]
        y = ops.wavlm_conv0(wav.float().contiguous(), w0, gw, gb, cfg["conv_stride"][0], eps)
        T, C = y.shape[1], y.shape[2]
        rows = y.view(B * T, C)
        for i, lin in enumerate(p["convs"], start=1):
            x, T = _gather_taps(rows, B, T, C, cfg["conv_kernel"][i], cfg["conv_stride"][i], lin.K)
            rows, C = lin(x, epilogue=EPI_GELU), lin.N
        return rows, T

    def rel_table(self, T, device):
        tab = self._tabs.get((T, str(device)))
        if tab is None:
            tab = self._tabs[(T, str(device))] = bias_table(self._p["rel"], T, self.config["num_buckets"], self.config["max_bucket_distance"]).to(device)
        return tab

    @torch.inference_mode()
    def hidden_states(self, wav_16k, upto=None):
        """wav_16k [B, N] -> list of hidden_states[0 .. upto] (each (B, T, hidden) fp32), upto = max(taps) by default."""
        if self._p is None:
            self.prepare()
        p = self._p
        upto = max(self.taps) if upto is None else upto
        B = wav_16k.shape[0]
        rows, T = self.front_end(wav_16k)
        h = p["proj"](rows, norm=p["proj_ln"])
        pc = self.encoder.pos_conv_embed.conv
        h = ops.conv1d_grouped(h, p["pos_w"], B, T, pc.groups, pc.kernel_size[0], bias=p["pos_b"], resid=h, gelu=True)
        h = ops.layernorm_rows(h, *p["ln"])
        out = [h]
        if upto > 0:
            kv = self._kvs.get((B, T))
            if kv is None:
                kv = self._kvs[(B, T)] = DenseKV(B, T, self.heads, self.hidden_size // self.heads, p["dtype"], h.device)
            tab = self.rel_table(T, h.device)
            for l in list(self.encoder.layers)[:upto]:
                h = l.run(h, kv, tab)
                out.append(h)
        return [t.view(B, T, self.hidden_size) for t in out]

    @torch.inference_mode()
    def forward(self, wav_16k):
        """wav_16k [B, N] fp32 on the device -> (B, T, hidden) fp32: the mean of hidden_states[taps], added in tap order."""
        hs = self.hidden_states(wav_16k)
        acc = hs[self.taps[0]]
        for t in self.taps[1:]:
            acc = ops.ew_fma(acc, c=hs[t])
        return ops.ew_fma(acc, alpha=1.0 / len(self.taps))
