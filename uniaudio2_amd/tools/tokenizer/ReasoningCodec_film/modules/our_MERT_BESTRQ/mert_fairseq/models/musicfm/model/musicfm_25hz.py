"""BEST-RQ (MusicFM 25 Hz) encoder of the codec's tokenizer — the source of `bestrq_acoustic` / `bestrq_semantic` — host side.

Mirror of the reference's modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm/model/musicfm_25hz.py `MusicFM25Hz` over
modules/conv.py (`Res2dModule`, `Conv2dSubsampling`) and transformers' `Wav2Vec2ConformerEncoder` as configured by the reference's
w2v2_config.json (rotary positions, swish, depthwise kernel 31): same class and attribute names, hence the same state-dict keys
(`conv.conv.{0,1}.{conv1,bn1,conv2,bn2,conv3,bn3}`, `conv.linear`, `conformer.layers.N.{ffn1_layer_norm, ffn1.*, self_attn_layer_norm,
self_attn.linear_{q,k,v,out}, conv_module.*, ffn2_layer_norm, ffn2.*, final_layer_norm}`), so a MusicFM checkpoint loads.  The modules
only hold parameters; `prepare()` packs them and `forward()` issues, on the device:

  mel front end   ops.melspec: exact-fp32 ua2_linear against the windowed DFT basis + ua2_melspec_db        musicfm_25hz.py:199-233
  stem            per Res2dModule three ua2_conv2d launches (BatchNorm2d folded, ReLU / residual fused)      modules/conv.py:36-42
                  "b c f t -> b t (c f)" (a copy) + linear                                                   modules/conv.py:80-81
  per layer       LayerNorm -> intermediate_dense | swish | output_dense x 0.5 + residual                    HF encoder layer :600-604
                  ua2_layernorm_rope_rows -> [rot | plain]; ONE ua2_linear over it with the block weight
                  [[Wq, 0], [Wk, 0], [0, Wv]] (QKV epilogue, no rotation, K/V to DenseKV); ua2_attn over all
                  positions, no mask; linear_out + residual                                                  :608-616, 466-505
                  LayerNorm -> pointwise_conv1 + GLU (UA2_GATE_SIGMOID_SECOND) -> ua2_dwconv1d (k 31, the
                  eval BatchNorm1d folded) -> swish -> pointwise_conv2 + residual                            :398-417
                  FFN 2 as FFN 1; final_layer_norm                                                           :624-628

The codec builds `BESTRQ_Model(..., layers = [4, 11])` (AudioDiffusion1D.py:237-238; the class default [3, 11] is not what the
tokenizer uses).  The two numbers index the encoder's `hidden_states`, whose entry k is the INPUT of layer k: only layers 0 .. 10 run
and the row sets after layers 3 and 10 are returned.  pos_conv_embed, the encoder's final layer_norm, the last layer, `linear`,
`cls_token` and the quantizers are never evaluated and are not part of this module tree.

`dtype` of prepare(): torch.float32 is the parity plan and the default — the reference runs this encoder in fp32
(AudioDiffusion1D.py:502 `autocast(enabled=False)`) — torch.bfloat16 an opt-in speed plan of the conformer's GEMMs; the stem and the mel
front end are always exact fp32 (their features feed integer RVQ decisions).  Every GEMM keeps the row-invariant summation order: a
clip's features have the same bits alone and inside a batch.  transformers is not imported; there is no CPU fallback."""
import torch
import torch.nn as nn

from uniaudio2_amd import ops
from uniaudio2_amd._lib import EPI_QKV_ROPE, EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, EW_SILU, GATE_SIGMOID_SECOND, ROPE_NONE
from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models._dense import DenseKV, PackedLinear

# MusicFM25Hz defaults + the values of the reference's w2v2_config.json that the encoder reads
RELEASED_CONFIG = dict(n_mels=128, conv_dim=512, encoder_dim=1024, encoder_depth=12, num_attention_heads=16, intermediate_size=4096,
                       conv_depthwise_kernel_size=31, rotary_embedding_base=10000, layer_norm_eps=1e-5)
TAPS = (4, 11)                      # AudioDiffusion1D.py:238 BESTRQ_Model(layers = [4, 11]): (acoustic, semantic)
# checkpoint keys that belong to parts the tokenizer never evaluates
UNUSED_PREFIXES = ("conformer.pos_conv_embed.", "conformer.layer_norm.", "conformer.embed_positions.", "linear.", "cls_token", "quantizer_",
                   "rvq.", "preprocessor_", "loss.")

_f32 = lambda t: t.detach().float().contiguous()


def fold_batchnorm(weight, bias, bn):
    """(w', b') of conv + eval-mode BatchNorm: w' = w g / sqrt(var + eps) per output channel, b' = (b - mean) g / sqrt(var + eps) + beta."""
    g = _f32(bn.weight) / torch.sqrt(_f32(bn.running_var) + bn.eps)
    w = _f32(weight) * g.view(-1, *([1] * (weight.dim() - 1)))
    b0 = _f32(bias) if bias is not None else torch.zeros_like(g)
    return w.contiguous(), ((b0 - _f32(bn.running_mean)) * g + _f32(bn.bias)).contiguous()


class Res2dModule(nn.Module):
    def __init__(self, idim, odim, stride=(2, 2)):
        super().__init__()
        self.stride, self.odim = tuple(stride), odim
        self.conv1 = nn.Conv2d(idim, odim, 3, padding=1, stride=stride)
        self.bn1 = nn.BatchNorm2d(odim)
        self.conv2 = nn.Conv2d(odim, odim, 3, padding=1)
        self.bn2 = nn.BatchNorm2d(odim)
        self.diff = False
        if (idim != odim) or (stride[0] > 1):
            self.conv3 = nn.Conv2d(idim, odim, 3, padding=1, stride=stride)
            self.bn3 = nn.BatchNorm2d(odim)
            self.diff = True

    def prepare(self):
        self._p = {}
        for i in (1, 2, 3) if self.diff else (1, 2):
            conv = getattr(self, f"conv{i}")
            w, b = fold_batchnorm(conv.weight, conv.bias, getattr(self, f"bn{i}"))
            self._p[i] = (ops.pack_conv2d_weight(w), b)

    def run(self, x):
        """relu(shortcut(x) + bn2(conv2(relu(bn1(conv1(x)))))) — three launches (two without the strided shortcut)."""
        p = self._p
        h = ops.conv2d(x, p[1][0], self.odim, stride=self.stride, bias=p[1][1], relu=True)
        sc = ops.conv2d(x, p[3][0], self.odim, stride=self.stride, bias=p[3][1]) if self.diff else x
        return ops.conv2d(h, p[2][0], self.odim, bias=p[2][1], residual=sc, relu=True)


class Conv2dSubsampling(nn.Module):
    def __init__(self, idim, hdim, odim, strides=(2, 2), n_bands=64):
        super().__init__()
        self.conv = nn.Sequential(Res2dModule(idim, hdim, (2, strides[0])), Res2dModule(hdim, hdim, (2, strides[1])))
        self.linear = nn.Linear(hdim * n_bands // 2 // 2, odim)

    def prepare(self):
        for m in self.conv:
            m.prepare()
        self._lin = PackedLinear(self.linear.weight, self.linear.bias, torch.float32)      # the stem is always exact fp32

    def run(self, x):
        """x [B, n_bands, T] fp32 -> rows [B * T', odim] fp32 (T' = T // 4 for the strides of the model), T'."""
        if x.dim() == 3:
            x = x.unsqueeze(1)
        x = x.contiguous()
        for m in self.conv:
            x = m.run(x)
        B, Cc, Fo, To = x.shape
        rows = x.permute(0, 3, 1, 2).reshape(B * To, Cc * Fo).contiguous()                  # "b c f t -> b t (c f)": data movement only
        return self._lin(rows), To


class Wav2Vec2ConformerFeedForward(nn.Module):
    def __init__(self, d, inter):
        super().__init__()
        self.intermediate_dense = nn.Linear(d, inter)
        self.output_dense = nn.Linear(inter, d)


class Wav2Vec2ConformerSelfAttention(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.num_heads, self.head_size = heads, d // heads
        self.linear_q = nn.Linear(d, d)
        self.linear_k = nn.Linear(d, d)
        self.linear_v = nn.Linear(d, d)
        self.linear_out = nn.Linear(d, d)


class Wav2Vec2ConformerConvolutionModule(nn.Module):
    def __init__(self, d, k):
        super().__init__()
        if (k - 1) % 2 == 1:
            raise ValueError("`config.conv_depthwise_kernel_size` should be a odd number for 'SAME' padding")
        self.layer_norm = nn.LayerNorm(d)
        self.pointwise_conv1 = nn.Conv1d(d, 2 * d, kernel_size=1, bias=False)
        self.depthwise_conv = nn.Conv1d(d, d, k, padding=(k - 1) // 2, groups=d, bias=False)
        self.batch_norm = nn.BatchNorm1d(d)
        self.pointwise_conv2 = nn.Conv1d(d, d, kernel_size=1, bias=False)


class Wav2Vec2ConformerEncoderLayer(nn.Module):
    def __init__(self, d, heads, inter, k, eps):
        super().__init__()
        self.d, self.heads = d, heads
        self.ffn1_layer_norm = nn.LayerNorm(d)
        self.ffn1 = Wav2Vec2ConformerFeedForward(d, inter)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.self_attn = Wav2Vec2ConformerSelfAttention(d, heads)
        self.conv_module = Wav2Vec2ConformerConvolutionModule(d, k)
        self.ffn2_layer_norm = nn.LayerNorm(d)
        self.ffn2 = Wav2Vec2ConformerFeedForward(d, inter)
        self.final_layer_norm = nn.LayerNorm(d)

    def prepare(self, dtype):
        d, a, c = self.d, self.self_attn, self.conv_module
        ln = lambda m: (_f32(m.weight), _f32(m.bias), float(m.eps))
        z = torch.zeros(d, d, dtype=torch.float32, device=a.linear_q.weight.device)
        wq, wk, wv = (_f32(m.weight) for m in (a.linear_q, a.linear_k, a.linear_v))
        # operand [rot | plain] of width 2 d: q and k read the rotated half, v the plain one
        w_qkv = torch.cat([torch.cat([wq, z], 1), torch.cat([wk, z], 1), torch.cat([z, wv], 1)], 0)
        b_qkv = torch.cat([_f32(a.linear_q.bias), _f32(a.linear_k.bias), _f32(a.linear_v.bias)], 0)
        pw1 = _f32(c.pointwise_conv1.weight).view(2 * d, d)
        dw_w, dw_b = fold_batchnorm(c.depthwise_conv.weight, None, c.batch_norm)
        ffn = lambda f: (PackedLinear(f.intermediate_dense.weight, f.intermediate_dense.bias, dtype),
                         PackedLinear(f.output_dense.weight, f.output_dense.bias, dtype, scale=0.5))     # x 0.5: exact, folded
        self._p = dict(dtype=dtype, ln_f1=ln(self.ffn1_layer_norm), ffn1=ffn(self.ffn1), ln_a=ln(self.self_attn_layer_norm),
                       qkv=PackedLinear(w_qkv, b_qkv, dtype), out=PackedLinear(a.linear_out.weight, a.linear_out.bias, dtype),
                       ln_c=ln(c.layer_norm), glu_x=PackedLinear(pw1[:d], None, dtype), glu_g=PackedLinear(pw1[d:], None, dtype),
                       dw_w=dw_w.view(d, -1).contiguous(), dw_b=dw_b, pw2=PackedLinear(_f32(c.pointwise_conv2.weight).view(d, d), None, dtype),
                       ln_f2=ln(self.ffn2_layer_norm), ffn2=ffn(self.ffn2), ln_o=ln(self.final_layer_norm))

    def _ffn(self, h, pair, norm):
        t = ops.ew_act(pair[0](h, norm=norm), EW_SILU)
        pair[1](t, epilogue=EPI_RESIDUAL, resid=h, y=h)

    def run(self, h, kv: DenseKV, cos, sin):
        """h [B * P, d] fp32 rows -> the layer's output rows (a new tensor)."""
        p, d = self._p, self.d
        B, P, M = kv.B, kv.T, h.shape[0]
        self._ffn(h, p["ffn1"], p["ln_f1"])
        xr = ops.layernorm_rope_rows(h, *p["ln_a"], cos, sin, kv.row_pos, d // self.heads)
        q = torch.empty(M, d, dtype=torch.float32, device=h.device)
        p["qkv"](xr, epilogue=EPI_QKV_ROPE, rope_mode=ROPE_NONE, row_pos=kv.row_pos, row_seq=kv.row_seq, q_out=q, kv=kv.geom)
        p["out"](kv.attend(q), epilogue=EPI_RESIDUAL, resid=h, y=h)
        g = p["glu_x"](h, epilogue=EPI_SWIGLU, w1=p["glu_g"], act_kind=GATE_SIGMOID_SECOND, norm=p["ln_c"])
        k = p["dw_w"].shape[1]
        c = ops.dwconv1d(g.view(B, P, d).transpose(1, 2).contiguous(), p["dw_w"], pad_left=(k - 1) // 2, Tout=P, bias=p["dw_b"])
        c = ops.ew_act(c, EW_SILU).transpose(1, 2).contiguous().view(M, d)                  # the two transposes are copies
        p["pw2"](c, epilogue=EPI_RESIDUAL, resid=h, y=h)
        self._ffn(h, p["ffn2"], p["ln_f2"])
        return ops.layernorm_rows(h, *p["ln_o"])


class Wav2Vec2ConformerEncoder(nn.Module):
    def __init__(self, cfg, n_layers):
        super().__init__()
        d = cfg["encoder_dim"]
        self.layers = nn.ModuleList([Wav2Vec2ConformerEncoderLayer(d, cfg["num_attention_heads"], cfg["intermediate_size"],
                                                                   cfg["conv_depthwise_kernel_size"], cfg["layer_norm_eps"]) for _ in range(n_layers)])


def rotary_tables(P, head_size, base):
    """(cos, sin) [P, head_size] fp32 on the host, as Wav2Vec2ConformerRotaryPositionalEmbedding builds them."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_size, 2, dtype=torch.int64).float() / head_size))
    freqs = torch.einsum("i,j->ij", torch.arange(P).type_as(inv_freq), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


class MusicFM25Hz(nn.Module):
    def __init__(self, config=None, taps=TAPS, **kw):
        super().__init__()
        cfg = dict(RELEASED_CONFIG)
        cfg.update(config or {})
        cfg.update(kw)
        self.config = {k: cfg[k] for k in RELEASED_CONFIG}
        self.taps = tuple(int(t) for t in taps)
        if not self.taps or min(self.taps) < 1 or max(self.taps) > cfg["encoder_depth"] or list(self.taps) != sorted(self.taps):
            raise ValueError(f"taps {self.taps}: ascending indices into hidden_states, 1 .. encoder_depth = {cfg['encoder_depth']}")
        d, heads = cfg["encoder_dim"], cfg["num_attention_heads"]
        if d % heads or (d // heads) % 2:
            raise ValueError(f"encoder_dim {d} must split into {heads} heads of even size")
        self.n_mels, self.d, self.heads = cfg["n_mels"], d, heads
        self.conv = Conv2dSubsampling(1, cfg["conv_dim"], d, strides=[2, 2], n_bands=self.n_mels)
        self.conformer = Wav2Vec2ConformerEncoder(cfg, max(self.taps))       # hidden_states[k] = input of layer k: layers 0 .. max - 1
        self._dtype = None
        self._kv, self._rot = None, None           # K/V pools and rotary tables of the LAST (B, P) only: P follows the clip length

    # ---- loading -----------------------------------------------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, path, config=None, taps=TAPS):
        """`path`: a torch file whose top level is a state dict or holds one under "model" / "state_dict" (the fairseq and the
        MusicFM layouts).  `model.` prefixes are stripped, the keys of parts that never run (UNUSED_PREFIXES, conformer layers past
        the last tap) are ignored; a parameter of this module tree that the file does not name is an error — never silently
        random weights.  The file is first read with weights_only=True; a file that needs the full unpickler must be trusted."""
        try:
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:           # a fairseq checkpoint pickles its `cfg` objects next to the tensors: only such a file needs the full
            ck = torch.load(path, map_location="cpu", weights_only=False)       # unpickler, which runs code from the file — trusted files only
        for key in ("model", "state_dict"):
            if isinstance(ck, dict) and key in ck and isinstance(ck[key], dict):
                ck = ck[key]
                break
        model = cls(config, taps=taps)
        mine = model.state_dict()
        own, unknown = {}, []
        for k, v in ck.items():
            while k.startswith("model."):
                k = k[len("model."):]
            if k in mine:
                own[k] = v
            elif not (k.startswith(UNUSED_PREFIXES) or k.startswith("conformer.layers.")):
                unknown.append(k)
        missing = sorted(set(mine) - set(own))
        if missing:
            raise RuntimeError(f"{path}: {len(missing)} parameter(s) of the BEST-RQ encoder are not in the checkpoint (first: {missing[:5]}; "
                               f"unrecognised keys in the file: {unknown[:5]}) — a key-name mismatch between this module tree and the checkpoint")
        model.load_state_dict(own, strict=True)
        return model

    # ---- plan --------------------------------------------------------------------------------------------------
    def prepare(self, dtype=torch.float32):
        if self.conv.linear.weight.device.type != "cuda":
            raise RuntimeError("uniaudio2_amd runs on a ROCm device only (no CPU fallback); move the model to cuda")
        self.eval()
        self.conv.prepare()
        for l in self.conformer.layers:
            l.prepare(dtype)
        self._dtype = dtype
        self._kv, self._rot = None, None
        return self

    def preprocess(self, wav):
        """wav [B, N] fp32 at 24 kHz -> normalised mel [B, n_mels, 4 (N // 960)] (preprocessing + normalize, :199-233)."""
        return ops.melspec(wav.float().contiguous(), self.n_mels)

    def stem(self, mel):
        return self.conv.run(mel.float())

    @torch.inference_mode()
    def encode(self, mel):
        """mel [B, n_mels, T] fp32 on the device -> tuple of [B, T // 4, encoder_dim] fp32, one per tap."""
        if self._dtype is None:
            self.prepare()
        B = mel.shape[0]
        h, P = self.stem(mel)
        if self._kv is None or (self._kv.B, self._kv.T) != (B, P):
            self._kv = DenseKV(B, P, self.heads, self.d // self.heads, self._dtype, h.device)
        if self._rot is None or self._rot[0].shape[0] != P:
            self._rot = tuple(t.to(h.device) for t in rotary_tables(P, self.d // self.heads, self.config["rotary_embedding_base"]))
        kv, rot = self._kv, self._rot
        out = []
        for i, l in enumerate(self.conformer.layers):
            h = l.run(h, kv, *rot)
            if i + 1 in self.taps:
                out.append(h.view(B, P, self.d).clone())
        return tuple(out)

    def forward(self, wav):
        """wav [B, N] or [B, 1, N] fp32 at 24 kHz -> the taps, each [B, N // 960, encoder_dim]."""
        if wav.dim() == 3:
            wav = wav[:, 0]
        return self.encode(self.preprocess(wav))
