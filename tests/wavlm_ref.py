"""WavLM encoder: an own restatement in plain torch (fp32 or float64, any device) of what transformers' `WavLMModel` computes for the
codec's call (feat_extract_norm "group", post-norm layers, gated relative-position bias, no attention mask), the toy config, seeded
weights under transformers' state-dict names and seeded clips.  tests/golden/make_golden_wavlm.py pins it on transformers itself
(wavlm_toy.json: gap_front_fp32, gap_enc_fp32); the GPU tests use it in float64 as the reference of the single kernels.

Test data plumbing, not product code."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from weights import seeded_tensor

TOY = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=3, conv_dim=(32, 32, 32), conv_kernel=(10, 3, 2),
           conv_stride=(5, 2, 2), conv_bias=False, feat_extract_norm="group", do_stable_layer_norm=False, num_conv_pos_embeddings=16,
           num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=40, layer_norm_eps=1e-5, feat_extract_activation="gelu",
           hidden_act="gelu")
TAPS = (1, 2, 3)
CASES = {"a": 4000, "b": 1365}            # samples per clip: 199 and 67 frames (the log-spaced and the saturated buckets are reached)
BATCH = 2
BIAS_T = (50, 130)                        # position_bias goldens at the released 320 buckets / 800 distance


def clips(name):
    """[BATCH, N] fp32 seeded clips."""
    n = CASES[name]
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    rows = []
    for b in range(BATCH):
        noise = seeded_tensor((n,), 6100 + 10 * sorted(CASES).index(name) + b, std=0.1)
        rows.append(0.3 * torch.sin(2 * math.pi * (220.0 + 90.0 * b) * t) + noise)
    return torch.stack(rows)


def shapes(cfg, n_layers=None):
    """Ordered {transformers key: shape} of a WavLMModel of `cfg` with its first n_layers layers (masked_spec_embed left out)."""
    d, H, ff = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"]
    n_layers = cfg["num_hidden_layers"] if n_layers is None else n_layers
    s = OrderedDict()
    dims = (1,) + tuple(cfg["conv_dim"])
    for i, (k, _) in enumerate(zip(cfg["conv_kernel"], cfg["conv_stride"])):
        s[f"feature_extractor.conv_layers.{i}.conv.weight"] = (dims[i + 1], dims[i], k)
        if i == 0:
            s["feature_extractor.conv_layers.0.layer_norm.weight"] = (dims[1],)
            s["feature_extractor.conv_layers.0.layer_norm.bias"] = (dims[1],)
    s["feature_projection.layer_norm.weight"] = (dims[-1],)
    s["feature_projection.layer_norm.bias"] = (dims[-1],)
    s["feature_projection.projection.weight"] = (d, dims[-1])
    s["feature_projection.projection.bias"] = (d,)
    K, g = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    s["encoder.pos_conv_embed.conv.bias"] = (d,)
    s["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, K)
    s["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (d, d // g, K)
    s["encoder.layer_norm.weight"] = (d,)
    s["encoder.layer_norm.bias"] = (d,)
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[p + f"attention.{n}.weight"] = (d, d)
            s[p + f"attention.{n}.bias"] = (d,)
        s[p + "attention.gru_rel_pos_const"] = (1, H, 1, 1)
        s[p + "attention.gru_rel_pos_linear.weight"] = (8, d // H)
        s[p + "attention.gru_rel_pos_linear.bias"] = (8,)
        if i == 0:
            s[p + "attention.rel_attn_embed.weight"] = (cfg["num_buckets"], H)
        s[p + "layer_norm.weight"] = (d,)
        s[p + "layer_norm.bias"] = (d,)
        s[p + "feed_forward.intermediate_dense.weight"] = (ff, d)
        s[p + "feed_forward.intermediate_dense.bias"] = (ff,)
        s[p + "feed_forward.output_dense.weight"] = (d, ff)
        s[p + "feed_forward.output_dense.bias"] = (d,)
        s[p + "final_layer_norm.weight"] = (d,)
        s[p + "final_layer_norm.bias"] = (d,)
    return s


def state_dict(cfg, seed=6000, n_layers=None):
    """Seeded weights that make every term matter: fan-in scaled matrices, gains around 1, a relative-position table and gate
    projections of order 1 (so gate * table moves the softmax)."""
    out = OrderedDict()
    for i, (k, shp) in enumerate(shapes(cfg, n_layers).items()):
        t = seeded_tensor(shp, seed * 100003 + i, std=1.0)
        if k.endswith("rel_attn_embed.weight"):
            t = 1.5 * t
        elif k.endswith("gru_rel_pos_const"):
            t = 1.0 + 0.5 * t
        elif k.endswith("original0"):
            t = 1.0 + 0.3 * t.abs()
        elif k.endswith("gru_rel_pos_linear.weight"):
            t = 0.5 * t
        elif "layer_norm" in k and k.endswith("weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith("bias"):
            t = 0.1 * t
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            t = t / max(fan_in, 1) ** 0.5
        out[k] = t
    return out


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def conv0_ref(x, w, gn_w, gn_b, stride, eps=1e-5):
    """x [B, N], w [C, K] -> [B, T0, C]: conv, per-(clip, channel) normalisation over time (biased variance), affine, GELU."""
    y = F.conv1d(x[:, None, :], w[:, None, :], stride=stride)                       # [B, C, T0]
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    y = (y - mu) / torch.sqrt(var + eps) * gn_w[None, :, None] + gn_b[None, :, None]
    return gelu(y).transpose(1, 2)


def frontend_ref(sd, cfg, wav, dtype=torch.float32):
    """wav [B, N] -> feature-extractor output [B, T, conv_dim[-1]] (transformers' extract_features before the projection's LayerNorm)."""
    sd = _cast(sd, dtype)
    p = "feature_extractor.conv_layers."
    y = conv0_ref(wav.to(dtype), sd[p + "0.conv.weight"][:, 0, :], sd[p + "0.layer_norm.weight"], sd[p + "0.layer_norm.bias"], cfg["conv_stride"][0])
    y = y.transpose(1, 2)
    for i in range(1, len(cfg["conv_dim"])):
        y = gelu(F.conv1d(y, sd[p + f"{i}.conv.weight"], stride=cfg["conv_stride"][i]))
    return y.transpose(1, 2)


def pos_weight(sd):
    """weight norm (dim 2) of the positional conv folded: g * v / ||v|| with the norm over (out, in) per tap."""
    g, v = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"], sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
    return g * v / torch.sqrt((v * v).sum((0, 1), keepdim=True))


def grouped_conv_ref(x, w, bias, groups, act, resid):
    """x [B, T, C], w [C, C / groups, K] -> resid + act(conv(x, padding K // 2)[..., :T] + bias)."""
    K, T = w.shape[-1], x.shape[1]
    y = F.conv1d(x.transpose(1, 2), w, bias, padding=K // 2, groups=groups)[:, :, :T].transpose(1, 2)
    y = gelu(y) if act else y
    return y + resid if resid is not None else y


def pos_conv_ref(sd, cfg, h):
    return grouped_conv_ref(h, pos_weight(sd), sd["encoder.pos_conv_embed.conv.bias"], cfg["num_conv_pos_embedding_groups"], True, h)


def gate_ref(h, w, b, c, n_head):
    """h [R, n_head * hs], w [8, hs], b [8], c [n_head] -> [R, n_head]."""
    R = h.shape[0]
    p = h.view(R, n_head, -1) @ w.t() + b                                            # [R, H, 8]
    s = torch.sigmoid(p.view(R, n_head, 2, 4).sum(-1))
    return s[..., 0] * (s[..., 1] * c[None, :] - 1.0) + 2.0


def buckets(rel, num_buckets, max_distance):
    """The bidirectional bucket rule (relative position = key - query): sign picks the half, |d| < num_buckets / 4 is its own bucket,
    larger distances are log-spaced up to max_distance and saturate in the last bucket of the half.  The logarithm is taken in
    fp32 and divided by a Python float, as transformers does, so the boundaries agree."""
    nb = num_buckets // 2
    exact = nb // 2
    a = rel.abs()
    big = torch.log(a.float() / exact) / math.log(max_distance / exact) * (nb - exact)
    big = torch.clamp((exact + big).to(torch.long), max=nb - 1)
    return torch.where(rel > 0, nb, 0) + torch.where(a < exact, a, big)


def bias_table(embed, T, num_buckets, max_distance):
    """embed [num_buckets, H] -> position_bias [H, T, T]: [h][q][k] = embed[bucket(k - q)][h]."""
    pos = torch.arange(T)
    return embed[buckets(pos[None, :] - pos[:, None], num_buckets, max_distance)].permute(2, 0, 1)


def attn_ref(q, k, v, gate, bias, n_keys=None):
    """q [B, H, Tq, hs] (pre-scaled), k, v [B, H, Tk, hs], gate [B, H, Tq], bias [H, Tq, Tk] -> [B, H, Tq, hs]; n_keys: keys 0 .. n_keys - 1 only."""
    s = q @ k.transpose(-1, -2) + gate[..., None] * bias[None]
    if n_keys is not None:
        s = s[..., :n_keys]
        v = v[:, :, :n_keys]
    return torch.softmax(s, -1) @ v


def encoder_ref(sd, cfg, wav, dtype=torch.float32, n_layers=None):
    """wav [B, N] -> (front [B, T, C], [hidden_states[0 .. n_layers]] each [B, T, d])."""
    front = frontend_ref(sd, cfg, wav, dtype)
    sd = _cast(sd, dtype)
    eps, H, d = cfg["layer_norm_eps"], cfg["num_attention_heads"], cfg["hidden_size"]
    hs = d // H
    h = _ln(front, sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"], eps)
    h = h @ sd["feature_projection.projection.weight"].t() + sd["feature_projection.projection.bias"]
    h = pos_conv_ref(sd, cfg, h)
    h = _ln(h, sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], eps)
    B, T, _ = h.shape
    out = [h]
    n_layers = cfg["num_hidden_layers"] if n_layers is None else n_layers
    bias = bias_table(sd["encoder.layers.0.attention.rel_attn_embed.weight"], T, cfg["num_buckets"], cfg["max_bucket_distance"]) if n_layers else None
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        lin = lambda x, n: x @ sd[p + n + ".weight"].t() + sd[p + n + ".bias"]
        heads = lambda x: x.view(B, T, H, hs).transpose(1, 2)
        gate = gate_ref(h.reshape(B * T, d), sd[p + "attention.gru_rel_pos_linear.weight"], sd[p + "attention.gru_rel_pos_linear.bias"],
                        sd[p + "attention.gru_rel_pos_const"].view(-1), H).view(B, T, H).transpose(1, 2)
        q = heads(lin(h, "attention.q_proj")) * hs ** -0.5
        o = attn_ref(q, heads(lin(h, "attention.k_proj")), heads(lin(h, "attention.v_proj")), gate, bias)
        o = lin(o.transpose(1, 2).reshape(B, T, d), "attention.out_proj")
        h = _ln(h + o, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], eps)
        f = lin(gelu(lin(h, "feed_forward.intermediate_dense")), "feed_forward.output_dense")
        h = _ln(h + f, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], eps)
        out.append(h)
    return front, out


def tap_mean(hidden, taps=TAPS):
    acc = hidden[taps[0]]
    for t in taps[1:]:
        acc = acc + hidden[t]
    return acc * (1.0 / len(taps))


# ---- inputs of the single-kernel tests (shared with the golden generator, which measures the restatement's own fp32 error on them) ----
GATE_CASES = [(37, 2, 64), (5, 12, 64)]
ATTN_CASES = [(2, 2, 64, 50), (1, 12, 64, 130), (1, 2, 64, 64), (1, 2, 64, 1), (1, 2, 128, 70)]     # (B, H, hs, T)


def gate_case(R, H, hs, seed=6400):
    return (seeded_tensor((R, H * hs), seed, std=1.0), seeded_tensor((8, hs), seed + 1, std=1.0) / hs ** 0.5, seeded_tensor((8,), seed + 2, std=0.3),
            1.0 + 0.5 * seeded_tensor((H,), seed + 3, std=1.0))


def attn_case(B, H, hs, T, seed=6500):
    """q (pre-scaled by hs^-0.5), k, v [B, H, T, hs]; gate [B, H, T] in (1, 2.5); embed [320, H] of order 1 (gate * table of order 1)."""
    q = seeded_tensor((B, H, T, hs), seed, std=1.0) * hs ** -0.5
    k, v = seeded_tensor((B, H, T, hs), seed + 1, std=1.0), seeded_tensor((B, H, T, hs), seed + 2, std=1.0)
    gate = 1.0 + 1.5 * torch.sigmoid(seeded_tensor((B, H, T), seed + 3, std=1.0))
    embed = seeded_tensor((320, H), seed + 4, std=1.0)
    return q, k, v, gate, embed
