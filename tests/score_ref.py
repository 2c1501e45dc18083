"""The teacher-forced pass (llm_models/model_new.py:402-454 forward) restated over oracle.lm_oracle (test infrastructure, not product
code): Stage3Oracle._trunk over the whole sequence, lm_head, and its depth decoder GPTOracle over the eight codebook positions of
every row, fed with h_final and the embeddings of the LABELS (:447-453).  The oracle's arithmetic mode decides the contract — "fp32":
the reference as shipped; "bf16": the product's reduced-precision contract in the decode frame's scaled form, which the product's
scoring pass runs (its chunks are launched as decode frames are) — and the cross-entropies are taken in float64 from those logits
(`xent64`), so a comparison sees the logits' error only.

`teacher_forced` returns every row's logits (the product scores every row and masks on the host); `forward_outputs` cuts them into
the reference's 4-tuple; `reference_metrics` restates :59-109 in float64 on given logits."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.lm_oracle import GPTOracle, norm_linear


@torch.inference_mode()
def teacher_forced(oracle, tokens, labels, tokens_mask, scaled=True):
    """tokens (B, S, 9) long, labels (B, S, 8) long, tokens_mask (B, >= S + 1, 9) bool.  Returns text_logits (B, S, Vt) and
    audio_logits (B, S, 8, Va) of EVERY row, float32 tensors."""
    B, S, W = tokens.shape
    ncb = W - 1
    pos = torch.arange(S).unsqueeze(0).expand(B, S)
    oracle.setup_caches(B)
    h_final = oracle._trunk(tokens, tokens_mask[:, :S].bool(), pos, None, scaled=scaled)                 # :421-444
    text_logits = F.linear(oracle.qa(h_final), oracle.lm_head)                                            # :445
    off = oracle.va * torch.arange(ncb - 1)
    local = oracle.audio_embeddings[labels[:, :, :-1] + off]                                              # :447 _embed_local_audio
    curr_h = torch.cat([h_final.unsqueeze(2), local], dim=2).reshape(B * S, ncb, -1)                      # :448
    d_in = F.linear(oracle.qa(curr_h), oracle.projection)                                                 # :452
    dec = oracle.decoder
    fresh = GPTOracle.__new__(GPTOracle)                                                                  # the decoder with a cache of B * S sequences
    fresh.__dict__.update(dec.__dict__)
    fresh.set_kv_cache(B * S)
    dpos = torch.arange(ncb).unsqueeze(0).expand(B * S, ncb)
    d_x = fresh.forward(d_in, dpos, None, final_norm=False, scaled=scaled)
    logits = [norm_linear(d_x[:, i], dec.ln_f, dec.s.norm_eps, [oracle.audio_head[i].t()], oracle.mode, scaled)[0] for i in range(ncb)]
    return text_logits, torch.stack(logits, dim=1).view(B, S, ncb, -1)                                    # :453


def forward_outputs(text_logits, audio_logits, labels, tokens_mask, loss_mask):
    """The reference's 4-tuple (:449-454): rows selected by tokens_mask[:, 1:, 0] in its row order."""
    S = text_logits.shape[1]
    sel = tokens_mask[:, 1:S + 1, 0].bool()
    return text_logits, audio_logits[sel], labels[sel], loss_mask[:, 1:S + 1, :][sel]


def xent64(logits, labels):
    """float64 lse - logit[label] per row of (..., V) logits; 0 where label == -1.  numpy arrays or tensors in, numpy out."""
    x = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels).astype(np.int64)
    mx = x.max(axis=-1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(axis=-1)) + mx[..., 0]
    tgt = np.take_along_axis(x, np.clip(y, 0, None)[..., None], axis=-1)[..., 0]
    return np.where(y < 0, 0.0, lse - tgt)


def reference_metrics(text_logits, text_labels, text_mask, ci_logits, choosed_label, choosed_mask, n_weights):
    """model_new.py:59-109 in float64 from given logits: the dict with acc_text, loss_text, acc_i, loss_i (i = 1 .. n_weights)."""
    nll_t = xent64(text_logits, text_labels)
    tm = np.asarray(text_mask).astype(bool)
    nt = tm.sum()
    out = {"acc_text": float(((np.asarray(text_logits).argmax(-1) == np.asarray(text_labels)) & tm).sum() / nt),
           "loss_text": float((nll_t * tm).sum() / nt)}
    ci, y, cm = np.asarray(ci_logits), np.asarray(choosed_label), np.asarray(choosed_mask)
    N = y.shape[0]
    for i in range(n_weights):
        out[f"acc_{i + 1}"] = float((ci[:, i].argmax(-1) == y[:, i]).sum() / N)
        out[f"loss_{i + 1}"] = float((xent64(ci[:, i], y[:, i]) * cm[:, i]).sum() / N)
    return out


# ---- inputs and host restatements of the cross-entropy tail's parity test (include/ua2hip.h ua2_xent_embed) ------------------------
XENT_SHAPES = [(1, 1), (37, 37), (110, 110), (500, 512), (4099, 4099), (128256, 128256)]     # (V, ld)
XENT_ROWS = (1, 5, 67)


def xent_rows(V, ld, M, seed=0):
    """logits (M, ld) float32 ~ N(0, 4) (columns >= V hold a large value the kernel must never read into its result) and labels (M,)
    int32.  Row m % 10 decides the special content, so M = 5 holds the first five kinds and M = 67 all of them several times:
      0 shifted by +1e4, 1 shifted by -1e4 (the maximum subtraction), 2 a tie at the maximum (lowest index wins), 3 -inf everywhere
      but one entry, 4 a -inf target, 5 all -inf, 6 a NaN in the row, 7 label -1, 8 label 0, 9 label V - 1."""
    g = np.random.default_rng(seed + 7919 * V + M)
    x = (2.0 * g.standard_normal((M, ld))).astype(np.float32)
    y = g.integers(0, V, size=M).astype(np.int32)
    x[:, V:] = 3.0e4
    for m in range(M):
        kind, r = m % 10, x[m, :V]
        if kind == 0:
            r += np.float32(1e4)
        elif kind == 1:
            r -= np.float32(1e4)
        elif kind == 2 and V >= 2:
            a, b = sorted(g.choice(V, size=2, replace=False))
            r[a] = r[b] = np.float32(r.max() + 1.0)
        elif kind == 3:
            keep = int(g.integers(0, V))
            v = r[keep]
            r[:] = -np.inf
            r[keep] = v
            y[m] = keep
        elif kind == 4:
            r[y[m]] = -np.inf
        elif kind == 5:
            r[:] = -np.inf
        elif kind == 6:
            r[int(g.integers(0, V))] = np.nan
        elif kind == 7:
            y[m] = -1
        elif kind == 8:
            y[m] = 0
        elif kind == 9:
            y[m] = V - 1
    return x, y


def xent32(x, y):
    """The kernel's formula in float32 numpy: log(sum(exp(x - max))) - (x[label] - max), every operation rounded to fp32; numpy's
    own (pairwise) summation order.  x (M, V) float32, y (M,) -> (M,) float32."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float32)
        mx = x.max(axis=-1, keepdims=True)
        s = np.exp(x - mx, dtype=np.float32).sum(axis=-1, dtype=np.float32)
        tgt = np.take_along_axis(x, np.clip(y, 0, None).astype(np.int64)[:, None], axis=-1)[:, 0]
        return np.where(y < 0, np.float32(0), np.log(s, dtype=np.float32) - (tgt - mx[:, 0])).astype(np.float32)


def xent64_stable(x, y):
    """float64 reference of the same rows, NaN / inf as F.cross_entropy gives them."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        mx = np.nanmax(np.where(np.isnan(x), -np.inf, x), axis=-1, keepdims=True)
        s = np.exp(x - mx).sum(axis=-1)
        tgt = np.take_along_axis(x, np.clip(y, 0, None).astype(np.int64)[:, None], axis=-1)[:, 0]
        return np.where(y < 0, 0.0, np.log(s) - (tgt - mx[:, 0]))
