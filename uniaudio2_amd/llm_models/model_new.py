"""Audio-text LM of the decode loop, host side.

Mirror of the reference's llm_models/model_new.py `Model_stage3` (:334-687) for its inference
methods: `setup_caches` (:554-565), `reset_caches` (:647-651), `forward_prefix` (:456-507),
`generate_frame` (:568-645) and the teacher-forced `forward` (:402-454, with the cross-entropy helpers of :59-109; `score` is
the on-device form) keep their signatures, the state-dict keys are identical
(`backbone.*`, `decoder.*`, `audio_understanding_expert.*`, `audio_generation_expert.*`,
`audio_embeddings.weight`, `projection.weight`, `audio_head`), so a reference checkpoint loads
with `load_state_dict`.

All arithmetic runs in libua2hip.so through the frame executor (include/ua2hip.h
ua2_stage3_*): one C call per prefill chunk / per frame, hipGraph replay for the frame.
`generate_frames` is the MI355X-native fast path the generators use: N frames back to back
with the sample -> next-input feedback, forbid_prefix switch and frame log all on device.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import BeamNgram, BeamPool, BeamState, Stage3Desc, W8Entry, check, lib, vp
from .config import Config as gpt_config
from .lit_model import GPT


@dataclass
class ModelArgs:
    llm_name: str
    decoder_name: str
    llm_pretrained_model: str
    audio_embeddings_path: str
    audio_understanding_expert_path: str
    audio_semantic_vocab_size: int
    audio_reason_vocab_size: int
    audio_num_codebooks: int


_UNSET = object()      # "argument left out" where None is a meaningful value


def backtrack_beam_log(log, slot):
    """log [steps, W, 4] (parent, text id or -1, score bits, fin) as ua2_beam_step writes it: the text ids of the hypothesis that
    ends in `slot` — the device never permutes histories, the host walks the parents back."""
    ids, j = [], int(slot)
    for t in range(len(log) - 1, -1, -1):
        parent, tok = int(log[t][j][0]), int(log[t][j][1])
        if tok >= 0:
            ids.append(tok)
        j = parent
    return ids[::-1]


# The plan an admitting session follows, worked out ahead for fixed frame counts.  Nothing in the package plans ahead (admitting_session
# decides after every chunk): the two functions are the reference the host tests hold the running loop to.
def ragged_schedule(n_frames):
    """Continuous-batching plan for fixed per-sequence frame counts: yields (step, active, keep) — run `step` frames with
    the sequences `active` (original indices, in row order), then keep the rows at positions `keep` (in order) as rows
    0..len(keep)-1.  Every sequence runs exactly n_frames[b] frames; a sequence leaves the batch the frame it finishes."""
    active = list(range(len(n_frames)))
    t_now = 0
    while active:
        step = min(int(n_frames[b]) for b in active) - t_now
        t_now += step
        keep = [r for r, b in enumerate(active) if int(n_frames[b]) > t_now]
        yield step, list(active), keep
        active = [active[r] for r in keep]


def admission_schedule(n_frames, batch_size=None):
    """ragged_schedule with admission: at most `batch_size` sequences are live (None: all of them, which is ragged_schedule);
    the first batch_size start together and a waiting sequence is admitted, in input order, at the first chunk boundary at which
    a row is free.  Yields (step, active, keep, admit): run `step` frames with the sequences `active` (original indices, in row
    order), keep the rows at positions `keep` as rows 0..len(keep)-1, then append the sequences `admit` as the rows behind them.
    The first step's `active` is the set to start with.  Every sequence runs exactly n_frames[b] frames from its admission."""
    N = len(n_frames)
    cap = N if batch_size is None else int(batch_size)
    if cap < 1 and N:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    waiting = list(range(N))
    active, waiting = waiting[:cap], waiting[cap:]
    end = {b: int(n_frames[b]) for b in active}          # the frame count of the session at which sequence b finishes
    t_now = 0
    while active:
        step = min(end[b] for b in active) - t_now
        t_now += step
        keep = [r for r, b in enumerate(active) if end[b] > t_now]
        free = cap - len(keep)
        admit, waiting = waiting[:free], waiting[free:]
        yield step, list(active), keep, admit
        active = [active[r] for r in keep] + admit
        for b in admit:
            end[b] = t_now + int(n_frames[b])


def _seed_words(seed):
    """A 64-bit seed as the (lo, hi) int32 pair of row_key."""
    seed = int(seed) & (2 ** 64 - 1)
    s32 = lambda x: x - (1 << 32) if x >= (1 << 31) else x
    return [s32(seed & 0xFFFFFFFF), s32(seed >> 32)]


def admitting_session(model, *, rows_of, n_utt, cap, limit, chunk, seeds, run, take, start=None):
    """The loop of every batched generation (continuous batching with admission): at most `cap` of the `n_utt` utterances are live;
    the first `cap` start together (begin_ragged) and a waiting one is admitted, in input order, at the first chunk boundary at
    which a slot is free (admit_rows).  rows_of(b): the prompt rows of utterance b — one, or the (conditional, unconditional) pair;
    an utterance's rows stay adjacent, survivors keep their order and the admitted follow them.  Utterance b runs at most limit[b]
    frames from its own admission, in chunks of min(chunk, the least budget left among the live); run(n, rows) runs one chunk and
    returns its log slice (n, rows, 9), copied out of the frame log; take(b, log_of_b) consumes the utterance's own rows of it and
    returns True once b is finished.  An utterance leaves when `take` says so or when its budget is spent; retire_rows is called
    only when somebody leaves.  seeds (or None): utterance b draws under seeds[b] on each of its rows (set_row_seeds, off again
    when the session ends, also by an exception).  start(): whatever the caller sets up between begin_ragged and the row seeds.
    The session may run more frames than log_frames: the log slot is rewound once the slices before it have been copied out.
    The loop itself never synchronises with the device."""
    if n_utt == 0:
        return
    if cap < 1:
        raise ValueError(f"batch_size must be >= 1, got {cap}")
    active, waiting = list(range(n_utt))[:cap], list(range(n_utt))[cap:]     # live utterances in row order; the queue
    first = [p for b in active for p in rows_of(b)]
    per = len(first) // len(active)
    keys_of = lambda seq: None if seeds is None else [seeds[b] for b in seq for _ in range(per)]
    model.begin_ragged(first)
    ran = [0] * n_utt                                      # frames run per utterance
    used, log_frames = 0, model._st["log_frames"]          # log slots taken since the last rewind (begin_ragged starts at 0)
    try:
        if start is not None:
            start()
        if seeds is not None:
            model.set_row_seeds(keys_of(active))
        while active:
            n = min(chunk, min(limit[b] - ran[b] for b in active))
            if n:                                          # (0: utterances of no frames at all, which only leave)
                if used + n > log_frames:
                    model.rewind_frame_log()               # every earlier slice has been copied out
                    used = 0
                log = run(n, per * len(active))
                used += n
            keep = []
            for r, b in enumerate(active):
                ran[b] += n
                done = bool(n) and take(b, log[:, per * r:per * (r + 1)])
                if not done and ran[b] < limit[b]:
                    keep.append(r)
            if len(keep) < len(active):
                model.retire_rows([per * r + j for r in keep for j in range(per)], per * len(active))
                active = [active[r] for r in keep]
            admit, waiting = waiting[:cap - len(active)], waiting[cap - len(active):]
            if admit:
                model.admit_rows([p for b in admit for p in rows_of(b)], per * len(active), seeds=keys_of(admit))
                active += admit
    finally:
        if seeds is not None:
            model.set_row_seeds(None)


DEFER_CAP_ROWS = 64     # include/ua2hip.h UA2_DEFER_CAP_ROWS: rows of the executor's stash ring


def defer_windows(start: int, n_frames: int, R: int, cap_rows: int = DEFER_CAP_ROWS):
    """Flush windows of a generate_frames call that defers its text head: the call's frames are log slots start .. start +
    n_frames - 1, every frame but the last is deferred, and a deferred frame f of R rows sits in slot f % cap_frames of the
    executor's stash ring (cap_frames = cap_rows // R).  Returns [(frame0, n), ...] in issue order: window (frame0, n) is
    flushed right after frame frame0 + n - 1.  The windows tile the deferred frames, none crosses a multiple of cap_frames
    (so none wraps the ring, and a slot is flushed before it is written again) and none holds more than cap_rows rows."""
    cap_frames = cap_rows // R
    if cap_frames < 1:
        raise ValueError(f"a stash ring of {cap_rows} rows holds no frame of {R} rows")
    out, f, end = [], start, start + n_frames - 1          # deferred frames: [start, end)
    while f < end:
        stop = min(end, (f // cap_frames + 1) * cap_frames)
        out.append((f, stop - f))
        f = stop
    return out


def CrossEntropyAndAccuracy_text(logits, y, mask, ignore_id=-1):
    """model_new.py:59-73.  logits (B, T, K), y (B, T), mask (B, T).  Returns (loss, {'acc_text', 'loss_text'}): the per-token
    cross-entropy (0 where y == ignore_id) and the hits of the arg-max, both summed under `mask` and divided by mask.sum() — a token
    that is ignored but not masked still counts in the divisor, as in the reference."""
    y, mask = y.to(logits.device), mask.to(logits.device)
    K = logits.shape[-1]
    nll = F.cross_entropy(logits.reshape(-1, K), y.reshape(-1), ignore_index=ignore_id, reduction="none").view(y.shape)
    n = mask.int().sum()
    hit = (logits.argmax(-1) == y) & mask.bool()
    loss = (nll * mask).sum() / n
    return loss, {"acc_text": hit.int().sum() / n, "loss_text": loss.clone().detach()}


def CrossEntropyAndAccuracy_residual(logits, y, loss_mask, loss_weights=[1, 1, 1], ignore_id=None):
    """model_new.py:75-109.  logits (N, n_cb, K), y (N, n_cb), loss_mask (N, >= n_cb) over the N selected audio steps; one codebook
    per entry of `loss_weights` (the default scores the first three).  Returns (weighted mean loss, {'acc_i', 'loss_i'}, i from 1).
    The reference's quirks are kept: the accuracy ignores loss_mask, and both it and the loss divide by N, not by the unmasked count.
    ignore_id None = no label is ignored (F.cross_entropy's own default id, -100, which no label takes)."""
    y = y.to(logits.device)
    ignore = -100 if ignore_id is None else int(ignore_id)
    N = y.shape[0]
    acc, losses, total = {}, {}, 0
    for i, w in enumerate(loss_weights):
        li, yi = logits[:, i, :], y[:, i]
        nll = F.cross_entropy(li, yi, ignore_index=ignore, reduction="none") * loss_mask[:, i]
        acc[f"acc_{i + 1}"] = (li.argmax(1) == yi).int().sum() / N
        loss_i = nll.sum() / N
        total = total + loss_i * w
        losses[f"loss_{i + 1}"] = loss_i.clone().detach()
    return total / len(loss_weights), {**acc, **losses}


def score_stats(nll, pred, lab, step_mask, loss_mask):
    """Sufficient statistics of the two reference cross-entropy functions over scored rows, float64 on the tensors' device.  nll, pred,
    lab (..., W) in the token layout (audio streams first, text last), step_mask / loss_mask (..., W) bool: the masks of the steps
    the rows predict (tokens_mask[:, 1:], loss_mask[:, 1:]).  Per stream: sum_nll (under the loss mask), hits (audio: over every
    selected row, loss mask ignored — the reference's quirk; text: under the mask), rows (the divisor: audio steps selected by
    step_mask[..., 0]; text: step_mask & loss_mask of the text stream) and n_tokens (labels that contribute a loss)."""
    W = nll.shape[-1]
    n64, hit = nll.double().reshape(-1, W), (pred == lab).reshape(-1, W)
    tm, lm, lab = step_mask.reshape(-1, W).bool(), loss_mask.reshape(-1, W).bool(), lab.reshape(-1, W)
    sel = tm[:, :1].expand(-1, W - 1)
    counted = torch.cat([sel & lm[:, :-1], tm[:, -1:] & lm[:, -1:]], dim=1)            # rows whose loss enters the sum
    hits_in = torch.cat([sel, counted[:, -1:]], dim=1)
    rows = torch.cat([sel, counted[:, -1:]], dim=1).sum(0).double()
    return {"sum_nll": (n64 * counted).sum(0), "hits": (hit & hits_in).sum(0).double(), "rows": rows,
            "n_tokens": (counted & (lab >= 0)).sum(0).double()}


def metrics_from_stats(stats, n_weights=None):
    """The metric keys of CrossEntropyAndAccuracy_text / _residual (model_new.py:59-109) from score_stats (summed over any number
    of sequences): acc_text, loss_text, acc_i, loss_i for the first n_weights codebooks (None: all), i from 1."""
    W = stats["rows"].shape[0]
    acc, loss = stats["hits"] / stats["rows"], stats["sum_nll"] / stats["rows"]
    out = {"acc_text": acc[-1], "loss_text": loss[-1]}
    for i in range(W - 1 if n_weights is None else n_weights):
        out[f"acc_{i + 1}"] = acc[i]
    for i in range(W - 1 if n_weights is None else n_weights):
        out[f"loss_{i + 1}"] = loss[i]
    return out


class Model_stage3(nn.Module):
    """Stage 3: text-audio joint model (inference)."""

    def __init__(self, config: ModelArgs, device=None):
        super().__init__()
        self.config = config
        self.backbone = GPT(gpt_config.from_name(config.llm_name), device=device)
        backbone_dim = self.backbone.config.n_embd
        self.decoder = GPT(gpt_config.from_name(config.decoder_name), device=device, with_embeddings=False)
        decoder_dim = self.decoder.config.n_embd
        va = config.audio_semantic_vocab_size + config.audio_reason_vocab_size
        self.audio_embeddings = nn.Embedding(va * config.audio_num_codebooks, backbone_dim, device=device)
        self.projection = nn.Linear(backbone_dim, decoder_dim, bias=False, device=device)
        self.audio_head = nn.Parameter(torch.empty(config.audio_num_codebooks, decoder_dim, va, device=device))
        self.audio_understanding_expert = GPT(gpt_config.from_name("meta-llama/Llama-3.2-Understanding"),
                                              device=device, with_embeddings=False)
        self.audio_generation_expert = GPT(gpt_config.from_name("meta-llama/Llama-3.2-Generation"),
                                           device=device, with_embeddings=False)
        self._h = None
        self._st = None
        self.sampling_seed = None      # set by callers that key the sampler themselves (CLI: per-utterance keys)
        self.weight_dtype = None       # torch.float8_e4m3fn: every bf16 plan setup_caches builds computes with the fp8 weight-only forms W' and streams fp8 images in its few-row launches (CLI --weight_dtype)
        self.order_free_rows = 0       # > 0: every plan setup_caches builds opts its many-row launches into the order-free GEMM (CLI --order_free_rows)
        self.top_p = 0.0               # set_top_p: nucleus filter of the sampled heads (0 = off), re-applied to every plan setup_caches builds
        self.repetition_penalty = (1.0, 64)   # set_repetition_penalty: (penalty, window) of the sampled heads (1.0 = off), re-applied likewise

    # ---- caches / device plan ----------------------------------------------------------------
    def setup_caches(self, max_batch_size: int, dtype: Optional[torch.dtype] = None, max_seq_length: int = 2048,
                     max_rows: Optional[int] = None, log_frames: int = 512, weight_dtype=_UNSET):
        """model_new.py:554-565: 2048-slot caches for the three 3072-d GPTs, `audio_num_codebooks`
        slots for the local decoder.  `dtype` selects the kernel precision (default: the
        parameters' dtype, as in the reference where `.to(dtype)` decides).
        weight_dtype: None | torch.float8_e4m3fn (left out: self.weight_dtype).  fp8 (bf16 plans only; LOSSY: relative rms error of a
        weight 2.7e-2 against bf16's 1.6e-3): every Linear of the four GPTs, projection, audio_head[i] and lm_head is replaced by
        W' = RNE_e4m3fn(W 2^-e) 2^e with a power-of-two scale per output row (ops.dequant_w8) — embeddings, norms, RoPE tables and
        the K/V caches are not touched.  The packed bf16 weights then hold W' and the launches of decode frames of up to 64 rows (the few-row decode kernel up to 5, the weights-stationary kernel above) stream the fp8 images
        (half the bytes); the plan is bit-identical to a bf16 plan loaded with W'.  Costs 1.5 x the bf16 weight memory."""
        p0 = self.projection.weight
        device, dtype = p0.device, (dtype or p0.dtype)
        if weight_dtype is _UNSET:
            weight_dtype = getattr(self, "weight_dtype", None)
        if weight_dtype is not None and weight_dtype != torch.float8_e4m3fn:
            raise ValueError(f"weight_dtype must be None or torch.float8_e4m3fn, got {weight_dtype}")
        if weight_dtype is not None and dtype != torch.bfloat16:
            raise ValueError("weight_dtype=torch.float8_e4m3fn needs a bf16 plan (dtype=torch.bfloat16); the fp32 plan is the exact contract")
        if device.type != "cuda":
            raise RuntimeError("uniaudio2_amd runs on a ROCm device only (no CPU fallback); call model.to('cuda')")
        cfg = self.config
        ncb, va = cfg.audio_num_codebooks, cfg.audio_semantic_vocab_size + cfg.audio_reason_vocab_size
        B = max_batch_size
        max_rows = max(max_rows or 64, B)
        self._destroy()
        for g in (self.audio_understanding_expert, self.backbone, self.audio_generation_expert):
            g.set_kv_cache(B, max_seq_length=max_seq_length, device=device, dtype=dtype, weight_dtype=weight_dtype)
        self.decoder.set_kv_cache(B, max_seq_length=ncb, device=device, dtype=dtype, weight_dtype=weight_dtype)
        st = dict(dtype=dtype, device=device, B=B, max_rows=max_rows, log_frames=log_frames, ncb=ncb, va=va, weight_dtype=weight_dtype)
        w8 = []                        # (bf16 twin, fp8 image, exponents) of the heads' weights

        def pack(w, transposed=False):
            if weight_dtype is None:
                return ops.pack_linear(w.detach(), dtype, transposed=transposed)
            q, e, twin = ops.pack_linear_w8(w.detach(), transposed=transposed)
            w8.append((twin, q, e))
            return twin

        cast = lambda t: t.detach().to(device=device, dtype=dtype).contiguous()
        st["wte"] = cast(self.backbone.transformer.wte.weight)
        st["audio_emb"] = cast(self.audio_embeddings.weight)
        st["lm_head"] = pack(self.backbone.lm_head.weight)
        st["projection"] = pack(self.projection.weight)
        st["audio_head"] = [pack(self.audio_head[i], transposed=True) for i in range(ncb)]
        i32 = dict(dtype=torch.int32, device=device)
        st["tokens"] = torch.zeros(max_rows, ncb + 1, **i32)
        st["mask"] = torch.zeros(max_rows, ncb + 1, dtype=torch.uint8, device=device)
        st["row_pos"] = torch.zeros(max_rows, **i32)
        st["row_seq"] = torch.zeros(max_rows, **i32)
        st["dec_pos"] = torch.arange(ncb, **i32).unsqueeze(1).expand(ncb, max_rows).contiguous()
        st["dec_seq"] = torch.arange(max_rows, **i32)
        st["forbid"] = torch.zeros(max_rows, **i32)
        st["out_tokens"] = torch.zeros(max_rows, ncb + 1, **i32)
        st["frame_log"] = torch.zeros(log_frames, max_rows, ncb + 1, **i32)
        st["counters"] = torch.zeros(4, **i32)

        d = Stage3Desc()
        d.dtype, d.n_cb, d.va, d.vt = ops.dtype_code(dtype), ncb, va, self.backbone.config.padded_vocab_size
        d.max_rows, d.max_batch = max_rows, B
        gd = [self.audio_understanding_expert.desc(), self.backbone.desc(), self.audio_generation_expert.desc(),
              self.decoder.desc()]
        d.und, d.backbone, d.gen, d.decoder = gd
        d.wte, d.audio_emb = st["wte"].data_ptr(), st["audio_emb"].data_ptr()
        d.lm_head, d.projection = st["lm_head"].data_ptr(), st["projection"].data_ptr()
        ah = (vp * ncb)(*[t.data_ptr() for t in st["audio_head"]])
        d.audio_head = ah
        for k in ("tokens", "mask", "row_pos", "row_seq", "dec_pos", "dec_seq", "forbid", "out_tokens", "frame_log",
                  "counters"):
            setattr(d, k, st[k].data_ptr())
        d.log_frames = log_frames
        n = lib.ua2_stage3_scratch_floats(C.byref(d))
        st["scratch"] = torch.empty(n, dtype=torch.float32, device=device)
        d.scratch, d.scratch_floats = st["scratch"].data_ptr(), n
        h = vp()
        check(lib.ua2_stage3_create(C.byref(d), C.byref(h)), "ua2_stage3_create")
        st["keep"] = (d, gd, ah)
        self._h, self._st = h, st
        self._sampling = None
        self._cfg = 1.0
        self._w8_on = False            # fp8 twins attached (set_w8)
        self._order_free = 0           # set_order_free_rows
        self._pos_hi = 0
        self._text_fed_back = 0        # rows 0.._text_fed_back-1 were fed back by a text-feedback frame (they hold masks audio 0 / text 1); 0 = none known
        self._ngram = None             # (n, fallback, capacity) of the text frames' n-gram filter (set_ngram); None = off
        self._ngram_rows = [0] * B     # per-row upper bounds of the n-gram history lengths (host side: no device sync), in row order
        self._beam = None              # the running beam search (begin_beams .. end_beams); None = off
        self._row_streams = False      # per-row sampler streams registered with the executor (set_row_seeds)
        if getattr(self, "order_free_rows", 0) > 0 and dtype == torch.bfloat16:
            self.set_order_free_rows(self.order_free_rows)
        if getattr(self, "top_p", 0.0) > 0.0:
            self.set_top_p(self.top_p)         # a new plan starts with the filter off: re-apply what set_top_p remembered
        if getattr(self, "repetition_penalty", (1.0, 64))[0] != 1.0:
            self.set_repetition_penalty(*self.repetition_penalty)
        if weight_dtype is not None:
            for g in (self.audio_understanding_expert, self.backbone, self.audio_generation_expert, self.decoder):
                w8 += g.plan["w8"]
            st["w8"] = w8              # keeps the fp8 images alive while the executor points at them
            self.set_w8(True)

    def set_w8(self, on: bool = True):
        """Attach (or, on=False, clear) the fp8 images of a plan built with weight_dtype=torch.float8_e4m3fn.  Cleared, every launch
        reads the bf16 forms of W' — the same ids and logits bit for bit, at the bf16 plan's speed.  Either way the captured frame
        graphs are dropped (include/ua2hip.h ua2_stage3_set_w8)."""
        self._need()
        w8 = self._st.get("w8")
        if w8 is None:
            raise ValueError("this plan was built without fp8 weights (setup_caches(..., weight_dtype=torch.float8_e4m3fn))")
        if not on:
            check(lib.ua2_stage3_set_w8(self._h, None, 0), "ua2_stage3_set_w8")
            self._w8_on = False
            return
        tab = (W8Entry * len(w8))(*[W8Entry(t.data_ptr(), q.data_ptr(), e.data_ptr()) for t, q, e in w8])
        check(lib.ua2_stage3_set_w8(self._h, tab, len(w8)), "ua2_stage3_set_w8")
        self._w8_on = True

    def set_lossless(self, on: bool = True):
        """Switch the plan's lossless 13-bit weight images (bf16 plans; on by default) on or off: the same ids and logits bit for bit
        either way; the captured frame graphs are dropped (include/ua2hip.h ua2_stage3_set_lossless)."""
        self._need()
        check(lib.ua2_stage3_set_lossless(self._h, int(bool(on))), "ua2_stage3_set_lossless")

    def lossless_stats(self):
        """ua2_stage3_lossless_stats as a dict: matrices with / without an image, bytes per frame, extra device memory, build time."""
        from .._lib import LosslessInfo
        self._need()
        info = LosslessInfo()
        check(lib.ua2_stage3_lossless_stats(self._h, C.byref(info)), "ua2_stage3_lossless_stats")
        return {k: getattr(info, k) for k, _ in LosslessInfo._fields_ if k != "reserved"}

    def _destroy(self):
        if self._h is not None:
            lib.ua2_stage3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def reset_caches(self):
        """model_new.py:647-651."""
        self._need()
        st = self._st
        st["counters"][0:1].zero_()      # frame-log slot; the sampler's draw index [1] keeps counting (like a generator)
        st["forbid"].zero_()

    def rewind_frame_log(self):
        """Rewinds the frame-log slot (counters[0]) between two generate_frames calls of a running session, once the caller has
        copied the last call's slice out (the returned slice is a view of the log): a session that admits runs more frames than
        log_frames.  Nothing else moves — positions, forbid, draws and the caches stay.  Safe against the deferred text head: its
        ring is indexed by counters[0] % capacity, the flush windows of a call are planned from the slot the call starts at, and
        every flush is issued before generate_frames returns, so no stashed row outlives a call."""
        self._need()
        self._st["counters"][0:1].zero_()

    @property
    def _ngram_hi(self):
        """Upper bound of the longest n-gram history of any row of the plan; assigning sets every row's bound."""
        return max(self._ngram_rows, default=0)

    @_ngram_hi.setter
    def _ngram_hi(self, frames):
        self._ngram_rows = [int(frames)] * len(self._ngram_rows)

    def _need(self):
        if self._h is None:
            raise TypeError("You need to call `model.setup_caches()`")

    def _check_positions(self, max_pos: int):
        """Every position a launch touches must lie inside the caches planned by setup_caches: the QKV epilogue
        indexes the RoPE tables and the page table by position, so a position past the end would write K/V into
        another sequence's pages.  The reference fails loudly in the same situation (`index_copy_` on the
        2048-slot cache, lit_model.py:831-856); so does this."""
        limit = self.backbone.plan["max_seq"]
        if max_pos >= limit or max_pos < 0:
            raise ValueError(f"position {max_pos} is outside the KV cache / RoPE tables planned for max_seq_length="
                             f"{limit} (setup_caches); shorten the prompt, generate fewer frames or plan a longer cache")

    def _set_groups(self, pos, seq):
        """Row groups of the next prefill chunk for the MFMA flash attention (bf16 plans; the exact-fp32 plan keeps the
        row-by-row kernel).  pos, seq: the chunk's row positions / sequences (any device)."""
        st = self._st
        if st["dtype"] != torch.bfloat16:
            return
        cfg = self.backbone.config
        g = ops.attn_groups(pos.cpu().numpy(), seq.cpu().numpy(), cfg.n_head, cfg.n_query_groups, st["device"])
        st["groups"] = g                   # keeps the device tables alive while the executor points at them
        check(lib.ua2_stage3_set_prefill_groups(self._h, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[0].shape[0], g[3]),
              "ua2_stage3_set_prefill_groups")

    def _load_rows(self, tokens, tokens_mask, pos, seq):
        """tokens (R, 9) any int dtype, mask (R, 9) bool, pos (R,), seq (R,) -> device state."""
        st = self._st
        R = tokens.shape[0]
        self._text_fed_back = 0                    # tokens / masks from outside: nothing is known about the rows' step kinds
        st["tokens"][:R].copy_(tokens)
        st["mask"][:R].copy_(tokens_mask)
        st["row_pos"][:R].copy_(pos)
        st["row_seq"][:R].copy_(seq)
        if "ngram_len" in st:                      # rows that start here start with an empty n-gram history
            st["ngram_len"][:R].zero_()
            self._ngram_hi = 0                     # (every row: a session starts here)
        if "rep_len" in st:                        # ... and with empty repetition histories
            st["rep_len"][:R].zero_()
        return R

    def _run_chunks(self, tk, mk, ps, sq, chunk, groups, after=None):
        """The time-major chunk loop of prefill and scoring.  tk, mk (R, 9), ps, sq (R,): the rows' tokens, masks, positions and
        sequences.  Rows are sorted by position (stable), so a chunk only needs K/V of itself and of earlier chunks, and run `chunk`
        rows at a time through ua2_stage3_trunk — with prefill row groups when `groups`.  after(order, s0, n), when given, is called
        after each chunk's trunk, the chunk being rows order[s0:s0 + n] of the input.  Returns order."""
        order = torch.argsort(ps, stable=True)
        tk, mk, ps, sq = tk[order], mk[order], ps[order], sq[order]
        lo, hi = ps[[0, -1]].tolist()                       # sorted: the extremes
        self._check_positions(hi)
        self._check_positions(lo)
        s = ops.stream()
        for s0 in range(0, tk.shape[0], chunk):
            c = slice(s0, s0 + chunk)
            n = self._load_rows(tk[c], mk[c], ps[c], sq[c])
            if groups:
                self._set_groups(ps[c], sq[c])
            check(lib.ua2_stage3_trunk(self._h, n, s), "ua2_stage3_trunk")
            if after is not None:
                after(order, s0, n)
        return order

    # ---- reference-compatible methods ---------------------------------------------------------
    @torch.inference_mode()
    def forward_prefix(self, tokens: torch.Tensor, labels: torch.Tensor = None, tokens_mask: torch.Tensor = None,
                       loss_mask: torch.Tensor = None, input_pos=None, input_pos_maxp1=None):
        """model_new.py:456-507 — fills the KV caches of the three trunk GPTs for `tokens`
        (B, S, 9) at `input_pos` (B, S).  `tokens_mask` is (B, S+1, 9) as the generators pass it
        (evaluation/tts_task.py:244); only [:, :-1] is used (:476-480).  The reference's lm_head /
        local-decoder pass over the prefix (:498-506) produces values every caller discards and is
        skipped; returns None."""
        self._need()
        st = self._st
        B, S, W = tokens.shape
        if input_pos is None:
            input_pos = torch.arange(S, device=tokens.device).unsqueeze(0).expand(B, S)
        mask = tokens_mask[:, :S]
        seq = torch.arange(B, device=tokens.device).unsqueeze(1).expand(B, S)
        self._run_chunks(tokens.reshape(B * S, W), mask.reshape(B * S, W), input_pos.reshape(-1), seq.reshape(-1), st["max_rows"], True)
        return None

    # ---- teacher-forced scoring (model_new.py:402-454 forward; include/ua2hip.h ua2_stage3_score) ---------------------------------
    def _teacher_forced(self, tokens, labels, tokens_mask, text_labels, input_pos, sink=None):
        """The chunk loop shared by score and forward: the B * S rows in time-major order, at most max_batch per chunk, each chunk
        through ua2_stage3_trunk + ua2_stage3_score.  Returns (nll, pred, lab) as (B, S, W) tensors in the token layout; sink(rows,
        n), when given, is called after every chunk with the chunk's flat row indices (b * S + s) while the plan's two logits
        buffers hold that chunk."""
        self._need()
        st = self._st
        if self._beam is not None:
            raise ValueError("a beam search is running (end_beams): its rows and pages are live in the plan")
        dev = st["device"]
        B, S, W = tokens.shape
        ncb, va, vt = st["ncb"], st["va"], self.backbone.config.padded_vocab_size
        if W != ncb + 1 or tuple(labels.shape) != (B, S, ncb) or tokens_mask.shape[0] != B or tokens_mask.shape[1] < S + 1:
            raise ValueError(f"expected tokens (B, S, {ncb + 1}), labels (B, S, {ncb}), tokens_mask (B, S + 1, {ncb + 1}); got "
                             f"{tuple(tokens.shape)}, {tuple(labels.shape)}, {tuple(tokens_mask.shape)}")
        if B > st["B"]:
            raise ValueError(f"setup_caches({st['B']}) is too small for {B} sequences")
        tokens, labels, tokens_mask = tokens.to(dev), labels.to(dev), tokens_mask.to(dev)
        if text_labels is None:
            text_labels = torch.full((B, S), -1, dtype=torch.long, device=dev)
        text_labels = text_labels.to(dev)
        if tuple(text_labels.shape) != (B, S):
            raise ValueError(f"text_labels must be (B, S) = ({B}, {S}), got {tuple(text_labels.shape)}")
        for name, t, V in (("labels", labels, va), ("text_labels", text_labels, vt)):
            if t.numel() and (int(t.min().item()) < -1 or int(t.max().item()) >= V):
                raise ValueError(f"{name} must lie in [-1, {V}) (-1 = ignored); got [{int(t.min().item())}, {int(t.max().item())}]")
        if input_pos is None:
            input_pos = torch.arange(S, device=dev).unsqueeze(0).expand(B, S)
        audio_next = tokens_mask[:, 1:S + 1, 0].bool()                     # rows whose NEXT step is an audio step: the rows the local decoder scores
        lab = torch.cat([torch.where(audio_next.unsqueeze(-1), labels, torch.full_like(labels, -1)), text_labels.unsqueeze(-1)], dim=-1)
        seq = torch.arange(B, device=dev).unsqueeze(1).expand(B, S)
        R = B * S
        lb = lab.reshape(R, W).to(torch.int32)
        nll = torch.zeros(R, W, dtype=torch.float32, device=dev)           # both in the chunks' (time-major) row order
        pred = torch.zeros(R, W, dtype=torch.int32, device=dev)

        def score_chunk(order, s0, n):
            rows = order[s0:s0 + n]
            lab_n = lb[rows]                                               # the chunk's labels, contiguous
            check(lib.ua2_stage3_score(self._h, n, lab_n.data_ptr(), nll[s0:].data_ptr(), pred[s0:].data_ptr(), ops.stream()), "ua2_stage3_score")
            if sink is not None:
                sink(rows, n)

        order = self._run_chunks(tokens.reshape(R, W), tokens_mask[:, :S].reshape(R, W), input_pos.to(dev).reshape(-1), seq.reshape(-1),
                                 st["B"], False, score_chunk)
        inv = torch.empty_like(order)
        inv[order] = torch.arange(R, device=dev)
        nll, pred = nll[inv].view(B, S, W), pred[inv].view(B, S, W)
        nll[..., :ncb] = torch.where(audio_next.unsqueeze(-1), nll[..., :ncb], torch.zeros_like(nll[..., :ncb]))
        pred[..., :ncb] = torch.where(audio_next.unsqueeze(-1), pred[..., :ncb], torch.full_like(pred[..., :ncb], -1))
        return nll, pred, lab

    @torch.inference_mode()
    def score(self, tokens: torch.Tensor, labels: torch.Tensor, tokens_mask: torch.Tensor, loss_mask: torch.Tensor = None,
              text_labels: torch.Tensor = None, input_pos=None, loss_weights=None):
        """Teacher-forced scoring on the device: what model_new.py:402-454 `forward` computes, reduced to per-token losses by the
        cross-entropy tail (ua2_xent_embed) — no logits leave the plan.  Shapes as forward: tokens (B, S, 9), labels (B, S, 8) audio
        only, tokens_mask and loss_mask (B, S + 1, 9) (loss_mask None: ones); text_labels (B, S), -1 = ignored (default: all -1).
        Labels outside [-1, V) raise ValueError before any launch.  The B * S rows run time-major in chunks of at most max_batch
        rows (ua2_stage3_trunk + ua2_stage3_score per chunk), in the decode frame's launch forms, so on the default plans a row's
        bits depend neither on the batch nor on the chunking.  Needs setup_caches (B <= max_batch_size); overwrites the K/V
        positions it visits and the decode state's rows, so it must not be called in the middle of a generation.
        Returns dict(nll (B, S, 9) fp32, pred (B, S, 9) int32, metrics): token layout (audio streams first, text last); the audio
        streams of rows with tokens_mask[:, 1:, 0] == 0 hold 0 / -1.  metrics: the keys of CrossEntropyAndAccuracy_text (mask =
        tokens_mask[:, 1:, -1] & loss_mask[:, 1:, -1]) and CrossEntropyAndAccuracy_residual (over the rows tokens_mask[:, 1:, 0]
        selects, loss_weights = ones(n_cb) unless given), reduced on the device in float64 from nll / pred by the reference's formulas."""
        nll, pred, lab = self._teacher_forced(tokens, labels, tokens_mask, text_labels, input_pos)
        S = nll.shape[1]
        tm = tokens_mask.to(nll.device)[:, 1:S + 1].bool()
        lm = torch.ones_like(tm) if loss_mask is None else loss_mask.to(nll.device)[:, 1:S + 1].bool()
        metrics = metrics_from_stats(score_stats(nll, pred, lab, tm, lm), None if loss_weights is None else len(loss_weights))
        return {"nll": nll, "pred": pred, "metrics": metrics}

    @torch.inference_mode()
    def score_sequence(self, tokens: torch.Tensor, mask: torch.Tensor, loss_mask: torch.Tensor = None, loss_weights=None):
        """score of whole sequences: tokens (B, L, 9), mask (B, L, 9), loss_mask (B, L, 9) or None.  Step t predicts step t + 1:
        tokens[:, :-1] go in, labels = tokens[:, 1:, :-1], text_labels = tokens[:, 1:, -1] where mask[:, 1:, -1], else -1.  The
        result's row s scores the tokens of step s + 1."""
        text_labels = torch.where(mask[:, 1:, -1].bool(), tokens[:, 1:, -1], torch.full_like(tokens[:, 1:, -1], -1))
        return self.score(tokens[:, :-1], tokens[:, 1:, :-1], mask, loss_mask, text_labels=text_labels, loss_weights=loss_weights)

    @torch.inference_mode()
    def forward(self, tokens: torch.Tensor, labels: torch.Tensor, tokens_mask: torch.Tensor, loss_mask: torch.Tensor,
                input_pos=None, input_pos_maxp1=None):
        """model_new.py:402-454: returns (text_logits (B, S, Vt), ci_logits (N, 8, Va), choosed_label, choosed_mask) with the N audio
        steps in the reference's row order (tokens_mask[:, 1:, 0].bool() indexing).  Assembled chunk by chunk from the plan's two
        logits buffers behind the launches of `score`.  Departures from the reference: it needs setup_caches; it overwrites the K/V
        positions it visits (and the decode state's rows), so it must not be called in the middle of a generation; it materialises
        the logits (B * S * Vt floats), so it is meant for parity checks and small inputs — `score` is the form for corpora.
        Inference only (no gradients)."""
        self._need()
        st = self._st
        dev = st["device"]
        B, S, W = tokens.shape
        ncb, va, vt = st["ncb"], st["va"], self.backbone.config.padded_vocab_size
        text_all = torch.empty(B * S, vt, dtype=torch.float32, device=dev)
        audio_all = torch.empty(B * S, ncb, va, dtype=torch.float32, device=dev)

        def sink(rows, n):
            text_all[rows] = self.buffer("text_logits", n)
            audio_all[rows] = self.buffer("audio_logits", n)

        self._teacher_forced(tokens, labels, tokens_mask, None, input_pos, sink=sink)
        sel = tokens_mask.to(dev)[:, 1:S + 1, 0].bool()
        return (text_all.view(B, S, vt), audio_all.view(B, S, ncb, va)[sel], labels.to(dev)[sel],
                loss_mask.to(dev)[:, 1:S + 1, :][sel])

    @torch.inference_mode()
    def generate_frame(self, tokens: torch.Tensor, tokens_mask: torch.Tensor, input_pos: torch.Tensor,
                       input_pos_maxp1=None, temperature: float = 1.0, topk: int = 1, forbid_prefix: int = 0,
                       cfg_scale: float = 1.0) -> torch.Tensor:
        """model_new.py:568-645.  tokens (B, 1, 9), tokens_mask (B, 1, 9), input_pos (1,) shared
        or (B,) per sequence.  Returns (B, 9) int32 [text, a0..a7] on device."""
        self._need()
        self.set_sampling(topk, temperature)
        self.set_cfg(cfg_scale if tokens.size(0) > 1 else 1.0)
        if temperature <= 0:
            raise ValueError("temperature must be > 0")
        st = self._st
        B, S, W = tokens.shape
        assert S == 1 and W == st["ncb"] + 1, "last stream must be text"
        pos = input_pos.reshape(-1)
        if pos.numel() == 1:
            pos = pos.expand(B)
        seq = torch.arange(B, device=tokens.device)
        self._load_rows(tokens.reshape(B, W), tokens_mask.reshape(B, W), pos, seq)
        st["forbid"][:B].fill_(int(forbid_prefix))
        self._check_positions(int(pos.max().item()))
        self._check_positions(int(pos.min().item()))
        check(lib.ua2_stage3_frame(self._h, B, -1, 0, 0, 1, ops.stream()), "ua2_stage3_frame")
        return st["out_tokens"][:B].clone()

    def set_sampling(self, topk: int = 1, temperature: float = 1.0, seed: Optional[int] = None):
        """topk == 1: greedy (masked arg-max, lowest index on ties).  topk > 1: model_new.py:146-187 on device
        (top-k threshold, exponential-race draw) with a counter-based generator keyed by `seed` (default: the
        torch seed, multi_task_inference.py:159) — reproducible, but not torch's random stream."""
        self._need()
        if temperature <= 0:
            raise ValueError("temperature must be > 0")
        va = self._st["va"]
        if topk <= 0 or topk > va:
            raise ValueError(f"topk must be in 1..{va}")
        if seed is None:
            seed = self.sampling_seed if self.sampling_seed is not None else torch.initial_seed()
        key = (int(topk), float(temperature), int(seed) & (2 ** 64 - 1))
        if getattr(self, "_sampling", None) != key:
            # a new key rewinds the draw index on the device; the same key keeps counting (like a global generator)
            check(lib.ua2_stage3_set_sampling(self._h, key[0], key[1], key[2], ops.stream()), "ua2_stage3_set_sampling")
            self._sampling = key

    def set_top_p(self, top_p: float = 0.0):
        """Nucleus (top-p) filter of the sampled heads (llm_utils/sampling.py:66-82; include/ua2hip.h ua2_sample_topp): with
        set_sampling(topk > 1, ...) and 0 < top_p < 1 every sampler keeps, among its top-k columns, those whose strictly-more-probable
        mass is at most top_p of the kept mass (ties at the threshold all kept), then draws as before.  0.0 (the default) and 1.0 are
        off; pure nucleus sampling is topk = the audio vocabulary width.  Greedy frames and beam search ignore it.  The value is
        remembered and re-applied to every plan setup_caches builds."""
        top_p = float(top_p)
        if not 0.0 <= top_p <= 1.0:            # (NaN fails both comparisons)
            raise ValueError(f"top_p must be in [0, 1] (0 = off), got {top_p}")
        self.top_p = top_p
        if self._h is not None:
            check(lib.ua2_stage3_set_top_p(self._h, top_p), "ua2_stage3_set_top_p")

    def set_repetition_penalty(self, penalty: float = 1.0, window: int = 64):
        """Repetition penalty of the sampled heads (include/ua2hip.h ua2_sample_penalized / ua2_stage3_set_rep_penalty; the CTRL /
        Hugging Face rule over a window; not in the reference): with set_sampling(topk > 1, ...) and penalty != 1 every sampler reads
        the logits of the distinct ids among the last `window` ids ITS stream has produced for the row (0 = text head, 1 + i = audio
        codebook i; prompt tokens do not count) as l * penalty if l < 0 else l / penalty, before the temperature, and appends the id
        it draws.  The histories (st["rep_hist"] [B, 1 + n_cb, window], st["rep_len"] [B, 1 + n_cb]) are allocated on first use (and
        again for a new window), start empty for every row that begin_decode / begin_ragged / admit_rows starts, and travel with
        retire_rows.  penalty = 1.0 (the default) clears it.  Greedy frames, beam search and scoring ignore it.  The value is
        remembered and re-applied to every plan setup_caches builds.  Its effect on audio quality is not measured: no trained
        checkpoint ships."""
        penalty, window = float(penalty), int(window)
        if not (math.isfinite(penalty) and penalty > 0.0):
            raise ValueError(f"repetition penalty must be finite and > 0 (1 = off), got {penalty}")
        if not 1 <= window <= 512:
            raise ValueError(f"repetition window must be in 1..512, got {window}")
        self.repetition_penalty = (penalty, window)
        if self._h is None:
            return
        st = self._st
        if penalty == 1.0:
            check(lib.ua2_stage3_set_rep_penalty(self._h, 1.0, window, None, None), "ua2_stage3_set_rep_penalty")
            return
        if max(st["va"], self.backbone.config.padded_vocab_size) > 131072:
            raise ValueError("the repetition penalty serves vocabularies up to 131072 columns")
        if "rep_hist" not in st or st["rep_hist"].shape[2] != window:
            with torch.inference_mode(False):      # decode state like the rest of st: written in and out of inference mode
                i32 = dict(dtype=torch.int32, device=st["device"])
                st["rep_hist"] = torch.zeros(st["B"], st["ncb"] + 1, window, **i32)
                st["rep_len"] = torch.zeros(st["B"], st["ncb"] + 1, **i32)      # a new history: every row starts empty
        check(lib.ua2_stage3_set_rep_penalty(self._h, penalty, window, st["rep_hist"].data_ptr(), st["rep_len"].data_ptr()),
              "ua2_stage3_set_rep_penalty")

    def set_row_seeds(self, seeds, rows=None):
        """Per-row sampler streams (include/ua2hip.h ua2_stage3_set_row_streams): row rows[i] (default i) of the decode state draws
        under its own 64-bit key seeds[i] from draw index 0, so under top-k a row's ids depend on its key and its own frame count
        alone — not on its row index, its neighbours or the frames run before it.  Row b with seed k then generates what a B = 1
        run under set_sampling(topk, T, seed=k) generates.  The arrays (st["row_key"] [B, 2], st["row_draw"] [B]) are allocated on
        first use, travel with retire_rows, and give both rows of a guided pair one stream when the caller gives them one seed.
        set_row_seeds(None) returns to the shared stream of set_sampling.  Greedy frames never read the streams."""
        self._need()
        st = self._st
        if seeds is None:
            check(lib.ua2_stage3_set_row_streams(self._h, None, None), "ua2_stage3_set_row_streams")
            self._row_streams = False
            return
        seeds = list(seeds)
        rows = list(range(len(seeds))) if rows is None else [int(r) for r in rows]
        if len(rows) != len(seeds) or len(set(rows)) != len(rows) or any(not 0 <= r < st["B"] for r in rows):
            raise ValueError(f"rows must name {len(seeds)} distinct rows of the plan (0..{st['B'] - 1}), got {rows}")
        if "row_key" not in st:
            with torch.inference_mode(False):      # decode state like the rest of st: written in and out of inference mode
                st["row_key"] = torch.zeros(st["B"], 2, dtype=torch.int32, device=st["device"])
                st["row_draw"] = torch.zeros(st["B"], dtype=torch.int32, device=st["device"])
        if rows:
            idx = torch.tensor(rows, dtype=torch.long, device=st["device"])
            st["row_key"][idx] = torch.tensor([_seed_words(s) for s in seeds], dtype=torch.int32, device=st["device"])
            st["row_draw"][idx] = 0
        check(lib.ua2_stage3_set_row_streams(self._h, st["row_key"].data_ptr(), st["row_draw"].data_ptr()), "ua2_stage3_set_row_streams")
        self._row_streams = True

    def set_cfg(self, cfg_scale: float = 1.0):
        """Classifier-free guidance (model_new.py:618-622, 634-637): with cfg_scale > 1 a frame of two rows
        (conditional, unconditional) samples from l[1] + (l[0] - l[1]) * cfg_scale and both rows take that sample.
        Applies to generate_frame and generate_frames (mode 2 continues every row from row 0)."""
        self._need()
        cfg_scale = max(float(cfg_scale), 1.0)
        if getattr(self, "_cfg", 1.0) != cfg_scale:
            check(lib.ua2_stage3_set_cfg(self._h, cfg_scale), "ua2_stage3_set_cfg")
            self._cfg = cfg_scale

    def set_ngram(self, n: int = 0, fallback: int = 128000, capacity: int = 512):
        """n-gram repeat filter of the text-feedback frames (generate_frames mode 1; evaluation/asr_task.py:329-432
        generate_asr_with_ngram_sampling): a text id that would repeat an n-gram of the ids the row's filtered text frames have
        produced since its decode started becomes `fallback`, on the device between the text sample and the feedback
        (include/ua2hip.h ua2_ngram_filter).  n <= 1 turns it off (the reference bans nothing with n == 1 either).  The history,
        [max_batch, capacity] int32, is allocated on first use (and again for a new capacity) and kept in the decode state; the
        rows that begin_decode / begin_ragged start begin with an empty one, and retire_rows carries it along.  generate_frames
        refuses a call that would grow a history past `capacity`.  generate_frame (the reference-shaped single frame) is never
        filtered."""
        self._need()
        st = self._st
        n, fallback, capacity = int(n), int(fallback), int(capacity)
        if n > 16:
            raise ValueError(f"no_repeat_ngram_size must be <= 16, got {n}")
        if n <= 1:
            check(lib.ua2_stage3_set_ngram(self._h, 0, 0, None, None, 0), "ua2_stage3_set_ngram")
            self._ngram = None
            return
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        if "ngram_hist" not in st or st["ngram_hist"].shape[1] != capacity:
            i32 = dict(dtype=torch.int32, device=st["device"])
            st["ngram_hist"] = torch.zeros(st["B"], capacity, **i32)
            st["ngram_len"] = torch.zeros(st["B"], **i32)          # a new history: every row starts empty
            self._ngram_hi = 0
        check(lib.ua2_stage3_set_ngram(self._h, n, fallback, st["ngram_hist"].data_ptr(), st["ngram_len"].data_ptr(), capacity),
              "ua2_stage3_set_ngram")
        self._ngram = (n, fallback, capacity)

    def set_order_free_rows(self, rows: int = 0):
        """bf16 plans: trunk launches of >= `rows` rows (batched prefill, decode frames of that many sequences) run on the
        order-free 256-row-tile GEMM (include/ua2hip.h ua2_stage3_set_order_free_rows; 0 = off, the default: every row keeps
        the bits of its single-sequence run)."""
        self._need()
        check(lib.ua2_stage3_set_order_free_rows(self._h, int(rows)), "ua2_stage3_set_order_free_rows")
        self._order_free = int(rows)

    def _defer_cap_rows(self, batch: int, mode: int, n_frames: int, skip_text_head: bool) -> int:
        """Rows of the stash ring a generate_frames call may defer its text head into; 0 = the call runs every frame as it is."""
        st = self._st
        if mode != 0 or skip_text_head or n_frames < 2 or DEFER_CAP_ROWS // batch < 2:
            return 0
        if (self._sampling is not None and self._sampling[0] != 1) or self._cfg != 1.0 or self._w8_on:
            return 0                   # top-k sampling, guided pairs and fp8 plans keep lm_head in the frame
        if st["dtype"] == torch.bfloat16 and 0 < self._order_free <= batch:
            return 0                   # the order-free opt-in covers frames of `batch` rows: their lm_head is not row-invariant
        cap = int(lib.ua2_stage3_defer_rows())   # UA2_DEFER_ROWS (tests, sweeps); 0 under UA2_NO_DEFER_TEXT_HEAD=1
        return cap if cap // batch >= 1 else 0

    # ---- MI355X-native fast path ---------------------------------------------------------------
    @torch.inference_mode()
    def generate_frames(self, n_frames: int, batch: int, mode: int, reason_eos: int = -1, reason_card: int = 0,
                        max_pos: Optional[int] = None, use_graph: bool = True, frame_events=None,
                        skip_text_head: bool = False, skip_audio_experts: bool = False,
                        defer_text_head: bool = True) -> torch.Tensor:
        """Runs `n_frames` frames back to back from the state left by the previous frame (first
        call: after `begin_decode`).  mode 0 = audio feedback (evaluation/tts_task.py:259-280),
        1 = text feedback (evaluation/asr_task.py:668-682; the depth decoder is skipped there — its samples are
        never fed back — so the audio columns of the log are zeros), 2 = guided pair.  Returns the log slice
        (n_frames, batch, 9) int32 (device).
        skip_text_head (modes 0 and 2): lm_head and the text sample are skipped — the audio loops feed the text id back under
        a zero mask and never read it (tts_task.py:259,274-277), so the audio columns are bit-identical with and without it;
        the text column of the log then holds -1.  The reference-shaped generate_frame always computes it.
        Mode 1 under set_ngram(n >= 2): the log's text column and the fed-back text id are the n-gram-filtered ids.
        defer_text_head (mode 0 without skip_text_head; greedy, unguided, no fp8 twins, not under the order-free opt-in, n_frames
        >= 2, batch <= 32; UA2_NO_DEFER_TEXT_HEAD=1 turns it off): in the audio loop the text id is fed back under a zero mask, so
        the text ids of different frames are independent of each other and of the audio ids.  Every frame but the call's last
        runs as UA2_FRAME_DEFER_TEXT_HEAD — no lm_head, its h_final rows kept in a 64-row ring — and lm_head runs once per
        64 // batch frames over the kept rows (ua2_stage3_text_flush, windows: defer_windows): one pass over its weights instead
        of one per frame, the same ids and logits bit for bit (row invariance).  The last frame runs whole, so text_logits,
        out_tokens and the fed-back state hold after the call what they hold without deferral; every flush is issued before the
        call returns, so the returned log slice is complete in stream order and nothing deferred outlives the call."""
        if skip_text_head:
            if mode not in (0, 2):
                raise ValueError("skip_text_head applies to the audio-feedback modes (0, 2)")
            mode = mode | 16                                  # UA2_FRAME_SKIP_TEXT_HEAD
        if skip_audio_experts and mode not in (1, 3):
            raise ValueError("skip_audio_experts applies to the text-feedback modes (1, 3)")
        self._need()
        st = self._st
        if mode == 3:
            # a beam frame: one row per slot of every group; every step writes one record of each group's step log and reads one more
            # length-penalty entry
            bm = self._beam
            if bm is None:
                raise ValueError("mode 3 runs between begin_beams and end_beams")
            if batch != bm["G"] * bm["W"]:
                raise ValueError(f"a beam frame has one row per slot: batch must be {bm['G'] * bm['W']}, got {batch}")
            if bm["steps"] + n_frames > bm["cap"]:
                raise ValueError(f"beam step log full: {bm['steps']} + {n_frames} steps > max_length {bm['cap']} (begin_beams)")
            bm["steps"] += n_frames
        if mode == 1 and self._ngram is not None:
            # every text frame appends one id to each live row's n-gram history: never filter against a truncated one.  The bound
            # follows the rows (retire_rows permutes it, admit_rows starts a row at 0): a session that admits may run more frames
            # in all than `capacity`, no row may
            ngram_hi = max(self._ngram_rows[:batch], default=0)
            if ngram_hi + n_frames > self._ngram[2]:
                raise ValueError(f"n-gram history full: {ngram_hi} + {n_frames} frames > capacity {self._ngram[2]} (set_ngram)")
        start = int(st["counters"][0].item())
        if start + n_frames > st["log_frames"]:
            raise ValueError("frame log too small: raise log_frames in setup_caches")
        # the last frame of this call reads / writes position (current max row_pos) + n_frames - 1.  The host-side bound
        # `_pos_hi` avoids a device sync; it can only over-estimate (after retirements), so the exact value is fetched
        # before refusing.  `max_pos` is accepted for compatibility with round-1 callers and ignored.
        limit = self.backbone.plan["max_seq"]
        if self._pos_hi + n_frames - 1 >= limit:
            self._pos_hi = int(st["row_pos"][:batch].max().item())
            self._check_positions(self._pos_hi + n_frames - 1)
        self._pos_hi += n_frames
        if mode == 1 and self._ngram is not None:
            self._ngram_rows[:batch] = [k + n_frames for k in self._ngram_rows[:batch]]
        s = ops.stream()
        cap_rows = self._defer_cap_rows(batch, mode, n_frames, skip_text_head) if defer_text_head else 0
        flush_after = {f0 + n - 1: (f0, n) for f0, n in defer_windows(start, n_frames, batch, cap_rows)} if cap_rows else {}
        for i in range(n_frames):
            # skip_audio_experts (text-only continuations: asr_task.py:666-682 and twins): from the session's SECOND text-feedback frame on
            # every row is a text step fed back by the executor itself (masks audio 0 / text 1) — the first frame consumes the prompt's
            # last token, which may be an audio step, and runs whole.  UA2_FRAME_SKIP_AUDIO_EXPERTS = 32.
            m = mode | 32 if (skip_audio_experts and batch <= self._text_fed_back) else mode
            if cap_rows and i < n_frames - 1:
                m = mode | 64                      # UA2_FRAME_DEFER_TEXT_HEAD
            check(lib.ua2_stage3_frame(self._h, batch, m, reason_eos, reason_card, int(use_graph), s),
                  "ua2_stage3_frame")
            if start + i in flush_after:           # the frame filled the ring's last slot, or is the call's last deferred one
                f0, n = flush_after[start + i]
                check(lib.ua2_stage3_text_flush(self._h, batch, f0, n, s), "ua2_stage3_text_flush")
            self._text_fed_back = batch if mode in (1, 3) else 0       # rows past `batch` may still hold a prompt's audio step
            if frame_events is not None:           # measurement hook: one event after every frame (bench.py p50 / p99)
                frame_events[i].record()
        return st["frame_log"][start:start + n_frames, :batch]

    # ---- ragged batches / continuous batching (the reference has neither: SURVEY.md A.17, §8e) ------
    @torch.inference_mode()
    def forward_prefix_ragged(self, tokens_list, mask_list, seq_ids=None):
        """Prefill of prompts of different lengths in one pass.  tokens_list[b] (L_b, 9), mask_list[b] (L_b, 9):
        the rows to cache for sequence b (callers pass prompt[:-1] as with forward_prefix); sequence b takes
        page-table row seq_ids[b] (default b: rows 0..B-1; distinct, within the plan) and positions 0..L_b-1.  Rows are
        issued time-major in chunks of `max_rows`, so a chunk only ever needs K/V written by itself or by earlier chunks."""
        self._need()
        st = self._st
        dev = st["device"]
        assert len(tokens_list) == len(mask_list) <= st["B"]
        if seq_ids is None:
            seq_ids = range(len(tokens_list))
        seq_ids = [int(b) for b in seq_ids]
        if len(seq_ids) != len(tokens_list) or len(set(seq_ids)) != len(seq_ids) or any(not 0 <= b < st["B"] for b in seq_ids):
            raise ValueError(f"seq_ids must name {len(tokens_list)} distinct sequences of the plan (0..{st['B'] - 1}), got {seq_ids}")
        tk = torch.cat([t.reshape(-1, t.shape[-1]) for t in tokens_list]).to(dev)
        mk = torch.cat([m.reshape(-1, m.shape[-1]) for m in mask_list]).to(dev)
        ps = torch.cat([torch.arange(t.shape[0], device=dev) for t in tokens_list])
        sq = torch.cat([torch.full((t.shape[0],), b, device=dev) for b, t in zip(seq_ids, tokens_list)])
        self._run_chunks(tk, mk, ps, sq, st["max_rows"], True)
        return None

    @torch.inference_mode()
    def retire_rows(self, keep, batch: int):
        """Continuous batching: of the `batch` live sequences (rows 0..batch-1 of the decode state) keep those at
        indices `keep`, in that order, as rows 0..len(keep)-1.  The per-row decode state and the page-table rows
        of the three trunk caches are permuted together (a permutation, so no page is lost); the local decoder's
        8-slot cache is rewritten every frame and needs nothing.  A row's results do not depend on its index or
        on its neighbours (tests/test_gpu_invariance.py), so retiring never changes what the survivors generate."""
        self._need()
        st = self._st
        keep = [int(k) for k in keep]
        assert len(set(keep)) == len(keep) and all(0 <= k < batch for k in keep)
        gone = [r for r in range(batch) if r not in set(keep)]
        perm = torch.tensor(keep + gone, dtype=torch.long, device=st["device"])
        for k in self._ROW_STATE:
            if k in st:
                st[k][:batch] = st[k][:batch][perm]
        for g in (self.audio_understanding_expert, self.backbone, self.audio_generation_expert):
            pt = g.kv_cache.page_table
            pt[:batch] = pt[:batch][perm]
        self._ngram_rows[:batch] = [self._ngram_rows[r] for r in keep + gone]
        # the survivors are text-fed-back rows only if every permuted row was one; the rows behind them are not vouched for any more
        self._text_fed_back = len(keep) if batch <= self._text_fed_back else 0
        return len(keep)

    # the per-row decode state: what retire_rows permutes and admit_rows keeps across its prefill
    _ROW_STATE = ("tokens", "mask", "row_pos", "forbid", "out_tokens", "ngram_hist", "ngram_len", "row_key", "row_draw", "rep_hist", "rep_len")

    @torch.inference_mode()
    def admit_rows(self, prompts, batch: int, seeds=None):
        """Continuous batching: appends len(prompts) new sequences, prompts[i] = (tokens (L_i, 9), mask (L_i, 9)), as rows batch ..
        batch + len(prompts) - 1 of a RUNNING decode session whose live sequences are rows 0..batch-1; returns the new row count.
        The live rows are not disturbed: after retire_rows the page-table rows at indices >= batch are exactly the free ones
        (retirement permutes), so every prompt[:-1] is prefilled into them (forward_prefix_ragged with seq_ids = batch ..); the
        prefill's chunks pass through the decode state's first rows, so the live rows' state (_ROW_STATE and row_seq) is saved
        before and put back after.  Each prompt's last frame then becomes the first decode frame of its row: position L_i - 1,
        forbid 0, an empty n-gram history and, under set_row_seeds, key seeds[i] at draw 0.  The frame after an admission runs
        the audio experts for every row (an admitted row's first frame consumes a prompt token).  Under guidance (mode 2) the
        caller admits the two rows of a pair together, at an even row, with one seed.  ValueError: more rows than the plan holds,
        or a prompt that does not fit max_seq_length."""
        self._need()
        st = self._st
        dev = st["device"]
        n, batch = len(prompts), int(batch)
        if self._beam is not None:
            raise ValueError("a beam search is running (end_beams): its rows and pages are live in the plan")
        if not 0 <= batch <= st["B"] or batch + n > st["B"]:
            raise ValueError(f"cannot admit {n} sequences beside {batch} live ones: setup_caches({st['B']}) holds {st['B']}")
        if n == 0:
            return batch
        prompts = [(t.to(dev), m.to(dev)) for t, m in prompts]
        Ls = [int(t.shape[0]) for t, _ in prompts]
        limit = self.backbone.plan["max_seq"]
        if min(Ls) < 1 or max(Ls) > limit:
            raise ValueError(f"prompt lengths {Ls}: every prompt needs 1 .. {limit} frames (max_seq_length of setup_caches)")
        if self._row_streams and (seeds is None or len(seeds) != n):
            raise ValueError(f"row streams are on (set_row_seeds): admit_rows needs one seed per prompt, got {seeds}")
        # the prefill loads its chunks through rows 0.. of these (_load_rows): whole copies, the live rows among them
        saved = {k: st[k].clone() for k in ("tokens", "mask", "row_pos", "row_seq", "ngram_len", "rep_len") if k in st}
        ngram_rows = list(self._ngram_rows)
        pre = [i for i in range(n) if Ls[i] > 1]
        if pre:
            self.forward_prefix_ragged([prompts[i][0][:-1] for i in pre], [prompts[i][1][:-1] for i in pre], seq_ids=[batch + i for i in pre])
        for k, v in saved.items():
            st[k].copy_(v)
        self._ngram_rows = ngram_rows
        self._ngram_rows[batch:batch + n] = [0] * n      # as on the device: an admitted row starts with an empty history
        new = slice(batch, batch + n)
        st["tokens"][new] = torch.stack([t[-1] for t, _ in prompts]).to(torch.int32)
        st["mask"][new] = torch.stack([m[-1] for _, m in prompts]).to(torch.uint8)
        st["row_pos"][new] = torch.tensor([L - 1 for L in Ls], dtype=torch.int32, device=dev)
        st["row_seq"][new] = torch.arange(batch, batch + n, dtype=torch.int32, device=dev)
        st["forbid"][new] = 0
        if "ngram_len" in st:
            st["ngram_len"][new] = 0
        if "rep_len" in st:
            st["rep_len"][new] = 0
        if self._row_streams:
            self.set_row_seeds(seeds, rows=range(batch, batch + n))
        self._pos_hi = max(self._pos_hi, max(Ls) - 1)
        self._text_fed_back = 0            # the admitted rows' first frame is a prompt step: the next frame runs whole
        return batch + n

    @torch.inference_mode()
    def begin_ragged(self, prompts):
        """Start of a batched generation: prompts[b] = (tokens (L_b, 9), mask (L_b, 9)) of any lengths.  Resets the caches
        and the page tables (undoing earlier retirements), prefills every prompt[:-1] in one ragged pass and loads each
        last prompt frame as the first decode frame of row b.  Returns the (B,) tensor of decode start positions."""
        self._need()
        st = self._st
        dev = st["device"]
        B = len(prompts)
        assert B <= st["B"], f"setup_caches({st['B']}) is too small for {B} sequences"
        self.reset_caches()
        for g in (self.audio_understanding_expert, self.backbone, self.audio_generation_expert):
            kv = g.kv_cache
            kv.page_table.copy_(torch.arange(kv.page_table.numel(), dtype=torch.int32, device=dev).view_as(kv.page_table))
        self.forward_prefix_ragged([t[:-1] for t, _ in prompts], [m[:-1] for _, m in prompts])
        last_t = torch.stack([t[-1] for t, _ in prompts]).to(dev)
        last_m = torch.stack([m[-1] for _, m in prompts]).to(dev)
        pos = torch.tensor([t.shape[0] - 1 for t, _ in prompts], device=dev)
        self.begin_decode(last_t.unsqueeze(1), last_m.unsqueeze(1), pos)
        return pos

    @torch.inference_mode()
    def generate_ragged(self, prompts, n_frames, mode: int = 0, reason_eos: int = -1, reason_card: int = 0, skip_text_head: bool = False,
                        batch_size: Optional[int] = None, seeds=None):
        """Batched fixed-length generation with continuous batching: prompts[b] = (tokens (L_b, 9), mask (L_b, 9)),
        n_frames[b] frames for sequence b (deterministic stop).  A sequence leaves the batch the frame it
        finishes.  batch_size (default: all): at most that many sequences are live; a waiting prompt is admitted into a running
        session at the first chunk boundary at which a row is free (admitting_session, admit_rows).  seeds: per-row sampler
        streams for the call, sequence b draws under seeds[b] (set_row_seeds).  Returns a list of (n_frames[b], 9) int32 id
        tensors (device), each bit-identical to the sequence's own B = 1 run — under top-k with seeds: its run under
        set_sampling(topk, T, seed=seeds[b]) — for any batch_size, on the default row-invariant plans.  The session may run more
        frames than log_frames: the log slot is rewound between calls (rewind_frame_log)."""
        B = len(prompts)
        assert len(n_frames) == B and (seeds is None or len(seeds) == B)
        st = self._st
        out = [[] for _ in range(B)]
        run = lambda n, rows: self.generate_frames(n, rows, mode, reason_eos, reason_card, skip_text_head=skip_text_head).clone()
        take = lambda b, log: out[b].append(log[:, 0])           # (None: nobody finishes before its count)
        admitting_session(self, rows_of=lambda b: [prompts[b]], n_utt=B, cap=B if batch_size is None else min(int(batch_size), B),
                          limit=[int(k) for k in n_frames], chunk=st["log_frames"], seeds=seeds, run=run, take=take)
        return [torch.cat(o) if o else torch.zeros(0, st["ncb"] + 1, dtype=torch.int32, device=st["device"]) for o in out]

    def begin_decode(self, tokens, tokens_mask, input_pos, forbid_prefix=0):
        """Loads the first decode frame (the last prompt frame, tts_task.py:253-255) into the device state."""
        self._need()
        B, W = tokens.shape[0], tokens.shape[-1]
        pos = input_pos.reshape(-1)
        if pos.numel() == 1:
            pos = pos.expand(B)
        lo, hi = int(pos.min().item()), int(pos.max().item())
        self._check_positions(lo)
        self._check_positions(hi)
        self._pos_hi = hi
        self._load_rows(tokens.reshape(B, W), tokens_mask.reshape(B, W), pos, torch.arange(B, device=tokens.device))
        self._st["forbid"][:B].fill_(int(forbid_prefix))

    # ---- beam search of the text loop (include/ua2hip.h ua2_beam_step / ua2_beam_reorder) -------------------------
    def _static_page_tables(self):
        """Sequence b owns pages [b * max_pages, (b + 1) * max_pages): the layout setup_caches starts from."""
        for g in (self.audio_understanding_expert, self.backbone, self.audio_generation_expert):
            pt = g.kv_cache.page_table
            pt.copy_(torch.arange(pt.numel(), dtype=torch.int32, device=pt.device).view_as(pt))

    def _beam_checks(self, W, G, max_length, no_repeat_ngram_size=0):
        st = self._st
        if no_repeat_ngram_size != 0 and not 2 <= no_repeat_ngram_size <= 16:
            raise ValueError(f"no_repeat_ngram_size of a beam search must be 0 (off) or in 2..16, got {no_repeat_ngram_size}")
        if not 1 <= W <= 8:
            raise ValueError(f"beam_width must be in 1..8, got {W}")
        if G * W > 64:
            raise ValueError(f"{G} prompts with beam_width={W} are {G * W} rows: a beam frame holds at most 64")
        if st["B"] < 2 * G * W:
            of = f"{G} prompts and " if G > 1 else ""
            raise ValueError(f"beam search with {of}beam_width={W} needs setup_caches(max_batch_size={2 * G * W}) or larger (the pages of "
                             f"sequences {G * W}..{2 * G * W - 1} are the second page set of the K/V fork); this plan holds {st['B']}")
        if max_length < 1:
            raise ValueError("max_length must be >= 1")
        if self._cfg > 1.0 or self._ngram is not None or (self._sampling is not None and self._sampling[0] != 1):
            raise ValueError("beam search runs without classifier-free guidance, without the n-gram filter and with topk = 1")
        if self._beam is not None:
            raise ValueError("a beam search is already running (end_beams)")

    def _attach_beams(self, W, G, length_penalty, max_length, eos_id, no_repeat_ngram_size=0):
        """The device state of G beams of W slots (include/ua2hip.h: group g at fixed strides from the base pointers), attached to
        the executor, and the start of the fork for the rows the caller has loaded: every slot of a group gets slot 0's pages.
        no_repeat_ngram_size >= 2: the two history sets of every group (ua2_beam_ngram: [G][2][8][max_length] ids) behind the log."""
        st = self._st
        dev = st["device"]
        # state: one int32 buffer carved into the fields of ua2_beam_state (score and cand_logp are fp32 views of their words)
        n_log = max_length * W * 4
        n_hist = 2 * 8 * max_length if no_repeat_ngram_size else 0
        words = torch.zeros(G * (4 * 8 + 4 + 2 * 64 + n_log + n_hist), dtype=torch.int32, device=dev)
        at = [0]

        def f(n):
            at[0] += n
            return words[at[0] - n:at[0]]
        score, fin, ln, parent, ctrl = f(8 * G).view(torch.float32), f(8 * G), f(8 * G), f(8 * G), f(4 * G)
        cand_logp, cand_id, log = f(64 * G).view(torch.float32), f(64 * G), f(G * n_log)
        hist = f(G * n_hist)
        score.fill_(float("-inf")); score[::8] = 0.0
        fin.fill_(2); fin[::8] = 0
        ctrl[1::4] = -1
        lp_inv = torch.tensor([1.0 / (((5 + n) / 6) ** float(length_penalty)) for n in range(max_length + 1)], dtype=torch.float64)
        lp_inv = lp_inv.to(torch.float32).to(dev)
        bs = BeamState(score.data_ptr(), fin.data_ptr(), ln.data_ptr(), parent.data_ptr(), ctrl.data_ptr(), cand_logp.data_ptr(),
                       cand_id.data_ptr(), log.data_ptr(), max_length, lp_inv.data_ptr(), max_length + 1)
        pools, tables = [], []
        esz = torch.empty(0, dtype=st["dtype"]).element_size()
        for ti, g in enumerate((self.audio_understanding_expert, self.backbone, self.audio_generation_expert)):
            kv, cfg = g.kv_cache, g.config
            tables.append(kv.page_table)
            if (cfg.head_size * esz) % 16:
                raise ValueError("beam search copies K/V in 16-byte units: head_size * element size must be a multiple of 16")
            pools += [BeamPool(t.data_ptr(), ti, cfg.n_query_groups, cfg.head_size * esz, 0) for t in kv.k + kv.v]
        raw = bytes((BeamPool * len(pools))(*pools))
        pools_dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        tabs = (vp * 3)(*[t.data_ptr() for t in tables])
        max_pages = self.backbone.kv_cache.max_pages
        self._beam = dict(W=W, G=G, cap=max_length, steps=0, eos=int(eos_id), words=words, score=score.view(G, 8), fin=fin.view(G, 8),
                          len=ln, ctrl=ctrl.view(G, 4), log=log.view(G, max_length, W, 4), lp_inv=lp_inv, pools=pools_dev, state=bs)
        check(lib.ua2_stage3_set_beam_groups(self._h, W, G, int(eos_id), C.byref(bs), pools_dev.data_ptr(), len(pools)),
              "ua2_stage3_set_beam_groups")
        if no_repeat_ngram_size:                     # (detaching the beam clears it: end_beams_groups)
            ng = BeamNgram(int(no_repeat_ngram_size), max_length, hist.data_ptr())
            check(lib.ua2_stage3_set_beam_ngram(self._h, C.byref(ng)), "ua2_stage3_set_beam_ngram")
        # the start of the fork: all parents slot 0 of their group, before the first frame (pos_add 0)
        check(lib.ua2_beam_reorder_groups(W, G, None, st["row_pos"].data_ptr(), 0, pools_dev.data_ptr(), len(pools), tabs, 3, st["B"],
                                          max_pages, ops.stream()), "ua2_beam_reorder_groups")

    @torch.inference_mode()
    def begin_beams(self, tokens, tokens_mask, beam_width: int = 5, length_penalty: float = 0.6, max_length: int = 500,
                    eos_id: int = 128001, no_repeat_ngram_size: int = 0):
        """Start of a beam search over one prompt: tokens (L, 9), tokens_mask (L, 9).  Prefills prompt[:-1] as sequence 0, loads the
        prompt's last frame into the W = beam_width rows of the decode state, attaches the beam state to the executor and gives every
        slot its view of the prompt's K/V (shared full pages, a copy of the partial one).  Slot 0 starts live with score 0, the others
        dead.  Run steps with generate_frames(n, W, 3); end_beams() must follow (beam_search does so in a `finally`).
        no_repeat_ngram_size = n in 2..16 (0 = off, the reference's behaviour): every step runs under the no-repeat-n-gram ban of
        DESIGN.md §2 — an id that would complete an n-gram the slot's text already holds counts as -inf before the softmax."""
        self._need()
        st = self._st
        W, max_length, ng = int(beam_width), int(max_length), int(no_repeat_ngram_size)
        self._beam_checks(W, 1, max_length, ng)
        dev = st["device"]
        tokens, tokens_mask = tokens.to(dev), tokens_mask.bool().to(dev)
        L = tokens.shape[0]
        self._check_positions(L - 1 + max_length - 1)
        self.reset_caches()
        self._static_page_tables()
        pos = torch.arange(0, L, device=dev).unsqueeze(0)
        self.forward_prefix(tokens[None, :-1], tokens_mask=tokens_mask[None], input_pos=pos[:, :-1])
        self.begin_decode(tokens[-1:].unsqueeze(0).repeat(W, 1, 1), tokens_mask[-1:].unsqueeze(0).repeat(W, 1, 1),
                          torch.tensor([L - 1], device=dev))
        self._attach_beams(W, 1, length_penalty, max_length, eos_id, ng)

    @torch.inference_mode()
    def begin_beams_groups(self, prompts, beam_width: int = 5, length_penalty: float = 0.6, max_length: int = 500, eos_id: int = 128001,
                           no_repeat_ngram_size: int = 0):
        """Start of G = len(prompts) beam searches in one frame: prompts[g] = (tokens (L_g, 9), mask (L_g, 9)) of any lengths.  Group
        g's slot j is row g * W + j.  Every prompt[:-1] is prefilled in one ragged pass, prompt g as sequence g * W (slot 0 of its
        group then owns the prompt's pages); each prompt's last frame is loaded into its group's W rows at position L_g - 1; one
        start fork gives every slot its view of its own prompt.  Run steps with generate_frames(n, G * W, 3); end_beams_groups()
        must follow.  no_repeat_ngram_size: as in begin_beams, every group under its own histories."""
        self._need()
        st = self._st
        W, G, max_length, ng = int(beam_width), len(prompts), int(max_length), int(no_repeat_ngram_size)
        if G < 1:
            raise ValueError("beam search over an empty list of prompts")
        self._beam_checks(W, G, max_length, ng)
        dev = st["device"]
        prompts = [(t.to(dev), m.bool().to(dev)) for t, m in prompts]
        Ls = [int(t.shape[0]) for t, _ in prompts]
        if min(Ls) < 1:
            raise ValueError("an empty prompt")
        self._check_positions(max(Ls) - 1 + max_length - 1)
        self.reset_caches()
        self._static_page_tables()
        pre = [g for g in range(G) if Ls[g] > 1]
        if pre:
            self.forward_prefix_ragged([prompts[g][0][:-1] for g in pre], [prompts[g][1][:-1] for g in pre], seq_ids=[g * W for g in pre])
        last_t = torch.stack([t[-1] for t, _ in prompts]).repeat_interleave(W, dim=0)
        last_m = torch.stack([m[-1] for _, m in prompts]).repeat_interleave(W, dim=0)
        pos = torch.tensor(Ls, device=dev).repeat_interleave(W) - 1
        self.begin_decode(last_t.unsqueeze(1), last_m.unsqueeze(1), pos)
        self._attach_beams(W, G, length_penalty, max_length, eos_id, ng)

    def beams_all_finished(self) -> int:
        """The step at which every slot of every group had first finished (the last group's latch), -1 while one is live.  One copy of
        the G ctrl records: the only thing the host reads between chunks."""
        done = self._beam["ctrl"][:, 1].cpu().tolist()
        return -1 if min(done) < 0 else max(done)

    @torch.inference_mode()
    def end_beams_groups(self):
        """End of the searches: reads the state and every group's step log, recovers every slot's text ids by walking the log
        backwards, restores the static page tables and detaches the beam state — a later greedy call behaves as if no search had
        happened.  Slots still live count as finished with their score unchanged.  Returns one (best ids, best score, hypotheses) per
        group with hypotheses = [dict(ids, score, finished)] in slot order; the best is the highest score, the first such slot on
        ties.  beam_info_groups[g] = dict(steps, all_finished) of group g."""
        bm, self._beam = self._beam, None
        try:
            if bm is None:
                raise ValueError("no beam search is running (begin_beams)")
            torch.cuda.synchronize()
            W, G = bm["W"], bm["G"]
            ctrl = bm["ctrl"].cpu().tolist()
            steps = [min(c[0], bm["cap"]) for c in ctrl]
            log = bm["log"][:, :max(steps)].cpu().numpy()
            score, fin = bm["score"][:, :W].cpu().tolist(), bm["fin"][:, :W].cpu().tolist()
        finally:
            if self._h is not None:
                check(lib.ua2_stage3_set_beam(self._h, 0, 0, None, None, 0), "ua2_stage3_set_beam")
                self._static_page_tables()
        # steps run; the step at which all slots of the group were first finished (-1: never)
        self.beam_info_groups = [dict(steps=steps[g], all_finished=ctrl[g][1]) for g in range(G)]
        self.beam_info = self.beam_info_groups[0]
        out = []
        for g in range(G):
            hyps = [dict(ids=backtrack_beam_log(log[g][:steps[g]], j), score=float(score[g][j]), finished=fin[g][j] == 1) for j in range(W)]
            best = max(range(W), key=lambda j: (hyps[j]["score"] if fin[g][j] != 2 else float("-inf"), -j))
            out.append((hyps[best]["ids"], hyps[best]["score"], hyps))
        return out

    @torch.inference_mode()
    def end_beams(self):
        """End of a beam search over one prompt (begin_beams): end_beams_groups for its one group.  Returns (best ids, best score,
        hypotheses); beam_info = dict(steps, all_finished)."""
        return self.end_beams_groups()[0]

    def _run_beams(self, rows, max_length, chunk_frames, use_graph, skip_audio_experts):
        try:
            done = 0
            while done < max_length:
                n = min(int(chunk_frames), max_length - done)
                self.generate_frames(n, rows, 3, use_graph=use_graph, skip_audio_experts=skip_audio_experts)
                done += n
                if self.beams_all_finished() >= 0:
                    break
        except BaseException:
            try:
                self.end_beams_groups()
            except Exception:
                pass
            raise
        return self.end_beams_groups()

    @torch.inference_mode()
    def beam_search(self, tokens, tokens_mask, beam_width: int = 5, length_penalty: float = 0.6, max_length: int = 500,
                    eos_id: int = 128001, early_stopping: bool = True, chunk_frames: int = 16, use_graph: bool = True,
                    skip_audio_experts: bool = True, no_repeat_ngram_size: int = 0):
        """Beam search over the text continuation of one prompt (the reference's evaluation/asr_task.py:438-576 rule,
        corrected).  tokens / tokens_mask (L, 9).  The W hypotheses run as the W rows of one frame; the search stops when all W are
        finished or after max_length steps.  With all W finished a further step reproduces the beam, so the result does not depend on
        chunk_frames, and stopping there is what early_stopping=False would compute as well (the reference keeps looping over
        finished beams without changing them).  no_repeat_ngram_size = n in 2..16 runs every step under the no-repeat-n-gram ban
        (begin_beams; 0, the default, bans nothing, as the reference does).  Returns (best ids, best score, all W hypotheses)."""
        self.begin_beams(tokens, tokens_mask, beam_width, length_penalty, max_length, eos_id, no_repeat_ngram_size)
        return self._run_beams(int(beam_width), int(max_length), chunk_frames, use_graph, skip_audio_experts)[0]

    @torch.inference_mode()
    def beam_search_batch(self, prompts, beam_width: int = 5, length_penalty: float = 0.6, max_length: int = 500, eos_id: int = 128001,
                          chunk_frames: int = 16, use_graph: bool = True, skip_audio_experts: bool = True, no_repeat_ngram_size: int = 0):
        """Beam search over several prompts at once: prompts[g] = (tokens (L_g, 9), mask (L_g, 9)); G * beam_width <= 64 rows, a plan
        of 2 * G * beam_width sequences.  The G beams are the row groups of one frame, so G searches cost about one
        search's frames.  Group g's result is what beam_search returns for prompts[g] alone — on the default (row-invariant) plan bit
        for bit: a group that has finished keeps being stepped as a fixed point beside the live ones, and the loop stops when every
        group has latched or after max_length steps.  no_repeat_ngram_size: as in beam_search, for every group.  Returns
        [(best ids, best score, hypotheses)] in the order of prompts."""
        prompts = list(prompts)
        if not prompts:
            raise ValueError("beam_search_batch needs at least one prompt")
        self.begin_beams_groups(prompts, beam_width, length_penalty, max_length, eos_id, no_repeat_ngram_size)
        return self._run_beams(len(prompts) * int(beam_width), int(max_length), chunk_frames, use_graph, skip_audio_experts)

    def buffer(self, name: str, rows: int):
        """Intermediate buffers for tests: 'h_final' (rows, C), 'text_logits' (rows, Vt), 'audio_logits' (rows, 8, Va)."""
        self._need()
        st = self._st
        p = lib.ua2_stage3_buffer(self._h, name.encode())
        if not p:
            raise KeyError(name)
        Cb = self.backbone.config.n_embd
        shape = {"h_final": (rows, Cb), "h": (rows, Cb), "text_logits": (rows, self.backbone.config.padded_vocab_size),
                 "audio_logits": (rows, st["ncb"], st["va"])}[name]
        base = st["scratch"]
        off = (C.cast(p, C.c_void_p).value - base.data_ptr()) // 4
        n = 1
        for s_ in shape:
            n *= s_
        return base[off:off + n].view(shape)

    def get_fsdp_wrap_module_list(self) -> List[nn.Module]:
        return (list(self.backbone.transformer.h) + list(self.audio_understanding_expert.transformer.h) +
                list(self.audio_generation_expert.transformer.h))
