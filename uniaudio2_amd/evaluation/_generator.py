"""Task generators of the decode loop, host side: prompt layout, prefill, frame loop, EOS / phase logic.

Mirror of the reference's evaluation/*_task.py `Generator` classes (tts_task.py:53-285 and its
audiogen / musicgen / songen twins, which differ only in the special-token key; asr_task.py
prepare_asr_task :299-326, generate_asr :630-688; audio_understanding.py get_condition_seq :233-282,
generate_answer :284-339).  Same constructor, attributes, method names, argument meaning and return
values: (8, T) int32 reason / semantic tensors with the semantic offset removed and the first frame of
each phase dropped (tts_task.py:271,283-284), or the decoded text.

What differs is where the loop runs: the reference calls `generate_frame` from Python and
synchronises twice per frame to test EOS (tts_task.py:261,263); here frames run on the device in
chunks (`Model_stage3.generate_frames`: hipGraph replay, feedback and the reason_eos ->
forbid_prefix switch on device) and the host reads the id log once per chunk.  Frames computed past
the EOS frame are discarded, so the returned ids are those of the reference's loop.
"""
from typing import Tuple

import os

import torch

from ..llm_models.model_new import admitting_session

SPECIAL_TOKENS = {'<think>': 128002, '</think>': 128003, '</answer>': 128005,
                  '<transcription>': 128011, '</transcription>': 128012, '<lyric>': 128013,
                  '</lyric>': 128014, '<caption>': 128015, '</caption>': 128016, '<answer>': 128017,
                  '<reason_token>': 128018, '<semantic_token>': 128019}
TEXT_EOS = 128001            # evaluation/asr_task.py:674


class PhaseSplitter:
    """Host-side bookkeeping of the generation loop (tts_task.py:253-284), one frame at a time:
    stop at the semantic EOS frame, switch from the reason phase to the semantic phase at the
    reason EOS frame (which is not stored), strip the semantic offset, drop the first stored frame of
    each phase when stacking."""

    def __init__(self, reason_eos, semantic_eos, reason_card):
        self.reason_eos, self.sem_eos, self.reason_card = reason_eos, semantic_eos + reason_card, reason_card
        self.is_reason, self.save_flag, self.done = True, True, False
        self.pre_reason, self.pre_sem = [], []

    def push(self, audio):
        """audio: (1, 8) int tensor of one frame (conditional row).  Returns False once generation is over."""
        if self.done:
            return False
        if torch.all(audio == self.sem_eos):
            self.done = True
            return False
        if torch.all(audio == self.reason_eos):
            self.is_reason, self.save_flag = False, False
        if self.save_flag:
            if self.is_reason:
                self.pre_reason.append(audio)
            else:
                self.pre_sem.append(audio - self.reason_card)
        else:
            self.save_flag = True
        return True

    def result(self):
        if len(self.pre_reason) < 2 or len(self.pre_sem) < 2:
            from ..parallel import GenerationFailed
            raise GenerationFailed("stack expects a non-empty TensorList: the model produced no reason/semantic frames "
                                   "(same failure as the reference's torch.stack at tts_task.py:283-284)")
        de_reason = torch.stack(self.pre_reason[1:]).permute(1, 2, 0).squeeze(0)      # (8, T_r)
        de_sem = torch.stack(self.pre_sem[1:]).permute(1, 2, 0).squeeze(0)
        return de_reason, de_sem


class GeneratorBase:
    chunk_frames = 16        # frames per device-side chunk between host EOS checks
    # The audio-feedback loops never read the text id a frame samples (tts_task.py:259 appends it to a list nobody uses, :274-277
    # feed it back under text_mask = False): the on-device loop skips lm_head + its sample there (ua2hip.h
    # UA2_FRAME_SKIP_TEXT_HEAD; identical (reason, semantic)).  UA2_KEEP_TEXT_HEAD=1 computes it as the reference does.
    skip_text_head = os.environ.get("UA2_KEEP_TEXT_HEAD") is None
    # Nucleus (top-p) filter of every sampled loop (CLI --top_p; llm_utils/sampling.py:66-82): 0.0 = off.  It applies where the loop
    # samples (topk > 1): the audio loops, single and batched (row seeds, admission, guided pairs), and the text loops; greedy loops
    # ignore it.  Pure nucleus sampling is topk = the audio vocabulary width.
    top_p = 0.0
    # Repetition penalty of every sampled loop (CLI --repetition_penalty / --repetition_window; Model_stage3.set_repetition_penalty; not in
    # the reference, effect on audio quality not measured): 1.0 = off.  It applies where top_p does; greedy loops and beam search ignore it.
    repetition_penalty = 1.0
    repetition_window = 64

    def __init__(self, model, train_args, audio_tokenizer_config=None, audio_model_path=None,
                 text_tokenizer_path=None, is_cfg=False):
        from ..tools.tokenizer.Text2ID.text_tokenizer import load_text_tokenizer
        self._model = model
        self.is_cfg = is_cfg
        self._model.setup_caches(2 if is_cfg else 1)          # tts_task.py:64-67
        self._text_tokenizer = load_text_tokenizer(text_tokenizer_path)
        # the reference also loads the audio codec here (tts_task.py:71); generation never calls it,
        # so it is created lazily by the CLI stages that need it
        self._audio_tokenizer = None
        self.device = next(model.parameters()).device
        self.sample_rate = 24000
        self.empty_token = 0
        for k in ("text_pad_token", "semantic_pad_token", "semantic_eos", "semantic_bos", "reason_eos", "reason_bos",
                  "reason_pad_token", "parallel_number", "audio_reason_card"):
            setattr(self, k, getattr(train_args, k))
        self.audio_prompt_bos = getattr(train_args, "audio_prompt_bos", None)
        self.audio_prompt_eos = getattr(train_args, "audio_prompt_eos", None)
        self.special_token_dict = self.get_special_token()

    def get_special_token(self):
        return dict(SPECIAL_TOKENS)

    # ---- prompt layout ((T, 9) frames: 8 audio streams + 1 text stream, with masks) ------------
    def text_pad(self, x):
        seq = torch.zeros((len(x), self.parallel_number), dtype=torch.int64)
        seq[:, -1] = x
        seq[:, :-1] = self.empty_token
        return seq

    def audio_pad(self, x):
        seq = torch.full((x.shape[0], self.parallel_number), self.empty_token, dtype=torch.int64)
        seq[:, :-1] = x
        return seq

    def add_offset_semantic(self, x, offset_value):
        return x + offset_value

    def add_special_token(self, key, this_data):
        if key.startswith('text_seq'):
            return this_data
        key = key.replace('_seq', '')
        bos = torch.ones(1) * self.special_token_dict['<' + key + '>']
        eos = torch.ones(1) * self.special_token_dict['</' + key + '>']
        return torch.cat([bos, this_data, eos], dim=0)

    def reason_seq_bos_eos(self, d):
        bos = torch.ones(1, d.shape[1]) * self.reason_bos
        eos = torch.ones(1, d.shape[1]) * self.reason_eos
        return torch.cat([bos, d, eos], dim=0)

    def semantic_seq_bos_eos(self, d):
        bos = torch.ones(1, d.shape[1]) * self.semantic_bos
        eos = torch.ones(1, d.shape[1]) * self.semantic_eos
        return self.add_offset_semantic(torch.cat([bos, d, eos], dim=0), self.audio_reason_card)

    def _text_block(self, data):
        data = self.text_pad(data)
        mask = torch.zeros((data.shape[0], self.parallel_number))
        mask[:, -1] = True
        return data, mask

    def _audio_block(self, data):
        data = self.audio_pad(data)
        mask = torch.zeros((data.shape[0], self.parallel_number))
        mask[:, :-1] = True
        return data, mask

    def _prepare_text_conditioned(self, task_prompt, text_seq, key, cfg=False):
        """prepare_tts_task / prepare_tts_task_for_cfg and twins (tts_task.py:175-205)."""
        text_seq = self.add_special_token(key, text_seq)
        if cfg:
            task_prompt = torch.ones_like(task_prompt) * self.text_pad_token
            text_seq = torch.ones_like(text_seq) * self.text_pad_token
        pd, pm = self._text_block(task_prompt)
        td, tm = self._text_block(text_seq)
        return torch.cat([pd, td], dim=0), torch.cat([pm, tm], dim=0)

    def prepare_asr_task(self, task_prompt, this_reason_data, this_semantic_data):
        """asr_task.py:299-326: prompt text frames, then [reason_bos, reason.., reason_eos] and
        [sem_bos, sem.., sem_eos] (+ reason_card) audio frames."""
        td, tm = self._text_block(task_prompt)
        audio = torch.cat([self.reason_seq_bos_eos(this_reason_data), self.semantic_seq_bos_eos(this_semantic_data)], dim=0)
        ad, am = self._audio_block(audio)
        return torch.cat([td, ad], dim=0), torch.cat([tm, am], dim=0)

    def get_condition_seq(self, d, keys, types, task_prompt_data):
        """audio_understanding.py:233-282."""
        sequence, mask = [], []
        data, m = self._text_block(task_prompt_data)
        sequence.append(data); mask.append(m)
        for key, tp in zip(keys, types):
            if tp == 'text':
                data, m = self._text_block(self.add_special_token(key, d[key]))
            else:
                this = d[key].transpose(0, 1).long()
                if tp == 'audio_prompt':
                    this = self.semantic_seq_bos_eos(this)
                    bos = torch.ones(1, this.shape[1]) * self.audio_prompt_bos
                    eos = torch.ones(1, this.shape[1]) * self.audio_prompt_eos
                    this = torch.cat([bos, this[1:-1, :], eos], dim=0)
                elif key.startswith('reason_seq'):
                    this = self.reason_seq_bos_eos(this)
                else:
                    this = self.semantic_seq_bos_eos(this)
                data, m = self._audio_block(this)
            sequence.append(data); mask.append(m)
        return torch.cat(sequence, dim=0).to(torch.int64), torch.cat(mask, dim=0)

    # ---- loops ----------------------------------------------------------------------------------
    def _set_sampling(self, topk, temperature):
        self._model.set_sampling(topk, temperature)
        # nucleus filter (Model_stage3.set_top_p): the model hears of it only while it is on, and once more to turn it off
        top_p = float(self.top_p)
        if top_p != 0.0 or getattr(self, "_top_p_set", 0.0) != 0.0:
            self._model.set_top_p(top_p)
            self._top_p_set = top_p
        # repetition penalty (Model_stage3.set_repetition_penalty): the same rule
        rep = (float(self.repetition_penalty), int(self.repetition_window))
        if rep[0] != 1.0 or getattr(self, "_rep_set", (1.0, 64))[0] != 1.0:
            self._model.set_repetition_penalty(*rep)
            self._rep_set = rep

    def _prefill(self, rows_tokens, rows_mask):
        """rows_*: list of (L, 9) prompts of equal length (1, or 2 with CFG; tts_task.py:228-245)."""
        dev = self.device
        tok = torch.stack(rows_tokens).to(dev)
        msk = torch.stack(rows_mask).bool().to(dev)
        B, L, _ = tok.shape
        pos = torch.arange(0, L, device=dev).unsqueeze(0).repeat(B, 1)
        self._model.reset_caches()
        self._model.forward_prefix(tok[:, :-1], labels=tok[:, 1:, :-1], tokens_mask=msk, loss_mask=msk,
                                   input_pos=pos[:, :-1])
        self._model.begin_decode(tok[:, -1:], msk[:, -1:], torch.tensor([L - 1], device=dev))
        return B, L

    @torch.inference_mode()
    def score_continuation(self, tokens, tokens_mask, cont_tokens, cont_mask):
        """Teacher-forced score of a given continuation under a prompt: tokens / tokens_mask (L, 9) as the prepare_* methods build
        the prompt, cont_tokens / cont_mask (T, 9) the frames to score (a reference transcript as _text_block lays it out, a
        reference token file as _audio_block does).  The loss mask covers the continuation only.  Returns Model_stage3.score_sequence's
        dict for the one sequence: row s of nll / pred (1, L + T - 1, 9) scores frame s + 1, so the continuation's rows are [L - 1:]."""
        dev = self.device
        tok = torch.cat([tokens, cont_tokens], dim=0).to(torch.int64).to(dev)
        msk = torch.cat([tokens_mask, cont_mask], dim=0).bool().to(dev)
        loss = torch.zeros_like(msk)
        loss[tokens.shape[0]:] = True
        return self._model.score_sequence(tok[None], msk[None], loss[None])

    @torch.inference_mode()
    def _generate_audio_tokens(self, tokens, tokens_mask, cfg_tokens=None, cfg_mask=None, topk=1, temperature=1.0,
                               max_audio_frames=500) -> Tuple[torch.Tensor, torch.Tensor]:
        """The loop of generate_tts / generate_audio / generate_LTS (tts_task.py:246-285)."""
        rows_t, rows_m = [tokens], [tokens_mask]
        if self.is_cfg:
            rows_t.append(cfg_tokens); rows_m.append(cfg_mask)
        B, L = self._prefill(rows_t, rows_m)
        self._set_sampling(topk, temperature)
        ph = PhaseSplitter(self.reason_eos, self.semantic_eos, self.audio_reason_card)
        frame = 0
        while not ph.done and frame < max_audio_frames:
            n = min(self.chunk_frames, max_audio_frames - frame)
            log = self._model.generate_frames(n, B, 2 if self.is_cfg else 0, reason_eos=self.reason_eos,
                                              reason_card=self.audio_reason_card, max_pos=L + max_audio_frames,
                                              skip_text_head=self.skip_text_head).cpu()       # (n, B, 9)
            for f in range(n):
                if not ph.push(log[f, 0:1, 1:]):                      # conditional row only (tts_task.py:256-258)
                    break
            frame += n
        de_reason, de_sem = ph.result()
        return de_reason.to(self.device), de_sem.to(self.device)

    def _size_plan(self, prompts, cap, per, frames):
        """The model's plan for a batched session: `cap` live utterances of `per` rows each, the ragged prefill of the first `cap`
        prompts (at most 8192 rows a pass) and a frame log for the `frames` one utterance may run.  A plan that is large enough is kept."""
        st = getattr(self._model, "_st", None)
        need_rows = per * sum(int(t.shape[0]) - 1 for t, _ in prompts[:cap])
        if st is None or st["B"] < per * cap or st["max_rows"] < min(need_rows, 8192) or st["log_frames"] < frames:
            self._model.setup_caches(per * cap, max_rows=max(64, min(need_rows, 8192)), log_frames=max(512, frames))

    @torch.inference_mode()
    def _generate_audio_tokens_batch(self, prompts, topk=1, temperature=1.0, max_audio_frames=500, cfg_prompts=None, seeds=None,
                                     batch_size=None):
        """Many utterances at once on one GPU (the reference loops over them one by one,
        multi_task_inference.py:510): prompts = [(tokens (L_b, 9), mask (L_b, 9)), ...] of any lengths.  One ragged prefill,
        then all sequences decode together in device-side chunks (model_new.admitting_session is the loop); after each
        chunk the host runs every sequence's own phase / EOS bookkeeping (the same PhaseSplitter as the single-utterance
        loop) and retires the finished ones.
        batch_size (default: all): at most that many utterances are live; a waiting one is admitted into the running session
        (Model_stage3.admit_rows) at the first chunk boundary at which a row is free, and runs its own max_audio_frames.
        seeds: one sampler key per utterance (Model_stage3.set_row_seeds) — utterance b then draws what its own single run
        draws under set_sampling(topk, temperature, seed=seeds[b]), whatever shares its batch.  Greedy results, and sampled
        ones under seeds, equal the one-by-one results bit for bit (row invariance).
        With `is_cfg` (the reference's --use_cfg: an unconditional twin of every prompt, tts_task.py:228-245) utterance b
        occupies a row PAIR (conditional, unconditional): guidance mixes inside a pair (model_new.py:618-622,634-637), both
        rows continue from the pair's conditional sample (tts_task.py:278-280) and share the utterance's key, the bookkeeping
        reads the conditional row, and an utterance admits and retires both of its rows.
        Returns one slot per utterance, in input order: (reason, semantic), or — for an utterance whose generation failed
        (PhaseSplitter.result) — the GenerationFailed instance; its batch-mates are not affected.  A call in which EVERY utterance
        failed raises the first failure, as the single-utterance loop does."""
        from ..parallel import GenerationFailed
        per = 2 if self.is_cfg else 1
        if self.is_cfg:
            if cfg_prompts is None or len(cfg_prompts) != len(prompts):
                raise ValueError("is_cfg: one unconditional prompt per prompt (prepare_*_for_cfg) is needed")
            for (t, _), (ct, _) in zip(prompts, cfg_prompts):
                if t.shape != ct.shape:
                    raise ValueError("a prompt and its unconditional twin must have the same shape")
        n_utt = len(prompts)
        if seeds is not None and len(seeds) != n_utt:
            raise ValueError(f"one seed per utterance: got {len(seeds)} seeds for {n_utt} utterances")
        if n_utt == 0:
            return []
        cap = n_utt if batch_size is None else max(1, min(int(batch_size), n_utt))      # live utterances
        rows_of = lambda b: [(t, m.bool()) for t, m in ([prompts[b], cfg_prompts[b]] if self.is_cfg else [prompts[b]])]
        self._size_plan(prompts, cap, per, max_audio_frames)
        longest = max(int(t.shape[0]) for t, _ in prompts)
        splitters = [PhaseSplitter(self.reason_eos, self.semantic_eos, self.audio_reason_card) for _ in range(n_utt)]
        run = lambda n, rows: self._model.generate_frames(n, rows, 2 if self.is_cfg else 0, reason_eos=self.reason_eos,
                                                          reason_card=self.audio_reason_card, max_pos=longest + max_audio_frames,
                                                          skip_text_head=self.skip_text_head).cpu()       # (n, rows, 9)

        def take(b, log):                                            # the utterance's conditional row (tts_task.py:256-258)
            for f in range(log.shape[0]):
                if not splitters[b].push(log[f, 0:1, 1:]):
                    break
            return splitters[b].done
        admitting_session(self._model, rows_of=rows_of, n_utt=n_utt, cap=cap, limit=[max_audio_frames] * n_utt, chunk=self.chunk_frames,
                          seeds=seeds, run=run, take=take, start=lambda: self._set_sampling(topk, temperature))
        out = []
        for ph in splitters:
            try:
                de_reason, de_sem = ph.result()
                out.append((de_reason.to(self.device), de_sem.to(self.device)))
            except GenerationFailed as e:
                out.append(e)
        if all(isinstance(o, GenerationFailed) for o in out):       # nothing succeeded: there is no batch-mate to protect, the call fails as it always has
            raise out[0]
        return out

    def _batch_twin(self, prepare, prepare_cfg, inputs, topk, temperature, seeds, batch_size):
        """The body of every generate_*_batch: inputs[b] = the arguments of the task's prepare_* methods for utterance b."""
        prompts = [prepare(*a) for a in inputs]
        cfg = [prepare_cfg(*a) for a in inputs] if self.is_cfg else None
        return self._generate_audio_tokens_batch(prompts, topk=topk, temperature=temperature, cfg_prompts=cfg, seeds=seeds, batch_size=batch_size)

    @torch.inference_mode()
    def _generate_text(self, tokens, tokens_mask, topk=1, temperature=1.0, max_frames=500, no_repeat_ngram_size=0,
                       ngram_fallback=128000) -> str:
        """The loop of generate_asr / generate_audio_caption / generate_answer (asr_task.py:658-688).
        no_repeat_ngram_size >= 2: the loop of generate_asr_with_ngram_sampling (asr_task.py:359-400) — every frame's text id
        that would repeat an n-gram of the ids generated so far becomes `ngram_fallback`, on the device (Model_stage3.set_ngram);
        the filter is on for this loop only."""
        B, L = self._prefill([tokens], [tokens_mask])
        self._set_sampling(topk, temperature)
        if no_repeat_ngram_size > 1:
            self._model.set_ngram(no_repeat_ngram_size, ngram_fallback, capacity=max_frames)
            try:
                return self._text_loop(L, max_frames)
            finally:
                self._model.set_ngram(0)
        return self._text_loop(L, max_frames)

    @torch.inference_mode()
    def _beam_search_text(self, tokens, tokens_mask, beam_width, length_penalty, early_stopping, max_length, no_repeat_ngram_size=0) -> str:
        """The loop of generate_asr_beam_search (asr_task.py:438-576) on the device: Model_stage3.beam_search.
        no_repeat_ngram_size >= 2: under the no-repeat-n-gram ban (the model is called as before when it is 0)."""
        beam_width = int(beam_width)
        ngram = dict(no_repeat_ngram_size=int(no_repeat_ngram_size)) if no_repeat_ngram_size else {}
        if not 1 <= beam_width <= 8:
            raise ValueError(f"beam_width must be in 1..8, got {beam_width}")
        st = getattr(self._model, "_st", None)
        if st is not None and st["B"] < 2 * beam_width:       # the K/V fork keeps a second page set: 2 W sequences
            self._model.setup_caches(2 * beam_width)
        self._set_sampling(1, 1.0)
        ids, _, _ = self._model.beam_search(tokens, tokens_mask.bool(), beam_width=beam_width, length_penalty=length_penalty,
                                            max_length=max_length, eos_id=TEXT_EOS, early_stopping=early_stopping,
                                            chunk_frames=self.chunk_frames,
                                            skip_audio_experts=os.environ.get("UA2_KEEP_AUDIO_EXPERTS") is None, **ngram)
        return self._text_tokenizer.decode(torch.tensor(ids, dtype=torch.long))

    @torch.inference_mode()
    def _beam_search_text_batch(self, prompts, beam_width, length_penalty, max_length, no_repeat_ngram_size=0):
        """generate_asr_beam_search over several prompts in one frame: Model_stage3.beam_search_batch.  prompts = [(tokens, mask)].
        no_repeat_ngram_size: as in _beam_search_text."""
        beam_width, G = int(beam_width), len(prompts)
        ngram = dict(no_repeat_ngram_size=int(no_repeat_ngram_size)) if no_repeat_ngram_size else {}
        if not 1 <= beam_width <= 8:
            raise ValueError(f"beam_width must be in 1..8, got {beam_width}")
        if G < 1:
            raise ValueError("beam search over an empty list of utterances")
        if G * beam_width > 64:
            raise ValueError(f"{G} utterances with beam_width={beam_width} are {G * beam_width} rows: a beam frame holds at most 64")
        st = getattr(self._model, "_st", None)
        if st is not None and st["B"] < 2 * G * beam_width:   # two page sets of G * W rows each
            self._model.setup_caches(2 * G * beam_width)
        self._set_sampling(1, 1.0)
        out = self._model.beam_search_batch([(t, m.bool()) for t, m in prompts], beam_width=beam_width, length_penalty=length_penalty,
                                            max_length=max_length, eos_id=TEXT_EOS, chunk_frames=self.chunk_frames,
                                            skip_audio_experts=os.environ.get("UA2_KEEP_AUDIO_EXPERTS") is None, **ngram)
        return [self._text_tokenizer.decode(torch.tensor(ids, dtype=torch.long)) for ids, _, _ in out]

    @torch.inference_mode()
    def _generate_text_batch(self, prompts, topk=1, temperature=1.0, max_frames=500, no_repeat_ngram_size=0, ngram_fallback=128000,
                             seeds=None, batch_size=None):
        """_generate_text for many utterances at once — the text twin of _generate_audio_tokens_batch (the reference decodes them one
        by one, multi_task_inference.py:300-382): prompts = [(tokens (L_b, 9), mask (L_b, 9)), ...] of any lengths.  One ragged
        prefill, then all live rows decode together in text-feedback chunks of `chunk_frames` (model_new.admitting_session); after
        each chunk the host scans every live row's text column up to its first TEXT_EOS, exactly as _text_loop does, and retires
        the rows that met it or have run their max_frames.  batch_size (default: all): at most that many utterances are live; a
        waiting one is admitted into the running session (Model_stage3.admit_rows) at the first chunk boundary at which a row is free.
        max_frames: an int, or one int per utterance.  no_repeat_ngram_size >= 2: the device n-gram filter is on for the call, every
        row against its own history (capacity: the largest max_frames; an admitted row starts with an empty one).  seeds: one
        sampler key per utterance (Model_stage3.set_row_seeds) — utterance b then draws what its own _generate_text draws under
        set_sampling(topk, temperature, seed=seeds[b]), whatever shares its batch.  Greedy and n-gram-filtered texts, and sampled
        ones under seeds, equal the one-by-one texts (row invariance).  Returns the decoded texts in input order."""
        n_utt = len(prompts)
        if seeds is not None and len(seeds) != n_utt:
            raise ValueError(f"one seed per utterance: got {len(seeds)} seeds for {n_utt} utterances")
        limit = [int(max_frames)] * n_utt if isinstance(max_frames, int) else [int(x) for x in max_frames]
        if len(limit) != n_utt:
            raise ValueError(f"max_frames: one int, or one per utterance; got {len(limit)} for {n_utt} utterances")
        if n_utt == 0:
            return []
        if min(limit) < 1:
            raise ValueError(f"max_frames must be >= 1 for every utterance, got {min(limit)}")
        cap = n_utt if batch_size is None else max(1, min(int(batch_size), n_utt))      # live utterances = rows of the plan
        longest, most = max(int(t.shape[0]) for t, _ in prompts), max(limit)
        self._size_plan(prompts, cap, 1, most)
        ngram = no_repeat_ngram_size > 1
        text = [[] for _ in range(n_utt)]
        # text-only continuation: see _text_loop.  The frame after the prefill, and the one after every admission, run whole
        skip = os.environ.get("UA2_KEEP_AUDIO_EXPERTS") is None
        run = lambda n, rows: self._model.generate_frames(n, rows, 1, max_pos=longest + most, skip_audio_experts=skip).cpu()   # (n, rows, 9)

        def take(b, log):                                            # as _text_loop: the row's text column up to its first TEXT_EOS
            for t in log[:, 0, 0].tolist():
                if t == TEXT_EOS:
                    return True
                text[b].append(t)
            return False

        def start():
            self._set_sampling(topk, temperature)
            if ngram:
                self._model.set_ngram(no_repeat_ngram_size, ngram_fallback, capacity=max(most, 1))
        try:
            admitting_session(self._model, rows_of=lambda b: [(prompts[b][0], prompts[b][1].bool())], n_utt=n_utt, cap=cap, limit=limit,
                              chunk=self.chunk_frames, seeds=seeds, run=run, take=take, start=start)
        finally:
            if ngram:
                self._model.set_ngram(0)
        return [self._text_tokenizer.decode(torch.tensor(ids, dtype=torch.long)) for ids in text]

    def _text_twin(self, prepare, inputs, **kw):
        """The body of every batched text method: inputs[b] = the arguments of the task's prepare_* method for utterance b."""
        return self._generate_text_batch([prepare(*a) for a in inputs], **kw)

    def _text_loop(self, L, max_frames):
        text, frame, done = [], 0, False
        while not done and frame < max_frames:
            n = min(self.chunk_frames, max_frames - frame)
            # text-only continuation: from its second frame on the understanding / generation experts are dead code (their outputs are
            # masked out and their caches never read again: UA2_FRAME_SKIP_AUDIO_EXPERTS, identical text ids; UA2_KEEP_AUDIO_EXPERTS=1 runs them)
            log = self._model.generate_frames(n, 1, 1, max_pos=L + max_frames,
                                              skip_audio_experts=os.environ.get("UA2_KEEP_AUDIO_EXPERTS") is None).cpu()
            for f in range(n):
                t = int(log[f, 0, 0])
                if t == TEXT_EOS:
                    done = True
                    break
                text.append(t)
            frame += n
        return self._text_tokenizer.decode(torch.tensor(text, dtype=torch.long))
