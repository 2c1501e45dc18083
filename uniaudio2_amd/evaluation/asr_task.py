"""Mirror of the reference's evaluation/asr_task.py `Generator`: greedy `generate_asr`, the n-gram-constrained
`generate_asr_with_ngram_sampling` (:329-432) and `generate_asr_beam_search` (:438-576) — the last as a working restatement of the
rule the reference wrote down: its own function calls a method Model_stage3 lacks (:593) and cannot run."""
import torch

from ._generator import GeneratorBase


class Generator(GeneratorBase):
    # The opt-in of the beam search's no-repeat-n-gram ban (an extension).  False: `no_repeat_ngram_size` is accepted and has no
    # effect, exactly as in the reference.  True: generate_asr_beam_search[_batch] hand it to the device search.  An
    # attribute and not a parameter: generate_asr_beam_search keeps the reference's parameter list to the letter.
    enforce_ngram = False

    def _enforced_ngram(self, no_repeat_ngram_size) -> int:
        """The n the beam search bans with: 0 unless enforce_ngram is set."""
        if not self.enforce_ngram:
            return 0
        n = int(no_repeat_ngram_size)
        if n != 0 and not 2 <= n <= 16:
            raise ValueError(f"enforce_ngram: no_repeat_ngram_size must be 0 (off) or in 2..16, got {n}")
        return n

    @torch.inference_mode()
    def generate_asr(self, task_prompt, task_name, text_token=None, semantic_token=None, reason_token=None,
                     temperature: float = 0.9, topk: int = 200, cfg_scale=1.0) -> str:
        """reason_token (T_r, 8), semantic_token (T_s, 8) long -> transcription text (asr_task.py:630-688)."""
        tokens, mask = self.prepare_asr_task(task_prompt, reason_token, semantic_token)
        return self._generate_text(tokens, mask, topk=topk, temperature=temperature)

    @torch.inference_mode()
    def generate_asr_with_ngram_sampling(self, task_prompt, task_name, text_token=None, semantic_token=None, reason_token=None,
                                         temperature: float = 0.9, topk: int = 200, cfg_scale=1.0, no_repeat_ngram_size: int = 3,
                                         repetition_penalty: float = 1.2, *, fallback_token: int = 128000) -> str:
        """asr_task.py:329-405: the generate_asr loop where a text id that would repeat an n-gram of the ids generated so far
        (`no_repeat_ngram_size`; the prompt is not part of the history) is replaced by the fixed id `fallback_token` (128000 in
        the reference, _get_fallback_token :417-421), which is fed back and enters the history; the loop stops at EOS (128001),
        which therefore is never banned.  The filter runs on the device between the text sample and the feedback
        (Model_stage3.set_ngram).  `repetition_penalty` is unused, as in the reference.  no_repeat_ngram_size <= 1 bans nothing
        (the reference's n == 1 never finds a banned id either) and runs the plain loop.
        One departure: the reference prefills with the training forward `self._model(...)` (:356), which passes no positions to the
        two experts and so never fills their KV caches — its first frame then attends to zeroed expert K/V.  Here the prefill is
        generate_asr's (forward_prefix), so the n-gram loop decodes from the same state as the greedy one."""
        tokens, mask = self.prepare_asr_task(task_prompt, reason_token, semantic_token)
        return self._generate_text(tokens, mask, topk=topk, temperature=temperature, no_repeat_ngram_size=no_repeat_ngram_size,
                                   ngram_fallback=fallback_token)

    @torch.inference_mode()
    def generate_asr_beam_search(self, task_prompt, task_name, text_token=None, semantic_token=None, reason_token=None,
                                 beam_width: int = 5, length_penalty: float = 0.6, no_repeat_ngram_size: int = 3,
                                 early_stopping: bool = True, max_length: int = 500) -> str:
        """asr_task.py:438-576 with the reference's parameter names, order and defaults; returns the decoded text of the best
        hypothesis.  The search rule is the reference's: per live hypothesis the beam_width most probable next ids,
        score += log p / ((5 + length) / 6) ** length_penalty, EOS (128001) finishes a hypothesis without entering its text, the
        beam_width best candidates survive, the search ends when all are finished or after max_length steps, the highest score
        wins.  It runs on the device: the hypotheses are the rows of one frame and fork their K/V page-wise
        (Model_stage3.beam_search; the plan is re-made for 2 * beam_width sequences when it is smaller).
        `no_repeat_ngram_size` is accepted and has no effect, exactly as in the reference, whose `_apply_ngram_constraint`
        (:610-628) bans an always-empty set.  With the attribute enforce_ngram = True (an extension) it does what that function was
        meant to do: every step runs under the no-repeat-n-gram ban of DESIGN.md §2 on the device (no_repeat_ngram_size in 2..16;
        an id that would complete an n-gram the hypothesis already holds counts as -inf before the softmax).  As for
        generate_asr_with_ngram_sampling the prefill is generate_asr's (forward_prefix of prompt[:-1]), not the reference's
        training-mode forward (:476)."""
        tokens, mask = self.prepare_asr_task(task_prompt, reason_token, semantic_token)
        return self._beam_search_text(tokens, mask, beam_width, length_penalty, early_stopping, max_length,
                                      self._enforced_ngram(no_repeat_ngram_size))

    @torch.inference_mode()
    def generate_asr_beam_search_batch(self, task_prompt, task_name, reason_tokens, semantic_tokens, beam_width: int = 5,
                                       length_penalty: float = 0.6, max_length: int = 500, *, no_repeat_ngram_size: int = 3) -> list:
        """generate_asr_beam_search for several utterances at once (an extension: the reference has no batched search).
        reason_tokens / semantic_tokens: lists of (T, 8) tensors, one pair per utterance.  Each prompt is built with
        prepare_asr_task; the utterances' beams are the row groups of one frame (Model_stage3.beam_search_batch), at most
        64 // beam_width utterances; the plan is re-made for 2 * len(reason_tokens) * beam_width sequences when it is smaller.
        Returns the decoded texts in the order given — each the text generate_asr_beam_search returns for that utterance alone.
        no_repeat_ngram_size (keyword-only): as in generate_asr_beam_search — no effect unless the attribute enforce_ngram is set."""
        if len(reason_tokens) != len(semantic_tokens):
            raise ValueError("one semantic tensor per reason tensor is needed")
        prompts = [self.prepare_asr_task(task_prompt, r, s) for r, s in zip(reason_tokens, semantic_tokens)]
        return self._beam_search_text_batch(prompts, beam_width, length_penalty, max_length,
                                            self._enforced_ngram(no_repeat_ngram_size))

    @torch.inference_mode()
    def generate_asr_batch(self, task_prompt, task_name, reason_tokens, semantic_tokens, temperature: float = 0.9, topk: int = 200,
                           cfg_scale=1.0, seeds=None, batch_size=None) -> list:
        """generate_asr for several utterances at once (an extension: the reference decodes them one by one).  reason_tokens /
        semantic_tokens: lists of (T, 8) tensors, one pair per utterance, argument order as generate_asr_beam_search_batch.  At most
        batch_size utterances (default: all) are live in one decode session, a waiting one is admitted into a freed row
        (_generate_text_batch).  Returns the texts in the order given — greedy (topk = 1): each the text generate_asr returns for
        that utterance alone; sampled: under seeds, utterance b's run with the sampler keyed by seeds[b]."""
        if len(reason_tokens) != len(semantic_tokens):
            raise ValueError("one semantic tensor per reason tensor is needed")
        return self._text_twin(self.prepare_asr_task, [(task_prompt, r, s) for r, s in zip(reason_tokens, semantic_tokens)], topk=topk,
                               temperature=temperature, seeds=seeds, batch_size=batch_size)

    @torch.inference_mode()
    def generate_asr_with_ngram_sampling_batch(self, task_prompt, task_name, reason_tokens, semantic_tokens, temperature: float = 0.9,
                                               topk: int = 200, cfg_scale=1.0, no_repeat_ngram_size: int = 3,
                                               repetition_penalty: float = 1.2, *, fallback_token: int = 128000, seeds=None,
                                               batch_size=None) -> list:
        """generate_asr_with_ngram_sampling for several utterances at once: generate_asr_batch with the device n-gram filter on, every
        row against its own history (an admitted row starts with an empty one).  Each text is the one the single method returns."""
        if len(reason_tokens) != len(semantic_tokens):
            raise ValueError("one semantic tensor per reason tensor is needed")
        return self._text_twin(self.prepare_asr_task, [(task_prompt, r, s) for r, s in zip(reason_tokens, semantic_tokens)], topk=topk,
                               temperature=temperature, no_repeat_ngram_size=no_repeat_ngram_size, ngram_fallback=fallback_token,
                               seeds=seeds, batch_size=batch_size)

    # audio_music_caption_task.py uses the same prompt layout and loop under another name
    generate_audio_caption = generate_asr
    generate_audio_caption_batch = generate_asr_batch

    @torch.inference_mode()
    def generate_answer(self, task_prompt, task_name, d=None, keys=None, types=None, temperature: float = 0.9,
                        topk: int = 200, cfg_scale=1.0) -> str:
        """audio_understanding.py:284-339."""
        tokens, mask = self.get_condition_seq(d, keys, types, task_prompt)
        return self._generate_text(tokens, mask, topk=topk, temperature=temperature)

    @torch.inference_mode()
    def generate_answer_batch(self, task_prompt, task_name, ds, keys, types, temperature: float = 0.9, topk: int = 200, cfg_scale=1.0,
                              seeds=None, batch_size=None) -> list:
        """generate_answer for several utterances at once: ds = one `d` per utterance, keys / types shared (_generate_text_batch)."""
        return self._text_twin(self.get_condition_seq, [(d, keys, types, task_prompt) for d in ds], topk=topk, temperature=temperature,
                               seeds=seeds, batch_size=batch_size)
