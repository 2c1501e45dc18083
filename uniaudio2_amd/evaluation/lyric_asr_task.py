"""Mirror of the reference's evaluation/lyric_asr_task.py `Generator` (task "lyric_recognition",
multi_task_inference.py:195-200): the ASR prompt layout under another name (`prepare_lyric_asr_task` :175-200 is
`prepare_asr_task` line for line: task prompt | reason bos..eos | semantic bos..eos + offset) and the greedy text loop
(`generate_lyric_asr` :202-254) — both in _generator.py."""
import torch

from .asr_task import Generator as _AsrGenerator


class Generator(_AsrGenerator):
    def prepare_lyric_asr_task(self, task_prompt, this_reason_data, this_semantic_data):
        """lyric_asr_task.py:175-200."""
        return self.prepare_asr_task(task_prompt, this_reason_data, this_semantic_data)

    @torch.inference_mode()
    def generate_lyric_asr(self, task_prompt, task_name, text_token=None, semantic_token=None, reason_token=None,
                           temperature: float = 0.9, topk: int = 200, cfg_scale=1.0) -> str:
        """reason_token (T_r, 8), semantic_token (T_s, 8) long -> lyric text (lyric_asr_task.py:202-254)."""
        tokens, mask = self.prepare_lyric_asr_task(task_prompt, reason_token, semantic_token)
        return self._generate_text(tokens, mask, topk=topk, temperature=temperature)

    @torch.inference_mode()
    def generate_lyric_asr_batch(self, task_prompt, task_name, reason_tokens, semantic_tokens, temperature: float = 0.9, topk: int = 200,
                                 cfg_scale=1.0, seeds=None, batch_size=None) -> list:
        """generate_lyric_asr for several utterances at once (an extension; asr_task.Generator.generate_asr_batch): lists of (T, 8)
        tensors in, the lyric texts out in the order given, each the text generate_lyric_asr returns for that utterance alone."""
        if len(reason_tokens) != len(semantic_tokens):
            raise ValueError("one semantic tensor per reason tensor is needed")
        return self._text_twin(self.prepare_lyric_asr_task, [(task_prompt, r, s) for r, s in zip(reason_tokens, semantic_tokens)],
                               topk=topk, temperature=temperature, seeds=seeds, batch_size=batch_size)

    # the command line calls generate_asr for this task as well (multi_task_inference.py:310-327), and so its batched form
    generate_asr_batch = generate_lyric_asr_batch

    def generate_asr_beam_search(self, *args, **kwargs):
        """The reference's lyric Generator has no beam search either."""
        raise ValueError("beam search is not available for lyric_recognition: the reference's lyric Generator "
                         "(evaluation/lyric_asr_task.py) has no generate_asr_beam_search")

    def generate_asr_with_ngram_sampling(self, *args, **kwargs):
        """The reference's lyric Generator has no n-gram variant (the CLI's `--decode_type ngram` fails there with AttributeError)."""
        raise ValueError("--decode_type ngram is not available for lyric_recognition: the reference's lyric Generator "
                         "(evaluation/lyric_asr_task.py) has no generate_asr_with_ngram_sampling")

    generate_asr_with_ngram_sampling_batch = generate_asr_with_ngram_sampling       # refused alike
