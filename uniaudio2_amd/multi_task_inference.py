#!/usr/bin/env python3
"""Command line of the hot path — mirror of the reference's multi_task_inference.py (flags :554-598,
validation :601-649, run_understanding :258-382, run_generation_stage1 :408-525, stage 2 :529-549) on the
MI355X kernels.  Same flags, same `{name}_reason.pt` / `{name}_semantic.pt` (8, T) tensor contract
(generation writes int32, :523-524), same error messages for missing inputs.

    python -m uniaudio2_amd.multi_task_inference --task TTS --stage 1 --text "..." --topk 1 \\
        --llm_train_config cfg.yaml --resume llm.checkpoint --text_tokenizer_path tok_dir --prompt_json prompts.json

Differences, all explicit:
  * `--dtype {bf16,fp32}` (default bf16) picks the kernel precision; the reference runs fp32.
  * `--batch_size N` decodes N utterances of a --text_file together per GPU (continuous batching; TTS / Yue_TTS, TTA, TTM, LTS,
    InstructTTS — speech_s2s stays one by one).  Every utterance samples under its own key (--seed and its global index), so the
    sampled output is the same for every --batch_size and world size, and equal to --batch_size 1.  A rank's shard runs as one
    session of N rows: a waiting utterance is admitted into a row the moment one frees up.
  * Under `torchrun` (WORLD_SIZE > 1) the texts of --text_file are sharded over the ranks, one utterance
    per GPU at a time, and gathered with one RCCL all-gather (uniaudio2_amd/parallel.py); rank 0 writes.
  * --topk > 1 samples on the device with a counter-based generator seeded by --seed: reproducible, same
    distribution as the reference's sample_topk, but not torch's random stream.
  * `--top_p P` (default 0 = off) adds the nucleus filter of the reference's llm_utils/sampling.py sample_top_p to every sampled loop,
    on the device, after the --topk threshold; ties at the threshold value are all kept.  Pure nucleus sampling is --topk = the audio
    vocabulary width (--topk 0 stays refused).  Outside [0, 1] it raises ValueError before a model is built.
  * `--repetition_penalty P` (default 1 = off) with `--repetition_window W` (default 64, 1..512) adds a repetition penalty to every sampled
    loop, on the device inside the samplers: each stream (text head, every audio codebook) of each utterance reads the logits of the distinct
    ids among the last W ids it has produced as l * P if l < 0 else l / P, before the temperature (the CTRL / Hugging Face rule over a
    window; prompt tokens do not count).  Not in the reference, and its effect on audio quality is not measured (no trained checkpoint
    ships).  It routes where --top_p routes; the greedy understanding tasks ignore it; a bad value, or P != 1 with --topk 1 on a generation
    task or with --beam_width, raises ValueError before a model is built.
  * --decode_type ngram (ASR / Yue_ASR: generate_asr_with_ngram_sampling, greedy, n = 3, as the reference's :310-322) runs the
    n-gram filter on the device; its prefill is generate_asr's (the reference's trains-mode prefill leaves the experts' caches
    empty, evaluation/asr_task.py).  lyric_recognition + ngram raises ValueError (the reference's lyric Generator has no such
    method: AttributeError); the caption / understanding / s2t tasks ignore the flag, as the reference does.
  * Beam search: `--beam_width N` (N in 1..8; default 0 = off) with `--length_penalty` (default 0.6), for --task ASR / Yue_ASR under
    --decode_type greedy, runs Generator.generate_asr_beam_search — the reference's search rule (evaluation/asr_task.py:438-576) on the
    device, the N hypotheses as the rows of one frame.  --decode_type beamsearch itself still raises NotImplementedError: the
    reference's function behind that flag cannot run (it calls a method its model lacks), and the message points to --beam_width.
    --beam_width with --decode_type ngram, with lyric_recognition or with a caption / understanding / s2t task raises ValueError.
    `--batch_size N` together with --beam_width W decodes the utterances of --token_dir / --audio_dir in chunks of N, the N beams as
    row groups of one frame (Generator.generate_asr_beam_search_batch): the same results file as --batch_size 1 on the default plan,
    in the order of the names, missing files skipped as before.  N * W is at most 64 (ValueError otherwise); the plan holds 2 * N * W
    sequences — 128 sequences at 2048 positions are about 35 GB of K/V at the released sizes (135 kB per position).
    `--beam_no_repeat_ngram N` (N in 2..16; default 0 = off, the reference's behaviour) runs that search under a no-repeat-n-gram ban
    on the device: an id that would complete an n-gram the hypothesis already holds counts as -inf before the softmax (the
    corrected reading of the reference's `_apply_ngram_constraint`, which bans an always-empty set).  It needs --beam_width >= 1 and works
    with --batch_size; any other value raises ValueError before a model is built.  Its effect on task quality is not measured.
  * `--batch_size N` without --beam_width decodes the understanding tasks in batches too (greedy and --decode_type ngram ASR /
    Yue_ASR, lyric_recognition, audio_caption / music_caption, audio_understanding, speech_s2t): the utterances of --token_dir /
    --audio_dir that exist go into ONE `generate_*_batch` call — one decode session of at most N rows (N is clamped to the number of
    utterances), a row retired at its EOS and a waiting utterance admitted into it at the next chunk boundary — and the results file
    has one line per utterance in the order of the names.  Greedy and n-gram results files are byte-identical to --batch_size 1.
    speech_s2t samples: with N > 1 utterance i (its index among the names) draws under its own key, parallel.utterance_seed(--seed, i),
    so its text is the same for every N >= 2 and equals its single run under that key; --batch_size 1 keeps the one-by-one loop and
    its single sampler stream, whose draws depend on the utterances before.
    Any non-greedy --decode_type for the generation tasks raises NotImplementedError.  No trained checkpoint ships with this
    repository: the search is verified on toy and random weights, not for task quality.
  * Encoding raw audio (--audio / --audio_dir; the understanding tasks and the speech_s2s source) runs the codec's three frozen
    SSL encoders (Whisper, WavLM, BEST-RQ) on the device when the codec yaml (--codec_config) names all three checkpoints
    (`whisper_path`, `wav_lm_path`, `best_rq_ckpt`): `tokenize(path)`, the `{name}_reason.pt` / `{name}_semantic.pt` pair written to
    --output_dir as the reference's _encode_audio_to_tokens does (:124-150, without its discarded 10-step decode), then as for
    --token_dir.  With an encoder missing it raises NotImplementedError naming it; pre-tokenised
    `--reason_pt/--semantic_pt/--token_dir` inputs always work.  The codec is loaded after the LLM and stays loaded (the reference
    loads it first and unloads it).  Stage 2 (tokens -> wav: RVQ look-ups, flow-matching DiT, SQ-Codec) runs on the device; wav
    files are written with scipy (16-bit PCM) because torchaudio is not a dependency.
"""
import argparse
import glob
import json
import math
import os
import random

import torch
import yaml

from .llm_models.model_new import Model_stage3, ModelArgs

UNDERSTANDING_TASKS = ["ASR", "Yue_ASR", "lyric_recognition", "audio_caption", "music_caption", "audio_understanding", "speech_s2t"]
GENERATION_TASKS = ["TTS", "Yue_TTS", "TTA", "TTM", "LTS", "InstructTTS", "speech_s2s"]
TASK_PROMPT_SUFFIX = "\n\n"


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def _prompt_key_from_task(task):
    t = task.strip().lower()
    fixed = {"yue_tts": "Yue_TTS", "yue_asr": "Yue_ASR", "instruct_tts": "InstructTTS", "speech_s2s": "speech_s2s",
             "speech_s2t": "speech_s2t"}
    if t in fixed:
        return fixed[t]
    return t.upper() if t in ("asr", "tts", "tta", "ttm", "lts") else t


def _get_prompt_tensor(args, text_tokenizer, task_name):
    prompt_text = (getattr(args, "prompt_text", None) or "").strip()
    path = getattr(args, "prompt_json", None)
    if prompt_text:
        chosen = prompt_text
    elif path and os.path.isfile(path):
        with open(path, "r", encoding="utf-8") as f:
            prompts = json.load(f)
        key = _prompt_key_from_task(task_name)
        if key not in prompts:
            key = task_name if task_name in prompts else task_name.upper()
        if key not in prompts:
            key = list(prompts.keys())[0]
        if not prompts[key]:
            raise ValueError(f"Task '{key}' has no prompts in {path}.")
        chosen = random.choice(prompts[key])
    else:
        raise ValueError("Provide --prompt_text or --prompt_json.")
    return torch.tensor(text_tokenizer.tokenize(chosen.strip() + TASK_PROMPT_SUFFIX), dtype=torch.long)


def resume_for_inference(resume, exp_dir, model, device):
    """llm_utils/train_utils.py:159-177: {'model': state_dict}, 'module.' prefixes stripped; latest epN.checkpoint of exp_dir otherwise."""
    if resume is None and exp_dir:
        cands = sorted(glob.glob(os.path.join(exp_dir, "ep*.checkpoint")), key=os.path.getmtime)
        resume = cands[-1] if cands else None
    if resume is None:
        raise ValueError("Set --resume or --exp_dir with a checkpoint.")
    ckpt = torch.load(resume, map_location="cpu")
    sd = ckpt["model"] if "model" in ckpt else ckpt
    sd = {(k.split("module.")[-1] if k.startswith("module.") else k): v for k, v in sd.items()}
    model.load_state_dict(sd)
    return model


def _load_config_and_llm(args):
    with open(args.llm_train_config, "r", encoding="utf-8") as f:
        train_args = argparse.Namespace(**yaml.safe_load(f))
    torch.manual_seed(args.seed)
    random.seed(args.seed)            # every rank draws the same task prompt from --prompt_json (random.choice below)
    if not torch.cuda.is_available():
        raise RuntimeError("uniaudio2_amd needs a ROCm GPU (no CPU fallback)")
    rank = int(os.environ.get("LOCAL_RANK", getattr(args, "rank", 0)))
    device = torch.device(f"cuda:{rank % torch.cuda.device_count()}")
    torch.cuda.set_device(device)
    config = ModelArgs(decoder_name=train_args.local_model, llm_pretrained_model=train_args.llm_pretrained_model,
                       llm_name=train_args.llm_name, audio_semantic_vocab_size=train_args.audio_semantic_card,
                       audio_reason_vocab_size=train_args.audio_reason_card, audio_num_codebooks=train_args.parallel_number - 1,
                       audio_embeddings_path=train_args.audio_embeddings_path,
                       audio_understanding_expert_path=train_args.audio_understanding_expert_path)
    model = Model_stage3(config)
    resume_for_inference(args.resume, args.exp_dir, model, device)
    model.to(device=device, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model.order_free_rows = max(0, int(getattr(args, "order_free_rows", 0) or 0))     # applied by setup_caches (bf16 plans)
    model.weight_dtype = torch.float8_e4m3fn if getattr(args, "weight_dtype", "none") == "fp8_e4m3" else None   # likewise
    return train_args, model, device


def _get_generator_class(task):
    task = task.strip().lower()
    from .evaluation import (asr_task, audio_music_caption_task, audio_understanding, audiogen_task, insturct_tts_task, lyric_asr_task,
                             musicgen_task, songen_task, speech_s2s, speech_s2t, tts_task)
    # the reference's routing, module for module (multi_task_inference.py:187-255)
    table = {"asr": asr_task, "yue_asr": asr_task, "lyric_recognition": lyric_asr_task, "audio_caption": audio_music_caption_task,
             "music_caption": audio_music_caption_task, "audio_understanding": audio_understanding, "speech_s2t": speech_s2t,
             "tts": tts_task, "yue_tts": tts_task, "tta": audiogen_task, "ttm": musicgen_task, "lts": songen_task,
             "instruct_tts": insturct_tts_task, "instructtts": insturct_tts_task, "speech_s2s": speech_s2s}
    if task not in table:
        raise ValueError(f"Unknown task: {task}. Understanding: {UNDERSTANDING_TASKS}. Generation: {GENERATION_TASKS}.")
    return table[task].Generator


def _save_tokens(args, name, reason, semantic):
    """The reference's on-disk contract (multi_task_inference.py:522-523): `{name}_reason.pt` / `{name}_semantic.pt`, each a
    torch.save of an (8, T) int32 CPU tensor.  `--save_safetensors` adds `{name}_tokens.safetensors` with the same two
    tensors (keys "reason", "semantic") for consumers that do not unpickle."""
    reason, semantic = reason.cpu().contiguous(), semantic.cpu().contiguous()
    torch.save(reason, os.path.join(args.output_dir, f"{name}_reason.pt"))
    torch.save(semantic, os.path.join(args.output_dir, f"{name}_semantic.pt"))
    if getattr(args, "save_safetensors", False):
        from safetensors.torch import save_file
        save_file({"reason": reason, "semantic": semantic}, os.path.join(args.output_dir, f"{name}_tokens.safetensors"))


def _generation_method_name(task):
    t = task.strip().lower()
    if t in ("tts", "yue_tts"):
        return "generate_tts"
    if t in ("tta", "ttm"):
        return "generate_audio"
    if t == "lts":
        return "generate_LTS"
    if t in ("instruct_tts", "instructtts"):
        return "generate_instruct_tts"
    if t == "speech_s2s":
        return "generate_audio"
    raise ValueError(f"Unknown generation task: {task}")


def _check_top_p(args):
    """--top_p: 0.0 = off, (0, 1) = the nucleus filter, 1.0 = off as well; anything else (NaN included) is refused before a model is built."""
    top_p = float(getattr(args, "top_p", 0.0) or 0.0)
    if not 0.0 <= top_p <= 1.0:
        raise ValueError(f"--top_p must be in [0, 1] (0 = off), got {top_p}")
    return top_p


def _apply_top_p(args, generator):
    """The generator hears of --top_p only when it is set: with the default nothing new is called anywhere."""
    top_p = _check_top_p(args)
    if top_p != 0.0:
        generator.top_p = top_p
    return generator


def _check_repetition(args, generation):
    """--repetition_penalty / --repetition_window: 1.0 = off; refused before a model is built: a penalty that is not finite or not > 0, a
    window outside 1..512, a penalty != 1 with --topk 1 on a generation task (a greedy frame has no logits pass to penalise) or with
    --beam_width (beam search ranks the logits itself).  -> (penalty, window)."""
    penalty = getattr(args, "repetition_penalty", None)
    penalty = 1.0 if penalty is None else float(penalty)
    window = getattr(args, "repetition_window", None)
    window = 64 if window is None else int(window)
    if not (math.isfinite(penalty) and penalty > 0.0):
        raise ValueError(f"--repetition_penalty must be finite and > 0 (1 = off), got {penalty}")
    if not 1 <= window <= 512:
        raise ValueError(f"--repetition_window must be in 1..512, got {window}")
    if penalty != 1.0:
        if generation and int(getattr(args, "topk", 50) or 0) == 1:
            raise ValueError("--repetition_penalty needs a sampled loop: with --topk 1 the frame is greedy and has no logits pass to penalise")
        if int(getattr(args, "beam_width", 0) or 0) >= 1:
            raise ValueError("--repetition_penalty does not combine with --beam_width: beam search ranks the logits itself "
                             "(--beam_no_repeat_ngram N bans repeated n-grams inside the beam)")
    return penalty, window


def _apply_repetition(args, generator, generation):
    """As _apply_top_p: the generator hears of the penalty only when it is on."""
    penalty, window = _check_repetition(args, generation)
    if penalty != 1.0:
        generator.repetition_penalty, generator.repetition_window = penalty, window
    return generator


def _check_decode(args):
    if args.decode_type != "greedy":
        raise NotImplementedError("--decode_type ngram/beamsearch are not on the device path (greedy only this round)")


def _check_understanding_decode(args, task):
    """multi_task_inference.py:310-322 of the reference: ngram reaches generate_asr_with_ngram_sampling for the ASR tasks and is
    ignored by the others; its lyric Generator lacks the method.  Beam search is dead code there."""
    if args.decode_type == "beamsearch":
        raise NotImplementedError("--decode_type beamsearch is not routed: the reference's generate_asr_beam_search cannot run (it calls "
                                  "Model_stage3.get_next_logits, which does not exist); the working search is --beam_width N "
                                  "(with --decode_type greedy, --task ASR / Yue_ASR)")
    bw = int(getattr(args, "beam_width", 0) or 0)
    if bw < 0 or bw > 8:
        raise ValueError(f"--beam_width must be in 0..8 (0 = off), got {bw}")
    bn = int(getattr(args, "beam_no_repeat_ngram", 0) or 0)
    if bn != 0 and not 2 <= bn <= 16:
        raise ValueError(f"--beam_no_repeat_ngram must be 0 (off) or in 2..16, got {bn}")
    if bn != 0 and bw < 1:
        raise ValueError(f"--beam_no_repeat_ngram {bn} needs a beam search: --beam_width N with N in 1..8")
    if bw >= 1:
        if args.decode_type == "ngram":
            raise ValueError("--beam_width does not combine with --decode_type ngram: the reference's beam search bans no n-gram "
                             "(its _apply_ngram_constraint works on an empty set) and its n-gram loop is greedy; "
                             "--beam_no_repeat_ngram N bans repeated n-grams inside the beam")
        if task == "lyric_recognition":
            raise ValueError("--beam_width is not available for lyric_recognition: the reference's lyric Generator "
                             "(evaluation/lyric_asr_task.py) has no generate_asr_beam_search")
        if task not in ("asr", "yue_asr"):
            raise ValueError(f"--beam_width is not available for {task}: the reference defines beam search for the ASR Generator "
                             "only (evaluation/asr_task.py); the caption / understanding / s2t generators have no such method")
        bs = int(getattr(args, "batch_size", 1) or 1)
        if bs * bw > 64:
            raise ValueError(f"--batch_size {bs} x --beam_width {bw} = {bs * bw} rows: a beam frame holds at most 64 "
                             "(lower --batch_size or --beam_width)")
    if args.decode_type == "ngram" and task == "lyric_recognition":
        raise ValueError("--decode_type ngram is not available for lyric_recognition: the reference's lyric Generator "
                         "(evaluation/lyric_asr_task.py) has no generate_asr_with_ngram_sampling")


def _has_raw_audio(args):
    return bool((args.audio and os.path.isfile(args.audio)) or (args.audio_dir and os.path.isdir(args.audio_dir)))


SSL_ENCODERS = (("Whisper", "whisper_encoder", "whisper_path"), ("WavLM", "wavlm_encoder", "wav_lm_path"), ("BEST-RQ", "bestrq_encoder", "best_rq_ckpt"))


def _encode_audio_to_tokens(args, generator, out_dir, alternative):
    """multi_task_inference.py:124-150: --audio / --audio_dir -> `{name}_reason.pt` / `{name}_semantic.pt` in out_dir through the
    generator's audio tokenizer (created from --codec_config on first use); returns (out_dir, names).  The tokenizer must carry the
    three frozen SSL encoders; otherwise NotImplementedError names the ones its yaml did not provide."""
    tok = getattr(generator, "_audio_tokenizer", None)
    if tok is None and getattr(args, "codec_config", None):
        tok = generator._audio_tokenizer = _load_codec(args, generator.device)
    model = getattr(tok, "model", None)
    missing = [f"{name} (yaml key {key})" for name, attr, key in SSL_ENCODERS if getattr(model, attr, None) is None]
    if getattr(model, "ssl_features", None) is not None:          # an injected callable stands in for whatever is missing
        missing = []
    if tok is None or missing:
        raise NotImplementedError("encoding raw audio needs the codec's frozen SSL encoders (out of scope, SURVEY.md §8f); "
                                  f"{alternative} — not provided by the codec yaml: {', '.join(missing)}")
    if args.audio and os.path.isfile(args.audio):
        audio_list = [(os.path.splitext(os.path.basename(args.audio))[0], args.audio)]
    else:
        audio_list = [(os.path.splitext(os.path.basename(p))[0], p) for p in sorted(glob.glob(os.path.join(args.audio_dir, "*.wav")))]
    os.makedirs(out_dir, exist_ok=True)
    names = []
    for name, path in audio_list:
        with torch.no_grad():
            reason, rec = tok.tokenize(path, return_reasoning_text=False)
        torch.save(reason.cpu(), os.path.join(out_dir, f"{name}_reason.pt"))
        torch.save(rec.cpu(), os.path.join(out_dir, f"{name}_semantic.pt"))
        names.append(name)
        print(f"[Encode] {path} -> {name}_reason.pt, {name}_semantic.pt")
    return out_dir, names


def _load_token_pair(token_dir, name):
    """(reason, semantic) as (T, 8) long tensors (:304-308), or None (and the [Skip] line) when either file is missing."""
    rp, sp = os.path.join(token_dir, f"{name}_reason.pt"), os.path.join(token_dir, f"{name}_semantic.pt")
    if not os.path.isfile(rp) or not os.path.isfile(sp):
        print(f"[Skip] {name}: missing reason/semantic .pt")
        return None
    return torch.load(rp, map_location="cpu").transpose(0, 1).long(), torch.load(sp, map_location="cpu").transpose(0, 1).long()


def _beam_ngram_kwargs(args, generator):
    """--beam_no_repeat_ngram N >= 2: the generator's opt-in ban (Generator.enforce_ngram) and its n; nothing otherwise (the
    generators are called as before)."""
    n = int(getattr(args, "beam_no_repeat_ngram", 0) or 0)
    if not n:
        return {}
    generator.enforce_ngram = True
    return dict(no_repeat_ngram_size=n)


def _beam_search_in_chunks(args, generator, task, task_prompt, token_dir, names, f_out):
    """--beam_width with --batch_size N > 1: the names in their order, in chunks of N that exist (a missing file is skipped and does not
    count), each chunk one generate_asr_beam_search_batch call; one results line per utterance, in the order of names."""
    n = int(args.batch_size)
    chunk = []

    def flush():
        if not chunk:
            return
        texts = generator.generate_asr_beam_search_batch(task_prompt, task_name=task, reason_tokens=[r for _, r, _ in chunk],
                                                         semantic_tokens=[s for _, _, s in chunk], beam_width=args.beam_width,
                                                         length_penalty=args.length_penalty, **_beam_ngram_kwargs(args, generator))
        if len(texts) != len(chunk):
            raise RuntimeError(f"beam search returned {len(texts)} texts for {len(chunk)} utterances")
        for (name, _, _), text_out in zip(chunk, texts):
            f_out.write(f"{name}\t{text_out}\n")
            print(f"[{task}] {name} -> {text_out[:80]}...")
        del chunk[:]

    for name in names:
        pair = _load_token_pair(token_dir, name)
        if pair is None:
            continue
        chunk.append((name, pair[0], pair[1]))
        if len(chunk) == n:
            flush()
    flush()


def _understand_in_one_session(args, generator, task, task_prompt, token_dir, names, f_out):
    """--batch_size N > 1 without --beam_width: the pairs that exist, in the order of names, through ONE generate_*_batch call — a
    decode session of at most N rows with admission into freed rows (GeneratorBase._generate_text_batch); one results line per
    utterance, in the order of names.  Greedy and n-gram tasks: the texts of the one-by-one loop.  speech_s2t: utterance i of names
    samples under parallel.utterance_seed(--seed, i), whatever shares its batch."""
    from . import parallel
    items = []                                                   # (index in names, name, reason (T, 8), semantic (T, 8))
    for i, name in enumerate(names):
        pair = _load_token_pair(token_dir, name)
        if pair is not None:
            items.append((i, name, pair[0], pair[1]))
    if not items:
        return
    kw = dict(temperature=args.temperature, cfg_scale=args.cfg_scale, batch_size=int(args.batch_size))
    if task == "audio_understanding":
        question = _question(args)
        q = torch.tensor(generator._text_tokenizer.tokenize(question), dtype=torch.long)
        ds = [{"text_seq_question": q, "reason_seq": r.transpose(0, 1), "semantic_seq": s.transpose(0, 1)} for _, _, r, s in items]
        texts = generator.generate_answer_batch(task_prompt, task_name=task, ds=ds, keys=list(ds[0]), types=["text", "audio", "audio"],
                                                topk=1, **kw)
    elif task == "speech_s2t":                                   # samples with --topk: one key per utterance
        ds = [{"reason_seq": r, "semantic_seq": s} for _, _, r, s in items]
        texts = generator.generate_answer_batch(task_prompt, task_name="speech_s2t", ds=ds, keys=["reason_seq", "semantic_seq"],
                                                types=["audio", "audio"], topk=args.topk,
                                                seeds=[parallel.utterance_seed(args.seed, i) for i, _, _, _ in items], **kw)
    else:
        method = ("generate_audio_caption_batch" if task in ("audio_caption", "music_caption") else
                  "generate_asr_with_ngram_sampling_batch" if args.decode_type == "ngram" else "generate_asr_batch")
        texts = getattr(generator, method)(task_prompt, task_name=task, reason_tokens=[r for _, _, r, _ in items],
                                           semantic_tokens=[s for _, _, _, s in items], topk=1, **kw)
    if len(texts) != len(items):
        raise RuntimeError(f"the batched decode returned {len(texts)} texts for {len(items)} utterances")
    for (_, name, _, _), text_out in zip(items, texts):
        if task == "speech_s2t":
            if text_out == (-1, -1):
                print(f"[Skip] {name}: sequence too long for speech_s2t")
                continue
            text_out = text_out[0] if isinstance(text_out, tuple) else text_out
        f_out.write(f"{name}\t{text_out}\n")
        print(f"[{task}] {name} -> {text_out[:80]}...")


def _question(args):
    """--question, else the text of --question_file, else the reference's default (:345-349)."""
    question = (args.question or "").strip()
    if not question and args.question_file and os.path.isfile(args.question_file):      # :345-347
        with open(args.question_file, "r", encoding="utf-8") as f:
            question = f.read().strip()
    return question or "What is described in this audio?"


def run_understanding(args):
    task = args.task.strip().lower()
    _check_understanding_decode(args, task)
    _check_top_p(args)
    _check_repetition(args, False)
    raw_audio = _has_raw_audio(args)
    if raw_audio:
        token_dir, names = args.output_dir, []
    elif args.reason_pt and args.semantic_pt and os.path.isfile(args.reason_pt) and os.path.isfile(args.semantic_pt):
        token_dir = os.path.dirname(args.reason_pt) or "."
        names = [os.path.basename(args.reason_pt).replace("_reason.pt", "")]
    elif args.token_dir and os.path.isdir(args.token_dir):
        names = [os.path.basename(p).replace("_reason.pt", "") for p in sorted(glob.glob(os.path.join(args.token_dir, "*_reason.pt")))]
        token_dir = args.token_dir
    else:
        raise ValueError("For understanding task provide --audio/--audio_dir, --reason_pt+--semantic_pt, or --token_dir with *_reason.pt.")
    train_args, model, device = _load_config_and_llm(args)
    generator = _get_generator_class(task)(model, train_args, audio_tokenizer_config=args.audio_tokenizer_config,
                                           audio_model_path=args.audio_model_path, text_tokenizer_path=args.text_tokenizer_path,
                                           is_cfg=args.use_cfg)
    _apply_top_p(args, generator)
    _apply_repetition(args, generator, False)
    if raw_audio:
        token_dir, names = _encode_audio_to_tokens(args, generator, args.output_dir, "pass --reason_pt + --semantic_pt or --token_dir")
    beam_batch = int(getattr(args, "batch_size", 1) or 1) if int(getattr(args, "beam_width", 0) or 0) >= 1 else 1
    if int(getattr(args, "beam_width", 0) or 0) >= 1:            # the K/V fork of a beam of W keeps two page sets: a plan of 2 W sequences
        model.setup_caches(2 * int(args.beam_width) * max(1, min(beam_batch, len(names))))    # ... per utterance of a chunk
    task_prompt = _get_prompt_tensor(args, generator._text_tokenizer, args.task)
    results_path = args.results or os.path.join(args.output_dir, f"{task}_results.txt")
    os.makedirs(os.path.dirname(results_path) or ".", exist_ok=True)
    with open(results_path, "w") as f_out:
        if beam_batch > 1:                                       # asr, yue_asr under --beam_width (checked above)
            _beam_search_in_chunks(args, generator, task, task_prompt, token_dir, names, f_out)
            names = []
        elif int(getattr(args, "beam_width", 0) or 0) < 1 and int(getattr(args, "batch_size", 1) or 1) > 1:
            _understand_in_one_session(args, generator, task, task_prompt, token_dir, names, f_out)
            names = []
        for name in names:
            pair = _load_token_pair(token_dir, name)
            if pair is None:
                continue
            reason, semantic = pair                              # (T, 8)
            if task == "audio_understanding":
                question = _question(args)
                d = {"text_seq_question": torch.tensor(generator._text_tokenizer.tokenize(question), dtype=torch.long),
                     "reason_seq": reason.transpose(0, 1), "semantic_seq": semantic.transpose(0, 1)}
                text_out = generator.generate_answer(task_prompt, task_name=task, d=d, keys=list(d), types=["text", "audio", "audio"],
                                                     temperature=args.temperature, topk=1, cfg_scale=args.cfg_scale)
            elif task == "speech_s2t":                                                             # :363-379: samples with --topk
                d = {"reason_seq": reason, "semantic_seq": semantic}                                # (T, 8) as the reference passes them (:368)
                result = generator.generate_answer(task_prompt, task_name="speech_s2t", d=d, keys=["reason_seq", "semantic_seq"],
                                                   types=["audio", "audio"], temperature=args.temperature, topk=args.topk,
                                                   cfg_scale=args.cfg_scale)
                if result == (-1, -1):                                                             # :379-381
                    print(f"[Skip] {name}: sequence too long for speech_s2t")
                    continue
                text_out = result[0] if isinstance(result, tuple) else result
            elif task in ("audio_caption", "music_caption"):                                       # :329-342
                text_out = generator.generate_audio_caption(task_prompt, task_name=task, reason_token=reason, semantic_token=semantic,
                                                            temperature=args.temperature, topk=1, cfg_scale=args.cfg_scale)
            elif int(getattr(args, "beam_width", 0) or 0) >= 1:                                     # asr, yue_asr (checked above)
                text_out = generator.generate_asr_beam_search(task_prompt, task_name=task, reason_token=reason, semantic_token=semantic,
                                                              beam_width=args.beam_width, length_penalty=args.length_penalty,
                                                              **_beam_ngram_kwargs(args, generator))
            elif args.decode_type == "ngram":                                                       # :316-321: asr, yue_asr
                text_out = generator.generate_asr_with_ngram_sampling(task_prompt, task_name=task, reason_token=reason,
                                                                      semantic_token=semantic, temperature=args.temperature, topk=1,
                                                                      cfg_scale=args.cfg_scale)
            else:   # asr, yue_asr, lyric_recognition (:310-327: the reference calls generate_asr on all three; its lyric module only
                    # defines generate_lyric_asr, so the call fails there — here the lyric Generator has both names)
                text_out = generator.generate_asr(task_prompt, task_name=task, reason_token=reason, semantic_token=semantic,
                                                  temperature=args.temperature, topk=1, cfg_scale=args.cfg_scale)
            f_out.write(f"{name}\t{text_out}\n")
            print(f"[{task}] {name} -> {text_out[:80]}...")
    print(f"Results written to {results_path}")


def run_generation_stage1(args):
    import torch.distributed as dist
    from . import parallel
    task = args.task.strip().lower()
    _check_decode(args)
    _check_top_p(args)
    _check_repetition(args, True)
    os.makedirs(args.output_dir, exist_ok=True)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl")
    train_args, model, device = _load_config_and_llm(args)
    generator = _get_generator_class(task)(model, train_args, audio_tokenizer_config=args.audio_tokenizer_config,
                                           audio_model_path=args.audio_model_path, text_tokenizer_path=args.text_tokenizer_path,
                                           is_cfg=args.use_cfg)
    _apply_top_p(args, generator)
    _apply_repetition(args, generator, True)
    tok = generator._text_tokenizer
    task_prompt = _get_prompt_tensor(args, tok, args.task)
    if task == "speech_s2s":
        return _run_speech_s2s(args, generator, task_prompt)
    if args.text and args.text.strip():
        items = [("utt_0", args.text.strip())]
    elif args.text_file and os.path.isfile(args.text_file):
        with open(args.text_file, "r", encoding="utf-8") as f:
            items = [(f"utt_{i}", line.strip()) for i, line in enumerate(f) if line.strip()]
    else:
        raise ValueError("Generation requires --text or --text_file.")
    if not items:
        raise ValueError("No text input.")
    gen_fn = getattr(generator, _generation_method_name(task))
    ids = [torch.tensor(tok.tokenize(t), dtype=torch.long) for _, t in items]

    extra = (lambda i: {"caption": ids[i]}) if _generation_method_name(task) == "generate_instruct_tts" else (lambda i: {})   # :520-521

    def one(i):
        # the sampler's key folds in the global utterance index and a new key rewinds the device's draw index
        # (ua2_stage3_set_sampling), so with one utterance at a time an utterance's samples depend only on (seed, index):
        # not on the world size, nor on what its rank generated before it (tests/test_gpu_lm.py)
        model.sampling_seed = parallel.utterance_seed(args.seed, i)
        return gen_fn(task_prompt=task_prompt, task_name=task, text_token=ids[i], temperature=args.temperature,
                      topk=args.topk, cfg_scale=args.cfg_scale, **extra(i))

    twin_name = _generation_method_name(task) + "_batch"
    twin = getattr(generator, twin_name, None)
    if args.batch_size > 1 and twin is not None:
        def many(idx):
            # every utterance draws under its own key (its global index), whatever shares its batch: sampled output is the same
            # for every --batch_size and world size, and equal to --batch_size 1 (tests/test_gpu_row_streams.py)
            kw = {"captions": [ids[i] for i in idx]} if twin_name == "generate_instruct_tts_batch" else {}      # :520-521
            return twin(task_prompt=task_prompt, task_name=task, text_tokens=[ids[i] for i in idx], temperature=args.temperature,
                        topk=args.topk, cfg_scale=args.cfg_scale, seeds=[parallel.utterance_seed(args.seed, i) for i in idx],
                        batch_size=args.batch_size, **kw)
        # the rank's whole shard in one session of --batch_size rows: a waiting utterance is admitted into a freed row (measured
        # faster than consecutive chunks of --batch_size on every workload tried: profiles/row_streams_admission.txt)
        results = parallel.run_sharded_stream(list(range(len(items))), [len(x) for x in ids], many)
    else:
        results = parallel.run_sharded(list(range(len(items))), [len(x) for x in ids], one)
    _write_results(args, items, results, "[Stage1]")
    return args.output_dir


def _write_results(args, items, results, tag):
    """Rank 0 writes the gathered token tensors; an utterance whose generation failed on its rank (parallel.Failed:
    e.g. the model never produced the semantic phase) is reported after everything else was saved."""
    from . import parallel
    failed = []
    rank0 = int(os.environ.get("RANK", "0")) == 0
    for i, (name, _) in enumerate(items):                       # every rank holds every result (the all-gather): all of them raise
        if isinstance(results[i], parallel.Failed):             # together, none is left waiting in stage 2's barrier
            failed.append(name)
            if rank0:
                print(f"[Fail] {name}: {results[i].message}")
            continue
        if rank0:
            reason, semantic = results[i]
            _save_tokens(args, name, reason, semantic)
            print(f"{tag} {name} -> {name}_reason.pt, {name}_semantic.pt")
    if failed:
        raise RuntimeError(f"{len(failed)} of {len(items)} utterances failed: {', '.join(failed)}")


def _run_speech_s2s(args, generator, task_prompt):
    """multi_task_inference.py:414-483: source = *_reason.pt / *_semantic.pt pairs of --token_dir; output = generated pairs."""
    import glob
    from . import parallel
    from .evaluation.speech_s2s import S2S_KEYS, S2S_TYPES
    if _has_raw_audio(args):                                                  # :425-434: the sources go to <output_dir>/source
        source_dir, names = _encode_audio_to_tokens(args, generator, os.path.join(args.output_dir, "source"),
                                                    "pass --token_dir with the source *_reason.pt / *_semantic.pt")
    elif args.token_dir and os.path.isdir(args.token_dir):
        source_dir = args.token_dir
        names = [os.path.basename(p).replace("_reason.pt", "") for p in sorted(glob.glob(os.path.join(args.token_dir, "*_reason.pt")))]
    else:
        raise ValueError("speech_s2s requires --audio, --audio_dir, or --token_dir (source reason/semantic .pt).")
    items = []
    for name in names:
        rp, sp = os.path.join(source_dir, f"{name}_reason.pt"), os.path.join(source_dir, f"{name}_semantic.pt")
        if not os.path.isfile(sp):
            print(f"[Skip] {name}: missing source {rp} or {sp}")
            continue
        reason, semantic = torch.load(rp, map_location="cpu"), torch.load(sp, map_location="cpu")
        items.append((name, {"reason_seq_1": reason, "semantic_seq_1": semantic, "reason_seq_2": reason, "semantic_seq_2": semantic}))

    def one(i):
        generator._model.sampling_seed = parallel.utterance_seed(args.seed, i)
        return generator.generate_audio(task_prompt=task_prompt, task_name="speech_s2s", d=items[i][1], keys=S2S_KEYS[:-2],
                                        types=S2S_TYPES[:-2], temperature=args.temperature, topk=args.topk, cfg_scale=args.cfg_scale)

    results = parallel.run_sharded(list(range(len(items))), [int(d["semantic_seq_1"].shape[-1]) for _, d in items], one)
    _write_results(args, items, results, "[Stage1] speech_s2s")
    return args.output_dir


def _load_codec(args, device):
    """multi_task_inference.py:84-97."""
    from .tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    if not args.codec_config:
        raise ValueError("Stage 2 requires --codec_config (the codec's infer yaml) and --codec_ckpt.")
    return ReasoningTokenizer(train_config=args.codec_config, model_path=args.codec_ckpt, music_ssl_folder=args.music_ssl_folder, device=device)


def save_wav(path, wave, sample_rate):
    """torchaudio.save(path, wave (1, N) float32, sr) of the reference (:546) without torchaudio: 16-bit PCM, the
    default encoding torchaudio picks for float input to a .wav."""
    import numpy as np
    from scipy.io import wavfile
    x = wave.detach().cpu().float().clamp(-1.0, 1.0).numpy()
    wavfile.write(path, int(sample_rate), np.round(x.T * 32767.0).astype(np.int16))


def stage2_shard(names, world, rank, lengths=None):
    """Utterances of stage 2 this rank decodes ("codec stage 2 shards the same way ... by utterance"; the reference
    loops over all of them on one GPU, multi_task_inference.py:540-548).  With `lengths` (semantic frames per utterance) the split is
    stage 1's — longest first, dealt round-robin (parallel.shard_indices) — so every rank gets the same mix of 1-, 2- and 3-window
    utterances and a rank's list comes back longest first: consecutive --codec_batch groups then hold utterances with the same
    window count and do not shrink window by window.  Without lengths: names[rank::world] of the sorted list.  The outputs are
    files, so the stage needs no collective: the union over ranks is every name, the shards are disjoint."""
    if lengths is None:
        return list(names[rank::max(1, world)])
    from . import parallel
    return [names[i] for i in parallel.shard_indices(list(lengths), max(1, world), rank)]


def _semantic_frames(path):
    """T of a `{name}_semantic.pt` (8, T) file; 0 when it is missing (the utterance is then skipped with a message)."""
    if not os.path.isfile(path):
        return 0
    return int(torch.load(path, map_location="cpu").shape[-1])


def run_generation_stage2(args):
    """multi_task_inference.py:529-549: every `*_semantic.pt` of --token_dir (default: --output_dir) -> `{wav_dir}/{name}.wav`
    through ReasoningTokenizer.detokenize_no_reason (RVQ look-ups -> flow-matching DiT + guided Euler ODE -> SQ-Codec decode ->
    cross-faded 20-s windows).  Under torchrun every rank decodes its shard of the utterances (stage2_shard), --codec_batch of them
    at a time (detokenize_no_reason_batch: window k of the batch in one DiT solve)."""
    if not torch.cuda.is_available():
        raise RuntimeError("uniaudio2_amd needs a ROCm GPU (no CPU fallback)")
    rank = int(os.environ.get("LOCAL_RANK", getattr(args, "rank", 0)))
    device = torch.device(f"cuda:{rank % torch.cuda.device_count()}")
    torch.cuda.set_device(device)
    return decode_token_dir(_load_codec(args, device), args, device)


def decode_token_dir(codec, args, device):
    """Stage 2 proper, on a loaded codec (anything with detokenize_no_reason / detokenize_no_reason_batch / sample_rate): this
    rank's shard of the token files -> wav files.  RANK / WORLD_SIZE as torchrun sets them."""
    token_dir = args.token_dir or args.output_dir
    names = [os.path.basename(p).replace("_reason.pt", "") for p in sorted(glob.glob(os.path.join(token_dir, "*_reason.pt")))]
    wav_dir = args.wav_dir or os.path.join(token_dir, "wavs")
    os.makedirs(wav_dir, exist_ok=True)
    world, grank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    frames = [_semantic_frames(os.path.join(token_dir, f"{n}_semantic.pt")) for n in names]       # every rank reads the same few bytes
    mine = []
    for name in stage2_shard(names, world, grank, lengths=frames):
        sp = os.path.join(token_dir, f"{name}_semantic.pt")
        if not os.path.isfile(sp):
            print(f"[Skip] {name}: missing {sp}")
            continue
        mine.append((name, sp))
    bs = max(1, int(getattr(args, "codec_batch", 1) or 1))
    for b0 in range(0, len(mine), bs):
        chunk = mine[b0:b0 + bs]
        codes = [torch.load(sp, map_location=device).long() for _, sp in chunk]
        if len(chunk) == 1:
            waves = [codec.detokenize_no_reason(codes[0], return_reasoning_text=False, steps=args.codec_steps)]
        else:
            waves = codec.detokenize_no_reason_batch(codes, steps=args.codec_steps, max_batch=bs)
        for (name, _), wave in zip(chunk, waves):
            wav_path = os.path.join(wav_dir, f"{name}.wav")
            save_wav(wav_path, wave, codec.sample_rate)
            print(f"[Stage2] {name} -> {wav_path}")
    return wav_dir


class _Parser(argparse.ArgumentParser):
    """Checks the options that only make sense together at parse time (a usage error, not a failure after the checkpoint loaded)."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.weight_dtype != "none" and ns.dtype != "bf16":
            self.error("--weight_dtype fp8_e4m3 needs --dtype bf16 (the fp32 plan is the exact contract)")
        return ns


def get_parser():
    p = _Parser(description="Multi-task inference: understanding (audio->text) or generation (text->wav)")
    p.add_argument("--task", type=str, required=True)
    p.add_argument("--stage", type=str, default="all", choices=["1", "2", "all"])
    for name in ("audio", "audio_dir", "reason_pt", "semantic_pt", "question", "question_file", "text_file", "results", "token_dir",
                 "wav_dir", "prompt_text", "prompt_json", "llm_train_config", "resume", "exp_dir", "text_tokenizer_path",
                 "audio_tokenizer_config", "audio_model_path", "codec_config", "codec_ckpt", "music_ssl_folder"):
        p.add_argument(f"--{name}", type=str, default=None)
    p.add_argument("--text", type=str, default="")
    p.add_argument("--output_dir", type=str, default="./multi_task_out")
    p.add_argument("--repetition_penalty", type=float, default=1.0,
                   help="repetition penalty of the sampled loops (extension, not in the reference; the CTRL / Hugging Face rule over a window): "
                        "every sampler reads the logits of the distinct ids among the last --repetition_window ids its own stream (text head, each "
                        "audio codebook) has produced for the utterance as l * penalty if l < 0 else l / penalty, before --temperature.  1 = off "
                        "(default); prompt tokens do not count.  It acts where --top_p does: the sampled audio loops (single, --batch_size, "
                        "--use_cfg) and speech_s2t; the greedy understanding tasks ignore it, and it is refused with --topk 1 on a generation task "
                        "and with --beam_width.  Its effect on audio quality is not measured: no trained checkpoint ships")
    p.add_argument("--repetition_window", type=int, default=64, help="ids of history the repetition penalty looks back over, per stream (1..512)")
    p.add_argument("--use_cfg", type=str2bool, default=False)
    p.add_argument("--temperature", type=float, default=0.9)
    p.add_argument("--topk", type=int, default=50)
    p.add_argument("--top_p", type=float, default=0.0,
                   help="nucleus sampling (extension; the rule of the reference's llm_utils/sampling.py sample_top_p): among the --topk most "
                        "probable ids keep those whose strictly-more-probable mass is at most this share of the kept mass (ties at the "
                        "threshold all kept), then draw.  0 = off (default), as is 1; it acts where --topk does (no effect on greedy loops).  "
                        "Pure nucleus sampling: --topk = the audio vocabulary width (reason + semantic cardinality)")
    p.add_argument("--cfg_scale", type=float, default=1.0)
    p.add_argument("--decode_type", type=str, default="greedy", choices=["greedy", "ngram", "beamsearch"])
    p.add_argument("--codec_steps", type=int, default=50)
    p.add_argument("--codec_duration", type=float, default=30.0)
    p.add_argument("--seed", type=int, default=888)
    p.add_argument("--rank", type=int, default=0)
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="kernel precision (extension; the reference runs fp32)")
    p.add_argument("--weight_dtype", type=str, default="none", choices=["none", "fp8_e4m3"],
                   help="stage 1, --dtype bf16 only (extension): fp8_e4m3 replaces every Linear weight of the LM by its weight-only 8-bit form "
                        "(OCP e4m3fn, one power-of-two scale per output row; embeddings, norms and the K/V cache stay as they are) and decode "
                        "frames of up to 5 sequences stream the fp8 copies.  LOSSY: a weight's relative rms error is 2.7e-2 (bf16: 1.6e-3), ids "
                        "can differ from the bf16 run.  Costs 1.5 x the bf16 weight memory.  Default none")
    p.add_argument("--save_safetensors", action="store_true",
                   help="also write {name}_tokens.safetensors next to the reference's two .pt files (extension)")
    p.add_argument("--codec_batch", type=int, default=1,
                   help="utterances whose k-th windows share one DiT solve / SQ-Codec decode in stage 2 (extension; default 1 = one by one as "
                        "the reference: a waveform then never depends on which other files are in the directory, on WORLD_SIZE or on this "
                        "flag.  8 halves the time per window; under the DiT's default order-free GEMM plan a waveform then differs from its "
                        "one-by-one value by bf16 rounding noise (~3e-3 relative rms); UA2_DIT_SUM_ORDER=0 keeps the bits at any batch)")
    p.add_argument("--order_free_rows", type=int, default=0,
                   help="stage 1, bf16 (extension): LM launches of at least this many rows (batched prefill, decode frames of that many "
                        "sequences) take the order-free 256-row-tile GEMM — faster, but a sequence's ids may then depend on what shares "
                        "its batch.  Default 0 = off: every row keeps the bits of its single-sequence run")
    p.add_argument("--beam_width", type=int, default=0,
                   help="ASR / Yue_ASR with --decode_type greedy (extension): N in 1..8 decodes with beam search over N hypotheses on the "
                        "device (the reference's generate_asr_beam_search rule, which its own --decode_type beamsearch cannot run).  "
                        "With --batch_size N the utterances are decoded N at a time, their beams side by side in one frame: N * W <= 64, "
                        "same results.  Default 0 = off")
    p.add_argument("--length_penalty", type=float, default=0.6,
                   help="--beam_width: exponent of the length normalisation ((5 + length) / 6) ** length_penalty (the reference's default 0.6)")
    p.add_argument("--beam_no_repeat_ngram", type=int, default=0,
                   help="--beam_width (extension): N in 2..16 runs the beam search under a no-repeat-n-gram ban on the device — an id that "
                        "would complete an n-gram the hypothesis already holds counts as -inf before the softmax.  Works with --batch_size.  "
                        "Default 0 = off: the reference's search, which accepts no_repeat_ngram_size and bans nothing")
    p.add_argument("--batch_size", type=int, default=1,
                   help="utterances decoded together per GPU (extension; 1 = one by one as the reference).  TTS / Yue_TTS / TTA / TTM / LTS / "
                        "InstructTTS with --text_file: at most N live utterances per GPU, waiting ones admitted into freed rows; greedy and sampled output "
                        "independent of N.  ASR / Yue_ASR with --beam_width W: chunks of N utterances per beam-search frame, N * W <= 64; "
                        "the K/V plan then holds 2 * N * W sequences (128 sequences at 2048 positions: about 35 GB at the released sizes).  "
                        "The understanding tasks without --beam_width (ASR / Yue_ASR greedy or --decode_type ngram, lyric_recognition, the "
                        "caption tasks, audio_understanding, speech_s2t): the utterances of --token_dir / --audio_dir decode in one session of "
                        "at most N rows (N is clamped to their number), a finished row taken by the next waiting utterance; greedy and ngram "
                        "results equal --batch_size 1 byte for byte; speech_s2t then samples utterance i under its own key (--seed and i), the "
                        "same text for every N >= 2")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    _check_top_p(args)
    task = args.task.strip().lower()
    _check_repetition(args, task not in [t.lower() for t in UNDERSTANDING_TASKS])
    if task in [t.lower() for t in UNDERSTANDING_TASKS]:
        has_input = ((args.audio and os.path.isfile(args.audio)) or (args.audio_dir and os.path.isdir(args.audio_dir)) or
                     (args.reason_pt and args.semantic_pt and os.path.isfile(args.reason_pt) and os.path.isfile(args.semantic_pt)) or
                     (args.token_dir and os.path.isdir(args.token_dir)))
        if not has_input:
            raise ValueError("For understanding task provide --audio, --audio_dir, or --reason_pt + --semantic_pt.")
        if not args.llm_train_config or not args.text_tokenizer_path:
            raise ValueError("Set --llm_train_config and --text_tokenizer_path.")
        if not (args.prompt_text or (args.prompt_json and os.path.isfile(args.prompt_json))):
            raise ValueError("Set --prompt_text or --prompt_json.")
        run_understanding(args)
        return
    if task in [t.lower() for t in GENERATION_TASKS]:
        if task == "speech_s2s":
            if not ((args.audio and os.path.isfile(args.audio)) or (args.audio_dir and os.path.isdir(args.audio_dir)) or
                    (args.token_dir and os.path.isdir(args.token_dir))):
                raise ValueError("speech_s2s requires --audio, --audio_dir, or --token_dir (source reason/semantic .pt).")
        elif not ((args.text and args.text.strip()) or (args.text_file and os.path.isfile(args.text_file))):
            raise ValueError("For generation task provide --text or --text_file.")
        if not args.llm_train_config or not args.text_tokenizer_path:
            raise ValueError("Set --llm_train_config and --text_tokenizer_path.")
        if not (args.prompt_text or (args.prompt_json and os.path.isfile(args.prompt_json))):
            raise ValueError("Set --prompt_text or --prompt_json.")
        if args.stage in ("1", "all"):
            run_generation_stage1(args)
            if args.stage == "1":
                print("[Done] Stage 1 only. Run with --stage 2 --token_dir ... to decode to wav.")
                return
        # stage 2 decodes the token files rank 0 wrote, every rank its shard of the utterances (stage2_shard): the files must be
        # complete before any rank lists them
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()
        run_generation_stage2(args)
        return
    raise ValueError(f"Unsupported task: {task}. Understanding: {UNDERSTANDING_TASKS}. Generation: {GENERATION_TASKS}.")


if __name__ == "__main__":
    main()
