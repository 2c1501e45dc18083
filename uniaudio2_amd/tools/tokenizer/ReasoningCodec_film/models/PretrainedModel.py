"""The frozen BEST-RQ feature extractor of the codec's tokenizer.

Mirror of the reference's tools/tokenizer/ReasoningCodec_film/models/PretrainedModel.py `BESTRQ_Model` (:12-62) for the one method the
token path calls, `extract_continous_embeds_multiple` (AudioDiffusion1D.py:503): `layers` (the codec passes [4, 11], AudioDiffusion1D.py:238) pick two entries of the encoder's
`hidden_states` — the acoustic and the semantic stream — returned as (B, D, T25).  The encoder is
modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm/model/musicfm_25hz.py on the HIP kernels; fairseq is not needed."""
import torch
import torch.nn as nn

from ..modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz import MusicFM25Hz


class BESTRQ_Model(nn.Module):
    def __init__(self, model_dir="modules/our_MERT_BESTRQ/mert_fairseq", checkpoint_dir="", output_features="continous", layers=(4, 11),
                 model=None, device="cuda", dtype=torch.float32):
        """checkpoint_dir: the MusicFM checkpoint FILE (MusicFM25Hz.from_checkpoint); or pass a built `model` (tests).  `dtype`: plan
        of the conformer's GEMMs — torch.float32, what the reference computes in (AudioDiffusion1D.py:502), or torch.bfloat16 (opt-in, faster).
        `layers` defaults to the codec's call site, not to the reference class's own default [3, 11]."""
        super().__init__()
        if len(layers) != 2:
            raise NotImplementedError("extract_continous_embeds_multiple takes two layers (acoustic, semantic)")
        self.layers = [int(l) for l in layers]
        if model is None:
            if not checkpoint_dir:
                raise ValueError("BESTRQ_Model needs a checkpoint file (checkpoint_dir=) or a built MusicFM25Hz (model=): "
                                 "it never runs on random weights silently")
            model = MusicFM25Hz.from_checkpoint(checkpoint_dir, taps=tuple(self.layers))
        if tuple(model.taps) != tuple(self.layers):
            raise ValueError(f"the encoder returns hidden_states {model.taps}, layers = {self.layers} asked")
        self.model = model.to(device).prepare(dtype)

    @torch.inference_mode()
    def extract_continous_embeds_multiple(self, input_audio):
        """input_audio (B, N) or (B, 1, N) fp32 at 24 kHz -> (acoustic, semantic), each (B, D, N // 960) fp32."""
        acoustic, semantic = self.model(input_audio.float())
        return acoustic.permute(0, 2, 1).contiguous(), semantic.permute(0, 2, 1).contiguous()
