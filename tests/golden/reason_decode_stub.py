"""Stand-ins and seeded inputs shared by tests/golden/make_golden_reason_decode.py (which runs the REFERENCE's
ReasoningTokenizer.token2audio and AudioDiffusion1D.inference_codes with codes = [reason, rec] on them) and by the tests
(which run the product on the same stand-ins and never touch the reference).  Test data plumbing only."""
import torch

from codec_model_stub import CFG
from tokenizer_stub import StubModel
from weights import seeded_tensor

T_CASES = (1, 250, 375, 376, 700, 1200)          # rec codes: one window short / exact, one code over, 3 and 4 windows
SEED = 4321
WAVE_STRIDE = 997                                # the fixture keeps every 997th sample + float64 checksums
INFER = dict(T=25, T_q=11, latent_length=44, incontext=12, card=32)    # 11 x 2.5 = 27 rows: feature_combine crops to 25


def reason_len(T):
    return int(T * 0.4) + 1


def make_reason_codes(T_q):
    """(1, 8, T_q) int64, every entry distinct and different from tokenizer_stub.make_codes' values."""
    t = torch.arange(T_q, dtype=torch.int64)
    return torch.stack([(t * 8 + l) * 3 % 4096 + 1 for l in range(8)]).unsqueeze(0)


class StubReasonModel(StubModel):
    """StubModel (latents from the rec codes and `true_latents` only) that also records the reason window codes_input[0].
    The latents do not depend on the reason codes, so the waves of the reference (whose windows k >= 1 all take reason codes
    [0, 150)) and of the product (which advances them) can be compared bit for bit while the reason windows differ.
    **kw absorbs the reference's `return_reasoning_text=` of its second and later windows (reason_tokenizer.py:201)."""

    def __init__(self):
        super().__init__()
        self.reason_windows = []

    def inference_codes(self, codes_input, spk_embeds, true_latents, latent_length, incontext_length, additional_feats=None,
                        guidance_scale=1.5, num_steps=20, disable_progress=True, scenario="other_seg", **kw):
        assert len(codes_input) == 2
        self.reason_windows.append(codes_input[0].detach().cpu().clone())
        return super().inference_codes(codes_input, spk_embeds, true_latents, latent_length, incontext_length, additional_feats,
                                       guidance_scale, num_steps, disable_progress, scenario)


class NoisyStubReasonModel(StubReasonModel):
    """The stand-in with the real model's second source of randomness: `prepare_latents` (AudioDiffusion1D.py:651-656)
    draws the start noise inside inference_codes unless the caller hands it in."""

    def prepare_latents(self, batch_size, num_frames, dtype, device):
        return torch.randn(batch_size, num_frames, self.sq_codec_latent, device=device, dtype=torch.float32)

    def inference_codes(self, codes_input, spk_embeds, true_latents, latent_length, incontext_length, noise=None, **kw):
        if noise is None:
            noise = self.prepare_latents(codes_input[-1].shape[0], latent_length, torch.float32, true_latents.device)
        lat = super().inference_codes(codes_input, spk_embeds, true_latents, latent_length, incontext_length, **kw)
        lat = lat + 0.01 * noise.to(lat.device)
        if incontext_length > 0:
            lat[:, :incontext_length] = true_latents[:, :incontext_length].float()
        return lat


def infer_reason_inputs():
    """Two-stream inference_codes at the codec_model_stub toy widths (D 256, latent 24)."""
    c, i = CFG, INFER
    B, T, D, L = 1, i["T"], c["D"], c["latent"]
    g = torch.Generator().manual_seed(521)
    return dict(codes=torch.randint(0, i["card"], (B, 8, T), generator=g), reason=torch.randint(0, i["card"], (B, 8, i["T_q"]), generator=g),
                tab_phone=seeded_tensor((1, i["card"], D), 522, std=0.5), tab_sem=seeded_tensor((1, i["card"], D), 523, std=0.5),
                tab_ac=seeded_tensor((6, i["card"], D), 524, std=0.3), tab_reason=seeded_tensor((8, i["card"], D), 525, std=0.3),
                noise=seeded_tensor((B, 2 * T, L), 526, std=1.0), first_latent=seeded_tensor((B, 2 * T, L), 527, std=1.0),
                true_latent=seeded_tensor((B, 2 * T, L), 528, std=1.0), zero_cond=seeded_tensor((D,), 529, std=0.5),
                latent_length=i["latent_length"], incontext=i["incontext"])
