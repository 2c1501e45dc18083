"""Helpers of the fp8 weight-only tests: which tensors of a Model_stage3 state dict the option quantises, and the state dict of the
bf16 model it is defined against (every quantised tensor replaced by W' = q 2^e)."""
import torch


def is_quantised(key, tensor):
    """The five Linears of every layer of the four GPTs, projection, lm_head (2-D) and audio_head (3-D, [i] is [K, N]); never the embedding
    tables, the norms or anything else."""
    if key == "audio_head":
        return True
    return tensor.dim() == 2 and not key.endswith("wte.weight") and not key.startswith("audio_embeddings")


def w8_state_dict(sd):
    from uniaudio2_amd import ops
    out = {}
    for k, v in sd.items():
        if not is_quantised(k, v):
            out[k] = v.clone()
        elif k == "audio_head":
            out[k] = torch.stack([ops.dequant_w8(v[i].float().t().contiguous()).t().contiguous() for i in range(v.shape[0])]).to(v.dtype)
        else:
            out[k] = ops.dequant_w8(v.float()).to(v.dtype)
    return out
