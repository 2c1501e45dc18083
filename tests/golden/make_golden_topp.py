#!/usr/bin/env python3
"""Generate the golden kept masks of the nucleus (top-p) filter by RUNNING THE REFERENCE's sample_top_p.

Container-only tool, like make_golden_lm.py: needs the reference on PYTHONPATH; only its output ``tests/golden/topp_mask.npz``
travels (a few KB).

llm_utils/sampling.py:66-82 sample_top_p sorts the probabilities, zeroes what its mask `probs_sum - probs_sort > p` removes,
renormalises and hands the result to the module-level `multinomial`.  That function is patched here to capture its argument: the
positions of `probs_sort` that are non-zero are the kept ones, and — the rows being tie-free — the descending sort maps them back
to columns without ambiguity.  Recorded: the probability rows (float32, as the function received them), the p values, and the kept
mask [rows, ps, V].  Every (row, p) decision is at least 1e-4 of the row's mass away from flipping (asserted here in float64), so
float32 cumsum noise does not decide any of them.

Usage:  PYTHONPATH=<reference checkout> python tests/golden/make_golden_topp.py
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
V = 48
PS = (0.1, 0.3, 0.5, 0.8, 0.95)
# (seed, scale of the logits): peaked rows and flat rows
ROWS = ((1, 4.0), (2, 2.0), (3, 1.0), (4, 0.25), (5, 8.0), (7, 0.05))


def main():
    import llm_utils.sampling as S

    captured = []

    def tap(input, num_samples, replacement=False, *, generator=None):
        captured.append(input.clone())
        return torch.zeros(*input.shape[:-1], 1, dtype=torch.long)

    S.multinomial = tap
    probs = []
    for seed, scale in ROWS:
        g = torch.Generator().manual_seed(seed)
        probs.append(torch.softmax(torch.randn(V, generator=g) * scale, dim=-1))
    probs = torch.stack(probs)
    assert all(torch.unique(r).numel() == V for r in probs), "rows must be tie-free"
    mask = np.zeros((len(ROWS), len(PS), V), dtype=bool)
    for j, p in enumerate(PS):
        del captured[:]
        S.sample_top_p(probs.clone(), p)
        kept_sorted = captured[0] > 0
        order = torch.sort(probs, dim=-1, descending=True).indices
        for i in range(len(ROWS)):
            mask[i, j, order[i][kept_sorted[i]].numpy()] = True
            pr = np.sort(probs[i].double().numpy())[::-1]
            s_gt = np.cumsum(pr) - pr
            assert np.abs(s_gt - p).min() > 1e-4, (i, p, np.abs(s_gt - p).min())
    out = os.path.join(HERE, "topp_mask.npz")
    np.savez_compressed(out, probs=probs.numpy(), ps=np.asarray(PS, dtype=np.float64), mask=mask)
    print(out, "kept sizes", mask.sum(-1).tolist())


if __name__ == "__main__":
    main()
