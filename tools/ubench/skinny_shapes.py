#!/usr/bin/env python3
"""Sweep of the batched-decode linear kernel (csrc/ua2_skinny.hip) over its tile parameters at the model's shapes,
beside round 2's skinny kernel and the tiled GEMM; every variant's output is compared bit for bit with the old kernel's.
The operand is handed over pre-packed (x_packed), so the numbers are the GEMM launch alone (no prep launch).
Usage on the GPU box: python tools/ubench/skinny_shapes.py [M ...]
                      python tools/ubench/skinny_shapes.py --w8 [M ...]   the fp8-weight form (ua2_linear_w8_many) beside the bf16 form on the twin W',
                                                                          default variant and the forced variants that have an fp8 form; M <= 64"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from uniaudio2_amd import ops
from uniaudio2_amd._lib import EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_CAST, lib

dev = torch.device("cuda")
dt = torch.bfloat16
L = 4
SHAPES = (("trunk qkv-sized", 5120, 3072, EPI_STORE), ("trunk oproj", 3072, 3072, EPI_RESIDUAL),
          ("trunk swiglu", 8192, 3072, EPI_SWIGLU), ("trunk down", 3072, 8192, EPI_RESIDUAL),
          ("dec qkv-sized", 3072, 2048, EPI_STORE), ("dec oproj", 2048, 2048, EPI_RESIDUAL),
          ("dec swiglu", 8192, 2048, EPI_SWIGLU), ("dec down", 2048, 8192, EPI_RESIDUAL),
          ("projection", 2048, 3072, EPI_STORE), ("audio_head", 12296, 2048, EPI_STORE), ("lm_head", 128256, 3072, EPI_STORE))
W8 = "--w8" in sys.argv[1:]
MS = [int(v) for v in sys.argv[1:] if v != "--w8"] or ([8, 16, 32, 64] if W8 else [64, 256])


def sweep_w8():
    """fp8 form against the bf16 form on the twin, per released Linear shape and row count: time of the GEMM launch alone (operand pre-packed).
    Both sides go through the same C-side chain (ua2_linear_chain_timed / ua2_linear_w8_many_chain_timed: all launches enqueued between two
    events by one C loop), over enough weight sets that one pass over them exceeds the 256 MB Infinity Cache even as fp8 (>= 320 MB of fp8
    images per pass: a launch finds its weights in HBM, as in the frame), in windows of >= 3000 launches (tens of ms); best of two windows,
    the two sides alternated.  Outputs compared bit for bit."""
    for name, N, K, epi in SHAPES:
        if N > 100000:
            continue                                        # lm_head: not a launch of the weights-stationary kernel
        nt = 2 if epi == EPI_SWIGLU else 1
        sets = max(4, -(-320_000_000 // (N * K * nt)))
        packs = [[ops.pack_linear_w8(torch.randn(N, K, device=dev) * 0.02) for _ in range(nt)] for _ in range(sets)]
        twins = [(p[0][:2], p[1][:2] if nt == 2 else None) for p in packs]
        iters = max(2, -(-3000 // sets))
        for M in MS:
            x, res = torch.randn(M, K, device=dev), torch.randn(M, N, device=dev)
            ws = ops.linear_workspace(dt, M, K, dev)
            y0 = torch.empty(M, N, device=dev)
            os.environ.pop("UA2_SKINNY2", None)
            ops.linear(dtype=dt, M=M, N=N, K=K, w0=packs[0][0][2], w1=packs[0][1][2] if nt == 2 else None, prologue=PRO_CAST, epilogue=epi, x=x, y=y0,
                       resid=res if epi == EPI_RESIDUAL else None, workspace=ws)          # fills ws with the packed operand; y0 = the bf16 form's result
            torch.cuda.synchronize()
            y = torch.zeros(M, N, device=dev)
            args = [ops.linear(dtype=dt, M=M, N=N, K=K, w0=p[0][2], w1=p[1][2] if nt == 2 else None, prologue=PRO_CAST, epilogue=epi, x_packed=ws, y=y,
                               resid=res if epi == EPI_RESIDUAL else None, launch=False) for p in packs]
            out = []
            forced = ["1,4,1,1", "1,2,2,1", "2,4,1,1", "2,2,2,1", "1,2,2,2", "2,2,2,2", "2,4,1,1,6", "2,4,2,1,6", "2,4,1,1,4"]
            for v in ["auto"] + forced:
                if v == "auto":
                    os.environ.pop("UA2_SKINNY2", None)
                else:
                    os.environ["UA2_SKINNY2"] = v
                y.zero_()
                try:
                    ops.linear_w8_many_chain_timed(args[:1], twins[:1], 1)
                except Exception:                           # no fp8 form of this variant for this geometry
                    continue
                torch.cuda.synchronize()
                same = bool(torch.equal(y, y0))
                try:                                        # the bf16 form under the same variant, where it is built
                    ops.linear_chain_timed(args[:1], 1)
                    has_bf16 = True
                except Exception:
                    has_bf16 = False
                t8, tb = [], []
                ops.linear_w8_many_chain_timed(args, twins, 1)          # warm-up pass of each side
                if has_bf16:
                    ops.linear_chain_timed(args, 1)
                for _ in range(2):
                    t8.append(ops.linear_w8_many_chain_timed(args, twins, iters) * 1e3)
                    if has_bf16:
                        tb.append(ops.linear_chain_timed(args, iters) * 1e3)
                out.append((v, min(t8), min(tb) if tb else float("nan"), same, abs(t8[0] - t8[1])))
            os.environ.pop("UA2_SKINNY2", None)
            auto = out[0]
            rest = sorted(out[1:], key=lambda r: r[1])[:5]
            wbytes = N * K * nt
            print(f"M={M:3d} {name:16s} N={N:6d} K={K:5d} sets {sets:3d} default: fp8 {auto[1]:6.2f} us (two windows differ by {auto[4]:.2f})  bf16 twin {auto[2]:6.2f} us  "
                  f"ratio {auto[1] / auto[2]:.2f}  fp8 image {wbytes / auto[1] / 1e6:.2f} TB/s{'' if auto[3] else '  (DIFF)'} | forced, fp8 / bf16 us: "
                  + ", ".join(f"{v}: {t8:.2f}/{tb:.2f}{'' if same else '(DIFF)'}" for v, t8, tb, same, _ in rest), flush=True)
            del args
        del packs, twins


def variants(M):
    mt = (M + 15) // 16
    out = ["off", "auto"]
    for ct in (1, 2):
        for mtw, la in ((4, 1), (4, 2), (2, 2)):
            ps = sorted({1, max(1, (mt + mtw - 1) // mtw), max(1, (mt + 2 * mtw - 1) // (2 * mtw)), max(1, (mt + 4 * mtw - 1) // (4 * mtw))})
            for p in ps:
                out.append(f"{ct},{mtw},{la},{p}")
    # round 6: weight-ring forms (one pass, grid.y = row tiles / mt): "ct,mt,la,1,wd"
    out += ["2,4,1,1,6", "2,4,2,1,6", "2,4,1,1,4", "2,4,1,1,3", "2,2,2,1,4",                       # SwiGLU
            "2,2,2,1,8", "2,4,1,1,8", "3,2,2,1,4", "4,2,2,1,4",                                   # RESIDUAL (+ 2,2,2,1,4 / 2,4,1,1,4)
            "3,2,2,1,6", "4,2,2,1,6", "4,2,2,1,4", "4,4,1,1,4", "3,4,1,1,6", "3,4,1,1,4"]         # STORE / q|k|v
    out += ["1,4,4,1,0,2", "1,4,1,1,0,2", "1,2,4,2,0,2", "1,2,4,1,0,2"]      # two ranges per wave (K = 8192)
    return out


if W8:
    sweep_w8()
    sys.exit(0)

for M in MS:
    for name, N, K, epi in SHAPES:
        if N > 100000 and M > 64:
            Lw = 1
        else:
            Lw = L if N < 100000 else 2
        w0 = [ops.pack_linear(torch.randn(N, K, device=dev) * 0.02, dt) for _ in range(Lw)]
        w1 = [ops.pack_linear(torch.randn(N, K, device=dev) * 0.02, dt) for _ in range(Lw)] if epi == EPI_SWIGLU else [None] * Lw
        x = torch.randn(M, K, device=dev)
        res = torch.randn(M, N, device=dev)
        ws = ops.linear_workspace(dt, M, K, dev)
        # one ordinary launch fills the workspace with the packed operand; reuse it as x_packed
        os.environ["UA2_SKINNY_MAX_ROWS"] = "100000"
        os.environ["UA2_SKINNY2"] = "off"
        y0 = torch.empty(M, N, device=dev)
        lib.ua2_debug_force_general_linear(4)
        ops.linear(dtype=dt, M=M, N=N, K=K, w0=w0[0], w1=w1[0], prologue=PRO_CAST, epilogue=epi, x=x, y=y0,
                   resid=res if epi == EPI_RESIDUAL else None, workspace=ws)
        lib.ua2_debug_force_general_linear(0)
        torch.cuda.synchronize()
        results = []
        for v in variants(M) + ["tiled"]:
            if v == "tiled":
                os.environ["UA2_SKINNY_MAX_ROWS"] = "0"
                os.environ["UA2_SKINNY2"] = "off"
            elif v == "auto":
                os.environ["UA2_SKINNY_MAX_ROWS"] = "100000"
                os.environ.pop("UA2_SKINNY2", None)
            else:
                os.environ["UA2_SKINNY_MAX_ROWS"] = "100000"
                os.environ["UA2_SKINNY2"] = v
            y = torch.zeros(M, N, device=dev)
            try:
                args = [ops.linear(dtype=dt, M=M, N=N, K=K, w0=a, w1=b, prologue=PRO_CAST, epilogue=epi, x_packed=ws, y=y,
                                   resid=res if epi == EPI_RESIDUAL else None, launch=False) for a, b in zip(w0, w1)]
                ops.linear_chain_timed(args[:1], 1)
                torch.cuda.synchronize()
                same = bool(torch.equal(y, y0))
                ops.linear_chain_timed(args, 3)
                t = ops.linear_chain_timed(args, 10) * 1e3
            except Exception as e:      # variant not instantiated for this geometry
                continue
            results.append((t, v, same))
        base = [r for r in results if r[1] == "off"][0][0]
        tl = [r for r in results if r[1] == "tiled"]
        results.sort()
        wbytes = N * K * 2 * (2 if epi == EPI_SWIGLU else 1)
        best = ", ".join(f"{v}:{t:.1f}{'' if same else '(DIFF)'}" for t, v, same in results[:8])
        bad = [v for _, v, same in results if not same]
        print(f"M={M:4d} {name:16s} N={N:6d} K={K:5d} old {base:7.1f} us | tiled {tl[0][0] if tl else float('nan'):7.1f} | best: {best} | "
              f"W/best {wbytes/results[0][0]/1e6:.2f} TB/s | mismatches: {bad}", flush=True)
        del w0, w1
