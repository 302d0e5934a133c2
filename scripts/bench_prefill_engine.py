#!/usr/bin/env python3
"""The prompt pass of the decode engine, measured (JSON lines appended to profiles/prefill_engine.jsonl):

    --ttft     time to first token: DecodeEngine.prefill(prompt) against the same engine fed through forward() token by token (the
               per-token graph replay), alternated within one run, three repeats each: min / median / max and the ratio of medians.
               OPT-1.3B and Llama-2-7B w2 twins (scripts/decode_engine_bench.py's builders), 1 and 8 sequences, prompts 128 / 512 / 2048.
    --kernel   quipamd_prefill_attention alone (append + attention launches): 1 and 8 sequences, T 512 / 2048 / 4096 at start 0,
               head_dim 128, 32 heads multi-head and 64 over 8 grouped: microseconds and FLOP/s from 4 bs heads hd T (T + 1) / 2 counted
               here, next to torch.nn.functional.scaled_dot_product_attention(is_causal=True) on the same tensors in the same run.
    --pass     one 2048-token prefill of a model, untimed, after a warm-up: the workload for `rocprofv3 --kernel-trace --stats -- python
               scripts/bench_prefill_engine.py --pass --arch llama` (the per-block split of operators / GEMMs / attention / glue is read
               off its kernel statistics).

Every timed window is synchronised at both ends and lasts at least 0.5 s (a shape that is faster is repeated inside its window);
every shape is warmed up first."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from quip_amd import decode, ops  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "prefill_engine.jsonl")
MIN_WINDOW = 0.5


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def window(fn, min_s=MIN_WINDOW):
    """seconds per call of fn over one synchronised window of at least min_s (the repeat count comes from a first timed call)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    reps = max(1, int(np.ceil(min_s / max(one, 1e-6))))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, reps


def stats(xs):
    return {"min": float(np.min(xs)), "median": float(np.median(xs)), "max": float(np.max(xs))}


# ------------------------------------------------------------------------------------------------------------------------ time to first token
def build(arch, layers):
    import decode_engine_bench as B
    a = types.SimpleNamespace(arch=arch, layers=layers, bits=2, blocked=False)
    return B.build(a)


def ttft(a):
    for arch in a.arch.split(","):
        model, nbytes, name = build(arch, a.layers)
        for bs in (1, 8):
            eng = decode.DecodeEngine(model, bs=bs, max_len=2048)
            for n in (128, 512, 2048):
                ids = torch.randint(0, 30000, (bs, n), device=DEV)

                def by_prefill():
                    eng.reset()
                    eng.prefill(ids)

                def by_token():
                    eng.reset()
                    for i in range(n):
                        eng.forward(ids[:, i])
                by_prefill(), by_token()                                     # warm-up of both paths at this shape
                tp, tt, reps = [], [], []
                for _ in range(3):                                           # alternate the two within the run
                    s, r = window(by_prefill)
                    tp.append(s), reps.append(r)
                    tt.append(window(by_token)[0])
                emit({"what": "ttft", "arch": name, "layers": len(model.blocks), "engine_mode": eng.mode, "bs": bs, "prompt": n,
                      "prefill_chunk": eng.prefill_chunk(), "prefill_s": stats(tp), "prefill_calls_per_window": reps,
                      "token_by_token_s": stats(tt), "speedup_of_medians": float(np.median(tt) / np.median(tp)),
                      "prefill_tok_per_s": bs * n / float(np.median(tp))}, a.out)
            del eng
        del model
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------ the kernel alone
def kernel(a):
    hd = 128
    for dtype in (torch.float16, torch.bfloat16):
        for heads, kv in ((32, 32), (64, 8)):
            for bs in (1, 8):
                for T in (512, 2048, 4096):
                    gen = torch.Generator().manual_seed(T + heads)
                    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)       # random data: zeros flatter an attention kernel
                    q, k, v = mk(bs * T, heads * hd), mk(bs * T, kv * hd), mk(bs * T, kv * hd)
                    kc, vc = torch.zeros(bs, kv, T, hd, dtype=dtype, device=DEV), torch.zeros(bs, kv, T, hd, dtype=dtype, device=DEV)
                    start = torch.zeros(1, dtype=torch.int64, device=DEV)
                    ours = lambda: ops.prefill_attention(q, k, v, kc, vc, start, T)
                    q4 = q.view(bs, T, heads, hd).transpose(1, 2)
                    k4, v4 = (t.view(bs, T, kv, hd).transpose(1, 2) for t in (k, v))
                    sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, is_causal=True, enable_gqa=kv != heads)
                    got, ref = ours(), sdpa().transpose(1, 2).reshape(bs * T, heads * hd)
                    err = float((got.float() - ref.float()).abs().max())
                    ours(), sdpa()
                    t_o, t_s = [], []
                    for _ in range(3):
                        t_o.append(window(ours)[0])
                        t_s.append(window(sdpa)[0])
                    flop = 4.0 * bs * heads * hd * T * (T + 1) / 2
                    emit({"what": "kernel", "dtype": str(dtype).split(".")[-1], "heads": heads, "kv_heads": kv, "hd": hd, "bs": bs, "T": T,
                          "prefill_attention_us": {k_: v_ * 1e6 for k_, v_ in stats(t_o).items()},
                          "torch_sdpa_causal_us": {k_: v_ * 1e6 for k_, v_ in stats(t_s).items()},
                          "flop": flop, "prefill_attention_TFLOPs": flop / float(np.median(t_o)) / 1e12,
                          "torch_sdpa_TFLOPs": flop / float(np.median(t_s)) / 1e12,
                          "time_ratio_ours_over_sdpa": float(np.median(t_o) / np.median(t_s)), "max_abs_diff_vs_sdpa": err}, a.out)
                    del q, k, v, kc, vc
                    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------------ one pass, for a trace
def one_pass(a):
    model, _, name = build(a.arch.split(",")[0], a.layers)
    eng = decode.DecodeEngine(model, bs=1, max_len=2048)
    ids = torch.randint(0, 30000, (1, 2048), device=DEV)
    eng.prefill(ids)                                                         # warm-up (tables, allocator)
    eng.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.prefill(ids)
    torch.cuda.synchronize()
    print(json.dumps({"what": "pass", "arch": name, "layers": len(model.blocks), "prompt": 2048, "seconds": time.perf_counter() - t0}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ttft", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--pass", dest="one_pass", action="store_true")
    ap.add_argument("--arch", default="opt,llama")
    ap.add_argument("--layers", type=int, default=0, help="0: the full model (24 / 32 blocks)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with torch.no_grad():
        if a.kernel:
            kernel(a)
        if a.ttft:
            ttft(a)
        if a.one_pass:
            one_pass(a)


if __name__ == "__main__":
    main()
