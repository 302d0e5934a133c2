#!/usr/bin/env python3
"""The sample launch (ops.sample_rows, csrc/decode_sample.hip) against the torch chain it replaces, and the decode engine greedy against
sampled -- all in ONE process, appended to profiles/decode_sampling.jsonl:

  launch   rows in {1, 4, 16} x vocab in {32000, 50272, 128256}, fp16 logits, parameter sets greedy / temperature / top-k 50 / top-p 0.9 /
           both.  Device events around `--launches` back-to-back launches, `--repeats` windows, the two contenders alternating; per window
           the time per launch, reported as median and min .. max (the spread a difference has to exceed).
  torch    the same sampler as torch calls on the same logits: topk + masked_fill, sort + softmax + cumsum + mask + scatter, softmax,
           multinomial (argmax for greedy).
  engine   tok/s of the OPT-1.3B-shape random-init packed model (scripts/decode_engine_bench.py's build), free-running steps by graph
           replay, greedy and sampled alternating.

    python scripts/bench_sampling.py [--layers 24] [--tokens 256] [--skip-engine] [--out profiles/decode_sampling.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from quip_amd import decode, ops  # noqa: E402

DEV = torch.device("cuda:0")
SETS = [("greedy", 0.0, 0, 1.0), ("temperature", 0.8, 0, 1.0), ("top_k_50", 0.8, 50, 1.0), ("top_p_0.9", 0.8, 0, 0.9), ("top_k_50_top_p_0.9", 0.8, 50, 0.9)]


def torch_sampler(logits, T, k, p, gen):
    """Hugging Face's warpers and sampler as torch calls: temperature, TopKLogitsWarper, TopPLogitsWarper, multinomial"""
    if T <= 0:
        return torch.argmax(logits, -1)
    z = logits.float() / T
    if k:
        kth = torch.topk(z, k)[0][:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    if p < 1.0:
        srt, idx = torch.sort(z, descending=True)
        probs = torch.softmax(srt, -1)
        srt = srt.masked_fill(probs.cumsum(-1) - probs >= p, float("-inf"))
        z = torch.empty_like(z).scatter_(1, idx, srt)
    return torch.multinomial(torch.softmax(z, -1), 1, generator=gen)[:, 0]


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches                               # us per launch


def stats(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def bench_launch(a, emit):
    gen = torch.Generator(device=DEV).manual_seed(0)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for vocab in (32000, 50272, 128256):
        for rows in (1, 4, 16):
            logits = (4 * torch.randn(rows, vocab, generator=torch.Generator().manual_seed(vocab + rows))).to(torch.float16).to(DEV)
            out = torch.empty(rows, dtype=torch.int64, device=DEV)
            lp = torch.empty(rows, dtype=torch.float32, device=DEV)
            kn = torch.empty(rows, dtype=torch.int32, device=DEV)
            km = torch.empty(rows, dtype=torch.float32, device=DEV)
            for name, T, k, p in SETS:
                params = ops.sample_params(T, top_k=k, top_p=p, seed=1, device=DEV)
                ours = lambda: ops.sample_rows(logits, params, counter, out, lp, kn, km)
                theirs = lambda: torch_sampler(logits, T, k, p, gen)
                argmax = lambda: ops.argmax_rows(logits, out=out)
                for f in (ours, theirs, argmax):                             # warm-up: code objects, allocator
                    for _ in range(10):
                        f()
                torch.cuda.synchronize()
                t_ours, t_theirs, t_argmax = [], [], []
                for _ in range(a.repeats):                                   # alternating windows
                    t_ours.append(window(ours, a.launches))
                    t_theirs.append(window(theirs, max(a.launches // 4, 10)))
                    t_argmax.append(window(argmax, a.launches))
                rec = {"what": "launch", "rows": rows, "vocab": vocab, "params": name, "temperature": T, "top_k": k, "top_p": p,
                       "sample_rows": stats(t_ours), "torch_chain": stats(t_theirs), "argmax_rows": stats(t_argmax),
                       "kept_n": kn.tolist()[:4], "faster_beyond_spread": max(t_ours) < min(t_theirs)}
                emit(rec)


def bench_engine(a, emit):
    import decode_engine_bench as B
    ns = argparse.Namespace(arch="opt", layers=a.layers, bits=2, blocked=False)
    model, nbytes, arch = B.build(ns)
    s = decode.Sampling(0.8, top_k=50, top_p=0.95, seed=1)
    for bs in (1, 4):
        eng = decode.DecodeEngine(model, bs=bs, max_len=a.tokens + 16)
        res = {"greedy": [], "sampled": []}
        for rep in range(a.repeats):
            for name, setting in (("greedy", None), ("sampled", s)):
                eng.set_sampling(setting)
                eng.reset()
                eng.forward(torch.randint(0, 30000, (bs,), device=DEV))
                for _ in range(8):
                    eng.step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.tokens):
                    eng.step()
                torch.cuda.synchronize()
                res[name].append(bs * a.tokens / (time.perf_counter() - t0))
        emit({"what": "engine", "arch": arch, "layers": len(model.blocks), "engine_mode": eng.mode, "bs": bs, "tokens": a.tokens,
              "sampling": repr(s), "greedy_tok_per_s": {"median": round(float(np.median(res["greedy"])), 1), "min": round(min(res["greedy"]), 1),
                                                        "max": round(max(res["greedy"]), 1)},
              "sampled_tok_per_s": {"median": round(float(np.median(res["sampled"])), 1), "min": round(min(res["sampled"]), 1),
                                    "max": round(max(res["sampled"]), 1)}})
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_sampling.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit({"what": "run", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "launches": a.launches, "repeats": a.repeats})
        bench_launch(a, emit)
        if not a.skip_engine:
            bench_engine(a, emit)


if __name__ == "__main__":
    main()
