#!/usr/bin/env python3
"""The generate launch (ops.generate_rows, csrc/decode_generate.hip) against the sample launch it extends (ops.sample_rows), and the decode
engine with and without a decode.Generation -- all in ONE process, appended to profiles/decode_generation.jsonl:

  launch   50272 x fp16 logits, 1 and 16 rows, temperature 0.8 / top-k 50 / top-p 0.9; three cases of generate_rows, each next to sample_rows
           on the same logits in alternating windows:
             a  penalty 1, no history, no stop ids
             b  penalty 1.2 over a 2048-token history
             c  the same plus 4 stop ids, done and stop_pos
           Device events around `--launches` back-to-back launches, `--repeats` windows; per window the time per launch, reported as median
           and min .. max (the spread a difference has to exceed).
  engine   tok/s of the OPT-1.3B-shape random-init packed model (scripts/decode_engine_bench.py's build), free-running steps by graph
           replay: the engine with a Sampling against the engine with Generation(that Sampling, repetition_penalty 1.2, 4 stop ids that are
           never drawn), alternating.

    python scripts/bench_generation.py [--layers 24] [--tokens 256] [--skip-engine] [--out profiles/decode_generation.jsonl]"""
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
from bench_sampling import stats, window  # noqa: E402

DEV = torch.device("cuda:0")
VOCAB, HISTORY = 50272, 2048
T, K, P = 0.8, 50, 0.9


def bench_launch(a, emit):
    for rows in (1, 16):
        logits = (4 * torch.randn(rows, VOCAB, generator=torch.Generator().manual_seed(VOCAB + rows))).to(torch.float16).to(DEV)
        out = torch.empty(rows, dtype=torch.int64, device=DEV)
        lp = torch.empty(rows, dtype=torch.float32, device=DEV)
        kn = torch.empty(rows, dtype=torch.int32, device=DEV)
        km = torch.empty(rows, dtype=torch.float32, device=DEV)
        sp = ops.sample_params(T, top_k=K, top_p=P, seed=1, device=DEV)
        hist = torch.randint(0, VOCAB, (rows, HISTORY + 8), generator=torch.Generator().manual_seed(rows)).to(torch.int32).to(DEV)
        counter0 = torch.zeros(1, dtype=torch.int64, device=DEV)
        counter = torch.full((1,), HISTORY, dtype=torch.int64, device=DEV)           # 2048 positions of history are read, position 2048 is written
        stop_ids = torch.tensor([VOCAB + 1, VOCAB + 2, VOCAB + 3, VOCAB + 4], dtype=torch.int32, device=DEV)   # never drawn: every row keeps running
        done = torch.zeros(rows, dtype=torch.int32, device=DEV)
        stop_pos = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
        plain = ops.write_generate_params(ops.generate_params(rows, device=DEV), None, T, K, P, 1, 1.0)
        pen = ops.write_generate_params(ops.generate_params(rows, device=DEV), None, T, K, P, 1, 1.2)
        cases = {
            "a_penalty_1_no_stop": (lambda: ops.generate_rows(logits, plain, counter0, out=out, logprob=lp, kept_n=kn, kept_mass=km), counter0),
            "b_penalty_1.2_history_2048": (lambda: ops.generate_rows(logits, pen, counter, hist=hist, out=out, logprob=lp, kept_n=kn, kept_mass=km), counter),
            "c_penalty_1.2_history_2048_4_stop_ids": (lambda: ops.generate_rows(logits, pen, counter, hist=hist, stop_ids=stop_ids, done=done,
                                                                                 stop_pos=stop_pos, out=out, logprob=lp, kept_n=kn, kept_mass=km), counter),
        }
        for name, (ours, ctr) in cases.items():
            base = lambda: ops.sample_rows(logits, sp, ctr, out, lp, kn, km)
            for f in (ours, base):                                               # warm-up: code objects, the LDS attribute, allocator
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            t_ours, t_base = [], []
            for _ in range(a.repeats):                                           # alternating windows
                t_ours.append(window(ours, a.launches))
                t_base.append(window(base, a.launches))
            emit({"what": "launch", "case": name, "rows": rows, "vocab": VOCAB, "dtype": "float16", "temperature": T, "top_k": K, "top_p": P,
                  "generate_rows": stats(t_ours), "sample_rows": stats(t_base),
                  "ratio_of_medians": round(float(np.median(t_ours) / np.median(t_base)), 3),
                  "beyond_spread": min(t_ours) > max(t_base) or max(t_ours) < min(t_base)})


def bench_engine(a, emit):
    import decode_engine_bench as B
    ns = argparse.Namespace(arch="opt", layers=a.layers, bits=2, blocked=False)
    model, nbytes, arch = B.build(ns)
    s = decode.Sampling(T, top_k=K, top_p=0.95, seed=1)
    gen = decode.Generation(sampling=s, repetition_penalty=1.2, stop_ids=[(1 << 20) + i for i in range(4)])   # outside any vocabulary: never drawn
    for bs in (1, 4):
        eng = decode.DecodeEngine(model, bs=bs, max_len=a.tokens + 16)
        eng.set_sampling(s)
        res = {"sampled": [], "generation": []}
        for rep in range(a.repeats):
            for name, setting in (("sampled", None), ("generation", gen)):
                eng.set_generation(setting)
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
              "sampling": repr(s), "generation": repr(gen), "finished": eng.finished.tolist(),
              **{f"{k}_tok_per_s": {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in res.items()}})
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_generation.jsonl"))
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
