#!/usr/bin/env python3
"""Timing of the group-wise fused dequant-GEMM (ops.dequant_gemm_groupwise, csrc/dqgemm_gw.hip); one JSON line per case, printed and
appended to profiles/dqgemm_groupwise.jsonl.

Rows 1 / 16 / 256; shapes (m x d) 4096 x 4096, 11008 x 4096, 4096 x 11008, 8192 x 8192; w4 / g128, w3 / g128, w2 / g64; fp16 activations,
fp16 y.  Three legs on the same seeded inputs:
  (a) groupwise   the new kernel;
  (b) dense       what such a layer ran before it could be packed: F.linear on the fp16 fake-quant weight scale * (code - zero);
  (c) per_row     ops.dequant_gemm qfn 'a' on the same codes with ONE (scale, zero) per row -- a different function of the codes, timed
                  for the price of the groups alone.
Each leg is one hipGraph of `--steps` launches that walk a ring of weight copies larger than the 256 MiB Infinity Cache (every launch
streams its weights from HBM, as a decode step does); the three graphs are replayed in turn, `--rounds` times, and the median per launch
is reported.  bytes = codes + tables + x + y of leg (a); GB/s of every leg is ITS OWN algorithmic bytes over its median.
Leg (a) is checked against the fp64 formula before anything is timed.  No GPU: the script fails, it does not fall back.

    python scripts/bench_groupwise.py [--steps 48] [--rounds 7] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quip_amd import ops  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "dqgemm_groupwise.jsonl")
RING_BYTES = 320 << 20                                       # per leg: more than the Infinity Cache


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def make_case(m, d, bits, G, seed):
    g = torch.Generator().manual_seed(seed)
    maxq = 2 ** bits - 1
    codes = torch.randint(0, maxq + 1, (m, d), generator=g, dtype=torch.uint8).to(DEV)
    scale = (0.01 * 10.0 ** torch.rand(m, d // G, generator=g)).to(DEV)
    zero = torch.randint(0, maxq + 1, (m, d // G), generator=g).float().to(DEV)
    return codes, scale, zero


def ring_of(tensors, nbytes):
    """copies of a tuple of tensors until the ring holds more than RING_BYTES"""
    n = max(2, min(64, RING_BYTES // max(nbytes, 1) + 1))
    return [tensors] + [tuple(t.clone() for t in tensors) for _ in range(n - 1)]


def capture(launch, ring, steps):
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for i in range(min(3, len(ring))):
            launch(*ring[i])
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for i in range(steps):
                launch(*ring[i % len(ring)])
    graph.replay()
    torch.cuda.synchronize()
    return graph


def replay_us(graph, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def bench_case(m, d, bits, G, rows_list, steps, rounds):
    codes, scale, zero = make_case(m, d, bits, G, seed=m + d + bits)
    qs = ops.pack(codes, bits, ops.LAYOUT_STREAM)
    gs, gz = ops.group_tables(scale, zero)
    Wd = (scale.repeat_interleave(G, dim=1) * (codes.float() - zero.repeat_interleave(G, dim=1))).half()       # the fake-quant weight
    srow, zrow = scale[:, 0].contiguous(), zero[:, 0].contiguous()
    cb = ops.container_bits(bits)
    code_bytes, tab_bytes = m * d * cb // 8, 2 * (d // G) * m * 4
    rings = {"groupwise": ring_of((qs, gs, gz), code_bytes + tab_bytes), "dense": ring_of((Wd,), m * d * 2),
             "per_row": ring_of((qs, srow, zrow), code_bytes + 8 * m)}
    del codes
    for rows in rows_list:
        x = torch.randn(rows, d, generator=torch.Generator().manual_seed(rows)).half().to(DEV)
        y = torch.empty(rows, m, dtype=torch.float16, device=DEV)
        io = rows * d * 2 + rows * m * 2
        legs = {"groupwise": (lambda q, s, z: ops.dequant_gemm_groupwise(x, q, bits, G, s, z, None, out=y, m=m), code_bytes + tab_bytes + io),
                "dense": (lambda W: F.linear(x, W), m * d * 2 + io),
                "per_row": (lambda q, s, z: ops.dequant_gemm(x, q, bits, 'a', s, z, None, out=y, m=m), code_bytes + 8 * m + io)}
        # parity of leg (a) first: fp64 on the 16-bit x, against the fp16-rounded dense weight's fp32 original
        ref = x.double() @ (scale.repeat_interleave(G, dim=1).double() * (ops.unpack(qs, bits, ops.LAYOUT_STREAM, m, d).double()
                                                                          - zero.repeat_interleave(G, dim=1).double())).T
        got = ops.dequant_gemm_groupwise(x, qs, bits, G, gs, gz, None, out_dtype=torch.float32, m=m).double()
        err = float((got - ref).norm() / ref.norm())
        del ref, got
        graphs = {k: capture(fn, rings[k], steps) for k, (fn, _) in legs.items()}
        times = {k: [] for k in legs}
        for _ in range(rounds):                              # the legs alternate: same clocks, same neighbours
            for k in legs:
                times[k].append(replay_us(graphs[k], steps))
        med = {k: float(np.median(v)) for k, v in times.items()}
        rec = {"bench": "dqgemm_groupwise", "m": m, "d": d, "bits": bits, "groupsize": G, "rows": rows, "act": "fp16", "steps": steps, "rounds": rounds,
               "rel_err_fp32_y": err, "bytes": legs["groupwise"][1]}
        for k, (_, nb) in legs.items():
            rec[k] = {"median_us": round(med[k], 2), "min_us": round(float(np.min(times[k])), 2), "max_us": round(float(np.max(times[k])), 2),
                      "bytes": nb, "gbps": round(nb / med[k] / 1e3, 1)}
        rec["dense_over_groupwise"] = round(med["dense"] / med["groupwise"], 3)
        rec["groupwise_over_per_row"] = round(med["groupwise"] / med["per_row"], 3)
        emit(rec)
        del graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, w4 / g128 only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_groupwise.py needs a GPU: there is nothing to time without one")
    shapes = [(4096, 4096)] if args.quick else [(4096, 4096), (11008, 4096), (4096, 11008), (8192, 8192)]
    configs = [(4, 128)] if args.quick else [(4, 128), (3, 128), (2, 64)]
    for m, d in shapes:
        for bits, G in configs:
            if d % ops.stream_chunk(bits):                    # (11008 = 43 x 256: every listed shape fits every width)
                continue
            bench_case(m, d, bits, G, (1, 16, 256), args.steps, args.rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
