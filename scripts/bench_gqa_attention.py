#!/usr/bin/env python3
"""Grouped-query decode attention (quipamd_decode_attention_grouped, csrc/decode_gqa.hip) against the multi-head launch
(quipamd_decode_attention) on the cache repeated out to `heads` -- what serving a grouped-query model without the grouped launch
would take.  One JSON line per case: microseconds per launch from device events over many launches replayed from a hipGraph (warmed), the K / V
bytes the grouped launch must read (2 bs kv T hd 2) over that time as a fraction of 8 TB/s, and the same for the multi-head launch
(which reads g times as many bytes).  T = the number of cached positions attended to (pos = T - 1; maxlen = T).

usage: python scripts/bench_gqa_attention.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_amd import ops  # noqa: E402

HBM = 8e12


def _time(fn, iters, warmup, per_graph=20):
    """device time per launch: `per_graph` launches captured in one hipGraph (the host's per-call cost out of the picture), the graph
    replayed after `warmup` launches until `iters` launches ran, between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    g.replay()
    torch.cuda.synchronize()
    reps = max(1, iters // per_graph)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * per_graph)


def case(bs, heads, kv, hd, T, iters, warmup, dtype=torch.float16):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(bs * 1000 + heads + T)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dtype)
    q, k, v = mk(bs, heads * hd), mk(bs, kv * hd), mk(bs, kv * hd)
    kc, vc = mk(bs, kv, T, hd), mk(bs, kv, T, hd)
    pos = torch.tensor([T - 1], dtype=torch.int64, device=dev)
    ws = ops.decode_attention_grouped_workspace(bs, heads, kv, hd, T, dev)
    us_g = _time(lambda: ops.decode_attention_grouped(q, k, v, kc, vc, pos, workspace=ws), iters, warmup)
    # the multi-head launch on the repeated cache (repeat_kv) and repeated k / v
    rk, rv = kc.repeat_interleave(heads // kv, dim=1).contiguous(), vc.repeat_interleave(heads // kv, dim=1).contiguous()
    k2, v2 = k.view(bs, kv, hd).repeat_interleave(heads // kv, dim=1).reshape(bs, heads * hd), v.view(bs, kv, hd).repeat_interleave(heads // kv, dim=1).reshape(bs, heads * hd)
    us_m = _time(lambda: ops.decode_attention(q, k2, v2, rk, rv, pos), iters, warmup)
    o_g = ops.decode_attention_grouped(q, k, v, kc.clone(), vc.clone(), pos)
    o_m = ops.decode_attention(q, k2, v2, rk, rv, pos)
    torch.cuda.synchronize()
    byt = 2 * bs * kv * T * hd * 2
    return {"bs": bs, "heads": heads, "kv_heads": kv, "hd": hd, "T": T, "grouped_us": round(us_g, 2), "grouped_kv_bytes": byt,
            "grouped_frac_of_8TBps": round(byt / (us_g * 1e-6) / HBM, 3), "mha_repeated_us": round(us_m, 2),
            "mha_frac_of_8TBps": round(byt * heads // kv / (us_m * 1e-6) / HBM, 3), "speedup": round(us_m / us_g, 2),
            "max_abs_diff_vs_mha": float((o_g.float() - o_m.float()).abs().max())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    for bs in (1, 16):
        for heads, kv in ((64, 8), (32, 8)):
            for T in (512, 4096):
                print(json.dumps(case(bs, heads, kv, 128, T, a.iters, a.warmup)), flush=True)
