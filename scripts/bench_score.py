"""Timing and peak memory of the scoring path; one JSON line per shape, printed and appended to profiles/head_score.jsonl.

  (a) ops.head_score against the torch chain it replaces -- F.linear -> .float() log_softmax -> gather + argmax -- at rows = 2048, fp16,
      (h, vocab) = (2048, 50272), (4096, 32000), (7168, 50272).  The two arms alternate inside one process, every call between two
      device events, after a warm-up; median, min and max over the rounds; the peak of torch.cuda.max_memory_allocated() above the
      baseline for one call of each arm.  Inputs x ~ N(0, 1), W ~ N(0, 1 / h) (random data: a zero fill would flatter both arms).
  (b) DecodeEngine.loglikelihood over synthetic ragged requests on the OPT-1.3B-shape packed (2-bit) model against the same loop with
      prefill(all_logits=True) and the chain above; host clock around each whole call, which ends in a device-to-host copy.

    python scripts/bench_score.py [--rounds 20] [--skip-engine] [--layers 24]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from quip_amd import ops, decode  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "head_score.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def chain(x, W, t):
    lg = F.linear(x, W)
    lp = torch.log_softmax(lg.float(), dim=-1)
    return lp.gather(1, t[:, None])[:, 0], lg.argmax(dim=-1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def bench_op(rows, h, vocab, rounds):
    g = torch.Generator().manual_seed(h + vocab)
    x = torch.randn(rows, h, generator=g).half().to(DEV)
    W = (torch.randn(vocab, h, generator=g) / h ** 0.5).half().to(DEV)
    t = torch.randint(0, vocab, (rows,), generator=g).to(DEV)
    ws = ops.head_score_workspace(rows, vocab, DEV)
    out = (torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, dtype=torch.int64, device=DEV))
    fused = lambda: ops.head_score(x, W, t, out=out, workspace=ws)
    ref = lambda: chain(x, W, t)
    for _ in range(3):
        fused(), ref()
    torch.cuda.synchronize()
    lp, _, gr = fused()
    lp_c, gr_c = ref()
    diff = (lp - lp_c).abs().max().item()
    same = (gr == gr_c).double().mean().item()
    tf, tc = [], []
    for _ in range(rounds):                                   # alternating: both arms see the same clocks and the same neighbours
        tf.append(timed(fused))
        tc.append(timed(ref))
    flop = 2.0 * rows * h * vocab
    rec = {"bench": "head_score_op", "dtype": "fp16", "rows": rows, "h": h, "vocab": vocab, "rounds": rounds,
           "head_score": stats(tf), "chain": stats(tc),
           "head_score_tflops": round(flop / np.median(tf) / 1e9, 1), "chain_tflops": round(flop / np.median(tc) / 1e9, 1),
           "speedup_median": round(float(np.median(tc) / np.median(tf)), 3),
           "head_score_peak_bytes": peak_of(fused) + ws.numel(), "chain_peak_bytes": peak_of(ref),
           "max_abs_logprob_diff": diff, "greedy_agreement": same}
    emit(rec)


def synthetic_requests(n, max_len, vocab, seed=0):
    g = torch.Generator().manual_seed(seed)
    reqs = []
    for _ in range(n):
        c = int(torch.randint(32, max_len - 16, (1,), generator=g))
        k = int(torch.randint(1, 17, (1,), generator=g))
        reqs.append((torch.randint(1, vocab, (c,), generator=g).tolist(), torch.randint(1, vocab, (k,), generator=g).tolist()))
    return reqs


@torch.no_grad()
def chain_loglikelihood(eng, requests):
    """DecodeEngine.loglikelihood's loop with the logits materialised: prefill(all_logits=True), then the torch chain"""
    out = [None] * len(requests)
    for b in decode.collate_requests(requests, eng.bs, eng.max_len):
        eng.reset()
        tg = b.targets.to(eng.dev)
        lg = eng.prefill(b.ids.to(eng.dev), all_logits=True)
        lp = torch.log_softmax(lg.float(), dim=-1).gather(2, tg.clamp(min=0)[..., None])[..., 0]
        lp = torch.where(tg < 0, torch.zeros_like(lp), lp)
        hit = ((lg.argmax(dim=-1) == tg) | (tg < 0)).all(dim=1)
        both = torch.stack([lp.double().sum(dim=1), hit.double()], dim=1).cpu()
        for r in range(b.real):
            out[b.index[r]] = (float(both[r, 0]), bool(both[r, 1] != 0))
    eng.reset()
    return out


def bench_engine(layers, rounds):
    import decode_opt as D
    bs, max_len, nreq, vocab = 8, 512, 64, 50272
    dec = D.Decoder(layers=layers, h=2048, ffn=8192, heads=32, vocab=vocab, maxpos=2048, dtype=torch.float16).to(DEV).eval()
    torch.manual_seed(0)
    for p_ in dec.parameters():
        p_.data.normal_(0, 0.02) if p_.dim() > 1 else p_.data.add_(0.05 * torch.randn_like(p_))
    D.pack_model(dec, 2, DEV, twin=False)
    eng = decode.DecodeEngine(dec, bs=bs, max_len=max_len)
    reqs = synthetic_requests(nreq, max_len, vocab)
    fused = lambda: eng.loglikelihood(reqs)
    ref = lambda: chain_loglikelihood(eng, reqs)
    a, b = fused(), ref()                                     # warm-up of both arms, and the two answers side by side
    diff = max(abs(u[0] - v[0]) for u, v in zip(a, b))
    tf, tc = [], []
    for _ in range(rounds):
        for arm, ts in ((fused, tf), (ref, tc)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            ts.append((time.perf_counter() - t0) * 1e3)
    emit({"bench": "loglikelihood", "model": f"OPT-1.3B shape, {layers} layers, 2-bit packed", "mode": eng.mode, "bs": bs, "max_len": max_len,
          "requests": nreq, "tokens_fed": int(sum(b_.ids.numel() for b_ in decode.collate_requests(reqs, bs, max_len))), "rounds": rounds,
          "loglikelihood": stats(tf), "all_logits_loop": stats(tc), "speedup_median": round(float(np.median(tc) / np.median(tf)), 3),
          "loglikelihood_peak_bytes": peak_of(fused), "all_logits_loop_peak_bytes": peak_of(ref), "max_abs_sum_diff": diff,
          "flags_equal": sum(u[1] == v[1] for u, v in zip(a, b))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--skip-engine", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score.py needs a GPU: there is nothing to time without one")
    for h, vocab in ((2048, 50272), (4096, 32000), (7168, 50272)):
        bench_op(2048, h, vocab, args.rounds)
    if not args.skip_engine:
        bench_engine(args.layers, max(3, args.rounds // 4))


if __name__ == "__main__":
    main()
