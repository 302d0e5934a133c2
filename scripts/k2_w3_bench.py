"""K2 on 3-bit codes: the 4-bit container (the kernels that served --wbits 3 before the STREAM3 layout existed) against the native
STREAM3 layout (csrc/dqgemm_w3.hip), the same codes, one process, the two alternated repetition by repetition.

    python scripts/k2_w3_bench.py [--out profiles/w3_native_vs_container.jsonl] [--launches 200] [--reps 7]

Cold regime as in bench.py: every launch of a repetition reads a different weight copy out of a ring larger than the 256 MiB last-level
cache, device events around the `launches` launches of a repetition, warm-up first.  fp16 x, fp32 y, qfn b.  One JSON line per
(shape, bs): us per launch for both (median, min, max over the repetitions), algorithmic bytes m d bits / 8 + 2 bs (d + m),
GB/s and the share of the 8 TB/s roof, and the ratio native / container.  The baseline is the container path, never the code under test."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_amd import _lib, ops  # noqa: E402

SHAPES = [(4096, 4096), (8192, 8192), (28672, 7168), (7168, 28672), (4096, 11008)]
LLC_BYTES = 256 << 20
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "w3_native_vs_container.jsonl"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--shapes", default="", help="m x d pairs, e.g. 4096x4096,8192x8192 (default: the five of the issue)")
    args = ap.parse_args()
    assert args.launches >= 200 and args.reps >= 5
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")] if args.shapes else SHAPES
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    lib = _lib.load()
    fn, vp = lib.quipamd_dequant_gemm, ctypes.c_void_p
    side = torch.cuda.Stream()
    st = vp(side.cuda_stream)
    for m, d in shapes:
        torch.manual_seed(m + d)
        codes = torch.randint(0, 8, (m, d), dtype=torch.uint8, device=dev)
        scale = torch.tensor([0.05], device=dev)
        forms = {}
        for name, layout, bits_stored in (("container", ops.LAYOUT_STREAM, 4), ("stream3", ops.LAYOUT_STREAM3, 3)):
            q = ops.pack(codes, 3, layout)
            nbytes = q.numel() * 4
            ncopy = max(2, -(-(LLC_BYTES + LLC_BYTES // 2) // nbytes))           # ring of 1.5 x the last-level cache
            forms[name] = dict(layout=layout, bits=bits_stored, ring=[q] + [q.clone() for _ in range(ncopy - 1)])
        del codes
        for bs in (1, 16):
            x = torch.randn(bs, d, device=dev).half()
            y = torch.empty((bs, m), dtype=torch.float32, device=dev)
            times = {name: [] for name in forms}

            def run(name, n, start):
                # straight through the C ABI (the wrapper's host time per call is longer than the small kernels)
                f = forms[name]
                ring = f["ring"]
                for i in range(n):
                    rc = fn(vp(x.data_ptr()), 1, vp(ring[(start + i) % len(ring)].data_ptr()), 3, f["layout"], 1, vp(scale.data_ptr()), vp(0), vp(0),
                            vp(y.data_ptr()), 0, 0, bs, m, d, st)
                    if rc:
                        raise RuntimeError(lib.quipamd_last_error())

            outs = {}
            with torch.cuda.stream(side):
                for name in forms:                                               # warm-up over the whole ring, and the two forms must agree
                    run(name, max(args.warmup, len(forms[name]["ring"])), 0)
                    outs[name] = y.clone()
                side.synchronize()
                agree = float((outs["stream3"].double() - outs["container"].double()).norm() / outs["container"].double().norm())
                assert agree < 1e-3, f"{m}x{d} bs {bs}: the two forms disagree ({agree:.2e})"
                for rep in range(args.reps):
                    for name in (("container", "stream3") if rep % 2 == 0 else ("stream3", "container")):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        # the launches are enqueued while a spin kernel holds the stream: they run back to back from the queue (bench.py)
                        torch.cuda._sleep(int(args.launches * 30000 + 300000))
                        run(name, 8, rep)
                        e0.record(side)
                        run(name, args.launches, rep + 8)
                        e1.record(side)
                        side.synchronize()
                        times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            rec = {"m": m, "d": d, "bs": bs, "x": "fp16", "y": "fp32", "launches": args.launches, "reps": args.reps, "agree_rel": agree}
            for name, f in forms.items():
                t = times[name]
                alg = m * d * f["bits"] // 8 + 2 * bs * (d + m)
                med = statistics.median(t)
                rec[name] = {"us_median": round(med, 3), "us_min": round(min(t), 3), "us_max": round(max(t), 3), "ring_copies": len(f["ring"]),
                             "algorithmic_bytes": alg, "GBps": round(alg / med / 1e3, 1), "roof_frac": round(alg / med / 1e3 / HBM_PEAK_GBS, 4)}
            rec["time_ratio_stream3_over_container"] = round(rec["stream3"]["us_median"] / rec["container"]["us_median"], 4)
            rec["byte_ratio"] = round(rec["stream3"]["algorithmic_bytes"] / rec["container"]["algorithmic_bytes"], 4)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del forms
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
