#!/usr/bin/env python3
"""In-situ phase stamps of the HEADLINE launch (dq_h_kernel, 4 waves x 4 adjacent chunks) on the probe build of the library (csrc/probe.h):
every launch streams a different cold weight copy out of a ring (> Infinity Cache), runs alone, and leaves slot i of its four waves in the
probe buffer.  VERDICT r5 next #3: "re-stamp the CURRENT 4 x 4 kernel -- the meet figure is from round-2 code", and "why is 8192 x 2048 (half
the x) not faster cold".  Medians over the launches, clocks since the first wave's first stamp: first wave .. last wave."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# QUIP_AMD_LIB, when set, names another probe build: `python __graft_entry__.py --variant probe_nch -DQA_PROBE -DK2_AHEAD=99` is the
# "request everything, then consume" schedule next to the shipped one (profiles/k2h_pipeline.md)
os.environ.setdefault("QUIP_AMD_LIB", os.path.join(ROOT, "quip_amd", "csrc", "libquip_amd_probe.so"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from quip_amd import _lib, ops  # noqa: E402

NAMES = ["start", "every request issued (weights, then the x slabs)", "first chunk landed (wait -> first dequant)", "last chunk landed",
         "last MFMA issued", "partials parked in LDS", "block barrier passed", "reduce + epilogue + store issued"]


def run(m, d, bs, dt, launches=48, warm=False, cfg=None):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 4, (m, d), generator=g, dtype=torch.uint8).to(dev)
    q0 = ops.pack(codes, 2, ops.LAYOUT_STREAM)
    nring = 1 if warm else max(2, (400 << 20) // (m * d // 4) + 1)
    ring = [q0] + [q0.clone() for _ in range(nring - 1)]
    x = torch.randn(bs, d, generator=g).to(dt).to(dev)
    y = torch.empty(bs, m, dtype=dt, device=dev)
    sc = torch.tensor([0.05], device=dev)
    buf = torch.zeros(256, dtype=torch.int64, device=dev)
    _lib.call("quipamd_probe_set", buf.data_ptr())
    for i in range(nring):                                              # one walk: pages mapped, data long evicted again when its turn comes
        ops.dequant_gemm(x, ring[i], 2, "b", sc, None, None, out=y, cfg=cfg)
    torch.cuda.synchronize()
    rows = []
    for i in range(launches):
        buf.zero_()
        torch.cuda.synchronize()
        ops.dequant_gemm(x, ring[i % nring], 2, "b", sc, None, None, out=y, cfg=cfg)
        torch.cuda.synchronize()
        st = buf.cpu().numpy().astype(np.int64).reshape(16, 16)
        live = st[:, 0] > 0
        t0 = st[live][:, 0].min()
        rows.append(np.stack([np.where(st[live][:, k] > 0, st[live][:, k] - t0, -1) for k in range(16)], 1))
    _lib.call("quipamd_probe_set", None)
    a = np.stack(rows)                                                   # [launch, wave, slot]
    print(f"\n{'kernel cfg ' + str(cfg) if cfg else 'default kernel'}: {m} x {d}, bs {bs}, {str(dt).split('.')[-1]}, {'WARM (one copy)' if warm else f'COLD (ring of {nring} copies)'}: {a.shape[1]} waves stamped in workgroup 5, "
          f"median over {launches} launches; clocks (us at 2.4 GHz)")
    prev = 0
    for k in range(8):
        lo, hi = np.median(a[:, :, k].min(1)), np.median(a[:, :, k].max(1))
        print(f"  {k} {NAMES[k]:<52} {lo:7.0f} .. {hi:7.0f}   (+{hi - prev:6.0f} on the last wave; {hi / 2400:5.2f} us)")
        prev = hi
    # slot 12 (dq_h_body.inc): immediately in front of the first weight request -- the head of the launch: what a wave spends between its
    # start and the request whose HBM round trip everything else waits for (profiles/k2h_head.md)
    if (a[:, :, 12] > 0).any():
        hd = a[:, :, 12] - a[:, :, 0]                                    # per wave: its own start -> its own first weight request
        print(f"  head: own start -> first weight request, per wave: median {np.median(hd):6.0f}, first wave {np.median(hd.min(1)):6.0f}, "
              f"last wave {np.median(hd.max(1)):6.0f}; first weight request of the last wave at {np.median(a[:, :, 12].max(1)):6.0f}")
    # slots 8 + i / 12 + i (dq_h_body.inc, chunks 0..3; behind chunk 0's wait: slot 2, which sits right behind it): in front of / behind the counted vmcnt wait of chunk i.  Per wave: the time STALLED in the
    # wait, and the time in INSTRUCTIONS from that wait to the next one (ds_read, dequant, MFMA, the requests issued between the steps) --
    # the two numbers the single "last chunk landed" stamp used to add up.
    if (a[:, :, 8:16] > 0).any():
        nxt = [9, 10, 11, 4]                                             # what follows chunk i's arithmetic: the next wait, or "last MFMA issued"
        print("  chunk: wait reached at / stalled in the wait / instructions to the next wait -- median over launches of the per-launch "
              "median wave (of the last wave)")
        st_sum = in_sum = 0.0
        for i in range(4):
            behind = 2 if i == 0 else 12 + i
            if not (a[:, :, behind] > 0).any():
                continue
            reach, stall, instr = a[:, :, 8 + i], a[:, :, behind] - a[:, :, 8 + i], a[:, :, nxt[i]] - a[:, :, behind]
            last = a[:, :, 4].argmax(1)                                  # the wave that issues its last MFMA last
            pick = lambda v: np.median(v[np.arange(len(last)), last])
            print(f"    chunk {i}: {np.median(np.median(reach, 1)):7.0f} ({pick(reach):7.0f})   stalled {np.median(np.median(stall, 1)):6.0f} ({pick(stall):6.0f})"
                  f"   instructions {np.median(np.median(instr, 1)):6.0f} ({pick(instr):6.0f})")
            st_sum += pick(stall)
            in_sum += pick(instr)
        print(f"    last wave, chunks 0..3: {st_sum:.0f} clocks stalled in waits, {in_sum:.0f} in instructions")


if __name__ == "__main__":
    if "--headline" in sys.argv:                                     # the headline launch alone, cold and warm
        run(4096, 4096, 16, torch.bfloat16, cfg=(2, 4, 4))
        run(4096, 4096, 16, torch.bfloat16, warm=True, cfg=(2, 4, 4))
        sys.exit(0)
    run(4096, 4096, 16, torch.bfloat16, cfg=(2, 4, 4))               # dq_h_kernel 4 x 4: x through LDS-DMA slabs
    run(4096, 4096, 16, torch.bfloat16, warm=True, cfg=(2, 4, 4))
    run(4096, 4096, 16, torch.bfloat16, cfg=(2, 44, 4))              # dq_hr_kernel: x straight into registers (round 6)
    run(4096, 4096, 16, torch.bfloat16, warm=True, cfg=(2, 44, 4))
    run(8192, 2048, 16, torch.bfloat16)
    run(8192, 2048, 16, torch.bfloat16, warm=True)
