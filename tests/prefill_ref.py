"""References for the prompt-side attention (quipamd_prefill_attention, csrc/prefill_attn.hip), shared by tests/test_prefill_host.py and
the -m gpu prefill tests.  A plain module: no fixtures, no pytest settings; everything runs on whatever device its inputs live on.

  gate(dtype)            the attention gate of test_gpu_decode_attn.py / test_gpu_decode_gqa.py: the output rounding of the 16-bit type
  tables(hd, rows)       HF rotary tables (decode.rotary_tables)
  rope(x, cos, sin, ..)  the fp32 expression of rope_kernel, rounded to x's dtype -- what quipamd_rope_inplace leaves, bit for bit
  causal_fp64(...)       fp64 causal attention over HF's repeat_kv, for T new positions behind `start` cached ones
  kernel_model(...)      the kernel's arithmetic restated in torch: fp32 scores, online softmax over 64-position tiles aligned to absolute
                         positions, P rounded to the 16-bit type for the P V product only, fp32 accumulation, output rounded
"""
import math

import torch

TILE = 64


def gate(dtype):
    return 2e-3 if dtype == torch.float16 else 1.6e-2


def within_gate(got, want, dtype):
    """(passes, error as a fraction of the gate)"""
    lim = gate(dtype) * max(1.0, want.abs().max().item())
    err = (got.double() - want.double()).abs().max().item()
    return err <= lim, err / lim


def tables(hd, rows):
    from quip_amd import decode
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    return decode.rotary_tables(inv, rows)


def rope(x, cos, sin, start, T, nheads):
    """x [bs*T, nheads*hd] (row b*T + t at position start + t) -> rotated, in x's dtype: a*c - b*s | b*c + a*s in fp32, each product and
    sum rounded once (the library is built without fused multiply-add contraction), then one rounding to the dtype"""
    hd = cos.shape[1]
    half = hd // 2
    rows = x.shape[0]
    xf = x.float().view(rows // T, T, nheads, hd)
    c = cos[start:start + T, :half].to(x.device).view(1, T, 1, half)
    s = sin[start:start + T, :half].to(x.device).view(1, T, 1, half)
    a, b = xf[..., :half], xf[..., half:]
    out = torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    return out.to(x.dtype).view(rows, nheads * hd)


def causal_fp64(q, kc, vc, start, T, g, scale=None):
    """q [bs*T, heads*hd] (already rotated), kc / vc [bs, kv, maxlen, hd] holding positions 0 .. start + T - 1; fp64 [bs*T, heads*hd]"""
    bs, kv, _, hd = kc.shape
    n = start + T
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    K = kc[:, :, :n].double().repeat_interleave(g, dim=1)                  # HF repeat_kv: query head j reads kv head j // g
    V = vc[:, :, :n].double().repeat_interleave(g, dim=1)
    Q = q.double().view(bs, T, kv * g, hd).transpose(1, 2)                 # [bs, heads, T, hd]
    out = torch.empty(bs, kv * g, T, hd, dtype=torch.float64, device=q.device)
    step = 512                                                              # rows of scores at a time: [bs, heads, step, n] in fp64
    kpos = torch.arange(n, device=q.device)
    for lo in range(0, T, step):
        hi = min(T, lo + step)
        s = torch.matmul(Q[:, :, lo:hi], K.transpose(2, 3)) * scale
        qpos = start + torch.arange(lo, hi, device=q.device)
        s = s.masked_fill(kpos[None, :] > qpos[:, None], float("-inf"))
        out[:, :, lo:hi] = torch.matmul(torch.softmax(s, -1), V)
    return out.transpose(1, 2).reshape(bs * T, kv * g * hd)


def kernel_model(q, kc, vc, start, T, g, scale=None):
    """the arithmetic of pf_attn_kernel in torch (not its reduction order inside a product): per query row, tiles [64 c, 64 c + 64) of the
    cache up to the row's own position; fp32 scores * scale, running max / sum in fp32, P rounded to q's dtype as the operand of P V,
    fp32 accumulator rescaled by exp(m_old - m_new), output / sum rounded to q's dtype"""
    bs, kv, _, hd = kc.shape
    dt = q.dtype
    n = start + T
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    K = kc[:, :, :n].float().repeat_interleave(g, dim=1)
    V = vc[:, :, :n].float().repeat_interleave(g, dim=1)
    Q = q.float().view(bs, T, kv * g, hd).transpose(1, 2)
    qpos = start + torch.arange(T, device=q.device)
    m = torch.full((bs, kv * g, T), float("-inf"), device=q.device)
    l = torch.zeros(bs, kv * g, T, device=q.device)
    acc = torch.zeros(bs, kv * g, T, hd, device=q.device)
    for c in range((n + TILE - 1) // TILE):
        lo, hi = c * TILE, min(n, c * TILE + TILE)
        kp = torch.arange(lo, hi, device=q.device)
        s = torch.matmul(Q, K[:, :, lo:hi].transpose(2, 3)) * scale
        s = s.masked_fill(kp[None, :] > qpos[:, None], float("-inf"))
        mn = torch.maximum(m, s.max(-1).values)                            # finite from tile 0 on: position 0 is below every row
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + torch.matmul(p.to(dt).float(), V[:, :, lo:hi])
        m = mn
    out = (acc / l[..., None]).to(dt)
    return out.transpose(1, 2).reshape(bs * T, kv * g * hd)


def append_want(k, v, kc, vc, start, T, cos=None, sin=None):
    """the caches after the append: rows start .. start + T - 1 hold k (rotated when tables are given) and v, nothing else changes"""
    bs, kv, _, hd = kc.shape
    kc, vc = kc.clone(), vc.clone()
    kr = k if cos is None else rope(k, cos, sin, start, T, kv)
    kc[:, :, start:start + T] = kr.reshape(bs, T, kv, hd).transpose(1, 2)
    vc[:, :, start:start + T] = v.reshape(bs, T, kv, hd).transpose(1, 2)
    return kc, vc
